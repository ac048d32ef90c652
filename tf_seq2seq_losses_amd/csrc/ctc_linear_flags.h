// Constants of the linear-domain number format (float32 mantissas, one integer exponent per lane) and the flags D1..D10 that say
// when an utterance leaves it -- shared by the loss + gradient kernel (ctc_fused6.hip) and the Hessian-vector kernel
// (ctc_hvp_fused.hip), which until r04 each carried a hand-kept copy (the copies had drifted -- the HVP's mass check still
// used 1e-4 after fused6 had tightened it to 3e-5).  The list of conditions is at the top of ctc_fused6.hip.
#pragma once

namespace ctc {
namespace linear {

constexpr int DEAD = -(1 << 24);  // exponent of a lane whose mantissas are all zero
constexpr int GAP = 16;           // a lane adopts / is lifted to its upstream neighbour's exponent minus GAP, per adoption level
// ... when ONE level suffices (a lane of 4 or 8 label positions is never crossed within a period): neighbouring lanes then differ by
// 2^100 and more on benign inputs, and lifting a lane to 2^-16 of its neighbour pushed its own values towards the float32 underflow (D4)
constexpr int GAP_WIDE = 64;
// D3 / D4: a lane's own values pushed 2^-96 below its exponent (by a larger inflow scale / by decay).  A float32 mantissa
// holds them down to 2^-126, so nothing is lost yet; the margin is for what happens before the next renormalisation.  (64
// was too tight once a lane spans eight label positions: neighbouring lanes then differ by more than 2^64 on benign inputs
// and every loss-only call at U > 256 went to the log domain.)
constexpr int DOWN_MAX = 96;      // D3: a renormalisation pushes a lane's own live values down by more than 2^-96
constexpr int DECAY_MAX = 96;     // D4: a lane's maximum decays by more than 2^-96 within one renormalisation period
// Posterior scale 2^KK_MAX at most in ONE factor.  The posterior of a state is (alpha mantissa)(beta mantissa) 2^(kA + kB - log2 P);
// the mantissa PRODUCT underflows below 2^-126, which is harmless while the scale stays below 2^90 (the lost term is < 2^-5 units of
// 2^-30) and fatal beyond -- sharp logits on a nearly forced alignment get there in the frames just before a renormalisation, and so do
// benign long utterances (T >= 3000: a lane whose two label positions differ by more than 2^90 in alpha and by as much the other way
// in beta while the alignment crosses between them).  Beyond KK_MAX fused6 applies the scale in TWO factors: the excess 2^(k - KK_MAX)
// goes onto the chain's own operand BEFORE the product (then nothing that matters underflows), the rest after it as before; a
// wave-uniform branch per frame, taken only while some lane of the wavefront needs it.  (The Hessian-vector kernel raises D5 at KK_MAX.)
constexpr int KK_MAX = 90;
constexpr int KK_MAX2 = 200;      // D5 (fused6): beyond this even the pre-scaled operand would leave float32
constexpr float EMIS_MIN = 7.52316384526264e-37f;  // D2: 2^-120 of the row maximum
// D7 (loss-only calls): a needed emission below 2^-16 of its row maximum -- "sharp" logits.  The r03 soak runs found utterances with
// logits N(0, 3^2) on nearly forced alignments (2..15 frames more than labels) whose linear-domain sweeps lose mass that matters later
// WITHOUT tripping D1..D5 (loss off by 1e-4 .. 3e-2 relative): a call with a gradient sees it in the posterior mass (D6) and redoes the
// utterance, a loss-only call has nothing to check against.  Every such case had a needed emission below 2^-18.9; N(0,1) logits stay
// above 2^-13 (the 4.5-sigma tail of 129 000 draws).  So a loss-only call hands sharp utterances to the log domain.
constexpr float EMIS_SOFT = 1.52587890625e-05f;
// D6: tolerated deviation of a frame's posterior mass from 1.  The gradient of an unflagged utterance is off by about as much, and the
// bar is 1e-4: with a tolerance of 1e-4 the soak runs measured up to 9.0e-5 on unflagged utterances -- no margin (r03).
constexpr float MASS_TOL = 3e-5f;

// The bits of an utterance's flag word (Lds::flag, flags[b] of the workspace; Python and the tests read them as numbers).
constexpr int D1_NO_P = 1;      // P == 0, inf or NaN at the meeting point
constexpr int D2_EMIS = 2;      // a needed emission below EMIS_MIN of its row maximum
constexpr int D3_DOWN = 4;      // a renormalisation pushed a lane's live values down by more than 2^-DOWN_MAX
constexpr int D4_DECAY = 8;     // a lane's maximum decayed by more than 2^-DECAY_MAX within one period ...
constexpr int D4_DIED = 16;     // ... or a live lane went to zero.  (D3_DOWN .. D4_DIED: the per-lane bits Chain::flag_or() collects)
constexpr int D5_SCALE = 32;    // a posterior scale beyond what the products can hold (KK_MAX2 in fused6, KK_MAX in the HVP)
constexpr int D6_MASS = 64;     // the posterior mass of a sampled frame is off by more than MASS_TOL
constexpr int D7_SHARP = 128;   // a needed emission below EMIS_SOFT of its row maximum
// D8 (a wait on the producer / consumer words that once replaced the phase-1 barrier timed out) and D9 (a checked renormalisation saw
// a value leave its lane's range -- flagged 60 % of benign utterances and still missed a harmful one, tests/tools/flag_stats.py) are
// retired, never set, and stay reserved: still in the masks of fused6's meeting point and in its flag_or() -- the same device code.
constexpr int D8_RETIRED = 256, D9_RETIRED = 512;
constexpr int D10_DWELL = 2048; // loss-only call with more frames per label position than fused6's DWELL_HARD
constexpr int HARD_FLAGS = D1_NO_P | D2_EMIS;                       // honoured by every call
constexpr int SOFT_FLAGS = D3_DOWN | D4_DECAY | D4_DIED | D7_SHARP; // heuristic signs: loss-only calls outside the trusted range

}  // namespace linear
}  // namespace ctc
