// The linear-domain lattice chain shared by the loss + gradient kernel (ctc_fused6.hip) and the Hessian-vector kernel
// (ctc_hvp_fused.hip): the state of one direction (float32 mantissas, one integer exponent per lane), its start, its
// RENORMALISATION POLICY, the block cadence of the renormalisations and the exponent group of an R row.  One copy: until r04 each
// kernel carried its own, and every defect found in one had to be carried to the other by hand.  Each kernel derives its Chain from
// ChainCore and adds its own step() (values only / values and tangents side by side).  Everything here is __forceinline__ or constexpr.
#pragma once
#include "ctc_lane_ops.h"
#include "ctc_linear_flags.h"

namespace ctc {
namespace fused {

using namespace ctc::linear;  // the number format's constants and the flag bits

// renormalisation period inside a block and the number of lanes the lattice front can cross in one period
template <int BLK, int NL>
struct Cad {
  // 12-frame blocks: two label positions per lane renormalise every 6 frames (r03: with the posterior scale in two factors the
  // longer period no longer raises D5 on long utterances; -4 us at the north-star shape), one position per lane every 4
  static constexpr int RN12 = 6;  // other periods were measured as build variants, profiles/r04_kernel_experiments.md
  static constexpr int RN = (BLK % 4 == 0) ? (NL == 2 ? RN12 : 4) : 3;
  static constexpr int NG = BLK / RN;            // exponent groups of the rows of one block
  static constexpr int LV = (RN + NL - 1) / NL;  // adoption levels: lanes the lattice front can cross in one period
  static constexpr int NSEG = 2 * NG + 1;        // posterior-scale segments of one block (fused6: kl_segment)
  static_assert(BLK % RN == 0, "block length must be a multiple of the renormalisation period");
};

// exponent group of the R row at position d of a block with nv frames: rows are written BEFORE the recompute chain renormalises,
// s steps after its checkpoint -> group max(s-1, 0) / RN.  s = nv-1-d (A, simplified B) / nv-d (classic B).
// (The reference arguments and the `grp` lambda around the call in ctc_fused6.hip keep fused6's device code: profiles/linear_chain_core.md.)
template <int KIND, int DIR, int RN>
__device__ __forceinline__ constexpr int r_group(const int &d, const int &nv) {
  const int s = (KIND == 0 && DIR == 1) ? nv - d : nv - 1 - d;
  return (s > 0 ? s - 1 : 0) / RN;
}

// Gap to which a lane that HOLDS mass is lifted towards its upstream neighbour.  It has to be the adoption gap: r04 tried 80 (a live
// lane's own thin values then survive 2^64 deeper -- tests/tools/linear_model.py shows the mass of tests/golden/soak_case_endloss_u128.npz
// intact with it), but mantissas then reach 2^120 where a steep front crosses thin live lanes, the posterior PRODUCTS of phase 2
// overflow, and between the frames D6 samples that went unnoticed: a gradient 3.0 off, unflagged (tests/tools/flag_stats.py, cell
// sigma 5, V = 3, U = 32, slack 2).  With 16 per level and LV levels a mantissa stays below 2^55 and a product below 2^110.
constexpr int GAP_LIVE = 16;

// ------------------------------------------------------------------------------------------------
// The lattice state of one direction: mantissas + one exponent per lane.  Slot i = lane*NL + j is label position i.
//   classic    A (DIR 0): c[j] = closed(l=i+1), o[j] = open(l=i+1), cx = closed(l=0)
//              B (DIR 1): c[j] = closed(l=i),   o[j] = open(l=i+1), cx = closed(l=UP)
//   simplified A: c[j] = a(l=i+1), cx = a(l=0);   B: c[j] = b(l=i), cx = b(l=UP)
// true value = mantissa * 2^k (lanes) / 2^kx (cx).  dk = (exponent of the upstream neighbour) - k: what the one value a
// lane receives per step has to be shifted by (upstream = previous lane for A, next lane for B; cx for the first / last).
// ------------------------------------------------------------------------------------------------
// The mantissas are the first members of the chain, in a struct of their own so that a chain with more per slot can say where its
// extras sit among them (the Hessian-vector kernel: a tangent beside every value).  Any such struct has c[NL], o[NL], cx.
template <int NL>
struct Mantissas {
  float c[NL], o[NL], cx;
};
template <int KIND, int NL, int DIR, class M = Mantissas<NL>>
struct ChainCore : M {
  using M::c; using M::o; using M::cx;
  static constexpr int SLOT_CX = NL;  // renorm's hook: the "slot" of the boundary value cx
  int k, kx, dk;
  bool norep[NL], norep_next[NL];
  int flag;
  static constexpr bool PACKED = KIND == 0 && NL == 2;
  float nrf[NL];  // PACKED: 1.0 where the repeat rule lets the diagonal pass (norep_next for A, norep for B), else 0.0
  float sc, scb;  // PACKED: 2^dk as a float (0 below 2^-126: what v_ldexp_f32 would flush), and the same on the boundary lane only
  bool boundary = false;
  bool alive = false;  // the lane had mass at its last renormalisation
  int age = 0;         // consecutive renormalisations with mass
  bool relevant = true;

  __device__ __forceinline__ void init_labels(const Problem &p, int b, int lane, int ll) {
    const int32_t *lab = label_row(p, b);
    const LabelTok tok{ll, p, lab};
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int i = lane * NL + j;
      const int tk = tok(i);
      norep[j] = (i == 0) || tk != tok(i - 1);
      norep_next[j] = tok(i + 1) != tk;
      nrf[j] = ((DIR == 0) ? norep_next[j] : norep[j]) ? 1.f : 0.f;
      c[j] = 0.f;
      o[j] = 0.f;
    }
    cx = 0.f; k = DEAD; kx = DEAD; dk = 0; flag = 0; sc = 1.f;
    scb = (lane == (DIR == 0 ? 0 : 63)) ? 1.f : 0.f;
    boundary = lane == (DIR == 0 ? 0 : 63);
    relevant = lane * NL <= ll;  // the lane holds a label position that can carry mass (lanes beyond the label stay empty for good)
  }

  // starting state: alpha[0] = delta(closed(l=0)) / beta[len] = delta(closed(l=ll)) + delta(open(l=ll))
  // (a chain that carries tangents has them all zero here: nothing of theirs to shift)
  template <int LV>
  __device__ __forceinline__ void start(int lane, int ll, int UP) {
    if constexpr (DIR == 0) {
      cx = 1.f; kx = 0;
    } else {
      if (ll == UP) { cx = 1.f; kx = 0; }
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const int i = lane * NL + j;
        if (i == ll) { c[j] = 1.f; k = 0; }
        if (KIND == 0 && i == ll - 1) { o[j] = 1.f; k = 0; }
      }
    }
    renorm<LV>();
    flag = 0;
  }

  // per-lane renormalisation: k <- exponent of the lane maximum (lanes without mass adopt the upstream exponent - GAP so
  // that what flows in during the next period is representable), cx to its own exponent, dk refreshed.  Decided by the VALUES
  // alone; whatever rides on them (the tangents of the Hessian-vector kernel) follows through `also(slot, shift)`, called right
  // after the values of a slot have been shifted: slot j < NL = the lane's mantissas of position j, SLOT_CX = cx.
  template <int LV, class Also>
  __device__ __forceinline__ void renorm(Also &&also) {
    float m = c[0];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      if constexpr (KIND == 0) m = (j == 0) ? vmax_raw(m, o[0]) : vmax3_raw(m, c[j], o[j]);
      else if (j > 0) m = vmax_raw(m, c[j]);
    }
    const bool live = m > 0.f;
    const int fe = frexp_e(m);
    const int e_own = live ? fe + k : DEAD;
    const bool xlive = cx > 0.f;
    const int ex = xlive ? frexp_e(cx) + kx : DEAD;
    int kn = e_own;
    // the first level: a lane far below its upstream neighbour is lifted to that neighbour's exponent - GAP (a lane that holds mass:
    // - GAP_LIVE at least); lanes without mass get an exponent this way before the front reaches them
    {
      const int nb = (DIR == 0) ? from_prev_lane_i(kn, ex) : from_next_lane_i(kn, ex);
      kn = imax(kn, nb - (live ? imax(GAP_LIVE, LV == 1 ? GAP_WIDE : GAP) : (LV == 1 ? GAP_WIDE : GAP)));
    }
    // ALL levels for every lane, with or without mass (until r04 the further levels ran only while some lane of the wavefront was
    // empty): a STEEP profile of live lanes -- each 2^-100 below its upstream neighbour: sharp logits -- kept, after the one level,
    // exponents 2^100 apart two lanes down (each lane had been lifted against its neighbour's exponent BEFORE that neighbour's own
    // lift), and when the bulk crossed two lanes within a period the inflow arrived scaled by 2^100: mantissas of 2^60 .. 2^127,
    // inf at the meeting point (D1).  19 of 256 N(0, 3^2) utterances at the north-star shape were in that state at the meeting
    // point and 4 overflowed (tests/tools/linear_model.py); with every level applied dk <= GAP holds for every lane.
    {
#pragma unroll
      for (int lv = 1; lv < LV; ++lv) {
        const int nb = (DIR == 0) ? from_prev_lane_i(kn, ex) : from_next_lane_i(kn, ex);
        kn = imax(kn, nb - GAP);
      }
    }
    kn = imax(kn, DEAD);
    const int d = k - kn;
    // D3: own live values crushed by a much larger inflow scale; D4: decayed by more than 2^-DECAY_MAX, or live -> zero
    // (D3 only for a lane that has had mass for a few periods: at the lattice front the first thin paths of a lane are
    // legitimately swamped when the bulk arrives, ~1 in 256 benign utterances)
    age = (live && alive) ? age + 1 : 0;
    flag |= (live && age >= 3 && d < -DOWN_MAX ? D3_DOWN : 0) | (live && fe < -DECAY_MAX ? D4_DECAY : 0) | (!live && alive ? D4_DIED : 0);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      c[j] = ldexp_f(c[j], d);
      if constexpr (KIND == 0) o[j] = ldexp_f(o[j], d);
      also(j, d);
    }
    k = kn;
    cx = ldexp_f(cx, kx - ex);
    also(SLOT_CX, kx - ex);
    kx = ex;
    dk = ((DIR == 0) ? from_prev_lane_i(k, kx) : from_next_lane_i(k, kx)) - k;
    set_scale();
    alive = live;
  }
  template <int LV>
  __device__ __forceinline__ void renorm() {
    renorm<LV>([](int, int) {});
  }
  // dk as the factor the packed step multiplies by (after every change of dk)
  __device__ __forceinline__ void set_scale() {
    if constexpr (PACKED) {
      sc = (dk < -126) ? 0.f : ldexp_f(1.f, imin(dk, 127));
      scb = boundary ? sc : 0.f;
    }
  }
  // after c, o, cx, k, kx have been set from a checkpoint row: what a renormalisation would have left beside them
  __device__ __forceinline__ void restored() {
    dk = ((DIR == 0) ? from_prev_lane_i(k, kx) : from_next_lane_i(k, kx)) - k;
    set_scale();
    float m = 0.f;
#pragma unroll
    for (int j = 0; j < NL; ++j) m = fmaxf(m, fmaxf(c[j], o[j]));
    alive = m > 0.f;  // (a lane that only adopted its neighbour's exponent has no mass yet)
  }
  // number of label positions 1 .. ll-1 that repeat their predecessor (classic: each costs one more frame); wave-uniform
  __device__ __forceinline__ int repeats(int ll, int lane) const {
    int n = 0;
#pragma unroll
    for (int j = 0; j < NL; ++j) n += __builtin_popcountll(__builtin_amdgcn_ballot_w64(!norep[j] && lane * NL + j < ll));
    return n;
  }
  // OR of the lanes' flags D3_DOWN .. D4_DIED (wave-uniform)
  __device__ __forceinline__ int flag_or() const {
    int f = 0;
#pragma unroll
    for (int bit = D3_DOWN; bit <= D4_DIED; bit <<= 1) f |= (__builtin_amdgcn_ballot_w64((flag & bit) != 0) != 0) ? bit : 0;
    return f;
  }
};

}  // namespace fused
}  // namespace ctc
