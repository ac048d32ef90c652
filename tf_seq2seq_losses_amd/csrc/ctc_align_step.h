// What the best-path units share (ctc_align.hip: one workgroup per utterance; ctc_align_long.hip: one workgroup per tile of the
// lattice): the workgroup's roles and ring, the back-pointer word, one frame of the chain, and the producers' gather and row
// statistics of a group of frames.  Device code only; every function is inlined into its caller's loop.
//
// States.  Classic: O[i] = the last frame emitted label i (open), C[i] = labels 0..i are done and the last frame was blank
// (closed).  Simplified: S[i] = labels 0..i are emitted (kept in C; O unused).
//   O'[i] = max(O[i], C[i-1], O[i-1] if label[i] != label[i-1]) + x[label[i]]      2 bits: 0, 1, 2
//   C'[i] = max(C[i], O[i]) + x[blank]                                            1 bit
//   S'[i] = max(S[i] + x[blank], S[i-1] + x[label[i]])                            1 bit (1 = the frame emits label i)
// Ties keep the first candidate in the order written (strict comparisons): deterministic.
#pragma once
#include <type_traits>

#include "ctc_common.h"

namespace ctc {

constexpr int ALIGN_PW = 4;                         // producer wavefronts
constexpr int ALIGN_THREADS = 64 * (1 + ALIGN_PW);  // + the chain
constexpr int ALIGN_RING = 4096;                    // label emissions per ring buffer (two buffers): frames per block = 4096 / UP

// back-pointer word of one lane and frame: 3 bits per label position (classic; simplified uses 1), NL positions
template <int NL> struct BpWord { typedef unsigned char type; };
template <> struct BpWord<4> { typedef unsigned short type; };
template <> struct BpWord<8> { typedef unsigned int type; };
template <> struct BpWord<16> { typedef unsigned long long type; };
// ... and the register the chain collects it in
template <int NL> struct BpBits { typedef typename std::conditional<NL == 16, unsigned long long, unsigned int>::type type; };

constexpr int bp_word_bytes(int NL) { return NL <= 2 ? 1 : NL / 2; }

// elements k .. k+3 of a row of element type dt (0 = float32, 1 = bfloat16, 2 = float16) as float32 (row_load1: ctc_common.h)
__device__ __forceinline__ float4 row_load4(const char *row, int k, int dt) {
  if (dt == 0) return *reinterpret_cast<const float4 *>(row + (size_t)k * 4);
  const uint2 u = *reinterpret_cast<const uint2 *>(row + (size_t)k * 2);
  return make_float4(h16_to_f32((unsigned short)(u.x & 0xffffu), dt), h16_to_f32((unsigned short)(u.x >> 16), dt),
                     h16_to_f32((unsigned short)(u.y & 0xffffu), dt), h16_to_f32((unsigned short)(u.y >> 16), dt));
}

// running (max, sum of exp(x - max)) of one lane: one more element
__device__ __forceinline__ void stat_add(float &m, float &s, float x) {
  const float mn = fmaxf(m, x);
  s = s * fexp2((m - mn) * LOG2E) + fexp2((x - mn) * LOG2E);
  m = mn;
}
__device__ __forceinline__ void stat_add4(float &m, float &s, const float4 v) {
  const float mn = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
  s = s * fexp2((m - mn) * LOG2E) +
      ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
  m = mn;
}

// One frame of the chain for the NL positions of this lane.  fillO / fillC: what lane 0 takes for the position before its first --
// the state of that position BEFORE this frame (whole utterance: -inf and the start state; a tile further right: its left
// neighbour's last position).  Returns the lane's back-pointer bits.
template <int KIND, int NL>
__device__ __forceinline__ typename BpBits<NL>::type align_chain_step(double (&O)[NL], double (&C)[NL], unsigned allow, double fillO,
                                                                      double fillC, const float (&e)[NL], double ebd) {
  typedef typename BpBits<NL>::type Bits;
  const double NINF = -__builtin_inf();
  Bits bits = 0;
  if (KIND == 0) {
    const double pO = from_prev_lane(O[NL - 1], fillO);
    const double pC = from_prev_lane(C[NL - 1], fillC);
#pragma unroll
    for (int j = NL - 1; j >= 0; --j) {
      const double qO = j > 0 ? O[j > 0 ? j - 1 : 0] : pO;
      const double qC = j > 0 ? C[j > 0 ? j - 1 : 0] : pC;
      const double a2 = ((allow >> j) & 1u) ? qO : NINF;
      double best = O[j];
      unsigned src = 0;
      if (qC > best) { best = qC; src = 1; }
      if (a2 > best) { best = a2; src = 2; }
      const unsigned sc = O[j] > C[j] ? 1u : 0u;
      const double bc = sc ? O[j] : C[j];
      O[j] = best + (double)e[j];
      C[j] = bc + ebd;
      bits |= (Bits)(src | (sc << 2)) << (3 * j);
    }
  } else {
    const double pS = from_prev_lane(C[NL - 1], fillC);
#pragma unroll
    for (int j = NL - 1; j >= 0; --j) {
      const double q = j > 0 ? C[j > 0 ? j - 1 : 0] : pS;
      const double d = q + (double)e[j], h = C[j] + ebd;
      const unsigned sd = d > h ? 1u : 0u;
      C[j] = sd ? d : h;
      bits |= (Bits)sd << j;
    }
  }
  return bits;
}

// Producers, G frames t .. t + G - 1 of one utterance (those at or beyond Tb are read as frame Tb - 1 and dropped): gathers
// x[t, label] of this lane's NL positions (lab < 0: no emission, -inf) and x[t, blank] into the ring rows r, r + RS, ... (blank at
// [UP]); with `stats`, adds the frames' log-sum-exp (float32 row statistics, one V-wide pass) to lse.
template <int NL, int G>
__device__ __forceinline__ void align_produce(const Problem &p, const char *xb, int esz, bool vec, const int (&lab)[NL], int t, int Tb,
                                              float *r, int lane, bool stats, double &lse) {
  constexpr int UP = 64 * NL, RS = UP + 4;
  const int V = p.V, blank = p.blank, dt = p.xdtype;
  const char *row[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int tt = t + g < Tb ? t + g : Tb - 1;  // (past the end: a valid row, its results are dropped)
    row[g] = xb + (size_t)((long)tt * p.xst) * esz;
  }
  float e[G][NL], eb[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const float v = row_load1(row[g], lab[j] >= 0 ? lab[j] : blank, dt);
      e[g][j] = lab[j] >= 0 ? v : -__builtin_inff();
    }
    eb[g] = row_load1(row[g], blank, dt);
  }
  if (stats) {
    float m[G], s[G];
#pragma unroll
    for (int g = 0; g < G; ++g) { m[g] = -3.402823466e38f; s[g] = 0.f; }
    if (vec) {
      for (int k = lane * 4; k < V; k += 256) {
        float4 v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = row_load4(row[g], k, dt);
#pragma unroll
        for (int g = 0; g < G; ++g) stat_add4(m[g], s[g], v[g]);
      }
    } else {
      for (int k = lane; k < V; k += 64) {
        float v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = row_load1(row[g], k, dt);
#pragma unroll
        for (int g = 0; g < G; ++g) stat_add(m[g], s[g], v[g]);
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float M = wave_max(m[g]);
      const float S = wave_sum(s[g] * fexp2((m[g] - M) * LOG2E));
      if (t + g < Tb) lse += (double)M + (double)flog2(S) * LN2_D;
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (t + g < Tb) {
      float *const rg = r + g * RS;
#pragma unroll
      for (int j = 0; j < NL; ++j) rg[lane * NL + j] = e[g][j];
      if (lane == 0) rg[UP] = eb[g];
    }
  }
}

}  // namespace ctc
