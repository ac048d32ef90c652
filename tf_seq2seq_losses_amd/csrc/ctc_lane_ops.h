// Lane and LDS primitives of the fused tiers -- the log-domain roles (ctc_fused5_roles.h), the linear-domain loss + gradient
// (ctc_fused6.hip) and the linear-domain Hessian-vector product (ctc_hvp_fused.hip): the block barrier, the integer lane moves and
// exponent helpers, the one-instruction DPP inflow, a lane's slots of an LDS / HBM row, the block geometry and the phase-1 split.
// One copy: every function here is __forceinline__ or constexpr.  Included through ctc_fused_common.h.
#pragma once
#include "ctc_common.h"

namespace ctc {
namespace fused {

// The ONE raw barrier per block of every role (no __syncthreads: that would also drain the loads and stores in flight).
__device__ __forceinline__ void block_barrier() {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's LDS writes have landed; vmcnt untouched
  __builtin_amdgcn_s_barrier();
}

// integer twins of from_prev_lane / from_next_lane (ctc_common.h): the per-lane exponents of the linear-domain chains
__device__ __forceinline__ int from_prev_lane_i(int x, int fill) { return __builtin_amdgcn_update_dpp(fill, x, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int from_next_lane_i(int x, int fill) { return __builtin_amdgcn_update_dpp(fill, x, 0x130, 0xf, 0xf, false); }
__device__ __forceinline__ float ldexp_f(float x, int e) { return __builtin_ldexpf(x, e); }
__device__ __forceinline__ int frexp_e(float x) { return __builtin_amdgcn_frexp_expf(x); }
__device__ __forceinline__ int readlane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
// Packed float32 pairs (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: two label positions per instruction; a wavefront issues one
// vector instruction per ~8 cycles whatever its width, profiles/r03_issue_rate.txt) for the two-positions-per-lane classic chains --
// the roles whose time is their own dependent instruction stream.  NOT for the helpers: their E / G stage arithmetic packed the same
// way (r04: 263 -> 238 instructions per block) made phase 1 two microseconds SLOWER and phase 2 no faster -- a packed operation
// occupies the SIMD for two passes, and the helpers share their SIMDs' pipes with the chains (profiles/r04_kernel_experiments.md).
typedef float f2v __attribute__((ext_vector_type(2)));
// acc += (x of the upstream neighbour lane) * sc in ONE instruction (v_fmac_f32 with a DPP source; was v_mov_b32_dpp + v_ldexp_f32 +
// v_add_f32).  The lane without an upstream neighbour (0 for wave_shr, 63 for wave_shl) is left unchanged (bound_ctrl off: the
// lane is disabled).  `s_nop 1`: a DPP source written by the preceding VALU instruction needs two wait states, and the compiler
// does not look into inline assembly.
template <int DIR>
__device__ __forceinline__ void fmac_from_upstream(float &acc, float x, float sc) {
  if constexpr (DIR == 0) asm("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(sc));
  else asm("s_nop 1\n\tv_fmac_f32_dpp %0, %1, %2 wave_shl:1 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(sc));
}

// NL consecutive floats (or NL consecutive (a, b) pairs) of this lane in an LDS / HBM row, NL = 1, 2, 4, 8 (ld_slots / st_slots: any
// multiple of 4; ctc_nbest.hip reads 16): widest accesses
template <int NL>
__device__ __forceinline__ void ld_slots(const float *p, float (&v)[NL]) {
  if constexpr (NL == 1) v[0] = p[0];
  else if constexpr (NL == 2) { const float2 t = *reinterpret_cast<const float2 *>(p); v[0] = t.x; v[1] = t.y; }
  else {
#pragma unroll
    for (int q = 0; q < NL / 4; ++q) {
      const float4 t = *reinterpret_cast<const float4 *>(p + 4 * q);
      v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
    }
  }
}
template <int NL>
__device__ __forceinline__ void st_slots(float *p, const float (&v)[NL]) {
  if constexpr (NL == 1) p[0] = v[0];
  else if constexpr (NL == 2) *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
  else {
#pragma unroll
    for (int q = 0; q < NL / 4; ++q) *reinterpret_cast<float4 *>(p + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
  }
}
template <int NL>
__device__ __forceinline__ void ld_pairs(const float *p, float (&a)[NL], float (&b)[NL]) {
  if constexpr (NL == 1) { const float2 t = *reinterpret_cast<const float2 *>(p); a[0] = t.x; b[0] = t.y; }
  else {
#pragma unroll
    for (int q = 0; q < NL / 2; ++q) {
      const float4 t = *reinterpret_cast<const float4 *>(p + 4 * q);
      a[2 * q] = t.x; b[2 * q] = t.y; a[2 * q + 1] = t.z; b[2 * q + 1] = t.w;
    }
  }
}
template <int NL>
__device__ __forceinline__ void st_pairs(float *p, const float (&a)[NL], const float (&b)[NL]) {
  if constexpr (NL == 1) *reinterpret_cast<float2 *>(p) = make_float2(a[0], b[0]);
  else {
#pragma unroll
    for (int q = 0; q < NL / 2; ++q) *reinterpret_cast<float4 *>(p + 4 * q) = make_float4(a[2 * q], b[2 * q], a[2 * q + 1], b[2 * q + 1]);
  }
}

// Block geometry shared by every wavefront of the workgroup: G blocks of BLK frames, side A takes the first tmb of them in phase 1.
template <int BLK>
struct Geo {
  int len, G, tmb, tm, NB;
  __device__ __forceinline__ void init(int len_) {
    len = len_;
    G = (len + BLK - 1) / BLK;
    tmb = G / 2;
    tm = tmb * BLK;
    NB = G - tmb;  // >= tmb: blocks per side and phase, as iteration bound
  }
  __device__ __forceinline__ int nvof(int g) const { int r = len - BLK * g; return r < BLK ? r : BLK; }
  // side-local block j of (phase, side) -> absolute block; count of blocks
  __device__ __forceinline__ int nblocks(int phase, int side) const { return (phase == 1) == (side == 0) ? tmb : G - tmb; }
  __device__ __forceinline__ int absblock(int phase, int side, int j) const {
    if (phase == 1) return side == 0 ? j : G - 1 - j;
    return side == 0 ? tmb + j : tmb - 1 - j;
  }
  // frame processed at position d of block g by `side` (A ascending, B descending)
  __device__ __forceinline__ int frame(int side, int g, int d) const { return side == 0 ? BLK * g + d : BLK * g + nvof(g) - 1 - d; }
  // checkpoint slot of lattice time t (multiples of BLK, and `len`): distinct per direction (the linear-domain tiers)
  __device__ __forceinline__ int slot(int t) const { return (t + BLK - 1) / BLK; }
};

// Frames of a BLK-frame block per E-stage worker of a side in phase 1; worker 0 .. NH-1 = the helpers, NH = the recompute wavefront.
// NH = 4 (12-frame blocks): X4 / X4 / Y4 / Y4 for the helpers -- each tier's own measured choice -- and the rest for the recompute
// wavefront.  NH = 2 (6-frame blocks of the 4-positions-per-lane variant): the two helpers and the recompute wavefront take a third
// each.  NH = 1 (3-frame blocks of the 8-positions-per-lane variant): two frames for the helper, one for the recompute wavefront.
template <int BLK, int NH, int X4, int Y4>
struct P1Split {
  static constexpr int X = NH == 4 ? X4 : NH == 2 ? BLK / 3 : 2, Y = NH == 4 ? Y4 : NH == 2 ? BLK / 3 : 0;
  static constexpr int R = NH == 4 ? BLK - 2 * X - 2 * Y : NH == 2 ? BLK - X - Y : BLK - X;
  static_assert(NH == 4 || NH == 2 || NH == 1, "helpers per side");
  static_assert(X >= 0 && Y >= 0 && R >= 0 && X <= 6 && Y <= 6 && R <= 6, "phase-1 split: at most 6 frames per worker");
  static constexpr int count(int worker) {
    if (NH == 4) return worker < 2 ? X : worker < 4 ? Y : R;
    if (NH == 1) return worker == 0 ? X : R;
    return worker == 0 ? X : worker == 1 ? Y : R;
  }
  static constexpr int first(int worker) {
    int f = 0;
    for (int w = 0; w < worker; ++w) f += count(w);
    return f;
  }
};

}  // namespace fused
}  // namespace ctc
