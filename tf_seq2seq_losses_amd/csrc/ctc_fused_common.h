// Building blocks shared by the fused loss+gradient kernels (ctc_fused5.hip / ctc_fused5_roles.h: log-domain chains + recompute
// chains + helpers; ctc_fused6.hip: the same roles in the linear domain) and by the Hessian kernels (ctc_hessian.hip: the sweeps;
// ctc_hvp.hip / ctc_hvp_device.h and ctc_hvp_fused.hip: the Hessian-vector products).  See those files for the algorithms.
// (ctc_lane_ops.h: lane and LDS primitives of the fused tiers; ctc_linear_flags.h and ctc_linear_chain.h: the number format, the
// chain state and the renormalisation policy of the two linear-domain kernels.)
#pragma once
#include <type_traits>

#include "ctc_common.h"
#include "ctc_dpp_batch.h"
#include "ctc_lane_ops.h"

namespace ctc {

namespace fused {

// Compile-time loop: f(std::integral_constant<int, I>) for I in [0, N).  Used instead of `#pragma unroll` where a
// register-resident array is indexed by the loop variable: the index is a constant already in the front end, so the
// array is scalarised even when the late loop unroller would run after SROA (otherwise it lands in scratch memory).
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

constexpr int PF = 16;   // logits rows of look-ahead (= unrolled block length = renormalisation period)
constexpr int PFS = 8;   // spilled lattice rows of look-ahead in phase 2 (keeps the kernel inside 256 VGPRs)
constexpr int NPACE = 48; // pacing stores after a ring prologue (see Side::pace)

// (wave64 DPP reductions wave_sum_dpp / wave_max_dpp: ctc_common.h)
__device__ __forceinline__ double readlane_f(double v, int l) {  // (float64 state of the log-domain roles: the two halves)
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ float readlane_f(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// One spilled lattice row as the other side reads it: per lane NL slots of (first[, second]) plus the 16-byte tail.
template <int KIND, int NL>
struct SRow {
  float a[NL];   // classic: closed part / simplified: the state
  float b[NL];   // classic: open part (unused for simplified)
  float4 tail;   // (state outside the slot range, -, off_hi, off_lo)
  float2 stat;   // (row max, log2 sum exp) of the frame the reader processes with this row
};

template <int KIND, int NL>
__device__ __forceinline__ void load_srow(SRow<KIND, NL> &r, const float *__restrict__ row, int lane, int UP) {
  if constexpr (KIND == 0) {
    ld_pairs<NL>(row + 2 * lane * NL, r.a, r.b);
    r.tail = *reinterpret_cast<const float4 *>(row + 2 * UP);
    r.stat = *reinterpret_cast<const float2 *>(row + 2 * UP + 4);
  } else {
    ld_slots<NL>(row + lane * NL, r.a);
    r.tail = *reinterpret_cast<const float4 *>(row + UP);
    r.stat = *reinterpret_cast<const float2 *>(row + UP + 4);
  }
}

template <int KIND, int NL>
__device__ __forceinline__ void store_srow(float *__restrict__ row, int lane, int UP, const float (&a)[NL],
                                           const float (&b)[NL], float4 tail, float2 stat) {
  if constexpr (KIND == 0) st_pairs<NL>(row + 2 * lane * NL, a, b);
  else st_slots<NL>(row + lane * NL, a);
  // 32-byte wave-uniform tail in ONE store instruction: even lanes write the first half, odd lanes the second
  const bool odd = lane & 1;
  *reinterpret_cast<float4 *>(row + (KIND == 0 ? 2 : 1) * UP + (odd ? 4 : 0)) =
      make_float4(odd ? stat.x : tail.x, odd ? stat.y : tail.y, odd ? 0.f : tail.z, odd ? 0.f : tail.w);
}

// Per-frame emissions in base-2 logs.
template <int NL>
struct Emis {
  float y[NL];
  float bl, mx, l2s;
};

// The whole per-side program.  DIR 0 = side A (alpha, forward), DIR 1 = side B (beta, backward).
// Slot i = lane*NL + j is label position i.  State convention (same as Scan in ctc_kernels.hip):
//   classic    A: c[j] = closed(l=i+1), o[j] = open(l=i+1), cx = closed(l=0)
//              B: c[j] = closed(l=i),   o[j] = open(l=i+1), cx = closed(l=UP)
//   simplified A: c[j] = a(l=i+1), cx = a(l=0);   B: c[j] = b(l=i), cx = b(l=UP)
// Rows are spilled in the layout the OTHER side's slots are aligned with:
//   A -> rows[t] : slot i = (state_c(l=i) [, open(l=i+1)]), tail.x = state_c(l=UP)       (read by B)
//   B -> rows[t] : slot i = (state_c(l=i+1) [, open(l=i+1)]), tail.x = state_c(l=0)      (read by A)
// XT: format of logits and gradient in HBM: 0 = contiguous float32 (frame stride V folded into the addressing),
// 1 = float32 with run-time frame strides, 2 = bfloat16 with run-time frame strides, 3 = float32, any vocabulary size
// and stride (rows not 16-byte aligned: element-wise loads and stores).  Arithmetic is float32 either way.
// ST: type of the lattice state.  float32 (the Hessian's scans); float64 in the log-domain roles of the fused tiers since r04 --
// rows in LDS and HBM stay float32 (one rounding where a state is written out, none accumulated along the sweep).
template <int KIND, int NL, int VPL, int DIR, bool LOGITS, int XT = 0, class ST = float>
struct Side {
  static constexpr int V = 256 * VPL;
  // lattice state
  ST c[NL], o[NL], cx;
  double off;
  bool norep[NL], norep_next[NL];
  int tokoff[NL];  // byte offset of label[i] inside the LDS copy of the logits row (pad slot for i >= label_length)
  float mb[4 * VPL];  // 1.0 at this lane's element that is the blank column, else 0
  // geometry
  int lane, UP, len, ll, blank;
  const float *xbase;   // logits of this utterance (XT = 1: really bfloat16)
  float *gbase;         // gradient of this utterance (XT = 1: really bfloat16)
  long xst = V, gst = V;  // element stride between frames (time-major producers: B*V)
  int Vr = V;             // XT != 0: actual vocabulary size <= V (multiple of 4); lanes beyond it read -inf, write nothing
  float *own_rows;      // spill rows this side writes
  const float *oth_rows;  // spill rows the other side writes
  int SRS;
  float *sink;  // global: 1 KB per wavefront, target of the pacing stores of the ring prologues
  float *xs;    // LDS: 2 x (V + 4) floats, gather copies of the logits row
  float *bins;  // LDS: V floats, posterior per token
  float dl;

  __device__ __forceinline__ int frame(int t0, int k) const { return DIR == 0 ? t0 + k : t0 - k; }

  // Pacing store.  hipcc derives the s_waitcnt vmcnt(N) of a software-pipelined loop from the LEAST number of memory
  // operations it can prove to lie between a prefetch and its use, and that minimum comes from the ring prologue where
  // the prefetches would be back to back.  Giving every prologue slot as many memory operations as a steady-state step
  // has makes the derived N as large as in the steady state, so a wait never reaches stores/loads of the last few steps.
  __device__ __forceinline__ void pace(int slot) const {
    volatile float *q = sink + lane * 4;  // volatile: identical stores to one address must not be merged away
    q[0] = (float)slot;
  }

  __device__ __forceinline__ void load_x(float4 (&xr)[VPL], int t) const {
    if constexpr (XT == 0) {
      const float *row = xbase + (long)t * V + lane * 4;
#pragma unroll
      for (int q = 0; q < VPL; ++q) xr[q] = *reinterpret_cast<const float4 *>(row + 256 * q);
    } else if constexpr (XT == 1) {
      const float *row = xbase + (long)t * xst + lane * 4;
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        xr[q] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);  // tokens beyond the vocabulary: log 0
        if (lane * 4 + 256 * q < Vr) xr[q] = *reinterpret_cast<const float4 *>(row + 256 * q);
      }
    } else if constexpr (XT == 3) {
      const float *row = xbase + (long)t * xst + lane * 4;
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        const int k = lane * 4 + 256 * q;
        xr[q] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (k < Vr) xr[q].x = row[256 * q];
        if (k + 1 < Vr) xr[q].y = row[256 * q + 1];
        if (k + 2 < Vr) xr[q].z = row[256 * q + 2];
        if (k + 3 < Vr) xr[q].w = row[256 * q + 3];
      }
    } else {  // 4 bfloat16 = 8 bytes per lane; widening is a shift / mask
      const unsigned short *row = reinterpret_cast<const unsigned short *>(xbase) + (long)t * xst + lane * 4;
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        uint2 w = make_uint2(0xff80ff80u, 0xff80ff80u);  // bfloat16 -inf
        if (lane * 4 + 256 * q < Vr) w = *reinterpret_cast<const uint2 *>(row + 256 * q);
        xr[q] = make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xffff0000u), __uint_as_float(w.y << 16),
                            __uint_as_float(w.y & 0xffff0000u));
      }
    }
  }
  // one gradient row segment (4 values of this lane) in the output element type.  Non-temporal stores: the gradient is
  // written once and never read here; keeping it out of L2 leaves the cache to the logits, checkpoints and statistics
  // (measured -4.5 % kernel time; non-temporal LOADS of the logits cost +5 %).
  __device__ __forceinline__ static void nt_store4(float *p, float4 r) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f v = {r.x, r.y, r.z, r.w};
    __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(p));
  }
  __device__ __forceinline__ void store_g(int t, int q, float4 r) const {
    if constexpr (XT == 0) {
      nt_store4(gbase + (long)t * V + lane * 4 + 256 * q, r);
    } else if constexpr (XT == 1) {
      if (lane * 4 + 256 * q < Vr) nt_store4(gbase + (long)t * gst + lane * 4 + 256 * q, r);
    } else if constexpr (XT == 3) {
      float *row = gbase + (long)t * gst + lane * 4 + 256 * q;
      const int k = lane * 4 + 256 * q;
      if (k < Vr) __builtin_nontemporal_store(r.x, row);
      if (k + 1 < Vr) __builtin_nontemporal_store(r.y, row + 1);
      if (k + 2 < Vr) __builtin_nontemporal_store(r.z, row + 2);
      if (k + 3 < Vr) __builtin_nontemporal_store(r.w, row + 3);
    } else {
      unsigned short *row = reinterpret_cast<unsigned short *>(gbase) + (long)t * gst + lane * 4 + 256 * q;
      typedef unsigned v2u __attribute__((ext_vector_type(2)));
      v2u w;
      w.x = f32x2_to_bf16x2(r.x, r.y);
      w.y = f32x2_to_bf16x2(r.z, r.w);
      if (lane * 4 + 256 * q < Vr) __builtin_nontemporal_store(w, reinterpret_cast<v2u *>(row));
    }
  }

  // log-softmax statistics (tools.py:27-40): row max and log2 sum exp by DPP reductions
  __device__ __forceinline__ void stats(const float4 (&xr)[VPL], float &mx, float &l2s) const {
    mx = 0.f; l2s = 0.f;
    if constexpr (LOGITS) {
      float m = fmaxf(fmaxf(xr[0].x, xr[0].y), fmaxf(xr[0].z, xr[0].w));
#pragma unroll
      for (int q = 1; q < VPL; ++q) m = fmaxf(m, fmaxf(fmaxf(xr[q].x, xr[q].y), fmaxf(xr[q].z, xr[q].w)));
      mx = wave_max_dpp(m);
      mx = (mx == -INFINITY) ? 0.f : mx;
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < VPL; ++q)
        s += fexp2((xr[q].x - mx) * LOG2E) + fexp2((xr[q].y - mx) * LOG2E) + fexp2((xr[q].z - mx) * LOG2E) +
             fexp2((xr[q].w - mx) * LOG2E);
      l2s = flog2(wave_sum_dpp(s));
    }
  }

  // emission gather through an LDS copy of the row (base_loss.py:328-344, 365-371), split in two so that the LDS
  // round trip of frame t+1 is in flight while frame t is processed: gather_issue early, gather_finish late.
  struct Raw { float xg[NL]; float xb; };
  __device__ __forceinline__ void gather_issue(const float4 (&xr)[VPL], int parity, Raw &w) const {
    float *buf = xs + parity * (V + 4);
#pragma unroll
    for (int q = 0; q < VPL; ++q)  // element-wise rebuild: a whole-float4 copy out of the register ring keeps the ring in scratch
      *reinterpret_cast<float4 *>(buf + 256 * q + lane * 4) = make_float4(xr[q].x, xr[q].y, xr[q].z, xr[q].w);
    const char *bb = reinterpret_cast<const char *>(buf);
#pragma unroll
    for (int j = 0; j < NL; ++j) w.xg[j] = *reinterpret_cast<const float *>(bb + tokoff[j]);
    w.xb = buf[blank];
  }
  __device__ __forceinline__ void gather_finish(const Raw &w, float mx, float l2s, Emis<NL> &e) const {
#pragma unroll
    for (int j = 0; j < NL; ++j)
      e.y[j] = fmaxf((w.xg[j] - mx) * LOG2E - l2s, NEG);  // v_max returns the non-NaN operand: (-inf) - (-inf) -> sentinel
    e.bl = fmaxf((w.xb - mx) * LOG2E - l2s, NEG);
    e.mx = mx;
    e.l2s = l2s;
  }
  __device__ __forceinline__ void gather(const float4 (&xr)[VPL], int parity, float mx, float l2s, Emis<NL> &e) const {
    Raw w;
    gather_issue(xr, parity, w);
    gather_finish(w, mx, l2s, e);
  }

  __device__ __forceinline__ void emit(const float4 (&xr)[VPL], int parity, Emis<NL> &e) const {
    float mx, l2s;
    stats(xr, mx, l2s);
    gather(xr, parity, mx, l2s, e);
  }

  // Q frames at once: the two wave reductions of the statistics are batched (ctc_dpp_batch.h: no s_nop padding, one
  // dependency chain of 6 levels instead of Q) and all LDS gathers are in flight before the first one is consumed.
  // One LDS row copy serves all Q frames: LDS operations of a wavefront execute in program order.
  template <int Q>
  __device__ __forceinline__ void emit_n(const float4 (&xr)[Q][VPL], Emis<NL> (&e)[Q]) const {
    float mx[Q], l2s[Q];
    if constexpr (LOGITS) {
      float m[Q];
#pragma unroll
      for (int f = 0; f < Q; ++f) {
        m[f] = fmaxf(fmaxf(xr[f][0].x, xr[f][0].y), fmaxf(xr[f][0].z, xr[f][0].w));
#pragma unroll
        for (int q = 1; q < VPL; ++q) m[f] = fmaxf(m[f], fmaxf(fmaxf(xr[f][q].x, xr[f][q].y), fmaxf(xr[f][q].z, xr[f][q].w)));
      }
      dpp_max_n<Q>(m);
      float sm[Q];
#pragma unroll
      for (int f = 0; f < Q; ++f) {
        mx[f] = readlane_f(m[f], 63);
        mx[f] = (mx[f] == -INFINITY) ? 0.f : mx[f];
        sm[f] = 0.f;
#pragma unroll
        for (int q = 0; q < VPL; ++q)
          sm[f] += fexp2((xr[f][q].x - mx[f]) * LOG2E) + fexp2((xr[f][q].y - mx[f]) * LOG2E) +
                   fexp2((xr[f][q].z - mx[f]) * LOG2E) + fexp2((xr[f][q].w - mx[f]) * LOG2E);
      }
      dpp_sum_n<Q>(sm);
#pragma unroll
      for (int f = 0; f < Q; ++f) l2s[f] = flog2(readlane_f(sm[f], 63));
    } else {
#pragma unroll
      for (int f = 0; f < Q; ++f) { mx[f] = 0.f; l2s[f] = 0.f; }
    }
    Raw w[Q];
#pragma unroll
    for (int f = 0; f < Q; ++f) gather_issue(xr[f], 0, w[f]);
#pragma unroll
    for (int f = 0; f < Q; ++f) gather_finish(w[f], mx[f], l2s[f], e[f]);
  }

  // one lattice step (identical recursions to Scan::step in ctc_kernels.hip)
  __device__ __forceinline__ void step(const Emis<NL> &e) {
    const float bl = e.bl;
    if constexpr (KIND == 0 && DIR == 0) {
      ST m[NL], x[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        m[j] = lse2(c[j], o[j]);
        x[j] = norep_next[j] ? m[j] : c[j];
      }
      ST xin0 = from_prev_lane(x[NL - 1], cx);
#pragma unroll
      for (int j = NL - 1; j >= 0; --j) {
        ST xin = (j == 0) ? xin0 : x[j - 1];
        o[j] = e.y[j] + lse2(o[j], xin);
        c[j] = bl + m[j];
      }
      cx += bl;
    } else if constexpr (KIND == 0 && DIR == 1) {
      ST h[NL], ee[NL], pn[NL], x[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        h[j] = bl + c[j];
        ee[j] = e.y[j] + o[j];
        pn[j] = lse2(h[j], ee[j]);
        x[j] = norep[j] ? pn[j] : h[j];
      }
      cx += bl;
      ST xinl = from_next_lane(x[0], cx);
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        ST xin = (j == NL - 1) ? xinl : x[j + 1];
        o[j] = lse2(xin, ee[j]);
        c[j] = pn[j];
      }
    } else if constexpr (KIND == 1 && DIR == 0) {
      ST pin0 = from_prev_lane(c[NL - 1], cx);
#pragma unroll
      for (int j = NL - 1; j >= 0; --j) {
        ST pin = (j == 0) ? pin0 : c[j - 1];
        c[j] = lse2(bl + c[j], e.y[j] + pin);
      }
      cx += bl;
    } else {
      ST nin = from_next_lane(c[0], cx);
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        ST nx = (j == NL - 1) ? nin : c[j + 1];
        c[j] = lse2(bl + c[j], e.y[j] + nx);
      }
      cx += bl;
    }
  }

  __device__ __forceinline__ void renorm() {
    float mx = (float)cx;  // (any common shift will do: the float32 image of the maximum, subtracted as it is)
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      mx = fmaxf(mx, (float)c[j]);
      if constexpr (KIND == 0) mx = fmaxf(mx, (float)o[j]);
    }
    mx = wave_max_dpp(mx);
    mx = (mx > NEG_THR) ? mx : 0.f;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      c[j] -= mx;
      if constexpr (KIND == 0) o[j] -= mx;
    }
    cx -= mx;
    off += (double)mx;
  }

  // spill the current state as lattice row `t` in the layout the other side is aligned with
  __device__ __forceinline__ void spill(int t, float smx, float sl2s) const {
    float cs[NL], os[NL];  // (rows are float32 whatever the state type)
    float tx;
    if constexpr (DIR == 0) {  // slot i <- state_c(l=i): previous slot's c; tail <- state_c(l=UP): last slot's c
#pragma unroll
      for (int j = NL - 1; j > 0; --j) cs[j] = (float)c[j - 1];
      cs[0] = from_prev_lane((float)c[NL - 1], (float)cx);
      tx = readlane_f((float)c[NL - 1], 63);
    } else {  // slot i <- state_c(l=i+1): next slot's c; tail <- state_c(l=0): first slot's c
#pragma unroll
      for (int j = 0; j < NL - 1; ++j) cs[j] = (float)c[j + 1];
      cs[NL - 1] = from_next_lane((float)c[0], (float)cx);
      tx = readlane_f((float)c[0], 0);
    }
#pragma unroll
    for (int j = 0; j < NL; ++j) os[j] = (float)o[j];
    const float oh = (float)off;
    store_srow<KIND, NL>(own_rows + (long)t * SRS, lane, UP, cs, os, make_float4(tx, 0.f, oh, (float)(off - (double)oh)),
                         make_float2(smx, sl2s));
  }

  // log2 P at the meeting point from this side's state and the other side's row of the same time index
  __device__ __forceinline__ double meet(const SRow<KIND, NL> &r) const {
    ST v[2 * NL + 1];
    float m = (float)(cx + r.tail.x);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      v[2 * j] = c[j] + r.a[j];
      v[2 * j + 1] = (KIND == 0) ? o[j] + r.b[j] : (ST)NEG;
      m = fmaxf(m, fmaxf((float)v[2 * j], (float)v[2 * j + 1]));
    }
    m = wave_max_dpp(m);
    if (!(m > NEG_THR)) return -INFINITY;
    float s = (lane == 0) ? fexp2((float)(cx + r.tail.x - m)) : 0.f;
#pragma unroll
    for (int j = 0; j < 2 * NL; ++j) s += fexp2((float)(v[j] - m));
    s = wave_sum_dpp(s);
    return (double)m + (double)flog2(s) + off + (double)r.tail.z + (double)r.tail.w;
  }

  // posterior scatter + gradient row of frame t.  s1/s2/s0 are base-2 log posteriors of the blank parts, the token parts
  // and the out-of-range blank part (see the table in the kernel body); xr is the logits row, e its statistics.
  __device__ __forceinline__ void grad_row(int t, const float (&s1)[NL], const float (&s2)[NL], float s0,
                                           const float4 (&xr)[VPL], const Emis<NL> &e) const {
#pragma unroll
    for (int q = 0; q < VPL; ++q) *reinterpret_cast<uint4 *>(bins + 256 * q + lane * 4) = make_uint4(0u, 0u, 0u, 0u);  // (same type as the atomics and the read: float stores may be reordered against them)
    float qb = (lane == 0) ? fexp2(s0) : 0.f;
    float qt[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      qb += fexp2(s1[j]);
      qt[j] = fexp2(s2[j]);
    }
    // Normalised by the frame's OWN mass (= 1 when the log P of the meeting point and both sweeps are exact; the invariant of the
    // reference's tests/test_classic_ctc_loss.py:146-167): what a long float32 log-domain sweep has accumulated in rounding enters
    // every posterior of a frame as the same factor -- dividing it out took this tier's gradient error at T = 1000 with sharp
    // logits from ~1e-3 to the 1e-4 class (r03; the three-kernel pipeline does the same, ctc_grad_row.h).
    {
      float tot = qb;
#pragma unroll
      for (int j = 0; j < NL; ++j) tot += qt[j];
      const float mass = wave_sum_dpp(tot);
      const float f = (mass > 0.f && mass < INFINITY) ? 1.0f / mass : 1.0f;
      qb *= f;
#pragma unroll
      for (int j = 0; j < NL; ++j) qt[j] *= f;
    }
    // (no wave barrier needed: LDS ops of one wave execute in order and may-alias accesses keep program order)
    // Scatter by label with FIXED-POINT integer atomics.  ds_add_f32 turned out to be the bottleneck of the whole kernel
    // on gfx950 (it throttles every wavefront of the CU that touches LDS; replacing it with a plain store -- wrong for
    // repeated tokens -- made the kernel 1.4x faster), ds_add_u32 runs at the normal LDS rate.  Posteriors lie in [0, 1]:
    // 2^-30 resolution, the per-token sum of posteriors is <= 1, and the clamp keeps degenerate inputs from wrapping.
    char *bb = reinterpret_cast<char *>(bins);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const unsigned qi = (unsigned)(fminf(qt[j], 1.0f) * 1073741824.0f + 0.5f);
      if (tokoff[j] != 4 * V) atomicAdd(reinterpret_cast<unsigned *>(bb + tokoff[j]), qi);  // (positions >= label_length point at the pad slot: their adds would serialise on it)
    }
    wave_lds_fence();  // the bins read below were written by other lanes
    qb = wave_sum_dpp(qb);
    // (no wave barrier needed: LDS ops of one wave execute in order and may-alias accesses keep program order)
#pragma unroll
    for (int q = 0; q < VPL; ++q) {
      const uint4 pu = *reinterpret_cast<const uint4 *>(bins + 256 * q + lane * 4);
      float4 pq = make_float4((float)pu.x * 9.31322574615478515625e-10f, (float)pu.y * 9.31322574615478515625e-10f,
                              (float)pu.z * 9.31322574615478515625e-10f, (float)pu.w * 9.31322574615478515625e-10f);
      pq.x += mb[4 * q] * qb; pq.y += mb[4 * q + 1] * qb; pq.z += mb[4 * q + 2] * qb; pq.w += mb[4 * q + 3] * qb;
      float4 r;
      if constexpr (LOGITS) {
        r.x = dl * (fexp2((xr[q].x - e.mx) * LOG2E - e.l2s) - pq.x);
        r.y = dl * (fexp2((xr[q].y - e.mx) * LOG2E - e.l2s) - pq.y);
        r.z = dl * (fexp2((xr[q].z - e.mx) * LOG2E - e.l2s) - pq.z);
        r.w = dl * (fexp2((xr[q].w - e.mx) * LOG2E - e.l2s) - pq.w);
      } else {
        r.x = -dl * pq.x; r.y = -dl * pq.y; r.z = -dl * pq.z; r.w = -dl * pq.w;
      }
      store_g(t, q, r);
    }
    // (no wave barrier needed: LDS ops of one wave execute in order and may-alias accesses keep program order)
  }

  // grad_row with the posterior exponents pre-biased by +30 (the caller adds 30 to the block scale): exp2 then yields
  // the posterior already in the 2^30 fixed-point unit of the LDS token row, and the way back folds 2^-30 and d_loss into
  // one fused multiply-add per token (6 VALU instructions per frame less than grad_row).  Posteriors of a feasible sample
  // are <= 1, so 2^30 q fits the 32-bit integer row without a clamp.
  __device__ __forceinline__ void grad_row30(int t, const float (&s1)[NL], const float (&s2)[NL], float s0,
                                             const float4 (&xr)[VPL], const Emis<NL> &e) const {
#pragma unroll
    for (int q = 0; q < VPL; ++q) *reinterpret_cast<uint4 *>(bins + 256 * q + lane * 4) = make_uint4(0u, 0u, 0u, 0u);  // (same type as the atomics and the read: float stores may be reordered against them)
    float qb = (lane == 0) ? fexp2(s0) : 0.f;
    float qt[NL], tot;
    char *bb = reinterpret_cast<char *>(bins);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      qb += fexp2(s1[j]);
      qt[j] = fexp2(s2[j]);
    }
    tot = qb;
#pragma unroll
    for (int j = 0; j < NL; ++j) tot += qt[j];
    // normalised by the frame's own mass (2^30 in these units when everything is exact; see grad_row)
    const float mass = wave_sum_dpp(tot);
    const float f = (mass > 0.f && mass < INFINITY) ? 1073741824.0f / mass : 1.0f;
#pragma unroll
    for (int j = 0; j < NL; ++j)
      if (tokoff[j] != 4 * V) atomicAdd(reinterpret_cast<unsigned *>(bb + tokoff[j]), (unsigned)(qt[j] * f + 0.5f));
    wave_lds_fence();  // the bins read below were written by other lanes
    qb = wave_sum_dpp(qb) * f;  // blank posterior, in units of 2^-30
    const float c1 = -dl * 9.31322574615478515625e-10f;
#pragma unroll
    for (int q = 0; q < VPL; ++q) {
      const uint4 pu = *reinterpret_cast<const uint4 *>(bins + 256 * q + lane * 4);
      const float4 pq = make_float4((float)pu.x + mb[4 * q] * qb, (float)pu.y + mb[4 * q + 1] * qb,
                                    (float)pu.z + mb[4 * q + 2] * qb, (float)pu.w + mb[4 * q + 3] * qb);
      float4 r;
      if constexpr (LOGITS) {
        r.x = pq.x * c1 + dl * fexp2((xr[q].x - e.mx) * LOG2E - e.l2s);
        r.y = pq.y * c1 + dl * fexp2((xr[q].y - e.mx) * LOG2E - e.l2s);
        r.z = pq.z * c1 + dl * fexp2((xr[q].z - e.mx) * LOG2E - e.l2s);
        r.w = pq.w * c1 + dl * fexp2((xr[q].w - e.mx) * LOG2E - e.l2s);
      } else {
        r.x = pq.x * c1; r.y = pq.y * c1; r.z = pq.z * c1; r.w = pq.w * c1;
      }
      store_g(t, q, r);
    }
  }

  // phase-2 frame: posterior of frame t from this side's state and the other side's row, then the gradient row.
  //   classic    A: after the step, state = alpha[t+1], r = beta[t+1]      B: before the step, state = beta[t+1], r = alpha[t+1]
  //   simplified A: before the step, state = a[t], r = b[t+1]              B: before the step, state = b[t+1], r = a[t]
  // (blank part, token part) per slot:  classic (c + r.a, o + r.b);  simplified A (c + bl + r.a, pin + y + r.a);
  // simplified B (c + bl + r.a, r.a + y + next)   -- regroupings of classic_ctc_loss.py:565-669 / simplified_ctc_loss.py:456-534
  // posterior exponents of one frame (+ the lattice step at the right place): fills s1 (blank parts), s2 (token parts), s0
  __device__ __forceinline__ void post_step(const Emis<NL> &e, const SRow<KIND, NL> &r, double dlogp, float (&s1)[NL],
                                            float (&s2)[NL], float &s0) {
    post_step_sc(e, r, (float)((double)r.tail.z + (off - dlogp)) + r.tail.w, s1, s2, s0);
  }
  // same with the scale sc = off + row offset - log2 P supplied by the caller (constant inside a block when neither this
  // chain nor the producer of the rows renormalises inside the block)
  __device__ __forceinline__ void post_step_sc(const Emis<NL> &e, const SRow<KIND, NL> &r, float sc, float (&s1)[NL],
                                               float (&s2)[NL], float &s0) {
    if constexpr (KIND == 0 && DIR == 0) step(e);
    if constexpr (KIND == 0) {
#pragma unroll
      for (int j = 0; j < NL; ++j) { s1[j] = (float)(c[j] + r.a[j] + sc); s2[j] = (float)(o[j] + r.b[j] + sc); }
      s0 = (float)(cx + r.tail.x + sc);
    } else if constexpr (DIR == 0) {
      ST pin0 = from_prev_lane(c[NL - 1], cx);
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        ST pin = (j == 0) ? pin0 : c[j - 1];
        s1[j] = (float)(c[j] + e.bl + r.a[j] + sc);
        s2[j] = (float)(pin + e.y[j] + r.a[j] + sc);
      }
      s0 = (float)(cx + e.bl + r.tail.x + sc);
    } else {
      ST nin = from_next_lane(c[0], cx);
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        ST nx = (j == NL - 1) ? nin : c[j + 1];
        s1[j] = (float)(c[j] + e.bl + r.a[j] + sc);
        s2[j] = (float)(r.a[j] + e.y[j] + nx + sc);
      }
      s0 = (float)(cx + e.bl + r.tail.x + sc);
    }
    if constexpr (!(KIND == 0 && DIR == 0)) step(e);
  }

  __device__ __forceinline__ void frame2(int t, const float4 (&xr)[VPL], const Emis<NL> &e, const SRow<KIND, NL> &r, double dlogp) {
    float s1[NL], s2[NL], s0;
    post_step(e, r, dlogp, s1, s2, s0);
    grad_row(t, s1, s2, s0, xr, e);
  }

  __device__ __forceinline__ void zero_rows(int t_from, int t_to) const {
    for (int t = t_from; t < t_to; ++t) {
#pragma unroll
      for (int q = 0; q < VPL; ++q) store_g(t, q, make_float4(0.f, 0.f, 0.f, 0.f));
    }
  }
};

}  // namespace fused
}  // namespace ctc
