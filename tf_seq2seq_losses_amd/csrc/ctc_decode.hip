// Greedy (best-token-per-frame) CTC decoding for both lattices: ctc_amd_greedy_decode (include/ctc_amd.h), DESIGN.md section 5.7.
//
// Two launches on the caller's stream:
//   row stage      frame-parallel over the B * T rows.  One wavefront reduces a row, DECODE_G rows in flight per wavefront; every
//                  lane keeps (max, lowest index at the max, sum of exp(x - max)) of its elements, the wave reduction takes the
//                  maximum and then the lowest index among the lanes that hold it.  Writes tokens[b, t] and the float32
//                  lp[b, t] = x[b, t, tok] - LSE_t (log-probability input: x[b, t, tok]) into the workspace.  The logits are read
//                  once, rows beyond logit_length not at all; no row is staged in LDS, so any V works.
//   collapse stage one wavefront per utterance, 64 frames per step: the previous frame's token comes from the neighbour lane
//                  (DPP, with a carry across steps), the keep predicate goes through a ballot, and the prefix popcount is the
//                  output position.  Classic keeps a frame whose token is no blank and differs from the previous frame's;
//                  simplified keeps every frame whose token is no blank.  Also the score (float64), the padding and the
//                  per-label run scores: on the classic lattice the lane that owns a label walks its run forward.
// No MFMA, no LDS, no scratch.
#include "ctc_common.h"
#include "ctc_lane_ops.h"
#include "ctc_launch.h"

namespace ctc {
namespace {

using fused::from_prev_lane_i;

constexpr int DECODE_G = 4;                          // rows in flight per wavefront
constexpr int DECODE_WAVES = 4;                      // wavefronts per workgroup of the row stage
constexpr int DECODE_ROWS = DECODE_G * DECODE_WAVES;  // rows per workgroup
constexpr int COLLAPSE_S = 4;                        // 64-frame steps of the collapse stage whose loads are in flight together
constexpr float FLT_LOWEST = -3.402823466e38f;
constexpr int NO_INDEX = 0x7fffffff;

// elements k .. k+3 of a row of element type dt (0 = float32, 1 = bfloat16, 2 = float16) as float32 (row_load1: ctc_common.h)
// (non-temporal: every row is read exactly once -- measured against the default policy in profiles/decode_time.md)
typedef float v4f __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 row_load4(const char *row, int k, int dt) {
  if (dt == 0) {
    const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f *>(row + (size_t)k * 4));
    return make_float4(t.x, t.y, t.z, t.w);
  }
  const v2u u = __builtin_nontemporal_load(reinterpret_cast<const v2u *>(row + (size_t)k * 2));
  return make_float4(h16_to_f32((unsigned short)(u.x & 0xffffu), dt), h16_to_f32((unsigned short)(u.x >> 16), dt),
                     h16_to_f32((unsigned short)(u.y & 0xffffu), dt), h16_to_f32((unsigned short)(u.y >> 16), dt));
}

// Running statistic of one lane: m = the maximum so far (-inf before the first element), idx = the lowest index holding it,
// s = sum of exp(x - max(m, FLT_LOWEST)) (the clamp keeps -inf elements and all -inf rows free of inf - inf).  A lane visits its
// indices in ascending order, so a strict comparison keeps the lowest one.  WRT == 1 (log-probabilities): no sum is needed.
template <int WRT>
__device__ __forceinline__ void stat_add4(float &m, int &idx, float &s, const float4 v, int k) {
  const float mo = fmaxf(m, FLT_LOWEST);
  if (v.x > m) { m = v.x; idx = k; }
  if (v.y > m) { m = v.y; idx = k + 1; }
  if (v.z > m) { m = v.z; idx = k + 2; }
  if (v.w > m) { m = v.w; idx = k + 3; }
  if (WRT == 0) {
    const float mn = fmaxf(m, FLT_LOWEST);
    s = s * fexp2((mo - mn) * LOG2E) +
        ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
  }
}

// wave-wide minimum of unsigned values, the same value in every lane (the reduction of ctc_common.h with v_min_u32)
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
  asm(CTC_WAVE_REDUCE_ASM("v_min_u32_dpp") : "+v"(v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

template <int WRT, bool VEC>
__global__ __launch_bounds__(64 * DECODE_WAVES) void decode_rows_kernel(const Problem p, long rows, int *__restrict__ tokens,
                                                                        float *__restrict__ lp) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = p.T, V = p.V, dt = p.xdtype;
  const int esz = dt == 0 ? 4 : 2;
  const long r0 = ((long)blockIdx.x * DECODE_WAVES + wave) * DECODE_G;
  if (r0 >= rows) return;

  // rows r0 .. r0 + G - 1 as (utterance, frame); a row past the end or beyond its utterance's length is not read
  const char *row[DECODE_G];
  bool live[DECODE_G];
  const char *any = nullptr;
  {
    int b = (int)(r0 / T), t = (int)(r0 - (long)b * T);
#pragma unroll
    for (int g = 0; g < DECODE_G; ++g) {
      live[g] = false;
      row[g] = nullptr;
      if (r0 + g < rows) {
        if (t < frame_count(p, b)) {
          live[g] = true;
          row[g] = reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb + (long)t * p.xst) * esz;
          if (!any) any = row[g];
        }
        if (++t == T) { t = 0; ++b; }
      }
    }
  }
  float m[DECODE_G], s[DECODE_G];
  int idx[DECODE_G];
  if (any) {
    // (a dead row of the group reads a live one's data again: the loads stay uniform, its results are dropped)
#pragma unroll
    for (int g = 0; g < DECODE_G; ++g) {
      if (!live[g]) row[g] = any;
      m[g] = -__builtin_inff(); s[g] = 0.f;
    }
    // Both paths give a lane the same elements in the same order -- k .. k+3 for k = 4 * lane, + 256, ... -- so their results are
    // the same bits: the element-wise one differs in the width of its loads alone (an element past V enters as -inf: it never
    // wins and adds exp(-inf) = 0).
#pragma unroll
    for (int g = 0; g < DECODE_G; ++g) idx[g] = lane * 4 < V ? lane * 4 : NO_INDEX;
    for (int k = lane * 4; k < V; k += 256) {
      float4 v[DECODE_G];
#pragma unroll
      for (int g = 0; g < DECODE_G; ++g) {
        if (VEC) {
          v[g] = row_load4(row[g], k, dt);
        } else {
          const float ninf = -__builtin_inff();
          v[g].x = row_load1(row[g], k, dt);
          v[g].y = k + 1 < V ? row_load1(row[g], k + 1, dt) : ninf;
          v[g].z = k + 2 < V ? row_load1(row[g], k + 2, dt) : ninf;
          v[g].w = k + 3 < V ? row_load1(row[g], k + 3, dt) : ninf;
        }
      }
#pragma unroll
      for (int g = 0; g < DECODE_G; ++g) stat_add4<WRT>(m[g], idx[g], s[g], v[g], k);
    }
  }
  // lane g of the wavefront writes row g's two results
  int my_tok = -1;
  float my_lp = 0.f;
#pragma unroll
  for (int g = 0; g < DECODE_G; ++g) {
    if (!any || !live[g]) continue;  // (uniform)
    const float M = wave_max(m[g]);
    // every lane whose maximum is the row's offers its lowest index; an all -inf row: every lane does, index 0 wins
    unsigned tok = wave_min_u(m[g] == M ? (unsigned)idx[g] : (unsigned)NO_INDEX);
    if (tok >= (unsigned)V) tok = 0;  // (NaN rows only: unspecified, but a token of the vocabulary)
    float v = M;
    if (WRT == 0) {
      const float Mf = fmaxf(M, FLT_LOWEST);
      const float S = wave_sum(s[g] * fexp2((fmaxf(m[g], FLT_LOWEST) - Mf) * LOG2E));
      // x[tok] - LSE = M - (M + ln S) = -ln S, S >= 1; a row whose maximum is -inf has log-probability -inf
      v = M == -__builtin_inff() ? M : (float)(-((double)flog2(S) * LN2_D));
    }
    if (lane == g) { my_tok = (int)tok; my_lp = v; }
  }
  if (lane < DECODE_G && r0 + lane < rows) {
    tokens[r0 + lane] = my_tok;
    if (my_tok >= 0) lp[r0 + lane] = my_lp;
  }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <int KIND>
__global__ __launch_bounds__(64) void decode_collapse_kernel(const Problem p, const int *__restrict__ tokens,
                                                             const float *__restrict__ lp, float *__restrict__ score,
                                                             int *__restrict__ decoded, int *__restrict__ decoded_length,
                                                             int *__restrict__ frames, float *__restrict__ label_score) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = p.T, blank = p.blank;
  const int Tb = frame_count(p, b);
  const size_t base = (size_t)b * T;
  const int *const tok_in = tokens + base;
  const float *const lp_in = lp + base;
  int *const dec = decoded + base;
  int *const frm = frames ? frames + base : nullptr;
  float *const lsc = label_score ? label_score + base : nullptr;

  int count = 0;   // labels written so far (uniform)
  int carry = -1;  // token of the frame before this step's first (-1: none)
  double acc = 0.0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int t0 = 0; t0 < Tb; t0 += 64 * COLLAPSE_S) {
    // the loads of COLLAPSE_S steps together (one wavefront per utterance: their latency is the stage's time), and the token
    // that follows them
    int tok[COLLAPSE_S];
    float v[COLLAPSE_S];
#pragma unroll
    for (int j = 0; j < COLLAPSE_S; ++j) {
      const int t = t0 + 64 * j + lane;
      tok[j] = t < Tb ? tok_in[t] : -1;
      v[j] = t < Tb ? lp_in[t] : 0.f;
    }
    const int after = t0 + 64 * COLLAPSE_S < Tb ? tok_in[t0 + 64 * COLLAPSE_S] : -1;
#pragma unroll
    for (int j = 0; j < COLLAPSE_S; ++j) {
      const int t = t0 + 64 * j + lane;
      const bool in = t < Tb;
      const int prev = from_prev_lane_i(tok[j], carry);
      const bool keep = in && tok[j] != blank && (KIND == 1 || tok[j] != prev);
      const unsigned long long mask = __builtin_amdgcn_ballot_w64(keep);
      // classic: the token of the next frame decides whether the label's run goes on (-1 past the length: it never does)
      const int next = fused::from_next_lane_i(tok[j], j + 1 < COLLAPSE_S ? __builtin_amdgcn_readlane(tok[j + 1 < COLLAPSE_S ? j + 1 : j], 0) : after);
      if (keep) {
        const int pos = count + __builtin_popcountll(mask & below);
        dec[pos] = tok[j];
        if (frm) frm[pos] = t;
        if (lsc) {
          // simplified: the label is that one frame.  Classic: the unbroken repeat of its token that starts here -- the lane that
          // owns the label walks the run forward, adding in time order.
          double sum = (double)v[j];
          if (KIND == 0 && next == tok[j])
            for (int u = t + 1; u < Tb && tok_in[u] == tok[j]; ++u) sum += (double)lp_in[u];
          lsc[pos] = (float)sum;
        }
      }
      count += __builtin_popcountll(mask);
      carry = __builtin_amdgcn_readlane(tok[j], 63);
      acc += (double)v[j];
    }
  }
  const double total = wave_sum_f64(acc);
  if (lane == 0) {
    score[b] = (float)total;
    decoded_length[b] = count;
  }
  for (int i = count + lane; i < T; i += 64) {
    dec[i] = -1;
    if (frm) frm[i] = -1;
    if (lsc) lsc[i] = -__builtin_inff();
  }
}

}  // namespace

size_t decode_workspace_bytes(int B, int T) { return ((size_t)B * T * 4 + 255) & ~size_t(255); }

bool decode_vector_rows(const Problem &p) {
  return ((p.V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (p.xdtype == 0 ? 15 : 7)) == 0;
}

hipError_t run_decode(const Problem &p, char *ws, float *score, int *tokens, int *decoded, int *decoded_length, int *frames,
                      float *label_score, hipStream_t st) {
  float *const lp = reinterpret_cast<float *>(ws);
  const long rows = (long)p.B * p.T;
  if (rows > 0) {
    const long blocks = (rows + DECODE_ROWS - 1) / DECODE_ROWS;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(64 * DECODE_WAVES);
    const bool vec = decode_vector_rows(p);
    if (p.wrt == 0) {
      if (vec) hipLaunchKernelGGL((decode_rows_kernel<0, true>), grid, block, 0, st, p, rows, tokens, lp);
      else hipLaunchKernelGGL((decode_rows_kernel<0, false>), grid, block, 0, st, p, rows, tokens, lp);
    } else {
      if (vec) hipLaunchKernelGGL((decode_rows_kernel<1, true>), grid, block, 0, st, p, rows, tokens, lp);
      else hipLaunchKernelGGL((decode_rows_kernel<1, false>), grid, block, 0, st, p, rows, tokens, lp);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (p.kind == 0) hipLaunchKernelGGL((decode_collapse_kernel<0>), dim3(p.B), dim3(64), 0, st, p, tokens, lp, score, decoded, decoded_length, frames, label_score);
  else hipLaunchKernelGGL((decode_collapse_kernel<1>), dim3(p.B), dim3(64), 0, st, p, tokens, lp, score, decoded, decoded_length, frames, label_score);
  return hipGetLastError();
}

}  // namespace ctc
