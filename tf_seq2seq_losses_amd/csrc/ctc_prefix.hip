// CTC prefix scores, the step-wise scorer of label-synchronous decoding: ctc_amd_prefix_rows / ctc_amd_prefix_extend /
// ctc_amd_prefix_score (include/ctc_amd.h), DESIGN.md section 5.14.
//
// The state of a prefix g (hypothesis (b, n)) is SD = 2 T + 2 float64 base-2 logarithms:
//   [t]        s[t]  = lse(rn[t], rb[t]): frames 0..t emit exactly g                       (t < T_b; -inf behind)
//   [T + t]    rb[t]: ... and frame t is a blank                                           (t < T_b; -inf behind)
//   [2 T]      rep   = lse_{t >= 1}(rb[t-1] + lp[t, last(g)]): the classic lattice's score of repeating the last token
//   [2 T + 1]  ref   = max_t (s[t-1] - log2 sum_t), the reference exponent of the score kernel (s[-1] = 0 for the empty prefix)
// rn itself is never needed again: the entry weight of every other candidate is s[t-1], the repeated token's is rb[t-1].
//
//   prefix_rows_kernel     one wavefront per row (b, t): row maximum and log2 sum exp(x - max), once per scorer;
//   prefix_extend_kernel   one wavefront per new hypothesis.  Per block of 64 frames the lanes gather x[t, c], x[t, blank], the row
//                          statistics and the parent's entry weight of frame t0 + lane and form the float64 emissions in parallel;
//                          the two-value recurrence then runs its <= 64 dependent steps on wavefront-uniform values (operands by
//                          v_readlane), lane k keeps step k's result, and s, rep and ref are finished lane-parallel;
//   prefix_score_kernel    one workgroup per (utterance, 64 columns, group of 8 hypotheses): lane = column, wavefront = time
//                          slice (chunks of 8 frames, round robin).  Per chunk a wavefront reads 8 x 64 logits once and uses them
//                          for all eight hypotheses: v = y[t, c] + w[n, t] with y = (x - max) log2 e shared and the float32 weight
//                          w = s[t-1] - log2 sum_t - ref of hypothesis n broadcast by v_readlane.  Accumulation: running maximum
//                          per (n, c), rescaled once per chunk, so a term far below the maximum adds 0 and nothing overflows;
//                          the four slices meet in LDS and are added in slice order.
// Numerics as ctc_nbest.hip: float64 state, float32 exp2 / log2 of float64 differences, a true -inf, and the emission from
// (double)x - (double)max.  Every result of hypothesis (b, n) is a function of its own state and of utterance b's rows: the same
// bits for every N, slot and neighbour.
#include "ctc_common.h"
#include "ctc_prefix.h"

namespace ctc {
namespace {

constexpr double LOG2E_D = 1.44269504088896340736;
constexpr int PFX_WAVES = 4;            // wavefronts per workgroup of every kernel here; the score kernel's time slices
constexpr int PFX_FB = 8;               // frames per chunk of the score kernel: PFX_G * PFX_FB = 64 weights, one per lane
constexpr float PFX_FLOOR = -3.0e38f;   // the running maximum before anything was added (finite: no inf - inf)

// base-2 log(2^a + 2^b) of float64 operands that may be -inf (ctc_nbest.hip nb_lse)
__device__ __forceinline__ double pf_lse(double a, double b) {
  const double m = fmax(a, b);
  const double mm = m == -__builtin_inf() ? 0.0 : m;
  return mm + (double)flog2(fexp2((float)(a - mm)) + fexp2((float)(b - mm)));
}
// lane k's value in every lane (k wavefront-uniform)
__device__ __forceinline__ float lane_bcast(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ double lane_bcast(double v, int k) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), k), __builtin_amdgcn_readlane(__double2loint(v), k));
}

struct PfxIo {
  const float2 *rows;      // [B][T] (row max, log2 sum exp(x - max)); not read for WRT_LOGPROBS
  const double *state_in;  // [B][N][SD]
  const int *last_in, *len_in, *parent, *token;
  double *state_out;
  int *last_out, *len_out;
  float *full;
  int N;
};

__device__ __forceinline__ const char *pf_row(const Problem &p, int b, int t) {
  return reinterpret_cast<const char *>(p.logits) + (size_t)((long)b * p.xsb + (long)t * p.xst) * (p.xdtype == 0 ? 4 : 2);
}

__global__ __launch_bounds__(64 * PFX_WAVES) void prefix_rows_kernel(const Problem p, float2 *__restrict__ rows) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long row = (long)blockIdx.x * PFX_WAVES + wv;
  if (row >= (long)p.B * p.T) return;  // (wavefront-uniform)
  const int b = (int)(row / p.T), t = (int)(row % p.T);
  if (t >= frame_count(p, b)) {
    if (lane == 0) rows[row] = make_float2(0.f, 0.f);
    return;
  }
  const char *const x = pf_row(p, b, t);
  float m = PFX_FLOOR, s = 0.f;
  for (int k = lane; k < p.V; k += 64) {
    const float v = row_load1(x, k, p.xdtype);
    const float mn = fmaxf(m, v);
    s = s * fexp2((m - mn) * LOG2E) + fexp2((v - mn) * LOG2E);
    m = mn;
  }
  float M = wave_max(m);
  const float S = wave_sum(s * fexp2((m - M) * LOG2E));
  float l2s = flog2(S);
  if (!(S > 0.f)) { M = 0.f; l2s = __builtin_inff(); }  // a row of -inf: every emission of the frame is -inf
  if (lane == 0) rows[row] = make_float2(M, l2s);
}

template <int KIND>
__global__ __launch_bounds__(64 * PFX_WAVES) void prefix_extend_kernel(const Problem p, const PfxIo a) {
  const double NINF = -__builtin_inf();
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long h = (long)blockIdx.x * PFX_WAVES + wv;
  if (h >= (long)p.B * a.N) return;  // (wavefront-uniform; nothing below synchronises beyond the wavefront)
  const int b = (int)(h / a.N);
  const int T = p.T, Tb = frame_count(p, b);
  const size_t SD = 2 * (size_t)T + 2;
  double *const so = a.state_out + (size_t)h * SD;
  const int par = a.parent[h], tok = a.token[h];
  const bool empty = par == -2;  // the empty prefix: no parent, the token is not looked at
  int plen = -1, plast = -1;
  const double *si = nullptr;
  if (par >= 0 && par < a.N && a.state_in) {
    const long ph = (long)b * a.N + par;
    plen = a.len_in[ph]; plast = a.last_in[ph];
    si = a.state_in + (size_t)ph * SD;
  }
  if (!(empty || (plen >= 0 && emits(p, tok)))) {  // no parent, a dead parent or an impossible emission: the dead state
    for (size_t i = lane; i < SD; i += 64) so[i] = NINF;
    if (lane == 0) { a.last_out[h] = -1; a.len_out[h] = -1; a.full[h] = -__builtin_inff(); }
    return;
  }
  const int c = empty ? p.blank : tok;
  const bool rep = KIND == 0 && !empty && tok == plast;  // classic: a repeated token enters from the parent's blank state alone
  const bool stats = p.wrt == 0;
  double rn = NINF, rb = empty ? 0.0 : NINF;  // the chain, wavefront-uniform: the state after the frame before
  double carry_s = rb, carry_rb = rb;         // s and rb of the frame before the block
  double uacc = NINF, racc = NINF;            // lane-wise: max of s[t-1] - log2 sum_t; lse of rb[t-1] + e[t]
  for (int t0 = 0; t0 < Tb; t0 += 64) {
    const int t = t0 + lane;
    const bool valid = t < Tb;
    double e = NINF, eb = NINF, phi = NINF, l2s = 0.0;
    if (valid) {
      const char *const x = pf_row(p, b, t);
      const float xc = row_load1(x, c, p.xdtype), xk = row_load1(x, p.blank, p.xdtype);
      double Md = 0.0;
      if (stats) {
        const float2 r = a.rows[(size_t)b * T + t];
        Md = (double)r.x; l2s = (double)r.y;
      }
      e = fma((double)xc - Md, LOG2E_D, -l2s);
      eb = fma((double)xk - Md, LOG2E_D, -l2s);
      if (!empty) phi = t == 0 ? (plen == 0 ? 0.0 : NINF) : si[(rep ? T : 0) + t - 1];
    }
    const int nf = Tb - t0 < 64 ? Tb - t0 : 64;
    double my_rn = NINF, my_rb = NINF;
    for (int k = 0; k < nf; ++k) {
      const double pk = lane_bcast(phi, k), ek = lane_bcast(e, k), ebk = lane_bcast(eb, k);
      const double rn1 = (KIND == 0 ? pf_lse(rn, pk) : pk) + ek;
      rb = pf_lse(rb, rn) + ebk;
      rn = rn1;
      if (lane == k) { my_rn = rn; my_rb = rb; }
    }
    const double my_s = pf_lse(my_rn, my_rb);
    const double prev_s = from_prev_lane(my_s, carry_s), prev_rb = from_prev_lane(my_rb, carry_rb);
    if (valid) {
      so[t] = my_s;
      so[(size_t)T + t] = my_rb;
      uacc = fmax(uacc, prev_s - l2s);
      if (KIND == 0 && !empty) racc = pf_lse(racc, prev_rb + e);
    }
    carry_s = lane_bcast(my_s, 63);
    carry_rb = lane_bcast(my_rb, 63);
  }
  for (int t = Tb + lane; t < T; t += 64) { so[t] = NINF; so[(size_t)T + t] = NINF; }
  // the two summaries: float32 wave reductions around a reference, in a fixed order
  const float fr = wave_max((float)uacc);
  const float fm = wave_max((float)racc);
  const double mm = fm == -__builtin_inff() ? 0.0 : (double)fm;
  const float S = wave_sum(fexp2((float)(racc - mm)));
  const double fin = pf_lse(rn, rb);  // T_b == 0: 0 for the empty prefix, -inf otherwise
  if (lane == 0) {
    so[2 * (size_t)T] = mm + (double)flog2(S);
    so[2 * (size_t)T + 1] = (double)fr;
    a.last_out[h] = empty ? -1 : tok;
    a.len_out[h] = empty ? 0 : plen + 1;
    a.full[h] = (float)(fin * LN2_D);
  }
}

template <int KIND>
__global__ __launch_bounds__(64 * PFX_WAVES) void prefix_score_kernel(const Problem p, const PfxIo a, float *__restrict__ score) {
  constexpr int G = PREFIX_G;
  static_assert(G * PFX_FB == 64, "one weight per lane");
  __shared__ float2 part[PFX_WAVES][G][64];
  const double NINF = -__builtin_inf();
  const int b = blockIdx.x, n0 = blockIdx.z * G;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = blockIdx.y * 64 + lane;
  const bool cv = c < p.V;
  const int T = p.T, Tb = frame_count(p, b), N = a.N;
  const size_t SD = 2 * (size_t)T + 2;
  const bool stats = p.wrt == 0;
  // lane (g8, kk) makes the weight of hypothesis n0 + g8 at frame t0 + kk
  const int g8 = lane >> 3, kk = lane & 7;
  const bool hv = n0 + g8 < N;
  const size_t h8 = (size_t)b * N + (hv ? n0 + g8 : 0);
  const double *const s8 = a.state_in + h8 * SD;
  const int len8 = hv ? a.len_in[h8] : -1;
  const double ref8 = hv ? s8[2 * (size_t)T + 1] : NINF;
  const bool alive8 = len8 >= 0 && ref8 > NINF;

  float m[G], s[G];
#pragma unroll
  for (int g = 0; g < G; ++g) { m[g] = PFX_FLOOR; s[g] = 0.f; }
  const int nch = (Tb + PFX_FB - 1) / PFX_FB;
  for (int ch = wv; ch < nch; ch += PFX_WAVES) {
    const int t0 = ch * PFX_FB;
    float uf = -__builtin_inff(), Mk = 0.f;
    if (t0 + kk < Tb) {
      double l2s = 0.0;
      if (stats) {
        const float2 r = a.rows[(size_t)b * T + t0 + kk];
        Mk = r.x; l2s = (double)r.y;
      }
      if (alive8) {
        const double sp = t0 + kk == 0 ? (len8 == 0 ? 0.0 : NINF) : s8[t0 + kk - 1];
        uf = (float)((sp - l2s) - ref8);
      }
    }
    float y[PFX_FB];
#pragma unroll
    for (int k = 0; k < PFX_FB; ++k) {
      float xv = -__builtin_inff();
      if (cv && t0 + k < Tb) xv = row_load1(pf_row(p, b, t0 + k), c, p.xdtype);
      y[k] = (float)((double)xv - (double)lane_bcast(Mk, k)) * LOG2E;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float v[PFX_FB];
#pragma unroll
      for (int k = 0; k < PFX_FB; ++k) v[k] = y[k] + lane_bcast(uf, g * PFX_FB + k);
      float mx = v[0];
#pragma unroll
      for (int k = 1; k < PFX_FB; ++k) mx = fmaxf(mx, v[k]);
      const float mn = fmaxf(m[g], mx);
      float acc = s[g] * fexp2(m[g] - mn);
#pragma unroll
      for (int k = 0; k < PFX_FB; ++k) acc += fexp2(v[k] - mn);
      s[g] = acc; m[g] = mn;
    }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) part[wv][g][lane] = make_float2(m[g], s[g]);
  __syncthreads();
  // wavefront wv finishes hypotheses 2 wv and 2 wv + 1 of the group
#pragma unroll
  for (int q = 0; q < G / PFX_WAVES; ++q) {
    const int g = wv * (G / PFX_WAVES) + q, n = n0 + g;
    if (n >= N || !cv) continue;
    float M = part[0][g][lane].x;
#pragma unroll
    for (int i = 1; i < PFX_WAVES; ++i) M = fmaxf(M, part[i][g][lane].x);
    float S = 0.f;
#pragma unroll
    for (int i = 0; i < PFX_WAVES; ++i) S += part[i][g][lane].y * fexp2(part[i][g][lane].x - M);
    const size_t h = (size_t)b * N + n;
    const double *const st = a.state_in + h * SD;
    const int len = a.len_in[h];
    float out = -__builtin_inff();
    if (S > 0.f) out = (float)((st[2 * (size_t)T + 1] + (double)M + (double)flog2(S)) * LN2_D);
    if (KIND == 0 && len >= 1 && c == a.last_in[h]) out = (float)(st[2 * (size_t)T] * LN2_D);
    if (c == p.blank || len < 0) out = -__builtin_inff();
    score[h * (size_t)p.V + c] = out;
  }
}

}  // namespace

size_t prefix_rows_bytes(int B, int T) { return (size_t)B * T * sizeof(float2); }
size_t prefix_state_bytes(int B, int T, int N) { return (size_t)B * N * (2 * (size_t)T + 2) * sizeof(double); }

hipError_t run_prefix_rows(const Problem &p, void *rows, hipStream_t st) {
  const long nrows = (long)p.B * p.T;
  if (nrows == 0) return hipSuccess;
  hipLaunchKernelGGL(prefix_rows_kernel, dim3((unsigned)((nrows + PFX_WAVES - 1) / PFX_WAVES)), dim3(64 * PFX_WAVES), 0, st, p,
                     static_cast<float2 *>(rows));
  return hipGetLastError();
}

hipError_t run_prefix_extend(const Problem &p, int N, const void *rows, const double *state_in, const int *last_in, const int *len_in,
                             const int *parent, const int *token, double *state_out, int *last_out, int *len_out, float *full,
                             hipStream_t st) {
  const PfxIo a{static_cast<const float2 *>(rows), state_in, last_in, len_in, parent, token, state_out, last_out, len_out, full, N};
  const dim3 grid((unsigned)(((long)p.B * N + PFX_WAVES - 1) / PFX_WAVES));
  if (p.kind == 0) hipLaunchKernelGGL((prefix_extend_kernel<0>), grid, dim3(64 * PFX_WAVES), 0, st, p, a);
  else hipLaunchKernelGGL((prefix_extend_kernel<1>), grid, dim3(64 * PFX_WAVES), 0, st, p, a);
  return hipGetLastError();
}

hipError_t run_prefix_score(const Problem &p, int N, const void *rows, const double *state, const int *last, const int *len,
                            float *score, hipStream_t st) {
  const PfxIo a{static_cast<const float2 *>(rows), state, last, len, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, N};
  const dim3 grid(p.B, (p.V + 63) / 64, (N + PREFIX_G - 1) / PREFIX_G);
  if (p.kind == 0) hipLaunchKernelGGL((prefix_score_kernel<0>), grid, dim3(64 * PFX_WAVES), 0, st, p, a, score);
  else hipLaunchKernelGGL((prefix_score_kernel<1>), grid, dim3(64 * PFX_WAVES), 0, st, p, a, score);
  return hipGetLastError();
}

}  // namespace ctc
