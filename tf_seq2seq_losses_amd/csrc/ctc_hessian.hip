// gfx950 kernel of the dense CTC Hessian hess[B][T][V][T][V] (the O(l^4) path of base_loss.py:186-260).
//
// The reference builds the all-pairs transition tensor gamma[B,T+1,L(,2),T+1,L(,2)] (classic_ctc_loss.py:167-308,
// simplified_ctc_loss.py:85-191; 22.5 GB at B=32,T=200,U=32) and contracts it twice.  Here gamma is never formed.
// With g = -posterior the log-probability-space Hessian is
//     H[t1,k1,t2,k2] = -P(k1 at t1 and k2 at t2 | label) + g[t1,k1] g[t2,k2]            (t1 != t2)
//     H[t,k1,t,k2]   = delta_{k1 k2} g[t,k1] + g[t,k1] g[t,k2]
// One wavefront owns one (b, t1, k1) slab [T][V] and writes ALL of it:
//   * rows t2 > t1: alpha[t1] is pushed through frame t1 with every emission but k1 masked, the restricted vector is
//     propagated forward with the ordinary alpha step and closed with beta[t2+1] exactly like the gradient does;
//   * rows t2 < t1: symmetrically, beta[t1+1] is pulled back through frame t1 with only k1 allowed and propagated
//     backward with the ordinary beta step, closing with alpha (this IS the symmetric half of base_loss.py:223-233,
//     generated directly instead of by transposing 10 GB);
//   * the lattice/emission rows of the next step are prefetched while the current step is processed.
// For logits-space output (what tape.batch_jacobian returns, README.md:58-71) the t1 == t2 blocks get
// + diag(s) - s s^T (s = softmax), because every k-sum of H vanishes and sum_k g = -1.
// The closing / step code is the one of the fused loss+grad kernels (Side::post_step_sc in ctc_fused_common.h).
#include <stdlib.h>

#include "ctc_fused_common.h"
#include "ctc_launch.h"

namespace ctc {

using namespace ctc::fused;

// The Hessian is written once and never read here: non-temporal stores keep 21 GB of output out of the caches the
// sweeps read their lattice, emission and gradient rows through.
__device__ __forceinline__ void nt_store(float *p, float v) { __builtin_nontemporal_store(v, p); }
__device__ __forceinline__ void nt_store(float *p, float4 r) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  v4f v = {r.x, r.y, r.z, r.w};
  __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(p));
}

template <int KIND, int NL>
__global__ __launch_bounds__(256) void hess_slab_kernel(Problem p, Layout L, const float *__restrict__ emis,
                                                         const float *__restrict__ alpha, const float *__restrict__ beta,
                                                         const double *__restrict__ logp, const float *__restrict__ g_lp,
                                                         const int *__restrict__ order, float *__restrict__ hess, int wpb,
                                                         unsigned long long stride) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: keeps everything derived from it in SGPRs
  const int T = p.T, V = p.V, UP = L.UP;
  const long ntask = (long)p.B * T * V;
  // Task list: token-position major over the per-utterance order that lists the tokens present in the label first
  // (hess_plan_kernel, below), walked with a stride permutation of the workgroups -- see hess_pair_kernel for why.
  const long wg = (long)(((unsigned long long)blockIdx.x * stride) % gridDim.x);
  const long task = wg * wpb + w;
  if (task >= ntask) return;
  const int idx = (int)(task / ((long)p.B * T));
  const int t1 = (int)(task % T);
  const int b = (int)((task / T) % p.B);
  const int k1 = order[(long)b * V + idx];
  float *out = hess + (((long)b * T + t1) * V + k1) * ((long)T * V);
  const int len = frame_count(p, b);
  int ll = label_count(p, b);
  const double lp = logp[b];
  const int32_t *lab = label_row(p, b);
  const LabelTok tok{ll, p, lab};

  auto zero_rows = [&](int t_from, int t_to) {
    if (t_to <= t_from) return;
    float *q = out + (long)t_from * V;
    const long n = (long)(t_to - t_from) * V;
    if (((n | (q - hess)) & 3) == 0) {
      for (long k = 4l * lane; k < n; k += 256) nt_store(q + k, make_float4(0.f, 0.f, 0.f, 0.f));
    } else {
      for (long k = lane; k < n; k += 64) nt_store(q + k, 0.f);
    }
  };
  const bool valid = (t1 < len) && (lp != -INFINITY) && !too_many_labels(p, ll);
  if (!valid) {  // padded frame or infeasible sample: the whole slab is zero (base_loss.py:240-258)
    zero_rows(0, T);
    return;
  }

  bool sel[NL];
  int tokb[NL];  // byte offset of label[i] in the LDS token row (pad slot for positions beyond the label)
  bool any = (k1 == p.blank);
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int i = lane * NL + j;
    const int tk = tok(i);
    sel[j] = (k1 != p.blank) && tk == k1;
    tokb[j] = 4 * ((tk >= 0 && tk < V && tk != p.blank) ? tk : V);  // (emits(p, tk), written out: the helper moves this kernel's code)
    any = any || sel[j];
  }
  any = __any(any);

  const float *grow = g_lp + (long)b * T * V;
  const float g1 = grow[(long)t1 * V + k1];
  const float *erows = emis + (long)b * T * L.ERS;
  const float *arows = alpha + (long)b * (T + 1) * L.SRS;
  const float *brows = beta + (long)b * (T + 1) * L.SRS;
  constexpr int PAIR = (KIND == 0) ? 2 : 1;
  const int tailpos = PAIR * UP;

  // ---- diagonal block t2 == t1 (base_loss.py:205-221: set_diag with the log-gradient) ----
  {
    float s1 = 0.f, mx = 0.f, l2s = 0.f;
    const float *x = p.logits + ((long)b * T + t1) * V;
    if (p.wrt == 0) {
      mx = erows[(long)t1 * L.ERS + UP + 1];
      l2s = erows[(long)t1 * L.ERS + UP + 2];
      s1 = fexp2((x[k1] - mx) * LOG2E - l2s);
    }
    for (int k2 = lane; k2 < V; k2 += 64) {
      float val = g1 * grow[(long)t1 * V + k2] + (k2 == k1 ? g1 : 0.f);
      if (p.wrt == 0) {
        float s2 = fexp2((x[k2] - mx) * LOG2E - l2s);
        val += (k2 == k1 ? s1 : 0.f) - s1 * s2;
      }
      out[(long)t1 * V + k2] = val;
    }
  }
  zero_rows(len, T);  // columns beyond logit_length (base_loss.py:254-258)
  if (!any) {  // token absent from the label: no joint mass with any other frame, g1 == 0
    zero_rows(0, t1);
    zero_rows(t1 + 1, len);
    return;
  }

  // joint posteriors are scattered by label with fixed-point integer LDS atomics (2^-30 resolution): ds_add_f32 is an
  // order of magnitude slower than ds_add_u32 on gfx950 (see ctc_fused_common.h)
  unsigned *ubin = reinterpret_cast<unsigned *>(lds + (long)w * (V + 4));
  auto tofix = [](float q) -> unsigned { return (unsigned)(fminf(q, 1.0f) * 1073741824.0f + 0.5f); };
  for (int k = lane; k < V + 4; k += 64) ubin[k] = 0u;

  // one prefetched step: emissions of frame t2 and the closing lattice row, already in the layout the sweep is aligned with
  struct Pre {
    float y[NL], bl;
    float a[NL], b2[NL], tx, oh, ol;
  };
  // wave-uniform values are fetched with VECTOR loads (scalar loads share lgkmcnt with the LDS traffic of emit_row and
  // return out of order, so every LDS wait also waited for the prefetched tails of the next step); vz is an opaque zero
  int vz;
  asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
  auto load_e = [&](Pre &q, int t) {
    const float *er = erows + (long)t * L.ERS;
#pragma unroll
    for (int j = 0; j < NL; ++j) q.y[j] = er[lane * NL + j];
    q.bl = er[UP + vz];
  };
  // beta row (workspace layout: slot i = state of l = i+1, the l = 0 state at the tail) as the forward sweep needs it
  auto load_fwd_row = [&](Pre &q, int trow) {
    const float *r = brows + (long)trow * L.SRS;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int i = lane * NL + j;
      if constexpr (KIND == 0) { float2 v = *reinterpret_cast<const float2 *>(r + 2 * i); q.a[j] = v.x; q.b2[j] = v.y; }
      else { q.a[j] = r[i]; q.b2[j] = NEG; }
    }
    q.tx = r[tailpos + vz]; q.oh = r[tailpos + 2 + vz]; q.ol = r[tailpos + 3 + vz];
  };
  // alpha row shifted into the layout the backward sweep is aligned with: slot i = (state_c(l=i), open(l=i+1)), tail l=UP
  auto load_bwd_row = [&](Pre &q, int trow) {
    const float *r = arows + (long)trow * L.SRS;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int i = lane * NL + j;
      q.a[j] = (i == 0) ? r[tailpos] : r[PAIR * (i - 1)];
      q.b2[j] = (KIND == 0) ? r[2 * i + 1] : NEG;
    }
    q.tx = r[PAIR * (UP - 1) + vz]; q.oh = r[tailpos + 2 + vz]; q.ol = r[tailpos + 3 + vz];
  };

  // close one frame: scatter the joint posteriors and write the Hessian row of frame t2
  auto emit_row = [&](int t2, const float (&s1)[NL], const float (&s2)[NL], float s0) {
    float qb = (lane == 0) ? fexp2(s0) : 0.f;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      qb += fexp2(s1[j]);
      atomicAdd(reinterpret_cast<unsigned *>(reinterpret_cast<char *>(ubin) + tokb[j]), tofix(fexp2(s2[j])));
    }
    qb = wave_sum_dpp(qb);
    if (lane == 0) ubin[p.blank] = tofix(qb);
    wave_lds_fence();
    for (int k2 = lane; k2 < V; k2 += 64) {  // base_loss.py:235-237 : -exp(.) + g (x) g
      nt_store(out + (long)t2 * V + k2, g1 * grow[(long)t2 * V + k2] - (float)ubin[k2] * 9.31322574615478515625e-10f);
      ubin[k2] = 0u;
    }
    wave_lds_fence();
  };

  auto fill_common = [&](auto &S) {
    S.lane = lane; S.UP = UP; S.blank = p.blank; S.ll = ll;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int i = lane * NL + j;
      S.norep[j] = (i == 0) || tok(i) != tok(i - 1);
      S.norep_next[j] = tok(i + 1) != tok(i);
    }
  };
  auto masked = [&](const Pre &q, Emis<NL> &e) {  // frame t1 with every emission but k1 forbidden
#pragma unroll
    for (int j = 0; j < NL; ++j) e.y[j] = sel[j] ? q.y[j] : NEG;
    e.bl = (k1 == p.blank) ? q.bl : NEG;
  };

  // =============== rows t2 > t1 : restricted alpha vector pushed forward ===============
  if (t1 + 1 < len) {
    Side<KIND, NL, 1, 0, true> S;
    fill_common(S);
    {
      const float *r = arows + (long)t1 * L.SRS;  // alpha[t1], workspace layout = native layout of an alpha chain
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const int i = lane * NL + j;
        if constexpr (KIND == 0) { float2 v = *reinterpret_cast<const float2 *>(r + 2 * i); S.c[j] = v.x; S.o[j] = v.y; }
        else { S.c[j] = r[i]; S.o[j] = NEG; }
      }
      S.cx = r[tailpos];
      S.off = (double)r[tailpos + 2] + (double)r[tailpos + 3];
      Pre q1;
      load_e(q1, t1);
      Emis<NL> e1;
      masked(q1, e1);
      S.step(e1);  // = alpha[t1+1] restricted to the states entered by emitting k1 at t1
    }
    Pre cur, nxt;
    load_e(cur, t1 + 1);
    load_fwd_row(cur, t1 + 2);
    for (int t2 = t1 + 1; t2 < len; ++t2) {
      const int tn = (t2 + 1 < len) ? t2 + 1 : t2;
      load_e(nxt, tn);          // prefetch the next step while this one is processed
      load_fwd_row(nxt, tn + 1);
      Emis<NL> e;
      SRow<KIND, NL> r;
#pragma unroll
      for (int j = 0; j < NL; ++j) { e.y[j] = cur.y[j]; r.a[j] = cur.a[j]; r.b[j] = cur.b2[j]; }
      e.bl = cur.bl;
      r.tail = make_float4(cur.tx, 0.f, cur.oh, cur.ol);
      const float sc = (float)((double)cur.oh + (S.off - lp)) + cur.ol;
      float s1[NL], s2[NL], s0;
      S.post_step_sc(e, r, sc, s1, s2, s0);
      emit_row(t2, s1, s2, s0);
      if (((t2 - t1) & 15) == 0) S.renorm();
      cur = nxt;
    }
  }

  // =============== rows t2 < t1 : restricted beta vector pulled backward ===============
  if (t1 > 0) {
    Side<KIND, NL, 1, 1, true> S;
    fill_common(S);
    {
      const float *r = brows + (long)(t1 + 1) * L.SRS;  // beta[t1+1] -> native layout of a beta chain (slot i = l = i)
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const int i = lane * NL + j;
        S.c[j] = (i == 0) ? r[tailpos] : r[PAIR * (i - 1)];
        S.o[j] = (KIND == 0) ? r[2 * i + 1] : NEG;
      }
      S.cx = r[PAIR * (UP - 1)];
      S.off = (double)r[tailpos + 2] + (double)r[tailpos + 3];
      Pre q1;
      load_e(q1, t1);
      Emis<NL> e1;
      masked(q1, e1);
      S.step(e1);  // = beta-like vector at t1 of the paths that emit k1 at t1
    }
    Pre cur, nxt;
    load_e(cur, t1 - 1);
    load_bwd_row(cur, KIND == 0 ? t1 : t1 - 1);  // classic closes with alpha[t2+1], simplified with a[t2]
    for (int t2 = t1 - 1; t2 >= 0; --t2) {
      const int tn = (t2 > 0) ? t2 - 1 : 0;
      load_e(nxt, tn);
      load_bwd_row(nxt, KIND == 0 ? tn + 1 : tn);
      Emis<NL> e;
      SRow<KIND, NL> r;
#pragma unroll
      for (int j = 0; j < NL; ++j) { e.y[j] = cur.y[j]; r.a[j] = cur.a[j]; r.b[j] = cur.b2[j]; }
      e.bl = cur.bl;
      r.tail = make_float4(cur.tx, 0.f, cur.oh, cur.ol);
      const float sc = (float)((double)cur.oh + (S.off - lp)) + cur.ol;
      float s1[NL], s2[NL], s0;
      S.post_step_sc(e, r, sc, s1, s2, s0);
      emit_row(t2, s1, s2, s0);
      if (((t1 - t2) & 15) == 0) S.renorm();
      cur = nxt;
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Short labels (U <= 32): TWO slabs per wavefront.
// With U <= 32 the lattice fills half a wavefront, so lanes 0-31 sweep the slab of one token and lanes 32-63 the slab of
// another token of the same (b, t1): the emission and closing rows are shared, the instruction count per slab halves.
// Tokens are paired by a per-utterance order that lists the tokens present in the label first (hess_plan_kernel), so
// that slabs with work share wavefronts and the all-zero slabs of absent tokens are plain fills.
// Half-wave conventions: hf = lane >> 5 selects the slab, hl = lane & 31 is the label slot (native layouts of
// ctc_fused_common.h with UP -> 32: the states l = 0 / l = 32 outside the slot range live in `cx`).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void hess_plan_kernel(Problem p, int *__restrict__ order, int *__restrict__ npres) {
  extern __shared__ unsigned char flag[];
  const int lane = threadIdx.x, b = blockIdx.x, V = p.V;
  int ll = label_count(p, b);
  if (too_many_labels(p, ll)) ll = 0;
  for (int k = lane; k < V; k += 64) flag[k] = 0;
  __syncthreads();
  if (lane == 0) flag[p.blank] = 1;
  for (int i = lane; i < ll && i < p.label_stride; i += 64) {
    const int tk = label_row(p, b)[i];
    if (in_vocab(p, tk)) flag[tk] = 1;  // (a label equal to the blank marks the blank, which is marked anyway)
  }
  __syncthreads();
  int base = 0;
  int *ord = order + (long)b * V;
  for (int pass = 0; pass < 2; ++pass) {  // present tokens first, then the absent ones
    for (int k0 = 0; k0 < V; k0 += 64) {
      const int k = k0 + lane;
      const bool f = k < V && (flag[k] != 0) == (pass == 0);
      const unsigned long long m = __ballot(f);
      if (f) ord[base + __popcll(m & ((1ull << lane) - 1ull))] = k;
      base += __popcll(m);
    }
    if (pass == 0 && lane == 0) npres[b] = base;
  }
}

// per-half reduction: afterwards lane 31 holds the result of lanes 0-31 and lane 63 the one of lanes 32-63
#define CTC_HALF_REDUCE_ASM(OP)                                                      \
  "s_nop 1\n\t" OP " %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"            \
  "s_nop 1\n\t" OP " %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"            \
  "s_nop 1\n\t" OP " %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"            \
  "s_nop 1\n\t" OP " %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"            \
  "s_nop 1\n\t" OP " %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"         \
  "s_nop 0"

__host__ __device__ inline int pairs_per_frame(int V, int U) {
  const int all = (V + 1) / 2, need = (U + 2) / 2;
  return need < all ? need : all;
}

template <int KIND>
__global__ __launch_bounds__(256, 6) void hess_pair_kernel(Problem p, Layout L, const float *__restrict__ emis,
                                                         const float *__restrict__ alpha, const float *__restrict__ beta,
                                                         const double *__restrict__ logp, const float *__restrict__ g_lp,
                                                         const int *__restrict__ order, const int *__restrict__ npres,
                                                         float *__restrict__ hess, int wpb, unsigned long long stride,
                                                         unsigned long long *dbg) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#ifdef CTC_HESS_STAMPS  // diagnostic build: cycle counts of the row-loop segments of one wavefront -> dbg[0..7]
  unsigned long long hst[6] = {0, 0, 0, 0, 0, 0}, hst_t = __builtin_amdgcn_s_memtime();
#define HST(i) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); hst[i] += t_ - hst_t; hst_t = t_; }
#else
#define HST(i)
#endif
  const int hf = lane >> 5, hl = lane & 31;
  const bool first = hl == 0, last = hl == 31;
  const int T = p.T, V = p.V, UP = L.UP;
  // wavefronts per (b, t1): one per pair of tokens that can be present (a label of U positions has at most U + 1
  // distinct tokens, the blank included); the slabs of the other tokens are shared out among them (below)
  const int npair = pairs_per_frame(V, p.U);
  const long ntask = (long)p.B * T * npair;
  const long task = (long)blockIdx.x * wpb + w;
  if (task >= ntask) return;
  // pair-major task list (all (b, t1) of pair 0, then pair 1, ...): the slabs with work come first, the fills last
  const int pair = (int)(task / ((long)p.B * T));
  const int t1 = (int)(task % T);
  const int b = (int)((task / T) % p.B);
  const int len = frame_count(p, b);
  const int ll = label_count(p, b);
  const double lp = logp[b];
  const long slab = (long)T * V;
  const int idx = 2 * pair + hf;
  const bool have = idx < V;                              // V odd: the last pair has one slab only
  const int k1 = have ? order[(long)b * V + idx] : 0;
  float *out = hess + (((long)b * T + t1) * V + k1) * slab;  // this half's slab
  const int k1a = __builtin_amdgcn_readlane(k1, 0), k1b = __builtin_amdgcn_readlane(k1, 32);
  const bool have_b = 2 * pair + 1 < V;
  auto fill_zero = [&](float *q, long n) {                // whole wavefront, wave-uniform arguments
    if (((n | (q - hess)) & 3) == 0) {
      for (long k = 4l * lane; k < n; k += 256) nt_store(q + k, make_float4(0.f, 0.f, 0.f, 0.f));
    } else {
      for (long k = lane; k < n; k += 64) nt_store(q + k, 0.f);
    }
  };
  float *out_a = hess + (((long)b * T + t1) * V + k1a) * slab;
  float *out_b = hess + (((long)b * T + t1) * V + k1b) * slab;
  auto zero_rows = [&](int t_from, int t_to) {            // rows [t_from, t_to) of both slabs
    if (t_to <= t_from) return;
    fill_zero(out_a + (long)t_from * V, (long)(t_to - t_from) * V);
    if (have_b) fill_zero(out_b + (long)t_from * V, (long)(t_to - t_from) * V);
  };
  const bool valid = (t1 < len) && (lp != -INFINITY) && !too_many_labels(p, ll);
  if (!valid) {  // padded frame or infeasible sample: all V slabs are zero (base_loss.py:240-258); this wavefront's share
    for (int i = (int)(((long)pair * V) / npair); i < (int)(((long)(pair + 1) * V) / npair); ++i)
      fill_zero(hess + (((long)b * T + t1) * V + i) * slab, slab);
    return;
  }
  // Slabs of tokens absent from the label are zero apart from their diagonal row.  They are not given wavefronts of
  // their own: the nh wavefronts of this (b, t1) that sweep share them and write them a little per sweep step (the
  // sweeps are VALU-bound, the fills HBM-bound; run back to back they did not overlap: 5.4 ms = 3.5 + 1.9).
  const int nh = (npres[b] + 1) / 2;   // pairs with at least one present token (the blank is always present)
  if (pair >= nh) return;
  const int32_t *lab = label_row(p, b);
  const LabelTok tok{ll, p, lab};
  const int tk = tok(hl);
  const bool sel = have && (k1 != p.blank) && tk == k1;
  const bool isblank = have && (k1 == p.blank);
  const bool norep = (hl == 0) || tk != tok(hl - 1);
  const bool norep_next = tok(hl + 1) != tk;

  const float *grow = g_lp + (long)b * T * V;
  const float g1 = have ? grow[(long)t1 * V + k1] : 0.f;
  const float *erows = emis + (long)b * T * L.ERS;
  const float *arows = alpha + (long)b * (T + 1) * L.SRS;
  const float *brows = beta + (long)b * (T + 1) * L.SRS;
  constexpr int PAIR = (KIND == 0) ? 2 : 1;
  const int tailpos = PAIR * UP;
  constexpr int W = 32;  // slots per slab

  // ---- diagonal block t2 == t1 (base_loss.py:205-221) ----
  {
    float s1 = 0.f, mx = 0.f, l2s = 0.f;
    const float *x = p.logits + ((long)b * T + t1) * V;
    if (p.wrt == 0) {
      mx = erows[(long)t1 * L.ERS + UP + 1];
      l2s = erows[(long)t1 * L.ERS + UP + 2];
      s1 = fexp2((x[k1] - mx) * LOG2E - l2s);
    }
    if (have) {
      for (int k2 = hl; k2 < V; k2 += W) {
        float val = g1 * grow[(long)t1 * V + k2] + (k2 == k1 ? g1 : 0.f);
        if (p.wrt == 0) {
          const float s2 = fexp2((x[k2] - mx) * LOG2E - l2s);
          val += (k2 == k1 ? s1 : 0.f) - s1 * s2;
        }
        out[(long)t1 * V + k2] = val;
      }
    }
  }
  zero_rows(len, T);  // columns beyond logit_length (base_loss.py:254-258)
  // ---- this wavefront's share of the absent tokens' slabs: order positions [a_lo, a_hi) ----
  const int na = V - 2 * nh;
  const int a_lo = 2 * nh + (int)(((long)pair * na) / nh), a_hi = 2 * nh + (int)(((long)(pair + 1) * na) / nh);
  const bool vec4 = (V & 3) == 0;
  const int funit = vec4 ? 256 : 64;  // floats per fill instruction
  const int *ord_b = order + (long)b * V;
  {  // diagonal rows of the assigned slabs (g1 = 0 there, so only the log-softmax term of the logits-space Hessian is left)
    const float *x = p.logits + ((long)b * T + t1) * V;
    const float mx = erows[(long)t1 * L.ERS + UP + 1], l2s = erows[(long)t1 * L.ERS + UP + 2];
    for (int i = a_lo; i < a_hi; ++i) {
      const int kx = ord_b[i];
      float *row = hess + (((long)b * T + t1) * V + kx) * slab + (long)t1 * V;
      const float s1 = (p.wrt == 0) ? fexp2((x[kx] - mx) * LOG2E - l2s) : 0.f;
      for (int k2 = lane; k2 < V; k2 += 64) {
        float val = 0.f;
        if (p.wrt == 0) val = (k2 == kx ? s1 : 0.f) - s1 * fexp2((x[k2] - mx) * LOG2E - l2s);
        row[k2] = val;
      }
    }
  }
  // streaming zero fill of rows [0, t1) and (t1, T) of those slabs: wave-uniform cursor, one instruction per call
  int f_idx = a_lo - 1, f_part = 1;
  long f_left = 0;
  float *f_ptr = hess;
  bool f_done = a_lo >= a_hi;
  auto f_advance = [&]() {
    while (f_left == 0 && !f_done) {
      if (f_part == 0) {
        f_part = 1;
        f_ptr += (long)V;  // skip the diagonal row
        f_left = (long)(T - 1 - t1) * V;
      } else {
        ++f_idx;
        if (f_idx >= a_hi) { f_done = true; break; }
        const int kx = __builtin_amdgcn_readfirstlane(ord_b[f_idx]);
        f_ptr = hess + (((long)b * T + t1) * V + kx) * slab;
        f_part = 0;
        f_left = (long)t1 * V;
      }
    }
  };
  f_advance();
  auto fill_step = [&]() {
    if (f_done) return;
    const int n = f_left < funit ? (int)f_left : funit;
    if (vec4) { if (4 * lane < n) nt_store(f_ptr + 4 * lane, make_float4(0.f, 0.f, 0.f, 0.f)); }
    else if (lane < n) nt_store(f_ptr + lane, 0.f);
    f_ptr += n;
    f_left -= n;
    if (f_left == 0) f_advance();
  };
  int f_per_row = 0;
  {
    const long per_slab = ((long)t1 * V + funit - 1) / funit + ((long)(T - 1 - t1) * V + funit - 1) / funit;
    const long units = per_slab * (a_hi - a_lo);
    const int rows = len - 1 > 0 ? len - 1 : 1;
    f_per_row = (int)((units + rows - 1) / rows);
  }

  // LDS per wavefront: two token rows (V + 4 each), then two staging buffers of SR output rows (burst writes, below)
  constexpr int SR = 8;
  float *wl = lds + (long)w * 2 * (V + 4 + SR * V);
  unsigned *ubin = reinterpret_cast<unsigned *>(wl) + hf * (V + 4);  // this half's token row
  float *stage = wl + 2 * (V + 4) + hf * (SR * V);                    // this half's SR staged rows
  auto tofix = [](float q) -> unsigned { return (unsigned)(fminf(q, 1.0f) * 1073741824.0f + 0.5f); };
  for (int k = hl; k < V + 4; k += W) ubin[k] = 0u;
  char *abin = reinterpret_cast<char *>(ubin) + 4 * ((tk >= 0 && tk < V && tk != p.blank) ? tk : V);  // (emits(p, tk), written out: as above)

  auto half_bcast = [&](float v) -> float {  // value of lane 31 / 63 to every lane of the half
    const float a = readlane_f(v, 31), bb = readlane_f(v, 63);
    return hf ? bb : a;
  };
  auto half_sum = [&](float v) -> float { asm(CTC_HALF_REDUCE_ASM("v_add_f32_dpp") : "+v"(v)); return half_bcast(v); };
  auto half_max = [&](float v) -> float { asm(CTC_HALF_REDUCE_ASM("v_max_f32_dpp") : "+v"(v)); return half_bcast(v); };
  auto prev_slot = [&](float x, float cx) -> float { const float s = from_prev_lane(x, cx); return first ? cx : s; };
  auto next_slot = [&](float x, float cx) -> float { const float s = from_next_lane(x, cx); return last ? cx : s; };

  // Wave-uniform values of the sweep (blank emission, row tails) are fetched with VECTOR loads: as scalar loads they
  // share lgkmcnt with the LDS traffic of emit_row, and since scalar loads return out of order every LDS wait became a
  // wait for the prefetched row tails of the NEXT step (a scalar-cache miss each, ~1 us).  `vz` is a zero the compiler
  // cannot see through.
  int vz;
  asm volatile("v_mov_b32 %0, 0" : "=v"(vz));
  struct Pre { float y, bl, a, b2, tx, oh, ol, g0, g1v; };
  auto load_e = [&](Pre &q, int t) {
    const float *er = erows + (long)t * L.ERS;
    q.y = er[hl];
    q.bl = er[UP + vz];
    const float *gr = grow + (long)t * V;  // gradient row of the same frame (the g (x) g term), first 64 tokens
    q.g0 = hl < V ? gr[hl] : 0.f;
    q.g1v = hl + W < V ? gr[hl + W] : 0.f;
  };
  auto load_fwd_row = [&](Pre &q, int trow) {  // beta row: slot i = states of l = i+1, l = 0 at the tail
    const float *r = brows + (long)trow * L.SRS;
    if constexpr (KIND == 0) { const float2 v = *reinterpret_cast<const float2 *>(r + 2 * hl); q.a = v.x; q.b2 = v.y; }
    else { q.a = r[hl]; q.b2 = NEG; }
    q.tx = r[tailpos + vz]; q.oh = r[tailpos + 2 + vz]; q.ol = r[tailpos + 3 + vz];
  };
  auto load_bwd_row = [&](Pre &q, int trow) {  // alpha row shifted: slot i = (state_c(l=i), open(l=i+1)), tail l = 32
    const float *r = arows + (long)trow * L.SRS;
    q.a = first ? r[tailpos] : r[PAIR * (hl - 1)];
    q.b2 = (KIND == 0) ? r[2 * hl + 1] : NEG;
    q.tx = r[PAIR * (W - 1) + vz]; q.oh = r[tailpos + 2 + vz]; q.ol = r[tailpos + 3 + vz];
  };

  float c, o, cx;
  double off;
  // the lattice steps of Side::step (ctc_fused_common.h) for one slot per lane and 32-lane halves
  auto step_fwd = [&](float y, float bl) {
    if constexpr (KIND == 0) {
      const float m = lse2(c, o);
      const float x = norep_next ? m : c;
      const float xin = prev_slot(x, cx);
      o = y + lse2(o, xin);
      c = bl + m;
    } else {
      const float pin = prev_slot(c, cx);
      c = lse2(bl + c, y + pin);
    }
    cx += bl;
  };
  auto step_bwd = [&](float y, float bl) {
    if constexpr (KIND == 0) {
      const float h = bl + c, ee = y + o;
      const float pn = lse2(h, ee);
      const float x = norep ? pn : h;
      cx += bl;
      const float xin = next_slot(x, cx);
      o = lse2(xin, ee);
      c = pn;
    } else {
      const float nx = next_slot(c, cx);
      c = lse2(bl + c, y + nx);
      cx += bl;
    }
  };
  auto renorm = [&]() {
    float mx = fmaxf(cx, c);
    if constexpr (KIND == 0) mx = fmaxf(mx, o);
    mx = half_max(mx);
    mx = (mx > NEG_THR) ? mx : 0.f;
    c -= mx; cx -= mx;
    if constexpr (KIND == 0) o -= mx;
    off += (double)mx;
  };
  // Output rows are staged in LDS and written SR rows (SR*V*4 bytes, contiguous) at a time: with one 128-byte store per
  // row and ~10^4 slabs in flight the HBM write stream had no page locality (2.5 TB/s where a plain fill reaches 6.8).
  auto flush = [&](int lo, int hi) {  // rows lo..hi of this half's slab, lo and hi in the same aligned group of SR rows
    wave_lds_fence();
    if (have) {
      const float *src = stage + (lo & (SR - 1)) * V;
      float *dst = out + (long)lo * V;
      const int n = (hi - lo + 1) * V;
      if (vec4) {
        for (int k = 4 * hl; k < n; k += 4 * W) nt_store(dst + k, *reinterpret_cast<const float4 *>(src + k));
      } else {
        for (int k = hl; k < n; k += W) nt_store(dst + k, src[k]);
      }
    }
    wave_lds_fence();
  };
  const float *grow_l = grow + hl;
  auto emit_row = [&](int t2, float s1, float s2, float s0, float gq0, float gq1) {
    float qb = (first ? fexp2(s0) : 0.f) + fexp2(s1);
    atomicAdd(reinterpret_cast<unsigned *>(abin), tofix(fexp2(s2)));
    asm(CTC_HALF_REDUCE_ASM("v_add_f32_dpp") : "+v"(qb));  // lanes 31 / 63 now hold their half's sum ...
    HST(5);
    if (last) ubin[p.blank] = tofix(qb);                    // ... and write it: no broadcast needed
    wave_lds_fence();
    float *srow = stage + (t2 & (SR - 1)) * V + hl;
    // base_loss.py:235-237 : -exp(.) + g (x) g ; the first two chunks use the prefetched gradient values
    if (hl < V) { srow[0] = g1 * gq0 - (float)ubin[hl] * 9.31322574615478515625e-10f; ubin[hl] = 0u; }
    if (hl + W < V) { srow[W] = g1 * gq1 - (float)ubin[hl + W] * 9.31322574615478515625e-10f; ubin[hl + W] = 0u; }
    for (int k2 = 2 * W; k2 < V; k2 += W) {
      if (k2 + hl < V) {
        srow[k2] = g1 * grow_l[(long)t2 * V + k2] - (float)ubin[k2 + hl] * 9.31322574615478515625e-10f;
        ubin[k2 + hl] = 0u;
      }
    }
    wave_lds_fence();
  };

  // =============== rows t2 > t1 : restricted alpha vector pushed forward ===============
  if (t1 + 1 < len) {
    {
      const float *r = arows + (long)t1 * L.SRS;  // alpha[t1]: slot i = states of l = i+1, l = 0 at the tail
      if constexpr (KIND == 0) { const float2 v = *reinterpret_cast<const float2 *>(r + 2 * hl); c = v.x; o = v.y; }
      else { c = r[hl]; o = NEG; }
      cx = r[tailpos];
      off = (double)r[tailpos + 2] + (double)r[tailpos + 3];
      Pre q1;
      load_e(q1, t1);
      step_fwd(sel ? q1.y : NEG, isblank ? q1.bl : NEG);  // alpha[t1+1] restricted to the states entered by k1 at t1
    }
    Pre cur, nxt;
    load_e(cur, t1 + 1);
    load_fwd_row(cur, t1 + 2);
    int lo = t1 + 1;
    for (int t2 = t1 + 1; t2 < len; ++t2) {
      const int tn = (t2 + 1 < len) ? t2 + 1 : t2;
      HST(0);
      load_e(nxt, tn);  // prefetch the next step while this one is processed
      load_fwd_row(nxt, tn + 1);
      for (int f = 0; f < f_per_row; ++f) fill_step();  // after the loads: a wait for them does not wait for these stores
      const float sc = (float)((double)cur.oh + (off - lp)) + cur.ol;
      HST(1);
      float s1, s2, s0;
      if constexpr (KIND == 0) {
        step_fwd(cur.y, cur.bl);
        s1 = c + cur.a + sc; s2 = o + cur.b2 + sc; s0 = cx + cur.tx + sc;
      } else {
        const float pin = prev_slot(c, cx);
        s1 = c + cur.bl + cur.a + sc; s2 = pin + cur.y + cur.a + sc; s0 = cx + cur.bl + cur.tx + sc;
        step_fwd(cur.y, cur.bl);
      }
      HST(2);
      emit_row(t2, s1, s2, s0, cur.g0, cur.g1v);
      HST(3);
      if (((t2 - t1) & 15) == 0) renorm();
      cur = nxt;
      if ((t2 & (SR - 1)) == SR - 1 || t2 == len - 1) { flush(lo, t2); lo = t2 + 1; }
      HST(4);
    }
  }

#ifdef CTC_HESS_STAMPS
  if (b == 0 && t1 == 10 && pair == 0 && lane == 0) {
    for (int i = 0; i < 6; ++i) dbg[i] = hst[i];
    dbg[6] = len - t1 - 1;
  }
#endif
  // =============== rows t2 < t1 : restricted beta vector pulled backward ===============
  if (t1 > 0) {
    {
      const float *r = brows + (long)(t1 + 1) * L.SRS;  // beta[t1+1] -> slot i = (state_c(l=i), open(l=i+1)), cx = l = 32
      c = first ? r[tailpos] : r[PAIR * (hl - 1)];
      o = (KIND == 0) ? r[2 * hl + 1] : NEG;
      cx = r[PAIR * (W - 1)];
      off = (double)r[tailpos + 2] + (double)r[tailpos + 3];
      Pre q1;
      load_e(q1, t1);
      step_bwd(sel ? q1.y : NEG, isblank ? q1.bl : NEG);  // beta-like vector at t1 of the paths that emit k1 at t1
    }
    Pre cur, nxt;
    load_e(cur, t1 - 1);
    load_bwd_row(cur, KIND == 0 ? t1 : t1 - 1);  // classic closes with alpha[t2+1], simplified with a[t2]
    int hi = t1 - 1;
    for (int t2 = t1 - 1; t2 >= 0; --t2) {
      const int tn = (t2 > 0) ? t2 - 1 : 0;
      load_e(nxt, tn);
      load_bwd_row(nxt, KIND == 0 ? tn + 1 : tn);
      for (int f = 0; f < f_per_row; ++f) fill_step();
      const float sc = (float)((double)cur.oh + (off - lp)) + cur.ol;
      float s1, s2, s0;
      if constexpr (KIND == 0) {
        s1 = c + cur.a + sc; s2 = o + cur.b2 + sc; s0 = cx + cur.tx + sc;
      } else {
        const float nx = next_slot(c, cx);
        s1 = c + cur.bl + cur.a + sc; s2 = cur.a + cur.y + nx + sc; s0 = cx + cur.bl + cur.tx + sc;
      }
      step_bwd(cur.y, cur.bl);
      emit_row(t2, s1, s2, s0, cur.g0, cur.g1v);
      if (((t1 - t2) & 15) == 0) renorm();
      cur = nxt;
      if ((t2 & (SR - 1)) == 0) { flush(t2, hi); hi = t2 - 1; }
    }
  }
  while (!f_done) fill_step();  // whatever the sweeps did not get to (short utterances)
}

static unsigned long long wg_stride(long nblk) {  // odd stride near nblk / golden ratio, coprime to nblk
  auto gcd = [](unsigned long long a, unsigned long long b) { while (b) { unsigned long long t = a % b; a = b; b = t; } return a; };
  if (nblk < 8) return 1;
  unsigned long long stride = (unsigned long long)((double)nblk * 0.6180339887) | 1ull;
  while (gcd(stride, (unsigned long long)nblk) != 1) stride += 2;
  return stride;
}

size_t hessian_extra_bytes(int kind, int B, int T, int V, int U) {
  (void)kind; (void)U;
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  // log-probability-space gradient g = -posterior, then the token order and present-token count of hess_plan_kernel
  return al((size_t)B * T * V * sizeof(float)) + al((size_t)B * V * sizeof(int)) + al((size_t)B * sizeof(int));
}

template <int KIND>
static hipError_t launch_pair(const Problem &p, const Layout &L, const float *emis, const float *alpha, const float *beta,
                              const double *logp, const float *g_lp, int *order, int *npres, float *hess,
                              unsigned long long *dbg, hipStream_t st) {
  hipLaunchKernelGGL(hess_plan_kernel, dim3(p.B), dim3(64), (size_t)p.V, st, p, order, npres);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  int wpb = 4;
  const size_t per_wave = (size_t)2 * (p.V + 4 + 8 * p.V) * 4;  // token rows + 8 staged output rows, per half
  while (wpb > 1 && wpb * per_wave > 64 * 1024) wpb >>= 1;
  const size_t shmem = wpb * per_wave;
  const long ntask = (long)p.B * p.T * pairs_per_frame(p.V, p.U);
  const long nblk = (ntask + wpb - 1) / wpb;
  if (nblk > 0x7fffffffL) return hipErrorInvalidValue;
  const unsigned long long stride = wg_stride(nblk);
  hipLaunchKernelGGL(hess_pair_kernel<KIND>, dim3((unsigned)nblk), dim3(64 * wpb), shmem, st, p, L, emis, alpha, beta, logp,
                     g_lp, order, npres, hess, wpb, stride, dbg);
  return hipGetLastError();
}

template <int KIND>
static hipError_t launch_slab(const Problem &p, const Layout &L, const float *emis, const float *alpha, const float *beta,
                              const double *logp, const float *g_lp, int *order, int *npres, float *hess, hipStream_t st) {
  hipLaunchKernelGGL(hess_plan_kernel, dim3(p.B), dim3(64), (size_t)p.V, st, p, order, npres);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  int wpb = 4;
  while (wpb > 1 && (size_t)wpb * (p.V + 4) * 4 > 64 * 1024) wpb >>= 1;
  const size_t shmem = (size_t)wpb * (p.V + 4) * 4;
  const long ntask = (long)p.B * p.T * p.V;
  const long nblk = (ntask + wpb - 1) / wpb;
  if (nblk > 0x7fffffffL) return hipErrorInvalidValue;
  const unsigned long long stride = wg_stride(nblk);
  dim3 grid((unsigned)nblk), block(64 * wpb);
  switch (L.NL) {
    case 1: hipLaunchKernelGGL((hess_slab_kernel<KIND, 1>), grid, block, shmem, st, p, L, emis, alpha, beta, logp, g_lp, order, hess, wpb, stride); break;
    case 2: hipLaunchKernelGGL((hess_slab_kernel<KIND, 2>), grid, block, shmem, st, p, L, emis, alpha, beta, logp, g_lp, order, hess, wpb, stride); break;
    case 4: hipLaunchKernelGGL((hess_slab_kernel<KIND, 4>), grid, block, shmem, st, p, L, emis, alpha, beta, logp, g_lp, order, hess, wpb, stride); break;
    case 8: hipLaunchKernelGGL((hess_slab_kernel<KIND, 8>), grid, block, shmem, st, p, L, emis, alpha, beta, logp, g_lp, order, hess, wpb, stride); break;
    case 16: hipLaunchKernelGGL((hess_slab_kernel<KIND, 16>), grid, block, shmem, st, p, L, emis, alpha, beta, logp, g_lp, order, hess, wpb, stride); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t run_hessian(const Problem &p, const Layout &L, char *ws, const float *g_lp, float *hess, hipStream_t st) {
  if ((long)p.B * p.T == 0) return hipSuccess;
  const float *emis = reinterpret_cast<const float *>(ws + L.off_emis);
  const float *alpha = reinterpret_cast<const float *>(ws + L.off_alpha);
  const float *beta = reinterpret_cast<const float *>(ws + L.off_beta);
  const double *logp = reinterpret_cast<const double *>(ws + L.off_logp);
  auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
  char *ex = ws + L.off_extra + al((size_t)p.B * p.T * p.V * sizeof(float));
  int *order = reinterpret_cast<int *>(ex);
  int *npres = reinterpret_cast<int *>(ex + al((size_t)p.B * p.V * sizeof(int)));
  // short labels: two slabs per wavefront (ctc_amd_debug_override("hessian", "slab") forces the one-slab kernel; the parity tests run both)
  if (p.U <= 32 && (size_t)2 * (p.V + 4 + 8 * p.V) * 4 <= 64 * 1024 && !g_force_hessian_slab) {
    unsigned long long *dbg = reinterpret_cast<unsigned long long *>(ws + L.off_dummy);  // diagnostic builds only
    return p.kind == 0 ? launch_pair<0>(p, L, emis, alpha, beta, logp, g_lp, order, npres, hess, dbg, st)
                       : launch_pair<1>(p, L, emis, alpha, beta, logp, g_lp, order, npres, hess, dbg, st);
  }
  return p.kind == 0 ? launch_slab<0>(p, L, emis, alpha, beta, logp, g_lp, order, npres, hess, st)
                     : launch_slab<1>(p, L, emis, alpha, beta, logp, g_lp, order, npres, hess, st);
}

}  // namespace ctc
