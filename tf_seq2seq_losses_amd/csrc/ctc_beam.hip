// Prefix beam search for both lattices, N-best: ctc_amd_beam_search (include/ctc_amd.h), DESIGN.md section 5.9.
//
// Two launches on the caller's stream:
//   row stage     frame-parallel over the B * T rows, in the shape of decode_rows_kernel (ctc_decode.hip): one wavefront per row,
//                 BEAM_G rows in flight per wavefront, the same access paths.  Per row: the float32 (max, sum of exp(x - max)),
//                 x[blank] and the K non-blank tokens with the largest values (ties to the lowest index) as a SET -- a radix
//                 select on the order-preserving integer image of the float32 values: at most 32 counting passes (ballot +
//                 popcount, no cross-lane reduction), fewer when a pass isolates exactly K elements.  Rows of up to 256 tokens stay
//                 in registers (the logits are read once); wider rows are read again per pass (from the caches).
//   search stage  one wavefront per utterance, sequential in t, one hypothesis per lane.  Masses are linear-domain float64 relative
//                 to the row maxima, rescaled by exact powers of two; prefixes are a trie in the workspace (node = (parent, token),
//                 node 1 + t * W + lane is made by frame t).  The W * (K + 1) candidates of a frame sit in LDS; a merge is found from
//                 the receiving side (a lane looks for the lane that holds its parent prefix, by the prefixes' 64-bit hashes: a
//                 prefix that left the beam and was made again has a new node but the same hash) and cancels the duplicate
//                 candidate; the W survivors are those above a threshold found by a radix select on the float64 bit patterns.
// No MFMA, no scratch.
#include "ctc_beam.h"

namespace ctc {
namespace {

constexpr int BEAM_G = 4;                        // rows in flight per wavefront of the row stage
constexpr int BEAM_WAVES = 4;                    // wavefronts per workgroup of the row stage
constexpr int BEAM_ROWS = BEAM_G * BEAM_WAVES;   // rows per workgroup
constexpr int BEAM_MAX_K = 32;                   // include/ctc_amd.h: top_k <= 32 (and beam_width <= 64: one hypothesis per lane)
constexpr int BEAM_MAX_V = 16384;                // CTC_AMD_MAX_V: one byte of LDS per token (token -> candidate index of the frame)
constexpr int REC_HEAD = 4;                      // floats in front of a row record: row max, score term, x[blank], unused
constexpr float FLT_LOWEST = -3.402823466e38f;

// Row record of frame (b, t), (REC_HEAD + 2 * K) words: [0] row max M, [1] the frame's term of the score (logits: -ln sum exp(x - M);
// log-probabilities: M), [2] x[blank], [4 .. 4 + K) the candidates' values, [4 + K .. 4 + 2K) their token indices.
__host__ __device__ inline int rec_words(int K) { return REC_HEAD + 2 * K; }

// elements k .. k+3 of a row as float32, non-temporal (the row_load4 of ctc_decode.hip, which is local to that unit)
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

// elements k .. k+3 through either access path: the same values in the same lanes (an element past V enters as -inf)
template <bool VEC>
__device__ __forceinline__ float4 row_chunk(const char *row, int k, int V, int dt) {
  const float ninf = -__builtin_inff();
  if (k >= V) return make_float4(ninf, ninf, ninf, ninf);
  if (VEC) return row_load4(row, k, dt);
  float4 v;
  v.x = row_load1(row, k, dt);
  v.y = k + 1 < V ? row_load1(row, k + 1, dt) : ninf;
  v.z = k + 2 < V ? row_load1(row, k + 2, dt) : ninf;
  v.w = k + 3 < V ? row_load1(row, k + 3, dt) : ninf;
  return v;
}

// Order-preserving image of a float32: a > b as floats <=> key(a) > key(b) as unsigned, equal floats give equal keys (-0 counts
// as +0).  A candidate's key is at least 1; 0 stands for "no candidate" (the blank, an element past V).
__device__ __forceinline__ unsigned order_key(float x, int idx, int V, int blank) {
  if (x == 0.f) x = 0.f;
  const unsigned u = __float_as_uint(x);
  const unsigned k = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return (idx >= V || idx == blank) ? 0u : (k ? k : 1u);
}

__device__ __forceinline__ int popc64(unsigned long long m) { return __builtin_popcountll(m); }
__device__ __forceinline__ unsigned long long ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// One row.  `chunk(k)` returns elements k .. k+3 (k = 4 * lane, + 256, ...): from registers when the row has one chunk per lane,
// from memory otherwise.  Every lane ends with the same M, S; the record is written by the lanes that hold the candidates.
template <int WRT, bool REG, class Chunk>
__device__ __forceinline__ void beam_row(const Chunk &chunk, const char *row, int V, int dt, int blank, int K, float *__restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  // every lane walks the same number of chunks (the ballots below need the whole wavefront); REG: one, known to the compiler
  const int nch = REG ? 1 : (V + 255) >> 8;
  // (max, sum of exp(x - max)) exactly as the greedy row stage takes them
  float m = -__builtin_inff(), s = 0.f;
  for (int ch = 0; ch < nch; ++ch) {
    const int k = ch * 256 + lane * 4;
    const float4 v = chunk(k);
    const float mo = fmaxf(m, FLT_LOWEST);
    m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    if (WRT == 0) {
      const float mn = fmaxf(m, FLT_LOWEST);
      s = s * fexp2((mo - mn) * LOG2E) +
          ((fexp2((v.x - mn) * LOG2E) + fexp2((v.y - mn) * LOG2E)) + (fexp2((v.z - mn) * LOG2E) + fexp2((v.w - mn) * LOG2E)));
    }
  }
  const float M = wave_max(m);
  float term = M;
  if (WRT == 0) {
    const float Mf = fmaxf(M, FLT_LOWEST);
    const float S = wave_sum(s * fexp2((fmaxf(m, FLT_LOWEST) - Mf) * LOG2E));
    term = M == -__builtin_inff() ? 0.f : (float)(-((double)flog2(S) * LN2_D));
  }
  if (lane == 0) {
    rec[0] = M;
    rec[1] = term;
    rec[2] = row_load1(row, blank, dt);
    rec[3] = 0.f;
  }
  if (K == 0) return;

  // the K-th largest key: the largest thr with count(key >= thr) >= K, bit by bit from the top
  auto count_ge = [&](unsigned thr) {
    int n = 0;
    for (int ch = 0; ch < nch; ++ch) {
    const int k = ch * 256 + lane * 4;
      const float4 v = chunk(k);
      n += popc64(ballot(order_key(v.x, k, V, blank) >= thr)) + popc64(ballot(order_key(v.y, k + 1, V, blank) >= thr)) +
           popc64(ballot(order_key(v.z, k + 2, V, blank) >= thr)) + popc64(ballot(order_key(v.w, k + 3, V, blank) >= thr));
    }
    return n;
  };
  unsigned thr = 0;
  bool exact = false;  // count(key >= thr) == K: no ties to break
  for (int bit = 31; bit >= 0; --bit) {
    const unsigned cand = thr | (1u << bit);
    const int n = count_ge(cand);
    if (n >= K) {
      thr = cand;
      if (n == K) { exact = true; break; }
    }
  }
  // keys above thr are all taken; of the keys equal to thr the ones with the lowest indices, until K are there
  int ties_wanted = 0;
  if (!exact) ties_wanted = K - (thr == 0xffffffffu ? 0 : count_ge(thr + 1u));
  float *const rv = rec + REC_HEAD;
  int *const ri = reinterpret_cast<int *>(rec + REC_HEAD + K);
  int filled = 0, ties_seen = 0;
  for (int ch = 0; ch < nch; ++ch) {
    const int k = ch * 256 + lane * 4;
    const float4 v = chunk(k);
    const float x[4] = {v.x, v.y, v.z, v.w};
    bool tie[4];
    unsigned long long tmask[4];
    int ties_below = 0, ties_chunk = 0;  // ties in lower lanes of this chunk (index order: lane-major, then the element)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tie[j] = !exact && order_key(x[j], k + j, V, blank) == thr;
      tmask[j] = ballot(tie[j]);
      ties_below += popc64(tmask[j] & below);
      ties_chunk += popc64(tmask[j]);
    }
    int own = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned key = order_key(x[j], k + j, V, blank);
      const bool take = (exact ? key >= thr : key > thr) || (tie[j] && ties_seen + ties_below + own < ties_wanted);
      own += tie[j];
      const unsigned long long tk = ballot(take);
      const int pos = filled + popc64(tk & below);
      if (take && pos < K) {  // (pos < K: always, for numbers; a guard for the stores)
        rv[pos] = x[j];
        ri[pos] = k + j;
      }
      filled += popc64(tk);
    }
    ties_seen += ties_chunk;
  }
}

// REG: V <= 256, the row is one float4 per lane and is read once; otherwise every pass reads it again.
template <int WRT, bool VEC, bool REG>
__global__ __launch_bounds__(64 * BEAM_WAVES) void beam_rows_kernel(const Problem p, long rows, int K, float *__restrict__ recs) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int T = p.T, V = p.V, dt = p.xdtype, blank = p.blank;
  const int esz = dt == 0 ? 4 : 2;
  const long r0 = ((long)blockIdx.x * BEAM_WAVES + wave) * BEAM_G;
  if (r0 >= rows) return;
  const char *row[BEAM_G];
  bool live[BEAM_G];
  const char *any = nullptr;
  {
    int b = (int)(r0 / T), t = (int)(r0 - (long)b * T);
#pragma unroll
    for (int g = 0; g < BEAM_G; ++g) {
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
  if (!any) return;
  const size_t rw = (size_t)rec_words(K);
  if (REG) {
    // the loads of the BEAM_G rows together (a dead row of the group reads a live one's data again, its results are dropped)
    float4 v[BEAM_G];
    const int k0 = lane * 4;
#pragma unroll
    for (int g = 0; g < BEAM_G; ++g) {
      v[g] = row_chunk<VEC>(live[g] ? row[g] : any, k0, V, dt);
    }
#pragma unroll
    for (int g = 0; g < BEAM_G; ++g) {
      if (!live[g]) continue;  // (uniform)
      const float4 vg = v[g];
      beam_row<WRT, true>([&](int) { return vg; }, row[g], V, dt, blank, K, recs + (size_t)(r0 + g) * rw);
    }
  } else {
#pragma unroll 1
    for (int g = 0; g < BEAM_G; ++g) {
      if (!live[g]) continue;
      const char *const r = row[g];
      beam_row<WRT, false>([&](int k) { return row_chunk<VEC>(r, k, V, dt); }, r, V, dt, blank, K, recs + (size_t)(r0 + g) * rw);
    }
  }
}

// ---- search stage ----

struct BeamShape {
  int W, K, nbest;   // K: the effective cut min(top_k, V - 1)
  long trie_nodes;   // nodes per utterance: 1 + W * T
};

__device__ __forceinline__ unsigned long long f64_bits(double x) { return (unsigned long long)__double_as_longlong(x); }

// hash of a prefix from its parent's and its last token (never 0, which stands for "no prefix")
__device__ __forceinline__ unsigned long long hash_step(unsigned long long h, int tok) {
  h = (h + (unsigned long long)(unsigned)tok + 1ull) * 0x9e3779b97f4a7c15ull;
  h ^= h >> 32;
  h *= 0xd6e8feb86659fd93ull;
  h ^= h >> 29;
  return h | 1ull;
}

__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
  asm(CTC_WAVE_REDUCE_ASM("v_max_u32_dpp") : "+v"(v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

template <int KIND>
__global__ __launch_bounds__(64) void beam_search_kernel(const Problem p, const BeamShape q, const float *__restrict__ recs,
                                                         int2 *__restrict__ trie_all, float *__restrict__ score,
                                                         int *__restrict__ decoded, int *__restrict__ decoded_length) {
  __shared__ double candm[(BEAM_MAX_K + 1) * 64];  // [c][lane]: c = 0 the prefix itself, c >= 1 its extension by candidate c
  __shared__ unsigned table32[BEAM_MAX_V / 4];     // token -> candidate index of this frame (a byte each), 0 = not a candidate
  __shared__ double em[BEAM_MAX_K + 1];            // emissions exp(x - M): [0] blank, [c] candidate c
  __shared__ int ctok[BEAM_MAX_K + 1];
  __shared__ double s_pb[64], s_pnb[64];
  __shared__ unsigned long long s_hash[64], s_phash[64];
  __shared__ int s_node[64], s_last[64], s_len[64];
  unsigned char *const table = reinterpret_cast<unsigned char *>(table32);

  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = p.T, V = p.V, blank = p.blank, W = q.W, K = q.K, nbest = q.nbest;
  const int Tb = frame_count(p, b);
  const unsigned long long below = (1ull << lane) - 1ull;
  const size_t rw = (size_t)rec_words(K);
  const float *const rec0 = recs + (size_t)b * T * rw;
  int2 *const trie = trie_all + (size_t)b * q.trie_nodes;

  for (int i = lane; i < (V + 3) / 4; i += 64) table32[i] = 0u;
  wave_lds_fence();

  // a lane's hypothesis: trie node, last token (-1: the empty prefix), length, hash of the prefix and of its parent prefix, masses
  // (simplified: pb is the one mass)
  int node = 0, last = -1, len = 0;
  unsigned long long hash = 0x243f6a8885a308d3ull, phash = 0ull;
  double pb = lane == 0 ? 1.0 : 0.0, pnb = 0.0;
  int alive = 1;        // hypotheses in lanes 0 .. alive - 1 (uniform)
  int scale = 0;        // true mass = mass * 2^scale (uniform)
  double terms = 0.0;   // sum of the frames' score terms (uniform)

  // the record of frame t as this lane reads it: the head in every lane, candidate `lane` in lanes 1 .. K
  struct Rec { float M, term, xb, val; int idx; };
  auto load_rec = [&](int t) {
    Rec r;
    const float *const rp = rec0 + (size_t)t * rw;
    r.M = rp[0]; r.term = rp[1]; r.xb = rp[2];
    r.val = 0.f; r.idx = 0;
    if (lane >= 1 && lane <= K) {
      r.val = rp[REC_HEAD + lane - 1];
      r.idx = reinterpret_cast<const int *>(rp)[REC_HEAD + K + lane - 1];
    }
    return r;
  };
  Rec next = {};
  if (Tb > 0) next = load_rec(0);

  for (int t = 0; t < Tb; ++t) {
    const Rec cur = next;
    if (t + 1 < Tb) next = load_rec(t + 1);  // in flight during this frame
    // emissions relative to the row maximum, float64 from the float32 values
    const int mytok = lane == 0 ? blank : cur.idx;
    if (lane <= K) {
      const float x = lane == 0 ? cur.xb : cur.val;
      double e = 0.0;
      if (cur.M != -__builtin_inff()) e = x == cur.M ? 1.0 : exp((double)x - (double)cur.M);
      em[lane] = e;
      ctok[lane] = mytok;
      if (lane >= 1 && (unsigned)mytok < (unsigned)V) table[mytok] = (unsigned char)lane;
    }
    terms += (double)cur.term;
    wave_lds_fence();

    const double tot = pb + pnb;
    const int ci = last >= 0 ? (int)table[last] : 0;  // the last label's candidate index, 0: outside the cut
    double keep_pb = tot * em[0], keep_pnb = 0.0;
    if (KIND == 0 && ci) keep_pnb = pnb * em[ci];
    for (int c = 1; c <= K; ++c) candm[c * 64 + lane] = ((KIND == 0 && c == ci) ? pb : tot) * em[c];
    wave_lds_fence();
    // the extension of the parent prefix by this prefix's last label IS this prefix: take its mass, cancel the duplicate
    int pl = -1;  // the lane that holds the parent prefix
    {
      const unsigned hlo = (unsigned)hash, hhi = (unsigned)(hash >> 32);
      for (int i = 0; i < alive; ++i) {
        const unsigned long long hi = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hhi, i) << 32) |
                                      (unsigned)__builtin_amdgcn_readlane((int)hlo, i);
        if (hi == phash) pl = i;
      }
    }
    if (lane < alive && pl >= 0 && ci) {
      const double m = candm[ci * 64 + pl];
      candm[ci * 64 + pl] = 0.0;
      if (KIND == 0) keep_pnb += m; else keep_pb += m;
    }
    candm[lane] = keep_pb + keep_pnb;
    wave_lds_fence();
    if (lane >= 1 && lane <= K && (unsigned)mytok < (unsigned)V) table[mytok] = 0;

    // threshold: the largest thr with count(bits >= thr) >= W (masses are >= 0, so their bit patterns order as integers)
    auto count_ge = [&](unsigned long long thr) {
      int n = 0;
      for (int c = 0; c <= K; ++c) n += popc64(ballot(f64_bits(candm[c * 64 + lane]) >= thr));
      return n;
    };
    unsigned long long thr = 1ull;  // (zero masses are dropped)
    bool exact = true;
    if (count_ge(1ull) > W) {
      thr = 0ull;
      exact = false;
      for (int bit = 62; bit >= 0; --bit) {
        const unsigned long long cand = thr | (1ull << bit);
        const int n = count_ge(cand);
        if (n >= W) {
          thr = cand;
          if (n == W) { exact = true; break; }
        }
      }
    }
    int ties_wanted = 0;
    if (!exact) ties_wanted = W - count_ge(thr + 1ull);

    // survivors move to lanes 0, 1, ... in the order (candidate index, lane)
    int filled = 0, ties_seen = 0;
    for (int c = 0; c <= K; ++c) {
      const double mass = candm[c * 64 + lane];
      const unsigned long long bits = f64_bits(mass);
      const bool tie = !exact && bits == thr;
      const unsigned long long tm = ballot(tie);
      const bool take = (exact ? bits >= thr : bits > thr) || (tie && ties_seen + popc64(tm & below) < ties_wanted);
      ties_seen += popc64(tm);
      const unsigned long long tk = ballot(take);
      const int d = filled + popc64(tk & below);
      filled += popc64(tk);
      if (take && d < W) {  // (d < W: always; a guard for the stores)
        if (c == 0) {
          s_node[d] = node; s_last[d] = last; s_len[d] = len; s_hash[d] = hash; s_phash[d] = phash;
          s_pb[d] = keep_pb; s_pnb[d] = keep_pnb;
        } else {
          const int nn = 1 + t * W + d;
          s_node[d] = nn; s_last[d] = ctok[c]; s_len[d] = len + 1; s_hash[d] = hash_step(hash, ctok[c]); s_phash[d] = hash;
          s_pb[d] = KIND == 0 ? 0.0 : mass; s_pnb[d] = KIND == 0 ? mass : 0.0;
          trie[nn] = make_int2(node, ctok[c]);
        }
      }
    }
    alive = filled < W ? filled : W;
    wave_lds_fence();
    if (lane < alive) {
      node = s_node[lane]; last = s_last[lane]; len = s_len[lane]; hash = s_hash[lane]; phash = s_phash[lane];
      pb = s_pb[lane]; pnb = s_pnb[lane];
    } else {
      node = 0; last = -1; len = 0; hash = 0ull; phash = 0ull; pb = 0.0; pnb = 0.0;
    }
    // keep the largest mass near 1: an exact power of two, accounted for in `scale`
    const unsigned hi = wave_max_u((unsigned)(f64_bits(pb + pnb) >> 32));
    const int ex = (int)((hi >> 20) & 0x7ffu);
    if (ex > 0 && ex < 0x7ff && (ex < 1023 - 32 || ex > 1023 + 32)) {
      const double f = __longlong_as_double((long long)(unsigned long long)(2046 - ex) << 52);  // 2^(1023 - ex)
      pb *= f; pnb *= f;
      scale += ex - 1023;
    }
    wave_lds_fence();
  }

  // final order: by total mass, descending (equal masses: by lane)
  const double tot = lane < alive ? pb + pnb : 0.0;
  const unsigned long long key = f64_bits(tot);
  const unsigned klo = (unsigned)key, khi = (unsigned)(key >> 32);
  int rank = 0;
  for (int i = 0; i < alive; ++i) {
    const unsigned long long ki = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)khi, i) << 32) |
                                  (unsigned)__builtin_amdgcn_readlane((int)klo, i);
    rank += (ki > key || (ki == key && i < lane)) ? 1 : 0;
  }
  // (the trie was written by other lanes of this wavefront: make it visible before it is walked)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  if (lane < nbest) s_len[lane] = 0;
  wave_lds_fence();
  const size_t out0 = (size_t)b * nbest;
  if (lane < alive && rank < nbest) {
    score[out0 + rank] = (float)(log(tot) + (double)scale * LN2_D + terms);
    decoded_length[out0 + rank] = len;
    s_len[rank] = len;
    int *const out = decoded + (out0 + rank) * T;
    int n = node;
    for (int i = len - 1; i >= 0; --i) {
      const int2 e = trie[n];
      out[i] = e.y;
      n = e.x;
    }
  }
  if (lane >= alive && lane < nbest) {  // missing hypotheses
    score[out0 + lane] = -__builtin_inff();
    decoded_length[out0 + lane] = 0;
  }
  wave_lds_fence();
  for (int r = 0; r < nbest; ++r) {
    int *const out = decoded + (out0 + r) * T;
    for (int i = s_len[r] + lane; i < T; i += 64) out[i] = -1;
  }
}

size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
size_t beam_rec_bytes(int B, int T, int K) { return align256((size_t)B * T * rec_words(K) * 4); }

}  // namespace

int beam_effective_k(int V, int top_k) { return top_k < V - 1 ? top_k : V - 1; }

size_t beam_workspace_bytes(int B, int T, int V, int beam_width, int top_k) {
  return beam_rec_bytes(B, T, beam_effective_k(V, top_k)) + align256((size_t)B * (1 + (size_t)beam_width * T) * sizeof(int2));
}

hipError_t run_beam(const Problem &p, int beam_width, int top_k, int nbest, char *ws, float *score, int *decoded, int *decoded_length,
                    hipStream_t st) {
  const int K = beam_effective_k(p.V, top_k);
  float *const recs = reinterpret_cast<float *>(ws);
  int2 *const trie = reinterpret_cast<int2 *>(ws + beam_rec_bytes(p.B, p.T, K));
  const long rows = (long)p.B * p.T;
  if (rows > 0) {
    const long blocks = (rows + BEAM_ROWS - 1) / BEAM_ROWS;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(64 * BEAM_WAVES);
    // 16-byte (float32) / 8-byte (16-bit types) row accesses when V, the strides and the base pointer allow them
    const bool vec = ((p.V | p.xsb | p.xst) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.logits) & (p.xdtype == 0 ? 15 : 7)) == 0;
    const bool reg = p.V <= 256;
#define CTC_BEAM_ROWS(WRT, VEC, REG) hipLaunchKernelGGL((beam_rows_kernel<WRT, VEC, REG>), grid, block, 0, st, p, rows, K, recs)
    if (p.wrt == 0) {
      if (vec) { if (reg) CTC_BEAM_ROWS(0, true, true); else CTC_BEAM_ROWS(0, true, false); }
      else { if (reg) CTC_BEAM_ROWS(0, false, true); else CTC_BEAM_ROWS(0, false, false); }
    } else {
      if (vec) { if (reg) CTC_BEAM_ROWS(1, true, true); else CTC_BEAM_ROWS(1, true, false); }
      else { if (reg) CTC_BEAM_ROWS(1, false, true); else CTC_BEAM_ROWS(1, false, false); }
    }
#undef CTC_BEAM_ROWS
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const BeamShape q{beam_width, K, nbest, 1 + (long)beam_width * p.T};
  if (p.kind == 0) hipLaunchKernelGGL((beam_search_kernel<0>), dim3(p.B), dim3(64), 0, st, p, q, recs, trie, score, decoded, decoded_length);
  else hipLaunchKernelGGL((beam_search_kernel<1>), dim3(p.B), dim3(64), 0, st, p, q, recs, trie, score, decoded, decoded_length);
  return hipGetLastError();
}

}  // namespace ctc
