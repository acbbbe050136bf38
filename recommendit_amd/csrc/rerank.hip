// Diversified top-k: greedy Maximal Marginal Relevance (MMR) re-ranking of the ranked candidates, the optional last
// stage of the serving chain (it replaces rank_topk_kernel of features.hip when a diversity weight is asked for).
// The arithmetic is the contract of include/recommendit_hip.h (rihip_rank_topk_diverse): tests compare ids exactly
// against a sequential NumPy reference, so every f64 operation below is a single correctly rounded operation.
#include "common.h"
#include "recommendit_hip.h"
#include <math.h>
#include <stdlib.h>

// no FMA contraction anywhere in this file: dot products, the sums of squares and the objective are unfused
#pragma clang fp contract(off)

namespace {

constexpr int MMR_MAX_KC = 4096, MMR_MAX_W = 256, MMR_MAX_WAVES = 16;
constexpr size_t MMR_LDS_LIMIT = 160 * 1024;

enum : unsigned char { ST_OPEN = 0, ST_TAKEN = 1, ST_NAN = 2, ST_PAD = 3 };

// (obj, raw score, retrieval position): larger obj, then larger score (== : -0.0 ties +0.0), then smaller position.
// pos < 0 = no candidate.  obj is never NaN here (sanitised to -inf) and eligible scores are never NaN: a total order,
// so the result of a reduction does not depend on its shape.
struct Best { double obj, sc; int pos; };
__device__ __forceinline__ bool better(const Best& a, const Best& b) {
  if (a.pos < 0) return false;
  if (b.pos < 0) return true;
  if (a.obj != b.obj) return a.obj > b.obj;
  if (a.sc != b.sc) return a.sc > b.sc;
  return a.pos < b.pos;
}
__device__ __forceinline__ Best wave_best(Best v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Best u;
    u.obj = __shfl_xor(v.obj, o, 64);
    u.sc = __shfl_xor(v.sc, o, 64);
    u.pos = __shfl_xor(v.pos, o, 64);
    if (better(u, v)) v = u;
  }
  return v;
}

// One workgroup per request.  Candidate i of the request belongs to thread i % blockDim; its state lives in LDS:
//   sn[i] normalised relevance, raw[i] ranker score, nrm[i] |v_i| (0: no vector => sim 0), mm[i] running max sim,
//   st[i] open / taken / NaN score / padding.
// STAGED: the candidates' vectors are copied once into LDS, component-major (vec[j * kc + i]: lane i reads bank
// 2i mod 64, conflict free); otherwise every step reads them again from the table (L2).
template <bool STAGED>
__global__ __launch_bounds__(1024) void mmr_kernel(const double* __restrict__ scores, const int64_t* __restrict__ cand,
                                                   const float* __restrict__ rs, int kc, int k,
                                                   const double* __restrict__ V, int64_t n_rows, int64_t ld, int col0,
                                                   int w, double delta, int64_t* __restrict__ out_ids,
                                                   double* __restrict__ out_scores, float* __restrict__ out_rs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
  double* sn = reinterpret_cast<double*>(sm);
  double* raw = sn + kc;
  double* nrm = raw + kc;
  double* mm = nrm + kc;
  double* selv = mm + kc;                       // [w] vector of the item selected last
  double* red_d = selv + w;                     // [2 * MMR_MAX_WAVES] obj, score of each wave's best
  int* red_i = reinterpret_cast<int*>(red_d + 2 * MMR_MAX_WAVES);   // [MMR_MAX_WAVES] its position
  unsigned char* st = reinterpret_cast<unsigned char*>(red_i + MMR_MAX_WAVES);   // [kc rounded up to 8]
  double* vec = reinterpret_cast<double*>(st + ((kc + 7) & ~7));    // STAGED: [w * kc]

  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
  const int64_t* cq = cand + q * kc;
  const double* sq = scores + q * kc;
  const float* rq = rs + q * kc;
  const int kk = k < kc ? k : kc;               // slots that hold a candidate

  // ---- per-candidate set-up: class, norm (once per request), range of the finite eligible scores -----------------
  double lo = INFINITY, hi = -INFINITY;
  for (int i = tid; i < kc; i += nt) {
    const int64_t id = cq[i];
    const double s = sq[i];
    const unsigned char c = id < 0 ? ST_PAD : (s != s ? ST_NAN : ST_OPEN);
    double n = 0.0;
    if (c == ST_OPEN && id < n_rows) {
      const double* v = V + id * ld + col0;
      double ss = 0.0;
      for (int j = 0; j < w; ++j) {
        const double x = v[j];
        if (STAGED) vec[(size_t)j * kc + i] = x;
        ss = ss + x * x;
      }
      n = sqrt(ss);
    }
    if (c == ST_OPEN && s > -INFINITY && s < INFINITY) {
      lo = s < lo ? s : lo;
      hi = s > hi ? s : hi;
    }
    st[i] = c; raw[i] = s; nrm[i] = n; mm[i] = 0.0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double a = __shfl_xor(lo, o, 64), b = __shfl_xor(hi, o, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if (lane == 0) { red_d[2 * wave] = lo; red_d[2 * wave + 1] = hi; }
  __syncthreads();
  lo = INFINITY; hi = -INFINITY;
  for (int x = 0; x < nw; ++x) {
    const double a = red_d[2 * x], b = red_d[2 * x + 1];
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  const bool flat = !(hi > lo);                 // one distinct finite score, or none
  const double span = hi - lo;
  for (int i = tid; i < kc; i += nt) {
    const double s = raw[i];
    double r = 0.0;
    if (!flat && st[i] == ST_OPEN) r = s == INFINITY ? 1.0 : (s == -INFINITY ? 0.0 : (s - lo) / span);
    sn[i] = r;
  }
  const double one_minus = 1.0 - delta;
  __syncthreads();                              // red_d is rewritten below; sn / st are read by their owners only

  // ---- greedy selection ------------------------------------------------------------------------------------------
  double sel_norm = 0.0;
  int sel_pos = -1;
  int t = 0;
  for (; t < kk; ++t) {
    Best b;
    b.obj = -INFINITY; b.sc = 0.0; b.pos = -1;
    for (int i = tid; i < kc; i += nt) {
      if (st[i] != ST_OPEN) continue;
      double m = mm[i];
      if (t > 0) {
        double sim = 0.0;
        const double ni = nrm[i];
        if (ni != 0.0 && sel_norm != 0.0) {
          double dot = 0.0;
          if (STAGED) {
            for (int j = 0; j < w; ++j) dot = dot + vec[(size_t)j * kc + i] * selv[j];
          } else {
            const double* v = V + cq[i] * ld + col0;
            for (int j = 0; j < w; ++j) dot = dot + v[j] * selv[j];
          }
          sim = dot / (ni * sel_norm);
        }
        m = (t == 1 || sim > m) ? sim : m;
        mm[i] = m;
      }
      Best c;
      c.obj = one_minus * sn[i] - delta * m;
      if (c.obj != c.obj) c.obj = -INFINITY;    // non-finite vectors: never preferred, never a hole in the order
      c.sc = raw[i]; c.pos = i;
      if (better(c, b)) b = c;
    }
    b = wave_best(b);
    if (lane == 0) { red_d[2 * wave] = b.obj; red_d[2 * wave + 1] = b.sc; red_i[wave] = b.pos; }
    __syncthreads();
    b.obj = red_d[0]; b.sc = red_d[1]; b.pos = red_i[0];
    for (int x = 1; x < nw; ++x) {
      Best c;
      c.obj = red_d[2 * x]; c.sc = red_d[2 * x + 1]; c.pos = red_i[x];
      if (better(c, b)) b = c;
    }
    sel_pos = b.pos;                            // the same value in every thread
    if (sel_pos < 0) break;                     // the eligible candidates ran out (uniform: no barrier is skipped)
    sel_norm = nrm[sel_pos];
    if (sel_norm != 0.0 && t + 1 < kk) {        // broadcast its vector for the next step
      if (STAGED) {
        for (int j = tid; j < w; j += nt) selv[j] = vec[(size_t)j * kc + sel_pos];
      } else {
        const double* v = V + cq[sel_pos] * ld + col0;      // nrm != 0 => the id is inside the table
        for (int j = tid; j < w; j += nt) selv[j] = v[j];
      }
    }
    if (tid == 0) {
      st[sel_pos] = ST_TAKEN;
      out_ids[q * k + t] = cq[sel_pos];
      out_scores[q * k + t] = b.sc;
      out_rs[q * k + t] = rq[sel_pos];
    }
    __syncthreads();
  }

  // ---- the rest: NaN scores, then padding, each in retrieval order (rank_topk's order); then -1 / -inf -----------
  if (t < kk && wave == 0) {
    int slot = t;
    for (int pass = 0; pass < 2 && slot < kk; ++pass) {
      const unsigned char want = pass == 0 ? ST_NAN : ST_PAD;
      for (int base = 0; base < kc && slot < kk; base += 64) {
        const int i = base + lane;
        const bool hit = i < kc && st[i] == want;
        const unsigned long long mask = __ballot(hit);
        const int at = slot + __popcll(mask & ((1ull << lane) - 1ull));
        if (hit && at < kk) {
          out_ids[q * k + at] = cq[i];
          out_scores[q * k + at] = want == ST_NAN ? raw[i] : -INFINITY;
          out_rs[q * k + at] = rq[i];
        }
        slot += __popcll(mask);
      }
    }
  }
  for (int i = kk + tid; i < k; i += nt) {
    out_ids[q * k + i] = -1;
    out_scores[q * k + i] = -INFINITY;
    out_rs[q * k + i] = -INFINITY;
  }
}

size_t mmr_state_bytes(int kc, int w) {
  return (size_t)(4 * (size_t)kc + (size_t)w + 2 * MMR_MAX_WAVES) * sizeof(double) + MMR_MAX_WAVES * sizeof(int) +
         (((size_t)kc + 7) & ~(size_t)7);
}

}  // namespace

extern "C" int rihip_rank_topk_diverse(const double* scores, const int64_t* cand, const float* retrieval_scores, int64_t nq,
                                       int kc, int k, const double* vec_tab, int64_t n_rows, int64_t ld, int col0, int w,
                                       double diversity, int64_t* out_ids, double* out_scores, float* out_retrieval_scores,
                                       void* stream) {
  RIHIP_REQUIRE(scores && cand && retrieval_scores && vec_tab && out_ids && out_scores && out_retrieval_scores,
                RIHIP_ERR_ARG, "rank_topk_diverse: null pointer");
  RIHIP_REQUIRE(nq >= 0 && nq <= 0x7fffffffll && kc >= 1 && kc <= MMR_MAX_KC && k >= 1, RIHIP_ERR_ARG,
                "rank_topk_diverse: nq=%lld, kc=%d (1..%d), k=%d (>= 1)", (long long)nq, kc, MMR_MAX_KC, k);
  RIHIP_REQUIRE(w >= 1 && w <= MMR_MAX_W, RIHIP_ERR_ARG, "rank_topk_diverse: w=%d (1..%d)", w, MMR_MAX_W);
  RIHIP_REQUIRE(n_rows >= 0 && col0 >= 0 && ld >= (int64_t)col0 + w, RIHIP_ERR_ARG,
                "rank_topk_diverse: n_rows=%lld, columns %d..%d of a table of row stride %lld", (long long)n_rows, col0,
                col0 + w - 1, (long long)ld);
  RIHIP_REQUIRE(diversity >= 0.0 && diversity <= 1.0, RIHIP_ERR_ARG, "rank_topk_diverse: diversity=%g (0..1)", diversity);
  if (nq == 0) return RIHIP_OK;
  const size_t state = mmr_state_bytes(kc, w), staged = state + (size_t)kc * w * sizeof(double);
  // the candidates' vectors go to LDS when they fit beside the state; RIHIP_RERANK_STAGE=0 / 1 forces
  // the table (L2) path / the LDS path where it fits (measurements)
  bool stage = staged <= MMR_LDS_LIMIT;
  if (const char* e = getenv("RIHIP_RERANK_STAGE")) stage = stage && e[0] != '0';
  static bool granted = false;
  if (!granted) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mmr_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)MMR_LDS_LIMIT);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mmr_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)MMR_LDS_LIMIT);
    granted = true;
  }
  int nt = ((kc + 63) / 64) * 64;
  if (nt > 1024) nt = 1024;
  if (stage)
    hipLaunchKernelGGL(mmr_kernel<true>, dim3((unsigned)nq), dim3(nt), staged, (hipStream_t)stream, scores, cand,
                       retrieval_scores, kc, k, vec_tab, n_rows, ld, col0, w, diversity, out_ids, out_scores,
                       out_retrieval_scores);
  else
    hipLaunchKernelGGL(mmr_kernel<false>, dim3((unsigned)nq), dim3(nt), state, (hipStream_t)stream, scores, cand,
                       retrieval_scores, kc, k, vec_tab, n_rows, ld, col0, w, diversity, out_ids, out_scores,
                       out_retrieval_scores);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
