// Offline evaluation report on the GPU -- replaces the per-user Python loop of the reference's evaluate_model
// (src/evaluation/metrics.py:301-384) and the functions it calls (ndcg_at_k :20-69, recall_at_k :72-87,
// precision_at_k :90-99, mrr :104-118, coverage :143-165, intra_list_diversity :168-190), reading the device top-K
// id tensor that retrieval / rank_topk produce (int64 [n, K], -1 = padding, anywhere in a row).
//
// * eval_rank_kernel: one wave per user row.  Lanes walk the positions 64 at a time; a ballot/popcount prefix over
//   the >= 0 mask gives each entry's position in the compacted list; membership is a binary search in the user's
//   sorted, de-duplicated ground-truth segment (held one item per lane and searched with shuffles when it has <= 64
//   items, in global memory otherwise).  The hits of a chunk are then walked in position order by the whole wave,
//   lane j keeping the running DCG / hit count of the j-th requested k: every k in one pass, and each DCG is the same
//   left-to-right sum of the same host-built 1/log2(i+2) terms as the Python loop, so it is bit-identical.
//   Optionally marks the ids of scored rows in a byte-flag array (coverage).  HBM-bound on the id read.
// * eval_diversity_kernel: one wave per scored user: the first L listed items that have a vector, their norms, and
//   the L x L Gram matrix on the exact-f32 MFMA (v_mfma_f32_32x32x2_f32, upper-triangle 32x32 tiles), summing
//   1 - dot/(n_i n_j) over the pairs with both norms > 0.
// * eval_reduce_*: fixed-partition f64 sums (no float atomics): bitwise reproducible run to run.
// Everything is enqueued on the caller's stream with no host synchronisation (capturable in a hipGraph).
#include "common.h"
#include "recommendit_hip.h"

namespace {

constexpr int EVAL_MAX_K = 64;        // requested k values, one lane each
constexpr int EVAL_MAX_ROW = 16384;   // K
constexpr int EVAL_MAX_L = 512;       // diversity list length
constexpr int EVAL_MAX_G = 256;       // vector width
constexpr int EVAL_PARTS = 512;       // fixed partition of the per-user reductions

struct KList {
  int n;
  int kmax;
  int k[EVAL_MAX_K];
};

__device__ __forceinline__ uint64_t lanes_below(int lane) { return lane ? (~0ull >> (64 - lane)) : 0ull; }

template <bool COV>
__global__ __launch_bounds__(256) void eval_rank_kernel(const int64_t* __restrict__ rec, int64_t n, int K,
                                                        const int64_t* __restrict__ off,
                                                        const int64_t* __restrict__ items,
                                                        const int64_t* __restrict__ raw, KList kl,
                                                        const double* __restrict__ disc,
                                                        const double* __restrict__ idcg, double* __restrict__ vals,
                                                        double* __restrict__ rr, uint8_t* __restrict__ scored,
                                                        uint8_t* flags, int64_t n_id_space, int* err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  const uint64_t below = lanes_below(lane);
  int my_k = 0;  // the k of this lane's output slot (static indexing: no scratch copy of the argument block)
#pragma unroll
  for (int j = 0; j < EVAL_MAX_K; ++j)
    if (j == lane) my_k = kl.k[j];
  const int nk = kl.n;
  for (int64_t row = wave0; row < n; row += nwaves) {
    const int64_t nraw = raw[row];
    if (nraw <= 0) {  // no ground truth: skipped everywhere (metrics.py:320-322)
      if (lane < nk) {
        double* v = vals + (row * nk + lane) * 3;
        v[0] = 0.0; v[1] = 0.0; v[2] = 0.0;
      }
      if (lane == 0) { rr[row] = 0.0; scored[row] = 0; }
      continue;
    }
    const int64_t s0 = off[row];
    const int cnt = (int)(off[row + 1] - s0);
    const bool small = cnt <= 64;
    const int64_t segv = (small && lane < cnt) ? items[s0 + lane] : 0;
    int top = 1;
    while ((top << 1) <= cnt) top <<= 1;
    double dcg = 0.0;
    int hits = 0;
    int64_t first = -1, nvalid = 0;
    const int64_t* r = rec + row * (int64_t)K;
    for (int base0 = 0; base0 < K; base0 += 512) {
      int64_t ids[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int pos = base0 + c * 64 + lane;
        ids[c] = pos < K ? __builtin_nontemporal_load(r + pos) : -1;
      }
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        if (base0 + c * 64 >= K) break;
        const int64_t id = ids[c];
        const bool valid = id >= 0;
        const uint64_t vmask = __ballot(valid);
        const int64_t cpos = nvalid + __popcll(vmask & below);
        if (COV && valid) {
          if (id < n_id_space) flags[id] = 1;  // every writer stores 1: the race is benign
          else atomicOr(err, 1);
        }
        bool hit = false;
        if (small) {  // lower bound over the lane-held segment (uniform trip count, all lanes shuffle)
          int p = 0;
          for (int b = top; b > 0; b >>= 1) {
            const int q = p + b - 1;
            const int64_t v = __shfl(segv, q < 64 ? q : 63, 64);
            if (p + b <= cnt && v < id) p += b;
          }
          const int64_t v = __shfl(segv, p < 64 ? p : 63, 64);
          hit = valid && p < cnt && v == id;
        } else if (valid) {
          int64_t lo = s0, hi = s0 + cnt;
          while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (items[mid] < id) lo = mid + 1;
            else hi = mid;
          }
          hit = lo < s0 + cnt && items[lo] == id;
        }
        uint64_t hmask = __ballot(hit);
        while (hmask) {  // hits in position order: the Python loop's order of additions
          const int l = __ffsll((unsigned long long)hmask) - 1;
          const int p = __builtin_amdgcn_readlane((int)cpos, l);
          if (first < 0) first = p;
          if (p < my_k) { dcg += disc[p]; ++hits; }
          hmask &= hmask - 1;
        }
        nvalid += __popcll(vmask);
      }
      if (!COV && first >= 0 && nvalid >= kl.kmax) break;  // nothing further can change a value
    }
    if (lane < nk) {
      const int64_t m = nraw < (int64_t)my_k ? nraw : (int64_t)my_k;
      const double id = idcg[m];
      double* v = vals + (row * nk + lane) * 3;
      v[0] = id == 0.0 ? 0.0 : dcg / id;
      v[1] = (double)hits / (double)cnt;
      v[2] = my_k == 0 ? 0.0 : (double)hits / (double)my_k;
    }
    if (lane == 0) {
      rr[row] = first >= 0 ? 1.0 / (double)(first + 1) : 0.0;
      scored[row] = 1;
    }
  }
}

// one wave per block; grid-strided over users
template <bool VEC>
__global__ __launch_bounds__(64) void eval_diversity_kernel(const int64_t* __restrict__ rec, int64_t n, int K,
                                                            const uint8_t* __restrict__ scored, int L,
                                                            const float* __restrict__ tab, int64_t n_rows, int g,
                                                            const uint8_t* __restrict__ present,
                                                            double* __restrict__ div) {
  __shared__ int64_t sid[EVAL_MAX_L];
  __shared__ float snorm[EVAL_MAX_L];
  const int lane = threadIdx.x;
  const uint64_t below = lanes_below(lane);
  const int H = (g + 1) >> 1;  // k of the Gram split in two contiguous halves, one per lane half
  for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
    if (!scored[row]) {
      if (lane == 0) div[row] = 0.0;
      continue;
    }
    const int64_t* r = rec + row * (int64_t)K;
    int nvalid = 0, m = 0;
    for (int base = 0; base < K && nvalid < L; base += 64) {
      const int pos = base + lane;
      const int64_t id = pos < K ? r[pos] : -1;
      const bool valid = id >= 0;
      const uint64_t vmask = __ballot(valid);
      const int cpos = nvalid + __popcll(vmask & below);
      const bool pres = valid && cpos < L && id < n_rows && (present == nullptr || present[id]);
      const uint64_t pmask = __ballot(pres);
      if (pres) sid[m + __popcll(pmask & below)] = id;
      nvalid += __popcll(vmask);
      m += __popcll(pmask);
    }
    if (nvalid > L) nvalid = L;
    if (nvalid < 2 || m < 2) {  // fewer than 2 listed items, or fewer than 2 vectors (metrics.py:173-177)
      if (lane == 0) div[row] = 0.0;
      continue;
    }
    __syncthreads();
    for (int i = lane; i < m; i += 64) {
      const float* v = tab + sid[i] * (int64_t)g;
      float s = 0.f;
      for (int e = 0; e < g; ++e) s = fmaf(v[e], v[e], s);
      snorm[i] = sqrtf(s);
    }
    __syncthreads();
    const int nt = (m + 31) >> 5, h = lane >> 5;
    double sum = 0.0;
    int count = 0;
    for (int I = 0; I < nt; ++I) {
      const int ia = I * 32 + (lane & 31);
      const float* pa = ia < m ? tab + sid[ia] * (int64_t)g + h * H : nullptr;
      for (int J = I; J < nt; ++J) {
        const int jb = J * 32 + (lane & 31);
        const float* pb = jb < m ? tab + sid[jb] * (int64_t)g + h * H : nullptr;
        f32x16 acc = zero16();
        if (VEC) {  // g % 8 == 0: both halves are whole float4s; up to 8 of each in flight before their 32 MFMAs
          for (int s0 = 0; s0 < H; s0 += 32) {
            f32x4 a[8], b[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const int s = s0 + 4 * q;
              a[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
              b[q] = a[q];
              if (s < H) {
                if (pa) a[q] = *reinterpret_cast<const f32x4*>(pa + s);
                if (pb) b[q] = *reinterpret_cast<const f32x4*>(pb + s);
              }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              if (s0 + 4 * q >= H) break;
              acc = mfma32(a[q][0], b[q][0], acc);
              acc = mfma32(a[q][1], b[q][1], acc);
              acc = mfma32(a[q][2], b[q][2], acc);
              acc = mfma32(a[q][3], b[q][3], acc);
            }
          }
        } else {
          for (int s = 0; s < H; ++s) {
            const bool in = h * H + s < g;
            const float a = (pa && in) ? pa[s] : 0.f;
            const float b = (pb && in) ? pb[s] : 0.f;
            acc = mfma32(a, b, acc);
          }
        }
        const int j = J * 32 + (lane & 31);
        const float nj = j < m ? snorm[j] : 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int i = I * 32 + acc_row(q, lane);
          if (i < j && j < m) {
            const float ni = snorm[i];
            if (ni > 0.f && nj > 0.f) {
              const float c = acc[q] / (ni * nj);
              sum += (double)(1.f - c);
              ++count;
            }
          }
        }
      }
    }
    sum = wave_sum_d(sum);
    for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
    if (lane == 0) div[row] = count > 0 ? sum / (double)count : 0.0;
    __syncthreads();  // sid / snorm are rewritten by the next row
  }
}

// partials[b][c], c < 3*nk: sums of vals columns; then mrr, diversity, scored count -- over rows of part b
__global__ __launch_bounds__(256) void eval_reduce_partial(int64_t n, int nk, const double* __restrict__ vals,
                                                           const double* __restrict__ rr,
                                                           const double* __restrict__ div,
                                                           const uint8_t* __restrict__ scored,
                                                           double* __restrict__ partials) {
  __shared__ double sh[256];
  const int ncol = 3 * nk, W = ncol + 3, t = threadIdx.x;
  const int64_t per = (n + EVAL_PARTS - 1) / EVAL_PARTS;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = r0 + per < n ? r0 + per : n;
  double* out = partials + (int64_t)blockIdx.x * W;
  // per-k columns: thread t -> column t % ncol, row offset t / ncol
  const int rpi = 256 / ncol, c = t % ncol, sub = t / ncol;
  double acc = 0.0;
  if (sub < rpi)
    for (int64_t row = r0 + sub; row < r1; row += rpi) acc += vals[row * ncol + c];
  sh[t] = acc;
  __syncthreads();
  if (t < ncol) {
    double s = 0.0;
    for (int q = 0; q < rpi; ++q) s += sh[q * ncol + t];
    out[t] = s;
  }
  __syncthreads();
  // mrr, diversity, count: 256-way strided, then a fixed tree
  for (int w = 0; w < 3; ++w) {
    double a = 0.0;
    for (int64_t row = r0 + t; row < r1; row += 256) {
      if (w == 0) a += rr[row];
      else if (w == 1) a += div ? div[row] : 0.0;
      else a += scored[row] ? 1.0 : 0.0;
    }
    sh[t] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (t < o) sh[t] += sh[t + o];
      __syncthreads();
    }
    if (t == 0) out[ncol + w] = sh[0];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void eval_count_flags(const uint8_t* __restrict__ flags, int64_t n_bytes,
                                                        int64_t* __restrict__ partials) {
  __shared__ int64_t sh[256];
  const int t = threadIdx.x;
  const int64_t per = (n_bytes + EVAL_PARTS - 1) / EVAL_PARTS;
  const int64_t b0 = (int64_t)blockIdx.x * per, b1 = b0 + per < n_bytes ? b0 + per : n_bytes;
  int64_t c = 0;
  for (int64_t i = b0 + t; i < b1; i += 256) c += flags[i] != 0;
  sh[t] = c;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (t < o) sh[t] += sh[t + o];
    __syncthreads();
  }
  if (t == 0) partials[blockIdx.x] = sh[0];
}

// out: [3*nk means][mrr mean][diversity mean][n_scored][coverage][error bits]
__global__ __launch_bounds__(256) void eval_reduce_final(int nk, const double* __restrict__ partials,
                                                         const int64_t* __restrict__ cov_partials, int64_t catalog,
                                                         const int* __restrict__ err, double* __restrict__ out) {
  __shared__ double nsc;
  const int ncol = 3 * nk, W = ncol + 3, t = threadIdx.x;
  if (t == 0) {
    double s = 0.0;
    for (int b = 0; b < EVAL_PARTS; ++b) s += partials[(int64_t)b * W + ncol + 2];
    nsc = s;
  }
  __syncthreads();
  for (int c = t; c < ncol + 2; c += 256) {
    double s = 0.0;
    for (int b = 0; b < EVAL_PARTS; ++b) s += partials[(int64_t)b * W + c];
    out[c] = nsc > 0 ? s / nsc : 0.0;
  }
  if (t == 0) {
    out[ncol + 2] = nsc;
    double cov = 0.0;
    if (cov_partials && catalog > 0) {
      int64_t s = 0;
      for (int b = 0; b < EVAL_PARTS; ++b) s += cov_partials[b];
      cov = (double)s / (double)catalog;
    }
    out[ncol + 3] = cov;
    out[ncol + 4] = err ? (double)*err : 0.0;
  }
}

}  // namespace

extern "C" int rihip_eval_nparts(void) { return EVAL_PARTS; }

extern "C" int rihip_eval_topk(const int64_t* rec_ids, int64_t n, int K, const int64_t* gt_offsets,
                               const int64_t* gt_items, const int64_t* gt_raw, const int* k_values, int n_k,
                               const double* disc, const double* idcg, int n_tab, double* vals, double* rr,
                               uint8_t* scored, uint8_t* flags, int64_t n_id_space, int* err, void* stream) {
  RIHIP_REQUIRE(rec_ids && gt_offsets && gt_items && gt_raw && k_values && disc && idcg && vals && rr && scored,
                RIHIP_ERR_ARG, "eval_topk: null pointer");
  RIHIP_REQUIRE(n >= 0 && K >= 1 && K <= EVAL_MAX_ROW, RIHIP_ERR_ARG, "eval_topk: K=%d (1..%d)", K, EVAL_MAX_ROW);
  RIHIP_REQUIRE(n_k >= 1 && n_k <= EVAL_MAX_K, RIHIP_ERR_ARG, "eval_topk: %d k values (1..%d)", n_k, EVAL_MAX_K);
  RIHIP_REQUIRE(!flags || (err && n_id_space > 0), RIHIP_ERR_ARG, "eval_topk: coverage flags need err and n_id_space > 0");
  KList kl;
  kl.n = n_k;
  kl.kmax = 0;
  for (int j = 0; j < EVAL_MAX_K; ++j) kl.k[j] = 0;
  for (int j = 0; j < n_k; ++j) {
    RIHIP_REQUIRE(k_values[j] >= 0, RIHIP_ERR_ARG, "eval_topk: k=%d < 0", k_values[j]);
    kl.k[j] = k_values[j];
    if (k_values[j] > kl.kmax) kl.kmax = k_values[j];
  }
  // disc[p] is read for p < min(K, k), idcg[m] for m <= k
  RIHIP_REQUIRE(n_tab > kl.kmax && n_tab >= (K < kl.kmax ? K : kl.kmax), RIHIP_ERR_ARG,
                "eval_topk: discount table of %d entries, max k %d", n_tab, kl.kmax);
  if (flags) {
    RIHIP_CHECK_HIP(hipMemsetAsync(flags, 0, (size_t)n_id_space, (hipStream_t)stream));
    RIHIP_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int), (hipStream_t)stream));
  }
  if (n == 0) return RIHIP_OK;
  const int64_t nb = (n + 3) / 4;
  const unsigned grid = (unsigned)(nb < 8192 ? nb : 8192);
  if (flags)
    hipLaunchKernelGGL(eval_rank_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, rec_ids, n, K, gt_offsets,
                       gt_items, gt_raw, kl, disc, idcg, vals, rr, scored, flags, n_id_space, err);
  else
    hipLaunchKernelGGL(eval_rank_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, rec_ids, n, K,
                       gt_offsets, gt_items, gt_raw, kl, disc, idcg, vals, rr, scored, (uint8_t*)nullptr, (int64_t)0,
                       (int*)nullptr);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int rihip_eval_diversity(const int64_t* rec_ids, int64_t n, int K, const uint8_t* scored, int L,
                                    const float* item_vectors, int64_t n_rows, int g, const uint8_t* item_present,
                                    double* div, void* stream) {
  RIHIP_REQUIRE(rec_ids && scored && item_vectors && div, RIHIP_ERR_ARG, "eval_diversity: null pointer");
  RIHIP_REQUIRE(n >= 0 && K >= 1 && K <= EVAL_MAX_ROW, RIHIP_ERR_ARG, "eval_diversity: K=%d (1..%d)", K, EVAL_MAX_ROW);
  RIHIP_REQUIRE(L >= 0 && L <= EVAL_MAX_L, RIHIP_ERR_ARG, "eval_diversity: L=%d (0..%d)", L, EVAL_MAX_L);
  RIHIP_REQUIRE(g >= 1 && g <= EVAL_MAX_G && n_rows >= 0, RIHIP_ERR_ARG, "eval_diversity: g=%d (1..%d)", g, EVAL_MAX_G);
  if (n == 0) return RIHIP_OK;
  const unsigned grid = (unsigned)(n < 65536 ? n : 65536);
  const bool vec = (g % 8) == 0 && (reinterpret_cast<uintptr_t>(item_vectors) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(eval_diversity_kernel<true>, dim3(grid), dim3(64), 0, (hipStream_t)stream, rec_ids, n, K, scored,
                       L, item_vectors, n_rows, g, item_present, div);
  else
    hipLaunchKernelGGL(eval_diversity_kernel<false>, dim3(grid), dim3(64), 0, (hipStream_t)stream, rec_ids, n, K,
                       scored, L, item_vectors, n_rows, g, item_present, div);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int rihip_eval_reduce(int64_t n, int n_k, const double* vals, const double* rr, const double* div,
                                 const uint8_t* scored, const uint8_t* flags, int64_t n_id_space, int64_t catalog_size,
                                 const int* err, double* partials, int64_t* cov_partials, double* out, void* stream) {
  RIHIP_REQUIRE(vals && rr && scored && partials && out, RIHIP_ERR_ARG, "eval_reduce: null pointer");
  RIHIP_REQUIRE(n >= 0 && n_k >= 1 && n_k <= EVAL_MAX_K, RIHIP_ERR_ARG, "eval_reduce: n_k=%d (1..%d)", n_k, EVAL_MAX_K);
  RIHIP_REQUIRE(!flags || (cov_partials && n_id_space > 0), RIHIP_ERR_ARG, "eval_reduce: coverage needs cov_partials");
  hipLaunchKernelGGL(eval_reduce_partial, dim3(EVAL_PARTS), dim3(256), 0, (hipStream_t)stream, n, n_k, vals, rr, div,
                     scored, partials);
  RIHIP_CHECK_LAUNCH();
  if (flags) {
    hipLaunchKernelGGL(eval_count_flags, dim3(EVAL_PARTS), dim3(256), 0, (hipStream_t)stream, flags, n_id_space,
                       cov_partials);
    RIHIP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(eval_reduce_final, dim3(1), dim3(256), 0, (hipStream_t)stream, n_k, partials,
                     flags ? cov_partials : nullptr, catalog_size, err, out);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
