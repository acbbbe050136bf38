// Training-serving skew on the GPU -- replaces the per-column host loop of the reference's
// detect_training_serving_skew and the histograms of kl_divergence_bins (src/evaluation/metrics.py:197-294) for two
// row-major samples that already live on the device (a training feature matrix, the serving feature log).
//
// Per column c (cols_a[c] of sample A, cols_b[c] of sample B; rows whose id is < 0 are left out):
// * skew_range_kernel: count of non-NaN and NaN values, min and max, compared in f64 (f32 -> f64 is exact).  Each
//   block owns a contiguous row range and a group of <= 256 columns; consecutive threads read consecutive columns of
//   consecutive rows (coalesced), and the block writes one partial per column to a fixed slab (no atomics).
// * skew_edges_kernel: one block per column folds the partials (min / max / counts: order-independent), then writes
//   the edges of np.linspace(min, max, n_bins + 1) bit for bit -- edge[i] = fl(fl(i * step) + min) with
//   step = (max - min) / n_bins, edge[n_bins] = max; fl(fl(i / n_bins) * delta) + min when step underflows to 0 --
//   without FMA contraction, and zeroes the column's counts.
// * skew_hist_kernel: np.histogram's array-bin rule: bin i holds edge[i] <= x < edge[i+1], the last bin also takes
//   x == edge[n_bins], NaN is never counted.  A guess (x - min) / step is corrected by compare-and-step against the
//   edges held in LDS; runs of equal bins are counted in a register, then into LDS-private u32 bins, and each block
//   adds its non-zero bins into the int64 totals with integer atomics (order-independent).
// * skew_finalize_kernel: one wave per column: density = n / diff(edge) / N, + epsilon, normalised, KL = sum(p *
//   log(p / q)); every sum is numpy's pairwise order for <= 128 terms.
// Everything is enqueued on the caller's stream with no host synchronisation (capturable in a hipGraph).
//
// The serving feature log: skew_log_append_kernel copies a batch of ranking-feature rows into a device ring at a
// device-resident cursor, and skew_log_advance_kernel moves the cursor (one thread), so a captured chain logs
// correctly on every replay.
#include <math.h>

#include "common.h"
#include "recommendit_hip.h"

// No FMA contraction anywhere below: the edges and the KL terms are numpy's separately rounded operations.
#pragma clang fp contract(off)

namespace {

constexpr int SKEW_THREADS = 256;
constexpr int SKEW_MAX_BINS = 128;
constexpr int SKEW_GMAX = 1024;              // blocks per sample and column group in the range / histogram passes
constexpr int SKEW_ROWS_PER_BLOCK = 4096;    // target rows per block
constexpr int SKEW_MAX_GROUP = 256;          // columns per block
constexpr int SKEW_LDS_BUDGET = 65536;       // histogram pass: edges + bounds + u32 bins of a column group

struct RangePart {
  int64_t cnt, nan;
  double lo, hi;
};
struct ColAux {
  double lo, hi;
  int64_t nan;
  int64_t ok;  // 1: both column indices are in range
};

template <typename T>
struct Sample {
  const T* x;
  int64_t n, ld;
  const int* cols;
  const int64_t* ids;
  int64_t chunk;  // rows per block
  int nblk;
};

template <typename T>
__device__ __forceinline__ double ld_f64(const T* p) { return (double)__builtin_nontemporal_load(p); }

__device__ __forceinline__ bool col_ok(int col, int64_t ld) { return col >= 0 && (int64_t)col < ld; }

template <typename T>
__device__ void range_body(const Sample<T> s, int nc, int c0, int cg, RangePart* __restrict__ part) {
  __shared__ RangePart sh[SKEW_THREADS];
  const int t = threadIdx.x, b = blockIdx.x;
  const int rpi = SKEW_THREADS / cg, j = t % cg, roff = t / cg;
  RangePart a{0, 0, INFINITY, -INFINITY};
  if (b < s.nblk && roff < rpi) {
    const int col = s.cols[c0 + j];
    if (col_ok(col, s.ld)) {
      const int64_t r0 = (int64_t)b * s.chunk, r1 = r0 + s.chunk < s.n ? r0 + s.chunk : s.n;
      auto acc = [&](double x, bool keep) {
        if (!keep) return;
        if (x != x) {
          ++a.nan;
        } else {
          ++a.cnt;
          a.lo = x < a.lo ? x : a.lo;
          a.hi = x > a.hi ? x : a.hi;
        }
      };
      int64_t r = r0 + roff;
      for (; r + 3 * rpi < r1; r += 4 * rpi) {
        double v[4];
        bool keep[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ld_f64(s.x + (r + u * rpi) * s.ld + col);
#pragma unroll
        for (int u = 0; u < 4; ++u) keep[u] = !s.ids || s.ids[r + u * rpi] >= 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) acc(v[u], keep[u]);
      }
      for (; r < r1; r += rpi) acc(ld_f64(s.x + r * s.ld + col), !s.ids || s.ids[r] >= 0);
    }
  }
  sh[t] = a;
  __syncthreads();
  if (b < s.nblk && t < cg) {
    RangePart m = sh[t];
    for (int q = 1; q < rpi; ++q) {
      const RangePart o = sh[q * cg + t];
      m.cnt += o.cnt;
      m.nan += o.nan;
      m.lo = o.lo < m.lo ? o.lo : m.lo;
      m.hi = o.hi > m.hi ? o.hi : m.hi;
    }
    part[(int64_t)b * nc + c0 + t] = m;
  }
}

// grid (max blocks, 2 samples, column groups); part [2][SKEW_GMAX][nc]
template <typename TA, typename TB>
__global__ __launch_bounds__(SKEW_THREADS) void skew_range_kernel(const Sample<TA> sa, const Sample<TB> sb, int nc,
                                                                  int cg, RangePart* __restrict__ part) {
  const int c0 = blockIdx.z * cg, g = nc - c0 < cg ? nc - c0 : cg;
  if (blockIdx.y == 0)
    range_body(sa, nc, c0, g, part);
  else
    range_body(sb, nc, c0, g, part + (int64_t)SKEW_GMAX * nc);
}

// one block per column
__global__ __launch_bounds__(SKEW_THREADS) void skew_edges_kernel(const RangePart* __restrict__ part, int nblk_a,
                                                                  int nblk_b, const int* __restrict__ cols_a,
                                                                  int64_t lda, const int* __restrict__ cols_b,
                                                                  int64_t ldb, int nc, int nb, ColAux* __restrict__ aux,
                                                                  int64_t* __restrict__ valid,
                                                                  double* __restrict__ edges,
                                                                  int64_t* __restrict__ counts) {
  __shared__ RangePart sh[2][SKEW_THREADS];
  __shared__ double s_lo, s_step, s_delta;
  __shared__ int s_zero_step;
  const int c = blockIdx.x, t = threadIdx.x;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int nblk = s ? nblk_b : nblk_a;
    const RangePart* p = part + (int64_t)s * SKEW_GMAX * nc + c;
    RangePart m{0, 0, INFINITY, -INFINITY};
    for (int b = t; b < nblk; b += SKEW_THREADS) {
      const RangePart o = p[(int64_t)b * nc];
      m.cnt += o.cnt;
      m.nan += o.nan;
      m.lo = o.lo < m.lo ? o.lo : m.lo;
      m.hi = o.hi > m.hi ? o.hi : m.hi;
    }
    sh[s][t] = m;
  }
  __syncthreads();
  for (int w = SKEW_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        RangePart& m = sh[s][t];
        const RangePart o = sh[s][t + w];
        m.cnt += o.cnt;
        m.nan += o.nan;
        m.lo = o.lo < m.lo ? o.lo : m.lo;
        m.hi = o.hi > m.hi ? o.hi : m.hi;
      }
    }
    __syncthreads();
  }
  if (t == 0) {
    const RangePart a = sh[0][0], b = sh[1][0];
    const double lo = a.lo < b.lo ? a.lo : b.lo, hi = a.hi > b.hi ? a.hi : b.hi;
    ColAux x;
    x.lo = lo;
    x.hi = hi;
    x.nan = a.nan + b.nan;
    x.ok = col_ok(cols_a[c], lda) && col_ok(cols_b[c], ldb);
    aux[c] = x;
    valid[2 * c] = a.cnt;
    valid[2 * c + 1] = b.cnt;
    // np.linspace(lo, hi, nb + 1): delta, step = delta / div, y = arange * step (or (arange / div) * delta when step
    // == 0), y += start, y[-1] = stop
    const double delta = hi - lo;
    const double step = delta / (double)nb;
    s_lo = lo;
    s_delta = delta;
    s_step = step;
    s_zero_step = step == 0.0;
  }
  __syncthreads();
  double* e = edges + (int64_t)c * (nb + 1);
  for (int i = t; i <= nb; i += SKEW_THREADS) {
    double y;
    if (i == nb)
      y = sh[1][0].hi > sh[0][0].hi ? sh[1][0].hi : sh[0][0].hi;
    else if (s_zero_step)
      y = ((double)i / (double)nb) * s_delta + s_lo;
    else
      y = (double)i * s_step + s_lo;
    e[i] = y;
  }
  for (int i = t; i < 2 * nb; i += SKEW_THREADS) counts[(int64_t)c * 2 * nb + i] = 0;
}

// dynamic LDS of a histogram block: edges [cg][nb+1] f64, lo [cg] f64, step [cg] f64 (< 0: column not binned),
// bins [cg][nb] u32
__host__ __device__ inline int64_t hist_col_bytes(int nb) { return (int64_t)(nb + 1) * 8 + 16 + (int64_t)nb * 4; }

template <typename T>
__device__ void hist_body(const Sample<T> s, int side, int c0, int cg, int nb, const double* __restrict__ edges,
                          const ColAux* __restrict__ aux, int64_t* __restrict__ counts, unsigned char* lds) {
  double* e = reinterpret_cast<double*>(lds);
  double* lo = e + (int64_t)cg * (nb + 1);
  double* step = lo + cg;
  unsigned* bins = reinterpret_cast<unsigned*>(step + cg);
  const int t = threadIdx.x, b = blockIdx.x;
  for (int i = t; i < cg * (nb + 1); i += SKEW_THREADS) e[i] = edges[(int64_t)c0 * (nb + 1) + i];
  for (int i = t; i < cg * nb; i += SKEW_THREADS) bins[i] = 0u;
  for (int i = t; i < cg; i += SKEW_THREADS) {
    const ColAux a = aux[c0 + i];
    const bool binned = a.ok && a.lo < a.hi && isfinite(a.lo) && isfinite(a.hi);
    lo[i] = a.lo;
    step[i] = binned ? (a.hi - a.lo) / (double)nb : -1.0;
  }
  __syncthreads();
  const int rpi = SKEW_THREADS / cg, j = t % cg, roff = t / cg;
  if (b < s.nblk && roff < rpi && step[j] >= 0.0) {
    const int col = s.cols[c0 + j];
    const double* ej = e + (int64_t)j * (nb + 1);
    const double lj = lo[j], sj = step[j];
    unsigned* bj = bins + j * nb;
    int cur = 0;
    unsigned run = 0;
    auto put = [&](double x, bool keep) {
      if (!keep || x != x) return;
      const double q = (x - lj) / sj;  // only a guess: the edges decide
      int g = q >= 0.0 ? (q < (double)nb ? (int)q : nb - 1) : 0;
      while (g > 0 && x < ej[g]) --g;
      while (g < nb - 1 && x >= ej[g + 1]) ++g;
      if (g == cur) {
        ++run;
      } else {
        if (run) atomicAdd(bj + cur, run);
        cur = g;
        run = 1;
      }
    };
    const int64_t r0 = (int64_t)b * s.chunk, r1 = r0 + s.chunk < s.n ? r0 + s.chunk : s.n;
    int64_t r = r0 + roff;
    for (; r + 3 * rpi < r1; r += 4 * rpi) {
      double v[4];
      bool keep[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = ld_f64(s.x + (r + u * rpi) * s.ld + col);
#pragma unroll
      for (int u = 0; u < 4; ++u) keep[u] = !s.ids || s.ids[r + u * rpi] >= 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) put(v[u], keep[u]);
    }
    for (; r < r1; r += rpi) put(ld_f64(s.x + r * s.ld + col), !s.ids || s.ids[r] >= 0);
    if (run) atomicAdd(bj + cur, run);
  }
  __syncthreads();
  if (b < s.nblk) {
    for (int i = t; i < cg * nb; i += SKEW_THREADS) {
      const unsigned v = bins[i];
      if (v) {
        const int jj = i / nb, k = i - jj * nb;
        atomicAdd(reinterpret_cast<unsigned long long*>(counts + ((int64_t)(c0 + jj) * 2 + side) * nb + k),
                  (unsigned long long)v);
      }
    }
  }
}

// grid (max blocks, 2 samples, column groups)
template <typename TA, typename TB>
__global__ __launch_bounds__(SKEW_THREADS) void skew_hist_kernel(const Sample<TA> sa, const Sample<TB> sb, int nc,
                                                                 int cg, int nb, const double* __restrict__ edges,
                                                                 const ColAux* __restrict__ aux,
                                                                 int64_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char skew_lds[];
  const int c0 = blockIdx.z * cg, g = nc - c0 < cg ? nc - c0 : cg;
  if (blockIdx.y == 0)
    hist_body(sa, 0, c0, g, nb, edges, aux, counts, skew_lds);
  else
    hist_body(sb, 1, c0, g, nb, edges, aux, counts, skew_lds);
}

// numpy's pairwise summation (add.reduce of a contiguous float64 array) for n <= 128 terms
__device__ double np_sum(const double* a, int n) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += a[i];
    return r;
  }
  double r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = a[k];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] += a[i + k];
  }
  double res = (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])));
  for (; i < n; ++i) res += a[i];
  return res;
}

// one wave per column
__global__ __launch_bounds__(64) void skew_finalize_kernel(const ColAux* __restrict__ aux,
                                                           const int64_t* __restrict__ valid,
                                                           const double* __restrict__ edges,
                                                           const int64_t* __restrict__ counts, int nb, double eps,
                                                           int64_t min_count, int propagate_nan,
                                                           double* __restrict__ kl, int* __restrict__ status) {
  __shared__ double p[SKEW_MAX_BINS], q[SKEW_MAX_BINS];
  __shared__ double s_sp, s_sq;
  const int c = blockIdx.x, t = threadIdx.x;
  const ColAux a = aux[c];
  const int64_t na = valid[2 * c], nbv = valid[2 * c + 1];
  int st;
  if (!a.ok)
    st = RIHIP_SKEW_BAD_COLUMN;
  else if (na < min_count || nbv < min_count)
    st = RIHIP_SKEW_TOO_FEW;
  else if (propagate_nan && a.nan > 0)
    st = RIHIP_SKEW_NAN;
  else if (a.lo == a.hi)
    st = RIHIP_SKEW_CONSTANT;
  else if (!isfinite(a.lo) || !isfinite(a.hi))
    st = RIHIP_SKEW_INFINITE;
  else
    st = RIHIP_SKEW_OK;
  if (st != RIHIP_SKEW_OK) {
    if (t == 0) {
      kl[c] = st == RIHIP_SKEW_CONSTANT ? 0.0 : NAN;
      status[c] = st;
    }
    return;
  }
  const double* e = edges + (int64_t)c * (nb + 1);
  const int64_t* ca = counts + (int64_t)c * 2 * nb;
  const int64_t* cb = ca + nb;
  const double Na = (double)na, Nb = (double)nbv;
  for (int i = t; i < nb; i += 64) {
    const double db = e[i + 1] - e[i];
    p[i] = (double)ca[i] / db / Na + eps;
    q[i] = (double)cb[i] / db / Nb + eps;
  }
  __syncthreads();
  if (t == 0) {
    s_sp = np_sum(p, nb);
    s_sq = np_sum(q, nb);
  }
  __syncthreads();
  const double sp = s_sp, sq = s_sq;
  __syncthreads();
  for (int i = t; i < nb; i += 64) {
    const double pi = p[i] / sp, qi = q[i] / sq;
    p[i] = pi * log(pi / qi);
  }
  __syncthreads();
  if (t == 0) {
    kl[c] = np_sum(p, nb);
    status[c] = RIHIP_SKEW_OK;
  }
}

// ---- serving feature log ----
// rows r >= n - R of the batch (the newest R) go to slot (cursor + r) % R.  Each block copies SKEW_LOG_ROWS
// consecutive rows, V floats per thread; the slot of its first row is the only 64-bit modulo.
constexpr int SKEW_LOG_ROWS = 64;
template <int V>
__global__ __launch_bounds__(256) void skew_log_append_kernel(const float* __restrict__ X, int64_t n, int nf,
                                                              const int64_t* __restrict__ uid,
                                                              const int64_t* __restrict__ cand, int kc,
                                                              float* __restrict__ ring, int64_t* __restrict__ ring_uid,
                                                              int64_t* __restrict__ ring_iid, int64_t R,
                                                              const int64_t* __restrict__ cursor) {
  typedef float vec_t __attribute__((ext_vector_type(V)));
  const int64_t first = n > R ? n - R : 0;
  const int64_t rb = first + (int64_t)blockIdx.x * SKEW_LOG_ROWS;
  if (rb >= n) return;
  const int rows = n - rb < SKEW_LOG_ROWS ? (int)(n - rb) : SKEW_LOG_ROWS;
  const int64_t slot0 = (cursor[0] + rb) % R;
  const unsigned vpr = (unsigned)(nf / V), nvec = (unsigned)rows * vpr;
  for (unsigned li = threadIdx.x; li < nvec; li += 256) {
    const unsigned lr = li / vpr, k = li - lr * vpr;
    int64_t slot = slot0 + lr;
    if (slot >= R) slot -= R;
    const int64_t r = rb + lr;
    *reinterpret_cast<vec_t*>(ring + slot * nf + k * V) = *reinterpret_cast<const vec_t*>(X + r * nf + k * V);
  }
  for (int lr = threadIdx.x; lr < rows; lr += 256) {
    int64_t slot = slot0 + lr;
    if (slot >= R) slot -= R;
    const int64_t r = rb + lr;
    ring_uid[slot] = uid[r / kc];
    ring_iid[slot] = cand[r];
  }
}

// cursor[1] = where this batch started (the rewind mark), cursor[0] += n
__global__ void skew_log_advance_kernel(int64_t* cursor, int64_t n) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    const int64_t c = cursor[0];
    cursor[1] = c;
    cursor[0] = c + n;
  }
}

__global__ void skew_log_rewind_kernel(int64_t* cursor) {
  if (threadIdx.x == 0 && blockIdx.x == 0) cursor[0] = cursor[1];
}

struct Plan {
  int cg_range, ng_range, cg_hist, ng_hist;
  int64_t chunk_a, chunk_b;
  int nblk_a, nblk_b;
};

void plan_rows(int64_t n, int64_t* chunk, int* nblk) {
  int64_t g = (n + SKEW_ROWS_PER_BLOCK - 1) / SKEW_ROWS_PER_BLOCK;
  if (g < 1) g = 1;
  if (g > SKEW_GMAX) g = SKEW_GMAX;
  int64_t c = (n + g - 1) / g;
  if (c < 1) c = 1;
  *chunk = c;
  *nblk = (int)((n + c - 1) / c);
}

template <typename TA, typename TB>
int launch_passes(const Plan& pl, const void* A, int64_t na, int64_t lda, const int* cols_a, const int64_t* ids_a,
                  const void* B, int64_t nb_rows, int64_t ldb, const int* cols_b, const int64_t* ids_b, int nc,
                  int n_bins, RangePart* part, ColAux* aux, int64_t* counts, double* edges, int64_t* valid,
                  hipStream_t st) {
  Sample<TA> sa{static_cast<const TA*>(A), na, lda, cols_a, ids_a, pl.chunk_a, pl.nblk_a};
  Sample<TB> sb{static_cast<const TB*>(B), nb_rows, ldb, cols_b, ids_b, pl.chunk_b, pl.nblk_b};
  const int gmax = pl.nblk_a > pl.nblk_b ? pl.nblk_a : pl.nblk_b;
  const unsigned gx = (unsigned)(gmax > 1 ? gmax : 1);
  hipLaunchKernelGGL((skew_range_kernel<TA, TB>), dim3(gx, 2, pl.ng_range), dim3(SKEW_THREADS), 0, st, sa, sb, nc,
                     pl.cg_range, part);
  RIHIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(skew_edges_kernel, dim3(nc), dim3(SKEW_THREADS), 0, st, part, pl.nblk_a, pl.nblk_b, cols_a, lda,
                     cols_b, ldb, nc, n_bins, aux, valid, edges, counts);
  RIHIP_CHECK_LAUNCH();
  const size_t lds = (size_t)(pl.cg_hist * hist_col_bytes(n_bins));
  hipLaunchKernelGGL((skew_hist_kernel<TA, TB>), dim3(gx, 2, pl.ng_hist), dim3(SKEW_THREADS), lds, st, sa, sb, nc,
                     pl.cg_hist, n_bins, edges, aux, counts);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

}  // namespace

extern "C" int64_t rihip_skew_workspace_bytes(int nc) {
  if (nc < 1) return 0;
  return align256((int64_t)2 * SKEW_GMAX * nc * (int64_t)sizeof(RangePart)) + align256((int64_t)nc * sizeof(ColAux));
}

extern "C" int rihip_skew_compute(const void* A, int a_f64, int64_t na, int64_t lda, const int* cols_a,
                                  const int64_t* ids_a, const void* B, int b_f64, int64_t nb, int64_t ldb,
                                  const int* cols_b, const int64_t* ids_b, int nc, int n_bins, double epsilon,
                                  int64_t min_count, int propagate_nan, void* workspace, int64_t workspace_bytes,
                                  int64_t* counts, double* edges, int64_t* valid, double* kl, int* status,
                                  void* stream) {
  RIHIP_REQUIRE(n_bins >= 1 && n_bins <= SKEW_MAX_BINS, RIHIP_ERR_ARG, "skew: n_bins=%d (1..%d)", n_bins,
                SKEW_MAX_BINS);
  RIHIP_REQUIRE(nc >= 1, RIHIP_ERR_ARG, "skew: nc=%d (>= 1)", nc);
  RIHIP_REQUIRE(A && B && cols_a && cols_b && workspace && counts && edges && valid && kl && status, RIHIP_ERR_ARG,
                "skew: null pointer");
  RIHIP_REQUIRE(na >= 0 && nb >= 0 && lda >= 1 && ldb >= 1, RIHIP_ERR_ARG, "skew: bad shape na=%lld nb=%lld",
                (long long)na, (long long)nb);
  RIHIP_REQUIRE(na <= (int64_t)SKEW_GMAX << 31 && nb <= (int64_t)SKEW_GMAX << 31, RIHIP_ERR_ARG,
                "skew: too many rows");
  RIHIP_REQUIRE(workspace_bytes >= rihip_skew_workspace_bytes(nc), RIHIP_ERR_ARG, "skew: workspace of %lld bytes < %lld",
                (long long)workspace_bytes, (long long)rihip_skew_workspace_bytes(nc));
  RIHIP_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, RIHIP_ERR_ARG, "skew: workspace not 16-B aligned");
  hipStream_t st = (hipStream_t)stream;
  Plan pl;
  pl.cg_range = nc < SKEW_MAX_GROUP ? nc : SKEW_MAX_GROUP;
  pl.ng_range = (nc + pl.cg_range - 1) / pl.cg_range;
  int cg = (int)(SKEW_LDS_BUDGET / hist_col_bytes(n_bins));
  if (cg > SKEW_MAX_GROUP) cg = SKEW_MAX_GROUP;
  if (cg > nc) cg = nc;
  pl.cg_hist = cg;
  pl.ng_hist = (nc + cg - 1) / cg;
  plan_rows(na, &pl.chunk_a, &pl.nblk_a);
  plan_rows(nb, &pl.chunk_b, &pl.nblk_b);
  RangePart* part = static_cast<RangePart*>(workspace);
  ColAux* aux = reinterpret_cast<ColAux*>(static_cast<char*>(workspace) +
                                          align256((int64_t)2 * SKEW_GMAX * nc * (int64_t)sizeof(RangePart)));
  int rc;
  if (a_f64 && b_f64)
    rc = launch_passes<double, double>(pl, A, na, lda, cols_a, ids_a, B, nb, ldb, cols_b, ids_b, nc, n_bins, part, aux,
                                       counts, edges, valid, st);
  else if (a_f64)
    rc = launch_passes<double, float>(pl, A, na, lda, cols_a, ids_a, B, nb, ldb, cols_b, ids_b, nc, n_bins, part, aux,
                                      counts, edges, valid, st);
  else if (b_f64)
    rc = launch_passes<float, double>(pl, A, na, lda, cols_a, ids_a, B, nb, ldb, cols_b, ids_b, nc, n_bins, part, aux,
                                      counts, edges, valid, st);
  else
    rc = launch_passes<float, float>(pl, A, na, lda, cols_a, ids_a, B, nb, ldb, cols_b, ids_b, nc, n_bins, part, aux,
                                     counts, edges, valid, st);
  if (rc != RIHIP_OK) return rc;
  hipLaunchKernelGGL(skew_finalize_kernel, dim3(nc), dim3(64), 0, st, aux, valid, edges, counts, n_bins, epsilon,
                     min_count, propagate_nan, kl, status);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int rihip_feature_log_append(const float* X, int64_t n_rows, int nf, const int64_t* user_ids,
                                        const int64_t* cand_ids, int kc, float* ring, int64_t* ring_user,
                                        int64_t* ring_item, int64_t R, int64_t* cursor, void* stream) {
  RIHIP_REQUIRE(X && user_ids && cand_ids && ring && ring_user && ring_item && cursor, RIHIP_ERR_ARG,
                "feature_log_append: null pointer");
  RIHIP_REQUIRE(n_rows >= 0 && nf >= 1 && kc >= 1 && R >= 1 && n_rows % kc == 0, RIHIP_ERR_ARG,
                "feature_log_append: n_rows=%lld nf=%d kc=%d R=%lld", (long long)n_rows, nf, kc, (long long)R);
  hipStream_t st = (hipStream_t)stream;
  if (n_rows > 0) {
    const int64_t rows = n_rows < R ? n_rows : R;
    const bool a16 = ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(ring)) & 15) == 0;
    const bool a8 = ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(ring)) & 7) == 0;
    const int V = (nf % 4 == 0 && a16) ? 4 : (nf % 2 == 0 && a8) ? 2 : 1;
    const unsigned grid = (unsigned)((rows + SKEW_LOG_ROWS - 1) / SKEW_LOG_ROWS);
    if (V == 4)
      hipLaunchKernelGGL(skew_log_append_kernel<4>, dim3(grid), dim3(256), 0, st, X, n_rows, nf, user_ids,
                         cand_ids, kc, ring, ring_user, ring_item, R, cursor);
    else if (V == 2)
      hipLaunchKernelGGL(skew_log_append_kernel<2>, dim3(grid), dim3(256), 0, st, X, n_rows, nf, user_ids,
                         cand_ids, kc, ring, ring_user, ring_item, R, cursor);
    else
      hipLaunchKernelGGL(skew_log_append_kernel<1>, dim3(grid), dim3(256), 0, st, X, n_rows, nf, user_ids,
                         cand_ids, kc, ring, ring_user, ring_item, R, cursor);
    RIHIP_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(skew_log_advance_kernel, dim3(1), dim3(64), 0, st, cursor, n_rows);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int rihip_feature_log_rewind(int64_t* cursor, void* stream) {
  RIHIP_REQUIRE(cursor, RIHIP_ERR_ARG, "feature_log_rewind: null pointer");
  hipLaunchKernelGGL(skew_log_rewind_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, cursor);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
