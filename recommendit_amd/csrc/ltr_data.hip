// LambdaMART training-set construction on the GPU: ratings -> entity statistics -> the two feature tables ->
// (user, item, label) pairs with sampled negatives -> X f32 [n_rows, nf], labels and query groups.  Replaces the
// pandas stages of the reference's FeatureEngineer (src/features/feature_engineering.py: build_user_features
// :91-166, build_item_features :172-219, build_training_pairs :225-300, build_interaction_features :306-370).
//
// Integer, HBM- and latency-bound work; no MFMA.  Design choices:
//
// * Statistics (ltr_stats_kernel): INTEGER ATOMICS, pre-aggregated per wave, not a segmented reduction after
//   grouping.  Every accumulator is an integer (counts, rating sums, sums of squares, sum (rating-3)*genre, max
//   timestamp), so the result is independent of order and needs no float atomics.  Integer atomics execute in the
//   L2 (only the float forms go to the memory side), a rating touches 3 item words and 5 user words, and ratings
//   arrive user-major: a wave whose 64 ratings belong to one user -- the common case -- reduces the user scalars with
//   shuffles and issues ONE atomic per word; a mixed wave falls back to one atomic per lane.  Item words are
//   scattered over a few thousand lines, where contention is low.  A grouping pass first would cost a sort of R keys
//   to save ~8 R L2 atomics; the grouping this file does need (per-user buckets for the pair stage) is built FROM
//   the counts, by an exclusive scan and one cursor atomic per rating.
// * Buckets ([ratings >= 4 | the rest] per user) are filled in atomic-cursor order, which is not deterministic;
//   nothing reads that order.  Positives are placed by their RANK under the key (timestamp, input position) among the
//   user's positives (a quadratic count through LDS tiles: sum P_u^2 compares, ~1e8 for ML-1M, spread over one block
//   per user), membership goes through an LDS bitmap over the candidate items (one bit per item that has a rating,
//   up to 2^20 items = 128 KiB).
// * Negatives: a keyed pseudo-random permutation of [0, 4^k) (4^k >= n_candidates, balanced Feistel network, 8 rounds
//   of rihip_splitmix64 keyed by (seed, user id)), walked in order by one wave; images >= n_candidates and items the
//   user rated are skipped, survivors are compacted by ballot + prefix so the draw order is the walk order.  Exactly
//   without replacement (a permutation visits each item once), independent of grid and scheduling, and still
//   correct when m_u = U_u (the walk then covers the whole domain).  Cost per user: m_u * n_cand / U_u * (4^k /
//   n_cand <= 4) Feistel evaluations, i.e. proportional to the rows produced while m_u << U_u.  The alternative
//   (random key per (user, item) + radix select of the m_u smallest) costs n_cand per user whatever m_u is, and is
//   not built.
// * The train / test split uses the same permutation over [0, n_queries) (cycle-walked to a bijection): query q is
//   held out iff perm(q) < n_test.  Rows are emitted straight into [train rows | test rows], each part ordered by
//   query id, so no gather pass follows.
// * Join (ltr_join_kernel): the row-per-wave layout of rank_features_wave_kernel with TRAINING semantics: the
//   popularity ratio in float32, rows the left merge leaves empty (and NaN metadata) become 0.0; two rows in flight
//   per wave and scalar id loads (comment at the kernel).
#include "common.h"
#include "recommendit_hip.h"

namespace {

constexpr int UW = 24, IW = 23, NG = 18, UA = 24, IA = 3, MW = 1 + NG;
constexpr unsigned long long TS_BIAS = 0x8000000000000000ull;
constexpr int ERR_ID = 1, ERR_RATING = 2, ERR_PAIR_ID = 4;

__device__ __forceinline__ bool rating_ok(int64_t u, int64_t it, int r, int64_t n_users, int64_t n_items, int* err) {
  if (u < 1 || u > n_users || it < 1 || it > n_items) { atomicOr(err, ERR_ID); return false; }
  if (r < 1 || r > 5) { atomicOr(err, ERR_RATING); return false; }
  return true;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(v, o, 64); v = t > v ? t : v; }
  return v;
}
__device__ __forceinline__ void add64(int64_t* p, long long v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }

// user_acc i64 [n_users+1, 24]: count, rating sum, last timestamp (biased to unsigned order), liked (rating >= 4),
// liked with a catalogue item, unused, 18 genre accumulators.  item_acc i64 [n_items+1, 3]: count, sum, sum of squares.
__global__ __launch_bounds__(256) void ltr_stats_kernel(const int64_t* __restrict__ ru, const int64_t* __restrict__ ri,
                                                        const int* __restrict__ rv, const int64_t* __restrict__ rt,
                                                        int64_t R, int64_t n_users, int64_t n_items,
                                                        const double* __restrict__ item_meta,
                                                        const uint8_t* __restrict__ in_cat, int64_t* uacc, int64_t* iacc,
                                                        int* err) {
  const int lane = threadIdx.x & 63;
  for (int64_t i0 = (int64_t)blockIdx.x * 256; i0 < R; i0 += (int64_t)gridDim.x * 256) {
    const int64_t i = i0 + threadIdx.x;
    bool ok = i < R;
    int64_t u = 0, it = 0;
    int r = 0;
    unsigned long long ts = 0;
    if (ok) {
      u = ru[i]; it = ri[i]; r = rv[i]; ts = (unsigned long long)rt[i] ^ TS_BIAS;
      ok = rating_ok(u, it, r, n_users, n_items, err);
    }
    const bool liked = ok && r >= 4;
    const bool liked_cat = liked && in_cat[it];
    if (ok) {
      add64(iacc + it * IA + 0, 1);
      add64(iacc + it * IA + 1, r);
      add64(iacc + it * IA + 2, r * r);
    }
    if (liked_cat) {
#pragma unroll 1
      for (int g = 0; g < NG; ++g)
        if (item_meta[it * MW + 1 + g] != 0.0) add64(uacc + u * UA + 6 + g, r - 3);
    }
    // user scalars: one atomic per word when the whole wave holds one user
    const unsigned long long okm = __ballot(ok);
    if (okm == 0ull) continue;
    const int first = __ffsll((long long)okm) - 1;
    const int64_t u0 = __shfl(u, first, 64);
    if (__all(!ok || u == u0)) {
      const int c = wave_sum_i(ok ? 1 : 0), s = wave_sum_i(ok ? r : 0), l = wave_sum_i(liked ? 1 : 0),
                lc = wave_sum_i(liked_cat ? 1 : 0);
      const unsigned long long mx = wave_max_u64(ok ? ts : 0ull);
      if (lane == 0) {
        add64(uacc + u0 * UA + 0, c);
        add64(uacc + u0 * UA + 1, s);
        atomicMax(reinterpret_cast<unsigned long long*>(uacc + u0 * UA + 2), mx);
        if (l) add64(uacc + u0 * UA + 3, l);
        if (lc) add64(uacc + u0 * UA + 4, lc);
      }
    } else if (ok) {
      add64(uacc + u * UA + 0, 1);
      add64(uacc + u * UA + 1, r);
      atomicMax(reinterpret_cast<unsigned long long*>(uacc + u * UA + 2), ts);
      if (liked) add64(uacc + u * UA + 3, 1);
      if (liked_cat) add64(uacc + u * UA + 4, 1);
    }
  }
}

// scratch u64 [3]: min / max of the per-user last timestamps (biased), max item count
__global__ __launch_bounds__(256) void ltr_minmax_kernel(const int64_t* __restrict__ uacc, const int64_t* __restrict__ iacc,
                                                         int64_t n_users, int64_t n_items, unsigned long long* scratch) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i <= n_users && uacc[i * UA] > 0) {
    const unsigned long long l = (unsigned long long)uacc[i * UA + 2];
    atomicMin(scratch + 0, l);
    atomicMax(scratch + 1, l);
  }
  if (i <= n_items && iacc[i * IA] > 0) atomicMax(scratch + 2, (unsigned long long)iacc[i * IA]);
}

__global__ __launch_bounds__(256) void ltr_finalize_user_kernel(const int64_t* __restrict__ uacc,
                                                                const double* __restrict__ user_meta, int64_t n_users,
                                                                const unsigned long long* __restrict__ scratch,
                                                                double* tab) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u > n_users) return;
  double* row = tab + u * UW;
  const int64_t* a = uacc + u * UA;
  const int64_t cnt = a[0];
  if (cnt <= 0) {   // the serving defaults (recommender.py:227-232)
    row[0] = 3.5; row[1] = 0.0; row[2] = 0.5; row[3] = 0.0; row[4] = 0.3; row[5] = 0.3;
    for (int g = 0; g < NG; ++g) row[6 + g] = 0.0;
    return;
  }
  row[0] = (double)a[1] / (double)cnt;
  row[1] = (double)(float)log1p((double)cnt);
  const unsigned long long lo = scratch[0], hi = scratch[1];
  const double range = (double)(hi - lo);
  row[2] = range > 0.0 ? (double)(float)((double)((unsigned long long)a[2] - lo) / range) : 1.0;
  row[3] = user_meta[u * 3 + 0]; row[4] = user_meta[u * 3 + 1]; row[5] = user_meta[u * 3 + 2];
  const int64_t n = a[4];
  double v[NG], ss = 0.0;
#pragma unroll
  for (int g = 0; g < NG; ++g) {
    v[g] = n > 0 ? (double)a[6 + g] / (double)n : 0.0;
    ss += v[g] * v[g];
  }
  const double norm = sqrt(ss);
#pragma unroll
  for (int g = 0; g < NG; ++g) row[6 + g] = norm > 0.0 ? v[g] / norm : v[g];
}

__global__ __launch_bounds__(256) void ltr_finalize_item_kernel(const int64_t* __restrict__ iacc,
                                                                const double* __restrict__ item_meta, int64_t n_items,
                                                                const unsigned long long* __restrict__ scratch,
                                                                double* tab) {
  const int64_t it = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (it > n_items) return;
  double* row = tab + it * IW;
  const int64_t n = iacc[it * IA], s = iacc[it * IA + 1], q = iacc[it * IA + 2];
  if (n <= 0) {     // the serving defaults (recommender.py:234-238)
    row[0] = 3.5; row[1] = 0.0; row[2] = 0.0; row[3] = 0.0; row[4] = 0.5;
    for (int g = 0; g < NG; ++g) row[5 + g] = 0.0;
    return;
  }
  const float lg = (float)log1p((double)n), lmax = (float)log1p((double)scratch[2]);
  row[0] = (double)s / (double)n;
  row[1] = (double)lg;
  row[2] = (double)(lg / lmax);
  row[3] = n > 1 ? sqrt((double)(n * q - s * s) / (double)(n * (n - 1))) : 0.0;
  row[4] = item_meta[it * MW];
  for (int g = 0; g < NG; ++g) row[5 + g] = item_meta[it * MW + 1 + g];
}

// ---- scans (one block of 1024 threads; n_users / n_items entries, a few passes) ---------------------------------
__device__ __forceinline__ long long block_exscan(long long v, long long* total) {
  __shared__ long long ws[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long long inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) ws[w] = inc;
  __syncthreads();
  long long base = 0, tot = 0;
  for (int k = 0; k < 16; ++k) {
    const long long x = ws[k];
    if (k < w) base += x;
    tot += x;
  }
  *total = tot;
  return base + inc - v;
}

__device__ __forceinline__ uint32_t feistel(uint32_t x, int hb, uint64_t key) {
  const uint32_t mask = (1u << hb) - 1u;
  uint32_t L = x >> hb, Rr = x & mask;
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const uint32_t F = (uint32_t)(rihip_splitmix64(key ^ (((uint64_t)(r + 1) << 32) | Rr)) >> 32) & mask;
    const uint32_t nl = Rr;
    Rr = L ^ F;
    L = nl;
  }
  return (L << hb) | Rr;
}
__device__ __forceinline__ int half_bits(int64_t n) {   // smallest k >= 1 with 4^k >= n
  int k = 1;
  while (((int64_t)1 << (2 * k)) < n) ++k;
  return k;
}

// cand_index[i] = rank of item i among the items with a rating, cand_items = its inverse; bucket_off = exclusive scan
// of the per-user counts.  totals[5] = n_cand.
__global__ __launch_bounds__(1024) void ltr_scan1_kernel(const int64_t* __restrict__ uacc, const int64_t* __restrict__ iacc,
                                                         int64_t n_users, int64_t n_items, int* cand_index,
                                                         int64_t* cand_items, int64_t* bucket_off, int64_t* totals) {
  long long run = 0, tot;
  for (int64_t b = 0; b <= n_items; b += 1024) {
    const int64_t i = b + threadIdx.x;
    const long long f = (i <= n_items && iacc[i * IA] > 0) ? 1 : 0;
    const long long p = run + block_exscan(f, &tot);
    if (i <= n_items) cand_index[i] = f ? (int)p : -1;
    if (f) cand_items[p] = i;
    run += tot;
  }
  if (threadIdx.x == 0) totals[5] = run;
  run = 0;
  for (int64_t b = 0; b <= n_users; b += 1024) {
    const int64_t u = b + threadIdx.x;
    const long long c = u <= n_users ? uacc[u * UA] : 0;
    const long long p = run + block_exscan(c, &tot);
    if (u <= n_users) bucket_off[u] = p;
    run += tot;
  }
  if (threadIdx.x == 0) bucket_off[n_users + 1] = run;
}

// bucket of user u = [its ratings >= 4 | its other ratings], each part in atomic-cursor order (cursor i32
// [2, n_users+1]); the statistics pass already knows where the second part starts
__global__ __launch_bounds__(256) void ltr_bucket_kernel(const int64_t* __restrict__ ru, const int64_t* __restrict__ ri,
                                                         const int* __restrict__ rv, int64_t R, int64_t n_users,
                                                         int64_t n_items, const int64_t* __restrict__ uacc,
                                                         const int64_t* __restrict__ bucket_off, int* cursor, int* bucket) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < R; i += (int64_t)gridDim.x * 256) {
    const int64_t u = ru[i], it = ri[i];
    const int r = rv[i];
    if (u < 1 || u > n_users || it < 1 || it > n_items || r < 1 || r > 5) continue;   // flagged by the statistics pass
    const int64_t slot = r >= 4 ? atomicAdd(cursor + u, 1) : uacc[u * UA + 3] + atomicAdd(cursor + (n_users + 1) + u, 1);
    bucket[bucket_off[u] + slot] = (int)i;
  }
}

// LDS bitmap of the candidate indices user u rated; returns (to every thread) the number of distinct rated items
__device__ __forceinline__ int fill_bitmap(unsigned* bm, int words, const int* __restrict__ bucket, int64_t off, int64_t n,
                                           const int64_t* __restrict__ ri, const int* __restrict__ cand_index, int* s_cnt) {
  for (int w = threadIdx.x; w < words; w += 256) bm[w] = 0u;
  if (threadIdx.x == 0) *s_cnt = 0;
  __syncthreads();
  for (int64_t k = threadIdx.x; k < n; k += 256) {
    const int c = cand_index[ri[bucket[off + k]]];
    atomicOr(bm + (c >> 5), 1u << (c & 31));
  }
  __syncthreads();
  int part = 0;
  for (int w = threadIdx.x; w < words; w += 256) part += __popc(bm[w]);
  part = wave_sum_i(part);
  if ((threadIdx.x & 63) == 0 && part) atomicAdd(s_cnt, part);
  __syncthreads();
  return *s_cnt;
}

// user_rows[u] = P_u + m_u for a kept user, 0 otherwise (reference :257-262; m_u = min(P_u * n_neg, U_u))
__global__ __launch_bounds__(256) void ltr_plan_user_kernel(const int64_t* __restrict__ uacc, const int64_t* __restrict__ ri,
                                                            const int* __restrict__ bucket,
                                                            const int64_t* __restrict__ bucket_off,
                                                            const int* __restrict__ cand_index, int64_t n_users,
                                                            int n_neg, int64_t* totals, int* user_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned bm[];
  __shared__ int s_cnt;
  const int64_t n_cand = totals[5];
  const int words = (int)((n_cand + 31) >> 5);
  for (int64_t u = 1 + blockIdx.x; u <= n_users; u += gridDim.x) {
    const int64_t off = bucket_off[u], n = bucket_off[u + 1] - off;
    const int64_t P = uacc[u * UA + 3];
    if (n == 0 || P == 0) {
      if (threadIdx.x == 0) user_rows[u] = 0;
      continue;
    }
    const int D = fill_bitmap(bm, words, bucket, off, n, ri, cand_index, &s_cnt);
    if (threadIdx.x == 0) {
      const int64_t U = n_cand - D;
      int64_t rows = 0;
      if (U >= n_neg) {
        const int64_t want = P * n_neg;
        rows = P + (want < U ? want : U);
      }
      if (rows > 0x7fffffffll) rows = 0x7fffffffll;
      user_rows[u] = (int)rows;
      if (rows > 0) atomicMax(reinterpret_cast<unsigned long long*>(totals + 4), (unsigned long long)rows);
    }
    __syncthreads();
  }
}

// query ids, the seeded split and every row offset.  totals: [0] n_rows, [1] n_queries, [2] n_train_rows,
// [3] n_train_queries, [4] max rows of a query, [5] n_cand, [6] n_test_queries
__global__ __launch_bounds__(1024) void ltr_scan2_kernel(const int* __restrict__ user_rows, int64_t n_users,
                                                         double test_ratio, uint64_t split_key, int* query_id,
                                                         int64_t* row_start, int* groups, int64_t* totals) {
  long long run = 0, tot;
  for (int64_t b = 1; b <= n_users; b += 1024) {
    const int64_t u = b + threadIdx.x;
    const long long f = (u <= n_users && user_rows[u] > 0) ? 1 : 0;
    const long long p = run + block_exscan(f, &tot);
    if (u <= n_users) query_id[u] = f ? (int)p : -1;
    run += tot;
  }
  const long long nq = run;
  long long n_test = (long long)((double)nq * test_ratio);     // max(1, int(n_queries * test_ratio)), reference :289
  if (n_test < 1) n_test = 1;
  if (n_test > nq) n_test = nq;
  const int hb = half_bits(nq);
  if (threadIdx.x == 0) { query_id[0] = -1; row_start[0] = -1; }
  long long rows_run = 0, q_run = 0;
  for (int part = 0; part < 2; ++part) {          // train rows first, then the held-out queries
    for (int64_t b = 1; b <= n_users; b += 1024) {
      const int64_t u = b + threadIdx.x;
      long long rows = 0;
      if (u <= n_users && user_rows[u] > 0) {
        uint32_t y = (uint32_t)query_id[u];
        do y = feistel(y, hb, split_key); while ((long long)y >= nq);   // cycle walk: a bijection on [0, nq)
        if (((long long)y < n_test) == (part == 1)) rows = user_rows[u];
      }
      long long tr, tq;
      const long long pr = block_exscan(rows, &tr);
      const long long pq = block_exscan(rows > 0 ? 1 : 0, &tq);
      if (rows > 0) {
        row_start[u] = rows_run + pr;
        groups[q_run + pq] = (int)rows;
      } else if (part == 0 && u <= n_users) {
        row_start[u] = -1;
      }
      rows_run += tr;
      q_run += tq;
    }
    if (part == 0 && threadIdx.x == 0) { totals[2] = rows_run; totals[3] = q_run; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { totals[0] = rows_run; totals[1] = nq; totals[6] = n_test; }
}

__global__ __launch_bounds__(256) void ltr_emit_kernel(const int64_t* __restrict__ ri, const int* __restrict__ rv,
                                                       const int64_t* __restrict__ rt, const int64_t* __restrict__ uacc,
                                                       const int* __restrict__ bucket, const int64_t* __restrict__ bucket_off,
                                                       const int* __restrict__ cand_index,
                                                       const int64_t* __restrict__ cand_items,
                                                       const int* __restrict__ user_rows, const int64_t* __restrict__ row_start,
                                                       const int* __restrict__ query_id, const int64_t* __restrict__ totals,
                                                       int64_t n_users, int64_t n_rows, uint64_t seed_mix, int64_t* out_user,
                                                       int64_t* out_item, float* out_label, int* out_rating,
                                                       int64_t* out_query) {
  extern __shared__ __attribute__((aligned(16))) unsigned bm[];
  __shared__ int s_cnt;
  __shared__ long long s_ts[1024];
  __shared__ int s_pos[1024];
  const int64_t n_cand = totals[5];
  const int words = (int)((n_cand + 31) >> 5);
  const int hb = half_bits(n_cand);
  const int64_t dom = (int64_t)1 << (2 * hb);
  const int lane = threadIdx.x & 63;
  for (int64_t u = 1 + blockIdx.x; u <= n_users; u += gridDim.x) {
    const int64_t base = row_start[u];
    if (base < 0) continue;
    const int64_t off = bucket_off[u], n = bucket_off[u + 1] - off;
    const int64_t P = uacc[u * UA + 3], m = (int64_t)user_rows[u] - P;
    if (base + P + m > n_rows) continue;          // never taken: the plan and the buffers come from one call
    const int q = query_id[u];
    fill_bitmap(bm, words, bucket, off, n, ri, cand_index, &s_cnt);
    // positives = the first P bucket entries, placed by rank under (timestamp, input position)
    const bool single = P <= 1024;
    for (int64_t r0 = 0; r0 < P; r0 += 256) {
      const int64_t i = r0 + threadIdx.x;
      const bool mine = i < P;
      int pos_i = 0;
      long long ts_i = 0;
      if (mine) {
        pos_i = bucket[off + i];
        ts_i = rt[pos_i];
      }
      int64_t rank = 0;
      for (int64_t t0 = 0; t0 < P; t0 += 1024) {
        const int lim = (int)(P - t0 < 1024 ? P - t0 : 1024);
        if (!(single && r0 > 0)) {
          __syncthreads();
          for (int k = threadIdx.x; k < lim; k += 256) {
            const int p = bucket[off + t0 + k];
            s_pos[k] = p; s_ts[k] = rt[p];
          }
          __syncthreads();
        }
        if (mine)
          for (int k = 0; k < lim; ++k) {
            const int p = s_pos[k];
            const long long t = s_ts[k];
            rank += (t < ts_i || (t == ts_i && p < pos_i)) ? 1 : 0;
          }
      }
      if (mine && rank < P) {
        const int64_t o = base + rank;
        out_user[o] = u; out_item[o] = ri[pos_i]; out_label[o] = 1.f; out_rating[o] = rv[pos_i]; out_query[o] = q;
      }
    }
    // negatives: wave 0 walks the user's permutation of the candidate indices
    if (threadIdx.x < 64) {
      const uint64_t key = rihip_splitmix64(seed_mix ^ rihip_splitmix64((uint64_t)u));
      int64_t found = 0;
      for (int64_t t0 = 0; t0 < dom && found < m; t0 += 64) {
        const int64_t t = t0 + lane;
        bool ok = false;
        uint32_t y = 0;
        if (t < dom) {
          y = feistel((uint32_t)t, hb, key);
          ok = (int64_t)y < n_cand && !((bm[y >> 5] >> (y & 31)) & 1u);
        }
        const unsigned long long mask = __ballot(ok);
        const int64_t idx = found + __popcll(mask & ((1ull << lane) - 1ull));
        if (ok && idx < m) {
          const int64_t o = base + P + idx;
          out_user[o] = u; out_item[o] = cand_items[y]; out_label[o] = 0.f; out_rating[o] = 0; out_query[o] = q;
        }
        found += __popcll(mask);
      }
    }
    __syncthreads();
  }
}

__device__ __forceinline__ double readlane_d(double x, int lane) {
  const long long b = __double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// one wave per (user, item) row: lanes 0..23 hold the user row, 24..46 the item row.  A side that the left merge would
// leave empty -- an entity without ratings, which both tables mark with log_rating_count == 0.0 (log1p of a count >= 1
// is >= 0.69; the default rows hold 0.0) -- is NaN, and every NaN becomes 0.0 at the end (fillna(0.0), :369).
// Against the serving kernel's one-row loop: the row index is wave-uniform by construction (readfirstlane), so the
// two ids are scalar loads; and two rows per wave and iteration have all their loads issued before either is
// computed, which doubles the bytes in flight per wave.
struct JoinRow {
  double v, pg;
  bool live, bad;
};
__device__ __forceinline__ JoinRow join_load(const double* __restrict__ user_tab, int64_t n_urows,
                                             const double* __restrict__ item_tab, int64_t n_irows, int64_t uid,
                                             int64_t iid, bool live, int lane) {
  JoinRow r;
  r.live = live;
  r.bad = live && (uid < 0 || uid >= n_urows || iid < 0 || iid >= n_irows);
  if (!live || r.bad) uid = iid = 0;
  r.v = 0.0;
  if (lane < UW) r.v = user_tab[uid * UW + lane];
  else if (lane < UW + IW) r.v = item_tab[iid * IW + (lane - UW)];
  r.pg = 0.0;
  if (lane < NG) r.pg = user_tab[uid * UW + 6 + lane] * item_tab[iid * IW + 5 + lane];
  return r;
}
__device__ __forceinline__ void join_store(const JoinRow& r, int64_t row, int c, int src, int lane, int nf, float* X,
                                           int* err) {
  if (!r.live) return;
  if (r.bad) {
    if (lane == 0) atomicOr(err, ERR_PAIR_ID);
    if (lane < nf) X[row * nf + lane] = 0.f;
    return;
  }
  const double qnan = __longlong_as_double(0x7ff8000000000000ll);
  const double u0 = readlane_d(r.v, 0), u1 = readlane_d(r.v, 1), i0 = readlane_d(r.v, UW), i1 = readlane_d(r.v, UW + 1);
  const bool hu = u1 != 0.0, hi = i1 != 0.0;
  double v = r.v, pg = r.pg;
  if ((lane < UW && !hu) || (lane >= UW && !hi)) v = qnan;
  if (!(hu && hi)) pg = qnan;
  double aff = 0.0;
#pragma unroll
  for (int g = 0; g < NG; ++g) aff += readlane_d(pg, g);
  double f = __shfl(v, src, 64);
  float out;
  if (c == 12) out = (float)u1 / ((float)i1 + 1e-8f);     // float32 / (float32 + float32(1e-8)), as the merged frame does
  else {
    if (c == 11) f = u0 - i0;
    else if (c == 13) f = aff;
    out = (float)f;
  }
  if (!(hu && hi) && (c == 11 || c == 12)) out = 0.f;
  if (out != out || c < 0) out = 0.f;
  if (lane < nf) X[row * nf + lane] = out;
}
__global__ __launch_bounds__(256) void ltr_join_kernel(const double* __restrict__ user_tab, int64_t n_urows,
                                                       const double* __restrict__ item_tab, int64_t n_irows,
                                                       const int64_t* __restrict__ user_ids,
                                                       const int64_t* __restrict__ item_ids, int64_t n_rows,
                                                       const int* __restrict__ col_map, int nf, float* X, int* err) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane < nf ? col_map[lane] : -1;
  int src = 0;
  if (c >= 0) {
    if (c < 6) src = c;
    else if (c < 11) src = UW + (c - 6);
    else if (c >= 14 && c < 14 + NG) src = 6 + (c - 14);
    else if (c >= 14 + NG) src = UW + 5 + (c - 14 - NG);
  }
  const int64_t stride = (int64_t)gridDim.x * 4;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < n_rows; row += 2 * stride) {
    const int64_t row2 = row + stride;
    const bool live2 = row2 < n_rows;
    const int64_t ua = user_ids[row], ia = item_ids[row];
    const int64_t ub = live2 ? user_ids[row2] : 0, ib = live2 ? item_ids[row2] : 0;
    const JoinRow a = join_load(user_tab, n_urows, item_tab, n_irows, ua, ia, true, lane);
    const JoinRow b = join_load(user_tab, n_urows, item_tab, n_irows, ub, ib, live2, lane);
    join_store(a, row, c, src, lane, nf, X, err);
    join_store(b, row2, c, src, lane, nf, X, err);
  }
}

int grid_for(int64_t work_items, int per_block, int grid_blocks) {
  if (grid_blocks > 0) return grid_blocks;
  int64_t nb = (work_items + per_block - 1) / per_block;
  if (nb < 1) nb = 1;
  return (int)(nb < 16384 ? nb : 16384);
}

constexpr int64_t MAX_CAND = 1ll << 20;   // LDS bitmap: 2^20 bits = 128 KiB

int grant_bitmap_lds() {
  static bool granted = false;
  if (!granted) {
    RIHIP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ltr_plan_user_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)(MAX_CAND / 8)));
    RIHIP_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ltr_emit_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)(MAX_CAND / 8)));
    granted = true;
  }
  return RIHIP_OK;
}

}  // namespace

extern "C" int rihip_ltr_widths(int* user_acc_width, int* item_acc_width, int* n_totals) {
  if (user_acc_width) *user_acc_width = UA;
  if (item_acc_width) *item_acc_width = IA;
  if (n_totals) *n_totals = 8;
  return RIHIP_OK;
}

extern "C" int rihip_ltr_stats(const int64_t* rating_user, const int64_t* rating_item, const int* rating_value,
                               const int64_t* rating_ts, int64_t n_ratings, int64_t n_users, int64_t n_items,
                               const double* item_meta, const uint8_t* item_in_catalog, int64_t* user_acc,
                               int64_t* item_acc, int* err, int grid_blocks, void* stream) {
  RIHIP_REQUIRE(item_meta && item_in_catalog && user_acc && item_acc && err, RIHIP_ERR_ARG, "ltr_stats: null pointer");
  RIHIP_REQUIRE(n_ratings == 0 || (rating_user && rating_item && rating_value && rating_ts), RIHIP_ERR_ARG,
                "ltr_stats: null rating array");
  RIHIP_REQUIRE(n_ratings >= 0 && n_ratings < (1ll << 31) && n_users >= 0 && n_items >= 0 && grid_blocks >= 0,
                RIHIP_ERR_ARG, "ltr_stats: bad sizes (n_ratings=%lld, n_users=%lld, n_items=%lld)", (long long)n_ratings,
                (long long)n_users, (long long)n_items);
  hipStream_t s = (hipStream_t)stream;
  RIHIP_CHECK_HIP(hipMemsetAsync(user_acc, 0, sizeof(int64_t) * UA * (size_t)(n_users + 1), s));
  RIHIP_CHECK_HIP(hipMemsetAsync(item_acc, 0, sizeof(int64_t) * IA * (size_t)(n_items + 1), s));
  RIHIP_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int), s));
  if (n_ratings == 0) return RIHIP_OK;
  hipLaunchKernelGGL(ltr_stats_kernel, dim3(grid_for(n_ratings, 256, grid_blocks)), dim3(256), 0, s, rating_user,
                     rating_item, rating_value, rating_ts, n_ratings, n_users, n_items, item_meta, item_in_catalog,
                     user_acc, item_acc, err);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int rihip_ltr_finalize(const int64_t* user_acc, const int64_t* item_acc, const double* user_meta,
                                  const double* item_meta, int64_t n_users, int64_t n_items, int64_t* scratch,
                                  double* user_tab, double* item_tab, void* stream) {
  RIHIP_REQUIRE(user_acc && item_acc && user_meta && item_meta && scratch && user_tab && item_tab, RIHIP_ERR_ARG,
                "ltr_finalize: null pointer");
  RIHIP_REQUIRE(n_users >= 0 && n_items >= 0, RIHIP_ERR_ARG, "ltr_finalize: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  RIHIP_CHECK_HIP(hipMemsetAsync(scratch, 0xff, sizeof(int64_t), s));
  RIHIP_CHECK_HIP(hipMemsetAsync(scratch + 1, 0, 2 * sizeof(int64_t), s));
  const int64_t nmax = (n_users > n_items ? n_users : n_items) + 1;
  unsigned long long* sc = reinterpret_cast<unsigned long long*>(scratch);
  hipLaunchKernelGGL(ltr_minmax_kernel, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, s, user_acc, item_acc, n_users,
                     n_items, sc);
  hipLaunchKernelGGL(ltr_finalize_user_kernel, dim3((unsigned)((n_users + 256) / 256)), dim3(256), 0, s, user_acc,
                     user_meta, n_users, sc, user_tab);
  hipLaunchKernelGGL(ltr_finalize_item_kernel, dim3((unsigned)((n_items + 256) / 256)), dim3(256), 0, s, item_acc,
                     item_meta, n_items, sc, item_tab);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int rihip_ltr_plan(const int64_t* rating_user, const int64_t* rating_item, const int* rating_value,
                              int64_t n_ratings, const int64_t* user_acc, const int64_t* item_acc, int64_t n_users,
                              int64_t n_items, int n_negatives, double test_ratio, uint64_t seed, int64_t* bucket_off,
                              int* bucket, int* cursor, int* cand_index, int64_t* cand_items, int* user_rows,
                              int* query_id, int64_t* row_start, int* groups, int64_t* totals, int grid_blocks,
                              void* stream) {
  RIHIP_REQUIRE(user_acc && item_acc && bucket_off && bucket && cursor && cand_index && cand_items && user_rows &&
                    query_id && row_start && groups && totals, RIHIP_ERR_ARG, "ltr_plan: null pointer");
  RIHIP_REQUIRE(n_ratings == 0 || (rating_user && rating_item && rating_value), RIHIP_ERR_ARG,
                "ltr_plan: null rating array");
  RIHIP_REQUIRE(n_ratings >= 0 && n_ratings < (1ll << 31) && n_users >= 0 && n_items >= 0 && n_items < MAX_CAND &&
                    grid_blocks >= 0, RIHIP_ERR_ARG,
                "ltr_plan: bad sizes (n_ratings=%lld, n_users=%lld, n_items=%lld; at most %lld items)",
                (long long)n_ratings, (long long)n_users, (long long)n_items, (long long)MAX_CAND - 1);
  RIHIP_REQUIRE(n_negatives >= 1 && n_negatives <= 4096 && test_ratio >= 0.0 && test_ratio <= 1.0, RIHIP_ERR_ARG,
                "ltr_plan: n_negatives=%d (1..4096), test_ratio=%g (0..1)", n_negatives, test_ratio);
  if (int rc = grant_bitmap_lds()) return rc;
  hipStream_t s = (hipStream_t)stream;
  RIHIP_CHECK_HIP(hipMemsetAsync(totals, 0, 8 * sizeof(int64_t), s));
  RIHIP_CHECK_HIP(hipMemsetAsync(cursor, 0, sizeof(int) * 2 * (size_t)(n_users + 1), s));
  RIHIP_CHECK_HIP(hipMemsetAsync(user_rows, 0, sizeof(int) * (size_t)(n_users + 1), s));
  hipLaunchKernelGGL(ltr_scan1_kernel, dim3(1), dim3(1024), 0, s, user_acc, item_acc, n_users, n_items, cand_index,
                     cand_items, bucket_off, totals);
  if (n_ratings > 0)
    hipLaunchKernelGGL(ltr_bucket_kernel, dim3(grid_for(n_ratings, 256, grid_blocks)), dim3(256), 0, s, rating_user,
                       rating_item, rating_value, n_ratings, n_users, n_items, user_acc, bucket_off, cursor, bucket);
  const size_t lds = (size_t)((n_items + 1 + 31) / 32) * 4;     // n_cand <= n_items + 1
  if (n_users > 0)
    hipLaunchKernelGGL(ltr_plan_user_kernel, dim3(grid_for(n_users, 1, grid_blocks)), dim3(256), lds, s, user_acc,
                       rating_item, bucket, bucket_off, cand_index, n_users, n_negatives, totals, user_rows);
  const uint64_t split_key = rihip_splitmix64(rihip_splitmix64(seed) ^ 0x53504c4954ull);   // "SPLIT"
  hipLaunchKernelGGL(ltr_scan2_kernel, dim3(1), dim3(1024), 0, s, user_rows, n_users, test_ratio, split_key, query_id,
                     row_start, groups, totals);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int rihip_ltr_emit(const int64_t* rating_item, const int* rating_value, const int64_t* rating_ts,
                              const int64_t* user_acc, const int64_t* bucket_off, const int* bucket,
                              const int* cand_index, const int64_t* cand_items, const int* user_rows,
                              const int* query_id, const int64_t* row_start, const int64_t* totals, int64_t n_users,
                              int64_t n_items, int64_t n_rows, uint64_t seed, int64_t* out_user, int64_t* out_item,
                              float* out_label, int* out_rating, int64_t* out_query, int grid_blocks, void* stream) {
  RIHIP_REQUIRE(user_acc && bucket_off && bucket && cand_index && cand_items && user_rows && query_id && row_start &&
                    totals, RIHIP_ERR_ARG, "ltr_emit: null pointer");
  RIHIP_REQUIRE(n_users >= 0 && n_items >= 0 && n_items < MAX_CAND && n_rows >= 0 && grid_blocks >= 0, RIHIP_ERR_ARG,
                "ltr_emit: bad sizes");
  if (n_rows == 0 || n_users == 0) return RIHIP_OK;
  RIHIP_REQUIRE(rating_item && rating_value && rating_ts && out_user && out_item && out_label && out_rating && out_query,
                RIHIP_ERR_ARG, "ltr_emit: null pointer");
  if (int rc = grant_bitmap_lds()) return rc;
  const size_t lds = (size_t)((n_items + 1 + 31) / 32) * 4;
  hipLaunchKernelGGL(ltr_emit_kernel, dim3(grid_for(n_users, 1, grid_blocks)), dim3(256), lds, (hipStream_t)stream,
                     rating_item, rating_value, rating_ts, user_acc, bucket, bucket_off, cand_index, cand_items, user_rows,
                     row_start, query_id, totals, n_users, n_rows, rihip_splitmix64(seed), out_user, out_item, out_label,
                     out_rating, out_query);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int rihip_ltr_join(const double* user_tab, int64_t n_user_rows, const double* item_tab, int64_t n_item_rows,
                              const int64_t* user_ids, const int64_t* item_ids, int64_t n_rows, const int* col_map,
                              int nf, float* X, int* err, int grid_blocks, void* stream) {
  RIHIP_REQUIRE(user_tab && item_tab && col_map && err, RIHIP_ERR_ARG, "ltr_join: null pointer");
  RIHIP_REQUIRE(n_rows >= 0 && nf >= 1 && nf <= 64 && n_user_rows > 0 && n_item_rows > 0 && grid_blocks >= 0,
                RIHIP_ERR_ARG, "ltr_join: bad sizes (n_rows=%lld, nf=%d: 1..64)", (long long)n_rows, nf);
  RIHIP_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int), (hipStream_t)stream));
  if (n_rows == 0) return RIHIP_OK;
  RIHIP_REQUIRE(user_ids && item_ids && X, RIHIP_ERR_ARG, "ltr_join: null pointer");
  hipLaunchKernelGGL(ltr_join_kernel, dim3(grid_for(n_rows, 4, grid_blocks)), dim3(256), 0, (hipStream_t)stream, user_tab,
                     n_user_rows, item_tab, n_item_rows, user_ids, item_ids, n_rows, col_map, nf, X, err);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
