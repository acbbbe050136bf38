// Cold-start users: the query vector and the ranking-feature row of a user who has no trained row in the user tower,
// from a short rating history -- not in the reference, which answers such users with _popularity_recommendations only
// (src/serving/recommender.py:304-307, :393-410).  The definition is at rihip_fold_in_users in recommendit_hip.h: a
// closed form (the weighted mean of the liked items' stored vectors minus beta times the corpus mean, renormalised),
// no per-user optimisation loop, no random numbers.
//
// fold_in_kernel: one 256-thread workgroup per slot; the slot's CSR row is walked in tiles of FOLD_TILE entries.
//  * Scan (every thread, FOLD_TILE / 256 entries of the tile, coalesced): range checks (the error word), the integer
//    statistics of the feature row (count, rating sum, liked count and the 18 genre accumulators: the arithmetic of
//    ltr_stats_kernel, kept in registers), the membership test through row_of, and the (row, weight) of each entry into
//    LDS.  The item -> row_of -> vector chain of dependent loads is cut here: the gather below starts from LDS.
//  * Gather: the work is ragged rows of d * 4 bytes.  A row of d floats is owned by LPR = pow2 >= d / 4 lanes, 16 B
//    each (d % 4 == 0 and an aligned table; else one float per lane and 64-column stripe), so a wave reads 64 / LPR rows
//    per instruction and keeps FOLD_ILP of them in flight; a lane's four f64 column accumulators stay in registers.
//    w * v is exact in f64 (w <= 5, v an f32), so the only roundings are the additions, in an order fixed by the
//    entry's position: no atomics, two launches agree bit for bit.
//  * Combine: every lane's accumulators go to LDS once, column c is summed over the (wave, row group) partials in a
//    fixed order, wave 0 takes the norm, all threads write q; wave 1 finalises the feature row as
//    ltr_finalize_user_kernel does (lane g owns genre g).
// LDS: 8 KiB partials + 8 KiB tile + 2 KiB column vector + the integer partials: 8 workgroups (32 waves) per CU.  No host
// synchronisation, no allocation: capturable in a hipGraph.
#include <math.h>

#include "common.h"
#include "recommendit_hip.h"

namespace {

constexpr int UW = 24, IW = 23, NG = 18;
constexpr int ERR_ITEM = 1, ERR_RATING = 2;
constexpr int FOLD_TILE = 1024;   // entries staged per pass: 4 per thread
constexpr int FOLD_ILP = 4;       // gathered rows in flight per row group
constexpr int NI = 4 + NG;        // integer statistics per slot: count, rating sum, liked, W, genre accumulators

struct FoldArgs {
  const int64_t* offsets;
  const int32_t* items;
  const int32_t* ratings;
  int64_t n_entries;
  const float* V;
  int64_t n_rows, ldv;
  int d;
  const int32_t* row_of;
  int64_t n_ids;
  const double* mu;
  int min_rating, weighting;
  double beta;
  const double* item_tab;
  int64_t n_item_rows;
  const double* user_meta;
  float* q;
  double* rows;
  int* flags;
  int* err;
  int lpr_shift;   // VEC: log2 of the lanes that own one row
};

__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(256, 4) void fold_in_kernel(const FoldArgs a) {
  __shared__ double sh_part[256 * 4];       // [thread][accumulator]
  __shared__ double sh_m[256];
  __shared__ int sh_row[FOLD_TILE];
  __shared__ int sh_w[FOLD_TILE];
  __shared__ long long sh_int[4][NI];
  __shared__ double sh_norm;

  const int64_t s = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int d = a.d;
  // the slot's row, clamped into the entry arrays (a row outside them reads as empty)
  int64_t off = a.offsets[s], end = a.offsets[s + 1];
  off = off < 0 ? 0 : (off > a.n_entries ? a.n_entries : off);
  end = end < off ? off : (end > a.n_entries ? a.n_entries : end);
  const int64_t len = end - off;
  const int32_t* __restrict__ items = a.items + off;
  const int32_t* __restrict__ ratings = a.ratings + off;

  // gather geometry (wave-uniform)
  const int lpr = VEC ? 1 << a.lpr_shift : 64;            // lanes per row
  const int groups = 4 * (64 / lpr);                      // rows the workgroup reads per instruction
  const int gidx = wave * (64 / lpr) + (VEC ? lane >> a.lpr_shift : 0);
  const int chunk = VEC ? lane & (lpr - 1) : lane;
  const bool owner = VEC ? 4 * chunk < d : true;

  int st[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) st[i] = 0;
  int ebits = 0;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};

  for (int64_t t0 = 0; t0 < len; t0 += FOLD_TILE) {
    const int n_tile = (int)(len - t0 < FOLD_TILE ? len - t0 : FOLD_TILE);
    // ---- scan ----
    int it[FOLD_TILE / 256], r[FOLD_TILE / 256];
#pragma unroll
    for (int j = 0; j < FOLD_TILE / 256; ++j) {
      const int e = tid + 256 * j;
      it[j] = e < n_tile ? items[t0 + e] : 0;
      r[j] = e < n_tile ? ratings[t0 + e] : 0;
    }
    int row[FOLD_TILE / 256];
#pragma unroll
    for (int j = 0; j < FOLD_TILE / 256; ++j) {
      const bool in = tid + 256 * j < n_tile;
      const bool valid = in && it[j] >= 0 && r[j] >= 1 && r[j] <= 5;
      if (in && it[j] < 0) ebits |= ERR_ITEM;
      if (in && (r[j] < 1 || r[j] > 5)) ebits |= ERR_RATING;
      if (!valid) r[j] = 0;                               // r == 0 from here on: the entry is skipped everywhere
      row[j] = -1;
      if (valid && r[j] >= a.min_rating && (int64_t)it[j] < a.n_ids) row[j] = a.row_of[it[j]];
    }
#pragma unroll
    for (int j = 0; j < FOLD_TILE / 256; ++j) {
      const int e = tid + 256 * j;
      if (r[j] > 0) {
        st[0] += 1;
        st[1] += r[j];
        if (r[j] >= 4 && it[j] > 0 && (int64_t)it[j] < a.n_item_rows) {
          st[2] += 1;
          const double* __restrict__ g = a.item_tab + (int64_t)it[j] * IW + 5;
#pragma unroll
          for (int k = 0; k < NG; ++k)
            if (g[k] != 0.0) st[4 + k] += r[j] - 3;
        }
      }
      const bool member = row[j] >= 0 && (int64_t)row[j] < a.n_rows;
      const int w = member ? (a.weighting ? r[j] - (a.min_rating - 1) : 1) : 0;
      st[3] += w;
      if (e < n_tile) {
        sh_row[e] = member ? row[j] : 0;
        sh_w[e] = w;
      }
    }
    __syncthreads();
    // ---- gather ----
    for (int e0 = gidx; e0 < n_tile; e0 += groups * FOLD_ILP) {
      int w[FOLD_ILP];
      float v[FOLD_ILP][4];
#pragma unroll
      for (int j = 0; j < FOLD_ILP; ++j) {
        const int e = e0 + groups * j;
        w[j] = e < n_tile ? sh_w[e] : 0;
        const int rw = e < n_tile ? sh_row[e] : 0;
        const float* __restrict__ p = a.V + (int64_t)rw * a.ldv;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[j][c] = 0.f;
        if (w[j] != 0) {
          if (VEC) {
            if (owner) {
              const f32x4 x = *reinterpret_cast<const f32x4*>(p + 4 * chunk);
#pragma unroll
              for (int c = 0; c < 4; ++c) v[j][c] = x[c];
            }
          } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
              if (lane + 64 * c < d) v[j][c] = p[lane + 64 * c];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < FOLD_ILP; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] += (double)w[j] * (double)v[j][c];
    }
    __syncthreads();      // the tile is read: the next scan may overwrite it
  }
  if (ebits) atomicOr(a.err, ebits);

  // ---- combine ----
#pragma unroll
  for (int c = 0; c < 4; ++c) sh_part[tid * 4 + c] = acc[c];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int t = wave_sum_i32(st[i]);
    if (lane == 0) sh_int[wave][i] = t;
  }
  __syncthreads();
  const long long W = sh_int[0][3] + sh_int[1][3] + sh_int[2][3] + sh_int[3][3];
  if (tid < d) {
    const int l0 = VEC ? tid >> 2 : tid & 63, c = VEC ? tid & 3 : tid >> 6;
    double sum = 0.0;
    for (int wv = 0; wv < 4; ++wv)
      for (int sub = 0; sub < 64 / lpr; ++sub) sum += sh_part[(wv * 64 + sub * lpr + l0) * 4 + c];
    sh_m[tid] = W > 0 ? sum / (double)W - a.beta * a.mu[tid] : 0.0;
  }
  __syncthreads();
  if (wave == 0) {
    double ss = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (lane + 64 * c < d) ss += sh_m[lane + 64 * c] * sh_m[lane + 64 * c];
    ss = wave_sum_d(ss);
    if (lane == 0) sh_norm = sqrt(ss);
  }
  __syncthreads();
  const double nrm = sh_norm;
  const bool flag = W <= 0 || nrm < 1e-12;
  if (tid < d) a.q[s * d + tid] = flag ? 0.f : (float)(sh_m[tid] / nrm);
  if (tid == 0) a.flags[s] = flag ? 1 : 0;

  // ---- the slot's ranking-feature row (ltr_finalize_user_kernel's arithmetic), by wave 1: lane g owns genre g ----
  if (wave == 1) {
    auto total = [&](int i) { return sh_int[0][i] + sh_int[1][i] + sh_int[2][i] + sh_int[3][i]; };
    const long long cnt = total(0), liked = total(2);
    const double vg = lane < NG && liked > 0 ? (double)total(4 + (lane < NG ? lane : 0)) / (double)liked : 0.0;
    double ss = 0.0;
    for (int g = 0; g < NG; ++g) {      // in genre order, fused: what the compiler makes of the finalize kernel's sum
      const double x = __shfl(vg, g, 64);
      ss = fma(x, x, ss);
    }
    const double norm = sqrt(ss);
    double* row = a.rows + s * UW;
    if (lane < NG) {
      row[6 + lane] = cnt <= 0 ? 0.0 : (norm > 0.0 ? vg / norm : vg);
    } else if (lane == NG) {            // cnt <= 0: the serving defaults (recommender.py:227-232)
      row[0] = cnt <= 0 ? 3.5 : (double)total(1) / (double)cnt;
      row[1] = cnt <= 0 ? 0.0 : (double)(float)log1p((double)cnt);
    } else if (lane < NG + 5) {
      const int k = lane - NG - 1;
      const double dflt = k == 0 ? 0.5 : (k == 1 ? 0.0 : 0.3);
      row[2 + k] = cnt > 0 && a.user_meta ? a.user_meta[s * 4 + k] : dflt;
    }
  }
}

}  // namespace

extern "C" int rihip_fold_in_users(const int64_t* hist_offsets, const int32_t* hist_items, const int32_t* hist_ratings,
                                   int64_t nq, int64_t n_entries, const float* V, int64_t n_rows, int64_t ldv, int d,
                                   const int32_t* row_of, int64_t n_ids, const double* mu, int min_rating, int weighting,
                                   double beta, const double* item_tab, int64_t n_item_rows, const double* user_meta,
                                   float* q, double* rows, int* flags, int* err, void* stream) {
  RIHIP_REQUIRE(nq >= 0 && nq <= 0x7fffffffll && n_entries >= 0, RIHIP_ERR_ARG, "fold_in_users: nq=%lld, n_entries=%lld",
                (long long)nq, (long long)n_entries);
  RIHIP_REQUIRE(d >= 1 && d <= 256, RIHIP_ERR_ARG, "fold_in_users: d=%d outside 1..256", d);
  RIHIP_REQUIRE(n_rows >= 0 && n_rows <= 0x7fffffffll && ldv >= d && n_ids >= 0 && n_item_rows >= 0, RIHIP_ERR_ARG,
                "fold_in_users: n_rows=%lld, ldv=%lld (d=%d), n_ids=%lld, n_item_rows=%lld", (long long)n_rows,
                (long long)ldv, d, (long long)n_ids, (long long)n_item_rows);
  RIHIP_REQUIRE(min_rating >= 1 && min_rating <= 5 && (weighting == 0 || weighting == 1), RIHIP_ERR_ARG,
                "fold_in_users: min_rating=%d (1..5), weighting=%d (0 or 1)", min_rating, weighting);
  RIHIP_REQUIRE(beta >= 0.0 && beta <= 1.0, RIHIP_ERR_ARG, "fold_in_users: beta=%g outside [0, 1]", beta);
  RIHIP_REQUIRE(err, RIHIP_ERR_ARG, "fold_in_users: null error word");
  hipStream_t st = (hipStream_t)stream;
  RIHIP_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int), st));
  if (nq == 0) return RIHIP_OK;
  RIHIP_REQUIRE(hist_offsets && mu && q && rows && flags, RIHIP_ERR_ARG, "fold_in_users: null pointer");
  RIHIP_REQUIRE(n_entries == 0 || (hist_items && hist_ratings), RIHIP_ERR_ARG, "fold_in_users: null history arrays");
  RIHIP_REQUIRE(n_rows == 0 || V, RIHIP_ERR_ARG, "fold_in_users: %lld rows without a vector table", (long long)n_rows);
  RIHIP_REQUIRE(n_ids == 0 || row_of, RIHIP_ERR_ARG, "fold_in_users: %lld ids without row_of", (long long)n_ids);
  RIHIP_REQUIRE(n_item_rows == 0 || item_tab, RIHIP_ERR_ARG, "fold_in_users: %lld item rows without an item table",
                (long long)n_item_rows);
  FoldArgs a;
  a.offsets = hist_offsets; a.items = hist_items; a.ratings = hist_ratings; a.n_entries = n_entries;
  a.V = V; a.n_rows = n_rows; a.ldv = ldv; a.d = d; a.row_of = row_of; a.n_ids = n_ids; a.mu = mu;
  a.min_rating = min_rating; a.weighting = weighting; a.beta = beta;
  a.item_tab = item_tab; a.n_item_rows = n_item_rows; a.user_meta = user_meta;
  a.q = q; a.rows = rows; a.flags = flags; a.err = err;
  const bool vec = d % 4 == 0 && ldv % 4 == 0 && (reinterpret_cast<uintptr_t>(V) & 15u) == 0;
  a.lpr_shift = 0;
  while (vec && (4 << a.lpr_shift) < d) ++a.lpr_shift;
  if (vec)
    hipLaunchKernelGGL(fold_in_kernel<true>, dim3((unsigned)nq), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(fold_in_kernel<false>, dim3((unsigned)nq), dim3(256), 0, st, a);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
