// Validation by exact full-catalogue ranks (not in the reference, which evaluates once, after training, from top-k
// lists: src/pipelines/run_pipeline.py:166-220).  For every held-out (user, target) pair: the number of non-excluded
// items that outrank the target -- no list, no over-fetch, no selection.  Contract: include/recommendit_hip.h.
//
// Three kernels, all on the skeleton of gen_sweep.h (exact-f32 MFMA, wg_gemm<false>, one product):
// * rank_pair_score_kernel: s for the entries (user row, item row) = every pair's target, then every exclusion entry.
//   32 entries per owner group: their user rows go to Os through the entry list, their item rows are gathered into the
//   workgroup's own 32-row slab of the workspace, and the 32 x 32 product's diagonal is kept (the diag_s idiom of
//   hard_select_kernel).  An element's accumulation chain in wg_gemm depends only on its two rows, so these are the
//   bits the sweep below computes for the same rows: a row compared with a bytewise equal row ties exactly.  The grid
//   is capped and strides over the groups, so the slabs are RP_GRID * 32 * d floats whatever n_excl is.
// * rank_count_kernel: owners = pairs (user row through pair_user), swept set = all of Y, split over blockIdx.y by
//   whole 128-row tiles.  Epilogue per accumulator element: two float compares and an index compare against the owner's
//   threshold held in registers, added to one of 16 register counters; no branch per score.  The counters are reduced
//   over the 32 lanes of a row once per owner group and added to rank[p] with an integer atomic: partial counts add
//   exactly, so the result does not depend on the split.
// * rank_correct_kernel: one wave per pair walks the user's exclusion row and takes back the entries that the sweep
//   counted (same scores, same rule), and writes -1 for a target outside the catalogue.
// rihip_eval_ranks turns ranks into the per-user outputs of rihip_eval_topk (eval.hip), one wave per user.
#include "common.h"
#include "gen_sweep.h"
#include "recommendit_hip.h"

using namespace rihip_gen;

namespace {

constexpr int RP_GRID = 1024;         // workgroups of the pair-score kernel at most = slabs in the workspace
constexpr int RC_BLOCKS = 512;        // workgroups the count sweep aims at (2 per CU)
constexpr int EVAL_MAX_K = 64;        // requested k values, one lane each (eval.hip)

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// workspace layout (bytes), all 256-B aligned: pair_user i32 [n_pairs] | excl_score f32 [n_excl] | slabs f32 [g][32][d]
struct RankWs {
  int* pair_user; float* excl_score; float* slabs; size_t total;
};
int64_t score_groups(int64_t n_pairs, int64_t n_excl) { return (n_pairs + n_excl + 31) / 32; }
void rank_ws_layout(int64_t n_pairs, int64_t n_excl, int d, void* base, RankWs* ws) {
  const int64_t ng = score_groups(n_pairs, n_excl);
  const int64_t g = ng < RP_GRID ? ng : RP_GRID;
  size_t off = 0;
  char* b = (char*)base;
  ws->pair_user = (int*)(b + off); off += align256(sizeof(int) * (size_t)n_pairs);
  ws->excl_score = (float*)(b + off); off += align256(sizeof(float) * (size_t)n_excl);
  ws->slabs = (float*)(b + off); off += align256(sizeof(float) * (size_t)g * 32 * d);
  ws->total = off;
}

struct RankArgs {
  const float* U; int64_t n_users;
  const float* Y; int64_t n_items;
  int D;
  const int64_t* pair_off; const int* pair_item; int64_t n_pairs;
  const int64_t* excl_off; const int* excl_items; int64_t n_excl;   // excl_off null: no exclusion
  int* pair_user; float* excl_score; float* slabs;
  int* rank; float* target_score; int* err;
  int64_t tiles_per_split;
};

// the row of a CSR that holds entry x: the largest u in [0, n) with off[u] <= x (rows may be empty); reads off[1..n]
__device__ __forceinline__ int64_t csr_row_of(const int64_t* off, int64_t n, int64_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid + 1] <= x) lo = mid + 1; else hi = mid;
  }
  return lo < n ? lo : n - 1;
}

__global__ __launch_bounds__(256) void rank_pair_score_kernel(RankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D, ldo = gen_ldo(D);
  float* Os = smem;                      // [32][ldo] the entries' user rows
  float* Wp = Os + 32 * ldo;             // [256][GLDP] k-panel of the slab
  __shared__ int su[32];                 // user row of the entry, -1 = no entry
  __shared__ int sj[32];                 // item row of the entry, -1 = none or outside the catalogue
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r31 = lane & 31;
  float* slab = a.slabs + (size_t)blockIdx.x * 32 * D;
  const int64_t n_ent = a.n_pairs + a.n_excl, ng = (n_ent + 31) / 32;
  for (int64_t g = blockIdx.x; g < ng; g += gridDim.x) {
    __syncthreads();                     // the previous group's readers of su / sj / Os are done
    if (tid < 32) {
      const int64_t e = g * 32 + tid;
      int u = -1, j = -1;
      if (e < a.n_pairs) {
        u = (int)csr_row_of(a.pair_off, a.n_users, e);
        j = a.pair_item[e];
        a.pair_user[e] = u;
        if (j < 0 || (int64_t)j >= a.n_items) { j = -1; atomicOr(a.err, 2); a.target_score[e] = 0.f; }
      } else if (e < n_ent) {
        const int64_t x = e - a.n_pairs;
        u = (int)csr_row_of(a.excl_off, a.n_users, x);
        j = a.excl_items[x];
        if (j < 0 || (int64_t)j >= a.n_items) { j = -1; atomicOr(a.err, 1); a.excl_score[x] = 0.f; }
      }
      su[tid] = u; sj[tid] = j;
    }
    __syncthreads();
    for (int idx = tid; idx < 32 * D; idx += 256) {
      const int r = idx / D, k = idx % D;
      const int u = su[r], j = sj[r];
      Os[r * ldo + k] = u >= 0 ? a.U[(int64_t)u * D + k] : 0.f;
      slab[r * D + k] = j >= 0 ? a.Y[(int64_t)j * D + k] : 0.f;
    }
    __syncthreads();                     // the slab is complete before wg_gemm's first panel load reads it
    f32x16 sacc[GNT];
    wg_gemm<false>(Os, ldo, D, slab, D, 32, Wp, sacc, tid);                            // S = O.slab^T, wave 0 only
    if (w == 0) {
      const int j = sj[r31];
      const int64_t e = g * 32 + r31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (acc_row(r, lane) == r31 && j >= 0) {           // the diagonal: one element of one lane per entry
          const float s = sacc[0][r] + 0.f;                // -0 -> +0: one score
          if (e < a.n_pairs) a.target_score[e] = s;
          else a.excl_score[e - a.n_pairs] = s;
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void rank_count_kernel(RankArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D, ldo = gen_ldo(D);
  float* Os = smem;                      // [32][ldo] the pairs' user rows
  float* Wp = Os + 32 * ldo;             // [256][GLDP] k-panel of the tile (no Gs, no red)
  __shared__ int su[32];
  __shared__ int stt[32];                // target row
  __shared__ float sst[32];              // target score
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r31 = lane & 31;
  const int64_t ntiles = (a.n_items + GSW - 1) / GSW;
  const int64_t t0 = (int64_t)blockIdx.y * a.tiles_per_split;
  const int64_t t1 = t0 + a.tiles_per_split < ntiles ? t0 + a.tiles_per_split : ntiles;
  for (int og = 0; og < GOG; ++og) {
    const int64_t o_base = owner_base(og);
    if (o_base >= a.n_pairs) break;
    __syncthreads();                     // the previous group's readers of Os and of the thresholds are done
    if (tid < 32) {
      const int64_t p = o_base + tid;
      const bool ok = p < a.n_pairs;
      su[tid] = ok ? a.pair_user[p] : -1;
      stt[tid] = ok ? a.pair_item[p] : -1;
      sst[tid] = ok ? a.target_score[p] : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < 32 * D; idx += 256) {
      const int r = idx / D, k = idx % D;
      const int u = su[r];
      Os[r * ldo + k] = u >= 0 ? a.U[(int64_t)u * D + k] : 0.f;
    }
    float st[16];
    int tt[16], cnt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ol = acc_row(r, lane);
      st[r] = sst[ol]; tt[r] = stt[ol]; cnt[r] = 0;
    }
    for (int64_t tile = t0; tile < t1; ++tile) {
      const int64_t sb = tile * GSW;
      const int nsw = (a.n_items - sb < GSW) ? (int)(a.n_items - sb) : GSW;
      f32x16 sacc[GNT];
      wg_gemm<false>(Os, ldo, D, a.Y + sb * D, D, nsw, Wp, sacc, tid);                 // S = O.Y^T
      const int64_t jl = sb + w * 32 + r31;
      const int j = (int)jl;
      const int s_ok = jl < a.n_items ? 1 : 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float s = sacc[0][r] + 0.f;
        // j == t neither exceeds nor precedes itself: the target is never counted
        const int out = (s > st[r]) | ((s == st[r]) & (j < tt[r]));
        cnt[r] += out & s_ok;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      int v = cnt[r];
      v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
      v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64);
      const int64_t p = o_base + acc_row(r, lane);
      if (r31 == 0 && p < a.n_pairs && v != 0) atomicAdd(&a.rank[p], v);
    }
  }
}

// one wave per pair
__global__ __launch_bounds__(256) void rank_correct_kernel(RankArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= a.n_pairs) return;
  const int t = a.pair_item[p];
  if (t < 0 || (int64_t)t >= a.n_items) {
    if (lane == 0) a.rank[p] = -1;
    return;
  }
  if (!a.excl_off) return;
  const int u = a.pair_user[p];
  const float st = a.target_score[p];
  int64_t e0 = a.excl_off[u], e1 = a.excl_off[u + 1];
  e0 = e0 < 0 ? 0 : e0;
  e1 = e1 > a.n_excl ? a.n_excl : e1;
  int c = 0;
  for (int64_t e = e0 + lane; e < e1; e += 64) {
    const int j = a.excl_items[e];
    if (j >= 0 && (int64_t)j < a.n_items && j != t) {
      const float s = a.excl_score[e];
      c += (s > st || (s == st && j < t)) ? 1 : 0;
    }
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0 && c != 0) {
    const int r = a.rank[p] - c;
    a.rank[p] = r < 0 ? 0 : r;
  }
}

size_t count_lds(int D) { return sizeof(float) * ((size_t)32 * gen_ldo(D) + 256 * GLDP); }

struct KList {
  int n;
  int kmax;
  int k[EVAL_MAX_K];
};

// one wave per user: the user's ranks in ascending order, lane j keeping the running DCG / hit count of the j-th k
__global__ __launch_bounds__(256) void eval_ranks_kernel(const int* __restrict__ rank, const int64_t* __restrict__ off,
                                                         int64_t n, int64_t n_pairs, const int64_t* __restrict__ raw,
                                                         KList kl, const double* __restrict__ disc,
                                                         const double* __restrict__ idcg, double* __restrict__ vals,
                                                         double* __restrict__ rr, uint8_t* __restrict__ scored) {
  const int lane = threadIdx.x & 63;
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
  int my_k = 0;
#pragma unroll
  for (int j = 0; j < EVAL_MAX_K; ++j)
    if (j == lane) my_k = kl.k[j];
  const int nk = kl.n;
  for (int64_t row = wave0; row < n; row += nwaves) {
    int64_t s0 = off[row], s1 = off[row + 1];
    s0 = s0 < 0 ? 0 : s0;
    s1 = s1 > n_pairs ? n_pairs : s1;
    const int64_t cnt = s1 - s0;
    const int64_t nraw = raw ? raw[row] : cnt;
    if (nraw <= 0 || cnt <= 0) {
      if (lane < nk) {
        double* v = vals + (row * nk + lane) * 3;
        v[0] = 0.0; v[1] = 0.0; v[2] = 0.0;
      }
      if (lane == 0) { rr[row] = 0.0; scored[row] = 0; }
      continue;
    }
    double dcg = 0.0;
    int hits = 0;
    int64_t first = -1, prev = -1;
    for (;;) {                           // the smallest rank above prev: hits in position order
      int64_t best = INT64_MAX;
      for (int64_t e = s0 + lane; e < s1; e += 64) {
        const int64_t r = rank[e];
        if (r > prev && r < best) best = r;      // rank -1 (a target outside the catalogue) is a miss
      }
      for (int o = 32; o > 0; o >>= 1) {
        const int64_t other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
      }
      if (best == INT64_MAX) break;
      if (first < 0) first = best;
      if (best >= kl.kmax) break;        // nothing further can change a value
      if (best < my_k) { dcg += disc[best]; ++hits; }
      prev = best;
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

bool sizes_ok(int64_t n_pairs, int64_t n_excl, int d) {
  return n_pairs >= 0 && n_pairs < (1ll << 31) && n_excl >= 0 && n_excl < (1ll << 40) && gen_width_ok(d);
}

}  // namespace

extern "C" int64_t rihip_rank_targets_workspace_bytes(int64_t n_pairs, int64_t n_excl, int d) {
  if (!sizes_ok(n_pairs, n_excl, d)) return -1;
  RankWs ws;
  rank_ws_layout(n_pairs, n_excl, d, nullptr, &ws);
  return (int64_t)(ws.total > 256 ? ws.total : 256);
}

extern "C" int rihip_rank_targets(const float* U, int64_t n_users, const float* Y, int64_t n_items, int d,
                                  const int64_t* pair_offsets, const int32_t* pair_item, int64_t n_pairs,
                                  const int64_t* excl_offsets, const int32_t* excl_items, int64_t n_excl,
                                  int grid_splits, int32_t* rank, float* target_score, int* err, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
  RIHIP_REQUIRE(gen_width_ok(d), RIHIP_ERR_ARG, "rank_targets: unsupported embed_dim=%d (multiples of 16 up to 256)", d);
  RIHIP_REQUIRE(n_pairs >= 0 && n_pairs < (1ll << 31) && n_items >= 0 && n_items < (1ll << 31) && n_users >= 0,
                RIHIP_ERR_ARG, "rank_targets: sizes users=%lld items=%lld pairs=%lld (items and pairs below 2^31)",
                (long long)n_users, (long long)n_items, (long long)n_pairs);
  RIHIP_REQUIRE(err, RIHIP_ERR_ARG, "rank_targets: null error word");
  RIHIP_REQUIRE(grid_splits >= 0, RIHIP_ERR_ARG, "rank_targets: grid_splits=%d < 0", grid_splits);
  if (!excl_offsets) n_excl = 0;
  RIHIP_REQUIRE(sizes_ok(n_pairs, n_excl, d), RIHIP_ERR_ARG, "rank_targets: n_excl=%lld out of range", (long long)n_excl);
  RIHIP_REQUIRE(n_excl == 0 || excl_items, RIHIP_ERR_ARG, "rank_targets: exclusion offsets without items");
  hipStream_t st = (hipStream_t)stream;
  if (n_pairs == 0) {
    RIHIP_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int), st));
    return RIHIP_OK;
  }
  RIHIP_REQUIRE(U && Y && pair_offsets && pair_item && rank && target_score && workspace, RIHIP_ERR_ARG,
                "rank_targets: null pointer");
  RIHIP_REQUIRE(n_users > 0 && n_items > 0, RIHIP_ERR_ARG, "rank_targets: %lld pairs over %lld users and %lld items",
                (long long)n_pairs, (long long)n_users, (long long)n_items);
  RankWs ws;
  rank_ws_layout(n_pairs, n_excl, d, workspace, &ws);
  RIHIP_REQUIRE(workspace_bytes >= (int64_t)ws.total, RIHIP_ERR_ARG, "rank_targets: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)ws.total);
  static bool granted = false;
  if (!granted) {
    RIHIP_CHECK_HIP(grant_dynamic_lds(reinterpret_cast<const void*>(rank_pair_score_kernel), count_lds(256)));
    RIHIP_CHECK_HIP(grant_dynamic_lds(reinterpret_cast<const void*>(rank_count_kernel), count_lds(256)));
    granted = true;
  }
  RIHIP_CHECK_HIP(hipMemsetAsync(err, 0, sizeof(int), st));
  RIHIP_CHECK_HIP(hipMemsetAsync(rank, 0, sizeof(int32_t) * (size_t)n_pairs, st));
  const int64_t nblk = (n_pairs + GOW - 1) / GOW, ntiles = (n_items + GSW - 1) / GSW;
  int64_t splits = grid_splits > 0 ? grid_splits : (RC_BLOCKS + nblk - 1) / nblk;
  if (splits > ntiles) splits = ntiles;
  if (splits > 65535) splits = 65535;
  if (splits < 1) splits = 1;
  RankArgs a;
  a.U = U; a.n_users = n_users; a.Y = Y; a.n_items = n_items; a.D = d;
  a.pair_off = pair_offsets; a.pair_item = pair_item; a.n_pairs = n_pairs;
  a.excl_off = excl_offsets; a.excl_items = excl_items; a.n_excl = n_excl;
  a.pair_user = ws.pair_user; a.excl_score = ws.excl_score; a.slabs = ws.slabs;
  a.rank = rank; a.target_score = target_score; a.err = err;
  a.tiles_per_split = (ntiles + splits - 1) / splits;
  const int64_t ng = score_groups(n_pairs, n_excl);
  hipLaunchKernelGGL(rank_pair_score_kernel, dim3((unsigned)(ng < RP_GRID ? ng : RP_GRID)), dim3(256), count_lds(d), st,
                     a);
  RIHIP_CHECK_LAUNCH();
  const unsigned gy = (unsigned)((ntiles + a.tiles_per_split - 1) / a.tiles_per_split);
  hipLaunchKernelGGL(rank_count_kernel, dim3((unsigned)nblk, gy), dim3(256), count_lds(d), st, a);
  RIHIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(rank_correct_kernel, dim3((unsigned)((n_pairs + 3) / 4)), dim3(256), 0, st, a);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int rihip_eval_ranks(const int32_t* rank, const int64_t* pair_offsets, int64_t n_users, int64_t n_pairs,
                                const int64_t* gt_raw, const int* k_values, int n_k, const double* disc,
                                const double* idcg, int n_tab, double* vals, double* rr, uint8_t* scored,
                                void* stream) {
  RIHIP_REQUIRE(pair_offsets && k_values && disc && idcg && vals && rr && scored && (rank || n_pairs == 0),
                RIHIP_ERR_ARG, "eval_ranks: null pointer");
  RIHIP_REQUIRE(n_users >= 0 && n_pairs >= 0 && n_pairs < (1ll << 31), RIHIP_ERR_ARG,
                "eval_ranks: sizes users=%lld pairs=%lld", (long long)n_users, (long long)n_pairs);
  RIHIP_REQUIRE(n_k >= 1 && n_k <= EVAL_MAX_K, RIHIP_ERR_ARG, "eval_ranks: %d k values (1..%d)", n_k, EVAL_MAX_K);
  KList kl;
  kl.n = n_k;
  kl.kmax = 0;
  for (int j = 0; j < EVAL_MAX_K; ++j) kl.k[j] = 0;
  for (int j = 0; j < n_k; ++j) {
    RIHIP_REQUIRE(k_values[j] >= 0, RIHIP_ERR_ARG, "eval_ranks: k=%d < 0", k_values[j]);
    kl.k[j] = k_values[j];
    if (k_values[j] > kl.kmax) kl.kmax = k_values[j];
  }
  // disc[p] is read for p < k, idcg[m] for m <= k
  RIHIP_REQUIRE(n_tab > kl.kmax, RIHIP_ERR_ARG, "eval_ranks: discount table of %d entries, max k %d", n_tab, kl.kmax);
  if (n_users == 0) return RIHIP_OK;
  const int64_t nb = (n_users + 3) / 4;
  const unsigned grid = (unsigned)(nb < 8192 ? nb : 8192);
  hipLaunchKernelGGL(eval_ranks_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, rank, pair_offsets, n_users,
                     n_pairs, gt_raw, kl, disc, idcg, vals, rr, scored);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
