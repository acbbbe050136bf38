// Mixed in-batch objective L = L_inbatch + hard_weight * L_hard on the stored-G passes (not in the reference): the hard
// negatives are mined from the weights sigma(s_ij - s_ii) that rihip_inbatch_user_pass leaves in `gmat`, not from a
// second score sweep.  For a fixed user sigma is non-decreasing in the score, so a row's hardest negatives are its
// largest stored weights, and the hard term's gradient weight sigma_ij / (n c_i) is the stored weight times a per-row
// constant: boosting the selected entries of gmat in place and correcting dU and r makes the unchanged item pass yield
// the mixed dI.  Contract: include/recommendit_hip.h (rihip_inbatch_gmat_mine / rihip_inbatch_mixed_apply).
//
// Mine (bandwidth-bound).  gmat is 32x32-blocked G^T: a row of a block is 32 consecutive users = 128 B, a user's column
// strides through the item blocks g_ub * 1024 floats apart.  One workgroup owns 32 users (one block column) and one
// split of the item range; thread t holds user t & 31 and the rows (t >> 5) + 8k of every 64-item tile, so each wave
// load is two whole 128-B rows.  The next tile's eight loads are in flight while the current one is examined.  Every
// user keeps its M = skip + m best keys so far (search_keys.h order word << 32 | ~local item) in LDS, sorted
// descending; a weight is first compared with the user's M-th key (one compare per element), the few that pass are
// queued per user with an LDS integer atomic and merged after the tile by rank counting, as in hard_select_kernel.
// Keys are distinct and totally ordered, so neither the arrival order nor the number of splits changes the result.  A
// second launch merges the splits' lists per user by rank counting and writes ranks skip .. skip+m-1.
//
// Apply: a wave per user at a time in slot order, 32 users per wave in sequence (as hard_user_kernel): boost, dU and r
// corrections, loss row.
// No float atomics, fixed summation order, no allocation, no host synchronisation: capturable in a graph.
#include <cmath>

#include "common.h"
#include "search_keys.h"

using rihip_index::f2ord;
using rihip_index::ord2f;

namespace {

constexpr int XMAXM = 64;     // skip + m at most
constexpr int XMAXN = 32;     // m at most
constexpr int XTILE = 64;     // items per tile of the mining loop (two gmat blocks)
constexpr int XROWS = 8;      // rows of a tile per thread
constexpr int XMAXSPLIT = 16; // item-range splits at most
constexpr int XOW = 128;      // users per loss part

struct MineArgs {
  const float* gmat;
  int64_t nu, u_goff, ni, i_goff, g_ub;
  int m, skip, nsplit;
  const int64_t* o_ids;      // user_pos_ids [nu], nullable together with s_ids
  const int64_t* s_ids;      // item_ids [ni]
  uint64_t* plist;           // [nsplit][32 ceil(nu/32)][M] the splits' lists, 0 = empty
  int* neg_idx;              // [nu,m]
  float* neg_w;              // [nu,m]
};

__device__ __forceinline__ int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

__global__ __launch_bounds__(256) void mine_partial_kernel(MineArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint64_t xsm[];
  const int M = a.skip + a.m;
  uint64_t* list = xsm;                      // [32][M] best keys so far, descending
  uint64_t* tmp = list + 32 * M;             // [32][M] merged list
  uint64_t* queue = tmp + 32 * M;            // [32][XTILE] survivors of the current tile
  __shared__ uint64_t thr[32];               // the user's M-th key, 0 while its list is not full (every key is > 0)
  __shared__ int lcnt[32];
  __shared__ int qcnt[32];
  const int tid = threadIdx.x, il = tid & 31, sub = tid >> 5;
  const int64_t ib = blockIdx.x;
  const int64_t i = ib * 32 + il;
  const bool uvalid = i < a.nu;
  const bool ids = a.o_ids != nullptr;
  const int64_t gu = a.u_goff + i;
  const int64_t own = (ids && uvalid) ? a.o_ids[i] : 0;
  if (tid < 32) { thr[tid] = 0ull; lcnt[tid] = 0; qcnt[tid] = 0; }
  const int64_t ntiles = cdiv64(a.ni, XTILE), per = cdiv64(ntiles, a.nsplit);
  const int64_t t0 = (int64_t)blockIdx.y * per, t1 = (t0 + per < ntiles) ? t0 + per : ntiles;
  const int64_t nblk = cdiv64(a.ni, 32);     // item blocks that hold an in-range item: the only ones read
  const float* gcol = a.gmat + (size_t)ib * 1024 + il;
  const size_t gstep = (size_t)a.g_ub * 1024;

  float v[XROWS], vn[XROWS];
  auto load_tile = [&](int64_t t, float* vv) {
#pragma unroll
    for (int k = 0; k < XROWS; ++k) {
      const int jt = sub + 8 * k;
      const int64_t jb = (t * XTILE + jt) >> 5;
      vv[k] = (t < t1 && jb < nblk) ? gcol[(size_t)jb * gstep + (jt & 31) * 32] : 0.f;
    }
  };
  load_tile(t0, v);
  __syncthreads();
  for (int64_t t = t0; t < t1; ++t) {
    load_tile(t + 1, vn);
    const uint64_t th = thr[il];
    int pushed = 0;
#pragma unroll
    for (int k = 0; k < XROWS; ++k) {
      const int64_t j = t * XTILE + sub + 8 * k;
      const bool cand = uvalid && j < a.ni && a.i_goff + j != gu;
      const uint64_t key = cand ? (((uint64_t)f2ord(v[k] + 0.f) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)j)) : 0ull;
      // the only per-weight branch, rare after the first tiles; the id mask is looked up for its survivors alone
      if (key > th && !(ids && a.s_ids[j] == own)) {
        const int slot = atomicAdd(&qcnt[il], 1);          // < XTILE: one candidate per item of the tile
        queue[il * XTILE + slot] = key;
        pushed = 1;
      }
    }
    // ---- merge the survivors: 8 threads per user, rank = number of greater keys (keys are distinct)
    if (__syncthreads_or(pushed)) {
      const int mo = tid >> 3, s8 = tid & 7;
      const int q = qcnt[mo], lc = lcnt[mo];
      if (q > 0) {
        for (int e = s8; e < lc + q; e += 8) {
          const bool old = e < lc;
          const uint64_t kk = old ? list[mo * M + e] : queue[mo * XTILE + e - lc];
          int rank = old ? e : 0;                          // the list is sorted: e greater keys inside it
          if (!old)
            for (int f = 0; f < lc; ++f) rank += list[mo * M + f] > kk ? 1 : 0;
          for (int f = 0; f < q; ++f) rank += queue[mo * XTILE + f] > kk ? 1 : 0;
          if (rank < M) tmp[mo * M + rank] = kk;
        }
      }
      __syncthreads();
      if (q > 0) {
        const int nl = lc + q < M ? lc + q : M;
        for (int e = s8; e < nl; e += 8) list[mo * M + e] = tmp[mo * M + e];
        if (s8 == 0) {
          lcnt[mo] = nl; qcnt[mo] = 0;
          thr[mo] = nl == M ? tmp[mo * M + M - 1] : 0ull;
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < XROWS; ++k) v[k] = vn[k];
  }
  // ---- the split's list of every user of the block column (ragged users: empty lists)
  __syncthreads();
  uint64_t* out = a.plist + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 32 * M;
  for (int e = tid; e < 32 * M; e += 256) {
    const int ol = e / M, p = e % M;
    out[e] = p < lcnt[ol] ? list[ol * M + p] : 0ull;
  }
}

// One wave per user: the nsplit * M keys of its lists by rank counting; ranks skip .. skip+m-1, empty slots last.
__global__ __launch_bounds__(256) void mine_merge_kernel(MineArgs a) {
  __shared__ uint64_t keys[4][XMAXSPLIT * XMAXM];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + w;
  const bool valid = i < a.nu;                             // wave-uniform
  const int M = a.skip + a.m, n = a.nsplit * M;
  const size_t per_split = (size_t)cdiv64(a.nu, 32) * 32 * M;
  int cnt = 0;
  if (valid) {
    for (int e = lane; e < n; e += 64) {
      const uint64_t kk = a.plist[(size_t)(e / M) * per_split + (size_t)i * M + e % M];
      keys[w][e] = kk;
      cnt += kk != 0ull ? 1 : 0;
    }
  }
  int total = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o, 64);
  __syncthreads();
  if (!valid) return;
  for (int e = lane; e < n; e += 64) {
    const uint64_t kk = keys[w][e];
    if (kk == 0ull) continue;
    int rank = 0;
    for (int f = 0; f < n; ++f) rank += keys[w][f] > kk ? 1 : 0;
    if (rank >= a.skip && rank < M) {
      a.neg_idx[i * a.m + rank - a.skip] = (int)(0xFFFFFFFFu - (uint32_t)kk);
      a.neg_w[i * a.m + rank - a.skip] = ord2f((uint32_t)(kk >> 32));
    }
  }
  if (lane < a.m && a.skip + lane >= total) {
    a.neg_idx[i * a.m + lane] = -1;
    a.neg_w[i * a.m + lane] = 0.f;
  }
}

// ---- apply -------------------------------------------------------------------------------------------------------
struct ApplyArgs {
  float* gmat;
  const float* users; int64_t nu, u_goff;
  const float* items; int64_t ni, i_goff;
  int64_t g_ub;
  int d, m;
  const float* pos; const int* neg_idx; const float* neg_w;
  float hw; double hw_d, nm1; float c;
  float* dU; float* r; double* loss_part;
};

// A wave works on one user at a time, lane s < m holding slot s, and walks 32 users in sequence: a workgroup of four waves
// covers 128 users = one loss part, the grid has ceil(n_users / 128) workgroups (2 048 waves at B = 65 536, about two per
// SIMD: the eight the registers allow are not reached; at 0.3 - 0.5 ms the launch is not worth a finer grid).
__global__ __launch_bounds__(256) void mixed_apply_kernel(ApplyArgs a) {
  __shared__ double row_loss[XOW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m = a.m, d = a.d;
  for (int u = 0; u < 32; ++u) {
    const int li = w * 32 + u;
    const int64_t i = (int64_t)blockIdx.x * XOW + li;
    if (i >= a.nu) {                                       // wave-uniform
      if (lane == 0) row_loss[li] = 0.0;
      continue;
    }
    int j = -1;
    float sg = 0.f;
    if (lane < m) { j = a.neg_idx[i * m + lane]; sg = a.neg_w[i * m + lane]; }
    const bool ok = lane < m && j >= 0 && (int64_t)j < a.ni;
    const int c = __popcll(__ballot(ok));
    if (c == 0 || a.hw == 0.f) {                           // wave-uniform: nothing selected, or nothing to add
      if (lane == 0) row_loss[li] = 0.0;
      continue;
    }
    const float f = (float)(1.0 + a.hw_d * a.nm1 / (double)c);
    const float sb = __fmul_rn(sg, f);                     // one rounded multiply, never fused with the subtraction
    const float dl = ok ? __fsub_rn(sb, sg) : 0.f;
    const int jv = ok ? j : -1;
    if (ok)
      a.gmat[((size_t)(j >> 5) * a.g_ub + (size_t)(i >> 5)) * 1024 + (size_t)(j & 31) * 32 + (size_t)(i & 31)] = sb;
    float D = 0.f;
    for (int s = 0; s < m; ++s) D += __shfl(dl, s, 64);    // slot order
    const int64_t drow = a.u_goff + i - a.i_goff;          // inside [0, ni): checked by the entry
    const float posi = a.pos[i];
    double ls = 0.0;
    for (int s = 0; s < m; ++s) {                          // z_ij = <u_i, y_j> - pos_i of the selected pairs, slot order
      const int jj = __shfl(jv, s, 64);
      if (jj < 0) continue;                                // wave-uniform
      float p = 0.f;
      for (int k = lane; k < d; k += 64) p = fmaf(a.users[i * d + k], a.items[(int64_t)jj * d + k], p);
      p = wave_sum(p);
      const float z = p - posi;
      ls += (double)(fmaxf(z, 0.f) + log1pf(__expf(-fabsf(z))));
    }
    if (lane == 0) {
      row_loss[li] = ls / (double)c;
      a.r[i] = fmaf(a.c, D, a.r[i]);
    }
    for (int k = lane; k < d; k += 64) {
      float acc = 0.f;
      for (int s = 0; s < m; ++s) {
        const int jj = __shfl(jv, s, 64);
        const float ds = __shfl(dl, s, 64);
        if (jj >= 0) acc = fmaf(ds, a.items[(int64_t)jj * d + k], acc);
      }
      acc = fmaf(-D, a.items[drow * d + k], acc);
      a.dU[i * d + k] = fmaf(a.c, acc, a.dU[i * d + k]);
    }
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int rr = 0; rr < XOW; ++rr) s += row_loss[rr];
    a.loss_part[blockIdx.x] = a.hw_d * a.nm1 * s;
  }
}

int64_t gmat_ub(int64_t n_users) { return 8 * ((n_users + 255) / 256); }

int mine_max_nsplit(int64_t n_items) {
  const int64_t ntiles = (n_items + XTILE - 1) / XTILE;
  return (int)(ntiles < XMAXSPLIT ? ntiles : XMAXSPLIT);
}

// Four workgroups per CU at small batches (measured at B = 8192: 1 / 2 / 4 / 8 / 16 splits take 0.37 / 0.23 / 0.17 /
// 0.23 / 0.28 ms), and never fewer than two splits, which even out the tail of the grid once the block columns alone
// fill the chip (B = 65536: 4.9 / 4.3 / 4.3 / 4.9 / 5.7 ms).  The result does not depend on the choice.
int mine_auto_nsplit(int64_t n_users, int64_t n_items) {
  const int64_t nub = (n_users + 31) / 32;
  int64_t want = (4 * RIHIP_NCU + nub - 1) / nub;
  if (want < 2) want = 2;
  const int mx = mine_max_nsplit(n_items);
  return (int)(want > mx ? mx : want);
}

int check_shape(const char* who, int m, int skip, int64_t n_users, int64_t user_goff, int64_t n_items,
                int64_t item_goff) {
  RIHIP_REQUIRE(m >= 1 && m <= XMAXN && skip >= 0 && skip + m <= XMAXM, RIHIP_ERR_ARG,
                "%s: m=%d skip=%d need 1 <= m <= %d, skip >= 0 and skip + m <= %d", who, m, skip, XMAXN, XMAXM);
  RIHIP_REQUIRE(n_users > 0 && n_items > 0 && n_items < (1ll << 31) && n_users < (1ll << 31) / (XMAXN + 1),
                RIHIP_ERR_ARG, "%s: sizes users=%lld items=%lld (items below 2^31, users below 2^31 / %d)", who,
                (long long)n_users, (long long)n_items, XMAXN + 1);
  RIHIP_REQUIRE(user_goff >= item_goff && user_goff + n_users <= item_goff + n_items, RIHIP_ERR_ARG,
                "%s: users [%lld, %lld) have partners outside the given items [%lld, %lld)", who, (long long)user_goff,
                (long long)(user_goff + n_users), (long long)item_goff, (long long)(item_goff + n_items));
  return RIHIP_OK;
}

}  // namespace

extern "C" int rihip_inbatch_gmat_mine_max_nsplit(int64_t n_items) {
  return n_items > 0 ? mine_max_nsplit(n_items) : -1;
}

extern "C" int64_t rihip_inbatch_gmat_mine_workspace_bytes(int64_t n_users, int64_t n_items, int m, int skip,
                                                           int nsplit) {
  if (n_users <= 0 || n_items <= 0 || n_items >= (1ll << 31) || n_users >= (1ll << 31) / (XMAXN + 1) || m < 1 ||
      m > XMAXN || skip < 0 || skip + m > XMAXM || nsplit < 0 || nsplit > mine_max_nsplit(n_items))
    return -1;
  const int ns = nsplit ? nsplit : mine_auto_nsplit(n_users, n_items);
  return (int64_t)sizeof(uint64_t) * ns * ((n_users + 31) / 32) * 32 * (skip + m);
}

extern "C" int rihip_inbatch_gmat_mine(const float* gmat, int64_t n_users, int64_t user_goff, int64_t n_items,
                                       int64_t item_goff, int m, int skip, const int64_t* user_pos_ids,
                                       const int64_t* item_ids, int nsplit, int* neg_idx, float* neg_w,
                                       void* workspace, void* stream) {
  const int rc = check_shape("inbatch_gmat_mine", m, skip, n_users, user_goff, n_items, item_goff);
  if (rc != RIHIP_OK) return rc;
  RIHIP_REQUIRE((user_pos_ids == nullptr) == (item_ids == nullptr), RIHIP_ERR_ARG,
                "inbatch_gmat_mine: user_pos_ids and item_ids must be given together or both be null");
  RIHIP_REQUIRE(nsplit >= 0 && nsplit <= mine_max_nsplit(n_items), RIHIP_ERR_ARG,
                "inbatch_gmat_mine: nsplit=%d need 0 (the library's choice) or 1 .. %d for %lld items", nsplit,
                mine_max_nsplit(n_items), (long long)n_items);
  RIHIP_REQUIRE(gmat && neg_idx && neg_w && workspace, RIHIP_ERR_ARG, "inbatch_gmat_mine: null pointer");
  MineArgs a;
  a.gmat = gmat; a.nu = n_users; a.u_goff = user_goff; a.ni = n_items; a.i_goff = item_goff;
  a.g_ub = gmat_ub(n_users); a.m = m; a.skip = skip;
  a.nsplit = nsplit ? nsplit : mine_auto_nsplit(n_users, n_items);
  a.o_ids = user_pos_ids; a.s_ids = item_ids; a.plist = (uint64_t*)workspace; a.neg_idx = neg_idx; a.neg_w = neg_w;
  const int M = skip + m;
  const size_t lds = sizeof(uint64_t) * ((size_t)64 * M + 32 * XTILE);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mine_partial_kernel, dim3((unsigned)((n_users + 31) / 32), (unsigned)a.nsplit), dim3(256), lds, st,
                     a);
  RIHIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(mine_merge_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, a);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int64_t rihip_inbatch_mixed_loss_parts(int64_t n_users) { return (n_users + XOW - 1) / XOW; }

extern "C" int rihip_inbatch_mixed_apply(float* gmat, const float* users, int64_t n_users, int64_t user_goff,
                                         const float* items, int64_t n_items, int64_t item_goff, int d, const float* pos,
                                         int m, const int* neg_idx, const float* neg_w, float hard_weight,
                                         int64_t n_global, float* d_users, float* r, double* loss_part, void* stream) {
  const int rc = check_shape("inbatch_mixed_apply", m, 0, n_users, user_goff, n_items, item_goff);
  if (rc != RIHIP_OK) return rc;
  RIHIP_REQUIRE(d == 32 || d == 64 || d == 128, RIHIP_ERR_SHAPE,
                "inbatch_mixed_apply: unsupported embed_dim=%d (the stored-G passes take 32, 64 or 128)", d);
  RIHIP_REQUIRE(n_global >= 2, RIHIP_ERR_ARG, "inbatch_mixed_apply: B=%lld must be >= 2", (long long)n_global);
  RIHIP_REQUIRE(std::isfinite(hard_weight) && hard_weight >= 0.f, RIHIP_ERR_ARG,
                "inbatch_mixed_apply: hard_weight=%g must be finite and >= 0", (double)hard_weight);
  RIHIP_REQUIRE(gmat && users && items && pos && neg_idx && neg_w && d_users && r && loss_part, RIHIP_ERR_ARG,
                "inbatch_mixed_apply: null pointer");
  ApplyArgs a;
  a.gmat = gmat; a.users = users; a.nu = n_users; a.u_goff = user_goff; a.items = items; a.ni = n_items;
  a.i_goff = item_goff; a.g_ub = gmat_ub(n_users); a.d = d; a.m = m; a.pos = pos; a.neg_idx = neg_idx; a.neg_w = neg_w;
  a.hw = hard_weight; a.hw_d = (double)hard_weight; a.nm1 = (double)(n_global - 1);
  a.c = (float)(1.0 / ((double)n_global * (double)(n_global - 1)));
  a.dU = d_users; a.r = r; a.loss_part = loss_part;
  hipLaunchKernelGGL(mixed_apply_kernel, dim3((unsigned)((n_users + XOW - 1) / XOW)), dim3(256), 0, (hipStream_t)stream,
                     a);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
