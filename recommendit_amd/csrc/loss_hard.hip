// In-batch hard-negative BPR: every user trains against the m highest-scoring other items of the batch (online hard-
// negative mining; not in the reference).  Runtime-width, exact-f32 MFMA, any embedding width that is a multiple of 16
// up to 256.
//
// Contract.  A row's global index is its offset argument plus its local index.  User i (global gu = user_goff + i) has
// the item of global index gu as its positive partner; every user's partner lies inside the given items.
//   score     s_ij = <u_i, y_j> (exact-f32 MFMA), s_ii = the partner's score from the same sweep
//   eligible  item j for user i iff j is not i's partner and, when id arrays are given, item_ids[j] != user_pos_ids[i]
//   order     eligible items by (score descending, global item index ascending); -0 and +0 are one score
//   N_i       the items at ranks skip .. skip+m-1 of that order (fewer may exist); c_i = |N_i|
//   loss      (1/n_global) sum_i [c_i > 0] (1/c_i) sum_{j in N_i} softplus(s_ij - s_ii)
//   w_ij = sigma(s_ij - s_ii) / (n_global c_i),  W_i = sum_j w_ij
//   dU_i = sum_{j in N_i} w_ij y_j - W_i y_partner      dI_j = sum_{i: j in N_i} w_ij u_i - [j partner of i] W_i u_i
//
// Select sweep (skeleton: gen_sweep.h, the score product only).  Every owner keeps its M = skip + m best candidates so
// far as a list of 64-bit keys (score order word << 32 | ~row, search_keys.h) in LDS, sorted descending.  A score is
// first compared with the owner's M-th key; the few that pass are queued per owner with an LDS integer atomic and
// merged into the list after the tile by rank counting.  Keys are distinct and totally ordered, so the merged list does
// not depend on the order of arrival: the result is bitwise reproducible.  No float atomics anywhere.
//
// Gradients: one wave per user gathers its <= m + 1 item rows in slot order (dU, the loss row, the pair weights); the
// n_users (m + 1) (item, pair) entries are sorted stably by item (rocprim radix sort, the partner term is slot m, empty
// slots go to a sentinel item) and one wave per item walks its run in ascending pair order (dI).  No allocation, no
// host synchronisation: capturable in a graph.
#include <cmath>
#include <cstring>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "gen_sweep.h"
#include "search_keys.h"

using namespace rihip_gen;
using rihip_index::f2ord;
using rihip_index::ord2f;

namespace {

constexpr int HMAXM = 64;   // skip + m at most
constexpr int HMAXN = 32;   // m at most

struct SelectArgs {
  const float* Xo;           // users [No,d]
  int64_t No, o_goff;
  const float* Ys;           // items [Ns,d]
  int64_t Ns, s_goff;
  int D, m, skip;
  const int64_t* o_ids;      // user_pos_ids [No], nullable together with s_ids
  const int64_t* s_ids;      // item_ids [Ns]
  int* neg_idx;              // [No,m]
  float* neg_score;          // [No,m]
  float* pos_score;          // [No]
};

__global__ __launch_bounds__(256) void hard_select_kernel(SelectArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D, M = a.skip + a.m;
  const int ldo = gen_ldo(D);
  float* Os = smem;                                                  // [32][ldo] owners
  float* Wp = Os + 32 * ldo;                                         // [256][GLDP] k-panel of the tile (no Gs, no red)
  uint64_t* list = reinterpret_cast<uint64_t*>(Wp + 256 * GLDP);     // [32][M] best keys so far, descending
  uint64_t* queue = list + 32 * M;                                   // [32][GSW] survivors of the current tile
  uint64_t* tmp = reinterpret_cast<uint64_t*>(Wp);                   // [32][HMAXM] merged list (the panel is idle then)
  __shared__ int64_t own_id[32];       // user_pos_ids of the 32 owners
  __shared__ uint64_t thr[32];         // the owner's M-th key, 0 while its list is not full (every key is > 0)
  __shared__ int lcnt[32];             // list length
  __shared__ int qcnt[32];             // queue length
  __shared__ float diag_s[32];         // s_ii, written by the one lane that meets the diagonal
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r31 = lane & 31;
  const bool ids = a.o_ids != nullptr;
  for (int og = 0; og < GOG; ++og) {
    const int64_t o_base = owner_base(og);
    if (o_base >= a.No) break;
    stage_owners(Os, ldo, a.Xo, o_base, a.No, D, tid);
    if (tid < 32) {
      own_id[tid] = (ids && o_base + tid < a.No) ? a.o_ids[o_base + tid] : 0;
      thr[tid] = 0ull; lcnt[tid] = 0; qcnt[tid] = 0; diag_s[tid] = 0.f;
    }
    const int64_t og0 = a.o_goff + o_base;
    for (int64_t sb = 0; sb < a.Ns; sb += GSW) {
      const int nsw = (a.Ns - sb < GSW) ? (int)(a.Ns - sb) : GSW;
      f32x16 sacc[GNT];
      wg_gemm<false>(Os, ldo, D, a.Ys + sb * D, D, nsw, Wp, sacc, tid);                // S = O.Y^T
      const TileLane tl = tile_lane(sb, w, r31, a.Ns, a.s_goff);
      const int64_t id_s = swept_id(ids, a.s_ids, tl);
      const uint32_t low = 0xFFFFFFFFu - (uint32_t)tl.srow;   // local row: the same order as the global index
      int pushed = 0;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const TileElem e = tile_elem(r, lane, o_base, a.No, a.o_goff, tl);
        const int ol = e.ol;
        const float s = sacc[0][r] + 0.f;                  // -0 -> +0: one score, one order word
        const bool elig = e.valid && !e.diag && !masked(ids, e.diag, id_s, own_id[ol]);
        const uint64_t key = elig ? (((uint64_t)f2ord(s) << 32) | (uint64_t)low) : 0ull;
        if (key > thr[ol]) {                               // the only per-score branch: rare after the first tiles
          const int slot = atomicAdd(&qcnt[ol], 1);        // < GSW: one candidate per swept row of the tile
          queue[ol * GSW + slot] = key;
          pushed = 1;
        }
      }
      // the diagonal crosses this wave's 32 x 32 tile in one of n_items / 32 tiles only (wave-uniform test)
      const int64_t wg0 = a.s_goff + sb + w * 32;
      if (wg0 < og0 + 32 && og0 < wg0 + 32) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const TileElem e = tile_elem(r, lane, o_base, a.No, a.o_goff, tl);
          if (e.valid && e.diag) diag_s[e.ol] = sacc[0][r] + 0.f;
        }
      }
      // ---- merge the survivors: 8 threads per owner, rank = number of greater keys (keys are distinct)
      if (__syncthreads_or(pushed)) {
        const int mo = tid >> 3, sub = tid & 7;
        const int q = qcnt[mo], lc = lcnt[mo];
        if (q > 0) {
          for (int e = sub; e < lc + q; e += 8) {
            const bool old = e < lc;
            const uint64_t k = old ? list[mo * M + e] : queue[mo * GSW + e - lc];
            int rank = old ? e : 0;                        // the list is sorted: e greater keys inside it
            if (!old)
              for (int f = 0; f < lc; ++f) rank += list[mo * M + f] > k ? 1 : 0;
            for (int f = 0; f < q; ++f) rank += queue[mo * GSW + f] > k ? 1 : 0;
            if (rank < M) tmp[mo * HMAXM + rank] = k;
          }
        }
        __syncthreads();
        if (q > 0) {
          const int nl = lc + q < M ? lc + q : M;
          for (int e = sub; e < nl; e += 8) list[mo * M + e] = tmp[mo * HMAXM + e];
          if (sub == 0) {
            lcnt[mo] = nl; qcnt[mo] = 0;
            thr[mo] = nl == M ? tmp[mo * HMAXM + M - 1] : 0ull;
          }
        }
      }
    }
    // ---- epilogue of the owner group: ranks skip .. skip+m-1, empty slots last
    __syncthreads();
    for (int idx = tid; idx < 32 * a.m; idx += 256) {
      const int ol = idx / a.m, s = idx % a.m;
      const int64_t orow = o_base + ol;
      if (orow < a.No) {
        const int pos = a.skip + s;
        int j = -1;
        float sc = 0.f;
        if (pos < lcnt[ol]) {
          const uint64_t k = list[ol * M + pos];
          j = (int)(0xFFFFFFFFu - (uint32_t)k);
          sc = ord2f((uint32_t)(k >> 32));
        }
        a.neg_idx[orow * a.m + s] = j;
        a.neg_score[orow * a.m + s] = sc;
      }
    }
    if (tid < 32 && o_base + tid < a.No) a.pos_score[o_base + tid] = diag_s[tid];
  }
}

size_t select_lds(int D, int M) {
  return sizeof(float) * ((size_t)32 * gen_ldo(D) + 256 * GLDP) + sizeof(uint64_t) * ((size_t)32 * M + 32 * GSW);
}

// ---- gradients ---------------------------------------------------------------------------------------------------
struct GradArgs {
  const float* users; int64_t nu, u_goff;
  const float* items; int64_t ni, i_goff;
  int d, m;
  const int* neg_idx; const float* neg_score; const float* pos_score;
  int64_t n_global;
  float* dU; float* dI; double* loss_part;
  uint32_t* keys_in; uint32_t* keys_out; int* vals_in; int* vals_out; float* wbuf;
};

// One wave per user, 128 users (one loss part) per workgroup.  Lane s < m holds slot s.
__global__ __launch_bounds__(256) void hard_user_kernel(GradArgs a) {
  __shared__ double row_loss[GOW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int m = a.m, m1 = a.m + 1, d = a.d;
  for (int u = 0; u < 32; ++u) {
    const int li = w * 32 + u;
    const int64_t i = (int64_t)blockIdx.x * GOW + li;
    if (i >= a.nu) {                                       // wave-uniform
      if (lane == 0) row_loss[li] = 0.0;
      continue;
    }
    int j = -1;
    float sc = 0.f;
    if (lane < m) { j = a.neg_idx[i * m + lane]; sc = a.neg_score[i * m + lane]; }
    const bool ok = lane < m && j >= 0 && (int64_t)j < a.ni;
    const int c = __popcll(__ballot(ok));
    const float z = sc - a.pos_score[i];
    const float sig = 1.f / (1.f + __expf(-z));
    const float sp = fmaxf(z, 0.f) + log1pf(__expf(-fabsf(z)));
    const float scale = c > 0 ? (float)(1.0 / ((double)a.n_global * (double)c)) : 0.f;
    const float wv = ok ? sig * scale : 0.f;
    const float spv = ok ? sp : 0.f;
    const int jv = ok ? j : -1;
    float W = 0.f;
    double ls = 0.0;
    for (int s = 0; s < m; ++s) {                          // slot order
      W += __shfl(wv, s, 64);
      ls += (double)__shfl(spv, s, 64);
    }
    const int64_t drow = a.u_goff + i - a.i_goff;          // inside [0, ni): checked by the entry
    const int64_t p0 = i * m1;
    if (lane < m) {
      a.wbuf[p0 + lane] = wv;
      a.keys_in[p0 + lane] = ok ? (uint32_t)j : (uint32_t)a.ni;
      a.vals_in[p0 + lane] = (int)(p0 + lane);
    }
    if (lane == 0) {
      a.wbuf[p0 + m] = -W;
      a.keys_in[p0 + m] = c > 0 ? (uint32_t)drow : (uint32_t)a.ni;
      a.vals_in[p0 + m] = (int)(p0 + m);
      row_loss[li] = c > 0 ? ls / (double)c : 0.0;
    }
    for (int k0 = 0; k0 < d; k0 += 64) {
      const int k = k0 + lane;
      const bool kin = k < d;
      float acc = 0.f;
      for (int s = 0; s < m; ++s) {
        const int jj = __shfl(jv, s, 64);
        const float ws = __shfl(wv, s, 64);
        if (jj >= 0 && kin) acc = fmaf(ws, a.items[(int64_t)jj * d + k], acc);
      }
      if (kin) a.dU[i * d + k] = fmaf(-W, a.items[drow * d + k], acc);
    }
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int r = 0; r < GOW; ++r) s += row_loss[r];
    a.loss_part[blockIdx.x] = s;
  }
}

// One wave per item: the run of its entries in the sorted list, ascending pair order.
__global__ __launch_bounds__(256) void hard_item_kernel(GradArgs a, int64_t n_ent) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t j = (int64_t)blockIdx.x * 4 + w;
  if (j >= a.ni) return;
  const int d = a.d, m1 = a.m + 1;
  int64_t lo = 0, hi = n_ent;                              // first entry with key >= j
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)a.keys_out[mid] < j) lo = mid + 1; else hi = mid;
  }
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int64_t e = lo; e < n_ent && (int64_t)a.keys_out[e] == j; ++e) {
    const int p = a.vals_out[e];
    const int64_t i = p / m1;
    const float wv = a.wbuf[p];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int k = lane + 64 * t;
      if (k < d) acc[t] = fmaf(wv, a.users[i * d + k], acc[t]);
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int k = lane + 64 * t;
    if (k < d) a.dI[j * d + k] = acc[t];
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

unsigned key_bits(int64_t n_items) {   // keys are 0 .. n_items (the sentinel): sort only the bits that can differ
  unsigned b = 1;
  while (b < 32 && (1ll << b) <= n_items) ++b;
  return b;
}

// workspace layout (bytes), all 256-B aligned:
//   keys_in u32[n] | keys_out u32[n] | vals_in i32[n] | vals_out i32[n] | w f32[n] | rocprim temp      n = n_users (m + 1)
struct HardWs {
  uint32_t* keys_in; uint32_t* keys_out; int* vals_in; int* vals_out; float* w; void* temp; size_t temp_bytes, total;
};

int hard_ws_layout(int64_t n_users, int64_t n_items, int m, void* base, HardWs* ws) {
  const size_t n = (size_t)n_users * (m + 1);
  size_t sort_bytes = 0;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                 (const int*)nullptr, (int*)nullptr, n, 0, key_bits(n_items));
  if (e != hipSuccess) return RIHIP_ERR_HIP;
  size_t off = 0;
  char* b = (char*)base;
  ws->keys_in = (uint32_t*)(b + off); off += align256(sizeof(uint32_t) * n);
  ws->keys_out = (uint32_t*)(b + off); off += align256(sizeof(uint32_t) * n);
  ws->vals_in = (int*)(b + off); off += align256(sizeof(int) * n);
  ws->vals_out = (int*)(b + off); off += align256(sizeof(int) * n);
  ws->w = (float*)(b + off); off += align256(sizeof(float) * n);
  ws->temp = (void*)(b + off);
  ws->temp_bytes = sort_bytes;
  off += align256(sort_bytes);
  ws->total = off;
  return RIHIP_OK;
}

int check_shape(const char* who, int d, int m, int skip, int64_t n_users, int64_t user_goff, int64_t n_items,
                int64_t item_goff) {
  RIHIP_REQUIRE(gen_width_ok(d), RIHIP_ERR_SHAPE, "%s: unsupported embed_dim=%d (multiples of 16 up to 256)", who, d);
  RIHIP_REQUIRE(m >= 1 && m <= HMAXN && skip >= 0 && skip + m <= HMAXM, RIHIP_ERR_ARG,
                "%s: m=%d skip=%d need 1 <= m <= %d, skip >= 0 and skip + m <= %d", who, m, skip, HMAXN, HMAXM);
  RIHIP_REQUIRE(n_users > 0 && n_items > 0 && n_items < (1ll << 31), RIHIP_ERR_ARG,
                "%s: sizes users=%lld items=%lld (items below 2^31)", who, (long long)n_users, (long long)n_items);
  RIHIP_REQUIRE(user_goff >= item_goff && user_goff + n_users <= item_goff + n_items, RIHIP_ERR_ARG,
                "%s: users [%lld, %lld) have partners outside the given items [%lld, %lld)", who, (long long)user_goff,
                (long long)(user_goff + n_users), (long long)item_goff, (long long)(item_goff + n_items));
  return RIHIP_OK;
}

}  // namespace

extern "C" int rihip_inbatch_hard_select(const float* users, int64_t n_users, int64_t user_goff, const float* items,
                                         int64_t n_items, int64_t item_goff, int d, int m, int skip,
                                         const int64_t* user_pos_ids, const int64_t* item_ids, int* neg_idx,
                                         float* neg_score, float* pos_score, void* stream) {
  const int rc = check_shape("inbatch_hard_select", d, m, skip, n_users, user_goff, n_items, item_goff);
  if (rc != RIHIP_OK) return rc;
  RIHIP_REQUIRE((user_pos_ids == nullptr) == (item_ids == nullptr), RIHIP_ERR_ARG,
                "inbatch_hard_select: user_pos_ids and item_ids must be given together or both be null");
  RIHIP_REQUIRE(users && items && neg_idx && neg_score && pos_score, RIHIP_ERR_ARG, "inbatch_hard_select: null pointer");
  static bool granted = false;
  if (!granted) {
    RIHIP_CHECK_HIP(grant_dynamic_lds(reinterpret_cast<const void*>(hard_select_kernel), select_lds(256, HMAXM)));
    granted = true;
  }
  SelectArgs a;
  a.Xo = users; a.No = n_users; a.o_goff = user_goff; a.Ys = items; a.Ns = n_items; a.s_goff = item_goff;
  a.D = d; a.m = m; a.skip = skip; a.o_ids = user_pos_ids; a.s_ids = item_ids;
  a.neg_idx = neg_idx; a.neg_score = neg_score; a.pos_score = pos_score;
  const dim3 grid((unsigned)((n_users + GOW - 1) / GOW));
  hipLaunchKernelGGL(hard_select_kernel, grid, dim3(256), select_lds(d, skip + m), (hipStream_t)stream, a);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int64_t rihip_inbatch_hard_loss_parts(int64_t n_users) { return (n_users + GOW - 1) / GOW; }

extern "C" int64_t rihip_inbatch_hard_workspace_bytes(int64_t n_users, int64_t n_items, int m) {
  HardWs ws;
  if (n_users <= 0 || n_items <= 0 || n_items >= (1ll << 31) || m < 1 || m > HMAXN ||
      n_users * (m + 1) >= (1ll << 31) || hard_ws_layout(n_users, n_items, m, nullptr, &ws) != RIHIP_OK)
    return -1;
  return (int64_t)ws.total;
}

extern "C" int rihip_inbatch_hard_grads(const float* users, int64_t n_users, int64_t user_goff, const float* items,
                                        int64_t n_items, int64_t item_goff, int d, int m, const int* neg_idx,
                                        const float* neg_score, const float* pos_score, int64_t n_global, float* d_users,
                                        float* d_items, double* loss_part, void* workspace, void* stream) {
  const int rc = check_shape("inbatch_hard_grads", d, m, 0, n_users, user_goff, n_items, item_goff);
  if (rc != RIHIP_OK) return rc;
  RIHIP_REQUIRE(n_global >= 1 && n_users * (m + 1) < (1ll << 31), RIHIP_ERR_ARG,
                "inbatch_hard_grads: B=%lld must be >= 1 and users * (m + 1) = %lld below 2^31", (long long)n_global,
                (long long)(n_users * (m + 1)));
  RIHIP_REQUIRE(users && items && neg_idx && neg_score && pos_score && d_users && d_items && loss_part && workspace,
                RIHIP_ERR_ARG, "inbatch_hard_grads: null pointer");
  HardWs ws;
  RIHIP_REQUIRE(hard_ws_layout(n_users, n_items, m, workspace, &ws) == RIHIP_OK, RIHIP_ERR_HIP,
                "inbatch_hard_grads: rocprim size query failed");
  GradArgs a;
  a.users = users; a.nu = n_users; a.u_goff = user_goff; a.items = items; a.ni = n_items; a.i_goff = item_goff;
  a.d = d; a.m = m; a.neg_idx = neg_idx; a.neg_score = neg_score; a.pos_score = pos_score; a.n_global = n_global;
  a.dU = d_users; a.dI = d_items; a.loss_part = loss_part;
  a.keys_in = ws.keys_in; a.keys_out = ws.keys_out; a.vals_in = ws.vals_in; a.vals_out = ws.vals_out; a.wbuf = ws.w;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(hard_user_kernel, dim3((unsigned)((n_users + GOW - 1) / GOW)), dim3(256), 0, st, a);
  RIHIP_CHECK_LAUNCH();
  const size_t n_ent = (size_t)n_users * (m + 1);
  size_t tb = ws.temp_bytes;
  RIHIP_CHECK_HIP(rocprim::radix_sort_pairs(ws.temp, tb, ws.keys_in, ws.keys_out, ws.vals_in, ws.vals_out, n_ent, 0,
                                            key_bits(n_items), st));
  hipLaunchKernelGGL(hard_item_kernel, dim3((unsigned)((n_items + 3) / 4)), dim3(256), 0, st, a, (int64_t)n_ent);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
