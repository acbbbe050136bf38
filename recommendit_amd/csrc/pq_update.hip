// Add / remove / replace items of a built PQ index under FROZEN codebooks: rihip_pq_update_* behind PQIndex.add_items /
// remove_items / update_items (opt-in: PQIndex.frozen_updates).
//
// One update is ONE repack of the entry-number matrix pq_codes [Np, M] on the device.  The handle's centroids, its SQ8
// quantiser, its list codes K_l and its codebooks are all frozen; a kept row keeps its M bytes, only the new rows are
// encoded.  The handle ends bit for bit where rihip_pq_index_from_ip_index_residual of the final corpus with the same
// centroids and lists, the handle's own quantiser and its own codebooks injected (injected codebooks skip the training,
// and a row's bytes are a function of the row, its list and that frozen state alone), rihip_sq8_filter_set_tags and
// rihip_sq8_refine_attach_vectors would leave it.
//   driver   : sq8_update_run (sq8_update.hip) -- masks, id checks, renumbering, the list of every new row, grouping, the
//              one host read in the middle of the call, offsets, row ids, tags, vectors and the swap are the SQ8 index's;
//              the SQ8-grid clamp count is the integer its sq8_update_clamp_kernel forms.  PqCodes below supplies the stages
//              that depend on the storage (Sq8UpdateStorage in sq8_index.h).
//   encode   : pq_update_encode_kernel<DSUB, RES> -- grid (blocks of 2048 new rows in grouped order, M sub-spaces).  The
//              sub-space's 256 entries and their squared norms lie in LDS and are read as a broadcast, as in pq.hip's
//              pq_assign_kernel.  A thread forms the SQ8 code of its row's DSUB columns (sq8_code; the columns beyond the
//              f32 row are 0), with RES subtracts K_l of the row's list and clamps to +-127, counting each clamp, then
//              takes the entry of the smallest D = |c|^2 + |b|^2 - 2 <c, b> in i32 (v_dot4_i32_i8), the lowest entry on a
//              tie.  The byte goes to a temporary [n_add, M] in grouped order; the row's smallest D and the clamps are
//              added to two u64 words (integer atomics after a wave reduction) that travel with the driver's host read.
//   repack   : pq_update_repack_kernel<V> -- source driven like sq8_update_repack_kernel with M-byte rows (V = 4, 8 or 16
//              bytes): one lane per row, one vector load and one vector store each.  A kept physical row goes to its
//              list's new offset + its rank among the list's kept rows, a new row's bytes follow behind them, every
//              list's padding is zero bytes with row id -1 and tag 0.  ~2*Np*(M + 8 + 4) bytes.
//   vectors  : compacted by the driver; the new state is decoded transiently (pq_decode_all, or pq_decode_all16 on a
//              residual handle) and e_j / a_j are recomputed by the matching sq8_launch_ranges overload.
// Peak device memory (computed from the allocations, not measured): old + new index arrays (Np*(M+8+4) + Np_new*(M+8+4)
// bytes, plus 2 * 4*dk bytes per row with vectors), + n_add*M bytes of new entry numbers, + the driver's scratch
// (~8*(N+Np) bytes), + with vectors the transient decode of the new state: Np_new*dpad bytes, 2*Np_new*dpad on a residual
// handle -- dsub (twice dsub) times the new pq_codes, and the largest term of a handle that holds vectors.
// A refused or failed call leaves the old index searchable and unchanged.
#pragma clang fp contract(off)   // the SQ8 quantiser is specified operation by operation: no fused multiply-add
#include "common.h"
#include "recommendit_hip.h"
#include "ip_index.h"
#include "sq8_index.h"

#include <limits.h>

using namespace rihip_index;

namespace {

typedef unsigned long long u64;

constexpr int PQU_RPT = 8;                // new rows per thread of the encode kernel
constexpr int PQU_RPB = 256 * PQU_RPT;    // new rows per workgroup: one LDS fill of the sub-space's entries serves 2048 rows
constexpr int W_RCLAMP = 0, W_DIST = 1;   // the storage's two counters behind the driver's host block

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int acc) {   // four signed bytes each, exact in i32
  return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false);
}

// enc[g][m] = the entry of sub-space m = blockIdx.y for new row g of the grouped order, g in [blockIdx.x * PQU_RPB, + PQU_RPB).
// X [n_add, dk] f32; K: the list codes [nlist, dpad] (RES only).  words[W_RCLAMP] += residual values clamped,
// words[W_DIST] += the rows' smallest D.
template <int DSUB, bool RES>
__global__ __launch_bounds__(256) void pq_update_encode_kernel(const float* __restrict__ X, int64_t n_add, int dk, int dpad,
                                                               const int* __restrict__ g_rows, const int* __restrict__ g_keys,
                                                               const float* __restrict__ centre, const float* __restrict__ scale,
                                                               const int8_t* __restrict__ K, const int8_t* __restrict__ book,
                                                               uint8_t* enc, u64* words) {
  constexpr int W = DSUB / 4;
  __shared__ uint32_t s_b[256 * W];
  __shared__ int s_n[256];
  const int tid = threadIdx.x, m = blockIdx.y, M = dpad / DSUB, col = m * DSUB;
  {
    const uint32_t* gb = reinterpret_cast<const uint32_t*>(book + ((size_t)m * 256 + tid) * DSUB);
    int nn = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint32_t v = gb[w];
      s_b[tid * W + w] = v;
      nn = dot4(v, v, nn);
    }
    s_n[tid] = nn;
  }
  __syncthreads();
  long long dist = 0;
  int n_cl = 0;
  const int64_t base = (int64_t)blockIdx.x * PQU_RPB;
  for (int it = 0; it < PQU_RPT; ++it) {
    const int64_t g = base + it * 256 + tid;
    if (g >= n_add) continue;
    uint32_t c[W];
#pragma unroll
    for (int w = 0; w < W; ++w) c[w] = 0u;
    if (col < dk) {   // dk is a multiple of 32: the sub-space lies inside the f32 row or all beyond it (code 0)
      const f32x4* x = reinterpret_cast<const f32x4*>(X + (size_t)g_rows[g] * dk + col);
      const f32x4* mm = reinterpret_cast<const f32x4*>(centre + col);
      const f32x4* ss = reinterpret_cast<const f32x4*>(scale + col);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const f32x4 xv = x[w], mv = mm[w], sv = ss[w];
#pragma unroll
        for (int u = 0; u < 4; ++u) c[w] |= ((uint32_t)sq8_code(xv[u], mv[u], sv[u]) & 0xFFu) << (8 * u);
      }
    }
    if constexpr (RES) {
      const uint32_t* kw = reinterpret_cast<const uint32_t*>(K + (size_t)g_keys[g] * dpad + col);
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const uint32_t cw = c[w], k = kw[w];
        uint32_t packed = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          int r = (int)(int8_t)(cw >> (8 * u)) - (int)(int8_t)(k >> (8 * u));
          if (r > 127) { r = 127; ++n_cl; }
          if (r < -127) { r = -127; ++n_cl; }
          packed |= ((uint32_t)r & 0xFFu) << (8 * u);
        }
        c[w] = packed;
      }
    }
    int cn = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) cn = dot4(c[w], c[w], cn);
    int best = 0, bd = INT_MAX;
#pragma unroll 4
    for (int e = 0; e < 256; ++e) {
      int dp = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) dp = dot4(c[w], s_b[e * W + w], dp);
      const int d = s_n[e] - 2 * dp;
      if (d < bd) { bd = d; best = e; }   // strictly smaller: the lowest e keeps a tie
    }
    dist += cn + bd;
    enc[(size_t)g * M + m] = (uint8_t)best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    dist += __shfl_xor(dist, o, 64);
    if constexpr (RES) n_cl += __shfl_xor(n_cl, o, 64);
  }
  if ((tid & 63) == 0) {
    if (dist != 0) atomicAdd(words + W_DIST, (u64)dist);
    if (RES && n_cl != 0) atomicAdd(words + W_RCLAMP, (u64)n_cl);
  }
}

struct PqRepackArgs {
  const uint8_t* codes_old; const int64_t* row_ids_old; const uint32_t* tags_old; const int* tile_list_old;
  const int64_t* poff_old; int64_t Np_old;
  const int* keep; const int* rscan; const int* pscan;
  const uint8_t* enc; const uint32_t* add_tags; const int* g_rows; const int* g_keys; const int* g_off; int64_t n_add;
  const unsigned long long* cnt_keep; const int64_t* poff_new;
  uint8_t* codes_new; int64_t* row_ids_new; uint32_t* tags_new;   // tags_new: null on an untagged handle
  int64_t n_keep; int nlist;
};

// work item = one source row of sizeof(V) = M bytes, one lane each: the Np_old physical rows, then the n_add new rows in
// grouped order (their bytes are enc's), then 64 candidate padding rows per list.  Every destination row in [0, Np_new)
// is written exactly once.
template <typename V>
__global__ __launch_bounds__(256) void pq_update_repack_kernel(const PqRepackArgs a) {
  int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  V v{};
  int64_t dest, rid;
  uint32_t tag = 0u;
  if (it < a.Np_old) {
    const int64_t old = a.row_ids_old[it];
    if (old < 0 || !a.keep[old]) return;
    const int c = a.tile_list_old[it / TR];
    dest = a.poff_new[c] + (a.pscan[it] - a.pscan[a.poff_old[c]]);
    rid = a.rscan[old];
    v = reinterpret_cast<const V*>(a.codes_old)[it];
    if (a.tags_new) tag = a.tags_old[it];
  } else if ((it -= a.Np_old) < a.n_add) {
    const int j = a.g_rows[it], c = a.g_keys[it];
    dest = a.poff_new[c] + (int64_t)a.cnt_keep[c] + (it - a.g_off[c]);
    rid = a.n_keep + j;
    v = reinterpret_cast<const V*>(a.enc)[it];
    if (a.add_tags) tag = a.add_tags[j];
  } else {
    it -= a.n_add;
    const int c = (int)(it / TR);
    if (c >= a.nlist) return;
    dest = a.poff_new[c] + (int64_t)a.cnt_keep[c] + (a.g_off[c + 1] - a.g_off[c]) + it % TR;
    if (dest >= a.poff_new[c + 1]) return;
    rid = -1;
  }
  reinterpret_cast<V*>(a.codes_new)[dest] = v;
  a.row_ids_new[dest] = rid;
  if (a.tags_new) a.tags_new[dest] = tag;
}

// the entry-number matrix: new rows are encoded before the host read (their counters travel with it), the repack moves
// bytes only, the ranges read a transient decode of the new state
struct PqCodes : Sq8UpdateStorage {
  uint8_t* enc = nullptr;        // [n_add, M] grouped order
  uint8_t* codes = nullptr;      // [Np_new, M]
  int8_t* dec = nullptr;         // the transient decodes of `ranges`
  int16_t* dec16 = nullptr;
  PqCodes() { who = "pq_update_apply"; n_words = 2; }
  ~PqCodes() override { hipFree(enc); hipFree(codes); hipFree(dec); hipFree(dec16); }

  int encode(const Sq8UpdateCtx& c) override {
    const Sq8Index* h = c.h;
    const int dsub = h->pq_dsub, M = h->dpad / dsub;
    HIPCHK(hipMalloc((void**)&enc, (size_t)c.n_add * M));
    const dim3 grid((unsigned)((c.n_add + PQU_RPB - 1) / PQU_RPB), (unsigned)M);
#define PQU_ENCODE(DSUB, RES)                                                                                                   \
  hipLaunchKernelGGL((pq_update_encode_kernel<DSUB, RES>), grid, dim3(256), 0, c.st, c.X_add, c.n_add, h->dk, h->dpad, c.g_rows, \
                     c.g_keys, h->centre, h->scale, h->pq_list_codes, h->pq_book, enc, c.words)
    if (h->pq_residual) { if (dsub == 8) PQU_ENCODE(8, true); else PQU_ENCODE(16, true); }
    else { if (dsub == 8) PQU_ENCODE(8, false); else PQU_ENCODE(16, false); }
#undef PQU_ENCODE
    return check_launch("pq update encode");
  }

  int repack(const Sq8UpdateCtx& c) override {
    const Sq8Index* h = c.h;
    const int M = h->dpad / h->pq_dsub;   // 4, 8 or 16
    HIPCHK(hipMalloc((void**)&codes, (size_t)c.Np_new * M));
    PqRepackArgs a;
    a.codes_old = h->pq_codes; a.row_ids_old = h->row_ids; a.tags_old = h->tags; a.tile_list_old = c.tile_list_old; a.poff_old = h->list_poff;
    a.Np_old = h->Np; a.keep = c.keep; a.rscan = c.rscan; a.pscan = c.pscan;
    a.enc = enc; a.add_tags = c.add_tags; a.g_rows = c.g_rows; a.g_keys = c.g_keys; a.g_off = c.g_off; a.n_add = c.n_add;
    a.cnt_keep = c.cnt_keep; a.poff_new = c.poff_new;
    a.codes_new = codes; a.row_ids_new = c.row_ids_new; a.tags_new = c.tags_new; a.n_keep = c.n_keep; a.nlist = h->nlist;
    const int64_t tot = h->Np + c.n_add + (int64_t)h->nlist * TR;
    const dim3 grid((unsigned)((tot + 255) / 256));
    if (M == 4) hipLaunchKernelGGL(pq_update_repack_kernel<uint32_t>, grid, dim3(256), 0, c.st, a);
    else if (M == 8) hipLaunchKernelGGL(pq_update_repack_kernel<uint2>, grid, dim3(256), 0, c.st, a);
    else hipLaunchKernelGGL(pq_update_repack_kernel<uint4>, grid, dim3(256), 0, c.st, a);
    return check_launch("pq update repack");
  }

  int ranges(const Sq8UpdateCtx& c) override {
    const Sq8Index* h = c.h;
    Sq8Index v;   // the new state as far as the decode reads it; owns nothing
    v.dpad = h->dpad; v.Np = c.Np_new; v.nlist = h->nlist; v.pq_dsub = h->pq_dsub; v.pq_residual = h->pq_residual;
    v.pq_codes = codes; v.pq_book = h->pq_book; v.pq_list_codes = h->pq_list_codes;
    v.row_ids = c.row_ids_new; v.list_poff = const_cast<int64_t*>(c.poff_new);
    if (h->pq_residual) {
      RCCHK(pq_decode_all16(&v, &dec16, c.st));
      sq8_launch_ranges(true, c.vec_new, dec16, c.row_ids_new, c.Np_new, h->dk, h->dpad, h->centre, h->scale, c.part, c.nb, c.e_new, c.a_new, c.st);
    } else {
      RCCHK(pq_decode_all(&v, &dec, c.st));
      sq8_launch_ranges(true, c.vec_new, dec, c.row_ids_new, c.Np_new, h->dk, h->dpad, h->centre, h->scale, c.part, c.nb, c.e_new, c.a_new, c.st);
    }
    return check_launch("pq update ranges");
  }

  void swap(Sq8Index* h, const unsigned long long* w) override {
    hipFree(h->pq_codes);
    h->pq_codes = codes;
    codes = nullptr;
    h->pq_upd_stats[0] += (int64_t)w[W_RCLAMP]; h->pq_upd_stats[1] += (int64_t)w[W_DIST];
    h->pq_upd_stats[2] = (int64_t)w[W_RCLAMP]; h->pq_upd_stats[3] = (int64_t)w[W_DIST];
  }
};

}  // namespace

extern "C" int rihip_pq_update_apply(void* handle, const int64_t* item_ids, const int64_t* drop_ids, int64_t n_drop,
                                     const float* X_add, const int64_t* add_ids, const uint32_t* add_tags, int64_t n_add,
                                     int64_t* item_ids_out, int64_t* n_total, int64_t* n_dropped, int64_t* n_clamped,
                                     int64_t* bad_id, int* bad_kind, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && h->pq_codes && h->pq_book, RIHIP_ERR_STATE,
                "rihip_pq_update_apply: not a PQ index (an SQ8 index is updated by rihip_sq8_update_apply)");
  RIHIP_REQUIRE(h->N > 0, RIHIP_ERR_STATE, "pq_update_apply: index is empty");
  PqCodes stg;
  return sq8_update_run(h, stg, item_ids, drop_ids, n_drop, X_add, add_ids, add_tags, n_add, item_ids_out, n_total, n_dropped, n_clamped,
                        bad_id, bad_kind, (hipStream_t)stream);
}

extern "C" int rihip_pq_update_stats(void* handle, int64_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "pq_update_stats: bad arguments");
  RIHIP_REQUIRE(h->pq_codes, RIHIP_ERR_STATE, "pq_update_stats: not a PQ index");
  for (int i = 0; i < 4; ++i) { out[i] = h->upd_stats[i]; out[4 + i] = h->pq_upd_stats[i]; }
  return RIHIP_OK;
}
