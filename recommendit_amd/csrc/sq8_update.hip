// Add / remove / replace items of a built 8-bit index without its f32 source and without re-encoding the rows that stay:
// rihip_sq8_update_* behind SQ8Index.add_items / remove_items / update_items.
//
// One update is ONE repack of the code matrix on the device under the handle's own centroids and its own quantiser; it
// leaves the handle bit for bit in the state rihip_sq8_index_from_ip_index of the final corpus with that quantiser (same
// centroids, kept rows in their lists, new rows in their arg-max list), rihip_sq8_filter_set_tags of the final tag words
// and rihip_sq8_refine_attach_vectors would leave it in.  The quantiser is per row and per dimension, so a kept row's
// code is the code it has; only the new rows are encoded.
//   mask, renumber, lists : index_update_kernels.h, as the f32 index's update (index_update.hip); the handle holds no
//              granule table, so sq8_update_tile_list_kernel derives one from list_poff.  sq8_update_clamp_kernel counts,
//              as an integer, the code values of the new rows that the frozen quantiser clamps.  One device->host read of
//              <= 2*2048+6 integers gives the checks, the clamp count and the new list lengths.
//   repack   : sq8_update_repack_kernel -- source driven: a kept physical row goes to its list's new offset + its rank
//              among the list's kept rows, a new row is encoded from its f32 row behind them (sq8_code), the padding of
//              every list is written as zero rows with row id -1 and tag 0.  16-byte accesses, dpad/16 lanes per row; the
//              row id and the tag word travel with lane 0.  ~2*Np*(dpad + 8 + 4) bytes.
//   vectors  : the attached f32 rows are compacted in insertion order (index_update_compact_kernel), then e_j and a_j
//              are recomputed in f64 over the final rows against the final stored codes (a removed row can shrink a
//              maximum), by the range pass that attached them (sq8_launch_ranges in sq8_refine.hip, reading the f32 row
//              of a physical row through its row id), without atomics.
// Flat handles (nlist == 1) take the same kernels.  The new arrays are built next to the old ones and swapped in at the
// end (peak device memory = old + new); a call that is refused or fails leaves the old index searchable.
//
// Only the repack, the ranges' code matrix and the counters depend on how the handle stores its codes.  Everything else
// is sq8_update_run below, which a PQ handle's update (pq_update.hip) runs as well with stages of its own
// (Sq8UpdateStorage in sq8_index.h); Sq8Codes here is the int8 matrix's.
#pragma clang fp contract(off)   // the quantiser is specified operation by operation: no fused multiply-add
#include "common.h"
#include "recommendit_hip.h"
#include "ip_index.h"
#include "sq8_index.h"
#include "index_update_kernels.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include <rocprim/rocprim.hpp>

using namespace rihip_index;

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// tile_list[g] = list of physical granule g: the last list that starts at or before row g * TR (an empty list shares
// its offset with the next one, which is the one that owns the granule)
__global__ void sq8_update_tile_list_kernel(const int64_t* __restrict__ poff, int nlist, int64_t n_gran, int* tile_list) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_gran) return;
  const int64_t p = g * TR;
  int lo = 0, hi = nlist;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (poff[mid] <= p) lo = mid; else hi = mid;
  }
  tile_list[g] = lo;
}

// *slot += the pairs (new row i, column j < du) whose unclamped rintf((x_ij - m_j) / s_j) lies outside +-127; X [n, dk]
__global__ __launch_bounds__(256) void sq8_update_clamp_kernel(const float* __restrict__ X, int64_t n, int du, int dk,
                                                               const float* __restrict__ centre, const float* __restrict__ scale,
                                                               unsigned long long* slot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool out = false;
  if (i < n * dk) {
    const int j = (int)(i % dk);
    if (j < du) {
      const float v = rintf((X[i] - centre[j]) / scale[j]);
      out = v > 127.f || v < -127.f;
    }
  }
  const unsigned long long b = __ballot(out);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(slot, (unsigned long long)__popcll(b));
}

struct Sq8RepackArgs {
  const int8_t* codes_old; const int64_t* row_ids_old; const uint32_t* tags_old; const int* tile_list_old;
  const int64_t* poff_old; int64_t Np_old;
  const int* keep; const int* rscan; const int* pscan;
  const float* X_add; const uint32_t* add_tags; const int* g_rows; const int* g_keys; const int* g_off; int64_t n_add;
  const float* centre; const float* scale;
  const unsigned long long* cnt_keep; const int64_t* poff_new;
  int8_t* codes_new; int64_t* row_ids_new; uint32_t* tags_new;   // tags_new: null on an untagged handle
  int64_t n_keep; int nlist; int dk; int lanes;                  // lanes = dpad / 16
};

// work item = one source row (dpad/16 lanes, 16 bytes each): the Np_old physical rows, then the n_add new rows in grouped
// order, then 64 candidate padding rows per list.  Every destination row in [0, Np_new) is written exactly once.
__global__ __launch_bounds__(256) void sq8_update_repack_kernel(const Sq8RepackArgs a) {
  const int L = a.lanes;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t it = idx / L;
  const int l = (int)(idx % L);
  i32x4 v = {0, 0, 0, 0};
  int64_t dest, rid;
  uint32_t tag = 0u;
  if (it < a.Np_old) {
    const int64_t old = a.row_ids_old[it];
    if (old < 0 || !a.keep[old]) return;
    const int c = a.tile_list_old[it / TR];
    dest = a.poff_new[c] + (a.pscan[it] - a.pscan[a.poff_old[c]]);
    rid = a.rscan[old];
    v = reinterpret_cast<const i32x4*>(a.codes_old + (size_t)it * L * 16)[l];
    if (l == 0 && a.tags_new) tag = a.tags_old[it];
  } else if ((it -= a.Np_old) < a.n_add) {
    const int j = a.g_rows[it], c = a.g_keys[it];
    dest = a.poff_new[c] + (int64_t)a.cnt_keep[c] + (it - a.g_off[c]);
    rid = a.n_keep + j;
    const int col = 16 * l;
    if (col < a.dk) {   // dk is a multiple of 32: the lane's 16 columns lie inside the f32 row or all beyond it (code 0)
      const f32x4* x = reinterpret_cast<const f32x4*>(a.X_add + (size_t)j * a.dk + col);
      const f32x4* m = reinterpret_cast<const f32x4*>(a.centre + col);
      const f32x4* s = reinterpret_cast<const f32x4*>(a.scale + col);
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const f32x4 xv = x[w], mv = m[w], sv = s[w];
        uint32_t packed = 0;
#pragma unroll
        for (int u = 0; u < 4; ++u) packed |= ((uint32_t)sq8_code(xv[u], mv[u], sv[u]) & 0xFFu) << (8 * u);
        v[w] = (int)packed;
      }
    }
    if (l == 0 && a.add_tags) tag = a.add_tags[j];
  } else {
    it -= a.n_add;
    const int c = (int)(it / TR);
    if (c >= a.nlist) return;
    dest = a.poff_new[c] + (int64_t)a.cnt_keep[c] + (a.g_off[c + 1] - a.g_off[c]) + it % TR;
    if (dest >= a.poff_new[c + 1]) return;
    rid = -1;
  }
  reinterpret_cast<i32x4*>(a.codes_new + (size_t)dest * L * 16)[l] = v;
  if (l == 0) {
    a.row_ids_new[dest] = rid;
    if (a.tags_new) a.tags_new[dest] = tag;
  }
}

struct Owned {   // everything the driver must free on every way out
  UpdateScratch s; Grouper g;
  int64_t* rid = nullptr; uint32_t* tags = nullptr; int64_t* poff = nullptr; int* len = nullptr;
  float* vec = nullptr; double* e = nullptr; double* a = nullptr; double* part = nullptr;
  ~Owned() {
    hipFree(s.base); g.release();
    hipFree(rid); hipFree(tags); hipFree(poff); hipFree(len); hipFree(vec); hipFree(e); hipFree(a); hipFree(part);
  }
};

// the int8 code matrix: new rows are encoded inside the repack, the ranges read the new matrix as it is
struct Sq8Codes : Sq8UpdateStorage {
  int8_t* codes = nullptr;
  Sq8Codes() { who = "sq8_update_apply"; }
  ~Sq8Codes() override { hipFree(codes); }
  int repack(const Sq8UpdateCtx& c) override {
    const Sq8Index* h = c.h;
    const int L = h->dpad / 16;
    HIPCHK(hipMalloc((void**)&codes, (size_t)c.Np_new * h->dpad));
    Sq8RepackArgs a;
    a.codes_old = h->codes; a.row_ids_old = h->row_ids; a.tags_old = h->tags; a.tile_list_old = c.tile_list_old; a.poff_old = h->list_poff;
    a.Np_old = h->Np; a.keep = c.keep; a.rscan = c.rscan; a.pscan = c.pscan;
    a.X_add = c.X_add; a.add_tags = c.add_tags; a.g_rows = c.g_rows; a.g_keys = c.g_keys; a.g_off = c.g_off; a.n_add = c.n_add;
    a.centre = h->centre; a.scale = h->scale; a.cnt_keep = c.cnt_keep; a.poff_new = c.poff_new;
    a.codes_new = codes; a.row_ids_new = c.row_ids_new; a.tags_new = c.tags_new; a.n_keep = c.n_keep; a.nlist = h->nlist; a.dk = h->dk; a.lanes = L;
    const int64_t tot = (h->Np + c.n_add + (int64_t)h->nlist * TR) * L;
    hipLaunchKernelGGL(sq8_update_repack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c.st, a);
    RIHIP_CHECK_LAUNCH();
    return RIHIP_OK;
  }
  int ranges(const Sq8UpdateCtx& c) override {
    sq8_launch_ranges(true, c.vec_new, codes, c.row_ids_new, c.Np_new, c.h->dk, c.h->dpad, c.h->centre, c.h->scale, c.part, c.nb, c.e_new,
                      c.a_new, c.st);
    RIHIP_CHECK_LAUNCH();
    return RIHIP_OK;
  }
  void swap(Sq8Index* h, const unsigned long long*) override {
    hipFree(h->codes);
    h->codes = codes;
    codes = nullptr;
  }
};

}  // namespace

namespace rihip_index {
// h: a handle with storage and N > 0 (the caller's check, with its own text)
int sq8_update_run(Sq8Index* h, Sq8UpdateStorage& stg, const int64_t* item_ids, const int64_t* drop_ids, int64_t n_drop,
                   const float* X_add, const int64_t* add_ids, const uint32_t* add_tags, int64_t n_add, int64_t* item_ids_out,
                   int64_t* n_total, int64_t* n_dropped, int64_t* n_clamped, int64_t* bad_id, int* bad_kind, hipStream_t st) {
  RIHIP_REQUIRE(item_ids && item_ids_out && n_total && n_dropped && n_clamped && bad_id && bad_kind && n_drop >= 0 && n_add >= 0 &&
                (n_drop == 0 || drop_ids) && (n_add == 0 || (X_add && add_ids)), RIHIP_ERR_ARG, "%s: bad arguments", stg.who);
  *bad_kind = 0; *bad_id = 0; *n_total = h->N; *n_dropped = 0; *n_clamped = 0;
  if (n_drop == 0 && n_add == 0) return RIHIP_OK;
  const int64_t N = h->N, Np = h->Np;
  const int dk = h->dk, nlist = h->nlist;
  RIHIP_REQUIRE(N + n_add + (int64_t)TR * (nlist + 1) < (1ll << 31) && n_drop < (1ll << 31), RIHIP_ERR_ARG,
                "%s: %lld + %lld rows exceed the 2^31 row limit", stg.who, (long long)N, (long long)n_add);
  // zero-padded to dk, as the source index held them
  if (n_add > 0) {
    char misaligned[96];
    snprintf(misaligned, sizeof(misaligned), "%s: the rows must be 16-byte aligned", stg.who);
    RCCHK(sq8_rows_at_dk(h, X_add, n_add, misaligned, st));
  }

  Owned o;
  UpdateScratch& s = o.s;
  const int64_t n_lists_hb = HB_LISTS + 2 * (int64_t)nlist + 1;   // the block of index_update_kernels.h ...
  const int64_t nhb = n_lists_hb + stg.n_words;                    // ... and behind it the storage's own counters
  const size_t o_hb = s.plan<unsigned long long>(nhb), o_sdrop = s.plan<int64_t>(n_drop), o_sadd = s.plan<int64_t>(n_add);
  const size_t o_keep = s.plan<int>(N + 1), o_rscan = s.plan<int>(N + 1), o_pkeep = s.plan<int>(Np + 1), o_pscan = s.plan<int>(Np + 1);
  const size_t o_anew = s.plan<int>(n_add), o_zoff = s.plan<int>(nlist + 1), o_tl = s.plan<int>(Np / TR);
  size_t t_sort_d = 0, t_sort_a = 0, t_scan_r = 0, t_scan_p = 0;
  if (n_drop) HIPCHK(rocprim::radix_sort_keys(nullptr, t_sort_d, (const int64_t*)nullptr, (int64_t*)nullptr, (size_t)n_drop, 0, 64, st));
  if (n_add) HIPCHK(rocprim::radix_sort_keys(nullptr, t_sort_a, (const int64_t*)nullptr, (int64_t*)nullptr, (size_t)n_add, 0, 64, st));
  HIPCHK(rocprim::exclusive_scan(nullptr, t_scan_r, (const int*)nullptr, (int*)nullptr, 0, (size_t)(N + 1), rocprim::plus<int>(), st));
  HIPCHK(rocprim::exclusive_scan(nullptr, t_scan_p, (const int*)nullptr, (int*)nullptr, 0, (size_t)(Np + 1), rocprim::plus<int>(), st));
  const size_t t_bytes = std::max(std::max(t_sort_d, t_sort_a), std::max(t_scan_r, t_scan_p));
  const size_t o_temp = s.plan<char>((int64_t)t_bytes);
  if (hipMalloc((void**)&s.base, s.used) != hipSuccess) {
    rihip_set_error("%s: device allocation of %lld bytes failed", stg.who, (long long)s.used);
    return RIHIP_ERR_HIP;
  }
  unsigned long long* hb = s.at<unsigned long long>(o_hb);
  if (stg.n_words) HIPCHK(hipMemsetAsync(hb + n_lists_hb, 0, sizeof(unsigned long long) * stg.n_words, st));
  int64_t* sdrop = s.at<int64_t>(o_sdrop);
  int64_t* sadd = s.at<int64_t>(o_sadd);
  int* keep = s.at<int>(o_keep);
  int* rscan = s.at<int>(o_rscan);
  int* pkeep = s.at<int>(o_pkeep);
  int* pscan = s.at<int>(o_pscan);
  int* a_new = s.at<int>(o_anew);
  int* zoff = s.at<int>(o_zoff);
  int* tl_old = s.at<int>(o_tl);
  void* temp = s.at<char>(o_temp);

  // 1. masks, counts, id checks
  hipLaunchKernelGGL(index_update_init_kernel, dim3(1), dim3(64), 0, st, hb);
  if (n_drop) {
    size_t tb = t_bytes;
    HIPCHK(rocprim::radix_sort_keys(temp, tb, drop_ids, sdrop, (size_t)n_drop, 0, 64, st));
    hipLaunchKernelGGL(index_update_repeat_kernel, dim3((unsigned)((n_drop + 255) / 256)), dim3(256), 0, st, sdrop, n_drop, hb + HB_REP_DROP);
  }
  if (n_add) {
    size_t tb = t_bytes;
    HIPCHK(rocprim::radix_sort_keys(temp, tb, add_ids, sadd, (size_t)n_add, 0, 64, st));
    hipLaunchKernelGGL(index_update_repeat_kernel, dim3((unsigned)((n_add + 255) / 256)), dim3(256), 0, st, sadd, n_add, hb + HB_REP_ADD);
  }
  hipLaunchKernelGGL(index_update_mask_kernel, dim3((unsigned)((N + 1 + 255) / 256)), dim3(256), 0, st, item_ids, N, sdrop, n_drop,
                     sadd, n_add, keep, hb);
  RIHIP_CHECK_LAUNCH();
  { size_t tb = t_bytes; HIPCHK(rocprim::exclusive_scan(temp, tb, (const int*)keep, rscan, 0, (size_t)(N + 1), rocprim::plus<int>(), st)); }

  // 2. kept rows per list, list of every new row, clamp count, the storage's own work on the new rows
  const int* g_rows = nullptr; const int* g_keys = nullptr; const int* g_off = zoff;
  hipLaunchKernelGGL(index_update_pmask_kernel, dim3((unsigned)((Np + 1 + 255) / 256)), dim3(256), 0, st, h->row_ids, Np, keep, pkeep);
  hipLaunchKernelGGL(sq8_update_tile_list_kernel, dim3((unsigned)((Np / TR + 255) / 256)), dim3(256), 0, st, h->list_poff, nlist,
                     Np / TR, tl_old);
  RIHIP_CHECK_LAUNCH();
  { size_t tb = t_bytes; HIPCHK(rocprim::exclusive_scan(temp, tb, (const int*)pkeep, pscan, 0, (size_t)(Np + 1), rocprim::plus<int>(), st)); }
  HIPCHK(hipMemsetAsync(zoff, 0, sizeof(int) * (nlist + 1), st));
  if (n_add) {
    if (nlist == 1) HIPCHK(hipMemsetAsync(a_new, 0, sizeof(int) * n_add, st));   // a flat-built handle: its one list
    else RCCHK(launch_assign(dk, X_add, n_add, h->C, nlist, a_new, st));
    RCCHK(o.g.init(n_add, nlist, st));
    RCCHK(o.g.group(a_new, st));
    g_rows = o.g.rows; g_keys = o.g.keys; g_off = o.g.off;
    hipLaunchKernelGGL(sq8_update_clamp_kernel, dim3((unsigned)((n_add * dk + 255) / 256)), dim3(256), 0, st, X_add, n_add, h->du, dk,
                       h->centre, h->scale, hb + HB_SPARE);
  }
  const bool tagged = h->tags != nullptr, with_vec = h->vec != nullptr;
  Sq8UpdateCtx cx{};
  cx.h = h; cx.st = st; cx.X_add = X_add; cx.add_tags = tagged ? add_tags : nullptr; cx.n_add = n_add;
  cx.keep = keep; cx.rscan = rscan; cx.pscan = pscan; cx.tile_list_old = tl_old;
  cx.g_rows = g_rows; cx.g_keys = g_keys; cx.g_off = g_off; cx.words = hb + n_lists_hb;
  if (n_add) RCCHK(stg.encode(cx));
  hipLaunchKernelGGL(index_update_list_count_kernel, dim3((unsigned)((nlist + 1 + 255) / 256)), dim3(256), 0, st, pscan,
                     h->list_poff, g_off, nlist, hb);
  RIHIP_CHECK_LAUNCH();

  // 3. the one synchronisation in the middle: counts and checks
  std::vector<unsigned long long> hbh(nhb);
  HIPCHK(hipMemcpyAsync(hbh.data(), hb, sizeof(unsigned long long) * nhb, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (hbh[HB_REP_DROP] != NO_ID || hbh[HB_REP_ADD] != NO_ID) {
    *bad_kind = 1; *bad_id = id_of(hbh[hbh[HB_REP_ADD] != NO_ID ? HB_REP_ADD : HB_REP_DROP]);
    rihip_set_error("item id %lld is repeated inside one update", (long long)*bad_id);
    return RIHIP_ERR_ARG;
  }
  if (hbh[HB_STORED] != NO_ID) {
    *bad_kind = 2; *bad_id = id_of(hbh[HB_STORED]);
    rihip_set_error("item id %lld is already stored (update_items replaces a stored item)", (long long)*bad_id);
    return RIHIP_ERR_ARG;
  }
  const int64_t n_gone = (int64_t)hbh[HB_NDROP], n_keep = N - n_gone, n_new = n_keep + n_add;
  if (n_new <= 0) {
    *bad_kind = 3;
    rihip_set_error("the update would leave the index empty");
    return RIHIP_ERR_ARG;
  }
  if (n_gone == 0 && n_add == 0) return RIHIP_OK;   // only unknown ids: nothing changes

  // 4. new list lengths and offsets
  std::vector<int64_t> len_n(nlist), poff(nlist + 1, 0);
  std::vector<int> len32(nlist);
  for (int c = 0; c < nlist; ++c) {
    len_n[c] = (int64_t)hbh[HB_LISTS + c] + (int64_t)(hbh[HB_LISTS + nlist + c + 1] - hbh[HB_LISTS + nlist + c]);
    len32[c] = (int)len_n[c];
    poff[c + 1] = poff[c] + (len_n[c] + TR - 1) / TR * TR;
  }
  const int64_t Np_n = poff[nlist];   // > 0: n_new > 0
  const int nb = (int)std::min<int64_t>(4096, (Np_n + 255) / 256);   // blocks of the range pass (a maximum: any split gives the same bits)
  HIPCHK(hipMalloc((void**)&o.rid, sizeof(int64_t) * (size_t)Np_n));
  HIPCHK(hipMalloc((void**)&o.poff, sizeof(int64_t) * (nlist + 1)));
  HIPCHK(hipMalloc((void**)&o.len, sizeof(int) * nlist));
  if (tagged) HIPCHK(hipMalloc((void**)&o.tags, sizeof(uint32_t) * (size_t)Np_n));
  if (with_vec) {
    HIPCHK(hipMalloc((void**)&o.vec, sizeof(float) * (size_t)n_new * dk));
    HIPCHK(hipMalloc((void**)&o.e, sizeof(double) * dk));
    HIPCHK(hipMalloc((void**)&o.a, sizeof(double) * dk));
    HIPCHK(hipMalloc((void**)&o.part, sizeof(double) * (size_t)nb * 2 * dk));
  }
  HIPCHK(hipMemcpyAsync(o.poff, poff.data(), sizeof(int64_t) * (nlist + 1), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(o.len, len32.data(), sizeof(int) * nlist, hipMemcpyHostToDevice, st));

  // 5. result ids, the storage's repack, vectors and their ranges
  hipLaunchKernelGGL(index_update_ids_kernel, dim3((unsigned)((N + n_add + 255) / 256)), dim3(256), 0, st, item_ids, N, keep, rscan,
                     add_ids, n_add, n_keep, item_ids_out);
  RIHIP_CHECK_LAUNCH();
  cx.cnt_keep = hb + HB_LISTS; cx.poff_new = o.poff; cx.n_keep = n_keep; cx.Np_new = Np_n; cx.row_ids_new = o.rid; cx.tags_new = o.tags;
  RCCHK(stg.repack(cx));
  if (with_vec) {
    const int d4 = dk / 4;
    const int64_t tv = (N + n_add) * d4;
    hipLaunchKernelGGL(index_update_compact_kernel, dim3((unsigned)((tv + 255) / 256)), dim3(256), 0, st, h->vec, N, keep, rscan, X_add,
                       n_add, n_keep, d4, o.vec);
    RIHIP_CHECK_LAUNCH();
    cx.vec_new = o.vec; cx.part = o.part; cx.nb = nb; cx.e_new = o.e; cx.a_new = o.a;
    RCCHK(stg.ranges(cx));
  }
  HIPCHK(hipStreamSynchronize(st));   // (the host vectors go away; the caller's rows may go away after the call)

  // 6. swap
  rihip_bump_generation();
  hipFree(h->row_ids); hipFree(h->list_poff); hipFree(h->list_len_dev); hipFree(h->tags);
  hipFree(h->vec); hipFree(h->ref_e); hipFree(h->ref_a);
  hipFree(h->inv_pos); h->inv_pos = nullptr;   // (a new physical order)
  h->row_ids = o.rid; h->list_poff = o.poff; h->list_len_dev = o.len; h->tags = o.tags;
  h->vec = o.vec; h->ref_e = o.e; h->ref_a = o.a;
  o.rid = nullptr; o.poff = nullptr; o.len = nullptr; o.tags = nullptr; o.vec = nullptr; o.e = nullptr; o.a = nullptr;
  h->N = n_new; h->Np = Np_n; h->list_len = len_n; h->id_map = nullptr;
  *n_total = n_new; *n_dropped = n_gone; *n_clamped = (int64_t)hbh[HB_SPARE];
  h->upd_stats[0] += 1; h->upd_stats[1] += n_gone; h->upd_stats[2] += n_add; h->upd_stats[3] += *n_clamped;
  stg.swap(h, hbh.data() + n_lists_hb);
  return RIHIP_OK;
}
}  // namespace rihip_index

extern "C" int rihip_sq8_update_apply(void* handle, const int64_t* item_ids, const int64_t* drop_ids, int64_t n_drop,
                                      const float* X_add, const int64_t* add_ids, const uint32_t* add_tags, int64_t n_add,
                                      int64_t* item_ids_out, int64_t* n_total, int64_t* n_dropped, int64_t* n_clamped,
                                      int64_t* bad_id, int* bad_kind, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(!h || !h->pq_codes, RIHIP_ERR_STATE,
                "sq8_update_apply: a PQ index is not updated in place (its codebooks are trained on the corpus): rebuild it");
  RIHIP_REQUIRE(h && h->codes && h->N > 0, RIHIP_ERR_STATE, "sq8_update_apply: index is empty");
  Sq8Codes stg;
  return sq8_update_run(h, stg, item_ids, drop_ids, n_drop, X_add, add_ids, add_tags, n_add, item_ids_out, n_total, n_dropped, n_clamped,
                        bad_id, bad_kind, (hipStream_t)stream);
}

extern "C" int rihip_sq8_update_assign(void* handle, const float* X, int64_t n, int32_t* assign_out, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "sq8_update_assign: index is empty");
  RIHIP_REQUIRE(X && assign_out && n > 0, RIHIP_ERR_ARG, "sq8_update_assign: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (h->nlist == 1) {   // a flat-built handle: its one list
    HIPCHK(hipMemsetAsync(assign_out, 0, sizeof(int32_t) * (size_t)n, st));
    return RIHIP_OK;
  }
  RCCHK(sq8_rows_at_dk(h, X, n, "sq8_update_assign: the rows must be 16-byte aligned", st));
  return launch_assign(h->dk, X, n, h->C, h->nlist, assign_out, st);
}

extern "C" int rihip_sq8_update_stats(void* handle, int64_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "sq8_update_stats: bad arguments");
  for (int i = 0; i < 4; ++i) out[i] = h->upd_stats[i];
  return RIHIP_OK;
}
