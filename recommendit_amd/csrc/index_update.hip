// Add / remove / replace items of a built index without retraining -- what faiss offers as add_with_ids / remove_ids
// behind FAISSIndex.add_items / remove_items / update_items.
//
// One update is ONE repack of the corpus on the device under the existing centroids; it leaves the handle bit for bit
// in the state a from-scratch rihip_ip_index_set_vectors + rihip_ip_index_set_ivf of the final corpus (same centroids,
// same list of every row) would leave it in:
//   mask     : drop ids sorted (rocPRIM); every stored row's id binary-searches them (index_update_mask_kernel, which
//              also counts the hits and checks the ids to add against the rows that stay)
//   renumber : exclusive scan of the keep flags in insertion order; appended rows get N_keep + j
//   lists    : exclusive scan of the keep flags in PHYSICAL order -> kept rows per list; the new rows are assigned
//              (launch_assign) and grouped stably (Grouper); one device->host read of <= 2*2048+5 integers gives the new
//              list lengths, offsets and granule table (the one synchronisation build_lists has as well)
//   repack   : index_update_repack_kernel -- source driven: a kept row goes to its list's new offset + its rank among
//              the list's kept rows (old physical order = ascending row number), a new row behind them in insertion
//              order, the padding of every list is written as zero rows with row id -1.  16-byte accesses, d/4 lanes per
//              row, streaming: ~2*N*d*4 bytes.
// Flat index: index_update_compact_kernel with the same mask and scan, then prepare_flat.
// No float atomics, no data-dependent order: bitwise reproducible.  The new arrays are built next to the old ones and
// swapped in at the end (peak device memory = old + new corpus); a call that fails leaves the old index searchable.
#include "common.h"
#include "recommendit_hip.h"
#include "ip_index.h"
#include "index_update_kernels.h"

#include <stdlib.h>
#include <string.h>
#include <vector>

#include <rocprim/rocprim.hpp>

using namespace rihip_index;

namespace {

// (sorted ids, keep masks, id checks, list counts and result ids: index_update_kernels.h, shared with the 8-bit index)
struct RepackArgs {
  const float* X_old; const int64_t* row_ids_old; const int* tile_list_old; const int64_t* poff_old; int64_t Np_old;
  const int* keep; const int* rscan; const int* pscan;
  const float* X_add; const int* g_rows; const int* g_keys; const int* g_off; int64_t n_add;
  const unsigned long long* cnt_keep; const int64_t* poff_new;
  float* X_new; int64_t* row_ids_new; int64_t n_keep; int nlist; int d4;
};

// work item = one source row (d4 lanes, 16 bytes each): the Np_old physical rows, then the n_add new rows in grouped
// order, then 64 candidate padding rows per list.  Every destination row in [0, Np_new) is written exactly once.
__global__ __launch_bounds__(256) void index_update_repack_kernel(const RepackArgs a) {
  const int d4 = a.d4;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t it = idx / d4;
  const int c4 = (int)(idx % d4);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  int64_t dest, rid;
  if (it < a.Np_old) {
    const int64_t old = a.row_ids_old[it];
    if (old < 0 || !a.keep[old]) return;
    const int c = a.tile_list_old[it / TR];
    dest = a.poff_new[c] + (a.pscan[it] - a.pscan[a.poff_old[c]]);
    rid = a.rscan[old];
    v = reinterpret_cast<const f32x4*>(a.X_old + (size_t)it * d4 * 4)[c4];
  } else if ((it -= a.Np_old) < a.n_add) {
    const int j = a.g_rows[it], c = a.g_keys[it];
    dest = a.poff_new[c] + (int64_t)a.cnt_keep[c] + (it - a.g_off[c]);
    rid = a.n_keep + j;
    v = reinterpret_cast<const f32x4*>(a.X_add + (size_t)j * d4 * 4)[c4];
  } else {
    it -= a.n_add;
    const int c = (int)(it / TR);
    if (c >= a.nlist) return;
    dest = a.poff_new[c] + (int64_t)a.cnt_keep[c] + (a.g_off[c + 1] - a.g_off[c]) + it % TR;
    if (dest >= a.poff_new[c + 1]) return;
    rid = -1;
  }
  reinterpret_cast<f32x4*>(a.X_new + (size_t)dest * d4 * 4)[c4] = v;
  if (c4 == 0) a.row_ids_new[dest] = rid;
}

using Scratch = UpdateScratch;

struct Owned {   // everything the call must free on every way out
  Scratch s; Grouper g; float* Xn = nullptr; int64_t* rid_n = nullptr; int* tl_n = nullptr;
  ~Owned() { hipFree(s.base); g.release(); hipFree(Xn); hipFree(rid_n); hipFree(tl_n); }
};

}  // namespace

extern "C" int rihip_ip_index_update(void* handle, const int64_t* item_ids, const int64_t* drop_ids, int64_t n_drop,
                                     const float* X_add, const int64_t* add_ids, int64_t n_add, int64_t* item_ids_out,
                                     int64_t* n_total, int64_t* n_dropped, int64_t* bad_id, int* bad_kind, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && h->X && h->N > 0, RIHIP_ERR_STATE, "ip_index_update: index is empty");
  RIHIP_REQUIRE(!h->pending.active, RIHIP_ERR_STATE, "ip_index_update: a deferred search awaits rihip_ip_index_search_finish");
  RIHIP_REQUIRE(item_ids && item_ids_out && n_total && n_dropped && bad_id && bad_kind && n_drop >= 0 && n_add >= 0 &&
                (n_drop == 0 || drop_ids) && (n_add == 0 || (X_add && add_ids)), RIHIP_ERR_ARG, "ip_index_update: bad arguments");
  *bad_kind = 0; *bad_id = 0; *n_total = h->N; *n_dropped = 0;
  if (n_drop == 0 && n_add == 0) return RIHIP_OK;
  const int64_t N = h->N, Np = h->ivf ? h->Np : 0;
  const int d = h->d, d4 = d / 4, nlist = h->ivf ? h->nlist : 0;
  RIHIP_REQUIRE(N + n_add + (int64_t)TR * (nlist + 1) < (1ll << 31) && n_drop < (1ll << 31), RIHIP_ERR_ARG,
                "ip_index_update: %lld + %lld rows exceed the 2^31 row limit", (long long)N, (long long)n_add);
  hipStream_t st = (hipStream_t)stream;
  if (n_add > 0 && h->du != d) {   // zero-pad the new rows to the kernel width, as set_vectors does
    RCCHK(h->qpad.reserve(n_add * d));
    RCCHK(pad_rows(X_add, n_add, h->du, d, h->qpad.p, st));
    X_add = h->qpad.p;
  }
  RIHIP_REQUIRE((reinterpret_cast<uintptr_t>(X_add) & 15) == 0, RIHIP_ERR_ARG, "ip_index_update: X_add must be 16-byte aligned");

  Owned o;
  Scratch& s = o.s;
  const int64_t nhb = HB_LISTS + 2 * (int64_t)nlist + 1;
  const size_t o_hb = s.plan<unsigned long long>(nhb), o_sdrop = s.plan<int64_t>(n_drop), o_sadd = s.plan<int64_t>(n_add);
  const size_t o_keep = s.plan<int>(N + 1), o_rscan = s.plan<int>(N + 1), o_pkeep = s.plan<int>(Np + 1), o_pscan = s.plan<int>(Np + 1);
  const size_t o_anew = s.plan<int>(n_add), o_zoff = s.plan<int>(nlist + 1), o_poffn = s.plan<int64_t>(nlist + 1);
  size_t t_sort_d = 0, t_sort_a = 0, t_scan_r = 0, t_scan_p = 0;
  if (n_drop) HIPCHK(rocprim::radix_sort_keys(nullptr, t_sort_d, (const int64_t*)nullptr, (int64_t*)nullptr, (size_t)n_drop, 0, 64, st));
  if (n_add) HIPCHK(rocprim::radix_sort_keys(nullptr, t_sort_a, (const int64_t*)nullptr, (int64_t*)nullptr, (size_t)n_add, 0, 64, st));
  HIPCHK(rocprim::exclusive_scan(nullptr, t_scan_r, (const int*)nullptr, (int*)nullptr, 0, (size_t)(N + 1), rocprim::plus<int>(), st));
  if (h->ivf) HIPCHK(rocprim::exclusive_scan(nullptr, t_scan_p, (const int*)nullptr, (int*)nullptr, 0, (size_t)(Np + 1), rocprim::plus<int>(), st));
  size_t t_bytes = t_sort_d > t_sort_a ? t_sort_d : t_sort_a;
  if (t_scan_r > t_bytes) t_bytes = t_scan_r;
  if (t_scan_p > t_bytes) t_bytes = t_scan_p;
  const size_t o_temp = s.plan<char>((int64_t)t_bytes);
  if (hipMalloc((void**)&s.base, s.used) != hipSuccess) {
    rihip_set_error("ip_index_update: device allocation of %lld bytes failed", (long long)s.used);
    return RIHIP_ERR_HIP;
  }
  unsigned long long* hb = s.at<unsigned long long>(o_hb);
  int64_t* sdrop = s.at<int64_t>(o_sdrop);
  int64_t* sadd = s.at<int64_t>(o_sadd);
  int* keep = s.at<int>(o_keep);
  int* rscan = s.at<int>(o_rscan);
  int* pkeep = s.at<int>(o_pkeep);
  int* pscan = s.at<int>(o_pscan);
  int* a_new = s.at<int>(o_anew);
  int* zoff = s.at<int>(o_zoff);
  int64_t* poff_n = s.at<int64_t>(o_poffn);
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

  // 2. IVF: kept rows per list, list of every new row
  const int* g_rows = nullptr; const int* g_keys = nullptr; const int* g_off = zoff;
  if (h->ivf) {
    hipLaunchKernelGGL(index_update_pmask_kernel, dim3((unsigned)((Np + 1 + 255) / 256)), dim3(256), 0, st, h->row_ids, Np, keep, pkeep);
    RIHIP_CHECK_LAUNCH();
    { size_t tb = t_bytes; HIPCHK(rocprim::exclusive_scan(temp, tb, (const int*)pkeep, pscan, 0, (size_t)(Np + 1), rocprim::plus<int>(), st)); }
    HIPCHK(hipMemsetAsync(zoff, 0, sizeof(int) * (nlist + 1), st));
    if (n_add) {
      RCCHK(launch_assign(d, X_add, n_add, h->C, nlist, a_new, st));
      RCCHK(o.g.init(n_add, nlist, st));
      RCCHK(o.g.group(a_new, st));
      g_rows = o.g.rows; g_keys = o.g.keys; g_off = o.g.off;
    }
    hipLaunchKernelGGL(index_update_list_count_kernel, dim3((unsigned)((nlist + 1 + 255) / 256)), dim3(256), 0, st, pscan,
                       h->list_poff, g_off, nlist, hb);
    RIHIP_CHECK_LAUNCH();
  }

  // 3. the one synchronisation: counts and checks
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
  *n_dropped = n_gone;
  if (n_gone == 0 && n_add == 0) return RIHIP_OK;   // only unknown ids: nothing changes

  hipLaunchKernelGGL(index_update_ids_kernel, dim3((unsigned)((N + n_add + 255) / 256)), dim3(256), 0, st, item_ids, N, keep, rscan,
                     add_ids, n_add, n_keep, item_ids_out);
  RIHIP_CHECK_LAUNCH();

  if (!h->ivf) {
    HIPCHK(hipMalloc((void**)&o.Xn, sizeof(float) * (size_t)n_new * d));
    const int64_t tot = (N + n_add) * d4;
    hipLaunchKernelGGL(index_update_compact_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, h->X, N, keep, rscan,
                       X_add, n_add, n_keep, d4, o.Xn);
    RIHIP_CHECK_LAUNCH();
    HIPCHK(hipStreamSynchronize(st));
    hipFree(h->X); hipFree(h->Xb);
    drop_tags(h);
    h->X = o.Xn; o.Xn = nullptr; h->Xb = nullptr; h->max_norm = 0.f; h->N = n_new; h->id_map = nullptr;
    rihip_bump_generation();
    *n_total = n_new;
    return prepare_flat(h, st);
  }

  // 4. new list lengths, offsets, granule table
  std::vector<int64_t> len_n(nlist), poff(nlist + 1, 0);
  for (int c = 0; c < nlist; ++c) {
    len_n[c] = (int64_t)hbh[HB_LISTS + c] + (int64_t)(hbh[HB_LISTS + nlist + c + 1] - hbh[HB_LISTS + nlist + c]);
    poff[c + 1] = poff[c] + (len_n[c] + TR - 1) / TR * TR;
  }
  const int64_t Np_n = poff[nlist] > 0 ? poff[nlist] : TR;
  std::vector<int> tl(Np_n / TR, 0);
  for (int c = 0; c < nlist; ++c)
    for (int64_t t = poff[c] / TR; t < poff[c + 1] / TR; ++t) tl[t] = c;
  HIPCHK(hipMalloc((void**)&o.Xn, sizeof(float) * (size_t)Np_n * d));
  HIPCHK(hipMalloc((void**)&o.rid_n, sizeof(int64_t) * Np_n));
  HIPCHK(hipMalloc((void**)&o.tl_n, sizeof(int) * (Np_n / TR)));
  HIPCHK(hipMemcpyAsync(o.tl_n, tl.data(), sizeof(int) * (Np_n / TR), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(poff_n, poff.data(), sizeof(int64_t) * (nlist + 1), hipMemcpyHostToDevice, st));

  // 5. repack
  RepackArgs a;
  a.X_old = h->X; a.row_ids_old = h->row_ids; a.tile_list_old = h->tile_list; a.poff_old = h->list_poff; a.Np_old = Np;
  a.keep = keep; a.rscan = rscan; a.pscan = pscan;
  a.X_add = X_add; a.g_rows = g_rows; a.g_keys = g_keys; a.g_off = g_off; a.n_add = n_add;
  a.cnt_keep = hb + HB_LISTS; a.poff_new = poff_n;
  a.X_new = o.Xn; a.row_ids_new = o.rid_n; a.n_keep = n_keep; a.nlist = nlist; a.d4 = d4;
  const int64_t tot = (Np + n_add + (int64_t)nlist * TR) * d4;
  hipLaunchKernelGGL(index_update_repack_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, a);
  RIHIP_CHECK_LAUNCH();
  HIPCHK(hipStreamSynchronize(st));

  // 6. swap
  hipFree(h->X); hipFree(h->row_ids); hipFree(h->tile_list);
  h->X = o.Xn; h->row_ids = o.rid_n; h->tile_list = o.tl_n;
  o.Xn = nullptr; o.rid_n = nullptr; o.tl_n = nullptr;
  h->N = n_new; h->Np = Np_n; h->list_len = len_n; h->id_map = nullptr;
  *n_total = n_new;
  const int rc = derive_ivf_aux(h, st);
  rihip_bump_generation();
  return rc;
}

// real rows of every IVF list (host int64 [nlist])
extern "C" int rihip_ip_index_list_sizes(void* handle, int64_t* out) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && h->ivf && out, RIHIP_ERR_STATE, "ip_index_list_sizes: not an IVF index");
  for (int c = 0; c < h->nlist; ++c) out[c] = h->list_len[c];
  return RIHIP_OK;
}
