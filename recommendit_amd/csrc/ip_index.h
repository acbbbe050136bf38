// Handle of the inner-product index shared by the search (topk.hip and the kernel files behind search_kernels.h), ivf.hip
// (k-means, list layout, state I/O) and index_update.hip.
#pragma once
#include "common.h"

#include <type_traits>
#include <vector>

namespace rihip_index {

constexpr int TR = 64;         // list granule: every IVF list is padded to a multiple of TR physical rows
constexpr int TRS = 32;        // corpus rows per LDS tile of the exact-f32 scan kernel
constexpr int K_MAX = 16384;   // largest k served by the device select/sort buffer (128 KiB of LDS)
constexpr int NLIST_MAX = 2048;  // probe bitset: 64 words per query
constexpr int64_t XMASK_BUDGET = 64ll << 20;   // bytes of exclusion-mask scratch a search may hold: 512 queries at 1 M rows
// slots of IpIndex::search_stats, in the order rihip_ip_index_search_stats reports them (recommendit_hip.h)
enum SearchStat {
  ST_FLAT_DENSE = 0, ST_FLAT_F32, ST_FLAT_FUSED, ST_FLAT_UNFUSED, ST_IVF_UNFILTERED, ST_IVF_THRESHOLDED, ST_SAMPLE_TOP,
  ST_PREPARE_SMALL, ST_THR_QUERIES, ST_REDONE, ST_REDO_CHUNKS, ST_PASSES, ST_COUNT
};
static_assert(ST_COUNT == 12, "rihip_ip_index_search_stats reports 12 counters");

template <typename T>
struct DevBuf {
  T* p = nullptr;
  int64_t n = 0;
  __attribute__((noinline)) int reserve(int64_t want) {   // (one copy per element type for the driver's ~40 call sites)
    if (n >= want) return RIHIP_OK;
    if (p) { hipFree(p); rihip_bump_generation(); }   // a graph that captured the old pointer is stale now
    p = nullptr; n = 0;
    if (hipMalloc((void**)&p, sizeof(T) * (size_t)want) != hipSuccess) {
      rihip_set_error("ip_index: device allocation of %lld bytes failed", (long long)(sizeof(T) * (size_t)want));
      return RIHIP_ERR_HIP;
    }
    n = want;
    return RIHIP_OK;
  }
  void release() { if (p) { hipFree(p); rihip_bump_generation(); } p = nullptr; n = 0; }
};

struct IpIndex {
  int d = 0;             // kernel width: 32 / 64 / 128 (the template instantiations)
  int du = 0;            // caller's embedding width (1 .. 128): rows are zero-padded to d inside the handle, which
                         // changes no inner product (the extra terms are exact zeros of the fmaf chain)
  int64_t N = 0;         // real vectors
  float* X = nullptr;    // brute force: [N,d]; IVF: [Np,d] list-ordered, zero-padded to 64-row granules
  __bf16* Xb = nullptr;  // bf16 copy of X for the filter pass (flat index, N > 4*SAMPLE)
  float max_norm = 0.f;  // max row 2-norm (error bound of the bf16 filter)
  int two_precision = 1; // 1: bf16 filter + exact f32 re-score; 0: all-f32 search
  const int64_t* id_map = nullptr;   // optional device array: search results are id_map[row] instead of row (not owned)
  DevBuf<float> qnorm;
  // IVF
  int nlist = 0, nprobe = 1;
  bool ivf = false;
  int64_t Np = 0;              // padded physical rows
  float* C = nullptr;          // [nlist,d]
  int* tile_list = nullptr;    // [Np/64] list of each granule
  int64_t* list_poff = nullptr; // [nlist+1] first physical row of each list (device)
  int* list_len_dev = nullptr;  // [nlist] real rows of each list (device)
  int64_t* row_ids = nullptr;  // [Np] original row per physical row, -1 for padding
  // filtered search (rihip_ip_index_set_tags): one 32-bit tag word per scanned row, in the order the scan reads them
  // (flat: [N] row order; IVF: [Np] physical order, padding slots 0); null = untagged
  uint32_t* tags = nullptr;
  int64_t filt_stats[2] = {0, 0};   // queries searched filtered, of those re-done by the exact fallback
  // seen-item exclusion inside the scan (rihip_ip_index_search_excluding): bit p & 31 of xmask[q * W + (p >> 5)],
  // W = ceil(rows scanned / 32), is set iff the row at scan position p is excluded for query q of the chunk in flight.
  // The scratch is all zero between calls: a chunk sets its bits, searches and clears exactly the words it touched
  // (xmask_dirty: a call that failed in between; the next one zeroes the whole buffer first).
  int* inv_pos = nullptr;           // IVF: [N] original row -> physical position; built on first use (drop_inv_pos)
  DevBuf<uint32_t> xmask;
  bool xmask_dirty = false;
  int64_t xmask_budget = XMASK_BUDGET;
  int64_t excl_stats[3] = {0, 0, 0};   // queries searched this way, of those re-done exactly, mask chunks
  // what the search driver did since the handle was made (rihip_ip_index_search_stats; slots: SearchStat).  Host
  // counters of the driver functions in topk.hip: no kernel reads or writes them
  int64_t search_stats[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<int64_t> list_len;  // host copy
  // scratch (grown on demand, owned by the handle)
  DevBuf<uint64_t> cand, scand, fcand, seg;   // seg: per (query, corpus split) survivor segments of the bf16 filter
  DevBuf<int> seg_cnt;
  DevBuf<int> count, fail_flags, fail_list, n_fail, fcount;
  DevBuf<int> n_pass;             // filtered search: rows that pass each query's predicate (IVF: of its probed lists)
  DevBuf<uint32_t> fpred;         // filtered search: predicates of the queries being re-done
  DevBuf<float> thr, thr2, fQ, qpad;    // qpad: queries / rows zero-padded from du to d columns
  DevBuf<float> coarse;                                    // IVF: coarse scores [nq,nlist]
  DevBuf<int> probe_list, list_q, list_cnt, list_qoff, list_cur, work_off, plan;
  int* h_nfail = nullptr;  // pinned
  // deferred exactness check (rihip_ip_index_set_deferred_check): a thresholded IVF search of at most one internal chunk
  // returns without its host synchronisation; rihip_ip_index_search_finish() reads the failure count and re-does the
  // failed queries (unfiltered pass) into the same output rows
  bool defer_check = false, defer_ok = false;
  struct { bool active = false; const float* Q = nullptr; int64_t nq = 0; int k = 0; float* out_s = nullptr; int64_t* out_r = nullptr; } pending;
  hipEvent_t ev_fail = nullptr;      // recorded behind the failure count's copy of a deferred search (not while capturing)
  bool ev_recorded = false;
};

// a new row order or layout invalidates the tag copy: the index reports untagged until the caller sets tags again
inline void drop_tags(IpIndex* h) {
  if (h->tags) { hipFree(h->tags); h->tags = nullptr; }
}

// ... and the inverse of row_ids the exclusion mask is built through
inline void drop_inv_pos(IpIndex* h) {
  if (h->inv_pos) { hipFree(h->inv_pos); h->inv_pos = nullptr; }
}

inline void free_index_arrays(IpIndex* h) {
  rihip_bump_generation();
  drop_tags(h);
  drop_inv_pos(h);
  hipFree(h->X); hipFree(h->C); hipFree(h->tile_list); hipFree(h->list_poff); hipFree(h->list_len_dev); hipFree(h->row_ids); hipFree(h->Xb);
  h->X = nullptr; h->C = nullptr; h->tile_list = nullptr; h->list_poff = nullptr; h->list_len_dev = nullptr; h->row_ids = nullptr; h->Xb = nullptr;
  h->N = 0; h->Np = 0; h->ivf = false; h->nlist = 0; h->list_len.clear();
}

// The kernels are instantiated for the widths 32, 64 and 128: f(std::integral_constant<int, D>{}) for d == D.
template <typename F>
int dispatch_d(int d, F&& f) {
  if (d == 32) f(std::integral_constant<int, 32>{});
  else if (d == 64) f(std::integral_constant<int, 64>{});
  else if (d == 128) f(std::integral_constant<int, 128>{});
  else { rihip_set_error("ip_index: unsupported embed_dim=%d (32/64/128)", d); return RIHIP_ERR_SHAPE; }
  return RIHIP_OK;
}

// zero-pad n rows of width du (device) into rows of width d (device)
int pad_rows(const float* src, int64_t n, int du, int d, float* dst, hipStream_t st);
// flat index: (re)build the bf16 filter copy and the row-norm bound (scan_bf16.hip)
int prepare_flat(IpIndex* h, hipStream_t st);
// upload the per-list offsets/lengths the list-major scan reads (from the host copy list_len; ivf.hip)
int derive_ivf_aux(IpIndex* h, hipStream_t st);
// arg-max-IP list (lowest list id wins ties) of each of N device rows of width d under C [nlist,d] (ivf.hip)
int launch_assign(int d, const float* X, int64_t N, const float* C, int nlist, int* assign, hipStream_t st);
// (list,row) pairs sorted by list; rows ascending inside a list (the sort is stable); off: [nlist+1] list bounds (ivf.hip)
struct Grouper {
  int* keys = nullptr; int* rows_in = nullptr; int* rows = nullptr; int* off = nullptr; void* temp = nullptr;
  size_t temp_bytes = 0;
  int64_t N = 0; int nlist = 0; int end_bit = 1;
  int init(int64_t N_, int nlist_, hipStream_t st);
  int group(const int* assign, hipStream_t st);
  void release();
};

}  // namespace rihip_index

#define HIPCHK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { rihip_set_error("%s:%d %s", __FILE__, __LINE__, hipGetErrorString(_e)); return RIHIP_ERR_HIP; } } while (0)
#define RCCHK(e) do { int _rc = (e); if (_rc) return _rc; } while (0)
