// What the index-search driver (topk.hip) and the kernel files share: tile constants, the argument structs of the
// kernels and one launcher per kernel family.  A kernel sits in the anonymous namespace of its own file next to its
// launcher; the launcher picks the instantiation (width, filtered or not), owns the family's dynamic-LDS grant and
// reports a failed launch.
#pragma once
#include "ip_index.h"

namespace rihip_index __attribute__((visibility("hidden"))) {   // (internal to the library: not exported)

constexpr int QB = 128;         // queries per workgroup (32 per wave)
constexpr int SAMPLE = 16384;   // corpus rows scored for the threshold estimate
constexpr int CSTRIDE = 32;     // IVF candidate counters: one 128-byte line per query (same-line atomics serialise in L2)
constexpr int QBB = 256;  // queries per workgroup of the bf16 filter (64 per wave: two 32-query groups)
constexpr int TRB = 64;     // corpus rows per pipeline stage of the bf16 filter (two 32-row MFMA sub-tiles)
constexpr int SAMPLE_T = 8;  // threshold sample: scores kept per stream (query, corpus split, row half)

struct ScanArgs {
  const float* X;        // corpus [N,d] (list-ordered for IVF)
  const void* Xb;        // bf16 copy of the corpus [N,d] (filter pass of the two-precision search), or null
  int64_t n_virtual;     // virtual rows scanned: row(i) = i * row_stride
  int64_t row_stride;
  const float* Q;        // [nq,d]
  int64_t nq;
  const float* thr;      // [nq] or null (=> -inf)
  uint64_t* cand;        // [nq, cap]
  int64_t cap;
  int* count;            // [nq]
  int nsplit;            // splits of the tile sequence (gridDim.y)
  int dense;             // 1: slot = virtual row (no atomics, count preset); 0: atomic append
  int qgrid;                  // bf16 filter: number of query blocks (1-D XCD-aware launch)
  // bf16 filter: every (query, corpus split) pair has ONE writer (a wave), so its survivors go to a private segment
  // with the fill count kept in LDS -- no global atomic in the scan (returning global atomics cost 0.64 of 1.8 ms)
  uint64_t* seg;              // [nq, nsplit, seg_cap] keys
  int* seg_cnt;               // [nq, nsplit] survivors found (may exceed seg_cap: the query is then re-done exactly)
  int seg_cap;
  int cs;                     // ints between two queries' candidate counters (0/1 = dense; CSTRIDE = a 128-B line each)
  // filtered search (scan_kernel<D, true> only)
  const uint32_t* tags;       // [N] tag word of every corpus row
  const uint32_t* pred;       // query q's predicate (any_of, all_of, none_of) at pred[q * pred_stride]
  int pred_stride;            // 3 = one per query, 0 = one shared by the batch
  // seen-item exclusion (the masked instantiations of scan_kernel): row v * row_stride is excluded for query q iff bit
  // (row & 31) of xmask[mrow * xW + (row >> 5)] is set, mrow = xrow ? xrow[q] : q (xrow: the re-do's original queries)
  const uint32_t* xmask;
  int64_t xW;
  const int* xrow;
};

// ---- finalize: radix-select the k_sel best keys of query q, sort them, emit -------------------
struct FinArgs {
  const uint64_t* cand;  // [nq, cap]
  int64_t cap;
  const int* count;      // [nq * count_stride]
  int count_stride;      // 0/1 = dense
  const int* qmap;       // optional: output slot -> query index inside cand/count (fallback), or null
  int64_t nq;
  int k;                 // requested k (<= K_MAX)
  // mode 0: write top-k scores/rows ; mode 1: write thr[q] = score of the k_sel-th key
  int mode;
  int rank;              // mode 1: r
  float* out_scores;     // [nq_out, k]
  int64_t* out_rows;     // [nq_out, k]
  uint64_t* out_keys;    // mode 0, optional: write the k best KEYS (0-padded) instead of scores/rows (hierarchical select)
  const int* out_slot;   // optional: where query i's results go (fallback), or null
  float* thr_out;        // mode 1
  int* fail_flags;       // [nq] mode 0: 1 if count<need_min or count>cap
  int64_t need_min;      // min(k, N_effective): candidates required for exactness (0 => no check)
  // two-precision search: candidates were filtered by APPROXIMATE scores >= thr_chk[q]; the exact top-k is
  // proven complete iff its k-th exact score >= thr_chk[q] + eps_scale*qnorm[q] + 2e-6
  const float* thr_chk;
  const float* qnorm;
  float eps_scale;
  // IVF with a sampled threshold: fewer than k candidates is only acceptable when nothing was filtered (thr = -inf)
  const float* ivf_thr;
  const int64_t* id_map;  // optional: out_rows[i] = id_map[row] (the wrapper's faiss index -> item id), or null
  int* zero_me;           // optional: one int this launch resets (the failed-query counter of the kernels that follow)
  int* fail_list; int* n_fail;   // optional (mode 0): a failed query appends itself here (n_fail reset by an earlier launch's zero_me)
  int lds_keys;           // > 0: key slots in dynamic LDS behind the sort buffer (set by launch_finalize for small launches)
  int sort_slots;         // uint64 slots of the sort buffer in front of them
  // filtered search (finalize_kernel<true>): rows that pass query q's predicate at n_pass[q * n_pass_stride]; a query
  // fails when it holds fewer than min(k, n_pass) candidates -- fewer than k passing rows is an ordinary answer
  const int* n_pass;
  int n_pass_stride;
};

// fused refinement of the two-precision search (refine_kernel, select.hip)
struct RefineArgs {
  const uint64_t* seg; const int* seg_cnt; int nsplit, seg_cap;
  int64_t cap;            // candidate slots per query of the global scratch list `cand`
  int lds_slots;          // candidate slots in LDS; a longer list is refined in `cand` (same code, slower)
  uint64_t* cand;         // [nq, cap]
  const float* X; const float* Q; int64_t N; int k;
  const float* thr;       // approximate-score threshold the filter used (completeness proof)
  float eps_scale;
  float* out_scores; int64_t* out_rows; int* fail_flags;
  int* fail_list; int* n_fail;   // failed queries are appended here (n_fail zeroed by an earlier launch)
  const int64_t* id_map;  // optional: out_rows[i] = id_map[row] (the wrapper's faiss index -> item id), or null
};

// list-major IVF scan (ivf_scan_lm_kernel, ivf_search.hip)
struct LmArgs {
  const float* X;            // [Np,d] list-ordered corpus
  const float* Q;            // [nq,d]
  const float* thr;          // [nq] or null (every probed row is a candidate)
  uint64_t* cand;            // [nq, cap]
  int64_t cap;
  int* count;                // [nq]
  const int64_t* row_ids;    // [Np] original row of each physical row
  const int64_t* list_poff;  // [nlist+1] first physical row of each list (multiples of 64)
  const int* list_len;       // [nlist] real rows of each list
  const int* list_qoff;      // [nlist+1] first slot of each list in list_q
  const int* list_q;         // [nq*nprobe] query indices grouped by list
  const int* work_off;       // [nlist+1] first work item of each list
  const int* plan;           // [0] = number of work items, [1] = tiles per work item
  int nlist;
  int tile_step;             // visit every tile_step-th tile of a list (threshold sample), 1 = all
  int nprobe;                // list_q holds pair indices q * nprobe + p
  int count_stride;          // ints between two queries' candidate counters (32 = one 128-B line each: same-line
                             // atomics serialise in L2)
  int64_t dense_cap;         // > 0: dense slots, cand = [nq*nprobe, dense_cap] pre-zeroed keys (no atomics)
  int dense_ids;             // dense slots carry the original row id (unfiltered search) instead of 0 (threshold sample)
  // filtered search (ivf_scan_lm_kernel<D, true> only)
  const uint32_t* tags;      // [Np] tag word of every physical row (padding slots 0)
  const uint32_t* pred;      // query q's predicate at pred[q * pred_stride]
  int pred_stride;
  // seen-item exclusion (the masked instantiations): a 32-row tile at physical row p is the one aligned word
  // xmask[mrow * xW + (p >> 5)] of every query, mrow = xrow ? xrow[q] : q (xrow: the re-do's original queries)
  const uint32_t* xmask;
  int64_t xW;
  const int* xrow;
};

// one-launch IVF prepare of a small query batch (ivf_prepare_small_kernel, ivf_search.hip)
struct PrepSmallArgs {
  const float* Q; int64_t nq; const float* C; int nlist, nprobe;
  float* cs; int* probe_list; int* list_cnt; const int64_t* list_poff; int tile_step, target_items;
  int *list_qoff, *list_cur, *work_off, *plan, *count; int64_t n_count; int* list_q;
  uint64_t* zero_buf; int64_t zero_n;
};

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { rihip_set_error("%s launch: %s", what, hipGetErrorString(e)); return RIHIP_ERR_HIP; }
  return RIHIP_OK;
}

// ---- scan_f32.hip: exact-f32 scan (a.tags != null: the filtered instantiation, a.xmask != null: the masked ones);
// grid = (query blocks, corpus splits)
int launch_scan(int d, const ScanArgs& a, dim3 grid, hipStream_t st);

// ---- scan_bf16.hip: bf16 filter (mode 0) and its sample passes (1: dense, 2: register top-T) over a.nsplit corpus splits
// and a.qgrid query blocks (prepare_flat, declared in ip_index.h, lives there too)
int launch_scan_bf16(int d, int mode, const ScanArgs& a, hipStream_t st);

// ---- select.hip: select and re-score
// finalize: the sort buffer is dynamic LDS sized to the power of two >= k (mode 0); mode 1 needs none
int launch_finalize(const FinArgs& f, unsigned n, hipStream_t st);
// fused refinement, one workgroup per query
int launch_refine(int d, const RefineArgs& r, int64_t nq, hipStream_t st);
// the unfused re-score (k > 2048) around finalize: segments -> candidate lists, exact re-score of the lists
void launch_compact_segments(const uint64_t* seg, const int* seg_cnt, int nsplit, int seg_cap, uint64_t* cand, int64_t cap,
                             int* count, int cs, int64_t nq, hipStream_t st);
int launch_rerank(int d, const float* X, const float* Q, uint64_t* cand, int64_t cap, const int* count, float* qnorm,
                  int64_t N, const float* kth_approx, float eps_scale, int cs, int64_t nq, hipStream_t st);
// list[0 .. *n_fail) = the queries whose flag is set (n_fail zeroed by the caller)
void launch_collect_fail(const int* flags, int64_t nq, int* list, int* n_fail, hipStream_t st);

// ---- ivf_search.hip: coarse quantizer -> probed lists -> (query, list) pairs grouped by list -> list-major scan
int launch_ivf_prepare_small(int d, const PrepSmallArgs& p, unsigned grid, hipStream_t st);
int launch_ivf_coarse(int d, const float* Q, int64_t nq, const float* C, int nlist, float* cs, hipStream_t st);
void launch_ivf_select(const float* cs, int64_t nq, int nlist, int nprobe, int* probe_list, int* list_cnt, hipStream_t st);
void launch_ivf_plan(const int* list_cnt, const int64_t* list_poff, int nlist, int tile_step, int target_items, int* list_qoff,
                     int* list_cur, int* work_off, int* plan, int* count, int64_t n_count, hipStream_t st);
void launch_ivf_scatter(const int* probe_list, int64_t n_pairs, int nprobe, int* list_cur, int* list_q, hipStream_t st);
int launch_ivf_scan(int d, const LmArgs& a, unsigned grid, hipStream_t st);   // a.tags != null: filtered, a.xmask != null: masked

// ---- search_filter.hip: helpers of the filtered search
// n_pass[q] (pred_stride 3) or n_pass[0] (one shared predicate, pred_stride 0) = rows of the flat index that pass
void launch_count_pass(const uint32_t* tags, int64_t N, const uint32_t* pred, int pred_stride, int64_t nq, int* n_pass,
                       hipStream_t st);
// n_pass[q] += passing rows of query q's probed lists
void launch_count_pass_ivf(const uint32_t* tags, const int64_t* list_poff, const int* list_len, const int* probe_list,
                           int64_t nq, int nprobe, const uint32_t* pred, int pred_stride, int* n_pass, hipStream_t st);
// thr[q] = -inf where the sample held too few passing rows or all passing rows fit the candidate list
void launch_filt_thr(float* thr, const int* n_pass, int n_pass_stride, int64_t cap, int64_t nq, hipStream_t st);
void launch_gather_pred(const uint32_t* pred, const int* idx, int n, uint32_t* out, hipStream_t st);
void launch_tags_to_scan_order(const uint32_t* by_row, const int64_t* row_ids, int64_t Np, uint32_t* out, hipStream_t st);


// ---- search_exclude.hip: the per-query exclusion mask of a seen-item search inside the scan
// the seen lists every mask is built from (device arrays of the caller); query q reads row user_ids[q] (null: row q)
struct SeenArgs {
  const int64_t* user_ids;      // [nq] or null; an id outside [0, n_seen_rows) excludes nothing
  const int64_t* seen_offsets;  // [n_seen_rows + 1]
  int64_t n_seen_rows;
  const int32_t* seen_items;    // item ids, ascending and unique per row
  const int32_t* row_of;        // [n_ids] item id -> original row, -1 absent
  int64_t n_ids;
};
// inv_pos[row_ids[p]] = p for the real rows of the physical order
void launch_inv_pos(const int64_t* row_ids, int64_t Np, int* inv_pos, hipStream_t st);
// queries q0 .. q0 + nq of `s` -> mask rows 0 .. nq: set = 1 ORs the bit of every stored seen item in, set = 0 zeroes the
// words those bits live in.  inv_pos null: position = row (flat index)
void launch_xmask(const SeenArgs& s, int64_t q0, int64_t nq, const int* inv_pos, int64_t N, uint32_t* mask, int64_t W, int set,
                  hipStream_t st);
// n_pass[q] = rows of the flat index that pass query q's predicate (tags null: every row) and are not masked
void launch_count_pass_x(const uint32_t* tags, int64_t N, const uint32_t* pred, int pred_stride, const uint32_t* xmask, int64_t W,
                         int64_t nq, int* n_pass, hipStream_t st);
// n_pass[q] += such rows of query q's probed lists
void launch_count_pass_ivf_x(const uint32_t* tags, const int64_t* list_poff, const int* list_len, const int* probe_list, int64_t nq,
                             int nprobe, const uint32_t* pred, int pred_stride, const uint32_t* xmask, int64_t W, int* n_pass,
                             hipStream_t st);
// *out += non-zero words of buf[0 .. n)
void launch_count_nonzero(const uint32_t* buf, int64_t n, unsigned long long* out, hipStream_t st);

}  // namespace rihip_index
