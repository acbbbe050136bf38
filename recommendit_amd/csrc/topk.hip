// Inner-product top-K retrieval for gfx950 -- replaces the faiss calls behind
// FAISSIndex.search / batch_search (reference src/models/faiss_index.py:113, :145).
// This file is the host side: the search driver (one function per search path, search_pass selects) and the C ABI of the
// index handle.  The kernels and their launchers are in scan_f32.hip, scan_bf16.hip, select.hip, ivf_search.hip and
// search_filter.hip (search_kernels.h).
//
// Exact brute force, no score matrix in HBM:
//   small corpus (N <= 4 * SAMPLE): every score is a candidate key in a dense slot, then the select.
//   large corpus:
//   (0) threshold estimate: score a strided sample of the corpus, radix-select the r-th
//       largest sample score per query  (r chosen so that P(#{score>=thr} < k) ~ 1e-5)
//   (1) scan: scores >= thr[q] become (score,row) candidates of the query (rare: ~0.1-0.3 % of scores) -- on exact-f32
//       MFMA, or (two-precision, the default) on bf16 MFMA into per-(query, corpus split) segments
//   (2) two-precision: exact f32 re-score of the candidates and the proof that none is missing (fused: refine_kernel)
//   (3) finalize: one workgroup per query radix-selects the k best 64-bit keys
//       (orderable score << 32 | ~row: ties -> lowest row, total order) and bitonic-sorts them.
//   Queries whose candidate list under- or overflows (heavy ties / adversarial data) are
//   re-done exactly with thr=-inf and capacity N ("fallback"), so the result is always exact.
//
// IVF-Flat (IP): k-means lists built on device, corpus re-ordered list-contiguous and padded
// to the 64-row tile so a tile belongs to one list; the scan skips tiles whose list no query
// of the block probes and masks per query.
//
// Filtered search (rihip_ip_index_search_filtered; faiss SearchParameters.sel): one 32-bit tag word per row, one
// (any_of, all_of, none_of) predicate per query, tested in the scans' emit (the FILT instantiations of scan_kernel and
// ivf_scan_lm_kernel).  The thresholded paths count each query's passing rows first: few passing rows mean "keep them
// all", not "re-do the query".
#include "common.h"
#include "recommendit_hip.h"

#include <algorithm>
#include <math.h>
#include <string.h>
#include <vector>

#include "search_kernels.h"

using namespace rihip_index;

namespace {

__global__ void gather_rows_kernel(const float* __restrict__ Q, const int* __restrict__ idx, int n, int d, float* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < (int64_t)n * d) out[i] = Q[(size_t)idx[i / d] * d + (i % d)];
}

__global__ void map_rows_kernel(int64_t* rows, int64_t n, const int64_t* __restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const int64_t r = rows[i]; rows[i] = (r >= 0) ? ids[r] : -1; }
}

__global__ void fill_int_kernel(int* p, int64_t n, int v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

// One internal pass of a search: at most 4 096 queries of one call.
struct Search {
  IpIndex* h;
  const float* Q;          // [nq, h->d] device
  int64_t nq;
  int k;
  float* out_s;            // [nq, k]
  int64_t* out_r;          // [nq, k]
  hipStream_t st;
  // filtered search (rihip_ip_index_search_filtered), else null: the predicates the scans test against h->tags -- query q's at
  // pred[q * pred_stride]; pred_stride 3 = one per query, 0 = one shared by the batch.  The thresholded paths of a
  // filtered search count the passing rows first and never defer their exactness check.
  const uint32_t* pred;
  int pred_stride;
  // seen-item exclusion inside the scan (rihip_ip_index_search_excluding), else null: the mask rows of these queries
  // (row q, or row xrow[q] in the re-do of failed queries), xW words each.  Such a search goes the way a filtered one
  // goes, with or without predicates.
  const uint32_t* xmask = nullptr;
  int64_t xW = 0;
  const int* xrow = nullptr;
  bool filt() const { return pred || xmask; }   // rows are tested in the scans: the counted, synchronising paths
};

void gather_rows(const Search& s, const int* idx, int n, float* out) {
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n * s.h->d + 255) / 256)), dim3(256), 0, s.st, s.Q, idx, n, s.h->d, out);
}

// The Search of the re-do of `n` failed queries of `s` (the fail-list entries `slots`): their rows of Q are in h->fQ
// (gather_rows), their predicates are gathered into h->fpred here, in the same order.
Search redo_of(const Search& s, const int* slots, int n) {
  Search r = s;
  r.Q = s.h->fQ.p; r.nq = n;
  if (s.pred && s.pred_stride) {
    launch_gather_pred(s.pred, slots, n, s.h->fpred.p, s.st);
    r.pred = s.h->fpred.p;
  }
  if (s.xmask) r.xrow = slots;   // (the fail list holds the queries' positions in `s`: their mask rows)
  return r;
}

FinArgs fin_args(const Search& s) {
  FinArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.nq = s.nq; fa.k = s.k; fa.count = s.h->count.p; fa.out_scores = s.out_s; fa.out_rows = s.out_r; fa.id_map = s.h->id_map;
  return fa;
}

// The failure count of the thresholded pass just enqueued, read on the host (one synchronisation).
int read_fail_count(const Search& s, int* nf) {
  HIPCHK(hipStreamSynchronize(s.st));
  *nf = *s.h->h_nfail;
  if (s.pred) s.h->filt_stats[1] += *nf;
  if (s.xmask) s.h->excl_stats[1] += *nf;
  return RIHIP_OK;
}

// ------------------------------------------ IVF paths ------------------------------------------
constexpr int IVF_TARGET = 16 * RIHIP_NCU;  // wave work items aimed at: 2 waves per SIMD on every CU, twice over
constexpr int IVF_SS = 16;                  // threshold sample: every 16th probed tile

struct IvfGeom {
  int nlist, nprobe;
  int64_t cap_full;    // population upper bound of one query = the nprobe longest lists
  int64_t max_tiles;   // 32-row tiles of the longest list (padded to the 64-row granule)
  int64_t cap_lf;      // dense slots per (query, probe) pair of the unfiltered pass: the longest list
  int64_t cap_df;      // ... per query
};
int ivf_geom(const IpIndex* h, IvfGeom* g) {
  std::vector<int64_t> ll = h->list_len;
  std::sort(ll.begin(), ll.end(), [](int64_t x, int64_t y) { return x > y; });
  g->cap_full = 0;
  for (int i = 0; i < h->nprobe && i < (int)ll.size(); ++i) g->cap_full += ll[i];
  if (g->cap_full < 1) g->cap_full = 1;
  g->nlist = h->nlist;
  g->nprobe = h->nprobe < h->nlist ? h->nprobe : h->nlist;
  RIHIP_REQUIRE(g->nlist <= NLIST_MAX, RIHIP_ERR_SHAPE, "ip_index: nlist=%d > %d unsupported", g->nlist, NLIST_MAX);
  g->max_tiles = 0;
  for (int c = 0; c < g->nlist; ++c) g->max_tiles = std::max<int64_t>(g->max_tiles, (h->list_len[c] + TR - 1) / TR * (TR / TRS));
  g->cap_lf = std::max<int64_t>(g->max_tiles * TRS, TRS);
  g->cap_df = g->cap_lf * g->nprobe;
  return RIHIP_OK;
}

// coarse quantizer -> probed lists -> (query, list) pairs grouped by list, planned for a first scan with tile step
// `first_tile_step`; zeroes `zero_buf` (the dense slots of that scan: key 0 = below every score)
int ivf_prepare(const Search& s, const IvfGeom& g, int first_tile_step, uint64_t* zero_buf, int64_t zero_n) {
  IpIndex* h = s.h;
  const int64_t n = s.nq;
  const int nlist = g.nlist, nprobe = g.nprobe;
  RCCHK(h->coarse.reserve(n * nlist));
  RCCHK(h->probe_list.reserve(n * nprobe));
  RCCHK(h->list_q.reserve(n * nprobe));
  RCCHK(h->list_cnt.reserve(nlist)); RCCHK(h->list_qoff.reserve(nlist + 1)); RCCHK(h->list_cur.reserve(nlist));
  RCCHK(h->work_off.reserve(nlist + 1)); RCCHK(h->plan.reserve(2));
  if (n <= 8) {   // one launch (see ivf_prepare_small_kernel): the single workgroup takes the queries 4 at a time, so beyond a
                  // handful of queries the four parallel kernels are faster (64 queries: 0.48 vs 0.37 ms per batch)
    ++h->search_stats[ST_PREPARE_SMALL];
    PrepSmallArgs p;
    p.Q = s.Q; p.nq = n; p.C = h->C; p.nlist = nlist; p.nprobe = nprobe; p.cs = h->coarse.p; p.probe_list = h->probe_list.p;
    p.list_cnt = h->list_cnt.p; p.list_poff = h->list_poff; p.tile_step = first_tile_step; p.target_items = IVF_TARGET;
    p.list_qoff = h->list_qoff.p; p.list_cur = h->list_cur.p; p.work_off = h->work_off.p; p.plan = h->plan.p;
    p.count = h->count.p; p.n_count = n * CSTRIDE; p.list_q = h->list_q.p; p.zero_buf = zero_buf; p.zero_n = zero_buf ? zero_n : 0;
    int64_t zb = zero_buf ? (zero_n + 256 * 16 - 1) / (256 * 16) : 0;      // ~16 stores per thread
    if (zb > 2 * RIHIP_NCU) zb = 2 * RIHIP_NCU;
    return launch_ivf_prepare_small(h->d, p, (unsigned)(1 + zb), s.st);
  }
  if (zero_buf) HIPCHK(hipMemsetAsync(zero_buf, 0, sizeof(uint64_t) * (size_t)zero_n, s.st));
  HIPCHK(hipMemsetAsync(h->list_cnt.p, 0, sizeof(int) * nlist, s.st));
  RCCHK(launch_ivf_coarse(h->d, s.Q, n, h->C, nlist, h->coarse.p, s.st));
  launch_ivf_select(h->coarse.p, n, nlist, nprobe, h->probe_list.p, h->list_cnt.p, s.st);
  // slot offsets + the work split of the first scan + zeroed candidate counters
  launch_ivf_plan(h->list_cnt.p, h->list_poff, nlist, first_tile_step, IVF_TARGET, h->list_qoff.p, h->list_cur.p, h->work_off.p,
                  h->plan.p, h->count.p, n * CSTRIDE, s.st);
  launch_ivf_scatter(h->probe_list.p, n * nprobe, nprobe, h->list_cur.p, h->list_q.p, s.st);
  return check_launch("ivf prepare");
}

// one IVF pass over the queries of `s`: plan (tile split for this sampling step) -> list-major scan
int ivf_scan(const Search& s, const IvfGeom& g, const float* thr, uint64_t* cand, int64_t cap, int tile_step, int64_t dense_cap,
             bool planned, int dense_ids) {
  IpIndex* h = s.h;
  if (!planned)   // (ivf_prepare already planned for the first scan that follows it)
    launch_ivf_plan(h->list_cnt.p, h->list_poff, g.nlist, tile_step, IVF_TARGET, h->list_qoff.p, h->list_cur.p, h->work_off.p,
                    h->plan.p, h->count.p, s.nq * CSTRIDE, s.st);
  LmArgs x;
  memset(&x, 0, sizeof(x));
  x.X = h->X; x.Q = s.Q; x.thr = thr; x.cand = cand; x.cap = cap; x.count = h->count.p; x.row_ids = h->row_ids;
  x.list_poff = h->list_poff; x.list_len = h->list_len_dev; x.list_qoff = h->list_qoff.p; x.list_q = h->list_q.p;
  x.work_off = h->work_off.p; x.plan = h->plan.p; x.nlist = g.nlist; x.tile_step = tile_step; x.nprobe = g.nprobe;
  x.dense_cap = dense_cap; x.count_stride = CSTRIDE; x.dense_ids = dense_ids;
  if (s.pred) { x.tags = h->tags; x.pred = s.pred; x.pred_stride = s.pred_stride; }
  if (s.xmask) { x.xmask = s.xmask; x.xW = s.xW; x.xrow = s.xrow; }
  // n_work <= sum over (list, group) of (tiles/tpi + 1) <= target + #(list, query group) pairs
  const int64_t bound = (int64_t)IVF_TARGET + g.nlist + (s.nq * g.nprobe + 31) / 32 + 4;
  return launch_ivf_scan(h->d, x, (unsigned)((bound + 3) / 4), s.st);
}

// Unfiltered pass (every probed vector is a candidate): small populations, small batches and the exact re-do.
// Every (query, probed list) pair owns a dense slot range (slot = row inside the list): no atomics, no threshold sample,
// no exactness check and no host sync.  out_slot: the output row of every query (the re-do), or null.
int ivf_unfiltered(const Search& s, const IvfGeom& g, const int* out_slot) {
  IpIndex* h = s.h;
  const int64_t n = s.nq;
  RCCHK(h->fcand.reserve(n * g.cap_df));
  RCCHK(ivf_prepare(s, g, 1, h->fcand.p, n * g.cap_df));
  RCCHK(ivf_scan(s, g, nullptr, h->fcand.p, g.cap_df, 1, g.cap_lf, true, 1));
  // two-level select: the k best keys of every (query, probe) pair (one workgroup per pair), then the k best of a
  // query's nprobe * k survivors -- a single workgroup over all ~100k slots of a query took 150 us
  const int64_t np_ = n * g.nprobe;
  RCCHK(h->scand.reserve(np_ * s.k));
  FinArgs f1;      // (count = null: every list is full -- all cap_lf dense slots of a pair, all nprobe * k survivors)
  memset(&f1, 0, sizeof(f1));
  f1.nq = np_; f1.k = s.k; f1.count = nullptr; f1.cand = h->fcand.p; f1.cap = g.cap_lf; f1.mode = 0; f1.out_keys = h->scand.p;
  RCCHK(launch_finalize(f1, (unsigned)np_, s.st));
  FinArgs f2;
  memset(&f2, 0, sizeof(f2));
  f2.nq = n; f2.k = s.k; f2.count = nullptr; f2.out_scores = s.out_s; f2.out_rows = s.out_r; f2.cand = h->scand.p;
  f2.cap = (int64_t)g.nprobe * s.k; f2.mode = 0; f2.out_slot = out_slot; f2.id_map = h->id_map;
  return launch_finalize(f2, (unsigned)n, s.st);
}

// Threshold too aggressive (or candidate overflow) for the `nf` queries of h->fail_list: unfiltered re-do, 64 at a time.
int ivf_redo(const Search& s, const IvfGeom& g, int nf) {
  IpIndex* h = s.h;
  const int FCH = 64;
  RCCHK(h->fQ.reserve((int64_t)FCH * h->d));
  h->search_stats[ST_REDONE] += nf;
  for (int f0 = 0; f0 < nf; f0 += FCH) {
    const int nfc = (nf - f0 < FCH) ? nf - f0 : FCH;
    ++h->search_stats[ST_REDO_CHUNKS];
    gather_rows(s, h->fail_list.p + f0, nfc, h->fQ.p);
    RCCHK(ivf_unfiltered(redo_of(s, h->fail_list.p + f0, nfc), g, h->fail_list.p + f0));
  }
  return RIHIP_OK;
}

// Thresholded pass: (A) every IVF_SS-th tile of each probed list scored into dense slots, the rank-th best is the
// query's threshold; (B) all probed tiles, scores >= threshold appended; select + exactness check; the queries that
// fail it are re-done unfiltered -- now, or by rihip_ip_index_search_finish when the check is deferred.
int ivf_thresholded(const Search& s, const IvfGeom& g) {
  IpIndex* h = s.h;
  const int64_t nq = s.nq;
  const int k = s.k;
  const int SS = IVF_SS;
  const double m = (double)k / SS;
  const int rank = (int)ceil(m + 4.0 * sqrt(m) + 4.0);
  int64_t cap = 4096;
  while ((double)cap < 2.5 * rank * SS) cap <<= 1;
  if (cap > g.cap_full) cap = g.cap_full;
  const int64_t cap_l = (g.max_tiles + SS - 1) / SS * TRS;             // sampled rows of the longest list
  const int64_t cap_s = cap_l * g.nprobe;
  ++h->search_stats[ST_IVF_THRESHOLDED];
  h->search_stats[ST_THR_QUERIES] += nq;
  RCCHK(h->scand.reserve(nq * cap_s));
  RCCHK(h->cand.reserve(nq * cap));
  // ---- pass A
  RCCHK(ivf_prepare(s, g, SS, h->scand.p, nq * cap_s));
  if (s.filt()) {   // passing (and unmasked) rows of every query's probed lists
    HIPCHK(hipMemsetAsync(h->n_pass.p, 0, sizeof(int) * nq, s.st));
    if (s.xmask) launch_count_pass_ivf_x(s.pred ? h->tags : nullptr, h->list_poff, h->list_len_dev, h->probe_list.p, nq, g.nprobe,
                                         s.pred, s.pred_stride, s.xmask, s.xW, h->n_pass.p, s.st);
    else launch_count_pass_ivf(h->tags, h->list_poff, h->list_len_dev, h->probe_list.p, nq, g.nprobe, s.pred, s.pred_stride,
                               h->n_pass.p, s.st);
  }
  RCCHK(ivf_scan(s, g, nullptr, h->scand.p, cap_s, SS, cap_l, true, 0));
  // (the sample's lists are dense: count = null means cap_s keys each; this launch also resets the failed-query counter
  // that the final select appends to -- no fill / collect launches of their own)
  FinArgs fa = fin_args(s);
  fa.cand = h->scand.p; fa.cap = cap_s; fa.mode = 1; fa.rank = rank; fa.thr_out = h->thr.p; fa.count = nullptr;
  fa.zero_me = h->n_fail.p;
  RCCHK(launch_finalize(fa, (unsigned)nq, s.st));
  if (s.filt()) {   // (the sampled share of the passing rows beats the threshold like the sampled share of all rows did: same rank)
    launch_filt_thr(h->thr.p, h->n_pass.p, 1, cap, nq, s.st);
    fa.n_pass = h->n_pass.p; fa.n_pass_stride = 1;
  }
  // ---- pass B
  RCCHK(ivf_scan(s, g, h->thr.p, h->cand.p, cap, 1, 0, false, 0));
  fa.cand = h->cand.p; fa.cap = cap; fa.mode = 0; fa.thr_out = nullptr; fa.fail_flags = h->fail_flags.p;
  fa.count = h->count.p; fa.zero_me = nullptr; fa.fail_list = h->fail_list.p; fa.n_fail = h->n_fail.p;
  fa.ivf_thr = h->thr.p; fa.count_stride = CSTRIDE;
  RCCHK(launch_finalize(fa, (unsigned)nq, s.st));
  // ---- exactness check
  HIPCHK(hipMemcpyAsync(h->h_nfail, h->n_fail.p, sizeof(int), hipMemcpyDeviceToHost, s.st));
  if (h->defer_check && h->defer_ok && !s.filt()) {   // the caller checks later (rihip_ip_index_search_finish): no host sync here
    // finish then waits for THIS point of the stream only: whatever the caller enqueues behind the search keeps the GPU
    // busy while the host is already back (a capturing stream records no event: replays use _last_fail_count)
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(s.st, &cs);
    h->ev_recorded = false;
    if (cs == hipStreamCaptureStatusNone) {
      if (!h->ev_fail) HIPCHK(hipEventCreateWithFlags(&h->ev_fail, hipEventDisableTiming));
      HIPCHK(hipEventRecord(h->ev_fail, s.st));
      h->ev_recorded = true;
    }
    h->pending.active = true; h->pending.Q = s.Q; h->pending.nq = nq; h->pending.k = k; h->pending.out_s = s.out_s; h->pending.out_r = s.out_r;
    return RIHIP_OK;
  }
  int nf = 0;
  RCCHK(read_fail_count(s, &nf));
  return nf > 0 ? ivf_redo(s, g, nf) : RIHIP_OK;
}

// ------------------------------------------ flat paths -----------------------------------------
int pick_nsplit(int64_t nq, int64_t n_tiles) {
  const int64_t qblocks = (nq + QB - 1) / QB;
  int64_t ns = (2 * RIHIP_NCU + qblocks - 1) / qblocks;  // aim at >= 2 workgroups per CU
  if (ns > n_tiles) ns = n_tiles;
  if (ns < 1) ns = 1;
  if (ns > 65535) ns = 65535;
  return (int)ns;
}
// corpus splits of the bf16 passes: `wgs_per_cu` resident workgroups per CU (launch bounds: filter 3, sample 2)
int bf16_nsplit(int64_t nq, int64_t tiles, int wgs_per_cu) {
  const int64_t qblocks = (nq + QBB - 1) / QBB;
  int64_t ns = (wgs_per_cu * RIHIP_NCU + qblocks - 1) / qblocks;
  if (ns > tiles) ns = tiles;
  if (ns < 1) ns = 1;
  if (ns > 65535) ns = 65535;
  return (int)ns;
}

ScanArgs scan_args(const Search& s) {
  ScanArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.X = s.h->X; sa.Q = s.Q; sa.nq = s.nq; sa.count = s.h->count.p;
  if (s.pred) { sa.tags = s.h->tags; sa.pred = s.pred; sa.pred_stride = s.pred_stride; }
  if (s.xmask) { sa.xmask = s.xmask; sa.xW = s.xW; sa.xrow = s.xrow; }
  return sa;
}
unsigned f32_qgrid(int64_t nq) { return (unsigned)((nq + QB - 1) / QB); }
int64_t f32_tiles(const IpIndex* h) { return (h->N + TRS - 1) / TRS; }

// small corpus: every score is a candidate (dense slots, no atomics)
int flat_dense(const Search& s) {
  IpIndex* h = s.h;
  const int64_t nq = s.nq;
  ++h->search_stats[ST_FLAT_DENSE];
  RCCHK(h->cand.reserve(nq * h->N));
  hipLaunchKernelGGL(fill_int_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s.st, h->count.p, nq, (int)h->N);
  ScanArgs sa = scan_args(s);
  sa.n_virtual = h->N; sa.row_stride = 1; sa.thr = nullptr; sa.cand = h->cand.p; sa.cap = h->N; sa.dense = 1;
  sa.nsplit = pick_nsplit(nq, f32_tiles(h));
  RCCHK(launch_scan(h->d, sa, dim3(f32_qgrid(nq), sa.nsplit), s.st));
  FinArgs fa = fin_args(s);
  fa.cand = h->cand.p; fa.cap = h->N; fa.mode = 0;
  return launch_finalize(fa, (unsigned)nq, s.st);
}

// exact re-do of the `nf` under/overflowed queries of h->fail_list (heavy ties, adversarial data): dense scan with
// capacity N, 8 queries at a time
int flat_redo(const Search& s, int nf) {
  IpIndex* h = s.h;
  const int FCH = 8;
  RCCHK(h->fcand.reserve((int64_t)FCH * h->N));
  RCCHK(h->fQ.reserve((int64_t)FCH * h->d));
  RCCHK(h->fcount.reserve(FCH));
  h->search_stats[ST_REDONE] += nf;
  for (int f0 = 0; f0 < nf; f0 += FCH) {
    const int nfc = (nf - f0 < FCH) ? nf - f0 : FCH;
    ++h->search_stats[ST_REDO_CHUNKS];
    gather_rows(s, h->fail_list.p + f0, nfc, h->fQ.p);
    hipLaunchKernelGGL(fill_int_kernel, dim3(1), dim3(64), 0, s.st, h->fcount.p, nfc, (int)h->N);
    ScanArgs fs = scan_args(redo_of(s, h->fail_list.p + f0, nfc));
    fs.n_virtual = h->N; fs.row_stride = 1; fs.thr = nullptr;
    fs.cand = h->fcand.p; fs.cap = h->N; fs.count = h->fcount.p; fs.dense = 1; fs.nsplit = pick_nsplit(nfc, f32_tiles(h));
    RCCHK(launch_scan(h->d, fs, dim3(1, fs.nsplit), s.st));
    FinArgs ff;
    memset(&ff, 0, sizeof(ff));
    ff.cand = h->fcand.p; ff.cap = h->N; ff.count = h->fcount.p; ff.nq = nfc; ff.k = s.k; ff.mode = 0;
    ff.out_scores = s.out_s; ff.out_rows = s.out_r; ff.out_slot = h->fail_list.p + f0; ff.id_map = h->id_map;
    RCCHK(launch_finalize(ff, (unsigned)nfc, s.st));
  }
  return check_launch("fallback");
}

// Large corpus: sample -> threshold -> filter -> re-score or refine -> check.  All-f32, or two-precision (bf16 filter,
// exact f32 re-score with a completeness proof).  A filtered search takes the all-f32 scan: the bf16 filter does not
// read tags.
int flat_thresholded(const Search& s) {
  IpIndex* h = s.h;
  const int64_t nq = s.nq;
  const int k = s.k, d = h->d;
  const bool two_prec = h->two_precision && h->Xb != nullptr && !s.filt();
  // the two-precision path samples twice as many rows: the threshold estimate tightens (expected survivors per query
  // 2 200 -> 1 700 at k = 500, N = 1 M), which saves more in the filter's emission and in the re-score than the longer
  // sample pass costs (measured 2.33 -> 2.16 ms per 4 096 queries; 3x, 4x the same, 6x slower again)
  const int64_t n_sample = (int64_t)SAMPLE * (two_prec ? 2 : 1);
  const int64_t stride = h->N / n_sample > 0 ? h->N / n_sample : 1;
  const int64_t S = (h->N + stride - 1) / stride;  // virtual rows i*stride < N
  const double m = (double)k * (double)S / (double)h->N;
  // rank of the sample score used as threshold; the two-precision filter needs a little more head-room because
  // the completeness proof asks for s_k >= thr + eps
  const int rank = (int)ceil((m + 4.0 * sqrt(m) + 4.0) * (two_prec ? 1.5 : 1.0));
  const double expect = (double)rank * (double)h->N / (double)S;
  int64_t cap = 4096;
  while ((double)cap < 2.5 * expect) cap <<= 1;
  if (cap > h->N) cap = h->N;
  RCCHK(h->scand.reserve(nq * S));
  RCCHK(h->cand.reserve(nq * cap));
  const int64_t filter_tiles = two_prec ? (h->N + TRB - 1) / TRB : f32_tiles(h);
  const int64_t sample_tiles = (S + (two_prec ? TRB : TRS) - 1) / (two_prec ? TRB : TRS);
  int seg_cap = 64;   // per (query, corpus split) segment of the bf16 filter: 4x the expected survivors
  if (two_prec) {
    while ((double)seg_cap < 4.0 * expect / bf16_nsplit(nq, filter_tiles, 3)) seg_cap <<= 1;
    if ((int64_t)seg_cap > cap) seg_cap = (int)cap;
  }
  // The two-precision sample pass keeps the SAMPLE_T best scores of every stream (query x corpus split x row half) in
  // registers instead of writing all S scores per query.  The threshold is the rank-th best of their union: exact while no
  // stream holds more than SAMPLE_T of the sample's top `rank` -- with rank <= streams * SAMPLE_T / 4 (mean <= 2 per
  // stream) a stream overflows with probability ~2e-4, and an overflow only lowers the threshold (more survivors, same
  // result).  Larger ranks keep the dense sample.
  const int64_t streams = (int64_t)2 * bf16_nsplit(nq, sample_tiles, 2);
  const bool sample_top = two_prec && (int64_t)rank * 4 <= streams * SAMPLE_T;
  const int64_t cap_s = sample_top ? streams * SAMPLE_T : S;
  ++h->search_stats[!two_prec ? ST_FLAT_F32 : (k <= 2048 ? ST_FLAT_FUSED : ST_FLAT_UNFUSED)];
  if (sample_top) ++h->search_stats[ST_SAMPLE_TOP];
  h->search_stats[ST_THR_QUERIES] += nq;

  // ---- sample: a strided share of the corpus, dense (the register top-T sample writes every stream slot, empty streams as key 0)
  ScanArgs sa = scan_args(s);
  sa.n_virtual = S; sa.row_stride = stride; sa.thr = nullptr; sa.cand = h->scand.p; sa.cap = cap_s; sa.dense = 1;
  if (two_prec) {
    sa.Xb = h->Xb; sa.qgrid = (int)((nq + QBB - 1) / QBB);
    sa.nsplit = bf16_nsplit(nq, sample_tiles, 2);
    RCCHK(launch_scan_bf16(d, sample_top ? 2 : 1, sa, s.st));
  } else {
    sa.nsplit = pick_nsplit(nq, sample_tiles);
    RCCHK(launch_scan(d, sa, dim3(f32_qgrid(nq), sa.nsplit), s.st));
  }
  // ---- threshold: the rank-th best sample score
  FinArgs fa = fin_args(s);
  fa.cand = h->scand.p; fa.cap = cap_s; fa.mode = 1; fa.rank = rank; fa.thr_out = h->thr.p;
  fa.count = nullptr;                  // dense sample lists: cap_s keys each
  fa.zero_me = h->n_fail.p;            // (reset here: refine_kernel appends the failed queries itself)
  RCCHK(launch_finalize(fa, (unsigned)nq, s.st));
  fa.count = h->count.p; fa.zero_me = nullptr;
  if (s.filt()) {   // exact passing-row counts; queries whose passing rows all fit the candidate list skip the threshold
    const int np_stride = (s.pred_stride == 0 && !s.xmask) ? 0 : 1;   // (a mask is per query whatever the predicate is)
    HIPCHK(hipMemsetAsync(h->n_pass.p, 0, sizeof(int) * (np_stride ? nq : 1), s.st));
    if (s.xmask) launch_count_pass_x(s.pred ? h->tags : nullptr, h->N, s.pred, s.pred_stride, s.xmask, s.xW, nq, h->n_pass.p, s.st);
    else launch_count_pass(h->tags, h->N, s.pred, s.pred_stride, nq, h->n_pass.p, s.st);
    launch_filt_thr(h->thr.p, h->n_pass.p, np_stride, cap, nq, s.st);
    fa.n_pass = h->n_pass.p; fa.n_pass_stride = np_stride;
  }
  // ---- filter: the thresholded scan (bf16: survivors into per-(query, split) segments; f32: appended through `count`)
  sa.n_virtual = h->N; sa.row_stride = 1; sa.thr = h->thr.p; sa.cand = h->cand.p; sa.cap = cap; sa.dense = 0;
  sa.cs = CSTRIDE; fa.count_stride = CSTRIDE;
  if (two_prec) {
    sa.nsplit = bf16_nsplit(nq, filter_tiles, 3);
    RIHIP_REQUIRE(sa.nsplit <= 1024, RIHIP_ERR_SHAPE, "ip_index: %d corpus splits", sa.nsplit);
    RCCHK(h->seg.reserve(nq * sa.nsplit * seg_cap));
    RCCHK(h->seg_cnt.reserve(nq * sa.nsplit));
    sa.seg = h->seg.p; sa.seg_cnt = h->seg_cnt.p; sa.seg_cap = seg_cap;
    RCCHK(launch_scan_bf16(d, 0, sa, s.st));
  } else {
    hipLaunchKernelGGL(fill_int_kernel, dim3((unsigned)((nq * CSTRIDE + 255) / 256)), dim3(256), 0, s.st, h->count.p, nq * CSTRIDE, 0);
    sa.nsplit = pick_nsplit(nq, filter_tiles);
    RCCHK(launch_scan(d, sa, dim3(f32_qgrid(nq), sa.nsplit), s.st));
  }
  const float eps_scale = (float)((1.0 / 256.0 + 1.0 / 262144.0) * (double)h->max_norm * 1.001);   // bf16 error bound
  if (two_prec && k <= 2048) {
    // ---- refine: one workgroup per query takes the survivors from the segments through approximate select, exact
    // re-score, top-k select + sort and the completeness proof; it appends the failed queries itself
    RefineArgs r;
    memset(&r, 0, sizeof(r));
    r.seg = h->seg.p; r.seg_cnt = h->seg_cnt.p; r.nsplit = sa.nsplit; r.seg_cap = seg_cap; r.cap = cap;
    r.lds_slots = 2048; r.cand = h->cand.p; r.X = h->X; r.Q = s.Q; r.N = h->N; r.k = k; r.thr = h->thr.p;
    r.eps_scale = eps_scale;
    r.out_scores = s.out_s; r.out_rows = s.out_r; r.fail_flags = h->fail_flags.p; r.id_map = h->id_map;
    r.fail_list = h->fail_list.p; r.n_fail = h->n_fail.p;
    RCCHK(launch_refine(d, r, nq, s.st));
  } else {
    if (two_prec) {  // ---- re-score: exact f32 scores of the survivors (keys rewritten in place)
      launch_compact_segments(h->seg.p, h->seg_cnt.p, sa.nsplit, seg_cap, h->cand.p, cap, h->count.p, CSTRIDE, nq, s.st);
      RCCHK(h->qnorm.reserve(nq));
      RCCHK(h->thr2.reserve(nq));
      {  // k-th largest APPROXIMATE score per query (a lower bound of it: the select stops early): rerank_kernel uses it
         // to skip survivors that provably cannot reach the top-k -- about half of them
        FinArgs f2 = fa;
        f2.cand = h->cand.p; f2.cap = cap; f2.mode = 1; f2.rank = k; f2.thr_out = h->thr2.p; f2.fail_flags = nullptr;
        f2.thr_chk = nullptr; f2.qnorm = nullptr; f2.ivf_thr = nullptr; f2.need_min = 0;
        RCCHK(launch_finalize(f2, (unsigned)nq, s.st));
      }
      RCCHK(launch_rerank(d, h->X, s.Q, h->cand.p, cap, h->count.p, h->qnorm.p, h->N, h->thr2.p, eps_scale, CSTRIDE, nq, s.st));
      fa.thr_chk = h->thr.p; fa.qnorm = h->qnorm.p;
      fa.eps_scale = eps_scale;
    }
    // ---- select + exactness flags, then the list of the failed queries
    fa.cand = h->cand.p; fa.cap = cap; fa.mode = 0; fa.fail_flags = h->fail_flags.p;
    fa.need_min = k < h->N ? k : h->N; fa.thr_out = nullptr;
    RCCHK(launch_finalize(fa, (unsigned)nq, s.st));
    hipLaunchKernelGGL(fill_int_kernel, dim3(1), dim3(64), 0, s.st, h->n_fail.p, 1, 0);
    launch_collect_fail(h->fail_flags.p, nq, h->fail_list.p, h->n_fail.p, s.st);
    RCCHK(check_launch("finalize"));
  }
  // ---- check
  HIPCHK(hipMemcpyAsync(h->h_nfail, h->n_fail.p, sizeof(int), hipMemcpyDeviceToHost, s.st));
  int nf = 0;
  RCCHK(read_fail_count(s, &nf));
  return nf > 0 ? flat_redo(s, nf) : RIHIP_OK;
}

// scratch every path uses, then the path
int search_pass(const Search& s) {
  IpIndex* h = s.h;
  const int64_t nq = s.nq;
  ++h->search_stats[ST_PASSES];
  RCCHK(h->count.reserve(nq * CSTRIDE));
  RCCHK(h->fail_flags.reserve(nq));
  RCCHK(h->fail_list.reserve(nq));
  RCCHK(h->thr.reserve(nq));
  RCCHK(h->n_fail.reserve(1));
  if (!h->h_nfail) HIPCHK(hipHostMalloc((void**)&h->h_nfail, sizeof(int)));
  if (s.filt()) RCCHK(h->n_pass.reserve(nq));
  if (s.pred) {
    RCCHK(h->fpred.reserve(64 * 3));
    h->filt_stats[0] += nq;
  }
  if (s.xmask) h->excl_stats[0] += nq;
  if (h->ivf) {
    IvfGeom g;
    RCCHK(ivf_geom(h, &g));
    // small populations or small batches (single requests): the unfiltered pass
    if (g.cap_full <= 16384 || (double)s.k * 4.0 > (double)g.cap_full / IVF_SS || nq * g.cap_df <= (int64_t)(1 << 23)) {
      ++h->search_stats[ST_IVF_UNFILTERED];   // (as a first choice: the re-dos count under ST_REDONE)
      return ivf_unfiltered(s, g, nullptr);
    }
    return ivf_thresholded(s, g);
  }
  if (h->N <= 4 * (int64_t)SAMPLE) return flat_dense(s);
  return flat_thresholded(s);
}

// the parts the two search entry points share: queries zero-padded to the kernel width (scratch of the handle) ...
int kernel_width_queries(IpIndex* h, const char* who, const float** Q, int64_t nq, hipStream_t st) {
  if (h->du != h->d) {
    RCCHK(h->qpad.reserve(nq * h->d));
    RCCHK(pad_rows(*Q, nq, h->du, h->d, h->qpad.p, st));
    *Q = h->qpad.p;
  }
  RIHIP_REQUIRE((reinterpret_cast<uintptr_t>(*Q) & 15) == 0, RIHIP_ERR_ARG, "%s: Q must be 16-byte aligned", who);
  return RIHIP_OK;
}
constexpr int64_t CH = 4096;  // queries per internal pass (bounds scratch)
// ... and the passes over them (pred = null: unfiltered)
int search_in_chunks(IpIndex* h, const float* Q, int64_t nq, int k, const uint32_t* pred, int pred_stride, float* out_scores,
                     int64_t* out_rows, hipStream_t st) {
  for (int64_t q0 = 0; q0 < nq; q0 += CH) {
    const int64_t n = (nq - q0 < CH) ? nq - q0 : CH;
    RCCHK(search_pass(Search{h, Q + q0 * h->d, n, k, out_scores + q0 * k, out_rows + q0 * k, st,
                              pred ? pred + q0 * pred_stride : nullptr, pred_stride}));
  }
  return RIHIP_OK;
}

}  // namespace

namespace rihip_index {
__global__ void pad_rows_kernel(const float* __restrict__ src, int64_t n, int du, int d, float* __restrict__ dst) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * d) return;
  const int64_t r = i / d;
  const int k = (int)(i % d);
  dst[i] = k < du ? src[r * du + k] : 0.f;
}
int pad_rows(const float* src, int64_t n, int du, int d, float* dst, hipStream_t st) {
  const int64_t tot = n * d;
  hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, src, n, du, d, dst);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
}  // namespace rihip_index

extern "C" int rihip_ip_index_create(int d, void** handle) {
  RIHIP_REQUIRE(handle, RIHIP_ERR_ARG, "ip_index_create: null handle");
  RIHIP_REQUIRE(d >= 1 && d <= 128, RIHIP_ERR_SHAPE, "ip_index_create: unsupported embed_dim=%d (1..128)", d);
  IpIndex* h = new IpIndex();
  h->du = d;
  h->d = d <= 32 ? 32 : (d <= 64 ? 64 : 128);   // the scan kernels are instantiated for these widths: rows are zero-padded
  *handle = h;
  return RIHIP_OK;
}

extern "C" int rihip_ip_index_destroy(void* handle) {
  IpIndex* h = (IpIndex*)handle;
  if (!h) return RIHIP_OK;
  free_index_arrays(h);
  h->n_pass.release(); h->fpred.release(); h->xmask.release();
  h->cand.release(); h->scand.release(); h->fcand.release(); h->count.release(); h->fail_flags.release();
  h->fail_list.release(); h->n_fail.release(); h->fcount.release(); h->thr.release(); h->thr2.release(); h->fQ.release();
  h->coarse.release(); h->probe_list.release(); h->list_q.release(); h->list_cnt.release(); h->list_qoff.release();
  h->list_cur.release(); h->work_off.release(); h->plan.release(); h->qnorm.release(); h->seg.release(); h->seg_cnt.release();
  h->qpad.release();
  if (h->h_nfail) hipHostFree(h->h_nfail);
  if (h->ev_fail) (void)hipEventDestroy(h->ev_fail);
  delete h;
  return RIHIP_OK;
}

// Replace the index content with N vectors (host or device pointer; copied, caller keeps ownership).
extern "C" int rihip_ip_index_set_vectors(void* handle, const float* X, int64_t N, int x_on_device, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && X && N > 0 && N < (1ll << 31), RIHIP_ERR_ARG, "ip_index_set_vectors: bad arguments");
  free_index_arrays(h);
  HIPCHK(hipMalloc((void**)&h->X, sizeof(float) * (size_t)N * h->d));
  if (h->du == h->d) {
    HIPCHK(hipMemcpyAsync(h->X, X, sizeof(float) * (size_t)N * h->d, x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                          (hipStream_t)stream));
  } else {   // zero-pad the rows to the kernel width
    const float* src = X;
    float* tmp = nullptr;
    if (!x_on_device) {
      HIPCHK(hipMalloc((void**)&tmp, sizeof(float) * (size_t)N * h->du));
      if (hipMemcpyAsync(tmp, X, sizeof(float) * (size_t)N * h->du, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) {
        hipFree(tmp); rihip_set_error("ip_index_set_vectors: upload failed"); return RIHIP_ERR_HIP;
      }
      src = tmp;
    }
    const int rc = pad_rows(src, N, h->du, h->d, h->X, (hipStream_t)stream);
    (void)hipStreamSynchronize((hipStream_t)stream);
    if (tmp) hipFree(tmp);
    if (rc) return rc;
  }
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  h->N = N;
  RCCHK(prepare_flat(h, (hipStream_t)stream));
  return RIHIP_OK;
}

extern "C" int rihip_ip_index_set_two_precision(void* handle, int enable) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h, RIHIP_ERR_ARG, "ip_index_set_two_precision: null handle");
  h->two_precision = enable ? 1 : 0;
  rihip_bump_generation();
  return RIHIP_OK;
}

extern "C" int64_t rihip_ip_index_ntotal(void* handle) { return handle ? ((IpIndex*)handle)->N : 0; }
extern "C" int rihip_ip_index_is_ivf(void* handle) { return handle ? (((IpIndex*)handle)->ivf ? 1 : 0) : 0; }
extern "C" int rihip_ip_index_max_k(void) { return K_MAX; }

extern "C" int rihip_ip_index_set_nprobe(void* handle, int nprobe) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && nprobe >= 1, RIHIP_ERR_ARG, "ip_index_set_nprobe: bad arguments");
  if (h->nprobe != nprobe) rihip_bump_generation();
  h->nprobe = nprobe;
  return RIHIP_OK;
}

// queries: device [nq,d]; outputs: device scores f32[nq,k] (desc, -inf pad), rows i64[nq,k] (-1 pad)
extern "C" int rihip_ip_index_search(void* handle, const float* Q, int64_t nq, int k, float* out_scores,
                                     int64_t* out_rows, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && h->X && h->N > 0, RIHIP_ERR_STATE, "ip_index_search: index is empty");
  RIHIP_REQUIRE(Q && out_scores && out_rows && nq > 0, RIHIP_ERR_ARG, "ip_index_search: bad arguments");
  RIHIP_REQUIRE(k >= 1 && k <= K_MAX, RIHIP_ERR_ARG, "ip_index_search: k=%d outside [1,%d]", k, K_MAX);
  hipStream_t st = (hipStream_t)stream;
  RCCHK(kernel_width_queries(h, "ip_index_search", &Q, nq, st));
  h->pending.active = false;
  h->defer_ok = nq <= CH;
  return search_in_chunks(h, Q, nq, k, nullptr, 0, out_scores, out_rows, st);
}

// ---- filtered search: per-query tag predicates inside the scan ----------------------------------------------------
extern "C" int rihip_ip_index_set_tags(void* handle, const uint32_t* tags_by_row_dev, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && h->X && h->N > 0, RIHIP_ERR_STATE, "ip_index_set_tags: index is empty");
  RIHIP_REQUIRE(!h->pending.active, RIHIP_ERR_STATE, "ip_index_set_tags: a deferred search is pending");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(st));   // (searches in flight still read the old copy)
  drop_tags(h);
  if (!tags_by_row_dev) return RIHIP_OK;
  const int64_t n = h->ivf ? h->Np : h->N;
  uint32_t* t = nullptr;
  HIPCHK(hipMalloc((void**)&t, sizeof(uint32_t) * (size_t)n));
  hipError_t e;
  if (h->ivf) {
    launch_tags_to_scan_order(tags_by_row_dev, h->row_ids, n, t, st);
    e = hipGetLastError();
  } else {
    e = hipMemcpyAsync(t, tags_by_row_dev, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);   // the caller's array may go away after the call
  if (e != hipSuccess) { hipFree(t); rihip_set_error("ip_index_set_tags: %s", hipGetErrorString(e)); return RIHIP_ERR_HIP; }
  h->tags = t;
  return RIHIP_OK;
}

extern "C" int rihip_ip_index_has_tags(void* handle) { return handle && ((IpIndex*)handle)->tags ? 1 : 0; }

extern "C" int rihip_ip_index_filtered_stats(void* handle, int64_t* out) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "ip_index_filtered_stats: bad arguments");
  out[0] = h->filt_stats[0]; out[1] = h->filt_stats[1];
  return RIHIP_OK;
}

// What the driver did, cumulative since the handle was made: host counters only (IpIndex::search_stats).
extern "C" int rihip_ip_index_search_stats(void* handle, int64_t* out) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "ip_index_search_stats: bad arguments");
  for (int i = 0; i < ST_COUNT; ++i) out[i] = h->search_stats[i];
  return RIHIP_OK;
}

extern "C" int rihip_ip_index_search_filtered(void* handle, const float* Q, int64_t nq, int k, const uint32_t* pred_dev,
                                              int64_t pred_stride, float* out_scores, int64_t* out_rows, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && h->X && h->N > 0, RIHIP_ERR_STATE, "ip_index_search_filtered: index is empty");
  RIHIP_REQUIRE(h->tags, RIHIP_ERR_STATE, "ip_index_search_filtered: the index has no tags (rihip_ip_index_set_tags)");
  RIHIP_REQUIRE(!h->pending.active, RIHIP_ERR_STATE, "ip_index_search_filtered: a deferred search is pending (rihip_ip_index_search_finish)");
  RIHIP_REQUIRE(Q && pred_dev && out_scores && out_rows && nq > 0, RIHIP_ERR_ARG, "ip_index_search_filtered: bad arguments");
  RIHIP_REQUIRE(pred_stride == 0 || pred_stride == 3, RIHIP_ERR_ARG, "ip_index_search_filtered: pred_stride=%lld (0 or 3)", (long long)pred_stride);
  RIHIP_REQUIRE(k >= 1 && k <= K_MAX, RIHIP_ERR_ARG, "ip_index_search_filtered: k=%d outside [1,%d]", k, K_MAX);
  hipStream_t st = (hipStream_t)stream;
  RCCHK(kernel_width_queries(h, "ip_index_search_filtered", &Q, nq, st));
  return search_in_chunks(h, Q, nq, k, pred_dev, (int)pred_stride, out_scores, out_rows, st);
}

// ---- seen-item exclusion inside the scan --------------------------------------------------------------------------
namespace {
int check_seen_args(const char* who, int64_t nq, const int64_t* seen_offsets, int64_t n_seen_rows, const int32_t* seen_items,
                    const int32_t* row_of, int64_t n_ids) {
  RIHIP_REQUIRE(nq > 0 && seen_offsets && seen_items && n_seen_rows >= 0, RIHIP_ERR_ARG, "%s: bad seen lists", who);
  RIHIP_REQUIRE(row_of && n_ids > 0, RIHIP_ERR_ARG, "%s: no row_of table", who);
  return RIHIP_OK;
}
// the handle's inverse of row_ids, made on first use (flat: positions are rows, none needed)
int ensure_inv_pos(IpIndex* h, hipStream_t st) {
  if (!h->ivf || h->inv_pos) return RIHIP_OK;
  int* ip = nullptr;
  HIPCHK(hipMalloc((void**)&ip, sizeof(int) * (size_t)h->N));
  launch_inv_pos(h->row_ids, h->Np, ip, st);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    hipFree(ip); rihip_set_error("ip_index: building the row -> position table failed"); return RIHIP_ERR_HIP;
  }
  h->inv_pos = ip;
  return RIHIP_OK;
}
int64_t mask_words_per_query(const IpIndex* h) { return ((h->ivf ? h->Np : h->N) + 31) / 32; }
}  // namespace

extern "C" int rihip_ip_index_set_exclusion_budget(void* handle, int64_t bytes) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && bytes >= 0, RIHIP_ERR_ARG, "ip_index_set_exclusion_budget: bad arguments");
  h->xmask_budget = bytes > 0 ? bytes : XMASK_BUDGET;
  return RIHIP_OK;
}

extern "C" int rihip_ip_index_exclusion_stats(void* handle, int64_t* out) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "ip_index_exclusion_stats: bad arguments");
  for (int i = 0; i < 3; ++i) out[i] = h->excl_stats[i];
  return RIHIP_OK;
}

extern "C" int rihip_ip_index_exclusion_mask_words(void* handle, int64_t* words_per_query) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && h->X && h->N > 0 && words_per_query, RIHIP_ERR_STATE, "ip_index_exclusion_mask_words: index is empty");
  *words_per_query = mask_words_per_query(h);
  return RIHIP_OK;
}

extern "C" int rihip_ip_index_exclusion_mask(void* handle, int64_t nq, const int64_t* user_ids, const int64_t* seen_offsets,
                                             int64_t n_seen_rows, const int32_t* seen_items, const int32_t* row_of, int64_t n_ids,
                                             uint32_t* out_mask, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && h->X && h->N > 0, RIHIP_ERR_STATE, "ip_index_exclusion_mask: index is empty");
  RCCHK(check_seen_args("ip_index_exclusion_mask", nq, seen_offsets, n_seen_rows, seen_items, row_of, n_ids));
  RIHIP_REQUIRE(out_mask, RIHIP_ERR_ARG, "ip_index_exclusion_mask: null output");
  hipStream_t st = (hipStream_t)stream;
  RCCHK(ensure_inv_pos(h, st));
  const int64_t W = mask_words_per_query(h);
  HIPCHK(hipMemsetAsync(out_mask, 0, sizeof(uint32_t) * (size_t)(nq * W), st));
  const SeenArgs sn{user_ids, seen_offsets, n_seen_rows, seen_items, row_of, n_ids};
  for (int64_t q0 = 0; q0 < nq; q0 += CH) {
    const int64_t n = (nq - q0 < CH) ? nq - q0 : CH;
    launch_xmask(sn, q0, n, h->inv_pos, h->N, out_mask + q0 * W, W, 1, st);
  }
  return check_launch("exclusion mask");
}

extern "C" int rihip_ip_index_exclusion_scratch_nonzero(void* handle, int64_t* n_words, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && n_words, RIHIP_ERR_ARG, "ip_index_exclusion_scratch_nonzero: bad arguments");
  *n_words = 0;
  if (!h->xmask.p) return RIHIP_OK;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* cnt = nullptr;
  HIPCHK(hipMalloc((void**)&cnt, sizeof(unsigned long long)));
  unsigned long long host = 0;
  hipError_t e = hipMemsetAsync(cnt, 0, sizeof(unsigned long long), st);
  if (e == hipSuccess) { launch_count_nonzero(h->xmask.p, h->xmask.n, cnt, st); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipMemcpyAsync(&host, cnt, sizeof(host), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipFree(cnt);
  HIPCHK(e);
  *n_words = (int64_t)host;
  return RIHIP_OK;
}

extern "C" int rihip_ip_index_search_excluding(void* handle, const float* Q, int64_t nq, int k, const int64_t* user_ids,
                                               const int64_t* seen_offsets, int64_t n_seen_rows, const int32_t* seen_items,
                                               const int32_t* row_of, int64_t n_ids, const uint32_t* pred_dev, int64_t pred_stride,
                                               float* out_scores, int64_t* out_rows, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && h->X && h->N > 0, RIHIP_ERR_STATE, "ip_index_search_excluding: index is empty");
  RIHIP_REQUIRE(!pred_dev || h->tags, RIHIP_ERR_STATE, "ip_index_search_excluding: the index has no tags (rihip_ip_index_set_tags)");
  RIHIP_REQUIRE(!h->pending.active, RIHIP_ERR_STATE, "ip_index_search_excluding: a deferred search is pending (rihip_ip_index_search_finish)");
  RIHIP_REQUIRE(Q && out_scores && out_rows && nq > 0, RIHIP_ERR_ARG, "ip_index_search_excluding: bad arguments");
  RCCHK(check_seen_args("ip_index_search_excluding", nq, seen_offsets, n_seen_rows, seen_items, row_of, n_ids));
  RIHIP_REQUIRE(pred_stride == 0 || pred_stride == 3, RIHIP_ERR_ARG, "ip_index_search_excluding: pred_stride=%lld (0 or 3)", (long long)pred_stride);
  RIHIP_REQUIRE(k >= 1 && k <= K_MAX, RIHIP_ERR_ARG, "ip_index_search_excluding: k=%d outside [1,%d]", k, K_MAX);
  hipStream_t st = (hipStream_t)stream;
  RCCHK(kernel_width_queries(h, "ip_index_search_excluding", &Q, nq, st));
  RCCHK(ensure_inv_pos(h, st));
  const int64_t W = mask_words_per_query(h);
  // queries per mask chunk: what the budget holds (whole 128-query blocks where it holds one), at most an internal pass
  int64_t per = h->xmask_budget / (int64_t)(sizeof(uint32_t) * W);
  if (per > CH) per = CH;
  if (per >= QB) per = per / QB * QB;
  if (per < 1) per = 1;
  if (per > nq) per = nq;
  const bool grown = h->xmask.n < per * W;
  RCCHK(h->xmask.reserve(per * W));
  if (grown || h->xmask_dirty) HIPCHK(hipMemsetAsync(h->xmask.p, 0, sizeof(uint32_t) * (size_t)h->xmask.n, st));
  const SeenArgs sn{user_ids, seen_offsets, n_seen_rows, seen_items, row_of, n_ids};
  h->xmask_dirty = true;   // (until the last chunk's clear is enqueued: an error return in between leaves bits behind)
  for (int64_t q0 = 0; q0 < nq; q0 += per) {
    const int64_t n = (nq - q0 < per) ? nq - q0 : per;
    ++h->excl_stats[2];
    launch_xmask(sn, q0, n, h->inv_pos, h->N, h->xmask.p, W, 1, st);
    RCCHK(check_launch("exclusion mask"));
    Search s{h, Q + q0 * h->d, n, k, out_scores + q0 * k, out_rows + q0 * k, st,
             pred_dev ? pred_dev + q0 * pred_stride : nullptr, (int)pred_stride};
    s.xmask = h->xmask.p; s.xW = W;
    RCCHK(search_pass(s));
    launch_xmask(sn, q0, n, h->inv_pos, h->N, h->xmask.p, W, 0, st);
    RCCHK(check_launch("exclusion mask clear"));
  }
  h->xmask_dirty = false;
  return RIHIP_OK;
}

// Deferred exactness check (serving chains): with enable = 1 a thresholded IVF search of <= 4 096 queries enqueues its
// work and returns WITHOUT the host synchronisation that reads the count of queries whose candidate threshold was too
// aggressive; the caller enqueues whatever consumes the results, then calls rihip_ip_index_search_finish (one sync):
// n_redone > 0 means that many queries were re-done exactly into the same output rows AFTER the consumers ran -- run them
// again.  finish must be called before the next search of the handle.  Other search paths are unaffected (n_redone = 0).
extern "C" int rihip_ip_index_set_deferred_check(void* handle, int enable) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h, RIHIP_ERR_ARG, "ip_index_set_deferred_check: null handle");
  h->defer_check = enable != 0;
  h->pending.active = false;   // (also drops a pending check: what a caller does after CAPTURING a chain, which ran nothing)
  return RIHIP_OK;
}
// 1 while a deferred search awaits its finish (what a hipGraph capture of a chain needs to know about itself)
extern "C" int rihip_ip_index_search_pending(void* handle) { return handle && ((IpIndex*)handle)->pending.active ? 1 : 0; }
// The failure count the LAST enqueued deferred search wrote (after a synchronisation of `stream`): for replays of a
// captured chain, which run no host code -- n > 0: run the chain again eagerly, not deferred.
extern "C" int rihip_ip_index_last_fail_count(void* handle, int* n, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && n && h->h_nfail, RIHIP_ERR_ARG, "ip_index_last_fail_count: no deferred search has run");
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *n = *h->h_nfail;
  return RIHIP_OK;
}
extern "C" int rihip_ip_index_search_finish(void* handle, int* n_redone, void* stream) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h && n_redone, RIHIP_ERR_ARG, "ip_index_search_finish: bad arguments");
  *n_redone = 0;
  if (!h->pending.active) return RIHIP_OK;
  hipStream_t st = (hipStream_t)stream;
  h->pending.active = false;
  if (h->ev_recorded) HIPCHK(hipEventSynchronize(h->ev_fail));
  else HIPCHK(hipStreamSynchronize(st));
  const int nf = *h->h_nfail;
  if (nf <= 0) return RIHIP_OK;
  // the exact re-do only (the scratch every search reserves is in place: this search's own pass reserved it)
  IvfGeom g;
  RCCHK(ivf_geom(h, &g));
  RCCHK(ivf_redo(Search{h, h->pending.Q, h->pending.nq, h->pending.k, h->pending.out_s, h->pending.out_r, st, nullptr, 0}, g, nf));
  HIPCHK(hipStreamSynchronize(st));
  *n_redone = nf;
  return RIHIP_OK;
}

extern "C" int rihip_ip_index_set_id_map(void* handle, const int64_t* item_ids_dev) {
  IpIndex* h = (IpIndex*)handle;
  RIHIP_REQUIRE(h, RIHIP_ERR_ARG, "ip_index_set_id_map: null handle");
  if (h->id_map != item_ids_dev) rihip_bump_generation();
  h->id_map = item_ids_dev;   // not owned: must stay valid (>= ntotal entries) while searches run; NULL switches it off
  return RIHIP_OK;
}

extern "C" int rihip_map_rows_to_ids(int64_t* rows, int64_t n, const int64_t* item_ids, void* stream) {
  RIHIP_REQUIRE(rows && item_ids && n >= 0, RIHIP_ERR_ARG, "map_rows_to_ids: bad arguments");
  if (n == 0) return RIHIP_OK;
  hipLaunchKernelGGL(map_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, n, item_ids);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
