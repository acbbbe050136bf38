// 8-bit scalar-quantised inner-product index (flat and IVF): the search driver and the plain, filtered and excluding
// search of the C ABI.  (The handle and its build: sq8_build.hip; the scan kernel: sq8_scan.hip; the refined search:
// sq8_refine.hip; state files: sq8_state.hip; updates: sq8_update.hip; product-quantised storage: pq.hip.)
//
// The index stores one int8 code per dimension (sq8_build.hip).  The query side keeps 16 bits: w_j = q_j s_j,
// t = max|w| / 32512, n_j = rint(w_j / t) split into two int8 limbs n = 256 hi + lo.  The scan scores
// S_i = sum_j n_j c_ij on the i8 MFMA (two chains into two i32 accumulators, S = 256 S_hi + S_lo,
// |S| <= 32512 * 127 * 128 < 2^31): integers, so ranking, ties and the completeness check of the thresholded pass are
// exact.  The reported score is (float)(b + t S) with b = sum_j q_j m_j in f64.
//
// The search reuses what does not depend on the corpus representation: the coarse quantizer, probe selection, work plan
// and scatter of ivf_search.hip and finalize_kernel of select.hip.  Candidate keys are make_key's with the integer score
// in the high word ((uint32)S ^ 0x80000000: unsigned order = signed order; never 0, the empty-slot key).  finalize emits a
// key's high word through ord2f, a bijection of the 32 bits, so sq8_decode_kernel recovers S from the float it wrote.
//
// A handle may hold product-quantised storage instead of the int8 matrix.  sq8_scan picks the source; the PQ
// instantiations of the scan gather the operand bytes from the codebooks in LDS, and everything else in this file is the
// same code for both.  A residual PQ handle adds one kernel: T of every (query, probed list) pair, filled in sq8_prepare
// once the probes are known and added to the gathered dot product by the residual instantiations of the scan.
#pragma clang fp contract(off)   // the query transform and the decode are specified operation by operation: no fused multiply-add
#include "common.h"
#include "recommendit_hip.h"

#include <algorithm>
#include <math.h>
#include <string.h>
#include <vector>

#include "search_kernels.h"
#include "search_keys.h"
#include "sq8_index.h"
#include "sq8_scan.h"

using namespace rihip_index;

namespace {

constexpr float SQ8_QMAX = 32512.0f;            // largest |n_j|: 127 * 256, so both limbs fit int8
constexpr int64_t SQ8_DENSE_BUDGET = 1ll << 26;  // dense candidate slots (8 B each) of one query chunk: 512 MiB
constexpr int64_t SQ8_DENSE_AUTO = 1ll << 23;    // auto: dense while the batch's slots stay under 64 MiB (the f32 index's rule;
                                                 // at 256 queries x IVF 100/10 of 1 M rows dense measured 0.46 ms, thresholded 0.23)
constexpr int SQ8_TARGET = 16 * RIHIP_NCU;      // wave work items aimed at (as the f32 list-major scan)
constexpr int SQ8_SS = 16;                      // threshold sample: every 16th probed tile
constexpr int64_t SQ8_CH = 4096;                // queries per internal pass at most

// ------------------------------------------------ query transform ----------------------------------------------------
// one workgroup of 128 threads per query: limb rows (zero beyond du), t, b, and optionally n as int16 [nq, du]
__global__ __launch_bounds__(128) void sq8_query_kernel(const float* __restrict__ Q, int64_t nq, int du, int dpad,
                                                        const float* __restrict__ centre, const float* __restrict__ scale,
                                                        int8_t* qhi, int8_t* qlo, float* qt, double* qb, int16_t* n16) {
  __shared__ float smax[2];
  __shared__ double sprod[128];
  const int64_t q = blockIdx.x;
  const int j = threadIdx.x;
  float w = 0.f;
  double pm = 0.0;
  if (j < du) {
    const float x = Q[q * du + j];
    w = x * scale[j];
    pm = (double)x * (double)centre[j];   // exact in f64
  }
  sprod[j] = pm;
  float a = fabsf(w);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
  if ((j & 63) == 0) smax[j >> 6] = a;
  __syncthreads();
  const float A = fmaxf(smax[0], smax[1]);
  const float t = A / SQ8_QMAX;
  int n = 0;
  if (A != 0.f) {
    float v = rintf(w / t);
    v = fminf(fmaxf(v, -SQ8_QMAX), SQ8_QMAX);
    n = (int)v;
  }
  const int hi = (n + 128) >> 8, lo = n - 256 * hi;
  if (j < dpad) { qhi[q * dpad + j] = (int8_t)hi; qlo[q * dpad + j] = (int8_t)lo; }
  if (n16 && j < du) n16[q * du + j] = (int16_t)n;
  if (j == 0) {
    double b = 0.0;
    for (int i = 0; i < du; ++i) b += sprod[i];   // ascending j
    qb[q] = b;
    qt[q] = (A != 0.f) ? t : 0.f;
  }
}

// ------------------------------------------------ decode -------------------------------------------------------------
// finalize wrote, per result, the key's high word as ord2f(word) and the original row (-1 = padding): recover S, report
// (float)(b + t S), the optional i32 score and the row or mapped id
__global__ void sq8_decode_kernel(float* scores, int64_t* rows, int* iscores, int64_t nq, int k, const float* __restrict__ qt,
                                  const double* __restrict__ qb, const int64_t* __restrict__ id_map) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq * k) return;
  const int64_t q = i / k;
  const int64_t row = rows[i];
  if (row < 0) {
    scores[i] = -INFINITY; rows[i] = -1;
    if (iscores) iscores[i] = (int)0x80000000;
    return;
  }
  const int S = sq8_score_of_word(f2ord(scores[i]));
  scores[i] = (float)(qb[q] + (double)qt[q] * (double)S);
  if (iscores) iscores[i] = S;
  if (id_map) rows[i] = id_map[row];
}

__global__ void sq8_gather_kernel(const int8_t* __restrict__ hi, const int8_t* __restrict__ lo, const float* __restrict__ Qf,
                                  const int* __restrict__ idx, int n, int dpad, int dk, int8_t* ohi, int8_t* olo, float* oQ) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)n * dpad) return;
  const int64_t r = i / dpad;
  const int j = (int)(i % dpad);
  const size_t src = (size_t)idx[r];
  ohi[i] = hi[src * dpad + j]; olo[i] = lo[src * dpad + j];
  if (j < dk) oQ[r * dk + j] = Qf[src * dk + j];
}

// Residual PQ: T[pair] = sum_j n_j K_l[j] of every (query, probed list) pair, l = probe_list[pair], pair = q * nprobe +
// probe rank (what list_q holds and the scan reads).  dpad / 16 lanes per pair, 16 columns each: eight packed int8 dot
// products on the limbs (v_dot4_i32_i8), T = 256 <hi, K> + <lo, K>, |T| <= 32512 * 127 * 128 < 2^30: exact in i32.
__global__ __launch_bounds__(256) void sq8_pair_offset_kernel(const int8_t* __restrict__ qhi, const int8_t* __restrict__ qlo,
                                                              const int* __restrict__ probe_list, const int8_t* __restrict__ K,
                                                              int64_t n_pairs, int nprobe, int dpad, int* pair_t) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const int lpp = dpad / 16;   // 4 or 8 lanes per pair
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t pair = i / lpp;
  const int part = (int)(i % lpp);
  int sh = 0, sl = 0;
  int c = -1;
  if (pair < n_pairs) c = probe_list[pair];
  if (c >= 0) {
    const int64_t q = pair / nprobe;
    const i32x4 vh = *reinterpret_cast<const i32x4*>(qhi + (size_t)q * dpad + 16 * part);
    const i32x4 vl = *reinterpret_cast<const i32x4*>(qlo + (size_t)q * dpad + 16 * part);
    const i32x4 vk = *reinterpret_cast<const i32x4*>(K + (size_t)c * dpad + 16 * part);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      sh = __builtin_amdgcn_sdot4(vh[u], vk[u], sh, false);
      sl = __builtin_amdgcn_sdot4(vl[u], vk[u], sl, false);
    }
  }
  int t = sh * 256 + sl;
  for (int o = lpp >> 1; o > 0; o >>= 1) t += __shfl_xor(t, o, 64);   // (the lanes of a pair are aligned: 256 % lpp == 0)
  if (part == 0 && pair < n_pairs) pair_t[pair] = t;
}

// ------------------------------------------------ search driver ------------------------------------------------------
// one internal pass: the queries [0, nq) of the pointers below
struct Sq8Search {
  Sq8Index* h;
  const float* Qf;      // [nq, dk] f32 (coarse quantizer)
  const int8_t* qhi;    // [nq, dpad]
  const int8_t* qlo;
  int64_t nq;
  int k;
  float* out_s; int64_t* out_r;   // [nq, k]: finalize's raw output, decoded by the caller
  hipStream_t st;
  const uint32_t* pred;   // filtered search: these queries' predicates, query q's at pred[q * pred_stride]; else null
  int pred_stride;
  // seen-item exclusion inside the scan: these queries' mask rows (row q, or xrow[q] in the re-do), xW words each; else null
  const uint32_t* xmask = nullptr;
  int64_t xW = 0;
  const int* xrow = nullptr;
};

struct Sq8Geom {
  int nlist, nprobe;
  int64_t cap_full, max_tiles, cap_lf, cap_df;
};
Sq8Geom sq8_geom(const Sq8Index* h) {
  Sq8Geom g;
  std::vector<int64_t> ll = h->list_len;
  std::sort(ll.begin(), ll.end(), [](int64_t x, int64_t y) { return x > y; });
  g.nlist = h->nlist;
  g.nprobe = h->nprobe < h->nlist ? h->nprobe : h->nlist;
  g.cap_full = 0;
  for (int i = 0; i < g.nprobe; ++i) g.cap_full += ll[i];
  if (g.cap_full < 1) g.cap_full = 1;
  g.max_tiles = ll.empty() ? 0 : (ll[0] + TR - 1) / TR * (TR / TRS);
  g.cap_lf = std::max<int64_t>(g.max_tiles * TRS, TRS);
  g.cap_df = g.cap_lf * g.nprobe;
  return g;
}

int sq8_prepare(const Sq8Search& s, const Sq8Geom& g, int first_tile_step, uint64_t* zero_buf, int64_t zero_n) {
  Sq8Index* h = s.h;
  const int64_t n = s.nq;
  RCCHK(h->coarse.reserve(n * g.nlist));
  RCCHK(h->probe_list.reserve(n * g.nprobe));
  RCCHK(h->list_q.reserve(n * g.nprobe));
  RCCHK(h->list_cnt.reserve(g.nlist)); RCCHK(h->list_qoff.reserve(g.nlist + 1)); RCCHK(h->list_cur.reserve(g.nlist));
  RCCHK(h->work_off.reserve(g.nlist + 1)); RCCHK(h->plan.reserve(2));
  if (zero_buf) HIPCHK(hipMemsetAsync(zero_buf, 0, sizeof(uint64_t) * (size_t)zero_n, s.st));
  HIPCHK(hipMemsetAsync(h->list_cnt.p, 0, sizeof(int) * g.nlist, s.st));
  RCCHK(launch_ivf_coarse(h->dk, s.Qf, n, h->C, g.nlist, h->coarse.p, s.st));
  launch_ivf_select(h->coarse.p, n, g.nlist, g.nprobe, h->probe_list.p, h->list_cnt.p, s.st);
  launch_ivf_plan(h->list_cnt.p, h->list_poff, g.nlist, first_tile_step, SQ8_TARGET, h->list_qoff.p, h->list_cur.p, h->work_off.p,
                  h->plan.p, h->count.p, n * CSTRIDE, s.st);
  launch_ivf_scatter(h->probe_list.p, n * g.nprobe, g.nprobe, h->list_cur.p, h->list_q.p, s.st);
  if (h->pq_residual) {   // T of this pass's pairs (the re-do's renumbered queries come through here with their own limbs)
    const int64_t n_pairs = n * g.nprobe, nthr = n_pairs * (h->dpad / 16);
    RCCHK(h->pair_t.reserve(n_pairs));
    hipLaunchKernelGGL(sq8_pair_offset_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s.st, s.qhi, s.qlo, h->probe_list.p,
                       h->pq_list_codes, n_pairs, g.nprobe, h->dpad, h->pair_t.p);
  }
  return check_launch("sq8 prepare");
}

int sq8_scan(const Sq8Search& s, const Sq8Geom& g, const float* thr, uint64_t* cand, int64_t cap, int tile_step,
             int64_t dense_cap, bool planned, int dense_ids) {
  Sq8Index* h = s.h;
  if (!planned)
    launch_ivf_plan(h->list_cnt.p, h->list_poff, g.nlist, tile_step, SQ8_TARGET, h->list_qoff.p, h->list_cur.p, h->work_off.p,
                    h->plan.p, h->count.p, s.nq * CSTRIDE, s.st);
  Sq8LmArgs x;
  memset(&x, 0, sizeof(x));
  // the source: the int8 matrix, or (a PQ handle) the entry numbers and the codebooks
  x.codes = h->pq_codes ? reinterpret_cast<const int8_t*>(h->pq_codes) : h->codes; x.pq_book = h->pq_book;
  x.qhi = s.qhi; x.qlo = s.qlo; x.thr = thr; x.cand = cand; x.cap = cap; x.count = h->count.p;
  x.row_ids = h->row_ids; x.list_poff = h->list_poff; x.list_len = h->list_len_dev; x.list_qoff = h->list_qoff.p;
  x.list_q = h->list_q.p; x.work_off = h->work_off.p; x.plan = h->plan.p; x.nlist = g.nlist; x.tile_step = tile_step;
  x.nprobe = g.nprobe; x.count_stride = CSTRIDE; x.dense_cap = dense_cap; x.dense_ids = dense_ids;
  x.tags = s.pred ? h->tags : nullptr; x.pred = s.pred; x.pred_stride = s.pred_stride;
  x.xmask = s.xmask; x.xW = s.xW; x.xrow = s.xrow;
  x.pair_t = h->pq_residual ? h->pair_t.p : nullptr;
  // n_work <= sum over (list, group) of (tiles/tpi + 1) <= target + #(list, query group) pairs
  const int64_t bound = (int64_t)SQ8_TARGET + g.nlist + (s.nq * g.nprobe + 31) / 32 + 4;
  const dim3 grid((unsigned)((bound + 3) / 4));
  const int fm = x.xmask ? (x.tags ? FM_TAGS_MASK : FM_MASK) : (x.tags ? FM_TAGS : FM_NONE);
  const char* what = fm == FM_TAGS_MASK ? "masked filtered sq8 scan" : fm == FM_MASK ? "masked sq8 scan" : fm == FM_TAGS ? "filtered sq8 scan" : "sq8 scan";
  sq8_launch_scan(h->dpad, fm, h->pq_codes ? h->pq_dsub : 0, h->pq_residual, grid, s.st, x);
  return check_launch(what);
}

// dense emission: every (query, probed list) pair owns a slot per row of the longest list, then the two-level select
int sq8_dense(const Sq8Search& s, const Sq8Geom& g, const int* out_slot) {
  Sq8Index* h = s.h;
  const int64_t n = s.nq;
  RCCHK(h->fcand.reserve(n * g.cap_df));
  RCCHK(sq8_prepare(s, g, 1, h->fcand.p, n * g.cap_df));
  RCCHK(sq8_scan(s, g, nullptr, h->fcand.p, g.cap_df, 1, g.cap_lf, true, 1));
  const int64_t np_ = n * g.nprobe;
  RCCHK(h->scand.reserve(np_ * s.k));
  FinArgs f1;
  memset(&f1, 0, sizeof(f1));
  f1.nq = np_; f1.k = s.k; f1.count = nullptr; f1.cand = h->fcand.p; f1.cap = g.cap_lf; f1.mode = 0; f1.out_keys = h->scand.p;
  RCCHK(launch_finalize(f1, (unsigned)np_, s.st));
  FinArgs f2;
  memset(&f2, 0, sizeof(f2));
  f2.nq = n; f2.k = s.k; f2.count = nullptr; f2.out_scores = s.out_s; f2.out_rows = s.out_r; f2.cand = h->scand.p;
  f2.cap = (int64_t)g.nprobe * s.k; f2.mode = 0; f2.out_slot = out_slot;
  return launch_finalize(f2, (unsigned)n, s.st);
}

// the `nf` failed queries of h->fail_list, dense, 64 at a time, into their own output rows; a filtered search's chunk
// carries its queries' own predicates (one shared by the batch is handed on as it is)
int sq8_redo(const Sq8Search& s, const Sq8Geom& g, int nf) {
  Sq8Index* h = s.h;
  const int FCH = 64;
  const bool own_pred = s.pred && s.pred_stride != 0;
  if (own_pred) RCCHK(h->fpred.reserve((int64_t)FCH * 3));
  RCCHK(h->fQ.reserve((int64_t)FCH * h->dk));
  RCCHK(h->fhi.reserve((int64_t)FCH * h->dpad));
  RCCHK(h->flo.reserve((int64_t)FCH * h->dpad));
  for (int f0 = 0; f0 < nf; f0 += FCH) {
    const int nfc = (nf - f0 < FCH) ? nf - f0 : FCH;
    hipLaunchKernelGGL(sq8_gather_kernel, dim3((unsigned)(((int64_t)nfc * h->dpad + 255) / 256)), dim3(256), 0, s.st, s.qhi, s.qlo,
                       s.Qf, h->fail_list.p + f0, nfc, h->dpad, h->dk, h->fhi.p, h->flo.p, h->fQ.p);
    Sq8Search r = s;
    r.Qf = h->fQ.p; r.qhi = h->fhi.p; r.qlo = h->flo.p; r.nq = nfc;
    if (own_pred) {
      launch_gather_pred(s.pred, h->fail_list.p + f0, nfc, h->fpred.p, s.st);
      r.pred = h->fpred.p;
    }
    if (s.xmask) r.xrow = h->fail_list.p + f0;   // (the fail list holds the queries' positions in `s`: their mask rows)
    RCCHK(sq8_dense(r, g, h->fail_list.p + f0));
  }
  return RIHIP_OK;
}

// Thresholded pass, built as the f32 index's: (A) every 16th tile of each probed list into dense slots, the rank-th best
// sampled score is the query's threshold; (B) all probed tiles, S >= threshold appended; select; a query whose list
// overflowed, or that holds fewer than k candidates under a real threshold, is re-done dense.  Integer scores: a query that
// passes holds every probed row with S >= threshold and at least k of them, so its top k is complete -- no epsilon.
// Filtered: "row" reads "passing row" throughout (a failing row is in neither the sample nor the survivors), so the same
// argument holds under any pass rate; a sample with fewer than rank passing rows gives no threshold.
int sq8_thresholded(const Sq8Search& s, const Sq8Geom& g) {
  Sq8Index* h = s.h;
  const int64_t nq = s.nq;
  const int k = s.k;
  const double m = (double)k / SQ8_SS;
  const int rank = (int)ceil(m + 4.0 * sqrt(m) + 4.0);
  int64_t cap = 4096;
  while ((double)cap < 2.5 * rank * SQ8_SS) cap <<= 1;
  if (cap > g.cap_full) cap = g.cap_full;
  const int64_t cap_l = std::max<int64_t>((g.max_tiles + SQ8_SS - 1) / SQ8_SS * TRS, TRS);
  const int64_t cap_s = cap_l * g.nprobe;
  RCCHK(h->scand.reserve(nq * cap_s));
  RCCHK(h->cand.reserve(nq * cap));
  RCCHK(sq8_prepare(s, g, SQ8_SS, h->scand.p, nq * cap_s));
  RCCHK(sq8_scan(s, g, nullptr, h->scand.p, cap_s, SQ8_SS, cap_l, true, 0));
  FinArgs fa;
  memset(&fa, 0, sizeof(fa));
  fa.nq = nq; fa.k = k; fa.out_scores = s.out_s; fa.out_rows = s.out_r;
  fa.cand = h->scand.p; fa.cap = cap_s; fa.mode = 1; fa.rank = rank; fa.thr_out = h->thr.p; fa.count = nullptr;
  fa.zero_me = h->n_fail.p;
  RCCHK(launch_finalize(fa, (unsigned)nq, s.st));
  RCCHK(sq8_scan(s, g, h->thr.p, h->cand.p, cap, 1, 0, false, 0));
  fa.cand = h->cand.p; fa.cap = cap; fa.mode = 0; fa.thr_out = nullptr; fa.fail_flags = h->fail_flags.p;
  fa.count = h->count.p; fa.zero_me = nullptr; fa.fail_list = h->fail_list.p; fa.n_fail = h->n_fail.p;
  fa.ivf_thr = h->thr.p; fa.count_stride = CSTRIDE;
  RCCHK(launch_finalize(fa, (unsigned)nq, s.st));
  HIPCHK(hipMemcpyAsync(h->h_nfail, h->n_fail.p, sizeof(int), hipMemcpyDeviceToHost, s.st));
  HIPCHK(hipStreamSynchronize(s.st));
  const int nf = *h->h_nfail;
  h->stats[0] += nq; h->stats[1] += nf;
  if (s.pred) h->filt_stats[1] += nf;
  if (s.xmask) h->excl_stats[1] += nf;
  return nf > 0 ? sq8_redo(s, g, nf) : RIHIP_OK;
}

}  // namespace

namespace rihip_index {

int sq8_transform_queries(Sq8Index* h, const float* Q, int64_t nq, int16_t* n16, float* t_out, double* b_out, hipStream_t st) {
  RCCHK(h->qhi.reserve(nq * h->dpad));
  RCCHK(h->qlo.reserve(nq * h->dpad));
  if (!t_out) { RCCHK(h->qt.reserve(nq)); t_out = h->qt.p; }
  if (!b_out) { RCCHK(h->qb.reserve(nq)); b_out = h->qb.p; }
  hipLaunchKernelGGL(sq8_query_kernel, dim3((unsigned)nq), dim3(128), 0, st, Q, nq, h->du, h->dpad, h->centre, h->scale, h->qhi.p,
                     h->qlo.p, t_out, b_out, n16);
  return check_launch("sq8 query transform");
}

int sq8_ensure_inv_pos(Sq8Index* h, hipStream_t st) {
  if (h->inv_pos) return RIHIP_OK;
  int* ip = nullptr;
  HIPCHK(hipMalloc((void**)&ip, sizeof(int) * (size_t)h->N));
  launch_inv_pos(h->row_ids, h->Np, ip, st);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
    hipFree(ip); rihip_set_error("sq8_index: building the row -> position table failed"); return RIHIP_ERR_HIP;
  }
  h->inv_pos = ip;
  return RIHIP_OK;
}

int sq8_rows_at_dk(Sq8Index* h, const float*& X, int64_t n, const char* misaligned, hipStream_t st) {
  if (h->du != h->dk) {
    RCCHK(h->qpad.reserve(n * h->dk));
    RCCHK(pad_rows(X, n, h->du, h->dk, h->qpad.p, st));
    X = h->qpad.p;
  }
  RIHIP_REQUIRE((reinterpret_cast<uintptr_t>(X) & 15) == 0, RIHIP_ERR_ARG, "%s", misaligned);
  return RIHIP_OK;
}

// o.seen: the excluded search -- every internal chunk sets its mask bits, searches and clears the words it touched
int sq8_search(Sq8Index* h, const float* Q, int64_t nq, int k, int mode, float* out_s, int64_t* out_r, int* out_i, hipStream_t st,
               const Sq8SearchOpts& o) {
  RCCHK(sq8_transform_queries(h, Q, nq, nullptr, nullptr, nullptr, st));
  const float* Qf = Q;
  RCCHK(sq8_rows_at_dk(h, Qf, nq, "sq8_index_search: Q must be 16-byte aligned", st));
  const Sq8Geom g = sq8_geom(h);
  bool thresholded = mode == 2;
  if (mode == 0)
    thresholded = !(nq * g.cap_df <= SQ8_DENSE_AUTO || g.cap_full <= 16384 || (double)k * 4.0 > (double)g.cap_full / SQ8_SS);
  int64_t ch = SQ8_CH;
  if (!thresholded) ch = std::max<int64_t>(1, std::min<int64_t>(SQ8_CH, SQ8_DENSE_BUDGET / g.cap_df));
  const int64_t W = (h->Np + 31) / 32;
  if (o.seen) {   // queries per chunk: what the mask budget holds as well (whole 128-query blocks where it holds one)
    int64_t per = h->xmask_budget / (int64_t)(sizeof(uint32_t) * W);
    if (per >= QB) per = per / QB * QB;
    ch = std::max<int64_t>(1, std::min(ch, per));
    RCCHK(sq8_ensure_inv_pos(h, st));
    const int64_t want = std::min(nq, ch) * W;
    const bool grown = h->xmask.n < want;
    RCCHK(h->xmask.reserve(want));
    if (grown || h->xmask_dirty) HIPCHK(hipMemsetAsync(h->xmask.p, 0, sizeof(uint32_t) * (size_t)h->xmask.n, st));
    h->xmask_dirty = true;   // (until the last chunk's clear is enqueued: an error return in between leaves bits behind)
  }
  const int64_t nmax = std::min(nq, ch);
  RCCHK(h->count.reserve(nmax * CSTRIDE));
  RCCHK(h->fail_flags.reserve(nmax)); RCCHK(h->fail_list.reserve(nmax)); RCCHK(h->thr.reserve(nmax)); RCCHK(h->n_fail.reserve(1));
  if (!h->h_nfail) HIPCHK(hipHostMalloc((void**)&h->h_nfail, sizeof(int)));
  for (int64_t q0 = 0; q0 < nq; q0 += ch) {
    const int64_t n = std::min(ch, nq - q0);
    Sq8Search s{h, Qf + q0 * h->dk, h->qhi.p + q0 * h->dpad, h->qlo.p + q0 * h->dpad, n, k, out_s + q0 * k, out_r + q0 * k, st,
                o.pred ? o.pred + q0 * o.pred_stride : nullptr, o.pred_stride};
    if (o.seen) {
      ++h->excl_stats[2];
      launch_xmask(*o.seen, o.q_base + q0, n, h->inv_pos, h->N, h->xmask.p, W, 1, st);
      RCCHK(check_launch("sq8 exclusion mask"));
      s.xmask = h->xmask.p; s.xW = W;
    }
    RCCHK(thresholded ? sq8_thresholded(s, g) : sq8_dense(s, g, nullptr));
    if (o.seen) {
      launch_xmask(*o.seen, o.q_base + q0, n, h->inv_pos, h->N, h->xmask.p, W, 0, st);
      RCCHK(check_launch("sq8 exclusion mask clear"));
    }
  }
  if (o.seen) { h->xmask_dirty = false; h->excl_stats[0] += nq; }
  if (o.pred) h->filt_stats[0] += nq;
  const int64_t tot = nq * k;
  hipLaunchKernelGGL(sq8_decode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, out_s, out_r, out_i, nq, k, h->qt.p,
                     h->qb.p, o.map_ids ? h->id_map : nullptr);
  return check_launch("sq8 decode");
}

int sq8_check_search(const Sq8Index* h, const Sq8SearchCall& c) {
  const char* who = c.who;
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "%s: index is empty", who);
  RIHIP_REQUIRE(c.k_scan == 0 || h->vec, RIHIP_ERR_STATE, "%s: no vectors attached (rihip_sq8_refine_attach_vectors)", who);
  RIHIP_REQUIRE(!(c.filtered || c.pred) || h->tags, RIHIP_ERR_STATE, "%s: the index has no tags (rihip_sq8_filter_set_tags)", who);
  if (c.seen) {   // (its outputs have a message of their own)
    RIHIP_REQUIRE(c.Q && c.nq > 0, RIHIP_ERR_ARG, "%s: bad arguments", who);
    RIHIP_REQUIRE(c.seen->seen_offsets && c.seen->seen_items && c.seen->n_seen_rows >= 0, RIHIP_ERR_ARG, "%s: bad seen lists", who);
    RIHIP_REQUIRE(c.seen->row_of && c.seen->n_ids > 0, RIHIP_ERR_ARG, "%s: no row_of table", who);
  } else {
    RIHIP_REQUIRE(c.Q && (!c.filtered || c.pred) && c.outputs && c.nq > 0, RIHIP_ERR_ARG, "%s: bad arguments", who);
  }
  RIHIP_REQUIRE(c.pred_stride == 0 || c.pred_stride == 3, RIHIP_ERR_ARG, "%s: pred_stride=%lld (0 or 3)", who, (long long)c.pred_stride);
  RIHIP_REQUIRE(!c.seen || c.outputs, RIHIP_ERR_ARG, "%s: null output", who);
  if (c.k_scan)
    RIHIP_REQUIRE(c.k >= 1 && c.k <= c.k_scan && c.k_scan <= K_MAX, RIHIP_ERR_ARG, "%s: k=%d, k_scan=%d (1 <= k <= k_scan <= %d)", who,
                  c.k, c.k_scan, K_MAX);
  else
    RIHIP_REQUIRE(c.k >= 1 && c.k <= K_MAX, RIHIP_ERR_ARG, "%s: k=%d outside [1,%d]", who, c.k, K_MAX);
  RIHIP_REQUIRE(c.mode >= 0 && c.mode <= 2, RIHIP_ERR_ARG, "%s: mode=%d (0 auto, 1 dense, 2 thresholded)", who, c.mode);
  return RIHIP_OK;
}

}  // namespace rihip_index

// ------------------------------------------------ C ABI --------------------------------------------------------------
extern "C" int rihip_sq8_index_encode_queries(void* handle, const float* Q, int64_t nq, int16_t* out_n, float* out_t, double* out_b,
                                              void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && Q && out_n && out_t && out_b && nq > 0, RIHIP_ERR_ARG, "sq8_index_encode_queries: bad arguments");
  return sq8_transform_queries(h, Q, nq, out_n, out_t, out_b, (hipStream_t)stream);
}

extern "C" int rihip_sq8_index_search(void* handle, const float* Q, int64_t nq, int k, int mode, float* out_scores, int64_t* out_rows,
                                      int32_t* out_iscores, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RCCHK(sq8_check_search(h, {"sq8_index_search", Q, nq, k, 0, mode, out_scores && out_rows, false, nullptr, 0, nullptr}));
  return sq8_search(h, Q, nq, k, mode, out_scores, out_rows, out_iscores, (hipStream_t)stream, {});
}

// ---- filtered search: per-query tag predicates inside the int8 scan ---------------------------------------------------
extern "C" int rihip_sq8_filter_set_tags(void* handle, const uint32_t* tags_by_row_dev, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "sq8_filter_set_tags: index is empty");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(st));   // (searches in flight still read the old copy)
  sq8_drop_tags(h);
  if (!tags_by_row_dev) return RIHIP_OK;
  uint32_t* t = nullptr;
  HIPCHK(hipMalloc((void**)&t, sizeof(uint32_t) * (size_t)h->Np));
  launch_tags_to_scan_order(tags_by_row_dev, h->row_ids, h->Np, t, st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);   // the caller's array may go away after the call
  if (e != hipSuccess) { hipFree(t); rihip_set_error("sq8_filter_set_tags: %s", hipGetErrorString(e)); return RIHIP_ERR_HIP; }
  rihip_bump_generation();
  h->tags = t;
  return RIHIP_OK;
}

extern "C" int rihip_sq8_filter_has_tags(void* handle) { return handle && ((Sq8Index*)handle)->tags ? 1 : 0; }

extern "C" int rihip_sq8_filter_stats(void* handle, int64_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "sq8_filter_stats: bad arguments");
  out[0] = h->filt_stats[0]; out[1] = h->filt_stats[1];
  return RIHIP_OK;
}

extern "C" int rihip_sq8_filter_search(void* handle, const float* Q, int64_t nq, int k, int mode, const uint32_t* pred_dev,
                                       int64_t pred_stride, float* out_scores, int64_t* out_rows, int32_t* out_iscores,
                                       void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RCCHK(sq8_check_search(h, {"sq8_filter_search", Q, nq, k, 0, mode, out_scores && out_rows, true, pred_dev, pred_stride, nullptr}));
  Sq8SearchOpts o;
  o.pred = pred_dev; o.pred_stride = (int)pred_stride;
  return sq8_search(h, Q, nq, k, mode, out_scores, out_rows, out_iscores, (hipStream_t)stream, o);
}

// ---- seen-item exclusion inside the int8 scan ---------------------------------------------------------------------
extern "C" int rihip_sq8_exclude_search(void* handle, const float* Q, int64_t nq, int k, int mode, const int64_t* user_ids,
                                        const int64_t* seen_offsets, int64_t n_seen_rows, const int32_t* seen_items,
                                        const int32_t* row_of, int64_t n_ids, const uint32_t* pred_dev, int64_t pred_stride,
                                        float* out_scores, int64_t* out_rows, int32_t* out_iscores, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  const SeenArgs sn{user_ids, seen_offsets, n_seen_rows, seen_items, row_of, n_ids};
  RCCHK(sq8_check_search(h, {"sq8_exclude_search", Q, nq, k, 0, mode, out_scores && out_rows, false, pred_dev, pred_stride, &sn}));
  Sq8SearchOpts o;
  o.pred = pred_dev; o.pred_stride = (int)pred_stride; o.seen = &sn;
  return sq8_search(h, Q, nq, k, mode, out_scores, out_rows, out_iscores, (hipStream_t)stream, o);
}

extern "C" int rihip_sq8_exclude_mask_words(void* handle, int64_t* words_per_query) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0 && words_per_query, RIHIP_ERR_STATE, "sq8_exclude_mask_words: index is empty");
  *words_per_query = (h->Np + 31) / 32;
  return RIHIP_OK;
}

extern "C" int rihip_sq8_exclude_mask(void* handle, int64_t nq, const int64_t* user_ids, const int64_t* seen_offsets,
                                      int64_t n_seen_rows, const int32_t* seen_items, const int32_t* row_of, int64_t n_ids,
                                      uint32_t* out_mask, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "sq8_exclude_mask: index is empty");
  RIHIP_REQUIRE(nq > 0 && seen_offsets && seen_items && n_seen_rows >= 0 && row_of && n_ids > 0 && out_mask, RIHIP_ERR_ARG,
                "sq8_exclude_mask: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  RCCHK(sq8_ensure_inv_pos(h, st));
  const int64_t W = (h->Np + 31) / 32;
  HIPCHK(hipMemsetAsync(out_mask, 0, sizeof(uint32_t) * (size_t)(nq * W), st));
  const SeenArgs sn{user_ids, seen_offsets, n_seen_rows, seen_items, row_of, n_ids};
  for (int64_t q0 = 0; q0 < nq; q0 += SQ8_CH) {
    const int64_t n = std::min(SQ8_CH, nq - q0);
    launch_xmask(sn, q0, n, h->inv_pos, h->N, out_mask + q0 * W, W, 1, st);
  }
  return check_launch("sq8 exclusion mask");
}

extern "C" int rihip_sq8_exclude_set_exclusion_budget(void* handle, int64_t bytes) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && bytes >= 0, RIHIP_ERR_ARG, "sq8_exclude_set_exclusion_budget: bad arguments");
  h->xmask_budget = bytes > 0 ? bytes : XMASK_BUDGET;
  return RIHIP_OK;
}

extern "C" int rihip_sq8_exclude_scratch_nonzero(void* handle, int64_t* n_words, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && n_words, RIHIP_ERR_ARG, "sq8_exclude_scratch_nonzero: bad arguments");
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

extern "C" int rihip_sq8_exclude_exclusion_stats(void* handle, int64_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "sq8_exclude_exclusion_stats: bad arguments");
  for (int i = 0; i < 3; ++i) out[i] = h->excl_stats[i];
  return RIHIP_OK;
}
