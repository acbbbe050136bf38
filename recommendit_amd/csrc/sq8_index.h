// Handle of the 8-bit scalar-quantised index, shared by sq8.hip (build, search, refine, filter, state I/O),
// sq8_update.hip (add / remove / replace) and pq.hip (the product-quantised storage of the same handle: training,
// encoding, decoding, state I/O), and the one function that makes a code.  All three compile with
// `#pragma clang fp contract(off)` at their top: the quantisers are specified operation by operation.
#pragma once
#include "common.h"
#include "ip_index.h"

#include <vector>

namespace rihip_index {

struct Sq8Index {
  int du = 0;        // caller's width (1 .. 128)
  int dk = 0;        // width of the f32 side (centroids, coarse queries): 32 / 64 / 128, as the source index
  int dpad = 0;      // bytes per code row: 64 / 128
  int64_t N = 0, Np = 0;
  int nlist = 0, nprobe = 1;
  int8_t* codes = nullptr;        // [Np, dpad] physical order, padding rows and columns 0 (null on a PQ handle)
  // product-quantised storage (pq.hip) in place of `codes`: the row's SQ8 code is book[m][pq_codes[p][m]][:] per sub-space
  uint8_t* pq_codes = nullptr;    // [Np, M] physical order, M = dpad / pq_dsub; padding rows 0
  int8_t* pq_book = nullptr;      // [M, 256, pq_dsub], entries in [-127, 127]
  int pq_dsub = 0;                // 8 / 16 (0: an SQ8 handle)
  std::vector<int64_t> pq_trace;  // distortion of every assignment pass of the build (empty: injected codebooks, loaded)
  int64_t pq_peak_bytes = 0;      // device bytes at the build's peak (the transient SQ8 codes included)
  double pq_ms[3] = {0, 0, 0};    // host time of the build: range pass + SQ8 encode, codebook training, final assignment
  float* centre = nullptr;       // [dpad] (columns >= du: 0)
  float* scale = nullptr;         // [dpad] (columns >= du: 1)
  float* C = nullptr;             // [nlist, dk]
  int64_t* list_poff = nullptr;   // [nlist+1]
  int* list_len_dev = nullptr;    // [nlist]
  int64_t* row_ids = nullptr;     // [Np] original row, -1 = padding
  std::vector<int64_t> list_len;
  const int64_t* id_map = nullptr;   // not owned
  int64_t stats[2] = {0, 0};         // queries searched thresholded, of those re-done dense
  // filtered search (rihip_sq8_filter_set_tags): one 32-bit tag word per physical row, padding rows 0, or null
  uint32_t* tags = nullptr;          // [Np]
  int64_t filt_stats[2] = {0, 0};    // queries searched filtered, of those re-done dense
  // seen-item exclusion inside the scan (rihip_sq8_exclude_search): as IpIndex's -- the inverse of row_ids (built on first
  // use, dropped with the row order), the mask scratch (all zero between calls) and its budget
  int* inv_pos = nullptr;            // [N] original row -> physical position
  DevBuf<uint32_t> xmask;
  bool xmask_dirty = false;
  int64_t xmask_budget = XMASK_BUDGET;
  int64_t excl_stats[3] = {0, 0, 0};   // queries searched this way, of those re-done dense, mask chunks
  // refined search (rihip_sq8_refine_attach_vectors): the f32 rows next to the codes, or null
  float* vec = nullptr;              // [N, dk] insertion-row order (stage 1 returns rows: no inverse map)
  double* ref_e = nullptr;           // [dk] e_j = max_i |x_ij - (m_j + s_j c_ij)| over the stored rows
  double* ref_a = nullptr;           // [dk] a_j = max_i |x_ij|
  // updates (rihip_sq8_update_apply): calls that changed the index, rows dropped, rows added, code values clamped
  int64_t upd_stats[4] = {0, 0, 0, 0};
  // scratch
  DevBuf<int8_t> qhi, qlo, fhi, flo;
  DevBuf<float> qt, qpad, fQ, coarse, thr;
  DevBuf<double> qb;
  DevBuf<uint64_t> cand, scand, fcand;
  DevBuf<uint32_t> fpred;            // the predicates of one re-do chunk
  // refined search: stage 1's output at k_scan, the f32 keys, valid candidates and smallest integer score per query
  DevBuf<float> rs;
  DevBuf<int64_t> rr;
  DevBuf<int> ri, rnv, rcut;
  DevBuf<uint64_t> rkeys;
  DevBuf<int> count, probe_list, list_q, list_cnt, list_qoff, list_cur, work_off, plan, fail_flags, fail_list, n_fail;
  int* h_nfail = nullptr;   // pinned
};

inline bool sq8_has_storage(const Sq8Index* h) { return h && (h->codes || h->pq_codes); }

// what pq.hip needs of sq8.hip: the SQ8 build (layout, row ids, quantiser, codes), the layout upload, the bytes a handle
// holds and its destructor
int sq8_build_handle(Sq8Index* h, const IpIndex* src, const float* centre, const float* scale, hipStream_t st);
int sq8_upload_list_layout(Sq8Index* h, hipStream_t st);
int64_t sq8_held_bytes(const Sq8Index* h);
void sq8_free_handle(Sq8Index* h);
// and what sq8.hip needs of pq.hip: the decoded code matrix [Np, dpad] of a PQ handle in a fresh device allocation the
// caller frees (a transient Np * dpad bytes)
int pq_decode_all(const Sq8Index* h, int8_t** out_dev, hipStream_t st);

__device__ __forceinline__ int sq8_code(float x, float m, float s) {
  float v = rintf((x - m) / s);            // one f32 subtraction, one correctly rounded f32 division, round to nearest even
  v = fminf(fmaxf(v, -127.f), 127.f);
  return (int)v;
}

}  // namespace rihip_index
