// Handle of the 8-bit scalar-quantised index, shared by sq8.hip (build, search, refine, filter, state I/O) and
// sq8_update.hip (add / remove / replace), and the one function that makes a code.  Both files compile with
// `#pragma clang fp contract(off)` at their top: the quantiser is specified operation by operation.
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
  int8_t* codes = nullptr;        // [Np, dpad] physical order, padding rows and columns 0
  float* centre = nullptr;        // [dpad] (columns >= du: 0)
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

__device__ __forceinline__ int sq8_code(float x, float m, float s) {
  float v = rintf((x - m) / s);            // one f32 subtraction, one correctly rounded f32 division, round to nearest even
  v = fminf(fmaxf(v, -127.f), 127.f);
  return (int)v;
}

}  // namespace rihip_index
