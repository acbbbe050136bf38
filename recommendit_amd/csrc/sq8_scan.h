// The list-major int8 scan's arguments, its candidate key and its launcher (sq8_scan.hip, the only unit that instantiates
// sq8_scan_lm_kernel).  sq8.hip fills the arguments and decodes the keys.
#pragma once
#include "common.h"

namespace rihip_index {

struct Sq8LmArgs {
  const int8_t* codes;       // [Np, DP]
  const int8_t* qhi;         // [nq, DP]
  const int8_t* qlo;
  const float* thr;          // [nq] threshold as finalize (mode 1) wrote it, or null: every probed row is a candidate
  uint64_t* cand; int64_t cap; int* count;
  const int64_t* row_ids; const int64_t* list_poff; const int* list_len;
  const int* list_qoff; const int* list_q; const int* work_off; const int* plan;
  int nlist, tile_step, nprobe, count_stride;
  int64_t dense_cap;         // > 0: dense slots, cand = [nq*nprobe, dense_cap]
  int dense_ids;             // dense slots carry the original row id instead of 0 (threshold sample)
  // filtered search (sq8_scan_lm_kernel<DP, true> only)
  const uint32_t* tags;      // [Np] tag word of every physical row (padding rows 0)
  const uint32_t* pred;      // query q's predicate (any_of, all_of, none_of) at pred[q * pred_stride]
  int pred_stride;           // 3 = one per query, 0 = one shared by the batch
  // seen-item exclusion (the masked instantiations): a tile at physical row p is the one aligned word
  // xmask[mrow * xW + (p >> 5)] of every query, mrow = xrow ? xrow[q] : q (xrow: the re-do's original queries)
  const uint32_t* xmask;
  int64_t xW;
  const int* xrow;
  // product-quantised source (the PQ instantiations): codes is then the [Np, DP / PQ] matrix of entry numbers
  const int8_t* pq_book;     // [DP / PQ, 256, PQ]
  // residual PQ (the residual instantiations): T of every (query, probed list) pair, indexed as list_q names a pair
  const int* pair_t;         // [nq * nprobe]
};

__device__ __forceinline__ uint64_t sq8_key(int S, uint32_t row) {
  return ((uint64_t)((uint32_t)S ^ 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - row);
}
__device__ __forceinline__ int sq8_score_of_word(uint32_t hw) { return (int)(hw ^ 0x80000000u); }

// sq8_scan_lm_kernel<dpad, fm, pq_dsub> over `grid` workgroups of 256: dpad 64 / 128, fm an FM_* of search_keys.h,
// pq_dsub 0 (the int8 matrix) / 8 / 16 (entry numbers and codebooks); residual (pq_dsub != 0 only): scores carry pair_t
void sq8_launch_scan(int dpad, int fm, int pq_dsub, bool residual, dim3 grid, hipStream_t st, const Sq8LmArgs& x);

}  // namespace rihip_index
