// 8-bit scalar-quantised inner-product index (flat and IVF): the handle, its kernels and its C ABI.
//
// A second handle type next to IpIndex.  It is built from the f32 rows of a built IpIndex, in that index's physical order
// (lists padded to 64-row granules; a flat source becomes one list), and stores one int8 code per dimension:
//   m_j = 0.5f (lo_j + hi_j), s_j = (hi_j - lo_j) / 254.0f (1 where hi_j == lo_j), c_ij = clamp(rint((x_ij - m_j) / s_j), +-127)
// The query side keeps 16 bits: w_j = q_j s_j, t = max|w| / 32512, n_j = rint(w_j / t) split into two int8 limbs
// n = 256 hi + lo.  The scan scores S_i = sum_j n_j c_ij on the i8 MFMA (two chains into two i32 accumulators,
// S = 256 S_hi + S_lo, |S| <= 32512 * 127 * 128 < 2^31): integers, so ranking, ties and the completeness check of the
// thresholded pass are exact.  The reported score is (float)(b + t S) with b = sum_j q_j m_j in f64.
//
// The search reuses what does not depend on the corpus representation: the coarse quantizer, probe selection, work plan
// and scatter of ivf_search.hip and finalize_kernel of select.hip.  Candidate keys are make_key's with the integer score
// in the high word ((uint32)S ^ 0x80000000: unsigned order = signed order; never 0, the empty-slot key).  finalize emits a
// key's high word through ord2f, a bijection of the 32 bits, so sq8_decode_kernel recovers S from the float it wrote.
//
// Opt-in on top of that (the "refined search" section): the source's f32 rows attached next to the codes, an exact f32
// re-score of the search's best k_scan candidates, and a per-query certificate that the re-ranked list is the exact one.
//
// A handle may hold product-quantised storage instead of the int8 matrix (pq.hip builds it: one byte per sub-space and row
// plus int8 codebooks).  sq8_scan picks the source; the PQ instantiations of the scan gather the operand bytes from the
// codebooks in LDS, and everything else in this file is the same code for both.
#pragma clang fp contract(off)   // the quantiser is specified operation by operation: no fused multiply-add
#include "common.h"
#include "recommendit_hip.h"

#include <algorithm>
#include <math.h>
#include <string.h>
#include <vector>

#include "search_kernels.h"
#include "search_keys.h"
#include "sq8_index.h"

using namespace rihip_index;

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr float SQ8_QMAX = 32512.0f;            // largest |n_j|: 127 * 256, so both limbs fit int8
constexpr int64_t SQ8_DENSE_BUDGET = 1ll << 26;  // dense candidate slots (8 B each) of one query chunk: 512 MiB
constexpr int64_t SQ8_DENSE_AUTO = 1ll << 23;    // auto: dense while the batch's slots stay under 64 MiB (the f32 index's rule;
                                                 // at 256 queries x IVF 100/10 of 1 M rows dense measured 0.46 ms, thresholded 0.23)
constexpr int SQ8_TARGET = 16 * RIHIP_NCU;      // wave work items aimed at (as the f32 list-major scan)
constexpr int SQ8_SS = 16;                      // threshold sample: every 16th probed tile
constexpr int64_t SQ8_CH = 4096;                // queries per internal pass at most

int64_t held_bytes(const Sq8Index* h) {
  // the code storage: the int8 matrix, or (a PQ handle) one byte per sub-space and row plus the codebooks
  const int64_t rows = h->pq_codes ? h->Np * (h->dpad / h->pq_dsub) + 256 * (int64_t)h->dpad : h->Np * h->dpad;
  return rows + 2 * 4 * (int64_t)h->dpad + 4 * (int64_t)h->nlist * h->dk + 8 * (int64_t)(h->nlist + 1) +
         4 * (int64_t)h->nlist + 8 * h->Np + (h->vec ? 4 * h->N * h->dk + 2 * 8 * (int64_t)h->dk : 0) + (h->tags ? 4 * h->Np : 0);
}

void drop_tags(Sq8Index* h) {
  if (!h->tags) return;
  rihip_bump_generation();
  hipFree(h->tags);
  h->tags = nullptr;
}

void drop_vectors(Sq8Index* h) {
  if (!h->vec) return;
  rihip_bump_generation();
  hipFree(h->vec); hipFree(h->ref_e); hipFree(h->ref_a);
  h->vec = nullptr; h->ref_e = nullptr; h->ref_a = nullptr;
}

void free_sq8(Sq8Index* h) {
  rihip_bump_generation();
  drop_vectors(h);
  drop_tags(h);
  h->fpred.release(); h->xmask.release();
  hipFree(h->inv_pos);
  h->rs.release(); h->rr.release(); h->ri.release(); h->rnv.release(); h->rcut.release(); h->rkeys.release();
  hipFree(h->codes); hipFree(h->pq_codes); hipFree(h->pq_book); hipFree(h->centre); hipFree(h->scale); hipFree(h->C); hipFree(h->list_poff); hipFree(h->list_len_dev);
  hipFree(h->row_ids);
  h->qhi.release(); h->qlo.release(); h->fhi.release(); h->flo.release(); h->qt.release(); h->qpad.release(); h->fQ.release();
  h->coarse.release(); h->thr.release(); h->qb.release(); h->cand.release(); h->scand.release(); h->fcand.release();
  h->count.release(); h->probe_list.release(); h->list_q.release(); h->list_cnt.release(); h->list_qoff.release();
  h->list_cur.release(); h->work_off.release(); h->plan.release(); h->fail_flags.release(); h->fail_list.release();
  h->n_fail.release();
  if (h->h_nfail) hipHostFree(h->h_nfail);
  delete h;
}

// ------------------------------------------------ quantiser ----------------------------------------------------------
// column min / max of the real rows, fixed order: block b takes a contiguous row range, thread (rr, c) every rpp-th row of
// column c, the rpp partial results of a column are combined in rr order, the blocks' results in block order (no atomics)
__global__ __launch_bounds__(256) void sq8_colrange_part_kernel(const float* __restrict__ X, const int64_t* __restrict__ row_ids,
                                                                int64_t n_rows, int dk, float* part) {
  __shared__ float slo[256], shi[256];
  const int tid = threadIdx.x, rpp = 256 / dk, rr = tid / dk, c = tid % dk;
  const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = (r0 + per < n_rows) ? r0 + per : n_rows;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t r = r0 + rr; r < r1; r += rpp) {
    if (row_ids && row_ids[r] < 0) continue;
    const float v = X[(size_t)r * dk + c];
    lo = fminf(lo, v); hi = fmaxf(hi, v);
  }
  slo[tid] = lo; shi[tid] = hi;
  __syncthreads();
  if (rr == 0) {
    for (int k = 1; k < rpp; ++k) { lo = fminf(lo, slo[k * dk + c]); hi = fmaxf(hi, shi[k * dk + c]); }
    part[((size_t)blockIdx.x * 2 + 0) * dk + c] = lo;
    part[((size_t)blockIdx.x * 2 + 1) * dk + c] = hi;
  }
}
__global__ void sq8_colrange_final_kernel(const float* __restrict__ part, int nb, int dk, int dpad, float* centre, float* scale) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= dpad) return;
  float m = 0.f, s = 1.f;
  if (j < dk) {
    float lo = INFINITY, hi = -INFINITY;
    for (int b = 0; b < nb; ++b) { lo = fminf(lo, part[((size_t)b * 2 + 0) * dk + j]); hi = fmaxf(hi, part[((size_t)b * 2 + 1) * dk + j]); }
    if (lo <= hi) {
      m = 0.5f * (lo + hi);
      s = (hi == lo) ? 1.f : (hi - lo) / 254.0f;
    }
  }
  centre[j] = m; scale[j] = s;
}

// four codes per thread; rows beyond n_src, padding rows (row_ids < 0) and columns >= dk are 0
__global__ void sq8_encode_kernel(const float* __restrict__ X, const int64_t* __restrict__ row_ids, int64_t n_src, int64_t Np,
                                  int dk, int dpad, const float* __restrict__ centre, const float* __restrict__ scale,
                                  int8_t* codes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_row = dpad / 4;
  if (i >= Np * per_row) return;
  const int64_t r = i / per_row;
  const int j = (int)(i % per_row) * 4;
  uint32_t packed = 0;
  if (r < n_src && j < dk && row_ids[r] >= 0) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(X + (size_t)r * dk + j);
#pragma unroll
    for (int u = 0; u < 4; ++u) packed |= ((uint32_t)sq8_code(x[u], centre[j + u], scale[j + u]) & 0xFFu) << (8 * u);
  }
  *reinterpret_cast<uint32_t*>(codes + (size_t)r * dpad + j) = packed;
}

__global__ void sq8_identity_rows_kernel(int64_t* row_ids, int64_t N, int64_t Np) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Np) row_ids[i] = i < N ? i : -1;
}

// decoded rows in original row order: out[row, j] = m_j + s_j c (two roundings)
__global__ void sq8_reconstruct_kernel(const int8_t* __restrict__ codes, const int64_t* __restrict__ row_ids, int64_t Np, int du,
                                       int dpad, const float* __restrict__ centre, const float* __restrict__ scale, float* out,
                                       int8_t* out_codes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Np * du) return;
  const int64_t p = i / du;
  const int j = (int)(i % du);
  const int64_t row = row_ids[p];
  if (row < 0) return;
  const int8_t c = codes[(size_t)p * dpad + j];
  if (out_codes) out_codes[(size_t)row * du + j] = c;
  if (out) {
    const float prod = scale[j] * (float)c;
    out[(size_t)row * du + j] = centre[j] + prod;
  }
}

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

// ------------------------------------------------ list-major scan ----------------------------------------------------
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
};

__device__ __forceinline__ uint64_t sq8_key(int S, uint32_t row) {
  return ((uint64_t)((uint32_t)S ^ 0x80000000u) << 32) | (uint64_t)(0xFFFFFFFFu - row);
}
__device__ __forceinline__ int sq8_score_of_word(uint32_t hw) { return (int)(hw ^ 0x80000000u); }

// The work plan is ivf_scan_lm_kernel's: a wave takes (one list, 32 of the queries that probe it, a range of the list's
// 32-row tiles).  The 32 queries' limb rows are the B operands and stay in registers; a code tile is loaded straight into
// the A-operand registers (lane (r, h) holds bytes 32 ks + 16 h .. + 15 of row r for k-step ks -- the same bytes of its
// query on the B side, so whatever order the instruction gives the 16 bytes of a lane, both operands agree on it), the
// next tile's loads are in flight under the chain.  No LDS, no barrier, no float arithmetic.
//
// FILT: a lane holds query column lane & 31, so it keeps that query's three predicate words; the tag words of its 16
// accumulator rows (four runs of four consecutive rows: acc_row) are four 16-byte loads per tile, issued with the next
// tile's code loads.  A row that fails is absent from all three emissions: its dense or sample slot holds the empty key 0
// and it is not a survivor.
// FM (search_keys.h): FM_TAGS is the above; FM_TAGS_MASK / FM_MASK add the seen-item mask: the tile is one aligned word of
// the lane's query, loaded one tile ahead with the code and tag loads; FM_MASK compiles the tag test out (an untagged
// index).  FM_NONE and FM_TAGS are the kernels as they were.
//
// PQ = 8 / 16 (0: the int8 matrix as above): the source is product-quantised with PQ dimensions per sub-space.  The
// workgroup copies the codebooks [DP / PQ, 256, PQ] to LDS once (DP * 256 bytes: two workgroups per CU still fit) and
// meets at one barrier before any wave leaves.  What is loaded one tile ahead is the row's DP / PQ entry numbers; the 16
// operand bytes of lane (r, h) at k-step ks are then gathered from LDS when the tile's chain starts: columns
// 32 ks + 16 h .. + 15 are sub-spaces 4 ks + 2 h and + 1 (PQ = 8: two 8-byte reads) or sub-space 2 ks + h (PQ = 16: one
// 16-byte read).  An entry lies in LDS in column order, so the lane holds the bytes the int8 matrix of the decoded rows
// would have given it, in the same order: the B side does not change.  A row beyond its list's length decodes to entry 0
// of every sub-space, not to zeros; n_ok keeps it out of every emission, as before.
template <int DP, int FM = FM_NONE, int PQ = 0>
__global__ __launch_bounds__(256, 2) void sq8_scan_lm_kernel(Sq8LmArgs a) {
  constexpr bool FILT = FM == FM_TAGS || FM == FM_TAGS_MASK, XM = FM == FM_TAGS_MASK || FM == FM_MASK;
  constexpr int KS = DP / 32;
  constexpr int CW = PQ ? DP / PQ / 4 : 1;   // 32-bit words of entry numbers per row
  __shared__ i32x4 s_book[PQ ? DP * 16 : 1];
  if constexpr (PQ != 0) {
    if (blockIdx.x * 4 >= a.plan[0]) return;   // workgroup-uniform: no wave of it has work
    const i32x4* gb = reinterpret_cast<const i32x4*>(a.pq_book);
    for (int i = threadIdx.x; i < DP * 16; i += 256) s_book[i] = gb[i];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r31 = lane & 31, hh = lane >> 5;
  const int wi = blockIdx.x * 4 + w;
  if (wi >= a.plan[0]) return;  // wave-uniform
  int lo = 0, hi = a.nlist;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.work_off[mid] <= wi) lo = mid; else hi = mid;
  }
  const int c = lo;
  const int rem = wi - a.work_off[c];
  const int64_t p0 = a.list_poff[c];
  const int64_t tiles = (a.list_poff[c + 1] - p0) / TRS;
  const int tstep = a.tile_step > 1 ? a.tile_step : 1;
  const int64_t n_seq = (tiles + tstep - 1) / tstep;
  const int tpi = a.plan[1];
  const int s_c = (int)((n_seq + tpi - 1) / tpi);
  if (s_c <= 0) return;
  const int grp = rem / s_c, split = rem % s_c;
  const int q0 = a.list_qoff[c], m = a.list_qoff[c + 1] - q0;
  if (grp * 32 >= m) return;
  const int slot = grp * 32 + r31;
  const bool q_ok = slot < m;
  const int pair = a.list_q[q0 + (q_ok ? slot : grp * 32)];
  const int64_t q = pair / a.nprobe;
  const int len = a.list_len[c];
  i32x4 bh[KS], bl[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    bh[ks] = *reinterpret_cast<const i32x4*>(a.qhi + (size_t)q * DP + ks * 32 + 16 * hh);
    bl[ks] = *reinterpret_cast<const i32x4*>(a.qlo + (size_t)q * DP + ks * 32 + 16 * hh);
  }
  const int thr = a.thr ? sq8_score_of_word(f2ord(a.thr[q])) : (int)0x80000000;
  uint64_t* my_cand = a.cand + (size_t)q * a.cap;
  uint64_t* my_dense = a.dense_cap > 0 ? a.cand + (size_t)pair * a.dense_cap : nullptr;
  const int64_t i0 = (int64_t)split * tpi;
  const int64_t i1 = (i0 + tpi < n_seq) ? i0 + tpi : n_seq;
  if (i0 >= i1) return;

  i32x4 av[KS], nx[KS];
  auto load_tile = [&](int64_t i, i32x4* dst) {
    const i32x4* src = reinterpret_cast<const i32x4*>(a.codes + (size_t)(p0 + i * tstep * TRS + r31) * DP + 16 * hh);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) dst[ks] = src[ks * 2];
  };
  // PQ: the entry numbers of the lane's row (both lanes of a row load all of them: 4 to 16 bytes), and the gather
  uint32_t cw[CW], cn[CW];
  auto load_words = [&](int64_t i, uint32_t* dst) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.codes) + (size_t)(p0 + i * tstep * TRS + r31) * CW;
#pragma unroll
    for (int c = 0; c < CW; ++c) dst[c] = src[c];
  };
  auto gather = [&](const uint32_t* words, i32x4* dst) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      if constexpr (PQ == 8) {
        const uint32_t two = words[ks] >> (16 * hh);   // sub-spaces 4 ks + 2 hh and + 1 are bytes 2 hh and 2 hh + 1 of word ks
        const int m0 = 4 * ks + 2 * hh;
        const uint2* lb = reinterpret_cast<const uint2*>(s_book);
        const uint2 x = lb[m0 * 256 + (int)(two & 255u)];
        const uint2 y = lb[(m0 + 1) * 256 + (int)((two >> 8) & 255u)];
        dst[ks] = i32x4{(int)x.x, (int)x.y, (int)y.x, (int)y.y};
      } else {
        const uint32_t e = (words[ks >> 1] >> (8 * (2 * (ks & 1) + hh))) & 255u;   // sub-space 2 ks + hh
        dst[ks] = s_book[(2 * ks + hh) * 256 + (int)e];
      }
    }
  };
  Pred pr{0u, 0u, 0u};
  uint4 tw[4], tn[4];
  auto load_tags = [&](int64_t i, uint4* dst) {   // rows 4 hh + 8 g .. + 3 of tile i: the lane's accumulator rows 4 g .. 4 g + 3
    const uint4* tp = reinterpret_cast<const uint4*>(a.tags + p0 + i * tstep * TRS + 4 * hh);
#pragma unroll
    for (int g = 0; g < 4; ++g) dst[g] = tp[2 * g];
  };
  if constexpr (FILT) {
    pr = load_pred(a.pred, q, a.pred_stride);
    load_tags(i0, tw);
  }
  const uint32_t* my_mask = nullptr;
  uint32_t mw = 0u, mn = 0u;
  if constexpr (XM) {
    my_mask = a.xmask + (size_t)(a.xrow ? a.xrow[q] : q) * a.xW;
    mw = my_mask[(p0 + i0 * tstep * TRS) >> 5];
  }
  auto row_ok = [&](int r) -> bool {   // FILT / XM: may accumulator row r of the lane be a candidate?
    bool ok = true;
    if constexpr (FILT) ok = pr.pass(tag_of(tw, r));
    if constexpr (XM) ok = ok && !((mw >> acc_row(r, lane)) & 1u);
    return ok;
  };
  if constexpr (PQ != 0) load_words(i0, cw);
  else load_tile(i0, av);
#pragma unroll 1
  for (int64_t i = i0; i < i1; ++i) {
    const bool more = i + 1 < i1;
    if constexpr (PQ != 0) gather(cw, av);
    if (more) {
      if constexpr (PQ != 0) load_words(i + 1, cn);
      else load_tile(i + 1, nx);
      if constexpr (FILT) load_tags(i + 1, tn);
      if constexpr (XM) mn = my_mask[(p0 + (i + 1) * tstep * TRS) >> 5];
    }
    i32x16 ah, al;
#pragma unroll
    for (int r = 0; r < 16; ++r) { ah[r] = 0; al[r] = 0; }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[ks], bh[ks], ah, 0, 0, 0);
      al = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[ks], bl[ks], al, 0, 0, 0);
    }
    if (q_ok) {
      const int64_t t_row0 = i * tstep * TRS;
      const int64_t left = (int64_t)len - t_row0;
      const int n_ok = left >= TRS ? TRS : (left > 0 ? (int)left : 0);
      if (my_dense) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int rr = acc_row(r, lane);
          const int64_t sl = i * TRS + rr;
          if (sl < a.dense_cap)
            my_dense[sl] = (rr < n_ok && row_ok(r)) ? sq8_key(ah[r] * 256 + al[r], a.dense_ids ? (uint32_t)a.row_ids[p0 + t_row0 + rr] : 0u) : 0ull;
        }
      } else {
        unsigned hits = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (acc_row(r, lane) < n_ok && ah[r] * 256 + al[r] >= thr && row_ok(r)) hits |= (1u << r);
        if (hits) {
          int pos = atomicAdd(&a.count[q * a.count_stride], __popc(hits));
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (hits & (1u << r)) {
              const int64_t v = p0 + t_row0 + acc_row(r, lane);
              if (pos < a.cap) my_cand[pos] = sq8_key(ah[r] * 256 + al[r], (uint32_t)a.row_ids[v]);
              ++pos;
            }
          }
        }
      }
    }
    if (more) {
      if constexpr (PQ != 0) {
#pragma unroll
        for (int c = 0; c < CW; ++c) cw[c] = cn[c];
      } else {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) av[ks] = nx[ks];
      }
      if constexpr (FILT) {
#pragma unroll
        for (int g = 0; g < 4; ++g) tw[g] = tn[g];
      }
      if constexpr (XM) mw = mn;
    }
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
  return check_launch("sq8 prepare");
}

template <int PQ>
void sq8_launch_scan(int dpad, int fm, dim3 grid, hipStream_t st, const Sq8LmArgs& x) {
  auto go = [&](auto FMv) {
    constexpr int FM = decltype(FMv)::value;
    if (dpad == 64) hipLaunchKernelGGL((sq8_scan_lm_kernel<64, FM, PQ>), grid, dim3(256), 0, st, x);
    else hipLaunchKernelGGL((sq8_scan_lm_kernel<128, FM, PQ>), grid, dim3(256), 0, st, x);
  };
  if (fm == FM_TAGS_MASK) go(std::integral_constant<int, FM_TAGS_MASK>{});
  else if (fm == FM_MASK) go(std::integral_constant<int, FM_MASK>{});
  else if (fm == FM_TAGS) go(std::integral_constant<int, FM_TAGS>{});
  else go(std::integral_constant<int, FM_NONE>{});
}

int sq8_scan(const Sq8Search& s, const Sq8Geom& g, const float* thr, uint64_t* cand, int64_t cap, int tile_step,
             int64_t dense_cap, bool planned, int dense_ids) {
  Sq8Index* h = s.h;
  if (!planned)
    launch_ivf_plan(h->list_cnt.p, h->list_poff, g.nlist, tile_step, SQ8_TARGET, h->list_qoff.p, h->list_cur.p, h->work_off.p,
                    h->plan.p, h->count.p, s.nq * CSTRIDE, s.st);
  Sq8LmArgs x;
  memset(&x, 0, sizeof(x));
  x.codes = h->codes; x.qhi = s.qhi; x.qlo = s.qlo; x.thr = thr; x.cand = cand; x.cap = cap; x.count = h->count.p;
  x.row_ids = h->row_ids; x.list_poff = h->list_poff; x.list_len = h->list_len_dev; x.list_qoff = h->list_qoff.p;
  x.list_q = h->list_q.p; x.work_off = h->work_off.p; x.plan = h->plan.p; x.nlist = g.nlist; x.tile_step = tile_step;
  x.nprobe = g.nprobe; x.count_stride = CSTRIDE; x.dense_cap = dense_cap; x.dense_ids = dense_ids;
  x.tags = s.pred ? h->tags : nullptr; x.pred = s.pred; x.pred_stride = s.pred_stride;
  x.xmask = s.xmask; x.xW = s.xW; x.xrow = s.xrow;
  // n_work <= sum over (list, group) of (tiles/tpi + 1) <= target + #(list, query group) pairs
  const int64_t bound = (int64_t)SQ8_TARGET + g.nlist + (s.nq * g.nprobe + 31) / 32 + 4;
  const dim3 grid((unsigned)((bound + 3) / 4));
  const int fm = x.xmask ? (x.tags ? FM_TAGS_MASK : FM_MASK) : (x.tags ? FM_TAGS : FM_NONE);
  const char* what = fm == FM_TAGS_MASK ? "masked filtered sq8 scan" : fm == FM_MASK ? "masked sq8 scan" : fm == FM_TAGS ? "filtered sq8 scan" : "sq8 scan";
  if (h->pq_codes) {   // the product-quantised source: entry numbers and the codebooks
    x.codes = reinterpret_cast<const int8_t*>(h->pq_codes); x.pq_book = h->pq_book;
    if (h->pq_dsub == 8) sq8_launch_scan<8>(h->dpad, fm, grid, s.st, x);
    else sq8_launch_scan<16>(h->dpad, fm, grid, s.st, x);
    return check_launch(what);
  }
  sq8_launch_scan<0>(h->dpad, fm, grid, s.st, x);
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

int sq8_transform_queries(Sq8Index* h, const float* Q, int64_t nq, int16_t* n16, float* t_out, double* b_out, hipStream_t st) {
  RCCHK(h->qhi.reserve(nq * h->dpad));
  RCCHK(h->qlo.reserve(nq * h->dpad));
  if (!t_out) { RCCHK(h->qt.reserve(nq)); t_out = h->qt.p; }
  if (!b_out) { RCCHK(h->qb.reserve(nq)); b_out = h->qb.p; }
  hipLaunchKernelGGL(sq8_query_kernel, dim3((unsigned)nq), dim3(128), 0, st, Q, nq, h->du, h->dpad, h->centre, h->scale, h->qhi.p,
                     h->qlo.p, t_out, b_out, n16);
  return check_launch("sq8 query transform");
}

// the handle's inverse of row_ids, made on first use
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

// seen: the excluded search (rihip_sq8_exclude_search) -- the queries are query q_base .. of the caller's batch; every
// internal chunk sets its mask bits, searches and clears the words it touched
int sq8_search(Sq8Index* h, const float* Q, int64_t nq, int k, int mode, float* out_s, int64_t* out_r, int* out_i,
               hipStream_t st, const uint32_t* pred = nullptr, int pred_stride = 0, const SeenArgs* seen = nullptr,
               int64_t q_base = 0) {
  RCCHK(sq8_transform_queries(h, Q, nq, nullptr, nullptr, nullptr, st));
  const float* Qf = Q;
  if (h->du != h->dk) {
    RCCHK(h->qpad.reserve(nq * h->dk));
    RCCHK(pad_rows(Q, nq, h->du, h->dk, h->qpad.p, st));
    Qf = h->qpad.p;
  }
  RIHIP_REQUIRE((reinterpret_cast<uintptr_t>(Qf) & 15) == 0, RIHIP_ERR_ARG, "sq8_index_search: Q must be 16-byte aligned");
  const Sq8Geom g = sq8_geom(h);
  bool thresholded = mode == 2;
  if (mode == 0)
    thresholded = !(nq * g.cap_df <= SQ8_DENSE_AUTO || g.cap_full <= 16384 || (double)k * 4.0 > (double)g.cap_full / SQ8_SS);
  int64_t ch = SQ8_CH;
  if (!thresholded) ch = std::max<int64_t>(1, std::min<int64_t>(SQ8_CH, SQ8_DENSE_BUDGET / g.cap_df));
  const int64_t W = (h->Np + 31) / 32;
  if (seen) {   // queries per chunk: what the mask budget holds as well (whole 128-query blocks where it holds one)
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
                pred ? pred + q0 * pred_stride : nullptr, pred_stride};
    if (seen) {
      ++h->excl_stats[2];
      launch_xmask(*seen, q_base + q0, n, h->inv_pos, h->N, h->xmask.p, W, 1, st);
      RCCHK(check_launch("sq8 exclusion mask"));
      s.xmask = h->xmask.p; s.xW = W;
    }
    RCCHK(thresholded ? sq8_thresholded(s, g) : sq8_dense(s, g, nullptr));
    if (seen) {
      launch_xmask(*seen, q_base + q0, n, h->inv_pos, h->N, h->xmask.p, W, 0, st);
      RCCHK(check_launch("sq8 exclusion mask clear"));
    }
  }
  if (seen) { h->xmask_dirty = false; h->excl_stats[0] += nq; }
  if (pred) h->filt_stats[0] += nq;
  const int64_t tot = nq * k;
  hipLaunchKernelGGL(sq8_decode_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, out_s, out_r, out_i, nq, k, h->qt.p,
                     h->qb.p, h->id_map);
  return check_launch("sq8 decode");
}

// ------------------------------------------------ build --------------------------------------------------------------
// list offsets / lengths on the device from the host copy list_len (lists padded to 64-row granules)
int sq8_upload_layout(Sq8Index* h, hipStream_t st) {
  std::vector<int64_t> poff(h->nlist + 1, 0);
  std::vector<int> len(h->nlist);
  for (int c = 0; c < h->nlist; ++c) {
    poff[c + 1] = poff[c] + (h->list_len[c] + TR - 1) / TR * TR;
    len[c] = (int)h->list_len[c];
  }
  RIHIP_REQUIRE(poff[h->nlist] == h->Np, RIHIP_ERR_STATE, "sq8_index: list lengths give %lld padded rows, the index holds %lld",
                (long long)poff[h->nlist], (long long)h->Np);
  HIPCHK(hipMalloc((void**)&h->list_poff, sizeof(int64_t) * (h->nlist + 1)));
  HIPCHK(hipMalloc((void**)&h->list_len_dev, sizeof(int) * h->nlist));
  HIPCHK(hipMemcpyAsync(h->list_poff, poff.data(), sizeof(int64_t) * (h->nlist + 1), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->list_len_dev, len.data(), sizeof(int) * h->nlist, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));   // (the host vectors go away)
  return RIHIP_OK;
}

int sq8_build(Sq8Index* h, const IpIndex* src, const float* centre, const float* scale, hipStream_t st) {
  h->du = src->du; h->dk = src->d; h->dpad = src->d <= 64 ? 64 : 128;
  h->N = src->N;
  h->nprobe = src->ivf ? src->nprobe : 1;
  const int64_t n_src = src->ivf ? src->Np : src->N;
  if (src->ivf) {
    RIHIP_REQUIRE(src->C && src->row_ids && (int)src->list_len.size() == src->nlist && src->nlist >= 1, RIHIP_ERR_STATE,
                  "sq8_index_from_ip_index: the IVF source is incomplete");
    h->nlist = src->nlist; h->Np = src->Np; h->list_len = src->list_len;
  } else {
    h->nlist = 1; h->Np = (src->N + TR - 1) / TR * TR; h->list_len.assign(1, src->N);
  }
  RCCHK(sq8_upload_layout(h, st));
  HIPCHK(hipMalloc((void**)&h->row_ids, sizeof(int64_t) * (size_t)h->Np));
  HIPCHK(hipMalloc((void**)&h->C, sizeof(float) * (size_t)h->nlist * h->dk));
  HIPCHK(hipMalloc((void**)&h->codes, (size_t)h->Np * h->dpad));
  HIPCHK(hipMalloc((void**)&h->centre, sizeof(float) * h->dpad));
  HIPCHK(hipMalloc((void**)&h->scale, sizeof(float) * h->dpad));
  if (src->ivf) {
    HIPCHK(hipMemcpyAsync(h->row_ids, src->row_ids, sizeof(int64_t) * (size_t)h->Np, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(h->C, src->C, sizeof(float) * (size_t)h->nlist * h->dk, hipMemcpyDeviceToDevice, st));
  } else {
    hipLaunchKernelGGL(sq8_identity_rows_kernel, dim3((unsigned)((h->Np + 255) / 256)), dim3(256), 0, st, h->row_ids, h->N, h->Np);
    HIPCHK(hipMemsetAsync(h->C, 0, sizeof(float) * (size_t)h->dk, st));
  }
  if (centre) {   // injected quantiser: [du] host arrays, columns beyond du are (0, 1)
    std::vector<float> m(h->dpad, 0.f), s(h->dpad, 1.f);
    for (int j = 0; j < h->du; ++j) {
      RIHIP_REQUIRE(isfinite(centre[j]) && isfinite(scale[j]) && scale[j] > 0.f, RIHIP_ERR_ARG,
                    "sq8_index_from_ip_index: column %d: centre %g, scale %g (finite, scale > 0)", j, (double)centre[j], (double)scale[j]);
      m[j] = centre[j]; s[j] = scale[j];
    }
    HIPCHK(hipMemcpyAsync(h->centre, m.data(), sizeof(float) * h->dpad, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->scale, s.data(), sizeof(float) * h->dpad, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  } else {
    const int nb = (int)std::min<int64_t>(1024, (n_src + 255) / 256);
    float* part = nullptr;
    HIPCHK(hipMalloc((void**)&part, sizeof(float) * (size_t)nb * 2 * h->dk));
    hipLaunchKernelGGL(sq8_colrange_part_kernel, dim3(nb), dim3(256), 0, st, src->X, src->ivf ? h->row_ids : nullptr, n_src, h->dk, part);
    hipLaunchKernelGGL(sq8_colrange_final_kernel, dim3(1), dim3(128), 0, st, part, nb, h->dk, h->dpad, h->centre, h->scale);
    const hipError_t e = hipStreamSynchronize(st);
    hipFree(part);
    HIPCHK(e);
  }
  const int64_t nthr = h->Np * (h->dpad / 4);
  hipLaunchKernelGGL(sq8_encode_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, src->X, h->row_ids, n_src, h->Np, h->dk,
                     h->dpad, h->centre, h->scale, h->codes);
  RCCHK(check_launch("sq8 encode"));
  HIPCHK(hipStreamSynchronize(st));   // the source may be dropped as soon as the call returns
  return RIHIP_OK;
}

// ------------------------------------------------ refined search -----------------------------------------------------
// Stage 1 is sq8_search at k_scan; stage 2 re-scores its candidates in f32 against the attached rows and selects the top k
// by (f, row); the certificate says when that list is the exact one over every probed row.  f, the bound and the
// certificate are specified at rihip_sq8_refine_search in recommendit_hip.h; the kernels below follow that text
// operation by operation (this file compiles with fp contract off, so a * b + c is two roundings unless written fmaf).

// *mismatch = 1 where the handle's physical rows differ from the source's (want == null: a flat source, row p is row p)
__global__ void sq8_rows_differ_kernel(const int64_t* __restrict__ have, const int64_t* __restrict__ want, int64_t N, int64_t Np,
                                       int* mismatch) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Np) return;
  const int64_t w = want ? want[i] : (i < N ? i : -1);
  if (have[i] != w) *mismatch = 1;
}

// vec[row_ids[p], :] = X[p, :] for the physical rows p < n_src that hold a row, four floats per thread
__global__ void sq8_scatter_rows_kernel(const float* __restrict__ X, const int64_t* __restrict__ row_ids, int64_t n_src, int dk,
                                        float* vec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_row = dk / 4;
  if (i >= n_src * per_row) return;
  const int64_t p = i / per_row;
  const int j = (int)(i % per_row) * 4;
  const int64_t row = row_ids[p];
  if (row < 0) return;
  *reinterpret_cast<f32x4*>(vec + (size_t)row * dk + j) = *reinterpret_cast<const f32x4*>(X + (size_t)p * dk + j);
}

// e_j and a_j: the layout of sq8_colrange_part_kernel (block b a contiguous range of physical rows, thread (rr, c) every
// rpp-th row of column c), f64, no atomics.  A maximum does not depend on the order it is taken in; the order is fixed
// all the same.  The STORED code is read, so a clamped code of an injected quantiser counts with its full error.
__global__ __launch_bounds__(256) void sq8_refine_range_part_kernel(const float* __restrict__ X, const int8_t* __restrict__ codes,
                                                                    const int64_t* __restrict__ row_ids, int64_t n_rows, int dk,
                                                                    int dpad, const float* __restrict__ centre,
                                                                    const float* __restrict__ scale, double* part) {
  __shared__ double se[256], sa[256];
  const int tid = threadIdx.x, rpp = 256 / dk, rr = tid / dk, c = tid % dk;
  const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = (r0 + per < n_rows) ? r0 + per : n_rows;
  const double m = (double)centre[c], s = (double)scale[c];
  double e = 0.0, a = 0.0;
  for (int64_t r = r0 + rr; r < r1; r += rpp) {
    if (row_ids[r] < 0) continue;
    const double x = (double)X[(size_t)r * dk + c];
    const double prod = s * (double)codes[(size_t)r * dpad + c];   // exact: 24 x 8 bits
    const double dec = m + prod;
    e = fmax(e, fabs(x - dec));
    a = fmax(a, fabs(x));
  }
  se[tid] = e; sa[tid] = a;
  __syncthreads();
  if (rr == 0) {
    for (int k = 1; k < rpp; ++k) { e = fmax(e, se[k * dk + c]); a = fmax(a, sa[k * dk + c]); }
    part[((size_t)blockIdx.x * 2 + 0) * dk + c] = e;
    part[((size_t)blockIdx.x * 2 + 1) * dk + c] = a;
  }
}
__global__ void sq8_refine_range_final_kernel(const double* __restrict__ part, int nb, int dk, double* e_out, double* a_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= dk) return;
  double e = 0.0, a = 0.0;
  for (int b = 0; b < nb; ++b) { e = fmax(e, part[((size_t)b * 2 + 0) * dk + j]); a = fmax(a, part[((size_t)b * 2 + 1) * dk + j]); }
  e_out[j] = e; a_out[j] = a;
}

template <int PER>
__device__ __forceinline__ void sq8_load_lane(const float* __restrict__ p, float* x) {
  if constexpr (PER == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    x[0] = v.x; x[1] = v.y;
  } else {
#pragma unroll
    for (int v = 0; v < PER / 4; ++v) {
      const f32x4 t = reinterpret_cast<const f32x4*>(p)[v];
      x[4 * v] = t[0]; x[4 * v + 1] = t[1]; x[4 * v + 2] = t[2]; x[4 * v + 3] = t[3];
    }
  }
}

// Stage 2, one workgroup per query: 16 lanes per candidate (rerank_kernel's arithmetic), four candidates of a lane group
// in flight.  keys[q, i] = make_key(f + 0.f, row) of stage 1's i-th candidate, 0 where it returned padding; n_valid[q] and
// s_cut[q] (smallest integer score among the valid candidates, 0 without any) go to the certificate.  The loop bound is
// the same for every lane, so the shuffles always run with the whole wave.
template <int D>
__global__ __launch_bounds__(256) void sq8_refine_kernel(const float* __restrict__ vec, const float* __restrict__ Q, int du, int64_t N,
                                                         const int64_t* __restrict__ rows, const int* __restrict__ iscores,
                                                         int k_scan, uint64_t* __restrict__ keys, int* n_valid, int* s_cut) {
  constexpr int PER = D / 16;   // floats per lane
  constexpr int UNR = 4;
  __shared__ int s_cnt, s_min;
  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, l16 = tid & 15, grp = tid >> 4;
  if (tid == 0) { s_cnt = 0; s_min = 0x7FFFFFFF; }
  float qv[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) {
    const int c = l16 * PER + j;
    qv[j] = c < du ? Q[q * du + c] : 0.f;
  }
  const int64_t* my_rows = rows + q * k_scan;
  const int* my_is = iscores + q * k_scan;
  uint64_t* my_keys = keys + q * k_scan;
  int cnt = 0, smin = 0x7FFFFFFF;
  __syncthreads();
  for (int base = 0; base < k_scan; base += 16 * UNR) {
    int64_t row[UNR];
    float x[UNR][PER];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int i = base + 16 * u + grp;
      int64_t r = i < k_scan ? my_rows[i] : -1;
      if (r >= N) r = -1;
      row[u] = r;
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) sq8_load_lane<PER>(vec + (size_t)(row[u] >= 0 ? row[u] : 0) * D + l16 * PER, x[u]);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int i = base + 16 * u + grp;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < PER; ++j) s = fmaf(qv[j], x[u][j], s);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (l16 == 0 && i < k_scan) {
        if (row[u] >= 0) {
          my_keys[i] = make_key(s + 0.f, (uint32_t)row[u]);
          ++cnt;
          const int sv = my_is[i];
          smin = sv < smin ? sv : smin;
        } else {
          my_keys[i] = 0ull;
        }
      }
    }
  }
  if (l16 == 0 && cnt > 0) { atomicAdd(&s_cnt, cnt); atomicMin(&s_min, smin); }
  __syncthreads();
  if (tid == 0) { n_valid[q] = s_cnt; s_cut[q] = s_cnt > 0 ? s_min : 0; }
}

// The certificate, one workgroup of 128 threads per query: thread j forms the five terms of column j, threads 0 .. 4 add
// one array each in ascending j, thread 0 finishes.  All f64; every product of two f32 (or an f32 and an integer below
// 2^16) is exact there.
__global__ __launch_bounds__(128) void sq8_cert_kernel(const float* __restrict__ Q, int du, int dk, int dpad,
                                                       const float* __restrict__ centre, const float* __restrict__ scale,
                                                       const double* __restrict__ ref_e, const double* __restrict__ ref_a,
                                                       const int8_t* __restrict__ qhi, const int8_t* __restrict__ qlo,
                                                       const float* __restrict__ qt, const double* __restrict__ qb,
                                                       const int* __restrict__ n_valid, const int* __restrict__ s_cut,
                                                       const float* __restrict__ out_scores, int k, int k_scan,
                                                       uint8_t* out_cert, double* out_bound) {
  __shared__ double term[5][128];
  __shared__ double sum[5];
  const int64_t q = blockIdx.x;
  const int j = threadIdx.x;
  const double t = (double)qt[q];
  double e1 = 0.0, e2 = 0.0, ta = 0.0, tm = 0.0, tw = 0.0;
  if (j < du) {
    const double x = (double)Q[q * du + j], ax = fabs(x);
    const double n = (double)(256 * (int)qhi[q * dpad + j] + (int)qlo[q * dpad + j]);
    const double tn = t * n;                         // exact
    e1 = ax * ref_e[j];
    e2 = fabs(x * (double)scale[j] - tn);            // the product is exact, the difference rounds once
    ta = ax * ref_a[j];
    tm = fabs(x * (double)centre[j]);                // exact
    tw = fabs(tn);
  }
  term[0][j] = e1; term[1][j] = e2; term[2][j] = ta; term[3][j] = tm; term[4][j] = tw;
  __syncthreads();
  if (j < 5) {
    double s = 0.0;
    for (int i = 0; i < du; ++i) s += term[j][i];
    sum[j] = s;
  }
  __syncthreads();
  if (j != 0) return;
  const double u = (double)dk * 0x1p-24;
  const double gamma = u / (1.0 - u);
  const double E1 = sum[0];
  const double E2 = 127.0 * sum[1];
  const double E3 = gamma * sum[2];
  const double W = 127.0 * sum[4];
  const double mag = (((sum[3] + W) + sum[2]) + E1) + E2;
  const double slack = 0x1p-44 * mag + (double)dk * 0x1p-126;
  const double bound = ((E1 + E2) + E3) + slack;
  if (out_bound) out_bound[q] = bound;
  const int nv = n_valid[q];
  uint8_t cert = 1;
  if (nv >= k_scan) {
    const double U = (qb[q] + t * (double)s_cut[q]) + bound;
    cert = (double)out_scores[q * k + (k - 1)] > U ? 1 : 0;
  }
  out_cert[q] = cert;
}

int sq8_search_refined(Sq8Index* h, const float* Q, int64_t nq, int k, int k_scan, int mode, float* out_s, int64_t* out_r,
                       uint8_t* out_cert, double* out_bound, hipStream_t st, const uint32_t* pred = nullptr, int pred_stride = 0,
                       const SeenArgs* seen = nullptr) {
  const int64_t ch = std::max<int64_t>(1, std::min<int64_t>(nq, (1ll << 24) / k_scan));   // stage-1 slots per pass: 2^24
  RCCHK(h->rs.reserve(ch * k_scan)); RCCHK(h->rr.reserve(ch * k_scan)); RCCHK(h->ri.reserve(ch * k_scan));
  RCCHK(h->rkeys.reserve(ch * k_scan)); RCCHK(h->rnv.reserve(ch)); RCCHK(h->rcut.reserve(ch));
  const int64_t* id_map = h->id_map;
  for (int64_t q0 = 0; q0 < nq; q0 += ch) {
    const int64_t n = std::min(ch, nq - q0);
    const float* Qc = Q + q0 * h->du;
    h->id_map = nullptr;   // stage 1 hands on rows; the map is applied after the select
    const int rc = sq8_search(h, Qc, n, k_scan, mode, h->rs.p, h->rr.p, h->ri.p, st, pred ? pred + q0 * pred_stride : nullptr,
                              pred_stride, seen, q0);
    h->id_map = id_map;
    RCCHK(rc);
    RCCHK(dispatch_d(h->dk, [&](auto D) {
      hipLaunchKernelGGL((sq8_refine_kernel<decltype(D)::value>), dim3((unsigned)n), dim3(256), 0, st, h->vec, Qc, h->du, h->N, h->rr.p,
                         h->ri.p, k_scan, h->rkeys.p, h->rnv.p, h->rcut.p);
    }));
    RCCHK(check_launch("sq8 refine"));
    FinArgs f;
    memset(&f, 0, sizeof(f));
    f.nq = n; f.k = k; f.count = nullptr; f.cand = h->rkeys.p; f.cap = k_scan; f.mode = 0; f.out_scores = out_s + q0 * k;
    f.out_rows = out_r + q0 * k; f.id_map = id_map;
    RCCHK(launch_finalize(f, (unsigned)n, st));
    // (stage 1 left this pass's limbs, t and b in the handle's scratch)
    hipLaunchKernelGGL(sq8_cert_kernel, dim3((unsigned)n), dim3(128), 0, st, Qc, h->du, h->dk, h->dpad, h->centre, h->scale, h->ref_e,
                       h->ref_a, h->qhi.p, h->qlo.p, h->qt.p, h->qb.p, h->rnv.p, h->rcut.p, out_s + q0 * k, k, k_scan, out_cert + q0,
                       out_bound ? out_bound + q0 : nullptr);
    RCCHK(check_launch("sq8 certificate"));
  }
  return RIHIP_OK;
}

int sq8_attach(Sq8Index* h, const IpIndex* src, hipStream_t st) {
  RIHIP_REQUIRE(src->N == h->N && src->d == h->dk && src->du == h->du, RIHIP_ERR_STATE,
                "sq8_refine_attach_vectors: the source holds %lld rows of width %d, the index %lld of width %d", (long long)src->N,
                src->du, (long long)h->N, h->du);
  if (src->ivf) {
    RIHIP_REQUIRE(src->row_ids && src->nlist == h->nlist && src->Np == h->Np && src->list_len == h->list_len, RIHIP_ERR_STATE,
                  "sq8_refine_attach_vectors: the source's lists are not the lists the index was encoded from");
  } else {
    RIHIP_REQUIRE(h->nlist == 1 && h->Np == (h->N + TR - 1) / TR * TR, RIHIP_ERR_STATE,
                  "sq8_refine_attach_vectors: a flat source, but the index was encoded from %d lists", h->nlist);
  }
  const int64_t n_src = src->ivf ? src->Np : src->N;
  const int dk = h->dk;
  const int nb = (int)std::min<int64_t>(1024, (n_src + 255) / 256);
  int* flag = nullptr; float* vec = nullptr; double* e = nullptr; double* a = nullptr; double* part = nullptr;
  int8_t* decoded = nullptr;   // a PQ handle: its decoded code matrix, a transient Np * dpad bytes
  auto work = [&]() -> int {
    if (!h->codes) RCCHK(pq_decode_all(h, &decoded, st));
    const int8_t* codes = h->codes ? h->codes : decoded;
    HIPCHK(hipMalloc((void**)&flag, sizeof(int)));
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), st));
    hipLaunchKernelGGL(sq8_rows_differ_kernel, dim3((unsigned)((h->Np + 255) / 256)), dim3(256), 0, st, h->row_ids,
                       src->ivf ? src->row_ids : nullptr, h->N, h->Np, flag);
    int differ = 0;
    HIPCHK(hipMemcpyAsync(&differ, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    RIHIP_REQUIRE(!differ, RIHIP_ERR_STATE, "sq8_refine_attach_vectors: the source's rows are in another order than the index's");
    HIPCHK(hipMalloc((void**)&vec, sizeof(float) * (size_t)h->N * dk));
    HIPCHK(hipMalloc((void**)&e, sizeof(double) * dk));
    HIPCHK(hipMalloc((void**)&a, sizeof(double) * dk));
    HIPCHK(hipMalloc((void**)&part, sizeof(double) * (size_t)nb * 2 * dk));
    const int64_t nthr = n_src * (dk / 4);
    hipLaunchKernelGGL(sq8_scatter_rows_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, src->X, h->row_ids, n_src, dk, vec);
    hipLaunchKernelGGL(sq8_refine_range_part_kernel, dim3(nb), dim3(256), 0, st, src->X, codes, h->row_ids, n_src, dk, h->dpad,
                       h->centre, h->scale, part);
    hipLaunchKernelGGL(sq8_refine_range_final_kernel, dim3(1), dim3(128), 0, st, part, nb, dk, e, a);
    RCCHK(check_launch("sq8 attach vectors"));
    HIPCHK(hipStreamSynchronize(st));   // the source may be dropped as soon as the call returns
    return RIHIP_OK;
  };
  const int rc = work();
  hipFree(flag); hipFree(part); hipFree(decoded);
  if (rc) { hipFree(vec); hipFree(e); hipFree(a); return rc; }   // the handle is as it was
  drop_vectors(h);
  h->vec = vec; h->ref_e = e; h->ref_a = a;
  return RIHIP_OK;
}

}  // namespace

// ------------------------------------------------ C ABI --------------------------------------------------------------
extern "C" int rihip_sq8_index_from_ip_index(void* ip_handle, const float* centre, const float* scale, void** handle, void* stream) {
  const IpIndex* src = (const IpIndex*)ip_handle;
  RIHIP_REQUIRE(src && handle, RIHIP_ERR_ARG, "sq8_index_from_ip_index: null handle");
  RIHIP_REQUIRE(src->X && src->N > 0, RIHIP_ERR_STATE, "sq8_index_from_ip_index: the source index is empty");
  RIHIP_REQUIRE((centre == nullptr) == (scale == nullptr), RIHIP_ERR_ARG, "sq8_index_from_ip_index: give both centre and scale, or neither");
  Sq8Index* h = new Sq8Index();
  const int rc = sq8_build(h, src, centre, scale, (hipStream_t)stream);
  if (rc) { free_sq8(h); return rc; }
  *handle = h;
  return RIHIP_OK;
}

extern "C" int rihip_sq8_index_destroy(void* handle) {
  if (handle) free_sq8((Sq8Index*)handle);
  return RIHIP_OK;
}

extern "C" int64_t rihip_sq8_index_ntotal(void* handle) { return handle ? ((Sq8Index*)handle)->N : 0; }
extern "C" int rihip_sq8_index_nlist(void* handle) { return handle ? ((Sq8Index*)handle)->nlist : 0; }

extern "C" int rihip_sq8_index_set_nprobe(void* handle, int nprobe) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && nprobe >= 1, RIHIP_ERR_ARG, "sq8_index_set_nprobe: bad arguments");
  h->nprobe = nprobe;
  return RIHIP_OK;
}

extern "C" int rihip_sq8_index_set_id_map(void* handle, const int64_t* item_ids_dev) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h, RIHIP_ERR_ARG, "sq8_index_set_id_map: null handle");
  h->id_map = item_ids_dev;
  return RIHIP_OK;
}

extern "C" int rihip_sq8_index_get_quantizer(void* handle, float* centre, float* scale) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && centre && scale, RIHIP_ERR_ARG, "sq8_index_get_quantizer: bad arguments");
  HIPCHK(hipMemcpy(centre, h->centre, sizeof(float) * h->du, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(scale, h->scale, sizeof(float) * h->du, hipMemcpyDeviceToHost));
  return RIHIP_OK;
}

namespace {
int sq8_rows_out(Sq8Index* h, float* out_x, int8_t* out_c) {
  float* dx = nullptr; int8_t* dc = nullptr;
  const size_t n = (size_t)h->N * h->du;
  if (out_x) HIPCHK(hipMalloc((void**)&dx, sizeof(float) * n));
  if (out_c && hipMalloc((void**)&dc, n) != hipSuccess) { hipFree(dx); rihip_set_error("sq8_index: device allocation failed"); return RIHIP_ERR_HIP; }
  int8_t* decoded = nullptr;   // a PQ handle: its decoded code matrix, a transient Np * dpad bytes
  if (!h->codes && pq_decode_all(h, &decoded, 0) != RIHIP_OK) { hipFree(dx); hipFree(dc); return RIHIP_ERR_HIP; }
  const int64_t tot = h->Np * h->du;
  hipLaunchKernelGGL(sq8_reconstruct_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, h->codes ? h->codes : decoded, h->row_ids, h->Np, h->du,
                     h->dpad, h->centre, h->scale, dx, dc);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && out_x) e = hipMemcpy(out_x, dx, sizeof(float) * n, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out_c) e = hipMemcpy(out_c, dc, n, hipMemcpyDeviceToHost);
  hipFree(dx); hipFree(dc); hipFree(decoded);
  HIPCHK(e);
  return RIHIP_OK;
}
}  // namespace

// ---- what pq.hip builds on (sq8_index.h) ------------------------------------------------------------------------------
namespace rihip_index {
int sq8_build_handle(Sq8Index* h, const IpIndex* src, const float* centre, const float* scale, hipStream_t st) {
  return sq8_build(h, src, centre, scale, st);
}
int sq8_upload_list_layout(Sq8Index* h, hipStream_t st) { return sq8_upload_layout(h, st); }
int64_t sq8_held_bytes(const Sq8Index* h) { return held_bytes(h); }
void sq8_free_handle(Sq8Index* h) { free_sq8(h); }
}  // namespace rihip_index

extern "C" int rihip_sq8_index_get_codes(void* handle, int8_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "sq8_index_get_codes: bad arguments");
  return sq8_rows_out(h, nullptr, out);
}

extern "C" int rihip_sq8_index_reconstruct(void* handle, float* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "sq8_index_reconstruct: bad arguments");
  return sq8_rows_out(h, out, nullptr);
}

extern "C" int rihip_sq8_index_encode_queries(void* handle, const float* Q, int64_t nq, int16_t* out_n, float* out_t, double* out_b,
                                              void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && Q && out_n && out_t && out_b && nq > 0, RIHIP_ERR_ARG, "sq8_index_encode_queries: bad arguments");
  return sq8_transform_queries(h, Q, nq, out_n, out_t, out_b, (hipStream_t)stream);
}

extern "C" int rihip_sq8_index_search(void* handle, const float* Q, int64_t nq, int k, int mode, float* out_scores, int64_t* out_rows,
                                      int32_t* out_iscores, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "sq8_index_search: index is empty");
  RIHIP_REQUIRE(Q && out_scores && out_rows && nq > 0, RIHIP_ERR_ARG, "sq8_index_search: bad arguments");
  RIHIP_REQUIRE(k >= 1 && k <= K_MAX, RIHIP_ERR_ARG, "sq8_index_search: k=%d outside [1,%d]", k, K_MAX);
  RIHIP_REQUIRE(mode >= 0 && mode <= 2, RIHIP_ERR_ARG, "sq8_index_search: mode=%d (0 auto, 1 dense, 2 thresholded)", mode);
  return sq8_search(h, Q, nq, k, mode, out_scores, out_rows, out_iscores, (hipStream_t)stream);
}

// ---- filtered search: per-query tag predicates inside the int8 scan ---------------------------------------------------
extern "C" int rihip_sq8_filter_set_tags(void* handle, const uint32_t* tags_by_row_dev, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "sq8_filter_set_tags: index is empty");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(st));   // (searches in flight still read the old copy)
  drop_tags(h);
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
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "sq8_filter_search: index is empty");
  RIHIP_REQUIRE(h->tags, RIHIP_ERR_STATE, "sq8_filter_search: the index has no tags (rihip_sq8_filter_set_tags)");
  RIHIP_REQUIRE(Q && pred_dev && out_scores && out_rows && nq > 0, RIHIP_ERR_ARG, "sq8_filter_search: bad arguments");
  RIHIP_REQUIRE(pred_stride == 0 || pred_stride == 3, RIHIP_ERR_ARG, "sq8_filter_search: pred_stride=%lld (0 or 3)", (long long)pred_stride);
  RIHIP_REQUIRE(k >= 1 && k <= K_MAX, RIHIP_ERR_ARG, "sq8_filter_search: k=%d outside [1,%d]", k, K_MAX);
  RIHIP_REQUIRE(mode >= 0 && mode <= 2, RIHIP_ERR_ARG, "sq8_filter_search: mode=%d (0 auto, 1 dense, 2 thresholded)", mode);
  return sq8_search(h, Q, nq, k, mode, out_scores, out_rows, out_iscores, (hipStream_t)stream, pred_dev, (int)pred_stride);
}

extern "C" int rihip_sq8_refine_search_filtered(void* handle, const float* Q, int64_t nq, int k, int k_scan, int mode,
                                                const uint32_t* pred_dev, int64_t pred_stride, float* out_scores, int64_t* out_rows,
                                                uint8_t* out_cert, double* out_bound, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "sq8_refine_search_filtered: index is empty");
  RIHIP_REQUIRE(h->vec, RIHIP_ERR_STATE, "sq8_refine_search_filtered: no vectors attached (rihip_sq8_refine_attach_vectors)");
  RIHIP_REQUIRE(h->tags, RIHIP_ERR_STATE, "sq8_refine_search_filtered: the index has no tags (rihip_sq8_filter_set_tags)");
  RIHIP_REQUIRE(Q && pred_dev && out_scores && out_rows && out_cert && nq > 0, RIHIP_ERR_ARG, "sq8_refine_search_filtered: bad arguments");
  RIHIP_REQUIRE(pred_stride == 0 || pred_stride == 3, RIHIP_ERR_ARG, "sq8_refine_search_filtered: pred_stride=%lld (0 or 3)", (long long)pred_stride);
  RIHIP_REQUIRE(k >= 1 && k <= k_scan && k_scan <= K_MAX, RIHIP_ERR_ARG,
                "sq8_refine_search_filtered: k=%d, k_scan=%d (1 <= k <= k_scan <= %d)", k, k_scan, K_MAX);
  RIHIP_REQUIRE(mode >= 0 && mode <= 2, RIHIP_ERR_ARG, "sq8_refine_search_filtered: mode=%d (0 auto, 1 dense, 2 thresholded)", mode);
  return sq8_search_refined(h, Q, nq, k, k_scan, mode, out_scores, out_rows, out_cert, out_bound, (hipStream_t)stream, pred_dev,
                            (int)pred_stride);
}

// ---- seen-item exclusion inside the int8 scan ---------------------------------------------------------------------
namespace {
int sq8_check_excluding(const char* who, Sq8Index* h, const float* Q, int64_t nq, const int64_t* seen_offsets, int64_t n_seen_rows,
                        const int32_t* seen_items, const int32_t* row_of, int64_t n_ids, const uint32_t* pred_dev,
                        int64_t pred_stride, int mode) {
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "%s: index is empty", who);
  RIHIP_REQUIRE(!pred_dev || h->tags, RIHIP_ERR_STATE, "%s: the index has no tags (rihip_sq8_filter_set_tags)", who);
  RIHIP_REQUIRE(Q && nq > 0, RIHIP_ERR_ARG, "%s: bad arguments", who);
  RIHIP_REQUIRE(seen_offsets && seen_items && n_seen_rows >= 0, RIHIP_ERR_ARG, "%s: bad seen lists", who);
  RIHIP_REQUIRE(row_of && n_ids > 0, RIHIP_ERR_ARG, "%s: no row_of table", who);
  RIHIP_REQUIRE(pred_stride == 0 || pred_stride == 3, RIHIP_ERR_ARG, "%s: pred_stride=%lld (0 or 3)", who, (long long)pred_stride);
  RIHIP_REQUIRE(mode >= 0 && mode <= 2, RIHIP_ERR_ARG, "%s: mode=%d (0 auto, 1 dense, 2 thresholded)", who, mode);
  return RIHIP_OK;
}
}  // namespace

extern "C" int rihip_sq8_exclude_search(void* handle, const float* Q, int64_t nq, int k, int mode, const int64_t* user_ids,
                                        const int64_t* seen_offsets, int64_t n_seen_rows, const int32_t* seen_items,
                                        const int32_t* row_of, int64_t n_ids, const uint32_t* pred_dev, int64_t pred_stride,
                                        float* out_scores, int64_t* out_rows, int32_t* out_iscores, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RCCHK(sq8_check_excluding("sq8_exclude_search", h, Q, nq, seen_offsets, n_seen_rows, seen_items, row_of, n_ids, pred_dev,
                            pred_stride, mode));
  RIHIP_REQUIRE(out_scores && out_rows, RIHIP_ERR_ARG, "sq8_exclude_search: null output");
  RIHIP_REQUIRE(k >= 1 && k <= K_MAX, RIHIP_ERR_ARG, "sq8_exclude_search: k=%d outside [1,%d]", k, K_MAX);
  const SeenArgs sn{user_ids, seen_offsets, n_seen_rows, seen_items, row_of, n_ids};
  return sq8_search(h, Q, nq, k, mode, out_scores, out_rows, out_iscores, (hipStream_t)stream, pred_dev, (int)pred_stride, &sn, 0);
}

extern "C" int rihip_sq8_refine_search_excluding(void* handle, const float* Q, int64_t nq, int k, int k_scan, int mode,
                                                 const int64_t* user_ids, const int64_t* seen_offsets, int64_t n_seen_rows,
                                                 const int32_t* seen_items, const int32_t* row_of, int64_t n_ids,
                                                 const uint32_t* pred_dev, int64_t pred_stride, float* out_scores,
                                                 int64_t* out_rows, uint8_t* out_cert, double* out_bound, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RCCHK(sq8_check_excluding("sq8_refine_search_excluding", h, Q, nq, seen_offsets, n_seen_rows, seen_items, row_of, n_ids, pred_dev,
                            pred_stride, mode));
  RIHIP_REQUIRE(h->vec, RIHIP_ERR_STATE, "sq8_refine_search_excluding: no vectors attached (rihip_sq8_refine_attach_vectors)");
  RIHIP_REQUIRE(out_scores && out_rows && out_cert, RIHIP_ERR_ARG, "sq8_refine_search_excluding: null output");
  RIHIP_REQUIRE(k >= 1 && k <= k_scan && k_scan <= K_MAX, RIHIP_ERR_ARG,
                "sq8_refine_search_excluding: k=%d, k_scan=%d (1 <= k <= k_scan <= %d)", k, k_scan, K_MAX);
  const SeenArgs sn{user_ids, seen_offsets, n_seen_rows, seen_items, row_of, n_ids};
  return sq8_search_refined(h, Q, nq, k, k_scan, mode, out_scores, out_rows, out_cert, out_bound, (hipStream_t)stream, pred_dev,
                            (int)pred_stride, &sn);
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

extern "C" int rihip_sq8_refine_attach_vectors(void* handle, void* ip_handle, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  const IpIndex* src = (const IpIndex*)ip_handle;
  RIHIP_REQUIRE(h && src, RIHIP_ERR_ARG, "sq8_refine_attach_vectors: null handle");
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "sq8_refine_attach_vectors: index is empty");
  RIHIP_REQUIRE(src->X && src->N > 0, RIHIP_ERR_STATE, "sq8_refine_attach_vectors: the source index is empty");
  return sq8_attach(h, src, (hipStream_t)stream);
}

extern "C" int rihip_sq8_refine_drop_vectors(void* handle) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h, RIHIP_ERR_ARG, "sq8_refine_drop_vectors: null handle");
  HIPCHK(hipDeviceSynchronize());   // a refined search may still be reading them
  drop_vectors(h);
  return RIHIP_OK;
}

extern "C" int rihip_sq8_refine_has_vectors(void* handle) { return handle && ((Sq8Index*)handle)->vec ? 1 : 0; }

extern "C" int rihip_sq8_refine_get_ranges(void* handle, double* e, double* a) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && e && a, RIHIP_ERR_ARG, "sq8_refine_get_ranges: bad arguments");
  RIHIP_REQUIRE(h->vec, RIHIP_ERR_STATE, "sq8_refine_get_ranges: no vectors attached");
  HIPCHK(hipMemcpy(e, h->ref_e, sizeof(double) * h->du, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(a, h->ref_a, sizeof(double) * h->du, hipMemcpyDeviceToHost));
  return RIHIP_OK;
}

extern "C" int rihip_sq8_refine_search(void* handle, const float* Q, int64_t nq, int k, int k_scan, int mode, float* out_scores,
                                              int64_t* out_rows, uint8_t* out_cert, double* out_bound, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(sq8_has_storage(h) && h->N > 0, RIHIP_ERR_STATE, "sq8_refine_search: index is empty");
  RIHIP_REQUIRE(h->vec, RIHIP_ERR_STATE, "sq8_refine_search: no vectors attached (rihip_sq8_refine_attach_vectors)");
  RIHIP_REQUIRE(Q && out_scores && out_rows && out_cert && nq > 0, RIHIP_ERR_ARG, "sq8_refine_search: bad arguments");
  RIHIP_REQUIRE(k >= 1 && k <= k_scan && k_scan <= K_MAX, RIHIP_ERR_ARG, "sq8_refine_search: k=%d, k_scan=%d (1 <= k <= k_scan <= %d)",
                k, k_scan, K_MAX);
  RIHIP_REQUIRE(mode >= 0 && mode <= 2, RIHIP_ERR_ARG, "sq8_refine_search: mode=%d (0 auto, 1 dense, 2 thresholded)", mode);
  return sq8_search_refined(h, Q, nq, k, k_scan, mode, out_scores, out_rows, out_cert, out_bound, (hipStream_t)stream);
}

extern "C" int rihip_sq8_index_stats(void* handle, int64_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "sq8_index_stats: bad arguments");
  out[0] = h->stats[0]; out[1] = h->stats[1]; out[2] = held_bytes(h);
  return RIHIP_OK;
}

// File: "RIHIPSQ8", int64 header {version 1, du, dk, dpad, N, Np, nlist, nprobe}, centre f32[dpad], scale f32[dpad],
// centroids f32[nlist, dk], list lengths int64[nlist], row ids int64[Np], codes int8[Np, dpad]
extern "C" int rihip_sq8_index_save(void* handle, const char* path) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && path, RIHIP_ERR_ARG, "sq8_index_save: bad arguments");
  RIHIP_REQUIRE(!h->pq_codes, RIHIP_ERR_STATE, "sq8_index_save: a PQ index has a file format of its own (rihip_pq_index_save)");
  RIHIP_REQUIRE(h->codes, RIHIP_ERR_STATE, "sq8_index_save: index is empty");
  std::vector<float> m(h->dpad), s(h->dpad), C((size_t)h->nlist * h->dk);
  std::vector<int64_t> rid((size_t)h->Np);
  std::vector<int8_t> codes((size_t)h->Np * h->dpad);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(m.data(), h->centre, sizeof(float) * m.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(s.data(), h->scale, sizeof(float) * s.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(C.data(), h->C, sizeof(float) * C.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rid.data(), h->row_ids, sizeof(int64_t) * rid.size(), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(codes.data(), h->codes, codes.size(), hipMemcpyDeviceToHost));
  FILE* f = fopen(path, "wb");
  RIHIP_REQUIRE(f, RIHIP_ERR_IO, "sq8_index_save: cannot open %s", path);
  const int64_t hdr[8] = {1, h->du, h->dk, h->dpad, h->N, h->Np, h->nlist, h->nprobe};
  bool ok = fwrite("RIHIPSQ8", 1, 8, f) == 8 && fwrite(hdr, sizeof(int64_t), 8, f) == 8 &&
            fwrite(m.data(), sizeof(float), m.size(), f) == m.size() && fwrite(s.data(), sizeof(float), s.size(), f) == s.size() &&
            fwrite(C.data(), sizeof(float), C.size(), f) == C.size() &&
            fwrite(h->list_len.data(), sizeof(int64_t), h->nlist, f) == (size_t)h->nlist &&
            fwrite(rid.data(), sizeof(int64_t), rid.size(), f) == rid.size() && fwrite(codes.data(), 1, codes.size(), f) == codes.size();
  ok = (fclose(f) == 0) && ok;
  RIHIP_REQUIRE(ok, RIHIP_ERR_IO, "sq8_index_save: short write to %s", path);
  return RIHIP_OK;
}

extern "C" int rihip_sq8_index_load(const char* path, void** handle) {
  RIHIP_REQUIRE(path && handle, RIHIP_ERR_ARG, "sq8_index_load: bad arguments");
  FILE* f = fopen(path, "rb");
  RIHIP_REQUIRE(f, RIHIP_ERR_IO, "sq8_index_load: cannot open %s", path);
  char magic[8]; int64_t hdr[8];
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "RIHIPSQ8", 8) != 0 || fread(hdr, sizeof(int64_t), 8, f) != 8 || hdr[0] != 1) {
    fclose(f); rihip_set_error("sq8_index_load: %s is not an SQ8 index file (magic / version)", path); return RIHIP_ERR_IO;
  }
  const int64_t du = hdr[1], dk = hdr[2], dpad = hdr[3], N = hdr[4], Np = hdr[5], nlist = hdr[6], nprobe = hdr[7];
  const bool hdr_ok = du >= 1 && du <= 128 && dk == (du <= 32 ? 32 : (du <= 64 ? 64 : 128)) && dpad == (dk <= 64 ? 64 : 128) &&
                      N >= 1 && N < (1ll << 31) && nlist >= 1 && nlist <= NLIST_MAX && nprobe >= 1 && nprobe < (1ll << 31) &&
                      Np >= N && Np % TR == 0 && Np <= N + (int64_t)TR * nlist;
  int64_t expect = 0, have = -1;
  if (hdr_ok) {
    expect = 8 + 64 + 8 * dpad + 4 * nlist * dk + 8 * nlist + 8 * Np + Np * dpad;
    if (fseek(f, 0, SEEK_END) == 0) have = (int64_t)ftell(f);
    if (fseek(f, 72, SEEK_SET) != 0) have = -1;
  }
  if (!hdr_ok || have != expect) {
    fclose(f);
    rihip_set_error("sq8_index_load: %s: %s", path, hdr_ok ? "file size does not match its header (truncated?)" : "header field out of range");
    return RIHIP_ERR_IO;
  }
  std::vector<float> m(dpad), s(dpad), C((size_t)nlist * dk);
  std::vector<int64_t> ll(nlist), rid((size_t)Np);
  std::vector<int8_t> codes((size_t)Np * dpad);
  bool ok = fread(m.data(), sizeof(float), m.size(), f) == m.size() && fread(s.data(), sizeof(float), s.size(), f) == s.size() &&
            fread(C.data(), sizeof(float), C.size(), f) == C.size() && fread(ll.data(), sizeof(int64_t), nlist, f) == (size_t)nlist &&
            fread(rid.data(), sizeof(int64_t), rid.size(), f) == rid.size() && fread(codes.data(), 1, codes.size(), f) == codes.size();
  fclose(f);
  RIHIP_REQUIRE(ok, RIHIP_ERR_IO, "sq8_index_load: short read from %s", path);
  int64_t tot = 0, ptot = 0;
  for (int64_t c = 0; c < nlist; ++c) {
    RIHIP_REQUIRE(ll[c] >= 0 && ll[c] <= N, RIHIP_ERR_IO, "sq8_index_load: %s: list %lld has length %lld", path, (long long)c, (long long)ll[c]);
    tot += ll[c]; ptot += (ll[c] + TR - 1) / TR * TR;
  }
  RIHIP_REQUIRE(tot == N && ptot == Np, RIHIP_ERR_IO, "sq8_index_load: %s: list lengths do not add up to the header's row counts", path);
  for (int64_t p = 0; p < Np; ++p)
    RIHIP_REQUIRE(rid[p] >= -1 && rid[p] < N, RIHIP_ERR_IO, "sq8_index_load: %s: row id %lld out of range", path, (long long)rid[p]);
  for (int64_t j = 0; j < dpad; ++j)
    RIHIP_REQUIRE(isfinite(m[j]) && isfinite(s[j]) && s[j] > 0.f, RIHIP_ERR_IO, "sq8_index_load: %s: quantiser column %lld is not finite", path, (long long)j);
  Sq8Index* h = new Sq8Index();
  h->du = (int)du; h->dk = (int)dk; h->dpad = (int)dpad; h->N = N; h->Np = Np; h->nlist = (int)nlist; h->nprobe = (int)nprobe;
  h->list_len = ll;
  auto fill = [&]() -> int {
    RCCHK(sq8_upload_layout(h, 0));
    HIPCHK(hipMalloc((void**)&h->row_ids, sizeof(int64_t) * rid.size()));
    HIPCHK(hipMalloc((void**)&h->C, sizeof(float) * C.size()));
    HIPCHK(hipMalloc((void**)&h->codes, codes.size()));
    HIPCHK(hipMalloc((void**)&h->centre, sizeof(float) * dpad));
    HIPCHK(hipMalloc((void**)&h->scale, sizeof(float) * dpad));
    HIPCHK(hipMemcpy(h->row_ids, rid.data(), sizeof(int64_t) * rid.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->C, C.data(), sizeof(float) * C.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->codes, codes.data(), codes.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->centre, m.data(), sizeof(float) * dpad, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->scale, s.data(), sizeof(float) * dpad, hipMemcpyHostToDevice));
    return RIHIP_OK;
  };
  const int rc = fill();
  if (rc) { free_sq8(h); return rc; }
  *handle = h;
  return RIHIP_OK;
}
