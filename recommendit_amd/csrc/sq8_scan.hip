// The list-major int8 MFMA scan of the 8-bit index: sq8_scan_lm_kernel and its launcher.  The only unit that instantiates
// the kernel (2 widths x 4 filter modes x 3 sources, and the two PQ sources once more with residual scores); sq8.hip drives it.
#pragma clang fp contract(off)   // as every unit of the 8-bit index (sq8_index.h)
#include "common.h"

#include <type_traits>

#include "search_kernels.h"
#include "search_keys.h"
#include "sq8_scan.h"

using namespace rihip_index;

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

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
//
// RES (PQ instantiations only): the codebooks hold residuals against the list's centroid code K_l, so a row's score is
// T[q, l] + the gathered dot product.  The work item is one list and its lane one query: the lane loads its pair's T once,
// next to thr, and adds it wherever a score is formed.  Nothing else changes; with RES false the term is compiled out.
template <int DP, int FM = FM_NONE, int PQ = 0, bool RES = false>
__global__ __launch_bounds__(256, 2) void sq8_scan_lm_kernel(Sq8LmArgs a) {
  static_assert(!RES || PQ != 0, "residual scores exist on product-quantised storage only");
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
  int pt = 0;
  if constexpr (RES) pt = a.pair_t[pair];
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
  auto score = [&](int sh, int sl) -> int {
    if constexpr (RES) return sh * 256 + sl + pt;
    else return sh * 256 + sl;
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
            my_dense[sl] = (rr < n_ok && row_ok(r)) ? sq8_key(score(ah[r], al[r]), a.dense_ids ? (uint32_t)a.row_ids[p0 + t_row0 + rr] : 0u) : 0ull;
        }
      } else {
        unsigned hits = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (acc_row(r, lane) < n_ok && score(ah[r], al[r]) >= thr && row_ok(r)) hits |= (1u << r);
        if (hits) {
          int pos = atomicAdd(&a.count[q * a.count_stride], __popc(hits));
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            if (hits & (1u << r)) {
              const int64_t v = p0 + t_row0 + acc_row(r, lane);
              if (pos < a.cap) my_cand[pos] = sq8_key(score(ah[r], al[r]), (uint32_t)a.row_ids[v]);
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

}  // namespace

namespace rihip_index {

void sq8_launch_scan(int dpad, int fm, int pq_dsub, bool residual, dim3 grid, hipStream_t st, const Sq8LmArgs& x) {
  auto go = [&](auto FMv, auto PQv) {
    constexpr int FM = decltype(FMv)::value, PQ = decltype(PQv)::value;
    if constexpr (PQ != 0) {
      if (residual) {
        if (dpad == 64) hipLaunchKernelGGL((sq8_scan_lm_kernel<64, FM, PQ, true>), grid, dim3(256), 0, st, x);
        else hipLaunchKernelGGL((sq8_scan_lm_kernel<128, FM, PQ, true>), grid, dim3(256), 0, st, x);
        return;
      }
    }
    if (dpad == 64) hipLaunchKernelGGL((sq8_scan_lm_kernel<64, FM, PQ>), grid, dim3(256), 0, st, x);
    else hipLaunchKernelGGL((sq8_scan_lm_kernel<128, FM, PQ>), grid, dim3(256), 0, st, x);
  };
  auto by_fm = [&](auto PQv) {
    if (fm == FM_TAGS_MASK) go(std::integral_constant<int, FM_TAGS_MASK>{}, PQv);
    else if (fm == FM_MASK) go(std::integral_constant<int, FM_MASK>{}, PQv);
    else if (fm == FM_TAGS) go(std::integral_constant<int, FM_TAGS>{}, PQv);
    else go(std::integral_constant<int, FM_NONE>{}, PQv);
  };
  if (pq_dsub == 8) by_fm(std::integral_constant<int, 8>{});
  else if (pq_dsub == 16) by_fm(std::integral_constant<int, 16>{});
  else by_fm(std::integral_constant<int, 0>{});
}

}  // namespace rihip_index
