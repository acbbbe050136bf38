// IVF search of the inner-product index: coarse quantizer, probe plan and the list-major scan.
// faiss IndexIVFFlat.search (reference src/models/faiss_index.py:113,:145): coarse top-nprobe lists per query by inner
// product with the centroids, then an exact scan of the probed lists only.  Batched the list-major way: the
// (query, probed list) pairs are grouped by LIST, and every wave takes (one list, 32 of the queries that probe it,
// a range of the list's 32-row tiles): the 32 queries sit in registers (MFMA B operand), the tile rows are loaded
// straight into the MFMA A-operand registers (no LDS, no barrier: waves are independent, the plan decides how many of
// them a list gets), exact-f32 MFMA, scores >= thr[q] appended to the query's candidate list.  Work = nprobe/nlist of
// the brute force, whatever the batch size; rows of a list are re-read by its query groups from L2.
#include "search_kernels.h"
#include "search_keys.h"

using namespace rihip_index;

namespace {

// coarse scores cs[q, c] = <Q[q], C[c]> on exact-f32 MFMA (4 waves x 32 register-stationary queries, centroid tiles
// of 32 through LDS) -- the IndexFlatIP quantizer
template <int D>
__device__ __forceinline__ void ivf_coarse_body(const float* __restrict__ Q, int64_t nq, const float* __restrict__ C,
                                                int nlist, float* cs, int64_t block) {
  constexpr int LDC = D + 4, KB = D / 8;
  constexpr int NV = (32 * (D / 4) + 255) / 256;
  __shared__ __attribute__((aligned(16))) float Cs[32 * LDC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r31 = lane & 31, hh = lane >> 5;
  const int64_t q = block * 128 + w * 32 + r31;
  const int64_t qc = q < nq ? q : nq - 1;
  f32x4 xr[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) xr[kb] = *reinterpret_cast<const f32x4*>(&Q[qc * D + kb * 8 + 4 * hh]);
  const int ntile = (nlist + 31) / 32;
  for (int t = 0; t < ntile; ++t) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      const int r = idx / (D / 4), c4 = idx % (D / 4);
      if (idx < 32 * (D / 4)) {
        const int c = t * 32 + r;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (c < nlist) v = reinterpret_cast<const f32x4*>(C + (size_t)c * D)[c4];
        *reinterpret_cast<f32x4*>(&Cs[r * LDC + c4 * 4]) = v;
      }
    }
    __syncthreads();
    f32x16 acc = zero16();
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(&Cs[r31 * LDC + kb * 8 + 4 * hh]);
      acc = mfma32(av.x, xr[kb].x, acc);
      acc = mfma32(av.y, xr[kb].y, acc);
      acc = mfma32(av.z, xr[kb].z, acc);
      acc = mfma32(av.w, xr[kb].w, acc);
    }
    if (q < nq) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = t * 32 + acc_row(r, lane);
        if (c < nlist) cs[(size_t)q * nlist + c] = acc[r];
      }
    }
  }
}
template <int D>
__global__ __launch_bounds__(256, 2) void ivf_coarse_kernel(const float* __restrict__ Q, int64_t nq,
                                                            const float* __restrict__ C, int nlist, float* cs) {
  ivf_coarse_body<D>(Q, nq, C, nlist, cs, blockIdx.x);
}

// top-nprobe lists of each query (ties -> lowest list id), one wave per query; counts the probes of every list
__device__ __forceinline__ void ivf_select_body(const float* __restrict__ cs, int64_t nq, int nlist, int nprobe,
                                                int* probe_list, int* list_cnt, float* sc, int64_t block) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t q = block * 4 + w;
  if (q >= nq) return;
  float* my = sc + (size_t)w * nlist;
  for (int c = lane; c < nlist; c += 64) my[c] = cs[(size_t)q * nlist + c];
  __builtin_amdgcn_wave_barrier();
  for (int p = 0; p < nprobe; ++p) {
    float best = -INFINITY;
    int bi = 0x7fffffff;
    for (int c = lane; c < nlist; c += 64) {
      const float v = my[c];
      if (v > best || (v == best && c < bi)) { best = v; bi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (bi == 0x7fffffff) bi = -1;  // fewer than nprobe lists (or only NaN scores left)
    if (lane == 0) {
      probe_list[(size_t)q * nprobe + p] = bi;
      if (bi >= 0) { atomicAdd(&list_cnt[bi], 1); my[bi] = -INFINITY; }
    }
    __builtin_amdgcn_wave_barrier();
  }
}
__global__ __launch_bounds__(256) void ivf_select_kernel(const float* __restrict__ cs, int64_t nq, int nlist, int nprobe,
                                                         int* probe_list, int* list_cnt) {
  extern __shared__ float sc[];  // [4][nlist]
  ivf_select_body(cs, nq, nlist, nprobe, probe_list, list_cnt, sc, blockIdx.x);
}

// one workgroup: slot offsets of the lists, the tile split and the work-item offsets; zeroes the candidate counters
__device__ __forceinline__ void ivf_plan_body(const int* __restrict__ list_cnt, const int64_t* __restrict__ list_poff,
                                              int nlist, int tile_step, int target_items, int* list_qoff,
                                              int* list_cur, int* work_off, int* plan, int* count, int64_t nq) {
  __shared__ int part[256];
  __shared__ int s_total;
  const int tid = threadIdx.x;
  const int per = (nlist + 255) / 256;
  const int c0 = tid * per, c1 = (c0 + per < nlist) ? c0 + per : nlist;
  for (int64_t i = tid; i < nq; i += 256) count[i] = 0;
  // exclusive prefix of `mine` over the 256 threads; s_total = sum.  Wave scans + four wave totals (a serial scan by one
  // thread was 3 x 256 dependent LDS round trips = most of this kernel's 10 us)
  auto block_excl = [&](int mine) -> int {
    const int lane = tid & 63, wv = tid >> 6;
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (lane == 63) part[wv] = incl;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < wv; ++k) base += part[k];
    if (tid == 0) s_total = part[0] + part[1] + part[2] + part[3];
    __syncthreads();
    const int out = base + incl - mine;
    __syncthreads();     // part / s_total are reused by the next call
    return out;
  };
  // pass 1: slots (queries per list) and the total work = sum over (list, 32-query group) of the list's sampled tiles
  int m_sum = 0, g_sum = 0;
  for (int c = c0; c < c1; ++c) {
    const int64_t tiles = (list_poff[c + 1] - list_poff[c]) / TRS;
    const int64_t n_seq = (tiles + tile_step - 1) / tile_step;
    m_sum += list_cnt[c];
    g_sum += ((list_cnt[c] + 31) / 32) * (int)n_seq;
  }
  int q_off = block_excl(m_sum);
  const int m_total = s_total;
  (void)block_excl(g_sum);
  const int total_tiles = s_total;
  // tiles per work item: every item gets about the same number of tiles, whatever the length of its list
  int tpi = (total_tiles + target_items - 1) / (target_items > 0 ? target_items : 1);
  if (tpi < 1) tpi = 1;
  // pass 2: work items
  int w_sum = 0;
  for (int c = c0; c < c1; ++c) {
    const int64_t tiles = (list_poff[c + 1] - list_poff[c]) / TRS;
    const int64_t n_seq = (tiles + tile_step - 1) / tile_step;
    w_sum += ((list_cnt[c] + 31) / 32) * (int)((n_seq + tpi - 1) / tpi);
  }
  int w_off = block_excl(w_sum);
  const int n_work = s_total;
  for (int c = c0; c < c1; ++c) {
    list_qoff[c] = q_off; list_cur[c] = q_off; work_off[c] = w_off;
    q_off += list_cnt[c];
    const int64_t tiles = (list_poff[c + 1] - list_poff[c]) / TRS;
    const int64_t n_seq = (tiles + tile_step - 1) / tile_step;
    w_off += ((list_cnt[c] + 31) / 32) * (int)((n_seq + tpi - 1) / tpi);
  }
  if (tid == 0) { list_qoff[nlist] = m_total; work_off[nlist] = n_work; plan[0] = n_work; plan[1] = tpi; }
}
__global__ __launch_bounds__(256) void ivf_plan_kernel(const int* __restrict__ list_cnt, const int64_t* __restrict__ list_poff,
                                                       int nlist, int tile_step, int target_items, int* list_qoff,
                                                       int* list_cur, int* work_off, int* plan, int* count, int64_t nq) {
  ivf_plan_body(list_cnt, list_poff, nlist, tile_step, target_items, list_qoff, list_cur, work_off, plan, count, nq);
}

__global__ void ivf_scatter_kernel(const int* __restrict__ probe_list, int64_t n_pairs, int nprobe, int* list_cur, int* list_q) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  const int c = probe_list[i];
  if (c >= 0) list_q[atomicAdd(&list_cur[c], 1)] = (int)i;   // the pair index: query = i / nprobe, probe rank = i % nprobe
}

// Small query batches (single requests above all): coarse scores -> probed lists -> plan -> scatter by ONE workgroup in
// one launch instead of a memset and four dependent launches of a few microseconds of work each; the other workgroups of
// the grid zero the dense candidate slots of the unfiltered scan that follows (what was a fifth launch).  The stages
// hand over through global memory: every array is written before the workgroup barrier that precedes its first read.
template <int D>
__global__ __launch_bounds__(256, 2) void ivf_prepare_small_kernel(PrepSmallArgs a) {
  extern __shared__ float sc[];  // [4][nlist]
  const int tid = threadIdx.x;
  if (blockIdx.x > 0) {
    const int64_t stride = (int64_t)(gridDim.x - 1) * 256;
    for (int64_t i = (int64_t)(blockIdx.x - 1) * 256 + tid; i < a.zero_n; i += stride) a.zero_buf[i] = 0ull;
    return;
  }
  for (int c = tid; c < a.nlist; c += 256) a.list_cnt[c] = 0;
  __syncthreads();
  ivf_coarse_body<D>(a.Q, a.nq, a.C, a.nlist, a.cs, 0);      // nq <= 128: one block of the coarse product
  __syncthreads();
  for (int64_t b = 0; b * 4 < a.nq; ++b) ivf_select_body(a.cs, a.nq, a.nlist, a.nprobe, a.probe_list, a.list_cnt, sc, b);
  __syncthreads();
  ivf_plan_body(a.list_cnt, a.list_poff, a.nlist, a.tile_step, a.target_items, a.list_qoff, a.list_cur, a.work_off, a.plan,
                a.count, a.n_count);
  __syncthreads();
  const int64_t n_pairs = a.nq * a.nprobe;
  for (int64_t i = tid; i < n_pairs; i += 256) {
    const int c = a.probe_list[i];
    if (c >= 0) a.list_q[atomicAdd(&a.list_cur[c], 1)] = (int)i;
  }
}

// FILT: the tile's 32 tag words are contiguous in the physical order the handle keeps them in; every lane loads the four
// 16-byte runs of its accumulator rows before the MFMA chain (two addresses per wave and load, in flight under the chain).
// FM (search_keys.h): FM_TAGS as above; FM_TAGS_MASK / FM_MASK add the seen-item mask -- the tile is one aligned word of the
// lane's query, loaded where the tag words are (in flight under the chain); FM_MASK compiles the tag test out, so an
// untagged index is excluded from as well.  FM_NONE and FM_TAGS are the kernels as they were.
template <int D, int FM = FM_NONE>
__global__ __launch_bounds__(256, 2) void ivf_scan_lm_kernel(LmArgs a) {
  constexpr bool FILT = FM == FM_TAGS || FM == FM_TAGS_MASK, XM = FM == FM_TAGS_MASK || FM == FM_MASK;
  constexpr int KB = D / 8, LDX = D + 4;
  constexpr int NL = (TRS * (D / 4)) / 64;  // 16-byte pieces per lane per tile (fully coalesced 1-KiB wave loads)
  // wave-private staging tile: no workgroup barrier anywhere (a wave's LDS operations execute in order)
  __shared__ __attribute__((aligned(16))) float Xs_all[4][TRS * LDX];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r31 = lane & 31, hh = lane >> 5;
  float* Xs = Xs_all[w];
  const int wi = blockIdx.x * 4 + w;
  if (wi >= a.plan[0]) return;  // wave-uniform
  // which list: largest c with work_off[c] <= wi
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
  const int tpi = a.plan[1];                              // tiles per work item
  const int s_c = (int)((n_seq + tpi - 1) / tpi);
  const int grp = rem / s_c, split = rem % s_c;
  const int q0 = a.list_qoff[c], m = a.list_qoff[c + 1] - q0;
  const int slot = grp * 32 + r31;
  const bool q_ok = slot < m;
  const int pair = a.list_q[q0 + (q_ok ? slot : grp * 32)];   // pair = query * nprobe + probe rank
  const int64_t q = pair / a.nprobe;
  const int len = a.list_len[c];
  f32x4 qf[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) qf[kb] = *reinterpret_cast<const f32x4*>(&a.Q[q * D + kb * 8 + 4 * hh]);
  const float thr = a.thr ? a.thr[q] : -INFINITY;
  uint64_t* my_cand = a.cand + (size_t)q * a.cap;
  Pred pr{0u, 0u, 0u};
  if constexpr (FILT) pr = load_pred(a.pred, q, a.pred_stride);
  uint4 tw[4];
  const uint32_t* my_mask = nullptr;   // XM: the lane's query's mask row
  uint32_t mw = 0u;
  if constexpr (XM) my_mask = a.xmask + (size_t)(a.xrow ? a.xrow[q] : q) * a.xW;
  // FILT / XM: may accumulator row r of the lane be a candidate?
  auto row_ok = [&](int r) -> bool {
    bool ok = true;
    if constexpr (FILT) ok = pr.pass(tag_of(tw, r));
    if constexpr (XM) ok = ok && !((mw >> acc_row(r, lane)) & 1u);
    return ok;
  };
  // dense mode (threshold sample): slot = (pair, sampled tile, row): no atomics, no row-id gather
  uint64_t* my_dense = a.dense_cap > 0 ? a.cand + (size_t)pair * a.dense_cap : nullptr;
  const int64_t per = tpi;
  const int64_t i0 = (int64_t)split * per;
  const int64_t i1 = (i0 + per < n_seq) ? i0 + per : n_seq;
  if (i0 >= i1) return;

  f32x4 stage[NL];
  auto load_tile = [&](int64_t i) {  // rows of the tile are contiguous: lane l takes bytes [1024 j + 16 l, +16)
    const f32x4* src = reinterpret_cast<const f32x4*>(a.X + (size_t)(p0 + i * tstep * TRS) * D) + lane;
#pragma unroll
    for (int j = 0; j < NL; ++j) stage[j] = src[j * 64];
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int idx = j * 64 + lane;                 // 16-byte piece of the tile
      const int r = idx / (D / 4), c4 = idx % (D / 4);
      *reinterpret_cast<f32x4*>(&Xs[r * LDX + c4 * 4]) = stage[j];
    }
  };
  auto chain = [&]() -> f32x16 {
    f32x16 acc = zero16();
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(&Xs[r31 * LDX + kb * 8 + 4 * hh]);
      acc = mfma32(av.x, qf[kb].x, acc);
      acc = mfma32(av.y, qf[kb].y, acc);
      acc = mfma32(av.z, qf[kb].z, acc);
      acc = mfma32(av.w, qf[kb].w, acc);
    }
    return acc;
  };
  auto emit = [&](const f32x16& acc, int64_t i) {
    if (!q_ok) return;
    const int64_t t_row0 = i * tstep * TRS;              // first row of the tile inside the list
    const int64_t left = (int64_t)len - t_row0;           // list padding rows are never candidates
    const int n_ok = left >= TRS ? TRS : (left > 0 ? (int)left : 0);
    if (my_dense) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rr = acc_row(r, lane);
        const int64_t sl = i * TRS + rr;
        if (sl < a.dense_cap)
          my_dense[sl] = (rr < n_ok && row_ok(r))
                             ? make_key(acc[r], a.dense_ids ? (uint32_t)a.row_ids[p0 + t_row0 + rr] : 0u) : 0ull;
      }
      return;
    }
    unsigned hits = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (acc_row(r, lane) < n_ok && acc[r] >= thr && row_ok(r)) hits |= (1u << r);
    if (hits) {
      int pos = atomicAdd(&a.count[q * a.count_stride], __popc(hits));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (hits & (1u << r)) {
          const int64_t v = p0 + t_row0 + acc_row(r, lane);
          if (pos < a.cap) my_cand[pos] = make_key(acc[r], (uint32_t)a.row_ids[v]);
          ++pos;
        }
      }
    }
  };
  load_tile(i0);
  store_tile();
#pragma unroll 1
  for (int64_t i = i0; i < i1; ++i) {
    const bool more = i + 1 < i1;
    if (more) load_tile(i + 1);          // in flight during this tile's MFMA chain
    if constexpr (FILT) {
      const uint4* tp = reinterpret_cast<const uint4*>(a.tags + p0 + i * tstep * TRS + 4 * hh);
#pragma unroll
      for (int g = 0; g < 4; ++g) tw[g] = tp[2 * g];
    }
    if constexpr (XM) mw = my_mask[(p0 + i * tstep * TRS) >> 5];
    const f32x16 acc = chain();
    if (more) store_tile();              // after the chain's LDS reads (same wave: in order)
    emit(acc, i);
  }
}

}  // namespace

namespace rihip_index {

int launch_ivf_prepare_small(int d, const PrepSmallArgs& p, unsigned grid, hipStream_t st) {
  const size_t lds = sizeof(float) * 4 * p.nlist;
  RCCHK(dispatch_d(d, [&](auto D) { hipLaunchKernelGGL((ivf_prepare_small_kernel<decltype(D)::value>), dim3(grid), dim3(256), lds, st, p); }));
  return check_launch("ivf prepare (small)");
}

int launch_ivf_coarse(int d, const float* Q, int64_t nq, const float* C, int nlist, float* cs, hipStream_t st) {
  const dim3 grid((unsigned)((nq + 127) / 128));
  return dispatch_d(d, [&](auto D) { hipLaunchKernelGGL((ivf_coarse_kernel<decltype(D)::value>), grid, dim3(256), 0, st, Q, nq, C, nlist, cs); });
}

void launch_ivf_select(const float* cs, int64_t nq, int nlist, int nprobe, int* probe_list, int* list_cnt, hipStream_t st) {
  hipLaunchKernelGGL(ivf_select_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), sizeof(float) * 4 * nlist, st, cs, nq, nlist,
                     nprobe, probe_list, list_cnt);
}

void launch_ivf_plan(const int* list_cnt, const int64_t* list_poff, int nlist, int tile_step, int target_items, int* list_qoff,
                     int* list_cur, int* work_off, int* plan, int* count, int64_t n_count, hipStream_t st) {
  hipLaunchKernelGGL(ivf_plan_kernel, dim3(1), dim3(256), 0, st, list_cnt, list_poff, nlist, tile_step, target_items, list_qoff,
                     list_cur, work_off, plan, count, n_count);
}

void launch_ivf_scatter(const int* probe_list, int64_t n_pairs, int nprobe, int* list_cur, int* list_q, hipStream_t st) {
  hipLaunchKernelGGL(ivf_scatter_kernel, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, st, probe_list, n_pairs, nprobe,
                     list_cur, list_q);
}

int launch_ivf_scan(int d, const LmArgs& a, unsigned grid, hipStream_t st) {
  RCCHK(dispatch_d(d, [&](auto D) {
    if (a.xmask && a.tags) hipLaunchKernelGGL((ivf_scan_lm_kernel<decltype(D)::value, FM_TAGS_MASK>), dim3(grid), dim3(256), 0, st, a);
    else if (a.xmask) hipLaunchKernelGGL((ivf_scan_lm_kernel<decltype(D)::value, FM_MASK>), dim3(grid), dim3(256), 0, st, a);
    else if (a.tags) hipLaunchKernelGGL((ivf_scan_lm_kernel<decltype(D)::value, FM_TAGS>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((ivf_scan_lm_kernel<decltype(D)::value>), dim3(grid), dim3(256), 0, st, a);
  }));
  return check_launch(a.xmask ? "masked ivf scan" : a.tags ? "filtered ivf scan" : "ivf scan");
}

}  // namespace rihip_index
