// Exact-f32 scan of the inner-product index: every (query, corpus row) score on exact-f32 MFMA, the scores that reach
// the query's threshold kept as 64-bit keys (dense slots or appended candidate lists).  Used by the small-corpus search,
// the all-f32 thresholded search, the filtered flat search and the exact re-do of failed queries.
#include "search_kernels.h"
#include "search_keys.h"

using namespace rihip_index;

namespace {

template <bool FILT>
__device__ __forceinline__ uint32_t* tag_tiles() {   // LDS only in the filtered instantiation
  if constexpr (FILT) {
    __shared__ __attribute__((aligned(16))) uint32_t Ts[3 * TRS];
    return Ts;
  } else {
    return nullptr;
  }
}

// 4 waves x 32 register-stationary queries share each 32-row corpus tile.  Same software pipeline as the
// in-batch sweep: 3 LDS buffers, tile t+2 prefetched through registers, the S chain of tile t+1 interleaved with
// the threshold test / candidate emission of tile t, one barrier per tile.
// FILT: every tile brings its 32 tag words along through the same prefetch (one coalesced 128-byte load by 32 threads, a
// slot of LDS per stage); emit tests the lane's query predicate against them.  A failing row is key 0 (below every score)
// in a dense slot and simply no hit in append mode.  FM_NONE compiles to the unfiltered kernel as it was.
// FM_TAGS_MASK / FM_MASK (seen-item exclusion, search_exclude.hip): a stride-1 tile is one aligned mask word of the lane's
// query, loaded two tiles ahead with the operand prefetch and handed down a register per stage; a strided pass (the
// threshold sample) scans rows that are not adjacent and reads each row's own bit in emit.  FM_MASK compiles the tag test out.
template <int D, int FM = FM_NONE>
__global__ __launch_bounds__(256, 2) void scan_kernel(ScanArgs a) {
  constexpr bool FILT = FM == FM_TAGS || FM == FM_TAGS_MASK, XM = FM == FM_TAGS_MASK || FM == FM_MASK;
  constexpr int LDX = D + 4, KB = D / 8;
  constexpr int EPK = 16 / KB > 0 ? 16 / KB : 1;
  constexpr int NV = (TRS * (D / 4) + 255) / 256;
  __shared__ __attribute__((aligned(16))) float Xs[3][TRS * LDX];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r31 = lane & 31, hh = lane >> 5;
  const int64_t q = (int64_t)blockIdx.x * QB + w * 32 + r31;
  const bool q_ok = q < a.nq;
  const int64_t qrow = q_ok ? q : (a.nq - 1);

  f32x4 qf[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) qf[kb] = *reinterpret_cast<const f32x4*>(&a.Q[qrow * D + kb * 8 + 4 * hh]);
  const float thr = (a.thr && q_ok) ? a.thr[q] : -INFINITY;
  uint64_t* my_cand = a.cand + (size_t)qrow * a.cap;
  uint32_t* Ts = tag_tiles<FILT>();
  Pred pr{0u, 0u, 0u};
  if constexpr (FILT) pr = load_pred(a.pred, qrow, a.pred_stride);
  uint32_t tg = 0u;   // FILT: staged tag word (threads 0..31)
  const uint32_t* my_mask = nullptr;   // XM: the lane's query's mask row
  uint32_t mw0 = 0u, mw1 = 0u, mw2 = 0u;   // XM, stride 1: mask words of the tile in emit, the next one and the prefetched one
  if constexpr (XM) my_mask = a.xmask + (size_t)(a.xrow ? a.xrow[qrow] : qrow) * a.xW;
  const bool x_tile = XM && a.row_stride == 1;

  const int64_t n_seq = (a.n_virtual + TRS - 1) / TRS;
  const int64_t per = (n_seq + a.nsplit - 1) / a.nsplit;
  const int64_t i0 = (int64_t)blockIdx.y * per;
  const int64_t i1 = (i0 + per < n_seq) ? i0 + per : n_seq;
  if (i0 >= i1) return;  // uniform across the workgroup

  f32x4 stage[NV];
  auto tile_at = [&](int64_t i) -> int64_t { return i; };
  auto load_tile = [&](int64_t tile) {
    const int64_t v_base = tile * TRS;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      const int r = idx / (D / 4), c4 = idx % (D / 4);
      const int64_t v = v_base + r;
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (idx < TRS * (D / 4) && v < a.n_virtual)
        val = reinterpret_cast<const f32x4*>(a.X + (size_t)(v * a.row_stride) * D)[c4];
      stage[i] = val;
    }
    if constexpr (FILT) {
      tg = 0u;
      if (tid < TRS && v_base + tid < a.n_virtual) tg = a.tags[(size_t)((v_base + tid) * a.row_stride)];
    }
    if constexpr (XM) {
      if (x_tile) mw2 = my_mask[tile];
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * 256;
      const int r = idx / (D / 4), c4 = idx % (D / 4);
      if (idx < TRS * (D / 4)) *reinterpret_cast<f32x4*>(&Xs[buf][r * LDX + c4 * 4]) = stage[i];
    }
    if constexpr (FILT) {
      if (tid < TRS) Ts[buf * TRS + tid] = tg;
    }
  };
  auto emit = [&](const f32x16& acc, int64_t tile, int buf) {
    const int64_t v_base = tile * TRS;
    if (!q_ok) return;
    uint4 tw[4];
    if constexpr (FILT) {
#pragma unroll
      for (int g = 0; g < 4; ++g) tw[g] = *reinterpret_cast<const uint4*>(&Ts[buf * TRS + 8 * g + 4 * hh]);
    }
    // XM: is accumulator row r of the lane (virtual row v < n_virtual) excluded for the lane's query?
    auto masked = [&](int r, int64_t v) -> bool {
      if (x_tile) return (mw0 >> acc_row(r, lane)) & 1u;
      const int64_t p = v * a.row_stride;
      return (my_mask[p >> 5] >> (p & 31)) & 1u;
    };
    if (a.dense) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t v = v_base + acc_row(r, lane);
        if constexpr (XM) {
          if (v < a.n_virtual) {
            bool ok = !masked(r, v);
            if constexpr (FILT) ok = ok && pr.pass(tag_of(tw, r));
            my_cand[v] = ok ? make_key(acc[r], (uint32_t)v) : 0ull;
          }
        } else if constexpr (FILT) {
          if (v < a.n_virtual) my_cand[v] = pr.pass(tag_of(tw, r)) ? make_key(acc[r], (uint32_t)v) : 0ull;
        } else {
          if (v < a.n_virtual) my_cand[v] = make_key(acc[r], (uint32_t)v);
        }
      }
      return;
    }
    const int n_ok = (a.n_virtual - v_base) < TRS ? (int)(a.n_virtual - v_base) : TRS;
    unsigned hits = 0;  // per-lane aggregation: one atomic per (query, tile) that has survivors
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if constexpr (XM) {
        if (acc_row(r, lane) < n_ok && acc[r] >= thr) {
          bool ok = !masked(r, v_base + acc_row(r, lane));
          if constexpr (FILT) ok = ok && pr.pass(tag_of(tw, r));
          if (ok) hits |= (1u << r);
        }
      } else if constexpr (FILT) {
        if (acc_row(r, lane) < n_ok && acc[r] >= thr && pr.pass(tag_of(tw, r))) hits |= (1u << r);
      } else {
        if (acc_row(r, lane) < n_ok && acc[r] >= thr) hits |= (1u << r);
      }
    }
    if (hits) {
      int pos = atomicAdd(&a.count[q * (a.cs > 1 ? a.cs : 1)], __popc(hits));
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (hits & (1u << r)) {
          const int64_t v = v_base + acc_row(r, lane);
          if (pos < a.cap) my_cand[pos] = make_key(acc[r], (uint32_t)v);
          ++pos;
        }
      }
    }
  };
  auto s_chain = [&](const float* Xt, f32x16& acc) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(&Xt[r31 * LDX + kb * 8 + 4 * hh]);
      acc = mfma32(av.x, qf[kb].x, acc);
      acc = mfma32(av.y, qf[kb].y, acc);
      acc = mfma32(av.z, qf[kb].z, acc);
      acc = mfma32(av.w, qf[kb].w, acc);
    }
  };

  load_tile(tile_at(i0));
  store_tile(0);
  if constexpr (XM) mw0 = mw2;
  if (i0 + 1 < i1) {
    load_tile(tile_at(i0 + 1));
    store_tile(1);
    if constexpr (XM) mw1 = mw2;
  }
  __syncthreads();
  f32x16 st = zero16();
  s_chain(Xs[0], st);

#pragma unroll 1
  for (int64_t i = i0; i < i1; ++i) {
    const int it = (int)((i - i0) % 3);
    const int nxt = (it + 1) % 3, pre = (it + 2) % 3;
    const bool has_next = (i + 1 < i1), has_pre = (i + 2 < i1);
    if (has_pre) load_tile(tile_at(i + 2));
    f32x16 sn = zero16();
    if (has_next) s_chain(Xs[nxt], sn);  // the compiler interleaves the (independent) emit below into this chain
    emit(st, tile_at(i), it);
    if (has_pre) store_tile(pre);
    st = sn;
    if constexpr (XM) { mw0 = mw1; mw1 = mw2; }
    __syncthreads();
  }
}

template <int D>
void launch_scan_d(const ScanArgs& a, dim3 grid, hipStream_t st) {
  if (a.xmask && a.tags) hipLaunchKernelGGL((scan_kernel<D, FM_TAGS_MASK>), grid, dim3(256), 0, st, a);
  else if (a.xmask) hipLaunchKernelGGL((scan_kernel<D, FM_MASK>), grid, dim3(256), 0, st, a);
  else if (a.tags) hipLaunchKernelGGL((scan_kernel<D, FM_TAGS>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((scan_kernel<D, FM_NONE>), grid, dim3(256), 0, st, a);
}

}  // namespace

namespace rihip_index {

int launch_scan(int d, const ScanArgs& a, dim3 grid, hipStream_t st) {
  RCCHK(dispatch_d(d, [&](auto D) { launch_scan_d<decltype(D)::value>(a, grid, st); }));
  return check_launch("scan");
}

}  // namespace rihip_index
