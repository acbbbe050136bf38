// The owner sweep shared by the runtime-width in-batch loss kernels (loss_generic.hip, loss_softmax.hip and the select
// sweep of loss_hard.hip): exact-f32 MFMA, any embedding width gen_width_ok accepts.
//
// One workgroup (4 waves) owns GOW = 128 owners = one loss slot, 32 at a time in LDS (Os, zero-padded).  The swept rows
// go by in tiles of GSW = 128: wg_gemm<false> leaves one 32 x 32 tile of S = O.Y^T per wave (wave w holds the swept rows
// sb + 32w .., accumulator element r of a lane is owner acc_row(r, lane) against swept row sb + 32w + (lane & 31)).  A
// kernel that needs a second product writes the tile's weights to Gs and multiplies them back against the same swept
// rows with wg_gemm<true, true> (B[n = c][k = s] = Y[(sb + s)*D + c]: transposed panel): dOwner += G.Y, output column
// out_col(t, w, r31) in out[t][r].  Per-owner row statistics are reduced over the 32 lanes that hold an owner's row
// (row32_*), parked per wave in red and combined over the four waves in fixed order (red4_*).  No atomics on floats,
// fixed summation order.  Dynamic LDS: Os [32][D+4] | Gs [32][GLDG] | Wp [256][GLDP] (k-panel of wg_gemm) | red [4][32],
// gen_sweep_lds(D) bytes; a one-product sweep has no Gs and no red.
// A kernel is: for og < GOG { o_base = owner_base(og); break past No; stage_owners; for each tile { nsw; wg_gemm<false>;
// tile_lane; 16 x (tile_elem + its own element math); wg_gemm<true, true> } its own epilogue }.  The LDS carve, the nsw
// line and the wg_gemm calls are written out in each kernel on purpose: behind helpers (a struct of pointers, a
// row-count function, call wrappers) the same source compiled to slower code, measured on the device
// (profiles/r21_gen_sweep.md).
#pragma once
#include "gen_gemm.h"

namespace rihip_gen {

constexpr int GOW = 128;         // owners per workgroup = one loss slot
constexpr int GOG = GOW / 32;    // owner groups per workgroup
constexpr int GSW = 128;         // swept rows per tile
constexpr int GLDG = GSW + 4;    // row stride of Gs

__host__ __device__ inline int gen_ldo(int D) { return D + 4; }   // row stride of Os

// dynamic LDS of a two-product sweep: Os [32][D+4] | Gs [32][GLDG] | Wp [256][GLDP] | red [4][32]
inline size_t gen_sweep_lds(int D) {
  return sizeof(float) * ((size_t)32 * gen_ldo(D) + 32 * GLDG + 256 * GLDP + 128);
}

__device__ __forceinline__ int64_t owner_base(int og) { return (int64_t)blockIdx.x * GOW + og * 32; }

// Owners o_base .. o_base + 31 into Os, zero beyond No.  Opens with a workgroup barrier (the previous group's readers of
// Os and of the kernel's per-group LDS are done): every wave must call it.
__device__ __forceinline__ void stage_owners(float* Os, int ldo, const float* Xo, int64_t o_base, int64_t No, int D,
                                             int tid) {
  __syncthreads();
  for (int idx = tid; idx < 32 * D; idx += 256) {
    const int r = idx / D, k = idx % D;
    Os[r * ldo + k] = (o_base + r < No) ? Xo[(o_base + r) * D + k] : 0.f;
  }
}

__device__ __forceinline__ int out_col(int t, int w, int r31) { return (w + 4 * t) * 32 + r31; }

// the swept row of a lane in the tile at sb
struct TileLane {
  int64_t srow;   // local index
  bool s_ok;      // inside the swept set
  int64_t s_g;    // global index
};
__device__ __forceinline__ TileLane tile_lane(int64_t sb, int w, int r31, int64_t Ns, int64_t s_goff) {
  const int64_t srow = sb + w * 32 + r31;
  return {srow, srow < Ns, s_goff + srow};
}
// accumulator element r of a lane
struct TileElem {
  int ol;         // owner inside the group
  int64_t orow;   // local owner index
  bool valid;     // owner and swept row both exist
  bool diag;      // the swept row is the owner's positive partner
};
__device__ __forceinline__ TileElem tile_elem(int r, int lane, int64_t o_base, int64_t No, int64_t o_goff,
                                              const TileLane& t) {
  const int ol = acc_row(r, lane);
  const int64_t orow = o_base + ol;
  return {ol, orow, t.s_ok && orow < No, (o_goff + orow) == t.s_g};
}
__device__ __forceinline__ int64_t swept_id(bool ids, const int64_t* s_ids, const TileLane& t) {
  return (ids && t.s_ok) ? s_ids[t.srow] : 0;
}
// accidental hit: another row that carries the owner's positive; the diagonal is never masked
__device__ __forceinline__ bool masked(bool ids, bool diag, int64_t id_s, int64_t own_id) {
  return ids && !diag && id_s == own_id;
}

// over the 32 lanes that hold one owner's row of the tile
__device__ __forceinline__ float row32_sum(float v) {
  v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64);
  return v;
}
__device__ __forceinline__ float row32_max(float v) {
  v = fmaxf(v, __shfl_xor(v, 1, 64)); v = fmaxf(v, __shfl_xor(v, 2, 64)); v = fmaxf(v, __shfl_xor(v, 4, 64));
  v = fmaxf(v, __shfl_xor(v, 8, 64)); v = fmaxf(v, __shfl_xor(v, 16, 64));
  return v;
}
// over the four waves' entries red[w*32 + ol], fixed order
__device__ __forceinline__ float red4_sum(const float* red, int ol) {
  return ((red[ol] + red[32 + ol]) + red[64 + ol]) + red[96 + ol];
}
__device__ __forceinline__ float red4_max(const float* red, int ol) {
  return fmaxf(fmaxf(red[ol], red[32 + ol]), fmaxf(red[64 + ol], red[96 + ol]));
}

// A kernel's dynamic LDS beyond the default 64 KB has to be granted once per process before its first launch.
inline hipError_t grant_dynamic_lds(const void* kernel, size_t bytes) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

}  // namespace rihip_gen
