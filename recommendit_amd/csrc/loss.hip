// BPR losses for gfx950.
//  * bpr_pair:   sampled-negative BPR (reference src/models/two_tower.py:117-130), loss + grads fused.
//  * inbatch sweep: in-batch-negative BPR (reference src/models/two_tower.py:132-160) as a
//    flash-style fused score/loss/gradient sweep on exact-f32 MFMA.  The B x B score matrix is
//    never materialised: a workgroup owns 32 "owner" rows (users in MODE_USER, items in
//    MODE_ITEM), keeps their embedding fragments register-stationary, and sweeps tiles of the
//    other side through LDS.  For each 32x32 tile:  S^T = Y.Xo^T (MFMA) -> sigma/softplus (VALU)
//    -> dOwner += G^T-as-A-operand . Y (MFMA; the accumulator registers ARE the next A operand,
//    no LDS round trip).  Owner gradients never cross workgroups => no atomics, bitwise
//    reproducible.  dU and dI come from two launches of the same kernel with roles swapped
//    (S is recomputed; 8 B^2 d FLOP instead of 6 B^2 d, but zero atomic traffic).
#include <stdlib.h>
#include "common.h"
#include "recommendit_hip.h"
#include "loss_sweep_args.h"

void rihip_launch_sweep_bf16x3(int d, bool mode_user, const SweepArgs& a, dim3 grid, hipStream_t st);
void rihip_launch_sweep_x6(int d, bool mode_user, const SweepArgs& a, dim3 grid, int nw, hipStream_t st);
void rihip_launch_gt_x6(int d, const SweepArgs& a, dim3 grid, int nw, hipStream_t st);

namespace {

// ------------------------------------------------------------------------------------------
// sampled-negative BPR: one wave per row
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bpr_pair_kernel(const float* __restrict__ U, const float* __restrict__ P,
                                                       const float* __restrict__ N, int64_t B, int d, float inv_B,
                                                       float* dU, float* dP, float* dN, double* part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc = 0.0;
  for (int64_t b = (int64_t)blockIdx.x * 4 + w; b < B; b += (int64_t)gridDim.x * 4) {
    float sp = 0.f, sn = 0.f;
    for (int c = lane; c < d; c += 64) {
      const float u = U[b * d + c];
      sp += u * P[b * d + c];
      sn += u * N[b * d + c];
    }
    sp = wave_sum(sp);
    sn = wave_sum(sn);
    const float delta = sp - sn;
    // -logsigmoid(delta) = softplus(-delta); d/d delta = -sigmoid(-delta)
    const float e = expf(-fabsf(delta));
    const float loss = fmaxf(-delta, 0.f) + log1pf(e);
    const float sig_neg = (delta >= 0.f) ? e / (1.f + e) : 1.f / (1.f + e);  // sigmoid(-delta)
    const float wgt = -sig_neg * inv_B;
    for (int c = lane; c < d; c += 64) {
      const float u = U[b * d + c], p = P[b * d + c], n = N[b * d + c];
      dU[b * d + c] = wgt * (p - n);
      dP[b * d + c] = wgt * u;
      dN[b * d + c] = -wgt * u;
    }
    if (lane == 0) acc += (double)loss;
  }
  __shared__ double sh[4];
  if (lane == 0) sh[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// float4 form for d in {32, 64, 128}: LPR = d/4 lanes per row, 64/LPR rows per wave side by side
template <int LPR>
__global__ __launch_bounds__(256) void bpr_pair_v4_kernel(const float* __restrict__ U, const float* __restrict__ P,
                                                          const float* __restrict__ N, int64_t B, float inv_B,
                                                          float* dU, float* dP, float* dN, double* part) {
  constexpr int RPW = 64 / LPR, d = LPR * 4;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane / LPR, c4 = lane % LPR;
  double acc = 0.0;
  for (int64_t b0 = ((int64_t)blockIdx.x * 4 + w) * RPW; b0 < B; b0 += (int64_t)gridDim.x * 4 * RPW) {
    const int64_t b = b0 + sub;
    const bool ok = b < B;
    const int64_t bc = ok ? b : B - 1;
    const f32x4 u = reinterpret_cast<const f32x4*>(U + bc * d)[c4];
    const f32x4 p = reinterpret_cast<const f32x4*>(P + bc * d)[c4];
    const f32x4 n = reinterpret_cast<const f32x4*>(N + bc * d)[c4];
    float sp = (u.x * p.x + u.y * p.y) + (u.z * p.z + u.w * p.w);
    float sn = (u.x * n.x + u.y * n.y) + (u.z * n.z + u.w * n.w);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) {
      sp += __shfl_xor(sp, o, 64);
      sn += __shfl_xor(sn, o, 64);
    }
    const float delta = sp - sn;
    const float e = expf(-fabsf(delta));
    const float loss = fmaxf(-delta, 0.f) + log1pf(e);
    const float sig_neg = (delta >= 0.f) ? e / (1.f + e) : 1.f / (1.f + e);  // sigmoid(-delta)
    const float wgt = -sig_neg * inv_B;
    if (ok) {
      reinterpret_cast<f32x4*>(dU + b * d)[c4] = f32x4{wgt * (p.x - n.x), wgt * (p.y - n.y), wgt * (p.z - n.z), wgt * (p.w - n.w)};
      reinterpret_cast<f32x4*>(dP + b * d)[c4] = f32x4{wgt * u.x, wgt * u.y, wgt * u.z, wgt * u.w};
      reinterpret_cast<f32x4*>(dN + b * d)[c4] = f32x4{-wgt * u.x, -wgt * u.y, -wgt * u.z, -wgt * u.w};
      if (c4 == 0) acc += (double)loss;
    }
  }
  acc = wave_sum_d(acc);
  __shared__ double sh[4];
  if (lane == 0) sh[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// loss = scale * sum(part[0..n))  -- single wave, fixed order => deterministic
__global__ void finalize_sum_kernel(const double* __restrict__ part, int n, double scale, float* out) {
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 64) s += part[i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) *out = (float)(s * scale);
}

// pos[i] = U[i] . I[i + off]
__global__ __launch_bounds__(256) void rowdot_kernel(const float* __restrict__ U, const float* __restrict__ I,
                                                     int64_t B, int64_t off, int d, float* pos) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t b = (int64_t)blockIdx.x * 4 + w; b < B; b += (int64_t)gridDim.x * 4) {
    float s = 0.f;
    for (int c = lane; c < d; c += 64) s += U[b * d + c] * I[(b + off) * d + c];
    s = wave_sum(s);
    if (lane == 0) pos[b] = s;
  }
}

// ------------------------------------------------------------------------------------------
// in-batch sweep
// ------------------------------------------------------------------------------------------
// B operands of the G.Y products.  Lane (r31, hh) of accumulator out[t] owns output column r31 * CT + t (not
// t * 32 + r31), so the CT values it needs from one k-row of the row-major LDS tile are contiguous: one ds_read_b128
// (d = 128), ds_read_b64 (d = 64) or ds_read_b32 (d = 32) per k-row, conflict-free for every lane group.  Each output
// element still sums the same products in the same k-order, so only the lane -> column map changes.
template <int CT>
struct BRow {
  float v[CT];
};
template <int CT>
__device__ __forceinline__ BRow<CT> lds_brow(const float* p) {
  BRow<CT> b;
  if constexpr (CT == 4) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(p);
    b.v[0] = x.x; b.v[1] = x.y; b.v[2] = x.z; b.v[3] = x.w;
  } else if constexpr (CT == 2) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 x = *reinterpret_cast<const f32x2*>(p);
    b.v[0] = x.x; b.v[1] = x.y;
  } else {
    static_assert(CT == 1, "embed_dim 32 / 64 / 128");
    b.v[0] = p[0];
  }
  return b;
}
// Left to itself the scheduler sinks each read next to its first use (a wait on every read).  Pin the order: the
// reads of LEAD k-rows, then per read instruction (while any are left) the MFMAs of the k-rows it covers.  The 4- and
// 8-byte reads of two neighbouring k-rows are fused into one ds_read2_b32 / ds_read2_b64, so those count in pairs.
template <int CT, int LEAD>
__device__ __forceinline__ void brow_schedule(int nrows) {
  constexpr int RPI = CT == 4 ? 1 : 2;  // k-rows per read instruction
  __builtin_amdgcn_sched_group_barrier(0x100, LEAD / RPI, 0);  // DS read
#pragma unroll
  for (int j = 0; j < nrows; j += RPI) {
    if (j + LEAD < nrows) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x8, RPI * CT, 0);    // MFMA
  }
}
// Scalar (kernel-argument) loads share lgkmcnt with the LDS reads and return out of order: one still pending at a
// loop's entry makes the first LDS wait of every trip a full lgkmcnt(0).  Called in front of the tile loops.
__device__ __forceinline__ void scalar_loads_done() { __builtin_amdgcn_s_waitcnt(0xc07f); }  // lgkmcnt(0) only
// The steady tile loops address global memory as a uniform base (a buffer resource rebuilt from an advancing scalar
// pointer once per trip, so there is no 4 GB window) plus a constant 32-bit lane offset plus a constant: no per-lane
// 64-bit address arithmetic.  Reads past `bytes` return 0; the loops never make one.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const float* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);  // raw, 32-bit data
}
__device__ __forceinline__ f32x4 buffer_load_f32x4(__amdgpu_buffer_rsrc_t r, unsigned lane_off, int off) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)lane_off, off, 0));
}
// GOUT (user mode only): additionally write the G tile (diagonal and ragged entries = 0) to a.gmat, so that the item
// gradients come from a plain G^T.U product (inbatch_gt_kernel) instead of a second score sweep.
template <int D, bool MODE_USER, bool GOUT = false, int NW = 4>
__global__ __launch_bounds__(NW * 64, 2) void inbatch_sweep_kernel(SweepArgs a) {
  constexpr int NT = NW * 64;  // NW = 8: one 512-thread workgroup per CU, half the swept-tile traffic per owner
  static_assert(!GOUT || MODE_USER, "G is stored by the user-mode sweep");
  constexpr int LDY = D + 4;
  constexpr int KB = D / 8, CT = D / 32;
  constexpr int EPK = 16 / KB > 0 ? 16 / KB : 1;   // score elements processed per k-block of the next S chain
  constexpr int NV = (TSW * (D / 4) + NT - 1) / NT;  // float4 staged per thread per tile
  static_assert(KB <= 16, "embed_dim <= 128");
  __shared__ __attribute__((aligned(16))) float Ysh[3][TSW * LDY];
  __shared__ float posS[3][TSW];
  __shared__ float rS[3][TSW];
  __shared__ float rsum[NW][32];
  __shared__ double red_loss[NW];

  // w through readfirstlane: the wave index is uniform, and the tile tests built on o_base then stay in SGPRs
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r31 = lane & 31, hh = lane >> 5;
  const int64_t o_base = (int64_t)blockIdx.x * (NW * 32) + w * 32;
  const int64_t o_loc = o_base + r31;  // this lane's owner (S^T accumulator column)
  const bool o_ok = o_loc < a.No;
  const int64_t o_gidx = a.o_goff + o_loc;
  const bool owners_full = (o_base + 32 <= a.No);

  // register-stationary owner fragments: B[k][n=o] = Xo[o][k]
  f32x4 xo[KB];
  {
    const int64_t orow = o_ok ? o_loc : (a.No - 1);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      xo[kb] = *reinterpret_cast<const f32x4*>(&a.Xo[orow * D + kb * 8 + 4 * hh]);
      xo[kb] *= RIHIP_LOG2E;  // scores come out of the MFMA chain in log2 units (sweep_elem)
    }
  }
  const float pos_o = (MODE_USER && o_ok) ? a.pos[o_loc] * RIHIP_LOG2E : 0.f;
  const float inv_c = 1.f / a.c;

  f32x16 out[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) out[t] = zero16();
  float r_acc = 0.f, loss_acc = 0.f;

  const int64_t ntiles = (a.Ns + TSW - 1) / TSW;
  const int64_t per = (ntiles + a.nsplit - 1) / a.nsplit;
  const int64_t t0 = (int64_t)blockIdx.y * per;
  const int64_t t1 = (t0 + per < ntiles) ? t0 + per : ntiles;

  f32x4 stage[NV];
  float st_pos = 0.f, st_r = 0.f;
  auto load_tile = [&](int64_t tile) {
    const int64_t s_base = tile * TSW;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * NT;
      const int r = idx / (D / 4), c4 = idx % (D / 4);
      const int64_t srow = s_base + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (idx < TSW * (D / 4) && srow < a.Ns) v = reinterpret_cast<const f32x4*>(a.Ys + srow * D)[c4];
      stage[i] = v;
    }
    if (!MODE_USER && tid < TSW) {
      const int64_t srow = s_base + tid;
      st_pos = (srow < a.Ns) ? a.pos[srow] * RIHIP_LOG2E : 0.f;
      st_r = (srow < a.Ns) ? a.r_in[srow] : 0.f;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * NT;
      const int r = idx / (D / 4), c4 = idx % (D / 4);
      if (idx < TSW * (D / 4)) *reinterpret_cast<f32x4*>(&Ysh[buf][r * LDY + c4 * 4]) = stage[i];
    }
    if (!MODE_USER && tid < TSW) {
      posS[buf][tid] = st_pos;
      rS[buf][tid] = st_r;
    }
  };

  if (t0 >= t1) {  // empty split (can only happen for degenerate splits): contribute zeros
    if (hh == 0) rsum[w][r31] = 0.f;
    if (MODE_USER && lane == 0) red_loss[w] = 0.0;
  }
  f32x16 st = zero16();
  if (t0 < t1) {
    load_tile(t0);
    store_tile(0);
    if (t0 + 1 < t1) {
      load_tile(t0 + 1);
      store_tile(1);
    }
    __syncthreads();
    const float* Y0 = Ysh[0];
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {  // S^T of the first tile (not overlapped)
      const f32x4 av = *reinterpret_cast<const f32x4*>(&Y0[r31 * LDY + kb * 8 + 4 * hh]);
      st = mfma32(av.x, xo[kb].x, st);
      st = mfma32(av.y, xo[kb].y, st);
      st = mfma32(av.z, xo[kb].z, st);
      st = mfma32(av.w, xo[kb].w, st);
    }
  }

  // S^T(next tile) chain from Yn into sb, interleaved with the branch-free element work on sa (full tile, off the
  // diagonal).  Unconditional: on the last tile this multiplies a stale buffer and the result is dropped -- a branch
  // here splits the block and the scheduler then parks all the VALU work behind the MFMA chain.
  auto fast_block = [&](const float* Yn, int cur, const f32x16& sa, f32x16& sb, float (&g)[16]) {
    float den_prod = 1.f;  // running product of (1 + e^-z): one log per eight elements
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(&Yn[r31 * LDY + kb * 8 + 4 * hh]);
      sb = mfma32(av.x, xo[kb].x, sb);
      sb = mfma32(av.y, xo[kb].y, sb);
      sb = mfma32(av.z, xo[kb].z, sb);
      sb = mfma32(av.w, xo[kb].w, sb);
#pragma unroll
      for (int e = 0; e < EPK; ++e) {
        const int r = kb * EPK + e;
        const float pos = MODE_USER ? pos_o : posS[cur][acc_row(r, lane)];
        g[r] = sweep_elem<MODE_USER, true>(sa[r], pos, true, false, 0.f, loss_acc, den_prod, r_acc);
        if constexpr (SWEEP_STEADY(D, MODE_USER, GOUT, NW)) {
          // The SLP vectoriser pairs independent f32 adds (loss_acc with r_acc, 1 + e of two elements) into v_pk_*_f32,
          // which cost far more than two scalar ops beside the MFMAs.  An empty asm makes each value opaque to it.
          asm("" : "+v"(loss_acc));
          asm("" : "+v"(r_acc));
          asm("" : "+v"(g[r]));
          asm("" : "+v"(den_prod));
        }
        if (MODE_USER && (r & 7) == 7) {
          loss_acc += __builtin_amdgcn_logf(den_prod);
          den_prod = 1.f;
        }
      }
    }
  };
  // ---- dOwner[o][c] += sum_s G[s][o] * Y[s][c]   (A operand = g registers, k = acc_row(r))
  // k-row of g[r] is acc_row(r) = (r & 3) + 8 (r >> 2) + 4 hh; its B operands are read LEAD k-rows ahead.
  // gstore(k-row within the half, value): the GOUT store of one G element (2 full 128 B lines per wave store)
  auto gy_block = [&](const float* Yc, const float (&g)[16], auto gstore) {
    const float* Yb = Yc + 4 * hh * LDY + r31 * CT;
    constexpr int LEAD = 8 / CT;
    BRow<CT> yb[16];
#pragma unroll
    for (int r = 0; r < LEAD; ++r) yb[r] = lds_brow<CT>(Yb + ((r & 3) + 8 * (r >> 2)) * LDY);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rn = r + LEAD;
      if (rn < 16) yb[rn] = lds_brow<CT>(Yb + ((rn & 3) + 8 * (rn >> 2)) * LDY);
      if (GOUT) gstore((r & 3) + 8 * (r >> 2), g[r]);
#pragma unroll
      for (int t = 0; t < CT; ++t) out[t] = mfma32(g[r], yb[r].v[t], out[t]);
    }
    brow_schedule<CT, LEAD>(16);
  };

  int64_t tile = t0;
  int it = 0;  // (tile - t0) % 3: the LDS ring position of the current tile
  auto general_tile = [&]() {
    const int cur = it, nxt = (it + 1) % 3, pre = (it + 2) % 3;
    const int64_t s_base = tile * TSW;
    const bool has_pre = (tile + 2 < t1);
    if (has_pre) load_tile(tile + 2);  // global loads stay in flight under the MFMA blocks below

    // does this tile touch the diagonal of this wave's owners or a ragged edge?
    const int64_t sg0 = a.s_goff + s_base, og0 = a.o_goff + o_base;
    const bool slow = !(owners_full && (s_base + TSW <= a.Ns)) || (sg0 < og0 + 32 && og0 < sg0 + TSW);
    // 32-bit forms of the per-element tests (only evaluated on slow tiles)
    const int64_t dd = og0 - sg0;                                        // diag  <=>  sl - r31 == dd
    const int ddi = (dd > -64 && dd < 64) ? (int)dd : 1000;
    const int64_t left = a.Ns - s_base;
    const int n_valid = left < TSW ? (int)left : TSW;                    // valid <=>  sl < n_valid (and o_ok)
    const float* Yn = Ysh[nxt];
    const float* Yc = Ysh[cur];
    f32x16 sn = zero16();
    float g[16];
    if (!slow) {
      fast_block(Yn, cur, st, sn, g);
    } else {
      float den_prod = 1.f;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        {  // unconditional, as in fast_block
          const f32x4 av = *reinterpret_cast<const f32x4*>(&Yn[r31 * LDY + kb * 8 + 4 * hh]);
          sn = mfma32(av.x, xo[kb].x, sn);
          sn = mfma32(av.y, xo[kb].y, sn);
          sn = mfma32(av.z, xo[kb].z, sn);
          sn = mfma32(av.w, xo[kb].w, sn);
        }
#pragma unroll
        for (int e = 0; e < EPK; ++e) {
          const int r = kb * EPK + e;
          const int sl = acc_row(r, lane);
          const bool valid = o_ok && (sl < n_valid);
          const bool diag = (sl - r31 == ddi);
          const float pos = MODE_USER ? pos_o : posS[cur][sl];
          const float rd = MODE_USER ? 0.f : -rS[cur][sl] * inv_c;  // weights are unscaled until the epilogue
          g[r] = sweep_elem<MODE_USER, false>(st[r], pos, valid, diag, rd, loss_acc, den_prod, r_acc);
          if (MODE_USER && (r & 7) == 7) {
            loss_acc += __builtin_amdgcn_logf(den_prod);
            den_prod = 1.f;
          }
        }
      }
    }
    float* gp = nullptr;
    if (GOUT) gp = a.gmat + ((size_t)tile * a.g_ub + (size_t)blockIdx.x * NW + w) * 1024 + (4 * hh) * 32 + r31;
    gy_block(Yc, g, [&](int krow, float v) { gp[krow * 32] = v; });
    if (has_pre) store_tile(pre);
    st = sn;
    __syncthreads();
    ++tile;
    it = (it == 2 ? 0 : it + 1);
  };

  // Which instantiations take the steady loop: SWEEP_STEADY (loss_sweep_args.h).  The one-tile loop runs every tile
  // of the others, and the first three tiles (one turn of the LDS ring) otherwise.
  constexpr bool STEADY = SWEEP_STEADY(D, MODE_USER, GOUT, NW);
  const int64_t lead_end = (STEADY && t0 + 3 < t1) ? t0 + 3 : t1;
  scalar_loads_done();
#pragma unroll 1
  while (tile < lead_end) general_tile();

  // Steady tiles: full, off the diagonal band of the workgroup's owners, tile + 2 a full tile of this split -- so no
  // bounds test, no conditional load and no `slow` evaluation.  They run six per trip (the LDS ring has period 3, the
  // st / sn pair period 2), so ring positions and accumulator names are static and nothing is copied.  Two ranges:
  // before the band and after it.  Everything else (the band, the last two tiles, the up to five tiles left before a
  // range can start at ring position 0) goes through the one-tile code, one tile at a time.
  if constexpr (STEADY) {
    static_assert(!STEADY || (MODE_USER && GOUT && (TSW * (D / 4)) % NT == 0), "user pass with stored G, whole rows");
    const int ntl = (int)(t1 - t0);
    auto rel = [&](int64_t t) { t -= t0; return (int)(t < 0 ? 0 : (t > ntl ? ntl : t)); };  // tile -> [0, ntl]
    const int64_t nfull = a.Ns / TSW;
    const bool wg_full = (int64_t)(blockIdx.x + 1) * (NW * 32) <= a.No;
    const int s_lim = wg_full ? rel((t1 < nfull ? t1 : nfull) - 2) : 0;
    // tiles [band_lo, band_hi) hold a diagonal element of one of the workgroup's NW * 32 owners
    const int64_t ddw = a.o_goff + (int64_t)blockIdx.x * (NW * 32) - a.s_goff;
    const int band_lo = rel(ddw >> 5), band_hi = rel((ddw + NW * 32 + 31) >> 5);
    const unsigned soff = (unsigned)((tid / (D / 4)) * LDY + (tid % (D / 4)) * 4) * 4u;  // store_tile's address, i = 0
    const unsigned yoff = (unsigned)tid * 16u, goff = (unsigned)((4 * hh) * 32 + r31) * 4u;
    constexpr int YB = TSW * D * 4;  // bytes per swept tile
    int rt = (int)(tile - t0);
    auto steady_tile = [&](int p, __amdgpu_buffer_rsrc_t ry, const float* gblk, const f32x16& sa, f32x16& sb) {
      const int cur = p % 3, nxt = (p + 1) % 3, pre = (p + 2) % 3;
#pragma unroll
      for (int i = 0; i < NV; ++i) stage[i] = buffer_load_f32x4(ry, yoff, p * YB + i * NT * 16);
      float g[16];
      sb = zero16();
      fast_block(Ysh[nxt], cur, sa, sb, g);
      const __amdgpu_buffer_rsrc_t rg = buffer_rsrc(gblk, 4096);
      gy_block(Ysh[cur], g, [&](int krow, float v) {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rg, (int)goff, krow * 128, 0);
      });
#pragma unroll
      for (int i = 0; i < NV; ++i)
        *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(Ysh[pre]) + (soff + i * (NT / (D / 4)) * LDY * 4)) = stage[i];
      __syncthreads();
    };
#pragma unroll 1
    for (;;) {
      int n = 0;  // steady tiles from here (a multiple of 6)
      if (it == 0) {
        const int end = rt < band_lo ? (band_lo < s_lim ? band_lo : s_lim) : (rt >= band_hi ? s_lim : rt);
        n = end > rt ? (end - rt) / 6 * 6 : 0;
      }
      if (n > 0) {
        const float* yt = a.Ys + (tile + 2) * (TSW * D);  // tile + 2 of the trip's first tile
        const size_t gstep = (size_t)a.g_ub * 1024;
        const float* gt = a.gmat + ((size_t)tile * a.g_ub + (size_t)blockIdx.x * NW + w) * 1024;
        scalar_loads_done();
#pragma unroll 1
        for (int k = n; k > 0; k -= 6) {
          const __amdgpu_buffer_rsrc_t ry = buffer_rsrc(yt, 6 * YB);
          f32x16 sn;
          steady_tile(0, ry, gt, st, sn);
          steady_tile(1, ry, gt + gstep, sn, st);
          steady_tile(2, ry, gt + 2 * gstep, st, sn);
          steady_tile(3, ry, gt + 3 * gstep, sn, st);
          steady_tile(4, ry, gt + 4 * gstep, st, sn);
          steady_tile(5, ry, gt + 5 * gstep, sn, st);
          yt += 6 * TSW * D;
          gt += 6 * gstep;
        }
        tile += n;
        rt += n;
      }
      if (rt >= ntl) break;
      general_tile();
      ++rt;
    }
  }

  // ---- epilogue
  if (t0 < t1) {
    const float rr = (r_acc + __shfl_xor(r_acc, 32, 64)) * a.c;  // both halves hold the same owner column
    if (hh == 0) rsum[w][r31] = rr;
    if (MODE_USER) {
      const float ls = wave_sum(loss_acc);
      if (lane == 0) red_loss[w] = (double)ls * (double)RIHIP_LN2;  // log2 units -> nats
    }
  }
  __syncthreads();
  const bool final_pass = (a.nsplit == 1);
  float* dst = final_pass ? a.dOwner : a.slab + (size_t)blockIdx.y * a.No * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = acc_row(r, lane);
    const int64_t orow = o_base + o;
    if (orow < a.No) {
      const int64_t drow = a.o_goff + orow - a.s_goff;  // owner's positive partner inside the swept set
      const bool fix = final_pass && MODE_USER && drow >= 0 && drow < a.Ns;
      const float rs = rsum[w][o];
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        float v = out[t][r] * a.c;
        if (fix) v -= rs * a.Ys[drow * D + r31 * CT + t];  // G_ii = -sum_{j!=i} G_ij
        dst[orow * D + r31 * CT + t] = v;
      }
    }
  }
  if (MODE_USER && hh == 0 && o_ok) {
    if (final_pass) a.r_out[o_loc] = rsum[w][r31];
    else a.r_part[(size_t)blockIdx.y * a.No + o_loc] = rsum[w][r31];
  }
  // loss partials keep the 128-owner granularity of rihip_inbatch_loss_parts() whatever the workgroup size
  if (MODE_USER && tid < NW / 4) {
    const int64_t gx128 = (a.No + OW - 1) / OW;
    const int64_t slot = (int64_t)blockIdx.x * (NW / 4) + tid;
    if (slot < gx128)
      a.loss_part[(size_t)blockIdx.y * gx128 + slot] =
          ((red_loss[4 * tid] + red_loss[4 * tid + 1]) + red_loss[4 * tid + 2]) + red_loss[4 * tid + 3];
  }
}

// nsplit>1: dOwner = sum_s slab[s] (- r * Y[diag] in user mode); r_out = sum_s r_part[s]   (fixed order)
template <bool MODE_USER>
__global__ __launch_bounds__(256) void sweep_finish_kernel(SweepArgs a, int d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one float4 of one owner row
  const int v4 = d / 4;
  if (i >= a.No * v4) return;
  const int64_t orow = i / v4;
  const int c4 = (int)(i % v4);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < a.nsplit; ++s) {
    const f32x4 u = reinterpret_cast<const f32x4*>(a.slab + ((size_t)s * a.No + orow) * d)[c4];
    acc.x += u.x; acc.y += u.y; acc.z += u.z; acc.w += u.w;
  }
  if (MODE_USER) {
    float rs = 0.f;
    for (int s = 0; s < a.nsplit; ++s) rs += a.r_part[(size_t)s * a.No + orow];
    const int64_t drow = a.o_goff + orow - a.s_goff;
    if (drow >= 0 && drow < a.Ns) {
      const f32x4 y = reinterpret_cast<const f32x4*>(a.Ys + drow * d)[c4];
      acc.x -= rs * y.x; acc.y -= rs * y.y; acc.z -= rs * y.z; acc.w -= rs * y.w;
    }
    if (c4 == 0) a.r_out[orow] = rs;
  }
  reinterpret_cast<f32x4*>(a.dOwner + orow * d)[c4] = acc;
}


// ------------------------------------------------------------------------------------------
// item gradients from the stored G:  dI[j][:] = sum_i G[i][j] * U[i][:]  - r_j U_j   (plain exact-f32 GEMM)
// owners = items (4 waves x 32 per workgroup, one 32x32 G^T block per wave and swept tile, loaded straight into the
// MFMA A-operand registers: lane (item, hh) holds users 16*hh .. 16*hh+15 of its item = 64 contiguous bytes);
// swept = the local users, staged through the same 3-buffer LDS pipeline as the sweep kernel.
// ------------------------------------------------------------------------------------------
template <int D, int NW>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 3 : 2) void inbatch_gt_kernel(SweepArgs a) {
  constexpr int NT = NW * 64;
  constexpr int LDY = D + 4;
  constexpr int CT = D / 32;
  constexpr int NV = (TSW * (D / 4) + NT - 1) / NT;
  __shared__ __attribute__((aligned(16))) float Ysh[3][TSW * LDY];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r31 = lane & 31, hh = lane >> 5;
  const int64_t o_base = (int64_t)blockIdx.x * (NW * 32) + w * 32;

  f32x16 out[CT];
#pragma unroll
  for (int t = 0; t < CT; ++t) out[t] = zero16();

  const int64_t ntiles = (a.Ns + TSW - 1) / TSW;
  const int64_t per = (ntiles + a.nsplit - 1) / a.nsplit;
  const int64_t t0 = (int64_t)blockIdx.y * per;
  const int64_t t1 = (t0 + per < ntiles) ? t0 + per : ntiles;

  f32x4 stage[NV];
  auto load_tile = [&](int64_t tile) {
    const int64_t s_base = tile * TSW;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * NT;
      const int r = idx / (D / 4), c4 = idx % (D / 4);
      const int64_t srow = s_base + r;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (idx < TSW * (D / 4) && srow < a.Ns) v = reinterpret_cast<const f32x4*>(a.Ys + srow * D)[c4];
      stage[i] = v;
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int idx = tid + i * NT;
      const int r = idx / (D / 4), c4 = idx % (D / 4);
      if (idx < TSW * (D / 4)) *reinterpret_cast<f32x4*>(&Ysh[buf][r * LDY + c4 * 4]) = stage[i];
    }
  };
  // this wave's G^T block row; consecutive swept tiles are consecutive 4 KB blocks
  const f32x4* gp = reinterpret_cast<const f32x4*>(a.gmat + ((size_t)(blockIdx.x * NW + w) * a.g_ub) * 1024 +
                                                   r31 * 32 + 16 * hh);
  // Pipeline: the user tile t+2 and the G block t+2 are requested at the top of iteration t; the tile sits in
  // registers for one whole iteration and goes to LDS at the top of iteration t+1 (published by that iteration's
  // barrier, read in iteration t+2).  vmcnt retires in order, so the wait for a tile only covers requests that are
  // at least one full iteration (64 MFMAs per wave) old -- the HBM stream of G never stalls the L2-resident tile.
  // G of tile, tile+1, ..., tile+GA.  With d <= 64 a tile is only 32 MFMAs per wave (0.85 us): the HBM stream of G needs
  // four tiles of lead there, two at d = 128.
  constexpr int GA = (D >= 128) ? 2 : 4;
  f32x4 gs[GA + 1][4];
#pragma unroll
  for (int j = 0; j <= GA; ++j)
#pragma unroll
    for (int q = 0; q < 4; ++q) gs[j][q] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (t0 < t1) {
#pragma unroll
    for (int j = 0; j < GA; ++j)
      if (t0 + j < t1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) gs[j][q] = gp[(size_t)(t0 + j) * 256 + q];
      }
    load_tile(t0);
    store_tile(0);
    if (t0 + 1 < t1) load_tile(t0 + 1);  // stays in registers until the top of the first iteration
    __syncthreads();
  }
  // out += G(tile)^T . Y(tile): lane (r31, hh) consumes k-rows 16 hh .. 16 hh + 15 in order; row j + LEAD is requested
  // before row j's MFMAs
  // early_barrier: the tile's barrier goes in front of the last k-row's MFMAs (they read registers only), where the
  // wait for that row's operands -- the last read in flight, so a full lgkmcnt(0) -- is the barrier's own
  auto gy_tile = [&](int cur, const f32x4 (&g)[4], bool early_barrier) {
    const float* Yb = Ysh[cur] + 16 * hh * LDY + r31 * CT;
    // k-rows read ahead: 16 MFMAs (about 1000 cycles) of lead, 8 under the 168-VGPR cap of the 3-wave form and at
    // d = 32 (where a lead of the whole tile leaves the scheduler no room and it falls back to a wait per read)
    constexpr int LEAD = (NW == 4 || CT == 1 ? 8 : 16) / CT;
    BRow<CT> yb[16];
#pragma unroll
    for (int j = 0; j < LEAD; ++j) yb[j] = lds_brow<CT>(Yb + j * LDY);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      if (j + LEAD < 16) yb[j + LEAD] = lds_brow<CT>(Yb + (j + LEAD) * LDY);
      if (early_barrier && j == 15) __syncthreads();
#pragma unroll
      for (int t = 0; t < CT; ++t) out[t] = mfma32(g[j >> 2][j & 3], yb[j].v[t], out[t]);
    }
    brow_schedule<CT, LEAD>(16);
  };
  // Steady tiles (GT_STEADY instantiations): tile + 2 is a full tile of this split, so every load of the iteration
  // is unconditional.  They run in a loop of three tiles per trip (the period of the LDS ring and, with GA = 2, of
  // the G ring), so buffer indices and the gs[] names are static and nothing is copied; the swept rows and the G
  // blocks are addressed as a uniform base that advances by one tile plus a constant 32-bit lane offset.  The
  // one-tile code runs whatever is left: the last tiles of the split and ragged swept ranges.
  constexpr bool STEADY = GT_STEADY(D, NW);
  int64_t tile = t0;
  int it = 0;
  auto general_tile = [&]() {
    const int cur = it, nxt = (it + 1) % 3;
    if (tile + 1 < t1) store_tile(nxt);  // buffer nxt was last read two iterations ago
    if (tile + 2 < t1) load_tile(tile + 2);
    if (tile + GA < t1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) gs[GA][q] = gp[(size_t)(tile + GA) * 256 + q];
    }
    gy_tile(cur, gs[0], false);
#pragma unroll
    for (int j = 0; j < GA; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) gs[j][q] = gs[j + 1][q];
    __syncthreads();
    ++tile;
    it = (it == 2 ? 0 : it + 1);
  };
  // The one-tile loop: every tile of the instantiations without a steady loop, the first three otherwise (one turn
  // of the ring, so that the steady loop starts at phase 0 like t0 does).
  const int64_t lead_end = (STEADY && t0 + 3 < t1) ? t0 + 3 : t1;
  scalar_loads_done();
#pragma unroll 1
  while (tile < lead_end) general_tile();
  if constexpr (STEADY) {
    static_assert(!STEADY || (GA == 2 && (TSW * (D / 4)) % NT == 0), "three-tile period, whole float4 rows");
    const int64_t nfull = a.Ns / TSW;
    const int64_t s_lim = (t1 < nfull ? t1 : nfull) - 2;
    const int64_t s_end = s_lim > tile ? tile + (s_lim - tile) / 3 * 3 : tile;
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const float* yt = a.Ys + (tile + 2) * (TSW * D);  // tile + 2 of the trip's first tile
    const float* gt = a.gmat + ((size_t)(blockIdx.x * NW + wu) * a.g_ub + (tile + 2)) * 1024;
    const unsigned soff = (unsigned)((tid / (D / 4)) * LDY + (tid % (D / 4)) * 4) * 4u;  // store_tile's address, i = 0
    const unsigned yoff = (unsigned)tid * 16u, goff = (unsigned)(r31 * 32 + 16 * hh) * 4u;
    constexpr int YB = TSW * D * 4, GB = 4096;  // bytes per swept tile, per G block
    auto steady_tile = [&](int p, __amdgpu_buffer_rsrc_t ry, __amdgpu_buffer_rsrc_t rg) {  // p = tile % 3, static
#pragma unroll
      for (int i = 0; i < NV; ++i)
        *reinterpret_cast<f32x4*>(reinterpret_cast<char*>(Ysh[(p + 1) % 3]) + (soff + i * (NT / (D / 4)) * LDY * 4)) = stage[i];
#pragma unroll
      for (int i = 0; i < NV; ++i) stage[i] = buffer_load_f32x4(ry, yoff, p * YB + i * NT * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) gs[(p + 2) % 3][q] = buffer_load_f32x4(rg, goff, p * GB + 16 * q);
      __builtin_amdgcn_sched_group_barrier(0x200, NV, 0);      // DS write, then the VMEM reads: a full tile (and
      __builtin_amdgcn_sched_group_barrier(0x020, NV + 4, 0);  // for G two) ahead of their use, as in the one-tile loop
      gy_tile(p, gs[p], true);
    };
    scalar_loads_done();
#pragma unroll 1
    for (int n = (int)(s_end - tile); n > 0; n -= 3) {
      const __amdgpu_buffer_rsrc_t ry = buffer_rsrc(yt, 3 * YB), rg = buffer_rsrc(gt, 3 * GB);
      steady_tile(0, ry, rg);
      steady_tile(1, ry, rg);
      steady_tile(2, ry, rg);
      yt += 3 * TSW * D;
      gt += 3 * 1024;
    }
    tile = s_end;
    scalar_loads_done();
#pragma unroll 1
    while (tile < t1) general_tile();  // the last tiles of the split and ragged swept ranges
  }

  const bool final_pass = (a.nsplit == 1);
  float* dst = final_pass ? a.dOwner : a.slab + (size_t)blockIdx.y * a.No * D;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t orow = o_base + acc_row(r, lane);
    if (orow < a.No) {
      const int64_t drow = a.o_goff + orow - a.s_goff;  // the item's own user inside the swept (local) users
      const bool fix = final_pass && drow >= 0 && drow < a.Ns;
      const float rs = fix ? a.r_in[drow] : 0.f;
#pragma unroll
      for (int t = 0; t < CT; ++t) {
        float v = out[t][r] * a.c;                          // the stored weights are unscaled sigma(z)
        if (fix) v -= rs * a.Ys[drow * D + r31 * CT + t];  // G_jj = -r_j
        dst[orow * D + r31 * CT + t] = v;
      }
    }
  }
}

// nsplit>1 finish of the stored-G item pass: dOwner = sum_s slab[s] - r * U[diag]   (fixed order)
__global__ __launch_bounds__(256) void gt_finish_kernel(SweepArgs a, int d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int v4 = d / 4;
  if (i >= a.No * v4) return;
  const int64_t orow = i / v4;
  const int c4 = (int)(i % v4);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < a.nsplit; ++s) {
    const f32x4 u = reinterpret_cast<const f32x4*>(a.slab + ((size_t)s * a.No + orow) * d)[c4];
    acc.x += u.x; acc.y += u.y; acc.z += u.z; acc.w += u.w;
  }
  const int64_t drow = a.o_goff + orow - a.s_goff;
  if (drow >= 0 && drow < a.Ns) {
    const float rs = a.r_in[drow];
    const f32x4 y = reinterpret_cast<const f32x4*>(a.Ys + drow * d)[c4];
    acc.x -= rs * y.x; acc.y -= rs * y.y; acc.z -= rs * y.z; acc.w -= rs * y.w;
  }
  reinterpret_cast<f32x4*>(a.dOwner + orow * d)[c4] = acc;
}

template <int D>
void launch_sweep(bool mode_user, const SweepArgs& a, dim3 grid, int nw, hipStream_t st) {
  if (nw == 8) {
    if (mode_user && a.gmat) hipLaunchKernelGGL((inbatch_sweep_kernel<D, true, true, 8>), grid, dim3(512), 0, st, a);
    else if (mode_user) hipLaunchKernelGGL((inbatch_sweep_kernel<D, true, false, 8>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((inbatch_sweep_kernel<D, false, false, 8>), grid, dim3(512), 0, st, a);
    return;
  }
  if (mode_user && a.gmat) hipLaunchKernelGGL((inbatch_sweep_kernel<D, true, true>), grid, dim3(256), 0, st, a);
  else if (mode_user) hipLaunchKernelGGL((inbatch_sweep_kernel<D, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((inbatch_sweep_kernel<D, false>), grid, dim3(256), 0, st, a);
}

// workgroup shape: 8 waves x 32 owners (one workgroup per CU) once the problem is large enough to fill the chip that
// way -- the swept tile is then fetched once per 256 owners instead of once per 128; 4 waves otherwise.
int sweep_nw(int64_t n_owner, int64_t n_swept) {
  static const char* ev = getenv("RIHIP_SWEEP_NW");
  if (ev) return atoi(ev) == 8 ? 8 : 4;
  return (n_owner >= 4096 && n_swept >= 16384) ? 8 : 4;   // (8192 x 8192 at d = 64 measured 2 % faster with 4 waves)
}

// swept-range splits (bounded by the 128-owner formula: the workspace / loss-part sizes are computed from it)
int sweep_nsplit(int64_t n_owner, int64_t n_swept, int nw = 4) {
  const int64_t tiles = (n_swept + TSW - 1) / TSW;
  const int64_t gx4 = (n_owner + OW - 1) / OW;
  int64_t ns4 = (2 * RIHIP_NCU + gx4 - 1) / gx4;  // 4-wave workgroups: aim at >= 2 workgroups per CU
  if (ns4 > 16) ns4 = 16;
  if (ns4 > tiles) ns4 = tiles;
  if (ns4 < 1) ns4 = 1;
  if (nw == 4) return (int)ns4;
  const int64_t gx8 = (n_owner + 2 * OW - 1) / (2 * OW);
  int64_t ns = (RIHIP_NCU + gx8 - 1) / gx8;      // 8-wave workgroups: >= 1 per CU
  if (ns > ns4) ns = ns4;
  if (ns < 1) ns = 1;
  return (int)ns;
}

}  // namespace

extern "C" int rihip_bpr_pair_loss(const float* U, const float* P, const float* N, int64_t B, int d, float* loss,
                                   float* dU, float* dP, float* dN, double* workspace, void* stream) {
  RIHIP_REQUIRE(U && P && N && dU && dP && dN && workspace, RIHIP_ERR_ARG, "bpr_pair_loss: null pointer");
  RIHIP_REQUIRE(B > 0 && d > 0, RIHIP_ERR_ARG, "bpr_pair_loss: bad sizes B=%lld d=%d", (long long)B, d);
  hipStream_t st = (hipStream_t)stream;
  const int64_t nb = (B + 3) / 4;
  const int grid = (int)(nb < 1024 ? nb : 1024);
  const bool al = ((reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(N) |
                    reinterpret_cast<uintptr_t>(dU) | reinterpret_cast<uintptr_t>(dP) | reinterpret_cast<uintptr_t>(dN)) & 15) == 0;
  const float inv_B = 1.f / (float)B;
  if (al && d == 128) hipLaunchKernelGGL((bpr_pair_v4_kernel<32>), dim3(grid), dim3(256), 0, st, U, P, N, B, inv_B, dU, dP, dN, workspace);
  else if (al && d == 64) hipLaunchKernelGGL((bpr_pair_v4_kernel<16>), dim3(grid), dim3(256), 0, st, U, P, N, B, inv_B, dU, dP, dN, workspace);
  else if (al && d == 32) hipLaunchKernelGGL((bpr_pair_v4_kernel<8>), dim3(grid), dim3(256), 0, st, U, P, N, B, inv_B, dU, dP, dN, workspace);
  else hipLaunchKernelGGL(bpr_pair_kernel, dim3(grid), dim3(256), 0, st, U, P, N, B, d, inv_B, dU, dP, dN, workspace);
  RIHIP_CHECK_LAUNCH();
  // loss == NULL: the caller sums workspace[0 .. rihip_bpr_pair_nparts(B)) * (1/B) itself (rihip_sum_partials or
  // rihip_clip_coef_step) -- one dependent launch less on the step's critical path
  if (loss) hipLaunchKernelGGL(finalize_sum_kernel, dim3(1), dim3(64), 0, st, workspace, grid, 1.0 / (double)B, loss);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

extern "C" int64_t rihip_bpr_pair_nparts(int64_t B) {
  const int64_t nb = (B + 3) / 4;
  return nb < 1024 ? (nb > 0 ? nb : 1) : 1024;
}

extern "C" int rihip_rowdot(const float* U, const float* I, int64_t B, int64_t i_offset, int d, float* pos,
                            void* stream) {
  RIHIP_REQUIRE(U && I && pos && B > 0 && d > 0, RIHIP_ERR_ARG, "rowdot: bad arguments");
  const int64_t nb = (B + 3) / 4;
  const int grid = (int)(nb < 1024 ? nb : 1024);
  hipLaunchKernelGGL(rowdot_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, U, I, B, i_offset, d, pos);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

// loss partials written per sweep (doubles) and float workspace (split slabs) needed by rihip_inbatch_sweep
extern "C" int64_t rihip_inbatch_workspace_doubles(int64_t n_owner) { return ((n_owner + OW - 1) / OW) * 16 + 1; }
extern "C" int64_t rihip_inbatch_loss_parts(int64_t n_owner, int64_t n_swept) {
  return ((n_owner + OW - 1) / OW) * sweep_nsplit(n_owner, n_swept, sweep_nw(n_owner, n_swept));
}
extern "C" int64_t rihip_inbatch_workspace_floats(int64_t n_owner, int64_t n_swept, int d) {
  const int ns = sweep_nsplit(n_owner, n_swept);
  return ns > 1 ? (int64_t)ns * n_owner * (d + 1) : 1;
}

extern "C" int rihip_inbatch_sweep(int mode_user, const float* owners, int64_t n_owner, int64_t owner_goff,
                                   const float* swept, int64_t n_swept, int64_t swept_goff, int d, const float* pos,
                                   const float* r_in, int64_t n_global, float* d_owner, float* r_out,
                                   double* loss_part, float* workspace, int precision, void* stream) {
  const bool tuned = d == 32 || d == 64 || d == 128;
  RIHIP_REQUIRE(tuned || rihip_inbatch_generic_ok(d), RIHIP_ERR_SHAPE,
                "inbatch_sweep: unsupported embed_dim=%d (multiples of 16 up to 256)", d);
  RIHIP_REQUIRE(tuned || precision == 0, RIHIP_ERR_SHAPE,
                "inbatch_sweep: the split-bf16 modes exist for embed_dim 32/64/128 only (embed_dim=%d)", d);
  RIHIP_REQUIRE(precision >= 0 && precision <= 2, RIHIP_ERR_ARG,
                "inbatch_sweep: precision=%d (0=f32 MFMA, 1=bf16x3, 2=bf16x6)", precision);
  RIHIP_REQUIRE(owners && swept && pos && d_owner, RIHIP_ERR_ARG, "inbatch_sweep: null pointer");
  RIHIP_REQUIRE(mode_user ? (r_out && loss_part) : (r_in != nullptr), RIHIP_ERR_ARG,
                "inbatch_sweep: mode-specific pointer missing");
  RIHIP_REQUIRE(n_owner > 0 && n_swept > 0 && n_global >= 2, RIHIP_ERR_ARG,
                "inbatch_sweep: sizes No=%lld Ns=%lld B=%lld", (long long)n_owner, (long long)n_swept,
                (long long)n_global);
  SweepArgs a;
  a.Xo = owners; a.No = n_owner; a.o_goff = owner_goff; a.Ys = swept; a.Ns = n_swept; a.s_goff = swept_goff;
  a.pos = pos; a.r_in = r_in; a.c = (float)(1.0 / ((double)n_global * (double)(n_global - 1)));
  a.dOwner = d_owner; a.r_out = r_out; a.loss_part = loss_part;
  a.gmat = nullptr; a.g_ub = 0;
  const int nw_f32 = sweep_nw(n_owner, n_swept);
  const int nw = precision == 1 ? 4 : nw_f32;   // the split-bf16 kernel has 4-wave workgroups only
  a.nsplit = sweep_nsplit(n_owner, n_swept, nw_f32);
  RIHIP_REQUIRE(a.nsplit == 1 || workspace, RIHIP_ERR_ARG, "inbatch_sweep: workspace required (nsplit=%d)", a.nsplit);
  a.slab = workspace;
  a.r_part = workspace ? workspace + (size_t)a.nsplit * n_owner * d : nullptr;
  const dim3 grid((unsigned)((n_owner + nw * 32 - 1) / (nw * 32)), (unsigned)a.nsplit);
  hipStream_t st = (hipStream_t)stream;
  if (!tuned) {   // runtime-width kernel: final results in one launch (it fills every loss slot of the tuned layout)
    rihip_launch_sweep_generic(d, mode_user != 0, a, a.nsplit, st);
    RIHIP_CHECK_LAUNCH();
    return RIHIP_OK;
  }
  if (precision == 1) rihip_launch_sweep_bf16x3(d, mode_user != 0, a, grid, st);
  else if (precision == 2) rihip_launch_sweep_x6(d, mode_user != 0, a, grid, nw, st);
  else if (d == 32) launch_sweep<32>(mode_user != 0, a, grid, nw, st);
  else if (d == 64) launch_sweep<64>(mode_user != 0, a, grid, nw, st);
  else launch_sweep<128>(mode_user != 0, a, grid, nw, st);
  RIHIP_CHECK_LAUNCH();
  if (a.nsplit > 1) {
    const int64_t n4 = n_owner * (d / 4);
    if (mode_user) hipLaunchKernelGGL((sweep_finish_kernel<true>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a, d);
    else hipLaunchKernelGGL((sweep_finish_kernel<false>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a, d);
    RIHIP_CHECK_LAUNCH();
  }
  return RIHIP_OK;
}

// ---- stored-G variant: user pass writes G, item pass is a plain G^T.U product --------------------------------------
extern "C" int64_t rihip_inbatch_gmat_floats(int64_t n_users, int64_t n_items) {
  const int64_t ub = 8 * ((n_users + 2 * OW - 1) / (2 * OW)), ib = 8 * ((n_items + 2 * OW - 1) / (2 * OW));
  return ub * ib * 1024;
}

extern "C" int rihip_inbatch_user_pass(const float* users, int64_t n_users, int64_t user_goff, const float* items,
                                       int64_t n_items, int64_t item_goff, int d, const float* pos, int64_t n_global,
                                       float* d_users, float* r_out, double* loss_part, float* workspace, float* gmat,
                                       int precision, void* stream) {
  RIHIP_REQUIRE(d == 32 || d == 64 || d == 128, RIHIP_ERR_SHAPE,
                "inbatch_user_pass: the stored-G form exists for embed_dim 32/64/128 only (embed_dim=%d: use rihip_inbatch_sweep)", d);
  RIHIP_REQUIRE(users && items && pos && d_users && r_out && loss_part && gmat, RIHIP_ERR_ARG,
                "inbatch_user_pass: null pointer");
  RIHIP_REQUIRE(precision == 0 || precision == 2, RIHIP_ERR_ARG,
                "inbatch_user_pass: precision=%d (0=f32 MFMA, 2=bf16x6)", precision);
  RIHIP_REQUIRE(n_users > 0 && n_items > 0 && n_global >= 2, RIHIP_ERR_ARG,
                "inbatch_user_pass: sizes users=%lld items=%lld B=%lld", (long long)n_users, (long long)n_items,
                (long long)n_global);
  SweepArgs a;
  a.Xo = users; a.No = n_users; a.o_goff = user_goff; a.Ys = items; a.Ns = n_items; a.s_goff = item_goff;
  a.pos = pos; a.r_in = nullptr; a.c = (float)(1.0 / ((double)n_global * (double)(n_global - 1)));
  a.dOwner = d_users; a.r_out = r_out; a.loss_part = loss_part;
  a.gmat = gmat; a.g_ub = 8 * ((n_users + 2 * OW - 1) / (2 * OW));
  const int nw = sweep_nw(n_users, n_items);
  a.nsplit = sweep_nsplit(n_users, n_items, nw);
  RIHIP_REQUIRE(a.nsplit == 1 || workspace, RIHIP_ERR_ARG, "inbatch_user_pass: workspace required (nsplit=%d)", a.nsplit);
  a.slab = workspace;
  a.r_part = workspace ? workspace + (size_t)a.nsplit * n_users * d : nullptr;
  const dim3 grid((unsigned)((n_users + nw * 32 - 1) / (nw * 32)), (unsigned)a.nsplit);
  hipStream_t st = (hipStream_t)stream;
  if (precision == 2) rihip_launch_sweep_x6(d, true, a, grid, nw, st);
  else if (d == 32) launch_sweep<32>(true, a, grid, nw, st);
  else if (d == 64) launch_sweep<64>(true, a, grid, nw, st);
  else launch_sweep<128>(true, a, grid, nw, st);
  RIHIP_CHECK_LAUNCH();
  if (a.nsplit > 1) {
    const int64_t n4 = n_users * (d / 4);
    hipLaunchKernelGGL((sweep_finish_kernel<true>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a, d);
    RIHIP_CHECK_LAUNCH();
  }
  return RIHIP_OK;
}

extern "C" int rihip_inbatch_item_pass(const float* gmat, const float* users, int64_t n_users, int64_t user_goff,
                                       int64_t n_items, int64_t item_goff, int d, const float* r, int64_t n_global,
                                       float* d_items, float* workspace, int precision, void* stream) {
  RIHIP_REQUIRE(d == 32 || d == 64 || d == 128, RIHIP_ERR_SHAPE, "inbatch_item_pass: unsupported embed_dim=%d", d);
  RIHIP_REQUIRE(gmat && users && r && d_items, RIHIP_ERR_ARG, "inbatch_item_pass: null pointer");
  RIHIP_REQUIRE(precision == 0 || precision == 2, RIHIP_ERR_ARG,
                "inbatch_item_pass: precision=%d (0=f32 MFMA, 2=bf16x6)", precision);
  RIHIP_REQUIRE(n_users > 0 && n_items > 0 && n_global >= 2, RIHIP_ERR_ARG,
                "inbatch_item_pass: sizes users=%lld items=%lld B=%lld", (long long)n_users, (long long)n_items,
                (long long)n_global);
  SweepArgs a;
  a.Xo = nullptr; a.No = n_items; a.o_goff = item_goff; a.Ys = users; a.Ns = n_users; a.s_goff = user_goff;
  a.pos = nullptr; a.r_in = r; a.c = (float)(1.0 / ((double)n_global * (double)(n_global - 1))); a.dOwner = d_items; a.r_out = nullptr; a.loss_part = nullptr;
  a.gmat = const_cast<float*>(gmat); a.g_ub = 8 * ((n_users + 2 * OW - 1) / (2 * OW));
  // 8-wave workgroups (256 items) halve the L2->L1 traffic of the swept user tiles; used when they still fill the chip
  const int nw = sweep_nw(n_items, n_users);
  const int ow = nw * 32;
  const int64_t gx = (n_items + ow - 1) / ow;
  a.nsplit = sweep_nsplit(n_items, n_users, nw);
  RIHIP_REQUIRE(a.nsplit == 1 || workspace, RIHIP_ERR_ARG, "inbatch_item_pass: workspace required (nsplit=%d)", a.nsplit);
  a.slab = workspace; a.r_part = nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)gx, (unsigned)a.nsplit);
  if (precision == 2) {
    rihip_launch_gt_x6(d, a, grid, nw, st);
  } else if (nw == 8) {
    if (d == 32) hipLaunchKernelGGL((inbatch_gt_kernel<32, 8>), grid, dim3(512), 0, st, a);
    else if (d == 64) hipLaunchKernelGGL((inbatch_gt_kernel<64, 8>), grid, dim3(512), 0, st, a);
    else hipLaunchKernelGGL((inbatch_gt_kernel<128, 8>), grid, dim3(512), 0, st, a);
  } else {
    if (d == 32) hipLaunchKernelGGL((inbatch_gt_kernel<32, 4>), grid, dim3(256), 0, st, a);
    else if (d == 64) hipLaunchKernelGGL((inbatch_gt_kernel<64, 4>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((inbatch_gt_kernel<128, 4>), grid, dim3(256), 0, st, a);
  }
  RIHIP_CHECK_LAUNCH();
  if (a.nsplit > 1) {
    const int64_t n4 = n_items * (d / 4);
    hipLaunchKernelGGL(gt_finish_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, a, d);
    RIHIP_CHECK_LAUNCH();
  }
  return RIHIP_OK;
}

extern "C" int rihip_sum_partials(const double* part, int64_t n, double scale, float* out, void* stream) {
  RIHIP_REQUIRE(part && out && n > 0, RIHIP_ERR_ARG, "sum_partials: bad arguments");
  hipLaunchKernelGGL(finalize_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, part, (int)n, scale, out);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}
