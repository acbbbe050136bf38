// bf16 filter of the two-precision flat search, its threshold-sample passes, and the bf16 copy of the corpus they read.
#include "search_kernels.h"
#include "search_keys.h"

#include <math.h>
#include <string.h>

using namespace rihip_index;

namespace {

// ---------------------------------------------------------------------------------------------------------
// Two-precision exact search for large corpora: FILTER on plain-bf16 MFMA (16x fewer matrix cycles than exact
// f32), then RE-SCORE the few survivors in exact f32.  |s - s_bf16| <= (2^-8 + 2^-18) |q| |x| (each operand
// rounded to bf16 with relative error <= 2^-9), so rows outside the candidate set {s_bf16 >= thr} have exact
// score < thr + eps; if the k-th exact score of the candidates is >= thr + eps the top-k is proven complete,
// otherwise the query takes the exact-f32 fallback.  Results are therefore bit-identical to the all-f32 search.
// ---------------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

__global__ void to_bf16_kernel(const float* __restrict__ x, int64_t n, __bf16* __restrict__ y) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < n) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
    y[i] = (__bf16)v.x; y[i + 1] = (__bf16)v.y; y[i + 2] = (__bf16)v.z; y[i + 3] = (__bf16)v.w;
  } else {
    for (int64_t j = i; j < n; ++j) y[j] = (__bf16)x[j];
  }
}
// max over rows of |x_row|^2 (order-independent: max of non-negative floats via int atomicMax)
__global__ __launch_bounds__(256) void rownorm_max_kernel(const float* __restrict__ X, int64_t N, int d, int* out_bits) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float best = 0.f;
  for (int64_t row = (int64_t)blockIdx.x * 4 + w; row < N; row += (int64_t)gridDim.x * 4) {
    float s = 0.f;
    for (int k = lane; k < d; k += 64) { const float v = X[row * d + k]; s += v * v; }
    s = wave_sum(s);
    best = fmaxf(best, s);
  }
  if (lane == 0) atomicMax(out_bits, __float_as_int(best));
}

#ifndef RIHIP_SCAN_ABLATE
#define RIHIP_SCAN_ABLATE 0
#endif
constexpr int WQE = 192;    // survivor queue: 16-byte entries (score, row, query) per WAVE (LDS)

__device__ __forceinline__ float max3_raw(float a, float b, float c) {  // no NaN-canonicalising pre-ops
  float m;
  asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(m) : "v"(a), "v"(b), "v"(c));
  return m;
}

// DENSE=false: survivors (score >= thr[q]) are queued in LDS and flushed to the per-query candidate lists now and then,
// so the hot loop contains no global store/atomic (those make hipcc drain the in-flight prefetch with vmcnt(0)).
// MODE 1 (dense): every score is stored at slot = virtual row (threshold-sample pass for large k).
// MODE 2 (top-T sample): every lane keeps the SAMPLE_T best scores of its stream (query, split, half of the rows) in
// registers and writes only those: the r-th largest of the union is a LOWER bound of the sample's r-th largest (a
// subset can only lose large scores), i.e. a safe threshold, and the sample pass writes 100x less.
// (launch bounds: the filter (MODE 0) wants 3 workgroups per CU even at the price of 72 spilled registers -- 2 per CU
// measured 2.27 instead of 2.04 ms per batch; the short sample passes spilled 130-250 registers at that bound and run
// 1.6x faster with 2 per CU and none)
template <int D, int MODE>
__global__ __launch_bounds__(256, MODE == 0 ? 3 : 2) void scan_bf16_kernel(ScanArgs a) {
  constexpr bool DENSE = MODE != 0;
  constexpr int LDB = D + 8, KB = D / 16;
  constexpr int NV = (TRB * (D / 8) + 255) / 256;  // 16-byte pieces staged per thread per stage
  __shared__ __attribute__((aligned(16))) __bf16 Xs[2][TRB * LDB];
  // A survivor is rare per lane but not per 64-lane wave (a wave meets one in ~90 % of its 16-score columns at k = 500),
  // so the hot path must neither wait nor synchronise.  A column whose maximum passes the threshold is scanned score by
  // score; the lanes holding a survivor write ONE 16-byte entry (score, row, query) each into their WAVE's private queue
  // at a slot computed from the compare mask (no LDS atomic, no returning operation: with a workgroup-wide atomic
  // counter this path cost more than the MFMA work).  Until round 3 the whole 16-score column was dumped (4 x
  // ds_write_b128 + 2 header words per column, thresholded again in the flush): those six LDS instructions per column
  // loaded the LDS pipe as much as the MFMA operand reads did, and the 72-byte columns filled the queue nine times
  // sooner.
  __shared__ __attribute__((aligned(16))) uint4 qent[DENSE ? 1 : 4][DENSE ? 1 : WQE];
  __shared__ int qcntS[DENSE ? 1 : QBB];    // survivors of each query in this corpus split (one writer wave each)
  __shared__ unsigned wcnt[2][4];           // queue lengths published at the stage barrier, double-buffered by parity
  int wpar = 0;
  unsigned wq_cnt = 0;            // wave-uniform: columns in this wave's queue
  const __bf16* Xb = reinterpret_cast<const __bf16*>(a.Xb);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r31 = lane & 31, hh = lane >> 5;
  // XCD-aware block map (workgroups are dealt round-robin over the 8 XCDs, each with its own L2): all query blocks
  // that stream the SAME corpus split are placed on one XCD and next to each other in dispatch order, so a corpus
  // tile is fetched from HBM once per XCD instead of once per query block.  Pure speed: any placement is correct.
  const unsigned lin = blockIdx.x;
  const unsigned xcd = lin & 7u, kk = lin >> 3;
  const unsigned bx = kk % (unsigned)a.qgrid, by = (kk / (unsigned)a.qgrid) * 8u + xcd;
  if ((int)by >= a.nsplit) return;
  const int64_t qb0 = (int64_t)bx * QBB;
  const int ql0 = w * 64 + r31, ql1 = ql0 + 32;  // block-local query index of this lane's two query groups
  const bool ok0 = qb0 + ql0 < a.nq, ok1 = qb0 + ql1 < a.nq;
  const int64_t qr0 = ok0 ? qb0 + ql0 : a.nq - 1, qr1 = ok1 ? qb0 + ql1 : a.nq - 1;
  const float th0 = (a.thr && ok0) ? a.thr[qr0] : -INFINITY, th1 = (a.thr && ok1) ? a.thr[qr1] : -INFINITY;
  bf16x8_t qf0[KB], qf1[KB];
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const f32x4 u0 = *reinterpret_cast<const f32x4*>(&a.Q[qr0 * D + kb * 16 + 8 * hh]);
    const f32x4 u1 = *reinterpret_cast<const f32x4*>(&a.Q[qr0 * D + kb * 16 + 8 * hh + 4]);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(&a.Q[qr1 * D + kb * 16 + 8 * hh]);
    const f32x4 v1 = *reinterpret_cast<const f32x4*>(&a.Q[qr1 * D + kb * 16 + 8 * hh + 4]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      qf0[kb][j] = (__bf16)u0[j]; qf0[kb][4 + j] = (__bf16)u1[j];
      qf1[kb][j] = (__bf16)v0[j]; qf1[kb][4 + j] = (__bf16)v1[j];
    }
  }
  const int64_t n_seq = (a.n_virtual + TRB - 1) / TRB;
  const int64_t per = (n_seq + a.nsplit - 1) / a.nsplit;
  const int64_t i0 = (int64_t)by * per;
  const int64_t i1 = (i0 + per < n_seq) ? i0 + per : n_seq;
  if (i0 >= i1) {   // a split without rows (nsplit does not divide the stages): its segments are empty, and SAY so
    if (MODE == 0 && hh == 0) {
      if (ok0) a.seg_cnt[(size_t)qr0 * a.nsplit + by] = 0;
      if (ok1) a.seg_cnt[(size_t)qr1 * a.nsplit + by] = 0;
    }
    if (MODE == 2) {   // empty streams hold key 0 (below every score): no memset of the stream table needed
      const int64_t slot = ((int64_t)by * 2 + hh) * SAMPLE_T;
#pragma unroll
      for (int i = 0; i < SAMPLE_T; ++i) {
        if (ok0) a.cand[(size_t)qr0 * a.cap + slot + i] = 0ull;
        if (ok1) a.cand[(size_t)qr1 * a.cap + slot + i] = 0ull;
      }
    }
    return;
  }
  if (!DENSE) {   // visible to the flush after the first stage barrier
    if (hh == 0) { qcntS[ql0] = 0; qcntS[ql1] = 0; }
  }

  // staging: every thread owns the same (row-in-16, 16-byte column) slot of each 16-row slab of a stage, so a full
  // tile of the contiguous corpus is NV loads off ONE per-thread pointer with compile-time offsets
  bf16x8_t stA[NV], stB[NV];
  const int sr0 = tid / (D / 8), sc8 = tid % (D / 8);
  constexpr int SROWS = 256 / (D / 8);   // rows covered by one load instruction of the workgroup
  const __bf16* my_src = Xb + (size_t)sr0 * D + sc8 * 8;
  auto load_tile = [&](bf16x8_t* stage, int64_t tile) {
    const int64_t v_base = tile * TRB;
    if (a.row_stride == 1 && v_base + TRB <= a.n_virtual) {   // workgroup-uniform fast path
      const __bf16* src = my_src + (size_t)v_base * D;
#pragma unroll
      for (int i = 0; i < NV; ++i) stage[i] = *reinterpret_cast<const bf16x8_t*>(src + (size_t)i * SROWS * D);
      return;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int64_t v = v_base + sr0 + i * SROWS;
      bf16x8_t val;
#pragma unroll
      for (int j = 0; j < 8; ++j) val[j] = (__bf16)0.f;
      if (sr0 + i * SROWS < TRB && v < a.n_virtual)
        val = *reinterpret_cast<const bf16x8_t*>(Xb + (size_t)(v * a.row_stride) * D + sc8 * 8);
      stage[i] = val;
    }
  };
  auto store_tile = [&](const bf16x8_t* stage, int buf) {
#pragma unroll
    for (int i = 0; i < NV; ++i)
      if (sr0 + i * SROWS < TRB) *reinterpret_cast<bf16x8_t*>(&Xs[buf][(sr0 + i * SROWS) * LDB + sc8 * 8]) = stage[i];
  };
  float top0[SAMPLE_T], top1[SAMPLE_T];
#pragma unroll
  for (int i = 0; i < SAMPLE_T; ++i) { top0[i] = -INFINITY; top1[i] = -INFINITY; }
  auto emit = [&](const f32x16& acc, int64_t v_base, int ql, bool ok, float th, int64_t qrow) {
    if (MODE != 0 && !ok) return;   // MODE 0: every lane takes part in the ballot below (wq_cnt must stay wave-uniform)
    if (MODE == 2) {
      float* top = (ql == ql0) ? top0 : top1;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float sc = (v_base + acc_row(r, lane) < a.n_virtual) ? acc[r] : -INFINITY;
        // insert into the descending list: t_i' = med3(t_{i-1}, s, t_i) (in place, from the tail)
#pragma unroll
        for (int i = SAMPLE_T - 1; i > 0; --i) top[i] = __builtin_amdgcn_fmed3f(top[i - 1], sc, top[i]);
        top[0] = fmaxf(top[0], sc);
      }
      return;
    }
    if (DENSE) {
      uint64_t* cnd = a.cand + (size_t)qrow * a.cap;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t v = v_base + acc_row(r, lane);
        if (v < a.n_virtual) cnd[v] = make_key(acc[r], (uint32_t)v);
      }
      return;
    }
    // The v_max3 ops are inline asm, which the compiler's MFMA->VALU hazard recognizer does not see: they must not be the
    // first readers of the accumulator (they read stale registers when they directly followed the MFMAs and lost
    // survivors).  Every group maximum starts with a compiler-visible fmaxf (hipcc pads it with the required wait
    // states), so every asm read is ordered behind one.
    float g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = max3_raw(fmaxf(acc[4 * k], acc[4 * k + 1]), acc[4 * k + 2], acc[4 * k + 3]);
    const float mx = max3_raw(fmaxf(g[0], g[1]), g[2], g[3]);
    const float te = ok ? th : INFINITY;
#if RIHIP_SCAN_ABLATE == 1   // experiments: the filter without survivor handling (scores computed, maxima taken, nothing kept)
    asm volatile("" :: "v"(mx));
    return;
#endif
    if (__ballot(mx >= te) == 0ull) return;   // wave-uniform: no survivor in the wave's 64 columns (1 in 6 at k = 500)
    // Survivors are found group of four by group of four, all branches wave-uniform: a wave's 1 024 scores hold ~1.7
    // survivors, so ~1.4 of the 4 groups and ~1.1 scores of such a group take the queue path.
    const unsigned vl = (unsigned)v_base + 4u * (unsigned)hh;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (__ballot(g[k] >= te) == 0ull) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float sc = acc[4 * k + j];
        const bool h = sc >= te;
        const unsigned long long m = __ballot(h);
        if (m == 0ull) continue;
        const unsigned pos = wq_cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        wq_cnt += (unsigned)__popcll(m);
        if (h) {
          if (pos < (unsigned)WQE) qent[w][pos] = uint4{__float_as_uint(sc), vl + (unsigned)(j + 8 * k), (unsigned)ql, 0u};
          else atomicOr(&qcntS[ql], 1 << 30);   // queue full (a stage brought > 64 survivors to one wave): the segment is
                                                // marked overflowed and the query takes the exact re-do path
        }
      }
    }
  };
  // The wave empties its OWN queue (no barrier, no other wave involved): one entry per lane, slot in the query's segment
  // from a returning LDS atomic, all loads / atomics / stores of a pass in flight together.
  auto wave_flush = [&]() {
    const unsigned n = wq_cnt < (unsigned)WQE ? wq_cnt : (unsigned)WQE;   // entries beyond WQE went the slow path
    uint4 en[WQE / 64]; int pos[WQE / 64];
#pragma unroll
    for (int j = 0; j < WQE / 64; ++j) en[j] = qent[w][j * 64 + lane];
#pragma unroll
    for (int j = 0; j < WQE / 64; ++j) {
      const bool in = (unsigned)(j * 64 + lane) < n && (int64_t)en[j].y < a.n_virtual;
      pos[j] = in ? atomicAdd(&qcntS[en[j].z], 1) : a.seg_cap;   // LDS
    }
#pragma unroll
    for (int j = 0; j < WQE / 64; ++j)
      if (pos[j] < a.seg_cap)
        a.seg[((size_t)(qb0 + en[j].z) * a.nsplit + by) * a.seg_cap + pos[j]] = make_key(__uint_as_float(en[j].x), en[j].y);
    wq_cnt = 0;
  };
  // after every stage: the barrier hands the LDS tile buffer over.  ALL waves empty their queues at the same stage, as
  // soon as one of them is half full: a wave that flushes alone makes its three siblings wait at the next barrier, and
  // with four independent triggers the workgroup stalled four times as often (0.64 of 1.8 ms).
  auto stage_end = [&](bool last) {
    if (!DENSE && lane == 0) wcnt[wpar][w] = wq_cnt;
    __syncthreads();
    if (!DENSE) {
      // the slot read here is rewritten two barriers later at the earliest: every wave sees the same four values
      const unsigned m01 = wcnt[wpar][0] > wcnt[wpar][1] ? wcnt[wpar][0] : wcnt[wpar][1];
      const unsigned m23 = wcnt[wpar][2] > wcnt[wpar][3] ? wcnt[wpar][2] : wcnt[wpar][3];
      wpar ^= 1;
      if (last || (m01 > m23 ? m01 : m23) >= (unsigned)(WQE - 64)) wave_flush();   // workgroup-uniform decision (a stage adds ~10-20 entries per wave)
    }
  };
  auto compute = [&](int buf, int64_t i) {
#pragma unroll 1
    for (int sub = 0; sub < TRB / 32; ++sub) {
      const __bf16* Xt = &Xs[buf][sub * 32 * LDB];
      f32x16 a0 = zero16(), a1 = zero16();
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        const bf16x8_t av = *reinterpret_cast<const bf16x8_t*>(&Xt[r31 * LDB + kb * 16 + 8 * hh]);
        a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, qf0[kb], a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, qf1[kb], a1, 0, 0, 0);
      }
      const int64_t v_base = i * TRB + sub * 32;
      emit(a0, v_base, ql0, ok0, th0, qr0);
      emit(a1, v_base, ql1, ok1, th1, qr1);
    }
  };

  // two stages in flight through registers (global latency under load is 2-4 stages of MFMA work), two LDS buffers
  load_tile(stA, i0);
  store_tile(stA, 0);
  if (i0 + 1 < i1) load_tile(stA, i0 + 1);
  __syncthreads();
#pragma unroll 1
  for (int64_t i = i0; i < i1; i += 2) {
    // even phase: buffer 0 = stage i, stA = stage i+1 (in flight)
    if (i + 2 < i1) load_tile(stB, i + 2);
    compute(0, i);
    if (i + 1 < i1) store_tile(stA, 1);
    stage_end(i + 1 >= i1);
    if (i + 1 >= i1) break;
    // odd phase: buffer 1 = stage i+1, stB = stage i+2 (in flight)
    if (i + 3 < i1) load_tile(stA, i + 3);
    compute(1, i + 1);
    if (i + 2 < i1) store_tile(stB, 0);
    stage_end(i + 2 >= i1);
  }
  if (MODE == 0 && hh == 0) {   // the wave's own LDS atomics are complete (in order): publish the segment fills
    if (ok0) a.seg_cnt[(size_t)qr0 * a.nsplit + by] = qcntS[ql0];
    if (ok1) a.seg_cnt[(size_t)qr1 * a.nsplit + by] = qcntS[ql1];
  }
  if (MODE == 2) {   // stream = (corpus split, row half): SAMPLE_T key slots each, [nq, 2 * nsplit * SAMPLE_T]
    const int64_t slot = ((int64_t)by * 2 + hh) * SAMPLE_T;
#pragma unroll
    for (int i = 0; i < SAMPLE_T; ++i) {
      if (ok0) a.cand[(size_t)qr0 * a.cap + slot + i] = make_key(top0[i], 0u);
      if (ok1) a.cand[(size_t)qr1 * a.cap + slot + i] = make_key(top1[i], 0u);
    }
  }
}

}  // namespace

namespace rihip_index {

int launch_scan_bf16(int d, int mode, const ScanArgs& a, hipStream_t st) {
  const dim3 grid((unsigned)a.qgrid * 8u * (unsigned)((a.nsplit + 7) / 8));   // (XCD-aware 1-D block map)
  RCCHK(dispatch_d(d, [&](auto D) {
    if (mode == 2) hipLaunchKernelGGL((scan_bf16_kernel<decltype(D)::value, 2>), grid, dim3(256), 0, st, a);
    else if (mode == 1) hipLaunchKernelGGL((scan_bf16_kernel<decltype(D)::value, 1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((scan_bf16_kernel<decltype(D)::value, 0>), grid, dim3(256), 0, st, a);
  }));
  return check_launch("scan_bf16");
}

// flat index with N > 4*SAMPLE: the bf16 filter copy of the two-precision search + the row-norm bound it needs
int prepare_flat(IpIndex* h, hipStream_t st) {
  if (h->ivf || h->N <= 4 * (int64_t)SAMPLE) return RIHIP_OK;
  const int64_t n = h->N * h->d;
  hipFree(h->Xb);
  h->Xb = nullptr;
  // (exactly N rows: scan_bf16_kernel takes whole-stage loads only where v_base + TRB <= n_virtual and guards every row
  // of a partial last stage, so no load passes row N)
  HIPCHK(hipMalloc((void**)&h->Xb, sizeof(__bf16) * (size_t)n));
  hipLaunchKernelGGL(to_bf16_kernel, dim3((unsigned)((n / 4 + 255) / 256 + 1)), dim3(256), 0, st, h->X, n, h->Xb);
  int* bits = nullptr;
  HIPCHK(hipMalloc((void**)&bits, sizeof(int)));
  HIPCHK(hipMemsetAsync(bits, 0, sizeof(int), st));
  hipLaunchKernelGGL(rownorm_max_kernel, dim3(1024), dim3(256), 0, st, h->X, h->N, h->d, bits);
  int hb = 0;
  HIPCHK(hipMemcpyAsync(&hb, bits, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  hipFree(bits);
  float sq;
  memcpy(&sq, &hb, sizeof(float));
  h->max_norm = sqrtf(sq);
  return RIHIP_OK;
}

}  // namespace rihip_index
