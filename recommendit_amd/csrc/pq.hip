// Product-quantised inner-product index: the training, encoding and decoding kernels, the build and the C ABI.
//
// A PQ index is an Sq8Index handle whose code storage is one byte per sub-space and row (pq_codes) plus int8 codebooks
// (pq_book) in place of the int8 matrix: the row's SQ8 code is, per sub-space, the codebook entry its byte names.  The
// search is sq8.hip's, whose scan (sq8_scan.hip, sq8_scan_lm_kernel<DP, FM, PQ>) gathers the operand bytes from the codebooks in LDS;
// nothing else of the search knows the difference, so a PQ index is the SQ8 index of its own reconstruction.
//
// The quantiser works on the rows' SQ8 codes c (int8, padding columns 0), in integers only (recommendit_hip.h at
// rihip_pq_index_*): sub-space m covers columns m dsub .. + dsub - 1; D(i, m, e) = sum_j (c[i][m dsub + j] - book[m][e][j])^2
// in i32; a row's byte is the e of the smallest D, the lowest e on a tie; a Lloyd step replaces an entry by
// clamp(rint((double)sum / (double)cnt), +-127) of the rows assigned to it (exact integer sums) and leaves an entry without
// rows as it is.  The sums are integer atomics, privatised in LDS per workgroup and then added to i64 words in global
// memory: exact in any order, so the result does not depend on the physical row order.
//
// D is evaluated as |c|^2 + |b|^2 - 2 <c, b> with the packed int8 dot product (v_dot4_i32_i8): the same integer.
//
// Residual encoding (opt-in, IVF sources; recommendit_hip.h at rihip_pq_index_from_ip_index_residual): the list's centroid
// is snapped to the SQ8 grid (pq_list_codes, int8 [nlist, dpad]) and the quantiser above runs, unchanged, on
// clamp(c - K_l, +-127) written over the transient SQ8 codes.  The decoded code K_l + entry is an int16 in [-254, 254]
// (pq_decode_all16); the search adds T[q, l] = sum_j n_j K_l[j] to the gathered dot product (sq8.hip, sq8_scan.hip).
#pragma clang fp contract(off)
#include "common.h"
#include "recommendit_hip.h"

#include <algorithm>
#include <chrono>
#include <limits.h>
#include <math.h>
#include <string.h>
#include <vector>

#include "search_kernels.h"
#include "sq8_index.h"

using namespace rihip_index;

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr int PQ_RPT = 8;                 // rows per thread of the assignment kernel
constexpr int PQ_RPB = 256 * PQ_RPT;      // rows per workgroup: an LDS sum stays below 2048 * 127 < 2^18

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int acc) {   // four signed bytes each, exact in i32
  return __builtin_amdgcn_sdot4((int)a, (int)b, acc, false);
}

// book[m][e][:] = the SQ8 sub-vectors of ORIGINAL row (e N) / 256 (int64).  One thread per physical row: the entries that
// name its row are e = ceil(256 row / N) .. while (e N) / 256 == row (none for most rows; several where N < 256)
__global__ void pq_init_book_kernel(const int8_t* __restrict__ codes, const int64_t* __restrict__ row_ids, int64_t N, int64_t Np,
                                    int dpad, int dsub, int8_t* book) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= Np) return;
  const int64_t row = row_ids[p];
  if (row < 0) return;
  for (int64_t e = (row * 256 + N - 1) / N; e < 256 && (e * N) / 256 == row; ++e)
    for (int j = 0; j < dpad; ++j) book[((size_t)(j / dsub) * 256 + e) * dsub + (j % dsub)] = codes[(size_t)p * dpad + j];
}

// One assignment pass of sub-space blockIdx.y over the physical rows [blockIdx.x * PQ_RPB, + PQ_RPB).  The sub-space's 256
// entries lie in LDS as packed words next to their squared norms and are read as a broadcast (every lane the same
// address); a thread holds its row's DSUB bytes in registers.  ACC: the row is added to the sums of its entry, first in
// LDS (i32), then once per workgroup and non-zero word in global memory (i64).  Padding rows (row_ids < 0) get byte 0 and
// take no part.  *distortion += the pass's sum of the smallest D.
template <int DSUB, bool ACC>
__global__ __launch_bounds__(256) void pq_assign_kernel(const int8_t* __restrict__ codes, const int64_t* __restrict__ row_ids,
                                                        int64_t Np, int dpad, const int8_t* __restrict__ book, uint8_t* pq_codes,
                                                        u64* gsum, u64* gcnt, u64* distortion) {
  constexpr int W = DSUB / 4;
  __shared__ uint32_t s_b[256 * W];
  __shared__ int s_n[256];
  __shared__ int s_sum[ACC ? 256 * DSUB : 1];
  __shared__ int s_cnt[ACC ? 256 : 1];
  const int tid = threadIdx.x, m = blockIdx.y, M = dpad / DSUB;
  {
    const uint32_t* gb = reinterpret_cast<const uint32_t*>(book + ((size_t)m * 256 + tid) * DSUB);
    int nn = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const uint32_t v = gb[w];
      s_b[tid * W + w] = v;
      nn = dot4(v, v, nn);
    }
    s_n[tid] = nn;
    if constexpr (ACC) {
#pragma unroll
      for (int j = 0; j < DSUB; ++j) s_sum[tid * DSUB + j] = 0;
      s_cnt[tid] = 0;
    }
  }
  __syncthreads();
  long long dist = 0;
  const int64_t base = (int64_t)blockIdx.x * PQ_RPB;
  for (int it = 0; it < PQ_RPT; ++it) {
    const int64_t p = base + it * 256 + tid;
    if (p >= Np) continue;
    int best = 0;
    if (row_ids[p] >= 0) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(codes + (size_t)p * dpad + m * DSUB);
      uint32_t c[W];
      int cn = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) { c[w] = src[w]; cn = dot4(c[w], c[w], cn); }
      int bd = INT_MAX;
#pragma unroll 4
      for (int e = 0; e < 256; ++e) {
        int dp = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) dp = dot4(c[w], s_b[e * W + w], dp);
        const int d = s_n[e] - 2 * dp;
        if (d < bd) { bd = d; best = e; }   // strictly smaller: the lowest e keeps a tie
      }
      dist += cn + bd;
      if constexpr (ACC) {
#pragma unroll
        for (int j = 0; j < DSUB; ++j) {
          const int v = (int)(int8_t)(c[j >> 2] >> (8 * (j & 3)));
          if (v != 0) atomicAdd(&s_sum[best * DSUB + j], v);
        }
        atomicAdd(&s_cnt[best], 1);
      }
    }
    pq_codes[(size_t)p * M + m] = (uint8_t)best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) dist += __shfl_xor(dist, o, 64);
  if ((tid & 63) == 0 && dist != 0) atomicAdd(distortion, (u64)dist);
  if constexpr (ACC) {
    __syncthreads();
    for (int i = tid; i < 256 * DSUB; i += 256) {
      const int v = s_sum[i];
      if (v != 0) atomicAdd(&gsum[(size_t)m * 256 * DSUB + i], (u64)(long long)v);   // two's complement: a signed i64 sum
    }
    if (s_cnt[tid] != 0) atomicAdd(&gcnt[m * 256 + tid], (u64)s_cnt[tid]);
  }
}

// the Lloyd step's division, one thread per codebook byte; an entry without rows keeps its value
__global__ void pq_update_book_kernel(const u64* __restrict__ gsum, const u64* __restrict__ gcnt, int n, int dsub, int8_t* book) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 cnt = gcnt[i / dsub];
  if (cnt == 0) return;
  double v = rint((double)(long long)gsum[i] / (double)cnt);   // one correctly rounded division, half to even
  v = fmin(fmax(v, -127.0), 127.0);
  book[i] = (int8_t)(int)v;
}

// pq_decode_rows: entry numbers + codebooks -> int8 [rows, dpad], one thread per (row, sub-space); padding rows are zeros
template <int DSUB>
__global__ void pq_decode_rows_kernel(const uint8_t* __restrict__ pq_codes, const int8_t* __restrict__ book,
                                      const int64_t* __restrict__ row_ids, int64_t rows, int dpad, int8_t* out) {
  typedef typename std::conditional<DSUB == 8, uint2, i32x4>::type V;
  const int M = dpad / DSUB;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * M) return;
  const int64_t p = i / M;
  const int m = (int)(i % M);
  V v{};
  if (row_ids[p] >= 0) v = *reinterpret_cast<const V*>(book + ((size_t)m * 256 + pq_codes[i]) * DSUB);
  *reinterpret_cast<V*>(out + (size_t)p * dpad + m * DSUB) = v;
}

// ---- residual encoding (by_residual): the quantiser above runs on r = clamp(c - K_l, +-127), K_l the centroid of the
// row's list on the SQ8 grid; the decoded code K_l + entry is an int16 in [-254, 254]

// the list that holds physical row p: the largest l with list_poff[l] <= p (an empty list shares its offset with the
// next one, which then wins; p < Np = list_poff[nlist])
__device__ __forceinline__ int pq_list_of(const int64_t* __restrict__ list_poff, int nlist, int64_t p) {
  int lo = 0, hi = nlist;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (list_poff[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

// K[l][j] = sq8_code(C[l][j], m_j, s_j) for j < du, 0 in the padding columns; one thread per byte
__global__ void pq_list_codes_kernel(const float* __restrict__ C, int nlist, int du, int dk, int dpad, const float* __restrict__ centre,
                                     const float* __restrict__ scale, int8_t* K) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nlist * dpad) return;
  const int l = i / dpad, j = i % dpad;
  K[i] = j < du ? (int8_t)sq8_code(C[(size_t)l * dk + j], centre[j], scale[j]) : (int8_t)0;
}

// codes[p][:] = clamp(codes[p][:] - K[list of p][:], +-127) in place, four bytes per thread; padding rows stay 0.
// *clamped += the values that left [-127, 127]
__global__ __launch_bounds__(256) void pq_residual_kernel(int8_t* codes, const int64_t* __restrict__ row_ids,
                                                          const int64_t* __restrict__ list_poff, int nlist, int64_t Np, int dpad,
                                                          const int8_t* __restrict__ K, u64* clamped) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_row = dpad / 4;
  int n_cl = 0;
  if (i < Np * per_row) {
    const int64_t p = i / per_row;
    const int j = (int)(i % per_row) * 4;
    if (row_ids[p] >= 0) {
      const int l = pq_list_of(list_poff, nlist, p);
      uint32_t* at = reinterpret_cast<uint32_t*>(codes + (size_t)p * dpad + j);
      const uint32_t cw = *at, kw = *reinterpret_cast<const uint32_t*>(K + (size_t)l * dpad + j);
      uint32_t packed = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int r = (int)(int8_t)(cw >> (8 * u)) - (int)(int8_t)(kw >> (8 * u));
        if (r > 127) { r = 127; ++n_cl; }
        if (r < -127) { r = -127; ++n_cl; }
        packed |= ((uint32_t)r & 0xFFu) << (8 * u);
      }
      *at = packed;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n_cl += __shfl_xor(n_cl, o, 64);
  if ((threadIdx.x & 63) == 0 && n_cl != 0) atomicAdd(clamped, (u64)n_cl);
}

// the decoded codes of a residual handle: int16 [rows, dpad] = K[list of p] + entry, one thread per (row, sub-space);
// padding rows are zeros
template <int DSUB>
__global__ void pq_decode_rows16_kernel(const uint8_t* __restrict__ pq_codes, const int8_t* __restrict__ book,
                                        const int8_t* __restrict__ K, const int64_t* __restrict__ row_ids,
                                        const int64_t* __restrict__ list_poff, int nlist, int64_t rows, int dpad, int16_t* out) {
  const int M = dpad / DSUB;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * M) return;
  const int64_t p = i / M;
  const int m = (int)(i % M);
  int16_t* o = out + (size_t)p * dpad + m * DSUB;
  if (row_ids[p] < 0) {
#pragma unroll
    for (int j = 0; j < DSUB; ++j) o[j] = 0;
    return;
  }
  const int8_t* b = book + ((size_t)m * 256 + pq_codes[i]) * DSUB;
  const int8_t* k = K + (size_t)pq_list_of(list_poff, nlist, p) * dpad + m * DSUB;
#pragma unroll
  for (int j = 0; j < DSUB; ++j) o[j] = (int16_t)((int)k[j] + (int)b[j]);
}

// the entry numbers in original row order
__global__ void pq_codes_by_row_kernel(const uint8_t* __restrict__ pq_codes, const int64_t* __restrict__ row_ids, int64_t Np, int M,
                                       uint8_t* out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Np * M) return;
  const int64_t row = row_ids[i / M];
  if (row >= 0) out[(size_t)row * M + (i % M)] = pq_codes[i];
}

template <bool ACC>
void launch_assign_pass(const Sq8Index* h, const int8_t* codes, int dsub, u64* gsum, u64* gcnt, u64* dist, hipStream_t st) {
  const dim3 grid((unsigned)((h->Np + PQ_RPB - 1) / PQ_RPB), (unsigned)(h->dpad / dsub));
  if (dsub == 8)
    hipLaunchKernelGGL((pq_assign_kernel<8, ACC>), grid, dim3(256), 0, st, codes, h->row_ids, h->Np, h->dpad, h->pq_book, h->pq_codes, gsum, gcnt, dist);
  else
    hipLaunchKernelGGL((pq_assign_kernel<16, ACC>), grid, dim3(256), 0, st, codes, h->row_ids, h->Np, h->dpad, h->pq_book, h->pq_codes, gsum, gcnt, dist);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct PqTimes { double sq8 = 0, train = 0, encode = 0; };

// h: a fresh handle.  The SQ8 build first (layout, row ids, quantiser and, transiently, the int8 codes), then the
// codebooks (injected, or trained in n_iter Lloyd steps) and the final assignment; the int8 codes are freed before the
// call returns.
// residual: the list codes first, then the SQ8 codes become residuals in place and everything after runs on those.
int pq_build(Sq8Index* h, const IpIndex* src, const float* centre, const float* scale, int dsub, int n_iter, const int8_t* book_host,
             bool residual, PqTimes* tm, hipStream_t st) {
  auto t0 = std::chrono::steady_clock::now();
  RCCHK(sq8_build(h, src, centre, scale, st));   // (synchronises)
  tm->sq8 = ms_since(t0);
  const int M = h->dpad / dsub;
  const size_t book_bytes = (size_t)h->dpad * 256;
  int8_t* sq8_codes = h->codes;
  u64* gsum = nullptr; u64* gcnt = nullptr; u64* dist = nullptr;
  const int64_t sq8_bytes = sq8_held_bytes(h);
  auto work = [&]() -> int {
    HIPCHK(hipMalloc((void**)&h->pq_codes, (size_t)h->Np * M));
    HIPCHK(hipMalloc((void**)&h->pq_book, book_bytes));
    HIPCHK(hipMalloc((void**)&dist, sizeof(u64) * (size_t)(n_iter + 2)));   // (the last word: the residual clamp count)
    HIPCHK(hipMemsetAsync(dist, 0, sizeof(u64) * (size_t)(n_iter + 2), st));
    h->pq_dsub = dsub;
    h->pq_peak_bytes = sq8_bytes + h->Np * M + (int64_t)book_bytes + 8 * (int64_t)(n_iter + 1);
    if (residual) {
      const int nk = h->nlist * h->dpad;
      HIPCHK(hipMalloc((void**)&h->pq_list_codes, (size_t)nk));
      h->pq_residual = true;
      h->pq_peak_bytes += nk;
      hipLaunchKernelGGL(pq_list_codes_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, st, h->C, h->nlist, h->du, h->dk, h->dpad,
                         h->centre, h->scale, h->pq_list_codes);
      const int64_t nthr = h->Np * (h->dpad / 4);
      hipLaunchKernelGGL(pq_residual_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, sq8_codes, h->row_ids, h->list_poff,
                         h->nlist, h->Np, h->dpad, h->pq_list_codes, dist + (n_iter + 1));
      RCCHK(check_launch("pq residual"));
    }
    auto t1 = std::chrono::steady_clock::now();
    int passes = 1;
    if (book_host) {
      HIPCHK(hipMemcpyAsync(h->pq_book, book_host, book_bytes, hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));
    } else {
      passes = n_iter + 1;
      HIPCHK(hipMalloc((void**)&gsum, sizeof(u64) * book_bytes));
      HIPCHK(hipMalloc((void**)&gcnt, sizeof(u64) * (size_t)M * 256));
      h->pq_peak_bytes += 8 * (int64_t)book_bytes + 8 * (int64_t)M * 256;
      hipLaunchKernelGGL(pq_init_book_kernel, dim3((unsigned)((h->Np + 255) / 256)), dim3(256), 0, st, sq8_codes, h->row_ids, h->N, h->Np,
                         h->dpad, dsub, h->pq_book);
      for (int it = 0; it < n_iter; ++it) {
        HIPCHK(hipMemsetAsync(gsum, 0, sizeof(u64) * book_bytes, st));
        HIPCHK(hipMemsetAsync(gcnt, 0, sizeof(u64) * (size_t)M * 256, st));
        launch_assign_pass<true>(h, sq8_codes, dsub, gsum, gcnt, dist + it, st);
        hipLaunchKernelGGL(pq_update_book_kernel, dim3((unsigned)((book_bytes + 255) / 256)), dim3(256), 0, st, gsum, gcnt, (int)book_bytes,
                           dsub, h->pq_book);
      }
      RCCHK(check_launch("pq train"));
      HIPCHK(hipStreamSynchronize(st));
    }
    tm->train = ms_since(t1);
    auto t2 = std::chrono::steady_clock::now();
    launch_assign_pass<false>(h, sq8_codes, dsub, nullptr, nullptr, dist + (passes - 1), st);
    RCCHK(check_launch("pq encode"));
    std::vector<u64> tr(passes);
    u64 n_clamped = 0;
    HIPCHK(hipMemcpyAsync(tr.data(), dist, sizeof(u64) * passes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&n_clamped, dist + (n_iter + 1), sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    h->pq_clamped = (int64_t)n_clamped;
    tm->encode = ms_since(t2);
    h->pq_trace.assign(tr.begin(), tr.end());
    return RIHIP_OK;
  };
  const int rc = work();
  hipFree(gsum); hipFree(gcnt); hipFree(dist);
  if (rc) return rc;   // (the caller frees the handle and with it whatever was allocated)
  hipFree(h->codes);
  h->codes = nullptr;
  return RIHIP_OK;
}

}  // namespace

namespace rihip_index {
int pq_decode_all(const Sq8Index* h, int8_t** out_dev, hipStream_t st) {
  RIHIP_REQUIRE(h && h->pq_codes && h->pq_book && out_dev, RIHIP_ERR_STATE, "pq_decode_rows: not a PQ index");
  RIHIP_REQUIRE(!h->pq_residual, RIHIP_ERR_STATE, "pq_decode_rows: the decoded codes of a residual PQ index are 16-bit");
  int8_t* out = nullptr;
  HIPCHK(hipMalloc((void**)&out, (size_t)h->Np * h->dpad));
  const int64_t tot = h->Np * (h->dpad / h->pq_dsub);
  const dim3 grid((unsigned)((tot + 255) / 256));
  if (h->pq_dsub == 8) hipLaunchKernelGGL(pq_decode_rows_kernel<8>, grid, dim3(256), 0, st, h->pq_codes, h->pq_book, h->row_ids, h->Np, h->dpad, out);
  else hipLaunchKernelGGL(pq_decode_rows_kernel<16>, grid, dim3(256), 0, st, h->pq_codes, h->pq_book, h->row_ids, h->Np, h->dpad, out);
  const int rc = check_launch("pq decode rows");
  if (rc) { hipFree(out); return rc; }
  *out_dev = out;
  return RIHIP_OK;
}

int pq_decode_all16(const Sq8Index* h, int16_t** out_dev, hipStream_t st) {
  RIHIP_REQUIRE(h && h->pq_codes && h->pq_book && h->pq_list_codes && out_dev, RIHIP_ERR_STATE, "pq_decode_rows16: not a residual PQ index");
  int16_t* out = nullptr;
  HIPCHK(hipMalloc((void**)&out, sizeof(int16_t) * (size_t)h->Np * h->dpad));
  const int64_t tot = h->Np * (h->dpad / h->pq_dsub);
  const dim3 grid((unsigned)((tot + 255) / 256));
  if (h->pq_dsub == 8)
    hipLaunchKernelGGL(pq_decode_rows16_kernel<8>, grid, dim3(256), 0, st, h->pq_codes, h->pq_book, h->pq_list_codes, h->row_ids,
                       h->list_poff, h->nlist, h->Np, h->dpad, out);
  else
    hipLaunchKernelGGL(pq_decode_rows16_kernel<16>, grid, dim3(256), 0, st, h->pq_codes, h->pq_book, h->pq_list_codes, h->row_ids,
                       h->list_poff, h->nlist, h->Np, h->dpad, out);
  const int rc = check_launch("pq decode rows (residual)");
  if (rc) { hipFree(out); return rc; }
  *out_dev = out;
  return RIHIP_OK;
}
}  // namespace rihip_index

// ------------------------------------------------ C ABI --------------------------------------------------------------
extern "C" int rihip_pq_index_from_ip_index_residual(void* ip_handle, const float* centre, const float* scale, int dsub, int n_iter,
                                                     const int8_t* book, int by_residual, void** handle, void* stream) {
  const IpIndex* src = (const IpIndex*)ip_handle;
  RIHIP_REQUIRE(src && handle, RIHIP_ERR_ARG, "pq_index_from_ip_index: null handle");
  RIHIP_REQUIRE(src->X && src->N > 0, RIHIP_ERR_STATE, "pq_index_from_ip_index: the source index is empty");
  RIHIP_REQUIRE((centre == nullptr) == (scale == nullptr), RIHIP_ERR_ARG, "pq_index_from_ip_index: give both centre and scale, or neither");
  RIHIP_REQUIRE(dsub == 8 || dsub == 16, RIHIP_ERR_ARG, "pq_index_from_ip_index: dsub=%d (8 or 16)", dsub);
  RIHIP_REQUIRE(n_iter >= 0 && n_iter <= 1000, RIHIP_ERR_ARG, "pq_index_from_ip_index: n_iter=%d outside [0, 1000]", n_iter);
  if (book) {
    const size_t nb = (size_t)(src->d <= 64 ? 64 : 128) * 256;
    for (size_t i = 0; i < nb; ++i)
      RIHIP_REQUIRE(book[i] != -128, RIHIP_ERR_ARG, "pq_index_from_ip_index: codebook byte %lld is -128 (entries lie in [-127, 127])", (long long)i);
  }
  RIHIP_REQUIRE(!by_residual || src->ivf, RIHIP_ERR_ARG,
                "pq_index_from_ip_index: by_residual needs an IVF source (a flat index has one list and no centroids)");
  Sq8Index* h = new Sq8Index();
  PqTimes tm;
  const int rc = pq_build(h, src, centre, scale, dsub, n_iter, book, by_residual != 0, &tm, (hipStream_t)stream);
  if (rc) { sq8_free(h); return rc; }
  h->pq_ms[0] = tm.sq8; h->pq_ms[1] = tm.train; h->pq_ms[2] = tm.encode;
  *handle = h;
  return RIHIP_OK;
}

extern "C" int rihip_pq_index_from_ip_index(void* ip_handle, const float* centre, const float* scale, int dsub, int n_iter,
                                            const int8_t* book, void** handle, void* stream) {
  return rihip_pq_index_from_ip_index_residual(ip_handle, centre, scale, dsub, n_iter, book, 0, handle, stream);
}

extern "C" int rihip_pq_index_is_residual(void* handle) { return handle && ((Sq8Index*)handle)->pq_residual ? 1 : 0; }

extern "C" int rihip_pq_index_get_list_codes(void* handle, int8_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && h->pq_list_codes && out, RIHIP_ERR_STATE, "pq_index_get_list_codes: not a residual PQ index");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, h->pq_list_codes, (size_t)h->nlist * h->dpad, hipMemcpyDeviceToHost));
  return RIHIP_OK;
}

extern "C" int rihip_pq_index_get_decoded16(void* handle, int16_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && h->pq_residual && out, RIHIP_ERR_STATE, "pq_index_get_decoded16: not a residual PQ index");
  return sq8_rows_out(h, nullptr, out);
}

extern "C" int rihip_pq_index_residual_clamped(void* handle, int64_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && h->pq_codes && out, RIHIP_ERR_STATE, "pq_index_residual_clamped: not a PQ index");
  *out = h->pq_clamped;
  return RIHIP_OK;
}

extern "C" int rihip_pq_index_dims(void* handle, int* dsub, int* M) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && h->pq_codes && dsub && M, RIHIP_ERR_STATE, "pq_index_dims: not a PQ index");
  *dsub = h->pq_dsub; *M = h->dpad / h->pq_dsub;
  return RIHIP_OK;
}

extern "C" int rihip_pq_index_get_codes(void* handle, uint8_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && h->pq_codes && out, RIHIP_ERR_STATE, "pq_index_get_codes: not a PQ index");
  const int M = h->dpad / h->pq_dsub;
  uint8_t* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, (size_t)h->N * M));
  const int64_t tot = h->Np * M;
  hipLaunchKernelGGL(pq_codes_by_row_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, 0, h->pq_codes, h->row_ids, h->Np, M, d);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(out, d, (size_t)h->N * M, hipMemcpyDeviceToHost);
  hipFree(d);
  HIPCHK(e);
  return RIHIP_OK;
}

extern "C" int rihip_pq_index_get_codebooks(void* handle, int8_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && h->pq_codes && out, RIHIP_ERR_STATE, "pq_index_get_codebooks: not a PQ index");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out, h->pq_book, (size_t)h->dpad * 256, hipMemcpyDeviceToHost));
  return RIHIP_OK;
}

extern "C" int rihip_pq_index_train_stats(void* handle, int64_t* trace, int cap, int* n_trace, int64_t* peak_bytes, double* ms) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && h->pq_codes && n_trace, RIHIP_ERR_STATE, "pq_index_train_stats: not a PQ index");
  *n_trace = (int)h->pq_trace.size();
  if (trace) for (int i = 0; i < cap && i < *n_trace; ++i) trace[i] = h->pq_trace[i];
  if (peak_bytes) *peak_bytes = h->pq_peak_bytes;
  if (ms) for (int i = 0; i < 3; ++i) ms[i] = h->pq_ms[i];
  return RIHIP_OK;
}

// File: "RIHIPPQ1", int64 header {version 1, du, dk, dpad, N, Np, nlist, nprobe, dsub, M}, centre f32[dpad], scale
// f32[dpad], centroids f32[nlist, dk], list lengths int64[nlist], row ids int64[Np], codebooks int8[M, 256, dsub],
// entry numbers uint8[Np, M].  The codec is sq8_state.hip's; the format adds its two header words and its payload.
// Residual PQ file: "RIHIPPR1", the same with a third header word of its own {dsub, M, nlist * dpad} and the list codes
// int8[nlist, dpad] in front of the codebooks.  A "RIHIPPQ1" file is written and read as it always was.
namespace {

int pq_fill(Sq8Index* h, const int64_t* x, const int8_t* payload, const char* path) {
  const size_t book_bytes = (size_t)h->dpad * 256, code_bytes = (size_t)h->Np * x[1];
  for (size_t i = 0; i < book_bytes; ++i)
    RIHIP_REQUIRE(payload[i] != -128, RIHIP_ERR_IO, "pq_index_load: %s: codebook byte %lld is -128", path, (long long)i);
  h->pq_dsub = (int)x[0];
  HIPCHK(hipMalloc((void**)&h->pq_codes, code_bytes));
  HIPCHK(hipMalloc((void**)&h->pq_book, book_bytes));
  HIPCHK(hipMemcpy(h->pq_codes, payload + book_bytes, code_bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->pq_book, payload, book_bytes, hipMemcpyHostToDevice));
  h->pq_peak_bytes = sq8_held_bytes(h);
  return RIHIP_OK;
}

// the residual format's payload: list codes, then what pq_fill reads
int pq_residual_fill(Sq8Index* h, const int64_t* x, const int8_t* payload, const char* path) {
  const size_t nk = (size_t)h->nlist * h->dpad;
  RIHIP_REQUIRE((int64_t)nk == x[2], RIHIP_ERR_IO, "pq_index_load: %s: %lld list code bytes for %d lists of %d", path, (long long)x[2],
                h->nlist, h->dpad);
  for (size_t i = 0; i < nk; ++i)
    RIHIP_REQUIRE(payload[i] != -128, RIHIP_ERR_IO, "pq_index_load: %s: list code byte %lld is -128", path, (long long)i);
  RCCHK(pq_fill(h, x, payload + nk, path));
  HIPCHK(hipMalloc((void**)&h->pq_list_codes, nk));
  HIPCHK(hipMemcpy(h->pq_list_codes, payload, nk, hipMemcpyHostToDevice));
  h->pq_residual = true;
  h->pq_peak_bytes = sq8_held_bytes(h);
  return RIHIP_OK;
}

const Sq8StateFormat PQ_RESIDUAL_FORMAT = {
    "RIHIPPR1", "pq_index", "a residual PQ", 3,
    [](const int64_t* x, int64_t dpad) { return (x[0] == 8 || x[0] == 16) && x[1] * x[0] == dpad && x[2] >= dpad && x[2] % dpad == 0 && x[2] <= (int64_t)NLIST_MAX * dpad; },
    [](const int64_t* x, int64_t Np, int64_t dpad) { return x[2] + 256 * dpad + Np * x[1]; },
    pq_residual_fill,
};

const Sq8StateFormat PQ_FORMAT = {
    "RIHIPPQ1", "pq_index", "a PQ", 2,
    [](const int64_t* x, int64_t dpad) { return (x[0] == 8 || x[0] == 16) && x[1] * x[0] == dpad; },
    [](const int64_t* x, int64_t Np, int64_t dpad) { return 256 * dpad + Np * x[1]; },
    pq_fill,
};

}  // namespace

extern "C" int rihip_pq_index_save(void* handle, const char* path) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && path, RIHIP_ERR_ARG, "pq_index_save: bad arguments");
  RIHIP_REQUIRE(h->pq_codes, RIHIP_ERR_STATE, "pq_index_save: not a PQ index (an SQ8 index is saved by rihip_sq8_index_save)");
  const int64_t M = h->dpad / h->pq_dsub;
  const int64_t x[3] = {h->pq_dsub, M, (int64_t)h->nlist * h->dpad};
  const Sq8StateBlock blocks[3] = {{h->pq_list_codes, (size_t)x[2]}, {h->pq_book, (size_t)h->dpad * 256}, {h->pq_codes, (size_t)h->Np * M}};
  if (h->pq_residual) return sq8_state_save(h, path, PQ_RESIDUAL_FORMAT, x, blocks, 3);   // (a residual handle: its own format)
  return sq8_state_save(h, path, PQ_FORMAT, x, blocks + 1, 2);
}

extern "C" int rihip_pq_index_load_residual(const char* path, void** handle) { return sq8_state_load(path, PQ_RESIDUAL_FORMAT, handle); }

extern "C" int rihip_pq_index_load(const char* path, void** handle) { return sq8_state_load(path, PQ_FORMAT, handle); }

