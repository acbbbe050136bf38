// Helper kernels of the filtered search (rihip_ip_index_search_filtered).
#include "search_kernels.h"
#include "search_keys.h"

using namespace rihip_index;

namespace {

// The thresholded searches assume that about k*S/N of the sample beats the threshold and that at least min(k, N)
// candidates exist.  Under a predicate both depend on how many rows PASS, so the filtered search counts them first.
constexpr int CNT_TAGS = 4096;   // tag words staged in LDS per workgroup of the flat count
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// flat index, per-query predicates: n_pass[q] = #{r < N : row r passes query q}.  A workgroup stages CNT_TAGS tag words in
// LDS and every thread tests all of them against its own query's predicate (broadcast LDS reads, 16 bytes at a time).
__global__ __launch_bounds__(256) void count_pass_kernel(const uint32_t* __restrict__ tags, int64_t N,
                                                         const uint32_t* __restrict__ pred, int64_t nq, int* n_pass) {
  __shared__ __attribute__((aligned(16))) uint32_t Tg[CNT_TAGS];
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * CNT_TAGS;
  const int n = (int)((N - r0) < CNT_TAGS ? (N - r0) : CNT_TAGS);
  for (int i = tid; i < CNT_TAGS; i += 256) Tg[i] = i < n ? tags[r0 + i] : 0u;
  __syncthreads();
  const int64_t q = (int64_t)blockIdx.y * 256 + tid;
  if (q >= nq) return;
  const Pred pr = load_pred(pred, q, 3);
  int cnt = 0;
  const int n4 = n & ~3;
  for (int i = 0; i < n4; i += 4) {
    const uint4 t = *reinterpret_cast<const uint4*>(&Tg[i]);
    cnt += (int)pr.pass(t.x) + (int)pr.pass(t.y) + (int)pr.pass(t.z) + (int)pr.pass(t.w);
  }
  for (int i = n4; i < n; ++i) cnt += (int)pr.pass(Tg[i]);
  if (cnt) atomicAdd(&n_pass[q], cnt);
}
// flat index, one shared predicate: n_pass[0] = #{r < N : row r passes}; a thread per row, one atomic per wave
__global__ __launch_bounds__(256) void count_pass_shared_kernel(const uint32_t* __restrict__ tags, int64_t N,
                                                                const uint32_t* __restrict__ pred, int* n_pass) {
  const Pred pr = load_pred(pred, 0, 0);
  int cnt = 0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < N; r += (int64_t)gridDim.x * 256) cnt += (int)pr.pass(tags[r]);
  cnt = wave_sum_i(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_pass, cnt);
}
// IVF: n_pass[q] = passing rows of query q's probed lists; one workgroup per (query, probe) pair over the list's tag run
__global__ __launch_bounds__(256) void count_pass_ivf_kernel(const uint32_t* __restrict__ tags, const int64_t* __restrict__ list_poff,
                                                             const int* __restrict__ list_len, const int* __restrict__ probe_list,
                                                             int nprobe, const uint32_t* __restrict__ pred, int pred_stride,
                                                             int* n_pass) {
  const int64_t pair = blockIdx.x;
  const int c = probe_list[pair];
  if (c < 0) return;
  const int64_t q = pair / nprobe;
  const Pred pr = load_pred(pred, q, pred_stride);
  const uint32_t* t = tags + list_poff[c];
  const int len = list_len[c];
  int cnt = 0;
  for (int i = threadIdx.x; i < len; i += 256) cnt += (int)pr.pass(t[i]);
  cnt = wave_sum_i(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&n_pass[q], cnt);
}
// The sample's rank-th best is key 0 when fewer than `rank` sampled rows pass, and ord2f(0) is a NaN that `score >= thr`
// rejects for every row: such a query keeps EVERY passing row (thr = -inf), and so does one whose passing rows all fit
// the candidate list.
__global__ void filt_thr_kernel(float* thr, const int* __restrict__ n_pass, int n_pass_stride, int64_t cap, int64_t nq) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const float t = thr[q];
  if (t != t || (int64_t)n_pass[q * n_pass_stride] <= cap) thr[q] = -INFINITY;
}
__global__ void gather_pred_kernel(const uint32_t* __restrict__ pred, const int* __restrict__ idx, int n, uint32_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * 3) out[i] = pred[(size_t)idx[i / 3] * 3 + (i % 3)];
}
// tags in insertion-row order -> the order the IVF scan reads them (padding slots 0)
__global__ void tags_to_scan_order_kernel(const uint32_t* __restrict__ by_row, const int64_t* __restrict__ row_ids, int64_t Np,
                                          uint32_t* out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < Np) { const int64_t r = row_ids[p]; out[p] = r >= 0 ? by_row[r] : 0u; }
}

}  // namespace

namespace rihip_index {

void launch_count_pass(const uint32_t* tags, int64_t N, const uint32_t* pred, int pred_stride, int64_t nq, int* n_pass,
                       hipStream_t st) {
  if (pred_stride) hipLaunchKernelGGL(count_pass_kernel, dim3((unsigned)((N + CNT_TAGS - 1) / CNT_TAGS), (unsigned)((nq + 255) / 256)),
                                      dim3(256), 0, st, tags, N, pred, nq, n_pass);
  else hipLaunchKernelGGL(count_pass_shared_kernel, dim3(2 * RIHIP_NCU), dim3(256), 0, st, tags, N, pred, n_pass);
}

void launch_count_pass_ivf(const uint32_t* tags, const int64_t* list_poff, const int* list_len, const int* probe_list,
                           int64_t nq, int nprobe, const uint32_t* pred, int pred_stride, int* n_pass, hipStream_t st) {
  hipLaunchKernelGGL(count_pass_ivf_kernel, dim3((unsigned)(nq * nprobe)), dim3(256), 0, st, tags, list_poff, list_len,
                     probe_list, nprobe, pred, pred_stride, n_pass);
}

void launch_filt_thr(float* thr, const int* n_pass, int n_pass_stride, int64_t cap, int64_t nq, hipStream_t st) {
  hipLaunchKernelGGL(filt_thr_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, thr, n_pass, n_pass_stride, cap, nq);
}

void launch_gather_pred(const uint32_t* pred, const int* idx, int n, uint32_t* out, hipStream_t st) {
  hipLaunchKernelGGL(gather_pred_kernel, dim3((unsigned)((n * 3 + 255) / 256)), dim3(256), 0, st, pred, idx, n, out);
}

void launch_tags_to_scan_order(const uint32_t* by_row, const int64_t* row_ids, int64_t Np, uint32_t* out, hipStream_t st) {
  hipLaunchKernelGGL(tags_to_scan_order_kernel, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, st, by_row, row_ids, Np, out);
}

}  // namespace rihip_index
