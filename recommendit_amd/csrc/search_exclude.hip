// Seen-item exclusion inside the index scan (rihip_ip_index_search_excluding): the per-query exclusion mask and the
// passing-row counts under it.  One bit per (query, scanned row): bit p & 31 of mask[q * W + (p >> 5)] is set iff the row
// at scan position p (flat: the row; IVF: the list-major physical position) is excluded for query q.  Lists are padded
// to 64 rows and tiles are 32 rows, so a tile of the list-major scan and of the stride-1 flat scan is one aligned word.
#include "search_kernels.h"
#include "search_keys.h"

using namespace rihip_index;

namespace {

constexpr int XM_SLICES = 8;   // workgroups per query of the builder: a 20 000-item list is 10 entries per thread

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void inv_pos_kernel(const int64_t* __restrict__ row_ids, int64_t Np, int* inv_pos) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= Np) return;
  const int64_t r = row_ids[p];
  if (r >= 0) inv_pos[r] = (int)p;
}

// Work is spread over (query, seen entry): workgroup (q, slice) strides over the list of the query's user.  Two queries of
// one user each own a mask row.  set = 0 is the same walk storing zero words: the clear costs what the build cost.
__global__ __launch_bounds__(256) void xmask_kernel(SeenArgs s, int64_t q0, const int* __restrict__ inv_pos, int64_t N,
                                                    uint32_t* mask, int64_t W, int set) {
  const int64_t q = blockIdx.x;
  const int64_t u = s.user_ids ? s.user_ids[q0 + q] : q0 + q;
  if (u < 0 || u >= s.n_seen_rows) return;
  const int64_t b = s.seen_offsets[u], e = s.seen_offsets[u + 1];
  uint32_t* row = mask + (size_t)q * W;
  for (int64_t j = b + (int64_t)blockIdx.y * 256 + threadIdx.x; j < e; j += (int64_t)gridDim.y * 256) {
    const int64_t id = s.seen_items[j];
    if (id < 0 || id >= s.n_ids) continue;
    const int64_t r = s.row_of[id];
    if (r < 0 || r >= N) continue;
    const int64_t p = inv_pos ? inv_pos[r] : r;
    if (p < 0 || (p >> 5) >= W) continue;
    if (set) atomicOr(&row[p >> 5], 1u << (p & 31));
    else row[p >> 5] = 0u;
  }
}

// flat index: n_pass[q] = #{r < N : row r passes query q and is not masked}; workgroup (row block, query), a word of the
// mask per thread and step (untagged: 32 rows by one popcount)
constexpr int CNT_WORDS = 4096;   // mask words per workgroup
__global__ __launch_bounds__(256) void count_pass_x_kernel(const uint32_t* __restrict__ tags, int64_t N,
                                                           const uint32_t* __restrict__ pred, int pred_stride,
                                                           const uint32_t* __restrict__ xmask, int64_t W, int* n_pass) {
  const int64_t q = blockIdx.y;
  const uint32_t* row = xmask + (size_t)q * W;
  Pred pr{0u, 0u, 0u};
  if (tags) pr = load_pred(pred, q, pred_stride);
  const int64_t w0 = (int64_t)blockIdx.x * CNT_WORDS;
  const int64_t w1 = (w0 + CNT_WORDS < W) ? w0 + CNT_WORDS : W;
  int cnt = 0;
  for (int64_t w = w0 + threadIdx.x; w < w1; w += 256) {
    const int64_t r0 = w * 32;
    const int n = (N - r0) < 32 ? (int)(N - r0) : 32;
    uint32_t ok = ~row[w];
    if (n < 32) ok &= (1u << n) - 1u;
    if (tags) {
      for (int i = 0; i < n; ++i)
        if (!pr.pass(tags[r0 + i])) ok &= ~(1u << i);
    }
    cnt += __popc(ok);
  }
  cnt = wave_sum_i(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&n_pass[q], cnt);
}

// IVF: n_pass[q] += such rows of query q's probed lists; one workgroup per (query, probe) pair
__global__ __launch_bounds__(256) void count_pass_ivf_x_kernel(const uint32_t* __restrict__ tags, const int64_t* __restrict__ list_poff,
                                                               const int* __restrict__ list_len, const int* __restrict__ probe_list,
                                                               int nprobe, const uint32_t* __restrict__ pred, int pred_stride,
                                                               const uint32_t* __restrict__ xmask, int64_t W, int* n_pass) {
  const int64_t pair = blockIdx.x;
  const int c = probe_list[pair];
  if (c < 0) return;
  const int64_t q = pair / nprobe;
  Pred pr{0u, 0u, 0u};
  if (tags) pr = load_pred(pred, q, pred_stride);
  const int64_t p0 = list_poff[c];
  const uint32_t* row = xmask + (size_t)q * W;
  const int len = list_len[c];
  int cnt = 0;
  for (int i = threadIdx.x; i < len; i += 256) {
    const int64_t p = p0 + i;
    const bool masked = (row[p >> 5] >> (p & 31)) & 1u;
    cnt += (int)(!masked && (!tags || pr.pass(tags[p])));
  }
  cnt = wave_sum_i(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&n_pass[q], cnt);
}

__global__ __launch_bounds__(256) void count_nonzero_kernel(const uint32_t* __restrict__ buf, int64_t n, unsigned long long* out) {
  int cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) cnt += (int)(buf[i] != 0u);
  cnt = wave_sum_i(cnt);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(out, (unsigned long long)cnt);
}

}  // namespace

namespace rihip_index {

void launch_inv_pos(const int64_t* row_ids, int64_t Np, int* inv_pos, hipStream_t st) {
  hipLaunchKernelGGL(inv_pos_kernel, dim3((unsigned)((Np + 255) / 256)), dim3(256), 0, st, row_ids, Np, inv_pos);
}

void launch_xmask(const SeenArgs& s, int64_t q0, int64_t nq, const int* inv_pos, int64_t N, uint32_t* mask, int64_t W, int set,
                  hipStream_t st) {
  hipLaunchKernelGGL(xmask_kernel, dim3((unsigned)nq, XM_SLICES), dim3(256), 0, st, s, q0, inv_pos, N, mask, W, set);
}

void launch_count_pass_x(const uint32_t* tags, int64_t N, const uint32_t* pred, int pred_stride, const uint32_t* xmask, int64_t W,
                         int64_t nq, int* n_pass, hipStream_t st) {
  hipLaunchKernelGGL(count_pass_x_kernel, dim3((unsigned)((W + CNT_WORDS - 1) / CNT_WORDS), (unsigned)nq), dim3(256), 0, st, tags, N,
                     pred, pred_stride, xmask, W, n_pass);
}

void launch_count_pass_ivf_x(const uint32_t* tags, const int64_t* list_poff, const int* list_len, const int* probe_list, int64_t nq,
                             int nprobe, const uint32_t* pred, int pred_stride, const uint32_t* xmask, int64_t W, int* n_pass,
                             hipStream_t st) {
  hipLaunchKernelGGL(count_pass_ivf_x_kernel, dim3((unsigned)(nq * nprobe)), dim3(256), 0, st, tags, list_poff, list_len, probe_list,
                     nprobe, pred, pred_stride, xmask, W, n_pass);
}

void launch_count_nonzero(const uint32_t* buf, int64_t n, unsigned long long* out, hipStream_t st) {
  if (n <= 0) return;
  int64_t g = (n + 255) / 256;
  if (g > 4 * RIHIP_NCU) g = 4 * RIHIP_NCU;
  hipLaunchKernelGGL(count_nonzero_kernel, dim3((unsigned)g), dim3(256), 0, st, buf, n, out);
}

}  // namespace rihip_index
