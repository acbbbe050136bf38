// 8-bit index, opt-in refined search: the source's f32 rows attached next to the codes, an exact f32 re-score of the
// search's best k_scan candidates, and a per-query certificate that the re-ranked list is the exact one.
//
// Stage 1 is sq8_search (sq8.hip) at k_scan; stage 2 re-scores its candidates in f32 against the attached rows and selects
// the top k by (f, row); the certificate says when that list is the exact one over every probed row.  f, the bound and the
// certificate are specified at rihip_sq8_refine_search in recommendit_hip.h; the kernels below follow that text
// operation by operation (this file compiles with fp contract off, so a * b + c is two roundings unless written fmaf).
#pragma clang fp contract(off)
#include "common.h"
#include "recommendit_hip.h"

#include <algorithm>
#include <math.h>
#include <string.h>

#include "search_kernels.h"
#include "search_keys.h"
#include "sq8_index.h"

using namespace rihip_index;

namespace {

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
// BY_ROW: the f32 row of physical row r is X[row_ids[r]] (the insertion-order copy), else X[r] (a physical-order source).
// CT: int8, or the int16 decoded codes of a residual PQ handle (|c| <= 254: the product stays exact, 24 x 9 bits).
template <bool BY_ROW, typename CT>
__global__ __launch_bounds__(256) void sq8_range_part_kernel(const float* __restrict__ X, const CT* __restrict__ codes,
                                                             const int64_t* __restrict__ row_ids, int64_t n_rows, int dk, int dpad,
                                                             const float* __restrict__ centre, const float* __restrict__ scale,
                                                             double* part) {
  __shared__ double se[256], sa[256];
  const int tid = threadIdx.x, rpp = 256 / dk, rr = tid / dk, c = tid % dk;
  const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = (r0 + per < n_rows) ? r0 + per : n_rows;
  const double m = (double)centre[c], s = (double)scale[c];
  double e = 0.0, a = 0.0;
  for (int64_t r = r0 + rr; r < r1; r += rpp) {
    const int64_t row = row_ids[r];
    if (row < 0) continue;
    const double x = (double)X[(size_t)(BY_ROW ? row : r) * dk + c];
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
// one workgroup of 256 threads per column: thread t takes the blocks t, t + 256, ..., then thread 0 the 256 results in order
__global__ __launch_bounds__(256) void sq8_range_final_kernel(const double* __restrict__ part, int nb, int dk, double* e_out,
                                                              double* a_out) {
  __shared__ double se[256], sa[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  double e = 0.0, a = 0.0;
  for (int b = tid; b < nb; b += 256) { e = fmax(e, part[((size_t)b * 2 + 0) * dk + j]); a = fmax(a, part[((size_t)b * 2 + 1) * dk + j]); }
  se[tid] = e; sa[tid] = a;
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < 256; ++k) { e = fmax(e, se[k]); a = fmax(a, sa[k]); }
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
                                                       const float* __restrict__ out_scores, int k, int k_scan, double cmax,
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
  const double E2 = cmax * sum[1];   // cmax: the bound on |c_ij|, 127, or 254 on a residual PQ handle
  const double E3 = gamma * sum[2];
  const double W = cmax * sum[4];
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

// o: the predicates and seen lists of the whole batch; stage 1 is asked for rows, the id map is applied after the select
int sq8_search_refined(Sq8Index* h, const float* Q, int64_t nq, int k, int k_scan, int mode, float* out_s, int64_t* out_r,
                       uint8_t* out_cert, double* out_bound, hipStream_t st, Sq8SearchOpts o) {
  const int64_t ch = std::max<int64_t>(1, std::min<int64_t>(nq, (1ll << 24) / k_scan));   // stage-1 slots per pass: 2^24
  RCCHK(h->rs.reserve(ch * k_scan)); RCCHK(h->rr.reserve(ch * k_scan)); RCCHK(h->ri.reserve(ch * k_scan));
  RCCHK(h->rkeys.reserve(ch * k_scan)); RCCHK(h->rnv.reserve(ch)); RCCHK(h->rcut.reserve(ch));
  const uint32_t* pred = o.pred;
  o.map_ids = false;
  for (int64_t q0 = 0; q0 < nq; q0 += ch) {
    const int64_t n = std::min(ch, nq - q0);
    const float* Qc = Q + q0 * h->du;
    o.pred = pred ? pred + q0 * o.pred_stride : nullptr;
    o.q_base = q0;
    RCCHK(sq8_search(h, Qc, n, k_scan, mode, h->rs.p, h->rr.p, h->ri.p, st, o));
    RCCHK(dispatch_d(h->dk, [&](auto D) {
      hipLaunchKernelGGL((sq8_refine_kernel<decltype(D)::value>), dim3((unsigned)n), dim3(256), 0, st, h->vec, Qc, h->du, h->N, h->rr.p,
                         h->ri.p, k_scan, h->rkeys.p, h->rnv.p, h->rcut.p);
    }));
    RCCHK(check_launch("sq8 refine"));
    FinArgs f;
    memset(&f, 0, sizeof(f));
    f.nq = n; f.k = k; f.count = nullptr; f.cand = h->rkeys.p; f.cap = k_scan; f.mode = 0; f.out_scores = out_s + q0 * k;
    f.out_rows = out_r + q0 * k; f.id_map = h->id_map;
    RCCHK(launch_finalize(f, (unsigned)n, st));
    // (stage 1 left this pass's limbs, t and b in the handle's scratch)
    hipLaunchKernelGGL(sq8_cert_kernel, dim3((unsigned)n), dim3(128), 0, st, Qc, h->du, h->dk, h->dpad, h->centre, h->scale, h->ref_e,
                       h->ref_a, h->qhi.p, h->qlo.p, h->qt.p, h->qb.p, h->rnv.p, h->rcut.p, out_s + q0 * k, k, k_scan, h->pq_residual ? 254.0 : 127.0,
                       out_cert + q0,
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
  int16_t* decoded16 = nullptr;   // (a residual one: int16, twice that)
  auto work = [&]() -> int {
    if (h->pq_residual) RCCHK(pq_decode_all16(h, &decoded16, st));
    else if (!h->codes) RCCHK(pq_decode_all(h, &decoded, st));
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
    if (decoded16) sq8_launch_ranges(false, src->X, decoded16, h->row_ids, n_src, dk, h->dpad, h->centre, h->scale, part, nb, e, a, st);
    else sq8_launch_ranges(false, src->X, codes, h->row_ids, n_src, dk, h->dpad, h->centre, h->scale, part, nb, e, a, st);
    RCCHK(check_launch("sq8 attach vectors"));
    HIPCHK(hipStreamSynchronize(st));   // the source may be dropped as soon as the call returns
    return RIHIP_OK;
  };
  const int rc = work();
  hipFree(flag); hipFree(part); hipFree(decoded); hipFree(decoded16);
  if (rc) { hipFree(vec); hipFree(e); hipFree(a); return rc; }   // the handle is as it was
  sq8_drop_vectors(h);
  h->vec = vec; h->ref_e = e; h->ref_a = a;
  return RIHIP_OK;
}

}  // namespace

namespace {
template <typename CT>
void launch_ranges(bool by_row, const float* X, const CT* codes, const int64_t* row_ids, int64_t n_rows, int dk, int dpad,
                   const float* centre, const float* scale, double* part, int nb, double* e_out, double* a_out, hipStream_t st) {
  if (by_row) hipLaunchKernelGGL((sq8_range_part_kernel<true, CT>), dim3(nb), dim3(256), 0, st, X, codes, row_ids, n_rows, dk, dpad, centre, scale, part);
  else hipLaunchKernelGGL((sq8_range_part_kernel<false, CT>), dim3(nb), dim3(256), 0, st, X, codes, row_ids, n_rows, dk, dpad, centre, scale, part);
  hipLaunchKernelGGL(sq8_range_final_kernel, dim3(dk), dim3(256), 0, st, part, nb, dk, e_out, a_out);
}
}  // namespace

namespace rihip_index {
void sq8_launch_ranges(bool by_row, const float* X, const int8_t* codes, const int64_t* row_ids, int64_t n_rows, int dk, int dpad,
                       const float* centre, const float* scale, double* part, int nb, double* e_out, double* a_out, hipStream_t st) {
  launch_ranges(by_row, X, codes, row_ids, n_rows, dk, dpad, centre, scale, part, nb, e_out, a_out, st);
}
void sq8_launch_ranges(bool by_row, const float* X, const int16_t* codes, const int64_t* row_ids, int64_t n_rows, int dk, int dpad,
                       const float* centre, const float* scale, double* part, int nb, double* e_out, double* a_out, hipStream_t st) {
  launch_ranges(by_row, X, codes, row_ids, n_rows, dk, dpad, centre, scale, part, nb, e_out, a_out, st);
}
}  // namespace rihip_index

// ------------------------------------------------ C ABI --------------------------------------------------------------
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
  sq8_drop_vectors(h);
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
  RCCHK(sq8_check_search(h, {"sq8_refine_search", Q, nq, k, k_scan, mode, out_scores && out_rows && out_cert, false, nullptr, 0, nullptr}));
  return sq8_search_refined(h, Q, nq, k, k_scan, mode, out_scores, out_rows, out_cert, out_bound, (hipStream_t)stream, {});
}

extern "C" int rihip_sq8_refine_search_filtered(void* handle, const float* Q, int64_t nq, int k, int k_scan, int mode,
                                                const uint32_t* pred_dev, int64_t pred_stride, float* out_scores, int64_t* out_rows,
                                                uint8_t* out_cert, double* out_bound, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  RCCHK(sq8_check_search(h, {"sq8_refine_search_filtered", Q, nq, k, k_scan, mode, out_scores && out_rows && out_cert, true, pred_dev,
                             pred_stride, nullptr}));
  Sq8SearchOpts o;
  o.pred = pred_dev; o.pred_stride = (int)pred_stride;
  return sq8_search_refined(h, Q, nq, k, k_scan, mode, out_scores, out_rows, out_cert, out_bound, (hipStream_t)stream, o);
}

extern "C" int rihip_sq8_refine_search_excluding(void* handle, const float* Q, int64_t nq, int k, int k_scan, int mode,
                                                 const int64_t* user_ids, const int64_t* seen_offsets, int64_t n_seen_rows,
                                                 const int32_t* seen_items, const int32_t* row_of, int64_t n_ids,
                                                 const uint32_t* pred_dev, int64_t pred_stride, float* out_scores,
                                                 int64_t* out_rows, uint8_t* out_cert, double* out_bound, void* stream) {
  Sq8Index* h = (Sq8Index*)handle;
  const SeenArgs sn{user_ids, seen_offsets, n_seen_rows, seen_items, row_of, n_ids};
  RCCHK(sq8_check_search(h, {"sq8_refine_search_excluding", Q, nq, k, k_scan, mode, out_scores && out_rows && out_cert, false, pred_dev,
                             pred_stride, &sn}));
  Sq8SearchOpts o;
  o.pred = pred_dev; o.pred_stride = (int)pred_stride; o.seen = &sn;
  return sq8_search_refined(h, Q, nq, k, k_scan, mode, out_scores, out_rows, out_cert, out_bound, (hipStream_t)stream, o);
}
