// 8-bit scalar-quantised inner-product index: the quantiser kernels, the build, the handle's lifetime and its accessors.
//
// A second handle type next to IpIndex.  It is built from the f32 rows of a built IpIndex, in that index's physical order
// (lists padded to 64-row granules; a flat source becomes one list), and stores one int8 code per dimension:
//   m_j = 0.5f (lo_j + hi_j), s_j = (hi_j - lo_j) / 254.0f (1 where hi_j == lo_j), c_ij = clamp(rint((x_ij - m_j) / s_j), +-127)
// The search is sq8.hip's over sq8_scan.hip's kernel.  A handle may hold product-quantised storage instead of the int8
// matrix (pq.hip builds it on top of sq8_build).
#pragma clang fp contract(off)   // the quantiser is specified operation by operation: no fused multiply-add
#include "common.h"
#include "recommendit_hip.h"

#include <algorithm>
#include <math.h>
#include <vector>

#include "search_kernels.h"
#include "sq8_index.h"

using namespace rihip_index;

namespace {

// ------------------------------------------------ quantiser ----------------------------------------------------------
// column min / max of the real rows, fixed order: block b takes a contiguous row range, thread (rr, c) every rpp-th row of
// column c, the rpp partial results of a column are combined in rr order, the blocks' results in block order (no atomics)
__global__ __launch_bounds__(256) void sq8_colrange_part_kernel(const float* __restrict__ X, const int64_t* __restrict__ row_ids,
                                                                int64_t n_rows, int dk, float* part) {
  __shared__ float slo[256], shi[256];
  const int tid = threadIdx.x, rpp = 256 / dk, rr = tid / dk, c = tid % dk;
  const int64_t per = (n_rows + gridDim.x - 1) / gridDim.x;
  const int64_t r0 = (int64_t)blockIdx.x * per, r1 = (r0 + per < n_rows) ? r0 + per : n_rows;
  float lo = INFINITY, hi = -INFINITY;
  for (int64_t r = r0 + rr; r < r1; r += rpp) {
    if (row_ids && row_ids[r] < 0) continue;
    const float v = X[(size_t)r * dk + c];
    lo = fminf(lo, v); hi = fmaxf(hi, v);
  }
  slo[tid] = lo; shi[tid] = hi;
  __syncthreads();
  if (rr == 0) {
    for (int k = 1; k < rpp; ++k) { lo = fminf(lo, slo[k * dk + c]); hi = fmaxf(hi, shi[k * dk + c]); }
    part[((size_t)blockIdx.x * 2 + 0) * dk + c] = lo;
    part[((size_t)blockIdx.x * 2 + 1) * dk + c] = hi;
  }
}
__global__ void sq8_colrange_final_kernel(const float* __restrict__ part, int nb, int dk, int dpad, float* centre, float* scale) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= dpad) return;
  float m = 0.f, s = 1.f;
  if (j < dk) {
    float lo = INFINITY, hi = -INFINITY;
    for (int b = 0; b < nb; ++b) { lo = fminf(lo, part[((size_t)b * 2 + 0) * dk + j]); hi = fmaxf(hi, part[((size_t)b * 2 + 1) * dk + j]); }
    if (lo <= hi) {
      m = 0.5f * (lo + hi);
      s = (hi == lo) ? 1.f : (hi - lo) / 254.0f;
    }
  }
  centre[j] = m; scale[j] = s;
}

// four codes per thread; rows beyond n_src, padding rows (row_ids < 0) and columns >= dk are 0
__global__ void sq8_encode_kernel(const float* __restrict__ X, const int64_t* __restrict__ row_ids, int64_t n_src, int64_t Np,
                                  int dk, int dpad, const float* __restrict__ centre, const float* __restrict__ scale,
                                  int8_t* codes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_row = dpad / 4;
  if (i >= Np * per_row) return;
  const int64_t r = i / per_row;
  const int j = (int)(i % per_row) * 4;
  uint32_t packed = 0;
  if (r < n_src && j < dk && row_ids[r] >= 0) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(X + (size_t)r * dk + j);
#pragma unroll
    for (int u = 0; u < 4; ++u) packed |= ((uint32_t)sq8_code(x[u], centre[j + u], scale[j + u]) & 0xFFu) << (8 * u);
  }
  *reinterpret_cast<uint32_t*>(codes + (size_t)r * dpad + j) = packed;
}

__global__ void sq8_identity_rows_kernel(int64_t* row_ids, int64_t N, int64_t Np) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Np) row_ids[i] = i < N ? i : -1;
}

// decoded rows in original row order: out[row, j] = m_j + s_j c (two roundings).  CT: int8, or the int16 decoded codes of
// a residual PQ handle (|c| <= 254: (float)c and s_j * c round as for int8)
template <typename CT>
__global__ void sq8_reconstruct_kernel(const CT* __restrict__ codes, const int64_t* __restrict__ row_ids, int64_t Np, int du,
                                       int dpad, const float* __restrict__ centre, const float* __restrict__ scale, float* out,
                                       CT* out_codes) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Np * du) return;
  const int64_t p = i / du;
  const int j = (int)(i % du);
  const int64_t row = row_ids[p];
  if (row < 0) return;
  const CT c = codes[(size_t)p * dpad + j];
  if (out_codes) out_codes[(size_t)row * du + j] = c;
  if (out) {
    const float prod = scale[j] * (float)c;
    out[(size_t)row * du + j] = centre[j] + prod;
  }
}

}  // namespace

namespace rihip_index {

// out_c: int8 [N, du], or int16 [N, du] on a residual PQ handle
int sq8_rows_out(Sq8Index* h, float* out_x, void* out_c) {
  const bool wide = h->pq_residual;
  const size_t n = (size_t)h->N * h->du, cb = wide ? 2 * n : n;
  float* dx = nullptr; void* dc = nullptr;
  if (out_x) HIPCHK(hipMalloc((void**)&dx, sizeof(float) * n));
  if (out_c && hipMalloc(&dc, cb) != hipSuccess) { hipFree(dx); rihip_set_error("sq8_index: device allocation failed"); return RIHIP_ERR_HIP; }
  int8_t* decoded = nullptr;     // a PQ handle: its decoded code matrix, a transient Np * dpad bytes
  int16_t* decoded16 = nullptr;  // (a residual one: twice that)
  if (wide ? pq_decode_all16(h, &decoded16, 0) != RIHIP_OK : (!h->codes && pq_decode_all(h, &decoded, 0) != RIHIP_OK)) {
    hipFree(dx); hipFree(dc); return RIHIP_ERR_HIP;
  }
  const int64_t tot = h->Np * h->du;
  const dim3 grid((unsigned)((tot + 255) / 256));
  if (wide)
    hipLaunchKernelGGL(sq8_reconstruct_kernel<int16_t>, grid, dim3(256), 0, 0, decoded16, h->row_ids, h->Np, h->du, h->dpad, h->centre,
                       h->scale, dx, (int16_t*)dc);
  else
    hipLaunchKernelGGL(sq8_reconstruct_kernel<int8_t>, grid, dim3(256), 0, 0, h->codes ? h->codes : decoded, h->row_ids, h->Np, h->du,
                       h->dpad, h->centre, h->scale, dx, (int8_t*)dc);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && out_x) e = hipMemcpy(out_x, dx, sizeof(float) * n, hipMemcpyDeviceToHost);
  if (e == hipSuccess && out_c) e = hipMemcpy(out_c, dc, cb, hipMemcpyDeviceToHost);
  hipFree(dx); hipFree(dc); hipFree(decoded); hipFree(decoded16);
  HIPCHK(e);
  return RIHIP_OK;
}

int64_t sq8_held_bytes(const Sq8Index* h) {
  // the code storage: the int8 matrix, or (a PQ handle) one byte per sub-space and row plus the codebooks
  const int64_t rows = h->pq_codes ? h->Np * (h->dpad / h->pq_dsub) + 256 * (int64_t)h->dpad : h->Np * h->dpad;
  return rows + (h->pq_list_codes ? (int64_t)h->nlist * h->dpad : 0) + 2 * 4 * (int64_t)h->dpad +4 * (int64_t)h->nlist * h->dk + 8 * (int64_t)(h->nlist + 1) +
         4 * (int64_t)h->nlist + 8 * h->Np + (h->vec ? 4 * h->N * h->dk + 2 * 8 * (int64_t)h->dk : 0) + (h->tags ? 4 * h->Np : 0);
}

void sq8_drop_tags(Sq8Index* h) {
  if (!h->tags) return;
  rihip_bump_generation();
  hipFree(h->tags);
  h->tags = nullptr;
}

void sq8_drop_vectors(Sq8Index* h) {
  if (!h->vec) return;
  rihip_bump_generation();
  hipFree(h->vec); hipFree(h->ref_e); hipFree(h->ref_a);
  h->vec = nullptr; h->ref_e = nullptr; h->ref_a = nullptr;
}

void sq8_free(Sq8Index* h) {
  rihip_bump_generation();
  sq8_drop_vectors(h);
  sq8_drop_tags(h);
  h->fpred.release(); h->xmask.release();
  hipFree(h->inv_pos);
  h->rs.release(); h->rr.release(); h->ri.release(); h->rnv.release(); h->rcut.release(); h->rkeys.release();
  hipFree(h->codes); hipFree(h->pq_codes); hipFree(h->pq_book); hipFree(h->pq_list_codes); hipFree(h->centre); hipFree(h->scale); hipFree(h->C); hipFree(h->list_poff); hipFree(h->list_len_dev);
  hipFree(h->row_ids);
  h->qhi.release(); h->qlo.release(); h->fhi.release(); h->flo.release(); h->qt.release(); h->qpad.release(); h->fQ.release();
  h->coarse.release(); h->thr.release(); h->qb.release(); h->cand.release(); h->scand.release(); h->fcand.release();
  h->count.release(); h->probe_list.release(); h->list_q.release(); h->list_cnt.release(); h->list_qoff.release();
  h->list_cur.release(); h->work_off.release(); h->plan.release(); h->fail_flags.release(); h->fail_list.release();
  h->n_fail.release(); h->pair_t.release();
  if (h->h_nfail) hipHostFree(h->h_nfail);
  delete h;
}

// list offsets / lengths on the device from the host copy list_len (lists padded to 64-row granules)
int sq8_upload_layout(Sq8Index* h, hipStream_t st) {
  std::vector<int64_t> poff(h->nlist + 1, 0);
  std::vector<int> len(h->nlist);
  for (int c = 0; c < h->nlist; ++c) {
    poff[c + 1] = poff[c] + (h->list_len[c] + TR - 1) / TR * TR;
    len[c] = (int)h->list_len[c];
  }
  RIHIP_REQUIRE(poff[h->nlist] == h->Np, RIHIP_ERR_STATE, "sq8_index: list lengths give %lld padded rows, the index holds %lld",
                (long long)poff[h->nlist], (long long)h->Np);
  HIPCHK(hipMalloc((void**)&h->list_poff, sizeof(int64_t) * (h->nlist + 1)));
  HIPCHK(hipMalloc((void**)&h->list_len_dev, sizeof(int) * h->nlist));
  HIPCHK(hipMemcpyAsync(h->list_poff, poff.data(), sizeof(int64_t) * (h->nlist + 1), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->list_len_dev, len.data(), sizeof(int) * h->nlist, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));   // (the host vectors go away)
  return RIHIP_OK;
}

int sq8_build(Sq8Index* h, const IpIndex* src, const float* centre, const float* scale, hipStream_t st) {
  h->du = src->du; h->dk = src->d; h->dpad = src->d <= 64 ? 64 : 128;
  h->N = src->N;
  h->nprobe = src->ivf ? src->nprobe : 1;
  const int64_t n_src = src->ivf ? src->Np : src->N;
  if (src->ivf) {
    RIHIP_REQUIRE(src->C && src->row_ids && (int)src->list_len.size() == src->nlist && src->nlist >= 1, RIHIP_ERR_STATE,
                  "sq8_index_from_ip_index: the IVF source is incomplete");
    h->nlist = src->nlist; h->Np = src->Np; h->list_len = src->list_len;
  } else {
    h->nlist = 1; h->Np = (src->N + TR - 1) / TR * TR; h->list_len.assign(1, src->N);
  }
  RCCHK(sq8_upload_layout(h, st));
  HIPCHK(hipMalloc((void**)&h->row_ids, sizeof(int64_t) * (size_t)h->Np));
  HIPCHK(hipMalloc((void**)&h->C, sizeof(float) * (size_t)h->nlist * h->dk));
  HIPCHK(hipMalloc((void**)&h->codes, (size_t)h->Np * h->dpad));
  HIPCHK(hipMalloc((void**)&h->centre, sizeof(float) * h->dpad));
  HIPCHK(hipMalloc((void**)&h->scale, sizeof(float) * h->dpad));
  if (src->ivf) {
    HIPCHK(hipMemcpyAsync(h->row_ids, src->row_ids, sizeof(int64_t) * (size_t)h->Np, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(h->C, src->C, sizeof(float) * (size_t)h->nlist * h->dk, hipMemcpyDeviceToDevice, st));
  } else {
    hipLaunchKernelGGL(sq8_identity_rows_kernel, dim3((unsigned)((h->Np + 255) / 256)), dim3(256), 0, st, h->row_ids, h->N, h->Np);
    HIPCHK(hipMemsetAsync(h->C, 0, sizeof(float) * (size_t)h->dk, st));
  }
  if (centre) {   // injected quantiser: [du] host arrays, columns beyond du are (0, 1)
    std::vector<float> m(h->dpad, 0.f), s(h->dpad, 1.f);
    for (int j = 0; j < h->du; ++j) {
      RIHIP_REQUIRE(isfinite(centre[j]) && isfinite(scale[j]) && scale[j] > 0.f, RIHIP_ERR_ARG,
                    "sq8_index_from_ip_index: column %d: centre %g, scale %g (finite, scale > 0)", j, (double)centre[j], (double)scale[j]);
      m[j] = centre[j]; s[j] = scale[j];
    }
    HIPCHK(hipMemcpyAsync(h->centre, m.data(), sizeof(float) * h->dpad, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(h->scale, s.data(), sizeof(float) * h->dpad, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
  } else {
    const int nb = (int)std::min<int64_t>(1024, (n_src + 255) / 256);
    float* part = nullptr;
    HIPCHK(hipMalloc((void**)&part, sizeof(float) * (size_t)nb * 2 * h->dk));
    hipLaunchKernelGGL(sq8_colrange_part_kernel, dim3(nb), dim3(256), 0, st, src->X, src->ivf ? h->row_ids : nullptr, n_src, h->dk, part);
    hipLaunchKernelGGL(sq8_colrange_final_kernel, dim3(1), dim3(128), 0, st, part, nb, h->dk, h->dpad, h->centre, h->scale);
    const hipError_t e = hipStreamSynchronize(st);
    hipFree(part);
    HIPCHK(e);
  }
  const int64_t nthr = h->Np * (h->dpad / 4);
  hipLaunchKernelGGL(sq8_encode_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, src->X, h->row_ids, n_src, h->Np, h->dk,
                     h->dpad, h->centre, h->scale, h->codes);
  RCCHK(check_launch("sq8 encode"));
  HIPCHK(hipStreamSynchronize(st));   // the source may be dropped as soon as the call returns
  return RIHIP_OK;
}

}  // namespace rihip_index

// ------------------------------------------------ C ABI --------------------------------------------------------------
extern "C" int rihip_sq8_index_from_ip_index(void* ip_handle, const float* centre, const float* scale, void** handle, void* stream) {
  const IpIndex* src = (const IpIndex*)ip_handle;
  RIHIP_REQUIRE(src && handle, RIHIP_ERR_ARG, "sq8_index_from_ip_index: null handle");
  RIHIP_REQUIRE(src->X && src->N > 0, RIHIP_ERR_STATE, "sq8_index_from_ip_index: the source index is empty");
  RIHIP_REQUIRE((centre == nullptr) == (scale == nullptr), RIHIP_ERR_ARG, "sq8_index_from_ip_index: give both centre and scale, or neither");
  Sq8Index* h = new Sq8Index();
  const int rc = sq8_build(h, src, centre, scale, (hipStream_t)stream);
  if (rc) { sq8_free(h); return rc; }
  *handle = h;
  return RIHIP_OK;
}

extern "C" int rihip_sq8_index_destroy(void* handle) {
  if (handle) sq8_free((Sq8Index*)handle);
  return RIHIP_OK;
}

extern "C" int64_t rihip_sq8_index_ntotal(void* handle) { return handle ? ((Sq8Index*)handle)->N : 0; }
extern "C" int rihip_sq8_index_nlist(void* handle) { return handle ? ((Sq8Index*)handle)->nlist : 0; }

extern "C" int rihip_sq8_index_set_nprobe(void* handle, int nprobe) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && nprobe >= 1, RIHIP_ERR_ARG, "sq8_index_set_nprobe: bad arguments");
  h->nprobe = nprobe;
  return RIHIP_OK;
}

extern "C" int rihip_sq8_index_set_id_map(void* handle, const int64_t* item_ids_dev) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h, RIHIP_ERR_ARG, "sq8_index_set_id_map: null handle");
  h->id_map = item_ids_dev;
  return RIHIP_OK;
}

extern "C" int rihip_sq8_index_get_quantizer(void* handle, float* centre, float* scale) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && centre && scale, RIHIP_ERR_ARG, "sq8_index_get_quantizer: bad arguments");
  HIPCHK(hipMemcpy(centre, h->centre, sizeof(float) * h->du, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(scale, h->scale, sizeof(float) * h->du, hipMemcpyDeviceToHost));
  return RIHIP_OK;
}

extern "C" int rihip_sq8_index_get_codes(void* handle, int8_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "sq8_index_get_codes: bad arguments");
  RIHIP_REQUIRE(!h->pq_residual, RIHIP_ERR_STATE,
                "sq8_index_get_codes: the decoded codes of a residual PQ index are 16-bit (rihip_pq_index_get_decoded16)");
  return sq8_rows_out(h, nullptr, out);
}

extern "C" int rihip_sq8_index_reconstruct(void* handle, float* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "sq8_index_reconstruct: bad arguments");
  return sq8_rows_out(h, out, nullptr);
}

extern "C" int rihip_sq8_index_stats(void* handle, int64_t* out) {
  Sq8Index* h = (Sq8Index*)handle;
  RIHIP_REQUIRE(h && out, RIHIP_ERR_ARG, "sq8_index_stats: bad arguments");
  out[0] = h->stats[0]; out[1] = h->stats[1]; out[2] = sq8_held_bytes(h);
  return RIHIP_OK;
}
