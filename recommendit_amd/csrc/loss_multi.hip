// Sampled-negative BPR with K negatives per positive (not in the reference, which trains one negative per positive):
//   z_ik = u_i.p_i - u_i.n_ik,  L = 1/(B K) sum_ik softplus(-z_ik),  g_ik = sigma(-z_ik) / (B K)
//   dN_ik = g_ik u_i,  dP_i = -(sum_k g_ik) u_i,  dU_i = -sum_k g_ik (p_i - n_ik)
// N and dN are k-major ([K, B, d]: negative k of sample i is row k B + i), so K = 1 is the pos || neg layout of the pair
// loss and is handed to rihip_bpr_pair_loss.  The kernel is bandwidth-bound ((2 + K) B d 4 bytes each way): a lane group
// keeps its 16 bytes of u_i and p_i in registers across the k loop, the rows of KU negatives are requested before the
// first of them is used, dU and dP are written once after the loop.  Operation order: the contract in recommendit_hip.h.
#include "common.h"
#include "recommendit_hip.h"

namespace {

constexpr int KU = 4;   // negatives in flight per lane group

// softplus(-z) and g = sigma(-z) * inv: the stable branches of bpr_pair_v4_kernel
__device__ __forceinline__ float multi_pair(float z, float inv, float& loss) {
  const float e = expf(-fabsf(z));
  loss = fmaxf(-z, 0.f) + log1pf(e);
  const float sig_neg = (z >= 0.f) ? e / (1.f + e) : 1.f / (1.f + e);  // sigmoid(-z)
  return sig_neg * inv;
}

// float4 form: LPR lanes per row, 64/LPR rows per wave side by side.  FULL (the tuned d = 32 / 64 / 128): d = 4 LPR is
// a constant; otherwise d is any multiple of 4 up to 4 LPR and the lanes beyond the row carry zeros.
template <int LPR, bool FULL>
__global__ __launch_bounds__(256) void bpr_multi_v4_kernel(const float* __restrict__ U, const float* __restrict__ P,
                                                            const float* __restrict__ N, int64_t B, int K, int d_rt,
                                                            float inv, float* __restrict__ dU, float* __restrict__ dP,
                                                            float* __restrict__ dN, double* part) {
  constexpr int RPW = 64 / LPR;
  __builtin_assume(K >= 2);   // (K = 1 is the pair kernel) without it the first chunk's loads wait behind a K > 0 branch
  static_assert(LPR % KU == 0, "lane j of a row's group evaluates pair j of the chunk");
  const int d = FULL ? LPR * 4 : d_rt;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int sub = lane / LPR;
  const bool on = FULL || (lane % LPR) < d / 4;
  const int c4 = on ? lane % LPR : 0;
  const size_t kstride = (size_t)B * (d / 4);   // f32x4 units between the rows of negatives k and k + 1
  double acc = 0.0;
  for (int64_t b0 = ((int64_t)blockIdx.x * 4 + w) * RPW; b0 < B; b0 += (int64_t)gridDim.x * 4 * RPW) {
    const int64_t b = b0 + sub;
    const bool ok = b < B && on;
    const int64_t bc = b < B ? b : B - 1;
    f32x4 u = reinterpret_cast<const f32x4*>(U + bc * d)[c4];
    if (!on) u = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 p = reinterpret_cast<const f32x4*>(P + bc * d)[c4];
    const f32x4* nrow = reinterpret_cast<const f32x4*>(N + bc * d) + c4;
    f32x4* dnrow = reinterpret_cast<f32x4*>(dN + bc * d) + c4;
    // the rows of a chunk of KU negatives are requested a chunk ahead: the first chunk together with u and p (one
    // round trip to memory per sample, not two), chunk c + 1 before chunk c is consumed
    f32x4 nx[KU];
#pragma unroll
    for (int j = 0; j < KU; ++j) nx[j] = nrow[(size_t)(j < K ? j : K - 1) * kstride];
    float sp = (u.x * p.x + u.y * p.y) + (u.z * p.z + u.w * p.w);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) sp += __shfl_xor(sp, o, 64);
    f32x4 au = {0.f, 0.f, 0.f, 0.f};
    float gs = 0.f;
    for (int k0 = 0; k0 < K; k0 += KU) {
      f32x4 n[KU];
#pragma unroll
      for (int j = 0; j < KU; ++j) n[j] = nx[j];
      if (k0 + KU < K) {
#pragma unroll
        for (int j = 0; j < KU; ++j) {
          const int k = k0 + KU + j < K ? k0 + KU + j : K - 1;
          nx[j] = nrow[(size_t)k * kstride];
        }
      }
      float sn[KU];
#pragma unroll
      for (int j = 0; j < KU; ++j) {
        sn[j] = (u.x * n[j].x + u.y * n[j].y) + (u.z * n[j].z + u.w * n[j].w);
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) sn[j] += __shfl_xor(sn[j], o, 64);
      }
      // every lane of the row now holds all KU scores.  Lane j of the row's group evaluates pair j (the exponential,
      // the logarithm and the quotient once per chunk instead of once per pair: 0.191 -> 0.168 ps per byte at d = 64,
      // K = 4 on MI355X, nothing at d = 128) and the group reads g_j back from it.
      const int jsel = lane & (KU - 1);
      float zn = sn[0];
#pragma unroll
      for (int j = 1; j < KU; ++j) zn = jsel == j ? sn[j] : zn;
      float loss;
      const float g_own = multi_pair(sp - zn, inv, loss);
      if (b < B && lane % LPR < KU && k0 + jsel < K) acc += (double)loss;
#pragma unroll
      for (int j = 0; j < KU; ++j) {
        if (k0 + j < K) {   // uniform over the launch
          const float g = __shfl(g_own, (lane & ~(LPR - 1)) | j, 64);
          gs += g;
          au.x += g * (p.x - n[j].x); au.y += g * (p.y - n[j].y);
          au.z += g * (p.z - n[j].z); au.w += g * (p.w - n[j].w);
          if (ok) dnrow[(size_t)(k0 + j) * kstride] = f32x4{g * u.x, g * u.y, g * u.z, g * u.w};
        }
      }
    }
    if (ok) {
      reinterpret_cast<f32x4*>(dU + b * d)[c4] = f32x4{-au.x, -au.y, -au.z, -au.w};
      const float wp = -gs;
      reinterpret_cast<f32x4*>(dP + b * d)[c4] = f32x4{wp * u.x, wp * u.y, wp * u.z, wp * u.w};
    }
  }
  acc = wave_sum_d(acc);
  __shared__ double sh[4];
  if (lane == 0) sh[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// any d >= 1, any alignment: one wave per row.  The running sum of dU lives in dU itself (the lane that wrote an
// element is the lane that reads it back), so the additions are the same sequential float32 additions as above.
__global__ __launch_bounds__(256) void bpr_multi_kernel(const float* __restrict__ U, const float* __restrict__ P,
                                                        const float* __restrict__ N, int64_t B, int K, int d, float inv,
                                                        float* dU, float* __restrict__ dP, float* __restrict__ dN,
                                                        double* part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc = 0.0;
  for (int64_t b = (int64_t)blockIdx.x * 4 + w; b < B; b += (int64_t)gridDim.x * 4) {
    const float* ub = U + b * d;
    const float* pb = P + b * d;
    float* dub = dU + b * d;
    float sp = 0.f;
    for (int c = lane; c < d; c += 64) sp += ub[c] * pb[c];
    sp = wave_sum(sp);
    float gs = 0.f;
    for (int k = 0; k < K; ++k) {
      const float* nb = N + ((int64_t)k * B + b) * d;
      float* dnb = dN + ((int64_t)k * B + b) * d;
      float sn = 0.f;
      for (int c = lane; c < d; c += 64) sn += ub[c] * nb[c];
      sn = wave_sum(sn);
      float loss;
      const float g = multi_pair(sp - sn, inv, loss);
      gs += g;
      for (int c = lane; c < d; c += 64) {
        const float u = ub[c];
        const float prev = k == 0 ? 0.f : dub[c];          // minus the sum so far
        dub[c] = prev - g * (pb[c] - nb[c]);
        dnb[c] = g * u;
      }
      if (lane == 0) acc += (double)loss;
    }
    const float wp = -gs;
    for (int c = lane; c < d; c += 64) dP[b * d + c] = wp * ub[c];
  }
  __shared__ double sh[4];
  if (lane == 0) sh[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

}  // namespace

extern "C" int64_t rihip_bpr_multi_nparts(int64_t B, int K) {
  (void)K;   // one partial per workgroup, and the grid is the pair loss's at every K
  return rihip_bpr_pair_nparts(B);
}

extern "C" int rihip_bpr_multi_loss(const float* U, const float* P, const float* N, int64_t B, int K, int d, float* loss,
                                    float* dU, float* dP, float* dN, double* workspace, void* stream) {
  RIHIP_REQUIRE(U && P && N && dU && dP && dN && workspace, RIHIP_ERR_ARG, "bpr_multi_loss: null pointer");
  RIHIP_REQUIRE(B >= 1 && d >= 1 && K >= 1, RIHIP_ERR_ARG, "bpr_multi_loss: bad sizes B=%lld K=%d d=%d", (long long)B, K, d);
  RIHIP_REQUIRE(B <= (int64_t)0x7fffffff / (1 + (int64_t)K), RIHIP_ERR_ARG,
                "bpr_multi_loss: (1 + K) B rows exceed 2^31 - 1 (B=%lld K=%d)", (long long)B, K);
  if (K == 1) return rihip_bpr_pair_loss(U, P, N, B, d, loss, dU, dP, dN, workspace, stream);
  hipStream_t st = (hipStream_t)stream;
  const int grid = (int)rihip_bpr_multi_nparts(B, K);
  const bool al = ((reinterpret_cast<uintptr_t>(U) | reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(N) |
                    reinterpret_cast<uintptr_t>(dU) | reinterpret_cast<uintptr_t>(dP) | reinterpret_cast<uintptr_t>(dN)) & 15) == 0;
  const float inv = 1.f / (float)(B * K);
#define MULTI_V4(LPR, FULL) \
  hipLaunchKernelGGL((bpr_multi_v4_kernel<LPR, FULL>), dim3(grid), dim3(256), 0, st, U, P, N, B, K, d, inv, dU, dP, dN, workspace)
  const bool v4 = al && d % 4 == 0 && d <= 256;
  if (v4 && d == 128) MULTI_V4(32, true);
  else if (v4 && d == 64) MULTI_V4(16, true);
  else if (v4 && d == 32) MULTI_V4(8, true);
  else if (v4 && d < 32) MULTI_V4(8, false);
  else if (v4 && d < 128) MULTI_V4(32, false);
  else if (v4) MULTI_V4(64, false);
  else hipLaunchKernelGGL(bpr_multi_kernel, dim3(grid), dim3(256), 0, st, U, P, N, B, K, d, inv, dU, dP, dN, workspace);
#undef MULTI_V4
  RIHIP_CHECK_LAUNCH();
  // loss == NULL: the caller sums workspace[0 .. rihip_bpr_multi_nparts(B, K)) * 1/(B K) itself, as with the pair loss
  if (loss) return rihip_sum_partials(workspace, grid, 1.0 / ((double)B * (double)K), loss, stream);
  return RIHIP_OK;
}
