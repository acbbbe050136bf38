// In-batch sampled softmax with temperature, logQ correction and accidental-hit masking (not in the reference, which
// trains with BPR only).  Runtime-width, exact-f32 MFMA, any embedding width that is a multiple of 16 up to 256.
//
// Contract.  A row's global index is its offset argument plus its local index.  User i (global gu = user_goff + i) has
// the item of global index gu as its positive partner.
//   logit    l_ij = inv_temp <u_i, y_j> - logq_j           logq: nullable, aligned with the items; applies to the diagonal too
//   mask     pair (i, j) is dropped iff id arrays are given, j is not i's partner and item_ids[j] == user_pos_ids[i]
//            (user_pos_ids[i] = id of i's positive; both int64, nullable together); the diagonal is never masked
//   softmax  lse_i = log sum_{j unmasked} exp(l_ij) ;  p_ij = exp(l_ij - lse_i), 0 where masked
//   loss     (1/n_global) sum_i (lse_i - l_ii)
//   dU_i = (inv_temp/n_global) (sum_j p_ij y_j - y_partner)      dI_j = (inv_temp/n_global) (sum_i p_ij u_i - u_partner)
// User mode (owners = users, swept = items) writes dU, lse[n_users] and one double loss partial per 128 users (summed by
// rihip_sum_partials with scale 1/n_global); every user's partner must lie inside the swept items (the entry checks it).
// Item mode (owners = items, swept = users) reads lse and user_pos_ids of the swept users, logq and item_ids of its
// owners, and writes dI; an item whose partner user lies outside the swept users gets no -u_partner term, so dI is
// additive over slices of the users.
//
// Form: flash-style, 8 No Ns d FLOP for the pair.  The user sweep keeps a running row maximum m and row sum per owner,
// rescales the row sums and the dOwner accumulators by exp(m_old - m_new) whenever a tile raises the maximum (the
// decision is taken before the tile's weights are exponentiated, so nothing is ever at a mixed scale), and finishes
// dU, lse and the loss in the same launch.  The item sweep recomputes the scores and exponentiates against the stored
// lse.  Every exponent is <= 0 in user mode whatever the logits are: no fixed shift, no assumption of unit rows.
// Skeleton: gen_sweep.h.
#include <cmath>

#include "common.h"
#include "gen_sweep.h"

using namespace rihip_gen;

namespace {

struct SoftmaxArgs {
  const float* Xo;           // owners [No,d]
  int64_t No, o_goff;
  const float* Ys;           // swept [Ns,d]
  int64_t Ns, s_goff;
  int D;
  float inv_temp;
  float c;                   // inv_temp / n_global
  const float* logq;         // user mode: [Ns] by swept item ; item mode: [No] by owner item ; nullable
  const int64_t* o_ids;      // user mode: user_pos_ids [No] ; item mode: item_ids [No] ; nullable together with s_ids
  const int64_t* s_ids;      // user mode: item_ids [Ns]     ; item mode: user_pos_ids [Ns]
  float* dOwner;             // [No,d]
  float* lse;                // user mode: out [No] ; item mode: in [Ns]
  double* loss_part;         // user mode: [gridDim.x]
};

template <bool MODE_USER>
__global__ __launch_bounds__(256) void inbatch_softmax_kernel(SoftmaxArgs a) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int D = a.D;
  const int ldo = gen_ldo(D);
  float* Os = smem;                    // [32][ldo] owners
  float* Gs = Os + 32 * ldo;           // [32][GLDG] weights of the current swept tile
  float* Wp = Gs + 32 * GLDG;          // [256][GLDP]
  float* red = Wp + 256 * GLDP;        // [4][32] per-wave row maxima of a tile, then the per-wave row sums
  __shared__ float own_lq[32];         // item mode: logq of the 32 owners
  __shared__ int64_t own_id[32];       // ids of the 32 owners
  __shared__ float diag_l[32];         // user mode: l_ii, written by the one lane that meets the diagonal
  __shared__ float row_loss[32];       // user mode: lse_i - l_ii
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r31 = lane & 31;
  const bool ids = a.o_ids != nullptr;
  const float NEG_INF = -INFINITY;
  double loss_wg = 0.0;
  for (int og = 0; og < GOG; ++og) {
    const int64_t o_base = owner_base(og);
    if (o_base >= a.No) break;
    stage_owners(Os, ldo, a.Xo, o_base, a.No, D, tid);
    if (tid < 32) {
      const bool ok = o_base + tid < a.No;
      own_id[tid] = (ids && ok) ? a.o_ids[o_base + tid] : 0;
      own_lq[tid] = (!MODE_USER && a.logq && ok) ? a.logq[o_base + tid] : 0.f;
    }
    f32x16 out[GNT];
#pragma unroll
    for (int t = 0; t < GNT; ++t) out[t] = zero16();
    float m_run[16], l_run[16];        // user mode: running maximum and this lane's share of the running row sum
#pragma unroll
    for (int r = 0; r < 16; ++r) { m_run[r] = NEG_INF; l_run[r] = 0.f; }
    for (int64_t sb = 0; sb < a.Ns; sb += GSW) {
      const int nsw = (a.Ns - sb < GSW) ? (int)(a.Ns - sb) : GSW;
      f32x16 sacc[GNT];
      wg_gemm<false>(Os, ldo, D, a.Ys + sb * D, D, nsw, Wp, sacc, tid);                // S = O.Y^T
      const TileLane tl = tile_lane(sb, w, r31, a.Ns, a.s_goff);
      const int64_t id_s = swept_id(ids, a.s_ids, tl);
      if (MODE_USER) {
        const float lq_s = (a.logq && tl.s_ok) ? a.logq[tl.srow] : 0.f;
        float lg[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const TileElem e = tile_elem(r, lane, o_base, a.No, a.o_goff, tl);
          const float l = a.inv_temp * sacc[0][r] - lq_s;
          lg[r] = (e.valid && !masked(ids, e.diag, id_s, own_id[e.ol])) ? l : NEG_INF;
          if (e.valid && e.diag) diag_l[e.ol] = l;
          const float v = row32_max(lg[r]);
          if (r31 == 0) red[w * 32 + e.ol] = v;
        }
        __syncthreads();
        // the new maximum is settled BEFORE anything of this tile is exponentiated: accumulators and row sums move to
        // it by one factor, the tile's weights are formed against it
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ol = acc_row(r, lane);
          const float mt = red4_max(red, ol);
          const float mn = fmaxf(m_run[r], mt);
          const float alpha = (m_run[r] == NEG_INF) ? 0.f : __expf(m_run[r] - mn);   // nothing accumulated yet: any factor
          const float p = (lg[r] == NEG_INF) ? 0.f : __expf(lg[r] - mn);            // masked / out of range: exactly 0
          l_run[r] = l_run[r] * alpha + p;
          m_run[r] = mn;
#pragma unroll
          for (int t = 0; t < GNT; ++t) out[t][r] *= alpha;
          Gs[ol * GLDG + w * 32 + r31] = p;
        }
      } else {
        const float lse_s = tl.s_ok ? a.lse[tl.srow] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const TileElem e = tile_elem(r, lane, o_base, a.No, a.o_goff, tl);
          const float l = a.inv_temp * sacc[0][r] - own_lq[e.ol];
          float p = (e.valid && !masked(ids, e.diag, id_s, own_id[e.ol])) ? __expf(l - lse_s) : 0.f;
          if (e.valid && e.diag) p -= 1.f;       // the partner user is in this tile: its -u term rides in the product
          Gs[e.ol * GLDG + w * 32 + r31] = p;
        }
      }
      wg_gemm<true, true>(Gs, GLDG, GSW, a.Ys + sb * D, D, D, Wp, out, tid, nsw);     // dOwner += G.Y
    }
    // ---- epilogue of the owner group
    __syncthreads();
    if (MODE_USER) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = row32_sum(l_run[r]);
        if (r31 == 0) red[w * 32 + acc_row(r, lane)] = v;
      }
      __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ol = acc_row(r, lane);
      const int64_t orow = o_base + ol;
      float inv_sum = 1.f;
      if (MODE_USER) {
        const float sum = red4_sum(red, ol);   // >= 1: the maximum's own term
        inv_sum = 1.f / sum;
        if (w == 0 && r31 == 0) {
          float rl = 0.f;
          if (orow < a.No) {
            const float lse = m_run[r] + logf(sum);
            a.lse[orow] = lse;
            rl = lse - diag_l[ol];
          }
          row_loss[ol] = rl;
        }
      }
#pragma unroll
      for (int t = 0; t < GNT; ++t) {
        const int col = out_col(t, w, r31);
        if (col < D && orow < a.No) {
          float v = out[t][r];
          if (MODE_USER) {
            const int64_t drow = a.o_goff + orow - a.s_goff;   // inside [0, Ns): checked by the entry
            v = v * inv_sum - a.Ys[drow * D + col];
          }
          a.dOwner[orow * D + col] = v * a.c;
        }
      }
    }
    if (MODE_USER) {
      __syncthreads();
      if (tid == 0) {
        double s = 0.0;
        for (int r = 0; r < 32; ++r) s += (double)row_loss[r];
        loss_wg += s;
      }
    }
  }
  if (MODE_USER && tid == 0) a.loss_part[blockIdx.x] = loss_wg;
}

int launch(bool mode_user, const SoftmaxArgs& a, hipStream_t st) {
  static bool granted = false;
  if (!granted) {
    RIHIP_CHECK_HIP(grant_dynamic_lds(reinterpret_cast<const void*>(inbatch_softmax_kernel<true>), gen_sweep_lds(256)));
    RIHIP_CHECK_HIP(grant_dynamic_lds(reinterpret_cast<const void*>(inbatch_softmax_kernel<false>), gen_sweep_lds(256)));
    granted = true;
  }
  const dim3 grid((unsigned)((a.No + GOW - 1) / GOW));
  if (mode_user) hipLaunchKernelGGL(inbatch_softmax_kernel<true>, grid, dim3(256), gen_sweep_lds(a.D), st, a);
  else hipLaunchKernelGGL(inbatch_softmax_kernel<false>, grid, dim3(256), gen_sweep_lds(a.D), st, a);
  RIHIP_CHECK_LAUNCH();
  return RIHIP_OK;
}

int check_common(const char* who, int d, float inv_temp, const int64_t* user_pos_ids, const int64_t* item_ids,
                 int64_t n_users, int64_t n_items, int64_t n_global) {
  RIHIP_REQUIRE(gen_width_ok(d), RIHIP_ERR_SHAPE, "%s: unsupported embed_dim=%d (multiples of 16 up to 256)", who, d);
  RIHIP_REQUIRE(std::isfinite(inv_temp) && inv_temp > 0.f, RIHIP_ERR_ARG, "%s: inv_temp=%g must be finite and > 0", who,
                (double)inv_temp);
  RIHIP_REQUIRE((user_pos_ids == nullptr) == (item_ids == nullptr), RIHIP_ERR_ARG,
                "%s: user_pos_ids and item_ids must be given together or both be null", who);
  RIHIP_REQUIRE(n_users > 0 && n_items > 0 && n_global >= 1, RIHIP_ERR_ARG, "%s: sizes users=%lld items=%lld B=%lld", who,
                (long long)n_users, (long long)n_items, (long long)n_global);
  return RIHIP_OK;
}

}  // namespace

extern "C" int64_t rihip_inbatch_softmax_loss_parts(int64_t n_users) { return (n_users + GOW - 1) / GOW; }

extern "C" int rihip_inbatch_softmax_user_sweep(const float* users, int64_t n_users, int64_t user_goff,
                                                const float* items, int64_t n_items, int64_t item_goff, int d,
                                                float inv_temp, const float* logq, const int64_t* user_pos_ids,
                                                const int64_t* item_ids, int64_t n_global, float* d_users, float* lse,
                                                double* loss_part, void* stream) {
  const int rc = check_common("inbatch_softmax_user_sweep", d, inv_temp, user_pos_ids, item_ids, n_users, n_items, n_global);
  if (rc != RIHIP_OK) return rc;
  RIHIP_REQUIRE(users && items && d_users && lse && loss_part, RIHIP_ERR_ARG, "inbatch_softmax_user_sweep: null pointer");
  RIHIP_REQUIRE(user_goff >= item_goff && user_goff + n_users <= item_goff + n_items, RIHIP_ERR_ARG,
                "inbatch_softmax_user_sweep: users [%lld, %lld) have partners outside the swept items [%lld, %lld) "
                "(a log-sum-exp over a slice of the items is meaningless)", (long long)user_goff,
                (long long)(user_goff + n_users), (long long)item_goff, (long long)(item_goff + n_items));
  SoftmaxArgs a;
  a.Xo = users; a.No = n_users; a.o_goff = user_goff; a.Ys = items; a.Ns = n_items; a.s_goff = item_goff; a.D = d;
  a.inv_temp = inv_temp; a.c = (float)((double)inv_temp / (double)n_global);
  a.logq = logq; a.o_ids = user_pos_ids; a.s_ids = item_ids;
  a.dOwner = d_users; a.lse = lse; a.loss_part = loss_part;
  return launch(true, a, (hipStream_t)stream);
}

extern "C" int rihip_inbatch_softmax_item_sweep(const float* items, int64_t n_items, int64_t item_goff,
                                                const float* users, int64_t n_users, int64_t user_goff, int d,
                                                float inv_temp, const float* logq, const int64_t* item_ids,
                                                const int64_t* user_pos_ids, const float* lse, int64_t n_global,
                                                float* d_items, void* stream) {
  const int rc = check_common("inbatch_softmax_item_sweep", d, inv_temp, user_pos_ids, item_ids, n_users, n_items, n_global);
  if (rc != RIHIP_OK) return rc;
  RIHIP_REQUIRE(items && users && lse && d_items, RIHIP_ERR_ARG, "inbatch_softmax_item_sweep: null pointer");
  SoftmaxArgs a;
  a.Xo = items; a.No = n_items; a.o_goff = item_goff; a.Ys = users; a.Ns = n_users; a.s_goff = user_goff; a.D = d;
  a.inv_temp = inv_temp; a.c = (float)((double)inv_temp / (double)n_global);
  a.logq = logq; a.o_ids = item_ids; a.s_ids = user_pos_ids;
  a.dOwner = d_items; a.lse = const_cast<float*>(lse); a.loss_part = nullptr;
  return launch(false, a, (hipStream_t)stream);
}
