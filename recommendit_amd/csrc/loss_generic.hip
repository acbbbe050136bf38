// In-batch-negative BPR (TwoTowerModel.in_batch_bpr_loss, src/models/two_tower.py:132-160) for embedding widths without
// a tuned sweep instantiation: any multiple of 16 up to 256.  Same contract as inbatch_sweep_kernel (loss.hip), recompute
// form: mode user = owners are users, swept are items (loss, r, dU); mode item = owners are items, swept are users (dI).
//   S = O.Y^T ; z_ij = s_ij - pos ; g = sigma(z) ; dOwner = c (G.Y) (- r_i Y_i) ; loss = sum softplus(z)
// Skeleton: gen_sweep.h.
#include "common.h"
#include "gen_sweep.h"
#include "loss_sweep_args.h"

using namespace rihip_gen;

namespace {

static_assert(GOW == OW, "one workgroup fills one loss slot of the tuned layout (rihip_inbatch_loss_parts)");

struct GenSweep {
  SweepArgs a;
  int D;
};

template <bool MODE_USER>
__global__ __launch_bounds__(256) void inbatch_sweep_generic_kernel(GenSweep g) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const SweepArgs& a = g.a;
  const int D = g.D;
  const int ldo = gen_ldo(D);
  float* Os = smem;                    // [32][ldo] owners
  float* Gs = Os + 32 * ldo;           // [32][GLDG] weights of the current swept tile
  float* Wp = Gs + 32 * GLDG;          // [256][GLDP]
  float* red = Wp + 256 * GLDP;        // [4][32] per-wave row sums
  __shared__ double red_loss[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r31 = lane & 31;
  const int64_t gx128 = (a.No + GOW - 1) / GOW;
  if (blockIdx.y > 0) {                // the tuned layout reserves a loss slot per swept split: unused here
    if (MODE_USER && tid == 0) a.loss_part[(size_t)blockIdx.y * gx128 + blockIdx.x] = 0.0;
    return;
  }
  double loss_wg = 0.0;
  for (int og = 0; og < GOG; ++og) {
    const int64_t o_base = owner_base(og);
    if (o_base >= a.No) break;
    stage_owners(Os, ldo, a.Xo, o_base, a.No, D, tid);
    f32x16 out[GNT];
#pragma unroll
    for (int t = 0; t < GNT; ++t) out[t] = zero16();
    float racc[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) racc[r] = 0.f;
    float loss_acc = 0.f;
    for (int64_t sb = 0; sb < a.Ns; sb += GSW) {
      const int nsw = (a.Ns - sb < GSW) ? (int)(a.Ns - sb) : GSW;
      f32x16 sacc[GNT];
      wg_gemm<false>(Os, ldo, D, a.Ys + sb * D, D, nsw, Wp, sacc, tid);                // S = O.Y^T
      const TileLane tl = tile_lane(sb, w, r31, a.Ns, a.s_goff);
      const float pos_s = (!MODE_USER && tl.s_ok) ? a.pos[tl.srow] : 0.f;
      const float rd_s = (!MODE_USER && tl.s_ok) ? -a.r_in[tl.srow] / a.c : 0.f;   // weights are unscaled until the epilogue
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const TileElem e = tile_elem(r, lane, o_base, a.No, a.o_goff, tl);
        const float z = sacc[0][r] - (MODE_USER ? (e.orow < a.No ? a.pos[e.orow] : 0.f) : pos_s);
        float gv = 1.f / (1.f + __expf(-z));
        if (MODE_USER) {
          if (e.valid && !e.diag) {
            loss_acc += fmaxf(z, 0.f) + log1pf(__expf(-fabsf(z)));
            racc[r] += gv;
          } else gv = 0.f;
        } else {
          if (!e.valid) gv = 0.f;
          else if (e.diag) gv = rd_s;
        }
        Gs[e.ol * GLDG + w * 32 + r31] = gv;
      }
      wg_gemm<true, true>(Gs, GLDG, GSW, a.Ys + sb * D, D, D, Wp, out, tid, nsw);     // dOwner += G.Y
    }
    // ---- row sums of G per owner (user mode) and the loss of this owner group
    __syncthreads();
    if (MODE_USER) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = row32_sum(racc[r]);
        if (r31 == 0) red[w * 32 + acc_row(r, lane)] = v;
      }
      const float ls = wave_sum(loss_acc);
      if (lane == 0) red_loss[w] = (double)ls;
    }
    __syncthreads();
    if (MODE_USER) loss_wg += ((red_loss[0] + red_loss[1]) + red_loss[2]) + red_loss[3];
#pragma unroll
    for (int t = 0; t < GNT; ++t) {
      const int col = out_col(t, w, r31);
      if (col < D) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ol = acc_row(r, lane);
          const int64_t orow = o_base + ol;
          if (orow < a.No) {
            float v = out[t][r] * a.c;
            if (MODE_USER) {
              const float rs = red4_sum(red, ol) * a.c;
              const int64_t drow = a.o_goff + orow - a.s_goff;    // the owner's positive partner inside the swept set
              if (drow >= 0 && drow < a.Ns) v -= rs * a.Ys[drow * D + col];   // G_ii = -sum_{j != i} G_ij
              if (col == 0) a.r_out[orow] = rs;
            }
            a.dOwner[orow * D + col] = v;
          }
        }
      }
    }
  }
  if (MODE_USER && tid == 0) a.loss_part[blockIdx.x] = loss_wg;
}

}  // namespace

bool rihip_inbatch_generic_ok(int d) { return gen_width_ok(d); }

void rihip_launch_sweep_generic(int d, bool mode_user, const SweepArgs& a, int nsplit_slots, hipStream_t st) {
  GenSweep g;
  g.a = a; g.D = d;
  static bool granted = false;
  if (!granted) {
    (void)grant_dynamic_lds(reinterpret_cast<const void*>(inbatch_sweep_generic_kernel<true>), gen_sweep_lds(256));
    (void)grant_dynamic_lds(reinterpret_cast<const void*>(inbatch_sweep_generic_kernel<false>), gen_sweep_lds(256));
    granted = true;
  }
  const dim3 grid((unsigned)((a.No + GOW - 1) / GOW), (unsigned)(mode_user ? nsplit_slots : 1));
  if (mode_user) hipLaunchKernelGGL(inbatch_sweep_generic_kernel<true>, grid, dim3(256), gen_sweep_lds(d), st, g);
  else hipLaunchKernelGGL(inbatch_sweep_generic_kernel<false>, grid, dim3(256), gen_sweep_lds(d), st, g);
}
