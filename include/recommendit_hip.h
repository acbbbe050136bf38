/* recommendit_hip.h -- C ABI of librecommendit_hip.so (gfx950 / MI355X).
 *
 * The reference (sarihammad/recommendit) has no FFI of its own: its seam is three Python
 * classes (src/models/__init__.py:1-3).  Each entry point below names the reference code
 * whose *body* it replaces (paths relative to the reference root); the Python classes in
 * recommendit_amd/ keep the reference's class surface and call these through ctypes.
 * INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 (RIHIP_OK) or a non-zero status; rihip_last_error() gives the
 *     message (thread-local).  Nothing aborts the process: the callers' fallbacks
 *     (src/serving/recommender.py:202-207, src/serving/app.py:182-185) must keep working.
 *   - all array pointers are DEVICE pointers unless a comment says host; the caller allocates
 *     inputs, outputs and workspaces; the library never frees caller memory and never keeps a
 *     caller pointer after returning.  Opaque handles (ip_index, gbdt) own their device memory
 *     and are destroyed by their paired *_destroy.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are
 *     asynchronous on that stream except where documented.
 *   - float = IEEE binary32, ids/rows = int64_t.
 */
#ifndef RECOMMENDIT_HIP_H
#define RECOMMENDIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RIHIP_ABI_VERSION 1

int rihip_abi_version(void);
/* "gfx950": the only ISA this library carries code objects for */
const char* rihip_target_arch(void);
/* last error message of the calling thread ("" if none) */
const char* rihip_last_error(void);
/* Generation of the library state a captured hipGraph can have baked in: handle-owned scratch buffers of the index and
 * the forest (grown on demand: the old allocation is freed), nprobe, the id map, the index / forest content.  Bumped on
 * every such change, library-wide.  A caller that replays a captured chain (GpuRecommendationPipeline, the batched form
 * of recommender.py:269-387) records the value after capture and re-captures when it differs. */
uint64_t rihip_scratch_generation(void);
/* name of device 0's ISA as reported by the runtime (host buffer); needs a GPU */
int rihip_device_arch(char* buf, int buf_len);

/* ---- Two-Tower towers ----------------------------------------------------------------------
 * rihip_tower_forward replaces UserTower.forward (src/models/two_tower.py:39-42; genres==NULL)
 * and ItemTower.forward (:68-72; genres = [B,18] multi-hot):
 *   x = table[ids] (|| genres) ; h = dropout(relu(x W1^T + b1)) ; y = h W2^T + b2 ;
 *   out = y / max(|y|_2, 1e-12).
 * table [n_rows,d]; W1 [hidden, d(+18)]; b1 [hidden]; W2 [d,hidden]; b2 [d]  (nn.Linear layout).
 * training!=0 && dropout_p>0: keep-mask from the counter-based generator keyed by
 * (seed, (row0+row)*hidden+col) -- see oracle/two_tower_np.py:dropout_keep_mask.
 * hid [B,hidden] (post-dropout activations) and denom [B] are saved for backward (nullable).
 * err_flag (device int, nullable) is set to 1 if an id is outside [0,n_rows) (row 0 is used).
 * workspace (nullable): rihip_tower_forward_workspace_floats(d, hidden, item) floats, 16-B aligned; holds the
 * MFMA-fragment-major copy of W1/W2 rebuilt each call (coalesced weight loads).
 * seed_step_dev (nullable): device int64 mixed into the dropout seed, so a captured hipGraph draws a fresh
 * mask on every replay (the counter is advanced by rihip_adam_hyper_step).
 * Shapes: the reference takes any (embed_dim, hidden_dim) (two_tower.py:80-95).  rihip_tower_shape_ok(d, hidden) = 1 for
 * every pair of multiples of 16 up to 256; rihip_tower_supported(d, hidden) = 1 for the pairs with tuned template
 * instantiations (the fast path) -- every other pair runs the runtime-shape kernels of csrc/tower_generic.hip. */
int rihip_tower_supported(int d, int hidden);
int rihip_tower_shape_ok(int d, int hidden);
int64_t rihip_tower_forward_workspace_floats(int d, int hidden, int item);
int rihip_tower_forward(const float* table, int64_t n_rows, const int64_t* ids, const float* genres, int64_t B,
                        int d, int hidden, const float* W1, const float* b1, const float* W2, const float* b2,
                        int training, float dropout_p, uint64_t seed, int64_t row0, float* out, float* hid,
                        float* denom, int* err_flag, float* workspace, const int64_t* seed_step_dev, void* stream);

/* Backward of the above (autograd of two_tower.py:39-42/:68-72, run by
 * src/training/train_embeddings.py:190).  grad_out = dL/d out [B,d].
 * Outputs: dX [B,d] per-sample embedding-row gradients (scatter them with
 * rihip_embedding_scatter_add or the row-sparse path); dW1/db1/dW2/db2 in nn.Linear layout,
 * overwritten (accumulate=0) or added to (accumulate=1).  dropout_scale = 1/(1-p) if the
 * forward ran in training mode with p>0, else 1.  workspace: floats, size from
 * rihip_tower_backward_workspace_floats. */
int64_t rihip_tower_backward_workspace_floats(int64_t B, int d, int hidden, int item);
int rihip_tower_backward(const float* table, int64_t n_rows, const int64_t* ids, const float* genres, int64_t B,
                         int d, int hidden, const float* W1, const float* W2, const float* grad_out,
                         const float* out, const float* denom, const float* hid, float dropout_scale, float* dX,
                         float* dW1, float* db1, float* dW2, float* db2, int accumulate, float* workspace,
                         void* stream);
/* Same, plus dx_event (a hipEvent_t, nullable): recorded on `stream` as soon as dX is complete -- before the
 * weight-gradient kernels -- so a caller can start the embedding-row gradient reduction on another stream beside them. */
int rihip_tower_backward_ev(const float* table, int64_t n_rows, const int64_t* ids, const float* genres, int64_t B,
                            int d, int hidden, const float* W1, const float* W2, const float* grad_out,
                            const float* out, const float* denom, const float* hid, float dropout_scale, float* dX,
                            float* dW1, float* db1, float* dW2, float* db2, int accumulate, float* workspace,
                            void* stream, void* dx_event);
/* The backward in two halves, for a step with two towers: _partial launches the gradient kernels only (dX complete,
 * weight-gradient slabs left in `workspace`, their count in *n_slabs); _reduce2 then sums the slabs of BOTH towers
 * (b may be absent: ws_b = NULL) in one pair of launches -- the same sums in the same order as rihip_tower_backward,
 * so the results are bit-identical.  The two towers need separate workspaces. */
int rihip_tower_backward_partial(const float* table, int64_t n_rows, const int64_t* ids, const float* genres, int64_t B,
                                 int d, int hidden, const float* W1, const float* W2, const float* grad_out,
                                 const float* out, const float* denom, const float* hid, float dropout_scale,
                                 float* dX, float* workspace, void* stream, void* dx_event, int* n_slabs);
int rihip_tower_backward_reduce2(int d, int hidden, float* ws_a, int64_t B_a, int item_a, int n_slabs_a, float* dW1_a,
                                 float* db1_a, float* dW2_a, float* db2_a, float* ws_b, int64_t B_b, int item_b,
                                 int n_slabs_b, float* dW1_b, float* db1_b, float* dW2_b, float* db2_b, int accumulate,
                                 void* stream);

/* Both towers of one training step in one launch each way (a step of batch 256 is bounded by its ~10 dependent
 * launches).  rihip_tower_io carries what differs per tower in rihip_tower_forward / rihip_tower_backward_partial;
 * user->genres must be NULL and item->genres non-NULL.  Batches that take the chip-filling kernels (>= 49 152 rows)
 * or arguments the pair kernels do not cover fall back to the two single calls -- the results are bit-identical either
 * way.  The two towers need separate workspaces. */
typedef struct rihip_tower_io {
  const float* table; int64_t n_rows; const int64_t* ids; const float* genres; int64_t B;
  const float *W1, *b1, *W2, *b2;
  uint64_t seed; int64_t row0;
  float *out, *hid, *denom;          /* forward outputs = backward inputs */
  float* fwd_workspace;              /* rihip_tower_forward_workspace_floats, nullable */
  const float* grad_out; float* dX;  /* backward */
  float* bwd_workspace;              /* rihip_tower_backward_workspace_floats */
} rihip_tower_io;
int rihip_tower_forward_pair(const rihip_tower_io* user, const rihip_tower_io* item, int d, int hidden, int training,
                             float dropout_p, int* err_flag, const int64_t* seed_step_dev, void* stream);
int rihip_tower_backward_partial_pair(const rihip_tower_io* user, const rihip_tower_io* item, int d, int hidden,
                                      float dropout_scale, void* stream, void* dx_event_user, void* dx_event_item,
                                      int* n_slabs_user, int* n_slabs_item);

/* The whole sampled-negative training step with the reference's optimiser (towers -> bpr_loss -> backward ->
 * clip_grad_norm_ -> dense Adam + coupled L2 on the MLPs and BOTH tables: src/training/train_embeddings.py:178-195,
 * :160-161) in ONE launch: a persistent grid walks the step behind three grid barriers (csrc/step_persistent.hip).  For
 * the batch sizes the reference trains at (BATCH_SIZE = 1024, src/config.py:25; B <= 2048 here) a step is otherwise
 * seven dependent launches.  Any (embed_dim, hidden_dim) of rihip_tower_shape_ok.  item.B = 2*user.B (pos || neg).
 * grad_out / dX / out / hid / denom of both rihip_tower_io are scratch the step fills; bwd_workspace needs B*(d+hidden)
 * floats.  dW1_u ... db2_i: the MLP gradient tensors (views of flat_g).  *_tab_g: dense table gradients, zero on entry and
 * left zero.  step_dev / lr_dev / hyper_dev / coef / gnorm / loss as in rihip_clip_coef_step (the clock is advanced).
 * barrier: 4 zero-initialised words owned by the caller for the life of the trainer.  Error bit 8 of *err_flag: the grid
 * was not co-resident (another kernel held CUs) and the step was abandoned; bit 1: an id outside its table. */
typedef struct rihip_step_args {
  rihip_tower_io user, item;
  float *dW1_u, *db1_u, *dW2_u, *db2_u, *dW1_i, *db1_i, *dW2_i, *db2_i;
  float *flat_p, *flat_g, *flat_m, *flat_v; int64_t n_flat;
  float *utab_g, *utab_m, *utab_v, *itab_g, *itab_m, *itab_v;
  int d, hidden, training; float dropout_p;
  float beta1, beta2, eps, weight_decay, max_norm;
  const float* lr_dev; int64_t* step_dev; float* hyper_dev; float* coef; float* gnorm; float* loss; int* err_flag;
  double* scratch_doubles; int64_t n_scratch_doubles;   /* >= rihip_bpr_step_scratch_doubles(B) */
  unsigned* barrier;
} rihip_step_args;
int rihip_bpr_step_persistent_supported(int64_t B, int d, int hidden);
int64_t rihip_bpr_step_scratch_doubles(int64_t B);
int rihip_bpr_step_persistent(const rihip_step_args* a, void* stream);

/* nn.Embedding backward (dense): grad_table[ids[b]] += dX[b]; row 0 (padding_idx, two_tower.py:27,54) and ids outside
 * [1, n_rows) are skipped.  Bitwise reproducible: every row receives its samples one after the other in batch order,
 * starting from its current contents (the float32 chain of index_add_ on a CPU) -- no floating-point atomics.
 * _add2 handles two tables (user + item) in one launch. */
int rihip_embedding_scatter_add(float* grad_table, int64_t n_rows, const int64_t* ids, const float* dX, int64_t B,
                                int d, void* stream);
int rihip_embedding_scatter_add2(float* grad_a, int64_t n_rows_a, const int64_t* ids_a, const float* dX_a, int64_t B_a,
                                 float* grad_b, int64_t n_rows_b, const int64_t* ids_b, const float* dX_b,
                                 int64_t B_b, int d, void* stream);
/* rihip_tower_backward_reduce2 and rihip_embedding_scatter_add2 together: both wait only for the tower backward, so
 * the scatter launch carries one slab-reduction level in extra workgroups (a dense small-batch step saves a dependent
 * launch).  Results are bit-identical to the two separate calls.  Bs_* = samples scattered into each table. */
int rihip_backward_reduce2_scatter2(int d, int hidden, float* ws_a, int64_t B_a, int item_a, int n_slabs_a, float* dW1_a,
                                    float* db1_a, float* dW2_a, float* db2_a, float* ws_b, int64_t B_b, int item_b,
                                    int n_slabs_b, float* dW1_b, float* db1_b, float* dW2_b, float* db2_b, int accumulate,
                                    float* grad_a, int64_t n_rows_a, const int64_t* ids_a, const float* dX_a, int64_t Bs_a,
                                    float* grad_b, int64_t n_rows_b, const int64_t* ids_b, const float* dX_b, int64_t Bs_b,
                                    void* stream);

/* ---- losses --------------------------------------------------------------------------------
 * rihip_bpr_pair_loss replaces TwoTowerModel.bpr_loss (two_tower.py:117-130) and its backward:
 * loss = mean softplus(-(u.p - u.n)); dU,dP,dN = d loss / d inputs.  workspace: >=1024 doubles.
 * loss may be NULL: the value is then (1/B) * sum(workspace[0 .. rihip_bpr_pair_nparts(B))), summed later by the
 * caller (rihip_sum_partials / rihip_clip_coef_step). */
int rihip_bpr_pair_loss(const float* U, const float* P, const float* N, int64_t B, int d, float* loss, float* dU,
                        float* dP, float* dN, double* workspace, void* stream);
int64_t rihip_bpr_pair_nparts(int64_t B);

/* rihip_bpr_multi_loss (not in the reference): sampled-negative BPR with K negatives per positive.
 *   z_ik = u_i.p_i - u_i.n_ik      L = 1/(B K) sum_i sum_k softplus(-z_ik)      g_ik = sigma(-z_ik) / (B K)
 *   dN_ik = g_ik u_i               dP_i = -(sum_k g_ik) u_i                     dU_i = -sum_k g_ik (p_i - n_ik)
 * U, P, dU, dP: [B, d].  N, dN: [K, B, d], k-major: negative k of sample i is row k B + i, so K = 1 is the pos || neg
 * layout of rihip_bpr_pair_loss.  The loss is the MEAN over the B K pairs, not a sum over k: the loss scale and the
 * gradient norm that the clip sees then mean the same thing at every K.  The K negatives of a sample are independent
 * terms (a repeated negative counts twice).  The outputs must not overlap the inputs or each other.
 * Operation order (float32 throughout, a product may be fused into the addition that consumes it):
 *   u_i.x is a sum of d products in a fixed tree: with 16-byte accesses (d a multiple of 4 up to 256, all six pointers
 *     16-byte aligned; tuned for d = 32 / 64 / 128) each lane forms (x0 y0 + x1 y1) + (x2 y2 + x3 y3) of its four
 *     columns and the lanes of a row are combined by a butterfly; otherwise (any d >= 1, any alignment) lane l adds the
 *     products of columns l, l + 64, ... in order and the 64 lanes are combined by a butterfly.  Either way the result
 *     is within d u S of the exact dot product (u = 2^-24, S = the sum of the absolute products).
 *   z_ik = fl(u_i.p_i - u_i.n_ik): u_i.p_i is formed once per sample, one rounding on the difference.
 *   e = expf(-|z|); softplus(-z) = max(-z, 0) + log1pf(e); sigma(-z) = e / (1 + e) for z >= 0, 1 / (1 + e) for z < 0.
 *   g_ik = sigma(-z_ik) * inv, inv = 1.0f / (float)(B K).
 *   k runs ascending.  dN_ik = g_ik * u_i.  The sums over k are sequential float32 additions from 0:
 *     s_k = s_(k-1) + g_ik,  a_k = a_(k-1) + g_ik * (p_i - n_ik) per column;  dP_i = (-s_K) * u_i,  dU_i = -a_K.
 *   Loss: every softplus value is added, as a double, into one partial per workgroup in a fixed order.
 * workspace: >= 1024 doubles; it receives rihip_bpr_multi_nparts(B, K) partials.  loss may be NULL: the value is then
 * 1/(B K) * sum(workspace[0 .. nparts)), summed later by the caller (rihip_sum_partials / rihip_clip_coef_step), exactly
 * as with the pair loss.  No float atomics: two calls are bitwise equal.  K = 1 IS rihip_bpr_pair_loss (same launches,
 * same bits).  RIHIP_ERR_ARG: a null pointer (loss excepted), B < 1, d < 1, K < 1, (1 + K) B > 2^31 - 1. */
int rihip_bpr_multi_loss(const float* U, const float* P, const float* N, int64_t B, int K, int d, float* loss, float* dU,
                         float* dP, float* dN, double* workspace, void* stream);
int64_t rihip_bpr_multi_nparts(int64_t B, int K);

/* In-batch-negative BPR (TwoTowerModel.in_batch_bpr_loss, two_tower.py:132-160, closed form
 *   L = 1/(B(B-1)) sum_i sum_{j!=i} softplus(s_ij - s_ii)) is three calls:
 *   rihip_rowdot        pos[i] = U[i].I[i+i_offset]
 *   rihip_inbatch_sweep mode_user=1: owners=users, swept=items -> d_owner=dU, r_out, loss_part
 *   rihip_inbatch_sweep mode_user=0: owners=items, swept=users (+pos, r_in=r) -> d_owner=dI
 *   rihip_sum_partials  loss = scale * sum(loss_part[0 .. rihip_inbatch_loss_parts))  with scale = 1/(B(B-1))
 * workspace: floats, rihip_inbatch_workspace_floats(n_owner, n_swept, d) (slabs of the swept-range splits that
 * keep small batches chip-filling; combined in fixed order => bitwise reproducible).
 * precision: 0 = exact-f32 MFMA (v_mfma_f32_32x32x2_f32, an fmaf chain); 2 = "bf16x6": every fp32 operand split
 * EXACTLY into three bf16 pieces (8+8+8 bits), six of the nine partial products on bf16 MFMA with f32 accumulation
 * (dropped terms <= 2^-23 |a||b|: fp32-level accuracy, same test tolerances as precision 0, ~2.5x faster);
 * 1 = "bf16x3": two pieces, products hi.hi+hi.lo+lo.hi (relative product error ~2^-16).  The stored-G passes take
 * precision 0 or 2.
 * Global indices (owner_goff / swept_goff) place a rank's local rows inside the all-gathered
 * batch for multi-GPU in-batch negatives; n_global = B.  d in {32,64,128}. */
int rihip_rowdot(const float* U, const float* I, int64_t B, int64_t i_offset, int d, float* pos, void* stream);
int64_t rihip_inbatch_workspace_doubles(int64_t n_owner);
int64_t rihip_inbatch_loss_parts(int64_t n_owner, int64_t n_swept);
int64_t rihip_inbatch_workspace_floats(int64_t n_owner, int64_t n_swept, int d);
int rihip_inbatch_sweep(int mode_user, const float* owners, int64_t n_owner, int64_t owner_goff, const float* swept,
                        int64_t n_swept, int64_t swept_goff, int d, const float* pos, const float* r_in,
                        int64_t n_global, float* d_owner, float* r_out, double* loss_part, float* workspace,
                        int precision, void* stream);
int rihip_sum_partials(const double* part, int64_t n, double scale, float* out, void* stream);

/* In-batch sampled softmax with temperature, logQ correction and accidental-hit masking (not in the reference).
 * A row's global index is its offset argument plus its local index; user i (global gu = user_goff + i) has the item of
 * global index gu as its positive partner.
 *   logit    l_ij = inv_temp <u_i, y_j> - logq_j    logq: nullable float[n_items] (NULL = 0); applies to the diagonal too
 *   mask     pair (i, j) is dropped iff the id arrays are given, j is not i's partner and item_ids[j] == user_pos_ids[i]
 *            (user_pos_ids[i] = id of i's positive; both int64, NULL together); the diagonal is never masked
 *   softmax  lse_i = log sum_{j unmasked} exp(l_ij);  p_ij = exp(l_ij - lse_i), 0 where masked
 *   loss     (1/n_global) sum_i (lse_i - l_ii)
 *   d_users[i] = (inv_temp/n_global) (sum_j p_ij y_j - y_partner)
 *   d_items[j] = (inv_temp/n_global) (sum_i p_ij u_i - u_partner)
 * Finite and accurate for any finite logits (a running row maximum is subtracted; nothing relies on unit rows).
 * rihip_inbatch_softmax_user_sweep: owners = users, swept = items.  Writes d_users, lse[n_users] and
 *   rihip_inbatch_softmax_loss_parts(n_users) doubles to loss_part (loss = rihip_sum_partials with scale 1/n_global).
 *   Every user's partner must lie inside the swept items (item_goff <= user_goff and user_goff + n_users <=
 *   item_goff + n_items), else RIHIP_ERR_ARG: a log-sum-exp over a slice of the items is meaningless.
 * rihip_inbatch_softmax_item_sweep: owners = items, swept = users.  Reads lse[n_users] and user_pos_ids[n_users] of the
 *   swept users, logq[n_items] and item_ids[n_items] of its owners; writes d_items.  An item whose partner user lies
 *   outside the swept users gets no -u_partner term, so d_items is additive over slices of the users.
 * d: any multiple of 16 up to 256 (exact-f32 MFMA).  inv_temp finite and > 0.  One launch each, no atomics, no host
 * synchronisation: bitwise reproducible and capturable in a graph. */
int64_t rihip_inbatch_softmax_loss_parts(int64_t n_users);
int rihip_inbatch_softmax_user_sweep(const float* users, int64_t n_users, int64_t user_goff, const float* items,
                                     int64_t n_items, int64_t item_goff, int d, float inv_temp, const float* logq,
                                     const int64_t* user_pos_ids, const int64_t* item_ids, int64_t n_global,
                                     float* d_users, float* lse, double* loss_part, void* stream);
int rihip_inbatch_softmax_item_sweep(const float* items, int64_t n_items, int64_t item_goff, const float* users,
                                     int64_t n_users, int64_t user_goff, int d, float inv_temp, const float* logq,
                                     const int64_t* item_ids, const int64_t* user_pos_ids, const float* lse,
                                     int64_t n_global, float* d_items, void* stream);

/* In-batch hard-negative BPR: every user trains against the m highest-scoring other items of the batch (online hard-
 * negative mining; not in the reference).  Indices are global as above: user i has gu = user_goff + i, item j has
 * gi = item_goff + j, user i's positive partner is the item with gi == gu.  Every user's partner must lie inside the
 * given items (item_goff <= user_goff and user_goff + n_users <= item_goff + n_items), else RIHIP_ERR_ARG.
 *   score     s_ij = <u_i, y_j>, exact-f32 MFMA; s_ii is the partner's score from the same sweep
 *   eligible  item j for user i iff j is not i's partner and, when the id arrays are given, item_ids[j] !=
 *             user_pos_ids[i] (the softmax mask; both int64, NULL together)
 *   order     eligible items by (score descending, global item index ascending): a total order, so the result does not
 *             depend on the order in which tiles or lanes deliver candidates; -0 and +0 are one score
 *   N_i       the items at ranks skip .. skip+m-1 of that order (fewer may exist); c_i = |N_i|, 0 <= c_i <= m
 *   loss      (1/n_global) sum_i [c_i > 0] (1/c_i) sum_{j in N_i} softplus(s_ij - s_ii)
 *   w_ij      sigma(s_ij - s_ii) / (n_global c_i) for j in N_i;  W_i = sum_j w_ij
 *   d_users[i] = sum_{j in N_i} w_ij y_j - W_i y_partner
 *   d_items[j] = sum_{i : j in N_i} w_ij u_i - [j is the partner of a given user i] W_i u_i
 *   softplus(z) = fmaxf(z,0) + log1pf(__expf(-|z|)), sigma(z) = 1/(1 + __expf(-z)), as in the in-batch BPR sweeps.
 * d_items covers all given items, exact zeros where nothing lands, and is additive over slices of the users.
 * Limits: 1 <= m <= 32, skip >= 0, skip + m <= 64, n_items < 2^31, n_users (m + 1) < 2^31, d any multiple of 16 up to
 * 256.  Inputs must be finite: non-finite scores give an unspecified selection, but never an index outside
 * [0, n_items) or -1 and never a fault.  A row with c_i = 0 has zero loss and zero gradient (no 0/0).  Two rows that
 * carry the same item id count as two negatives, as in in-batch BPR.
 * rihip_inbatch_hard_select: neg_idx int32[n_users, m] = LOCAL item indices in rank order, -1 in empty slots (empties
 *   come last); neg_score f32[n_users, m], 0 in empty slots; pos_score f32[n_users] = s_ii.  One launch.
 * rihip_inbatch_hard_grads: reads what select wrote (a slot whose index is outside [0, n_items) counts as empty);
 *   writes d_users, d_items and rihip_inbatch_hard_loss_parts(n_users) doubles to loss_part (one per 128 users; loss =
 *   rihip_sum_partials with scale 1/n_global).  workspace: rihip_inbatch_hard_workspace_bytes(n_users, n_items, m)
 *   bytes (-1 for sizes outside the limits), 256-byte aligned.  d_items is built by a stable sort of the n_users (m + 1)
 *   (item, pair) entries and one walk per item in ascending pair order.
 * No float atomics, no allocation, no host synchronisation: bitwise reproducible and capturable in a graph. */
int rihip_inbatch_hard_select(const float* users, int64_t n_users, int64_t user_goff, const float* items,
                              int64_t n_items, int64_t item_goff, int d, int m, int skip, const int64_t* user_pos_ids,
                              const int64_t* item_ids, int* neg_idx, float* neg_score, float* pos_score, void* stream);
int64_t rihip_inbatch_hard_loss_parts(int64_t n_users);
int64_t rihip_inbatch_hard_workspace_bytes(int64_t n_users, int64_t n_items, int m);
int rihip_inbatch_hard_grads(const float* users, int64_t n_users, int64_t user_goff, const float* items, int64_t n_items,
                             int64_t item_goff, int d, int m, const int* neg_idx, const float* neg_score,
                             const float* pos_score, int64_t n_global, float* d_users, float* d_items, double* loss_part,
                             void* workspace, void* stream);

/* Stored-G form of the same loss (two_tower.py:132-160), the default when memory allows: the user pass is the
 * mode_user=1 sweep that ALSO writes the weights sigma(s_ij - s_ii) (0 on the diagonal; G = weight/(B(B-1))) to `gmat`
 * (rihip_inbatch_gmat_floats(n_users, n_items) floats, 32x32-blocked G^T); the item pass is then a plain exact-f32
 * product d_items[j] = sum_i G[i][j] users[i] - r_j users[j] over the LOCAL users for ALL n_items items -- no second
 * score sweep (6 B^2 d FLOP per step instead of 8 B^2 d).  Multi-GPU: every rank calls both with its local users and
 * the all-gathered items, then reduce-scatters d_items.  Workspaces: rihip_inbatch_workspace_floats(n_users, n_items, d)
 * for the user pass and (n_items, n_users, d) for the item pass. */
int64_t rihip_inbatch_gmat_floats(int64_t n_users, int64_t n_items);
int rihip_inbatch_user_pass(const float* users, int64_t n_users, int64_t user_goff, const float* items,
                            int64_t n_items, int64_t item_goff, int d, const float* pos, int64_t n_global,
                            float* d_users, float* r_out, double* loss_part, float* workspace, float* gmat,
                            int precision, void* stream);
int rihip_inbatch_item_pass(const float* gmat, const float* users, int64_t n_users, int64_t user_goff,
                            int64_t n_items, int64_t item_goff, int d, const float* r, int64_t n_global,
                            float* d_items, float* workspace, int precision, void* stream);

/* Mixed in-batch objective L = L_inbatch + hard_weight * L_hard on the stored-G passes (not in the reference): the hard
 * negatives are mined from the weights the user pass left in `gmat`, no second score sweep.  Call order:
 *   rihip_rowdot, rihip_inbatch_user_pass (gmat), rihip_inbatch_gmat_mine, rihip_inbatch_mixed_apply,
 *   rihip_inbatch_item_pass (unchanged, on the boosted gmat and the corrected r), then ONE sum with scale c over the
 *   user pass's loss parts and the rihip_inbatch_mixed_loss_parts(n_users) parts of apply.
 * Indices are global as above: user i has gu = user_goff + i, item j has gi = item_goff + j, user i's positive partner is
 * the item with gi == gu.  Every user's partner must lie inside the given items (item_goff <= user_goff and user_goff +
 * n_users <= item_goff + n_items), else RIHIP_ERR_ARG.
 *   sigma_ij  the f32 stored in gmat for (item j, user i), at ((j/32) g_ub + i/32) 1024 + (j%32) 32 + i%32 with
 *             g_ub = 8 ceil(n_users/256);  n = n_global >= 2;  c = 1/(n(n-1))
 *   eligible  item j for user i iff j is not i's partner and, when the id arrays are given, item_ids[j] !=
 *             user_pos_ids[i] (both int64, NULL together).  By index, never by value: ragged slots and the 0 on the
 *             diagonal are never candidates, an eligible weight of 0 is one.  Only the 32x32 blocks that hold an in-range
 *             (item, user) pair are read (the blocks the user pass writes).
 *   order     eligible items by (sigma_ij descending, global item index ascending), on the orderable key of the f32
 *             bits of sigma_ij + 0.f: a total order, so the result depends neither on arrival order nor on nsplit.  NaN
 *             weights are undefined behaviour (an unspecified selection; never an index outside [0, n_items) or -1).
 *   N_i       the items at ranks skip .. skip+m-1 (fewer may exist); c_i = |N_i|, 0 <= c_i <= m
 *   boost     for c_i > 0: f_i = (float)(1.0 + (double)hard_weight (double)(n-1) / (double)c_i);  sigma'_ij = sigma_ij f_i,
 *             one round-to-nearest f32 multiply, written back to gmat in place for j in N_i; nothing else in gmat changes
 *   corrections, with D_ij = sigma'_ij - sigma_ij in f32 and S_i = sum_j D_ij, slots in rank order, fused multiply-adds:
 *             r_i += c S_i          d_users[i] += c (sum_j D_ij y_j - S_i y_partner)
 *   loss      z_ij = <u_i, y_j> - pos_i in f32 for the selected pairs only (pos: the array given to the user pass);
 *             loss_part[b] = hard_weight (n-1) sum_{i in 128-user block b} [c_i > 0] (1/c_i) sum_{j in N_i} softplus(z_ij)
 *             in double, so that c * (user-pass parts + these parts) = L_inbatch + hard_weight * L_hard
 *   A row with c_i = 0 changes nothing and contributes nothing; hard_weight = 0 writes nothing but zero loss parts.
 * Since sigma is non-decreasing in the score, N_i is rihip_inbatch_hard_select's selection except where two distinct
 * scores round to one f32 weight (saturated weights tie by index).
 * Limits: 1 <= m <= 32, skip >= 0, skip + m <= 64, n_items < 2^31, n_users < 2^31 / 33; apply: d in {32, 64, 128},
 * hard_weight finite and >= 0.
 * rihip_inbatch_gmat_mine: the bandwidth-bound pass, two launches.  neg_idx int32[n_users, m] = LOCAL item indices in
 *   rank order, -1 in empty slots (empties come last); neg_w f32[n_users, m] = the stored weight BEFORE the boost, 0 in
 *   empty slots.  nsplit: item-range splits whose partial lists are merged by key, 0 = the library's choice, at most
 *   rihip_inbatch_gmat_mine_max_nsplit(n_items); the result does not depend on it.  workspace:
 *   rihip_inbatch_gmat_mine_workspace_bytes(n_users, n_items, m, skip, nsplit) bytes for the same nsplit (-1 for
 *   arguments outside the limits), 8-byte aligned.
 * rihip_inbatch_mixed_apply: one launch; a wave handles one user at a time and 32 users in sequence (128 users = one
 *   loss part per workgroup).  Reads neg_idx / neg_w as mine wrote them (sigma_ij is
 *   taken from neg_w; a slot whose index is outside [0, n_items) counts as empty).  Mining and applying twice on one
 *   gmat boosts twice: the second mine sees the boosted weights.  Applying one selection twice rewrites the same
 *   sigma' but corrects r and d_users twice.
 * No float atomics, fixed summation order, no allocation, no host synchronisation: two calls on equal inputs are
 * bitwise equal, and the step is capturable in a graph. */
int rihip_inbatch_gmat_mine_max_nsplit(int64_t n_items);
int64_t rihip_inbatch_gmat_mine_workspace_bytes(int64_t n_users, int64_t n_items, int m, int skip, int nsplit);
int rihip_inbatch_gmat_mine(const float* gmat, int64_t n_users, int64_t user_goff, int64_t n_items, int64_t item_goff,
                            int m, int skip, const int64_t* user_pos_ids, const int64_t* item_ids, int nsplit,
                            int* neg_idx, float* neg_w, void* workspace, void* stream);
int64_t rihip_inbatch_mixed_loss_parts(int64_t n_users);
int rihip_inbatch_mixed_apply(float* gmat, const float* users, int64_t n_users, int64_t user_goff, const float* items,
                              int64_t n_items, int64_t item_goff, int d, const float* pos, int m, const int* neg_idx,
                              const float* neg_w, float hard_weight, int64_t n_global, float* d_users, float* r,
                              double* loss_part, void* stream);

/* ---- optimiser -----------------------------------------------------------------------------
 * clip_grad_norm_(max_norm) (train_embeddings.py:191): rihip_sumsq writes rihip_sumsq_nparts()
 * partial sums of x^2 per call; rihip_clip_coef reduces any number of partials to
 * coef = min(1, max_norm/(norm+1e-6)) ON DEVICE (no host sync), consumed by the Adam kernels. */
int rihip_sumsq_nparts(void);
/* Multi-tensor forms of rihip_sumsq / rihip_adam_dense for steps that are bounded by dependent kernel boundaries
 * (batch 256 ... 8192 at ML-1M scale): up to 4 tensors per launch, HOST arrays of device pointers and sizes; the
 * arithmetic and the partial layout (rihip_sumsq_nparts() doubles per tensor, consecutively) equal the single calls.
 * zero_grad_mask bit t: tensor t's gradient is overwritten with zeros after the update (dense table gradients). */
int rihip_sumsq_multi(int n_tensors, const float* const* x, const int64_t* n, double* part, void* stream);
int rihip_adam_dense_multi(int n_tensors, float* const* p, float* const* g, float* const* m, float* const* v,
                           const int64_t* n, int zero_grad_mask, float lr, float beta1, float beta2, float eps,
                           float weight_decay, int64_t step, const float* clip_coef, const float* hyper_dev,
                           void* stream);
int rihip_sumsq(const float* x, int64_t n, double* part, void* stream);
int rihip_clip_coef(const double* part, int64_t n_part, float max_norm, float* coef, float* total_norm, void* stream);
/* torch.optim.Adam(lr, betas, eps, weight_decay) single step with coupled L2
 * (train_embeddings.py:160,192); g is scaled by *clip_coef (nullable) first.  step >= 1. */
int rihip_adam_dense(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                     float eps, float weight_decay, int64_t step, const float* clip_coef, const float* hyper_dev,
                     void* stream);
/* Graph-replay clock: *step_dev += 1, then hyper_dev[0] = *lr_dev / (1 - beta1^t), hyper_dev[1] = sqrt(1 - beta2^t).
 * Passing hyper_dev (non-NULL) to rihip_adam_dense / rihip_adam_rows overrides their host-side lr/step arguments. */
int rihip_adam_hyper_step(int64_t* step_dev, const float* lr_dev, float beta1, float beta2, float* hyper_dev,
                          void* stream);
/* The same clock folded into the launches a step makes anyway (a small-batch step costs ~5 us per dependent launch):
 * rihip_clip_coef_step = rihip_clip_coef, then hyper_dev for t = *step_dev (the step that is running: initialise
 * *step_dev to 1), then *step_dev = t + 1.  loss_part (nullable): *loss = loss_scale * sum(loss_part[0..n)) as well --
 * the loss partials of rihip_bpr_pair_loss(loss = NULL) / the in-batch passes, summed off the critical path. */
int rihip_clip_coef_step(const double* part, int64_t n_part, float max_norm, float* coef, float* total_norm,
                         int64_t* step_dev, const float* lr_dev, float beta1, float beta2, float* hyper_dev,
                         const double* loss_part, int64_t n_loss_part, double loss_scale, float* loss, void* stream);

/* Row-sparse path for tables too large for a dense pass per step (SURVEY.md §7 hard part 1):
 * group (id,sample) pairs by id (radix sort), sum each row's contributions in sorted order
 * (bitwise reproducible), then Adam on touched rows only.  workspace bytes from
 * rihip_rows_workspace_bytes(B, d); uniq int64[B]; Gc float[B,d]; part double[rihip_rows_nparts()].
 * n_rows: number of table rows (ids < n_rows) -- only the significant key bits are sorted; 0 = unknown (all 63).
 * An id that is negative, or >= n_rows when n_rows is given, counts as the padding row 0: its gradient is dropped.
 * uniq[0 .. n_unique) is strictly ascending; row 0, when present, comes first with Gc = 0.  With n_rows = 0 the caller
 * vouches that every non-negative id is a row of the table rihip_adam_rows is given. */
int64_t rihip_rows_workspace_bytes(int64_t B, int d);
int rihip_rows_nparts(void);
int rihip_rows_group(const int64_t* ids, int64_t B, int d, int64_t n_rows, int64_t* uniq, void* workspace,
                     int64_t workspace_bytes, void* stream);
int rihip_rows_n_unique_ptr(void* workspace, int64_t B, int d, const int** n_unique_dev);
int rihip_rows_reduce(const float* dX, int64_t B, int d, const int64_t* uniq, void* workspace, float* Gc,
                      double* part, void* stream);
int rihip_adam_rows(float* table, float* m, float* v, const int64_t* uniq, const float* Gc, int64_t B, int d,
                    void* workspace, float lr, float beta1, float beta2, float eps, float weight_decay,
                    int64_t step, const float* clip_coef, const float* hyper_dev, void* stream);

/* ---- row-sharded tables (multi-GPU; BASELINE cfg4) ---------------------------------------------
 * The reference keeps each embedding table on one device (src/models/two_tower.py:27,:54; device picked at
 * src/training/train_embeddings.py:102-109).  Cut by rows over `world` ranks, global row g >= 1 lives on rank
 * (g-1) % world at local row (g-1)/world + 1 (local row 0 = unused padding).  route_rows sorts a batch of global
 * ids by owner (stable): sorted_local int64[B] = owner-local rows in send order, perm int64[B] = pair of each send
 * slot, pos int64[B] = send slot of each pair (the ids the tower kernels use on the received-row staging table),
 * counts int64[world] = requests per owner (the all-to-all split sizes).  gather_rows: out[i] = table[ids[i]]. */
int64_t rihip_route_workspace_bytes(int64_t B);
int rihip_route_rows(const int64_t* ids, int64_t B, int world, int64_t* sorted_local, int64_t* perm, int64_t* pos,
                     int64_t* counts, int* err_flag, void* workspace, int64_t workspace_bytes, void* stream);
/* Fixed-capacity form (no split size ever crosses to the host: equal-split all-to-alls of `cap` slots per peer):
 * slot_ids int64[world*cap] = owner-local rows in slot (owner*cap + position), 0 (the padding row: gradient dropped by
 * the row-sparse optimiser) in unused slots; slot_of_pair int64[B] = slot of each pair = its row in the
 * [world*cap, d] received-rows staging table; counts int64[world] (device).  cap = B can never overflow; a smaller cap
 * that does sets bit 2 of *err_flag.  scatter_rows: out[slot[i]] = src[i] (row gradients into their send slots). */
int rihip_route_rows_fixed(const int64_t* ids, int64_t B, int world, int64_t cap, int64_t* slot_ids,
                           int64_t* slot_of_pair, int64_t* counts, int* err_flag, void* workspace,
                           int64_t workspace_bytes, void* stream);
int rihip_scatter_rows(const float* src, const int64_t* slot, int64_t n, int64_t n_slots, int d, float* out,
                       int* err_flag, void* stream);
int rihip_gather_rows(const float* table, int64_t n_rows, const int64_t* ids, int64_t n, int d, float* out,
                      int* err_flag, void* stream);

/* ---- LambdaMART training -------------------------------------------------------
 * Replaces the body of LightGBMRanker.train (src/models/ranker.py:52-155): lgb.train(objective="lambdarank", ...) with
 * the reference's parameters (defaults below = ranker.py:107-121).  X device f32 [n,F] row-major, y device f32 [n]
 * (integer relevance grades), groups HOST int32 [ng] (documents per query, in row order; <= 16384 each); the
 * validation set is optional (NULL / 0): with it, training stops when an eval metric has not improved for
 * early_stopping_rounds.  model_text receives a malloc'd LightGBM-format text model (free with rihip_free):
 * rihip_gbdt_create_from_text loads it.  history (host, nullable): [n_rounds][2][n_eval_at] NDCG of train / valid
 * (valid = NaN without a validation set).  Synchronous.  Algorithm and its NumPy restatement: csrc/gbdt_train.hip,
 * oracle/lambdamart_np.py (lightgbm itself is not available offline: parity unpinned).
 * The ideal DCG (gradients and NDCG) takes the labels from the highest LABEL down, so label_gain must be non-decreasing.
 * Refused before anything is launched, reason in rihip_last_error: RIHIP_ERR_SHAPE for a group outside 1..16384;
 * RIHIP_ERR_ARG for F outside 1..255, group sizes that do not sum to n, num_leaves outside 2..128, max_bin outside
 * 2..255, truncation_level outside 1..32, n_label_gain outside 2..32, n_eval_at outside 1..8, an eval_at < 1,
 * n_estimators / bin_sample / min_child_samples / early_stopping_rounds < 1, a learning_rate, feature_fraction or sigmoid
 * that is not finite and > 0, a reg_alpha, reg_lambda or min_sum_hessian that is not finite and >= 0, hist_bits other
 * than 0, 20, 40, and a label_gain that decreases (or holds a NaN). */
typedef struct rihip_lambdamart_params {
  int num_leaves, n_estimators, min_child_samples, max_bin, truncation_level, early_stopping_rounds, lambdarank_norm,
      bin_sample;
  int n_eval_at;
  int eval_at[8];
  int n_label_gain;
  double label_gain[32];
  double learning_rate, reg_alpha, reg_lambda, feature_fraction, min_sum_hessian, sigmoid;
  uint64_t seed;
  /* fidelity switches towards LightGBM's defaults (0 = the integer-2^20 / NaN-as-zero / lowest-threshold behaviour):
   * hist_bits 20|40 (40: float-histogram fidelity, sums still order-independent integers); use_missing 1: NaN gets its
   * own bin and every node learns a default direction (decision_type missing = NaN); split_order 1: equal-gain
   * thresholds resolved in FeatureHistogram::FindBestThreshold's scan order */
  int hist_bits, use_missing, split_order, reserved;
} rihip_lambdamart_params;
int rihip_lambdamart_train(const float* X, const float* y, const int32_t* groups, int64_t n, int F, int ng,
                           const float* Xv, const float* yv, const int32_t* groups_v, int64_t nv, int ngv,
                           const rihip_lambdamart_params* params, const char* feature_names, char** model_text,
                           int* best_iteration, int* n_rounds, double* history, void* stream);
/* The gradient pass of one boosting round on its own -- the code rihip_lambdamart_train runs, not a copy: the stable
 * segmented sort of every query by descending score (+0.0 and -0.0 are one score), LambdarankNDCG::
 * GetGradientsForOneQuery per query, and the scatter back to document order.  scores device f64 [n], labels device f32
 * [n] (a label below 0 counts as 0, one above n_label_gain - 1 as n_label_gain - 1), groups HOST int32 [ng], label_gain
 * HOST f64 [n_label_gain]; out: lam, hes device f64 [n] in document order, sorted device int32 [n]: the row (0 .. n-1)
 * at every rank position, the queries one after another.  The checks of groups, n_label_gain, label_gain, sigmoid and
 * truncation_level are the trainer's.  Synchronous. */
int rihip_lambdarank_gradients(const double* scores, const float* labels, const int32_t* groups, int64_t n, int ng,
                               const double* label_gain, int n_label_gain, double sigmoid, int truncation_level,
                               int lambdarank_norm, double* lam, double* hes, int32_t* sorted, void* stream);
void rihip_free(void* p);

/* ---- inner-product index -------------------------------------------------------------------
 * Replaces faiss.IndexFlatIP / IndexIVFFlat(METRIC_INNER_PRODUCT) behind FAISSIndex
 * (src/models/faiss_index.py:68-74 build, :113/:145 search, :164/:196 write/read).
 * Normalisation of vectors/queries stays in the wrapper (faiss_index.py:64-65,:108-110).
 * search: Q device [nq,d]; out_scores f32[nq,k] descending, -inf padded; out_rows i64[nq,k]
 * row numbers in insertion order, -1 padded (faiss convention kept by faiss_index.py:148-152).
 * Exact for a flat index (ties -> lowest row); synchronises the stream once per 4096 queries
 * (exactness check).  k <= rihip_ip_index_max_k() (16384).  1 <= d <= 128: the handle zero-pads rows, queries and
 * centroids to its kernel width (32 / 64 / 128), which changes no inner product; every array that crosses the ABI is
 * [*, d] at the caller's width.  nlist <= 2048.
 * IVF (faiss_index.py:68-74): train_ivf = k-means (Lloyd, IP assignment, mean update, empty lists keep their
 * centroid) from seeded rows, then list-contiguous layout; train_ivf_from = the same from caller-supplied
 * initial centroids (host [nlist,d]; n_iter = 0 partitions by them as they are); set_ivf injects centroids AND
 * the list of every row (host int32 [N]) -- what a FAISS IndexIVFFlat file holds; get_ivf reads both back
 * (host, either may be NULL); reconstruct returns the stored vectors in insertion order (host [N,d]);
 * assign = list of each of n device rows under the index's centroids (device int32 [n]). */
int rihip_ip_index_create(int d, void** handle);
int rihip_ip_index_destroy(void* handle);
int rihip_ip_index_set_vectors(void* handle, const float* X, int64_t N, int x_on_device, void* stream);
int64_t rihip_ip_index_ntotal(void* handle);
int rihip_ip_index_is_ivf(void* handle);
int rihip_ip_index_nlist(void* handle);
int rihip_ip_index_max_k(void);
int rihip_ip_index_train_ivf(void* handle, int nlist, int n_iter, uint64_t seed, void* stream);
int rihip_ip_index_train_ivf_from(void* handle, int nlist, int n_iter, const float* init_centroids, void* stream);
int rihip_ip_index_set_ivf(void* handle, int nlist, const float* centroids, const int32_t* assign, void* stream);
int rihip_ip_index_get_ivf(void* handle, float* centroids, int32_t* assign);   /* synchronous */
int rihip_ip_index_reconstruct(void* handle, float* out);                       /* synchronous */
int rihip_ip_index_assign(void* handle, const float* X, int64_t n, int32_t* assign, void* stream);
int rihip_ip_index_set_nprobe(void* handle, int nprobe);
/* flat indexes with N > 65536: 1 (default) = bf16-MFMA filter with a rigorous error bound + exact f32 re-score of
 * the survivors (results identical to the all-f32 search, proven per query, exact fallback otherwise); 0 = all-f32 */
int rihip_ip_index_set_two_precision(void* handle, int enable);
int rihip_ip_index_search(void* handle, const float* Q, int64_t nq, int k, float* out_scores, int64_t* out_rows,
                          void* stream);
/* Deferred exactness check for serving chains (the reference's recommender.py:269-387 runs retrieval -> features ->
 * ranker per request; here the chain is enqueued without a host round trip in its middle): with enable = 1 a thresholded
 * IVF search of <= 4096 queries returns WITHOUT the host synchronisation that reads how many queries need the exact
 * re-do; enqueue the consumers of the result, then call rihip_ip_index_search_finish (one synchronisation): *n_redone > 0
 * means that many queries were re-done exactly into the same output rows after the consumers ran -- run them again.
 * finish must be called before the next search of the handle; all other search paths are unaffected (*n_redone = 0). */
int rihip_ip_index_set_deferred_check(void* handle, int enable);
int rihip_ip_index_search_finish(void* handle, int* n_redone, void* stream);
/* for hipGraph replays of a captured chain (no host code runs inside a replay): _pending = 1 while a deferred search
 * awaits its finish (ask right after capture); _last_fail_count synchronises `stream` and returns the failure count the
 * last enqueued deferred search wrote -- n > 0: run the chain again eagerly with the check not deferred */
int rihip_ip_index_search_pending(void* handle);
int rihip_ip_index_last_fail_count(void* handle, int* n, void* stream);
int rihip_ip_index_save(void* handle, const char* path);          /* host path; synchronous */
int rihip_ip_index_load(const char* path, void** handle);         /* host path; synchronous */
/* rows[i] = rows[i] >= 0 ? item_ids[rows[i]] : -1   (faiss_index.py:123, :148-152) */
int rihip_map_rows_to_ids(int64_t* rows, int64_t n, const int64_t* item_ids, void* stream);
/* The same mapping inside rihip_ip_index_search (no second pass over the result): with a non-NULL device array of
 * >= ntotal item ids, out_rows receives item_ids[row] (-1 padding unchanged).  The array is not copied and must stay
 * valid while searches run; NULL restores row numbers. */
int rihip_ip_index_set_id_map(void* handle, const int64_t* item_ids_dev);
/* Add / remove / replace items of a built index without retraining (faiss add_with_ids / remove_ids): ONE repack of the
 * corpus on the device under the existing centroids.  item_ids: device [N], the id of every stored row; drop_ids: device
 * [n_drop], any order, ids that are not stored are ignored; X_add: device [n_add,d] normalised rows, appended in call order
 * as rows N_keep .. N_keep+n_add-1 with the ids add_ids (device [n_add]); surviving rows keep their relative order and are
 * renumbered densely.  item_ids_out: device [N + n_add], receives the id of every row of the result (first *n_total
 * entries).  Host outputs: *n_total rows of the result, *n_dropped stored rows removed.  The handle is left bit for bit in
 * the state rihip_ip_index_set_vectors + rihip_ip_index_set_ivf of the final corpus (same centroids, kept rows in their
 * lists, new rows in their arg-max list) would leave it in; centroids are not retrained.  Refused with RIHIP_ERR_ARG and
 * *bad_kind = 1: an id is repeated inside drop_ids or add_ids, 2: an id to add is stored and not dropped by this call
 * (*bad_id names one such id), 3: the result would be empty; RIHIP_ERR_STATE while a deferred search is pending.  A
 * refused or failed call leaves the index as it was.  A call that drops and adds nothing changes nothing.  Synchronises the
 * stream.  Peak device memory: the old plus the new corpus.  Captured serve graphs are stale afterwards
 * (rihip_scratch_generation advances). */
int rihip_ip_index_update(void* handle, const int64_t* item_ids, const int64_t* drop_ids, int64_t n_drop,
                          const float* X_add, const int64_t* add_ids, int64_t n_add, int64_t* item_ids_out,
                          int64_t* n_total, int64_t* n_dropped, int64_t* bad_id, int* bad_kind, void* stream);
/* real rows of every IVF list (host int64 [nlist]) */
int rihip_ip_index_list_sizes(void* handle, int64_t* out);
/* Filtered search (faiss SearchParameters.sel / IDSelector on IndexFlat and IndexIVFFlat; the reference's FAISSIndex has
 * none): every stored row carries one 32-bit tag word, a query carries (any_of, all_of, none_of), and row r passes iff
 * (any_of == 0 || (tag[r] & any_of) != 0) && (tag[r] & all_of) == all_of && (tag[r] & none_of) == 0.  The result is the
 * exact top k of the passing rows (IVF: of the passing rows of the probed lists; probing does not look at tags) in the
 * plain search's order, padded with -inf / -1; (0,0,0) equals rihip_ip_index_search bit for bit.
 * set_tags: device uint32 [ntotal] in insertion-row order, copied into the order the scan reads (NULL clears);
 * synchronises the stream.  set_vectors, train_ivf*, set_ivf and rihip_ip_index_update drop the tags (has_tags = 0): set
 * them again in the new row order.  save / load do not carry tags.
 * search_filtered: pred_dev device uint32, query q's three words at pred_dev[q * pred_stride]; pred_stride = 3 (one
 * predicate per query) or 0 (one shared by the batch).  Honours set_id_map.  Its exactness check is always synchronous
 * (set_deferred_check is ignored); RIHIP_ERR_STATE without tags or while a deferred search is pending.  A large flat
 * index takes the all-f32 scan whatever set_two_precision says.
 * filtered_stats: cumulative {queries searched filtered, of those re-done by the exact fallback}.
 * search_stats: what the search driver did since the handle was made, plain and filtered searches alike: 12 cumulative
 * host-side counters (no kernel reads or writes them; reading them synchronises nothing).  A search of nq queries runs
 * ceil(nq / 4096) internal passes, each on one path:
 *   out[0]  passes on the flat dense path (N <= 65 536)
 *   out[1]  passes on the flat thresholded path, all-f32 (set_two_precision(0), or a filtered search)
 *   out[2]  ... two-precision with the fused refine (k <= 2048)       out[3]  ... two-precision, unfused re-score
 *   out[4]  passes on the unfiltered IVF path as the first choice (its use as the exact re-do is not counted here)
 *   out[5]  passes on the thresholded IVF path
 *   out[6]  of out[2] + out[3], the passes whose threshold sample kept the best scores per stream in registers
 *   out[7]  IVF prepares done in one launch (<= 8 queries; the re-do's prepares count)
 *   out[8]  queries that went through a thresholded pass (flat or IVF)
 *   out[9]  of those, the queries re-done exactly, those of rihip_ip_index_search_finish included
 *   out[10] re-do chunks (8 queries flat, 64 IVF)                     out[11] internal passes in all */
int rihip_ip_index_set_tags(void* handle, const uint32_t* tags_by_row_dev, void* stream);
int rihip_ip_index_has_tags(void* handle);
int rihip_ip_index_search_filtered(void* handle, const float* Q, int64_t nq, int k, const uint32_t* pred_dev,
                                   int64_t pred_stride, float* out_scores, int64_t* out_rows, void* stream);
int rihip_ip_index_filtered_stats(void* handle, int64_t* out);
int rihip_ip_index_search_stats(void* handle, int64_t* out);     /* out: int64[12] */
/* Seen-item exclusion inside the scan (not in the reference; the second implementation next to the over-fetch of
 * rihip_exclude_topk): query q of user u = user_ids[q] never returns a row whose item id is in row u of the seen lists.
 * The result is the first k rows, in the plain search's order (score descending, lower row first on ties), among the rows
 * of the probed lists (flat: all rows) that are not excluded and, with pred_dev, pass the predicate; -inf / -1 padded when
 * fewer qualify.  Scores and rows are bit for bit those rihip_ip_index_search reports for the same row.  There is no
 * over-fetch, so k + |seen| is not bounded by rihip_ip_index_max_k().
 * Seen lists: seen_offsets device i64 [n_seen_rows + 1], seen_items device i32 item ids, ascending and unique per row
 * (the convention of rihip_exclude_topk); user_ids device i64 [nq], NULL = row q, an id outside [0, n_seen_rows) excludes
 * nothing.  row_of: device i32 [n_ids], item id -> insertion row, -1 = not stored; ids outside the table or mapped to -1
 * are ignored.  pred_dev / pred_stride as in search_filtered; pred_dev may be NULL (no tag filter, tags not needed).
 * The scans test one bit per (query, row): bit p & 31 of word q * W + (p >> 5), W = ceil(P / 32), is set iff the row at
 * scan position p is excluded for query q (flat: p = row, P = ntotal; IVF: p = the list-major physical position, P = the
 * padded row count).  The mask is scratch of the handle, all zero between calls: a chunk of queries sets its bits,
 * searches and clears the words it touched.  The batch is taken in chunks of queries whose mask fits the budget
 * (set_exclusion_budget, bytes; 0 restores the default of 64 MiB; at least one query per chunk); results do not depend on
 * it.  The search goes the way a filtered one goes (synchronous exactness check, all-f32 scan on a large flat index).
 * RIHIP_ERR_STATE while a deferred search is pending or with pred_dev on an index without tags; a refused call leaves the
 * handle as it was.
 * exclusion_mask_words: W.   exclusion_mask: writes the mask [nq, W] the search would build to out_mask (device).
 * exclusion_scratch_nonzero: non-zero words of the handle's mask scratch (0 between calls; synchronises).
 * exclusion_stats: cumulative {queries searched this way, of those re-done by the exact fallback, mask chunks}. */
int rihip_ip_index_search_excluding(void* handle, const float* Q, int64_t nq, int k, const int64_t* user_ids,
                                    const int64_t* seen_offsets, int64_t n_seen_rows, const int32_t* seen_items,
                                    const int32_t* row_of, int64_t n_ids, const uint32_t* pred_dev, int64_t pred_stride,
                                    float* out_scores, int64_t* out_rows, void* stream);
int rihip_ip_index_exclusion_mask_words(void* handle, int64_t* words_per_query);
int rihip_ip_index_exclusion_mask(void* handle, int64_t nq, const int64_t* user_ids, const int64_t* seen_offsets,
                                  int64_t n_seen_rows, const int32_t* seen_items, const int32_t* row_of, int64_t n_ids,
                                  uint32_t* out_mask, void* stream);
int rihip_ip_index_set_exclusion_budget(void* handle, int64_t bytes);
int rihip_ip_index_exclusion_scratch_nonzero(void* handle, int64_t* n_words, void* stream);
int rihip_ip_index_exclusion_stats(void* handle, int64_t* out);  /* out: int64[3] */

/* ---- 8-bit scalar-quantised index (faiss IndexScalarQuantizer / IndexIVFScalarQuantizer at 8 bits; the reference's
 * FAISSIndex has none) ----------------------------------------------------------------------
 * A second handle type, built from the f32 rows of a built ip_index (which may be destroyed afterwards): one int8 code
 * per dimension, rows of 64 or 128 bytes, in the source's physical order (IVF: its lists and centroids; flat: one list).
 * Quantiser, per dimension j over all rows, in f32:  m_j = 0.5f * (lo_j + hi_j),  s_j = (hi_j - lo_j) / 254.0f  (1 where
 * hi_j == lo_j),  c_ij = clamp(rintf((x_ij - m_j) / s_j), -127, 127)  (one subtraction, one correctly rounded division),
 * decoded x^_ij = m_j + s_j * c_ij.  from_ip_index: centre / scale host f32 [d] inject (m, s) instead (both or neither;
 * scale > 0).  This is not faiss's QT_8bit (codes 0..255 over [lo, hi]); faiss SQ files are not read or written.
 * Query side (asymmetric, 16 bits):  w_j = q_j * s_j,  A = max_j |w_j|,  t = A / 32512.0f  (t = 0, n = 0 when A == 0),
 * n_j = clamp(rintf(w_j / t), -32512, 32512).  Integer score S_i = sum_j n_j * c_ij  (|S| < 2^31); ranking is by S, ties
 * to the lower row; reported score (float)(b + (double)t * S) with b = sum_j (double)q_j * (double)m_j in ascending j.
 * encode_queries: the search's first stage exposed -- device outputs n int16 [nq,d], t f32 [nq], b f64 [nq].
 * search: Q device f32 [nq,d]; outputs device scores f32 [nq,k] (-inf pad), rows i64 [nq,k] (-1 pad; set_id_map as for
 * ip_index), out_iscores i32 [nq,k] or NULL (INT32_MIN pad).  mode 0 = auto, 1 = dense slots per (query, probed list)
 * and the two-level select, queries chunked to a fixed scratch budget (auto takes it for small batches and small probed
 * populations), 2 = sampled threshold, survivors S >= threshold,
 * exact completeness check (integers: no epsilon), failed queries re-done dense; every mode returns the same bytes.
 * The thresholded pass synchronises the stream.  k <= rihip_ip_index_max_k().
 * get_codes: host int8 [N,d], reconstruct: host f32 [N,d], both in original row order; get_quantizer: host f32 [d] each.
 * stats: out[0] = queries searched thresholded, out[1] = of those re-done, out[2] = device bytes the index holds.
 * save / load: own format ("RIHIPSQ8", version word; header fields are range-checked on load). */
int rihip_sq8_index_from_ip_index(void* ip_handle, const float* centre, const float* scale, void** handle, void* stream);
int rihip_sq8_index_destroy(void* handle);
int64_t rihip_sq8_index_ntotal(void* handle);
int rihip_sq8_index_nlist(void* handle);
int rihip_sq8_index_set_nprobe(void* handle, int nprobe);
int rihip_sq8_index_set_id_map(void* handle, const int64_t* item_ids_dev);
int rihip_sq8_index_get_quantizer(void* handle, float* centre, float* scale);   /* synchronous */
int rihip_sq8_index_get_codes(void* handle, int8_t* out);                        /* synchronous */
int rihip_sq8_index_reconstruct(void* handle, float* out);                       /* synchronous */
int rihip_sq8_index_encode_queries(void* handle, const float* Q, int64_t nq, int16_t* out_n, float* out_t, double* out_b,
                                   void* stream);
int rihip_sq8_index_search(void* handle, const float* Q, int64_t nq, int k, int mode, float* out_scores, int64_t* out_rows,
                           int32_t* out_iscores, void* stream);
int rihip_sq8_index_stats(void* handle, int64_t* out);
int rihip_sq8_index_save(void* handle, const char* path);          /* host path; synchronous */
int rihip_sq8_index_load(const char* path, void** handle);         /* host path; synchronous */

/* ---- SQ8 index: tag filters inside the int8 scan.  Opt-in: without tags every call above returns what it returned
 * before.  The calls take an sq8_index handle and carry a prefix of their own, rihip_sq8_filter_*, as the refined search's do.
 * Filtered search (the ip_index's predicate, word for word): every stored row carries one 32-bit tag word, a query carries
 * (any_of, all_of, none_of), and row r passes iff
 *   (any_of == 0 || (tag[r] & any_of) != 0) && (tag[r] & all_of) == all_of && (tag[r] & none_of) == 0.
 * A filtered search returns the exact top k by (S descending, row ascending) of the PASSING rows of the probed lists:
 * probing does not look at tags, ties go to the lower row, padding is -inf / -1 / INT32_MIN, the reported score is the
 * plain search's (float)(b + t * S), and the predicate (0,0,0) returns rihip_sq8_index_search's bytes in every mode.  A
 * failing row is simply absent from the scan's output: it enters neither the threshold sample nor the survivor list nor
 * a dense slot (its slot holds the empty key 0).  So the thresholded pass keeps its integer completeness argument
 * unchanged under any pass rate, with "row" read as "passing row": the threshold is the rank-th best passing sampled
 * score; a sample with fewer than rank passing rows gives no threshold (INT_MIN: every passing probed row is a
 * candidate, as the plain search does for a short sample); a query that overflows its candidate slots, or holds fewer
 * than k candidates under a real threshold (one with fewer than k passing rows included), is re-done dense with its
 * predicate applied.  No passing rows are counted beforehand.
 * set_tags: device uint32 [ntotal] in insertion-row order, copied through the handle's row ids into the order the scan
 * reads, padding rows 0; NULL clears; synchronises the stream; captured graphs are stale afterwards
 * (rihip_scratch_generation advances).  save / load do not carry tags; rihip_sq8_index_stats out[2] counts 4 bytes per padded row.
 * search: rihip_sq8_index_search with pred_dev device uint32, query q's three words at
 * pred_dev[q * pred_stride]; pred_stride = 3 (one predicate per query) or 0 (one shared by the batch).  Honours
 * set_id_map.  RIHIP_ERR_STATE without tags.
 * stats: cumulative {queries searched filtered (any mode), of those re-done dense by the thresholded pass}. */
int rihip_sq8_filter_set_tags(void* handle, const uint32_t* tags_by_row_dev, void* stream);
int rihip_sq8_filter_has_tags(void* handle);
int rihip_sq8_filter_search(void* handle, const float* Q, int64_t nq, int k, int mode, const uint32_t* pred_dev,
                            int64_t pred_stride, float* out_scores, int64_t* out_rows, int32_t* out_iscores, void* stream);
int rihip_sq8_filter_stats(void* handle, int64_t* out);     /* out: int64[2] */

/* ---- SQ8 index: exact f32 re-ranking of the 8-bit candidates, with a per-query certificate (faiss has the first half as
 * IndexRefineFlat).  Opt-in: without attached vectors every call above returns what it returned before.  The calls take
 * an sq8_index handle; they carry a prefix of their own, rihip_sq8_refine_*, so the rihip_sq8_index_* family stays the set it was.
 * attach_vectors: copies the f32 rows of a built ip_index into the handle, in insertion-row order [N, dk] (the source may
 * be destroyed afterwards).  The source must hold the handle's rows in the handle's order: same N, width, list count and
 * list lengths, and the same row of every physical slot (compared on the device); anything else, an index updated since
 * the encode included, is RIHIP_ERR_STATE and leaves the handle as it was.  The call also computes, in f64 over the
 * stored rows and the STORED codes c_ij (so a clamped code of an injected quantiser counts with its full error),
 *   e_j = max_i | x_ij - (m_j + s_j * c_ij) |      (s_j * c_ij exact; one rounding in the sum, one in the difference)
 *   a_j = max_i | x_ij |
 * without atomics.  get_ranges: host f64 [d] each, synchronous.  drop_vectors / has_vectors: as named.  stats out[2]
 * counts the vectors; save / load do not carry them: a loaded index has none until they are attached again.
 *
 * search, k <= k_scan <= rihip_ip_index_max_k():
 *   Stage 1: rihip_sq8_index_search at k_scan in `mode`: the top k_scan of the probed rows by (S descending, row ascending).
 *   Stage 2: every valid stage-1 candidate is re-scored as f(q, x_row) in f32 and the top k by (f + 0.f descending, row
 *   ascending) is written: scores f32 [nq,k] (-inf pad), rows i64 [nq,k] (-1 pad where stage 1 held fewer than k rows;
 *   set_id_map applied after the select).  No host synchronisation beyond stage 1's.
 *   f(q, x), one fixed function of the two rows zero-padded to dk = 32 / 64 / 128 columns -- not of the batch, k, k_scan, the
 *   candidate's position or mode:  P = dk / 16;  for l = 0 .. 15:  s_l = 0.f, then for j = l*P .. l*P + P-1 ascending
 *   s_l = fmaf(q_j, x_j, s_l);  then for o = 8, 4, 2, 1:  s_l = s_l + s_(l xor o)  for all l at once;  f = s_0.
 *   Certificate: out_cert u8 [nq], out_bound f64 [nq] or NULL, all f64 on the device, sums in ascending j over j < d:
 *     E1 = sum_j |q_j| * e_j          the codes' error
 *     E2 = 127 * sum_j | q_j * s_j - t * n_j |     the query's 16-bit rounding (both products exact in f64), |c_ij| <= 127
 *                                                  (a residual PQ handle: 254 here and in W, the bound on its int16 codes)
 *     A  = sum_j |q_j| * a_j,   E3 = g * A,   g = u / (1 - u),  u = dk * 2^-24      f's own rounding: at most dk roundings on
 *                                                                                   any path from a product to f
 *     M  = sum_j |q_j * m_j|,   W = 127 * sum_j |t * n_j|       (magnitudes of b and of any t * S)
 *     slack = 2^-44 * ((((M + W) + A) + E1) + E2) + dk * 2^-126
 *     bound = ((E1 + E2) + E3) + slack
 *   slack: b is a sum of d exact products (relative error below 128 * 2^-53 of M); t * S rounds once (2^-53 W); each of
 *   the sums has at most 128 additions and three roundings per term (below 132 * 2^-53 relative); e_j carries two
 *   roundings, at most 2^-52 (a_j + e_j), i.e. 2^-52 (A + E1) in E1; U below adds three times (4 * 2^-53 of its terms).
 *   Together below 300 * 2^-53 of (M + W + A + E1 + E2); 2^-44 = 512 * 2^-53.  dk * 2^-126 covers f32 underflow in f.
 *   With S_cut the smallest integer score among the stage-1 candidates and U = (b + t * S_cut) + bound:
 *     cert = 1  iff  stage 1 returned fewer than k_scan valid rows (every probed row was re-scored)
 *                    or the k-th refined score > U.
 *   cert = 1 implies: the output equals the top k by (f, row) over ALL rows of the probed lists.  A probed row outside the
 *   candidates has S <= S_cut, so its real inner product is at most b + t * S_cut + E1 + E2 (its decoded row is within e of
 *   it, and the integer score is within E2 / t of the decoded row's product with q) and its f at most that plus E3; it is
 *   below the k-th refined score, and the k best candidates are k rows with a larger f.  bound does not depend on stage 1.
 *
 * search_filtered: rihip_sq8_refine_search with the two predicate arguments of rihip_sq8_filter_search.  Stage 1
 * is the filtered search at k_scan; stage 2 and the certificate are the same kernels with the same inputs.  cert = 1 then
 * proves that the list is the exact top k by (f, row) of the PASSING rows of the probed lists: the certificate's first
 * clause, "stage 1 returned fewer than k_scan valid rows", reads n_valid < k_scan, and a filtered stage 1 returns fewer
 * than k_scan rows exactly when fewer than k_scan probed rows pass -- it ran out of passing rows and every one of them
 * was re-scored; in the second clause S_cut bounds every passing probed row outside the candidates, and rows that fail
 * are outside the claim.  RIHIP_ERR_STATE without vectors or without tags. */
int rihip_sq8_refine_attach_vectors(void* handle, void* ip_handle, void* stream);   /* synchronous */
int rihip_sq8_refine_drop_vectors(void* handle);                                    /* synchronous */
int rihip_sq8_refine_has_vectors(void* handle);
int rihip_sq8_refine_get_ranges(void* handle, double* e, double* a);         /* synchronous */
int rihip_sq8_refine_search(void* handle, const float* Q, int64_t nq, int k, int k_scan, int mode, float* out_scores,
                                   int64_t* out_rows, uint8_t* out_cert, double* out_bound, void* stream);
int rihip_sq8_refine_search_filtered(void* handle, const float* Q, int64_t nq, int k, int k_scan, int mode,
                                     const uint32_t* pred_dev, int64_t pred_stride, float* out_scores, int64_t* out_rows,
                                     uint8_t* out_cert, double* out_bound, void* stream);

/* ---- SQ8 index: seen-item exclusion inside the int8 scan (the SQ8 side of rihip_ip_index_search_excluding; the calls
 * take an sq8_index handle and carry the prefix rihip_sq8_exclude_*, the refined one rihip_sq8_refine_*).
 * exclude_search: rihip_sq8_index_search / rihip_sq8_filter_search (pred_dev non-NULL; NULL needs no tags) over the rows
 * that are not excluded for the query's user: the first k of the probed rows by (S descending, row ascending) among the
 * rows whose item id is not in the user's seen list and that pass the predicate; -inf / -1 / INT32_MIN padded.  Scores,
 * integer scores and rows are bit for bit those the plain search reports for the same row, in every mode.  user_ids,
 * seen_offsets, seen_items, row_of and the mask layout are those of rihip_ip_index_search_excluding; scan positions are the
 * handle's physical rows (a flat-built handle is one list, padded to 64 rows), W = ceil(padded rows / 32).  The mask is
 * handle scratch, all zero between calls (set, search, clear the touched words per chunk of queries); the chunk is the
 * smaller of the search's own and what the budget holds.  rihip_sq8_update_apply drops the row -> position table with the
 * row order; it is rebuilt on the next call.  RIHIP_ERR_STATE with pred_dev on an index without tags; a refused call
 * leaves the handle as it was.
 * refine_search_excluding: rihip_sq8_refine_search whose stage 1 is exclude_search at k_scan.  Stage 2, f, the bound and
 * the certificate are the same kernels; "stage 1 returned fewer than k_scan valid rows" then means that every probed row
 * that is not excluded (and passes) was re-scored, so cert = 1 implies: the output equals the top k by (f, row) over all
 * such rows of the probed lists.
 * exclude_mask_words / exclude_mask / exclude_set_exclusion_budget / exclude_scratch_nonzero / exclude_exclusion_stats:
 * as the rihip_ip_index_exclusion_* calls. */
int rihip_sq8_exclude_search(void* handle, const float* Q, int64_t nq, int k, int mode, const int64_t* user_ids,
                             const int64_t* seen_offsets, int64_t n_seen_rows, const int32_t* seen_items,
                             const int32_t* row_of, int64_t n_ids, const uint32_t* pred_dev, int64_t pred_stride,
                             float* out_scores, int64_t* out_rows, int32_t* out_iscores, void* stream);
int rihip_sq8_refine_search_excluding(void* handle, const float* Q, int64_t nq, int k, int k_scan, int mode,
                                      const int64_t* user_ids, const int64_t* seen_offsets, int64_t n_seen_rows,
                                      const int32_t* seen_items, const int32_t* row_of, int64_t n_ids,
                                      const uint32_t* pred_dev, int64_t pred_stride, float* out_scores, int64_t* out_rows,
                                      uint8_t* out_cert, double* out_bound, void* stream);
int rihip_sq8_exclude_mask_words(void* handle, int64_t* words_per_query);
int rihip_sq8_exclude_mask(void* handle, int64_t nq, const int64_t* user_ids, const int64_t* seen_offsets,
                           int64_t n_seen_rows, const int32_t* seen_items, const int32_t* row_of, int64_t n_ids,
                           uint32_t* out_mask, void* stream);
int rihip_sq8_exclude_set_exclusion_budget(void* handle, int64_t bytes);
int rihip_sq8_exclude_scratch_nonzero(void* handle, int64_t* n_words, void* stream);
int rihip_sq8_exclude_exclusion_stats(void* handle, int64_t* out);   /* out: int64[3] */

/* ---- SQ8 index: add / remove / replace items without the f32 source and without re-encoding the rows that stay (what
 * rihip_ip_index_update is to the ip_index).  The calls take an sq8_index handle and carry a prefix of their own,
 * rihip_sq8_update_*.  ONE repack of the code matrix on the device under the handle's own centroids and its own
 * quantiser (centre, scale); neither is retrained.  The quantiser is per row and per dimension, so a kept row keeps its
 * code; only the new rows are encoded, c_ij = clamp(rintf((x_ij - m_j) / s_j), -127, 127) as above.
 * apply: item_ids: device [N], the id of every stored row; drop_ids: device [n_drop], any order, ids that are not stored
 * are ignored; X_add: device f32 [n_add,d] normalised rows, 16-byte aligned, appended in call order as rows N_keep ..
 * N_keep+n_add-1 with the ids add_ids (device [n_add]); add_tags: device uint32 [n_add], the tag words of the new rows,
 * or NULL meaning 0 (ignored on a handle without tags); surviving rows keep their relative order and are renumbered
 * densely.  item_ids_out: device [N + n_add], receives the id of every row of the result (first *n_total entries).  Host
 * outputs: *n_total rows of the result, *n_dropped stored rows removed, *n_clamped the pairs (new row i, column j < d)
 * whose unclamped rintf((x_ij - m_j) / s_j) lies outside +-127: an integer count, the drift signal of a frozen quantiser.
 * The handle is left bit for bit in the state that
 *   rihip_sq8_index_from_ip_index(ip, centre, scale) with ip an f32 index of the final corpus (same centroids, kept rows
 *   in their lists, new rows in their arg-max list, lowest list id on ties) and the handle's own quantiser,
 *   rihip_sq8_filter_set_tags of the final tag words, if the handle had tags, and
 *   rihip_sq8_refine_attach_vectors(ip), if the handle had vectors (e_j and a_j are recomputed over the final rows against
 *   the final stored codes, not updated incrementally: removing a row can shrink a maximum)
 * would leave it in.  A flat-built handle (one list) keeps its one list.  set_id_map is reset to NULL.  Refused with
 * RIHIP_ERR_ARG and *bad_kind = 1: an id is repeated inside drop_ids or add_ids, 2: an id to add is stored and not
 * dropped by this call (*bad_id names one such id), 3: the result would be empty; more than 2^31 rows are refused.  A
 * refused or failed call leaves the index searchable exactly as it was (the new arrays are built next to the old ones and
 * swapped at the end; peak device memory: the old plus the new index).  A call that drops and adds nothing changes
 * nothing.  One host synchronisation for the checks and one before the swap.  Captured serve graphs are stale afterwards
 * (rihip_scratch_generation advances).
 * assign: assign_out device int32 [n] = the list each of the n device rows X [n,d] would be added to (arg-max inner
 * product with the centroids, lowest list id on ties); a flat-built handle gives 0 for every row.
 * stats: cumulative {updates applied, rows dropped, rows added, code values clamped} since the handle was made. */
int rihip_sq8_update_apply(void* handle, const int64_t* item_ids, const int64_t* drop_ids, int64_t n_drop,
                           const float* X_add, const int64_t* add_ids, const uint32_t* add_tags, int64_t n_add,
                           int64_t* item_ids_out, int64_t* n_total, int64_t* n_dropped, int64_t* n_clamped,
                           int64_t* bad_id, int* bad_kind, void* stream);
int rihip_sq8_update_assign(void* handle, const float* X, int64_t n, int32_t* assign_out, void* stream);
int rihip_sq8_update_stats(void* handle, int64_t* out);     /* out: int64[4] */

/* ---- Product-quantised index (faiss IndexPQ / IndexIVFPQ; the reference's FAISSIndex has none) -------------------
 * An sq8_index handle whose storage is one byte per sub-space and row plus int8 codebooks: dpad / dsub bytes per row
 * (dsub = 8 or 16 dimensions per sub-space) instead of dpad.  The quantiser works on the rows' SQ8 codes
 * c[i][j] = the SQ8 code of x_ij under (centre, scale) (trained as above, or injected; padding columns 0), in integers:
 *   sub-space m = columns m dsub .. + dsub - 1, M = dpad / dsub (one lying in the padding columns is treated like any other);
 *   book[m][e][j] int8 in [-127, 127], 256 entries per sub-space;
 *   D(i, m, e) = sum_j (c[i][m dsub + j] - book[m][e][j])^2 (i32); a row's byte is the e of the smallest D, lowest e on ties;
 *   init: book[m][e] = the sub-vector of original row (e N) / 256 (int64; N < 256 repeats rows, the repeats stay empty);
 *   one Lloyd step: assign every stored row, book[m][e][j] = clamp(rint((double)sum / (double)cnt), -127, 127) (half to
 *   even) over the rows assigned to e, exact integer sums; an entry with cnt = 0 keeps its value;
 *   n_iter steps, then the final assignment, which is stored.  The sum of the smallest D of every assignment pass is the
 *   distortion trace (n_iter + 1 values).  Nothing depends on the physical row order: a flat and an IVF build of the same
 *   rows under the same (centre, scale) give the same codebooks and the same byte for every original row.
 *   Decoded code c^[i][m dsub + j] = book[m][byte[i][m]][j].
 * No residual encoding against the IVF centroids by default: one integer score per row, comparable across lists (the
 * opt-in residual form follows below at rihip_pq_index_from_ip_index_residual).
 * from_ip_index: as the SQ8 call; book host int8 [M,256,dsub] injects the codebooks and skips training (no byte -128).
 * The build holds the SQ8 codes transiently (train_stats: peak_bytes) and frees them before it returns.
 * Every rihip_sq8_* search, filter, exclude, refine, stats and id-map call takes the handle and returns what it returns
 * on the SQ8 index whose code matrix is the decoded one; rihip_sq8_index_get_codes / _reconstruct return that decoded
 * matrix (a transient N * dpad bytes on the device, as rihip_sq8_refine_attach_vectors takes for e_j / a_j).
 * rihip_sq8_update_apply returns RIHIP_ERR_STATE and changes nothing (rihip_pq_update_apply below updates the handle under
 * frozen codebooks); rihip_sq8_index_save refuses the handle.
 * get_codes: host uint8 [N,M] in original row order; get_codebooks: host int8 [M,256,dsub]; dims: dsub and M.
 * train_stats: trace (up to cap values; *n_trace = how many the build recorded: n_iter + 1, 1 with injected codebooks, 0
 * after load), peak_bytes, ms[3] = host time of {range pass + SQ8 encode, training, final assignment}; any may be NULL.
 * save / load: own format ("RIHIPPQ1", version word, range-checked header); each of the two loaders refuses the other's
 * file.  faiss PQ files are not read or written. */
int rihip_pq_index_from_ip_index(void* ip_handle, const float* centre, const float* scale, int dsub, int n_iter,
                                 const int8_t* book, void** handle, void* stream);
int rihip_pq_index_dims(void* handle, int* dsub, int* M);
int rihip_pq_index_get_codes(void* handle, uint8_t* out);          /* synchronous */
int rihip_pq_index_get_codebooks(void* handle, int8_t* out);       /* synchronous */
int rihip_pq_index_train_stats(void* handle, int64_t* trace, int cap, int* n_trace, int64_t* peak_bytes, double* ms);
int rihip_pq_index_save(void* handle, const char* path);           /* host path; synchronous */
int rihip_pq_index_load(const char* path, void** handle);          /* host path; synchronous */

/* ---- Product-quantised index: residual codes against the IVF centroids (faiss IndexIVFPQ's by_residual) -----------
 * Opt-in (by_residual != 0); without it every call above does what it did, bit for bit.  The source must be an IVF
 * ip_index (a flat one has one list and no centroids: RIHIP_ERR_ARG).  m, s: the handle's SQ8 quantiser, computed over the
 * rows or injected as above; c_i: row i's SQ8 code, int8 [dpad], padding columns 0; l(i): the list that holds row i;
 * C_l: the handle's centroid, f32 [nlist, dk].
 *   1. List codes   K_l[j] = clamp(rintf((C_l[j] - m_j) / s_j), -127, 127) for j < d, 0 in the padding columns: int8
 *      [nlist, dpad].  An empty list has a centroid and so a K_l.
 *   2. Residual     r_i[j] = clamp((int)c_i[j] - (int)K_l(i)[j], -127, 127), int8.  The clamp is part of the definition; the
 *      values it changed are counted (residual_clamped) and are never a reason to refuse.
 *   3. Quantiser    the quantiser above, unchanged, with r in place of c: seeds from original rows (e N) / 256, n_iter
 *      Lloyd steps with exact integer sums, one f64 division per codebook byte, ties to the lowest entry, entries in
 *      [-127, 127].  The distortion trace is over r.  Injected codebooks are residual codebooks and skip the training.
 *   4. Decoded code c^_i[j] = K_l(i)[j] + book[m][byte[i][m]][j mod dsub]: an int16 in [-254, 254], NOT clamped.  The
 *      reconstruction is x^_ij = m_j + s_j * c^_ij (f32: (float)c^, one product, one sum).
 *   5. Score        S_i = sum_j n_j c^_ij = T[q, l(i)] + sum_j n_j book[..][j],  T[q, l] = sum_j n_j K_l[j] an exact i32.
 *      |n_j| <= 32512, |c^| <= 254, dpad <= 128: |S| <= 32512 * 254 * 128 = 1 057 030 144 < 2^30, so the candidate key, the
 *      i32 threshold, out_iscores and S_cut are used as they are.  T is computed per (query, probed list) pair after the
 *      query transform; the scan adds it to the gathered dot product wherever it forms a score.
 *      A residual PQ index is thereby the exact-integer-score index of its own int16 reconstruction: everything the
 *      rihip_sq8_* searches promise holds with "the decoded matrix" read as c^ -- ranking by (S descending, row ascending),
 *      the reported score (float)(b + t S), the same bytes from all three modes, the integer completeness argument of the
 *      thresholded pass and its re-do, tag filters, both exclusion routes.
 *   6. Refine       stage 2 reads only the attached f32 rows and does not change.  e_j is taken over the int16 decoded
 *      codes (s_j * c^_ij is still exact in f64).  In the certificate of rihip_sq8_refine_search the factor 127 in E2 and W
 *      is the bound on |c_ij|; on a residual handle it is 254, on every other handle it stays 127 with the same bits.  The
 *      proof reads as before: the integer score is within E2 / t of the decoded row's product with q because each of the d
 *      terms |q_j s_j - t n_j| is multiplied by a code of magnitude at most 254, and W bounds |t S| the same way.
 *   7. rihip_sq8_index_get_codes (int8) returns RIHIP_ERR_STATE on a residual handle; get_decoded16 returns the decoded
 *      matrix, host int16 [N, d] in original row order.  rihip_sq8_index_reconstruct works.  Live updates: rihip_pq_update_apply below.
 * is_residual: 1 / 0.  get_list_codes: host int8 [nlist, dpad].  residual_clamped: the count of step 2 (0 after load, and
 * on a handle that is not residual).
 * save: rihip_pq_index_save writes a residual handle in a format of its own: "RIHIPPR1", the PQ header with a third
 * word of its own {dsub, M, nlist * dpad}, and the payload list codes int8[nlist, dpad], codebooks, entry numbers.
 * load_residual reads it; rihip_sq8_index_load, rihip_pq_index_load and load_residual refuse each other's files. */
int rihip_pq_index_from_ip_index_residual(void* ip_handle, const float* centre, const float* scale, int dsub, int n_iter,
                                          const int8_t* book, int by_residual, void** handle, void* stream);
int rihip_pq_index_is_residual(void* handle);
int rihip_pq_index_get_list_codes(void* handle, int8_t* out);      /* synchronous */
int rihip_pq_index_get_decoded16(void* handle, int16_t* out);      /* synchronous */
int rihip_pq_index_residual_clamped(void* handle, int64_t* out);
int rihip_pq_index_load_residual(const char* path, void** handle); /* host path; synchronous */

/* ---- Product-quantised index: add / remove / replace items under frozen codebooks (faiss IndexIVFPQ::add after train) --
 * What rihip_sq8_update_apply is to the SQ8 handle, for a handle with PQ storage (plain or residual, flat or IVF, dsub 8
 * or 16).  rihip_sq8_update_apply itself keeps refusing such a handle; the caller chooses this entry point knowingly,
 * because nothing is retrained: the centroids, the SQ8 quantiser (m, s), the list codes K_l and the codebooks stay as
 * they are.  ONE repack of the entry-number matrix; a kept row keeps its M bytes, a new row x in list l (its arg-max
 * list, lowest on ties; the one list of a flat-built handle) gets
 *   c[j] = clamp(rintf((x_j - m_j) / s_j), -127, 127) for j < d, 0 in the padding columns,
 *   on a residual handle r[j] = clamp((int)c[j] - (int)K_l[j], -127, 127) in place of c (each clamp counted),
 *   byte[m] = the e of the smallest D = sum_j (c[m dsub + j] - book[m][e][j])^2 (i32), the lowest e on a tie.
 * Parameters, outputs, checks, *bad_kind codes and refusal texts are those of rihip_sq8_update_apply; *n_clamped is the
 * SQ8-grid clamp count of this call (the same integer).  The handle is left bit for bit in the state that
 *   rihip_pq_index_from_ip_index_residual(ip, m, s, dsub, any n_iter, the handle's own codebooks, by_residual as the
 *   handle) with ip an f32 index of the final corpus (same centroids, kept rows in their lists, new rows in theirs),
 *   rihip_sq8_filter_set_tags of the final tag words, if the handle had tags, and
 *   rihip_sq8_refine_attach_vectors(ip), if the handle had vectors
 * would leave it in: entry numbers, row ids, list offsets and lengths, tags, vectors, e_j / a_j; saved files are byte
 * for byte the same ("RIHIPPQ1" / "RIHIPPR1" unchanged).  With vectors the new state is decoded transiently (N' * dpad
 * bytes, twice that on a residual handle) for e_j / a_j.  A refused or failed call leaves the handle searchable exactly
 * as it was; the generation advances only on a real change.  RIHIP_ERR_STATE on a handle without PQ storage.
 * stats: {updates applied, rows dropped, rows added, SQ8 code values clamped, residual values clamped, the summed smallest
 * D over all added rows and sub-spaces} cumulative since the handle was made, then the last two of the last update that
 * changed the index.  distortion_added / rows added against the build's last trace value / N is the drift signal of
 * frozen codebooks.  rihip_sq8_update_assign and rihip_sq8_update_stats take the handle as before. */
int rihip_pq_update_apply(void* handle, const int64_t* item_ids, const int64_t* drop_ids, int64_t n_drop,
                          const float* X_add, const int64_t* add_ids, const uint32_t* add_tags, int64_t n_add,
                          int64_t* item_ids_out, int64_t* n_total, int64_t* n_dropped, int64_t* n_clamped,
                          int64_t* bad_id, int* bad_kind, void* stream);
int rihip_pq_update_stats(void* handle, int64_t* out);      /* out: int64[8] */

/* ---- LambdaMART forward --------------------------------------------------------------------
 * Replaces lgb.Booster(model_file=...) (src/models/ranker.py:219) and Booster.predict
 * (ranker.py:174): raw score = sum over trees of the reached leaf value, float64.
 * X device f32 [n, ldx]; out device f64 [n].
 * predict_path names the kernel rihip_gbdt_predict launches for this handle (chosen when the model is parsed):
 * 0 general (any forest), 1 compact nodes with missing types, 2 compact nodes without, 3 walk-ordered records. */
int rihip_gbdt_load_text(const char* path, void** handle);
int rihip_gbdt_create_from_text(const char* text, int64_t len, void** handle);
int rihip_gbdt_destroy(void* handle);
int rihip_gbdt_num_trees(void* handle);
int rihip_gbdt_num_features(void* handle);
int rihip_gbdt_predict_path(void* handle);
int64_t rihip_gbdt_feature_names(void* handle, char* buf, int64_t buf_len); /* '\n'-joined, host */
int rihip_gbdt_feature_importance(void* handle, int importance_type, double* out_host);
int rihip_gbdt_predict(void* handle, const float* X, int64_t n, int ldx, double* out, void* stream);

/* Per-feature contributions to the raw score (lgb.Booster.predict(X, pred_contrib=True)): TreeSHAP with
 * path-dependent covers (Lundberg, Erion, Lee: "Consistent individualized feature attribution for tree ensembles",
 * Algorithm 2) over the leaf_count / internal_count lines of the model text.
 *   out[r, f] = sum over trees and root-to-leaf paths P of  (one_f - zero_f) * U_f(P, r) * leaf_value(P)    (f < F)
 *   out[r, F] = sum over trees of  sum_leaves leaf_value * leaf_count / count(root)     (the expected value)
 * A path keeps one element per distinct feature it splits on: zero_f is the product of count(child on the path) /
 * count(node) over its splits on f; one_f is 1 when row r goes to the path's child at every one of them (the decision
 * rule of rihip_gbdt_predict, every decision type) and 0 otherwise.  U_f is the sum of the path weights -- EXTEND over
 * the root's dummy element and all elements -- with element f unwound again.  A tree of one leaf adds its value to
 * out[r, F] only.  For an average_output model every column is divided by the tree count, so out[r, :] sums to what
 * rihip_gbdt_predict returns for row r (up to f64 rounding).
 * X device f32 [n, ldx]; out device f64 [n, F + 1], F = rihip_gbdt_num_features.  f64 arithmetic throughout, no
 * floating-point atomics: two calls are bitwise equal and a row's result does not depend on the other rows.  Enqueues
 * on `stream`, no host synchronisation; the path tables are built on the first call and the scratch (at most 64 MiB,
 * longer calls run as several row blocks) belongs to the handle.
 * rihip_gbdt_has_counts: 1 when every tree with a split carries both count lines.
 * Errors (non-zero, reason in rihip_last_error, nothing launched): a model without counts; a non-positive
 * internal_count or leaf_count; a tree of more than 128 leaves; a path with more than 64 distinct features;
 * more than 65535 trees. */
int rihip_gbdt_has_counts(void* handle);
int rihip_gbdt_predict_contrib(void* handle, const float* X, int64_t n, int ldx, double* out, void* stream);

/* ---- ranking-feature assembly ----------------------------------------------------------------
 * Replaces RecommendationPipeline._build_ranking_features (src/serving/recommender.py:213-263) and the
 * feature-store fetch in front of it (recommender.py:319-322) with GPU-resident float64 tables:
 * user_tab [n_user_rows, 24] = avg_rating, log_rating_count, recency_score, gender_encoded, age_normalized,
 * occupation_normalized, genre_pref[18]; item_tab [n_item_rows, 23] = avg_rating, log_rating_count,
 * popularity_score, rating_stddev, year_normalized, genre_vector[18]; row 0 and absent rows = the reference's
 * defaults.  cand_ids [nq,kc] (-1 = padding -> zero row).  col_map[nf]: canonical column index (order of
 * src/features/feature_engineering.py:434-443) of each ranker feature, -1 => 0.0 (recommender.py:334-336).
 * X f32 [nq*kc, nf]: values computed in float64 and cast once, like ranker.py:173. */
int rihip_rank_features_widths(int* user_width, int* item_width, int* n_canonical);
int rihip_rank_features_build(const double* user_tab, int64_t n_user_rows, const double* item_tab,
                              int64_t n_item_rows, const int64_t* user_ids, const int64_t* cand_ids, int64_t nq,
                              int kc, const int* col_map, int nf, float* X, void* stream);
/* nlargest(k, "score") of every request (src/serving/recommender.py:346): scores f64 [nq,kc] (ranker output), cand i64
 * [nq,kc] (-1 = padding, ranked last), retrieval_scores f32 [nq,kc]; outputs [nq,k], ties keep the retrieval order
 * (-0.0 ties with +0.0 and comes back with its sign; NaN scores rank after every number, before padding; outputs past
 * the kc candidates are -1 / -inf). */
int rihip_rank_topk(const double* scores, const int64_t* cand, const float* retrieval_scores, int64_t nq, int kc, int k,
                    int64_t* out_ids, double* out_scores, float* out_retrieval_scores, void* stream);

/* Diversified top-k (not in the reference, which stops at nlargest): greedy Maximal Marginal Relevance re-ranking.
 * Replaces rihip_rank_topk as the last stage of the serving chain when a diversity weight is asked for; inputs and
 * outputs are rihip_rank_topk's.  vec_tab: device f64 table, row index = item id, n_rows rows of stride ld; the vector
 * of an item is columns col0 .. col0 + w - 1 of its row.  diversity = d in [0, 1].
 *  - Eligible: cand >= 0 and a score that is not NaN.  Candidates with NaN scores, then padded ones, fill the slots
 *    left once the eligible ones run out, each group in retrieval order (rihip_rank_topk's order; their output score is
 *    the NaN / -inf); slots past kc are -1 / -inf / -inf.
 *  - Relevance r = (s - smin) / (smax - smin) in f64, smin / smax over the finite eligible scores; r = 0 for every
 *    candidate when smax == smin or no score is finite; +inf -> 1.0, -inf -> 0.0.
 *  - sim(a, b) = dot(a, b) / (|a| * |b|): dot and the sums of squares in f64, sequentially over components 0..w-1,
 *    multiply and add unfused (no FMA); |.| a correctly rounded sqrt; sim = 0 when either norm is 0 or either id is
 *    outside [0, n_rows).  This is intra_list_diversity's cosine (src/evaluation/metrics.py:168-190).
 *  - For t = 0..k-1 pick the eligible, unselected candidate of largest obj = (1 - d) * r - d * m, m = the largest sim
 *    to anything selected so far (0 while nothing is); 1 - d is one f64 subtraction, obj two unfused multiplies and
 *    one subtraction (a NaN obj, possible only with non-finite vectors, counts as -inf).  Ties in obj: the larger raw
 *    score (==, so -0.0 ties +0.0), then the smaller retrieval position.
 *  - Outputs [nq, k] in selection order: ids, raw ranker scores, retrieval scores.  d = 0 is rihip_rank_topk bit for
 *    bit; at d = 1 the first pick is still the best score.
 * Limits: 1 <= kc <= 4096, k >= 1, 1 <= w <= 256, col0 >= 0, ld >= col0 + w, 0 <= d <= 1 (NaN rejected): anything
 * else is RIHIP_ERR_ARG and nothing is launched.  One workgroup per request, O(k * kc * w) work; no host
 * synchronisation, no allocation, no atomics: capturable in a hipGraph and bitwise reproducible. */
int rihip_rank_topk_diverse(const double* scores, const int64_t* cand, const float* retrieval_scores, int64_t nq, int kc,
                            int k, const double* vec_tab, int64_t n_rows, int64_t ld, int col0, int w, double diversity,
                            int64_t* out_ids, double* out_scores, float* out_retrieval_scores, void* stream);

/* ---- seen-item exclusion ----------------------------------------------------------------------
 * Not in the reference, which serves and evaluates every retrieved candidate whether the user has rated it or not
 * (src/serving/recommender.py:269-387, src/pipelines/run_pipeline.py:166-220; SURVEY.md section 3.4, hazard ii).  Replaces the
 * host-side `[i for i in ids if i not in seen][:k]` after FAISSIndex.batch_search with a device stage.
 * scores f32 / ids i64 [nq, kc]: an over-fetched search result (item ids in descending score order, -1 / -inf only as a
 * tail).  The excluded ids are a CSR: seen_offsets i64 [n_seen_rows + 1] into seen_items i32, row u = the ids of user
 * u, ascending and unique.  Query q uses row user_ids[q] (device i64 [nq]; outside [0, n_seen_rows): nothing excluded);
 * user_ids NULL: row q (n_seen_rows >= nq).  Output row out_slot[q] (device int [nq]; NULL: row q) of out_scores f32 /
 * out_ids i64 [.., k] = the first k entries of the input row whose id is >= 0 and not in the list, in order, then
 * -1 / -inf.  deficit (device int, nullable; added to, never reset here) counts queries that produced fewer than k
 * entries although their input row had no -1 tail: kc was too small for them.  No host synchronisation, no allocation;
 * capturable in a hipGraph; deterministic. */
int rihip_exclude_topk(const float* scores, const int64_t* ids, int64_t nq, int kc, const int64_t* user_ids,
                       const int64_t* seen_offsets, int64_t n_seen_rows, const int32_t* seen_items, int k,
                       float* out_scores, int64_t* out_ids, const int* out_slot, int* deficit, void* stream);

/* ---- cold-start users: closed-form fold-in ------------------------------------------------------
 * Not in the reference, which answers a user without a trained row with _popularity_recommendations only
 * (src/serving/recommender.py:304-307, :393-410).  Gives such a user a query vector in the space the index searches
 * and the ranking-feature row the ranker reads, from a rating history, in one launch.
 * A cold user is a SLOT s in 0..nq-1 (not a user id).  Its history is row s of a CSR: hist_offsets i64 [nq + 1]
 * (ascending, inside [0, n_entries]; a row outside reads as empty) into hist_items i32 / hist_ratings i32 [n_entries]:
 * item ids ascending and unique inside a row (the convention of rihip_exclude_topk, so the row doubles as the slot's
 * exclusion list), ratings 1..5.
 * V f32 [n_rows, ldv >= d]: the item vectors as stored in the index, L2-normalised.  row_of i32 [n_ids]: item id -> row
 * of V, a value outside [0, n_rows) = not stored.  mu f64 [d]: the mean of the stored vectors.  min_rating 1..5 (4 =
 * the trainer's positive threshold).  weighting 0: w = 1; 1: w = r - (min_rating - 1).  beta in [0, 1].
 * Per slot:
 *   P = the entries with r >= min_rating, 0 <= item < n_ids and row_of[item] stored;  W = sum over P of w (an integer)
 *   m = (sum over P of w * V[row_of[item]]) / W - beta * mu, accumulated in f64;  n = sqrt(sum_c m_c^2)
 *   P empty or n < 1e-12: flags[s] = 1 and q[s] = 0;  otherwise flags[s] = 0 and q[s] = (float)(m / n).
 * beta = 1: the gradient at u = 0 of sum_p E_n log sigmoid(u.v_p - u.v_n) with uniform negatives is 1/2 sum_p (v_p - mu),
 * so q is the direction of one full-batch BPR step from the origin in tower-output space; beta = 0 is the plain mean
 * of the liked items.
 * rows f64 [nq, 24]: the slot's row in the user-table layout of rihip_rank_features_build, with the arithmetic of
 * rihip_ltr_stats / rihip_ltr_finalize (integer accumulators: order-independent, bit-exact).  Valid entries are those
 * with item >= 0 and a rating 1..5; cnt and sum run over all of them; row[0] = sum / cnt; row[1] =
 * (double)(float)log1p(cnt); genre preference: every entry with r >= 4 (the reference's constant, not min_rating) and
 * 0 < item < n_item_rows adds r - 3 to each genre g with item_tab[item, 5 + g] != 0 (item_tab f64 [n_item_rows, 23],
 * nullable with n_item_rows = 0) and counts towards L; v_g = acc_g / L (0 when L = 0), divided by its L2 norm (sum of
 * squares over g = 0..17 in order, each term a fused multiply-add) when that is > 0.  row[2..5] (recency, gender, age, occupation) = user_meta f64
 * [nq, 4], or 0.5, 0, 0.3, 0.3 when it is NULL.  cnt = 0: the full defaults row (3.5, 0, 0.5, 0, 0.3, 0.3, zeros).
 * err (device int, zeroed here, OR-ed): bit 0 = an item id < 0, bit 1 = a rating outside 1..5; such entries are
 * skipped everywhere, and no id is used as an address before it is range-checked.
 * 1 <= d <= 256; nq = 0 launches nothing; anything else out of range is RIHIP_ERR_ARG and nothing is launched.  One
 * launch, no host synchronisation, no allocation, no atomics but the error word: capturable in a hipGraph, and two
 * calls agree bit for bit. */
int rihip_fold_in_users(const int64_t* hist_offsets, const int32_t* hist_items, const int32_t* hist_ratings, int64_t nq,
                        int64_t n_entries, const float* V, int64_t n_rows, int64_t ldv, int d, const int32_t* row_of,
                        int64_t n_ids, const double* mu, int min_rating, int weighting, double beta,
                        const double* item_tab, int64_t n_item_rows, const double* user_meta, float* q, double* rows,
                        int* flags, int* err, void* stream);

/* ---- evaluation report ------------------------------------------------------------------------
 * Replaces the per-user loop of evaluate_model (src/evaluation/metrics.py:301-384) and the component functions it
 * calls: ndcg_at_k (:20-69, binary relevance), recall_at_k (:72-87), precision_at_k (:90-99), mrr (:104-118),
 * coverage (:143-165), intra_list_diversity (:168-190).  rec_ids device i64 [n, K] (K <= 16384), -1 = padding
 * anywhere in a row: a row means its entries >= 0, in order.  Ground truth as CSR: gt_offsets [n+1] into gt_items
 * (each row's segment sorted ascending, de-duplicated), gt_raw [n] = the row's list length with duplicates (IDCG);
 * gt_raw == 0 -> the user is not scored.  k_values: HOST array of n_k (1..64) values >= 0.  disc[i] = 1/log2(i+2)
 * and idcg[m] = disc[0] + ... + disc[m-1] (f64, n_tab > max k entries).  Outputs vals f64 [n, n_k, 3] (ndcg,
 * recall, precision), rr f64 [n] (reciprocal rank over the whole row), scored u8 [n].  With non-NULL flags
 * (u8 [n_id_space], zeroed here) the ids of scored rows are marked for coverage; an id >= n_id_space sets bit 0
 * of *err (device int, zeroed here). */
int rihip_eval_nparts(void);
int rihip_eval_topk(const int64_t* rec_ids, int64_t n, int K, const int64_t* gt_offsets, const int64_t* gt_items,
                    const int64_t* gt_raw, const int* k_values, int n_k, const double* disc, const double* idcg,
                    int n_tab, double* vals, double* rr, uint8_t* scored, uint8_t* flags, int64_t n_id_space, int* err,
                    void* stream);
/* intra_list_diversity of recs[:L] of every scored user: item_vectors device f32 [n_rows, g] (g <= 256),
 * item_present u8 [n_rows] (NULL = every row; ids >= n_rows have no vector); L <= 512.  div f64 [n]. */
int rihip_eval_diversity(const int64_t* rec_ids, int64_t n, int K, const uint8_t* scored, int L,
                         const float* item_vectors, int64_t n_rows, int g, const uint8_t* item_present, double* div,
                         void* stream);
/* Fixed-order f64 means over the scored users (no float atomics: bitwise reproducible).  div, flags, err nullable.
 * partials f64 [nparts, 3*n_k+3], cov_partials i64 [nparts] (workspace).  out f64 [3*n_k+5] = means of vals
 * (k-major), mean rr, mean div, n_scored, distinct flagged ids / catalog_size (0 if catalog_size <= 0), *err. */
int rihip_eval_reduce(int64_t n, int n_k, const double* vals, const double* rr, const double* div,
                      const uint8_t* scored, const uint8_t* flags, int64_t n_id_space, int64_t catalog_size,
                      const int* err, double* partials, int64_t* cov_partials, double* out, void* stream);

/* ---- validation by exact full-catalogue ranks ---------------------------------------------------
 * Not in the reference, which evaluates once, after training, from top-k lists.  For held-out (user, item) pairs: the
 * position each item would have in its user's exact list over the whole catalogue, without building a list.
 * U f32 [n_users, d], Y f32 [n_items, d]: tower outputs, any finite values (nothing relies on unit rows).  Pairs as a
 * CSR by user: pair_offsets i64 [n_users + 1] into pair_item i32 [n_pairs] = the target ROW of Y; a user may have no
 * pairs.  Optional exclusion CSR by the same user index: excl_offsets i64 [n_users + 1] (NULL: nothing excluded) into
 * excl_items i32 [n_excl], rows of Y, ascending and unique inside a row (the convention of rihip_exclude_topk).
 * For pair p = (u, t):
 *   s_uj = the f32 score of user u against item j from the owner sweep's product code (exact-f32 MFMA, fixed k order,
 *          s + 0.f: -0 and +0 are one score).  Every score that enters a comparison -- the target's, the swept ones,
 *          the excluded items' -- comes from that code, whose result for an element depends only on its two rows: a
 *          row compared with a bytewise equal row ties exactly.
 *   item j OUTRANKS t iff s_uj > s_ut, or s_uj == s_ut and j < t (score descending, row ascending: the tie rule of the
 *          exact index search)
 *   rank[p] = #{ j in [0, n_items) : j != t, j not in excl(u), j outranks t }: the 0-based position of t in u's exact
 *          top-n_items list with excl(u) removed.  An exclusion entry equal to t is ignored; other targets of the same
 *          user are ordinary competitors.
 *   target_score[p] = s_ut.
 * err (device int, zeroed here, OR-ed): bit 0 = an exclusion entry outside [0, n_items): ignored, never used as an
 * address; bit 1 = a target outside [0, n_items): rank[p] = -1, target_score[p] = 0.  Non-finite scores give
 * unspecified ranks inside [-1, n_items).
 * grid_splits: workgroups the item range is divided over, by whole 128-row tiles (0 = the library's choice, which fills
 * the chip at small n_pairs).  Counts are integers added with integer atomics: the result does not depend on the
 * split, and two calls agree bit for bit.
 * Limits: n_items < 2^31, n_pairs < 2^31, d a multiple of 16 up to 256.  workspace: device memory of
 * rihip_rank_targets_workspace_bytes(n_pairs, n_excl, d) bytes (-1 for sizes out of range), bounded in n_excl * d.
 * Argument errors return RIHIP_ERR_ARG with a reason and launch nothing; n_pairs == 0 zeroes err and launches nothing.
 * No host synchronisation, no allocation; capturable in a hipGraph. */
int64_t rihip_rank_targets_workspace_bytes(int64_t n_pairs, int64_t n_excl, int d);
int rihip_rank_targets(const float* U, int64_t n_users, const float* Y, int64_t n_items, int d,
                       const int64_t* pair_offsets, const int32_t* pair_item, int64_t n_pairs,
                       const int64_t* excl_offsets, const int32_t* excl_items, int64_t n_excl, int grid_splits,
                       int32_t* rank, float* target_score, int* err, void* workspace, int64_t workspace_bytes,
                       void* stream);
/* Ranks -> the per-user outputs of rihip_eval_topk: vals f64 [n_users, n_k, 3] (ndcg, recall, precision), rr f64
 * [n_users], scored u8 [n_users], from rank i32 [n_pairs] and the pairs' CSR.  Same k_values (HOST array, 1..64
 * values), disc / idcg tables (n_tab > max k) and per-k formulas; user u's hits are its pairs with 0 <= rank < k, its
 * DCG the sum of disc[rank] in ascending rank order (what the list kernel adds walking its row), recall = hits / its
 * pairs, rr = 1 / (1 + its smallest rank >= 0) over the whole catalogue.  gt_raw i64 [n_users] as in rihip_eval_topk
 * (NULL: the user's number of pairs).  rank -1 is a miss; a user without pairs or with gt_raw <= 0 is not scored.
 * rihip_eval_reduce then produces the means unchanged. */
int rihip_eval_ranks(const int32_t* rank, const int64_t* pair_offsets, int64_t n_users, int64_t n_pairs,
                     const int64_t* gt_raw, const int* k_values, int n_k, const double* disc, const double* idcg,
                     int n_tab, double* vals, double* rr, uint8_t* scored, void* stream);

/* ---- training-serving skew ------------------------------------------------------------------
 * Replaces the per-column loop of detect_training_serving_skew and the histograms of kl_divergence_bins
 * (src/evaluation/metrics.py:197-294) for two row-major device samples A [na, lda] and B [nb, ldb] (f32, or f64 when
 * *_f64 != 0).  Column c is cols_a[c] of A against cols_b[c] of B (device int32 [nc]; an index outside [0, ld) gives
 * status RIHIP_SKEW_BAD_COLUMN); ids_a / ids_b (device int64 [na] / [nb], nullable): a row whose id is < 0 is left out.
 * Per column, in f64: edges [nc, n_bins+1] = np.linspace(min, max, n_bins + 1) of the combined non-NaN range (bit for
 * bit), counts i64 [nc, 2, n_bins] = np.histogram of each sample on those edges (NaN never counted; zero when the
 * range is not finite or is a single value), valid i64 [nc, 2] = non-NaN values per sample, kl f64 [nc] = sum(p *
 * log(p / q)) of the densities + epsilon, normalised, status i32 [nc].  min_count: fewer non-NaN values on either side
 * -> RIHIP_SKEW_TOO_FEW (the detector's skip); propagate_nan != 0: any NaN -> kl nan (kl_divergence_bins on raw
 * input).  n_bins 1..128.  No host synchronisation; capturable in a hipGraph; bitwise repeatable (no float atomics). */
#define RIHIP_SKEW_OK 0
#define RIHIP_SKEW_CONSTANT 1     /* min == max: kl 0.0 */
#define RIHIP_SKEW_INFINITE 2     /* an infinite bound: kl nan */
#define RIHIP_SKEW_NAN 3          /* propagate_nan and a NaN in the input: kl nan */
#define RIHIP_SKEW_TOO_FEW 4      /* fewer than min_count values on a side: kl nan, the column is not checked */
#define RIHIP_SKEW_BAD_COLUMN 5   /* a column index outside its row: kl nan */
int64_t rihip_skew_workspace_bytes(int nc);
int rihip_skew_compute(const void* A, int a_f64, int64_t na, int64_t lda, const int* cols_a, const int64_t* ids_a,
                       const void* B, int b_f64, int64_t nb, int64_t ldb, const int* cols_b, const int64_t* ids_b,
                       int nc, int n_bins, double epsilon, int64_t min_count, int propagate_nan, void* workspace,
                       int64_t workspace_bytes, int64_t* counts, double* edges, int64_t* valid, double* kl,
                       int* status, void* stream);
/* Serving feature log (the "feature DataFrame from serving (recent requests)" that detect_training_serving_skew,
 * src/evaluation/metrics.py:234-260, compares against): appends the ranking-feature rows X f32 [n_rows, nf] of one
 * served batch (n_rows = nq * kc; row r belongs to user_ids[r / kc] and candidate cand_ids[r], -1 = padding) to the
 * device ring [R, nf] / ring_user [R] / ring_item [R] at slot (cursor[0] + r) % R, keeping the newest R rows of the
 * batch; then cursor[1] = cursor[0] (the batch's start) and cursor[0] += n_rows.  cursor: device int64 [2].
 * rewind: cursor[0] = cursor[1] (the batch is logged again, e.g. after the exactness re-do). */
int rihip_feature_log_append(const float* X, int64_t n_rows, int nf, const int64_t* user_ids, const int64_t* cand_ids,
                             int kc, float* ring, int64_t* ring_user, int64_t* ring_item, int64_t R, int64_t* cursor,
                             void* stream);
int rihip_feature_log_rewind(int64_t* cursor, void* stream);

/* ---- negative sampler -----------------------------------------------------------------------
 * Replaces UserItemDataset._sample_negative (src/training/train_embeddings.py:58-63) for a batch: neg_out[i] =
 * uniform draw from catalog[], re-drawn (up to max_attempts) while users[i]*key_stride + item is in the sorted
 * array rated_keys[] (one key per rating of any value, :48-50).  Counter-based draws keyed by (seed, i, attempt).
 * gave_up (device int, nullable) counts samples whose attempts were exhausted. */
int rihip_sample_negatives(const int64_t* users, int64_t n, const int64_t* catalog, int64_t n_catalog,
                           const int64_t* rated_keys, int64_t n_rated, int64_t key_stride, uint64_t seed,
                           int max_attempts, int64_t* neg_out, int* gave_up, void* stream);
/* rihip_sample_negatives_multi (not in the reference): K negatives per sample, uniform or proportional to item weights.
 * neg_out: [K n], k-major (negative k of sample i at k n + i).  One thread per output slot s = k n + i; attempt a draws
 *   r = splitmix64(splitmix64(seed ^ splitmix64(s)) + a),  column j = ((r >> 32) * n_catalog) >> 32,
 *   pick = j                                                      (alias_prob = alias_idx = NULL: uniform)
 *   pick = ((uint32_t)r < alias_prob[j]) ? j : alias_idx[j]       (Walker's alias method: two dependent reads per
 *                                                                  attempt where a search of the CDF would take twenty)
 * and the negative is catalog[pick], re-drawn while users[i] * key_stride + catalog[pick] is in rated_keys; after
 * max_attempts the slot keeps its last pick and adds one to *gave_up.  alias_prob u32 [n_catalog] (the probability of
 * keeping the column, in units of 2^-32: a column that is always kept holds any value with alias_idx[j] = j),
 * alias_idx i32 [n_catalog]; an alias_idx[j] outside [0, n_catalog) is read as j, so no table content makes the kernel
 * read out of bounds.  The K draws of a sample are independent (WITH replacement: a sample may hold the same negative
 * twice).  At K = 1 the slot is the sample, so K = 1 with a NULL table equals rihip_sample_negatives bit for bit.
 * RIHIP_ERR_ARG: as rihip_sample_negatives, plus K < 1, exactly one of the two table pointers NULL, a table with
 * n_catalog > 2^31 - 1, K n beyond one launch (256 (2^31 - 1) slots). */
int rihip_sample_negatives_multi(const int64_t* users, int64_t n, int K, const int64_t* catalog, int64_t n_catalog,
                                 const uint32_t* alias_prob, const int32_t* alias_idx, const int64_t* rated_keys,
                                 int64_t n_rated, int64_t key_stride, uint64_t seed, int max_attempts, int64_t* neg_out,
                                 int* gave_up, void* stream);

/* ---- LambdaMART training set from raw ratings ---------------------------------------------------
 * Replaces the pandas stages of FeatureEngineer (src/features/feature_engineering.py): build_user_features :91-166,
 * build_item_features :172-219, build_training_pairs :225-300 and build_interaction_features :306-370, i.e. what
 * RankerTrainer.run (src/training/train_ranker.py:45-137) does before LightGBMRanker.train.  All arrays are device
 * arrays.  Ratings: rating_user / rating_item i64 [R] (ids 1..n_users / 1..n_items), rating_value i32 [R] (1..5),
 * rating_ts i64 [R] (seconds), in any order, R < 2^31.  Metadata: user_meta f64 [n_users+1, 3] (gender_encoded,
 * age_normalized, occupation_normalized), item_meta f64 [n_items+1, 19] (year_normalized, 18 genre flags),
 * item_in_catalog u8 [n_items+1].  *err (device int, zeroed by stats and by join): bit 0 = a rating with an id out
 * of range, bit 1 = a rating outside 1..5 (such ratings are left out everywhere), bit 2 = a join pair with an id
 * outside its table (that row of X is zero).  grid_blocks: 0 = the library's launch geometry, > 0 = that many
 * workgroups (results never depend on it; for tests).
 *
 * rihip_ltr_widths: row widths of user_acc (24) / item_acc (3) and the length of totals (8).
 * rihip_ltr_stats (:104-108, :130-139, :183-187): integer accumulators, zeroed here.  user_acc i64 [n_users+1, 24] =
 *   count, rating sum, last timestamp (sign bit flipped), ratings >= 4, of those with a catalogue item, unused, 18
 *   sums of (rating-3)*genre; item_acc i64 [n_items+1, 3] = count, sum, sum of squares.
 * rihip_ltr_finalize (:110-121, :139-143, :188-193): the two tables in the layout of rihip_rank_features_build (user
 *   [n_users+1, 24], item [n_items+1, 23], f64; entities without ratings hold the serving defaults, whose
 *   log_rating_count is 0.0).  scratch: i64 [3] workspace.
 * rihip_ltr_plan (:248-262, :283-293): per-user buckets of rating positions (bucket_off i64 [n_users+2], bucket i32
 *   [R]: a user's ratings >= 4 first; cursor i32 [2, n_users+1] workspace), the candidate items (cand_index i32
 *   [n_items+1], cand_items i64 [n_items+1]: items with a rating, ascending), and per user: user_rows i32 = P_u + m_u with P_u = ratings >= 4,
 *   m_u = min(P_u * n_negatives, U_u), U_u = candidates the user never rated; 0 when P_u = 0 or U_u < n_negatives;
 *   query_id i32 (rank among kept users, -1 = dropped); row_start i64 (first row in [train rows | test rows], -1 =
 *   dropped); groups i32 [n_users+1]: rows per query in that same order.  n_test = max(1, int(n_queries *
 *   test_ratio)) whole queries are held out by a permutation keyed by seed.  totals i64 [8] = n_rows, n_queries,
 *   n_train_rows, n_train_queries, largest query, n_candidates, n_test_queries, 0.  At most 2^20 - 1 items.
 * rihip_ltr_emit (:264-280): a kept user's rows = its positives in (timestamp, input position) order (label 1, its
 *   rating) then m_u negatives (label 0, rating 0) drawn without replacement, uniformly, from the candidates the user
 *   never rated, by a permutation keyed by (seed, user id).  Outputs [n_rows]: out_user, out_item, out_query i64,
 *   out_label f32, out_rating i32.  n_rows must be totals[0] of the plan.
 * rihip_ltr_join (:306-370): X f32 [n_rows, nf] (nf <= 64) for flat (user, item) rows in TRAINING semantics:
 *   col_map as in rihip_rank_features_build; user_item_popularity_ratio in float32; a user / item without ratings
 *   (its row's log_rating_count is 0.0: the left merge finds nothing) gives 0.0 in its columns and in the
 *   interaction columns, as does NaN metadata. */
int rihip_ltr_widths(int* user_acc_width, int* item_acc_width, int* n_totals);
int rihip_ltr_stats(const int64_t* rating_user, const int64_t* rating_item, const int* rating_value,
                    const int64_t* rating_ts, int64_t n_ratings, int64_t n_users, int64_t n_items,
                    const double* item_meta, const uint8_t* item_in_catalog, int64_t* user_acc, int64_t* item_acc,
                    int* err, int grid_blocks, void* stream);
int rihip_ltr_finalize(const int64_t* user_acc, const int64_t* item_acc, const double* user_meta,
                       const double* item_meta, int64_t n_users, int64_t n_items, int64_t* scratch, double* user_tab,
                       double* item_tab, void* stream);
int rihip_ltr_plan(const int64_t* rating_user, const int64_t* rating_item, const int* rating_value, int64_t n_ratings,
                   const int64_t* user_acc, const int64_t* item_acc, int64_t n_users, int64_t n_items, int n_negatives,
                   double test_ratio, uint64_t seed, int64_t* bucket_off, int* bucket, int* cursor, int* cand_index,
                   int64_t* cand_items, int* user_rows, int* query_id, int64_t* row_start, int* groups, int64_t* totals,
                   int grid_blocks, void* stream);
int rihip_ltr_emit(const int64_t* rating_item, const int* rating_value, const int64_t* rating_ts,
                   const int64_t* user_acc, const int64_t* bucket_off, const int* bucket, const int* cand_index,
                   const int64_t* cand_items, const int* user_rows, const int* query_id, const int64_t* row_start,
                   const int64_t* totals, int64_t n_users, int64_t n_items, int64_t n_rows, uint64_t seed,
                   int64_t* out_user, int64_t* out_item, float* out_label, int* out_rating, int64_t* out_query,
                   int grid_blocks, void* stream);
int rihip_ltr_join(const double* user_tab, int64_t n_user_rows, const double* item_tab, int64_t n_item_rows,
                   const int64_t* user_ids, const int64_t* item_ids, int64_t n_rows, const int* col_map, int nf,
                   float* X, int* err, int grid_blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RECOMMENDIT_HIP_H */
