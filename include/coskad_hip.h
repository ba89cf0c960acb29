/* coskad_hip.h -- C ABI of the MI355X (gfx950) HIP library for COSKAD's STS-GCN hot path.
 *
 * The reference (aleflabo/COSKAD) has no FFI: the path is a chain of PyTorch ops inside
 * nn.Modules.  Each entry point below replaces the op chain of the reference lines it
 * cites; the Python host code in coskad_amd/ (torch.autograd.Functions / nn.Modules with
 * the reference's names) is the only caller.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - all tensors: device pointers, fp32, contiguous, layout [N, C, T, V] (T*V = "positions")
 *   - nothing is allocated, nothing synchronises; kernels are enqueued on `stream`
 *   - return 0 on success, negative COSKAD_ERR_* otherwise; text via coskad_last_error()
 *   - re-entrant; no global mutable state (last-error text is thread-local)
 */
#ifndef COSKAD_HIP_H
#define COSKAD_HIP_H
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

int coskad_abi_version(void);
const char* coskad_last_error(void);

/* Timing probe for benchmarks: after coskad_probe_begin(kernel, Ci, Co) every launch of that tile kernel
 * (1 = layer_apply, 2 = bwd_data, 3 = bwd_reduce, 4 = fwd_moments, 5 = gcn_params; 6 = ALL launches of one
 * coskad_layer_bwd*_f32 call together; 7 = the fused eval-mode encoder kernel) with those channel counts is bracketed by
 * HIP events on its launch stream; coskad_probe_end() waits for them and returns the average duration. */
int coskad_probe_begin(int kernel, int Ci, int Co);
int coskad_probe_stride(int n);   /* time every n-th matching launch only (default 1) */
int coskad_probe_end(float* avg_ms, int* launches);

/* ---- forward ------------------------------------------------------------------------ */

/* 1 for the (T, V) that have MIXING kernels only (csrc/gcn_window.hip): T in {8, 16, 24} x V in {14, 17, 18, 25}.  0 otherwise,
 * T = 12 -- the geometry of the tile kernels -- included.  coskad_gcn_f32, coskad_gcn_bwd_params_f32, coskad_gcn_bwd_params_dx_f32
 * and coskad_gcn_bwd_params_ws_bytes take these geometries; every other entry point with a (T, V) stays at T = 12, so a layer of
 * such a window length is composed from the mixing, coskad_gemm_f32 and the coskad_bn2_* kernels.  Host arithmetic. */
int coskad_window_ok(int T, int V);

/* ConvTemporalGraphical.forward (models/graph_layers/stsgcn.py:143-156) on rows = N*C rows
 * of T*V floats; adjoint != 0 applies the transposed operator (its backward w.r.t. X).
 * (T, V): T = 12 or coskad_window_ok; others fail with COSKAD_ERR_SHAPE ("unsupported ...") before the device is touched. */
int coskad_gcn_f32(const float* in, float* out, const float* A, const float* Tm, int rows, int T, int V,
                   int adjoint, hipStream_t stream);

/* BatchNorm2d statistics -> folded conv weights for one ST_GCNN_layer
 * (stsgcn.py:56-80: tcn = Conv1x1+BN, residual = Conv1x1+BN or Identity when Wr == NULL).
 * wfold: [2*Ci][CoP], bias: [CoP], CoP = Co rounded up to 16. */
int coskad_bn_fold_f32(const float* Wt, const float* bt, const float* gamma_t, const float* beta_t,
                       const float* mean_t, const float* var_t, const float* Wr, const float* br,
                       const float* gamma_r, const float* beta_r, const float* mean_r,
                       const float* var_r, float* wfold, float* bias, int Ci, int Co,
                       hipStream_t stream);

/* ST_GCNN_layer.forward (stsgcn.py:94-116) with folded BatchNorm:
 *   out = [PReLU_out]( Wz . gcn([PReLU_in] in) + Wx . [PReLU_in] in + b )
 * in_slope / out_slope: device pointers to the 1-element PReLU weight, or NULL to skip.
 * (T, V): T = 12, or a window length where coskad_layer_apply_window_ok(T, V, Ci, Co) holds: there the layer is one launch with one clip
 * per workgroup (csrc/eval_layer_clip.hip, which also serves T = 12 at 17 / 25 joints and those channels), `in` and `out` must be
 * 16-byte aligned at the window lengths 8 / 16 / 24 (COSKAD_ERR_ARG naming the pointer otherwise, before anything is launched; not asked
 * for at T = 12), wfold is [2*Ci][Co].  Other geometries fail with COSKAD_ERR_SHAPE ("unsupported ..."). */
int coskad_layer_apply_window_ok(int T, int V, int Ci, int Co);
int coskad_layer_apply_f32(const float* in, float* out, const float* A, const float* Tm,
                           const float* wfold, const float* bias, const float* in_slope,
                           const float* out_slope, int B, int Ci, int Co, int T, int V,
                           hipStream_t stream);

/* The TAIL of a decoder in eval mode (csrc/eval_tail_window.hip): the same layer with TWO output channels, one clip per workgroup
 * on a persistent grid, and -- in the same launch, without atomics -- the clip's reconstruction error against the target x [B, Co, T, V]:
 *   out [B, Co, T, V] = PReLU_out( Wz . gcn(PReLU_in in) + Wx . PReLU_in in + b )      (optional)
 *   score [B]         = mean over (c, t, v) of (out - x)^2                             (optional; needs x)
 * coskad_layer_tail_ok: 1 for T in {8, 12, 16, 24} x V in {17, 25} x Ci in {16, 32} x Co = 2, 0 otherwise (a set of its own: the other
 * `*_ok` predicates keep their answers).  coskad_layer_tail_max_grid: the persistent grid's cap (workgroups), 0 where not ok.
 * wfold [2*Ci][16], bias [16]: as coskad_bn_fold_f32 writes them for Co = 2.  At least one of out / score; `in`, `x`, `out` 16-byte
 * aligned (COSKAD_ERR_ARG naming the pointer), `score` 4-byte aligned; other shapes fail with COSKAD_ERR_SHAPE ("unsupported ...").
 * Every check runs before the device is touched.  A clip's results do not depend on B or on the workgroup that forms them. */
int coskad_layer_tail_ok(int T, int V, int Ci, int Co);
int coskad_layer_tail_max_grid(int T, int V, int Ci);
int coskad_layer_tail_f32(const float* in, const float* x, float* out, float* score,
                          const float* A, const float* Tm, const float* wfold, const float* bias,
                          const float* in_slope, const float* out_slope,
                          int B, int Ci, int Co, int T, int V, hipStream_t stream);

/* coskad_layer_tail_f32 with, from the same launch, the per-position map of the reconstruction error (one 16-byte store per thread,
 * no atomics, no further barrier):
 *   emap [B, T, V] = ((out_0 - x_0)^2 + (out_1 - x_1)^2) / (2 T V),     sum over (t, v) of emap[n] = score[n]
 * `score` is formed from the same differences by the same reduction: bit for bit what coskad_layer_tail_f32 stores.  The shape set
 * is coskad_layer_tail_ok's and the checks are coskad_layer_tail_f32's; beyond them x, score and emap are required and emap must be
 * 16-byte aligned (COSKAD_ERR_ARG naming the operand).  `out` stays optional.  A clip's map does not depend on B or on the workgroup
 * that forms it. */
int coskad_layer_tail_map_f32(const float* in, const float* x, float* out, float* score, float* emap,
                              const float* A, const float* Tm, const float* wfold, const float* bias,
                              const float* in_slope, const float* out_slope,
                              int B, int Ci, int Co, int T, int V, hipStream_t stream);

/* The ADJOINT of coskad_layer_apply_f32's folded layer (csrc/eval_layer_adj.hip): the gradient with respect to the layer's input of
 * whatever dU is the gradient of, one clip per workgroup on a persistent grid, no batch coupling:
 *   dIn [B, Ci, T, V] = PReLU_in'(in) (.) ( gcn^T(Wz^T . dU) + Wx^T . dU ),    dU [B, Co, T, V]
 * gcn^T: coskad_gcn_f32's adjoint.  wfold [2*Ci][Co]: exactly what coskad_bn_fold_f32 hands coskad_layer_apply_f32 (read transposed).
 * in_slope NULL (the network input): the mask is 1 and `in` is not read (may be NULL); otherwise PReLU' is 1 where in > 0 and
 * in_slope[0] elsewhere (an exact 0 gets the slope).
 * coskad_layer_input_grad_ok: 1 for T in {8, 12, 16, 24} x V in {17, 25} x Ci in {2, 16, 32} x Co in {16, 32, 64}, 0 otherwise (a set
 * of its own).  coskad_layer_input_grad_max_grid: the persistent grid's cap (workgroups) of that shape, 0 where not ok.
 * dU, dIn and (with in_slope) `in` non-NULL and 16-byte aligned: COSKAD_ERR_ARG naming the pointer otherwise, BEFORE the shape is
 * judged; other shapes fail with COSKAD_ERR_SHAPE ("unsupported ...").  Every check runs before the device is touched.  A clip's
 * result does not depend on B or on the workgroup that forms it. */
int coskad_layer_input_grad_ok(int T, int V, int Ci, int Co);
int coskad_layer_input_grad_max_grid(int T, int V, int Ci, int Co);
int coskad_layer_input_grad_f32(const float* dU, const float* in, float* dIn, const float* A, const float* Tm,
                                const float* wfold, const float* in_slope, int B, int Ci, int Co, int T, int V,
                                hipStream_t stream);

/* nn.PReLU() with one shared weight (stsgcn.py:82,110), elementwise, for API paths that must
 * materialise the post-activation tensor.  bwd: du = dout * PReLU'(u); dslope (+)= sum dout*u [u<0];
 * ws >= 1024 floats.  fwd moves 16-byte vectors: u and out must be 16-byte aligned (COSKAD_ERR_ARG naming the pointer otherwise,
 * before anything is launched). */
int coskad_prelu_fwd_f32(const float* u, const float* slope, float* out, size_t n, hipStream_t stream);
int coskad_prelu_bwd_f32(const float* u, const float* dout, const float* slope, float* du, float* dslope,
                         float* ws, int accumulate, size_t n, hipStream_t stream);

/* Reconstruction head of the decoder models: x_rec = PReLU_slope(U) (the last decoder layer's activation, stsgcn.py:110),
 * loss[0] = F.mse_loss(x_rec, x) (euclidean_autoencoder.py:111, spherical_vae.py:90); dU (optional) = upstream * dloss/dU,
 * dslope (optional, needs dU) (+)= upstream * dloss/dslope, xrec (optional) = the reconstruction.  ws: >= 2048 floats. */
int coskad_rec_head_f32(const float* U, const float* x, const float* slope, float* xrec, float* dU, float* loss, float* dslope,
                        float upstream, float* ws, int accumulate, size_t n, hipStream_t stream);

/* `rev_btlnk` of the decoder models (models/sts/ae.py:223-227: nn.Linear(latent_dim -> hidden * T * V)) and its autograd as
 * streaming kernels over the one large tensor (csrc/rev_btlnk.hip) at latent_dim L in {8, 16}, and as three fp32 MFMA GEMMs
 * (csrc/rev_btlnk_wide.hip) where coskad_rev_btlnk_wide_ok(N, L) holds: 16 < L <= 512; N % 4 == 0 at either; every other L fails
 * with COSKAD_ERR_SHAPE.  H 16-byte aligned (and dH at L in {8, 16}).
 *   fwd: H [B, N] = z [B, L] W^T + bias        (W [N, L])
 *   bwd: dz [B, L] (+)= dH W (dz_accumulate);  dW [N, L], db [N] (may be NULL) (+)= their batch sums (accumulate);
 *        ws: coskad_rev_btlnk_ws_floats(B, N, L) floats; two-stage fixed-order reductions (deterministic) */
size_t coskad_rev_btlnk_ws_floats(int B, int N, int L);
int coskad_rev_btlnk_wide_ok(int N, int L);
int coskad_rev_btlnk_fwd_f32(const float* z, const float* W, const float* bias, float* H, int B, int N, int L, hipStream_t stream);
int coskad_rev_btlnk_bwd_f32(const float* dH, const float* z, const float* W, float* dz, int dz_accumulate, float* dW, float* db,
                             int accumulate, float* ws, int B, int N, int L, hipStream_t stream);

/* ---- train-mode BatchNorm statistics -------------------------------------------------- */

/* Bytes of scratch `ws` that coskad_layer_train_stats_f32 needs for C_in = Ci. */
size_t coskad_train_stats_ws_bytes(int Ci);
/* Floats in the per-layer stat block saved for the backward pass. */
int coskad_stat_floats(int Ci, int Co);

/* Batch statistics of both BatchNorm2d of one ST_GCNN_layer in training mode
 * (stsgcn.py:65,76 via 106-108), from the moments of the conv inputs; writes the folded
 * weights for coskad_layer_apply_f32, the stat block for the backward pass, and updates
 * running_mean / running_var (unbiased) / num_batches_tracked in place (NULL to skip).
 * Wr == NULL: identity residual (stsgcn.py:79-80). */
int coskad_layer_train_stats_f32(const float* in, const float* A, const float* Tm, const float* in_slope,
                                 const float* Wt, const float* bt, const float* gamma_t,
                                 const float* beta_t, float* rmean_t, float* rvar_t, long long* nbt_t,
                                 const float* Wr, const float* br, const float* gamma_r,
                                 const float* beta_r, float* rmean_r, float* rvar_r, long long* nbt_r,
                                 float momentum, float* wfold, float* bias, float* stat, void* ws,
                                 size_t ws_bytes, int B, int Ci, int Co, int T, int V,
                                 hipStream_t stream);

/* 1 when a (Ci -> Co) ST_GCNN layer of window length T (8, 16, 24) trains on the stored-Z layer kernels (statistics pass, apply,
 * backward); 0 otherwise, T = 12 included (the tile kernels' own geometry).  Host arithmetic.
 * Holds for T in {8, 16, 24} x V in {17, 25} x Ci in {2, 16, 32} x Co in {16, 32, 64} (csrc/train_window_moments.hip,
 * csrc/train_window_flat.hip, csrc/gcn_window.hip).  Where it holds, coskad_layer_train_stats_z_f32, coskad_layer_train_stats_f32,
 * coskad_layer_apply_z_f32, coskad_layer_bwd_z_f32, coskad_layer_bwd_chain_f32, coskad_layer_bwd_stats_f32 and
 * coskad_layer_bwd_ws_bytes serve the layer with the contracts stated for T = 12 (the backward needs the stored Z; `below_*` is
 * refused; coskad_layer_bwd_below_rows is 0); coskad_layer_train_moments_f32 serves every such (T, V, Ci).
 * Alignment at EVERY window geometry of coskad_window_ok: the activation pointers of these entry points (`in`, `Z`, `dU`, `dIn`, `out`)
 * must be 16-byte aligned -- rows are staged as 16-byte vectors -- else COSKAD_ERR_ARG naming the pointer, before anything is launched
 * and before the shape is judged.  Parameters, gradients and tables need 4-byte alignment only. */
int coskad_layer_train_window_ok(int T, int V, int Ci, int Co);

/* 1 when a FEW-CHANNEL (Ci -> Co) layer of window length T trains on the same entry points: exactly T in {8, 16, 24} x V in {17, 25} x
 * (Ci, Co) = (4, 2), the virtual layer a stack's last (C -> 2) layer runs as by commutation; 0 for everything else (T = 12, V = 14 / 18,
 * (6, 3), ...).  A set of its own: coskad_layer_train_window_ok is unchanged and stays 0 there.  Where either predicate holds the entry
 * points listed above serve the layer, with the same alignment rule; coskad_layer_train_moments_f32 serves Ci = 4 as well. */
int coskad_layer_train_window_narrow_ok(int T, int V, int Ci, int Co);

/* Stored-Z variant of the training forward: the statistics pass also writes Z = gcn(PReLU(in)) [B,Ci,T,V]; the layer
 * is then a streaming GEMM over Z and `in` (no staging, no mixing recompute), and the backward reads Z as well.
 * (T, V): T = 12, or a window geometry where coskad_layer_train_window_ok holds (see there for the alignment rule). */
int coskad_layer_train_stats_z_f32(const float* in, const float* A, const float* Tm, const float* in_slope,
                                   const float* Wt, const float* bt, const float* gamma_t,
                                   const float* beta_t, float* rmean_t, float* rvar_t, long long* nbt_t,
                                   const float* Wr, const float* br, const float* gamma_r,
                                   const float* beta_r, float* rmean_r, float* rvar_r, long long* nbt_r,
                                   float momentum, float* wfold, float* bias, float* stat, void* ws,
                                   size_t ws_bytes, int B, int Ci, int Co, int T, int V,
                                   hipStream_t stream, float* Z);
/* U = Wz Z + Wx PReLU_in(in) + b from the stored Z.  (T, V): T = 12, or a window geometry of coskad_layer_train_window_ok -- see its comment for the set and the 16-byte alignment of the activation pointers: at EVERY window length 8 / 16 / 24
 * (coskad_window_ok), the few-channel first-layer route and geometries no kernel serves included, a misaligned `Z`, `in` or `out` is
 * COSKAD_ERR_ARG naming the pointer (those routes load 16-byte vectors too), before the shape is judged. */
int coskad_layer_apply_z_f32(const float* Z, const float* in, float* out, const float* A, const float* Tm,
                             const float* wfold, const float* bias, const float* in_slope, const float* out_slope,
                             int B, int Ci, int Co, int T, int V, hipStream_t stream);

/* ---- training forward with the NEXT layer's statistics fused into the apply kernel (csrc/fused_apply_next.hip) --------
 * Layer i's apply holds a clip's whole U_i on chip; for T = 12, V = 17, C_in in {2, 16, 32}, C_out in {16, 32} it also forms
 * X_{i+1} = PReLU_i(U_i), Z_{i+1} = gcn_{i+1}(X_{i+1}) (stsgcn.py:154-155 of the next layer) and the moment partials
 * [sum x x^T | sum x | sum z z^T | sum z] that layer i+1's BatchNorms need (stsgcn.py:65,76), so the statistics pass of
 * layer i+1 (coskad_layer_train_stats_z_f32's first kernel) and its re-read of U_i disappear.
 *   coskad_build_ftab_f32       : forward mixing tables (coskad_ftab_floats() floats each) of n <= 4 layers from their A / T
 *                                 (host arrays of n device pointers), one launch
 *   coskad_layer_apply_next_f32 : out = U_i [B,Co,T,V]; Z_next [B,Co,T,V]; partials [coskad_layer_apply_next_rows(B, Ci, Co)][2 (Co^2 + Co)]
 *   coskad_layer_train_fold_f32 : the rest of coskad_layer_train_stats_f32 for layer i+1 (fp64 sums of the partial rows, statistics,
 *                                 folded weights, stat block, running-stat update); ws >= coskad_train_stats_ws_bytes(Ci). */
int coskad_layer_apply_next_ok(int Ci, int Co, int T, int V);
int coskad_ftab_floats(void);
int coskad_layer_apply_next_rows(int B, int Ci, int Co);
int coskad_build_ftab_f32(const float* const* A, const float* const* Tm, float* const* tab, int n, int T, int V,
                          hipStream_t stream);
/* coskad_layer_train_stats_z_f32 of a stack's first layer (C_in <= 4, Z stored, T = 12, V = 17) with the tables of
 * coskad_build_ftab_f32 (ntab <= 4 layers: tab[i] from tab_A[i], tab_Tm[i]) built by extra blocks of the statistics pass's launch:
 * the moments depend on the clips only, the tables on parameters only, so neither waits for the other and one launch leaves the step. */
int coskad_layer_train_stats_z_ftab_f32(const float* in, const float* A, const float* Tm, const float* in_slope,
                                        const float* Wt, const float* bt, const float* gamma_t,
                                        const float* beta_t, float* rmean_t, float* rvar_t, long long* nbt_t,
                                        const float* Wr, const float* br, const float* gamma_r,
                                        const float* beta_r, float* rmean_r, float* rvar_r, long long* nbt_r,
                                        float momentum, float* wfold, float* bias, float* stat, void* ws,
                                        size_t ws_bytes, int B, int Ci, int Co, int T, int V,
                                        hipStream_t stream, float* Z, const float* const* tab_A, const float* const* tab_Tm,
                                        float* const* tab, int ntab);

int coskad_layer_apply_next_f32(const float* Z, const float* in, float* out, const float* wfold, const float* bias,
                                const float* in_slope, const float* out_slope, const float* ftab_next, float* Z_next,
                                float* partials, size_t partials_bytes, int B, int Ci, int Co, int T, int V,
                                hipStream_t stream);
int coskad_layer_train_fold_f32(const float* partials, int rows, const float* Wt, const float* bt, const float* gamma_t,
                                const float* beta_t, float* rmean_t, float* rvar_t, long long* nbt_t,
                                const float* Wr, const float* br, const float* gamma_r,
                                const float* beta_r, float* rmean_r, float* rvar_r, long long* nbt_r,
                                float momentum, float* wfold, float* bias, float* stat, void* ws,
                                size_t ws_bytes, int B, int Ci, int Co, int T, int V, hipStream_t stream);

/* ---- fused eval-mode encoder (models/common/components.py:94-105 in one kernel) ------------------------------
 * Built for the reference's default geometry: n_frames 12, n_joints 17, channels 2-32-16-32-64.
 * coskad_gather_f32 : out[i] = idx[i] >= 0 ? src[idx[i]] : 0 -- builds the operand streams (coskad_amd/fused_plan.py
 *                     holds the index maps) from the concatenated A / T / folded-weight / bias / bottleneck tensors.
 * x     [B,2,12,17]; tab, wreg: operand streams; slopes[4]: the PReLU weights of the four layers;
 * out   [B][coskad_fused_encoder_out_floats()]: PReLU(last layer) in tile-major order, zero in the padding columns:
 *       the bottleneck (coskad_btlnk_fwd_f32 with slope NULL) reads it with the weight permuted the same way. */
int coskad_gather_f32(const float* src, const int* idx, float* out, size_t n, hipStream_t stream);
int coskad_fused_encoder_out_floats(void);
int coskad_fused_encoder_f32(const float* x, float* out, const float* tab, const float* wreg, const float* slopes, int B,
                             int T, int V, hipStream_t stream);

/* ---- strided batched fp32 GEMM (plain-GCN encoders: learnable_gcn.py:65-72, gcn.py:48-54; 1x1 convs of wide layers) ----
 * C[b][m][n] = act(sum_k A[b][m][k] B[b][k][n] + bias), every operand addressed by element strides (s?_b may be 0).
 * bias_mode: 0 none, 1 bias[m % bias_mod], 2 bias[n];  relu != 0: max(., 0).
 * reduce != 0: C receives partial sums [ceil(batch / chunk)][M][N] (contiguous) over the batches of each chunk -- sum them
 *              with coskad_gemm_sum_f32 (fp64, fixed order).  ktotal > 0: element (b, k) exists iff b*K + k < ktotal.
 * accum != 0 (reduce == 0): C += the product (after bias / ReLU). */
int coskad_gemm_f32(const float* A, const float* B, float* C, const float* bias, long long sa_b, long long sa_m,
                    long long sa_k, long long sb_b, long long sb_k, long long sb_n, long long sc_b, long long sc_m,
                    long long sc_n, int M, int N, int K, int batch, int bias_mode, int bias_mod, int relu, int reduce,
                    int chunk, long long ktotal, int accum, hipStream_t stream);
int coskad_gemm_sum_f32(const float* partials, int chunks, size_t E, float* out, int accumulate, hipStream_t stream);
/* g = dout * (out > 0) on [Nb, C, P]; part [slices][C]: per-slice channel sums of g (bias gradient partials) */
int coskad_relu_bwd_f32(const float* out, const float* dout, float* g, float* part, int Nb, int C, int P, int slices,
                        hipStream_t stream);
/* row softmax of an n x n matrix (nn.Softmax() on the 2-D learnable adjacency, learnable_gcn.py:36,66) and its backward */
int coskad_softmax_rows_f32(const float* x, float* y, int n, hipStream_t stream);
int coskad_softmax_rows_bwd_f32(const float* y, const float* dy, float* dx, int n, hipStream_t stream);

/* ---- fused plain-GCN layer (learnable_gcn.py:54-72, gcn.py:48-54 + ReLU; csrc/plain_gcn.hip) ------------------------------------
 * O[b] = relu(W^T . X[b] . A'^T + bias): X [B][Ci][P], W [Ci][Co], A' [P][P] (softmax of the learnable adjacency, or the fixed
 * graph), bias [Co] or NULL, O [B][Co][P]; one launch, the narrow-side intermediate stays on chip.  The mixing runs on
 * min(Ci, Co) channels: Y = X . A'^T first when Ci <= Co, H = W^T . X first otherwise.
 * coskad_plain_gcn_ok: 1 <= Ci, Co <= 64 and P in {168, 204, 216, 300} (12 frames x 14 / 17 / 18 / 25 joints); other shapes fail
 *   with COSKAD_ERR_SHAPE ("unsupported ...") before the device is touched -- compose them from coskad_gemm_f32.  Host arithmetic.
 * save (optional): receives that intermediate, Y [B][Ci][P] or H [B][Co][P].  The backward needs Y (Ci <= Co) always and H
 *   (Ci > Co) only for the adjacency gradient.
 * grid_cap: upper bound of the persistent grid, 0 = the kernels' default.
 * Backward: G = dO * (O > 0) formed on load; dW [Ci][Co] and db [Co] (NULL: no bias) (+)= (accumulate) fixed-order fp64 sums of one
 *   partial row per workgroup in ws (coskad_plain_gcn_ws_bytes) -- bitwise reproducible; dX [B][Ci][P] iff need_dx; need_da: D
 *   receives the narrow-side gradient, dY [B][Ci][P] (Ci <= Co; then dA'[q][p] = sum_rows D[r][q] X[r][p]) or G [B][Co][P]
 *   (Ci > Co; dA'[q][p] = sum_rows G[r][q] H[r][p]) for a coskad_gemm_f32 reduction.  S: the saved Y (Ci <= Co; otherwise unused,
 *   may be NULL); X is read only when Ci > Co.  X, S, O, dO, D, A' 16-byte aligned. */
int coskad_plain_gcn_ok(int Ci, int Co, int P);
size_t coskad_plain_gcn_ws_bytes(int B, int Ci, int Co, int P, int grid_cap);
int coskad_plain_gcn_fwd_f32(const float* X, const float* W, const float* Ap, const float* bias, float* O, float* save, int B,
                             int Ci, int Co, int P, int grid_cap, hipStream_t stream);
int coskad_plain_gcn_bwd_f32(const float* X, const float* S, const float* O, const float* dO, const float* W, const float* Ap,
                             float* dX, float* dW, float* db, float* D, void* ws, size_t ws_bytes, int B, int Ci, int Co, int P,
                             int need_dx, int need_da, int accumulate, int grid_cap, hipStream_t stream);

/* ---- 1x1 convolution in NCHW for wide layers (nn.Conv2d(C_in, C_out, 1) of stsgcn.py:57-63,71-75; csrc/conv1x1.hip) -----------
 * Out[b][m][p] (+)= sum_k A(m,k) In[b][k][p] (+ bias[m]) with In [batch][K][P], Out [batch][M][P] contiguous; A(m,k) = A[m sa_m + k sa_k],
 * sa_k == 1 (forward: W [M][K]) or sa_m == 1 (data gradient: W^T of W [K][M]).  Layout-specialised MFMA kernel (float4 loads, K tiles
 * double-buffered through registers, 16-byte stores) for P in {204, 300}, K % 16 == 0, M % 32 == 0 (coskad_conv1x1_ok); other shapes:
 * coskad_gemm_f32.  stats (optional): [coskad_conv1x1_stat_rows()][M][2] doubles receive the per-channel sum / sum of squares of Out --
 * the train-mode BatchNorm statistics without another pass over the tensor; coskad_bn2_stats_parts_f32 turns them into
 * stat [2C] = (mean, 1 / sqrt(var + eps)) and updates the running statistics like coskad_bn2_stats_f32. */
int coskad_conv1x1_ok(int M, int K, int P);
int coskad_conv1x1_stat_rows(int M, int K, int P, int batch);
int coskad_conv1x1_f32(const float* A, long long sa_m, long long sa_k, const float* In, float* Out, const float* bias, double* stats,
                       int M, int K, int P, int batch, int accumulate, hipStream_t stream);
int coskad_bn2_stats_parts_f32(const double* parts, int rows, float* stat, float* running_mean, float* running_var,
                               long long* num_batches_tracked, float momentum, float eps, double count, int C, hipStream_t stream);
/* weight gradient of the 1x1 convolution: partials [ceil(batch / chunk)][M][K] of dW[m][k] = sum_b sum_p G[b][m][p] X[b][k][p]
 * (G = gradient of the conv output [batch][M][P], X = conv input [batch][K][P]); P in {204, 300}, M a multiple of 32, K of 64
 * (coskad_conv1x1_wgrad_ok); sum the partials with coskad_gemm_sum_f32 (fp64, fixed order: deterministic) */
int coskad_conv1x1_wgrad_ok(int M, int K, int P);
int coskad_conv1x1_wgrad_f32(const float* G, const float* X, float* partials, int M, int K, int P, int batch, int chunk,
                             hipStream_t stream);

/* ---- BatchNorm2d + residual add + PReLU of an ST_GCNN layer on [Nb, C, P] tensors (stsgcn.py:56-80,106-110), for layers
 * beyond the LDS-resident tile kernels (their 1x1 convolutions are coskad_gemm_f32, their mixing coskad_gcn_f32).
 * stat [2C] = (mean, 1/sqrt(var + eps)); stat_r == NULL: identity residual.  ws: coskad_bn2_ws_bytes / _bwd_ws_bytes. */
size_t coskad_bn2_ws_bytes(int Nb, int C);
size_t coskad_bn2_bwd_ws_bytes(int Nb, int C);
int coskad_bn2_stats_f32(const float* x, float* stat, float* running_mean, float* running_var, long long* num_batches_tracked,
                         float momentum, float eps, int training, void* ws, size_t ws_bytes, int Nb, int C, int P,
                         hipStream_t stream);
int coskad_bn2_apply_prelu_f32(const float* Ct, const float* Cr, const float* stat_t, const float* gamma_t, const float* beta_t,
                               const float* stat_r, const float* gamma_r, const float* beta_r, const float* slope, float* out,
                               int Nb, int C, int P, hipStream_t stream, float drop_p, unsigned long long drop_seed);
int coskad_bn2_bwd_f32(const float* Ct, const float* Cr, const float* dOut, const float* stat_t, const float* gamma_t,
                       const float* beta_t, const float* stat_r, const float* gamma_r, const float* beta_r, const float* slope,
                       float* dCt, float* dCr, float* dgamma_t, float* dbeta_t, float* dgamma_r, float* dbeta_r, float* dslope,
                       int training, void* ws, size_t ws_bytes, int Nb, int C, int P, hipStream_t stream, float drop_p,
                       unsigned long long drop_seed);
/* Train-mode nn.Dropout(p) of the tcn branch (stsgcn.py:66, between BatchNorm and the residual add) in the two calls above:
 * drop_p in [0, 1) and a seed; element i of the [Nb, C, P] tensor is kept (and scaled by 1 / (1 - p)) iff a counter-based hash
 * of (seed, i) says so -- the backward recomputes the mask from the same seed, nothing is stored.  drop_p = 0: no dropout.
 * coskad_dropout_mask_f32 writes that mask (values 0 or 1 / (1 - p)) for tests / oracles. */
int coskad_dropout_mask_f32(float* out, size_t n, float drop_p, unsigned long long drop_seed, hipStream_t stream);

/* ---- `mlp` projector tail (models/common/components.py:209-226 behind its first Linear, which runs on the bottleneck
 * kernels): z = W2 . relu(BatchNorm1d(y1)) + b2 on y1 [B, H]; H, L <= 64.
 * forward : training != 0 -> batch statistics (biased variance normalises, running_mean / running_var (unbiased) and
 *           num_batches_tracked are updated in place; they may be NULL), else the running statistics.
 *           stat [0:2H] receives (mean, 1/sqrt(var + eps)) for the backward; the buffer holds coskad_mlp_head_ws_floats(B,H,L)
 *           floats (behind the 2H values: the per-block partial sums of the hidden, out <= 16 kernels).
 * backward: dy1 [B,H], dgamma, dbeta [H], dW2 [L,H], db2 [L] (may be NULL); red: coskad_mlp_head_ws_floats(B,H,L) floats of
 *           scratch; accumulate != 0 adds into the parameter gradients. */
size_t coskad_mlp_head_ws_floats(int B, int H, int L);   /* floats of `stat` (forward) and of `red` (backward), 8-byte aligned */
int coskad_mlp_head_fwd_f32(const float* y1, const float* gamma, const float* beta, float* running_mean,
                            float* running_var, long long* num_batches_tracked, float momentum, float eps, int training,
                            const float* W2, const float* b2, float* z, float* stat, int B, int H, int L,
                            hipStream_t stream);
int coskad_mlp_head_bwd_f32(const float* y1, const float* stat, const float* gamma, const float* beta, const float* W2,
                            const float* dz, float* dy1, float* dgamma, float* dbeta, float* dW2, float* db2, float* red,
                            int training, int accumulate, int B, int H, int L, hipStream_t stream);

/* ---- backward of one ST_GCNN_layer (autograd of stsgcn.py:94-116 in training mode) ------ */

/* (window geometries of coskad_layer_train_window_ok: what that route needs -- one more [B, Ci, T, V] buffer than at T = 12) */
size_t coskad_layer_bwd_ws_bytes(int B, int Ci, int Co, int T, int V);

/* 1 when one clip of a (Ci -> Co) ST_GCNN layer fits the LDS-resident tile kernels (forward, statistics, backward);
 * 0 otherwise (more than 64 channels, or 64 input channels on the 25-joint layout): callers then compose the layer
 * from coskad_gcn_f32 + GEMMs. */
int coskad_layer_fits(int Ci, int Co, int T, int V);

/* coskad_layer_bwd_z_f32 inside a chain of layers (reference: autograd walks stsgcn.py:94-116 layer by layer, last to first).
 * Stage 1 of a layer's backward (the batch reductions P = sum dU.Z^T, Q = sum dU.X^T, sdU) reads the dU the layer ABOVE has
 * just produced; where that layer's data kernel holds it on chip, it forms the reductions itself:
 *   stats_in, stats_in_rows                : this layer's chain buffer, filled by the call for the layer above (NULL: stage 1 runs
 *                                            here, as in coskad_layer_bwd_z_f32)
 *   below_in, below_Z [B,below_Ci,T,V]     : input of the layer below as stored (pre-activation; below_in_slope = its producer's
 *                                            PReLU weight, NULL for the raw network input) and its stored Z
 *   below_stats [coskad_layer_bwd_below_floats(B,Ci,Co,below_Ci,T,V) floats, 8-byte aligned] : ITS chain buffer (NULL: not formed):
 *       coskad_layer_bwd_below_rows(...) partial rows of 2 Ci below_Ci + Ci floats, then their fp64 sums (formed by this call's
 *       partial-sum launch: the layer below runs neither its batch reductions nor their summation)
 * coskad_layer_bwd_below_rows returns 0 when the (Ci -> Co) data kernel cannot form them (built at T = 12, V = 17: 32 -> 16 above
 * a 2-channel layer, 16 -> 32 above a 32-channel layer, 32 -> 64 above a 16-channel layer: the default stack). */
int coskad_layer_bwd_below_rows(int B, int Ci, int Co, int below_Ci, int T, int V);
size_t coskad_layer_bwd_below_floats(int B, int Ci, int Co, int below_Ci, int T, int V);
/* (T, V): T = 12, or a window geometry of coskad_layer_train_window_ok -- see its comment for the set and the 16-byte alignment of the activation pointers (`in`, `Z`, `dU`, `dIn`); there `below_*` is refused. */
int coskad_layer_bwd_chain_f32(const float* in, const float* dU, const float* A, const float* Tm,
                               const float* in_slope, const float* stat, const float* Wt, const float* gamma_t,
                               const float* Wr, const float* gamma_r, float* dIn, float* dA, float* dT, float* dWt,
                               float* dbt, float* dgamma_t, float* dbeta_t, float* dWr, float* dbr,
                               float* dgamma_r, float* dbeta_r, float* dslope_in, void* ws, size_t ws_bytes,
                               int accumulate, int B, int Ci, int Co, int T, int V, hipStream_t stream, const float* Z,
                               const float* stats_in, int stats_in_rows, size_t stats_in_bytes, const float* below_in,
                               const float* below_Z, const float* below_in_slope, int below_Ci, float* below_stats,
                               size_t below_stats_bytes, double stats_count);

/* ---- SyncBN (optional: the reference trains with per-rank BatchNorm statistics, train_COSKAD.py:75-78) -------------
 * The batch reductions and the folds behind them as separate calls, so that a data-parallel caller can add the other ranks'
 * fp64 sums (one small all-reduce per BatchNorm boundary) in between.  Forward: coskad_layer_train_moments_f32 (a layer with its own
 * statistics pass) or coskad_layer_moment_sums_f32 (moment partials from coskad_layer_apply_next_f32) -> sums [2 (Ci^2 + Ci)]
 * doubles: [sum xx^T][sum x][sum zz^T][sum z] -> all-reduce -> coskad_layer_train_fold_sums_f32 with count = global clips x T x V.
 * Backward: coskad_layer_bwd_stats_f32 (stage 1 alone, into a chain buffer: rows, then sums at coskad_layer_bwd_sums_offset floats)
 * or the chain buffer the layer above filled -> all-reduce the sums in place -> coskad_layer_bwd_chain_f32 with stats_in and
 * stats_count = global clips x T x V (0: this batch). */
/* coskad_layer_train_moments_f32, coskad_layer_bwd_stats_f32 -- (T, V): T = 12, or the window lengths 8 / 16 / 24 at 17 / 25 joints with
 * Ci in {2, 4, 16, 32} (and, for the backward's stage 1, coskad_layer_train_window_ok or _narrow_ok(T, V, Ci, Co)); activation pointers (`in`, `Z`, `dU`)
 * 16-byte aligned there, as coskad_layer_train_window_ok's comment states. */
int coskad_layer_train_moments_f32(const float* in, const float* A, const float* Tm, const float* in_slope, float* Z, double* sums,
                                   void* ws, size_t ws_bytes, int B, int Ci, int T, int V, hipStream_t stream);
int coskad_layer_moment_sums_f32(const float* partials, int rows, int Ci, double* sums, hipStream_t stream);
int coskad_layer_train_fold_sums_f32(const double* sums, double count, const float* Wt, const float* bt, const float* gamma_t,
                                     const float* beta_t, float* rmean_t, float* rvar_t, long long* nbt_t,
                                     const float* Wr, const float* br, const float* gamma_r,
                                     const float* beta_r, float* rmean_r, float* rvar_r, long long* nbt_r,
                                     float momentum, float* wfold, float* bias, float* stat, int Ci, int Co, hipStream_t stream);
size_t coskad_layer_bwd_stats_floats(int B, int Ci, int Co, int T, int V);
size_t coskad_layer_bwd_sums_offset(int rows, int Ci, int Co);
int coskad_layer_bwd_stats_f32(const float* in, const float* dU, const float* A, const float* Tm, const float* in_slope,
                               int has_residual, float* stats_out, size_t stats_out_bytes, int* rows_out, void* ws, size_t ws_bytes,
                               int B, int Ci, int Co, int T, int V, hipStream_t stream, const float* Z);

/* in   : the layer's input as stored by the producer (pre-activation; in_slope = its PReLU weight,
 *        NULL when `in` is the raw network input)
 * dU   : gradient w.r.t. this layer's pre-activation output [B,Co,T,V]
 * stat : stat block written by coskad_layer_train_stats_f32 in the forward pass
 * dIn  : gradient w.r.t. `in` (already multiplied by the producer's PReLU derivative); NULL to skip
 * dslope_in : gradient of the producer's PReLU weight (1 float); NULL to skip
 * parameter gradients are written (accumulate == 0) or added (accumulate != 0).
 * Wr == NULL: identity residual. */
int coskad_layer_bwd_f32(const float* in, const float* dU, const float* A, const float* Tm,
                         const float* in_slope, const float* stat, const float* Wt, const float* gamma_t,
                         const float* Wr, const float* gamma_r, float* dIn, float* dA, float* dT, float* dWt,
                         float* dbt, float* dgamma_t, float* dbeta_t, float* dWr, float* dbr,
                         float* dgamma_r, float* dbeta_r, float* dslope_in, void* ws, size_t ws_bytes,
                         int accumulate, int B, int Ci, int Co, int T, int V, hipStream_t stream);

/* coskad_layer_bwd_f32 reading the stored Z = gcn(PReLU(in)) of coskad_layer_train_stats_z_f32 instead of recomputing
 * the mixing in its reduction and data kernels (Z == NULL: identical to coskad_layer_bwd_f32). */
/* (T, V): T = 12, or a window geometry of coskad_layer_train_window_ok -- see its comment for the set and the 16-byte alignment of the activation pointers (`in`, `Z`, `dU`, `dIn`);
 * there Z must be given. */
int coskad_layer_bwd_z_f32(const float* in, const float* dU, const float* A, const float* Tm,
                           const float* in_slope, const float* stat, const float* Wt, const float* gamma_t,
                           const float* Wr, const float* gamma_r, float* dIn, float* dA, float* dT, float* dWt,
                           float* dbt, float* dgamma_t, float* dbeta_t, float* dWr, float* dbr,
                           float* dgamma_r, float* dbeta_r, float* dslope_in, void* ws, size_t ws_bytes,
                           int accumulate, int B, int Ci, int Co, int T, int V, hipStream_t stream, const float* Z);

/* The same backward split in two calls, so that stage 4 (dA, dT; independent of the rest of the chain) can be enqueued
 * on a second stream: coskad_layer_bwd_data_f32 = batch reductions + fold + data path, with the mixing-output gradient
 * dZ [B,Ci,T,V] written to the caller's buffer; coskad_layer_gcn_params_f32 = dA, dT from `in` and that dZ. */
int coskad_layer_bwd_data_f32(const float* in, const float* dU, const float* A, const float* Tm,
                              const float* in_slope, const float* stat, const float* Wt, const float* gamma_t,
                              const float* Wr, const float* gamma_r, float* dIn, float* dZ, float* dWt, float* dbt,
                              float* dgamma_t, float* dbeta_t, float* dWr, float* dbr, float* dgamma_r,
                              float* dbeta_r, float* dslope_in, void* ws, size_t ws_bytes, int accumulate, int B,
                              int Ci, int Co, int T, int V, hipStream_t stream, const float* Z /* stored gcn(in) or NULL */);
size_t coskad_layer_gcn_params_ws_bytes(int T, int V);
int coskad_layer_gcn_params_f32(const float* in, const float* in_slope, const float* dZ, const float* A,
                                const float* Tm, float* dA, float* dT, void* ws, size_t ws_bytes, int accumulate,
                                int B, int Ci, int T, int V, hipStream_t stream);

/* Parameter gradients of ConvTemporalGraphical alone (stsgcn.py:154-155), given its input x and
 * the gradient dZ of its output; rows = N*C.  The workspace holds one partial row of T*V*V + V*T*T floats per workgroup:
 * 1024 rows at T = 12, 256 or 512 at the coskad_window_ok geometries. */
size_t coskad_gcn_bwd_params_ws_bytes(int T, int V);
int coskad_gcn_bwd_params_f32(const float* x, const float* dZ, const float* A, const float* Tm, float* dA,
                              float* dT, void* ws, size_t ws_bytes, int accumulate, int rows, int T, int V,
                              hipStream_t stream);

/* coskad_gcn_bwd_params_f32 AND the input gradient of ConvTemporalGraphical (models/graph_layers/stsgcn.py:143-156 under
 * autograd) in one pass over dZ: dX = gcn^T(dZ) (+ dX_add, optional, same shape: the gradient an identity residual carries
 * beside the mix) -- what coskad_gcn_f32(adjoint = 1) computes from a second read of dZ. */
int coskad_gcn_bwd_params_dx_f32(const float* x, const float* dZ, const float* A, const float* Tm, float* dA, float* dT,
                                 float* dX, const float* dX_add, void* ws, size_t ws_bytes, int accumulate, int rows, int T,
                                 int V, hipStream_t stream);

/* ---- bottleneck Linear (models/sts/ae.py:97-101,157) ---------------------------------- */

/* z[n][j] = bias[j] + sum_k W[j][k] * PReLU_slope(U[n][k]);  slope NULL: no activation. L <= 16 (wider: the _ws entry point). */
int coskad_btlnk_fwd_f32(const float* U, const float* W, const float* bias, const float* slope, float* z,
                         int B, int K, int L, hipStream_t stream);

/* The same as a split-K GEMM (blocks of 64 clips x 8 K slices, fixed-order sum of the partials) with a workspace of
 * coskad_btlnk_fwd_ws_bytes(B) bytes: the large-batch path; K must be a multiple of 16. */
size_t coskad_btlnk_fwd_ws_bytes(int B);
/* Workspace bytes of coskad_btlnk_fwd_ws_f32 at any latent L <= 512: coskad_btlnk_fwd_ws_bytes(B) at L <= 16; above, the K-slice
 * partials of the wide GEMM (csrc/btlnk_wide.hip; any K).  coskad_btlnk_fwd_f32 (no workspace) stays at L <= 16. */
size_t coskad_btlnk_fwd_ws_bytes_l(int B, int K, int L);
int coskad_btlnk_fwd_ws_f32(const float* U, const float* W, const float* bias, const float* slope, float* z, void* ws,
                            size_t ws_bytes, int B, int K, int L, hipStream_t stream);
size_t coskad_btlnk_bwd_ws_bytes(int B, int K, int L);
/* dU = (dz W) * PReLU'(U);  dW (+)= dz^T PReLU(U);  db (+)= sum_n dz;  dslope (+)= sum (dz W) U [U<0].
 * coskad_btlnk_fwd_ws_f32 / coskad_btlnk_bwd_f32 at 16 < L <= 512: fp32 MFMA GEMMs tiled in LDS (csrc/btlnk_wide.hip), any K. */
int coskad_btlnk_bwd_f32(const float* U, const float* W, const float* dz, const float* slope, float* dU,
                         float* dW, float* db, float* dslope, void* ws, size_t ws_bytes, int accumulate,
                         int B, int K, int L, hipStream_t stream);

/* The same backward AND the batch reductions of the encoder's top ST_GCNN layer (models/graph_layers/stsgcn.py:94-116 under
 * autograd in training mode: P = sum dU Z^T, Q = sum dU PReLU(U_prev)^T, s = sum dU over clips and positions) from ONE pass
 * (csrc/btlnk_chain.hip: K tiled position-major, so the dU tile meets Z and U_prev of the same clips and positions on chip).
 * U is that layer's pre-activation [B, 64, TV] (K = 64 TV, TV % 4 == 0), below_in [B, below_Ci, TV] its input (pre-activation
 * of the layer below, below_in_slope its PReLU slope or NULL), below_Z [B, below_Ci, TV] its stored gcn output; below_Ci 16 / 32.
 * stats_out (8-byte aligned, coskad_btlnk_bwd_chain_floats(...) floats) receives the layer's backward chain buffer --
 * *stats_rows partial rows of 2 * 64 * below_Ci + 64 floats, then their fp64 sums -- which coskad_layer_bwd_chain_f32 takes
 * as `stats_in`.  ws: coskad_btlnk_bwd_chain_ws_bytes(B, K, L, TV) bytes.  Fixed-order sums: deterministic. */
int coskad_btlnk_bwd_chain_ok(int K, int TV, int below_Ci);
int coskad_btlnk_bwd_chain_rows(int B, int TV);
size_t coskad_btlnk_bwd_chain_floats(int B, int TV, int below_Ci);
size_t coskad_btlnk_bwd_chain_ws_bytes(int B, int K, int L, int TV);
int coskad_btlnk_bwd_chain_f32(const float* U, const float* W, const float* dz, const float* slope, float* dU, float* dW,
                               float* db, float* dslope, void* ws, size_t ws_bytes, int accumulate, int B, int K, int L,
                               const float* below_in, const float* below_Z, const float* below_in_slope, int below_Ci, int TV,
                               float* stats_out, size_t stats_out_bytes, int* stats_rows, hipStream_t stream);

/* The same with the Euclidean one-class head riding in the backward's launch (csrc/btlnk_chain.hip, HD form).  Instead of a finished
 * dz the call takes the split-K partials part [KS][B][16] of coskad_btlnk_fwd_parts_f32 (KS = coskad_btlnk_fwd_ks(); the forward
 * without its summing launch), the Linear's bias (or NULL), the centre c and `upstream`; the backward's workgroups form their
 * tiles of dz = 2 (z - c) upstream / (B L), z = (sum of the slices, in order) + bias, on chip, and extra blocks of the same launch
 * do the head: z, dz [B][L] written, score [B] / stats / acc as in coskad_mse_head_f32 (NULL to skip; head_ws:
 * coskad_head_ws_floats(B) floats; above 512 clips the statistics are finished by one more block of the reduce launch).  Every
 * value is bit-identical to coskad_btlnk_fwd_ws_f32 + coskad_mse_head_f32 + coskad_btlnk_bwd_chain_f32: three launches fewer. */
int coskad_btlnk_fwd_ks(void);
int coskad_btlnk_fwd_parts_f32(const float* U, const float* W, const float* slope, float* part, size_t part_bytes, int B, int K,
                               int L, hipStream_t stream);
int coskad_btlnk_bwd_chain_head_f32(const float* U, const float* W, const float* part, int KS, const float* bias, const float* c,
                                    float upstream, float* z, float* dz, float* score, float* stats, float* acc, float* head_ws,
                                    const float* slope, float* dU, float* dW, float* db, float* dslope, void* ws, size_t ws_bytes,
                                    int accumulate, int B, int K, int L, const float* below_in, const float* below_Z,
                                    const float* below_in_slope, int below_Ci, int TV, float* stats_out, size_t stats_out_bytes,
                                    int* stats_rows, hipStream_t stream);

/* ---- batch formation from the HBM-resident window table (callers' side of the path) ----- */

/* out[b, c, :] = M[t][c][0] x[s] + M[t][c][1] y[s] + M[t][c][2] with s = index[b] % N, t = index[b] / N, c < 2:
 * the item rule of utils/dataset.py:65-77 with the affine PoseTransform of utils/dataset_utils.py:272-310.
 * xy: [N, 2, TV], index: [B] int64, mats: [ntrans, 3, 3], out: [B, 2, TV]. */
int coskad_gather_transform_f32(const float* xy, const long long* index, const float* mats, float* out, int B, int N,
                                int ntrans, int TV, hipStream_t stream);

/* The same items from a FRAME table: one normalised row per trajectory frame instead of one row per window, so a frame is stored
 * once however many windows overlap it (coskad_amd.utils.dataset.PoseFramesRobust / FrameWindows).  With s = index[b] % N,
 * tr = index[b] / N and r = win_row[s] + t step:
 *   out[b, c, t, v] = (M[tr][c][0] x + M[tr][c][1] y) + M[tr][c][2],  (x, y) = fxy[r, 0 / 1, v],  c < 2, t < T, v < V
 * in the association of coskad_gather_transform_f32: for the same normalised values the two entries give the same bits.
 * fxy: [F, 2, V], win_row: [N] int32 (row of each window's first frame), index: [B] int64, mats: [ntrans, 3, 3], out: [B, 2, T, V]
 * (16-byte aligned where T V % 4 == 0).  T, V and step are run-time values.  index[b] < 0, index[b] >= N ntrans and a window whose
 * rows are not all inside [0, F) give a zero clip and read nothing out of bounds.  NULL pointers, a non-positive B, N, ntrans, T, V or
 * step and F outside [1, 2^31) fail with COSKAD_ERR_ARG. */
int coskad_gather_frames_f32(const float* fxy, const int* win_row, const long long* index, const float* mats, float* out, int B,
                             int N, long long F, int ntrans, int T, int V, int step, hipStream_t stream);

/* ---- frame-level scoring of a validation pass (csrc/score_frames.hip) ------------------------------- */

/* Per-window scores -> frame-level AUC on index tables that coskad_amd.utils.score_plan.ScorePlan derives once from the window table
 * (eval_COSKAD.py:140-253, utils/eval_utils.py:200-248).  fp64, fixed summation order, no floating-point atomics: deterministic.
 *   person_frames: pf[e] = mean of scores[win_idx[k]] != 0 over k in [win_ptr[e], win_ptr[e+1]) (0 when none is left); e = one
 *                  (person, frame), n_rows of them; scores: n_scores floats (scores_f64 = 0) or doubles (1)
 *   pad          : pad_scores on every person's row pf[row_ptr[p] .. row_ptr[p+1]) in place; n_max = the longest row, at most
 *                  coskad_score_pad_row_max() frames
 *   clip_max     : raw[t, o] = max over the persons pc_ptr[t n_clips + c] .. pc_ptr[t n_clips + c + 1] of pf[row_ptr[p] + out_frame[o]],
 *                  c = out_clip[o]; 0 for a clip without persons; raw: [n_transform, F]
 *   smooth       : per segment [seg0, seg1) of the F positions: shift by 11, reflect boundary, symmetric filter of taps[0] (centre) ..
 *                  taps[120]; tiles: n_tiles rows of {seg0, seg1, tile start}, coskad_score_tile() outputs each; per_t [n_transform, F],
 *                  mean [F] = their mean over the transformations
 *   auc          : sorted_scores ascending, gt_sorted the ground truth in that order (non-zero = positive), cum_neg its inclusive count
 *                  of negatives; out = {AUC, n_pos, n_neg} (AUC NaN when one class is empty); ws: coskad_score_auc_ws(F) elements */
int coskad_score_pad_row_max(void);
int coskad_score_tile(void);
int coskad_score_auc_ws(int F);
int coskad_score_person_frames_f64(const void* scores, int scores_f64, const int* win_ptr, const int* win_idx, double* pf,
                                   int n_scores, int n_rows, hipStream_t stream);
int coskad_score_pad_f64(double* pf, const int* row_ptr, int n_persons, int pad_size, int n_max, hipStream_t stream);
int coskad_score_clip_max_f64(const double* pf, const int* row_ptr, const int* pc_ptr, const int* out_clip, const int* out_frame,
                              double* raw, int n_clips, int n_transform, int F, hipStream_t stream);
int coskad_score_smooth_f64(const double* raw, const int* tiles, const double* taps, int n_taps, double* per_t, double* mean,
                            int n_tiles, int n_transform, int F, hipStream_t stream);
int coskad_score_auc_f64(const double* sorted_scores, const int* gt_sorted, const long long* cum_neg, double* out, long long* ws,
                         size_t ws_elems, int F, hipStream_t stream);

/* ---- the evaluation report: per-segment AUCs and ROC thresholds (csrc/score_report.hip) ------------------------------- */

/* The AUC of every segment of every row, and per row the thresholds where its ROC curve crosses tpr = 1 - fpr (eval_COSKAD.py:222-242,
 * utils/eval_utils.py:216-230).  Rows are [n_rows, F]; fp64 comparisons, integer counts, no floating-point atomics: deterministic.
 *   auc       : segments: n_seg rows {start, end} that do not overlap, each inside [0, F]; sorted_scores ascending inside every
 *               segment, gt_sorted the ground truth in that order, cum_neg its inclusive count of negatives along the whole row;
 *               tile_ptr [n_seg + 1]: the running sum of ceil((end - start) / coskad_score_report_tile()), n_tiles >= tile_ptr[n_seg]
 *               the launch's tile count (at most F / tile + n_seg); out [n_rows, n_seg, 3] = {AUC, n_pos, n_neg}, the statistic and
 *               the quotient formed as coskad_score_auc_f64 forms them (AUC NaN for one class or no frame; {NaN, -1, -1} for a
 *               segment outside [0, F] or a tile_ptr that does not match it); ws: coskad_score_report_auc_ws(n_rows, n_tiles) elements
 *   thresholds: sorted_scores ascending along each row of F; out [n_rows, 3] = {n, thr0, thr1}: the n = 1 or 2 values
 *               tr[np.argwhere(np.diff(np.sign(tpr - (1 - fpr))))] of sklearn's roc_curve(drop_intermediate=True), thr0 may be +inf;
 *               n = 0 for a single-class row; ws: coskad_score_report_thr_ws(n_rows, F) elements */
int coskad_score_report_tile(void);
long long coskad_score_report_auc_ws(int n_rows, int n_tiles);
long long coskad_score_report_thr_ws(int n_rows, int F);
int coskad_score_report_auc_f64(const double* sorted_scores, const int* gt_sorted, const long long* cum_neg, const int* segments,
                                const int* tile_ptr, double* out, long long* ws, size_t ws_elems, int n_tiles, int n_rows, int n_seg,
                                int F, hipStream_t stream);
int coskad_score_report_thresholds_f64(const double* sorted_scores, const long long* cum_neg, double* out, int* ws, size_t ws_elems,
                                       int n_rows, int F, hipStream_t stream);

/* Per-window attribution maps attr [n_windows, T, V] -> per-person frame maps out [n_rows, V] (csrc/attribution_frames.hip), on the
 * window CSR of coskad_score_person_frames_f64: out[e] = the mean over the windows win_idx[win_ptr[e] .. win_ptr[e + 1]) of
 * attr[w][t], t the first position with frames[w][t] == entry_frame[e] (frames [n_windows, T], the window table's frame numbers;
 * entry_frame [n_rows], the frame number of every row); NaN where no window holds the frame.  fp64 sums in ascending window order, no
 * atomics: bitwise reproducible. */
int coskad_attribution_frames_f64(const float* attr, const int* frames, const int* win_ptr, const int* win_idx, const int* entry_frame,
                                  double* out, int n_windows, int n_rows, int T, int V, hipStream_t stream);

/* ---- online scoring: live pose tracks, one frame at a time (csrc/stream.hip; coskad_amd/stream.py) ------------------------------- */

/* The offline route's arithmetic per frame.  State of M tracks, R = (T - 1) step + 1: ring [M, R, 2, V] f32 (row r of a track at slot
 * r % R), count [M] int32 (rows pushed per track), wscore [M, K, R] f64 (the score of the window ENDING at row e at slot e % R).
 *   push  : one wave per detection.  raw [n, 34] pixel rows (x1, y1, ...; zeros = missing joint) -> bounding-box-centred coordinates
 *           (utils/data.py:9-43,159-181, fp32) -> RobustScaler (center / scale [34] f64, both NULL = normalize_pose off; f32(f64(x) -
 *           center), then f32(f64(.) / scale); a centred 0 stays 0) -> layout (flags: 1 kp18_format, 2 headless; V = 17 / 18 / 14) ->
 *           ring row count[slot] (count <- 0 first where reset[i] != 0), count + 1.  flags & 4: the rows are normalised already and only
 *           the layout applies.  Where out_index[i] = j >= 0 the window that ends at this row (rows e - (R - 1) + t step) is written K
 *           times: x_out[k m + j] = (M[k][c][0] x + M[k][c][1] y) + M[k][c][2], bit for bit coskad_gather_frames_f32's items;
 *           x_out [K m, 2, T, V] (may be NULL at m = 0), mats [K, 3, 3].  A ready row whose count is below R gives a zero window.
 *   frames: scores [K m] of x_out (floats, or doubles with scores_f64) -> wscore; frame_mean [K, m] = for each ready track the row
 *           e - (R - 1), final now: the mean over the windows that end at e - t step (t < T, end >= R - 1) by ascending window start,
 *           exact zeros missing, 0 when none is left (the rules of coskad_score_person_frames_f64).  clip [K, clip_frames] (or NULL):
 *           clip[k][clip_index[j]] = max(., mean), an unsigned 64-bit atomic max on the bit pattern (scores are non-negative; the max
 *           is order-free, so the result is reproducible); clip_index[j] outside [0, clip_frames) is skipped.
 *   close : row_slot / row_index [rows]: trailing rows of closed tracks (at most min(count, R - 1) per track) -> frame_mean [K, rows]
 *           from the windows that exist (0 for a track that never filled one), folded into clip likewise.
 *   push_cams: `push` for the detections of several cameras in one launch (coskad_amd.stream.StreamBank): res [n, 2] f32 on
 *           the device = (width, height) of each detection's video instead of the two scalars, res_host the host's copy, which the
 *           launcher checks (every side >= 1); both are ignored (may be NULL) with flags & 4.  Same arithmetic, same results.
 *   smooth: fixed-lag smoothing over a flat clip buffer clip [K, F] that holds one segment per camera.  items [n_items, 3] int32 =
 *           (segment offset, segment length n, output index i), items_host the host's copy: per transformation shifted[j] = raw[j - 11]
 *           (0 below 11) under the `reflect` boundary of period 2n, the centre tap first, then (x[i - k] + x[i + k]) taps[k] for
 *           k = 120 .. 1 -- bit for bit coskad_score_smooth_f64's value of that segment; per_t [K, n_items], mean [n_items] = (sum over
 *           t in order) / K.  No atomics.  An item reads raw[max(0, i - 131) .. min(n - 1, i + 109)] (reflected where i + 120 >= n or
 *           i < 120): while a segment's right end is open the caller asks only for i whose reads are final.  n_taps != 121:
 *           COSKAD_ERR_SHAPE; an item with offset < 0, n <= 0, offset + n > F or i outside [0, n): COSKAD_ERR_ARG, naming the row.
 * slot_host / row_slot_host: the host's copy of the slots, which the launcher checks before the launch.  NULL pointers, non-positive
 * sizes, m > n, a slot outside [0, M) or twice in one push / frames launch, V that does not match the flags: COSKAD_ERR_ARG;
 * T outside {8, 12, 16, 24} or V outside {14, 17, 18}: COSKAD_ERR_SHAPE; all before the device is touched. */
int coskad_stream_ok(int T, int V);
int coskad_stream_smooth_lag(void);      /* 120: frames between a final raw clip score and its final smoothed score */
int coskad_stream_push_f32(const float* raw, const int* slot, const int* slot_host, const int* reset, const int* out_index,
                           const double* center, const double* scale, float width, float height, int flags, const float* mats,
                           float* ring, int* count, float* x_out, int n, int m, int M, int K, int T, int V, int step,
                           hipStream_t stream);
int coskad_stream_push_cams_f32(const float* raw, const int* slot, const int* slot_host, const int* reset, const int* out_index,
                                const double* center, const double* scale, const float* res, const float* res_host, int flags,
                                const float* mats, float* ring, int* count, float* x_out, int n, int m, int M, int K, int T, int V,
                                int step, hipStream_t stream);
int coskad_stream_frames_f64(const void* scores, int scores_f64, const int* slot, const int* slot_host, const int* clip_index,
                             const int* count, double* wscore, double* frame_mean, double* clip, int clip_frames, int m, int M, int K,
                             int T, int step, hipStream_t stream);
int coskad_stream_close_f64(const int* row_slot, const int* row_slot_host, const int* row_index, const int* clip_index, const int* count,
                            const double* wscore, double* frame_mean, double* clip, int clip_frames, int rows, int M, int K, int T,
                            int step, hipStream_t stream);
int coskad_stream_smooth_f64(const double* clip, const int* items, const int* items_host, const double* taps, int n_taps, double* per_t,
                             double* mean, int n_items, int K, int F, hipStream_t stream);

/* Per-joint maps beside the scores: the streaming counterpart of coskad_attribution_frames_f64.  state: one buffer of
 * coskad_stream_maps_state_bytes(M, K, T, V, step) bytes, aligned to 8 -- running fp64 sums [M, K, R, V], then int32 counts [M, K, R],
 * row i of a track at slot i % R (0 bytes for sizes the entries refuse).  The caller never has to clear it: a track's first window
 * (count == R) overwrites every slot of the track, so a reused slot does not see its previous track's sums.
 *   maps      : after `frames` of the same push.  maps [K m, T, V] f32, item k m + j as in x_out: the map of the window that ends at
 *               the ready track's newest row e = count - 1; its row t is added to track row e - (T - 1 - t) step.  frame_map [K, m, V]
 *               = the map of row e - (R - 1), final now: the mean over the windows that cover the row of the row each holds for it --
 *               fp64 sums in ascending window start (the order of arrival), one division by the count, bit for bit
 *               coskad_attribution_frames_f64's value.  Unlike `frames` an exact 0 counts.  NaN where count < R (the host's mirror and
 *               `count` disagree).  One wave per (transformation, track), no atomics.  It must follow EVERY push that hands the track
 *               a window: the sums are formed on arrival.
 *   maps_close: row_slot / row_index [rows] as for `close`, before the slot's next push -> frame_map [K, rows, V] from the windows
 *               that exist; NaN for a track that never filled a window, for a row no window covers (step > 1) and for a row the state
 *               no longer holds.
 * NULL pointers, non-positive sizes, m > M, a slot outside [0, M) or twice in one maps launch, state_bytes below the query or a
 * misaligned state: COSKAD_ERR_ARG; T outside {8, 12, 16, 24} or V outside {14, 17, 18}: COSKAD_ERR_SHAPE; all before the device is
 * touched. */
size_t coskad_stream_maps_state_bytes(int M, int K, int T, int V, int step);
int coskad_stream_maps_f64(const float* maps, const int* slot, const int* slot_host, const int* count, double* state, size_t state_bytes,
                           double* frame_map, int m, int M, int K, int T, int V, int step, hipStream_t stream);
int coskad_stream_maps_close_f64(const int* row_slot, const int* row_slot_host, const int* row_index, const int* count,
                                 const double* state, size_t state_bytes, double* frame_map, int rows, int M, int K, int T, int V,
                                 int step, hipStream_t stream);

/* ---- one-class heads, centre statistics, regulariser, optimiser ------------------------ */

int coskad_head_slots(void);            /* floats in a stats / acc block (19) at latent <= 16 */
size_t coskad_head_ws_floats(int B);    /* scratch floats the head kernels need at latent <= 16 */
/* The same at latent L <= 512 (csrc/heads_wide.hip above 16): with Lp = max(L, 16) a stats / acc block holds Lp + 3 floats,
 * [0] loss term, [1..Lp] vector sum, [Lp+1] scalar A, [Lp+2] scalar B -- the 19-slot layout at L <= 16.  0 beyond 512. */
int coskad_head_slots_l(int L);
size_t coskad_head_ws_floats_l(int B, int L);

/* Every head, centre and midpoint entry point takes latents L <= 512; stats / acc then hold coskad_head_slots_l(L) floats
 * ([17], [18] below read [Lp+1], [Lp+2]) and ws coskad_head_ws_floats_l(B, L) floats.
 * F.mse_loss(z, c) (euclidean_encoder_staticCenter.py:187, _dynamicCenter.py:116), its gradient,
 * the per-window score of utils/eval_utils.py:63-64, and the running-centre sums (:172-178).
 * stats: [0] loss, [1..L] sum_n z, [17] B, [18] sum_n |z_n|;  acc += raw sums. */
int coskad_mse_head_f32(const float* z, const float* c, float* dz, float* score, float* stats, float* acc,
                        float upstream, float* ws, int B, int L, hipStream_t stream);

/* Mahalanobis head: loss = mean_n sqrt((z_n-c)^T VI (z_n-c)) (utils/eval_utils.py:28-38, called at
 * euclidean_encoder_staticCenter.py:178-181), gradient, score (eval_utils.py:41-47), the MSE head's centre sums, and
 * gram[L*L] (+)= sum_n z_n z_n^T, from which batch_cov_mat_step / compute_inv_cov_mat (:40-46,133-142) follow. */
int coskad_mahalanobis_head_f32(const float* z, const float* c, const float* VI, float* dz, float* score,
                                float* stats, float* acc, float* gram, int gram_accumulate, float upstream,
                                float* ws, int B, int L, hipStream_t stream);

/* zh = project(expmap0(z)); loss = mean dist(c, zh) (hyperbolic_encoder.py:147,157 with the formulas
 * of utils/hyper_math.py:13-29,100-105,173-179,207-210,302-306), gradient w.r.t. z, score = dist,
 * stats: [0] loss, [1..L] sum gamma*zh, [17] sum (gamma-1), [18] sum |zh|;  c NULL: embed + sums only. */
int coskad_poincare_head_f32(const float* z, const float* c, float* dz, float* zh, float* score,
                             float* stats, float* acc, float upstream, float* ws, int B, int L,
                             hipStream_t stream);
int coskad_poincare_dist_f32(const float* zh, const float* c, float* score, int B, int L, hipStream_t stream);
/* out[n] = logmap0(y[n]) = y / |y| * artanh(|y|) for points on the unit Poincare ball (utils/hyper_math.py:367-370 at c = 1, with its
 * 1e-5 norm floor and Artanh's +-(1 - 1e-5) clamp, :18-24): the inverse of expmap0 that north_star names; the reference's wrappers
 * never call it, so it stands alone (no gradient entry). */
int coskad_poincare_logmap0_f32(const float* y, float* out, int B, int L, hipStream_t stream);

/* The statistics algebra of the folded first decoder layer (coskad_amd/lowrank.py: rev_btlnk, models/sts/ae.py:223-227, + the first
 * ST_GCNN layer of the decoder, models/graph_layers/stsgcn.py:106-110, on a rank-(latent + 1) input) for latent 8: X [2, 9, Co, TV] holds
 * the nine basis images of the two BatchNorm branches, G [9, 9] (fp64) the latents' Gram matrix sum_n [z, 1][z, 1]^T.
 *   fwd: batch statistics of both branches from G (fp64), running-statistics update (momentum, unbiased variance; conv biases shift
 *        the running means only), folded images in the rev_btlnk kernels' weight layout Mw [Co TV, 8], Mb [Co TV]; saved / xbar / xx:
 *        fp64 scratch of 6 Co / 18 Co / 162 Co doubles for the backward
 *   bwd: from dMw / dMb: dX [2, 9, Co, TV], dgamma [2][Co], dbeta [Co] (both BatchNorms'), dGc [Co][9][9] (its sum over Co is dG) */
int coskad_lowrank_fold_ok(int latent, int TV);
int coskad_lowrank_fold_fwd_f32(const float* X, const double* G, const float* gamma0, const float* beta0, const float* cbias0,
                                float* rmean0, float* rvar0, long long* nbt0, float momentum0, float eps0, const float* gamma1,
                                const float* beta1, const float* cbias1, float* rmean1, float* rvar1, long long* nbt1, float momentum1,
                                float eps1, double n_pos, float* Mw, float* Mb, double* saved, double* xbar, double* xx, int Co, int TV,
                                hipStream_t stream);
int coskad_lowrank_fold_bwd_f32(const float* X, const double* G, const float* dMw, const float* dMb, const double* saved,
                                const double* xbar, const double* xx, const float* gamma0, const float* gamma1, double n_pos, float* dX,
                                float* dgamma, float* dbeta, double* dGc, int Co, int TV, hipStream_t stream);

/* Narrow-output layers (C_out <= 4 behind 16 / 32 / 64 input channels: the decoder's last layer, models/common/components.py:143-179 ->
 * models/graph_layers/stsgcn.py:94-116) by commutation -- the mixing acts per channel, a 1x1 convolution per position, so
 * Wt gcn(X) = gcn(Wt X): both convolutions of the layer run first, as one streaming pass over the wide input, and mixing / BatchNorm /
 * PReLU see 2 C_out-channel tensors (csrc/last_layer.hip).
 *   fwd : out [B, J, TV] = W [J, Ci] . PReLU(U [B, Ci, TV])   (in_slope NULL: U is activated already); J = 2 C_out in {2, 4, 6, 8}
 *   bwd : dU [B, Ci, TV] = (W^T dOut) * PReLU'(U); partials [coskad_narrow_conv_rows(B, TV)][J Ci + 1]: per-workgroup sums of
 *         dW[j][c] = sum dOut_j PReLU(U)_c and, last column, of the producer's slope gradient -- add the rows with coskad_gemm_sum_f32
 * Both passes move 16-byte vectors: U, out, dOut and dU must be 16-byte aligned (COSKAD_ERR_ARG naming the pointer otherwise, before
 * anything is launched). */
int coskad_narrow_conv_rows(int B, int TV);
int coskad_narrow_conv_fwd_f32(const float* U, const float* in_slope, const float* W, float* out, int B, int Ci, int J, int TV,
                               hipStream_t stream);
int coskad_narrow_conv_bwd_f32(const float* U, const float* in_slope, const float* W, const float* dOut, float* dU, float* partials,
                               size_t partials_floats, int B, int Ci, int J, int TV, hipStream_t stream);

/* coskad_layer_apply_z_f32 AND the next layer's statistics pass in one kernel on the 25-joint layout (what coskad_layer_apply_next_f32 is
 * at 17 joints; csrc/fused_apply_flat.hip): U = Wz.Z + Wx.PReLU_in(in) + b -> out; Z_next = gcn_next(PReLU_out(U)) [B, Co, T, V]; partials:
 * coskad_layer_apply_next_flat_rows(B) rows of [sum x x^T][sum x][sum z z^T][sum z] (2 (Co^2 + Co) floats) for
 * coskad_layer_train_fold_f32 (models/graph_layers/stsgcn.py:94-116 of layer i; 56-80 + the batch statistics of layer i + 1's
 * BatchNorms).  ok: 1 for 12 x 25, 16 / 32 -> 16 / 32 channels. */
int coskad_layer_apply_next_flat_ok(int Ci, int Co, int T, int V);
int coskad_layer_apply_next_flat_rows(int B);
int coskad_layer_apply_next_flat_f32(const float* Z, const float* in, float* out, const float* wfold, const float* bias,
                                     const float* in_slope, const float* out_slope, const float* A_next, const float* T_next,
                                     float* Z_next, float* partials, size_t partials_bytes, int B, int Ci, int Co, int T, int V,
                                     hipStream_t stream);

/* The FIRST two ST_GCNN layers of the encoder with folded BatchNorm (coskad_layer_apply_f32 twice: models/graph_layers/stsgcn.py:94-116
 * in eval mode, entries 0 and 1 of the nn.Sequential of models/common/components.py:94-105) in ONE pass -- x [B, 2, T, V] is the network
 * input, the first layer (2 -> 32) is formed per clip on the VALU inside the second layer's kernel and its output never reaches HBM
 * (csrc/eval_layer_clip.hip, FIRST form; at the window lengths 8 / 16 / 24 x and out must be 16-byte aligned).  ok: 1 when
 * (n_frames, n_joints, C_in, C_mid, C_out) is built (8 | 12 | 16 | 24, 17 | 25, 2, 32, 16 | 32 | 64).
 * wfold1 [4, 32] / bias1, wfold2 [64, Co] / bias2 from coskad_bn_fold_f32; mid_slope: the first layer's PReLU weight; out_slope NULL:
 * pre-activation output. */
int coskad_layer_first_pair_ok(int T, int V, int Ci, int Cm, int Co);
int coskad_layer_first_pair_apply_f32(const float* x, float* out, const float* A1, const float* T1, const float* wfold1, const float* bias1,
                                      const float* A2, const float* T2, const float* wfold2, const float* bias2, const float* mid_slope,
                                      const float* out_slope, int B, int Cm, int Co, int T, int V, hipStream_t stream);

/* A (32 -> 16) ST_GCNN layer in training mode by the same commutation, on its own kernels (csrc/commute_layer.hip; replaces
 * models/graph_layers/stsgcn.py:94-116 and its autograd for such a layer on the 12 x 25 layout): Y = Wt X, R = Wr X first (X = PReLU(u_prev)),
 * Zy = gcn(Y); both BatchNorms become per-channel affine maps of Zy and R (batch statistics = row sums); the backward is one kernel per clip
 * behind two row-sum reductions.
 *   ok        : 1 when (n_frames, n_joints, C_in, C_out) is built (12, 25, 32, 16)
 *   ws_floats : floats of the scratch both entries need
 *   fwd       : writes YR [B, 32, TV] = [Y; R], Zy [B, 16, TV], U [B, 16, TV] (the layer's pre-activation output), stat [128]; updates the
 *               running statistics / num_batches_tracked of both BatchNorms as torch does (NULL: not tracked; momentum a number);
 *               A_next != NULL: the next layer's statistics pass in the same launches (Z_next = gcn_next(PReLU(U)), *rows_next rows of
 *               moment partials for coskad_layer_train_fold_f32; slope_out = this layer's PReLU weight)
 *   bwd       : dU [B, 16, TV] -> d_in [B, 32, TV] (PReLU mask of u_prev applied), dA [T, V, V], dT [V, T, T], dWt / dWr [16, 32],
 *               dgamma / dbeta [16] of both BatchNorms, dslope [1] (the producer's PReLU weight; NULL iff in_slope NULL): all overwritten;
 *               below_stats != NULL (a 2-channel layer in front, fed by the network input below_x, stored Z below_z): that layer's batch
 *               reductions too, as the chain buffer coskad_layer_bwd_chain_f32 takes (stats_in, coskad_commute_below_rows(B) rows,
 *               coskad_commute_below_floats(B) floats) */
int coskad_commute_ok(int T, int V, int Ci, int Co);
size_t coskad_commute_ws_floats(int B, int T, int V);
int coskad_commute_fwd_f32(const float* u_prev, const float* in_slope, const float* wt, const float* wr, const float* A, const float* Tm,
                           const float* gamma_t, const float* beta_t, const float* gamma_r, const float* beta_r, const float* bias_t,
                           const float* bias_r, float* rm_t, float* rv_t, float* rm_r, float* rv_r, long long* nbt_t, long long* nbt_r,
                           float momentum, float eps, float* YR, float* Zy, float* U, float* stat, float* ws, size_t ws_floats,
                           const float* A_next, const float* T_next, const float* slope_out, float* Z_next, float* partials_next,
                           int* rows_next, int B, int T, int V, hipStream_t stream);
int coskad_commute_bwd_f32(const float* u_prev, const float* in_slope, const float* wt, const float* wr, const float* A, const float* Tm,
                           const float* YR, const float* Zy, const float* stat, const float* dU, float* d_in, float* dA, float* dT,
                           float* dWt, float* dWr, float* dgamma_t, float* dbeta_t, float* dgamma_r, float* dbeta_r, float* dslope,
                           float* ws, size_t ws_floats, const float* below_x, const float* below_z, float* below_stats,
                           size_t below_stats_floats, int B, int T, int V, hipStream_t stream);
int coskad_commute_below_rows(int B);
size_t coskad_commute_below_floats(int B);

/* The spherical VAE's latent head between the raw outputs of fc_mean / fc_var and the decoder's input (models/sts/vae.py:79-91,
 * 104-118; loss terms of models/spherical_vae.py:86-94; PowerSpherical of the un-vendored `power_spherical` package, restated in
 * coskad_amd/models/sts/vae.py).  Rows are clips; mean_raw [B, L] and var_raw [B] are addressed with row strides ld_* (floats), so both
 * may be columns of ONE [B, L + 1] tensor.  2 <= L <= 512 (to 16: one thread per clip, csrc/vae_head.hip; above: one wave per clip,
 * csrc/vae_head_wide.hip); other L fail with COSKAD_ERR_SHAPE.
 *   prep  : mu = mean_raw / |mean_raw|, kappa = softplus(var_raw) + 1, concentration [B, 2] = ((L-1)/2 + kappa, (L-1)/2), total [B]
 *   (the caller draws x ~ Dirichlet(concentration) [B, 2] and eps ~ N(0, I) [B, L-1]; torch._dirichlet_grad gives the sampler's
 *    implicit reparameterisation gradient [B, 2] for the backward)
 *   sample: z [B, L] = Householder(e1 -> mu) applied to [2 x_0 - 1, sqrt(1 - t^2) eps / |eps|]; kl [B] = KL(PowerSpherical(mu, kappa) ||
 *           uniform on the sphere) per clip; inv_kappa [B] = 1 / kappa
 *   bwd   : d_mean_raw, d_var_raw from dz (gradient w.r.t. z) and the weights w_kl = d loss / d kl[n], w_exp = d loss / d inv_kappa[n] */
int coskad_ps_head_prep_f32(const float* mean_raw, int ld_mean, const float* var_raw, int ld_var, float* mu, float* kappa,
                            float* concentration, float* total, int B, int L, hipStream_t stream);
int coskad_ps_head_sample_f32(const float* x, const float* eps, const float* mu, const float* kappa, float* z, float* kl,
                              float* inv_kappa, int B, int L, hipStream_t stream);
int coskad_ps_head_bwd_f32(const float* dz, const float* x, const float* dirichlet_grad, const float* eps, const float* mu,
                           const float* kappa, const float* mean_raw, int ld_mean, const float* var_raw, int ld_var, float w_kl,
                           float w_exp, float* d_mean_raw, int ld_dmean, float* d_var_raw, int ld_dvar, int B, int L,
                           hipStream_t stream);

/* The Gaussian VAE's latent head (`distribution: 'normal'`: models/sts/vae.py:85,106-108,129; loss terms of
 * models/spherical_vae.py:89-90,98), csrc/vae_head_normal.hip.  Rows are clips; mean_raw [B, L] and var_raw [B, L] are addressed with
 * row strides ld_* (floats), so both may be column blocks of ONE [B, 2L] tensor, and so are the gradient destinations; eps, z, sigma
 * and dz are contiguous [B, L].  1 <= L <= 512 (coskad_normal_head_ok); other L fail with COSKAD_ERR_SHAPE, as does B = 0; B < 0, a
 * stride below L, score without ref, and neither z nor score fail with COSKAD_ERR_ARG.
 *   fwd: sigma = softplus(var_raw) + 1;  z = mean_raw + sigma eps (eps: the caller's N(0, 1) draw);
 *        kl [B] = sum_l 0.5 (sigma^2 + mu^2 - 1 - log sigma^2);  inv [B] = sum_l 1 / sigma;  sigma, kl, inv may be NULL.
 *        ref [L] with score [B]: score[n] = 1 - F.cosine_similarity(ref, z[n]) (each norm clamped at 1e-8); z may then be NULL.
 *   bwd: d_mean_raw = dz + w_kl mu;  d_var_raw = (dz eps + w_kl (sigma - 1 / sigma) - w_exp / sigma^2) softplus'(var_raw), with
 *        w_kl = d loss / d kl[n] and w_exp = d loss / d (1 / sigma) per element.
 * Every sum is formed in an order that depends on L alone: a clip's results do not depend on the batch. */
int coskad_normal_head_ok(int L);
int coskad_normal_head_fwd_f32(const float* mean_raw, int ld_mean, const float* var_raw, int ld_var, const float* eps, float* z,
                               float* sigma, float* kl, float* inv, const float* ref, float* score, int B, int L,
                               hipStream_t stream);
int coskad_normal_head_bwd_f32(const float* dz, const float* eps, const float* sigma, const float* mean_raw, int ld_mean,
                               const float* var_raw, int ld_var, float w_kl, float w_exp, float* d_mean_raw, int ld_dmean,
                               float* d_var_raw, int ld_dvar, int B, int L, hipStream_t stream);

/* c = acc[1..L] / acc[17], then |c| < eps -> +-eps (staticCenter.py:118-121). */
int coskad_center_finalize_f32(const float* acc, float* c, float eps, int L, hipStream_t stream);
/* gyromidpoint from acc of coskad_poincare_head_f32 (hyperbolic_encoder.py:122,179). */
int coskad_midpoint_finalize_f32(const float* acc, float* c, int L, hipStream_t stream);

/* out[0] = scale * sum_i mask[i] p[i]^2  (utils/model_utils.py:90-105). ws: 256 floats. */
int coskad_sqnorm_f32(const float* p, const float* mask, size_t n, float scale, float* out, float* ws,
                      hipStream_t stream);
/* torch.optim.Adam step on flat buffers with g = grad*gscale + reg_coef*mask*p. */
int coskad_adam_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float lr,
                    float beta1, float beta2, float eps, int step, float gscale, float reg_coef,
                    hipStream_t stream);

/* coskad_adam_f32 with the caller's fp32 running products b1pow = beta1^t, b2pow = beta2^t instead of the step count: the
 * arithmetic of coskad_adam_dev_f32's device-side tick (an eager step and a hipGraph-captured one then agree bit for bit). */
int coskad_adam_pow_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float lr, float beta1,
                        float beta2, float eps, float b1pow, float b2pow, float gscale, float reg_coef, hipStream_t stream);

/* Adam with {lr, beta1^t, beta2^t} in device memory (hipGraph-replayable; init hyper = {lr, 1, 1}). */
int coskad_adam_dev_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float* hyper,
                        float beta1, float beta2, float eps, float gscale, float reg_coef, hipStream_t stream);

/* Gradient clipping and accumulation on the flat buffers (csrc/grad_clip.hip).
 * partials[0 .. 255] (fp64) = per-workgroup sums of g_eff[i]^2 with g_eff = g*gscale + reg_coef*mask*p formed in fp32 as
 * coskad_adam_*_f32 forms it; entries no workgroup owns are written 0.  No atomics: repeated calls agree bit for bit. */
int coskad_grad_sqnorm_f32(const float* g, const float* p, const float* mask, size_t n, float gscale, float reg_coef,
                           double* partials, hipStream_t stream);

/* coskad_adam_pow_f32 / coskad_adam_dev_f32 with g_eff clipped before the moment updates.  clip_mode 1: by global norm, coef =
 * min(1, clip_val / (sqrt(sum partials) + 1e-6)) with the norm in fp32 (torch.nn.utils.clip_grad_norm_), every workgroup summing
 * `partials` (coskad_grad_sqnorm_f32's) in the same fixed order; the unclipped norm goes to norm_out[0] unless norm_out is NULL.
 * clip_mode 2: by value, clamp to [-clip_val, clip_val]; partials may be NULL and norm_out is not written.  clip_val must be
 * finite and > 0.  A coefficient of exactly 1 leaves p, m, v bit-identical to the unclipped entry points. */
int coskad_adam_clip_pow_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float lr, float beta1,
                             float beta2, float eps, float b1pow, float b2pow, float gscale, float reg_coef,
                             const double* partials, float clip_val, int clip_mode, float* norm_out, hipStream_t stream);
int coskad_adam_clip_dev_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float* hyper, float beta1,
                             float beta2, float eps, float gscale, float reg_coef, const double* partials, float clip_val,
                             int clip_mode, float* norm_out, hipStream_t stream);

/* acc = first ? g : acc + g over n floats (gradient accumulation over micro-batches). */
int coskad_grad_accum_f32(float* acc, const float* g, size_t n, int first, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* COSKAD_HIP_H */
