// The launch layer: what the host code behind the C ABI shares across files.
//   * the argument structs of the layer launchers (stsgcn_bwd.hip, stsgcn_train.hip): an entry point names what it has, everything
//     else is absent by construction (NULL / 0);
//   * every launcher and `*_ok` predicate that one .hip file defines and another calls, declared ONCE: the file that defines one and
//     the files that call it include this header, so a changed signature is a compile error and not a stale copy that still links;
//   * the A/B switches (ablate_env): read from the environment in -DCOSKAD_ABLATE builds only.
#pragma once
#include "common.h"
#include <cstdlib>
#include <type_traits>

extern "C" int coskad_window_ok(int T, int V);   // gcn_window.hip
extern "C" int coskad_layer_train_window_ok(int T, int V, int Ci, int Co);   // train_window_flat.hip
extern "C" int coskad_layer_train_window_narrow_ok(int T, int V, int Ci, int Co);

namespace coskad {

// ---- A/B switches ------------------------------------------------------------------------------------------------------------------
// The product library reads no environment variable: without -DCOSKAD_ABLATE a switch IS its default, at compile time.
// Use: `static const int x = ablate_env("COSKAD_X", 0);` (read once per process in the A/B builds of tools/).
#ifdef COSKAD_ABLATE
inline int ablate_env(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
#else
constexpr int ablate_env(const char*, int dflt) { return dflt; }
#endif

// f(std::integral_constant<int, n>{}) for a runtime tile count n in 1..4 (anything else: 4): the kernels take their tile counts
// as template parameters, the launch is written once as a generic lambda
template <class F>
inline void with_tiles(int n, F&& f) {
  if (n == 1) f(std::integral_constant<int, 1>{});
  else if (n == 2) f(std::integral_constant<int, 2>{});
  else if (n == 3) f(std::integral_constant<int, 3>{});
  else f(std::integral_constant<int, 4>{});
}

// ---- the layer backward (stsgcn_bwd.hip: launch_layer_bwd) --------------------------------------------------------------------------
struct LayerGrads {
  float* dIn = nullptr;        // NULL: the raw network input needs none
  float* dA = nullptr;
  float* dT = nullptr;
  float* dWt = nullptr;
  float* dbt = nullptr;
  float* dgt = nullptr;
  float* dbet = nullptr;
  float* dWr = nullptr;
  float* dbr = nullptr;
  float* dgr = nullptr;
  float* dber = nullptr;
  float* dslope_in = nullptr;  // the producer's PReLU weight
};
// this layer's stage-1 partial rows and (behind them, chain_sums_offset) their fp64 sums, written by the call for the layer above:
// stage 1 is skipped
struct ChainIn {
  const float* stats = nullptr;
  int rows = 0;
};
// the layer below's input / stored Z and the chain buffer ITS partial rows go to (fused data kernel only)
struct Below {
  const float* in = nullptr;
  const float* Z = nullptr;
  const float* slope = nullptr;
  int Ci = 0;
  float* stats = nullptr;
};
// run stage 1 ONLY, into that chain buffer (partial rows, then their fp64 sums); *rows_out = rows written
struct StatsOnly {
  float* out = nullptr;
  int* rows_out = nullptr;
};
struct LayerBwdArgs {
  const float* in = nullptr;
  const float* dU = nullptr;
  const float* A = nullptr;
  const float* Tm = nullptr;
  const float* in_slope = nullptr;
  const float* stat = nullptr;
  const float* Wt = nullptr;
  const float* gt = nullptr;
  const float* Wr = nullptr;    // stage 1 only asks whether it is there
  const float* gr = nullptr;
  const float* Z = nullptr;     // gcn(PReLU(in)) as stored by the forward (NULL: recomputed)
  LayerGrads g;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  int accumulate = 0;
  int B = 0, Ci = 0, Co = 0;
  hipStream_t stream = nullptr;
  ChainIn chain;
  double stats_count = 0.0;     // positions the stage-1 sums cover (0: this batch, B T V; SyncBN: all ranks' batches)
  Below below;
  StatsOnly stats_only;
  float* dz_ext = nullptr;      // dZ goes to (stage 4 alone: comes from) the caller's buffer; stage 4 is a call of its own
};

// ---- the layer statistics (stsgcn_train.hip: launch_train_stats, launch_reduce_fold) ------------------------------------------------
struct BnConvParams {   // the two 1x1 convolutions of a layer with their BatchNorms (t: the main branch, r: the residual)
  const float* Wt = nullptr;
  const float* bt = nullptr;
  const float* gt = nullptr;
  const float* bet = nullptr;
  float* rm_t = nullptr;
  float* rv_t = nullptr;
  long long* nbt_t = nullptr;
  const float* Wr = nullptr;
  const float* br = nullptr;
  const float* gr = nullptr;
  const float* ber = nullptr;
  float* rm_r = nullptr;
  float* rv_r = nullptr;
  long long* nbt_r = nullptr;
  float momentum = 0.f;
};
struct FoldOut {
  float* wfold = nullptr;
  float* bias = nullptr;
  float* stat = nullptr;
};
struct FtabArgs;        // ftab_ops.h
struct LayerStatsArgs {
  const FtabArgs* ftab = nullptr;    // operand tables of the layers above, built by extra blocks of the first layer's moments launch
  const float* in = nullptr;
  const float* A = nullptr;
  const float* Tm = nullptr;
  const float* in_slope = nullptr;
  const float* partials = nullptr;   // moment partial rows the previous layer's kernel wrote (no statistics pass here)
  int rows = 0;
  BnConvParams p;                    // p.Wt NULL: stop behind the fp64 moment sums
  FoldOut out;
  float* Zout = nullptr;             // gcn(PReLU(in)), stored for the apply kernel and the backward (NULL: not stored)
  double* sums = nullptr;            // the fp64 moment sums: written where the call stops behind them, read where it starts there
  void* ws = nullptr;
  size_t ws_bytes = 0;
  int B = 0, Ci = 0, Co = 0;
  hipStream_t stream = nullptr;
};

// ---- launchers and predicates that cross files -------------------------------------------------------------------------------------
// stsgcn_train.hip: out[e] = fp64 sum over `rows` partial rows of E floats (fixed order)
void launch_reduce_partials(const float* partials, int rows, int E, double* out, hipStream_t st);

// gcn_window.hip: the mixing kernels of the window lengths 8, 16 and 24 (coskad_window_ok), behind the entry points of
// stsgcn_fwd.hip / stsgcn_bwd.hip.  dX NULL: parameter gradients only.  in_slope (optional; 17 / 25 joints, 16-byte aligned rows):
// `x` is a pre-activation -- activated on load, dX multiplied by PReLU'(x) on store, the slope-gradient partials of the
// *rows_out workgroups to dap (summed by the caller).  in_slope NULL: results as without the three arguments, bit for bit.
int launch_window_gcn(const float* in, float* out, const float* Aw, const float* Tw, int rows, int T, int V, int adjoint,
                      hipStream_t st);
int launch_window_params(const float* x, const float* dZ, const float* Aw, const float* Tw, float* dA, float* dT, void* ws,
                         int accumulate, int rows, int T, int V, hipStream_t st, float* dX, const float* add,
                         const float* in_slope = nullptr, float* dap = nullptr, int* rows_out = nullptr);
size_t window_params_ws_bytes(int T, int V);

// train_window_moments.hip: the statistics pass of a training layer at the window lengths 8, 16 and 24 (17 / 25 joints; 2, 16, 32
// input channels): Z = gcn(PReLU(in)) -> Zout (NULL: not stored), *rows_out (<= 512) moment partial rows.  `in` / `Zout` 16-byte aligned
bool window_moments_ok(int T, int V, int Ci);
int launch_window_moments(const float* in, const float* Aw, const float* Tw, const float* in_slope, float* partials, int B, int Ci,
                          int T, int V, int need_x, float* Zout, hipStream_t st, int* rows_out);
// train_window_flat.hip: the position-wise passes of such a layer over a clip's T V positions (16-byte aligned activations):
// the stored-Z apply, stage 1 of the backward (<= 1024 partial rows) and its data pass (dXr NULL: dZ alone)
bool window_flat_ok(int TV, int Ci, int Co);
int launch_window_apply(const float* Z, const float* in, float* out, const float* wfold, const float* bias, const float* in_slope,
                        int B, int Ci, int Co, int TV, hipStream_t st);
int launch_window_stats(const float* in, const float* Zg, const float* dU, const float* in_slope, float* partials, int B, int Ci, int Co,
                        int TV, int need_q, hipStream_t st, int* rows_out);
int launch_window_data(const float* in, const float* Z, const float* dU, const float* coef, const float* in_slope, float* dZ, float* dXr,
                       int B, int Ci, int Co, int TV, hipStream_t st);

// fused_bwd.hip
int layer_bwd_below_rows(int T_, int V_, int B, int Ci, int Co, int below_Ci);
int launch_layer_bwd_bpc(const float* in, const float* Zg, const float* dU, const float* coef, const float* in_slope, float* dIn,
                         float* btab, float* partials, float* dap, int B, int Ci, int Co, hipStream_t st, int* rows_out,
                         const float* below_z, const float* below_x, const float* below_slope, int below_Ci, float* below_stats);
bool layer_bwd_fused_ok(int T_, int V_, int Ci, int Co);
int launch_reduce_fused(const float* partials, int rows, float* dA, float* dT, const float* dap, float* dslope, int accumulate,
                        hipStream_t st, const float* brows, int bE, double* bout);
// fused_stats.hip
bool bwd_stats_ring_ok(int T_, int V_, int Ci, int Co);
int launch_bwd_stats_ring(const float* in, const float* Zg, const float* dU, const float* in_slope, float* partials, int B,
                          int Ci, int Co, hipStream_t st, int* rows_out);
bool bwd_stats_bpc_ok(int T_, int V_, int Ci, int Co);
bool bwd_stats_flat_ok(int TV_, int Ci, int Co);
int launch_bwd_stats_flat(const float* in, const float* Zg, const float* dU, const float* in_slope, float* partials, int B,
                          int Ci, int Co, int TV_, hipStream_t st, int* rows_out);
int launch_bwd_stats_bpc(const float* in, const float* Zg, const float* dU, const float* in_slope, float* partials, int B,
                         int Ci, int Co, hipStream_t st, int* rows_out);
// bwd_data_bpc.hip
bool bwd_data_bpc_ok(int T_, int V_, int Ci, int Co);
int launch_bwd_data_bpc(const float* in, const float* Zg, const float* dU, const float* Aw, const float* Tw, const float* coef,
                        const float* in_slope, float* dIn, float* dZout, float* dap, int B, int Ci, int Co, int T_, int V_,
                        hipStream_t st, int* rows_out, float* gpart);
// gcn_params_bpc.hip
bool gcn_params_bpc_ok(int T_, int V_);
int launch_gcn_params_bpc(const float* in, const float* in_slope, const float* dz, const float* Aw, const float* Tw, float* partials,
                          int rows_total, int T_, int V_, hipStream_t st, int* rows_out);
// first_layer.hip
bool first_layer_ok(int T_, int V_, int Ci, int Co);
int launch_first_stats(const float* in, const float* Zg, const float* dU, const float* in_slope, float* partials, int B, int Ci,
                       int Co, int TVr, int need_q, int max_rows, hipStream_t st, int* rows_out);
int launch_first_bwd(const float* in, const float* Zg, const float* dU, const float* Aw, const float* Tw, const float* coef,
                     const float* in_slope, float* partials, int B, int Ci, int Co, int T, int V, int max_rows, hipStream_t st,
                     int* rows_out);
// ride (n > 0; T = 12, V = 17): extra blocks build the forward operand tables of n layers (ftab_ops.h) in the same launch
int launch_first_moments(const float* in, const float* Aw, const float* Tw, const float* in_slope, float* partials, int B, int Ci,
                         int T, int V, float* Zout, int max_rows, hipStream_t st, int* rows_out, const FtabArgs* ride = nullptr);
int launch_first_apply(const float* Z, const float* in, float* out, const float* wfold, const float* bias, const float* in_slope,
                       int B, int Ci, int Co, int TVr, hipStream_t st);
// fwd_moments_bpc.hip
bool fwd_moments_bpc_ok(int T_, int V_, int Ci);
int launch_fwd_moments_bpc(const float* in, const float* Aw, const float* Tw, const float* in_slope, float* partials, int B, int Ci,
                           int T_, int V_, int need_x, float* Zout, hipStream_t st, int* rows_out);
// (the next layer's statistics pass with a commuted layer's combine formed on the way in: commute_layer.hip)
int launch_combine_moments_bpc(const float* Zy, const float* YR, const float* stat, float* U, const float* Aw, const float* Tw,
                               const float* slope, float* partials, int B, int T_, int V_, float* Zout, hipStream_t st, int* rows_out);
// stsgcn_fwd_mfma.hip (instantiated there for the geometries of COSKAD_DISPATCH_TV); 1: the tile does not fit the LDS
template <int T, int V>
int launch_layer_apply_m(const float* in, float* out, const float* Aw, const float* Tw, const float* wfold,
                         const float* bias, const float* in_slope, const float* out_slope, int B, int Ci,
                         int Co, hipStream_t st, const float* Zg);
// eval_layer_clip.hip: the folded layer (16 / 32 input channels) and the first pair 2 -> 32 -> Co, one clip per four-wave workgroup,
// at 8 / 12 / 16 / 24 frames x 17 / 25 joints; at the window lengths 8 / 16 / 24 the launchers check `in` / `out` for 16-byte
// alignment (COSKAD_ERR_ARG) before anything is launched
bool eval_layer_clip_ok(int T_, int V_, int Ci, int Co);
int launch_eval_layer_clip(const float* in, float* out, const float* Aw, const float* Tw, const float* wfold, const float* bias,
                           const float* in_slope, const float* out_slope, int B, int Ci, int Co, int T_, int V_, hipStream_t st);
bool eval_first_pair_clip_ok(int T_, int V_, int Ci, int Cm, int Co);
int launch_eval_first_pair_clip(const float* x, float* out, const float* A1, const float* T1, const float* wfold1,
                                const float* bias1, const float* A2, const float* T2, const float* wfold2, const float* bias2,
                                const float* mid_slope, const float* out_slope, int B, int Co, int T_, int V_, hipStream_t st);
// fused_apply.hip
bool layer_apply_ring_ok(int T_, int V_, int Ci, int Co);
int launch_layer_apply_ring(const float* Z, const float* in, float* out, const float* wfold, const float* bias,
                            const float* in_slope, int B, int Ci, int Co, hipStream_t st);
// fused_apply_bpc.hip
int launch_layer_apply_bpc(const float* Z, const float* in, float* out, const float* wfold, const float* bias,
                           const float* in_slope, int B, int Ci, int Co, hipStream_t st);
// fused_apply_flat.hip
bool layer_apply_flat_ok(int TV_, int Ci, int Co);
int launch_layer_apply_flat(const float* Z, const float* in, float* out, const float* wfold, const float* bias,
                            const float* in_slope, int B, int Ci, int Co, int TV_, hipStream_t st);
// ([Y; R] = [Wt; Wr] PReLU(in), Zy = gcn(Y), per-workgroup row sums of Zy, Zy^2, R, R^2: commute_layer.hip)
int launch_commute_apply_mix(const float* in, float* out, const float* wt, const float* wr, const float* in_slope, const float* Aw,
                             const float* Tw, float* zy, float* mixpart, int B, int Ci, int Jo, int TV_, hipStream_t st, int* rows_out);
// fused_apply_next_bpc.hip: one clip per workgroup for the three layer shapes of the default stack
int apply_next_bpc_rows(int B);
int launch_layer_apply_next_bpc(const float* Z, const float* in, float* out, const float* wfold, const float* bias,
                                const float* in_slope, const float* out_slope, const float* ftab, float* Znext, float* partials,
                                int B, int Ci, int Co, hipStream_t st);
// bottleneck.hip: every reduction of the bottleneck backward in one launch.  fin (part != NULL): one more block turns the P partial
// rows of the one-class head's blocks into stats / acc (k_head_finalize's sums; `block` is set by the launcher)
struct HeadFin {
  const float* part = nullptr;
  int P = 0;
  float scale0 = 0.f;
  float* stats = nullptr;
  float* acc = nullptr;
  unsigned block = 0;
};
int launch_btlnk_reduce(const float* partials, int P, size_t E, float* out, const float* dz, int B, int L, float* db,
                        const float* dap, int nda, float* dslope, int accumulate, hipStream_t stream, const float* rows,
                        int RP, int RE, double* rsum, HeadFin fin = HeadFin());
// btlnk_wide.hip: latents above 64
size_t wide_btlnk_fwd_ws_bytes(int B, int K, int L);
size_t wide_btlnk_bwd_ws_bytes(int B, int K, int L);
int wide_btlnk_fwd(const float* U, const float* W, const float* bias, const float* slope, float* z, void* ws, int B, int K, int L,
                   hipStream_t stream);
int wide_btlnk_bwd(const float* U, const float* W, const float* dz, const float* slope, float* dU, float* dW, float* db,
                   float* dslope, void* ws, int accumulate, int B, int K, int L, hipStream_t stream);
// rev_btlnk_wide.hip: the decoder entry at latents 17 .. 512 (N % 4 == 0), behind coskad_rev_btlnk_{fwd,bwd}_f32; ws in floats
bool wide_rev_btlnk_ok(int N, int L);
size_t wide_rev_btlnk_ws_floats(int B, int N, int L);
int wide_rev_btlnk_fwd(const float* z, const float* W, const float* bias, float* H, int B, int N, int L, hipStream_t stream);
int wide_rev_btlnk_bwd(const float* dH, const float* z, const float* W, float* dz, int dz_accumulate, float* dW, float* db, int accumulate,
                       float* ws, int B, int N, int L, hipStream_t stream);

}  // namespace coskad
