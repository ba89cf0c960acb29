// Space-time mixing of ConvTemporalGraphical for the window lengths 8, 16 and 24 (dataset_seg_len beyond 12).
//
// The tile, block-per-clip and fused kernels of this library are built for T = 12.  A layer with another window length takes
// the composed path (stsgcn.py: wide_forward / wide_backward), and on that path only the mixing and its gradients see (T, V):
//
//   forward    Y[r,q,v] = sum_t X[r,t,v] T[v,t,q],   Z[r,t,w] = sum_v Y[r,t,v] A[t,v,w]
//   adjoint    dY[r,t,v] = sum_w dZ[r,t,w] A[t,v,w], dX[r,t,v] = sum_q dY[r,q,v] T[v,t,q]  (+ add[r,t,v])
//   parameters dA[t,v,w] = sum_r Y[r,t,v] dZ[r,t,w], dT[v,t,q] = sum_r X[r,t,v] dY[r,q,v]
//
// with rows r = (n, c) of T*V contiguous floats.  Everything is v_mfma_f32_16x16x4_f32 (exact fp32) on an LDS image of 16-row
// tiles: the rows are the M side of the two mixes (K = T: 2 / 4 / 6 exact k-steps; K = V padded to a multiple of 4 with ZERO
// operands on both sides) and the K side (four k-steps per tile) of the two outer accumulations.  The joints (temporal mix, dT)
// and the frames (spatial mix, dA) are dealt round-robin to the waves of a workgroup, so that
//   * the mixing kernel keeps the B operands of a wave's joints and frames in its registers and the LDS holds rows alone,
//   * the accumulator tiles of dA / dT are spread over the workgroup (at (24, 25), sixteen waves: 2 frames x 4 tiles + 2 joints x
//     4 tiles = 16 f32x4 per wave), and
//   * a mix that follows an accumulation over the same frame / joint runs in place in the wave that owns it.
// Grids are persistent (grid-stride loop over row tiles).
//
// Determinism: no atomics.  Every workgroup of the parameter kernel writes ONE partial row of T*V*V + V*T*T floats; a second
// kernel sums the rows per column in fp64 in a fixed order (common.h: column_sum_f64).
#include "common.h"
#include "mfma_ops.h"
#include "layer_launch.h"
#include "window_ops.h"

namespace coskad {
namespace {

// Y = gcn(X) or its adjoint on a persistent grid: up to MixRT 16-row tiles per workgroup pass, mixed in place in LDS.  Every wave
// owns the joints v = wave, wave + 8, .. and the frames t = wave, wave + 8, ..; their B operands are loaded once, into registers.
template <int T, int V, bool ADJ>
__global__ __launch_bounds__(kWinBlock, 4) void k_win_gcn(const float* __restrict__ in, float* __restrict__ out,
                                                           const float* __restrict__ Aw, const float* __restrict__ Tw, int rows,
                                                           int vec) {
  using G = WinGeo<T, V>;
  constexpr int TV = G::TV, LD = G::LD, RT = G::MixRT, NR = 16 * RT;
  extern __shared__ float win_smem[];
  float* img = win_smem;
  const int wave = uniform(threadIdx.x >> 6);
  float bT[G::JPW][G::NTT][G::KST], bA[G::FPW][G::NTV][G::KSV];
#pragma unroll
  for (int jn = 0; jn < G::JPW; ++jn) {
    const int v = wave + kWinWaves * jn;
    win_temporal_b<T, V, ADJ>(Tw + (v < V ? v : 0) * T * T, threadIdx.x & 63, bT[jn]);
  }
#pragma unroll
  for (int f = 0; f < G::FPW; ++f) {
    const int t = wave + kWinWaves * f;
    win_spatial_b<T, V, ADJ>(Aw + (t < T ? t : 0) * V * V, threadIdx.x & 63, bA[f]);
  }
  auto temporal = [&]() {
#pragma unroll
    for (int jn = 0; jn < G::JPW; ++jn) {
      const int v = wave + kWinWaves * jn;
      if (kWinWaves * (jn + 1) <= V || v < V) {   // (decided at compile time for all but a ragged last round)
        const int lane = tid_here() & 63;          // LDS addresses formed here, not hoisted out of the tile loop
        for (int rt = 0; rt < RT; ++rt) win_temporal_mix<T, V>(img + rt * G::IMG, img + rt * G::IMG, v, lane, bT[jn]);
      }
    }
  };
  auto spatial = [&]() {
#pragma unroll
    for (int f = 0; f < G::FPW; ++f) {
      const int t = wave + kWinWaves * f;
      if (kWinWaves * (f + 1) <= T || t < T) {
        const int lane = tid_here() & 63;
        for (int rt = 0; rt < RT; ++rt) win_spatial_mix<T, V>(img + rt * G::IMG, img + rt * G::IMG, t, lane, bA[f]);
      }
    }
  };
  const int ntiles = ceil_div(rows, NR);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t r0 = (size_t)tile * NR;
    const int left = rows - tile * NR, nv = left < NR ? left : NR;
    win_load<TV, LD, NR, kWinBlock, G::MixUB>(img, in, r0, nv, vec != 0);
    __syncthreads();
    if constexpr (!ADJ) temporal(); else spatial();
    __syncthreads();
    if constexpr (!ADJ) spatial(); else temporal();
    __syncthreads();
    win_store<TV, LD, NR, kWinBlock>(img, out, nullptr, r0, nv, vec != 0);
    __syncthreads();   // the image is loaded again
  }
}

// dA, dT partial row of this workgroup and (DX) dX = gcn^T(dZ) (+ add), one read of X and dZ.
//   1. X, dZ -> LDS                      2. per joint: Y_v = X_v . T[v] into a third image
//   3. per frame t of this wave: dA[t] += Y_t^T dZ_t, then dY_t = dZ_t . A[t]^T in place
//   4. per joint v of this wave: dT[v] += X_v^T dY_v, then (DX) dX_v = dY_v . T[v]^T in place      5. (DX) image -> dX
// ACT (the stored-Z layer backward of a training layer, float4 rows only): `x` is the PRE-activation of the layer's input with PReLU
// weight in_slope[0].  It is activated on the way into LDS, dX leaves multiplied by PReLU'(x), and the workgroup's share of the slope
// gradient, sum (dX + add) x over x < 0, goes to dap[blockIdx.x].  Without ACT the kernel is what it was.
template <int T, int V, bool DX, bool ACT = false>
__global__ __launch_bounds__((WinGeo<T, V>::ParBlock)) void k_win_params(const float* __restrict__ x, const float* __restrict__ dZ,
                                                                        const float* __restrict__ Aw, const float* __restrict__ Tw,
                                                                        float* __restrict__ partials, float* __restrict__ dX,
                                                                        const float* __restrict__ add, int rows, int vec,
                                                                        const float* __restrict__ in_slope = nullptr,
                                                                        float* __restrict__ dap = nullptr) {
  using G = WinGeo<T, V>;
  constexpr int TV = G::TV, LD = G::LD, RT = G::ParRT, NR = 16 * RT, BLOCK = G::ParBlock, NW = BLOCK / 64;
  constexpr bool TL = G::ParTL;
  constexpr int FPW = (T + NW - 1) / NW, JPW = (V + NW - 1) / NW;   // frames / joints per wave
  constexpr int NTV = G::NTV, NTT = G::NTT;
  extern __shared__ float win_smem[];
  float* imgX = win_smem;
  float* imgD = imgX + RT * G::IMG;
  float* imgY = imgD + RT * G::IMG;
  const float* At = Aw;
  const float* Tt = Tw;
  if constexpr (TL) {
    float* AwL = imgY + RT * G::IMG;
    float* TwL = AwL + G::NA;
    copy_to_lds(AwL, Aw, G::NA);
    copy_to_lds(TwL, Tw, G::NT);
    At = AwL;
    Tt = TwL;
  }
  const int wave = uniform(threadIdx.x >> 6);
  float a_in = 0.f, da = 0.f;
  if constexpr (ACT) a_in = in_slope[0];
  f32x4 accA[FPW][NTV][NTV], accT[JPW][NTT][NTT];
#pragma unroll
  for (int f = 0; f < FPW; ++f)
#pragma unroll
    for (int ta = 0; ta < NTV; ++ta)
#pragma unroll
      for (int tb = 0; tb < NTV; ++tb) accA[f][ta][tb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < JPW; ++j)
#pragma unroll
    for (int ta = 0; ta < NTT; ++ta)
#pragma unroll
      for (int tb = 0; tb < NTT; ++tb) accT[j][ta][tb] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ntiles = ceil_div(rows, NR);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t r0 = (size_t)tile * NR;
    const int left = rows - tile * NR, nv = left < NR ? left : NR;
    const int nrt = (nv + 15) >> 4;          // row tiles with a valid row (the others are skipped, not mixed as zeros)
    if constexpr (ACT) win_load<TV, LD, NR, BLOCK, 2, true>(imgX, x, r0, nv, true, a_in);
    else win_load<TV, LD, NR, BLOCK, 2>(imgX, x, r0, nv, vec != 0);
    win_load<TV, LD, NR, BLOCK, 2>(imgD, dZ, r0, nv, vec != 0);
    __syncthreads();   // (the first pass: the tables too)
    for (int it = wave; it < nrt * V; it += NW) {
      const int rt = it / V, v = it - rt * V;
      win_temporal<T, V, false>(imgX + rt * G::IMG, imgY + rt * G::IMG, Tt + v * T * T, v, tid_here() & 63);
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < FPW; ++f) {
      // (tid_here: the lane's LDS addresses are formed here, per frame, not hoisted out of the tile loop and held in VGPRs)
      const int lane = tid_here() & 63, i = lane & 15, k = lane >> 4;
      const int t = wave + NW * f;
      if (NW * (f + 1) <= T || t < T) {   // (decided at compile time for all but a ragged last round)
        for (int rt = 0; rt < nrt; ++rt) {
          const float* yi = imgY + rt * G::IMG;
          const float* zi = imgD + rt * G::IMG;
#pragma unroll
          for (int s = 0; s < 4; ++s) {   // K = the tile's 16 rows (absent rows are zeros)
            const int row = 4 * s + k;
            float a[NTV], b[NTV];
#pragma unroll
            for (int ta = 0; ta < NTV; ++ta) {
              const int j = 16 * ta + i;
              const int o = row * LD + t * V + (j < V ? j : 0);
              const float yv = yi[o], zv = zi[o];
              a[ta] = j < V ? yv : 0.f;
              b[ta] = j < V ? zv : 0.f;
            }
#pragma unroll
            for (int ta = 0; ta < NTV; ++ta)
#pragma unroll
              for (int tb = 0; tb < NTV; ++tb) accA[f][ta][tb] = mfma4(a[ta], b[tb], accA[f][ta][tb]);
          }
        }
        float bm[NTV][G::KSV];
        win_spatial_b<T, V, true>(At + t * V * V, lane, bm);
        for (int rt = 0; rt < nrt; ++rt) win_spatial_mix<T, V>(imgD + rt * G::IMG, imgD + rt * G::IMG, t, lane, bm);
      }
      __builtin_amdgcn_sched_barrier(0);   // one frame's operands at a time: the accumulators own the register file
    }
    __syncthreads();
#pragma unroll
    for (int jn = 0; jn < JPW; ++jn) {
      const int lane = tid_here() & 63, i = lane & 15, k = lane >> 4;
      const int v = wave + NW * jn;
      if (NW * (jn + 1) <= V || v < V) {
        for (int rt = 0; rt < nrt; ++rt) {
          const float* xi = imgX + rt * G::IMG;
          const float* yi = imgD + rt * G::IMG;
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const int row = 4 * s + k;
            float a[NTT], b[NTT];
#pragma unroll
            for (int ta = 0; ta < NTT; ++ta) {
              const int j = 16 * ta + i;
              const int o = row * LD + (j < T ? j : 0) * V + v;
              const float xv = xi[o], yv = yi[o];
              a[ta] = j < T ? xv : 0.f;
              b[ta] = j < T ? yv : 0.f;
            }
#pragma unroll
            for (int ta = 0; ta < NTT; ++ta)
#pragma unroll
              for (int tb = 0; tb < NTT; ++tb) accT[jn][ta][tb] = mfma4(a[ta], b[tb], accT[jn][ta][tb]);
          }
        }
        if constexpr (DX) {
          float bm[NTT][G::KST];
          win_temporal_b<T, V, true>(Tt + v * T * T, lane, bm);
          for (int rt = 0; rt < nrt; ++rt) win_temporal_mix<T, V>(imgD + rt * G::IMG, imgD + rt * G::IMG, v, lane, bm);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    if constexpr (DX) {
      if constexpr (ACT) da += win_store_act<TV, LD, NR, BLOCK>(imgD, dX, add, x, r0, nv, a_in);
      else win_store<TV, LD, NR, BLOCK>(imgD, dX, add, r0, nv, vec != 0);
      __syncthreads();   // the images are loaded again
    }
  }
  if constexpr (ACT && DX) {
    // the slope-gradient share: lanes -> waves -> one float, in a fixed order (the images are dead: every tile ended with a barrier)
    da = wave_sum(da);
    if ((threadIdx.x & 63) == 0) imgX[threadIdx.x >> 6] = da;
    __syncthreads();
    if (threadIdx.x == 0 && dap) {
      float t = 0.f;
      for (int w = 0; w < NW; ++w) t += imgX[w];
      dap[blockIdx.x] = t;
    }
  }

  // D[row = 4k + r][col = i] of tile (ta, tb)
  const int lane = threadIdx.x & 63, i = lane & 15, k = lane >> 4;
  float* prow = partials + (size_t)blockIdx.x * G::E;
#pragma unroll
  for (int f = 0; f < FPW; ++f) {
    const int t = wave + NW * f;
    if (t < T) {
#pragma unroll
      for (int ta = 0; ta < NTV; ++ta)
#pragma unroll
        for (int tb = 0; tb < NTV; ++tb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int v = 16 * ta + 4 * k + r, w = 16 * tb + i;
            if (v < V && w < V) prow[t * V * V + v * V + w] = accA[f][ta][tb][r];
          }
    }
  }
#pragma unroll
  for (int jn = 0; jn < JPW; ++jn) {
    const int v = wave + NW * jn;
    if (v < V) {
#pragma unroll
      for (int ta = 0; ta < NTT; ++ta)
#pragma unroll
        for (int tb = 0; tb < NTT; ++tb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int t = 16 * ta + 4 * k + r, q = 16 * tb + i;
            if (t < T && q < T) prow[G::NA + v * T * T + t * T + q] = accT[jn][ta][tb][r];
          }
    }
  }
}

// [dA | dT] (+)= the column sums of P partial rows: 64 columns x 16 row slices per block, fp64, fixed order
__global__ __launch_bounds__(1024) void k_win_reduce(const float* __restrict__ partials, int P, int E, int nA,
                                                      float* __restrict__ dA, float* __restrict__ dT, int accumulate) {
  __shared__ double sh[1024];
  const int e = blockIdx.x * 64 + (threadIdx.x % 64);
  const double t = column_sum_f64<64>(partials, P, (size_t)E, e, e < E, sh);
  if (threadIdx.x < 64 && e < E) {
    float* o = e < nA ? dA + e : dT + (e - nA);
    *o = accumulate ? *o + (float)t : (float)t;
  }
}

template <int T, int V>
int launch_win_gcn(const float* in, float* out, const float* Aw, const float* Tw, int rows, int adjoint, hipStream_t st) {
  using G = WinGeo<T, V>;
  constexpr int kGridCap = 512;   // persistent: two workgroups per CU
  const size_t lds = (size_t)G::MixLds * sizeof(float);
  const int ntiles = ceil_div(rows, 16 * G::MixRT);
  const int grid = ntiles < kGridCap ? ntiles : kGridCap;
  const int vec = aligned16(in) && aligned16(out);
  if (adjoint) return launch_lds<k_win_gcn<T, V, true>>("gcn (window)", dim3(grid), dim3(kWinBlock), lds, st, in, out, Aw, Tw, rows, vec);
  return launch_lds<k_win_gcn<T, V, false>>("gcn (window)", dim3(grid), dim3(kWinBlock), lds, st, in, out, Aw, Tw, rows, vec);
}

// in_slope != NULL: the ACT form (16-byte aligned rows; 17 / 25 joints); dap: its slope-gradient partials, one per workgroup;
// *rows_out: the workgroups launched
template <int T, int V>
int launch_win_params(const float* x, const float* dZ, const float* Aw, const float* Tw, float* dA, float* dT, void* ws,
                      int accumulate, int rows, hipStream_t st, float* dX, const float* add, const float* in_slope, float* dap,
                      int* rows_out) {
  using G = WinGeo<T, V>;
  const size_t lds = (size_t)G::ParLds * sizeof(float);
  const int ntiles = ceil_div(rows, 16 * G::ParRT);
  const int grid = ntiles < G::ParGrid ? ntiles : G::ParGrid;
  float* partials = reinterpret_cast<float*>(ws);
  const int vec = aligned16(x) && aligned16(dZ) && aligned16(dX) && aligned16(add);   // (NULL counts as aligned)
  int rc;
  if (rows_out) *rows_out = grid;
#define LAUNCH_WP(DX, ACT, SLOPE, DAP)                                                                                                  \
  rc = launch_lds<k_win_params<T, V, DX, ACT>>("gcn_bwd_params (window)", dim3(grid), dim3(G::ParBlock), lds, st, x, dZ, Aw, Tw, partials, dX, \
                                               add, rows, vec, SLOPE, DAP)
  if (in_slope) {
    if constexpr (V == 17 || V == 25) {
      if (!vec) return fail(COSKAD_ERR_ARG, "gcn_bwd_params (window): the activating form needs 16-byte aligned rows");
      if (dX) LAUNCH_WP(true, true, in_slope, dap);
      else LAUNCH_WP(false, true, in_slope, dap);
    } else {
      return fail(COSKAD_ERR_SHAPE, "gcn_bwd_params (window): the activating form is built for 17 / 25 joints");
    }
  } else if (dX) {
    LAUNCH_WP(true, false, (const float*)nullptr, (float*)nullptr);
  } else {
    LAUNCH_WP(false, false, (const float*)nullptr, (float*)nullptr);
  }
#undef LAUNCH_WP
  if (rc) return rc;
  hipLaunchKernelGGL(k_win_reduce, dim3(ceil_div(G::E, 64)), dim3(1024), 0, st, partials, grid, G::E, G::NA, dA, dT, accumulate);
  return check_launch("gcn_bwd_params (window)");
}

// the twelve geometries of coskad_window_ok
#define COSKAD_WINDOW_V(T_, V_, CALL)            \
  do {                                           \
    if ((V_) == 17) { CALL(T_, 17); }            \
    else if ((V_) == 25) { CALL(T_, 25); }       \
    else if ((V_) == 14) { CALL(T_, 14); }       \
    else if ((V_) == 18) { CALL(T_, 18); }       \
  } while (0)
#define COSKAD_DISPATCH_WINDOW(T_, V_, CALL)                 \
  do {                                                       \
    if ((T_) == 8) COSKAD_WINDOW_V(8, V_, CALL);             \
    else if ((T_) == 16) COSKAD_WINDOW_V(16, V_, CALL);      \
    else if ((T_) == 24) COSKAD_WINDOW_V(24, V_, CALL);      \
    return fail(COSKAD_ERR_SHAPE, "unsupported window geometry (n_frames=%d, n_joints=%d)", (T_), (V_)); \
  } while (0)

}  // namespace

size_t window_params_ws_bytes(int T, int V) {
#define CALL(T_, V_) return (size_t)WinGeo<T_, V_>::ParGrid * WinGeo<T_, V_>::E * sizeof(float)
  do {
    if (T == 8) COSKAD_WINDOW_V(8, V, CALL);
    else if (T == 16) COSKAD_WINDOW_V(16, V, CALL);
    else if (T == 24) COSKAD_WINDOW_V(24, V, CALL);
  } while (0);
#undef CALL
  return 0;
}

int launch_window_gcn(const float* in, float* out, const float* Aw, const float* Tw, int rows, int T, int V, int adjoint,
                      hipStream_t st) {
#define CALL(T_, V_) return launch_win_gcn<T_, V_>(in, out, Aw, Tw, rows, adjoint, st)
  COSKAD_DISPATCH_WINDOW(T, V, CALL);
#undef CALL
}

int launch_window_params(const float* x, const float* dZ, const float* Aw, const float* Tw, float* dA, float* dT, void* ws,
                         int accumulate, int rows, int T, int V, hipStream_t st, float* dX, const float* add, const float* in_slope,
                         float* dap, int* rows_out) {
#define CALL(T_, V_) return launch_win_params<T_, V_>(x, dZ, Aw, Tw, dA, dT, ws, accumulate, rows, st, dX, add, in_slope, dap, rows_out)
  COSKAD_DISPATCH_WINDOW(T, V, CALL);
#undef CALL
}

}  // namespace coskad

extern "C" {

/* 1 for the window lengths that have mixing kernels only (T in {8, 16, 24}, V in {14, 17, 18, 25}): layers of such a model
 * take the composed path.  0 otherwise, T = 12 (the tile kernels' own geometry) included.  Host arithmetic. */
int coskad_window_ok(int T, int V) {
  return (T == 8 || T == 16 || T == 24) && (V == 14 || V == 17 || V == 18 || V == 25);
}

}  // extern "C"
