// The statistics pass of a TRAINING layer at the window lengths 8, 16 and 24 (17 / 25 joints; 2, 4, 16 or 32 input channels):
//     X = PReLU_in(in),  Z = gcn(X) -> Zout,  one partial row [sum x x^T | sum x | sum z z^T | sum z] per workgroup
// (reference: models/graph_layers/stsgcn.py:56-80 and the batch statistics of both BatchNorms, 94-110; the moment form is the one of
// stsgcn_train.hip, whose launch_reduce_fold finishes the pass unchanged).
//
// The mixing is gcn_window.hip's: 16-row tiles of rows (clip, channel) in LDS, the joints and frames dealt round-robin to the eight
// waves, a wave's B operands of both mixes in its registers for the whole launch, K = V zero-padded to whole k-steps on both operands
// (window_ops.h).  A workgroup pass takes RT row tiles = whole clips (RT even, so that a 32-channel clip's two tiles travel together).
// The Gram sums run over FLAT positions of the same image, before (X) and after (Z) the mixing: K = positions, four per k-step, the
// k-steps dealt to the waves; the A and the B operand of a diagonal tile are the same register.  With two (four) input channels a row
// tile holds eight (four) clips: the 16 x 16 tile Gram is accumulated as it is and its eight 2 x 2 (four 4 x 4) diagonal blocks are
// added at the end.
//
// Determinism: no atomics.  The waves add their accumulators into one LDS row one after another, the row leaves as the workgroup's
// partial row, launch_reduce_partials sums the rows in fp64 in a fixed order.  Rows beyond the batch are zeros in LDS.
#include "common.h"
#include "mfma_ops.h"
#include "layer_launch.h"
#include "window_ops.h"

namespace coskad {
namespace {

constexpr int kMomGrid = 512;   // persistent workgroups = partial rows (<= kMaxGrid of stsgcn_train.hip's workspace): two per CU

template <int T, int V>
struct MomGeo {
  using G = WinGeo<T, V>;
  static constexpr int RT = (kLdsFloats / 2) / G::IMG >= 4 ? 4 : 2;   // row tiles per pass (even), within half the LDS
  static_assert(RT * G::IMG <= kLdsFloats / 2, "statistics pass: two row tiles exceed half the LDS");
  static constexpr int Lds = RT * G::IMG;
  // registers of a wave's mixing operands: beyond 64 the kernel is compiled for two waves per SIMD
  static constexpr int Ops = G::JPW * G::NTT * G::KST + G::FPW * G::NTV * G::KSV;
};

template <int T, int V, int CI>
__global__ __launch_bounds__(kWinBlock, (MomGeo<T, V>::Ops > 64 ? 2 : 4)) void k_win_moments(
    const float* __restrict__ in, const float* __restrict__ Aw, const float* __restrict__ Tw, const float* __restrict__ in_slope,
    float* __restrict__ partials, float* __restrict__ Zout, int rows, int need_x) {
  using G = WinGeo<T, V>;
  constexpr int TV = G::TV, LD = G::LD, RT = MomGeo<T, V>::RT, NR = 16 * RT;
  constexpr int ROWS = CI == 32 ? 32 : 16;        // rows of one Gram image: a clip of 16 / 32 channels, or 16 / CI clips of two / four
  constexpr int NACC = CI == 32 ? 3 : 1;          // tiles 00, 01, 11 (symmetric) or the one tile
  constexpr int NS = CI == 32 ? 2 : 1;
  constexpr int GF = ROWS * ROWS + ROWS;          // floats of one Gram + row sums in the final LDS row
  static_assert(CI == 2 || CI == 4 || CI == 16 || CI == 32, "built for 2, 4, 16 and 32 input channels");
  static_assert(2 * GF <= RT * G::IMG, "the final row is aliased onto the image");
  extern __shared__ float win_smem[];
  float* img = win_smem;
  const int wave = uniform(threadIdx.x >> 6);
  const bool pre = in_slope != nullptr;
  const float a_in = pre ? in_slope[0] : 0.f;
  float bT[G::JPW][G::NTT][G::KST], bA[G::FPW][G::NTV][G::KSV];
#pragma unroll
  for (int jn = 0; jn < G::JPW; ++jn) {
    const int v = wave + kWinWaves * jn;
    win_temporal_b<T, V, false>(Tw + (v < V ? v : 0) * T * T, threadIdx.x & 63, bT[jn]);
  }
#pragma unroll
  for (int f = 0; f < G::FPW; ++f) {
    const int t = wave + kWinWaves * f;
    win_spatial_b<T, V, false>(Aw + (t < T ? t : 0) * V * V, threadIdx.x & 63, bA[f]);
  }
  f32x4 gx[NACC], gz[NACC];
  float sx[NS], sz[NS];
#pragma unroll
  for (int a = 0; a < NACC; ++a) { gx[a] = f32x4{0.f, 0.f, 0.f, 0.f}; gz[a] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int a = 0; a < NS; ++a) { sx[a] = 0.f; sz[a] = 0.f; }

  // Gram sums of the image's row tiles over this wave's k-steps (positions 4 ks .. 4 ks + 3, ks = wave, wave + 8, ..)
  auto gram = [&](f32x4 (&g)[NACC], float (&s)[NS]) {
    const int lane = tid_here() & 63, i = lane & 15, k = lane >> 4;
    for (int ks = wave; ks < TV / 4; ks += kWinWaves) {
      const float* p = img + i * LD + 4 * ks + k;
      if constexpr (CI == 32) {
#pragma unroll
        for (int rt = 0; rt < RT; rt += 2) {
          const float a0 = p[rt * G::IMG], a1 = p[(rt + 1) * G::IMG];
          g[0] = mfma4(a0, a0, g[0]);
          g[1] = mfma4(a0, a1, g[1]);
          g[2] = mfma4(a1, a1, g[2]);
          s[0] += a0;
          s[1] += a1;
        }
      } else {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const float a0 = p[rt * G::IMG];
          g[0] = mfma4(a0, a0, g[0]);
          s[0] += a0;
        }
      }
    }
  };

  const int ntiles = ceil_div(rows, NR);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const size_t r0 = (size_t)tile * NR;
    const int left = rows - tile * NR, nv = left < NR ? left : NR;
    if (pre) win_load<TV, LD, NR, kWinBlock, G::MixUB, true>(img, in, r0, nv, true, a_in);
    else win_load<TV, LD, NR, kWinBlock, G::MixUB>(img, in, r0, nv, true);
    __syncthreads();
    if (need_x) {
      gram(gx, sx);
      __syncthreads();   // every wave has read X: the mixing overwrites it
    }
#pragma unroll
    for (int jn = 0; jn < G::JPW; ++jn) {
      const int v = wave + kWinWaves * jn;
      if (kWinWaves * (jn + 1) <= V || v < V) {   // (decided at compile time for all but a ragged last round)
        const int lane = tid_here() & 63;
        for (int rt = 0; rt < RT; ++rt) win_temporal_mix<T, V>(img + rt * G::IMG, img + rt * G::IMG, v, lane, bT[jn]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int f = 0; f < G::FPW; ++f) {
      const int t = wave + kWinWaves * f;
      if (kWinWaves * (f + 1) <= T || t < T) {
        const int lane = tid_here() & 63;
        for (int rt = 0; rt < RT; ++rt) win_spatial_mix<T, V>(img + rt * G::IMG, img + rt * G::IMG, t, lane, bA[f]);
      }
    }
    __syncthreads();     // the image holds Z
    if (Zout) win_store<TV, LD, NR, kWinBlock>(img, Zout, nullptr, r0, nv, true);
    gram(gz, sz);
    __syncthreads();     // the image is loaded again
  }

  // the waves add their accumulators into one row in LDS, one after another (fixed order): [Gram X ROWS^2][sums X ROWS][Gram Z][sums Z]
  float* row = img;
  const int lane = threadIdx.x & 63, i = lane & 15, k = lane >> 4;
  auto put = [&](int w, float* base, const f32x4 (&g)[NACC], const float (&s)[NS]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {                          // D layout: register r <-> row 4 k + r, column i
      const int m = 4 * k + r;
      if constexpr (CI == 32) {
        float* p00 = base + m * ROWS + i;
        float* p01 = base + m * ROWS + 16 + i;
        float* p10 = base + (16 + i) * ROWS + m;
        float* p11 = base + (16 + m) * ROWS + 16 + i;
        p00[0] = (w ? p00[0] : 0.f) + g[0][r];
        p01[0] = (w ? p01[0] : 0.f) + g[1][r];
        p10[0] = (w ? p10[0] : 0.f) + g[1][r];
        p11[0] = (w ? p11[0] : 0.f) + g[NACC - 1][r];
      } else {
        float* p = base + m * ROWS + i;
        p[0] = (w ? p[0] : 0.f) + g[0][r];
      }
    }
#pragma unroll
    for (int a = 0; a < NS; ++a) {
      float t = s[a];
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      if (k == 0) {
        float* p = base + ROWS * ROWS + 16 * a + i;
        p[0] = (w ? p[0] : 0.f) + t;
      }
    }
  };
  for (int w = 0; w < kWinWaves; ++w) {
    if (wave == w) {
      put(w, row, gx, sx);
      put(w, row + GF, gz, sz);
    }
    __syncthreads();
  }
  // partial row: [MX CI^2][sumX CI][MZ CI^2][sumZ CI]
  constexpr int EH = CI * CI + CI;
  float* dst = partials + (size_t)blockIdx.x * (2 * EH);
  if constexpr (CI < 16) {                         // the tile's 16 / CI clips: their diagonal blocks, one after another (fixed order)
    if (threadIdx.x < 2 * EH) {
      const int which = threadIdx.x / EH, e = threadIdx.x - which * EH;
      const float* base = row + which * GF;
      float t = 0.f;
      for (int b = 0; b < 16 / CI; ++b)
        t += e < CI * CI ? base[(CI * b + e / CI) * ROWS + CI * b + e % CI] : base[ROWS * ROWS + CI * b + (e - CI * CI)];
      dst[threadIdx.x] = t;
    }
  } else {
    for (int e = threadIdx.x; e < 2 * EH; e += kWinBlock) dst[e] = row[e];   // (ROWS == CI: the LDS row has the partial row's layout)
  }
}

template <int T, int V>
int launch_win_moments(const float* in, const float* Aw, const float* Tw, const float* in_slope, float* partials, int B, int Ci,
                       int need_x, float* Zout, hipStream_t st, int* rows_out) {
  using M = MomGeo<T, V>;
  const size_t lds = (size_t)M::Lds * sizeof(float);
  const int rows = B * Ci;
  const int ntiles = ceil_div(rows, 16 * M::RT);
  const int grid = ntiles < kMomGrid ? ntiles : kMomGrid;
  *rows_out = grid;
#define LAUNCH_MOM(CI)                                                                                                    \
  return launch_lds<k_win_moments<T, V, CI>>("fwd_moments (window)", dim3(grid), dim3(kWinBlock), lds, st, in, Aw, Tw, in_slope, \
                                             partials, Zout, rows, need_x)
  ProbeScope probe(KID_FWD_MOMENTS, Ci, Ci, st);
  if (Ci == 2) LAUNCH_MOM(2);
  else if (Ci == 4) LAUNCH_MOM(4);
  else if (Ci == 16) LAUNCH_MOM(16);
  else LAUNCH_MOM(32);
#undef LAUNCH_MOM
}

#define COSKAD_TRAIN_WINDOW_TV(T_, V_, CALL)                              \
  do {                                                                    \
    if ((T_) == 8 && (V_) == 17) { CALL(8, 17); }                         \
    else if ((T_) == 8 && (V_) == 25) { CALL(8, 25); }                    \
    else if ((T_) == 16 && (V_) == 17) { CALL(16, 17); }                  \
    else if ((T_) == 16 && (V_) == 25) { CALL(16, 25); }                  \
    else if ((T_) == 24 && (V_) == 17) { CALL(24, 17); }                  \
    else if ((T_) == 24 && (V_) == 25) { CALL(24, 25); }                  \
  } while (0)

}  // namespace

bool window_moments_ok(int T, int V, int Ci) {
  return (T == 8 || T == 16 || T == 24) && (V == 17 || V == 25) && (Ci == 2 || Ci == 4 || Ci == 16 || Ci == 32);
}

int launch_window_moments(const float* in, const float* Aw, const float* Tw, const float* in_slope, float* partials, int B, int Ci,
                          int T, int V, int need_x, float* Zout, hipStream_t st, int* rows_out) {
  if (!window_moments_ok(T, V, Ci))
    return fail(COSKAD_ERR_SHAPE, "train moments (window): unsupported (n_frames=%d, n_joints=%d, C_in=%d)", T, V, Ci);
#define CALL(T_, V_) return launch_win_moments<T_, V_>(in, Aw, Tw, in_slope, partials, B, Ci, need_x, Zout, st, rows_out)
  COSKAD_TRAIN_WINDOW_TV(T, V, CALL);
#undef CALL
  return fail(COSKAD_ERR_SHAPE, "train moments (window): unsupported geometry");
}

}  // namespace coskad
