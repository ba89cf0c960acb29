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

namespace coskad {
namespace {

constexpr int kWinBlock = 512;            // eight waves
constexpr int kWinWaves = kWinBlock / 64;
constexpr int kLdsFloats = kMaxLdsBytes / 4;

template <int T, int V>
struct WinGeo {
  static_assert(T % 4 == 0, "the window length is the K side of the temporal mix: whole k-steps");
  static constexpr int TV = T * V;
  static constexpr int LD = TV + 1;              // (TV is even) odd row stride: rows <-> lanes and positions <-> lanes without bank conflicts
  static constexpr int IMG = 16 * LD;            // floats of one 16-row tile image
  static constexpr int NA = T * V * V, NT = V * T * T, E = NA + NT;
  static constexpr int KST = T / 4, NTT = (T + 15) / 16;          // temporal mix: k-steps, 16-column tiles
  static constexpr int KSV = (V + 3) / 4, NTV = (V + 15) / 16;    // spatial mix
  static constexpr int FPW = (T + kWinWaves - 1) / kWinWaves, JPW = (V + kWinWaves - 1) / kWinWaves;   // frames / joints per wave of the mixing kernel
  // mixing kernel: the B operands of a wave's frames and joints stay in its registers (<= 90 at (24, 25)), the LDS holds the row
  // image alone: up to four row tiles per workgroup pass, within half the LDS so that two workgroups share a CU
  static constexpr int MixRT = (kLdsFloats / 2) / IMG < 4 ? (kLdsFloats / 2) / IMG : 4;
  static_assert(MixRT >= 1, "mixing kernel: one row tile exceeds half the LDS");
  static constexpr int MixLds = MixRT * IMG;
  static constexpr int MixUB = JPW * NTT * KST + FPW * NTV * KSV > 64 ? 2 : 4;   // float4 loads in flight: what the operands leave room for
  // parameter kernel: images of X, dZ (-> dY -> dX) and Y of ParRT row tiles; the tables join them in LDS where they fit beside one
  // tile of each ((24, 25): 28 848 + 29 400 floats do not -- its B operands come from global memory, i.e. from L2).  Where two
  // workgroups share a CU they are eight waves each; where one workgroup takes more than half the LDS it is sixteen waves, so that
  // the CU still runs four waves per SIMD and a wave holds half the accumulator tiles.
  static constexpr bool ParTL = 3 * IMG + E <= kLdsFloats;
  static constexpr int ParTab = ParTL ? E : 0;
  static constexpr bool ParOne = 3 * IMG + ParTab > kLdsFloats / 2;
  static constexpr int ParBlock = ParOne ? 1024 : 512;
  static constexpr int ParRTmax = ((ParOne ? kLdsFloats : kLdsFloats / 2) - ParTab) / (3 * IMG);
  static constexpr int ParRT = ParRTmax < 4 ? ParRTmax : 4;
  static_assert(ParRT >= 1, "parameter kernel: three images exceed the LDS");
  static constexpr int ParLds = 3 * ParRT * IMG + ParTab;
  // persistent grid of the parameter kernel = partial rows of its workspace
  static constexpr int ParGrid = ParOne ? 256 : 512;
};

// B operand of the temporal mix of joint v for this lane: tb = T[v][T][T]; columns >= T are zeros.
//   forward: B[k = t][j = q] = T[v][t][q];  adjoint: B[k = q][j = t] = T[v][t][q]
template <int T, int V, bool ADJ>
__device__ __forceinline__ void win_temporal_b(const float* tb, int lane, float (&b)[WinGeo<T, V>::NTT][WinGeo<T, V>::KST]) {
  const int i = lane & 15, k = lane >> 4;
#pragma unroll
  for (int nt = 0; nt < WinGeo<T, V>::NTT; ++nt) {
    const int col = 16 * nt + i;
    const int cc = col < T ? col : 0;
#pragma unroll
    for (int s = 0; s < WinGeo<T, V>::KST; ++s) {
      const int kk = 4 * s + k;
      const float tv = ADJ ? tb[cc * T + kk] : tb[kk * T + cc];
      b[nt][s] = col < T ? tv : 0.f;
    }
  }
}

// 16 rows x (frames of joint v) . B  ->  dst (may be src: every operand is in registers before the first store, and a
// wave's LDS accesses complete in order).
template <int T, int V>
__device__ __forceinline__ void win_temporal_mix(const float* src, float* dst, int v, int lane,
                                                 const float (&b)[WinGeo<T, V>::NTT][WinGeo<T, V>::KST]) {
  constexpr int LD = WinGeo<T, V>::LD, KS = WinGeo<T, V>::KST, NT = WinGeo<T, V>::NTT;
  const int i = lane & 15, k = lane >> 4;
  float a[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) a[s] = src[i * LD + (4 * s + k) * V + v];
  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) acc[nt] = mfma4(a[s], b[nt][s], acc[nt]);
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int col = 16 * nt + i;
    if (col < T) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(4 * k + r) * LD + col * V + v] = acc[nt][r];
    }
  }
}

template <int T, int V, bool ADJ>
__device__ __forceinline__ void win_temporal(const float* src, float* dst, const float* tb, int v, int lane) {
  float b[WinGeo<T, V>::NTT][WinGeo<T, V>::KST];
  win_temporal_b<T, V, ADJ>(tb, lane, b);
  win_temporal_mix<T, V>(src, dst, v, lane, b);
}

// B operand of the spatial mix of frame t for this lane: ab = A[t][V][V].  K = V is padded to whole k-steps with zeros on BOTH
// operands: neither the image next to the frame nor the table next to A[t] is read.
//   forward: B[k = v][j = w] = A[t][v][w];  adjoint: B[k = w][j = v] = A[t][v][w]
template <int T, int V, bool ADJ>
__device__ __forceinline__ void win_spatial_b(const float* ab, int lane, float (&b)[WinGeo<T, V>::NTV][WinGeo<T, V>::KSV]) {
  const int i = lane & 15, k = lane >> 4;
#pragma unroll
  for (int nt = 0; nt < WinGeo<T, V>::NTV; ++nt) {
    const int col = 16 * nt + i;
    const int cc = col < V ? col : 0;
#pragma unroll
    for (int s = 0; s < WinGeo<T, V>::KSV; ++s) {
      const int kk = 4 * s + k;
      const int kc = kk < V ? kk : 0;
      const float av = ADJ ? ab[cc * V + kc] : ab[kc * V + cc];
      b[nt][s] = (col < V && kk < V) ? av : 0.f;
    }
  }
}

// 16 rows x (joints of frame t) . B  ->  dst (may be src)
template <int T, int V>
__device__ __forceinline__ void win_spatial_mix(const float* src, float* dst, int t, int lane,
                                                const float (&b)[WinGeo<T, V>::NTV][WinGeo<T, V>::KSV]) {
  constexpr int LD = WinGeo<T, V>::LD, KS = WinGeo<T, V>::KSV, NT = WinGeo<T, V>::NTV;
  const int i = lane & 15, k = lane >> 4;
  float a[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int kk = 4 * s + k;
    const float xv = src[i * LD + t * V + (kk < V ? kk : 0)];
    a[s] = kk < V ? xv : 0.f;
  }
  f32x4 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < KS; ++s) acc[nt] = mfma4(a[s], b[nt][s], acc[nt]);
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int col = 16 * nt + i;
    if (col < V) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(4 * k + r) * LD + t * V + col] = acc[nt][r];
    }
  }
}

// LDS image of NR rows starting at global row r0; rows beyond the nv valid ones are zeros.  vec: the tile is 16-byte aligned
// (T*V is a multiple of 4, so the tensor's base decides) -> float4 loads, UB in flight per thread.
template <int TV, int LD, int NR, int BLOCK, int UB>
__device__ __forceinline__ void win_load(float* img, const float* __restrict__ g, size_t r0, int nv, bool vec) {
  static_assert(TV % 4 == 0, "a float4 stays inside one row");
  const float* base = g + r0 * TV;
  if (vec) {
    const float4* g4 = reinterpret_cast<const float4*>(base);
    constexpr int N4 = NR * TV / 4;
    const int n4 = nv * (TV / 4);
    for (int i0 = threadIdx.x; i0 < N4; i0 += UB * BLOCK) {
      float4 v[UB];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int i = i0 + u * BLOCK;
        v[u] = i < n4 ? g4[i] : float4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const int i = i0 + u * BLOCK;
        if (i < N4) {
          const int e = 4 * i, r = e / TV, p = e - r * TV;
          float* d = img + r * LD + p;
          d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
        }
      }
    }
  } else {
    for (int e = threadIdx.x; e < NR * TV; e += BLOCK) {
      const int r = e / TV, p = e - r * TV;
      img[r * LD + p] = r < nv ? base[e] : 0.f;
    }
  }
}

// the nv valid rows of the LDS image (+ add) -> global rows r0..
template <int TV, int LD, int NR, int BLOCK>
__device__ __forceinline__ void win_store(const float* img, float* __restrict__ g, const float* __restrict__ add, size_t r0, int nv,
                                          bool vec) {
  float* ob = g + r0 * TV;
  const float* ab = add ? add + r0 * TV : nullptr;
  if (vec) {
    float4* o4 = reinterpret_cast<float4*>(ob);
    const float4* a4 = reinterpret_cast<const float4*>(ab);
    const int n4 = nv * (TV / 4);
    for (int i = threadIdx.x; i < n4; i += BLOCK) {
      const int e = 4 * i, r = e / TV, p = e - r * TV;
      const float* s = img + r * LD + p;
      float4 o = float4{s[0], s[1], s[2], s[3]};
      if (a4) { const float4 q = a4[i]; o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w; }
      o4[i] = o;
    }
  } else {
    for (int e = threadIdx.x; e < nv * TV; e += BLOCK) {
      const int r = e / TV, p = e - r * TV;
      ob[e] = ab ? img[r * LD + p] + ab[e] : img[r * LD + p];
    }
  }
}

__host__ inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

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
template <int T, int V, bool DX>
__global__ __launch_bounds__((WinGeo<T, V>::ParBlock)) void k_win_params(const float* __restrict__ x, const float* __restrict__ dZ,
                                                                        const float* __restrict__ Aw, const float* __restrict__ Tw,
                                                                        float* __restrict__ partials, float* __restrict__ dX,
                                                                        const float* __restrict__ add, int rows, int vec) {
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
    win_load<TV, LD, NR, BLOCK, 2>(imgX, x, r0, nv, vec != 0);
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
      win_store<TV, LD, NR, BLOCK>(imgD, dX, add, r0, nv, vec != 0);
      __syncthreads();   // the images are loaded again
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

template <class K>
int set_lds(K k, size_t lds) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail(COSKAD_ERR_LAUNCH, "window mixing: %zu B of LDS refused", lds);
  return COSKAD_OK;
}

template <int T, int V>
int launch_win_gcn(const float* in, float* out, const float* Aw, const float* Tw, int rows, int adjoint, hipStream_t st) {
  using G = WinGeo<T, V>;
  constexpr int kGridCap = 512;   // persistent: two workgroups per CU
  const size_t lds = (size_t)G::MixLds * sizeof(float);
  const int ntiles = ceil_div(rows, 16 * G::MixRT);
  const int grid = ntiles < kGridCap ? ntiles : kGridCap;
  const int vec = aligned16(in) && aligned16(out);
  int rc;
  if (adjoint) {
    if ((rc = set_lds(k_win_gcn<T, V, true>, lds))) return rc;
    hipLaunchKernelGGL((k_win_gcn<T, V, true>), dim3(grid), dim3(kWinBlock), lds, st, in, out, Aw, Tw, rows, vec);
  } else {
    if ((rc = set_lds(k_win_gcn<T, V, false>, lds))) return rc;
    hipLaunchKernelGGL((k_win_gcn<T, V, false>), dim3(grid), dim3(kWinBlock), lds, st, in, out, Aw, Tw, rows, vec);
  }
  return check_launch("gcn (window)");
}

template <int T, int V>
int launch_win_params(const float* x, const float* dZ, const float* Aw, const float* Tw, float* dA, float* dT, void* ws,
                      int accumulate, int rows, hipStream_t st, float* dX, const float* add) {
  using G = WinGeo<T, V>;
  const size_t lds = (size_t)G::ParLds * sizeof(float);
  const int ntiles = ceil_div(rows, 16 * G::ParRT);
  const int grid = ntiles < G::ParGrid ? ntiles : G::ParGrid;
  float* partials = reinterpret_cast<float*>(ws);
  const int vec = aligned16(x) && aligned16(dZ) && aligned16(dX) && aligned16(add);   // (NULL counts as aligned)
  int rc;
  if (dX) {
    if ((rc = set_lds(k_win_params<T, V, true>, lds))) return rc;
    hipLaunchKernelGGL((k_win_params<T, V, true>), dim3(grid), dim3(G::ParBlock), lds, st, x, dZ, Aw, Tw, partials, dX, add, rows, vec);
  } else {
    if ((rc = set_lds(k_win_params<T, V, false>, lds))) return rc;
    hipLaunchKernelGGL((k_win_params<T, V, false>), dim3(grid), dim3(G::ParBlock), lds, st, x, dZ, Aw, Tw, partials, dX, add, rows, vec);
  }
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
                         int accumulate, int rows, int T, int V, hipStream_t st, float* dX, const float* add) {
#define CALL(T_, V_) return launch_win_params<T_, V_>(x, dZ, Aw, Tw, dA, dT, ws, accumulate, rows, st, dX, add)
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
