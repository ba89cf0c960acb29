// What the kernels of the window lengths 8, 16 and 24 share (gcn_window.hip: the mixing and its parameter gradients;
// train_window_moments.hip: the statistics pass of a training layer): the geometry of a 16-row tile image in LDS, the two mixes on
// v_mfma_f32_16x16x4_f32 with their B operands in registers, and the float4 staging of row tiles.  Everything here has internal
// linkage: a file that includes it gets its own copy.
#pragma once
#include "common.h"
#include "mfma_ops.h"

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
// (T*V is a multiple of 4, so the tensor's base decides) -> float4 loads, UB in flight per thread.  ACT: the rows are
// pre-activations, PReLU(slope) is applied on the way in (float4 form only).
template <int TV, int LD, int NR, int BLOCK, int UB, bool ACT = false>
__device__ __forceinline__ void win_load(float* img, const float* __restrict__ g, size_t r0, int nv, bool vec, float slope = 0.f) {
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
          if constexpr (ACT) {
            d[0] = prelu_f(v[u].x, slope); d[1] = prelu_f(v[u].y, slope); d[2] = prelu_f(v[u].z, slope); d[3] = prelu_f(v[u].w, slope);
          } else {
            d[0] = v[u].x; d[1] = v[u].y; d[2] = v[u].z; d[3] = v[u].w;
          }
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

// win_store (float4 form) through the PReLU in front of the layer: the image holds dX w.r.t. the ACTIVATED input, `pre` the
// pre-activation rows it was formed from (re-read: one L2 round trip, the tile was loaded by this workgroup a pass ago).
// g = (dX + add) . PReLU'(pre);  returns this thread's share of  sum (dX + add) . pre  over pre < 0  (the slope gradient).
template <int TV, int LD, int NR, int BLOCK>
__device__ __forceinline__ float win_store_act(const float* img, float* __restrict__ g, const float* __restrict__ add,
                                               const float* __restrict__ pre, size_t r0, int nv, float slope) {
  float4* o4 = reinterpret_cast<float4*>(g + r0 * TV);
  const float4* a4 = add ? reinterpret_cast<const float4*>(add + r0 * TV) : nullptr;
  const float4* u4 = reinterpret_cast<const float4*>(pre + r0 * TV);
  const int n4 = nv * (TV / 4);
  float da = 0.f;
  for (int i = threadIdx.x; i < n4; i += BLOCK) {
    const int e = 4 * i, r = e / TV, p = e - r * TV;
    const float* s = img + r * LD + p;
    float4 o = float4{s[0], s[1], s[2], s[3]};
    const float4 u = u4[i];
    if (a4) { const float4 q = a4[i]; o.x += q.x; o.y += q.y; o.z += q.z; o.w += q.w; }
    if (u.x < 0.f) da = fmaf(o.x, u.x, da);
    if (u.y < 0.f) da = fmaf(o.y, u.y, da);
    if (u.z < 0.f) da = fmaf(o.z, u.z, da);
    if (u.w < 0.f) da = fmaf(o.w, u.w, da);
    o.x = u.x > 0.f ? o.x : slope * o.x;
    o.y = u.y > 0.f ? o.y : slope * o.y;
    o.z = u.z > 0.f ? o.z : slope * o.z;
    o.w = u.w > 0.f ? o.w : slope * o.w;
    o4[i] = o;
  }
  return da;
}

__host__ inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

}  // namespace
}  // namespace coskad
