// Constants and slot layout shared by the one-class heads: heads.hip (latent <= 16, one thread per clip) and heads_wide.hip
// (16 < latent <= 512, one wave per clip).
#pragma once
#include "common.h"

namespace coskad {

constexpr int LMAX = 16;               // latent width of the one-thread-per-clip heads (heads.hip)
constexpr int kWideLMax = 512;         // latent width of the one-wave-per-clip heads (heads_wide.hip): 8 values per lane
constexpr float kMinNorm = 1e-5f;      // hyper_math.py:101,303
constexpr float kBallEps = 1e-3f;      // hyper_math.py:102
constexpr float kArtanhEps = 1e-5f;    // hyper_math.py:21
constexpr float kMobiusEps = 1e-5f;    // hyper_math.py:179
constexpr float kTanhClamp = 15.f;     // hyper_math.py:13

// Slots of a stats / acc block at latent L, Lp = max(L, 16):  [0] loss term  [1..Lp] vector sum  [Lp+1] scalar A  [Lp+2] scalar B.
// At L <= 16 this is the 19-slot layout of heads.hip.
__host__ __device__ inline int head_lp(int L) { return L > LMAX ? L : LMAX; }
__host__ __device__ inline int head_slots_for(int L) { return head_lp(L) + 3; }

// heads_wide.hip (16 < L <= kWideLMax); ws: wide_head_ws_floats(B, L) floats
size_t wide_head_ws_floats(int B, int L);
int wide_mse_head(const float* z, const float* c, float* dz, float* score, float* stats, float* acc, float upstream, float* ws,
                  int B, int L, hipStream_t stream);
int wide_mahalanobis_head(const float* z, const float* c, const float* VI, float* dz, float* score, float* stats, float* acc,
                          float* gram, int gram_accumulate, float upstream, float* ws, int B, int L, hipStream_t stream);
int wide_poincare_head(const float* z, const float* c, float* dz, float* zh, float* score, float* stats, float* acc,
                       float upstream, float* ws, int B, int L, hipStream_t stream);
int wide_poincare_dist(const float* zh, const float* c, float* score, int B, int L, hipStream_t stream);
int wide_poincare_logmap0(const float* y, float* out, int B, int L, hipStream_t stream);
int wide_center_finalize(const float* acc, float* c, float eps, int L, hipStream_t stream);
int wide_midpoint_finalize(const float* acc, float* c, int L, hipStream_t stream);

}  // namespace coskad
