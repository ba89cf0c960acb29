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

// ---- the one-thread-per-clip heads (heads.hip; the Euclidean head's rows also ride in btlnk_chain.hip's launch) ----------------
struct Vec {
  float v[LMAX];
};

__device__ __forceinline__ Vec load_vec(const float* p, int L) {
  Vec r;
#pragma unroll
  for (int j = 0; j < LMAX; ++j) r.v[j] = j < L ? p[j] : 0.f;
  return r;
}
__device__ __forceinline__ void store_vec(float* p, const Vec& a, int L) {
#pragma unroll
  for (int j = 0; j < LMAX; ++j)
    if (j < L) p[j] = a.v[j];
}
__device__ __forceinline__ float dot(const Vec& a, const Vec& b) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < LMAX; ++j) s = fmaf(a.v[j], b.v[j], s);
  return s;
}

// Per-block partial row of kHeadSlots floats (fixed slots, summed in block order later):
//   [0] loss term   [1..16] vector sum   [17] scalar A   [18] scalar B
constexpr int kHeadSlots = LMAX + 3;

// A one-block launch (B <= kHeadSingleRows clips) writes the finished statistics itself -- no partial row, no k_head_finalize
// launch behind it.  Larger batches keep one row per thread: ONE block striding over 4096 rows measured 65 us against 12 + 5 us
// for eight blocks + k_head_finalize (eight dependent load rounds per thread).
constexpr int kHeadSingleRows = kFlatBlock;
__host__ __device__ inline int head_blocks(int B) { return B <= kHeadSingleRows ? 1 : ceil_div(B, kFlatBlock); }

// block `bid` of `nb` head blocks (kFlatBlock threads each): its partial row, or, when it is the only one, the finished statistics
__device__ __forceinline__ void block_partials(const float (&vals)[kHeadSlots], float* partials, float scale0, float* stats,
                                               float* acc, int bid, int nb) {
  __shared__ float sh[kFlatBlock / 64][kHeadSlots];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kHeadSlots; ++k) {
    const float s = wave_sum(vals[k]);
    if (lane == 0) sh[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < kHeadSlots) {
    float s = 0.f;
    for (int w = 0; w < kFlatBlock / 64; ++w) s += sh[w][threadIdx.x];
    if (nb == 1) {
      if (stats) stats[threadIdx.x] = threadIdx.x == 0 ? s * scale0 : s;
      if (acc) acc[threadIdx.x] += s;
    } else {
      partials[bid * kHeadSlots + threadIdx.x] = s;
    }
  }
}

// One clip of the Euclidean head: latent u against the centre c -> its gradient g and squared distance; the clip's terms are
// added to the thread's slots ([0] sum (z-c)^2, [1..L] sum z, [17] #clips, [18] sum |z|)
__device__ __forceinline__ float mse_head_row(const Vec& u, const Vec& c, int L, float gscale, float (&vals)[kHeadSlots], Vec& g) {
  float sq = 0.f;
#pragma unroll
  for (int j = 0; j < LMAX; ++j) {
    const float d = j < L ? u.v[j] - c.v[j] : 0.f;
    sq = fmaf(d, d, sq);
    g.v[j] = 2.f * d * gscale;  // d mean((z-c)^2)/dz, gscale = upstream / (B*L)
    vals[1 + j] += u.v[j];
  }
  vals[0] += sq;
  vals[LMAX + 1] += 1.f;
  vals[LMAX + 2] += sqrtf(dot(u, u));
  return sq;
}

// stats[k] = sum_p partials[p][k] (slot 0 additionally * scale0);  acc[k] += raw sums: thread k of one block
__device__ __forceinline__ void head_finalize_slot(const float* __restrict__ partials, int P, float scale0,
                                                   float* __restrict__ stats, float* __restrict__ acc, int k) {
  if (k >= kHeadSlots) return;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += (double)partials[p * kHeadSlots + k];
  if (stats) stats[k] = (float)(k == 0 ? s * (double)scale0 : s);
  if (acc) acc[k] += (float)s;
}

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
