// Constants, slot layout and block sums shared by the one-class heads (heads.hip: rows over latent_row.h's two maps;
// heads_wide.hip: the MFMA Mahalanobis head above 16 latents) and by the launches the Euclidean head rides in.
#pragma once
#include "latent_row.h"

namespace coskad {

constexpr float kMinNorm = 1e-5f;      // hyper_math.py:101,303
constexpr float kBallEps = 1e-3f;      // hyper_math.py:102
constexpr float kArtanhEps = 1e-5f;    // hyper_math.py:21
constexpr float kMobiusEps = 1e-5f;    // hyper_math.py:179
constexpr float kTanhClamp = 15.f;     // hyper_math.py:13

// Slots of a stats / acc block at latent L, Lp = max(L, 16):  [0] loss term  [1..Lp] vector sum  [Lp+1] scalar A  [Lp+2] scalar B.
__host__ __device__ inline int head_lp(int L) { return L > LMAX ? L : LMAX; }
__host__ __device__ inline int head_slots_for(int L) { return head_lp(L) + 3; }
constexpr int kHeadSlots = LMAX + 3;   // the 19 slots at L <= 16

// ---- launch geometry -----------------------------------------------------------------------------------------------------------
// PerThread: kFlatBlock clips per block.  A one-block launch (B <= kHeadSingleRows clips) writes the finished statistics itself --
// no partial row, no k_head_finalize launch behind it.  Larger batches keep one row per thread: ONE block striding over 4096 rows
// measured 65 us against 12 + 5 us for eight blocks + k_head_finalize (eight dependent load rounds per thread).
constexpr int kHeadSingleRows = kFlatBlock;
__host__ __device__ inline int head_blocks(int B) { return B <= kHeadSingleRows ? 1 : ceil_div(B, kFlatBlock); }
// PerWave: 256 threads, four clips per round; a block per 16 clips (one MFMA row tile of the Mahalanobis head), grid-stride beyond
// 16 K clips (the finalize reads one partial row per block and slot)
constexpr int kWideBlock = 256;
constexpr int kWideWaves = kWideBlock / 64;
constexpr int kWideTileRows = 16;
constexpr int kWideMaxBlocks = 1024;
inline int wide_head_blocks(int B) { const int p = ceil_div(B, kWideTileRows); return p < kWideMaxBlocks ? p : kWideMaxBlocks; }
template <class M> inline constexpr int kHeadBlock = kFlatBlock;   // threads per block of the row kernels
template <> inline constexpr int kHeadBlock<PerWave> = kWideBlock;

// ---- what a thread sums over its clips: the slots' terms, under the thread's map ---------------------------------------------------
template <class M>
struct HeadSums {
  float s0 = 0.f;          // [0]
  float v[M::NE] = {};     // [1 + index(i)]
  float sA = 0.f, sB = 0.f;
};
// where a block's sums go: its partial row, or (PerThread, a one-block launch) the finished stats / acc
struct HeadOut {
  float* partials;
  float scale0;
  float *stats, *acc;
};

// The two block-sum schemes keep their own summation orders (the kernel tests pin both).
// PerThread, block `bid` of `nb` (kFlatBlock threads each): a wave_sum per slot, the waves in order; its partial row of kHeadSlots
// floats, or, when it is the only block, the finished statistics.
__device__ __forceinline__ void flush(const HeadSums<PerThread>& t, const HeadOut& o, int L, int bid, int nb) {
  __shared__ float sh[kFlatBlock / 64][kHeadSlots];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kHeadSlots; ++k) {
    const float s = wave_sum(k == 0 ? t.s0 : k <= LMAX ? t.v[k - 1] : k == LMAX + 1 ? t.sA : t.sB);
    if (lane == 0) sh[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < kHeadSlots) {
    float s = 0.f;
    for (int w = 0; w < kFlatBlock / 64; ++w) s += sh[w][threadIdx.x];
    if (nb == 1) {
      if (o.stats) o.stats[threadIdx.x] = threadIdx.x == 0 ? s * o.scale0 : s;
      if (o.acc) o.acc[threadIdx.x] += s;
    } else {
      o.partials[bid * kHeadSlots + threadIdx.x] = s;
    }
  }
}
// PerWave, block `bid` (kWideBlock threads): the lane slots of every wave, the four waves in order; always a partial row of
// head_slots_for(L) floats (k_wide_finalize sums the rows in fp64)
__device__ __forceinline__ void flush(const HeadSums<PerWave>& t, const HeadOut& o, int L, int bid, int /*nb*/) {
  __shared__ float sh[kWideWaves][kWideLMax + 3];
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < PerWave::NE; ++i)
    if (PerWave::index(i) < L) sh[wave][1 + PerWave::index(i)] = t.v[i];
  if (PerWave::first()) { sh[wave][0] = t.s0; sh[wave][L + 1] = t.sA; sh[wave][L + 2] = t.sB; }
  __syncthreads();
  float* row = o.partials + (size_t)bid * (L + 3);
  for (int k = threadIdx.x; k < L + 3; k += kWideBlock) row[k] = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
}

// One clip of the Euclidean head: latent u against the centre c -> its gradient g and squared distance; the clip's terms are
// added to the thread's sums ([0] sum (z-c)^2, [1..L] sum z, [Lp+1] #clips, [Lp+2] sum |z|)
template <class M>
__device__ __forceinline__ float mse_head_row(const Row<M>& u, const Row<M>& c, float gscale, HeadSums<M>& t, Row<M>& g) {
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < M::NE; ++i) {
    const float d = u.v[i] - c.v[i];  // 0 beyond L (both rows hold 0)
    sq = fmaf(d, d, sq);
    g.v[i] = 2.f * d * gscale;        // d mean((z-c)^2)/dz, gscale = upstream / (B*L)
    t.v[i] += u.v[i];
  }
  sq = M::reduce(sq);
  t.s0 += sq;
  t.sA += 1.f;
  t.sB += sqrtf(dot(u, u));
  return sq;
}

// stats[k] = sum_p partials[p][k] (slot 0 additionally * scale0);  acc[k] += raw sums: thread k of one block (L <= 16)
__device__ __forceinline__ void head_finalize_slot(const float* __restrict__ partials, int P, float scale0,
                                                   float* __restrict__ stats, float* __restrict__ acc, int k) {
  if (k >= kHeadSlots) return;
  double s = 0.0;
  for (int p = 0; p < P; ++p) s += (double)partials[p * kHeadSlots + k];
  if (stats) stats[k] = (float)(k == 0 ? s * (double)scale0 : s);
  if (acc) acc[k] += (float)s;
}

// heads_wide.hip (16 < L <= kWideLMax): the partial rows' fp64 sum (a no-op when stats and acc are NULL), and the MFMA
// Mahalanobis head with its Gram launch; ws: wide_head_blocks(B) * head_slots_for(L) floats
void wide_head_finalize(const float* ws, int P, int L, float scale0, float* stats, float* acc, hipStream_t stream);
int wide_mahalanobis_head(const float* z, const float* c, const float* VI, float* dz, float* score, float* stats, float* acc,
                          float* gram, int gram_accumulate, float upstream, float* ws, int B, int L, hipStream_t stream);

}  // namespace coskad
