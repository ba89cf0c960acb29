// A clip's latent row in registers, over two element-to-thread maps.  The latent heads (heads.hip, vae_head.hip) write each
// formula once as `template <class M>` over a map; narrow and wide latents are its two instantiations.
//
//   PerThread (L <= LMAX)            one thread per clip: 16 elements, element i is latent index i, sums need no reduction
//   PerWave   (LMAX < L <= kWideLMax) one wave per clip: 8 elements per lane, element i is latent index lane + 64 i, a sum is the
//                                    lane's fmaf chain followed by wave_sum (a fixed butterfly: every lane receives the same bits)
//
// Pad elements (index >= L) hold exact zeros in every row and store nothing.  Per-clip scalars are uniform over the clip's
// threads; M::first() picks the one that stores them.  The names follow vae_head_normal.hip's maps (reduce, first), which stay
// apart: segmented waves and 16-byte accesses are another layout family.
#pragma once
#include "common.h"

namespace coskad {

constexpr int LMAX = 16;          // widest latent of the one-thread-per-clip map
constexpr int kWideLMax = 512;    // widest latent of the one-wave-per-clip map: 8 values per lane

struct PerThread {
  static constexpr int NE = LMAX;
  static __device__ __forceinline__ int index(int i) { return i; }
  static __device__ __forceinline__ float reduce(float v) { return v; }
  static __device__ __forceinline__ bool first() { return true; }
  // a block of `threads` threads: clips per round, and this thread's clip in the block's first round
  static __host__ __device__ constexpr int clips(int threads) { return threads; }
  static __device__ __forceinline__ int clip(int threads) { return blockIdx.x * threads + threadIdx.x; }
};

struct PerWave {
  static constexpr int NE = kWideLMax / 64;
  static __device__ __forceinline__ int index(int i) { return (threadIdx.x & 63) + 64 * i; }
  static __device__ __forceinline__ float reduce(float v) { return wave_sum(v); }
  static __device__ __forceinline__ bool first() { return (threadIdx.x & 63) == 0; }
  static __host__ __device__ constexpr int clips(int threads) { return threads / 64; }
  static __device__ __forceinline__ int clip(int threads) { return blockIdx.x * (threads / 64) + (threadIdx.x >> 6); }
};

// f(PerWave{}) for a wide latent, f(PerThread{}) otherwise: the entry points pick a kernel's instantiation by L
template <class F>
inline void by_width(int L, F f) {
  if (L > LMAX) f(PerWave{});
  else f(PerThread{});
}

template <class M>
struct Row {
  float v[M::NE];
};

template <class M>
__device__ __forceinline__ Row<M> load(const float* p, int L) {
  Row<M> r;
#pragma unroll
  for (int i = 0; i < M::NE; ++i) r.v[i] = M::index(i) < L ? p[M::index(i)] : 0.f;
  return r;
}
// row[j] = eps[j - 1] for 1 <= j < L (eps: a clip's L - 1 draws), 0 elsewhere
template <class M>
__device__ __forceinline__ Row<M> load_eps(const float* eps, int L) {
  Row<M> r;
#pragma unroll
  for (int i = 0; i < M::NE; ++i) r.v[i] = (M::index(i) >= 1 && M::index(i) < L) ? eps[M::index(i) - 1] : 0.f;
  return r;
}
template <class M>
__device__ __forceinline__ void store(float* p, const Row<M>& a, int L) {
#pragma unroll
  for (int i = 0; i < M::NE; ++i)
    if (M::index(i) < L) p[M::index(i)] = a.v[i];
}
// one fmaf chain over the thread's elements in index order, then the map's reduction
template <class M>
__device__ __forceinline__ float dot(const Row<M>& a, const Row<M>& b) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < M::NE; ++i) s = fmaf(a.v[i], b.v[i], s);
  return M::reduce(s);
}

}  // namespace coskad
