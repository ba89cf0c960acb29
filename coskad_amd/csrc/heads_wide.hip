// The one-class heads' MFMA half, at 16 < latent <= 512 (the row heads of those latents are heads.hip's PerWave instantiations):
//
//   Mahalanobis : per block a 16-clip tile, Y = (Z - c) VI^T and Y' = (Z - c) VI on v_mfma_f32_16x16x4_f32 (exact fp32 FMA
//                 chains), the tile's columns split over the four waves; the row epilogue forms the distance, the score and
//                 dz = (Y + Y') / (2 dist) from the accumulators in registers.
//   gram        : sum_n z_n z_n^T on the same MFMA, one wave per 16 x 16 tile of the [L, L] result.
//   finalize    : every block of a wide head writes one partial row of head_slots_for(L) floats; k_wide_finalize sums the rows
//                 per slot in fp64 in block order.
// No float atomics: two identical calls give bitwise-identical results.
#include "heads_common.h"

namespace coskad {
namespace hw {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kBlock = kWideBlock;
constexpr int kWaves = kWideWaves;
constexpr int kTileRows = kWideTileRows;    // clips per block and pass (4 per wave; one MFMA row tile)
constexpr int kMahaTiles = kWideLMax / 16 / kWaves;   // 16-column tiles per wave

// Mahalanobis head.  slots: [0] sum dist, [1..L] sum z, [L+1] #clips, [L+2] sum |z|.
// dist = sqrt(d^T VI d), d = z - c;  d dist / dz = (VI + VI^T) d / (2 dist)  (k_mahalanobis_head: VI is not assumed symmetric)
__global__ __launch_bounds__(kBlock) void k_mahalanobis_wide(const float* __restrict__ z, const float* __restrict__ cvec,
                                                            const float* __restrict__ VI, float* __restrict__ dz,
                                                            float* __restrict__ score, float* __restrict__ partials, int B,
                                                            int L, float gscale) {
  __shared__ float ddp[kWaves][kTileRows];
  __shared__ float dist_s[kTileRows];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kk = lane >> 4;
  const int NT = ceil_div(L, 16);
  float s0 = 0.f, sA = 0.f, sB = 0.f;       // s0, sA: thread 0;  sB: lane 0 of each wave
  float vs0 = 0.f, vs1 = 0.f;               // column sums of columns threadIdx.x and threadIdx.x + 256
  const int ntiles = ceil_div(B, kTileRows);
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int n0 = tile * kTileRows;
    const int na = n0 + i;
    const bool rowa = na < B;
    f32x4 aw[kMahaTiles], at[kMahaTiles];
#pragma unroll
    for (int t = 0; t < kMahaTiles; ++t) { aw[t] = f32x4{0.f, 0.f, 0.f, 0.f}; at[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    // Y[row][col] = sum_k d[row][k] VI[col][k],  Y'[row][col] = sum_k d[row][k] VI[k][col]
    for (int k0 = 0; k0 < L; k0 += 4) {
      const int k = k0 + kk;
      const bool kok = k < L;
      const float a = (rowa && kok) ? z[(size_t)na * L + k] - cvec[k] : 0.f;
#pragma unroll
      for (int t = 0; t < kMahaTiles; ++t) {
        const int jt = wave + kWaves * t;
        if (jt < NT) {                               // wave-uniform
          const int col = jt * 16 + i;
          const bool ok = kok && col < L;
          const float bw = ok ? VI[(size_t)col * L + k] : 0.f;
          const float bt = ok ? VI[(size_t)k * L + col] : 0.f;
          aw[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bw, aw[t], 0, 0, 0);
          at[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bt, at[t], 0, 0, 0);
        }
      }
    }
    // d^T Y per row: lane (i, kk) reg r <-> row 4 kk + r, column jt * 16 + i
    float dd[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < kMahaTiles; ++t) {
      const int jt = wave + kWaves * t;
      if (jt < NT) {
        const int col = jt * 16 + i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = n0 + 4 * kk + r;
          const float d = (n < B && col < L) ? z[(size_t)n * L + col] - cvec[col] : 0.f;
          dd[r] = fmaf(d, aw[t][r], dd[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int off = 8; off > 0; off >>= 1) dd[r] += __shfl_xor(dd[r], off, 64);   // the 16 lanes of one row group
      if (i == 0) ddp[wave][4 * kk + r] = dd[r];
    }
    __syncthreads();
    if (threadIdx.x < kTileRows) {
      const int n = n0 + threadIdx.x;
      const float dist = sqrtf(((ddp[0][threadIdx.x] + ddp[1][threadIdx.x]) + ddp[2][threadIdx.x]) + ddp[3][threadIdx.x]);
      dist_s[threadIdx.x] = dist;
      if (n < B && score) score[n] = dist;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int r = 0; r < kTileRows && n0 + r < B; ++r) { s0 += dist_s[r]; sA += 1.f; }
    }
    if (dz) {
#pragma unroll
      for (int t = 0; t < kMahaTiles; ++t) {
        const int jt = wave + kWaves * t;
        if (jt < NT) {
          const int col = jt * 16 + i;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int n = n0 + 4 * kk + r;
            const float inv = gscale / (2.f * dist_s[4 * kk + r]);   // dist == 0: inf * 0 = NaN, as torch.sqrt's backward gives
            if (n < B && col < L) dz[(size_t)n * L + col] = (aw[t][r] + at[t][r]) * inv;
          }
        }
      }
    }
    // centre sums: column sums in clip order, row norms (wave w: rows 4w .. 4w+3)
    for (int r = 0; r < kTileRows && n0 + r < B; ++r) {
      const float* zr = z + (size_t)(n0 + r) * L;
      if ((int)threadIdx.x < L) vs0 += zr[threadIdx.x];
      if ((int)threadIdx.x + kBlock < L) vs1 += zr[threadIdx.x + kBlock];
    }
#pragma unroll
    for (int r = 0; r < kTileRows / kWaves; ++r) {
      const int n = n0 + kWaves * wave + r;
      if (n < B) {
        const Row<PerWave> u = load<PerWave>(z + (size_t)n * L, L);
        sB += sqrtf(dot(u, u));
      }
    }
    __syncthreads();   // ddp / dist_s are rewritten by the next tile
  }
  __shared__ float sbw[kWaves];
  if (lane == 0) sbw[wave] = sB;
  __syncthreads();
  float* row = partials + (size_t)blockIdx.x * (L + 3);
  if ((int)threadIdx.x < L) row[1 + threadIdx.x] = vs0;
  if ((int)threadIdx.x + kBlock < L) row[1 + threadIdx.x + kBlock] = vs1;
  if (threadIdx.x == 0) {
    row[0] = s0;
    row[L + 1] = sA;
    row[L + 2] = ((sbw[0] + sbw[1]) + sbw[2]) + sbw[3];
  }
}

// gram (+)= sum_n z_n z_n^T [L x L]: one wave per 16 x 16 tile, the clips in order (4 per MFMA)
__global__ __launch_bounds__(kBlock) void k_gram_wide(const float* __restrict__ z, float* __restrict__ gram, int B, int L,
                                                     int accumulate) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 15, kk = lane >> 4;
  const int NT = ceil_div(L, 16);
  const int t = blockIdx.x * kWaves + wave;
  if (t >= NT * NT) return;
  const int it = t / NT, jt = t - it * NT;
  const int ci = it * 16 + i, cj = jt * 16 + i;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int n0 = 0; n0 < B; n0 += 4) {
    const int n = n0 + kk;
    const float a = (n < B && ci < L) ? z[(size_t)n * L + ci] : 0.f;
    const float b = (n < B && cj < L) ? z[(size_t)n * L + cj] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = it * 16 + 4 * kk + r, col = jt * 16 + i;
    if (row < L && col < L) {
      float* g = gram + (size_t)row * L + col;
      *g = accumulate ? *g + acc[r] : acc[r];
    }
  }
}

// stats[k] = sum_p partials[p][k] (slot 0 additionally * scale0);  acc[k] += raw sums.  64 slots per block, fp64, rows in order.
__global__ __launch_bounds__(1024) void k_wide_finalize(const float* __restrict__ partials, int P, int S, float scale0,
                                                        float* __restrict__ stats, float* __restrict__ acc) {
  __shared__ double sh[1024];
  const int k = blockIdx.x * 64 + (threadIdx.x & 63);
  const double s = column_sum_f64<64>(partials, P, (size_t)S, k, k < S, sh);
  if (threadIdx.x < 64 && k < S) {
    if (stats) stats[k] = (float)(k == 0 ? s * (double)scale0 : s);
    if (acc) acc[k] += (float)s;
  }
}

}  // namespace hw

void wide_head_finalize(const float* ws, int P, int L, float scale0, float* stats, float* acc, hipStream_t stream) {
  const int S = head_slots_for(L);
  if (stats || acc) hipLaunchKernelGGL(hw::k_wide_finalize, dim3(ceil_div(S, 64)), dim3(1024), 0, stream, ws, P, S, scale0, stats, acc);
}

int wide_mahalanobis_head(const float* z, const float* c, const float* VI, float* dz, float* score, float* stats, float* acc,
                          float* gram, int gram_accumulate, float upstream, float* ws, int B, int L, hipStream_t stream) {
  const int P = wide_head_blocks(B);
  hipLaunchKernelGGL(hw::k_mahalanobis_wide, dim3(P), dim3(hw::kBlock), 0, stream, z, c, VI, dz, score, ws, B, L,
                     upstream / (float)B);
  wide_head_finalize(ws, P, L, 1.f / (float)B, stats, acc, stream);
  if (gram) {
    const int NT = ceil_div(L, 16);
    hipLaunchKernelGGL(hw::k_gram_wide, dim3(ceil_div(NT * NT, hw::kWaves)), dim3(hw::kBlock), 0, stream, z, gram, B, L,
                       gram_accumulate);
  }
  return check_launch("mahalanobis_head (wide)");
}

}  // namespace coskad
