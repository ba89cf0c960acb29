// One-class heads at 16 < latent <= 512: the formulas, epsilons and clamps of heads.hip (heads_common.h), one WAVE per clip.
//
//   Euclidean / Poincare : lane l holds latent values j = l + 64 v (v < 8); norms and dots are cross-lane sums (wave_sum).
//   Mahalanobis          : per block a 16-clip tile, Y = (Z - c) VI^T and Y' = (Z - c) VI on v_mfma_f32_16x16x4_f32 (exact fp32
//                          FMA chains), the tile's columns split over the four waves; the row epilogue forms the distance, the
//                          score and dz = (Y + Y') / (2 dist) from the accumulators in registers.
//   gram                 : sum_n z_n z_n^T on the same MFMA, one wave per 16 x 16 tile of the [L, L] result.
//
// Every block writes one partial row of head_slots_for(L) floats; k_wide_finalize sums the rows per slot in fp64 in block order.
// No float atomics: two identical calls give bitwise-identical results.
#include "heads_common.h"

namespace coskad {
namespace hw {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int NV = kWideLMax / 64;          // latent values per lane
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTileRows = 16;               // clips per block and pass (4 per wave; one MFMA row tile for Mahalanobis)
constexpr int kMaxBlocks = 1024;            // partial rows: grid-stride beyond 16 K clips (the finalize reads P rows per slot)
constexpr int kMahaTiles = kWideLMax / 16 / kWaves;   // 16-column tiles per wave (Mahalanobis)

inline int blocks(int B) { const int p = ceil_div(B, kTileRows); return p < kMaxBlocks ? p : kMaxBlocks; }

struct WVec {
  float v[NV];
};

__device__ __forceinline__ WVec wload(const float* p, int L) {
  const int lane = threadIdx.x & 63;
  WVec r;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int j = lane + 64 * v;
    r.v[v] = j < L ? p[j] : 0.f;
  }
  return r;
}
__device__ __forceinline__ void wstore(float* p, const WVec& a, int L) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int j = lane + 64 * v;
    if (j < L) p[j] = a.v[v];
  }
}
// every lane receives the same sum (an xor butterfly adds the same pair on both partners)
__device__ __forceinline__ float wdot(const WVec& a, const WVec& b) {
  float s = 0.f;
#pragma unroll
  for (int v = 0; v < NV; ++v) s = fmaf(a.v[v], b.v[v], s);
  return wave_sum(s);
}

struct Embed {
  WVec p;
  float un_raw, un, tn, en_raw;
  bool clamped;
};
// e = expmap0(u), p = project(e) (heads.hip hyp_embed)
__device__ __forceinline__ Embed hyp_embed(const WVec& u) {
  Embed r;
  r.un_raw = sqrtf(wdot(u, u));
  r.un = fmaxf(r.un_raw, kMinNorm);
  r.tn = tanhf(fminf(fmaxf(r.un, -kTanhClamp), kTanhClamp));
  const float f = r.tn / r.un;
  WVec e;
#pragma unroll
  for (int v = 0; v < NV; ++v) e.v[v] = f * u.v[v];
  r.en_raw = sqrtf(wdot(e, e));
  const float en = fmaxf(r.en_raw, kMinNorm);
  const float maxnorm = 1.f - kBallEps;
  r.clamped = en > maxnorm;
#pragma unroll
  for (int v = 0; v < NV; ++v) r.p.v[v] = r.clamped ? e.v[v] / en * maxnorm : e.v[v];
  return r;
}

// d = dist(c, p) = 2 artanh(|(-c) (+) p|), and dd/dp (heads.hip poincare_dist)
__device__ __forceinline__ float poincare_dist(const WVec& c, const WVec& p, WVec* gp) {
  const float x2 = wdot(c, c), y2 = wdot(p, p), xy = -wdot(c, p);
  const float alpha = 1.f + 2.f * xy + y2, beta = 1.f - x2;
  const float den = 1.f + 2.f * xy + x2 * y2;
  const float D = den + kMobiusEps;
  WVec m;
#pragma unroll
  for (int v = 0; v < NV; ++v) m.v[v] = (alpha * (-c.v[v]) + beta * p.v[v]) / D;
  const float mn = sqrtf(wdot(m, m));
  const float mc = fminf(fmaxf(mn, -1.f + kArtanhEps), 1.f - kArtanhEps);
  const float d = (log1pf(mc) - log1pf(-mc));
  if (gp) {
    const float gmn = 2.f / (1.f - mc * mc);
    const float inv = mn > 0.f ? gmn / mn : 0.f;
    WVec gm;
#pragma unroll
    for (int v = 0; v < NV; ++v) gm.v[v] = inv * m.v[v];
    const float gD = -wdot(gm, m) / D;
    float ga = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) ga = fmaf(gm.v[v] / D, -c.v[v], ga);
    const float galpha = wave_sum(ga);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float x = -c.v[v], y = p.v[v];
      gp->v[v] = beta * gm.v[v] / D + galpha * (2.f * x + 2.f * y) + gD * (2.f * x + 2.f * x2 * y);
    }
  }
  return d;
}

// dL/dp back through project and expmap0 (heads.hip hyp_embed_bwd)
__device__ __forceinline__ WVec hyp_embed_bwd(const WVec& u, const Embed& em, const WVec& gp) {
  const float f = em.tn / em.un;
  WVec ge;
  if (em.clamped) {
    const float maxnorm = 1.f - kBallEps;
    const float en = em.en_raw;
    float e = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) e = fmaf(f * u.v[v], gp.v[v], e);
    const float egp = wave_sum(e);
#pragma unroll
    for (int v = 0; v < NV; ++v) ge.v[v] = maxnorm * (gp.v[v] / en - f * u.v[v] * egp / (en * en * en));
  } else {
    ge = gp;
  }
  WVec gu;
  const float gf = wdot(ge, u);
  float coef = 0.f;
  if (em.un_raw > kMinNorm) {
    const float sech2 = em.un < kTanhClamp ? 1.f - em.tn * em.tn : 0.f;
    const float df = (sech2 * em.un - em.tn) / (em.un * em.un);
    coef = gf * df / em.un_raw;
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) gu.v[v] = f * ge.v[v] + coef * u.v[v];
  return gu;
}

// The block's partial row: [0] s0, [1..L] vector sums (lane slots of every wave), [L+1] sA, [L+2] sB; the four waves in order.
__device__ __forceinline__ void block_partials(const float (&vs)[NV], float s0, float sA, float sB, float* __restrict__ partials, int L) {
  __shared__ float sh[kWaves][kWideLMax + 3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int j = lane + 64 * v;
    if (j < L) sh[wave][1 + j] = vs[v];
  }
  if (lane == 0) { sh[wave][0] = s0; sh[wave][L + 1] = sA; sh[wave][L + 2] = sB; }
  __syncthreads();
  float* row = partials + (size_t)blockIdx.x * (L + 3);
  for (int k = threadIdx.x; k < L + 3; k += kBlock) row[k] = ((sh[0][k] + sh[1][k]) + sh[2][k]) + sh[3][k];
}

// Euclidean head.  slots: [0] sum (z-c)^2, [1..L] sum z, [L+1] #clips, [L+2] sum |z|
__global__ __launch_bounds__(kBlock) void k_mse_wide(const float* __restrict__ z, const float* __restrict__ cvec,
                                                    float* __restrict__ dz, float* __restrict__ score,
                                                    float* __restrict__ partials, int B, int L, float gscale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float vs[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) vs[v] = 0.f;
  float s0 = 0.f, sA = 0.f, sB = 0.f;
  const WVec c = wload(cvec, L);
  for (int n = blockIdx.x * kWaves + wave; n < B; n += gridDim.x * kWaves) {
    const WVec u = wload(z + (size_t)n * L, L);
    WVec g;
    float sq = 0.f;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const float d = u.v[v] - c.v[v];             // 0 beyond L (both loads read 0)
      sq = fmaf(d, d, sq);
      g.v[v] = 2.f * d * gscale;                   // d mean((z-c)^2)/dz, gscale = upstream / (B*L)
      vs[v] += u.v[v];
    }
    sq = wave_sum(sq);
    s0 += sq;
    sA += 1.f;
    sB += sqrtf(wdot(u, u));
    if (dz) wstore(dz + (size_t)n * L, g, L);
    if (score && lane == 0) score[n] = sq / (float)L;
  }
  block_partials(vs, s0, sA, sB, partials, L);
}

// Poincare head.  slots: [0] sum dist, [1..L] sum gamma*zh, [L+1] sum (gamma-1), [L+2] sum |zh|
__global__ __launch_bounds__(kBlock) void k_poincare_wide(const float* __restrict__ z, const float* __restrict__ cvec,
                                                         float* __restrict__ dz, float* __restrict__ zh,
                                                         float* __restrict__ score, float* __restrict__ partials, int B, int L,
                                                         float gscale) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float vs[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) vs[v] = 0.f;
  float s0 = 0.f, sA = 0.f, sB = 0.f;
  for (int n = blockIdx.x * kWaves + wave; n < B; n += gridDim.x * kWaves) {
    const WVec u = wload(z + (size_t)n * L, L);
    const Embed em = hyp_embed(u);
    if (zh) wstore(zh + (size_t)n * L, em.p, L);
    const float y2 = wdot(em.p, em.p);
    const float gamma = 2.f / (1.f - y2);
#pragma unroll
    for (int v = 0; v < NV; ++v) vs[v] += gamma * em.p.v[v];
    sA += gamma - 1.f;
    sB += sqrtf(y2);
    if (cvec) {
      const WVec c = wload(cvec, L);
      WVec gp;
      const float d = poincare_dist(c, em.p, dz ? &gp : nullptr);
      s0 += d;
      if (score && lane == 0) score[n] = d;
      if (dz) {
#pragma unroll
        for (int v = 0; v < NV; ++v) gp.v[v] *= gscale;   // gscale = upstream / B
        wstore(dz + (size_t)n * L, hyp_embed_bwd(u, em, gp), L);
      }
    }
  }
  block_partials(vs, s0, sA, sB, partials, L);
}

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
        const WVec u = wload(z + (size_t)n * L, L);
        sB += sqrtf(wdot(u, u));
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

__global__ __launch_bounds__(kBlock) void k_poincare_dist_wide(const float* __restrict__ zh, const float* __restrict__ cvec,
                                                              float* __restrict__ score, int B, int L) {
  const int wave = threadIdx.x >> 6;
  const WVec c = wload(cvec, L);
  for (int n = blockIdx.x * kWaves + wave; n < B; n += gridDim.x * kWaves) {
    const WVec p = wload(zh + (size_t)n * L, L);
    const float d = poincare_dist(c, p, nullptr);
    if ((threadIdx.x & 63) == 0) score[n] = d;
  }
}

__global__ __launch_bounds__(kBlock) void k_poincare_logmap0_wide(const float* __restrict__ y, float* __restrict__ out, int B, int L) {
  const int wave = threadIdx.x >> 6;
  for (int n = blockIdx.x * kWaves + wave; n < B; n += gridDim.x * kWaves) {
    const WVec p = wload(y + (size_t)n * L, L);
    const float yn = fmaxf(sqrtf(wdot(p, p)), kMinNorm);
    const float yc = fminf(fmaxf(yn, -1.f + kArtanhEps), 1.f - kArtanhEps);
    const float at = 0.5f * (log1pf(yc) - log1pf(-yc));
    WVec o;
#pragma unroll
    for (int v = 0; v < NV; ++v) o.v[v] = p.v[v] / yn * at;
    wstore(out + (size_t)n * L, o, L);
  }
}

// Euclidean centre: c = S / n (n = acc[L+1]), then |c| < eps -> +-eps  (heads.hip k_center_finalize)
__global__ __launch_bounds__(kBlock) void k_center_finalize_wide(const float* __restrict__ acc, float eps, float* __restrict__ cvec,
                                                                int L) {
  const int j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= L) return;
  float c = acc[1 + j] / acc[L + 1];
  if (fabsf(c) < eps && c < 0.f) c = -eps;
  if (fabsf(c) < eps && c > 0.f) c = eps;
  cvec[j] = c;
}

// Gyromidpoint from the running sums (heads.hip k_midpoint_finalize): m = S / s, centre = (1/2) (x) m
__global__ void k_midpoint_finalize_wide(const float* __restrict__ acc, float* __restrict__ cvec, int L) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double s = fmax((double)acc[L + 1], 1e-10);
  double mn2 = 0.0;
  for (int j = 0; j < L; ++j) {
    const double m = (double)acc[1 + j] / s;
    mn2 += m * m;
  }
  const double mn = fmax(sqrt(mn2), 1e-15);
  const double mc = fmin(mn, 1.0 - 1e-7);
  const double at = 0.5 * log((1.0 + mc) / (1.0 - mc));
  const double sc = tanh(0.5 * at) / mn;
  for (int j = 0; j < L; ++j) cvec[j] = (float)(sc * ((double)acc[1 + j] / s));
}

static void finalize(const float* ws, int P, int L, float scale0, float* stats, float* acc, hipStream_t stream) {
  const int S = head_slots_for(L);
  if (stats || acc) hipLaunchKernelGGL(k_wide_finalize, dim3(ceil_div(S, 64)), dim3(1024), 0, stream, ws, P, S, scale0, stats, acc);
}

}  // namespace hw

size_t wide_head_ws_floats(int B, int L) { return (size_t)hw::blocks(B > 0 ? B : 1) * (size_t)head_slots_for(L); }

int wide_mse_head(const float* z, const float* c, float* dz, float* score, float* stats, float* acc, float upstream, float* ws,
                  int B, int L, hipStream_t stream) {
  const int P = hw::blocks(B);
  hipLaunchKernelGGL(hw::k_mse_wide, dim3(P), dim3(hw::kBlock), 0, stream, z, c, dz, score, ws, B, L,
                     upstream / ((float)B * (float)L));
  hw::finalize(ws, P, L, 1.f / ((float)B * (float)L), stats, acc, stream);
  return check_launch("mse_head (wide)");
}

int wide_mahalanobis_head(const float* z, const float* c, const float* VI, float* dz, float* score, float* stats, float* acc,
                          float* gram, int gram_accumulate, float upstream, float* ws, int B, int L, hipStream_t stream) {
  const int P = hw::blocks(B);
  hipLaunchKernelGGL(hw::k_mahalanobis_wide, dim3(P), dim3(hw::kBlock), 0, stream, z, c, VI, dz, score, ws, B, L,
                     upstream / (float)B);
  hw::finalize(ws, P, L, 1.f / (float)B, stats, acc, stream);
  if (gram) {
    const int NT = ceil_div(L, 16);
    hipLaunchKernelGGL(hw::k_gram_wide, dim3(ceil_div(NT * NT, hw::kWaves)), dim3(hw::kBlock), 0, stream, z, gram, B, L,
                       gram_accumulate);
  }
  return check_launch("mahalanobis_head (wide)");
}

int wide_poincare_head(const float* z, const float* c, float* dz, float* zh, float* score, float* stats, float* acc,
                       float upstream, float* ws, int B, int L, hipStream_t stream) {
  const int P = hw::blocks(B);
  hipLaunchKernelGGL(hw::k_poincare_wide, dim3(P), dim3(hw::kBlock), 0, stream, z, c, dz, zh, score, ws, B, L, upstream / (float)B);
  hw::finalize(ws, P, L, 1.f / (float)B, stats, acc, stream);
  return check_launch("poincare_head (wide)");
}

int wide_poincare_dist(const float* zh, const float* c, float* score, int B, int L, hipStream_t stream) {
  hipLaunchKernelGGL(hw::k_poincare_dist_wide, dim3(hw::blocks(B)), dim3(hw::kBlock), 0, stream, zh, c, score, B, L);
  return check_launch("poincare_dist (wide)");
}

int wide_poincare_logmap0(const float* y, float* out, int B, int L, hipStream_t stream) {
  hipLaunchKernelGGL(hw::k_poincare_logmap0_wide, dim3(hw::blocks(B)), dim3(hw::kBlock), 0, stream, y, out, B, L);
  return check_launch("poincare_logmap0 (wide)");
}

int wide_center_finalize(const float* acc, float* c, float eps, int L, hipStream_t stream) {
  hipLaunchKernelGGL(hw::k_center_finalize_wide, dim3(ceil_div(L, hw::kBlock)), dim3(hw::kBlock), 0, stream, acc, eps, c, L);
  return check_launch("center_finalize (wide)");
}

int wide_midpoint_finalize(const float* acc, float* c, int L, hipStream_t stream) {
  hipLaunchKernelGGL(hw::k_midpoint_finalize_wide, dim3(1), dim3(64), 0, stream, acc, c, L);
  return check_launch("midpoint_finalize (wide)");
}

}  // namespace coskad
