// Plain-GCN layer (learnable_gcn.py:54-72, gcn.py:48-54 + ReLU) as ONE forward and ONE backward kernel per layer:
//
//   O[b] = relu(W^T . X[b] . A'^T + bias)      X [B, Ci, P], W [Ci, Co], A' [P, P] dense, O [B, Co, P], P = T * V
//
// The P x P mixing runs on the narrower channel side: mix first (Y = X . A'^T, then the channel product) when Ci <= Co,
// channel product first (H = W^T . X, then the mixing) otherwise.  Rows (clip, channel) are the M side of the mixing; a
// workgroup takes a GROUP of clips (32 rows; one clip when the narrow side has more than 32 channels), keeps the group's
// narrow-side tensor in LDS and streams A' through the B operand in k-slices straight from L2 (A' is 166 KB at P = 204 and
// 360 KB at P = 300: it fits no LDS, and one B fragment feeds every row tile of the group from registers).  The
// intermediate never leaves the chip unless the caller asks for a copy (`save`: what the backward needs).
//
// Backward: G = dO * (O > 0) is formed on load; db and dW leave as one partial row per workgroup (summed in fp64 in a fixed
// order by k_pgcn_reduce: no atomics, bitwise reproducible); the narrow-side gradient (dY = W . G, or dH = G . A') stays in
// LDS and feeds dX.  For the learnable adjacency the kernel also writes the narrow-side D (dY, or G) so that
// dA'[p', p] = sum_rows D[r, p'] S[r, p] is one coskad_gemm_f32 reduction outside.
//
// fp32 v_mfma_f32_16x16x4_f32 throughout; operand maps as in mfma_ops.h.  Channel counts are padded with zeros in
// registers (predicated loads), never by reading neighbouring data.  P is a runtime multiple of 4 (float4 rows).
#include "mfma_ops.h"

namespace coskad {
namespace pgcn {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kCMax = 64;           // widest channel count on either side
constexpr int kTiles = kCMax / 16;  // row tiles of a group / of a channel side

struct Shape {
  int B, Ci, Co, P;
  int Cn;    // channels on the mixing side
  int G;     // clips per group
  int R16;   // rows of a group, rounded up to the row tile
  int LD;    // LDS row stride (floats): P rounded up to 16, + 4 (keeps float4 rows aligned)
  int NG;    // groups
};

__host__ __device__ inline Shape make_shape(int B, int Ci, int Co, int P) {
  Shape s;
  s.B = B; s.Ci = Ci; s.Co = Co; s.P = P;
  s.Cn = Ci <= Co ? Ci : Co;
  s.G = s.Cn <= 32 ? 32 / s.Cn : 1;
  s.R16 = round_up(s.G * s.Cn, 16);
  s.LD = round_up(P, 16) + 4;
  s.NG = ceil_div(B, s.G);
  return s;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 zero4() { return float4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x4 mfma4x4(const float4& a, const float4& b, f32x4 c) {
  c = mfma4(a.x, b.x, c);
  c = mfma4(a.y, b.y, c);
  c = mfma4(a.z, b.z, c);
  return mfma4(a.w, b.w, c);
}

// out[r][j] = sum_k src[r][k] M(k, j) for the RT row tiles of the LDS image `src` (columns >= P of the image are zero).
//   TRANS: M(k, j) = Ap[j][k] (X . A'^T: both operands as float4 along k; a lane's four k-steps are k0 + 4 (lane >> 4) + 0..3
//          on both sides)            else: M(k, j) = Ap[k][j] (D . A')
// A column tile belongs to one wave, which holds its B fragment in registers for every row tile.
template <bool TRANS, class Store>
__device__ __forceinline__ void mix_rows(const float* src, int LD, int RT, const float* __restrict__ Ap, int P, Store&& store) {
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int i = lane & 15, kq = lane >> 4;
  const int NT = ceil_div(P, 16);
  for (int nt = wave; nt < NT; nt += kWaves) {
    const int j = 16 * nt + i;
    const bool jok = j < P;
    const int jc = jok ? j : P - 1;
    f32x4 acc[kTiles];
#pragma unroll
    for (int q = 0; q < kTiles; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (TRANS) {
      const float* brow = Ap + (size_t)jc * P;
      for (int k0 = 0; k0 < P; k0 += 16) {
        const int k = k0 + 4 * kq;
        const float4 b = (jok && k < P) ? ld4(brow + k) : zero4();
#pragma unroll
        for (int q = 0; q < kTiles; ++q)
          if (q < RT) acc[q] = mfma4x4(ld4(src + (16 * q + i) * LD + k), b, acc[q]);
      }
    } else {
      for (int k0 = 0; k0 < P; k0 += 4) {
        const int k = k0 + kq;   // < P: P is a multiple of 4
        const float bv = Ap[(size_t)k * P + jc];
        const float b = jok ? bv : 0.f;
#pragma unroll
        for (int q = 0; q < kTiles; ++q)
          if (q < RT) acc[q] = mfma4(src[(16 * q + i) * LD + k], b, acc[q]);
      }
    }
    if (jok) {
#pragma unroll
      for (int q = 0; q < kTiles; ++q)
        if (q < RT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) store(16 * q + 4 * kq + r, j, acc[q][r]);
        }
    }
  }
}

// per clip g < ncl of the group and per 16-position tile: out(g, m, p) = sum_k wa(m, k) sb(g, k, p), m < M, k < K
template <class WA, class SB, class Store>
__device__ __forceinline__ void chan_prod(int M, int K, int P, int ncl, WA&& wa, SB&& sb, Store&& store) {
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int i = lane & 15, kq = lane >> 4;
  const int NT = ceil_div(P, 16), MT = ceil_div(M, 16);
  for (int it = wave; it < ncl * NT; it += kWaves) {
    const int g = it / NT, nt = it - g * NT;
    const int j = 16 * nt + i;
    const bool jok = j < P;
    f32x4 acc[kTiles];
#pragma unroll
    for (int q = 0; q < kTiles; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += 4) {
      const int k = k0 + kq;
      const bool kok = k < K;
      const float b = (kok && jok) ? sb(g, k, j) : 0.f;
#pragma unroll
      for (int q = 0; q < kTiles; ++q)
        if (q < MT) {
          const int m = 16 * q + i;
          acc[q] = mfma4((kok && m < M) ? wa(m, k) : 0.f, b, acc[q]);
        }
    }
    if (jok) {
#pragma unroll
      for (int q = 0; q < kTiles; ++q)
        if (q < MT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = 16 * q + 4 * kq + r;
            if (m < M) store(g, m, j, acc[q][r]);
          }
        }
    }
  }
}

// accW[q][t] += sum_p ya(g, c, p) gb(g, o, p) over the group's clips and positions (c = 16 q + i rows, o = 16 t + i columns): the
// weight gradient's share of this wave.  ya / gb return the float4 at positions p4 .. p4 + 3 (p4 < P); dbacc[t] (DB) collects
// the lane's share of sum_p gb(g, o, p).
template <bool DB, class YA, class GB>
__device__ __forceinline__ void wgrad(int Ci, int Co, int P, int ncl, YA&& ya, GB&& gb, f32x4 (&accW)[kTiles][kTiles],
                                      float (&dbacc)[kTiles]) {
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int i = lane & 15, kq = lane >> 4;
  const int NT = ceil_div(P, 16), CT = ceil_div(Ci, 16), OT = ceil_div(Co, 16);
  for (int it = wave; it < ncl * NT; it += kWaves) {
    const int g = it / NT, nt = it - g * NT;
    const int p4 = 16 * nt + 4 * kq;
    const bool pok = p4 < P;
    float4 y[kTiles];
#pragma unroll
    for (int q = 0; q < kTiles; ++q) y[q] = (q < CT && pok && 16 * q + i < Ci) ? ya(g, 16 * q + i, p4) : zero4();
#pragma unroll
    for (int t = 0; t < kTiles; ++t)
      if (t < OT) {
        const float4 gq = (pok && 16 * t + i < Co) ? gb(g, 16 * t + i, p4) : zero4();
        if constexpr (DB) dbacc[t] += (gq.x + gq.y) + (gq.z + gq.w);
#pragma unroll
        for (int q = 0; q < kTiles; ++q)
          if (q < CT) accW[q][t] = mfma4x4(y[q], gq, accW[q][t]);
      }
  }
}

__device__ __forceinline__ void zero_lds(float* buf, int n) {
  for (int e = threadIdx.x; e < n; e += kBlock) buf[e] = 0.f;
}

// ---- forward -------------------------------------------------------------------------------------------------------------
template <bool MIXFIRST>
__global__ __launch_bounds__(kBlock) void k_pgcn_fwd(const float* __restrict__ X, const float* __restrict__ W,
                                                     const float* __restrict__ Ap, const float* __restrict__ bias,
                                                     float* __restrict__ O, float* __restrict__ save, Shape s) {
  extern __shared__ __align__(16) float lds[];
  const int P = s.P, LD = s.LD, Ci = s.Ci, Co = s.Co, RT = s.R16 / 16;
  float* buf0 = lds;
  float* buf1 = lds + s.R16 * LD;     // (MIXFIRST only)
  zero_lds(lds, (MIXFIRST ? 2 : 1) * s.R16 * LD);
  __syncthreads();
  for (int grp = blockIdx.x; grp < s.NG; grp += gridDim.x) {
    const int b0 = grp * s.G;
    const int ncl = min(s.G, s.B - b0);
    const int rows = ncl * s.Cn;
    if constexpr (MIXFIRST) {
      const float* xg = X + (size_t)b0 * Ci * P;
      for (int e = 4 * threadIdx.x; e < rows * P; e += 4 * kBlock) {
        const int r = e / P, c = e - r * P;
        *reinterpret_cast<float4*>(buf0 + r * LD + c) = ld4(xg + e);
      }
      __syncthreads();
      float* sv = save ? save + (size_t)b0 * Ci * P : nullptr;
      mix_rows<true>(buf0, LD, RT, Ap, P, [&](int row, int col, float v) {
        buf1[row * LD + col] = v;
        if (sv && row < rows) sv[(size_t)row * P + col] = v;
      });
      __syncthreads();
      chan_prod(Co, Ci, P, ncl, [&](int m, int k) { return W[k * Co + m]; },
                [&](int g, int k, int j) { return buf1[(g * Ci + k) * LD + j]; },
                [&](int g, int m, int j, float v) {
                  v += bias ? bias[m] : 0.f;
                  O[((size_t)(b0 + g) * Co + m) * P + j] = v > 0.f ? v : 0.f;
                });
      __syncthreads();
    } else {
      float* sv = save ? save + (size_t)b0 * Co * P : nullptr;
      chan_prod(Co, Ci, P, ncl, [&](int m, int k) { return W[k * Co + m]; },
                [&](int g, int k, int j) { return X[((size_t)(b0 + g) * Ci + k) * P + j]; },
                [&](int g, int m, int j, float v) {
                  buf0[(g * Co + m) * LD + j] = v;
                  if (sv) sv[((size_t)g * Co + m) * P + j] = v;
                });
      __syncthreads();
      float* og = O + (size_t)b0 * Co * P;
      mix_rows<true>(buf0, LD, RT, Ap, P, [&](int row, int col, float v) {
        if (row < rows) {
          v += bias ? bias[row % Co] : 0.f;
          og[(size_t)row * P + col] = v > 0.f ? v : 0.f;
        }
      });
      __syncthreads();
    }
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------
// partial row of this workgroup: [Ci * Co of dW][Co of db]
template <bool MIXFIRST>
__global__ __launch_bounds__(kBlock) void k_pgcn_bwd(const float* __restrict__ X, const float* __restrict__ S,
                                                     const float* __restrict__ O, const float* __restrict__ dO,
                                                     const float* __restrict__ W, const float* __restrict__ Ap,
                                                     float* __restrict__ dX, float* __restrict__ D, float* __restrict__ partials,
                                                     Shape s) {
  extern __shared__ __align__(16) float lds[];
  const int P = s.P, LD = s.LD, Ci = s.Ci, Co = s.Co, RT = s.R16 / 16;
  const int lane = threadIdx.x & 63, wave = uniform(threadIdx.x >> 6);
  const int i = lane & 15, kq = lane >> 4;
  float* buf0 = lds;
  float* buf1 = lds + s.R16 * LD;     // (channel-first only)
  zero_lds(lds, (MIXFIRST ? 1 : 2) * s.R16 * LD);
  __syncthreads();
  f32x4 accW[kTiles][kTiles];
  float dbacc[kTiles];
#pragma unroll
  for (int q = 0; q < kTiles; ++q) {
    dbacc[q] = 0.f;
#pragma unroll
    for (int t = 0; t < kTiles; ++t) accW[q][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  float dbrow = 0.f;       // channel-first: this thread's share of one row of G, summed over the groups

  auto gval4 = [&](size_t off) {       // G = dO * (O > 0), four positions
    const float4 o = ld4(O + off), d = ld4(dO + off);
    return float4{o.x > 0.f ? d.x : 0.f, o.y > 0.f ? d.y : 0.f, o.z > 0.f ? d.z : 0.f, o.w > 0.f ? d.w : 0.f};
  };

  for (int grp = blockIdx.x; grp < s.NG; grp += gridDim.x) {
    const int b0 = grp * s.G;
    const int ncl = min(s.G, s.B - b0);
    const int rows = ncl * s.Cn;
    if constexpr (MIXFIRST) {
      // dY = W . G per clip -> LDS (and D); dW += Y . G^T, db += sum G
      float* dg = D ? D + (size_t)b0 * Ci * P : nullptr;
      chan_prod(Ci, Co, P, ncl, [&](int m, int k) { return W[m * Co + k]; },
                [&](int g, int k, int j) {
                  const size_t off = ((size_t)(b0 + g) * Co + k) * P + j;
                  return O[off] > 0.f ? dO[off] : 0.f;
                },
                [&](int g, int m, int j, float v) {
                  buf0[(g * Ci + m) * LD + j] = v;
                  if (dg) dg[((size_t)g * Ci + m) * P + j] = v;
                });
      wgrad<true>(Ci, Co, P, ncl, [&](int g, int c, int p4) { return ld4(S + ((size_t)(b0 + g) * Ci + c) * P + p4); },
                  [&](int g, int o, int p4) { return gval4(((size_t)(b0 + g) * Co + o) * P + p4); }, accW, dbacc);
      __syncthreads();
      if (dX) {
        float* xg = dX + (size_t)b0 * Ci * P;
        mix_rows<false>(buf0, LD, RT, Ap, P, [&](int row, int col, float v) {
          if (row < rows) xg[(size_t)row * P + col] = v;
        });
      }
      __syncthreads();
    } else {
      // G rows -> LDS (and D); db; dH = G . A' -> LDS; dX = W . dH per clip; dW += X . dH^T
      const size_t base = (size_t)b0 * Co * P;
      for (int e = 4 * threadIdx.x; e < rows * P; e += 4 * kBlock) {
        const int r = e / P, c = e - r * P;
        const float4 g = gval4(base + e);
        *reinterpret_cast<float4*>(buf0 + r * LD + c) = g;
        if (D) *reinterpret_cast<float4*>(D + base + e) = g;
      }
      __syncthreads();
      {
        const int row = threadIdx.x >> 2, part = threadIdx.x & 3;
        if (row < rows) {
          float sum = 0.f;
          for (int p = part; p < P; p += 4) sum += buf0[row * LD + p];
          dbrow += sum;
        }
      }
      mix_rows<false>(buf0, LD, RT, Ap, P, [&](int row, int col, float v) { buf1[row * LD + col] = v; });
      __syncthreads();
      if (dX)
        chan_prod(Ci, Co, P, ncl, [&](int m, int k) { return W[m * Co + k]; },
                  [&](int g, int k, int j) { return buf1[(g * Co + k) * LD + j]; },
                  [&](int g, int m, int j, float v) { dX[((size_t)(b0 + g) * Ci + m) * P + j] = v; });
      wgrad<false>(Ci, Co, P, ncl, [&](int g, int c, int p4) { return ld4(X + ((size_t)(b0 + g) * Ci + c) * P + p4); },
                   [&](int g, int o, int p4) { return ld4(buf1 + (g * Co + o) * LD + p4); }, accW, dbacc);
      __syncthreads();
    }
  }

  // the workgroup's partial row: waves one after another (fixed order), then db from the per-lane / per-thread shares
  float* red = buf0;                 // [64][64] image of dW, then 1024 floats of db shares (the smallest image has 5760 floats)
  float* sdb = buf0 + kCMax * kCMax;
  const int CT = ceil_div(Ci, 16), OT = ceil_div(Co, 16);
  for (int w = 0; w < kWaves; ++w) {
    if (wave == w) {
#pragma unroll
      for (int q = 0; q < kTiles; ++q)
#pragma unroll
        for (int t = 0; t < kTiles; ++t)
          if (q < CT && t < OT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float* dst = red + (16 * q + 4 * kq + r) * kCMax + 16 * t + i;
              *dst = w == 0 ? accW[q][t][r] : *dst + accW[q][t][r];
            }
          }
    }
    __syncthreads();
  }
  if constexpr (MIXFIRST) {
#pragma unroll
    for (int t = 0; t < kTiles; ++t) sdb[(wave * kTiles + t) * 64 + lane] = dbacc[t];
  } else {
    sdb[threadIdx.x] = dbrow;
  }
  __syncthreads();
  float* prow = partials + (size_t)blockIdx.x * (Ci * Co + Co);
  for (int e = threadIdx.x; e < Ci * Co; e += kBlock) {
    const int c = e / Co, o = e - c * Co;
    prow[e] = red[c * kCMax + o];
  }
  if ((int)threadIdx.x < Co) {
    const int o = threadIdx.x;
    float sum = 0.f;
    if constexpr (MIXFIRST) {
      for (int w = 0; w < kWaves; ++w)
        for (int k = 0; k < 4; ++k) sum += sdb[(w * kTiles + (o >> 4)) * 64 + 16 * k + (o & 15)];
    } else {
      for (int row = o; row < s.G * Co; row += Co)
        for (int k = 0; k < 4; ++k) sum += sdb[4 * row + k];
    }
    prow[Ci * Co + o] = sum;
  }
}

// [dW | db] (+)= the column sums of the partial rows: 64 columns x 16 row slices per block, fp64, fixed order
__global__ __launch_bounds__(1024) void k_pgcn_reduce(const float* __restrict__ partials, int rows, int E, int nW,
                                                       float* __restrict__ dW, float* __restrict__ db, int accumulate) {
  __shared__ double sh[1024];
  const int e = blockIdx.x * 64 + (threadIdx.x % 64);
  const double t = column_sum_f64<64>(partials, rows, (size_t)E, e, e < E, sh);
  if (threadIdx.x < 64 && e < E) {
    float* o = e < nW ? dW + e : (db ? db + (e - nW) : nullptr);
    if (o) *o = accumulate ? *o + (float)t : (float)t;
  }
}

inline int grid_of(const Shape& s, int grid_cap) {
  constexpr int kGridCap = 512;      // persistent: two workgroups per CU where the LDS image allows
  const int cap = grid_cap > 0 ? grid_cap : kGridCap;
  return s.NG < cap ? s.NG : cap;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

int check_shape(const char* what, int B, int Ci, int Co, int P);

}  // namespace pgcn
}  // namespace coskad

using namespace coskad;

extern "C" {

/* 1 where the fused plain-GCN kernels take a (Ci -> Co) layer on P = T * V positions: 1 <= Ci, Co <= 64 and the 12-frame
 * window of the four joint layouts (P in {168, 204, 216, 300}).  Host arithmetic. */
int coskad_plain_gcn_ok(int Ci, int Co, int P) {
  return Ci >= 1 && Ci <= pgcn::kCMax && Co >= 1 && Co <= pgcn::kCMax && (P == 168 || P == 204 || P == 216 || P == 300);
}

}  // extern "C"

namespace coskad {
namespace pgcn {
int check_shape(const char* what, int B, int Ci, int Co, int P) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || P <= 0) return fail(COSKAD_ERR_ARG, "%s: B=%d Ci=%d Co=%d P=%d", what, B, Ci, Co, P);
  if (!coskad_plain_gcn_ok(Ci, Co, P))
    return fail(COSKAD_ERR_SHAPE, "%s: unsupported layer (Ci=%d, Co=%d, P=%d): 1..64 channels, P = 12 x {14,17,18,25}", what, Ci, Co, P);
  return COSKAD_OK;
}
}  // namespace pgcn
}  // namespace coskad

extern "C" {

size_t coskad_plain_gcn_ws_bytes(int B, int Ci, int Co, int P, int grid_cap) {
  if (B <= 0 || !coskad_plain_gcn_ok(Ci, Co, P)) return 0;
  const pgcn::Shape s = pgcn::make_shape(B, Ci, Co, P);
  return (size_t)pgcn::grid_of(s, grid_cap) * (Ci * Co + Co) * sizeof(float);
}

int coskad_plain_gcn_fwd_f32(const float* X, const float* W, const float* Ap, const float* bias, float* O, float* save, int B,
                             int Ci, int Co, int P, int grid_cap, hipStream_t stream) {
  if (!X || !W || !Ap || !O) return fail(COSKAD_ERR_ARG, "plain_gcn_fwd: null pointer");
  if (int rc = pgcn::check_shape("plain_gcn_fwd", B, Ci, Co, P)) return rc;
  if (grid_cap < 0) return fail(COSKAD_ERR_ARG, "plain_gcn_fwd: grid_cap=%d", grid_cap);
  if (!pgcn::aligned16(X) || !pgcn::aligned16(Ap)) return fail(COSKAD_ERR_ARG, "plain_gcn_fwd: X and A' must be 16-byte aligned");
  const pgcn::Shape s = pgcn::make_shape(B, Ci, Co, P);
  const int grid = pgcn::grid_of(s, grid_cap);
  const bool mixfirst = Ci <= Co;
  const size_t lds = (size_t)(mixfirst ? 2 : 1) * s.R16 * s.LD * sizeof(float);
  if (mixfirst)
    return launch_lds<pgcn::k_pgcn_fwd<true>>("plain_gcn_fwd", dim3(grid), dim3(pgcn::kBlock), lds, stream, X, W, Ap, bias, O, save, s);
  return launch_lds<pgcn::k_pgcn_fwd<false>>("plain_gcn_fwd", dim3(grid), dim3(pgcn::kBlock), lds, stream, X, W, Ap, bias, O, save, s);
}

int coskad_plain_gcn_bwd_f32(const float* X, const float* S, const float* O, const float* dO, const float* W, const float* Ap,
                             float* dX, float* dW, float* db, float* D, void* ws, size_t ws_bytes, int B, int Ci, int Co, int P,
                             int need_dx, int need_da, int accumulate, int grid_cap, hipStream_t stream) {
  if (!O || !dO || !W || !Ap || !dW || !ws) return fail(COSKAD_ERR_ARG, "plain_gcn_bwd: null pointer");
  if (int rc = pgcn::check_shape("plain_gcn_bwd", B, Ci, Co, P)) return rc;
  const bool mixfirst = Ci <= Co;
  if (mixfirst ? !S : !X) return fail(COSKAD_ERR_ARG, "plain_gcn_bwd: null pointer (%s)", mixfirst ? "the saved Y" : "X");
  if ((need_dx && !dX) || (need_da && !D)) return fail(COSKAD_ERR_ARG, "plain_gcn_bwd: null pointer (dX / D asked for)");
  if (grid_cap < 0) return fail(COSKAD_ERR_ARG, "plain_gcn_bwd: grid_cap=%d", grid_cap);
  if (!pgcn::aligned16(X) || !pgcn::aligned16(S) || !pgcn::aligned16(O) || !pgcn::aligned16(dO) || !pgcn::aligned16(D))
    return fail(COSKAD_ERR_ARG, "plain_gcn_bwd: activations must be 16-byte aligned");
  if (ws_bytes < coskad_plain_gcn_ws_bytes(B, Ci, Co, P, grid_cap))
    return fail(COSKAD_ERR_WORKSPACE, "plain_gcn_bwd: workspace of %zu B, %zu needed", ws_bytes,
                coskad_plain_gcn_ws_bytes(B, Ci, Co, P, grid_cap));
  const pgcn::Shape s = pgcn::make_shape(B, Ci, Co, P);
  const int grid = pgcn::grid_of(s, grid_cap);
  const size_t lds = (size_t)(mixfirst ? 1 : 2) * s.R16 * s.LD * sizeof(float);
  float* partials = reinterpret_cast<float*>(ws);
  float* dx = need_dx ? dX : nullptr;
  float* d = need_da ? D : nullptr;
  const int rc = mixfirst ? launch_lds<pgcn::k_pgcn_bwd<true>>("plain_gcn_bwd", dim3(grid), dim3(pgcn::kBlock), lds, stream, X, S, O, dO, W, Ap,
                                                              dx, d, partials, s)
                          : launch_lds<pgcn::k_pgcn_bwd<false>>("plain_gcn_bwd", dim3(grid), dim3(pgcn::kBlock), lds, stream, X, S, O, dO, W, Ap,
                                                               dx, d, partials, s);
  if (rc) return rc;
  const int E = Ci * Co + Co;
  hipLaunchKernelGGL(pgcn::k_pgcn_reduce, dim3(ceil_div(E, 64)), dim3(1024), 0, stream, partials, grid, E, Ci * Co, dW, db, accumulate);
  return check_launch("plain_gcn_bwd");
}

}  // extern "C"
