// The position-wise passes of a TRAINING layer on the stored-Z path at the window lengths 8, 16 and 24 (reference:
// models/graph_layers/stsgcn.py:94-116 with both BatchNorms folded from this batch's statistics, and its backward under autograd).
// None of them sees frames or joints -- only the T V positions of a clip (136 .. 600, a runtime number here):
//
//   apply    U  = Wz Z + Wx PReLU(in) + b                                     (wfold / bias of launch_reduce_fold)
//   data     dZ = Bt dU + Kt Z + kt,   dX_res = Br dU + Kr PReLU(in) + kr     (the coefficient block of k_bwd_fold)
//   stage 1  P = sum dU Z^T,  Q = sum dU PReLU(in)^T,  sdU = sum dU           (partial rows [P | Q | sdU] for sum_stage1_rows)
//
// A tile is one clip x one chunk of <= 64 positions (a clip's positions are cut into equal chunks, multiples of four).  The rows of
// the tile's sources are staged into LDS as 16-byte vectors, zeros beyond the chunk; a workgroup is four waves, wave w owns
// positions 16 w .. 16 w + 15 of the chunk.  Everything is v_mfma_f32_16x16x4_f32 (exact fp32).
//   * apply / data are GEMMs over channels: A operand = a [K][M] weight table held in LDS for the launch (rows padded to whole k-steps
//     with ZERO rows), B operand = four source rows x 16 positions; the results go through LDS and leave as 16-byte vectors.
//     The data pass forms both products from one staging of dU.
//   * stage 1 is a GEMM over positions: both operands are source rows (K = a wave's 16 positions), the accumulators live across
//     the persistent loop, the waves add them into one LDS row one after another and the row leaves as the partial row.
// Grids are persistent with a stated cap; no atomics; a tile's result does not depend on the workgroup or the round that took it.
#include "common.h"
#include "mfma_ops.h"
#include "layer_launch.h"

namespace coskad {
namespace {

constexpr int kFlatThreads = 256;
constexpr int kChunk = 64;              // positions per tile at most
constexpr int kLdG = kChunk + 16;       // row stride of the GEMM images: 16-byte rows, the four rows of a k-step on distinct bank quarters
constexpr int kLdS = kChunk + 2;        // row stride of stage 1's images: == 2 (mod 4), (row, position) operand reads without conflicts
constexpr int kFlatGrid = 1024;         // persistent workgroups of apply / data / stage 1 (= kMaxGridBwd partial rows)

__host__ __device__ inline int pad4(int n) { return (n + 3) / 4 * 4; }
// chunks of a clip and their length
__host__ __device__ inline int flat_chunks(int TV) { return (TV + kChunk - 1) / kChunk; }
__host__ __device__ inline int flat_chunk_len(int TV) { return pad4(ceil_div(TV, flat_chunks(TV))); }
// stride of a weight table of MP = 16 MT columns: the two k rows of a half-wave on distinct banks
__host__ __device__ inline int wtab_stride(int MP) { return MP % 32 == 0 ? MP + 16 : MP; }

struct FlatGemm {
  // sources [B][n?][TV]: out A = Wa^T [s0; s1] + ba, out B = Wb^T [s0; s2] + bb  (s2 / out B absent: n2 = 0)
  const float* s0; const float* s1; const float* s2;
  int n0, n1, n2;
  int act1, act2;             // PReLU(slope) on s1 / s2 on the way in
  const float* slope;
  const float* wa; const float* ba; float* oa;   // wa: [n0 + n1][ldw]
  const float* wb; const float* bb; float* ob;
  int ldw, M;                 // columns of the weight tables in memory, output rows
  int B, TV;
};

// rows [row0, row0 + np) of the image <- n rows of `src` (this clip, positions p0 .. p0 + npos), zeros elsewhere; 16-byte vectors
template <int LDI, bool V4>
__device__ __forceinline__ void flat_stage(float* img, int row0, const float* __restrict__ src, int n, int np, int TV, int p0, int npos,
                                           bool act, float a) {
  constexpr int C4 = kChunk / 4, UB = 4;
  const int total = np * C4;
  for (int e0 = threadIdx.x; e0 < total; e0 += UB * kFlatThreads) {
    float4 v[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int e = e0 + u * kFlatThreads;
      const int r = e / C4, q = e - r * C4;
      const bool ok = e < total && r < n && 4 * q < npos;
      v[u] = ok ? *reinterpret_cast<const float4*>(src + (size_t)r * TV + p0 + 4 * q) : float4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int e = e0 + u * kFlatThreads;
      if (e < total) {
        const int r = e / C4, q = e - r * C4;
        float4 w = v[u];
        if (act) { w.x = prelu_f(w.x, a); w.y = prelu_f(w.y, a); w.z = prelu_f(w.z, a); w.w = prelu_f(w.w, a); }
        float* d = img + (row0 + r) * LDI + 4 * q;
        if constexpr (V4) {
          *reinterpret_cast<float4*>(d) = w;
        } else {
          *reinterpret_cast<float2*>(d) = float2{w.x, w.y};
          *reinterpret_cast<float2*>(d + 2) = float2{w.z, w.w};
        }
      }
    }
  }
}

// MT: 16-row tiles of the output; DUAL: the second product
template <int MT, bool DUAL>
__global__ __launch_bounds__(kFlatThreads) void k_flat_gemm(const FlatGemm g) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int MP = 16 * MT;
  const int WS = wtab_stride(MP);
  const int r0p = pad4(g.n0), r1p = pad4(g.n1), r2p = DUAL ? pad4(g.n2) : 0;
  const int src_rows = r0p + r1p + r2p, out_rows = (DUAL ? 2 : 1) * g.M;
  float* img = lds;                                                   // sources, then (aliased) the outputs
  float* WA = lds + (src_rows > out_rows ? src_rows : out_rows) * kLdG;
  float* WB = WA + (r0p + r1p) * WS;
  float* BA = WB + (DUAL ? (r0p + r2p) * WS : 0);                     // [MP] (+ [MP])
  // the weight tables, once per workgroup: padding rows and columns beyond the table are zeros
  for (int e = threadIdx.x; e < (r0p + r1p) * MP; e += kFlatThreads) {
    const int r = e / MP, c = e - r * MP;
    const int src = r < r0p ? (r < g.n0 ? r : -1) : (r - r0p < g.n1 ? g.n0 + r - r0p : -1);
    WA[r * WS + c] = (src >= 0 && c < g.ldw) ? g.wa[src * g.ldw + c] : 0.f;
  }
  if constexpr (DUAL) {
    for (int e = threadIdx.x; e < (r0p + r2p) * MP; e += kFlatThreads) {
      const int r = e / MP, c = e - r * MP;
      const int src = r < r0p ? (r < g.n0 ? r : -1) : (r - r0p < g.n2 ? g.n0 + r - r0p : -1);
      WB[r * WS + c] = (src >= 0 && c < g.ldw) ? g.wb[src * g.ldw + c] : 0.f;
    }
  }
  for (int e = threadIdx.x; e < (DUAL ? 2 : 1) * MP; e += kFlatThreads) {
    const int c = e % MP;
    const float* b = e < MP ? g.ba : g.bb;
    BA[e] = c < g.M ? b[c] : 0.f;
  }
  const float a_in = g.slope ? g.slope[0] : 0.f;
  const int nch = flat_chunks(g.TV), PC = flat_chunk_len(g.TV);
  const int wave = uniform(threadIdx.x >> 6);
  const long long ntiles = (long long)g.B * nch;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int clip = (int)(tile / nch), ch = (int)(tile - (long long)clip * nch);
    const int p0 = ch * PC, npos = min(PC, g.TV - p0);
    __syncthreads();                                                  // the previous tile's outputs have left (first pass: nothing)
    flat_stage<kLdG, true>(img, 0, g.s0 + (size_t)clip * g.n0 * g.TV, g.n0, r0p, g.TV, p0, npos, false, 0.f);
    flat_stage<kLdG, true>(img, r0p, g.s1 + (size_t)clip * g.n1 * g.TV, g.n1, r1p, g.TV, p0, npos, g.act1 != 0, a_in);
    if constexpr (DUAL)
      flat_stage<kLdG, true>(img, r0p + r1p, g.s2 + (size_t)clip * g.n2 * g.TV, g.n2, r2p, g.TV, p0, npos, g.act2 != 0, a_in);
    __syncthreads();                                                  // (the first pass: the tables too)
    const int lane = tid_here() & 63, i = lane & 15, k = lane >> 4;
    const bool mine = 16 * wave < npos;
    f32x4 acca[MT], accb[DUAL ? MT : 1];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acca[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < (DUAL ? MT : 1); ++mt) accb[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (mine) {
      const float* bp = img + k * kLdG + 16 * wave + i;
      const float* wa = WA + k * WS + i;
      const float* wb = WB + k * WS + i;
      for (int s = 0; s < r0p / 4; ++s) {
        const float b = bp[4 * s * kLdG];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          acca[mt] = mfma4(wa[4 * s * WS + 16 * mt], b, acca[mt]);
          if constexpr (DUAL) accb[mt] = mfma4(wb[4 * s * WS + 16 * mt], b, accb[mt]);
        }
      }
      for (int s = 0; s < r1p / 4; ++s) {
        const float b = bp[(r0p + 4 * s) * kLdG];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acca[mt] = mfma4(wa[(r0p + 4 * s) * WS + 16 * mt], b, acca[mt]);
      }
      if constexpr (DUAL) {
        for (int s = 0; s < r2p / 4; ++s) {
          const float b = bp[(r0p + r1p + 4 * s) * kLdG];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) accb[mt] = mfma4(wb[(r0p + 4 * s) * WS + 16 * mt], b, accb[mt]);
        }
      }
    }
    __syncthreads();                                                  // every wave has read the sources: the outputs take their place
    if (mine) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                 // D layout: register r <-> row 4 k + r, column i
          const int m = 16 * mt + 4 * k + r;
          if (m < g.M) {
            img[m * kLdG + 16 * wave + i] = acca[mt][r] + BA[m];
            if constexpr (DUAL) img[(g.M + m) * kLdG + 16 * wave + i] = accb[mt][r] + BA[MP + m];
          }
        }
    }
    __syncthreads();
    const int n4 = npos >> 2;
    for (int e = threadIdx.x; e < out_rows * n4; e += kFlatThreads) {
      const int r = e / n4, q = e - r * n4;
      const float4 v = *reinterpret_cast<const float4*>(img + r * kLdG + 4 * q);
      float* o = r < g.M ? g.oa + ((size_t)clip * g.M + r) * g.TV : g.ob + ((size_t)clip * g.M + (r - g.M)) * g.TV;
      *reinterpret_cast<float4*>(o + p0 + 4 * q) = v;
    }
  }
}

size_t flat_gemm_lds(const FlatGemm& g, int MT, bool dual) {
  const int MP = 16 * MT, WS = wtab_stride(MP);
  const int r0p = pad4(g.n0), r1p = pad4(g.n1), r2p = dual ? pad4(g.n2) : 0;
  const int src_rows = r0p + r1p + r2p, out_rows = (dual ? 2 : 1) * g.M;
  return ((size_t)(src_rows > out_rows ? src_rows : out_rows) * kLdG + (size_t)(r0p + r1p) * WS + (dual ? (size_t)(r0p + r2p) * WS : 0) +
          2 * (size_t)MP) * sizeof(float);
}

template <int MT, bool DUAL>
int launch_flat_gemm_t(const FlatGemm& g, const char* what, hipStream_t st) {
  const size_t lds = flat_gemm_lds(g, MT, DUAL);
  const long long ntiles = (long long)g.B * flat_chunks(g.TV);
  const int grid = (int)(ntiles < kFlatGrid ? ntiles : kFlatGrid);
  return launch_lds<k_flat_gemm<MT, DUAL>>(what, dim3(grid), dim3(kFlatThreads), lds, st, g);
}

template <bool DUAL>
int launch_flat_gemm(const FlatGemm& g, const char* what, hipStream_t st) {
  const int mt = ceil_div(g.M, 16);
  if (mt == 1) return launch_flat_gemm_t<1, DUAL>(g, what, st);
  if (mt == 2) return launch_flat_gemm_t<2, DUAL>(g, what, st);
  if constexpr (!DUAL) {
    if (mt <= 4) return launch_flat_gemm_t<4, false>(g, what, st);
  }
  return fail(COSKAD_ERR_SHAPE, "%s: %d output rows not supported", what, g.M);
}

// stage 1.  NTO / NTC: 16-row tiles of dU / of Z and X.  LDS: dU, Z (, X) images of the tile, stride kLdS
template <int NTO, int NTC>
__global__ __launch_bounds__(kFlatThreads) void k_flat_stats(const float* __restrict__ in, const float* __restrict__ Zg,
                                                             const float* __restrict__ dU, const float* __restrict__ in_slope,
                                                             float* __restrict__ partials, int B, int TV, int need_q) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int Co = 16 * NTO, Ci = 16 * NTC;
  float* ldu = lds;
  float* ldz = ldu + Co * kLdS;
  float* ldx = ldz + Ci * kLdS;
  const bool pre = in_slope != nullptr;
  const float a_in = pre ? in_slope[0] : 0.f;
  const int nch = flat_chunks(TV), PC = flat_chunk_len(TV);
  const int wave = uniform(threadIdx.x >> 6);
  f32x4 pacc[NTO][NTC], qacc[NTO][NTC];
  float srow[NTO];
#pragma unroll
  for (int a = 0; a < NTO; ++a) {
    srow[a] = 0.f;
#pragma unroll
    for (int b = 0; b < NTC; ++b) { pacc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; qacc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  }
  const long long ntiles = (long long)B * nch;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int clip = (int)(tile / nch), ch = (int)(tile - (long long)clip * nch);
    const int p0 = ch * PC, npos = min(PC, TV - p0);
    __syncthreads();                                                  // the previous tile has been consumed
    flat_stage<kLdS, false>(ldu, 0, dU + (size_t)clip * Co * TV, Co, Co, TV, p0, npos, false, 0.f);
    flat_stage<kLdS, false>(ldz, 0, Zg + (size_t)clip * Ci * TV, Ci, Ci, TV, p0, npos, false, 0.f);
    if (need_q) flat_stage<kLdS, false>(ldx, 0, in + (size_t)clip * Ci * TV, Ci, Ci, TV, p0, npos, pre, a_in);
    __syncthreads();
    if (16 * wave < npos) {                                           // (positions beyond the chunk are zeros: whole idle tiles are skipped)
      const int lane = tid_here() & 63, i = lane & 15, k = lane >> 4;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int off = i * kLdS + 16 * wave + 4 * s + k;
        float a[NTO], bz[NTC], bx[NTC];
#pragma unroll
        for (int t = 0; t < NTO; ++t) a[t] = ldu[16 * t * kLdS + off];
#pragma unroll
        for (int t = 0; t < NTC; ++t) bz[t] = ldz[16 * t * kLdS + off];
        if (need_q) {
#pragma unroll
          for (int t = 0; t < NTC; ++t) bx[t] = ldx[16 * t * kLdS + off];
        }
#pragma unroll
        for (int ta = 0; ta < NTO; ++ta) {
#pragma unroll
          for (int tb = 0; tb < NTC; ++tb) {
            pacc[ta][tb] = mfma4(a[ta], bz[tb], pacc[ta][tb]);
            if (need_q) qacc[ta][tb] = mfma4(a[ta], bx[tb], qacc[ta][tb]);
          }
          srow[ta] += a[ta];
        }
      }
    }
  }
  // the waves add their accumulators into one row in LDS, one after another (fixed order): [P Co Ci][Q Co Ci][sdU Co]
  constexpr int E = 2 * Co * Ci + Co;
  float* row = lds;
  __syncthreads();
  const int lane = threadIdx.x & 63, i = lane & 15, k = lane >> 4;
  for (int w = 0; w < kFlatThreads / 64; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ta = 0; ta < NTO; ++ta) {
#pragma unroll
        for (int tb = 0; tb < NTC; ++tb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {                               // D layout: register r <-> row 4 k + r (of dU), column i (of Z / X)
            float* p = row + (16 * ta + 4 * k + r) * Ci + 16 * tb + i;
            p[0] = (w ? p[0] : 0.f) + pacc[ta][tb][r];
            p[Co * Ci] = (w ? p[Co * Ci] : 0.f) + qacc[ta][tb][r];
          }
        float t = srow[ta];
        t += __shfl_xor(t, 16, 64);
        t += __shfl_xor(t, 32, 64);
        if (k == 0) {
          float* p = row + 2 * Co * Ci + 16 * ta + i;
          p[0] = (w ? p[0] : 0.f) + t;
        }
      }
    }
    __syncthreads();
  }
  float* dst = partials + (size_t)blockIdx.x * E;
  for (int e = threadIdx.x; e < E; e += kFlatThreads) dst[e] = row[e];
}

}  // namespace

bool window_flat_ok(int TV, int Ci, int Co) {
  return TV % 4 == 0 && TV >= 16 && TV <= 640 && (Ci == 16 || Ci == 32) && (Co == 16 || Co == 32 || Co == 64);
}

// U = Wz Z + Wx PReLU(in) + b: wfold [2 Ci][round_up(Co, 16)], bias [round_up(Co, 16)]
int launch_window_apply(const float* Z, const float* in, float* out, const float* wfold, const float* bias, const float* in_slope,
                        int B, int Ci, int Co, int TV, hipStream_t st) {
  if (!window_flat_ok(TV, Ci, Co)) return fail(COSKAD_ERR_SHAPE, "layer_apply_z (window): unsupported (%d positions, %d -> %d)", TV, Ci, Co);
  FlatGemm g{};
  g.s0 = Z; g.n0 = Ci; g.s1 = in; g.n1 = Ci; g.act1 = in_slope != nullptr; g.slope = in_slope;
  g.wa = wfold; g.ba = bias; g.oa = out; g.ldw = round_up(Co, 16); g.M = Co; g.B = B; g.TV = TV;
  ProbeScope probe(KID_LAYER_APPLY, Ci, Co, st);
  return launch_flat_gemm<false>(g, "layer_apply_z (window)", st);
}

// dZ = Bt dU + Kt Z + kt (always) and dX_res = Br dU + Kr PReLU(in) + kr (dXr != NULL) from the coefficient block of k_bwd_fold:
// [wDZ (Co + Ci) x CiP][kt CiP][wDX (Co + Ci) x CiP][kr CiP], CiP = round_up(Ci, 16).  Ci: 2 (the first layer), 16, 32; or the
// few-channel (4 -> 2) layer of coskad_layer_train_window_narrow_ok: M = 4 output rows, K = 6 table rows padded with zero rows
int launch_window_data(const float* in, const float* Z, const float* dU, const float* coef, const float* in_slope, float* dZ, float* dXr,
                       int B, int Ci, int Co, int TV, hipStream_t st) {
  const bool wide = (Ci == 2 || Ci == 16 || Ci == 32) && (Co == 16 || Co == 32 || Co == 64), narrow = Ci == 4 && Co == 2;
  if (TV % 4 || !(wide || narrow))
    return fail(COSKAD_ERR_SHAPE, "layer_bwd (window): unsupported (%d positions, %d -> %d)", TV, Ci, Co);
  const int CiP = round_up(Ci, 16);
  FlatGemm g{};
  g.s0 = dU; g.n0 = Co; g.s1 = Z; g.n1 = Ci; g.slope = in_slope;
  g.wa = coef; g.ba = coef + (Co + Ci) * CiP; g.oa = dZ; g.ldw = CiP; g.M = Ci; g.B = B; g.TV = TV;
  ProbeScope probe(KID_BWD_DATA, Ci, Co, st);
  if (!dXr) return launch_flat_gemm<false>(g, "bwd_data (window)", st);
  g.s2 = in; g.n2 = Ci; g.act2 = in_slope != nullptr;
  g.wb = g.ba + CiP; g.bb = g.wb + (Co + Ci) * CiP; g.ob = dXr;
  return launch_flat_gemm<true>(g, "bwd_data (window)", st);
}

// stage 1 partial rows [P Co Ci][Q Co Ci][sdU Co]; *rows_out rows (<= 1024)
int launch_window_stats(const float* in, const float* Zg, const float* dU, const float* in_slope, float* partials, int B, int Ci, int Co,
                        int TV, int need_q, hipStream_t st, int* rows_out) {
  if (!window_flat_ok(TV, Ci, Co)) return fail(COSKAD_ERR_SHAPE, "layer_bwd stage 1 (window): unsupported (%d positions, %d -> %d)", TV, Ci, Co);
  const long long ntiles = (long long)B * flat_chunks(TV);
  const int grid = (int)(ntiles < kFlatGrid ? ntiles : kFlatGrid);
  *rows_out = grid;
  const size_t img = (size_t)(Co + (need_q ? 2 : 1) * Ci) * kLdS, row = 2 * (size_t)Co * Ci + Co;
  const size_t lds = (img > row ? img : row) * sizeof(float);
#define LAUNCH_FS(NTO, NTC) \
  hipLaunchKernelGGL((k_flat_stats<NTO, NTC>), dim3(grid), dim3(kFlatThreads), lds, st, in, Zg, dU, in_slope, partials, B, TV, need_q)
  {
    ProbeScope probe(KID_BWD_REDUCE, Ci, Co, st);
    if (Co == 16 && Ci == 16) LAUNCH_FS(1, 1);
    else if (Co == 16 && Ci == 32) LAUNCH_FS(1, 2);
    else if (Co == 32 && Ci == 16) LAUNCH_FS(2, 1);
    else if (Co == 32 && Ci == 32) LAUNCH_FS(2, 2);
    else if (Co == 64 && Ci == 16) LAUNCH_FS(4, 1);
    else LAUNCH_FS(4, 2);
  }
#undef LAUNCH_FS
  return check_launch("bwd_stats (window)");
}

}  // namespace coskad

extern "C" {

/* 1 when a (Ci -> Co) ST_GCNN layer of window length T (8, 16, 24) trains on the stored-Z layer kernels (statistics pass, apply,
 * backward); 0 otherwise, T = 12 included (the tile kernels' own geometry).  Host arithmetic. */
int coskad_layer_train_window_ok(int T, int V, int Ci, int Co) {
  return (T == 8 || T == 16 || T == 24) && (V == 17 || V == 25) && (Ci == 2 || Ci == 16 || Ci == 32) &&
         (Co == 16 || Co == 32 || Co == 64);
}

/* 1 when a FEW-CHANNEL (Ci -> Co) layer of window length T (8, 16, 24) trains on the stored-Z layer kernels: the virtual (4 -> 2)
 * layer a stack's last (C -> 2) layer runs as by commutation.  A set of its own beside coskad_layer_train_window_ok.  Host
 * arithmetic. */
int coskad_layer_train_window_narrow_ok(int T, int V, int Ci, int Co) {
  return (T == 8 || T == 16 || T == 24) && (V == 17 || V == 25) && Ci == 4 && Co == 2;
}

}  // extern "C"
