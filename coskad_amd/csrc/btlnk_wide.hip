// Bottleneck projection of STSE at 16 < latent <= 512 (reference models/sts/ae.py:97-101,154-157):
//     z = PReLU(U) W^T + b,   U [B, K] (K = hid * T * V, the last layer's pre-activation; slope NULL: U is already activated)
// and its backward, as three fp32 GEMMs on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains at the MFMA rate):
//
//   FWD : z-partials [KS][B][L] = PReLU(U) W^T over KS slices of K     (M = B, N = L, reduction K; PReLU applied on the U load)
//   DX  : dU = (dz W) * PReLU'(U), dslope partials                     (M = B, N = K, reduction L; epilogue reads U)
//   DW  : dW-partials [S][L][K] = dz^T PReLU(U) over S chunks of clips  (M = L, N = K, reduction B; PReLU applied on the U load)
//
// Block = 4 waves = a (32 TM) x (32 TN) tile, the reduction axis in steps of 16 through double-buffered LDS (k-major images:
// an MFMA operand read is 16 consecutive floats per k); a wave owns (16 TM) x (16 TN).  Global loads map consecutive threads
// onto whichever operand dimension is contiguous in memory; every load is bounds-checked, so B, L and K may be ragged.
// Partials are summed in a fixed order (k_wfwd_sum, launch_btlnk_reduce): no atomics, bitwise-repeatable.  The slice count of
// the forward depends on (K, L) only, so a clip's latent does not depend on the batch it arrives in.
//
// DX and DW stay two passes over U: fusing the dW contraction into the dU pass would hold an L x (K tile)
// accumulator per block across the clip loop -- 512 x 128 floats = 256 registers per lane at L = 512 on top of the dU tile.
#include "common.h"
#include "layer_launch.h"

namespace coskad {
namespace bw {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int BK = 16;
enum { FWD = 0, DX = 1, DW = 2 };

struct Args {
  const float* U;
  const float* W;
  const float* dz;
  const float* slope;
  float* out;          // FWD: partials [KS][B][L]; DX: dU; DW: partials [S][L][K]
  float* dap;          // DX: one dslope partial per block
  int B, K, L;
  int rchunk;          // reduction elements per blockIdx.z (a multiple of BK): FWD a slice of K, DW a chunk of clips
};

template <int MODE, int TM, int TN>
__global__ __launch_bounds__(256) void k_wide(Args a) {
  constexpr int BM = 32 * TM, BN = 32 * TN;
  constexpr int LDA = BM + 4, LDB = BN + 4;
  constexpr int EA = BM / 16, EB = BN / 16;
  constexpr bool A_RC = MODE != DW;     // A contiguous along the reduction axis (FWD: U rows, DX: dz rows); DW: dz^T, along m
  constexpr bool B_NC = MODE != FWD;    // B contiguous along n (DX: W rows, DW: U rows); FWD: W^T, along the reduction axis
  __shared__ __attribute__((aligned(16))) float As[2][BK][LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][LDB];
  __shared__ float sred[4];
  const int M = MODE == DW ? a.L : a.B;
  const int N = MODE == FWD ? a.L : a.K;
  const int R = MODE == FWD ? a.K : (MODE == DX ? a.L : a.B);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const int wm = (wave >> 1) * 16 * TM, wn = (wave & 1) * 16 * TN;
  const int j = lane & 15, q = lane >> 4;
  const int r_first = blockIdx.z * a.rchunk, r_last = min(R, r_first + a.rchunk);
  const bool pre = a.slope != nullptr;
  const float sl = pre ? a.slope[0] : 0.f;
  int am[EA], ar[EA], bn[EB], br[EB];
#pragma unroll
  for (int i = 0; i < EA; ++i) {
    if (A_RC) { am[i] = (tid >> 4) + 16 * i; ar[i] = tid & 15; }
    else { am[i] = tid % BM; ar[i] = tid / BM + (256 / BM) * i; }
  }
#pragma unroll
  for (int i = 0; i < EB; ++i) {
    if (B_NC) { bn[i] = tid % BN; br[i] = tid / BN + (256 / BN) * i; }
    else { bn[i] = (tid >> 4) + 16 * i; br[i] = tid & 15; }
  }
  f32x4 acc[TM][TN];
#pragma unroll
  for (int x = 0; x < TM; ++x)
#pragma unroll
    for (int y = 0; y < TN; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int total = r_last > r_first ? ceil_div(r_last - r_first, BK) : 0;
  float ra[EA], rb[EB];
  auto gload = [&](int it) {
    const int r0 = r_first + it * BK;
#pragma unroll
    for (int i = 0; i < EA; ++i) {
      const int m = m0 + am[i], r = r0 + ar[i];
      float v = 0.f;
      if (m < M && r < r_last) {
        if (MODE == FWD) { v = a.U[(size_t)m * a.K + r]; if (pre) v = prelu_f(v, sl); }
        else if (MODE == DX) v = a.dz[(size_t)m * a.L + r];
        else v = a.dz[(size_t)r * a.L + m];
      }
      ra[i] = v;
    }
#pragma unroll
    for (int i = 0; i < EB; ++i) {
      const int n = n0 + bn[i], r = r0 + br[i];
      float v = 0.f;
      if (n < N && r < r_last) {
        if (MODE == FWD) v = a.W[(size_t)n * a.K + r];
        else if (MODE == DX) v = a.W[(size_t)r * a.K + n];
        else { v = a.U[(size_t)r * a.K + n]; if (pre) v = prelu_f(v, sl); }
      }
      rb[i] = v;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < EA; ++i) As[buf][ar[i]][am[i]] = ra[i];
#pragma unroll
    for (int i = 0; i < EB; ++i) Bs[buf][br[i]][bn[i]] = rb[i];
  };
  if (total > 0) {
    gload(0);
    sstore(0);
  }
  __syncthreads();
  for (int it = 0; it < total; ++it) {
    const int buf = it & 1;
    if (it + 1 < total) gload(it + 1);
#pragma unroll
    for (int s = 0; s < BK / 4; ++s) {
      float av[TM], bv[TN];
#pragma unroll
      for (int x = 0; x < TM; ++x) av[x] = As[buf][4 * s + q][wm + 16 * x + j];
#pragma unroll
      for (int y = 0; y < TN; ++y) bv[y] = Bs[buf][4 * s + q][wn + 16 * y + j];
#pragma unroll
      for (int x = 0; x < TM; ++x)
#pragma unroll
        for (int y = 0; y < TN; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[x], bv[y], acc[x][y], 0, 0, 0);
    }
    if (it + 1 < total) sstore(buf ^ 1);
    __syncthreads();
  }
  // epilogue: lane (j, q), reg r <-> row m0 + wm + 16 x + 4 q + r, column n0 + wn + 16 y + j
  float da = 0.f;
#pragma unroll
  for (int x = 0; x < TM; ++x)
#pragma unroll
    for (int y = 0; y < TN; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * x + 4 * q + r, n = n0 + wn + 16 * y + j;
        if (m >= M || n >= N) continue;
        const float v = acc[x][y][r];
        if (MODE == DX) {
          const size_t e = (size_t)m * a.K + n;
          const float u = a.U[e];
          float g = v;
          if (pre) {
            da += u < 0.f ? g * u : 0.f;
            g = u > 0.f ? g : sl * g;
          }
          a.out[e] = g;
        } else {
          a.out[((size_t)blockIdx.z * M + m) * N + n] = v;
        }
      }
  if (MODE == DX) {
    da = wave_sum(da);
    if (lane == 0) sred[wave] = da;
    __syncthreads();
    if (tid == 0) a.dap[blockIdx.y * gridDim.x + blockIdx.x] = (sred[0] + sred[1]) + (sred[2] + sred[3]);
  }
}

// z[n][l] = sum_s part[s][n][l] + b[l], slices in order
__global__ __launch_bounds__(256) void k_wfwd_sum(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ z,
                                                  int B, int L, int KS) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t E = (size_t)B * L;
  if (e >= E) return;
  float s = 0.f;
  for (int k = 0; k < KS; ++k) s += part[(size_t)k * E + e];
  z[e] = s + (bias ? bias[e % L] : 0.f);
}

// Forward: the N tile follows L (32 / 64 / 128 latents per block), 128 clips per block; the K slices depend on (K, L) only
// and give ~512 blocks at B = 4096 (two 4-wave blocks per CU).
static int fwd_tn(int L) { return L <= 32 ? 1 : (L <= 64 ? 2 : 4); }
static int fwd_rchunk(int K, int L) {
  const int nt = ceil_div(L, 32 * fwd_tn(L));
  int ks = 16 / nt;
  if (ks < 2) ks = 2;
  const int kmax = ceil_div(K, 8 * BK);           // at least eight 16-wide steps per slice
  if (ks > kmax) ks = kmax;
  if (ks < 1) ks = 1;
  return round_up(ceil_div(K, ks), BK);
}
static int fwd_slices(int K, int L) { return ceil_div(K, fwd_rchunk(K, L)); }

// Weight gradient: the M tile follows L (32 / 64 / 128 rows), 128 columns of K per block, clip chunks to ~1024 blocks
static int dw_tm(int L) { return L <= 32 ? 1 : (L <= 64 ? 2 : 4); }
static int dw_chunk(int B, int K, int L) {
  const int tiles = ceil_div(K, 128) * ceil_div(L, 32 * dw_tm(L));
  int s = (1024 + tiles / 2) / tiles;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  return round_up(ceil_div(B, s), BK);
}
static int dw_chunks(int B, int K, int L) { return ceil_div(B, dw_chunk(B, K, L)); }
static int dx_blocks(int B, int K) { return ceil_div(K, 128) * ceil_div(B, 128); }

template <int MODE, int TM, int TN>
static void launch(const Args& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((k_wide<MODE, TM, TN>), grid, dim3(256), 0, stream, a);
}

}  // namespace bw

size_t wide_btlnk_fwd_ws_bytes(int B, int K, int L) {
  if (B <= 0 || K <= 0 || L <= 0) return 0;
  return (size_t)bw::fwd_slices(K, L) * (size_t)B * (size_t)L * sizeof(float);
}

size_t wide_btlnk_bwd_ws_bytes(int B, int K, int L) {
  if (B <= 0 || K <= 0 || L <= 0) return 0;
  return ((size_t)bw::dw_chunks(B, K, L) * L * K + (size_t)bw::dx_blocks(B, K) + 64) * sizeof(float);
}

int wide_btlnk_fwd(const float* U, const float* W, const float* bias, const float* slope, float* z, void* ws, int B, int K, int L,
                   hipStream_t stream) {
  const int ks = bw::fwd_slices(K, L);
  float* part = reinterpret_cast<float*>(ws);
  bw::Args a{U, W, nullptr, slope, part, nullptr, B, K, L, bw::fwd_rchunk(K, L)};
  const int tn = bw::fwd_tn(L);
  const dim3 grid(ceil_div(L, 32 * tn), ceil_div(B, 128), ks);
  if (tn == 1) bw::launch<bw::FWD, 4, 1>(a, grid, stream);
  else if (tn == 2) bw::launch<bw::FWD, 4, 2>(a, grid, stream);
  else bw::launch<bw::FWD, 4, 4>(a, grid, stream);
  int rc = check_launch("btlnk_fwd (wide)");
  if (rc) return rc;
  const size_t E = (size_t)B * L;
  hipLaunchKernelGGL(bw::k_wfwd_sum, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, stream, part, bias, z, B, L, ks);
  return check_launch("btlnk_fwd_sum (wide)");
}

int wide_btlnk_bwd(const float* U, const float* W, const float* dz, const float* slope, float* dU, float* dW, float* db,
                   float* dslope, void* ws, int accumulate, int B, int K, int L, hipStream_t stream) {
  const int S = bw::dw_chunks(B, K, L);
  float* dWp = reinterpret_cast<float*>(ws);
  float* dap = dWp + (size_t)S * L * K;
  // dU and the dslope partials
  bw::Args ax{U, W, dz, slope, dU, dap, B, K, L, round_up(L, bw::BK)};
  bw::launch<bw::DX, 4, 4>(ax, dim3(ceil_div(K, 128), ceil_div(B, 128), 1), stream);
  int rc = check_launch("btlnk_bwd_dx (wide)");
  if (rc) return rc;
  // dW partials per clip chunk
  bw::Args aw{U, W, dz, slope, dWp, nullptr, B, K, L, bw::dw_chunk(B, K, L)};
  const int tm = bw::dw_tm(L);
  const dim3 grid(ceil_div(K, 128), ceil_div(L, 32 * tm), S);
  if (tm == 1) bw::launch<bw::DW, 1, 4>(aw, grid, stream);
  else if (tm == 2) bw::launch<bw::DW, 2, 4>(aw, grid, stream);
  else bw::launch<bw::DW, 4, 4>(aw, grid, stream);
  if ((rc = check_launch("btlnk_bwd_dw (wide)"))) return rc;
  return launch_btlnk_reduce(dWp, S, (size_t)L * K, dW, dz, B, L, db, dap, bw::dx_blocks(B, K), (dslope && slope) ? dslope : nullptr,
                             accumulate, stream, nullptr, 0, 0, nullptr);
}

}  // namespace coskad
