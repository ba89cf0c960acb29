// `rev_btlnk` of the decoder models (reference models/sts/ae.py:223-227: nn.Linear(latent_dim -> hidden * T * V)) and its autograd at
// 16 < latent <= 512, where the three products ARE GEMM-shaped (54.8 GFLOP each at L = 512, B = 4096, N = 13 056): three fp32 GEMMs
// on v_mfma_f32_16x16x4_f32 -- the FWD / DX / DW modes of csrc/btlnk_wide.hip with the roles of the operands exchanged:
//
//   FWD : H[b][n]  = sum_l z[b][l] W[n][l] + bias[n]           (rows p = n, columns q = b, reduction l: whole, no partials)
//   DZ  : dz-partials [KS][B][L] = dH W over KS slices of N     (rows p = l, columns q = b, reduction n)
//   DW  : dW-partials [S][N][L]  = dH^T z over S chunks of clips (rows p = l, columns q = n, reduction b), db-partials [S][N] = the
//         column sums of the dH values the block stages anyway
//
// An MFMA lane holds FOUR CONSECUTIVE ROWS of one column, so the row dimension p is whichever is contiguous in the output: H rows
// are written as 16-byte vectors, two neighbouring 16-row tiles interleaved (pidx) so that a lane owns 8 consecutive floats and the
// four lanes of a clip cover a whole 128-byte line.  Block = 4 waves = a (32 TP) x (32 TQ) tile, the reduction axis in steps of 16
// through double-buffered LDS (k-major images), every load bounds-checked: B, L and N may be ragged (N % 4 == 0 for the vector
// stores).  Partials are summed in a fixed order straight into the destination (k_sum_slices): no atomics, bitwise-repeatable.  The
// slice count of DZ depends on (N, L) only, so a clip's dz does not depend on the batch it arrives in.
#include "common.h"
#include "layer_launch.h"

namespace coskad {
namespace rbw {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int BK = 16;
enum { FWD = 0, DZ = 1, DW = 2 };

struct Args {
  const float* z;
  const float* W;
  const float* dH;
  const float* bias;
  float* out;          // FWD: H; DZ: partials [KS][B][L]; DW: partials [S][N][L]
  float* dbp;          // DW: partials [S][N] of the bias gradient
  int B, N, L;
  int rchunk;          // reduction elements per blockIdx.z (a multiple of BK)
};

// row of tile x, MFMA row i (0..15) within a wave's 16 TP rows; 4 q + r -> 4 consecutive rows.  Even TP: tiles 2a, 2a + 1 interleaved
// in groups of four, so that lane group q owns rows 8 q .. 8 q + 7 of the 32-row pair.
template <int TP>
__device__ __forceinline__ int pidx(int x, int i) {
  if (TP % 2 == 0) return (x >> 1) * 32 + (i >> 2) * 8 + (x & 1) * 4 + (i & 3);
  return 16 * x + i;
}

template <int MODE, int TP, int TQ>
__global__ __launch_bounds__(256) void k_rev_wide(Args a) {
  constexpr int BP = 32 * TP, BQ = 32 * TQ;
  constexpr int LDP = BP + 4, LDQ = BQ + 4;
  constexpr int EP = BP / 16, EQ = BQ / 16;
  constexpr bool P_RC = MODE == FWD;    // P contiguous along the reduction axis (FWD: W rows); DZ: W rows along l, DW: z rows along l
  constexpr bool Q_RC = MODE != DW;     // Q contiguous along the reduction axis (FWD: z rows, DZ: dH rows); DW: dH rows along n
  __shared__ __attribute__((aligned(16))) float Ps[2][BK][LDP];
  __shared__ __attribute__((aligned(16))) float Qs[2][BK][LDQ];
  const int P = MODE == FWD ? a.N : a.L;
  const int Q = MODE == DW ? a.N : a.B;
  const int R = MODE == FWD ? a.L : (MODE == DZ ? a.N : a.B);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = blockIdx.x * BP, q0 = blockIdx.y * BQ;
  const int wp = (wave >> 1) * 16 * TP, wq = (wave & 1) * 16 * TQ;
  const int j = lane & 15, q = lane >> 4;
  const int r_first = blockIdx.z * a.rchunk, r_last = min(R, r_first + a.rchunk);
  const bool want_db = MODE == DW && blockIdx.x == 0;
  int pp[EP], pr[EP], qq[EQ], qr[EQ];
#pragma unroll
  for (int i = 0; i < EP; ++i) {
    if (P_RC) { pp[i] = (tid >> 4) + 16 * i; pr[i] = tid & 15; }
    else { pp[i] = tid % BP; pr[i] = tid / BP + (256 / BP) * i; }
  }
#pragma unroll
  for (int i = 0; i < EQ; ++i) {
    if (Q_RC) { qq[i] = (tid >> 4) + 16 * i; qr[i] = tid & 15; }
    else { qq[i] = tid % BQ; qr[i] = tid / BQ + (256 / BQ) * i; }
  }
  f32x4 acc[TP][TQ];
#pragma unroll
  for (int x = 0; x < TP; ++x)
#pragma unroll
    for (int y = 0; y < TQ; ++y) acc[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int total = r_last > r_first ? ceil_div(r_last - r_first, BK) : 0;
  float rp[EP], rq[EQ];
  float colsum = 0.f;                   // DW: sum over this block's clips of dH[.][q0 + tid % BQ] (every load of a thread is one column)
  auto gload = [&](int it) {
    const int r0 = r_first + it * BK;
#pragma unroll
    for (int i = 0; i < EP; ++i) {
      const int p = p0 + pp[i], r = r0 + pr[i];
      float v = 0.f;
      if (p < P && r < r_last) {
        if (MODE == FWD) v = a.W[(size_t)p * a.L + r];
        else if (MODE == DZ) v = a.W[(size_t)r * a.L + p];
        else v = a.z[(size_t)r * a.L + p];
      }
      rp[i] = v;
    }
#pragma unroll
    for (int i = 0; i < EQ; ++i) {
      const int c = q0 + qq[i], r = r0 + qr[i];
      float v = 0.f;
      if (c < Q && r < r_last) {
        if (MODE == FWD) v = a.z[(size_t)c * a.L + r];
        else if (MODE == DZ) v = a.dH[(size_t)c * a.N + r];
        else v = a.dH[(size_t)r * a.N + c];
      }
      rq[i] = v;
      if (MODE == DW) colsum += v;
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < EP; ++i) Ps[buf][pr[i]][pp[i]] = rp[i];
#pragma unroll
    for (int i = 0; i < EQ; ++i) Qs[buf][qr[i]][qq[i]] = rq[i];
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
      float pv[TP], qv[TQ];
#pragma unroll
      for (int x = 0; x < TP; ++x) pv[x] = Ps[buf][4 * s + q][wp + pidx<TP>(x, j)];
#pragma unroll
      for (int y = 0; y < TQ; ++y) qv[y] = Qs[buf][4 * s + q][wq + 16 * y + j];
#pragma unroll
      for (int x = 0; x < TP; ++x)
#pragma unroll
        for (int y = 0; y < TQ; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(pv[x], qv[y], acc[x][y], 0, 0, 0);
    }
    if (it + 1 < total) sstore(buf ^ 1);
    __syncthreads();
  }
  // epilogue: lane (j, q), reg r <-> row p0 + wp + pidx(x, 4 q) + r, column q0 + wq + 16 y + j
#pragma unroll
  for (int y = 0; y < TQ; ++y) {
    const int c = q0 + wq + 16 * y + j;
    if (c >= Q) continue;
#pragma unroll
    for (int x = 0; x < TP; ++x) {
      const int p = p0 + wp + pidx<TP>(x, 4 * q);
      if (p >= P) continue;
      if (MODE == FWD) {                      // p % 4 == 0 and N % 4 == 0: the four rows are inside together
        f32x4 v = acc[x][y];
        if (a.bias) {
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] += a.bias[p + r];
        }
        *reinterpret_cast<f32x4*>(a.out + (size_t)c * a.N + p) = v;
      } else {
        float* o = a.out + ((size_t)blockIdx.z * Q + c) * P + p;
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (p + r < P) o[r] = acc[x][y][r];
      }
    }
  }
  if (MODE == DW && want_db) {                 // (block-uniform; the loop's last barrier released Qs)
    float* sh = &Qs[0][0][0];                  // 256 floats of 2 * BK * LDQ
    sh[tid] = colsum;
    __syncthreads();
    if (tid < BQ && q0 + tid < Q) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 256 / BQ; ++k) s += sh[tid + BQ * k];
      a.dbp[(size_t)blockIdx.z * a.N + q0 + tid] = s;
    }
  }
}

// out[e] (+)= sum_s part[s][e], slices in order (fp64)
__global__ __launch_bounds__(256) void k_sum_slices(const float* __restrict__ part, int S, size_t E, float* __restrict__ out, int accumulate) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += (double)part[(size_t)k * E + e];
  out[e] = accumulate ? out[e] + (float)s : (float)s;
}

// the row tile follows L (32 / 64 / 128 latents per block) in DZ and DW
static int tp_of(int L) { return L <= 32 ? 1 : (L <= 64 ? 2 : 4); }
// DZ: 128 clips per block; the N slices depend on (N, L) only and give ~512 blocks at B = 4096
static int dz_rchunk(int N, int L) {
  const int nt = ceil_div(L, 32 * tp_of(L));
  int ks = 16 / nt;
  if (ks < 2) ks = 2;
  const int kmax = ceil_div(N, 8 * BK);            // at least eight 16-wide steps per slice
  if (ks > kmax) ks = kmax;
  if (ks < 1) ks = 1;
  return round_up(ceil_div(N, ks), BK);
}
static int dz_slices(int N, int L) { return ceil_div(N, dz_rchunk(N, L)); }
// DW: 128 columns of N per block, clip chunks to ~1024 blocks
static int dw_chunk(int B, int N, int L) {
  const int tiles = ceil_div(N, 128) * ceil_div(L, 32 * tp_of(L));
  int s = (1024 + tiles / 2) / tiles;
  if (s > 64) s = 64;
  if (s < 1) s = 1;
  return round_up(ceil_div(B, s), BK);
}
static int dw_chunks(int B, int N, int L) { return ceil_div(B, dw_chunk(B, N, L)); }

template <int MODE, int TP, int TQ>
static void launch(const Args& a, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((k_rev_wide<MODE, TP, TQ>), grid, dim3(256), 0, stream, a);
}
template <int MODE>
static void launch_by_l(const Args& a, dim3 grid, hipStream_t stream) {
  const int tp = tp_of(a.L);
  if (tp == 1) launch<MODE, 1, 4>(a, grid, stream);
  else if (tp == 2) launch<MODE, 2, 4>(a, grid, stream);
  else launch<MODE, 4, 4>(a, grid, stream);
}

static int sum_slices(const float* part, int S, size_t E, float* out, int accumulate, hipStream_t stream, const char* what) {
  hipLaunchKernelGGL(k_sum_slices, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, stream, part, S, E, out, accumulate);
  return check_launch(what);
}

}  // namespace rbw

bool wide_rev_btlnk_ok(int N, int L) { return N > 0 && N % 4 == 0 && L > 16 && L <= 512; }

size_t wide_rev_btlnk_ws_floats(int B, int N, int L) {
  if (B <= 0 || !wide_rev_btlnk_ok(N, L)) return 0;
  const size_t dz = (size_t)rbw::dz_slices(N, L) * (size_t)B * (size_t)L;
  const size_t dw = (size_t)rbw::dw_chunks(B, N, L) * ((size_t)N * (size_t)L + (size_t)N);
  return dz > dw ? dz : dw;                        // the two passes follow each other on one stream
}

int wide_rev_btlnk_fwd(const float* z, const float* W, const float* bias, float* H, int B, int N, int L, hipStream_t stream) {
  rbw::Args a{z, W, nullptr, bias, H, nullptr, B, N, L, round_up(L, rbw::BK)};
  const int tq = B <= 32 ? 1 : (B <= 64 ? 2 : 4);   // clips per block: 32 / 64 / 128
  const dim3 grid(ceil_div(N, 128), ceil_div(B, 32 * tq), 1);
  if (tq == 1) rbw::launch<rbw::FWD, 4, 1>(a, grid, stream);
  else if (tq == 2) rbw::launch<rbw::FWD, 4, 2>(a, grid, stream);
  else rbw::launch<rbw::FWD, 4, 4>(a, grid, stream);
  return check_launch("rev_btlnk_fwd (wide)");
}

int wide_rev_btlnk_bwd(const float* dH, const float* z, const float* W, float* dz, int dz_accumulate, float* dW, float* db, int accumulate,
                       float* ws, int B, int N, int L, hipStream_t stream) {
  const int tp = rbw::tp_of(L);
  int rc;
  // dz partials per slice of N, then their sum (+ the given dz)
  const int ks = rbw::dz_slices(N, L);
  rbw::Args az{z, W, dH, nullptr, ws, nullptr, B, N, L, rbw::dz_rchunk(N, L)};
  rbw::launch_by_l<rbw::DZ>(az, dim3(ceil_div(L, 32 * tp), ceil_div(B, 128), ks), stream);
  if ((rc = check_launch("rev_btlnk_dz (wide)"))) return rc;
  if ((rc = rbw::sum_slices(ws, ks, (size_t)B * L, dz, dz_accumulate, stream, "rev_btlnk_dz_sum (wide)"))) return rc;
  // dW / db partials per clip chunk, then their sums into the destinations
  const int S = rbw::dw_chunks(B, N, L);
  float* dbp = ws + (size_t)S * N * L;
  rbw::Args aw{z, W, dH, nullptr, ws, dbp, B, N, L, rbw::dw_chunk(B, N, L)};
  rbw::launch_by_l<rbw::DW>(aw, dim3(ceil_div(L, 32 * tp), ceil_div(N, 128), S), stream);
  if ((rc = check_launch("rev_btlnk_dw (wide)"))) return rc;
  if ((rc = rbw::sum_slices(ws, S, (size_t)N * L, dW, accumulate, stream, "rev_btlnk_dw_sum (wide)"))) return rc;
  if (db && (rc = rbw::sum_slices(dbp, S, (size_t)N, db, accumulate, stream, "rev_btlnk_db_sum (wide)"))) return rc;
  return COSKAD_OK;
}

}  // namespace coskad
