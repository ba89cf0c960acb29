// The ADJOINT of the folded eval layer of eval_layer_clip.hip: the gradient of anything downstream with respect to a layer's input,
// for a layer whose BatchNorm is folded (no batch coupling: a clip's gradient depends on that clip alone).
//     forward   U   = Wz . gcn(X) + Wx . X + b                        X = PReLU(in)
//     adjoint   dIn = PReLU'(in) (.) ( gcn^T(Wz^T . dU) + Wx^T . dU )
//     gcn^T(G)[t, v] = sum_t' Tm[v][t][t'] sum_w A[t'][v][w] G[t', w]  (spatial transpose FIRST, then the temporal one: the opposite
//                                                                      order to the forward, and the two do not commute)
// at 8, 12, 16 or 24 frames, 17 or 25 joints, ONE CLIP PER WORKGROUP OF FOUR WAVES on a persistent grid; only dU, `in` (for the mask)
// and dIn touch HBM.  wfold [2 Ci][Co] is what coskad_bn_fold_f32 hands the forward (rows [0, Ci) act on Z, rows [Ci, 2 Ci) on X; an
// identity residual is whatever the fold put into the X rows): it is read TRANSPOSED as the A operand, lane (j, q) of input tile `it`
// holds wfold[16 it + j][4 s + q] -- no transposed copy exists.
// Phases of a clip (16 / 32 input channels, v_mfma_f32_16x16x4_f32):
//   1. dU [Co][T V] is staged into the image (float4 loads, rows of stride T V + 2);
//   2. BOTH products read it: a wave owns an input-channel tile x a share of the position tiles and forms Gz = Wz^T dU and
//      Gx = Wx^T dU from ONE read of every B operand; both accumulator sets (2 x 4 x MAXT registers) are held;
//   3. Gz goes into the image rows [0, Ci) (dU is dead) and is mixed in place: frames dealt to the waves for the spatial transpose,
//      joints for the temporal one, K zero-padded on BOTH operands (no neighbouring frame, no neighbouring table row leaks in);
//   4. every lane adds its Gx registers to the elements it owns, and the rows leave in full 16-byte lines through the PReLU' mask.
// Two input channels (the first layer, 32 -> 2) run the same phases on the VALU: a 16-row MFMA tile would be 7/8 padding
// (last_layer.hip's reasoning for its few-channel forms); a thread owns a position through phases 2 and 4.
// No atomics, no scratch; a clip's result does not depend on the workgroup or loop round that forms it.  Resources per instantiation
// and what was decided from them: DESIGN 5.24.
#include "fused_ops.h"
#include "layer_launch.h"
#include <cstdint>

namespace coskad {
namespace eva {

using ff::f32x4;
using ff::Lane;
using ff::mfma;

constexpr int imin(int a, int b) { return a < b ? a : b; }
constexpr int imax(int a, int b) { return a > b ? a : b; }

// CT = Ci / 16 (0: the two-channel form), OT = Co / 16
template <int T, int V, int CT, int OT>
struct Geo {
  static_assert(T % 4 == 0 && T <= 32, "8 / 12 / 16 / 24 frames");
  static constexpr bool FEW = CT == 0;
  static constexpr int TV = T * V, LD = TV + 2, R4 = TV / 4, Ci = FEW ? 2 : 16 * CT, Co = 16 * OT;
  static_assert(TV % 4 == 0, "rows are staged as float4");
  static constexpr int XL = (Co * R4 + 255) / 256;                            // float4 loads of a thread's share of dU
  static constexpr int KT = T / 4, NTT = (T + 15) / 16;                       // temporal transpose: k-steps, output column tiles
  static constexpr int NTV = (V + 15) / 16, KV = (V + 3) / 4;                 // spatial transpose
  static constexpr int MAXF = T / 4, MAXJ = (V + 3) / 4;                      // a wave's frames / joints
  static constexpr int NT = (TV + 15) / 16;                                   // position tiles
  // a wave's share of a product: 32 input channels: tile wave & 1 x half of the position tiles; 16: a quarter of them
  static constexpr int SHARES = FEW ? 1 : 4 / CT;
  static constexpr int MAXT = FEW ? 0 : (NT + SHARES - 1) / SHARES;
  static constexpr int KS = Co / 4;
  static constexpr int NP = (TV + 255) / 256;                                 // (two channels) positions of a thread
  // the image: dU's Co rows, then Gz in rows [0, Ci) (two channels: Gz, its spatial transpose and the result in rows 0 .. 5 of >= 16)
  static constexpr int ROWS = imax(Co, Ci);
  static constexpr int LDS_BYTES = ROWS * LD * 4;
  static_assert(LDS_BYTES <= kMaxLdsBytes, "160 KB of LDS");
  // registers of a wave: both accumulator sets, both weight sets, a mixing step's operands and addresses (the compiler's counts run
  // 70 .. 95 above the first two terms: 24 x 25 at 32 input channels spills inside 256 and gets a CU to itself)
  static constexpr int REGS = FEW ? 96 : 8 * MAXT + 2 * KS + 100;
  static constexpr int by_reg(int regs) { return regs <= 168 ? 3 : (regs <= 256 ? 2 : 1); }
  static constexpr int BY_REG = by_reg(REGS);
  static constexpr int BY_LDS = kMaxLdsBytes / LDS_BYTES;
  // workgroups (= waves per SIMD) a CU is asked to hold: a third one was worth less than anything else in the forward
  static constexpr int PER_CU = imin(2, imin(BY_LDS, BY_REG));
  static_assert(PER_CU >= 1, "one workgroup per CU at least");
  // what rides in registers across the phases where that costs no workgroup per CU: the NEXT clip's dU rows (PF: 4 XL registers, in
  // flight from the staging of this clip to the staging of the next) and this clip's `in` rows for the mask (MPF: 4 ML registers, in
  // flight across the mixing phases); otherwise the rows are loaded where they are used
  static constexpr int ML = (Ci * R4 + 255) / 256;
  static constexpr bool PF = !FEW && XL <= 13 && imin(2, imin(BY_LDS, by_reg(REGS + 4 * XL))) >= PER_CU;
  static constexpr bool MPF = !FEW && ML <= 8 && imin(2, imin(BY_LDS, by_reg(REGS + 4 * ((PF ? XL : 0) + ML)))) >= PER_CU;
};

// four positions (e: float4 index into the clip's rows) of one row into the image
template <int R4, int LD>
__device__ __forceinline__ void stage_row(float* img, int e, float4 v) {
  const int row = e / R4, col = 4 * (e - row * R4);
  *reinterpret_cast<float2*>(img + row * LD + col) = float2{v.x, v.y};
  *reinterpret_cast<float2*>(img + row * LD + col + 2) = float2{v.z, v.w};
}

// rows [0, NROWS) of the image -> dIn rows of this clip in full lines, through PReLU'(in): 1 where in > 0, the slope elsewhere (an
// exact 0 gets the slope: oracle/ref_cpu.prelu); mask off: `in` is not read
// (HAVE: the `in` rows are in `pre`, loaded by this thread for these indices earlier in the clip)
template <int NROWS, int R4, int LD, bool HAVE = false>
__device__ __forceinline__ void flush_rows(const float* img, float* __restrict__ dIn, const float* __restrict__ in, size_t clip_off,
                                           bool mask, float a_in, int tid, const float4* pre = nullptr) {
  constexpr int n4 = NROWS * R4;
  float4* o4 = reinterpret_cast<float4*>(dIn + clip_off);
  const float4* u4 = reinterpret_cast<const float4*>(in + (mask ? clip_off : 0));
#pragma unroll
  for (int i = 0; i < (n4 + 255) / 256; ++i) {
    const int e4 = tid + 256 * i;
    if (e4 < n4) {
      const int row = e4 / R4, col = 4 * (e4 - row * R4);
      const float2 g0 = *reinterpret_cast<const float2*>(img + row * LD + col);
      const float2 g1 = *reinterpret_cast<const float2*>(img + row * LD + col + 2);
      float4 o = float4{g0.x, g0.y, g1.x, g1.y};
      if (mask) {
        float4 u;
        if constexpr (HAVE) u = pre[i];
        else u = u4[e4];
        o.x = u.x > 0.f ? o.x : a_in * o.x;
        o.y = u.y > 0.f ? o.y : a_in * o.y;
        o.z = u.z > 0.f ? o.z : a_in * o.z;
        o.w = u.w > 0.f ? o.w : a_in * o.w;
      }
      o4[e4] = o;
    }
  }
}

template <int T, int V, int CT, int OT>
__global__ __launch_bounds__(256, (Geo<T, V, CT, OT>::PER_CU)) void k_layer_input_grad(
    const float* __restrict__ dU, const float* __restrict__ in, float* __restrict__ dIn, const float* __restrict__ Aw,
    const float* __restrict__ Tw, const float* __restrict__ wfold, const float* __restrict__ in_slope, int B) {
  using G = Geo<T, V, CT, OT>;
  constexpr int TV = G::TV, LD = G::LD, R4 = G::R4, Ci = G::Ci, Co = G::Co, XL = G::XL;
  constexpr int KT = G::KT, NTT = G::NTT, NTV = G::NTV, KV = G::KV, MAXF = G::MAXF, MAXJ = G::MAXJ, NT = G::NT, MAXT = G::MAXT;
  constexpr int KS = G::KS, ML = G::ML;
  constexpr bool PF = G::PF, MPF = G::MPF;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* img = lds;                  // dU -> Gz -> its spatial transpose -> its temporal transpose (+ Gx): the flush
  const int tid0 = threadIdx.x, lane = tid0 & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid0 >> 6);
  auto geo = [&]() {
    int l = lane;
    asm volatile("" : "+v"(l));
    return Lane{l & 15, l >> 4};
  };
  auto tid_now = [&]() {
    int t = tid0;
    asm volatile("" : "+v"(t));
    return t;
  };
  Lane L = geo();
  const bool mask = in_slope != nullptr;
  const float a_in = mask ? in_slope[0] : 1.f;
  const int it = wave % CT, share = wave / CT;
  const int t0 = share * MAXT;
  const int left = NT - t0;
  const int nt = left < 0 ? 0 : (left < MAXT ? left : MAXT);      // may be 0: the wave stores nothing and keeps every barrier
  // the folded weights of this wave's input tile, TRANSPOSED, for the launch: A[i = c][k = 4 s + q] = wfold[16 it + c][4 s + q]
  float wz[KS], wx[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    wz[s] = wfold[(16 * it + L.j) * Co + 4 * s + L.q];
    wx[s] = wfold[(Ci + 16 * it + L.j) * Co + 4 * s + L.q];
  }
  const float* Ap = Aw;
  const float* Tp = Tw;
  float4 px[PF ? XL : 1];
  auto xload = [&](int c) {
    if constexpr (PF) {
      const int tid = tid_now();
      const float4* g4 = reinterpret_cast<const float4*>(dU + (size_t)(c < B ? c : 0) * Co * TV);
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int e = tid + 256 * i;
        px[i] = (e < Co * R4 && c < B) ? g4[e] : float4{0.f, 0.f, 0.f, 0.f};   // (past the batch: nothing is read)
      }
    }
  };
  xload(blockIdx.x);
  for (int clip = blockIdx.x; clip < B; clip += gridDim.x) {
    __syncthreads();                                     // the previous clip's flush is done with the image
    {
      const int tid = tid_now();
      const float4* g4 = reinterpret_cast<const float4*>(dU + (size_t)clip * Co * TV);
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int e = tid + 256 * i;
        if (e < Co * R4) {
          if constexpr (PF) stage_row<R4, LD>(img, e, px[i]);
          else stage_row<R4, LD>(img, e, g4[e]);
        }
      }
    }
    xload(clip + gridDim.x);                             // the next clip's rows: a whole clip of products and mixing to arrive
    float4 um[MPF ? ML : 1];
    if constexpr (MPF) {
      if (mask) {
        const int tid = tid_now();
        const float4* u4 = reinterpret_cast<const float4*>(in + (size_t)clip * Ci * TV);
#pragma unroll
        for (int i = 0; i < ML; ++i) {
          const int e = tid + 256 * i;
          um[i] = e < Ci * R4 ? u4[e] : float4{0.f, 0.f, 0.f, 0.f};
        }
      }
    }
    asm volatile("" : "+s"(Ap), "+s"(Tp));               // (the mixing operands are read per clip through L2, not held across clips)
    __syncthreads();                                     // the image holds dU
    L = geo();
    // ---- both products from one read of dU: G tile = sum_k W[c][k] dU[k][p] ----------------------------------------------------------
    f32x4 az[MAXT], ax[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) { az[t] = f32x4{0.f, 0.f, 0.f, 0.f}; ax[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    {
      const float* bp = lds + L.q * LD;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
          const int tile = t0 + t < NT ? t0 + t : NT - 1;             // (beyond the wave's share: clamped -- never stored)
          const int p = 16 * tile + L.j;
          const float b = bp[4 * s * LD + (p < TV ? p : TV - 1)];
          az[t] = mfma(wz[s], b, az[t]);
          ax[t] = mfma(wx[s], b, ax[t]);
        }
      }
    }
    __syncthreads();                                     // every wave has read dU
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      if (t < nt) {
        const int p = 16 * (t0 + t) + L.j;
        float* dst = img + (16 * it + 4 * L.q) * LD + (p < TV ? p : TV);   // (past the clip: the padding column)
        dst[0] = az[t][0]; dst[LD] = az[t][1]; dst[2 * LD] = az[t][2]; dst[3 * LD] = az[t][3];
      }
    }
    __syncthreads();                                     // the image holds Gz
    // ---- spatial transpose, in place: S[t, v] = sum_w G[t, w] A[t][v][w]; frames t = wave, wave + 4, ..  B[k = w][j = v] --------------
#pragma unroll
    for (int tt = 0; tt < MAXF; ++tt) {
      const int t = wave + 4 * tt;
      float bb[NTV][KV];
#pragma unroll
      for (int c = 0; c < NTV; ++c)
#pragma unroll
        for (int s = 0; s < KV; ++s)
          bb[c][s] = (16 * c + L.j < V && 4 * s + L.q < V) ? Ap[(t * V + 16 * c + L.j) * V + 4 * s + L.q] : 0.f;
#pragma unroll
      for (int rt = 0; rt < CT; ++rt) {
        float a[KV];
#pragma unroll
        for (int s = 0; s < KV; ++s) a[s] = 4 * s + L.q < V ? img[(16 * rt + L.j) * LD + t * V + 4 * s + L.q] : 0.f;
        f32x4 d[NTV];
#pragma unroll
        for (int c = 0; c < NTV; ++c) {
          d[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < KV; ++s) d[c] = mfma(a[s], bb[c][s], d[c]);
        }
#pragma unroll
        for (int c = 0; c < NTV; ++c)
          if (16 * c + L.j < V) {
#pragma unroll
            for (int r = 0; r < 4; ++r) img[(16 * rt + 4 * L.q + r) * LD + t * V + 16 * c + L.j] = d[c][r];
          }
      }
    }
    __syncthreads();
    // ---- temporal transpose, in place: D[t, v] = sum_t' S[t', v] Tm[v][t][t']; joints v = wave, wave + 4, ..  B[k = t'][j = t] --------
#pragma unroll
    for (int k = 0; k < MAXJ; ++k) {
      const int v = wave + 4 * k;
      if (v < V) {
        float tb[NTT][KT];
#pragma unroll
        for (int c = 0; c < NTT; ++c)
#pragma unroll
          for (int s = 0; s < KT; ++s) tb[c][s] = 16 * c + L.j < T ? Tp[(v * T + 16 * c + L.j) * T + 4 * s + L.q] : 0.f;
#pragma unroll
        for (int rt = 0; rt < CT; ++rt) {
          float a[KT];                                   // every read of this (row tile, joint) before either column tile is stored
#pragma unroll
          for (int s = 0; s < KT; ++s) a[s] = img[(16 * rt + L.j) * LD + (4 * s + L.q) * V + v];
          f32x4 d[NTT];
#pragma unroll
          for (int c = 0; c < NTT; ++c) {
            d[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KT; ++s) d[c] = mfma(a[s], tb[c][s], d[c]);
          }
#pragma unroll
          for (int c = 0; c < NTT; ++c)
            if (16 * c + L.j < T) {
#pragma unroll
              for (int r = 0; r < 4; ++r) img[(16 * rt + 4 * L.q + r) * LD + (16 * c + L.j) * V + v] = d[c][r];
            }
        }
      }
    }
    __syncthreads();                                     // the image holds gcn^T(Gz)
    L = geo();
    // ---- + Gx: a lane adds to the elements its accumulators own ------------------------------------------------------------------------
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
      const int p = 16 * (t0 + t) + L.j;
      if (t < nt && p < TV) {
        float* dst = img + (16 * it + 4 * L.q) * LD + p;
        dst[0] += ax[t][0]; dst[LD] += ax[t][1]; dst[2 * LD] += ax[t][2]; dst[3 * LD] += ax[t][3];
      }
    }
    __syncthreads();
    flush_rows<Ci, R4, LD, MPF>(img, dIn, in, (size_t)clip * Ci * TV, mask, a_in, tid_now(), um);
  }
}

// two input channels: wfold [4][Co] (rows Z0 Z1 X0 X1), everything on the VALU; a thread owns positions tid, tid + 256, ..
template <int T, int V, int OT>
__global__ __launch_bounds__(256, (Geo<T, V, 0, OT>::PER_CU)) void k_layer_input_grad_few(
    const float* __restrict__ dU, const float* __restrict__ in, float* __restrict__ dIn, const float* __restrict__ Aw,
    const float* __restrict__ Tw, const float* __restrict__ wfold, const float* __restrict__ in_slope, int B) {
  using G = Geo<T, V, 0, OT>;
  constexpr int TV = G::TV, LD = G::LD, R4 = G::R4, Co = G::Co, XL = G::XL, NP = G::NP;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* img = lds;
  float* gz = lds;                   // (after the products) Gz [2][LD]
  float* sp = lds + 2 * LD;          // its spatial transpose
  float* res = lds + 4 * LD;         // the result rows
  const int tid0 = threadIdx.x;
  auto tid_now = [&]() {
    int t = tid0;
    asm volatile("" : "+v"(t));
    return t;
  };
  const bool mask = in_slope != nullptr;
  const float a_in = mask ? in_slope[0] : 1.f;
  const float* Ap = Aw;
  const float* Tp = Tw;
  const float* Wp = wfold;
  for (int clip = blockIdx.x; clip < B; clip += gridDim.x) {
    __syncthreads();
    {
      const int tid = tid_now();
      const float4* g4 = reinterpret_cast<const float4*>(dU + (size_t)clip * Co * TV);
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int e = tid + 256 * i;
        if (e < Co * R4) stage_row<R4, LD>(img, e, g4[e]);
      }
    }
    // (table and weight pointers through an optimisation barrier per clip: uniform weights come through the scalar cache, a thread's
    // table values are L1 / L2 hits, neither is held across clips)
    asm volatile("" : "+s"(Ap), "+s"(Tp), "+s"(Wp));
    __syncthreads();
    const int tid = tid_now();
    float g[NP][4];                                      // Gz0 Gz1 Gx0 Gx1 of this thread's positions
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = tid + 256 * i;
      const float* col = img + (p < TV ? p : TV - 1);
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 8
      for (int k = 0; k < Co; ++k) {
        const float d = col[k * LD];
        s0 = fmaf(Wp[k], d, s0);
        s1 = fmaf(Wp[Co + k], d, s1);
        s2 = fmaf(Wp[2 * Co + k], d, s2);
        s3 = fmaf(Wp[3 * Co + k], d, s3);
      }
      g[i][0] = s0; g[i][1] = s1; g[i][2] = s2; g[i][3] = s3;
    }
    __syncthreads();                                     // every thread has read dU
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int p = tid + 256 * i;
      if (p < TV) { gz[p] = g[i][0]; gz[LD + p] = g[i][1]; }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NP; ++i) {                       // p = t * V + v:  S[r][t, v] = sum_w G[r][t, w] A[t][v][w]
      const int p = tid + 256 * i;
      if (p < TV) {
        const int t = p / V;
        const float* arow = Ap + (size_t)p * V;
        const float* grow = gz + t * V;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll 5
        for (int w = 0; w < V; ++w) {
          const float a = arow[w];
          s0 = fmaf(grow[w], a, s0);
          s1 = fmaf(grow[LD + w], a, s1);
        }
        sp[p] = s0;
        sp[LD + p] = s1;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NP; ++i) {                       // p = t * V + v:  D[r][t, v] = sum_t' S[r][t', v] Tm[v][t][t'], + Gx
      const int p = tid + 256 * i;
      if (p < TV) {
        const int t = p / V, v = p - t * V;
        const float* trow = Tp + (v * T + t) * T;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int q = 0; q < T; ++q) {
          const float w = trow[q];
          s0 = fmaf(sp[q * V + v], w, s0);
          s1 = fmaf(sp[LD + q * V + v], w, s1);
        }
        res[p] = s0 + g[i][2];
        res[LD + p] = s1 + g[i][3];
      }
    }
    __syncthreads();
    flush_rows<2, R4, LD>(res, dIn, in, (size_t)clip * 2 * TV, mask, a_in, tid_now());
  }
}

struct Args {
  const float* dU;
  const float* in;
  float* dIn;
  const float* Aw;
  const float* Tw;
  const float* wfold;
  const float* in_slope;
  int B;
  hipStream_t st;
};

template <int T_, int V_, int CT_, int OT_>
struct Tag {
  using G = Geo<T_, V_, CT_, OT_>;
  static constexpr int T = T_, V = V_, CT = CT_, OT = OT_;
};

// f(Tag<T, V, CT, OT>{}) for a shape of layer_input_grad_ok
template <int T, int V, class F>
static int with_channels(int Ci, int Co, F&& f) {
  if (Ci == 2) {
    if (Co == 16) return f(Tag<T, V, 0, 1>{});
    else if (Co == 32) return f(Tag<T, V, 0, 2>{});
    else return f(Tag<T, V, 0, 4>{});
  } else if (Ci == 16) {
    if (Co == 16) return f(Tag<T, V, 1, 1>{});
    else if (Co == 32) return f(Tag<T, V, 1, 2>{});
    else return f(Tag<T, V, 1, 4>{});
  } else {
    if (Co == 16) return f(Tag<T, V, 2, 1>{});
    else if (Co == 32) return f(Tag<T, V, 2, 2>{});
    else return f(Tag<T, V, 2, 4>{});
  }
}

template <class F>
static int with_shape(int T, int V, int Ci, int Co, F&& f) {
  if (V == 17) {
    if (T == 8) return with_channels<8, 17>(Ci, Co, f);
    else if (T == 12) return with_channels<12, 17>(Ci, Co, f);
    else if (T == 16) return with_channels<16, 17>(Ci, Co, f);
    else return with_channels<24, 17>(Ci, Co, f);
  } else {
    if (T == 8) return with_channels<8, 25>(Ci, Co, f);
    else if (T == 12) return with_channels<12, 25>(Ci, Co, f);
    else if (T == 16) return with_channels<16, 25>(Ci, Co, f);
    else return with_channels<24, 25>(Ci, Co, f);
  }
}

static bool ok(int T, int V, int Ci, int Co) {
  return (T == 8 || T == 12 || T == 16 || T == 24) && (V == 17 || V == 25) && (Ci == 2 || Ci == 16 || Ci == 32) &&
         (Co == 16 || Co == 32 || Co == 64);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace eva

extern "C" {

/* 1: coskad_layer_input_grad_f32 takes the (Ci -> Co) layer at this geometry */
int coskad_layer_input_grad_ok(int T, int V, int Ci, int Co) { return eva::ok(T, V, Ci, Co) ? 1 : 0; }

/* the persistent grid's cap (workgroups) of that shape's kernel, 0 where not ok */
int coskad_layer_input_grad_max_grid(int T, int V, int Ci, int Co) {
  if (!eva::ok(T, V, Ci, Co)) return 0;
  return eva::with_shape(T, V, Ci, Co, [](auto tag) { return 256 * decltype(tag)::G::PER_CU; });
}

int coskad_layer_input_grad_f32(const float* dU, const float* in, float* dIn, const float* A, const float* Tm, const float* wfold,
                                const float* in_slope, int B, int Ci, int Co, int T, int V, hipStream_t stream) {
  if (!dU) return fail(COSKAD_ERR_ARG, "layer_input_grad: `dU` is NULL");
  if (!dIn) return fail(COSKAD_ERR_ARG, "layer_input_grad: `dIn` is NULL");
  if (in_slope && !in) return fail(COSKAD_ERR_ARG, "layer_input_grad: `in` is NULL (the PReLU mask of `in_slope` reads it)");
  if (!eva::aligned16(dU)) return fail(COSKAD_ERR_ARG, "layer_input_grad: `dU` (%p) must be 16-byte aligned", (const void*)dU);
  if (in_slope && !eva::aligned16(in)) return fail(COSKAD_ERR_ARG, "layer_input_grad: `in` (%p) must be 16-byte aligned", (const void*)in);
  if (!eva::aligned16(dIn)) return fail(COSKAD_ERR_ARG, "layer_input_grad: `dIn` (%p) must be 16-byte aligned", (const void*)dIn);
  if (!A || !Tm || !wfold) return fail(COSKAD_ERR_ARG, "layer_input_grad: null pointer (A, Tm or wfold)");
  if (B <= 0) return fail(COSKAD_ERR_ARG, "layer_input_grad: B=%d", B);
  if (!eva::ok(T, V, Ci, Co))
    return fail(COSKAD_ERR_SHAPE, "layer_input_grad: unsupported (T=%d, V=%d, Ci=%d, Co=%d): built for 8 / 12 / 16 / 24 x 17 / 25, "
                "2 / 16 / 32 -> 16 / 32 / 64 channels", T, V, Ci, Co);
  const eva::Args a{dU, in, dIn, A, Tm, wfold, in_slope, B, stream};
  return eva::with_shape(T, V, Ci, Co, [&](auto tag) {
    using Tg = decltype(tag);
    using G = typename Tg::G;
    const int cap = 256 * G::PER_CU;                     // the persistent grid: PER_CU workgroups on each of 256 CUs
    const int grid = a.B < cap ? a.B : cap;
    if constexpr (G::FEW)
      return launch_lds<eva::k_layer_input_grad_few<Tg::T, Tg::V, Tg::OT>>("layer_input_grad", dim3(grid), dim3(256), G::LDS_BYTES, a.st,
                                                                          a.dU, a.in, a.dIn, a.Aw, a.Tw, a.wfold, a.in_slope, a.B);
    else
      return launch_lds<eva::k_layer_input_grad<Tg::T, Tg::V, Tg::CT, Tg::OT>>("layer_input_grad", dim3(grid), dim3(256), G::LDS_BYTES,
                                                                              a.st, a.dU, a.in, a.dIn, a.Aw, a.Tw, a.wfold, a.in_slope,
                                                                              a.B);
  });
}

}  // extern "C"

}  // namespace coskad
