// One ST_GCNN layer with BatchNorm folded (eval mode, or any caller that hands over folded weights; reference
// models/graph_layers/stsgcn.py:56-80 the mixing, 94-116 the layer):
//     U = Wz . gcn(X) + Wx . X + b          X = PReLU(in) (in_slope), optional PReLU on the way out (out_slope)
// at 8, 12, 16 or 24 frames, 17 or 25 joints, ONE CLIP PER WORKGROUP OF FOUR WAVES, nothing but the layer's input and output in HBM;
// and its FIRST form (the network input [B, 2, T, V] -> layer 1 on the VALU -> PReLU -> this layer: the first layer's kernel, its
// 32-row write and this kernel's 32-row read gone).
// The mixes are dealt by joint and by frame, as in fwd_moments_bpc.hip, so that a wave's operands of both are the same for every clip.
// ONE image: the residual convolution Wx . X runs first, straight from the staged rows (B operands read from the image, the folded
// weights as A operands held in registers for the launch; a wave owns output tiles x position tiles), its sums wait in registers while
// the image is mixed in place into Z, then Wz . Z is added; the sums leave through the image in full lines.  (Measurements at 12
// frames against the LDS-table kernel k_layer_apply_m and against two layers in one kernel: DESIGN 5.10.)  With the frame count:
//   * the temporal mix has T / 4 k-steps and, at T = 24, two output column tiles (frames 0..15, 16..23): a wave reads every A operand
//     of a (row tile, joint), forms both tiles and only then stores either (at T = 8 / 12 the B operand's columns T..15 are zero and
//     never stored);
//   * the spatial mix pads K = V to a multiple of 4 with zeros on BOTH operands, so no neighbouring frame leaks in;
//   * a wave's share of the position tiles can be EMPTY (16 output channels at 8 x 17: 9 tiles, 3 per wave): it still walks every
//     phase and barrier, reads clamped columns and stores nothing;
//   * Geo<> decides per instantiation what stays in registers for the launch -- the mixing operands (HOLD; else read per clip
//     through L2: up to 120 / 168 registers at T = 24) and the next clip's rows (PF; else this clip's rows go straight into the
//     image) -- and whether 64 output channels leave through 64 rows at once or through the 32 input rows in two rounds (TWO), so
//     that a CU holds two workgroups wherever anything allows it (PER_CU: launch bounds and the persistent grid); at T = 12
//     everything fits and is kept, and PER_CU is what was measured there;
//   * FIRST keeps x, Y0, Z0 behind the 32 input rows of the image (rows 32..37), so 2 -> 32 -> 64 at 24 x 25 stays inside 160 KB.
// No atomics; a clip's output does not depend on the workgroup or loop round that forms it.
#include "fused_ops.h"
#include "layer_launch.h"
#include <cstdint>

namespace coskad {
namespace evc {

using ff::f32x4;
using ff::Lane;
using ff::mfma;
using ff::prelu;

// the first layer (2 -> 32, folded) of the FIRST form: mixing parameters, folded weights [4][32] (rows Z0 Z1 X0 X1), bias [32]; the
// PReLU between the layers is the main kernel's `in_slope`
struct FirstLayer {
  const float* A;
  const float* T;
  const float* wfold;
  const float* bias;
};

constexpr int imin(int a, int b) { return a < b ? a : b; }

template <int T, int V, int CT, int OT, bool FIRST>
struct Geo {
  static_assert(T % 4 == 0 && T <= 32, "8 / 12 / 16 / 24 frames");
  static_assert(!FIRST || CT == 2, "the first layer has 32 output channels");
  static constexpr int TV = T * V, LD = TV + 2, R4 = TV / 4, Ci = 16 * CT, Co = 16 * OT;
  static_assert(TV % 4 == 0, "rows are staged as float4");
  static constexpr int N4 = (FIRST ? 2 : Ci) * R4, XL = (N4 + 255) / 256;
  static constexpr int KT = T / 4, NTT = (T + 15) / 16;                       // temporal mix: k-steps, output column tiles
  static constexpr int NTV = (V + 15) / 16, KV = (V + 3) / 4;                 // spatial mix: output column tiles, k-steps
  static constexpr int MAXF = T / 4, MAXJ = (V + 3) / 4;                      // a wave's frames / joints
  static constexpr int NT = (TV + 15) / 16;                                   // position tiles
  // a wave's share of the output: 64 channels: its own tile x all position tiles; 32: tile wave & 1 x half of them; 16: a quarter
  static constexpr int MAXT = OT == 4 ? NT : (OT == 2 ? (NT + 1) / 2 : (NT + 3) / 4);
  static constexpr int KS = Ci / 4;
  static constexpr int OPS = MAXJ * KT * NTT + MAXF * NTV * KV;               // registers of a wave's mixing operands
  static constexpr int STATIC_BYTES = FIRST ? 640 : 0;
  // registers of a wave with / without the mixing operands held for the launch (hold) and the next clip's rows in flight (pf; with 64
  // output channels they meet the whole accumulator and the flush) -> workgroups (= waves per SIMD) a CU can hold
  static constexpr int regs(bool hold, bool pf) {
    return 4 * MAXT + (hold ? OPS : 0) + (pf ? 4 * XL : 0) + 2 * KS + 48 + (OT == 4 ? 16 : 0);
  }
  static constexpr int by_reg(bool hold, bool pf) { return regs(hold, pf) <= 168 ? 3 : (regs(hold, pf) <= 256 ? 2 : 1); }
  static constexpr int by_lds(int rows) { return kMaxLdsBytes / (rows * LD * 4 + STATIC_BYTES); }
  // What is worth a workgroup per CU (measured): a second one is worth more than held operands or rows in flight; a
  // third one is worth less than either.  So, on the 32 input rows: the rows are prefetched, and then the operands held (in VGPRs
  // only), where that leaves two workgroups per CU if anything does.
  static constexpr int IN_ROWS = FIRST ? 38 : 32;                             // (FIRST: x, Y0, Z0 in rows 32..37)
  static constexpr int per_cu_in(bool hold, bool pf) { return imin(3, imin(by_lds(IN_ROWS), by_reg(hold, pf))); }
  static constexpr int TARGET = imin(2, per_cu_in(false, false));
  // T = 12 was measured on its own, before this rule: rows prefetched, operands held (63 registers), 64 output channels
  // through 64 rows, and three workgroups per CU asked for except at 64 output channels and at 32 -> 32 (the estimate regs() would
  // ask for 3 / 3 / 2 / 2 at 17 x 32 -> 32, 17 x 2 -> 32 -> 32, 25 x 16 -> 32, 25 x 32 -> 16 and drop the held operands at 25 x 32 -> 64)
  static constexpr bool T12 = T == 12;
  static constexpr bool PF = T12 || FIRST || (XL <= 13 && per_cu_in(false, true) >= TARGET);
  static constexpr bool HOLD = T12 || (regs(true, PF) <= 256 && per_cu_in(true, PF) >= TARGET);
  // 64 output channels leave through 64 rows at once, or -- where those rows would cost a workgroup per CU -- through the 32 input
  // rows in two rounds (waves 0, 1 then waves 2, 3)
  static constexpr bool TWO = !T12 && OT == 4 && imin(3, by_lds(64)) < per_cu_in(HOLD, PF);
  static constexpr int ROWS = (OT == 4 && !TWO) ? 64 : IN_ROWS;
  static constexpr int FR = TWO ? 32 : Co, NR = Co / FR;                      // rows per flush round, rounds
  static constexpr int LDS_BYTES = ROWS * LD * 4;
  static_assert(LDS_BYTES + STATIC_BYTES <= kMaxLdsBytes, "160 KB of LDS");
  static constexpr int BY_LDS = by_lds(ROWS);
  static constexpr int BY_REG = by_reg(HOLD, PF);
  // workgroups (= waves per SIMD) a CU is asked to hold
  static constexpr int PER_CU = T12 ? ((OT == 4 || (CT == 2 && OT == 2)) ? 2 : 3) : imin(3, imin(BY_LDS, BY_REG));
};

// the 12-frame choices, for both V and all nine (CT, OT, FIRST): grid, block and dynamic LDS follow from them
template <int V, int CT, int OT, bool FIRST>
constexpr bool geo12_pinned() {
  using G = Geo<12, V, CT, OT, FIRST>;
  return G::PER_CU == ((OT == 4 || (CT == 2 && OT == 2)) ? 2 : 3) && G::HOLD && G::PF && !G::TWO &&
         G::ROWS == (OT == 4 ? 64 : (FIRST ? 38 : 32));
}
template <int V>
constexpr bool geo12_pinned_v() {
  return geo12_pinned<V, 1, 1, false>() && geo12_pinned<V, 1, 2, false>() && geo12_pinned<V, 1, 4, false>() &&
         geo12_pinned<V, 2, 1, false>() && geo12_pinned<V, 2, 2, false>() && geo12_pinned<V, 2, 4, false>() &&
         geo12_pinned<V, 2, 1, true>() && geo12_pinned<V, 2, 2, true>() && geo12_pinned<V, 2, 4, true>();
}
static_assert(geo12_pinned_v<17>() && geo12_pinned_v<25>(), "Geo<12, ..>: the measured 12-frame choices");

// four positions (e: float4 index into the clip's rows) of one input row into the image
template <int R4, int LD>
__device__ __forceinline__ void stage_row(float* imz, bool pre, float a_in, int e, float4 v) {
  const int row = e / R4, col = 4 * (e - row * R4);
  if (pre) { v.x = prelu(v.x, a_in); v.y = prelu(v.y, a_in); v.z = prelu(v.z, a_in); v.w = prelu(v.w, a_in); }
  *reinterpret_cast<float2*>(imz + row * LD + col) = float2{v.x, v.y};
  *reinterpret_cast<float2*>(imz + row * LD + col + 2) = float2{v.z, v.w};
}

template <int T, int V, int CT, int OT, bool FIRST>
__global__ __launch_bounds__(256, (Geo<T, V, CT, OT, FIRST>::PER_CU)) void k_eval_layer_clip(
    const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ Aw, const float* __restrict__ Tw,
    const float* __restrict__ wfold, const float* __restrict__ bias, const float* __restrict__ in_slope,
    const float* __restrict__ out_slope, int B, FirstLayer fl) {
  using G = Geo<T, V, CT, OT, FIRST>;
  constexpr int TV = G::TV, LD = G::LD, R4 = G::R4, Ci = G::Ci, Co = G::Co, N4 = G::N4, XL = G::XL;
  constexpr int KT = G::KT, NTT = G::NTT, NTV = G::NTV, KV = G::KV, MAXF = G::MAXF, MAXJ = G::MAXJ, NT = G::NT, MAXT = G::MAXT;
  constexpr int KS = G::KS;
  constexpr bool HOLD = G::HOLD, PF = G::PF;
  constexpr int FR = G::FR, NR = G::NR;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* imz = lds;                  // X -> Y -> Z (mixed in place); then the flush
  float* fx = lds + 32 * LD;         // (FIRST) x [2][LD], its temporal mix, its spatial mix
  float* fy = fx + 2 * LD;
  float* fz = fy + 2 * LD;
  __shared__ float fw[FIRST ? 160 : 1];   // (FIRST) W1 | b1
  if constexpr (FIRST) {
    if (threadIdx.x < 160) fw[threadIdx.x] = threadIdx.x < 128 ? fl.wfold[threadIdx.x] : fl.bias[threadIdx.x - 128];
  }
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
  const bool pre = in_slope != nullptr, post = out_slope != nullptr;
  const float a_in = pre ? in_slope[0] : 0.f, a_out = post ? out_slope[0] : 0.f;
  // a wave's joints and frames are the same for every clip: B operands of both mixes
  //   temporal  Y[q,v] = sum_t X[t,v] T[v][t][q]:   B[k = t][j = q];   spatial  Z[t,w] = sum_v Y[t,v] A[t][v][w]:   B[k = v][j = w]
  auto tb_load = [&](const float* Tp, int v, int c, int s) {
    return (v < V && 16 * c + L.j < T) ? Tp[(v * T + 4 * s + L.q) * T + 16 * c + L.j] : 0.f;
  };
  auto bb_load = [&](const float* Ap, int t, int c, int s) {
    return (16 * c + L.j < V && 4 * s + L.q < V) ? Ap[(t * V + 4 * s + L.q) * V + 16 * c + L.j] : 0.f;
  };
  float tbv[HOLD ? MAXJ : 1][NTT][KT], bbv[HOLD ? MAXF : 1][NTV][KV];
  if constexpr (HOLD) {
#pragma unroll
    for (int k = 0; k < MAXJ; ++k)
#pragma unroll
      for (int c = 0; c < NTT; ++c)
#pragma unroll
        for (int s = 0; s < KT; ++s) tbv[k][c][s] = tb_load(Tw, wave + 4 * k, c, s);
#pragma unroll
    for (int tt = 0; tt < MAXF; ++tt)
#pragma unroll
      for (int c = 0; c < NTV; ++c)
#pragma unroll
        for (int s = 0; s < KV; ++s) bbv[tt][c][s] = bb_load(Aw, wave + 4 * tt, c, s);
  }
  const int ot = OT == 4 ? wave : (OT == 2 ? (wave & 1) : 0);
  const int t0 = OT == 4 ? 0 : (OT == 2 ? (wave >> 1) * MAXT : wave * MAXT);
  const int left = NT - t0;
  const int nt = left < 0 ? 0 : (left < MAXT ? left : MAXT);      // may be 0: the wave stores nothing and keeps every barrier
  // the folded weights of this wave's output tile, for the launch: A[i = o][k = 4 s + q] = wfold[k][16 ot + o]; rows [0, Ci) act on Z,
  // rows [Ci, 2 Ci) on X
  float wz[KS], wx[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    wz[s] = wfold[(4 * s + L.q) * Co + 16 * ot + L.j];
    wx[s] = wfold[(Ci + 4 * s + L.q) * Co + 16 * ot + L.j];
  }
  float4 px[PF ? XL : 1];
  auto xload = [&](int clip) {
    if constexpr (PF) {
      const int tid = tid_now();
      const float4* g4 = reinterpret_cast<const float4*>(in + (size_t)(clip < B ? clip : 0) * (FIRST ? 2 : Ci) * TV);
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int e = tid + 256 * i;
        px[i] = (e < N4 && clip < B) ? g4[e] : float4{0.f, 0.f, 0.f, 0.f};   // (past the batch: nothing is read)
      }
    }
  };
  // (the window lengths stage through a by-reference lambda, T = 12 calls stage_row itself: each as it was measured.  The lambda costs
  // the mixes of a 12-frame clip 26 .. 41 VALU instructions of LDS address arithmetic, 0.5 - 1.4 % of a launch: DESIGN 5.10)
  auto stage = [&](int e, float4 v) { stage_row<R4, LD>(imz, pre, a_in, e, v); };
  const float* Ap = Aw;
  const float* Tp = Tw;
  int clip = blockIdx.x;
  xload(clip);
  for (; clip < B; clip += gridDim.x) {
    __syncthreads();                                     // the previous clip's flush is done with the image
    if constexpr (FIRST) {
      // ---- the first layer on the VALU: x -> Y0 (temporal) -> Z0 (spatial) -> X = PReLU(W1 [Z0; x] + b1) into the image ---------------
      const int tid = tid_now();
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int e = tid + 256 * i;
        if (e < N4) {
          const int row = e / R4, col = 4 * (e - row * R4);
          const float4 v = px[i];
          *reinterpret_cast<float2*>(fx + row * LD + col) = float2{v.x, v.y};
          *reinterpret_cast<float2*>(fx + row * LD + col + 2) = float2{v.z, v.w};
        }
      }
      xload(clip + gridDim.x);
      // (the table pointers through an optimisation barrier per clip: a thread's table values are L1 hits, not held registers)
      const float* A1 = fl.A;
      const float* T1 = fl.T;
      asm volatile("" : "+s"(A1), "+s"(T1));
      __syncthreads();
      for (int idx = tid; idx < TV; idx += 256) {        // idx = v * T + q:  Y0[r][q, v] = sum_t x[r][t, v] T1[v][t][q]
        const int v = idx / T, q = idx - v * T;
        float y0 = 0.f, y1 = 0.f;
#pragma unroll
        for (int t = 0; t < T; ++t) {
          const float w = T1[(v * T + t) * T + q];
          y0 = fmaf(fx[t * V + v], w, y0);
          y1 = fmaf(fx[LD + t * V + v], w, y1);
        }
        fy[q * V + v] = y0;
        fy[LD + q * V + v] = y1;
      }
      __syncthreads();
      for (int idx = tid; idx < TV; idx += 256) {        // idx = t * V + w:   Z0[r][t, w] = sum_v Y0[r][t, v] A1[t][v][w]
        const int t = idx / V, w = idx - t * V;
        float z0 = 0.f, z1 = 0.f;
#pragma unroll 5
        for (int v = 0; v < V; ++v) {
          const float a = A1[(t * V + v) * V + w];
          z0 = fmaf(fy[t * V + v], a, z0);
          z1 = fmaf(fy[LD + t * V + v], a, z1);
        }
        fz[idx] = z0;
        fz[LD + idx] = z1;
      }
      __syncthreads();
      // thread <-> (channel, four positions): full 16-byte rows of the image
      for (int e = tid; e < 32 * R4; e += 256) {
        const int o = e / R4, col = 4 * (e - o * R4);
        const float w0 = fw[o], w1 = fw[32 + o], w2 = fw[64 + o], w3 = fw[96 + o], bb = fw[128 + o];
        float u[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          // (bias added to the finished sum, as the first layer's own kernels do)
          float s = w0 * fz[col + c];
          s = fmaf(w1, fz[LD + col + c], s);
          s = fmaf(w2, fx[col + c], s);
          s = fmaf(w3, fx[LD + col + c], s);
          s += bb;
          u[c] = pre ? prelu(s, a_in) : s;
        }
        *reinterpret_cast<float2*>(imz + o * LD + col) = float2{u[0], u[1]};
        *reinterpret_cast<float2*>(imz + o * LD + col + 2) = float2{u[2], u[3]};
      }
    } else if constexpr (PF) {
      const int tid = tid_now();
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int e = tid + 256 * i;
        if (e < N4) {
          if constexpr (T == 12) stage_row<R4, LD>(imz, pre, a_in, e, px[i]);
          else stage(e, px[i]);
        }
      }
    } else {
      // (the big clips: no registers for the next clip's rows across the phases -- this clip's rows, straight into the image)
      const int tid = tid_now();
      const float4* g4 = reinterpret_cast<const float4*>(in + (size_t)clip * Ci * TV);
#pragma unroll
      for (int i = 0; i < XL; ++i) {
        const int e = tid + 256 * i;
        if (e < N4) stage(e, g4[e]);
      }
    }
    if constexpr (OT < 4 && !FIRST) xload(clip + gridDim.x);       // the next clip's rows: a whole clip of products to arrive
    if constexpr (!HOLD) asm volatile("" : "+s"(Ap), "+s"(Tp));    // (the mixing operands are read per clip, not held across clips)
    __syncthreads();                                     // the image holds X
    L = geo();
    // ---- residual convolution: U tile = sum_k Wx[k][o] X[k][p], in registers while the image is mixed --------------------------------
    f32x4 acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto product = [&](const float (&w)[KS]) {
      const float* bp = lds + L.q * LD;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
          const int tile = t0 + t < NT ? t0 + t : NT - 1;             // (beyond the wave's share: clamped -- never stored)
          const int p = 16 * tile + L.j;
          acc[t] = mfma(w[s], bp[4 * s * LD + (p < TV ? p : TV - 1)], acc[t]);
        }
      }
    };
    product(wx);
    __syncthreads();                                     // every wave has read X
    // ---- Y = temporal mix, in place: joints v = wave, wave + 4, .. ---------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < MAXJ; ++k) {
      const int v = wave + 4 * k;
      if (v < V) {
        float tb[NTT][KT];
#pragma unroll
        for (int c = 0; c < NTT; ++c)
#pragma unroll
          for (int s = 0; s < KT; ++s) {
            if constexpr (HOLD) tb[c][s] = tbv[k][c][s];
            else tb[c][s] = tb_load(Tp, v, c, s);
          }
#pragma unroll
        for (int rt = 0; rt < CT; ++rt) {
          float a[KT];                                   // every read of this (row tile, joint) before either column tile is stored
#pragma unroll
          for (int s = 0; s < KT; ++s) a[s] = imz[(16 * rt + L.j) * LD + (4 * s + L.q) * V + v];
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
              for (int r = 0; r < 4; ++r) imz[(16 * rt + 4 * L.q + r) * LD + (16 * c + L.j) * V + v] = d[c][r];
            }
        }
      }
    }
    __syncthreads();
    // ---- Z = spatial mix, in place: frames t = wave, wave + 4, .. (T is a multiple of 4: every wave has T / 4 of them) ----------------
#pragma unroll
    for (int tt = 0; tt < MAXF; ++tt) {
      const int t = wave + 4 * tt;
      float bb[NTV][KV];
#pragma unroll
      for (int c = 0; c < NTV; ++c)
#pragma unroll
        for (int s = 0; s < KV; ++s) {
          if constexpr (HOLD) bb[c][s] = bbv[tt][c][s];
          else bb[c][s] = bb_load(Ap, t, c, s);
        }
#pragma unroll
      for (int rt = 0; rt < CT; ++rt) {
        float a[KV];
#pragma unroll
        for (int s = 0; s < KV; ++s) a[s] = 4 * s + L.q < V ? imz[(16 * rt + L.j) * LD + t * V + 4 * s + L.q] : 0.f;
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
            for (int r = 0; r < 4; ++r) imz[(16 * rt + 4 * L.q + r) * LD + t * V + 16 * c + L.j] = d[c][r];
          }
      }
    }
    __syncthreads();                                     // the image holds Z
    L = geo();
    if constexpr (OT == 4 && !FIRST) xload(clip + gridDim.x);      // (64 output channels: no registers for them through the mixing phases)
    product(wz);
    const float* bo = bias + 16 * ot + 4 * L.q;          // (scalar loads: only `in` and `out` are asked to be 16-byte aligned)
    const f32x4 bq = {bo[0], bo[1], bo[2], bo[3]};
    // ---- flush through the image (FR rows a round), full lines to HBM ---------------------------------------------------------------
#pragma unroll
    for (int rnd = 0; rnd < NR; ++rnd) {
      __syncthreads();                                   // the product's readers / the previous round's rows are done with the image
      if (NR == 1 || (16 * ot) / FR == rnd) {
        const int row0 = 16 * ot - FR * rnd;
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
          const int p = 16 * (t0 + t) + L.j;
          if (t < nt) {
            f32x4 v = acc[t] + bq;
            if (post) { v[0] = prelu(v[0], a_out); v[1] = prelu(v[1], a_out); v[2] = prelu(v[2], a_out); v[3] = prelu(v[3], a_out); }
            float* dst = lds + (row0 + 4 * L.q) * LD + (p < TV ? p : TV);   // (past the clip: the padding column)
            dst[0] = v[0]; dst[LD] = v[1]; dst[2 * LD] = v[2]; dst[3 * LD] = v[3];
          }
        }
      }
      __syncthreads();
      constexpr int n4 = FR * R4;
      const int tid = tid_now();
      float4* g4 = reinterpret_cast<float4*>(out + ((size_t)clip * Co + FR * rnd) * TV);
#pragma unroll
      for (int i = 0; i < (n4 + 255) / 256; ++i) {
        const int e4 = tid + 256 * i;
        if (e4 < n4) {
          const int row = e4 / R4, col = 4 * (e4 - row * R4);
          const float2 g0 = *reinterpret_cast<const float2*>(lds + row * LD + col);
          const float2 g1 = *reinterpret_cast<const float2*>(lds + row * LD + col + 2);
          g4[e4] = float4{g0.x, g0.y, g1.x, g1.y};
        }
      }
    }
  }
}

struct Args {
  const float* in;
  float* out;
  const float* Aw;
  const float* Tw;
  const float* wfold;
  const float* bias;
  const float* in_slope;
  const float* out_slope;
  int B;
  FirstLayer fl;
  hipStream_t st;
  const char* what;   // names the launch in an error text
};

template <int T, int V, int CT, int OT, bool FIRST>
static int launch_one(const Args& a) {
  using G = Geo<T, V, CT, OT, FIRST>;
  const int cap = 256 * G::PER_CU;                       // the persistent grid: PER_CU workgroups on each of 256 CUs
  const int grid = a.B < cap ? a.B : cap;
  ProbeScope probe(KID_LAYER_APPLY, FIRST ? 2 : G::Ci, G::Co, a.st);
  return launch_lds<k_eval_layer_clip<T, V, CT, OT, FIRST>>(a.what, dim3(grid), dim3(256), G::LDS_BYTES, a.st, a.in, a.out, a.Aw, a.Tw,
                                                            a.wfold, a.bias, a.in_slope, a.out_slope, a.B, a.fl);
}

template <int T, int V>
static int launch_tv(const Args& a, int Ci, int Co, bool first) {
  if (first) {
    if (Co == 16) return launch_one<T, V, 2, 1, true>(a);
    else if (Co == 32) return launch_one<T, V, 2, 2, true>(a);
    else return launch_one<T, V, 2, 4, true>(a);
  } else if (Ci == 16) {
    if (Co == 16) return launch_one<T, V, 1, 1, false>(a);
    else if (Co == 32) return launch_one<T, V, 1, 2, false>(a);
    else return launch_one<T, V, 1, 4, false>(a);
  } else {
    if (Co == 16) return launch_one<T, V, 2, 1, false>(a);
    else if (Co == 32) return launch_one<T, V, 2, 2, false>(a);
    else return launch_one<T, V, 2, 4, false>(a);
  }
}

static int launch_any(const Args& a, int T, int V, int Ci, int Co, bool first) {
  if (V == 17) {
    if (T == 8) return launch_tv<8, 17>(a, Ci, Co, first);
    else if (T == 12) return launch_tv<12, 17>(a, Ci, Co, first);
    else if (T == 16) return launch_tv<16, 17>(a, Ci, Co, first);
    else return launch_tv<24, 17>(a, Ci, Co, first);
  } else {
    if (T == 8) return launch_tv<8, 25>(a, Ci, Co, first);
    else if (T == 12) return launch_tv<12, 25>(a, Ci, Co, first);
    else if (T == 16) return launch_tv<16, 25>(a, Ci, Co, first);
    else return launch_tv<24, 25>(a, Ci, Co, first);
  }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace evc

// every (T, V) of 8 / 12 / 16 / 24 x 17 / 25 builds without scratch inside 160 KB for every channel pair: none is declined
static bool clip_geometry(int T_, int V_) { return (T_ == 8 || T_ == 12 || T_ == 16 || T_ == 24) && (V_ == 17 || V_ == 25); }

bool eval_layer_clip_ok(int T_, int V_, int Ci, int Co) {
  return clip_geometry(T_, V_) && (Ci == 16 || Ci == 32) && (Co == 16 || Co == 32 || Co == 64);
}

bool eval_first_pair_clip_ok(int T_, int V_, int Ci, int Cm, int Co) {
  return clip_geometry(T_, V_) && Ci == 2 && Cm == 32 && (Co == 16 || Co == 32 || Co == 64);
}

// (16-byte alignment of the clip tensors is asked for at the window lengths 8 / 16 / 24 only: the 12-frame callers never had to)
int launch_eval_layer_clip(const float* in, float* out, const float* Aw, const float* Tw, const float* wfold, const float* bias,
                           const float* in_slope, const float* out_slope, int B, int Ci, int Co, int T_, int V_, hipStream_t st) {
  if (!eval_layer_clip_ok(T_, V_, Ci, Co))
    return fail(COSKAD_ERR_SHAPE, "eval_layer_clip: built for 8 / 12 / 16 / 24 x 17 / 25, 16 / 32 -> 16 / 32 / 64 channels");
  if (T_ != 12) {
    if (!evc::aligned16(in)) return fail(COSKAD_ERR_ARG, "layer_apply: `in` (%p) must be 16-byte aligned at window lengths 8 / 16 / 24", (const void*)in);
    if (!evc::aligned16(out)) return fail(COSKAD_ERR_ARG, "layer_apply: `out` (%p) must be 16-byte aligned at window lengths 8 / 16 / 24", (const void*)out);
  }
  return evc::launch_any(evc::Args{in, out, Aw, Tw, wfold, bias, in_slope, out_slope, B, evc::FirstLayer{}, st, "eval_layer_clip"}, T_, V_,
                         Ci, Co, false);
}

int launch_eval_first_pair_clip(const float* x, float* out, const float* A1, const float* T1, const float* wfold1,
                                const float* bias1, const float* A2, const float* T2, const float* wfold2, const float* bias2,
                                const float* mid_slope, const float* out_slope, int B, int Co, int T_, int V_, hipStream_t st) {
  if (!eval_first_pair_clip_ok(T_, V_, 2, 32, Co))
    return fail(COSKAD_ERR_SHAPE, "eval_first_pair_clip: built for 8 / 12 / 16 / 24 x 17 / 25, 2 -> 32 -> 16 / 32 / 64 channels");
  if (T_ != 12) {
    if (!evc::aligned16(x)) return fail(COSKAD_ERR_ARG, "layer_first_pair_apply: `x` (%p) must be 16-byte aligned at window lengths 8 / 16 / 24", (const void*)x);
    if (!evc::aligned16(out))
      return fail(COSKAD_ERR_ARG, "layer_first_pair_apply: `out` (%p) must be 16-byte aligned at window lengths 8 / 16 / 24", (const void*)out);
  }
  return evc::launch_any(evc::Args{x, out, A2, T2, wfold2, bias2, mid_slope, out_slope, B, evc::FirstLayer{A1, T1, wfold1, bias1}, st,
                                   "eval_first_pair_clip"}, T_, V_, 32, Co, true);
}

extern "C" {

/* 1: coskad_layer_apply_f32 runs the layer as ONE launch (folded BatchNorm, one clip per workgroup) at this window length other than
 * 12; 0 at T = 12 (which coskad_layer_fits describes, though the same kernel serves it) and everywhere else */
int coskad_layer_apply_window_ok(int T, int V, int Ci, int Co) { return (T != 12 && eval_layer_clip_ok(T, V, Ci, Co)) ? 1 : 0; }

/* 1: coskad_layer_first_pair_apply_f32 takes the first layer (Ci = 2 -> Cm) with the layer behind it (Cm -> Co) on this layout */
int coskad_layer_first_pair_ok(int T, int V, int Ci, int Cm, int Co) { return eval_first_pair_clip_ok(T, V, Ci, Cm, Co) ? 1 : 0; }

/* The first two ST_GCNN layers of the encoder with folded BatchNorm (models/common/components.py:94-105 -> models/graph_layers/
 * stsgcn.py:94-116 twice, eval mode) in ONE pass: out [B, Co, T, V] = layer2(PReLU_mid(layer1(x))), x [B, 2, T, V] the network input; the
 * 32-channel activation between them never reaches HBM.  wfold1 [4, 32] / bias1 [32], wfold2 [64, Co] / bias2 from coskad_bn_fold_f32;
 * out_slope may be NULL (pre-activation output). */
int coskad_layer_first_pair_apply_f32(const float* x, float* out, const float* A1, const float* T1, const float* wfold1, const float* bias1,
                                      const float* A2, const float* T2, const float* wfold2, const float* bias2, const float* mid_slope,
                                      const float* out_slope, int B, int Cm, int Co, int T, int V, hipStream_t stream) {
  if (!x || !out || !A1 || !T1 || !wfold1 || !bias1 || !A2 || !T2 || !wfold2 || !bias2 || !mid_slope)
    return fail(COSKAD_ERR_ARG, "layer_first_pair_apply: null pointer");
  if (B <= 0 || !eval_first_pair_clip_ok(T, V, 2, Cm, Co))
    return fail(COSKAD_ERR_SHAPE, "layer_first_pair_apply: built for 8 / 12 / 16 / 24 x 17 / 25, 2 -> 32 -> 16 / 32 / 64 channels");
  return launch_eval_first_pair_clip(x, out, A1, T1, wfold1, bias1, A2, T2, wfold2, bias2, mid_slope, out_slope, B, Co, T, V, stream);
}

}  // extern "C"

}  // namespace coskad
