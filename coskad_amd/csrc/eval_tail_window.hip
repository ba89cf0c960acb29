// The TAIL of a decoder in eval mode: one ST_GCNN layer with BatchNorm folded and TWO output channels (coskad_layer_apply_f32's
// contract: U = Wz . gcn(X) + Wx . X + b, X = PReLU_in(in), x_rec = PReLU_out(U)) behind 16 or 32 input channels, at 8 / 12 / 16 / 24
// frames x 17 / 25 joints, ONE CLIP PER WORKGROUP on a persistent grid -- and, in the same launch, the clip's reconstruction error
//     score[n] = mean over (c, t, v) of (x_rec[n] - x[n])^2,
// so that scoring a window never writes a reconstruction.
// The mixing acts per channel on (frame, joint), a 1x1 convolution mixes channels at one position: they commute, Wz gcn(X) = gcn(Wz X)
// (last_layer.hip is the training-side sibling).  So the wide input is read ONCE, straight from global memory as 16-byte vectors with
// the PReLU applied on load, into four products per position -- Y = Wz X and R = Wx X + b, two rows each -- and everything behind that
// is 2-channel work on the VALU:
//   * products: thread <-> (channel group, four consecutive positions).  A clip has T V / 4 = 34 .. 150 vectors for 256 threads, so the
//     input channels are split over NG = 4 / 2 / 1 groups of threads; a group's partial sums go to LDS and are added in the fixed order
//     0, 1, .. (NG = 1: no partials, the thread's sums are the products);
//   * Y goes to LDS as a T V image of channel PAIRS (8 bytes a position: one read serves both rows); temporal mix (Y -> Yt) and
//     spatial mix (Yt -> Z) run thread <-> position with the loop over frames / joints at its exact length: no K padding exists, so
//     no neighbouring frame can leak in.  Lanes of one instruction read one address per (frame, joint) column (broadcast) or
//     consecutive pairs and write pairs with stride 1 or V (17 / 25: odd, so the 8-byte writes of a column collide two-way at most,
//     frames q and q + 16), and there is no row stride to choose;
//   * a thread's table values (T + V per position) are read per clip through L1 / L2 (held for the launch they would cost up to 147
//     registers, and the stream wants workgroups per CU more than it wants them);
//   * epilogue: thread <-> four positions again: x_rec = PReLU_out(Z + R), stored as 16-byte vectors when `out` is given; the squared
//     difference to `x` is summed lanes -> waves -> one value in a fixed order and ONE thread stores score[n];
//   * (coskad_layer_tail_map_f32) the same differences also leave as the per-position error map emap[n, t, v], whose sum is score[n].
// No atomics; a clip's results do not depend on B, on the workgroup that forms them or on the loop round.  Threads beyond a clip's
// vectors / positions walk every barrier and store nothing.
#include "layer_launch.h"
#include <cstdint>

namespace coskad {
namespace evt {

constexpr int kThreads = 256;
constexpr int kCUs = 256;

template <int T, int V, int Ci>
struct Geo {
  static_assert(T % 4 == 0, "rows are read as float4");
  static constexpr int TV = T * V, R4 = TV / 4;
  static_assert(R4 <= kThreads, "a thread per 16-byte vector of a row");
  // channel groups of the products: the largest of 4, 2, 1 whose threads fit the workgroup
  static constexpr int NG = 4 * R4 <= kThreads ? 4 : (2 * R4 <= kThreads ? 2 : 1);
  static constexpr int CG = Ci / NG;                      // channels of a group
  static_assert(Ci % NG == 0 && CG % 4 == 0, "four loads in flight per thread and step");
  static constexpr int PER_CU = 4;                        // workgroups (= waves per SIMD) a CU is asked to hold: <= 128 registers
  static constexpr int PART = NG > 1 ? NG * 4 * TV : 0;   // floats of the partial sums
  static constexpr int LDS_FLOATS = 16 + 4 * Ci + 2 * 2 * TV + PART;
  static_assert(LDS_FLOATS * 4 <= 48 * 1024, "far inside the LDS");
};

__device__ __forceinline__ float4 prelu4(float4 v, float a) {
  return float4{prelu_f(v.x, a), prelu_f(v.y, a), prelu_f(v.z, a), prelu_f(v.w, a)};
}
__device__ __forceinline__ void fma4(float4& acc, float w, const float4& x) {
  acc.x = fmaf(w, x.x, acc.x); acc.y = fmaf(w, x.y, acc.y); acc.z = fmaf(w, x.z, acc.z); acc.w = fmaf(w, x.w, acc.w);
}
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w}; }

// kMap: also the clip's per-position error map, emap[n, t, v] = ((x_rec_0 - x_0)^2 + (x_rec_1 - x_1)^2) / (2 T V), from the differences the
// score is summed from -- one 16-byte store per `own` thread, behind no barrier of its own; the score's arithmetic is untouched.  The
// switch is the parameter pack `Map`: empty (the score / out kernel: its argument segment, and with it every instruction, is what it
// was without the switch) or one `float` (the map kernel, whose last argument is `emap`).
__device__ __forceinline__ float* map_base(float* p) { return p; }

template <int T, int V, int Ci, typename... Map>
__global__ __launch_bounds__(kThreads, (Geo<T, V, Ci>::PER_CU)) void k_eval_tail(
    const float* __restrict__ in, const float* __restrict__ x, float* __restrict__ out, float* __restrict__ score,
    const float* __restrict__ Aw, const float* __restrict__ Tw, const float* __restrict__ wfold, const float* __restrict__ bias,
    const float* __restrict__ in_slope, const float* __restrict__ out_slope, int B, Map* __restrict__... emap) {
  constexpr bool kMap = sizeof...(Map) == 1;
  static_assert(sizeof...(Map) <= 1, "at most the map's base");
  using G = Geo<T, V, Ci>;
  constexpr int TV = G::TV, R4 = G::R4, NG = G::NG, CG = G::CG;
  constexpr int CoP = 16;                                  // coskad_bn_fold_f32's column count for two output channels
  __shared__ __attribute__((aligned(16))) float lds[G::LDS_FLOATS];
  float* red = lds;                  // [4] a wave's sum of squared differences
  float* wl = lds + 16;              // [4][Ci]: rows Wz0, Wz1, Wx0, Wx1
  float2* ya = reinterpret_cast<float2*>(wl + 4 * Ci);   // [TV] pairs (channel 0, channel 1): Y, then Z
  float2* yb = ya + TV;                                  // [TV] pairs: Yt
  float* part = reinterpret_cast<float*>(yb + TV);       // (NG > 1) [NG][4][TV]
  const int tid = threadIdx.x;
  for (int e = tid; e < 4 * Ci; e += kThreads) {
    const int j = e / Ci, c = e - j * Ci;
    wl[e] = wfold[((j >> 1) * Ci + c) * CoP + (j & 1)];
  }
  const float b0 = bias[0], b1 = bias[1];
  const bool pre = in_slope != nullptr, post = out_slope != nullptr;
  const float a_in = pre ? in_slope[0] : 0.f, a_out = post ? out_slope[0] : 0.f;
  const int grp = tid / R4, e4 = tid - grp * R4;           // products: channel group, vector of the row
  const bool prod = grp < NG, own = tid < R4;              // `own`: the thread of four positions in the sum and the epilogue
  // temporal  Yt[q, v] = sum_t Y[t, v] T[v][t][q]  (position idx = v T + q);  spatial  Z[t, w] = sum_v Yt[t, v] A[t][v][w]  (idx = t V + w)
  const float* Ap = Aw;
  const float* Tp = Tw;
  __syncthreads();                                         // wl
  for (int clip = blockIdx.x; clip < B; clip += gridDim.x) {
    // ---- products: [Y; R] = [Wz; Wx] PReLU(in) over this group's channels ------------------------------------------------------------
    float4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = float4{0.f, 0.f, 0.f, 0.f};
    if (prod) {
      const float4* src = reinterpret_cast<const float4*>(in) + ((size_t)clip * Ci + grp * CG) * R4 + e4;
      const float* wg = wl + grp * CG;
#pragma unroll 1
      for (int c = 0; c < CG; c += 4) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = src[(size_t)(c + u) * R4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 xv = pre ? prelu4(v[u], a_in) : v[u];
#pragma unroll
          for (int j = 0; j < 4; ++j) fma4(acc[j], wg[j * Ci + c + u], xv);
        }
      }
    }
    // the clip's target, in flight through the mixing phases
    float4 xt[2] = {float4{0.f, 0.f, 0.f, 0.f}, float4{0.f, 0.f, 0.f, 0.f}};
    if (score != nullptr && own) {
      const float4* x4 = reinterpret_cast<const float4*>(x) + (size_t)clip * 2 * R4 + e4;
      xt[0] = x4[0];
      xt[1] = x4[R4];
    }
    float4 r0, r1;
    if constexpr (NG > 1) {
      if (prod) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(part + (grp * 4 + j) * TV + 4 * e4) = acc[j];
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = float4{0.f, 0.f, 0.f, 0.f};
      if (own) {
#pragma unroll
        for (int g = 0; g < NG; ++g)                       // the groups in a fixed order
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = add4(acc[j], *reinterpret_cast<const float4*>(part + (g * 4 + j) * TV + 4 * e4));
      }
    }
    if (own) {
      float4* y4 = reinterpret_cast<float4*>(ya + 4 * e4);
      y4[0] = float4{acc[0].x, acc[1].x, acc[0].y, acc[1].y};
      y4[1] = float4{acc[0].z, acc[1].z, acc[0].w, acc[1].w};
    }
    r0 = float4{acc[2].x + b0, acc[2].y + b0, acc[2].z + b0, acc[2].w + b0};
    r1 = float4{acc[3].x + b1, acc[3].y + b1, acc[3].z + b1, acc[3].w + b1};
    asm volatile("" : "+s"(Ap), "+s"(Tp));             // (the table values are read per clip, not hoisted into registers)
    __syncthreads();                                       // the image holds Y
    // ---- temporal mix: ya -> yb ------------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int idx = tid; idx < TV; idx += kThreads) {
      const int v = idx / T, q = idx - v * T;
      float y0 = 0.f, y1 = 0.f;
#pragma unroll 4
      for (int k = 0; k < T; ++k) {
        const float w = Tp[(v * T + k) * T + q];
        const float2 y = ya[k * V + v];
        y0 = fmaf(y.x, w, y0);
        y1 = fmaf(y.y, w, y1);
      }
      yb[q * V + v] = float2{y0, y1};
    }
    __syncthreads();
    // ---- spatial mix: yb -> ya -------------------------------------------------------------------------------------------------------
#pragma unroll 1
    for (int idx = tid; idx < TV; idx += kThreads) {
      const int t = idx / V, w = idx - t * V;
      float z0 = 0.f, z1 = 0.f;
#pragma unroll 5
      for (int k = 0; k < V; ++k) {
        const float a = Ap[(t * V + k) * V + w];
        const float2 y = yb[t * V + k];
        z0 = fmaf(y.x, a, z0);
        z1 = fmaf(y.y, a, z1);
      }
      ya[idx] = float2{z0, z1};
    }
    __syncthreads();                                       // the image holds Z
    // ---- epilogue: x_rec = PReLU_out(Z + R); the clip's squared error ------------------------------------------------------------------
    float sq = 0.f;
    if (own) {
      const float4* z4 = reinterpret_cast<const float4*>(ya + 4 * e4);
      const float4 za = z4[0], zb = z4[1];
      float4 u0 = add4(float4{za.x, za.z, zb.x, zb.z}, r0);
      float4 u1 = add4(float4{za.y, za.w, zb.y, zb.w}, r1);
      if (post) { u0 = prelu4(u0, a_out); u1 = prelu4(u1, a_out); }
      if (out != nullptr) {
        float4* o4 = reinterpret_cast<float4*>(out) + (size_t)clip * 2 * R4 + e4;
        o4[0] = u0;
        o4[R4] = u1;
      }
      const float d[8] = {u0.x - xt[0].x, u0.y - xt[0].y, u0.z - xt[0].z, u0.w - xt[0].w,
                          u1.x - xt[1].x, u1.y - xt[1].y, u1.z - xt[1].z, u1.w - xt[1].w};
#pragma unroll
      for (int k = 0; k < 8; ++k) sq = fmaf(d[k], d[k], sq);
      if constexpr (kMap) {                                // positions idx = t V + v = 4 e4 .. 4 e4 + 3: TV % 4 == 0, a 16-byte address
        constexpr float kScale = 1.f / (2 * TV);
        *reinterpret_cast<float4*>(map_base(emap...) + (size_t)clip * TV + 4 * e4) =
            float4{(d[0] * d[0] + d[4] * d[4]) * kScale, (d[1] * d[1] + d[5] * d[5]) * kScale,
                   (d[2] * d[2] + d[6] * d[6]) * kScale, (d[3] * d[3] + d[7] * d[7]) * kScale};
      }
    }
    if (score != nullptr) {                                // (uniform over the workgroup)
      sq = wave_sum(sq);
      if ((tid & 63) == 0) red[tid >> 6] = sq;
      __syncthreads();
      if (tid == 0) score[clip] = (((red[0] + red[1]) + red[2]) + red[3]) * (1.f / (2 * TV));
    } else if constexpr (NG == 1) {
      __syncthreads();                                     // (no partials: the next clip's Y goes straight into the image read above)
    }
    // (the next clip's write to `red` comes behind three more barriers; its writes to `part` / the images behind a barrier that
    // follows this clip's last reads of them)
  }
}

struct Args {
  const float* in;
  const float* x;
  float* out;
  float* score;
  const float* Aw;
  const float* Tw;
  const float* wfold;
  const float* bias;
  const float* in_slope;
  const float* out_slope;
  int B;
  hipStream_t st;
  float* emap;   // the map entry only
};

template <int T, int V, int Ci, bool kMap>
static void launch_one(const Args& a) {
  using G = Geo<T, V, Ci>;
  const int cap = kCUs * G::PER_CU;                        // the persistent grid: PER_CU workgroups on each CU
  const int grid = a.B < cap ? a.B : cap;
  ProbeScope probe(KID_LAYER_APPLY, Ci, 2, a.st);
  if constexpr (kMap)
    hipLaunchKernelGGL((k_eval_tail<T, V, Ci, float>), dim3(grid), dim3(kThreads), 0, a.st, a.in, a.x, a.out, a.score, a.Aw, a.Tw,
                       a.wfold, a.bias, a.in_slope, a.out_slope, a.B, a.emap);
  else
    hipLaunchKernelGGL((k_eval_tail<T, V, Ci>), dim3(grid), dim3(kThreads), 0, a.st, a.in, a.x, a.out, a.score, a.Aw, a.Tw, a.wfold,
                       a.bias, a.in_slope, a.out_slope, a.B);
}

template <int T, int V, bool kMap>
static void launch_tv(const Args& a, int Ci) {
  if (Ci == 16) launch_one<T, V, 16, kMap>(a);
  else launch_one<T, V, 32, kMap>(a);
}

template <int V, bool kMap>
static void launch_v(const Args& a, int T, int Ci) {
  if (T == 8) launch_tv<8, V, kMap>(a, Ci);
  else if (T == 12) launch_tv<12, V, kMap>(a, Ci);
  else if (T == 16) launch_tv<16, V, kMap>(a, Ci);
  else launch_tv<24, V, kMap>(a, Ci);
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static bool tail_ok(int T, int V, int Ci, int Co) {
  return (T == 8 || T == 12 || T == 16 || T == 24) && (V == 17 || V == 25) && (Ci == 16 || Ci == 32) && Co == 2;
}

}  // namespace evt
}  // namespace coskad

using namespace coskad;

extern "C" {

int coskad_layer_tail_ok(int T, int V, int Ci, int Co) { return evt::tail_ok(T, V, Ci, Co) ? 1 : 0; }

int coskad_layer_tail_max_grid(int T, int V, int Ci) {
  // (one value today: every instantiation is compiled for four workgroups per CU -- evt::Geo::PER_CU)
  return evt::tail_ok(T, V, Ci, 2) ? evt::kCUs * evt::Geo<8, 17, 16>::PER_CU : 0;
}

int coskad_layer_tail_f32(const float* in, const float* x, float* out, float* score, const float* A, const float* Tm,
                          const float* wfold, const float* bias, const float* in_slope, const float* out_slope, int B, int Ci,
                          int Co, int T, int V, hipStream_t stream) {
  if (!in || !A || !Tm || !wfold || !bias) return fail(COSKAD_ERR_ARG, "layer_tail: null pointer");
  if (B <= 0 || Ci <= 0 || Co <= 0) return fail(COSKAD_ERR_ARG, "layer_tail: B=%d Ci=%d Co=%d", B, Ci, Co);
  if (!out && !score) return fail(COSKAD_ERR_ARG, "layer_tail: neither `out` nor `score` asked for");
  if (score && !x) return fail(COSKAD_ERR_ARG, "layer_tail: `score` needs the target `x`");
  if (!evt::aligned16(in)) return fail(COSKAD_ERR_ARG, "layer_tail: `in` (%p) must be 16-byte aligned", (const void*)in);
  if (!evt::aligned16(x)) return fail(COSKAD_ERR_ARG, "layer_tail: `x` (%p) must be 16-byte aligned", (const void*)x);
  if (!evt::aligned16(out)) return fail(COSKAD_ERR_ARG, "layer_tail: `out` (%p) must be 16-byte aligned", (const void*)out);
  if ((reinterpret_cast<uintptr_t>(score) & 3) != 0)
    return fail(COSKAD_ERR_ARG, "layer_tail: `score` (%p) must be 4-byte aligned", (const void*)score);
  if (!evt::tail_ok(T, V, Ci, Co))
    return fail(COSKAD_ERR_SHAPE, "unsupported layer_tail shape (n_frames=%d, n_joints=%d, C_in=%d, C_out=%d): built for T in "
                "{8,12,16,24}, V in {17,25}, C_in in {16,32}, C_out = 2", T, V, Ci, Co);
  const evt::Args a{in, x, out, score, A, Tm, wfold, bias, in_slope, out_slope, B, stream, nullptr};
  if (V == 17) evt::launch_v<17, false>(a, T, Ci);
  else evt::launch_v<25, false>(a, T, Ci);
  return check_launch("layer_tail");
}

int coskad_layer_tail_map_f32(const float* in, const float* x, float* out, float* score, float* emap, const float* A, const float* Tm,
                              const float* wfold, const float* bias, const float* in_slope, const float* out_slope, int B, int Ci,
                              int Co, int T, int V, hipStream_t stream) {
  if (!in || !A || !Tm || !wfold || !bias) return fail(COSKAD_ERR_ARG, "layer_tail_map: null pointer");
  if (B <= 0 || Ci <= 0 || Co <= 0) return fail(COSKAD_ERR_ARG, "layer_tail_map: B=%d Ci=%d Co=%d", B, Ci, Co);
  if (!x) return fail(COSKAD_ERR_ARG, "layer_tail_map: the target `x` is NULL");
  if (!score) return fail(COSKAD_ERR_ARG, "layer_tail_map: `score` is NULL");
  if (!emap) return fail(COSKAD_ERR_ARG, "layer_tail_map: `emap` is NULL");
  if (!evt::aligned16(in)) return fail(COSKAD_ERR_ARG, "layer_tail_map: `in` (%p) must be 16-byte aligned", (const void*)in);
  if (!evt::aligned16(x)) return fail(COSKAD_ERR_ARG, "layer_tail_map: `x` (%p) must be 16-byte aligned", (const void*)x);
  if (!evt::aligned16(out)) return fail(COSKAD_ERR_ARG, "layer_tail_map: `out` (%p) must be 16-byte aligned", (const void*)out);
  if (!evt::aligned16(emap)) return fail(COSKAD_ERR_ARG, "layer_tail_map: `emap` (%p) must be 16-byte aligned", (const void*)emap);
  if ((reinterpret_cast<uintptr_t>(score) & 3) != 0)
    return fail(COSKAD_ERR_ARG, "layer_tail_map: `score` (%p) must be 4-byte aligned", (const void*)score);
  if (!evt::tail_ok(T, V, Ci, Co))
    return fail(COSKAD_ERR_SHAPE, "unsupported layer_tail_map shape (n_frames=%d, n_joints=%d, C_in=%d, C_out=%d): built for T in "
                "{8,12,16,24}, V in {17,25}, C_in in {16,32}, C_out = 2", T, V, Ci, Co);
  const evt::Args a{in, x, out, score, A, Tm, wfold, bias, in_slope, out_slope, B, stream, emap};
  if (V == 17) evt::launch_v<17, true>(a, T, Ci);
  else evt::launch_v<25, true>(a, T, Ci);
  return check_launch("layer_tail_map");
}

}  // extern "C"
