// The Gaussian VAE's latent head (`distribution: 'normal'`; reference models/sts/vae.py:85,106-108,129 and the loss terms of
// models/spherical_vae.py:89-90,98 -- three torch.distributions calls, so torch in float64 on the same noise is the specification):
// everything between the raw outputs of fc_mean / fc_var and the decoder's input, one launch forward and one backward.
//
//   fwd   sigma = softplus(var_raw) + 1 (beta = 1, threshold = 20);  z = mean_raw + sigma eps  (Normal.rsample on the caller's eps)
//         kl[n]  = sum_l 0.5 (sigma^2 + mu^2 - 1 - log sigma^2)   = kl_divergence(Normal(mu, sigma), Normal(0, 1)).sum(-1)
//         inv[n] = sum_l 1 / sigma
//         score[n] = 1 - F.cosine_similarity(ref, z[n]): sum_l (ref_l / max(|ref|, 1e-8)) (z_l / max(|z|, 1e-8)), torch's order
//   bwd   d_mean_raw = dz + w_kl mu;  d_var_raw = (dz eps + w_kl (sigma - 1 / sigma) - w_exp / sigma^2) softplus'(var_raw),
//         softplus' = e^x / (e^x + 1) at x <= 20, 1 above (torch's softplus_backward)
//
// Lanes run along l.  L <= 64: a clip is a segment of SEG = the next power of two >= L lanes, 64 / SEG clips per wave, and a row sum
// is a butterfly of log2 SEG cross-lane moves.  L > 64: one wave per clip, lane `lane` holds elements 4 (lane + 64 c) + k (c < 2,
// k < 4): one 16-byte access per chunk where L, the row strides and the pointers are multiples of 4 floats, four dwords otherwise
// -- the SAME element-to-lane map either way, so a row sum (the lane's eight terms in (c, k) order, then wave_sum) is formed in an
// order that depends on L alone: not on B, the grid, the wave that takes the clip or the operands' alignment.  Pad lanes (l >= L)
// and clips beyond B hold exact zeros in every sum and store nothing.  Grid-stride over waves' clip groups; no atomics, no LDS.
#include "latent_row.h"
#include "ps_math.h"

namespace coskad {
namespace vhn {

using vh::softplus_f;
constexpr int kWaves = 4;              // waves per block
constexpr float kCosEps = 1e-8f;       // F.cosine_similarity's default eps: each norm is clamped from below on its own

// ---- element-to-lane maps ---------------------------------------------------------------------------------------------------------
template <int SEG_>
struct Small {                         // L <= SEG <= 64: one element per lane, 64 / SEG clips per wave
  static constexpr int CPW = 64 / SEG_, NE = 1;
  static __device__ __forceinline__ int sub(int lane) { return lane / SEG_; }
  static __device__ __forceinline__ void load(const float* __restrict__ p, int L, int lane, bool row, float (&v)[NE]) {
    const int l = lane % SEG_;
    v[0] = (row && l < L) ? p[l] : 0.f;
  }
  static __device__ __forceinline__ void store(float* __restrict__ p, int L, int lane, bool row, const float (&v)[NE]) {
    const int l = lane % SEG_;
    if (row && l < L) p[l] = v[0];
  }
  static __device__ __forceinline__ bool ok(int L, int lane, int e) { return lane % SEG_ < L; }
  static __device__ __forceinline__ bool first(int lane) { return lane % SEG_ == 0; }
  static __device__ __forceinline__ float reduce(float v) {
#pragma unroll
    for (int off = SEG_ / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
  }
};

template <bool VEC>
struct Wide {                          // 64 < L <= 512: one clip per wave, elements 4 (lane + 64 c) + k
  static constexpr int CPW = 1, NC = kWideLMax / 256, NE = 4 * NC;
  static __device__ __forceinline__ int sub(int) { return 0; }
  static __device__ __forceinline__ void load(const float* __restrict__ p, int L, int lane, bool row, float (&v)[NE]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int l = 4 * (lane + 64 * c);
      if (VEC) {                       // L % 4 == 0: the four elements are inside together
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row && l < L) q = *reinterpret_cast<const float4*>(p + l);
        v[4 * c] = q.x; v[4 * c + 1] = q.y; v[4 * c + 2] = q.z; v[4 * c + 3] = q.w;
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[4 * c + k] = (row && l + k < L) ? p[l + k] : 0.f;
      }
    }
  }
  static __device__ __forceinline__ void store(float* __restrict__ p, int L, int lane, bool row, const float (&v)[NE]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const int l = 4 * (lane + 64 * c);
      if (VEC) {
        if (row && l < L) *reinterpret_cast<float4*>(p + l) = make_float4(v[4 * c], v[4 * c + 1], v[4 * c + 2], v[4 * c + 3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (row && l + k < L) p[l + k] = v[4 * c + k];
      }
    }
  }
  static __device__ __forceinline__ bool ok(int L, int lane, int e) { return 4 * (lane + 64 * (e / 4)) + (e % 4) < L; }
  static __device__ __forceinline__ bool first(int lane) { return lane == 0; }
  static __device__ __forceinline__ float reduce(float v) { return wave_sum(v); }
};

struct FwdArgs {
  const float *mean_raw, *var_raw, *eps, *ref;
  float *z, *sigma, *kl, *inv, *score;
  int ld_mean, ld_var, B, L;
};

template <class M>
__global__ __launch_bounds__(64 * kWaves) void k_fwd(FwdArgs a) {
  constexpr int NE = M::NE;
  const int lane = threadIdx.x & 63, L = a.L;
  const int nwaves = gridDim.x * kWaves, groups = ceil_div(a.B, M::CPW);
  float r[NE], rn = 0.f;
  if (a.score) {                       // the reference direction, divided by its clamped norm once per wave
    M::load(a.ref, L, lane, true, r);
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) s = fmaf(r[e], r[e], s);
    rn = fmaxf(sqrtf(M::reduce(s)), kCosEps);
#pragma unroll
    for (int e = 0; e < NE; ++e) r[e] = r[e] / rn;
  }
  for (int g = blockIdx.x * kWaves + (threadIdx.x >> 6); g < groups; g += nwaves) {   // wave-uniform bound: every lane takes the butterflies
    const int n = g * M::CPW + M::sub(lane);
    const bool row = n < a.B;
    const size_t nn = row ? (size_t)n : 0;
    float m[NE], x[NE], ep[NE], sg[NE], zz[NE];
    M::load(a.mean_raw + nn * a.ld_mean, L, lane, row, m);
    M::load(a.var_raw + nn * a.ld_var, L, lane, row, x);
    M::load(a.eps + nn * L, L, lane, row, ep);
    float skl = 0.f, sinv = 0.f, szz = 0.f;
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const bool ok = row && M::ok(L, lane, e);
      const float s = softplus_f(x[e]) + 1.f;
      const float v = s * s;
      sg[e] = s;
      zz[e] = ok ? m[e] + s * ep[e] : 0.f;
      skl += ok ? 0.5f * (v + m[e] * m[e] - 1.f - logf(v)) : 0.f;
      sinv += ok ? 1.f / s : 0.f;
      szz = fmaf(zz[e], zz[e], szz);
    }
    if (a.z) M::store(a.z + nn * L, L, lane, row, zz);
    if (a.sigma) M::store(a.sigma + nn * L, L, lane, row, sg);
    if (a.kl) {
      skl = M::reduce(skl);
      if (row && M::first(lane)) a.kl[n] = skl;
    }
    if (a.inv) {
      sinv = M::reduce(sinv);
      if (row && M::first(lane)) a.inv[n] = sinv;
    }
    if (a.score) {
      const float zn = fmaxf(sqrtf(M::reduce(szz)), kCosEps);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < NE; ++e) d += r[e] * (zz[e] / zn);
      d = M::reduce(d);
      if (row && M::first(lane)) a.score[n] = 1.f - d;
    }
  }
}

struct BwdArgs {
  const float *dz, *eps, *sigma, *mean_raw, *var_raw;
  float *d_mean, *d_var;
  float w_kl, w_exp;
  int ld_mean, ld_var, ld_dmean, ld_dvar, B, L;
};

template <class M>
__global__ __launch_bounds__(64 * kWaves) void k_bwd(BwdArgs a) {
  constexpr int NE = M::NE;
  const int lane = threadIdx.x & 63, L = a.L;
  const int nwaves = gridDim.x * kWaves, groups = ceil_div(a.B, M::CPW);
  for (int g = blockIdx.x * kWaves + (threadIdx.x >> 6); g < groups; g += nwaves) {
    const int n = g * M::CPW + M::sub(lane);
    const bool row = n < a.B;
    const size_t nn = row ? (size_t)n : 0;
    float gz[NE], ep[NE], sg[NE], m[NE], x[NE], dm[NE], dv[NE];
    M::load(a.dz + nn * L, L, lane, row, gz);
    M::load(a.eps + nn * L, L, lane, row, ep);
    M::load(a.sigma + nn * L, L, lane, row, sg);
    M::load(a.mean_raw + nn * a.ld_mean, L, lane, row, m);
    M::load(a.var_raw + nn * a.ld_var, L, lane, row, x);
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      const float s = (row && M::ok(L, lane, e)) ? sg[e] : 1.f;       // (pad lanes: keep the divisions finite; nothing is stored)
      dm[e] = gz[e] + a.w_kl * m[e];
      const float ds = gz[e] * ep[e] + a.w_kl * (s - 1.f / s) - a.w_exp / (s * s);
      const float ex = expf(x[e]);
      dv[e] = x[e] > 20.f ? ds : ds * ex / (ex + 1.f);
    }
    M::store(a.d_mean + nn * a.ld_dmean, L, lane, row, dm);
    M::store(a.d_var + nn * a.ld_dvar, L, lane, row, dv);
  }
}

inline int grid_of(int B, int cpw) {
  constexpr int kGridCap = 2048;       // eight 4-wave blocks per CU; more clips than that ride the grid-stride loop
  const int blocks = ceil_div(ceil_div(B, cpw), kWaves);
  return blocks < kGridCap ? blocks : kGridCap;
}

template <class M>
int launch_fwd(const FwdArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_fwd<M>, dim3(grid_of(a.B, M::CPW)), dim3(64 * kWaves), 0, stream, a);
  return check_launch("normal_head_fwd");
}
template <class M>
int launch_bwd(const BwdArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_bwd<M>, dim3(grid_of(a.B, M::CPW)), dim3(64 * kWaves), 0, stream, a);
  return check_launch("normal_head_bwd");
}

// one instantiation per segment width (the next power of two >= L) and the two access widths above 64
#define COSKAD_NORMAL_HEAD_DISPATCH(LAUNCH, L_, VEC_, ARGS, STREAM)     \
  do {                                                                  \
    if ((L_) > 64) return (VEC_) ? LAUNCH<Wide<true>>(ARGS, STREAM) : LAUNCH<Wide<false>>(ARGS, STREAM); \
    if ((L_) > 32) return LAUNCH<Small<64>>(ARGS, STREAM);              \
    if ((L_) > 16) return LAUNCH<Small<32>>(ARGS, STREAM);              \
    if ((L_) > 8) return LAUNCH<Small<16>>(ARGS, STREAM);               \
    if ((L_) > 4) return LAUNCH<Small<8>>(ARGS, STREAM);                \
    if ((L_) > 2) return LAUNCH<Small<4>>(ARGS, STREAM);                \
    if ((L_) > 1) return LAUNCH<Small<2>>(ARGS, STREAM);                \
    return LAUNCH<Small<1>>(ARGS, STREAM);                              \
  } while (0)

inline bool al16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }   // (a null pointer counts as aligned)

}  // namespace vhn
}  // namespace coskad

using namespace coskad;

extern "C" {

int coskad_normal_head_ok(int L) { return (L >= 1 && L <= kWideLMax) ? 1 : 0; }

int coskad_normal_head_fwd_f32(const float* mean_raw, int ld_mean, const float* var_raw, int ld_var, const float* eps, float* z,
                               float* sigma, float* kl, float* inv, const float* ref, float* score, int B, int L,
                               hipStream_t stream) {
  if (!mean_raw || !var_raw || !eps) return fail(COSKAD_ERR_ARG, "normal_head_fwd: null pointer (mean_raw / var_raw / eps)");
  if (!coskad_normal_head_ok(L)) return fail(COSKAD_ERR_SHAPE, "normal_head_fwd: latent=%d outside 1..%d", L, kWideLMax);
  if (B == 0) return fail(COSKAD_ERR_SHAPE, "normal_head_fwd: B=%d latent=%d", B, L);      // as the ps_head entries
  if (B < 0) return fail(COSKAD_ERR_ARG, "normal_head_fwd: B=%d", B);
  if (ld_mean < L) return fail(COSKAD_ERR_ARG, "normal_head_fwd: ld_mean=%d < latent=%d", ld_mean, L);
  if (ld_var < L) return fail(COSKAD_ERR_ARG, "normal_head_fwd: ld_var=%d < latent=%d", ld_var, L);
  if (score && !ref) return fail(COSKAD_ERR_ARG, "normal_head_fwd: score without ref");
  if (!z && !score) return fail(COSKAD_ERR_ARG, "normal_head_fwd: neither z nor score");
  const vhn::FwdArgs a{mean_raw, var_raw, eps, score ? ref : nullptr, z, sigma, kl, inv, score, ld_mean, ld_var, B, L};
  const bool vec = L % 4 == 0 && ld_mean % 4 == 0 && ld_var % 4 == 0 && vhn::al16(mean_raw) && vhn::al16(var_raw) && vhn::al16(eps) &&
                   vhn::al16(z) && vhn::al16(sigma) && vhn::al16(a.ref);
  using namespace vhn;
  COSKAD_NORMAL_HEAD_DISPATCH(launch_fwd, L, vec, a, stream);
}

int coskad_normal_head_bwd_f32(const float* dz, const float* eps, const float* sigma, const float* mean_raw, int ld_mean,
                               const float* var_raw, int ld_var, float w_kl, float w_exp, float* d_mean_raw, int ld_dmean,
                               float* d_var_raw, int ld_dvar, int B, int L, hipStream_t stream) {
  if (!dz || !eps || !sigma || !mean_raw || !var_raw || !d_mean_raw || !d_var_raw)
    return fail(COSKAD_ERR_ARG, "normal_head_bwd: null pointer");
  if (!coskad_normal_head_ok(L)) return fail(COSKAD_ERR_SHAPE, "normal_head_bwd: latent=%d outside 1..%d", L, kWideLMax);
  if (B == 0) return fail(COSKAD_ERR_SHAPE, "normal_head_bwd: B=%d latent=%d", B, L);
  if (B < 0) return fail(COSKAD_ERR_ARG, "normal_head_bwd: B=%d", B);
  if (ld_mean < L) return fail(COSKAD_ERR_ARG, "normal_head_bwd: ld_mean=%d < latent=%d", ld_mean, L);
  if (ld_var < L) return fail(COSKAD_ERR_ARG, "normal_head_bwd: ld_var=%d < latent=%d", ld_var, L);
  if (ld_dmean < L) return fail(COSKAD_ERR_ARG, "normal_head_bwd: ld_dmean=%d < latent=%d", ld_dmean, L);
  if (ld_dvar < L) return fail(COSKAD_ERR_ARG, "normal_head_bwd: ld_dvar=%d < latent=%d", ld_dvar, L);
  const vhn::BwdArgs a{dz, eps, sigma, mean_raw, var_raw, d_mean_raw, d_var_raw, w_kl, w_exp, ld_mean, ld_var, ld_dmean, ld_dvar, B, L};
  const bool vec = L % 4 == 0 && ld_mean % 4 == 0 && ld_var % 4 == 0 && ld_dmean % 4 == 0 && ld_dvar % 4 == 0 && vhn::al16(dz) &&
                   vhn::al16(eps) && vhn::al16(sigma) && vhn::al16(mean_raw) && vhn::al16(var_raw) && vhn::al16(d_mean_raw) &&
                   vhn::al16(d_var_raw);
  using namespace vhn;
  COSKAD_NORMAL_HEAD_DISPATCH(launch_bwd, L, vec, a, stream);
}

}  // extern "C"
