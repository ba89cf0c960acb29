// The spherical VAE's latent head at 16 < latent <= 512: the three launches of csrc/vae_head.hip (prep, sample, bwd -- that file's
// comments and the torch restatement in coskad_amd/models/sts/vae.py are the specification) with ONE WAVE per clip, four clips per
// 256-thread block.  Lane `lane` holds elements lane, lane + 64, ... (up to 8 per lane); norms and dots are a per-lane fma chain
// followed by wave_sum (a fixed butterfly: two runs agree bit for bit).  Lanes beyond the latent hold exact zeros in every row
// and store nothing.  The per-clip scalars (t, kappa, s, |e1 - mu|, y.u, ...) are wave-uniform; the fp64 entropy / trigamma
// expressions (ps_math.h) run on lane 0, which also stores the per-clip outputs.  Rows are column views of a [B, L + 1] tensor
// (row strides ld_*): not 16-byte aligned, so every load and store is a dword, consecutive lanes on consecutive floats.
#include "common.h"
#include "ps_math.h"

namespace coskad {
namespace vhw {

using namespace vh;
constexpr int NV = kWideLMax / 64;     // elements per lane
constexpr int CLIPS = 4;               // clips (waves) per block

struct Row {
  float v[NV];
};
__device__ __forceinline__ Row load_row(const float* p, int L, int lane) {
  Row r;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = lane + 64 * i;
    r.v[i] = j < L ? p[j] : 0.f;
  }
  return r;
}
// row[j] = eps[j - 1] for 1 <= j < L (eps: the clip's L - 1 Gaussian draws), 0 elsewhere
__device__ __forceinline__ Row load_eps(const float* eps, int L, int lane) {
  Row r;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = lane + 64 * i;
    r.v[i] = (j >= 1 && j < L) ? eps[j - 1] : 0.f;
  }
  return r;
}
__device__ __forceinline__ void store_row(float* p, const Row& r, int L, int lane) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = lane + 64 * i;
    if (j < L) p[j] = r.v[i];
  }
}
__device__ __forceinline__ float dot(const Row& a, const Row& b) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) s = fmaf(a.v[i], b.v[i], s);
  return wave_sum(s);
}

// u = normalize(e1 - mu) (F.normalize: divide by max(|.|, 1e-12))
__device__ __forceinline__ Row reflect_vec(const Row& mu, int L, int lane, float* wn_out) {
  Row w;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = lane + 64 * i;
    w.v[i] = j < L ? (j == 0 ? 1.f : 0.f) - mu.v[i] : 0.f;
  }
  const float wn = fmaxf(sqrtf(dot(w, w)), 1e-12f);
#pragma unroll
  for (int i = 0; i < NV; ++i) w.v[i] = w.v[i] / wn;
  *wn_out = wn;
  return w;
}

__global__ __launch_bounds__(64 * CLIPS) void k_ps_prep(const float* __restrict__ m, int ldm, const float* __restrict__ vr, int ldv,
                                                         float* __restrict__ mu, float* __restrict__ kappa, float* __restrict__ conc,
                                                         float* __restrict__ total, int B, int L) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * CLIPS + (threadIdx.x >> 6);
  if (n >= B) return;                                          // a whole wave: no block barrier below
  const Row a = load_row(m + (size_t)n * ldm, L, lane);
  const float nm = sqrtf(dot(a, a));
  Row o;
#pragma unroll
  for (int i = 0; i < NV; ++i) o.v[i] = a.v[i] / nm;
  store_row(mu + (size_t)n * L, o, L, lane);
  if (lane == 0) {
    const float k = softplus_f(vr[(size_t)n * ldv]) + 1.f;
    const float c = 0.5f * (float)(L - 1);
    kappa[n] = k;
    conc[2 * n] = c + k;
    conc[2 * n + 1] = c;
    total[n] = (c + k) + c;
  }
}

__global__ __launch_bounds__(64 * CLIPS) void k_ps_sample(const float* __restrict__ x, const float* __restrict__ eps,
                                                           const float* __restrict__ mu, const float* __restrict__ kappa,
                                                           float* __restrict__ z, float* __restrict__ kl, float* __restrict__ ikappa, int B,
                                                           int L) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * CLIPS + (threadIdx.x >> 6);
  if (n >= B) return;
  const float t = 2.f * x[2 * n] - 1.f;
  const Row e = load_eps(eps + (size_t)n * (L - 1), L, lane);
  const float en = fmaxf(sqrtf(dot(e, e)), 1e-12f);
  const float s = sqrtf(fmaxf(1.f - t * t, 0.f));
  Row y;
#pragma unroll
  for (int i = 0; i < NV; ++i) y.v[i] = lane + 64 * i == 0 ? t : s * (e.v[i] / en);
  const Row m = load_row(mu + (size_t)n * L, L, lane);
  float wn;
  const Row u = reflect_vec(m, L, lane, &wn);
  const float yu = dot(y, u);
  Row o;
#pragma unroll
  for (int i = 0; i < NV; ++i) o.v[i] = y.v[i] - 2.f * yu * u.v[i];
  store_row(z + (size_t)n * L, o, L, lane);
  if (lane == 0) {
    // KL(PowerSpherical || uniform) = -H(q) + H(p), as in vae_head.hip
    const double k = (double)kappa[n], b = 0.5 * (double)(L - 1), a = b + k;
    const double hq = (a + b) * kLog2 + lgamma(a) - lgamma(a + b) + b * kLogPi - k * (kLog2 + digamma_d(a) - digamma_d(a + b));
    const double hp = kLog2 + 0.5 * (double)L * kLogPi - lgamma(0.5 * (double)L);
    kl[n] = (float)(hp - hq);
    ikappa[n] = 1.f / (float)k;
  }
}

__global__ __launch_bounds__(64 * CLIPS) void k_ps_bwd(const float* __restrict__ dz, const float* __restrict__ x, const float* __restrict__ g,
                                                        const float* __restrict__ eps, const float* __restrict__ mu,
                                                        const float* __restrict__ kappa, const float* __restrict__ m, int ldm,
                                                        const float* __restrict__ vr, int ldv, float w_kl, float w_exp,
                                                        float* __restrict__ dm, int lddm, float* __restrict__ dv, int lddv, int B, int L) {
  const int lane = threadIdx.x & 63, n = blockIdx.x * CLIPS + (threadIdx.x >> 6);
  if (n >= B) return;
  const Row gz = load_row(dz + (size_t)n * L, L, lane);
  const Row mur = load_row(mu + (size_t)n * L, L, lane);
  const float zb = x[2 * n], t = 2.f * zb - 1.f;
  const Row e = load_eps(eps + (size_t)n * (L - 1), L, lane);
  const float en = fmaxf(sqrtf(dot(e, e)), 1e-12f);
  const float om = 1.f - t * t, s = sqrtf(fmaxf(om, 0.f));
  Row vv, y;
#pragma unroll
  for (int i = 0; i < NV; ++i) { vv.v[i] = e.v[i] / en; y.v[i] = lane + 64 * i == 0 ? t : s * vv.v[i]; }
  float wn;
  const Row u = reflect_vec(mur, L, lane, &wn);
  const float yu = dot(y, u), gu = dot(gz, u);
  // z = y - 2 (y.u) u:  dy = dz - 2 (dz.u) u;  du = -2 ((y.u) dz + (dz.u) y)
  Row dy, du;
#pragma unroll
  for (int i = 0; i < NV; ++i) { dy.v[i] = gz.v[i] - 2.f * gu * u.v[i]; du.v[i] = -2.f * (yu * gz.v[i] + gu * y.v[i]); }
  // u = w / |w|, w = e1 - mu:  dw = (du - (du.u) u) / |w|;  dmu = -dw
  const float duu = dot(du, u);
  Row dmu;
#pragma unroll
  for (int i = 0; i < NV; ++i) dmu.v[i] = lane + 64 * i < L ? -(du.v[i] - duu * u.v[i]) / wn : 0.f;
  // mu = m / |m|:  dm = (dmu - (dmu.mu) mu) / |m|
  const Row mr = load_row(m + (size_t)n * ldm, L, lane);
  const float nm = sqrtf(dot(mr, mr)), dmm = dot(dmu, mur);
  Row o;
#pragma unroll
  for (int i = 0; i < NV; ++i) o.v[i] = (dmu.v[i] - dmm * mur.v[i]) / nm;
  store_row(dm + (size_t)n * lddm, o, L, lane);
  // y = [t, s v]:  dt = dy_0 + (dy_{1:}.v) ds/dt, ds/dt = -t / s where 1 - t^2 > 0
  float dyv = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) dyv = lane + 64 * i >= 1 ? fmaf(dy.v[i], vv.v[i], dyv) : dyv;
  dyv = wave_sum(dyv);
  if (lane == 0) {                                             // (lane 0 holds element 0: dy.v[0] is dy_0)
    const float dt = dy.v[0] + (om > 0.f ? dyv * (-t / s) : 0.f);
    // _Dirichlet_backward with the upstream gradient (2 dt, 0): d alpha = g_0 (2 dt - x_0 2 dt)
    const float dz0 = 2.f * dt;
    const float dalpha = g[2 * n] * (dz0 - zb * dz0);
    // d kl / d kappa = kappa (psi1(alpha) - psi1(alpha + beta));  d (1 / kappa) = -1 / kappa^2
    const double k = (double)kappa[n], b = 0.5 * (double)(L - 1), a = b + k;
    const double dk = (double)dalpha + (double)w_kl * k * (trigamma_d(a) - trigamma_d(a + b)) - (double)w_exp / (k * k);
    // kappa = softplus(v) + 1:  dv = dk sigmoid(v)   (v > 20: softplus is the identity there)
    const float v = vr[(size_t)n * ldv];
    const float sg = v > 20.f ? 1.f : 1.f / (1.f + expf(-v));
    dv[(size_t)n * lddv] = (float)dk * sg;
  }
}

}  // namespace vhw

int wide_ps_head_prep(const float* mean_raw, int ld_mean, const float* var_raw, int ld_var, float* mu, float* kappa, float* concentration,
                      float* total, int B, int L, hipStream_t stream) {
  hipLaunchKernelGGL(vhw::k_ps_prep, dim3(ceil_div(B, vhw::CLIPS)), dim3(64 * vhw::CLIPS), 0, stream, mean_raw, ld_mean, var_raw, ld_var,
                     mu, kappa, concentration, total, B, L);
  return check_launch("ps_head_prep (wide)");
}

int wide_ps_head_sample(const float* x, const float* eps, const float* mu, const float* kappa, float* z, float* kl, float* inv_kappa, int B,
                        int L, hipStream_t stream) {
  hipLaunchKernelGGL(vhw::k_ps_sample, dim3(ceil_div(B, vhw::CLIPS)), dim3(64 * vhw::CLIPS), 0, stream, x, eps, mu, kappa, z, kl, inv_kappa,
                     B, L);
  return check_launch("ps_head_sample (wide)");
}

int wide_ps_head_bwd(const float* dz, const float* x, const float* dirichlet_grad, const float* eps, const float* mu, const float* kappa,
                     const float* mean_raw, int ld_mean, const float* var_raw, int ld_var, float w_kl, float w_exp, float* d_mean_raw,
                     int ld_dmean, float* d_var_raw, int ld_dvar, int B, int L, hipStream_t stream) {
  hipLaunchKernelGGL(vhw::k_ps_bwd, dim3(ceil_div(B, vhw::CLIPS)), dim3(64 * vhw::CLIPS), 0, stream, dz, x, dirichlet_grad, eps, mu, kappa,
                     mean_raw, ld_mean, var_raw, ld_var, w_kl, w_exp, d_mean_raw, ld_dmean, d_var_raw, ld_dvar, B, L);
  return check_launch("ps_head_bwd (wide)");
}

}  // namespace coskad
