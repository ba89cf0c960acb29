// Scalar special functions of the PowerSpherical head (csrc/vae_head.hip at latent <= 16, csrc/vae_head_wide.hip above):
// digamma / trigamma by recurrence + asymptotic series in fp64, F.softplus, and the entropy constants.
#pragma once
#include "common.h"

namespace coskad {
namespace vh {

constexpr double kLog2 = 0.6931471805599453, kLogPi = 1.1447298858494002;

__device__ __forceinline__ double digamma_d(double x) {       // x > 0
  double r = 0.0;
  while (x < 6.0) { r -= 1.0 / x; x += 1.0; }
  const double f = 1.0 / (x * x);
  return r + log(x) - 0.5 / x - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132)))));
}
__device__ __forceinline__ double trigamma_d(double x) {      // x > 0
  double r = 0.0;
  while (x < 6.0) { r += 1.0 / (x * x); x += 1.0; }
  const double f = 1.0 / (x * x);
  return r + 1.0 / x + 0.5 * f + (1.0 / x) * f * (1.0 / 6 - f * (1.0 / 30 - f * (1.0 / 42 - f * (1.0 / 30 - f * (5.0 / 66)))));
}
__device__ __forceinline__ float softplus_f(float v) { return v > 20.f ? v : log1pf(expf(v)); }   // F.softplus(beta = 1, threshold = 20)

constexpr int kWideLMax = 512;      // widest latent of the head (vae_head_wide.hip)

}  // namespace vh

// vae_head_wide.hip (16 < L <= vh::kWideLMax): the launches behind coskad_ps_head_{prep,sample,bwd}_f32, arguments as there
int wide_ps_head_prep(const float* mean_raw, int ld_mean, const float* var_raw, int ld_var, float* mu, float* kappa, float* concentration,
                      float* total, int B, int L, hipStream_t stream);
int wide_ps_head_sample(const float* x, const float* eps, const float* mu, const float* kappa, float* z, float* kl, float* inv_kappa, int B,
                        int L, hipStream_t stream);
int wide_ps_head_bwd(const float* dz, const float* x, const float* dirichlet_grad, const float* eps, const float* mu, const float* kappa,
                     const float* mean_raw, int ld_mean, const float* var_raw, int ld_var, float w_kl, float w_exp, float* d_mean_raw,
                     int ld_dmean, float* d_var_raw, int ld_dvar, int B, int L, hipStream_t stream);

}  // namespace coskad
