// Scalar special functions of the latent heads of the VAEs (csrc/vae_head.hip, csrc/vae_head_normal.hip):
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

}  // namespace vh
}  // namespace coskad
