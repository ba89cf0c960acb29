// Gradient clipping and accumulation on the flat buffers of the fused train steps
// (Lightning's Trainer arguments gradient_clip_val / gradient_clip_algorithm / accumulate_grad_batches, which the reference
// honours through pl.Trainer.from_argparse_args, train_COSKAD.py:75-78).
//
//   grad_sqnorm : per-workgroup fp64 partials of |g_eff|^2, g_eff = g * gscale + reg_coef * mask * p -- the fp32 expression
//                 of k_adam (heads.hip), so the norm is that of what Adam applies
//   adam_clip   : k_adam / k_adam_dev with the clip folded in.  Norm mode: every workgroup sums the partials in one fixed
//                 order (no atomics, no ticket, no device-scope fence: one extra launch instead, DESIGN appendix) and scales
//                 g_eff by min(1, clip / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s arithmetic with an fp32 norm.
//                 Value mode: clamp of g_eff, clip_grad_value_.
//   grad_accum  : acc = first ? g : acc + g
#include "common.h"
#include <cmath>

namespace coskad {

constexpr int kClipPartials = 256;      // entries of `partials`: one per workgroup of k_grad_sqnorm, the rest 0

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the sum a 256-thread block holds one value per thread of, in a fixed order; returned to every thread.  sh: 4 doubles
__device__ __forceinline__ double block_sum_f64(double s, double* sh) {
  s = wave_sum_f64(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// the gradient Adam applies, as k_adam forms it
__device__ __forceinline__ float effective_grad(float g, float p, const float* __restrict__ mask, size_t i, float gscale,
                                                float reg_coef) {
  float gi = g * gscale;
  if (reg_coef != 0.f) gi = fmaf(reg_coef * (mask ? mask[i] : 1.f), p, gi);
  return gi;
}

__global__ __launch_bounds__(256) void k_grad_sqnorm(const float* __restrict__ g, const float* __restrict__ p,
                                                      const float* __restrict__ mask, size_t n, float gscale, float reg_coef,
                                                      double* __restrict__ partials) {
  __shared__ double sh[4];
  double s = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const double ge = (double)effective_grad(g[i], p[i], mask, i, gscale, reg_coef);
    s += ge * ge;
  }
  s = block_sum_f64(s, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
  // the entries no workgroup owns (gridDim.x <= kClipPartials)
  if (blockIdx.x == 0 && threadIdx.x >= gridDim.x) partials[threadIdx.x] = 0.0;
}

// MODE 1: clip by global norm, 2: by value.  hyper: {lr, beta1^t, beta2^t} in device memory (then lr, bc1, bc2_sqrt are unused), or
// NULL.  The update is k_adam's / k_adam_dev's expression by expression: a coefficient of exactly 1 leaves every bit as they do.
template <int MODE>
__global__ __launch_bounds__(256) void k_adam_clip(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, const float* __restrict__ mask, size_t n,
                                                    const float* __restrict__ hyper, float lr, float beta1, float beta2, float eps,
                                                    float bc1, float bc2_sqrt, float gscale, float reg_coef,
                                                    const double* __restrict__ partials, float clip_val,
                                                    float* __restrict__ norm_out) {
  float coef = 1.f;
  if (MODE == 1) {
    __shared__ double sh[4];
    const double total = block_sum_f64(partials[threadIdx.x], sh);
    const float norm = (float)sqrt(total);
    coef = fminf(1.f, clip_val / (norm + 1e-6f));
    if (norm_out && blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
  }
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (hyper) {
    lr = hyper[0];
    bc1 = 1.f - hyper[1];
    bc2_sqrt = sqrtf(1.f - hyper[2]);
  }
  const float pi = p[i];
  float gi = effective_grad(g[i], pi, mask, i, gscale, reg_coef);
  if (MODE == 1) gi = gi * coef;
  else gi = gi < -clip_val ? -clip_val : (gi > clip_val ? clip_val : gi);      // (a NaN gradient stays NaN, as under torch.clamp)
  const float mi = beta1 * m[i] + (1.f - beta1) * gi;
  const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = pi - (lr / bc1) * (mi / denom);
}

__global__ __launch_bounds__(256) void k_grad_accum(float* __restrict__ acc, const float* __restrict__ g, size_t n, int first) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  acc[i] = first ? g[i] : acc[i] + g[i];
}

static int clip_args(const char* what, const void* p, const void* g, const void* m, const void* v, size_t n,
                     const double* partials, float clip_val, int clip_mode) {
  if (!p || !g || !m || !v || n == 0) return fail(COSKAD_ERR_ARG, "%s: bad argument", what);
  if (clip_mode != 1 && clip_mode != 2) return fail(COSKAD_ERR_ARG, "%s: clip_mode %d (1 = norm, 2 = value)", what, clip_mode);
  if (!std::isfinite(clip_val) || !(clip_val > 0.f)) return fail(COSKAD_ERR_ARG, "%s: clip_val must be finite and > 0", what);
  if (clip_mode == 1 && !partials) return fail(COSKAD_ERR_ARG, "%s: norm clipping needs the partials of grad_sqnorm", what);
  return COSKAD_OK;
}

static int launch_adam_clip(const char* what, float* p, const float* g, float* m, float* v, const float* mask, size_t n,
                            const float* hyper, float lr, float beta1, float beta2, float eps, float bc1, float bc2_sqrt, float gscale,
                            float reg_coef, const double* partials, float clip_val, int clip_mode, float* norm_out,
                            hipStream_t stream) {
  const dim3 grid((unsigned)((n + 255) / 256));
  if (clip_mode == 1)
    hipLaunchKernelGGL(k_adam_clip<1>, grid, dim3(256), 0, stream, p, g, m, v, mask, n, hyper, lr, beta1, beta2, eps, bc1, bc2_sqrt,
                       gscale, reg_coef, partials, clip_val, norm_out);
  else
    hipLaunchKernelGGL(k_adam_clip<2>, grid, dim3(256), 0, stream, p, g, m, v, mask, n, hyper, lr, beta1, beta2, eps, bc1, bc2_sqrt,
                       gscale, reg_coef, partials, clip_val, norm_out);
  return check_launch(what);
}

}  // namespace coskad

using namespace coskad;

extern "C" {

/* partials[0 .. 255] (fp64): per-workgroup sums of g_eff[i]^2, g_eff = g * gscale + reg_coef * mask * p in fp32 as coskad_adam_*
 * forms it; entries beyond the grid are written 0.  Fixed summation order: repeated calls agree bit for bit. */
int coskad_grad_sqnorm_f32(const float* g, const float* p, const float* mask, size_t n, float gscale, float reg_coef,
                           double* partials, hipStream_t stream) {
  if (!g || !p || !partials || n == 0) return fail(COSKAD_ERR_ARG, "grad_sqnorm: bad argument");
  const size_t blocks = (n + 255) / 256;
  const int grid = (int)(blocks < (size_t)kClipPartials ? blocks : (size_t)kClipPartials);
  hipLaunchKernelGGL(k_grad_sqnorm, dim3(grid), dim3(256), 0, stream, g, p, mask, n, gscale, reg_coef, partials);
  return check_launch("grad_sqnorm");
}

/* coskad_adam_pow_f32 with the effective gradient clipped: clip_mode 1 by the global norm whose squared partials
 * coskad_grad_sqnorm_f32 left in `partials` (coef = min(1, clip_val / (norm + 1e-6)); the unclipped norm goes to norm_out[0]
 * when that is given), clip_mode 2 by value to [-clip_val, clip_val] (`partials` may be NULL, norm_out is not written). */
int coskad_adam_clip_pow_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float lr, float beta1,
                             float beta2, float eps, float b1pow, float b2pow, float gscale, float reg_coef,
                             const double* partials, float clip_val, int clip_mode, float* norm_out, hipStream_t stream) {
  if (int rc = clip_args("adam_clip_pow", p, g, m, v, n, partials, clip_val, clip_mode)) return rc;
  if (!(b1pow < 1.f) || !(b2pow < 1.f)) return fail(COSKAD_ERR_ARG, "adam_clip_pow: beta^t must be < 1 (t >= 1)");
  return launch_adam_clip("adam_clip_pow", p, g, m, v, mask, n, nullptr, lr, beta1, beta2, eps, 1.f - b1pow, sqrtf(1.f - b2pow),
                          gscale, reg_coef, partials, clip_val, clip_mode, norm_out, stream);
}

/* coskad_adam_dev_f32 with the same clipping: hyper = {lr, beta1^t, beta2^t} in device memory, advanced by every call. */
int coskad_adam_clip_dev_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float* hyper, float beta1,
                             float beta2, float eps, float gscale, float reg_coef, const double* partials, float clip_val,
                             int clip_mode, float* norm_out, hipStream_t stream) {
  if (int rc = clip_args("adam_clip_dev", p, g, m, v, n, partials, clip_val, clip_mode)) return rc;
  if (!hyper) return fail(COSKAD_ERR_ARG, "adam_clip_dev: bad argument");
  launch_adam_tick(hyper, beta1, beta2, stream);      // heads.hip: coskad_adam_dev_f32's own tick, so that a captured step replays
  return launch_adam_clip("adam_clip_dev", p, g, m, v, mask, n, hyper, 0.f, beta1, beta2, eps, 1.f, 1.f, gscale, reg_coef, partials,
                          clip_val, clip_mode, norm_out, stream);
}

/* acc = first ? g : acc + g over n floats. */
int coskad_grad_accum_f32(float* acc, const float* g, size_t n, int first, hipStream_t stream) {
  if (!acc || !g || n == 0) return fail(COSKAD_ERR_ARG, "grad_accum: bad argument");
  hipLaunchKernelGGL(k_grad_accum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, acc, g, n, first);
  return check_launch("grad_accum");
}

}  // extern "C"
