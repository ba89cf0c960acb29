// One-class heads on the latent z [B, L] (L <= 512), their gradients, the centre statistics,
// the L2 regulariser and the optimiser step.
//
//   Euclidean : F.mse_loss(z, c)                 (reference euclidean_encoder_staticCenter.py:187,
//                                                  euclidean_encoder_dynamicCenter.py:116)
//   Poincare  : dist(c, project(expmap0(z))).mean()        (hyperbolic_encoder.py:147,157) with the
//               formulas and epsilons of utils/hyper_math.py (:13-29, 100-105, 173-179, 207-210,
//               302-306); geoopt itself is not in the tree (parity unpinned vs geoopt).
//   centre    : running sums for c = mean(z) (staticCenter.py:114-118,172-178) and for the
//               gyromidpoint  m = sum(gamma_i z_i) / sum(gamma_i - 1)  (hyperbolic_encoder.py:122,179)
//   reg       : utils/model_utils.py:90-105 (0.5 * sum ||p||^2 over non-bias tensors / #tensors)
//
// Every row formula is written once over latent_row.h's two maps: one thread per clip with a 16-float latent in registers
// (L <= 16), one wave per clip with 8 values per lane (16 < L <= 512); the entry points below pick the instantiation by L.
// Block partials are summed in a fixed order per map (deterministic, no float atomics).  The Mahalanobis head and the Gram
// matrix are two algorithms, not two maps: LDS broadcast here, MFMA tiles in heads_wide.hip.
#include "tile_ops.h"
#include "heads_common.h"

namespace coskad {

// e = expmap0(u), p = project(e); returns p and the pieces the backward needs
template <class M>
struct Embed {
  Row<M> p;
  float un_raw, un, tn, en_raw;
  bool clamped;
};
template <class M>
__device__ __forceinline__ Embed<M> hyp_embed(const Row<M>& u) {
  Embed<M> r;
  r.un_raw = sqrtf(dot(u, u));
  r.un = fmaxf(r.un_raw, kMinNorm);
  r.tn = tanhf(fminf(fmaxf(r.un, -kTanhClamp), kTanhClamp));
  const float f = r.tn / r.un;
  Row<M> e;
#pragma unroll
  for (int i = 0; i < M::NE; ++i) e.v[i] = f * u.v[i];
  r.en_raw = sqrtf(dot(e, e));
  const float en = fmaxf(r.en_raw, kMinNorm);
  const float maxnorm = 1.f - kBallEps;
  r.clamped = en > maxnorm;
#pragma unroll
  for (int i = 0; i < M::NE; ++i) r.p.v[i] = r.clamped ? e.v[i] / en * maxnorm : e.v[i];
  return r;
}

// d = dist(c, p) = 2 artanh(|(-c) (+) p|), and dd/dp
template <class M>
__device__ __forceinline__ float poincare_dist(const Row<M>& c, const Row<M>& p, Row<M>* gp) {
  const float x2 = dot(c, c), y2 = dot(p, p), xy = -dot(c, p);
  const float alpha = 1.f + 2.f * xy + y2, beta = 1.f - x2;
  const float den = 1.f + 2.f * xy + x2 * y2;
  const float D = den + kMobiusEps;
  Row<M> m;
#pragma unroll
  for (int i = 0; i < M::NE; ++i) m.v[i] = (alpha * (-c.v[i]) + beta * p.v[i]) / D;
  const float mn = sqrtf(dot(m, m));
  const float mc = fminf(fmaxf(mn, -1.f + kArtanhEps), 1.f - kArtanhEps);
  const float d = (log1pf(mc) - log1pf(-mc));  // 2 * 0.5 * (log(1+x) - log(1-x))
  if (gp) {
    const float gmn = 2.f / (1.f - mc * mc);      // Artanh.backward on the clamped input, times 2
    const float inv = mn > 0.f ? gmn / mn : 0.f;  // d|m|/dm = m/|m| (0 at m = 0)
    Row<M> gm;
#pragma unroll
    for (int i = 0; i < M::NE; ++i) gm.v[i] = inv * m.v[i];
    // m = num / D,  num = alpha x + beta y,  x = -c, y = p
    const float gD = -dot(gm, m) / D;
    float galpha = 0.f;
#pragma unroll
    for (int i = 0; i < M::NE; ++i) galpha = fmaf(gm.v[i] / D, -c.v[i], galpha);
    galpha = M::reduce(galpha);
#pragma unroll
    for (int i = 0; i < M::NE; ++i) {
      const float x = -c.v[i], y = p.v[i];
      gp->v[i] = beta * gm.v[i] / D + galpha * (2.f * x + 2.f * y) + gD * (2.f * x + 2.f * x2 * y);
    }
  }
  return d;
}

// chain dL/dp back through project and expmap0 to dL/du
template <class M>
__device__ __forceinline__ Row<M> hyp_embed_bwd(const Row<M>& u, const Embed<M>& em, const Row<M>& gp) {
  const float f = em.tn / em.un;
  Row<M> ge;
  if (em.clamped) {
    // p = maxnorm * e / |e|  ->  ge = maxnorm (gp/|e| - e (e.gp)/|e|^3)
    const float maxnorm = 1.f - kBallEps;
    const float en = em.en_raw;
    float egp = 0.f;
#pragma unroll
    for (int i = 0; i < M::NE; ++i) egp = fmaf(f * u.v[i], gp.v[i], egp);
    egp = M::reduce(egp);
#pragma unroll
    for (int i = 0; i < M::NE; ++i) ge.v[i] = maxnorm * (gp.v[i] / en - f * u.v[i] * egp / (en * en * en));
  } else {
    ge = gp;
  }
  // e = f(un) u ; un = max(|u|, 1e-5): the norm carries gradient only when not clamped
  Row<M> gu;
  const float gf = dot(ge, u);
  float coef = 0.f;
  if (em.un_raw > kMinNorm) {
    const float sech2 = em.un < kTanhClamp ? 1.f - em.tn * em.tn : 0.f;
    const float df = (sech2 * em.un - em.tn) / (em.un * em.un);
    coef = gf * df / em.un_raw;
  }
#pragma unroll
  for (int i = 0; i < M::NE; ++i) gu.v[i] = f * ge.v[i] + coef * u.v[i];
  return gu;
}

// The row kernels' clip loop: a block of T = kHeadBlock<M> threads takes M::clips(T) clips per round, grid-stride.  The PerThread
// grids (head_blocks, ceil_div(B, kFlatBlock)) cover B in one round; the PerWave grid (wide_head_blocks) strides.
//
// Euclidean head.  slots: [0] sum (z-c)^2, [1..L] sum z, [Lp+1] #clips, [Lp+2] sum |z|
template <class M>
__global__ __launch_bounds__(kHeadBlock<M>) void k_mse_head(const float* __restrict__ z, const float* __restrict__ cvec,
                                                            float* __restrict__ dz, float* __restrict__ score, int B, int L,
                                                            float gscale, HeadOut out) {
  constexpr int T = kHeadBlock<M>;
  HeadSums<M> sums;
  const Row<M> c = load<M>(cvec, L);
  for (int n = M::clip(T); n < B; n += gridDim.x * M::clips(T)) {
    const Row<M> u = load<M>(z + (size_t)n * L, L);
    Row<M> g;
    const float sq = mse_head_row(u, c, gscale, sums, g);
    if (dz) store(dz + (size_t)n * L, g, L);
    if (score && M::first()) score[n] = sq / (float)L;  // MSELoss(reduction='none')(c, z).mean(-1), eval_utils.py:63-64
  }
  flush(sums, out, L, blockIdx.x, gridDim.x);
}

// Mahalanobis head (eval_utils.py:28-38; staticCenter.py:178-181).  slots: [0] sum dist, [1..L] sum z, [17] #clips,
// [18] sum |z|.  dist = sqrt(d^T VI d), d = z - c;  d dist / dz = (VI + VI^T) d / (2 dist).
__global__ __launch_bounds__(kFlatBlock) void k_mahalanobis_head(const float* __restrict__ z,
                                                            const float* __restrict__ cvec,
                                                            const float* __restrict__ VI,
                                                            float* __restrict__ dz, float* __restrict__ score, int B, int L,
                                                            float gscale, HeadOut out) {
  using Vec = Row<PerThread>;
  __shared__ float vi[LMAX * LMAX];
  for (int e = threadIdx.x; e < LMAX * LMAX; e += kFlatBlock) {
    const int r = e / LMAX, q = e - r * LMAX;
    vi[e] = (r < L && q < L) ? VI[r * L + q] : 0.f;
  }
  __syncthreads();
  HeadSums<PerThread> sums;
  const Vec c = load<PerThread>(cvec, L);
  for (int n = blockIdx.x * kFlatBlock + threadIdx.x; n < B; n += gridDim.x * kFlatBlock) {
    const Vec u = load<PerThread>(z + (size_t)n * L, L);
    Vec d, w, wt;
#pragma unroll
    for (int j = 0; j < LMAX; ++j) { d.v[j] = j < L ? u.v[j] - c.v[j] : 0.f; w.v[j] = 0.f; wt.v[j] = 0.f; }
#pragma unroll
    for (int r = 0; r < LMAX; ++r)
#pragma unroll
      for (int q = 0; q < LMAX; ++q) {
        const float a = vi[r * LMAX + q];          // wave-uniform address: LDS broadcast
        w.v[r] = fmaf(a, d.v[q], w.v[r]);          // (VI d)[r]
        wt.v[q] = fmaf(a, d.v[r], wt.v[q]);        // (VI^T d)[q]
      }
    const float dist = sqrtf(dot(d, w));
    sums.s0 += dist;
#pragma unroll
    for (int j = 0; j < LMAX; ++j) sums.v[j] += u.v[j];
    sums.sA += 1.f;
    sums.sB += sqrtf(dot(u, u));
    if (score) score[n] = dist;
    if (dz) {
      Vec g;
      const float inv = gscale / (2.f * dist);     // dist == 0: inf * 0 = NaN, as torch.sqrt's backward gives
#pragma unroll
      for (int j = 0; j < LMAX; ++j) g.v[j] = (w.v[j] + wt.v[j]) * inv;
      store(dz + (size_t)n * L, g, L);
    }
  }
  flush(sums, out, L, blockIdx.x, gridDim.x);
}

// gram (+)= sum_n z_n z_n^T  [L x L]; one block, thread (i, j), clips staged through LDS in fixed order.
// Sigma (z-mu)(z-mu)^T for any mu follows from it and the [1..L], [17] slots (batch_cov_mat_step, staticCenter.py:40-46).
__global__ __launch_bounds__(LMAX * LMAX) void k_gram(const float* __restrict__ z, float* __restrict__ gram, int B,
                                                     int L, int accumulate) {
  constexpr int CH = 256;
  __shared__ float zs[CH * LMAX];
  const int i = threadIdx.x / LMAX, j = threadIdx.x % LMAX;
  float s = 0.f;
  for (int n0 = 0; n0 < B; n0 += CH) {
    const int nc = min(CH, B - n0);
    __syncthreads();
    for (int e = threadIdx.x; e < nc * L; e += LMAX * LMAX) {
      const int r = e / L, q = e - r * L;
      zs[r * LMAX + q] = z[(size_t)(n0 + r) * L + q];
    }
    __syncthreads();
    if (i < L && j < L)
      for (int r = 0; r < nc; ++r) s = fmaf(zs[r * LMAX + i], zs[r * LMAX + j], s);
  }
  if (i < L && j < L) gram[i * L + j] = accumulate ? gram[i * L + j] + s : s;
}

// Poincare head.  slots: [0] sum dist, [1..L] sum gamma*zh, [Lp+1] sum (gamma-1), [Lp+2] sum |zh|
template <class M>
__global__ __launch_bounds__(kHeadBlock<M>) void k_poincare_head(const float* __restrict__ z, const float* __restrict__ cvec,
                                                                 float* __restrict__ dz, float* __restrict__ zh,
                                                                 float* __restrict__ score, int B, int L, float gscale, HeadOut out) {
  constexpr int T = kHeadBlock<M>;
  HeadSums<M> sums;
  for (int n = M::clip(T); n < B; n += gridDim.x * M::clips(T)) {
    const Row<M> u = load<M>(z + (size_t)n * L, L);
    const Embed<M> em = hyp_embed(u);
    if (zh) store(zh + (size_t)n * L, em.p, L);
    const float y2 = dot(em.p, em.p);
    const float gamma = 2.f / (1.f - y2);
#pragma unroll
    for (int i = 0; i < M::NE; ++i) sums.v[i] += gamma * em.p.v[i];
    sums.sA += gamma - 1.f;
    sums.sB += sqrtf(y2);
    if (cvec) {
      const Row<M> c = load<M>(cvec, L);
      Row<M> gp;
      const float d = poincare_dist(c, em.p, dz ? &gp : nullptr);
      sums.s0 += d;
      if (score && M::first()) score[n] = d;
      if (dz) {
#pragma unroll
        for (int i = 0; i < M::NE; ++i) gp.v[i] *= gscale;  // gscale = upstream / B
        store(dz + (size_t)n * L, hyp_embed_bwd(u, em, gp), L);
      }
    }
  }
  flush(sums, out, L, blockIdx.x, gridDim.x);
}

// stats[k] = sum_p partials[p][k] (slot 0 additionally * scale0);  acc[k] += raw sums
__global__ __launch_bounds__(64) void k_head_finalize(const float* __restrict__ partials, int P,
                                                       float scale0, float* __restrict__ stats,
                                                       float* __restrict__ acc) {
  head_finalize_slot(partials, P, scale0, stats, acc, threadIdx.x);
}

// dist(c, zh) per row for points already on the ball (eval scoring, eval_utils.py:66-67)
template <class M>
__global__ __launch_bounds__(kHeadBlock<M>) void k_poincare_dist(const float* __restrict__ zh, const float* __restrict__ cvec,
                                                                 float* __restrict__ score, int B, int L) {
  constexpr int T = kHeadBlock<M>;
  const Row<M> c = load<M>(cvec, L);
  for (int n = M::clip(T); n < B; n += gridDim.x * M::clips(T)) {
    const Row<M> p = load<M>(zh + (size_t)n * L, L);
    const float d = poincare_dist<M>(c, p, nullptr);
    if (M::first()) score[n] = d;
  }
}

// logmap0(y) = y / |y| * artanh(|y|) at curvature -1 (hyper_math.py:367-370: norm clamp 1e-5, artanh on the clamped argument)
template <class M>
__global__ __launch_bounds__(kHeadBlock<M>) void k_poincare_logmap0(const float* __restrict__ y, float* __restrict__ out, int B, int L) {
  constexpr int T = kHeadBlock<M>;
  for (int n = M::clip(T); n < B; n += gridDim.x * M::clips(T)) {
    const Row<M> p = load<M>(y + (size_t)n * L, L);
    const float yn = fmaxf(sqrtf(dot(p, p)), kMinNorm);
    const float yc = fminf(fmaxf(yn, -1.f + kArtanhEps), 1.f - kArtanhEps);
    const float at = 0.5f * (log1pf(yc) - log1pf(-yc));
    Row<M> o;
#pragma unroll
    for (int i = 0; i < M::NE; ++i) o.v[i] = p.v[i] / yn * at;
    store(out + (size_t)n * L, o, L);
  }
}

// Gyromidpoint from the running sums: m = S / s ; centre = (1/2) (x) m  (Mobius scalar mul)
//   acc: head slot layout, [1..L] = sum gamma*zh, [Lp+1] = sum (gamma-1)
__global__ void k_midpoint_finalize(const float* __restrict__ acc, float* __restrict__ cvec, int L) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double s = fmax((double)acc[head_lp(L) + 1], 1e-10);
  double mn2 = 0.0;
  for (int j = 0; j < L; ++j) {
    const double m = (double)acc[1 + j] / s;
    mn2 += m * m;
  }
  const double mn = fmax(sqrt(mn2), 1e-15);
  const double mc = fmin(mn, 1.0 - 1e-7);
  const double at = 0.5 * log((1.0 + mc) / (1.0 - mc));
  const double sc = tanh(0.5 * at) / mn;
  for (int j = 0; j < L; ++j) cvec[j] = (float)(sc * ((double)acc[1 + j] / s));
}

// Euclidean centre: c = S / n (n = acc[Lp+1]), then |c| < eps -> +-eps  (staticCenter.py:118-121); a thread per latent
__global__ void k_center_finalize(const float* __restrict__ acc, float eps, float* __restrict__ cvec, int L) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= L) return;
  float c = acc[1 + j] / acc[head_lp(L) + 1];
  if (fabsf(c) < eps && c < 0.f) c = -eps;
  if (fabsf(c) < eps && c > 0.f) c = eps;
  cvec[j] = c;
}

// The launches behind a head's row kernel: the map's grid in front, the partial rows' sum behind (PerThread: none when the one
// block wrote the statistics itself).
static int head_grid(int B, int L) { return L > LMAX ? wide_head_blocks(B) : head_blocks(B); }
static void head_finalize(const float* ws, int P, int L, float scale0, float* stats, float* acc, hipStream_t stream) {
  if (L > LMAX) wide_head_finalize(ws, P, L, scale0, stats, acc, stream);
  else if ((stats || acc) && P > 1) hipLaunchKernelGGL(k_head_finalize, dim3(1), dim3(64), 0, stream, ws, P, scale0, stats, acc);
}

// ---- regulariser + Adam on flat buffers -------------------------------------------------
// partials[b] = sum over this block's slice of mask[i] * p[i]^2
__global__ __launch_bounds__(256) void k_sqnorm_masked(const float* __restrict__ p,
                                                        const float* __restrict__ mask, size_t n,
                                                        float* __restrict__ partials) {
  __shared__ float sh[4];
  float s = 0.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float v = p[i];
    s = fmaf(mask ? mask[i] * v : v, v, s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// torch.optim.Adam (no amsgrad, weight_decay 0) on flat fp32 buffers, with the regulariser's
// gradient folded in: g = grad * gscale + reg_coef * mask * p.
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g,
                                               float* __restrict__ m, float* __restrict__ v,
                                               const float* __restrict__ mask, size_t n, float lr,
                                               float beta1, float beta2, float eps, float bc1,
                                               float bc2_sqrt, float gscale, float reg_coef) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float pi = p[i];
  float gi = g[i] * gscale;
  if (reg_coef != 0.f) gi = fmaf(reg_coef * (mask ? mask[i] : 1.f), pi, gi);
  const float mi = beta1 * m[i] + (1.f - beta1) * gi;
  const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = pi - (lr / bc1) * (mi / denom);
}

// hyper[0] = lr, hyper[1] = beta1^t, hyper[2] = beta2^t  (device-resident so a captured hipGraph can be
// replayed: the step count advances in memory, not in kernel arguments)
__global__ void k_adam_tick(float* __restrict__ hyper, float beta1, float beta2) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    hyper[1] *= beta1;
    hyper[2] *= beta2;
  }
}
// the one launch of it: the Adam entry points that keep beta^t in device memory share this tick (csrc/grad_clip.hip's too), so the
// eager and the captured pairs multiply up the same way
void launch_adam_tick(float* hyper, float beta1, float beta2, hipStream_t stream) {
  hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(64), 0, stream, hyper, beta1, beta2);
}

__global__ __launch_bounds__(256) void k_adam_dev(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v,
                                                   const float* __restrict__ mask, size_t n,
                                                   const float* __restrict__ hyper, float beta1, float beta2,
                                                   float eps, float gscale, float reg_coef) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float lr = hyper[0], bc1 = 1.f - hyper[1], bc2s = sqrtf(1.f - hyper[2]);
  const float pi = p[i];
  float gi = g[i] * gscale;
  if (reg_coef != 0.f) gi = fmaf(reg_coef * (mask ? mask[i] : 1.f), pi, gi);
  const float mi = beta1 * m[i] + (1.f - beta1) * gi;
  const float vi = beta2 * v[i] + (1.f - beta2) * gi * gi;
  m[i] = mi;
  v[i] = vi;
  p[i] = pi - (lr / bc1) * (mi / (sqrtf(vi) / bc2s + eps));
}

__global__ __launch_bounds__(256) void k_scale_sum(const float* __restrict__ v, int n, float scale,
                                                    float* __restrict__ out) {
  __shared__ double sh[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)(sh[0] * (double)scale);
}

}  // namespace coskad

using namespace coskad;

extern "C" {

int coskad_head_slots(void) { return kHeadSlots; }
size_t coskad_head_ws_floats(int B) { return (size_t)ceil_div(B, kFlatBlock) * kHeadSlots; }
int coskad_head_slots_l(int L) { return L > 0 && L <= kWideLMax ? head_slots_for(L) : 0; }
size_t coskad_head_ws_floats_l(int B, int L) {
  if (L > LMAX && L <= kWideLMax) return (size_t)wide_head_blocks(B > 0 ? B : 1) * (size_t)head_slots_for(L);
  return coskad_head_ws_floats(B);
}

/* Euclidean one-class head on z [B,L] (staticCenter.py:187, dynamicCenter.py:116, eval_utils.py:63-64).
 *   stats: [0] = mean_{n,j} (z-c)^2 (the loss), [1..L] = sum_n z, [Lp+1] = B, [Lp+2] = sum_n |z_n|   (Lp = max(L, 16))
 *   acc  : += the raw sums (running centre accumulation, staticCenter.py:172-178); NULL to skip
 *   dz   : upstream * d loss / dz, NULL to skip;  score[n] = mean_j (c - z_n)^2, NULL to skip */
int coskad_mse_head_f32(const float* z, const float* c, float* dz, float* score, float* stats, float* acc,
                        float upstream, float* ws, int B, int L, hipStream_t stream) {
  if (!z || !c || !ws) return fail(COSKAD_ERR_ARG, "mse_head: null pointer");
  if (B <= 0 || L <= 0 || L > kWideLMax) return fail(COSKAD_ERR_SHAPE, "mse_head: B=%d latent=%d (max %d)", B, L, kWideLMax);
  const int P = head_grid(B, L);
  const float scale0 = 1.f / ((float)B * (float)L);
  by_width(L, [&](auto m) {
    using M = decltype(m);
    hipLaunchKernelGGL(k_mse_head<M>, dim3(P), dim3(kHeadBlock<M>), 0, stream, z, c, dz, score, B, L,
                       upstream / ((float)B * (float)L), HeadOut{ws, scale0, stats, acc});
  });
  head_finalize(ws, P, L, scale0, stats, acc, stream);
  return check_launch(L > LMAX ? "mse_head (wide)" : "mse_head");
}

/* Mahalanobis one-class head: loss = mean_n sqrt((z_n-c)^T VI (z_n-c)) (utils/eval_utils.py:28-38 as called at
 * euclidean_encoder_staticCenter.py:181), gradient, per-window score (eval_utils.py:41-47), centre sums as in the
 * MSE head, and optionally gram (+)= sum_n z_n z_n^T (the second moments behind compute_inv_cov_mat, :133-142). */
int coskad_mahalanobis_head_f32(const float* z, const float* c, const float* VI, float* dz, float* score,
                                float* stats, float* acc, float* gram, int gram_accumulate, float upstream,
                                float* ws, int B, int L, hipStream_t stream) {
  if (!z || !c || !VI || !ws) return fail(COSKAD_ERR_ARG, "mahalanobis_head: null pointer");
  if (B <= 0 || L <= 0 || L > kWideLMax) return fail(COSKAD_ERR_SHAPE, "mahalanobis_head: B=%d latent=%d (max %d)", B, L, kWideLMax);
  if (L > LMAX) return wide_mahalanobis_head(z, c, VI, dz, score, stats, acc, gram, gram_accumulate, upstream, ws, B, L, stream);
  const int P = head_blocks(B);
  hipLaunchKernelGGL(k_mahalanobis_head, dim3(P), dim3(kFlatBlock), 0, stream, z, c, VI, dz, score, B, L, upstream / (float)B,
                     HeadOut{ws, 1.f / (float)B, stats, acc});
  head_finalize(ws, P, L, 1.f / (float)B, stats, acc, stream);
  if (gram) hipLaunchKernelGGL(k_gram, dim3(1), dim3(LMAX * LMAX), 0, stream, z, gram, B, L, gram_accumulate);
  return check_launch("mahalanobis_head");
}

/* Poincare one-class head (hyperbolic_encoder.py:147,157; utils/hyper_math.py formulas):
 *   zh = project(expmap0(z)) ; loss = mean_n dist(c, zh_n)
 *   stats: [0] = loss, [1..L] = sum gamma*zh, [Lp+1] = sum (gamma-1), [Lp+2] = sum |zh|   (gamma = 2/(1-|zh|^2))
 *   acc  : += raw sums (gyromidpoint accumulation replacing the reference's torch.cat, :148-153)
 *   c == NULL: embedding + midpoint sums only (centre initialisation, :110-122). */
int coskad_poincare_head_f32(const float* z, const float* c, float* dz, float* zh, float* score,
                             float* stats, float* acc, float upstream, float* ws, int B, int L,
                             hipStream_t stream) {
  if (!z || !ws) return fail(COSKAD_ERR_ARG, "poincare_head: null pointer");
  if (B <= 0 || L <= 0 || L > kWideLMax) return fail(COSKAD_ERR_SHAPE, "poincare_head: B=%d latent=%d (max %d)", B, L, kWideLMax);
  const int P = head_grid(B, L);
  by_width(L, [&](auto m) {
    using M = decltype(m);
    hipLaunchKernelGGL(k_poincare_head<M>, dim3(P), dim3(kHeadBlock<M>), 0, stream, z, c, dz, zh, score, B, L, upstream / (float)B,
                       HeadOut{ws, 1.f / (float)B, stats, acc});
  });
  head_finalize(ws, P, L, 1.f / (float)B, stats, acc, stream);
  return check_launch(L > LMAX ? "poincare_head (wide)" : "poincare_head");
}

/* score[n] = dist(c, zh_n) for points already on the ball (eval_utils.py:66-67). */
int coskad_poincare_dist_f32(const float* zh, const float* c, float* score, int B, int L, hipStream_t stream) {
  if (!zh || !c || !score) return fail(COSKAD_ERR_ARG, "poincare_dist: null pointer");
  if (B <= 0 || L <= 0 || L > kWideLMax) return fail(COSKAD_ERR_SHAPE, "poincare_dist: B=%d latent=%d (max %d)", B, L, kWideLMax);
  const int grid = L > LMAX ? wide_head_blocks(B) : ceil_div(B, kFlatBlock);
  by_width(L, [&](auto m) {
    using M = decltype(m);
    hipLaunchKernelGGL(k_poincare_dist<M>, dim3(grid), dim3(kHeadBlock<M>), 0, stream, zh, c, score, B, L);
  });
  return check_launch(L > LMAX ? "poincare_dist (wide)" : "poincare_dist");
}

int coskad_poincare_logmap0_f32(const float* y, float* out, int B, int L, hipStream_t stream) {
  if (!y || !out) return fail(COSKAD_ERR_ARG, "poincare_logmap0: null pointer");
  if (B <= 0 || L <= 0 || L > kWideLMax) return fail(COSKAD_ERR_SHAPE, "poincare_logmap0: B=%d latent=%d (max %d)", B, L, kWideLMax);
  const int grid = L > LMAX ? wide_head_blocks(B) : ceil_div(B, kFlatBlock);
  by_width(L, [&](auto m) {
    using M = decltype(m);
    hipLaunchKernelGGL(k_poincare_logmap0<M>, dim3(grid), dim3(kHeadBlock<M>), 0, stream, y, out, B, L);
  });
  return check_launch(L > LMAX ? "poincare_logmap0 (wide)" : "poincare_logmap0");
}

/* Euclidean centre from accumulated sums (acc layout of coskad_mse_head_f32): c = S/n with n = acc[Lp+1],
 * then |c| < eps -> +-eps (staticCenter.py:118-121). */
int coskad_center_finalize_f32(const float* acc, float* c, float eps, int L, hipStream_t stream) {
  if (!acc || !c || L <= 0 || L > kWideLMax) return fail(COSKAD_ERR_ARG, "center_finalize: bad argument (latent=%d, max %d)", L, kWideLMax);
  const int threads = L > LMAX ? kWideBlock : 64;
  hipLaunchKernelGGL(k_center_finalize, dim3(ceil_div(L, threads)), dim3(threads), 0, stream, acc, eps, c, L);
  return check_launch(L > LMAX ? "center_finalize (wide)" : "center_finalize");
}

/* Gyromidpoint (geoopt weighted_midpoint with unit weights; hyperbolic_encoder.py:122,179) from the
 * sums accumulated by coskad_poincare_head_f32. */
int coskad_midpoint_finalize_f32(const float* acc, float* c, int L, hipStream_t stream) {
  if (!acc || !c || L <= 0 || L > kWideLMax) return fail(COSKAD_ERR_ARG, "midpoint_finalize: bad argument (latent=%d, max %d)", L, kWideLMax);
  hipLaunchKernelGGL(k_midpoint_finalize, dim3(1), dim3(64), 0, stream, acc, c, L);
  return check_launch(L > LMAX ? "midpoint_finalize (wide)" : "midpoint_finalize");
}

/* out[0] = scale * sum_i mask[i] * p[i]^2   (calc_reg_loss: scale = 0.5 / #non-bias tensors;
 * utils/model_utils.py:90-105).  mask NULL = all ones.  ws: >= 256 floats. */
int coskad_sqnorm_f32(const float* p, const float* mask, size_t n, float scale, float* out, float* ws,
                      hipStream_t stream) {
  if (!p || !out || !ws || n == 0) return fail(COSKAD_ERR_ARG, "sqnorm: bad argument");
  const int grid = (int)((n + 255) / 256 < 256 ? (n + 255) / 256 : 256);
  hipLaunchKernelGGL(k_sqnorm_masked, dim3(grid), dim3(256), 0, stream, p, mask, n, ws);
  hipLaunchKernelGGL(k_scale_sum, dim3(1), dim3(256), 0, stream, ws, grid, scale, out);
  return check_launch("sqnorm");
}

/* torch.optim.Adam step (amsgrad off, weight_decay 0) on flat buffers, with the regulariser gradient
 * folded in: g = grad * gscale + reg_coef * mask * p.  `step` is the 1-based step count. */
int coskad_adam_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float lr,
                    float beta1, float beta2, float eps, int step, float gscale, float reg_coef,
                    hipStream_t stream) {
  if (!p || !g || !m || !v || n == 0 || step < 1) return fail(COSKAD_ERR_ARG, "adam: bad argument");
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, g, m, v, mask, n, lr,
                     beta1, beta2, eps, (float)bc1, (float)sqrt(bc2), gscale, reg_coef);
  return check_launch("adam");
}

/* Same update with the caller's running products b1pow = beta1^t, b2pow = beta2^t (fp32, multiplied up step by step: the arithmetic
 * of coskad_adam_dev_f32's device-side tick, so that an eager step and a hipGraph-captured one agree bit for bit). */
int coskad_adam_pow_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float lr, float beta1,
                        float beta2, float eps, float b1pow, float b2pow, float gscale, float reg_coef, hipStream_t stream) {
  if (!p || !g || !m || !v || n == 0) return fail(COSKAD_ERR_ARG, "adam_pow: bad argument");
  if (!(b1pow < 1.f) || !(b2pow < 1.f)) return fail(COSKAD_ERR_ARG, "adam_pow: beta^t must be < 1 (t >= 1)");
  hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, g, m, v, mask, n, lr,
                     beta1, beta2, eps, 1.f - b1pow, sqrtf(1.f - b2pow), gscale, reg_coef);
  return check_launch("adam_pow");
}

/* Same update with lr / beta^t read from device memory: hyper = {lr, beta1^t, beta2^t} (initialise to
 * {lr, 1, 1}); every call first advances beta^t, so the call is replayable inside a hipGraph. */
int coskad_adam_dev_f32(float* p, const float* g, float* m, float* v, const float* mask, size_t n, float* hyper,
                        float beta1, float beta2, float eps, float gscale, float reg_coef, hipStream_t stream) {
  if (!p || !g || !m || !v || !hyper || n == 0) return fail(COSKAD_ERR_ARG, "adam_dev: bad argument");
  launch_adam_tick(hyper, beta1, beta2, stream);
  hipLaunchKernelGGL(k_adam_dev, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, g, m, v, mask, n, hyper,
                     beta1, beta2, eps, gscale, reg_coef);
  return check_launch("adam_dev");
}

}  // extern "C"
