// Frame-level scoring on the device: per-window scores -> per-person frame means -> absence padding -> max over a clip's persons ->
// shift + Gaussian smoothing -> mean over transformations -> AUC (eval_COSKAD.py:140-253, utils/eval_utils.py:200-248 of the reference,
// as restated in oracle/ref_scoring.py).  Everything that depends only on the window table -- which windows cover which frame of which
// person, which persons belong to which clip, where a clip's frames land in the concatenated vector -- comes precomputed from
// coskad_amd.utils.score_plan.ScorePlan; these kernels only read its index tables.  fp64 throughout, no floating-point atomics, one
// fixed summation order per output: two runs agree bit for bit.  The library is built with -ffp-contract=off, so every product and sum
// below rounds where numpy / scipy round theirs.
#include "common.h"

namespace coskad {

constexpr int kScoreBlock = 256;
constexpr int kSmoothRadius = 120;                    // int(4.0 * 30 + 0.5): gaussian_filter1d(sigma = 30)
constexpr int kSmoothTaps = kSmoothRadius + 1;        // centre + one side of the symmetric filter
constexpr int kSmoothShift = 11;                      // 8 + 8 // 2 - 1 (score_process)
constexpr int kPadRowMax = 8192;                      // frames of one person's row in LDS (64 KB of doubles)

// one thread = one (person, frame): mean of the covering windows whose score is not exactly 0, in ascending window order
template <typename S>
__global__ __launch_bounds__(kScoreBlock) void k_score_person_frames(const S* __restrict__ scores, const int* __restrict__ win_ptr,
                                                                    const int* __restrict__ win_idx, double* __restrict__ pf,
                                                                    int n_scores, int n_rows) {
  const int e = blockIdx.x * kScoreBlock + threadIdx.x;
  if (e >= n_rows) return;
  const int k0 = win_ptr[e], k1 = win_ptr[e + 1];
  double sum = 0.0;
  int cnt = 0;
  for (int k = k0; k < k1; ++k) {
    const int w = win_idx[k];
    if ((unsigned)w >= (unsigned)n_scores) continue;   // a table that does not belong to these scores: never read out of bounds
    const double s = (double)scores[w];
    if (s != 0.0) { sum += s; ++cnt; }
  }
  pf[e] = cnt > 0 ? sum / (double)cnt : 0.0;
}

// one workgroup = one person's row, held in LDS while the zeros are stored: pad_scores branch for branch.  A thread that owns the first
// frame of an absence run walks to its end and zeroes [lo, hi); runs are found on the LDS copy, so no store changes what another
// thread reads, and all stores write the same value.
__global__ __launch_bounds__(kScoreBlock) void k_score_pad(double* __restrict__ pf, const int* __restrict__ row_ptr, int pad, int n_max) {
  extern __shared__ double row[];
  const int p = blockIdx.x;
  const int r0 = row_ptr[p], n = row_ptr[p + 1] - r0;
  if (n < 2 || n > n_max) return;                      // uniform per block
  double* g = pf + r0;
  for (int i = threadIdx.x; i < n; i += kScoreBlock) row[i] = g[i];
  __syncthreads();
  const int last = n - 2;                              // absence is looked for among frames 0 .. n-2 only
  for (int a = threadIdx.x; a <= last; a += kScoreBlock) {
    if (row[a] != 0.0 || (a > 0 && row[a - 1] == 0.0)) continue;
    int b = a;
    while (b < last && row[b + 1] == 0.0) ++b;
    if (a == 0 && b == last) continue;                 // absent throughout: left alone
    const int lo = a == 0 ? 0 : max(a - pad, 0);
    const int hi = (b == last && a != 0) ? b : min(b + pad, n);
    for (int i = lo; i < hi; ++i) g[i] = 0.0;
  }
}

// one thread = one (transformation, output position): max over the clip's persons of the source frame, written straight into the
// concatenated (human-related-compacted) layout; a clip without persons scores 0
__global__ __launch_bounds__(kScoreBlock) void k_score_clip_max(const double* __restrict__ pf, const int* __restrict__ row_ptr,
                                                               const int* __restrict__ pc_ptr, const int* __restrict__ out_clip,
                                                               const int* __restrict__ out_frame, double* __restrict__ raw,
                                                               int n_clips, int F) {
  const int o = blockIdx.x * kScoreBlock + threadIdx.x;
  const int t = blockIdx.y;
  if (o >= F) return;
  const int c = out_clip[o], f = out_frame[o];
  double m = 0.0;
  if ((unsigned)c < (unsigned)n_clips) {
    const int p0 = pc_ptr[t * n_clips + c], p1 = pc_ptr[t * n_clips + c + 1];
    bool any = false;
    for (int p = p0; p < p1; ++p) {
      const int r0 = row_ptr[p];
      if ((unsigned)f >= (unsigned)(row_ptr[p + 1] - r0)) continue;
      const double v = pf[r0 + f];
      m = (!any || v > m) ? v : m;
      any = true;
    }
  }
  raw[(size_t)t * F + o] = m;
}

// one workgroup = one tile of kScoreBlock outputs of one clip segment, every transformation in turn: the shifted scores of the tile and
// a 120-element halo on both sides go to LDS through scipy's `reflect` boundary (d c b a | a b c d | d c b a: period 2m, so a segment
// shorter than the halo reflects several times), then each thread accumulates as scipy's correlate1d does for a symmetric filter:
// centre tap first, then (x[c-k] + x[c+k]) * w[k] for k = 120 .. 1.  Consecutive lanes read consecutive doubles (distinct banks for
// ds_read_b64); the taps are addressed uniformly and come through the scalar cache.
__global__ __launch_bounds__(kScoreBlock) void k_score_smooth(const double* __restrict__ raw, const int* __restrict__ tiles,
                                                             const double* __restrict__ taps, double* __restrict__ per_t,
                                                             double* __restrict__ mean, int n_transform, int F) {
  __shared__ double x[kScoreBlock + 2 * kSmoothRadius];
  const int seg0 = tiles[3 * blockIdx.x], seg1 = tiles[3 * blockIdx.x + 1], tile0 = tiles[3 * blockIdx.x + 2];
  const int m = seg1 - seg0;
  if (m <= 0 || seg0 < 0 || seg1 > F || tile0 < seg0 || tile0 >= seg1) return;   // uniform per block
  const int o = tile0 + threadIdx.x;
  const bool live = o < seg1;
  double acc_t = 0.0;
  for (int t = 0; t < n_transform; ++t) {
    const double* r = raw + (size_t)t * F + seg0;
    for (int li = threadIdx.x; li < kScoreBlock + 2 * kSmoothRadius; li += kScoreBlock) {
      int j = (tile0 - seg0 - kSmoothRadius + li) % (2 * m);
      if (j < 0) j += 2 * m;
      if (j >= m) j = 2 * m - 1 - j;
      x[li] = j >= kSmoothShift ? r[j - kSmoothShift] : 0.0;        // shifted[i] = raw[i - 11] for i >= 11, else 0
    }
    __syncthreads();
    if (live) {
      const int c = threadIdx.x + kSmoothRadius;
      double acc = x[c] * taps[0];
      for (int k = kSmoothRadius; k >= 1; --k) acc += (x[c - k] + x[c + k]) * taps[k];
      per_t[(size_t)t * F + o] = acc;
      acc_t += acc;
    }
    __syncthreads();
  }
  if (live) mean[o] = acc_t / (double)n_transform;
}

// 2U = sum over groups of equal score of pos_g (2 neg_below_g + neg_g), one positive at a time: a positive of group g adds
// neg_below_g + (neg_below_g + neg_g) = cum_neg[first of g - 1] + cum_neg[last of g], both found by bisection in the sorted scores.
// int64 sums: exact and independent of their order.  ws[block] receives the block's sum.
__global__ __launch_bounds__(kScoreBlock) void k_score_auc_partial(const double* __restrict__ s, const int* __restrict__ gt,
                                                                  const long long* __restrict__ cum_neg, long long* __restrict__ ws,
                                                                  int F) {
  __shared__ long long red[kScoreBlock];
  const int i = blockIdx.x * kScoreBlock + threadIdx.x;
  long long u = 0;
  if (i < F && gt[i] != 0) {
    const double v = s[i];
    int lo = 0, hi = i;                                 // first index whose score is not below v
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s[mid] < v) lo = mid + 1; else hi = mid;
    }
    const int first = lo;
    lo = i + 1; hi = F;                                 // first index whose score is above v
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s[mid] > v) hi = mid; else lo = mid + 1;
    }
    u = (first > 0 ? cum_neg[first - 1] : 0) + cum_neg[lo - 1];
  }
  red[threadIdx.x] = u;
  __syncthreads();
  for (int w = kScoreBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[blockIdx.x] = red[0];
}

// out = {AUC = 2U / (2 n_pos n_neg), n_pos, n_neg}; AUC is NaN for a single-class ground truth (the caller raises)
__global__ __launch_bounds__(kScoreBlock) void k_score_auc_final(const long long* __restrict__ ws, int n_ws,
                                                                const long long* __restrict__ cum_neg, double* __restrict__ out, int F) {
  __shared__ long long red[kScoreBlock];
  long long u = 0;
  for (int b = threadIdx.x; b < n_ws; b += kScoreBlock) u += ws[b];
  red[threadIdx.x] = u;
  __syncthreads();
  for (int w = kScoreBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const long long n_neg = cum_neg[F - 1], n_pos = (long long)F - n_neg;
    const double den = 2.0 * (double)n_pos * (double)n_neg;
    out[0] = (n_pos > 0 && n_neg > 0) ? (double)red[0] / den : __builtin_nan("");
    out[1] = (double)n_pos;
    out[2] = (double)n_neg;
  }
}

}  // namespace coskad

using namespace coskad;

extern "C" {

int coskad_score_pad_row_max(void) { return kPadRowMax; }
int coskad_score_tile(void) { return kScoreBlock; }
int coskad_score_auc_ws(int F) { return F > 0 ? ceil_div(F, kScoreBlock) : 0; }

int coskad_score_person_frames_f64(const void* scores, int scores_f64, const int* win_ptr, const int* win_idx, double* pf,
                                   int n_scores, int n_rows, hipStream_t stream) {
  if (!scores || !win_ptr || !win_idx || !pf) return fail(COSKAD_ERR_ARG, "score_person_frames: null pointer");
  if (n_scores <= 0 || n_rows <= 0) return fail(COSKAD_ERR_ARG, "score_person_frames: n_scores=%d n_rows=%d", n_scores, n_rows);
  const dim3 grid((unsigned)ceil_div(n_rows, kScoreBlock));
  if (scores_f64)
    hipLaunchKernelGGL(k_score_person_frames<double>, grid, dim3(kScoreBlock), 0, stream, (const double*)scores, win_ptr, win_idx, pf,
                       n_scores, n_rows);
  else
    hipLaunchKernelGGL(k_score_person_frames<float>, grid, dim3(kScoreBlock), 0, stream, (const float*)scores, win_ptr, win_idx, pf,
                       n_scores, n_rows);
  return check_launch("score_person_frames");
}

int coskad_score_pad_f64(double* pf, const int* row_ptr, int n_persons, int pad_size, int n_max, hipStream_t stream) {
  if (!pf || !row_ptr) return fail(COSKAD_ERR_ARG, "score_pad: null pointer");
  if (n_persons <= 0 || n_max <= 0) return fail(COSKAD_ERR_ARG, "score_pad: n_persons=%d n_max=%d", n_persons, n_max);
  if (n_max > kPadRowMax)
    return fail(COSKAD_ERR_SHAPE, "score_pad: unsupported clip length %d: a person's row of more than %d frames does not fit the kernel's LDS",
                n_max, kPadRowMax);
  hipLaunchKernelGGL(k_score_pad, dim3((unsigned)n_persons), dim3(kScoreBlock), (size_t)n_max * sizeof(double), stream, pf, row_ptr,
                     pad_size, n_max);
  return check_launch("score_pad");
}

int coskad_score_clip_max_f64(const double* pf, const int* row_ptr, const int* pc_ptr, const int* out_clip, const int* out_frame,
                              double* raw, int n_clips, int n_transform, int F, hipStream_t stream) {
  if (!pf || !row_ptr || !pc_ptr || !out_clip || !out_frame || !raw) return fail(COSKAD_ERR_ARG, "score_clip_max: null pointer");
  if (n_clips <= 0 || n_transform <= 0 || F <= 0 || n_transform > 65535)
    return fail(COSKAD_ERR_ARG, "score_clip_max: n_clips=%d n_transform=%d F=%d", n_clips, n_transform, F);
  hipLaunchKernelGGL(k_score_clip_max, dim3((unsigned)ceil_div(F, kScoreBlock), (unsigned)n_transform), dim3(kScoreBlock), 0, stream, pf,
                     row_ptr, pc_ptr, out_clip, out_frame, raw, n_clips, F);
  return check_launch("score_clip_max");
}

int coskad_score_smooth_f64(const double* raw, const int* tiles, const double* taps, int n_taps, double* per_t, double* mean,
                            int n_tiles, int n_transform, int F, hipStream_t stream) {
  if (!raw || !tiles || !taps || !per_t || !mean) return fail(COSKAD_ERR_ARG, "score_smooth: null pointer");
  if (n_tiles <= 0 || n_transform <= 0 || F <= 0)
    return fail(COSKAD_ERR_ARG, "score_smooth: n_tiles=%d n_transform=%d F=%d", n_tiles, n_transform, F);
  if (n_taps != kSmoothTaps)
    return fail(COSKAD_ERR_SHAPE, "score_smooth: unsupported tap table of %d entries: the filter has %d taps (centre + radius %d)", n_taps,
                kSmoothTaps, kSmoothRadius);
  hipLaunchKernelGGL(k_score_smooth, dim3((unsigned)n_tiles), dim3(kScoreBlock), 0, stream, raw, tiles, taps, per_t, mean, n_transform, F);
  return check_launch("score_smooth");
}

int coskad_score_auc_f64(const double* sorted_scores, const int* gt_sorted, const long long* cum_neg, double* out, long long* ws,
                         size_t ws_elems, int F, hipStream_t stream) {
  if (!sorted_scores || !gt_sorted || !cum_neg || !out || !ws) return fail(COSKAD_ERR_ARG, "score_auc: null pointer");
  if (F <= 0) return fail(COSKAD_ERR_ARG, "score_auc: F=%d", F);
  const int blocks = ceil_div(F, kScoreBlock);
  if (ws_elems < (size_t)blocks) return fail(COSKAD_ERR_WORKSPACE, "score_auc: workspace of %zu elements, %d needed", ws_elems, blocks);
  hipLaunchKernelGGL(k_score_auc_partial, dim3((unsigned)blocks), dim3(kScoreBlock), 0, stream, sorted_scores, gt_sorted, cum_neg, ws, F);
  hipLaunchKernelGGL(k_score_auc_final, dim3(1), dim3(kScoreBlock), 0, stream, ws, blocks, cum_neg, out, F);
  return check_launch("score_auc");
}

}  // extern "C"
