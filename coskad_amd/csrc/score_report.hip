// The evaluation report on the device (eval_COSKAD.py:222-242, utils/eval_utils.py:216-230 of the reference): the ROC-AUC of every
// clip segment of every score row, and per row the thresholds at which its ROC curve crosses tpr = 1 - fpr.  The rows are the
// per-transformation frame scores and their mean as csrc/score_frames.hip leaves them; ordering (each row sorted inside every segment,
// the ground truth in that order, its inclusive count of negatives along the row) is the caller's plumbing, as for coskad_score_auc_f64.
// One launch covers every (row, segment): the grid is a list of 256-element tiles of the segments, so the number of launches does not
// depend on the number of clips.  Counts are int64 / int32 and exact, comparisons are fp64, there are no floating-point atomics and
// every output has one fixed order: two runs agree bit for bit.  -ffp-contract=off: the quotients round where numpy rounds them.
#include "common.h"

namespace coskad {

constexpr int kReportBlock = 256;
constexpr int kReportNone = 0x7fffffff;

__device__ inline long long report_block_sum(long long u, long long* red) {
  red[threadIdx.x] = u;
  __syncthreads();
  for (int w = kReportBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  return red[0];
}

__device__ inline int report_block_min(int u, int* red) {
  red[threadIdx.x] = u;
  __syncthreads();
  for (int w = kReportBlock / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  return red[0];
}

// one workgroup = one tile of one segment [a, b) of one row; tile_ptr[c] .. tile_ptr[c + 1] are segment c's tiles.  Per positive the
// term of k_score_auc_partial (csrc/score_frames.hip), with the bisections and the counts confined to the segment:
// 2U = sum over positives of neg_below + (neg_below + neg_equal).  ws[row, tile] receives the tile's sum; a tile beyond the list, or of
// a segment that does not lie in [0, F], contributes 0 and reads nothing.
__global__ __launch_bounds__(kReportBlock) void k_report_auc_partial(const double* __restrict__ s, const int* __restrict__ gt,
                                                                    const long long* __restrict__ cum_neg,
                                                                    const int* __restrict__ segments, const int* __restrict__ tile_ptr,
                                                                    long long* __restrict__ ws, int n_seg, int n_tiles, int F) {
  __shared__ long long red[kReportBlock];
  const int tile = blockIdx.x, row = blockIdx.y;
  int lo = 1, hi = n_seg + 1;                             // first j in 1 .. n_seg with tile_ptr[j] > tile (n_seg + 1: none)
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tile_ptr[mid] > tile) hi = mid; else lo = mid + 1;
  }
  long long u = 0;
  if (lo <= n_seg) {                                      // uniform per block
    const int c = lo - 1;
    const int a = segments[2 * c], b = segments[2 * c + 1];
    const long long k = (long long)tile - tile_ptr[c];
    const long long at = (long long)a + k * kReportBlock + threadIdx.x;
    if (a >= 0 && a <= b && b <= F && k >= 0 && at < b) {
      const int i = (int)at;
      const double* sr = s + (size_t)row * F;
      const long long* cn = cum_neg + (size_t)row * F;
      if (gt[(size_t)row * F + i] != 0) {
        const double v = sr[i];
        int l = a, h = i;                                 // first index of the segment whose score is not below v
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (sr[mid] < v) l = mid + 1; else h = mid;
        }
        const int first = l;
        l = i + 1; h = b;                                 // first index of the segment whose score is above v
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (sr[mid] > v) h = mid; else l = mid + 1;
        }
        const long long base = a > 0 ? cn[a - 1] : 0;
        u = (first > a ? cn[first - 1] - base : 0) + (cn[l - 1] - base);
      }
    }
  }
  u = report_block_sum(u, red);
  if (threadIdx.x == 0) ws[(size_t)row * n_tiles + tile] = u;
}

// one workgroup = one (segment, row): out[row, c] = {AUC = 2U / (2 n_pos n_neg), n_pos, n_neg}, the quotient formed as
// k_score_auc_final forms it; AUC is NaN for a segment with one class or no frame, and {NaN, -1, -1} marks a segment outside [0, F] or
// a tile list that does not match it
__global__ __launch_bounds__(kReportBlock) void k_report_auc_final(const long long* __restrict__ ws,
                                                                  const long long* __restrict__ cum_neg,
                                                                  const int* __restrict__ segments, const int* __restrict__ tile_ptr,
                                                                  double* __restrict__ out, int n_seg, int n_tiles, int F) {
  __shared__ long long red[kReportBlock];
  const int c = blockIdx.x, row = blockIdx.y;
  const int a = segments[2 * c], b = segments[2 * c + 1];
  const int t0 = tile_ptr[c], t1 = tile_ptr[c + 1];
  const bool ok = a >= 0 && a <= b && b <= F && t0 >= 0 && t1 <= n_tiles && t1 - t0 == ceil_div(b - a, kReportBlock);   // uniform
  long long u = 0;
  if (ok)
    for (int t = t0 + threadIdx.x; t < t1; t += kReportBlock) u += ws[(size_t)row * n_tiles + t];
  u = report_block_sum(u, red);
  if (threadIdx.x == 0) {
    double* o = out + ((size_t)row * n_seg + c) * 3;
    if (!ok) {
      o[0] = __builtin_nan(""); o[1] = -1.0; o[2] = -1.0;
    } else {
      const long long* cn = cum_neg + (size_t)row * F;
      const long long n_neg = b > a ? cn[b - 1] - (a > 0 ? cn[a - 1] : 0) : 0, n_pos = (long long)(b - a) - n_neg;
      const double den = 2.0 * (double)n_pos * (double)n_neg;
      o[0] = (n_pos > 0 && n_neg > 0) ? (double)u / den : __builtin_nan("");
      o[1] = (double)n_pos;
      o[2] = (double)n_neg;
    }
  }
}

// roc_curve(drop_intermediate=True) and the crossing of tpr = 1 - fpr, one thread per element of a row sorted ascending.  A group of
// equal scores is one point of the curve (walked from the highest score down): fps = negatives at or above the score, tps likewise.
// roc_curve keeps the first point, the last, and every point where the second difference of fps or tps is non-zero -- that is, where
// the group's (negatives, positives) differ from those of the next lower group.  d = tpr - (1 - fpr) does not decrease along the curve,
// is -1 at the prepended (0, 0, inf) point and +1 at the last, so np.argwhere(np.diff(np.sign(d))) is: the last kept point with d < 0,
// and, when a kept point has d == 0, the last of those.  Along a row sorted ascending "last" is the lowest index; the thread that owns
// the first element of a kept group proposes its index, ws[row, block] = {min over d < 0, min over d == 0}.
__global__ __launch_bounds__(kReportBlock) void k_report_thr_partial(const double* __restrict__ s, const long long* __restrict__ cum_neg,
                                                                    int* __restrict__ ws, int F) {
  __shared__ int red[kReportBlock];
  const int i = blockIdx.x * kReportBlock + threadIdx.x, row = blockIdx.y;
  const double* sr = s + (size_t)row * F;
  const long long* cn = cum_neg + (size_t)row * F;
  const long long N = cn[F - 1], P = (long long)F - N;
  int neg_at = kReportNone, zero_at = kReportNone;
  if (i < F && P > 0 && N > 0) {
    const double v = sr[i];
    if (i == 0 || sr[i - 1] < v) {                        // the first element of its group
      int l = i + 1, h = F;                               // the group's end: first index whose score is above v
      while (l < h) {
        const int mid = (l + h) >> 1;
        if (sr[mid] > v) h = mid; else l = mid + 1;
      }
      const int e = l;
      const long long below = i > 0 ? cn[i - 1] : 0;      // negatives of lower score
      bool kept = i == 0 || e == F;
      if (!kept) {
        const long long neg_g = cn[e - 1] - below, pos_g = (long long)(e - i) - neg_g;
        const double w = sr[i - 1];
        l = 0; h = i - 1;                                 // the next lower group's start
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (sr[mid] < w) l = mid + 1; else h = mid;
        }
        const long long neg_l = below - (l > 0 ? cn[l - 1] : 0), pos_l = (long long)(i - l) - neg_l;
        kept = neg_l != neg_g || pos_l != pos_g;
      }
      if (kept) {
        const long long fps = N - below, tps = (long long)(F - i) - fps;
        const double d = (double)tps / (double)P - (1.0 - (double)fps / (double)N);
        if (d < 0.0) neg_at = i;
        else if (d == 0.0) zero_at = i;
      }
    }
  }
  neg_at = report_block_min(neg_at, red);
  __syncthreads();
  zero_at = report_block_min(zero_at, red);
  if (threadIdx.x == 0) {
    ws[((size_t)row * gridDim.x + blockIdx.x) * 2] = neg_at;
    ws[((size_t)row * gridDim.x + blockIdx.x) * 2 + 1] = zero_at;
  }
}

// out[row] = {n, thr0, thr1}: n = 1 or 2 thresholds (0 for a single-class row), thr0 = +inf when every point of the row has d >= 0
__global__ __launch_bounds__(kReportBlock) void k_report_thr_final(const double* __restrict__ s, const long long* __restrict__ cum_neg,
                                                                  const int* __restrict__ ws, int n_ws, double* __restrict__ out, int F) {
  __shared__ int red[kReportBlock];
  const int row = blockIdx.x;
  int neg_at = kReportNone, zero_at = kReportNone;
  for (int b = threadIdx.x; b < n_ws; b += kReportBlock) {
    neg_at = min(neg_at, ws[((size_t)row * n_ws + b) * 2]);
    zero_at = min(zero_at, ws[((size_t)row * n_ws + b) * 2 + 1]);
  }
  neg_at = report_block_min(neg_at, red);
  __syncthreads();
  zero_at = report_block_min(zero_at, red);
  if (threadIdx.x == 0) {
    const double* sr = s + (size_t)row * F;
    const long long N = cum_neg[(size_t)row * F + F - 1], P = (long long)F - N;
    double* o = out + (size_t)row * 3;
    const double nan = __builtin_nan("");
    if (P <= 0 || N <= 0) {
      o[0] = 0.0; o[1] = nan; o[2] = nan;
    } else {
      o[0] = zero_at != kReportNone ? 2.0 : 1.0;
      o[1] = (neg_at != kReportNone && neg_at < F) ? sr[neg_at] : __builtin_inf();
      o[2] = (zero_at != kReportNone && zero_at < F) ? sr[zero_at] : nan;
    }
  }
}

}  // namespace coskad

using namespace coskad;

extern "C" {

int coskad_score_report_tile(void) { return kReportBlock; }

long long coskad_score_report_auc_ws(int n_rows, int n_tiles) {
  return (n_rows > 0 && n_tiles > 0) ? (long long)n_rows * n_tiles : 0;
}

long long coskad_score_report_thr_ws(int n_rows, int F) {
  return (n_rows > 0 && F > 0) ? 2ll * n_rows * ceil_div(F, kReportBlock) : 0;
}

int coskad_score_report_auc_f64(const double* sorted_scores, const int* gt_sorted, const long long* cum_neg, const int* segments,
                                const int* tile_ptr, double* out, long long* ws, size_t ws_elems, int n_tiles, int n_rows, int n_seg,
                                int F, hipStream_t stream) {
  if (!sorted_scores || !gt_sorted || !cum_neg || !segments || !tile_ptr || !out || !ws)
    return fail(COSKAD_ERR_ARG, "score_report_auc: null pointer");
  if (n_rows <= 0 || n_seg <= 0 || F <= 0 || n_tiles <= 0 || n_rows > 65535)
    return fail(COSKAD_ERR_ARG, "score_report_auc: n_rows=%d n_seg=%d F=%d n_tiles=%d", n_rows, n_seg, F, n_tiles);
  if (n_tiles > F / kReportBlock + n_seg)
    return fail(COSKAD_ERR_ARG, "score_report_auc: %d tiles for %d segments that do not overlap in %d frames (at most %d)", n_tiles,
                n_seg, F, F / kReportBlock + n_seg);
  if (ws_elems < (size_t)n_rows * (size_t)n_tiles)
    return fail(COSKAD_ERR_WORKSPACE, "score_report_auc: workspace of %zu elements, %zu needed", ws_elems, (size_t)n_rows * (size_t)n_tiles);
  hipLaunchKernelGGL(k_report_auc_partial, dim3((unsigned)n_tiles, (unsigned)n_rows), dim3(kReportBlock), 0, stream, sorted_scores,
                     gt_sorted, cum_neg, segments, tile_ptr, ws, n_seg, n_tiles, F);
  hipLaunchKernelGGL(k_report_auc_final, dim3((unsigned)n_seg, (unsigned)n_rows), dim3(kReportBlock), 0, stream, ws, cum_neg, segments,
                     tile_ptr, out, n_seg, n_tiles, F);
  return check_launch("score_report_auc");
}

int coskad_score_report_thresholds_f64(const double* sorted_scores, const long long* cum_neg, double* out, int* ws, size_t ws_elems,
                                       int n_rows, int F, hipStream_t stream) {
  if (!sorted_scores || !cum_neg || !out || !ws) return fail(COSKAD_ERR_ARG, "score_report_thresholds: null pointer");
  if (n_rows <= 0 || F <= 0 || n_rows > 65535) return fail(COSKAD_ERR_ARG, "score_report_thresholds: n_rows=%d F=%d", n_rows, F);
  const int blocks = ceil_div(F, kReportBlock);
  if (ws_elems < 2 * (size_t)n_rows * (size_t)blocks)
    return fail(COSKAD_ERR_WORKSPACE, "score_report_thresholds: workspace of %zu elements, %zu needed", ws_elems,
                2 * (size_t)n_rows * (size_t)blocks);
  hipLaunchKernelGGL(k_report_thr_partial, dim3((unsigned)blocks, (unsigned)n_rows), dim3(kReportBlock), 0, stream, sorted_scores,
                     cum_neg, ws, F);
  hipLaunchKernelGGL(k_report_thr_final, dim3((unsigned)n_rows), dim3(kReportBlock), 0, stream, sorted_scores, cum_neg, ws, blocks, out,
                     F);
  return check_launch("score_report_thresholds");
}

}  // extern "C"
