// Online scoring (coskad_amd/stream.py): the offline pipeline's arithmetic one frame at a time.  A pose tracker hands in a few
// raw skeletons per frame; k_stream_push normalises each of them as utils/data.py does per frame (bounding-box centring, RobustScaler,
// joint layout: coskad_amd.utils.dataset.bbox_centre_coordinates / scale_robust / pose_layout), stores the row into the track's ring and,
// where the track has a full window, writes the window's K affine copies with the expression of k_gather_frames (data.hip).  After the
// model has scored those windows, k_stream_frames keeps the scores in a ring per track and finalises the one row that no later window
// can cover, by the rules of k_score_person_frames (score_frames.hip).  k_stream_close finalises a closed track's trailing rows.
// For many cameras per tick (StreamBank) k_stream_push_cams is the push kernel with the video resolution per detection, and
// k_stream_smooth hands out the shifted, Gaussian-smoothed clip scores of a flat clip buffer (one segment per camera) item by item, with
// k_score_smooth's arithmetic.  k_stream_maps / k_stream_maps_close do for per-joint window maps (attribution, reconstruction error)
// what k_stream_frames / k_stream_close do for the scores, with k_attribution_frames' arithmetic.
//
// Device state, capacity M tracks, R = (T - 1) step + 1 rows between a window's first and last row:
//   ring   [M, R, 2, V] f32 : row r of a track at slot r % R
//   count  [M] i32          : rows pushed per track
//   wscore [M, K, R] f64    : score of the window ENDING at row e at slot e % R
// One wave per detection: the row a wave writes and the window it assembles need no grid-wide ordering, and the track's slots of one
// launch are distinct (the launcher checks the host mirror), so no two waves touch the same state.  Every store is a vector store.
#include "common.h"

#include <vector>

namespace coskad {

constexpr int kStreamWave = 64;
constexpr int kStreamKp = 17;                  // joints of a raw row (x1, y1, ..., x17, y17)
constexpr int kStreamBlock = 256;
enum { kStreamKp18 = 1, kStreamHeadless = 2, kStreamNormalised = 4 };
constexpr int kStreamRadius = 120;             // the smoothing filter of score_frames.hip: gaussian_filter1d(sigma 30), truncate 4
constexpr int kStreamTaps = kStreamRadius + 1;
constexpr int kStreamShift = 11;               // score_process's shift
constexpr int kStreamSmoothChunk = 8;          // transformations summed side by side per pass of k_stream_smooth

__host__ __device__ inline bool stream_window_ok(int T) { return T == 8 || T == 12 || T == 16 || T == 24; }
__host__ __device__ inline bool stream_joints_ok(int V) { return V == 14 || V == 17 || V == 18; }
__host__ __device__ inline int stream_layout_joints(int flags) {
  return (flags & kStreamHeadless) ? 14 : ((flags & kStreamKp18) ? 18 : 17);
}

__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, kStreamWave));
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kStreamWave));
  return v;
}

// compute_bounding_box's one side: rint(clip(v, 0, hi)), rounding half to even
__device__ __forceinline__ float box_side(float v, float hi) { return rintf(fminf(fmaxf(v, 0.f), hi)); }

// RobustScaler.transform on a float32 column, as numpy's in-place `X -= center_; X /= scale_` rounds it: the difference and the
// quotient are formed in fp64 and each is stored to fp32.  A centred value that is exactly 0 is a missing joint and stays 0.
__device__ __forceinline__ float robust_f32(float v, double center, double scale) {
  if (v == 0.f) return 0.f;
  const float y = (float)((double)v - center);
  return (float)((double)y / scale);
}

// one wave = one detection; lane j < 17 owns joint j of the raw row.  wmax / hmax: the video's width - 1 and height - 1 of THIS detection
// (uniform per wave), so one body serves a launch of one camera (k_stream_push) and of many (k_stream_push_cams).
__device__ __forceinline__ void stream_push_body(const float* __restrict__ raw, const int* __restrict__ slot,
                                                 const int* __restrict__ reset, const int* __restrict__ out_index,
                                                 const double* __restrict__ center, const double* __restrict__ scale, float wmax,
                                                 float hmax, int flags, const float* __restrict__ mats, float* __restrict__ ring,
                                                 int* __restrict__ count, float* __restrict__ x_out, int m, int M, int K, int T, int V,
                                                 int step) {
  const int d = blockIdx.x, lane = threadIdx.x;
  const int sl = slot[d];
  if ((unsigned)sl >= (unsigned)M) return;             // uniform per wave: never a store outside the state
  const int R = (T - 1) * step + 1;
  const bool kp = lane < kStreamKp;
  float x = kp ? raw[(size_t)d * (2 * kStreamKp) + 2 * lane] : 0.f;
  float y = kp ? raw[(size_t)d * (2 * kStreamKp) + 2 * lane + 1] : 0.f;
  if (!(flags & kStreamNormalised)) {
    // bbox_centre_coordinates, branch for branch, in fp32
    const bool xm = kp && x != 0.f, ym = kp && y != 0.f;
    const float inf = __builtin_inff();
    const float left = wave_min_f(xm ? x : inf), right = wave_max_f(xm ? x : -inf);
    const float top = wave_min_f(ym ? y : inf), bottom = wave_max_f(ym ? y : -inf);
    float l_ = 0.f, r_ = 0.f, t_ = 0.f, b_ = 0.f;       // the (0, 0, 0, 0) box unless both axes have a joint
    if (left != inf && top != inf) {
      const float ew = 0.1f * ((right - left) + 1.f), eh = 0.1f * ((bottom - top) + 1.f);
      l_ = box_side(left - ew, wmax);
      r_ = box_side(right + ew, wmax);
      t_ = box_side(top - eh, hmax);
      b_ = box_side(bottom + eh, hmax);
    }
    const float cx = (l_ + r_) / 2.f, cy = (t_ + b_) / 2.f, w = r_ - l_, h = b_ - t_;
    const float xs = (xm ? x : cx) - cx, ys = (ym ? y : cy) - cy;
    x = w != 0.f ? __fdiv_rn(xs, w) : 0.f;
    y = h != 0.f ? __fdiv_rn(ys, h) : 0.f;
    if (center != nullptr && kp) {
      x = robust_f32(x, center[2 * lane], scale[2 * lane]);
      y = robust_f32(y, center[2 * lane + 1], scale[2 * lane + 1]);
    }
  }
  // layout: keypoints17_to_coco18's order with the neck = mean of the shoulders in fp64, then the first 14 joints when headless
  float ox = x, oy = y;
  if (flags & kStreamKp18) {
    constexpr int order[18] = {0, 17, 6, 8, 10, 5, 7, 9, 12, 14, 16, 11, 13, 15, 2, 1, 4, 3};
    const float x5 = __shfl(x, 5, kStreamWave), x6 = __shfl(x, 6, kStreamWave);
    const float y5 = __shfl(y, 5, kStreamWave), y6 = __shfl(y, 6, kStreamWave);
    const float nx = (float)(0.5 * ((double)x5 + (double)x6)), ny = (float)(0.5 * ((double)y5 + (double)y6));
    const int src = order[lane < 18 ? lane : 0];
    const float sx = __shfl(x, src & 31, kStreamWave), sy = __shfl(y, src & 31, kStreamWave);
    ox = src == 17 ? nx : sx;
    oy = src == 17 ? ny : sy;
  }
  // ring write; `count` is read by every lane before lane 0 stores it (readfirstlane waits for the load)
  int r = reset[d] != 0 ? 0 : count[sl];
  r = uniform(r);
  if (r < 0) r = 0;
  float* row = ring + (((size_t)sl * R + (size_t)(r % R)) * 2) * V;
  if (lane < V) {
    row[lane] = ox;
    row[V + lane] = oy;
  }
  if (lane == 0) count[sl] = r + 1;
  __syncthreads();                                      // the wave's own row is visible to all its lanes
  // the window that ends at this row
  const int j = out_index[d];
  if (j < 0 || j >= m || x_out == nullptr) return;
  const int TV = T * V;
  const bool full = r >= R - 1;                         // else the host's mirror and `count` disagree: a zero window, no stray read
  const float* base = ring + ((size_t)sl * R * 2) * V;
  for (int p = lane; p < TV; p += kStreamWave) {
    const int t = p / V, v = p - t * V;
    float wx = 0.f, wy = 0.f;
    if (full) {
      const int rr = (r - (R - 1) + t * step) % R;
      wx = base[((size_t)rr * 2) * V + v];
      wy = base[((size_t)rr * 2 + 1) * V + v];
    }
    for (int k = 0; k < K; ++k) {
      const float* mm = mats + k * 9;
      float* o = x_out + ((size_t)(k * m + j) * 2) * TV + p;
      // (x*m0 + y*m1) + 1*m2, the association of k_gather_frames (no FMA contraction: -ffp-contract=off)
      o[0] = full ? (wx * mm[0] + wy * mm[1]) + mm[2] : 0.f;
      o[TV] = full ? (wx * mm[3] + wy * mm[4]) + mm[5] : 0.f;
    }
  }
}

__global__ __launch_bounds__(kStreamWave) void k_stream_push(const float* __restrict__ raw, const int* __restrict__ slot,
                                                             const int* __restrict__ reset, const int* __restrict__ out_index,
                                                             const double* __restrict__ center, const double* __restrict__ scale,
                                                             float wmax, float hmax, int flags, const float* __restrict__ mats,
                                                             float* __restrict__ ring, int* __restrict__ count,
                                                             float* __restrict__ x_out, int m, int M, int K, int T, int V, int step) {
  stream_push_body(raw, slot, reset, out_index, center, scale, wmax, hmax, flags, mats, ring, count, x_out, m, M, K, T, V, step);
}

// the detections of many cameras in one launch: res [n, 2] = (width, height) of each detection's video
__global__ __launch_bounds__(kStreamWave) void k_stream_push_cams(const float* __restrict__ raw, const int* __restrict__ slot,
                                                                  const int* __restrict__ reset, const int* __restrict__ out_index,
                                                                  const double* __restrict__ center, const double* __restrict__ scale,
                                                                  const float* __restrict__ res, int flags,
                                                                  const float* __restrict__ mats, float* __restrict__ ring,
                                                                  int* __restrict__ count, float* __restrict__ x_out, int m, int M, int K,
                                                                  int T, int V, int step) {
  const float wmax = res[2 * (size_t)blockIdx.x] - 1.f, hmax = res[2 * (size_t)blockIdx.x + 1] - 1.f;
  stream_push_body(raw, slot, reset, out_index, center, scale, wmax, hmax, flags, mats, ring, count, x_out, m, M, K, T, V, step);
}

// Row i of a track whose last window ends at row `last`: the mean over the windows that end at i + (R - 1) - t step, t < T, inside
// [R - 1, last], by ascending window start (t descending); exactly-zero scores are missing, 0 when none is left (k_score_person_frames)
__device__ __forceinline__ double stream_row_mean(const double* __restrict__ ws, int i, int last, int R, int T, int step) {
  double sum = 0.0;
  int cnt = 0;
  for (int t = T - 1; t >= 0; --t) {
    const int e = i + (R - 1) - t * step;
    if (e < R - 1 || e > last) continue;
    const double s = ws[e % R];
    if (s != 0.0) { sum += s; ++cnt; }
  }
  return cnt > 0 ? sum / (double)cnt : 0.0;
}

// max on the bit pattern: the order of non-negative doubles is the order of their bits, and max does not depend on the order of arrival
__device__ __forceinline__ void clip_fold(double* __restrict__ clip, int clip_frames, int k, int idx, double v) {
  if (clip == nullptr || (unsigned)idx >= (unsigned)clip_frames || !(v > 0.0)) return;
  atomicMax(reinterpret_cast<unsigned long long*>(clip) + (size_t)k * clip_frames + idx, (unsigned long long)__double_as_longlong(v));
}

// one thread = one (transformation, ready track): store the new window's score, finalise row e - (R - 1)
template <typename S>
__global__ __launch_bounds__(kStreamBlock) void k_stream_frames(const S* __restrict__ scores, const int* __restrict__ slot,
                                                                const int* __restrict__ clip_index, const int* __restrict__ count,
                                                                double* __restrict__ wscore, double* __restrict__ frame_mean,
                                                                double* __restrict__ clip, int m, int M, int K, int T, int step,
                                                                int clip_frames) {
  const int id = blockIdx.x * kStreamBlock + threadIdx.x;
  if (id >= m * K) return;
  const int k = id / m, j = id - k * m;
  const int sl = slot[j];
  const int R = (T - 1) * step + 1;
  double mean = 0.0;
  if ((unsigned)sl < (unsigned)M) {
    const int e = count[sl] - 1;
    if (e >= R - 1) {
      double* ws = wscore + ((size_t)sl * K + k) * R;
      ws[e % R] = (double)scores[id];
      mean = stream_row_mean(ws, e - (R - 1), e, R, T, step);
      clip_fold(clip, clip_frames, k, clip_index != nullptr ? clip_index[j] : -1, mean);
    }
  }
  frame_mean[id] = mean;
}

// one thread = one (transformation, trailing row of a closed track); the row is final with the windows that exist
__global__ __launch_bounds__(kStreamBlock) void k_stream_close(const int* __restrict__ row_slot, const int* __restrict__ row_index,
                                                               const int* __restrict__ clip_index, const int* __restrict__ count,
                                                               const double* __restrict__ wscore, double* __restrict__ frame_mean,
                                                               double* __restrict__ clip, int rows, int M, int K, int T, int step,
                                                               int clip_frames) {
  const int id = blockIdx.x * kStreamBlock + threadIdx.x;
  if (id >= rows * K) return;
  const int k = id / rows, q = id - k * rows;
  const int sl = row_slot[q], i = row_index[q];
  const int R = (T - 1) * step + 1;
  double mean = 0.0;
  if ((unsigned)sl < (unsigned)M) {
    const int last = count[sl] - 1;
    if (i >= 0 && i <= last && i > last - R) {          // the ring still holds every window that covers the row
      mean = stream_row_mean(wscore + ((size_t)sl * K + k) * R, i, last, R, T, step);
      clip_fold(clip, clip_frames, k, clip_index != nullptr ? clip_index[q] : -1, mean);
    }
  }
  frame_mean[id] = mean;
}

// Fixed-lag smoothing of the clip vectors.  The flat buffer clip [K, F] holds one segment per camera; an item
// (offset, n, i) asks for output i of the segment [offset, offset + n): shifted[j] = raw[j - 11] (0 below 11) under scipy's `reflect`
// boundary of period 2n (d c b a | a b c d | d c b a; a segment shorter than the halo reflects several times).
__device__ __forceinline__ double smooth_tap_in(const double* __restrict__ r, int n, int j) {
  j %= 2 * n;
  if (j < 0) j += 2 * n;
  if (j >= n) j = 2 * n - 1 - j;
  return j >= kStreamShift ? r[j - kStreamShift] : 0.0;
}

// One wave = one item.  The lanes form the 121 terms of a transformation -- x[i] taps[0] and (x[i - k] + x[i + k]) taps[k], each rounded
// once, as k_score_smooth (score_frames.hip) rounds them -- into LDS; then ONE lane per transformation adds them in that kernel's order
// (centre first, then k = 120 .. 1), and lane 0 adds the transformations in order of t and divides by K.  No atomics: the value of an
// item depends on the item alone, and equals k_score_smooth's of the same segment bit for bit.
__global__ __launch_bounds__(kStreamWave) void k_stream_smooth(const double* __restrict__ clip, const int* __restrict__ items,
                                                               const double* __restrict__ taps, double* __restrict__ per_t,
                                                               double* __restrict__ mean, int n_items, int K, int F) {
  __shared__ double term[kStreamSmoothChunk][kStreamTaps];
  __shared__ double sums[kStreamSmoothChunk];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int off = items[3 * (size_t)q], n = items[3 * (size_t)q + 1], i = items[3 * (size_t)q + 2];
  const bool ok = off >= 0 && n > 0 && off <= F - n && i >= 0 && i < n;        // uniform per wave; the launcher checked the host's copy
  double acc_t = 0.0;
  for (int t0 = 0; t0 < K; t0 += kStreamSmoothChunk) {
    const int kc = K - t0 < kStreamSmoothChunk ? K - t0 : kStreamSmoothChunk;
    if (ok) {
      for (int e = lane; e < kc * kStreamTaps; e += kStreamWave) {
        const int tt = e / kStreamTaps, k = e - tt * kStreamTaps;
        const double* r = clip + (size_t)(t0 + tt) * F + off;
        term[tt][k] = k == 0 ? smooth_tap_in(r, n, i) * taps[0] : (smooth_tap_in(r, n, i - k) + smooth_tap_in(r, n, i + k)) * taps[k];
      }
    }
    __syncthreads();
    if (lane < kc) {
      double acc = 0.0;
      if (ok) {
        acc = term[lane][0];
        for (int k = kStreamRadius; k >= 1; --k) acc += term[lane][k];
      }
      per_t[(size_t)(t0 + lane) * n_items + q] = acc;
      sums[lane] = acc;
    }
    __syncthreads();
    if (lane == 0)
      for (int tt = 0; tt < kc; ++tt) acc_t += sums[tt];
  }
  if (lane == 0) mean[q] = ok ? acc_t / (double)K : 0.0;
}

// Per-joint maps beside the scores: the streaming counterpart of k_attribution_frames (attribution_frames.hip).  A window's
// map [T, V] holds one row per frame of the window; a track row's map is the mean, over the windows that cover the row, of the row each
// holds for it.  Windows arrive in ascending start, so adding a window's rows on arrival forms that kernel's fp64 sums in its order.
// State per (track, transformation): sums [R, V] f64 and counts [R] i32, row i of the track at slot i % R; one buffer, the sums of all
// tracks [M, K, R, V] first, then the counts [M, K, R].  The state is keyed on `count`: a track's FIRST window (e == R - 1) overwrites
// every slot -- its T target rows with their value, the rows between them (step > 1) with an empty sum -- and a later window overwrites
// the slot of its newest row e, whose former tenant e - R was final a push ago.  So a reused slot never sees its previous track's sums
// and nothing has to be cleared.  Unlike the score ring an exact 0 counts, and a row no window covers is NaN.
__host__ __device__ inline size_t stream_maps_rows(int M, int K, int T, int step) { return (size_t)M * K * ((size_t)(T - 1) * step + 1); }

// one wave = one (transformation, ready track): its T target rows are distinct, so no two lanes add to one sum
__global__ __launch_bounds__(kStreamWave) void k_stream_maps(const float* __restrict__ maps, const int* __restrict__ slot,
                                                             const int* __restrict__ count, double* __restrict__ sums,
                                                             int* __restrict__ cnts, double* __restrict__ frame_map, int m, int M, int K,
                                                             int T, int V, int step) {
  const int j = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
  const int sl = slot[j];
  const int R = (T - 1) * step + 1;
  double* out = frame_map + ((size_t)k * m + j) * V;
  const int e = (unsigned)sl < (unsigned)M ? uniform(count[sl]) - 1 : -1;
  if (e < R - 1) {                                      // uniform per wave: the host's mirror and `count` disagree
    if (lane < V) out[lane] = __builtin_nan("");
    return;
  }
  double* S = sums + ((size_t)sl * K + k) * R * V;
  int* C = cnts + ((size_t)sl * K + k) * R;
  const bool first = e == R - 1;
  // the count of the row that becomes final, read by every lane before any lane stores one (readfirstlane waits for the load)
  const int c0 = first ? 0 : uniform(C[(e - (R - 1)) % R]);
  if (first && step > 1) {                              // rows between the first window's rows: covered later, or never
    for (int q = lane; q < R * V; q += kStreamWave) {
      const int r = q / V;
      if (r % step == 0) continue;
      S[q] = 0.0;
      if (q == r * V) C[r] = 0;
    }
  }
  const float* w = maps + ((size_t)k * m + j) * T * V;
  for (int p = lane; p < T * V; p += kStreamWave) {
    const int t = p / V, v = p - t * V;
    const int pos = (e - (T - 1 - t) * step) % R;
    const bool fresh = first || t == T - 1;
    const double s = (fresh ? 0.0 : S[(size_t)pos * V + v]) + (double)w[p];        // 0.0 + x: the offline sum's first step
    S[(size_t)pos * V + v] = s;
    if (v == 0) C[pos] = fresh ? 1 : C[pos] + 1;
    if (t == 0) out[v] = s / (double)(c0 + 1);
  }
}

// one thread = one (transformation, trailing row of a closed track, joint); the row is final with the windows that exist
__global__ __launch_bounds__(kStreamBlock) void k_stream_maps_close(const int* __restrict__ row_slot, const int* __restrict__ row_index,
                                                                    const int* __restrict__ count, const double* __restrict__ sums,
                                                                    const int* __restrict__ cnts, double* __restrict__ frame_map,
                                                                    int rows, int M, int K, int T, int V, int step) {
  const size_t id = (size_t)blockIdx.x * kStreamBlock + threadIdx.x;
  if (id >= (size_t)rows * K * V) return;
  const int v = (int)(id % V);
  const int q = (int)((id / V) % rows), k = (int)(id / V / rows);
  const int sl = row_slot[q], i = row_index[q];
  const int R = (T - 1) * step + 1;
  double mean = __builtin_nan("");
  if ((unsigned)sl < (unsigned)M) {
    const int last = count[sl] - 1;
    if (last >= R - 1 && i >= 0 && i <= last && i > last - R) {      // the track filled a window and the state still holds the row
      const size_t at = ((size_t)sl * K + k) * R + (size_t)(i % R);
      const int c = cnts[at];
      if (c > 0) mean = sums[at * V + v] / (double)c;
    }
  }
  frame_map[id] = mean;
}

// the host mirror of a launch's slots: every one inside [0, M); `distinct`: no slot twice (two waves would write one ring)
static const char* bad_slots(const int* slot_host, int n, int M, bool distinct) {
  for (int i = 0; i < n; ++i)
    if (slot_host[i] < 0 || slot_host[i] >= M) return "a slot outside [0, max_tracks)";
  if (distinct) {
    std::vector<bool> seen((size_t)M, false);
    for (int i = 0; i < n; ++i) {
      if (seen[(size_t)slot_host[i]]) return "a slot twice in one launch";
      seen[(size_t)slot_host[i]] = true;
    }
  }
  return nullptr;
}

}  // namespace coskad

using namespace coskad;

extern "C" {

int coskad_stream_ok(int T, int V) { return stream_window_ok(T) && stream_joints_ok(V) ? 1 : 0; }
int coskad_stream_smooth_lag(void) { return kStreamRadius; }

// the checks both push entries share; `who` names the entry in the message
static int push_args_bad(const char* who, const float* raw, const int* slot, const int* slot_host, const int* reset,
                         const int* out_index, const double* center, const double* scale, int flags, const float* mats,
                         const float* ring, const int* count, const float* x_out, int n, int m, int M, int K, int T, int V, int step) {
  if (!raw || !slot || !slot_host || !reset || !out_index || !mats || !ring || !count) return fail(COSKAD_ERR_ARG, "%s: null pointer", who);
  if ((center == nullptr) != (scale == nullptr)) return fail(COSKAD_ERR_ARG, "%s: center and scale come together", who);
  if (n <= 0 || m < 0 || m > n || M <= 0 || K <= 0 || step <= 0)
    return fail(COSKAD_ERR_ARG, "%s: n=%d m=%d max_tracks=%d K=%d step=%d", who, n, m, M, K, step);
  if (m > 0 && !x_out) return fail(COSKAD_ERR_ARG, "%s: null pointer", who);
  if (flags < 0 || flags > 7) return fail(COSKAD_ERR_ARG, "%s: flags=%d", who, flags);
  if (!coskad_stream_ok(T, V))
    return fail(COSKAD_ERR_SHAPE, "%s: unsupported (n_frames=%d, n_joints=%d): windows of 8 / 12 / 16 / 24 frames, 14 / 17 / 18 joints", who,
                T, V);
  if (V != stream_layout_joints(flags)) return fail(COSKAD_ERR_ARG, "%s: n_joints=%d with layout flags %d", who, V, flags);
  return 0;
}

int coskad_stream_push_f32(const float* raw, const int* slot, const int* slot_host, const int* reset, const int* out_index,
                           const double* center, const double* scale, float width, float height, int flags, const float* mats,
                           float* ring, int* count, float* x_out, int n, int m, int M, int K, int T, int V, int step,
                           hipStream_t stream) {
  if (int rc = push_args_bad("stream_push", raw, slot, slot_host, reset, out_index, center, scale, flags, mats, ring, count, x_out, n, m, M,
                             K, T, V, step))
    return rc;
  if (!(flags & kStreamNormalised) && !(width >= 1.f && height >= 1.f))
    return fail(COSKAD_ERR_ARG, "stream_push: video resolution %g x %g", (double)width, (double)height);
  if ((long long)(T - 1) * step + 1 > 0x7fffffffLL / (2 * 18)) return fail(COSKAD_ERR_ARG, "stream_push: step=%d", step);
  if (const char* why = bad_slots(slot_host, n, M, true)) return fail(COSKAD_ERR_ARG, "stream_push: %s", why);
  hipLaunchKernelGGL(k_stream_push, dim3((unsigned)n), dim3(kStreamWave), 0, stream, raw, slot, reset, out_index, center, scale,
                     width - 1.f, height - 1.f, flags, mats, ring, count, x_out, m, M, K, T, V, step);
  return check_launch("stream_push");
}

int coskad_stream_push_cams_f32(const float* raw, const int* slot, const int* slot_host, const int* reset, const int* out_index,
                                const double* center, const double* scale, const float* res, const float* res_host, int flags,
                                const float* mats, float* ring, int* count, float* x_out, int n, int m, int M, int K, int T, int V,
                                int step, hipStream_t stream) {
  if (int rc = push_args_bad("stream_push_cams", raw, slot, slot_host, reset, out_index, center, scale, flags, mats, ring, count, x_out, n,
                             m, M, K, T, V, step))
    return rc;
  if (!(flags & kStreamNormalised)) {
    if (!res || !res_host) return fail(COSKAD_ERR_ARG, "stream_push_cams: null pointer (res)");
    for (int i = 0; i < n; ++i)
      if (!(res_host[2 * i] >= 1.f && res_host[2 * i + 1] >= 1.f))
        return fail(COSKAD_ERR_ARG, "stream_push_cams: res[%d]: video resolution %g x %g", i, (double)res_host[2 * i],
                    (double)res_host[2 * i + 1]);
  }
  if ((long long)(T - 1) * step + 1 > 0x7fffffffLL / (2 * 18)) return fail(COSKAD_ERR_ARG, "stream_push_cams: step=%d", step);
  if (const char* why = bad_slots(slot_host, n, M, true)) return fail(COSKAD_ERR_ARG, "stream_push_cams: %s", why);
  if (flags & kStreamNormalised)        // the resolution is not read: no box is formed
    hipLaunchKernelGGL(k_stream_push, dim3((unsigned)n), dim3(kStreamWave), 0, stream, raw, slot, reset, out_index, center, scale, 0.f, 0.f,
                       flags, mats, ring, count, x_out, m, M, K, T, V, step);
  else
    hipLaunchKernelGGL(k_stream_push_cams, dim3((unsigned)n), dim3(kStreamWave), 0, stream, raw, slot, reset, out_index, center, scale, res,
                       flags, mats, ring, count, x_out, m, M, K, T, V, step);
  return check_launch("stream_push_cams");
}

int coskad_stream_frames_f64(const void* scores, int scores_f64, const int* slot, const int* slot_host, const int* clip_index,
                             const int* count, double* wscore, double* frame_mean, double* clip, int clip_frames, int m, int M, int K,
                             int T, int step, hipStream_t stream) {
  if (!scores || !slot || !slot_host || !count || !wscore || !frame_mean) return fail(COSKAD_ERR_ARG, "stream_frames: null pointer");
  if (m <= 0 || M <= 0 || K <= 0 || step <= 0 || (clip && clip_frames <= 0) || (long long)m * K > 0x7fffffffLL)
    return fail(COSKAD_ERR_ARG, "stream_frames: m=%d max_tracks=%d K=%d step=%d clip_frames=%d", m, M, K, step, clip_frames);
  if (clip && !clip_index) return fail(COSKAD_ERR_ARG, "stream_frames: null pointer");
  if (!stream_window_ok(T)) return fail(COSKAD_ERR_SHAPE, "stream_frames: unsupported n_frames=%d: windows of 8 / 12 / 16 / 24 frames", T);
  if (const char* why = bad_slots(slot_host, m, M, true)) return fail(COSKAD_ERR_ARG, "stream_frames: %s", why);
  const dim3 grid((unsigned)ceil_div(m * K, kStreamBlock));
  if (scores_f64)
    hipLaunchKernelGGL(k_stream_frames<double>, grid, dim3(kStreamBlock), 0, stream, (const double*)scores, slot, clip_index, count, wscore,
                       frame_mean, clip, m, M, K, T, step, clip_frames);
  else
    hipLaunchKernelGGL(k_stream_frames<float>, grid, dim3(kStreamBlock), 0, stream, (const float*)scores, slot, clip_index, count, wscore,
                       frame_mean, clip, m, M, K, T, step, clip_frames);
  return check_launch("stream_frames");
}

int coskad_stream_close_f64(const int* row_slot, const int* row_slot_host, const int* row_index, const int* clip_index, const int* count,
                            const double* wscore, double* frame_mean, double* clip, int clip_frames, int rows, int M, int K, int T,
                            int step, hipStream_t stream) {
  if (!row_slot || !row_slot_host || !row_index || !count || !wscore || !frame_mean) return fail(COSKAD_ERR_ARG, "stream_close: null pointer");
  if (rows <= 0 || M <= 0 || K <= 0 || step <= 0 || (clip && clip_frames <= 0) || (long long)rows * K > 0x7fffffffLL)
    return fail(COSKAD_ERR_ARG, "stream_close: rows=%d max_tracks=%d K=%d step=%d clip_frames=%d", rows, M, K, step, clip_frames);
  if (clip && !clip_index) return fail(COSKAD_ERR_ARG, "stream_close: null pointer");
  if (!stream_window_ok(T)) return fail(COSKAD_ERR_SHAPE, "stream_close: unsupported n_frames=%d: windows of 8 / 12 / 16 / 24 frames", T);
  if (const char* why = bad_slots(row_slot_host, rows, M, false)) return fail(COSKAD_ERR_ARG, "stream_close: %s", why);
  hipLaunchKernelGGL(k_stream_close, dim3((unsigned)ceil_div(rows * K, kStreamBlock)), dim3(kStreamBlock), 0, stream, row_slot, row_index,
                     clip_index, count, wscore, frame_mean, clip, rows, M, K, T, step, clip_frames);
  return check_launch("stream_close");
}

size_t coskad_stream_maps_state_bytes(int M, int K, int T, int V, int step) {
  if (M <= 0 || K <= 0 || step <= 0 || !coskad_stream_ok(T, V) || (long long)(T - 1) * step + 1 > 0x7fffffffLL / (2 * 18)) return 0;
  const size_t rows = stream_maps_rows(M, K, T, step);
  return rows * V * sizeof(double) + (rows * sizeof(int) + 7) / 8 * 8;
}

// the checks both maps entries share; `who` names the entry in the message
static int maps_args_bad(const char* who, const char* items, const void* state, size_t state_bytes, int n, int M, int K, int T, int V,
                         int step) {
  if (n <= 0 || M <= 0 || K <= 0 || step <= 0 || (long long)n * K * 18 > 0x7fffffffLL)
    return fail(COSKAD_ERR_ARG, "%s: %s=%d max_tracks=%d K=%d step=%d", who, items, n, M, K, step);
  if (!coskad_stream_ok(T, V))
    return fail(COSKAD_ERR_SHAPE, "%s: unsupported (n_frames=%d, n_joints=%d): windows of 8 / 12 / 16 / 24 frames, 14 / 17 / 18 joints", who,
                T, V);
  const size_t need = coskad_stream_maps_state_bytes(M, K, T, V, step);
  if (need == 0) return fail(COSKAD_ERR_ARG, "%s: step=%d", who, step);
  if (state_bytes < need) return fail(COSKAD_ERR_ARG, "%s: state of %zu bytes, coskad_stream_maps_state_bytes asks for %zu", who, state_bytes, need);
  if ((size_t)state % sizeof(double)) return fail(COSKAD_ERR_ARG, "%s: state is not aligned to 8 bytes", who);
  return 0;
}

int coskad_stream_maps_f64(const float* maps, const int* slot, const int* slot_host, const int* count, double* state, size_t state_bytes,
                           double* frame_map, int m, int M, int K, int T, int V, int step, hipStream_t stream) {
  if (!maps || !slot || !slot_host || !count || !state || !frame_map) return fail(COSKAD_ERR_ARG, "stream_maps: null pointer");
  if (m > M) return fail(COSKAD_ERR_ARG, "stream_maps: m=%d ready tracks, more than max_tracks=%d", m, M);
  if (int rc = maps_args_bad("stream_maps", "m", state, state_bytes, m, M, K, T, V, step)) return rc;
  if (K > 65535) return fail(COSKAD_ERR_ARG, "stream_maps: K=%d", K);
  if (const char* why = bad_slots(slot_host, m, M, true)) return fail(COSKAD_ERR_ARG, "stream_maps: %s", why);
  const size_t rows = stream_maps_rows(M, K, T, step);
  hipLaunchKernelGGL(k_stream_maps, dim3((unsigned)m, (unsigned)K), dim3(kStreamWave), 0, stream, maps, slot, count, state,
                     reinterpret_cast<int*>(state + rows * V), frame_map, m, M, K, T, V, step);
  return check_launch("stream_maps");
}

int coskad_stream_maps_close_f64(const int* row_slot, const int* row_slot_host, const int* row_index, const int* count,
                                 const double* state, size_t state_bytes, double* frame_map, int rows, int M, int K, int T, int V,
                                 int step, hipStream_t stream) {
  if (!row_slot || !row_slot_host || !row_index || !count || !state || !frame_map)
    return fail(COSKAD_ERR_ARG, "stream_maps_close: null pointer");
  if (int rc = maps_args_bad("stream_maps_close", "rows", state, state_bytes, rows, M, K, T, V, step)) return rc;
  if (const char* why = bad_slots(row_slot_host, rows, M, false)) return fail(COSKAD_ERR_ARG, "stream_maps_close: %s", why);
  const size_t all = stream_maps_rows(M, K, T, step);
  hipLaunchKernelGGL(k_stream_maps_close, dim3((unsigned)ceil_div(rows * K * V, kStreamBlock)), dim3(kStreamBlock), 0, stream, row_slot,
                     row_index, count, state, reinterpret_cast<const int*>(state + all * V), frame_map, rows, M, K, T, V, step);
  return check_launch("stream_maps_close");
}

int coskad_stream_smooth_f64(const double* clip, const int* items, const int* items_host, const double* taps, int n_taps, double* per_t,
                             double* mean, int n_items, int K, int F, hipStream_t stream) {
  if (!clip) return fail(COSKAD_ERR_ARG, "stream_smooth: null pointer (clip)");
  if (!items || !items_host) return fail(COSKAD_ERR_ARG, "stream_smooth: null pointer (items)");
  if (!taps) return fail(COSKAD_ERR_ARG, "stream_smooth: null pointer (taps)");
  if (!per_t || !mean) return fail(COSKAD_ERR_ARG, "stream_smooth: null pointer (per_t, mean)");
  if (n_items <= 0 || K <= 0 || F <= 0 || (long long)n_items * K > 0x7fffffffLL)
    return fail(COSKAD_ERR_ARG, "stream_smooth: n_items=%d K=%d F=%d", n_items, K, F);
  if (n_taps != kStreamTaps)
    return fail(COSKAD_ERR_SHAPE, "stream_smooth: unsupported tap table of %d entries: the filter has %d taps (centre + radius %d)", n_taps,
                kStreamTaps, kStreamRadius);
  for (int q = 0; q < n_items; ++q) {
    const int off = items_host[3 * q], n = items_host[3 * q + 1], i = items_host[3 * q + 2];
    if (off < 0 || n <= 0 || n > 0x3fffffff || off > F - n || i < 0 || i >= n)
      return fail(COSKAD_ERR_ARG, "stream_smooth: items[%d] = (offset %d, n %d, index %d) outside the buffer of %d frames", q, off, n, i, F);
  }
  hipLaunchKernelGGL(k_stream_smooth, dim3((unsigned)n_items), dim3(kStreamWave), 0, stream, clip, items, taps, per_t, mean, n_items, K, F);
  return check_launch("stream_smooth");
}

}  // extern "C"
