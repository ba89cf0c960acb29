// Online scoring (coskad_amd/stream.py): the offline pipeline's arithmetic one frame at a time.  A pose tracker hands in a few
// raw skeletons per frame; k_stream_push normalises each of them as utils/data.py does per frame (bounding-box centring, RobustScaler,
// joint layout: coskad_amd.utils.dataset.bbox_centre_coordinates / scale_robust / pose_layout), stores the row into the track's ring and,
// where the track has a full window, writes the window's K affine copies with the expression of k_gather_frames (data.hip).  After the
// model has scored those windows, k_stream_frames keeps the scores in a ring per track and finalises the one row that no later window
// can cover, by the rules of k_score_person_frames (score_frames.hip).  k_stream_close finalises a closed track's trailing rows.
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

// one wave = one detection; lane j < 17 owns joint j of the raw row
__global__ __launch_bounds__(kStreamWave) void k_stream_push(const float* __restrict__ raw, const int* __restrict__ slot,
                                                             const int* __restrict__ reset, const int* __restrict__ out_index,
                                                             const double* __restrict__ center, const double* __restrict__ scale,
                                                             float wmax, float hmax, int flags, const float* __restrict__ mats,
                                                             float* __restrict__ ring, int* __restrict__ count,
                                                             float* __restrict__ x_out, int m, int M, int K, int T, int V, int step) {
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

int coskad_stream_push_f32(const float* raw, const int* slot, const int* slot_host, const int* reset, const int* out_index,
                           const double* center, const double* scale, float width, float height, int flags, const float* mats,
                           float* ring, int* count, float* x_out, int n, int m, int M, int K, int T, int V, int step,
                           hipStream_t stream) {
  if (!raw || !slot || !slot_host || !reset || !out_index || !mats || !ring || !count)
    return fail(COSKAD_ERR_ARG, "stream_push: null pointer");
  if ((center == nullptr) != (scale == nullptr)) return fail(COSKAD_ERR_ARG, "stream_push: center and scale come together");
  if (n <= 0 || m < 0 || m > n || M <= 0 || K <= 0 || step <= 0)
    return fail(COSKAD_ERR_ARG, "stream_push: n=%d m=%d max_tracks=%d K=%d step=%d", n, m, M, K, step);
  if (m > 0 && !x_out) return fail(COSKAD_ERR_ARG, "stream_push: null pointer");
  if (flags < 0 || flags > 7) return fail(COSKAD_ERR_ARG, "stream_push: flags=%d", flags);
  if (!coskad_stream_ok(T, V))
    return fail(COSKAD_ERR_SHAPE, "stream_push: unsupported (n_frames=%d, n_joints=%d): windows of 8 / 12 / 16 / 24 frames, 14 / 17 / 18 joints",
                T, V);
  if (V != stream_layout_joints(flags)) return fail(COSKAD_ERR_ARG, "stream_push: n_joints=%d with layout flags %d", V, flags);
  if (!(flags & kStreamNormalised) && !(width >= 1.f && height >= 1.f))
    return fail(COSKAD_ERR_ARG, "stream_push: video resolution %g x %g", (double)width, (double)height);
  if ((long long)(T - 1) * step + 1 > 0x7fffffffLL / (2 * 18)) return fail(COSKAD_ERR_ARG, "stream_push: step=%d", step);
  if (const char* why = bad_slots(slot_host, n, M, true)) return fail(COSKAD_ERR_ARG, "stream_push: %s", why);
  hipLaunchKernelGGL(k_stream_push, dim3((unsigned)n), dim3(kStreamWave), 0, stream, raw, slot, reset, out_index, center, scale,
                     width - 1.f, height - 1.f, flags, mats, ring, count, x_out, m, M, K, T, V, step);
  return check_launch("stream_push");
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

}  // extern "C"
