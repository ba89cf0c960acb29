// Per-window attribution maps -> per-person frame maps, beside score_frames.hip and on the same tables (coskad_amd.utils.score_plan.
// ScorePlan): a person-frame's map is the mean over its covering windows of the row each of them holds for that frame -- window w
// contributes position t with frames[w][t] == the frame's number.  fp64 sums in ascending window order (the window CSR's), one thread
// per (person-frame, joint), no atomics: two runs agree bit for bit, and with the numpy loop of eval_utils.attribution_frames.  A
// person-frame no window covers is NaN.
#include "common.h"

namespace coskad {

constexpr int kAttrBlock = 256;

__global__ __launch_bounds__(kAttrBlock) void k_attribution_frames(const float* __restrict__ attr, const int* __restrict__ frames,
                                                                  const int* __restrict__ win_ptr, const int* __restrict__ win_idx,
                                                                  const int* __restrict__ entry_frame, double* __restrict__ out,
                                                                  int n_windows, int n_rows, int T, int V) {
  const size_t i = (size_t)blockIdx.x * kAttrBlock + threadIdx.x;
  if (i >= (size_t)n_rows * V) return;
  const int e = (int)(i / V), v = (int)(i - (size_t)e * V);
  const int frame = entry_frame[e];
  const int k0 = win_ptr[e], k1 = win_ptr[e + 1];
  double sum = 0.0;
  int cnt = 0;
  for (int k = k0; k < k1; ++k) {
    const int w = win_idx[k];
    if ((unsigned)w >= (unsigned)n_windows) continue;    // a table that does not belong to these maps: never read out of bounds
    const int* fr = frames + (size_t)w * T;
    int t = 0;
    while (t < T && fr[t] != frame) ++t;
    if (t == T) continue;
    sum += (double)attr[((size_t)w * T + t) * V + v];
    ++cnt;
  }
  out[i] = cnt > 0 ? sum / (double)cnt : __builtin_nan("");
}

}  // namespace coskad

using namespace coskad;

extern "C" {

int coskad_attribution_frames_f64(const float* attr, const int* frames, const int* win_ptr, const int* win_idx, const int* entry_frame,
                                  double* out, int n_windows, int n_rows, int T, int V, hipStream_t stream) {
  if (!attr || !frames || !win_ptr || !win_idx || !entry_frame || !out) return fail(COSKAD_ERR_ARG, "attribution_frames: null pointer");
  if (n_windows <= 0 || n_rows <= 0 || T <= 0 || V <= 0)
    return fail(COSKAD_ERR_ARG, "attribution_frames: n_windows=%d n_rows=%d T=%d V=%d", n_windows, n_rows, T, V);
  const size_t n = (size_t)n_rows * V, blocks = (n + kAttrBlock - 1) / kAttrBlock;
  if (blocks > 0x7fffffffu) return fail(COSKAD_ERR_SHAPE, "attribution_frames: unsupported size: %zu outputs", n);
  hipLaunchKernelGGL(k_attribution_frames, dim3((unsigned)blocks), dim3(kAttrBlock), 0, stream, attr, frames, win_ptr, win_idx,
                     entry_frame, out, n_windows, n_rows, T, V);
  return check_launch("attribution_frames");
}

}  // extern "C"
