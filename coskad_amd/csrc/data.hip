// Batch formation on the device: the window table [N, 2, T*V] stays resident in HBM; a batch is
// one gather + affine-transform launch.  Replaces the reference's per-item numpy path
// utils/dataset.py:65-77 (`sample = index % N`, `trans = index // N`, `transform_list[trans](data)[:num_coords]`) with
// utils/dataset_utils.py:272-286 (`einsum('ktv,ck->ctv', (x, y, 1), M)`).
// Second residency (`dataset_resident: 'frames'`): the table holds one row per trajectory FRAME, [F, 2, V], and k_gather_frames forms
// the window from the rows win_row[s] + t*step inside the same launch (utils/preprocessing.py:244-313 as an index, not a copy).
#include "common.h"

namespace coskad {

// one thread = 4 consecutive positions of one batch item (TV % 4 == 0) or 1 position (generic)
template <int VEC>
__global__ __launch_bounds__(256) void k_gather_transform(const float* __restrict__ xy, const long long* __restrict__ index,
                                                         const float* __restrict__ mats, float* __restrict__ out, int B,
                                                         int N, int ntrans, int TV) {
  const int per = TV / VEC;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)B * per) return;
  const int b = (int)(e / per), q = (int)(e - (long long)b * per) * VEC;
  const long long id = index[b];
  const long long t = id / N, s = id - t * N;
  float* o0 = out + ((size_t)b * 2) * TV + q;
  float* o1 = o0 + TV;
  if (id < 0 || t >= ntrans) {   // out-of-range index: a zero clip rather than an out-of-bounds read
#pragma unroll
    for (int u = 0; u < VEC; ++u) { o0[u] = 0.f; o1[u] = 0.f; }
    return;
  }
  const float* m = mats + t * 9;
  const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
  const float* px = xy + ((size_t)s * 2) * TV + q;
  const float* py = px + TV;
  if constexpr (VEC == 4) {
    const float4 x = *reinterpret_cast<const float4*>(px), y = *reinterpret_cast<const float4*>(py);
    // (x*m0 + y*m1) + 1*m2, in the einsum's summation order (no FMA contraction: -ffp-contract=off)
    *reinterpret_cast<float4*>(o0) = float4{(x.x * m00 + y.x * m01) + m02, (x.y * m00 + y.y * m01) + m02,
                                            (x.z * m00 + y.z * m01) + m02, (x.w * m00 + y.w * m01) + m02};
    *reinterpret_cast<float4*>(o1) = float4{(x.x * m10 + y.x * m11) + m12, (x.y * m10 + y.y * m11) + m12,
                                            (x.z * m10 + y.z * m11) + m12, (x.w * m10 + y.w * m11) + m12};
  } else {
    const float x = px[0], y = py[0];
    o0[0] = (x * m00 + y * m01) + m02;
    o1[0] = (x * m10 + y * m11) + m12;
  }
}

// The frame-resident form: fxy [F, 2, V] holds ONE row per trajectory frame and window s is the rows win_row[s] + t*step, t < T.
// one thread = 4 consecutive (t, v) positions of one batch item (T*V % 4 == 0) or 1 position (generic); a 4-group may straddle two
// frames (V = 17), so the loads are per element and only the stores are 16 bytes wide
template <int VEC>
__global__ __launch_bounds__(256) void k_gather_frames(const float* __restrict__ fxy, const int* __restrict__ win_row,
                                                      const long long* __restrict__ index, const float* __restrict__ mats,
                                                      float* __restrict__ out, int B, int N, long long F, int ntrans, int T, int V,
                                                      int step) {
  const int TV = T * V, per = TV / VEC;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)B * per) return;
  const int b = (int)(e / per), q = (int)(e - (long long)b * per) * VEC;
  const long long id = index[b];
  const long long tr = id / N, s = id - tr * N;
  float* o0 = out + ((size_t)b * 2) * TV + q;
  float* o1 = o0 + TV;
  const bool in_table = id >= 0 && tr < ntrans;
  const long long row0 = in_table ? (long long)win_row[s] : -1;
  // out-of-range index or a window that leaves the frame table: a zero clip rather than an out-of-bounds read
  if (row0 < 0 || row0 + (long long)(T - 1) * step >= F) {
#pragma unroll
    for (int u = 0; u < VEC; ++u) { o0[u] = 0.f; o1[u] = 0.f; }
    return;
  }
  const float* m = mats + tr * 9;
  const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5];
  float x[VEC], y[VEC];
#pragma unroll
  for (int u = 0; u < VEC; ++u) {
    const int t = (q + u) / V, v = (q + u) - t * V;
    const float* px = fxy + ((row0 + (long long)t * step) * 2) * V + v;
    x[u] = px[0];
    y[u] = px[V];
  }
  // (x*m0 + y*m1) + 1*m2, the association of k_gather_transform (no FMA contraction: -ffp-contract=off)
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(o0) = float4{(x[0] * m00 + y[0] * m01) + m02, (x[1] * m00 + y[1] * m01) + m02,
                                            (x[2] * m00 + y[2] * m01) + m02, (x[3] * m00 + y[3] * m01) + m02};
    *reinterpret_cast<float4*>(o1) = float4{(x[0] * m10 + y[0] * m11) + m12, (x[1] * m10 + y[1] * m11) + m12,
                                            (x[2] * m10 + y[2] * m11) + m12, (x[3] * m10 + y[3] * m11) + m12};
  } else {
    o0[0] = (x[0] * m00 + y[0] * m01) + m02;
    o1[0] = (x[0] * m10 + y[0] * m11) + m12;
  }
}

}  // namespace coskad

using namespace coskad;

extern "C" {

/* out[b, c, p] = M[t][c][0] x[s, p] + M[t][c][1] y[s, p] + M[t][c][2],  s = index[b] % N, t = index[b] / N, c < 2. */
int coskad_gather_transform_f32(const float* xy, const long long* index, const float* mats, float* out, int B, int N,
                                int ntrans, int TV, hipStream_t stream) {
  if (!xy || !index || !mats || !out) return fail(COSKAD_ERR_ARG, "gather_transform: null pointer");
  if (B <= 0 || N <= 0 || ntrans <= 0 || TV <= 0) return fail(COSKAD_ERR_ARG, "gather_transform: B=%d N=%d ntrans=%d TV=%d", B, N, ntrans, TV);
  if (TV % 4 == 0) {
    const long long n = (long long)B * (TV / 4);
    hipLaunchKernelGGL(k_gather_transform<4>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, xy, index, mats, out, B, N, ntrans, TV);
  } else {
    const long long n = (long long)B * TV;
    hipLaunchKernelGGL(k_gather_transform<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, xy, index, mats, out, B, N, ntrans, TV);
  }
  return check_launch("gather_transform");
}

/* out[b, c, t, v] = M[tr][c][0] x + M[tr][c][1] y + M[tr][c][2] with (x, y) = fxy[win_row[s] + t step, 0 / 1, v], s = index[b] % N,
 * tr = index[b] / N, c < 2: the same items from one row per trajectory frame. */
int coskad_gather_frames_f32(const float* fxy, const int* win_row, const long long* index, const float* mats, float* out, int B,
                             int N, long long F, int ntrans, int T, int V, int step, hipStream_t stream) {
  if (!fxy || !win_row || !index || !mats || !out) return fail(COSKAD_ERR_ARG, "gather_frames: null pointer");
  if (B <= 0 || N <= 0 || ntrans <= 0 || T <= 0 || V <= 0 || step <= 0)
    return fail(COSKAD_ERR_ARG, "gather_frames: B=%d N=%d ntrans=%d T=%d V=%d step=%d", B, N, ntrans, T, V, step);
  if (F <= 0 || F > 0x7fffffffLL) return fail(COSKAD_ERR_ARG, "gather_frames: F=%lld is not in [1, 2^31)", F);
  if ((long long)T * V > 0x7fffffffLL) return fail(COSKAD_ERR_ARG, "gather_frames: T=%d V=%d: a clip above 2^31 positions", T, V);
  const int TV = T * V;
  const long long n = TV % 4 == 0 ? (long long)B * (TV / 4) : (long long)B * TV;
  if ((n + 255) / 256 > 0x7fffffffLL) return fail(COSKAD_ERR_ARG, "gather_frames: B=%d T=%d V=%d: too many blocks for one launch", B, T, V);
  const dim3 grid((unsigned)((n + 255) / 256));
  if (TV % 4 == 0)
    hipLaunchKernelGGL(k_gather_frames<4>, grid, dim3(256), 0, stream, fxy, win_row, index, mats, out, B, N, F, ntrans, T, V, step);
  else
    hipLaunchKernelGGL(k_gather_frames<1>, grid, dim3(256), 0, stream, fxy, win_row, index, mats, out, B, N, F, ntrans, T, V, step);
  return check_launch("gather_frames");
}

}  // extern "C"
