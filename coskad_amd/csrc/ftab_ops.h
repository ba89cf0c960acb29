// The forward operand tables of the apply + next-layer-statistics kernels (fused_apply_next.hip), built from a layer's A / T:
// by k_build_ftab, or by extra blocks of the first layer's moments launch (first_layer.hip) -- parameter-only work.
#pragma once
#include "common.h"

namespace coskad {

// forward operand tables of up to 4 layers, the tab-stream layout of the eval-mode encoder (coskad_amd/fused_plan.py):
//   temporal  rec[v][l][s]     = T[v][4s+q][j]   (s < 3, j < 12)
//   spatial   rec[t][l][0..4]  = A[t][4s+q][j]   (4s+q < 17),  [5..9] = A[t][4s+q][16]
struct FtabArgs {
  const float* A[4];
  const float* Tm[4];
  float* tab[4];
  int n;                        // layers (the riding form; k_build_ftab's grid carries it)
};

template <int T, int V>
constexpr int ftab_elems() { return (V * 64 + T * 3 * 64) * 4; }

// element e of layer `layer`'s table
template <int T, int V>
__device__ __forceinline__ void ftab_store(const FtabArgs& args, int layer, int e) {
  constexpr int TEMP_F4 = V * 64;
  const float* __restrict__ Aw = args.A[layer];
  const float* __restrict__ Tw = args.Tm[layer];
  if (e >= ftab_elems<T, V>()) return;
  float val = 0.f;
  if (e < TEMP_F4 * 4) {
    const int v = e / 256, l = (e >> 2) & 63, s = e & 3, j = l & 15, q = l >> 4;
    if (s < 3 && j < T) val = Tw[v * T * T + (4 * s + q) * T + j];
  } else {
    const int r = e - TEMP_F4 * 4;
    const int t = r / (3 * 256), c = (r / 256) % 3, l = (r >> 2) & 63, k = 4 * c + (r & 3), j = l & 15, q = l >> 4;
    if (k < 10) {
      const int s = k < 5 ? k : k - 5, w = 4 * s + q;
      if (w < V) val = Aw[t * V * V + w * V + (k < 5 ? j : 16)];
    }
  }
  args.tab[layer][e] = val;
}

}  // namespace coskad
