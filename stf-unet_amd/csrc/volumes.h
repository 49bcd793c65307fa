// The volume table of the entry points that work per volume of stacked slices (ccl.hip,
// boundary.hip): starts int32 [V + 1], strictly ascending, starts[0] = 0, starts[V] = N.  The
// kernels read the device copy; the host copy is validated before anything is launched.
#pragma once
#include "common.h"

namespace stf {

struct Vol {
  int v;        // the volume of slice z
  int z0;       // its first slice, 0 <= z0 <= z
};

// wave-uniform.  Volumes: the largest v with starts[v] <= z.  Images: slice z is volume z.
template <bool VOL>
STF_DEV Vol volume_of(const int* __restrict__ starts, int V, int z) {
  if constexpr (!VOL) {
    return {z, z};
  } else {
    int lo = 0, hi = V;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (starts[mid] <= z) lo = mid; else hi = mid;
    }
    int z0 = starts[lo];
    if ((unsigned)z0 > (unsigned)z) z0 = z;
    return {lo, z0};
  }
}

// N, H, W, V inside the limits and N * H * W < 2^31 (images: V = N)
inline bool volume_sizes_ok(int N, int H, int W, int V, int maxdim) {
  if (N < 1 || H < 1 || W < 1 || H > maxdim || W > maxdim || V < 1 || V > N) return false;
  return (long)N * H * W < (1L << 31);
}

// strictly ascending from 0 to N
inline bool starts_ok(const int32_t* starts, int V, int N) {
  if (starts[0] != 0 || starts[V] != N) return false;
  for (int v = 0; v < V; ++v)
    if (starts[v] >= starts[v + 1]) return false;
  return true;
}

}  // namespace stf
