// Connected components of stacked binary masks on the device:
// the machinery of ccl.hip with more neighbour rows and a volume boundary that is never crossed.
// The uint8 [N][H][W] batch is cut into V volumes of consecutive slices by starts int32 [V + 1]
// (strictly ascending, starts[0] = 0, starts[V] = N; the host copy is validated, the device copy is
// what the kernels read).  Every volume is labelled on its own: foreground is mask != 0, outside
// the volume is background, connectivity is scipy's generate_binary_structure(3, 1 | 2 | 3).
//
// The state is one int32 parent per voxel, L[g], holding the IN-VOLUME linear index
// p = (z - z0) H W + y W + x of another voxel of the same component (z0 = the volume's first slice;
// -1 on the background), with the invariant L[p] <= p.  Row (z, y) is united with its "earlier"
// neighbour rows under in-row offsets:
//
//   connectivity   (z, y-1)     (z-1, y)     (z-1, y-1) and (z-1, y+1)
//        6         {0}          {0}          --
//       18         {-1,0,1}     {-1,0,1}     {0}
//       26         {-1,0,1}     {-1,0,1}     {-1,0,1}
//
// (z-1, .) only when z > z0, y +- 1 only inside [0, H).  Every offset set contains 0.  That is why
// the 2-D de-duplication holds for any pair of rows: with `cur` and `up` the two rows' foreground,
// two runs that touch under {-1,0,1} either overlap in some column (then the first column of the
// overlap is the one pair V picks) or meet only corner to corner (then exactly one of DL / DR fires,
// at the run's end, because `~up` and `~curL` / `~curR` exclude every pair an overlap or a nearer
// column already covers).  Under {0} alone only V applies.  One union per touching pair of runs.
//
// Launches, none of which waits for another workgroup, reads anything back or allocates:
//   init      as ccl.hip: the parent of a voxel is the first voxel of its horizontal run.
//   merge     one wave per row (z, y): the row and up to four neighbour rows as bit words, one
//             find + atomicMin union per touching pair of runs.
//   compress  every voxel's parent becomes its root; area[root] += run segment length (filter).
//   slice     one workgroup per slice walks it in raster order: the number of roots in the slice and
//             (filter) the best key (area << 32) | (0x7FFFFFFF - root) among them.
//   volume    one wave per volume scans its slices: the exclusive prefix of the root counts (the
//             rank before each slice), the volume's component count and its best key's root.
//   rank      (labels) the slice walk again, starting from the slice's prefix: 1-based ranks at the
//             roots.  Raster order (z, y, x) of the roots = of each component's first voxel, which is
//             scipy's numbering.
//   labels / filter   one pass over the voxels writes the output (and the filter's counts).
// The two-level rank pass keeps every workgroup's walk one slice long whatever the depth.
//
// Termination and visibility are ccl.hip's arguments, which never use where a neighbour lies: a
// union only ever lowers a parent to a smaller index of the same component, so L[p] <= p at all
// times and find strictly descends; inside merge a stale parent read names an earlier value of the
// word, i.e. a member of the same component with index >= the current one, and the atomicMin that
// follows executes at the memory side and returns the true word, so the union corrects itself.
// The new neighbour rows change which pairs are united, not these properties; links never leave the
// volume because every index is relative to z0 and no pair spans two volumes.  compress starts
// after merge has finished, the slice / volume / rank passes after compress: launch boundaries
// order them.
//
// Bounds do not depend on the device copy of starts being right: the first slice of a row's volume
// is clamped to [0, z], so every index stays inside [0, the voxel's own index].
//
// Integer only: the same code in both storage builds.
#include "ccl_common.h"
#include "../../include/stfunet.h"

namespace {

constexpr unsigned ROOT_TOP = 0x7FFFFFFFu;   // in-volume indices fit 31 bits

struct Vol {
  int v;        // the volume of slice z
  int z0;       // its first slice, 0 <= z0 <= z
};

// wave-uniform: the largest v with starts[v] <= z
STF_DEV Vol volume_of(const int* __restrict__ starts, int V, int z) {
  int lo = 0, hi = V;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (starts[mid] <= z) lo = mid; else hi = mid;
  }
  int z0 = starts[lo];
  if ((unsigned)z0 > (unsigned)z) z0 = z;
  return {lo, z0};
}

// rows = N * H.  L = in-volume index of the first voxel of the voxel's horizontal run, -1 on the
// background; area (or NULL) = 0.
__global__ __launch_bounds__(BT) void ccl3d_init_kernel(const uint8_t* __restrict__ mask, long rows, int H, int W,
                                                        const int* __restrict__ starts, int V,
                                                        int* __restrict__ L, int* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                                            // whole waves leave: no barrier below
  const int z = (int)(r / H);
  const int y = (int)(r - (long)z * H);
  const Vol vol = volume_of(starts, V, z);
  const int rowp = ((z - vol.z0) * H + y) * W;                      // < N H W < 2^31
  const long base = r * (long)W;
  const int nw = (W + 63) >> 6;
  int carry = -1;                       // start of the run that reaches the previous chunk's last pixel
  for (int c = 0; c < nw; ++c) {
    const int x = c * 64 + lane;
    const bool in = x < W;
    const bool fg = in && mask[base + x] != 0;
    const u64 w = __ballot(fg);
    const u64 zeros_below = ~w & ((1ull << lane) - 1);
    const int start = zeros_below ? c * 64 + 64 - __builtin_clzll(zeros_below) : (carry >= 0 ? carry : c * 64);
    if (in) {
      L[base + x] = fg ? rowp + start : -1;
      if (area) area[base + x] = 0;
    }
    const int last = __shfl(start, 63, 64);
    carry = (w >> 63) ? last : -1;
  }
}

// One union per touching pair of runs of the row `cur` (in-volume index of its first voxel: rowp)
// and the neighbour row `up`, which lies `delta` voxels earlier; diag: offsets {-1, 0, 1}, else {0}.
STF_DEV void merge_rows(int* Lv, u64 cur, u64 curL, u64 curR, const uint8_t* __restrict__ uprow, int W, int lane,
                        int rowp, int delta, bool diag) {
  const u64 up = row_word(uprow, W, lane);
  const u64 upL = (up << 1) | (shfl_up1(up, lane) >> 63);           // bit i = voxel x - 1
  const u64 upR = (up >> 1) | (shfl_down1(up, lane) << 63);         // bit i = voxel x + 1
  const u64 Vt = cur & up & ~(curL & upL);
  const u64 DL = diag ? cur & upL & ~up & ~curL : 0ull;
  const u64 DR = diag ? cur & upR & ~up & ~curR : 0ull;
  const int nw = (W + 63) >> 6;
  for (int c = 0; c < nw; ++c) {
    const u64 v = __shfl(Vt, c, 64), dl = __shfl(DL, c, 64), dr = __shfl(DR, c, 64);
    if (!(v | dl | dr)) continue;                                   // wave-uniform
    const int p = rowp + c * 64 + lane;
    if ((v >> lane) & 1) unite(Lv, p, p - delta);
    if ((dl >> lane) & 1) unite(Lv, p, p - delta - 1);              // x >= 1: bit 0 of word 0 of upL is zero
    if ((dr >> lane) & 1) unite(Lv, p, p - delta + 1);              // x + 1 < W: up has no bit at x >= W
  }
}

// level = 1, 2, 3 for connectivity 6, 18, 26
__global__ __launch_bounds__(BT) void ccl3d_merge_kernel(const uint8_t* __restrict__ mask, long rows, int H, int W,
                                                         const int* __restrict__ starts, int V, int level, int* L) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int z = (int)(r / H);
  const int y = (int)(r - (long)z * H);
  const Vol vol = volume_of(starts, V, z);
  const bool above = y > 0, below = y + 1 < H, back = z > vol.z0;   // wave-uniform
  if (!above && !back) return;
  const int HW = H * W;
  int* Lv = L + (long)vol.z0 * HW;
  const uint8_t* row = mask + r * (long)W;
  const int rowp = ((z - vol.z0) * H + y) * W;
  const u64 cur = row_word(row, W, lane);
  const u64 curL = (cur << 1) | (shfl_up1(cur, lane) >> 63);
  const u64 curR = (cur >> 1) | (shfl_down1(cur, lane) << 63);
  if (above) merge_rows(Lv, cur, curL, curR, row - W, W, lane, rowp, W, level >= 2);
  if (back) {
    const uint8_t* prev = row - (long)HW;
    merge_rows(Lv, cur, curL, curR, prev, W, lane, rowp, HW, level >= 2);
    if (level >= 2) {
      if (above) merge_rows(Lv, cur, curL, curR, prev - W, W, lane, rowp, HW + W, level >= 3);
      if (below) merge_rows(Lv, cur, curL, curR, prev + W, W, lane, rowp, HW - W, level >= 3);
    }
  }
}

// L[g] = root of the voxel, in place.  area (or NULL; zero on entry): area[root] += voxels, per run
// segment of a chunk or per row (below).  A volume's area is below 2^31: it fits the int32 word.
__global__ __launch_bounds__(BT) void ccl3d_compress_kernel(long rows, int H, int W, const int* __restrict__ starts,
                                                            int V, int* L, int* area) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int z = (int)(r / H);
  const Vol vol = volume_of(starts, V, z);
  const long vbase = (long)vol.z0 * H * W;
  int* Lv = L + vbase;
  const int nw = (W + 63) >> 6;
  int hot = -1, hot_sum = 0;            // wave-uniform: a root and the voxels of this row collected for it
  for (int c = 0; c < nw; ++c) {
    const int x = c * 64 + lane;
    const int v = x < W ? L[r * (long)W + x] : -1;
    const bool fg = v >= 0;
    int root = v;
    if (fg) {
      root = find_root<false>(Lv, v);
      L[r * (long)W + x] = root;
    }
    if (area) {
      // A volume-spanning component would take one add per run segment of the whole volume at one
      // address.  The segments of the chunk's first root are summed in the wave and carried along
      // the row while the next chunk starts with the same root; the other segments add on their own.
      const u64 w = __ballot(fg);
      const bool first = fg && (lane == 0 || !((w >> (lane - 1)) & 1));
      const u64 t = ~(w >> lane);                                   // zero only for lane 0 of a full word
      const int len = first ? (t ? __builtin_ctzll(t) : 64) : 0;
      const u64 adds = __ballot(first);
      if (adds) {                                                   // wave-uniform
        const int r0 = __shfl(root, __builtin_ctzll(adds), 64);
        const bool same = first && root == r0;
        const int s = wave_sum_i(same ? len : 0);
        if (r0 != hot) {
          if (lane == 0 && hot_sum) atomicAdd(&area[vbase + hot], hot_sum);
          hot = r0;
          hot_sum = 0;
        }
        hot_sum += s;
        if (first && !same) atomicAdd(&area[vbase + root], len);
      }
    }
  }
  if (area && lane == 0 && hot_sum) atomicAdd(&area[vbase + hot], hot_sum);
}

// One workgroup per slice walks it in raster order; "is a root" (L[g] == the voxel's own in-volume
// index) is scanned exclusively with a carry.
//   COUNT   cnt[z] = roots in the slice; best (or NULL) [z] = the largest key
//           (area << 32) | (ROOT_TOP - root) among them, 0 without a root (areas are >= 1).
//   !COUNT  aux[root] = 1-based rank in the volume, the carry starting at cnt[z], which by then
//           holds the roots of the volume's earlier slices (ccl3d_volume_kernel).
template <bool COUNT>
__global__ __launch_bounds__(RT) void ccl3d_slice_kernel(const int* __restrict__ L, int* __restrict__ aux, int HW,
                                                         const int* __restrict__ starts, int V, int* __restrict__ cnt,
                                                         u64* __restrict__ bestz) {
  __shared__ int wtot[RT / 64];
  __shared__ u64 wbest[RT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int z = blockIdx.x;
  const Vol vol = volume_of(starts, V, z);
  const int own = (z - vol.z0) * HW;                                // in-volume index of the slice's first voxel
  const int* Lz = L + (long)z * HW;
  int* Av = aux + (long)vol.z0 * HW;
  int carry = COUNT ? 0 : cnt[z];
  u64 best = 0;
  for (int base = 0; base < HW; base += RT * NK) {
    const int i0 = base + tid * NK;
    bool root[NK];
    int c = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      root[k] = i0 + k < HW && Lz[i0 + k] == own + i0 + k;
      c += root[k];
    }
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wtot[wv] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RT / 64; ++w) {
      const int t = wtot[w];
      before += w < wv ? t : 0;
      total += t;
    }
    int run = carry + before + inc - c;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if (!root[k]) continue;
      ++run;
      const int p = own + i0 + k;
      if (COUNT) {
        if (bestz) {
          const u64 key = ((u64)(unsigned)Av[p] << 32) | (u64)(ROOT_TOP - (unsigned)p);
          best = key > best ? key : best;
        }
      } else {
        Av[p] = run;
      }
    }
    carry += total;
    __syncthreads();                                                // wtot is free again
  }
  if (!COUNT) return;
  if (bestz) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 t = __shfl_xor(best, o, 64);
      best = t > best ? t : best;
    }
    if (lane == 0) wbest[wv] = best;
    __syncthreads();
  }
  if (tid != 0) return;
  cnt[z] = carry;
  if (bestz) {
    for (int w = 1; w < RT / 64; ++w) best = wbest[w] > best ? wbest[w] : best;
    bestz[z] = best;
  }
}

// One wave per volume over its slices in order: cnt[z] becomes the number of roots in the volume's
// earlier slices, num (or NULL) [v] the volume's total; with bestz, sel[v] = the root of the largest
// key (-1 without a component).
__global__ __launch_bounds__(64) void ccl3d_volume_kernel(const int* __restrict__ starts, int N, int* __restrict__ cnt,
                                                          const u64* __restrict__ bestz, int* __restrict__ num,
                                                          int* __restrict__ sel) {
  const int lane = threadIdx.x, v = blockIdx.x;
  int za = starts[v], zb = starts[v + 1];
  za = za < 0 ? 0 : za;
  zb = zb > N ? N : zb;
  int carry = 0;
  u64 best = 0;
  for (int z0 = za; z0 < zb; z0 += 64) {
    const int z = z0 + lane;
    const int c = z < zb ? cnt[z] : 0;
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (z < zb) {
      cnt[z] = carry + inc - c;
      if (bestz) best = bestz[z] > best ? bestz[z] : best;
    }
    carry += __shfl(inc, 63, 64);
  }
  if (bestz) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 t = __shfl_xor(best, o, 64);
      best = t > best ? t : best;
    }
  }
  if (lane != 0) return;
  if (num) num[v] = carry;
  if (bestz) sel[v] = best ? (int)(ROOT_TOP - (unsigned)(best & 0xFFFFFFFFull)) : -1;
}

__global__ __launch_bounds__(BT) void ccl3d_labels_kernel(const int* __restrict__ L, const int* __restrict__ rank,
                                                          long rows, int H, int W, const int* __restrict__ starts,
                                                          int V, int* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const Vol vol = volume_of(starts, V, (int)(r / H));
  const int* Rv = rank + (long)vol.z0 * H * W;
  for (int x = lane; x < W; x += 64) {
    const long i = r * (long)W + x;
    const int v = L[i];
    labels[i] = v < 0 ? 0 : Rv[v];
  }
}

constexpr int FR = 16;                  // rows of one slice per wave of the filter pass

// out = mask where the voxel's component passes, 0 elsewhere; counts (or NULL; zero on entry)
// [V][3] += (|P' & T|, |P'|, |T|) with stf_predict_mask's rules.  One wave per group of FR rows of one
// slice (groups = N * ceil(H / FR)): a volume's three words take one add per group, not per row.
__global__ __launch_bounds__(BT) void ccl3d_filter_kernel(const uint8_t* __restrict__ mask,
                                                          const int64_t* __restrict__ target, long groups, int H, int W,
                                                          const int* __restrict__ starts, int V,
                                                          const int* __restrict__ L, const int* __restrict__ area,
                                                          const int* __restrict__ sel, int keep_largest, long min_size,
                                                          long ignore, uint8_t* __restrict__ out,
                                                          u64* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (g >= groups) return;
  const int per = (H + FR - 1) / FR;
  const int z = (int)(g / per);
  const int y0 = (int)(g - (long)z * per) * FR;
  const int y1 = y0 + FR < H ? y0 + FR : H;
  const Vol vol = volume_of(starts, V, z);
  const int* Av = area + (long)vol.z0 * H * W;
  const int largest = keep_largest ? sel[vol.v] : -1;
  int ni = 0, np = 0, nt = 0;
  for (int y = y0; y < y1; ++y) {
    const long row = ((long)z * H + y) * W;
    for (int x = lane; x < W; x += 64) {
      const long i = row + x;
      const int v = L[i];
      const bool pass = v >= 0 && (long)Av[v] >= min_size && (!keep_largest || v == largest);
      const uint8_t m = pass ? mask[i] : (uint8_t)0;
      out[i] = m;
      if (counts) {
        const long tv = target[i];
        const bool keep = !(ignore >= 0 && tv == ignore);
        const bool p = keep && m != 0, t = keep && tv > 0;
        ni += p && t;
        np += p;
        nt += t;
      }
    }
  }
  if (!counts) return;                                              // wave-uniform
  ni = wave_sum_i(ni);
  np = wave_sum_i(np);
  nt = wave_sum_i(nt);
  if (lane == 0 && ni) atomicAdd(&counts[vol.v * 3], (u64)ni);
  if (lane == 1 && np) atomicAdd(&counts[vol.v * 3 + 1], (u64)np);
  if (lane == 2 && nt) atomicAdd(&counts[vol.v * 3 + 2], (u64)nt);
}

// N, H, W, V inside the limits and N * H * W < 2^31
inline bool sizes_ok(int N, int H, int W, int V) {
  if (N < 1 || H < 1 || W < 1 || H > MAXDIM || W > MAXDIM || V < 1 || V > N) return false;
  return (long)N * H * W < (1L << 31);
}

// strictly ascending from 0 to N
inline bool starts_ok(const int32_t* starts, int V, int N) {
  if (starts[0] != 0 || starts[V] != N) return false;
  for (int v = 0; v < V; ++v)
    if (starts[v] >= starts[v + 1]) return false;
  return true;
}

inline int level_of(int connectivity) { return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0; }

// scratch: [selected root int32 [V], 256-B rounded][roots per slice int32 [N], 256-B rounded]
//          [best key per slice u64 [N], 256-B rounded][parents int32 [n]][ranks or areas int32 [n]]
struct Scratch {
  int* sel;
  int* cnt;
  u64* best;
  int* L;
  int* aux;
};
inline size_t head_bytes(int N, int V) {
  return round_up((size_t)V * sizeof(int), 256) + round_up((size_t)N * sizeof(int), 256) +
         round_up((size_t)N * sizeof(u64), 256);
}
inline Scratch carve(void* scratch, int N, int V, long n) {
  char* p = (char*)scratch;
  Scratch s;
  s.sel = (int*)p;
  p += round_up((size_t)V * sizeof(int), 256);
  s.cnt = (int*)p;
  p += round_up((size_t)N * sizeof(int), 256);
  s.best = (u64*)p;
  p += round_up((size_t)N * sizeof(u64), 256);
  s.L = (int*)p;
  s.aux = s.L + n;
  return s;
}

// init, merge, compress: afterwards L holds every voxel's root (and aux the areas when with_area)
int label_roots(const uint8_t* mask, int N, int H, int W, const int* starts, int V, int level, const Scratch& sc,
                bool with_area, hipStream_t s) {
  const long rows = (long)N * H;
  int* area = with_area ? sc.aux : nullptr;
  hipLaunchKernelGGL(ccl3d_init_kernel, dim3(row_grid(rows)), dim3(BT), 0, s, mask, rows, H, W, starts, V, sc.L,
                     area);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl3d_merge_kernel, dim3(row_grid(rows)), dim3(BT), 0, s, mask, rows, H, W, starts, V, level,
                     sc.L);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl3d_compress_kernel, dim3(row_grid(rows)), dim3(BT), 0, s, rows, H, W, starts, V, sc.L, area);
  STF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t stf_ccl3d_scratch_bytes(int N, int H, int W, int V) {
  if (!sizes_ok(N, H, W, V)) return 0;
  const size_t n = (size_t)N * H * W;
  return round_up(head_bytes(N, V) + n * 2 * sizeof(int), 8);
}

extern "C" int stf_ccl3d_label(const uint8_t* mask, int N, int H, int W, const int32_t* starts_dev,
                               const int32_t* starts_host, int V, int connectivity, int32_t* labels, int32_t* num,
                               void* scratch, stf_stream_t stream) {
  if (!mask || !starts_dev || !starts_host || !labels || !num || !scratch || !sizes_ok(N, H, W, V))
    return STF_EINVAL;
  const int level = level_of(connectivity);
  if (!level) return STF_EINVAL;
  if (((uintptr_t)scratch & 7) || ((uintptr_t)labels & 3) || ((uintptr_t)num & 3) || ((uintptr_t)starts_dev & 3) ||
      ((uintptr_t)starts_host & 3))
    return STF_EINVAL;
  if (!starts_ok(starts_host, V, N)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)N * H * W, rows = (long)N * H;
  const Scratch sc = carve(scratch, N, V, n);
  const int rc = label_roots(mask, N, H, W, starts_dev, V, level, sc, false, s);
  if (rc) return rc;
  hipLaunchKernelGGL(ccl3d_slice_kernel<true>, dim3((unsigned)N), dim3(RT), 0, s, (const int*)sc.L, sc.aux, H * W,
                     starts_dev, V, sc.cnt, (u64*)nullptr);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl3d_volume_kernel, dim3((unsigned)V), dim3(64), 0, s, starts_dev, N, sc.cnt,
                     (const u64*)nullptr, num, sc.sel);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl3d_slice_kernel<false>, dim3((unsigned)N), dim3(RT), 0, s, (const int*)sc.L, sc.aux, H * W,
                     starts_dev, V, sc.cnt, (u64*)nullptr);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl3d_labels_kernel, dim3(row_grid(rows)), dim3(BT), 0, s, (const int*)sc.L, (const int*)sc.aux,
                     rows, H, W, starts_dev, V, labels);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_ccl3d_filter(const uint8_t* mask, const int64_t* target, int N, int H, int W,
                                const int32_t* starts_dev, const int32_t* starts_host, int V, int connectivity,
                                int keep_largest, int64_t min_size, int64_t ignore_index, uint8_t* out, int64_t* counts,
                                int32_t* num, void* scratch, stf_stream_t stream) {
  if (!mask || !starts_dev || !starts_host || !out || !scratch || !sizes_ok(N, H, W, V)) return STF_EINVAL;
  const int level = level_of(connectivity);
  if (!level || min_size < 0 || (counts && !target) || out == mask) return STF_EINVAL;
  if (((uintptr_t)scratch & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)target & 7) || ((uintptr_t)num & 3) ||
      ((uintptr_t)starts_dev & 3) || ((uintptr_t)starts_host & 3))
    return STF_EINVAL;
  if (!starts_ok(starts_host, V, N)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)N * H * W;
  const Scratch sc = carve(scratch, N, V, n);
  if (counts) {
    hipError_t e = stf::memset_async(counts, 0, (size_t)V * 3 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
  }
  const int rc = label_roots(mask, N, H, W, starts_dev, V, level, sc, true, s);
  if (rc) return rc;
  hipLaunchKernelGGL(ccl3d_slice_kernel<true>, dim3((unsigned)N), dim3(RT), 0, s, (const int*)sc.L, sc.aux, H * W,
                     starts_dev, V, sc.cnt, sc.best);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl3d_volume_kernel, dim3((unsigned)V), dim3(64), 0, s, starts_dev, N, sc.cnt,
                     (const u64*)sc.best, num, sc.sel);
  STF_CHECK_LAUNCH();
  const long groups = (long)N * ((H + FR - 1) / FR);
  hipLaunchKernelGGL(ccl3d_filter_kernel, dim3(row_grid(groups)), dim3(BT), 0, s, mask, counts ? target : nullptr,
                     groups, H, W, starts_dev, V, (const int*)sc.L, (const int*)sc.aux, (const int*)sc.sel,
                     keep_largest ? 1 : 0, (long)min_size, (long)ignore_index, out, (u64*)counts);
  STF_CHECK_LAUNCH();
  return 0;
}
