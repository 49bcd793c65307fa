// Connected components of binary masks on the device:
// labels in scipy.ndimage.label's numbering, and the post-processing filter of the usual
// segmentation recipe (keep the largest component, drop components below a size) with the counts
// of the filtered mask.  One kernel family serves two geometries, chosen at compile time (VOL):
//   volumes  the uint8 [N][H][W] stack is cut into V volumes of consecutive slices by starts
//            int32 [V + 1] (strictly ascending, starts[0] = 0, starts[V] = N; the host copy is
//            validated, the device copy is what the kernels read); connectivity 6 / 18 / 26 is
//            scipy's generate_binary_structure(3, 1 | 2 | 3).
//   images   every slice is a volume one slice deep: {v = z, z0 = z} with no table, no search and
//            no earlier slice; connectivity 4 / 8 is generate_binary_structure(2, 1 | 2).
// Every volume is labelled on its own: foreground is mask != 0, outside the volume is background.
//
// State.  One int32 parent per voxel, L[g], holding the IN-VOLUME linear index
// p = (z - z0) H W + y W + x of another voxel of the same component (z0 = the volume's first slice;
// -1 on the background).  Invariant: L[p] <= p at all times, and L[p] is a member of p's component.
//
// Neighbours.  Row (z, y) is united with its "earlier" neighbour rows under in-row offsets:
//
//   level  connectivity   (z, y-1)     (z-1, y)     (z-1, y-1) and (z-1, y+1)
//     1      4 |  6       {0}          {0}          --
//     2      8 | 18       {-1,0,1}     {-1,0,1}     {0}
//     3        | 26       {-1,0,1}     {-1,0,1}     {-1,0,1}
//
// (z-1, .) only when z > z0 -- never for an image, whose rows of the table end after the first
// column -- and y +- 1 only inside [0, H).  Every offset set contains 0.  That is why one
// de-duplication holds for any pair of rows: with `cur` and `up` the two rows' foreground, two runs
// that touch under {-1,0,1} either overlap in some column (then the first column of the overlap is
// the one pair V picks) or meet only corner to corner (then exactly one of DL / DR fires, at the
// run's end, because `~up` and `~curL` / `~curR` exclude every pair an overlap or a nearer column
// already covers).  Under {0} alone only V applies.  One union per touching pair of runs.
//
// Launches, none of which waits for another workgroup, reads anything back or allocates:
//   init      one wave per row walks the row's 64-voxel chunks.  The foreground of a chunk is a
//             ballot word; every voxel's parent is the first voxel of its horizontal run (clz on the
//             zeros below the lane; a run that reaches the chunk's first voxel inherits the start the
//             wave carries over the seam).  Only run starts are ever roots, so only they are ever the
//             target of an atomic.  Zeroes the area words when the filter needs them.
//   merge     one wave per row: the row and up to four neighbour rows as bit words (lane c keeps
//             word c), one find + atomicMin union per touching pair of runs (merge_rows).
//   compress  every voxel's parent becomes its root; area[root] += run segment lengths (filter).
//   rank      images: one workgroup per image walks it in raster order with a carry (root_walk):
//             "is a root" (L[p] == p) is scanned exclusively; the labels store the 1-based rank at
//             the root, the filter selects the largest key (area << 32) | (0x7FFFFFFF - root) in the
//             same walk -- the largest area, ties to the smaller root; the carry's final value is
//             the number of components.  Volumes: the same walk per slice, in two levels, so that a
//             workgroup's walk stays one slice long whatever the depth: `slice` counts each slice's
//             roots (and finds its best key), `volume` (one wave per volume) turns the counts into
//             the rank before each slice, the volume's total and its best key's root, and for the
//             labels `slice` walks again from that prefix.  Raster order (z, y, x) of the roots = of
//             each component's first voxel: scipy's numbering.
//   labels / filter   one pass over the voxels writes the output (and the filter's counts).
// Images: five launches for the labels, five and the counts' memset for the filter.  Volumes: seven,
// and six and the memset.
//
// Termination.  find walks v -> L[v] while L[v] < v, so v strictly decreases; unite replaces the pair
// (a, b) by two indices below max(a, b) (see unite).  Both compare unsigned and stop on any word
// that broke the invariant, so no memory content can make them loop or leave the volume.
//
// Order-free result.  Integer atomics only.  Every link points from a larger index to a smaller one
// of the same component, so the root of a tree is the smallest index of its component whatever
// order the atomics arrive in; ranks, areas (integer adds) and the selection follow from the roots.
//
// Visibility.  Launch boundaries make each launch's stores visible to the next, so only merge has
// concurrent writers of words it reads.  There a parent read may be stale (another XCD's L2, this
// CU's L1): a stale value is a value L[p] held earlier in the launch, so it is >= the current one and
// names a member of the same component.  A find over stale values therefore ends at a member of the
// right component that may no longer be a root; the union corrects that itself, because its
// atomicMin executes at the memory side and returns the word's true value (see unite).  Parents are
// nevertheless read with relaxed agent-scope atomic loads in merge, which skip the stale copies and
// save iterations; correctness does not rest on it.  compress starts after merge has finished:
// roots no longer change, and its in-place stores replace a parent by another ancestor of the same
// tree, so a concurrent find that reads either value still reaches the root.
// None of these arguments uses where a neighbour lies: which rows merge unites changes the
// partition, not the properties.  Links never leave the volume because every index is relative to
// z0 and no united pair spans two volumes.
//
// Bounds do not depend on the device copy of starts being right: the first slice of a row's volume
// is clamped to [0, z], so every index stays inside [0, the voxel's own index], and the volume
// number stays inside [0, V).
//
// Integer only: the same code in both storage builds.
#include "common.h"
#include "probs.h"
#include "volumes.h"
#include "../../include/stfunet.h"

namespace {

using stf::Vol;
using stf::volume_of;
using stf::starts_ok;

constexpr int BT = 256;                 // threads per workgroup of the row passes: one wave per row
constexpr int RT = 1024;                // threads of the raster walks
constexpr int NK = 4;                   // consecutive voxels per thread and step of the walks
constexpr int MAXDIM = 4096;
constexpr unsigned ROOT_TOP = 0x7FFFFFFFu;   // in-volume indices fit 31 bits

typedef unsigned long long u64;

STF_DEV u64 shfl_up1(u64 v, int lane) {
  const u64 t = __shfl_up(v, 1, 64);
  return lane == 0 ? 0ull : t;
}
STF_DEV u64 shfl_down1(u64 v, int lane) {
  const u64 t = __shfl_down(v, 1, 64);
  return lane == 63 ? 0ull : t;
}

// The foreground of one row as bit words, lane c keeping word c (W <= 4096 = 64 words); bits at
// x >= W are zero.
STF_DEV u64 row_word(const uint8_t* __restrict__ row, int W, int lane) {
  const int nw = (W + 63) >> 6;
  u64 mine = 0;
  for (int c = 0; c < nw; ++c) {
    const int x = c * 64 + lane;
    const u64 w = __ballot(x < W && row[x] != 0);
    if (lane == c) mine = w;
  }
  return mine;
}

// The root of foreground voxel v.  ATOMIC: relaxed agent-scope loads (merge, concurrent writers);
// otherwise plain loads (compress).
template <bool ATOMIC>
STF_DEV int find_root(const int* L, int v) {
  for (;;) {
    const int p = ATOMIC ? __hip_atomic_load(L + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : L[v];
    if ((unsigned)p >= (unsigned)v) return v;
    v = p;
  }
}

// Unite the components of foreground voxels a and b.
// Terminates on its own: every turn replaces the pair (a, b) by (old, lo) with old < hi and
// lo < hi, so max(a, b) strictly decreases and is bounded by 0; no turn waits for another thread.
// Correct whatever find returned, as long as a and b are members of the two components: if hi was a
// root, the atomicMin links it under lo and the two trees are one.  If it was not (another thread
// linked it first, or find read a stale parent), the atomicMin returns its true parent old and leaves
// L[hi] = min(old, lo); either way hi stays linked to one of the two and the other two, old and lo,
// remain to be united, which the next turn does.
STF_DEV void unite(int* L, int a, int b) {
  a = find_root<true>(L, a);
  b = find_root<true>(L, b);
  while (a != b) {
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicMin(&L[hi], lo);
    if ((unsigned)old >= (unsigned)hi) break;                       // hi was a root: linked
    a = old;
    b = lo;
  }
}

// wave_sum_i and wave_max: common.h

// The keep-largest key: the largest area wins, ties go to the smaller root; 0 = no component
// (areas are >= 1).
STF_DEV u64 key_of(int area, int root) { return ((u64)(unsigned)area << 32) | (u64)(ROOT_TOP - (unsigned)root); }
STF_DEV int root_of(u64 key) { return key ? (int)(ROOT_TOP - (unsigned)(key & 0xFFFFFFFFull)) : -1; }

// Vol and volume_of<VOL> (volumes.h): the volume of slice z and its first slice; images: {z, z}.

// rows = N * H.  L = in-volume index of the first voxel of the voxel's horizontal run, -1 on the
// background; area (or NULL) = 0.
template <bool VOL>
__global__ __launch_bounds__(BT) void ccl_init_kernel(const uint8_t* __restrict__ mask, long rows, int H, int W,
                                                      const int* __restrict__ starts, int V, int* __restrict__ L,
                                                      int* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                                            // whole waves leave: no barrier below
  const int z = (int)(r / H);
  const int y = (int)(r - (long)z * H);
  const Vol vol = volume_of<VOL>(starts, V, z);
  const int rowp = ((z - vol.z0) * H + y) * W;                      // < N H W < 2^31
  const long base = r * (long)W;
  const int nw = (W + 63) >> 6;
  int carry = -1;                       // start of the run that reaches the previous chunk's last voxel
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

// The only union picker: one union per touching pair of runs of the row `cur` (in-volume index of
// its first voxel: rowp) and the neighbour row `up`, which lies `delta` voxels earlier; diag: offsets
// {-1, 0, 1}, else {0}.
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

// level: the row of the neighbour table.  An image has no earlier slice: only (z, y-1) remains.
template <bool VOL>
__global__ __launch_bounds__(BT) void ccl_merge_kernel(const uint8_t* __restrict__ mask, long rows, int H, int W,
                                                       const int* __restrict__ starts, int V, int level, int* L) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int z = (int)(r / H);
  const int y = (int)(r - (long)z * H);
  const Vol vol = volume_of<VOL>(starts, V, z);
  const bool above = y > 0, below = y + 1 < H, back = VOL && z > vol.z0;   // wave-uniform
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
// segment of a chunk or, with CARRY, per row (below).  A volume's area is below 2^31: it fits the
// int32 word.  Images add per segment: measured at 256 x 256, the carried sum halves the time of a
// percolation mask's filter but costs the checkerboard's 4 to 6 % (profiles/ccl_family/README.md).
template <bool VOL, bool CARRY>
__global__ __launch_bounds__(BT) void ccl_compress_kernel(long rows, int H, int W, const int* __restrict__ starts,
                                                          int V, int* L, int* area) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const Vol vol = volume_of<VOL>(starts, V, (int)(r / H));
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
      const u64 w = __ballot(fg);
      const bool first = fg && (lane == 0 || !((w >> (lane - 1)) & 1));
      const u64 t = ~(w >> lane);                                   // zero only for lane 0 of a full word
      const int len = first ? (t ? __builtin_ctzll(t) : 64) : 0;
      // A spanning component would take one add per run segment of the whole volume at one
      // address.  With CARRY the segments of the chunk's first root are summed in the wave and
      // carried along the row while the next chunk starts with the same root; the other segments
      // add on their own, as all of them do without CARRY.
      const u64 adds = CARRY ? __ballot(first) : 0ull;
      if (!CARRY) {
        if (first) atomicAdd(&area[vbase + root], len);
      } else if (adds) {                                            // wave-uniform
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

// The raster walk of one workgroup of RT threads over one slice: word i of Lz (i < HW) is a root
// when it holds its own in-volume index own + i.  "Is a root" is scanned exclusively, starting at
// `carry`; every root p is handed to at_root(p, its 1-based rank), and the return value is carry +
// the slice's roots, in every thread.
template <class F>
STF_DEV int root_walk(const int* Lz, int HW, int own, int carry, F at_root) {
  __shared__ int wtot[RT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
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
      at_root(own + i0 + k, run);
    }
    carry += total;
    __syncthreads();                                                // wtot is free again
  }
  return carry;
}

// The workgroup's largest key in two steps: every thread of the RT publishes (each wave's maximum
// goes to wbest, a barrier follows), then thread 0 folds the waves' maxima into its own.
STF_DEV u64 publish_max(u64 best, u64* wbest) {
  best = wave_max(best);
  if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
  __syncthreads();
  return best;
}
STF_DEV u64 fold_max(u64 best, const u64* wbest) {
  for (int w = 1; w < RT / 64; ++w) best = wbest[w] > best ? wbest[w] : best;
  return best;
}

// Images: one workgroup per image.  !SELECT: aux[root] = 1-based rank of the root in raster order.
// SELECT: aux holds the areas; sel[b] = the root of the largest key (-1 without a component).
// num (or NULL) [b] = number of roots.
template <bool SELECT>
__global__ __launch_bounds__(RT) void ccl_scan_kernel(const int* __restrict__ L, int* __restrict__ aux, int HW,
                                                      int* __restrict__ num, int* __restrict__ sel) {
  __shared__ u64 wbest[RT / 64];
  const int b = blockIdx.x;
  int* Ai = aux + (long)b * HW;
  u64 best = 0;
  const int n = root_walk(L + (long)b * HW, HW, 0, 0, [&](int p, int rank) {
    if (SELECT) {
      const u64 key = key_of(Ai[p], p);
      best = key > best ? key : best;
    } else {
      Ai[p] = rank;
    }
  });
  if (SELECT) best = publish_max(best, wbest);
  if (threadIdx.x != 0) return;
  if (num) num[b] = n;
  if (SELECT) sel[b] = root_of(fold_max(best, wbest));
}

// Volumes: one workgroup per slice.
//   COUNT   cnt[z] = roots in the slice; bestz (or NULL) [z] = the largest key among them.
//   !COUNT  aux[root] = 1-based rank in the volume, the carry starting at cnt[z], which by then
//           holds the roots of the volume's earlier slices (ccl3d_volume_kernel).
template <bool COUNT>
__global__ __launch_bounds__(RT) void ccl_slice_kernel(const int* __restrict__ L, int* __restrict__ aux, int HW,
                                                       const int* __restrict__ starts, int V, int* __restrict__ cnt,
                                                       u64* __restrict__ bestz) {
  __shared__ u64 wbest[RT / 64];
  const int z = blockIdx.x;
  const Vol vol = volume_of<true>(starts, V, z);
  int* Av = aux + (long)vol.z0 * HW;
  u64 best = 0;
  const int n = root_walk(L + (long)z * HW, HW, (z - vol.z0) * HW, COUNT ? 0 : cnt[z], [&](int p, int rank) {
    if (COUNT) {
      if (bestz) {
        const u64 key = key_of(Av[p], p);
        best = key > best ? key : best;
      }
    } else {
      Av[p] = rank;
    }
  });
  if (!COUNT) return;
  if (bestz) best = publish_max(best, wbest);                       // workgroup-uniform
  if (threadIdx.x != 0) return;
  cnt[z] = n;
  if (bestz) bestz[z] = fold_max(best, wbest);
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
  if (bestz) best = wave_max(best);
  if (lane != 0) return;
  if (num) num[v] = carry;
  if (bestz) sel[v] = root_of(best);
}

template <bool VOL>
__global__ __launch_bounds__(BT) void ccl_labels_kernel(const int* __restrict__ L, const int* __restrict__ rank,
                                                        long rows, int H, int W, const int* __restrict__ starts,
                                                        int V, int* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const Vol vol = volume_of<VOL>(starts, V, (int)(r / H));
  const int* Rv = rank + (long)vol.z0 * H * W;
  for (int x = lane; x < W; x += 64) {
    const long i = r * (long)W + x;
    const int v = L[i];
    labels[i] = v < 0 ? 0 : Rv[v];
  }
}

// rows of one slice per wave of the filter pass: a volume's three count words take one add per
// group, not per row; an image's rows are few enough
template <bool VOL>
constexpr int FR = VOL ? 16 : 1;

// out = mask where the voxel's component passes, 0 elsewhere; counts (or NULL; zero on entry)
// [V][3] += (|P' & T|, |P'|, |T|) with stf_predict_mask's rules.  One wave per group of R rows of one
// slice (groups = N * ceil(H / R)).
template <bool VOL, int R>
__global__ __launch_bounds__(BT) void ccl_filter_kernel(const uint8_t* __restrict__ mask,
                                                        const int64_t* __restrict__ target, long groups, int H, int W,
                                                        const int* __restrict__ starts, int V,
                                                        const int* __restrict__ L, const int* __restrict__ area,
                                                        const int* __restrict__ sel, int keep_largest, long min_size,
                                                        long ignore, uint8_t* __restrict__ out,
                                                        u64* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long g = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (g >= groups) return;
  const int per = (H + R - 1) / R;
  const int z = (int)(g / per);
  const int y0 = (int)(g - (long)z * per) * R;
  const int y1 = y0 + R < H ? y0 + R : H;
  const Vol vol = volume_of<VOL>(starts, V, z);
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

// ---------------------------------------------------------------- host side
inline size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline unsigned row_grid(long rows) { return (unsigned)((rows + BT / 64 - 1) / (BT / 64)); }

// N, H, W, V inside the limits and N * H * W < 2^31 (images: V = N)
inline bool sizes_ok(int N, int H, int W, int V) { return stf::volume_sizes_ok(N, H, W, V, MAXDIM); }

// What all four entry points refuse before anything is launched, from the arguments they share:
// the row of the neighbour table for `connectivity`, 0 to refuse.  num may be NULL here.
template <bool VOL>
int level_or_refuse(const void* mask, int N, int H, int W, const int32_t* starts_dev, const int32_t* starts_host,
                    int V, int connectivity, const void* num, const void* scratch) {
  if (!mask || !scratch || !sizes_ok(N, H, W, V)) return 0;
  if (((uintptr_t)scratch & 7) || ((uintptr_t)num & 3)) return 0;
  if (VOL) {
    if (!starts_dev || !starts_host || ((uintptr_t)starts_dev & 3) || ((uintptr_t)starts_host & 3)) return 0;
    if (!starts_ok(starts_host, V, N)) return 0;
    return connectivity == 6 ? 1 : connectivity == 18 ? 2 : connectivity == 26 ? 3 : 0;
  }
  return connectivity == 4 ? 1 : connectivity == 8 ? 2 : 0;
}

// scratch: [selected root int32 [V], 256-B rounded]
//          volumes only: [roots per slice int32 [N], 256-B rounded][best key per slice u64 [N], 256-B rounded]
//          [parents int32 [n]][ranks or areas int32 [n]]
struct Scratch {
  int* sel;
  int* cnt;
  u64* best;
  int* L;
  int* aux;
};
template <bool VOL>
size_t scratch_bytes(int N, int H, int W, int V) {
  if (!sizes_ok(N, H, W, V)) return 0;
  size_t head = round_up((size_t)V * sizeof(int), 256);
  if (VOL) head += round_up((size_t)N * sizeof(int), 256) + round_up((size_t)N * sizeof(u64), 256);
  return round_up(head + (size_t)N * H * W * 2 * sizeof(int), 8);
}
template <bool VOL>
Scratch carve(void* scratch, int N, int V, long n) {
  char* p = (char*)scratch;
  Scratch s = {(int*)p, nullptr, nullptr, nullptr, nullptr};
  p += round_up((size_t)V * sizeof(int), 256);
  if (VOL) {
    s.cnt = (int*)p;
    p += round_up((size_t)N * sizeof(int), 256);
    s.best = (u64*)p;
    p += round_up((size_t)N * sizeof(u64), 256);
  }
  s.L = (int*)p;
  s.aux = s.L + n;
  return s;
}

// init, merge, compress: afterwards L holds every voxel's root (and aux the areas when with_area)
template <bool VOL>
int label_roots(const uint8_t* mask, int N, int H, int W, const int* starts, int V, int level, const Scratch& sc,
                bool with_area, hipStream_t s) {
  const long rows = (long)N * H;
  int* area = with_area ? sc.aux : nullptr;
  hipLaunchKernelGGL(ccl_init_kernel<VOL>, dim3(row_grid(rows)), dim3(BT), 0, s, mask, rows, H, W, starts, V, sc.L,
                     area);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl_merge_kernel<VOL>, dim3(row_grid(rows)), dim3(BT), 0, s, mask, rows, H, W, starts, V, level,
                     sc.L);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL((ccl_compress_kernel<VOL, VOL>), dim3(row_grid(rows)), dim3(BT), 0, s, rows, H, W, starts, V,
                     sc.L, area);
  STF_CHECK_LAUNCH();
  return 0;
}

// The rank passes between compress and the output pass.  Afterwards num (or NULL) holds the
// component counts and, with_area, sc.sel the selected roots; otherwise sc.aux holds the ranks.
template <bool VOL>
int rank_roots(int N, int H, int W, const int* starts, int V, const Scratch& sc, bool with_area, int32_t* num,
               hipStream_t s) {
  const int* L = sc.L;
  if (!VOL) {
    if (with_area)
      hipLaunchKernelGGL(ccl_scan_kernel<true>, dim3((unsigned)N), dim3(RT), 0, s, L, sc.aux, H * W, num, sc.sel);
    else
      hipLaunchKernelGGL(ccl_scan_kernel<false>, dim3((unsigned)N), dim3(RT), 0, s, L, sc.aux, H * W, num, sc.sel);
    STF_CHECK_LAUNCH();
    return 0;
  }
  u64* best = with_area ? sc.best : nullptr;
  hipLaunchKernelGGL(ccl_slice_kernel<true>, dim3((unsigned)N), dim3(RT), 0, s, L, sc.aux, H * W, starts, V, sc.cnt,
                     best);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl3d_volume_kernel, dim3((unsigned)V), dim3(64), 0, s, starts, N, sc.cnt, (const u64*)best, num,
                     sc.sel);
  STF_CHECK_LAUNCH();
  if (with_area) return 0;
  hipLaunchKernelGGL(ccl_slice_kernel<false>, dim3((unsigned)N), dim3(RT), 0, s, L, sc.aux, H * W, starts, V, sc.cnt,
                     best);
  STF_CHECK_LAUNCH();
  return 0;
}

template <bool VOL>
int label(const uint8_t* mask, int N, int H, int W, const int32_t* starts_dev, const int32_t* starts_host, int V,
          int connectivity, int32_t* labels, int32_t* num, void* scratch, stf_stream_t stream) {
  const int level = level_or_refuse<VOL>(mask, N, H, W, starts_dev, starts_host, V, connectivity, num, scratch);
  if (!level || !labels || !num || ((uintptr_t)labels & 3)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long rows = (long)N * H;
  const Scratch sc = carve<VOL>(scratch, N, V, rows * W);
  int rc = label_roots<VOL>(mask, N, H, W, starts_dev, V, level, sc, false, s);
  if (rc) return rc;
  rc = rank_roots<VOL>(N, H, W, starts_dev, V, sc, false, num, s);
  if (rc) return rc;
  hipLaunchKernelGGL(ccl_labels_kernel<VOL>, dim3(row_grid(rows)), dim3(BT), 0, s, (const int*)sc.L,
                     (const int*)sc.aux, rows, H, W, starts_dev, V, labels);
  STF_CHECK_LAUNCH();
  return 0;
}

template <bool VOL>
int filter(const uint8_t* mask, const int64_t* target, int N, int H, int W, const int32_t* starts_dev,
           const int32_t* starts_host, int V, int connectivity, int keep_largest, int64_t min_size,
           int64_t ignore_index, uint8_t* out, int64_t* counts, int32_t* num, void* scratch, stf_stream_t stream) {
  const int level = level_or_refuse<VOL>(mask, N, H, W, starts_dev, starts_host, V, connectivity, num, scratch);
  if (!level || !out || min_size < 0 || (counts && !target) || out == mask) return STF_EINVAL;
  if (((uintptr_t)counts & 7) || ((uintptr_t)target & 7)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const Scratch sc = carve<VOL>(scratch, N, V, (long)N * H * W);
  if (counts) {
    hipError_t e = stf::memset_async(counts, 0, (size_t)V * 3 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
  }
  int rc = label_roots<VOL>(mask, N, H, W, starts_dev, V, level, sc, true, s);
  if (rc) return rc;
  rc = rank_roots<VOL>(N, H, W, starts_dev, V, sc, true, num, s);
  if (rc) return rc;
  constexpr int R = FR<VOL>;
  const long groups = (long)N * ((H + R - 1) / R);
  hipLaunchKernelGGL((ccl_filter_kernel<VOL, R>), dim3(row_grid(groups)), dim3(BT), 0, s, mask,
                     counts ? target : nullptr, groups, H, W, starts_dev, V, (const int*)sc.L, (const int*)sc.aux,
                     (const int*)sc.sel, keep_largest ? 1 : 0, (long)min_size, (long)ignore_index, out, (u64*)counts);
  STF_CHECK_LAUNCH();
  return 0;
}

// ---------------------------------------------------------------- lesion-level detection metrics
// INTEGRATION.md 2.2 states the definition, DESIGN.md 5.19 the passes.  Both sides are labelled by the
// passes above in one go: the two binary masks lie behind each other as one stack of 2 N slices,
// target first, and are cut by a doubled table (volumes: starts2 int32 [2 V + 1], entry V + v =
// N + starts[v]; images need none), so side s of volume v is volume s V + v of that stack and no
// component spans two sides.  n = N H W voxels per side.

// The two masks, the doubled table and the zeroed (area << 32 | hit) words of both sides.
template <bool VOL>
__global__ __launch_bounds__(BT) void lesion_form_kernel(const uint8_t* __restrict__ mask,
                                                         const int64_t* __restrict__ target, long n, long ignore,
                                                         const int* __restrict__ starts, int V, int N,
                                                         uint8_t* __restrict__ bin, u64* __restrict__ acc,
                                                         int* __restrict__ starts2) {
  const long i = (long)blockIdx.x * BT + threadIdx.x;
  if (VOL && blockIdx.x == 0)
    for (int v = threadIdx.x; v <= 2 * V; v += BT) {                // either half inside its own side, whatever
      const int z = v == V ? N : starts[v < V ? v : v - V];         // the device table holds
      starts2[v] = (v > V ? N : 0) + (z < 0 ? 0 : z > N ? N : z);
    }
  if (i >= n) return;
  const long tv = target[i];
  const bool keep = !(ignore >= 0 && tv == ignore);
  bin[i] = keep && tv > 0;
  bin[n + i] = keep && mask[i] != 0;
  acc[i] = 0;
  acc[n + i] = 0;
}

// acc[root] += val for the run segments of one chunk (`first` marks a segment's first lane, which
// holds the segment's root and val).  The segments of the chunk's first root are summed in the wave
// and carried along the row (hot, hot_sum: wave-uniform) while the next chunk starts with the same
// root, as ccl_compress_kernel<VOL, true> carries its areas; every other segment adds on its own.
STF_DEV void add_segments(u64* acc, bool first, int root, u64 val, int lane, int& hot, u64& hot_sum) {
  const u64 adds = __ballot(first);
  if (!adds) return;                                                // wave-uniform
  const int r0 = __shfl(root, __builtin_ctzll(adds), 64);
  const bool same = first && root == r0;
  u64 s = same ? val : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (r0 != hot) {
    if (lane == 0 && hot_sum) atomicAdd(&acc[hot], hot_sum);
    hot = r0;
    hot_sum = 0;
  }
  hot_sum += s;
  if (first && !same) atomicAdd(&acc[root], val);
}

// The matching rule, once per root: one double multiply and one compare.
STF_DEV bool lesion_matched(u64 a, double min_overlap) {
  const unsigned area = (unsigned)(a >> 32), hit = (unsigned)a;
  return hit >= 1u && (double)hit >= min_overlap * (double)area;
}

// sc[root] = max(sc[root], val), val > 0.  The word only grows, so a plain load that already shows a
// value >= val settles it without an atomic; a stale load shows an earlier, smaller value and costs
// one redundant atomic, never a result.
STF_DEV void raise_to(int* sc, int root, int val) {
  if (sc[root] < val) atomicMax(&sc[root], val);
}

// sc[root] = max(sc[root], val) for the run segments of one chunk, shaped as add_segments: the
// segments of the chunk's first root are reduced in the wave and the running maximum is carried along
// the row (hot, hot_max: wave-uniform); every other segment raises its word on its own.
STF_DEV void max_segments(int* sc, bool first, int root, int val, int lane, int& hot, int& hot_max) {
  const u64 firsts = __ballot(first);
  if (!firsts) return;                                              // wave-uniform
  const int r0 = __shfl(root, __builtin_ctzll(firsts), 64);
  const bool same = first && root == r0;
  const int m = wave_max(same ? val : 0);
  if (r0 != hot) {
    if (lane == 0 && hot_max) raise_to(sc, hot, hot_max);
    hot = r0;
    hot_max = 0;
  }
  hot_max = m > hot_max ? m : hot_max;
  if (first && !same && val) raise_to(sc, root, val);
}

// One wave per row of the N H rows of one side, after compress (L [2 n] holds roots, -1 on the
// background).  For either side, every run segment of a chunk adds (its length << 32) | (its voxels
// on the other side's foreground) to the word of its root: area < 2^31 and hit <= area, so the two
// halves never carry into each other.  FROC: a segment of the prediction side also raises the
// confidence word of its root (sc [2 n], zero on entry, indexed as acc) to the largest row of its
// voxels (rowp uint16 [n]: row(p) on P).
template <bool VOL, bool FROC>
__global__ __launch_bounds__(BT) void lesion_overlap_kernel(const int* __restrict__ L, long n, long rows, int H, int W,
                                                            const int* __restrict__ starts2, int V, u64* acc,
                                                            const uint16_t* __restrict__ rowp, int* sc) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int z = (int)(r / H), N = (int)(rows / H);
  u64* accs[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) accs[s] = acc + (long)volume_of<VOL>(starts2, 2 * V, s * N + z).z0 * H * W;
  const int nw = (W + 63) >> 6;
  int hot[2] = {-1, -1};
  u64 hot_sum[2] = {0ull, 0ull};
  int* confs = FROC ? sc + (accs[1] - acc) : nullptr;               // the prediction side's words of this volume
  int hot_conf = -1, hot_max = 0;
  for (int c = 0; c < nw; ++c) {
    const int x = c * 64 + lane;
    const long i = r * (long)W + x;
    int root[2];
    u64 fg[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      root[s] = x < W ? L[s * n + i] : -1;
      fg[s] = __ballot(root[s] >= 0);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const u64 w = fg[s];
      const bool first = root[s] >= 0 && (lane == 0 || !((w >> (lane - 1)) & 1));
      const u64 t = ~(w >> lane);                                   // zero only for lane 0 of a full word
      const int len = t ? __builtin_ctzll(t) : 64;
      const u64 seg = (len == 64 ? ~0ull : (1ull << len) - 1) << lane;
      const u64 val = ((u64)len << 32) | (u64)__builtin_popcountll(seg & fg[1 - s]);
      add_segments(accs[s], first, root[s], val, lane, hot[s], hot_sum[s]);
      if (FROC && s == 1) {
        // the segment's maximum on its first lane: a suffix maximum that stops at the segment's last lane
        const int last = lane + len - 1;                            // background: len = 0, nothing is taken
        int mx = root[1] >= 0 ? (int)rowp[i] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_down(mx, o, 64);
          if (lane + o <= last && t > mx) mx = t;
        }
        max_segments(confs, first, root[1], mx, lane, hot_conf, hot_max);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < 2; ++s)
    if (lane == 0 && hot_sum[s]) atomicAdd(&accs[s][hot[s]], hot_sum[s]);
  if (FROC && lane == 0 && hot_max) raise_to(confs, hot_conf, hot_max);
}

// FROC, after overlap (every root's (area, hit) word and confidence are final): one wave per row.  A
// run of voxels of P & T lies in one candidate and one lesion, so its first lane speaks for it: when
// the candidate is matched, the lesion's word (side 0 of sc) is raised to the candidate's confidence.
// Rows where the sides do not overlap cost their two loads.
template <bool VOL>
__global__ __launch_bounds__(BT) void froc_pair_kernel(const int* __restrict__ L, long n, long rows, int H, int W,
                                                       const int* __restrict__ starts2, int V,
                                                       const u64* __restrict__ acc, double min_overlap, int* sc) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int z = (int)(r / H), N = (int)(rows / H);
  const long offT = (long)volume_of<VOL>(starts2, 2 * V, z).z0 * H * W;
  const long offP = (long)volume_of<VOL>(starts2, 2 * V, N + z).z0 * H * W;
  const int nw = (W + 63) >> 6;
  for (int c = 0; c < nw; ++c) {
    const int x = c * 64 + lane;
    const long i = r * (long)W + x;
    const int rt = x < W ? L[i] : -1, rp = x < W ? L[n + i] : -1;
    const bool both = rt >= 0 && rp >= 0;
    const u64 w = __ballot(both);
    if (!w) continue;                                               // wave-uniform
    if (both && (lane == 0 || !((w >> (lane - 1)) & 1))) {          // the first lane of its run
      const int conf = sc[offP + rp];
      if (conf && lesion_matched(acc[offP + rp], min_overlap)) raise_to(sc + offT, rt, conf);
    }
  }
}

// The raster walk of slice z of side blockIdx.y (grid N x 2).  Row rank - 1 of the side's table takes
// (area, hit) of the root with that rank while rank <= max_lesions.
//   images            the whole job: summary {n, matched} of the side, table rows, zeros past n.
//   volumes, COUNT    cnt[z'] = roots of the slice, mat[z'] = matched roots (z' = side N + z).
//   volumes, !COUNT   the table rows, the carry starting at cnt[z'], by then the roots of the volume's
//                     earlier slices (lesion_volume_kernel).
// FROC: a table row has a third column, the root's score word (sc, indexed as acc: det on side 0, conf on
// side 1), and the pass that sees every root once (images; volumes, COUNT) counts the root in its row
// of hist u64 [V][3][bins + 1] (zero on entry): a lesion in side 1, a candidate in side 2 when it is
// matched and in side 0 when not.  The workgroup counts in LDS (dynamic: unsigned [2][bins + 1]; the two
// end rows, where a trained model puts nearly every root, in registers, as curves.hip does) and adds
// each non-zero counter to hist once.
template <bool VOL, bool COUNT, bool FROC>
__global__ __launch_bounds__(RT) void lesion_walk_kernel(const int* __restrict__ L, const u64* __restrict__ acc,
                                                         int N, int HW, const int* __restrict__ starts2, int V,
                                                         int* __restrict__ cnt, int* __restrict__ mat,
                                                         double min_overlap, int max_lesions,
                                                         int64_t* __restrict__ summary, int64_t* __restrict__ table,
                                                         const int* __restrict__ sc, int bins,
                                                         u64* __restrict__ hist) {
  constexpr int COLS = FROC ? 3 : 2;
  constexpr bool HIST = FROC && (!VOL || COUNT);
  extern __shared__ unsigned tab[];
  __shared__ int wmat[RT / 64];
  const int side = blockIdx.y, z2 = side * N + (int)blockIdx.x;
  const Vol vol2 = volume_of<VOL>(starts2, 2 * V, z2);
  const int v = vol2.v - side * V;                                  // the volume in the caller's numbering
  const u64* Av = acc + (long)vol2.z0 * HW;
  const int* Sv = FROC ? sc + (long)vol2.z0 * HW : nullptr;
  int64_t* rowsT = table ? table + ((long)v * 2 + side) * max_lesions * COLS : nullptr;
  int matched = 0;
  unsigned ends[4] = {0, 0, 0, 0};                                  // [matched candidate * 2 + (row == bins)]
  if (HIST) {
    for (int i = threadIdx.x; i < 2 * (bins + 1); i += RT) tab[i] = 0;
    __syncthreads();
  }
  const int n = root_walk(L + (long)z2 * HW, HW, (z2 - vol2.z0) * HW, VOL && !COUNT ? cnt[z2] : 0,
                          [&](int p, int rank) {
    const u64 a = Av[p];
    const bool m = lesion_matched(a, min_overlap);
    if (!VOL || COUNT) matched += m;
    if ((!VOL || !COUNT) && rowsT && rank <= max_lesions) {
      rowsT[(long)(rank - 1) * COLS] = (int64_t)(a >> 32);
      rowsT[(long)(rank - 1) * COLS + 1] = (int64_t)(a & 0xFFFFFFFFull);
      if (FROC) rowsT[(long)(rank - 1) * COLS + 2] = (int64_t)Sv[p];
    }
    if (HIST) {
      int row = Sv[p];
      row = row < 0 ? 0 : row > bins ? bins : row;                  // inside the table whatever the word holds
      const unsigned slot = side && m, lo = row == 0, hi = row == bins;
      ends[0] += lo & (slot ^ 1u);                                  // constant indices: registers
      ends[1] += hi & (slot ^ 1u);
      ends[2] += lo & slot;
      ends[3] += hi & slot;
      if (!(lo | hi)) atomicAdd(&tab[slot * (bins + 1) + row], 1u);
    }
  });
  if (HIST) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned s = (unsigned)wave_sum_i((int)ends[j]);
      if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tab[(j >> 1) * (bins + 1) + ((j & 1) ? bins : 0)], s);
    }
    __syncthreads();
    u64* out = hist + (long)v * 3 * (bins + 1);
    for (int i = threadIdx.x; i < 2 * (bins + 1); i += RT) {
      const unsigned k = tab[i];
      const int slot = i > bins, row = i - slot * (bins + 1);
      if (k) atomicAdd(&out[(side ? slot * 2 : 1) * (bins + 1) + row], (u64)k);
    }
  }
  if (VOL && !COUNT) return;
  matched = wave_sum_i(matched);
  if ((threadIdx.x & 63) == 0) wmat[threadIdx.x >> 6] = matched;
  __syncthreads();
  if (!VOL && rowsT)
    for (long k = (long)n * COLS + threadIdx.x; k < (long)max_lesions * COLS; k += RT) rowsT[k] = 0;
  if (threadIdx.x != 0) return;
  matched = 0;
  for (int w = 0; w < RT / 64; ++w) matched += wmat[w];
  if (VOL) {
    cnt[z2] = n;
    mat[z2] = matched;
  } else {
    summary[(long)v * 4 + side * 2] = n;
    summary[(long)v * 4 + side * 2 + 1] = matched;
  }
}

// One wave per volume of the doubled stack (grid 2 V) over its slices in order: cnt[z'] becomes the
// roots of the volume's earlier slices; summary {n, matched} of the side; the table's rows (of COLS
// columns) past n = 0.
template <int COLS>
__global__ __launch_bounds__(64) void lesion_volume_kernel(const int* __restrict__ starts2, int N, int V,
                                                           int* __restrict__ cnt, const int* __restrict__ mat,
                                                           int max_lesions, int64_t* __restrict__ summary,
                                                           int64_t* __restrict__ table) {
  const int lane = threadIdx.x, v2 = blockIdx.x;
  const int side = v2 >= V, v = v2 - side * V;
  int za = starts2[v2], zb = starts2[v2 + 1];
  za = za < 0 ? 0 : za;
  zb = zb > 2 * N ? 2 * N : zb;
  int carry = 0, matched = 0;
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
      matched += mat[z];
    }
    carry += __shfl(inc, 63, 64);
  }
  matched = wave_sum_i(matched);
  if (table) {
    int64_t* rowsT = table + ((long)v * 2 + side) * max_lesions * COLS;
    for (long k = (long)carry * COLS + lane; k < (long)max_lesions * COLS; k += 64) rowsT[k] = 0;
  }
  if (lane != 0) return;
  summary[(long)v * 4 + side * 2] = carry;
  summary[(long)v * 4 + side * 2 + 1] = matched;
}

// FROC's form pass: lesion_form_kernel's outputs, the zeroed score words sc [2 n] and the row plane
// rowp uint16 [n] = row(p) on P, 0 elsewhere, p from src as curves.hip takes it (probs.h; SOURCE 1 / 2:
// src already points at plane `channel` and K = 1).  One thread per voxel, or per quad of one image's
// voxels (QUAD: HW % 4 == 0, n % 4 == 0 with it, and src / target 16-B, mask 4-B aligned; the scratch is
// 8-B aligned, which the 8-B row store and the 4-B mask stores need).  starts: NULL for images.
template <int SOURCE, int KM, bool QUAD>
__global__ __launch_bounds__(BT) void froc_form_kernel(const uint8_t* __restrict__ mask, const float* __restrict__ src,
                                                       long img_stride, int K, int channel,
                                                       const int64_t* __restrict__ target, long n, long HW, long ignore,
                                                       int bins, const int* __restrict__ starts, int V, int N,
                                                       uint8_t* __restrict__ bin, u64* __restrict__ acc,
                                                       int* __restrict__ sc, uint16_t* __restrict__ rowp,
                                                       int* __restrict__ starts2) {
  if (starts && blockIdx.x == 0)
    for (int v = threadIdx.x; v <= 2 * V; v += BT) {                // as lesion_form_kernel
      const int z = v == V ? N : starts[v < V ? v : v - V];
      starts2[v] = (v > V ? N : 0) + (z < 0 ? 0 : z > N ? N : z);
    }
  const long u = (long)blockIdx.x * BT + threadIdx.x;
  if (QUAD) {
    const long i = u * 4;
    if (i >= n) return;
    const long b = i / HW, off = i - b * HW;
    const uchar4 m = *reinterpret_cast<const uchar4*>(mask + i);
    const longlong2 t0 = *reinterpret_cast<const longlong2*>(target + i);
    const longlong2 t1 = *reinterpret_cast<const longlong2*>(target + i + 2);
    const long tv[4] = {t0.x, t0.y, t1.x, t1.y};
    const uint8_t mv[4] = {m.x, m.y, m.z, m.w};
    bool fgT[4], fgP[4];
    bool any = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool keep = !(ignore >= 0 && tv[j] == ignore);
      fgT[j] = keep && tv[j] > 0;
      fgP[j] = keep && mv[j] != 0;
      any |= fgP[j];
    }
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (any) p = stf::score_quad<SOURCE, KM>(src + b * img_stride, HW, off >> 2, K, channel);
    const float pv[4] = {p.x, p.y, p.z, p.w};
    ushort4 rw;
    rw.x = fgP[0] ? (uint16_t)stf::row_of(pv[0], bins) : (uint16_t)0;
    rw.y = fgP[1] ? (uint16_t)stf::row_of(pv[1], bins) : (uint16_t)0;
    rw.z = fgP[2] ? (uint16_t)stf::row_of(pv[2], bins) : (uint16_t)0;
    rw.w = fgP[3] ? (uint16_t)stf::row_of(pv[3], bins) : (uint16_t)0;
    *reinterpret_cast<ushort4*>(rowp + i) = rw;
    *reinterpret_cast<uchar4*>(bin + i) = make_uchar4(fgT[0], fgT[1], fgT[2], fgT[3]);
    *reinterpret_cast<uchar4*>(bin + n + i) = make_uchar4(fgP[0], fgP[1], fgP[2], fgP[3]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[i + j] = 0;
      acc[n + i + j] = 0;
      sc[i + j] = 0;
      sc[n + i + j] = 0;
    }
  } else {
    const long i = u;
    if (i >= n) return;
    const long b = i / HW, off = i - b * HW;
    const long tv = target[i];
    const bool keep = !(ignore >= 0 && tv == ignore);
    const bool fgP = keep && mask[i] != 0;
    bin[i] = keep && tv > 0;
    bin[n + i] = fgP;
    rowp[i] = fgP ? (uint16_t)stf::row_of(stf::score_at<SOURCE, KM>(src + b * img_stride, HW, off, K, channel), bins)
                  : (uint16_t)0;
    acc[i] = 0;
    acc[n + i] = 0;
    sc[i] = 0;
    sc[n + i] = 0;
  }
}

// scratch: [starts2 int32 [2 V + 1], 256-B rounded][roots per slice int32 [2 N], 256-B rounded]
//          [matched roots per slice int32 [2 N], 256-B rounded]       (images leave these three unused)
//          [(area << 32 | hit) u64 [2 n]][parents int32 [2 n]]
//          FROC only: [score words int32 [2 n]][rows uint16 [n]]
//          [the two masks uint8 [2 n]]
// 26 bytes per voxel of the input; FROC 36.
struct LesionScratch {
  int* starts2;
  int* cnt;
  int* mat;
  u64* acc;
  int* L;
  int* sc;
  uint16_t* rowp;
  uint8_t* bin;
};
inline size_t lesion_scratch_bytes(int N, int H, int W, int V, bool froc) {
  if (!sizes_ok(N, H, W, V)) return 0;
  const size_t head = round_up((2 * (size_t)V + 1) * sizeof(int), 256) + 2 * round_up((size_t)N * 2 * sizeof(int), 256);
  const size_t n = (size_t)N * H * W;
  return round_up(head + n * 2 * (sizeof(u64) + sizeof(int) + 1) + (froc ? n * (2 * sizeof(int) + 2) : 0), 8);
}
inline LesionScratch lesion_carve(void* scratch, int N, int V, long n, bool froc) {
  char* p = (char*)scratch;
  LesionScratch s;
  s.starts2 = (int*)p;
  p += round_up((2 * (size_t)V + 1) * sizeof(int), 256);
  s.cnt = (int*)p;
  p += round_up((size_t)N * 2 * sizeof(int), 256);
  s.mat = (int*)p;
  p += round_up((size_t)N * 2 * sizeof(int), 256);
  s.acc = (u64*)p;
  s.L = (int*)(s.acc + 2 * n);
  s.sc = froc ? s.L + 2 * n : nullptr;
  s.rowp = froc ? (uint16_t*)(s.sc + 2 * n) : nullptr;
  s.bin = froc ? (uint8_t*)(s.rowp + n) : (uint8_t*)(s.L + 2 * n);
  return s;
}

// What the lesion entry points refuse on top of level_or_refuse (which sees the rest).
inline bool lesion_args_ok(const void* target, double min_overlap, int max_lesions, const void* summary,
                           const void* table) {
  if (!target || !summary || max_lesions < 0 || (max_lesions > 0 && !table)) return false;
  if (!(min_overlap >= 0.0 && min_overlap <= 1.0)) return false;    // NaN fails both
  return !(((uintptr_t)target | (uintptr_t)summary | (uintptr_t)table) & 7);
}

// The score side of stf_froc / stf_froc3d, and what they refuse on top of the lesion entry points:
// stf_score_hist's limits.
constexpr int MAXK = 16;
constexpr int MAXBINS = 4096;
struct Froc {
  const float* src;
  int K, source, channel, bins;
  int64_t* hist;
};
inline bool bins_ok(int bins) { return bins >= 2 && bins <= MAXBINS && (bins & (bins - 1)) == 0; }
inline bool froc_args_ok(const Froc& f) {
  if (!f.src || !f.hist || ((uintptr_t)f.src & 3) || ((uintptr_t)f.hist & 7)) return false;
  if (f.K < 1 || f.K > MAXK || f.channel < 0 || f.channel >= f.K || f.source < 0 || f.source > 2) return false;
  return bins_ok(f.bins);
}

template <int SOURCE, int KM>
void launch_froc_form(bool quad, unsigned grid, hipStream_t s, const uint8_t* mask, const float* x, long img_stride,
                      int K, int channel, const int64_t* target, long n, long HW, long ignore, int bins,
                      const int* starts, int V, int N, const LesionScratch& ls) {
  if (quad)
    hipLaunchKernelGGL((froc_form_kernel<SOURCE, KM, true>), dim3(grid), dim3(BT), 0, s, mask, x, img_stride, K,
                       channel, target, n, HW, ignore, bins, starts, V, N, ls.bin, ls.acc, ls.sc, ls.rowp, ls.starts2);
  else
    hipLaunchKernelGGL((froc_form_kernel<SOURCE, KM, false>), dim3(grid), dim3(BT), 0, s, mask, x, img_stride, K,
                       channel, target, n, HW, ignore, bins, starts, V, N, ls.bin, ls.acc, ls.sc, ls.rowp, ls.starts2);
}

// The lesion metrics (FROC false: f is not looked at) and, with FROC, the confidences on top: the row
// plane in form, the candidates' maxima in overlap, the lesions' in pair, the third column and hist in
// the walks.  Launches.  Lesions: images 6; volumes 8, 7 without a table.  FROC: hist's memset and
// images 7; volumes 9, 8 without a table.
template <bool VOL, bool FROC>
int lesion(const uint8_t* mask, const int64_t* target, int N, int H, int W, const int32_t* starts_dev,
           const int32_t* starts_host, int V, int connectivity, double min_overlap, int max_lesions,
           int64_t ignore_index, int64_t* summary, int64_t* table, void* scratch, stf_stream_t stream,
           const Froc& f) {
  const int level = level_or_refuse<VOL>(mask, N, H, W, starts_dev, starts_host, V, connectivity, nullptr, scratch);
  if (!level || !lesion_args_ok(target, min_overlap, max_lesions, summary, table)) return STF_EINVAL;
  if (FROC && !froc_args_ok(f)) return STF_EINVAL;
  if (!max_lesions) table = nullptr;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)N * H * W, rows = (long)N * H, HW = (long)H * W;
  const LesionScratch ls = lesion_carve(scratch, N, V, n, FROC);
  const int bins = FROC ? f.bins : 0;
  const unsigned lds = FROC ? 2u * (unsigned)(bins + 1) * (unsigned)sizeof(unsigned) : 0u;
  u64* hist = FROC ? (u64*)f.hist : nullptr;
  if (FROC) {
    const hipError_t e = stf::memset_async(hist, 0, (size_t)V * 3 * (bins + 1) * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
    const bool quad = HW % 4 == 0 && !((uintptr_t)f.src & 15) && !((uintptr_t)target & 15) && !((uintptr_t)mask & 3);
    const long units = quad ? n / 4 : n;
    const unsigned grid = (unsigned)((units + BT - 1) / BT);
    const long ign = (long)ignore_index, stride = (long)f.K * HW;
    const float* plane = f.src + (long)f.channel * HW;
    if (f.source == 1)
      launch_froc_form<1, 1>(quad, grid, s, mask, plane, stride, 1, 0, target, n, HW, ign, bins, starts_dev, V, N, ls);
    else if (f.source == 2)
      launch_froc_form<2, 1>(quad, grid, s, mask, plane, stride, 1, 0, target, n, HW, ign, bins, starts_dev, V, N, ls);
    else if (f.K <= 2)
      launch_froc_form<0, 2>(quad, grid, s, mask, f.src, stride, f.K, f.channel, target, n, HW, ign, bins, starts_dev,
                             V, N, ls);
    else if (f.K <= 4)
      launch_froc_form<0, 4>(quad, grid, s, mask, f.src, stride, f.K, f.channel, target, n, HW, ign, bins, starts_dev,
                             V, N, ls);
    else if (f.K <= 8)
      launch_froc_form<0, 8>(quad, grid, s, mask, f.src, stride, f.K, f.channel, target, n, HW, ign, bins, starts_dev,
                             V, N, ls);
    else
      launch_froc_form<0, MAXK>(quad, grid, s, mask, f.src, stride, f.K, f.channel, target, n, HW, ign, bins,
                                starts_dev, V, N, ls);
  } else {
    hipLaunchKernelGGL(lesion_form_kernel<VOL>, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, s, mask, target, n,
                       (long)ignore_index, starts_dev, V, N, ls.bin, ls.acc, ls.starts2);
  }
  STF_CHECK_LAUNCH();
  const Scratch sc = {nullptr, nullptr, nullptr, ls.L, nullptr};
  const int rc = label_roots<VOL>(ls.bin, 2 * N, H, W, ls.starts2, 2 * V, level, sc, false, s);
  if (rc) return rc;
  hipLaunchKernelGGL((lesion_overlap_kernel<VOL, FROC>), dim3(row_grid(rows)), dim3(BT), 0, s, (const int*)ls.L, n,
                     rows, H, W, (const int*)ls.starts2, V, ls.acc, (const uint16_t*)ls.rowp, ls.sc);
  STF_CHECK_LAUNCH();
  if (FROC) {
    hipLaunchKernelGGL(froc_pair_kernel<VOL>, dim3(row_grid(rows)), dim3(BT), 0, s, (const int*)ls.L, n, rows, H, W,
                       (const int*)ls.starts2, V, (const u64*)ls.acc, min_overlap, ls.sc);
    STF_CHECK_LAUNCH();
  }
  const dim3 slices((unsigned)N, 2);
  if (!VOL) {
    hipLaunchKernelGGL((lesion_walk_kernel<false, false, FROC>), slices, dim3(RT), lds, s, (const int*)ls.L,
                       (const u64*)ls.acc, N, H * W, (const int*)nullptr, V, ls.cnt, ls.mat, min_overlap, max_lesions,
                       summary, table, (const int*)ls.sc, bins, hist);
    STF_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL((lesion_walk_kernel<true, true, FROC>), slices, dim3(RT), lds, s, (const int*)ls.L,
                     (const u64*)ls.acc, N, H * W, (const int*)ls.starts2, V, ls.cnt, ls.mat, min_overlap, max_lesions,
                     summary, table, (const int*)ls.sc, bins, hist);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(lesion_volume_kernel<FROC ? 3 : 2>, dim3((unsigned)(2 * V)), dim3(64), 0, s,
                     (const int*)ls.starts2, N, V, ls.cnt, (const int*)ls.mat, max_lesions, summary, table);
  STF_CHECK_LAUNCH();
  if (!table) return 0;
  hipLaunchKernelGGL((lesion_walk_kernel<true, false, FROC>), slices, dim3(RT), 0, s, (const int*)ls.L,
                     (const u64*)ls.acc, N, H * W, (const int*)ls.starts2, V, ls.cnt, ls.mat, min_overlap, max_lesions,
                     summary, table, (const int*)ls.sc, bins, hist);
  STF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t stf_lesion_scratch_bytes(int N, int H, int W, int V) {
  return lesion_scratch_bytes(N, H, W, V, false);
}

extern "C" size_t stf_froc_scratch_bytes(int N, int H, int W, int V, int bins) {
  return bins_ok(bins) ? lesion_scratch_bytes(N, H, W, V, true) : 0;
}

extern "C" int stf_froc(const uint8_t* mask, const float* src, int K, int source, int channel, const int64_t* target,
                        int B, int H, int W, int connectivity, double min_overlap, int max_lesions,
                        int64_t ignore_index, int bins, int64_t* summary, int64_t* table, int64_t* hist,
                        void* scratch, stf_stream_t stream) {
  return lesion<false, true>(mask, target, B, H, W, nullptr, nullptr, B, connectivity, min_overlap, max_lesions,
                             ignore_index, summary, table, scratch, stream, Froc{src, K, source, channel, bins, hist});
}

extern "C" int stf_froc3d(const uint8_t* mask, const float* src, int K, int source, int channel,
                          const int64_t* target, int N, int H, int W, const int32_t* starts_dev,
                          const int32_t* starts_host, int V, int connectivity, double min_overlap, int max_lesions,
                          int64_t ignore_index, int bins, int64_t* summary, int64_t* table, int64_t* hist,
                          void* scratch, stf_stream_t stream) {
  return lesion<true, true>(mask, target, N, H, W, starts_dev, starts_host, V, connectivity, min_overlap, max_lesions,
                            ignore_index, summary, table, scratch, stream, Froc{src, K, source, channel, bins, hist});
}

extern "C" int stf_lesion_metrics(const uint8_t* mask, const int64_t* target, int B, int H, int W, int connectivity,
                                  double min_overlap, int max_lesions, int64_t ignore_index, int64_t* summary,
                                  int64_t* table, void* scratch, stf_stream_t stream) {
  return lesion<false, false>(mask, target, B, H, W, nullptr, nullptr, B, connectivity, min_overlap, max_lesions,
                              ignore_index, summary, table, scratch, stream, Froc{});
}

extern "C" int stf_lesion3d_metrics(const uint8_t* mask, const int64_t* target, int N, int H, int W,
                                    const int32_t* starts_dev, const int32_t* starts_host, int V, int connectivity,
                                    double min_overlap, int max_lesions, int64_t ignore_index, int64_t* summary,
                                    int64_t* table, void* scratch, stf_stream_t stream) {
  return lesion<true, false>(mask, target, N, H, W, starts_dev, starts_host, V, connectivity, min_overlap, max_lesions,
                             ignore_index, summary, table, scratch, stream, Froc{});
}

extern "C" size_t stf_ccl_scratch_bytes(int B, int H, int W) { return scratch_bytes<false>(B, H, W, B); }

extern "C" size_t stf_ccl3d_scratch_bytes(int N, int H, int W, int V) { return scratch_bytes<true>(N, H, W, V); }

extern "C" int stf_ccl_label(const uint8_t* mask, int B, int H, int W, int connectivity, int32_t* labels,
                             int32_t* num, void* scratch, stf_stream_t stream) {
  return label<false>(mask, B, H, W, nullptr, nullptr, B, connectivity, labels, num, scratch, stream);
}

extern "C" int stf_ccl_filter(const uint8_t* mask, const int64_t* target, int B, int H, int W, int connectivity,
                              int keep_largest, int64_t min_size, int64_t ignore_index, uint8_t* out,
                              int64_t* counts, int32_t* num, void* scratch, stf_stream_t stream) {
  return filter<false>(mask, target, B, H, W, nullptr, nullptr, B, connectivity, keep_largest, min_size,
                       ignore_index, out, counts, num, scratch, stream);
}

extern "C" int stf_ccl3d_label(const uint8_t* mask, int N, int H, int W, const int32_t* starts_dev,
                               const int32_t* starts_host, int V, int connectivity, int32_t* labels, int32_t* num,
                               void* scratch, stf_stream_t stream) {
  return label<true>(mask, N, H, W, starts_dev, starts_host, V, connectivity, labels, num, scratch, stream);
}

extern "C" int stf_ccl3d_filter(const uint8_t* mask, const int64_t* target, int N, int H, int W,
                                const int32_t* starts_dev, const int32_t* starts_host, int V, int connectivity,
                                int keep_largest, int64_t min_size, int64_t ignore_index, uint8_t* out, int64_t* counts,
                                int32_t* num, void* scratch, stf_stream_t stream) {
  return filter<true>(mask, target, N, H, W, starts_dev, starts_host, V, connectivity, keep_largest, min_size,
                      ignore_index, out, counts, num, scratch, stream);
}
