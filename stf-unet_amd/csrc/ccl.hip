// Connected components of binary masks on the device: labels in
// scipy.ndimage.label's numbering, and the post-processing filter of the usual segmentation recipe
// (keep the largest component, drop components below a size) with the per-image counts of the
// filtered mask.  Every image of the uint8 [B][H][W] batch is labelled on its own; foreground is
// mask != 0, connectivity 4 or 8, background outside the image.
//
// The state is one int32 parent per pixel, L[p] (in-image linear index p = y W + x < 2^24; -1 on the
// background), with the invariant L[p] <= p.  A fixed sequence of launches, none of which waits for
// another workgroup, reads anything back or allocates:
//   init      one wave per image row walks the row's 64-pixel chunks.  The foreground of a chunk is a
//             ballot word; every pixel's parent is the first pixel of its horizontal run (clz on the
//             zeros below the lane; a run that reaches the chunk's first pixel inherits the start the
//             wave carries over the seam).  Only run starts are ever roots, so only they are ever the
//             target of an atomic.  Zeroes the area words when the filter needs them.
//   merge     one wave per row y >= 1, the row and the row above as bit words (lane c keeps word c).
//             Bit arithmetic picks one pixel pair per touching pair of runs (below); each pair is
//             united by find + atomicMin.  Integer atomics only, so the partition does not depend on
//             the order of arrival, and the root of a tree is the smallest index of its component:
//             every link points from a larger index to a smaller one of the same component.
//   compress  one wave per row: every foreground pixel follows parents to its root and stores it; the
//             first lane of every run segment of a chunk adds the segment's length to area[root]
//             (filter only; one integer atomic per run and chunk, not per pixel).
//   scan      one workgroup per image walks the image in raster order with a carry: "is a root"
//             (L[p] == p) is scanned exclusively.  For the labels the 1-based rank is stored at the
//             root: ranks follow each component's first pixel in raster order, scipy's numbering.  For
//             the filter the same walk selects the largest area, ties to the smaller root.  The
//             carry's final value is the number of components.
//   labels / filter   one pass over the pixels writes the output (and the filter's counts).
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
//
// Integer only: the same code in both storage builds.
#include "ccl_common.h"
#include "../../include/stfunet.h"

namespace {

constexpr unsigned ROOT_MAX = 0xFFFFFFu;   // in-image indices fit 24 bits

// rows = B * H.  L [B][H][W] = first pixel of the pixel's horizontal run, -1 on the background;
// area (or NULL) [B][H][W] = 0.
__global__ __launch_bounds__(BT) void ccl_init_kernel(const uint8_t* __restrict__ mask, long rows, int H, int W,
                                                      int* __restrict__ L, int* __restrict__ area) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;                                            // whole waves leave: no barrier below
  const int y = (int)(r % H);
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
      L[base + x] = fg ? y * W + start : -1;
      if (area) area[base + x] = 0;
    }
    const int last = __shfl(start, 63, 64);
    carry = (w >> 63) ? last : -1;
  }
}

// One union per touching pair of runs of rows y - 1 and y.  With cur / up the rows' foreground:
//   vertical    cur[x] & up[x], unless cur[x-1] & up[x-1] (the same two runs, united at x - 1 or before)
//   diagonals   (connectivity 8) cur[x] & up[x-1], unless up[x] (the upper run reaches x: vertical at
//               x) or cur[x-1] (vertical at x - 1); cur[x] & up[x+1], unless up[x] or cur[x+1].
__global__ __launch_bounds__(BT) void ccl_merge_kernel(const uint8_t* __restrict__ mask, long rows, int H, int W,
                                                       int conn8, int* L) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const long b = r / H;
  const int y = (int)(r - b * H);
  if (y == 0) return;                                               // wave-uniform
  int* Li = L + b * (long)H * W;
  const u64 cur = row_word(mask + r * (long)W, W, lane), up = row_word(mask + (r - 1) * (long)W, W, lane);
  const u64 curL = (cur << 1) | (shfl_up1(cur, lane) >> 63);        // bit i = pixel x - 1
  const u64 upL = (up << 1) | (shfl_up1(up, lane) >> 63);
  const u64 curR = (cur >> 1) | (shfl_down1(cur, lane) << 63);      // bit i = pixel x + 1
  const u64 upR = (up >> 1) | (shfl_down1(up, lane) << 63);
  const u64 V = cur & up & ~(curL & upL);
  const u64 DL = conn8 ? cur & upL & ~up & ~curL : 0ull;
  const u64 DR = conn8 ? cur & upR & ~up & ~curR : 0ull;
  const int nw = (W + 63) >> 6;
  for (int c = 0; c < nw; ++c) {
    const u64 v = __shfl(V, c, 64), dl = __shfl(DL, c, 64), dr = __shfl(DR, c, 64);
    if (!(v | dl | dr)) continue;                                   // wave-uniform
    const int p = y * W + c * 64 + lane;
    if ((v >> lane) & 1) unite(Li, p, p - W);
    if ((dl >> lane) & 1) unite(Li, p, p - W - 1);                  // x >= 1: bit 0 of word 0 of upL is zero
    if ((dr >> lane) & 1) unite(Li, p, p - W + 1);                  // x + 1 < W: up has no bit at x >= W
  }
}

// L[p] = root of p, in place.  area (or NULL; zero on entry): area[root] += pixels, one add per run
// segment of a chunk.
__global__ __launch_bounds__(BT) void ccl_compress_kernel(long rows, int H, int W, int* L, int* area) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const long b = r / H;
  const int y = (int)(r - b * H);
  int* Li = L + b * (long)H * W;
  const int nw = (W + 63) >> 6;
  for (int c = 0; c < nw; ++c) {
    const int x = c * 64 + lane;
    const int v = x < W ? Li[y * W + x] : -1;
    const bool fg = v >= 0;
    int root = v;
    if (fg) {
      root = find_root<false>(Li, v);
      Li[y * W + x] = root;
    }
    if (area) {
      const u64 w = __ballot(fg);
      if (fg && (lane == 0 || !((w >> (lane - 1)) & 1))) {
        const u64 t = ~(w >> lane);                                 // zero only for lane 0 of a full word
        atomicAdd(&area[b * (long)H * W + root], t ? __builtin_ctzll(t) : 64);
      }
    }
  }
}

// One workgroup per image.  select == 0: aux[root] = 1-based rank of the root in raster order.
// select != 0: aux holds the areas; sel[b] = the root of the largest area, ties to the smaller root
// (-1 without a component).  num (or NULL) [b] = number of roots.
__global__ __launch_bounds__(RT) void ccl_scan_kernel(const int* __restrict__ L, int* __restrict__ aux, int HW,
                                                      int select, int* __restrict__ num, int* __restrict__ sel) {
  __shared__ int wtot[RT / 64];
  __shared__ u64 wbest[RT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int* Li = L + (long)blockIdx.x * HW;
  int* Ai = aux + (long)blockIdx.x * HW;
  int carry = 0;
  u64 best = 0;                                                     // (area << 32) | (ROOT_MAX - root); 0 = none
  for (int base = 0; base < HW; base += RT * NK) {
    const int i0 = base + tid * NK;
    bool root[NK];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      root[k] = i0 + k < HW && Li[i0 + k] == i0 + k;
      cnt += root[k];
    }
    int inc = cnt;
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
    int run = carry + before + inc - cnt;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      if (!root[k]) continue;
      ++run;
      if (select) {
        const u64 key = ((u64)(unsigned)Ai[i0 + k] << 32) | (u64)(ROOT_MAX - (unsigned)(i0 + k));
        best = key > best ? key : best;
      } else {
        Ai[i0 + k] = run;
      }
    }
    carry += total;
    __syncthreads();                                                // wtot is free again
  }
  if (select) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 t = __shfl_xor(best, o, 64);
      best = t > best ? t : best;
    }
    if (lane == 0) wbest[wv] = best;
    __syncthreads();
  }
  if (tid != 0) return;
  if (num) num[blockIdx.x] = carry;
  if (select) {
    for (int w = 1; w < RT / 64; ++w) best = wbest[w] > best ? wbest[w] : best;
    sel[blockIdx.x] = best ? (int)(ROOT_MAX - (unsigned)(best & 0xFFFFFFFFull)) : -1;
  }
}

__global__ __launch_bounds__(BT) void ccl_labels_kernel(const int* __restrict__ L, const int* __restrict__ rank,
                                                        long n, long HW, int* __restrict__ labels) {
  const long i = (long)blockIdx.x * BT + threadIdx.x;
  if (i >= n) return;
  const int v = L[i];
  labels[i] = v < 0 ? 0 : rank[i / HW * HW + v];
}

// out = mask where the pixel's component passes, 0 elsewhere; counts (or NULL; zero on entry)
// [B][3] += (|P' & T|, |P'|, |T|) of the row with stf_predict_mask's rules.
__global__ __launch_bounds__(BT) void ccl_filter_kernel(const uint8_t* __restrict__ mask,
                                                        const int64_t* __restrict__ target, long rows, int H, int W,
                                                        const int* __restrict__ L, const int* __restrict__ area,
                                                        const int* __restrict__ sel, int keep_largest, long min_size,
                                                        long ignore, uint8_t* __restrict__ out,
                                                        u64* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (r >= rows) return;
  const long b = r / H;
  const int* Ai = area + b * (long)H * W;
  const int largest = keep_largest ? sel[b] : -1;
  int ni = 0, np = 0, nt = 0;
  for (int x = lane; x < W; x += 64) {
    const long i = r * (long)W + x;
    const int v = L[i];
    const bool pass = v >= 0 && (long)Ai[v] >= min_size && (!keep_largest || v == largest);
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
  if (!counts) return;                                              // wave-uniform
  ni = wave_sum_i(ni);
  np = wave_sum_i(np);
  nt = wave_sum_i(nt);
  if (lane == 0 && ni) atomicAdd(&counts[b * 3], (u64)ni);
  if (lane == 1 && np) atomicAdd(&counts[b * 3 + 1], (u64)np);
  if (lane == 2 && nt) atomicAdd(&counts[b * 3 + 2], (u64)nt);
}

// B, H, W inside the limits and B * H * W < 2^31
inline bool sizes_ok(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1 || H > MAXDIM || W > MAXDIM) return false;
  return (long)B * H * W < (1L << 31);
}

// scratch: [selected root int32 [B], 256-B rounded][parents int32 [n]][ranks or areas int32 [n]]
struct Scratch {
  int* sel;
  int* L;
  int* aux;
};
inline Scratch carve(void* scratch, int B, long n) {
  char* p = (char*)scratch;
  Scratch s;
  s.sel = (int*)p;
  p += round_up((size_t)B * sizeof(int), 256);
  s.L = (int*)p;
  s.aux = s.L + n;
  return s;
}

// init, merge, compress: afterwards L holds every pixel's root (and aux the areas when with_area)
int label_roots(const uint8_t* mask, int B, int H, int W, int connectivity, const Scratch& sc, bool with_area,
                hipStream_t s) {
  const long rows = (long)B * H;
  int* area = with_area ? sc.aux : nullptr;
  hipLaunchKernelGGL(ccl_init_kernel, dim3(row_grid(rows)), dim3(BT), 0, s, mask, rows, H, W, sc.L, area);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl_merge_kernel, dim3(row_grid(rows)), dim3(BT), 0, s, mask, rows, H, W,
                     connectivity == 8 ? 1 : 0, sc.L);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl_compress_kernel, dim3(row_grid(rows)), dim3(BT), 0, s, rows, H, W, sc.L, area);
  STF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t stf_ccl_scratch_bytes(int B, int H, int W) {
  if (!sizes_ok(B, H, W)) return 0;
  const size_t n = (size_t)B * H * W;
  return round_up(round_up((size_t)B * sizeof(int), 256) + n * 2 * sizeof(int), 8);
}

extern "C" int stf_ccl_label(const uint8_t* mask, int B, int H, int W, int connectivity, int32_t* labels,
                             int32_t* num, void* scratch, stf_stream_t stream) {
  if (!mask || !labels || !num || !scratch || !sizes_ok(B, H, W)) return STF_EINVAL;
  if (connectivity != 4 && connectivity != 8) return STF_EINVAL;
  if (((uintptr_t)scratch & 7) || ((uintptr_t)labels & 3) || ((uintptr_t)num & 3)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)B * H * W;
  const Scratch sc = carve(scratch, B, n);
  const int rc = label_roots(mask, B, H, W, connectivity, sc, false, s);
  if (rc) return rc;
  hipLaunchKernelGGL(ccl_scan_kernel, dim3((unsigned)B), dim3(RT), 0, s, (const int*)sc.L, sc.aux, H * W, 0, num,
                     sc.sel);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl_labels_kernel, dim3((unsigned)((n + BT - 1) / BT)), dim3(BT), 0, s, (const int*)sc.L,
                     (const int*)sc.aux, n, (long)H * W, labels);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_ccl_filter(const uint8_t* mask, const int64_t* target, int B, int H, int W, int connectivity,
                              int keep_largest, int64_t min_size, int64_t ignore_index, uint8_t* out,
                              int64_t* counts, int32_t* num, void* scratch, stf_stream_t stream) {
  if (!mask || !out || !scratch || !sizes_ok(B, H, W)) return STF_EINVAL;
  if ((connectivity != 4 && connectivity != 8) || min_size < 0 || (counts && !target) || out == mask)
    return STF_EINVAL;
  if (((uintptr_t)scratch & 7) || ((uintptr_t)counts & 7) || ((uintptr_t)target & 7) || ((uintptr_t)num & 3))
    return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const long n = (long)B * H * W, rows = (long)B * H;
  const Scratch sc = carve(scratch, B, n);
  if (counts) {
    hipError_t e = stf::memset_async(counts, 0, (size_t)B * 3 * sizeof(int64_t), s);
    if (e != hipSuccess) return (int)e;
  }
  const int rc = label_roots(mask, B, H, W, connectivity, sc, true, s);
  if (rc) return rc;
  hipLaunchKernelGGL(ccl_scan_kernel, dim3((unsigned)B), dim3(RT), 0, s, (const int*)sc.L, sc.aux, H * W, 1, num,
                     sc.sel);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ccl_filter_kernel, dim3(row_grid(rows)), dim3(BT), 0, s, mask, counts ? target : nullptr, rows,
                     H, W, (const int*)sc.L, (const int*)sc.aux, (const int*)sc.sel, keep_largest ? 1 : 0,
                     (long)min_size, (long)ignore_index, out, (u64*)counts);
  STF_CHECK_LAUNCH();
  return 0;
}
