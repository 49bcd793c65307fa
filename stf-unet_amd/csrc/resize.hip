// Full-resolution logits: bilinear resize of the fp32 NCHW logits planes (the layout of
// stf_head_fwd and the loss kernels) from h x w up to H x W, and its backward.
//
// The semantics are F.interpolate(mode="bilinear", align_corners=False, size=(H, W)) with
// PyTorch's arithmetic in fp32, per axis: scale = in / out, src = scale (dst + 0.5) - 0.5
// clamped at 0, i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1, and
//   value = l0h (l0w a + l1w b) + l1h (l0w c + l1w d).
// rs_coord is the one place that arithmetic lives: the forward reads through it and the backward
// asks it which outputs read a source pixel, so the backward is the forward's transpose by
// construction.  Only H >= h and W >= w (the model's half-resolution logits up to the frame);
// equal sizes copy bit for bit (every l1 is 0).
//
// Streaming work (cfg3: 2 MB in, 8 MB out), one element per thread, consecutive threads along W.
#include "common.h"
#include "../../include/stfunet.h"

namespace {

constexpr int NT = 256;
constexpr unsigned MAX_GRID = 2048;        // 256 CUs x 8 blocks; the rest grid-strides

unsigned grid_for(long units) {
  const long b = (units + NT - 1) / NT;
  return (unsigned)(b < 1 ? 1 : (b > MAX_GRID ? MAX_GRID : b));
}

// source indices and weights of output index ``dst`` along one axis (in -> out, scale = in / out).
// Every contraction is spelled out, so the forward, the backward and both libraries see the same
// weights whatever the compiler would fuse.  src is ONE fma, as PyTorch's kernels compute
// scale * (dst + 0.5) - 0.5 (its device kernels and its AVX2 / AVX-512 CPU kernels are built with
// contraction on): a separately rounded product moves l1 by an ulp of src (2^-18 at src = 33),
// which is 30x the rounding of the blend itself.
STF_DEV void rs_coord(int dst, float scale, int in, int& i0, int& i1, float& l0, float& l1) {
#pragma clang fp contract(off)
  float src = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
  src = src < 0.f ? 0.f : src;
  i0 = min((int)src, in - 1);
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

// y[p][oy][ox] over planes * H * W outputs (< 2^31: the unsigned index cannot wrap in the stride)
__global__ __launch_bounds__(NT) void resize_bilinear_fwd_kernel(const float* __restrict__ x, int planes, int h,
                                                                 int w, float* __restrict__ y, int H, int W) {
#pragma clang fp contract(off)
  const unsigned total = (unsigned)planes * (unsigned)H * (unsigned)W;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  for (unsigned u = blockIdx.x * NT + threadIdx.x; u < total; u += gridDim.x * NT) {
    const unsigned r = u / (unsigned)W;
    const int ox = (int)(u - r * (unsigned)W);
    const int p = (int)(r / (unsigned)H);
    const int oy = (int)(r - (unsigned)p * (unsigned)H);
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    rs_coord(oy, sh, h, y0, y1, ly0, ly1);
    rs_coord(ox, sw, w, x0, x1, lx0, lx1);
    const float* b = x + p * (h * w);
    const float a00 = b[y0 * w + x0], a01 = b[y0 * w + x1], a10 = b[y1 * w + x0], a11 = b[y1 * w + x1];
    y[u] = ly0 * (lx0 * a00 + lx1 * a01) + ly1 * (lx0 * a10 + lx1 * a11);
  }
}

// The outputs that can read source index i: src in [i - 1, i + 1), i.e. dst in
// [(i - 0.5) / scale - 0.5, (i + 1.5) / scale - 0.5), widened by one on each side against the
// rounding of the inverse and clamped to the axis.  src is monotonic in dst, so nothing outside
// reads i; inside, rs_coord decides.
STF_DEV void rs_range(int i, float scale, int out, int& lo, int& hi) {
  // (clamped as floats first: the conversions and the +-1 stay inside int for every accepted size)
  lo = (int)fmaxf(floorf(((float)i - 0.5f) / scale - 0.5f) - 1.f, 0.f);
  hi = min(out - 1, (int)fminf(ceilf(((float)i + 1.5f) / scale - 0.5f) + 1.f, (float)(out - 1)));
}

// weight with which output ``dst`` reads source index i (0: it does not); both halves when
// i0 == i1 == i (the last row / column)
STF_DEV float rs_weight(int dst, float scale, int in, int i) {
  int i0, i1;
  float l0, l1;
  rs_coord(dst, scale, in, i0, i1, l0, l1);
  return (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
}

// dx[p][iy][ix] = sum over the outputs that read it, ascending (row, column), fp32: a gather,
// no atomics, dx fully overwritten
__global__ __launch_bounds__(NT) void resize_bilinear_bwd_kernel(const float* __restrict__ dy, int planes, int H,
                                                                 int W, float* __restrict__ dx, int h, int w) {
#pragma clang fp contract(off)
  const unsigned total = (unsigned)planes * (unsigned)h * (unsigned)w;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  for (unsigned u = blockIdx.x * NT + threadIdx.x; u < total; u += gridDim.x * NT) {
    const unsigned r = u / (unsigned)w;
    const int ix = (int)(u - r * (unsigned)w);
    const int p = (int)(r / (unsigned)h);
    const int iy = (int)(r - (unsigned)p * (unsigned)h);
    int oy0, oy1, ox0, ox1;
    rs_range(iy, sh, H, oy0, oy1);
    rs_range(ix, sw, W, ox0, ox1);
    const float* g = dy + p * (H * W);
    float acc = 0.f;
    for (int oy = oy0; oy <= oy1; ++oy) {
      const float wy = rs_weight(oy, sh, h, iy);
      if (wy == 0.f) continue;
      for (int ox = ox0; ox <= ox1; ++ox) {
        const float wx = rs_weight(ox, sw, w, ix);
        if (wx == 0.f) continue;
        acc += (wy * wx) * g[oy * W + ox];
      }
    }
    dx[u] = acc;
  }
}

bool resize_args_ok(const void* a, const void* b, int planes, int h, int w, int H, int W) {
  if (!a || !b || planes < 1 || h < 1 || w < 1 || H < h || W < w) return false;
  return (long)planes * H * W < (1L << 31);          // 32-bit index math (and so planes * h * w too)
}

}  // namespace

extern "C" int stf_resize_bilinear_fwd(const float* x, int planes, int h, int w, float* y, int H, int W,
                                       stf_stream_t stream) {
  if (!resize_args_ok(x, y, planes, h, w, H, W)) return STF_EINVAL;
  hipLaunchKernelGGL(resize_bilinear_fwd_kernel, dim3(grid_for((long)planes * H * W)), dim3(NT), 0,
                     (hipStream_t)stream, x, planes, h, w, y, H, W);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_resize_bilinear_bwd(const float* dy, int planes, int H, int W, float* dx, int h, int w,
                                       stf_stream_t stream) {
  if (!resize_args_ok(dy, dx, planes, h, w, H, W)) return STF_EINVAL;
  hipLaunchKernelGGL(resize_bilinear_bwd_kernel, dim3(grid_for((long)planes * h * w)), dim3(NT), 0,
                     (hipStream_t)stream, dy, planes, H, W, dx, h, w);
  STF_CHECK_LAUNCH();
  return 0;
}
