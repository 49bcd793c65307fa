// Global L2 norm of a set of segments of one fp32 buffer (the flat gradient), the clip
// coefficient, and the in-place scale by it.  fp32 kernels: the same code in both storage builds.
//
// The segments' elements are cut into chunks of GN_CH, numbered through the table in order; chunk k
// belongs to workgroup k % grid.  The assignment is a function of the table and the grid alone (no
// work counter, no atomics), every workgroup writes one partial row, and one workgroup folds the
// rows in index order: the result is the same bits from run to run.
//
// Squares and sums are in double.  The pass is bound by reading the buffer (16 B per lane and load,
// four loads in flight); one v_cvt_f64_f32 and one v_fma_f64 per element are far off that path.
// In exchange the sum cannot overflow or flush for any fp32 input (gradients that still carry a
// 65536 loss scale, or 1e-30), and its relative error is below n * 2^-53, so the fp32 result is
// within 1 ulp of the fp32 rounding of the exact norm.
#include "common.h"
#include "../../include/stfunet.h"

namespace {

constexpr int GN_NT = 256;                    // threads per workgroup (4 waves)
constexpr int GN_LD = 4;                      // 16-B loads in flight per lane
constexpr int GN_CH = GN_NT * GN_LD * 4;      // elements per chunk
constexpr int GN_ROWS = 2048;                 // most workgroups (= partial rows): 8 per CU

long rows_for(long n) {
  const long r = (n + GN_CH - 1) / GN_CH;
  return r < 1 ? 1 : (r > GN_ROWS ? GN_ROWS : r);
}

// Calls full(q) for every whole chunk of this workgroup (q = this lane's first float4 of the chunk;
// its others are q[GN_NT], q[2 GN_NT], ...), and for the last, partial chunk of a segment vec(q) per
// whole float4 inside the segment and one(p) per element of the scalar tail (len % 4 elements).
template <class T, class Full, class Vec, class One>
STF_DEV void walk_chunks(T* buf, const stf_seg* __restrict__ segs, int count, Full&& full, Vec&& vec, One&& one) {
  using V = std::conditional_t<std::is_const_v<T>, const float4, float4>;
  const int grid = gridDim.x, tid = threadIdx.x;
  int first = blockIdx.x;                      // this workgroup's first chunk of the segment
  for (int s = 0; s < count; ++s) {
    const long off = segs[s].off, len = segs[s].len;
    const long nch = (len + GN_CH - 1) / GN_CH;
    for (long c = first; c < nch; c += grid) {
      const long e0 = c * GN_CH, rem = len - e0;
      T* base = buf + off + e0;
      if (rem >= GN_CH) {
        full(reinterpret_cast<V*>(base) + tid);
      } else {
        const long nv = rem >> 2;
        for (long i = tid; i < nv; i += GN_NT) vec(reinterpret_cast<V*>(base) + i);
        if (tid < (int)(rem & 3)) one(base + nv * 4 + tid);
      }
    }
    // chunk numbers continue in the next segment: its chunk j is number (chunks so far + j)
    first = (int)(((long)first + grid - nch % grid) % grid);
  }
}

STF_DEV double sq(float x) { return (double)x * (double)x; }

__global__ __launch_bounds__(GN_NT) void grad_norm_partial_kernel(const float* __restrict__ buf,
                                                                  const stf_seg* __restrict__ segs, int count,
                                                                  double* __restrict__ partial) {
  __shared__ double red[GN_NT / 64];
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  auto add4 = [&](const float4& v) { a0 += sq(v.x); a1 += sq(v.y); a2 += sq(v.z); a3 += sq(v.w); };
  walk_chunks(
      buf, segs, count,
      [&](const float4* q) {
        float4 v[GN_LD];
#pragma unroll
        for (int k = 0; k < GN_LD; ++k) v[k] = q[k * GN_NT];
#pragma unroll
        for (int k = 0; k < GN_LD; ++k) add4(v[k]);
      },
      [&](const float4* q) { add4(*q); }, [&](const float* p) { a0 += sq(*p); });
  const double w = wave_sum_d((a0 + a1) + (a2 + a3));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < GN_NT / 64; ++i) t += red[i];
    partial[blockIdx.x] = t;
  }
}

// out = {norm / scale, min(1, max_norm / (norm / scale + 1e-6)), norm not finite, 0}
__global__ __launch_bounds__(GN_NT) void grad_norm_fold_kernel(const double* __restrict__ partial, int rows,
                                                               const float* __restrict__ gscale, float max_norm,
                                                               float* __restrict__ out) {
  __shared__ double red[GN_NT / 64];
  double a = 0.0;
  for (int r = threadIdx.x; r < rows; r += GN_NT) a += partial[r];
  const double w = wave_sum_d(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t = 0.0;
  for (int i = 0; i < GN_NT / 64; ++i) t += red[i];
  double norm = sqrt(t);
  if (gscale) norm *= (double)(1.f / gscale[0]);        // GradScaler's fp32 reciprocal, exact for its scales
  const float total = (float)norm;
  const float c = max_norm / (total + 1e-6f);           // torch.nn.utils.clip_grad_norm_, in fp32
  out[0] = total;
  out[1] = c > 1.f ? 1.f : c;                           // clamp(max=1): a NaN stays a NaN
  out[2] = __builtin_isfinite(total) ? 0.f : 1.f;
  out[3] = 0.f;
}

__global__ __launch_bounds__(GN_NT) void grad_scale_kernel(float* __restrict__ buf, const stf_seg* __restrict__ segs,
                                                           int count, const float* __restrict__ clip) {
  const float coef = clip[1];
  if (coef == 1.f) return;                     // below max_norm: x * 1 is x, nothing to write
  auto mul4 = [&](float4 v) { return make_float4(v.x * coef, v.y * coef, v.z * coef, v.w * coef); };
  walk_chunks(
      buf, segs, count,
      [&](float4* q) {
        float4 v[GN_LD];
#pragma unroll
        for (int k = 0; k < GN_LD; ++k) v[k] = q[k * GN_NT];
#pragma unroll
        for (int k = 0; k < GN_LD; ++k) q[k * GN_NT] = mul4(v[k]);
      },
      [&](float4* q) { *q = mul4(*q); }, [&](float* p) { *p = *p * coef; });
}

// the host copy of the table: every offset a multiple of 4, no negative length; returns the
// number of elements, or -1
long checked_total(const stf_seg* segs_host, int count) {
  long n = 0;
  for (int s = 0; s < count; ++s) {
    if (segs_host[s].len < 0 || segs_host[s].off < 0 || (segs_host[s].off & 3)) return -1;
    n += segs_host[s].len;
  }
  return n;
}

}  // namespace

extern "C" int stf_grad_norm_rows(int64_t n) { return (int)rows_for(n < 0 ? 0 : (long)n); }

extern "C" int stf_grad_norm(const float* buf, const stf_seg* segs, const stf_seg* segs_host, int count,
                             const float* grad_scale, float max_norm, double* partial, float* out,
                             stf_stream_t stream) {
  if (!buf || !segs || !segs_host || !partial || !out || count < 1 || ((uintptr_t)buf & 15)) return STF_EINVAL;
  if (!(max_norm > 0.f)) return STF_EINVAL;                       // NaN, 0 and negatives
  const long n = checked_total(segs_host, count);
  if (n < 0) return STF_EINVAL;
  const int rows = (int)rows_for(n);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(rows), dim3(GN_NT), 0, s, buf, segs, count, partial);
  STF_CHECK_LAUNCH();
  hipLaunchKernelGGL(grad_norm_fold_kernel, dim3(1), dim3(GN_NT), 0, s, (const double*)partial, rows, grad_scale,
                     max_norm, out);
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_grad_scale(float* buf, const stf_seg* segs, const stf_seg* segs_host, int count,
                              const float* clip, stf_stream_t stream) {
  if (!buf || !segs || !segs_host || !clip || count < 1 || ((uintptr_t)buf & 15)) return STF_EINVAL;
  const long n = checked_total(segs_host, count);
  if (n < 0) return STF_EINVAL;
  hipLaunchKernelGGL(grad_scale_kernel, dim3(rows_for(n)), dim3(GN_NT), 0, (hipStream_t)stream, buf, segs, count,
                     clip);
  STF_CHECK_LAUNCH();
  return 0;
}
