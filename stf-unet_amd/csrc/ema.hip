// Exponential moving average of the weights, kept in one fp32 shadow buffer: the update
// shadow += w * (model - shadow) and the in-place exchange of model and shadow, each ONE launch over
// a table of segments (parameters and BatchNorm buffers together).  fp32 kernels: the same code in
// both storage builds.
//
// A segment is `len` model elements at `model` and their place `off` in the shadow.  As in clip.hip
// the segments' elements are cut into chunks of EM_CH, numbered through the table in order; chunk k
// belongs to workgroup k % grid.  No work counter, no atomics: every element is touched exactly once
// and the result is a function of the inputs alone.  Nothing outside a segment is read or written on
// either side (the padding between shadow segments included).
//
// Streaming passes: per element the update reads 8 B and writes 4 B, the swap reads 8 B and writes
// 8 B.  The shadow side is always 16-B aligned (off % 4 == 0 on a 16-B aligned buffer) and moves as
// float4, four per lane and side in flight in a whole chunk (clip.hip's shape).  The model side of a
// segment moves as float4 when its pointer is 16-B aligned (every FlatParams slice and every buffer
// torch allocates) and element by element when it is not (a view at an odd element offset); the
// branch is uniform per segment.
#include "common.h"
#include "../../include/stfunet.h"

namespace {

constexpr int EM_NT = 256;                    // threads per workgroup (4 waves)
constexpr int EM_LD = 4;                      // 16-B loads in flight per lane and side
constexpr int EM_CH = EM_NT * EM_LD * 4;      // elements per chunk
constexpr int EM_ROWS = 2048;                 // most workgroups: 8 per CU
constexpr int EM_TAB = EM_NT;                 // table entries staged in LDS per pass (one per thread)

// a value every lane holds alike, moved to scalar registers: the table walk's control flow stays scalar
STF_DEV long uniform(long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32));
  return (long)(((unsigned long)hi << 32) | lo);
}

// what happens to one (shadow, model) pair; WRITES_MODEL: the model side is stored back
struct Update {                               // e + w (p - e): the difference rounds, the fma rounds once
  static constexpr bool WRITES_MODEL = false;
  float w;
  STF_DEV void operator()(float& e, float& p) const { e = __builtin_fmaf(w, p - e, e); }
};
struct Copy {                                 // w == 1: the model's bits (e + (p - e) does not round to p)
  static constexpr bool WRITES_MODEL = false;
  STF_DEV void operator()(float& e, float& p) const { e = p; }
};
struct Swap {                                 // moves only: -0.0 and NaN payloads survive
  static constexpr bool WRITES_MODEL = true;
  STF_DEV void operator()(float& e, float& p) const { const float t = e; e = p; p = t; }
};

template <class Op>
STF_DEV void apply4(const Op& op, float4& e, float4& p) {
  op(e.x, p.x); op(e.y, p.y); op(e.z, p.z); op(e.w, p.w);
}

// model side of one float4 of the shadow: ALIGNED as a float4, else four elements
template <bool ALIGNED>
STF_DEV float4 load_model(const float* m) {
  if (ALIGNED) return *reinterpret_cast<const float4*>(m);
  return make_float4(m[0], m[1], m[2], m[3]);
}
template <bool ALIGNED>
STF_DEV void store_model(float* m, const float4& v) {
  if (ALIGNED) { *reinterpret_cast<float4*>(m) = v; return; }
  m[0] = v.x; m[1] = v.y; m[2] = v.z; m[3] = v.w;
}

// This workgroup's chunks (first, first + grid, ...) of one segment: whole chunks with EM_LD float4
// per lane and side in flight; the segment's last, partial chunk one float4 at a time and the
// len % 4 tail one element per lane (clip.hip's walk_chunks pattern).
template <bool ALIGNED, class Op>
STF_DEV void walk_segment(float* __restrict__ sh, float* __restrict__ mo, long len, long nch, int first, const Op& op) {
  const int grid = gridDim.x, tid = threadIdx.x;
  for (long c = first; c < nch; c += grid) {
    const long e0 = c * EM_CH, rem = len - e0;
    float* s = sh + e0;
    float* m = mo + e0;
    if (rem >= EM_CH) {
      float4 e[EM_LD], p[EM_LD];
#pragma unroll
      for (int k = 0; k < EM_LD; ++k) e[k] = reinterpret_cast<const float4*>(s)[k * EM_NT + tid];
#pragma unroll
      for (int k = 0; k < EM_LD; ++k) p[k] = load_model<ALIGNED>(m + 4 * (k * EM_NT + tid));
#pragma unroll
      for (int k = 0; k < EM_LD; ++k) apply4(op, e[k], p[k]);
#pragma unroll
      for (int k = 0; k < EM_LD; ++k) reinterpret_cast<float4*>(s)[k * EM_NT + tid] = e[k];
      if (Op::WRITES_MODEL) {
#pragma unroll
        for (int k = 0; k < EM_LD; ++k) store_model<ALIGNED>(m + 4 * (k * EM_NT + tid), p[k]);
      }
    } else {
      const long nv = rem >> 2;
      for (long i = tid; i < nv; i += EM_NT) {
        float4 e = reinterpret_cast<const float4*>(s)[i];
        float4 p = load_model<ALIGNED>(m + 4 * i);
        apply4(op, e, p);
        reinterpret_cast<float4*>(s)[i] = e;
        if (Op::WRITES_MODEL) store_model<ALIGNED>(m + 4 * i, p);
      }
      if (tid < (int)(rem & 3)) {
        float e = s[nv * 4 + tid], p = m[nv * 4 + tid];
        op(e, p);
        s[nv * 4 + tid] = e;
        if (Op::WRITES_MODEL) m[nv * 4 + tid] = p;
      }
    }
  }
}

template <class Op>
__global__ __launch_bounds__(EM_NT) void ema_kernel(float* __restrict__ shadow, const stf_ema_seg* __restrict__ segs,
                                                    int count, Op op) {
  // Every workgroup walks the whole table, and most entries (a BatchNorm buffer is one chunk) give
  // it nothing to do: read from global memory one entry at a time, that walk is a chain of dependent
  // loads, ~0.4 us per entry and workgroup (measured: 89 entries cost the STF table 40 us).  So the
  // table is staged through LDS, EM_TAB entries per pass, one coalesced load per pass.
  __shared__ stf_ema_seg tab[EM_TAB];
  const int grid = gridDim.x, tid = threadIdx.x;
  int first = blockIdx.x;                      // this workgroup's first chunk of the segment
  for (int t0 = 0; t0 < count; t0 += EM_TAB) {
    const int nt = count - t0 < EM_TAB ? count - t0 : EM_TAB;
    __syncthreads();                           // the previous pass's entries are no longer read
    if (tid < nt) tab[tid] = segs[t0 + tid];
    __syncthreads();
    for (int s = 0; s < nt; ++s) {
      float* mo = reinterpret_cast<float*>(uniform((long)(uintptr_t)tab[s].model));
      const long off = uniform(tab[s].off), len = uniform(tab[s].len);
      const long nch = (len + EM_CH - 1) / EM_CH;
      if (first < nch) {
        if (((uintptr_t)mo & 15) == 0)
          walk_segment<true>(shadow + off, mo, len, nch, first, op);
        else
          walk_segment<false>(shadow + off, mo, len, nch, first, op);
      }
      // chunk numbers continue in the next segment: its chunk j is number (chunks so far + j)
      first = (int)(((long)first + grid - nch % grid) % grid);
    }
  }
}

// the host copy of the table: returns the workgroups to launch (the table's chunks, at most
// EM_ROWS; 0: every segment is empty), or -1 for an entry the kernels must not see
int checked_grid(const float* shadow, const stf_ema_seg* segs, const stf_ema_seg* segs_host, int count) {
  if (!shadow || !segs || !segs_host || count < 1 || ((uintptr_t)shadow & 15)) return -1;
  long chunks = 0;
  for (int s = 0; s < count; ++s) {
    const stf_ema_seg& g = segs_host[s];
    if (g.len < 0 || g.off < 0 || (g.off & 3)) return -1;
    if (g.len > 0 && (!g.model || ((uintptr_t)g.model & 3))) return -1;
    chunks += (g.len + EM_CH - 1) / EM_CH;
  }
  return (int)(chunks > EM_ROWS ? EM_ROWS : chunks);
}

template <class Op>
int launch(float* shadow, const stf_ema_seg* segs, int count, int grid, Op op, stf_stream_t stream) {
  hipLaunchKernelGGL(ema_kernel<Op>, dim3(grid), dim3(EM_NT), 0, (hipStream_t)stream, shadow, segs, count, op);
  STF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int stf_ema_update(float* shadow, const stf_ema_seg* segs, const stf_ema_seg* segs_host, int count, float w,
                              stf_stream_t stream) {
  if (!(w >= 0.f && w <= 1.f)) return STF_EINVAL;                 // NaN and anything outside [0, 1]
  const int grid = checked_grid(shadow, segs, segs_host, count);
  if (grid < 0) return STF_EINVAL;
  if (grid == 0 || w == 0.f) return 0;         // w == 0 leaves the shadow's bits (0 * inf would not)
  if (w == 1.f) return launch(shadow, segs, count, grid, Copy{}, stream);
  return launch(shadow, segs, count, grid, Update{w}, stream);
}

extern "C" int stf_ema_swap(float* shadow, const stf_ema_seg* segs, const stf_ema_seg* segs_host, int count,
                            stf_stream_t stream) {
  const int grid = checked_grid(shadow, segs, segs_host, count);
  if (grid < 0) return STF_EINVAL;
  if (grid == 0) return 0;
  return launch(shadow, segs, count, grid, Swap{}, stream);
}
