// Training-mode BatchNorm2d (+ReLU, +residual add, +2x2 max pool) for NHWC bf16
// activations, with optional statistic *groups* along the image axis.
//
// Groups: the STF encoder runs all T time steps as one batch of T*B images
// (t-major), but the reference normalises every time step with its own batch
// statistics and advances the running statistics once per step
// (src/stf_lstm_unet.py:168-186).  Group g = images [g*N/G, (g+1)*N/G) keeps its
// own mean/invstd/scale/shift; running stats are updated group by group in t
// order, exactly like T sequential BatchNorm calls.  UNet uses G = 1.
//
// Forward: the producing conv's epilogue wrote per-tile (sum, sum^2) for tiles
// aligned to groups ([G][tpg][2][C]); stf_bn_finalize folds them (fp64) and
// stf_bn_act applies  out = act(y*scale+shift [+ residual])  where the residual
// is another bf16 tensor (identity shortcut) or a second BN of a raw conv output
// (downsample shortcut: ResNet BasicBlock, ResidualConvBlock), optionally also
// writing the 2x2 max-pooled tensor (UNet Down, src/unet.py:25).
//
// Backward (per group and channel, xhat = (y-mean)*invstd):
//   g = dz [+ maxpool routing of dpool] masked by the ReLU (recomputed from y,
//       or read from the saved output when the ReLU followed a residual add),
//   dgamma = sum g*xhat, dbeta = sum g,  dy = A*g + B*y + C  (fp64 coefficients).
//
// Layout of the file: the finalize tails, the per-unit arithmetic, the streaming kernels (flat,
// pooled, group-major, and the stem's three through its MaxPool(3,2,1)), then the host side: one
// BnRoute per launch signature from bn_route -- kernel, block, grid, partial rows, refusal, under the
// numbered rules above it -- which every streaming entry point and both row queries read.
#include <algorithm>

#include "common.h"
#include "../../include/stfunet.h"
#include "reduce.h"

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------ finalize
// stats: [G][T][2][C] with the first S rows of every group folded.  Grid =
// (channel chunks of 16) x G; block = 16 channels x 16 row-lanes folding ONE
// group.  With G > 1 the running statistics must see the G updates in order:
// each block parks (mean, biased var) in row 0 of its group (scratch) and
// bn_running_batch_kernel applies them sequentially.
// (mean, invstd, scale, shift) of channel c of group g from its mean and biased variance
STF_DEV void bn_fin_store(int g, int c, int C, double mu, double var, const float* gamma, const float* beta,
                          float eps, float* mean, float* invstd, float* scale, float* shift) {
  const float inv = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gamma[c] * inv;
  mean[g * C + c] = (float)mu;
  invstd[g * C + c] = inv;
  scale[g * C + c] = sc;
  shift[g * C + c] = beta[c] - (float)mu * sc;
}

// the training-mode finalize of channel c of group g from its folded (sum, sum of squares)
STF_DEV void bn_fin_fwd_out(float* base, int g, int c, int G, int C, long Mg, double s1, double s2,
                            const float* gamma, const float* beta, float mom, float eps, float* rm, float* rv,
                            float* mean, float* invstd, float* scale, float* shift) {
  const double mu = s1 / Mg;
  double var = s2 / Mg - mu * mu;
  if (var < 0) var = 0;
  bn_fin_store(g, c, C, mu, var, gamma, beta, eps, mean, invstd, scale, shift);
  if (G == 1) {
    if (!rm) return;
    const double unb = Mg > 1 ? var * Mg / (Mg - 1) : var;
    rm[c] = (1.f - mom) * rm[c] + mom * (float)mu;
    rv[c] = (1.f - mom) * rv[c] + mom * (float)unb;
  } else {                               // parked for bn_running_batch_kernel
    base[c] = (float)mu;
    base[C + c] = (float)var;
  }
}

__global__ __launch_bounds__(stf::FOLD_NT) void bn_finalize_kernel(float* __restrict__ stats, int S, int T, int G, int C,
                                                        long Mg, const float* gamma, const float* beta, float mom,
                                                        float eps, float* rm, float* rv, float* mean, float* invstd,
                                                        float* scale, float* shift) {
  __shared__ double red[stf::FOLD_NT];
  const int g = blockIdx.y;
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);
  const bool cok = c < C, lead = cok && (threadIdx.x >> 4) == 0;
  if (stats) {
    float* base = stats + (size_t)g * T * 2 * C;
    double s1, s2;
    stf::fold16_pair(base, S, 2L * C, C, c, cok, red, s1, s2);
    if (lead)
      bn_fin_fwd_out(base, g, c, G, C, Mg, s1, s2, gamma, beta, mom, eps, rm, rv, mean, invstd, scale, shift);
    return;
  }
  if (!lead) return;                     // eval mode: running statistics, no update
  bn_fin_store(g, c, C, rm ? rm[c] : 0.f, rv ? rv[c] : 1.f, gamma, beta, eps, mean, invstd, scale, shift);
}

// dy = A g + B y + C coefficients of channel c of group g from its folded (sum g, sum g*xhat)
STF_DEV void bn_fin_bwd_out(float* base, int g, int c, int G, int C, long Mg, double s1, double s2,
                            const float* gamma, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                            float* coef) {
  const double is = invstd[g * C + c];
  const double A = (double)gamma[c] * is;
  const double B = -A * is * s2 / Mg;
  const double Cc = -A * s1 / Mg + A * is * mean[g * C + c] * s2 / Mg;
  coef[(size_t)g * 3 * C + c] = (float)A;
  coef[(size_t)g * 3 * C + C + c] = (float)B;
  coef[(size_t)g * 3 * C + 2 * C + c] = (float)Cc;
  if (G == 1) {
    if (dgamma) dgamma[c] = (float)s2;
    if (dbeta) dbeta[c] = (float)s1;
  } else {
    base[c] = (float)s1;
    base[C + c] = (float)s2;
  }
}

// ------------------------------------------------------------------ per-unit arithmetic
// A unit is 8 consecutive channels (chunk cg) of one pixel: one 16-B load per tensor.  Every
// streaming kernel below finds its units its own way and calls these for what it does with one.

// chunk cg of group g of two [G][C] vectors: (scale, shift), (mean, invstd), the residual's affine
STF_DEV void load_pair(const float* a, const float* b, int g, int C, int cg, float (&va)[8], float (&vb)[8]) {
  load8f(a + (size_t)g * C, cg * 8, va);
  load8f(b + (size_t)g * C, cg * 8, vb);
}
// chunk cg of group g of coef [G][3][C]
STF_DEV void load_coef(const float* coef, int g, int C, int cg, float (&A)[8], float (&B)[8], float (&Cc)[8]) {
  load8f(coef + (size_t)g * 3 * C, cg * 8, A);
  load8f(coef + (size_t)g * 3 * C + C, cg * 8, B);
  load8f(coef + (size_t)g * 3 * C + 2 * C, cg * 8, Cc);
}

// forward: v = act(v*sc + sh [+ r | + r*rs + rh]), r = the unit at *rq; res_mode 0: none, 1: + r,
// 2: + r's own affine
STF_DEV void bn_affine8(float (&v)[8], const float (&sc)[8], const float (&sh)[8], int relu, int res_mode,
                        const uint4* rq, const float (&rs)[8], const float (&rh)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = v[j] * sc[j] + sh[j];
  if (res_mode) {
    float r[8];
    unpack8(*rq, r);
    if (res_mode == 2) {
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = r[j] * rs[j] + rh[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += r[j];
  }
  if (relu) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
  }
}

// backward reduce: d becomes the masked gradient g' (mask 0: d, 1: d where y*sc + sh > 0, 2: d where
// mk > 0; else 0), sg += g', sgx += g' * xhat
STF_DEV void bn_acc8(int mask, float (&d)[8], const float (&y)[8], const float (&sc)[8], const float (&sh)[8],
                     const float* mk, const float (&mu)[8], const float (&is)[8], float (&sg)[8], float (&sgx)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bool keep = true;
    if (mask == 1) keep = y[j] * sc[j] + sh[j] > 0.f;
    else if (mask == 2) keep = mk[j] > 0.f;
    const float gj = keep ? d[j] : 0.f;
    d[j] = gj;
    sg[j] += gj;
    sgx[j] += gj * (y[j] - mu[j]) * is[j];
  }
}

// backward apply: gv = dy = A*g' + B*y + C with g' = gv, or with mask the ReLU mask recomputed from y
// (g' = gv where y*ms + mh > 0, else 0); sb += dy (the bias gradient of the producing conv)
STF_DEV void bn_dy8(bool mask, float (&gv)[8], const float (&y)[8], const float (&ms)[8], const float (&mh)[8],
                    const float (&A)[8], const float (&B)[8], const float (&Cc)[8], float (&sb)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float gj = (mask && !(y[j] * ms[j] + mh[j] > 0.f)) ? 0.f : gv[j];
    gv[j] = A[j] * gj + B[j] * y[j] + Cc[j];
    sb[j] += gv[j];
  }
}

// Block fold of the threads' chunk sums into the block's row of out [rows][H][C], H = (RW - 1) / 8 sums
// per channel (s0 | s1, or s0 alone): every thread parks its 8 H floats in red; channel c's total is
// the sum over the threads that hold chunk c / 8 -- Q consecutive threads, repeating every `stride`
// threads -- in ascending thread order.  Row = gy * gridDim.x + blockIdx.x: gy = the group (blockIdx.y)
// in the group-major grids, 0 in the flat ones.
template <int Q = 1, int NTH, int RW>
STF_DEV void bn_block_fold(float (&red)[NTH][RW], const float (&s0)[8], const float (&s1)[8], int C, int stride,
                           int gy, float* __restrict__ out) {
  constexpr int H = (RW - 1) / 8;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[threadIdx.x][j] = s0[j];
    if (H == 2) red[threadIdx.x][8 + j] = s1[j];
  }
  __syncthreads();
  const size_t row = (size_t)gy * gridDim.x + blockIdx.x;
  for (int c = threadIdx.x; c < C; c += NTH) {
    const int gg = c >> 3, j = c & 7;
    float a = 0.f, b = 0.f;
    for (int t = Q * gg; t < NTH; t += stride)
      for (int q = 0; q < Q; ++q) {
        a += red[t + q][j];
        if (H == 2) b += red[t + q][8 + j];
      }
    out[row * H * C + c] = a;
    if (H == 2) out[row * H * C + C + c] = b;
  }
}

// ------------------------------------------------------------------ apply
// res_mode 0: none, 1: + res tensor, 2: + (res*rscale[g] + rshift[g])
template <bool POOL>
__global__ void bn_act_kernel(const uint16_t* __restrict__ y, int ycs, long N, int H, int W, int C, long Mg,
                              const float* scale, const float* shift, int relu, int res_mode,
                              const uint16_t* __restrict__ res, int rcs, const float* __restrict__ rscale,
                              const float* __restrict__ rshift, uint16_t* __restrict__ out, int ocs,
                              uint16_t* __restrict__ pooled) {
  const int CG = C / 8;
  const long units = POOL ? N * (H / 2) * (W / 2) * CG : N * H * W * CG;
  for (long u = blockIdx.x * (long)NT + threadIdx.x; u < units; u += (long)gridDim.x * NT) {
    const int cg = (int)(u % CG);
    const long pix = u / CG;
    if (!POOL) {
      const int g = (int)(pix / Mg);
      // (inline, not bn_affine8: this kernel loads the residual and its affine only when asked)
      float sc[8], sh[8], v[8];
      load_pair(scale, shift, g, C, cg, sc, sh);
      unpack8(*reinterpret_cast<const uint4*>(y + pix * ycs + cg * 8), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] * sc[j] + sh[j];
      if (res_mode) {
        float r[8];
        unpack8(*reinterpret_cast<const uint4*>(res + pix * rcs + cg * 8), r);
        if (res_mode == 2) {
          float rs[8], rh[8];
          load_pair(rscale, rshift, g, C, cg, rs, rh);
#pragma unroll
          for (int j = 0; j < 8; ++j) r[j] = r[j] * rs[j] + rh[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += r[j];
      }
      if (relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = fmaxf(v[j], 0.f);
      }
      *reinterpret_cast<uint4*>(out + pix * ocs + cg * 8) = pack8(v);
    } else {
      const int Wp = W / 2, Hp = H / 2;
      const long n = pix / ((long)Hp * Wp);
      const int rem = (int)(pix - n * Hp * Wp);
      const int py = rem / Wp, px = rem - py * Wp;
      const int g = (int)(n * H * W / Mg);
      float sc[8], sh[8], mx[8];
      load_pair(scale, shift, g, C, cg, sc, sh);
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const long p = (n * H + 2 * py + (d >> 1)) * W + 2 * px + (d & 1);
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(y + p * ycs + cg * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v[j] = v[j] * sc[j] + sh[j];
          if (relu) v[j] = fmaxf(v[j], 0.f);
          v[j] = round_e(v[j]);
          mx[j] = d == 0 ? v[j] : fmaxf(mx[j], v[j]);
        }
        *reinterpret_cast<uint4*>(out + p * ocs + cg * 8) = pack8(v);
      }
      *reinterpret_cast<uint4*>(pooled + pix * C + cg * 8) = pack8(mx);
    }
  }
}

// ------------------------------------------------------------------ backward reduce
// The pooled reduce with one thread per 2x2 WINDOW and channel chunk, for the chunk counts the DPP
// kernel below does not take (64 % (C / 8) != 0: C = 1024, 2048).  mask_mode 0: none,
// 1: relu(y*scale+shift) > 0 (2 has no pooled form: the mask-source parameters are unused).
__global__ void bn_bwd_reduce_win_kernel(const uint16_t* __restrict__ dz, int dzcs,
                                         const uint16_t* __restrict__ dpool, const uint16_t* __restrict__ y, int ycs,
                                         long N, int H, int W, int C, int G, int tpg,
                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                         const float* __restrict__ mean, const float* __restrict__ invstd,
                                         int mask_mode, const uint16_t* __restrict__ msrc, int mcs,
                                         uint16_t* __restrict__ g_out, float* __restrict__ partial) {
  __shared__ float red[NT][17];
  const int CG = C / 8;
  const int g = blockIdx.x / tpg, tile = blockIdx.x - g * tpg;
  const long wpg = (N / G) * (H / 2) * (W / 2);                           // windows per group
  const long upg = wpg * CG;
  const long gt = (long)tile * NT + threadIdx.x;
  const int cg = (int)(gt % CG);                 // constant: tpg*NT is a multiple of CG
  float sc[8], sh[8], mu[8], is[8];
  load_pair(scale, shift, g, C, cg, sc, sh);
  load_pair(mean, invstd, g, C, cg, mu, is);
  float sg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sgx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (long u = gt; u < upg; u += (long)tpg * NT) {
    const long pix = u / CG + g * wpg;
    const int Wp = W / 2, Hp = H / 2;
    const long n = pix / ((long)Hp * Wp);
    const int rem = (int)(pix - n * Hp * Wp);
    const int py = rem / Wp, px = rem - py * Wp;
    float v[4][8], a[4][8];
    long p[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      p[d] = (n * H + 2 * py + (d >> 1)) * W + 2 * px + (d & 1);
      unpack8(*reinterpret_cast<const uint4*>(y + p[d] * ycs + cg * 8), v[d]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = v[d][j] * sc[j] + sh[j];
        if (mask_mode == 1) t = fmaxf(t, 0.f);
        a[d][j] = round_e(t);
      }
    }
    float dp[8];
    unpack8(*reinterpret_cast<const uint4*>(dpool + pix * C + cg * 8), dp);
    int am[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      am[j] = 0;
      float best = a[0][j];
#pragma unroll
      for (int d = 1; d < 4; ++d) if (a[d][j] > best) { best = a[d][j]; am[j] = d; }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      float gd[8];
      if (dz) unpack8(*reinterpret_cast<const uint4*>(dz + p[d] * dzcs + cg * 8), gd);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) gd[j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {           // (inline, not bn_acc8: the routed dpool joins in the same pass)
        float t = gd[j] + (am[j] == d ? dp[j] : 0.f);
        if (mask_mode == 1 && !(v[d][j] * sc[j] + sh[j] > 0.f)) t = 0.f;
        gd[j] = t;
        sg[j] += t;
        sgx[j] += t * (v[d][j] - mu[j]) * is[j];
      }
      *reinterpret_cast<uint4*>(g_out + p[d] * C + cg * 8) = pack8(gd);
    }
  }
  bn_block_fold(red, sg, sgx, C, CG, 0, partial);
}

// The pooled reduce with one lane per PIXEL (the 4 pixels of a 2x2 window in the 4
// lanes of a DPP quad, 8 channels each): the window's first maximum of relu(BN(y))
// (bf16-rounded, as the forward stored it) comes from two quad_perm DPP moves, so a
// lane holds 3 loads and a few dozen registers instead of a whole window (13 loads,
// ~150 registers: occupancy/latency bound at 3.4 TB/s).  Unit u: window pixel d =
// u & 3, channel chunk (u >> 2) % CG, window (u >> 2) / CG.  Needs 64 % (C / 8) == 0
// (the grid stride then keeps a thread's d and chunk fixed).
STF_DEV float quad_xor1(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xB1, 0xF, 0xF, false));   // [1,0,3,2]
}
STF_DEV float quad_xor2(float v) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x4E, 0xF, 0xF, false));   // [2,3,0,1]
}

constexpr int PNT = 512;                      // 2x the waves of the other BN kernels: more loads in flight
__global__ __launch_bounds__(PNT) void bn_bwd_reduce_pool_kernel(const uint16_t* __restrict__ dz, int dzcs,
                                          const uint16_t* __restrict__ dpool, const uint16_t* __restrict__ y,
                                          int ycs, long N, int H, int W, int C, int G, int tpg,
                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                          int mask_mode, uint16_t* __restrict__ g_out,
                                          float* __restrict__ partial) {
  __shared__ float red[PNT][17];
  const int CG = C / 8;
  const int g = blockIdx.x / tpg, tile = blockIdx.x - g * tpg;
  const int Wp = W / 2, Hp = H / 2;
  const long wpg = (N / G) * Hp * Wp;                       // windows per group
  const long U = wpg * CG * 4;
  const long gt = (long)tile * PNT + threadIdx.x;
  const int d = (int)(gt & 3);
  const int cg = (int)((gt >> 2) % CG);
  float sc[8], sh[8], mu[8], is[8];
  load_pair(scale, shift, g, C, cg, sc, sh);
  load_pair(mean, invstd, g, C, cg, mu, is);
  const bool relu = mask_mode == 1;
  float sg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sgx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // 32-bit index math (a 64-bit division is a long emulated sequence per unit): every
  // tensor here has < 2^31 windows and pixels (checked by the host)
  const int HpWp = Hp * Wp, cshift = __builtin_ctz(CG);   // CG is a power of two (64 % CG == 0)
  // two units per iteration, all six loads issued before either is used (more bytes in
  // flight per lane); the pair test is quad-uniform (U and the stride are multiples of 4)
  const long S = (long)tpg * PNT;
  auto pix = [&](long u, int& win) {
    win = (int)(u >> (2 + cshift)) + (int)(g * wpg);
    const int n = win / HpWp;
    const int rem = win - n * HpWp;
    const int py = rem / Wp, px = rem - py * Wp;
    return ((long)(n * H + 2 * py + (d >> 1))) * W + 2 * px + (d & 1);
  };
  auto unit = [&](long p, int win, const uint4& yv, const uint4& zv, const uint4& pv) {
    float v[8], gd[8], dp[8];
    unpack8(yv, v);
    if (dz) unpack8(zv, gd);
    else {
#pragma unroll
      for (int j = 0; j < 8; ++j) gd[j] = 0.f;
    }
    unpack8(pv, dp);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float t = v[j] * sc[j] + sh[j];
      const float a = round_e(relu ? fmaxf(t, 0.f) : t);
      float m = fmaxf(a, quad_xor1(a));
      m = fmaxf(m, quad_xor2(m));
      float c = a == m ? (float)d : 4.f;                       // first maximum of the window
      c = fminf(c, quad_xor1(c));
      c = fminf(c, quad_xor2(c));
      float gj = gd[j] + (c == (float)d ? dp[j] : 0.f);    // (inline, not bn_acc8: t is already at hand)
      if (relu && !(t > 0.f)) gj = 0.f;
      gd[j] = gj;
      sg[j] += gj;
      sgx[j] += gj * (v[j] - mu[j]) * is[j];
    }
    *reinterpret_cast<uint4*>(g_out + p * C + cg * 8) = pack8(gd);
  };
  const uint4 zero4 = make_uint4(0, 0, 0, 0);
  for (long u = gt; u < U; u += 2 * S) {
    const bool two = u + S < U;
    int w0, w1 = 0;
    const long p0 = pix(u, w0);
    const long p1 = two ? pix(u + S, w1) : p0;
    const uint4 y0 = *reinterpret_cast<const uint4*>(y + p0 * ycs + cg * 8);
    const uint4 z0 = dz ? *reinterpret_cast<const uint4*>(dz + p0 * dzcs + cg * 8) : zero4;
    const uint4 q0 = *reinterpret_cast<const uint4*>(dpool + (long)w0 * C + cg * 8);
    uint4 y1 = zero4, z1 = zero4, q1 = zero4;
    if (two) {
      y1 = *reinterpret_cast<const uint4*>(y + p1 * ycs + cg * 8);
      if (dz) z1 = *reinterpret_cast<const uint4*>(dz + p1 * dzcs + cg * 8);
      q1 = *reinterpret_cast<const uint4*>(dpool + (long)w1 * C + cg * 8);
    }
    unit(p0, w0, y0, z0, q0);
    if (two) unit(p1, w1, y1, z1, q1);
  }
  bn_block_fold<4>(red, sg, sgx, C, 4 * CG, 0, partial);   // threads holding chunk gg: (t >> 2) % CG == gg
}

// partial: [G][T][2][C] (first S rows per group folded).  coef: [G][3][C].
// Grid = (channel chunks of 16) x G.  dgamma/dbeta are summed over the groups
// (one BatchNorm module, G calls): with G > 1 each block parks its group's sums
// in row 0 of the group and bn_groupsum_batch_kernel adds them in order.
__global__ __launch_bounds__(stf::FOLD_NT) void bn_bwd_finalize_kernel(float* __restrict__ partial, int S, int T, int G,
                                                            int C, long Mg, const float* gamma, const float* mean,
                                                            const float* invstd, float* dgamma, float* dbeta,
                                                            float* coef) {
  __shared__ double red[stf::FOLD_NT];
  const int g = blockIdx.y;
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);
  const bool cok = c < C, lead = cok && (threadIdx.x >> 4) == 0;
  float* base = partial + (size_t)g * T * 2 * C;
  double s1, s2;
  stf::fold16_pair(base, S, 2L * C, C, c, cok, red, s1, s2);
  if (lead) bn_fin_bwd_out(base, g, c, G, C, Mg, s1, s2, gamma, mean, invstd, dgamma, dbeta, coef);
}

// The running-statistics updates of grouped BatchNorms, group by group in order, many BatchNorms in
// one launch (blockIdx.y = descriptor): stf_bn_running_batch's deferred ones, or the single
// descriptor of a stf_bn_finalize call that was given the running statistics.
constexpr int RUN_BATCH = 32;
struct RunBatch { stf_bn_run_desc d[RUN_BATCH]; };
__global__ void bn_running_batch_kernel(RunBatch b) {
  const stf_bn_run_desc& d = b.d[blockIdx.y];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d.C) return;
  float run_m = d.running_mean[c], run_v = d.running_var[c];
  const long Mg = (long)d.Mg;
  for (int g = 0; g < d.groups; ++g) {
    const float* base = d.stats + (size_t)g * d.tiles * 2 * d.C;
    const double var = base[d.C + c];
    const double unb = Mg > 1 ? var * Mg / (Mg - 1) : var;
    run_m = (1.f - d.momentum) * run_m + d.momentum * base[c];
    run_v = (1.f - d.momentum) * run_v + d.momentum * (float)unb;
  }
  d.running_mean[c] = run_m;
  d.running_var[c] = run_v;
}

// The dgamma/dbeta sums over the groups of grouped BatchNorm backwards, many in one launch
// (stf_bn_groupsum_batch, or the single descriptor of a stf_bn_bwd_finalize call that wants them)
struct GsumBatch { stf_bn_gsum_desc d[RUN_BATCH]; };
__global__ void bn_groupsum_batch_kernel(GsumBatch b) {
  const stf_bn_gsum_desc& d = b.d[blockIdx.y];
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= d.C) return;
  double dg = 0.0, db = 0.0;
  for (int g = 0; g < d.groups; ++g) {
    const float* base = d.partial + (size_t)g * d.tiles * 2 * d.C;
    db += base[c];
    dg += base[d.C + c];
  }
  if (d.dgamma) d.dgamma[c] = (float)dg;
  if (d.dbeta) d.dbeta[c] = (float)db;
}

// ------------------------------------------------------------------ group-major streaming passes
// The three element-wise passes with the grid split by statistics group (blockIdx.y = g):
// a thread's channel chunk and its group's affine / coefficient vectors are fixed, so the loop
// carries no per-unit division (bn_act_kernel divides 64-bit unit and pixel indices by C/8
// and by the group size for every 16-B unit), and every thread issues the loads of UPT units
// (a block covers UPT x 256 consecutive units per iteration)
// before it uses any (UPT x 2-3 16-B loads in flight per lane: the STF encoder's 8-67 MB tensors
// are latency-bound at one unit per iteration).  Index math is 32-bit: units per group < 2^31
// (bn_route, rule 3).  Unit u of group g: pixel g * Mg + (u >> cgs), chunk u & (CG - 1).
constexpr int UPT = 4;

template <bool RES>
__global__ __launch_bounds__(NT) void bn_act_g_kernel(const uint16_t* __restrict__ y, int ycs, int Mg, int cgs,
                                                      const float* scale, const float* shift, int relu,
                                                      int res_mode, const uint16_t* __restrict__ res, int rcs,
                                                      const float* __restrict__ rscale,
                                                      const float* __restrict__ rshift, uint16_t* __restrict__ out,
                                                      int ocs) {
  const int g = blockIdx.y, C = 8 << cgs;
  const int upg = Mg << cgs, S = gridDim.x * NT * UPT;
  const int u0 = blockIdx.x * NT * UPT + threadIdx.x;
  const int cg = threadIdx.x & ((1 << cgs) - 1);
  float sc[8], sh[8], rs[8], rh[8];
  load_pair(scale, shift, g, C, cg, sc, sh);
  if (RES && res_mode == 2) load_pair(rscale, rshift, g, C, cg, rs, rh);
  const size_t p0 = (size_t)g * Mg;
  for (int u = u0; u < upg; u += S) {
    uint4 yv[UPT], rv[UPT];
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int uk = u + k * NT;
      if (uk < upg) {
        const size_t p = p0 + (uk >> cgs);
        yv[k] = *reinterpret_cast<const uint4*>(y + p * ycs + cg * 8);
        if (RES) rv[k] = *reinterpret_cast<const uint4*>(res + p * rcs + cg * 8);
      }
    }
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int uk = u + k * NT;
      if (uk >= upg) break;
      float v[8];
      unpack8(yv[k], v);
      bn_affine8(v, sc, sh, relu, RES ? (res_mode == 2 ? 2 : 1) : 0, &rv[k], rs, rh);
      *reinterpret_cast<uint4*>(out + (p0 + (uk >> cgs)) * ocs + cg * 8) = pack8(v);
    }
  }
}

// MASK 0: none, 1: relu(y*scale+shift) > 0, 2: mask_src > 0
template <int MASK>
__global__ __launch_bounds__(NT) void bn_bwd_reduce_g_kernel(const uint16_t* __restrict__ dz, int dzcs,
                                                             const uint16_t* __restrict__ y, int ycs, int Mg,
                                                             int cgs, const float* __restrict__ scale,
                                                             const float* __restrict__ shift,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ invstd,
                                                             const uint16_t* __restrict__ msrc, int mcs,
                                                             uint16_t* __restrict__ g_out, float* __restrict__ partial) {
  __shared__ float red[NT][17];
  const int g = blockIdx.y, CG = 1 << cgs, C = 8 << cgs;
  const int upg = Mg << cgs, S = gridDim.x * NT * UPT;
  const int u0 = blockIdx.x * NT * UPT + threadIdx.x;
  const int cg = threadIdx.x & (CG - 1);
  float sc[8], sh[8], mu[8], is[8];
  if (MASK == 1) load_pair(scale, shift, g, C, cg, sc, sh);
  load_pair(mean, invstd, g, C, cg, mu, is);
  float sg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sgx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const size_t p0 = (size_t)g * Mg;
  for (int u = u0; u < upg; u += S) {
    uint4 yv[UPT], zv[UPT], mv[UPT];
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int uk = u + k * NT;
      if (uk < upg) {
        const size_t p = p0 + (uk >> cgs);
        yv[k] = *reinterpret_cast<const uint4*>(y + p * ycs + cg * 8);
        zv[k] = *reinterpret_cast<const uint4*>(dz + p * dzcs + cg * 8);
        if (MASK == 2) mv[k] = *reinterpret_cast<const uint4*>(msrc + p * mcs + cg * 8);
      }
    }
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int uk = u + k * NT;
      if (uk >= upg) break;
      float v[8], d[8], mk[8];
      unpack8(yv[k], v);
      unpack8(zv[k], d);
      if (MASK == 2) unpack8(mv[k], mk);
      bn_acc8(MASK, d, v, sc, sh, mk, mu, is, sg, sgx);
      if (g_out) *reinterpret_cast<uint4*>(g_out + (p0 + (uk >> cgs)) * C + cg * 8) = pack8(d);
    }
  }
  bn_block_fold(red, sg, sgx, C, CG, g, partial);
}

// dy = A*g' + B*y + C, g' = g (already masked) or, with MASK, the ReLU mask recomputed from y:
// g' = (y*mscale+mshift > 0) ? g : 0 (saves the masked copy); bias_partial rows = g * gridDim.x + blockIdx.x
template <bool MASK>
__global__ __launch_bounds__(NT) void bn_bwd_apply_g_kernel(const uint16_t* g_in, int gcs,
                                                            const uint16_t* __restrict__ y, int ycs, int Mg, int cgs,
                                                            const float* coef, const float* __restrict__ mscale,
                                                            const float* __restrict__ mshift, uint16_t* dy,
                                                            int dycs, float* __restrict__ bias_partial) {
  __shared__ float red[NT][9];
  const int g = blockIdx.y, CG = 1 << cgs, C = 8 << cgs;
  const int upg = Mg << cgs, S = gridDim.x * NT * UPT;
  const int u0 = blockIdx.x * NT * UPT + threadIdx.x;
  const int cg = threadIdx.x & (CG - 1);
  float A[8], B[8], Cc[8], ms[8], mh[8];
  load_coef(coef, g, C, cg, A, B, Cc);
  if (MASK) load_pair(mscale, mshift, g, C, cg, ms, mh);
  float sb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const size_t p0 = (size_t)g * Mg;
  for (int u = u0; u < upg; u += S) {
    uint4 gq[UPT], yq[UPT];
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int uk = u + k * NT;
      if (uk < upg) {
        const size_t p = p0 + (uk >> cgs);
        gq[k] = *reinterpret_cast<const uint4*>(g_in + p * gcs + cg * 8);
        yq[k] = *reinterpret_cast<const uint4*>(y + p * ycs + cg * 8);
      }
    }
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
      const int uk = u + k * NT;
      if (uk >= upg) break;
      float gv[8], yv[8];
      unpack8(gq[k], gv);
      unpack8(yq[k], yv);
      bn_dy8(MASK, gv, yv, ms, mh, A, B, Cc, sb);
      *reinterpret_cast<uint4*>(dy + (p0 + (uk >> cgs)) * dycs + cg * 8) = pack8(gv);
    }
  }
  if (!bias_partial) return;
  bn_block_fold(red, sb, sb, C, CG, g, bias_partial);
}

// ------------------------------------------------------------------ stem: BN through MaxPool(3,2,1)
// Forward: the stem's BatchNorm + ReLU fused into its max pool (src/stf_lstm_unet.py:178-180): each
// window tap is relu(y*scale[g]+shift[g]) rounded to the 16-bit storage -- exactly the value
// stf_bn_act would have stored in the activation a0 -- so the pooled output and the recorded
// argmax equal bn_act followed by stf.hip's maxpool3_fwd_kernel bit for bit, and a0 (4x the pooled
// bytes) is never written nor read back.  g = n / ipg (per-time-step statistics of the encoder).
// (The 3x3 scan repeats maxpool3_fwd_kernel's with the affine inside.  The two stay apart: that one
// indexes 64-bit units and this one 32-bit, so a shared scan would take the tap's value as a callable
// and both index types as parameters -- more lines than the 12 it saves.)
__global__ void bn_act_maxpool3_kernel(const uint16_t* __restrict__ y, int N, int H, int W, int C, int Ho, int Wo,
                                       int ipg, const float* __restrict__ scale, const float* __restrict__ shift,
                                       uint16_t* __restrict__ out, uint8_t* __restrict__ argmax) {
  // 32-bit index math (the host checks units < 2^31; 64-bit divisions made this VALU-bound)
  const int CG = C / 8, HoWo = Ho * Wo;
  const int units = N * HoWo * CG;
  for (int u = blockIdx.x * NT + threadIdx.x; u < units; u += gridDim.x * NT) {
    const int p = u / CG, cg = u - p * CG;
    const int n = p / HoWo;
    const int rem = p - n * HoWo;
    const int oy = rem / Wo, ox = rem - oy * Wo;
    float sc[8], sh[8];
    load_pair(scale, shift, n / ipg, C, cg, sc, sh);
    // every valid tap's value is >= 0 (ReLU) > -inf, so the first valid tap always takes the
    // maximum and a strict '>' keeps the first maximum in row-major window order
    float mx[8];
    int am[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { mx[j] = -INFINITY; am[j] = 0; }
    for (int dy = 0; dy < 3; ++dy) {
      const int iy = 2 * oy - 1 + dy;
      if (iy < 0 || iy >= H) continue;
      for (int dx = 0; dx < 3; ++dx) {
        const int ix = 2 * ox - 1 + dx;
        if (ix < 0 || ix >= W) continue;
        float v[8];
        unpack8(*reinterpret_cast<const uint4*>(y + (((long)n * H + iy) * W + ix) * C + cg * 8), v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float a = round_e(fmaxf(v[j] * sc[j] + sh[j], 0.f));     // bn_act's stored value
          if (a > mx[j]) { mx[j] = a; am[j] = dy * 3 + dx; }
        }
      }
    }
    const size_t o = (size_t)p * C + cg * 8;          // N*Ho*Wo*C may pass 2^31 (units < 2^31 only)
    *reinterpret_cast<uint4*>(out + o) = pack8(mx);
    if (argmax) {
      uint32_t lo = 0, hi = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { lo |= (uint32_t)am[j] << (8 * j); hi |= (uint32_t)am[4 + j] << (8 * j); }
      *reinterpret_cast<uint2*>(argmax + o) = make_uint2(lo, hi);
    }
  }
}

// Backward: g of the stem's BatchNorm gathered straight from its max pool's backward: the sum of dout over the <= 4 windows whose recorded first maximum (argmax, index dy*3+dx) is this pixel,
// in the order stf_maxpool3s2_bwd adds them, rounded to the 16-bit storage -- so the values equal
// maxpool3s2_bwd + the mask-recomputing reduce / apply without writing or reading d a0.  A unit is
// a 2x2 block of input pixels (2by + a, 2bx + b): the windows (by + {0,1}, bx + {0,1}) cover all
// four, so each window's argmax and dout are loaded once per block (9 window reads for the four
// pixels in the per-pixel gather).
// APPLY = false: the (sum g, sum g*xhat) partials of bn_bwd_reduce_g_kernel<1>;
// APPLY = true: dy = A*g' + B*y + C with the ReLU mask recomputed (bn_bwd_apply_g_kernel<true>)
template <bool APPLY>
__global__ __launch_bounds__(NT) void bn_bwd_pool3_kernel(const uint8_t* __restrict__ argmax,
                                                          const uint16_t* __restrict__ dout,
                                                          const uint16_t* __restrict__ y, int H, int W, int Ho,
                                                          int Wo, int ipg, int cgs, const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ invstd,
                                                          const float* __restrict__ coef, uint16_t* __restrict__ dy,
                                                          float* __restrict__ partial) {
  __shared__ float red[APPLY ? 1 : NT][17];
  const int g = blockIdx.y, CG = 1 << cgs, C = 8 << cgs;
  const int H2 = (H + 1) >> 1, W2 = (W + 1) >> 1;
  const int bpi = H2 * W2;                               // 2x2 blocks per image
  const int upg = (ipg * bpi) << cgs, S = gridDim.x * NT;
  const int u0 = blockIdx.x * NT + threadIdx.x;
  const int cg = threadIdx.x & (CG - 1);
  float sc[8], sh[8], mu[8], is[8], A[8], B[8], Cc[8];
  load_pair(scale, shift, g, C, cg, sc, sh);
  if (APPLY) load_coef(coef, g, C, cg, A, B, Cc);
  else load_pair(mean, invstd, g, C, cg, mu, is);
  float sg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sgx[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // U units per iteration, all their loads issued before any use (the reduce runs <= 1024
  // blocks -- the finalize's row budget -- so it needs the memory-level parallelism per thread)
  constexpr int U = APPLY ? 1 : 2;
  for (int u = u0; u < upg; u += S * U) {
    uint2 am[U][2][2];
    uint4 dr[U][2][2], yr[U][2][2];
    int nn[U], bys[U], bxs[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int uk = u + k * S;
      const int b = uk >> cgs;
      const int n = g * ipg + b / bpi, rb = b - (b / bpi) * bpi;
      const int by = rb / W2, bx = rb - by * W2;
      nn[k] = uk < upg ? n : -1;
      bys[k] = by;
      bxs[k] = bx;
      // the four windows (by + wy, bx + wx): argmax (8 channel bytes) and dout (8 channels),
      // and the block's four pixels of y
#pragma unroll
      for (int wy = 0; wy < 2; ++wy)
#pragma unroll
        for (int wx = 0; wx < 2; ++wx) {
          const int oy = by + wy, ox = bx + wx;
          if (uk < upg && oy < Ho && ox < Wo) {
            const long wo = (((long)n * Ho + oy) * Wo + ox) * C + cg * 8;
            am[k][wy][wx] = *reinterpret_cast<const uint2*>(argmax + wo);
            dr[k][wy][wx] = *reinterpret_cast<const uint4*>(dout + wo);
          } else {
            am[k][wy][wx] = make_uint2(0xffffffffu, 0xffffffffu);    // matches no pixel
            dr[k][wy][wx] = make_uint4(0, 0, 0, 0);
          }
          const int iy = 2 * by + wy, ix = 2 * bx + wx;
          if (uk < upg && iy < H && ix < W)
            yr[k][wy][wx] = *reinterpret_cast<const uint4*>(y + (((size_t)n * H + iy) * W + ix) * C + cg * 8);
          else
            yr[k][wy][wx] = make_uint4(0, 0, 0, 0);
        }
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      if (nn[k] < 0) continue;
      const int n = nn[k], by = bys[k], bx = bxs[k];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
          const int iy = 2 * by + a, ix = 2 * bx + bb;
          if (iy >= H || ix >= W) continue;
          float v[8], gq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
          unpack8(yr[k][a][bb], v);
          // windows of pixel row iy: oy = by (always) and by + 1 (odd iy); same for x; ascending
#pragma unroll
          for (int wy = 0; wy < 2; ++wy) {
            if (wy > a) continue;
#pragma unroll
            for (int wx = 0; wx < 2; ++wx) {
              if (wx > bb) continue;
              const uint32_t me = (uint32_t)((iy - 2 * (by + wy) + 1) * 3 + (ix - 2 * (bx + wx) + 1));
              float d[8];
              unpack8(dr[k][wy][wx], d);
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                const uint32_t q = ((j < 4 ? am[k][wy][wx].x : am[k][wy][wx].y) >> (8 * (j & 3))) & 0xffu;
                if (q == me) gq[j] += d[j];
              }
            }
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) gq[j] = round_e(gq[j]);
          if (APPLY) {
            bn_dy8(true, gq, v, sc, sh, A, B, Cc, sg);                  // (sg: no bias sum here, unused)
            *reinterpret_cast<uint4*>(dy + (((size_t)n * H + iy) * W + ix) * C + cg * 8) = pack8(gq);
          } else {
            bn_acc8(1, gq, v, sc, sh, nullptr, mu, is, sg, sgx);
          }
        }
    }
  }
  if constexpr (!APPLY) bn_block_fold(red, sg, sgx, C, CG, g, partial);
}

// ------------------------------------------------------------------ the route
// What a streaming launch is asked for: the shape and the options that pick a kernel or size a grid
// (strides and pointers do neither; the entry points check those themselves).
enum class BnOp { Act, Reduce, Apply, ActPool3, ReducePool3, ApplyPool3 };
struct BnSig {
  BnOp op;
  long N;                  // images; Apply: the M pixels (H = W = 1)
  int H, W, C, groups;
  bool pooled = false;     // Act: the 2x2 max pool is written too; Reduce: dpool joins
  int mask = 0;            // Reduce: mask_mode 0 / 1 / 2; Apply: 1 = the ReLU mask is recomputed
  bool res = false;        // Act: a residual joins
  bool bias = false;       // Apply: the per-block bias sums are wanted
};
enum class BnKernel {
  None, ActG, ActGRes, ActFlat, ActFlatPool, ReduceG0, ReduceG1, ReduceG2, ReduceDpp, ReduceWin, ApplyG, ApplyGMask,
  ActPool3, ReducePool3, ApplyPool3
};
struct BnRoute {
  bool refused = true;     // STF_EINVAL, nothing is launched
  BnKernel kernel = BnKernel::None;
  int block = NT;
  dim3 grid;               // grid.x == 0: nothing to do (an empty tensor)
  int rows = 0;            // partial rows per group the launch writes (0: the kernel writes no partials)
  int alloc = 1;           // rows the caller allocates: per group (Reduce), over all groups (Apply)
  int cgs = 0;             // log2(C / 8) where rule 4 holds
  long Mg = 0;             // pixels per group
};

// The rules (a unit = 8 channels of one pixel, of one 2x2 window where the 2x2 pool joins, of one
// 2x2 block of input pixels in the stem's backward, of one pooled pixel in the stem's forward; upg =
// units per group):
//  1. Row budget.  A reduce writes one partial row per block and stf_bn_bwd_finalize's fp64 fold reads
//     up to FOLD16_ROWS = 1024 rows directly (more cost it a first colsum stage), so a reduce runs
//     ceil(upg / 256) blocks per group, at most ceil(1024 / groups), at least one: these are the rows of
//     stf_bn_bwd_tiles.  The bias sums of the apply come under the same budget, over all groups at
//     once: stf_bn_bwd_apply_tiles = ceil(M * (C / 8) / 256), at most 1024, at least one.
//  2. Block cap.  A streaming grid without partial rows has at most 8192 blocks (32 per CU: enough to
//     hide the tail, and a grid-stride loop beyond it); the flat kernels run min(ceil(units / 256),
//     8192), the group-major ones -- UPT units per thread and iteration -- ceil(upg / (256 * UPT))
//     blocks per group, at most max(8192 / groups, 1), at least one.  With bias sums the apply's cap is
//     rule 1's allocation in place of 8192; more groups than allocated rows (every group needs a block
//     of its own) is refused: groups x rows <= the allocation always.
//  3. 2^31 units.  The group-major and stem kernels index units and pixels in 32 bits: a group of
//     2^31 units or more is refused (the forward instead falls to the flat kernel, which divides 64-bit
//     indices), and so is a stem tensor of 2^31 pixels.  The stem's forward adds its grid stride:
//     units < 2^31 - 8192 * 256, and N*H*W*C < 2^34.
//  4. Power-of-two chunks.  The backward kernels and the group-major forward keep a thread's channel
//     chunk fixed: C / 8 divides the 256-thread block (so it is a power of two; C <= 2048).  Otherwise
//     the backward is refused and the forward takes the flat kernel (any C % 8 == 0).
//  5. DPP or window.  The pooled reduce puts a 2x2 window in a DPP quad, 512 threads a block (3 loads
//     and a few dozen registers per lane against 13 loads and ~150: the window form was occupancy /
//     latency bound at 3.4 TB/s), when 64 % (C / 8) == 0 (the grid stride then keeps a lane's pixel
//     and chunk fixed) and the tensor has fewer than 2^31 pixels (its 32-bit index math); else one
//     thread per window (C = 1024, 2048).  Both take rule 1's rows, counted in 256-unit blocks of
//     windows, as one flat grid of rows x groups blocks.
//  6. Stem grids.  The stem's reduce takes rule 1's rows for the UNPOOLED pixel count, because that is
//     what its caller allocates (stf_bn_bwd_tiles with pooled = 0; include/stfunet.h says so), although
//     its units are 2x2 blocks, a quarter as many: a block then meets ~64 units per iteration pair
//     and the kernel issues two units' loads per thread to keep bytes in flight.  The stem's apply
//     takes one unit per thread and iteration where rule 2's kernels take UPT, so it runs UPT blocks
//     for each block of rule 2: up to UPT x 8192 in all.  The stem's forward is a flat grid of rule 2.
constexpr long ROW_CAP = stf::FOLD16_ROWS, BLOCK_CAP = 8192, IDX_CAP = 1L << 31;

BnRoute bn_route(const BnSig& s) {
  BnRoute r;
  if (s.groups < 1) return r;
  const auto clamp = [](long want, long most) { return (int)std::max<long>(1, std::min(want, most)); };
  const auto ceil_div = [](long x, long y) { return (x + y - 1) / y; };
  const int CG = s.C / 8, Ho = (s.H - 1) / 2 + 1, Wo = (s.W - 1) / 2 + 1;
  const long Ng = s.N / s.groups, px = s.N * s.H * s.W;
  r.Mg = Ng * s.H * s.W;
  const bool chunk_ok = s.C >= 8 && s.C % 8 == 0 && NT % CG == 0;                  // rule 4
  const bool g_ok = chunk_ok && r.Mg * CG < IDX_CAP;                               // rules 3, 4
  if (chunk_ok) r.cgs = 31 - __builtin_clz(CG);
  const bool uneven = s.N % s.groups != 0, odd = ((s.H | s.W) & 1) != 0;
  const long upg = Ng * CG * (s.op == BnOp::ApplyPool3 ? (long)((s.H + 1) / 2) * ((s.W + 1) / 2)
                              : s.pooled ? (long)(s.H / 2) * (s.W / 2) : (long)s.H * s.W);
  const auto rows_of = [&](long units) { return clamp(ceil_div(units, NT), ceil_div(ROW_CAP, s.groups)); };   // rule 1
  const auto blocks_of = [&](long cap) { return clamp(ceil_div(upg, (long)NT * UPT), cap / s.groups); };      // rule 2
  const auto flat = [&](long units) { return (unsigned)std::min(ceil_div(units, NT), BLOCK_CAP); };           // rule 2
  switch (s.op) {
    case BnOp::Act:
      r.refused = s.C % 8 || uneven || (s.pooled && (odd || s.res));
      if (!s.pooled && g_ok) {
        r.kernel = s.res ? BnKernel::ActGRes : BnKernel::ActG;
        r.grid = dim3(upg ? blocks_of(BLOCK_CAP) : 0, s.groups);
      } else {
        r.kernel = s.pooled ? BnKernel::ActFlatPool : BnKernel::ActFlat;
        r.grid = dim3(flat(upg * s.groups));
      }
      break;
    case BnOp::Reduce:
      r.refused = !chunk_ok || uneven || (s.pooled ? odd || s.mask == 2 : !g_ok);
      r.rows = r.alloc = rows_of(upg);
      if (!s.pooled) {
        r.kernel = s.mask == 1 ? BnKernel::ReduceG1 : s.mask == 2 ? BnKernel::ReduceG2 : BnKernel::ReduceG0;
        r.grid = dim3(r.rows, s.groups);
      } else {                                                                     // rule 5
        const bool dpp = chunk_ok && 64 % CG == 0 && px < IDX_CAP;
        r.kernel = dpp ? BnKernel::ReduceDpp : BnKernel::ReduceWin;
        r.block = dpp ? PNT : NT;
        r.grid = dim3(r.rows * s.groups);
      }
      break;
    case BnOp::Apply:
      r.alloc = clamp(ceil_div(px * CG, NT), ROW_CAP);
      r.rows = blocks_of(s.bias ? r.alloc : BLOCK_CAP);
      r.refused = !g_ok || uneven || (s.bias && (long)r.rows * s.groups > r.alloc);
      r.kernel = s.mask ? BnKernel::ApplyGMask : BnKernel::ApplyG;
      r.grid = dim3(r.rows, s.groups);
      if (!s.bias) r.rows = 0;
      break;
    case BnOp::ActPool3: {                                                         // rules 3, 6
      const long units = s.N * Ho * Wo * CG;
      r.refused = s.C % 8 || uneven || units >= IDX_CAP - BLOCK_CAP * NT || px * s.C >= IDX_CAP * 8;
      r.kernel = BnKernel::ActPool3;
      r.grid = dim3(std::max(flat(units), 1u));
      break;
    }
    case BnOp::ReducePool3:                                                        // rule 6
      r.refused = !g_ok || uneven || px >= IDX_CAP;
      r.kernel = BnKernel::ReducePool3;
      r.rows = r.alloc = rows_of(r.Mg * CG);
      r.grid = dim3(r.rows, s.groups);
      break;
    case BnOp::ApplyPool3:                                                         // rule 6
      r.refused = !g_ok || uneven || px >= IDX_CAP;
      r.kernel = BnKernel::ApplyPool3;
      r.grid = dim3(blocks_of(BLOCK_CAP) * UPT, s.groups);
      break;
  }
  return r;
}

}  // namespace

// sum over tiles of partial[t][C] -> out[C] (fixed order); shared with misc.hip / loss.hip
// launch: grid ceil(C/16), 256 threads (16 channels x 16 row-lanes)
__global__ __launch_bounds__(stf::FOLD_NT) void stf_tile_sum_kernel(const float* __restrict__ partial, int tiles, int C,
                                                         float* __restrict__ out) {
  __shared__ double red[stf::FOLD_NT];
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);
  const bool cok = c < C;
  const double s = stf::fold16_finish(stf::fold16_partial(partial, tiles, C, c, cok), red);
  if (cok && (threadIdx.x >> 4) == 0) out[c] = (float)s;
}

extern "C" int stf_bn_finalize(float* stats, int tiles, int groups, int C, int64_t M, const float* gamma,
                               const float* beta, float momentum, float eps, float* running_mean,
                               float* running_var, float* mean, float* invstd, float* scale, float* shift,
                               stf_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (groups < 1 || M % groups) return STF_EINVAL;
  const int S = stats ? stf::colsum_stage1(stats, tiles, 2L * C, s, groups, stf::FOLD16_ROWS) : 0;
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 15) / 16, groups), dim3(stf::FOLD_NT), 0, s, stats, S, tiles, groups, C,
                     (long)(M / groups), gamma, beta, momentum, eps, running_mean, running_var, mean, invstd,
                     scale, shift);
  STF_CHECK_LAUNCH();
  if (stats && running_mean && groups > 1) {
    RunBatch b;
    b.d[0] = stf_bn_run_desc{stats, running_mean, running_var, M / groups, tiles, groups, C, momentum};
    hipLaunchKernelGGL(bn_running_batch_kernel, dim3((C + 255) / 256, 1), dim3(256), 0, s, b);
    STF_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int stf_bn_act(const void* y, int y_cstride, int N, int H, int W, int C, int groups,
                          const float* scale, const float* shift, int relu, const void* res, int res_cstride,
                          const float* res_scale, const float* res_shift, void* out, int out_cstride,
                          void* pooled, stf_stream_t stream) {
  const BnRoute r = bn_route({BnOp::Act, N, H, W, C, groups, pooled != nullptr, 0, res != nullptr});
  if (r.refused || y_cstride % 8 || out_cstride % 8 || (res && res_cstride % 8)) return STF_EINVAL;
  if (!r.grid.x) return 0;
  const int res_mode = res ? (res_scale ? 2 : 1) : 0;
  const auto group_major = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, r.grid, dim3(r.block), 0, (hipStream_t)stream, (const uint16_t*)y, y_cstride, (int)r.Mg,
                       r.cgs, scale, shift, relu, res_mode, (const uint16_t*)res, res_cstride, res_scale, res_shift,
                       (uint16_t*)out, out_cstride);
  };
  const auto flat = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, r.grid, dim3(r.block), 0, (hipStream_t)stream, (const uint16_t*)y, y_cstride, (long)N, H,
                       W, C, r.Mg, scale, shift, relu, res_mode, (const uint16_t*)res, res_cstride, res_scale,
                       res_shift, (uint16_t*)out, out_cstride, (uint16_t*)pooled);
  };
  switch (r.kernel) {
    case BnKernel::ActG: group_major(bn_act_g_kernel<false>); break;
    case BnKernel::ActGRes: group_major(bn_act_g_kernel<true>); break;
    case BnKernel::ActFlat: flat(bn_act_kernel<false>); break;
    case BnKernel::ActFlatPool: flat(bn_act_kernel<true>); break;
    default: return STF_EINVAL;
  }
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_bn_bwd_tiles(int N, int H, int W, int C, int groups, int pooled) {
  return bn_route({BnOp::Reduce, N, H, W, C, groups, pooled != 0}).alloc;
}

extern "C" int stf_bn_bwd_reduce(const void* dz, int dz_cstride, const void* dpool, const void* y, int y_cstride,
                                 int N, int H, int W, int C, int groups, const float* scale, const float* shift,
                                 const float* mean, const float* invstd, int mask_mode, const void* mask_src,
                                 int mask_cstride, void* g_out, float* partial, stf_stream_t stream) {
  const BnRoute r = bn_route({BnOp::Reduce, N, H, W, C, groups, dpool != nullptr, mask_mode});
  if (r.refused || y_cstride % 8 || (dz && dz_cstride % 8)) return STF_EINVAL;
  if (!dz && !dpool) return STF_EINVAL;
  if (!g_out && dpool) return STF_EINVAL;            // the pooled routing must be materialized
  if (mask_mode == 2 && (!mask_src || mask_cstride % 8)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const auto group_major = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, r.grid, dim3(r.block), 0, s, (const uint16_t*)dz, dz_cstride, (const uint16_t*)y,
                       y_cstride, (int)r.Mg, r.cgs, scale, shift, mean, invstd, (const uint16_t*)mask_src,
                       mask_cstride, (uint16_t*)g_out, partial);
  };
  switch (r.kernel) {
    case BnKernel::ReduceG0: group_major(bn_bwd_reduce_g_kernel<0>); break;
    case BnKernel::ReduceG1: group_major(bn_bwd_reduce_g_kernel<1>); break;
    case BnKernel::ReduceG2: group_major(bn_bwd_reduce_g_kernel<2>); break;
    case BnKernel::ReduceDpp:
      hipLaunchKernelGGL(bn_bwd_reduce_pool_kernel, r.grid, dim3(r.block), 0, s, (const uint16_t*)dz, dz_cstride,
                         (const uint16_t*)dpool, (const uint16_t*)y, y_cstride, (long)N, H, W, C, groups, r.rows, scale,
                         shift, mean, invstd, mask_mode, (uint16_t*)g_out, partial);
      break;
    case BnKernel::ReduceWin:
      hipLaunchKernelGGL(bn_bwd_reduce_win_kernel, r.grid, dim3(r.block), 0, s, (const uint16_t*)dz, dz_cstride,
                         (const uint16_t*)dpool, (const uint16_t*)y, y_cstride, (long)N, H, W, C, groups, r.rows, scale,
                         shift, mean, invstd, mask_mode, (const uint16_t*)mask_src, mask_cstride, (uint16_t*)g_out,
                         partial);
      break;
    default: return STF_EINVAL;
  }
  STF_CHECK_LAUNCH();
  return 0;
}

extern "C" int stf_bn_bwd_finalize(float* partial, int tiles, int groups, int C, int64_t M, const float* gamma,
                                   const float* mean, const float* invstd, float* dgamma, float* dbeta, float* coef,
                                   stf_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (groups < 1 || M % groups) return STF_EINVAL;
  const int S = stf::colsum_stage1(partial, tiles, 2L * C, s, groups, stf::FOLD16_ROWS);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 15) / 16, groups), dim3(stf::FOLD_NT), 0, s, partial, S, tiles, groups,
                     C, (long)(M / groups), gamma, mean, invstd, dgamma, dbeta, coef);
  STF_CHECK_LAUNCH();
  if (groups > 1 && (dgamma || dbeta)) {
    GsumBatch b;
    b.d[0] = stf_bn_gsum_desc{partial, dgamma, dbeta, tiles, groups, C};
    hipLaunchKernelGGL(bn_groupsum_batch_kernel, dim3((C + 255) / 256, 1), dim3(256), 0, s, b);
    STF_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int stf_bn_running_batch(const stf_bn_run_desc* descs, int count, stf_stream_t stream) {
  for (int i = 0; i < count; ++i)
    if (!descs[i].stats || !descs[i].running_mean || !descs[i].running_var || descs[i].groups < 1 ||
        descs[i].C < 1 || descs[i].tiles < 1)
      return STF_EINVAL;
  for (int i0 = 0; i0 < count; i0 += RUN_BATCH) {
    const int n = count - i0 < RUN_BATCH ? count - i0 : RUN_BATCH;
    RunBatch b;
    int cmax = 0;
    for (int i = 0; i < n; ++i) { b.d[i] = descs[i0 + i]; cmax = cmax > b.d[i].C ? cmax : b.d[i].C; }
    hipLaunchKernelGGL(bn_running_batch_kernel, dim3((cmax + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, b);
    STF_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int stf_bn_groupsum_batch(const stf_bn_gsum_desc* descs, int count, stf_stream_t stream) {
  for (int i = 0; i < count; ++i)
    if (!descs[i].partial || descs[i].groups < 1 || descs[i].C < 1 || descs[i].tiles < 1) return STF_EINVAL;
  for (int i0 = 0; i0 < count; i0 += RUN_BATCH) {
    const int n = count - i0 < RUN_BATCH ? count - i0 : RUN_BATCH;
    GsumBatch b;
    int cmax = 0;
    for (int i = 0; i < n; ++i) { b.d[i] = descs[i0 + i]; cmax = cmax > b.d[i].C ? cmax : b.d[i].C; }
    hipLaunchKernelGGL(bn_groupsum_batch_kernel, dim3((cmax + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, b);
    STF_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int stf_bn_bwd_apply_tiles(int64_t M, int C) {
  return bn_route({BnOp::Apply, M, 1, 1, C, 1, false, 0, false, true}).alloc;
}

extern "C" int stf_bn_bwd_apply(const void* g, int g_cstride, const void* y, int y_cstride, int64_t M, int C,
                                int groups, const float* mask_scale, const float* mask_shift, const float* coef,
                                void* dy, int dy_cstride, float* bias_partial, float* dbias, stf_stream_t stream) {
  const BnRoute r =
      bn_route({BnOp::Apply, M, 1, 1, C, groups, false, mask_scale != nullptr, false, bias_partial != nullptr});
  if (r.refused || y_cstride % 8 || dy_cstride % 8 || g_cstride % 8) return STF_EINVAL;
  if ((mask_scale == nullptr) != (mask_shift == nullptr)) return STF_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  const auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, r.grid, dim3(r.block), 0, s, (const uint16_t*)g, g_cstride, (const uint16_t*)y,
                       y_cstride, (int)r.Mg, r.cgs, coef, mask_scale, mask_shift, (uint16_t*)dy, dy_cstride,
                       bias_partial);
  };
  switch (r.kernel) {
    case BnKernel::ApplyG: launch(bn_bwd_apply_g_kernel<false>); break;
    case BnKernel::ApplyGMask: launch(bn_bwd_apply_g_kernel<true>); break;
    default: return STF_EINVAL;
  }
  STF_CHECK_LAUNCH();
  if (bias_partial && dbias) {
    const int S = stf::colsum_stage1(bias_partial, r.rows * groups, C, s, 1, stf::FOLD16_ROWS);
    hipLaunchKernelGGL(stf_tile_sum_kernel, dim3((C + 15) / 16), dim3(stf::FOLD_NT), 0, s, bias_partial, S, C, dbias);
    STF_CHECK_LAUNCH();
  }
  return 0;
}

// The STF stem's BatchNorm + ReLU inside its MaxPool(3,2,1) (src/stf_lstm_unet.py:178-180)
extern "C" int stf_bn_act_maxpool3s2(const void* y, int N, int H, int W, int C, int groups, const float* scale,
                                     const float* shift, void* out, void* argmax, stf_stream_t stream) {
  const BnRoute r = bn_route({BnOp::ActPool3, N, H, W, C, groups});
  if (r.refused || !y || !scale || !shift || !out) return STF_EINVAL;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(bn_act_maxpool3_kernel, r.grid, dim3(r.block), 0, (hipStream_t)stream, (const uint16_t*)y, N, H,
                     W, C, Ho, Wo, N / groups, scale, shift, (uint16_t*)out, (uint8_t*)argmax);
  STF_CHECK_LAUNCH();
  return 0;
}

// BatchNorm backward of the STF stem through that max pool: the incoming gradient is the pooled
// output's (dout [N][Ho][Wo][C]) routed by the forward's argmax (stf_bn_act_maxpool3s2 /
// stf_maxpool3s2_fwd), never materialized at full size.  Partials as stf_bn_bwd_reduce (rule 6).
extern "C" int stf_bn_bwd_reduce_pool3(const void* argmax, const void* dout, const void* y, int N, int H, int W,
                                       int C, int groups, const float* scale, const float* shift,
                                       const float* mean, const float* invstd, float* partial,
                                       stf_stream_t stream) {
  const BnRoute r = bn_route({BnOp::ReducePool3, N, H, W, C, groups});
  if (r.refused || !argmax || !dout || !y || !partial) return STF_EINVAL;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(bn_bwd_pool3_kernel<false>, r.grid, dim3(r.block), 0, (hipStream_t)stream,
                     (const uint8_t*)argmax, (const uint16_t*)dout, (const uint16_t*)y, H, W, Ho, Wo, N / groups,
                     r.cgs, scale, shift, mean, invstd, (const float*)nullptr, (uint16_t*)nullptr, partial);
  STF_CHECK_LAUNCH();
  return 0;
}

// dy = A g' + B y + C (coef from stf_bn_bwd_finalize), g' = the routed gradient masked by the ReLU.
extern "C" int stf_bn_bwd_apply_pool3(const void* argmax, const void* dout, const void* y, int N, int H, int W,
                                      int C, int groups, const float* scale, const float* shift, const float* coef,
                                      void* dy, stf_stream_t stream) {
  const BnRoute r = bn_route({BnOp::ApplyPool3, N, H, W, C, groups});
  if (r.refused || !argmax || !dout || !y || !coef || !dy) return STF_EINVAL;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  hipLaunchKernelGGL(bn_bwd_pool3_kernel<true>, r.grid, dim3(r.block), 0, (hipStream_t)stream, (const uint8_t*)argmax,
                     (const uint16_t*)dout, (const uint16_t*)y, H, W, Ho, Wo, N / groups, r.cgs, scale, shift,
                     (const float*)nullptr, (const float*)nullptr, coef, (uint16_t*)dy, (float*)nullptr);
  STF_CHECK_LAUNCH();
  return 0;
}
