// Implicit-GEMM convolution on MFMA (gfx950), the linear kernels: forward / dgrad /
// transposed-conv of any geometry, one GEMM row per destination pixel.
//
// GEMM view: D[n][m] = sum_k W[n][k] * X[m][k]
//   m = destination pixel (N*Hd*Wd rows), n = output channel, k = (r, s, c) over
//   the gathered source tensor (stf_conv_geom in include/stfunet.h).
// The weight tile is the MFMA A operand and the im2col tile the B operand, so
// each lane ends with 4 consecutive *channels* of one pixel: the epilogue packs
// them into one 8-byte store (NHWC), adds bias, and reduces per-channel BatchNorm
// partial sums (sum, sum^2 of the bf16-rounded values) without another pass.
//
// Tiling: 256 threads = 4 waves, BK = 32 (= one v_mfma_f32_16x16x32_bf16 K),
// register-staged global->LDS double buffer, one barrier per K step.  LDS rows
// are 64 B; the 16-B chunk of row r is stored at chunk ^ ((-(r>>2)) & 3), which
// makes the ds_read_b128 fragment reads conflict-free for all four lane groups.
#include "igemm_common.h"

namespace {
using namespace stf::ig;

// Shared epilogue: acc[i][j][r] = pixel mrow[i] (this lane's GEMM row of
// fragment i, -1 = outside the image / tile), channel n0 + wn*WTN + j*16 +
// (lane>>4)*4 + r.  `tile` indexes the BatchNorm partial-statistics row.
template <int BM, int BN, int WM, int WN, bool SCATTER, int EPI, int NTH>
STF_DEV void igemm_epilogue(const Geo& a, f32x4 (&acc)[BM / WM / 16][BN / WN / 16], const int (&mrow)[BM / WM / 16],
                            int n0, int wm, int wn, int tid, char* smem, int tile) {
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  const int lane = tid & 63, fr = lane & 15, fk = lane >> 4;
  const int Cout = SCATTER ? a.Nout / 4 : a.Nout;
  float s1[TN][4], s2[TN][4];
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nb = n0 + wn * WTN + j * 16 + fk * 4;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias && nb < a.Nout) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] = a.bias[SCATTER ? (nb + r) % Cout : nb + r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { s1[j][r] = 0.f; s2[j][r] = 0.f; }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = mrow[i];
      if (!(m >= 0 && nb < a.Nout)) continue;
      if (EPI == 1) {
        // LSTM cell (torch gate order i, f, g, o): c = f*c_prev + i*g, h = o*tanh(c)
        const int ch = nb >> 2, Ch = a.Nout >> 2;
        const float cp = a.c_prev ? a.c_prev[(size_t)m * Ch + ch] : 0.f;
        float gi, gf, gg, go, c, hh;
        lstm_cell_fwd(acc[i][j][0] + bv[0], acc[i][j][1] + bv[1], acc[i][j][2] + bv[2], acc[i][j][3] + bv[3], cp,
                      gi, gf, gg, go, c, hh);
        a.c_out[(size_t)m * Ch + ch] = c;
        reinterpret_cast<e16*>(a.h_out)[(size_t)m * a.hcs + ch] = f2e(hh);
        if (a.gates) *reinterpret_cast<float4*>(a.gates + (size_t)m * a.Nout + nb) = make_float4(gi, gf, gg, go);
        continue;
      }
      if (EPI == 2) {
        // LSTM cell backward on the recomputed gates (the forward's arithmetic, same GEMM):
        // dc = dh*o*(1-tanh(c)^2) + dc_next, dc_prev = dc*f, pre-activation gate gradients
        const int ch = nb >> 2, Ch = a.Nout >> 2;
        const size_t u = (size_t)m * Ch + ch;
        float gi, gf, gg, go, cx, hx;
        lstm_cell_fwd(acc[i][j][0] + bv[0], acc[i][j][1] + bv[1], acc[i][j][2] + bv[2], acc[i][j][3] + bv[3], 0.f,
                      gi, gf, gg, go, cx, hx);
        const float h = e2f(reinterpret_cast<const e16*>(a.l_dh)[(size_t)m * a.l_dhcs + ch]);
        const float cp = a.c_prev ? a.c_prev[u] : 0.f;
        float d_i, d_f, d_g, d_o, dcp;
        lstm_cell_bwd(gi, gf, gg, go, a.c_out[u], cp, h, a.l_dcn ? a.l_dcn[u] : 0.f, d_i, d_f, d_g, d_o, dcp);
        a.l_dcp[u] = dcp;
        *reinterpret_cast<uint2*>(a.l_dg + (size_t)m * a.Nout + nb) = make_uint2(pack2(d_i, d_f), pack2(d_g, d_o));
        continue;
      }
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = acc[i][j][r] + bv[r];
      size_t off;
      if (SCATTER) {
        const int blk = nb / Cout, co = nb - blk * Cout;
        const int hw = a.Hd * a.Wd;
        const int n = m / hw, rem = m - n * hw;
        const int yd = rem / a.Wd, xd = rem - yd * a.Wd;
        const int yo = 2 * yd + (blk >> 1), xo = 2 * xd + (blk & 1);
        off = ((size_t)(n * 2 * a.Hd + yo) * (2 * a.Wd) + xo) * a.dcs + co;
      } else {
        off = (size_t)m * a.dcs + nb;
      }
      if (a.accumulate) {
        const uint2 old = *reinterpret_cast<const uint2*>(a.dst + off);
        v[0] += lo16(old.x);
        v[1] += hi16(old.x);
        v[2] += lo16(old.y);
        v[3] += hi16(old.y);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = round_e(v[r]);
      *reinterpret_cast<uint2*>(a.dst + off) = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
#pragma unroll
      for (int r = 0; r < 4; ++r) { s1[j][r] += v[r]; s2[j][r] += v[r] * v[r]; }
    }
  }
  if (EPI != 0 || a.stats == nullptr) return;
  // reduce over the 16 pixels held by lanes with equal fk, then over the WM waves
#pragma unroll
  for (int j = 0; j < TN; ++j)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        s1[j][r] += __shfl_xor(s1[j][r], o, 64);
        s2[j][r] += __shfl_xor(s2[j][r], o, 64);
      }
  float* red = reinterpret_cast<float*>(smem);     // [WM][2][BN]
  __syncthreads();
  if (fr == 0) {
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int col = wn * WTN + j * 16 + fk * 4 + r;
        red[(wm * 2 + 0) * BN + col] = s1[j][r];
        red[(wm * 2 + 1) * BN + col] = s2[j][r];
      }
  }
  __syncthreads();
  for (int col = tid; col < BN; col += NTH) {
    const int n = n0 + col;
    if (n >= a.Nout) continue;
    float t1 = 0.f, t2 = 0.f;
#pragma unroll
    for (int w = 0; w < WM; ++w) { t1 += red[(w * 2) * BN + col]; t2 += red[(w * 2 + 1) * BN + col]; }
    a.stats[(size_t)tile * 2 * a.Nout + n] = t1;
    a.stats[(size_t)tile * 2 * a.Nout + a.Nout + n] = t2;
  }
}


// LDS-staged epilogue of the linear DMA kernels (EPI 0): the BM x BN tile goes to
// LDS as bf16(acc + bias) (16-B chunk c of row r at c ^ (r & 7)), then every
// thread stores whole 16-B chunks of output rows (one fixed 8-channel chunk per
// thread: full 128-B+ row segments per wave instead of 8-B pieces of 16 rows),
// adds the old value when accumulating, and sums BN statistics of the stored
// values.  Needs BM*BN*2 + NW*2*BN*4 bytes of LDS (the drained ring).
template <int BM, int BN, int WM, int WN, bool SCATTER, int NTH>
STF_DEV void staged_epilogue(const Geo& a, f32x4 (&acc)[BM / WM / 16][BN / WN / 16], int m0, int m_end, int n0,
                             int wm, int wn, int tid, char* smem, int tile, int pcls = -1) {
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int CPR = BN / 8, RPP = NTH / CPR, PASSES = BM / RPP, NW = WM * WN;
  static_assert(NTH % CPR == 0 && BM % RPP == 0, "epilogue mapping");
  const int lane = tid & 63, fr = lane & 15, fk = lane >> 4, wave = tid >> 6;
  const int Cout = SCATTER ? a.Nout / 4 : a.Nout;
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nl = wn * WTN + j * 16 + fk * 4;           // tile column of this lane's 4 channels
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias && n0 + nl < a.Nout) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] = a.bias[SCATTER ? (n0 + nl + r) % Cout : n0 + nl + r];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * WTM + i * 16 + fr;
      const uint2 v = make_uint2(pack2(acc[i][j][0] + bv[0], acc[i][j][1] + bv[1]),
                                 pack2(acc[i][j][2] + bv[2], acc[i][j][3] + bv[3]));
      *reinterpret_cast<uint2*>(smem + row * (BN * 2) + (((nl >> 3) ^ (row & 7)) << 4) + (nl & 7) * 2) = v;
    }
  }
  __syncthreads();
  const int c = tid % CPR, n = n0 + c * 8;
  const bool nok = n < a.Nout;
  const bool want = a.stats != nullptr;                 // uniform: no unpack / sums without statistics
  float s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  // ConvT 2x2 scatter: the thread's pixel advances RPP rows a pass; its column x on the small
  // grid and its output offset are carried with adds (+2 dcs per pixel, +2 Wd dcs more per
  // small-grid row; image rows follow each other, so an image boundary needs nothing extra)
  // instead of per-pass divisions, which made the small-K launches VALU-bound (up128 2.9 TB/s)
  int sc_x = 0;
  size_t sc_off = 0;
  if (SCATTER) {
    const int blk = n / Cout, co = n - blk * Cout;
    const int m = m0 + tid / CPR, gy = m / a.Wd;      // global small-grid row (img * Hd + y)
    sc_x = m - gy * a.Wd;
    sc_off = ((size_t)(2 * gy + (blk >> 1)) * (2 * a.Wd) + 2 * sc_x + (blk & 1)) * a.dcs + co;
  }
#pragma unroll 4
  for (int ps = 0; ps < PASSES; ++ps) {
    const int row = tid / CPR + ps * RPP;
    const int m = m0 + row;
    if (nok && m < m_end) {
      uint4 u = *reinterpret_cast<const uint4*>(smem + row * (BN * 2) + ((c ^ (row & 7)) << 4));
      size_t off;
      if (SCATTER) {
        off = sc_off;
      } else if (pcls >= 0) {                        // parity-class row -> output pixel
        const int py = pcls >> 1, px = pcls & 1;
        const int Hc = (a.Hd - py + 1) >> 1, Wc = (a.Wd - px + 1) >> 1;
        const int img = m / (Hc * Wc), rem = m - img * (Hc * Wc), uu = rem / Wc, v = rem - uu * Wc;
        off = ((size_t)(img * a.Hd + 2 * uu + py) * a.Wd + 2 * v + px) * a.dcs + n;
      } else {
        off = (size_t)m * a.dcs + n;
      }
      if (a.accumulate || want) {
        float f[8];
        unpack8(u, f);
        if (a.accumulate) {
          float o[8];
          unpack8(*reinterpret_cast<const uint4*>(a.dst + off), o);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = round_e(f[e] + o[e]);
          u = pack8(f);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) { s1[e] += f[e]; s2[e] += f[e] * f[e]; }
      }
      *reinterpret_cast<uint4*>(a.dst + off) = u;
    }
    if (SCATTER) {
      sc_x += RPP;
      sc_off += (size_t)(2 * RPP) * a.dcs;
      while (sc_x >= a.Wd) {
        sc_x -= a.Wd;
        sc_off += (size_t)(2 * a.Wd) * a.dcs;
      }
    }
  }
  if (a.stats == nullptr) return;
  // threads with equal c: fold within the wave (lanes c, c+CPR, ...), then over waves
#pragma unroll
  for (int e = 0; e < 8; ++e)
#pragma unroll
    for (int o = CPR; o < 64; o <<= 1) {
      s1[e] += __shfl_xor(s1[e], o, 64);
      s2[e] += __shfl_xor(s2[e], o, 64);
    }
  float* red = reinterpret_cast<float*>(smem + BM * BN * 2);   // [NW][2][BN]
  constexpr int CW = CPR < 64 ? CPR : 64;                       // distinct chunks per wave
  if (lane < CW) {
    const int cc = (wave * 64 + lane) % CPR;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(wave * 2 + 0) * BN + cc * 8 + e] = s1[e];
      red[(wave * 2 + 1) * BN + cc * 8 + e] = s2[e];
    }
  }
  __syncthreads();
  // chunk cc appears in the waves whose 64 lanes cover it
  for (int col = tid; col < 2 * BN; col += NTH) {
    const int q = col / BN, cl = col - q * BN, cc = cl >> 3;
    if (n0 + cl >= a.Nout) continue;
    float t = 0.f;
    for (int w = 0; w < NW; ++w) {
      const int first = (w * 64) % CPR;                         // chunks held by wave w: first .. first+CW-1 (mod CPR)
      if (((cc - first + CPR) % CPR) < CW) t += red[(w * 2 + q) * BN + cl];
    }
    a.stats[(size_t)tile * 2 * a.Nout + q * a.Nout + n0 + cl] = t;
  }
}

// LSTM cell epilogue of the DMA kernels, staged through LDS: the block's c_prev tile
// [BM pixels][BN/4 hidden channels] fp32 comes in as whole 16-B chunks of rows, the
// cell (gate order i, f, g, o: c = f c_prev + i g, h = o tanh c) runs on the MFMA
// layout (each lane holds the four gates of one hidden channel of one pixel), c and h go
// back to LDS and leave as whole row chunks (c: BN B per pixel row, h: BN/2 B) instead
// of one 4-B / 2-B store per lane for 16 scattered pixels.  The gates for the backward
// keep their direct float4 stores (64 contiguous B per pixel per instruction).
template <int BM, int BN, int WM, int WN, int NTH>
STF_DEV void lstm_staged_epilogue(const Geo& a, f32x4 (&acc)[BM / WM / 16][BN / WN / 16], int m0, int m_end,
                                  int n0, int wm, int wn, int tid, char* smem) {
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int HC = BN / 4;                            // hidden channels per tile
  constexpr int PS = HC + 4;                            // fp32 row stride (16-B aligned, skewed)
  constexpr int CCH = HC / 4, HCH = HC / 8;             // 16-B chunks per c row / h row
  float* cs = reinterpret_cast<float*>(smem);           // [BM][PS] c_prev, then c
  e16* hs = reinterpret_cast<e16*>(smem + BM * PS * 4);   // [BM][HC + 8] h
  constexpr int HS = HC + 8;
  const int lane = tid & 63, fr = lane & 15, fk = lane >> 4;
  const int Ch = a.Nout >> 2, ch0 = n0 >> 2;
  const int hcn = min(HC, Ch - ch0);                    // hidden channels present in this tile
  // whole 16-B chunks need Ch % 4 (row alignment) and a chunk inside the tile's channels;
  // a tail chunk (hcn % 4, hcn % 8 for h) moves element by element
  const bool cvec = (Ch & 3) == 0;
  for (int e = tid; e < BM * CCH; e += NTH) {
    const int r = e / CCH, q = e - r * CCH, m = m0 + r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.c_prev && m < m_end && q * 4 < hcn) {
      const float* src = a.c_prev + (size_t)m * Ch + ch0 + q * 4;
      if (cvec && q * 4 + 4 <= hcn) v = *reinterpret_cast<const float4*>(src);
      else {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < 4 && q * 4 + k < hcn; ++k) t[k] = src[k];
        v = make_float4(t[0], t[1], t[2], t[3]);
      }
    }
    *reinterpret_cast<float4*>(cs + r * PS + q * 4) = v;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nl = wn * WTN + j * 16 + fk * 4, nb = n0 + nl, hl = nl >> 2;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias && nb < a.Nout) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] = a.bias[nb + r];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * WTM + i * 16 + fr, m = m0 + row;
      if (!(m < m_end && nb < a.Nout)) continue;
      float gi, gf, gg, go, c, hh;
      lstm_cell_fwd(acc[i][j][0] + bv[0], acc[i][j][1] + bv[1], acc[i][j][2] + bv[2], acc[i][j][3] + bv[3],
                    cs[row * PS + hl], gi, gf, gg, go, c, hh);
      cs[row * PS + hl] = c;
      hs[row * HS + hl] = f2e(hh);
      if (a.gates) *reinterpret_cast<float4*>(a.gates + (size_t)m * a.Nout + nb) = make_float4(gi, gf, gg, go);
    }
  }
  __syncthreads();
  for (int e = tid; e < BM * CCH; e += NTH) {
    const int r = e / CCH, q = e - r * CCH, m = m0 + r;
    if (!(m < m_end && q * 4 < hcn)) continue;
    float* dst = a.c_out + (size_t)m * Ch + ch0 + q * 4;
    if (cvec && q * 4 + 4 <= hcn) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(cs + r * PS + q * 4);
    else
      for (int k = 0; k < 4 && q * 4 + k < hcn; ++k) dst[k] = cs[r * PS + q * 4 + k];
  }
  const bool hvec = ((reinterpret_cast<uintptr_t>(a.h_out) & 15) == 0) && (a.hcs & 7) == 0;
  for (int e = tid; e < BM * HCH; e += NTH) {
    const int r = e / HCH, q = e - r * HCH, m = m0 + r;
    if (!(m < m_end && q * 8 < hcn)) continue;
    uint16_t* dst = a.h_out + (size_t)m * a.hcs + ch0 + q * 8;
    const e16* src = hs + r * HS + q * 8;
    if (hvec && q * 8 + 8 <= hcn) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    else
      for (int k = 0; k < 8 && q * 8 + k < hcn; ++k) reinterpret_cast<e16*>(dst)[k] = src[k];
  }
}

// LSTM cell-backward epilogue (EPI 2), staged through LDS like the forward's: the
// block's c_t, c_{t-1}, dc_next (fp32) and dh (bf16) tiles come in as whole 16-B row
// chunks, the cell backward runs on the MFMA layout (a lane holds the four recomputed
// gate pre-activations of one hidden channel of one pixel), dc_prev goes back to LDS
// (over dc_next) and leaves as row chunks; the four bf16 gate gradients of a lane are
// one 8-B store (32 contiguous bytes per pixel per wave-instruction).
template <int BM, int BN>
constexpr int lstm_bwd_lds() { return 3 * BM * (BN / 4 + 4) * 4 + BM * (BN / 4 + 8) * 2; }

template <int BM, int BN, int WM, int WN, int NTH>
STF_DEV void lstm_bwd_staged_epilogue(const Geo& a, f32x4 (&acc)[BM / WM / 16][BN / WN / 16], int m0, int m_end,
                                      int n0, int wm, int wn, int tid, char* smem) {
  constexpr int WTM = BM / WM, WTN = BN / WN, TM = WTM / 16, TN = WTN / 16;
  constexpr int HC = BN / 4, PS = HC + 4, HS = HC + 8, CCH = HC / 4, HCH = HC / 8;
  float* cts = reinterpret_cast<float*>(smem);           // [BM][PS] c_t
  float* cps = cts + BM * PS;                            // [BM][PS] c_{t-1}
  float* dcs = cps + BM * PS;                            // [BM][PS] dc_next, then dc_prev
  e16* dhs = reinterpret_cast<e16*>(dcs + BM * PS);    // [BM][HS] dh
  const int lane = tid & 63, fr = lane & 15, fk = lane >> 4;
  const int Ch = a.Nout >> 2, ch0 = n0 >> 2;
  const int hcn = min(HC, Ch - ch0);
  const bool cvec = (Ch & 3) == 0;
  auto ld4 = [&](const float* base, int m, int q) {
    if (!base || m >= m_end || q * 4 >= hcn) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float* src = base + (size_t)m * Ch + ch0 + q * 4;
    if (cvec && q * 4 + 4 <= hcn) return *reinterpret_cast<const float4*>(src);
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < 4 && q * 4 + k < hcn; ++k) t[k] = src[k];
    return make_float4(t[0], t[1], t[2], t[3]);
  };
  for (int e = tid; e < BM * CCH; e += NTH) {
    const int r = e / CCH, q = e - r * CCH, m = m0 + r;
    *reinterpret_cast<float4*>(cts + r * PS + q * 4) = ld4(a.c_out, m, q);
    *reinterpret_cast<float4*>(cps + r * PS + q * 4) = ld4(a.c_prev, m, q);
    *reinterpret_cast<float4*>(dcs + r * PS + q * 4) = ld4(a.l_dcn, m, q);
  }
  const bool hvec = ((reinterpret_cast<uintptr_t>(a.l_dh) & 15) == 0) && (a.l_dhcs & 7) == 0;
  for (int e = tid; e < BM * HCH; e += NTH) {
    const int r = e / HCH, q = e - r * HCH, m = m0 + r;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (m < m_end && q * 8 < hcn) {
      const uint16_t* src = a.l_dh + (size_t)m * a.l_dhcs + ch0 + q * 8;
      if (hvec && q * 8 + 8 <= hcn) v = *reinterpret_cast<const uint4*>(src);
      else {
        uint16_t t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; k < 8 && q * 8 + k < hcn; ++k) t[k] = src[k];
        v = make_uint4(t[0] | ((uint32_t)t[1] << 16), t[2] | ((uint32_t)t[3] << 16), t[4] | ((uint32_t)t[5] << 16),
                       t[6] | ((uint32_t)t[7] << 16));
      }
    }
    *reinterpret_cast<uint4*>(dhs + r * HS + q * 8) = v;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int nl = wn * WTN + j * 16 + fk * 4, nb = n0 + nl, hl = nl >> 2;
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (a.bias && nb < a.Nout) {
#pragma unroll
      for (int r = 0; r < 4; ++r) bv[r] = a.bias[nb + r];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * WTM + i * 16 + fr, m = m0 + row;
      if (!(m < m_end && nb < a.Nout)) continue;
      float gi, gf, gg, go, cx, hx;
      lstm_cell_fwd(acc[i][j][0] + bv[0], acc[i][j][1] + bv[1], acc[i][j][2] + bv[2], acc[i][j][3] + bv[3], 0.f,
                    gi, gf, gg, go, cx, hx);
      float d_i, d_f, d_g, d_o, dcp;
      lstm_cell_bwd(gi, gf, gg, go, cts[row * PS + hl], cps[row * PS + hl], e2f(dhs[row * HS + hl]),
                    dcs[row * PS + hl], d_i, d_f, d_g, d_o, dcp);
      dcs[row * PS + hl] = dcp;
      *reinterpret_cast<uint2*>(a.l_dg + (size_t)m * a.Nout + nb) = make_uint2(pack2(d_i, d_f), pack2(d_g, d_o));
    }
  }
  __syncthreads();
  for (int e = tid; e < BM * CCH; e += NTH) {
    const int r = e / CCH, q = e - r * CCH, m = m0 + r;
    if (!(m < m_end && q * 4 < hcn)) continue;
    float* dst = a.l_dcp + (size_t)m * Ch + ch0 + q * 4;
    if (cvec && q * 4 + 4 <= hcn) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(dcs + r * PS + q * 4);
    else
      for (int k = 0; k < 4 && q * 4 + k < hcn; ++k) dst[k] = dcs[r * PS + q * 4 + k];
  }
}

template <int BM, int BN, int WM, int WN, bool SMALLC, bool TRANS, bool SCATTER, int EPI>
__global__ __launch_bounds__(NT, 2) void igemm_kernel(Geo a) {
  constexpr int WTM = BM / WM, WTN = BN / WN;     // wave tile (pixels x channels)
  constexpr int TM = WTM / 16, TN = WTN / 16;     // 16x16 fragments per wave
  constexpr int CHA = BM * BK / 8 / NT;           // 16-B chunks per thread (im2col)
  constexpr int CHB = BN * BK / 8 / NT;           // 16-B chunks per thread (weights)
  static_assert(WM * WN == 4, "4 waves");
  static_assert(CHA >= 1 && CHB >= 1, "tile too small");
  constexpr int LDS_A = BM * BK * 2, LDS_B = BN * BK * 2;
  constexpr int LDS_MAIN = 2 * (LDS_A + LDS_B), LDS_RED = WM * 2 * BN * 4;
  __shared__ __attribute__((aligned(16))) char smem[LDS_MAIN > LDS_RED ? LDS_MAIN : LDS_RED];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  // M tiles never straddle a statistics group: block x = (group, tile within group)
  const int grp = blockIdx.x / a.tpg, gtile = blockIdx.x - grp * a.tpg;
  const int m0 = grp * a.Mg + gtile * BM, n0 = blockIdx.y * BN;
  const int m_end = min(m0 + BM, min((grp + 1) * a.Mg, a.M));
  const int kc = tid & 3;                 // this thread's 16-B chunk within a 64-B row

  // per-row gather state for the im2col rows this thread stages
  int rbase[CHA], ry[CHA], rx[CHA];
  bool rok[CHA];
#pragma unroll
  for (int i = 0; i < CHA; ++i) {
    const int m = m0 + (tid >> 2) + i * (NT / 4);
    rok[i] = m < m_end;
    const int mm = rok[i] ? m : 0;
    const int hw = a.Hd * a.Wd;
    const int n = mm / hw, rem = mm - n * hw;
    const int yd = rem / a.Wd, xd = rem - yd * a.Wd;
    rbase[i] = n * a.Hs * a.Ws;
    if (TRANS) { ry[i] = yd + a.pad; rx[i] = xd + a.pad; }
    else { ry[i] = yd * a.st - a.pad; rx[i] = xd * a.st - a.pad; }
  }

  uint4 ra[CHA], rb[CHB];
  int tr = 0, ts = 0, tc = 0;             // tap / channel cursor of the next K step (non-SMALLC)
  const int KT = (a.K + BK - 1) / BK;

  auto gather_src = [&](int i, int r, int s, int c, uint4& out) {
    int ys, xs; bool ok = rok[i];
    if (TRANS) {
      const int ty = ry[i] - r, tx = rx[i] - s;
      if (a.st == 2) { ok = ok && !(ty & 1) && !(tx & 1); ys = ty >> 1; xs = tx >> 1; }
      else { ys = ty; xs = tx; }
      ok = ok && ty >= 0 && tx >= 0;
    } else { ys = ry[i] + r; xs = rx[i] + s; ok = ok && ys >= 0 && xs >= 0; }
    ok = ok && ys < a.Hs && xs < a.Ws;
    out = make_uint4(0, 0, 0, 0);
    if (ok) out = *reinterpret_cast<const uint4*>(a.src + (size_t)(rbase[i] + ys * a.Ws + xs) * a.scs + c);
  };

  auto load_tiles = [&](int kt) {
    const int k0 = kt * BK;
    if (SMALLC) {
      const int k = k0 + kc * 8;
      const bool kok = k < a.K;
      const int tap = kok ? k / a.Cs : 0;
      const int c = k - tap * a.Cs;
      const int r = tap / a.S, s = tap - r * a.S;
#pragma unroll
      for (int i = 0; i < CHA; ++i) {
        if (kok) gather_src(i, r, s, c, ra[i]); else ra[i] = make_uint4(0, 0, 0, 0);
      }
    } else {
#pragma unroll
      for (int i = 0; i < CHA; ++i) gather_src(i, tr, ts, tc + kc * 8, ra[i]);
      tc += BK;
      if (tc == a.Cs) { tc = 0; if (++ts == a.S) { ts = 0; ++tr; } }
    }
#pragma unroll
    for (int i = 0; i < CHB; ++i) {
      const int n = n0 + (tid >> 2) + i * (NT / 4);
      const int k = k0 + kc * 8;
      rb[i] = make_uint4(0, 0, 0, 0);
      if (n < a.Nout && k < a.K) rb[i] = *reinterpret_cast<const uint4*>(a.wgt + (size_t)n * a.K + k);
    }
  };

  auto store_tiles = [&](int buf) {
    char* sa = smem + buf * (LDS_A + LDS_B);
    char* sb = sa + LDS_A;
#pragma unroll
    for (int i = 0; i < CHA; ++i) {
      const int row = (tid >> 2) + i * (NT / 4);
      *reinterpret_cast<uint4*>(sa + row * 64 + swz(row, kc) * 16) = ra[i];
    }
#pragma unroll
    for (int i = 0; i < CHB; ++i) {
      const int row = (tid >> 2) + i * (NT / 4);
      *reinterpret_cast<uint4*>(sb + row * 64 + swz(row, kc) * 16) = rb[i];
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_tiles(0);
  store_tiles(0);
  __syncthreads();

  const int fr = lane & 15, fk = lane >> 4;
  for (int kt = 0; kt < KT; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < KT) load_tiles(kt + 1);
    const char* sa = smem + cur * (LDS_A + LDS_B);
    const char* sb = sa + LDS_A;
    e16x8 xf[TM], wf[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * WTM + i * 16 + fr;
      xf[i] = *reinterpret_cast<const e16x8*>(sa + row * 64 + swz(row, fk) * 16);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int row = wn * WTN + j * 16 + fr;
      wf[j] = *reinterpret_cast<const e16x8*>(sb + row * 64 + swz(row, fk) * 16);
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
        acc[i][j] = mfma16x16x32(wf[j], xf[i], acc[i][j]);
    if (kt + 1 < KT) store_tiles(cur ^ 1);
    __syncthreads();
  }

  int mrow[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + wm * WTM + i * 16 + (lane & 15);
    mrow[i] = m < m_end ? m : -1;
  }
  igemm_epilogue<BM, BN, WM, WN, SCATTER, EPI, NT>(a, acc, mrow, n0, wm, wn, tid, smem, blockIdx.x);
}

// ---------------------------------------------------------------------------
// LDS-DMA ring variant (Cs % BKK == 0): every 16-B chunk goes global -> LDS with
// buffer_load_dwordx4 ... lds (no VGPR staging, no ds_write).  The im2col halo
// and all tails are zero-filled by the buffer range check: an invalid lane gets
// voffset 0xFFFFFFF0 >= num_records.  One wave-instruction writes 1 KiB of rows
// linearly, so the chunk swizzle is applied on the SOURCE side (lane with LDS
// chunk slot p loads global chunk swz(row, p)); the fragment reads use the same
// involution.  STAGES-deep ring, STAGES-1 K steps in flight across the raw
// s_barrier; a counted vmcnt retires exactly the stage about to be read.
//   BKK = 32: 64-B rows, chunk ^ ((-(row>>2)) & 3)
//   BKK = 64: 128-B rows, chunk ^ ((row>>1) & 7)   (two MFMA k-halves per step)
// Both make each ds_read_b128 lane group (4 x 16 lanes) hit 16 distinct 16-B
// slots of the 256-B bank row.  Blocks are remapped so that consecutive tiles
// (shared halo rows) and all channel tiles of one pixel tile run on one XCD.
template <int BKK>
STF_DEV int swzk(int row, int kc) {
  if constexpr (BKK == 32) return kc ^ ((-(row >> 2)) & 3);
  else return kc ^ ((row >> 1) & 7);
}

// C8: 8-channel sources (network inputs): a 16-B chunk is one whole tap, so
// every lane gathers its own tap (k-step = 4 taps at BKK 32); K need not be a
// multiple of BKK (k >= K masked)
template <int BM, int BN, int WM, int WN, int BKK, int STAGES, bool TRANS, bool SCATTER, int EPI, bool C8 = false>
__global__ __launch_bounds__(64 * WM * WN, (WM * WN == 4 || (BM == 128 && BN == 256)) ? 2 : 1) void igemm_dma_kernel(
    Geo a, uint32_t src_bytes) {
  constexpr int NW = WM * WN, NTH = 64 * NW;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  constexpr int ROWB = BKK * 2;                         // bytes per LDS row
  constexpr int CPR = BKK / 8;                          // 16-B chunks per row
  constexpr int RPI = 64 / CPR;                         // rows per DMA wave-instruction (1 KiB)
  constexpr int LA = BM / NW / RPI, LB = BN / NW / RPI; // DMA instructions per wave per K step
  constexpr int STAGE = (BM + BN) * ROWB;
  constexpr int LDS_MAIN = STAGES * STAGE;
  constexpr int LDS_RED = EPI == 0 ? BM * BN * 2 + NW * 2 * BN * 4 : (EPI == 2 ? lstm_bwd_lds<BM, BN>() : WM * 2 * BN * 4);
  static_assert(LA >= 1 && LB >= 1 && LA * RPI * NW == BM && LB * RPI * NW == BN, "tile");
  __shared__ __attribute__((aligned(16))) char smem[LDS_MAIN > LDS_RED ? LDS_MAIN : LDS_RED];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  // XCD-aware bijective remap of the linear block id (8 XCDs, round-robin dispatch)
  const int gx = gridDim.x, gy = gridDim.y, nwg = gx * gy;
  const int orig = blockIdx.y * gx + blockIdx.x;
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int bx = wid / gy, by = wid - bx * gy;
  const int grp = bx / a.tpg, gtile = bx - grp * a.tpg;
  int m0 = grp * a.Mg + gtile * BM, m_end = min(m0 + BM, min((grp + 1) * a.Mg, a.M));
  const int n0 = by * BN;
  const int sub = lane / CPR, slot = lane % CPR;
  // Parity mode (stride-2 transposed gather): output pixel (y, x) only receives the taps
  // r = y + pad (mod 2), s = x + pad (mod 2).  Rows are ordered by class (y & 1, x & 1),
  // each block lies in one class and walks only that class's taps (1/2/2/4 of the nine
  // for 3x3, none for the odd classes of 1x1) instead of masking 3/4 of the MFMAs to zero.
  // par == 2 (an accumulating launch): classes without taps (the odd ones of a 1x1 / stride-2
  // transposed gather) add nothing -- they get no blocks at all (stf_igemm counts the same way)
  int pcls = -1, py = 0, px = 0, Hc = 0, Wc = 0, r0 = 0, s0 = 0;
  if (TRANS && a.par) {
    int b = gtile;
#pragma unroll
    for (int ci = 0; ci < 4; ++ci) {
      const int c = 3 - ci;                         // (1,1) first: 4 taps, then 2, 2, 1 (shorter tail)
      const int hc = (a.Hd - (c >> 1) + 1) >> 1, wc = (a.Wd - (c & 1) + 1) >> 1;
      const int mc = a.N * hc * wc, nb = (mc + BM - 1) / BM;
      const int ntap = ((a.R - (((c >> 1) + a.pad) & 1) + 1) >> 1) * ((a.S - (((c & 1) + a.pad) & 1) + 1) >> 1);
      if (a.par == 2 && ntap == 0) continue;
      if (pcls < 0) {
        if (b < nb) { pcls = c; Hc = hc; Wc = wc; m0 = b * BM; m_end = min(m0 + BM, mc); }
        else b -= nb;
      }
    }
    py = pcls >> 1; px = pcls & 1;
    r0 = (py + a.pad) & 1; s0 = (px + a.pad) & 1;
  }

  const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc((void*)a.src, 0, src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_wgt =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.wgt, 0, (uint32_t)a.Nout * a.K * 2, 0x00020000);

  int rbase[LA], ry[LA], rx[LA], akc[LA];
  bool rok[LA];
#pragma unroll
  for (int i = 0; i < LA; ++i) {
    const int row = wave * (BM / NW) + i * RPI + sub;
    const int m = m0 + row;
    rok[i] = m < m_end;
    const int mm = rok[i] ? m : m0;
    int n, yd, xd;
    if (TRANS && a.par) {
      n = mm / (Hc * Wc);
      const int rem = mm - n * (Hc * Wc), u = rem / Wc;
      yd = 2 * u + py; xd = 2 * (rem - u * Wc) + px;
    } else {
      const int hw = a.Hd * a.Wd;
      n = mm / hw;
      const int rem = mm - n * hw;
      yd = rem / a.Wd; xd = rem - yd * a.Wd;
    }
    rbase[i] = n * a.Hs * a.Ws;
    if (TRANS) { ry[i] = yd + a.pad; rx[i] = xd + a.pad; }
    else { ry[i] = yd * a.st - a.pad; rx[i] = xd * a.st - a.pad; }
    akc[i] = swzk<BKK>(row, slot);
  }
  int bn_[LB], bkc[LB];
#pragma unroll
  for (int i = 0; i < LB; ++i) {
    const int row = wave * (BN / NW) + i * RPI + sub;
    bn_[i] = n0 + row;
    bkc[i] = swzk<BKK>(row, slot);
  }
  constexpr uint32_t BAD = 0xFFFFFFF0u;
  const int tstep = (TRANS && a.par) ? 2 : 1;          // tap stride of the cursor
  const int KTall = C8 ? (a.K + BKK - 1) / BKK
                       : ((TRANS && a.par) ? ((a.R - r0 + 1) >> 1) * ((a.S - s0 + 1) >> 1) * (a.Cs / BKK) : a.K / BKK);
  int tr = r0, ts = s0, tc = 0;                         // tap / channel cursor of the next K step to issue
  // split-K (plain gathers only, see ksplit_of): this block's slice of the K steps
  int KT = KTall;
  if (!C8 && !TRANS && !SCATTER && EPI == 0 && a.ksplit > 1) {
    const int kb = (int)((long)KTall * blockIdx.z / a.ksplit);
    KT = (int)((long)KTall * (blockIdx.z + 1) / a.ksplit) - kb;
    const int k0 = kb * BKK, tap = k0 / a.Cs;
    tc = k0 - tap * a.Cs; tr = tap / a.S; ts = tap - tr * a.S;
  }

  auto issue = [&](int kt) {
    char* st = smem + (kt % STAGES) * STAGE;
#pragma unroll
    for (int i = 0; i < LA; ++i) {
      int ys, xs;
      bool ok = rok[i];
      if (C8) {
        const int tap = (kt * BKK) / 8 + akc[i], r = tap / a.S, s_ = tap - r * a.S;
        ys = ry[i] + r;
        xs = rx[i] + s_;
        ok = ok && tap < a.R * a.S && ys >= 0 && xs >= 0 && ys < a.Hs && xs < a.Ws;
        const uint32_t off = ok ? (uint32_t)(((rbase[i] + ys * a.Ws + xs) * a.scs) * 2) : BAD;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rs_src, (__attribute__((address_space(3))) void*)(st + (wave * (BM / NW) + i * RPI) * ROWB), 16, off, 0,
            0, 0);
        continue;
      }
      if (TRANS) {
        const int ty = ry[i] - tr, tx = rx[i] - ts;
        if (a.st == 2) { ok = ok && !(ty & 1) && !(tx & 1); ys = ty >> 1; xs = tx >> 1; }
        else { ys = ty; xs = tx; }
        ok = ok && ty >= 0 && tx >= 0;
      } else { ys = ry[i] + tr; xs = rx[i] + ts; ok = ok && ys >= 0 && xs >= 0; }
      ok = ok && ys < a.Hs && xs < a.Ws;
      const uint32_t off = ok ? (uint32_t)(((rbase[i] + ys * a.Ws + xs) * a.scs + tc + akc[i] * 8) * 2) : BAD;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs_src, (__attribute__((address_space(3))) void*)(st + (wave * (BM / NW) + i * RPI) * ROWB), 16, off, 0, 0,
          0);
    }
    const int k0 = C8 ? kt * BKK : (tr * a.S + ts) * a.Cs + tc;
#pragma unroll
    for (int i = 0; i < LB; ++i) {
      const bool ok = bn_[i] < a.Nout && (!C8 || k0 + bkc[i] * 8 < a.K);
      const uint32_t off = ok ? (uint32_t)((bn_[i] * a.K + k0 + bkc[i] * 8) * 2) : BAD;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs_wgt, (__attribute__((address_space(3))) void*)(st + BM * ROWB + (wave * (BN / NW) + i * RPI) * ROWB),
          16, off, 0, 0, 0);
    }
    tc += BKK;
    if (tc == a.Cs) { tc = 0; ts += tstep; if (ts >= a.S) { ts = s0; tr += tstep; } }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  constexpr int D = STAGES - 1;                         // K steps in flight
  constexpr int L = LA + LB;                            // DMA ops per wave per K step
  for (int s = 0; s < D && s < KT; ++s) issue(s);
  const int fr = lane & 15, fk = lane >> 4;
  for (int kt = 0; kt < KT; ++kt) {
    // retire stage kt (this wave's DMAs), then the barrier makes every wave's visible
    if (kt + D <= KT) asm volatile("s_waitcnt vmcnt(%0)" :: "n"((D - 1) * L) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // the stage read at kt-1 is free for everyone now: refill it D steps ahead
    if (kt + D < KT) issue(kt + D);
    const char* sa = smem + (kt % STAGES) * STAGE;
    const char* sb = sa + BM * ROWB;
#pragma unroll
    for (int h = 0; h < BKK / 32; ++h) {
      e16x8 xf[TM], wf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int row = wm * WTM + i * 16 + fr;
        xf[i] = *reinterpret_cast<const e16x8*>(sa + row * ROWB + swzk<BKK>(row, fk + 4 * h) * 16);
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int row = wn * WTN + j * 16 + fr;
        wf[j] = *reinterpret_cast<const e16x8*>(sb + row * ROWB + swzk<BKK>(row, fk + 4 * h) * 16);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = mfma16x16x32(wf[j], xf[i], acc[i][j]);
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if constexpr (!C8 && !TRANS && !SCATTER && EPI == 0) {
    if (a.ksplit > 1) {
      // raw fp32 partial of this K slice: lane holds 4 consecutive channels of one row
      float* wz = a.ws + (size_t)blockIdx.z * a.M * a.Nout;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int m = m0 + wm * WTM + i * 16 + fr;
        if (m >= m_end) continue;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int n = n0 + wn * WTN + j * 16 + fk * 4;
          if (n < a.Nout)
            *reinterpret_cast<float4*>(wz + (size_t)m * a.Nout + n) =
                make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
      }
      return;
    }
  }
  __syncthreads();
  if constexpr (EPI == 0) {
    staged_epilogue<BM, BN, WM, WN, SCATTER, NTH>(a, acc, m0, m_end, n0, wm, wn, tid, smem, bx, pcls);
  } else if (EPI == 1) {
    static_assert(EPI != 1 || LDS_MAIN >= BM * (BN / 4 + 4) * 4 + BM * (BN / 4 + 8) * 2, "LSTM staging");
    lstm_staged_epilogue<BM, BN, WM, WN, NTH>(a, acc, m0, m_end, n0, wm, wn, tid, smem);
  } else if (EPI == 2) {
    lstm_bwd_staged_epilogue<BM, BN, WM, WN, NTH>(a, acc, m0, m_end, n0, wm, wn, tid, smem);
  } else {
    int mrow[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * WTM + i * 16 + fr;
      mrow[i] = m < m_end ? m : -1;
    }
    igemm_epilogue<BM, BN, WM, WN, SCATTER, EPI, NTH>(a, acc, mrow, n0, wm, wn, tid, smem, bx);
  }
}


// Split-K fold: dst = bf16(sum_z ws[z] + bias) (+ old dst), plus the BN partial
// statistics of the stored values per row tile (tiles aligned to the statistic
// groups: [G][tpg][2][Nout]).  Thread = 8 consecutive channels of SK_PASS rows
// (a tile = SK_PASS * 256 / (Nout / 8) rows); every slab's loads for the SK_PASS
// rows are issued together (the fold is latency-bound otherwise).
constexpr int SK_PASS = 4;
__global__ __launch_bounds__(NT) void splitk_reduce_kernel(Geo a, int tpg) {
  __shared__ float red[NT][17];
  const int CG = a.Nout / 8, RPP = NT / CG, RB = SK_PASS * RPP;
  const int grp = blockIdx.x / tpg, t = blockIdx.x - grp * tpg;
  const int r0 = grp * a.Mg + t * RB, r1 = min(r0 + RB, (grp + 1) * a.Mg);
  const int cg = threadIdx.x % CG, n = cg * 8, rr = threadIdx.x / CG;
  float f[SK_PASS][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float bv = a.bias ? a.bias[n + e] : 0.f;
#pragma unroll
    for (int p = 0; p < SK_PASS; ++p) f[p][e] = bv;
  }
  const size_t slab = (size_t)a.M * a.Nout;
  for (int z = 0; z < a.ksplit; ++z) {
#pragma unroll
    for (int p = 0; p < SK_PASS; ++p) {
      const int m = r0 + rr + p * RPP;
      if (m >= r1) continue;
      const float* w = a.ws + z * slab + (size_t)m * a.Nout + n;
      const float4 lo = *reinterpret_cast<const float4*>(w);
      const float4 hi = *reinterpret_cast<const float4*>(w + 4);
      f[p][0] += lo.x; f[p][1] += lo.y; f[p][2] += lo.z; f[p][3] += lo.w;
      f[p][4] += hi.x; f[p][5] += hi.y; f[p][6] += hi.z; f[p][7] += hi.w;
    }
  }
  float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int p = 0; p < SK_PASS; ++p) {
    const int m = r0 + rr + p * RPP;
    if (m >= r1) continue;
    uint16_t* d = a.dst + (size_t)m * a.dcs + n;
    if (a.accumulate) {
      float o[8];
      unpack8(*reinterpret_cast<const uint4*>(d), o);
#pragma unroll
      for (int e = 0; e < 8; ++e) f[p][e] = round_e(f[p][e]) + o[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) f[p][e] = round_e(f[p][e]);
    *reinterpret_cast<uint4*>(d) = pack8(f[p]);
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] += f[p][e]; s2[e] += f[p][e] * f[p][e]; }
  }
  if (!a.stats) return;
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[threadIdx.x][e] = s1[e]; red[threadIdx.x][8 + e] = s2[e]; }
  __syncthreads();
  for (int c = threadIdx.x; c < a.Nout; c += NT) {
    const int g8 = c / 8, e = c - g8 * 8;
    float u = 0.f, v = 0.f;
    for (int q = g8; q < NT; q += CG) { u += red[q][e]; v += red[q][8 + e]; }
    a.stats[(size_t)blockIdx.x * 2 * a.Nout + c] = u;
    a.stats[(size_t)blockIdx.x * 2 * a.Nout + a.Nout + c] = v;
  }
}

const Variant VARIANTS[] = {
    V_DMA('A', TILE_A, false, false, 0, false), V_DMA('A', TILE_A, false, false, 1, false),
    V_DMA('A', TILE_A, false, false, 2, false), V_DMA('A', TILE_A, false, true, 0, false),
    V_DMA('A', TILE_A, true, false, 0, false),
    V_DMA('E', TILE_E, false, false, 0, false), V_DMA('E', TILE_E, false, true, 0, false),
    V_DMA('E', TILE_E, true, false, 0, false),
    V_DMA('a', TILE_A, false, false, 0, true), V_DMA('e', TILE_E, false, false, 0, true),
    V_DMA('B', TILE_B, false, false, 0, false), V_DMA('B', TILE_B, false, true, 0, false),
    V_DMA('C', TILE_C, false, false, 0, false), V_DMA('C', TILE_C, false, true, 0, false),
    V_DMA('D', TILE_D, false, false, 0, false), V_DMA('D', TILE_D, false, true, 0, false),
    V_DMA('F', TILE_F, false, false, 0, false), V_DMA('F', TILE_F, false, true, 0, false),   // forced only
    V_REG('R', TILE_R, false, false, false, 0), V_REG('R', TILE_R, true, false, false, 0),
    V_REG('R', TILE_R, false, true, false, 0), V_REG('R', TILE_R, true, true, false, 0),
    V_REG('R', TILE_R, false, false, true, 0), V_REG('R', TILE_R, true, false, true, 0),
    V_REG('R', TILE_R, false, false, false, 1), V_REG('R', TILE_R, false, false, false, 2),
    V_REG('S', TILE_S, false, false, false, 0), V_REG('S', TILE_S, true, false, false, 0),
    V_REG('S', TILE_S, false, true, false, 0), V_REG('S', TILE_S, true, true, false, 0),
    V_REG('S', TILE_S, false, false, true, 0), V_REG('S', TILE_S, true, false, true, 0),
};

}  // namespace

Variants stf::ig::linear_variants() { return {VARIANTS, (int)(sizeof VARIANTS / sizeof VARIANTS[0])}; }

int stf::ig::sk_rows(int Nout) { return SK_PASS * (NT / (Nout / 8)); }

int stf::ig::splitk_reduce(const Geo& g, hipStream_t s) {
  const int tpg = (g.Mg + sk_rows(g.Nout) - 1) / sk_rows(g.Nout);
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(tpg * (g.M / g.Mg)), dim3(NT), 0, s, g, tpg);
  STF_CHECK_LAUNCH();
  return 0;
}
