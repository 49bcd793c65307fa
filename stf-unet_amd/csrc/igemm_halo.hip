// Halo kernel: 3x3 / stride 1 / pad 1 convolution (forward, and the stride-1
// dgrad over flipped taps) as nine shifted views of one LDS halo.
//
// The linear kernels above gather the source rows of every tap separately, so
// each activation row crosses L2 -> LDS nine times; for the 64-channel
// full-resolution layers that re-read traffic (~26 GB/s per CU) is the bound.
// Here a workgroup owns a PH x PW pixel tile and a 64-channel output slice; per
// 32-channel source chunk one stage holds the (PH+2) x (PW+2) halo and the 64 x
// 9 weight rows of that chunk, and the nine taps are read from the halo at row
// offsets (r * (PW+2) + s).  Persistent: each workgroup walks a contiguous run
// of (tile, channel-slice) items through a 2-stage LDS-DMA ring, so the next
// stage streams in behind the MFMAs and the epilogue.  Rows are 64 B with the
// chunk swizzle kc ^ ((key >> 1) & 2): for weight rows key = row, for halo rows
// key = the halo COLUMN, so a tap's row shift dy leaves the swizzle unchanged (an
// immediate offset).  Both are conflict-free for every ds_read_b128 lane group at
// any tap shift (checked exhaustively over columns, shifts and row residues).
#include "igemm_common.h"

namespace {
using namespace stf::ig;

// tap before which the first wave half issues the next stage's DMA share (-1: at the stage start;
// the second half issues at tap 4); a build-time A/B switch (-DHALO_ATAP=2)
#ifndef HALO_ATAP
#define HALO_ATAP -1
#endif

// output row (pixel index of the destination) of tile pixel p, or -1 outside the image
template <int PH, int PW, int IX>
STF_DEV int halo_pixel(int p, int img, int ty, int tx, int Hd, int Wd) {
  int y = ty * PH + p / PW, x = tx * PW + p % PW;
  if constexpr (IX > 1) {
    const int b = (p % PW) / (PW / IX);
    x = p % PW - b * (PW / IX);
    img += b;
  }
  return (y < Hd && x < Wd) ? (img * Hd + y) * Wd + x : -1;
}

// NW waves x 64 pixels = PH x PW tile; STAGES = 2: one 8-wave workgroup per CU
// with a 2-stage ring; STAGES = 1: two 4-wave workgroups per CU, single stage
// each, so one workgroup's DMA wait and epilogue overlap the other's MFMAs.
// DIRECT: weight rows are fetched in the permuted order
// row j*16 + fk*4 + r <- channel (j>>1)*32 + fk*8 + (j&1)*4 + r, so a lane's
// accumulators of fragments (0,1) and (2,3) are 8 consecutive channels each and
// the epilogue stores 16-B chunks straight from registers (no LDS staging).
//
// IX > 1 (multi-image tiles, conv3x3_halo2_kernel): the PH x PW tile is IX whole images of
// PH x (PW / IX) side by side (STF layer3: two 16 x 16 images in one 16 x 32 tile), so a
// small image fills the wide tile instead of half a 16 x 16 one: twice the pixels per stage
// for the same weight rows.  Neighbouring images share one zero column in the halo (image
// b's column x sits at halo column b * (IW + 1) + 1 + x), PW + IX + 1 columns in all.
// DEFER (8-wave, 2-stage direct epilogues): the second wave half (waves NW/2.., the SIMD
// partners of the first half) runs each item's epilogue after the next stage barrier, ahead of
// its next taps, so on every SIMD one wave's epilogue (VALU, stores) overlaps its partner's
// MFMAs instead of both idling the matrix pipe together; BatchNorm partials are then kept per
// wave (one statistics row per (group, workgroup, wave): no cross-wave LDS pass, no epilogue
// barrier) and the BN-backward y tile is loaded to registers.
template <int PH, int PW, int NW, int STAGES, int DIAG, int DIRECT, bool BNR, int IX, bool DEFER_T = false>
__device__ __forceinline__ void halo_body(Geo a, uint32_t src_bytes, int TY, int TX, int per, int rem) {
  constexpr int NTH = 64 * NW, BN = 64, RPI = 16;       // 64-B rows: 16 per 1-KiB DMA instruction
  constexpr int IW = PW / IX;                           // image width in a multi-image tile
  constexpr int HW = PW + IX + 1, HR = (PH + 2) * HW;   // halo rows
  // DMA instructions per stage, dealt to the waves as evenly as they go (wave w: hcnt(w) from
  // hbeg(w)); the ring holds exactly these rows, so the stages leave room for the affine area
  constexpr int HIN = (HR + RPI - 1) / RPI, WIN = 9 * BN / RPI;
  constexpr int HI = (HIN + NW - 1) / NW, WI = (WIN + NW - 1) / NW;   // per wave, at most
  constexpr int HROWS = HIN * RPI, WROWS = WIN * RPI;
  constexpr int STAGE = (HROWS + WROWS) * 64;
  constexpr int AFF = STAGES * STAGE;                 // BNR: per-wave BN affine [4][64] fp32 after the ring
  static_assert(9 * BN % RPI == 0, "weight rows");
  constexpr int PX = PH * PW, WTM = PX / NW, TM = WTM / 16, TN = BN / 16;
  constexpr int PPP = NTH / 8, NSTORE = PX / PPP;      // epilogue: pixels per pass, stores per lane
  // next stage's DMA (STAGES == 2): even waves at the stage start, odd waves after tap 4.
  // DIAG 4 cycle buckets (tools/halo_timeline.py, 256^2 64->64): with every wave issuing
  // at once a third of the wave time is spent stalled issuing LDS-DMA; staggered, one wave
  // of each SIMD computes while the other issues (-8 % cycles).  Spreading every wave's
  // instructions over the taps only moves the stall into the taps: the DMA path itself
  // is the limit, fewer bytes per FLOP is what would help.
  constexpr bool STAGGER = STAGES == 2 && NW == 8;
  constexpr bool DF = DEFER_T && DIRECT != 0 && STAGGER;   // the deferred epilogue (8-wave direct kernels)
  static_assert((WTM == 64 || WTM == 32) && PW % 16 == 0 && PX % PPP == 0, "tile");
  static_assert(PX * 128 + NW * 2 * 64 * 4 <= STAGE, "epilogue scratch");
  // per-wave epilogue scratch after the ring (BNR or DF): [scale | shift | mean | invstd][64] fp32 of
  // the current (group, slice) for the BN-backward reduction, or (DF forward) the slice's 64 biases
  constexpr int EPS = (BNR || DF) ? NW * 1024 : 0;
  static_assert((AFF + EPS) * (STAGES == 1 ? 2 : 1) <= 163840, "LDS");
  __shared__ __attribute__((aligned(16))) char smem[STAGES * STAGE + EPS];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform: scalar DMA addressing
  const int fr = lane & 15, fk = lane >> 4, sub = lane >> 2, slot = lane & 3;
  const bool late = DF ? wave >= NW / 2 : (wave & 1);   // issues its DMA share at tap 4
  const int NTn = a.Nout / BN, CC = a.Cs / 32, tpi = TY * TX;
  const int ntiles = (a.N / IX) * tpi;                  // items: channel slice major, pixel tile minor
  const int ipg = a.Mg / (a.Hd * a.Wd);                 // images per statistics group
  const int vb = blockIdx.x;
  const int cnt = per + (int)(vb < rem);
  const int it0 = vb * per + min(vb, rem);
  const int S = cnt * CC;
  if (S == 0) return;

  const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc((void*)a.src, 0, src_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_wgt =
      __builtin_amdgcn_make_buffer_rsrc((void*)a.wgt, 0, (uint32_t)a.Nout * a.K * 2, 0x00020000);
  constexpr uint32_t BAD = 0xFFFFFFF0u;
  // NULL bias -> zero-sized range: the loads return 0 without a branch
  const __amdgpu_buffer_rsrc_t rs_bias = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.bias, 0, a.bias ? (uint32_t)a.Nout * 4 : 0u, 0x00020000);

  // live = false: a dummy stage (all lanes out of range) so every iteration issues the same DMA count
  // DMA instructions k0 .. k1-1 of this wave's HI halo + WI weight instructions
  // weight rows held by each ring stage: key nt * CC + cc (wave-uniform, every wave tracks
  // the same sequence).  With an even chunk count a stage holds the same source chunk for
  // every item, so within one output slice its weight rows never change and the refill
  // of the stage only streams the halo (half the DMA instructions at 64 source channels).
  int wkey0 = -1, wkey1 = -1;
  auto issue_part = [&](int item, int cc, int buf, bool live, int k0, int k1, bool wload) {
    const int nt = item / ntiles, tile = item - nt * ntiles;
    const int tq = tile / tpi, t2 = tile - tq * tpi, ty = t2 / TX, tx = t2 - ty * TX, img = tq * IX;
    const int y0 = ty * PH - 1, x0 = tx * PW - 1;
    char* st = smem + buf * STAGE;
    const int hcnt = HIN / NW + (wave < HIN % NW), hbeg = wave * (HIN / NW) + min(wave, HIN % NW);
    const int wcnt = WIN / NW + (wave < WIN % NW), wbeg = wave * (WIN / NW) + min(wave, WIN % NW);
#pragma unroll
    for (int i = 0; i < HI; ++i) {
      if (i < k0 || i >= k1 || i >= hcnt) continue;
      const int hr = (hbeg + i) * RPI + sub;
      const int hy = hr / HW, hx = hr - hy * HW;
      int ys = y0 + hy, xs = x0 + hx, im = img;
      if constexpr (IX > 1) {                         // image b, column hx - b (IW + 1) - 1 (-1: a pad)
        const int b = min(hx / (IW + 1), IX - 1);
        xs = hx - b * (IW + 1) - 1;
        im = img + b;
      }
      const bool ok = live && hr < HR && ys >= 0 && xs >= 0 && ys < a.Hs && xs < (IX > 1 ? IW : a.Ws);
      const uint32_t off =
          ok ? (uint32_t)((((im * a.Hs + ys) * a.Ws + xs) * a.scs + cc * 32 + swzh(hx, slot) * 8) * 2) : BAD;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs_src, (__attribute__((address_space(3))) void*)(st + (hbeg + i) * RPI * 64), 16, off, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      if (HI + i < k0 || HI + i >= k1 || !wload || i >= wcnt) continue;
      const int wr = (wbeg + i) * RPI + sub;            // weight row = tap * 64 + n
      const int wrow = wr & 63;
      const int tap = wr >> 6,
                n = nt * BN + (DIRECT ? ((wrow >> 5) * 32 + ((wrow >> 2) & 3) * 8 + ((wrow >> 4) & 1) * 4 + (wrow & 3))
                                      : wrow);
      const bool ok = live && wr < 9 * BN;
      const uint32_t off = ok ? (uint32_t)(((size_t)n * a.K + tap * a.Cs + cc * 32 + swzh(wr, slot) * 8) * 2) : BAD;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs_wgt, (__attribute__((address_space(3))) void*)(st + (HROWS + (wbeg + i) * RPI) * 64), 16, off, 0,
          0, 0);
    }
  };
  auto issue = [&](int item, int cc, int buf, bool live, bool wload = true) {
    issue_part(item, cc, buf, live, 0, HI + WI, wload);
  };
  // does filling stage buf with (item, cc) need the weight DMA?  (and record what it holds)
  auto need_w = [&](int item, int cc, int buf, bool live) {
    if (STAGES != 2 || !live) return true;
    const int key = (item / ntiles) * CC + cc;
    int& held = buf ? wkey1 : wkey0;
    const bool need = held != key;
    held = key;
    return need;
  };

  // byte offset (within a stage) of this lane's halo read for fragment i at tap column dx,
  // tap row 0: the swizzle is keyed on the halo column, so the tap row dy only adds the
  // immediate dy * HW * 64 (12 address registers instead of one per (i, tap))
  int xb[TM][3];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int p = wave * WTM + i * 16 + fr;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int px = p % PW, hx = px + px / IW * (IX > 1 ? 1 : 0) + dx;   // + one shared pad per image
      xb[i][dx] = ((p / PW) * HW + hx) * 64 + swzh(hx, fk) * 16;
    }
  }
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (STAGES == 2) issue(it0, 0, 0, true, need_w(it0, 0, 0, true));
  int iit = it0, icc = 0;                               // issue cursor (last issued stage)
  int cit = it0, ccc = 0;                               // compute cursor
  // BN partial statistics, one row per (group, workgroup): stats [groups][gridDim][2][Nout].
  // Thread tid < 128 owns (sum | sum of squares, channel col) of the current (group, slice) and
  // zeroes its rows first (same thread, same addresses: ordered).  DF: the two wave halves finish
  // an item on opposite sides of a barrier, so there is no per-item cross-wave pass: every lane
  // keeps its wave's running partials of the last KMAX (group, slice) keys in registers (lane (fr,
  // fk), fragment half h: row half fr >> 3, channel h*32 + fk*8 + (fr & 7), where
  // row16_reduce_scatter leaves them; the host checks a workgroup's item run spans <= KMAX keys)
  // and the waves' partials are folded once, in wave order, after the loop.
  constexpr int KMAX = 2;
  const int q_st = tid >> 6, col_st = tid & 63;
  const int groups = a.M / a.Mg;
  int run_key = -1;
  float run = 0.f;
  float kr[KMAX][2];                                     // DF: running partials, newest key first
  int kv[KMAX], nk = 0;                                  // DF: their keys (wave-uniform)
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { kr[k][0] = kr[k][1] = 0.f; kv[k] = -1; }
  // BNR: the same rows hold the fused BN-backward partials (sum g, sum g*xhat)
  float* const sbuf = BNR ? a.bnr_part : (DIRECT == 1 ? nullptr : a.stats);
  auto srow = [&](int g) { return (size_t)(g * gridDim.x + vb); };
  auto flush = [&]() {
    const int g = run_key / NTn, nt = run_key - g * NTn;
    sbuf[(srow(g) * 2 + q_st) * a.Nout + nt * BN + col_st] = run;
  };
  if (sbuf && tid < 128) {
    for (int g = 0; g < groups; ++g)
      for (int nt = 0; nt < NTn; ++nt) sbuf[(srow(g) * 2 + q_st) * a.Nout + nt * BN + col_st] = 0.f;
  }
  // BNR: this wave's copy of the BatchNorm affine of the current (group, slice) in LDS,
  // [scale | shift | mean | invstd][64 channels], reloaded when the key changes
  float* const aff = reinterpret_cast<float*>(smem + AFF) + wave * 256;
  int aff_key = -1, bias_key = -1;
  bool epi = false;                                      // previous stage ended with an epilogue (8 stores)
  bool wl_next = true;                                   // the next fill streams weight rows too
  bool pend = false;                                     // DF: this wave owes item pend_it's epilogue
  int pend_it = 0;
  f32x4 bv[TN];                                          // bias of the lane's 16 accumulator channels
#pragma unroll
  for (int j = 0; j < TN; ++j) bv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // DIAG 4: per-wave cycle buckets (s_memtime) -- DMA wait, barrier, DMA issue, taps, epilogue
  uint64_t tb[5] = {0, 0, 0, 0, 0}, tprev = 0;
  auto stamp = [&](int k) {
    if constexpr (DIAG == 4) {
      const uint64_t t = __builtin_amdgcn_s_memtime();
      if (k >= 0) tb[k] += t - tprev;
      tprev = t;
    }
  };

  // ---- direct epilogue of item `item` from acc / bv: lane (fr, fk) holds pixel p's channels
  // 8fk..8fk+7 (fragments 0,1) and 32+8fk.. (2,3).  Order: pack the accumulators (64 fp32 -> 32
  // bf16x2 registers, the accumulators die), [BNR: the y tile], the dz stores, then the partial
  // sums from the packed (stored, rounded) values.  Every load precedes every store (vmcnt
  // retires in order: a later load would wait for the stores in front of it); invalid pixels get
  // an out-of-range offset, so every lane issues exactly NSTORE = 2 * TM stores.  Sums: DPP
  // reduce-scatter over the 16 pixels of a fragment row; without DF one LDS pass over the
  // waves (the stage just read is the scratch: `buf`).
  auto direct_epi = [&](int item, int buf) {
    const int nt = item / ntiles, tile = item - nt * ntiles;
    const int tq = tile / tpi, t2 = tile - tq * tpi, ty = t2 / TX, tx = t2 - ty * TX, img = tq * IX;
    const uint32_t dst_records = (uint32_t)((size_t)a.M * a.dcs * 2);
    const __amdgpu_buffer_rsrc_t rs_dst = __builtin_amdgcn_make_buffer_rsrc((void*)a.dst, 0, dst_records, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    uint4 uq[2][TM];
    int mq[TM];
    // bias of the lane's 16 accumulator channels: DF -- from the wave's LDS copy of the slice's
    // biases (no registers held across the stage), else the registers load_bias filled
    f32x4 be[TN];
    if constexpr (DF) {
#pragma unroll
      for (int j = 0; j < TN; ++j) be[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (!BNR && a.bias) {
        if (nt != bias_key) {                          // same-wave LDS write -> read: ordered
          bias_key = nt;
          aff[lane] = a.bias[nt * BN + lane];
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) be[j] = *reinterpret_cast<const f32x4*>(aff + (j >> 1) * 32 + fk * 8 + (j & 1) * 4);
      }
    } else {
#pragma unroll
      for (int j = 0; j < TN; ++j) be[j] = bv[j];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int p = wave * WTM + i * 16 + fr;
      mq[i] = halo_pixel<PH, PW, IX>(p, img, ty, tx, a.Hd, a.Wd);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float f[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          f[r] = acc[i][2 * h][r] + be[2 * h][r];
          f[4 + r] = acc[i][2 * h + 1][r] + be[2 * h + 1][r];
        }
        if (a.accumulate && mq[i] >= 0) {
          float o[8];
          unpack8(*reinterpret_cast<const uint4*>(a.dst + (size_t)mq[i] * a.dcs + nt * BN + h * 32 + fk * 8), o);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] += o[e];
        }
        uq[h][i] = pack8(f);
        acc[i][2 * h] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc[i][2 * h + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    const int key = (img / ipg) * NTn + nt;
    float* red = reinterpret_cast<float*>(smem + buf * STAGE);   // [NW][2][64]
    // BNR scratch without DF: y rows [WTM][128 B] per wave in the stage just read, after the
    // [NW][2][64] reduction rows (16-B chunk c of pixel row r at slot c ^ (r & 7): conflict-free)
    char* yl = smem + buf * STAGE + NW * 2 * 64 * 4 + wave * WTM * 128;
    uint4 yq[2][TM];
    if constexpr (BNR) {
      if (key != aff_key) {                             // this wave's affine of (group, slice)
        aff_key = key;
        const size_t o = (size_t)(img / ipg) * a.Nout + nt * BN + lane;
        const float v0 = a.bnr_scale[o], v1 = a.bnr_shift[o], v2 = a.bnr_mean[o], v3 = a.bnr_invstd[o];
        aff[lane] = v0; aff[64 + lane] = v1; aff[128 + lane] = v2; aff[192 + lane] = v3;
      }
      const __amdgpu_buffer_rsrc_t rs_y = __builtin_amdgcn_make_buffer_rsrc(
          (void*)a.bnr_y, 0, (uint32_t)((size_t)a.M * a.bnr_ycs * 2), 0x00020000);
      if constexpr (DF) {
        // y straight to registers (the accumulators are dead): lane (fr, fk) loads exactly the
        // 8 channels of pixel i*16+fr that it holds in uq[h][i]
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int i = 0; i < TM; ++i) {
            const uint32_t off =
                mq[i] >= 0 ? (uint32_t)(((size_t)mq[i] * a.bnr_ycs + nt * BN + h * 32 + fk * 8) * 2) : 0xFFFFFFF0u;
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs_y, off, 0, 0);
            yq[h][i] = make_uint4(v.x, v.y, v.z, v.w);
          }
      } else {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                   // every wave is done reading this stage
        (buf ? wkey1 : wkey0) = -1;                     // the y rows overwrite its weight rows
#pragma unroll
        for (int k = 0; k < WTM / 8; ++k) {
          const int r = k * 8 + (lane >> 3), p = wave * WTM + r;       // 8 pixel rows per instruction
          const int m = halo_pixel<PH, PW, IX>(p, img, ty, tx, a.Hd, a.Wd);
          const int c = (lane & 7) ^ (r & 7);
          const uint32_t off = m >= 0 ? (uint32_t)(((size_t)m * a.bnr_ycs + nt * BN + c * 8) * 2) : 0xFFFFFFF0u;
          __builtin_amdgcn_raw_ptr_buffer_load_lds(
              rs_y, (__attribute__((address_space(3))) void*)(yl + k * 1024), 16, off, 0, 0, 0);
        }
      }
    }
    if (!BNR && IX == 1) {
      // (not with the fused BN-backward reduction, nor in the multi-image kernels: their registers
      // leave no room -- they spilled)
      // lane (fr, fk) holds chunks fk (h = 0) and 4 + fk (h = 1) of pixel i*16 + fr: its h = 1 chunk
      // and pixel index go to lane fr ^ 8 (DPP row_ror:8), so each store writes 8 whole 128-B pixel
      // rows (pixels 0-7 of the group, then 8-15) instead of half of 16 -- as many stores
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const uint4 u1 = uq[1][i];
        const uint4 rcv = make_uint4(__builtin_amdgcn_update_dpp(0u, u1.x, 0x128, 0xF, 0xF, false),
                                     __builtin_amdgcn_update_dpp(0u, u1.y, 0x128, 0xF, 0xF, false),
                                     __builtin_amdgcn_update_dpp(0u, u1.z, 0x128, 0xF, 0xF, false),
                                     __builtin_amdgcn_update_dpp(0u, u1.w, 0x128, 0xF, 0xF, false));
        const int mx = __builtin_amdgcn_update_dpp(0, mq[i], 0x128, 0xF, 0xF, false);
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const bool own = (half == 0) == (fr < 8);
          const uint4 v = own ? uq[0][i] : rcv;
          const int m = own ? mq[i] : mx;
          const int ch = (own ? 0 : 32) + fk * 8;
          const uint32_t off = m >= 0 ? (uint32_t)(((size_t)m * a.dcs + nt * BN + ch) * 2) : 0xFFFFFFF0u;
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{v.x, v.y, v.z, v.w}, rs_dst, off, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const uint4 u = uq[h][i];
          const uint32_t off =
              mq[i] >= 0 ? (uint32_t)(((size_t)mq[i] * a.dcs + nt * BN + h * 32 + fk * 8) * 2) : 0xFFFFFFF0u;
          __builtin_amdgcn_raw_buffer_store_b128(u32x4{u.x, u.y, u.z, u.w}, rs_dst, off, 0, 0);
        }
    }
    float res[2] = {0.f, 0.f};                           // row16_reduce_scatter results per half
    if constexpr (BNR) {
      // g = dz * [y*scale+shift > 0]; (sum g, sum g*xhat), like stf_bn_bwd_reduce
      // the y loads (issued before the stores) have landed; the stores stay in flight
      asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * TM) : "memory");
      auto aff8 = [&](int k, int c0, float* v) {
        const float4 lo = *reinterpret_cast<const float4*>(aff + k * 64 + c0);
        const float4 hi = *reinterpret_cast<const float4*>(aff + k * 64 + c0 + 4);
        v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w; v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
      };
      const bool norelu = !a.bnr_relu;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // sum g*y per lane (TM pixels), turned into sum g*xhat = invstd*(sum g*y - mean*sum g)
        float q1[8], q2[8], sc[8], sh[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { q1[e] = 0.f; q2[e] = 0.f; }
        aff8(0, h * 32 + fk * 8, sc);
        aff8(1, h * 32 + fk * 8, sh);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          float g[8], yv[8];
          unpack8(uq[h][i], g);
          const int r = i * 16 + fr;
          if constexpr (DF) unpack8(yq[h][i], yv);
          else unpack8(*reinterpret_cast<const uint4*>(yl + r * 128 + (((h * 4 + fk) ^ (r & 7)) << 4)), yv);
          const bool valid = mq[i] >= 0;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            // bitwise, not short-circuit: a select, no branch
            const bool keep = valid & (norelu | (yv[e] * sc[e] + sh[e] > 0.f));
            const float gg = keep ? g[e] : 0.f;
            q1[e] += gg;
            q2[e] += gg * yv[e];
          }
        }
        float mu[8], is[8], v[16];
        aff8(2, h * 32 + fk * 8, mu);
        aff8(3, h * 32 + fk * 8, is);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = q1[e];
          v[8 + e] = is[e] * (q2[e] - mu[e] * q1[e]);
        }
        res[h] = row16_reduce_scatter(v, fr);
      }
    } else if constexpr (DIRECT == 2) {
      // BN statistics (sum, sum of squares) of the stored values
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          float g[8];
          unpack8(uq[h][i], g);
          const float w = mq[i] >= 0 ? 1.f : 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) { v[e] += w * g[e]; v[8 + e] += w * g[e] * g[e]; }
        }
        // lane fr ends with value fr: sum (fr < 8) or sum of squares of channel fr & 7
        res[h] = row16_reduce_scatter(v, fr);
      }
      if constexpr (!DF) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                   // every wave is done reading this stage
      }
    }
    if (sbuf) {
      if constexpr (DF) {
        // this wave's running partials of the current (group, slice); a new key shifts them
        if (nk == 0 || key != kv[0]) {
#pragma unroll
          for (int k = KMAX - 1; k > 0; --k) { kr[k][0] = kr[k - 1][0]; kr[k][1] = kr[k - 1][1]; kv[k] = kv[k - 1]; }
          kr[0][0] = kr[0][1] = 0.f;
          kv[0] = key;
          ++nk;
        }
        kr[0][0] += res[0];
        kr[0][1] += res[1];
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) red[(wave * 2 + (fr >> 3)) * 64 + h * 32 + fk * 8 + (fr & 7)] = res[h];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (tid < 128) {
          const int q = tid >> 6, col = tid & 63;
          float t = 0.f;
#pragma unroll
          for (int w = 0; w < NW; ++w) t += red[(w * 2 + q) * 64 + col];
          if (key != run_key) {
            if (run_key >= 0) flush();
            run_key = key;
            run = 0.f;
          }
          run += t;
        }
      }
    }
  };

  // DF: one more pass through the loop head after the last stage runs the last epilogue
  for (int s = 0; s < S + (DF ? 1 : 0); ++s) {
    const int buf = STAGES == 2 ? (s & 1) : 0;
    stamp(-1);
    auto load_bias = [&]() {
      // bias of this lane's 16 accumulator channels, loaded BEFORE the next DMA so
      // that waiting for it never waits for the DMA (BNR: a dgrad, no bias)
      if constexpr (BNR || (DF && DIRECT)) {           // (DF: direct_epi reads them from LDS)
#pragma unroll
        for (int j = 0; j < TN; ++j) bv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      } else if (ccc == CC - 1) {
        const int nt = cit / ntiles;
#pragma unroll
        for (int j = 0; j < TN; ++j)
          bv[j] = __builtin_amdgcn_raw_buffer_load_b128(
            rs_bias, (nt * BN + (DIRECT ? (j >> 1) * 32 + fk * 8 + (j & 1) * 4 : j * 16 + fk * 4)) * 4, 0, 0);
      }
    };
    if constexpr (STAGES == 2) {
      // retire this stage's DMA; the previous epilogue's NSTORE buffer stores
      // (issued after it, stores and loads retire in order) may stay in flight
      if (epi) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(NSTORE) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      stamp(0);
      epi = false;
      if constexpr (DF) {
        // the epilogue of the item that ended with the previous stage: the first wave half runs
        // it before this stage barrier, the second half (its SIMD partners) after it, ahead of
        // its taps -- one code site, the barrier instruction placed by wave half (s_barrier
        // counts arrivals, not program points; `late` is wave-uniform)
        if (late) __builtin_amdgcn_s_barrier();
        if (pend) { direct_epi(pend_it, buf ^ 1); pend = false; }
        if (!late) __builtin_amdgcn_s_barrier();
        if (s == S) break;
      } else {
        __builtin_amdgcn_s_barrier();
      }
      stamp(1);
      load_bias();
      const bool live = s + 1 < S;
      if (live && ++icc == CC) { icc = 0; ++iit; }
      wl_next = need_w(iit, icc, (s + 1) & 1, live && (DIAG != 2 || s < 1));
      // the first wave half issues the next stage's DMA now, the second (DF: its SIMD partners,
      // waves >= NW/2; else the odd waves) after tap 4: the address path takes ~300 cycles per 1-KiB
      // LDS-DMA instruction under load, and with all eight waves issuing at once both waves of a
      // SIMD stalled together (DIAG 4: a third of the time); staggered, one wave of each SIMD
      // computes while the other issues
      if (!STAGGER || (!late && HALO_ATAP < 0)) issue(iit, icc, (s + 1) & 1, live && (DIAG != 2 || s < 1), wl_next);
      stamp(2);
    } else {
      // single stage: every wave is done with the buffer, refill it, wait
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      load_bias();
      issue(cit, ccc, 0, DIAG != 2 || s < 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    }
    const char* hb = smem + buf * STAGE;
    if (DIAG == 3) { if (++ccc == CC) { ccc = 0; ++cit; } continue; }
    const char* wb = hb + HROWS * 64;
    // software-pipelined taps: tap t+1's fragments are read while tap t's TM x TN MFMAs
    // run (double-buffered registers).  The reads are inline-asm ds_read_b128 (kept in
    // issue order; the compiler otherwise sinks them next to their MFMAs and exposes the
    // LDS latency) and the wait is explicit: lgkmcnt(TM + TN) leaves exactly the tap-t+1
    // reads in flight, and it passes tap t's fragments through as operands so no MFMA
    // can be scheduled above it.  All reads have retired (lgkmcnt(0)) by the last tap.
    e16x8 xf[2][TM], wf[2][TN];
    const uint32_t hb32 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const char*)hb;
    const uint32_t wrow0 = (uint32_t)((HROWS + fr) * 64 + swzh(fr, fk) * 16);    // weight row j*16+fr of tap 0
    auto rd_tap = [&](int t, int b) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
        asm volatile("ds_read_b128 %0, %1 offset:%2"
                     : "=v"(xf[b][i]) : "v"(hb32 + xb[i][t % 3]), "i"((t / 3) * HW * 64));
#pragma unroll
      for (int j = 0; j < TN; ++j)                 // (row >> 1) & 2 of t*64 + j*16 + fr = that of fr
        asm volatile("ds_read_b128 %0, %1 offset:%2"
                     : "=v"(wf[b][j]) : "v"(hb32 + wrow0), "i"((t * BN + j * 16) * 64));
    };
    rd_tap(0, 0);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int b = t & 1;
      if constexpr (STAGGER) {
        if (t == (late ? 4 : HALO_ATAP)) issue(iit, icc, (s + 1) & 1, s + 1 < S && (DIAG != 2 || s < 1), wl_next);
      }
      if (t + 1 < 9) rd_tap(t + 1, b ^ 1);
      // wait for tap t's fragments (the TM + TN tap-t+1 reads may stay in flight)
      static_assert(TN == 4 && (TM == 4 || TM == 2), "fragment wait");
      if constexpr (TM == 4) {
        if (t + 1 < 9)
          asm volatile("s_waitcnt lgkmcnt(8)" : "+v"(xf[b][0]), "+v"(xf[b][1]), "+v"(xf[b][2]), "+v"(xf[b][3]),
                       "+v"(wf[b][0]), "+v"(wf[b][1]), "+v"(wf[b][2]), "+v"(wf[b][3]));
        else
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xf[b][0]), "+v"(xf[b][1]), "+v"(xf[b][2]), "+v"(xf[b][3]),
                       "+v"(wf[b][0]), "+v"(wf[b][1]), "+v"(wf[b][2]), "+v"(wf[b][3]));
      } else {
        if (t + 1 < 9)
          asm volatile("s_waitcnt lgkmcnt(6)" : "+v"(xf[b][0]), "+v"(xf[b][1]),
                       "+v"(wf[b][0]), "+v"(wf[b][1]), "+v"(wf[b][2]), "+v"(wf[b][3]));
        else
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(xf[b][0]), "+v"(xf[b][1]),
                       "+v"(wf[b][0]), "+v"(wf[b][1]), "+v"(wf[b][2]), "+v"(wf[b][3]));
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = mfma16x16x32(wf[b][j], xf[b][i], acc[i][j]);
    }
    stamp(3);
    if (DIRECT && ccc + 1 == CC) {
      if constexpr (DF) {                              // at the next loop head
        pend = true;
        pend_it = cit;
      } else {
        direct_epi(cit, buf);
        epi = true;
      }
      stamp(4);
      ccc = 0;
      ++cit;
      continue;
    }
    if constexpr (DIRECT) {                            // (the last chunk took the branch above)
      ++ccc;
      continue;
    }
    if (++ccc == CC) {
      // ---- epilogue through LDS: the stage just read becomes the output tile
      // [PX][64] bf16 (128-B rows, 16-B chunk c at c ^ (p & 7)); full-row 16-B
      // buffer stores (invalid pixels get an out-of-range offset, so every lane
      // issues exactly NSTORE stores and the next stage can wait with vmcnt(NSTORE));
      // BN partial sums from the stored values; raw barriers only, so nothing
      // drains the stores or the DMA already in flight.
      const int nt = cit / ntiles, tile = cit - nt * ntiles;
      const int tq = tile / tpi, t2 = tile - tq * tpi, ty = t2 / TX, tx = t2 - ty * TX, img = tq * IX;
      char* ot = smem + buf * STAGE;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();                     // every wave is done reading this stage
      (buf ? wkey1 : wkey0) = -1;                       // the output tile overwrites its weight rows
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int p = wave * WTM + i * 16 + fr;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int ch = j * 16 + fk * 4, c16 = ch >> 3;
          const uint2 v = make_uint2(pack2(acc[i][j][0] + bv[j][0], acc[i][j][1] + bv[j][1]),
                                     pack2(acc[i][j][2] + bv[j][2], acc[i][j][3] + bv[j][3]));
          *reinterpret_cast<uint2*>(ot + p * 128 + ((c16 ^ (p & 7)) << 4) + (ch & 7) * 2) = v;
          acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      const int c16 = tid & 7;
      const uint32_t dst_records = (uint32_t)((size_t)a.M * a.dcs * 2);
      const __amdgpu_buffer_rsrc_t rs_dst = __builtin_amdgcn_make_buffer_rsrc((void*)a.dst, 0, dst_records, 0x00020000);
      float s1[8], s2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
#pragma unroll
      for (int k = 0; k < NSTORE; ++k) {
        const int p = (tid >> 3) + PPP * k;
        const int mm = halo_pixel<PH, PW, IX>(p, img, ty, tx, a.Hd, a.Wd);
        const bool ok = mm >= 0;
        const int m = ok ? mm : 0;
        uint4 u = *reinterpret_cast<const uint4*>(ot + p * 128 + ((c16 ^ (p & 7)) << 4));
        const uint32_t off = ok ? (uint32_t)(((size_t)m * a.dcs + nt * BN + c16 * 8) * 2) : 0xFFFFFFF0u;
        float f[8];
        unpack8(u, f);
        if (a.accumulate && ok) {
          float o[8];
          unpack8(*reinterpret_cast<const uint4*>(a.dst + (size_t)m * a.dcs + nt * BN + c16 * 8), o);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = round_e(f[e] + o[e]);
          u = pack8(f);
        }
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{u.x, u.y, u.z, u.w}, rs_dst, off, 0, 0);
        if (ok) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { s1[e] += f[e]; s2[e] += f[e] * f[e]; }
        }
      }
      if (a.stats) {
        // lanes with equal (lane & 7) hold the same 8 channels: fold 8 -> 1 per wave, then over waves
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
          for (int o = 8; o < 64; o <<= 1) {
            s1[e] += __shfl_xor(s1[e], o, 64);
            s2[e] += __shfl_xor(s2[e], o, 64);
          }
        float* red = reinterpret_cast<float*>(ot + PX * 128);   // [NW][2][64]
        if (lane < 8) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            red[(wave * 2 + 0) * 64 + lane * 8 + e] = s1[e];
            red[(wave * 2 + 1) * 64 + lane * 8 + e] = s2[e];
          }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (tid < 128) {
          const int q = tid >> 6, col = tid & 63;
          float t = 0.f;
#pragma unroll
          for (int w = 0; w < NW; ++w) t += red[(w * 2 + q) * 64 + col];
          const int key = (img / ipg) * NTn + nt;
          if (key != run_key) {
            if (run_key >= 0) flush();
            run_key = key;
            run = 0.f;
          }
          run += t;
        }
      }
      ccc = 0;
      ++cit;
      epi = true;
    }
  }
  if constexpr (DF) {
    if (sbuf) {
      // every wave has left the loop (the second half after its last epilogue) and every DMA has
      // landed (the loop head's vmcnt(0)): the ring is free.  Partials [KMAX][NW][2][64] fp32,
      // folded in wave order by the threads that own the rows.
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      float* part = reinterpret_cast<float*>(smem);
      const int nkk = nk < KMAX ? nk : KMAX;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < nkk)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            part[((k * NW + wave) * 2 + (fr >> 3)) * 64 + h * 32 + fk * 8 + (fr & 7)] = kr[k][h];
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (tid < 128) {
        for (int k = 0; k < nkk; ++k) {
          float t = 0.f;
#pragma unroll
          for (int w = 0; w < NW; ++w) t += part[((k * NW + w) * 2 + q_st) * 64 + col_st];
          run_key = kv[k];
          run = t;
          flush();
        }
      }
    }
  } else {
    if (sbuf && tid < 128 && run_key >= 0) flush();
  }
  if constexpr (DIAG == 4) {                           // a.stats doubles as the [grid][NW][8] u64 buffer
    if (lane == 0) {
      unsigned long long* d = reinterpret_cast<unsigned long long*>(a.stats) + (vb * NW + wave) * 8;
#pragma unroll
      for (int k = 0; k < 5; ++k) d[k] = tb[k];
    }
  }
}

template <int PH, int PW, int NW, int STAGES, int DIAG, int DIRECT = 0, bool BNR = false, bool DEFER = false>
__global__ __launch_bounds__(64 * NW, (STAGES == 1) ? 2 : 1) void conv3x3_halo_kernel(Geo a, uint32_t src_bytes,
                                                                                    int TY, int TX, int per, int rem) {
  halo_body<PH, PW, NW, STAGES, DIAG, DIRECT, BNR, 1, DEFER>(a, src_bytes, TY, TX, per, rem);
}

// two 16 x 16 images per 16 x 32 tile (IX = 2); TY = TX = 1
template <int DIRECT, bool BNR, bool DEFER = false>
__global__ __launch_bounds__(512, 1) void conv3x3_halo2_kernel(Geo a, uint32_t src_bytes, int TY, int TX, int per,
                                                               int rem) {
  halo_body<16, 32, 8, 2, 0, DIRECT, BNR, 2, DEFER>(a, src_bytes, TY, TX, per, rem);
}

// four 8 x 8 images per 8 x 32 tile (IX = 4; STF layer4), 4 waves, one stage, two workgroups per
// CU (61 KB of LDS each): one workgroup's DMA waits hide behind the other's MFMAs.  (A 2-stage
// ring at one workgroup per CU, for grids under 2 x CUs, was faster alone -- forward 64 -> 61 us,
// BN-backward dgrad 84 -> 66 us -- but its 123 KB of LDS kept the side streams' weight gradients
// and LSTMs off the CU: the STF step -0.5 % over five same-box repeats; removed in round 6.)
template <int DIRECT>
__global__ __launch_bounds__(256, 2) void conv3x3_halo4_kernel(Geo a, uint32_t src_bytes, int TY, int TX, int per,
                                                               int rem) {
  halo_body<8, 32, 4, 1, 0, DIRECT, false, 4>(a, src_bytes, TY, TX, per, rem);
}

const Variant VARIANTS[] = {
    V_TILE('4', 256, conv3x3_halo4_kernel, 0, 0, 0, 0, 0),
    V_HALO2(2, false), V_HALO2(1, false), V_HALO2(1, true),
    // (no 16 x 16 <1, false, false>: a launch without statistics rows always defers)
    V_HALO(16, 0, 2, false, false), V_HALO(16, 0, 2, false, true), V_HALO(16, 0, 1, false, true),
    V_HALO(16, 0, 1, true, false), V_HALO(16, 0, 1, true, true),
    V_HALO(32, 0, 2, false, false), V_HALO(32, 0, 2, false, true), V_HALO(32, 0, 1, false, true),
    V_HALO(32, 0, 1, true, false), V_HALO(32, 0, 1, true, true),
#if HALO_DIAG   // timing-only builds (igemm_common.h)
    V_HALO(32, 4, 1, false, false), V_HALO(32, 2, 2, false, false), V_HALO(32, 2, 1, false, false),
#endif
};

}  // namespace

Variants stf::ig::halo_variants() { return {VARIANTS, (int)(sizeof VARIANTS / sizeof VARIANTS[0])}; }
