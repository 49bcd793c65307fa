// Implicit-GEMM convolution on MFMA (gfx950): forward / dgrad / transposed-conv.  This file is the
// host side: the router and the C entry points.  The kernels live one family per file:
//   igemm_common.h    Geo (the kernel arguments), the LDS chunk swizzles, the Variant record and the
//                     V_* macros that build its entries, the tile shapes
//   igemm_linear.hip  any geometry, one GEMM row per destination pixel: igemm_kernel (register-
//                     staged), igemm_dma_kernel (LDS-DMA ring), their epilogues, the split-K fold
//   igemm_halo.hip    3x3 / stride 1 / pad 1 as nine shifted views of one LDS halo, 64-channel
//                     output slices: one, two or four images per tile
//   igemm_wide.hip    the same with 128-channel output slices
//   igemm_c8.hip      3x3 / stride 1 / pad 1 of the 8-channel network input
// Each family file ends with its entries of the variant table.
//
// Every entry point below computes one Route (route_of) and reads everything else from it.  The
// Route names one Variant, which carries the kernel's name as the profiler prints it AND the
// kernel, so stf_igemm_kernel_name and the launch cannot disagree.
#include "igemm_common.h"
#include <stdio.h>
#include <stdlib.h>

namespace {
using namespace stf::ig;

constexpr int HALO_PH = 16, HALO_PW = 32;   // halo tile: 16 x 32 pixels, 8 waves, 2-stage ring (1 WG/CU)
constexpr int HALO_MIN_W = 16;              // narrowest layer of the halo kernel (16 x 16 tiles below W = 32)

int num_cus() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
      v = 256;
    return v;
  }();
  return n;
}

Cfg cfg_of(char k) {
  switch (k) {
    case 'B': return Cfg{TILE_B};
    case 'C': return Cfg{TILE_C};
    case 'D': return Cfg{TILE_D};
    case 'E': case 'e': return Cfg{TILE_E};
    case 'F': return Cfg{TILE_F};
    default: return Cfg{TILE_A};
  }
}

const Variant* find_variant(char family, int k0, int k1, int k2, int k3) {
  for (const Variants s : {c8_variants(), halo_variants(), wide_variants(), linear_variants()})
    for (const Variant* v = s.v; v < s.v + s.n; ++v)
      if (v->family == family && v->key[0] == k0 && v->key[1] == k1 && v->key[2] == k2 && v->key[3] == k3) return v;
  return nullptr;
}

// STF_IGEMM_CFG forces a tile (tools/bench_gemm_shape.py): A-F a linear DMA tile, H the halo family
// wherever it applies, L the linear kernels only; '0' = auto
char forced_cfg() {
  static const char c = [] {
    const char e = stf::ab_letter("STF_IGEMM_CFG");
    return ((e >= 'A' && e <= 'F') || e == 'H' || e == 'L') ? e : '0';
  }();
  return c;
}

// Which kernel runs a launch, on what grid, and what its size queries answer.
struct Route {
  const Variant* variant = nullptr;   // nullptr: no kernel takes these arguments (STF_EINVAL)
  char kind = 'R';       // 'K' 8-channel input, 'H' halo family, a linear DMA tile letter, 'R' register-staged
  // persistent tile kernels ('K', 'H'): images per tile, tile width, tiles per image, work items
  // (tile x output slice), grid, items per workgroup and the remainder
  int ix = 1, pw = HALO_PW, ty = 0, tx = 0, grid = 0, per = 0, rem = 0;
  long items = 0;
  bool wide = false;         // 128-channel output slices (conv3x3_wide_kernel)
  int direct = 0;            // epilogue: 0 LDS-staged, 1 direct stores, 2 direct with statistics
  bool bnr_fused = false;    // the BN-backward reduction runs in the epilogue (else stf_bn_bwd_reduce after)
  bool defer = false;        // deferred epilogue of the second wave half
  // linear kernels: M tile, M tiles per statistics group, split-K factor, stride-2 transposed
  // parity mode (0 off, 1 rows by output parity class, 2 also skipping the tap-less classes)
  int bm = 128, tpg = 0, ksplit = 1, par = 0;
  int stat_tiles = 0, bnr_tiles = 0;   // partial rows per group: BN statistics, BN-backward sums
  size_t ws_bytes = 0;                 // split-K workspace
};

// with_stats: the launch writes BN statistics.  stf_igemm passes a->stats != nullptr; the size
// queries pass what the launch will do (stf_igemm_stat_tiles is asked before the statistics buffer
// exists: true; stf_igemm_bnr_tiles: false).
//
// The rules, in the order they apply (STF_IGEMM_CFG: see forced_cfg; it also turns rule 1 off):
//  1. 8-channel network input, 3x3, 64 outputs -> conv3x3_c8_kernel (cfg2 step 23.4 -> 23.2 ms against
//     the linear 'e' kernel, profiles/r03/ab_c8.txt); any other plain 8-channel gather -> 'e' / 'a'.
//  2. sources or weights past the 4 GiB buffer descriptor, or Cs not a multiple of 32 -> register-staged
//     (256 x 64 tile for Nout <= 64, else 128 x 128).
//  3. LSTM steps (1x1 GEMM, K = 2C) -> the 128 x 128 DMA tile (any tile gives the same gates -- the same
//     MFMA sequence over ascending K -- so the backward recompute may run another tile).
//  4. 3x3 / stride 1 / pad 1 with Nout % 64 == 0 -> the halo family when W >= 32; at 16 <= W < 32 up to
//     256 outputs (round 3: the 16 x 16 tile wins up to 256 output channels, the 256 x 256 linear tile
//     above); above 256 outputs when the two-image tile applies (rule 6; UNet's bottleneck); at
//     8 x 8 when the four-image tile applies (rule 5).
//  5. 8 x 8 layers, N and the images per statistics group multiples of 4 -> four images per 8 x 32 tile
//     (conv3x3_halo4_kernel, LDS-staged epilogue; against the linear split-K kernels the STF step
//     10.34 -> 10.25 ms, profiles/r03/ab_halo2.txt).  A BN-backward request is not fused on it.
//  6. 16 x 16 layers, N and the images per group even -> two images per 16 x 32 tile, for launches that
//     write statistics (the forward convs) and for every launch with more than 256 outputs (UNet's
//     bottleneck: its dgrads run 4-22 % faster on them than on single-image tiles or the linear
//     kernels, tools/bench_layers.py, profiles/r06/ab_bottleneck_halo2.txt).  The other dgrads stay on
//     single-image tiles: they run beside the side-stream weight gradients, and the 160 KiB workgroup
//     of the 16 x 32 tile cannot share a CU with them (128 KiB for 16 x 16); all on two-image tiles
//     re-measured neutral to -0.9 % (profiles/r06/ab_halo2_all_stf.txt).
//  7. single-image tiles, Nout % 128 == 0 and W >= 32 -> the wide kernel (128-channel slices), forward,
//     plain and BN-backward-fused dgrad (cfg2 +0.5..0.8 %, profiles/r06/ab_wide_halo.txt, ab_wide_bnr.txt).
//  8. every halo tile but the four-image one stores directly (1.7 % faster on the forward convs than
//     the LDS-staged epilogue) and fuses a BN-backward request into that epilogue.
//  9. single-image 64-channel-slice tiles defer the second wave half's epilogue (the two-image tiles
//     would spill registers).  Its statistics fold keeps at most 2 (group, slice) keys per workgroup:
//     the item run of a workgroup (items / grid + 1, slice-major, image-major within a slice) must not
//     span more, else the launch does not defer.
// 10. other gathers -> linear DMA tiles, measured per layer (tools/bench_layers.py, cfg2 shapes): with
//     Cs % 64 == 0 and not transposed C where it fills the chip, B for 128-multiples of outputs, D for
//     64 outputs; else E for Nout <= 64 and A.
// 11. stride-2 transposed gathers on A / E with one statistics group walk their rows by output parity
//     class, only that class's taps; accumulating launches whose epilogue adds nothing of its own (no
//     bias, statistics or BN reduce) skip the tap-less classes.
// 12. plain gathers on the upper-case DMA tiles that would leave the chip under-filled (small M: STF
//     layer4 at 8 x 8, LSTM backward GEMMs) split K: slices until ~256 workgroups, each keeping >= 8
//     K steps, at most 8.
Route route_of(const stf_igemm_args* a, bool with_stats) {
  const stf_conv_geom& c = a->g;
  Route r;
  const char f = forced_cfg();
  const long M = (long)c.N * c.Hd * c.Wd;
  const long Mg = a->group_rows > 0 ? a->group_rows : M;
  const long hw = (long)c.Hd * c.Wd, imgs = hw > 0 ? Mg / hw : 0;      // images per statistics group
  const int lstm_epi = a->lstm ? (a->lstm->backward ? 2 : 1) : 0;
  const bool plain = !a->lstm && !a->scatter2x2 && !c.transposed;
  const bool dma_ok = (uint64_t)c.N * c.Hs * c.Ws * c.src_cstride * 2 < 0xFFFFFF00ull &&
                      (uint64_t)a->Nout * c.R * c.S * c.Cs * 2 < 0xFFFFFF00ull;
  // the tile kernels ('K', halo family) store through a 32-bit buffer descriptor over the whole
  // destination and read the fused BN-backward y through one: both extents must fit it, else the
  // launch takes a linear kernel (64-bit destination addressing; the BN-backward reduce runs after)
  const bool tile_ok = (uint64_t)M * a->dst_cstride * 2 < 0xFFFFFF00ull &&
                       (!a->bnr || (uint64_t)M * a->bnr->y_cstride * 2 < 0xFFFFFF00ull);
  const bool conv3 = plain && c.R == 3 && c.S == 3 && c.stride == 1 && c.pad == 1 && c.Hd == c.Hs && c.Wd == c.Ws &&
                     tile_ok;
  const bool c8 = f == '0' && conv3 && !a->bnr && !a->accumulate && c.Cs == 8 && c.src_cstride % 8 == 0 &&
                  a->Nout == 64 && a->dst_cstride % 8 == 0 && ((uintptr_t)a->dst & 15) == 0;
  const bool four = c.Hd == 8 && c.Wd == 8 && c.N % 4 == 0 && a->Nout % 64 == 0 && c.Cs % 32 == 0 && imgs % 4 == 0;
  const bool two = !four && (with_stats || a->Nout > 256) && c.Hd == 16 && c.Wd == 16 && c.N % 2 == 0 && imgs % 2 == 0;
  const bool halo = conv3 && a->Nout % 64 == 0 &&
                    (f == 'H' || (f == '0' && (c.Wd >= 32 || (c.Wd >= HALO_MIN_W && a->Nout <= 256) ||
                                               (a->Nout > 256 && two) || four)));
  const char small = a->Nout <= 64 ? 'E' : 'A';
  const bool bk64 = c.Cs % 64 == 0 && !c.transposed;
  if (c8) r.kind = 'K';
  else if (dma_ok && plain && c.Cs == 8) r.kind = a->Nout <= 64 ? 'e' : 'a';
  else if (!dma_ok || c.Cs % 32) r.kind = 'R';
  else if (a->lstm) r.kind = 'A';
  else if (halo) r.kind = 'H';
  else if (f == 'A' || f == 'E') r.kind = f == 'E' ? small : 'A';
  else if (f >= 'B' && f <= 'F' && bk64) r.kind = f;
  else if (bk64 && a->Nout % 256 == 0 && ((M + 255) / 256) * ((a->Nout + 255) / 256) >= 240) r.kind = 'C';
  else if (bk64 && a->Nout % 128 == 0) r.kind = 'B';
  else if (bk64 && a->Nout == 64) r.kind = 'D';
  else r.kind = small;
  const char k = r.kind;

  if (k == 'K') {
    r.ty = (c.Hd + C8_T - 1) / C8_T;
    r.tx = (c.Wd + C8_T - 1) / C8_T;
    r.items = c.N * r.ty * r.tx;
    r.grid = (int)std::min<long>(r.items, 2 * num_cus());             // two workgroups per CU
    r.variant = find_variant('K', 0, 0, 0, 0);
  } else if (k == 'H') {
    r.ix = four ? 4 : two ? 2 : 1;
    r.pw = c.Wd >= 32 ? HALO_PW : 16;
    r.wide = r.ix == 1 && a->Nout % 128 == 0 && c.Wd >= 32;
    r.ty = r.ix > 1 ? 1 : (c.Hd + HALO_PH - 1) / HALO_PH;
    r.tx = r.ix > 1 ? 1 : (c.Wd + r.pw - 1) / r.pw;
    r.items = (long)(c.N / r.ix) * r.ty * r.tx * (a->Nout / (r.wide ? 128 : 64));
    // one workgroup per CU (160 KiB LDS each; the single-stage 8 x 8 kernel two)
    r.grid = (int)std::min<long>(r.items, (long)num_cus() * (four ? 2 : 1));
    r.direct = four ? 0 : with_stats ? 2 : 1;
    r.bnr_fused = a->bnr && !four;
    if (r.ix == 1 && !r.wide && r.grid > 0) {
      const long run = imgs * r.ty * r.tx, per = r.items / r.grid + 1;   // items per (group, slice) key
      r.defer = (!with_stats && !a->bnr) || (run > 0 && (per + run - 1) / run + 1 <= 2);
    }
    const int d = r.bnr_fused ? 1 : r.direct;
    if (four) r.variant = find_variant('4', 0, 0, 0, 0);
    else if (r.wide) r.variant = find_variant('W', r.direct, r.bnr_fused, 0, 0);
    else if (two) r.variant = find_variant('2', d, r.bnr_fused, 0, 0);
    else if (r.pw == 16) r.variant = find_variant('h', d, r.bnr_fused, r.defer, 0);
#if HALO_DIAG   // timing-only builds (igemm_common.h)
    else if (!r.bnr_fused) r.variant = find_variant('H', HALO_DIAG == 4 ? 1 : d, 0, 0, HALO_DIAG);
#endif
    else r.variant = find_variant('H', d, r.bnr_fused, r.defer, 0);
  } else {
    const bool reg = k == 'R';
    r.bm = reg ? ((a->Nout <= 64 && !a->lstm) ? 256 : 128) : cfg_of(k).bm;
    if (reg) r.variant = find_variant(r.bm == 256 ? 'S' : 'R', c.Cs % BK != 0, c.transposed != 0, a->scatter2x2 != 0, lstm_epi);
    else r.variant = find_variant(k, c.transposed != 0, a->scatter2x2 != 0, lstm_epi, 0);
  }
  if (r.grid > 0) {
    r.per = (int)(r.items / r.grid);
    r.rem = (int)(r.items % r.grid);
  }

  r.tpg = (int)((Mg + r.bm - 1) / r.bm);
  if (c.transposed && c.stride == 2 && (k == 'A' || k == 'E') && Mg == M) {
    r.par = a->accumulate && !a->bias && !with_stats && !a->bnr ? 2 : 1;
    long blocks = 0;
    for (int cl = 0; cl < 4; ++cl) {
      const int ntap = ((c.R - (((cl >> 1) + c.pad) & 1) + 1) >> 1) * ((c.S - (((cl & 1) + c.pad) & 1) + 1) >> 1);
      if (r.par == 2 && ntap == 0) continue;
      blocks += ((long)c.N * ((c.Hd - (cl >> 1) + 1) >> 1) * ((c.Wd - (cl & 1) + 1) >> 1) + r.bm - 1) / r.bm;
    }
    r.tpg = (int)blocks;
  }
  if (plain && c.Cs != 8 && k >= 'A' && k <= 'F' && a->Nout % 8 == 0 && NT % (a->Nout / 8) == 0 &&
      a->dst_cstride % 8 == 0 && ((uintptr_t)a->dst & 15) == 0) {
    const Cfg t = cfg_of(k);
    const long blocks = (M / Mg) * ((Mg + t.bm - 1) / t.bm) * ((a->Nout + t.bn - 1) / t.bn);
    const long kt = (long)c.R * c.S * c.Cs / t.bkk;
    if (blocks < 192 && kt >= 16) r.ksplit = (int)std::max<long>(1, std::min<long>({(256 + blocks - 1) / blocks, kt / 8, 8}));
  }
  if (r.ksplit > 1) r.ws_bytes = (size_t)r.ksplit * c.N * c.Hd * c.Wd * a->Nout * sizeof(float);

  if (k == 'H' || k == 'K') r.stat_tiles = r.grid;
  else if (r.ksplit > 1) r.stat_tiles = (int)((Mg + sk_rows(a->Nout) - 1) / sk_rows(a->Nout));
  else r.stat_tiles = (int)((Mg + r.bm - 1) / r.bm);
  const int groups = a->group_rows > 0 ? (int)std::max<long>(1, M / a->group_rows) : 1;
  r.bnr_tiles = r.bnr_fused ? r.grid : stf_bn_bwd_tiles(c.N, c.Hd, c.Wd, a->Nout, groups, 0);
  return r;
}

}  // namespace

// BatchNorm partial-statistics rows per group for the kernel that will run
extern "C" int stf_igemm_stat_tiles(const stf_igemm_args* a) { return route_of(a, true).stat_tiles; }

extern "C" size_t stf_igemm_ws_bytes(const stf_igemm_args* a) { return route_of(a, a->stats != nullptr).ws_bytes; }

extern "C" int stf_igemm_bnr_tiles(const stf_igemm_args* a) { return route_of(a, false).bnr_tiles; }

// Name of the device kernel these args run (as rocprofv3 prints it), for timers
extern "C" const char* stf_igemm_kernel_name(const stf_igemm_args* a) {
  const Route r = route_of(a, a->stats != nullptr);
  return r.variant ? r.variant->name : "(no kernel)";
}

extern "C" int stf_igemm(const stf_igemm_args* a, stf_stream_t stream) {
  const stf_conv_geom& c = a->g;
  if (a->Nout % 8 || c.Cs % 8 || c.src_cstride % 8 || a->dst_cstride % 4) return STF_EINVAL;
  if (c.transposed && !(c.stride == 1 || c.stride == 2)) return STF_EINVAL;
  if (a->scatter2x2 && (c.transposed || (a->Nout / 4) % 4)) return STF_EINVAL;
  if (((uintptr_t)a->src & 15) || ((uintptr_t)a->wgt & 15) || ((uintptr_t)a->dst & 7)) return STF_EINVAL;
  if (a->bnr && (a->stats || a->bias || a->lstm || a->scatter2x2 || !a->bnr->y || !a->bnr->partial || a->bnr->y_cstride % 8 ||
                 a->dst_cstride % 8 || ((uintptr_t)a->dst & 15) || ((uintptr_t)a->bnr->y & 15)))
    return STF_EINVAL;
  Geo g;
  g.src = (const uint16_t*)a->src; g.wgt = (const uint16_t*)a->wgt; g.dst = (uint16_t*)a->dst;
  g.bias = a->bias; g.stats = a->stats;
  g.N = c.N; g.Hs = c.Hs; g.Ws = c.Ws; g.Cs = c.Cs; g.scs = c.src_cstride;
  g.Hd = c.Hd; g.Wd = c.Wd; g.R = c.R; g.S = c.S; g.st = c.stride; g.pad = c.pad;
  g.M = c.N * c.Hd * c.Wd; g.K = c.R * c.S * c.Cs; g.Nout = a->Nout; g.dcs = a->dst_cstride;
  if (g.M <= 0) return 0;
  g.Mg = a->group_rows > 0 ? a->group_rows : g.M;
  if (g.M % g.Mg) return STF_EINVAL;
  g.accumulate = a->accumulate;
  g.c_prev = nullptr; g.c_out = nullptr; g.h_out = nullptr; g.hcs = 0; g.gates = nullptr;
  g.bnr_y = nullptr; g.bnr_ycs = 0; g.bnr_scale = g.bnr_shift = g.bnr_mean = g.bnr_invstd = nullptr;
  g.bnr_relu = 0; g.bnr_part = nullptr;
  g.ksplit = 1; g.ws = nullptr;
  if (a->bnr) {
    g.bnr_y = (const uint16_t*)a->bnr->y; g.bnr_ycs = a->bnr->y_cstride;
    g.bnr_scale = a->bnr->scale; g.bnr_shift = a->bnr->shift; g.bnr_mean = a->bnr->mean;
    g.bnr_invstd = a->bnr->invstd; g.bnr_relu = a->bnr->relu; g.bnr_part = a->bnr->partial;
  }
  g.l_dh = nullptr; g.l_dhcs = 0; g.l_dcn = nullptr; g.l_dcp = nullptr; g.l_dg = nullptr;
  if (a->lstm) {
    const stf_lstm_epi& l = *a->lstm;
    if (a->scatter2x2 || c.transposed || a->Nout % 4 || !l.c_out) return STF_EINVAL;
    if (l.backward) {
      if (!l.dh || !l.dc_prev || !l.dgates || ((uintptr_t)l.dgates & 7)) return STF_EINVAL;
      g.l_dh = (const uint16_t*)l.dh; g.l_dhcs = l.dh_cstride; g.l_dcn = l.dc_next; g.l_dcp = l.dc_prev;
      g.l_dg = (uint16_t*)l.dgates;
    } else if (!l.h_out) {
      return STF_EINVAL;
    }
    g.c_prev = l.c_prev; g.c_out = l.c_out; g.h_out = (uint16_t*)l.h_out;
    g.hcs = l.h_cstride; g.gates = l.gates;
  }
  const Route r = route_of(a, a->stats != nullptr);
  if (!r.variant) return STF_EINVAL;
  const Variant& v = *r.variant;
  g.tpg = r.tpg;
  g.par = r.par;
  if (r.ksplit > 1) {
    if (!a->ws || ((uintptr_t)a->ws & 15)) return STF_EINVAL;
    g.ksplit = r.ksplit; g.ws = a->ws;
  }
  hipStream_t s = (hipStream_t)stream;
  const uint32_t src_bytes = (uint32_t)((uint64_t)c.N * c.Hs * c.Ws * c.src_cstride * 2);
  const dim3 lin_grid(g.tpg * ((g.M + g.Mg - 1) / g.Mg), (g.Nout + v.bn - 1) / v.bn, g.ksplit);
  if (v.c8 || v.tile) {
    if ((g.Mg % (c.Hd * c.Wd)) != 0) return STF_EINVAL;
    if (v.c8) hipLaunchKernelGGL(v.c8, dim3(r.grid), dim3(v.threads), 0, s, g, r.ty, r.tx, r.per, r.rem);
    else hipLaunchKernelGGL(v.tile, dim3(r.grid), dim3(v.threads), 0, s, g, src_bytes, r.ty, r.tx, r.per, r.rem);
  } else if (v.dma) {
    hipLaunchKernelGGL(v.dma, lin_grid, dim3(v.threads), 0, s, g, src_bytes);
  } else {
    hipLaunchKernelGGL(v.reg, lin_grid, dim3(v.threads), 0, s, g);
  }
  STF_CHECK_LAUNCH();
  if (g.ksplit > 1) {
    const int e = splitk_reduce(g, s);
    if (e) return e;
  }
  if (!a->bnr || r.bnr_fused) return 0;
  // unfused: one stf_bn_bwd_reduce pass over the stored dz (same partial layout)
  const int groups = a->group_rows > 0 ? g.M / a->group_rows : 1;
  return stf_bn_bwd_reduce(a->dst, a->dst_cstride, nullptr, a->bnr->y, a->bnr->y_cstride, c.N, c.Hd, c.Wd, a->Nout,
                           groups, a->bnr->scale, a->bnr->shift, a->bnr->mean, a->bnr->invstd, a->bnr->relu ? 1 : 0,
                           nullptr, 0, nullptr, a->bnr->partial, stream);
}
