// What the implicit-GEMM translation units share (igemm.hip has the map of the files): the kernel
// argument record, the LDS chunk swizzles, the variant record with the macros that build its
// entries, and what the router in igemm.hip needs from each kernel family.
#pragma once
#include "common.h"
#include "../../include/stfunet.h"

namespace stf {
namespace ig {

constexpr int BK = 32;
constexpr int NT = 256;

struct Geo {
  const uint16_t* src; const uint16_t* wgt; uint16_t* dst;
  const float* bias; float* stats;
  int N, Hs, Ws, Cs, scs, Hd, Wd, R, S, st, pad, M, K, Nout, dcs;
  int Mg, tpg;          // rows per statistics group, M tiles per group
  int accumulate;
  // LSTM cell epilogue (Nout = 4*Ch, column 4c+q = gate q of hidden channel c)
  const float* c_prev; float* c_out; uint16_t* h_out; int hcs; float* gates;
  // LSTM cell backward epilogue (EPI 2, gates recomputed): c_out = c_t (read)
  const uint16_t* l_dh; int l_dhcs; const float* l_dcn; float* l_dcp; uint16_t* l_dg;
  // fused BN-backward reduction (stf_bnr_epi)
  const uint16_t* bnr_y; int bnr_ycs; const float *bnr_scale, *bnr_shift, *bnr_mean, *bnr_invstd;
  int bnr_relu; float* bnr_part;
  // stride-2 transposed gather with rows ordered by output parity class (see igemm_dma_kernel)
  int par;
  // split-K (plain DMA kernels): blockIdx.z = K slice, fp32 partials [ksplit][M][Nout] in ws,
  // folded by splitk_reduce_kernel (bias, bf16 store, BN statistics)
  int ksplit; float* ws;
};

// 64-B LDS rows of the linear kernels: the 16-B chunk of row r sits at chunk ^ ((-(r>>2)) & 3)
STF_DEV int swz(int row, int kc) { return kc ^ ((-(row >> 2)) & 3); }
// 64-B LDS rows of the halo and wide kernels (igemm_halo.hip explains the key)
STF_DEV int swzh(int key, int kc) { return kc ^ ((key >> 1) & 2); }

// pixel tile edge of conv3x3_c8_kernel (the router counts its tiles)
constexpr int C8_T = 16;

// Timing-only build of the 16 x 32 halo kernel (results wrong, never in the shipped build; made with
// tools/build_variant.sh and loaded through STF_LIB): every launch the router would give to a
// conv3x3_halo_kernel<16, 32, ...> without the fused BN-backward takes the DIAG instantiation instead.
// 4 = per-wave cycle buckets written over the statistics rows (tools/halo_timeline.py), 2 = no DMA
// reloads after the first stage.
#ifndef HALO_DIAG
#define HALO_DIAG 0
#endif
static_assert(HALO_DIAG == 0 || HALO_DIAG == 2 || HALO_DIAG == 4, "HALO_DIAG: 0, 2 or 4");

// Tiles of the linear DMA kernel (BM, BN, waves WM x WN, BK, ring stages) and of the register-staged one
struct Cfg { int bm, bn, wm, wn, bkk, stages; };
#define TILE_A 128, 128, 2, 2, 32, 4   // 4 waves, 2 blocks/CU
#define TILE_B 256, 128, 4, 2, 64, 3   // 8 waves
#define TILE_C 256, 256, 2, 4, 64, 2   // 8 waves
#define TILE_D 512, 64, 8, 1, 64, 2    // 8 waves
#define TILE_E 256, 64, 4, 1, 32, 4    // 4 waves, 2 blocks/CU
#define TILE_F 128, 256, 2, 4, 32, 2   // 8 waves, 2 blocks/CU (80 KiB each)
#define TILE_R 128, 128, 2, 2          // register-staged
#define TILE_S 256, 64, 4, 1           // register-staged, Nout <= 64

// One launchable instantiation.  family: 'K' 8-channel input, '4' four 8 x 8 images per tile, 'W' wide
// (128-channel slices), '2' two 16 x 16 images per tile, 'h' / 'H' single-image 16 x 16 / 16 x 32 tiles,
// a linear DMA tile letter ('a' / 'e': the 8-channel-input forms of A / E), 'R' / 'S' register-staged.
// key: halo families {DIRECT, BNR, DEFER, DIAG}; DMA {TRANS, SCATTER, EPI}; register-staged
// {SMALLC, TRANS, SCATTER, EPI}.  Name, key and kernel of an entry come from the same macro arguments.
struct Variant {
  const char* name;
  char family;
  int key[4];
  int threads, bn;
  void (*tile)(Geo, uint32_t, int, int, int, int);
  void (*c8)(Geo, int, int, int, int);
  void (*dma)(Geo, uint32_t);
  void (*reg)(Geo);
};
#define STF_STR_(...) #__VA_ARGS__
#define STF_STR(...) STF_STR_(__VA_ARGS__)
#define V_TILE(FAM, THREADS, KERNEL, K0, K1, K2, K3, ...) \
  {#KERNEL "<" STF_STR(__VA_ARGS__) ">", FAM, {K0, K1, K2, K3}, THREADS, 64, KERNEL<__VA_ARGS__>, nullptr, nullptr, nullptr}
#define V_HALO(PW, DIAG, DIRECT, BNR, DEFER) \
  V_TILE(PW == 16 ? 'h' : 'H', 512, conv3x3_halo_kernel, DIRECT, BNR, DEFER, DIAG, 16, PW, 8, 2, DIAG, DIRECT, BNR, DEFER)
#define V_HALO2(DIRECT, BNR) V_TILE('2', 512, conv3x3_halo2_kernel, DIRECT, BNR, 0, 0, DIRECT, BNR, false)
#define V_WIDE(DIRECT, BNR) V_TILE('W', 512, conv3x3_wide_kernel, DIRECT, BNR, 0, 0, DIRECT, BNR)
#define V_DMA(FAM, TILE, TR, SC, EPI, C8)                                                              \
  {"igemm_dma_kernel<" STF_STR(TILE, TR, SC, EPI, C8) ">", FAM, {TR, SC, EPI, 0},                      \
   64 * Cfg{TILE}.wm * Cfg{TILE}.wn, Cfg{TILE}.bn, nullptr, nullptr, igemm_dma_kernel<TILE, TR, SC, EPI, C8>, nullptr}
#define V_REG(FAM, TILE, SMALLC, TR, SC, EPI)                                                          \
  {"igemm_kernel<" STF_STR(TILE, SMALLC, TR, SC, EPI) ">", FAM, {SMALLC, TR, SC, EPI}, NT, Cfg{TILE, 0, 0}.bn, \
   nullptr, nullptr, nullptr, igemm_kernel<TILE, SMALLC, TR, SC, EPI>}

// Each family file's entries of the variant table; find_variant (igemm.hip) walks them in this order.
struct Variants { const Variant* v; int n; };
Variants c8_variants();       // igemm_c8.hip
Variants halo_variants();     // igemm_halo.hip
Variants wide_variants();     // igemm_wide.hip
Variants linear_variants();   // igemm_linear.hip

// igemm_linear.hip: rows per statistics tile of the split-K fold, and the fold's launch after a
// ksplit > 1 launch (a hipError_t, 0 on success)
int sk_rows(int Nout);
int splitk_reduce(const Geo& g, hipStream_t s);

}  // namespace ig
}  // namespace stf
