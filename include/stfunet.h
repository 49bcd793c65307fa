/*
 * stfunet.h -- C ABI of the MI355X (gfx950) STF-Unet training hot path.
 *
 * The reference (XiangFeng-Wen/STF-Unet) has no FFI: its hot path is the
 * PyTorch nn.Module surface of src/unet.py and src/stf_lstm_unet.py plus the
 * engine functions of train_utils/.  Every entry point below replaces the
 * PyTorch/MIOpen kernels behind one op *call site* of that path (cited per
 * function).  The Python host mirror (stf-unet_amd/stfunet) binds them with
 * ctypes; see INTEGRATION.md.
 *
 * Conventions
 *  - Activations: NHWC bf16.  A tensor argument is (pointer to its first used
 *    channel, channel stride in elements) so producers can write straight into
 *    a channel slice of a concat buffer ("virtual concat").
 *  - Weights: bf16, K-contiguous GEMM rows [Nout][R][S][Cs].
 *  - Statistics, master weights, gradients, optimizer state: fp32.
 *  - Every function is stream-ordered on `stream` (a hipStream_t), allocates
 *    nothing, keeps no pointer after it returns and has no mutable global state.
 *  - Return value: 0 on success, a hipError_t code on launch failure, or
 *    STF_EINVAL (100001) when the arguments violate a documented constraint.
 */
#ifndef STFUNET_H
#define STFUNET_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* stf_stream_t; /* hipStream_t */

/* Geometry of one implicit-GEMM pass.  GEMM rows m = (n, yd, xd) walk the
 * destination grid [N][Hd][Wd]; the reduction k = (r, s, c) gathers the source
 * tensor [N][Hs][Ws][Cs]:
 *   transposed == 0 : ys = yd*stride - pad + r        (Conv2d forward, ConvT dgrad)
 *   transposed == 1 : ys = (yd + pad - r) / stride    (Conv2d dgrad, ConvTranspose2d
 *                     forward); taps with a non-zero remainder contribute 0.
 */
typedef struct stf_conv_geom {
  int N;
  int Hs, Ws, Cs;      /* source spatial dims and reduction channels            */
  int src_cstride;     /* elements between consecutive source pixels (>= Cs)   */
  int Hd, Wd;          /* destination (GEMM row) spatial dims                   */
  int R, S;            /* taps                                                  */
  int stride, pad;     /* transposed==1 requires stride in {1, 2}               */
  int transposed;
} stf_conv_geom;

/* LSTM cell fused into the GEMM epilogue: the GEMM computes the gate
 * pre-activations [x_t | h_{t-1}] . [W_ih | W_hh]^T with gate-interleaved
 * columns (column 4c+q = gate q in torch order i, f, g, o, of hidden channel c),
 * the epilogue adds the bias and applies c_t = f*c_{t-1} + i*g, h_t = o*tanh(c_t)
 * (nn.LSTM, src/stf_lstm_unet.py:124-127,219-235). */
typedef struct stf_lstm_epi {
  const float* c_prev; /* [M][Ch] c_{t-1}, or NULL (zero initial state)           */
  float* c_out;        /* forward: c_t out [M][Ch]; backward: c_t in (read only)  */
  void* h_out;         /* bf16, h_t written with stride h_cstride (may be the next */
  int h_cstride;       /* step's [x | h] buffer or the decoder's concat slice)     */
  float* gates;        /* forward: [M][4Ch] activated gates (i, f, g, o), or NULL  */
                       /* when the backward recomputes them (backward = 1)        */
  /* backward = 1: the GEMM recomputes step t's gate pre-activations from the same
   * [x_t | h_{t-1}] rows and weights (same kernel, so bitwise the forward's gates)
   * and the epilogue runs the cell backward (h_out / gates unused):
   *   tc = tanh c_t; dc = dh*o*(1-tc^2) + dc_next; dc_prev = dc*f;
   *   dgates = (dc*g*i(1-i), dc*c_{t-1}*f(1-f), dc*i*(1-g^2), dh*tc*o(1-o)) */
  int backward;
  const void* dh;      /* bf16 dL/dh_t, stride dh_cstride                          */
  int dh_cstride;
  const float* dc_next;/* [M][Ch] dL/dc_t from step t+1, or NULL (t = T-1)          */
  float* dc_prev;      /* [M][Ch] out, dL/dc_{t-1} (may alias dc_next)              */
  void* dgates;        /* bf16 [M][4Ch] pre-activation gate gradients, interleaved */
} stf_lstm_epi;

/* BatchNorm-backward reduction fused into a dgrad: dst receives dz, the gradient
 * w.r.t. act(BN(y)); the epilogue also produces the partial sums of
 * stf_bn_bwd_reduce (g = relu ? dz * [y*scale+shift > 0] : dz; sum g, sum g*xhat)
 * without a separate pass over dz and y.  Affine arrays are [groups][C]. */
typedef struct stf_bnr_epi {
  const void* y;       /* bf16 pre-BN activation [M][y_cstride], first channel      */
  int y_cstride;
  const float* scale; const float* shift; const float* mean; const float* invstd;
  int relu;
  float* partial;      /* [groups][stf_igemm_bnr_tiles][2][C] for stf_bn_bwd_finalize */
} stf_bnr_epi;

typedef struct stf_igemm_args {
  stf_conv_geom g;
  const void* src;     /* bf16, first used channel                              */
  const void* wgt;     /* bf16 [Nout][R*S*Cs]                                   */
  int Nout;            /* GEMM columns; multiple of 8                           */
  void* dst;           /* bf16, first channel of the destination slice          */
  int dst_cstride;
  const float* bias;   /* [Nout] (scatter2x2: [Nout/4]) or NULL                 */
  float* stats;        /* [tiles][2][Nout] per-tile (sum, sum of squares) of    */
                       /* the stored bf16 outputs, or NULL (tiles: see          */
                       /* stf_igemm_stat_tiles)                                 */
  int scatter2x2;      /* 1: ConvTranspose2d(k=2,s=2) epilogue: column          */
                       /* n = (dy*2+dx)*Cout + co lands on pixel (2yd+dy,2xd+dx)*/
                       /* of a [N][2Hd][2Wd] destination                        */
  int group_rows;      /* >0: tiles aligned to groups of this many rows (whole  */
                       /* images) and stats laid out [M/group_rows][tiles][2][Nout] */
                       /* (per-time-step BatchNorm of the batched STF encoder)  */
  int accumulate;      /* 1: dst += result (bf16 read-modify-write)             */
  const stf_lstm_epi* lstm; /* non-NULL: LSTM cell epilogue, dst unused          */
  const stf_bnr_epi* bnr;   /* non-NULL: fused BN-backward reduction (no stats,  */
                            /* no scatter/LSTM); group_rows = the BN's groups    */
  float* ws;           /* split-K fp32 workspace of stf_igemm_ws_bytes(a) bytes */
                       /* (16-B aligned), or NULL when that is 0 (ABI v4)      */
} stf_igemm_args;

/* Workspace bytes stf_igemm needs for these args: > 0 when the GEMM is split over
 * K (small-M layers that would under-fill the chip; the partials are folded by a
 * second launch that also writes the statistics). */
size_t stf_igemm_ws_bytes(const stf_igemm_args* a);

/* Partial-statistics rows per group for these args (the tiling depends on the
 * kernel chosen): size `stats` as groups * stf_igemm_stat_tiles(a) * 2 * Nout. */
int stf_igemm_stat_tiles(const stf_igemm_args* a);
/* Partial rows per group stf_igemm writes into bnr->partial for these args. */
int stf_igemm_bnr_tiles(const stf_igemm_args* a);
/* Device kernel (template instance, as rocprofv3 names it) these args will run;
 * static thread-local string, for per-kernel timers and profile cross-checks. */
const char* stf_igemm_kernel_name(const stf_igemm_args* a);
/* Conv2d 3x3/1x1/strided forward with fused bias + BatchNorm partial statistics
 *   replaces nn.Conv2d in conv_block  (src/unet.py:12,15), ResidualConvBlock
 *   (src/stf_lstm_unet.py:13,16,23), ResNet-34 convs (src/stf_lstm_unet.py:108-114),
 *   out_conv/fusion/pk_fusion 1x1 (src/unet.py:37, src/stf_lstm_unet.py:46,118-121);
 * Conv2d input gradient (transposed gather) for the same layers;
 * ConvTranspose2d(k=2,s=2) forward with scatter epilogue straight into the
 *   concat buffer  (src/unet.py:28-34,47-54) and its input gradient (stride-2 2x2 gather);
 * ConvTranspose2d(k=3,s=2,p=1,op=1) forward (src/stf_lstm_unet.py:43,135). */
int stf_igemm(const stf_igemm_args* a, stf_stream_t stream);

typedef struct stf_wgrad_args {
  stf_conv_geom g;     /* forward geometry; transposed must be 0                */
  const void* dy;      /* bf16 [N*Hd*Wd][dy_cstride], first used channel        */
  int dy_cstride;
  int Nout;            /* columns of dy used; multiple of 8                     */
  const void* x;       /* bf16 source (gathered as in stf_conv_geom)            */
  float* ws;           /* workspace [splits][Nout][R*S*Cs] fp32                 */
  int splits;          /* pixel splits (from stf_wgrad_plan)                    */
  int grid_blocks;     /* workgroups the pixel split aims at (0: two per CU).   */
                       /* A weight gradient running on a side stream beside the */
                       /* dgrad / BatchNorm chain asks for one per CU, so the   */
                       /* chain's kernels still find registers on every CU (ABI v7) */
} stf_wgrad_args;

/* Choose splits and report workspace bytes for a weight-gradient pass. */
int stf_wgrad_plan(const stf_wgrad_args* a, int* splits, size_t* ws_bytes);
/* dW[n][r][s][c] partials = sum over pixels dy[m][n] * x[gather(m,r,s)][c]
 *   replaces the weight gradient of every Conv2d/ConvTranspose2d above. */
int stf_wgrad(const stf_wgrad_args* a, stf_stream_t stream);
/* Device kernel stf_wgrad runs for these args (see stf_igemm_kernel_name). */
const char* stf_wgrad_kernel_name(const stf_wgrad_args* a);
/* Sum `splits` slabs into out[Nout][Cs][R][S] (PyTorch Conv2d weight layout;
 * for ConvTranspose2d pass Nout=Cin, Cs=Cout and get [Cin][Cout][R][S]).
 * Partial-slab arguments of this and the *_finalize / channel-sum functions are
 * scratch: they are reduced in place (fixed order) and left clobbered. */
int stf_wgrad_reduce(float* ws, int splits, int Nout, int R, int S, int Cs,
                     float* out, stf_stream_t stream);

/* Per-channel column sums of a bf16 NHWC tensor (bias gradients of ConvT /
 * 1x1 convs, src/unet.py:28-37).  partial: [ceil(M/256)][C] scratch. */
int stf_channel_sum(const void* x, int x_cstride, int M, int C, float* partial,
                    float* out, stf_stream_t stream);
/* The same column sums taken from the BatchNorm statistics rows [tiles][2][Nout] that an
 * stf_igemm with `stats` produced (the per-tile sums of its stored outputs): out[c] = sum over
 * tiles of the sum half's column c0 + c, c < C.  The UNet's ConvT bias gradients come from the
 * statistics of the dgrad that writes the concat gradient, instead of another pass over it
 * (ABI v17). */
int stf_stat_sums(const float* stats, int tiles, int Nout, int c0, int C, float* out, stf_stream_t stream);

/* ---------------------------------------------------------------- BatchNorm2d
 * Training-mode BatchNorm2d (+ReLU) (src/unet.py:13-17; src/stf_lstm_unet.py:14-17,
 * ResNet bn1/bn2/downsample.1): batch mean, biased variance for normalisation,
 * unbiased variance into running_var, momentum 0.1, eps 1e-5 (torch defaults).
 * `groups` splits the N images into equal statistic groups (per-time-step BN of
 * the batched STF encoder, src/stf_lstm_unet.py:168-186): every group gets its
 * own mean/invstd/scale/shift ([groups][C]) and running stats advance once per
 * group, in order.  UNet passes groups = 1.  Partial-slab inputs are consumed. */
/* stats: [groups][tiles][2][C] from stf_igemm (tiles = per group), or NULL for
 * eval mode (normalise with running_mean/var, no update). */
int stf_bn_finalize(float* stats, int tiles, int groups, int C, int64_t M,
                    const float* gamma, const float* beta, float momentum, float eps,
                    float* running_mean, float* running_var, float* mean, float* invstd,
                    float* scale, float* shift, stf_stream_t stream);
/* Deferred running-statistics update of grouped BatchNorms (groups > 1): a
 * stf_bn_finalize call with running_mean = running_var = NULL leaves every
 * group's (mean, biased var) parked in row 0 of that group's stats slab; one
 * stf_bn_running_batch launch then advances each BatchNorm's running stats
 * group by group, in order (same arithmetic as the in-call update).  descs is a
 * HOST array; the stats slabs must stay alive until the launch has run. */
typedef struct stf_bn_run_desc {
  const float* stats;          /* [groups][tiles][2][C], parked by stf_bn_finalize */
  float* running_mean;
  float* running_var;
  int64_t Mg;                  /* rows per group */
  int tiles, groups, C;
  float momentum;
} stf_bn_run_desc;
int stf_bn_running_batch(const stf_bn_run_desc* descs, int count, stf_stream_t stream);
/* out = act(y*scale + shift [+ res | + res*res_scale + res_shift]) into a
 * channel slice.  Residual: identity shortcut (res_scale NULL) or a BN'd
 * downsample branch (ResNet BasicBlock src/stf_lstm_unet.py:108-114,
 * ResidualConvBlock :29-35).  Optional fused 2x2 max pool (MaxPool2d(2),
 * src/unet.py:25,41-45) into `pooled` [N][H/2][W/2][C] (no residual). */
int stf_bn_act(const void* y, int y_cstride, int N, int H, int W, int C, int groups,
               const float* scale, const float* shift, int relu, const void* res,
               int res_cstride, const float* res_scale, const float* res_shift, void* out,
               int out_cstride, void* pooled, stf_stream_t stream);
/* Backward of BN(+ReLU)(+2x2 max pool):  da = dz + maxpool_bwd(dpool) (either
 * may be NULL), g = da masked by mask_mode (0 none, 1 ReLU recomputed from
 * y*scale+shift, 2 mask_src > 0: ReLU after a residual add), written to g_out
 * [M][C]; partial [groups][tiles][2][C] = (sum g, sum g*xhat), tiles from
 * stf_bn_bwd_tiles.  C / 8 must divide 256.  Without dpool a statistics group
 * must hold fewer than 2^31 16-byte units ((M / groups) * (C / 8); a 32 GiB
 * tensor per group): STF_EINVAL otherwise, nothing is launched. */
int stf_bn_bwd_tiles(int N, int H, int W, int C, int groups, int pooled);
int stf_bn_bwd_reduce(const void* dz, int dz_cstride, const void* dpool, const void* y,
                      int y_cstride, int N, int H, int W, int C, int groups,
                      const float* scale, const float* shift, const float* mean,
                      const float* invstd, int mask_mode, const void* mask_src,
                      int mask_cstride, void* g_out, float* partial, stf_stream_t stream);
/* (g_out may be NULL without dpool: the masked gradient is then not stored and
 * stf_bn_bwd_apply recomputes the mask.) */
/* dgamma, dbeta (summed over groups) and coef [groups][3][C] of dy = A*g + B*y + C. */
int stf_bn_bwd_finalize(float* partial, int tiles, int groups, int C, int64_t M,
                        const float* gamma, const float* mean, const float* invstd,
                        float* dgamma, float* dbeta, float* coef, stf_stream_t stream);
/* Deferred dgamma/dbeta of grouped BatchNorm backwards: stf_bn_bwd_finalize with
 * dgamma = dbeta = NULL and groups > 1 leaves each group's (sum g, sum g*xhat)
 * parked in row 0 of that group's partial slab; stf_bn_groupsum_batch sums them
 * over the groups for many BatchNorms in one launch (descs: HOST array). */
typedef struct stf_bn_gsum_desc {
  const float* partial;        /* [groups][tiles][2][C] */
  float* dgamma;
  float* dbeta;
  int tiles, groups, C;
} stf_bn_gsum_desc;
int stf_bn_groupsum_batch(const stf_bn_gsum_desc* descs, int count, stf_stream_t stream);
/* dy = A*g' + B*y + C (bf16, dy_cstride; may alias g when dense).  g' = g, or
 * with mask_scale/mask_shift ([groups][C], the forward BN affine) the ReLU mask
 * recomputed from y: g' = g where y*scale+shift > 0 else 0 -- then g is the raw
 * incoming gradient (any channel stride) and stf_bn_bwd_reduce ran with
 * g_out = NULL.  Optional per-tile column sums of dy for the bias of the
 * producing conv (bias_partial [stf_bn_bwd_apply_tiles][C]) reduced into dbias.
 * C / 8 must divide 256 and a statistics group must hold fewer than 2^31
 * 16-byte units ((M / groups) * (C / 8)): STF_EINVAL otherwise, nothing is launched.
 * With bias_partial every group writes at least one row, so groups must not exceed
 * stf_bn_bwd_apply_tiles(M, C) (a tensor of fewer than groups x 256 units): STF_EINVAL. */
int stf_bn_bwd_apply_tiles(int64_t M, int C);
int stf_bn_bwd_apply(const void* g, int g_cstride, const void* y, int y_cstride, int64_t M,
                     int C, int groups, const float* mask_scale, const float* mask_shift,
                     const float* coef, void* dy, int dy_cstride, float* bias_partial,
                     float* dbias, stf_stream_t stream);

/* ---------------------------------------------------------------- head + loss
 * UNet OutConv fused with the last BN+ReLU (src/unet.py:16-17,37,56):
 * logits[b][k][h][w] (fp32 NCHW, the {"out": ...} tensor) =
 * bias[k] + sum_c relu(y*scale+shift)[c] * W[k][c]. */
int stf_head_fwd(const void* y, int N, int H, int W, int C, const float* scale,
                 const float* shift, const float* w, const float* bias, int classes,
                 float* logits, stf_stream_t stream);
/* Backward of the head and the BN+ReLU it absorbed: g = (dlogits . W) * relu',
 * partial (sum g, sum g*xhat) as stf_bn_bwd_reduce, head dW/db partials in
 * head_partial [(tiles+1)][classes*(C+1)] (last row = the reduction) copied
 * into dw (classes*C) and db (classes).  tiles = stf_head_tiles(N, H, W, C). */
int stf_head_bwd(const float* dlogits, const void* y, int N, int H, int W, int C,
                 const float* scale, const float* shift, const float* mean,
                 const float* invstd, const float* w, int classes, void* g_out,
                 float* bn_partial, float* head_partial, float* dw, float* db,
                 stf_stream_t stream);
int stf_head_tiles(int N, int H, int W, int C);

/* criterion (train_utils/train_and_eval.py:299-313) = cross_entropy +
 * multiclass Dice loss on softmax (train_utils/dice_coefficient_loss.py:5-55),
 * branch-free empty-set rule.  terms: stf_loss_scratch_floats() floats; its
 * first N*classes*3 + 1 hold (sum p*t, sum p, sum t) per (image, class) and the
 * CE sum after stf_loss_fwd; loss: device scalar.  This is the formula below with w = 1, m = 1 and
 * Dice on (the reference's default configuration). */
int stf_loss_scratch_floats(int N, int classes);
int stf_loss_fwd(const float* logits, const int64_t* target, int N, int H, int W,
                 int classes, float* terms, float* loss, stf_stream_t stream);
int stf_loss_bwd(const float* logits, const int64_t* target, int N, int H, int W,
                 int classes, const float* terms, const float* grad_out, float* dlogits,
                 stf_stream_t stream);
/* The criterion above with the reference's options (additive: the ABI version stays 17); terms and
 * loss as there, with stf_loss_opt_scratch_floats() floats and N*classes*3 + 2 leading ones: Wsum =
 * sum m w[t] follows the (now weighted) CE sum.  class_weight: [classes] fp32 or NULL (all ones);
 * ignore_index < 0: none, otherwise pixels whose target equals it are masked (m = 0); dice: 0 drops
 * the Dice term.
 *   CE   = sum m w[t] (-log p_t) / Wsum                (F.cross_entropy(weight, ignore_index))
 *   Dice = per (image, class) over the pixels with m = 1; an image with none has D = 1; the class
 *          weights do not enter it
 *   loss = CE + (dice ? 1 - mean_k mean_b D : 0)
 * The backward stores an exact 0 at masked pixels (dlogits may arrive uninitialised).  A batch
 * with every pixel masked has Wsum = 0: the loss is NaN, as F.cross_entropy gives.  A target
 * outside [0, classes) other than ignore_index weighs 0 in CE and counts in no class.
 * STF_EINVAL (nothing launched) for classes outside 1..4 or 0 <= ignore_index < classes.
 * Both families: deterministic (fixed summation order, no atomics), no host read-back. */
int stf_loss_opt_scratch_floats(int N, int classes);
int stf_loss_opt_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                     const float* class_weight, int ignore_index, int dice, float* terms,
                     float* loss, stf_stream_t stream);
int stf_loss_opt_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                     const float* class_weight, int ignore_index, int dice, const float* terms,
                     const float* grad_out, float* dlogits, stf_stream_t stream);
/* Head and criterion for 1..16 classes (additive: the ABI version stays 17).  Arguments, layouts
 * and formulas are those of stf_head_fwd / stf_head_bwd and of stf_loss_opt_fwd / stf_loss_opt_bwd
 * (stf_loss_mc_scratch_floats = N*classes*3 + 2 + N*64*(3*classes + 2), 0 for classes outside
 * 1..16); the kernels take the class count at run time, keep the head's weights in LDS and spill
 * nothing.  The entry points above stay as they are for classes <= 4 (their results are pinned bit
 * for bit); the Python package sends classes >= 5 here.  STF_EINVAL (nothing launched) for classes
 * outside 1..16, 0 <= ignore_index < classes, a C that stf_head_fwd refuses, N > 65535 images in
 * the criterion, a NULL required pointer (class_weight and grad_out may be NULL).  Deterministic. */
int stf_head_mc_fwd(const void* y, int N, int H, int W, int C, const float* scale,
                    const float* shift, const float* w, const float* bias, int classes,
                    float* logits, stf_stream_t stream);
int stf_head_mc_bwd(const float* dlogits, const void* y, int N, int H, int W, int C,
                    const float* scale, const float* shift, const float* mean,
                    const float* invstd, const float* w, int classes, void* g_out,
                    float* bn_partial, float* head_partial, float* dw, float* db,
                    stf_stream_t stream);
int stf_loss_mc_scratch_floats(int N, int classes);
int stf_loss_mc_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                    const float* class_weight, int ignore_index, int dice, float* terms,
                    float* loss, stf_stream_t stream);
int stf_loss_mc_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                    const float* class_weight, int ignore_index, int dice, const float* terms,
                    const float* grad_out, float* dlogits, stf_stream_t stream);
/* The option criterion with a focal cross-entropy and a Tversky overlap, classes in 1..16 (additive:
 * the ABI version stays 17; csrc/loss.hip, FT=true).  Arguments, terms layout and scratch size are those
 * of stf_loss_mc_fwd / stf_loss_mc_bwd (stf_loss_ft_scratch_floats == stf_loss_mc_scratch_floats, 0
 * for classes outside 1..16), with three floats after dice.  With q = p_t and nll = -log q:
 *   CE_f = sum m w[t] (1-q)^focal_gamma nll / Wsum      (Wsum = sum m w[t]; focal_gamma = 0 is CE)
 *   FP = sum m p - I, FN = sum m t - I                  per (image, class)
 *   D    = (2I + eps) / (2I + 2 tversky_alpha FP + 2 tversky_beta FN + eps)
 *                                                       (alpha = beta = 1/2 is Dice; D = 1 for an image
 *                                                        with every pixel masked)
 *   loss = CE_f + (dice ? 1 - mean_k mean_b D : 0)
 * 1-q is formed from the other classes' exponentials, so it keeps its precision where q rounds to 1;
 * where it is exactly 0 and focal_gamma > 0 the pixel's cross-entropy term and gradient are 0.
 * Masked pixels get a stored 0, an all-masked batch a NaN loss, as above.  STF_EINVAL (nothing
 * launched) for the refusals of stf_loss_mc_fwd / stf_loss_mc_bwd, a focal_gamma that is negative or
 * not finite, a tversky_alpha or tversky_beta that is negative or not finite, or both 0 (also with
 * dice == 0).  Deterministic (fixed summation order, no atomics), no host read-back. */
int stf_loss_ft_scratch_floats(int N, int classes);
int stf_loss_ft_fwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                    const float* class_weight, int ignore_index, int dice, float focal_gamma,
                    float tversky_alpha, float tversky_beta, float* terms, float* loss,
                    stf_stream_t stream);
int stf_loss_ft_bwd(const float* logits, const int64_t* target, int N, int H, int W, int classes,
                    const float* class_weight, int ignore_index, int dice, float focal_gamma,
                    float tversky_alpha, float tversky_beta, const float* terms,
                    const float* grad_out, float* dlogits, stf_stream_t stream);

/* ---------------------------------------------------------------- optimizer
 * torch.optim.AdamW(lr, betas, eps, weight_decay) (train.py:230-237) over one
 * flat fp32 parameter buffer. */
int stf_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr,
              float beta1, float beta2, float eps, float weight_decay, float bc1,
              float bc2, stf_stream_t stream);
/* Graph-capturable AdamW: hyper = DEVICE {lr, step} (step = this update's count,
 * already incremented); bias corrections computed on the device exactly as the host
 * computes them for stf_adamw. */
int stf_adamw_dev(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper,
                  float beta1, float beta2, float eps, float weight_decay, stf_stream_t stream);
/* AdamW under torch.amp.GradScaler without a host sync (the optimizer advertises
 * _step_supports_amp_scaling, as torch's fused AdamW does, which the reference builds with
 * fused=True, train.py:230-237): grad_scale = DEVICE scale the gradients carry (NULL:
 * already unscaled; multiplied by 1/scale in fp32 = GradScaler.unscale_'s arithmetic),
 * found_inf = DEVICE flag, != 0 skips the update and leaves hyper[1] (the step count)
 * unchanged; otherwise hyper[1] += 1 and the update is stf_adamw_dev's. */
int stf_adamw_amp(float* p, const float* g, float* m, float* v, int64_t n, float* hyper,
                  const float* grad_scale, const float* found_inf, float beta1, float beta2, float eps,
                  float weight_decay, stf_stream_t stream);

/* Gradient clipping by the global L2 norm, on the flat fp32 gradient buffer
 * (torch.nn.utils.clip_grad_norm_, norm_type 2).  A segment is `len` elements at element
 * offset `off` of the buffer: off >= 0 and a multiple of 4 (FlatParams alignment; the buffer
 * itself 16-B aligned), len >= 0 and arbitrary.  Only elements inside a segment are read or
 * written: the padding between parameters and the slices of frozen parameters stay out.
 * Every call takes the table twice: `segs` in DEVICE memory, which the kernels read, and
 * `segs_host`, the same `count` entries in host memory, which the call checks and sizes its
 * grid from before it returns (build both once per parameter set). */
typedef struct stf_seg {
  int64_t off;
  int64_t len;
} stf_seg;
/* out[0] = the norm of the segments' elements times 1 / *grad_scale (DEVICE; NULL: already
 *          unscaled), i.e. the norm of the unscaled gradient;
 * out[1] = the clip coefficient min(1, max_norm / (out[0] + 1e-6)), torch's fp32 arithmetic;
 * out[2] = 1.0 if out[0] is not finite, else 0.0;  out[3] = 0 (reserved).
 * Two launches: a streaming pass (one row of `partial` per workgroup; a fixed assignment of
 * elements to workgroups, no atomics) and a one-workgroup fold in row order, so `out` and
 * `partial` are the same bits from run to run.  Squares and sums are in double: no fp32 input
 * overflows or flushes the sum, whatever loss scale it carries, and out[0] is within 1 ulp of
 * the fp32 rounding of the exact norm.  partial = stf_grad_norm_rows(n) doubles, n >= the
 * table's total length (host-only query; never more than 2048).
 * STF_EINVAL, nothing launched: a NULL pointer other than grad_scale, count < 1, a negative
 * length, an offset that is negative or not a multiple of 4, max_norm NaN or <= 0. */
int stf_grad_norm_rows(int64_t n);
int stf_grad_norm(const float* buf, const stf_seg* segs, const stf_seg* segs_host, int count,
                  const float* grad_scale, float max_norm, double* partial, float* out,
                  stf_stream_t stream);
/* buf[e] *= clip[1] for every element e of the segments, in place, one launch (clip = the out
 * of stf_grad_norm; a coefficient of exactly 1 writes nothing).  Same argument checks. */
int stf_grad_scale(float* buf, const stf_seg* segs, const stf_seg* segs_host, int count,
                   const float* clip, stf_stream_t stream);
/* stf_adamw_amp with the clip folded into the update: clip = the out of stf_grad_norm over
 * this gradient.  The gradient enters as (g * (1 / *grad_scale)) * clip[1] -- two fp32
 * multiplications in this order (the first one only when grad_scale is given), the same bits
 * as stf_grad_scale on an unscaled buffer followed by the unclipped update; g itself is not
 * modified.  The update is skipped, and hyper[1] left unchanged, when *found_inf != 0
 * (found_inf may be NULL) OR clip[2] != 0: a step whose gradient norm is not finite is
 * skipped, not applied as NaN -- a deliberate difference from torch's
 * clip_grad_norm_(error_if_nonfinite=False) followed by step().  With clip = {., 1, 0, 0} and
 * no scale the update is stf_adamw_dev's bit for bit (the same kernel body). */
int stf_adamw_clip(float* p, const float* g, float* m, float* v, int64_t n, float* hyper,
                   const float* grad_scale, const float* found_inf, const float* clip, float beta1,
                   float beta2, float eps, float weight_decay, stf_stream_t stream);

/* Exponential moving average of the weights in one fp32 shadow buffer (16-B aligned).  A segment
 * is `len` fp32 elements of the model at `model` (4-B aligned is enough: a 16-B aligned pointer
 * moves as float4, any other element by element) and their place in the shadow, element offset
 * `off`: off >= 0 and a multiple of 4, len >= 0 (0: skipped).  Segments overlap neither in the
 * model nor in the shadow.  Only elements inside a segment are read or written, on either side.
 * The table is taken twice, like stf_grad_norm's: `segs` in DEVICE memory for the kernel and
 * `segs_host`, the same `count` entries on the host, for the checks and the grid. */
typedef struct stf_ema_seg {
  float* model;
  int64_t off;
  int64_t len;
} stf_ema_seg;
/* shadow = shadow + w * (model - shadow) for every element of every segment, in fp32 (the
 * difference rounds once, the multiply-add once), ONE launch for the whole table.  w == 1 writes
 * the model's bits, w == 0 leaves the shadow's bits; a fixed assignment of elements to
 * workgroups, no atomics.
 * STF_EINVAL, nothing launched: a NULL pointer, count < 1, shadow not 16-B aligned, a negative
 * off or len, off % 4 != 0, a NULL (or not 4-B aligned) model in a segment with len > 0, w NaN
 * or outside [0, 1]. */
int stf_ema_update(float* shadow, const stf_ema_seg* segs, const stf_ema_seg* segs_host, int count,
                   float w, stf_stream_t stream);
/* Exchanges model and shadow element by element as raw bits (-0.0 and NaN payloads survive), in
 * place, ONE launch; twice restores both sides.  Same argument checks. */
int stf_ema_swap(float* shadow, const stf_ema_seg* segs, const stf_ema_seg* segs_host, int count,
                 stf_stream_t stream);

/* ---------------------------------------------------------------- layout
 * x [N][C][H][W] fp32 -> NHWC bf16 with Cpad (>= C, multiple of 8) channels,
 * zero-filled (preprocess_input output, train_and_eval.py:9-22). */
int stf_pack_input(const float* x, int N, int C, int H, int W, int Cpad, void* out,
                   stf_stream_t stream);
/* fp32 weights -> bf16 GEMM rows.
 *  mode 0: Conv2d w[Co][Ci][R][S]       -> [Co][R][S][Cipad]   (forward)
 *  mode 1: Conv2d w[Co][Ci][R][S]       -> [Ci][R'][S'][Co]    (dgrad, no flip:
 *          the transposed gather indexes taps directly)
 *  mode 2: ConvT  w[Ci][Co][R][S]       -> [(r*S+s)*Co+co][Ci] (scatter2x2 fwd)
 *  mode 3: ConvT  w[Ci][Co][R][S]       -> [Ci][R][S][Co]      (ConvT dgrad)
 *  mode 4: ConvT  w[Ci][Co][R][S]       -> [Co][R][S][Ci]      (ConvT fwd gather)
 *  mode 5: Conv2d w[Co][Ci][R][S]       -> [Ci][R-1-r][S-1-s][Co] (stride-1 dgrad as a
 *          forward gather with pad' = R-1-pad) */
int stf_pack_weight(const float* w, int d0, int d1, int R, int S, int mode, int cpad,
                    void* out, stf_stream_t stream);
/* Many stf_pack_weight jobs in one launch.  descs: DEVICE array of count
 * descriptors (same fields and modes as stf_pack_weight); max_elems = the
 * largest packed element count among them (sizes the grid). */
typedef struct stf_pack_desc {
  const float* w;
  void* out;
  int d0, d1, R, S, mode, cpad;
} stf_pack_desc;
int stf_pack_weights(const stf_pack_desc* descs, int count, int64_t max_elems, stf_stream_t stream);
/* Same job through LDS-tiled transposes (whole source rows read, 16-B output
 * chunks written).  stf_pack_tiles(d0,d1,R,S,mode,cpad) = the tile count of one
 * descriptor, or -1 when the tiled kernel cannot take it (R*S > 9, or output rows
 * not a multiple of 8 elements); max_tiles = the largest count in the list (every
 * descriptor must have one >= 0).  ABI v5. */
int stf_pack_tiles(int d0, int d1, int R, int S, int mode, int cpad);
int stf_pack_weights_tiled(const stf_pack_desc* descs, int count, int max_tiles, stf_stream_t stream);

/* ---------------------------------------------------------------- STF-LSTM-UNet
 * x [B][Ttot][C][H][W] fp32 -> t-major NHWC bf16 [T*B][H][W][Cpad]: frame t of
 * sample b is image t*B+b; channels [0,C) the frame, [C,C+P) the P PK maps
 * x[b][T+p][0] (src/stf_lstm_unet.py:146-156,172-174), rest zero. */
int stf_pack_sequence(const float* x, int B, int Ttot, int C, int H, int W, int T, int P,
                      int Cpad, void* out, stf_stream_t stream);

/* Stem im2col (replaces the padded-channel input of the 7x7/s2 stem, reference
 * src/stf_lstm_unet.py:108,177): x as for stf_pack_sequence -> bf16
 * [T*B][Ho][Wo][Kpad], column k = ci*KS*KS + r*KS + s (PyTorch weight order),
 * zero padded; the stem conv is then a 1x1 GEMM over Kpad >= (C+P)*KS*KS columns. */
int stf_stem_im2col(const float* x, int B, int Ttot, int C, int H, int W, int T, int P, int KS,
                    int stride, int pad, int Kpad, void* out, stf_stream_t stream);
/* The same stem conv without the im2col tensor (ABI v15): x [B][Ttot][1][H][W] fp32 (frames 0..T-1,
 * no PK maps) -> y NHWC bf16 [T*B][Ho][Wo][64] (Ho = (H-1)/2+1), w = the 64 x 64 bf16 rows the GEMM
 * path packs (column k = r*7 + s, zero for k >= 49).  Bit-identical outputs to the im2col + 1x1 GEMM.
 * stats (NULL: none): BatchNorm partial rows [T][grid][2][64] (sum, sum of squares of the stored
 * bf16 values; grid = stf_stem_conv7_grid(B, T, H, W) rows per time step) for stf_bn_finalize. */
int stf_stem_conv7_grid(int B, int T, int H, int W);
int stf_stem_conv7(const float* x, int B, int Ttot, int H, int W, int T, const void* w, void* y, float* stats,
                   stf_stream_t stream);
/* Its weight gradient without the im2col tensor: dy NHWC bf16 [T*B][Ho][Wo][64] (the stem output's
 * gradient) -> fp32 partial slabs ws [grid][64][64] (dy channel x column k = r*7 + s; columns >= 49
 * zero; grid = stf_stem_conv7_grid(...)), folded with stf_wgrad_reduce(ws, grid, 64, 1, 1, 64, ..). */
int stf_stem_wgrad7(const float* x, int B, int Ttot, int H, int W, int T, const void* dy, float* ws,
                    stf_stream_t stream);
/* Input gradient of that stem conv (7x7/s2/p3, Cf input channels; what autograd returns for the
 * input sequence, src/stf_lstm_unet.py:139-256): dy [T*B][Ho][Wo][64] 16-bit (frame t*B + b), w the
 * fp32 conv1 weight [64][Cf][7][7] -> dx fp32 in the input's layout [B][Ttot][Cf][H][W], frames
 * t < T written (t >= T, the PK maps, untouched).  ABI v16. */
int stf_stem_dgrad7(const void* dy, const float* w, int B, int Ttot, int Cf, int H, int W, int T, float* dx,
                    stf_stream_t stream);
/* MaxPool2d(3, 2, 1) of the ResNet stem (src/stf_lstm_unet.py:110,180), NHWC bf16.
 * argmax (uint8 [N][Ho][Wo][C], NULL in eval) records each window's first maximum
 * (index dy*3+dx, torch's tie rule); backward gathers dout over the <= 4 windows
 * whose recorded maximum is the pixel. */
int stf_maxpool3s2_fwd(const void* x, int N, int H, int W, int C, void* out, void* argmax,
                       stf_stream_t stream);
int stf_maxpool3s2_bwd(const void* argmax, const void* dout, int N, int H, int W, int C, void* dx,
                       stf_stream_t stream);
/* The stem's BatchNorm + ReLU and that max pool in one pass (src/stf_lstm_unet.py:178-180):
 * pooled out and argmax exactly as stf_bn_act (scale / shift of group n / (N / groups), ReLU,
 * 16-bit rounding) followed by stf_maxpool3s2_fwd, without writing the activation.  ABI v11. */
int stf_bn_act_maxpool3s2(const void* y, int N, int H, int W, int C, int groups, const float* scale,
                          const float* shift, void* out, void* argmax, stf_stream_t stream);
/* The stem BatchNorm's backward through that max pool: the gradient of each pixel is gathered
 * from the pooled gradient dout [N][Ho][Wo][C] over the <= 4 windows whose recorded argmax it
 * is (rounded to 16 bits, as stf_maxpool3s2_bwd stores it), masked by the ReLU recomputed from
 * y; reduce -> partials as stf_bn_bwd_reduce (then stf_bn_bwd_finalize), apply -> dy, without
 * the full-size d(activation) tensor.  Same values as stf_maxpool3s2_bwd + stf_bn_bwd_reduce
 * (mask_mode 1) + stf_bn_bwd_apply.  ABI v11. */
int stf_bn_bwd_reduce_pool3(const void* argmax, const void* dout, const void* y, int N, int H, int W, int C,
                            int groups, const float* scale, const float* shift, const float* mean,
                            const float* invstd, float* partial, stf_stream_t stream);
int stf_bn_bwd_apply_pool3(const void* argmax, const void* dout, const void* y, int N, int H, int W, int C,
                           int groups, const float* scale, const float* shift, const float* coef, void* dy,
                           stf_stream_t stream);
/* nn.LSTM(C, C) weights -> gate-interleaved GEMM operands: wcat [4C][2C] (row
 * 4c+q = torch row q*C+c of [W_ih | W_hh]), wcat_t [2C][4C], bias = b_ih + b_hh
 * interleaved (src/stf_lstm_unet.py:124-127).  C in {16, 32, ..., 512} (STF_EINVAL otherwise). */
int stf_lstm_pack(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                  int C, void* wcat, void* wcat_t, float* bias, stf_stream_t stream);
/* The whole forward sequence of nn.LSTM(C, C) in one launch (src/stf_lstm_unet.py:214-242):
 * lbuf = [T][P][2C] 16-bit rows of step t = [x_t | h_{t-1}] (x_t given, the h slots of
 * steps 1..T-1 are written here, step 0's is ignored: h_{-1} = 0), wcat / bias from
 * stf_lstm_pack, c_out = [T][P][C] fp32 cell states, h_{T-1} -> h_last (stride h_cstride).
 * Same values as T launches of stf_igemm with the LSTM cell epilogue.  C = 64 only
 * (stf_lstm_seq_supported); 16-B aligned wcat / lbuf. */
int stf_lstm_seq_fwd(const void* wcat, const float* bias, void* lbuf, int P, int T, int C, float* c_out,
                     void* h_last, int h_cstride, stf_stream_t stream);
int stf_lstm_seq_supported(int C);
/* The whole backward (BPTT) of that sequence in one launch: recomputes every step's gates
 * from lbuf (as the forward computed them), runs the cell backward and the input-gradient
 * GEMM; dgates = [T][P][4C] 16-bit pre-activation gate gradients (for the weight gradient
 * afterwards), dx = rows [T][P] of stride dx_cstride receiving dL/dx_t in channels [0, C);
 * dh_last = dL/dh_{T-1} (stride dh_cstride).  Same values as the per-step path (stf_igemm
 * with the LSTM backward epilogue + the dgates x W GEMM).  C = 64 only; 16-B alignment.
 * dx == NULL (additive: the ABI version stays 17; it was STF_EINVAL before): nothing consumes
 * the input gradient (everything upstream of the LSTM is frozen).  Only dgates is written:
 * per step the launch computes just dh_{t-1} = dgates_t W_hh, with every dh element accumulated
 * in the same order as with dx, so dgates is bit-identical; dx_cstride is ignored. */
int stf_lstm_seq_bwd(const void* wcat, const void* wcat_t, const float* bias, const void* lbuf, int P, int T,
                     int C, const float* c_all, const void* dh_last, int dh_cstride, void* dgates, void* dx,
                     int dx_cstride, stf_stream_t stream);
/* Whole-sequence forward for C = 128 / 256 / 512 (stf_lstm_coop_supported) in ONE persistent
 * launch: the 4C gate rows are cut into C/32 slices of 128; the C/32 workgroups of a 64-pixel
 * block keep their weight slice in registers and hand h_t to each other through lbuf inside
 * the launch (agent-scope counters, write-through stores, an acquire per step).  Same
 * arguments, layout and values (bit for bit) as stf_lstm_seq_fwd / the per-step path, plus
 * `sync`: a caller-owned device buffer of stf_lstm_coop_sync_bytes(P, T) bytes (16-B aligned;
 * zeroed on the stream by the call itself; its last word is an error flag: nonzero = a step's
 * hand-off timed out, after which the launch drains at once with wrong values).  spin_limit: polls
 * before a hand-off gives up (0 = the default, ~4 s; 0xFFFFFFFF = every hand-off reports a timeout
 * at once: the error path, for tests).  ABI v12. */
size_t stf_lstm_coop_sync_bytes(int P, int T);
int stf_lstm_coop_supported(int C);
int stf_lstm_coop_fwd(const void* wcat, const float* bias, void* lbuf, int P, int T, int C, float* c_out,
                      void* h_last, int h_cstride, float* gates, unsigned* sync, int max_wg, unsigned spin_limit,
                      stf_stream_t stream);
/* gates (or NULL): [T][P][4C] fp32 activated gates (i, f, g, o interleaved per channel), kept
 * for the per-step backward's stf_lstm_cell_bwd (no gate recompute).  max_wg: at most this many
 * workgroups (one per CU; 0 = one per CU of the device) -- a launch on a side stream beside
 * other work leaves the rest of the chip to it (a group of C/32 must fit). */
/* sticky |= the error word of the launch that used `sync` (stream-ordered, no host sync): a program
 * keeps one sticky device word across steps and reads it back at a step boundary. */
int stf_lstm_coop_error(const unsigned* sync, int P, int T, unsigned* sticky, stf_stream_t stream);
/* The DecoderBlock's size fallback (src/stf_lstm_unet.py:56-57): F.interpolate(mode="bilinear",
 * align_corners=True) of x [N][H][W] (C channels, stride x_cstride, 16-bit NHWC) to y [N][h][w]
 * (stride y_cstride; e.g. the concat slice), PyTorch's coordinate arithmetic; and its backward,
 * dx [N][H][W] = the gather of dy [N][h][w] (no atomics: each input pixel sums the output pixels
 * that read it, in a fixed order).  C % 8 == 0, strides % 8 == 0, 16-B aligned.  ABI v12. */
int stf_bilinear_ac_fwd(const void* x, int N, int H, int W, int C, int x_cstride, void* y, int h, int w,
                        int y_cstride, stf_stream_t stream);
int stf_bilinear_ac_bwd(const void* dy, int N, int h, int w, int C, int dy_cstride, void* dx, int H, int W,
                        int dx_cstride, stf_stream_t stream);
/* The PK maps' share of the input gradient (ABI v17): dy = T frames of B images [T*B][h][w] (t-major,
 * channels [0, 8) of stride dy_cstride, 16-bit NHWC), summed over the frames in fp32 at (h, w) and taken
 * back through the same resize; channels [0, P) (P <= 8) are ADDED to the fp32 out[b*out_bstride +
 * c*out_cstride + y*W + x] (x [B][T+P][1][H][W]: out = &x[0][T], strides (T+P)*H*W and H*W). */
int stf_bilinear_ac_bwd_tsum(const void* dy, int T, int B, int h, int w, int dy_cstride, int P, float* out,
                             int64_t out_bstride, int64_t out_cstride, int H, int W, stf_stream_t stream);
/* Full-resolution logits (ABI v17, additive): F.interpolate(mode="bilinear", align_corners=False,
 * size=(H, W)) of `planes` = N*K contiguous fp32 planes x [planes][h][w] (the NCHW logits of
 * stf_head_fwd and the loss kernels) to y [planes][H][W], PyTorch's fp32 coordinate arithmetic
 * (scale = in / out, src = scale (dst + 0.5) - 0.5 clamped at 0); and its backward, dx [planes][h][w]
 * = the gather of dy [planes][H][W] (no atomics: each source pixel sums the outputs that read it in
 * ascending (row, column) order, through the forward's own index function; dx is fully overwritten).
 * Upsampling only; equal sizes copy bit for bit.  STF_EINVAL without a launch for a NULL pointer, a
 * size < 1, H < h or W < w, or planes*H*W >= 2^31 (32-bit index math).  The coordinates are fp32, as
 * PyTorch's: exact index ranges for axes up to 2^22.  The same fp32 kernels in both libraries. */
int stf_resize_bilinear_fwd(const float* x, int planes, int h, int w, float* y, int H, int W, stf_stream_t stream);
int stf_resize_bilinear_bwd(const float* dy, int planes, int H, int W, float* dx, int h, int w, stf_stream_t stream);
/* dwcat [4C][2C] / dbias [4C] (interleaved) -> torch-layout dW_ih, dW_hh, db_ih, db_hh. */
int stf_lstm_unpack_grad(const float* dwcat, const float* dbias, int C, float* dw_ih,
                         float* dw_hh, float* db_ih, float* db_hh, stf_stream_t stream);
/* One BPTT step of the LSTM cell: from activated gates [M][4C], c_t, c_{t-1}
 * (NULL = 0), dh_t (bf16, stride) and dc from step t+1 (NULL = 0) -> dgates
 * (pre-activation, bf16 [M][4C] interleaved) and dc for step t-1 (may alias dc_in). */
int stf_lstm_cell_bwd(const float* gates, const float* c_t, const float* c_prev, const void* dh,
                      int dh_cstride, const float* dc_in, float* dc_out, void* dgates, int64_t M,
                      int C, stf_stream_t stream);
/* F.interpolate(pk, (h, w), bilinear, align_corners=True) of the PK maps of x,
 * written for every time step into channels [coff, coff+P) of dst
 * [T*B][h][w][dst_cstride] (PK fusion concat, src/stf_lstm_unet.py:189-200). */
int stf_pk_resize(const float* x, int B, int Ttot, int T, int P, int H, int W, int h, int w,
                  void* dst, int dst_cstride, int coff, stf_stream_t stream);

/* ---------------------------------------------------------------- evaluation
 * One pass over a batch's logits [B][K][HW] (fp32, NCHW) and int64 targets [B][HW]
 * (train_utils/train_and_eval.py:30-39, 80-118, 316-336): pred = first argmax over K;
 * confmat [K][K] += (target t in [0,K)) at [t][pred]; dice_counts [K][3] += per-class
 * (|P&T|, |P|, |T|) after multiplying pred and target by (target != ignore_index)
 * when ignore_index >= 0 (the reference's DiceCoefficient masking).  Both outputs are
 * int64 device arrays that ACCUMULATE (zero them first).  K <= 16. */
int stf_eval_counts(const float* logits, const int64_t* target, int B, int K, int64_t HW,
                    int64_t ignore_index, int64_t* confmat, int64_t* dice_counts, stf_stream_t stream);
/* The same pass with the Dice prediction taken from probs (same layout): the first argmax
 * of torch.softmax(logits, 1), which is what DiceCoefficient.update argmaxes
 * (train_and_eval.py:84-85) -- fp32 softmax can round logits that differ by less than an
 * ulp of exp() into a tie that argmax(logits) would not see.  The confusion matrix keeps
 * the logits' argmax (evaluate(), :331).  ABI v9. */
int stf_eval_counts_sm(const float* logits, const float* probs, const int64_t* target, int B, int K,
                       int64_t HW, int64_t ignore_index, int64_t* confmat, int64_t* dice_counts,
                       stf_stream_t stream);

/* ---------------------------------------------------------------- inference outputs
 * The per-image side of the reference's test.py:146-176: the predicted mask, the counts of
 * train_utils/visualize.py:9-50 (compute_metrics) and the overlay of test.py:52-82 /
 * train_utils/merge_tumor_images.py:94-120.  Additive to ABI v17; no entry point allocates.
 *
 * Mask of a batch of fp32 logits [B][K][HW] (NCHW), written as uint8 [B][HW], in one pass:
 *   rule 0 (argmax)   the class id of the first maximum over the K planes, a NaN wins
 *                     (torch.argmax; the prediction of the evaluation counts above);
 *   rule 1 (sigmoid)  1/(1+exp(-x)) > threshold in fp32 on the plane `channel` alone
 *                     (test.py:168-169): x = 0 at threshold 0.5 gives 0, NaN 0, +inf 1, -inf 0.
 * With target (int64 [B][HW], may be NULL) counts [B][3] int64 is OVERWRITTEN with the
 * per-image (|P&T|, |P|, |T|), P = mask > 0 and T = target > 0 (compute_metrics' target > 0.5:
 * a 255 pad is foreground); ignore >= 0 leaves the pixels whose target equals it out of all
 * three, a negative value none.  The counts are integers: any summation order is exact.
 * STF_EINVAL (nothing launched) for K outside 1..16, channel outside [0, K), a rule other than
 * 0 / 1, a NULL logits or mask, or a target without counts. */
int stf_predict_mask(const float* logits, const int64_t* target, int B, int K, int64_t HW, int rule,
                     int channel, float threshold, int64_t ignore, uint8_t* mask, int64_t* counts,
                     stf_stream_t stream);
/* The same pass on a plane of probabilities (rule "threshold"): mask = probs[:, channel] > threshold
 * with no sigmoid; a NaN compares false, +inf is over every finite threshold.  Everything else
 * (target, counts, ignore, the refusals) as stf_predict_mask.  An entry point of its own: rule
 * codes other than 0 / 1 stay refused there. */
int stf_predict_threshold(const float* probs, const int64_t* target, int B, int K, int64_t HW, int channel,
                          float threshold, int64_t ignore, uint8_t* mask, int64_t* counts, stf_stream_t stream);
/* Bytes of the scratch the overlay needs for B images of HW pixels (per-image min / max rows). */
size_t stf_predict_overlay_scratch_bytes(int B, int64_t HW);
/* The mask painted over one fp32 [H][W] plane per image, out uint8 [B][H][W][3].  Image b's
 * plane starts at frames + b * batch_stride (elements), so the shown frame of a [B,T,C,H,W]
 * input is passed as the view inputs[:,0,0] without a copy.  Two launches: per-image min / max
 * into scratch, then, every fp32 operation rounded on its own (no FMA) as numpy evaluates them,
 *   gray = (uint8)(((x - min) / (max - min + 1e-8f)) * 255.f)                      (test.py:71)
 *   painted pixels:  (uint8)(gray * (1 - alpha) + colour_c * alpha), c = 0, 1, 2   (:114-118)
 *   other pixels:    gray in all three channels
 * where a pixel is painted when (mask != 0) == paint; test.py:75-76 inverts its mask before
 * painting, which is paint = 0.  A constant image gives gray = 0.  The result for a plane with
 * non-finite pixels is undefined.  Channel c of out takes colour c: the reference hands
 * (c0, c1, c2) to cv2 as B, G, R.  STF_EINVAL (nothing launched) for alpha outside [0, 1], a
 * colour outside 0..255, paint other than 0 / 1, a negative stride or a NULL pointer. */
int stf_predict_overlay(const float* frames, int64_t batch_stride, const uint8_t* mask, int B, int H,
                        int W, int c0, int c1, int c2, float alpha, int paint, uint8_t* out,
                        void* scratch, stf_stream_t stream);

/* ---------------------------------------------------------------- mirror test-time augmentation
 * The work around the model forwards of mirror TTA (INTEGRATION.md 2.2 states the definition):
 * additive to ABI v17, fp32 only, one launch each, nothing allocated, no atomics (the same bits
 * from run to run).  flip: bit 0 reverses the last axis W, bit 1 the axis before it, H.
 *
 * y = x with W and / or H reversed in each of `planes` contiguous fp32 [H][W] planes (torch.flip,
 * bit for bit; flip 0 is a copy).  STF_EINVAL (nothing launched) for a NULL pointer, x == y, a size
 * below 1, flip outside 0..3 or planes * H * W >= 2^31. */
int stf_flip_planes(const float* x, int64_t planes, int H, int W, int flip, float* y, stf_stream_t stream);
/* One view's logits [B][K][H][W] (computed on the flipped input) -> probabilities per pixel, every
 * fp32 operation rounded on its own (no FMA):
 *   rule 0 (argmax)   m = max_k z, e_k = expf(z_k - m), s = e_0 + e_1 + ... in ascending k,
 *                     p_k = e_k / s: K planes;
 *   rule 1 (sigmoid)  1 / (1 + expf(-z[channel])), stf_predict_mask's arithmetic: one plane;
 * un-flipped (the value computed at (y, x) lands at (H-1-y if bit 1 else y, W-1-x if bit 0 else x))
 * and folded into acc [B][K or 1][H][W]: acc = p when first != 0 (acc may arrive uninitialised),
 * acc = acc + p otherwise; with views_if_last > 0 the stored value is that sum / (float)views_if_last
 * (one fp32 divide).  The K logit planes are read once, acc is read (unless first) and written once.
 * STF_EINVAL (nothing launched) for a NULL pointer, K outside 1..16, channel outside [0, K), a rule
 * other than 0 / 1, flip outside 0..3, a size below 1, views_if_last < 0 or B * K * H * W >= 2^31. */
int stf_tta_accumulate(const float* logits, int B, int K, int H, int W, int rule, int channel, int flip,
                       int first, int views_if_last, float* acc, stf_stream_t stream);

/* ---------------------------------------------------------------- boundary metrics
 * Per-image Hausdorff distance, its 95th percentile and the average symmetric surface distance of
 * two binary masks, as MedPy's hd / hd95 / assd define them at unit pixel spacing (INTEGRATION.md
 * 2.2 states the definition), and the exact squared Euclidean distance transform underneath.
 * Additive to ABI v17.  Limits: 1 <= B, 1 <= H, W <= 4096, B * H * W < 2^31 (so d2 < 2^25).
 * STF_EINVAL (nothing launched) for a NULL required pointer, a size outside the limits, a scratch,
 * out, counts or target that is not 8-byte aligned or a d2 that is not 4-byte aligned.  No entry
 * point allocates or reads back; results are the same bits from run to run.
 *
 * Bytes of the scratch either call needs for B images of H x W pixels, a multiple of 8 (0 outside
 * the limits). */
size_t stf_boundary_scratch_bytes(int B, int H, int W);
/* mask uint8 [B][H][W] (nonzero = predicted foreground), target int64 [B][H][W] (> 0 = foreground),
 * ignore as in stf_predict_mask.  out double [B][3] = {hd, hd95, assd} (NaN x3 when either border is
 * empty), counts int64 [B][2] = {|dP|, |dT|}; both OVERWRITTEN, may arrive uninitialised. */
int stf_boundary_metrics(const uint8_t* mask, const int64_t* target, int B, int H, int W, int64_t ignore,
                         double* out, int64_t* counts, void* scratch, stf_stream_t stream);
/* Squared distance of every pixel to the nearest nonzero pixel of sites (uint8 [B][H][W]) as int32
 * [B][H][W]; an image without sites gets INT32_MAX everywhere.  where (uint8, may be NULL): compute
 * only where it is nonzero, write -1 elsewhere.  The same row / column kernels as above.  The cost
 * per computed pixel grows with the distance found (an outward scan along the column). */
int stf_edt_sq(const uint8_t* sites, const uint8_t* where, int B, int H, int W, int32_t* d2,
               void* scratch, stf_stream_t stream);

/* ---------------------------------------------------------------- connected components
 * Labels and component post-processing of binary masks (INTEGRATION.md 2.2 states the definition).
 * Every image of mask uint8 [B][H][W] is labelled on its own: foreground is mask != 0, connectivity
 * is 4 (edge neighbours) or 8 (edges and corners), pixels outside the image are background.
 * Additive to ABI v17.  Limits: 1 <= B, 1 <= H, W <= 4096, B * H * W < 2^31.  STF_EINVAL (nothing
 * launched) for a NULL required pointer, a size outside the limits, a connectivity other than 4 or
 * 8, min_size < 0, counts without target, out == mask, a labels or num that is not 4-byte aligned,
 * or a scratch, counts or target that is not 8-byte aligned (mask and out may sit at any byte).
 * No entry point allocates, reads back or waits between workgroups; the number of launches is
 * fixed; the results are integers and the same bits from run to run.  All outputs are OVERWRITTEN
 * and may arrive uninitialised, the scratch too.
 *
 * Bytes of the scratch either call needs, a multiple of 8 (0 outside the limits). */
size_t stf_ccl_scratch_bytes(int B, int H, int W);
/* labels int32 [B][H][W]: 0 on the background, 1..n on the components, numbered per image in raster
 * order of each component's first pixel (scipy.ndimage.label's numbering); num int32 [B] = n. */
int stf_ccl_label(const uint8_t* mask, int B, int H, int W, int connectivity, int32_t* labels, int32_t* num,
                  void* scratch, stf_stream_t stream);
/* out uint8 [B][H][W] (may not alias mask): a foreground pixel keeps its own value when its
 * component passes, every other pixel is 0.  A component passes when its area is >= min_size and,
 * with keep_largest != 0, it is the image's largest (equal areas: the one whose first pixel comes
 * first in raster order); min_size applies first, so an image whose largest component is below it
 * comes out empty.  With target (int64 [B][H][W], or NULL) and counts (int64 [B][3], or NULL):
 * counts = (|P' & T|, |P'|, |T|) of the filtered mask with stf_predict_mask's rules (P' = out != 0,
 * T = target > 0, pixels whose target equals ignore_index left out of all three; ignore_index < 0:
 * none).  The mask is labelled with those pixels in.  num (or NULL) int32 [B]: the number of
 * components BEFORE filtering. */
int stf_ccl_filter(const uint8_t* mask, const int64_t* target, int B, int H, int W, int connectivity,
                   int keep_largest, int64_t min_size, int64_t ignore_index, uint8_t* out, int64_t* counts,
                   int32_t* num, void* scratch, stf_stream_t stream);

/* ---------------------------------------------------------------- connected components of volumes
 * The same for stacked slices.  mask uint8 [N][H][W] is cut into
 * V volumes of consecutive slices by starts int32 [V + 1]: strictly ascending, starts[0] = 0,
 * starts[V] = N.  The table is taken twice, like stf_grad_norm's: starts_dev in DEVICE memory, which
 * the kernels read, and starts_host, the same V + 1 entries on the host, which the call validates
 * before it returns.  Every volume is labelled on its own (volumes never touch, whatever their
 * adjacent slices hold): foreground is mask != 0, outside the volume is background, connectivity is
 * 6, 18 or 26 = scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3).
 * Additive to ABI v17.  Limits: 1 <= V <= N, 1 <= H, W <= 4096, N * H * W < 2^31.  STF_EINVAL
 * (nothing launched) for a NULL required pointer, a size outside the limits, V < 1, a host starts
 * that is not strictly ascending from 0 to N, a connectivity other than 6, 18 or 26, min_size < 0,
 * counts without target, out == mask, a labels, num or starts that is not 4-byte aligned, or a
 * scratch, counts or target that is not 8-byte aligned (mask and out may sit at any byte).
 * No entry point allocates, reads back or waits between workgroups; the number of launches is
 * fixed; atomics are integer only, so the results are the same bits from run to run.  All outputs
 * are OVERWRITTEN and may arrive uninitialised, the scratch too.
 *
 * Bytes of the scratch either call needs, a multiple of 8 (0 outside the limits). */
size_t stf_ccl3d_scratch_bytes(int N, int H, int W, int V);
/* labels int32 [N][H][W]: 0 on the background, 1..n on the components, numbered per volume in raster
 * order (z, y, x) of each component's first voxel (scipy.ndimage.label's numbering; a volume of
 * depth 1 gets stf_ccl_label's labels with 6 -> 4 and 18, 26 -> 8); num int32 [V] = n. */
int stf_ccl3d_label(const uint8_t* mask, int N, int H, int W, const int32_t* starts_dev,
                    const int32_t* starts_host, int V, int connectivity, int32_t* labels, int32_t* num,
                    void* scratch, stf_stream_t stream);
/* stf_ccl_filter's contract per volume instead of per image: min_size is in voxels and applies
 * first, keep_largest keeps the volume's largest component (equal areas: the one whose first voxel
 * comes first in raster order), a surviving voxel keeps its value.  counts (int64 [V][3], or NULL;
 * needs target int64 [N][H][W]) = (|P' & T|, |P'|, |T|) over the volume with stf_predict_mask's
 * ignore rule; num (or NULL) int32 [V]: the number of components BEFORE filtering. */
int stf_ccl3d_filter(const uint8_t* mask, const int64_t* target, int N, int H, int W,
                     const int32_t* starts_dev, const int32_t* starts_host, int V, int connectivity,
                     int keep_largest, int64_t min_size, int64_t ignore_index, uint8_t* out, int64_t* counts,
                     int32_t* num, void* scratch, stf_stream_t stream);

/* ---------------------------------------------------------------- lesion-level detection metrics
 * How many target lesions were found and how many predicted components are false findings, per image
 * or per volume (INTEGRATION.md 2.2 states the definition, DESIGN.md 5.19 the passes).
 * P = (mask != 0) & (target != ignore_index), T = (target > 0) & (target != ignore_index); ignored
 * voxels are background on BOTH sides before labelling (ignore_index < 0: none).  Each side is
 * labelled on its own by the stf_ccl_* / stf_ccl3d_* code (connectivity 4 / 8 for images, 6 / 18 / 26
 * for volumes, scipy's numbering).  A component of either side has an area (its voxels) and a hit
 * (its voxels on the other side's foreground) and is MATCHED iff hit >= 1 and
 * (double)hit >= min_overlap * (double)area.
 *   summary int64 [V][4] = {n_T, matched_T, n_P, matched_P}  (images: V = B)
 *   table   int64 [V][2][max_lesions][2]: side 0 the target, side 1 the prediction; row l - 1 holds
 *           (area, hit) of label l, rows past n are 0, labels above max_lesions are left out (but
 *           counted in summary, so n > max_lesions says the table was cut).  max_lesions = 0: no
 *           table is written and table may be NULL.
 * Additive to ABI v17.  Limits as for stf_ccl_* / stf_ccl3d_*.  STF_EINVAL (nothing launched) for a
 * NULL mask, target, summary, scratch (or table with max_lesions > 0, or starts), a size outside the
 * limits, a bad connectivity, a min_overlap outside [0, 1] or NaN, max_lesions < 0, a host starts
 * that is not strictly ascending from 0 to N, a starts that is not 4-byte aligned, or a target,
 * summary, table or scratch that is not 8-byte aligned (mask may sit at any byte).  No entry point
 * allocates, reads back or waits between workgroups; the number of launches is fixed (images 6;
 * volumes 8, 7 without a table); atomics are integer only, so the results are the same bits from run
 * to run and for a volume passed alone or inside a stack.  All outputs are OVERWRITTEN and may arrive
 * uninitialised, the scratch too.
 *
 * Bytes of the scratch either call needs, a multiple of 8 (0 outside the limits); V = B for images. */
size_t stf_lesion_scratch_bytes(int N, int H, int W, int V);
int stf_lesion_metrics(const uint8_t* mask, const int64_t* target, int B, int H, int W, int connectivity,
                       double min_overlap, int max_lesions, int64_t ignore_index, int64_t* summary,
                       int64_t* table, void* scratch, stf_stream_t stream);
/* The same per volume; starts_dev / starts_host / V as stf_ccl3d_* take them. */
int stf_lesion3d_metrics(const uint8_t* mask, const int64_t* target, int N, int H, int W,
                         const int32_t* starts_dev, const int32_t* starts_host, int V, int connectivity,
                         double min_overlap, int max_lesions, int64_t ignore_index, int64_t* summary,
                         int64_t* table, void* scratch, stf_stream_t stream);

/* ---------------------------------------------------------------- score histograms
 * The object every threshold-free figure is made of (INTEGRATION.md 2.2 states the definitions,
 * DESIGN.md 5.20 the pass): per image, the histogram of the foreground score split by the target.
 * src fp32 [N][K][H][W]; the score p of a pixel is
 *   source 0   plane `channel` of the softmax over the K logit planes (stf_tta_accumulate's rule 0);
 *   source 1   1 / (1 + expf(-x)) of logit plane `channel` (stf_predict_mask's rule 1);
 *   source 2   plane `channel` itself (probabilities already);
 * and its row, with bins a power of two in [2, 4096],
 *   row(p) = 0                                       if not (p > 0)   (0, -0, negatives, NaN)
 *          = min(bins, (int)ceilf(p * (float)bins))  otherwise        (+inf and p > 1: row bins)
 * p * bins is exact, so row j >= 1 holds (j - 1) / bins < p <= j / bins, and row(p) > j <=> p > j / bins
 * for p <= 1: the rows above j are the pixels stf_predict_threshold marks at threshold j / bins.
 * hist int64 [N][2][bins + 1] is OVERWRITTEN (zeroed on the stream, then counted; it may arrive
 * uninitialised): hist[n][s][r] = pixels of image n with row r on side s; side 1 is target > 0
 * (positive < 0) or target == positive, side 0 every other pixel; pixels whose target equals
 * ignore_index (>= 0; negative: none) are in neither.  One launch; integer atomics only, so the same
 * bits from run to run.  Additive to ABI v17.  Limits: 1 <= N, 1 <= H, W <= 4096, N * H * W < 2^31,
 * 1 <= K <= 16.  STF_EINVAL (nothing launched) for a NULL pointer, a size outside the limits,
 * channel outside [0, K), a source other than 0 / 1 / 2, bins not a power of two in [2, 4096], or a
 * target or hist that is not 8-byte aligned (src may sit at any multiple of 4). */
int stf_score_hist(const float* src, int N, int K, int H, int W, int source, int channel, const int64_t* target,
                   int64_t positive, int64_t ignore_index, int bins, int64_t* hist, stf_stream_t stream);

/* ---------------------------------------------------------------- lesion confidence and FROC
 * The lesion-level metrics swept over the confidence of each predicted component, per image or per
 * volume (INTEGRATION.md 2.2 states the definition, DESIGN.md 5.21 the passes).  mask, target, P, T,
 * the ignore rule, the labelling, connectivity, starts and the MATCHED rule are stf_lesion_metrics' /
 * stf_lesion3d_metrics'; every component of P is a candidate.  src fp32 [N][K][H][W], source, channel
 * and bins are stf_score_hist's: the score p of a voxel and its row(p) in 0..bins.
 *   conf(c) = max row(p) over the voxels of candidate c
 *   det(t)  = max conf(c) over the MATCHED candidates c that share a voxel with lesion t, 0 without one
 *   summary int64 [V][4] = {n_T, matched_T, n_P, matched_P}: stf_lesion_metrics' bits  (images: V = B)
 *   table   int64 [V][2][max_lesions][3]: stf_lesion_metrics' table with a third column: row l - 1
 *           holds (area, hit, score) of label l, score = det on side 0 (target) and conf on side 1
 *           (prediction); rows past n are 0, labels above max_lesions are left out; max_lesions = 0:
 *           no table is written and table may be NULL.
 *   hist    int64 [V][3][bins + 1]: side 0 the candidates that are not matched (false findings) by
 *           conf, side 1 the target lesions by det (row 0: the lesions no matched candidate reached),
 *           side 2 the matched candidates by conf.  The sides sum to n_P - matched_P, n_T, matched_P.
 *           Integers, additive over cases.
 * Additive to ABI v17.  The limits are stf_lesion_metrics' and stf_score_hist's: 1 <= K <= 16.  STF_EINVAL
 * (nothing launched, outputs untouched) for whatever either of the two refuses: a NULL mask, src,
 * target, summary, hist, scratch (or table with max_lesions > 0, or starts), a size outside the limits,
 * a bad connectivity, a min_overlap outside [0, 1] or NaN, max_lesions < 0, K outside 1..16, channel
 * outside [0, K), a source other than 0 / 1 / 2, bins not a power of two in [2, 4096], a host starts
 * that is not strictly ascending from 0 to N, a src or starts that is not 4-byte aligned, or a target,
 * summary, table, hist or scratch that is not 8-byte aligned (mask may sit at any byte).  No entry
 * point allocates, reads back or waits between workgroups; the number of launches is fixed (hist's
 * memset and: images 7; volumes 9, 8 without a table); atomics are integer only, so the results are
 * the same bits from run to run and for a volume passed alone or inside a stack.  All outputs are
 * OVERWRITTEN and may arrive uninitialised, the scratch too.
 *
 * Bytes of the scratch either call needs, a multiple of 8 (0 outside the limits, bins' included);
 * V = B for images. */
size_t stf_froc_scratch_bytes(int N, int H, int W, int V, int bins);
int stf_froc(const uint8_t* mask, const float* src, int K, int source, int channel, const int64_t* target, int B,
             int H, int W, int connectivity, double min_overlap, int max_lesions, int64_t ignore_index, int bins,
             int64_t* summary, int64_t* table, int64_t* hist, void* scratch, stf_stream_t stream);
/* The same per volume; starts_dev / starts_host / V as stf_ccl3d_* take them. */
int stf_froc3d(const uint8_t* mask, const float* src, int K, int source, int channel, const int64_t* target, int N,
               int H, int W, const int32_t* starts_dev, const int32_t* starts_host, int V, int connectivity,
               double min_overlap, int max_lesions, int64_t ignore_index, int bins, int64_t* summary,
               int64_t* table, int64_t* hist, void* scratch, stf_stream_t stream);

/* ---------------------------------------------------------------- boundary metrics of volumes
 * Per-volume (per-case) HD, HD95 and ASSD with voxel spacing: MedPy's hd / hd95 / assd on a 3-D
 * array with voxelspacing = (sz, sy, sx) and connectivity 1 (INTEGRATION.md 2.2 states the
 * definition, DESIGN.md 5.17 the passes), and the squared weighted distance transform underneath.
 * The stack [N][H][W] is cut into V volumes by the starts table of stf_ccl3d_*, taken twice in the
 * same way (starts_dev for the kernels, starts_host validated before the call returns); volumes
 * never see each other, neither for the border (6-neighbour cross, outside the volume background)
 * nor for distances.  spacing_dev: DEVICE double [V][3], one (sz, sy, sx) per volume, finite and
 * > 0 (the caller's duty: the table is on the device).  Squared distances are float64 throughout,
 * ((sx dx)^2 + (sy dy)^2) + (sz dz)^2 with one rounding per operation: exact whenever the products
 * are (unit spacing; spacings of few significant bits).
 * Additive to ABI v17.  Limits: 1 <= V <= N, 1 <= H, W <= 4096, N * H * W < 2^31.  STF_EINVAL
 * (nothing launched) for a NULL required pointer, a size outside the limits, V < 1, a host starts
 * that is not strictly ascending from 0 to N, a starts that is not 4-byte aligned, or a scratch,
 * spacing_dev, out, counts, target or d2 that is not 8-byte aligned (mask, sites and where may sit
 * at any byte).  No entry point allocates, reads back or waits between workgroups; the number of
 * launches is fixed; floating-point sums are taken in a fixed order that depends only on the
 * position inside the volume, so the results are the same bits from run to run and for a volume
 * passed alone or inside a stack.  All outputs are OVERWRITTEN and may arrive uninitialised, the
 * scratch too.
 *
 * Bytes of the scratch either call needs, a multiple of 8 (0 outside the limits). */
size_t stf_boundary3d_scratch_bytes(int N, int H, int W, int V);
/* mask uint8 [N][H][W] (nonzero = predicted foreground), target int64 [N][H][W] (> 0 = foreground),
 * ignore as in stf_predict_mask.  out double [V][3] = {hd, hd95, assd} in the spacing's unit (NaN x3
 * when either border of the volume is empty), counts int64 [V][2] = {|dP|, |dT|}. */
int stf_boundary3d_metrics(const uint8_t* mask, const int64_t* target, int N, int H, int W,
                           const int32_t* starts_dev, const int32_t* starts_host, int V,
                           const double* spacing_dev, int64_t ignore, double* out, int64_t* counts,
                           void* scratch, stf_stream_t stream);
/* d2 double [N][H][W]: the squared weighted distance of every voxel to the nearest nonzero voxel of
 * sites (uint8 [N][H][W]) of the same volume; +inf throughout a volume without sites.  where (uint8,
 * may be NULL): compute only where it is nonzero, write -1 elsewhere.  The same row, plane and depth
 * code as above.  The cost per computed voxel grows with the distance found. */
int stf_edt3d_sq(const uint8_t* sites, const uint8_t* where, int N, int H, int W, const int32_t* starts_dev,
                 const int32_t* starts_host, int V, const double* spacing_dev, double* d2, void* scratch,
                 stf_stream_t stream);

/* ---------------------------------------------------------------- boundary loss
 * The boundary loss of Kervadec et al. (MIDL 2019; INTEGRATION.md 2.1 states the definition, DESIGN.md
 * 5.18 the passes): dense signed distance maps of the targets, the term and its gradient.  Additive
 * to ABI v17; no entry point allocates or reads back; no floating-point atomics, the same bits from
 * run to run.
 *
 * The maps.  target int64 [N][H][W], classes K in 2..16; phi float32 [N][K-1][H][W], OVERWRITTEN,
 * channel k-1 for class k = 1..K-1 with G = {target == k} (a pixel whose target equals ignore, when
 * ignore >= 0, is in no G): +d(q, G) outside G, 1 - d(q, not G) inside (0 on G's innermost border),
 * d the exact Euclidean distance in pixels as (float)sqrt((double)d2); 0 everywhere where G is empty
 * or the whole image.  Limits: N >= 1, 1 <= H, W <= 4096, N * (K-1) * H * W < 2^31.  The cost does
 * not depend on where the sites are.  STF_EINVAL (nothing launched) for a NULL pointer, a size outside
 * the limits, a scratch or target that is not 8-byte aligned or a phi that is not 4-byte aligned.
 *
 * Bytes of the scratch stf_sdf needs, a multiple of 8 (0 outside the limits). */
size_t stf_sdf_scratch_bytes(int N, int H, int W, int classes);
int stf_sdf(const int64_t* target, int N, int H, int W, int classes, int64_t ignore, float* phi, void* scratch,
            stf_stream_t stream);
/* The term.  With m = (ignore >= 0 ? target != ignore : 1), p = softmax(logits) over the K classes,
 * M = sum m over the batch and phi_0 = 0:
 *   L_B  = sum_{n, q, k >= 1} m p_k phi_k / ((K-1) M)
 *   dz_j = m p_j (phi_j - sum_{c >= 1} p_c phi_c) / ((K-1) M)
 * Both entry points ACCUMULATE, so they follow a criterion route's forward / backward on the same
 * stream: stf_bloss_fwd does loss[0] += alpha * L_B (NaN when every pixel is ignored, as the
 * cross-entropy) and leaves (sum, M) in partials[0..1]; stf_bloss_bwd does
 * dlogits += grad_out[0] * alpha * dz (grad_out NULL = 1) with M = partials + 1 of the forward, and
 * does not touch an ignored pixel.  logits fp32 [N][K][H][W], phi as above, partials
 * stf_bloss_scratch_floats(N) floats (0 for N outside 1..65535).  STF_EINVAL (nothing launched) for a
 * NULL required pointer, K outside 2..16, an ignore that is a class id, N outside 1..65535,
 * H * W >= 2^31 or an alpha that is negative or not finite. */
int stf_bloss_scratch_floats(int N);
int stf_bloss_fwd(const float* logits, const int64_t* target, const float* phi, int N, int H, int W, int classes,
                  int ignore, float alpha, float* partials, float* loss, stf_stream_t stream);
int stf_bloss_bwd(const float* logits, const int64_t* target, const float* phi, int N, int H, int W, int classes,
                  int ignore, float alpha, const float* grad_out, const float* M, float* dlogits,
                  stf_stream_t stream);

/* ---------------------------------------------------------------- PK maps (extended Tofts)
 * pk_fitting.py ToftsModelFitter, all fp32.  The host builds
 * the reference's constant tables exactly as the reference does (pk_fitting.py:
 * 193-203): time_points t[T], cp_t = Cp(t), the convolution grid tau = arange(0,
 * t[T-1], dt) and cp_tau = Cp(tau) (n_conv entries), and n_valid[i] = #{tau_j < t_i}
 * (device int array).  T <= 32, n_conv <= 8192. */
/* C[P][T] = extended_tofts_model_batch(t, ktrans, ve, vp) (pk_fitting.py:193-231). */
int stf_tofts_forward(const float* ktrans, const float* ve, const float* vp, int P, int T,
                      const float* time_points, const float* cp_t, const float* tau,
                      const float* cp_tau, const int* n_valid, int n_conv, float dt, float* out,
                      stf_stream_t stream);
/* The fit loop of fit_volume_gpu (pk_fitting.py:280-365) for P tissue curves [P][T]
 * (row-major pixel order): batches of `batch` pixels, `epochs` passes, torch Adam
 * over the whole parameter vectors after every batch (pixels outside the batch take
 * a zero-gradient step), clamps after each step.  params [3][P] (Ktrans, ve, vp):
 * initial values in, fitted values out.  adam_sched: DEVICE [epochs*nbatches][2] =
 * (lr / (1 - beta1^s), sqrt(1 - beta2^s)) for s = 1.. (double-precision bias
 * corrections rounded to fp32, as torch applies them).  bounds: HOST [3][2] clamp
 * ranges. */
int stf_tofts_fit(const float* curves, int P, int T, const float* time_points, const float* cp_t,
                  const float* tau, const float* cp_tau, const int* n_valid, int n_conv, float dt,
                  int batch, int epochs, const float* adam_sched, float beta1, float beta2, float eps,
                  const float* bounds, float* params, stf_stream_t stream);

/* ---------------------------------------------------------------- training augmentation
 * Replaces the per-sample CPU transforms of the reference's DataLoader workers
 * (transforms.py:18-157 as composed by train.py:51-73 get_transform; my_dataset.py:
 * 200-239 applies them per frame): RandomResize (Pillow bilinear / nearest) ->
 * RandomHorizontalFlip -> RandomVerticalFlip -> RandomRotation (Pillow bilinear /
 * nearest, expand=False) -> RandomCrop (zero pad) -> ToTensor + Normalize, bit-exact
 * to Pillow 12's integer / double arithmetic.  The host draws the random parameters
 * (Python `random`, the reference's draw order), builds Pillow's coefficient tables
 * and fills one descriptor per frame / mask; sources of any sizes sit in one uint8
 * arena (src offsets in bytes).
 *
 * frames: coefficient rows at coef[cx + j*(kx+2)] = {xmin, n, k_0..k_{kx-1}} for
 * output column j (likewise cy/ky for rows; 22-bit fixed point, Pillow
 * ImagingResample); the resized H2 x W2 image goes to scratch[rs]; the output
 * window oh x ow (crop origin h0, w0 in the zero-padded rotated image) is written
 * as fp32 (v/255 - mean)/std at out[out + y*ow + x].  m = Image.rotate's inverse
 * affine (double), used when flags & STF_AUG_ROTATE.
 * masks: cx / cy index int tables of W2 / H2 source columns / rows (-1 = outside,
 * Pillow ImagingScaleAffine), fx = {a0, a1, a3, a4, xo, yo} 16.16 fixed-point
 * rotation; output int64.
 * max_resized_px / max_out_px = largest H2*W2 / oh*ow in the list (grid size). */
#define STF_AUG_HFLIP 1
#define STF_AUG_VFLIP 2
#define STF_AUG_ROTATE 4
typedef struct stf_aug_frame {
  int64_t src, rs, out;
  int H, W, H2, W2;
  int cx, cy, kx, ky;
  int oh, ow, h0, w0;
  int flags;
  int fx[6];
  int pad_;
  double m[6];
} stf_aug_frame;
int stf_augment_frames(const uint8_t* src, const stf_aug_frame* frames, int n, const int* coef,
                       uint8_t* scratch, int max_resized_px, int max_out_px, float mean, float stdv,
                       float* out, stf_stream_t stream);
int stf_augment_masks(const uint8_t* src, const stf_aug_frame* masks, int n, const int* tabs,
                      int max_out_px, int64_t* out, stf_stream_t stream);

/* ---------------------------------------------------------------- launch plans
 * The native step runtime behind the models' forward / backward (stfunet/plan.py).
 * The reference's step is Python issuing one PyTorch op per layer and per LSTM time
 * step (src/stf_lstm_unet.py:168-254 forward, its autograd backward;
 * train_utils/train_and_eval.py:384-404); here the first steps of a shape run the
 * programs' schedule from Python and one of them RECORDS it: while a plan records on
 * the calling thread, every launch, async memset / device copy and stream wait of
 * this library executes as usual and is appended to the plan with its final
 * arguments (tile choices, split plans, workspace pointers resolved).  Later steps
 * replay ranges of it with stf_plan_replay: the same kernels, streams and events,
 * bit for bit the recorded step's results, no per-launch host logic.  The caller
 * keeps every buffer the recorded step touched alive at its address.
 * These are the only entry points that keep state: a plan owns its ops and events
 * (stf_plan_destroy frees them); the recording flag is per host thread.
 *
 * stf_plan_tag(name, flops) / stf_plan_tag_end(): while recording, mark the ops of
 * the following C-ABI call (a kernel family and its algorithmic FLOPs: bench.py's
 * roofline); stf_plan_replay(.., timed_tag) brackets every range with that name by
 * HIP events on its stream, stf_plan_timing sums them (and synchronizes).
 * stf_stream_wait: `waiter` waits for the work enqueued on `waitee` so far (an
 * event record + stream wait; recorded like a launch).
 * stf_memset / stf_copy_rows (dst[r][0:cols] = src[r][0:cols], fp32, row strides in
 * elements) / stf_i64_add_batch (*ptrs[i] += inc: BatchNorm num_batches_tracked):
 * the step's remaining tensor ops as plan-recordable launches. */
typedef struct stf_plan stf_plan;
stf_plan* stf_plan_create(void);
void stf_plan_destroy(stf_plan* plan);
int stf_plan_record(stf_plan* plan);
int stf_plan_stop(void);
int stf_plan_size(const stf_plan* plan);
int stf_plan_tag(const char* name, double flops);
int stf_plan_tag_end(void);
int stf_plan_replay(stf_plan* plan, int first, int last, const char* timed_tag);
int stf_plan_timing(stf_plan* plan, int* launches, double* ms, double* flops);
int stf_stream_wait(stf_stream_t waiter, stf_stream_t waitee);
int stf_memset(void* p, int value, size_t bytes, stf_stream_t stream);
int stf_copy_rows(const float* src, int64_t src_ld, float* dst, int64_t dst_ld, int rows, int cols,
                  stf_stream_t stream);
int stf_i64_add_batch(int64_t* const* ptrs, int count, int64_t inc, stf_stream_t stream);

const char* stf_error_string(int code);
int stf_abi_version(void);

/* 16-bit activation storage this library was built for: every entry point above
 * reads and writes its 16-bit tensors (activations, packed weights, gradients w.r.t.
 * activations) in this type.  libstfunet_hip.so = bf16, libstfunet_hip_f16.so = fp16
 * (the reference's autocast(float16) + GradScaler path, train_and_eval.py:389,
 * train.py:240); same entry points, layouts and constraints otherwise. */
#define STF_STORAGE_BF16 0
#define STF_STORAGE_FP16 1
int stf_storage_type(void);

#ifdef __cplusplus
}
#endif
#endif /* STFUNET_H */
