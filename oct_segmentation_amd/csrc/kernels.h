// Host-side launchers of the gfx950 kernels (all stream-ordered, never synchronise).
#pragma once
#include "common.h"

namespace octseg {

// conv_mfma.hip
int conv_num_mtiles(const ConvArgs& a, int dtype);       // M tiles of a launch as given
int conv_num_mtiles_flat(const ConvArgs& a, int dtype);  // ... as launch_conv runs it (= BN-stat slab rows)
// Layout of the packed weight image a launch expects in ConvArgs::W:
// [wtap][chunk][N tile][BN rows][RB bytes], zero padded, 16-byte chunks XOR-swizzled per row.
struct ConvPackInfo { int BN, RB, nchunks, ntiles; };
ConvPackInfo conv_pack_info(const ConvArgs& a, int dtype);
static inline size_t conv_image_bytes(const ConvPackInfo& p, int wtaps) {
  return (size_t)wtaps * p.nchunks * p.ntiles * p.BN * p.RB;
}
hipError_t launch_conv(int dtype, const ConvArgs& a, hipStream_t st);
// Which kernel launch_conv gives a launch to (thin.hip, gemm1x1.hip, conv3x3p.hip or conv_mfma_kernel), and conv_mfma_kernel's tiling of a
// ROUTE_MFMA launch: 16-pixel-wide tiles (16 or 8 rows), 11 x 11 tiles, or the 256-channel wide-N tile.  Queries: nothing is launched.
enum ConvRoute { ROUTE_THIN, ROUTE_GEMM1X1, ROUTE_CONV3X3P, ROUTE_MFMA };
enum ConvTile { TILE_16, TILE_11, TILE_WIDE_N };
ConvRoute conv_route(const ConvArgs& a, int dtype);
int conv_mfma_tile(const ConvArgs& a, int dtype);
// How a destination element is rounded (T = the storage type; `y` = the f32 accumulator + bias, after relu_out):
//   conv_mfma_kernel, gemm1x1, conv3x3p (the tile is transposed through LDS as T):
//     store  T(y);   accum  T(f32(T(y)) + old);   pool  T(old + T(y00) + T(y01) + T(y10) + T(y11)), the sum in f32 in that order
//     -- bit for bit what a T temp followed by masked_accum / pool2x2_accum gives;
//   thin.hip (the accumulators go to memory straight from registers):
//     store  T(y);   accum  T(y + old);           pool  T(old + (y00 + y10 + y01 + y11)), nothing rounded before the last step.
// BatchNorm statistics are always those of the f32 `y`, over the pixels inside the map.  tests/conv_ref.py states both rules.
// The tied decoder layer (ConvLayer::tie; its launches all run in conv_mfma_kernel) follows from the first rule, launch by launch:
//   forward        the skip slice's launch stores T(s), the parity launch that owns a pixel adds its T(u):  y = T(f32(T(u)) + T(s));
//                  without skip channels each parity launch stores T(u).  (u, s: the sums over the up / skip channels.)
//   data gradient  of the `up` source, at the LOW resolution:  T(g);  accum  T(f32(T(g)) + old),  g = the whole sum over the 2x2 quad and all its
//                  taps in one f32 accumulator -- the pooled rule above (four T(q) added to old) does not apply: nothing is pooled
//   weight gradient  f32 throughout: dW3 += fold(dK4) (+ dW3s), launch_tied_fold.     tests/tied_cases.py states these rules.
// The stem kernels see the frame as T(f32(f32(raw - mean) * f32(1 / std))), zero outside the frame (tests/stem_ref.py): thin.hip keeps the f32 product
// in registers, stem_im2col_kernel must not let the f16 conversion absorb the multiply (v_fma_mixlo_f16 rounds the exact product once).
bool conv_masked_eligible(const ConvArgs& a, int dtype);   // launches with per-source tap subsets (ConvArgs::taps_per_src): can the masked loop take this one?

// gemm1x1.hip: stride-1, single-source 1x1 convs and their data gradients as a persistent GEMM (2-byte dtypes); consumes the same
// packed weight image as conv_mfma_kernel.  launch_conv routes eligible launches there; its BN-stat slab has one row per
// workgroup (gemm1x1_rows) instead of one per M tile.
bool gemm1x1_eligible(const ConvArgs& a, int dtype);
int gemm1x1_rows(const ConvArgs& a);
hipError_t launch_gemm1x1(int dtype, const ConvArgs& a, hipStream_t st);

// Deterministic-reduction mode (octseg_set_deterministic / OCTSEG_DETERMINISTIC=1): no floating-point atomic meets another
// workgroup's -- weight gradients without split-K, Dice sums and bias gradients by one workgroup per output.  Slower; bit-stable.
bool deterministic_mode();

// conv3x3p.hip: persistent 3x3 stride-1 conv / data gradient (2-byte dtypes, interior tiles, 128-channel N tile): one software pipeline
// over the flattened (tile, K chunk, tap) sequence of a workgroup; same weight image and BN-stat slab rows as conv_mfma_kernel's 16x16 tile
bool conv3x3p_eligible(const ConvArgs& a, int dtype);
int conv3x3p_rows(const ConvArgs& a);
hipError_t launch_conv3x3p(int dtype, const ConvArgs& a, hipStream_t st);

// thin.hip: 3x3 stride-1 layers with 16 / 32 input and <= 32 output channels on large maps (the last decoder block and the head) as
// HBM-bound persistent kernels: forward / data gradient (weights as the MFMA A operand, built from the fp32 master weights; BN-stat
// slab: one row per workgroup = thin_conv_rows) and weight gradient.  launch_conv / launch_wgrad route eligible launches there.
bool thin_conv_eligible(const ConvArgs& a, int dtype);
int thin_conv_rows(const ConvArgs& a);
hipError_t launch_thin_conv(int dtype, const ConvArgs& a, hipStream_t st);
bool thin_wgrad_eligible(const WgradArgs& a, int dtype);
hipError_t launch_thin_wgrad(int dtype, const WgradArgs& a, hipStream_t st);
// ... and the ResNet stem (7x7 stride 2, 3 -> 64) straight from the NCHW f32 frame: forward (+ BN partials, one slab row per workgroup =
// thin_stem_rows) and weight gradient; no im2col tensor
struct StemArgs {
  const float* img; int N, H, W;            // frame [N][3][H][W] f32
  int normalize; float mean[3], stdv[3];
  const float* w;                            // fp32 master [64][160], k = (r * 7 + s) * 3 + ci
  const float* wscale; const float* bias; int relu_out;   // eval: folded BatchNorm
  void* y;                                   // forward: raw output NHWC T [N][H/2][W/2][64]
  float* slab; int slab_row0;
  const void* dy; float* dW;                 // weight gradient: dy NHWC T [N][H/2][W/2][64], dW [64][160] accumulated
};
bool thin_stem_eligible(int dtype);
int thin_stem_rows(int N, int H, int W);
hipError_t launch_thin_stem_forward(int dtype, const StemArgs& s, hipStream_t st);
hipError_t launch_thin_stem_wgrad(int dtype, const StemArgs& s, hipStream_t st);

// pan.hip: smp's PAN decoder beside its convs -- MaxPool2d(2, 2), the feature-pyramid-attention block's one-channel pyramid (one workgroup, f32),
// its wide 7x7 -> 1-channel conv, the final u * mid + b1 mix, and a plain add
hipError_t launch_maxpool2(int dtype, const void* x, void* p, const void* dp, void* dx, int N, int H, int W, int C, int accum, hipStream_t st);   // dp == nullptr: forward
hipError_t launch_fpa_in_fwd(int dtype, const void* p, const float* w, const float* b, float* y, int N, int H, int W, int C, int K, hipStream_t st);
hipError_t launch_fpa_in_bwd(int dtype, const void* p, const float* dy, const float* w, void* dp, float* dw, float* db, int N, int H, int W, int C, int K,
                             hipStream_t st);
struct FpaPyrArgs {        // layers 0..5 = down1, down2, down3.1, down3.2, conv2, conv1 (each conv k x k + bias, BatchNorm2d(1), ReLU)
  int N, h, w, train;      // h x w: the block's input map; the pyramid lives on h/2, h/4, h/8
  float* scratch; float* gscratch; const float* duu;
  const float* w_[6]; const float* b_[6]; const float* g_[6]; const float* be_[6]; float* rm_[6]; float* rv_[6];
  float* dw_[6]; float* db_[6]; float* dg_[6]; float* dbe_[6];
};
size_t fpa_pyr_scratch_floats(int N, int h, int w);    // forward values kept for the backward (+ the upsampled map uu [N][h][w] and 12 statistics)
size_t fpa_pyr_gscratch_floats(int N, int h, int w);   // gradients; d(x1raw) is the N (h/2) (w/2) floats at gscratch + N (h/2) (w/2)
hipError_t launch_fpa_pyr_fwd(const FpaPyrArgs& a, hipStream_t st);   // x1raw in scratch[0 .. n1) -> uu at scratch + fpa_pyr_uu_offset
hipError_t launch_fpa_pyr_bwd(const FpaPyrArgs& a, hipStream_t st);
static inline size_t fpa_pyr_uu_offset(int N, int h, int w) { return fpa_pyr_scratch_floats(N, h, w) - 16 - (size_t)N * h * w; }
hipError_t launch_fpa_mix(int dtype, const float* uu, const void* mid, const void* b1, void* out, const void* g, void* dmid, float* duu, int N, int HW, int C,
                          hipStream_t st);             // g == nullptr: forward out = uu mid + b1; else dmid = g uu, duu = sum_c g mid
hipError_t launch_add2(int dtype, const void* a, const void* b, void* out, size_t numel, hipStream_t st);

// pab.hip: the position attention block of smp's MAnet decoder between its convolutions (strided f32-accumulating GEMMs on activations,
// softmax over a whole position map, the un-transposed reshape of the attended map)
struct PabGemm {           // C[b][m][n] (+)= sum_k A[b][m][k] B[b][k][n]; strides in elements; *_f32: the operand is float whatever the plan's dtype
  const void* A; const void* B; void* C;
  size_t sAb, sAm, sAk, sBb, sBk, sBn, sCb, sCm, sCn;
  int M, N, K, batch, a_f32, b_f32, c_f32, accum;
};
hipError_t launch_pab_gemm(int dtype, const PabGemm& g, hipStream_t st);
hipError_t launch_pab_softmax(float* S, const float* P, int batch, size_t n, int backward, hipStream_t st);   // forward: in place; backward: dP -> dS in place
hipError_t launch_pab_mix(int dtype, const void* x, const float* M, void* y, float* dM, const void* dy, int N, int HW, int C, hipStream_t st);

// effnet.hip: the non-GEMM operators of efficientnet_pytorch's MBConvBlock (smp 'efficientnet-b0' / '-b5' / '-b7')
struct DwgArgs {           // depthwise K x K (3 | 5), stride 1 | 2, top/left padding `pad` (TF static "same"); w / dw: fp32 [K][K][C]
  const void* in; void* out; void* gin; const float* w; float* dw;   // backward: out = gout, gin = gradient of `in`
  int N, H, W, C, OH, OW, K, stride, pad, accum;
};
hipError_t launch_dwg_fwd(int dtype, const DwgArgs& a, hipStream_t st);
hipError_t launch_dwg_bwd_data(int dtype, const DwgArgs& a, hipStream_t st);
hipError_t launch_dwg_bwd_w(int dtype, const DwgArgs& a, hipStream_t st);
struct BnxArgs {           // forward: out = act(y * scale + shift) * dscale[n] + post;  backward: out = g(=post) * dscale[n] * act'(y * scale + shift)
  const void* y; const float* scale; const float* shift; const float* dscale; const void* post; void* out;
  size_t npix; int hw, C, act;    // act: 0 identity, 1 swish
};
hipError_t launch_bnx_fwd(int dtype, const BnxArgs& a, hipStream_t st);
hipError_t launch_bnx_bwd(int dtype, const BnxArgs& a, hipStream_t st);
struct SefcArgs {          // s = W2 swish(W1 m + b1) + b2 on pooled vectors m [N][C] (T); W1 [R][C], W2 [C][R] fp32; h / dh: float [N][R] scratch
  const void* m; void* s; const void* ds; void* dm;
  const float* w1; const float* b1; const float* w2; const float* b2; float* dw1; float* db1; float* dw2; float* db2;
  float* h; float* dh;
  int N, C, R;
  int act;                 // activation between the two layers: 1 swish (EfficientNet), 0 ReLU (MAnet's SE_ll / SE_hl)
};
hipError_t launch_sefc_fwd(int dtype, const SefcArgs& a, hipStream_t st);
hipError_t launch_sefc_bwd(int dtype, const SefcArgs& a, hipStream_t st);   // dm, dh, then the four parameter gradients (accumulated)

// se.hip: squeeze-excite gate of timm's SEModule (RegNetY): out (+)= in * sigmoid(s[n][c]) and the gate's own gradient
// ds[n][c] = sigmoid'(s) * sum_p g * x (float scratch `part`: N x se_dgate_shares(HW) x C floats)
// (s2 / ds2 != nullptr: MAnet's MFAB gate sigmoid(s) + sigmoid(s2) -- two excitations of one tensor)
hipError_t launch_se_gate(int dtype, const void* in, const void* s, void* out, int N, int HW, int C, int accum, hipStream_t st, const void* s2 = nullptr);
int se_dgate_shares(int HW);
hipError_t launch_se_dgate(int dtype, const void* g, const void* x, const void* s, void* ds, float* part, int N, int HW, int C, hipStream_t st,
                           const void* s2 = nullptr, void* ds2 = nullptr);

// wgrad_mfma.hip
hipError_t launch_wgrad(int dtype, const WgradArgs& a, hipStream_t st);
enum WgradRoute { WROUTE_THIN, WROUTE_1X1, WROUTE_MFMA };
WgradRoute wgrad_route(const WgradArgs& a, int dtype);   // the kernel launch_wgrad gives a launch to (a query: nothing is launched)
// wgrad1x1.hip: stride-1 1x1 weight gradients (bf16, 64-divisible channel counts, flattened pixel list) as an LDS-DMA ring pipeline;
// wgrad_convt.hip: ConvTranspose2d(k4, s2, p1) weight gradient, all four output parities (16 taps) in one launch; `a` = any of the four
// per-parity launches of the transposed form (they share sources, extents, dy and dW)
bool wgrad_convt16_eligible(const WgradArgs& a, int dtype);
hipError_t launch_wgrad_convt16(int dtype, const WgradArgs& a, hipStream_t st);
// launch_wgrad routes eligible launches there after flatten_1x1
bool wgrad1x1_eligible(const WgradArgs& flattened, int dtype);
hipError_t launch_wgrad1x1(int dtype, const WgradArgs& flattened, hipStream_t st);

// elementwise.hip -----------------------------------------------------------------------------
// BatchNorm finalize (training): reduce the [rows][C][2] slab -> mean/var, scale/shift, running stats.
hipError_t launch_bn_finalize_train(const float* slab, int rows, int C, double count, const float* gamma,
                                    const float* beta, float* running_mean, float* running_var,
                                    float momentum, float eps, float* scale, float* shift, float* mean,
                                    float* rstd, double* part, unsigned* counters, hipStream_t st);
// `part` (SLAB_PART_CAP x 2 doubles) and `counters` (64 zeroed uints) are the scratch of the two-level slab reduction.
constexpr int SLAB_PART_CAP = 16384;
// eval: scale/shift from the running statistics.
// statistics of a tensor with <= BN_SMALL_COUNT values per channel, two-pass in double from the conv output itself (no slab)
constexpr int BN_SMALL_COUNT = 1024;
hipError_t launch_bn_finalize_small(int dtype, const void* y, int count, int C, const float* gamma, const float* beta, float* running_mean,
                                    float* running_var, float momentum, float eps, float* scale, float* shift, float* mean, float* rstd,
                                    hipStream_t st);
hipError_t launch_bn_finalize_eval(int C, const float* gamma, const float* beta, const float* running_mean,
                                   const float* running_var, float eps, float* scale, float* shift,
                                   hipStream_t st);

// frozen (training op path on the running statistics): scale = gamma / sqrt(rv + eps), shift = beta - rm * scale, mean = rm, rstd = 1 / sqrt(rv + eps),
// and the backward's two coefficients coef[C][2] = 0 -- bn_bwd_apply then computes gamma * rstd * mask * g.  Writes no buffer.
hipError_t launch_bn_finalize_frozen(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                                     float* scale, float* shift, float* mean, float* rstd, float* coef, hipStream_t st);

// eval: scale/shift of every BatchNorm of a plan in one launch (job table + channel prefix sums in the workspace)
struct BnEvalJob { size_t gamma_off, beta_off, rm_off, rv_off /*floats*/, ss_off /*bytes*/; int C;
                   size_t bias_off; /* floats: bias of the conv in front of this BN, folded into the shift (~0: none) */
                   float eps;       /* this BatchNorm's eps (> 0; 0: the launch's default -- 1e-5 torch, 1e-3 efficientnet_pytorch) */ };
hipError_t launch_bn_finalize_eval_all(const float* params, const float* buffers, void* ws, const BnEvalJob* tab, const unsigned* prefix,
                                       int njobs, unsigned total, float eps, hipStream_t st);

// out = relu?( y*scale+shift [+ res*rscale+rshift | + res] ) [+ post]   (NHWC, T)
struct BnActArgs {
  const void* y; const float* scale; const float* shift;
  const void* res; const float* rscale; const float* rshift;  // pre-activation residual (nullable)
  const void* post;                                           // post-activation addend (nullable)
  void* out; size_t npix; int C; int relu;
  unsigned char* maskbits;   // nullable (training forwards): one byte per 16-byte vector, bit i = (output element i > 0): the ReLU mask the
                             // BatchNorm backward would otherwise re-read the whole output tensor for, twice
};
hipError_t launch_bn_act(int dtype, const BnActArgs& a, hipStream_t st);

// BatchNorm backward.  g = gradient w.r.t. the post value; mask: 0 none, 1 relu(y*scale+shift) > 0,
// 2 out > 0 (materialised tensor `out`).  Pass 1 writes [rows][C][2] partials (sum dz, sum dz*xhat).
struct BnBwdArgs {
  const void* g; const void* y; const void* out;  // out: mask source for mode 2
  const unsigned char* maskbits;                  // mode 2: the forward's saved mask bits (BnActArgs::maskbits) instead of `out` when not null
  const float* scale; const float* shift; const float* mean; const float* rstd; const float* gamma;
  size_t npix; int C; int mask;
  float* slab; int rows;                 // pass 1 output
  float* dgamma; float* dbeta;           // pass 2 output (fp32 grad arena, accumulated)
  float* coef;                           // [C][2]: (sum dz / M, sum dz*xhat / M)
  void* dy;                              // pass 3 output (may alias g)
  double* part; unsigned* counters;      // scratch of the two-level slab reduction (pass 2)
  void* res_grad; int res_store;         // pass 3, optional: the identity shortcut's gradient  res_grad (+)= g * mask  in the same sweep
};                                       // (what masked_accum would re-read g and the mask source for); res_store = 1: first writer

hipError_t launch_bn_bwd_small(int dtype, const BnBwdArgs& a, hipStream_t st);   // reduce + finalize of a small tensor in one launch, double accumulation
hipError_t launch_bn_bwd_reduce(int dtype, const BnBwdArgs& a, hipStream_t st);
hipError_t launch_bn_bwd_finalize(const BnBwdArgs& a, hipStream_t st);
hipError_t launch_bn_bwd_apply(int dtype, const BnBwdArgs& a, hipStream_t st);

// dst (+)= g * (mask ? out > 0 : 1)   (residual / skip gradient); store = 1: first writer, plain store
hipError_t launch_masked_accum(int dtype, void* dst, const void* g, const void* out_mask, size_t n, int store,
                               hipStream_t st);
// dst[n, y, x, c] += sum_{2x2} src[n, 2y+dy, 2x+dx, c]   (gradient of nearest x2 upsample)
hipError_t launch_pool2x2_accum(int dtype, void* dst, const void* src, int N, int H, int W, int C, int store,
                                hipStream_t st);
// per-channel sum over pixels of a NHWC T tensor -> out[c] += sum (bias gradients)
hipError_t launch_channel_sum(int dtype, const void* g, size_t npix, int Cstride, int C, float* out,
                              hipStream_t st);

// maxpool 3x3 s2 p1 (NHWC T)
hipError_t launch_maxpool_fwd(int dtype, const void* in, void* out, unsigned char* idx /*nullable: window position of every maximum*/,
                              int N, int H, int W, int C, hipStream_t st);
hipError_t launch_maxpool_bwd_idx(int dtype, const unsigned char* idx, const void* gout, void* gin, int N, int H, int W, int C, int store,
                                  hipStream_t st);
// stem: NCHW f32 image -> (normalise) -> im2col rows [N, H/2, W/2, KP] T for the k x k stride-2 pad-(k / 2) conv (k = 7 ResNet, 3 RegNet)
hipError_t launch_stem_im2col(int dtype, const float* img, void* col, int N, int H, int W, int KP,
                              const float* mean, const float* stdv, int normalize, hipStream_t st, int ksize = 7, int pad = -1 /* top / left; -1: ksize / 2 */);

// Dice loss (multilabel, from logits) and / or mean binary cross-entropy with logits + confusion counts, logits/target NCHW f32
constexpr int DICE_NS = 4;                                   // doubles per (image, class): I, S, T, BCE sum
enum { LOSS_DICE = 0, LOSS_BCE = 1, LOSS_DICE_BCE = 2 };     // = octseg_loss_kind
struct DiceArgs {
  const float* logits; const float* target; int B, C; size_t HW;
  int loss_kind;       // LOSS_*
  double* sums;        // [1 + B][C][DICE_NS]: I, S, T, BCE totals, then per-image replicas (zeroed by the launcher)
  long long* stats;    // [B][C][4]: tp, fp, fn, tn (zeroed by the launcher), nullable
  float* loss;         // scalar
};
hipError_t launch_dice_fwd(const DiceArgs& a, hipStream_t st);
// dL/dz written as NHWC T rows padded to CP channels (zeros beyond C)
hipError_t launch_dice_bwd(int dtype, const DiceArgs& a, float grad_scale, void* dlogits, int CP,
                           hipStream_t st);

// weight packing: master fp32 [taps][O][I] -> LDS-image slabs of a conv launch.  transpose = 0: rows are
// O, K runs over I (forward);  transpose = 1: rows are I, K runs over O (data gradient); K is padded
// to Kpad (>= the contraction length the launch uses).
// oscale (forward images only, nullable): W'[o][i] = W[o][i] * oscale[o] in f32 before the rounding to T -- launch_pack_all's eval fold.
hipError_t launch_pack_weight_image(int dtype, const float* w, void* img, int taps, int O, int I, int transpose,
                                    const ConvPackInfo& p, hipStream_t st, const float* oscale = nullptr);

// every weight image of a plan in one launch (job table + prefix sums live in the workspace)
struct PackJob { size_t src_off /*floats*/, dst_off /*bytes*/; int taps, O, I, transpose, BN, RB, nchunks, ntiles;
                 size_t scale_off; /* bytes in the workspace: eval scale[O] of the BatchNorm behind this conv, folded into the
                                      forward image when packing for eval (~0: none) */
                 int src_I;        /* row length of the SOURCE weight when the image covers a channel slice of it (0: I) */
                 int src_c0;       /* first source channel of that slice */
                 int tied;         /* 2: the masked data-gradient image of the same kernel (taps == 9 offsets, K = 4 O: dy's four parity planes);
                                      1: taps == 16, the image is the 4x4 stride-2 kernel that a nearest-x2 upsample followed by the 3x3
                                         source is equal to: K4[u][v] = sum of W3[r][s] over r in A(u), s in A(v), A(k) = [max(0, 2 - k), min(2, 3 - k)] */ };
// gradient of the tied image back into the 3x3 weight it was derived from: dW3[t][o][i] += (i < Ca ? sum of dK4 over the (u, v) whose
// A(u) x A(v) holds tap t : dW3s[t][o][i - Ca]);  dK4 [16][O][Ca], dW3s [9][O][Cs] (nullptr when Cs == 0), dW3 [9][O][Ca + Cs], all f32
hipError_t launch_tied_fold(const float* dK4, const float* dW3s, float* dW3, int O, int Ca, int Cs, hipStream_t st);
hipError_t launch_pack_all(int dtype, const float* params, void* ws, const PackJob* tab, const unsigned long long* prefix, int njobs,
                           unsigned long long total, int fold, hipStream_t st);

// fpn.hip: what the FPN decoder (smp decoders/fpn; reference configs/tune.yaml:9-18) adds -- GroupNorm(32) + ReLU (+ bilinear x2,
// align_corners=True) forward / backward, the resample's adjoint, nearest-x2 fill, merge-add + Dropout2d, x4 bilinear of the logits.
struct GnArgs {
  const void* y;            // raw conv output [N][HW][C] T
  const void* g; void* dy;  // backward: gradient w.r.t. relu(gn(y)) at y's resolution in, gradient w.r.t. y out (may alias)
  void* out;                // forward: relu(gn(y)), resampled
  const float* gamma; const float* beta; float* dgamma; float* dbeta;
  float* part;              // [N][S][C][2] partial sums (S = gn_num_slabs(HW))
  float* ss;                // [N][C][2]: scale = gamma * rstd, shift = beta - mean * scale
  float* stat;              // [N][G][2]: mean, rstd
  float* coef;              // [N][G][2]: backward group means
  size_t HW; int C, G, cpg; float eps;
};
int gn_num_slabs(size_t HW);
hipError_t launch_gn_forward(int dtype, const GnArgs& a, int N, int H, int W, int up, hipStream_t st);
hipError_t launch_gn_backward(int dtype, const GnArgs& a, int N, hipStream_t st);
hipError_t launch_bilinear_adjoint(int dtype, const void* gout, void* gin, int N, int H, int W, int C, int up, hipStream_t st);   // gin [N][H][W][C] <- gout [N][H*up][W*up][C]
hipError_t launch_up2_fill(int dtype, const void* in, void* out, int N, int H, int W, int C, hipStream_t st);                    // out [N][2H][2W][C] = nearest x2 of in
hipError_t launch_merge_drop(int dtype, const void* a0, const void* a1, const void* a2, const void* a3, const float* m, float mscale, void* out,
                             int N, size_t HW, int C, hipStream_t st);
hipError_t launch_drop_bwd(int dtype, const void* gout, const float* m, float mscale, void* gin, int N, size_t HW, int C, hipStream_t st);
hipError_t launch_bilinear_nchw(const float* z, float* out, int NC, int H, int W, int up, hipStream_t st);                          // NCHW f32, align_corners=True

// ---- DeepLabV3+ (deeplab.hip)
hipError_t launch_parity_permute(int dtype, const void* src, void* dst, int N, int H, int W, int C, int to_coarse, int accum, hipStream_t st);   // fine [N][H][W][C] <-> coarse [4N][H/2][W/2][C]
hipError_t launch_dw_conv(int dtype, const void* in, int inC, int ic0, void* out, int outC, int oc0, const float* w, int wC, int wc0, int N, int H,
                          int W, int C, int dil, int flip, int accum, hipStream_t st);                                                          // depthwise 3x3, dilation = padding = dil
hipError_t launch_dw_wgrad(int dtype, const void* in, int inC, int ic0, const void* gout, int goC, int oc0, float* dw, int wC, int wc0, int N, int H,
                           int W, int C, int dil, hipStream_t st);
hipError_t launch_image_sum(int dtype, const void* in, void* out, int N, int HW, int C, float div, hipStream_t st);                              // out [N][C] = sum over pixels / div
hipError_t launch_image_bcast(int dtype, const void* in, void* out, int N, int HW, int C, float scale, int accum, hipStream_t st);              // out [N][HW][C] (+)= scale * in [N][C]
hipError_t launch_drop_elem(int dtype, const void* in, const float* keep, float mscale, void* out, size_t numel, hipStream_t st);                // out = in * keep * mscale
hipError_t launch_bilinear_up(int dtype, const void* in, void* out, int N, int H, int W, int C, int up, hipStream_t st);                         // NHWC, align_corners=True
// ---- DeepLabV3 (deeplab.hip): dense dilated convs as plain 3x3 convs on a mosaic of the rate^2 sub-grids
hipError_t launch_mosaic(int dtype, const void* src, void* dst, int N, int H, int W, int C, int r, int to_mosaic, int accum, hipStream_t st);      // fine [N][H][W][C] <-> mosaic [N][r (hs + 1) + 1][r (ws + 1) + 1][C]
hipError_t launch_tensor_stats(int dtype, const void* y, size_t npix, int C, float* slab, int rows, hipStream_t st);   // (any C: channel chunks of <= 256 vectors)                            // slab [rows][C][2] = (sum, sum of squares)
// ---- PSPNet (deeplab.hip)
hipError_t launch_bin_mean(int dtype, const void* in, void* out, int N, int H, int W, int C, int k, hipStream_t st);                              // AdaptiveAvgPool2d((k, k)): out [N][k][k][C]
hipError_t launch_bin_mean_bwd(int dtype, const void* gout, void* gin, int N, int H, int W, int C, int k, int accum, hipStream_t st);
hipError_t launch_bilinear_resize(int dtype, const void* in, void* out, int N, int IH, int IW, int OH, int OW, int C, hipStream_t st);          // align_corners=True, any sizes
hipError_t launch_bilinear_resize_adjoint(int dtype, const void* gout, void* gin, int N, int IH, int IW, int OH, int OW, int C, hipStream_t st);
bool bilinear_adjoint_grid(long long npx, int& gy, int& gz);   // its one-workgroup-per-source-pixel grid, grid.y x grid.z = npx exactly; false: no such pair
hipError_t launch_relu(int dtype, const void* in, const void* mask, void* out, size_t numel, hipStream_t st);                                   // mask == nullptr: max(in, 0); else in where mask > 0

// serving: out[n][y][x][out_ch] = (logits[n][ch] nearest-resized to OH x OW) > 0, out has OC channels per pixel
hipError_t launch_mask_assemble(const float* logits, int N, int C, int SH, int SW, int ch, float* out, int OH, int OW, int OC, int out_ch,
                                const int* rows, const int* cols, hipStream_t st);

// serving, voted (vote.hip): one mask from M members (folds x views), the mean probability, the dissent map and per-frame counts in one launch.
// The member table travels in the kernel argument by value.  view = a + 2 b + 4 t (transpose, then rows reversed, then columns reversed); mode 0
// soft (mean probability > 0.5), 1 majority (a tie is not set); prob / dissent / stats are optional (null = skipped), stats is cleared on the stream
constexpr int VOTE_MAX_MEMBERS = 64;
struct VoteArgs {
  const float* z[VOTE_MAX_MEMBERS]; int classes[VOTE_MAX_MEMBERS], ch[VOTE_MAX_MEMBERS], view[VOTE_MAX_MEMBERS];
  int M, N, H, W, mode;
  float* out; int OH, OW, OC, out_ch;
  const int* rows; const int* cols;
  float* prob; uint8_t* dissent; int* stats;
};
hipError_t launch_vote_assemble(const VoteArgs& a, hipStream_t st);

// operating curves (curves.hip): hist int32 [N][classes][2][CURVE_BINS], label-major (0 = truth-negative, 1 = truth-positive pixels, target != 0),
// bin = clamp((int)ceilf(sigmoid_acc(z) * 256) - 1, 0, 255); cleared on the stream, then one launch.  N * classes <= 65535, H * W < 2^31
constexpr int CURVE_BINS = 256;
hipError_t launch_logit_histogram(const float* logits, const float* target, int N, int classes, int H, int W, int* hist, hipStream_t st);

// on-GPU training augmentation (augment.hip): AUG_NPARAM floats per frame, layout in the kernel's header comment
constexpr int AUG_NPARAM = 36;
hipError_t launch_augment(const float* img, const float* mask, float* img_out, float* mask_out, const float* params, int B, int C, int H,
                          int W, hipStream_t st);

// uint8 frames / masks -> the nets' float32 NCHW batch (ingest.hip): cv2.resize's 8-bit INTER_LINEAR (INTER_AREA at exactly 2x in both axes) and
// INTER_NEAREST + class-channel select, from host-made tap tables.  variant 0 = the shipped kernels (ingest_image_kernel, ingest_mask_kernel),
// 1 = the one-thread-per-pixel gather forms (measurement yardstick)
hipError_t launch_ingest_image(const uint8_t* src, int B, int Hs, int Ws, int swap_rb, float* out, int Hd, int Wd, const int* xtab,
                               const int* ytab, int variant, hipStream_t st);
hipError_t launch_ingest_mask(const uint8_t* src, int B, int Hs, int Ws, int Cs, const int* ch_ids, int C, float* out, int Hd, int Wd,
                              const int* rows, const int* cols, int variant, hipStream_t st);

// save_results on the GPU (render.hip): closing, ring, blur, the two pastes per class and the colour mask in one launch; uint8 HWC in and out
hipError_t launch_render_results(const float* stack, const uint8_t* frames, int N, int H, int W, int SC, const int* class_ch,
                                 const uint8_t* class_rgb, int C, const uint8_t* alpha_tab, int ring_alpha, int iters, uint8_t* overlay,
                                 uint8_t* cmask, hipStream_t st);

// the per-epoch sample strips of the training loop (panels.hip): frame | ground truth | prediction as RGB bytes plus the two label maps, one launch
// per group of frames that share a ground-truth source size; labels may be null
hipError_t launch_epoch_panels(const float* frames, const float* logits, const uint8_t* gt, int N, int S, int C, int Hs, int Ws, int SC,
                               const int* rows, const int* cols, const int* gt_ch, const uint8_t* class_rgb, const uint8_t* class_ids,
                               uint8_t* panels, uint8_t* labels, hipStream_t st);

// the app's per-pullback measurements (measure.hip): set pixels per slice and channel, and calculate_object_thickness's ray walk per slice,
// channel and degree from the host's pixel table; clears counts, then two launches
hipError_t launch_stack_measure(const float* stack, int N, int H, int W, int SC, const int* ray_pix, const int* ray_len, int R, int* counts,
                                int* radii, hipStream_t st);

// the polar plaque profile (polar.hip): the same ray walk carried to the end of every ray -- first entry, first exit, last set step, set steps and
// runs per slice, channel (at most 8) and degree, optionally the label map [N][360][R] with a bit per channel; one launch.  launch_frames_unwrap:
// the table as a nearest gather of uint8 frames [N][H][W][C], C = 1 | 3, into [N][360][R][C], zeros past the ray's end; one launch (none when R == 0)
hipError_t launch_stack_polar(const float* stack, int N, int H, int W, int SC, const int* ray_pix, const int* ray_len, int R, int* prof,
                              uint8_t* map, hipStream_t st);
hipError_t launch_frames_unwrap(const uint8_t* frames, int N, int H, int W, int C, const int* ray_pix, const int* ray_len, int R, uint8_t* out,
                                hipStream_t st);

// lumen geometry (shape.hip): launch_stack_moments -- int64 [N][SC][12] raw moments to second order, bounding box and crack perimeter of every
// plane; one initialising launch, then one streaming pass.  launch_moment_origins -- int32 [N][SC][3] = the centroid rounded to a pixel and whether
// the plane is set there, from the plane's own moments (ref_channel < 0) or from channel ref_channel of the slice; one tiny launch.
// launch_stack_polar_at -- polar.hip's five integers per slice, channel (at most 8) and degree from origins[n][c] along ray_off [360][R][2], and
// the number of steps inside the frame; one launch
constexpr int SHAPE_MOMENT_FIELDS = 12;
constexpr int SHAPE_MAX_EXTENT = 32768;                     // H, W <= 2^15 and H * W < 2^31: every sum stays below 2^60
hipError_t launch_stack_moments(const float* stack, int N, int H, int W, int SC, long long* mom, hipStream_t st);
hipError_t launch_moment_origins(const float* stack, const long long* mom, int N, int H, int W, int SC, int ref_channel, int* origins,
                                 hipStream_t st);
hipError_t launch_stack_polar_at(const float* stack, int N, int H, int W, int SC, const int* origins, const int* ray_off, int R, int* prof,
                                 int* length, hipStream_t st);

// mask clean-up (components.hip): connected components of every (slice, channel) plane by union-find on bit planes, the 8 largest with their
// bounding boxes, keep-largest / min-area filter, hole fill (the same labelling on the complement, 4-connected) and the reference's
// smooth_mask chain.  scratch: components_scratch_bytes(N * C, H, W) device bytes; labels / ncomp / top are optional (null = skipped)
size_t components_scratch_bytes(size_t planes, int H, int W);
hipError_t launch_stack_components(const float* stack, int N, int H, int W, int C, void* scratch, int* labels, int* ncomp, int* top, hipStream_t st);
hipError_t launch_stack_cleanup(const float* stack, int N, int H, int W, int C, int smooth_k, int keep, int min_area, int fill_holes, void* scratch,
                                float* out, int* ncomp, int* top, hipStream_t st);

// mask outlines (contours.hip): the crack contours of every (slice, channel) plane -- closed polygons along pixel sides, found by pointer jumping
// over the edges' predecessor links, not by following them.  launch_stack_contour_counts: int64 [N][C][2] = edges, contour vertices, one memset and
// one pass over the stack.  launch_stack_contours: ncont [N][C], table [contours][CONTOUR_FIELDS], vertices [.][2]; scratch:
// contours_scratch_bytes(N * C, H, W, edge_capacity) device bytes; contours_rounds: the jump launches a call enqueues
constexpr int CONTOUR_FIELDS = 10;
size_t contours_scratch_bytes(size_t planes, int H, int W, size_t edge_capacity);
int contours_rounds(int H, int W, size_t edge_capacity);
hipError_t launch_stack_contour_counts(const float* stack, int N, int H, int W, int C, long long* counts, hipStream_t st);
hipError_t launch_stack_contours(const float* stack, int N, int H, int W, int C, void* scratch, int edge_capacity, int contour_capacity,
                                 int vertex_capacity, int* ncont, int* table, int* vertices, int* overflow, hipStream_t st);

// lesions in 3-D (lesions.hip): the connected components of every channel's volume across the slices (8-connected inside a slice; between slices
// the same pixel only, or with full != 0 the 3 x 3), the 32 largest with their extents, the per-slice area profile, and the voxel / rank / slice-span
// filter.  scratch: lesions_scratch_bytes(C, N, H, W) device bytes; labels / nles / top / profile are optional (null = skipped)
size_t lesions_scratch_bytes(size_t channels, int N, int H, int W);
hipError_t launch_volume_components(const float* stack, int N, int H, int W, int C, int full, void* scratch, int* labels, int* nles, int* top,
                                    int* profile, hipStream_t st);
hipError_t launch_volume_cleanup(const float* stack, int N, int H, int W, int C, int full, int keep, int min_voxels, int min_slices, void* scratch,
                                 float* out, int* nles, int* top, hipStream_t st);

// predicted against annotated lesions (match.hip): both stacks labelled and ranked as above, then per channel the 33 x 33 table of the voxels both
// set by the rank of their lesion on either side (32 = beyond the 32 listed) and |P & T|, |P|, |T| per slice.  scratch: match_scratch_bytes(C, N,
// H, W) device bytes; nles int32 [C][2], overlap int32 [C][33][33]; top int32 [C][2][32][8] and frames int32 [C][N][3] are optional
size_t match_scratch_bytes(size_t channels, int N, int H, int W);
hipError_t launch_volume_match(const float* pred, const float* truth, int N, int H, int W, int C, int full, void* scratch, int* nles, int* top,
                               int* overlap, int* frames, hipStream_t st);

// boundary distances (distance.hip): the boundary of every plane, the exact squared Euclidean distance map (column pass + row minimum in LDS), and
// per (slice, pair of channels) the counts, the keyed list of d2 at the query pixels, and their minimum with its location.  scratch:
// distance_scratch_bytes(N, H, W, Ca, Cb, pairs) device bytes (one-stack calls: Cb = 0, pairs = 0).  part / to: 0 set, 1 clear, 2 boundary
size_t distance_scratch_bytes(size_t N, int H, int W, int Ca, int Cb, int pairs);
hipError_t launch_stack_boundary(const float* stack, int N, int H, int W, int C, void* scratch, float* out, hipStream_t st);
hipError_t launch_stack_distance(const float* stack, int N, int H, int W, int C, int to, void* scratch, int* d2, hipStream_t st);
hipError_t launch_pair_distance_counts(const float* src, const float* dst, int N, int H, int W, int Ca, int Cb, const int* pairs, int P, int src_part,
                                       int dst_part, void* scratch, int* counts, int* overlap, hipStream_t st);
hipError_t launch_pair_distance_query(const float* src, const float* dst, int N, int H, int W, int Ca, int Cb, const int* pairs, int P, int src_part,
                                      int dst_part, void* scratch, long long seg0, const long long* offsets, long long* keys, long long capacity,
                                      int* overflow, unsigned long long* minout, hipStream_t st);
// the same over the volume a channel's N planes form, slices slice_step pixels apart (distance.hip): the 6-neighbour boundary,
// the per-slice map of a band of `rows` rows of all slices plus a pass along the slice axis, band after band; a segment is a pair, counts are
// int64 [P][2] / [P][3].  scratch: volume_distance_scratch_bytes(N, H, W, Ca, Cb, pairs, rows) device bytes, rows = 0 for boundary and counts;
// volume_distance_rows: the most rows (1 .. H) that fit `bytes`, 0 when one row does not
size_t volume_distance_scratch_bytes(size_t N, int H, int W, int Ca, int Cb, int pairs, int rows);
int volume_distance_rows(size_t bytes, size_t N, int H, int W, int Ca, int Cb, int pairs);
hipError_t launch_volume_boundary(const float* stack, int N, int H, int W, int C, void* scratch, float* out, hipStream_t st);
hipError_t launch_volume_distance(const float* stack, int N, int H, int W, int C, int to, int slice_step, int rows, void* scratch, int* d2,
                                  hipStream_t st);
hipError_t launch_volume_pair_counts(const float* src, const float* dst, int N, int H, int W, int Ca, int Cb, const int* pairs, int P, int src_part,
                                     int dst_part, void* scratch, long long* counts, long long* overlap, hipStream_t st);
hipError_t launch_volume_pair_query(const float* src, const float* dst, int N, int H, int W, int Ca, int Cb, const int* pairs, int P, int src_part,
                                    int dst_part, int slice_step, int rows, void* scratch, long long seg0, const long long* offsets, long long* keys,
                                    long long capacity, int* overflow, unsigned long long* minout, hipStream_t st);
// signed squared distance maps and the blend of two of them by integer weights (distance.hip): sd2 int32 [N][C][H][W], + inside,
// - outside, never 0; plan device int32 [M][6] = (channel, out_slice, lo, hi, w_lo, w_hi), out f32 [Nout][H][W][C], made (may be null) int32 [M].
// scratch: signed_distance_scratch_bytes(N, H, W, C) device bytes
size_t signed_distance_scratch_bytes(size_t N, int H, int W, int C);
hipError_t launch_stack_signed_distance(const float* stack, int N, int H, int W, int C, void* scratch, int* sd2, hipStream_t st);
hipError_t launch_signed_blend(const int* sd2, int K, int H, int W, int C, const int* plan, int M, float* out, int Nout, int* made, hipStream_t st);

// centrelines (skeleton.hip): Guo and Hall's thinning of every plane by one workgroup per plane, all passes in one launch -- from
// the padded LDS image of planepass.h when skeleton_fits_lds(H, W) and force_global == 0, else over ping-pong images in scratch --, and the census
// int32 [N][C][6] = set, skeleton, end, junction, isolated pixels, passes.  scratch: skeleton_scratch_bytes(N, H, W, C) device bytes; out / census
// are optional (null = skipped)
size_t skeleton_scratch_bytes(size_t N, int H, int W, int C);
bool skeleton_fits_lds(int H, int W);
hipError_t launch_stack_skeleton(const float* stack, int N, int H, int W, int C, int force_global, void* scratch, float* out, int* census,
                                 hipStream_t st);

// centreline pruning (prune.hip): of every plane of a skeleton stack the side branches of at most `spur` pixels removed,
// `trim` pixels taken off every end that is left, a component this would erase returned whole -- one workgroup per plane, all phases in one launch,
// from the padded LDS image of planepass.h when skeleton_fits_lds(H, W) and force_global == 0, else over images in scratch --, and the census
// int32 [N][C][9] = input pixels, output pixels, tips, end, junction, isolated points, orthogonal links, diagonal links, restored pixels.  scratch:
// prune_scratch_bytes(N, H, W, C) device bytes; out / census are optional (null = skipped)
size_t prune_scratch_bytes(size_t N, int H, int W, int C);
hipError_t launch_stack_prune(const float* skel, int N, int H, int W, int C, int spur, int trim, int force_global, void* scratch, float* out,
                              int* census, hipStream_t st);

// raw pullback volumes (volume.hip): per-slice min / max + cv2.normalize(NORM_MINMAX, CV_8U) + channel order into uint8 [S][H][W][3] (one init,
// two launches), and Pillow's 8-bit two-pass resample from host tables (a launch per axis that changes length; a copy when none does)
hipError_t launch_volume_normalize(const void* src, int src_u16, int S, int H, int W, int C, int swap_rb, unsigned* minmax, uint8_t* dst,
                                   hipStream_t st);
hipError_t launch_resize_pil_u8(const uint8_t* src, int S, int H, int W, int C, uint8_t* tmp, uint8_t* dst, int oh, int ow, const int* xbounds,
                                const int* xkk, int xksize, const int* ybounds, const int* ykk, int yksize, hipStream_t st);

// class activation maps (cam.hip).  launch_cam_seed: dL/dlogits NCHW f32 [B][C][HW] -> NHWC T rows padded to CP channels (launch_dice_bwd's layout).
hipError_t launch_cam_seed(int dtype, const float* seed, void* dlogits, int B, int C, size_t HW, int CP, hipStream_t st);
// launch_cam_maps: A, G NHWC T [N][h][w][K] -> maps f32 [N][S][S] in [0, 1] and, where the pointers are set, the thresholded map, the confusion
// counts against a ground-truth plane and the JET overlay (see include/octseg.h, octseg_cam_maps).  scratch: cam_scratch_bytes() device bytes.
struct CamArgs {
  const void* A; const void* G; int N, h, w, K, method, S;
  void* scratch; float* maps;
  float threshold; uint8_t* bin;
  const uint8_t* gt; int gt_h, gt_w; const int* row_index; const int* col_index; int* counts;
  const float* frames; const uint8_t* jet; double image_weight; uint8_t* overlay;
};
size_t cam_scratch_bytes(int N, int h, int w, int K);
hipError_t launch_cam_maps(int dtype, const CamArgs& a, hipStream_t st);
hipError_t launch_cam_overlay(const float* maps, const float* frames, const uint8_t* jet, int N, int S, double image_weight, uint8_t* overlay,
                              void* acc /* 16 N device bytes */, hipStream_t st);

// fused optimizers over the flat fp32 arenas
struct OptArgs {
  float* p; const float* g; float* m; float* v; size_t n;
  int kind;  // 0 SGD, 1 Adam, 2 RMSprop, 3 RAdam
  float lr, wd, beta1, beta2, eps, alpha, momentum; int step; float grad_scale;
};
hipError_t launch_optim_step(const OptArgs& a, hipStream_t st);

}  // namespace octseg
