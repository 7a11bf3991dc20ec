// sweep_api.cpp -- octseg_sweep_op: one C-ABI door to the HBM-bound NHWC sweep launchers (elementwise.hip, fpn.hip, deeplab.hip, se.hip,
// pan.hip's add2), so that each kernel can be pinned against a float64 reference alone (tests/test_gpu_sweeps.py) instead of only through a
// whole network.  The entry fills the launcher's arguments and calls the launcher on the given stream; it refuses, before any launch, what
// the kernel cannot take.  Buffer sizes are the caller's contract (oct_segmentation_amd/sweeps.py checks them): see include/octseg.h.
#include "plan_internal.h"

#include <cstring>
#include <initializer_list>

using namespace octseg;
using namespace octseg::detail;

namespace {

// per op: pointer count, bit i = pointer i must not be null, integer / float argument counts, does the launcher take f16
struct SweepSpec { int nptrs; unsigned required; int niargs, nfargs; bool f16; const char* name; };

constexpr unsigned bits(std::initializer_list<int> l) { unsigned m = 0; for (int i : l) m |= 1u << i; return m; }

// pointer slots of the four BatchNorm-backward ops (one layout = BnBwdArgs)
enum { BW_G, BW_Y, BW_OUT, BW_MASKBITS, BW_SCALE, BW_SHIFT, BW_MEAN, BW_RSTD, BW_GAMMA, BW_SLAB, BW_DGAMMA, BW_DBETA, BW_COEF, BW_DY, BW_PART,
       BW_COUNTERS, BW_RES_GRAD, BW_NPTRS };

const SweepSpec SPECS[OCTSEG_SWEEP_NUM_OPS] = {
  /* BN_FINALIZE_TRAIN  */ {11, 0x7ffu, 2, 3, true, "bn_finalize_train"},
  /* BN_FINALIZE_SMALL  */ {9, 0x1ffu, 2, 2, false, "bn_finalize_small"},
  /* BN_FINALIZE_EVAL   */ {6, 0x3fu, 1, 1, true, "bn_finalize_eval"},
  /* BN_FINALIZE_FROZEN */ {9, 0x1ffu, 1, 1, true, "bn_finalize_frozen"},
  /* BN_ACT             */ {9, bits({0, 7}), 3, 0, true, "bn_act"},
  /* BN_BWD_SMALL       */ {BW_NPTRS, bits({BW_G, BW_Y, BW_SCALE, BW_SHIFT, BW_MEAN, BW_RSTD, BW_GAMMA, BW_DGAMMA, BW_DBETA, BW_COEF, BW_DY}), 5, 0, false, "bn_bwd_small"},
  /* BN_BWD_REDUCE      */ {BW_NPTRS, bits({BW_G, BW_Y, BW_SCALE, BW_SHIFT, BW_MEAN, BW_RSTD, BW_SLAB}), 5, 0, false, "bn_bwd_reduce"},
  /* BN_BWD_FINALIZE    */ {BW_NPTRS, bits({BW_SLAB, BW_DGAMMA, BW_DBETA, BW_COEF, BW_PART, BW_COUNTERS}), 5, 0, false, "bn_bwd_finalize"},
  /* BN_BWD_APPLY       */ {BW_NPTRS, bits({BW_G, BW_Y, BW_SCALE, BW_SHIFT, BW_MEAN, BW_RSTD, BW_GAMMA, BW_COEF, BW_DY}), 5, 0, false, "bn_bwd_apply"},
  /* MASKED_ACCUM       */ {3, bits({0, 1}), 2, 0, false, "masked_accum"},
  /* POOL2X2_ACCUM      */ {2, 0x3u, 5, 0, false, "pool2x2_accum"},
  /* UP2_FILL           */ {2, 0x3u, 4, 0, true, "up2_fill"},
  /* RELU               */ {3, bits({0, 2}), 1, 0, true, "relu"},
  /* ADD2               */ {3, 0x7u, 1, 0, true, "add2"},
  /* DROP_ELEM          */ {3, bits({0, 2}), 1, 1, true, "drop_elem"},
  /* MERGE_DROP         */ {6, bits({0, 1, 2, 3, 5}), 3, 1, true, "merge_drop"},
  /* DROP_BWD           */ {3, bits({0, 2}), 3, 1, true, "drop_bwd"},
  /* CHANNEL_SUM        */ {2, 0x3u, 3, 0, false, "channel_sum"},
  /* TENSOR_STATS       */ {2, 0x3u, 3, 0, false, "tensor_stats"},
  /* MAXPOOL_FWD        */ {3, 0x3u, 4, 0, true, "maxpool_fwd"},
  /* MAXPOOL_BWD_IDX    */ {3, 0x7u, 5, 0, false, "maxpool_bwd_idx"},
  /* BILINEAR_RESIZE    */ {2, 0x3u, 6, 0, true, "bilinear_resize"},
  /* BILINEAR_RESIZE_ADJ*/ {2, 0x3u, 6, 0, false, "bilinear_resize_adjoint"},
  /* BILINEAR_ADJOINT   */ {2, 0x3u, 5, 0, false, "bilinear_adjoint"},
  /* BIN_MEAN           */ {2, 0x3u, 5, 0, true, "bin_mean"},
  /* BIN_MEAN_BWD       */ {2, 0x3u, 6, 0, false, "bin_mean_bwd"},
  /* IMAGE_SUM          */ {2, 0x3u, 3, 1, true, "image_sum"},
  /* IMAGE_BCAST        */ {2, 0x3u, 4, 1, true, "image_bcast"},
  /* SE_GATE            */ {4, bits({0, 1, 2}), 4, 0, true, "se_gate"},
  /* SE_DGATE           */ {7, bits({0, 1, 2, 3, 4}), 3, 0, false, "se_dgate"},
  /* PARITY_PERMUTE     */ {2, 0x3u, 6, 0, true, "parity_permute"},
  /* MOSAIC             */ {2, 0x3u, 7, 0, true, "mosaic"},
  /* DW_CONV            */ {3, 0x7u, 13, 0, true, "dw_conv"},
  /* DW_WGRAD           */ {3, 0x7u, 11, 0, false, "dw_wgrad"},
  /* CAM_SEED           */ {2, 0x3u, 4, 0, false, "cam_seed"},
  /* DWG_FWD            */ {3, 0x7u, 9, 0, true, "dwg_fwd"},
  /* DWG_BWD_DATA       */ {3, 0x7u, 10, 0, false, "dwg_bwd_data"},
  /* DWG_BWD_W          */ {3, 0x7u, 9, 0, false, "dwg_bwd_w"},
  /* BNX_FWD            */ {6, bits({0, 5}), 4, 0, true, "bnx_fwd"},
  /* BNX_BWD            */ {6, bits({4, 5}), 4, 0, false, "bnx_bwd"},
  /* DICE_BWD           */ {4, 0xfu, 5, 1, false, "dice_bwd"},
  /* GN_FORWARD         */ {7, 0x7fu, 6, 1, true, "gn_forward"},
  /* GN_BACKWARD        */ {10, 0x3ffu, 4, 0, false, "gn_backward"},
  /* SEFC_FWD           */ {7, 0x7fu, 4, 0, true, "sefc_fwd"},
  /* SEFC_BWD           */ {11, 0x7fu, 4, 0, false, "sefc_bwd"},
};

bool fits_int(long long v) { return v >= 0 && v <= 0x7fffffffll; }

}  // namespace

extern "C" int octseg_sweep_op(int op, int dtype, const void* const* ptrs, int nptrs, const long long* iargs, int niargs, const double* fargs,
                               int nfargs, void* stream) {
  if (op < 0 || op >= OCTSEG_SWEEP_NUM_OPS) return fail(OCTSEG_BAD_ARG, "sweep_op: unknown op");
  const SweepSpec& S = SPECS[op];
  const std::string who = std::string("sweep_op ") + S.name + ": ";
  if (dtype != OCTSEG_F32 && dtype != OCTSEG_BF16 && dtype != OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, who + "dtype must be f32, bf16 or f16");
  if (dtype == OCTSEG_F16 && !S.f16) return fail(OCTSEG_BAD_DTYPE, who + "a training-only sweep has no f16 form (f16 is the serving dtype)");
  if (nptrs != S.nptrs || niargs != S.niargs || nfargs != S.nfargs || !ptrs || !iargs || (nfargs > 0 && !fargs))
    return fail(OCTSEG_BAD_ARG, who + "argument counts do not match the op (include/octseg.h)");
  for (int i = 0; i < nptrs; ++i) {
    if (!ptrs[i] && ((S.required >> i) & 1u)) return fail(OCTSEG_BAD_ARG, who + "null required pointer");
    if ((uintptr_t)ptrs[i] & 15) return fail(OCTSEG_BAD_ARG, who + "every pointer must be 16-byte aligned");
  }
  for (int i = 0; i < niargs; ++i)
    if (!fits_int(iargs[i])) return fail(OCTSEG_BAD_SHAPE, who + "integer argument negative or beyond 2^31 - 1");
  const int vec = ev_vec(dtype);
  hipStream_t st = (hipStream_t)stream;
  auto P = [&](int i) { return const_cast<void*>(ptrs[i]); };
  auto F = [&](int i) { return (float*)const_cast<void*>(ptrs[i]); };
  auto I = [&](int i) { return (int)iargs[i]; };
  auto bad_shape = [&](const char* m) { return fail(OCTSEG_BAD_SHAPE, who + m); };
  auto bad_arg = [&](const char* m) { return fail(OCTSEG_BAD_ARG, who + m); };
  // a tensor of n >= 1 pixels with C channels in whole 16-byte vectors
#define NEED_TENSOR(npix_, C_) do { if ((npix_) < 1 || (C_) < 1 || (C_) % vec != 0) return bad_shape("empty tensor, or C not a multiple of the 16-byte vector"); } while (0)

  switch (op) {
    case OCTSEG_SWEEP_BN_FINALIZE_TRAIN: {
      const int rows = I(0), C = I(1);
      if (rows < 1 || C < 1 || !(fargs[0] >= 1.0)) return bad_shape("rows, C and count must be at least 1");
      HIPCHK(launch_bn_finalize_train(F(0), rows, C, fargs[0], F(1), F(2), F(3), F(4), (float)fargs[1], (float)fargs[2], F(5), F(6), F(7), F(8),
                                      (double*)P(9), (unsigned*)P(10), st));
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_BN_FINALIZE_SMALL: {
      const int count = I(0), C = I(1);
      if (count < 1 || count > BN_SMALL_COUNT || C < 1) return bad_shape("1 <= count <= 1024 values per channel, C >= 1");
      HIPCHK(launch_bn_finalize_small(dtype, P(0), count, C, F(1), F(2), F(3), F(4), (float)fargs[0], (float)fargs[1], F(5), F(6), F(7), F(8), st));
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_BN_FINALIZE_EVAL:
      if (I(0) < 1) return bad_shape("C >= 1");
      HIPCHK(launch_bn_finalize_eval(I(0), F(0), F(1), F(2), F(3), (float)fargs[0], F(4), F(5), st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_BN_FINALIZE_FROZEN:
      if (I(0) < 1) return bad_shape("C >= 1");
      HIPCHK(launch_bn_finalize_frozen(I(0), F(0), F(1), F(2), F(3), (float)fargs[0], F(4), F(5), F(6), F(7), F(8), st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_BN_ACT: {
      BnActArgs a;
      a.y = P(0); a.scale = F(1); a.shift = F(2); a.res = P(3); a.rscale = F(4); a.rshift = F(5); a.post = P(6); a.out = P(7);
      a.maskbits = (unsigned char*)P(8);
      a.npix = (size_t)iargs[0]; a.C = I(1); a.relu = I(2) != 0;
      NEED_TENSOR(iargs[0], a.C);
      if ((a.scale == nullptr) != (a.shift == nullptr)) return bad_arg("scale and shift come together");
      if ((a.rscale == nullptr) != (a.rshift == nullptr) || (a.rscale && !a.res)) return bad_arg("rscale and rshift come together, with res");
      HIPCHK(launch_bn_act(dtype, a, st));
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_BN_BWD_SMALL: case OCTSEG_SWEEP_BN_BWD_REDUCE: case OCTSEG_SWEEP_BN_BWD_FINALIZE: case OCTSEG_SWEEP_BN_BWD_APPLY: {
      BnBwdArgs a;
      memset(&a, 0, sizeof(a));
      a.g = P(BW_G); a.y = P(BW_Y); a.out = P(BW_OUT); a.maskbits = (const unsigned char*)P(BW_MASKBITS);
      a.scale = F(BW_SCALE); a.shift = F(BW_SHIFT); a.mean = F(BW_MEAN); a.rstd = F(BW_RSTD); a.gamma = F(BW_GAMMA);
      a.slab = F(BW_SLAB); a.dgamma = F(BW_DGAMMA); a.dbeta = F(BW_DBETA); a.coef = F(BW_COEF); a.dy = P(BW_DY);
      a.part = (double*)P(BW_PART); a.counters = (unsigned*)P(BW_COUNTERS); a.res_grad = P(BW_RES_GRAD);
      a.npix = (size_t)iargs[0]; a.C = I(1); a.mask = I(2); a.rows = I(3); a.res_store = I(4) != 0;
      NEED_TENSOR(iargs[0], a.C);
      if (a.mask < 0 || a.mask > 2) return bad_arg("mask must be 0 (none), 1 (recomputed) or 2 (from out / mask bits)");
      if (op != OCTSEG_SWEEP_BN_BWD_FINALIZE && a.mask == 2 && !a.out && !a.maskbits) return bad_arg("mask 2 needs out or the mask bits");
      if (op == OCTSEG_SWEEP_BN_BWD_SMALL && a.npix > (size_t)BN_SMALL_COUNT) return bad_shape("at most 1024 values per channel");
      if ((op == OCTSEG_SWEEP_BN_BWD_REDUCE || op == OCTSEG_SWEEP_BN_BWD_FINALIZE) && (a.rows < 1 || a.rows > 65535)) return bad_shape("1 <= rows <= 65535");
      if (op == OCTSEG_SWEEP_BN_BWD_SMALL) HIPCHK(launch_bn_bwd_small(dtype, a, st));
      else if (op == OCTSEG_SWEEP_BN_BWD_REDUCE) HIPCHK(launch_bn_bwd_reduce(dtype, a, st));
      else if (op == OCTSEG_SWEEP_BN_BWD_FINALIZE) HIPCHK(launch_bn_bwd_finalize(a, st));
      else HIPCHK(launch_bn_bwd_apply(dtype, a, st));
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_POOL2X2_ACCUM:
      NEED_TENSOR((long long)I(0) * I(1) * I(2), I(3));
      HIPCHK(launch_pool2x2_accum(dtype, P(0), P(1), I(0), I(1), I(2), I(3), I(4) != 0, st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_UP2_FILL:
      NEED_TENSOR((long long)I(0) * I(1) * I(2), I(3));
      HIPCHK(launch_up2_fill(dtype, P(0), P(1), I(0), I(1), I(2), I(3), st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_MASKED_ACCUM: case OCTSEG_SWEEP_RELU: case OCTSEG_SWEEP_ADD2: case OCTSEG_SWEEP_DROP_ELEM:
      if (iargs[0] < 1 || iargs[0] % vec != 0) return bad_shape("element count not a positive multiple of the 16-byte vector");
      if (op == OCTSEG_SWEEP_MASKED_ACCUM) HIPCHK(launch_masked_accum(dtype, P(0), P(1), P(2), (size_t)iargs[0], I(1) != 0, st));
      else if (op == OCTSEG_SWEEP_RELU) HIPCHK(launch_relu(dtype, P(0), P(1), P(2), (size_t)iargs[0], st));
      else if (op == OCTSEG_SWEEP_ADD2) HIPCHK(launch_add2(dtype, P(0), P(1), P(2), (size_t)iargs[0], st));
      else HIPCHK(launch_drop_elem(dtype, P(0), F(1), (float)fargs[0], P(2), (size_t)iargs[0], st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_MERGE_DROP:
      NEED_TENSOR((long long)I(0) * I(1), I(2));
      HIPCHK(launch_merge_drop(dtype, P(0), P(1), P(2), P(3), F(4), (float)fargs[0], P(5), I(0), (size_t)iargs[1], I(2), st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_DROP_BWD:
      NEED_TENSOR((long long)I(0) * I(1), I(2));
      HIPCHK(launch_drop_bwd(dtype, P(0), F(1), (float)fargs[0], P(2), I(0), (size_t)iargs[1], I(2), st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_CHANNEL_SUM:   // (any C: the scalar kernel takes what does not fill vectors)
      if (iargs[0] < 1 || I(2) < 1 || I(1) < I(2)) return bad_shape("npix >= 1 and 1 <= C <= Cstride required");
      HIPCHK(launch_channel_sum(dtype, P(0), (size_t)iargs[0], I(1), I(2), F(1), st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_TENSOR_STATS:
      NEED_TENSOR(iargs[0], I(1));
      if (I(2) < 1 || I(2) > 65535) return bad_shape("1 <= rows <= 65535");
      HIPCHK(launch_tensor_stats(dtype, P(0), (size_t)iargs[0], I(1), F(1), I(2), st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_MAXPOOL_FWD: case OCTSEG_SWEEP_MAXPOOL_BWD_IDX:
      NEED_TENSOR((long long)I(0) * I(1) * I(2), I(3));
      if ((I(1) & 1) || (I(2) & 1)) return bad_shape("the 3x3 stride-2 pool takes even H and W");
      if (op == OCTSEG_SWEEP_MAXPOOL_FWD) HIPCHK(launch_maxpool_fwd(dtype, P(0), P(1), (unsigned char*)P(2), I(0), I(1), I(2), I(3), st));
      else HIPCHK(launch_maxpool_bwd_idx(dtype, (const unsigned char*)P(0), P(1), P(2), I(0), I(1), I(2), I(3), I(4) != 0, st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_BILINEAR_RESIZE: case OCTSEG_SWEEP_BILINEAR_RESIZE_ADJOINT: {
      NEED_TENSOR((long long)I(0) * I(1) * I(2), I(5));
      if (I(3) < 1 || I(4) < 1) return bad_shape("empty output map");
      if (op == OCTSEG_SWEEP_BILINEAR_RESIZE) { HIPCHK(launch_bilinear_resize(dtype, P(0), P(1), I(0), I(1), I(2), I(3), I(4), I(5), st)); return OCTSEG_OK; }
      int gy, gz;
      if (!bilinear_adjoint_grid((long long)I(0) * I(1) * I(2), gy, gz)) return bad_shape("source pixel count does not factor into a launch grid");
      HIPCHK(launch_bilinear_resize_adjoint(dtype, P(0), P(1), I(0), I(1), I(2), I(3), I(4), I(5), st));
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_BILINEAR_ADJOINT:
      NEED_TENSOR((long long)I(0) * I(1) * I(2), I(3));
      if (I(4) < 2) return bad_shape("up >= 2");
      HIPCHK(launch_bilinear_adjoint(dtype, P(0), P(1), I(0), I(1), I(2), I(3), I(4), st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_BIN_MEAN: case OCTSEG_SWEEP_BIN_MEAN_BWD:
      NEED_TENSOR((long long)I(0) * I(1) * I(2), I(3));
      if (I(4) < 1 || (long long)I(0) * I(4) * I(4) > 65535) return bad_shape("k >= 1 and N k^2 <= 65535");
      if (op == OCTSEG_SWEEP_BIN_MEAN) HIPCHK(launch_bin_mean(dtype, P(0), P(1), I(0), I(1), I(2), I(3), I(4), st));
      else HIPCHK(launch_bin_mean_bwd(dtype, P(0), P(1), I(0), I(1), I(2), I(3), I(4), I(5) != 0, st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_IMAGE_SUM:
      NEED_TENSOR((long long)I(0) * I(1), I(2));
      if (I(0) > 65535) return bad_shape("N <= 65535");
      HIPCHK(launch_image_sum(dtype, P(0), P(1), I(0), I(1), I(2), (float)fargs[0], st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_IMAGE_BCAST:
      NEED_TENSOR((long long)I(0) * I(1), I(2));
      HIPCHK(launch_image_bcast(dtype, P(0), P(1), I(0), I(1), I(2), (float)fargs[0], I(3) != 0, st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_SE_GATE:
      NEED_TENSOR((long long)I(0) * I(1), I(2));
      HIPCHK(launch_se_gate(dtype, P(0), P(1), P(2), I(0), I(1), I(2), I(3) != 0, st, P(3)));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_SE_DGATE:
      NEED_TENSOR((long long)I(0) * I(1), I(2));
      if (I(0) > 65535) return bad_shape("N <= 65535");
      if ((P(5) == nullptr) != (P(6) == nullptr)) return bad_arg("s2 and ds2 come together");
      HIPCHK(launch_se_dgate(dtype, P(0), P(1), P(2), P(3), F(4), I(0), I(1), I(2), st, P(5), P(6)));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_PARITY_PERMUTE:
      NEED_TENSOR((long long)I(0) * I(1) * I(2), I(3));
      if ((I(1) & 1) || (I(2) & 1)) return bad_shape("even H and W required");
      HIPCHK(launch_parity_permute(dtype, P(0), P(1), I(0), I(1), I(2), I(3), I(4) != 0, I(5) != 0, st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_MOSAIC:
      NEED_TENSOR((long long)I(0) * I(1) * I(2), I(3));
      if (I(4) < 1) return bad_shape("r >= 1");
      HIPCHK(launch_mosaic(dtype, P(0), P(1), I(0), I(1), I(2), I(3), I(4), I(5) != 0, I(6) != 0, st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_DW_CONV: case OCTSEG_SWEEP_DW_WGRAD: {   // iargs: inC, ic0, outC, oc0, wC, wc0, N, H, W, C, dil (, flip, accum)
      const int inC = I(0), ic0 = I(1), outC = I(2), oc0 = I(3), wC = I(4), wc0 = I(5), C = I(9), dil = I(10);
      NEED_TENSOR((long long)I(6) * I(7) * I(8), C);
      if (inC % vec || outC % vec || ic0 % vec || oc0 % vec || wC % 4 || wc0 % 4 || ic0 + C > inC || oc0 + C > outC || wc0 + C > wC)
        return bad_shape("channel slices must lie inside their tensors, on 16-byte vector boundaries");
      if (dil < 1) return bad_shape("dilation >= 1");
      if (op == OCTSEG_SWEEP_DW_CONV) HIPCHK(launch_dw_conv(dtype, P(0), inC, ic0, P(1), outC, oc0, F(2), wC, wc0, I(6), I(7), I(8), C, dil, I(11) != 0, I(12) != 0, st));
      else HIPCHK(launch_dw_wgrad(dtype, P(0), inC, ic0, P(1), outC, oc0, F(2), wC, wc0, I(6), I(7), I(8), C, dil, st));
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_CAM_SEED:   // iargs: B, C, HW, CP
      if (I(0) < 1 || I(1) < 1 || I(2) < 1) return bad_shape("empty batch, class list or map");
      if (I(1) > I(3) || (I(3) != 8 && I(3) != 16)) return bad_shape("C <= CP and CP = 8 or 16 required");
      HIPCHK(launch_cam_seed(dtype, F(0), P(1), I(0), I(1), (size_t)iargs[2], I(3), st));
      return OCTSEG_OK;
    case OCTSEG_SWEEP_DWG_FWD: case OCTSEG_SWEEP_DWG_BWD_DATA: case OCTSEG_SWEEP_DWG_BWD_W: {   // iargs: N, H, W, C, OH, OW, K, stride, pad (, accum)
      DwgArgs a;
      memset(&a, 0, sizeof(a));
      a.N = I(0); a.H = I(1); a.W = I(2); a.C = I(3); a.OH = I(4); a.OW = I(5); a.K = I(6); a.stride = I(7); a.pad = I(8);
      NEED_TENSOR((long long)a.N * a.H * a.W, a.C);
      if ((a.K != 3 && a.K != 5) || (a.stride != 1 && a.stride != 2) || a.pad >= a.K) return bad_shape("K = 3 | 5, stride = 1 | 2, 0 <= pad < K");
      if (a.OH < 1 || a.OW < 1 || (long long)(a.OH - 1) * a.stride - a.pad >= a.H || (long long)(a.OW - 1) * a.stride - a.pad >= a.W)
        return bad_shape("the output map does not fit the input map");
      if (op == OCTSEG_SWEEP_DWG_FWD) { a.in = P(0); a.out = P(1); a.w = F(2); HIPCHK(launch_dwg_fwd(dtype, a, st)); }
      else if (op == OCTSEG_SWEEP_DWG_BWD_DATA) { a.out = P(0); a.gin = P(1); a.w = F(2); a.accum = I(9) != 0; HIPCHK(launch_dwg_bwd_data(dtype, a, st)); }
      else { a.in = P(0); a.out = P(1); a.dw = F(2); HIPCHK(launch_dwg_bwd_w(dtype, a, st)); }
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_BNX_FWD: case OCTSEG_SWEEP_BNX_BWD: {   // ptrs y, scale, shift, dscale, post | g, out; iargs npix, hw, C, act
      BnxArgs a;
      a.y = P(0); a.scale = F(1); a.shift = F(2); a.dscale = F(3); a.post = P(4); a.out = P(5);
      a.npix = (size_t)iargs[0]; a.hw = I(1); a.C = I(2); a.act = I(3);
      NEED_TENSOR(iargs[0], a.C);
      if (a.hw < 1 || iargs[0] % a.hw != 0) return bad_shape("npix must be a multiple of the pixels per image");
      if (a.act != 0 && a.act != 1) return bad_arg("act must be 0 (identity) or 1 (swish)");
      if ((a.scale == nullptr) != (a.shift == nullptr)) return bad_arg("scale and shift come together");
      if (op == OCTSEG_SWEEP_BNX_BWD && a.act == 1 && (!a.y || !a.scale)) return bad_arg("the swish gradient needs y, scale and shift");
      if (op == OCTSEG_SWEEP_BNX_FWD) HIPCHK(launch_bnx_fwd(dtype, a, st));
      else HIPCHK(launch_bnx_bwd(dtype, a, st));
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_DICE_BWD: {   // ptrs logits, target (f32 NCHW), sums (double [1 + B][C][4]), dlogits; iargs B, C, HW, CP, loss kind; fargs grad_scale
      DiceArgs a;
      memset(&a, 0, sizeof(a));
      a.logits = F(0); a.target = F(1); a.sums = (double*)P(2); a.B = I(0); a.C = I(1); a.HW = (size_t)iargs[2]; a.loss_kind = I(4);
      if (a.B < 1 || a.C < 1 || iargs[2] < 1) return bad_shape("empty batch, class list or map");
      if (a.C > I(3) || (I(3) != 8 && I(3) != 16)) return bad_shape("C <= CP and CP = 8 or 16 required");
      if (a.loss_kind < LOSS_DICE || a.loss_kind > LOSS_DICE_BCE) return bad_arg("loss kind must be 0 (dice), 1 (bce) or 2 (dice + bce)");
      HIPCHK(launch_dice_bwd(dtype, a, (float)fargs[0], P(3), I(3), st));
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_GN_FORWARD: case OCTSEG_SWEEP_GN_BACKWARD: {
      GnArgs a;
      memset(&a, 0, sizeof(a));
      const bool fwd = op == OCTSEG_SWEEP_GN_FORWARD;
      const int N = I(0);
      int H = 0, W = 0, up = 1;
      if (fwd) {   // ptrs y, gamma, beta, out, part, ss, stat; iargs N, H, W, C, G, up; fargs eps
        H = I(1); W = I(2); a.C = I(3); a.G = I(4); up = I(5); a.HW = (size_t)H * W; a.eps = (float)fargs[0];
        a.y = P(0); a.gamma = F(1); a.beta = F(2); a.out = P(3); a.part = F(4); a.ss = F(5); a.stat = F(6);
      } else {     // ptrs y, g, dy, gamma, dgamma, dbeta, part, ss, stat, coef; iargs N, HW, C, G
        a.HW = (size_t)iargs[1]; a.C = I(2); a.G = I(3);
        a.y = P(0); a.g = P(1); a.dy = P(2); a.gamma = F(3); a.dgamma = F(4); a.dbeta = F(5); a.part = F(6); a.ss = F(7); a.stat = F(8); a.coef = F(9);
      }
      NEED_TENSOR((long long)N * (long long)a.HW, a.C);
      if (N > 65535) return bad_shape("N <= 65535");
      const int vpc = a.C / vec;
      if (a.C > 1024 || vpc > 256 || 256 % vpc != 0) return bad_shape("GroupNorm width: C <= 1024 and a vector count that divides 256");
      if (a.G < 1 || a.C % a.G != 0) return bad_shape("C must be a multiple of the group count");
      a.cpg = a.C / a.G;
      if (fwd && up != 1 && up != 2) return bad_shape("up must be 1 or 2");
      if (fwd) HIPCHK(launch_gn_forward(dtype, a, N, H, W, up, st));
      else HIPCHK(launch_gn_backward(dtype, a, N, st));
      return OCTSEG_OK;
    }
    case OCTSEG_SWEEP_SEFC_FWD: case OCTSEG_SWEEP_SEFC_BWD: {   // iargs N, C, R, act
      SefcArgs a;
      memset(&a, 0, sizeof(a));
      a.N = I(0); a.C = I(1); a.R = I(2); a.act = I(3);
      if (a.N < 1 || a.N > 65535 || a.C < 1 || a.R < 1 || (size_t)(a.C + a.R) * sizeof(float) > 60 * 1024) return bad_shape("1 <= N <= 65535, C, R >= 1, (C + R) floats within 60 KiB");
      if (a.act != 0 && a.act != 1) return bad_arg("act must be 0 (ReLU) or 1 (swish)");
      if (op == OCTSEG_SWEEP_SEFC_FWD) {   // ptrs m, s, w1, b1, w2, b2, h
        a.m = P(0); a.s = P(1); a.w1 = F(2); a.b1 = F(3); a.w2 = F(4); a.b2 = F(5); a.h = F(6);
        HIPCHK(launch_sefc_fwd(dtype, a, st));
      } else {                             // ptrs m, ds, dm, w1, w2, h, dh, dw1?, db1?, dw2?, db2? (the four together or none)
        a.m = P(0); a.ds = P(1); a.dm = P(2); a.w1 = F(3); a.w2 = F(4); a.h = F(5); a.dh = F(6); a.dw1 = F(7); a.db1 = F(8); a.dw2 = F(9); a.db2 = F(10);
        const int ng = (a.dw1 != nullptr) + (a.db1 != nullptr) + (a.dw2 != nullptr) + (a.db2 != nullptr);
        if (ng != 0 && ng != 4) return bad_arg("the four parameter gradients come together or not at all");
        HIPCHK(launch_sefc_bwd(dtype, a, st));
      }
      return OCTSEG_OK;
    }
  }
#undef NEED_TENSOR
  return fail(OCTSEG_BAD_ARG, "sweep_op: unknown op");
}
