// stem_api.cpp -- octseg_stem_op: one C-ABI door to the stem kernels, so that each can be pinned against a float64 reference one launch at a
// time (tests/test_gpu_stemops.py) instead of only through a whole resnet-encoder network: the im2col rows of the f32 / deterministic path
// (elementwise.hip launch_stem_im2col: 7x7 pad 3, RegNet's 3x3 pad 1, EfficientNet's 3x3 pad 0) and thin.hip's KSTEM forward and weight
// gradient, which read the NCHW f32 frame directly.  The entry fills the StemArgs the plan fills (plan_forward.cpp OP_CONV of a stem layer,
// plan_backward.cpp conv_backward) from a plain C descriptor; the kernels stay what they are.  It refuses, before any launch, what the
// launchers cannot take.  Buffer sizes are the caller's contract (oct_segmentation_amd/convops.py checks them): see include/octseg.h.
#include "plan_internal.h"

#include <cmath>

using namespace octseg;
using namespace octseg::detail;

namespace {

bool aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

int check(int stage, int dtype, const octseg_stem_desc* d) {
  const std::string who = "stem_op: ";
  auto bad_arg = [&](const char* m) { return fail(OCTSEG_BAD_ARG, who + m); };
  auto bad_shape = [&](const char* m) { return fail(OCTSEG_BAD_SHAPE, who + m); };
  if (stage != OCTSEG_STEM_IM2COL && stage != OCTSEG_STEM_FORWARD && stage != OCTSEG_STEM_WGRAD) return bad_arg("unknown stage");
  if (dtype != OCTSEG_F32 && dtype != OCTSEG_BF16 && dtype != OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, who + "dtype must be f32, bf16 or f16");
  if (stage != OCTSEG_STEM_IM2COL && !thin_stem_eligible(dtype))
    return fail(OCTSEG_BAD_DTYPE, who + "thin.hip's stem kernels take bf16 and f16 (f32: IM2COL + the 1x1 conv over its rows)");
  if (stage == OCTSEG_STEM_WGRAD && dtype != OCTSEG_BF16) return fail(OCTSEG_BAD_DTYPE, who + "the stem weight gradient is a bf16 kernel");
  if (d == nullptr) return bad_arg("null descriptor");
  if (d->N < 1 || d->H < 2 || d->W < 2) return bad_shape("empty frame");
  // the kernels compute H / 2 x W / 2 outputs: torch's (H + 2 pad - k) / 2 + 1 only for even extents
  if ((d->H & 1) || (d->W & 1)) return bad_shape("odd H or W");
  if ((long long)d->N * d->H * d->W * 3 >= (1ll << 31) || (long long)d->N * (d->H / 2) * (d->W / 2) * 160 >= (1ll << 31))
    return bad_shape("tensor of 2^31 elements or more");
  if (d->img == nullptr || !aligned(d->img)) return bad_arg("null or misaligned frame");
  if (d->normalize != 0 && d->normalize != 1) return bad_arg("normalize is 0 or 1");
  if (d->normalize)
    for (int i = 0; i < 3; ++i)
      if (!(d->stdv[i] > 0.f) || !std::isfinite(d->stdv[i]) || !std::isfinite(d->mean[i])) return bad_arg("normalize needs finite means and positive finite stds");
  if (!aligned(d->col) || !aligned(d->w) || !aligned(d->wscale) || !aligned(d->bias) || !aligned(d->y) || !aligned(d->stat_slab) || !aligned(d->dy) ||
      !aligned(d->dW))
    return bad_arg("misaligned pointer");
  if (stage == OCTSEG_STEM_IM2COL) {
    const bool k7 = d->ksize == 7 && d->pad == 3 && d->KP == 160;
    const bool k3 = d->ksize == 3 && (d->pad == 1 || d->pad == 0) && d->KP == 32;
    if (!k7 && !k3) return bad_shape("(ksize, pad, KP) is (7, 3, 160), (3, 1, 32) or (3, 0, 32)");
    if (d->col == nullptr) return bad_arg("null col");
    return OCTSEG_OK;
  }
  if (stage == OCTSEG_STEM_FORWARD) {
    if (d->w == nullptr || d->y == nullptr) return bad_arg("null weight or destination");
    if (d->relu_out && d->bias == nullptr) return bad_arg("relu_out comes with the folded bias");
    if (d->relu_out && d->stat_slab != nullptr) return bad_arg("relu_out together with stat_slab (eval against training)");
    if (d->slab_row0 < 0) return bad_arg("negative slab_row0");
    if (d->dy != nullptr || d->dW != nullptr) return bad_arg("dy and dW belong to the weight gradient");
    return OCTSEG_OK;
  }
  if (d->dy == nullptr || d->dW == nullptr) return bad_arg("null dy or dW");
  if (d->w || d->wscale || d->bias || d->relu_out || d->y || d->stat_slab || d->slab_row0) return bad_arg("w, wscale, bias, relu_out, y and the slab belong to the forward");
  // (plan_backward.cpp: the deterministic-reduction mode rebuilds the im2col rows and runs the atomics-free kernel instead)
  if (deterministic_mode()) return bad_arg("deterministic mode: the plan runs IM2COL + the 1x1 weight gradient, not this kernel");
  return OCTSEG_OK;
}

}  // namespace

extern "C" {

int octseg_stem_op(int stage, int dtype, const octseg_stem_desc* d, void* stream) {
  const int rc = check(stage, dtype, d);
  if (rc != OCTSEG_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (stage == OCTSEG_STEM_IM2COL) {
    HIPCHK(launch_stem_im2col(dtype, d->img, d->col, d->N, d->H, d->W, d->KP, d->mean, d->stdv, d->normalize, st, d->ksize, d->pad));
    return OCTSEG_OK;
  }
  StemArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.img = d->img; sa.N = d->N; sa.H = d->H; sa.W = d->W; sa.normalize = d->normalize;
  for (int i = 0; i < 3; ++i) { sa.mean[i] = d->normalize ? d->mean[i] : 0.f; sa.stdv[i] = d->normalize ? d->stdv[i] : 1.f; }   // (as plan_forward.cpp)
  if (stage == OCTSEG_STEM_FORWARD) {
    sa.w = d->w; sa.wscale = d->wscale; sa.bias = d->bias; sa.relu_out = d->relu_out ? 1 : 0;
    sa.y = d->y; sa.slab = d->stat_slab; sa.slab_row0 = d->slab_row0;
    HIPCHK(launch_thin_stem_forward(dtype, sa, st));
  } else {
    sa.dy = d->dy; sa.dW = d->dW;
    HIPCHK(launch_thin_stem_wgrad(dtype, sa, st));
  }
  return OCTSEG_OK;
}

int octseg_stem_slab_rows(int N, int H, int W) {
  if (N < 1 || H < 2 || W < 2) return 0;
  return thin_stem_rows(N, H, W);
}

}  // extern "C"
