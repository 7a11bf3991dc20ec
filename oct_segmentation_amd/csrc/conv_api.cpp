// conv_api.cpp -- octseg_conv_layer_op: one C-ABI door to the conv kernels' fused operand and epilogue paths (conv_mfma.hip, gemm1x1.hip,
// conv3x3p.hip, thin.hip, wgrad_mfma.hip, wgrad1x1.hip, wgrad_convt.hip), so that every route can be pinned against a float64 reference one
// launch at a time (tests/test_gpu_convops.py) instead of only through a whole network.  The entry builds the ConvArgs / WgradArgs the plan
// builds for one layer pass (plan_forward.cpp OP_CONV, plan_backward.cpp conv_backward) from a plain C descriptor and hands them to
// launch_conv / launch_wgrad: the kernels and their routing stay what they are.  It refuses, before any launch, what the launchers cannot
// take.  Buffer sizes are the caller's contract (oct_segmentation_amd/convops.py checks them): see include/octseg.h.
// octseg_tied_layer_op (second half of this file) is the same door for the tied decomposition of a decoder layer.
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

namespace {

struct Built {
  std::vector<ConvArgs> conv;     // forward / data-gradient launches
  std::vector<WgradArgs> wg;      // weight-gradient launches
  bool convt16 = false;           // weight gradient of a ConvTranspose2d: the four parities in ONE launch (wgrad_convt.hip)
  ConvPackInfo pk{};              // packed weight image of the forward / data-gradient launches
  int rows = 0;                   // forward: BatchNorm-statistics slab rows of all launches
};

bool aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Validates the descriptor and builds the launches exactly as the plan does.  Returns OCTSEG_OK or the refusal.
int build(int mode, int dtype, const octseg_conv_layer_desc* d, Built& B) {
  const std::string who = "conv_layer_op: ";
  auto bad_arg = [&](const char* m) { return fail(OCTSEG_BAD_ARG, who + m); };
  auto bad_shape = [&](const char* m) { return fail(OCTSEG_BAD_SHAPE, who + m); };
  if (mode != OCTSEG_CONV_FORWARD && mode != OCTSEG_CONV_BACKWARD_DATA && mode != OCTSEG_CONV_BACKWARD_WEIGHT) return bad_arg("unknown mode");
  if (dtype != OCTSEG_F32 && dtype != OCTSEG_BF16 && dtype != OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, who + "dtype must be f32, bf16 or f16");
  if (dtype == OCTSEG_F16 && mode != OCTSEG_CONV_FORWARD) return fail(OCTSEG_BAD_DTYPE, who + "f16 is the serving dtype: no gradient kernels");
  if (d == nullptr) return bad_arg("null descriptor");
  const bool fwd = mode == OCTSEG_CONV_FORWARD, dgrad = mode == OCTSEG_CONV_BACKWARD_DATA, wgrad = mode == OCTSEG_CONV_BACKWARD_WEIGHT;
  const int vec = ev_vec(dtype);

  // ---- geometry
  if (d->N < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->Cout < 1) return bad_shape("empty tensor");
  if (d->transposed ? !(d->R == 4 && d->stride == 2 && d->pad == 1) : !((d->R == 1 || d->R == 3) && (d->stride == 1 || d->stride == 2)))
    return bad_shape("R must be 1 or 3 at stride 1 or 2, or 4 / stride 2 / pad 1 when transposed");
  if (d->pad < 0 || d->pad > d->R / 2) return bad_shape("pad must lie in [0, R / 2]");
  if (!geom_ok(dtype, d->Cin, d->Cout, d->R, d->R, d->stride, d->transposed)) return bad_shape("geometry refused by geom_ok (Cin in whole 16-byte vectors, square kernel, stride 1 | 2)");
  const Geom g = op_geom(d->N, d->H, d->W, d->Cin, d->Cout, d->R, d->R, d->stride, d->pad, d->transposed);
  if (g.OH < 1 || g.OW < 1) return bad_shape("the map is smaller than the kernel");
  if ((long long)g.N * std::max(g.IH, g.OH) * std::max(g.IW, g.OW) * std::max(g.Cin, g.Cout) >= (1ll << 31)) return bad_shape("tensor of 2^31 elements or more");
  const bool head = d->head != 0;
  if (head && !fwd) return bad_arg("head mode is a forward store");
  if (!head && d->Cout % vec != 0) return bad_shape("Cout is not a whole number of 16-byte vectors");

  // ---- sources
  if (d->nsrc < 1 || d->nsrc > MAX_SRC) return bad_shape("1 .. 5 sources");
  SrcDesc src[MAX_SRC];
  int c0 = 0;
  const bool use_src = !dgrad;   // the data gradient reads dy; the sources only say where the gradient goes
  for (int i = 0; i < d->nsrc; ++i) {
    const octseg_conv_src& s = d->src[i];
    if (s.C < 1 || s.C % vec != 0) return bad_shape("a source's C is not a whole number of 16-byte vectors");
    if (s.up != 0 && s.up != 1) return bad_arg("up is 0 or 1");
    if ((s.H << s.up) != d->H || (s.W << s.up) != d->W) return bad_shape("a source's stored extent is not H >> up x W >> up");
    if ((s.scale != nullptr) != (s.shift != nullptr)) return bad_arg("scale and shift come together");
    if (s.relu && s.scale == nullptr) return bad_arg("relu without the affine (the plan never builds it)");
    if (use_src && (s.ptr == nullptr || !aligned(s.ptr) || !aligned(s.scale) || !aligned(s.shift))) return bad_arg("null or misaligned source pointer");
    SrcDesc o;
    o.ptr = s.ptr; o.scale = use_src ? s.scale : nullptr; o.shift = use_src ? s.shift : nullptr; o.C = s.C; o.c0 = c0; o.H = s.H; o.W = s.W; o.up = s.up;
    o.relu = s.relu ? 1 : 0;
    src[i] = o;
    c0 += s.C;
  }
  if (c0 != d->Cin) return bad_shape("the sources' channels do not add up to Cin");
  if (d->w == nullptr && !wgrad) return bad_arg("null weight");
  if (!aligned(d->w) || !aligned(d->wscale) || !aligned(d->bias) || !aligned(d->stat_slab) || !aligned(d->dy) || !aligned(d->dW) || !aligned(d->scratch))
    return bad_arg("misaligned pointer");
  if (!fwd && (d->wscale || d->bias || d->relu_out || d->stat_slab || d->slab_row0)) return bad_arg("wscale, bias, relu_out and the slab belong to the forward");
  if (d->slab_row0 < 0) return bad_arg("negative slab_row0");

  if (wgrad) {
    if (d->dy == nullptr || d->dW == nullptr) return bad_arg("null dy or dW");
    wgrad_launches(g, B.wg);
    for (auto& a : B.wg) {
      a.nsrc = d->nsrc;
      for (int i = 0; i < d->nsrc; ++i) a.src[i] = src[i];
      a.dy = d->dy; a.dyC = d->Cout; a.dW = d->dW; a.stamp = nullptr; a.wg_target = 0;
    }
    B.convt16 = d->transposed && B.wg.size() == 4 && wgrad_convt16_eligible(B.wg[0], dtype);   // the plan's route for a ConvTranspose2d
    return OCTSEG_OK;
  }

  if (d->scratch == nullptr) return bad_arg("null scratch");
  const int wtaps = d->R * d->R;
  if (fwd) {
    if (d->relu_out && d->bias == nullptr) return bad_arg("relu_out comes with the folded bias");
    if (d->relu_out && d->stat_slab != nullptr) return bad_arg("relu_out together with stat_slab (eval against training)");
    if (head && (d->stat_slab != nullptr || d->dst[0].accum || d->transposed)) return bad_arg("head mode: no slab, no accum, no transposed layer");
    if (d->dst[0].ptr == nullptr || !aligned(d->dst[0].ptr)) return bad_arg("null or misaligned destination");
    if (d->dst[0].pool) return bad_arg("pool is a data-gradient store");
    fwd_launches(g, B.conv);
    B.pk = conv_pack_info(B.conv[0], dtype);          // (as plan_build.cpp: from the bare launch)
    int row0 = d->slab_row0;
    for (auto& a : B.conv) {
      a.nsrc = d->nsrc;
      for (int i = 0; i < d->nsrc; ++i) a.src[i] = src[i];
      a.W = d->scratch; a.bias = d->bias; a.relu_out = d->relu_out ? 1 : 0; a.wscale = d->wscale;
      a.Wmaster = d->w; a.wO = d->Cout; a.wI = d->Cin; a.wtrans = 0;   // (ConvT: [4][4][O][I], same indexing -- as plan_forward.cpp)
      DstDesc o;
      o.ptr = d->dst[0].ptr; o.C = d->Cout; o.c0 = 0; o.cn = d->Cout; o.H = g.OH; o.W = g.OW; o.accum = d->dst[0].accum ? 1 : 0; o.pool = 0;
      a.dst[0] = o; a.ndst = 1; a.out_mode = head ? OUT_HEAD_NCHW : OUT_STORE;
      a.stat_slab = d->stat_slab; a.slab_row0 = row0; a.stamp = nullptr;
      if (a.bias != nullptr && a.stat_slab != nullptr) {
        ConvArgs nb = a;
        nb.bias = nullptr;
        if (conv_route(nb, dtype) == ROUTE_GEMM1X1) return bad_arg("bias together with the slab on a gemm1x1 launch (the plan never builds it)");
      }
      const int r = conv_num_mtiles_flat(a, dtype);
      row0 += r; B.rows += r;
    }
  } else {
    if (d->dy == nullptr) return bad_arg("null dy");
    dgrad_launches(g, B.conv);
    bool full_cover = true;
    for (auto& a : B.conv) if (a.ntaps == 0) full_cover = false;
    ConvArgs d0 = B.conv[0];
    for (auto& a : B.conv) if (a.ntaps > 0) { d0 = a; break; }
    d0.Cin = d->Cout;
    B.pk = conv_pack_info(d0, dtype);                 // (as plan_build.cpp: from the first launch with taps, bare)
    DstDesc dst[MAX_SRC];
    for (int i = 0; i < d->nsrc; ++i) {
      const octseg_conv_dst& t = d->dst[i];
      if (t.ptr == nullptr || !aligned(t.ptr)) return bad_arg("null or misaligned destination");
      DstDesc o;
      o.ptr = t.ptr; o.C = src[i].C; o.c0 = src[i].c0; o.cn = src[i].C; o.H = g.IH; o.W = g.IW; o.accum = t.accum ? 1 : 0; o.pool = 0;
      if (t.pool) {   // where plan_backward.cpp sets it: an `up` source whose data gradient is ONE stride-1 launch over an even map
        if (!src[i].up || B.conv.size() != 1 || B.conv[0].ostride != 1 || d->stride != 1 || d->transposed) return bad_arg("pool needs an `up` source and stride 1");
        o.H = src[i].H; o.W = src[i].W; o.pool = 1;
      }
      if (!o.accum && !full_cover) return bad_arg("this data gradient covers one pixel parity only: accum = 1 over a zeroed destination");
      dst[i] = o;
    }
    for (auto& a : B.conv) {
      SrcDesc s;
      s.ptr = d->dy; s.scale = nullptr; s.shift = nullptr; s.C = d->Cout; s.c0 = 0; s.H = g.OH; s.W = g.OW; s.up = 0; s.relu = 0;
      a.src[0] = s; a.nsrc = 1; a.Cin = d->Cout; a.W = d->scratch;
      if (!d->transposed) { a.Wmaster = d->w; a.wO = d->Cout; a.wI = d->Cin; a.wtrans = 1; }
      for (int i = 0; i < d->nsrc; ++i) a.dst[i] = dst[i];
      a.ndst = d->nsrc; a.out_mode = OUT_STORE;   // per-destination accumulate flags decide
      a.bias = nullptr; a.stat_slab = nullptr; a.stamp = nullptr;
    }
  }
  if (conv_image_bytes(B.pk, wtaps) > d->scratch_bytes) return bad_arg("scratch smaller than the packed weight image");
  // one image serves every launch of the layer: a launch whose own tiling wants another image layout cannot run on it
  for (auto& a : B.conv) {
    if (a.ntaps == 0 || conv_route(a, dtype) == ROUTE_THIN) continue;   // (thin.hip reads the master weights)
    const ConvPackInfo p = conv_pack_info(a, dtype);
    if (p.BN != B.pk.BN || p.RB != B.pk.RB || p.nchunks != B.pk.nchunks || p.ntiles != B.pk.ntiles)
      return bad_shape("a launch's tiling does not match the layer's packed weight image");
  }
  return OCTSEG_OK;
}

int public_route(const ConvArgs& a, int dtype) {
  if (a.ntaps <= 0) return -1;
  switch (conv_route(a, dtype)) {
    case ROUTE_THIN: return OCTSEG_ROUTE_THIN;
    case ROUTE_GEMM1X1: return OCTSEG_ROUTE_GEMM1X1;
    case ROUTE_CONV3X3P: return OCTSEG_ROUTE_CONV3X3P;
    case ROUTE_MFMA: break;
  }
  const int t = conv_mfma_tile(a, dtype);
  return t == TILE_11 ? OCTSEG_ROUTE_MFMA11 : t == TILE_WIDE_N ? OCTSEG_ROUTE_MFMA_WIDEN : OCTSEG_ROUTE_MFMA16;
}

}  // namespace

extern "C" {

int octseg_conv_layer_op(int mode, int dtype, const octseg_conv_layer_desc* d, void* stream) {
  Built B;
  const int rc = build(mode, dtype, d, B);
  if (rc != OCTSEG_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (mode == OCTSEG_CONV_BACKWARD_WEIGHT) {
    if (B.convt16) { HIPCHK(launch_wgrad_convt16(dtype, B.wg[0], st)); return OCTSEG_OK; }
    for (auto& a : B.wg) HIPCHK(launch_wgrad(dtype, a, st));
    return OCTSEG_OK;
  }
  const bool fwd = mode == OCTSEG_CONV_FORWARD;
  HIPCHK(launch_pack_weight_image(dtype, d->w, d->scratch, d->R * d->R, d->Cout, d->Cin, fwd ? 0 : 1, B.pk, st, fwd ? d->wscale : nullptr));
  for (auto& a : B.conv) HIPCHK(launch_conv(dtype, a, st));
  return OCTSEG_OK;
}

int octseg_conv_layer_route(int mode, int dtype, const octseg_conv_layer_desc* d, int* route_per_launch, int* nlaunch) {
  if (route_per_launch == nullptr || nlaunch == nullptr) return fail(OCTSEG_BAD_ARG, "conv_layer_route: null output");
  Built B;
  const int rc = build(mode, dtype, d, B);
  if (rc != OCTSEG_OK) return rc;
  int n = 0;
  if (mode == OCTSEG_CONV_BACKWARD_WEIGHT) {
    if (B.convt16) route_per_launch[n++] = OCTSEG_WROUTE_CONVT16;
    else
      for (auto& a : B.wg) {
        const WgradRoute r = wgrad_route(a, dtype);
        route_per_launch[n++] = a.ntaps <= 0 ? -1 : r == WROUTE_THIN ? OCTSEG_WROUTE_THIN : r == WROUTE_1X1 ? OCTSEG_WROUTE_WGRAD1X1 : OCTSEG_WROUTE_MFMA;
      }
  } else {
    for (auto& a : B.conv) route_per_launch[n++] = public_route(a, dtype);
  }
  *nlaunch = n;
  return OCTSEG_OK;
}

int octseg_conv_layer_slab_rows(int dtype, const octseg_conv_layer_desc* d, int* rows) {
  if (rows == nullptr) return fail(OCTSEG_BAD_ARG, "conv_layer_slab_rows: null output");
  Built B;
  const int rc = build(OCTSEG_CONV_FORWARD, dtype, d, B);
  if (rc != OCTSEG_OK) return rc;
  *rows = B.rows;
  return OCTSEG_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------- the tied decoder layer
// octseg_tied_layer_op: one pass of a (nearest x2, concat, 3x3) decoder layer through the tied decomposition (ConvLayer::tie), built from the
// same descriptor as above exactly as tied_forward (plan_forward.cpp) and the `L.tie & 2` / `L.tie & 4` branches of conv_backward
// (plan_backward.cpp) build it: eligibility, image geometry and pack jobs come from the helpers the plan builder calls (plan_geom.cpp).
namespace {

constexpr size_t TIE_TAB_BYTES = 512, TIE_PREFIX_BYTES = 512;   // job table (4 PackJobs) and prefix sums at the head of the caller's scratch
static_assert(4 * sizeof(PackJob) <= TIE_TAB_BYTES, "the job table fits its slot");

struct Tied {
  int Ca = 0, Cs = 0, ns = 0;
  Geom gu{}, gs{};
  TieImages im{};
  TieOffsets at{};
  size_t dk4_off = 0, bytes = 0;          // the weight gradient's f32 scratch ([16][O][Ca] + [9][O][Cs]) and the whole scratch
  std::vector<PackJob> jobs; std::vector<unsigned long long> prefix; unsigned long long total = 0;
  std::vector<ConvArgs> conv;             // forward: (skip,) four parities; data gradient: the up slice's launch(es) (, skip)
  std::vector<WgradArgs> wg;              // weight gradient: the four parity launches (, skip)
  bool convt16 = false, masked = false;
};

// layer geometry only (what octseg_tied_layer_scratch_bytes needs); pointers are looked at by tied_build
int tied_shape(int dtype, const octseg_conv_layer_desc* d, Tied& B) {
  const std::string who = "tied_layer_op: ";
  auto bad_shape = [&](const char* m) { return fail(OCTSEG_BAD_SHAPE, who + m); };
  if (dtype != OCTSEG_F32 && dtype != OCTSEG_BF16 && dtype != OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, who + "dtype must be f32, bf16 or f16");
  if (dtype != OCTSEG_BF16) return fail(OCTSEG_BAD_DTYPE, who + "the tied decomposition is a bf16 training path");
  if (d == nullptr) return fail(OCTSEG_BAD_ARG, who + "null descriptor");
  if (d->N < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->Cout < 1) return bad_shape("empty tensor");
  if (d->nsrc < 1 || d->nsrc > MAX_SRC) return bad_shape("1 .. 5 sources");
  if ((long long)d->N * d->H * d->W * std::max(d->Cin, d->Cout) >= (1ll << 31)) return bad_shape("tensor of 2^31 elements or more");
  int c = 0;
  TieQuery q{};
  q.esz = (int)dtype_size(dtype); q.transposed = d->transposed != 0; q.head = d->head != 0; q.has_bn = true; q.has_bias = d->bias != nullptr;
  q.R = q.S = d->R; q.stride = d->stride; q.pad = d->pad; q.nsrc = d->nsrc;
  q.up0_whole_grad = d->src[0].up == 1; q.skips_plain_grad = true;
  for (int i = 0; i < d->nsrc; ++i) {
    const octseg_conv_src& s = d->src[i];
    if (s.C < 1 || s.C % 8 != 0) return bad_shape("a source's C is not a whole number of 16-byte vectors");
    if (s.up != 0 && s.up != 1) return fail(OCTSEG_BAD_ARG, who + "up is 0 or 1");
    if ((s.H << s.up) != d->H || (s.W << s.up) != d->W) return bad_shape("a source's stored extent is not H >> up x W >> up");
    if (i > 0 && s.up) q.skips_plain_grad = false;
    c += s.C;
  }
  if (c != d->Cin) return bad_shape("the sources' channels do not add up to Cin");
  q.Ca = d->src[0].C; q.Cs = d->Cin - q.Ca; q.Cout = d->Cout;
  if (d->Cout % 8 != 0) return bad_shape("Cout is not a whole number of 16-byte vectors");
  if (!tie_eligible(q)) return bad_shape("the plan would not tie this layer (tie_eligible: src[0] nearest x2 with >= 64 channels, plain skips of 0 or >= 32, 3x3 stride 1 pad 1, Cout >= 32)");
  B.Ca = q.Ca; B.Cs = q.Cs; B.ns = d->nsrc;
  B.gu = Geom{4, 4, 2, 1, true, d->N, d->H / 2, d->W / 2, B.Ca, d->H, d->W, d->Cout};   // (= tie_geom_up / tie_geom_skip of the plan's layer)
  B.gs = Geom{3, 3, 1, 1, false, d->N, d->H, d->W, B.Cs, d->H, d->W, d->Cout};
  B.im = tie_images(dtype, B.gu, B.gs);
  size_t off = TIE_TAB_BYTES + TIE_PREFIX_BYTES;
  B.at.fu = off; off += align_up(conv_image_bytes(B.im.pk_fu, 16));
  B.at.du = off; off += align_up(conv_image_bytes(B.im.pk_du, B.im.du_taps()));
  if (B.Cs > 0) {
    B.at.fs = off; off += align_up(conv_image_bytes(B.im.pk_fs, 9));
    B.at.ds = off; off += align_up(conv_image_bytes(B.im.pk_ds, 9));
  }
  B.dk4_off = off; off += align_up(((size_t)16 * B.Ca + (size_t)9 * B.Cs) * d->Cout * sizeof(float));
  B.bytes = off;
  tie_pack_jobs(B.im, B.at, 0, d->Cout, d->Cin, B.Ca, B.Cs, B.jobs, B.prefix, B.total);
  return OCTSEG_OK;
}

int tied_build(int pass, int dtype, const octseg_conv_layer_desc* d, int wg_target, Tied& B) {
  const std::string who = "tied_layer_op: ";
  auto bad_arg = [&](const char* m) { return fail(OCTSEG_BAD_ARG, who + m); };
  if (pass != OCTSEG_CONV_FORWARD && pass != OCTSEG_CONV_BACKWARD_DATA && pass != OCTSEG_CONV_BACKWARD_WEIGHT) return bad_arg("unknown pass");
  const int rc = tied_shape(dtype, d, B);
  if (rc != OCTSEG_OK) return rc;
  const bool fwd = pass == OCTSEG_CONV_FORWARD, dgrad = pass == OCTSEG_CONV_BACKWARD_DATA;
  if (wg_target < 0) return bad_arg("negative wg_target");
  if (d->wscale || d->bias || d->relu_out || d->stat_slab || d->slab_row0 || d->head)
    return bad_arg("wscale, bias, relu_out, the slab and head mode are not part of a tied pass (training only; the statistics are a sweep of their own)");
  if (!aligned(d->w) || !aligned(d->dy) || !aligned(d->dW) || !aligned(d->scratch)) return bad_arg("misaligned pointer");
  if (d->scratch == nullptr) return bad_arg("null scratch");
  if (d->scratch_bytes < B.bytes) return bad_arg("scratch smaller than octseg_tied_layer_scratch_bytes()");
  SrcDesc src[MAX_SRC];
  int c0 = 0;
  for (int i = 0; i < d->nsrc; ++i) {
    const octseg_conv_src& s = d->src[i];
    // (the data gradient reads dy: its sources only say where the gradient goes, their affine fields are not looked at)
    if (!dgrad && (s.scale != nullptr) != (s.shift != nullptr)) return bad_arg("scale and shift come together");
    if (!dgrad && s.relu && s.scale == nullptr) return bad_arg("relu without the affine (the plan never builds it)");
    if (!dgrad && (s.ptr == nullptr || !aligned(s.ptr) || !aligned(s.scale) || !aligned(s.shift))) return bad_arg("null or misaligned source pointer");
    SrcDesc o;
    o.ptr = s.ptr; o.scale = dgrad ? nullptr : s.scale; o.shift = dgrad ? nullptr : s.shift; o.C = s.C; o.c0 = c0; o.H = s.H; o.W = s.W; o.up = s.up;
    o.relu = s.relu ? 1 : 0;
    src[i] = o;
    c0 += s.C;
  }
  char* ws = (char*)d->scratch;
  const int O = d->Cout;
  if (fwd) {   // tied_forward
    if (d->w == nullptr) return bad_arg("null weight");
    if (d->dst[0].ptr == nullptr || !aligned(d->dst[0].ptr)) return bad_arg("null or misaligned destination");
    if (d->dst[0].accum || d->dst[0].pool) return bad_arg("the tied forward stores its output (no accum, no pool)");
    DstDesc dd;
    dd.ptr = d->dst[0].ptr; dd.C = O; dd.c0 = 0; dd.cn = O; dd.H = d->H; dd.W = d->W; dd.accum = 0; dd.pool = 0;
    if (B.Cs > 0) {
      std::vector<ConvArgs> v;
      fwd_launches(B.gs, v);
      ConvArgs& a = v[0];
      a.nsrc = B.ns - 1;
      for (int i = 1; i < B.ns; ++i) { a.src[i - 1] = src[i]; a.src[i - 1].c0 -= B.Ca; }
      a.W = ws + B.at.fs;
      a.dst[0] = dd; a.ndst = 1; a.out_mode = OUT_STORE;
      B.conv.push_back(a);
    }
    std::vector<ConvArgs> v;
    fwd_launches(B.gu, v);
    for (auto& a : v) {
      a.nsrc = 1; a.src[0] = src[0]; a.src[0].up = 0; a.src[0].c0 = 0;
      a.W = ws + B.at.fu;
      dd.accum = B.Cs > 0 ? 1 : 0;   // (the four parities are disjoint: without a skip launch each one stores its own pixels)
      a.dst[0] = dd; a.ndst = 1; a.out_mode = OUT_STORE;
      B.conv.push_back(a);
    }
  } else if (dgrad) {   // conv_backward, L.tie & 2
    if (d->w == nullptr || d->dy == nullptr) return bad_arg("null weight or dy");
    for (int i = 0; i < d->nsrc; ++i) {
      if (d->dst[i].ptr == nullptr || !aligned(d->dst[i].ptr)) return bad_arg("null or misaligned destination");
      if (d->dst[i].pool) return bad_arg("pool: the tied data gradient is computed at the low resolution, nothing is pooled");
    }
    const size_t esz = dtype_size(dtype);
    std::vector<ConvArgs> lu;
    B.masked = B.im.du_masked;
    if (B.masked) { lu.resize(1); tied_dgrad_masked(B.gu, lu[0]); }
    else dgrad_launches(B.gu, lu);   // (one launch: 16 taps at stride 2 over dy)
    for (int k = 0; k < (int)lu.size(); ++k) {
      ConvArgs& a = lu[k];
      if (B.masked) {
        for (int p = 0; p < 4; ++p) {   // plane p of dy as a tensor of its own: first pixel (p >> 1, p & 1), doubled pixel and row strides
          SrcDesc& s = a.src[p];
          s.ptr = (const char*)d->dy + ((size_t)(p >> 1) * d->W + (p & 1)) * O * esz;
          s.scale = nullptr; s.shift = nullptr; s.C = 2 * O; s.c0 = p * O; s.H = d->H / 2; s.W = d->W; s.up = 0; s.relu = 0;
        }
      } else {
        SrcDesc s;
        s.ptr = d->dy; s.scale = nullptr; s.shift = nullptr; s.C = O; s.c0 = 0; s.H = d->H; s.W = d->W; s.up = 0; s.relu = 0;
        a.src[0] = s; a.nsrc = 1;
        a.Cin = O;
      }
      a.W = ws + B.at.du;
      DstDesc t;
      t.ptr = d->dst[0].ptr; t.C = B.Ca; t.c0 = 0; t.cn = B.Ca; t.H = d->H / 2; t.W = d->W / 2; t.accum = k == 0 ? (d->dst[0].accum ? 1 : 0) : 1; t.pool = 0;
      a.dst[0] = t; a.ndst = 1; a.out_mode = OUT_STORE; a.bias = nullptr; a.stat_slab = nullptr;
      B.conv.push_back(a);
    }
    if (B.Cs > 0) {
      std::vector<ConvArgs> ls;
      dgrad_launches(B.gs, ls);
      ConvArgs& a = ls[0];
      SrcDesc s;
      s.ptr = d->dy; s.scale = nullptr; s.shift = nullptr; s.C = O; s.c0 = 0; s.H = d->H; s.W = d->W; s.up = 0; s.relu = 0;
      a.src[0] = s; a.nsrc = 1;
      a.Cin = O;
      a.W = ws + B.at.ds;
      int nd = 0, cc = 0;
      for (int i = 1; i < d->nsrc; ++i) {
        DstDesc t;
        t.ptr = d->dst[i].ptr; t.C = src[i].C; t.c0 = cc; t.cn = src[i].C; t.H = d->H; t.W = d->W; t.accum = d->dst[i].accum ? 1 : 0; t.pool = 0;
        a.dst[nd++] = t;
        cc += src[i].C;
      }
      a.ndst = nd; a.out_mode = OUT_STORE; a.bias = nullptr; a.stat_slab = nullptr;
      B.conv.push_back(a);
    }
  } else {   // conv_backward, L.tie & 4
    if (d->dy == nullptr || d->dW == nullptr) return bad_arg("null dy or dW");
    float* dK4 = (float*)(ws + B.dk4_off);
    float* dW3s = dK4 + (size_t)16 * O * B.Ca;
    wgrad_launches(B.gu, B.wg);
    for (auto& a : B.wg) {
      a.nsrc = 1; a.src[0] = src[0]; a.src[0].up = 0; a.src[0].c0 = 0;
      a.dy = d->dy; a.dyC = O; a.dW = dK4; a.stamp = nullptr;
      a.wg_target = wg_target;
    }
    B.convt16 = wgrad_convt16_eligible(B.wg[0], dtype);   // all four parities from one staged window (wgrad_convt.hip)
    if (B.Cs > 0) {
      std::vector<WgradArgs> lw;
      wgrad_launches(B.gs, lw);
      WgradArgs& a = lw[0];
      a.nsrc = B.ns - 1;
      for (int i = 1; i < B.ns; ++i) { a.src[i - 1] = src[i]; a.src[i - 1].c0 -= B.Ca; }
      a.dy = d->dy; a.dyC = O; a.dW = dW3s; a.stamp = nullptr;
      a.wg_target = wg_target;
      B.wg.push_back(a);
    }
  }
  return OCTSEG_OK;
}

int tied_route_of(const ConvArgs& a, int dtype) {
  const int r = public_route(a, dtype);
  if (a.taps_per_src == 0) return r;
  return r == OCTSEG_ROUTE_MFMA11 ? OCTSEG_ROUTE_MFMA11_MASKED : r == OCTSEG_ROUTE_MFMA16 ? OCTSEG_ROUTE_MFMA16_MASKED : r;
}

}  // namespace

extern "C" {

int octseg_tied_layer_op(int pass, int dtype, const octseg_conv_layer_desc* d, int wg_target, void* stream) {
  Tied B;
  const int rc = tied_build(pass, dtype, d, wg_target, B);
  if (rc != OCTSEG_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)d->scratch;
  if (pass == OCTSEG_CONV_BACKWARD_WEIGHT) {
    const size_t O = d->Cout;
    float* dK4 = (float*)(ws + B.dk4_off);
    float* dW3s = dK4 + (size_t)16 * O * B.Ca;
    HIPCHK(hipMemsetAsync(dK4, 0, ((size_t)16 * B.Ca + (size_t)9 * B.Cs) * O * sizeof(float), st));
    if (B.convt16) HIPCHK(launch_wgrad_convt16(dtype, B.wg[0], st));
    else
      for (int k = 0; k < 4; ++k) HIPCHK(launch_wgrad(dtype, B.wg[k], st));
    if (B.Cs > 0) HIPCHK(launch_wgrad(dtype, B.wg[4], st));
    HIPCHK(launch_tied_fold(dK4, B.Cs > 0 ? dW3s : nullptr, d->dW, d->Cout, B.Ca, B.Cs, st));
    return OCTSEG_OK;
  }
  // the images as the plan packs them: one launch_pack_all over the layer's jobs (table and prefix sums at the head of the scratch)
  HIPCHK(hipMemcpyAsync(ws, B.jobs.data(), B.jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(ws + TIE_TAB_BYTES, B.prefix.data(), B.prefix.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));   // (the two host vectors die with this call)
  HIPCHK(launch_pack_all(dtype, d->w, ws, (const PackJob*)ws, (const unsigned long long*)(ws + TIE_TAB_BYTES), (int)B.jobs.size(), B.total, 0, st));
  for (auto& a : B.conv) HIPCHK(launch_conv(dtype, a, st));
  return OCTSEG_OK;
}

int octseg_tied_layer_route(int pass, int dtype, const octseg_conv_layer_desc* d, int wg_target, int* route_per_launch, int* nlaunch) {
  if (route_per_launch == nullptr || nlaunch == nullptr) return fail(OCTSEG_BAD_ARG, "tied_layer_route: null output");
  Tied B;
  const int rc = tied_build(pass, dtype, d, wg_target, B);
  if (rc != OCTSEG_OK) return rc;
  int n = 0;
  if (pass == OCTSEG_CONV_BACKWARD_WEIGHT) {
    auto name = [&](const WgradArgs& a) {
      const WgradRoute r = wgrad_route(a, dtype);
      return a.ntaps <= 0 ? -1 : r == WROUTE_THIN ? (int)OCTSEG_WROUTE_THIN : r == WROUTE_1X1 ? (int)OCTSEG_WROUTE_WGRAD1X1 : (int)OCTSEG_WROUTE_MFMA;
    };
    if (B.convt16) route_per_launch[n++] = OCTSEG_WROUTE_CONVT16;
    else
      for (int k = 0; k < 4; ++k) route_per_launch[n++] = name(B.wg[k]);
    if (B.Cs > 0) route_per_launch[n++] = name(B.wg[4]);
  } else {
    for (auto& a : B.conv) route_per_launch[n++] = tied_route_of(a, dtype);
  }
  *nlaunch = n;
  return OCTSEG_OK;
}

size_t octseg_tied_layer_scratch_bytes(int dtype, const octseg_conv_layer_desc* d) {
  Tied B;
  return tied_shape(dtype, d, B) == OCTSEG_OK ? B.bytes : 0;
}

int octseg_side_wgs(void) { return side_wgs(); }

}  // extern "C"
