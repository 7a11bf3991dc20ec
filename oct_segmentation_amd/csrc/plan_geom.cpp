// plan_geom.cpp -- tap tables and launch geometry: how one conv layer (plain, strided, transposed, tied) becomes the ConvArgs / WgradArgs
// of its forward, data-gradient and weight-gradient launches, and the OCTSEG_TIED switches that choose the tied decomposition.
#include "plan_internal.h"

namespace octseg {
namespace detail {

// ================================================================ tap tables / launch geometry
static void set_taps(int* tdy, int* tdx, int* tw, int n, int& ntaps, int& min_dy,
                     int& min_dx, int& span_y, int& span_x) {
  ntaps = n;
  if (n == 0) { min_dy = min_dx = 0; span_y = span_x = 1; return; }
  int mny = 127, mnx = 127, mxy = -127, mxx = -127;
  for (int i = 0; i < n; ++i) {
    mny = std::min(mny, (int)tdy[i]); mxy = std::max(mxy, (int)tdy[i]);
    mnx = std::min(mnx, (int)tdx[i]); mxx = std::max(mxx, (int)tdx[i]);
  }
  (void)tw;
  min_dy = mny; min_dx = mnx; span_y = mxy - mny + 1; span_x = mxx - mnx + 1;
}

// forward launches: taps + grid + output mapping (sources / weights / destinations filled by caller)
void fwd_launches(const Geom& g, std::vector<ConvArgs>& out) {
  if (!g.transposed) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    int n = 0;
    for (int r = 0; r < g.R; ++r)
      for (int s = 0; s < g.S; ++s) { a.tap_dy[n] = r - g.pad; a.tap_dx[n] = s - g.pad; a.tap_w[n] = r * g.S + s; ++n; }
    set_taps(a.tap_dy, a.tap_dx, a.tap_w, n, a.ntaps, a.min_dy, a.min_dx, a.span_y, a.span_x);
    a.istride = g.stride; a.N = g.N; a.IH = g.IH; a.IW = g.IW; a.OH = g.OH; a.OW = g.OW;
    a.Cin = g.Cin; a.Cout = g.Cout; a.ostride = 1; a.ooy = a.oox = 0;
    out.push_back(a);
  } else {  // ConvTranspose2d k4 s2 p1: one launch per output parity, 2x2 taps each
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        int n = 0;
        for (int r = 0; r < g.R; ++r) {
          if (((py + g.pad - r) & 1) != 0) continue;
          for (int s = 0; s < g.S; ++s) {
            if (((px + g.pad - s) & 1) != 0) continue;
            a.tap_dy[n] = (py + g.pad - r) / 2; a.tap_dx[n] = (px + g.pad - s) / 2; a.tap_w[n] = r * g.S + s; ++n;
          }
        }
        set_taps(a.tap_dy, a.tap_dx, a.tap_w, n, a.ntaps, a.min_dy, a.min_dx, a.span_y, a.span_x);
        a.istride = 1; a.N = g.N; a.IH = g.IH; a.IW = g.IW; a.OH = g.IH; a.OW = g.IW;  // grid = input grid
        a.Cin = g.Cin; a.Cout = g.Cout; a.ostride = 2; a.ooy = py; a.oox = px;
        out.push_back(a);
      }
  }
}

// data-gradient launches: "input" is dy [N,OH,OW,Cout], "output" is dx [N,IH,IW,Cin]
void dgrad_launches(const Geom& g, std::vector<ConvArgs>& out) {
  if (g.transposed) {  // gradient of ConvT = plain conv k4 s2 p1 over dy
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    int n = 0;
    for (int r = 0; r < g.R; ++r)
      for (int s = 0; s < g.S; ++s) { a.tap_dy[n] = r - g.pad; a.tap_dx[n] = s - g.pad; a.tap_w[n] = r * g.S + s; ++n; }
    set_taps(a.tap_dy, a.tap_dx, a.tap_w, n, a.ntaps, a.min_dy, a.min_dx, a.span_y, a.span_x);
    a.istride = 2; a.N = g.N; a.IH = g.OH; a.IW = g.OW; a.OH = g.IH; a.OW = g.IW;
    a.Cin = g.Cout; a.Cout = g.Cin; a.ostride = 1;
    out.push_back(a);
  } else if (g.stride == 1) {
    ConvArgs a;
    memset(&a, 0, sizeof(a));
    int n = 0;
    for (int r = 0; r < g.R; ++r)
      for (int s = 0; s < g.S; ++s) { a.tap_dy[n] = g.pad - r; a.tap_dx[n] = g.pad - s; a.tap_w[n] = r * g.S + s; ++n; }
    set_taps(a.tap_dy, a.tap_dx, a.tap_w, n, a.ntaps, a.min_dy, a.min_dx, a.span_y, a.span_x);
    a.istride = 1; a.N = g.N; a.IH = g.OH; a.IW = g.OW; a.OH = g.IH; a.OW = g.IW;
    a.Cin = g.Cout; a.Cout = g.Cin; a.ostride = 1;
    out.push_back(a);
  } else {  // stride 2: one launch per input parity
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        int n = 0;
        for (int r = 0; r < g.R; ++r) {
          if (((py + g.pad - r) & 1) != 0) continue;
          for (int s = 0; s < g.S; ++s) {
            if (((px + g.pad - s) & 1) != 0) continue;
            a.tap_dy[n] = (py + g.pad - r) / 2; a.tap_dx[n] = (px + g.pad - s) / 2; a.tap_w[n] = r * g.S + s; ++n;
          }
        }
        set_taps(a.tap_dy, a.tap_dx, a.tap_w, n, a.ntaps, a.min_dy, a.min_dx, a.span_y, a.span_x);
        a.istride = 1; a.N = g.N; a.IH = g.OH; a.IW = g.OW;
        a.OH = (g.IH - py + 1) / 2; a.OW = (g.IW - px + 1) / 2;
        a.Cin = g.Cout; a.Cout = g.Cin; a.ostride = 2; a.ooy = py; a.oox = px;
        out.push_back(a);
      }
  }
}

void wgrad_launches(const Geom& g, std::vector<WgradArgs>& out) {
  if (!g.transposed) {
    WgradArgs a;
    memset(&a, 0, sizeof(a));
    int n = 0;
    for (int r = 0; r < g.R; ++r)
      for (int s = 0; s < g.S; ++s) { a.tap_dy[n] = r - g.pad; a.tap_dx[n] = s - g.pad; a.tap_w[n] = r * g.S + s; ++n; }
    set_taps(a.tap_dy, a.tap_dx, a.tap_w, n, a.ntaps, a.min_dy, a.min_dx, a.span_y, a.span_x);
    a.istride = g.stride; a.N = g.N; a.IH = g.IH; a.IW = g.IW; a.OH = g.OH; a.OW = g.OW;
    a.Cin = g.Cin; a.Cout = g.Cout; a.DH = g.OH; a.DW = g.OW; a.dstride = 1;
    out.push_back(a);
  } else {
    for (int py = 0; py < 2; ++py)
      for (int px = 0; px < 2; ++px) {
        WgradArgs a;
        memset(&a, 0, sizeof(a));
        int n = 0;
        for (int r = 0; r < g.R; ++r) {
          if (((py + g.pad - r) & 1) != 0) continue;
          for (int s = 0; s < g.S; ++s) {
            if (((px + g.pad - s) & 1) != 0) continue;
            a.tap_dy[n] = (py + g.pad - r) / 2; a.tap_dx[n] = (px + g.pad - s) / 2; a.tap_w[n] = r * g.S + s; ++n;
          }
        }
        set_taps(a.tap_dy, a.tap_dx, a.tap_w, n, a.ntaps, a.min_dy, a.min_dx, a.span_y, a.span_x);
        a.istride = 1; a.N = g.N; a.IH = g.IH; a.IW = g.IW; a.OH = g.IH; a.OW = g.IW;
        a.Cin = g.Cin; a.Cout = g.Cout; a.DH = g.OH; a.DW = g.OW; a.dstride = 2; a.doy = py; a.dox = px;
        out.push_back(a);
      }
  }
}

// Data gradient of the tied ConvTranspose2d (Geom of the ConvT: IH x IW = the low-resolution map) as ONE stride-1 launch whose four sources are
// dy's parity planes (virtual channels [p O, (p + 1) O) = plane p), every plane contracting
// with its own 2 x 2 of the 3 x 3 tap offsets (ConvArgs::taps_per_src, conv_mfma.hip's masked loop): plane (py, px) at offset (dy, dx) carries
// kernel tap r = py + 1 + 2 dy, s = px + 1 + 2 dx where that lies in [0, 3].  Sources (pointers, strides) are filled by the caller.
void tied_dgrad_masked(const Geom& g, ConvArgs& a) {
  memset(&a, 0, sizeof(a));
  int n = 0;
  for (int t = 0; t < 9; ++t) { a.tap_dy[n] = t / 3 - 1; a.tap_dx[n] = t % 3 - 1; a.tap_w[n] = t; ++n; }
  set_taps(a.tap_dy, a.tap_dx, a.tap_w, n, a.ntaps, a.min_dy, a.min_dx, a.span_y, a.span_x);
  a.istride = 1; a.N = g.N; a.IH = g.IH; a.IW = g.IW; a.OH = g.IH; a.OW = g.IW;
  a.Cin = 4 * g.Cout; a.Cout = g.Cin; a.ostride = 1;
  a.taps_per_src = 4; a.nsrc = 4;
  for (int p = 0; p < 4; ++p) {
    const int py = p >> 1, px = p & 1;
    int list = 0, k = 0;
    for (int t = 0; t < 9; ++t) {
      const int r = py + 1 + 2 * (t / 3 - 1), s = px + 1 + 2 * (t % 3 - 1);
      if (r >= 0 && r <= 3 && s >= 0 && s <= 3) list |= t << (4 * k++);
    }
    a.src_taps[p] = list;
    SrcDesc d{};
    d.C = 2 * g.Cout; d.c0 = p * g.Cout; d.H = g.IH; d.W = 2 * g.IW;
    a.src[p] = d;
  }
}

// OCTSEG_TIED=[f][d][w]: which passes of the decoder's (nearest x2, concat, 3x3) layers run the tied decomposition (ConvLayer::tie).  Default `dw`.
// The weight gradient is the same fp32 sum of the same bf16 products in another order, 16 instead of 36 of them per source pixel; the data
// gradient contracts dy with the 4x4 image (sums of taps rounded to bf16 once) at the low resolution instead of with nine taps at the high one
// followed by a 2x2 pool.  U-Net++/resnet101 16 x 704^2: weight-gradient class 21.4 -> 18.4 ms, data-gradient class 21.6 -> 20.1 ms
// (profiles/r4_tied_ab.txt).  `f` is exact up to bf16 rounding too but not faster: four parity launches that add into the output plus a sweep
// for the BatchNorm statistics -- opt-in.  OCTSEG_TIED=0 (or any string without f / d / w): none.
int tie_mask() {   // (read when a plan is built, so that one process can hold plans of both kinds)
  const char* e = getenv("OCTSEG_TIED");
  if (e == nullptr) return 2 | 4;
  int v = 0;
  for (const char* c = e; *c; ++c) v |= *c == 'f' ? 1 : *c == 'd' ? 2 : *c == 'w' ? 4 : 0;
  return v;
}

Geom tie_geom_up(const ConvLayer& L) { return Geom{4, 4, 2, 1, true, L.N, L.IH / 2, L.IW / 2, L.tie_Ca, L.OH, L.OW, L.Cout}; }
Geom tie_geom_skip(const ConvLayer& L) { return Geom{3, 3, 1, 1, false, L.N, L.IH, L.IW, L.tie_Cs, L.OH, L.OW, L.Cout}; }

// A decoder layer of the form (nearest x2, concat, 3x3 stride 1 pad 1 + BatchNorm, no bias) over 2-byte elements whose sources all want a gradient.
bool tie_eligible(const TieQuery& q) {
  if (!(q.esz == 2 && !q.transposed && !q.stem && !q.head && !q.sliced && !q.accum_out && q.R == 3 && q.S == 3 && q.stride == 1 && q.pad == 1 &&
        q.has_bn && !q.has_bias && q.nsrc >= 1 && q.up0_whole_grad))
    return false;
  if (!q.skips_plain_grad) return false;
  // (narrow layers stay whole: below 64 channels a launch is a single K chunk and the thin kernels own the 16 / 32-channel decoder tail)
  return q.Ca >= 64 && q.Ca % 8 == 0 && q.Cs % 8 == 0 && q.Cout >= 32 && (q.Cs == 0 || q.Cs >= 32);
}

TieImages tie_images(int dtype, const Geom& gu, const Geom& gs) {
  TieImages im{};
  std::vector<ConvArgs> v;
  fwd_launches(gu, v);
  im.pk_fu = conv_pack_info(v[0], dtype);
  v.clear();
  im.du_masked = false;
  if (gu.Cout % 64 == 0) {   // one masked launch over the four parity planes: the planes are whole K chunks
    ConvArgs am;
    tied_dgrad_masked(gu, am);
    DstDesc dd{}; dd.H = gu.IH; dd.W = gu.IW; dd.C = gu.Cin; dd.cn = gu.Cin; am.dst[0] = dd; am.ndst = 1;
    if (conv_masked_eligible(am, dtype)) { im.du_masked = true; v.push_back(am); }
  }
  if (!im.du_masked) dgrad_launches(gu, v);
  im.pk_du = conv_pack_info(v[0], dtype);
  if (gs.Cin > 0) {
    v.clear(); fwd_launches(gs, v);
    im.pk_fs = conv_pack_info(v[0], dtype);
    v.clear(); dgrad_launches(gs, v);
    im.pk_ds = conv_pack_info(v[0], dtype);
  }
  return im;
}

// the tied images: 4x4 kernel over the upsampled source's channels, the plain 3x3 over the skip channels (training only: no fold)
void tie_pack_jobs(const TieImages& im, const TieOffsets& at, size_t w_off, int Cout, int Cin, int Ca, int Cs, std::vector<PackJob>& jobs,
                   std::vector<unsigned long long>& prefix, unsigned long long& total) {
  auto add = [&](size_t dst, int ntaps, int I, int c0, int tr, int tied, const ConvPackInfo& pk) {
    PackJob j{w_off, dst, ntaps, Cout, I, tr, pk.BN, pk.RB, pk.nchunks, pk.ntiles, ~(size_t)0, Cin, c0, tied};
    prefix.push_back(total);
    jobs.push_back(j);
    total += (unsigned long long)ntaps * pk.nchunks * pk.ntiles * pk.BN * (pk.RB / 16);
  };
  add(at.fu, 16, Ca, 0, 0, 1, im.pk_fu);
  add(at.du, im.du_taps(), Ca, 0, 1, im.du_masked ? 2 : 1, im.pk_du);
  if (Cs > 0) {
    add(at.fs, 9, Cs, Ca, 0, 0, im.pk_fs);
    add(at.ds, 9, Cs, Ca, 1, 0, im.pk_ds);
  }
}

// algorithmic multiply-accumulates of one pass (forward = dgrad = wgrad) over a conv layer
double layer_macs(const ConvLayer& L) {
  return (double)L.N * L.OH * L.OW * L.Cout * (L.stem ? 3.0 * L.stem_k * L.stem_k : (double)L.Cin * (L.transposed ? 4.0 : (double)L.R * L.S));
}

// ---------------------------------------------------------------- single-op entry points (octseg_conv2d_*): what they accept, and its Geom
bool geom_ok(int dtype, int Cin, int Cout, int R, int S, int stride, int transposed) {
  const int v = ev_vec(dtype);
  (void)Cout;
  if (Cin % v != 0) return false;
  if (R != S || R < 1 || R > 7) return false;
  if (stride != 1 && stride != 2) return false;
  if (transposed && !(R == 4 && stride == 2)) return false;
  return true;
}
Geom op_geom(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int transposed) {
  Geom g{R, S, stride, pad, transposed != 0, N, H, W, Cin, 0, 0, Cout};
  if (transposed) { g.OH = H * 2; g.OW = W * 2; } else { g.OH = (H + 2 * pad - R) / stride + 1; g.OW = (W + 2 * pad - S) / stride + 1; }
  return g;
}

}  // namespace detail
}  // namespace octseg
