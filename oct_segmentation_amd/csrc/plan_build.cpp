// plan_build.cpp -- graph builder and workspace planner: the encoders (torchvision ResNet, timm RegNet, EfficientNet) and the smp decoders
// (U-Net, U-Net++, LinkNet, FPN, DeepLabV3 / V3+, PSPNet, MAnet, PAN) as a list of ops, the forward lanes, and the workspace layout.
//
// The graph is built once per (arch, encoder, classes, B, H, W, dtype).  Convolutions never see
// a materialised concat / upsample / BN-apply: a consumer reads `Value`s = (raw tensor, BN id)
// and applies relu(x*scale+shift) while staging (conv_mfma.hip).  Only residual-block outputs
// (and LinkNet skip sums) are materialised by bn_act.  Module / parameter names reproduce the
// smp 0.3.3 + torchvision module tree so that the Python facade can serve a reference
// state_dict (reference src/predict.py:39-48).
#include "plan_internal.h"

#include <map>

namespace octseg {
namespace detail {

// ================================================================ graph builder
namespace {

struct Builder {
  octseg_plan* P;
  size_t esz;

  int tensor(int N, int H, int W, int C, bool need_grad = true, bool external = false) {
    TensorInfo t{N, H, W, C, 0, 0, need_grad, external};
    P->tensors.push_back(t);
    return (int)P->tensors.size() - 1;
  }
  int param(const std::string& name, int kind, int R, int S, int O, int I, int KP) {
    ParamInfo p;
    p.name = name; p.kind = kind; p.R = R; p.S = S; p.O = O; p.I = I; p.KP = KP;
    p.numel = kind == OCTSEG_P_VEC ? (size_t)O : kind == OCTSEG_P_STEM ? (size_t)O * KP : (size_t)R * S * O * I;
    p.off = P->param_numel;
    P->param_numel += (p.numel + 3) / 4 * 4;  // keep 16-byte alignment of every parameter
    P->params.push_back(p);
    return (int)P->params.size() - 1;
  }
  int bn(const std::string& name, int C, int y, bool lazy) {
    BNInfo b;
    b.name = name; b.C = C;
    b.gamma = param(name + ".weight", OCTSEG_P_VEC, 1, 1, C, 1, 0);
    b.beta = param(name + ".bias", OCTSEG_P_VEC, 1, 1, C, 1, 0);
    b.rm_off = P->buffer_numel; P->buffer_numel += C;
    b.rv_off = P->buffer_numel; P->buffer_numel += C;
    b.ss_off = 0; b.rows = 0; b.lazy = lazy; b.y = y;
    const TensorInfo& t = P->tensors[y];
    b.count = (double)t.N * t.H * t.W;
    P->bns.push_back(b);
    return (int)P->bns.size() - 1;
  }

  // conv (+ optional BN whose statistics the epilogue emits).  Returns Value{raw output, bn}.
  Value conv(const std::string& name, const std::vector<ConvSrc>& srcs, int Cout, int R, int stride, int pad,
             const std::string& bn_name, bool bias, bool transposed = false, bool head = false,
             bool stem = false, bool bn_lazy = true, int accum_into = -1, bool defer_fin = false) {
    ConvLayer L;
    L.name = name; L.R = R; L.S = R; L.stride = stride; L.pad = pad;
    L.transposed = transposed; L.head = head; L.stem = stem; L.srcs = srcs; L.Cout = Cout;
    int Cin = 0;
    const TensorInfo& t0 = P->tensors[srcs[0].v.t];
    L.N = t0.N; L.IH = t0.H << srcs[0].up; L.IW = t0.W << srcs[0].up;
    for (auto& s : srcs) Cin += s.cn ? s.cn : P->tensors[s.v.t].C;
    L.Cin = Cin;
    L.stem_k = P->stem_k;
    if (transposed) { L.OH = L.IH * 2; L.OW = L.IW * 2; }
    else { L.OH = (L.IH + 2 * pad - R) / stride + 1; L.OW = (L.IW + 2 * pad - R) / stride + 1; }
    if (stem) L.w = param(name + ".weight", OCTSEG_P_STEM, P->stem_k, P->stem_k, Cout, 3, Cin);
    else L.w = param(name + ".weight", transposed ? OCTSEG_P_CONVT : OCTSEG_P_CONV, R, R, Cout, Cin, 0);
    L.b = bias ? param(name + ".bias", OCTSEG_P_VEC, 1, 1, Cout, 1, 0) : -1;
    L.OP = (Cout + 15) / 16 * 16;
    L.out = head ? -1 : (accum_into >= 0 ? accum_into : tensor(L.N, L.OH, L.OW, Cout));
    L.accum_out = accum_into >= 0;
    L.bn = -1; L.wimg_fwd_off = L.wimg_dgrad_off = 0; L.has_dgrad = false;
    P->convs.push_back(L);
    const int ci = (int)P->convs.size() - 1;
    Op op; op.kind = OP_CONV; op.conv = ci;
    P->ops.push_back(op);
    const double taps = (double)R * R;
    // MACs: every output pixel of a plain conv sees R*S*Cin; ConvT k4 s2 sees 4 taps per output pixel
    P->fwd_macs += (double)L.N * L.OH * L.OW * Cout * (stem ? 3.0 * P->stem_k * P->stem_k : (double)Cin * (transposed ? 4.0 : taps));
    Value v; v.t = L.out; v.bn = -1;
    if (!bn_name.empty()) {
      const int b = bn(bn_name, Cout, L.out, bn_lazy);
      P->convs[ci].bn = b;
      if (!defer_fin) {            // (deferred: the statistics come from another tensor, stats_fin() finishes the BatchNorm)
        Op f; f.kind = OP_BN_FIN; f.bn = b;
        P->ops.push_back(f);
      }
      v.bn = b;
    }
    return v;
  }
  // Grouped k x k conv (timm RegNet's conv2: groups = width / group width) + BatchNorm: G independent convs, each reading a channel
  // slice of `in` and writing a channel slice of ONE output tensor through the ordinary conv kernels (slices are pointer offsets: the
  // descriptors carry the channel stride separately).  The parameter of group g is named <name>.weight#g<g>: the host mirror joins the
  // groups along dim 0 into torch's [Cout][gw][k][k] tensor.  The BatchNorm's statistics come from the whole tensor (OP_STATS).
  Value gconv(const std::string& name, Value in, int C, int R, int stride, int pad, int gw, const std::string& bn_name) {
    const TensorInfo ti = P->tensors[in.t];
    const int OH = (ti.H + 2 * pad - R) / stride + 1, OW = (ti.W + 2 * pad - R) / stride + 1;
    const int out = tensor(ti.N, OH, OW, C);
    for (int g = 0; g < C / gw; ++g) {
      ConvSrc sc; sc.v = in; sc.up = 0; sc.c0 = g * gw; sc.cn = gw;
      conv(name, {sc}, gw, R, stride, pad, "", false, false, false, false, true, out);
      ConvLayer& L = P->convs.back();
      L.accum_out = false; L.sliced = true; L.out_c0 = g * gw;
      P->params[L.w].name = name + ".weight#g" + std::to_string(g);
    }
    const int bi = bn(bn_name, C, out, true);
    for (auto& L : P->convs) if (L.sliced && L.out == out) L.fold_bn = bi;
    stats_fin(bi, out);
    Value v; v.t = out; v.bn = bi;
    return v;
  }
  // out = relu?(bn(y) + res) + post, materialised
  int bn_act(Value y, Value res, int post, bool relu) {
    const TensorInfo& t = P->tensors[y.t];
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_BN_ACT; op.y = y; op.res = res; op.post = post; op.relu = relu; op.out = o;
    P->ops.push_back(op);
    P->bns[y.bn].lazy = false;
    if (res.t >= 0 && res.bn >= 0) P->bns[res.bn].lazy = false;
    return o;
  }
  int maxpool(int in) {
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, t.H / 2, t.W / 2, t.C);
    Op op; op.kind = OP_MAXPOOL; op.in = in; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  // ---- FPN decoder pieces (smp decoders/fpn/decoder.py, restated in oracle/nets.py)
  int up2(int in) {   // F.interpolate(x, scale_factor=2, mode='nearest'), materialised: the FPNBlock's skip conv accumulates into it
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, t.H * 2, t.W * 2, t.C);
    Op op; op.kind = OP_UP2; op.in = in; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  int gn_act(const std::string& name, int y, int up) {   // GroupNorm(32) + ReLU (+ bilinear x2, align_corners=True)
    const TensorInfo& t = P->tensors[y];
    GNInfo g;
    g.name = name; g.C = t.C; g.G = 32; g.y = y;
    g.gamma = param(name + ".weight", OCTSEG_P_VEC, 1, 1, t.C, 1, 0);
    g.beta = param(name + ".bias", OCTSEG_P_VEC, 1, 1, t.C, 1, 0);
    g.part_off = g.ss_off = g.stat_off = g.coef_off = 0;
    P->gns.push_back(g);
    const int o = tensor(t.N, t.H * up, t.W * up, t.C);
    Op op; op.kind = OP_GN; op.in = y; op.out = o; op.gn = (int)P->gns.size() - 1; op.up = up;
    P->ops.push_back(op);
    return o;
  }
  // ---- DeepLabV3+ pieces (smp decoders/deeplabv3, restated in oracle/nets.py; kernels in deeplab.hip)
  int parity(int in, bool to_coarse) {   // [N][H][W] -> [4N][H/2][W/2] parity sub-grids (a dilation-2 3x3 is a plain 3x3 on them), or back
    const TensorInfo& t = P->tensors[in];
    const int o = to_coarse ? tensor(t.N * 4, t.H / 2, t.W / 2, t.C) : tensor(t.N / 4, t.H * 2, t.W * 2, t.C);
    Op op; op.kind = OP_PARITY; op.in = in; op.out = o; op.up = to_coarse ? 1 : 0;
    P->ops.push_back(op);
    return o;
  }
  int dw_param(const std::string& name, int C) { return param(name + ".weight", OCTSEG_P_CONV, 3, 3, C, 1, 0); }   // torch [C][1][3][3]
  void dw(int in, int out, int oc0, int dwp, int wc0, int dil) {   // depthwise 3x3 of `in` into channels [oc0, oc0 + C_in) of `out`
    const TensorInfo& t = P->tensors[in];
    Op op; op.kind = OP_DW; op.in = in; op.out = out; op.oc0 = oc0; op.dwp = dwp; op.wc0 = wc0; op.up = dil;
    P->ops.push_back(op);
    P->fwd_macs += (double)t.N * t.H * t.W * t.C * 9.0;
  }
  int gap(int in) {                       // AdaptiveAvgPool2d(1)
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, 1, 1, t.C);
    Op op; op.kind = OP_GAP; op.in = in; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  int bcast(int in, int H, int W) {       // F.interpolate of a 1x1 map to H x W
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, H, W, t.C);
    Op op; op.kind = OP_BCAST; op.in = in; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  int drope(int in) {                     // nn.Dropout (element-wise), keep mask injected
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_DROPE; op.in = in; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  int upb(int in, int up) {               // nn.UpsamplingBilinear2d(scale_factor=up)
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, t.H * up, t.W * up, t.C);
    Op op; op.kind = OP_UPB; op.in = in; op.out = o; op.up = up;
    P->ops.push_back(op);
    return o;
  }
  // ---- DeepLabV3 pieces: a dense dilated 3x3 conv as a plain conv on the mosaic of its rate^2 sub-grids (deeplab.hip)
  int mosaic(int in, int r, bool to_mosaic, int H = 0, int W = 0) {
    const TensorInfo& t = P->tensors[in];
    int o;
    if (to_mosaic) { const int hs = (t.H + r - 1) / r, ws = (t.W + r - 1) / r; o = tensor(t.N, r * (hs + 1) + 1, r * (ws + 1) + 1, t.C); }
    else o = tensor(t.N, H, W, t.C);
    Op op; op.kind = OP_MOSAIC; op.in = in; op.out = o; op.up = r; op.oc0 = to_mosaic ? 1 : 0;
    P->ops.push_back(op);
    return o;
  }
  // the BatchNorm `bn` (created by a conv with defer_fin) normalises tensor y, not the conv's own output: statistics from y, then finalize
  void stats_fin(int bn, int y) {
    const TensorInfo& t = P->tensors[y];
    P->bns[bn].y = y;
    P->bns[bn].count = (double)t.N * t.H * t.W;
    Op s; s.kind = OP_STATS; s.bn = bn; s.in = y;
    P->ops.push_back(s);
    Op f; f.kind = OP_BN_FIN; f.bn = bn;
    P->ops.push_back(f);
  }
  // ---- PSPNet pieces (smp decoders/pspnet, restated in oracle/nets.py)
  int binpool(int in, int k) {            // nn.AdaptiveAvgPool2d((k, k))
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, k, k, t.C);
    Op op; op.kind = OP_BINPOOL; op.in = in; op.out = o; op.up = k;
    P->ops.push_back(op);
    return o;
  }
  int resize(int in, int H, int W) {      // F.interpolate(size=(H, W), mode='bilinear', align_corners=True)
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, H, W, t.C);
    Op op; op.kind = OP_RESIZE; op.in = in; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  int relu(int in) {
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_RELU; op.in = in; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  int drop2d(int in) {                    // nn.Dropout2d, keep pattern [N][C] injected
    const TensorInfo& t = P->tensors[in];
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_DROP2D; op.in = in; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  // timm SEModule(channels, rd_channels): x * sigmoid(fc2(relu(fc1(mean_hw(x))))), x = the materialised activation `in`
  int se(const std::string& name, int in, int rd) {
    const TensorInfo t = P->tensors[in];
    const int g = gap(in);
    const Value f1 = conv(name + ".fc1", {{mat_(g), 0}}, rd, 1, 1, 0, "", true);
    const int r1 = relu(f1.t);
    const Value f2 = conv(name + ".fc2", {{mat_(r1), 0}}, t.C, 1, 1, 0, "", true);
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_SEGATE; op.in = in; op.ins[0] = f2.t; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  static Value mat_(int t) { Value v; v.t = t; v.bn = -1; return v; }
  // ---- PAN pieces (smp decoders/pan, restated in oracle/nets.py; kernels in pan.hip)
  int add2(int a, int c) {
    const TensorInfo t = P->tensors[a];
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_ADD; op.in = a; op.ins[0] = c; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  // GAUBlock(x = low-level feature, y = high-level map): bilinear(y) + relu(bn(conv3x3(x))) * sigmoid(bn(conv1x1(mean(y))))
  int gau(const std::string& pre, int x, int y) {
    const TensorInfo tx = P->tensors[x];
    const Value v2 = conv(pre + ".conv2.conv", {{mat_(x), 0}}, 32, 3, 1, 1, pre + ".conv2.bn", true);
    const int xg = bn_act(v2, Value(), -1, true);
    const Value v1 = conv(pre + ".conv1.1.conv", {{mat_(gap(y)), 0}}, 32, 1, 1, 0, pre + ".conv1.1.bn", true);
    const int s = bn_act(v1, Value(), -1, false);
    const int z = tensor(tx.N, tx.H, tx.W, 32);
    { Op op; op.kind = OP_SEGATE; op.in = xg; op.ins[0] = s; op.out = z; P->ops.push_back(op); }
    return add2(resize(y, tx.H, tx.W), z);
  }
  // FPABlock: global branch b1, 1x1 branch mid, the one-channel pyramid (pan.hip), out = pyramid * mid + b1
  int fpa(const std::string& pre, int x) {
    const TensorInfo t = P->tensors[x];
    const Value vb = conv(pre + ".branch1.1.conv", {{mat_(gap(x)), 0}}, 32, 1, 1, 0, pre + ".branch1.1.bn", true);
    const int b1 = bn_act(vb, Value(), -1, true);
    const Value vm = conv(pre + ".mid.0.conv", {{mat_(x), 0}}, 32, 1, 1, 0, pre + ".mid.0.bn", true);
    const int mid = bn_act(vm, Value(), -1, true);
    const char* names[6] = {".down1.1", ".down2.1", ".down3.1", ".down3.2", ".conv2", ".conv1"};
    const int ks[6] = {7, 5, 3, 3, 5, 7};
    for (int l = 0; l < 6; ++l) {
      const std::string n = pre + names[l];
      P->fpa.w[l] = param(n + ".conv.weight", OCTSEG_P_CONV, ks[l], ks[l], 1, l == 0 ? t.C : 1, 0);
      P->fpa.b[l] = param(n + ".conv.bias", OCTSEG_P_VEC, 1, 1, 1, 1, 0);
      P->fpa.bn[l] = bn(n + ".bn", 1, x, false);
    }
    P->fpa.pool = tensor(t.N, t.H / 2, t.W / 2, t.C);                 // MaxPool2d(2, 2) of the feature (the 7x7 conv's input)
    const int o = tensor(t.N, t.H, t.W, 32);
    Op op; op.kind = OP_FPA; op.in = x; op.ins[0] = mid; op.ins[1] = b1; op.out = o;
    P->ops.push_back(op);
    P->fwd_macs += (double)t.N * (t.H / 2) * (t.W / 2) * 49.0 * t.C;
    return o;
  }
  // ---- MAnet pieces (smp decoders/manet, restated in oracle/nets.py; kernels in pab.hip / se.hip / effnet.hip's sefc)
  // nn.Sequential(AdaptiveAvgPool2d(1), Conv2d(C, rd, 1), ReLU, Conv2d(rd, C, 1), Sigmoid) up to the sigmoid: the excitation s [N][1][1][C]
  int se_relu(const std::string& name, int in, int rd) {
    const TensorInfo t = P->tensors[in];
    const int g = gap(in);
    const int s = tensor(t.N, 1, 1, t.C);
    Op f; f.kind = OP_SEFC; f.in = g; f.out = s; f.up = rd; f.oc0 = 0;
    f.ins[0] = param(name + ".1.weight", OCTSEG_P_CONV, 1, 1, rd, t.C, 0);
    f.ins[1] = param(name + ".1.bias", OCTSEG_P_VEC, 1, 1, rd, 1, 0);
    f.ins[2] = param(name + ".3.weight", OCTSEG_P_CONV, 1, 1, t.C, rd, 0);
    f.ins[3] = param(name + ".3.bias", OCTSEG_P_VEC, 1, 1, t.C, 1, 0);
    P->ops.push_back(f);
    return s;
  }
  int gate2(int in, int s1, int s2) {    // in * (sigmoid(s1) + sigmoid(s2))
    const TensorInfo t = P->tensors[in];
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_SEGATE; op.in = in; op.ins[0] = s1; op.ins[1] = s2; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  int pab(const std::string& name, int x) {
    const TensorInfo t = P->tensors[x];
    const Value top = conv(name + ".top_conv", {{mat_(x), 0}}, 64, 1, 1, 0, "", true);
    const Value center = conv(name + ".center_conv", {{mat_(x), 0}}, 64, 1, 1, 0, "", true);
    const Value bottom = conv(name + ".bottom_conv", {{mat_(x), 0}}, t.C, 3, 1, 1, "", true);
    const int y = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_PAB; op.in = x; op.ins[0] = top.t; op.ins[1] = center.t; op.ins[2] = bottom.t; op.out = y;
    P->ops.push_back(op);
    P->fwd_macs += (double)t.N * t.H * t.W * t.H * t.W * (64.0 + t.C);
    return conv(name + ".out_conv", {{mat_(y), 0}}, t.C, 3, 1, 1, "", true).t;
  }
  // ---- EfficientNet pieces (efficientnet_pytorch MBConvBlock, restated in oracle/nets.py; kernels in effnet.hip)
  void set_bn_effnet(int bi) { P->bns[bi].eps = 1e-3f; P->bns[bi].momentum = 0.01f; }
  // out = act(bn(y)) * drop_connect + post, materialised (swish has no lazy form in the conv kernels' staging)
  int bnx(Value y, int act, int post, int dc_block, bool conv_bn) {
    const TensorInfo t = P->tensors[y.t];
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_BNX; op.y = y; op.up = act; op.post = post; op.oc0 = dc_block; op.out = o; op.conv_bn = conv_bn;
    P->ops.push_back(op);
    P->bns[y.bn].lazy = false;
    return o;
  }
  // depthwise K x K conv (torch weight [C][1][K][K] -> arena [K][K][C]) + BatchNorm (statistics from the output tensor)
  Value dwg(const std::string& name, int in, int K, int stride, int pad, const std::string& bn_name) {
    const TensorInfo t = P->tensors[in];
    const int OH = (t.H + stride - 1) / stride, OW = (t.W + stride - 1) / stride;      // TF "same"
    const int o = tensor(t.N, OH, OW, t.C);
    Op op; op.kind = OP_DWG; op.in = in; op.out = o; op.dwp = param(name + ".weight", OCTSEG_P_CONV, K, K, t.C, 1, 0); op.up = stride; op.oc0 = pad; op.wc0 = K;
    P->ops.push_back(op);
    P->fwd_macs += (double)t.N * OH * OW * t.C * K * K;
    const int bi = bn(bn_name, t.C, o, false);
    set_bn_effnet(bi);
    stats_fin(bi, o);
    Value v; v.t = o; v.bn = bi;
    return v;
  }
  // squeeze-excite of an MBConv block: mean -> W1, b1 -> swish -> W2, b2 -> sigmoid gate (reduction widths 4 .. 160: a kernel of its own)
  int se_effnet(const std::string& pre, int in, int rd) {
    const TensorInfo t = P->tensors[in];
    const int g = gap(in);
    const int s = tensor(t.N, 1, 1, t.C);
    Op f; f.kind = OP_SEFC; f.in = g; f.out = s; f.up = rd; f.oc0 = 1;
    f.ins[0] = param(pre + "._se_reduce.weight", OCTSEG_P_CONV, 1, 1, rd, t.C, 0);
    f.ins[1] = param(pre + "._se_reduce.bias", OCTSEG_P_VEC, 1, 1, rd, 1, 0);
    f.ins[2] = param(pre + "._se_expand.weight", OCTSEG_P_CONV, 1, 1, t.C, rd, 0);
    f.ins[3] = param(pre + "._se_expand.bias", OCTSEG_P_VEC, 1, 1, t.C, 1, 0);
    P->ops.push_back(f);
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_SEGATE; op.in = in; op.ins[0] = s; op.out = o;
    P->ops.push_back(op);
    return o;
  }
  // parameters and buffers of a layer the graph never runs (smp's get_encoder(depth=3) keeps layer3 / layer4 in the module and in state_dict)
  void dead_conv(const std::string& name, int Cout, int Cin, int R) { param(name + ".weight", OCTSEG_P_CONV, R, R, Cout, Cin, 0); }
  void dead_bn(const std::string& name, int C, int any_tensor) { bn(name, C, any_tensor, false); }
  int merge4(const int (&ins)[4]) {   // MergeBlock('add') + Dropout2d: every summand receives the same gradient -> one shared buffer
    const TensorInfo& t = P->tensors[ins[0]];
    const int o = tensor(t.N, t.H, t.W, t.C);
    Op op; op.kind = OP_MERGE; op.out = o;
    for (int i = 0; i < 4; ++i) { op.ins[i] = ins[i]; if (i > 0) P->tensors[ins[i]].grad_alias = ins[0]; }
    P->ops.push_back(op);
    return o;
  }
};

Value mat(int t) { Value v; v.t = t; v.bn = -1; return v; }

// torchvision ResNet; returns materialised features f1..f5
// dilate4: smp's make_dilated(output_stride=16) -- every conv of layer4 at stride 1 / dilation 2.  Built as the ordinary layer4 (stride 1)
// on the parity re-arrangement of layer3's output (deeplab.hip header): no dilated conv kernel exists or is needed.
// depth: smp encoder_depth (5, or 3 for PSPNet: layer3 / layer4 keep their parameters and buffers but no op).
// dilate3: smp's make_dilated(8) on top -- layer3 at dilation 2 (one parity re-arrangement), layer4 at dilation 4 (= dilation 2 on layer3's
// sub-grids: a second, nested re-arrangement); both are undone behind layer4.
std::vector<int> build_resnet(Builder& b, const std::string& enc, bool dilate4 = false, int depth = 5, bool dilate3 = false) {
  octseg_plan* P = b.P;
  const bool bottleneck = enc == "resnet50" || enc == "resnet101" || enc == "resnet152";
  int nblocks[4];
  if (enc == "resnet18") { int v[4] = {2, 2, 2, 2}; memcpy(nblocks, v, sizeof v); }
  else if (enc == "resnet34" || enc == "resnet50") { int v[4] = {3, 4, 6, 3}; memcpy(nblocks, v, sizeof v); }
  else if (enc == "resnet152") { int v[4] = {3, 8, 36, 3}; memcpy(nblocks, v, sizeof v); }
  else { int v[4] = {3, 4, 23, 3}; memcpy(nblocks, v, sizeof v); }
  const int KP = 160;  // 7*7*3 = 147 padded to a multiple of 32
  P->col_tensor = b.tensor(P->B, P->H / 2, P->W / 2, KP, false);
  { Op op; op.kind = OP_STEM_COL; op.out = P->col_tensor; P->ops.push_back(op); }
  Value ystem = b.conv("encoder.conv1", {{mat(P->col_tensor), 0}}, 64, 1, 1, 0, "encoder.bn1", false, false, false, true);
  std::vector<int> feats;
  int f1 = b.bn_act(ystem, Value(), -1, true);
  feats.push_back(f1);
  int x = b.maxpool(f1);
  int inplanes = 64;
  const int planes_l[4] = {64, 128, 256, 512};
  for (int li = 0; li < 4; ++li) {
    const int planes = planes_l[li];
    const int exp = bottleneck ? 4 : 1;
    const bool dil = (dilate4 && li == 3) || (dilate3 && li >= 2);
    if (li + 2 > depth) {               // a stage behind the last feature the decoder reads: parameters only
      for (int bi = 0; bi < nblocks[li]; ++bi) {
        const int stride = (bi == 0 && li > 0) ? 2 : 1;
        const std::string pre = "encoder.layer" + std::to_string(li + 1) + "." + std::to_string(bi);
        const bool ds = (stride != 1) || (inplanes != planes * exp);
        if (!bottleneck) {
          b.dead_conv(pre + ".conv1", planes, inplanes, 3); b.dead_bn(pre + ".bn1", planes, x);
          b.dead_conv(pre + ".conv2", planes, planes, 3); b.dead_bn(pre + ".bn2", planes, x);
        } else {
          b.dead_conv(pre + ".conv1", planes, inplanes, 1); b.dead_bn(pre + ".bn1", planes, x);
          b.dead_conv(pre + ".conv2", planes, planes, 3); b.dead_bn(pre + ".bn2", planes, x);
          b.dead_conv(pre + ".conv3", planes * 4, planes, 1); b.dead_bn(pre + ".bn3", planes * 4, x);
        }
        if (ds) { b.dead_conv(pre + ".downsample.0", planes * exp, inplanes, 1); b.dead_bn(pre + ".downsample.1", planes * exp, x); }
        inplanes = planes * exp;
      }
      continue;
    }
    if (dil) x = b.parity(x, true);
    for (int bi = 0; bi < nblocks[li]; ++bi) {
      const int stride = (bi == 0 && li > 0 && !dil) ? 2 : 1;
      const std::string pre = "encoder.layer" + std::to_string(li + 1) + "." + std::to_string(bi);
      const bool ds = (stride != 1) || (inplanes != planes * exp);
      Value last;
      if (!bottleneck) {
        Value v1 = b.conv(pre + ".conv1", {{mat(x), 0}}, planes, 3, stride, 1, pre + ".bn1", false);
        last = b.conv(pre + ".conv2", {{v1, 0}}, planes, 3, 1, 1, pre + ".bn2", false);
      } else {
        Value v1 = b.conv(pre + ".conv1", {{mat(x), 0}}, planes, 1, 1, 0, pre + ".bn1", false);
        Value v2 = b.conv(pre + ".conv2", {{v1, 0}}, planes, 3, stride, 1, pre + ".bn2", false);
        last = b.conv(pre + ".conv3", {{v2, 0}}, planes * 4, 1, 1, 0, pre + ".bn3", false);
      }
      Value res = mat(x);
      if (ds) res = b.conv(pre + ".downsample.0", {{mat(x), 0}}, planes * exp, 1, stride, 0, pre + ".downsample.1", false);
      x = b.bn_act(last, res, -1, true);
      inplanes = planes * exp;
    }
    if (dil && li == 3) { x = b.parity(x, false); if (dilate3) x = b.parity(x, false); }
    feats.push_back(x);
  }
  return feats;  // f1 (S/2) .. f5 (S/32)
}

// timm RegNet as smp's RegNetEncoder wraps it (oracle/nets.py RegNetEncoder; reference configs/tune.yaml:19-24: timm-regnetx_002 /
// timm-regnetx_064): stem 3x3 s2 -> 32 + BN + ReLU (im2col rows of 27 values padded to 32, then the GEMM the ResNet stem uses in f32),
// four stages of bottleneck blocks -- conv1 1x1, conv2 GROUPED 3x3 (stride 2 in a stage's first block), conv3 1x1 without activation,
// 1x1 stride-s conv shortcut where the shape changes, ReLU behind the sum.  Widths / depths / group width: timm generate_regnet.
struct RegNetCfg { int w[4], d[4], gw; bool se; };   // se: RegNetY -- SEModule behind conv2 with round(0.25 * block input channels) reduction channels
static bool regnet_cfg(const std::string& enc, RegNetCfg& c) {
  if (enc == "timm-regnetx_002") { c = RegNetCfg{{24, 56, 152, 368}, {1, 1, 4, 7}, 8, false}; return true; }
  if (enc == "timm-regnetx_064") { c = RegNetCfg{{168, 392, 784, 1624}, {2, 4, 10, 1}, 56, false}; return true; }
  if (enc == "timm-regnety_120") { c = RegNetCfg{{224, 448, 896, 2240}, {2, 5, 11, 1}, 112, true}; return true; }
  return false;
}
std::vector<int> build_regnet(Builder& b, const RegNetCfg& cfg, int depth) {
  octseg_plan* P = b.P;
  P->stem_k = 3; P->stem_pad = 1;
  const int KP = 32;   // 3 * 3 * 3 = 27 padded
  P->col_tensor = b.tensor(P->B, P->H / 2, P->W / 2, KP, false);
  { Op op; op.kind = OP_STEM_COL; op.out = P->col_tensor; P->ops.push_back(op); }
  Value ystem = b.conv("encoder.stem.conv", {{mat(P->col_tensor), 0}}, 32, 1, 1, 0, "encoder.stem.bn", false, false, false, true);
  std::vector<int> feats;
  int x = b.bn_act(ystem, Value(), -1, true);
  feats.push_back(x);
  int prev = 32;
  for (int si = 0; si < 4; ++si) {
    const int w = cfg.w[si];
    for (int bi = 0; bi < cfg.d[si]; ++bi) {
      const int stride = bi == 0 ? 2 : 1;
      const std::string pre = "encoder.s" + std::to_string(si + 1) + ".b" + std::to_string(bi + 1);
      if (si + 2 > depth) {   // (smp encoder_depth 3: the stage keeps its parameters and buffers, no op)
        b.dead_conv(pre + ".conv1.conv", w, prev, 1); b.dead_bn(pre + ".conv1.bn", w, x);
        for (int g = 0; g < w / cfg.gw; ++g) { b.dead_conv(pre + ".conv2.conv", cfg.gw, cfg.gw, 3); P->params.back().name = pre + ".conv2.conv.weight#g" + std::to_string(g); }
        b.dead_bn(pre + ".conv2.bn", w, x);
        if (cfg.se) {
          const int rd = (int)lround(prev * 0.25);
          b.dead_conv(pre + ".se.fc1", rd, w, 1); b.param(pre + ".se.fc1.bias", OCTSEG_P_VEC, 1, 1, rd, 1, 0);
          b.dead_conv(pre + ".se.fc2", w, rd, 1); b.param(pre + ".se.fc2.bias", OCTSEG_P_VEC, 1, 1, w, 1, 0);
        }
        b.dead_conv(pre + ".conv3.conv", w, w, 1); b.dead_bn(pre + ".conv3.bn", w, x);
        if (prev != w || stride != 1) { b.dead_conv(pre + ".downsample.conv", w, prev, 1); b.dead_bn(pre + ".downsample.bn", w, x); }
        prev = w;
        continue;
      }
      Value v1 = b.conv(pre + ".conv1.conv", {{mat(x), 0}}, w, 1, 1, 0, pre + ".conv1.bn", false);
      Value v2 = b.gconv(pre + ".conv2.conv", v1, w, 3, stride, 1, cfg.gw, pre + ".conv2.bn");
      if (cfg.se) {   // RegNetY: the gate acts on relu(bn(conv2)), materialised for it
        const int xa = b.bn_act(v2, Value(), -1, true);
        v2 = mat(b.se(pre + ".se", xa, (int)lround(prev * 0.25)));
      }
      Value v3 = b.conv(pre + ".conv3.conv", {{v2, 0}}, w, 1, 1, 0, pre + ".conv3.bn", false);
      Value res = mat(x);
      if (prev != w || stride != 1) res = b.conv(pre + ".downsample.conv", {{mat(x), 0}}, w, 1, stride, 0, pre + ".downsample.bn", false);
      x = b.bn_act(v3, res, -1, true);
      prev = w;
    }
    if (si + 2 <= depth) feats.push_back(x);
  }
  return feats;
}

// efficientnet_pytorch's EfficientNet as smp's EfficientNetEncoder runs it (oracle/nets.py EfficientNetEncoder; reference configs/tune.yaml:
// 25-28: efficientnet-b0 / -b5 / -b7): stem 3x3 s2 (static "same" padding: top / left 0) + BN + swish, MBConv blocks -- expand 1x1 + BN + swish
// (expand ratio 6), depthwise k3 / k5 stride 1 / 2 + BN + swish, squeeze-excite with swish, project 1x1 + BN, id skip with drop_connect
// where stride 1 and equal widths --, features behind smp's stage indices; _conv_head / _bn1 stay as never-run parameters.
struct EffBlock { int k, stride, expand, cin, cout, se, pad; };
struct EffCfg { int stem, head, stage_idx[3]; std::vector<EffBlock> blocks; };
static bool effnet_cfg(const std::string& enc, EffCfg& c) {
  double w, d; int size;
  if (enc == "efficientnet-b0") { w = 1.0; d = 1.0; size = 224; int si[3] = {3, 5, 9}; memcpy(c.stage_idx, si, sizeof si); }
  else if (enc == "efficientnet-b5") { w = 1.6; d = 2.2; size = 456; int si[3] = {8, 13, 27}; memcpy(c.stage_idx, si, sizeof si); }
  else if (enc == "efficientnet-b7") { w = 2.0; d = 3.1; size = 600; int si[3] = {11, 18, 38}; memcpy(c.stage_idx, si, sizeof si); }
  else return false;
  auto rf = [&](int f) { const double x = f * w; int n = std::max(8, (int)(x + 4) / 8 * 8); if (n < 0.9 * x) n += 8; return n; };
  auto same_pad_top = [](int ih, int k, int s) { const int oh = (ih + s - 1) / s; const int pad = std::max((oh - 1) * s + k - ih, 0); return pad / 2; };
  static const int B[7][6] = {{1, 3, 1, 1, 32, 16}, {2, 3, 2, 6, 16, 24}, {2, 5, 2, 6, 24, 40}, {3, 3, 2, 6, 40, 80}, {3, 5, 1, 6, 80, 112}, {4, 5, 2, 6, 112, 192},
                              {1, 3, 1, 6, 192, 320}};
  c.stem = rf(32); c.head = rf(1280); c.blocks.clear();
  size = (size + 1) / 2;       // behind the stem (its own static padding: top 0 for the even nominal sizes 224 / 456 / 600)
  for (auto& r : B) {
    const int rep = (int)ceil(d * r[0]), cin = rf(r[4]), cout = rf(r[5]);
    for (int j = 0; j < rep; ++j) {
      const int st = j == 0 ? r[2] : 1, ci = j == 0 ? cin : cout;
      c.blocks.push_back(EffBlock{r[1], st, r[3], ci, cout, std::max(1, (int)(ci * 0.25)), same_pad_top(size, r[1], st)});
      size = (size + st - 1) / st;
    }
  }
  return true;
}
std::vector<int> build_effnet(Builder& b, const EffCfg& cfg, int depth) {
  octseg_plan* P = b.P;
  P->stem_k = 3; P->stem_pad = 0;
  const int KP = 32;
  P->col_tensor = b.tensor(P->B, P->H / 2, P->W / 2, KP, false);
  { Op op; op.kind = OP_STEM_COL; op.out = P->col_tensor; P->ops.push_back(op); }
  Value ystem = b.conv("encoder._conv_stem", {{mat(P->col_tensor), 0}}, cfg.stem, 1, 1, 0, "encoder._bn0", false, false, false, true);
  b.set_bn_effnet(ystem.bn);
  std::vector<int> feats;
  int x = b.bnx(ystem, 1, -1, -1, true);
  feats.push_back(x);
  const int nb = (int)cfg.blocks.size();
  int stage = 0;      // blocks [0, stage_idx[0]) -> feature 2, ...
  bool live = true;
  for (int bi = 0; bi < nb; ++bi) {
    const EffBlock& e = cfg.blocks[bi];
    const std::string pre = "encoder._blocks." + std::to_string(bi);
    const int mid = e.cin * e.expand;
    if (stage < 3 && bi == cfg.stage_idx[stage]) { feats.push_back(x); ++stage; if ((int)feats.size() >= depth) live = false; }
    if (!live) {        // (smp encoder_depth 3: the later blocks keep parameters and buffers, no op)
      if (e.expand != 1) { b.dead_conv(pre + "._expand_conv", mid, e.cin, 1); b.dead_bn(pre + "._bn0", mid, x); }
      b.param(pre + "._depthwise_conv.weight", OCTSEG_P_CONV, e.k, e.k, mid, 1, 0); b.dead_bn(pre + "._bn1", mid, x);
      b.dead_conv(pre + "._se_reduce", e.se, mid, 1); b.param(pre + "._se_reduce.bias", OCTSEG_P_VEC, 1, 1, e.se, 1, 0);
      b.dead_conv(pre + "._se_expand", mid, e.se, 1); b.param(pre + "._se_expand.bias", OCTSEG_P_VEC, 1, 1, mid, 1, 0);
      b.dead_conv(pre + "._project_conv", e.cout, mid, 1); b.dead_bn(pre + "._bn2", e.cout, x);
      continue;
    }
    int t = x;
    if (e.expand != 1) {
      Value v = b.conv(pre + "._expand_conv", {{mat(x), 0}}, mid, 1, 1, 0, pre + "._bn0", false);
      b.set_bn_effnet(v.bn);
      t = b.bnx(v, 1, -1, -1, true);
    }
    Value vd = b.dwg(pre + "._depthwise_conv", t, e.k, e.stride, e.pad, pre + "._bn1");
    const int td = b.bnx(vd, 1, -1, -1, false);
    const int ts = b.se_effnet(pre, td, e.se);
    Value vp = b.conv(pre + "._project_conv", {{mat(ts), 0}}, e.cout, 1, 1, 0, pre + "._bn2", false);
    b.set_bn_effnet(vp.bn);
    const bool id_skip = e.stride == 1 && e.cin == e.cout;
    int dc = -1;
    if (id_skip && bi > 0) { dc = (int)P->dc_rates.size(); P->dc_rates.push_back(0.2f * (float)bi / (float)nb); }   // (block 0: rate 0 -> no drop)
    x = b.bnx(vp, 0, id_skip ? x : -1, dc, true);
  }
  if (live) feats.push_back(x);
  // smp deletes only _fc: the classifier's 1x1 conv and BatchNorm stay in the module and in state_dict
  b.dead_conv("encoder._conv_head", cfg.head, cfg.blocks.back().cout, 1);
  b.dead_bn("encoder._bn1", cfg.head, x);
  return feats;
}

Value unet_block(Builder& b, const std::string& pre, Value x, const std::vector<Value>& skips, int cout) {
  std::vector<ConvSrc> srcs;
  srcs.push_back({x, 1});
  for (auto& s : skips) srcs.push_back({s, 0});
  Value v1 = b.conv(pre + ".conv1.0", srcs, cout, 3, 1, 1, pre + ".conv1.1", false);
  return b.conv(pre + ".conv2.0", {{v1, 0}}, cout, 3, 1, 1, pre + ".conv2.1", false);
}

}  // namespace

// Forward lanes.  A dense decoder (U-Net++) has nodes that do not need the deepest encoder feature: they are moved right
// behind the encoder op that completes their inputs and run on a side stream beside the deep encoder stages and the
// deepest decoder nodes, whose small grids (44^2 / 22^2 maps) leave most of the chip idle (measured: +1.7 % frames/s
// with everything that does not depend on layer4 on the side lane, +0.8 % with only what does not depend on layer3).  Any topological order is a valid plan; the backward
// walks the same list in reverse.  Nothing moves for U-Net / LinkNet (their decoders start at the deepest feature).
static void assign_lanes(octseg_plan* P) {
  const int n = (int)P->ops.size();
  auto op_name = [&](const Op& o) -> std::string {
    if (o.kind == OP_CONV) return P->convs[o.conv].name;
    if (o.kind == OP_BN_FIN) return P->bns[o.bn].name;
    return std::string();
  };
  int enc_end = n, l3_begin = -1;
  for (int i = 0; i < n; ++i) {
    const std::string nm = op_name(P->ops[i]);
    if (nm.rfind("decoder.", 0) == 0 || nm.rfind("segmentation_head", 0) == 0) { enc_end = i; break; }
  }
  const std::string stage = "encoder.layer4.";   // the encoder stage the side lane may not depend on
  for (int i = 0; i < enc_end; ++i)
    if (op_name(P->ops[i]).rfind(stage, 0) == 0) { l3_begin = i; break; }
  if (enc_end >= n || l3_begin < 0) return;
  std::vector<int> prod_t(P->tensors.size(), -1), fin_bn(P->bns.size(), -1), depmax(n, -1);
  auto dep = [&](int i, int j) {   // op i reads what op j wrote
    if (j < 0) return;
    depmax[i] = std::max(depmax[i], j < enc_end ? j : depmax[j]);
  };
  auto dep_val = [&](int i, const Value& v) {
    if (v.t >= 0) dep(i, prod_t[v.t]);
    if (v.bn >= 0) dep(i, fin_bn[v.bn]);
  };
  for (int i = 0; i < n; ++i) {
    const Op& o = P->ops[i];
    switch (o.kind) {
      case OP_STEM_COL: prod_t[o.out] = i; break;
      case OP_CONV: {
        const ConvLayer& L = P->convs[o.conv];
        for (auto& sct : L.srcs) dep_val(i, sct.v);
        if (L.out >= 0) prod_t[L.out] = i;
        break;
      }
      case OP_BN_FIN: dep(i, prod_t[P->bns[o.bn].y]); fin_bn[o.bn] = i; break;
      case OP_BN_ACT: dep_val(i, o.y); dep_val(i, o.res); if (o.post >= 0) dep(i, prod_t[o.post]); prod_t[o.out] = i; break;
      case OP_MAXPOOL: dep(i, prod_t[o.in]); prod_t[o.out] = i; break;
    }
  }
  std::vector<std::vector<int>> after(enc_end);   // side ops to insert behind encoder op e
  std::vector<char> side(n, 0);
  bool any = false;
  for (int i = enc_end; i < n; ++i)
    if (depmax[i] >= 0 && depmax[i] < l3_begin && op_name(P->ops[i]).rfind("decoder.", 0) == 0) {
      // the lane starts no earlier than the last op in front of layer3 that it can follow
      side[i] = 1; any = true;
      after[depmax[i]].push_back(i);
    }
  if (!any) return;
  std::vector<Op> order;
  order.reserve(n);
  for (int e = 0; e < enc_end; ++e) {
    order.push_back(P->ops[e]);
    for (int i : after[e]) { Op o = P->ops[i]; o.lane = 1; order.push_back(o); }
  }
  for (int i = enc_end; i < n; ++i)
    if (!side[i]) order.push_back(P->ops[i]);
  P->ops.swap(order);
  P->has_lanes = true;
}

int build_plan(octseg_plan* P) {
  Builder b{P, dtype_size(P->dtype)};
  const bool dlv3 = P->arch == "deeplabv3";
  std::vector<int> f;
  RegNetCfg rcfg;
  const bool regnet = regnet_cfg(P->encoder, rcfg);
  EffCfg ecfg;
  const bool effnet = effnet_cfg(P->encoder, ecfg);
  if ((effnet || regnet) && P->arch == "pan") return fail(OCTSEG_UNSUPPORTED_ARCH, "PAN dilates its encoder (output stride 16): built over the ResNets");
  if (effnet) {
    if (P->arch == "deeplabv3plus" || dlv3) return fail(OCTSEG_UNSUPPORTED_ARCH, "EfficientNet encoders cannot be dilated (smp raises for DeepLabV3 / DeepLabV3+ over them too)");
    f = build_effnet(b, ecfg, P->arch == "pspnet" ? 3 : 5);
  } else if (regnet) {
    if (P->arch == "deeplabv3plus" || dlv3) return fail(OCTSEG_UNSUPPORTED_ARCH, "the dilated RegNet encoders (smp make_dilated) are not built");
    if ((P->arch == "linknet" && (rcfg.w[3] / 4) % 8 != 0) || (P->arch == "pspnet" && (rcfg.w[1] / 4) % 8 != 0))   // LinkNet's decoder blocks and PSPNet's pyramid branches run on a QUARTER of a feature's channels
      return fail(OCTSEG_UNSUPPORTED_ARCH, P->arch + " over " + P->encoder + ": its decoder narrows a feature to a quarter of its channels (" +
                  std::to_string(rcfg.w[P->arch == "pspnet" ? 1 : 3]) + " / 4 is not a multiple of the 8-channel vector the NHWC kernels move)");
    f = build_regnet(b, rcfg, P->arch == "pspnet" ? 3 : 5);
  } else {
    f = build_resnet(b, P->encoder, P->arch == "deeplabv3plus" || P->arch == "pan" || dlv3, P->arch == "pspnet" ? 3 : 5, dlv3);  // f[0]=f1 .. f[4]=f5
  }
  while (f.size() < 5) f.push_back(f.back());       // (PSPNet: three features; the slots of the others are never read)
  std::vector<int> fr(f.rbegin(), f.rend());          // features[1:][::-1]: f5, f4, f3, f2, f1
  std::vector<int> ench;
  for (int t : fr) ench.push_back(P->tensors[t].C);
  const int dec[5] = {256, 128, 64, 32, 16};
  Value x;
  int head_k = 3;
  if (P->arch == "unet") {
    x = mat(fr[0]);
    for (int i = 0; i < 5; ++i) {
      std::vector<Value> skips;
      if (i < 4) skips.push_back(mat(fr[i + 1]));
      x = unet_block(b, "decoder.blocks." + std::to_string(i), x, skips, dec[i]);
    }
  } else if (P->arch == "unetplusplus") {
    // smp UnetPlusPlusDecoder
    std::vector<int> skip_ch(ench.begin() + 1, ench.end());
    skip_ch.push_back(0);
    std::map<std::string, Value> dense;
    auto key = [](int d, int l) { return "x_" + std::to_string(d) + "_" + std::to_string(l); };
    const int depth = 4;
    for (int layer = 0; layer < 4; ++layer) {
      for (int d = 0; d < depth - layer; ++d) {
        if (layer == 0) {
          const int cout = d == 0 ? dec[0] : skip_ch[d];
          dense[key(d, d)] = unet_block(b, "decoder.blocks." + key(d, d), mat(fr[d]), {mat(fr[d + 1])}, cout);
        } else {
          const int li = d + layer;
          std::vector<Value> cat;
          for (int idx = d + 1; idx <= li; ++idx) cat.push_back(dense[key(idx, li)]);
          cat.push_back(mat(fr[li + 1]));
          const int cout = d == 0 ? dec[li] : skip_ch[li];
          dense[key(d, li)] = unet_block(b, "decoder.blocks." + key(d, li), dense[key(d, li - 1)], cat, cout);
        }
      }
    }
    x = unet_block(b, "decoder.blocks." + key(0, depth), dense[key(0, depth - 1)], {}, dec[4]);
  } else if (P->arch == "pan") {
    // smp PAN (reference sweep, configs/tune.yaml:18) at its defaults: encoder_output_stride 16 (layer4 dilated, as DeepLabV3+), decoder_channels
    // 32, FPA on the last feature, three GAU blocks down to stride 4, 3x3 head + UpsamplingBilinear2d(4)
    head_k = 3;
    P->head_up = 4;
    const TensorInfo t5 = P->tensors[f[4]];
    // (frames below 128 x 128 leave nothing for the pyramid's third max-pool -- torch fails there too; the plan is still built, for its
    //  parameter table, and refuses to run: run_forward)
    if (t5.H < 8 || t5.W < 8) P->run_error = "PAN needs frames of at least 128 x 128 (its pyramid pools the stride-16 feature three times)";
    const int x5 = b.fpa("decoder.fpa", f[4]);
    const int x4 = b.gau("decoder.gau3", f[3], x5);
    const int x3 = b.gau("decoder.gau2", f[2], x4);
    x = mat(b.gau("decoder.gau1", f[1], x3));
  } else if (P->arch == "manet") {
    // smp MAnet (reference sweep, configs/tune.yaml:17) at its defaults: PAB on the deepest feature, MFAB blocks (SE gates on the upsampled
    // high-level path and on the skip, summed) where there is a skip, a plain U-Net block for the last one; 3x3 head on 16 channels
    x = mat(b.pab("decoder.center", fr[0]));
    for (int i = 0; i < 5; ++i) {
      const std::string pre = "decoder.blocks." + std::to_string(i);
      const int in_ch = i == 0 ? ench[0] : dec[i - 1];
      if (i < 4) {
        const int skip = fr[i + 1], skip_ch = ench[i + 1];
        Value v1 = b.conv(pre + ".hl_conv.0.0", {{x, 0}}, in_ch, 3, 1, 1, pre + ".hl_conv.0.1", false);
        Value v2 = b.conv(pre + ".hl_conv.1.0", {{v1, 0}}, skip_ch, 1, 1, 0, pre + ".hl_conv.1.1", false);
        const int hl = b.bn_act(v2, Value(), -1, true);
        const int rd = std::max(1, skip_ch / 16);
        const int s_ll = b.se_relu(pre + ".SE_ll", skip, rd);          // (parameter order of the module: SE_ll before SE_hl)
        const int s_hl = b.se_relu(pre + ".SE_hl", hl, rd);            // mean of the nearest-x2 upsampled map = mean of the map
        const int gated = b.gate2(hl, s_hl, s_ll);                      // the gate is per (image, channel): applied BEFORE the upsample
        x = unet_block(b, pre, mat(gated), {mat(skip)}, dec[i]);
      } else {
        x = unet_block(b, pre, x, {}, dec[i]);
      }
    }
  } else if (P->arch == "linknet") {
    head_k = 1;
    std::vector<int> ch = ench;
    ch.push_back(32);
    x = mat(fr[0]);
    for (int i = 0; i < 5; ++i) {
      const std::string pre = "decoder.blocks." + std::to_string(i) + ".block";
      const int cin = ch[i], mid = cin / 4, cout = ch[i + 1];
      if (mid % 8 != 0)
        return fail(OCTSEG_UNSUPPORTED_ARCH, "linknet over " + P->encoder + ": its decoder narrows a feature to a quarter of its channels (" +
                    std::to_string(cin) + " / 4 is not a multiple of the 8-channel vector the NHWC kernels move)");
      Value v1 = b.conv(pre + ".0.0", {{x, 0}}, mid, 1, 1, 0, pre + ".0.1", false);
      Value v2 = b.conv(pre + ".1.0", {{v1, 0}}, mid, 4, 2, 1, pre + ".1.1", true, true);
      Value v3 = b.conv(pre + ".2.0", {{v2, 0}}, cout, 1, 1, 0, pre + ".2.1", false);
      if (i < 4) x = mat(b.bn_act(v3, Value(), fr[i + 1], true));
      else x = v3;
    }
  } else if (P->arch == "fpn") {
    // smp FPN (reference sweep, configs/tune.yaml:9-18): pyramid_channels 256, segmentation_channels 128, merge 'add', Dropout2d(0.2),
    // head = 1x1 conv at stride 4 + UpsamplingBilinear2d(4).  f[1..4] = c2..c5 (strides 4..32).
    head_k = 1;
    P->head_up = 4;
    int pyr[4];
    pyr[0] = b.conv("decoder.p5", {{mat(f[4]), 0}}, 256, 1, 1, 0, "", true).t;
    const char* lvl[3] = {"decoder.p4", "decoder.p3", "decoder.p2"};
    for (int i = 0; i < 3; ++i) {
      const int up = b.up2(pyr[i]);
      b.conv(std::string(lvl[i]) + ".skip_conv", {{mat(f[3 - i]), 0}}, 256, 1, 1, 0, "", true, false, false, false, true, up);
      pyr[i + 1] = up;
    }
    int seg[4];
    for (int i = 0; i < 4; ++i) {
      const int nup = 3 - i, nblk = nup > 1 ? nup : 1;
      int t = pyr[i];
      for (int j = 0; j < nblk; ++j) {
        const std::string pre = "decoder.seg_blocks." + std::to_string(i) + ".block." + std::to_string(j) + ".block";
        const Value y = b.conv(pre + ".0", {{mat(t), 0}}, 128, 3, 1, 1, "", false);
        t = b.gn_act(pre + ".1", y.t, nup > 0 ? 2 : 1);
      }
      seg[i] = t;
    }
    x = mat(b.merge4(seg));
  } else if (P->arch == "deeplabv3") {
    // smp DeepLabV3 (reference sweep, configs/tune.yaml:9-18) with its defaults: output stride 8, dense ASPP (12, 24, 36), decoder_channels
    // 256, 3x3 conv + BN + ReLU, head = 1x1 conv + UpsamplingBilinear2d(8).  Only the last feature is read.
    head_k = 1;
    P->head_up = 8;
    P->dropout_p = 0.5f;
    const int X = f[4];                       // stride 8
    const TensorInfo tx = P->tensors[X];
    const std::string A = "decoder.0";
    std::vector<ConvSrc> cat;
    cat.push_back({b.conv(A + ".convs.0.0", {{mat(X), 0}}, 256, 1, 1, 0, A + ".convs.0.1", false), 0});
    const int rates[3] = {12, 24, 36};
    for (int i = 0; i < 3; ++i) {             // ASPPConv: dense dilated 3x3 as a plain 3x3 on the mosaic of its sub-grids, BN, ReLU
      const std::string pre = A + ".convs." + std::to_string(i + 1);
      const int m = b.mosaic(X, rates[i], true);
      const Value v = b.conv(pre + ".0", {{mat(m), 0}}, 256, 3, 1, 1, pre + ".1", false, false, false, false, true, -1, true);
      const int yf = b.mosaic(v.t, rates[i], false, tx.H, tx.W);
      b.stats_fin(v.bn, yf);
      Value vf; vf.t = yf; vf.bn = v.bn;
      cat.push_back({vf, 0});
    }
    {
      const std::string pre = A + ".convs.4";
      const int g = b.gap(X);
      const Value v = b.conv(pre + ".1", {{mat(g), 0}}, 256, 1, 1, 0, pre + ".2", false);
      cat.push_back({mat(b.bcast(b.bn_act(v, Value(), -1, true), tx.H, tx.W)), 0});
    }
    const Value pr = b.conv(A + ".project.0", cat, 256, 1, 1, 0, A + ".project.1", false);
    const int pd = b.drope(b.bn_act(pr, Value(), -1, true));
    x = b.conv("decoder.1", {{mat(pd), 0}}, 256, 3, 1, 1, "decoder.2", false);
  } else if (P->arch == "pspnet") {
    // smp PSPNet (reference sweep, configs/tune.yaml:9-18) with its defaults: encoder_depth 3 (the stride-8 feature), pyramid pooling to
    // 1 / 2 / 3 / 6 bins, 1x1 conv to 512 + BN + ReLU, Dropout2d(0.2), 3x3 head + UpsamplingBilinear2d(8)
    head_k = 3;
    P->head_up = 8;
    P->dropout_p = 0.2f;
    const int X = f[2];
    const TensorInfo tx = P->tensors[X];
    const int sizes[4] = {1, 2, 3, 6};
    if ((tx.C / 4) % 8 != 0)
      return fail(OCTSEG_UNSUPPORTED_ARCH, "pspnet over " + P->encoder + ": its pyramid branches run on a quarter of the feature's channels (" +
                  std::to_string(tx.C) + " / 4 is not a multiple of the 8-channel vector the NHWC kernels move)");
    std::vector<ConvSrc> cat;
    for (int i = 0; i < 4; ++i) {
      const std::string pre = "decoder.psp.blocks." + std::to_string(i) + ".pool.1";
      const int g = b.binpool(X, sizes[i]);
      int a;
      if (sizes[i] == 1) a = b.relu(b.conv(pre + ".0", {{mat(g), 0}}, tx.C / 4, 1, 1, 0, "", true).t);      // no BatchNorm on a 1x1 map: biased conv
      else a = b.bn_act(b.conv(pre + ".0", {{mat(g), 0}}, tx.C / 4, 1, 1, 0, pre + ".1", false), Value(), -1, true);
      cat.push_back({mat(b.resize(a, tx.H, tx.W)), 0});
    }
    cat.push_back({mat(X), 0});
    const Value v = b.conv("decoder.conv.0", cat, 512, 1, 1, 0, "decoder.conv.1", false);
    x = mat(b.drop2d(b.bn_act(v, Value(), -1, true)));
  } else if (P->arch == "deeplabv3plus") {
    // smp DeepLabV3Plus (reference sweep, configs/tune.yaml:9-18) with its defaults: encoder_output_stride 16, decoder_channels 256,
    // atrous rates (12, 24, 36), 48-channel high-resolution branch from the stride-4 feature, head = 1x1 conv + UpsamplingBilinear2d(4).
    head_k = 1;
    P->head_up = 4;
    P->dropout_p = 0.5f;
    const int X = f[4];                       // stride 16 (layer4 dilated)
    const TensorInfo tx = P->tensors[X];
    const std::string A = "decoder.aspp.0";
    std::vector<ConvSrc> cat;
    cat.push_back({b.conv(A + ".convs.0.0", {{mat(X), 0}}, 256, 1, 1, 0, A + ".convs.0.1", false), 0});
    const int rates[3] = {12, 24, 36};
    for (int i = 0; i < 3; ++i) {             // ASPPSeparableConv: depthwise dilated 3x3, pointwise 1x1, BN, ReLU
      const std::string pre = A + ".convs." + std::to_string(i + 1);
      const int wp = b.dw_param(pre + ".0.0", tx.C);
      const int t = b.tensor(tx.N, tx.H, tx.W, tx.C);
      b.dw(X, t, 0, wp, 0, rates[i]);
      cat.push_back({b.conv(pre + ".0.1", {{mat(t), 0}}, 256, 1, 1, 0, pre + ".1", false), 0});
    }
    {                                         // ASPPPooling: mean, 1x1 conv, BN (over the batch only), ReLU, resize = broadcast
      const std::string pre = A + ".convs.4";
      const int g = b.gap(X);
      const Value v = b.conv(pre + ".1", {{mat(g), 0}}, 256, 1, 1, 0, pre + ".2", false);
      cat.push_back({mat(b.bcast(b.bn_act(v, Value(), -1, true), tx.H, tx.W)), 0});
    }
    const Value pr = b.conv(A + ".project.0", cat, 256, 1, 1, 0, A + ".project.1", false);
    const int pd = b.drope(b.bn_act(pr, Value(), -1, true));
    const int wp1 = b.dw_param("decoder.aspp.1.0", 256);
    const int t1 = b.tensor(tx.N, tx.H, tx.W, 256);
    b.dw(pd, t1, 0, wp1, 0, 1);
    const Value a2 = b.conv("decoder.aspp.1.1", {{mat(t1), 0}}, 256, 1, 1, 0, "decoder.aspp.2", false);
    const int au = b.upb(b.bn_act(a2, Value(), -1, true), 4);
    const Value h1 = b.conv("decoder.block1.0", {{mat(f[1]), 0}}, 48, 1, 1, 0, "decoder.block1.1", false);
    const int hm = b.bn_act(h1, Value(), -1, true);
    const int wp2 = b.dw_param("decoder.block2.0.0", 256 + 48);
    const TensorInfo tu = P->tensors[au];
    const int t2 = b.tensor(tu.N, tu.H, tu.W, 256 + 48);     // torch.cat([aspp, high_res]) exists only as the depthwise conv's output
    b.dw(au, t2, 0, wp2, 0, 1);
    b.dw(hm, t2, 256, wp2, 256, 1);
    x = b.conv("decoder.block2.0.1", {{mat(t2), 0}}, 256, 1, 1, 0, "decoder.block2.1", false);
  } else {
    return fail(OCTSEG_UNSUPPORTED_ARCH, "unknown arch '" + P->arch + "' (unet | unetplusplus | linknet | fpn | deeplabv3plus | deeplabv3 | pspnet | manet | pan)");
  }
  b.conv("segmentation_head.0", {{x, 0}}, P->classes, head_k, 1, head_k / 2, "", true, false, true);
  if (P->head_up > 1) { Op op; op.kind = OP_UPLOGITS; P->ops.push_back(op); }

  if (!regnet && !effnet && P->arch != "manet" && P->arch != "pan" && P->arch != "fpn" && P->arch != "deeplabv3plus" && P->arch != "pspnet" && P->arch != "deeplabv3") assign_lanes(P);

  // ---------------- workspace layout ----------------
  P->dlogits_C = 16;
  const size_t esz = dtype_size(P->dtype);
  size_t off = 0;
  P->act_begin = off;
  for (auto& t : P->tensors) { t.off = off; off += align_up((size_t)t.N * t.H * t.W * t.C * esz); }
  P->act_end = off;
  P->grad_begin = off;
  for (auto& t : P->tensors)
    if (t.need_grad && t.grad_alias < 0) { t.goff = off; off += align_up((size_t)t.N * t.H * t.W * t.C * esz); }
  for (auto& t : P->tensors)
    if (t.need_grad && t.grad_alias >= 0) t.goff = P->tensors[t.grad_alias].goff;
  P->grad_end = off;
  for (auto& op : P->ops)
    if (op.kind == OP_BN_ACT && op.relu && op.post < 0) {
      TensorInfo& t = P->tensors[op.out];
      const size_t nvec = (size_t)t.N * t.H * t.W * t.C * esz / 16;
      t.mask_off = off; off += align_up(nvec);
    }
  for (auto& g : P->gns) {
    const TensorInfo& t = P->tensors[g.y];
    const size_t S = (size_t)gn_num_slabs((size_t)t.H * t.W);
    g.part_off = off; off += align_up((size_t)t.N * S * g.C * 2 * sizeof(float));
    g.ss_off = off; off += align_up((size_t)t.N * g.C * 2 * sizeof(float));
    g.stat_off = off; off += align_up((size_t)t.N * g.G * 2 * sizeof(float));
    g.coef_off = off; off += align_up((size_t)t.N * g.G * 2 * sizeof(float));
  }
  if (P->head_up > 1) {
    const size_t h4 = P->H / P->head_up, w4 = P->W / P->head_up;
    P->z4_off = off; off += align_up((size_t)P->B * P->classes * h4 * w4 * sizeof(float));
    P->dz4_off = off; off += align_up((size_t)P->B * h4 * w4 * 16 * esz);
  }
  for (auto& bn : P->bns) { bn.ss_off = off; off += align_up((size_t)bn.C * 6 * sizeof(float)); }
  size_t slab = 0, tmp = 0, tie_scratch = 0;
  for (auto& L : P->convs) {
    Geom g{L.R, L.S, L.stride, L.pad, L.transposed, L.N, L.IH, L.IW, L.Cin, L.OH, L.OW, L.Cout};
    if (L.stem) { g.R = g.S = 1; g.pad = 0; }
    const int wtaps = g.R * g.S;
    std::vector<ConvArgs> la;
    fwd_launches(g, la);
    L.pk_fwd = conv_pack_info(la[0], P->dtype);
    L.wimg_fwd_off = off; off += align_up(conv_image_bytes(L.pk_fwd, wtaps));
    L.has_dgrad = false;
    for (auto& s : L.srcs) L.has_dgrad = L.has_dgrad || P->tensors[s.v.t].need_grad;
    if (L.has_dgrad) {
      std::vector<ConvArgs> ld;
      dgrad_launches(g, ld);
      ConvArgs d0 = ld[0];
      for (auto& d : ld) if (d.ntaps > 0) { d0 = d; break; }
      d0.Cin = L.head ? P->dlogits_C : L.Cout;
      L.pk_dgrad = conv_pack_info(d0, P->dtype);
      L.wimg_dgrad_off = off; off += align_up(conv_image_bytes(L.pk_dgrad, wtaps));
    }
    L.tie = 0;
    if (tie_mask() != 0 && !L.srcs.empty()) {
      TieQuery q{};
      q.esz = (int)esz; q.transposed = L.transposed; q.stem = L.stem; q.head = L.head; q.sliced = L.sliced; q.accum_out = L.accum_out;
      q.has_bn = L.bn >= 0; q.has_bias = L.b >= 0; q.R = L.R; q.S = L.S; q.stride = L.stride; q.pad = L.pad; q.nsrc = (int)L.srcs.size();
      q.up0_whole_grad = L.srcs[0].up && L.srcs[0].cn == 0 && P->tensors[L.srcs[0].v.t].need_grad;
      q.skips_plain_grad = true;
      for (size_t i = 1; i < L.srcs.size(); ++i)
        q.skips_plain_grad = q.skips_plain_grad && !L.srcs[i].up && L.srcs[i].cn == 0 && P->tensors[L.srcs[i].v.t].need_grad;
      q.Ca = P->tensors[L.srcs[0].v.t].C; q.Cs = L.Cin - q.Ca; q.Cout = L.Cout;
      if (tie_eligible(q)) {
        const int Ca = q.Ca, Cs = q.Cs;
        L.tie = tie_mask(); L.tie_Ca = Ca; L.tie_Cs = Cs;
        const TieImages im = tie_images(P->dtype, tie_geom_up(L), tie_geom_skip(L));
        L.tie_pk_fu = im.pk_fu; L.tie_pk_du = im.pk_du; L.tie_du_masked = im.du_masked;
        L.tie_fu_off = off; off += align_up(conv_image_bytes(L.tie_pk_fu, 16));
        L.tie_du_off = off; off += align_up(conv_image_bytes(L.tie_pk_du, im.du_taps()));
        if (Cs > 0) {
          L.tie_pk_fs = im.pk_fs; L.tie_pk_ds = im.pk_ds;
          L.tie_fs_off = off; off += align_up(conv_image_bytes(L.tie_pk_fs, 9));
          L.tie_ds_off = off; off += align_up(conv_image_bytes(L.tie_pk_ds, 9));
        }
        tie_scratch = std::max(tie_scratch, ((size_t)16 * Ca + (size_t)9 * Cs) * L.Cout * sizeof(float));
      }
    }
    if ((L.tie & 1) && L.bn >= 0) {
      P->bns[L.bn].rows = 512;   // the launches accumulate into the output: its statistics come from a sweep over the finished tensor
      slab = std::max(slab, (size_t)512 * L.Cout * 2 * sizeof(float));
    } else if (L.bn >= 0 && L.stem && (P->stem_k == 7 && thin_stem_eligible(P->dtype))) {
      P->bns[L.bn].rows = thin_stem_rows(L.N, P->H, P->W);   // the stem runs in thin.hip straight from the frame: one slab row per workgroup
      slab = std::max(slab, (size_t)P->bns[L.bn].rows * L.Cout * 2 * sizeof(float));
    } else if (L.bn >= 0) {
      int rows = 0;
      for (auto& a : la) {
        // geometry-only descriptors, so that the tile count equals what run_forward will launch
        // (everything the kernel choice looks at: launch_conv routes stride-1 single-source 1x1 layers to gemm1x1.hip, whose
        //  slab has one row per workgroup; run_forward checks that it lands on the same row count)
        a.nsrc = 0;
        int c0 = 0;
        for (auto& s : L.srcs) {
          SrcDesc d{}; d.H = P->tensors[s.v.t].H; d.W = P->tensors[s.v.t].W; d.up = s.up; d.C = P->tensors[s.v.t].C; d.c0 = c0;
          c0 += s.cn ? s.cn : d.C; a.src[a.nsrc++] = d;
        }
        DstDesc dd{}; dd.H = L.OH; dd.W = L.OW; dd.C = L.Cout; dd.cn = L.Cout; a.dst[0] = dd; a.ndst = 1;
        a.bias = L.b >= 0 ? (const float*)(uintptr_t)16 : nullptr;   // presence only
        a.stat_slab = (float*)(uintptr_t)16;                          // (the rows are those of a TRAINING forward)
        a.Wmaster = (const float*)(uintptr_t)16; a.wO = L.Cout; a.wI = L.Cin; a.wtrans = 0;
        a.out_mode = L.head ? OUT_HEAD_NCHW : OUT_STORE;
        rows += conv_num_mtiles_flat(a, P->dtype);
      }
      P->bns[L.bn].rows = rows;
      slab = std::max(slab, (size_t)rows * L.Cout * 2 * sizeof(float));
    }
    for (auto& s : L.srcs)
      if (s.up) tmp = std::max(tmp, (size_t)L.N * L.IH * L.IW * P->tensors[s.v.t].C * esz);
  }
  for (auto& bn : P->bns)   // a BatchNorm behind a grouped conv: no conv epilogue feeds it, OP_STATS writes `rows` partial sums of the whole tensor
    if (bn.rows == 0) bn.rows = 512;
  // one-launch weight packing: job table + prefix sums (uploaded into the workspace on first use)
  P->pack_jobs.clear(); P->pack_prefix.clear(); P->pack_total = 0;
  for (auto& L : P->convs) {
    const int taps = L.stem ? 1 : L.R * L.S;
    for (int tr = 0; tr < 2; ++tr) {
      if (tr == 1 && !L.has_dgrad) continue;
      const ConvPackInfo& pk = tr ? L.pk_dgrad : L.pk_fwd;
      PackJob j{P->params[L.w].off, tr ? L.wimg_dgrad_off : L.wimg_fwd_off, taps, L.Cout, L.Cin, tr, pk.BN, pk.RB, pk.nchunks, pk.ntiles,
                (!tr && L.bn >= 0) ? P->bns[L.bn].ss_off : (!tr && L.fold_bn >= 0) ? P->bns[L.fold_bn].ss_off + (size_t)L.out_c0 * sizeof(float) : ~(size_t)0};
      P->pack_prefix.push_back(P->pack_total);
      P->pack_jobs.push_back(j);
      P->pack_total += (unsigned long long)taps * pk.nchunks * pk.ntiles * pk.BN * (pk.RB / 16);
    }
    if (L.tie)
      tie_pack_jobs(TieImages{L.tie_pk_fu, L.tie_pk_du, L.tie_pk_fs, L.tie_pk_ds, L.tie_du_masked},
                    TieOffsets{L.tie_fu_off, L.tie_du_off, L.tie_fs_off, L.tie_ds_off}, P->params[L.w].off, L.Cout, L.Cin, L.tie_Ca, L.tie_Cs,
                    P->pack_jobs, P->pack_prefix, P->pack_total);
  }
  P->bn_jobs.clear(); P->bn_prefix.clear(); P->bn_total = 0;
  for (auto& b : P->bns) {
    P->bn_prefix.push_back(P->bn_total);
    P->bn_jobs.push_back(BnEvalJob{P->params[b.gamma].off, P->params[b.beta].off, b.rm_off, b.rv_off, b.ss_off, b.C, ~(size_t)0, b.eps});
    P->bn_total += (unsigned)b.C;
  }
  for (auto& L : P->convs)   // a biased conv in front of a BatchNorm (LinkNet's ConvTranspose2d): its bias folds into the eval shift
    if (L.bn >= 0 && L.b >= 0) P->bn_jobs[L.bn].bias_off = P->params[L.b].off;
  P->bn_tab_off = off; off += align_up(P->bn_jobs.size() * sizeof(BnEvalJob));
  P->bn_prefix_off = off; off += align_up(P->bn_prefix.size() * sizeof(unsigned));
  P->pack_tab_off = off; off += align_up(P->pack_jobs.size() * sizeof(PackJob));
  P->pack_prefix_off = off; off += align_up(P->pack_prefix.size() * sizeof(unsigned long long));
  // the BN backward reduce uses up to 1024 slab rows
  for (auto& bn : P->bns) slab = std::max(slab, (size_t)1024 * bn.C * 2 * sizeof(float));
  P->slab_off = off; P->slab_bytes = align_up(slab); off += 2 * align_up(slab);          // one slab per forward lane
  P->fin_part_off = off; off += 2 * align_up((size_t)SLAB_PART_CAP * 2 * sizeof(double));   // two-level slab reduction scratch (per lane)
  P->fin_cnt_off = off; off += align_up(2 * 64 * sizeof(unsigned));
  {
    size_t pool_elems = 0;
    for (auto& op : P->ops)
      if (op.kind == OP_MAXPOOL) { const TensorInfo& t = P->tensors[op.out]; pool_elems = std::max(pool_elems, (size_t)t.N * t.H * t.W * t.C); }
    P->pool_idx_off = off; off += align_up(pool_elems);   // one buffer: the ResNet stems have exactly one max-pool
  }
  P->tmp_off = off; P->tmp_bytes = tmp; off += align_up(tmp);
  P->tie_scratch_off = off; off += align_up(tie_scratch);
  for (int k = 0; k < 3; ++k) {
    P->exec_macs[k] = P->fwd_macs;
    for (auto& L : P->convs)   // a tied pass runs 16 of the 36 multiply-accumulates per low-resolution pixel over the upsampled source's channels
      if (L.tie & (1 << k)) P->exec_macs[k] -= layer_macs(L) * L.tie_Ca / L.Cin * (5.0 / 9.0);
  }
  {
    size_t se_part = 0;
    for (auto& op : P->ops)
      if (op.kind == OP_SEGATE) { const TensorInfo& t = P->tensors[op.in]; se_part = std::max(se_part, (size_t)t.N * se_dgate_shares(t.H * t.W) * t.C * sizeof(float)); }
    P->se_part_off = off; off += align_up(se_part);
    for (auto& op : P->ops)
      if (op.kind == OP_SEFC) { const TensorInfo& t = P->tensors[op.in]; op.aux_off = off; off += align_up((size_t)2 * t.N * op.up * sizeof(float)); }
      else if (op.kind == OP_FPA) {
        const TensorInfo& t = P->tensors[op.in];
        P->fpa.scratch_off = off; off += align_up(fpa_pyr_scratch_floats(t.N, t.H, t.W) * sizeof(float));
        P->fpa.gscratch_off = off; off += align_up((fpa_pyr_gscratch_floats(t.N, t.H, t.W) + (size_t)t.N * t.H * t.W) * sizeof(float));   // + d uu
      }
      else if (op.kind == OP_PAB) {
        const TensorInfo& t = P->tensors[op.in];
        const size_t hw = (size_t)t.H * t.W;
        op.aux_off = off; off += align_up((size_t)t.N * hw * hw * sizeof(float)) * 2 + align_up((size_t)t.N * hw * t.C * sizeof(float));
      }
  }
  P->dlogits_off = off; off += align_up((size_t)P->B * P->H * P->W * P->dlogits_C * esz);
  P->dice_off = off; off += align_up((size_t)(1 + P->B) * P->classes * DICE_NS * sizeof(double));   // totals + per-image replicas
  P->ws_bytes = off;
  return OCTSEG_OK;
}

}  // namespace detail
}  // namespace octseg
