// plan_backward.cpp -- the backward executor: BatchNorm backward, the data / weight gradients of one conv layer (tied layers included,
// weight gradients on the side stream), the gradient-arena slices of the data-parallel backward, and run_backward over the op list.
#include "plan_internal.h"

namespace octseg {
namespace detail {

// Split-K width of the multi-tap weight gradients when they run on the side stream beside the chain's kernels.  A weight gradient that fills
// all 256 CUs with one long-running workgroup each (110-150 KB of LDS, 380 registers) leaves the data gradient and the BatchNorm sweeps of the
// chain nothing to start on until its workgroups retire; on 144-160 CUs it takes 30 % longer by itself (24.5 against 18.9 ms per step at 160, alone)
// and the step gets shorter: 65.1 -> 63.0 ms at 144 workgroups (ABAB on one box; 112: 67.8, 128: 63.5, 136: 63.0, 152: 63.3, 160: 63.4-63.7, 176: 63.7).  On the caller's own stream (one-stream
// mode, the kernels-alone pass of bench.py) nothing runs beside it and it keeps the full width (wg_target = 0).
int side_wgs() { return 144; }

// BN backward of BN `bn` over raw tensor y: g -> dy (written to grad(y))
static int bn_backward(Exec& E, int bn, const void* g, int mask, const void* out_mask, void* res_grad = nullptr, int res_store = 0,
                       const unsigned char* maskbits = nullptr) {
  octseg_plan* P = E.P;
  const BNInfo& b = P->bns[bn];
  const TensorInfo& t = P->tensors[b.y];
  BnBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.g = g; a.y = E.act(b.y); a.out = out_mask; a.maskbits = maskbits;
  a.scale = E.bn_scale(bn); a.shift = E.bn_shift(bn); a.mean = E.bn_mean(bn); a.rstd = E.bn_rstd(bn);
  a.gamma = E.params + P->params[b.gamma].off;
  a.npix = (size_t)t.N * t.H * t.W; a.C = b.C; a.mask = mask;
  a.slab = (float*)(E.ws + P->slab_off);
  a.part = (double*)(E.ws + P->fin_part_off); a.counters = (unsigned*)(E.ws + P->fin_cnt_off);
  const int VEC = ev_vec(P->dtype);
  const int vpc = b.C / VEC;
  const int tpv = vpc >= 256 ? 1 : 256 / vpc;
  size_t rows = (a.npix + tpv - 1) / tpv;
  // slab rows = workgroups of the reduce pass (<= 1024: the slab's size).  Measured on U-Net++/resnet101: 256 rows everywhere +1.7 % at
  // --batch 2, +-0 at 4, -2 % at 16; 64 rows -9 % at 2; a size rule (256 rows up to 4 M elements) moved nothing: 1024 stays.
  if (rows > 1024) rows = 1024;
  a.rows = (int)rows;
  if (E.grads) {
    a.dgamma = E.grads + P->params[b.gamma].off;
    a.dbeta = E.grads + P->params[b.beta].off;
  }
  a.coef = E.bn_coef(bn);
  a.dy = E.grad(b.y);
  a.res_grad = res_grad; a.res_store = res_store;
  E.ginit[b.y] = 1;   // written (stored) by the apply pass below
  const double tbytes = (double)a.npix * b.C * dtype_size(P->dtype);   // class 3 = HBM-bound sweeps: "flops" carries algorithmic bytes
  if (P->frozen_bn) {
    // running statistics: no batch term in the gradient.  The forward's finalize left coef = 0 (launch_bn_finalize_frozen), so the apply sweep
    // alone computes dy = gamma * rstd * mask * g -- small tensors included; no dgamma / dbeta
  } else if (a.npix <= (size_t)BN_SMALL_COUNT) {   // small tensors: reduce, finalize and apply in one launch, in double (elementwise.hip)
    ProfScope ps(3, tbytes * ((mask == 2 && !maskbits) ? 5 : 4), E.st, b.name + ".bwd_small");
    HIPCHK(launch_bn_bwd_small(P->dtype, a, E.st));
    return OCTSEG_OK;
  } else {
    {
      ProfScope ps(3, tbytes * ((mask == 2 && !maskbits) ? 3 : 2), E.st, b.name + ".bwd_reduce");
      HIPCHK(launch_bn_bwd_reduce(P->dtype, a, E.st));
    }
    HIPCHK(launch_bn_bwd_finalize(a, E.st));
  }
  {
    ProfScope ps(3, tbytes * (((mask == 2 && !maskbits) ? 4 : 3) + (res_grad ? (res_store ? 1 : 2) : 0)), E.st, b.name + ".bwd_apply");
    HIPCHK(launch_bn_bwd_apply(P->dtype, a, E.st));
  }
  return OCTSEG_OK;
}

static int conv_backward(Exec& E, const ConvLayer& L, const void* dy, int dyC) {
  octseg_plan* P = E.P;
  const size_t esz = dtype_size(P->dtype);
  const Geom g = E.geom(L);
  if (E.data_only && L.stem) return OCTSEG_OK;   // the frame needs no gradient
  if (L.stem && (P->stem_k == 7 && thin_stem_eligible(P->dtype))) {
    // the forward built no im2col tensor.  Weight gradient straight from the frame (thin.hip); the deterministic-reduction mode keeps the
    // atomics-free kernel and rebuilds the im2col rows for it here.  The frame needs no gradient.
    if (P->stem_image == nullptr) return fail(OCTSEG_BAD_ARG, "backward without a training forward of this plan (stem frame unknown)");
    hipStream_t ws_ = E.wst ? E.wst : E.st;
    if (ws_ != E.st) {
      HIPCHK(hipEventRecord(P->ev_fork, E.st));
      HIPCHK(hipStreamWaitEvent(ws_, P->ev_fork, 0));
    }
    if (P->dtype == DT_BF16 && !deterministic_mode()) {
      StemArgs sa;
      memset(&sa, 0, sizeof(sa));
      sa.img = P->stem_image; sa.N = P->B; sa.H = P->H; sa.W = P->W; sa.normalize = P->stem_normalize;
      for (int i = 0; i < 3; ++i) { sa.mean[i] = P->stem_mean[i]; sa.stdv[i] = P->stem_std[i]; }
      sa.dy = dy; sa.dW = E.grads + P->params[L.w].off;
      ProfScope ps(2, 2.0 * layer_macs(L), ws_, L.name);
      HIPCHK(launch_thin_stem_wgrad(P->dtype, sa, ws_));
      return OCTSEG_OK;
    }
    const TensorInfo& tc = P->tensors[P->col_tensor];
    HIPCHK(launch_stem_im2col(P->dtype, P->stem_image, E.act(P->col_tensor), P->B, P->H, P->W, tc.C, P->stem_mean, P->stem_std,
                              P->stem_normalize, ws_));
  }
  // The weight gradient depends on dy and on saved activations only: forked in front of the layer's data gradient.  Forked behind it, so
  // that it would start together with the BatchNorm sweeps of the layer below (HBM-bound; at <= 128 registers they fit beside its
  // one-wave-per-SIMD workgroups), measured 70.2 against 68.5 ms per step (round 4, ABAB on one box; round 2: 78.8 against 78.4): the side
  // stream then idles through every data gradient's first half and the step's tail grows.
  auto wgrad_part = [&]() -> int {
    // weight gradient (+ bias gradient) on the side stream: fork after everything that produced dy
    hipStream_t ws_ = E.wst ? E.wst : E.st;
    if (ws_ != E.st) {
      HIPCHK(hipEventRecord(P->ev_fork, E.st));
      HIPCHK(hipStreamWaitEvent(ws_, P->ev_fork, 0));
    }
    // bias gradient
    if (L.b >= 0)
      HIPCHK(launch_channel_sum(P->dtype, dy, (size_t)L.N * L.OH * L.OW, dyC, L.Cout, E.grads + P->params[L.b].off, ws_));
    if (L.tie & 4) {
      // tied: gradient of the 4x4 image (low-resolution source x dy's parity planes) and of the skip slice's 3x3 into scratch, folded into the
      // 3x3 gradient by one sweep (the side stream runs the layers one after the other: one scratch serves them all)
      SrcDesc src[MAX_SRC];
      const int ns = E.fill_srcs(L, src);
      const int Ca = L.tie_Ca, Cs = L.tie_Cs;
      float* dK4 = (float*)(E.ws + P->tie_scratch_off);
      float* dW3s = dK4 + (size_t)16 * L.Cout * Ca;
      HIPCHK(hipMemsetAsync(dK4, 0, ((size_t)16 * Ca + (size_t)9 * Cs) * L.Cout * sizeof(float), ws_));
      const double macs = layer_macs(L);
      std::vector<WgradArgs> lw;
      wgrad_launches(tie_geom_up(L), lw);
      for (auto& a : lw) {
        a.nsrc = 1; a.src[0] = src[0]; a.src[0].up = 0; a.src[0].c0 = 0;
        a.dy = dy; a.dyC = dyC; a.dW = dK4; a.stamp = nullptr;
        a.wg_target = ws_ != E.st ? side_wgs() : 0;
      }
      if (wgrad_convt16_eligible(lw[0], P->dtype)) {   // all four parities from one staged window (wgrad_convt.hip)
        ProfScope ps(2, 2.0 * macs * Ca / L.Cin, ws_, L.name);
        HIPCHK(launch_wgrad_convt16(P->dtype, lw[0], ws_));
      } else {
        for (auto& a : lw) {
          ProfScope ps(2, 2.0 * macs * Ca / L.Cin / 4.0, ws_, L.name);
          HIPCHK(launch_wgrad(P->dtype, a, ws_));
        }
      }
      if (Cs > 0) {
        lw.clear();
        wgrad_launches(tie_geom_skip(L), lw);
        WgradArgs& a = lw[0];
        a.nsrc = ns - 1;
        for (int i = 1; i < ns; ++i) { a.src[i - 1] = src[i]; a.src[i - 1].c0 -= Ca; }
        a.dy = dy; a.dyC = dyC; a.dW = dW3s; a.stamp = nullptr;
        a.wg_target = ws_ != E.st ? side_wgs() : 0;
        ProfScope ps(2, 2.0 * macs * Cs / L.Cin, ws_, L.name);
        HIPCHK(launch_wgrad(P->dtype, a, ws_));
      }
      HIPCHK(launch_tied_fold(dK4, Cs > 0 ? dW3s : nullptr, E.grads + P->params[L.w].off, L.Cout, Ca, Cs, ws_));
    } else {
      std::vector<WgradArgs> lw;
      wgrad_launches(g, lw);
      for (auto& a : lw) {
        a.nsrc = E.fill_srcs(L, a.src);
        a.dy = dy; a.dyC = dyC;
        a.dW = E.grads + P->params[L.w].off;
        a.stamp = nullptr;
        a.wg_target = ws_ != E.st ? side_wgs() : 0;
      }
      if (L.transposed && lw.size() == 4 && wgrad_convt16_eligible(lw[0], P->dtype)) {   // ConvTranspose2d: the four parities in one launch
        ProfScope ps(2, 2.0 * layer_macs(L), ws_, L.name);
        HIPCHK(launch_wgrad_convt16(P->dtype, lw[0], ws_));
        lw.clear();
      }
      const double nl = (double)lw.size();
      for (auto& a : lw) {
        ProfScope ps(2, 2.0 * layer_macs(L) / nl, ws_, L.name);
        HIPCHK(launch_wgrad(P->dtype, a, ws_));
      }
    }
    return OCTSEG_OK;
  };
  auto dgrad_part = [&]() -> int {
    // data gradient
    bool any = false;
    for (auto& s : L.srcs) any = any || P->tensors[s.v.t].need_grad;
    if (!any) return OCTSEG_OK;
    if (L.tie & 2) {
      // tied: the low-resolution source's gradient from the four parity planes of dy (2x2 taps each, all of them cover the whole map: the first
      // stores unless somebody wrote before, the others add); the skip sources' from a 3x3 data gradient over their own channels
      const int ti0 = L.srcs[0].v.t;
      const TensorInfo& t0 = P->tensors[ti0];
      const double macs = layer_macs(L);
      std::vector<ConvArgs> lu;
      if (L.tie_du_masked) { lu.resize(1); tied_dgrad_masked(tie_geom_up(L), lu[0]); }
      else dgrad_launches(tie_geom_up(L), lu);   // (one launch: 16 taps at stride 2 over dy)
      const int acc0 = E.claim(ti0);
      for (int k = 0; k < (int)lu.size(); ++k) {
        ConvArgs& a = lu[k];
        if (L.tie_du_masked) {
          for (int p = 0; p < 4; ++p) {   // plane p of dy as a tensor of its own: first pixel (p >> 1, p & 1), doubled pixel and row strides
            SrcDesc& s = a.src[p];
            s.ptr = (const char*)dy + ((size_t)(p >> 1) * L.OW + (p & 1)) * dyC * esz;
            s.scale = nullptr; s.shift = nullptr; s.C = 2 * dyC; s.c0 = p * L.Cout; s.H = L.OH / 2; s.W = L.OW; s.up = 0; s.relu = 0;
          }
        } else {
          SrcDesc s;
          s.ptr = dy; s.scale = nullptr; s.shift = nullptr; s.C = dyC; s.c0 = 0; s.H = L.OH; s.W = L.OW; s.up = 0; s.relu = 0;
          a.src[0] = s; a.nsrc = 1;
          a.Cin = L.Cout;
        }
        a.W = E.ws + L.tie_du_off;
        DstDesc d;
        d.ptr = E.grad(ti0); d.C = t0.C; d.c0 = 0; d.cn = L.tie_Ca; d.H = t0.H; d.W = t0.W; d.accum = k == 0 ? acc0 : 1; d.pool = 0;
        a.dst[0] = d; a.ndst = 1; a.out_mode = OUT_STORE; a.bias = nullptr; a.stat_slab = nullptr;
        ProfScope ps(1, 2.0 * macs * L.tie_Ca / L.Cin / (double)lu.size(), E.st, L.name);
        HIPCHK(launch_conv(P->dtype, a, E.st));
      }
      if (L.tie_Cs > 0) {
        std::vector<ConvArgs> ls;
        dgrad_launches(tie_geom_skip(L), ls);
        ConvArgs& a = ls[0];
        SrcDesc s;
        s.ptr = dy; s.scale = nullptr; s.shift = nullptr; s.C = dyC; s.c0 = 0; s.H = L.OH; s.W = L.OW; s.up = 0; s.relu = 0;
        a.src[0] = s; a.nsrc = 1;
        a.Cin = L.Cout;
        a.W = E.ws + L.tie_ds_off;
        int nd = 0, c0 = 0;
        for (size_t i = 1; i < L.srcs.size(); ++i) {
          const int ti = L.srcs[i].v.t;
          const TensorInfo& t = P->tensors[ti];
          DstDesc d;
          d.ptr = E.grad(ti); d.C = t.C; d.c0 = c0; d.cn = t.C; d.H = L.IH; d.W = L.IW; d.accum = E.claim(ti); d.pool = 0;
          a.dst[nd++] = d;
          c0 += t.C;
        }
        a.ndst = nd; a.out_mode = OUT_STORE; a.bias = nullptr; a.stat_slab = nullptr;
        ProfScope ps(1, 2.0 * macs * L.tie_Cs / L.Cin, E.st, L.name);
        HIPCHK(launch_conv(P->dtype, a, E.st));
      }
      return OCTSEG_OK;
    }
    std::vector<ConvArgs> ld;
    dgrad_launches(g, ld);
    // destinations: the forward sources' gradient buffers; upsampled sources go through a temp.  A destination
    // that nobody has written yet in this backward is stored to (no memset + read-modify-write), unless this
    // conv does not cover it completely (1x1 stride 2: only one pixel parity) -- then it is zeroed first.
    bool full_cover = true;
    for (auto& a : ld) if (a.ntaps == 0) full_cover = false;
    DstDesc dst[MAX_SRC];
    int nd = 0, c0 = 0;
    int up_src = -1;
    for (size_t i = 0; i < L.srcs.size(); ++i) {
      const int ti = L.srcs[i].v.t;
      const TensorInfo& t = P->tensors[ti];
      const int scn = L.srcs[i].cn ? L.srcs[i].cn : t.C;      // channels of this source inside the layer's input (a slice for grouped convs)
      const size_t soff = (size_t)L.srcs[i].c0 * esz;
      DstDesc d;
      d.C = t.C; d.c0 = c0; d.cn = scn; d.H = L.IH; d.W = L.IW; d.accum = 0; d.pool = 0;
      if (L.srcs[i].up && t.need_grad && ld.size() == 1 && ld[0].ostride == 1 && (L.IH % 2) == 0 && (L.IW % 2) == 0) {
        // gradient of the nearest-x2 upsample: the dgrad epilogue sums the 2x2 quads straight into the source's gradient
        d.ptr = E.grad(ti); d.H = t.H; d.W = t.W; d.pool = 1;
        d.accum = E.claim(ti);
      } else if (L.srcs[i].up) {
        d.ptr = E.ws + P->tmp_off;     // fully covered by this dgrad, pooled into the source afterwards
        up_src = (int)i;
      } else if (!t.need_grad) {
        d.ptr = E.ws + P->tmp_off; d.accum = 0;   // never happens for multi-source convs; keeps the descriptor valid
      } else if (L.srcs[i].cn) {
        // one group of a grouped conv: it owns a channel slice of the source's gradient.  The first group to arrive zeroes the whole
        // tensor, every group then accumulates into its slice (first-writer stores are per tensor, not per slice)
        if (!E.ginit[ti]) { HIPCHK(hipMemsetAsync(E.grad(ti), 0, (size_t)t.N * t.H * t.W * t.C * esz, E.st)); E.ginit[ti] = 1; }
        d.ptr = (char*)E.grad(ti) + soff;
        d.accum = 1;
      } else {
        d.ptr = E.grad(ti);
        d.accum = E.claim(ti);
        if (!d.accum && !full_cover) {
          HIPCHK(hipMemsetAsync(d.ptr, 0, (size_t)t.N * t.H * t.W * t.C * esz, E.st));
          d.accum = 1;
        }
      }
      dst[nd++] = d;
      c0 += scn;
    }
    for (auto& a : ld) {
      SrcDesc s;
      s.ptr = dy; s.scale = nullptr; s.shift = nullptr; s.C = dyC; s.c0 = 0; s.H = L.OH; s.W = L.OW; s.up = 0; s.relu = 0;
      a.src[0] = s; a.nsrc = 1;
      a.Cin = L.sliced ? L.Cout : dyC;  // contraction runs over the (padded) output channels; the pad columns of the image are zero (a group: its own channels, dyC is the stride)
      a.W = E.ws + L.wimg_dgrad_off;
      if (!L.stem && !L.transposed) { a.Wmaster = E.params + P->params[L.w].off; a.wO = L.Cout; a.wI = L.Cin; a.wtrans = 1; }
      for (int i = 0; i < nd; ++i) a.dst[i] = dst[i];
      a.ndst = nd;
      a.out_mode = OUT_STORE;   // per-destination accumulate flags decide
      a.bias = nullptr; a.stat_slab = nullptr;
      ProfScope ps(1, 2.0 * layer_macs(L) / (double)ld.size(), E.st, L.name);
      HIPCHK(launch_conv(P->dtype, a, E.st));
    }
    if (up_src >= 0) {
      const TensorInfo& t = P->tensors[L.srcs[up_src].v.t];
      const int ti = L.srcs[up_src].v.t;
      const int acc = E.claim(ti);
      HIPCHK(launch_pool2x2_accum(P->dtype, E.grad(ti), E.ws + P->tmp_off, t.N, t.H, t.W, t.C, acc ? 0 : 1, E.st));
    }
    return OCTSEG_OK;
  };
  if (!E.data_only) { const int rc = wgrad_part(); if (rc) return rc; }
  return dgrad_part();
}

// The loss kernels' arguments without the forward's outputs (octseg_dice_forward and the training step add `stats` and `loss`).
DiceArgs dice_args(const octseg_plan* P, char* ws, const float* logits, const float* target) {
  DiceArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = logits; a.target = target; a.B = P->B; a.C = P->classes; a.HW = (size_t)P->H * P->W;
  a.sums = (double*)(ws + P->dice_off); a.loss_kind = P->loss_kind;
  return a;
}

static void slice_plan(const octseg_plan* P, SliceCtx& S) {
  const int n = S.n;
  S.bounds.assign(n + 1, 0);
  S.bounds[n] = P->param_numel;
  for (int k = 1; k < n; ++k) {   // boundary k = start of the first parameter at or behind k/n of the arena
    const size_t want = P->param_numel * (size_t)k / n;
    size_t b = P->param_numel;
    for (auto& q : P->params) if (q.off >= want && q.off < b) b = q.off;
    S.bounds[k] = b;
  }
  for (int k = 1; k <= n; ++k) S.bounds[k] = std::max(S.bounds[k], S.bounds[k - 1]);
  S.last_op.assign(n, -1);
  auto touch = [&](int oi, int param) {
    if (param < 0) return;
    const size_t off = P->params[param].off;
    for (int k = 0; k < n; ++k)
      if (off >= S.bounds[k] && off < S.bounds[k + 1]) { if (S.last_op[k] < 0 || oi < S.last_op[k]) S.last_op[k] = oi; }
  };
  for (int oi = 0; oi < (int)P->ops.size(); ++oi) {   // the backward walks the ops downwards: the last writer has the SMALLEST index
    const Op& op = P->ops[oi];
    if (op.kind == OP_CONV) { touch(oi, P->convs[op.conv].w); touch(oi, P->convs[op.conv].b); }
    else if (op.kind == OP_BN_FIN) { if (P->bns[op.bn].lazy) { touch(oi, P->bns[op.bn].gamma); touch(oi, P->bns[op.bn].beta); } }
    else if (op.kind == OP_GN) { touch(oi, P->gns[op.gn].gamma); touch(oi, P->gns[op.gn].beta); }
    else if (op.kind == OP_DW || op.kind == OP_DWG) touch(oi, op.dwp);
    else if (op.kind == OP_BNX) { touch(oi, P->bns[op.y.bn].gamma); touch(oi, P->bns[op.y.bn].beta); }
    else if (op.kind == OP_SEFC) { for (int i = 0; i < 4; ++i) touch(oi, op.ins[i]); }
    else if (op.kind == OP_FPA) {
      for (int l = 0; l < 6; ++l) { touch(oi, P->fpa.w[l]); touch(oi, P->fpa.b[l]); touch(oi, P->bns[P->fpa.bn[l]].gamma); touch(oi, P->bns[P->fpa.bn[l]].beta); }
    }
    else if (op.kind == OP_BN_ACT) {
      touch(oi, P->bns[op.y.bn].gamma); touch(oi, P->bns[op.y.bn].beta);
      if (op.res.t >= 0 && op.res.bn >= 0) { touch(oi, P->bns[op.res.bn].gamma); touch(oi, P->bns[op.res.bn].beta); }
    }
  }
}

int run_backward(Exec& E, const float* logits, const float* target, float grad_scale, SliceCtx* S) {
  octseg_plan* P = E.P;
  if (S) slice_plan(P, *S);
  // slice k is complete once everything enqueued so far on the dgrad stream and on the weight-gradient stream has run:
  // the communication stream is made to wait for both, then the caller enqueues its collective there
  auto fire = [&](int k) -> int {
    if (S->bounds[k + 1] == S->bounds[k]) return OCTSEG_OK;
    if (!P->ev_slice) HIPCHK(hipEventCreateWithFlags(&P->ev_slice, hipEventDisableTiming));
    HIPCHK(hipEventRecord(P->ev_slice, E.st));
    HIPCHK(hipStreamWaitEvent(S->comm, P->ev_slice, 0));
    if (E.wst && E.wst != E.st) {
      HIPCHK(hipEventRecord(P->ev_slice, E.wst));
      HIPCHK(hipStreamWaitEvent(S->comm, P->ev_slice, 0));
    }
    S->cb(S->user, k, S->bounds[k], S->bounds[k + 1]);
    return OCTSEG_OK;
  };
  if (E.data_only) {
    if (S || !P->frozen_bn) return fail(OCTSEG_BAD_ARG, "a data-only backward needs the plan in frozen-BatchNorm mode and takes no slices");
    for (int oi = (int)P->ops.size() - 1; oi > E.stop_op; --oi) {   // every op of the walk must have a gradient that leaves the parameters alone
      const OpKind k = P->ops[oi].kind;
      if (k == OP_GN || k == OP_DW || k == OP_DWG || k == OP_BNX || k == OP_FPA || k == OP_MERGE || k == OP_DROPE || k == OP_DROP2D)
        return fail(OCTSEG_UNSUPPORTED_ARCH, "a data-only backward of this graph is not built (" + P->arch + ")");
    }
  } else {
    HIPCHK(hipMemsetAsync(E.grads, 0, P->param_numel * sizeof(float), E.st));
  }
  HIPCHK(hipMemsetAsync(E.ws + P->fin_cnt_off, 0, 2 * 64 * sizeof(unsigned), E.st));
  E.ginit.assign(P->tensors.size(), 0);
  if (!serial_mode() && !E.data_only) {
    // (a step that is being captured / replayed as one hipGraph keeps the default priority: replaying a graph whose side branch was captured
    //  from a lowest-priority stream took 34.9 instead of 20.7 ms per step at 2 frames, profiles/r4_graph_ab.txt)
    hipStream_t* wsp = P->tgraph_enabled ? &P->side : &P->side_bwd;
    if (!*wsp) HIPCHK(create_side_stream(wsp, !P->tgraph_enabled));
    if (!P->ev_fork) {
      HIPCHK(hipEventCreateWithFlags(&P->ev_fork, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&P->ev_join, hipEventDisableTiming));
    }
    E.wst = *wsp;
    // the side stream must see the zeroed parameter-gradient arena
    HIPCHK(hipEventRecord(P->ev_fork, E.st));
    HIPCHK(hipStreamWaitEvent(E.wst, P->ev_fork, 0));
  }
  // dL/dlogits (NHWC, padded channels)
  if (E.seed) {
    HIPCHK(launch_cam_seed(P->dtype, E.seed, E.ws + P->dlogits_off, P->B, P->classes, (size_t)P->H * P->W, P->dlogits_C, E.st));
  } else {
    const DiceArgs da = dice_args(P, E.ws, logits, target);
    HIPCHK(launch_dice_bwd(P->dtype, da, grad_scale, E.ws + P->dlogits_off, P->dlogits_C, E.st));
  }
  int rc;
  for (int oi = (int)P->ops.size() - 1; oi >= 0; --oi) {
    if (oi == E.stop_op) break;   // every consumer of that op's output has run: its gradient is complete
    const Op& op = P->ops[oi];
    switch (op.kind) {
      case OP_STEM_COL: break;
      case OP_CONV: {
        const ConvLayer& L = P->convs[op.conv];
        if (L.head) rc = conv_backward(E, L, E.ws + (P->head_up > 1 ? P->dz4_off : P->dlogits_off), P->dlogits_C);
        else if (L.sliced) rc = conv_backward(E, L, (char*)E.grad(L.out) + (size_t)L.out_c0 * dtype_size(P->dtype), P->tensors[L.out].C);
        else rc = conv_backward(E, L, E.grad(L.out), L.Cout);
        if (rc) return rc;
        break;
      }
      case OP_BN_FIN: {
        const BNInfo& b = P->bns[op.bn];
        if (b.lazy) {  // consumers accumulated d/d relu(bn(y)) into grad(y): turn it into dy in place
          rc = bn_backward(E, op.bn, E.grad(b.y), 1, nullptr);
          if (rc) return rc;
        }
        break;
      }
      case OP_BN_ACT: {
        const TensorInfo& t = P->tensors[op.out];
        const void* G = E.grad(op.out);
        const size_t n = (size_t)t.N * t.H * t.W * t.C;
        // main branch: with a post-add the relu mask must come from bn(y) itself
        const int mask = !op.relu ? 0 : (op.post >= 0 ? 1 : 2);
        // identity shortcut of a residual block (no BatchNorm on it, ReLU mask from the block's output): its gradient G * mask is
        // written by the main branch's apply sweep, which holds G and the mask already (was a masked_accum pass of its own)
        const bool fuse_res = mask == 2 && op.res.t >= 0 && op.res.bn < 0 && P->tensors[op.res.t].need_grad &&
                              E.grad(op.res.t) != G && E.grad(op.res.t) != E.grad(P->bns[op.y.bn].y);
        const unsigned char* mbits = (mask == 2 && t.mask_off) ? (const unsigned char*)(E.ws + t.mask_off) : nullptr;
        if (fuse_res) {
          const int acc = E.claim(op.res.t);
          rc = bn_backward(E, op.y.bn, G, mask, E.act(op.out), E.grad(op.res.t), acc ? 0 : 1, mbits);
        } else {
          rc = bn_backward(E, op.y.bn, G, mask, E.act(op.out), nullptr, 0, mbits);
        }
        if (rc) return rc;
        if (op.res.t >= 0 && !fuse_res) {
          if (op.res.bn >= 0) {
            rc = bn_backward(E, op.res.bn, G, op.relu ? 2 : 0, E.act(op.out), nullptr, 0, (op.relu && t.mask_off) ? (const unsigned char*)(E.ws + t.mask_off) : nullptr);
            if (rc) return rc;
          } else if (P->tensors[op.res.t].need_grad) {
            const int acc = E.claim(op.res.t);
            HIPCHK(launch_masked_accum(P->dtype, E.grad(op.res.t), G, op.relu ? E.act(op.out) : nullptr, n, acc ? 0 : 1, E.st));
          }
        }
        if (op.post >= 0 && P->tensors[op.post].need_grad) {
          const int acc = E.claim(op.post);
          HIPCHK(launch_masked_accum(P->dtype, E.grad(op.post), G, nullptr, n, acc ? 0 : 1, E.st));
        }
        break;
      }
      case OP_DROP2D: {
        const TensorInfo& t = P->tensors[op.out];
        HIPCHK(launch_drop_bwd(P->dtype, E.grad(op.out), P->dropout_keep, 1.0f / (1.0f - P->dropout_p), E.grad(op.in), t.N, (size_t)t.H * t.W, t.C, E.st));
        E.ginit[op.in] = 1;
        break;
      }
      case OP_RELU: {
        const TensorInfo& t = P->tensors[op.out];
        HIPCHK(launch_relu(P->dtype, E.grad(op.out), E.act(op.out), E.grad(op.in), (size_t)t.N * t.H * t.W * t.C, E.st));
        E.ginit[op.in] = 1;
        break;
      }
      case OP_RESIZE: {
        const TensorInfo& ti = P->tensors[op.in];
        const TensorInfo& to = P->tensors[op.out];
        HIPCHK(launch_bilinear_resize_adjoint(P->dtype, E.grad(op.out), E.grad(op.in), ti.N, ti.H, ti.W, to.H, to.W, ti.C, E.st));
        E.ginit[op.in] = 1;
        break;
      }
      case OP_STATS: break;
      case OP_DWG: {
        const TensorInfo& ti = P->tensors[op.in];
        const TensorInfo& to = P->tensors[op.out];
        DwgArgs a;
        memset(&a, 0, sizeof(a));
        a.in = E.act(op.in); a.out = E.grad(op.out); a.w = E.params + P->params[op.dwp].off; a.dw = E.grads + P->params[op.dwp].off;
        a.N = ti.N; a.H = ti.H; a.W = ti.W; a.C = ti.C; a.OH = to.H; a.OW = to.W; a.K = op.wc0; a.stride = op.up; a.pad = op.oc0;
        HIPCHK(launch_dwg_bwd_w(P->dtype, a, E.st));
        if (ti.need_grad) {
          a.gin = E.grad(op.in); a.accum = E.claim(op.in);
          HIPCHK(launch_dwg_bwd_data(P->dtype, a, E.st));
        }
        break;
      }
      case OP_BNX: {        // gradient wrt bn(y) into grad(y) (act', drop_connect factor), the ordinary BatchNorm backward on it in place; post: + g
        const TensorInfo& t = P->tensors[op.out];
        BnxArgs a;
        memset(&a, 0, sizeof(a));
        a.y = E.act(op.y.t); a.scale = E.bn_scale(op.y.bn); a.shift = E.bn_shift(op.y.bn);
        a.dscale = op.oc0 >= 0 ? P->drop_connect + (size_t)op.oc0 * t.N : nullptr;
        a.post = E.grad(op.out); a.out = E.grad(op.y.t);
        a.npix = (size_t)t.N * t.H * t.W; a.hw = t.H * t.W; a.C = t.C; a.act = op.up;
        HIPCHK(launch_bnx_bwd(P->dtype, a, E.st));
        rc = bn_backward(E, op.y.bn, E.grad(op.y.t), 0, nullptr);
        if (rc) return rc;
        if (op.post >= 0 && P->tensors[op.post].need_grad) {
          const int acc = E.claim(op.post);
          HIPCHK(launch_masked_accum(P->dtype, E.grad(op.post), E.grad(op.out), nullptr, (size_t)t.N * t.H * t.W * t.C, acc ? 0 : 1, E.st));
        }
        break;
      }
      case OP_SEFC: {
        const TensorInfo& t = P->tensors[op.in];
        SefcArgs a;
        memset(&a, 0, sizeof(a));
        a.m = E.act(op.in); a.ds = E.grad(op.out); a.dm = E.grad(op.in);
        a.w1 = E.params + P->params[op.ins[0]].off; a.w2 = E.params + P->params[op.ins[2]].off;
        if (E.grads) {   // (a data-only backward leaves them null: launch_sefc_bwd then skips its weight-gradient launch)
          a.dw1 = E.grads + P->params[op.ins[0]].off; a.db1 = E.grads + P->params[op.ins[1]].off;
          a.dw2 = E.grads + P->params[op.ins[2]].off; a.db2 = E.grads + P->params[op.ins[3]].off;
        }
        a.h = (float*)(E.ws + op.aux_off); a.dh = a.h + (size_t)t.N * op.up;
        a.N = t.N; a.C = t.C; a.R = op.up; a.act = op.oc0;
        HIPCHK(launch_sefc_bwd(P->dtype, a, E.st));
        E.ginit[op.in] = 1;
        break;
      }
      case OP_SEGATE: {     // d x (+)= g * sigmoid(s);  d s = sigmoid'(s) * sum_p g * x
        const TensorInfo& t = P->tensors[op.in];
        const bool two = op.ins[1] >= 0;
        HIPCHK(launch_se_dgate(P->dtype, E.grad(op.out), E.act(op.in), E.act(op.ins[0]), E.grad(op.ins[0]), (float*)(E.ws + P->se_part_off), t.N, t.H * t.W,
                               t.C, E.st, two ? E.act(op.ins[1]) : nullptr, two ? E.grad(op.ins[1]) : nullptr));
        E.ginit[op.ins[0]] = 1;
        if (two) E.ginit[op.ins[1]] = 1;
        const int acc = E.claim(op.in);
        HIPCHK(launch_se_gate(P->dtype, E.grad(op.out), E.act(op.ins[0]), E.grad(op.in), t.N, t.H * t.W, t.C, acc, E.st, two ? E.act(op.ins[1]) : nullptr));
        break;
      }
      case OP_ADD: {
        const TensorInfo& t = P->tensors[op.out];
        const size_t n = (size_t)t.N * t.H * t.W * t.C;
        for (int src : {op.in, op.ins[0]})
          if (P->tensors[src].need_grad) {
            const int acc = E.claim(src);
            HIPCHK(launch_masked_accum(P->dtype, E.grad(src), E.grad(op.out), nullptr, n, acc ? 0 : 1, E.st));
          }
        break;
      }
      case OP_FPA: {
        const TensorInfo& t = P->tensors[op.in];
        const int n1 = t.N * (t.H / 2) * (t.W / 2);
        float* scr = (float*)(E.ws + P->fpa.scratch_off);
        float* gs = (float*)(E.ws + P->fpa.gscratch_off);
        float* duu = gs + fpa_pyr_gscratch_floats(t.N, t.H, t.W);
        // out = uu * mid + b1
        HIPCHK(launch_fpa_mix(P->dtype, scr + fpa_pyr_uu_offset(t.N, t.H, t.W), E.act(op.ins[0]), nullptr, nullptr, E.grad(op.out), E.grad(op.ins[0]), duu, t.N,
                              t.H * t.W, 32, E.st));
        E.ginit[op.ins[0]] = 1;
        HIPCHK(launch_image_sum(P->dtype, E.grad(op.out), E.grad(op.ins[1]), t.N, t.H * t.W, 32, 1.f, E.st));
        E.ginit[op.ins[1]] = 1;
        FpaPyrArgs a;
        memset(&a, 0, sizeof(a));
        a.N = t.N; a.h = t.H; a.w = t.W; a.train = 1; a.scratch = scr; a.gscratch = gs; a.duu = duu;
        for (int l = 0; l < 6; ++l) {
          const BNInfo& bn = P->bns[P->fpa.bn[l]];
          a.w_[l] = E.params + P->params[P->fpa.w[l]].off; a.b_[l] = E.params + P->params[P->fpa.b[l]].off;
          a.g_[l] = E.params + P->params[bn.gamma].off; a.be_[l] = E.params + P->params[bn.beta].off;
          a.rm_[l] = E.buffers; a.rv_[l] = E.buffers;
          a.dw_[l] = E.grads + P->params[P->fpa.w[l]].off; a.db_[l] = E.grads + P->params[P->fpa.b[l]].off;
          a.dg_[l] = E.grads + P->params[bn.gamma].off; a.dbe_[l] = E.grads + P->params[bn.beta].off;
        }
        HIPCHK(launch_fpa_pyr_bwd(a, E.st));
        // the wide 7x7 conv: d x1raw sits behind the first n1 floats of the gradient scratch; its input's gradient goes back through the max-pool
        HIPCHK(launch_fpa_in_bwd(P->dtype, E.act(P->fpa.pool), gs + n1, E.params + P->params[P->fpa.w[0]].off, E.grad(P->fpa.pool),
                                 E.grads + P->params[P->fpa.w[0]].off, E.grads + P->params[P->fpa.b[0]].off, t.N, t.H / 2, t.W / 2, t.C, 7, E.st));
        {
          const int acc = E.claim(op.in);
          HIPCHK(launch_maxpool2(P->dtype, E.act(op.in), nullptr, E.grad(P->fpa.pool), E.grad(op.in), t.N, t.H, t.W, t.C, acc, E.st));
        }
        break;
      }
      case OP_PAB: {
        const TensorInfo& t = P->tensors[op.in];
        const int hw = t.H * t.W;
        const size_t sbytes = align_up((size_t)t.N * hw * hw * sizeof(float));
        float* Pm = (float*)(E.ws + op.aux_off);
        float* dP = (float*)(E.ws + op.aux_off + sbytes);
        float* dM = (float*)(E.ws + op.aux_off + 2 * sbytes);
        // y = x + reshape(M): the gradient of y flows into x as it is, and into M through the same index map
        {
          const int acc = E.claim(op.in);
          HIPCHK(launch_masked_accum(P->dtype, E.grad(op.in), E.grad(op.out), nullptr, (size_t)t.N * hw * t.C, acc ? 0 : 1, E.st));
        }
        HIPCHK(launch_pab_mix(P->dtype, nullptr, nullptr, nullptr, dM, E.grad(op.out), t.N, hw, t.C, E.st));
        PabGemm g;
        memset(&g, 0, sizeof(g));
        g.batch = t.N;
        // dP[i][j] = sum_c dM[i][c] bottom[j][c]
        g.A = dM; g.a_f32 = 1; g.sAb = (size_t)hw * t.C; g.sAm = t.C; g.sAk = 1;
        g.B = E.act(op.ins[2]); g.sBb = (size_t)hw * t.C; g.sBk = 1; g.sBn = t.C;
        g.C = dP; g.c_f32 = 1; g.sCb = (size_t)hw * hw; g.sCm = hw; g.sCn = 1; g.M = hw; g.N = hw; g.K = t.C;
        HIPCHK(launch_pab_gemm(P->dtype, g, E.st));
        // d bottom[j][c] = sum_i P[i][j] dM[i][c]
        g.A = Pm; g.a_f32 = 1; g.sAb = (size_t)hw * hw; g.sAm = 1; g.sAk = hw;
        g.B = dM; g.b_f32 = 1; g.sBb = (size_t)hw * t.C; g.sBk = t.C; g.sBn = 1;
        g.C = E.grad(op.ins[2]); g.c_f32 = 0; g.sCb = (size_t)hw * t.C; g.sCm = t.C; g.sCn = 1; g.M = hw; g.N = t.C; g.K = hw;
        HIPCHK(launch_pab_gemm(P->dtype, g, E.st));
        E.ginit[op.ins[2]] = 1;
        HIPCHK(launch_pab_softmax(dP, Pm, t.N, (size_t)hw * hw, 1, E.st));     // dP -> dS in place
        // d center[i][k] = sum_j dS[i][j] top[j][k];   d top[j][k] = sum_i dS[i][j] center[i][k]
        g.A = dP; g.a_f32 = 1; g.sAb = (size_t)hw * hw; g.sAm = hw; g.sAk = 1;
        g.B = E.act(op.ins[0]); g.b_f32 = 0; g.sBb = (size_t)hw * 64; g.sBk = 64; g.sBn = 1;
        g.C = E.grad(op.ins[1]); g.sCb = (size_t)hw * 64; g.sCm = 64; g.sCn = 1; g.M = hw; g.N = 64; g.K = hw;
        HIPCHK(launch_pab_gemm(P->dtype, g, E.st));
        E.ginit[op.ins[1]] = 1;
        g.sAm = 1; g.sAk = hw;
        g.B = E.act(op.ins[1]);
        g.C = E.grad(op.ins[0]);
        HIPCHK(launch_pab_gemm(P->dtype, g, E.st));
        E.ginit[op.ins[0]] = 1;
        break;
      }
      case OP_MOSAIC: {     // the inverse re-arrangement of the gradient (gutters of a mosaic gradient are zero)
        const TensorInfo& tf = P->tensors[op.oc0 ? op.in : op.out];
        const int acc = E.claim(op.in);
        HIPCHK(launch_mosaic(P->dtype, E.grad(op.out), E.grad(op.in), tf.N, tf.H, tf.W, tf.C, op.up, op.oc0 ? 0 : 1, op.oc0 ? acc : 0, E.st));
        break;
      }
      case OP_BINPOOL: {
        const TensorInfo& t = P->tensors[op.in];
        const int acc = E.claim(op.in);
        HIPCHK(launch_bin_mean_bwd(P->dtype, E.grad(op.out), E.grad(op.in), t.N, t.H, t.W, t.C, op.up, acc, E.st));
        break;
      }
      case OP_UPB: {
        const TensorInfo& t = P->tensors[op.in];
        HIPCHK(launch_bilinear_adjoint(P->dtype, E.grad(op.out), E.grad(op.in), t.N, t.H, t.W, t.C, op.up, E.st));
        E.ginit[op.in] = 1;
        break;
      }
      case OP_DROPE: {
        const TensorInfo& t = P->tensors[op.out];
        HIPCHK(launch_drop_elem(P->dtype, E.grad(op.out), P->dropout_keep, 1.0f / (1.0f - P->dropout_p), E.grad(op.in),
                                (size_t)t.N * t.H * t.W * t.C, E.st));
        E.ginit[op.in] = 1;
        break;
      }
      case OP_BCAST: {      // gradient of a broadcast: per-image sums
        const TensorInfo& t = P->tensors[op.out];
        HIPCHK(launch_image_sum(P->dtype, E.grad(op.out), E.grad(op.in), t.N, t.H * t.W, t.C, 1.f, E.st));
        E.ginit[op.in] = 1;
        break;
      }
      case OP_GAP: {        // gradient of the mean: broadcast / HW, next to the other consumers of the ASPP input
        const TensorInfo& t = P->tensors[op.in];
        const int acc = E.claim(op.in);
        HIPCHK(launch_image_bcast(P->dtype, E.grad(op.out), E.grad(op.in), t.N, t.H * t.W, t.C, 1.f / (float)(t.H * t.W), acc, E.st));
        break;
      }
      case OP_DW: {
        const TensorInfo& ti = P->tensors[op.in];
        const TensorInfo& to = P->tensors[op.out];
        const ParamInfo& w = P->params[op.dwp];
        HIPCHK(launch_dw_wgrad(P->dtype, E.act(op.in), ti.C, 0, E.grad(op.out), to.C, op.oc0, E.grads + w.off, w.O, op.wc0, ti.N, ti.H, ti.W, ti.C,
                               op.up, E.st));
        if (ti.need_grad) {
          const int acc = E.claim(op.in);
          HIPCHK(launch_dw_conv(P->dtype, E.grad(op.out), to.C, op.oc0, E.grad(op.in), ti.C, 0, E.params + w.off, w.O, op.wc0, ti.N, ti.H, ti.W,
                                ti.C, op.up, 1, acc, E.st));
        }
        break;
      }
      case OP_PARITY: {     // the inverse permutation of the gradient
        const TensorInfo& tf = P->tensors[op.up ? op.in : op.out];
        const int acc = E.claim(op.in);
        HIPCHK(launch_parity_permute(P->dtype, E.grad(op.out), E.grad(op.in), tf.N, tf.H, tf.W, tf.C, op.up ? 0 : 1, acc, E.st));
        break;
      }
      case OP_UPLOGITS: {   // adjoint of the x4 bilinear resample: dL/dlogits (NHWC, padded channels) -> gradient of the stride-4 map
        const int h4 = P->H / P->head_up, w4 = P->W / P->head_up;
        HIPCHK(launch_bilinear_adjoint(P->dtype, E.ws + P->dlogits_off, E.ws + P->dz4_off, P->B, h4, w4, P->dlogits_C, P->head_up, E.st));
        break;
      }
      case OP_MERGE: {      // every summand's gradient = dropout mask * gradient of the sum: written once into the shared buffer
        const TensorInfo& t = P->tensors[op.out];
        HIPCHK(launch_drop_bwd(P->dtype, E.grad(op.out), P->dropout_keep, 1.0f / (1.0f - P->dropout_p), E.grad(op.ins[0]), t.N, (size_t)t.H * t.W,
                               t.C, E.st));
        for (int i = 0; i < 4; ++i) E.ginit[op.ins[i]] = 1;
        break;
      }
      case OP_GN: {
        const TensorInfo& t = P->tensors[op.in];
        GnArgs ga = E.gn_args(op.gn);
        if (op.up > 1) {      // gradient w.r.t. relu(gn(y)) at y's resolution: adjoint of the bilinear x2, parked in y's gradient buffer
          HIPCHK(launch_bilinear_adjoint(P->dtype, E.grad(op.out), E.grad(op.in), t.N, t.H, t.W, t.C, op.up, E.st));
          ga.g = E.grad(op.in);
        } else {
          ga.g = E.grad(op.out);
        }
        ga.dy = E.grad(op.in);
        E.ginit[op.in] = 1;
        HIPCHK(launch_gn_backward(P->dtype, ga, t.N, E.st));
        break;
      }
      case OP_UP2: {        // gradient of the nearest x2: 2x2 sums into the coarser level
        const TensorInfo& t = P->tensors[op.in];
        const int acc = E.claim(op.in);
        HIPCHK(launch_pool2x2_accum(P->dtype, E.grad(op.in), E.grad(op.out), t.N, t.H, t.W, t.C, acc ? 0 : 1, E.st));
        break;
      }
      case OP_MAXPOOL: {
        const TensorInfo& t = P->tensors[op.in];
        const int acc = E.claim(op.in);
        HIPCHK(launch_maxpool_bwd_idx(P->dtype, (const unsigned char*)(E.ws + P->pool_idx_off), E.grad(op.out), E.grad(op.in), t.N, t.H, t.W,
                                      t.C, acc ? 0 : 1, E.st));
        break;
      }
    }
    if (S)
      for (int k = 0; k < S->n; ++k)
        if (S->last_op[k] == oi) { rc = fire(k); if (rc) return rc; }
  }
  if (S)
    for (int k = 0; k < S->n; ++k)
      if (S->last_op[k] < 0) { rc = fire(k); if (rc) return rc; }   // (a slice nobody writes: zeros, still part of the exchange)
  if (E.wst && E.wst != E.st) {   // join: the caller's stream owns the complete gradient arena again
    HIPCHK(hipEventRecord(P->ev_join, E.wst));
    HIPCHK(hipStreamWaitEvent(E.st, P->ev_join, 0));
  }
  return OCTSEG_OK;
}

}  // namespace detail
}  // namespace octseg
