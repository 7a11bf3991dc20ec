// plan_forward.cpp -- the forward executor: side-stream creation, one-launch weight packing (training images, or eval images with the
// BatchNorm folded in), the tied forward of the decoder layers, and run_forward, which walks the op list over one or two lanes.
#include "plan_internal.h"

namespace octseg {
namespace detail {

// ---------------------------------------------------------------- error state and in-process kernel timing (plan_internal.h)
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

bool g_prof_on = false;
bool g_capturing = false;
bool g_prof_hbm = false;
std::vector<ProfRec> g_prof;
std::vector<hipEvent_t> g_prof_pool;
hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
  hipEvent_t e;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

// Side streams carry work that is off the critical chain: the second forward lane (default priority -- at low priority the fp16 ensemble's
// B = 1 replay, whose lanes ARE its critical path, fell from 148 to 121 frames/s) and the backward's weight gradients.  The latter's stream is
// created with the LOWEST priority: the chain's kernels win the dispatch whenever compute units free up, the weight gradients fill what is
// left (round 4, ABAB on one box, eager steps: 67.75-68.0 ms per step against 68.2-68.3 at the default priority, 69.1 at the highest; under
// graph replay round 3 saw no difference).
hipError_t create_side_stream(hipStream_t* st, bool backward) {
  if (backward) {
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) return e;
    return hipStreamCreateWithPriority(st, hipStreamNonBlocking, least);
  }
  // (a side stream confined to a share of the compute units -- hipExtStreamCreateWithCUMask, 6 / 4 / 7 of every 8 CUs -- so that the caller's
  //  stream always finds free CUs for its sweeps: 75.2 -> 91.7 ms per step whatever the share; measured once, not kept)
  return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}

// fold = 1 (eval forwards): scale / shift of every BatchNorm from the running statistics first (one launch), then every forward
// image with its BatchNorm's scale folded in (reference: what conv + BN in eval mode computes, src/predict.py / model.py:183-200);
// fold = 0 (training): plain images.  Cached until the parameters / buffers change or the mode flips.
int pack_all_weights(Exec& E, bool fold) {
  octseg_plan* P = E.P;
  if (P->packed_valid && P->packed_fold == fold && P->packed_ws == (const void*)E.ws && P->packed_params == (const void*)E.params &&
      (!fold || P->packed_buffers == (const void*)E.buffers))
    return OCTSEG_OK;
  if (P->pack_tab_ws != (const void*)E.ws) {   // first use of this workspace: upload the job table
    HIPCHK(hipMemcpyAsync(E.ws + P->pack_tab_off, P->pack_jobs.data(), P->pack_jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice, E.st));
    HIPCHK(hipMemcpyAsync(E.ws + P->pack_prefix_off, P->pack_prefix.data(), P->pack_prefix.size() * sizeof(unsigned long long),
                          hipMemcpyHostToDevice, E.st));
    if (!P->bn_jobs.empty()) {
      HIPCHK(hipMemcpyAsync(E.ws + P->bn_tab_off, P->bn_jobs.data(), P->bn_jobs.size() * sizeof(BnEvalJob), hipMemcpyHostToDevice, E.st));
      HIPCHK(hipMemcpyAsync(E.ws + P->bn_prefix_off, P->bn_prefix.data(), P->bn_prefix.size() * sizeof(unsigned), hipMemcpyHostToDevice, E.st));
    }
    P->pack_tab_ws = E.ws;
  }
  if (fold && !P->bn_jobs.empty())
    HIPCHK(launch_bn_finalize_eval_all(E.params, E.buffers, E.ws, (const BnEvalJob*)(E.ws + P->bn_tab_off),
                                       (const unsigned*)(E.ws + P->bn_prefix_off), (int)P->bn_jobs.size(), P->bn_total, 1e-5f, E.st));
  HIPCHK(launch_pack_all(P->dtype, E.params, E.ws, (const PackJob*)(E.ws + P->pack_tab_off),
                         (const unsigned long long*)(E.ws + P->pack_prefix_off), (int)P->pack_jobs.size(), P->pack_total, fold ? 1 : 0, E.st));
  P->packed_valid = true; P->packed_fold = fold; P->packed_ws = E.ws; P->packed_params = E.params; P->packed_buffers = E.buffers;
  return OCTSEG_OK;
}

static const void* fwd_weight(const Exec& E, const ConvLayer& L) { return E.ws + L.wimg_fwd_off; }

// Training forward of a tied layer (ConvLayer::tie & 1): the skip channels' 3x3 stores the output, the four parity launches of the 4x4
// stride-2 kernel over the low-resolution source add to it, one sweep takes the BatchNorm statistics of the finished tensor.
static int tied_forward(Exec& E, const ConvLayer& L, hipStream_t st, float* slab) {
  octseg_plan* P = E.P;
  SrcDesc src[MAX_SRC];
  const int ns = E.fill_srcs(L, src);
  DstDesc d;
  d.ptr = E.act(L.out); d.C = L.Cout; d.c0 = 0; d.cn = L.Cout; d.H = L.OH; d.W = L.OW; d.accum = 0; d.pool = 0;
  const double macs = layer_macs(L);   // (profile classes keep the reference graph's count: the nine taps over every upsampled pixel)
  if (L.tie_Cs > 0) {
    std::vector<ConvArgs> v;
    fwd_launches(tie_geom_skip(L), v);
    ConvArgs& a = v[0];
    a.nsrc = ns - 1;
    for (int i = 1; i < ns; ++i) { a.src[i - 1] = src[i]; a.src[i - 1].c0 -= L.tie_Ca; }
    a.W = E.ws + L.tie_fs_off;
    a.dst[0] = d; a.ndst = 1; a.out_mode = OUT_STORE;
    ProfScope ps(0, 2.0 * macs * L.tie_Cs / L.Cin, st, L.name);
    HIPCHK(launch_conv(P->dtype, a, st));
  }
  std::vector<ConvArgs> v;
  fwd_launches(tie_geom_up(L), v);
  for (auto& a : v) {
    a.nsrc = 1; a.src[0] = src[0]; a.src[0].up = 0; a.src[0].c0 = 0;
    a.W = E.ws + L.tie_fu_off;
    d.accum = L.tie_Cs > 0 ? 1 : 0;   // (the four parities are disjoint: without a skip launch each one stores its own pixels)
    a.dst[0] = d; a.ndst = 1; a.out_mode = OUT_STORE;
    ProfScope ps(0, 2.0 * macs * L.tie_Ca / L.Cin / 4.0, st, L.name);
    HIPCHK(launch_conv(P->dtype, a, st));
  }
  const BNInfo& b = P->bns[L.bn];
  HIPCHK(launch_tensor_stats(P->dtype, E.act(L.out), (size_t)L.N * L.OH * L.OW, b.C, slab, b.rows, st));
  return OCTSEG_OK;
}

int run_forward(Exec& E, const float* image, float* logits, int normalize, const float* mean, const float* stdv) {
  octseg_plan* P = E.P;
  if (!P->run_error.empty()) return fail(OCTSEG_BAD_SHAPE, P->run_error);
  const bool frozen = E.train && P->frozen_bn;   // BatchNorm on its running statistics inside the training op path (octseg_plan_set_frozen_bn)
  if (E.train && !frozen)
    for (auto& b : P->bns)
      if (b.count <= 1.0) {   // torch.nn.functional.batch_norm raises the same way (reference runs it in training)
        const TensorInfo& t = P->tensors[b.y];
        char buf[192];
        snprintf(buf, sizeof buf, "Expected more than 1 value per channel when training, got input size torch.Size([%d, %d, %d, %d])",
                 t.N, t.C, t.H, t.W);
        return fail(OCTSEG_BAD_SHAPE, buf);
      }
  int rc = pack_all_weights(E, !E.train);
  if (rc) return rc;
  if (E.train) HIPCHK(hipMemsetAsync(E.ws + P->fin_cnt_off, 0, 2 * 64 * sizeof(unsigned), E.st));
  // eval: BatchNorm is folded -- scale into the weight images (pack_all_weights), shift into the conv epilogue's bias, ReLU into
  // the epilogue of every conv whose BatchNorm is only read through relu(bn(y)): consumers stage plain activations
  const bool folded = !E.train;
  // ---- forward lanes (assign_lanes): lane-1 ops go to the side stream; a lane waits for the other one only when it
  // reads something the other lane produced and has not synchronised with since
  const bool lanes = P->has_lanes && !serial_mode();
  hipStream_t lst[2] = {E.st, E.st};
  if (lanes) {
    // training forwards share the backward's lowest-priority stream (the second lane yields to the encoder chain: 69.1 / 68.6 against 69.7 /
    // 69.0 ms per step, ABAB); eval forwards -- the ensemble's B = 1 replay, whose lanes are its critical path -- and captured steps keep the
    // default priority
    const bool low = E.train && !P->tgraph_enabled;
    hipStream_t* lsp = low ? &P->side_bwd : &P->side;
    if (!*lsp) HIPCHK(create_side_stream(lsp, low));
    if (!P->ev_fork) {
      HIPCHK(hipEventCreateWithFlags(&P->ev_fork, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&P->ev_join, hipEventDisableTiming));
    }
    lst[1] = *lsp;
  }
  std::vector<int> tseq(P->tensors.size(), 0), bseq(P->bns.size(), 0);   // producer: lane * 2^24 + sequence number on it
  int enq[2] = {1, 0}, seen[2] = {0, 0};   // ops enqueued per lane (main starts at 1: everything in front of the loop);
                                           // seen[l]: how much of the OTHER lane lane l has waited for
  auto need = [&](int lane, int stamp) -> int {   // make `lane` wait for the producer stamped `stamp`
    if (!lanes) return OCTSEG_OK;
    const int pl = stamp >> 24, ps = stamp & 0xffffff;
    if (pl == lane || ps <= seen[lane]) return OCTSEG_OK;
    hipEvent_t ev = lane == 1 ? P->ev_fork : P->ev_join;
    HIPCHK(hipEventRecord(ev, lst[pl]));
    HIPCHK(hipStreamWaitEvent(lst[lane], ev, 0));
    seen[lane] = enq[pl];
    return OCTSEG_OK;
  };
  auto need_val = [&](int lane, const Value& v) -> int {
    int rc2 = OCTSEG_OK;
    if (v.t >= 0) rc2 = need(lane, tseq[v.t]);
    if (!rc2 && v.bn >= 0) rc2 = need(lane, bseq[v.bn]);
    return rc2;
  };
  for (auto& op : P->ops) {
    const int lane = lanes ? op.lane : 0;
    hipStream_t st = lst[lane];
    const int stamp = (lane << 24) | (enq[lane] + 1);
    float* slab_l = (float*)(E.ws + P->slab_off + (size_t)lane * P->slab_bytes);
    double* part_l = (double*)(E.ws + P->fin_part_off) + (size_t)lane * SLAB_PART_CAP * 2;
    unsigned* cnt_l = (unsigned*)(E.ws + P->fin_cnt_off) + lane * 64;
    if (lane == 1 && enq[1] == 0) { rc = need(1, 1); if (rc) return rc; }   // the side lane starts behind the setup work
    switch (op.kind) {
      case OP_STEM_COL: {
        const TensorInfo& t = P->tensors[op.out];
        // (2-byte dtypes: the stem conv gathers its im2col rows straight from the frame in LDS, thin.hip KSTEM -- no 634 MB tensor)
        if (!(P->stem_k == 7 && thin_stem_eligible(P->dtype)))
          HIPCHK(launch_stem_im2col(P->dtype, image, E.act(op.out), P->B, P->H, P->W, t.C, mean, stdv, normalize, st, P->stem_k, P->stem_pad));
        tseq[op.out] = stamp;
        break;
      }
      case OP_CONV: {
        const ConvLayer& L = P->convs[op.conv];
        for (auto& sct : L.srcs) { rc = need_val(lane, sct.v); if (rc) return rc; }
        if (L.stem && (P->stem_k == 7 && thin_stem_eligible(P->dtype))) {
          StemArgs sa;
          memset(&sa, 0, sizeof(sa));
          sa.img = image; sa.N = P->B; sa.H = P->H; sa.W = P->W; sa.normalize = normalize;
          for (int i = 0; i < 3; ++i) { sa.mean[i] = normalize ? mean[i] : 0.f; sa.stdv[i] = normalize ? stdv[i] : 1.f; }
          sa.w = E.params + P->params[L.w].off;
          if (folded && L.bn >= 0) { sa.wscale = E.bn_scale(L.bn); sa.bias = E.bn_shift(L.bn); sa.relu_out = P->bns[L.bn].lazy ? 1 : 0; }
          sa.y = E.act(L.out);
          sa.slab = (L.bn >= 0 && E.train) ? slab_l : nullptr; sa.slab_row0 = 0;
          {
            ProfScope ps(0, 2.0 * layer_macs(L), st, L.name);
            HIPCHK(launch_thin_stem_forward(P->dtype, sa, st));
          }
          if (E.train) {   // the weight gradient re-gathers the frame: remember where it is (the caller keeps it alive until the backward)
            P->stem_image = image; P->stem_normalize = normalize;
            for (int i = 0; i < 3; ++i) { P->stem_mean[i] = sa.mean[i]; P->stem_std[i] = sa.stdv[i]; }
          }
          tseq[L.out] = stamp;
          break;
        }
        if ((L.tie & 1) && E.train && !folded) {
          rc = tied_forward(E, L, st, slab_l);
          if (rc) return rc;
          tseq[L.out] = stamp;
          break;
        }
        std::vector<ConvArgs> la;
        fwd_launches(E.geom(L), la);
        int row0 = 0;
        for (auto& a : la) {
          a.nsrc = E.fill_srcs(L, a.src);
          a.W = fwd_weight(E, L);
          a.bias = L.b >= 0 ? E.params + P->params[L.b].off : nullptr;
          // (ConvT: [4][4][O][I], same indexing; the stem's im2col GEMM: [O][KP] = one tap of KP input channels)
          a.Wmaster = E.params + P->params[L.w].off; a.wO = L.Cout; a.wI = L.Cin; a.wtrans = 0;
          if (folded) {
            for (int i = 0; i < a.nsrc; ++i) { a.src[i].scale = nullptr; a.src[i].shift = nullptr; a.src[i].relu = 0; }
            if (L.bn >= 0) { a.bias = E.bn_shift(L.bn); a.relu_out = P->bns[L.bn].lazy ? 1 : 0; a.wscale = E.bn_scale(L.bn); }
            else if (L.fold_bn >= 0) {   // one group of a grouped conv: its slice of the tensor's BatchNorm
              a.bias = E.bn_shift(L.fold_bn) + L.out_c0; a.relu_out = P->bns[L.fold_bn].lazy ? 1 : 0; a.wscale = E.bn_scale(L.fold_bn) + L.out_c0;
            }
          }
          a.ndst = 1;
          DstDesc d;
          d.accum = L.accum_out ? 1 : 0; d.pool = 0;
          if (L.head) {   // NCHW f32: the caller's logits, or (FPN) the stride-4 map that OP_UPLOGITS resamples
            d.ptr = P->head_up > 1 ? (void*)(E.ws + P->z4_off) : (void*)logits;
            d.C = L.Cout; d.c0 = 0; d.cn = L.Cout; d.H = L.OH; d.W = L.OW; a.out_mode = OUT_HEAD_NCHW;
          }
          else {
            d.ptr = (char*)E.act(L.out) + (size_t)L.out_c0 * dtype_size(P->dtype);
            d.C = L.sliced ? P->tensors[L.out].C : L.Cout; d.c0 = 0; d.cn = L.Cout; d.H = L.OH; d.W = L.OW; a.out_mode = OUT_STORE;
          }
          a.dst[0] = d;
          a.stat_slab = (L.bn >= 0 && E.train) ? slab_l : nullptr;
          a.slab_row0 = row0;
          row0 += conv_num_mtiles_flat(a, P->dtype);
          ProfScope ps(0, 2.0 * layer_macs(L) / (double)la.size(), st, L.name);
          HIPCHK(launch_conv(P->dtype, a, st));
        }
        if (L.bn >= 0 && E.train && row0 != P->bns[L.bn].rows)
          return fail(OCTSEG_BAD_ARG, "internal: BN-statistics slab rows of " + L.name + " differ between plan and launch");
        if (L.out >= 0) tseq[L.out] = stamp;
        break;
      }
      case OP_BN_FIN: {
        const BNInfo& b = P->bns[op.bn];
        const float* gamma = E.params + P->params[b.gamma].off;
        const float* beta = E.params + P->params[b.beta].off;
        rc = need(lane, tseq[b.y]);   // same lane as its conv by construction; kept for safety
        if (rc) return rc;
        if (frozen)   // the conv epilogues still fill their slabs (the training launches as they are); nobody reads them, no buffer is written
          HIPCHK(launch_bn_finalize_frozen(b.C, gamma, beta, E.buffers + b.rm_off, E.buffers + b.rv_off, b.eps, E.bn_scale(op.bn), E.bn_shift(op.bn),
                                           E.bn_mean(op.bn), E.bn_rstd(op.bn), E.bn_coef(op.bn), st));
        else if (E.train && b.count <= (double)BN_SMALL_COUNT)   // small tensors (pooled ASPP branch, 2x2 .. 16x16 maps): exact two-pass statistics
          HIPCHK(launch_bn_finalize_small(P->dtype, E.act(b.y), (int)b.count, b.C, gamma, beta, E.buffers + b.rm_off, E.buffers + b.rv_off, b.momentum,
                                          b.eps, E.bn_scale(op.bn), E.bn_shift(op.bn), E.bn_mean(op.bn), E.bn_rstd(op.bn), st));
        else if (E.train)
          HIPCHK(launch_bn_finalize_train(slab_l, b.rows, b.C, b.count, gamma, beta,
                                          E.buffers + b.rm_off, E.buffers + b.rv_off, b.momentum, b.eps, E.bn_scale(op.bn),
                                          E.bn_shift(op.bn), E.bn_mean(op.bn), E.bn_rstd(op.bn), part_l, cnt_l, st));
        // (eval: done for every BatchNorm at once in front of the loop)
        bseq[op.bn] = E.train ? stamp : 1;
        break;
      }
      case OP_BN_ACT: {
        const TensorInfo& t = P->tensors[op.out];
        rc = need_val(lane, op.y); if (rc) return rc;
        rc = need_val(lane, op.res); if (rc) return rc;
        if (op.post >= 0) { rc = need(lane, tseq[op.post]); if (rc) return rc; }
        BnActArgs a;
        memset(&a, 0, sizeof(a));
        a.y = E.act(op.y.t);
        if (!folded) { a.scale = E.bn_scale(op.y.bn); a.shift = E.bn_shift(op.y.bn); }
        if (op.res.t >= 0) {
          a.res = E.act(op.res.t);
          if (op.res.bn >= 0 && !folded) { a.rscale = E.bn_scale(op.res.bn); a.rshift = E.bn_shift(op.res.bn); }
        }
        if (op.post >= 0) a.post = E.act(op.post);
        a.out = E.act(op.out); a.npix = (size_t)t.N * t.H * t.W; a.C = t.C; a.relu = op.relu;
        if (E.train && t.mask_off) a.maskbits = (unsigned char*)(E.ws + t.mask_off);
        {
          const double tb = (double)a.npix * a.C * dtype_size(P->dtype);
          ProfScope ps(3, tb * (2 + (a.res ? 1 : 0) + (a.post ? 1 : 0)), st, "bn_act");
          HIPCHK(launch_bn_act(P->dtype, a, st));
        }
        tseq[op.out] = stamp;
        break;
      }
      case OP_UP2: {
        const TensorInfo& t = P->tensors[op.in];
        HIPCHK(launch_up2_fill(P->dtype, E.act(op.in), E.act(op.out), t.N, t.H, t.W, t.C, st));
        break;
      }
      case OP_GN: {
        const TensorInfo& t = P->tensors[op.in];
        const GnArgs ga = E.gn_args(op.gn);
        GnArgs a2 = ga;
        a2.out = E.act(op.out);
        HIPCHK(launch_gn_forward(P->dtype, a2, t.N, t.H, t.W, op.up, st));
        break;
      }
      case OP_MERGE: {
        const TensorInfo& t = P->tensors[op.out];
        if (E.train && P->dropout_keep == nullptr)
          return fail(OCTSEG_BAD_ARG, "FPN training forward: no Dropout2d keep mask set (octseg_plan_set_dropout: device float [B][128] of 0 / 1)");
        HIPCHK(launch_merge_drop(P->dtype, E.act(op.ins[0]), E.act(op.ins[1]), E.act(op.ins[2]), E.act(op.ins[3]),
                                 E.train ? P->dropout_keep : nullptr, 1.0f / (1.0f - P->dropout_p), E.act(op.out), t.N, (size_t)t.H * t.W, t.C, st));
        break;
      }
      case OP_PARITY: {
        const TensorInfo& tf = P->tensors[op.up ? op.in : op.out];   // the fine tensor
        HIPCHK(launch_parity_permute(P->dtype, E.act(op.in), E.act(op.out), tf.N, tf.H, tf.W, tf.C, op.up, 0, st));
        break;
      }
      case OP_DW: {
        const TensorInfo& ti = P->tensors[op.in];
        const TensorInfo& to = P->tensors[op.out];
        const ParamInfo& w = P->params[op.dwp];
        HIPCHK(launch_dw_conv(P->dtype, E.act(op.in), ti.C, 0, E.act(op.out), to.C, op.oc0, E.params + w.off, w.O, op.wc0, ti.N, ti.H, ti.W, ti.C,
                              op.up, 0, 0, st));
        break;
      }
      case OP_GAP: {
        const TensorInfo& t = P->tensors[op.in];
        HIPCHK(launch_image_sum(P->dtype, E.act(op.in), E.act(op.out), t.N, t.H * t.W, t.C, (float)(t.H * t.W), st));
        break;
      }
      case OP_BCAST: {
        const TensorInfo& t = P->tensors[op.out];
        HIPCHK(launch_image_bcast(P->dtype, E.act(op.in), E.act(op.out), t.N, t.H * t.W, t.C, 1.f, 0, st));
        break;
      }
      case OP_DROPE: {
        const TensorInfo& t = P->tensors[op.out];
        if (E.train && P->dropout_keep == nullptr)
          return fail(OCTSEG_BAD_ARG, "DeepLabV3(+) training forward: no dropout keep mask set (octseg_plan_set_dropout: device float "
                                      "[B][H/s][W/s][256] of 0 / 1, NHWC; s = 16, DeepLabV3: 8)");
        HIPCHK(launch_drop_elem(P->dtype, E.act(op.in), E.train ? P->dropout_keep : nullptr, 1.0f / (1.0f - P->dropout_p), E.act(op.out),
                                (size_t)t.N * t.H * t.W * t.C, st));
        break;
      }
      case OP_UPB: {
        const TensorInfo& t = P->tensors[op.in];
        HIPCHK(launch_bilinear_up(P->dtype, E.act(op.in), E.act(op.out), t.N, t.H, t.W, t.C, op.up, st));
        break;
      }
      case OP_BINPOOL: {
        const TensorInfo& t = P->tensors[op.in];
        HIPCHK(launch_bin_mean(P->dtype, E.act(op.in), E.act(op.out), t.N, t.H, t.W, t.C, op.up, st));
        break;
      }
      case OP_MOSAIC: {
        const TensorInfo& tf = P->tensors[op.oc0 ? op.in : op.out];   // the fine tensor
        HIPCHK(launch_mosaic(P->dtype, E.act(op.in), E.act(op.out), tf.N, tf.H, tf.W, tf.C, op.up, op.oc0, 0, st));
        break;
      }
      case OP_STATS: {
        if (E.train) {
          const BNInfo& b = P->bns[op.bn];
          const TensorInfo& t = P->tensors[op.in];
          HIPCHK(launch_tensor_stats(P->dtype, E.act(op.in), (size_t)t.N * t.H * t.W, b.C, slab_l, b.rows, st));
        }
        break;
      }
      case OP_SEGATE: {
        const TensorInfo& t = P->tensors[op.in];
        HIPCHK(launch_se_gate(P->dtype, E.act(op.in), E.act(op.ins[0]), E.act(op.out), t.N, t.H * t.W, t.C, 0, st,
                              op.ins[1] >= 0 ? E.act(op.ins[1]) : nullptr));
        break;
      }
      case OP_ADD: {
        const TensorInfo& t = P->tensors[op.out];
        HIPCHK(launch_add2(P->dtype, E.act(op.in), E.act(op.ins[0]), E.act(op.out), (size_t)t.N * t.H * t.W * t.C, st));
        break;
      }
      case OP_FPA: {
        const TensorInfo& t = P->tensors[op.in];
        float* scr = (float*)(E.ws + P->fpa.scratch_off);
        HIPCHK(launch_maxpool2(P->dtype, E.act(op.in), E.act(P->fpa.pool), nullptr, nullptr, t.N, t.H, t.W, t.C, 0, st));
        HIPCHK(launch_fpa_in_fwd(P->dtype, E.act(P->fpa.pool), E.params + P->params[P->fpa.w[0]].off, E.params + P->params[P->fpa.b[0]].off, scr, t.N, t.H / 2,
                                 t.W / 2, t.C, 7, st));
        FpaPyrArgs a;
        memset(&a, 0, sizeof(a));
        a.N = t.N; a.h = t.H; a.w = t.W; a.train = E.train; a.scratch = scr;
        for (int l = 0; l < 6; ++l) {
          const BNInfo& bn = P->bns[P->fpa.bn[l]];
          a.w_[l] = E.params + P->params[P->fpa.w[l]].off; a.b_[l] = E.params + P->params[P->fpa.b[l]].off;
          a.g_[l] = E.params + P->params[bn.gamma].off; a.be_[l] = E.params + P->params[bn.beta].off;
          a.rm_[l] = E.buffers + bn.rm_off; a.rv_[l] = E.buffers + bn.rv_off;
        }
        HIPCHK(launch_fpa_pyr_fwd(a, st));
        HIPCHK(launch_fpa_mix(P->dtype, scr + fpa_pyr_uu_offset(t.N, t.H, t.W), E.act(op.ins[0]), E.act(op.ins[1]), E.act(op.out), nullptr, nullptr, nullptr, t.N,
                              t.H * t.W, 32, st));
        break;
      }
      case OP_PAB: {
        const TensorInfo& t = P->tensors[op.in];
        const int hw = t.H * t.W;
        float* S = (float*)(E.ws + op.aux_off);
        float* M = (float*)(E.ws + op.aux_off + 2 * align_up((size_t)t.N * hw * hw * sizeof(float)));
        PabGemm g;
        memset(&g, 0, sizeof(g));
        g.batch = t.N;
        // S[i][j] = sum_k center[i][k] top[j][k]
        g.A = E.act(op.ins[1]); g.sAb = (size_t)hw * 64; g.sAm = 64; g.sAk = 1;
        g.B = E.act(op.ins[0]); g.sBb = (size_t)hw * 64; g.sBk = 1; g.sBn = 64;
        g.C = S; g.sCb = (size_t)hw * hw; g.sCm = hw; g.sCn = 1; g.c_f32 = 1; g.M = hw; g.N = hw; g.K = 64;
        HIPCHK(launch_pab_gemm(P->dtype, g, st));
        HIPCHK(launch_pab_softmax(S, nullptr, t.N, (size_t)hw * hw, 0, st));
        // M[i][c] = sum_j P[i][j] bottom[j][c]
        g.A = S; g.a_f32 = 1; g.sAb = (size_t)hw * hw; g.sAm = hw; g.sAk = 1;
        g.B = E.act(op.ins[2]); g.b_f32 = 0; g.sBb = (size_t)hw * t.C; g.sBk = t.C; g.sBn = 1;
        g.C = M; g.sCb = (size_t)hw * t.C; g.sCm = t.C; g.sCn = 1; g.M = hw; g.N = t.C; g.K = hw;
        HIPCHK(launch_pab_gemm(P->dtype, g, st));
        HIPCHK(launch_pab_mix(P->dtype, E.act(op.in), M, E.act(op.out), nullptr, nullptr, t.N, hw, t.C, st));
        break;
      }
      case OP_DWG: {
        const TensorInfo& ti = P->tensors[op.in];
        const TensorInfo& to = P->tensors[op.out];
        DwgArgs a;
        memset(&a, 0, sizeof(a));
        a.in = E.act(op.in); a.out = E.act(op.out); a.w = E.params + P->params[op.dwp].off;
        a.N = ti.N; a.H = ti.H; a.W = ti.W; a.C = ti.C; a.OH = to.H; a.OW = to.W; a.K = op.wc0; a.stride = op.up; a.pad = op.oc0;
        HIPCHK(launch_dwg_fwd(P->dtype, a, st));
        break;
      }
      case OP_BNX: {
        const TensorInfo& t = P->tensors[op.out];
        rc = need_val(lane, op.y); if (rc) return rc;
        BnxArgs a;
        memset(&a, 0, sizeof(a));
        a.y = E.act(op.y.t);
        if (!(folded && op.conv_bn)) { a.scale = E.bn_scale(op.y.bn); a.shift = E.bn_shift(op.y.bn); }   // (eval: a conv's BatchNorm is in its epilogue already)
        if (E.train && op.oc0 >= 0) {
          if (P->drop_connect == nullptr)
            return fail(OCTSEG_BAD_ARG, "EfficientNet training forward: no drop_connect factors set (octseg_plan_set_drop_connect: device float [" +
                                        std::to_string(P->dc_rates.size()) + "][B] of 0 or 1 / (1 - rate))");
          a.dscale = P->drop_connect + (size_t)op.oc0 * t.N;
        }
        a.post = op.post >= 0 ? E.act(op.post) : nullptr;
        a.out = E.act(op.out); a.npix = (size_t)t.N * t.H * t.W; a.hw = t.H * t.W; a.C = t.C; a.act = op.up;
        HIPCHK(launch_bnx_fwd(P->dtype, a, st));
        tseq[op.out] = stamp;
        break;
      }
      case OP_SEFC: {
        const TensorInfo& t = P->tensors[op.in];
        SefcArgs a;
        memset(&a, 0, sizeof(a));
        a.m = E.act(op.in); a.s = E.act(op.out);
        a.w1 = E.params + P->params[op.ins[0]].off; a.b1 = E.params + P->params[op.ins[1]].off;
        a.w2 = E.params + P->params[op.ins[2]].off; a.b2 = E.params + P->params[op.ins[3]].off;
        a.h = (float*)(E.ws + op.aux_off); a.dh = a.h + (size_t)t.N * op.up;
        a.N = t.N; a.C = t.C; a.R = op.up; a.act = op.oc0;
        HIPCHK(launch_sefc_fwd(P->dtype, a, st));
        break;
      }
      case OP_RESIZE: {
        const TensorInfo& ti = P->tensors[op.in];
        const TensorInfo& to = P->tensors[op.out];
        HIPCHK(launch_bilinear_resize(P->dtype, E.act(op.in), E.act(op.out), ti.N, ti.H, ti.W, to.H, to.W, ti.C, st));
        break;
      }
      case OP_RELU: {
        const TensorInfo& t = P->tensors[op.out];
        HIPCHK(launch_relu(P->dtype, E.act(op.in), nullptr, E.act(op.out), (size_t)t.N * t.H * t.W * t.C, st));
        break;
      }
      case OP_DROP2D: {
        const TensorInfo& t = P->tensors[op.out];
        if (E.train && P->dropout_keep == nullptr)
          return fail(OCTSEG_BAD_ARG, "PSPNet training forward: no Dropout2d keep mask set (octseg_plan_set_dropout: device float [B][512] of 0 / 1)");
        if (E.train) HIPCHK(launch_drop_bwd(P->dtype, E.act(op.in), P->dropout_keep, 1.0f / (1.0f - P->dropout_p), E.act(op.out), t.N, (size_t)t.H * t.W, t.C, st));
        else HIPCHK(launch_drop_elem(P->dtype, E.act(op.in), nullptr, 1.f, E.act(op.out), (size_t)t.N * t.H * t.W * t.C, st));   // eval: identity (copy)
        break;
      }
      case OP_UPLOGITS: {
        const int h4 = P->H / P->head_up, w4 = P->W / P->head_up;
        HIPCHK(launch_bilinear_nchw((const float*)(E.ws + P->z4_off), logits, P->B * P->classes, h4, w4, P->head_up, st));
        break;
      }
      case OP_MAXPOOL: {
        const TensorInfo& t = P->tensors[op.in];
        rc = need(lane, tseq[op.in]); if (rc) return rc;
        HIPCHK(launch_maxpool_fwd(P->dtype, E.act(op.in), E.act(op.out), E.train ? (unsigned char*)(E.ws + P->pool_idx_off) : nullptr, t.N,
                                  t.H, t.W, t.C, st));
        tseq[op.out] = stamp;
        break;
      }
    }
    ++enq[lane];
  }
  if (lanes && enq[1] > seen[0]) {   // join: the caller's stream owns everything again
    HIPCHK(hipEventRecord(P->ev_join, lst[1]));
    HIPCHK(hipStreamWaitEvent(lst[0], P->ev_join, 0));
  }
  return OCTSEG_OK;
}

}  // namespace detail
}  // namespace octseg
