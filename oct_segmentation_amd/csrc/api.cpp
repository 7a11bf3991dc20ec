// api.cpp -- the C ABI of include/octseg.h: plan lifetime and queries, the network entry points (eager, or captured into a hipGraph and
// replayed), profiling start / stop, the loss / optimizer / pipeline and single-op entry points, the debug and deterministic switches.
#include "plan_internal.h"

#include <cctype>

using namespace octseg;
using namespace octseg::detail;

static std::string lower(const char* s) {
  std::string r(s ? s : "");
  for (auto& c : r) c = (char)tolower((unsigned char)c);
  return r;
}

// The hipGraph lifecycle of a captured entry point.  A new argument set (`same_key` false) drops the old graph and starts over; the first
// call with a set runs `body` eagerly (function attributes, job tables, side streams and events exist afterwards), the second captures
// and instantiates it, and every call from then on replays the graph.  `outside` is work that stays out of the graph and runs before a
// replay or a capture.  `train` (the training step): the captured body repacks the weight images behind the host cache's back, so
// `packed_valid` is dropped wherever the workspace images stop matching it, and no profiling event is recorded inside the capture.
template <class Outside, class Body>
static int graph_call(octseg_plan* p, bool train, bool same_key, hipGraphExec_t& exec, int& seen, hipStream_t st, Outside&& outside, Body&& body) {
  if (!same_key) {   // new argument set: drop the old graph, start over with eager calls
    if (exec) { (void)hipGraphExecDestroy(exec); exec = nullptr; }
    seen = 0;
  }
  if (const int rc = outside()) return rc;
  // a replay of the training step repacks the UNFOLDED training weight images and rewrites the BatchNorm scale / shift in the workspace behind the
  // host cache's back: drop the cache, or an eval forward of this plan would take the hit and run its folded epilogue on unfolded images
  auto replay = [&]() -> int { HIPCHK(hipGraphLaunch(exec, st)); if (train) p->packed_valid = false; return OCTSEG_OK; };
  if (exec) return replay();
  if (seen++ == 0) return body();   // eager warm-up call
  if (train) p->packed_valid = false;   // the captured step must contain the weight packing (a replay meets new parameters)
  hipGraph_t g = nullptr;
  HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  g_capturing = train;
  const int rc = body();
  g_capturing = false;
  const hipError_t ce = hipStreamEndCapture(st, &g);
  if (train) p->packed_valid = false;   // (nothing was executed: the images in the workspace are whatever the last real step left)
  hipError_t ie = hipSuccess;
  if (!rc && ce == hipSuccess && (ie = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0)) != hipSuccess) exec = nullptr;
  if (g) (void)hipGraphDestroy(g);
  if (rc) return rc;
  if (ce != hipSuccess) return fail(OCTSEG_HIP_ERROR, std::string(train ? "training-step capture: " : "") + hipGetErrorString(ce));
  if (ie != hipSuccess) return fail(OCTSEG_HIP_ERROR, hipGetErrorString(ie));
  return replay();
}

// ================================================================ C ABI
extern "C" {

int octseg_version(void) { return 100; }
const char* octseg_last_error(void) { return g_err.c_str(); }

int octseg_plan_create(const octseg_net_desc* d, octseg_plan** out) {
  if (!d || !out) return fail(OCTSEG_BAD_ARG, "null argument");
  *out = nullptr;
  if (d->dtype != OCTSEG_F32 && d->dtype != OCTSEG_BF16 && d->dtype != OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, "dtype must be f32, bf16 or f16");
  if (d->height <= 0 || d->width <= 0 || d->height % 32 != 0 || d->width % 32 != 0) {
    char buf[256];
    snprintf(buf, sizeof buf, "Wrong input shape height=%d, width=%d. Expected image height and width divisible by 32.",
             d->height, d->width);
    return fail(OCTSEG_BAD_SHAPE, buf);
  }
  if (d->batch <= 0 || d->classes <= 0 || d->classes > 16) return fail(OCTSEG_BAD_SHAPE, "batch > 0 and 1 <= classes <= 16 required");
  const std::string enc = lower(d->encoder);
  if (enc != "resnet18" && enc != "resnet34" && enc != "resnet50" && enc != "resnet101" && enc != "resnet152" && enc != "timm-regnetx_002" &&
      enc != "timm-regnetx_064" && enc != "timm-regnety_120" && enc != "efficientnet-b0" && enc != "efficientnet-b5" && enc != "efficientnet-b7")
    return fail(OCTSEG_UNSUPPORTED_ARCH, "unknown encoder '" + enc + "' (resnet18 | resnet34 | resnet50 | resnet101 | resnet152 | timm-regnetx_002 | timm-regnetx_064 | timm-regnety_120 | efficientnet-b0 | efficientnet-b5 | efficientnet-b7)");
  octseg_plan* P = new octseg_plan();
  P->arch = lower(d->arch); P->encoder = enc; P->classes = d->classes;
  P->B = d->batch; P->H = d->height; P->W = d->width; P->dtype = d->dtype;
  const int rc = build_plan(P);
  if (rc) { delete P; return rc; }
  *out = P;
  return OCTSEG_OK;
}
int octseg_plan_destroy(octseg_plan* p) {
  if (p) {
    if (p->side) (void)hipStreamDestroy(p->side);
    if (p->side_bwd) (void)hipStreamDestroy(p->side_bwd);
    if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
    if (p->ev_join) (void)hipEventDestroy(p->ev_join);
    if (p->ev_slice) (void)hipEventDestroy(p->ev_slice);
    if (p->graph_exec) (void)hipGraphExecDestroy(p->graph_exec);
    if (p->tgraph_exec) (void)hipGraphExecDestroy(p->tgraph_exec);
  }
  delete p;
  return OCTSEG_OK;
}
size_t octseg_plan_workspace_bytes(const octseg_plan* p) { return p ? p->ws_bytes : 0; }
size_t octseg_plan_param_numel(const octseg_plan* p) { return p ? p->param_numel : 0; }
size_t octseg_plan_buffer_numel(const octseg_plan* p) { return p ? p->buffer_numel : 0; }
int octseg_plan_num_params(const octseg_plan* p) { return p ? (int)p->params.size() : 0; }
int octseg_plan_num_bn(const octseg_plan* p) { return p ? (int)p->bns.size() : 0; }
double octseg_plan_fwd_macs(const octseg_plan* p) { return p ? p->fwd_macs : 0.0; }
int octseg_plan_exec_macs(const octseg_plan* p, double* out3) {
  if (p == nullptr || out3 == nullptr) return OCTSEG_BAD_ARG;
  for (int k = 0; k < 3; ++k) out3[k] = p->exec_macs[k];
  return OCTSEG_OK;
}

int octseg_plan_param_info(const octseg_plan* p, int i, octseg_param_info* o) {
  if (!p || !o || i < 0 || i >= (int)p->params.size()) return fail(OCTSEG_BAD_ARG, "param index out of range");
  const ParamInfo& q = p->params[i];
  memset(o, 0, sizeof(*o));
  snprintf(o->name, sizeof o->name, "%s", q.name.c_str());
  o->kind = q.kind; o->R = q.R; o->S = q.S; o->O = q.O; o->I = q.I; o->KP = q.KP; o->offset = q.off; o->numel = q.numel;
  return OCTSEG_OK;
}
int octseg_plan_bn_info(const octseg_plan* p, int i, octseg_bn_info* o) {
  if (!p || !o || i < 0 || i >= (int)p->bns.size()) return fail(OCTSEG_BAD_ARG, "bn index out of range");
  const BNInfo& b = p->bns[i];
  memset(o, 0, sizeof(*o));
  snprintf(o->name, sizeof o->name, "%s", b.name.c_str());
  o->C = b.C; o->mean_offset = b.rm_off; o->var_offset = b.rv_off;
  return OCTSEG_OK;
}

int octseg_profile_start(void) {
  for (auto& r : g_prof) { g_prof_pool.push_back(r.a); g_prof_pool.push_back(r.b); }
  g_prof.clear();
  g_prof_on = true;
  return OCTSEG_OK;
}
// out[3*k + {0,1,2}] = {milliseconds, algorithmic FLOPs, launches} of class k = 0 fwd, 1 dgrad, 2 wgrad.
// Synchronises the device (bench / test use only).
int octseg_profile_stop(double* out) {
  g_prof_on = false;
  if (!out) return fail(OCTSEG_BAD_ARG, "null argument");
  HIPCHK(hipDeviceSynchronize());
  for (int i = 0; i < 12; ++i) out[i] = 0.0;
  FILE* dump = nullptr;
  if (const char* path = getenv("OCTSEG_PROFILE_DUMP")) dump = fopen(path, "w");
  if (dump) fprintf(dump, "layer,class,ms,gflop,tflops\n");
  for (auto& r : g_prof) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
    out[3 * r.kind] += ms; out[3 * r.kind + 1] += r.flops; out[3 * r.kind + 2] += 1.0;
    if (dump) fprintf(dump, "%s,%s,%.4f,%.3f,%.1f\n", r.name.c_str(), r.kind == 0 ? "fwd" : r.kind == 1 ? "dgrad" : r.kind == 2 ? "wgrad" : "hbm", ms,
                      r.flops / 1e9, ms > 0 ? r.flops / (ms * 1e-3) / 1e12 : 0.0);
  }
  if (dump) fclose(dump);
  for (auto& r : g_prof) { g_prof_pool.push_back(r.a); g_prof_pool.push_back(r.b); }
  g_prof.clear();
  return OCTSEG_OK;
}

// debug / test hook: byte offsets (inside the workspace) of a conv layer's raw output and its gradient
int octseg_plan_find_tensor(const octseg_plan* p, const char* conv_name, size_t* act_off, size_t* grad_off, int* dims) {
  if (!p || !conv_name) return fail(OCTSEG_BAD_ARG, "null argument");
  for (auto& L : p->convs)
    if (L.name == conv_name && L.out >= 0) {
      const TensorInfo& t = p->tensors[L.out];
      if (act_off) *act_off = t.off;
      if (grad_off) *grad_off = t.goff;
      if (dims) { dims[0] = t.N; dims[1] = t.H; dims[2] = t.W; dims[3] = t.C; }
      return OCTSEG_OK;
    }
  return fail(OCTSEG_BAD_ARG, std::string("no conv layer named ") + conv_name);
}

// The packed weight images in the workspace are reused until the caller says the parameters changed
// (optimizer step, load_state_dict); a fresh plan / another workspace or arena repacks by itself.
int octseg_plan_params_changed(octseg_plan* p) {
  if (!p) return fail(OCTSEG_BAD_ARG, "null argument");
  p->packed_valid = false;
  return OCTSEG_OK;
}

int octseg_net_forward(octseg_plan* p, const float* params, float* buffers, void* workspace, const float* image,
                       float* logits, int normalize, const float* mean, const float* stdv, int train, void* stream) {
  if (!p || !params || !buffers || !workspace || !image || !logits) return fail(OCTSEG_BAD_ARG, "null argument");
  if (normalize && (!mean || !stdv)) return fail(OCTSEG_BAD_ARG, "normalize=1 needs mean/std");
  if (train && p->dtype == OCTSEG_F16)
    return fail(OCTSEG_BAD_DTYPE, "f16 is a serving dtype (eval forwards, reference predict.py); train in bf16 or f32");
  Exec E{p, params, nullptr, buffers, (char*)workspace, (hipStream_t)stream, train};
  if (train || !p->graph_enabled) return run_forward(E, image, logits, normalize, mean, stdv);
  // ---- eval forward through a hipGraph
  octseg_plan::GraphKey key{params, buffers, workspace, image, logits, stream, normalize, {0, 0, 0}, {1, 1, 1}};
  if (normalize) for (int i = 0; i < 3; ++i) { key.mean[i] = mean[i]; key.stdv[i] = stdv[i]; }
  const bool same_key = key == p->graph_key;
  p->graph_key = key;
  // weight images are packed outside the graph (a replay never repacks; octseg_plan_params_changed brings us here)
  return graph_call(p, false, same_key, p->graph_exec, p->graph_seen, E.st, [&] { return pack_all_weights(E, true); },
                    [&] { return run_forward(E, image, logits, normalize, mean, stdv); });
}

// Eval-mode forwards of this plan are captured into a hipGraph and replayed while the argument set (pointers,
// stream, normalisation constants) stays the same.  Training calls are never captured.
int octseg_plan_set_graph(octseg_plan* p, int enable) {
  if (!p) return fail(OCTSEG_BAD_ARG, "null argument");
  p->graph_enabled = enable != 0;
  if (!enable && p->graph_exec) { (void)hipGraphExecDestroy(p->graph_exec); p->graph_exec = nullptr; p->graph_seen = 0; }
  return OCTSEG_OK;
}

// FPN's Dropout2d(0.2) (smp decoders/fpn: self.dropout after the merge): the keep pattern of the NEXT training forward(s), device float
// [B][128] of 0 / 1 (kept channels are scaled by 1 / (1 - p) as torch does).  The caller draws it (the reference's pattern comes from
// torch's global RNG and is not reproducible across implementations anyway); the backward reuses the same pointer.
int octseg_plan_set_dropout(octseg_plan* p, const float* keep_dev) {
  if (!p) return fail(OCTSEG_BAD_ARG, "null argument");
  p->dropout_keep = keep_dev;
  return OCTSEG_OK;
}

// Training-input augmentation on the GPU (dataset.py:160-207): see augment.hip.  img [B,3,H,W] f32 BGR 0..255, mask
// [B,classes,H,W] f32 0/1, params device f32 [B][OCTSEG_AUG_NPARAM]; outputs must not alias the inputs.
int octseg_augment(const float* img, const float* mask, float* img_out, float* mask_out, const float* params, int B, int classes, int H,
                   int W, void* stream) {
  if (!img || !mask || !img_out || !mask_out || !params) return fail(OCTSEG_BAD_ARG, "null argument");
  if (B <= 0 || classes <= 0 || H <= 0 || W <= 0) return fail(OCTSEG_BAD_SHAPE, "augment: empty batch or frame");
  if (img == img_out || mask == mask_out) return fail(OCTSEG_BAD_ARG, "augment: outputs must not alias the inputs (gather)");
  HIPCHK(launch_augment(img, mask, img_out, mask_out, params, B, classes, H, W, (hipStream_t)stream));
  return OCTSEG_OK;
}

// Serving epilogue of predict.py:92-100: sigmoid(logits[:, ch]) > 0.5, nearest resize (index tables: cv2 INTER_NEAREST) to out_h x out_w,
// written to channel out_ch of the NHWC mask stack out[N][out_h][out_w][out_channels] (f32 0/1).
int octseg_mask_assemble(const float* logits, int N, int classes, int H, int W, int ch, float* out, int out_h, int out_w,
                         int out_channels, int out_ch, const int* row_index, const int* col_index, void* stream) {
  if (!logits || !out) return fail(OCTSEG_BAD_ARG, "null argument");
  if (N <= 0 || classes <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || ch < 0 || ch >= classes || out_ch < 0 ||
      out_ch >= out_channels)
    return fail(OCTSEG_BAD_SHAPE, "mask_assemble: channel / extent out of range");
  HIPCHK(launch_mask_assemble(logits, N, classes, H, W, ch, out, out_h, out_w, out_channels, out_ch, row_index, col_index,
                              (hipStream_t)stream));
  return OCTSEG_OK;
}

// The input half of the pipeline (dataset.py:108-127, data/utils.py:159-166): see ingest.hip.  Enqueue only.
static int g_ingest_variant = 0;   // octseg_debug_set_ingest_variant
int octseg_debug_set_ingest_variant(int variant) {
  if (variant != 0 && variant != 1) return fail(OCTSEG_BAD_ARG, "ingest variant must be 0 (staged) or 1 (per-pixel gather)");
  g_ingest_variant = variant;
  return OCTSEG_OK;
}

int octseg_ingest_image(const uint8_t* src, int B, int src_h, int src_w, int swap_rb, float* out, int dst_h, int dst_w, const int* xtab,
                        const int* ytab, void* stream) {
  if (!src || !out || !xtab || !ytab) return fail(OCTSEG_BAD_ARG, "null argument");
  if (B <= 0 || src_h <= 0 || src_w <= 0 || dst_h <= 0 || dst_w <= 0) return fail(OCTSEG_BAD_SHAPE, "ingest_image: empty batch or frame");
  HIPCHK(launch_ingest_image(src, B, src_h, src_w, swap_rb != 0, out, dst_h, dst_w, xtab, ytab, g_ingest_variant, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_ingest_mask(const uint8_t* src, int B, int src_h, int src_w, int src_channels, const int* channel_ids, int C, float* out, int dst_h,
                       int dst_w, const int* row_index, const int* col_index, void* stream) {
  if (!src || !out || !channel_ids || !row_index || !col_index) return fail(OCTSEG_BAD_ARG, "null argument");
  if (B <= 0 || src_h <= 0 || src_w <= 0 || src_channels <= 0 || C <= 0 || dst_h <= 0 || dst_w <= 0)
    return fail(OCTSEG_BAD_SHAPE, "ingest_mask: empty batch, frame or class list");
  HIPCHK(launch_ingest_mask(src, B, src_h, src_w, src_channels, channel_ids, C, out, dst_h, dst_w, row_index, col_index, g_ingest_variant,
                            (hipStream_t)stream));
  return OCTSEG_OK;
}

// The output half of the pipeline (data/utils.py:195-235, models/smp/utils.py:203-213): see render.hip.  Enqueue only.
int octseg_render_results(const float* stack, const uint8_t* frames, int N, int H, int W, int stack_channels, const int* class_channels,
                          const uint8_t* class_rgb, int C, const uint8_t* alpha_table, int ring_alpha, int close_iterations, uint8_t* overlay,
                          uint8_t* color_mask, void* stream) {
  if (!stack || !frames || !class_channels || !class_rgb || !alpha_table || !overlay || !color_mask) return fail(OCTSEG_BAD_ARG, "null argument");
  if (N <= 0 || H <= 0 || W <= 0 || stack_channels <= 0 || C <= 0 || C > 16)
    return fail(OCTSEG_BAD_SHAPE, "render_results: empty batch or frame, or not 1..16 classes");
  if (close_iterations < 1 || close_iterations > 3) return fail(OCTSEG_BAD_SHAPE, "render_results: close_iterations must be 1, 2 or 3");
  HIPCHK(launch_render_results(stack, frames, N, H, W, stack_channels, class_channels, class_rgb, C, alpha_table, ring_alpha, close_iterations,
                               overlay, color_mask, (hipStream_t)stream));
  return OCTSEG_OK;
}

// The per-epoch sample dump of the training loop (models/smp/model.py:208-271): see panels.hip.  Enqueue only.
int octseg_epoch_panels(const float* frames, const float* logits, const uint8_t* gt, int N, int S, int C, int src_h, int src_w, int src_channels,
                        const int* row_index, const int* col_index, const int* gt_channels, const uint8_t* class_rgb, const uint8_t* class_ids,
                        uint8_t* panels, uint8_t* labels, void* stream) {
  if (!frames || !logits || !gt || !row_index || !col_index || !gt_channels || !class_rgb || !class_ids || !panels)
    return fail(OCTSEG_BAD_ARG, "null argument");
  if (N <= 0 || S <= 0 || C <= 0 || C > 16 || src_h <= 0 || src_w <= 0 || src_channels <= 0)
    return fail(OCTSEG_BAD_SHAPE, "epoch_panels: empty batch, frame or source, or not 1..16 classes");
  HIPCHK(launch_epoch_panels(frames, logits, gt, N, S, C, src_h, src_w, src_channels, row_index, col_index, gt_channels, class_rgb, class_ids,
                             panels, labels, (hipStream_t)stream));
  return OCTSEG_OK;
}

// The measurements of the app's get_analysis (app/tools/analysis.py:60-130,189,199-200): see measure.hip.  Enqueue only.
int octseg_stack_measure(const float* stack, int N, int H, int W, int stack_channels, const int* ray_pix, const int* ray_len, int R, int* counts,
                         int* radii, void* stream) {
  if (!stack || !ray_len || !counts || !radii || (!ray_pix && R != 0)) return fail(OCTSEG_BAD_ARG, "null argument");
  if (N <= 0 || H <= 0 || W <= 0 || stack_channels <= 0 || stack_channels > 16)
    return fail(OCTSEG_BAD_SHAPE, "stack_measure: empty batch or frame, or not 1..16 channels");
  if (R < 0) return fail(OCTSEG_BAD_SHAPE, "stack_measure: negative ray table length");
  if ((long long)H * W >= (1ll << 31)) return fail(OCTSEG_BAD_SHAPE, "stack_measure: H * W must be below 2^31");
  HIPCHK(launch_stack_measure(stack, N, H, W, stack_channels, ray_pix, ray_len, R, counts, radii, (hipStream_t)stream));
  return OCTSEG_OK;
}

// The polar plaque profile over the rays of calculate_object_thickness (app/tools/analysis.py:60-130): see polar.hip.  Enqueue only.
static int polar_args(const char* who, const void* in, int N, int H, int W, const int* ray_pix, const int* ray_len, int R, const void* out) {
  if (!in || !ray_len || !out || (!ray_pix && R != 0)) return fail(OCTSEG_BAD_ARG, std::string(who) + ": null argument");
  if (N <= 0 || H <= 0 || W <= 0) return fail(OCTSEG_BAD_ARG, std::string(who) + ": empty batch or frame");
  if (R < 0) return fail(OCTSEG_BAD_ARG, std::string(who) + ": negative ray table length");
  if ((long long)H * W >= (1ll << 31)) return fail(OCTSEG_BAD_ARG, std::string(who) + ": H * W must be below 2^31");
  return OCTSEG_OK;
}

int octseg_stack_polar(const float* stack, int N, int H, int W, int stack_channels, const int* ray_pix, const int* ray_len, int R, int* prof,
                       unsigned char* map, void* stream) {
  if (const int rc = polar_args("stack_polar", stack, N, H, W, ray_pix, ray_len, R, prof)) return rc;
  if (stack_channels <= 0 || stack_channels > 8) return fail(OCTSEG_BAD_ARG, "stack_polar: 1..8 channels (the label map keeps a bit per class in a byte)");
  HIPCHK(launch_stack_polar(stack, N, H, W, stack_channels, ray_pix, ray_len, R, prof, map, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_frames_unwrap(const unsigned char* frames, int N, int H, int W, int channels, const int* ray_pix, const int* ray_len, int R,
                         unsigned char* out, void* stream) {
  if (const int rc = polar_args("frames_unwrap", frames, N, H, W, ray_pix, ray_len, R, out)) return rc;
  if (channels != 1 && channels != 3) return fail(OCTSEG_BAD_ARG, "frames_unwrap: 1 or 3 channels");
  HIPCHK(launch_frames_unwrap(frames, N, H, W, channels, ray_pix, ray_len, R, out, (hipStream_t)stream));
  return OCTSEG_OK;
}

// Mask clean-up (data/mask_processor.py:5-37, run by process_pair, data/convert_int_to_cv.py:191-199): see components.hip.  Enqueue only.
static int components_args(const char* who, const void* stack, int N, int H, int W, int channels, const void* scratch, size_t scratch_bytes) {
  if (!stack || !scratch) return fail(OCTSEG_BAD_ARG, "null argument");
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, std::string(who) + ": scratch must be 8-byte aligned");
  if (N <= 0 || H <= 0 || W <= 0 || channels <= 0 || channels > 16)
    return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": empty batch or frame, or not 1..16 channels");
  if ((long long)H * W >= (1ll << 31) - 1) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": H * W must be below 2^31 - 1");
  if ((long long)N * channels >= (1ll << 31)) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": N * channels must be below 2^31");
  if (scratch_bytes < components_scratch_bytes((size_t)N * channels, H, W))
    return fail(OCTSEG_BAD_ARG, std::string(who) + ": scratch is smaller than octseg_components_scratch_bytes(N * channels, H, W)");
  return OCTSEG_OK;
}

size_t octseg_components_scratch_bytes(int planes, int H, int W) {
  if (planes <= 0 || H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31) - 1) return 0;
  return components_scratch_bytes((size_t)planes, H, W);
}

int octseg_stack_components(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, int* labels, int* ncomp,
                            int* top, void* stream) {
  if (const int rc = components_args("stack_components", stack, N, H, W, channels, scratch, scratch_bytes)) return rc;
  if (!labels && !ncomp && !top) return fail(OCTSEG_BAD_ARG, "stack_components: no output requested");
  HIPCHK(launch_stack_components(stack, N, H, W, channels, scratch, labels, ncomp, top, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_stack_cleanup(const float* stack, int N, int H, int W, int channels, int smooth_k, int keep, int min_area, int fill_holes, void* scratch,
                         size_t scratch_bytes, float* out, int* ncomp, int* top, void* stream) {
  if (!out) return fail(OCTSEG_BAD_ARG, "null argument");
  if (const int rc = components_args("stack_cleanup", stack, N, H, W, channels, scratch, scratch_bytes)) return rc;
  if (smooth_k < 0 || smooth_k > 7) return fail(OCTSEG_BAD_SHAPE, "stack_cleanup: smooth_k must be 0 (off) or 1..7 (frames whose short side is below 1600)");
  if (keep < 0 || min_area < 0) return fail(OCTSEG_BAD_ARG, "stack_cleanup: keep and min_area must not be negative");
  if (out == stack) return fail(OCTSEG_BAD_ARG, "stack_cleanup: the output must not alias the input");
  HIPCHK(launch_stack_cleanup(stack, N, H, W, channels, smooth_k, keep, min_area, fill_holes ? 1 : 0, scratch, out, ncomp, top, (hipStream_t)stream));
  return OCTSEG_OK;
}

// Raw pullback volumes (data/convert_dicoms.py:71-81, app/tools/analysis.py:167-177; data/utils.py:187): see volume.hip.  Enqueue only.
int octseg_volume_normalize(const void* src, int src_dtype, int S, int H, int W, int C, int swap_rb, unsigned* minmax, uint8_t* dst, void* stream) {
  if (!src || !minmax || !dst) return fail(OCTSEG_BAD_ARG, "null argument");
  if (src_dtype != 0 && src_dtype != 1) return fail(OCTSEG_BAD_DTYPE, "volume_normalize: src_dtype must be 0 (uint8) or 1 (uint16)");
  if (S <= 0 || H <= 0 || W <= 0) return fail(OCTSEG_BAD_SHAPE, "volume_normalize: empty volume or frame");
  if (C != 1 && C != 3) return fail(OCTSEG_BAD_SHAPE, "volume_normalize: 1 or 3 channels");
  if ((long long)H * W * C * (src_dtype ? 2 : 1) >= (1ll << 31) || (long long)H * W * 3 >= (1ll << 31))
    return fail(OCTSEG_BAD_SHAPE, "volume_normalize: a frame must stay below 2^31 bytes");
  if (src_dtype == 1 && ((uintptr_t)src & 1)) return fail(OCTSEG_BAD_ARG, "volume_normalize: a uint16 volume must be 2-byte aligned");
  HIPCHK(launch_volume_normalize(src, src_dtype, S, H, W, C, swap_rb != 0, minmax, dst, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_resize_pil_u8(const uint8_t* src, int S, int H, int W, int C, uint8_t* tmp, uint8_t* dst, int oh, int ow, const int* xbounds,
                         const int* xkk, int xksize, const int* ybounds, const int* ykk, int yksize, void* stream) {
  const bool horizontal = ow != W, vertical = oh != H;
  if (!src || !dst || (horizontal && vertical && !tmp)) return fail(OCTSEG_BAD_ARG, "null argument");
  if (S <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0) return fail(OCTSEG_BAD_SHAPE, "resize_pil_u8: empty batch or frame");
  if (C != 1 && C != 3) return fail(OCTSEG_BAD_SHAPE, "resize_pil_u8: 1 or 3 channels");
  if ((long long)H * W * C >= (1ll << 31) || (long long)H * ow * C >= (1ll << 31) || (long long)oh * ow * C >= (1ll << 31))
    return fail(OCTSEG_BAD_SHAPE, "resize_pil_u8: a frame must stay below 2^31 bytes");
  if ((horizontal && (!xbounds || !xkk)) || (vertical && (!ybounds || !ykk))) return fail(OCTSEG_BAD_ARG, "null table of a resampled axis");
  if ((horizontal && xksize <= 0) || (vertical && yksize <= 0)) return fail(OCTSEG_BAD_SHAPE, "resize_pil_u8: ksize of a resampled axis");
  HIPCHK(launch_resize_pil_u8(src, S, H, W, C, tmp, dst, oh, ow, xbounds, xkk, xksize, ybounds, ykk, yksize, (hipStream_t)stream));
  return OCTSEG_OK;
}

// ---------------------------------------------------------------- class activation maps (cam.hip)
// Which graphs the frozen-BatchNorm mode and the seeded backward are built for, and why not the others.
static int cam_supported(const octseg_plan* p) {
  const std::string& a = p->arch;
  if (p->dtype == OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, "f16 is a serving dtype: it has no backward, so no class activation maps");
  if (p->encoder.compare(0, 6, "resnet") != 0)
    return fail(OCTSEG_UNSUPPORTED_ARCH, "encoder '" + p->encoder + "' has no encoder.layer4 (the reference's target layer does not exist there either)");
  if (a == "pan" || a == "deeplabv3" || a == "deeplabv3plus")
    return fail(OCTSEG_UNSUPPORTED_ARCH, "arch '" + a + "': encoder.layer4 runs dilated, in a parity-re-arranged layout; its block output is not the reference's tensor" +
                                         (a == "pan" ? "" : ", and the graph holds a dropout op"));
  if (a == "fpn" || a == "pspnet")
    return fail(OCTSEG_UNSUPPORTED_ARCH, "arch '" + a + "': the graph holds a dropout op, which the frozen mode does not switch off" +
                                         (a == "pspnet" ? "; PSPNet never runs encoder.layer4" : ""));
  if (a != "unet" && a != "unetplusplus" && a != "linknet" && a != "manet")
    return fail(OCTSEG_UNSUPPORTED_ARCH, "arch '" + a + "' has no class-activation-map path");
  if (cam_target_op(p) < 0) return fail(OCTSEG_UNSUPPORTED_ARCH, "internal: no block output of encoder.layer4 in this graph");
  return OCTSEG_OK;
}

// Frozen-BatchNorm mode (the reference runs Grad-CAM on model.eval(), visualize_activation_maps.py:102): octseg_net_forward(train = 1) keeps the
// training op path -- unfolded weight images, saved activations and ReLU masks -- with every BatchNorm on its running statistics; no buffer is
// written.  The backward of such a forward is octseg_net_backward_seeded.
int octseg_plan_set_frozen_bn(octseg_plan* p, int on) {
  if (!p) return fail(OCTSEG_BAD_ARG, "null argument");
  if (on) { const int rc = cam_supported(p); if (rc) return rc; }
  p->frozen_bn = on != 0;
  return OCTSEG_OK;
}

// Workspace byte offsets of the OUTPUT of encoder.layer4's last block (after the residual add and the ReLU: the reference's target layer
// model.model.encoder.layer4[-1]) and of its gradient; dims = {N, h, w, K}.  NHWC, plan dtype.
int octseg_plan_cam_target(const octseg_plan* p, size_t* act_off, size_t* grad_off, int* dims) {
  if (!p) return fail(OCTSEG_BAD_ARG, "null argument");
  const int rc = cam_supported(p);
  if (rc) return rc;
  const TensorInfo& t = p->tensors[p->ops[cam_target_op(p)].out];
  if (act_off) *act_off = t.off;
  if (grad_off) *grad_off = t.goff;
  if (dims) { dims[0] = t.N; dims[1] = t.H; dims[2] = t.W; dims[3] = t.C; }
  return OCTSEG_OK;
}

// Backward of a frozen-mode forward from a caller-made dL/dlogits (NCHW f32 [B][classes][H][W]) down to the gradient of the CAM target
// tensor: data gradients and frozen-BatchNorm sweeps only -- no weight-, bias- or BatchNorm-parameter gradient is launched and no gradient
// arena is touched; the walk over the op list ends in front of the target's producer.
int octseg_net_backward_seeded(octseg_plan* p, const float* params, void* workspace, const float* dlogits, void* stream) {
  if (!p || !params || !workspace || !dlogits) return fail(OCTSEG_BAD_ARG, "null argument");
  if (!p->frozen_bn) return fail(OCTSEG_BAD_ARG, "octseg_net_backward_seeded needs a plan in frozen-BatchNorm mode (octseg_plan_set_frozen_bn)");
  Exec E{p, params, nullptr, nullptr, (char*)workspace, (hipStream_t)stream, 1};
  E.seed = dlogits; E.data_only = true; E.stop_op = cam_target_op(p);
  return run_backward(E, nullptr, nullptr, 1.f);
}

size_t octseg_cam_scratch_bytes(int N, int h, int w, int K) {
  if (N <= 0 || h <= 0 || w <= 0 || K <= 0) return 0;
  return cam_scratch_bytes(N, h, w, K);
}

int octseg_cam_maps(int dtype, const void* A, const void* G, int N, int h, int w, int K, int method, int S, void* scratch, float* maps,
                    float threshold, uint8_t* bin, const uint8_t* gt, int gt_h, int gt_w, const int* row_index, const int* col_index, int* counts,
                    const float* frames, const uint8_t* jet_bgr, double image_weight, uint8_t* overlay, void* stream) {
  if (!A || !G || !scratch || !maps) return fail(OCTSEG_BAD_ARG, "null argument");
  if (dtype != OCTSEG_F32 && dtype != OCTSEG_BF16) return fail(OCTSEG_BAD_DTYPE, "cam_maps: A and G are f32 or bf16 (f16 plans have no backward)");
  if (method < 0 || method > 5) return fail(OCTSEG_BAD_ARG, "cam_maps: method must be 0 GradCAM, 1 HiResCAM, 2 GradCAMElementWise, 3 GradCAMPlusPlus, 4 XGradCAM, 5 LayerCAM");
  if (N <= 0 || h <= 0 || w <= 0 || K <= 0 || K % 8 != 0 || S <= 0 || S > 16384 || (long long)h * w > (1ll << 24) || (long long)N * h * w >= (1ll << 31) ||
      (long long)N * K >= (1ll << 31))
    return fail(OCTSEG_BAD_SHAPE, "cam_maps: empty batch or map, K not a multiple of 8, or S outside 1..16384");
  if (counts && (!gt || !row_index || !col_index)) return fail(OCTSEG_BAD_ARG, "cam_maps: counts need the ground-truth plane and both index tables");
  if (counts && (gt_h <= 0 || gt_w <= 0 || (long long)gt_h * gt_w >= (1ll << 31))) return fail(OCTSEG_BAD_SHAPE, "cam_maps: empty or oversized ground truth");
  if (overlay && (!frames || !jet_bgr)) return fail(OCTSEG_BAD_ARG, "cam_maps: the overlay needs the frames and the colour table");
  if (overlay && !(image_weight >= 0.0 && image_weight <= 1.0)) return fail(OCTSEG_BAD_ARG, "cam_maps: image_weight must be in [0, 1]");
  CamArgs c;
  memset(&c, 0, sizeof(c));
  c.A = A; c.G = G; c.N = N; c.h = h; c.w = w; c.K = K; c.method = method; c.S = S; c.scratch = scratch; c.maps = maps;
  c.threshold = threshold; c.bin = bin; c.gt = gt; c.gt_h = gt_h; c.gt_w = gt_w; c.row_index = row_index; c.col_index = col_index; c.counts = counts;
  c.frames = frames; c.jet = jet_bgr; c.image_weight = image_weight; c.overlay = overlay;
  HIPCHK(launch_cam_maps(dtype, c, (hipStream_t)stream));
  return OCTSEG_OK;
}

// The overlay alone, of maps that exist already (CAMProcessor.overlay_activation_map): show_cam_on_image as in octseg_cam_maps, no rescaling.
int octseg_cam_overlay(const float* maps, const float* frames, const uint8_t* jet_bgr, int N, int S, double image_weight, uint8_t* overlay,
                       void* scratch, void* stream) {
  if (!maps || !frames || !jet_bgr || !overlay || !scratch) return fail(OCTSEG_BAD_ARG, "null argument");
  if (N <= 0 || S <= 0 || S > 16384) return fail(OCTSEG_BAD_SHAPE, "cam_overlay: empty batch, or S outside 1..16384");
  if (!(image_weight >= 0.0 && image_weight <= 1.0)) return fail(OCTSEG_BAD_ARG, "cam_overlay: image_weight must be in [0, 1]");
  HIPCHK(launch_cam_overlay(maps, frames, jet_bgr, N, S, image_weight, overlay, scratch, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_dice_forward(octseg_plan* p, void* workspace, const float* logits, const float* target, float* loss,
                        long long* stats, void* stream) {
  if (!p || !workspace || !logits || !target || !loss) return fail(OCTSEG_BAD_ARG, "null argument");
  DiceArgs a = dice_args(p, (char*)workspace, logits, target);
  a.stats = stats; a.loss = loss;
  HIPCHK(launch_dice_fwd(a, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_net_backward(octseg_plan* p, const float* params, float* grads, void* workspace, const float* logits,
                        const float* target, float grad_scale, void* stream) {
  if (!p || !params || !grads || !workspace || !logits || !target) return fail(OCTSEG_BAD_ARG, "null argument");
  if (p->dtype == OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, "f16 is a serving dtype: no backward");
  Exec E{p, params, grads, nullptr, (char*)workspace, (hipStream_t)stream, 1};
  return run_backward(E, logits, target, grad_scale);
}

// One training step's device work in one call: forward (batch statistics) + Dice (+ confusion counts) + backward -- what training_step
// and loss.backward() enqueue in the reference (src/models/smp/model.py:73-95, Lightning's automatic optimisation).  With
// octseg_plan_set_train_graph(plan, 1) the call is captured into a hipGraph (second call with an unchanged argument set) and replayed:
// the ~800 launches, the weight-gradient side stream, the forward lane and their event edges become ONE launch -- the host cost of a
// step drops from tens of milliseconds of enqueueing to microseconds, which is what small per-GPU batches (strong scaling) need.
// The replay runs the very launches of the eager call (weight images are repacked inside: the parameters change every step).
int octseg_net_train_step(octseg_plan* p, const float* params, float* grads, float* buffers, void* workspace, const float* image,
                          const float* target, float* logits, float* loss, long long* stats, int normalize, const float* mean,
                          const float* stdv, float grad_scale, void* stream) {
  if (!p || !params || !grads || !buffers || !workspace || !image || !target || !logits || !loss)
    return fail(OCTSEG_BAD_ARG, "null argument");
  if (normalize && (!mean || !stdv)) return fail(OCTSEG_BAD_ARG, "normalize=1 needs mean/std");
  if (p->dtype == OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, "f16 is a serving dtype (eval forwards, reference predict.py); train in bf16 or f32");
  hipStream_t st = (hipStream_t)stream;
  auto body = [&]() -> int {
    Exec Ef{p, params, nullptr, buffers, (char*)workspace, st, 1};
    int rc = run_forward(Ef, image, logits, normalize, mean, stdv);
    if (rc) return rc;
    DiceArgs a = dice_args(p, (char*)workspace, logits, target);
    a.stats = stats; a.loss = loss;
    HIPCHK(launch_dice_fwd(a, st));
    Exec Eb{p, params, grads, nullptr, (char*)workspace, st, 1};
    return run_backward(Eb, logits, target, grad_scale);
  };
  if (!p->tgraph_enabled || serial_mode()) return body();
  octseg_plan::TrainKey key{params, grads, buffers, workspace, image, target, logits, loss, stats, stream, p->dropout_keep, p->drop_connect,
                            normalize, {0, 0, 0}, {1, 1, 1}, grad_scale};
  if (normalize) for (int i = 0; i < 3; ++i) { key.mean[i] = mean[i]; key.stdv[i] = stdv[i]; }
  const bool same_key = key == p->tgraph_key;
  p->tgraph_key = key;
  return graph_call(p, true, same_key, p->tgraph_exec, p->tgraph_seen, st, [] { return (int)OCTSEG_OK; }, body);
}
// Loss behind octseg_dice_forward / the backward's dL/dlogits: smp DiceLoss (the reference, model.py:55), mean BCE-with-logits, or
// their sum.  A captured training step holds the old kind's kernels' arguments: drop it.
int octseg_plan_set_loss(octseg_plan* p, int kind) {
  if (!p) return fail(OCTSEG_BAD_ARG, "null argument");
  if (kind < LOSS_DICE || kind > LOSS_DICE_BCE) return fail(OCTSEG_BAD_ARG, "loss kind must be 0 (dice), 1 (bce) or 2 (dice + bce)");
  if (kind != p->loss_kind && p->tgraph_exec) { (void)hipGraphExecDestroy(p->tgraph_exec); p->tgraph_exec = nullptr; p->tgraph_seen = 0; }
  p->loss_kind = kind;
  return OCTSEG_OK;
}
// EfficientNet's drop_connect (efficientnet_pytorch.utils.drop_connect inside MBConvBlock.forward): the caller draws the per-sample keep
// decisions -- randomness stays with the caller, as with Dropout -- and hands over the FACTORS keep / (1 - rate).
int octseg_plan_set_drop_connect(octseg_plan* p, const float* factors_dev) {
  if (!p) return fail(OCTSEG_BAD_ARG, "null argument");
  p->drop_connect = factors_dev;
  return OCTSEG_OK;
}
int octseg_plan_num_drop_connect(const octseg_plan* p) { return p ? (int)p->dc_rates.size() : 0; }
float octseg_plan_drop_connect_rate(const octseg_plan* p, int i) { return (p && i >= 0 && i < (int)p->dc_rates.size()) ? p->dc_rates[i] : -1.f; }
int octseg_plan_set_train_graph(octseg_plan* p, int enable) {
  if (!p) return fail(OCTSEG_BAD_ARG, "null argument");
  p->tgraph_enabled = enable != 0;
  if (!enable && p->tgraph_exec) { (void)hipGraphExecDestroy(p->tgraph_exec); p->tgraph_exec = nullptr; p->tgraph_seen = 0; }
  return OCTSEG_OK;
}

// Data-parallel backward: the same launches as octseg_net_backward; the gradient arena is cut into `nslices` contiguous,
// parameter-aligned ranges and `cb(user, k, begin, end)` (element offsets) is called on the calling host thread as soon as the
// last launch that writes into slice k has been enqueued -- `comm_stream` has by then been made to wait for it, so a collective
// the callback enqueues on comm_stream runs beside the rest of the backward (reference: the bucketed, overlapped gradient
// all-reduce of torch DDP that Lightning sets up, src/models/smp/train.py:122-133).  Slices complete in backward order
// (head / decoder parameters first); every slice is reported exactly once.
int octseg_net_backward_sliced(octseg_plan* p, const float* params, float* grads, void* workspace, const float* logits,
                               const float* target, float grad_scale, void* stream, int nslices, void* comm_stream,
                               octseg_slice_cb cb, void* user) {
  if (!p || !params || !grads || !workspace || !logits || !target || !cb) return fail(OCTSEG_BAD_ARG, "null argument");
  if (nslices < 1 || nslices > 64) return fail(OCTSEG_BAD_ARG, "1 <= nslices <= 64 required");
  if (p->dtype == OCTSEG_F16) return fail(OCTSEG_BAD_DTYPE, "f16 is a serving dtype: no backward");
  if (!comm_stream || comm_stream == stream) return fail(OCTSEG_BAD_ARG, "comm_stream must be a stream of its own");
  Exec E{p, params, grads, nullptr, (char*)workspace, (hipStream_t)stream, 1};
  SliceCtx S;
  S.n = nslices; S.comm = (hipStream_t)comm_stream; S.cb = cb; S.user = user;
  return run_backward(E, logits, target, grad_scale, &S);
}

int octseg_optim_step(int kind, float* params, const float* grads, float* m, float* v, size_t numel, float lr,
                      float wd, int step, float grad_scale, void* stream) {
  if (!params || !grads) return fail(OCTSEG_BAD_ARG, "null argument");
  if (kind < 0 || kind > 3) return fail(OCTSEG_BAD_ARG, "optimizer kind must be 0..3");
  if ((kind == 1 || kind == 3) && (!m || !v)) return fail(OCTSEG_BAD_ARG, "Adam/RAdam need both state arenas");
  if (kind == 2 && !v) return fail(OCTSEG_BAD_ARG, "RMSprop needs the second-moment arena");
  OptArgs a;
  memset(&a, 0, sizeof(a));
  a.p = params; a.g = grads; a.m = m; a.v = v; a.n = numel; a.kind = kind; a.lr = lr; a.wd = wd;
  a.beta1 = 0.9f; a.beta2 = 0.999f; a.eps = 1e-8f; a.alpha = 0.99f; a.momentum = 0.f; a.step = step; a.grad_scale = grad_scale;
  HIPCHK(launch_optim_step(a, (hipStream_t)stream));
  return OCTSEG_OK;
}

// ---------------------------------------------------------------- single-op entry points
static unsigned long long* g_stamp = nullptr;
static bool g_serial = false;   // octseg_debug_set_serial: one stream, no lanes (isolated kernel durations)
// diagnostic builds only (-DOCTSEG_STAMP): device buffer of 6 u64 receiving the per-phase cycle sums
int octseg_debug_set_stamp(unsigned long long* dev_buf) { g_stamp = dev_buf; return OCTSEG_OK; }
int octseg_debug_set_serial(int on) { g_serial = on != 0; g_prof_hbm = g_serial; return OCTSEG_OK; }

size_t octseg_conv2d_scratch_bytes(int dtype, int N, int H, int W, int Cin, int Cout, int R, int S) {
  // upper bound over stride / transposed variants: both images use rows padded to <= 128 and K to <= 64 elements
  (void)N; (void)H; (void)W;
  const size_t esz = dtype_size(dtype);
  const size_t rows_f = ((size_t)Cout + 127) / 128 * 128, k_f = ((size_t)Cin + 63) / 64 * 64;
  const size_t rows_d = ((size_t)Cin + 127) / 128 * 128, k_d = ((size_t)Cout + 63) / 64 * 64;
  return align_up((size_t)R * S * rows_f * k_f * esz) + align_up((size_t)R * S * rows_d * k_d * esz);
}

int octseg_conv2d_forward(int dtype, const void* x, const float* w, const float* bias, void* y, int N, int H, int W,
                          int Cin, int Cout, int R, int S, int stride, int pad, int transposed, void* scratch, void* stream) {
  if (!geom_ok(dtype, Cin, Cout, R, S, stride, transposed)) return fail(OCTSEG_BAD_SHAPE, "unsupported conv geometry");
  hipStream_t st = (hipStream_t)stream;
  const Geom g = op_geom(N, H, W, Cin, Cout, R, S, stride, pad, transposed);
  std::vector<ConvArgs> la;
  fwd_launches(g, la);
  const ConvPackInfo pk = conv_pack_info(la[0], dtype);
  HIPCHK(launch_pack_weight_image(dtype, w, scratch, R * S, Cout, Cin, 0, pk, st));
  for (auto& a : la) {
    SrcDesc s; s.ptr = x; s.scale = nullptr; s.shift = nullptr; s.C = Cin; s.c0 = 0; s.H = H; s.W = W; s.up = 0; s.relu = 0;
    a.src[0] = s; a.nsrc = 1; a.W = scratch; a.bias = bias;
    if (!transposed) { a.Wmaster = w; a.wO = Cout; a.wI = Cin; a.wtrans = 0; }
    DstDesc d; d.ptr = y; d.C = Cout; d.c0 = 0; d.cn = Cout; d.H = g.OH; d.W = g.OW; d.accum = 0; d.pool = 0;
    a.dst[0] = d; a.ndst = 1; a.out_mode = OUT_STORE; a.stat_slab = nullptr; a.stamp = g_stamp;
    HIPCHK(launch_conv(dtype, a, st));
  }
  return OCTSEG_OK;
}

int octseg_conv2d_backward_data(int dtype, const void* dy, const float* w, void* dx, int N, int H, int W, int Cin,
                                int Cout, int R, int S, int stride, int pad, int transposed, void* scratch, void* stream) {
  const int v = ev_vec(dtype);
  if (!geom_ok(dtype, Cin, Cout, R, S, stride, transposed) || Cout % v != 0) return fail(OCTSEG_BAD_SHAPE, "unsupported conv geometry");
  hipStream_t st = (hipStream_t)stream;
  const size_t esz = dtype_size(dtype);
  const Geom g = op_geom(N, H, W, Cin, Cout, R, S, stride, pad, transposed);
  HIPCHK(hipMemsetAsync(dx, 0, (size_t)N * H * W * Cin * esz, st));
  std::vector<ConvArgs> ld;
  dgrad_launches(g, ld);
  ConvArgs d0 = ld[0];
  for (auto& d : ld) if (d.ntaps > 0) { d0 = d; break; }
  d0.Cin = Cout;
  const ConvPackInfo pk = conv_pack_info(d0, dtype);
  HIPCHK(launch_pack_weight_image(dtype, w, scratch, R * S, Cout, Cin, 1, pk, st));
  for (auto& a : ld) {
    SrcDesc s; s.ptr = dy; s.scale = nullptr; s.shift = nullptr; s.C = Cout; s.c0 = 0; s.H = g.OH; s.W = g.OW; s.up = 0; s.relu = 0;
    a.src[0] = s; a.nsrc = 1; a.Cin = Cout; a.W = scratch; a.bias = nullptr;
    if (!transposed) { a.Wmaster = w; a.wO = Cout; a.wI = Cin; a.wtrans = 1; }
    DstDesc d; d.ptr = dx; d.C = Cin; d.c0 = 0; d.cn = Cin; d.H = H; d.W = W; d.accum = 1; d.pool = 0;
    a.dst[0] = d; a.ndst = 1; a.out_mode = OUT_ACCUM; a.stat_slab = nullptr;
    HIPCHK(launch_conv(dtype, a, st));
  }
  return OCTSEG_OK;
}

int octseg_conv2d_backward_weight(int dtype, const void* x, const void* dy, float* dw, int N, int H, int W, int Cin,
                                  int Cout, int R, int S, int stride, int pad, int transposed, void* stream) {
  const int v = ev_vec(dtype);
  if (!geom_ok(dtype, Cin, Cout, R, S, stride, transposed) || Cout % v != 0) return fail(OCTSEG_BAD_SHAPE, "unsupported conv geometry");
  hipStream_t st = (hipStream_t)stream;
  const Geom g = op_geom(N, H, W, Cin, Cout, R, S, stride, pad, transposed);
  HIPCHK(hipMemsetAsync(dw, 0, (size_t)R * S * Cout * Cin * sizeof(float), st));
  std::vector<WgradArgs> lw;
  wgrad_launches(g, lw);
  for (auto& a : lw) {
    SrcDesc s; s.ptr = x; s.scale = nullptr; s.shift = nullptr; s.C = Cin; s.c0 = 0; s.H = H; s.W = W; s.up = 0; s.relu = 0;
    a.src[0] = s; a.nsrc = 1; a.dy = dy; a.dyC = Cout; a.dW = dw; a.stamp = g_stamp;
  }
  if (transposed && lw.size() == 4 && wgrad_convt16_eligible(lw[0], dtype)) {   // the plan's route for a ConvTranspose2d (conv_backward)
    HIPCHK(launch_wgrad_convt16(dtype, lw[0], st));
    return OCTSEG_OK;
  }
  for (auto& a : lw) HIPCHK(launch_wgrad(dtype, a, st));
  return OCTSEG_OK;
}

}  // extern "C"

bool octseg::detail::serial_mode() { return g_serial; }

int octseg::detail::cam_target_op(const octseg_plan* P) {
  int found = -1;
  for (int oi = 0; oi < (int)P->ops.size(); ++oi) {
    const Op& op = P->ops[oi];
    if (op.kind != OP_BN_ACT || op.y.bn < 0 || op.res.t < 0 || op.out < 0) continue;   // a residual block's output: relu(bn(y) + shortcut)
    if (P->bns[op.y.bn].name.compare(0, 15, "encoder.layer4.") == 0 && P->tensors[op.out].need_grad) found = oi;
  }
  return found;
}

static int g_deterministic = -1;   // -1: not decided yet (environment)
bool octseg::deterministic_mode() {
  if (g_deterministic < 0) g_deterministic = getenv("OCTSEG_DETERMINISTIC") != nullptr ? 1 : 0;
  return g_deterministic != 0;
}
extern "C" int octseg_set_deterministic(int on) { g_deterministic = on ? 1 : 0; return OCTSEG_OK; }
