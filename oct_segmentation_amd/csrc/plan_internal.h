// plan_internal.h -- what the translation units behind the C ABI share: error reporting, the in-process profiling scope, launch
// geometry, the executor context and the entry points of the plan builder and the two executors.  Declarations only: every piece of
// state named here is defined in exactly one .cpp.
#pragma once
#include "plan.h"
#include "ev.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace octseg {
namespace detail __attribute__((visibility("hidden"))) {

// ---------------------------------------------------------------- error state (plan_forward.cpp; read by octseg_last_error)
extern thread_local std::string g_err;
int fail(int code, const std::string& msg);
#define HIPCHK(expr)                                                                      \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return fail(OCTSEG_HIP_ERROR, std::string(#expr) + ": " + hipGetErrorString(_e));   \
  } while (0)

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// ---------------------------------------------------------------- in-process kernel timing (state in plan_forward.cpp)
// bench.py brackets every MFMA launch with HIP events on the launch stream (octseg_profile_start /
// _stop); classes: 0 conv forward, 1 conv data-gradient, 2 weight gradient.
struct ProfRec { hipEvent_t a, b; int kind; double flops; std::string name; };
extern bool g_prof_on;
extern bool g_capturing;   // a stream capture is in progress on this thread's call: no timing events inside it
extern bool g_prof_hbm;    // set with octseg_debug_set_serial
extern std::vector<ProfRec> g_prof;
extern std::vector<hipEvent_t> g_prof_pool;
hipEvent_t prof_event();
struct ProfScope {
  hipStream_t st; ProfRec r; bool on;
  ProfScope(int kind, double flops, hipStream_t s, const std::string& name = std::string()) : st(s), on(g_prof_on && !g_capturing) {
    if (kind == 3 && !g_prof_hbm) on = false;   // the BatchNorm sweeps are only bracketed in the one-stream measurement pass
    if (!on) return;
    r.kind = kind; r.flops = flops; r.name = name; r.a = prof_event(); r.b = prof_event();
    if (!r.a || !r.b) { on = false; return; }
    (void)hipEventRecord(r.a, st);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(r.b, st);
    g_prof.push_back(r);
  }
};

// ---------------------------------------------------------------- tap tables / launch geometry (plan_geom.cpp)
struct Geom {
  int R, S, stride, pad;
  bool transposed;
  int N, IH, IW, Cin, OH, OW, Cout;
};
void fwd_launches(const Geom& g, std::vector<ConvArgs>& out);
void dgrad_launches(const Geom& g, std::vector<ConvArgs>& out);
void wgrad_launches(const Geom& g, std::vector<WgradArgs>& out);
void tied_dgrad_masked(const Geom& g, ConvArgs& a);
int tie_mask();
Geom tie_geom_up(const ConvLayer& L);
Geom tie_geom_skip(const ConvLayer& L);
// What decides whether a conv layer runs tied (ConvLayer::tie), what its four weight images look like and how they are packed: shared by
// the plan builder (plan_build.cpp) and the single-layer door (conv_api.cpp, octseg_tied_layer_op), so that the door builds what the plan builds.
struct TieQuery {
  int esz;                                   // element size of the plan's dtype
  bool transposed, stem, head, sliced, accum_out, has_bn, has_bias;
  int R, S, stride, pad, nsrc;
  bool up0_whole_grad;                       // source 0: nearest x2, the whole tensor (no channel slice), wants a gradient
  bool skips_plain_grad;                     // every further source: full resolution, whole, wants a gradient
  int Ca, Cs, Cout;                          // channels of source 0, of the others together, of the output
};
bool tie_eligible(const TieQuery& q);
struct TieImages {
  ConvPackInfo pk_fu, pk_du, pk_fs, pk_ds;   // forward up / data gradient up / forward skip / data gradient skip (the skip pair only with Cs > 0)
  bool du_masked;                            // the up slice's data gradient is ONE masked launch over dy's parity planes (9-tap image)
  int du_taps() const { return du_masked ? 9 : 16; }
};
TieImages tie_images(int dtype, const Geom& up, const Geom& skip);   // the Geoms of tie_geom_up / tie_geom_skip
struct TieOffsets { size_t fu, du, fs, ds; };                        // bytes, relative to the base launch_pack_all receives
// appends the layer's 2 (Cs == 0) or 4 jobs; w_off: the layer's 3x3 weight [9][Cout][Cin] in floats relative to the params base
void tie_pack_jobs(const TieImages& im, const TieOffsets& at, size_t w_off, int Cout, int Cin, int Ca, int Cs, std::vector<PackJob>& jobs,
                   std::vector<unsigned long long>& prefix, unsigned long long& total);
int side_wgs();   // split-K width of the multi-tap weight gradients on the side stream (plan_backward.cpp)
double layer_macs(const ConvLayer& L);
bool geom_ok(int dtype, int Cin, int Cout, int R, int S, int stride, int transposed);   // the single-op entry points (octseg_conv2d_*)
Geom op_geom(int N, int H, int W, int Cin, int Cout, int R, int S, int stride, int pad, int transposed);

// ---------------------------------------------------------------- executors (plan_forward.cpp, plan_backward.cpp)
bool serial_mode();   // octseg_debug_set_serial (api.cpp): one stream, no lanes
hipError_t create_side_stream(hipStream_t* st, bool backward = false);

struct Exec {
  octseg_plan* P;
  const float* params;
  float* grads;
  float* buffers;
  char* ws;
  hipStream_t st;
  int train;
  hipStream_t wst = nullptr;  // stream of the weight-gradient launches (side stream or st)
  // seeded data-only backward (octseg_net_backward_seeded): dL/dlogits comes from the caller, no weight / bias / BatchNorm parameter
  // gradient is launched (grads == nullptr) and the walk ends in front of op `stop_op` (the producer of the tensor whose gradient is wanted)
  const float* seed = nullptr;
  bool data_only = false;
  int stop_op = -1;
  std::vector<char> ginit;   // backward: has the gradient buffer of tensor t been written yet?
  // first contribution stores, later ones accumulate
  int claim(int t) { const int acc = ginit[t] ? 1 : 0; ginit[t] = 1; return acc; }

  void* act(int t) const { return ws + P->tensors[t].off; }
  void* grad(int t) const { return ws + P->tensors[t].goff; }
  float* ss(int bn) const { return (float*)(ws + P->bns[bn].ss_off); }
  float* bn_scale(int bn) const { return ss(bn); }
  float* bn_shift(int bn) const { return ss(bn) + P->bns[bn].C; }
  float* bn_mean(int bn) const { return ss(bn) + 2 * P->bns[bn].C; }
  float* bn_rstd(int bn) const { return ss(bn) + 3 * P->bns[bn].C; }
  float* bn_coef(int bn) const { return ss(bn) + 4 * P->bns[bn].C; }

  GnArgs gn_args(int gi) const {
    const GNInfo& g = P->gns[gi];
    const TensorInfo& t = P->tensors[g.y];
    GnArgs a;
    memset(&a, 0, sizeof(a));
    a.y = act(g.y);
    a.gamma = params + P->params[g.gamma].off; a.beta = params + P->params[g.beta].off;
    if (grads) { a.dgamma = grads + P->params[g.gamma].off; a.dbeta = grads + P->params[g.beta].off; }
    a.part = (float*)(ws + g.part_off); a.ss = (float*)(ws + g.ss_off); a.stat = (float*)(ws + g.stat_off); a.coef = (float*)(ws + g.coef_off);
    a.HW = (size_t)t.H * t.W; a.C = g.C; a.G = g.G; a.cpg = g.C / g.G; a.eps = 1e-5f;
    return a;
  }
  Geom geom(const ConvLayer& L) const {
    Geom g{L.R, L.S, L.stride, L.pad, L.transposed, L.N, L.IH, L.IW, L.Cin, L.OH, L.OW, L.Cout};
    if (L.stem) { g.R = g.S = 1; g.pad = 0; }
    return g;
  }
  int fill_srcs(const ConvLayer& L, SrcDesc* src) const {
    int c0 = 0, n = 0;
    for (auto& s : L.srcs) {
      const TensorInfo& t = P->tensors[s.v.t];
      SrcDesc d;
      d.ptr = (char*)act(s.v.t) + (size_t)s.c0 * dtype_size(P->dtype);          // (channel slice of a grouped conv: pointer offset,
      d.scale = s.v.bn >= 0 ? bn_scale(s.v.bn) + s.c0 : nullptr;                 //  the channel stride stays the tensor's)
      d.shift = s.v.bn >= 0 ? bn_shift(s.v.bn) + s.c0 : nullptr;
      d.C = t.C; d.c0 = c0; d.H = t.H; d.W = t.W; d.up = s.up; d.relu = s.v.bn >= 0 ? 1 : 0;
      src[n++] = d;
      c0 += s.cn ? s.cn : t.C;
    }
    return n;
  }
};

// Gradient-arena slices handed to the caller as soon as their last writer is enqueued (data-parallel overlap of the
// all-reduce with the rest of the backward, octseg_net_backward_sliced).
struct SliceCtx {
  int n = 0;
  hipStream_t comm = nullptr;
  octseg_slice_cb cb = nullptr;
  void* user = nullptr;
  std::vector<size_t> bounds;   // n + 1 element offsets into the arena, parameter-aligned, ascending
  std::vector<int> last_op;     // per slice: index of the op whose backward writes into it last (-1: nobody)
};

int build_plan(octseg_plan* P);                                                                                  // plan_build.cpp
int pack_all_weights(Exec& E, bool fold);                                                                        // plan_forward.cpp
int run_forward(Exec& E, const float* image, float* logits, int normalize, const float* mean, const float* stdv);
DiceArgs dice_args(const octseg_plan* P, char* ws, const float* logits, const float* target);                    // plan_backward.cpp
int run_backward(Exec& E, const float* logits, const float* target, float grad_scale, SliceCtx* S = nullptr);
int cam_target_op(const octseg_plan* P);   // api.cpp: index of the OP_BN_ACT that writes the output of encoder.layer4's last block, or -1

}  // namespace detail
}  // namespace octseg
