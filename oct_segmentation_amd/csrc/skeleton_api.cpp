// skeleton_api.cpp -- the C ABI of the thinning and census kernels (skeleton.hip; no reference counterpart): argument checks in
// front of the launcher.  Enqueue only; every refusal happens before anything is launched.
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

namespace {

constexpr int MAX_SIDE = 4096, MAX_CH = 16;

// the census index plane * 6 + column stays in int32 on the host side of every caller
bool extents_ok(long long N, int H, int W, int channels) {
  return N > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE && channels > 0 && channels <= MAX_CH && N * channels * 6 < (1ll << 31);
}

}  // namespace

extern "C" {

size_t octseg_skeleton_scratch_bytes(int N, int H, int W, int channels) {
  if (!extents_ok(N, H, W, channels)) return 0;
  return skeleton_scratch_bytes((size_t)N, H, W, channels);
}

int octseg_stack_skeleton(const float* stack, int N, int H, int W, int channels, int flags, void* scratch, size_t scratch_bytes, float* out,
                          int* census, void* stream) {
  if (!stack || !scratch) return fail(OCTSEG_BAD_ARG, "null argument");
  if (!out && !census) return fail(OCTSEG_BAD_ARG, "stack_skeleton: out and census are both null, nothing to compute");
  if (out == stack) return fail(OCTSEG_BAD_ARG, "stack_skeleton: the output must not alias the input");
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, "stack_skeleton: scratch must be 8-byte aligned");
  if (flags & ~OCTSEG_SKEL_GLOBAL) return fail(OCTSEG_BAD_ARG, "stack_skeleton: unknown flag bits (only OCTSEG_SKEL_GLOBAL is defined)");
  if (!extents_ok(N, H, W, channels))
    return fail(OCTSEG_BAD_SHAPE, "stack_skeleton: empty batch or frame, a side above 4096, not 1..16 channels, or N * channels * 6 not below 2^31");
  if (scratch_bytes < skeleton_scratch_bytes((size_t)N, H, W, channels))
    return fail(OCTSEG_BAD_ARG, "stack_skeleton: scratch is smaller than octseg_skeleton_scratch_bytes(N, H, W, channels)");
  HIPCHK(launch_stack_skeleton(stack, N, H, W, channels, flags & OCTSEG_SKEL_GLOBAL, scratch, out, census, (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
