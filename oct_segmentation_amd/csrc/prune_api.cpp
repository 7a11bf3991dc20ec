// prune_api.cpp -- the C ABI of the centreline pruning and census kernels (prune.hip; no reference counterpart): argument
// checks in front of the launcher.  Enqueue only; every refusal happens before anything is launched.
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

namespace {

constexpr int MAX_SIDE = 4096, MAX_CH = 16, MAX_STEPS = 8192;

// the census index plane * 9 + column stays in int32 on the host side of every caller
bool extents_ok(long long N, int H, int W, int channels) {
  return N > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE && channels > 0 && channels <= MAX_CH && N * channels * 9 < (1ll << 31);
}

}  // namespace

extern "C" {

size_t octseg_prune_scratch_bytes(int N, int H, int W, int channels) {
  if (!extents_ok(N, H, W, channels)) return 0;
  return prune_scratch_bytes((size_t)N, H, W, channels);
}

int octseg_stack_prune(const float* skel, int N, int H, int W, int channels, int spur, int trim, int flags, void* scratch, size_t scratch_bytes,
                       float* out, int* census, void* stream) {
  if (!skel || !scratch) return fail(OCTSEG_BAD_ARG, "null argument");
  if (!out && !census) return fail(OCTSEG_BAD_ARG, "stack_prune: out and census are both null, nothing to compute");
  if (out == skel) return fail(OCTSEG_BAD_ARG, "stack_prune: the output must not alias the input");
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, "stack_prune: scratch must be 8-byte aligned");
  if (flags & ~OCTSEG_PRUNE_GLOBAL) return fail(OCTSEG_BAD_ARG, "stack_prune: unknown flag bits (only OCTSEG_PRUNE_GLOBAL is defined)");
  if (spur < 0 || spur > MAX_STEPS || trim < 0 || trim > MAX_STEPS)
    return fail(OCTSEG_BAD_ARG, "stack_prune: spur and trim must lie in 0..8192");
  if (!extents_ok(N, H, W, channels))
    return fail(OCTSEG_BAD_SHAPE, "stack_prune: empty batch or frame, a side above 4096, not 1..16 channels, or N * channels * 9 not below 2^31");
  if (scratch_bytes < prune_scratch_bytes((size_t)N, H, W, channels))
    return fail(OCTSEG_BAD_ARG, "stack_prune: scratch is smaller than octseg_prune_scratch_bytes(N, H, W, channels)");
  HIPCHK(launch_stack_prune(skel, N, H, W, channels, spur, trim, flags & OCTSEG_PRUNE_GLOBAL, scratch, out, census, (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
