// lesions_api.cpp -- the C ABI of the 3-D lesion kernels (lesions.hip; no reference counterpart): argument checks in front of
// the launchers.  Enqueue only; every refusal happens before any HIP call, launches nothing and touches no output.
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

namespace {

constexpr int MAX_CH = 16;

bool extents_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1ll << 31) - 1; }

int volume_args(const char* who, const void* stack, int N, int H, int W, int channels, int across, const void* scratch, size_t scratch_bytes) {
  if (!stack || !scratch) return fail(OCTSEG_BAD_ARG, "null argument");
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, std::string(who) + ": scratch must be 8-byte aligned");
  if (N <= 0 || H <= 0 || W <= 0 || channels <= 0 || channels > MAX_CH)
    return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": empty stack or frame, or not 1..16 channels");
  if (!extents_ok(N, H, W)) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": N * H * W must be below 2^31 - 1");
  if (across != OCTSEG_ACROSS_OVERLAP && across != OCTSEG_ACROSS_FULL)
    return fail(OCTSEG_BAD_ARG, std::string(who) + ": across must be OCTSEG_ACROSS_OVERLAP (0) or OCTSEG_ACROSS_FULL (1)");
  if (scratch_bytes < lesions_scratch_bytes((size_t)channels, N, H, W))
    return fail(OCTSEG_BAD_ARG, std::string(who) + ": scratch is smaller than octseg_lesions_scratch_bytes(channels, N, H, W)");
  return OCTSEG_OK;
}

}  // namespace

extern "C" {

size_t octseg_lesions_scratch_bytes(int channels, int N, int H, int W) {
  if (channels <= 0 || channels > MAX_CH || !extents_ok(N, H, W)) return 0;
  return lesions_scratch_bytes((size_t)channels, N, H, W);
}

int octseg_volume_components(const float* stack, int N, int H, int W, int channels, int across, void* scratch, size_t scratch_bytes, int* labels,
                             int* nles, int* top, int* profile, void* stream) {
  if (const int rc = volume_args("volume_components", stack, N, H, W, channels, across, scratch, scratch_bytes)) return rc;
  if (!labels && !nles && !top && !profile) return fail(OCTSEG_BAD_ARG, "volume_components: no output requested");
  HIPCHK(launch_volume_components(stack, N, H, W, channels, across == OCTSEG_ACROSS_FULL ? 1 : 0, scratch, labels, nles, top, profile,
                                  (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_volume_cleanup(const float* stack, int N, int H, int W, int channels, int across, int keep, int min_voxels, int min_slices, void* scratch,
                          size_t scratch_bytes, float* out, int* nles, int* top, void* stream) {
  if (!out) return fail(OCTSEG_BAD_ARG, "null argument");
  if (const int rc = volume_args("volume_cleanup", stack, N, H, W, channels, across, scratch, scratch_bytes)) return rc;
  if (keep < 0 || min_voxels < 0) return fail(OCTSEG_BAD_ARG, "volume_cleanup: keep and min_voxels must not be negative");
  if (min_slices < 1) return fail(OCTSEG_BAD_ARG, "volume_cleanup: min_slices must be at least 1");
  if (out == stack) return fail(OCTSEG_BAD_ARG, "volume_cleanup: the output must not alias the input");
  HIPCHK(launch_volume_cleanup(stack, N, H, W, channels, across == OCTSEG_ACROSS_FULL ? 1 : 0, keep, min_voxels, min_slices, scratch, out, nles, top,
                               (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
