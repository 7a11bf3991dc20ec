// shape_api.cpp -- the C ABI of the lumen geometry (shape.hip; no reference counterpart): argument checks in front of the
// launchers.  Enqueue only; every refusal is OCTSEG_BAD_ARG, happens before any HIP call, launches nothing and touches no output.
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

static_assert(OCTSEG_MOMENT_FIELDS == SHAPE_MOMENT_FIELDS, "the header's field count is the kernel's");
static_assert(OCTSEG_SHAPE_MAX_EXTENT == SHAPE_MAX_EXTENT, "the header's extent bound is the kernel's");
// the largest second moment: fewer than 2^31 pixels, each at most (2^15 - 1)^2
static_assert((long long)(OCTSEG_SHAPE_MAX_EXTENT - 1) * (OCTSEG_SHAPE_MAX_EXTENT - 1) < (1ll << 30), "a pixel's x^2, xy, y^2 stay below 2^30");

static int shape_args(const char* who, const void* stack, int N, int H, int W, int channels, int max_channels) {
  if (!stack) return fail(OCTSEG_BAD_ARG, std::string(who) + ": null argument");
  if (N <= 0 || H <= 0 || W <= 0) return fail(OCTSEG_BAD_ARG, std::string(who) + ": empty batch or frame");
  if (channels <= 0 || channels > max_channels) return fail(OCTSEG_BAD_ARG, std::string(who) + ": 1.." + std::to_string(max_channels) + " channels");
  if (H > OCTSEG_SHAPE_MAX_EXTENT || W > OCTSEG_SHAPE_MAX_EXTENT) return fail(OCTSEG_BAD_ARG, std::string(who) + ": H and W must be at most 32768");
  if ((long long)H * W >= (1ll << 31)) return fail(OCTSEG_BAD_ARG, std::string(who) + ": H * W must be below 2^31");
  return OCTSEG_OK;
}

extern "C" {

int octseg_stack_moments(const float* stack, int N, int H, int W, int channels, long long* mom, void* stream) {
  if (const int rc = shape_args("stack_moments", stack, N, H, W, channels, 16)) return rc;
  if (!mom) return fail(OCTSEG_BAD_ARG, "stack_moments: null argument");
  if ((uintptr_t)mom & 7) return fail(OCTSEG_BAD_ARG, "stack_moments: mom must be 8-byte aligned");
  HIPCHK(launch_stack_moments(stack, N, H, W, channels, mom, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_moment_origins(const float* stack, const long long* mom, int N, int H, int W, int channels, int ref_channel, int* origins,
                          void* stream) {
  if (const int rc = shape_args("moment_origins", stack, N, H, W, channels, 16)) return rc;
  if (!mom || !origins) return fail(OCTSEG_BAD_ARG, "moment_origins: null argument");
  if ((uintptr_t)mom & 7) return fail(OCTSEG_BAD_ARG, "moment_origins: mom must be 8-byte aligned");
  if (ref_channel >= channels) return fail(OCTSEG_BAD_ARG, "moment_origins: ref_channel must be negative (own moments) or a channel of the stack");
  HIPCHK(launch_moment_origins(stack, mom, N, H, W, channels, ref_channel < 0 ? -1 : ref_channel, origins, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_stack_polar_at(const float* stack, int N, int H, int W, int channels, const int* origins, const int* ray_off, int R, int* prof,
                          int* len, void* stream) {
  if (const int rc = shape_args("stack_polar_at", stack, N, H, W, channels, 8)) return rc;
  if (!origins || !prof || !len || (!ray_off && R != 0)) return fail(OCTSEG_BAD_ARG, "stack_polar_at: null argument");
  if (R < 0) return fail(OCTSEG_BAD_ARG, "stack_polar_at: negative ray table length");
  HIPCHK(launch_stack_polar_at(stack, N, H, W, channels, origins, ray_off, R, prof, len, (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
