// contours_api.cpp -- the C ABI of the mask outlines (contours.hip; no reference counterpart): argument checks in front of
// the launchers.  Enqueue only; every refusal happens before any HIP call, launches nothing and touches no output.
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

static_assert(OCTSEG_CONTOUR_FIELDS == CONTOUR_FIELDS, "the header's field count is the kernel's");

// the extents both calls take: an edge id ((y * (W + 1) + x) * 4 + dir) must fit 31 bits
static bool contour_extents_ok(long long planes, int H, int W) {
  if (planes <= 0 || H <= 0 || W <= 0 || planes >= (1ll << 31)) return false;
  if ((long long)H * W >= (1ll << 31) - 1) return false;
  if (((long long)H + 1) * ((long long)W + 1) >= OCTSEG_CONTOUR_MAX_VERTICES) return false;
  return planes * ((long long)H + 1) * ((long long)W / 64 + 1) < (1ll << 31);          // the vertex words of the call are counted in an int
}

static int contour_args(const char* who, const void* stack, int N, int H, int W, int channels) {
  if (!stack) return fail(OCTSEG_BAD_ARG, std::string(who) + ": null argument");
  if (N <= 0 || H <= 0 || W <= 0 || channels <= 0 || channels > 16)
    return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": empty batch or frame, or not 1..16 channels");
  if (!contour_extents_ok((long long)N * channels, H, W))
    return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": H * W must be below 2^31 - 1, (H + 1) * (W + 1) below 2^29, the call's vertex words below 2^31");
  return OCTSEG_OK;
}

static bool capacity_ok(long long c) { return c > 0 && c < (1ll << 31); }

extern "C" {

int octseg_stack_contour_counts(const float* stack, int N, int H, int W, int channels, long long* counts, void* stream) {
  if (!counts) return fail(OCTSEG_BAD_ARG, "stack_contour_counts: null argument");
  if (const int rc = contour_args("stack_contour_counts", stack, N, H, W, channels)) return rc;
  if ((uintptr_t)counts & 7) return fail(OCTSEG_BAD_ARG, "stack_contour_counts: counts must be 8-byte aligned");
  HIPCHK(launch_stack_contour_counts(stack, N, H, W, channels, counts, (hipStream_t)stream));
  return OCTSEG_OK;
}

size_t octseg_contours_scratch_bytes(int planes, int H, int W, long long edge_capacity) {
  if (!contour_extents_ok(planes, H, W) || !capacity_ok(edge_capacity)) return 0;
  return contours_scratch_bytes((size_t)planes, H, W, (size_t)edge_capacity);
}

int octseg_stack_contours(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, long long edge_capacity,
                          long long contour_capacity, long long vertex_capacity, int* ncont, int* table, int* vertices, int* overflow,
                          void* stream) {
  if (!scratch || !ncont || !table || !vertices || !overflow) return fail(OCTSEG_BAD_ARG, "stack_contours: null argument");
  if (const int rc = contour_args("stack_contours", stack, N, H, W, channels)) return rc;
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, "stack_contours: scratch must be 8-byte aligned");
  if (!capacity_ok(edge_capacity) || !capacity_ok(contour_capacity) || !capacity_ok(vertex_capacity))
    return fail(OCTSEG_BAD_ARG, "stack_contours: every capacity must be positive and below 2^31");
  if (scratch_bytes < contours_scratch_bytes((size_t)N * channels, H, W, (size_t)edge_capacity))
    return fail(OCTSEG_BAD_ARG, "stack_contours: scratch is smaller than octseg_contours_scratch_bytes(N * channels, H, W, edge_capacity)");
  HIPCHK(launch_stack_contours(stack, N, H, W, channels, scratch, (int)edge_capacity, (int)contour_capacity, (int)vertex_capacity, ncont, table,
                               vertices, overflow, (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
