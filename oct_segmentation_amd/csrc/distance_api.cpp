// distance_api.cpp -- the C ABI of the boundary-distance kernels (distance.hip; no reference counterpart): argument checks in
// front of the launchers.  Enqueue only; every refusal happens before anything is launched.
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

namespace {

constexpr int MAX_SIDE = 4096, MAX_CH = 16;

bool extents_ok(long long N, int H, int W) { return N > 0 && H > 0 && W > 0 && H <= MAX_SIDE && W <= MAX_SIDE; }

int stack_args(const char* who, const void* stack, int N, int H, int W, int channels, const void* scratch, size_t scratch_bytes) {
  if (!stack || !scratch) return fail(OCTSEG_BAD_ARG, "null argument");
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, std::string(who) + ": scratch must be 8-byte aligned");
  if (!extents_ok(N, H, W)) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": empty batch or frame, or a side above 4096 (squared distances stay below 2^25)");
  if (channels <= 0 || channels > MAX_CH) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": not 1..16 channels");
  if (scratch_bytes < distance_scratch_bytes((size_t)N, H, W, channels, 0, 0))
    return fail(OCTSEG_BAD_ARG, std::string(who) + ": scratch is smaller than octseg_distance_scratch_bytes(N, H, W, channels, 0, 0)");
  return OCTSEG_OK;
}

int pair_args(const char* who, const void* src, const void* dst, int N, int H, int W, int ca, int cb, const void* pairs, int npairs, int src_part,
              int dst_part, const void* scratch, size_t scratch_bytes) {
  if (!src || !dst || !pairs || !scratch) return fail(OCTSEG_BAD_ARG, "null argument");
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, std::string(who) + ": scratch must be 8-byte aligned");
  if (!extents_ok(N, H, W)) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": empty batch or frame, or a side above 4096 (squared distances stay below 2^25)");
  if (ca <= 0 || ca > MAX_CH || cb <= 0 || cb > MAX_CH) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": not 1..16 channels");
  if (npairs <= 0 || (long long)N * npairs >= (1ll << 31)) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": no pair, or N * pairs not below 2^31");
  if (src_part < 0 || src_part > 2 || dst_part < 0 || dst_part > 2) return fail(OCTSEG_BAD_ARG, std::string(who) + ": a part must be 0 (set), 1 (clear) or 2 (boundary)");
  if (scratch_bytes < distance_scratch_bytes((size_t)N, H, W, ca, cb, npairs))
    return fail(OCTSEG_BAD_ARG, std::string(who) + ": scratch is smaller than octseg_distance_scratch_bytes(N, H, W, channels_a, channels_b, pairs)");
  return OCTSEG_OK;
}

}  // namespace

extern "C" {

size_t octseg_distance_scratch_bytes(int N, int H, int W, int channels_a, int channels_b, int pairs) {
  if (!extents_ok(N, H, W) || channels_a <= 0 || channels_a > MAX_CH || channels_b < 0 || channels_b > MAX_CH || pairs < 0) return 0;
  return distance_scratch_bytes((size_t)N, H, W, channels_a, channels_b, pairs);
}

int octseg_stack_boundary(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, float* out, void* stream) {
  if (!out) return fail(OCTSEG_BAD_ARG, "null argument");
  if (const int rc = stack_args("stack_boundary", stack, N, H, W, channels, scratch, scratch_bytes)) return rc;
  if (out == stack) return fail(OCTSEG_BAD_ARG, "stack_boundary: the output must not alias the input");
  HIPCHK(launch_stack_boundary(stack, N, H, W, channels, scratch, out, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_stack_distance(const float* stack, int N, int H, int W, int channels, int to, void* scratch, size_t scratch_bytes, int* d2, void* stream) {
  if (!d2) return fail(OCTSEG_BAD_ARG, "null argument");
  if (const int rc = stack_args("stack_distance", stack, N, H, W, channels, scratch, scratch_bytes)) return rc;
  if (to < 0 || to > 2) return fail(OCTSEG_BAD_ARG, "stack_distance: to must be 0 (set), 1 (clear) or 2 (boundary)");
  HIPCHK(launch_stack_distance(stack, N, H, W, channels, to, scratch, d2, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_pair_distance_counts(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs, int npairs,
                                int src_part, int dst_part, void* scratch, size_t scratch_bytes, int* counts, int* overlap, void* stream) {
  if (!counts) return fail(OCTSEG_BAD_ARG, "null argument");
  if (const int rc = pair_args("pair_distance_counts", src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, scratch, scratch_bytes))
    return rc;
  HIPCHK(launch_pair_distance_counts(src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, scratch, counts, overlap,
                                     (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_pair_distance_keys(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs, int npairs,
                              int src_part, int dst_part, void* scratch, size_t scratch_bytes, long long first_segment, const long long* offsets,
                              long long* keys, long long capacity, int* overflow, void* stream) {
  if (!offsets || !keys || !overflow) return fail(OCTSEG_BAD_ARG, "null argument");
  if (const int rc = pair_args("pair_distance_keys", src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, scratch, scratch_bytes))
    return rc;
  if (capacity <= 0) return fail(OCTSEG_BAD_ARG, "pair_distance_keys: the key buffer has no capacity");
  if (first_segment < 0 || first_segment + (long long)N * npairs > (1ll << 31))
    return fail(OCTSEG_BAD_SHAPE, "pair_distance_keys: segment numbers must stay below 2^31");
  HIPCHK(launch_pair_distance_query(src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, scratch, first_segment, offsets, keys,
                                    capacity, overflow, nullptr, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_pair_distance_min(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs, int npairs,
                             int src_part, int dst_part, void* scratch, size_t scratch_bytes, unsigned long long* out, void* stream) {
  if (!out) return fail(OCTSEG_BAD_ARG, "null argument");
  if (const int rc = pair_args("pair_distance_min", src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, scratch, scratch_bytes))
    return rc;
  HIPCHK(launch_pair_distance_query(src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, scratch, 0, nullptr, nullptr, 0, nullptr,
                                    out, (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
