// distance_api.cpp -- the C ABI of the boundary-distance kernels (distance.hip; no reference counterpart): argument checks in
// front of the launchers.  Enqueue only; every refusal happens before anything is launched.  The volume calls (section 5p) and the signed maps with
// their blend (section 5s) follow in sections of their own.
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

// ---- the volume calls
namespace {

constexpr int MAX_SPAN = 32767;

// what every volume call checks; step < 0: the call takes no slice_step.  *rows (may be null: a call without a distance map) = the band's rows
int volume_args(const char* who, int N, int H, int W, int ca, int cb, int npairs, int step, const void* scratch, size_t scratch_bytes, int* rows) {
  const std::string w(who);
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, w + ": scratch must be 8-byte aligned");
  if (!extents_ok(N, H, W)) return fail(OCTSEG_BAD_SHAPE, w + ": empty volume or frame, or a side above 4096 (in-slice squared distances stay below 2^25)");
  if (ca <= 0 || ca > MAX_CH || cb < 0 || cb > MAX_CH) return fail(OCTSEG_BAD_SHAPE, w + ": not 1..16 channels");
  if ((long long)N * H * W > (1ll << 32)) return fail(OCTSEG_BAD_ARG, w + ": N * H * W above 2^32 (the packed minimum holds the voxel index in 32 bits)");
  if (step >= 0 && (step < 1 || (long long)step * (N - 1) > MAX_SPAN))
    return fail(OCTSEG_BAD_ARG, w + ": slice_step must be an integer >= 1 with slice_step * (N - 1) <= 32767 (squared distances stay below 2^30 + 2^25)");
  if (!rows) {
    const size_t need = volume_distance_scratch_bytes((size_t)N, H, W, ca, cb, npairs, 0);
    if (scratch_bytes < need)
      return fail(OCTSEG_BAD_ARG, w + ": scratch is smaller than the " + std::to_string(need) +
                                      " bytes of octseg_volume_distance_scratch_bytes(N, H, W, channels_a, channels_b, pairs, 0)");
    return OCTSEG_OK;
  }
  *rows = volume_distance_rows(scratch_bytes, (size_t)N, H, W, ca, cb, npairs);
  if (*rows < 1)
    return fail(OCTSEG_BAD_ARG, w + ": scratch is smaller than the " + std::to_string(volume_distance_scratch_bytes((size_t)N, H, W, ca, cb, npairs, 1)) +
                                    " bytes a band of one row needs (octseg_volume_distance_scratch_bytes(N, H, W, channels_a, channels_b, pairs, 1))");
  return OCTSEG_OK;
}

int volume_pair_args(const char* who, const void* src, const void* dst, int N, int H, int W, int ca, int cb, const void* pairs, int npairs, int src_part,
                     int dst_part, int step, const void* scratch, size_t scratch_bytes, int* rows) {
  if (!src || !dst || !pairs || !scratch) return fail(OCTSEG_BAD_ARG, "null argument");
  if (cb <= 0) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": not 1..16 channels");
  if (npairs <= 0 || (long long)N * npairs >= (1ll << 31)) return fail(OCTSEG_BAD_SHAPE, std::string(who) + ": no pair, or N * pairs not below 2^31");
  if (src_part < 0 || src_part > 2 || dst_part < 0 || dst_part > 2) return fail(OCTSEG_BAD_ARG, std::string(who) + ": a part must be 0 (set), 1 (clear) or 2 (boundary)");
  return volume_args(who, N, H, W, ca, cb, npairs, step, scratch, scratch_bytes, rows);
}

}  // namespace

extern "C" {

size_t octseg_volume_distance_scratch_bytes(int N, int H, int W, int channels_a, int channels_b, int pairs, int rows) {
  if (!extents_ok(N, H, W) || channels_a <= 0 || channels_a > MAX_CH || channels_b < 0 || channels_b > MAX_CH || pairs < 0 || rows < 0 || rows > H ||
      (long long)N * H * W > (1ll << 32) || (long long)N * pairs >= (1ll << 31))
    return 0;
  return volume_distance_scratch_bytes((size_t)N, H, W, channels_a, channels_b, pairs, rows);
}

int octseg_volume_boundary(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, float* out, void* stream) {
  if (!stack || !scratch || !out) return fail(OCTSEG_BAD_ARG, "null argument");
  if (const int rc = volume_args("volume_boundary", N, H, W, channels, 0, 0, -1, scratch, scratch_bytes, nullptr)) return rc;
  if (out == stack) return fail(OCTSEG_BAD_ARG, "volume_boundary: the output must not alias the input");
  HIPCHK(launch_volume_boundary(stack, N, H, W, channels, scratch, out, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_volume_distance(const float* stack, int N, int H, int W, int channels, int to, int slice_step, void* scratch, size_t scratch_bytes, int* d2,
                           void* stream) {
  if (!stack || !scratch || !d2) return fail(OCTSEG_BAD_ARG, "null argument");
  if (to < 0 || to > 2) return fail(OCTSEG_BAD_ARG, "volume_distance: to must be 0 (set), 1 (clear) or 2 (boundary)");
  int rows = 0;
  if (const int rc = volume_args("volume_distance", N, H, W, channels, 0, 0, std::max(slice_step, 0), scratch, scratch_bytes, &rows)) return rc;
  HIPCHK(launch_volume_distance(stack, N, H, W, channels, to, slice_step, rows, scratch, d2, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_volume_pair_distance_counts(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs,
                                       int npairs, int src_part, int dst_part, void* scratch, size_t scratch_bytes, long long* counts,
                                       long long* overlap, void* stream) {
  if (!counts) return fail(OCTSEG_BAD_ARG, "null argument");
  if (const int rc = volume_pair_args("volume_pair_distance_counts", src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, -1,
                                      scratch, scratch_bytes, nullptr))
    return rc;
  HIPCHK(launch_volume_pair_counts(src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, scratch, counts, overlap,
                                   (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_volume_pair_distance_keys(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs,
                                     int npairs, int src_part, int dst_part, int slice_step, void* scratch, size_t scratch_bytes,
                                     long long first_segment, const long long* offsets, long long* keys, long long capacity, int* overflow,
                                     void* stream) {
  if (!offsets || !keys || !overflow) return fail(OCTSEG_BAD_ARG, "null argument");
  if (capacity <= 0) return fail(OCTSEG_BAD_ARG, "volume_pair_distance_keys: the key buffer has no capacity");
  if (first_segment < 0 || first_segment + (long long)npairs > (1ll << 31))
    return fail(OCTSEG_BAD_SHAPE, "volume_pair_distance_keys: segment numbers must stay below 2^31");
  int rows = 0;
  if (const int rc = volume_pair_args("volume_pair_distance_keys", src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part,
                                      std::max(slice_step, 0), scratch, scratch_bytes, &rows))
    return rc;
  HIPCHK(launch_volume_pair_query(src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, slice_step, rows, scratch, first_segment,
                                  offsets, keys, capacity, overflow, nullptr, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_volume_pair_distance_min(const float* src, const float* dst, int N, int H, int W, int channels_a, int channels_b, const int* pairs, int npairs,
                                    int src_part, int dst_part, int slice_step, void* scratch, size_t scratch_bytes, unsigned long long* out,
                                    void* stream) {
  if (!out) return fail(OCTSEG_BAD_ARG, "null argument");
  int rows = 0;
  if (const int rc = volume_pair_args("volume_pair_distance_min", src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part,
                                      std::max(slice_step, 0), scratch, scratch_bytes, &rows))
    return rc;
  HIPCHK(launch_volume_pair_query(src, dst, N, H, W, channels_a, channels_b, pairs, npairs, src_part, dst_part, slice_step, rows, scratch, 0, nullptr,
                                  nullptr, 0, nullptr, out, (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"

// ---- signed maps and their blend
extern "C" {

size_t octseg_signed_distance_scratch_bytes(int N, int H, int W, int channels) {
  if (!extents_ok(N, H, W) || channels <= 0 || channels > MAX_CH) return 0;
  return signed_distance_scratch_bytes((size_t)N, H, W, channels);
}

int octseg_stack_signed_distance(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, int* sd2, void* stream) {
  if (!stack || !scratch || !sd2) return fail(OCTSEG_BAD_ARG, "null argument");
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, "stack_signed_distance: scratch must be 8-byte aligned");
  if (!extents_ok(N, H, W))
    return fail(OCTSEG_BAD_SHAPE, "stack_signed_distance: empty batch or frame, or a side above 4096 (squared distances stay below 2^25)");
  if (channels <= 0 || channels > MAX_CH) return fail(OCTSEG_BAD_SHAPE, "stack_signed_distance: not 1..16 channels");
  if (scratch_bytes < signed_distance_scratch_bytes((size_t)N, H, W, channels))
    return fail(OCTSEG_BAD_ARG, "stack_signed_distance: scratch is smaller than octseg_signed_distance_scratch_bytes(N, H, W, channels)");
  if ((const void*)sd2 == (const void*)stack) return fail(OCTSEG_BAD_ARG, "stack_signed_distance: the output must not alias the input");
  HIPCHK(launch_stack_signed_distance(stack, N, H, W, channels, scratch, sd2, (hipStream_t)stream));
  return OCTSEG_OK;
}

int octseg_signed_blend(const int* sd2, int K, int H, int W, int channels, const int* plan, int M, float* out, int N_out, int* made, void* stream) {
  if (!sd2 || !plan || !out) return fail(OCTSEG_BAD_ARG, "null argument");
  if (!extents_ok(K, H, W) || N_out <= 0)
    return fail(OCTSEG_BAD_SHAPE, "signed_blend: no key slice, no output slice or an empty frame, or a side above 4096");
  if (channels <= 0 || channels > MAX_CH) return fail(OCTSEG_BAD_SHAPE, "signed_blend: not 1..16 channels");
  if (M <= 0) return fail(OCTSEG_BAD_SHAPE, "signed_blend: a plan of no rows");
  if ((const void*)out == (const void*)sd2) return fail(OCTSEG_BAD_ARG, "signed_blend: the output must not alias the maps");
  HIPCHK(launch_signed_blend(sd2, K, H, W, channels, plan, M, out, N_out, made, (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
