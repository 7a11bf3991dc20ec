// match_api.cpp -- the C ABI of the lesion matching (match.hip; no reference counterpart): argument checks in front of the
// launcher.  Enqueue only; every refusal happens before any HIP call, launches nothing and touches no output.  The refusals and their codes are
// those of octseg_volume_components (lesions_api.cpp).
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

namespace {

constexpr int MAX_CH = 16;

bool extents_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && (long long)N * H * W < (1ll << 31) - 1; }

}  // namespace

extern "C" {

size_t octseg_match_scratch_bytes(int channels, int N, int H, int W) {
  if (channels <= 0 || channels > MAX_CH || !extents_ok(N, H, W)) return 0;
  return match_scratch_bytes((size_t)channels, N, H, W);
}

int octseg_volume_match(const float* pred, const float* truth, int N, int H, int W, int channels, int across, void* scratch, size_t scratch_bytes,
                        int* nles, int* top, int* overlap, int* frames, void* stream) {
  if (!pred) return fail(OCTSEG_BAD_ARG, "volume_match: null pred");
  if (!truth) return fail(OCTSEG_BAD_ARG, "volume_match: null truth");
  if (!scratch) return fail(OCTSEG_BAD_ARG, "volume_match: null scratch");
  if (!nles) return fail(OCTSEG_BAD_ARG, "volume_match: null nles");
  if (!overlap) return fail(OCTSEG_BAD_ARG, "volume_match: null overlap");
  if ((uintptr_t)scratch & 7) return fail(OCTSEG_BAD_ARG, "volume_match: scratch must be 8-byte aligned");
  if (N <= 0 || H <= 0 || W <= 0 || channels <= 0 || channels > MAX_CH)
    return fail(OCTSEG_BAD_SHAPE, "volume_match: empty stack or frame, or not 1..16 channels");
  if (!extents_ok(N, H, W)) return fail(OCTSEG_BAD_SHAPE, "volume_match: N * H * W must be below 2^31 - 1");
  if (across != OCTSEG_ACROSS_OVERLAP && across != OCTSEG_ACROSS_FULL)
    return fail(OCTSEG_BAD_ARG, "volume_match: across must be OCTSEG_ACROSS_OVERLAP (0) or OCTSEG_ACROSS_FULL (1)");
  if (scratch_bytes < match_scratch_bytes((size_t)channels, N, H, W))
    return fail(OCTSEG_BAD_ARG, "volume_match: scratch is smaller than octseg_match_scratch_bytes(channels, N, H, W)");
  HIPCHK(launch_volume_match(pred, truth, N, H, W, channels, across == OCTSEG_ACROSS_FULL ? 1 : 0, scratch, nles, top, overlap, frames,
                             (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
