// curves_api.cpp -- the C ABI of the logit histograms (curves.hip; no reference counterpart): argument checks in front of the
// launcher.  Enqueue only; every refusal happens before any HIP call, launches nothing and touches no output.
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

static_assert(OCTSEG_CURVE_BINS == CURVE_BINS, "the header's bin count is the kernel's");

extern "C" {

int octseg_logit_histogram(const float* logits, const float* target, int N, int classes, int H, int W, int* hist, void* stream) {
  if (!logits || !target || !hist) return fail(OCTSEG_BAD_ARG, "logit_histogram: null argument");
  if (N <= 0 || classes <= 0 || H <= 0 || W <= 0) return fail(OCTSEG_BAD_SHAPE, "logit_histogram: an extent is <= 0");
  if ((long long)H * W >= (1LL << 31)) return fail(OCTSEG_BAD_SHAPE, "logit_histogram: H * W >= 2^31");
  if ((long long)N * classes > 65535)
    return fail(OCTSEG_BAD_SHAPE, "logit_histogram: " + std::to_string((long long)N * classes) + " planes (N * classes), more than 65535 in one launch");
  HIPCHK(launch_logit_histogram(logits, target, N, classes, H, W, hist, (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
