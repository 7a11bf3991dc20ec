// vote_api.cpp -- the C ABI of the voted serving epilogue (vote.hip; no reference counterpart): argument checks in front of the
// launcher.  Enqueue only; every refusal happens before any HIP call, launches nothing and touches no output.
#include "plan_internal.h"

using namespace octseg;
using namespace octseg::detail;

static_assert(OCTSEG_VOTE_MAX_MEMBERS == VOTE_MAX_MEMBERS, "the header's member limit is the kernel argument's");

extern "C" {

int octseg_vote_assemble(const float* const* logits, const int* classes, const int* ch, const int* view, int M, int N, int H, int W, int mode,
                         float* out, int out_h, int out_w, int out_channels, int out_ch, const int* row_index, const int* col_index, float* prob,
                         uint8_t* dissent, int* stats, void* stream) {
  if (!logits || !classes || !ch || !view || !out) return fail(OCTSEG_BAD_ARG, "vote_assemble: null argument");
  if (M < 1 || M > OCTSEG_VOTE_MAX_MEMBERS)
    return fail(OCTSEG_BAD_SHAPE, "vote_assemble: " + std::to_string(M) + " members, not 1.." + std::to_string(OCTSEG_VOTE_MAX_MEMBERS));
  if (mode != OCTSEG_VOTE_SOFT && mode != OCTSEG_VOTE_MAJORITY) return fail(OCTSEG_BAD_ARG, "vote_assemble: mode must be 0 (soft) or 1 (majority)");
  if (N <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || out_channels <= 0) return fail(OCTSEG_BAD_SHAPE, "vote_assemble: an extent is <= 0");
  if (N > 65535 || (out_h + 15) / 16 > 65535) return fail(OCTSEG_BAD_SHAPE, "vote_assemble: more than 65535 frames or row tiles in one launch");
  if (out_ch < 0 || out_ch >= out_channels) return fail(OCTSEG_BAD_SHAPE, "vote_assemble: out_ch outside [0, out_channels)");
  VoteArgs a{};
  for (int m = 0; m < M; ++m) {
    const std::string who = "vote_assemble: member " + std::to_string(m);
    if (!logits[m]) return fail(OCTSEG_BAD_ARG, who + ": null logits");
    if (classes[m] <= 0 || ch[m] < 0 || ch[m] >= classes[m]) return fail(OCTSEG_BAD_SHAPE, who + ": channel outside [0, classes)");
    if (view[m] < 0 || view[m] > 7) return fail(OCTSEG_BAD_SHAPE, who + ": view code outside 0..7");
    if ((view[m] & 4) && H != W) return fail(OCTSEG_BAD_SHAPE, who + ": a transposed view needs H == W");
    a.z[m] = logits[m]; a.classes[m] = classes[m]; a.ch[m] = ch[m]; a.view[m] = view[m];
  }
  a.M = M; a.N = N; a.H = H; a.W = W; a.mode = mode;
  a.out = out; a.OH = out_h; a.OW = out_w; a.OC = out_channels; a.out_ch = out_ch;
  a.rows = row_index; a.cols = col_index;
  a.prob = prob; a.dissent = dissent; a.stats = stats;
  HIPCHK(launch_vote_assemble(a, (hipStream_t)stream));
  return OCTSEG_OK;
}

}  // extern "C"
