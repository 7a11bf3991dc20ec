// lesions_internal.h -- what lesions.hip (one labelled volume per channel) and match.hip (two of them at once) share: the carved scratch of one
// labelling, the launch sequence that labels and ranks a stack, the extents pass, and the in-wave reductions of the per-run kernels.  The
// definitions stand in lesions.hip; DESIGN.md sections 5j and 5o.
#pragma once

#include "bitplanes.h"

namespace octseg {

namespace {

constexpr int TOPL = 32, LCOL = 8;        // the table: voxels, first_voxel, z0, z1, y0, y1, x0, x1

// all 64 lanes of a wave take these together
__device__ __forceinline__ int wave_sum(int v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o); return v; }
__device__ __forceinline__ int wave_min(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ int wave_max(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }

}  // namespace

// the arrays of one labelling: parent / vox / zmax int32 [C][N * H * W], list int32 [C][cap], nroots / thr int32 [C], rank int32 [C][32] (the
// ranked roots, -1 = none), a = the stack's bit planes, b = the kept bits (the clean-up only; may be null otherwise)
struct VScratch {
  int *parent, *vox, *zmax, *list, *nroots, *thr, *rank;
  u64 *a, *b;
  int cap;
  size_t bytes;
};

// the most components a volume holds under either rule: N * ceil(H / 2) * ceil(W / 2)
inline int lesion_capacity(int N, int H, int W) { return (int)((size_t)N * (((size_t)H + 1) / 2) * (((size_t)W + 1) / 2)); }

// pack and label; with `rank` also count and select (the threshold, the count and the ranking; nles int32 [C] and top int32 [C][32][8] optional)
hipError_t label_and_rank(const float* stack, const BitGeo& g, int C, int full, bool rank, int keep, int min_voxels, int min_slices, const VScratch& s,
                          int* nles, int* top, hipStream_t st);
// the bounding boxes into top (columns 4..7) and the per-slice profile int32 [C][32][N] (cleared here), each where the pointer is not null
hipError_t volume_extents(const BitGeo& g, int C, const VScratch& s, int* top, int* profile, hipStream_t st);

}  // namespace octseg
