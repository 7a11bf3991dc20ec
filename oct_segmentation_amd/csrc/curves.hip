// curves.hip -- per frame and class, the histogram of the predicted probability over CURVE_BINS bins, once for the truth-negative and once for the
// truth-positive pixels (no reference counterpart: the reference scores at the one threshold 0.5).  From these integer
// counts tp / fp / fn / tn at every threshold k / 256 are suffix sums on the host (curves.py): ROC, precision-recall, reliability, the DSC-optimal cut.
//
// Rule per pixel: p = sigmoid_acc(z), bin = clamp((int)ceilf(p * 256.0f) - 1, 0, 255) (the product is by a power of two: exact), label = t != 0.
// Bin j holds p in (j / 256, (j + 1) / 256], p == 0 in bin 0; `bin >= k` is exactly `p > k / 256` in f32, at k = 128 the engine's `sigmoid_acc(z) > 0.5f`.
//
// Form: one pass, 8 bytes per pixel.  grid = (G chunks of a plane, N * classes planes), 512 threads = 8 waves.  A chunk is a multiple of 4 pixels;
// its first address decides the scalar head (a plane base (n * classes + c) * H * W floats is not 16-byte aligned when H * W % 4 != 0), then 16-byte
// loads, then a scalar tail; when the target's address is not congruent to the logits' the chunk is read with 4-byte loads throughout.
// Counting: a private [2][256] int table per wave in LDS.  On real logits most pixels land in bin 0 or bin 255, and LDS atomics of a whole wave on
// one address serialise; so the four hot cells (bin 0 / 255 x label) are counted with ballots in wave-uniform registers -- every loop below keeps
// all lanes active, a lane without a pixel votes false -- and only the other lanes go to LDS atomics.  Flush: the 512 threads sum the eight
// tables, one cell each, and issue one global atomicAdd per non-zero cell into the plane's row, which the launcher cleared on the stream.
// Integers only: exact and independent of the order.  G is chosen so that a launch has about TARGET_WGS workgroups (two per CU) and a workgroup
// at least MIN_CHUNK pixels: at 16 planes of 704 x 704 a workgroup takes 15488 pixels and issues at most 512 atomics (vote.hip's header records
// what workgroups that are too small cost in atomics).
#include <algorithm>
#include <cstdint>

#include "common.h"
#include "kernels.h"
#include "sigmoid.h"

namespace octseg {

namespace {
constexpr int NT = 512, WAVES = NT / 64;
constexpr int CELLS = 2 * CURVE_BINS;
constexpr int MIN_CHUNK = 4096;      // pixels: below this a plane is not split further
#ifndef CURVES_TARGET_WGS
#define CURVES_TARGET_WGS 512
#endif
constexpr int TARGET_WGS = CURVES_TARGET_WGS;
static_assert(NT == CELLS, "the flush gives every thread one cell");

struct Hot { int n0, n255, p0, p255; };   // wave-uniform: truth-negative / truth-positive pixels in bin 0 / bin 255

__device__ __forceinline__ void count(bool valid, float z, float t, int* tab, Hot& h) {
  const float p = sigmoid_acc(z);
  const int bin = min(max((int)ceilf(p * 256.0f) - 1, 0), CURVE_BINS - 1);
  const bool pos = t != 0.f;
  const bool lo = valid && bin == 0, hi = valid && bin == CURVE_BINS - 1;
  h.n0 += __popcll(__ballot(lo && !pos));
  h.p0 += __popcll(__ballot(lo && pos));
  h.n255 += __popcll(__ballot(hi && !pos));
  h.p255 += __popcll(__ballot(hi && pos));
  if (valid && !lo && !hi) atomicAdd(tab + (pos ? CURVE_BINS : 0) + bin, 1);
}
}  // namespace

__global__ __launch_bounds__(NT) void logit_histogram_kernel(const float* __restrict__ logits, const float* __restrict__ target, long long HW,
                                                             long long chunk, int* __restrict__ hist) {
  __shared__ int tabs[WAVES][CELLS];
  const int tid = threadIdx.x;
  const long long lo = (long long)blockIdx.x * chunk;
  if (lo >= HW) return;   // (uniform; the launcher's G leaves no such workgroup, kept as the bound of everything below)
  const long long len = min(chunk, HW - lo);
  const size_t plane = blockIdx.y;
  const float* z = logits + plane * (size_t)HW + lo;
  const float* t = target + plane * (size_t)HW + lo;
  for (int i = tid; i < WAVES * CELLS; i += NT) (&tabs[0][0])[i] = 0;
  __syncthreads();
  int* tab = tabs[tid >> 6];
  Hot h{0, 0, 0, 0};
  // scalar head up to the first 16-byte boundary of the logits; 16-byte loads only if the target is aligned there too (uniform)
  long long head = min((long long)((16 - ((uintptr_t)z & 15)) & 15) / 4, len);
  if ((((uintptr_t)(t + head)) & 15) != 0) head = len;
  const long long n4 = (len - head) / 4, tail0 = head + 4 * n4;
  for (long long b = 0; b < head; b += NT) {
    const bool v = b + tid < head;
    const long long i = v ? b + tid : 0;
    count(v, z[i], t[i], tab, h);
  }
  const float4* z4 = (const float4*)(z + head);
  const float4* t4 = (const float4*)(t + head);
  for (long long b = 0; b < n4; b += 2 * NT) {   // two 16-byte loads per array in flight per lane; a lane past the end rereads the last one
    const long long i0 = b + tid, i1 = i0 + NT;
    const bool v0 = i0 < n4, v1 = i1 < n4;
    const float4 za = z4[v0 ? i0 : n4 - 1], ta = t4[v0 ? i0 : n4 - 1], zb = z4[v1 ? i1 : n4 - 1], tb = t4[v1 ? i1 : n4 - 1];
    count(v0, za.x, ta.x, tab, h); count(v0, za.y, ta.y, tab, h); count(v0, za.z, ta.z, tab, h); count(v0, za.w, ta.w, tab, h);
    count(v1, zb.x, tb.x, tab, h); count(v1, zb.y, tb.y, tab, h); count(v1, zb.z, tb.z, tab, h); count(v1, zb.w, tb.w, tab, h);
  }
  {   // tail: at most 3 pixels
    const bool v = tail0 + tid < len;
    const long long i = v ? tail0 + tid : 0;
    count(v, z[i], t[i], tab, h);
  }
  if ((tid & 63) == 0) {   // the wave's hot cells join its table
    atomicAdd(tab + 0, h.n0); atomicAdd(tab + CURVE_BINS - 1, h.n255);
    atomicAdd(tab + CURVE_BINS, h.p0); atomicAdd(tab + CELLS - 1, h.p255);
  }
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) s += tabs[w][tid];
  if (s) atomicAdd(hist + plane * CELLS + tid, s);
}

hipError_t launch_logit_histogram(const float* logits, const float* target, int N, int classes, int H, int W, int* hist, hipStream_t st) {
  const long long HW = (long long)H * W;
  const int planes = N * classes;
  const hipError_t e = hipMemsetAsync(hist, 0, (size_t)planes * CELLS * sizeof(int), st);
  if (e != hipSuccess) return e;
  const long long want = std::min<long long>((HW + MIN_CHUNK - 1) / MIN_CHUNK, std::max(1, TARGET_WGS / planes));
  const long long chunk = ((HW + want - 1) / want + 3) & ~3LL;      // a multiple of 4: every chunk of a plane has the alignment of its first
  const long long G = (HW + chunk - 1) / chunk;
  hipLaunchKernelGGL(logit_histogram_kernel, dim3((unsigned)G, (unsigned)planes), dim3(NT), 0, st, logits, target, HW, chunk, hist);
  return hipGetLastError();
}

}  // namespace octseg
