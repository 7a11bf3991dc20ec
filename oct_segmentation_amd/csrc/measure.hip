// measure.hip -- the per-pullback measurements of the reference's app on the GPU: what get_analysis (src/app/tools/analysis.py:133-250) takes from
// every mask -- the number of set pixels of a class (np.nonzero, analysis.py:199-200; presence, np.unique, analysis.py:189, follows from it) --
// and the ray walk of calculate_object_thickness (analysis.py:60-130).  The grouping into objects and the statistics are a few integers per
// slice and stay on the host (oct_segmentation_amd/analysis.py).
//
// Ray rule, restated.  From the centre (W / 2, H / 2) a ray per whole degree visits step r = 1, 2, ... at
// (int(cx + r * cos), int(cy + r * sin)) in CPython's double arithmetic; there is no step 0.  The device does no trigonometry:
// the host ships ray_pix[angle][r - 1] = y * W + x and ray_len[angle] = the number of leading steps inside the frame (leaving the frame ends a ray,
// found or not).  With v[r] = "the class is set at step r", r = 1 .. ray_len:
//   f = the first r with v[r] set; none: radius 0 (the reference's radii are >= 1, so 0 is free to mean "no object on this ray");
//   g = the first r > f with v[r] clear: radius g - 1; none: radius ray_len.
// A gap before the object is skipped, the first gap after it ends the ray.  Everything is integer: counts and radii EQUAL the reference's.
//
// count_kernel: one streaming pass.  A workgroup takes 4096 consecutive pixels of one slice, a lane one pixel at a time (one float4 where the
// stack has four channels and a 16-byte aligned base, dword loads otherwise), eight loads in flight; `v != 0` per channel is a ballot whose
// population count accumulates in scalar registers, so a wave needs no reduction of its own.  The four waves meet in LDS and the workgroup
// issues ONE integer atomic per channel into counts (cleared by the launcher).
//
// ray_kernel: one wave per (slice, angle).  Lanes take 64 consecutive steps; ONE gather of the pixel's channels serves the rays of every class
// at that angle; per class a ballot gives first-set / first-clear-after-it by bit operations; "found" is carried across the 64-step chunks as a
// bit per class, the result of class c lives in lane c; the wave leaves once every class is resolved or the ray ends.  The table entries of the
// next chunk are loaded before the gather of this one, so a chunk costs one memory round trip, not two.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace octseg {

namespace {

constexpr int NT = 256, WAVES = NT / 64;
constexpr int MAXC = 16;
constexpr int CNT_UNROLL = 8, CNT_ROUNDS = 2;
constexpr int CNT_PIX = NT * CNT_UNROLL * CNT_ROUNDS;   // pixels of a slice one workgroup counts
constexpr int ANGLES = 360;
static_assert(ANGLES % WAVES == 0, "the waves of a workgroup share a slice");

typedef unsigned long long u64;

}  // namespace

template <bool VEC>
__global__ __launch_bounds__(NT) void count_kernel(const float* __restrict__ stack, int N, int HW, int SC, int* __restrict__ counts) {
  __shared__ int part[WAVES][MAXC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = (int)(((long long)HW + CNT_PIX - 1) / CNT_PIX);
  const size_t total = (size_t)N * tiles;
  for (size_t t = blockIdx.x; t < total; t += gridDim.x) {
    const size_t n = t / tiles;
    const int p0 = (int)(t % tiles) * CNT_PIX;             // < HW < 2^31
    const float* base = stack + n * (size_t)HW * SC;
    int cnt[MAXC];                                          // wave-uniform
#pragma unroll
    for (int c = 0; c < MAXC; ++c) cnt[c] = 0;
#pragma unroll
    for (int round = 0; round < CNT_ROUNDS; ++round) {
      if (VEC) {
        // lanes past the slice's end load its last pixel and are masked out of the ballots: unconditional loads can be issued back to back
        float4 v[CNT_UNROLL];
#pragma unroll
        for (int k = 0; k < CNT_UNROLL; ++k) {
          const long long p = (long long)p0 + (round * CNT_UNROLL + k) * NT + tid;
          v[k] = *(const float4*)(base + (size_t)min(p, (long long)HW - 1) * 4);
        }
#pragma unroll
        for (int k = 0; k < CNT_UNROLL; ++k) {
          const bool ok = (long long)p0 + (round * CNT_UNROLL + k) * NT + tid < HW;
          cnt[0] += __popcll(__ballot(ok && v[k].x != 0.f));
          cnt[1] += __popcll(__ballot(ok && v[k].y != 0.f));
          cnt[2] += __popcll(__ballot(ok && v[k].z != 0.f));
          cnt[3] += __popcll(__ballot(ok && v[k].w != 0.f));
        }
      } else {
#pragma unroll
        for (int k = 0; k < CNT_UNROLL; ++k) {
          const long long p = (long long)p0 + (round * CNT_UNROLL + k) * NT + tid;
          const bool ok = p < HW;
          const float* px = base + (size_t)min(p, (long long)HW - 1) * SC;
#pragma unroll
          for (int c = 0; c < MAXC; ++c) {
            if (c < SC) cnt[c] += __popcll(__ballot(ok && px[c] != 0.f));      // wave-uniform
          }
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < SC) part[wave][c] = cnt[c];
    }
    __syncthreads();
    if (tid < SC) {
      int s = 0;
#pragma unroll
      for (int w = 0; w < WAVES; ++w) s += part[w][tid];
      if (s) atomicAdd(counts + n * SC + tid, s);
    }
    __syncthreads();   // the next tile of this workgroup overwrites part
  }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void ray_kernel(const float* __restrict__ stack, int N, int HW, int SC, const int* __restrict__ ray_pix,
                                                 const int* __restrict__ ray_len, int R, int* __restrict__ radii) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t total = (size_t)N * (ANGLES / WAVES);
  const unsigned all = SC >= 32 ? ~0u : ((1u << SC) - 1u);
  for (size_t t = blockIdx.x; t < total; t += gridDim.x) {
    const size_t n = t / (ANGLES / WAVES);
    const int angle = (int)(t % (ANGLES / WAVES)) * WAVES + wave;
    const int len = min(max(ray_len[angle], 0), R);
    const int* tab = ray_pix + (size_t)angle * R;
    const float* base = stack + n * (size_t)HW * SC;
    unsigned found = 0u, done = 0u;                         // a bit per class, wave-uniform
    int res = 0;                                            // lane c: radius of class c
    int pix_next = lane < len ? tab[lane] : 0;
    for (int r0 = 0; r0 < len && done != all; r0 += 64) {   // lane holds step r0 + lane + 1
      const bool valid = r0 + lane < len;
      const int pix = min(max(pix_next, 0), HW - 1);
      pix_next = tab[min(r0 + 64 + lane, len - 1)];         // unconditional and inside [0, len): nothing waits for it in this chunk
      const u64 vmask = __ballot(valid);
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      if (VEC) q = *(const float4*)(base + (size_t)pix * 4);   // lanes past the ray's end read a clamped pixel and are masked below
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        if (c < SC && !((done >> c) & 1u)) {                // wave-uniform
          float f;
          if (VEC) f = c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w;
          else f = base[(size_t)pix * SC + c];
          const u64 set = __ballot(valid && f != 0.f);
          u64 clear = ~set & vmask;
          bool inside = (found >> c) & 1u;                  // the object began in an earlier chunk
          if (!inside && set) {
            const int first = __ffsll((long long)set) - 1;  // 0..63
            found |= 1u << c;
            clear &= first == 63 ? 0ull : (~0ull << (first + 1));
            inside = true;
          }
          if (inside && clear) {                            // step g = r0 + lane_g + 1 is clear: radius g - 1
            const int g = __ffsll((long long)clear) - 1;
            if (lane == c) res = r0 + g;
            done |= 1u << c;
          }
        }
      }
    }
    if (lane < SC) {
      if (((found & ~done) >> lane) & 1u) res = len;        // the object reaches the end of the ray
      radii[(n * SC + lane) * ANGLES + angle] = res;
    }
  }
}

hipError_t launch_stack_measure(const float* stack, int N, int H, int W, int SC, const int* ray_pix, const int* ray_len, int R, int* counts,
                                int* radii, hipStream_t st) {
  const int HW = H * W;
  const bool vec = SC == 4 && ((uintptr_t)stack & 15) == 0;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * SC * sizeof(int), st);
  if (e != hipSuccess) return e;
  const size_t tiles = (size_t)N * (((size_t)HW + CNT_PIX - 1) / CNT_PIX);
  const dim3 gc((unsigned)std::min<size_t>(tiles, 1u << 20)), gr((unsigned)std::min<size_t>((size_t)N * (ANGLES / WAVES), 1u << 20));
  if (vec) {
    hipLaunchKernelGGL(count_kernel<true>, gc, dim3(NT), 0, st, stack, N, HW, SC, counts);
    hipLaunchKernelGGL(ray_kernel<true>, gr, dim3(NT), 0, st, stack, N, HW, SC, ray_pix, ray_len, R, radii);
  } else {
    hipLaunchKernelGGL(count_kernel<false>, gc, dim3(NT), 0, st, stack, N, HW, SC, counts);
    hipLaunchKernelGGL(ray_kernel<false>, gr, dim3(NT), 0, st, stack, N, HW, SC, ray_pix, ray_len, R, radii);
  }
  return hipGetLastError();
}

}  // namespace octseg
