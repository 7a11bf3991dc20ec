// volume.hip -- the arithmetic between a catheter's pixel array and the nets: what the reference does to every slice of a DICOM volume before
// anything else sees it (src/data/convert_dicoms.py:71-81, again in src/app/tools/analysis.py:167-177),
//   cv2.normalize(slice, None, 0, 255, NORM_MINMAX, CV_8U) + cv2.cvtColor(BGR2RGB),
// and the Image.resize(output_size) of data_processing (src/data/utils.py:187), Pillow's default BICUBIC on 8-bit frames.
//
// minmax_kernel: per-slice minimum and maximum over ALL channels (minMaxIdx on a multi-channel Mat without an index request).  A workgroup
// takes 64 KiB of one slice: 16-byte loads between the first and the last 16-byte boundary inside its range, the bytes in front of and behind
// them one element per lane.  Samples are compared two to a register as packed 16-bit lanes (a byte quad is split into its even and odd
// bytes first); a wave-64 shuffle reduction, the four waves meet in LDS, and ONE integer atomicMin / atomicMax per workgroup lands in
// minmax[slice][0 / 1], which minmax_init_kernel set to (0xffffffff, 0) in the same call.  No workgroup waits for another.
//
// normalize_kernel: reads that pair on the device.  Per slice, in double as cv::normalize does,
//   scale = 255 * (smax - smin > DBL_EPSILON ? 1 / (smax - smin) : 0),  shift = 0 - smin * scale,  a = (float)scale,  b = (float)shift,
// per sample dst = saturate_cast<uchar>(x * a + b) as OpenCV's baseline convertTo computes it: the product and the sum each rounded to
// float32 by themselves (no fused multiply-add), rint to nearest even, clamp to 0..255.  A lane takes eight consecutive pixels of the flat
// [S * H * W] pixel list (a group may straddle a slice seam; a and b follow the pixel), loads and stores them as whole 8- or 16-byte words
// where both bases allow it, and writes three channels: reversed with swap_rb, the one channel of a grey volume three times.
//
// resample_kernel: ONE pass of Pillow's 8-bit ImagingResample along one axis from the host's tables (oct_segmentation_amd/pullback.py:
// precompute_coeffs + normalize_coeffs_8bpc): per output index a first source index and a tap count (bounds) and up to ksize int32
// coefficients at 22 fractional bits (kk).  ss = (1 << 21) + sum(src * k) in 32-bit arithmetic, out = clamp(ss >> 22, 0, 255) with an
// arithmetic shift -- bicubic taps overshoot, the clamp is live.  resample_taps serves both passes: horizontally the taps are C bytes apart,
// vertically a row.  Bounds outside the source are clamped, never followed.  The horizontal pass runs first, as in Pillow, into a uint8
// intermediate; a pass whose output length equals its input length is skipped, as Pillow skips it.
#include <algorithm>
#include <cfloat>

#include "common.h"
#include "kernels.h"

namespace octseg {

namespace {

constexpr int NT = 256, WAVES = NT / 64;
constexpr int MM_TILE = NT * 16 * 16;     // bytes of a slice one workgroup scans: 16 rounds of one 16-byte load per lane
constexpr int NORM_PIX = 8;               // pixels a lane normalises
constexpr unsigned MAX_GRID = 1u << 20;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ us2 as_us2(unsigned w) { return __builtin_bit_cast(us2, w); }

template <class T>
__device__ __forceinline__ void minmax_word(unsigned w, us2& lo, us2& hi) {
  if (sizeof(T) == 1) {
    const us2 e = as_us2(w & 0x00ff00ffu), o = as_us2((w >> 8) & 0x00ff00ffu);
    lo = __builtin_elementwise_min(lo, __builtin_elementwise_min(e, o));
    hi = __builtin_elementwise_max(hi, __builtin_elementwise_max(e, o));
  } else {
    lo = __builtin_elementwise_min(lo, as_us2(w));
    hi = __builtin_elementwise_max(hi, as_us2(w));
  }
}

}  // namespace

__global__ __launch_bounds__(NT) void minmax_init_kernel(unsigned* __restrict__ minmax, int S) {
  const int s = blockIdx.x * NT + threadIdx.x;
  if (s < S) { minmax[2 * s] = 0xffffffffu; minmax[2 * s + 1] = 0u; }
}

template <class T>
__global__ __launch_bounds__(NT) void minmax_kernel(const T* __restrict__ src, int S, int frame_bytes, unsigned* __restrict__ minmax) {
  __shared__ unsigned part[WAVES][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles = (int)(((long long)frame_bytes + MM_TILE - 1) / MM_TILE);
  const size_t total = (size_t)S * tiles;
  for (size_t t = blockIdx.x; t < total; t += gridDim.x) {
    const size_t s = t / tiles;
    const long long b0 = (long long)(t % tiles) * MM_TILE, b1 = std::min<long long>(b0 + MM_TILE, frame_bytes);
    const uintptr_t a0 = (uintptr_t)src + s * (size_t)frame_bytes + (size_t)b0, a1 = a0 + (size_t)(b1 - b0);
    const uintptr_t v0 = std::min<uintptr_t>((a0 + 15) & ~(uintptr_t)15, a1), v1 = std::max<uintptr_t>(a1 & ~(uintptr_t)15, v0);
    us2 plo = as_us2(0xffffffffu), phi = as_us2(0u);
    const int nvec = (int)((v1 - v0) >> 4);               // <= MM_TILE / 16
    const uint4* vp = (const uint4*)v0;
#pragma unroll 4
    for (int i = tid; i < nvec; i += NT) {
      const uint4 q = vp[i];
      minmax_word<T>(q.x, plo, phi); minmax_word<T>(q.y, plo, phi); minmax_word<T>(q.z, plo, phi); minmax_word<T>(q.w, plo, phi);
    }
    unsigned lo = std::min<unsigned>(plo.x, plo.y), hi = std::max<unsigned>(phi.x, phi.y);
    // fewer than 16 bytes on either side of the vectors: [a0, v0) and [v1, a1), one element per lane
    if (tid < (int)((v0 - a0) / sizeof(T))) { const unsigned x = ((const T*)a0)[tid]; lo = std::min(lo, x); hi = std::max(hi, x); }
    if (tid < (int)((a1 - v1) / sizeof(T))) { const unsigned x = ((const T*)v1)[tid]; lo = std::min(lo, x); hi = std::max(hi, x); }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      lo = std::min(lo, (unsigned)__shfl_xor((int)lo, d, 64));
      hi = std::max(hi, (unsigned)__shfl_xor((int)hi, d, 64));
    }
    if (lane == 0) { part[wave][0] = lo; part[wave][1] = hi; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
      for (int w = 1; w < WAVES; ++w) { lo = std::min(lo, part[w][0]); hi = std::max(hi, part[w][1]); }
      atomicMin(minmax + 2 * s, lo);
      atomicMax(minmax + 2 * s + 1, hi);
    }
    __syncthreads();   // the next tile of this workgroup overwrites part
  }
}

namespace {

// cv::normalize's scale and shift of one slice (double), handed to convertTo as floats
__device__ __forceinline__ void slice_ab(const unsigned* __restrict__ minmax, size_t s, float& a, float& b) {
#pragma clang fp contract(off)
  const double smin = (double)minmax[2 * s], smax = (double)minmax[2 * s + 1];
  const double d = smax - smin;
  const double scale = 255.0 * (d > DBL_EPSILON ? 1.0 / d : 0.0);
  const double shift = 0.0 - smin * scale;
  a = (float)scale;
  b = (float)shift;
}

__device__ __forceinline__ uint8_t convert_u8(float x, float a, float b) {
#pragma clang fp contract(off)
  // written out under the pragma: __fmul_rn / __fadd_rn are plain operators in headers compiled with contraction on, and fuse once inlined
  const float m = x * a;
  const float r = __builtin_rintf(m + b);                             // round half to even
  return (uint8_t)(int)fminf(fmaxf(r, 0.f), 255.f);
}

}  // namespace

// VEC: src is 16-byte and dst 8-byte aligned, so the full groups of eight pixels move as whole words
template <class T, int C, bool VEC>
__global__ __launch_bounds__(NT) void normalize_kernel(const T* __restrict__ src, const unsigned* __restrict__ minmax, size_t total, int HW,
                                                       int swap_rb, uint8_t* __restrict__ dst) {
  constexpr int IN_ALIGN = (NORM_PIX * C * (int)sizeof(T)) % 16 == 0 ? 16 : 8;
  const size_t groups = (total + NORM_PIX - 1) / NORM_PIX;
  for (size_t g = (size_t)blockIdx.x * NT + threadIdx.x; g < groups; g += (size_t)gridDim.x * NT) {
    const size_t p0 = g * NORM_PIX;
    const int n = (int)std::min<size_t>(NORM_PIX, total - p0);
    const bool whole = VEC && n == NORM_PIX;
    T in[NORM_PIX * C];
    uint8_t out[NORM_PIX * 3];
    if (whole) {
      __builtin_memcpy(in, __builtin_assume_aligned(src + p0 * C, IN_ALIGN), sizeof(in));
    } else {
#pragma unroll
      for (int k = 0; k < NORM_PIX * C; ++k) in[k] = k < n * C ? src[p0 * C + k] : (T)0;
    }
    size_t s = p0 / (size_t)HW;
    int rem = (int)(p0 - s * (size_t)HW);
    float a, b;
    slice_ab(minmax, s, a, b);
#pragma unroll
    for (int k = 0; k < NORM_PIX; ++k) {
      if (k < n) {
        while (rem >= HW) { rem -= HW; ++s; slice_ab(minmax, s, a, b); }    // the group crossed into the next slice
        ++rem;
      }
      if (C == 1) {
        out[3 * k] = out[3 * k + 1] = out[3 * k + 2] = convert_u8((float)in[k], a, b);
      } else {
        const uint8_t c0 = convert_u8((float)in[3 * k], a, b), c2 = convert_u8((float)in[3 * k + 2], a, b);
        out[3 * k] = swap_rb ? c2 : c0;
        out[3 * k + 1] = convert_u8((float)in[3 * k + 1], a, b);
        out[3 * k + 2] = swap_rb ? c0 : c2;
      }
    }
    if (whole) {
      __builtin_memcpy(__builtin_assume_aligned(dst + p0 * 3, 8), out, sizeof(out));
    } else {
#pragma unroll
      for (int k = 0; k < NORM_PIX * 3; ++k)
        if (k < n * 3) dst[p0 * 3 + k] = out[k];
    }
  }
}

namespace {

// n taps from p, `stride` bytes apart, C interleaved channels each: Pillow's ImagingResampleHorizontal_8bpc / Vertical_8bpc inner loop.
// The sum wraps like Pillow's int (coefficients of a sane table keep it far inside 32 bits); the shift is arithmetic.
template <int C>
__device__ __forceinline__ void resample_taps(const uint8_t* __restrict__ p, size_t stride, int n, const int* __restrict__ k,
                                              uint8_t* __restrict__ out) {
  unsigned ss[C];
#pragma unroll
  for (int c = 0; c < C; ++c) ss[c] = 1u << 21;
  for (int t = 0; t < n; ++t) {
    const unsigned kv = (unsigned)k[t];
#pragma unroll
    for (int c = 0; c < C; ++c) ss[c] += (unsigned)p[(size_t)t * stride + c] * kv;
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[c] = (uint8_t)min(max((int)ss[c] >> 22, 0), 255);
}

}  // namespace

// VERT = false: src [S][inH][inW][C] -> dst [S][inH][outLen][C] along x; VERT = true: -> dst [S][outLen][inW][C] along y.
// A workgroup takes NT consecutive output pixels of one output row, a lane one pixel with its C channels.
template <int C, bool VERT>
__global__ __launch_bounds__(NT) void resample_kernel(const uint8_t* __restrict__ src, int S, int inH, int inW, int outLen,
                                                      const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                      uint8_t* __restrict__ dst) {
  const int rows = VERT ? outLen : inH, width = VERT ? inW : outLen;
  const int xtiles = (width + NT - 1) / NT;
  const size_t total = (size_t)S * rows * xtiles;
  for (size_t t = blockIdx.x; t < total; t += gridDim.x) {
    const size_t row = t / xtiles;                          // s * rows + y
    const int x = (int)(t % xtiles) * NT + threadIdx.x;
    if (x >= width) continue;
    const size_t s = row / rows;
    const int y = (int)(row % rows);
    const int i = VERT ? y : x, inLen = VERT ? inH : inW;
    const int first = min(max(bounds[2 * i], 0), inLen - 1);
    const int n = min(max(bounds[2 * i + 1], 0), min(ksize, inLen - first));
    const uint8_t* p = VERT ? src + ((s * inH + first) * inW + x) * C : src + ((s * inH + y) * inW + first) * C;
    uint8_t px[C];
    resample_taps<C>(p, VERT ? (size_t)inW * C : (size_t)C, n, kk + (size_t)i * ksize, px);
    uint8_t* q = dst + (row * width + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = px[c];
  }
}

namespace {

template <class T>
hipError_t normalize_typed(const T* src, int S, int H, int W, int C, int swap_rb, unsigned* minmax, uint8_t* dst, hipStream_t st) {
  const int frame_bytes = (int)((size_t)H * W * C * sizeof(T));     // < 2^31, checked by the caller
  const size_t tiles = (size_t)S * (((size_t)frame_bytes + MM_TILE - 1) / MM_TILE);
  hipLaunchKernelGGL(minmax_init_kernel, dim3((S + NT - 1) / NT), dim3(NT), 0, st, minmax, S);
  hipLaunchKernelGGL(minmax_kernel<T>, dim3((unsigned)std::min<size_t>(tiles, MAX_GRID)), dim3(NT), 0, st, src, S, frame_bytes, minmax);
  const size_t total = (size_t)S * H * W, groups = (total + NORM_PIX - 1) / NORM_PIX;
  const dim3 grid((unsigned)std::min<size_t>((groups + NT - 1) / NT, MAX_GRID));
  const bool vec = ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 7) == 0;
  const int HW = H * W;
  if (C == 1) {
    if (vec) hipLaunchKernelGGL((normalize_kernel<T, 1, true>), grid, dim3(NT), 0, st, src, minmax, total, HW, swap_rb, dst);
    else hipLaunchKernelGGL((normalize_kernel<T, 1, false>), grid, dim3(NT), 0, st, src, minmax, total, HW, swap_rb, dst);
  } else {
    if (vec) hipLaunchKernelGGL((normalize_kernel<T, 3, true>), grid, dim3(NT), 0, st, src, minmax, total, HW, swap_rb, dst);
    else hipLaunchKernelGGL((normalize_kernel<T, 3, false>), grid, dim3(NT), 0, st, src, minmax, total, HW, swap_rb, dst);
  }
  return hipGetLastError();
}

template <bool VERT>
void resample_pass(const uint8_t* src, int S, int inH, int inW, int C, int outLen, const int* bounds, const int* kk, int ksize, uint8_t* dst,
                   hipStream_t st) {
  const size_t rows = VERT ? outLen : inH, width = VERT ? inW : outLen;
  const dim3 grid((unsigned)std::min<size_t>((size_t)S * rows * ((width + NT - 1) / NT), MAX_GRID));
  if (C == 1) hipLaunchKernelGGL((resample_kernel<1, VERT>), grid, dim3(NT), 0, st, src, S, inH, inW, outLen, bounds, kk, ksize, dst);
  else hipLaunchKernelGGL((resample_kernel<3, VERT>), grid, dim3(NT), 0, st, src, S, inH, inW, outLen, bounds, kk, ksize, dst);
}

}  // namespace

hipError_t launch_volume_normalize(const void* src, int src_u16, int S, int H, int W, int C, int swap_rb, unsigned* minmax, uint8_t* dst,
                                   hipStream_t st) {
  return src_u16 ? normalize_typed((const uint16_t*)src, S, H, W, C, swap_rb, minmax, dst, st)
                 : normalize_typed((const uint8_t*)src, S, H, W, C, swap_rb, minmax, dst, st);
}

hipError_t launch_resize_pil_u8(const uint8_t* src, int S, int H, int W, int C, uint8_t* tmp, uint8_t* dst, int oh, int ow, const int* xbounds,
                                const int* xkk, int xksize, const int* ybounds, const int* ykk, int yksize, hipStream_t st) {
  const bool horizontal = ow != W, vertical = oh != H;
  if (!horizontal && !vertical) return hipMemcpyAsync(dst, src, (size_t)S * H * W * C, hipMemcpyDeviceToDevice, st);
  if (horizontal) resample_pass<false>(src, S, H, W, C, ow, xbounds, xkk, xksize, vertical ? tmp : dst, st);
  if (vertical) resample_pass<true>(horizontal ? tmp : src, S, H, ow, C, oh, ybounds, ykk, yksize, dst, st);
  return hipGetLastError();
}

}  // namespace octseg
