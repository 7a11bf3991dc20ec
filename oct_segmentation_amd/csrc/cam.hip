// cam.hip -- class activation maps from the activation A and the gradient G of one encoder block (NHWC, plan dtype, [N][h][w][K]):
// what pytorch-grad-cam's GradCAM / HiResCAM / GradCAMElementWise / GradCAMPlusPlus / XGradCAM / LayerCAM compute behind the reference's
// CAMProcessor (src/models/cam_processor.py:83-98, src/models/visualize_activation_maps.py:102-199), and everything the reference's tool
// derives from a map: the thresholded map, its confusion counts against a ground-truth plane of another size, the JET overlay.
//
//   cam_seed      dL/dlogits (NCHW f32) -> the padded NHWC rows the head's data gradient reads (launch_dice_bwd's layout)
//   cam_weights   per (frame, channel): the weight of the three weighted methods.  One thread owns one 16-byte channel vector and walks the
//                 h * w pixels: neighbouring threads read neighbouring vectors (coalesced), no cross-lane reduction.  f32 accumulation.
//                 GradCAM++ needs sum(A) of the channel inside its weight: a second walk over a tensor of at most a few MB (L2)
//   cam_raw       per (frame, pixel): the K-channel contraction (or the element-wise variants), one wave per pixel, shuffle reduction, relu
//   cam_norm      per frame: min / max over the h * w raw values, (x - min) / (1e-7 + max); resets the frame's sweep accumulators
//   cam_resize    cv2.resize(INTER_LINEAR) of the map to S x S in float32 (half-pixel centres, clamped borders), relu, per-frame min / max
//   cam_finish    the second (x - min) / (1e-7 + max) on the resized map; on request the thresholded map and the overlay's whole-image maximum
//   cam_overlay   show_cam_on_image: uint8(255 * (o / max o)), o = (1 - w) * JET(uint8(255 * map)) / 255 + w * frame / 255
//   cam_counts    tp / pred / true of the thresholded map, nearest-resized (host index tables) to the ground truth's size
// A maximum over a whole image is taken by one launch and used by the next one (stream order): no workgroup waits for another.
#include "ev.h"
#include "kernels.h"

namespace octseg {

enum { CAM_GRADCAM = 0, CAM_HIRES = 1, CAM_ELEMENTWISE = 2, CAM_PLUSPLUS = 3, CAM_XGRAD = 4, CAM_LAYER = 5 };
static inline bool cam_weighted(int method) { return method == CAM_GRADCAM || method == CAM_PLUSPLUS || method == CAM_XGRAD; }

// ------------------------------------------------------------------ seed
template <typename T>
__global__ __launch_bounds__(256) void cam_seed_kernel(const float* __restrict__ seed, void* dl, int B, int C, size_t HW, int CP) {
  constexpr int VEC = EV<T>::VEC;
  constexpr int MAXC = 16;
  const size_t npix = (size_t)B * HW;
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (size_t)gridDim.x * blockDim.x) {
    const size_t b = p / HW, i = p - b * HW;
    float d[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) d[c] = c < C ? seed[(b * C + c) * HW + i] : 0.f;
    const size_t row = p * (size_t)(CP / VEC);
#pragma unroll
    for (int v = 0; v < MAXC / VEC; ++v)
      if (v < CP / VEC) stv<T>(dl, row + v, EV<T>::pack(d + v * VEC));
  }
}
hipError_t launch_cam_seed(int dtype, const float* seed, void* dlogits, int B, int C, size_t HW, int CP, hipStream_t st) {
  OCTSEG_NO_F16(dtype);
  if (C > CP || CP > 16 || CP % 8 != 0) return hipErrorInvalidValue;
  const int gr = grid_for((size_t)B * HW, 256);
  OCTSEG_LAUNCH_TRAIN(cam_seed_kernel, dim3(gr), dim3(256), seed, dlogits, B, C, HW, CP);
  return hipGetLastError();
}

// ------------------------------------------------------------------ channel weights
template <typename T>
__global__ __launch_bounds__(256) void cam_weights_kernel(const void* __restrict__ A, const void* __restrict__ G, float* __restrict__ wts, int N,
                                                          int hw, int K, int method) {
  constexpr int VEC = EV<T>::VEC;
  const int vpc = K / VEC;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * vpc) return;
  const int n = t / vpc, cv = t - n * vpc;
  const size_t base = (size_t)n * hw * vpc + cv;
  float sG[VEC], sA[VEC], sGA[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) { sG[i] = 0.f; sA[i] = 0.f; sGA[i] = 0.f; }
  for (int p = 0; p < hw; ++p) {
    float a[VEC], g[VEC];
    EV<T>::unpack(ldv<T>(A, base + (size_t)p * vpc), a);
    EV<T>::unpack(ldv<T>(G, base + (size_t)p * vpc), g);
#pragma unroll
    for (int i = 0; i < VEC; ++i) { sG[i] += g[i]; sA[i] += a[i]; sGA[i] = fmaf(g[i], a[i], sGA[i]); }
  }
  float w[VEC];
  if (method == CAM_GRADCAM) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) w[i] = sG[i] / (float)hw;
  } else if (method == CAM_XGRAD) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) w[i] = sGA[i] / (sA[i] + 1e-7f);
  } else {   // GradCAM++: w = sum max(g, 0) * g^2 / (2 g^2 + sum(A) g^3 + 1e-6), the ratio taken as 0 where g == 0
#pragma unroll
    for (int i = 0; i < VEC; ++i) w[i] = 0.f;
    for (int p = 0; p < hw; ++p) {
      float g[VEC];
      EV<T>::unpack(ldv<T>(G, base + (size_t)p * vpc), g);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float g2 = g[i] * g[i];
        const float den = 2.f * g2 + sA[i] * (g2 * g[i]) + 1e-6f;
        const float aij = g[i] != 0.f ? g2 / den : 0.f;
        w[i] += fmaxf(g[i], 0.f) * aij;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) wts[(size_t)n * K + cv * VEC + i] = w[i];
}

// ------------------------------------------------------------------ raw map: one wave per pixel
template <typename T>
__global__ __launch_bounds__(256) void cam_raw_kernel(const void* __restrict__ A, const void* __restrict__ G, const float* __restrict__ wts,
                                                      float* __restrict__ raw, int N, int hw, int K, int method) {
  constexpr int VEC = EV<T>::VEC;
  const int vpc = K / VEC;
  const int lane = threadIdx.x & 63;
  const size_t pix = (size_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   // wave-uniform
  if (pix >= (size_t)N * hw) return;
  const int n = (int)(pix / hw);
  float s = 0.f;
  for (int cv = lane; cv < vpc; cv += 64) {
    float a[VEC];
    EV<T>::unpack(ldv<T>(A, pix * vpc + cv), a);
    if (method == CAM_GRADCAM || method == CAM_PLUSPLUS || method == CAM_XGRAD) {
      const float* w = wts + (size_t)n * K + cv * VEC;
#pragma unroll
      for (int i = 0; i < VEC; ++i) s = fmaf(w[i], a[i], s);
    } else {
      float g[VEC];
      EV<T>::unpack(ldv<T>(G, pix * vpc + cv), g);
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        if (method == CAM_HIRES) s = fmaf(g[i], a[i], s);
        else if (method == CAM_ELEMENTWISE) s += fmaxf(g[i] * a[i], 0.f);
        else s = fmaf(fmaxf(g[i], 0.f), a[i], s);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) raw[pix] = fmaxf(s, 0.f);
}

// block-wide min / max of non-negative floats (256 threads); result valid in thread 0
static __device__ __forceinline__ void block_minmax(float& lo, float& hi) {
  __shared__ float red[2][4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
  __syncthreads();   // (red may still be read by an earlier call)
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) { lo = fminf(lo, red[0][k]); hi = fmaxf(hi, red[1][k]); }
}

constexpr unsigned CAM_INF_BITS = 0x7f800000u;
// per frame: raw = (raw - min) / (1e-7 + max(raw - min)); acc[n] = {min bits = +inf, max bits = 0, overlay max bits = 0, unused}: every value the
// sweeps reduce is >= 0, and non-negative floats order like their bit patterns, so the sweeps use integer atomicMin / atomicMax
__global__ __launch_bounds__(256) void cam_norm_kernel(float* __restrict__ raw, unsigned* __restrict__ acc, int hw) {
  __shared__ float mm[2];
  float* r = raw + (size_t)blockIdx.x * hw;
  float lo = __uint_as_float(CAM_INF_BITS), hi = 0.f;
  for (int p = threadIdx.x; p < hw; p += blockDim.x) { lo = fminf(lo, r[p]); hi = fmaxf(hi, r[p]); }
  block_minmax(lo, hi);
  if (threadIdx.x == 0) {
    mm[0] = lo; mm[1] = 1e-7f + (hi - lo);
    unsigned* a = acc + 4 * (size_t)blockIdx.x;
    a[0] = CAM_INF_BITS; a[1] = 0u; a[2] = 0u; a[3] = 0u;
  }
  __syncthreads();
  const float m0 = mm[0], den = mm[1];
  for (int p = threadIdx.x; p < hw; p += blockDim.x) r[p] = __fdiv_rn(r[p] - m0, den);
}

// cv2.resize's float32 INTER_LINEAR tap of destination coordinate d on an axis of `in` source and `out` destination samples
static __device__ __forceinline__ void cv2_tap(int d, int in, int out, int& i0, int& i1, float& f) {
  const double scale = (double)in / (double)out;
  float fx = (float)(((double)d + 0.5) * scale - 0.5);
  int sx = (int)floorf(fx);
  fx -= (float)sx;
  if (sx < 0) { sx = 0; fx = 0.f; }
  if (sx >= in - 1) { sx = in - 1; fx = 0.f; }
  i0 = sx; i1 = sx + 1 < in ? sx + 1 : in - 1; f = fx;
}

__global__ __launch_bounds__(256) void cam_resize_kernel(const float* __restrict__ raw, float* __restrict__ maps, unsigned* __restrict__ acc, int h,
                                                         int w, int S) {
  const int n = blockIdx.y;
  const float* r = raw + (size_t)n * h * w;
  float* m = maps + (size_t)n * S * S;
  float lo = __uint_as_float(CAM_INF_BITS), hi = 0.f;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < S * S; idx += gridDim.x * blockDim.x) {
    const int y = idx / S, x = idx - y * S;
    int x0, x1, y0, y1;
    float fx, fy;
    cv2_tap(x, w, S, x0, x1, fx);
    cv2_tap(y, h, S, y0, y1, fy);
    // horizontal pass of both rows, then the vertical one, products and sums rounded one by one as cv2's float loops do
    const float r0 = __fadd_rn(__fmul_rn(r[y0 * w + x0], 1.f - fx), __fmul_rn(r[y0 * w + x1], fx));
    const float r1 = __fadd_rn(__fmul_rn(r[y1 * w + x0], 1.f - fx), __fmul_rn(r[y1 * w + x1], fx));
    const float v = fmaxf(__fadd_rn(__fmul_rn(r0, 1.f - fy), __fmul_rn(r1, fy)), 0.f);
    m[idx] = v;
    lo = fminf(lo, v); hi = fmaxf(hi, v);
  }
  block_minmax(lo, hi);
  if (threadIdx.x == 0) {
    atomicMin(acc + 4 * (size_t)n, __float_as_uint(lo));
    atomicMax(acc + 4 * (size_t)n + 1, __float_as_uint(hi));
  }
}

struct CamOut {
  float* maps; unsigned* acc; int S; int rescale;      // rescale = 0: the maps are final already (overlay of a given map)
  float threshold; uint8_t* bin;                       // nullable: (map > threshold) * 255
  const float* frames; const uint8_t* jet; float wi, wh; uint8_t* overlay;   // overlay nullable; frames [N][3][S][S] BGR planes 0..255, jet [256][3] BGR
};
// o = wh * JET(uint8(255 * map)) / 255 + wi * frame / 255 per channel, every operation rounded to float32 by itself (numpy's order)
static __device__ __forceinline__ void cam_blend(const CamOut& a, int n, int idx, float v, float o[3]) {
  const int j = (int)__fmul_rn(255.f, v);
  const uint8_t* jt = a.jet + 3 * (j < 0 ? 0 : j > 255 ? 255 : j);
  const size_t SS = (size_t)a.S * a.S;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float heat = __fdiv_rn((float)jt[c], 255.f);
    const float img = __fdiv_rn(a.frames[((size_t)n * 3 + c) * SS + idx], 255.f);
    o[c] = __fadd_rn(__fmul_rn(a.wh, heat), __fmul_rn(a.wi, img));
  }
}
__global__ __launch_bounds__(256) void cam_finish_kernel(const CamOut a) {
  const int n = blockIdx.y;
  const int SS = a.S * a.S;
  float* m = a.maps + (size_t)n * SS;
  const float lo = __uint_as_float(a.acc[4 * (size_t)n]);
  const float den = 1e-7f + (__uint_as_float(a.acc[4 * (size_t)n + 1]) - lo);
  float omax = 0.f, unused = 0.f;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < SS; idx += gridDim.x * blockDim.x) {
    float v = m[idx];
    if (a.rescale) { v = __fdiv_rn(v - lo, den); m[idx] = v; }
    if (a.bin) a.bin[(size_t)n * SS + idx] = v > a.threshold ? 255 : 0;
    if (a.overlay) {
      float o[3];
      cam_blend(a, n, idx, v, o);
      omax = fmaxf(omax, fmaxf(o[0], fmaxf(o[1], o[2])));
    }
  }
  if (a.overlay == nullptr) return;   // launch-uniform
  block_minmax(unused, omax);
  if (threadIdx.x == 0) atomicMax(a.acc + 4 * (size_t)n + 2, __float_as_uint(omax));
}
__global__ __launch_bounds__(256) void cam_overlay_kernel(const CamOut a) {
  const int n = blockIdx.y;
  const int SS = a.S * a.S;
  const float* m = a.maps + (size_t)n * SS;
  const float omax = __uint_as_float(a.acc[4 * (size_t)n + 2]);
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < SS; idx += gridDim.x * blockDim.x) {
    float o[3];
    cam_blend(a, n, idx, m[idx], o);
    uint8_t* dst = a.overlay + ((size_t)n * SS + idx) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int q = (int)__fmul_rn(255.f, __fdiv_rn(o[c], omax));   // (omax == 0: an all-black frame under an all-zero JET entry cannot happen, JET(0) has blue 128)
      dst[c] = (uint8_t)(q < 0 ? 0 : q > 255 ? 255 : q);
    }
  }
}

// tp / pred / true over the ground truth's pixels: the thresholded map read through the nearest index tables
__global__ __launch_bounds__(256) void cam_counts_kernel(const float* __restrict__ maps, int S, float threshold, const uint8_t* __restrict__ gt, int gh,
                                                         int gw, const int* __restrict__ rows, const int* __restrict__ cols, int* __restrict__ counts) {
  __shared__ int red[3][4];
  const int n = blockIdx.y;
  const float* m = maps + (size_t)n * S * S;
  const uint8_t* g = gt + (size_t)n * gh * gw;
  int tp = 0, pr = 0, tr = 0;
  const int total = gh * gw;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
    const int y = idx / gw, x = idx - y * gw;
    int sy = rows[y], sx = cols[x];
    sy = sy < 0 ? 0 : sy > S - 1 ? S - 1 : sy;   // tables that are not a resize's give wrong samples, never a stray read
    sx = sx < 0 ? 0 : sx > S - 1 ? S - 1 : sx;
    const int p = m[sy * S + sx] > threshold ? 1 : 0, t = g[idx] != 0 ? 1 : 0;
    tp += p & t; pr += p; tr += t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { tp += __shfl_xor(tp, o, 64); pr += __shfl_xor(pr, o, 64); tr += __shfl_xor(tr, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = tp; red[1][threadIdx.x >> 6] = pr; red[2][threadIdx.x >> 6] = tr; }
  __syncthreads();
  if (threadIdx.x < 3) {   // one atomic per workgroup and count
    const int s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
    if (s) atomicAdd(counts + 3 * (size_t)n + threadIdx.x, s);
  }
}

size_t cam_scratch_bytes(int N, int h, int w, int K) {
  return ((size_t)N * K + (size_t)N * h * w + 4 * (size_t)N) * sizeof(float);
}

hipError_t launch_cam_maps(int dtype, const CamArgs& c, hipStream_t st) {
  OCTSEG_NO_F16(dtype);
  const int VEC = ev_vec(dtype);
  const int hw = c.h * c.w, vpc = c.K / VEC;
  if (c.K % VEC != 0 || c.method < 0 || c.method > 5) return hipErrorInvalidValue;
  float* wts = (float*)c.scratch;
  float* raw = wts + (size_t)c.N * c.K;
  unsigned* acc = (unsigned*)(raw + (size_t)c.N * hw);
  if (cam_weighted(c.method)) {
    const int g = (c.N * vpc + 255) / 256;
    OCTSEG_LAUNCH_TRAIN(cam_weights_kernel, dim3(g), dim3(256), c.A, c.G, wts, c.N, hw, c.K, c.method);
  }
  {
    const int g = (c.N * hw + 3) / 4;
    OCTSEG_LAUNCH_TRAIN(cam_raw_kernel, dim3(g), dim3(256), c.A, c.G, wts, raw, c.N, hw, c.K, c.method);
  }
  hipLaunchKernelGGL(cam_norm_kernel, dim3(c.N), dim3(256), 0, st, raw, acc, hw);
  const int SS = c.S * c.S;
  const dim3 grid(grid_for((size_t)SS, 256, 1024), c.N);
  hipLaunchKernelGGL(cam_resize_kernel, grid, dim3(256), 0, st, raw, c.maps, acc, c.h, c.w, c.S);
  CamOut o;
  o.maps = c.maps; o.acc = acc; o.S = c.S; o.rescale = 1; o.threshold = c.threshold; o.bin = c.bin;
  o.frames = c.frames; o.jet = c.jet; o.wi = (float)c.image_weight; o.wh = (float)(1.0 - c.image_weight); o.overlay = c.overlay;
  hipLaunchKernelGGL(cam_finish_kernel, grid, dim3(256), 0, st, o);
  if (c.overlay) hipLaunchKernelGGL(cam_overlay_kernel, grid, dim3(256), 0, st, o);
  if (c.counts) {
    hipError_t e = hipMemsetAsync(c.counts, 0, 3 * (size_t)c.N * sizeof(int), st);
    if (e != hipSuccess) return e;
    const dim3 gc(grid_for((size_t)c.gt_h * c.gt_w, 256, 1024), c.N);
    hipLaunchKernelGGL(cam_counts_kernel, gc, dim3(256), 0, st, c.maps, c.S, c.threshold, c.gt, c.gt_h, c.gt_w, c.row_index, c.col_index, c.counts);
  }
  return hipGetLastError();
}

// show_cam_on_image of maps that are final already: the maximum pass, then the write pass.  acc: 4 N unsigned of device scratch.
hipError_t launch_cam_overlay(const float* maps, const float* frames, const uint8_t* jet, int N, int S, double image_weight, uint8_t* overlay,
                              void* acc, hipStream_t st) {
  hipError_t e = hipMemsetAsync(acc, 0, 4 * (size_t)N * sizeof(unsigned), st);
  if (e != hipSuccess) return e;
  CamOut o;
  o.maps = const_cast<float*>(maps); o.acc = (unsigned*)acc; o.S = S; o.rescale = 0; o.threshold = 0.f; o.bin = nullptr;
  o.frames = frames; o.jet = jet; o.wi = (float)image_weight; o.wh = (float)(1.0 - image_weight); o.overlay = overlay;
  const dim3 grid(grid_for((size_t)S * S, 256, 1024), N);
  hipLaunchKernelGGL(cam_finish_kernel, grid, dim3(256), 0, st, o);
  hipLaunchKernelGGL(cam_overlay_kernel, grid, dim3(256), 0, st, o);
  return hipGetLastError();
}

}  // namespace octseg
