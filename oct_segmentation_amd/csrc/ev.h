// ev.h -- what every HBM-bound NHWC sweep kernel shares: the 16-byte element vectors (tensors are moved as 8 x bf16 / f16 or 4 x f32 per
// lane and processed in f32), scalar element access, the dtype dispatch of a launch, the grid rule, and torch's align_corners=True
// source-index rule.  A dtype is added, or a conversion changed, here and nowhere else.
#pragma once
#include "common.h"

namespace octseg {

template <typename T> struct EV;  // 16-byte element vector helpers
template <> struct EV<float> {
  static constexpr int VEC = 4;
  static __device__ __forceinline__ void unpack(const uint4& v, float* x) {
    x[0] = __uint_as_float(v.x); x[1] = __uint_as_float(v.y); x[2] = __uint_as_float(v.z); x[3] = __uint_as_float(v.w);
  }
  static __device__ __forceinline__ uint4 pack(const float* x) {
    return make_uint4(__float_as_uint(x[0]), __float_as_uint(x[1]), __float_as_uint(x[2]), __float_as_uint(x[3]));
  }
};
static __device__ __forceinline__ unsigned pk_bf16(float lo, float hi) {
  // one v_cvt_pk_bf16_f32 (two scalar conversions + shift + or took four instructions)
  typedef __attribute__((ext_vector_type(2))) float f32x2_t;
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
  const f32x2_t x = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2_t));
}
template <> struct EV<bf16_t> {
  static constexpr int VEC = 8;
  static __device__ __forceinline__ void unpack(const uint4& v, float* x) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[2 * i] = __uint_as_float(w[i] << 16); x[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
  }
  static __device__ __forceinline__ uint4 pack(const float* x) {
    return make_uint4(pk_bf16(x[0], x[1]), pk_bf16(x[2], x[3]), pk_bf16(x[4], x[5]), pk_bf16(x[6], x[7]));
  }
};
template <> struct EV<f16_t> {   // IEEE half (serving dtype): conversions round to nearest even
  static constexpr int VEC = 8;
  typedef __attribute__((ext_vector_type(2))) _Float16 h2_t;
  static __device__ __forceinline__ void unpack(const uint4& v, float* x) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { const h2_t p = __builtin_bit_cast(h2_t, w[i]); x[2 * i] = (float)p[0]; x[2 * i + 1] = (float)p[1]; }
  }
  static __device__ __forceinline__ uint4 pack(const float* x) {
    unsigned w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const h2_t p = {(_Float16)x[2 * i], (_Float16)x[2 * i + 1]}; w[i] = __builtin_bit_cast(unsigned, p); }
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
};
// one element (the kernels whose channel counts do not fill a vector)
template <typename T> static __device__ __forceinline__ float ld1(const void* p, size_t i);
template <> __device__ __forceinline__ float ld1<float>(const void* p, size_t i) { return ((const float*)p)[i]; }
template <> __device__ __forceinline__ float ld1<bf16_t>(const void* p, size_t i) { return __uint_as_float((unsigned)((const unsigned short*)p)[i] << 16); }
template <> __device__ __forceinline__ float ld1<f16_t>(const void* p, size_t i) { return (float)__builtin_bit_cast(_Float16, ((const unsigned short*)p)[i]); }
template <typename T> static __device__ __forceinline__ void st1(void* p, size_t i, float v);
template <> __device__ __forceinline__ void st1<float>(void* p, size_t i, float v) { ((float*)p)[i] = v; }
template <> __device__ __forceinline__ void st1<bf16_t>(void* p, size_t i, float v) { ((unsigned short*)p)[i] = (unsigned short)(pk_bf16(v, 0.f) & 0xffffu); }
template <> __device__ __forceinline__ void st1<f16_t>(void* p, size_t i, float v) { const _Float16 h = (_Float16)v; ((unsigned short*)p)[i] = __builtin_bit_cast(unsigned short, h); }

static inline int ev_vec(int dtype) { return dtype == DT_F32 ? 4 : 8; }   // elements of one 16-byte vector (EV<T>::VEC, on the host)

// KERNEL<T> for the `dtype` and on the stream `st` of the enclosing launcher.  OCTSEG_LAUNCH: every dtype.  OCTSEG_LAUNCH_TRAIN: kernels
// with no f16 instantiation (the training-only sweeps, and pure 16-byte moves): f32 -> float, everything else -> bf16_t.
#define OCTSEG_LAUNCH_LDS(KERNEL, grid, block, lds, ...)                                        \
  do {                                                                                          \
    if (dtype == DT_F32) hipLaunchKernelGGL(KERNEL<float>, grid, block, lds, st, __VA_ARGS__);      \
    else if (dtype == DT_F16) hipLaunchKernelGGL(KERNEL<f16_t>, grid, block, lds, st, __VA_ARGS__); \
    else hipLaunchKernelGGL(KERNEL<bf16_t>, grid, block, lds, st, __VA_ARGS__);                     \
  } while (0)
#define OCTSEG_LAUNCH_TRAIN_LDS(KERNEL, grid, block, lds, ...)                                  \
  do {                                                                                          \
    if (dtype == DT_F32) hipLaunchKernelGGL(KERNEL<float>, grid, block, lds, st, __VA_ARGS__);      \
    else hipLaunchKernelGGL(KERNEL<bf16_t>, grid, block, lds, st, __VA_ARGS__);                     \
  } while (0)
#define OCTSEG_LAUNCH(KERNEL, grid, block, ...) OCTSEG_LAUNCH_LDS(KERNEL, grid, block, 0, __VA_ARGS__)
#define OCTSEG_LAUNCH_TRAIN(KERNEL, grid, block, ...) OCTSEG_LAUNCH_TRAIN_LDS(KERNEL, grid, block, 0, __VA_ARGS__)
// f16 is the dtype of eval forwards only: the training-only sweeps have no f16 instantiation and refuse it
#define OCTSEG_NO_F16(dtype) do { if ((dtype) == DT_F16) return hipErrorInvalidValue; } while (0)
template <typename T> static __device__ __forceinline__ uint4 ldv(const void* p, size_t vec_idx) {
  return ((const uint4*)p)[vec_idx];
}
template <typename T> static __device__ __forceinline__ void stv(void* p, size_t vec_idx, const uint4& v) {
  ((uint4*)p)[vec_idx] = v;
}

static inline int grid_for(size_t n, int block, int cap = 8192) {
  size_t g = (n + block - 1) / block;
  if (g > (size_t)cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}


// torch's align_corners=True source index: scale = (in - 1) / (out - 1) in float, x = scale * o, i0 = (int)x, lambda1 = x - i0
struct Lerp { int i0, i1; float w0, w1; };
static __device__ __forceinline__ Lerp lerp_of(int o, int in, float scale) {
  const float x = scale * (float)o;
  Lerp l;
  l.i0 = min((int)x, in - 1);
  l.i1 = l.i0 + (l.i0 < in - 1 ? 1 : 0);
  l.w1 = x - (float)l.i0;
  l.w0 = 1.f - l.w1;
  return l;
}
static inline float lerp_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

}  // namespace octseg
