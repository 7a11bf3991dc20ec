// The one sigmoid behind every `sigmoid(z) > 0.5` of the engine (Dice kernel, serving epilogue, per-epoch panels): kernels that threshold
// logits include this, so two of them cannot disagree about a pixel.
#pragma once
#include <hip/hip_runtime.h>

namespace octseg {

static __device__ __forceinline__ float sigmoid_acc(float z) {
  // exp(logsigmoid(z)) as smp computes it, evaluated without cancellation
  const float e = expf(-fabsf(z));
  return z >= 0.f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

}  // namespace octseg
