// panels.hip -- the per-epoch sample dump of the training loop on the GPU: log_predict_model_on_epoch (reference src/models/smp/model.py:208-271,
// called from on_validation_epoch_end, model.py:134-148) with the class colours / ids of src/data/utils.py:16-45.
//
// Per file of <data_dir>/vis/img the reference resizes the frame (cv2.resize, BGR uint8) and the 4-channel TIFF mask (INTER_NEAREST, raw values
// kept), predicts the frame (sigmoid > 0.5), and paints two colour masks that start (128,128,128): for every class IN LIST ORDER the ground truth
// takes the class colour where mask[..., CLASS_ID - 1] == 255 (exactly 255, not != 0) and the prediction where pred[..., idy] == 1; later classes
// overwrite earlier ones.  hstack(img, color_gt, color_pred) goes to cv2.imwrite, two label maps with CLASS_ID instead of the colour go to W&B.
// Here the resized frames (octseg_ingest_image's planes), the logits and the RAW source-size TIFF samples of a group of frames meet in one
// launch that writes the strips as RGB (what the reference's BGR file decodes to) and the label maps.  Comparisons and integer moves only:
// the outputs EQUAL the reference's -- no tolerance.
//
// epoch_panels_kernel: bandwidth-bound, no neighbourhood, so no LDS beyond the class tables.  A thread takes 4 consecutive pixels of one pane
// of one strip row (12 output bytes); the items of a row are numbered pane-major, so with S % 4 == 0 a wave's lanes cover consecutive 12-byte
// pieces of the 9 S-byte row across the pane borders: three dword stores per lane, every cache line written whole.  The frame planes and the
// logits come in as one float4 per plane / class, a ground-truth source pixel as one dword (the 4-channel TIFF layout), a label quad leaves as
// one dword.  Rows whose byte offsets are not multiples of 4 (S % 4 != 0: S = 33 gives a 297-byte row; or unaligned tensors) take scalar loads
// and byte stores, item by item the same values.
#include <algorithm>

#include "common.h"
#include "kernels.h"
#include "sigmoid.h"

namespace octseg {

namespace {

constexpr int NT = 256;
constexpr int MAXC = 16;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// a frame sample (an integer 0..255 stored as float) as a byte
__device__ __forceinline__ unsigned u8f(float v) { return (unsigned)fminf(fmaxf(v, 0.f), 255.f); }

}  // namespace

// vec_* : S % 4 == 0 and the tensor's base is aligned for the wide access (frames / logits 16 bytes, panels / labels 4); dword_px: SC == 4 and
// gt 4-byte aligned.  labels may be null.
__global__ __launch_bounds__(NT) void epoch_panels_kernel(const float* __restrict__ frames, const float* __restrict__ logits,
                                                          const uint8_t* __restrict__ gt, int N, int S, int C, int Hs, int Ws, int SC,
                                                          const int* __restrict__ rows, const int* __restrict__ cols,
                                                          const int* __restrict__ gt_ch, const uint8_t* __restrict__ class_rgb,
                                                          const uint8_t* __restrict__ class_ids, uint8_t* __restrict__ panels,
                                                          uint8_t* __restrict__ labels, int vec_frames, int vec_logits, int vec_out, int vec_lab,
                                                          int dword_px) {
  __shared__ int chs[MAXC];
  __shared__ unsigned rgb[MAXC][3];
  __shared__ unsigned ids[MAXC];
  const int tid = threadIdx.x;
  if (tid < C) {
    chs[tid] = clampi(gt_ch[tid], 0, SC - 1);
    rgb[tid][0] = class_rgb[tid * 3]; rgb[tid][1] = class_rgb[tid * 3 + 1]; rgb[tid][2] = class_rgb[tid * 3 + 2];
    ids[tid] = class_ids[tid];
  }
  __syncthreads();

  const int qw = (S + 3) / 4;                      // quads of a pane row
  const size_t plane = (size_t)S * S, per_row = (size_t)3 * qw;
  const size_t total = (size_t)N * S * per_row;
  for (size_t i = (size_t)blockIdx.x * NT + tid; i < total; i += (size_t)gridDim.x * NT) {
    const int q = (int)(i % per_row);
    const int y = (int)((i / per_row) % S);
    const size_t n = i / (per_row * S);
    const int pane = q / qw, x = (q - pane * qw) * 4;
    const int np = min(4, S - x);                  // pixels of this quad inside the row (4 on the vector paths)
    unsigned px[4][3], lab[4] = {0u, 0u, 0u, 0u};
    if (pane == 0) {
      // ---- the frame: BGR planes -> RGB bytes
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float* p = frames + (n * 3 + (2 - k)) * plane + (size_t)y * S + x;
        if (vec_frames) {
          const float4 v = *(const float4*)p;
          px[0][k] = u8f(v.x); px[1][k] = u8f(v.y); px[2][k] = u8f(v.z); px[3][k] = u8f(v.w);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) px[j][k] = j < np ? u8f(p[j]) : 0u;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) px[j][0] = px[j][1] = px[j][2] = 128u;
      if (pane == 1) {
        // ---- ground truth: nearest-resized raw TIFF samples, painted where a class's channel is exactly 255
        const uint8_t* rowp = gt + (n * Hs + clampi(rows[y], 0, Hs - 1)) * Ws * SC;
        int xs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[j] = clampi(cols[min(x + j, S - 1)], 0, Ws - 1);
        uint32_t pd[4] = {0u, 0u, 0u, 0u};
        if (dword_px) {
#pragma unroll
          for (int j = 0; j < 4; ++j) pd[j] = ((const uint32_t*)rowp)[xs[j]];
        }
        for (int c = 0; c < C; ++c) {
          const int ch = chs[c];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const unsigned v = dword_px ? (pd[j] >> (8 * ch)) & 0xffu : (unsigned)rowp[(size_t)xs[j] * SC + ch];
            if (v == 255u) { px[j][0] = rgb[c][0]; px[j][1] = rgb[c][1]; px[j][2] = rgb[c][2]; lab[j] = ids[c]; }
          }
        }
      } else {
        // ---- prediction: the reference's `sigmoid() > 0.5` in fp32 (model.py:195), as the Dice kernel and octseg_mask_assemble
        for (int c = 0; c < C; ++c) {
          const float* p = logits + (n * C + c) * plane + (size_t)y * S + x;
          float z[4];
          if (vec_logits) {
            const float4 v = *(const float4*)p;
            z[0] = v.x; z[1] = v.y; z[2] = v.z; z[3] = v.w;
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = j < np ? p[j] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (sigmoid_acc(z[j]) > 0.5f) { px[j][0] = rgb[c][0]; px[j][1] = rgb[c][1]; px[j][2] = rgb[c][2]; lab[j] = ids[c]; }
        }
      }
    }
    const size_t off = ((n * S + y) * 3 + pane) * (size_t)S * 3 + (size_t)x * 3;     // strip row = three panes of 3 S bytes
    if (vec_out) {
      uint32_t* o = (uint32_t*)(panels + off);
      o[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
      o[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
      o[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < np) {
#pragma unroll
          for (int k = 0; k < 3; ++k) panels[off + j * 3 + k] = (uint8_t)px[j][k];
        }
    }
    if (labels && pane) {                            // plane 0: prediction, plane 1: ground truth
      uint8_t* l = labels + (n * 2 + (pane == 2 ? 0 : 1)) * plane + (size_t)y * S + x;
      if (vec_lab) {
        *(uint32_t*)l = lab[0] | (lab[1] << 8) | (lab[2] << 16) | (lab[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < np) l[j] = (uint8_t)lab[j];
      }
    }
  }
}

hipError_t launch_epoch_panels(const float* frames, const float* logits, const uint8_t* gt, int N, int S, int C, int Hs, int Ws, int SC,
                               const int* rows, const int* cols, const int* gt_ch, const uint8_t* class_rgb, const uint8_t* class_ids,
                               uint8_t* panels, uint8_t* labels, hipStream_t st) {
  const int q = S % 4 == 0;
  const int vec_frames = (q && ((uintptr_t)frames & 15) == 0) ? 1 : 0, vec_logits = (q && ((uintptr_t)logits & 15) == 0) ? 1 : 0;
  const int vec_out = (q && ((uintptr_t)panels & 3) == 0) ? 1 : 0, vec_lab = (q && ((uintptr_t)labels & 3) == 0) ? 1 : 0;
  const int dword_px = (SC == 4 && ((uintptr_t)gt & 3) == 0) ? 1 : 0;
  const size_t items = (size_t)N * S * 3 * ((S + 3) / 4);
  const size_t g = (items + NT - 1) / NT;
  hipLaunchKernelGGL(epoch_panels_kernel, dim3((unsigned)std::min<size_t>(std::max<size_t>(g, 1), 16384)), dim3(NT), 0, st, frames, logits, gt, N,
                     S, C, Hs, Ws, SC, rows, cols, gt_ch, class_rgb, class_ids, panels, labels, vec_frames, vec_logits, vec_out, vec_lab,
                     dword_px);
  return hipGetLastError();
}

}  // namespace octseg
