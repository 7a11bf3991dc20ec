// ingest.hip -- the input half of the pipeline on the GPU (reference src/models/smp/dataset.py:108-127, src/data/utils.py:159-166).
//
// The reference decodes a frame to uint8 HWC, resizes it with cv2.resize (8-bit INTER_LINEAR: 11-bit fixed-point coefficients; INTER_AREA's
// 2x2 mean for an exact 2x decimation in both axes), nearest-resizes the 4-channel uint8 mask, selects the class channels, casts bool -> float
// and transposes to CHW float32 -- all on the CPU, per frame.  Here the uint8 arrays cross to the device as they are (3 B / pixel instead of 12)
// and two kernels produce the float32 NCHW batch the nets take.  The arithmetic is integer and the per-axis tables come from the host
// (oct_segmentation_amd/predict.py cv2_linear_coeffs / cv2_nearest_index, pinned bit for bit against oracle/cv2_resize.py), so the result EQUALS
// the reference's -- no tolerance.
//
// ingest_image_kernel: one workgroup per 64 x 16 output tile of one frame.  (A) the source window of the tile goes to LDS with aligned dword loads
// (every source byte is fetched once per tile, not once per output sample and tap); (B) the horizontal pass r = s[x0] * a0 + s[x1] * a1 runs once
// per SOURCE row of the window and is shared by the output rows that use it (LDS, uint16 [row][plane][64]); (C) the vertical pass reads two
// ushort4 per lane and stores one float4: 16 lanes cover 256 contiguous bytes of an output plane row.
// ingest_mask_kernel: no neighbourhood, so no LDS: a lane takes 4 consecutive output x of one row, loads each source PIXEL once (one dword for the
// 4-channel TIFF layout) and writes one float4 per selected class plane.
// *_gather_kernel: the one-thread-per-output-pixel forms (byte loads from global).  The image one runs when a tile's source window does not fit LDS
// (decimation by more than ~3.5x) and both are kept selectable (octseg_debug_set_ingest_variant) as the yardstick the staged forms are timed against.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace octseg {

namespace {

constexpr int TW = 64, TH = 16, NT = 256;   // output tile, threads per workgroup (the kernel's lane maps assume NT == TW * 4 == TH * 16)
constexpr size_t LDS_MAX = 64 * 1024;       // dynamic LDS a launch may ask for without an attribute

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// VResizeLinear<uchar, int, short, FixedPtCast<int, uchar, 22>> / ResizeAreaFastVec on two horizontal sums; q = r >> 4 (area: q = r)
__device__ __forceinline__ float vpass_q(int q0, int q1, int b0, int b1, int area) {
  const int v = area ? (q0 + q1 + 2) >> 2 : (((b0 * q0) >> 16) + ((b1 * q1) >> 16) + 2) >> 2;
  return (float)clampi(v, 0, 255);
}
__device__ __forceinline__ float vpass(int r0, int r1, int b0, int b1, int area) {
  return area ? vpass_q(r0, r1, b0, b1, 1) : vpass_q(r0 >> 4, r1 >> 4, b0, b1, 0);
}

// one output sample straight from global memory; fr = the frame, indices already clamped to it
__device__ __forceinline__ float sample_direct(const uint8_t* fr, int Ws, int ch, int x0, int x1, int a0, int a1, int y0, int y1, int b0, int b1,
                                               int area) {
  const uint8_t* p0 = fr + (size_t)y0 * Ws * 3 + ch;
  const uint8_t* p1 = fr + (size_t)y1 * Ws * 3 + ch;
  const int r0 = (int)p0[(size_t)x0 * 3] * a0 + (int)p0[(size_t)x1 * 3] * a1;
  const int r1 = (int)p1[(size_t)x0 * 3] * a0 + (int)p1[(size_t)x1 * 3] * a1;
  return vpass(r0, r1, b0, b1, area);
}

}  // namespace

// xtab [4][Wd] / ytab [4][Hd] int32: first tap, second tap, coefficient of the first, coefficient of the second (x 2048).  area = 1 (exact 2x
// decimation in both axes): the taps of the tables, coefficients taken as 1 and the 2x2 mean's rounding.  Taps are clamped to the frame, so a
// malformed table gives wrong samples, never an access outside src.
__global__ __launch_bounds__(NT) void ingest_image_gather_kernel(const uint8_t* src, int B, int Hs, int Ws, int swap_rb, float* out, int Hd, int Wd,
                                                                 const int* xtab, const int* ytab, int area) {
  const size_t total = (size_t)B * Hd * Wd;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % Wd);
    const int y = (int)((i / Wd) % Hd);
    const size_t n = i / ((size_t)Wd * Hd);
    const int x0 = clampi(xtab[x], 0, Ws - 1), x1 = clampi(xtab[Wd + x], 0, Ws - 1);
    const int y0 = clampi(ytab[y], 0, Hs - 1), y1 = clampi(ytab[Hd + y], 0, Hs - 1);
    const int a0 = area ? 1 : xtab[2 * Wd + x], a1 = area ? 1 : xtab[3 * Wd + x];
    const int b0 = ytab[2 * Hd + y], b1 = ytab[3 * Hd + y];
    const uint8_t* fr = src + n * Hs * Ws * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      out[((n * 3 + c) * Hd + y) * Wd + x] = sample_direct(fr, Ws, swap_rb ? 2 - c : c, x0, x1, a0, a1, y0, y1, b0, b1, area);
  }
}

// Dynamic LDS: hbuf uint16 [raw_rows][3][TW] (horizontal sums of the window's rows, already >> 4 as the vertical pass takes them: at most
// 255 * 2048 >> 4 = 32640; area: the two-tap sum, at most 510), then raw dwords [raw_rows][raw_pitch_dw] (the window's bytes,
// each row from the 4-byte boundary at or below its first byte).  raw_rows / raw_pitch_dw are the host's bound for a tile's window; a tile whose
// window is larger (tables that are not a resize's) takes the direct path instead.
__global__ __launch_bounds__(NT) void ingest_image_kernel(const uint8_t* src, int B, int Hs, int Ws, int swap_rb, float* out, int Hd, int Wd,
                                                          const int* xtab, const int* ytab, int area, int raw_rows, int raw_pitch_dw, int vec4) {
  extern __shared__ __align__(16) unsigned short smem[];
  unsigned short* hbuf = smem;
  uint32_t* raw = (uint32_t*)(smem + (size_t)raw_rows * 3 * TW);
  const int tid = threadIdx.x;
  const int tiles_x = (Wd + TW - 1) / TW, tiles_y = (Hd + TH - 1) / TH;
  const size_t total = (size_t)B * tiles_x * tiles_y;
  for (size_t t = blockIdx.x; t < total; t += gridDim.x) {
    const int ox = (int)(t % tiles_x) * TW, oy = (int)((t / tiles_x) % tiles_y) * TH;
    const size_t n = t / ((size_t)tiles_x * tiles_y);
    const int ow = min(TW, Wd - ox), oh = min(TH, Hd - oy);
    const uint8_t* fr = src + n * Hs * Ws * 3;
    // the tile's source window: a resize's tap tables do not decrease, so the first output's first tap and the last one's second bound it
    const int sx_lo = clampi(xtab[ox], 0, Ws - 1), sx_hi = clampi(xtab[Wd + ox + ow - 1], 0, Ws - 1);
    const int sy_lo = clampi(ytab[oy], 0, Hs - 1), sy_hi = clampi(ytab[Hd + oy + oh - 1], 0, Hs - 1);
    const int nr = sy_hi - sy_lo + 1, nbx = (sx_hi - sx_lo + 1) * 3;
    const bool fits = nr >= 1 && nr <= raw_rows && nbx >= 3 && (nbx + 6) / 4 <= raw_pitch_dw;   // wave- and workgroup-uniform
    if (!fits) {
      for (int i = tid; i < oh * ow; i += NT) {
        const int x = ox + i % ow, y = oy + i / ow;
        const int x0 = clampi(xtab[x], 0, Ws - 1), x1 = clampi(xtab[Wd + x], 0, Ws - 1);
        const int y0 = clampi(ytab[y], 0, Hs - 1), y1 = clampi(ytab[Hd + y], 0, Hs - 1);
        const int a0 = area ? 1 : xtab[2 * Wd + x], a1 = area ? 1 : xtab[3 * Wd + x];
#pragma unroll
        for (int c = 0; c < 3; ++c)
          out[((n * 3 + c) * Hd + y) * Wd + x] =
              sample_direct(fr, Ws, swap_rb ? 2 - c : c, x0, x1, a0, a1, y0, y1, ytab[2 * Hd + y], ytab[3 * Hd + y], area);
      }
      continue;
    }
    // ---- (A) window -> LDS: two waves per window row.  A dword is loaded only if it holds at least one byte of the window: an aligned dword
    // never straddles a page, so the up to 3 bytes it may carry from outside the frame (or the tensor) are readable; they are never used
    // Eight rows' loads are issued before the first of them is waited for: one load per loop turn would pay a global-memory latency per row
    {
      const uint8_t* w0 = fr + ((size_t)sy_lo * Ws + sx_lo) * 3;      // first byte of the window
      const int m0 = (int)((uintptr_t)w0 & 3);
      const size_t rowb = (size_t)Ws * 3;
      for (int rbase = tid >> 7; rbase < nr; rbase += 8 * (NT / 128))
        for (int dw = tid & 127; dw < raw_pitch_dw; dw += 128) {
          uint32_t v[8];
          bool ok[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int r = rbase + k * (NT / 128);
            const size_t off = (size_t)r * rowb;                     // row r starts at w0 + off, (m0 + off) & 3 bytes past a dword boundary
            const int m = (int)((m0 + off) & 3);
            ok[k] = r < nr && dw * 4 < m + nbx;
            v[k] = ok[k] ? ((const uint32_t*)(w0 + off - m))[dw] : 0u;
          }
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (ok[k]) raw[(rbase + k * (NT / 128)) * raw_pitch_dw + dw] = v[k];
        }
    }
    __syncthreads();
    // ---- (B) horizontal pass, once per window row: a wave owns a row, its lanes the tile's 64 columns, three planes each
    {
      const int x = tid & (TW - 1), gx = min(ox + x, Wd - 1);
      const int i0 = (clampi(xtab[gx], sx_lo, sx_hi) - sx_lo) * 3, i1 = (clampi(xtab[Wd + gx], sx_lo, sx_hi) - sx_lo) * 3;
      const int a0 = area ? 1 : xtab[2 * Wd + gx], a1 = area ? 1 : xtab[3 * Wd + gx];
      const int c0 = swap_rb ? 2 : 0, c2 = 2 - c0, qs = area ? 0 : 4;
      for (int r = __builtin_amdgcn_readfirstlane(tid / TW); r < nr; r += NT / TW) {
        const int sh = (int)((uintptr_t)(fr + ((size_t)(sy_lo + r) * Ws + sx_lo) * 3) & 3);   // as in (A)
        const uint8_t* rb = (const uint8_t*)(raw + r * raw_pitch_dw) + sh;
        unsigned short* h = hbuf + r * 3 * TW + x;
        h[0] = (unsigned short)(((int)rb[i0 + c0] * a0 + (int)rb[i1 + c0] * a1) >> qs);
        h[TW] = (unsigned short)(((int)rb[i0 + 1] * a0 + (int)rb[i1 + 1] * a1) >> qs);
        h[2 * TW] = (unsigned short)(((int)rb[i0 + c2] * a0 + (int)rb[i1 + c2] * a1) >> qs);
      }
    }
    __syncthreads();
    // ---- (C) vertical pass: a lane takes 4 columns of one tile row in the three planes; 16 lanes x float4 = one 64-sample plane row
    {
      const int xq = (tid & 15) * 4, x = ox + xq, y = tid >> 4, gy = oy + y;
      if (y < oh && x < Wd) {
        const int r0 = clampi(ytab[gy], sy_lo, sy_hi) - sy_lo, r1 = clampi(ytab[Hd + gy], sy_lo, sy_hi) - sy_lo;
        const int b0 = ytab[2 * Hd + gy], b1 = ytab[3 * Hd + gy];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const ushort4 h0 = *(const ushort4*)&hbuf[(r0 * 3 + c) * TW + xq];
          const ushort4 h1 = *(const ushort4*)&hbuf[(r1 * 3 + c) * TW + xq];
          const float4 v = make_float4(vpass_q(h0.x, h1.x, b0, b1, area), vpass_q(h0.y, h1.y, b0, b1, area), vpass_q(h0.z, h1.z, b0, b1, area),
                                       vpass_q(h0.w, h1.w, b0, b1, area));
          float* o = out + ((n * 3 + c) * Hd + gy) * Wd + x;
          if (vec4) {
            *(float4*)o = v;                    // Wd % 4 == 0: a quad that starts inside the row ends inside it
          } else {
            o[0] = v.x;
            if (x + 1 < Wd) o[1] = v.y;
            if (x + 2 < Wd) o[2] = v.z;
            if (x + 3 < Wd) o[3] = v.w;
          }
        }
      }
    }
    __syncthreads();   // the next tile of this workgroup overwrites both LDS images
  }
}

// out[n][c][y][x] = src[n][rows[y]][cols[x]][ch[c]] != 0.  dword_px: Cs == 4 and src 4-byte aligned, a source pixel is one dword
__global__ __launch_bounds__(NT) void ingest_mask_kernel(const uint8_t* src, int B, int Hs, int Ws, int Cs, const int* ch_ids, int C, float* out,
                                                         int Hd, int Wd, const int* rows, const int* cols, int vec4, int dword_px) {
  const int qw = (Wd + 3) / 4;
  const size_t total = (size_t)B * Hd * qw, plane = (size_t)Hd * Wd;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % qw) * 4;
    const int y = (int)((i / qw) % Hd);
    const size_t n = i / ((size_t)qw * Hd);
    const uint8_t* rowp = src + (n * Hs + clampi(rows[y], 0, Hs - 1)) * Ws * Cs;
    int xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = clampi(cols[min(x + j, Wd - 1)], 0, Ws - 1);
    uint32_t px[4] = {0, 0, 0, 0};
    if (dword_px) {
#pragma unroll
      for (int j = 0; j < 4; ++j) px[j] = ((const uint32_t*)rowp)[xs[j]];
    }
    float* o = out + n * C * plane + (size_t)y * Wd + x;
    for (int c = 0; c < C; ++c, o += plane) {
      const int ch = clampi(ch_ids[c], 0, Cs - 1);
      float v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (dword_px ? ((px[j] >> (8 * ch)) & 0xffu) : (uint32_t)rowp[(size_t)xs[j] * Cs + ch]) ? 1.f : 0.f;
      if (vec4) {
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < Wd) o[j] = v[j];
      }
    }
  }
}

__global__ __launch_bounds__(NT) void ingest_mask_gather_kernel(const uint8_t* src, int B, int Hs, int Ws, int Cs, const int* ch_ids, int C,
                                                                float* out, int Hd, int Wd, const int* rows, const int* cols) {
  const size_t total = (size_t)B * Hd * Wd;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % Wd);
    const int y = (int)((i / Wd) % Hd);
    const size_t n = i / ((size_t)Wd * Hd);
    const uint8_t* p = src + ((n * Hs + clampi(rows[y], 0, Hs - 1)) * Ws + clampi(cols[x], 0, Ws - 1)) * Cs;
    for (int c = 0; c < C; ++c) out[((n * C + c) * Hd + y) * Wd + x] = p[clampi(ch_ids[c], 0, Cs - 1)] ? 1.f : 0.f;
  }
}

static unsigned capped_grid(size_t items) {
  size_t g = (items + NT - 1) / NT;
  return (unsigned)(g > 16384 ? 16384 : (g ? g : 1));
}

// variant 0: the LDS-staged kernel (the gather one when a tile's source window cannot fit LDS); 1: the per-pixel gather kernel
hipError_t launch_ingest_image(const uint8_t* src, int B, int Hs, int Ws, int swap_rb, float* out, int Hd, int Wd, const int* xtab,
                               const int* ytab, int variant, hipStream_t st) {
  const int area = (Ws == 2 * Wd && Hs == 2 * Hd) ? 1 : 0;   // cv::resize: INTER_LINEAR becomes INTER_AREA when both scales are exactly 2
  // bound of a tile's window: its first output's first tap to its last output's second tap span fewer than extent * scale + 3 samples
  const long long cols = std::min<long long>(Ws, ((long long)TW * Ws + Wd - 1) / Wd + 3);
  const long long rws = std::min<long long>(Hs, ((long long)TH * Hs + Hd - 1) / Hd + 3);
  const long long pitch_dw = (cols * 3 + 6) / 4;
  const unsigned long long lds = (unsigned long long)rws * (3 * TW * 2 + pitch_dw * 4);
  if (variant == 1 || lds > LDS_MAX) {
    hipLaunchKernelGGL(ingest_image_gather_kernel, dim3(capped_grid((size_t)B * Hd * Wd)), dim3(NT), 0, st, src, B, Hs, Ws, swap_rb, out, Hd, Wd,
                       xtab, ytab, area);
    return hipGetLastError();
  }
  const size_t tiles = (size_t)B * ((Wd + TW - 1) / TW) * ((Hd + TH - 1) / TH);
  const int vec4 = (Wd % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(ingest_image_kernel, dim3((unsigned)std::min<size_t>(tiles, 1u << 20)), dim3(NT), (size_t)lds, st, src, B, Hs, Ws, swap_rb,
                     out, Hd, Wd, xtab, ytab, area, (int)rws, (int)pitch_dw, vec4);
  return hipGetLastError();
}

hipError_t launch_ingest_mask(const uint8_t* src, int B, int Hs, int Ws, int Cs, const int* ch_ids, int C, float* out, int Hd, int Wd,
                              const int* rows, const int* cols, int variant, hipStream_t st) {
  if (variant == 1) {
    hipLaunchKernelGGL(ingest_mask_gather_kernel, dim3(capped_grid((size_t)B * Hd * Wd)), dim3(NT), 0, st, src, B, Hs, Ws, Cs, ch_ids, C, out, Hd,
                       Wd, rows, cols);
    return hipGetLastError();
  }
  const int vec4 = (Wd % 4 == 0 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  const int dword_px = (Cs == 4 && ((uintptr_t)src & 3) == 0) ? 1 : 0;
  hipLaunchKernelGGL(ingest_mask_kernel, dim3(capped_grid((size_t)B * Hd * ((Wd + 3) / 4))), dim3(NT), 0, st, src, B, Hs, Ws, Cs, ch_ids, C, out, Hd,
                     Wd, rows, cols, vec4, dword_px);
  return hipGetLastError();
}

}  // namespace octseg
