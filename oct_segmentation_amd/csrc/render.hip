// render.hip -- the output half of the pipeline on the GPU: save_results (reference src/data/utils.py:195-235) with its paste helper
// get_img_mask_union_pil (src/models/smp/utils.py:203-213) and the class colours / ids of src/data/utils.py:16-43.
//
// Per frame and per class, in list order, the reference closes the class's 0/1 mask with the 5x5 ellipse (cv2.morphologyEx MORPH_CLOSE),
// takes ring = dilate7(m) with erode7(m) > 0 cleared, blurs m with GaussianBlur((5,5), 0) (the fixed (1,4,6,4,1)/16 kernel per axis,
// BORDER_REFLECT_101; on a 0/1 mask the result is k / 256 with an integer k), and pastes the class colour into the frame twice through PIL:
// once with alpha = uint8(b * 64 * 0.85 * 255) and once with alpha = uint8(ring * 255 * 0.85 * 255) -- both products exceed 255 and the cast
// wraps, which is why a class's interior gets alpha 48 and the ring alpha 231.  The colour mask starts (128,128,128) and takes the class colour
// where the RAW mask is set.  Everything is integer: the 257 possible blur alphas come from the host as a table (postprocess.alpha_table),
// PIL's paste is t = in * (255 - a) + col * a + 128; out = ((t >> 8) + t) >> 8.  The outputs EQUAL the reference's -- no tolerance.
//
// render_kernel: one 256-thread workgroup per 96 x 32 pixel tile of one frame, grid-stride over the tiles.  Masks live in LDS as BIT PLANES: a
// tile row with its halo (16 columns and 15 rows on every side: the chain reaches 4 * close_iterations + 3 <= 15 pixels) is one 128-bit word.
//   (A) a wave loads 64 pixels of the stack (one float4 per lane where the stack has four channels) and a ballot of `v != 0` per class is half a
//       row word: the 16 B / pixel stack is read once per tile and leaves as 1 bit per pixel and class;
//   (B) dilation by a structuring-element row of width 2h + 1 is the OR of the word shifted by -h..h, rows of equal width are ORed first; erosion
//       the same with AND.  One thread makes one row of one class per stage; all classes go through a stage together (one barrier per stage).
//       OpenCV's morphology border is "outside the frame does not take part", so every stage READS its source through the frame mask: outside
//       positions are 0 for a dilation and 1 for an erosion whatever the stage before wrote there (a dilation sets halo positions outside the
//       frame, and the next stage must not see that).  What the shifts bring in at the tile's own edge is wrong and stays inside the halo;
//   (C) a thread takes 4 consecutive pixels of a row: 12 bytes of the frame are three dwords, kept in registers through the class loop (blur sum
//       from five row words, reflect-101 taken from the in-frame closed mask, two pastes), and leave as three dwords per output.  Rows whose
//       byte offset is not a multiple of 4 (W % 4 != 0 or unaligned tensors) take byte loads and stores.  A class whose mask bits under the
//       four pixels' taps are all clear is skipped, all set means k = 256: the weighted sums are paid only near a class's border.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace octseg {

namespace {

constexpr int TW = 96, TH = 32, NT = 256;       // pixels a tile renders, threads per workgroup
constexpr int XH = 16, YH = 15;                 // halo columns / rows on each side; reach of the chain = 4 * 3 + 3 = 15
constexpr int RH = TH + 2 * YH;                 // rows of a bit plane
constexpr int MAXC = 16;
static_assert(TW + 2 * XH == 128, "a plane row is one 128-bit word");
static_assert((TW / 4) * TH % NT == 0, "phase C: whole rounds of quads");

typedef unsigned long long u64;
struct B128 { u64 lo, hi; };   // bit i of lo = tile column i, bit j of hi = tile column 64 + j

__device__ __forceinline__ B128 bor(B128 a, B128 b) { return {a.lo | b.lo, a.hi | b.hi}; }
__device__ __forceinline__ B128 band(B128 a, B128 b) { return {a.lo & b.lo, a.hi & b.hi}; }
__device__ __forceinline__ B128 bnot(B128 a) { return {~a.lo, ~a.hi}; }
__device__ __forceinline__ B128 up(B128 a, int s) { return {a.lo << s, (a.hi << s) | (a.lo >> (64 - s))}; }     // towards higher x, 0 < s < 64
__device__ __forceinline__ B128 down(B128 a, int s) { return {(a.lo >> s) | (a.hi << (64 - s)), a.hi >> s}; }
// bits [a, b) of the row word, clipped to it
__device__ __forceinline__ u64 span64(int a, int b) {
  a = max(a, 0); b = min(b, 64);
  if (a >= b) return 0ull;
  return (b - a == 64) ? ~0ull : (((1ull << (b - a)) - 1ull) << a);
}

// the OR (ero = false) / AND (ero = true) of the word over horizontal offsets -h..h
template <bool ERO>
__device__ __forceinline__ B128 hspan(B128 w, int h) {
  B128 r = w;
  for (int s = 1; s <= h; ++s) {
    if (ERO) r = band(r, band(up(w, s), down(w, s)));
    else r = bor(r, bor(up(w, s), down(w, s)));
  }
  return r;
}

struct Tile {
  int y0, H;        // frame row of plane row 0, frame height
  B128 in;          // columns of the tile that lie inside the frame
};

// row r of a plane as a stage sees it: outside the frame = the stage's neutral value.  r beyond the plane (only reached from halo rows, whose
// results are never used) is clamped
template <bool ERO>
__device__ __forceinline__ B128 rd(const u64* plane, int r, const Tile& t) {
  r = min(max(r, 0), RH - 1);
  const int gy = t.y0 + r;
  if (gy < 0 || gy >= t.H) return ERO ? B128{~0ull, ~0ull} : B128{0ull, 0ull};
  const B128 w = {plane[2 * r], plane[2 * r + 1]};
  return ERO ? bor(w, bnot(t.in)) : band(w, t.in);
}

template <bool ERO>
__device__ __forceinline__ B128 comb(B128 a, B128 b) { return ERO ? band(a, b) : bor(a, b); }

// cv2.getStructuringElement(MORPH_ELLIPSE, (5, 5)): row widths 1, 5, 5, 5, 1
template <bool ERO>
__device__ __forceinline__ B128 morph5(const u64* p, int r, const Tile& t) {
  const B128 edge = comb<ERO>(rd<ERO>(p, r - 2, t), rd<ERO>(p, r + 2, t));
  const B128 mid = comb<ERO>(comb<ERO>(rd<ERO>(p, r - 1, t), rd<ERO>(p, r, t)), rd<ERO>(p, r + 1, t));
  return comb<ERO>(edge, hspan<ERO>(mid, 2));
}
// (7, 7): row widths 1, 5, 7, 7, 7, 5, 1
template <bool ERO>
__device__ __forceinline__ B128 morph7(const u64* p, int r, const Tile& t) {
  const B128 e3 = comb<ERO>(rd<ERO>(p, r - 3, t), rd<ERO>(p, r + 3, t));
  const B128 e2 = comb<ERO>(rd<ERO>(p, r - 2, t), rd<ERO>(p, r + 2, t));
  const B128 mid = comb<ERO>(comb<ERO>(rd<ERO>(p, r - 1, t), rd<ERO>(p, r, t)), rd<ERO>(p, r + 1, t));
  return comb<ERO>(comb<ERO>(e3, hspan<ERO>(e2, 2)), hspan<ERO>(mid, 3));
}

// cv::borderInterpolate(p, len, BORDER_REFLECT_101)
__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

// 16 bits of a plane row from tile column s on (0 <= s <= 112)
__device__ __forceinline__ unsigned bits16(const u64* plane, int r, int s) {
  const u64 lo = plane[2 * r], hi = plane[2 * r + 1];
  const u64 v = s >= 64 ? hi >> (s - 64) : (s ? (lo >> s) | (hi << (64 - s)) : lo);
  return (unsigned)v & 0xffffu;
}
__device__ __forceinline__ unsigned bit1(const u64* plane, int r, int s) {
  s = min(max(s, 0), 127);
  return (unsigned)(plane[2 * r + (s >> 6)] >> (s & 63)) & 1u;
}
// (1, 4, 6, 4, 1) over five mask bits
__device__ __forceinline__ int hsum5(unsigned b) {
  return (int)((b & 1u) + ((b >> 4) & 1u) + 4u * (((b >> 1) & 1u) + ((b >> 3) & 1u)) + 6u * ((b >> 2) & 1u));
}
// PIL's paste of a solid colour through an L mask (ImagingPaste / MULDIV255 + BLEND8)
__device__ __forceinline__ unsigned paste(unsigned in, unsigned col, unsigned a) {
  const unsigned t = in * (255u - a) + col * a + 128u;
  return ((t >> 8) + t) >> 8;
}

}  // namespace

// Dynamic LDS: three sets of C bit planes [C][RH][2] u64 (raw mask; two that the stages alternate between), then the 257-entry alpha table, the
// class colours [MAXC][3] and the class channels [MAXC].
__global__ __launch_bounds__(NT) void render_kernel(const float* __restrict__ stack, const uint8_t* __restrict__ frames, int N, int H, int W, int SC,
                                                    const int* __restrict__ class_ch, const uint8_t* __restrict__ class_rgb, int C,
                                                    const uint8_t* __restrict__ alpha_tab, int ring_alpha, int iters,
                                                    uint8_t* __restrict__ overlay, uint8_t* __restrict__ cmask, int vec_stack, int vec_rgb) {
  extern __shared__ __align__(16) u64 smem[];
  const int plane_words = RH * 2, set_words = C * plane_words;
  u64* raw = smem;
  u64* bufa = smem + set_words;
  u64* bufb = smem + 2 * set_words;
  uint8_t* tab = (uint8_t*)(smem + 3 * set_words);      // [257], padded to 272
  uint8_t* rgb = tab + 272;                             // [MAXC][3]
  int* chs = (int*)(rgb + MAXC * 3);                    // [MAXC]; 272 + 48 bytes: 4-byte aligned
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int i = tid; i < 257; i += NT) tab[i] = alpha_tab[i];
  if (tid < C) {
    chs[tid] = min(max(class_ch[tid], 0), SC - 1);
    rgb[tid * 3] = class_rgb[tid * 3]; rgb[tid * 3 + 1] = class_rgb[tid * 3 + 1]; rgb[tid * 3 + 2] = class_rgb[tid * 3 + 2];
  }
  __syncthreads();

  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const size_t total = (size_t)N * tiles_x * tiles_y;
  for (size_t t = blockIdx.x; t < total; t += gridDim.x) {
    const int ox = (int)(t % tiles_x) * TW, oy = (int)((t / tiles_x) % tiles_y) * TH;
    const size_t n = t / ((size_t)tiles_x * tiles_y);
    const int x0 = ox - XH;
    Tile tile;
    tile.y0 = oy - YH; tile.H = H;
    tile.in.lo = span64(-x0, W - x0);
    tile.in.hi = span64(-x0 - 64, W - x0 - 64);

    // ---- (A) stack -> raw bit planes.  A wave takes (row, half) items; eight items' loads are issued before the first ballot.  Only what the
    // chain reaches from the tile (4 * iters + 3 pixels) is loaded; the rest of the halo is stored as 0 and never reaches a rendered pixel
    const int reach = 4 * iters + 3;
    for (int base = wave; base < RH * 2; base += 8 * (NT / 64)) {
      float4 v[8];
      bool ok[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int item = base + k * (NT / 64);
        const int r = item >> 1, gy = tile.y0 + r, lx = (item & 1) * 64 + lane, gx = x0 + lx;
        ok[k] = item < RH * 2 && r >= YH - reach && r < YH + TH + reach && lx >= XH - reach && lx < XH + TW + reach && gy >= 0 && gy < H &&
                gx >= 0 && gx < W;
        v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[k] && vec_stack) v[k] = *(const float4*)(stack + ((n * H + gy) * W + gx) * 4);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int item = base + k * (NT / 64);
        if (item >= RH * 2) break;                       // wave-uniform
        const int r = item >> 1, gy = tile.y0 + r, gx = x0 + (item & 1) * 64 + lane;
        for (int c = 0; c < C; ++c) {
          const int ch = chs[c];
          float f;
          if (vec_stack) f = ch == 0 ? v[k].x : ch == 1 ? v[k].y : ch == 2 ? v[k].z : v[k].w;
          else f = ok[k] ? stack[((n * H + gy) * W + gx) * SC + ch] : 0.f;
          const u64 word = __ballot(f != 0.f);
          if (lane == 0) raw[c * plane_words + item] = word;
        }
      }
    }
    __syncthreads();

    // ---- (B) closing: iters dilations, iters erosions (5 x 5 ellipse); then ring = dilate7(m) & ~erode7(m).  m ends in bufb, ring in bufa
    {
      const u64* src = raw;
      u64* dst = bufa;
      for (int s = 0; s < 2 * iters; ++s) {
        for (int i = tid; i < C * RH; i += NT) {
          const int c = i / RH, r = i - c * RH;
          const B128 o = s < iters ? morph5<false>(src + c * plane_words, r, tile) : morph5<true>(src + c * plane_words, r, tile);
          dst[c * plane_words + 2 * r] = o.lo;
          dst[c * plane_words + 2 * r + 1] = o.hi;
        }
        __syncthreads();
        src = dst;
        dst = dst == bufa ? bufb : bufa;
      }
      for (int i = tid; i < C * RH; i += NT) {
        const int c = i / RH, r = i - c * RH;
        const B128 o = band(morph7<false>(bufb + c * plane_words, r, tile), bnot(morph7<true>(bufb + c * plane_words, r, tile)));
        bufa[c * plane_words + 2 * r] = o.lo;
        bufa[c * plane_words + 2 * r + 1] = o.hi;
      }
      __syncthreads();
    }

    // ---- (C) blend: 4 pixels per thread
    for (int q = tid; q < (TW / 4) * TH; q += NT) {
      const int qx = q % (TW / 4), qy = q / (TW / 4);
      const int gx = ox + qx * 4, gy = oy + qy;
      if (gy >= H || gx >= W) continue;
      const int np = min(4, W - gx);
      const size_t off = ((n * H + gy) * W + gx) * 3;
      unsigned px[4][3], cm[4][3];
      if (vec_rgb) {                                     // W % 4 == 0: np == 4 and off % 4 == 0
        const uint32_t* p = (const uint32_t*)(frames + off);
        const uint32_t d0 = p[0], d1 = p[1], d2 = p[2];
        px[0][0] = d0 & 255u; px[0][1] = (d0 >> 8) & 255u; px[0][2] = (d0 >> 16) & 255u;
        px[1][0] = d0 >> 24; px[1][1] = d1 & 255u; px[1][2] = (d1 >> 8) & 255u;
        px[2][0] = (d1 >> 16) & 255u; px[2][1] = d1 >> 24; px[2][2] = d2 & 255u;
        px[3][0] = (d2 >> 8) & 255u; px[3][1] = (d2 >> 16) & 255u; px[3][2] = d2 >> 24;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int k = 0; k < 3; ++k) px[j][k] = j < np ? frames[off + j * 3 + k] : 0u;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) cm[j][0] = cm[j][1] = cm[j][2] = 128u;
      const int lr = qy + YH, lx = qx * 4 + XH;
      const bool inner = gx >= 2 && gx + 5 < W;          // every tap column of the four pixels is inside the frame
      int ry[5];
#pragma unroll
      for (int d = 0; d < 5; ++d) ry[d] = min(max(reflect101(gy + d - 2, H) - tile.y0, 0), RH - 1);
      for (int c = 0; c < C; ++c) {
        const u64* pm = bufb + c * plane_words;
        const unsigned cr = rgb[c * 3], cg = rgb[c * 3 + 1], cb = rgb[c * 3 + 2];
        const unsigned ring = bits16(bufa + c * plane_words, lr, lx) & 15u, rw = bits16(raw + c * plane_words, lr, lx) & 15u;
        // the eight mask columns under the four pixels' taps, per tap row.  Most pixels are far from the class's border: all taps clear (the
        // class does not touch them) or all set (k = 256); only the rest pays for the weighted sums
        unsigned bw[5], any = 0u, all = 0xffu;
        if (inner) {
#pragma unroll
          for (int d = 0; d < 5; ++d) {
            bw[d] = bits16(pm, ry[d], lx - 2) & 0xffu;
            any |= bw[d];
            all &= bw[d];
          }
          if (!(any | ring | rw)) continue;
        }
        int k[4];
        if (inner && (any == 0u || all == 0xffu)) {
#pragma unroll
          for (int j = 0; j < 4; ++j) k[j] = any ? 256 : 0;
        } else {
          int hs[5][4];
#pragma unroll
          for (int d = 0; d < 5; ++d) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              unsigned b = 0;
              if (inner) {
                b = (bw[d] >> j) & 31u;
              } else {
#pragma unroll
                for (int e = 0; e < 5; ++e) b |= bit1(pm, ry[d], reflect101(gx + j + e - 2, W) - x0) << e;
              }
              hs[d][j] = hsum5(b);
            }
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) k[j] = hs[0][j] + hs[4][j] + 4 * (hs[1][j] + hs[3][j]) + 6 * hs[2][j];      // 0..256
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned a1 = tab[k[j]], a2 = ((ring >> j) & 1u) ? (unsigned)ring_alpha : 0u;
          if (a1 | a2) {                                 // a paste with alpha 0 changes nothing
            px[j][0] = paste(paste(px[j][0], cr, a1), cr, a2);
            px[j][1] = paste(paste(px[j][1], cg, a1), cg, a2);
            px[j][2] = paste(paste(px[j][2], cb, a1), cb, a2);
          }
          if ((rw >> j) & 1u) { cm[j][0] = cr; cm[j][1] = cg; cm[j][2] = cb; }
        }
      }
      if (vec_rgb) {
        uint32_t* o = (uint32_t*)(overlay + off);
        o[0] = px[0][0] | (px[0][1] << 8) | (px[0][2] << 16) | (px[1][0] << 24);
        o[1] = px[1][1] | (px[1][2] << 8) | (px[2][0] << 16) | (px[2][1] << 24);
        o[2] = px[2][2] | (px[3][0] << 8) | (px[3][1] << 16) | (px[3][2] << 24);
        uint32_t* m = (uint32_t*)(cmask + off);
        m[0] = cm[0][0] | (cm[0][1] << 8) | (cm[0][2] << 16) | (cm[1][0] << 24);
        m[1] = cm[1][1] | (cm[1][2] << 8) | (cm[2][0] << 16) | (cm[2][1] << 24);
        m[2] = cm[2][2] | (cm[3][0] << 8) | (cm[3][1] << 16) | (cm[3][2] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < np) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              overlay[off + j * 3 + k] = (uint8_t)px[j][k];
              cmask[off + j * 3 + k] = (uint8_t)cm[j][k];
            }
          }
      }
    }
    __syncthreads();   // the next tile of this workgroup overwrites the planes
  }
}

size_t render_lds_bytes(int C) { return (size_t)3 * C * RH * 2 * sizeof(u64) + 272 + MAXC * 3 + MAXC * sizeof(int); }

hipError_t launch_render_results(const float* stack, const uint8_t* frames, int N, int H, int W, int SC, const int* class_ch,
                                 const uint8_t* class_rgb, int C, const uint8_t* alpha_tab, int ring_alpha, int iters, uint8_t* overlay,
                                 uint8_t* cmask, hipStream_t st) {
  const size_t tiles = (size_t)N * ((W + TW - 1) / TW) * ((H + TH - 1) / TH);
  const int vec_stack = (SC == 4 && ((uintptr_t)stack & 15) == 0) ? 1 : 0;
  const int vec_rgb = (W % 4 == 0 && (((uintptr_t)frames | (uintptr_t)overlay | (uintptr_t)cmask) & 3) == 0) ? 1 : 0;
  hipLaunchKernelGGL(render_kernel, dim3((unsigned)std::min<size_t>(tiles, 1u << 20)), dim3(NT), render_lds_bytes(C), st, stack, frames, N, H, W, SC,
                     class_ch, class_rgb, C, alpha_tab, ring_alpha & 255, iters, overlay, cmask, vec_stack, vec_rgb);
  return hipGetLastError();
}

}  // namespace octseg
