// skeleton.hip -- the centreline of every plane of a mask stack by parallel thinning, and the census of what is left: set and skeleton pixels, end,
// junction and isolated points, passes.  No reference counterpart: the reference measures thickness along rays only (DESIGN.md section 5q states the
// definitions).  The width at the centreline is the distance family's d2 for dst_part = clear at the skeleton's pixels: no distance code here.
//
// A plane is one (slice, channel) pair of the float32 stack [N][H][W][C], any value != 0 set, everything outside the frame clear.  Planes live as
// the bit planes of bitplanes.h, every plane on its own (D = 1); pack and unpack are the shared kernels of bitplanes.hip.  The rule is Guo and
// Hall's two-sub-iteration thinning (1989, algorithm A1), booleans as 0 / 1, P2 .. P9 the neighbours clockwise from north:
//
//   C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
//   N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8)        N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9)
//   m  = sub-iteration 0: (P6 | P7 | !P9) & P8         sub-iteration 1: (P2 | P3 | !P5) & P4
//   delete a set pixel iff  C == 1  and  2 <= min(N1, N2) <= 3  and  m == 0
//
// Pure boolean, so it is evaluated on the 64 pixels of a word per operation: N, S = the words of rows y -+ 1, E = (w >> 1) | (next << 63),
// W = (w << 1) | (prev >> 63), the diagonals the same shifts of the rows above and below; sums of four booleans are compared through
// ge2(a, b, c, d) = "two or more" and the all-four AND.  An all-zero word has nothing to delete and is skipped.
//
//   thin (LDS)     skel_thin_lds_kernel<K>: one workgroup per plane, all passes in one launch.  The plane sits in ONE LDS image for the whole thinning
//                  (two images of 1024^2 would not fit 160 KiB), PADDED so that no read needs a bounds check: a row is pitch = W64 + 1 words, the
//                  last always zero -- it is the right neighbour of its own row and the left neighbour of the next --, a zero row above and below and
//                  one leading zero word: word (y, j) at 1 + (y + 1) * pitch + j of (H + 2) * pitch + 1 words (750^2: 76 KB, 1024^2: 136 KB).
//                  Thread t owns the positions 1 + pitch + t, + NT, ... of rows 0 .. H - 1, at most K of them (pad words are zero and skipped like
//                  any zero word); a sub-iteration computes the deletion mask of each into registers (K statically indexed u64), a barrier ends
//                  all reads, the owners clear their bits, a second barrier ends all writes.  "Any pixel deleted" is one of two LDS flags used in
//                  turn: set between the barriers, read after the second, cleared by thread 0 during the next sub-iteration's write phase.
//                  NT = the positions rounded up to a wave, at most 1024: at 1024 threads a 1024^2 plane is K = 17 words = 34 VGPRs of masks per
//                  thread, where 256 threads would need 136; more waves also hide the LDS latency of the nine reads per word.
//   thin (global)  skel_thin_global_kernel: a plane whose padded image is above 20478 words (up to 4096 x 4096), or any plane with flag bit 0: the same loop by the same
//                  single workgroup, every sub-iteration reading one image and writing all words of the other (input -> skel -> tmp -> skel ...),
//                  __syncthreads between them (one workgroup = one CU: its waves share the L1, workgroup-scope ordering suffices).  Bounded and
//                  correct, not tuned.
//   census         skel_census_kernel: a wave per 64 words of a plane, a thread per word over the input bits and the skeleton bits.  The number of
//                  skeleton neighbours of all 64 pixels comes from a bit-sliced adder over the eight neighbour words (three adders of ones, one of
//                  twos); popcounts are summed over the wave by shuffles, then one integer atomic per wave and column that is not zero.
//
// TERMINATION.  A productive pass clears at least one bit of a finite plane and no bit is ever set, so there are at most H * W productive passes; the
// pass loop ends on the first idle pass (both flags read 0 by every thread after a barrier: the exit is uniform).  One plane belongs to one
// workgroup, so no workgroup waits on another: no spin, no flag between workgroups, no cooperative launch, no inline assembly.
//
// BOUNDS.  LDS path: an owned position p lies in [1 + pitch, 1 + (H + 1) * pitch) (checked), and the neighbours p +- 1, p +- pitch, p +- pitch +- 1
// of a position that holds a set bit (a real word, never a pad) lie in [0, (H + 2) * pitch], the image.  Global path: every word index is checked
// against [0, words) before the access, and words left and right of a row read as zero.  Bits past the frame are zero in the packed planes and
// only ever cleared.
#include <algorithm>

#include "bitplanes.h"
#include "kernels.h"

namespace octseg {

namespace {

constexpr int SK_NT = 1024;                                    // the most threads of a thinning workgroup
constexpr int SK_KMAX = 20;                                    // words a thread owns at most on the LDS path
constexpr int SK_LDS_BYTES = 160 * 1024;
constexpr int SK_LDS_WORDS = (SK_LDS_BYTES - 16) / 8;          // the padded image; two flags and the first owned position behind it
static_assert(SK_LDS_WORDS <= SK_KMAX * SK_NT, "a thread owns at most SK_KMAX words");

// the padded LDS image of a plane: its words, or 0 when it does not fit
inline int lds_image_words(int H, int W) {
  const size_t n = ((size_t)H + 2) * (((size_t)W + 63) / 64 + 1) + 1;
  return n <= (size_t)SK_LDS_WORDS ? (int)n : 0;
}

__device__ __forceinline__ u64 ge2(u64 a, u64 b, u64 c, u64 d) { return (a & b) | (c & d) | ((a | b) & (c | d)); }

// the pixels of word w that sub-iteration `sub` deletes.  n, s: the words above and below; p / x suffix: the word before / after in the same row
__device__ __forceinline__ u64 thin_rule(u64 w, u64 wp, u64 wx, u64 n, u64 np, u64 nx, u64 s, u64 sp, u64 sx, int sub) {
  const u64 p2 = n, p3 = (n >> 1) | (nx << 63), p4 = (w >> 1) | (wx << 63), p5 = (s >> 1) | (sx << 63);
  const u64 p6 = s, p7 = (s << 1) | (sp >> 63), p8 = (w << 1) | (wp >> 63), p9 = (n << 1) | (np >> 63);
  const u64 a1 = p9 | p2, a2 = p3 | p4, a3 = p5 | p6, a4 = p7 | p8;
  const u64 b1 = p2 | p3, b2 = p4 | p5, b3 = p6 | p7, b4 = p8 | p9;
  const u64 c1 = ~p2 & a2, c2 = ~p4 & a3, c3 = ~p6 & a4, c4 = ~p8 & a1;
  const u64 one = (c1 ^ c2 ^ c3 ^ c4) & ~ge2(c1, c2, c3, c4);
  const u64 range = ge2(a1, a2, a3, a4) & ge2(b1, b2, b3, b4) & (~(a1 & a2 & a3 & a4) | ~(b1 & b2 & b3 & b4));
  const u64 m = sub ? ((p2 | p3 | ~p5) & p4) : ((p6 | p7 | ~p9) & p8);
  return w & one & range & ~m;
}

// word i of an image of `words` words, zero outside it
__device__ __forceinline__ u64 rd(const u64* img, int i, int words) { return (i >= 0 && i < words) ? img[i] : 0ull; }

// the deletion mask of word i (0 <= i < words); left / right: the word is the first / last of its row
__device__ __forceinline__ u64 thin_word(const u64* img, int i, int W64, int words, bool left, bool right, int sub) {
  const u64 w = img[i];
  if (!w) return 0ull;
  const int up = i - W64, dn = i + W64;
  const u64 n = rd(img, up, words), s = rd(img, dn, words);
  const u64 wp = left ? 0ull : rd(img, i - 1, words), np = left ? 0ull : rd(img, up - 1, words), sp = left ? 0ull : rd(img, dn - 1, words);
  const u64 wx = right ? 0ull : rd(img, i + 1, words), nx = right ? 0ull : rd(img, up + 1, words), sx = right ? 0ull : rd(img, dn + 1, words);
  return thin_rule(w, wp, wx, n, np, nx, s, sp, sx, sub);
}

}  // namespace

// ---- thinning from LDS: a workgroup per plane (grid-stride over the planes), blockDim.x * K >= H * pitch, the padded image of `total` words
// fits LDS.  passes (may be null): passes[plane * pstride] = the productive passes
template <int K>
__global__ __launch_bounds__(SK_NT) void skel_thin_lds_kernel(const u64* __restrict__ src, u64* __restrict__ dst, size_t P, BitGeo g, int total,
                                                               int* __restrict__ passes, int pstride) {
  extern __shared__ u64 sk_img[];
  const int words = g.H * g.W64, W64 = g.W64, pitch = W64 + 1, nt = blockDim.x, tid = threadIdx.x;
  const int first = 1 + pitch, end = 1 + (g.H + 1) * pitch;   // the positions of rows 0 .. H - 1, pad words included
  int* flag = (int*)(sk_img + total);
  for (size_t pl = blockIdx.x; pl < P; pl += gridDim.x) {
    const u64* in = src + pl * words;
    for (int p = tid; p < total; p += nt) {
      const int r = (p - 1) / pitch - 1, j = (p - 1) % pitch;  // p = 0: r = -1, a pad
      sk_img[p] = (p >= first && r < g.H && j < W64) ? in[r * W64 + j] : 0ull;
    }
    if (tid == 0) { flag[0] = 0; flag[1] = 0; flag[2] = first; }
    __syncthreads();
    int npass = 0;
    for (;;) {
      int hit = 0;
#pragma unroll
      for (int sub = 0; sub < 2; ++sub) {
        // the first position comes from LDS every sub-iteration: a value the compiler knows to be loop-invariant has the 3 K addresses of the
        // owned words and their rows above and below kept live across the whole loop, and with the K masks they do not fit 128 VGPRs
        const int mine = flag[2] + tid;
        u64 del[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int p = mine + k * nt;
          u64 d = 0ull;
          if (p < end) {
            const u64 w = sk_img[p];
            if (w) {                                           // a real word: its eight neighbours lie inside the image
              const u64* up = sk_img + p - pitch;
              const u64* dn = sk_img + p + pitch;
              d = thin_rule(w, sk_img[p - 1], sk_img[p + 1], up[0], up[-1], up[1], dn[0], dn[-1], dn[1], sub);
            }
          }
          del[k] = d;
        }
        __syncthreads();                                       // every read of this sub-iteration is done
        if (tid == 0) flag[sub ^ 1] = 0;                       // last read after the previous second barrier, next set after this one's
        u64 any = 0ull;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          if (del[k]) sk_img[mine + k * nt] &= ~del[k];        // del[k] != 0 only at a position that was in range
          any |= del[k];
        }
        if (any) flag[sub] = 1;
        __syncthreads();                                       // every write is done
        hit |= flag[sub];
      }
      if (!hit) break;                                         // uniform: every thread read the same two flags
      ++npass;
    }
    u64* out = dst + pl * words;
    for (int i = tid; i < words; i += nt) out[i] = sk_img[first + (i / W64) * pitch + i % W64];
    if (tid == 0 && passes) passes[pl * pstride] = npass;
    __syncthreads();                                           // the image and the flags are reused by the next plane
  }
}

// ---- thinning over images in global memory: a workgroup per plane, any size.  src is only read; the result ends in dst, tmp is the other image
__global__ __launch_bounds__(SK_NT) void skel_thin_global_kernel(const u64* __restrict__ src, u64* dst, u64* tmp, size_t P, BitGeo g,
                                                                  int* __restrict__ passes, int pstride) {
  // one barrier per sub-iteration, so three flags in turn: flag[f] is set before barrier t and read after it; thread 0 clears it again in
  // sub-iteration t + 2, when every thread has passed barrier t + 1 and so has read it, and before barrier t + 2, after which it is next set
  __shared__ int flag[3];
  const int words = g.H * g.W64, W64 = g.W64, nt = blockDim.x, tid = threadIdx.x;
  for (size_t pl = blockIdx.x; pl < P; pl += gridDim.x) {
    const u64* cur = src + pl * words;
    u64* a = dst + pl * words;
    u64* b = tmp + pl * words;
    if (tid == 0) { flag[0] = 0; flag[1] = 0; flag[2] = 0; }
    __syncthreads();
    int npass = 0, f = 0;
    for (;;) {
      int hit = 0;
      for (int sub = 0; sub < 2; ++sub) {
        const int fnext = f == 2 ? 0 : f + 1;
        if (tid == 0) flag[fnext] = 0;
        u64 any = 0ull;
        for (int i = tid; i < words; i += nt) {
          const int j = i % W64;
          const u64 del = thin_word(cur, i, W64, words, j == 0, j == W64 - 1, sub);
          a[i] = cur[i] & ~del;
          any |= del;
        }
        if (any) flag[f] = 1;
        __syncthreads();                                       // the new image is complete and visible to the workgroup
        hit |= flag[f];
        f = fnext;
        cur = a;
        u64* t = a; a = b; b = t;
      }
      if (!hit) break;
      ++npass;
    }
    // an even number of sub-iterations ran: input -> dst -> tmp -> dst -> ... leaves the result in tmp
    u64* out = dst + pl * words;
    for (int i = tid; i < words; i += nt) out[i] = cur[i];
    if (tid == 0 && passes) passes[pl * pstride] = npass;
    __syncthreads();
  }
}

// ---- census: a wave per 64 words of a plane.  census int32 [P][6], columns 0 .. 4 added to (cleared by the caller), column 5 written by the thinning
__global__ __launch_bounds__(NT) void skel_census_kernel(const u64* __restrict__ raw, const u64* __restrict__ skel, size_t P, BitGeo g,
                                                          int* __restrict__ census) {
  const int words = g.H * g.W64, chunks = (words + 63) / 64, lane = threadIdx.x & 63;
  const size_t total = P * chunks, nwaves = (size_t)gridDim.x * WAVES;
  for (size_t it = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < total; it += nwaves) {
    const size_t pl = it / chunks;
    const int i = (int)(it % chunks) * 64 + lane;
    int v[5] = {0, 0, 0, 0, 0};
    if (i < words) {
      const u64* sp = skel + pl * words;
      const u64 s = sp[i];
      v[0] = __popcll(raw[pl * words + i]);
      if (s) {
        const int y = i / g.W64, j = i % g.W64;
        const u64 n = rdw(sp, y - 1, j, g), np = rdw(sp, y - 1, j - 1, g), nx = rdw(sp, y - 1, j + 1, g);
        const u64 d = rdw(sp, y + 1, j, g), dp = rdw(sp, y + 1, j - 1, g), dx = rdw(sp, y + 1, j + 1, g);
        const u64 wp = rdw(sp, y, j - 1, g), wx = rdw(sp, y, j + 1, g);
        const u64 x0 = n, x1 = (n >> 1) | (nx << 63), x2 = (s >> 1) | (wx << 63), x3 = (d >> 1) | (dx << 63);
        const u64 x4 = d, x5 = (d << 1) | (dp >> 63), x6 = (s << 1) | (wp >> 63), x7 = (n << 1) | (np >> 63);
        // three adders of ones (carries t0 .. t2), their sums added again (carry t3): count = bit0 + 2 * (t0 + t1 + t2 + t3)
        const u64 s0 = x0 ^ x1 ^ x2, t0 = (x0 & x1) | (x2 & (x0 ^ x1));
        const u64 s1 = x3 ^ x4 ^ x5, t1 = (x3 & x4) | (x5 & (x3 ^ x4));
        const u64 s2 = x6 ^ x7, t2 = x6 & x7;
        const u64 bit0 = s0 ^ s1 ^ s2, t3 = (s0 & s1) | (s2 & (s0 ^ s1));
        const u64 twos = t0 | t1 | t2 | t3;                                          // count >= 2
        const u64 two = ~bit0 & (t0 ^ t1 ^ t2 ^ t3) & ~ge2(t0, t1, t2, t3);          // count == 2
        v[1] = __popcll(s);
        v[2] = __popcll(s & bit0 & ~twos);                                           // count == 1
        v[3] = __popcll(s & twos & ~two);                                            // count >= 3
        v[4] = __popcll(s & ~bit0 & ~twos);                                          // count == 0
      }
    }
#pragma unroll
    for (int c = 0; c < 5; ++c) {
      int t = v[c];
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
      if (lane == 0 && t) atomicAdd(census + pl * 6 + c, t);
    }
  }
}

namespace {

struct SkelScratch {
  u64 *raw, *skel, *tmp;
  size_t bytes;
};

SkelScratch skel_carve(void* base, size_t N, int H, int W, int C) {
  SkelScratch s;
  const size_t words = (size_t)H * (((size_t)W + 63) / 64), P = N * C;
  Carver cv(base);
  s.raw = cv.take<u64>(P * words);
  s.skel = cv.take<u64>(P * words);
  s.tmp = cv.take<u64>(P * words);
  s.bytes = cv.used;
  return s;
}

template <int K>
hipError_t thin_lds(const SkelScratch& s, size_t P, const BitGeo& g, int nt, int total, int* passes, int pstride, hipStream_t st) {
  static bool set = false;
  if (!set) {
    hipError_t e = hipFuncSetAttribute((const void*)skel_thin_lds_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, SK_LDS_BYTES);
    if (e != hipSuccess) return e;
    set = true;
  }
  hipLaunchKernelGGL(skel_thin_lds_kernel<K>, dim3((unsigned)std::min<size_t>(P, MAX_GRID)), dim3(nt), (size_t)total * 8 + 16, st, s.raw, s.skel, P, g,
                     total, passes, pstride);
  return hipSuccess;
}

}  // namespace

size_t skeleton_scratch_bytes(size_t N, int H, int W, int C) { return skel_carve(nullptr, N, H, W, C).bytes; }

bool skeleton_fits_lds(int H, int W) { return lds_image_words(H, W) != 0; }

hipError_t launch_stack_skeleton(const float* stack, int N, int H, int W, int C, int force_global, void* scratch, float* out, int* census,
                                 hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const SkelScratch s = skel_carve(scratch, N, H, W, C);
  const size_t P = (size_t)N * C;
  const int words = g.H * g.W64, total = lds_image_words(H, W);
  hipError_t e = hipSuccess;
  if (census) e = hipMemsetAsync(census, 0, P * 6 * sizeof(int), st);
  if (e != hipSuccess) return e;
  launch_bits_pack(stack, N, g, C, C, 1, s.raw, st);
  int* passes = census ? census + 5 : nullptr;
  if (!force_global && total) {
    const int owned = g.H * (g.W64 + 1), nt = std::min(SK_NT, (owned + 63) / 64 * 64), k = (owned + nt - 1) / nt;
    if (k <= 1) e = thin_lds<1>(s, P, g, nt, total, passes, 6, st);
    else if (k <= 2) e = thin_lds<2>(s, P, g, nt, total, passes, 6, st);
    else if (k <= 4) e = thin_lds<4>(s, P, g, nt, total, passes, 6, st);
    else if (k <= 7) e = thin_lds<7>(s, P, g, nt, total, passes, 6, st);
    else if (k <= 10) e = thin_lds<10>(s, P, g, nt, total, passes, 6, st);
    else if (k <= 13) e = thin_lds<13>(s, P, g, nt, total, passes, 6, st);
    else if (k <= 17) e = thin_lds<17>(s, P, g, nt, total, passes, 6, st);
    else e = thin_lds<SK_KMAX>(s, P, g, nt, total, passes, 6, st);
    if (e != hipSuccess) return e;
  } else {
    hipLaunchKernelGGL(skel_thin_global_kernel, dim3((unsigned)std::min<size_t>(P, MAX_GRID)), dim3(SK_NT), 0, st, s.raw, s.skel, s.tmp, P, g, passes, 6);
  }
  if (census)
    hipLaunchKernelGGL(skel_census_kernel, dim3(wave_grid(P * ((words + 63) / 64))), dim3(NT), 0, st, s.raw, s.skel, P, g, census);
  if (out) launch_bits_unpack(s.skel, N, g, C, C, 1, out, st);
  return hipGetLastError();
}

}  // namespace octseg
