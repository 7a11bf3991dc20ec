// planepass.h -- the plane-pass core shared by skeleton.hip (thinning) and prune.hip (centreline pruning): one workgroup works on one bit plane of
// bitplanes.h (D = 1) in passes, every change of a pass decided on the plane as the pass found it, until a count runs out or a pass changes nothing.
// Here: the constants and the layout of the plane in LDS, the 3 x 3 neighbourhood of a word, the pass itself over the LDS image and over images in
// global memory, the neighbour-count classes and the wave sums of the census kernels, and the host side (the K ladder, the dynamic-LDS launch, the
// scratch planes).  The rules stay with the operation they define.
//
// WORDS.  Everything is boolean and evaluated on the 64 pixels of a word per operation.  P2 .. P9 are the neighbours clockwise from north: N, S =
// the words of rows y -+ 1, E = (w >> 1) | (next << 63), W = (w << 1) | (prev >> 63), the diagonals the same shifts of the rows above and below.
//
// THE LDS IMAGE.  The plane sits in ONE LDS image for all passes (two images of 1024^2 would not fit 160 KiB), PADDED so that no read needs a bounds
// check: a row is pitch = W64 + 1 words, the last always zero -- it is the right neighbour of its own row and the left neighbour of the next --, a
// zero row above and below and one leading zero word: word (y, j) at 1 + (y + 1) * pitch + j of (H + 2) * pitch + 1 words (750^2: 76 KB, 1024^2:
// 136 KB).  Thread t owns the positions first + t, + NT, ... of rows 0 .. H - 1 (first = 1 + pitch, end = 1 + (H + 1) * pitch), at most K of them,
// pad words included.  A pass computes the mask of each owned word into registers (K statically indexed u64), a barrier ends all reads, the owners
// apply their masks, a second barrier ends all writes.  NT = the positions rounded up to a wave, at most 1024: at 1024 threads a 1024^2 plane is
// K = 17 words = 34 VGPRs of masks per thread, where 256 threads would need 136; more waves also hide the LDS latency of the nine reads per word.
// Three words lie behind the image: two flags and the first owned position.
//
// FLAGS.  "This pass changed something" is one of two LDS flags used in turn: set between the two barriers of a pass, read by every thread after
// the second, cleared by thread 0 between the barriers of the next pass -- every thread has read it by then -- and next set after the first barrier
// of the pass after that.  A pass over images in global memory has one barrier, so there are three flags in turn: flag f is set before barrier t and
// read after it; thread 0 clears it again in pass t + 2, when every thread has passed barrier t + 1 and so has read it, and before barrier t + 2,
// after which it is next set.  Barriers a caller puts between two passes change nothing in either argument.
//
// TERMINATION.  A pass returns the same value in every thread (all read the same flag after the same barrier), so a loop that ends on it is left by
// all threads or by none; why each loop ends is argued where it is written.  One plane belongs to one workgroup, so no workgroup waits on another:
// no spin, no flag between workgroups, no cooperative launch, no inline assembly.
//
// BOUNDS.  LDS: a pass visits the owned positions p in [first, end - 1).  The position end - 1 = (H + 1) * pitch is the last row's pad: it is zero
// for ever, and its neighbours would end one word past the image.  For every visited p the nine words p, p +- 1, p +- pitch, p +- pitch +- 1 lie in
// [0, (H + 2) * pitch], the image; a CLEAR pass reads them only around a word that holds a set bit (a real word, never a pad).  A pad position has
// no word in the packed plane (packed_index = -1): it starts as zero, and every rule offers it nothing but zero.  Global memory: every word index is
// checked against [0, words) before the access, and the words left and right of a row read as zero.  Bits past the frame are zero in the packed
// planes and stay so: a plane here only loses bits or gains them inside a plane that has them zero.
#pragma once

#include <algorithm>
#include <type_traits>

#include "bitplanes.h"

namespace octseg {

namespace {

constexpr int PP_NT = 1024;                                    // the most threads of a plane's workgroup
constexpr int PP_KMAX = 20;                                    // words a thread owns at most on the LDS path
constexpr int PP_LDS_BYTES = 160 * 1024;
constexpr int PP_LDS_WORDS = (PP_LDS_BYTES - 16) / 8;          // the padded image; two flags and the first owned position behind it
static_assert(PP_LDS_WORDS <= PP_KMAX * PP_NT, "a thread owns at most PP_KMAX words");

// the padded LDS image of a plane: its words, or 0 when it does not fit
inline int lds_image_words(int H, int W) {
  const size_t n = ((size_t)H + 2) * (((size_t)W + 63) / 64 + 1) + 1;
  return n <= (size_t)PP_LDS_WORDS ? (int)n : 0;
}

// ---- the neighbourhood of a word

// two or more of four
__device__ __forceinline__ u64 ge2(u64 a, u64 b, u64 c, u64 d) { return (a & b) | (c & d) | ((a | b) & (c | d)); }

// a word and the eight around it.  n, s: the words above and below; p / x suffix: the word before / after in the same row
struct Nine {
  u64 w, wp, wx, n, np, nx, s, sp, sx;
};

// P2 .. P9 of the 64 pixels of a word
struct Ring {
  u64 p2, p3, p4, p5, p6, p7, p8, p9;
};

__device__ __forceinline__ Ring ring(const Nine& q) {
  return Ring{q.n, (q.n >> 1) | (q.nx << 63), (q.w >> 1) | (q.wx << 63), (q.s >> 1) | (q.sx << 63),
              q.s, (q.s << 1) | (q.sp >> 63), (q.w << 1) | (q.wp >> 63), (q.n << 1) | (q.np >> 63)};
}

// the words around word i (0 <= i < words, w its value) of an image in global memory: zero outside the image and past the ends of the row
__device__ __forceinline__ Nine nine_global(const u64* img, int i, int W64, int words, u64 w) {
  const int j = i % W64, up = i - W64, dn = i + W64;
  const bool left = j == 0, right = j == W64 - 1;
  auto rd = [&](int k) { return (k >= 0 && k < words) ? img[k] : 0ull; };
  return Nine{w, left ? 0ull : rd(i - 1), right ? 0ull : rd(i + 1), rd(up), left ? 0ull : rd(up - 1), right ? 0ull : rd(up + 1),
              rd(dn), left ? 0ull : rd(dn - 1), right ? 0ull : rd(dn + 1)};
}

// the pixels of w with exactly one, three or more, and none of their eight neighbours set: a bit-sliced counter
struct Counted {
  u64 one, many, none;
};

__device__ __forceinline__ Counted count_neighbours(u64 w, const Ring& r) {
  // three adders of ones (carries t0 .. t2), their sums added again (carry t3): count = bit0 + 2 * (t0 + t1 + t2 + t3)
  const u64 s0 = r.p2 ^ r.p3 ^ r.p4, t0 = (r.p2 & r.p3) | (r.p4 & (r.p2 ^ r.p3));
  const u64 s1 = r.p5 ^ r.p6 ^ r.p7, t1 = (r.p5 & r.p6) | (r.p7 & (r.p5 ^ r.p6));
  const u64 s2 = r.p8 ^ r.p9, t2 = r.p8 & r.p9;
  const u64 bit0 = s0 ^ s1 ^ s2, t3 = (s0 & s1) | (s2 & (s0 ^ s1));
  const u64 twos = t0 | t1 | t2 | t3;                                          // count >= 2
  const u64 two = ~bit0 & (t0 ^ t1 ^ t2 ^ t3) & ~ge2(t0, t1, t2, t3);          // count == 2
  return Counted{w & bit0 & ~twos, w & twos & ~two, w & ~bit0 & ~twos};
}

// v[c] summed over the wave and added to dst[c]: one integer atomic per column that is not zero
template <int NC>
__device__ __forceinline__ void wave_add_columns(const int (&v)[NC], int* dst) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    int t = v[c];
    for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
    if (lane == 0 && t) atomicAdd(dst + c, t);
  }
}

// ---- the plane in LDS

// what a pass does with the mask of a word.  CLEAR: image &= ~mask, zero words skipped (nothing to clear); SET: image |= mask; ASSIGN: image = mask
enum class Apply { CLEAR, SET, ASSIGN };

// a workgroup's padded LDS image (THE LDS IMAGE above).  The workgroup's dynamic LDS is `total` words + 16 bytes; blockDim.x * K >= H * pitch
struct LdsPlane {
  int* flag;                                                   // flag[0], flag[1]: FLAGS; flag[2]: first
  int total, pitch, first, end, nt, tid, par;                  // par: which flag the next pass sets

  // The image, by the LDS symbol itself and not through a pointer member: with the base known to be the start of LDS the compiler re-derives the
  // address of an owned word where it is used; from a pointer it kept the K addresses live across the barrier of a pass, a VGPR per owned word
  __device__ __forceinline__ static u64* img() {
    extern __shared__ u64 lds_plane_words[];
    return lds_plane_words;
  }

  __device__ __forceinline__ LdsPlane(const BitGeo& g, int total_) {
    flag = (int*)(img() + total_);
    total = total_, pitch = g.W64 + 1, first = 1 + pitch, end = 1 + (g.H + 1) * pitch, nt = blockDim.x, tid = threadIdx.x, par = 0;
  }

  // the index of position p (first <= p < end) in the packed plane, -1 for a pad
  __device__ __forceinline__ int packed_index(int p) const {
    const int r = (p - 1) / pitch - 1, j = (p - 1) % pitch;
    return j < pitch - 1 ? r * (pitch - 1) + j : -1;
  }

  // f(p, i) at every own position p that is a real word, i its index in the packed plane.  No neighbour is read: no barrier is needed around it
  // beyond the one that ended the last pass
  template <class F>
  __device__ __forceinline__ void each_word(F f) const {
    for (int p = first + tid; p < end; p += nt) {
      const int i = packed_index(p);
      if (i >= 0) f(p, i);
    }
  }

  // the image = the packed plane `in`, pads zero, flags clear.  Starts with a barrier: the last plane's image and flags are still being read
  __device__ __forceinline__ void load(const u64* __restrict__ in) {
    __syncthreads();
    for (int p = tid; p < total; p += nt) {
      const int i = (p >= first && p < end) ? packed_index(p) : -1;
      img()[p] = i >= 0 ? in[i] : 0ull;
    }
    if (tid == 0) { flag[0] = 0; flag[1] = 0; flag[2] = first; }
    par = 0;
    __syncthreads();
  }

  __device__ __forceinline__ void store(u64* __restrict__ out) const {
    each_word([&](int p, int i) { out[i] = img()[p]; });
  }

  // the words around position p (BOUNDS), w its value
  __device__ __forceinline__ Nine nine(int p, u64 w) const {
    const u64* up = img() + p - pitch;
    const u64* dn = img() + p + pitch;
    return Nine{w, img()[p - 1], img()[p + 1], up[0], up[-1], up[1], dn[0], dn[-1], dn[1]};
  }

  // One pass: mask = rule(p, w) for every owned position p (w the word there), all decided before any is applied.  Returns whether any mask of
  // the workgroup was not zero, the same value in every thread.
  template <int K, Apply A, class F>
  __device__ __forceinline__ int pass(F rule) {
    // the first position comes from LDS every pass: a value the compiler knows to be loop-invariant has the 3 K addresses of the owned words
    // and their rows above and below kept live across the caller's whole loop, and with the K masks they do not fit 128 VGPRs
    const int mine = flag[2] + tid, last = end - 1;
    u64 m[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int p = mine + k * nt;
      u64 d = 0ull;
      if (p < last) {
        const u64 w = img()[p];
        if (A != Apply::CLEAR || w) d = rule(p, w);
      }
      m[k] = d;
    }
    __syncthreads();                                           // every read of this pass is done
    if (tid == 0) flag[par ^ 1] = 0;
    u64 any = 0ull;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int p = mine + k * nt;
      if (A == Apply::ASSIGN) {
        if (p < last) img()[p] = m[k];
      } else if (m[k]) {                                       // not zero only at a position that was in range
        if (A == Apply::SET) img()[p] |= m[k];
        else img()[p] &= ~m[k];
      }
      any |= m[k];
    }
    if (any) flag[par] = 1;
    __syncthreads();                                           // every write is done
    const int hit = flag[par];
    par ^= 1;
    return hit;
  }
};

// ---- the plane in global memory: a pass reads one image and writes every word of another

struct GlobalPlane {
  int* flag;                                                   // three ints of LDS (FLAGS)
  int words, W64, nt, tid, f;

  __device__ __forceinline__ GlobalPlane(int* flag3, const BitGeo& g)
      : flag(flag3), words(g.H * g.W64), W64(g.W64), nt(blockDim.x), tid(threadIdx.x), f(0) {}

  __device__ __forceinline__ void reset() {
    __syncthreads();
    if (tid == 0) { flag[0] = 0; flag[1] = 0; flag[2] = 0; }
    f = 0;
    __syncthreads();
  }

  // One pass: word(i) writes word i of the new image and returns the bits it changed.  Returns whether any thread changed a bit, the same value
  // in every thread; after it the new image is complete and visible to the workgroup (one workgroup = one CU: its waves share the L1,
  // workgroup-scope ordering suffices)
  template <class F>
  __device__ __forceinline__ int pass(F word) {
    const int fnext = f == 2 ? 0 : f + 1;
    if (tid == 0) flag[fnext] = 0;
    u64 any = 0ull;
    for (int i = tid; i < words; i += nt) any |= word(i);
    if (any) flag[f] = 1;
    __syncthreads();
    const int hit = flag[f];
    f = fnext;
    return hit;
  }
};

// ---- host side

// the threads of a plane's workgroup on the LDS path and, as f's first argument, the smallest K of the ladder with K * threads >= the owned words:
// f(std::integral_constant<int, K>{}, threads)
template <class F>
hipError_t dispatch_k(const BitGeo& g, F f) {
  const int owned = g.H * (g.W64 + 1), nt = std::min(PP_NT, (owned + 63) / 64 * 64), k = (owned + nt - 1) / nt;
  if (k <= 1) return f(std::integral_constant<int, 1>{}, nt);
  if (k <= 2) return f(std::integral_constant<int, 2>{}, nt);
  if (k <= 4) return f(std::integral_constant<int, 4>{}, nt);
  if (k <= 7) return f(std::integral_constant<int, 7>{}, nt);
  if (k <= 10) return f(std::integral_constant<int, 10>{}, nt);
  if (k <= 13) return f(std::integral_constant<int, 13>{}, nt);
  if (k <= 17) return f(std::integral_constant<int, 17>{}, nt);
  return f(std::integral_constant<int, PP_KMAX>{}, nt);
}

// a workgroup per plane (grid-stride over P planes) of `nt` threads over an LDS image of `total` words; the kernel is allowed the whole LDS once
template <auto Kernel, class... Args>
hipError_t launch_lds_planes(size_t P, int nt, int total, hipStream_t st, Args... args) {
  static bool set = false;
  if (!set) {
    hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, PP_LDS_BYTES);
    if (e != hipSuccess) return e;
    set = true;
  }
  hipLaunchKernelGGL(Kernel, dim3((unsigned)std::min<size_t>(P, MAX_GRID)), dim3(nt), (size_t)total * 8 + 16, st, args...);
  return hipSuccess;
}

// NP sets of the bit planes of a stack, carved in order out of a scratch block (null: a size query)
template <int NP>
struct ScratchPlanes {
  u64* p[NP];
  size_t bytes;
};

template <int NP>
ScratchPlanes<NP> carve_planes(void* base, size_t N, int H, int W, int C) {
  ScratchPlanes<NP> s;
  const size_t words = (size_t)H * (((size_t)W + 63) / 64), P = N * C;
  Carver cv(base);
  for (int k = 0; k < NP; ++k) s.p[k] = cv.take<u64>(P * words);
  s.bytes = cv.used;
  return s;
}

}  // namespace

}  // namespace octseg
