// prune.hip -- pruning of the centreline of every plane of a skeleton stack: side branches of at most `spur` pixels go away, `trim` pixels come off
// every end that is left, a component this would erase is returned whole; and the census of the result: pixels, tips, end, junction and isolated
// points, orthogonal and diagonal links (the length along the centreline), restored pixels.  No reference counterpart (DESIGN.md section 5r states
// the definitions; include/octseg.h repeats them in full).
//
// A plane is one (slice, channel) pair of the float32 stack [N][H][W][C], any value != 0 set, everything outside the frame clear; planes live as
// the bit planes of bitplanes.h (D = 1), pack and unpack are the shared kernels of bitplanes.hip.  P2 .. P9 are the neighbours clockwise from north.
//
//   tip(X)      a set pixel with  P2 & ~(P4|P5|P6|P7|P8)  or  P4 & ~(P6|P7|P8|P9|P2)  or  P6 & ~(P8|P9|P2|P3|P4)  or  P8 & ~(P2|P3|P4|P5|P6)
//               (the neighbour at an orthogonal d is set, the five others than d and d's adjacent diagonals are clear), or with no orthogonal
//               neighbour and exactly one diagonal one: the eight end-point structuring elements of morphological pruning
//   erode(X, n) n passes of X <- X \ tips(X), every tip of a pass decided on X as the pass found it; ends early at the first pass without a tip
//   grow(D,n,A) n passes of D <- D | (dil8(D) & A), dil8 the 3 x 3 dilation
//   result      X = erode(A, spur);  Y = X | grow(tips(X), spur, A) (spur == 0: Y = A);  Z = erode(Y, trim);
//               R = the 8-connected components of A that meet Z = grow(Z, until a pass adds nothing, A);  out = Z | (A & ~R)
//
// Pure boolean, evaluated on the 64 pixels of a word per operation with the shifts of skeleton.hip: E = (w >> 1) | (next << 63), W = (w << 1) |
// (prev >> 63), the diagonals the same shifts of the rows above and below.
//
//   prune (LDS)     prune_lds_kernel<K>: one workgroup per plane, all four phases in ONE launch, over the padded LDS image of skel_thin_lds_kernel:
//                   a row is pitch = W64 + 1 words, the last always zero, a zero row above and below and one leading zero word: word (y, j) at
//                   1 + (y + 1) * pitch + j of (H + 2) * pitch + 1 words.  Thread t owns the positions 1 + pitch + t, + NT, ..., at most K; a pass
//                   computes the mask of each owned word into registers (K statically indexed u64), a barrier ends all reads, the owners apply
//                   their masks, a second barrier ends all writes.  There is ONE image (two of 1024^2 do not fit 160 KiB): `& A` is pointwise, so
//                   a thread re-reads A at its own words from the packed input in global memory, and only where the dilation offers a new bit;
//                   X while D grows, and Z while R grows, are parked per owned word in one more bit plane in scratch, written and read back by
//                   the same thread.  An erosion pass skips zero words; a growth pass whose nine words are all zero offers nothing and touches
//                   neither A nor the image.  "Any bit changed" is one of two LDS flags used in turn, as in the thinning.
//   prune (global)  prune_global_kernel: a plane whose padded image does not fit LDS, or any plane with flag bit 0: the same phases by the same
//                   single workgroup over two images in scratch written in turn, every read bounds-checked.  Bounded and correct, not tuned.
//   census          prune_census_kernel: a wave per 64 words of a plane, a thread per word over the input, the result and the restored bits.
//                   Neighbour counts by the bit-sliced adder of skel_census_kernel, tips by the rule above, links w & E, w & S,
//                   w & SE & ~E & ~S, w & SW & ~W & ~S; sums by shuffles, one integer atomic per wave and column that is not zero.
//
// TERMINATION.  Every erosion loop runs at most spur or trim passes, the first growth loop at most spur passes (0 <= spur, trim <= 8192 at the
// interface).  The restore loop has no count: its plane only ever gains bits and stays inside the finite A, so it gains at most |A| times and the
// loop ends on the first pass that adds nothing.  Every early exit reads a flag that every thread reads after the same barrier, so it is taken by
// all threads or by none.  One plane belongs to one workgroup, so no workgroup waits on another: no spin, no flag between workgroups, no
// cooperative launch, no inline assembly.
//
// BOUNDS.  LDS path: an owned position p lies in [1 + pitch, 1 + (H + 1) * pitch).  An erosion pass reads the neighbours only of a position that
// holds a set bit (a real word, never a pad), a growth pass of every owned position but the last, (H + 1) * pitch, which is a pad: p +- 1,
// p +- pitch, p +- pitch +- 1 then lie in [0, (H + 2) * pitch], the image.  A pad position has no word in the packed planes: it is never parked,
// offered A = 0 and so stays zero.  Global path: every word index is checked against [0, words) before the access, and words left and right of a
// row read as zero.  Bits past the frame are zero in A and every plane here is a subset of A.
#include <algorithm>

#include "bitplanes.h"
#include "kernels.h"

namespace octseg {

namespace {

constexpr int PR_NT = 1024;                                    // the most threads of a pruning workgroup
constexpr int PR_KMAX = 20;                                    // words a thread owns at most on the LDS path
constexpr int PR_LDS_BYTES = 160 * 1024;
constexpr int PR_LDS_WORDS = (PR_LDS_BYTES - 16) / 8;          // the padded image; two flags and the first owned position behind it
static_assert(PR_LDS_WORDS <= PR_KMAX * PR_NT, "a thread owns at most PR_KMAX words");

// the padded LDS image of a plane: its words, or 0 when it does not fit (the thinning's layout and limit)
inline int lds_image_words(int H, int W) {
  const size_t n = ((size_t)H + 2) * (((size_t)W + 63) / 64 + 1) + 1;
  return n <= (size_t)PR_LDS_WORDS ? (int)n : 0;
}

__device__ __forceinline__ u64 ge2(u64 a, u64 b, u64 c, u64 d) { return (a & b) | (c & d) | ((a | b) & (c | d)); }

// the tips of word w.  n, s: the words above and below; p / x suffix: the word before / after in the same row
__device__ __forceinline__ u64 tip_rule(u64 w, u64 wp, u64 wx, u64 n, u64 np, u64 nx, u64 s, u64 sp, u64 sx) {
  const u64 p2 = n, p3 = (n >> 1) | (nx << 63), p4 = (w >> 1) | (wx << 63), p5 = (s >> 1) | (sx << 63);
  const u64 p6 = s, p7 = (s << 1) | (sp >> 63), p8 = (w << 1) | (wp >> 63), p9 = (n << 1) | (np >> 63);
  const u64 north = p2 & ~(p4 | p5 | p6 | p7 | p8), east = p4 & ~(p6 | p7 | p8 | p9 | p2);
  const u64 south = p6 & ~(p8 | p9 | p2 | p3 | p4), west = p8 & ~(p2 | p3 | p4 | p5 | p6);
  const u64 one = (p3 ^ p5 ^ p7 ^ p9) & ~ge2(p3, p5, p7, p9);                           // exactly one diagonal neighbour
  return w & (north | east | south | west | (~(p2 | p4 | p6 | p8) & one));
}

// the 3 x 3 dilation at word w
__device__ __forceinline__ u64 dil_rule(u64 w, u64 wp, u64 wx, u64 n, u64 np, u64 nx, u64 s, u64 sp, u64 sx) {
  const u64 v = n | w | s, vp = np | wp | sp, vx = nx | wx | sx;
  return v | (v >> 1) | (vx << 63) | (v << 1) | (vp >> 63);
}

// word i of an image of `words` words, zero outside it
__device__ __forceinline__ u64 rd(const u64* img, int i, int words) { return (i >= 0 && i < words) ? img[i] : 0ull; }

// the tips (grow == 0) or the dilation (grow == 1) of word i (0 <= i < words) of an image in global memory
__device__ __forceinline__ u64 rule_word(const u64* img, int i, int W64, int words, int grow) {
  const u64 w = img[i];
  if (!w && !grow) return 0ull;
  const int j = i % W64, up = i - W64, dn = i + W64;
  const bool left = j == 0, right = j == W64 - 1;
  const u64 n = rd(img, up, words), s = rd(img, dn, words);
  const u64 wp = left ? 0ull : rd(img, i - 1, words), np = left ? 0ull : rd(img, up - 1, words), sp = left ? 0ull : rd(img, dn - 1, words);
  const u64 wx = right ? 0ull : rd(img, i + 1, words), nx = right ? 0ull : rd(img, up + 1, words), sx = right ? 0ull : rd(img, dn + 1, words);
  return grow ? dil_rule(w, wp, wx, n, np, nx, s, sp, sx) : tip_rule(w, wp, wx, n, np, nx, s, sp, sx);
}

// the index of LDS position p (1 + pitch <= p < 1 + (H + 1) * pitch) in the packed plane, -1 for a pad
__device__ __forceinline__ int packed_index(int p, int pitch) {
  const int r = (p - 1) / pitch - 1, j = (p - 1) % pitch;
  return j < pitch - 1 ? r * (pitch - 1) + j : -1;
}

// the shape of a workgroup's LDS plane; par: which of flag[0] / flag[1] the next pass sets
struct LdsPlane {
  u64* img;
  int* flag;
  int pitch, end, nt, tid, par;
};

// The end of a pass, between its two barriers: thread 0 clears the other flag (last read after the previous pass's second barrier, next set after
// the next pass's first), whoever changed a bit sets this pass's.  Returns whether any thread did: the same value in every thread
__device__ __forceinline__ int pass_hit(LdsPlane& L, u64 any) {
  if (L.tid == 0) L.flag[L.par ^ 1] = 0;
  if (any) L.flag[L.par] = 1;
  __syncthreads();                                             // every write is done
  const int hit = L.flag[L.par];
  L.par ^= 1;
  return hit;
}

// at most n passes of image <- image \ tips(image)
template <int K>
__device__ __forceinline__ void erode_lds(LdsPlane& L, int n) {
  u64* img = L.img;
  const int pitch = L.pitch, end = L.end, nt = L.nt;
  for (int it = 0; it < n; ++it) {
    // the first position comes from LDS every pass, as in skel_thin_lds_kernel: a loop-invariant value has the addresses of the owned words and
    // their rows kept live across the loop, and with the K masks they do not fit 128 VGPRs
    const int mine = L.flag[2] + L.tid;
    u64 del[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int p = mine + k * nt;
      u64 d = 0ull;
      if (p < end) {
        const u64 w = img[p];
        if (w) {                                               // a real word: its eight neighbours lie inside the image
          const u64* up = img + p - pitch;
          const u64* dn = img + p + pitch;
          d = tip_rule(w, img[p - 1], img[p + 1], up[0], up[-1], up[1], dn[0], dn[-1], dn[1]);
        }
      }
      del[k] = d;
    }
    __syncthreads();                                           // every read of this pass is done
    u64 any = 0ull;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (del[k]) img[mine + k * nt] &= ~del[k];               // del[k] != 0 only at a position that was in range
      any |= del[k];
    }
    if (!pass_hit(L, any)) break;                              // uniform
  }
}

// at most n passes (n < 0: until a pass adds nothing) of image <- image | (dil8(image) & A), A = the packed plane `in`
template <int K>
__device__ __forceinline__ void grow_lds(LdsPlane& L, int n, const u64* __restrict__ in) {
  u64* img = L.img;
  const int pitch = L.pitch, last = L.end - 1, nt = L.nt;     // the position end - 1 is the last row's pad: its neighbours end past the image
  for (int it = 0; n < 0 || it < n; ++it) {
    const int mine = L.flag[2] + L.tid;
    u64 add[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int p = mine + k * nt;
      u64 d = 0ull;
      if (p < last) {
        const u64* up = img + p - pitch;
        const u64* dn = img + p + pitch;
        const u64 w = img[p];
        d = dil_rule(w, img[p - 1], img[p + 1], up[0], up[-1], up[1], dn[0], dn[-1], dn[1]) & ~w;
        if (d) {                                               // nine zero words offer nothing; A is read only where there is an offer
          const int i = packed_index(p, pitch);
          d = i >= 0 ? d & in[i] : 0ull;
        }
      }
      add[k] = d;
    }
    __syncthreads();
    u64 any = 0ull;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (add[k]) img[mine + k * nt] |= add[k];
      any |= add[k];
    }
    if (!pass_hit(L, any)) break;
  }
}

}  // namespace

// ---- pruning from LDS: a workgroup per plane (grid-stride over the planes), blockDim.x * K >= H * pitch, the padded image of `total` words fits
// LDS.  src: A, only read; dst: the result; park: X, then Z, at the end the restored bits A & ~R
template <int K>
__global__ __launch_bounds__(PR_NT) void prune_lds_kernel(const u64* __restrict__ src, u64* __restrict__ dst, u64* __restrict__ park, size_t P,
                                                           BitGeo g, int total, int spur, int trim) {
  extern __shared__ u64 pr_img[];
  const int words = g.H * g.W64, W64 = g.W64, pitch = W64 + 1, nt = blockDim.x, tid = threadIdx.x;
  const int first = 1 + pitch, end = 1 + (g.H + 1) * pitch;   // the positions of rows 0 .. H - 1, pad words included
  LdsPlane L{pr_img, (int*)(pr_img + total), pitch, end, nt, tid, 0};
  for (size_t pl = blockIdx.x; pl < P; pl += gridDim.x) {
    const u64* in = src + pl * words;
    u64* pk = park + pl * words;
    for (int p = tid; p < total; p += nt) {
      const int r = (p - 1) / pitch - 1, j = (p - 1) % pitch;  // p = 0: r = -1, a pad
      pr_img[p] = (p >= first && r < g.H && j < W64) ? in[r * W64 + j] : 0ull;
    }
    if (tid == 0) { L.flag[0] = 0; L.flag[1] = 0; L.flag[2] = first; }
    L.par = 0;
    __syncthreads();
    if (spur > 0) {
      erode_lds<K>(L, spur);                                   // the image is X
      {
        const int mine = L.flag[2] + tid;
        u64 t[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const int p = mine + k * nt;
          u64 d = 0ull;
          if (p < end) {
            const u64 w = pr_img[p];
            const int i = packed_index(p, pitch);
            if (i >= 0) pk[i] = w;                             // X is parked while D grows
            if (w) {
              const u64* up = pr_img + p - pitch;
              const u64* dn = pr_img + p + pitch;
              d = tip_rule(w, pr_img[p - 1], pr_img[p + 1], up[0], up[-1], up[1], dn[0], dn[-1], dn[1]);
            }
          }
          t[k] = d;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; ++k)
          if (mine + k * nt < end) pr_img[mine + k * nt] = t[k];
        __syncthreads();                                       // the image is D = tips(X)
      }
      grow_lds<K>(L, spur, in);
      for (int p = first + tid; p < end; p += nt) {            // own words only: no neighbour is read, the loop above ended on a barrier
        const int i = packed_index(p, pitch);
        if (i >= 0) pr_img[p] |= pk[i];
      }
      __syncthreads();                                         // the image is Y
    }
    erode_lds<K>(L, trim);                                     // the image is Z
    for (int p = first + tid; p < end; p += nt) {
      const int i = packed_index(p, pitch);
      if (i >= 0) pk[i] = pr_img[p];                           // Z is parked while R grows
    }
    grow_lds<K>(L, -1, in);                                    // the image is R
    u64* out = dst + pl * words;
    for (int p = first + tid; p < end; p += nt) {
      const int i = packed_index(p, pitch);
      if (i >= 0) {
        const u64 rest = in[i] & ~pr_img[p];
        out[i] = pk[i] | rest;
        pk[i] = rest;
      }
    }
    __syncthreads();                                           // the image and the flags are reused by the next plane
  }
}

// ---- pruning over images in global memory: a workgroup per plane, any size.  src is only read; the result ends in dst, tmp is the other image,
// park as above.  Thread t reads and writes park only at the words t, t + NT, ...
__global__ __launch_bounds__(PR_NT) void prune_global_kernel(const u64* __restrict__ src, u64* dst, u64* tmp, u64* park, size_t P, BitGeo g, int spur,
                                                              int trim) {
  // two flags in turn, two barriers per pass: flag[par] is set between the barriers of a pass and read after the second; thread 0 clears it between
  // the barriers of the next pass, when every thread has read it, and it is next set after the first barrier of the pass after that
  __shared__ int flag[2];
  const int words = g.H * g.W64, W64 = g.W64, nt = blockDim.x, tid = threadIdx.x;
  for (size_t pl = blockIdx.x; pl < P; pl += gridDim.x) {
    const u64* in = src + pl * words;
    u64* a = dst + pl * words;
    u64* b = tmp + pl * words;
    u64* pk = park + pl * words;
    const u64* cur = in;
    if (tid == 0) { flag[0] = 0; flag[1] = 0; }
    __syncthreads();
    int par = 0;
    // at most n passes (n < 0: until idle) of erosion (grow == 0) or growth inside A (grow == 1), each from `cur` into the image that is not `cur`
    auto passes = [&](int n, int grow) {
      for (int it = 0; n < 0 || it < n; ++it) {
        u64* nxt = cur == a ? b : a;
        u64 any = 0ull;
        for (int i = tid; i < words; i += nt) {
          const u64 w = cur[i];
          u64 d = rule_word(cur, i, W64, words, grow);
          if (grow) {
            d &= ~w;
            if (d) d &= in[i];
          }
          nxt[i] = grow ? w | d : w & ~d;
          any |= d;
        }
        __syncthreads();                                       // the new image is complete and visible to the workgroup
        if (tid == 0) flag[par ^ 1] = 0;
        if (any) flag[par] = 1;
        __syncthreads();
        const int hit = flag[par];
        par ^= 1;
        cur = nxt;
        if (!hit) break;                                       // uniform
      }
    };
    if (spur > 0) {
      passes(spur, 0);                                         // cur = X, in a or b: at least one pass ran
      u64* nxt = cur == a ? b : a;
      for (int i = tid; i < words; i += nt) {
        pk[i] = cur[i];
        nxt[i] = rule_word(cur, i, W64, words, 0);
      }
      __syncthreads();
      cur = nxt;                                               // D = tips(X)
      passes(spur, 1);
      u64* y = cur == a ? a : b;
      for (int i = tid; i < words; i += nt) y[i] |= pk[i];     // own words only
      __syncthreads();                                         // cur = Y
    }
    passes(trim, 0);                                           // cur = Z
    for (int i = tid; i < words; i += nt) pk[i] = cur[i];
    passes(-1, 1);                                             // cur = R
    for (int i = tid; i < words; i += nt) {                    // own words only: in place where R lies in dst
      const u64 rest = in[i] & ~cur[i];
      a[i] = pk[i] | rest;
      pk[i] = rest;
    }
    __syncthreads();
  }
}

// ---- census: a wave per 64 words of a plane.  census int32 [P][9], added to (cleared by the caller)
__global__ __launch_bounds__(NT) void prune_census_kernel(const u64* __restrict__ raw, const u64* __restrict__ res, const u64* __restrict__ rest,
                                                           size_t P, BitGeo g, int* __restrict__ census) {
  const int words = g.H * g.W64, chunks = (words + 63) / 64, lane = threadIdx.x & 63;
  const size_t total = P * chunks, nwaves = (size_t)gridDim.x * WAVES;
  for (size_t it = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < total; it += nwaves) {
    const size_t pl = it / chunks;
    const int i = (int)(it % chunks) * 64 + lane;
    int v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (i < words) {
      const u64* sp = res + pl * words;
      const u64 s = sp[i];
      v[0] = __popcll(raw[pl * words + i]);
      v[8] = __popcll(rest[pl * words + i]);
      if (s) {
        const int y = i / g.W64, j = i % g.W64;
        const u64 n = rdw(sp, y - 1, j, g), np = rdw(sp, y - 1, j - 1, g), nx = rdw(sp, y - 1, j + 1, g);
        const u64 d = rdw(sp, y + 1, j, g), dp = rdw(sp, y + 1, j - 1, g), dx = rdw(sp, y + 1, j + 1, g);
        const u64 wp = rdw(sp, y, j - 1, g), wx = rdw(sp, y, j + 1, g);
        // x0 .. x7 = P2 .. P9
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
        v[2] = __popcll(tip_rule(s, wp, wx, n, np, nx, d, dp, dx));
        v[3] = __popcll(s & bit0 & ~twos);                                           // count == 1
        v[4] = __popcll(s & twos & ~two);                                            // count >= 3
        v[5] = __popcll(s & ~bit0 & ~twos);                                          // count == 0
        v[6] = __popcll(s & x2) + __popcll(s & x4);                                  // w & E, w & S
        v[7] = __popcll(s & x3 & ~x2 & ~x4) + __popcll(s & x5 & ~x6 & ~x4);          // w & SE & ~E & ~S, w & SW & ~W & ~S
      }
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      int t = v[c];
      for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
      if (lane == 0 && t) atomicAdd(census + pl * 9 + c, t);
    }
  }
}

namespace {

struct PruneScratch {
  u64 *raw, *res, *park, *tmp;
  size_t bytes;
};

PruneScratch prune_carve(void* base, size_t N, int H, int W, int C) {
  PruneScratch s;
  const size_t words = (size_t)H * (((size_t)W + 63) / 64), P = N * C;
  Carver cv(base);
  s.raw = cv.take<u64>(P * words);
  s.res = cv.take<u64>(P * words);
  s.park = cv.take<u64>(P * words);
  s.tmp = cv.take<u64>(P * words);
  s.bytes = cv.used;
  return s;
}

template <int K>
hipError_t prune_lds(const PruneScratch& s, size_t P, const BitGeo& g, int nt, int total, int spur, int trim, hipStream_t st) {
  static bool set = false;
  if (!set) {
    hipError_t e = hipFuncSetAttribute((const void*)prune_lds_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, PR_LDS_BYTES);
    if (e != hipSuccess) return e;
    set = true;
  }
  hipLaunchKernelGGL(prune_lds_kernel<K>, dim3((unsigned)std::min<size_t>(P, MAX_GRID)), dim3(nt), (size_t)total * 8 + 16, st, s.raw, s.res, s.park, P, g,
                     total, spur, trim);
  return hipSuccess;
}

}  // namespace

size_t prune_scratch_bytes(size_t N, int H, int W, int C) { return prune_carve(nullptr, N, H, W, C).bytes; }

hipError_t launch_stack_prune(const float* skel, int N, int H, int W, int C, int spur, int trim, int force_global, void* scratch, float* out,
                              int* census, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const PruneScratch s = prune_carve(scratch, N, H, W, C);
  const size_t P = (size_t)N * C;
  const int words = g.H * g.W64, total = lds_image_words(H, W);
  hipError_t e = hipSuccess;
  if (census) e = hipMemsetAsync(census, 0, P * 9 * sizeof(int), st);
  if (e != hipSuccess) return e;
  launch_bits_pack(skel, N, g, C, C, 1, s.raw, st);
  if (!force_global && total) {
    const int owned = g.H * (g.W64 + 1), nt = std::min(PR_NT, (owned + 63) / 64 * 64), k = (owned + nt - 1) / nt;
    if (k <= 1) e = prune_lds<1>(s, P, g, nt, total, spur, trim, st);
    else if (k <= 2) e = prune_lds<2>(s, P, g, nt, total, spur, trim, st);
    else if (k <= 4) e = prune_lds<4>(s, P, g, nt, total, spur, trim, st);
    else if (k <= 7) e = prune_lds<7>(s, P, g, nt, total, spur, trim, st);
    else if (k <= 10) e = prune_lds<10>(s, P, g, nt, total, spur, trim, st);
    else if (k <= 13) e = prune_lds<13>(s, P, g, nt, total, spur, trim, st);
    else if (k <= 17) e = prune_lds<17>(s, P, g, nt, total, spur, trim, st);
    else e = prune_lds<PR_KMAX>(s, P, g, nt, total, spur, trim, st);
    if (e != hipSuccess) return e;
  } else {
    hipLaunchKernelGGL(prune_global_kernel, dim3((unsigned)std::min<size_t>(P, MAX_GRID)), dim3(PR_NT), 0, st, s.raw, s.res, s.tmp, s.park, P, g, spur,
                       trim);
  }
  if (census)
    hipLaunchKernelGGL(prune_census_kernel, dim3(wave_grid(P * ((words + 63) / 64))), dim3(NT), 0, st, s.raw, s.res, s.park, P, g, census);
  if (out) launch_bits_unpack(s.res, N, g, C, C, 1, out, st);
  return hipGetLastError();
}

}  // namespace octseg
