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
// Pure boolean, evaluated on the 64 pixels of a word per operation (planepass.h, WORDS).  The plane in LDS, both kinds of pass, their flags and
// their bounds are planepass.h's.
//
//   prune (LDS)     prune_lds_kernel<K>: one workgroup per plane, all four phases in ONE launch, over planepass.h's padded LDS image: an erosion
//                   pass is CLEAR, a growth pass SET, D = tips(X) ASSIGN.  There is ONE image (two of 1024^2 do not fit 160 KiB): `& A` is
//                   pointwise, so a thread re-reads A at its own words from the packed input in global memory, and only where the dilation offers
//                   a new bit; X while D grows, and Z while R grows, are parked per owned word in one more bit plane in scratch, written and read
//                   back by the same thread.  An erosion pass skips zero words; a growth pass whose nine words are all zero offers nothing and
//                   touches neither A nor the image.
//   prune (global)  prune_global_kernel: a plane whose padded image does not fit LDS, or any plane with flag bit 0: the same phases by the same
//                   single workgroup over two images in scratch written in turn, every read bounds-checked.  Bounded and correct, not tuned.
//   census          prune_census_kernel: a wave per 64 words of a plane, a thread per word over the input, the result and the restored bits.
//                   Neighbour counts by planepass.h's bit-sliced counter, tips by the rule above, links w & E, w & S, w & SE & ~E & ~S,
//                   w & SW & ~W & ~S; sums by shuffles, one integer atomic per wave and column that is not zero.
//
// TERMINATION.  Every erosion loop runs at most spur or trim passes, the first growth loop at most spur passes (0 <= spur, trim <= 8192 at the
// interface).  The restore loop has no count: its plane only ever gains bits and stays inside the finite A, so it gains at most |A| times and the
// loop ends on the first pass that adds nothing.  Every early exit takes a pass's result, the same in every thread.
//
// BOUNDS.  A growth pass reads the nine words of every position a pass visits, pads included: planepass.h's BOUNDS hold them inside the image.  A
// pad position has no word in the packed planes: it is never parked, offered A = 0 and so stays zero.  Bits past the frame are zero in A and every
// plane here is a subset of A.
#include "kernels.h"
#include "planepass.h"

namespace octseg {

namespace {

// the tips of word w
__device__ __forceinline__ u64 tip_rule(u64 w, const Ring& r) {
  const u64 north = r.p2 & ~(r.p4 | r.p5 | r.p6 | r.p7 | r.p8), east = r.p4 & ~(r.p6 | r.p7 | r.p8 | r.p9 | r.p2);
  const u64 south = r.p6 & ~(r.p8 | r.p9 | r.p2 | r.p3 | r.p4), west = r.p8 & ~(r.p2 | r.p3 | r.p4 | r.p5 | r.p6);
  const u64 one = (r.p3 ^ r.p5 ^ r.p7 ^ r.p9) & ~ge2(r.p3, r.p5, r.p7, r.p9);             // exactly one diagonal neighbour
  return w & (north | east | south | west | (~(r.p2 | r.p4 | r.p6 | r.p8) & one));
}

// the 3 x 3 dilation at a word: the three rows are ORed before they are shifted
__device__ __forceinline__ u64 dil_rule(const Nine& q) {
  const u64 v = q.n | q.w | q.s, vp = q.np | q.wp | q.sp, vx = q.nx | q.wx | q.sx;
  return v | (v >> 1) | (vx << 63) | (v << 1) | (vp >> 63);
}

// at most n passes of image <- image \ tips(image)
template <int K>
__device__ __forceinline__ void erode_lds(LdsPlane& L, int n) {
  for (int it = 0; it < n; ++it)
    if (!L.pass<K, Apply::CLEAR>([&](int p, u64 w) { return tip_rule(w, ring(L.nine(p, w))); })) break;
}

// at most n passes (n < 0: until a pass adds nothing) of image <- image | (dil8(image) & A), A = the packed plane `in`
template <int K>
__device__ __forceinline__ void grow_lds(LdsPlane& L, int n, const u64* __restrict__ in) {
  for (int it = 0; n < 0 || it < n; ++it) {
    const int hit = L.pass<K, Apply::SET>([&](int p, u64 w) {
      u64 d = dil_rule(L.nine(p, w)) & ~w;
      if (d) {                                                 // nine zero words offer nothing; A is read only where there is an offer
        const int i = L.packed_index(p);
        d = i >= 0 ? d & in[i] : 0ull;
      }
      return d;
    });
    if (!hit) break;
  }
}

}  // namespace

// ---- pruning from LDS: a workgroup per plane (grid-stride over the planes), blockDim.x * K >= H * pitch, the padded image of `total` words fits
// LDS.  src: A, only read; dst: the result; park: X, then Z, at the end the restored bits A & ~R
template <int K>
__global__ __launch_bounds__(PP_NT) void prune_lds_kernel(const u64* __restrict__ src, u64* __restrict__ dst, u64* __restrict__ park, size_t P,
                                                           BitGeo g, int total, int spur, int trim) {
  LdsPlane L(g, total);
  const int words = g.H * g.W64;
  for (size_t pl = blockIdx.x; pl < P; pl += gridDim.x) {
    const u64* in = src + pl * words;
    u64* pk = park + pl * words;
    u64* out = dst + pl * words;
    L.load(in);
    if (spur > 0) {
      erode_lds<K>(L, spur);                                   // the image is X
      L.pass<K, Apply::ASSIGN>([&](int p, u64 w) {             // the image is D = tips(X)
        const int i = L.packed_index(p);
        if (i >= 0) pk[i] = w;                                 // X is parked while D grows
        return w ? tip_rule(w, ring(L.nine(p, w))) : 0ull;
      });
      grow_lds<K>(L, spur, in);
      L.each_word([&](int p, int i) { L.img()[p] |= pk[i]; });
      __syncthreads();                                         // the image is Y
    }
    erode_lds<K>(L, trim);                                     // the image is Z
    L.each_word([&](int p, int i) { pk[i] = L.img()[p]; });      // Z is parked while R grows
    grow_lds<K>(L, -1, in);                                    // the image is R
    L.each_word([&](int p, int i) {
      const u64 rest = in[i] & ~L.img()[p];
      out[i] = pk[i] | rest;
      pk[i] = rest;
    });
  }
}

// ---- pruning over images in global memory: a workgroup per plane, any size.  src is only read; the result ends in dst, tmp is the other image,
// park as above.  Thread t reads and writes park only at the words t, t + NT, ...
__global__ __launch_bounds__(PP_NT) void prune_global_kernel(const u64* __restrict__ src, u64* dst, u64* tmp, u64* park, size_t P, BitGeo g, int spur,
                                                              int trim) {
  __shared__ int flag[3];
  GlobalPlane G(flag, g);
  const int words = G.words, nt = G.nt, tid = G.tid;
  for (size_t pl = blockIdx.x; pl < P; pl += gridDim.x) {
    const u64* in = src + pl * words;
    u64* a = dst + pl * words;
    u64* b = tmp + pl * words;
    u64* pk = park + pl * words;
    const u64* cur = in;
    G.reset();
    auto tips = [&](int i, u64 w) { return w ? tip_rule(w, ring(nine_global(cur, i, G.W64, words, w))) : 0ull; };
    // at most n passes (n < 0: until idle) of erosion or of growth inside A, each from `cur` into the image that is not `cur`
    auto passes = [&](int n, bool grow) {
      for (int it = 0; n < 0 || it < n; ++it) {
        u64* nxt = cur == a ? b : a;
        const int hit = G.pass([&](int i) {
          const u64 w = cur[i];
          u64 d;
          if (grow) {
            d = dil_rule(nine_global(cur, i, G.W64, words, w)) & ~w;
            if (d) d &= in[i];
            nxt[i] = w | d;
          } else {
            d = tips(i, w);
            nxt[i] = w & ~d;
          }
          return d;
        });
        cur = nxt;
        if (!hit) break;                                       // uniform
      }
    };
    if (spur > 0) {
      passes(spur, false);                                     // cur = X, in a or b: at least one pass ran
      u64* nxt = cur == a ? b : a;
      for (int i = tid; i < words; i += nt) {
        pk[i] = cur[i];
        nxt[i] = tips(i, cur[i]);
      }
      __syncthreads();
      cur = nxt;                                               // D = tips(X)
      passes(spur, true);
      u64* y = cur == a ? a : b;
      for (int i = tid; i < words; i += nt) y[i] |= pk[i];     // own words only
      __syncthreads();                                         // cur = Y
    }
    passes(trim, false);                                       // cur = Z
    for (int i = tid; i < words; i += nt) pk[i] = cur[i];
    passes(-1, true);                                          // cur = R
    for (int i = tid; i < words; i += nt) {                    // own words only: in place where R lies in dst
      const u64 rest = in[i] & ~cur[i];
      a[i] = pk[i] | rest;
      pk[i] = rest;
    }
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
        const Ring r = ring(nine_global(sp, i, g.W64, words, s));
        const Counted c = count_neighbours(s, r);
        v[1] = __popcll(s);
        v[2] = __popcll(tip_rule(s, r));
        v[3] = __popcll(c.one);
        v[4] = __popcll(c.many);
        v[5] = __popcll(c.none);
        v[6] = __popcll(s & r.p4) + __popcll(s & r.p6);                                          // w & E, w & S
        v[7] = __popcll(s & r.p5 & ~r.p4 & ~r.p6) + __popcll(s & r.p7 & ~r.p8 & ~r.p6);          // w & SE & ~E & ~S, w & SW & ~W & ~S
      }
    }
    wave_add_columns(v, census + pl * 9);
  }
}

size_t prune_scratch_bytes(size_t N, int H, int W, int C) { return carve_planes<4>(nullptr, N, H, W, C).bytes; }

hipError_t launch_stack_prune(const float* skel, int N, int H, int W, int C, int spur, int trim, int force_global, void* scratch, float* out,
                              int* census, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const auto s = carve_planes<4>(scratch, N, H, W, C);
  u64 *raw = s.p[0], *res = s.p[1], *park = s.p[2], *tmp = s.p[3];
  const size_t P = (size_t)N * C;
  const int words = g.H * g.W64, total = lds_image_words(H, W);
  hipError_t e = hipSuccess;
  if (census) e = hipMemsetAsync(census, 0, P * 9 * sizeof(int), st);
  if (e != hipSuccess) return e;
  launch_bits_pack(skel, N, g, C, C, 1, raw, st);
  if (!force_global && total) {
    e = dispatch_k(g, [&](auto k, int nt) {
      return launch_lds_planes<&prune_lds_kernel<decltype(k)::value>>(P, nt, total, st, (const u64*)raw, res, park, P, g, total, spur, trim);
    });
    if (e != hipSuccess) return e;
  } else {
    hipLaunchKernelGGL(prune_global_kernel, dim3((unsigned)std::min<size_t>(P, MAX_GRID)), dim3(PP_NT), 0, st, raw, res, tmp, park, P, g, spur, trim);
  }
  if (census)
    hipLaunchKernelGGL(prune_census_kernel, dim3(wave_grid(P * ((words + 63) / 64))), dim3(NT), 0, st, raw, res, park, P, g, census);
  if (out) launch_bits_unpack(res, N, g, C, C, 1, out, st);
  return hipGetLastError();
}

}  // namespace octseg
