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
// Pure boolean, so it is evaluated on the 64 pixels of a word per operation (planepass.h, WORDS); sums of four booleans are compared through
// ge2(a, b, c, d) = "two or more" and the all-four AND.  An all-zero word has nothing to delete and is skipped.  The plane in LDS, the pass, its
// flags and its bounds are planepass.h's.
//
//   thin (LDS)     skel_thin_lds_kernel<K>: one workgroup per plane, all passes in one launch over planepass.h's padded LDS image: a sub-iteration
//                  is one CLEAR pass.
//   thin (global)  skel_thin_global_kernel: a plane whose padded image is above 20478 words (up to 4096 x 4096), or any plane with flag bit 0: the same loop by the same
//                  single workgroup, every sub-iteration reading one image and writing all words of the other (input -> skel -> tmp -> skel ...).
//                  Bounded and correct, not tuned.
//   census         skel_census_kernel: a wave per 64 words of a plane, a thread per word over the input bits and the skeleton bits.  The number of
//                  skeleton neighbours of all 64 pixels comes from planepass.h's bit-sliced counter; popcounts are summed over the wave by
//                  shuffles, then one integer atomic per wave and column that is not zero.
//
// TERMINATION.  A productive pass clears at least one bit of a finite plane and no bit is ever set, so there are at most H * W productive passes; the
// pass loop ends on the first idle pass (both sub-iterations report no deletion to every thread: the exit is uniform).
#include "kernels.h"
#include "planepass.h"

namespace octseg {

namespace {

// the pixels of word w that sub-iteration `sub` deletes
__device__ __forceinline__ u64 thin_rule(u64 w, const Ring& r, int sub) {
  const u64 a1 = r.p9 | r.p2, a2 = r.p3 | r.p4, a3 = r.p5 | r.p6, a4 = r.p7 | r.p8;
  const u64 b1 = r.p2 | r.p3, b2 = r.p4 | r.p5, b3 = r.p6 | r.p7, b4 = r.p8 | r.p9;
  const u64 c1 = ~r.p2 & a2, c2 = ~r.p4 & a3, c3 = ~r.p6 & a4, c4 = ~r.p8 & a1;
  const u64 one = (c1 ^ c2 ^ c3 ^ c4) & ~ge2(c1, c2, c3, c4);
  const u64 range = ge2(a1, a2, a3, a4) & ge2(b1, b2, b3, b4) & (~(a1 & a2 & a3 & a4) | ~(b1 & b2 & b3 & b4));
  const u64 m = sub ? ((r.p2 | r.p3 | ~r.p5) & r.p4) : ((r.p6 | r.p7 | ~r.p9) & r.p8);
  return w & one & range & ~m;
}

}  // namespace

// ---- thinning from LDS: a workgroup per plane (grid-stride over the planes), blockDim.x * K >= H * pitch, the padded image of `total` words
// fits LDS.  passes (may be null): passes[plane * pstride] = the productive passes
template <int K>
__global__ __launch_bounds__(PP_NT) void skel_thin_lds_kernel(const u64* __restrict__ src, u64* __restrict__ dst, size_t P, BitGeo g, int total,
                                                               int* __restrict__ passes, int pstride) {
  LdsPlane L(g, total);
  const int words = g.H * g.W64;
  for (size_t pl = blockIdx.x; pl < P; pl += gridDim.x) {
    L.load(src + pl * words);
    int npass = 0;
    for (;;) {
      int hit = L.pass<K, Apply::CLEAR>([&](int p, u64 w) { return thin_rule(w, ring(L.nine(p, w)), 0); });
      hit |= L.pass<K, Apply::CLEAR>([&](int p, u64 w) { return thin_rule(w, ring(L.nine(p, w)), 1); });
      if (!hit) break;
      ++npass;
    }
    L.store(dst + pl * words);
    if (L.tid == 0 && passes) passes[pl * pstride] = npass;
  }
}

// ---- thinning over images in global memory: a workgroup per plane, any size.  src is only read; the result ends in dst, tmp is the other image
__global__ __launch_bounds__(PP_NT) void skel_thin_global_kernel(const u64* __restrict__ src, u64* dst, u64* tmp, size_t P, BitGeo g,
                                                                  int* __restrict__ passes, int pstride) {
  __shared__ int flag[3];
  GlobalPlane G(flag, g);
  for (size_t pl = blockIdx.x; pl < P; pl += gridDim.x) {
    const u64* cur = src + pl * G.words;
    u64* a = dst + pl * G.words;
    u64* b = tmp + pl * G.words;
    G.reset();
    int npass = 0;
    for (;;) {
      int hit = 0;
      for (int sub = 0; sub < 2; ++sub) {
        hit |= G.pass([&](int i) {
          const u64 w = cur[i];
          const u64 del = w ? thin_rule(w, ring(nine_global(cur, i, G.W64, G.words, w)), sub) : 0ull;
          a[i] = w & ~del;
          return del;
        });
        cur = a;
        u64* t = a; a = b; b = t;
      }
      if (!hit) break;
      ++npass;
    }
    // an even number of sub-iterations ran: input -> dst -> tmp -> dst -> ... leaves the result in tmp
    u64* out = dst + pl * G.words;
    for (int i = G.tid; i < G.words; i += G.nt) out[i] = cur[i];
    if (G.tid == 0 && passes) passes[pl * pstride] = npass;
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
        const Counted c = count_neighbours(s, ring(nine_global(sp, i, g.W64, words, s)));
        v[1] = __popcll(s);
        v[2] = __popcll(c.one);
        v[3] = __popcll(c.many);
        v[4] = __popcll(c.none);
      }
    }
    wave_add_columns(v, census + pl * 6);
  }
}

size_t skeleton_scratch_bytes(size_t N, int H, int W, int C) { return carve_planes<3>(nullptr, N, H, W, C).bytes; }

bool skeleton_fits_lds(int H, int W) { return lds_image_words(H, W) != 0; }

hipError_t launch_stack_skeleton(const float* stack, int N, int H, int W, int C, int force_global, void* scratch, float* out, int* census,
                                 hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const auto s = carve_planes<3>(scratch, N, H, W, C);
  u64 *raw = s.p[0], *skel = s.p[1], *tmp = s.p[2];
  const size_t P = (size_t)N * C;
  const int words = g.H * g.W64, total = lds_image_words(H, W);
  hipError_t e = hipSuccess;
  if (census) e = hipMemsetAsync(census, 0, P * 6 * sizeof(int), st);
  if (e != hipSuccess) return e;
  launch_bits_pack(stack, N, g, C, C, 1, raw, st);
  int* passes = census ? census + 5 : nullptr;
  if (!force_global && total) {
    e = dispatch_k(g, [&](auto k, int nt) {
      return launch_lds_planes<&skel_thin_lds_kernel<decltype(k)::value>>(P, nt, total, st, (const u64*)raw, skel, P, g, total, passes, 6);
    });
    if (e != hipSuccess) return e;
  } else {
    hipLaunchKernelGGL(skel_thin_global_kernel, dim3((unsigned)std::min<size_t>(P, MAX_GRID)), dim3(PP_NT), 0, st, raw, skel, tmp, P, g, passes, 6);
  }
  if (census)
    hipLaunchKernelGGL(skel_census_kernel, dim3(wave_grid(P * ((words + 63) / 64))), dim3(NT), 0, st, raw, skel, P, g, census);
  if (out) launch_bits_unpack(skel, N, g, C, C, 1, out, st);
  return hipGetLastError();
}

}  // namespace octseg
