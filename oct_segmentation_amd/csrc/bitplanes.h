// bitplanes.h -- the bit-plane and labelling core shared by components.hip (mask clean-up), lesions.hip (lesions in 3-D) and distance.hip (boundary
// distances): the geometry, the word helpers, the label-equivalence union-find, and the launchers of the kernels in bitplanes.hip.
//
// BITS.  A plane is one (slice, channel) pair of the float32 stack [N][H][W][C], any value != 0 set.  It lives as a BIT PLANE: row y is W64 =
// ceil(W / 64) 64-bit words, bit i of word j = pixel 64 j + i, bits past the frame always 0 (1 bit per pixel instead of the stack's 4 bytes; an
// all-zero word is the early exit of every kernel).  The planes are grouped as S independent SETS of D planes each, set after set: the clean-up
// and the distances label or measure every plane on its own (S = N * C, D = 1), the lesions connect a channel's planes across the slices (S = C,
// D = N).  parent and the counters are int32 [S][D * H * W] and hold indices v = n * H * W + y * W + x INSIDE a set.
//
// TERMINATION of every union-find loop: parent[x] <= x always (init writes a run start, atomicMin only lowers a value), a non-root has
// parent[x] < x, so a find walks strictly downwards and ends after at most D * H * W steps; a unite either links a root (done) or continues with a
// strictly smaller pair.  Labels only ever decrease.  Unites across the planes of a set keep all of this because the indices are global to the
// set: plane n - 1's pixels are simply smaller indices of the same array.  A stale read of parent (another CU's L1) yields an older, larger
// ancestor of the same set: the walk still descends, and the atomicMin that links returns the true value, so a lost race is seen and repeated,
// never missed.
#pragma once

#include <algorithm>

#include "common.h"

namespace octseg {

typedef unsigned long long u64;

// HW = H * W, DHW = D * H * W.  The plane comes first: a kernel that works plane by plane reads the leading four fields only
struct BitGeo {
  int H, W, W64, HW, D, DHW;
  __host__ __device__ size_t words() const { return (size_t)D * H * W64; }      // the words of one set
};

// ---- bitplanes.hip.  Every launcher enqueues one kernel of 256-thread workgroups on `st` and nothing else.
// pack / unpack: the plane of (slice n, channel c) is plane n * stride_n + c * stride_c of `bits` ([N][C] planes: (C, 1); [C][N] planes: (1, N));
// float4 accesses when C == 4 and the stack is 16-byte aligned
void launch_bits_pack(const float* stack, int N, const BitGeo& g, int C, int stride_n, int stride_c, u64* bits, hipStream_t st);
void launch_bits_unpack(const u64* bits, int N, const BitGeo& g, int C, int stride_n, int stride_c, float* out, hipStream_t st);
// labelling of the S sets in `bits` (inv: of their complement inside the frame; conn8: 8- instead of 4-connected inside a plane).  init leaves
// count = 0 (and zmax = its own plane; each where the pointer is not null) at every run start; merge unites inside every plane; the caller adds its own
// unites between planes; flatten leaves every pixel two hops from its root, the set's smallest index = its first pixel in raster order
void launch_ccl_init(const u64* bits, int S, const BitGeo& g, int inv, int* parent, int* count, int* zmax, hipStream_t st);
void launch_ccl_merge(const u64* bits, int S, const BitGeo& g, int inv, int conn8, int* parent, hipStream_t st);
void launch_ccl_flatten(const u64* bits, int S, const BitGeo& g, int inv, int* parent, hipStream_t st);
// labels int32 [S][D][H][W] = 1 + root, background 0
void launch_ccl_labels(const u64* bits, int S, const BitGeo& g, const int* parent, int* labels, hipStream_t st);
// kept = the runs whose component has count[root] >= thr[set] and, where zmax is not null, spans zmax[root] - root / HW + 1 >= min_slices planes
void launch_ccl_keep(const u64* bits, int S, const BitGeo& g, const int* parent, const int* count, const int* zmax, const int* thr, int min_slices,
                     u64* kept, hipStream_t st);

namespace {

constexpr int NT = 256, WAVES = NT / 64;
constexpr unsigned MAX_GRID = 1u << 20;

inline BitGeo bit_geo(int D, int H, int W) {
  const int W64 = (W + 63) / 64;
  return BitGeo{H, W, W64, H * W, D, D * H * W};
}
inline unsigned wave_grid(size_t words) { return (unsigned)std::min<size_t>((words + WAVES - 1) / WAVES, MAX_GRID); }   // a wave per word
inline unsigned item_grid(size_t items) { return (unsigned)std::min<size_t>((items + NT - 1) / NT, MAX_GRID); }        // a thread per item

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

// carves 256-byte-aligned arrays out of a scratch block.  Integer arithmetic: a size query carves from a null base and reads `used`
struct Carver {
  uintptr_t base;
  size_t used;
  explicit Carver(void* scratch) : base((uintptr_t)scratch), used(0) {}
  template <typename T> T* take(size_t n) {
    T* r = (T*)(base + used);
    used += al256(n * sizeof(T));
    return r;
  }
};

// word `it` of S sets of D planes -> its set, plane, row and word
struct Place { int s, n, y, j; };
__device__ __forceinline__ Place place(size_t it, const BitGeo& g) {
  Place p;
  p.j = (int)(it % g.W64);
  const size_t row = it / g.W64;
  p.y = (int)(row % g.H);
  const size_t pl = row / g.H;
  p.n = (int)(pl % g.D);
  p.s = (int)(pl / g.D);
  return p;
}

// the bits of word j that lie inside the frame (j < W64, so at least one)
__device__ __forceinline__ u64 inmask(int j, int W) {
  const int n = W - j * 64;
  return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}
// word j of row y of a plane: 0 outside the frame; inv = the complement inside the frame
__device__ __forceinline__ u64 rdw(const u64* __restrict__ plane, int y, int j, const BitGeo& g, int inv = 0) {
  if (y < 0 || y >= g.H || j < 0 || j >= g.W64) return 0ull;
  const u64 w = plane[(size_t)y * g.W64 + j];
  return inv ? ~w & inmask(j, g.W) : w;
}
__device__ __forceinline__ int ctz64(u64 v) { return __ffsll((long long)v) - 1; }            // v != 0
// length of the run of set bits that starts at bit s (bit s is set)
__device__ __forceinline__ int runlen(u64 c, int s) {
  const u64 z = ~(c >> s);                       // s > 0 shifts zeros in at the top, so z != 0 then
  return (s == 0 && z == 0ull) ? 64 : min(ctz64(z), 64 - s);
}
__device__ __forceinline__ u64 runmask(int s, int len) { return (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << s; }

// walks strictly downwards (parent[x] < x for a non-root)
__device__ __forceinline__ int find_root(const int* par, int x) {
  for (;;) {
    const int q = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q == x) return x;
    x = q;
  }
}
// Label-equivalence union.  Every round either links a root (return) or continues with a pair that is strictly smaller in its larger member.
__device__ __forceinline__ void unite(int* par, int a, int b) {
  for (;;) {
    a = find_root(par, a);
    b = find_root(par, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }          // a > b: the larger root goes under the smaller
    const int old = atomicMin(par + a, b);
    if (old == a) return;                                  // a was a root and now points at b
    a = old;                                               // a had been linked meanwhile: its former parent and b must still meet
  }
}

}  // namespace

}  // namespace octseg
