// distance.hip -- exact Euclidean distance maps of the mask stacks the pipeline carries, and what is read off them: the boundary of every plane,
// the squared distance of every pixel to the nearest target pixel, the directed boundary-to-boundary distance lists behind the Hausdorff
// family (HD, HD95, ASSD), the smallest distance between two classes with the pixel that attains it, and the overlap counts of the same
// planes.  No reference counterpart: the reference reports overlap scores only (DESIGN.md section 5i states the definitions).  The second half of the
// file does the same over the volume a channel's planes form (section 5p; its own comment below); the last section is the signed map and the
// blend of two of them, shape-based interpolation between slices (section 5s; its own comment below).
//
// A plane is one (slice, channel) pair of the float32 stack [N][H][W][C], any value != 0 set.  Planes live as the bit planes of bitplanes.h, every
// plane on its own (its geometry with D = 1); pack and unpack are the shared kernels of bitplanes.hip.  Everything is integer arithmetic on
// SQUARED distances: d2 = dx^2 + dy^2 < 2^25 for H, W <= 4096, exact in int32; no floating point takes part in any decision.  Every phase that
// needs a grid-wide order is a launch of its own on the caller's stream; no workgroup waits on another, no spin, no cooperative launch.
//
//   part      the plane a call works on, a thread per word: `set` = the plane, `clear` = its complement inside the frame, `boundary` =
//             m & ~erode(m) with the 4-neighbour cross, outside the frame clear (so a set pixel on the frame edge is boundary): the word ANDed with
//             the words above and below and with itself shifted by one bit either way, the neighbours' edge bits shifted in.  A word that is not
//             zero marks its plane as non-empty (every writer stores the same 1).
//   column    g[y][x] = the vertical distance from (y, x) to the nearest target pixel of column x, uint16, 0xFFFF = none in this column: a thread
//             per column, one scan down and one up, lanes on consecutive x.  An empty plane is skipped (its g is never read).
//   row min   d2(y, x) = min over x' of (x - x')^2 + g[y][x']^2, the device function both kernels below share: the row's g staged in LDS (at most
//             8 KiB), a lane per query pixel, best = g[x]^2, then k = 1, 2, ... testing x - k and x + k until k^2 >= best or both have left the
//             row.  The loop is bounded by W and best only falls.  O(W) per pixel when the only target sits in a far corner (measured, section 5i).
//   map       d2 of every pixel of every plane, int32 [N][C][H][W]; DIST_NONE on a plane whose target is empty
//   count     per (slice, pair): query and target pixels, |a & b|, |a|, |b| of the raw planes; a workgroup per (slice, pair), no atomics
//   query     d2 of the target plane at the query pixels of the source plane only.  keys: key = (slice * P + pair) << 32 | d2 stored at
//             offsets[slice * P + pair] + slot, the slot from an integer atomic; a position at or past the capacity is dropped and raises the
//             overflow flag -- never a store past the buffer.  min: a 64-bit atomicMin of d2 << 32 | (y * W + x) per (slice, pair): the smallest
//             squared distance and, among the pixels that attain it, the first in raster order.
//
// Every index is clamped or guarded: channel numbers of the pair list are clamped into their stacks, slots are checked against the capacity,
// neighbours outside the frame read as clear.  A wrong argument gives a wrong number, never a stray access.
#include <algorithm>

#include "bitplanes.h"
#include "kernels.h"

namespace octseg {

namespace {

constexpr int DIST_NONE = 0x7fffffff;
constexpr int G_NONE = 0xFFFF;
constexpr int MAX_W = 4096;
constexpr int COL_ROWS = 8;

typedef unsigned short u16;

// min over x' of (x - x')^2 + row[x']^2 for one query pixel; row: the W values of g in LDS.  k^2 and g^2 are below 2^24: the sum fits int32.
__device__ __forceinline__ int row_min(const u16* row, int W, int x) {
  const int v = row[x];
  int best = v == G_NONE ? DIST_NONE : v * v;
  for (int k = 1; k < W; ++k) {
    const int k2 = k * k;
    if (k2 >= best) break;
    const bool l = x - k >= 0, r = x + k < W;
    if (!l && !r) break;
    if (l) { const int a = row[x - k]; if (a != G_NONE) best = min(best, k2 + a * a); }
    if (r) { const int a = row[x + k]; if (a != G_NONE) best = min(best, k2 + a * a); }
  }
  return best;
}

}  // namespace

// ---- the part of every plane a call works on, a thread per word.  part: 0 set, 1 clear, 2 boundary.  any (may be null): any[plane] = 1 when the
// result holds a pixel; cleared by the caller beforehand
__global__ __launch_bounds__(NT) void dist_part_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int P, BitGeo g, int part, int* __restrict__ any) {
  const size_t total = (size_t)P * g.H * g.W64;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const int j = (int)(it % g.W64), y = (int)((it / g.W64) % g.H);
    const size_t pl = it / ((size_t)g.W64 * g.H);
    const u64* plane = src + pl * g.H * g.W64;
    const u64 w = src[it];
    u64 o;
    if (part == 0) {
      o = w;
    } else if (part == 1) {
      o = ~w & inmask(j, g.W);
    } else {
      o = 0ull;
      if (w) {                                                     // bits past the frame are clear: pixel W - 1 sees a clear right neighbour
        const u64 prev = rdw(plane, y, j - 1, g), next = rdw(plane, y, j + 1, g);
        const u64 ero = w & rdw(plane, y - 1, j, g) & rdw(plane, y + 1, j, g) & ((w << 1) | (prev >> 63)) & ((w >> 1) | (next << 63));
        o = w & ~ero;
      }
    }
    dst[it] = o;
    if (o && any) any[pl] = 1;
  }
}

// ---- column pass, a thread per (plane, column)
__global__ __launch_bounds__(NT) void dist_column_kernel(const u64* __restrict__ bits, int P, BitGeo g, const int* __restrict__ any, u16* __restrict__ gcol) {
  const size_t total = (size_t)P * g.W;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const int x = (int)(it % g.W);
    const size_t pl = it / g.W;
    if (!any[pl]) continue;
    const u64* col = bits + pl * g.H * g.W64 + (x >> 6);
    u16* gc = gcol + pl * g.HW + x;
    const int sh = x & 63;
    // both scans take COL_ROWS rows at a time, the loads of a group issued before its stores: the up scan reads what the down scan stored
    // through the same pointer, and a load per row behind a store per row would leave one load in flight per lane
    int d = G_NONE;
    for (int y0 = 0; y0 < g.H; y0 += COL_ROWS) {                   // d <= H - 1 <= 4095 wherever it counts
      u64 wv[COL_ROWS];
#pragma unroll
      for (int i = 0; i < COL_ROWS; ++i) wv[i] = col[(size_t)min(y0 + i, g.H - 1) * g.W64];
#pragma unroll
      for (int i = 0; i < COL_ROWS; ++i) {
        if (y0 + i >= g.H) break;
        if ((wv[i] >> sh) & 1ull) d = 0; else if (d != G_NONE) ++d;
        gc[(size_t)(y0 + i) * g.W] = (u16)d;
      }
    }
    d = G_NONE;
    for (int y1 = g.H - 1; y1 >= 0; y1 -= COL_ROWS) {
      int dn[COL_ROWS];
#pragma unroll
      for (int i = 0; i < COL_ROWS; ++i) dn[i] = gc[(size_t)max(y1 - i, 0) * g.W];
#pragma unroll
      for (int i = 0; i < COL_ROWS; ++i) {
        if (y1 - i < 0) break;
        if (dn[i] == 0) d = 0; else if (d != G_NONE) ++d;
        if (d < dn[i]) gc[(size_t)(y1 - i) * g.W] = (u16)d;
      }
    }
  }
}

// ---- full map: a workgroup per (plane, row), the row of g in LDS
__global__ __launch_bounds__(NT) void dist_map_kernel(const u16* __restrict__ gcol, const int* __restrict__ any, int P, BitGeo g, int* __restrict__ d2) {
  __shared__ u16 row[MAX_W];
  const size_t total = (size_t)P * g.H;
  for (size_t it = blockIdx.x; it < total; it += gridDim.x) {      // workgroup-uniform
    const size_t pl = it / g.H;
    int* out = d2 + it * g.W;
    if (!any[pl]) {
      for (int x = threadIdx.x; x < g.W; x += NT) out[x] = DIST_NONE;
      continue;
    }
    const u16* src = gcol + it * g.W;
    for (int x = threadIdx.x; x < g.W; x += NT) row[x] = src[x];
    __syncthreads();
    for (int x = threadIdx.x; x < g.W; x += NT) out[x] = row_min(row, g.W, x);
    __syncthreads();                                               // the next row overwrites the stage
  }
}

// ---- counts: a workgroup per (slice, pair).  counts [N][P][2] = query, target pixels; overlap [N][P][3] = |a & b|, |a|, |b| of the raw planes
__global__ __launch_bounds__(NT) void dist_count_kernel(const u64* __restrict__ rawa, const u64* __restrict__ rawb, const u64* __restrict__ qbits,
                                                        const u64* __restrict__ tbits, int N, BitGeo g, int Ca, int Cb, const int* __restrict__ pairs,
                                                        int P, int* __restrict__ counts, int* __restrict__ overlap) {
  __shared__ int red[5][NT];
  const size_t total = (size_t)N * P, words = (size_t)g.H * g.W64;
  for (size_t it = blockIdx.x; it < total; it += gridDim.x) {
    const size_t n = it / P;
    const int p = (int)(it % P);
    const int ca = min(max(pairs[2 * p], 0), Ca - 1), cb = min(max(pairs[2 * p + 1], 0), Cb - 1);
    const size_t oa = (n * Ca + ca) * words, ob = (n * Cb + cb) * words;
    int s[5] = {0, 0, 0, 0, 0};
    for (size_t i = threadIdx.x; i < words; i += NT) {
      const u64 a = rawa[oa + i], b = rawb[ob + i];
      s[0] += __popcll(qbits[oa + i]);
      s[1] += __popcll(tbits[ob + i]);
      s[2] += __popcll(a & b);
      s[3] += __popcll(a);
      s[4] += __popcll(b);
    }
    for (int k = 0; k < 5; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int st = NT >> 1; st > 0; st >>= 1) {
      if ((int)threadIdx.x < st) for (int k = 0; k < 5; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + st];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      counts[it * 2] = red[0][0];
      counts[it * 2 + 1] = red[1][0];
      if (overlap) { overlap[it * 3] = red[2][0]; overlap[it * 3 + 1] = red[3][0]; overlap[it * 3 + 2] = red[4][0]; }
    }
    __syncthreads();
  }
}

// ---- d2 at the query pixels: a workgroup per (slice, pair, row).  keys (with offsets, cursor, capacity, overflow) and / or minout
__global__ __launch_bounds__(NT) void dist_query_kernel(const u64* __restrict__ qbits, const u16* __restrict__ gcol, const int* __restrict__ any, int N,
                                                        BitGeo g, int Ca, int Cb, const int* __restrict__ pairs, int P, long long seg0,
                                                        const long long* __restrict__ offsets, int* __restrict__ cursor, long long* __restrict__ keys,
                                                        long long capacity, int* __restrict__ overflow, u64* __restrict__ minout) {
  __shared__ u16 row[MAX_W];
  __shared__ u64 qrow[MAX_W / 64];
  const size_t total = (size_t)N * P * g.H;
  const int lane = threadIdx.x & 63;
  for (size_t it = blockIdx.x; it < total; it += gridDim.x) {      // workgroup-uniform
    const int y = (int)(it % g.H);
    const size_t seg = it / g.H, n = seg / P;
    const int p = (int)(seg % P);
    const int ca = min(max(pairs[2 * p], 0), Ca - 1), cb = min(max(pairs[2 * p + 1], 0), Cb - 1);
    const size_t pa = n * Ca + ca, pb = n * Cb + cb;
    u64 mine = 0ull;
    if ((int)threadIdx.x < g.W64) mine = qbits[(pa * g.H + y) * g.W64 + threadIdx.x];
    if (!__syncthreads_or(mine != 0ull)) continue;                 // no query pixel in this row
    if ((int)threadIdx.x < g.W64) qrow[threadIdx.x] = mine;
    const int have = any[pb];
    if (have) {
      const u16* src = gcol + (pb * g.H + y) * (size_t)g.W;
      for (int x = threadIdx.x; x < g.W; x += NT) row[x] = src[x];
    }
    __syncthreads();
    u64 best = ~0ull;
    for (int x = threadIdx.x; x < g.W; x += NT) {
      if (!((qrow[x >> 6] >> (x & 63)) & 1ull)) continue;
      const int d = have ? row_min(row, g.W, x) : DIST_NONE;
      if (keys) {
        const int slot = atomicAdd(cursor + seg, 1);
        const long long pos = offsets[seg] + slot;
        if (pos >= 0 && pos < capacity) keys[pos] = (long long)(((u64)(seg0 + (long long)seg) << 32) | (u64)(unsigned)d);
        else *overflow = 1;
      }
      if (minout) {
        const u64 k = ((u64)(unsigned)d << 32) | (u64)(unsigned)(y * g.W + x);
        best = k < best ? k : best;
      }
    }
    if (minout) {                                                   // every lane takes part in the shuffles
      for (int s = 32; s > 0; s >>= 1) {
        const u64 o = __shfl_xor(best, s, 64);
        best = o < best ? o : best;
      }
      if (lane == 0 && best != ~0ull) atomicMin(minout + seg, best);
    }
    __syncthreads();                                               // the next row overwrites the stages
  }
}

namespace {

struct Scratch {
  u64 *rawa, *rawb, *qa, *tb;
  u16* g;
  int *any, *cursor;
  size_t bytes;
};

// one-stack calls: Cb = 0, pairs = 0 (rawa, qa = the part, g, any over N * Ca planes)
Scratch carve(void* base, size_t N, int H, int W, int Ca, int Cb, int pairs) {
  Scratch s;
  const size_t HW = (size_t)H * W, words = (size_t)H * (((size_t)W + 63) / 64);
  const size_t Pa = N * Ca, Pb = N * Cb, Pt = Cb ? Pb : Pa;
  Carver cv(base);
  s.rawa = cv.take<u64>(Pa * words);
  s.qa = cv.take<u64>(Pa * words);
  s.rawb = cv.take<u64>(Pb * words);
  s.tb = cv.take<u64>(Pb * words);
  s.g = cv.take<u16>(Pt * HW);
  s.any = cv.take<int>(Pt);
  s.cursor = cv.take<int>(N * (size_t)pairs);
  s.bytes = cv.used;
  return s;
}

unsigned block_grid(size_t blocks) { return (unsigned)std::min<size_t>(blocks, MAX_GRID); }

// pack both stacks, derive the query planes of src and the target planes of dst (any = which target planes hold a pixel)
hipError_t prepare_pair(const float* src, const float* dst, int N, const BitGeo& g, int Ca, int Cb, int src_part, int dst_part, const Scratch& s,
                        hipStream_t st) {
  const size_t wa = (size_t)N * Ca * g.H * g.W64, wb = (size_t)N * Cb * g.H * g.W64;
  launch_bits_pack(src, N, g, Ca, Ca, 1, s.rawa, st);
  launch_bits_pack(dst, N, g, Cb, Cb, 1, s.rawb, st);
  hipError_t e = hipMemsetAsync(s.any, 0, (size_t)N * Cb * sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dist_part_kernel, dim3(item_grid(wa)), dim3(NT), 0, st, s.rawa, s.qa, N * Ca, g, src_part, (int*)nullptr);
  hipLaunchKernelGGL(dist_part_kernel, dim3(item_grid(wb)), dim3(NT), 0, st, s.rawb, s.tb, N * Cb, g, dst_part, s.any);
  return hipSuccess;
}

}  // namespace

size_t distance_scratch_bytes(size_t N, int H, int W, int Ca, int Cb, int pairs) { return carve(nullptr, N, H, W, Ca, Cb, pairs).bytes; }

hipError_t launch_stack_boundary(const float* stack, int N, int H, int W, int C, void* scratch, float* out, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const Scratch s = carve(scratch, N, H, W, C, 0, 0);
  launch_bits_pack(stack, N, g, C, C, 1, s.rawa, st);
  hipLaunchKernelGGL(dist_part_kernel, dim3(item_grid((size_t)N * C * g.H * g.W64)), dim3(NT), 0, st, s.rawa, s.qa, N * C, g, 2, (int*)nullptr);
  launch_bits_unpack(s.qa, N, g, C, C, 1, out, st);
  return hipGetLastError();
}

hipError_t launch_stack_distance(const float* stack, int N, int H, int W, int C, int to, void* scratch, int* d2, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const int P = N * C;
  const Scratch s = carve(scratch, N, H, W, C, 0, 0);
  launch_bits_pack(stack, N, g, C, C, 1, s.rawa, st);
  hipError_t e = hipMemsetAsync(s.any, 0, (size_t)P * sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dist_part_kernel, dim3(item_grid((size_t)P * g.H * g.W64)), dim3(NT), 0, st, s.rawa, s.qa, P, g, to, s.any);
  hipLaunchKernelGGL(dist_column_kernel, dim3(item_grid((size_t)P * g.W)), dim3(NT), 0, st, s.qa, P, g, s.any, s.g);
  hipLaunchKernelGGL(dist_map_kernel, dim3(block_grid((size_t)P * g.H)), dim3(NT), 0, st, s.g, s.any, P, g, d2);
  return hipGetLastError();
}

hipError_t launch_pair_distance_counts(const float* src, const float* dst, int N, int H, int W, int Ca, int Cb, const int* pairs, int P, int src_part,
                                       int dst_part, void* scratch, int* counts, int* overlap, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const Scratch s = carve(scratch, N, H, W, Ca, Cb, P);
  hipError_t e = prepare_pair(src, dst, N, g, Ca, Cb, src_part, dst_part, s, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dist_count_kernel, dim3(block_grid((size_t)N * P)), dim3(NT), 0, st, s.rawa, s.rawb, s.qa, s.tb, N, g, Ca, Cb, pairs, P, counts,
                     overlap);
  return hipGetLastError();
}

// keys and / or minout (the other null)
hipError_t launch_pair_distance_query(const float* src, const float* dst, int N, int H, int W, int Ca, int Cb, const int* pairs, int P, int src_part,
                                      int dst_part, void* scratch, long long seg0, const long long* offsets, long long* keys, long long capacity,
                                      int* overflow, unsigned long long* minout, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const Scratch s = carve(scratch, N, H, W, Ca, Cb, P);
  hipError_t e = prepare_pair(src, dst, N, g, Ca, Cb, src_part, dst_part, s, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dist_column_kernel, dim3(item_grid((size_t)N * Cb * g.W)), dim3(NT), 0, st, s.tb, N * Cb, g, s.any, s.g);
  if (keys) e = hipMemsetAsync(s.cursor, 0, (size_t)N * P * sizeof(int), st);
  if (e == hipSuccess && minout) e = hipMemsetAsync(minout, 0xFF, (size_t)N * P * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dist_query_kernel, dim3(block_grid((size_t)N * P * g.H)), dim3(NT), 0, st, s.qa, s.g, s.any, N, g, Ca, Cb, pairs, P, seg0, offsets,
                     s.cursor, keys, capacity, overflow, (u64*)minout);
  return hipGetLastError();
}

// ==== the same over the VOLUME a channel's N planes form.  Voxel (z, y, x) of a channel is pixel (y, x) of its plane in slice z;
// neighbouring slices lie s = slice_step pixels apart, an integer, so d2 = (s dz)^2 + dy^2 + dx^2 stays exact in int32: s (N - 1) <= 32767 keeps it
// below 2^30 + 2^25.  The squared distance is separable: d2_3(z, y, x) = min over z' of d2_2(z', y, x) + (s (z - z'))^2, a third pass along the slice
// axis over the per-slice map the column pass and row_min give.  That map is never held whole: the slice-axis pass is independent per (y, x), so a
// BAND of rows y0 .. y0 + rows - 1 of ALL slices is mapped, passed along z and consumed, band after band, each band three launches.
//
//   part      as above, with the boundary's erosion also ANDed with the same word of slices n - 1 and n + 1 (the 6-neighbour cross; slices outside
//             0 .. N - 1 read as zero, so every set voxel of the first and last slice is boundary).  Two flags: any[plane] as above (a slice whose
//             2-D target is empty is skipped by the column pass and mapped to DIST_NONE) and anyvol[channel], the target of a DISTANCE: where it is 0
//             the result is DIST_NONE for the whole volume and the search along z is not run.
//   column    as above, a thread per (plane, column), but only the band's rows of g are stored: the scans still run the whole column, reading bits
//   map       dist_map_kernel over the band's rows: int32 [N * C planes][rows][W]; DIST_NONE on an empty plane
//   slice min a thread per voxel of the band, lanes on consecutive x, so every load along z is coalesced: best = the voxel's own slice, then k = 1,
//             2, ... testing z - k and z + k until (s k)^2 >= best or both have left the volume.  DIST_NONE entries are infinite: never added to.
//             Bounded by N, best only falls.
//   query     the slice minimum at the query voxels of the source part only; a SEGMENT is a pair.  keys: the wave's query lanes take their slots
//             from one 64-bit atomic of the wave's first query lane; min: a 64-bit atomicMin of d2 << 32 | (z H W + y W + x), N H W <= 2^32.
//   count     dist_count_kernel per (slice, pair) into scratch, then a thread per (pair, counter) sums the slices into int64.
namespace {

__device__ __forceinline__ int slice_min(const int* __restrict__ col, size_t stride, int N, int z, int s) {
  int best = col[(size_t)z * stride];
  for (int k = 1; k < N; ++k) {
    const int sk = s * k, k2 = sk * sk;                            // s k <= 32767
    if (k2 >= best) break;
    const bool l = z - k >= 0, r = z + k < N;
    if (!l && !r) break;
    if (l) { const int a = col[(size_t)(z - k) * stride]; if (a != DIST_NONE) best = min(best, k2 + a); }
    if (r) { const int a = col[(size_t)(z + k) * stride]; if (a != DIST_NONE) best = min(best, k2 + a); }
  }
  return best;
}

}  // namespace

// ---- the part of every plane, planes [N][C]; any [N * C] and anyvol [C] (either may be null) cleared by the caller
__global__ __launch_bounds__(NT) void dist_part3_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int N, int C, BitGeo g, int part,
                                                        int* __restrict__ any, int* __restrict__ anyvol) {
  const size_t words = (size_t)g.H * g.W64, total = (size_t)N * C * words;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const int j = (int)(it % g.W64), y = (int)((it / g.W64) % g.H);
    const size_t pl = it / words;
    const int n = (int)(pl / C);
    const u64* plane = src + pl * words;
    const u64 w = src[it];
    u64 o;
    if (part == 0) {
      o = w;
    } else if (part == 1) {
      o = ~w & inmask(j, g.W);
    } else {
      o = 0ull;
      if (w) {
        const u64 prev = rdw(plane, y, j - 1, g), next = rdw(plane, y, j + 1, g);
        const u64 before = n > 0 ? src[it - (size_t)C * words] : 0ull, after = n + 1 < N ? src[it + (size_t)C * words] : 0ull;
        const u64 ero = w & rdw(plane, y - 1, j, g) & rdw(plane, y + 1, j, g) & ((w << 1) | (prev >> 63)) & ((w >> 1) | (next << 63)) & before & after;
        o = w & ~ero;
      }
    }
    dst[it] = o;
    if (o) {
      if (any) any[pl] = 1;
      if (anyvol) anyvol[pl % C] = 1;
    }
  }
}

// ---- column pass of a band: a thread per (plane, column) scans the whole column from the bits and stores rows y0 .. y0 + rb - 1, gband [P][rb][W]
__global__ __launch_bounds__(NT) void dist_column_band_kernel(const u64* __restrict__ bits, int P, BitGeo g, const int* __restrict__ any, int y0, int rb,
                                                              u16* __restrict__ gband) {
  const size_t total = (size_t)P * g.W;
  const int y1 = min(y0 + rb, g.H);
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const int x = (int)(it % g.W);
    const size_t pl = it / g.W;
    if (!any[pl]) continue;
    const u64* col = bits + pl * g.H * g.W64 + (x >> 6);
    u16* gc = gband + pl * rb * g.W + x;
    const int sh = x & 63;
    int d = G_NONE;
#pragma unroll 4
    for (int y = 0; y < y1; ++y) {
      if ((col[(size_t)y * g.W64] >> sh) & 1ull) d = 0; else if (d != G_NONE) ++d;
      if (y >= y0) gc[(size_t)(y - y0) * g.W] = (u16)d;
    }
    d = G_NONE;
#pragma unroll 4
    for (int y = g.H - 1; y >= y0; --y) {
      if ((col[(size_t)y * g.W64] >> sh) & 1ull) d = 0; else if (d != G_NONE) ++d;
      if (y < y1 && d < (int)gc[(size_t)(y - y0) * g.W]) gc[(size_t)(y - y0) * g.W] = (u16)d;
    }
  }
}

// ---- slice-axis pass of a band into the full map: a thread per (slice, channel, band row, x).  d2band [N * C][rb][W], out [N][C][H][W]
__global__ __launch_bounds__(NT) void dist_slice_map_kernel(const int* __restrict__ d2band, const int* __restrict__ anyvol, int N, int C, int H, int W,
                                                            int y0, int rb, int s, int* __restrict__ out) {
  const size_t total = (size_t)N * C * rb * W, stride = (size_t)C * rb * W;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const int x = (int)(it % W), r = (int)((it / W) % rb);
    const size_t pl = it / ((size_t)W * rb);
    const int c = (int)(pl % C), z = (int)(pl / C);
    out[(pl * H + y0 + r) * W + x] = anyvol[c] ? slice_min(d2band + ((size_t)c * rb + r) * W + x, stride, N, z, s) : DIST_NONE;
  }
}

// ---- slice-axis pass of a band at the query voxels: a workgroup per 256 voxels of one pair.  keys (with offsets, cursor, capacity, overflow)
// and / or minout
__global__ __launch_bounds__(NT) void dist_query3_kernel(const u64* __restrict__ qbits, const int* __restrict__ d2band, const int* __restrict__ anyvol,
                                                         int N, BitGeo g, int Ca, int Cb, const int* __restrict__ pairs, int P, int y0, int rb, int s,
                                                         long long seg0, const long long* __restrict__ offsets, u64* __restrict__ cursor,
                                                         long long* __restrict__ keys, long long capacity, int* __restrict__ overflow,
                                                         u64* __restrict__ minout) {
  const size_t per = (size_t)N * rb * g.W, chunks = (per + NT - 1) / NT, total = chunks * P, stride = (size_t)Cb * rb * g.W;
  const int lane = threadIdx.x & 63;
  for (size_t ch = blockIdx.x; ch < total; ch += gridDim.x) {      // workgroup-uniform: every lane takes part in the ballots and shuffles
    const int p = (int)(ch / chunks);
    const size_t i = (ch % chunks) * NT + threadIdx.x;
    const int ca = min(max(pairs[2 * p], 0), Ca - 1), cb = min(max(pairs[2 * p + 1], 0), Cb - 1);
    bool q = false;
    int d = DIST_NONE;
    unsigned voxel = 0u;
    if (i < per) {
      const int x = (int)(i % g.W), r = (int)((i / g.W) % rb), z = (int)(i / ((size_t)g.W * rb)), y = y0 + r;
      q = (qbits[(((size_t)z * Ca + ca) * g.H + y) * g.W64 + (x >> 6)] >> (x & 63)) & 1ull;
      if (q && anyvol[cb]) d = slice_min(d2band + ((size_t)cb * rb + r) * g.W + x, stride, N, z, s);
      voxel = (unsigned)((size_t)z * g.HW + (size_t)y * g.W + x);
    }
    if (keys) {
      const u64 m = __ballot(q);
      if (m) {                                                     // wave-uniform
        const int leader = ctz64(m);
        u64 base = 0ull;
        if (lane == leader) base = atomicAdd(cursor + p, (u64)__popcll(m));
        base = __shfl(base, leader, 64);
        if (q) {
          const long long pos = offsets[p] + (long long)(base + (u64)__popcll(m & ((1ull << lane) - 1ull)));
          if (pos >= 0 && pos < capacity) keys[pos] = (long long)(((u64)(seg0 + p) << 32) | (u64)(unsigned)d);
          else *overflow = 1;
        }
      }
    }
    if (minout) {
      u64 best = q ? (((u64)(unsigned)d << 32) | (u64)voxel) : ~0ull;
      for (int sft = 32; sft > 0; sft >>= 1) {
        const u64 o = __shfl_xor(best, sft, 64);
        best = o < best ? o : best;
      }
      if (lane == 0 && best != ~0ull) atomicMin(minout + p, best);
    }
  }
}

// ---- the per-slice counts of dist_count_kernel summed over the slices: out int64 [P][2], overlap int64 [P][3] (may be null)
__global__ __launch_bounds__(NT) void dist_count_sum_kernel(const int* __restrict__ counts, const int* __restrict__ overlap, int N, int P,
                                                            long long* __restrict__ outc, long long* __restrict__ outo) {
  const size_t total = (size_t)P * 5;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const int p = (int)(it / 5), k = (int)(it % 5);
    long long sum = 0;
    for (int n = 0; n < N; ++n) sum += k < 2 ? counts[((size_t)n * P + p) * 2 + k] : overlap[((size_t)n * P + p) * 3 + k - 2];
    if (k < 2) outc[(size_t)p * 2 + k] = sum;
    else if (outo) outo[(size_t)p * 3 + k - 2] = sum;
  }
}

namespace {

struct Scratch3 {
  u64 *rawa, *rawb, *qa, *tb, *cursor;
  u16* g;
  int *any, *anyvol, *cnt, *d2;
  size_t bytes;
};

// one-stack calls: Cb = 0, pairs = 0 (the target planes are qa); rows = the rows of a band, 0 for the calls that take no distance
Scratch3 carve3(void* base, size_t N, int H, int W, int Ca, int Cb, int pairs, int rows) {
  Scratch3 s;
  const size_t words = (size_t)H * (((size_t)W + 63) / 64), Ct = Cb ? Cb : Ca, band = N * Ct * rows * W;
  Carver cv(base);
  s.rawa = cv.take<u64>(N * Ca * words);
  s.qa = cv.take<u64>(N * Ca * words);
  s.rawb = cv.take<u64>(N * Cb * words);
  s.tb = cv.take<u64>(N * Cb * words);
  s.any = cv.take<int>(N * Ct);
  s.anyvol = cv.take<int>(Ct);
  s.cursor = cv.take<u64>((size_t)pairs);
  s.cnt = cv.take<int>(N * (size_t)pairs * 5);
  s.g = cv.take<u16>(band);
  s.d2 = cv.take<int>(band);
  s.bytes = cv.used;
  return s;
}

hipError_t prepare_volume(const float* src, const float* dst, int N, const BitGeo& g, int Ca, int Cb, int src_part, int dst_part, const Scratch3& s,
                          hipStream_t st) {
  const size_t wa = (size_t)N * Ca * g.H * g.W64, wb = (size_t)N * Cb * g.H * g.W64;
  launch_bits_pack(src, N, g, Ca, Ca, 1, s.rawa, st);
  launch_bits_pack(dst, N, g, Cb, Cb, 1, s.rawb, st);
  hipError_t e = hipMemsetAsync(s.any, 0, (size_t)N * Cb * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(s.anyvol, 0, (size_t)Cb * sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dist_part3_kernel, dim3(item_grid(wa)), dim3(NT), 0, st, s.rawa, s.qa, N, Ca, g, src_part, (int*)nullptr, (int*)nullptr);
  hipLaunchKernelGGL(dist_part3_kernel, dim3(item_grid(wb)), dim3(NT), 0, st, s.rawb, s.tb, N, Cb, g, dst_part, s.any, s.anyvol);
  return hipSuccess;
}

// the per-slice map of band y0 .. y0 + rb - 1 of the target planes into s.d2
void launch_band(const u64* target, int P, const BitGeo& g, const Scratch3& s, int y0, int rb, hipStream_t st) {
  BitGeo gb = g;
  gb.H = rb;
  gb.HW = rb * g.W;
  hipLaunchKernelGGL(dist_column_band_kernel, dim3(item_grid((size_t)P * g.W)), dim3(NT), 0, st, target, P, g, s.any, y0, rb, s.g);
  hipLaunchKernelGGL(dist_map_kernel, dim3(block_grid((size_t)P * rb)), dim3(NT), 0, st, s.g, s.any, P, gb, s.d2);
}

}  // namespace

size_t volume_distance_scratch_bytes(size_t N, int H, int W, int Ca, int Cb, int pairs, int rows) {
  return carve3(nullptr, N, H, W, Ca, Cb, pairs, rows).bytes;
}

// the most rows of a band (1 .. H) whose scratch fits `bytes`; 0 when a band of one row does not.  The need grows with the rows.
int volume_distance_rows(size_t bytes, size_t N, int H, int W, int Ca, int Cb, int pairs) {
  if (volume_distance_scratch_bytes(N, H, W, Ca, Cb, pairs, 1) > bytes) return 0;
  int lo = 1, hi = H;
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (volume_distance_scratch_bytes(N, H, W, Ca, Cb, pairs, mid) <= bytes) lo = mid; else hi = mid - 1;
  }
  return lo;
}

hipError_t launch_volume_boundary(const float* stack, int N, int H, int W, int C, void* scratch, float* out, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const Scratch3 s = carve3(scratch, N, H, W, C, 0, 0, 0);
  launch_bits_pack(stack, N, g, C, C, 1, s.rawa, st);
  hipLaunchKernelGGL(dist_part3_kernel, dim3(item_grid((size_t)N * C * g.H * g.W64)), dim3(NT), 0, st, s.rawa, s.qa, N, C, g, 2, (int*)nullptr,
                     (int*)nullptr);
  launch_bits_unpack(s.qa, N, g, C, C, 1, out, st);
  return hipGetLastError();
}

hipError_t launch_volume_distance(const float* stack, int N, int H, int W, int C, int to, int slice_step, int rows, void* scratch, int* d2,
                                  hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const int P = N * C;
  const Scratch3 s = carve3(scratch, N, H, W, C, 0, 0, rows);
  launch_bits_pack(stack, N, g, C, C, 1, s.rawa, st);
  hipError_t e = hipMemsetAsync(s.any, 0, (size_t)P * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(s.anyvol, 0, (size_t)C * sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dist_part3_kernel, dim3(item_grid((size_t)P * g.H * g.W64)), dim3(NT), 0, st, s.rawa, s.qa, N, C, g, to, s.any, s.anyvol);
  for (int y0 = 0; y0 < H; y0 += rows) {
    const int rb = std::min(rows, H - y0);
    launch_band(s.qa, P, g, s, y0, rb, st);
    hipLaunchKernelGGL(dist_slice_map_kernel, dim3(item_grid((size_t)P * rb * W)), dim3(NT), 0, st, s.d2, s.anyvol, N, C, H, W, y0, rb, slice_step, d2);
  }
  return hipGetLastError();
}

hipError_t launch_volume_pair_counts(const float* src, const float* dst, int N, int H, int W, int Ca, int Cb, const int* pairs, int P, int src_part,
                                     int dst_part, void* scratch, long long* counts, long long* overlap, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const Scratch3 s = carve3(scratch, N, H, W, Ca, Cb, P, 0);
  hipError_t e = prepare_volume(src, dst, N, g, Ca, Cb, src_part, dst_part, s, st);
  if (e != hipSuccess) return e;
  int* over = s.cnt + (size_t)N * P * 2;
  hipLaunchKernelGGL(dist_count_kernel, dim3(block_grid((size_t)N * P)), dim3(NT), 0, st, s.rawa, s.rawb, s.qa, s.tb, N, g, Ca, Cb, pairs, P, s.cnt, over);
  hipLaunchKernelGGL(dist_count_sum_kernel, dim3(item_grid((size_t)P * 5)), dim3(NT), 0, st, s.cnt, over, N, P, counts, overlap);
  return hipGetLastError();
}

// keys and / or minout (the other null)
hipError_t launch_volume_pair_query(const float* src, const float* dst, int N, int H, int W, int Ca, int Cb, const int* pairs, int P, int src_part,
                                    int dst_part, int slice_step, int rows, void* scratch, long long seg0, const long long* offsets, long long* keys,
                                    long long capacity, int* overflow, unsigned long long* minout, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const Scratch3 s = carve3(scratch, N, H, W, Ca, Cb, P, rows);
  hipError_t e = prepare_volume(src, dst, N, g, Ca, Cb, src_part, dst_part, s, st);
  if (e == hipSuccess && keys) e = hipMemsetAsync(s.cursor, 0, (size_t)P * sizeof(u64), st);
  if (e == hipSuccess && minout) e = hipMemsetAsync(minout, 0xFF, (size_t)P * sizeof(unsigned long long), st);
  if (e != hipSuccess) return e;
  for (int y0 = 0; y0 < H; y0 += rows) {
    const int rb = std::min(rows, H - y0);
    launch_band(s.tb, N * Cb, g, s, y0, rb, st);
    const size_t chunks = ((size_t)N * rb * W + NT - 1) / NT * P;
    hipLaunchKernelGGL(dist_query3_kernel, dim3(block_grid(chunks)), dim3(NT), 0, st, s.qa, s.d2, s.anyvol, N, g, Ca, Cb, pairs, P, y0, rb, slice_step,
                       seg0, offsets, s.cursor, keys, capacity, overflow, (u64*)minout);
  }
  return hipGetLastError();
}

// ==== SIGNED squared distance maps and their blend: shape-based interpolation between slices.  sd2 int32 [N][C][H][W]:
// +d2 to the nearest clear pixel at a set pixel, -d2 to the nearest set pixel at a clear one, -/+ DIST_NONE on an empty / a full plane, never 0.
//
//   signed map  pack, then dist_part_kernel and dist_column_kernel as they are, once for part `set` and once for part `clear`, the second part
//               written over the first (its columns are taken by then: launches of one stream): two sets of bits, two uint16 column maps, two
//               sets of flags.  A workgroup per (plane, row) stages BOTH rows of g in LDS (2 x 8 KiB at most); a lane per pixel is set iff
//               g_set[x] == 0 and runs ONE row_min, over the other part's row.  A plane either flag shows as empty is filled without a search;
//               its g (which the column pass skipped) is never read.
//   blend       a lane per pixel of every plan row (channel, out_slice, lo, hi, w_lo, w_hi): two int32 loads, the integer rule below, one
//               float store of 0.0 / 1.0 into out [N_out][H][W][C].  Every workgroup lies inside one row, so a wave's set pixels are one
//               popcount of a ballot and one atomic into made[row].  The row's six numbers are clamped: a wrong plan gives a wrong plane.
//
// TERMINATION: the only loop whose trip count depends on data is row_min's, bounded by W (k < W) whatever the row holds, and best only falls; the
// grid-stride loops are bounded by their totals.  No workgroup waits on another: no spin, no flag, no cooperative launch; the only atomics are
// integer adds into made, whose result nobody reads inside the launch.
namespace {

constexpr int MAX_WEIGHT = 32767;

// wa * s_a + wb * s_b > 0 with s = sign(sd2) * sqrt(|sd2|), DIST_NONE infinite, decided in integers: a zero weight removes its side; equal signs
// decide; of opposite signs the larger of w^2 * |sd2| (int64, below 2^30 * 2^25) decides, an infinite side beats a finite one, two infinite ones go
// by the weights; a tie is clear
__device__ __forceinline__ bool blend_set(int a, int b, int wa, int wb) {
  if (wa == 0) return wb != 0 && b > 0;
  if (wb == 0) return a > 0;
  const bool pa = a > 0, pb = b > 0;
  if (pa == pb) return pa;
  const int p = pa ? a : b, q = pa ? b : a, wp = pa ? wa : wb, wq = pa ? wb : wa;   // p > 0 > q
  const bool pinf = p == DIST_NONE, qinf = q == -DIST_NONE;
  if (pinf || qinf) return pinf && (!qinf || wp > wq);
  return (long long)wp * wp * p > (long long)wq * wq * -(long long)q;
}

struct ScratchS {
  u64 *raw, *part;
  u16 *gset, *gclear;
  int* any;                                                          // [2][P]: set, clear; one memset
  size_t bytes;
};

ScratchS carve_signed(void* base, size_t N, int H, int W, int C) {
  ScratchS s;
  const size_t P = N * C, HW = (size_t)H * W, words = (size_t)H * (((size_t)W + 63) / 64);
  Carver cv(base);
  s.raw = cv.take<u64>(P * words);
  s.part = cv.take<u64>(P * words);
  s.gset = cv.take<u16>(P * HW);
  s.gclear = cv.take<u16>(P * HW);
  s.any = cv.take<int>(2 * P);
  s.bytes = cv.used;
  return s;
}

}  // namespace

// ---- signed map: a workgroup per (plane, row), both rows of g in LDS
__global__ __launch_bounds__(NT) void dist_signed_map_kernel(const u16* __restrict__ gset, const u16* __restrict__ gclear, const int* __restrict__ anyset,
                                                             const int* __restrict__ anyclear, int P, BitGeo g, int* __restrict__ sd2) {
  __shared__ u16 rows[2][MAX_W];
  const size_t total = (size_t)P * g.H;
  for (size_t it = blockIdx.x; it < total; it += gridDim.x) {      // workgroup-uniform
    const size_t pl = it / g.H;
    int* out = sd2 + it * g.W;
    const int hs = anyset[pl], hc = anyclear[pl];
    if (!hs || !hc) {                                                // empty: every pixel clear and no set pixel to measure to; full: the reverse
      const int v = hs ? DIST_NONE : -DIST_NONE;
      for (int x = threadIdx.x; x < g.W; x += NT) out[x] = v;
      continue;
    }
    const u16 *ss = gset + it * g.W, *sc = gclear + it * g.W;
    for (int x = threadIdx.x; x < g.W; x += NT) { rows[0][x] = ss[x]; rows[1][x] = sc[x]; }
    __syncthreads();
    for (int x = threadIdx.x; x < g.W; x += NT) {
      const bool set = rows[0][x] == 0;                              // the pixel's own bit: distance 0 to its own column's nearest set pixel
      const int d = row_min(rows[set ? 1 : 0], g.W, x);              // both parts hold a pixel: finite and >= 1
      out[x] = set ? d : -d;
    }
    __syncthreads();                                                 // the next row overwrites the stages
  }
}

// ---- blend: workgroups [M][chunks of NT pixels]; plan int32 [M][6]; made (may be null) int32 [M], cleared by the caller
__global__ __launch_bounds__(NT) void dist_blend_kernel(const int* __restrict__ sd2, int K, int HW, int C, const int* __restrict__ plan, int M,
                                                        float* __restrict__ out, int Nout, int* __restrict__ made) {
  const size_t chunks = ((size_t)HW + NT - 1) / NT, total = chunks * M;
  const int lane = threadIdx.x & 63;
  for (size_t it = blockIdx.x; it < total; it += gridDim.x) {      // workgroup-uniform: every lane takes part in the ballot
    const size_t r = it / chunks;
    const int* row = plan + r * 6;
    const int c = min(max(row[0], 0), C - 1), os = min(max(row[1], 0), Nout - 1);
    const int lo = min(max(row[2], 0), K - 1), hi = min(max(row[3], 0), K - 1);
    const int wa = min(max(row[4], 0), MAX_WEIGHT), wb = min(max(row[5], 0), MAX_WEIGHT);
    const size_t pix = (it % chunks) * NT + threadIdx.x;
    bool set = false;
    if (pix < (size_t)HW) {
      set = blend_set(sd2[((size_t)lo * C + c) * HW + pix], sd2[((size_t)hi * C + c) * HW + pix], wa, wb);
      out[((size_t)os * HW + pix) * C + c] = set ? 1.0f : 0.0f;
    }
    if (made) {
      const u64 m = __ballot(set);
      if (lane == 0 && m) atomicAdd(made + r, __popcll(m));
    }
  }
}

size_t signed_distance_scratch_bytes(size_t N, int H, int W, int C) { return carve_signed(nullptr, N, H, W, C).bytes; }

hipError_t launch_stack_signed_distance(const float* stack, int N, int H, int W, int C, void* scratch, int* sd2, hipStream_t st) {
  const BitGeo g = bit_geo(1, H, W);
  const int P = N * C;
  const ScratchS s = carve_signed(scratch, N, H, W, C);
  const size_t words = (size_t)P * g.H * g.W64;
  launch_bits_pack(stack, N, g, C, C, 1, s.raw, st);
  hipError_t e = hipMemsetAsync(s.any, 0, (size_t)2 * P * sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(dist_part_kernel, dim3(item_grid(words)), dim3(NT), 0, st, s.raw, s.part, P, g, 0, s.any);
  hipLaunchKernelGGL(dist_column_kernel, dim3(item_grid((size_t)P * g.W)), dim3(NT), 0, st, s.part, P, g, s.any, s.gset);
  hipLaunchKernelGGL(dist_part_kernel, dim3(item_grid(words)), dim3(NT), 0, st, s.raw, s.part, P, g, 1, s.any + P);
  hipLaunchKernelGGL(dist_column_kernel, dim3(item_grid((size_t)P * g.W)), dim3(NT), 0, st, s.part, P, g, s.any + P, s.gclear);
  hipLaunchKernelGGL(dist_signed_map_kernel, dim3(block_grid((size_t)P * g.H)), dim3(NT), 0, st, s.gset, s.gclear, s.any, s.any + P, P, g, sd2);
  return hipGetLastError();
}

hipError_t launch_signed_blend(const int* sd2, int K, int H, int W, int C, const int* plan, int M, float* out, int Nout, int* made, hipStream_t st) {
  if (made) {
    const hipError_t e = hipMemsetAsync(made, 0, (size_t)M * sizeof(int), st);
    if (e != hipSuccess) return e;
  }
  const size_t chunks = ((size_t)H * W + NT - 1) / NT;
  hipLaunchKernelGGL(dist_blend_kernel, dim3(block_grid(chunks * M)), dim3(NT), 0, st, sd2, K, H * W, C, plan, M, out, Nout, made);
  return hipGetLastError();
}

}  // namespace octseg
