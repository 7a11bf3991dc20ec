// bitplanes.hip -- the kernels every consumer of bit planes shares (bitplanes.h states the layout, the S x D geometry and the termination argument of
// the union-find loops): stack <-> bits, and connected-component labelling by label-equivalence union-find.  A phase that needs a grid-wide order is
// a launch of its own; no workgroup ever waits on another, there is no flag, no spin and no cooperative launch.
//
//   pack        stack -> bits: a wave takes 64 pixels of a row, `v != 0` per channel is a ballot = one word (the interleaved stack is read once)
//   unpack      bits -> float32 0.0 / 1.0 in the stack's layout
//   init        parent[v] = first pixel of v's horizontal run inside its word: runs need no atomics
//   merge       inside every plane: a set pixel unites with its left neighbour across a word border and with the row above; run structure makes
//               most pixels skip (only the first pixel of an overlap unites).  8-connected adds the two upper diagonals.  A plane's first row
//               has no row above: planes of a set meet only through the unites their owner adds (lesions.hip's across)
//   flatten     parent[run start] = root(run start); the other pixels of a run keep pointing at their run start, so every pixel is two hops
//               from its root and only one pixel per run walks a chain.  The root is the component's smallest index
//   labels      parent -> int32 [S][D][H][W], 1 + root, background 0
//   keep        kept bits = runs whose component passes the count threshold of its set (and the plane-span rule)
#include "bitplanes.h"

namespace octseg {

namespace {

// word `it` as the labelling sees it (inv = the complement inside the frame)
__device__ __forceinline__ u64 own_word(const u64* __restrict__ bits, size_t it, const BitGeo& g, int inv) {
  const u64 w = bits[it];
  return inv ? ~w & inmask((int)(it % g.W64), g.W) : w;
}

}  // namespace

// ---- stack <-> bit planes, a lane per pixel (a wave per word of a row; wave-uniform loops)
__global__ __launch_bounds__(NT) void bits_pack_kernel(const float* __restrict__ stack, int N, BitGeo g, int C, int sn, int sc, u64* __restrict__ bits,
                                                       int vec) {
  const int lane = threadIdx.x & 63;
  const size_t nw = (size_t)gridDim.x * WAVES, pw = (size_t)g.H * g.W64, total = N * pw;     // pw: the words of a plane
  for (size_t it = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < total; it += nw) {
    const size_t row = it / g.W64, n = it / pw;                // row = n * H + y of the stack; `it` is this word's place in plane n of N
    const int x = (int)(it - row * g.W64) * 64 + lane;
    const bool ok = x < g.W;
    const float* px = stack + (row * g.W + (ok ? x : g.W - 1)) * C;
    u64* dst = bits + it + n * (sn - 1) * pw;                  // channel 0's word: plane n * sn instead of plane n
    if (vec) {
      const float4 v = *(const float4*)px;
      const u64 w0 = __ballot(ok && v.x != 0.f), w1 = __ballot(ok && v.y != 0.f), w2 = __ballot(ok && v.z != 0.f), w3 = __ballot(ok && v.w != 0.f);
      if (lane < 4) dst[(size_t)lane * sc * pw] = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? w2 : w3;
    } else {
      for (int c = 0; c < C; ++c) {
        const u64 w = __ballot(ok && px[c] != 0.f);
        if (lane == 0) dst[(size_t)c * sc * pw] = w;
      }
    }
  }
}

__global__ __launch_bounds__(NT) void bits_unpack_kernel(const u64* __restrict__ bits, int N, BitGeo g, int C, int sn, int sc, float* __restrict__ out,
                                                         int vec) {
  const int lane = threadIdx.x & 63;
  const size_t nw = (size_t)gridDim.x * WAVES, pw = (size_t)g.H * g.W64, total = N * pw;
  for (size_t it = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < total; it += nw) {
    const size_t row = it / g.W64, n = it / pw;
    const int x = (int)(it - row * g.W64) * 64 + lane;
    if (x >= g.W) continue;
    float* px = out + (row * g.W + x) * C;
    const u64* src = bits + it + n * (sn - 1) * pw;            // channel 0's word
    const size_t step = (size_t)sc * pw;                       // from a channel's plane to the next one's
    if (vec) {
      float4 v;
      v.x = (float)((src[0] >> lane) & 1ull);
      v.y = (float)((src[step] >> lane) & 1ull);
      v.z = (float)((src[2 * step] >> lane) & 1ull);
      v.w = (float)((src[3 * step] >> lane) & 1ull);
      *(float4*)px = v;
    } else {
      for (int c = 0; c < C; ++c) px[c] = (float)((src[c * step] >> lane) & 1ull);
    }
  }
}

// ---- labelling, a lane per pixel (a wave per word)
// count (and zmax) are set at RUN STARTS only: they are only ever read or added to at a root, a root is its component's smallest index, so the
// pixel before it is clear and the root starts a run.  What the scratch held at any other pixel is never looked at.
__global__ __launch_bounds__(NT) void ccl_init_kernel(const u64* __restrict__ bits, int S, BitGeo g, int inv, int* __restrict__ parent,
                                                      int* __restrict__ count, int* __restrict__ zmax) {
  const int lane = threadIdx.x & 63;
  const size_t nw = (size_t)gridDim.x * WAVES, total = (size_t)S * g.words();
  for (size_t it = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < total; it += nw) {
    const u64 c = own_word(bits, it, g, inv);
    if (!c || !((c >> lane) & 1ull)) continue;                // bits past the frame are clear: x < W below
    const Place p = place(it, g);
    const u64 below = ~c & ((1ull << lane) - 1ull);           // clear bits under this lane
    const int start = below ? 64 - __clzll((long long)below) : 0;
    const int v0 = p.n * g.HW + p.y * g.W + p.j * 64;
    const size_t o = (size_t)p.s * g.DHW + (size_t)(v0 + lane);
    parent[o] = v0 + start;
    if (lane == start) {
      if (count) count[o] = 0;                                // (the contour tracer wants the labels only)
      if (zmax) zmax[o] = p.n;                                // the span of a component starts as its root's plane
    }
  }
}

__global__ __launch_bounds__(NT) void ccl_merge_kernel(const u64* __restrict__ bits, int S, BitGeo g, int inv, int conn8, int* __restrict__ parent) {
  const int lane = threadIdx.x & 63;
  const size_t nw = (size_t)gridDim.x * WAVES, total = (size_t)S * g.words();
  for (size_t it = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < total; it += nw) {
    const u64 c = own_word(bits, it, g, inv);
    if (!c || !((c >> lane) & 1ull)) continue;
    const Place p = place(it, g);
    const int y = p.y, j = p.j;
    const u64* plane = bits + (it - ((size_t)y * g.W64 + j));
    const u64 cl = rdw(plane, y, j - 1, g, inv), cr = rdw(plane, y, j + 1, g, inv);
    const u64 u = rdw(plane, y - 1, j, g, inv), ul = rdw(plane, y - 1, j - 1, g, inv), ur = rdw(plane, y - 1, j + 1, g, inv);
    const bool w = lane ? (c >> (lane - 1)) & 1ull : cl >> 63, e = lane < 63 ? (c >> (lane + 1)) & 1ull : cr & 1ull;
    const bool n = (u >> lane) & 1ull, nwb = lane ? (u >> (lane - 1)) & 1ull : ul >> 63, neb = lane < 63 ? (u >> (lane + 1)) & 1ull : ur & 1ull;
    int* par = parent + (size_t)p.s * g.DHW;
    const int v = p.n * g.HW + y * g.W + j * 64 + lane;
    if (lane == 0 && w) unite(par, v, v - 1);                           // runs were joined inside a word only
    if (n && !(w && nwb)) unite(par, v, v - g.W);                       // with w and nw set the left neighbour unites with the row above
    if (conn8 && !n) {
      if (nwb && !w) unite(par, v, v - g.W - 1);                        // with w set, nw is w's upper neighbour
      if (neb && !e) unite(par, v, v - g.W + 1);                        // with e set, ne is e's upper neighbour
    }
  }
}

__global__ __launch_bounds__(NT) void ccl_flatten_kernel(const u64* __restrict__ bits, int S, BitGeo g, int inv, int* __restrict__ parent) {
  const int lane = threadIdx.x & 63;
  const size_t nw = (size_t)gridDim.x * WAVES, total = (size_t)S * g.words();
  for (size_t it = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < total; it += nw) {
    const u64 c = own_word(bits, it, g, inv);
    if (!c || !((c >> lane) & 1ull)) continue;
    if (lane && ((c >> (lane - 1)) & 1ull)) continue;           // not a run start: its parent is the run start since init, one hop from the root
    const Place p = place(it, g);
    int* par = parent + (size_t)p.s * g.DHW;
    const int v = p.n * g.HW + p.y * g.W + p.j * 64 + lane;
    // the forest is final (the merges have completed): every value a concurrent flatten writes is the root, a valid ancestor
    const int r = find_root(par, v);
    if (r != v) par[v] = r;
  }
}

__global__ __launch_bounds__(NT) void ccl_labels_kernel(const u64* __restrict__ bits, int S, BitGeo g, const int* __restrict__ parent,
                                                        int* __restrict__ labels) {
  const int lane = threadIdx.x & 63;
  const size_t nw = (size_t)gridDim.x * WAVES, total = (size_t)S * g.words();
  for (size_t it = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < total; it += nw) {
    const Place p = place(it, g);
    const int x = p.j * 64 + lane;
    if (x >= g.W) continue;
    const u64 c = bits[it];
    const size_t base = (size_t)p.s * g.DHW, o = base + (size_t)(p.n * g.HW + p.y * g.W + x);
    labels[o] = ((c >> lane) & 1ull) ? parent[base + parent[o]] + 1 : 0;      // pixel -> run start -> root (a root points at itself)
  }
}

// ---- a thread per word
__global__ __launch_bounds__(NT) void ccl_keep_kernel(const u64* __restrict__ bits, int S, BitGeo g, const int* __restrict__ parent,
                                                      const int* __restrict__ count, const int* __restrict__ zmax, const int* __restrict__ thr,
                                                      int min_slices, u64* __restrict__ kept) {
  const size_t total = (size_t)S * g.words();
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    u64 c = bits[it], o = 0ull;
    if (c) {
      const Place p = place(it, g);
      const size_t base = (size_t)p.s * g.DHW;
      const int v0 = p.n * g.HW + p.y * g.W + p.j * 64, th = thr[p.s];
      while (c) {                                                         // every round clears the run it handled
        const int s = ctz64(c), len = runlen(c, s);
        const u64 m = runmask(s, len);
        const int r = parent[base + v0 + s];                              // a run start points at its root
        if (count[base + r] >= th && (!zmax || zmax[base + r] - r / g.HW + 1 >= min_slices)) o |= m;
        c &= ~m;
      }
    }
    kept[it] = o;
  }
}

// ---- launchers
void launch_bits_pack(const float* stack, int N, const BitGeo& g, int C, int stride_n, int stride_c, u64* bits, hipStream_t st) {
  const int vec = (C == 4 && ((uintptr_t)stack & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(bits_pack_kernel, dim3(wave_grid((size_t)N * g.H * g.W64)), dim3(NT), 0, st, stack, N, g, C, stride_n, stride_c, bits, vec);
}

void launch_bits_unpack(const u64* bits, int N, const BitGeo& g, int C, int stride_n, int stride_c, float* out, hipStream_t st) {
  const int vec = (C == 4 && ((uintptr_t)out & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(bits_unpack_kernel, dim3(wave_grid((size_t)N * g.H * g.W64)), dim3(NT), 0, st, bits, N, g, C, stride_n, stride_c, out, vec);
}

void launch_ccl_init(const u64* bits, int S, const BitGeo& g, int inv, int* parent, int* count, int* zmax, hipStream_t st) {
  hipLaunchKernelGGL(ccl_init_kernel, dim3(wave_grid((size_t)S * g.words())), dim3(NT), 0, st, bits, S, g, inv, parent, count, zmax);
}

void launch_ccl_merge(const u64* bits, int S, const BitGeo& g, int inv, int conn8, int* parent, hipStream_t st) {
  hipLaunchKernelGGL(ccl_merge_kernel, dim3(wave_grid((size_t)S * g.words())), dim3(NT), 0, st, bits, S, g, inv, conn8, parent);
}

void launch_ccl_flatten(const u64* bits, int S, const BitGeo& g, int inv, int* parent, hipStream_t st) {
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3(wave_grid((size_t)S * g.words())), dim3(NT), 0, st, bits, S, g, inv, parent);
}

void launch_ccl_labels(const u64* bits, int S, const BitGeo& g, const int* parent, int* labels, hipStream_t st) {
  hipLaunchKernelGGL(ccl_labels_kernel, dim3(wave_grid((size_t)S * g.words())), dim3(NT), 0, st, bits, S, g, parent, labels);
}

void launch_ccl_keep(const u64* bits, int S, const BitGeo& g, const int* parent, const int* count, const int* zmax, const int* thr, int min_slices,
                     u64* kept, hipStream_t st) {
  hipLaunchKernelGGL(ccl_keep_kernel, dim3(item_grid((size_t)S * g.words())), dim3(NT), 0, st, bits, S, g, parent, count, zmax, thr, min_slices, kept);
}

}  // namespace octseg
