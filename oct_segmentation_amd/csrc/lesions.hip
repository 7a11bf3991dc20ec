// lesions.hip -- lesions in 3-D (no reference counterpart): the connected components of a mask stack ACROSS its slices, the
// per-lesion table and area profile, and the flicker filter.  A VOLUME is one channel of the float32 stack [N][H][W][C], any value != 0 set, slices
// along N in the order given; channels are independent.  Inside a slice voxels are 8-connected; between adjacent slices either only the same pixel
// connects (`overlap`: the frame pitch of a pullback is an order of magnitude above the pixel pitch) or the whole 3 x 3 above / below (`full`,
// 26-connected).  The label of a lesion is 1 + n * H * W + y * W + x of its first voxel in raster order.
//
// The bits are the bit planes of bitplanes.h, one volume after the other: its geometry "S sets of D planes" with S = C, D = N, so word j of row y of
// slice n of channel c stands at ((c * N + n) * H + y) * W64 + j, and parent / vox / zmax are int32 [C][N * H * W] and hold VOLUME indices
// v = n * H * W + y * W + x.  Every phase that needs a grid-wide order is a launch of its own on the caller's stream; no workgroup ever waits on
// another, there is no flag, no spin, no cooperative launch and no inline assembly; nothing is allocated.
//
// pack / unpack, init (of a run start, vox = 0 and zmax = its own slice), the 8-connected merge inside every slice, flatten, labels and keep (voxels
// >= threshold and z1 - z0 + 1 >= min_slices) are the shared kernels of bitplanes.hip, where the termination argument of the union-find loops
// stands; the unites of `across` fall under it because slice n - 1's voxels are smaller indices of the same array.  Here:
//
//   across      between init / merge and flatten: a thread per word of slice n >= 1.  overlap: m = c & (the same word of slice n - 1), one unite per
//               maximal run of m with the voxel straight above: both sides of a run are horizontal runs, connected inside their slices already.
//               full: the same for each of the nine words (rows y - 1 .. y + 1 of slice n - 1, each as it is and shifted by +-1 with the neighbour
//               words' bits shifted in), the partner of a run's first bit being that one source voxel.  (One unite per run of the OR of the nine
//               would NOT do: two adjacent bits may see different source voxels, (y - 1, x - 1) and (y + 1, x + 2), that nothing connects in
//               slice n - 1.)
//   count       a thread per word: vox[root] += run length, zmax[root] = max(slice), summed per root inside the wave before one lane's atomic; a
//               run that starts at its root appends the root to the channel's lesion list (capacity N * ceil(H / 2) * ceil(W / 2), the most
//               components a volume holds under either rule)
//   select      ONE workgroup per channel: the threshold t (the keep-th largest voxel count, by bisection on the value), nles, the 32 largest kept
//               lesions by (voxels descending, first voxel ascending) with z0 = first voxel / (H * W) and z1 = zmax
//   extents     runs of ranked lesions reduce the bounding box (atomicMin / atomicMax) and add to profile[rank][slice]
//
// The other loops: run loops clear at least one set bit of a 64-bit word per round; grid-stride loops advance by the grid; the bisection of select
// halves hi - lo every round (at most 31 rounds); the ranking runs 32 rounds; the in-wave reduction of count and extents handles one destination
// per round and clears at least its leader's bit of a 64-bit ballot.
#include <algorithm>

#include "bitplanes.h"
#include "kernels.h"
#include "lesions_internal.h"

namespace octseg {

namespace {

constexpr int SEL_NT = 256;               // workgroup of vol_select_kernel (a power of two)

// one unite per maximal run of m: voxel a0 + s with voxel a0 + s + off, s the run's first bit
__device__ __forceinline__ void unite_runs(int* par, u64 m, int a0, int off) {
  while (m) {                                                  // every round clears the run it handled
    const int s = ctz64(m), len = runlen(m, s);
    unite(par, a0 + s, a0 + s + off);
    m &= ~runmask(s, len);
  }
}

}  // namespace

// a thread per word of the slices n >= 1
__global__ __launch_bounds__(NT) void vol_across_kernel(const u64* __restrict__ bits, int C, BitGeo g, int full, int* __restrict__ parent) {
  const size_t total = (size_t)C * g.words();
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const u64 c = bits[it];
    if (!c) continue;
    const Place p = place(it, g);
    if (p.n == 0) continue;
    const u64* up = bits + ((size_t)p.s * g.D + p.n - 1) * g.H * g.W64;
    int* par = parent + (size_t)p.s * g.DHW;
    const int a0 = p.n * g.HW + p.y * g.W + p.j * 64;
    if (!full) {
      unite_runs(par, c & rdw(up, p.y, p.j, g), a0, -g.HW);
      continue;
    }
    for (int dy = -1; dy <= 1; ++dy) {
      const u64 w = rdw(up, p.y + dy, p.j, g), wl = rdw(up, p.y + dy, p.j - 1, g), wr = rdw(up, p.y + dy, p.j + 1, g);
      const int off = -g.HW + dy * g.W;
      unite_runs(par, c & w, a0, off);
      // a bit whose own source column is set was united above, and that source is its row neighbours' neighbour: the shifted words skip it
      unite_runs(par, c & ((w >> 1) | (wr << 63)) & ~w, a0, off + 1);   // source column x + 1
      unite_runs(par, c & ((w << 1) | (wl >> 63)) & ~w, a0, off - 1);   // source column x - 1
    }
  }
}

// ---- per-run kernels, a thread per word.  Runs that share a destination are summed inside the wave first (a big lesion's runs all add to one
// root: one atomic per run serialises on that address), then ONE lane issues the atomics.  All 64 lanes of a wave take every step below together:
// the grid-stride loop runs on the block's base index, and the run loop goes on while any lane still has a run.
// (wave_sum / wave_min / wave_max: lesions_internal.h)

__global__ __launch_bounds__(NT) void vol_count_kernel(const u64* __restrict__ bits, int C, BitGeo g, const int* __restrict__ parent, int* __restrict__ vox,
                                                       int* __restrict__ zmax, int* __restrict__ list, int* __restrict__ nroots, int cap) {
  const int lane = threadIdx.x & 63;
  const size_t total = (size_t)C * g.words();
  for (size_t first = (size_t)blockIdx.x * NT; first < total; first += (size_t)gridDim.x * NT) {      // block-uniform
    const size_t it = first + threadIdx.x;
    u64 c = it < total ? bits[it] : 0ull;
    const Place p = place(it < total ? it : 0, g);
    const size_t base = (size_t)p.s * g.DHW;
    const int a0 = p.n * g.HW + p.y * g.W + p.j * 64;
    while (__any(c != 0ull)) {                                          // every round clears one run in every lane that has one
      const bool has = c != 0ull;
      long long key = -1;                                               // the root's place in vox / zmax
      int len = 0;
      if (has) {
        const int s = ctz64(c);
        len = runlen(c, s);
        const int r = parent[base + a0 + s];
        key = (long long)(base + r);
        if (r == a0 + s) {
          const int slot = atomicAdd(nroots + p.s, 1);
          if (slot < cap) list[(size_t)p.s * cap + slot] = r;
        }
        c &= ~runmask(s, len);
      }
      u64 pending = __ballot(has);
      while (pending) {                                                 // every round clears at least the leader's bit
        const int leader = ctz64(pending);
        const long long k = __shfl(key, leader);
        const bool mine = has && key == k;
        const int sum = wave_sum(mine ? len : 0), zhi = wave_max(mine ? p.n : 0);
        if (lane == leader) {
          atomicAdd(vox + k, sum);
          if (zhi > (int)((k % g.DHW) / g.HW)) atomicMax(zmax + k, zhi);      // zmax[root] starts at the root's slice z0: that slice needs no atomic
        }
        pending &= ~__ballot(mine);
      }
    }
  }
}

// One workgroup per channel.  t = the keep-th largest voxel count (0 with fewer lesions or keep = 0): the largest v with count(vox >= v) >= keep,
// by bisection between 1 and the largest count.  thr = max(t, min_voxels).  A lesion is KEPT iff vox >= thr and zmax - z0 + 1 >= min_slices; nles
// and the ranking cover the kept lesions.  key = vox << 32 | (2^31 - 1 - first voxel): the largest key is the largest lesion, ties to the earliest
// first voxel; keys are distinct and non-zero.  Round i takes the largest key below round i - 1's.  rank: the 32 ranked roots, -1 = none.
__global__ __launch_bounds__(SEL_NT) void vol_select_kernel(const int* __restrict__ vox, const int* __restrict__ zmax, const int* __restrict__ list,
                                                            const int* __restrict__ nroots, BitGeo g, int cap, int keep, int min_voxels, int min_slices,
                                                            int* __restrict__ thr_out, int* __restrict__ rank, int* __restrict__ nles,
                                                            int* __restrict__ top) {
  __shared__ u64 red[SEL_NT];
  __shared__ u64 keys[TOPL];
  const int tid = threadIdx.x, bd = blockDim.x;
  const size_t ch = blockIdx.x;
  const int n = min(max(nroots[ch], 0), cap);
  const int* vx = vox + ch * g.DHW;
  const int* zm = zmax + ch * g.DHW;
  const int* ls = list + ch * (size_t)cap;
  // workgroup-uniform reductions over red
  auto reduce_sum = [&](int mine) -> int {
    red[tid] = (u64)mine;
    __syncthreads();
    for (int s = bd >> 1; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    const int r = (int)red[0];
    __syncthreads();
    return r;
  };
  auto reduce_max = [&](u64 mine) -> u64 {
    red[tid] = mine;
    __syncthreads();
    for (int s = bd >> 1; s > 0; s >>= 1) {
      if (tid < s && red[tid + s] > red[tid]) red[tid] = red[tid + s];
      __syncthreads();
    }
    const u64 r = red[0];
    __syncthreads();
    return r;
  };
  int t = 0;
  if (keep > 0 && n >= keep) {               // count(vox >= lo) >= keep holds throughout: every lesion has at least one voxel
    u64 mx = 0ull;
    for (int e = tid; e < n; e += bd) mx = max(mx, (u64)(unsigned)vx[ls[e]]);
    int lo = 1, hi = (int)reduce_max(mx);
    while (lo < hi) {                        // hi - lo shrinks every round
      const int mid = lo + (hi - lo + 1) / 2;
      int cnt = 0;
      for (int e = tid; e < n; e += bd) cnt += vx[ls[e]] >= mid ? 1 : 0;
      if (reduce_sum(cnt) >= keep) lo = mid; else hi = mid - 1;
    }
    t = lo;
  }
  const int thr = max(t, max(min_voxels, 0));
  auto kept = [&](int r) -> bool { return vx[r] >= thr && zm[r] - r / g.HW + 1 >= min_slices; };
  int nk = n;
  if (thr > 1 || min_slices > 1) {
    int cnt = 0;
    for (int e = tid; e < n; e += bd) cnt += kept(ls[e]) ? 1 : 0;
    nk = reduce_sum(cnt);
  }
  if (tid < TOPL) keys[tid] = 0ull;
  __syncthreads();
  u64 prev = ~0ull;
  for (int i = 0; i < TOPL && i < nk; ++i) {                  // nk is workgroup-uniform
    u64 best = 0ull;
    for (int e = tid; e < n; e += bd) {
      const int r = ls[e];
      const u64 key = ((u64)(unsigned)vx[r] << 32) | (u64)(0x7fffffff - r);
      if (key < prev && key > best && kept(r)) best = key;
    }
    prev = reduce_max(best);
    if (tid == 0) keys[i] = prev;
  }
  __syncthreads();
  if (tid == 0) {
    thr_out[ch] = thr;
    if (nles) nles[ch] = nk;
  }
  for (int q = tid; q < TOPL * LCOL; q += bd) {
    const int i = q / LCOL, col = q % LCOL;
    const u64 key = keys[i];
    int v = 0, r = -1;
    if (key) {                               // the bounding box starts empty: vol_extent_kernel reduces into it
      r = 0x7fffffff - (int)(key & 0xffffffffull);
      v = col == 0 ? (int)(key >> 32) : col == 1 ? r : col == 2 ? r / g.HW : col == 3 ? zm[r] : col == 4 ? g.H : col == 6 ? g.W : -1;
    }
    if (top) top[ch * (TOPL * LCOL) + q] = v;
    if (col == 0) rank[ch * TOPL + i] = r;
  }
}

// grid (x, C): the runs of a channel's ranked lesions reduce their bounding box into top and add to profile[rank][slice]; runs of one lesion and
// slice are reduced inside the wave first, as in vol_count_kernel
__global__ __launch_bounds__(NT) void vol_extent_kernel(const u64* __restrict__ bits, BitGeo g, const int* __restrict__ parent, const int* __restrict__ rank,
                                                        int* __restrict__ top, int* __restrict__ profile) {
  __shared__ int rr[TOPL];
  const int lane = threadIdx.x & 63;
  const size_t ch = blockIdx.y;
  if (threadIdx.x < TOPL) rr[threadIdx.x] = rank[ch * TOPL + threadIdx.x];
  __syncthreads();
  if (rr[0] < 0) return;                                       // no lesion in this channel (workgroup-uniform, after the only barrier)
  const u64* vol = bits + ch * g.words();
  const int* par = parent + ch * g.DHW;
  for (size_t first = (size_t)blockIdx.x * NT; first < g.words(); first += (size_t)gridDim.x * NT) {   // block-uniform
    const size_t it = first + threadIdx.x;
    u64 c = it < g.words() ? vol[it] : 0ull;
    const Place p = place(it < g.words() ? it : 0, g);           // p.s == 0
    const int a0 = p.n * g.HW + p.y * g.W + p.j * 64;
    while (__any(c != 0ull)) {
      int key = -1, len = 0, x0 = 0;                           // key = rank * N + slice of a run of a ranked lesion
      if (c) {
        const int s = ctz64(c);
        len = runlen(c, s);
        x0 = p.j * 64 + s;
        const int r = par[a0 + s];
        for (int i = 0; i < TOPL; ++i)
          if (rr[i] == r) { key = i * g.D + p.n; break; }
        c &= ~runmask(s, len);
      }
      const bool has = key >= 0;
      u64 pending = __ballot(has);
      while (pending) {                                        // every round clears at least the leader's bit
        const int leader = ctz64(pending);
        const int k = __shfl(key, leader);
        const bool mine = has && key == k;
        if (top) {                                             // columns 0..3 are final: vol_select_kernel wrote them
          const int y0 = wave_min(mine ? p.y : g.H), y1 = wave_max(mine ? p.y : -1);
          const int xa = wave_min(mine ? x0 : g.W), xb = wave_max(mine ? x0 + len - 1 : -1);
          if (lane == leader) {
            int* t = top + (ch * TOPL + k / g.D) * LCOL;
            atomicMin(t + 4, y0);
            atomicMax(t + 5, y1);
            atomicMin(t + 6, xa);
            atomicMax(t + 7, xb);
          }
        }
        if (profile) {
          const int sum = wave_sum(mine ? len : 0);
          if (lane == leader) atomicAdd(profile + ch * TOPL * g.D + k, sum);      // (ch * 32 + rank) * N + slice
        }
        pending &= ~__ballot(mine);
      }
    }
  }
}

namespace {

VScratch carve(void* base, size_t C, int N, int H, int W) {
  VScratch s;
  const size_t NHW = (size_t)N * H * W, W64 = ((size_t)W + 63) / 64;
  s.cap = lesion_capacity(N, H, W);
  Carver cv(base);
  s.parent = cv.take<int>(C * NHW);
  s.vox = cv.take<int>(C * NHW);
  s.zmax = cv.take<int>(C * NHW);
  s.list = cv.take<int>(C * (size_t)s.cap);
  s.nroots = cv.take<int>(C);
  s.thr = cv.take<int>(C);
  s.rank = cv.take<int>(C * TOPL);
  s.a = cv.take<u64>(C * N * H * W64);
  s.b = cv.take<u64>(C * N * H * W64);
  s.bytes = cv.used;
  return s;
}

}  // namespace

// pack and label; with `rank` also count and select: the threshold, the count and the ranking (shared with match.hip: lesions_internal.h)
hipError_t label_and_rank(const float* stack, const BitGeo& g, int C, int full, bool rank, int keep, int min_voxels, int min_slices, const VScratch& s,
                          int* nles, int* top, hipStream_t st) {
  const unsigned gt = item_grid((size_t)C * g.words());
  launch_bits_pack(stack, g.D, g, C, 1, g.D, s.a, st);
  launch_ccl_init(s.a, C, g, 0, s.parent, s.vox, s.zmax, st);
  launch_ccl_merge(s.a, C, g, 0, 1, s.parent, st);
  if (g.D > 1) hipLaunchKernelGGL(vol_across_kernel, dim3(gt), dim3(NT), 0, st, s.a, C, g, full, s.parent);
  launch_ccl_flatten(s.a, C, g, 0, s.parent, st);
  if (!rank) return hipSuccess;                                 // labels only
  hipError_t e = hipMemsetAsync(s.nroots, 0, (size_t)C * sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(vol_count_kernel, dim3(gt), dim3(NT), 0, st, s.a, C, g, s.parent, s.vox, s.zmax, s.list, s.nroots, s.cap);
  hipLaunchKernelGGL(vol_select_kernel, dim3(C), dim3(SEL_NT), 0, st, s.vox, s.zmax, s.list, s.nroots, g, s.cap, keep, min_voxels, min_slices, s.thr,
                     s.rank, nles, top);
  return hipSuccess;
}

hipError_t volume_extents(const BitGeo& g, int C, const VScratch& s, int* top, int* profile, hipStream_t st) {
  if (profile) {
    hipError_t e = hipMemsetAsync(profile, 0, (size_t)C * TOPL * g.D * sizeof(int), st);
    if (e != hipSuccess) return e;
  }
  const unsigned gx = (unsigned)std::min<size_t>((g.words() + NT - 1) / NT, 1u << 16);
  hipLaunchKernelGGL(vol_extent_kernel, dim3(gx, C), dim3(NT), 0, st, s.a, g, s.parent, s.rank, top, profile);
  return hipSuccess;
}

size_t lesions_scratch_bytes(size_t channels, int N, int H, int W) { return carve(nullptr, channels, N, H, W).bytes; }

hipError_t launch_volume_components(const float* stack, int N, int H, int W, int C, int full, void* scratch, int* labels, int* nles, int* top,
                                    int* profile, hipStream_t st) {
  const BitGeo g = bit_geo(N, H, W);
  const VScratch s = carve(scratch, C, N, H, W);
  hipError_t e = label_and_rank(stack, g, C, full, nles || top || profile, 0, 0, 1, s, nles, top, st);
  if (e != hipSuccess) return e;
  if (labels) launch_ccl_labels(s.a, C, g, s.parent, labels, st);
  if (top || profile) {
    e = volume_extents(g, C, s, top, profile, st);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

hipError_t launch_volume_cleanup(const float* stack, int N, int H, int W, int C, int full, int keep, int min_voxels, int min_slices, void* scratch,
                                 float* out, int* nles, int* top, hipStream_t st) {
  const BitGeo g = bit_geo(N, H, W);
  const VScratch s = carve(scratch, C, N, H, W);
  hipError_t e = label_and_rank(stack, g, C, full, true, keep, min_voxels, min_slices, s, nles, top, st);
  if (e != hipSuccess) return e;
  if (top) {
    e = volume_extents(g, C, s, top, nullptr, st);
    if (e != hipSuccess) return e;
  }
  launch_ccl_keep(s.a, C, g, s.parent, s.vox, s.zmax, s.thr, min_slices, s.b, st);
  launch_bits_unpack(s.b, g.D, g, C, 1, g.D, out, st);
  return hipGetLastError();
}

}  // namespace octseg
