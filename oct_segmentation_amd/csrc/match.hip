// match.hip -- predicted against annotated lesions (no reference counterpart): two mask stacks of the same extents are each
// labelled and ranked as lesions.hip does it (section 5j: the same kernels through lesions_internal.h's label_and_rank, keep = 0, min_voxels = 0,
// min_slices = 1), then ONE pass over both sets of bit planes fills, per channel, the 33 x 33 contingency table of the voxels both sides set, by
// the RANK of their lesion on either side (0..31 = ranked, 32 = "rest": a lesion beyond the 32 listed), and the per-slice counts |P & T|, |P|, |T|.
// Side 0 = pred, side 1 = truth.  Everything is integer; integer adds commute, so the result does not depend on the order of any atomic.
//
// The bits, parent and the geometry are those of lesions.hip: word j of row y of slice n of channel c stands at ((c * N + n) * H + y) * W64 + j of
// a side's planes, parent is int32 [C][N * H * W] per side.  Every phase that needs a grid-wide order is a launch of its own on the caller's
// stream; no workgroup ever waits on another, there is no flag, no spin, no cooperative launch and no inline assembly; nothing is allocated.
//
//   label, rank   side 0, then side 1, each: pack, init, merge, across, flatten, count, select (and extents where `top` is asked for).  parent, the
//                 bits and the 32 ranked roots are per side and outlive the labelling; vox, zmax, the lesion list, the counters and the thresholds
//                 are one set that side 1 uses after side 0 (init rewrites vox / zmax at every run start, the only places ever read)
//   match         grid (x, C), a thread per word.  LDS: the two sides' 32 ranked roots and a 33 x 33 int table.  With a = pred's word and b =
//                 truth's: the three popcounts go to frames[c][slice] (summed inside the wave when its 64 words lie in one slice, else per slice by
//                 the ballot loop of vol_extent_kernel); then m = a & b run by run.  A maximal run of m lies inside one horizontal run of a and one of
//                 b, so all of it belongs to ONE lesion per side: one root lookup per side, one rank lookup per side against the LDS roots, one LDS
//                 add of the run length.  A run of m need not start where a run of a or b starts, and flatten leaves only run starts one hop from
//                 their root: every other pixel points at the start of its run inside its word (init), so the root is parent[parent[v]] -- for a run
//                 start, too, because a root points at itself.  At the end the workgroup adds its non-zero cells to the channel's table.
//   tables        nles and top of the two sides, which select / extents wrote side by side in scratch, interleaved into [C][2] and [C][2][32][8]
//
// The loops: run loops clear at least one set bit of a 64-bit word per round; grid-stride loops advance by the grid and run on the block's base
// index, so every lane of a workgroup takes the same rounds and reaches the one barrier pair; the rank lookup runs at most 32 rounds; the per-slice
// reduction handles one slice per round and clears at least its leader's bit of a 64-bit ballot; the flush and the table copy stride by the
// workgroup / grid.  The union-find loops are those of bitplanes.h, where their termination argument stands.
#include <algorithm>

#include "bitplanes.h"
#include "kernels.h"
#include "lesions_internal.h"

namespace octseg {

namespace {

constexpr int RANKS = TOPL + 1;                  // 0..31 ranked, 32 = rest
constexpr int CELLS = RANKS * RANKS;

// rank of root r among the 32 ranked roots (-1 = none; roots are >= 0), 32 = not listed
__device__ __forceinline__ int rank_of(const int* rr, int r) {
  for (int i = 0; i < TOPL; ++i)
    if (rr[i] == r) return i;
  return TOPL;
}

}  // namespace

__global__ __launch_bounds__(NT) void vol_match_kernel(const u64* __restrict__ bits_p, const u64* __restrict__ bits_t, BitGeo g,
                                                       const int* __restrict__ parent_p, const int* __restrict__ parent_t,
                                                       const int* __restrict__ rank_p, const int* __restrict__ rank_t, int* __restrict__ overlap,
                                                       int* __restrict__ frames) {
  __shared__ int rp[TOPL], rt[TOPL];
  __shared__ int tab[CELLS];
  const int lane = threadIdx.x & 63;
  const size_t ch = blockIdx.y, words = g.words(), pw = (size_t)g.H * g.W64;
  if (threadIdx.x < TOPL) {
    rp[threadIdx.x] = rank_p[ch * TOPL + threadIdx.x];
    rt[threadIdx.x] = rank_t[ch * TOPL + threadIdx.x];
  }
  for (int q = threadIdx.x; q < CELLS; q += NT) tab[q] = 0;
  __syncthreads();
  const u64* vp = bits_p + ch * words;
  const u64* vt = bits_t + ch * words;
  const int* pp = parent_p + ch * g.DHW;
  const int* pt = parent_t + ch * g.DHW;
  for (size_t first = (size_t)blockIdx.x * NT; first < words; first += (size_t)gridDim.x * NT) {        // block-uniform
    const size_t it = first + threadIdx.x;
    const bool in = it < words;
    const u64 a = in ? vp[it] : 0ull, b = in ? vt[it] : 0ull;
    if (!__any((a | b) != 0ull)) continue;                       // wave-uniform; no barrier inside the loop
    const Place p = place(in ? it : 0, g);                       // p.s == 0
    u64 m = a & b;
    if (frames) {
      const int ca = __popcll(a), cb = __popcll(b), cm = __popcll(m);
      const size_t w0 = first + (threadIdx.x & ~63);             // the wave's first word (< words: one of its lanes holds a set bit)
      const size_t w1 = w0 + 63 < words ? w0 + 63 : words - 1;
      int* fr = frames + ch * g.D * 3;
      if (w0 / pw == w1 / pw) {                                  // the wave's words share a slice
        const int sm = wave_sum(cm), sa = wave_sum(ca), sb = wave_sum(cb);
        if (lane == 0) {
          int* f = fr + (w0 / pw) * 3;
          if (sm) atomicAdd(f, sm);
          if (sa) atomicAdd(f + 1, sa);
          if (sb) atomicAdd(f + 2, sb);
        }
      } else {
        const bool has = (a | b) != 0ull;
        u64 pending = __ballot(has);
        while (pending) {                                        // every round clears at least the leader's bit
          const int leader = ctz64(pending);
          const int k = __shfl(p.n, leader);
          const bool mine = has && p.n == k;
          const int sm = wave_sum(mine ? cm : 0), sa = wave_sum(mine ? ca : 0), sb = wave_sum(mine ? cb : 0);
          if (lane == leader) {
            int* f = fr + (size_t)k * 3;
            if (sm) atomicAdd(f, sm);
            if (sa) atomicAdd(f + 1, sa);
            if (sb) atomicAdd(f + 2, sb);
          }
          pending &= ~__ballot(mine);
        }
      }
    }
    const int a0 = p.n * g.HW + p.y * g.W + p.j * 64;
    while (m) {                                                  // every round clears the run it handled
      const int s = ctz64(m), len = runlen(m, s);
      const int i = rank_of(rp, pp[pp[a0 + s]]), j = rank_of(rt, pt[pt[a0 + s]]);      // pixel -> run start -> root
      atomicAdd(&tab[i * RANKS + j], len);
      m &= ~runmask(s, len);
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < CELLS; q += NT) {
    const int v = tab[q];
    if (v) atomicAdd(overlap + ch * CELLS + q, v);
  }
}

// nles [C][2] and top [C][2][32][8] from the per-side tables nles_s [2][C], top_s [2][C][32][8]
__global__ __launch_bounds__(NT) void vol_match_tables_kernel(const int* __restrict__ nles_s, const int* __restrict__ top_s, int C, int* __restrict__ nles,
                                                              int* __restrict__ top) {
  const int per = TOPL * LCOL, total = C * 2 * (top ? per : 1);
  for (int q = blockIdx.x * NT + threadIdx.x; q < total; q += gridDim.x * NT) {
    if (top) {
      const int e = q % per, side = q / per % 2, c = q / (2 * per);
      top[q] = top_s[(side * C + c) * per + e];
      if (e == 0) nles[c * 2 + side] = nles_s[side * C + c];
    } else {
      nles[q] = nles_s[(q % 2) * C + q / 2];
    }
  }
}

namespace {

struct MScratch {
  VScratch side[2];
  int *nles, *top;                // [2][C], [2][C][32][8]
  size_t bytes;
};

// parent of both sides, then what the sides share (vox, zmax, list, nroots, thr), then the per-side small tables and the two sets of bit planes
MScratch carve_match(void* base, size_t C, int N, int H, int W) {
  MScratch m;
  const size_t NHW = (size_t)N * H * W, W64 = ((size_t)W + 63) / 64;
  const int cap = lesion_capacity(N, H, W);
  Carver cv(base);
  int* parent0 = cv.take<int>(C * NHW);
  int* parent1 = cv.take<int>(C * NHW);
  int* vox = cv.take<int>(C * NHW);
  int* zmax = cv.take<int>(C * NHW);
  int* list = cv.take<int>(C * (size_t)cap);
  int* nroots = cv.take<int>(C);
  int* thr = cv.take<int>(C);
  int* rank0 = cv.take<int>(C * TOPL);
  int* rank1 = cv.take<int>(C * TOPL);
  m.nles = cv.take<int>(2 * C);
  m.top = cv.take<int>(2 * C * TOPL * LCOL);
  u64* a0 = cv.take<u64>(C * N * H * W64);
  u64* a1 = cv.take<u64>(C * N * H * W64);
  m.bytes = cv.used;
  m.side[0] = VScratch{parent0, vox, zmax, list, nroots, thr, rank0, a0, nullptr, cap, m.bytes};
  m.side[1] = VScratch{parent1, vox, zmax, list, nroots, thr, rank1, a1, nullptr, cap, m.bytes};
  return m;
}

}  // namespace

size_t match_scratch_bytes(size_t channels, int N, int H, int W) { return carve_match(nullptr, channels, N, H, W).bytes; }

hipError_t launch_volume_match(const float* pred, const float* truth, int N, int H, int W, int C, int full, void* scratch, int* nles, int* top,
                               int* overlap, int* frames, hipStream_t st) {
  const BitGeo g = bit_geo(N, H, W);
  const MScratch m = carve_match(scratch, C, N, H, W);
  hipError_t e = hipMemsetAsync(overlap, 0, (size_t)C * CELLS * sizeof(int), st);
  if (e != hipSuccess) return e;
  if (frames) {
    e = hipMemsetAsync(frames, 0, (size_t)C * N * 3 * sizeof(int), st);
    if (e != hipSuccess) return e;
  }
  for (int side = 0; side < 2; ++side) {
    int* top_s = top ? m.top + (size_t)side * C * TOPL * LCOL : nullptr;
    e = label_and_rank(side ? truth : pred, g, C, full, true, 0, 0, 1, m.side[side], m.nles + (size_t)side * C, top_s, st);
    if (e != hipSuccess) return e;
    if (top) {
      e = volume_extents(g, C, m.side[side], top_s, nullptr, st);
      if (e != hipSuccess) return e;
    }
  }
  const unsigned gx = (unsigned)std::min<size_t>((g.words() + NT - 1) / NT, 1u << 16);
  hipLaunchKernelGGL(vol_match_kernel, dim3(gx, C), dim3(NT), 0, st, m.side[0].a, m.side[1].a, g, m.side[0].parent, m.side[1].parent, m.side[0].rank,
                     m.side[1].rank, overlap, frames);
  const int items = C * 2 * (top ? TOPL * LCOL : 1);
  hipLaunchKernelGGL(vol_match_tables_kernel, dim3((items + NT - 1) / NT), dim3(NT), 0, st, m.nles, m.top, C, nles, top);
  return hipGetLastError();
}

}  // namespace octseg
