// components.hip -- mask clean-up on the GPU: the reference's MaskProcessor (src/data/mask_processor.py:5-37), which process_pair runs over every
// annotated object (convert_int_to_cv.py:191-199): smooth_mask (open, close, dilate with a frame-sized ellipse) and remove_artifacts (keep the
// largest blobs, filled), restated on connected components by PIXEL COUNT (DESIGN.md section 5g states the deviation from cv2.contourArea).
//
// A plane is one (slice, channel) pair of the float32 stack [N][H][W][C] and lives as a bit plane in scratch (bitplanes.h: the layout, and the
// geometry "S sets of D planes" this file uses with S = N * C, D = 1, so parent and area hold pixel indices y * W + x).  An all-zero word is the
// early exit of every kernel, so an empty plane costs its word reads and nothing else.  Every phase that needs a grid-wide order is a launch of
// its own on the caller's stream; no workgroup ever waits on another, there is no flag, no spin and no cooperative launch.
//
// pack / unpack, the labelling (init, merge, flatten, labels; its termination argument) and keep are the shared kernels of bitplanes.hip.  Here:
//
//   morph       one smoothing stage: the row-word technique of render.hip on global words.  A structuring-element row of columns lo..hi is the
//               OR (dilate) / AND (erode) of the word shifted by lo..hi, neighbours' bits shifted in; outside the frame the source reads as the
//               stage's neutral value (OpenCV: "outside does not take part").  Element applied as given (not reflected), anchor k / 2.
//   area        a thread per word adds run lengths to area[root] with integer atomics; a run that starts at its own root appends the root to
//               the plane's component list.
//   select      ONE workgroup per plane: ncomp, the 8 largest by (area descending, first pixel ascending), the k-th largest area, the threshold.
//   bbox        runs of the table's components reduce their inclusive bounding box with atomicMin / atomicMax.
//   hole fill   THE SAME labelling on the complement inside the frame with 4-connectivity; `border` marks the roots of background components
//               that reach the frame border (the outside of the frame as one component), `fill` sets the runs of all others.
#include <algorithm>
#include <cmath>

#include "bitplanes.h"
#include "kernels.h"

namespace octseg {

namespace {

#ifndef OCTSEG_SEL_NT
#define OCTSEG_SEL_NT 256
#endif
constexpr int SEL_NT = OCTSEG_SEL_NT;     // workgroup of select_kernel (any power of two)
constexpr int TOPK = 8, TCOL = 6;

struct Elem { int k, a; int lo[7], hi[7]; };   // cv2.getStructuringElement(MORPH_ELLIPSE, (k, k)): row i is set on columns lo[i]..hi[i]; anchor a

// word j of row y as a morphology stage sees it: outside the frame = the neutral value (0 dilate, 1 erode)
__device__ __forceinline__ u64 rdm(const u64* __restrict__ plane, int y, int j, const BitGeo& g, int ero) {
  if (y < 0 || y >= g.H || j < 0 || j >= g.W64) return ero ? ~0ull : 0ull;
  const u64 w = plane[(size_t)y * g.W64 + j];
  return ero ? w | ~inmask(j, g.W) : w;
}

}  // namespace

// ---- one smoothing stage, a thread per word
__global__ __launch_bounds__(NT) void morph_kernel(const u64* __restrict__ src, u64* __restrict__ dst, int P, BitGeo g, Elem el, int ero) {
  const size_t total = (size_t)P * g.H * g.W64;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const int j = (int)(it % g.W64), y = (int)((it / g.W64) % g.H);
    const u64* plane = src + (it / ((size_t)g.W64 * g.H)) * g.H * g.W64;
    u64 acc = ero ? ~0ull : 0ull;
    for (int i = 0; i < el.k; ++i) {
      if (el.lo[i] > el.hi[i]) continue;
      const int y2 = y + i - el.a;
      const u64 prev = rdm(plane, y2, j - 1, g, ero), cur = rdm(plane, y2, j, g, ero), next = rdm(plane, y2, j + 1, g, ero);
      for (int dx = el.lo[i] - el.a; dx <= el.hi[i] - el.a; ++dx) {           // |dx| <= 3; output bit x takes source bit x + dx
        const u64 sh = dx == 0 ? cur : dx > 0 ? (cur >> dx) | (next << (64 - dx)) : (cur << -dx) | (prev >> (64 + dx));
        acc = ero ? acc & sh : acc | sh;
      }
    }
    dst[it] = acc & inmask(j, g.W);
  }
}

// ---- per-run kernels, a thread per word
// area[root] += run length; a run that starts at its root registers the component (the root is its component's smallest index, so the pixel
// before it is clear and the root starts a run).  cap = the list's capacity, ceil(H / 2) * ceil(W / 2), the most 8-connected components a plane holds
__global__ __launch_bounds__(NT) void area_kernel(const u64* __restrict__ bits, int P, BitGeo g, const int* __restrict__ parent, int* __restrict__ area,
                                                  int* __restrict__ list, int* __restrict__ nroots, int cap) {
  const size_t total = (size_t)P * g.H * g.W64;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    u64 c = bits[it];
    if (!c) continue;
    const int j = (int)(it % g.W64), y = (int)((it / g.W64) % g.H);
    const size_t pl = it / ((size_t)g.W64 * g.H);
    const int p0 = y * g.W + j * 64;
    while (c) {
      const int s = ctz64(c), len = runlen(c, s);
      const int r = parent[pl * g.HW + p0 + s];
      atomicAdd(area + pl * g.HW + r, len);
      if (r == p0 + s) {
        const int slot = atomicAdd(nroots + pl, 1);
        if (slot < cap) list[pl * cap + slot] = r;
      }
      c &= ~runmask(s, len);
    }
  }
}

// One workgroup per plane.  key = area << 32 | (2^31 - 1 - first pixel): the largest key is the largest area, ties to the earliest first pixel;
// keys are distinct.  Round i takes the largest key below round i - 1's.  The k-th largest area for k > 8 is a binary search on the value with a
// count per step.  thr = max(k-th largest area or 0, min_area); table_kept: ncomp and the table describe the components with area >= thr.
__global__ __launch_bounds__(SEL_NT) void select_kernel(const int* __restrict__ area, const int* __restrict__ list, const int* __restrict__ nroots,
                                                        BitGeo g, int cap, int keep, int min_area, int table_kept, int* __restrict__ thr_out,
                                                        int* __restrict__ ncomp, int* __restrict__ top) {
  __shared__ u64 red[SEL_NT];
  __shared__ u64 keys[TOPK];
  const int tid = threadIdx.x, bd = blockDim.x;
  const size_t pl = blockIdx.x;
  const int n = min(max(nroots[pl], 0), cap);
  const int* ar = area + pl * g.HW;
  const int* ls = list + pl * cap;
  u64 prev = ~0ull;
  for (int i = 0; i < TOPK; ++i) {
    u64 best = 0ull;
    for (int e = tid; e < n; e += bd) {
      const int r = ls[e];
      const u64 key = ((u64)(unsigned)ar[r] << 32) | (u64)(0x7fffffff - r);
      if (key < prev && key > best) best = key;
    }
    red[tid] = best;
    __syncthreads();
    for (int s = bd >> 1; s > 0; s >>= 1) {
      if (tid < s && red[tid + s] > red[tid]) red[tid] = red[tid + s];
      __syncthreads();
    }
    prev = red[0];                       // 0 = no component left: later rounds find nothing either
    if (tid == 0) keys[i] = prev;
    __syncthreads();                     // red is rewritten by the next round
  }
  // the count of components with area >= v, workgroup-uniform
  auto count_ge = [&](int v) -> int {
    int cnt = 0;
    for (int e = tid; e < n; e += bd) cnt += ar[ls[e]] >= v ? 1 : 0;
    red[tid] = (u64)cnt;
    __syncthreads();
    for (int s = bd >> 1; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    const int r = (int)red[0];
    __syncthreads();
    return r;
  };
  int t = 0;
  if (keep > 0 && n >= keep) {
    if (keep <= TOPK) {
      t = (int)(keys[keep - 1] >> 32);
    } else {                             // the k-th largest is at most the 8th largest and at least 1; count_ge(lo) >= keep holds throughout
      int lo = 1, hi = (int)(keys[TOPK - 1] >> 32);
      while (lo < hi) {                  // hi - lo shrinks every round
        const int mid = lo + (hi - lo + 1) / 2;
        if (count_ge(mid) >= keep) lo = mid; else hi = mid - 1;
      }
      t = lo;
    }
  }
  const int thr = max(t, max(min_area, 0));
  const int nk = table_kept ? (thr <= 1 ? n : count_ge(thr)) : n;
  if (tid == 0) {
    if (thr_out) thr_out[pl] = thr;
    if (ncomp) ncomp[pl] = nk;
  }
  for (int q = tid; top && q < TOPK * TCOL; q += bd) {
    const int i = q / TCOL, col = q % TCOL;
    const u64 key = keys[i];
    int v = 0;
    if (i < nk && key) {                 // bounding box starts empty: bbox_kernel reduces into it
      const int a = (int)(key >> 32), r = 0x7fffffff - (int)(key & 0xffffffffull);
      v = col == 0 ? a : col == 1 ? r : col == 2 ? g.W : col == 3 ? g.H : -1;
    }
    top[pl * (TOPK * TCOL) + q] = v;
  }
}

__global__ __launch_bounds__(NT) void bbox_kernel(const u64* __restrict__ bits, int P, BitGeo g, const int* __restrict__ parent, int* __restrict__ top) {
  const size_t total = (size_t)P * g.H * g.W64;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    u64 c = bits[it];
    if (!c) continue;
    const int j = (int)(it % g.W64), y = (int)((it / g.W64) % g.H);
    const size_t pl = it / ((size_t)g.W64 * g.H);
    int* t = top + pl * (TOPK * TCOL);
    const int p0 = y * g.W + j * 64;
    while (c) {
      const int s = ctz64(c), len = runlen(c, s);
      const int r = parent[pl * g.HW + p0 + s];
      for (int i = 0; i < TOPK; ++i) {
        if (t[i * TCOL] > 0 && t[i * TCOL + 1] == r) {                  // columns 0 and 1 are final: select_kernel wrote them
          atomicMin(t + i * TCOL + 2, j * 64 + s);
          atomicMin(t + i * TCOL + 3, y);
          atomicMax(t + i * TCOL + 4, j * 64 + s + len - 1);
          atomicMax(t + i * TCOL + 5, y);
          break;
        }
      }
      c &= ~runmask(s, len);
    }
  }
}

// hole fill, after init / merge / flatten on the complement: area[root] (0 since init) becomes 1 for background components on the frame border
__global__ __launch_bounds__(NT) void border_kernel(const u64* __restrict__ bits, int P, BitGeo g, const int* __restrict__ parent, int* __restrict__ area) {
  const size_t total = (size_t)P * g.H * g.W64;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const int j = (int)(it % g.W64), y = (int)((it / g.W64) % g.H);
    const size_t pl = it / ((size_t)g.W64 * g.H);
    u64 edge = 0ull;
    if (y == 0 || y == g.H - 1) edge = ~0ull;
    if (j == 0) edge |= 1ull;
    if (j == g.W64 - 1) edge |= 1ull << ((g.W - 1) & 63);
    u64 c = ~bits[it] & inmask(j, g.W) & edge;
    const int p0 = y * g.W + j * 64;
    while (c) {
      const int s = ctz64(c);
      area[pl * g.HW + parent[pl * g.HW + parent[pl * g.HW + p0 + s]]] = 1;      // pixel -> run start -> root; every writer stores the same value
      c &= c - 1ull;
    }
  }
}

__global__ __launch_bounds__(NT) void fill_kernel(u64* __restrict__ bits, int P, BitGeo g, const int* __restrict__ parent, const int* __restrict__ area) {
  const size_t total = (size_t)P * g.H * g.W64;
  for (size_t it = (size_t)blockIdx.x * NT + threadIdx.x; it < total; it += (size_t)gridDim.x * NT) {
    const int j = (int)(it % g.W64), y = (int)((it / g.W64) % g.H);
    const size_t pl = it / ((size_t)g.W64 * g.H);
    const u64 w = bits[it];
    u64 c = ~w & inmask(j, g.W), o = 0ull;
    const int p0 = y * g.W + j * 64;
    while (c) {
      const int s = ctz64(c), len = runlen(c, s);
      const u64 m = runmask(s, len);
      if (area[pl * g.HW + parent[pl * g.HW + p0 + s]] == 0) o |= m;     // not connected to the border through background: a hole
      c &= ~m;
    }
    if (o) bits[it] = w | o;
  }
}

namespace {

struct Scratch {
  int *parent, *area, *list, *nroots, *thr;
  u64 *a, *b;
  int cap;
  size_t bytes;
};

Scratch carve(void* base, size_t P, int H, int W) {
  Scratch s;
  const size_t HW = (size_t)H * W, W64 = ((size_t)W + 63) / 64;
  s.cap = (int)((((size_t)H + 1) / 2) * (((size_t)W + 1) / 2));
  Carver cv(base);
  s.parent = cv.take<int>(P * HW);
  s.area = cv.take<int>(P * HW);
  s.list = cv.take<int>(P * (size_t)s.cap);
  s.nroots = cv.take<int>(P);
  s.thr = cv.take<int>(P);
  s.a = cv.take<u64>(P * H * W64);
  s.b = cv.take<u64>(P * H * W64);
  s.bytes = cv.used;
  return s;
}

Elem ellipse(int k) {   // OpenCV 4.8.1 getStructuringElement(MORPH_ELLIPSE): postprocess.ellipse states the same
  Elem e;
  e.k = k; e.a = k / 2;
  const int r = k / 2, c = k / 2;
  const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
  for (int i = 0; i < 7; ++i) { e.lo[i] = 1; e.hi[i] = 0; }
  for (int i = 0; i < k; ++i) {
    const int dy = i - r;
    if (std::abs(dy) > r) continue;
    const int dx = (int)std::nearbyint(c * std::sqrt((r * r - dy * dy) * inv_r2));      // cvRound: half to even
    e.lo[i] = std::max(c - dx, 0);
    e.hi[i] = std::min(c + dx, k - 1);
  }
  return e;
}

// init / merge / flatten of the planes in `bits` (inv: of their complement inside the frame)
void label_planes(const u64* bits, int P, const BitGeo& g, int inv, int conn8, const Scratch& s, hipStream_t st) {
  launch_ccl_init(bits, P, g, inv, s.parent, s.area, nullptr, st);
  launch_ccl_merge(bits, P, g, inv, conn8, s.parent, st);
  launch_ccl_flatten(bits, P, g, inv, s.parent, st);
}

}  // namespace

size_t components_scratch_bytes(size_t planes, int H, int W) { return carve(nullptr, planes, H, W).bytes; }

hipError_t launch_stack_components(const float* stack, int N, int H, int W, int C, void* scratch, int* labels, int* ncomp, int* top, hipStream_t st) {
  const int P = N * C;
  const BitGeo g = bit_geo(1, H, W);
  const Scratch s = carve(scratch, P, H, W);
  const size_t words = (size_t)P * g.H * g.W64;
  launch_bits_pack(stack, N, g, C, C, 1, s.a, st);
  label_planes(s.a, P, g, 0, 1, s, st);
  if (labels) launch_ccl_labels(s.a, P, g, s.parent, labels, st);
  if (ncomp || top) {
    hipError_t e = hipMemsetAsync(s.nroots, 0, (size_t)P * sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(area_kernel, dim3(item_grid(words)), dim3(NT), 0, st, s.a, P, g, s.parent, s.area, s.list, s.nroots, s.cap);
    hipLaunchKernelGGL(select_kernel, dim3(P), dim3(SEL_NT), 0, st, s.area, s.list, s.nroots, g, s.cap, 0, 0, 0, (int*)nullptr, ncomp, top);
    if (top) hipLaunchKernelGGL(bbox_kernel, dim3(item_grid(words)), dim3(NT), 0, st, s.a, P, g, s.parent, top);
  }
  return hipGetLastError();
}

hipError_t launch_stack_cleanup(const float* stack, int N, int H, int W, int C, int smooth_k, int keep, int min_area, int fill_holes, void* scratch,
                                float* out, int* ncomp, int* top, hipStream_t st) {
  const int P = N * C;
  const BitGeo g = bit_geo(1, H, W);
  const Scratch s = carve(scratch, P, H, W);
  const size_t words = (size_t)P * g.H * g.W64;
  u64 *cur = s.a, *other = s.b;
  launch_bits_pack(stack, N, g, C, C, 1, cur, st);
  if (smooth_k > 1) {                                        // erode, dilate (open); dilate, erode (close); dilate
    const Elem el = ellipse(smooth_k);
    const int ero[5] = {1, 0, 0, 1, 0};
    for (int i = 0; i < 5; ++i) {
      hipLaunchKernelGGL(morph_kernel, dim3(item_grid(words)), dim3(NT), 0, st, cur, other, P, g, el, ero[i]);
      std::swap(cur, other);
    }
  }
  const bool filter = keep > 0 || min_area > 1;
  if (filter || ncomp || top) {
    label_planes(cur, P, g, 0, 1, s, st);
    hipError_t e = hipMemsetAsync(s.nroots, 0, (size_t)P * sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(area_kernel, dim3(item_grid(words)), dim3(NT), 0, st, cur, P, g, s.parent, s.area, s.list, s.nroots, s.cap);
    hipLaunchKernelGGL(select_kernel, dim3(P), dim3(SEL_NT), 0, st, s.area, s.list, s.nroots, g, s.cap, keep, min_area, 1, s.thr, ncomp, top);
    if (top) hipLaunchKernelGGL(bbox_kernel, dim3(item_grid(words)), dim3(NT), 0, st, cur, P, g, s.parent, top);
    if (filter) {
      launch_ccl_keep(cur, P, g, s.parent, s.area, nullptr, s.thr, 1, other, st);
      std::swap(cur, other);
    }
  }
  if (fill_holes) {                                          // the same labelling on the complement, 4-connected
    label_planes(cur, P, g, 1, 0, s, st);
    hipLaunchKernelGGL(border_kernel, dim3(item_grid(words)), dim3(NT), 0, st, cur, P, g, s.parent, s.area);
    hipLaunchKernelGGL(fill_kernel, dim3(item_grid(words)), dim3(NT), 0, st, cur, P, g, s.parent, s.area);
  }
  launch_bits_unpack(cur, N, g, C, C, 1, out, st);
  return hipGetLastError();
}

}  // namespace octseg
