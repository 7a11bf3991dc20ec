// contours.hip -- mask outlines on the GPU: the CRACK CONTOURS of every (slice, channel) plane of the float32 stack [N][H][W][C] (include/octseg.h
// states the definitions, DESIGN.md section 5n the algorithm).  A contour is a closed polygon along pixel sides with the set pixels on its right:
// unique, integer, and it fills back to the mask bit for bit.  Not cv2.findContours' pixel-centre border.
//
// VERTEX WORDS.  Vertex (x, y), 0 <= x <= W, 0 <= y <= H, touches the pixels a = (y-1, x-1), b = (y-1, x), c = (y, x-1), d = (y, x).  64 vertices of
// a vertex row are one item: from the bit planes of bitplanes.h, b and d are the words of the two pixel rows, a and c the same words shifted by one
// bit with the left neighbour's top bit carried in (the word and its three neighbours).  The edges that START at the vertices are four masks
//   E = d & ~b   S = c & ~d   W = a & ~c   N = b & ~a
// and an edge's id ((y * (W + 1) + x) * 4 + dir) orders the edges of a plane by vertex row, vertex, direction: the order in which a scan over the
// vertex words' popcounts numbers them.  Edge e of the call is that number: the COMPACT index, monotone in (plane, id).
//
// The phases, each a launch (or three: the scans) on the caller's stream; no workgroup waits on another, nothing spins, nothing is allocated:
//   pack, init / merge / flatten    the bit planes and the 8-connected labels (bitplanes.hip), for the label column
//   scan 1     exclusive edge count in front of every vertex word; the total decides the overflow and, per plane, the number of rounds
//   links      every edge: its predecessor (the edge that ends where it starts; at a vertex with two set diagonal pixels the one that turns from
//              (dir + 1) % 4), its id, whether it is a corner (the predecessor's direction differs)
//   jump       ceil(log2(most edges of a plane)) rounds of pointer jumping over the predecessor links carrying (smallest compact index in the
//              window, steps back to its first occurrence): afterwards every edge knows its LEADER and its RANK behind it
//   scan 2     leader flags -> contour index; cycle lengths (1 + rank of the leader's predecessor) -> the contour's base
//   scatter    order[base + rank] = edge; the leader writes its table row (plane, edges, empty box, label)
//   scan 3     corner flags in that order -> the vertex position
//   emit       vertices; area (S edges add x, N edges subtract x) and the box by integer atomics keyed by the contour: order-independent
//   finish     ncont per plane, the overflow of the contour and vertex capacities
// The scans are written here (tile sums, one workgroup over the sums, tile scan): three small kernels over a functor, no temporary-storage
// protocol and no second dependency; the sums saturate at 2^31 - 1 so that a stack with more edges than an int holds still reads as an overflow.
#include <algorithm>

#include "bitplanes.h"
#include "kernels.h"

namespace octseg {

namespace {

constexpr int ITEMS = 8, TILE = NT * ITEMS;          // scan: items per thread, per workgroup
constexpr int SAT = 0x7fffffff;
constexpr int CF = CONTOUR_FIELDS;
enum { F_PLANE, F_FIRST, F_NVERT, F_AREA, F_EDGES, F_X0, F_Y0, F_X1, F_Y1, F_LABEL };
enum { CT_NE, CT_ROUNDS, CT_ETOT, CT_PAD, CT_LEAD, CT_LEN, CT_VERT, CT_PAD2, CT_INTS };      // the call's device-side scalars

struct I2 { int x, y; };                             // a pair of non-negative sums, saturating
__host__ __device__ __forceinline__ int sat_add(int a, int b) {
  const unsigned s = (unsigned)a + (unsigned)b;
  return s > (unsigned)SAT ? SAT : (int)s;
}
__host__ __device__ __forceinline__ I2 operator+(const I2& a, const I2& b) { return I2{sat_add(a.x, b.x), sat_add(a.y, b.y)}; }

// the vertex words of a plane: H + 1 rows of W / 64 + 1 words (vertex W is the last one)
struct VGeo {
  BitGeo g;
  int VH, VW64;
  __host__ __device__ size_t per_plane() const { return (size_t)VH * VW64; }
};

struct Quad { u64 a, b, c, d; };
struct Masks { u64 e, s, w, n; };
__device__ __forceinline__ Masks out_masks(const Quad& q) { return Masks{q.d & ~q.b, q.c & ~q.d, q.a & ~q.c, q.b & ~q.a}; }
__device__ __forceinline__ int count_edges(const Masks& m) { return __popcll(m.e) + __popcll(m.s) + __popcll(m.w) + __popcll(m.n); }
// contour vertices at 64 lattice points: one where an odd number of the four pixels is set, two where two diagonal pixels are
__device__ __forceinline__ int count_corners(const Quad& q) {
  const u64 odd = q.a ^ q.b ^ q.c ^ q.d, diag = (q.a & q.d & ~q.b & ~q.c) | (q.b & q.c & ~q.a & ~q.d);
  return __popcll(odd) + 2 * __popcll(diag);
}
// vertex word jv of vertex row yv; all clear outside 0 <= yv <= H, 0 <= jv < VW64 (rdw reads 0 outside the frame)
__device__ __forceinline__ Quad quad(const u64* __restrict__ plane, int yv, int jv, const BitGeo& g) {
  const u64 b = rdw(plane, yv - 1, jv, g), d = rdw(plane, yv, jv, g);
  const u64 bl = rdw(plane, yv - 1, jv - 1, g), dl = rdw(plane, yv, jv - 1, g);
  return Quad{(b << 1) | (bl >> 63), b, (d << 1) | (dl >> 63), d};
}
__device__ __forceinline__ u64 dir_mask(const Masks& m, int dir) { return dir == 0 ? m.e : dir == 1 ? m.s : dir == 2 ? m.w : m.n; }
// the number of the word's edges in front of (vertex bit, dir)
__device__ __forceinline__ int edge_rank(const Masks& m, int bit, int dir) {
  const u64 lo = (1ull << bit) - 1ull;
  int r = __popcll(m.e & lo) + __popcll(m.s & lo) + __popcll(m.w & lo) + __popcll(m.n & lo);
  for (int k = 0; k < dir; ++k) r += (int)((dir_mask(m, k) >> bit) & 1ull);
  return r;
}

// ---- scan inputs and outputs
struct WordEdgesIn {                                   // item = vertex word -> its edge count
  const u64* bits; VGeo v;
  __device__ I2 operator()(size_t it) const {
    const int jv = (int)(it % v.VW64), yv = (int)((it / v.VW64) % v.VH);
    const u64* plane = bits + (it / v.per_plane()) * v.g.H * v.g.W64;
    return I2{count_edges(out_masks(quad(plane, yv, jv, v.g))), 0};
  }
};
struct FirstOut { int* dst; __device__ void operator()(size_t i, const I2& p) const { dst[i] = p.x; } };
struct PairOut { I2* dst; __device__ void operator()(size_t i, const I2& p) const { dst[i] = p; } };
struct LeaderIn {                                      // item = edge -> (is a leader, its cycle length)
  const int4* a; const int4* b; const int* pred; const int* ctl;
  __device__ I2 operator()(size_t e) const {
    const int4* fin = (ctl[CT_ROUNDS] & 1) ? b : a;
    if (fin[e].y != (int)e) return I2{0, 0};
    return I2{1, 1 + fin[pred[e]].z};
  }
};
struct CornerIn {                                      // item = position in contour order -> is a corner
  const int* order; const unsigned* info; const int* ctl;
  __device__ I2 operator()(size_t q) const {
    const unsigned e = (unsigned)order[q];
    return I2{e < (unsigned)ctl[CT_NE] ? (int)(info[e] >> 31) : 0, 0};       // (always inside: order is a permutation)
  }
};

// inclusive scan over the workgroup's NT values; `sh` is free again after the call
__device__ __forceinline__ I2 block_inclusive(I2 v, I2* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < NT; o <<= 1) {
    const I2 t = tid >= o ? sh[tid - o] : I2{0, 0};
    __syncthreads();
    sh[tid] = sh[tid] + t;
    __syncthreads();
  }
  const I2 r = sh[tid];
  __syncthreads();
  return r;
}

}  // namespace

// ---- the scan: tile sums, one workgroup over the sums, tile scan.  n = *nptr (a device-side count) or nfix; tiles past n sum to zero
template <class In>
__global__ __launch_bounds__(NT) void scan_sums_kernel(In in, const int* __restrict__ nptr, size_t nfix, I2* __restrict__ partial) {
  __shared__ I2 sh[NT];
  const size_t n = nptr ? (size_t)*nptr : nfix, t0 = (size_t)blockIdx.x * TILE;
  I2 s{0, 0};
  for (int k = 0; k < ITEMS; ++k) {
    const size_t i = t0 + (size_t)k * NT + threadIdx.x;
    if (i < n) s = s + in(i);
  }
  const I2 inc = block_inclusive(s, sh);
  if (threadIdx.x == NT - 1) partial[blockIdx.x] = inc;
}

__global__ __launch_bounds__(NT) void scan_partials_kernel(I2* __restrict__ partial, int nb, int* __restrict__ total) {
  __shared__ I2 sh[NT];
  __shared__ I2 carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = I2{0, 0};
  __syncthreads();
  for (int base = 0; base < nb; base += NT) {
    const int i = base + tid;
    const I2 v = i < nb ? partial[i] : I2{0, 0};
    const I2 inc = block_inclusive(v, sh);
    const I2 c = carry;
    sh[tid] = inc;
    __syncthreads();
    if (i < nb) partial[i] = tid ? c + sh[tid - 1] : c;     // exclusive: the tiles in front
    __syncthreads();
    if (tid == NT - 1) carry = c + inc;
    __syncthreads();
  }
  if (tid == 0) { total[0] = carry.x; total[1] = carry.y; }
}

template <class In, class Out>
__global__ __launch_bounds__(NT) void scan_tiles_kernel(In in, Out out, const int* __restrict__ nptr, size_t nfix, const I2* __restrict__ partial) {
  __shared__ I2 sh[NT];
  const size_t n = nptr ? (size_t)*nptr : nfix, t0 = (size_t)blockIdx.x * TILE + (size_t)threadIdx.x * ITEMS;
  if ((size_t)blockIdx.x * TILE >= n) return;             // workgroup-uniform
  I2 v[ITEMS], s{0, 0};
  for (int k = 0; k < ITEMS; ++k) {
    v[k] = t0 + k < n ? in(t0 + k) : I2{0, 0};
    s = s + v[k];
  }
  const I2 inc = block_inclusive(s, sh);
  sh[threadIdx.x] = inc;
  __syncthreads();
  I2 run = partial[blockIdx.x];
  if (threadIdx.x) run = run + sh[threadIdx.x - 1];
  for (int k = 0; k < ITEMS; ++k) {
    if (t0 + k < n) out(t0 + k, run);
    run = run + v[k];
  }
}

// ---- the local counts, straight from the stack: a wave per vertex word, a lane per pixel, the channels' words by ballot.  Every wave owns a
// contiguous range of items and lane c carries channel c's sums until the slice changes: few atomics
__global__ __launch_bounds__(NT) void contour_counts_kernel(const float* __restrict__ stack, int N, int H, int W, int C, int vec,
                                                            unsigned long long* __restrict__ counts) {
  const int lane = threadIdx.x & 63, VH = H + 1, VW64 = W / 64 + 1;
  const size_t nw = (size_t)gridDim.x * WAVES, wave = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
  const size_t total = (size_t)N * VH * VW64, per = (total + nw - 1) / nw;
  const size_t begin = wave * per < total ? wave * per : total, end = begin + per < total ? begin + per : total;
  unsigned long long ne = 0ull, nv = 0ull;
  long long cur = -1;
  auto flush = [&]() {
    if (cur >= 0 && lane < C) {
      if (ne) atomicAdd(counts + ((size_t)cur * C + lane) * 2, ne);
      if (nv) atomicAdd(counts + ((size_t)cur * C + lane) * 2 + 1, nv);
    }
    ne = nv = 0ull;
  };
  for (size_t it = begin; it < end; ++it) {
    const int jv = (int)(it % VW64), yv = (int)((it / VW64) % VH);
    const long long n = (long long)(it / ((size_t)VH * VW64));
    if (n != cur) { flush(); cur = n; }
    const int x = jv * 64 + lane;
    const bool up = yv > 0, dn = yv < H, in = x < W, left = lane == 0 && jv > 0;       // the pixel x - 1 of lane 0 carries into bit 0
    const float* rowu = stack + ((size_t)n * H + (up ? yv - 1 : 0)) * W * C;
    const float* rowd = stack + ((size_t)n * H + (dn ? yv : 0)) * W * C;
    for (int c0 = 0; c0 < C; c0 += 4) {
      float u[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f}, ul[4] = {0.f, 0.f, 0.f, 0.f}, dl[4] = {0.f, 0.f, 0.f, 0.f};
      auto ld = [&](const float* px, float* o) {
        if (vec) {
          const float4 t = *(const float4*)px;
          o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
        } else {
          for (int k = 0; k < 4; ++k) if (c0 + k < C) o[k] = px[c0 + k];
        }
      };
      if (up && in) ld(rowu + (size_t)x * C, u);
      if (dn && in) ld(rowd + (size_t)x * C, d);
      if (up && left) ld(rowu + (size_t)(x - 1) * C, ul);
      if (dn && left) ld(rowd + (size_t)(x - 1) * C, dl);
      for (int k = 0; k < 4; ++k) {
        if (c0 + k >= C) break;                                                       // wave-uniform
        const u64 b = __ballot(u[k] != 0.f), dd = __ballot(d[k] != 0.f);
        const u64 cb = __ballot(ul[k] != 0.f) & 1ull, cd = __ballot(dl[k] != 0.f) & 1ull;
        const Quad q{(b << 1) | cb, b, (dd << 1) | cd, dd};
        if (lane == c0 + k) {
          ne += (unsigned)count_edges(out_masks(q));
          nv += (unsigned)count_corners(q);
        }
      }
    }
  }
  flush();
}

// ---- after scan 1: the overflow of the edge capacity and the number of jump rounds.  One workgroup; ctl[CT_ETOT] is the scan's total
__global__ __launch_bounds__(NT) void contour_setup_kernel(const int* __restrict__ woff, int P, size_t vwp, int edge_capacity, int* __restrict__ ctl,
                                                           int* __restrict__ overflow) {
  __shared__ int most;
  if (threadIdx.x == 0) most = 0;
  __syncthreads();
  const int etot = ctl[CT_ETOT];
  const bool over = etot > edge_capacity || etot >= SAT;
  int mine = 0;
  for (int p = threadIdx.x; p < P && !over; p += NT) {
    const int s = woff[(size_t)p * vwp], t = p + 1 < P ? woff[(size_t)(p + 1) * vwp] : etot;
    mine = max(mine, t - s);
  }
  atomicMax(&most, mine);
  __syncthreads();
  if (threadIdx.x == 0) {
    int r = 0;
    while (r < 31 && (1ll << r) < (long long)most) ++r;          // 2^r >= the longest cycle any plane can hold
    ctl[CT_NE] = over ? 0 : etot;
    ctl[CT_ROUNDS] = r;
    if (over) *overflow = 1;
  }
}

// ---- links: a wave per vertex word, a lane per vertex (at most two edges start at a vertex)
__global__ __launch_bounds__(NT) void contour_links_kernel(const u64* __restrict__ bits, int P, VGeo v, const int* __restrict__ woff,
                                                           const int* __restrict__ ctl, int* __restrict__ pred, unsigned* __restrict__ info,
                                                           int4* __restrict__ node) {
  if (ctl[CT_NE] == 0) return;
  const int lane = threadIdx.x & 63;
  const size_t nw = (size_t)gridDim.x * WAVES, total = (size_t)P * v.per_plane();
  for (size_t it = (size_t)blockIdx.x * WAVES + (threadIdx.x >> 6); it < total; it += nw) {
    const int jv = (int)(it % v.VW64), yv = (int)((it / v.VW64) % v.VH);
    const u64* plane = bits + (it / v.per_plane()) * v.g.H * v.g.W64;
    const Quad q = quad(plane, yv, jv, v.g);
    const Masks m = out_masks(q);
    if (!(m.e | m.s | m.w | m.n)) continue;                                          // wave-uniform
    // the words an edge can come from: left, right, above, below (all clear outside the plane's vertex rows)
    const Masks ml = out_masks(quad(plane, yv, jv - 1, v.g)), mr = out_masks(quad(plane, yv, jv + 1, v.g));
    const Masks mu = out_masks(quad(plane, yv - 1, jv, v.g)), md = out_masks(quad(plane, yv + 1, jv, v.g));
    // edges that END at the vertex, by their direction: E = top of c, S = right of a, W = bottom of b, N = left of d
    const Masks in{q.c & ~q.a, q.a & ~q.b, q.b & ~q.d, q.d & ~q.c};
    const int base = woff[it];
    int r = base + edge_rank(m, lane, 0);
    for (int dir = 0; dir < 4; ++dir) {
      if (!((dir_mask(m, dir) >> lane) & 1ull)) continue;
      // the predecessor's direction k: the successor of k is (k + 3) % 4 where that edge exists, else k, else (k + 1) % 4
      int k = (dir + 1) & 3;
      if (!((dir_mask(in, k) >> lane) & 1ull)) k = dir;
      if (!((dir_mask(in, k) >> lane) & 1ull)) k = (dir + 3) & 3;
      int pe;
      if (k == 0) pe = lane ? base + edge_rank(m, lane - 1, 0) : woff[it - 1] + edge_rank(ml, 63, 0);                 // from (x - 1, y)
      else if (k == 2) pe = lane < 63 ? base + edge_rank(m, lane + 1, 2) : woff[it + 1] + edge_rank(mr, 0, 2);        // from (x + 1, y)
      else if (k == 1) pe = woff[it - v.VW64] + edge_rank(mu, lane, 1);                                               // from (x, y - 1)
      else pe = woff[it + v.VW64] + edge_rank(md, lane, 3);                                                           // from (x, y + 1)
      const unsigned id = (unsigned)(((yv * (v.g.W + 1) + jv * 64 + lane) << 2) | dir);
      pred[r] = pe;
      info[r] = id | (k != dir ? 0x80000000u : 0u);
      node[r] = make_int4(pe, r, 0, 0);                   // link, smallest index of the window {r}, steps back to it
      ++r;
    }
  }
}

// ---- one round of pointer jumping: the window of e (2^r edges back from e) joins the window of its link (the next 2^r)
__global__ __launch_bounds__(NT) void contour_jump_kernel(const int4* __restrict__ src, int4* __restrict__ dst, int r, const int* __restrict__ ctl) {
  if (r >= ctl[CT_ROUNDS]) return;
  const size_t n = (size_t)ctl[CT_NE];
  for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < n; e += (size_t)gridDim.x * NT) {
    const int4 a = src[e], b = src[a.x];
    // equal minima are the same edge met again after a full turn: the nearer occurrence stays
    dst[e] = b.y < a.y ? make_int4(b.x, b.y, (1 << r) + b.z, 0) : make_int4(b.x, a.y, a.z, 0);
  }
}

// ---- scatter into contour order; the leader opens its table row
__global__ __launch_bounds__(NT) void contour_scatter_kernel(int P, VGeo v, const int* __restrict__ woff,
                                                             const int* __restrict__ ctl, const int4* __restrict__ na, const int4* __restrict__ nb,
                                                             const int* __restrict__ pred, const unsigned* __restrict__ info,
                                                             const I2* __restrict__ lead, const int* __restrict__ parent, int* __restrict__ order,
                                                             int contour_capacity, int* __restrict__ table) {
  const size_t n = (size_t)ctl[CT_NE];
  const int4* fin = (ctl[CT_ROUNDS] & 1) ? nb : na;
  for (size_t e = (size_t)blockIdx.x * NT + threadIdx.x; e < n; e += (size_t)gridDim.x * NT) {
    const int4 f = fin[e];
    const I2 l = lead[f.y];
    const size_t q = (size_t)l.y + (size_t)f.z;           // base + rank: the cycle lengths sum to the edge count, a permutation of 0 .. n - 1
    if (q < n) order[q] = (int)e;                         // (the bound holds by that argument; the store does not lean on it)
    if (f.y != (int)e || l.x >= contour_capacity) continue;
    int lo = 0, hi = P - 1;                               // the plane: the last one whose first edge is not past e
    while (lo < hi) {
      const int mid = lo + (hi - lo + 1) / 2;
      if (woff[(size_t)mid * v.per_plane()] <= (int)e) lo = mid; else hi = mid - 1;
    }
    const unsigned id = info[e] & 0x7fffffffu;
    const int dir = (int)(id & 3u), vx = (int)((id >> 2) % (unsigned)(v.g.W + 1)), vy = (int)((id >> 2) / (unsigned)(v.g.W + 1));
    // the set pixel on the edge's right.  A leader starts at its cycle's first vertex in raster order, so it runs E (an outer contour: the pixel
    // under it) or S (a hole: the pixel left of it); the other two directions are spelled out so that no index ever depends on that argument
    const int px = (dir == 0 || dir == 3) ? vx : vx - 1, py = dir < 2 ? vy : vy - 1;
    const int* par = parent + (size_t)lo * v.g.HW;
    int* row = table + (size_t)l.x * CF;
    row[F_PLANE] = lo;
    row[F_AREA] = 0;
    row[F_EDGES] = 1 + fin[pred[e]].z;
    row[F_X0] = v.g.W + 1; row[F_Y0] = v.g.H + 1; row[F_X1] = -1; row[F_Y1] = -1;
    row[F_LABEL] = 1 + par[par[py * v.g.W + px]];         // pixel -> run start -> root
  }
}

// ---- vertices, area and box, a thread per position in contour order.  The sums wrap like any int32 sum; the total is below 2^31 in magnitude
__global__ __launch_bounds__(NT) void contour_emit_kernel(VGeo v, const int* __restrict__ ctl, const int4* __restrict__ na, const int4* __restrict__ nb,
                                                          const unsigned* __restrict__ info, const I2* __restrict__ lead,
                                                          const int* __restrict__ order, const int* __restrict__ vpos, int contour_capacity,
                                                          int vertex_capacity, int* __restrict__ table, int* __restrict__ vertices) {
  const size_t n = (size_t)ctl[CT_NE];
  const int4* fin = (ctl[CT_ROUNDS] & 1) ? nb : na;
  for (size_t q = (size_t)blockIdx.x * NT + threadIdx.x; q < n; q += (size_t)gridDim.x * NT) {
    const int e = order[q];
    if ((size_t)(unsigned)e >= n) continue;                // (never: order is a permutation)
    const int4 f = fin[e];
    const int c = lead[f.y].x;
    const unsigned inf = info[e], id = inf & 0x7fffffffu;
    const int dir = (int)(id & 3u), vx = (int)((id >> 2) % (unsigned)(v.g.W + 1)), vy = (int)((id >> 2) / (unsigned)(v.g.W + 1));
    const bool corner = inf >> 31, row_ok = c < contour_capacity;
    int* row = table + (size_t)c * CF;
    if (corner) {
      const int vp = vpos[q];
      if (vp < vertex_capacity) { vertices[2 * (size_t)vp] = vx; vertices[2 * (size_t)vp + 1] = vy; }
      if (row_ok) {                                        // the box of a polygon is the box of its corners
        atomicMin(row + F_X0, vx); atomicMin(row + F_Y0, vy);
        atomicMax(row + F_X1, vx); atomicMax(row + F_Y1, vy);
      }
    }
    if (row_ok && (dir & 1) && vx) atomicAdd(row + F_AREA, dir == 1 ? vx : -vx);
    if (row_ok && f.z == 0) {                              // the leader: its position is the contour's base
      const size_t endq = q + (size_t)row[F_EDGES];       // written by scatter, not touched here
      row[F_FIRST] = vpos[q];
      row[F_NVERT] = (endq < n ? vpos[endq] : ctl[CT_VERT]) - vpos[q];
    }
  }
}

__global__ __launch_bounds__(NT) void contour_finish_kernel(const int* __restrict__ woff, int P, size_t vwp, const int* __restrict__ ctl,
                                                            const I2* __restrict__ lead, int contour_capacity, int vertex_capacity,
                                                            int* __restrict__ ncont, int* __restrict__ overflow) {
  const int n = ctl[CT_NE];
  for (int p = blockIdx.x * NT + threadIdx.x; p < P; p += gridDim.x * NT) {
    int cnt = 0;
    if (n) {
      const int s = woff[(size_t)p * vwp], t = p + 1 < P ? woff[(size_t)(p + 1) * vwp] : n;
      cnt = (t < n ? lead[t].x : ctl[CT_LEAD]) - (s < n ? lead[s].x : ctl[CT_LEAD]);
    }
    ncont[p] = cnt;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && n && (ctl[CT_LEAD] > contour_capacity || ctl[CT_VERT] > vertex_capacity)) *overflow = 1;
}

namespace {

struct Scratch {
  u64* bits;
  int *parent, *woff, *pred, *order, *vpos, *ctl;
  unsigned* info;
  int4 *na, *nb;
  I2 *lead, *partial;
  size_t bytes;
};

inline size_t tiles(size_t n) { return (n + TILE - 1) / TILE; }

Scratch carve(void* base, size_t P, int H, int W, size_t EC) {
  Scratch s;
  const size_t W64 = ((size_t)W + 63) / 64, nvw = P * ((size_t)H + 1) * ((size_t)W / 64 + 1);
  Carver cv(base);
  s.bits = cv.take<u64>(P * H * W64);
  s.parent = cv.take<int>(P * (size_t)H * W);
  s.woff = cv.take<int>(nvw);
  s.pred = cv.take<int>(EC);
  s.info = cv.take<unsigned>(EC);
  s.na = cv.take<int4>(EC);
  s.nb = cv.take<int4>(EC);
  s.lead = cv.take<I2>(EC);
  s.order = cv.take<int>(EC);
  s.vpos = cv.take<int>(EC);
  s.partial = cv.take<I2>(std::max(tiles(nvw), tiles(EC)) + 1);
  s.ctl = cv.take<int>(CT_INTS);
  s.bytes = cv.used;
  return s;
}

template <class In, class Out>
void scan(In in, Out out, const int* nptr, size_t nmax, I2* partial, int* total, hipStream_t st) {
  const unsigned nb = (unsigned)tiles(nmax);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(scan_sums_kernel<In>), dim3(nb), dim3(NT), 0, st, in, nptr, nmax, partial);
  hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(NT), 0, st, partial, (int)nb, total);
  hipLaunchKernelGGL(HIP_KERNEL_NAME(scan_tiles_kernel<In, Out>), dim3(nb), dim3(NT), 0, st, in, out, nptr, nmax, (const I2*)partial);
}

}  // namespace

size_t contours_scratch_bytes(size_t planes, int H, int W, size_t edge_capacity) { return carve(nullptr, planes, H, W, edge_capacity).bytes; }

// rounds the host must launch: 2^rounds >= the most edges a plane of the call can hold (at most four per pixel, at most the capacity)
int contours_rounds(int H, int W, size_t edge_capacity) {
  const unsigned long long most = std::min<unsigned long long>(4ull * (unsigned long long)H * (unsigned long long)W, edge_capacity);
  int r = 0;
  while ((1ull << r) < most) ++r;
  return r;
}

hipError_t launch_stack_contour_counts(const float* stack, int N, int H, int W, int C, long long* counts, hipStream_t st) {
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * C * 2 * sizeof(long long), st);
  if (e != hipSuccess) return e;
  const size_t total = (size_t)N * ((size_t)H + 1) * ((size_t)W / 64 + 1);
  const int vec = (C == 4 && ((uintptr_t)stack & 15) == 0) ? 1 : 0;
  hipLaunchKernelGGL(contour_counts_kernel, dim3(std::min(wave_grid(total), 2048u)), dim3(NT), 0, st, stack, N, H, W, C, vec,
                     (unsigned long long*)counts);
  return hipGetLastError();
}

hipError_t launch_stack_contours(const float* stack, int N, int H, int W, int C, void* scratch, int edge_capacity, int contour_capacity,
                                 int vertex_capacity, int* ncont, int* table, int* vertices, int* overflow, hipStream_t st) {
  const int P = N * C;
  const size_t EC = (size_t)edge_capacity;
  VGeo v{bit_geo(1, H, W), H + 1, W / 64 + 1};
  const BitGeo& g = v.g;
  const Scratch s = carve(scratch, P, H, W, EC);
  const size_t nvw = (size_t)P * v.per_plane();
  launch_bits_pack(stack, N, g, C, C, 1, s.bits, st);
  launch_ccl_init(s.bits, P, g, 0, s.parent, nullptr, nullptr, st);
  launch_ccl_merge(s.bits, P, g, 0, 1, s.parent, st);
  launch_ccl_flatten(s.bits, P, g, 0, s.parent, st);
  scan(WordEdgesIn{s.bits, v}, FirstOut{s.woff}, nullptr, nvw, s.partial, s.ctl + CT_ETOT, st);
  hipLaunchKernelGGL(contour_setup_kernel, dim3(1), dim3(NT), 0, st, s.woff, P, v.per_plane(), edge_capacity, s.ctl, overflow);
  hipLaunchKernelGGL(contour_links_kernel, dim3(wave_grid(nvw)), dim3(NT), 0, st, s.bits, P, v, s.woff, s.ctl, s.pred, s.info, s.na);
  const int rounds = contours_rounds(H, W, EC);
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(contour_jump_kernel, dim3(item_grid(EC)), dim3(NT), 0, st, (r & 1) ? s.nb : s.na, (r & 1) ? s.na : s.nb, r, s.ctl);
  scan(LeaderIn{s.na, s.nb, s.pred, s.ctl}, PairOut{s.lead}, s.ctl + CT_NE, EC, s.partial, s.ctl + CT_LEAD, st);
  hipLaunchKernelGGL(contour_scatter_kernel, dim3(item_grid(EC)), dim3(NT), 0, st, P, v, s.woff, s.ctl, s.na, s.nb, s.pred, s.info, s.lead,
                     s.parent, s.order, contour_capacity, table);
  scan(CornerIn{s.order, s.info, s.ctl}, FirstOut{s.vpos}, s.ctl + CT_NE, EC, s.partial, s.ctl + CT_VERT, st);
  hipLaunchKernelGGL(contour_emit_kernel, dim3(item_grid(EC)), dim3(NT), 0, st, v, s.ctl, s.na, s.nb, s.info, s.lead, s.order, s.vpos,
                     contour_capacity, vertex_capacity, table, vertices);
  hipLaunchKernelGGL(contour_finish_kernel, dim3(item_grid((size_t)P)), dim3(NT), 0, st, s.woff, P, v.per_plane(), s.ctl, s.lead, contour_capacity,
                     vertex_capacity, ncont, overflow);
  return hipGetLastError();
}

}  // namespace octseg
