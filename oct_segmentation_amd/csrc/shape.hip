// shape.hip -- lumen geometry (no reference counterpart): the raw moments, bounding box and crack perimeter of every mask
// plane as one device reduction, the centroid of a plane as a pixel on the device, and the ray walk of polar.hip from an origin that is DATA.
// measure.hip and polar.hip walk from the frame centre (the A-lines of a catheter-centred frame); a ray from there through a lumen does not
// measure a lumen diameter.  Here the origin is computed on the device and read by the walk on the device: no host round trip in between.
//
// moments_kernel: one streaming pass, shaped like count_kernel (measure.hip).  A workgroup takes MOM_PIX consecutive pixels of one slice, a WAVE
// 64 * MOM_STEPS consecutive ones, a lane one pixel per step (one float4 where the stack has four channels and a 16-byte aligned base, dword
// loads otherwise; other channel counts are taken four channels at a time).  Per channel `v != 0` is a ballot: its population count is M00 and a
// zero ballot skips the channel's arithmetic for the step (wave-uniform).  Sums of x, y (32 bit: 64 steps of values below 2^15) and of x^2, xy,
// y^2 (24-bit multiply-adds into 32 bits over a round of four steps, then 64 bit) and the box are per-lane accumulators, reduced across the wave by shuffles once per tile, across the waves in LDS, and ONE set of
// integer atomics per workgroup and channel goes to mom.  A lane's (x, y) advances by (64 % W, 64 / W) per step: one division per tile.
//   EDGES = 4 * M00 - 2 * (set pixels whose LEFT neighbour is set) - 2 * (set pixels whose UPPER neighbour is set):
// every set pixel has four sides, and a side is not a crack exactly when the neighbour across it is inside the frame and set -- such sides
// come in pairs, one per member, and each pair is counted once at its right / lower member.  The left neighbour is the previous lane: a shift
// of the ballot, bit 63 of the previous step's ballot carried in (polar.hip's run-start idiom), one uniform load in front of the wave's first
// pixel, and the ballot of x == 0 masks the row starts.  The upper neighbour lies W pixels back.  The ballots of a tile are kept in LDS as bit
// planes (8 KB), and after the tile a thread per 64-pixel word ANDs its word with the plane shifted by W: no second pass over the frame.  Only
// the words that begin less than W pixels into the tile look into the previous tile; they load the upper pixel (streamed a moment ago: L2),
// W / MOM_PIX of the loads again, dealt round the four waves.  Loading the upper pixel at EVERY step was measured at 1.52 x count_kernel,
// this form at 0.93 x.  Everything is integer: the results are independent of order and EQUAL the restatement.
//
// origins_kernel: one thread per plane, the rounded centroid in integer arithmetic and whether the plane is set there.
//
// walk_kernel: polar.hip's profile_kernel with step r of degree a at (ox + ray_off[a][r-1][0], oy + ray_off[a][r-1][1]).  The ray's length is no
// longer a table entry: it ends at the first step outside the frame, found per 64-step chunk as the first set bit of the ballot of "outside".
// Only steps inside the frame are gathered, so no table entry is ever followed out of it.  One wave per (slice, degree): where all channels of
// the slice share an origin (wave-uniform, read from origins) ONE gather serves every class as in ray_kernel; otherwise the wave walks once per
// channel.  The next chunk's offsets are loaded before this chunk's gather.
#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace octseg {

namespace {

constexpr int NT = 256, WAVES = NT / 64;
constexpr int MOM_STEPS = 64, MOM_LOADS = 8, MOM_UNROLL = 4;   // steps of a wave, loads in flight, steps per 32-bit round
constexpr int MOM_WAVE_PIX = 64 * MOM_STEPS;                // consecutive pixels of one wave
constexpr int MOM_PIX = WAVES * MOM_WAVE_PIX;               // pixels of a slice one workgroup reduces
constexpr int MOM_WORDS = MOM_PIX / 64;                     // 64-pixel ballots of a tile
static_assert(MOM_WORDS == NT, "the vertical pass gives every thread one word of the tile");
constexpr int GROUP = 4;                                    // channels per pass
constexpr int MAXC = 8;                                     // channels of the walk, as polar.hip
constexpr int ANGLES = 360;
constexpr int FIELDS = 5;
constexpr int MOM_FIELDS = SHAPE_MOMENT_FIELDS;
static_assert(ANGLES % WAVES == 0, "the waves of a workgroup share a slice");
static_assert(MOM_STEPS % MOM_LOADS == 0 && MOM_LOADS % MOM_UNROLL == 0, "whole rounds");
static_assert((long long)MOM_UNROLL * (SHAPE_MAX_EXTENT - 1) * (SHAPE_MAX_EXTENT - 1) < (1ll << 32), "a round's second moments stay in 32 bits");
static_assert((long long)MOM_STEPS * (SHAPE_MAX_EXTENT - 1) < (1ll << 32), "a lane's sums of x and y stay in 32 bits");

typedef unsigned long long u64;
typedef long long i64;

__device__ inline unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ inline u64 wave_sum(u64 v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ inline unsigned wave_umin(unsigned v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}
__device__ inline int wave_smax(int v) {
#pragma unroll
  for (int m = 32; m; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}

}  // namespace

__global__ void moments_init_kernel(i64* __restrict__ mom, size_t planes, int H, int W) {
  const size_t total = planes * MOM_FIELDS;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % MOM_FIELDS);
    mom[i] = k == 6 ? W : k == 8 ? H : (k == 7 || k == 9) ? -1 : 0;
  }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void moments_kernel(const float* __restrict__ stack, int N, int H, int W, int SC, i64* __restrict__ mom) {
  __shared__ u64 part[WAVES][GROUP][MOM_FIELDS];
  __shared__ u64 bits[GROUP][MOM_WORDS];                    // the tile as bit planes: word i holds pixels 64 * i .. 64 * i + 63 of the tile
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned HW = (unsigned)H * (unsigned)W;            // < 2^31
  const unsigned tiles = (HW + MOM_PIX - 1) / MOM_PIX;
  const size_t total = (size_t)N * tiles;
  const unsigned dx = 64u % (unsigned)W, dy = 64u / (unsigned)W;
  for (size_t t = blockIdx.x; t < total; t += gridDim.x) {
    const size_t n = t / tiles;
    const unsigned pw = (unsigned)(t % tiles) * MOM_PIX + wave * MOM_WAVE_PIX;   // < 2^31 + MOM_PIX: the wave's first pixel
    const float* base = stack + n * (size_t)HW * SC;
    for (int cg = 0; cg < SC; cg += GROUP) {                // one pass with four channels, the only pass of the float4 path
      unsigned cnt[GROUP], hp[GROUP], vp[GROUP];            // wave-uniform
      unsigned ylo[GROUP];                                  // wave-uniform too: y does not decrease from lane to lane,
      int yhi[GROUP];                                       // so a step's smallest and largest y sit in its first and last set lane
      unsigned sx[GROUP], sy[GROUP], xlo[GROUP];
      int xhi[GROUP];
      u64 sxx[GROUP], sxy[GROUP], syy[GROUP];
#pragma unroll
      for (int j = 0; j < GROUP; ++j) {
        cnt[j] = hp[j] = vp[j] = sx[j] = sy[j] = 0u;
        xlo[j] = ylo[j] = ~0u;
        xhi[j] = yhi[j] = -1;
        sxx[j] = sxy[j] = syy[j] = 0ull;
      }
      unsigned vpl[GROUP] = {0u, 0u, 0u, 0u};               // per lane: vertical pairs found in the bit planes
      // Upper neighbours.  Most of them lie W pixels back in THIS tile and are read from its bit planes below.  The words that begin less
      // than W pixels into the tile look into the previous tile: those alone load the upper pixel (a row streamed a moment ago, from L2),
      // dealt round the four waves, four words of loads in flight.  Their pairs go to slot 11 of the wave that FOUND them, not the pixels' owner.
      const unsigned tile0 = pw - (unsigned)wave * MOM_WAVE_PIX;
      const int up_words = min((W + 63) / 64, MOM_WORDS);
      for (int i0 = wave; i0 < up_words && tile0 + (unsigned)i0 * 64u < HW; i0 += WAVES * MOM_UNROLL) {   // wave-uniform
        float4 a[MOM_UNROLL], b[MOM_UNROLL];
#pragma unroll
        for (int k = 0; k < MOM_UNROLL; ++k) {
          const unsigned q = min(tile0 + (unsigned)(i0 + k * WAVES) * 64u + lane, HW - 1u);    // past the slice or the words: masked below
          const unsigned qu = q >= (unsigned)W ? q - (unsigned)W : q;
          if (VEC) {
            a[k] = *(const float4*)(base + (size_t)q * 4);
            b[k] = *(const float4*)(base + (size_t)qu * 4);
          } else {
            const float* fa = base + (size_t)q * SC + cg;
            const float* fb = base + (size_t)qu * SC + cg;
            a[k].x = fa[0]; b[k].x = fb[0];
            a[k].y = cg + 1 < SC ? fa[1] : 0.f; b[k].y = cg + 1 < SC ? fb[1] : 0.f;
            a[k].z = cg + 2 < SC ? fa[2] : 0.f; b[k].z = cg + 2 < SC ? fb[2] : 0.f;
            a[k].w = cg + 3 < SC ? fa[3] : 0.f; b[k].w = cg + 3 < SC ? fb[3] : 0.f;
          }
        }
#pragma unroll
        for (int k = 0; k < MOM_UNROLL; ++k) {
          const unsigned pp = tile0 + (unsigned)(i0 + k * WAVES) * 64u + lane;
          const bool ok = i0 + k * WAVES < up_words && pp < HW && pp >= (unsigned)W;   // a word of this pass, inside the slice, not in row 0
          vp[0] += __popcll(__ballot(ok && a[k].x != 0.f && b[k].x != 0.f));
          vp[1] += __popcll(__ballot(ok && a[k].y != 0.f && b[k].y != 0.f));
          vp[2] += __popcll(__ballot(ok && a[k].z != 0.f && b[k].z != 0.f));
          vp[3] += __popcll(__ballot(ok && a[k].w != 0.f && b[k].w != 0.f));
        }
      }
#pragma unroll
      for (int j = 0; j < GROUP; ++j) bits[j][wave * MOM_STEPS + lane] = 0ull;   // steps past the slice's end stay clear
      unsigned carry = 0u;                                  // bit j: channel cg + j is set at the pixel in front of this step's lane 0
      if (pw >= 1u && pw < HW) {                            // wave-uniform; one address for the whole wave
        const float* px = base + (size_t)(pw - 1u) * SC + cg;
#pragma unroll
        for (int j = 0; j < GROUP; ++j)
          if (cg + j < SC && px[j] != 0.f) carry |= 1u << j;
      }
      unsigned p = pw + lane;
      unsigned y = p / (unsigned)W, x = p - y * (unsigned)W;
      for (int s0 = 0; s0 < MOM_STEPS && pw + (unsigned)s0 * 64u < HW; s0 += MOM_LOADS) {    // wave-uniform exit past the slice's end
        // lanes past the slice's end load its last pixel and are masked out of the ballots
        float4 v[MOM_LOADS];
#pragma unroll
        for (int k = 0; k < MOM_LOADS; ++k) {
          const unsigned q = min(p + (unsigned)k * 64u, HW - 1u);
          if (VEC) {
            v[k] = *(const float4*)(base + (size_t)q * 4);
          } else {
            const float* a = base + (size_t)q * SC + cg;
            v[k].x = a[0];
            v[k].y = cg + 1 < SC ? a[1] : 0.f;
            v[k].z = cg + 2 < SC ? a[2] : 0.f;
            v[k].w = cg + 3 < SC ? a[3] : 0.f;
          }
        }
#pragma unroll
        for (int k0 = 0; k0 < MOM_LOADS; k0 += MOM_UNROLL) {
        unsigned axx[GROUP], axy[GROUP], ayy[GROUP];        // the round's second moments: MOM_UNROLL products below 2^30 each fit 32 bits
#pragma unroll
        for (int j = 0; j < GROUP; ++j) axx[j] = axy[j] = ayy[j] = 0u;
#pragma unroll
        for (int k = k0; k < k0 + MOM_UNROLL; ++k) {
          const bool ok = p < HW;
          const u64 row0 = __ballot(x == 0u);               // lanes whose left neighbour is outside the frame
#pragma unroll
          for (int j = 0; j < GROUP; ++j) {
            const float f = j == 0 ? v[k].x : j == 1 ? v[k].y : j == 2 ? v[k].z : v[k].w;
            const bool on = ok && f != 0.f;
            const u64 set = __ballot(on);
            if (set) {                                      // wave-uniform
              cnt[j] += __popcll(set);
              hp[j] += __popcll(set & ((set << 1) | (u64)((carry >> j) & 1u)) & ~row0);
              if (lane == 0) bits[j][wave * MOM_STEPS + s0 + k] = set;
              const unsigned keep = on ? ~0u : 0u;
              const unsigned xm = x & keep, ym = y & keep;
              const unsigned xt = x | ~keep;                // all ones where clear: the largest unsigned, -1 as signed
              sx[j] += xm; sy[j] += ym;
              axx[j] += __umul24(xm, x); axy[j] += __umul24(xm, y); ayy[j] += __umul24(ym, y);   // x, y < 2^15: full-rate 24-bit multiply-adds
              xlo[j] = min(xlo[j], xt);
              xhi[j] = max(xhi[j], (int)xt);
              ylo[j] = min(ylo[j], (unsigned)__builtin_amdgcn_readlane((int)y, __ffsll((long long)set) - 1));
              yhi[j] = max(yhi[j], __builtin_amdgcn_readlane((int)y, 63 - __clzll((long long)set)));
            }
            carry = (carry & ~(1u << j)) | ((unsigned)(set >> 63) << j);
          }
          p += 64u; x += dx; y += dy;
          if (x >= (unsigned)W) { x -= (unsigned)W; ++y; }
        }
#pragma unroll
        for (int j = 0; j < GROUP; ++j) { sxx[j] += axx[j]; sxy[j] += axy[j]; syy[j] += ayy[j]; }
        }
      }
      __syncthreads();                                      // the bit planes of the tile are complete
      {
        const int rel = tid * 64 - W;                       // this thread's word begins W pixels after tile pixel rel
        if (rel >= 0) {                                     // else the loads above counted it from memory
          const int wlo = rel >> 6, sh = rel & 63;          // wlo + 1 <= tid
#pragma unroll
          for (int j = 0; j < GROUP; ++j) {
            const u64 up = sh ? (bits[j][wlo] >> sh) | (bits[j][wlo + 1] << (64 - sh)) : bits[j][wlo];
            vpl[j] = __popcll(bits[j][tid] & up);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < GROUP; ++j) {
        u64 r[MOM_FIELDS];
        if (cnt[j]) {                                       // wave-uniform
          r[0] = cnt[j]; r[1] = wave_sum(sx[j]); r[2] = wave_sum(sy[j]);   // a wave's sums of x and y: 64 lanes * 64 steps * 2^15 < 2^32
          r[3] = wave_sum(sxx[j]); r[4] = wave_sum(sxy[j]); r[5] = wave_sum(syy[j]);
          r[6] = wave_umin(xlo[j]); r[7] = (u64)(i64)wave_smax(xhi[j]);
          r[8] = ylo[j]; r[9] = (u64)(i64)yhi[j];
          r[10] = 4ull * cnt[j] - 2ull * hp[j] - 2ull * wave_sum(vpl[j]);   // >= 0: both kinds of pairs sit at pixels of this wave
        } else {
#pragma unroll
          for (int k = 0; k < MOM_FIELDS; ++k) r[k] = 0ull;
        }
        r[11] = vp[j];                                      // pairs this wave found for the tile's first rows: taken off EDGES below
        if (lane == 0) {
#pragma unroll
          for (int k = 0; k < MOM_FIELDS; ++k) part[wave][j][k] = r[k];
        }
      }
      __syncthreads();
      if (tid < GROUP * MOM_FIELDS) {
        const int j = tid / MOM_FIELDS, k = tid % MOM_FIELDS;
        if (cg + j < SC && k < 11) {
          u64 acc = 0ull;
          bool any = false;
#pragma unroll
          for (int w = 0; w < WAVES; ++w) {
            if (part[w][j][0] == 0ull) continue;            // a wave without a set pixel holds no box
            const u64 val = part[w][j][k];
            if (!any) acc = val;
            else if (k == 6 || k == 8) acc = min(acc, val);
            else if (k == 7 || k == 9) acc = (u64)max((i64)acc, (i64)val);
            else acc += val;
            any = true;
          }
          if (any && k == 10) {                             // the tile's EDGES is >= 0 as a whole
#pragma unroll
            for (int w = 0; w < WAVES; ++w) acc -= 2ull * part[w][j][11];
          }
          if (any) {
            i64* o = mom + (n * SC + cg + j) * (size_t)MOM_FIELDS + k;
            if (k == 6 || k == 8) atomicMin(o, (i64)acc);
            else if (k == 7 || k == 9) atomicMax(o, (i64)acc);
            else if (acc) atomicAdd((u64*)o, acc);
          }
        }
      }
      __syncthreads();   // the next pass of this workgroup overwrites part
    }
  }
}

__global__ void origins_kernel(const float* __restrict__ stack, const i64* __restrict__ mom, int N, int H, int W, int SC, int ref,
                               int* __restrict__ origins) {
  const size_t planes = (size_t)N * SC;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < planes; i += (size_t)gridDim.x * blockDim.x) {
    const size_t n = i / SC;
    const int c = (int)(i % SC);
    const i64* m = mom + (n * SC + (ref < 0 ? c : ref)) * (size_t)MOM_FIELDS;
    int ox = -1, oy = -1, at = 0;
    const i64 m00 = m[0];
    if (m00 > 0) {
      const i64 qx = (2 * m[1] + m00) / (2 * m00), qy = (2 * m[2] + m00) / (2 * m00);
      if (qx >= 0 && qx < W && qy >= 0 && qy < H) {         // moments of this stack always land inside; anything else reads nothing
        ox = (int)qx; oy = (int)qy;
        at = stack[((n * H + (size_t)oy) * W + ox) * SC + c] != 0.f ? 1 : 0;
      }
    }
    origins[i * 3 + 0] = ox; origins[i * 3 + 1] = oy; origins[i * 3 + 2] = at;
  }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void walk_kernel(const float* __restrict__ stack, int N, int H, int W, int SC, const int* __restrict__ origins,
                                                  const int* __restrict__ ray_off, int R, int* __restrict__ prof, int* __restrict__ length) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t total = (size_t)N * (ANGLES / WAVES);
  const int HW = H * W;
  for (size_t t = blockIdx.x; t < total; t += gridDim.x) {
    const size_t n = t / (ANGLES / WAVES);
    const int angle = (int)(t % (ANGLES / WAVES)) * WAVES + wave;
    const int* tab = ray_off + (size_t)angle * R * 2;      // (dx, dy) pairs; two dword loads, no alignment rule
    const float* base = stack + n * (size_t)HW * SC;
    const int* org = origins + n * SC * 3;
    bool shared = true;                                     // wave-uniform: every channel of the slice walks from one pixel
    for (int c = 1; c < SC; ++c) shared = shared && org[c * 3] == org[0] && org[c * 3 + 1] == org[1];
    const int walks = shared ? 1 : SC;
    for (int wk = 0; wk < walks; ++wk) {
      const int c0 = shared ? 0 : wk, c1 = shared ? SC : wk + 1;   // the channels of this walk
      const int ox = org[c0 * 3], oy = org[c0 * 3 + 1];
      const bool inside_frame = ox >= 0 && ox < W && oy >= 0 && oy < H;
      unsigned found = 0u, done = 0u, carry = 0u;           // a bit per class, wave-uniform
      int in_[MAXC], out_[MAXC], last_[MAXC], hits_[MAXC], runs_[MAXC];   // wave-uniform
#pragma unroll
      for (int c = 0; c < MAXC; ++c) in_[c] = out_[c] = last_[c] = hits_[c] = runs_[c] = 0;
      int len = 0;
      if (inside_frame && R > 0) {
        bool ended = false;
        int i_next = min(lane, R - 1) * 2;
        int2 off_next = make_int2(tab[i_next], tab[i_next + 1]);
        for (int r0 = 0; r0 < R && !ended; r0 += 64) {      // lane holds step r0 + lane + 1
          const int2 off = off_next;
          i_next = min(r0 + 64 + lane, R - 1) * 2;          // unconditional and inside the table: nothing waits for it in this chunk
          off_next = make_int2(tab[i_next], tab[i_next + 1]);
          const i64 x = (i64)ox + off.x, y = (i64)oy + off.y;
          const bool in = r0 + lane < R && x >= 0 && x < W && y >= 0 && y < H;
          const u64 outm = ~__ballot(in);                   // the ray ends at its first step outside the frame
          const int first = outm ? __ffsll((long long)outm) - 1 : 64;
          ended = first < 64;
          len = r0 + first;
          const bool valid = lane < first;
          const u64 vmask = __ballot(valid);
          if (!vmask) break;
          const int pix = valid ? (int)y * W + (int)x : 0;  // only steps inside the frame are gathered
          float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
          if (VEC) q = *(const float4*)(base + (size_t)pix * 4);
#pragma unroll
          for (int c = 0; c < MAXC; ++c) {
            if (c >= c0 && c < c1) {                        // wave-uniform
              float f;
              if (VEC) f = c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w;
              else f = base[(size_t)pix * SC + c];
              const u64 set = __ballot(valid && f != 0.f);
              if (set) {
                hits_[c] += __popcll(set);
                runs_[c] += __popcll(set & ~((set << 1) | (u64)((carry >> c) & 1u)));
                last_[c] = r0 + 64 - __clzll((long long)set);
              }
              u64 clear = ~set & vmask;
              bool inside = (found >> c) & 1u;              // the first run began in an earlier chunk
              if (!inside && set) {
                const int f1 = __ffsll((long long)set) - 1; // 0..63
                in_[c] = r0 + f1 + 1;
                found |= 1u << c;
                clear &= f1 == 63 ? 0ull : (~0ull << (f1 + 1));
                inside = true;
              }
              if (inside && !((done >> c) & 1u) && clear) { // step g = r0 + lane_g + 1 is clear: OUT = g - 1
                out_[c] = r0 + __ffsll((long long)clear) - 1;
                done |= 1u << c;
              }
              carry = (carry & ~(1u << c)) | ((unsigned)(set >> 63) << c);   // only a full chunk has a successor
            }
          }
        }
      }
      int res[FIELDS] = {0, 0, 0, 0, 0};                    // lane c: the profile of class c
#pragma unroll
      for (int c = 0; c < MAXC; ++c) {
        if (lane == c) {
          res[0] = in_[c];
          res[1] = ((found & ~done) >> c) & 1u ? len : out_[c];   // the first run reaches the end of the ray
          res[2] = last_[c]; res[3] = hits_[c]; res[4] = runs_[c];
        }
      }
      if (lane >= c0 && lane < c1) {
        int* o = prof + ((n * SC + lane) * ANGLES + angle) * (size_t)FIELDS;
#pragma unroll
        for (int k = 0; k < FIELDS; ++k) o[k] = res[k];
        length[(n * SC + lane) * ANGLES + angle] = len;
      }
    }
  }
}

hipError_t launch_stack_moments(const float* stack, int N, int H, int W, int SC, long long* mom, hipStream_t st) {
  const size_t planes = (size_t)N * SC;
  const dim3 gi((unsigned)std::min<size_t>((planes * MOM_FIELDS + NT - 1) / NT, 1u << 16));
  hipLaunchKernelGGL(moments_init_kernel, gi, dim3(NT), 0, st, mom, planes, H, W);
  const bool vec = SC == 4 && ((uintptr_t)stack & 15) == 0;
  const size_t tiles = (size_t)N * (((size_t)H * W + MOM_PIX - 1) / MOM_PIX);
  const dim3 g((unsigned)std::min<size_t>(tiles, 1u << 20));
  if (vec) hipLaunchKernelGGL(moments_kernel<true>, g, dim3(NT), 0, st, stack, N, H, W, SC, mom);
  else hipLaunchKernelGGL(moments_kernel<false>, g, dim3(NT), 0, st, stack, N, H, W, SC, mom);
  return hipGetLastError();
}

hipError_t launch_moment_origins(const float* stack, const long long* mom, int N, int H, int W, int SC, int ref_channel, int* origins,
                                 hipStream_t st) {
  const size_t planes = (size_t)N * SC;
  const dim3 g((unsigned)std::min<size_t>((planes + NT - 1) / NT, 1u << 16));
  hipLaunchKernelGGL(origins_kernel, g, dim3(NT), 0, st, stack, mom, N, H, W, SC, ref_channel, origins);
  return hipGetLastError();
}

hipError_t launch_stack_polar_at(const float* stack, int N, int H, int W, int SC, const int* origins, const int* ray_off, int R, int* prof,
                                 int* length, hipStream_t st) {
  const bool vec = SC == 4 && ((uintptr_t)stack & 15) == 0;
  const dim3 g((unsigned)std::min<size_t>((size_t)N * (ANGLES / WAVES), 1u << 20));
  if (vec) hipLaunchKernelGGL(walk_kernel<true>, g, dim3(NT), 0, st, stack, N, H, W, SC, origins, ray_off, R, prof, length);
  else hipLaunchKernelGGL(walk_kernel<false>, g, dim3(NT), 0, st, stack, N, H, W, SC, origins, ray_off, R, prof, length);
  return hipGetLastError();
}

}  // namespace octseg
