// vote.hip -- one mask voted by M member networks (folds x flipped / rotated views), with the map of where they disagree (no reference
// counterpart: the reference trains five folds per class and serves one).  One launch per (batch of frames, output class).
//
// A member is a logits tensor f32 NCHW [N][classes_m][H][W] in the coordinates of ITS view of the frame, a channel ch_m and a view code
// v = a + 2 b + 4 t in 0..7: the view of X[H][W] is transpose if t (square frames only), then reverse the rows if b, then reverse the columns
// if a -- the dihedral group D4.  The kernel undoes the view while it reads: for the source pixel (sy, sx) of the un-viewed frame,
//   (p, q) = t ? (sx, sy) : (sy, sx), (Ht, Wt) = t ? (W, H) : (H, W), the member is read at (b ? Ht - 1 - p : p, a ? Wt - 1 - q : q), rows of Wt.
// (sy, sx) comes from octseg_mask_assemble's resize rule (row / column tables, null = floor((i + 0.5) * S / O), clamped here).
//
// Per output pixel, s_m = sigmoid_acc(z_m): votes = #{s_m > 0.5}, pbar = (s_0 + ... + s_{M-1}) / M in f32 in member order; the mask is
// pbar > 0.5 (soft) or 2 votes > M (majority, a tie is not set); dissent = the number of members whose own threshold differs from the mask.
// With M = 1 and view 0 the mask is octseg_mask_assemble's bit for bit (s / 1.0f is exact).
//
// Form: 256 threads = a 16 x 16 tile of output pixels of one frame, x fastest, so that a wave covers 4 x 16 pixels and a transposed member is
// read along 4-byte strides of 16 rows, not of 64; one pixel per thread at a time, ROWS = 8 tiles below each other per workgroup.  The member
// table (pointers and three ints each) is the kernel argument itself: wave-uniform loads, no table upload.  The four per-frame counts are
// integers: ballots (and a per-lane sum, shuffled once at the end) per wave, LDS across the four waves, one atomicAdd per workgroup and column
// into the frame's row, which the launcher cleared on the stream -- exact and independent of the order.  With one tile per workgroup those
// atomics -- 63 x 63 x 16 workgroups on 64 addresses at 16 frames of 1000 x 1000 -- took 0.3 ms, more than the rest of the launch up to
// M = 8; eight tiles per workgroup is what cut them.
#include "common.h"
#include "kernels.h"
#include "sigmoid.h"

namespace octseg {

namespace {
constexpr int TILE = 16, NT = TILE * TILE, WAVES = NT / 64;
constexpr int ROWS = 8;   // tiles below each other that one workgroup takes, one after the other
}

__global__ __launch_bounds__(NT) void vote_assemble_kernel(const VoteArgs a) {
  __shared__ int part[WAVES][4];
  const int tid = threadIdx.x;
  const int x = blockIdx.x * TILE + (tid & (TILE - 1));
  const int n = blockIdx.z;
  // lanes outside the frame take its last pixel and write nothing: the loads below stay unconditional and in bounds
  const int xc = min(x, a.OW - 1);
  int sx = a.cols ? a.cols[xc] : (int)(((long long)(2 * xc + 1) * a.W) / (2 * a.OW));
  sx = min(max(sx, 0), a.W - 1);
  const size_t plane = (size_t)a.H * a.W;      // a transposed member has the same plane: t needs H == W
  int c0 = 0, c1 = 0, c2 = 0, dsum = 0;        // c0..c2 wave-uniform (ballots), dsum per lane until the end
  for (int k = 0; k < ROWS; ++k) {
    const int y0 = (blockIdx.y * ROWS + k) * TILE;
    if (y0 >= a.OH) break;                     // (uniform)
    const int y = y0 + (tid >> 4);
    const bool ok = x < a.OW && y < a.OH;
    const int yc = min(y, a.OH - 1);
    int sy = a.rows ? a.rows[yc] : (int)(((long long)(2 * yc + 1) * a.H) / (2 * a.OH));
    sy = min(max(sy, 0), a.H - 1);
    float sum = 0.f;
    int votes = 0;
    for (int m = 0; m < a.M; ++m) {
      const int v = a.view[m];
      const bool t = v & 4;
      const int p = t ? sx : sy, q = t ? sy : sx;
      const int Ht = t ? a.W : a.H, Wt = t ? a.H : a.W;
      const int r = (v & 2) ? Ht - 1 - p : p, c = (v & 1) ? Wt - 1 - q : q;
      const float s = sigmoid_acc(a.z[m][((size_t)n * a.classes[m] + a.ch[m]) * plane + (size_t)r * Wt + c]);
      sum += s;
      votes += s > 0.5f ? 1 : 0;
    }
    const float pbar = sum / (float)a.M;
    const bool set = a.mode ? 2 * votes > a.M : pbar > 0.5f;
    const int dis = set ? a.M - votes : votes;
    if (ok) {
      const size_t o = (((size_t)n * a.OH + y) * a.OW + x) * a.OC + a.out_ch;
      a.out[o] = set ? 1.f : 0.f;
      if (a.prob) a.prob[o] = pbar;
      if (a.dissent) a.dissent[o] = (uint8_t)dis;
    }
    if (a.stats) {   // (uniform)
      const bool disputed = votes > 0 && votes < a.M;
      c0 += __popcll(__ballot(ok && set));
      c1 += __popcll(__ballot(ok && disputed));
      c2 += __popcll(__ballot(ok && disputed && set));
      dsum += ok ? dis : 0;
    }
  }
  if (!a.stats) return;   // (uniform)
  for (int off = 32; off > 0; off >>= 1) dsum += __shfl_down(dsum, off, 64);
  if ((tid & 63) == 0) {
    int* w = part[tid >> 6];
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = dsum;
  }
  __syncthreads();
  if (tid < 4) {
    int s = 0;
    for (int w = 0; w < WAVES; ++w) s += part[w][tid];
    if (s) atomicAdd(a.stats + (size_t)n * 4 + tid, s);
  }
}

hipError_t launch_vote_assemble(const VoteArgs& a, hipStream_t st) {
  if (a.stats) {
    const hipError_t e = hipMemsetAsync(a.stats, 0, (size_t)a.N * 4 * sizeof(int), st);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((a.OW + TILE - 1) / TILE, (a.OH + TILE * ROWS - 1) / (TILE * ROWS), a.N);
  hipLaunchKernelGGL(vote_assemble_kernel, grid, dim3(NT), 0, st, a);
  return hipGetLastError();
}

}  // namespace octseg
