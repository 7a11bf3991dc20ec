// unionfind.h -- the row-word helpers and the label-equivalence union-find shared by components.hip (planes) and lesions.hip (volumes).
// `par` holds indices into itself (pixel indices of a plane, voxel indices of a volume); the termination argument stands at the top of both files.
#pragma once

#include "common.h"

namespace octseg {

namespace {

typedef unsigned long long u64;

// the bits of word j that lie inside the frame (j < W64, so at least one)
__device__ __forceinline__ u64 inmask(int j, int W) {
  const int n = W - j * 64;
  return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}
__device__ __forceinline__ int ctz64(u64 v) { return __ffsll((long long)v) - 1; }            // v != 0
// length of the run of set bits that starts at bit s (bit s is set)
__device__ __forceinline__ int runlen(u64 c, int s) {
  const u64 z = ~(c >> s);                       // s > 0 shifts zeros in at the top, so z != 0 then
  return (s == 0 && z == 0ull) ? 64 : min(ctz64(z), 64 - s);
}
__device__ __forceinline__ u64 runmask(int s, int len) { return (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << s; }

// walks strictly downwards (parent[x] < x for a non-root): at most H * W steps
__device__ __forceinline__ int find_root(const int* par, int x) {
  for (;;) {
    const int q = __hip_atomic_load(par + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (q == x) return x;
    x = q;
  }
}
// Label-equivalence union.  Every round either links a root (return) or continues with a pair that is strictly smaller in its larger member:
// labels only ever decrease, so the loop ends.
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
