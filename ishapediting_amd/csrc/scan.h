// Integer prefix sums shared by the geometry files (csrc/scan.hip): the workgroup scan, the exclusive scan of a u32 array,
// the scan of per-block sums, and the triangle-corner count that opens a CSR build.  Internal: C++ linkage, no C ABI.
#pragma once
#include "common.h"

constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 8, SCAN_BLOCK = SCAN_THREADS * SCAN_ITEMS;   // elements per workgroup of the array scan

// Workgroup exclusive scan of one value per thread (blockDim.x a multiple of 64, at most 1024): a wave-level inclusive scan,
// then the wave totals through the 16 words of `lds16`.  Returns the thread's prefix, leaves the workgroup's sum in `total`;
// ends on a barrier, so `lds16` may be reused at once.
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* lds16, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  unsigned inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) lds16[wave] = inc;
  __syncthreads();
  unsigned base = 0, tot = 0;
  for (int w = 0; w < nw; ++w) {
    const unsigned t = lds16[w];
    if (w < wave) base += t;
    tot += t;
  }
  __syncthreads();
  total = tot;
  return base + inc - v;
}

// workgroups of the array scan = words of `totals` it needs (a scratch layout adds one for a grand total kept behind them)
inline long long scan_u32_blocks(long long n) { return (n + SCAN_BLOCK - 1) / SCAN_BLOCK; }
// x[0, n), n >= 1 <- its exclusive prefix sums, in place, three launches: per-block scan + block totals, scan_block_totals, add-back.
// totals: scan_u32_blocks(n) words of scratch; grand (may be null) receives the sum of all n.  The launches are the caller's
// to check (hipGetLastError), as are the arguments.
void scan_exclusive_u32(unsigned* x, long long n, unsigned* totals, unsigned* grand, hipStream_t s);
// sums[0, nb) <- its exclusive prefix sums, in place, by ONE workgroup of 1024 (a carry runs from each 1024 to the next);
// total (may be null) receives the sum
void scan_block_totals(unsigned* sums, long long nb, unsigned* total, hipStream_t s);
// deg[v] += per_corner for every corner v of each of the ntris >= 1 triangles (deg cleared by the caller)
void count_triangle_corners(const int* tris, long long ntris, unsigned per_corner, unsigned* deg, hipStream_t s);
