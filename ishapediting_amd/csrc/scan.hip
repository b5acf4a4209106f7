// Kernels behind csrc/scan.h.  All of it is exact unsigned arithmetic: a result depends on the input alone.
#include "scan.h"

namespace {

__global__ __launch_bounds__(SCAN_THREADS) void scan_blocks_kernel(unsigned* __restrict__ x, long long n, unsigned* __restrict__ totals) {
  __shared__ unsigned lds[16];
  const long long i0 = (long long)blockIdx.x * SCAN_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
  unsigned v[SCAN_ITEMS], sum = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) { v[k] = i0 + k < n ? x[i0 + k] : 0u; sum += v[k]; }
  unsigned total;
  unsigned run = block_exclusive_scan(sum, lds, total);
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    if (i0 + k < n) x[i0 + k] = run;
    run += v[k];
  }
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}
__global__ __launch_bounds__(1024) void scan_totals_kernel(unsigned* __restrict__ sums, long long nb, unsigned* __restrict__ grand) {
  __shared__ unsigned lds[16];
  unsigned carry = 0;
  for (long long b0 = 0; b0 < nb; b0 += 1024) {
    const long long i = b0 + threadIdx.x;
    const unsigned v = i < nb ? sums[i] : 0u;
    unsigned total;
    const unsigned ex = block_exclusive_scan(v, lds, total);
    if (i < nb) sums[i] = carry + ex;
    carry += total;
  }
  if (grand && threadIdx.x == 0) *grand = carry;
}
__global__ __launch_bounds__(SCAN_THREADS) void scan_add_kernel(unsigned* __restrict__ x, long long n, const unsigned* __restrict__ totals) {
  const unsigned add = totals[blockIdx.x];
  const long long i0 = (long long)blockIdx.x * SCAN_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k)
    if (i0 + k < n) x[i0 + k] += add;
}
__global__ __launch_bounds__(256) void corner_degree_kernel(const int* __restrict__ tris, long long ntris, unsigned per_corner,
                                                            unsigned* __restrict__ deg) {
  const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
  if (f >= ntris) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) atomicAdd(deg + tris[3 * f + c], per_corner);
}

}  // namespace

void scan_block_totals(unsigned* sums, long long nb, unsigned* total, hipStream_t s) {
  hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(1024), 0, s, sums, nb, total);
}

void scan_exclusive_u32(unsigned* x, long long n, unsigned* totals, unsigned* grand, hipStream_t s) {
  const long long nb = scan_u32_blocks(n);
  hipLaunchKernelGGL(scan_blocks_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, x, n, totals);
  scan_block_totals(totals, nb, grand, s);
  hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, x, n, (const unsigned*)totals);
}

void count_triangle_corners(const int* tris, long long ntris, unsigned per_corner, unsigned* deg, hipStream_t s) {
  hipLaunchKernelGGL(corner_degree_kernel, dim3((unsigned)((ntris + 255) / 256)), dim3(256), 0, s, tris, ntris, per_corner, deg);
}
