// Part edits: select a part of a decoded volume, spread handles over it, move it rigidly (include/ishap.h: ishap_region_select,
// ishap_region_handles, ishap_region_transform).  Once per edit, nothing here is on the per-step path; what matters is that no
// voxel goes through the host and that every result repeats bit for bit: all arithmetic is integer or double, the only atomics
// are integer adds and 64-bit integer maxima, and floating-point contraction is off so the double expressions round as written.
//
//   select     a thread per voxel: volume - level > 0, and the voxel centre in the union of the primitives (the rules of
//              region_prim_kernel, in 3-D) or set in the grid.  One integer atomicAdd per workgroup counts the set voxels.
//   handles    farthest-point sampling over the set voxels of a mask:
//                1. parts_count_kernel: a wave per run of 64 voxels, a ballot -> the run's count;
//                2. scan_exclusive_u32 over the runs (scan.h): where each run's candidates start, and their number M (device);
//                3. parts_compact_kernel: the same ballot, every set voxel's packed coordinates (10 bits per axis) to its
//                   place -- candidates are in ascending linear index -- and its distance to the picks so far, "infinite";
//                4. one launch per pick over a FIXED grid (M is known to the device only) that strides over the candidates.
//                   A candidate's key is (value << 32) | (0xFFFFFFFF - linear index): the maximum over keys is the largest
//                   value and, among equals, the lowest index.  Wave maximum by shuffles, workgroup maximum through LDS, one
//                   64-bit atomicMax per workgroup into the slot of the round; the next round reads that slot.  Value of round
//                   0: 0x7FFFFFFF - |v - start|^2, or |2 v - (lo + hi)|^2 from the candidates' bounding box (integer atomicMax
//                   per wave); of round r >= 1: min over the picks so far of |v - pick|^2, kept per candidate and lowered by
//                   the latest pick only.  A picked candidate has value 0, so it is not picked again while r < M.
//                5. parts_emit_kernel: slots -> picks and squared distances; rounds beyond M give (-1, -1, -1).
//   transform  a thread per DESTINATION voxel (an inverse map: the moved region has no holes).
#include "../../include/ishap.h"
#include "parts.h"
#include "scan.h"
#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {
constexpr int PT = 256;
typedef unsigned long long u64;

__device__ __forceinline__ double vox_centre(int i, int D) { return 2.0 * (double)i / (double)(D - 1) - 1.0; }

// every thread of the workgroup calls this; one atomicAdd per workgroup that has any
__device__ __forceinline__ void block_count(bool set, int* __restrict__ count) {
  __shared__ int wsum[PT / 64];
  const int n = __popcll(__ballot(set));
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < PT / 64; ++w) t += wsum[w];
    if (t) atomicAdd(count, t);
  }
}

__global__ __launch_bounds__(PT) void region_select_kernel(const float* __restrict__ vol, float level, const RegionPrim* __restrict__ prims,
                                                           int n_prims, const unsigned char* __restrict__ grid, int D,
                                                           unsigned char* __restrict__ out, int* __restrict__ count) {
  const long long idx = (long long)blockIdx.x * PT + threadIdx.x, N = (long long)D * D * D;
  bool set = false;
  if (idx < N) {
    if (vol[idx] - level > 0.f) {                       // the inside rule of the surface and the components (a NaN is outside)
      set = grid && grid[idx] != 0;
      if (!set && n_prims > 0) {
        const int iz = (int)(idx % D), iy = (int)((idx / D) % D), ix = (int)(idx / ((long long)D * D));
        const double x = vox_centre(ix, D), y = vox_centre(iy, D), z = vox_centre(iz, D);
        for (int i = 0; i < n_prims && !set; ++i) {
          const RegionPrim q = prims[i];
          if (q.kind == 0) {
            set = x >= q.a[0] && x <= q.b[0] && y >= q.a[1] && y <= q.b[1] && z >= q.a[2] && z <= q.b[2];
          } else {
            const double dx = x - q.a[0], dy = y - q.a[1], dz = z - q.a[2];
            set = (dx * dx + dy * dy) + dz * dz <= q.b[0] * q.b[0];
          }
        }
      }
    }
    out[idx] = set ? 1 : 0;
  }
  block_count(set, count);
}

__global__ __launch_bounds__(PT) void region_transform_kernel(const unsigned char* __restrict__ src, int D, PartsRigid g,
                                                              unsigned char* __restrict__ out, int* __restrict__ count) {
  const long long idx = (long long)blockIdx.x * PT + threadIdx.x, N = (long long)D * D * D;
  bool set = false;
  if (idx < N) {
    const int iz = (int)(idx % D), iy = (int)((idx / D) % D), ix = (int)(idx / ((long long)D * D));
    const double d0 = vox_centre(ix, D) - g.pivot[0] - g.t[0], d1 = vox_centre(iy, D) - g.pivot[1] - g.t[1],
                 d2 = vox_centre(iz, D) - g.pivot[2] - g.t[2];
    // y = R^T d + pivot: row a of R^T is column a of R
    const double y0 = ((g.R[0] * d0 + g.R[3] * d1) + g.R[6] * d2) + g.pivot[0];
    const double y1 = ((g.R[1] * d0 + g.R[4] * d1) + g.R[7] * d2) + g.pivot[1];
    const double y2 = ((g.R[2] * d0 + g.R[5] * d1) + g.R[8] * d2) + g.pivot[2];
    const double top = (double)(D - 1);
    const double r0 = rint((y0 + 1.0) * top / 2.0), r1 = rint((y1 + 1.0) * top / 2.0), r2 = rint((y2 + 1.0) * top / 2.0);
    if (r0 >= 0.0 && r0 <= top && r1 >= 0.0 && r1 <= top && r2 >= 0.0 && r2 <= top)          // compared as doubles: no wild cast
      set = src[((long long)(int)r0 * D + (int)r1) * D + (int)r2] != 0;
    out[idx] = set ? 1 : 0;
  }
  block_count(set, count);
}

// ---------------------------------------------------------------------------------------------------- farthest-point handles
__device__ __forceinline__ unsigned pack3(int ix, int iy, int iz) { return ((unsigned)ix << 20) | ((unsigned)iy << 10) | (unsigned)iz; }
__device__ __forceinline__ unsigned lin_of(unsigned c, int D) { return ((c >> 20) * (unsigned)D + ((c >> 10) & 1023u)) * (unsigned)D + (c & 1023u); }
__device__ __forceinline__ int dist2(unsigned c, int px, int py, int pz) {
  const int dx = (int)(c >> 20) - px, dy = (int)((c >> 10) & 1023u) - py, dz = (int)(c & 1023u) - pz;
  return dx * dx + dy * dy + dz * dz;                   // at most 3 * 1023^2
}
__device__ __forceinline__ u64 make_key(unsigned value, unsigned lin) { return ((u64)value << 32) | (u64)(0xFFFFFFFFu - lin); }

// runs of 64 voxels, a wave each; the launch covers 4 * ceil(N / 256) runs and cnt has that many words
__global__ __launch_bounds__(PT) void parts_count_kernel(const unsigned char* __restrict__ mask, long long N, unsigned* __restrict__ cnt) {
  const long long idx = (long long)blockIdx.x * PT + threadIdx.x;
  const u64 b = __ballot(idx < N && mask[idx] != 0);
  if ((threadIdx.x & 63) == 0) cnt[idx >> 6] = (unsigned)__popcll(b);
}

__global__ __launch_bounds__(PT) void parts_compact_kernel(const unsigned char* __restrict__ mask, int D, long long N,
                                                           const unsigned* __restrict__ off, unsigned* __restrict__ cand,
                                                           unsigned* __restrict__ mind) {
  const long long idx = (long long)blockIdx.x * PT + threadIdx.x;
  const bool set = idx < N && mask[idx] != 0;
  const u64 b = __ballot(set);
  if (set) {
    const int lane = threadIdx.x & 63;
    const unsigned at = off[idx >> 6] + (unsigned)__popcll(b & ((1ull << lane) - 1ull));      // below M <= N: inside both arrays
    cand[at] = pack3((int)(idx / ((long long)D * D)), (int)((idx / D) % D), (int)(idx % D));
    mind[at] = 0xFFFFFFFFu;
  }
}

// box[a] = max (D - 1 - v_a), box[3 + a] = max v_a over the candidates (box cleared by the caller): one kind of atomic for both ends
__global__ __launch_bounds__(PT) void parts_bbox_kernel(const unsigned* __restrict__ cand, const int* __restrict__ Mp, int D, int* __restrict__ box) {
  const int M = *Mp;
  int m[6] = {-1, -1, -1, -1, -1, -1};
  for (long long i = (long long)blockIdx.x * PT + threadIdx.x; i < M; i += (long long)gridDim.x * PT) {
    const unsigned c = cand[i];
    const int v0 = (int)(c >> 20), v1 = (int)((c >> 10) & 1023u), v2 = (int)(c & 1023u);
    m[0] = max(m[0], D - 1 - v0), m[1] = max(m[1], D - 1 - v1), m[2] = max(m[2], D - 1 - v2);
    m[3] = max(m[3], v0), m[4] = max(m[4], v1), m[5] = max(m[5], v2);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    int v = m[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    if ((threadIdx.x & 63) == 0 && v > 0) atomicMax(box + k, v);
  }
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int d) {
  const unsigned lo = __shfl_xor((unsigned)v, d), hi = __shfl_xor((unsigned)(v >> 32), d);
  return ((u64)hi << 32) | lo;
}

// every thread of the workgroup calls this; key 0 = the thread saw no candidate
__device__ __forceinline__ void block_key_max(u64 key, u64* __restrict__ slot) {
  __shared__ u64 wmax[PT / 64];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 o = shfl_xor_u64(key, d);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 k = wmax[0];
    for (int w = 1; w < PT / 64; ++w) k = wmax[w] > k ? wmax[w] : k;
    if (k) atomicMax(slot, k);
  }
}

// round 0.  use_start: the candidate nearest to (sx, sy, sz); else the one farthest from the centre of the bounding box.
__global__ __launch_bounds__(PT) void parts_first_kernel(const unsigned* __restrict__ cand, const int* __restrict__ Mp, int D, int use_start,
                                                         int sx, int sy, int sz, const int* __restrict__ box, u64* __restrict__ slots) {
  const int M = *Mp;
  int cx = 0, cy = 0, cz = 0;                             // lo + hi per axis
  if (!use_start) cx = (D - 1 - box[0]) + box[3], cy = (D - 1 - box[1]) + box[4], cz = (D - 1 - box[2]) + box[5];
  u64 key = 0;
  for (long long i = (long long)blockIdx.x * PT + threadIdx.x; i < M; i += (long long)gridDim.x * PT) {
    const unsigned c = cand[i];
    unsigned value;
    if (use_start) {
      value = 0x7FFFFFFFu - (unsigned)dist2(c, sx, sy, sz);
    } else {
      const int dx = 2 * (int)(c >> 20) - cx, dy = 2 * (int)((c >> 10) & 1023u) - cy, dz = 2 * (int)(c & 1023u) - cz;
      value = (unsigned)(dx * dx + dy * dy + dz * dz);    // at most 3 * 2046^2
    }
    const u64 k = make_key(value, lin_of(c, D));
    key = k > key ? k : key;
  }
  block_key_max(key, slots);
}

// round r >= 1: lower every candidate's distance by the pick of round r - 1, then the maximum
__global__ __launch_bounds__(PT) void parts_round_kernel(const unsigned* __restrict__ cand, unsigned* __restrict__ mind, const int* __restrict__ Mp,
                                                         int D, int r, u64* __restrict__ slots) {
  const int M = *Mp;
  if (r >= M) return;                                     // the same for every thread: rounds beyond M leave their slot 0
  const unsigned plin = 0xFFFFFFFFu - (unsigned)slots[r - 1];
  const int px = (int)(plin / ((unsigned)D * D)), py = (int)((plin / (unsigned)D) % (unsigned)D), pz = (int)(plin % (unsigned)D);
  u64 key = 0;
  for (long long i = (long long)blockIdx.x * PT + threadIdx.x; i < M; i += (long long)gridDim.x * PT) {
    const unsigned c = cand[i];
    const unsigned m = min(mind[i], (unsigned)dist2(c, px, py, pz));
    mind[i] = m;
    const u64 k = make_key(m, lin_of(c, D));
    key = k > key ? k : key;
  }
  block_key_max(key, slots + r);
}

__global__ void parts_emit_kernel(const u64* __restrict__ slots, const int* __restrict__ Mp, int D, int n, int* __restrict__ picks,
                                  unsigned* __restrict__ d2) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  int x = -1, y = -1, z = -1;
  unsigned d = 0;
  if (r < *Mp) {
    const u64 k = slots[r];
    const unsigned lin = 0xFFFFFFFFu - (unsigned)k;
    x = (int)(lin / ((unsigned)D * D)), y = (int)((lin / (unsigned)D) % (unsigned)D), z = (int)(lin % (unsigned)D);
    if (r > 0) d = (unsigned)(k >> 32);
  }
  picks[3 * r + 0] = x, picks[3 * r + 1] = y, picks[3 * r + 2] = z;
  d2[r] = d;
}

// box and slots, clear_bytes from box on, are cleared at the start of a call
struct HandlesLayout { unsigned *off, *totals, *cand, *mind; int* box; u64* slots; long long runs, clear_bytes, bytes; };
HandlesLayout handles_layout(void* base, int D, int n) {
  Carve c{(char*)base};
  HandlesLayout L;
  const long long N = (long long)D * D * D;
  L.runs = 4 * ((N + PT - 1) / PT);
  L.off = c.take<unsigned>(L.runs);
  L.totals = c.take<unsigned>(scan_u32_blocks(L.runs) + 1);
  const long long box_at = c.total();
  L.box = (int*)c.bytes(256);
  L.slots = c.take<u64>(n);
  L.clear_bytes = c.total() - box_at;
  L.cand = c.take<unsigned>(N);
  L.mind = c.take<unsigned>(N);            // M is known to the device only: room for every voxel
  L.bytes = c.total();
  return L;
}
}  // namespace

extern "C" int ishap_region_select(const float* volume, int D, float level, const ishap_region_prim* prims, int n_prims,
                                   const unsigned char* grid, unsigned char* mask_out, int* count, void* stream) {
  static_assert(sizeof(ishap_region_prim) == sizeof(RegionPrim), "ishap_region_prim layout");
  ISHAP_REQUIRE(D >= 2 && D <= PARTS_MAX_D, "region select: D must be in 2..1024");
  ISHAP_REQUIRE(std::isfinite(level), "region select: level must be finite");
  ISHAP_REQUIRE(n_prims >= 0 && (prims || n_prims == 0), "region select: null primitives");
  ISHAP_REQUIRE(volume && mask_out && count, "region select: null argument");
  hipStream_t s = (hipStream_t)stream;
  const long long N = (long long)D * D * D;
  ISHAP_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int), s));
  hipLaunchKernelGGL(region_select_kernel, dim3((unsigned)((N + PT - 1) / PT)), dim3(PT), 0, s, volume, level, (const RegionPrim*)prims,
                     n_prims, grid, D, mask_out, count);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" long long ishap_region_handles_scratch_bytes(int D, int n) {
  if (D < 2 || D > PARTS_MAX_D || n < 1 || n > PARTS_MAX_HANDLES) return -1;
  return handles_layout(nullptr, D, n).bytes;
}

extern "C" int ishap_region_handles(const unsigned char* mask, int D, int n, const int* start, int* picks_out, unsigned* dist2_out,
                                    int* M_out, void* scratch, long long scratch_bytes, void* stream) {
  ISHAP_REQUIRE(D >= 2 && D <= PARTS_MAX_D, "region handles: D must be in 2..1024");
  ISHAP_REQUIRE(n >= 1 && n <= PARTS_MAX_HANDLES, "region handles: n must be in 1..4096");
  ISHAP_REQUIRE(mask && picks_out && dist2_out && M_out && scratch, "region handles: null argument");
  if (start)
    ISHAP_REQUIRE(start[0] >= 0 && start[0] < D && start[1] >= 0 && start[1] < D && start[2] >= 0 && start[2] < D,
                  "region handles: the start voxel lies outside the grid");
  const HandlesLayout L = handles_layout(scratch, D, n);
  ISHAP_REQUIRE(scratch_bytes >= L.bytes, "region handles: scratch smaller than ishap_region_handles_scratch_bytes(D, n)");
  ISHAP_REQUIRE(((unsigned long long)scratch & 15ull) == 0, "region handles: scratch must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  unsigned *off = L.off, *totals = L.totals, *cand = L.cand, *mind = L.mind;
  int* box = L.box; u64* slots = L.slots;
  const long long N = (long long)D * D * D;
  const unsigned vb = (unsigned)((N + PT - 1) / PT);
  const unsigned gb = (unsigned)std::min<long long>(1024, std::max<long long>(1, (N + 4 * PT - 1) / (4 * PT)));   // the rounds' fixed grid
  ISHAP_CHECK_HIP(hipMemsetAsync(box, 0, (size_t)L.clear_bytes, s));
  hipLaunchKernelGGL(parts_count_kernel, dim3(vb), dim3(PT), 0, s, mask, N, off);
  scan_exclusive_u32(off, L.runs, totals, (unsigned*)M_out, s);              // M <= N <= 2^30: an int holds it
  hipLaunchKernelGGL(parts_compact_kernel, dim3(vb), dim3(PT), 0, s, mask, D, N, (const unsigned*)off, cand, mind);
  if (!start) hipLaunchKernelGGL(parts_bbox_kernel, dim3(gb), dim3(PT), 0, s, (const unsigned*)cand, (const int*)M_out, D, box);
  hipLaunchKernelGGL(parts_first_kernel, dim3(gb), dim3(PT), 0, s, (const unsigned*)cand, (const int*)M_out, D, start ? 1 : 0,
                     start ? start[0] : 0, start ? start[1] : 0, start ? start[2] : 0, (const int*)box, slots);
  for (int r = 1; r < n; ++r)
    hipLaunchKernelGGL(parts_round_kernel, dim3(gb), dim3(PT), 0, s, (const unsigned*)cand, mind, (const int*)M_out, D, r, slots);
  hipLaunchKernelGGL(parts_emit_kernel, dim3((unsigned)((n + PT - 1) / PT)), dim3(PT), 0, s, (const u64*)slots, (const int*)M_out, D, n,
                     picks_out, dist2_out);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_region_transform(const unsigned char* mask, int D, const double* rigid15, unsigned char* mask_out, int* count,
                                      void* stream) {
  ISHAP_REQUIRE(D >= 2 && D <= PARTS_MAX_D, "region transform: D must be in 2..1024");
  ISHAP_REQUIRE(mask && rigid15 && mask_out && count, "region transform: null argument");
  ISHAP_REQUIRE(mask != mask_out, "region transform: the output must not be the input");
  PartsRigid g;
  for (int i = 0; i < 15; ++i) {
    ISHAP_REQUIRE(std::isfinite(rigid15[i]), "region transform: the rotation, pivot and translation must be finite");
    (i < 9 ? g.R[i] : i < 12 ? g.pivot[i - 9] : g.t[i - 12]) = rigid15[i];
  }
  hipStream_t s = (hipStream_t)stream;
  const long long N = (long long)D * D * D;
  ISHAP_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int), s));
  hipLaunchKernelGGL(region_transform_kernel, dim3((unsigned)((N + PT - 1) / PT)), dim3(PT), 0, s, mask, D, g, mask_out, count);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
