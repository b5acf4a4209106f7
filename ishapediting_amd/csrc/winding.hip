// Generalized winding number: inside / outside for open, doubled or badly closed triangle meshes (Jacobson et al. 2013)
// and for oriented point clouds (Barill et al. 2018), plus the per-point areas the cloud form needs.
//   mesh   w(q) = 1/(4 pi) sum_f Omega_f(q),  Omega = 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)
//          (van Oosterom-Strackee; a, b, c = the corners minus q); +1 inside a mesh that is counter-clockwise seen from outside
//   cloud  w(q) = 1/(4 pi) sum_i a_i (p_i - q).n_i / r^3,  r^2 = max(|p_i - q|^2, a_i / (2 pi)): one sample's share stays
//          below 1/2, the limit of a disc seen from its own surface
//   areas  a_i = pi d_k(i)^2 / k, d_k = distance to the k-th nearest OTHER point (by index: equal points are neighbours)
// All three are brute force over (query, primitive) pairs, laid out as occupancy_kernel (surface.hip): a lane owns a query,
// the primitives go through LDS in tiles of WN_TILE, and every lane reads the same LDS word at the same time (a broadcast).
// A primitive is staged as float4 rows that hold only what does not depend on the query: a triangle's normal
// (B - A) x (C - A) replaces b x c in the numerator (a.(b x c) = a.((b - a) x (c - a))), which costs less per pair and does
// not cancel for a small triangle seen from far away.
// Few queries against many primitives would leave most of the chip idle, so the primitive range is cut into `parts`
// (grid.y); a part writes its sums to scratch and a second launch adds them IN PART ORDER.  No float atomics: the split
// depends on (nprims, npts) alone, so a call repeats bit for bit and a query's value does not depend on its position.
#include "winding.h"

namespace {

constexpr int WN_THREADS = 256;
constexpr int WN_TILE = 256;            // primitives per LDS tile: 12 KB (triangles) / 8 KB (samples) of the CU's 160 KB
constexpr int WN_TARGET_BLOCKS = 1024;  // workgroups wanted before the primitive range stops being cut: 4 per CU of 256
constexpr int WN_MAX_PARTS = 64;
constexpr float WN_INV_4PI = 0.07957747154594767f;
constexpr float WN_INV_2PI = 0.15915494309189535f;
constexpr float WN_PI = 3.14159265358979324f;
constexpr float WN_AREA_FLOOR = 1e-12f;   // keeps r^2 = a / (2 pi) a positive normal float

struct WnSplit { int parts; int tiles_per_part; };

WnSplit wn_split(long long nprims, long long npts) {
  const long long ntiles = (nprims + WN_TILE - 1) / WN_TILE;
  const long long qblocks = (npts + WN_THREADS - 1) / WN_THREADS;
  long long parts = (WN_TARGET_BLOCKS + qblocks - 1) / qblocks;
  if (parts > ntiles) parts = ntiles;
  if (parts > WN_MAX_PARTS) parts = WN_MAX_PARTS;
  if (parts < 1) parts = 1;
  const long long tpp = (ntiles + parts - 1) / parts;
  parts = (ntiles + tpp - 1) / tpp;       // no empty part
  return {(int)parts, (int)tpp};
}

// compensated running sum: the rounding of a long sum stays at one ulp of the total
struct KahanSum {
  float sum = 0.f, comp = 0.f;
  __device__ __forceinline__ void add(float x) {
    const float y = x - comp;
    const float t = sum + y;
    comp = (t - sum) - y;
    sum = t;
  }
};

// binary 0: w itself; +1: inside flag of a counter-clockwise mesh (w > 0.5); -1: of a clockwise one (w < -0.5)
__device__ __forceinline__ float wn_value(float w, int binary) {
  if (binary == 0) return w;
  return (binary > 0 ? w : -w) > 0.5f ? 1.f : 0.f;
}

__device__ __forceinline__ void wn_store(float sum, long long i, long long np, float scale, int binary, float* __restrict__ out) {
  if (gridDim.y > 1) { out[(long long)blockIdx.y * np + i] = sum; return; }
  out[i] = wn_value(sum * scale, binary);
}

// out: w [np] when gridDim.y == 1, else the part sums [gridDim.y][np]
__global__ __launch_bounds__(WN_THREADS) void winding_mesh_kernel(const float* __restrict__ v, const int* __restrict__ t, long long nt,
                                                                  int tiles_per_part, const float* __restrict__ pts, long long np,
                                                                  int binary, float* __restrict__ out) {
  __shared__ float4 tri[WN_TILE][3];      // A.xyz B.x | B.yz C.xy | C.z n.xyz
  const long long i = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (i < np) { px = pts[3 * i]; py = pts[3 * i + 1]; pz = pts[3 * i + 2]; }
  const long long f_begin = (long long)blockIdx.y * tiles_per_part * WN_TILE;
  const long long f_end = min(nt, f_begin + (long long)tiles_per_part * WN_TILE);
  KahanSum acc;
  for (long long f0 = f_begin; f0 < f_end; f0 += WN_TILE) {
    const int m = (int)min((long long)WN_TILE, f_end - f0);
    __syncthreads();
    if ((int)threadIdx.x < m) {
      const long long f = f0 + threadIdx.x;
      const float* A = v + 3LL * t[3 * f];
      const float* B = v + 3LL * t[3 * f + 1];
      const float* Cv = v + 3LL * t[3 * f + 2];
      const float Ax = A[0], Ay = A[1], Az = A[2], Bx = B[0], By = B[1], Bz = B[2], Cx = Cv[0], Cy = Cv[1], Cz = Cv[2];
      const float ux = Bx - Ax, uy = By - Ay, uz = Bz - Az, wx = Cx - Ax, wy = Cy - Ay, wz = Cz - Az;
      // products rounded one by one (no fused multiply-add): equal factors cancel exactly, a repeated corner gives n = 0
      // (B == C: u == w and every difference is x - x; A == B or A == C: a zero factor in every product)
      const float nx = __fmul_rn(uy, wz) - __fmul_rn(uz, wy), ny = __fmul_rn(uz, wx) - __fmul_rn(ux, wz);
      const float nz = __fmul_rn(ux, wy) - __fmul_rn(uy, wx);
      tri[threadIdx.x][0] = make_float4(Ax, Ay, Az, Bx);
      tri[threadIdx.x][1] = make_float4(By, Bz, Cx, Cy);
      tri[threadIdx.x][2] = make_float4(Cz, nx, ny, nz);
    }
    __syncthreads();
#pragma unroll 2
    for (int k = 0; k < m; ++k) {
      const float4 r0 = tri[k][0], r1 = tri[k][1], r2 = tri[k][2];
      const float ax = r0.x - px, ay = r0.y - py, az = r0.z - pz;
      const float bx = r0.w - px, by = r1.x - py, bz = r1.y - pz;
      const float cx = r1.z - px, cy = r1.w - py, cz = r2.x - pz;
      const float la = sqrtf(ax * ax + ay * ay + az * az), lb = sqrtf(bx * bx + by * by + bz * bz);
      const float lc = sqrtf(cx * cx + cy * cy + cz * cz);
      const float det = ax * r2.y + ay * r2.z + az * r2.w;
      const float den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la +
                        (cx * ax + cy * ay + cz * az) * lb;
      // det == 0: a triangle without area, or a query in the triangle's plane -- no solid angle (and no atan2(0, den < 0) = pi)
      acc.add(det == 0.f ? 0.f : 2.f * atan2f(det, den));
    }
  }
  if (i < np) wn_store(acc.sum, i, np, WN_INV_4PI, binary, out);
}

__global__ __launch_bounds__(WN_THREADS) void winding_cloud_kernel(const float* __restrict__ p, const float* __restrict__ n,
                                                                   const float* __restrict__ area, long long npoints,
                                                                   int tiles_per_part, const float* __restrict__ pts, long long np,
                                                                   float* __restrict__ out) {
  __shared__ float4 smp[WN_TILE][2];      // p.xyz, r^2 floor | a n.xyz
  const long long i = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (i < np) { qx = pts[3 * i]; qy = pts[3 * i + 1]; qz = pts[3 * i + 2]; }
  const long long j_begin = (long long)blockIdx.y * tiles_per_part * WN_TILE;
  const long long j_end = min(npoints, j_begin + (long long)tiles_per_part * WN_TILE);
  KahanSum acc;
  for (long long j0 = j_begin; j0 < j_end; j0 += WN_TILE) {
    const int m = (int)min((long long)WN_TILE, j_end - j0);
    __syncthreads();
    if ((int)threadIdx.x < m) {
      const long long j = j0 + threadIdx.x;
      const float a = area[j];
      smp[threadIdx.x][0] = make_float4(p[3 * j], p[3 * j + 1], p[3 * j + 2], a * WN_INV_2PI);
      smp[threadIdx.x][1] = make_float4(a * n[3 * j], a * n[3 * j + 1], a * n[3 * j + 2], 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < m; ++k) {
      const float4 s0 = smp[k][0], s1 = smp[k][1];
      const float dx = s0.x - qx, dy = s0.y - qy, dz = s0.z - qz;
      const float r2 = fmaxf(dx * dx + dy * dy + dz * dz, s0.w);
      const float num = dx * s1.x + dy * s1.y + dz * s1.z;
      acc.add(r2 > 0.f ? num / (r2 * sqrtf(r2)) : 0.f);       // r2 = 0 only for a sample of area 0 at the query itself
    }
  }
  if (i < np) wn_store(acc.sum, i, np, WN_INV_4PI, 0, out);
}

// out[i] = scale * (part[0][i] + part[1][i] + ...), added in part order
__global__ __launch_bounds__(WN_THREADS) void winding_reduce_kernel(const float* __restrict__ part, int parts, long long np, float scale,
                                                                    int binary, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
  if (i >= np) return;
  float s = part[i];
  for (int k = 1; k < parts; ++k) s += part[(long long)k * np + i];
  out[i] = wn_value(s * scale, binary);
}

// The K smallest squared distances of a lane's point to the other points, ascending, in registers: a candidate bubbles
// through the list by min / max (every index a compile-time constant: no private memory).
template <int K>
__global__ __launch_bounds__(WN_THREADS) void cloud_areas_kernel(const float* __restrict__ p, long long n, int k_use,
                                                                 float* __restrict__ area) {
  __shared__ float4 tile[WN_TILE];
  const long long i = (long long)blockIdx.x * WN_THREADS + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (i < n) { px = p[3 * i]; py = p[3 * i + 1]; pz = p[3 * i + 2]; }
  float best[K];
#pragma unroll
  for (int c = 0; c < K; ++c) best[c] = 3.0e38f;
  for (long long j0 = 0; j0 < n; j0 += WN_TILE) {
    const int m = (int)min((long long)WN_TILE, n - j0);
    __syncthreads();
    if ((int)threadIdx.x < m) {
      const long long j = j0 + threadIdx.x;
      tile[threadIdx.x] = make_float4(p[3 * j], p[3 * j + 1], p[3 * j + 2], 0.f);
    }
    __syncthreads();
    const long long self = i - j0;        // the lane's own point, if it is in this tile
    for (int k = 0; k < m; ++k) {
      const float4 s = tile[k];
      const float dx = s.x - px, dy = s.y - py, dz = s.z - pz;
      float d2 = dx * dx + dy * dy + dz * dz;
      if (k == self || !(d2 < best[K - 1])) continue;
#pragma unroll
      for (int c = 0; c < K; ++c) {
        const float lo = fminf(d2, best[c]);
        d2 = fmaxf(d2, best[c]);
        best[c] = lo;
      }
    }
  }
  if (i >= n) return;
  float dk = best[0];
#pragma unroll
  for (int c = 1; c < K; ++c) dk = (c == k_use - 1) ? best[c] : dk;
  area[i] = fmaxf(WN_PI * dk / (float)k_use, WN_AREA_FLOOR);
}

}  // namespace

long long ishap_winding_bytes(long long nprims, long long npts) {
  if (nprims < 0 || npts < 0) return -1;
  if (nprims == 0 || npts == 0) return 256;
  const WnSplit sp = wn_split(nprims, npts);
  const long long b = sp.parts > 1 ? (long long)sp.parts * npts * (long long)sizeof(float) : 0;
  return align_up(b, 256) + 256;
}

void ishap_winding_launch_mesh(const float* verts, const int* tris, long long ntris, const float* pts, long long npts, float* out,
                               int binary, void* scratch, hipStream_t s) {
  const WnSplit sp = wn_split(ntris, npts);
  const unsigned qblocks = (unsigned)((npts + WN_THREADS - 1) / WN_THREADS);
  float* dst = sp.parts > 1 ? (float*)scratch : out;
  hipLaunchKernelGGL(winding_mesh_kernel, dim3(qblocks, (unsigned)sp.parts), dim3(WN_THREADS), 0, s, verts, tris, ntris,
                     sp.tiles_per_part, pts, npts, binary, dst);
  if (sp.parts > 1)
    hipLaunchKernelGGL(winding_reduce_kernel, dim3(qblocks), dim3(WN_THREADS), 0, s, (const float*)scratch, sp.parts, npts, WN_INV_4PI,
                       binary, out);
}

extern "C" long long ishap_winding_scratch_bytes(long long nprims, long long npts) { return ishap_winding_bytes(nprims, npts); }

extern "C" int ishap_mesh_winding(const float* verts, const int* tris, long long ntris, const float* pts, long long npts, float* w,
                                  void* scratch, long long scratch_bytes, void* stream) {
  ISHAP_REQUIRE(verts && tris && pts && w && scratch && ntris > 0 && npts > 0, "mesh_winding arguments");
  ISHAP_REQUIRE(ntris < (1ll << 31) && npts < (1ll << 31) * WN_THREADS, "mesh_winding: triangle and query counts");
  ISHAP_REQUIRE(scratch_bytes >= ishap_winding_bytes(ntris, npts),
                "mesh_winding: scratch smaller than ishap_winding_scratch_bytes(ntris, npts)");
  ishap_winding_launch_mesh(verts, tris, ntris, pts, npts, w, 0, scratch, (hipStream_t)stream);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_cloud_winding(const float* points, const float* normals, const float* areas, long long npoints, const float* pts,
                                   long long npts, float* w, void* scratch, long long scratch_bytes, void* stream) {
  ISHAP_REQUIRE(points && normals && areas && pts && w && scratch && npoints > 0 && npts > 0, "cloud_winding arguments");
  ISHAP_REQUIRE(npoints < (1ll << 31) && npts < (1ll << 31) * WN_THREADS, "cloud_winding: point and query counts");
  ISHAP_REQUIRE(scratch_bytes >= ishap_winding_bytes(npoints, npts),
                "cloud_winding: scratch smaller than ishap_winding_scratch_bytes(npoints, npts)");
  hipStream_t s = (hipStream_t)stream;
  const WnSplit sp = wn_split(npoints, npts);
  const unsigned qblocks = (unsigned)((npts + WN_THREADS - 1) / WN_THREADS);
  float* dst = sp.parts > 1 ? (float*)scratch : w;
  hipLaunchKernelGGL(winding_cloud_kernel, dim3(qblocks, (unsigned)sp.parts), dim3(WN_THREADS), 0, s, points, normals, areas, npoints,
                     sp.tiles_per_part, pts, npts, dst);
  if (sp.parts > 1)
    hipLaunchKernelGGL(winding_reduce_kernel, dim3(qblocks), dim3(WN_THREADS), 0, s, (const float*)scratch, sp.parts, npts, WN_INV_4PI,
                       0, w);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_cloud_areas(const float* points, long long npoints, int k, float* areas, void* stream) {
  ISHAP_REQUIRE(points && areas && npoints > 0, "cloud_areas arguments");
  ISHAP_REQUIRE(k >= 1 && k <= 16 && k < npoints, "cloud_areas: 1 <= k <= 16 and k < npoints (the k-th nearest OTHER point)");
  ISHAP_REQUIRE(npoints < (1ll << 31) * WN_THREADS, "cloud_areas: point count");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((npoints + WN_THREADS - 1) / WN_THREADS)), block(WN_THREADS);
  if (k <= 4) hipLaunchKernelGGL(cloud_areas_kernel<4>, grid, block, 0, s, points, npoints, k, areas);
  else if (k <= 8) hipLaunchKernelGGL(cloud_areas_kernel<8>, grid, block, 0, s, points, npoints, k, areas);
  else hipLaunchKernelGGL(cloud_areas_kernel<16>, grid, block, 0, s, points, npoints, k, areas);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
