// Front end for point clouds that come without normals: k nearest neighbours, PCA normals, consistent orientation.
//   knn      idx[i][0..k), d2[i][0..k) = the k nearest OTHER points of point i, ascending by (squared distance, index):
//            equal distances go to the smaller index, points equal to point i are neighbours at distance 0
//   normals  C_i = sum_{q in N_i} (q - m)(q - m)^T over N_i = {p_i} + its k neighbours, m their mean, every q taken relative
//            to p_i before any product (nothing cancels), in fp64; n_i = unit eigenvector of the smallest eigenvalue, signed so
//            that its component of largest magnitude is positive (ties: the lowest axis); variation = l0 / (l0 + l1 + l2)
//   orient   rounds over the directed kNN graph.  Round r: every point without a level looks at its OWN neighbours whose
//            level is in [1, r), takes the one with the largest |n_i . n_j| (ties: first in neighbour order), flips n_i where
//            that dot is negative and takes level r.  A round that orients nothing while points remain makes the remaining
//            point with the largest z (ties: smallest index) a seed of level r, flipped so that n_z >= 0.
// Layout of knn as cloud_areas_kernel (winding.hip): a lane owns a query, the candidates go through LDS in tiles of 256 and
// every lane reads the same LDS word at the same time.  An entry of the list is ONE 64-bit key, the float bits of d^2 in the
// high word and the index in the low word: non-negative floats order like their bits, so the (distance, index) order is the
// unsigned order of the keys and a candidate bubbles through the sorted list by unsigned min / max, every list index a
// compile-time constant (no private memory).  The candidate range is NOT split over workgroups: N / 256 workgroups fill the
// chip from about 65 000 points on, the sizes cloud_to_mesh is documented for; a small cloud leaves most of it idle and is
// done in well under a millisecond anyway.
// The level of a point, not a done flag, is what makes one normals buffer race-free: in round r a thread reads the normals
// of points with 1 <= level < r only, which nobody writes in round r, and writes its own; a level it reads is 0, r (both: not
// a parent) or final.  Nothing depends on the order in which threads run, so a call repeats bit for bit.
#include "common.h"

namespace {

constexpr int NR_THREADS = 256;
constexpr int NR_TILE = 256;             // candidates per LDS tile: 4 KB
constexpr int NR_SEED_THREADS = 1024;    // the one workgroup of the seed step
constexpr int NR_ORIENT_CHUNK = 16;      // rounds enqueued between two host reads of the state
constexpr int NR_JACOBI_SWEEPS = 6;      // cyclic sweeps of a 3 x 3: the off-diagonals are exactly 0 in fp64 after 5 (quadratic)

typedef unsigned long long u64;

struct OrientState { int remaining, progress, rounds, seeds; };

// Tiles are visited in the order t_s = s * stride mod ntiles (stride coprime with ntiles: every tile once).  The unsigned
// order of the keys does not depend on the order of the candidates, and a cloud stored along a sweep (a scanner's lines, a
// Fibonacci sphere) would otherwise bring a closer candidate -- an insertion -- at almost every step up to the query itself.
template <int K>
__global__ __launch_bounds__(NR_THREADS) void cloud_knn_kernel(const float* __restrict__ p, long long n, int k_use, int ntiles,
                                                               int stride, int* __restrict__ idx, float* __restrict__ d2out) {
  __shared__ float4 tile[NR_TILE];
  const long long i = (long long)blockIdx.x * NR_THREADS + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (i < n) { px = p[3 * i]; py = p[3 * i + 1]; pz = p[3 * i + 2]; }
  u64 best[K];
#pragma unroll
  for (int c = 0; c < K; ++c) best[c] = ~0ull;
  float worst = __uint_as_float(0xffffffffu);   // d^2 of the last entry; a NaN while the list is not full: no candidate is above it
  int t = 0;
  for (int step = 0; step < ntiles; ++step) {
    const long long j0 = (long long)t * NR_TILE;
    t += stride;
    t -= t >= ntiles ? ntiles : 0;
    const int m = (int)min((long long)NR_TILE, n - j0);
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
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (k == self || d2 > worst) continue;               // the float test is the hot one; equal d^2: the index decides below
      u64 key = ((u64)__float_as_uint(d2) << 32) | (u64)(unsigned)(j0 + k);
      if (key >= best[K - 1]) continue;
#pragma unroll
      for (int c = 0; c < K; ++c) {
        const u64 lo = key < best[c] ? key : best[c];
        key = key < best[c] ? best[c] : key;
        best[c] = lo;
      }
      worst = __uint_as_float((unsigned)(best[K - 1] >> 32));
    }
  }
  if (i >= n) return;
#pragma unroll
  for (int c = 0; c < K; ++c)
    if (c < k_use) {
      idx[i * k_use + c] = (int)(unsigned)(best[c] & 0xffffffffull);
      d2out[i * k_use + c] = __uint_as_float((unsigned)(best[c] >> 32));
    }
}

// One Jacobi rotation of the symmetric 3 x 3 in the (p, q) plane; r is the third axis.  v?p / v?q: columns p and q of V.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                                              double& v1p, double& v1q, double& v2p, double& v2q) {
  const double theta = (aqq - app) / (2. * apq);       // +-inf where apq is tiny: t = 0, the identity
  const double t = apq == 0. ? 0. : copysign(1., theta) / (fabs(theta) + sqrt(theta * theta + 1.));
  const double c = 1. / sqrt(t * t + 1.), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

// The covariance and its eigenvectors are computed in fp64: at k + 1 <= 17 points and 18 rotations per query it is a few
// microseconds of the chip's fp64 rate for 100 000 points, and an fp32 Jacobi measured four times the eigenvector error of
// LAPACK's fp32 solver where two eigenvalues lie close (error ~ eps / gap); in fp64 the result is the statement's, rounded
// once to fp32 on the way out.  A difference of two fp32 coordinates is exact in fp64, so nothing cancels.
// An index outside [0, n) is read as the point itself, so a bad `idx` cannot make the kernel read outside `p`.
__global__ __launch_bounds__(NR_THREADS) void cloud_normals_kernel(const float* __restrict__ p, long long n, const int* __restrict__ idx,
                                                                   int k, float* __restrict__ normals, float* __restrict__ variation) {
  const long long i = (long long)blockIdx.x * NR_THREADS + threadIdx.x;
  if (i >= n) return;
  const double px = p[3 * i], py = p[3 * i + 1], pz = p[3 * i + 2];
  const int* nb = idx + i * k;
  double sx = 0., sy = 0., sz = 0.;
  for (int c = 0; c < k; ++c) {
    long long j = nb[c];
    j = (j >= 0 && j < n) ? j : i;
    sx += (double)p[3 * j] - px; sy += (double)p[3 * j + 1] - py; sz += (double)p[3 * j + 2] - pz;
  }
  const double inv = 1. / (double)(k + 1);
  const double mx = sx * inv, my = sy * inv, mz = sz * inv;
  double cxx = mx * mx, cxy = mx * my, cxz = mx * mz, cyy = my * my, cyz = my * mz, czz = mz * mz;   // the point itself: 0 - m
  for (int c = 0; c < k; ++c) {
    long long j = nb[c];
    j = (j >= 0 && j < n) ? j : i;
    const double dx = ((double)p[3 * j] - px) - mx, dy = ((double)p[3 * j + 1] - py) - my, dz = ((double)p[3 * j + 2] - pz) - mz;
    cxx += dx * dx; cxy += dx * dy; cxz += dx * dz; cyy += dy * dy; cyz += dy * dz; czz += dz * dz;
  }
  // |c_ab| <= max diagonal for a positive semi-definite matrix: scaled to 1 the sweeps neither overflow nor underflow
  const double scale = fmax(cxx, fmax(cyy, czz));
  double nx = 1., ny = 0., nz = 0., var = 0.;            // all points equal: any unit vector
  if (scale > 0.) {
    double a00 = cxx / scale, a01 = cxy / scale, a02 = cxz / scale, a11 = cyy / scale, a12 = cyz / scale, a22 = czz / scale;
    double v00 = 1., v01 = 0., v02 = 0., v10 = 0., v11 = 1., v12 = 0., v20 = 0., v21 = 0., v22 = 1.;
#pragma unroll 1
    for (int sweep = 0; sweep < NR_JACOBI_SWEEPS; ++sweep) {
      jacobi_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
      jacobi_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
      jacobi_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    // the column of the smallest eigenvalue (ties: the lowest axis), picked by selects on two flags
    const bool use1 = a11 < a00;
    const double l01 = use1 ? a11 : a00;
    const bool use2 = a22 < l01;
    const double l0 = use2 ? a22 : l01;
    nx = use2 ? v02 : (use1 ? v01 : v00);
    ny = use2 ? v12 : (use1 ? v11 : v10);
    nz = use2 ? v22 : (use1 ? v21 : v20);
    const double sum = a00 + a11 + a22;
    var = sum > 0. ? fmax(l0, 0.) / sum : 0.;
  }
  // unit length and the sign rule hold for the fp32 numbers that leave, so both are applied after the rounding
  float fx = (float)nx, fy = (float)ny, fz = (float)nz;
  const float len = sqrtf(fx * fx + fy * fy + fz * fz);
  fx /= len; fy /= len; fz /= len;
  float lead = fx;
  if (fabsf(fy) > fabsf(lead)) lead = fy;
  if (fabsf(fz) > fabsf(lead)) lead = fz;
  if (lead < 0.f) { fx = -fx; fy = -fy; fz = -fz; }
  normals[3 * i] = fx; normals[3 * i + 1] = fy; normals[3 * i + 2] = fz;
  if (variation) variation[i] = (float)var;
}

__global__ void orient_init_kernel(OrientState* st, int n) {
  st->remaining = n; st->progress = 0; st->rounds = 0; st->seeds = 0;
}

// `level` and `normals` are read and written in the same launch (see the head of the file): no __restrict__ on them.
__global__ __launch_bounds__(NR_THREADS) void orient_round_kernel(float* normals, const int* __restrict__ idx, int n, int k, int r,
                                                                  int* level, OrientState* st) {
  if (st->remaining == 0) return;
  const long long i = (long long)blockIdx.x * NR_THREADS + threadIdx.x;
  if (i >= n || level[i] != 0) return;
  const float nx = normals[3 * i], ny = normals[3 * i + 1], nz = normals[3 * i + 2];
  const int* nb = idx + i * k;
  float best_abs = -1.f, best_dot = 0.f;
  for (int c = 0; c < k; ++c) {
    const int j = nb[c];
    if (j < 0 || j >= n) continue;
    const int lv = level[j];
    if (lv < 1 || lv >= r) continue;
    const float d = fmaf(nz, normals[3ll * j + 2], fmaf(ny, normals[3ll * j + 1], nx * normals[3ll * j]));
    if (fabsf(d) > best_abs) { best_abs = fabsf(d); best_dot = d; }
  }
  if (best_abs < 0.f) return;
  if (best_dot < 0.f) { normals[3 * i] = -nx; normals[3 * i + 1] = -ny; normals[3 * i + 2] = -nz; }
  level[i] = r;
  atomicAdd(&st->progress, 1);
}

// After round r, one workgroup: books the round's progress, or, where it made none and points remain, seeds.
__global__ __launch_bounds__(NR_SEED_THREADS) void orient_seed_kernel(const float* __restrict__ p, float* normals, int n, int r, int* level,
                                                                      OrientState* st) {
  __shared__ u64 red[NR_SEED_THREADS];
  __shared__ int state[2];
  const int tid = threadIdx.x;
  if (tid == 0) { state[0] = st->progress; state[1] = st->remaining; }
  __syncthreads();                       // every thread decides on the SAME two values; thread 0 writes them only after this
  const int progress = state[0], remaining = state[1];
  if (remaining == 0) return;
  if (progress > 0) {
    if (tid == 0) { st->remaining = remaining - progress; st->progress = 0; st->rounds += 1; }
    return;
  }
  u64 key = 0;                           // (z in an order-preserving code, ~index): the largest key is the top point, smallest index
  for (int j = tid; j < n; j += NR_SEED_THREADS) {
    if (level[j] != 0) continue;
    unsigned u = __float_as_uint(p[3ll * j + 2] + 0.f);              // + 0: -0 and +0 are one height
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    const u64 cand = ((u64)u << 32) | (u64)(0xffffffffu - (unsigned)j);
    key = cand > key ? cand : key;
  }
  red[tid] = key;
  __syncthreads();
  for (int w = NR_SEED_THREADS / 2; w > 0; w >>= 1) {
    if (tid < w) red[tid] = red[tid + w] > red[tid] ? red[tid + w] : red[tid];
    __syncthreads();
  }
  if (tid != 0 || red[0] == 0) return;
  const long long j = (long long)(0xffffffffu - (unsigned)(red[0] & 0xffffffffull));
  if (normals[3 * j + 2] < 0.f) {
    normals[3 * j] = -normals[3 * j]; normals[3 * j + 1] = -normals[3 * j + 1]; normals[3 * j + 2] = -normals[3 * j + 2];
  }
  level[j] = r;
  st->remaining = remaining - 1;
  st->seeds += 1;
}

// the step of the tile order: about 0.618 ntiles (successive tiles far apart, at every scale), coprime with ntiles
int knn_tile_stride(int ntiles) {
  if (ntiles < 3) return 1;
  int stride = (int)(0.6180339887 * ntiles);
  if (stride < 1) stride = 1;
  for (;; ++stride) {
    int a = stride, b = ntiles;
    while (b) { const int r = a % b; a = b; b = r; }
    if (a == 1) return stride;          // ntiles - 1 is coprime with ntiles: the search ends below ntiles
  }
}

struct OrientScratch { int* level; OrientState* st; long long bytes; };
OrientScratch orient_scratch(void* base, long long n) {
  Carve c{(char*)base};
  return {c.take<int>(n), c.take<OrientState>(1), c.total()};
}

}  // namespace

extern "C" int ishap_cloud_knn(const float* points, long long npoints, int k, int* idx, float* d2, void* stream) {
  ISHAP_REQUIRE(points && idx && d2 && npoints > 0, "cloud_knn arguments");
  ISHAP_REQUIRE(k >= 1 && k <= 16 && k < npoints, "cloud_knn: 1 <= k <= 16 and k < npoints (the k nearest OTHER points)");
  ISHAP_REQUIRE(npoints < (1ll << 31), "cloud_knn: point count (an index is an int)");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)((npoints + NR_THREADS - 1) / NR_THREADS)), block(NR_THREADS);
  const int ntiles = (int)((npoints + NR_TILE - 1) / NR_TILE);
  const int stride = knn_tile_stride(ntiles);
  if (k <= 4) hipLaunchKernelGGL(cloud_knn_kernel<4>, grid, block, 0, s, points, npoints, k, ntiles, stride, idx, d2);
  else if (k <= 8) hipLaunchKernelGGL(cloud_knn_kernel<8>, grid, block, 0, s, points, npoints, k, ntiles, stride, idx, d2);
  else hipLaunchKernelGGL(cloud_knn_kernel<16>, grid, block, 0, s, points, npoints, k, ntiles, stride, idx, d2);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_cloud_normals(const float* points, long long npoints, const int* idx, int k, float* normals, float* variation,
                                   void* stream) {
  ISHAP_REQUIRE(points && idx && normals && npoints > 0, "cloud_normals arguments");
  ISHAP_REQUIRE(k >= 1 && k <= 16 && k < npoints, "cloud_normals: 1 <= k <= 16 and k < npoints");
  ISHAP_REQUIRE(npoints < (1ll << 31), "cloud_normals: point count (an index is an int)");
  const dim3 grid((unsigned)((npoints + NR_THREADS - 1) / NR_THREADS)), block(NR_THREADS);
  hipLaunchKernelGGL(cloud_normals_kernel, grid, block, 0, (hipStream_t)stream, points, npoints, idx, k, normals, variation);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" long long ishap_cloud_orient_scratch_bytes(long long npoints) {
  if (npoints < 0) return -1;
  return orient_scratch(nullptr, npoints).bytes;
}

extern "C" int ishap_cloud_orient(const float* points, float* normals, const int* idx, long long npoints, int k, void* scratch,
                                  long long scratch_bytes, int* info, void* stream) {
  ISHAP_REQUIRE(points && normals && idx && scratch && info && npoints > 0, "cloud_orient arguments");
  ISHAP_REQUIRE(k >= 1 && k <= 16 && k < npoints, "cloud_orient: 1 <= k <= 16 and k < npoints");
  ISHAP_REQUIRE(npoints < (1ll << 30) - NR_ORIENT_CHUNK,
                "cloud_orient: point count (a level is an int, and there are up to 2 npoints rounds)");
  ISHAP_REQUIRE(scratch_bytes >= ishap_cloud_orient_scratch_bytes(npoints),
                "cloud_orient: scratch smaller than ishap_cloud_orient_scratch_bytes(npoints)");
  ISHAP_REQUIRE(((unsigned long long)scratch & 3ull) == 0, "cloud_orient: scratch must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int n = (int)npoints;
  const OrientScratch S = orient_scratch(scratch, npoints);
  int* level = S.level; OrientState* st = S.st;
  ISHAP_CHECK_HIP(hipMemsetAsync(level, 0, (size_t)npoints * sizeof(int), s));
  hipLaunchKernelGGL(orient_init_kernel, dim3(1), dim3(1), 0, s, st, n);
  const dim3 grid((unsigned)((npoints + NR_THREADS - 1) / NR_THREADS));
  OrientState h = {n, 0, 0, 0};
  // a round or its seed step orients at least one point while any remain: 2 n rounds always suffice
  const long long cap = 2 * npoints + 2;
  long long r = 1;
  while (h.remaining > 0) {
    ISHAP_REQUIRE(r <= cap, "cloud_orient: the rounds did not end (internal error)");
    for (int c = 0; c < NR_ORIENT_CHUNK; ++c, ++r) {
      hipLaunchKernelGGL(orient_round_kernel, grid, dim3(NR_THREADS), 0, s, normals, idx, n, k, (int)r, level, st);
      hipLaunchKernelGGL(orient_seed_kernel, dim3(1), dim3(NR_SEED_THREADS), 0, s, points, normals, n, (int)r, level, st);
    }
    ISHAP_CHECK_HIP(hipGetLastError());
    ISHAP_CHECK_HIP(hipMemcpyAsync(&h, st, sizeof(OrientState), hipMemcpyDeviceToHost, s));
    ISHAP_CHECK_HIP(hipStreamSynchronize(s));
  }
  info[0] = h.rounds;
  info[1] = h.seeds;
  return 0;
}
