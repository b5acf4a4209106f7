// Level-set surface of the decoded occupancy volume, on the device.
// Reference: triplane_decoder/visualize.py:100-104 (PyMCubes marching cubes at level 0, third-party, absent here),
// drag_utils.py:300 (Open3D filter_smooth_simple, 10 iterations), meshProcess.py:18-35 (Chamfer distance).
// PyMCubes' triangulation tables are not reproduced; the surface is extracted with MARCHING TETRAHEDRA: every grid cell
// is cut into the 6 tetrahedra around its main diagonal, each tetrahedron emits 0/1/2 triangles (16-case table).  The
// vertex SET is the one marching cubes produces on the 12 cube edges plus the crossings on face / body diagonals; every
// vertex sits on a grid edge at the linear zero crossing, is owned by the edge's lower end point, and is shared by all
// the triangles around it (indexed mesh, watertight inside the volume).
// Pipeline (HBM-bound scans over res^3 voxels, deterministic output order = voxel order):
//   count : per voxel, the 7 owned edges (+x, +y, +xy, +z, +xz, +yz, +xyz) that cross the level -> bit mask; per cell, the
//           number of triangles; per-block sums          -> exclusive scan of each array of block sums (scan.h), totals
//   emit  : vertices (block-local scan + block offset), per-voxel vertex offsets, then triangles through the
//           (owner voxel, edge type) -> vertex index lookup.
// The inside test, the tie rule and the edge interpolation are surface_rules.h, shared with the brick surface (sparse_surface.hip).
#include "common.h"
#include "mc_table.h"
#include "scan.h"
#include "surface_rules.h"
#include "winding.h"

namespace {

constexpr int SB_THREADS = 256;
constexpr int SB_ITEMS = 8;                       // voxels per thread
constexpr int SB_TILE = SB_THREADS * SB_ITEMS;    // voxels per workgroup

// cube corner i = (i & 1, (i >> 1) & 1, (i >> 2) & 1) -> (dx, dy, dz); the 6 tetrahedra share the diagonal 0-7
__constant__ unsigned char c_cube_tets[6][4] = {{0, 1, 3, 7}, {0, 3, 2, 7}, {0, 2, 6, 7}, {0, 6, 4, 7}, {0, 4, 5, 7}, {0, 5, 1, 7}};
__constant__ unsigned char c_tet_edges[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
__constant__ signed char c_tet_tri[16][6] = {{-1, -1, -1, -1, -1, -1}, {1, 0, 2, -1, -1, -1}, {4, 0, 3, -1, -1, -1}, {1, 4, 2, 1, 3, 4},
                                             {3, 1, 5, -1, -1, -1},   {2, 3, 0, 2, 5, 3},   {1, 4, 0, 1, 5, 4},   {4, 2, 5, -1, -1, -1},
                                             {4, 5, 2, -1, -1, -1},   {4, 1, 0, 4, 5, 1},   {3, 2, 0, 3, 5, 2},   {1, 3, 5, -1, -1, -1},
                                             {4, 1, 2, 4, 3, 1},      {3, 0, 4, -1, -1, -1}, {2, 0, 1, -1, -1, -1}, {-1, -1, -1, -1, -1, -1}};
__constant__ unsigned char c_tet_ntri[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};

struct SurfArgs {
  const float* vol;
  int res;
  float level;
  long long n;              // res^3
  unsigned char* emask;     // [n] crossing owned edges, bit (d-1) for direction bits d = dx | dy<<1 | dz<<2
  unsigned char* tcnt;      // [n] triangles of the cell whose lower corner is this voxel
  unsigned* voff;           // [n] index of the voxel's first vertex
  unsigned* bsum;           // [2][nblocks] per-block (vertices, triangles) -> exclusive prefix after the scan
  int nblocks;
  int method;               // 0: marching tetrahedra (7 edge types per voxel), 1: marching cubes (the 3 axis edges, 256-case table)
};

// inside bits of the 8 corners of the cell at (x, y, z); corners outside the grid read as "same as the voxel itself",
// which makes their edges non-crossing
__device__ __forceinline__ unsigned corner_bits(const SurfArgs& a, int x, int y, int z, bool& cell) {
  const int r = a.res;
  const long long p = ((long long)x * r + y) * r + z;
  const bool in0 = surf_inside(a.vol[p], a.level);
  const bool hx = x + 1 < r, hy = y + 1 < r, hz = z + 1 < r;
  cell = hx && hy && hz;
  unsigned bits = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bool ok = (!(c & 1) || hx) && (!(c & 2) || hy) && (!(c & 4) || hz);
    bool in = in0;
    if (ok && c) in = surf_inside(a.vol[p + ((long long)(c & 1) * r + ((c >> 1) & 1)) * r + ((c >> 2) & 1)], a.level);
    bits |= (in ? 1u : 0u) << c;
  }
  return bits;
}

__device__ __forceinline__ int cell_triangles(unsigned bits) {
  if (bits == 0u || bits == 255u) return 0;
  int n = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    unsigned code = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) code |= ((bits >> c_cube_tets[k][i]) & 1u) << i;
    n += c_tet_ntri[code];
  }
  return n;
}

__global__ __launch_bounds__(SB_THREADS) void surf_count_kernel(SurfArgs a) {
  __shared__ unsigned red[2][SB_THREADS];
  const int r = a.res;
  unsigned nv = 0, nt = 0;
  const long long base = (long long)blockIdx.x * SB_TILE + (long long)threadIdx.x * SB_ITEMS;
#pragma unroll
  for (int i = 0; i < SB_ITEMS; ++i) {
    const long long p = base + i;
    if (p >= a.n) break;
    const int z = (int)(p % r), y = (int)((p / r) % r), x = (int)(p / ((long long)r * r));
    bool cell;
    const unsigned bits = corner_bits(a, x, y, z, cell);
    const unsigned in0 = bits & 1u;
    unsigned m = 0;
#pragma unroll
    for (int d = 1; d < 8; ++d) m |= ((((bits >> d) & 1u) ^ in0) & 1u) << (d - 1);   // out-of-grid corners equal in0: never cross
    if (a.method == 1) m &= 0x0Bu;                                                    // marching cubes: only the axis edges d = 1, 2, 4
    const int tc = !cell ? 0 : (a.method == 1 ? (int)c_mc_ntri[bits] : cell_triangles(bits));
    a.emask[p] = (unsigned char)m;
    a.tcnt[p] = (unsigned char)tc;
    nv += __popc(m);
    nt += tc;
  }
  red[0][threadIdx.x] = nv;
  red[1][threadIdx.x] = nt;
  __syncthreads();
  for (int o = SB_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { a.bsum[blockIdx.x] = red[0][0]; a.bsum[a.nblocks + blockIdx.x] = red[1][0]; }
}

__global__ __launch_bounds__(SB_THREADS) void surf_emit_vertices_kernel(SurfArgs a, float* __restrict__ verts) {
  __shared__ unsigned lds[16];
  const int r = a.res;
  const long long base = (long long)blockIdx.x * SB_TILE + (long long)threadIdx.x * SB_ITEMS;
  unsigned cnt = 0;
  unsigned char m[SB_ITEMS];
#pragma unroll
  for (int i = 0; i < SB_ITEMS; ++i) {
    m[i] = base + i < a.n ? a.emask[base + i] : 0;
    cnt += __popc((unsigned)m[i]);
  }
  unsigned total;
  unsigned idx = a.bsum[blockIdx.x] + block_exclusive_scan(cnt, lds, total);
#pragma unroll
  for (int i = 0; i < SB_ITEMS; ++i) {
    const long long p = base + i;
    if (p >= a.n) break;
    a.voff[p] = idx;
    if (!m[i]) continue;
    const int z = (int)(p % r), y = (int)((p / r) % r), x = (int)(p / ((long long)r * r));
    const float va = a.vol[p] - a.level;
#pragma unroll
    for (int d = 1; d < 8; ++d) {
      if (!((m[i] >> (d - 1)) & 1)) continue;
      const int dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
      const float vb = a.vol[p + ((long long)dx * r + dy) * r + dz] - a.level;
      surf_edge_vertex(verts + 3LL * idx, x, y, z, dx, dy, dz, surf_edge_t(va, vb));
      ++idx;
    }
  }
}

__global__ __launch_bounds__(SB_THREADS) void surf_emit_triangles_kernel(SurfArgs a, int* __restrict__ tris) {
  __shared__ unsigned lds[16];
  const int r = a.res;
  const long long base = (long long)blockIdx.x * SB_TILE + (long long)threadIdx.x * SB_ITEMS;
  unsigned cnt = 0;
#pragma unroll
  for (int i = 0; i < SB_ITEMS; ++i) cnt += base + i < a.n ? a.tcnt[base + i] : 0;
  unsigned total;
  unsigned idx = a.bsum[a.nblocks + blockIdx.x] + block_exclusive_scan(cnt, lds, total);
  for (int i = 0; i < SB_ITEMS; ++i) {
    const long long p = base + i;
    if (p >= a.n) break;
    if (!a.tcnt[p]) continue;
    const int z = (int)(p % r), y = (int)((p / r) % r), x = (int)(p / ((long long)r * r));
    bool cell;
    const unsigned bits = corner_bits(a, x, y, z, cell);
    if (a.method == 1) {
      // marching cubes: each table entry names a cube edge = (lower corner, axis); its vertex is owned by that corner's
      // voxel under direction bit d = 1 << axis
      const int ntri = c_mc_ntri[bits];
      for (int tr = 0; tr < ntri; ++tr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int e = c_mc_tri[bits][3 * tr + c];
          const unsigned lo = c_mc_edge_lo[e], d = 1u << (e >> 2);
          const long long owner = p + ((long long)(lo & 1) * r + ((lo >> 1) & 1)) * r + ((lo >> 2) & 1);
          const unsigned below = (unsigned)a.emask[owner] & ((1u << (d - 1)) - 1u);
          tris[3LL * idx + c] = (int)(a.voff[owner] + __popc(below));
        }
        ++idx;
      }
      continue;
    }
    for (int k = 0; k < 6; ++k) {
      unsigned code = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) code |= ((bits >> c_cube_tets[k][j]) & 1u) << j;
      const int ntri = c_tet_ntri[code];
      for (int tr = 0; tr < ntri; ++tr) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int e = c_tet_tri[code][3 * tr + c];
          const unsigned ca = c_cube_tets[k][c_tet_edges[e][0]], cb = c_cube_tets[k][c_tet_edges[e][1]];
          const unsigned lo = ca & cb, hi = ca | cb;          // the corners of a tetrahedron form a chain: one contains the other
          const unsigned d = hi ^ lo;                          // direction bits of the edge, 1..7
          const long long owner = p + ((long long)(lo & 1) * r + ((lo >> 1) & 1)) * r + ((lo >> 2) & 1);
          const unsigned below = (unsigned)a.emask[owner] & ((1u << (d - 1)) - 1u);
          tris[3LL * idx + c] = (int)(a.voff[owner] + __popc(below));
        }
        ++idx;
      }
    }
  }
}

// ---- filter_smooth_simple: v <- (v + sum of neighbours) / (1 + #neighbours) -------------------------------------
// Neighbours are listed face by face (each directed edge of a face lists its head under its tail).  Inside a closed
// surface every undirected edge lies in exactly two faces, so each neighbour is listed twice: v <- (v + acc/2) / (1 + cnt/2).
// The lists are built ONCE per call as a CSR adjacency (count -> exclusive scan -> fill; 9 32-bit atomics per triangle in
// total) and every sweep is a gather, one thread per vertex, from the previous sweep's positions -- no atomics in the sweeps
// (round 4; the earlier form added every head to its tail with 64-bit atomics in every sweep: 18 ms per sweep on the 26 M
// triangles of a noise volume, 0.2 ms on a 300 k-triangle sphere).  The order of a vertex's list depends on the fill's
// atomics; the sum does not: it is formed in 64-bit fixed point (integer adds commute), so the result is bitwise
// reproducible and identical to the atomic form's.
constexpr float SMOOTH_SCALE = 1048576.f;     // 2^20: coordinates < 2^11, valence sums < 2^20 -> < 2^51

// which of the six faces of the grid box [0, bmax]^3 a vertex lies on (bit 2*axis: coordinate 0, bit 2*axis+1: bmax)
__global__ void smooth_boundary_mask_kernel(const float* __restrict__ v, long long nverts, float bmax, unsigned* __restrict__ mask) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nverts) return;
  unsigned m = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = v[3 * i + c];
    m |= (x <= 0.f ? 1u : 0u) << (2 * c);
    m |= (x >= bmax ? 1u : 0u) << (2 * c + 1);
  }
  mask[i] = m;
}
// An edge of a level-set mesh that lies IN a face of the grid box belongs to one triangle only (there is no cell on the
// other side), every other edge to two; the lone occurrence of a boundary edge therefore counts double (bit 31 of its list
// entry), so that after the halving in the sweep each neighbour has weight one -- Open3D's unique-adjacency rule -- on open
// meshes too.
__global__ void smooth_fill_kernel(const int* __restrict__ tris, long long ntris, const unsigned* __restrict__ off,
                                   unsigned* __restrict__ cursor, unsigned* __restrict__ adj, const unsigned* __restrict__ bmask) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= ntris) return;
  const int i[3] = {tris[3 * f], tris[3 * f + 1], tris[3 * f + 2]};
  unsigned bm[3] = {0u, 0u, 0u};
  if (bmask) { bm[0] = bmask[i[0]]; bm[1] = bmask[i[1]]; bm[2] = bmask[i[2]]; }
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int h1 = (e + 1) % 3, h2 = (e + 2) % 3;
    const unsigned slot = off[i[e]] + atomicAdd(cursor + i[e], 2u);
    adj[slot] = (unsigned)i[h1] | ((bm[e] & bm[h1]) ? 0x80000000u : 0u);
    adj[slot + 1] = (unsigned)i[h2] | ((bm[e] & bm[h2]) ? 0x80000000u : 0u);
  }
}
__global__ void smooth_sweep_kernel(const float* __restrict__ vin, float* __restrict__ vout, long long nverts,
                                    const unsigned* __restrict__ off, const unsigned* __restrict__ adj) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nverts) return;
  const unsigned lo = off[i], hi = off[i + 1];
  long long acc[3] = {0, 0, 0};
  unsigned cnt = 0;
  for (unsigned k = lo; k < hi; ++k) {
    const unsigned e = adj[k];
    const long long h = (long long)(e & 0x7fffffffu);
    const bool dbl = (e >> 31) != 0u;
    const float w = (dbl ? 2.f : 1.f) * SMOOTH_SCALE;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[c] += __float2ll_rn(vin[3 * h + c] * w);
    cnt += dbl ? 2u : 1u;
  }
  const float half_n = 0.5f * (float)cnt;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float sm = (float)acc[c] * (1.f / SMOOTH_SCALE);
    vout[3 * i + c] = (vin[3 * i + c] + 0.5f * sm) / (1.f + half_n);
  }
}

// ---- Chamfer: for every point of A the squared distance to its nearest point of B (exact differences) ------------
__global__ __launch_bounds__(256) void nearest_sq_kernel(const float* __restrict__ A, long long na, const float* __restrict__ B,
                                                          long long nb, float* __restrict__ out) {
  __shared__ float tile[1024 * 3];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float ax = 0.f, ay = 0.f, az = 0.f;
  if (i < na) { ax = A[3 * i]; ay = A[3 * i + 1]; az = A[3 * i + 2]; }
  float best = 3.0e38f;
  for (long long j0 = 0; j0 < nb; j0 += 1024) {
    const int m = (int)min(1024LL, nb - j0);
    __syncthreads();
    for (int k = threadIdx.x; k < m * 3; k += 256) tile[k] = B[3 * j0 + k];
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < m; ++k) {
      const float dx = ax - tile[3 * k], dy = ay - tile[3 * k + 1], dz = az - tile[3 * k + 2];
      best = fminf(best, dx * dx + dy * dy + dz * dz);
    }
  }
  if (i < na) out[i] = best;
}
// mean of n floats, fixed summation order (one workgroup, double accumulators)
__global__ __launch_bounds__(1024) void mean_kernel(const float* __restrict__ x, long long n, float* __restrict__ out) {
  __shared__ double red[1024];
  double s = 0.0;
  const long long per = (n + 1023) / 1024;
  const long long b0 = threadIdx.x * per, b1 = min(n, b0 + per);
  for (long long i = b0; i < b1; ++i) s += (double)x[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = n > 0 ? (float)(red[0] / (double)n) : 0.f;
}

// ---- occupancy sampling of an input mesh (drag_utils.py:411-440: Open3D sample_points_uniformly + RaycastingScene
//      .compute_occupancy in the reference) ----------------------------------------------------------------------------
__global__ void tri_area_kernel(const float* __restrict__ v, const int* __restrict__ t, long long nt, float* __restrict__ area) {
  const long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= nt) return;
  const float* A = v + 3LL * t[3 * f]; const float* B = v + 3LL * t[3 * f + 1]; const float* C = v + 3LL * t[3 * f + 2];
  const float ux = B[0] - A[0], uy = B[1] - A[1], uz = B[2] - A[2];
  const float wx = C[0] - A[0], wy = C[1] - A[1], wz = C[2] - A[2];
  const float cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
  area[f] = 0.5f * sqrtf(cx * cx + cy * cy + cz * cz);
}
// uniform point on triangle f = idx[i] from two uniforms (u, w): (1-sqrt(u)) A + sqrt(u)(1-w) B + sqrt(u) w C
__global__ void tri_point_kernel(const float* __restrict__ v, const int* __restrict__ t, const int* __restrict__ idx,
                                 const float* __restrict__ uw, long long n, float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long f = idx[i];
  const float* A = v + 3LL * t[3 * f]; const float* B = v + 3LL * t[3 * f + 1]; const float* C = v + 3LL * t[3 * f + 2];
  const float su = sqrtf(uw[2 * i]), w = uw[2 * i + 1];
  const float a = 1.f - su, b = su * (1.f - w), c = su * w;
#pragma unroll
  for (int k = 0; k < 3; ++k) out[3 * i + k] = a * A[k] + b * B[k] + c * C[k];
}
// inside / outside by the parity of the crossings of the ray p + s*(1,0,0), s > 0.  Triangles are staged through LDS
// (256 at a time); a thread owns one point.  A crossing needs the point's (y,z) strictly inside the triangle's (y,z)
// projection, so rays through an edge or a vertex (measure zero for random samples) are not counted.
__global__ __launch_bounds__(256) void occupancy_kernel(const float* __restrict__ v, const int* __restrict__ t, long long nt,
                                                        const float* __restrict__ pts, long long np, float* __restrict__ occ) {
  __shared__ float tri[256][9];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (i < np) { px = pts[3 * i]; py = pts[3 * i + 1]; pz = pts[3 * i + 2]; }
  unsigned crossings = 0;
  for (long long f0 = 0; f0 < nt; f0 += 256) {
    const int m = (int)min(256LL, nt - f0);
    __syncthreads();
    if ((int)threadIdx.x < m) {
      const long long f = f0 + threadIdx.x;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* P = v + 3LL * t[3 * f + c];
        tri[threadIdx.x][3 * c] = P[0]; tri[threadIdx.x][3 * c + 1] = P[1]; tri[threadIdx.x][3 * c + 2] = P[2];
      }
    }
    __syncthreads();
    for (int k = 0; k < m; ++k) {
      // barycentric coordinates in the (y,z) plane relative to vertex A: differences of nearby numbers stay accurate
      // however far the point is; a triangle seen edge-on (negligible projected area) cannot be crossed
      const float uy = tri[k][4] - tri[k][1], uz = tri[k][5] - tri[k][2];
      const float wy = tri[k][7] - tri[k][1], wz = tri[k][8] - tri[k][2];
      const float qy = py - tri[k][1], qz = pz - tri[k][2];
      const float D = uy * wz - uz * wy;
      if (fabsf(D) <= 1e-6f * (fabsf(uy) + fabsf(uz)) * (fabsf(wy) + fabsf(wz))) continue;
      const float sB = (qy * wz - qz * wy) / D, sC = (uy * qz - uz * qy) / D;
      if (sB > 0.f && sC > 0.f && sB + sC < 1.f) {
        const float xh = tri[k][0] + sB * (tri[k][3] - tri[k][0]) + sC * (tri[k][6] - tri[k][0]);
        crossings += xh > px ? 1u : 0u;
      }
    }
  }
  if (i < np) occ[i] = (crossings & 1u) ? 1.f : 0.f;
}

// ---- distance from a point to a triangle mesh (meshProcess.py:7-14, 108-118: RaycastingScene.compute_signed_distance /
//      compute_closest_points in the reference) ------------------------------------------------------------------------
// Triangles go through LDS in tiles of MD_TILE, one thread owns a point (as occupancy_kernel).  Every tile has an
// axis-aligned box (mesh_tile_box_kernel).  Before the tile loop a lane bounds its answer from above by the distance to the
// farthest corner of the nearest box; a workgroup then skips every tile whose box no lane could find a closer triangle in
// (block-wide vote).  Marching cubes emits triangles in voxel order, so a tile is a compact strip of the surface.
constexpr int MD_TILE = 256;
// The box test is a lower bound only up to rounding: a tile is skipped when its fp32 box distance exceeds the fp32 bound
// by a relative MD_REL plus MD_ABS times the coordinate magnitude (the error of the fp32 closest point is a few ulp of
// that magnitude).  Any triangle whose computed distance could reach the final minimum is therefore visited, and the
// outputs are bit for bit those of visiting every tile.
constexpr float MD_REL = 1e-4f, MD_ABS = 2e-5f;

// box of tile b: {lo.xyz, max |coordinate|}, {hi.xyz, 0}
__global__ __launch_bounds__(MD_TILE) void mesh_tile_box_kernel(const float* __restrict__ v, const int* __restrict__ t,
                                                                long long nt, float4* __restrict__ box) {
  __shared__ float red[6][MD_TILE];
  const long long f = (long long)blockIdx.x * MD_TILE + threadIdx.x;
  float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  if (f < nt) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* P = v + 3LL * t[3 * f + c];
#pragma unroll
      for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], P[k]); hi[k] = fmaxf(hi[k], P[k]); }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { red[k][threadIdx.x] = lo[k]; red[3 + k][threadIdx.x] = hi[k]; }
  __syncthreads();
  for (int o = MD_TILE / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        red[k][threadIdx.x] = fminf(red[k][threadIdx.x], red[k][threadIdx.x + o]);
        red[3 + k][threadIdx.x] = fmaxf(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + o]);
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    float mag = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) mag = fmaxf(mag, fabsf(red[k][0]));
    box[2 * blockIdx.x] = make_float4(red[0][0], red[1][0], red[2][0], mag);
    box[2 * blockIdx.x + 1] = make_float4(red[3][0], red[4][0], red[5][0], 0.f);
  }
}

// A triangle as the distance kernel stages it: a frame of its own and the triangle in that frame, built once per staged
// triangle (tri_frame) and read by every lane (tri_dist2).
//   r0 = {a.xyz, L}    a: first vertex after rotating the triangle so that its longest edge is a-b;  L = |ab|
//   r1 = {e1.xyz, cx}  e1 = ab / L
//   r2 = {e2.xyz, cy}  e2: unit, across e1 in the triangle's plane, towards c;  c = a + cx e1 + cy e2, cy >= 0
//   r3 = {1/|ac|^2, 1/|bc|^2, 0, 0}  (0 for an edge without length)
// A triangle without area has e2 = 0 (it is its longest edge), one without extent e1 = e2 = 0 (it is the point a).
//
// Why a frame and not Ericson's selection on the 3-D dot products: on a thin triangle the normal, and every barycentric
// coordinate made from products of dot products, is a difference of nearly equal numbers; in float32 a triangle whose height
// is 1e-3 of its length gets coordinates that are wrong by several percent, hence a closest point that far along the
// triangle.  Here the only ill-conditioned quantity is the direction of e2, off by about (ulp * length / height) radians on
// a thin triangle; turning the frame about the line a-b by that angle moves no point of the triangle by more than
// angle * height = a few ulp of its length.  e2 is orthogonalised against e1 twice, so that rounding noise standing in
// for the height of a (nearly) collinear triangle still gives an orthonormal frame.
__device__ __forceinline__ void tri_frame(const float* __restrict__ A, const float* __restrict__ B, const float* __restrict__ Cv,
                                          float4* __restrict__ out) {
  float a[3] = {A[0], A[1], A[2]}, b[3] = {B[0], B[1], B[2]}, c[3] = {Cv[0], Cv[1], Cv[2]};
  float lab = 0.f, lbc = 0.f, lca = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lab += (b[k] - a[k]) * (b[k] - a[k]); lbc += (c[k] - b[k]) * (c[k] - b[k]); lca += (a[k] - c[k]) * (a[k] - c[k]);
  }
  const bool rot1 = lbc > lab && lbc >= lca, rot2 = !rot1 && lca > lab && lca > lbc;      // (b, c, a) or (c, a, b)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float a0 = a[k], b0 = b[k], c0 = c[k];
    a[k] = rot1 ? b0 : rot2 ? c0 : a0; b[k] = rot1 ? c0 : rot2 ? a0 : b0; c[k] = rot1 ? a0 : rot2 ? b0 : c0;
  }
  float e1[3] = {0.f, 0.f, 0.f}, e2[3] = {0.f, 0.f, 0.f}, ac[3], L = 0.f, cx = 0.f, cy = 0.f, iac = 0.f, ibc = 0.f;
  float l2 = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) { ac[k] = c[k] - a[k]; l2 += (b[k] - a[k]) * (b[k] - a[k]); }
  if (l2 > 0.f) {
    L = sqrtf(l2);
#pragma unroll
    for (int k = 0; k < 3; ++k) e1[k] = (b[k] - a[k]) / L;
    cx = ac[0] * e1[0] + ac[1] * e1[1] + ac[2] * e1[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) e2[k] = ac[k] - cx * e1[k];
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {        // normalise; twice more after removing what is left along e1
      const float n2 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
      const float inv = n2 > 0.f ? 1.f / sqrtf(n2) : 0.f;
#pragma unroll
      for (int k = 0; k < 3; ++k) e2[k] *= inv;
      if (pass < 2) {
        const float along = e2[0] * e1[0] + e2[1] * e1[1] + e2[2] * e1[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) e2[k] -= along * e1[k];
      }
    }
    cy = ac[0] * e2[0] + ac[1] * e2[1] + ac[2] * e2[2];
    if (cy < 0.f) { cy = -cy; e2[0] = -e2[0]; e2[1] = -e2[1]; e2[2] = -e2[2]; }
    const float lac = cx * cx + cy * cy, lcb = (cx - L) * (cx - L) + cy * cy;
    iac = lac > 0.f ? 1.f / lac : 0.f;
    ibc = lcb > 0.f ? 1.f / lcb : 0.f;
  }
  out[0] = make_float4(a[0], a[1], a[2], L);
  out[1] = make_float4(e1[0], e1[1], e1[2], cx);
  out[2] = make_float4(e2[0], e2[1], e2[2], cy);
  out[3] = make_float4(iac, ibc, 0.f, 0.f);
}

// Squared distance from p to a staged triangle: p in the triangle's frame is (x, y) in its plane and a remainder across it;
// the answer is |remainder|^2 plus the squared 2-D distance from (x, y) to the triangle (0,0), (L,0), (cx,cy): zero strictly
// inside, else the nearest of the three clamped edges.  Straight-line code, no division.  A wrong inside decision next to
// an edge costs at most the rounding of the edge's position, because the 2-D distance goes to zero there.
__device__ __forceinline__ float tri_dist2(float px, float py, float pz, float4 r0, float4 r1, float4 r2, float4 r3) {
  const float apx = px - r0.x, apy = py - r0.y, apz = pz - r0.z;
  const float L = r0.w, cx = r1.w, cy = r2.w;
  const float x = apx * r1.x + apy * r1.y + apz * r1.z, y = apx * r2.x + apy * r2.y + apz * r2.z;
  const float rx = apx - x * r1.x - y * r2.x, ry = apy - x * r1.y - y * r2.y, rz = apz - x * r1.z - y * r2.z;
  const float z2 = rx * rx + ry * ry + rz * rz;
  const float u0 = x - fminf(fmaxf(x, 0.f), L);                                            // edge a-b
  const float d0 = u0 * u0 + y * y;
  const float t1 = fminf(fmaxf((x * cx + y * cy) * r3.x, 0.f), 1.f);                       // edge a-c
  const float u1 = x - t1 * cx, v1 = y - t1 * cy;
  const float d1 = u1 * u1 + v1 * v1;
  const float bx = x - L, ex = cx - L;
  const float t2 = fminf(fmaxf((bx * ex + y * cy) * r3.y, 0.f), 1.f);                      // edge b-c
  const float u2 = bx - t2 * ex, v2 = y - t2 * cy;
  const float d2 = u2 * u2 + v2 * v2;
  const bool inside = y > 0.f && ex * y - cy * bx > 0.f && cy * x - cx * y > 0.f;
  return z2 + (inside ? 0.f : fminf(fminf(d0, d1), d2));
}

// d2[i] = min over triangles of the squared distance, tri[i] = its lowest index (tiles and triangles are visited in index
// order and only a strictly smaller distance replaces the best).  occ (may be null): sign source, dist[i] = -sqrt(d2) where
// occ[i] != 0; out[i] may alias occ[i] (read before written by the same lane).
__global__ __launch_bounds__(MD_TILE) void mesh_distance_kernel(const float* __restrict__ v, const int* __restrict__ t,
                                                                long long nt, const float4* __restrict__ box,
                                                                const float* __restrict__ pts, long long np, const float* occ,
                                                                float* out, int* __restrict__ tri_out) {
  __shared__ float4 tri[MD_TILE][4];
  const long long i = (long long)blockIdx.x * MD_TILE + threadIdx.x;
  const bool live = i < np;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (live) { px = pts[3 * i]; py = pts[3 * i + 1]; pz = pts[3 * i + 2]; }
  const float pmag = fmaxf(fabsf(px), fmaxf(fabsf(py), fabsf(pz)));
  const int ntiles = (int)((nt + MD_TILE - 1) / MD_TILE);
  // upper bound: every triangle of a tile lies in its box, so none is farther than the box's farthest corner
  float bound = 3.0e38f;
  for (int b = 0; b < ntiles; ++b) {
    const float4 lo = box[2 * b], hi = box[2 * b + 1];
    const float fx = fmaxf(fabsf(px - lo.x), fabsf(hi.x - px)), fy = fmaxf(fabsf(py - lo.y), fabsf(hi.y - py));
    const float fz = fmaxf(fabsf(pz - lo.z), fabsf(hi.z - pz));
    bound = fminf(bound, fx * fx + fy * fy + fz * fz);
  }
  float best = 3.4e38f;
  int best_f = -1;
  for (int b = 0; b < ntiles; ++b) {
    const float4 lo = box[2 * b], hi = box[2 * b + 1];
    const float gx = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.f), gy = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.f);
    const float lim = sqrtf(fminf(bound, best)) * (1.f + MD_REL) + MD_ABS * (pmag + lo.w);
    const bool need = live && gx * gx + gy * gy + gz * gz <= lim * lim;
    if (!__syncthreads_or(need)) continue;          // also the barrier before the tile is restaged
    const long long f0 = (long long)b * MD_TILE;
    const int m = (int)min((long long)MD_TILE, nt - f0);
    if ((int)threadIdx.x < m) {
      const long long f = f0 + threadIdx.x;
      tri_frame(v + 3LL * t[3 * f], v + 3LL * t[3 * f + 1], v + 3LL * t[3 * f + 2], tri[threadIdx.x]);
    }
    __syncthreads();
    if (need) {
      for (int k = 0; k < m; ++k) {
        const float dd = tri_dist2(px, py, pz, tri[k][0], tri[k][1], tri[k][2], tri[k][3]);
        if (dd < best) { best = dd; best_f = (int)(f0 + k); }
      }
    }
  }
  if (!live) return;
  const float d = sqrtf(best);
  float s = d;
  if (occ) s = occ[i] != 0.f ? -d : d;
  out[i] = s;
  if (tri_out) tri_out[i] = best_f;
}

// out[0] = max of x[0, na), out[1] = max of x[na, na + nb) (one workgroup; the maximum does not depend on the order)
__global__ __launch_bounds__(1024) void max2_kernel(const float* __restrict__ x, long long na, long long nb, float* __restrict__ out) {
  __shared__ float red[1024];
  for (int h = 0; h < 2; ++h) {
    const float* y = h ? x + na : x;
    const long long n = h ? nb : na;
    float m = -3.4e38f;
    for (long long k = threadIdx.x; k < n; k += 1024) m = fmaxf(m, y[k]);
    __syncthreads();
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]);
      __syncthreads();
    }
    if (threadIdx.x == 0) out[h] = red[0];
  }
}

// Per group g of P values of two fields on the same sample positions: out[g] = |A and B| / |A or B| (inside: field < 0, or
// field != 0 when `occupancy`), out[G + g] = mean of (b - a)^2.  One workgroup per group, fixed summation order, double
// accumulators; the counts are exact.  An empty union gives 0/0 = NaN (the reference's division).
__global__ __launch_bounds__(256) void group_stats_kernel(const float* __restrict__ fa, const float* __restrict__ fb, long long P,
                                                          int G, int occupancy, float* __restrict__ out) {
  __shared__ double red[3][256];
  const long long g = blockIdx.x;
  const float* a = fa + g * P;
  const float* b = fb + g * P;
  const long long per = (P + 255) / 256;
  const long long k0 = threadIdx.x * per, k1 = min(P, k0 + per);
  double inter = 0.0, uni = 0.0, sq = 0.0;
  for (long long k = k0; k < k1; ++k) {
    const float x = a[k], y = b[k];
    const bool ia = occupancy ? x != 0.f : x < 0.f, ib = occupancy ? y != 0.f : y < 0.f;
    inter += (ia && ib) ? 1.0 : 0.0;
    uni += (ia || ib) ? 1.0 : 0.0;
    const double e = (double)y - (double)x;
    sq += e * e;
  }
  red[0][threadIdx.x] = inter; red[1][threadIdx.x] = uni; red[2][threadIdx.x] = sq;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[g] = (float)(red[0][0] / red[1][0]);
    out[G + g] = (float)(red[2][0] / (double)P);
  }
}
// out[2G] = mean over groups of out[0, G), out[2G + 1] = mean of out[G, 2G) (in group order)
__global__ void group_mean_kernel(int G, float* __restrict__ out) {
  if (threadIdx.x != 0) return;
  double s0 = 0.0, s1 = 0.0;
  for (int g = 0; g < G; ++g) { s0 += (double)out[g]; s1 += (double)out[G + g]; }
  out[2 * G] = (float)(s0 / G);
  out[2 * G + 1] = (float)(s1 / G);
}

// the scratch, packed: voff[n] | bsum[2 nblocks] | emask[n] | tcnt[n] | 256 bytes of slack.  Sets a's sizes and pointers, returns the bytes
long long surf_carve(SurfArgs& a, void* base, int res) {
  a.n = (long long)res * res * res;
  const long long nb = (a.n + SB_TILE - 1) / SB_TILE;
  a.nblocks = (int)nb;
  Carve c{(char*)base};
  a.voff = c.take<unsigned>(a.n, 1);
  a.bsum = c.take<unsigned>(2 * nb, 1);
  a.emask = c.take<unsigned char>(a.n, 1);
  a.tcnt = c.take<unsigned char>(a.n, 1);
  c.bytes(256, 1);
  return c.total(1);
}
int fill(SurfArgs& a, const float* volume, int res, float level, void* scratch) {
  ISHAP_REQUIRE(volume && scratch && res >= 2 && res <= 1024, "surface: volume, scratch and 2 <= res <= 1024");
  a.vol = volume; a.res = res; a.level = level; a.method = 0;
  surf_carve(a, scratch, res);
  return 0;
}

}  // namespace

extern "C" long long ishap_surface_scratch_bytes(int res) { SurfArgs a; return surf_carve(a, nullptr, res); }

extern "C" int ishap_surface_count(const float* volume, int res, float level, int method, void* scratch, unsigned* counts,
                                   void* stream) {
  SurfArgs a;
  ISHAP_TRY(fill(a, volume, res, level, scratch));
  ISHAP_REQUIRE(counts && (method == 0 || method == 1), "method: 0 marching tetrahedra, 1 marching cubes");
  a.method = method;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(surf_count_kernel, dim3(a.nblocks), dim3(SB_THREADS), 0, s, a);
  scan_block_totals(a.bsum, a.nblocks, counts, s);                       // vertices
  scan_block_totals(a.bsum + a.nblocks, a.nblocks, counts + 1, s);       // triangles
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_surface_emit(const float* volume, int res, float level, int method, void* scratch, float* verts, int* tris,
                                  void* stream) {
  SurfArgs a;
  ISHAP_TRY(fill(a, volume, res, level, scratch));
  ISHAP_REQUIRE(verts && tris && (method == 0 || method == 1), "null argument / method");
  a.method = method;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(surf_emit_vertices_kernel, dim3(a.nblocks), dim3(SB_THREADS), 0, s, a, verts);
  hipLaunchKernelGGL(surf_emit_triangles_kernel, dim3(a.nblocks), dim3(SB_THREADS), 0, s, a, tris);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

// scratch layout: off[nverts + 1] | cursor[nverts] | block totals | boundary mask[nverts] | second vertex buffer | adj[6 ntris]
namespace {
struct SmoothLayout { unsigned *off, *cursor, *totals, *bmask, *adj; float* vtmp; long long zero_end, bytes, nblocks; };
SmoothLayout smooth_layout(void* base, long long nverts, long long ntris) {
  Carve c{(char*)base};
  SmoothLayout L;
  L.nblocks = scan_u32_blocks(nverts + 1);
  L.off = c.take<unsigned>(nverts + 1);
  L.cursor = c.take<unsigned>(nverts);
  L.zero_end = c.total();                    // [0, zero_end): list lengths and fill cursors, cleared at the start of a call
  L.totals = c.take<unsigned>(L.nblocks + 1);
  L.bmask = c.take<unsigned>(nverts);
  L.vtmp = c.take<float>(3 * nverts);
  L.adj = c.take<unsigned>(6 * ntris);
  L.bytes = c.total();
  return L;
}
}  // namespace

extern "C" long long ishap_mesh_smooth_scratch_bytes(long long nverts, long long ntris) {
  if (nverts < 0 || ntris < 0) return -1;
  return smooth_layout(nullptr, nverts, ntris).bytes;
}

extern "C" int ishap_mesh_smooth(float* verts, long long nverts, const int* tris, long long ntris, int iterations, float box_max,
                                 void* scratch, long long scratch_bytes, void* stream) {
  ISHAP_REQUIRE(verts && tris && scratch && nverts >= 0 && ntris >= 0 && iterations >= 0, "mesh_smooth arguments");
  ISHAP_REQUIRE(scratch_bytes >= ishap_mesh_smooth_scratch_bytes(nverts, ntris), "mesh_smooth: scratch smaller than ishap_mesh_smooth_scratch_bytes(nverts, ntris)");
  ISHAP_REQUIRE(nverts < (1ll << 31) && 6 * ntris < (1ll << 32), "mesh_smooth: 32-bit vertex indices and list offsets");
  if (nverts == 0 || ntris == 0 || iterations == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const SmoothLayout L = smooth_layout(scratch, nverts, ntris);
  unsigned *off = L.off, *cursor = L.cursor, *totals = L.totals, *adj = L.adj, *bmask = box_max > 0.f ? L.bmask : nullptr;
  float* vtmp = L.vtmp;
  const unsigned tb = (unsigned)((ntris + 255) / 256), vb = (unsigned)((nverts + 255) / 256);
  ISHAP_CHECK_HIP(hipMemsetAsync(scratch, 0, (size_t)L.zero_end, s));         // list lengths and fill cursors
  if (bmask) hipLaunchKernelGGL(smooth_boundary_mask_kernel, dim3(vb), dim3(256), 0, s, verts, nverts, box_max, bmask);
  count_triangle_corners(tris, ntris, 2u, off, s);                           // every face lists two heads under each of its corners
  scan_exclusive_u32(off, nverts + 1, totals, totals + L.nblocks, s);        // list lengths -> list starts, off[nverts] = their sum
  hipLaunchKernelGGL(smooth_fill_kernel, dim3(tb), dim3(256), 0, s, tris, ntris, off, cursor, adj, bmask);
  for (int it = 0; it < iterations; ++it) {
    const float* src = (it & 1) ? vtmp : verts;
    float* dst = (it & 1) ? verts : vtmp;
    hipLaunchKernelGGL(smooth_sweep_kernel, dim3(vb), dim3(256), 0, s, src, dst, nverts, off, adj);
  }
  if (iterations & 1) ISHAP_CHECK_HIP(hipMemcpyAsync(verts, vtmp, (size_t)nverts * 12, hipMemcpyDeviceToDevice, s));
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_chamfer(const float* a, long long na, const float* b, long long nb, float* nearest, float* out2, void* stream) {
  ISHAP_REQUIRE(a && b && nearest && out2 && na > 0 && nb > 0, "chamfer arguments");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nearest_sq_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, s, a, na, b, nb, nearest);
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(1024), 0, s, nearest, na, out2);
  hipLaunchKernelGGL(nearest_sq_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, b, nb, a, na, nearest);
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(1024), 0, s, nearest, nb, out2 + 1);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_mesh_tri_areas(const float* verts, const int* tris, long long ntris, float* areas, void* stream) {
  ISHAP_REQUIRE(verts && tris && areas && ntris > 0, "mesh_tri_areas arguments");
  hipLaunchKernelGGL(tri_area_kernel, dim3((unsigned)((ntris + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, tris, ntris, areas);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_mesh_points_on_tris(const float* verts, const int* tris, const int* tri_idx, const float* uw, long long n,
                                         float* pts, void* stream) {
  ISHAP_REQUIRE(verts && tris && tri_idx && uw && pts && n > 0, "mesh_points_on_tris arguments");
  hipLaunchKernelGGL(tri_point_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, tris, tri_idx, uw, n, pts);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_mesh_occupancy(const float* verts, const int* tris, long long ntris, const float* pts, long long npts,
                                    float* occ, void* stream) {
  ISHAP_REQUIRE(verts && tris && pts && occ && ntris > 0 && npts > 0, "mesh_occupancy arguments");
  hipLaunchKernelGGL(occupancy_kernel, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, (hipStream_t)stream, verts, tris, ntris, pts,
                     npts, occ);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

// scratch layout: the tile boxes; sdf == 2 / -2 adds the winding number's part sums behind them (256-byte aligned)
namespace {
struct DistScratch { float4* box; char* wn; long long bytes; };
DistScratch dist_scratch(void* base, long long ntris, long long npts, bool winding) {
  Carve c{(char*)base};
  return {c.take<float4>((ntris + MD_TILE - 1) / MD_TILE * 2), winding ? c.bytes(ishap_winding_bytes(ntris, npts)) : nullptr,
          c.total(1)};
}
}  // namespace

extern "C" long long ishap_mesh_distance_scratch_bytes(long long ntris) {
  if (ntris < 0) return -1;
  return dist_scratch(nullptr, ntris, 0, false).bytes;
}

// every sdf other than 2 / -2 is what ishap_mesh_distance makes of it: unsigned (0) or signed by parity
extern "C" long long ishap_mesh_distance_scratch_bytes_sdf(long long ntris, long long npts, int sdf) {
  if (ntris < 0 || npts < 0) return -1;
  return dist_scratch(nullptr, ntris, npts, sdf == 2 || sdf == -2).bytes;
}

extern "C" int ishap_mesh_distance(const float* verts, const int* tris, long long ntris, const float* pts, long long npts, int sdf,
                                   float* dist, int* tri, void* scratch, long long scratch_bytes, void* stream) {
  ISHAP_REQUIRE(verts && tris && pts && dist && scratch && ntris > 0 && npts > 0, "mesh_distance arguments");
  ISHAP_REQUIRE(scratch_bytes >= ishap_mesh_distance_scratch_bytes(ntris),
                "mesh_distance: scratch smaller than ishap_mesh_distance_scratch_bytes(ntris)");
  ISHAP_REQUIRE(ntris < (1ll << 31), "mesh_distance: triangle indices must fit 31 bits");
  const bool winding = sdf == 2 || sdf == -2;
  ISHAP_REQUIRE(!winding || scratch_bytes >= ishap_mesh_distance_scratch_bytes_sdf(ntris, npts, 2),
                "mesh_distance: sdf == 2 / -2 needs ishap_mesh_distance_scratch_bytes_sdf(ntris, npts, 2) bytes of scratch");
  hipStream_t s = (hipStream_t)stream;
  const unsigned tiles = (unsigned)((ntris + MD_TILE - 1) / MD_TILE), blocks = (unsigned)((npts + MD_TILE - 1) / MD_TILE);
  const DistScratch S = dist_scratch(scratch, ntris, npts, winding);
  // the sign is an inside flag per point: its 0/1 value lands in dist and the distance kernel reads it back per point.
  // sdf == 2: inside where the winding number exceeds 0.5 (-2: is below -0.5, a clockwise mesh); any other non-zero sdf:
  // ishap_mesh_occupancy's ray parity
  if (winding) {
    ishap_winding_launch_mesh(verts, tris, ntris, pts, npts, dist, sdf > 0 ? 1 : -1, S.wn, s);
  } else if (sdf) {
    hipLaunchKernelGGL(occupancy_kernel, dim3(blocks), dim3(256), 0, s, verts, tris, ntris, pts, npts, dist);
  }
  hipLaunchKernelGGL(mesh_tile_box_kernel, dim3(tiles), dim3(MD_TILE), 0, s, verts, tris, ntris, S.box);
  hipLaunchKernelGGL(mesh_distance_kernel, dim3(blocks), dim3(MD_TILE), 0, s, verts, tris, ntris, (const float4*)S.box, pts, npts,
                     sdf ? (const float*)dist : nullptr, dist, tri);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_hausdorff(const float* a, long long na, const float* b, long long nb, float* nearest, float* out2, void* stream) {
  ISHAP_REQUIRE(a && b && nearest && out2 && na > 0 && nb > 0, "hausdorff arguments");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(nearest_sq_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, s, a, na, b, nb, nearest);
  hipLaunchKernelGGL(nearest_sq_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, b, nb, a, na, nearest + na);
  hipLaunchKernelGGL(max2_kernel, dim3(1), dim3(1024), 0, s, nearest, na, nb, out2);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_group_field_stats(const float* fa, const float* fb, int groups, long long per_group, int occupancy, float* out,
                                       void* stream) {
  ISHAP_REQUIRE(fa && fb && out && groups > 0 && per_group > 0, "group_field_stats arguments");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(group_stats_kernel, dim3((unsigned)groups), dim3(256), 0, s, fa, fb, per_group, groups, occupancy ? 1 : 0, out);
  hipLaunchKernelGGL(group_mean_kernel, dim3(1), dim3(64), 0, s, groups, out);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
