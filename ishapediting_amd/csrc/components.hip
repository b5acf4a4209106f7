// Connected components of a voxel volume, on the device: labels, a table of the components, and the flip that removes
// floaters / fills cavities (ishapediting_amd/volume.py).  The reference leaves this to the user's mesh tool.
//
// A voxel is INSIDE where vol[p] - level > 0.f (surface.hip's corner_bits expression: a NaN is outside), OUTSIDE otherwise;
// p = (x*ny + y)*nz + z.  One phase is labelled per call; two voxels of that phase are joined when they are face neighbours
// (connectivity 6) or face / edge / corner neighbours (26).  Every labelled voxel gets the LOWEST LINEAR INDEX of its
// component, a function of the input alone.
//
// Union-find over `labels` used as the parent array, a fixed sequence of three launches:
//   tile     a workgroup owns a CC_TX x CC_TY x CC_TZ box (z rows of 32 floats, loaded coalesced, 4 voxels per thread), joins
//            its voxels in LDS (atomicMin on LDS parents) and writes every voxel's tile root as a global index
//   seam     every voxel with a neighbour in ANOTHER tile joins itself to it in global memory: find both roots, atomicMin(
//            &parent[hi], lo), and go on with (previous parent of hi, lo) when hi was no longer a root (relaxed, agent scope)
//   flatten  every parent is replaced by its root
// Termination and correctness.  A parent is only ever written by atomicMin with the index of a voxel of the same component,
// and starts as the voxel itself or a lower voxel of its z run, so (1) parents only ever decrease and never exceed the voxel's
// own index: following parents strictly descends and ends at a root; (2) a parent always names a voxel of the same component.
// A join of (a, b) ends when both have one root, or its atomicMin found hi still a root and hung it under lo; otherwise hi had
// got a parent `old` < hi in the meantime and the join goes on with (old, lo), whose larger member is below hi: the larger
// member strictly decreases, so a join takes finitely many steps whatever the other lanes do and whatever age the values its
// loads return have -- no lane waits for another, there are no flags, tickets, grid barriers or host loops.  A link that an
// atomicMin replaces (parent[hi] was old, becomes lo < old) is re-made by that same join going on with (old, lo).  When every
// join has ended all voxels of a component hang in one tree, and by (1) its root is the component's lowest index.
// Joins that other joins imply are skipped (need_join): along z a voxel and its predecessor are joined by the run start the
// tile pass begins with (or by the z seam), so an offset (dx, dy, 0) from p is implied when p - z and its partner are both
// members, and an offset (dx, dy, +-1) when the voxel between them along z is one; a flat seam between two solid tiles costs
// one global atomic per row instead of one per voxel.
//
// The table (count / emit, as ishap_surface_count / _emit): roots are the voxels with labels[p] == p, compacted in index order
// by a scan; voxel counts and boxes are integer sums and min / max (exact, order-free).  A workgroup accumulates its tile's
// voxels per component in an LDS hash table (count, occupancy masks of the tile's x, y, z positions, border bit) and then
// issues one global atomic per field, tile and component.
#include <climits>

#include "common.h"
#include "scan.h"

namespace {

constexpr int CC_TX = 4, CC_TY = 8, CC_TZ = 32;            // the tile: 1024 voxels, z rows of 128 bytes
constexpr int CC_TV = CC_TX * CC_TY * CC_TZ;
constexpr int CC_THREADS = 256, CC_PER = CC_TV / CC_THREADS;
constexpr int CC_SLOTS = 2 * CC_TV;                        // LDS hash table of the accumulate pass (load factor <= 1/2)
constexpr int CC_ROW = 9;                                  // root, voxels, xmin, xmax, ymin, ymax, zmin, zmax, border

struct Box {
  int nx, ny, nz;
  int tby, tbz;      // tiles along y and z
};

// the forward half of the neighbourhood: (dx, dy, dz) > (0, 0, 0) in lexicographic order, 3 offsets (6) or 13 (26)
__device__ __forceinline__ bool forward_offset(int dx, int dy, int dz, int conn) {
  const bool fwd = dx == 1 || (dx == 0 && (dy == 1 || (dy == 0 && dz == 1)));
  return fwd && (conn == 26 || (dx != 0) + (dy != 0) + (dz != 0) == 1);
}

// ---- union-find on LDS parents (tile pass) ----
__device__ __forceinline__ int l_load(int* par, int i) { return __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int l_find(int* par, int x) {
  for (int p; (p = l_load(par, x)) != x;) x = p;
  return x;
}
__device__ __forceinline__ void l_join(int* par, int a, int b) {
  for (;;) {
    a = l_find(par, a);
    b = l_find(par, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = __hip_atomic_fetch_min(par + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (old == hi) return;
    a = old;
    b = lo;
  }
}
// ---- the same on the global parents (seam pass): every access an agent-scope atomic ----
__device__ __forceinline__ int g_load(int* par, int i) { return __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(int* par, int x) {
  for (int p; (p = g_load(par, x)) != x;) x = p;
  return x;
}
__device__ __forceinline__ void g_join(int* par, int a, int b) {
  for (;;) {
    a = g_find(par, a);
    b = g_find(par, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = __hip_atomic_fetch_min(par + hi, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == hi) return;
    a = old;
    b = lo;
  }
}

// Is the join of a member with its member neighbour at (dx, dy, dz) needed, or implied by other joins?  m_self(k): is the
// voxel k steps along z from the first one a member; m_nb(k): the same from the neighbour; both false where the voxel is out
// of reach (outside the tile in the tile pass, outside the box in the seam pass).
template <typename MSelf, typename MNb>
__device__ __forceinline__ bool need_join(int dz, MSelf m_self, MNb m_nb) {
  if (dz == 0) return !(m_self(-1) && m_nb(-1));     // (p - z, q - z) is joined by p - z, and each is joined to its successor
  return !(m_self(dz) || m_nb(-dz));                 // the voxel between them along z joins both
}

__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const float* __restrict__ vol, int* __restrict__ labels, Box b, float level,
                                                             int phase, int conn) {
  __shared__ int par[CC_TV];
  __shared__ unsigned char in[CC_TV];
  const int t = threadIdx.x;
  const int bz = blockIdx.x % b.tbz, by = (blockIdx.x / b.tbz) % b.tby, bx = blockIdx.x / (b.tbz * b.tby);
  const int x0 = bx * CC_TX, y0 = by * CC_TY, z0 = bz * CC_TZ;
  int gp[CC_PER];                                    // global index, -1 outside the box
#pragma unroll
  for (int i = 0; i < CC_PER; ++i) {
    const int l = i * CC_THREADS + t;                // lanes run along z: a wave loads two 128-byte rows
    const int x = x0 + (l >> 8), y = y0 + ((l >> 5) & 7), z = z0 + (l & 31);
    const bool inb = x < b.nx && y < b.ny && z < b.nz;
    gp[i] = inb ? (x * b.ny + y) * b.nz + z : -1;
    bool member = false;
    if (inb) member = (vol[gp[i]] - level > 0.f) == (phase != 0);
    in[l] = member ? 1 : 0;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CC_PER; ++i) {                 // parent = start of the voxel's z run: the z joins, without atomics
    const int l = i * CC_THREADS + t;
    int s = l;
    if (in[l])
      while ((s & 31) > 0 && in[s - 1]) --s;
    par[l] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CC_PER; ++i) {
    const int l = i * CC_THREADS + t;
    if (!in[l]) continue;
    const int lx = l >> 8, ly = (l >> 5) & 7, lz = l & 31;
    for (int dx = 0; dx <= 1; ++dx)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dz = -1; dz <= 1; ++dz) {
          if (!forward_offset(dx, dy, dz, conn) || (dx == 0 && dy == 0)) continue;
          const int qx = lx + dx, qy = ly + dy, qz = lz + dz;
          if (qx >= CC_TX || qy < 0 || qy >= CC_TY || qz < 0 || qz >= CC_TZ) continue;
          const int q = (qx * CC_TY + qy) * CC_TZ + qz;
          if (!in[q]) continue;
          auto m_self = [&](int k) { return lz + k >= 0 && lz + k < CC_TZ && in[l + k]; };
          auto m_nb = [&](int k) { return qz + k >= 0 && qz + k < CC_TZ && in[q + k]; };
          if (need_join(dz, m_self, m_nb)) l_join(par, l, q);
        }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < CC_PER; ++i) {
    if (gp[i] < 0) continue;
    const int l = i * CC_THREADS + t;
    int out = -1;
    if (in[l]) {
      const int r = l_find(par, l);                  // local and global order agree inside a tile: the lowest of both
      out = ((x0 + (r >> 8)) * b.ny + y0 + ((r >> 5) & 7)) * b.nz + z0 + (r & 31);
    }
    labels[gp[i]] = out;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_seam_kernel(int* labels, Box b, int n, int conn) {
  const long long pl = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (pl >= n) return;
  const int p = (int)pl;
  const int z = p % b.nz, y = (p / b.nz) % b.ny, x = p / (b.nz * b.ny);
  const int lx = x % CC_TX, ly = y % CC_TY, lz = z % CC_TZ;
  // only voxels on a tile face have a forward neighbour in another tile
  if (!(lx == CC_TX - 1 || ly == 0 || ly == CC_TY - 1 || lz == 0 || lz == CC_TZ - 1)) return;
  if (g_load(labels, p) < 0) return;
  for (int dx = 0; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dz = -1; dz <= 1; ++dz) {
        if (!forward_offset(dx, dy, dz, conn)) continue;
        const int qx = x + dx, qy = y + dy, qz = z + dz;
        if (qx >= b.nx || qy < 0 || qy >= b.ny || qz < 0 || qz >= b.nz) continue;
        if (qx / CC_TX == x / CC_TX && qy / CC_TY == y / CC_TY && qz / CC_TZ == z / CC_TZ) continue;   // the tile pass joined them
        const int q = (qx * b.ny + qy) * b.nz + qz;
        if (g_load(labels, q) < 0) continue;
        auto m_self = [&](int k) { return z + k >= 0 && z + k < b.nz && g_load(labels, p + k) >= 0; };
        auto m_nb = [&](int k) { return qz + k >= 0 && qz + k < b.nz && g_load(labels, q + k) >= 0; };
        if ((dx == 0 && dy == 0) || need_join(dz, m_self, m_nb)) g_join(labels, p, q);
      }
}

// labels[p] <- its root.  Other lanes replace parents by roots meanwhile: a load returns a voxel's parent or its root, both on
// the path to the same root.
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int* labels, int n) {
  const long long pl = (long long)blockIdx.x * CC_THREADS + threadIdx.x;
  if (pl >= n) return;
  const int p = (int)pl;
  int r = labels[p];
  if (r < 0) return;
  for (int q; (q = g_load(labels, r)) != r;) r = q;
  labels[p] = r;
}

// ---- table ----
// bit i: voxel i0 + i is a root
__device__ __forceinline__ unsigned root_bits(const int* __restrict__ labels, long long i0, long long n) {
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k)
    if (i0 + k < n && labels[i0 + k] == (int)(i0 + k)) m |= 1u << k;
  return m;
}
__global__ __launch_bounds__(SCAN_THREADS) void cc_count_kernel(const int* __restrict__ labels, long long n, unsigned* __restrict__ bsum) {
  __shared__ unsigned lds[16];
  const long long i0 = (long long)blockIdx.x * SCAN_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
  unsigned total;
  block_exclusive_scan(__popc(root_bits(labels, i0, n)), lds, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}
// a row per root in index order, ready for the accumulation; rank[root] = its row
__global__ __launch_bounds__(SCAN_THREADS) void cc_rows_kernel(const int* __restrict__ labels, long long n, const unsigned* __restrict__ bsum,
                                                             int* __restrict__ rank, int* __restrict__ table) {
  __shared__ unsigned lds[16];
  const long long i0 = (long long)blockIdx.x * SCAN_BLOCK + (long long)threadIdx.x * SCAN_ITEMS;
  const unsigned m = root_bits(labels, i0, n);
  unsigned total;
  unsigned row = bsum[blockIdx.x] + block_exclusive_scan(__popc(m), lds, total);
#pragma unroll
  for (int k = 0; k < SCAN_ITEMS; ++k) {
    if (!((m >> k) & 1u)) continue;
    rank[i0 + k] = (int)row;
    int* r = table + (long long)row * CC_ROW;
    r[0] = (int)(i0 + k);
    r[1] = 0;
    r[2] = r[4] = r[6] = INT_MAX;
    r[3] = r[5] = r[7] = -1;
    r[8] = 0;
    ++row;
  }
}
__global__ __launch_bounds__(CC_THREADS) void cc_accum_kernel(const int* __restrict__ labels, Box b, const int* __restrict__ rank,
                                                              int* __restrict__ table) {
  __shared__ int key[CC_SLOTS];
  __shared__ unsigned cnt[CC_SLOTS], mxy[CC_SLOTS], mz[CC_SLOTS];
  const int t = threadIdx.x;
  for (int s = t; s < CC_SLOTS; s += CC_THREADS) { key[s] = -1; cnt[s] = 0; mxy[s] = 0; mz[s] = 0; }
  __syncthreads();
  const int bz = blockIdx.x % b.tbz, by = (blockIdx.x / b.tbz) % b.tby, bx = blockIdx.x / (b.tbz * b.tby);
  const int x0 = bx * CC_TX, y0 = by * CC_TY, z0 = bz * CC_TZ;
#pragma unroll
  for (int i = 0; i < CC_PER; ++i) {
    const int l = i * CC_THREADS + t;
    const int lx = l >> 8, ly = (l >> 5) & 7, lz = l & 31;
    const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
    if (x >= b.nx || y >= b.ny || z >= b.nz) continue;
    const int r = labels[(x * b.ny + y) * b.nz + z];
    if (r < 0) continue;
    unsigned h = ((unsigned)r * 2654435761u) >> 21;          // 11 bits: CC_SLOTS = 2048
    for (;;) {                                               // at most CC_TV keys in CC_SLOTS slots: an empty slot exists
      const int k = atomicCAS(&key[h], -1, r);
      if (k == -1 || k == r) break;
      h = (h + 1) & (CC_SLOTS - 1);
    }
    const bool border = x == 0 || y == 0 || z == 0 || x == b.nx - 1 || y == b.ny - 1 || z == b.nz - 1;
    atomicAdd(&cnt[h], 1u);
    atomicOr(&mxy[h], (1u << lx) | (1u << (4 + ly)) | (border ? 1u << 12 : 0u));
    atomicOr(&mz[h], 1u << lz);
  }
  __syncthreads();
  for (int s = t; s < CC_SLOTS; s += CC_THREADS) {
    if (key[s] < 0) continue;
    int* r = table + (long long)rank[key[s]] * CC_ROW;
    const unsigned xm = mxy[s] & 15u, ym = (mxy[s] >> 4) & 255u, zm = mz[s];
    atomicAdd(r + 1, (int)cnt[s]);
    atomicMin(r + 2, x0 + __ffs(xm) - 1);
    atomicMax(r + 3, x0 + 31 - __clz(xm));
    atomicMin(r + 4, y0 + __ffs(ym) - 1);
    atomicMax(r + 5, y0 + 31 - __clz(ym));
    atomicMin(r + 6, z0 + __ffs(zm) - 1);
    atomicMax(r + 7, z0 + 31 - __clz(zm));
    if ((mxy[s] >> 12) & 1u) atomicOr(r + 8, 1);
  }
}

// ---- flip ----
__global__ __launch_bounds__(256) void cc_mark_kernel(const int* __restrict__ roots, long long nroots, int n, unsigned char* __restrict__ mark) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nroots) return;
  const int r = roots[i];
  if (r >= 0 && r < n) mark[r] = 1;
}
// vout may be vin: a lane reads and writes its own voxel only
__global__ __launch_bounds__(256) void cc_flip_kernel(const float* vin, float* vout, const int* __restrict__ labels, int n, float level,
                                                      const unsigned char* __restrict__ mark) {
  const long long pl = (long long)blockIdx.x * 256 + threadIdx.x;
  if (pl >= n) return;
  const float v = vin[pl];
  float o = v;
  const int l = labels[pl];
  if (l >= 0 && mark[l] && v == v) {
    const bool was_in = v - level > 0.f;
    o = level - (v - level);
    if (!was_in && !(o - level > 0.f)) o = nextafterf(level, INFINITY);   // v == level, or so close that the mirror image rounds to it
  }
  vout[pl] = o;
}

int fill_box(Box& b, int nx, int ny, int nz) {
  ISHAP_REQUIRE(nx > 0 && ny > 0 && nz > 0, "volume: positive extents");
  ISHAP_REQUIRE((long long)nx * ny < (1ll << 31) && (long long)nx * ny * nz < (1ll << 31), "volume: nx * ny * nz must be below 2^31");
  b.nx = nx; b.ny = ny; b.nz = nz;
  b.tby = (ny + CC_TY - 1) / CC_TY;
  b.tbz = (nz + CC_TZ - 1) / CC_TZ;
  return 0;
}
unsigned tiles(const Box& b) { return (unsigned)((b.nx + CC_TX - 1) / CC_TX) * (unsigned)b.tby * (unsigned)b.tbz; }
// scratch: rank int[n] (flip: mark bytes[n], the same bytes) | block sums, 256-byte aligned
struct CompScratch { int* rank; unsigned* bsum; long long bytes; };
CompScratch comp_scratch(void* base, long long n) {
  Carve c{(char*)base};
  return {c.take<int>(n), c.take<unsigned>(scan_u32_blocks(n)), c.total()};
}

}  // namespace

extern "C" long long ishap_volume_components_scratch_bytes(long long n) {
  if (n <= 0 || n >= (1ll << 31)) return -1;
  return comp_scratch(nullptr, n).bytes;
}

extern "C" int ishap_volume_label(const float* vol, int nx, int ny, int nz, float level, int phase, int connectivity, int* labels,
                                  void* stream) {
  Box b;
  ISHAP_TRY(fill_box(b, nx, ny, nz));
  ISHAP_REQUIRE(connectivity == 6 || connectivity == 26, "volume_label: connectivity 6 or 26");
  ISHAP_REQUIRE(phase == 0 || phase == 1, "volume_label: phase 1 (inside) or 0 (outside)");
  ISHAP_REQUIRE(vol && labels, "volume_label: null argument");
  const int n = nx * ny * nz;
  const unsigned vb = (unsigned)(((long long)n + CC_THREADS - 1) / CC_THREADS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_tile_kernel, dim3(tiles(b)), dim3(CC_THREADS), 0, s, vol, labels, b, level, phase, connectivity);
  hipLaunchKernelGGL(cc_seam_kernel, dim3(vb), dim3(CC_THREADS), 0, s, labels, b, n, connectivity);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(vb), dim3(CC_THREADS), 0, s, labels, n);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_volume_components_count(const int* labels, int nx, int ny, int nz, void* scratch, int* count, void* stream) {
  Box b;
  ISHAP_TRY(fill_box(b, nx, ny, nz));
  ISHAP_REQUIRE(labels && scratch && count, "volume_components_count: null argument");
  const long long n = (long long)nx * ny * nz, nb = scan_u32_blocks(n);
  unsigned* bsum = comp_scratch(scratch, n).bsum;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_count_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, labels, n, bsum);
  scan_block_totals(bsum, nb, (unsigned*)count, s);              // the count is below 2^31: fill_box bounds n
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_volume_components_emit(const int* labels, int nx, int ny, int nz, void* scratch, int* table, void* stream) {
  Box b;
  ISHAP_TRY(fill_box(b, nx, ny, nz));
  ISHAP_REQUIRE(labels && scratch && table, "volume_components_emit: null argument");
  const long long n = (long long)nx * ny * nz, nb = scan_u32_blocks(n);
  const CompScratch S = comp_scratch(scratch, n);
  int* rank = S.rank; const unsigned* bsum = S.bsum;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_rows_kernel, dim3((unsigned)nb), dim3(SCAN_THREADS), 0, s, labels, n, bsum, rank, table);
  hipLaunchKernelGGL(cc_accum_kernel, dim3(tiles(b)), dim3(CC_THREADS), 0, s, labels, b, (const int*)rank, table);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_volume_flip(const float* vol_in, float* vol_out, const int* labels, int nx, int ny, int nz, float level,
                                 const int* roots, long long nroots, void* scratch, void* stream) {
  Box b;
  ISHAP_TRY(fill_box(b, nx, ny, nz));
  ISHAP_REQUIRE(vol_in && vol_out && labels && scratch && nroots >= 0 && (roots || nroots == 0), "volume_flip: null argument");
  const int n = nx * ny * nz;
  hipStream_t s = (hipStream_t)stream;
  unsigned char* mark = (unsigned char*)comp_scratch(scratch, n).rank;
  ISHAP_CHECK_HIP(hipMemsetAsync(mark, 0, (size_t)n, s));
  if (nroots > 0)
    hipLaunchKernelGGL(cc_mark_kernel, dim3((unsigned)((nroots + 255) / 256)), dim3(256), 0, s, roots, nroots, n, mark);
  hipLaunchKernelGGL(cc_flip_kernel, dim3((unsigned)(((long long)n + 255) / 256)), dim3(256), 0, s, vol_in, vol_out, labels, n, level,
                     (const unsigned char*)mark);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
