// Level-set surface of the decoder's field on a FINE grid (R nodes per axis, 9 <= R <= 2048) without the dense R^3 volume: only
// bricks of 8^3 cells near the surface are decoded and cut (include/ishap.h, "Sparse high-resolution surface", states the scheme).
//   seed    : byte map [nb^3] of the bricks that overlap a crossing cell of a coarse dense volume (or any map the caller fills)
//   compact : map -> ascending list of brick ids + int32 slot map (scan.h)
//   decode  : csrc/decode.hip, values[slot][9][9][9]
//   grow    : one workgroup per active brick floods "reached" bits over the crossing edges among its samples, through the marching-
//             cubes triangles of its cells (three edges of one triangle are reached together); a seeded brick reaches every edge
//             its cells cut.  A newly reached edge is recorded with the brick that OWNS it and the bricks of the up-to-4 cells around
//             it are marked active.  The host repeats (compact the new bricks, decode them, grow) until a round changes nothing.
//   count / emit : marching cubes over (brick ascending, owned node x-slowest, axis x, y, z) for the reached edges and over
//             (brick, owned cell) for the triangles whose edges are reached.
// So the mesh is exactly the connected components (triangles joined through shared vertices) of the dense-at-R marching-cubes
// surface that cut a cell of a seeded brick -- a foreign component that merely passes through a brick the growth activated is
// not emitted.  Integer atomics (or / add) only: the reached sets are a least fixed point, the same whatever the order.
#include "common.h"
#include "scan.h"
#include "surface_rules.h"

namespace {
#include "mc_table.h"        // the same tables csrc/surface.hip cuts with; internal linkage here (one copy per code object)

constexpr int BN = 9, BNODES = BN * BN * BN;      // samples of a brick
constexpr int SS_THREADS = 256, SS_ITEMS = 3;     // 256 * 3 >= 729: a thread owns sample nodes 3 t .. 3 t + 2 (x-slowest order)
constexpr int REACH_WORDS = 184;                  // bytes [736 >= 729] per brick: bit a of byte n = the edge leaving node n along axis a is reached
constexpr int INFO_STRIDE = 736;                  // uint16 per sample node: (vertex offset within the brick) << 3 | reached owned edges

struct SparseArgs {
  const float* values;        // [n][9][9][9] by slot
  const int* list;            // the launch's brick ids, one workgroup each
  const int* slot;            // [nb^3] brick id -> slot, -1 inactive
  unsigned char* map;         // [nb^3] 0 inactive, 1 seeded, 2 grown
  unsigned* reach;            // [n][REACH_WORDS] by slot
  int R, nb;
  float level;
  unsigned short* info;       // [n][INFO_STRIDE] by slot
  unsigned* cntv;             // [n] in list order: vertices of the brick -> exclusive prefix after the scan
  unsigned* cntt;             // [n] triangles likewise
  unsigned* vbase;            // [n] by slot: index of the brick's first vertex
};

struct BrickPos { int id, s, bx, by, bz; };

__device__ __forceinline__ BrickPos brick_pos(const SparseArgs& a, int k) {
  BrickPos b;
  b.id = a.list[k];
  b.s = a.slot[b.id];
  b.bz = b.id % a.nb; b.by = (b.id / a.nb) % a.nb; b.bx = b.id / (a.nb * a.nb);
  return b;
}
__device__ __forceinline__ void node_local(int n, int& lx, int& ly, int& lz) { lz = n % BN; ly = (n / BN) % BN; lx = n / (BN * BN); }

// The brick that owns sample node (lx, ly, lz) of brick b and the node's index there: local index 8 belongs to the next brick
// (as its 0) except in the last brick of an axis, which keeps it (R - 1 = 8 nb: the grid's last node plane).
__device__ __forceinline__ int node_owner(const SparseArgs& a, const BrickPos& b, int lx, int ly, int lz, int& on) {
  const int ux = (lx == 8 && b.bx < a.nb - 1) ? 1 : 0, uy = (ly == 8 && b.by < a.nb - 1) ? 1 : 0, uz = (lz == 8 && b.bz < a.nb - 1) ? 1 : 0;
  on = ((ux ? 0 : lx) * BN + (uy ? 0 : ly)) * BN + (uz ? 0 : lz);
  return ((b.bx + ux) * a.nb + b.by + uy) * a.nb + b.bz + uz;
}
__device__ __forceinline__ int owner_slot(const SparseArgs& a, const BrickPos& b, int oid) { return oid == b.id ? b.s : a.slot[oid]; }

// the node exists on the fine grid (it is no clamped duplicate) and this brick owns it
__device__ __forceinline__ bool node_owned(const SparseArgs& a, const BrickPos& b, int lx, int ly, int lz) {
  const int m = a.R - 1;
  const bool exists = 8 * b.bx + lx <= m && 8 * b.by + ly <= m && 8 * b.bz + lz <= m;
  return exists && (lx < 8 || b.bx == a.nb - 1) && (ly < 8 || b.by == a.nb - 1) && (lz < 8 || b.bz == a.nb - 1);
}
// the cell whose lower corner is the node exists (all 8 corners are grid nodes); a brick owns the cells of local index 0..7
__device__ __forceinline__ bool cell_owned(const SparseArgs& a, const BrickPos& b, int lx, int ly, int lz) {
  const int m = a.R - 1;
  return lx < 8 && ly < 8 && lz < 8 && 8 * b.bx + lx + 1 <= m && 8 * b.by + ly + 1 <= m && 8 * b.bz + lz + 1 <= m;
}

// The brick's samples and the reached bits of every edge among them (a byte per edge: stores of 1 race benignly) into LDS.
// r0[i]: the reached byte of the thread's i-th node as loaded.
__device__ __forceinline__ void load_brick(const SparseArgs& a, const BrickPos& b, float* sv, unsigned char* sr, unsigned (&r0)[SS_ITEMS]) {
  const unsigned char* reach = reinterpret_cast<const unsigned char*>(a.reach);
#pragma unroll
  for (int i = 0; i < SS_ITEMS; ++i) {
    const int n = (int)threadIdx.x * SS_ITEMS + i;
    r0[i] = 0;
    if (n >= BNODES) continue;
    sv[n] = a.values[(long long)b.s * BNODES + n];
    int lx, ly, lz, on;
    node_local(n, lx, ly, lz);
    const int os = owner_slot(a, b, node_owner(a, b, lx, ly, lz, on));
    const unsigned byte = os >= 0 ? reach[(long long)os * (REACH_WORDS * 4) + on] : 0u;
    r0[i] = byte;
    sr[3 * n + 0] = byte & 1u; sr[3 * n + 1] = (byte >> 1) & 1u; sr[3 * n + 2] = (byte >> 2) & 1u;
  }
  __syncthreads();
}

// inside bits of the cell at sample node n (all corners are samples of the brick), 0 where the brick owns no such cell
__device__ __forceinline__ unsigned cell_bits(const SparseArgs& a, const BrickPos& b, const float* sv, int n) {
  if (n >= BNODES) return 0u;
  int lx, ly, lz;
  node_local(n, lx, ly, lz);
  if (!cell_owned(a, b, lx, ly, lz)) return 0u;
  unsigned bits = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    bits |= (surf_inside(sv[n + ((c & 1) * BN + ((c >> 1) & 1)) * BN + ((c >> 2) & 1)], a.level) ? 1u : 0u) << c;
  return bits;
}
// index into the LDS reached bytes of cube edge e of the cell at node n
__device__ __forceinline__ int edge_index(int n, int e) {
  const int lo = c_mc_edge_lo[e];
  return 3 * (n + ((lo & 1) * BN + ((lo >> 1) & 1)) * BN + ((lo >> 2) & 1)) + (e >> 2);
}

__global__ __launch_bounds__(SS_THREADS) void sparse_grow_kernel(SparseArgs a, unsigned* __restrict__ changed) {
  __shared__ float sv[BNODES];
  __shared__ unsigned char sr[3 * BNODES + 1];
  BrickPos b = brick_pos(a, blockIdx.x);
  unsigned r0[SS_ITEMS];
  load_brick(a, b, sv, sr, r0);
  const bool seeded = a.map[b.id] == 1;
  unsigned bits[SS_ITEMS];
#pragma unroll
  for (int i = 0; i < SS_ITEMS; ++i) bits[i] = cell_bits(a, b, sv, (int)threadIdx.x * SS_ITEMS + i);
  // least fixed point inside the brick: the three edges of a triangle are reached together
  for (;;) {
    int ch = 0;
#pragma unroll
    for (int i = 0; i < SS_ITEMS; ++i) {
      const int n = (int)threadIdx.x * SS_ITEMS + i;
      const int ntri = c_mc_ntri[bits[i]];
      for (int tr = 0; tr < ntri; ++tr) {
        const int k0 = edge_index(n, c_mc_tri[bits[i]][3 * tr]), k1 = edge_index(n, c_mc_tri[bits[i]][3 * tr + 1]);
        const int k2 = edge_index(n, c_mc_tri[bits[i]][3 * tr + 2]);
        const unsigned any = sr[k0] | sr[k1] | sr[k2], all = sr[k0] & sr[k1] & sr[k2];
        if ((seeded || any) && !all) { sr[k0] = 1; sr[k1] = 1; sr[k2] = 1; ch = 1; }
      }
    }
    if (!__syncthreads_or(ch)) break;
  }
  // record the newly reached edges with their owners and activate the bricks of the cells around them
  unsigned cnt = 0;
  const int m = a.R - 1;
#pragma unroll
  for (int i = 0; i < SS_ITEMS; ++i) {
    const int n = (int)threadIdx.x * SS_ITEMS + i;
    if (n >= BNODES) continue;
    const unsigned now = (unsigned)sr[3 * n] | ((unsigned)sr[3 * n + 1] << 1) | ((unsigned)sr[3 * n + 2] << 2);
    const unsigned fresh = now & ~r0[i];
    if (!fresh) continue;
    int lx, ly, lz, on;
    node_local(n, lx, ly, lz);
    const int os = owner_slot(a, b, node_owner(a, b, lx, ly, lz, on));
    if (os >= 0) {
      const unsigned word = fresh << (8 * (on & 3));
      const unsigned old = atomicOr(a.reach + (long long)os * REACH_WORDS + (on >> 2), word);
      cnt += __popc(word & ~old);
    } else {
      cnt += __popc(fresh);          // the owner is activated below; the edge is recorded in a later round
    }
    const int g[3] = {8 * b.bx + lx, 8 * b.by + ly, 8 * b.bz + lz};
    for (int ax = 0; ax < 3; ++ax) {
      if (!((fresh >> ax) & 1u)) continue;
      const int p = (ax + 1) % 3, q = (ax + 2) % 3;
      for (int w = 0; w < 4; ++w) {
        int c[3] = {g[0], g[1], g[2]};
        c[p] -= w & 1; c[q] -= w >> 1;
        if (c[0] < 0 || c[1] < 0 || c[2] < 0 || c[0] >= m || c[1] >= m || c[2] >= m) continue;     // cells outside the grid do not exist
        const int cid = ((c[0] >> 3) * a.nb + (c[1] >> 3)) * a.nb + (c[2] >> 3);
        if (a.map[cid] == 0) a.map[cid] = 2;
      }
    }
  }
  if (cnt) atomicAdd(changed, cnt);
}

__global__ __launch_bounds__(SS_THREADS) void sparse_count_kernel(SparseArgs a) {
  __shared__ float sv[BNODES];
  __shared__ unsigned char sr[3 * BNODES + 1];
  __shared__ unsigned lds[16];
  BrickPos b = brick_pos(a, blockIdx.x);
  unsigned r0[SS_ITEMS];
  load_brick(a, b, sv, sr, r0);
  unsigned mask[SS_ITEMS], nv = 0, nt = 0;
#pragma unroll
  for (int i = 0; i < SS_ITEMS; ++i) {
    const int n = (int)threadIdx.x * SS_ITEMS + i;
    mask[i] = 0;
    if (n >= BNODES) continue;
    int lx, ly, lz;
    node_local(n, lx, ly, lz);
    if (node_owned(a, b, lx, ly, lz)) mask[i] = r0[i] & 7u;
    nv += __popc(mask[i]);
    const unsigned bits = cell_bits(a, b, sv, n);
    const int ntri = c_mc_ntri[bits];
    for (int tr = 0; tr < ntri; ++tr) nt += sr[edge_index(n, c_mc_tri[bits][3 * tr])];
  }
  unsigned total_v, total_t;
  unsigned off = block_exclusive_scan(nv, lds, total_v);
  block_exclusive_scan(nt, lds, total_t);
#pragma unroll
  for (int i = 0; i < SS_ITEMS; ++i) {
    const int n = (int)threadIdx.x * SS_ITEMS + i;
    if (n >= BNODES) continue;
    a.info[(long long)b.s * INFO_STRIDE + n] = (unsigned short)((off << 3) | mask[i]);
    off += __popc(mask[i]);
  }
  if (threadIdx.x == 0) { a.cntv[blockIdx.x] = total_v; a.cntt[blockIdx.x] = total_t; }
}

__global__ __launch_bounds__(SS_THREADS) void sparse_emit_vertices_kernel(SparseArgs a, float* __restrict__ verts) {
  BrickPos b = brick_pos(a, blockIdx.x);
  const unsigned base = a.cntv[blockIdx.x];
  if (threadIdx.x == 0) a.vbase[b.s] = base;
  const float* val = a.values + (long long)b.s * BNODES;
#pragma unroll
  for (int i = 0; i < SS_ITEMS; ++i) {
    const int n = (int)threadIdx.x * SS_ITEMS + i;
    if (n >= BNODES) continue;
    const unsigned inf = a.info[(long long)b.s * INFO_STRIDE + n];
    if (!(inf & 7u)) continue;
    int lx, ly, lz;
    node_local(n, lx, ly, lz);
    long long idx = (long long)base + (inf >> 3);
    const float va = val[n] - a.level;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
      if (!((inf >> ax) & 1u)) continue;
      const int dx = ax == 0, dy = ax == 1, dz = ax == 2;
      const float vb = val[n + (dx * BN + dy) * BN + dz] - a.level;
      surf_edge_vertex(verts + 3 * idx, 8 * b.bx + lx, 8 * b.by + ly, 8 * b.bz + lz, dx, dy, dz, surf_edge_t(va, vb));
      ++idx;
    }
  }
}

__global__ __launch_bounds__(SS_THREADS) void sparse_emit_triangles_kernel(SparseArgs a, int* __restrict__ tris) {
  __shared__ float sv[BNODES];
  __shared__ unsigned char sr[3 * BNODES + 1];
  __shared__ unsigned lds[16];
  BrickPos b = brick_pos(a, blockIdx.x);
  unsigned r0[SS_ITEMS];
  load_brick(a, b, sv, sr, r0);
  unsigned bits[SS_ITEMS], nt = 0;
#pragma unroll
  for (int i = 0; i < SS_ITEMS; ++i) {
    const int n = (int)threadIdx.x * SS_ITEMS + i;
    bits[i] = cell_bits(a, b, sv, n);
    const int ntri = c_mc_ntri[bits[i]];
    for (int tr = 0; tr < ntri; ++tr) nt += sr[edge_index(n, c_mc_tri[bits[i]][3 * tr])];
  }
  unsigned total;
  long long idx = (long long)a.cntt[blockIdx.x] + block_exclusive_scan(nt, lds, total);
#pragma unroll
  for (int i = 0; i < SS_ITEMS; ++i) {
    const int n = (int)threadIdx.x * SS_ITEMS + i;
    const int ntri = c_mc_ntri[bits[i]];
    for (int tr = 0; tr < ntri; ++tr) {
      if (!sr[edge_index(n, c_mc_tri[bits[i]][3 * tr])]) continue;
      for (int c = 0; c < 3; ++c) {
        // a table entry names a cube edge = (lower corner, axis): its vertex is owned by that corner's node, in that node's brick
        const int e = c_mc_tri[bits[i]][3 * tr + c];
        const int lo = c_mc_edge_lo[e], ax = e >> 2;
        int lx, ly, lz, on;
        node_local(n, lx, ly, lz);
        const int os = owner_slot(a, b, node_owner(a, b, lx + (lo & 1), ly + ((lo >> 1) & 1), lz + ((lo >> 2) & 1), on));
        int v = 0;
        if (os >= 0) {     // closure: the owner of a reached edge is active
          const unsigned inf = a.info[(long long)os * INFO_STRIDE + on];
          v = (int)(a.vbase[os] + (inf >> 3) + __popc(inf & ((1u << ax) - 1u)));
        }
        tris[3 * idx + c] = v;
      }
      ++idx;
    }
  }
}

// ---- seeds: the bricks that overlap a crossing cell of a coarse dense volume ----
// Per axis, the bricks first .. last whose extent [8 b, min(8 b + 8, R - 1)] / (R - 1) meets coarse cell j's extent
// [j, j + 1] / (Rc - 1), end points included: 8 b (Rc - 1) <= (j + 1)(R - 1) and min(8 b + 8, R - 1)(Rc - 1) >= j (R - 1).
// Integers only (products below 2^25); for the last brick the second condition always holds.
__host__ __device__ inline void sparse_seed_range(int Rc, int R, int j, int& first, int& last) {
  const long long m = R - 1, mc = Rc - 1, nb = (m + 7) / 8;
  long long hi = ((long long)(j + 1) * m) / (8 * mc);
  if (hi > nb - 1) hi = nb - 1;
  long long lo = ((long long)j * m + 8 * mc - 1) / (8 * mc) - 1;
  if (lo < 0) lo = 0;
  first = (int)lo; last = (int)hi;
}

__global__ void sparse_seed_kernel(const float* __restrict__ coarse, int Rc, float level, int R, int nb, unsigned char* __restrict__ map) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int mc = Rc - 1;
  if (i >= (long long)mc * mc * mc) return;
  const int jz = (int)(i % mc), jy = (int)((i / mc) % mc), jx = (int)(i / ((long long)mc * mc));
  const long long p = ((long long)jx * Rc + jy) * Rc + jz;
  unsigned bits = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c)
    bits |= (surf_inside(coarse[p + ((long long)(c & 1) * Rc + ((c >> 1) & 1)) * Rc + ((c >> 2) & 1)], level) ? 1u : 0u) << c;
  if (bits == 0u || bits == 255u) return;
  int x0, x1, y0, y1, z0, z1;
  sparse_seed_range(Rc, R, jx, x0, x1);
  sparse_seed_range(Rc, R, jy, y0, y1);
  sparse_seed_range(Rc, R, jz, z0, z1);
  for (int x = x0; x <= x1; ++x)
    for (int y = y0; y <= y1; ++y)
      for (int z = z0; z <= z1; ++z) map[((long long)x * nb + y) * nb + z] = 1;
}

// ---- compaction: map -> ascending list (+ slots) ----
// mode 0: every marked brick, slot = rank, -1 written for the others; 1: the marked bricks without a slot, slot = first + rank;
// 2: every marked brick, the slot map is left alone
__global__ void sparse_flag_kernel(const unsigned char* __restrict__ map, const int* __restrict__ slot, long long n, int mode,
                                   unsigned* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = (map[i] != 0 && (mode != 1 || slot[i] < 0)) ? 1u : 0u;
}
__global__ void sparse_scatter_kernel(const unsigned char* __restrict__ map, int* __restrict__ slot, long long n, int mode, int first,
                                      const unsigned* __restrict__ rank, int* __restrict__ list, long long cap) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool sel = map[i] != 0 && (mode != 1 || slot[i] < 0);
  if (sel && (long long)rank[i] < cap) list[rank[i]] = (int)i;
  if (mode == 0) slot[i] = sel ? (int)rank[i] : -1;
  if (mode == 1 && sel) slot[i] = first + (int)rank[i];
}

bool sizes_ok(int R) { return R >= 9 && R <= 2048; }
int bricks_per_axis(int R) { return (R - 1 + 7) / 8; }

struct EmitLayout { unsigned short* info; unsigned *cntv, *cntt, *vbase, *totals; long long bytes; };
EmitLayout emit_layout(void* base, long long n) {
  Carve c{(char*)base};
  return {c.take<unsigned short>(INFO_STRIDE * n), c.take<unsigned>(n), c.take<unsigned>(n), c.take<unsigned>(n),
          c.take<unsigned>(scan_u32_blocks(n > 0 ? n : 1) + 1), c.total()};
}
// flag[n] | block totals of its scan, n = bricks_per_axis(R)^3
struct CompactLayout { long long n; unsigned *flag, *totals; long long bytes; };
CompactLayout compact_layout(void* base, int R) {
  Carve c{(char*)base};
  const long long nb = bricks_per_axis(R), n = nb * nb * nb;
  return {n, c.take<unsigned>(n), c.take<unsigned>(scan_u32_blocks(n) + 1), c.total()};
}

int fill(SparseArgs& a, const float* values, const int* list, long long n, int R, float level, const int* slot, unsigned* reach) {
  ISHAP_REQUIRE(sizes_ok(R), "sparse surface: 9 <= R <= 2048");
  ISHAP_REQUIRE(values && list && slot && reach, "sparse surface: null argument");
  ISHAP_REQUIRE(n >= 1 && n <= (1ll << 21), "sparse surface: 1 <= bricks <= 2^21");
  a.values = values; a.list = list; a.slot = slot; a.map = nullptr; a.reach = reach; a.R = R; a.nb = bricks_per_axis(R); a.level = level;
  a.info = nullptr; a.cntv = a.cntt = a.vbase = nullptr;
  return 0;
}
int fill_emit(SparseArgs& a, void* scratch, long long scratch_bytes, long long n, unsigned** totals = nullptr) {
  const EmitLayout L = emit_layout(scratch, n);
  ISHAP_REQUIRE(scratch, "sparse surface: null scratch");
  ISHAP_REQUIRE(scratch_bytes >= L.bytes, "sparse surface: scratch smaller than ishap_sparse_surface_scratch_bytes(R, bricks)");
  ISHAP_REQUIRE(((uintptr_t)scratch & 15) == 0, "sparse surface: scratch must be 16-byte aligned");
  a.info = L.info; a.cntv = L.cntv; a.cntt = L.cntt; a.vbase = L.vbase;
  if (totals) *totals = L.totals;
  return 0;
}

}  // namespace

extern "C" int ishap_sparse_bricks_per_axis(int R) { return sizes_ok(R) ? bricks_per_axis(R) : -1; }

extern "C" int ishap_sparse_seed_range(int Rc, int R, int j, int* first, int* last) {
  ISHAP_REQUIRE(sizes_ok(R) && Rc >= 2 && Rc <= 2048, "sparse seed: 9 <= R <= 2048, 2 <= Rc <= 2048");
  ISHAP_REQUIRE(first && last && j >= 0 && j < Rc - 1, "sparse seed: null argument / coarse cell outside 0 .. Rc - 2");
  sparse_seed_range(Rc, R, j, *first, *last);
  return 0;
}

extern "C" int ishap_sparse_seed_volume(const float* coarse, int Rc, float level, int R, unsigned char* map, void* stream) {
  ISHAP_REQUIRE(sizes_ok(R) && Rc >= 2 && Rc <= 2048, "sparse seed: 9 <= R <= 2048, 2 <= Rc <= 2048");
  ISHAP_REQUIRE(coarse && map, "sparse seed: null argument");
  // one thread stores the brick box of its coarse cell: at most (64 / 8 + 2)^3 bytes within this bound
  ISHAP_REQUIRE(R - 1 <= 64 * (Rc - 1), "sparse seed: the coarse volume is too coarse for this grid, R - 1 <= 64 (Rc - 1)");
  const long long cells = (long long)(Rc - 1) * (Rc - 1) * (Rc - 1);
  hipLaunchKernelGGL(sparse_seed_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, coarse, Rc, level, R,
                     bricks_per_axis(R), map);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" long long ishap_sparse_compact_scratch_bytes(int R) {
  if (!sizes_ok(R)) return -1;
  return compact_layout(nullptr, R).bytes;
}

extern "C" int ishap_sparse_compact(const unsigned char* map, int R, int mode, int first_slot, int* slot_map, int* list,
                                    long long list_capacity, unsigned* count, void* scratch, long long scratch_bytes, void* stream) {
  ISHAP_REQUIRE(sizes_ok(R), "sparse compact: 9 <= R <= 2048");
  ISHAP_REQUIRE(map && slot_map && list && count && scratch, "sparse compact: null argument");
  ISHAP_REQUIRE(mode >= 0 && mode <= 2 && first_slot >= 0 && list_capacity >= 0, "sparse compact: mode 0..2, first_slot >= 0, capacity >= 0");
  ISHAP_REQUIRE(scratch_bytes >= ishap_sparse_compact_scratch_bytes(R), "sparse compact: scratch smaller than ishap_sparse_compact_scratch_bytes(R)");
  ISHAP_REQUIRE(((uintptr_t)scratch & 15) == 0, "sparse compact: scratch must be 16-byte aligned");
  const CompactLayout L = compact_layout(scratch, R);
  const long long n = L.n;
  unsigned *flag = L.flag, *totals = L.totals;
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(sparse_flag_kernel, dim3(blocks), dim3(256), 0, s, map, (const int*)slot_map, n, mode, flag);
  scan_exclusive_u32(flag, n, totals, count, s);
  hipLaunchKernelGGL(sparse_scatter_kernel, dim3(blocks), dim3(256), 0, s, map, slot_map, n, mode, first_slot, (const unsigned*)flag, list,
                     list_capacity);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_sparse_grow(const float* values, const int* list, long long nbricks, int R, float level, unsigned char* map,
                                 const int* slot_map, unsigned* reach, unsigned* changed, void* stream) {
  SparseArgs a;
  ISHAP_TRY(fill(a, values, list, nbricks, R, level, slot_map, reach));
  ISHAP_REQUIRE(map && changed, "sparse grow: null argument");
  a.map = map;
  hipLaunchKernelGGL(sparse_grow_kernel, dim3((unsigned)nbricks), dim3(SS_THREADS), 0, (hipStream_t)stream, a, changed);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" long long ishap_sparse_surface_scratch_bytes(int R, long long nbricks) {
  if (!sizes_ok(R) || nbricks < 0 || nbricks > (1ll << 21)) return -1;
  return emit_layout(nullptr, nbricks).bytes;
}
extern "C" long long ishap_sparse_reach_bytes(long long nbricks) { return nbricks < 0 ? -1 : nbricks * REACH_WORDS * 4; }

extern "C" int ishap_sparse_surface_count(const float* values, const int* ordered, long long nbricks, int R, float level,
                                          const int* slot_map, unsigned* reach, void* scratch, long long scratch_bytes,
                                          unsigned* counts, void* stream) {
  SparseArgs a;
  ISHAP_TRY(fill(a, values, ordered, nbricks, R, level, slot_map, reach));
  ISHAP_REQUIRE(counts, "sparse surface: null argument");
  unsigned* totals;
  ISHAP_TRY(fill_emit(a, scratch, scratch_bytes, nbricks, &totals));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sparse_count_kernel, dim3((unsigned)nbricks), dim3(SS_THREADS), 0, s, a);
  scan_exclusive_u32(a.cntv, nbricks, totals, counts, s);
  scan_exclusive_u32(a.cntt, nbricks, totals, counts + 1, s);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_sparse_surface_emit(const float* values, const int* ordered, long long nbricks, int R, float level,
                                         const int* slot_map, unsigned* reach, void* scratch, long long scratch_bytes, float* verts,
                                         int* tris, void* stream) {
  SparseArgs a;
  ISHAP_TRY(fill(a, values, ordered, nbricks, R, level, slot_map, reach));
  ISHAP_REQUIRE(verts && tris, "sparse surface: null argument");
  ISHAP_TRY(fill_emit(a, scratch, scratch_bytes, nbricks));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sparse_emit_vertices_kernel, dim3((unsigned)nbricks), dim3(SS_THREADS), 0, s, a, verts);
  hipLaunchKernelGGL(sparse_emit_triangles_kernel, dim3((unsigned)nbricks), dim3(SS_THREADS), 0, s, a, tris);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
