// Quadric vertex clustering on the device (Open3D's simplify_vertex_clustering, contraction Quadric / Average), the rule as
// include/ishap.h states it ("Mesh simplification") and tests/simplify_ref.py restates it in float64 numpy.
//   count: cell bitmap (atomicOr) -> popcount per word -> scan = cluster ranks; per-cluster sums as 64-bit INTEGER atomics into
//          one 128-byte row per cluster (the arithmetic once per item, then sixteen neighbouring lanes per contribution);
//          triangles deduplicated through an open-addressing table of triangle indices (CAS, then atomicMin among equal
//          keys); survivors and referenced clusters flagged and scanned; the overflow guard checked.
//   emit:  representatives solved from the integer sums, triangles compacted in input order, the vertex map.
// Every value that crosses threads is an integer (sums, minima, or-ed bits), so the result depends on the input alone.
// No fused multiply-add in this file: the float64 expressions are the reference's, operation for operation.
#include "simplify.h"
#include "../../include/ishap.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;
constexpr int SM_THREADS = 256;

// cell c, unclamped grid coordinate q and clamped local coordinate p of one axis
__device__ __forceinline__ void axis_cell(float v, double lo, double h, int g, double& q, int& c, double& p) {
  q = ((double)v - lo) / h;
  double t = floor(q);
  if (t != t) t = 0.0;
  t = fmin(fmax(t, 0.0), (double)(g - 1));
  c = (int)t;
  p = q - ((double)c + 0.5);
  if (p != p) p = 0.0;
  p = fmin(fmax(p, -0.5), 0.5);
}
struct Local {
  double qx, qy, qz, px, py, pz;
  int cx, cy, cz, cell;
};
__device__ __forceinline__ Local locate(const SimplifyGrid& G, const float* __restrict__ verts, long long i) {
  Local a;
  axis_cell(verts[3 * i + 0], G.lo[0], G.h, G.g[0], a.qx, a.cx, a.px);
  axis_cell(verts[3 * i + 1], G.lo[1], G.h, G.g[1], a.qy, a.cy, a.py);
  axis_cell(verts[3 * i + 2], G.lo[2], G.h, G.g[2], a.qz, a.cz, a.pz);
  a.cell = (a.cx * G.g[1] + a.cy) * G.g[2] + a.cz;       // < 2^30
  return a;
}
__device__ __forceinline__ void add_u64(u64* p, long long v) {
  __hip_atomic_fetch_add(p, (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // result unused: the no-return form
}

__global__ __launch_bounds__(SM_THREADS) void simplify_mark_kernel(const float* __restrict__ verts, long long nverts, SimplifyGrid G,
                                                                   unsigned* __restrict__ bitmap) {
  const long long i = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= nverts) return;
  const int cell = locate(G, verts, i).cell;
  atomicOr(bitmap + (cell >> 5), 1u << (cell & 31));
}

__global__ __launch_bounds__(SM_THREADS) void simplify_popc_kernel(const unsigned* __restrict__ bitmap, long long words,
                                                                   unsigned* __restrict__ prefix) {
  const long long i = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i < words) prefix[i] = (unsigned)__popc(bitmap[i]);
}

// rows of the clusters there are (hdr[0], known on the device only): zero, the minimum slot all ones
__global__ __launch_bounds__(SM_THREADS) void simplify_clear_rows_kernel(const int* __restrict__ hdr, u64* __restrict__ rows) {
  const long long n = (long long)hdr[0] * SIMPLIFY_ROW;
  for (long long i = (long long)blockIdx.x * SM_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * SM_THREADS)
    rows[i] = (i & (SIMPLIFY_ROW - 1)) == SIMPLIFY_SLOT_MIN ? ~0ull : 0ull;
}

// Both accumulation kernels work in two phases.  Phase 1, one thread per item (vertex / triangle): the float64 arithmetic, once,
// its integer results into LDS.  Phase 2, sixteen neighbouring lanes per item, lane j owning slot j of the cluster's row: each
// group walks the sixteen items its own lanes wrote and issues their atomics, one 128-byte row segment per group and instruction.
// Records are 10 / 42 dwords: 16 records further on (the next group's item of the same step) lie 32 banks away.
constexpr int VREC = 10;      // dwords per vertex: rint(p 2^32) x 3 as i64, the cluster, padding
constexpr int TREC = 42;      // dwords per triangle: 19 i64 (below), the three clusters (the first < 0: nothing to add), padding

__global__ __launch_bounds__(SM_THREADS) void simplify_vertex_sums_kernel(const float* __restrict__ verts, long long nverts, SimplifyGrid G,
                                                                          const unsigned* __restrict__ bitmap,
                                                                          const unsigned* __restrict__ prefix, int* __restrict__ vcluster,
                                                                          u64* __restrict__ rows) {
  __shared__ __attribute__((aligned(8))) unsigned sh[SM_THREADS * VREC];
  const long long first = (long long)blockIdx.x * SM_THREADS;
  {
    const long long i = first + threadIdx.x;
    unsigned* rec = sh + threadIdx.x * VREC;
    int cluster = -1;
    if (i < nverts) {
      const Local a = locate(G, verts, i);
      const int w = a.cell >> 5;
      cluster = (int)(prefix[w] + (unsigned)__popc(bitmap[w] & ((1u << (a.cell & 31)) - 1u)));
      vcluster[i] = cluster;
      long long* val = reinterpret_cast<long long*>(rec);
      val[0] = __double2ll_rn(a.px * SIMPLIFY_P_SCALE);
      val[1] = __double2ll_rn(a.py * SIMPLIFY_P_SCALE);
      val[2] = __double2ll_rn(a.pz * SIMPLIFY_P_SCALE);
    }
    rec[6] = (unsigned)cluster;
  }
  __syncthreads();
  const int j = threadIdx.x & 15, g16 = threadIdx.x & ~15;
  if (j > SIMPLIFY_SLOT_MIN) return;
  // consecutive vertices of one cluster (the extractors emit cell by cell) are summed and leave as ONE row of atomics
  int cur = -1;
  long long acc = 0;
  auto flush = [&]() {
    if (cur < 0) return;
    u64* slot = rows + (long long)cur * SIMPLIFY_ROW + j;
    if (j == SIMPLIFY_SLOT_MIN) __hip_atomic_fetch_min(slot, (u64)acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else add_u64(slot, acc);
  };
  for (int s = 0; s < 16; ++s) {
    const unsigned* rec = sh + (g16 + s) * VREC;
    const int cluster = (int)rec[6];
    if (cluster < 0) break;                                 // past the last vertex
    // lane 0: one vertex more; lanes 1..3: its p; lane 4: its index (a run's lowest is its first)
    const long long v = j == SIMPLIFY_SLOT_COUNT ? 1 : j < SIMPLIFY_SLOT_MIN ? reinterpret_cast<const long long*>(rec)[j - SIMPLIFY_SLOT_P]
                                                                              : first + g16 + s;
    if (cluster == cur) {
      if (j != SIMPLIFY_SLOT_MIN) acc += v;
    } else {
      flush();
      cur = cluster;
      acc = v;
    }
  }
  flush();
}

// A triangle's 19 values: [0..5] w n n^T (slots 5..10) and [6] the guard (slot 15), the same for its three corners;
// [7 + 4 k .. 10 + 4 k] w n d, w d d with corner k's d (slots 11..14).  Whatever reaches one cluster in a row -- the corners of
// a triangle, then the triangles a group walks one after the other (the extractors emit cell by cell) -- is summed before the
// atomic (integer adds commute: not a bit changes).
__global__ __launch_bounds__(SM_THREADS) void simplify_quadric_sums_kernel(const float* __restrict__ verts, long long nverts,
                                                                           const int* __restrict__ tris, long long ntris, SimplifyGrid G,
                                                                           const int* __restrict__ vcluster, u64* __restrict__ rows) {
  __shared__ __attribute__((aligned(8))) unsigned sh[SM_THREADS * TREC];
  {
    const long long t = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    unsigned* rec = sh + threadIdx.x * TREC;
    long long* val = reinterpret_cast<long long*>(rec);
    int c0 = -1, c1 = -1, c2 = -1;
    if (t < ntris) {
      const long long i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
      if (i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < nverts && i1 < nverts && i2 < nverts) {
        const Local a = locate(G, verts, i0), b = locate(G, verts, i1), c = locate(G, verts, i2);
        const double ux = b.qx - a.qx, uy = b.qy - a.qy, uz = b.qz - a.qz;
        const double vx = c.qx - a.qx, vy = c.qy - a.qy, vz = c.qz - a.qz;
        const double Nx = uy * vz - uz * vy, Ny = uz * vx - ux * vz, Nz = ux * vy - uy * vx;
        const double L = sqrt((Nx * Nx + Ny * Ny) + Nz * Nz);
        if (L > 0.0 && L < __builtin_huge_val()) {
          c0 = vcluster[i0]; c1 = vcluster[i1]; c2 = vcluster[i2];
          const double nx = Nx / L, ny = Ny / L, nz = Nz / L, w = 0.5 * L;
          if (w >= (double)SIMPLIFY_GUARD) {               // the guard alone fails the call: no quadric entry is converted
#pragma unroll
            for (int k = 0; k < 19; ++k) val[k] = 0;
            val[6] = SIMPLIFY_GUARD;
          } else {
            val[0] = __double2ll_rn((w * (nx * nx)) * SIMPLIFY_Q_SCALE);
            val[1] = __double2ll_rn((w * (nx * ny)) * SIMPLIFY_Q_SCALE);
            val[2] = __double2ll_rn((w * (nx * nz)) * SIMPLIFY_Q_SCALE);
            val[3] = __double2ll_rn((w * (ny * ny)) * SIMPLIFY_Q_SCALE);
            val[4] = __double2ll_rn((w * (ny * nz)) * SIMPLIFY_Q_SCALE);
            val[5] = __double2ll_rn((w * (nz * nz)) * SIMPLIFY_Q_SCALE);
            val[6] = (long long)ceil(w);
            const double d0 = -((nx * a.px + ny * a.py) + nz * a.pz);
            const double d1 = -((nx * b.px + ny * b.py) + nz * b.pz);
            const double d2 = -((nx * c.px + ny * c.py) + nz * c.pz);
            val[7] = __double2ll_rn((w * (nx * d0)) * SIMPLIFY_Q_SCALE);
            val[8] = __double2ll_rn((w * (ny * d0)) * SIMPLIFY_Q_SCALE);
            val[9] = __double2ll_rn((w * (nz * d0)) * SIMPLIFY_Q_SCALE);
            val[10] = __double2ll_rn((w * (d0 * d0)) * SIMPLIFY_Q_SCALE);
            val[11] = __double2ll_rn((w * (nx * d1)) * SIMPLIFY_Q_SCALE);
            val[12] = __double2ll_rn((w * (ny * d1)) * SIMPLIFY_Q_SCALE);
            val[13] = __double2ll_rn((w * (nz * d1)) * SIMPLIFY_Q_SCALE);
            val[14] = __double2ll_rn((w * (d1 * d1)) * SIMPLIFY_Q_SCALE);
            val[15] = __double2ll_rn((w * (nx * d2)) * SIMPLIFY_Q_SCALE);
            val[16] = __double2ll_rn((w * (ny * d2)) * SIMPLIFY_Q_SCALE);
            val[17] = __double2ll_rn((w * (nz * d2)) * SIMPLIFY_Q_SCALE);
            val[18] = __double2ll_rn((w * (d2 * d2)) * SIMPLIFY_Q_SCALE);
          }
        }
      }
    }
    rec[38] = (unsigned)c0; rec[39] = (unsigned)c1; rec[40] = (unsigned)c2;
  }
  __syncthreads();
  const int j = threadIdx.x & 15, g16 = threadIdx.x & ~15;
  if (j < SIMPLIFY_SLOT_Q) return;
  // where lane j's value of corner k stands: slots 5..10 and 15 are shared by the corners, 11..14 are per corner
  const bool per_corner = j >= 11 && j <= 14;
  const int at0 = per_corner ? 7 + (j - 11) : (j == SIMPLIFY_SLOT_GUARD ? 6 : j - SIMPLIFY_SLOT_Q), step = per_corner ? 4 : 0;
  int cur = -1;
  long long acc = 0;
  auto push = [&](int cluster, long long v) {
    if (cluster == cur) { acc += v; return; }
    if (cur >= 0) add_u64(rows + (long long)cur * SIMPLIFY_ROW + j, acc);
    cur = cluster;
    acc = v;
  };
  for (int s = 0; s < 16; ++s) {
    const unsigned* rec = sh + (g16 + s) * TREC;
    const int c0 = (int)rec[38], c1 = (int)rec[39], c2 = (int)rec[40];
    if (c0 < 0) continue;
    const long long* val = reinterpret_cast<const long long*>(rec);
    long long v0 = val[at0], v1 = val[at0 + step], v2 = val[at0 + 2 * step];
    bool k1 = true, k2 = true;
    if (c1 == c0) { v0 += v1; k1 = false; }
    if (c2 == c0) { v0 += v2; k2 = false; }
    else if (c2 == c1 && k1) { v1 += v2; k2 = false; }
    // the corner that continues the running cluster goes first
    if (k1 && c1 == cur) { push(c1, v1); k1 = false; }
    else if (k2 && c2 == cur) { push(c2, v2); k2 = false; }
    push(c0, v0);
    if (k1) push(c1, v1);
    if (k2) push(c2, v2);
  }
  if (cur >= 0) add_u64(rows + (long long)cur * SIMPLIFY_ROW + j, acc);
}

// the rotated cluster triple of triangle t (smallest first, orientation kept); false: a corner outside the vertices or two
// corners in one cluster
__device__ __forceinline__ bool tri_key(const int* __restrict__ tris, const int* __restrict__ vcluster, long long nverts, long long t,
                                        int& a, int& b, int& c) {
  const long long i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= nverts || i1 >= nverts || i2 >= nverts) return false;
  const int c0 = vcluster[i0], c1 = vcluster[i1], c2 = vcluster[i2];
  if (c0 == c1 || c1 == c2 || c0 == c2) return false;
  if (c0 < c1 && c0 < c2) { a = c0; b = c1; c = c2; }
  else if (c1 < c0 && c1 < c2) { a = c1; b = c2; c = c0; }
  else { a = c2; b = c0; c = c1; }
  return true;
}
__device__ __forceinline__ unsigned tri_hash(int a, int b, int c) {
  unsigned h = (unsigned)a * 0x9E3779B1u;
  h = (h ^ (h >> 15)) + (unsigned)b * 0x85EBCA77u;
  h = (h ^ (h >> 13)) + (unsigned)c * 0xC2B2AE3Du;
  h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15;
  return h;
}

// every non-degenerate triangle enters the table; a slot ends with the lowest index among the triangles of its key.  All
// occupants a slot ever has share one key (atomicMin only follows an equal key), so comparing against any of them is valid;
// the table is at least twice the triangles, so a probe meets an empty slot within `mask` steps.
__global__ __launch_bounds__(SM_THREADS) void simplify_insert_kernel(const int* __restrict__ tris, long long ntris, long long nverts,
                                                                     const int* __restrict__ vcluster, unsigned* __restrict__ table,
                                                                     unsigned mask, int* __restrict__ counters) {
  const long long t = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
  int a = 0, b = 0, c = 0;
  const bool ok = t < ntris && tri_key(tris, vcluster, nverts, t, a, b, c);
  // the count of these triangles: one add per workgroup, spread over 64 words (adds to ONE word from every wave of a 20 M
  // triangle mesh took longer than everything else in this kernel)
  const int n = __syncthreads_count(ok);
  if (threadIdx.x == 0 && n > 0) atomicAdd(counters + (blockIdx.x & (SIMPLIFY_COUNTERS - 1)), n);
  if (!ok) return;
  unsigned s = tri_hash(a, b, c) & mask;
  for (unsigned step = 0; step <= mask; ++step, s = (s + 1) & mask) {
    const unsigned old = atomicCAS(table + s, SIMPLIFY_EMPTY, (unsigned)t);
    if (old == SIMPLIFY_EMPTY) return;
    int oa, ob, oc;
    if (tri_key(tris, vcluster, nverts, old, oa, ob, oc) && oa == a && ob == b && oc == c) {
      atomicMin(table + s, (unsigned)t);
      return;
    }
  }
}

__global__ __launch_bounds__(64) void simplify_sum_counters_kernel(const int* __restrict__ counters, int* __restrict__ total) {
  int v = counters[threadIdx.x];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  if (threadIdx.x == 0) *total = v;
}

__global__ __launch_bounds__(SM_THREADS) void simplify_survivors_kernel(const unsigned* __restrict__ table, long long slots,
                                                                        long long ntris, unsigned* __restrict__ flag) {
  const long long s = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (s >= slots) return;
  const unsigned t = table[s];
  if (t != SIMPLIFY_EMPTY && (long long)t < ntris) flag[t] = 1u;
}

__global__ __launch_bounds__(SM_THREADS) void simplify_mark_ref_kernel(const int* __restrict__ tris, long long ntris, long long nverts,
                                                                       const int* __restrict__ vcluster, const unsigned* __restrict__ flag,
                                                                       unsigned* __restrict__ ref) {
  const long long t = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (t >= ntris || flag[t] == 0u) return;
  int a, b, c;
  if (!tri_key(tris, vcluster, nverts, t, a, b, c)) return;
  ref[a] = 1u; ref[b] = 1u; ref[c] = 1u;
}

__global__ __launch_bounds__(SM_THREADS) void simplify_guard_kernel(const unsigned* __restrict__ ref, const u64* __restrict__ rows,
                                                                    long long cmax, int* __restrict__ status) {
  const long long c = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (c >= cmax || ref[c] == 0u) return;
  if ((long long)rows[c * SIMPLIFY_ROW + SIMPLIFY_SLOT_GUARD] >= SIMPLIFY_GUARD) atomicOr(status, SIMPLIFY_STATUS_OVERFLOW);
}

// ---- emit: ref and flag hold exclusive prefix sums over cmax + 1 / ntris + 1 entries, so entry i was set iff x[i + 1] != x[i] ----
__global__ __launch_bounds__(SM_THREADS) void simplify_emit_vertices_kernel(const float* __restrict__ verts, SimplifyGrid G,
                                                                            const u64* __restrict__ rows, const unsigned* __restrict__ ref,
                                                                            long long cmax, int average, double lambda,
                                                                            float* __restrict__ out) {
  const long long c = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (c >= cmax) return;
  const unsigned r = ref[c];
  if (ref[c + 1] == r) return;
  const u64* row = rows + c * SIMPLIFY_ROW;
  const long long n = (long long)row[SIMPLIFY_SLOT_COUNT], first = (long long)row[SIMPLIFY_SLOT_MIN];
  float* o = out + 3ll * r;
  if (n == 1) {                                            // the vertex itself, bit for bit
    o[0] = verts[3 * first]; o[1] = verts[3 * first + 1]; o[2] = verts[3 * first + 2];
    return;
  }
  const Local a = locate(G, verts, first);
  const double den = (double)n * SIMPLIFY_P_SCALE;
  const double mx = (double)(long long)row[1] / den, my = (double)(long long)row[2] / den, mz = (double)(long long)row[3] / den;
  double x = mx, y = my, z = mz;
  const double a00 = (double)(long long)row[5] / SIMPLIFY_Q_SCALE, a01 = (double)(long long)row[6] / SIMPLIFY_Q_SCALE;
  const double a02 = (double)(long long)row[7] / SIMPLIFY_Q_SCALE, a11 = (double)(long long)row[8] / SIMPLIFY_Q_SCALE;
  const double a12 = (double)(long long)row[9] / SIMPLIFY_Q_SCALE, a22 = (double)(long long)row[10] / SIMPLIFY_Q_SCALE;
  const double tr = (a00 + a11) + a22;
  if (!average && tr != 0.0) {
    // (A + mu I) x = mu mean - b, mu = lambda tr: symmetric positive definite, condition <= (1 + lambda) / lambda; LDL^T
    const double mu = lambda * tr;
    const double r0 = mu * mx - (double)(long long)row[11] / SIMPLIFY_Q_SCALE;
    const double r1 = mu * my - (double)(long long)row[12] / SIMPLIFY_Q_SCALE;
    const double r2 = mu * mz - (double)(long long)row[13] / SIMPLIFY_Q_SCALE;
    const double m00 = a00 + mu, m11 = a11 + mu, m22 = a22 + mu;
    const double l10 = a01 / m00, l20 = a02 / m00;
    const double e1 = m11 - l10 * a01;
    const double l21 = (a12 - l20 * a01) / e1;
    const double e2 = (m22 - l20 * a02) - l21 * (l21 * e1);
    const double y1 = r1 - l10 * r0, y2 = (r2 - l20 * r0) - l21 * y1;
    z = y2 / e2;
    y = y1 / e1 - l21 * z;
    x = (r0 / m00 - l10 * y) - l20 * z;
  }
  x = fmin(fmax(x, -0.5), 0.5); y = fmin(fmax(y, -0.5), 0.5); z = fmin(fmax(z, -0.5), 0.5);
  o[0] = (float)(G.lo[0] + G.h * (((double)a.cx + 0.5) + x));
  o[1] = (float)(G.lo[1] + G.h * (((double)a.cy + 0.5) + y));
  o[2] = (float)(G.lo[2] + G.h * (((double)a.cz + 0.5) + z));
}

__global__ __launch_bounds__(SM_THREADS) void simplify_emit_triangles_kernel(const int* __restrict__ tris, long long ntris, long long nverts,
                                                                             const int* __restrict__ vcluster,
                                                                             const unsigned* __restrict__ flag,
                                                                             const unsigned* __restrict__ ref, int* __restrict__ out) {
  const long long t = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (t >= ntris) return;
  const unsigned at = flag[t];
  if (flag[t + 1] == at) return;
  int a, b, c;
  if (!tri_key(tris, vcluster, nverts, t, a, b, c)) return;
  out[3ll * at] = (int)ref[a]; out[3ll * at + 1] = (int)ref[b]; out[3ll * at + 2] = (int)ref[c];
}

__global__ __launch_bounds__(SM_THREADS) void simplify_emit_map_kernel(const int* __restrict__ vcluster, long long nverts,
                                                                       const unsigned* __restrict__ ref, int* __restrict__ map) {
  const long long i = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
  if (i >= nverts) return;
  const int c = vcluster[i];
  map[i] = ref[c + 1] != ref[c] ? (int)ref[c] : -1;
}

struct Args {
  SimplifyGrid G;
  SimplifyLayout L;
  long long cells;
};
unsigned blocks_of(long long n) { return (unsigned)((n + SM_THREADS - 1) / SM_THREADS); }

bool dims_ok(const int* dims, long long& cells) {
  if (!dims || dims[0] < 1 || dims[1] < 1 || dims[2] < 1) return false;
  cells = (long long)dims[0] * dims[1];            // < 2^62
  if (cells > SIMPLIFY_MAX_CELLS) return false;
  cells *= dims[2];
  return cells <= SIMPLIFY_MAX_CELLS;
}

int fill(Args& a, const float* verts, long long nverts, const int* tris, long long ntris, const double* lo, double h, const int* dims,
         int contraction, void* scratch, long long scratch_bytes) {
  ISHAP_REQUIRE(lo && dims, "mesh simplify: null argument (lo, dims)");
  ISHAP_REQUIRE(nverts >= 0 && nverts <= 0x7fffffffll, "mesh simplify: 0 <= nverts <= 2^31 - 1 (vertex indices are int32)");
  ISHAP_REQUIRE(ntris >= 0 && ntris <= 0x7fffffffll / 3, "mesh simplify: 0 <= 3 ntris <= 2^31 - 1");
  ISHAP_REQUIRE(h > 0.0 && h < __builtin_huge_val(), "mesh simplify: the cell size h must be positive and finite");
  ISHAP_REQUIRE(lo[0] - lo[0] == 0.0 && lo[1] - lo[1] == 0.0 && lo[2] - lo[2] == 0.0, "mesh simplify: the origin lo must be finite");
  ISHAP_REQUIRE(dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1, "mesh simplify: every grid dim must be >= 1");
  ISHAP_REQUIRE(dims_ok(dims, a.cells), "mesh simplify: gx gy gz <= 2^30 cells (use a larger cell)");
  ISHAP_REQUIRE(contraction == SIMPLIFY_QUADRIC || contraction == SIMPLIFY_AVERAGE, "mesh simplify: unknown contraction (0 quadric, 1 average)");
  ISHAP_REQUIRE((verts || nverts == 0) && (tris || ntris == 0), "mesh simplify: null argument (verts, tris)");
  ISHAP_REQUIRE(scratch, "mesh simplify: null scratch");
  a.L = simplify_layout(scratch, nverts, ntris, a.cells);
  ISHAP_REQUIRE(scratch_bytes >= a.L.bytes, "mesh simplify: scratch smaller than ishap_mesh_simplify_scratch_bytes(nverts, ntris, dims)");
  ISHAP_REQUIRE(((uintptr_t)scratch & 15) == 0, "mesh simplify: scratch must be 16-byte aligned");
  for (int k = 0; k < 3; ++k) { a.G.lo[k] = lo[k]; a.G.g[k] = dims[k]; }
  a.G.h = h;
  return 0;
}

}  // namespace

extern "C" long long ishap_mesh_simplify_scratch_bytes(long long nverts, long long ntris, const int* dims) {
  long long cells;
  if (nverts < 0 || nverts > 0x7fffffffll || ntris < 0 || ntris > 0x7fffffffll / 3 || !dims_ok(dims, cells)) return -1;
  return simplify_layout(nullptr, nverts, ntris, cells).bytes;
}

extern "C" int ishap_mesh_simplify_count(const float* verts, long long nverts, const int* tris, long long ntris, const double* lo, double h,
                                         const int* dims, int contraction, void* scratch, long long scratch_bytes, int* counts,
                                         void* stream) {
  Args a;
  ISHAP_TRY(fill(a, verts, nverts, tris, ntris, lo, h, dims, contraction, scratch, scratch_bytes));
  ISHAP_REQUIRE(counts, "mesh simplify: null argument (counts)");
  const SimplifyLayout& L = a.L;
  hipStream_t s = (hipStream_t)stream;
  int* hdr = L.hdr;
  ISHAP_CHECK_HIP(hipMemsetAsync(counts, 0, 3 * sizeof(int), s));
  ISHAP_CHECK_HIP(hipMemsetAsync(hdr, 0, SIMPLIFY_HDR_BYTES, s));
  if (nverts == 0 || ntris == 0) return 0;                 // an empty mesh: nothing is launched
  unsigned *bitmap = L.bitmap, *prefix = L.prefix, *ref = L.ref, *table = L.tab, *flag = L.flag, *totals = L.totals;
  int* vcluster = L.vcluster; u64* rows = L.rows;
  ISHAP_CHECK_HIP(hipMemsetAsync(bitmap, 0, 4 * L.words, s));
  ISHAP_CHECK_HIP(hipMemsetAsync(ref, 0, 4 * (L.cmax + 1), s));
  ISHAP_CHECK_HIP(hipMemsetAsync(table, 0xff, 4 * L.table, s));
  ISHAP_CHECK_HIP(hipMemsetAsync(flag, 0, 4 * (ntris + 1), s));
  // a. cells -> clusters
  hipLaunchKernelGGL(simplify_mark_kernel, dim3(blocks_of(nverts)), dim3(SM_THREADS), 0, s, verts, nverts, a.G, bitmap);
  hipLaunchKernelGGL(simplify_popc_kernel, dim3(blocks_of(L.words)), dim3(SM_THREADS), 0, s, (const unsigned*)bitmap, L.words, prefix);
  scan_exclusive_u32(prefix, L.words, totals, (unsigned*)hdr, s);
  // b. per-cluster sums
  const long long row_words = L.cmax * SIMPLIFY_ROW;
  hipLaunchKernelGGL(simplify_clear_rows_kernel, dim3(blocks_of(row_words) < 8192u ? blocks_of(row_words) : 8192u), dim3(SM_THREADS), 0, s,
                     (const int*)hdr, rows);
  hipLaunchKernelGGL(simplify_vertex_sums_kernel, dim3(blocks_of(nverts)), dim3(SM_THREADS), 0, s, verts, nverts, a.G,
                     (const unsigned*)bitmap, (const unsigned*)prefix, vcluster, rows);
  if (contraction == SIMPLIFY_QUADRIC)
    hipLaunchKernelGGL(simplify_quadric_sums_kernel, dim3(blocks_of(ntris)), dim3(SM_THREADS), 0, s, verts, nverts, tris, ntris, a.G,
                       (const int*)vcluster, rows);
  // c. triangles
  hipLaunchKernelGGL(simplify_insert_kernel, dim3(blocks_of(ntris)), dim3(SM_THREADS), 0, s, tris, ntris, nverts, (const int*)vcluster, table,
                     (unsigned)(L.table - 1), hdr + SIMPLIFY_COUNTERS);
  hipLaunchKernelGGL(simplify_sum_counters_kernel, dim3(1), dim3(64), 0, s, (const int*)(hdr + SIMPLIFY_COUNTERS), hdr + 1);
  hipLaunchKernelGGL(simplify_survivors_kernel, dim3(blocks_of(L.table)), dim3(SM_THREADS), 0, s, (const unsigned*)table, L.table, ntris, flag);
  // d. referenced clusters, the guard, the output ranks
  hipLaunchKernelGGL(simplify_mark_ref_kernel, dim3(blocks_of(ntris)), dim3(SM_THREADS), 0, s, tris, ntris, nverts, (const int*)vcluster,
                     (const unsigned*)flag, ref);
  if (contraction == SIMPLIFY_QUADRIC)
    hipLaunchKernelGGL(simplify_guard_kernel, dim3(blocks_of(L.cmax)), dim3(SM_THREADS), 0, s, (const unsigned*)ref, (const u64*)rows, L.cmax,
                       counts + 2);
  scan_exclusive_u32(ref, L.cmax + 1, totals, (unsigned*)counts, s);
  scan_exclusive_u32(flag, ntris + 1, totals, (unsigned*)counts + 1, s);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_mesh_simplify_emit(const float* verts, long long nverts, const int* tris, long long ntris, const double* lo, double h,
                                        const int* dims, int contraction, double regularization, void* scratch, long long scratch_bytes,
                                        float* out_verts, int* out_tris, int* vertex_map, int* vertex_cluster, void* stream) {
  Args a;
  ISHAP_TRY(fill(a, verts, nverts, tris, ntris, lo, h, dims, contraction, scratch, scratch_bytes));
  ISHAP_REQUIRE(regularization > 0.0 && regularization < __builtin_huge_val(), "mesh simplify: regularization must be positive and finite");
  ISHAP_REQUIRE(vertex_map || nverts == 0, "mesh simplify: null argument (vertex_map)");
  hipStream_t s = (hipStream_t)stream;
  if (nverts == 0) return 0;
  if (ntris == 0) {                                        // an empty mesh: no vertex has an output index
    ISHAP_CHECK_HIP(hipMemsetAsync(vertex_map, 0xff, 4 * nverts, s));
    if (vertex_cluster) ISHAP_CHECK_HIP(hipMemsetAsync(vertex_cluster, 0xff, 4 * nverts, s));
    return 0;
  }
  ISHAP_REQUIRE(out_verts && out_tris, "mesh simplify: null argument (out_verts, out_tris)");
  const SimplifyLayout& L = a.L;
  const int* vcluster = L.vcluster; const u64* rows = L.rows;
  const unsigned *ref = L.ref, *flag = L.flag;
  hipLaunchKernelGGL(simplify_emit_vertices_kernel, dim3(blocks_of(L.cmax)), dim3(SM_THREADS), 0, s, verts, a.G, rows, ref, L.cmax,
                     contraction == SIMPLIFY_AVERAGE ? 1 : 0, regularization, out_verts);
  hipLaunchKernelGGL(simplify_emit_triangles_kernel, dim3(blocks_of(ntris)), dim3(SM_THREADS), 0, s, tris, ntris, nverts, vcluster, flag, ref,
                     out_tris);
  hipLaunchKernelGGL(simplify_emit_map_kernel, dim3(blocks_of(nverts)), dim3(SM_THREADS), 0, s, vcluster, nverts, ref, vertex_map);
  if (vertex_cluster) ISHAP_CHECK_HIP(hipMemcpyAsync(vertex_cluster, vcluster, 4 * nverts, hipMemcpyDeviceToDevice, s));
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
