// As-rigid-as-possible mesh deformation (meshProcess.py:222-236: Open3D's deform_as_rigid_as_possible in the reference) and
// the nearest-vertex pick that turns drag handles into vertex ids (main.py:525-527: a KD-tree query in the reference).
//
// ARAP is Sorkine & Alexa 2007, "spokes" energy, cotangent weights, all arithmetic in fp64:
//   setup   vertex -> triangle lists, a CSR adjacency (rows sorted, no duplicates), w_ij = max(0, 1/2 sum cot), the
//           connected components of the w > 0 graph (min-label propagation); a vertex is free when it is not constrained and
//           its component holds a constrained vertex, every other unconstrained vertex keeps its rest position bit for bit
//   local   S_i = sum_j w_ij e_ij e'_ij^T, R_i = V U^T from a one-sided Jacobi SVD, det fixed on the smallest singular value
//   global  L_ff x_f = b_f - L_fc x_c by Jacobi-preconditioned CG on three columns at once, warm-started
// Every sum has a fixed order (rows in column order, dot products per workgroup and then in one workgroup), the only atomics
// are integer ones whose results do not depend on their order (list lengths, sorted afterwards; min labels), so a call is
// bitwise repeatable.  CG runs in chunks of ARAP_CHUNK iterations; the host reads the device's done flag once per chunk.
#include "common.h"
#include "scan.h"

namespace {

constexpr int AB = 256;                 // threads of every per-vertex / per-triangle workgroup
constexpr int ARAP_CHUNK = 32;          // CG iterations enqueued between two reads of the done flag
constexpr int NPART = 9;                // doubles per workgroup partial

// device-resident state of one call; the host reads it at the end of setup steps and once per CG chunk
struct ArapState {
  double rz[3], alpha[3], beta[3], rhs_norm[3];
  int active[3];
  int iters, done, capped;
  int bad, changed, nfree, pad;
};

__device__ __forceinline__ unsigned grid_index() { return blockIdx.x * AB + threadIdx.x; }

// ---------------------------------------------------------------- argument validation (device-side ids)
// bad |= 1: a triangle index outside [0, V);  2: a constraint id outside [0, V);  4: a repeated constraint id
__global__ __launch_bounds__(AB) void arap_check_tris_kernel(const int* __restrict__ t, long long nt3, int nv, ArapState* st) {
  const long long k = (long long)blockIdx.x * AB + threadIdx.x;
  if (k < nt3) {
    const int v = t[k];
    if (v < 0 || v >= nv) atomicOr(&st->bad, 1);
  }
}
__global__ __launch_bounds__(AB) void arap_check_cons_kernel(const int* __restrict__ cons, int nc, int nv, int* __restrict__ ccount,
                                                             ArapState* st) {
  const int k = blockIdx.x * AB + threadIdx.x;
  if (k >= nc) return;
  const int c = cons[k];
  if (c < 0 || c >= nv) { atomicOr(&st->bad, 2); return; }
  if (atomicAdd(ccount + c, 1) != 0) atomicOr(&st->bad, 4);
}

// ---------------------------------------------------------------- adjacency
// the slot order depends on atomic timing; arap_rows_kernel sorts every list before it is read
__global__ __launch_bounds__(AB) void arap_vt_fill_kernel(const int* __restrict__ t, long long nt, const unsigned* __restrict__ off,
                                                          unsigned* __restrict__ cursor, unsigned* __restrict__ list) {
  const long long f = (long long)blockIdx.x * AB + threadIdx.x;
  if (f >= nt) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int v = t[3 * f + c];
    list[off[v] + atomicAdd(cursor + v, 1u)] = (unsigned)f;
  }
}
__device__ __forceinline__ void insertion_sort(unsigned* a, unsigned n) {
  for (unsigned k = 1; k < n; ++k) {
    const unsigned key = a[k];
    unsigned m = k;
    while (m > 0 && a[m - 1] > key) { a[m] = a[m - 1]; --m; }
    a[m] = key;
  }
}
// per vertex i: sort its triangle list; its neighbours (the other corners of those triangles, i itself excluded) go to
// cand[2 vt_off[i] ...], sorted and without duplicates; rowcnt[i] = how many
__global__ __launch_bounds__(AB) void arap_rows_kernel(const int* __restrict__ t, int nv, const unsigned* __restrict__ vt_off,
                                                       unsigned* __restrict__ vt_list, unsigned* __restrict__ cand,
                                                       unsigned* __restrict__ rowcnt) {
  const unsigned i = grid_index();
  if (i >= (unsigned)nv) return;
  const unsigned lo = vt_off[i], hi = vt_off[i + 1];
  insertion_sort(vt_list + lo, hi - lo);
  unsigned* c = cand + 2ull * lo;
  unsigned n = 0;
  for (unsigned k = lo; k < hi; ++k) {
    const long long f = vt_list[k];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const unsigned v = (unsigned)t[3 * f + q];
      if (v != i) c[n++] = v;
    }
  }
  insertion_sort(c, n);
  unsigned u = 0;
  for (unsigned k = 0; k < n; ++k)
    if (u == 0 || c[k] != c[u - 1]) c[u++] = c[k];
  rowcnt[i] = u;
}

// cot of the angle at corner k opposite the edge (i, j), with a from the lower and b from the higher of i, j so that
// w_ij and w_ji are the same operations; 0 for a triangle with |a x b| <= 1e-12 |a| |b|
__device__ __forceinline__ double edge_cot(const float* __restrict__ p, unsigned i, unsigned j, unsigned k) {
  const unsigned lo = i < j ? i : j, hi = i < j ? j : i;
  const double kx = p[3ull * k], ky = p[3ull * k + 1], kz = p[3ull * k + 2];
  const double ax = (double)p[3ull * lo] - kx, ay = (double)p[3ull * lo + 1] - ky, az = (double)p[3ull * lo + 2] - kz;
  const double bx = (double)p[3ull * hi] - kx, by = (double)p[3ull * hi + 1] - ky, bz = (double)p[3ull * hi + 2] - kz;
  const double dot = ax * bx + ay * by + az * bz;
  const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const double cr = sqrt(cx * cx + cy * cy + cz * cz);
  const double na = sqrt(ax * ax + ay * ay + az * az), nb = sqrt(bx * bx + by * by + bz * bz);
  return cr <= 1e-12 * na * nb ? 0.0 : dot / cr;
}
// per vertex i: the CSR row (col, w) from cand, weights summed over i's triangles in ascending index, diag = sum of the row
__global__ __launch_bounds__(AB) void arap_weights_kernel(const float* __restrict__ p, const int* __restrict__ t, int nv,
                                                          const unsigned* __restrict__ vt_off, const unsigned* __restrict__ vt_list,
                                                          const unsigned* __restrict__ cand, const unsigned* __restrict__ row,
                                                          unsigned* __restrict__ col, double* __restrict__ w, double* __restrict__ diag) {
  const unsigned i = grid_index();
  if (i >= (unsigned)nv) return;
  const unsigned lo = vt_off[i], hi = vt_off[i + 1], r0 = row[i], r1 = row[i + 1];
  const unsigned* c = cand + 2ull * lo;
  double d = 0.0;
  for (unsigned e = r0; e < r1; ++e) {
    const unsigned j = c[e - r0];
    double s = 0.0;
    for (unsigned k = lo; k < hi; ++k) {
      const long long f = vt_list[k];
      const unsigned v0 = (unsigned)t[3 * f], v1 = (unsigned)t[3 * f + 1], v2 = (unsigned)t[3 * f + 2];
      const int pi = v0 == i ? 0 : (v1 == i ? 1 : 2);
      const int pj = v0 == j ? 0 : (v1 == j ? 1 : (v2 == j ? 2 : -1));
      if (pj < 0) continue;
      const int pk = 3 - pi - pj;
      s += edge_cot(p, i, j, pk == 0 ? v0 : (pk == 1 ? v1 : v2));
    }
    const double we = fmax(0.0, 0.5 * s);
    col[e] = j;
    w[e] = we;
    d += we;
  }
  diag[i] = d;
}

// ---------------------------------------------------------------- components of the w > 0 graph (min-label propagation)
__global__ __launch_bounds__(AB) void arap_label_init_kernel(int nv, int* __restrict__ label) {
  const unsigned i = grid_index();
  if (i < (unsigned)nv) label[i] = (int)i;
}
// labels only decrease and always name a vertex of the same component with an index <= the holder's; the fixed point (no
// sweep changes anything) is every vertex labelled with its component's lowest index, whatever the order of the updates
__global__ __launch_bounds__(AB) void arap_label_sweep_kernel(int nv, const unsigned* __restrict__ row, const unsigned* __restrict__ col,
                                                              const double* __restrict__ w, int* label, ArapState* st) {
  const unsigned i = grid_index();
  if (i >= (unsigned)nv) return;
  const int l = label[i];
  int m = label[l];
  for (unsigned e = row[i]; e < row[i + 1]; ++e)
    if (w[e] > 0.0) m = min(m, label[col[e]]);
  if (m < l) {
    atomicMin(label + i, m);
    atomicMin(label + l, m);
    st->changed = 1;
  }
}
__global__ __launch_bounds__(AB) void arap_label_jump_kernel(int nv, int* label) {
  const unsigned i = grid_index();
  if (i < (unsigned)nv) {
    const int l = label[i];
    const int m = label[l];
    if (m < l) atomicMin(label + i, m);
  }
}
// has[component of every constrained vertex] = 1
__global__ __launch_bounds__(AB) void arap_mark_kernel(const int* __restrict__ cons, int nc, const int* __restrict__ label,
                                                       int* __restrict__ has) {
  const int k = blockIdx.x * AB + threadIdx.x;
  if (k < nc) has[label[cons[k]]] = 1;
}
// role 2: constrained (x = target), 1: free (x = rest, solved for), 0: kept at rest; x = p'^0
__global__ __launch_bounds__(AB) void arap_roles_kernel(const float* __restrict__ p, int nv, const int* __restrict__ ccount,
                                                        const int* __restrict__ label, const int* __restrict__ has,
                                                        int* __restrict__ role, double* __restrict__ x, ArapState* st) {
  const unsigned i = grid_index();
  if (i >= (unsigned)nv) return;
  const int r = ccount[i] ? 2 : (has[label[i]] ? 1 : 0);
  role[i] = r;
  if (r != 2) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[3ull * i + c] = (double)p[3ull * i + c];
  }
  if (r == 1) atomicAdd(&st->nfree, 1);
}
__global__ __launch_bounds__(AB) void arap_targets_kernel(const int* __restrict__ cons, const float* __restrict__ pos, int nc,
                                                          double* __restrict__ x) {
  const int k = blockIdx.x * AB + threadIdx.x;
  if (k >= nc) return;
  const long long c = cons[k];
#pragma unroll
  for (int q = 0; q < 3; ++q) x[3 * c + q] = (double)pos[3ll * k + q];
}

// ---------------------------------------------------------------- fixed-order reductions
// block partial of NV values per thread into part[blockIdx.x * NPART + k] (LDS tree, the same order every call)
template <int NV>
__device__ __forceinline__ void block_partials(const double (&v)[NV], double* __restrict__ part) {
  __shared__ double red[NV][AB];
#pragma unroll
  for (int k = 0; k < NV; ++k) red[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int o = AB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < NV; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    }
    __syncthreads();
  }
  if (threadIdx.x < NV) part[(long long)blockIdx.x * NPART + threadIdx.x] = red[threadIdx.x][0];
}
// one workgroup: out[k] = sum over the nb partials of value k (each thread sums a fixed stride, then an LDS tree)
template <int NV>
__device__ __forceinline__ void final_sums(const double* __restrict__ part, int nb, double (&out)[NV]) {
  __shared__ double red[NV][AB];
  double s[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) s[k] = 0.0;
  for (int b = threadIdx.x; b < nb; b += AB) {
#pragma unroll
    for (int k = 0; k < NV; ++k) s[k] += part[(long long)b * NPART + k];
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) red[k][threadIdx.x] = s[k];
  __syncthreads();
  for (int o = AB / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
#pragma unroll
      for (int k = 0; k < NV; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) out[k] = red[k][0];
}

// ---------------------------------------------------------------- local step: rotations and the energy
struct V3 { double x, y, z; };
__device__ __forceinline__ double dot3(const V3& a, const V3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// one Hestenes rotation making columns ap, aq of A orthogonal, applied to the same columns of V
__device__ __forceinline__ bool jacobi_pair(V3& ap, V3& aq, V3& vp, V3& vq) {
  const double al = dot3(ap, ap), be = dot3(aq, aq), ga = dot3(ap, aq);
  if (!(fabs(ga) > 1e-15 * sqrt(al * be))) return false;
  const double zeta = (be - al) / (2.0 * ga);
  const double sg = zeta >= 0.0 ? 1.0 : -1.0;
  const double t = fabs(zeta) > 1e100 ? 0.5 / zeta : sg / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  const V3 a0 = ap, v0 = vp;
  ap = {c * a0.x - s * aq.x, c * a0.y - s * aq.y, c * a0.z - s * aq.z};
  aq = {s * a0.x + c * aq.x, s * a0.y + c * aq.y, s * a0.z + c * aq.z};
  vp = {c * v0.x - s * vq.x, c * v0.y - s * vq.y, c * v0.z - s * vq.z};
  vq = {s * v0.x + c * vq.x, s * v0.y + c * vq.y, s * v0.z + c * vq.z};
  return true;
}
__device__ __forceinline__ void swap_if_less(V3& ap, V3& aq, V3& vp, V3& vq, double& sp, double& sq) {
  if (sp < sq) {
    const V3 ta = ap, tv = vp;
    const double ts = sp;
    ap = aq; aq = ta; vp = vq; vq = tv; sp = sq; sq = ts;
  }
}
// R = V U^T of S = U diag(s) V^T (S given by columns), det(R) = +1 by the sign of U's third column; I when s2 <= 1e-9 s1
__device__ __forceinline__ void fit_rotation(V3 a0, V3 a1, V3 a2, double (&R)[9]) {
  V3 v0 = {1.0, 0.0, 0.0}, v1 = {0.0, 1.0, 0.0}, v2 = {0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < 16; ++sweep) {
    bool rot = jacobi_pair(a0, a1, v0, v1);
    rot |= jacobi_pair(a0, a2, v0, v2);
    rot |= jacobi_pair(a1, a2, v1, v2);
    if (!rot) break;
  }
  // A V = U diag(s): the singular values are the column norms; sort them descending
  double s0 = sqrt(dot3(a0, a0)), s1 = sqrt(dot3(a1, a1)), s2 = sqrt(dot3(a2, a2));
  swap_if_less(a0, a1, v0, v1, s0, s1);
  swap_if_less(a1, a2, v1, v2, s1, s2);
  swap_if_less(a0, a1, v0, v1, s0, s1);
  if (!(s1 > 1e-9 * s0)) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  const V3 u0 = {a0.x / s0, a0.y / s0, a0.z / s0}, u1 = {a1.x / s1, a1.y / s1, a1.z / s1};
  // det(V U^T) < 0 would negate U's last column; taking u2 = det(V) (u0 x u1) is the same rule, and also defines u2 when
  // the smallest singular value is 0
  const double dv = v0.x * (v1.y * v2.z - v1.z * v2.y) - v1.x * (v0.y * v2.z - v0.z * v2.y) + v2.x * (v0.y * v1.z - v0.z * v1.y);
  const double sg = dv < 0.0 ? -1.0 : 1.0;
  const V3 u2 = {sg * (u0.y * u1.z - u0.z * u1.y), sg * (u0.z * u1.x - u0.x * u1.z), sg * (u0.x * u1.y - u0.y * u1.x)};
  // R[a][b] = sum_k V[a][k] U[b][k], column k of V is v_k
  const double V_[3][3] = {{v0.x, v1.x, v2.x}, {v0.y, v1.y, v2.y}, {v0.z, v1.z, v2.z}};
  const double U_[3][3] = {{u0.x, u1.x, u2.x}, {u0.y, u1.y, u2.y}, {u0.z, u1.z, u2.z}};
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) R[3 * a + b] = V_[a][0] * U_[b][0] + V_[a][1] * U_[b][1] + V_[a][2] * U_[b][2];
}
__global__ __launch_bounds__(AB) void arap_local_kernel(const float* __restrict__ p, int nv, const unsigned* __restrict__ row,
                                                        const unsigned* __restrict__ col, const double* __restrict__ w,
                                                        const double* __restrict__ x, double* __restrict__ Rout,
                                                        double* __restrict__ part) {
  const unsigned i = grid_index();
  double en[1] = {0.0};
  if (i < (unsigned)nv) {
    const double pix = p[3ull * i], piy = p[3ull * i + 1], piz = p[3ull * i + 2];
    const double xix = x[3ull * i], xiy = x[3ull * i + 1], xiz = x[3ull * i + 2];
    const unsigned r0 = row[i], r1 = row[i + 1];
    // S = sum w e e'^T, kept by columns: column b is sum w e e'_b
    V3 c0 = {0.0, 0.0, 0.0}, c1 = c0, c2 = c0;
    for (unsigned e = r0; e < r1; ++e) {
      const unsigned j = col[e];
      const double we = w[e];
      const double ex = pix - (double)p[3ull * j], ey = piy - (double)p[3ull * j + 1], ez = piz - (double)p[3ull * j + 2];
      const double fx = xix - x[3ull * j], fy = xiy - x[3ull * j + 1], fz = xiz - x[3ull * j + 2];
      const double wx = we * ex, wy = we * ey, wz = we * ez;
      c0.x += wx * fx; c0.y += wy * fx; c0.z += wz * fx;
      c1.x += wx * fy; c1.y += wy * fy; c1.z += wz * fy;
      c2.x += wx * fz; c2.y += wy * fz; c2.z += wz * fz;
    }
    double R[9];
    fit_rotation(c0, c1, c2, R);
#pragma unroll
    for (int k = 0; k < 9; ++k) Rout[9ull * i + k] = R[k];
    double E = 0.0;
    for (unsigned e = r0; e < r1; ++e) {
      const unsigned j = col[e];
      const double ex = pix - (double)p[3ull * j], ey = piy - (double)p[3ull * j + 1], ez = piz - (double)p[3ull * j + 2];
      const double dx = xix - x[3ull * j] - (R[0] * ex + R[1] * ey + R[2] * ez);
      const double dy = xiy - x[3ull * j + 1] - (R[3] * ex + R[4] * ey + R[5] * ez);
      const double dz = xiz - x[3ull * j + 2] - (R[6] * ex + R[7] * ey + R[8] * ez);
      E += w[e] * (dx * dx + dy * dy + dz * dz);
    }
    en[0] = E;
  }
  block_partials<1>(en, part);
}
__global__ __launch_bounds__(AB) void arap_energy_kernel(const double* __restrict__ part, int nb, double* __restrict__ energy) {
  double s[1];
  final_sums<1>(part, nb, s);
  if (threadIdx.x == 0) *energy = s[0];
}

// ---------------------------------------------------------------- global step: right-hand side and CG
// free rows: rhs = sum_j (w/2)(R_i + R_j) e_ij + sum_{j constrained} w_ij x_j, r = rhs - (diag x_i - sum_{j free} w_ij x_j),
// z = r / diag, p = z.  Partials: |rhs|^2, r.z, r.r per column.  Other rows: r = z = p = 0.
__global__ __launch_bounds__(AB) void arap_rhs_kernel(const float* __restrict__ p, int nv, const unsigned* __restrict__ row,
                                                      const unsigned* __restrict__ col, const double* __restrict__ w,
                                                      const double* __restrict__ diag, const int* __restrict__ role,
                                                      const double* __restrict__ R, const double* __restrict__ x,
                                                      double* __restrict__ r, double* __restrict__ z, double* __restrict__ pv,
                                                      double* __restrict__ part) {
  const unsigned i = grid_index();
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < (unsigned)nv) {
    double rr[3] = {0.0, 0.0, 0.0}, zz[3] = {0.0, 0.0, 0.0};
    if (role[i] == 1) {
      const double pix = p[3ull * i], piy = p[3ull * i + 1], piz = p[3ull * i + 2];
      double Ri[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) Ri[k] = R[9ull * i + k];
      double b[3] = {0.0, 0.0, 0.0}, ax[3] = {0.0, 0.0, 0.0};
      for (unsigned e = row[i]; e < row[i + 1]; ++e) {
        const unsigned j = col[e];
        const double we = w[e], hw = 0.5 * we;
        const double ex = pix - (double)p[3ull * j], ey = piy - (double)p[3ull * j + 1], ez = piz - (double)p[3ull * j + 2];
        const double* Rj = R + 9ull * j;
#pragma unroll
        for (int a = 0; a < 3; ++a)
          b[a] += hw * ((Ri[3 * a] + Rj[3 * a]) * ex + (Ri[3 * a + 1] + Rj[3 * a + 1]) * ey + (Ri[3 * a + 2] + Rj[3 * a + 2]) * ez);
        const int rj = role[j];
        if (rj == 2) {
#pragma unroll
          for (int a = 0; a < 3; ++a) b[a] += we * x[3ull * j + a];
        } else if (rj == 1) {
#pragma unroll
          for (int a = 0; a < 3; ++a) ax[a] += we * x[3ull * j + a];
        }
      }
      const double d = diag[i];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        rr[a] = b[a] - (d * x[3ull * i + a] - ax[a]);
        zz[a] = rr[a] / d;
        acc[a] = b[a] * b[a];
        acc[3 + a] = rr[a] * zz[a];
        acc[6 + a] = rr[a] * rr[a];
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { r[3ull * i + a] = rr[a]; z[3ull * i + a] = zz[a]; pv[3ull * i + a] = zz[a]; }
  }
  block_partials<9>(acc, part);
}
__device__ __forceinline__ bool met(double rr, double rhs_norm, double tol) { return sqrt(rr) <= tol * fmax(rhs_norm, 1e-300); }
__global__ __launch_bounds__(AB) void arap_cg_init_kernel(const double* __restrict__ part, int nb, double tol, ArapState* st) {
  double s[9];
  final_sums<9>(part, nb, s);
  if (threadIdx.x != 0) return;
  int any = 0;
  for (int c = 0; c < 3; ++c) {
    st->rhs_norm[c] = sqrt(s[c]);
    st->rz[c] = s[3 + c];
    st->alpha[c] = 0.0;
    st->beta[c] = 0.0;
    st->active[c] = met(s[6 + c], st->rhs_norm[c], tol) ? 0 : 1;
    any |= st->active[c];
  }
  st->iters = 0;
  st->capped = 0;
  st->done = any ? 0 : 1;
}
// p' = z + beta p, one expression for the owner row and for every neighbour that reads it
__device__ __forceinline__ double next_dir(double zj, double beta, double pj) { return __fma_rn(beta, pj, zj); }
// free rows: pdst = z + beta psrc, q = L_ff pdst; partials p.q per column
__global__ __launch_bounds__(AB) void arap_cg_spmv_kernel(int nv, const unsigned* __restrict__ row, const unsigned* __restrict__ col,
                                                          const double* __restrict__ w, const double* __restrict__ diag,
                                                          const int* __restrict__ role, const double* __restrict__ z,
                                                          const double* __restrict__ psrc, double* __restrict__ pdst,
                                                          double* __restrict__ q, const ArapState* __restrict__ st,
                                                          double* __restrict__ part) {
  if (st->done) return;
  const double b0 = st->beta[0], b1 = st->beta[1], b2 = st->beta[2];
  const unsigned i = grid_index();
  double acc[3] = {0.0, 0.0, 0.0};
  if (i < (unsigned)nv && role[i] == 1) {
    const double pi0 = next_dir(z[3ull * i], b0, psrc[3ull * i]);
    const double pi1 = next_dir(z[3ull * i + 1], b1, psrc[3ull * i + 1]);
    const double pi2 = next_dir(z[3ull * i + 2], b2, psrc[3ull * i + 2]);
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (unsigned e = row[i]; e < row[i + 1]; ++e) {
      const unsigned j = col[e];
      if (role[j] != 1) continue;
      const double we = w[e];
      s0 += we * next_dir(z[3ull * j], b0, psrc[3ull * j]);
      s1 += we * next_dir(z[3ull * j + 1], b1, psrc[3ull * j + 1]);
      s2 += we * next_dir(z[3ull * j + 2], b2, psrc[3ull * j + 2]);
    }
    const double d = diag[i];
    const double q0 = d * pi0 - s0, q1 = d * pi1 - s1, q2 = d * pi2 - s2;
    pdst[3ull * i] = pi0; pdst[3ull * i + 1] = pi1; pdst[3ull * i + 2] = pi2;
    q[3ull * i] = q0; q[3ull * i + 1] = q1; q[3ull * i + 2] = q2;
    acc[0] = pi0 * q0; acc[1] = pi1 * q1; acc[2] = pi2 * q2;
  }
  block_partials<3>(acc, part);
}
__global__ __launch_bounds__(AB) void arap_cg_alpha_kernel(const double* __restrict__ part, int nb, ArapState* st) {
  if (st->done) return;
  double s[3];
  final_sums<3>(part, nb, s);
  if (threadIdx.x != 0) return;
  int any = 0;
  for (int c = 0; c < 3; ++c) {
    st->alpha[c] = 0.0;
    if (!st->active[c]) continue;
    if (s[c] > 0.0) {
      st->alpha[c] = st->rz[c] / s[c];
    } else {            // p = 0 without r = 0: the column cannot go on and has not met the rule
      st->active[c] = 0;
      st->capped = 1;
    }
    any |= st->active[c];
  }
  if (!any) st->done = 1;
}
// free rows, active columns: x += alpha p, r -= alpha q, z = r / diag; partials r.z, r.r
__global__ __launch_bounds__(AB) void arap_cg_update_kernel(int nv, const double* __restrict__ diag, const int* __restrict__ role,
                                                            const double* __restrict__ pv, const double* __restrict__ q,
                                                            double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                            const ArapState* __restrict__ st, double* __restrict__ part) {
  if (st->done) return;
  const unsigned i = grid_index();
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (i < (unsigned)nv && role[i] == 1) {
    const double d = diag[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (!st->active[c]) continue;
      const double al = st->alpha[c];
      x[3ull * i + c] += al * pv[3ull * i + c];
      const double rc = r[3ull * i + c] - al * q[3ull * i + c];
      const double zc = rc / d;
      r[3ull * i + c] = rc;
      z[3ull * i + c] = zc;
      acc[c] = rc * zc;
      acc[3 + c] = rc * rc;
    }
  }
  block_partials<6>(acc, part);
}
__global__ __launch_bounds__(AB) void arap_cg_beta_kernel(const double* __restrict__ part, int nb, double tol, int max_cg, ArapState* st) {
  if (st->done) return;
  double s[6];
  final_sums<6>(part, nb, s);
  if (threadIdx.x != 0) return;
  const int it = st->iters + 1;
  st->iters = it;
  int any = 0;
  for (int c = 0; c < 3; ++c) {
    if (!st->active[c]) { st->beta[c] = 0.0; continue; }
    if (met(s[3 + c], st->rhs_norm[c], tol)) {
      st->active[c] = 0;
      st->beta[c] = 0.0;
    } else {
      st->beta[c] = s[c] / st->rz[c];
      st->rz[c] = s[c];
      any = 1;
    }
  }
  if (any && it >= max_cg) st->capped = 1;
  if (!any || it >= max_cg) st->done = 1;
}
__global__ void arap_cg_record_kernel(const ArapState* __restrict__ st, int* __restrict__ out) {
  if (threadIdx.x == 0) *out = st->capped ? -st->iters : st->iters;
}
__global__ __launch_bounds__(AB) void arap_output_kernel(const double* __restrict__ x, int nv, float* __restrict__ out) {
  const unsigned i = grid_index();
  if (i >= (unsigned)nv) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[3ull * i + c] = (float)x[3ull * i + c];
}

// ---------------------------------------------------------------- nearest vertex (main.py:525-527)
// idx[i] = argmin_v |pts[i] - verts[v]|^2 in fp64 (differences of fp32 values, exact squares up to the final sums), the
// lowest index on ties: vertices are visited in index order and only a strictly smaller distance replaces the best
__global__ __launch_bounds__(256) void nearest_vertex_kernel(const float* __restrict__ P, long long np, const float* __restrict__ Vt,
                                                             long long nv, int* __restrict__ idx) {
  __shared__ float tile[1024 * 3];
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double ax = 0.0, ay = 0.0, az = 0.0;
  if (i < np) { ax = P[3 * i]; ay = P[3 * i + 1]; az = P[3 * i + 2]; }
  double best = 1.0e300;
  long long best_v = 0;
  for (long long j0 = 0; j0 < nv; j0 += 1024) {
    const int m = (int)min(1024LL, nv - j0);
    __syncthreads();
    for (int k = threadIdx.x; k < m * 3; k += 256) tile[k] = Vt[3 * j0 + k];
    __syncthreads();
    for (int k = 0; k < m; ++k) {
      const double dx = ax - (double)tile[3 * k], dy = ay - (double)tile[3 * k + 1], dz = az - (double)tile[3 * k + 2];
      const double d = dx * dx + dy * dy + dz * dz;
      if (d < best) { best = d; best_v = j0 + k; }
    }
  }
  if (i < np) idx[i] = (int)best_v;
}

// ---------------------------------------------------------------- scratch layout
struct ArapLayout {
  ArapState* st;
  unsigned *vt_off, *vt_cur, *row, *totals, *vt_list, *cand, *col;
  int *ccount, *has, *label, *role;
  double *w, *diag, *x, *r, *z, *pbuf[2], *q, *R, *part;
  long long zero_end, bytes, nb;           // [0, zero_end) is cleared at the start of a call
};
ArapLayout arap_layout(void* base, long long nv, long long nt) {
  Carve c{(char*)base};
  ArapLayout L;
  L.nb = (nv + AB - 1) / AB;
  L.st = c.take<ArapState>(1);
  L.vt_off = c.take<unsigned>(nv + 1);
  L.vt_cur = c.take<unsigned>(nv);
  L.ccount = c.take<int>(nv);
  L.has = c.take<int>(nv);
  L.row = c.take<unsigned>(nv + 1);
  L.zero_end = c.total();
  L.totals = c.take<unsigned>(scan_u32_blocks(nv + 1) + 1);
  L.vt_list = c.take<unsigned>(3 * nt);
  L.cand = c.take<unsigned>(6 * nt);
  L.col = c.take<unsigned>(6 * nt);
  L.w = c.take<double>(6 * nt);
  L.label = c.take<int>(nv);
  L.role = c.take<int>(nv);
  L.diag = c.take<double>(nv);
  L.x = c.take<double>(3 * nv);
  L.r = c.take<double>(3 * nv);
  L.z = c.take<double>(3 * nv);
  L.pbuf[0] = c.take<double>(3 * nv);
  L.pbuf[1] = c.take<double>(3 * nv);
  L.q = c.take<double>(3 * nv);
  L.R = c.take<double>(9 * nv);
  L.part = c.take<double>(NPART * L.nb);
  L.bytes = c.total();
  return L;
}

int read_state(const ArapState* d, ArapState& h, hipStream_t s) {
  ISHAP_CHECK_HIP(hipMemcpyAsync(&h, d, sizeof(ArapState), hipMemcpyDeviceToHost, s));
  ISHAP_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // namespace

extern "C" long long ishap_arap_scratch_bytes(long long nverts, long long ntris, long long ncons) {
  if (nverts < 0 || ntris < 0 || ncons < 0) return -1;
  return arap_layout(nullptr, nverts, ntris).bytes;
}

extern "C" int ishap_arap(const float* rest, long long nverts, const int* tris, long long ntris, const int* cons_ids,
                          const float* cons_pos, long long ncons, int max_iter, double tol, long long max_cg, float* out,
                          double* energy, int* cg_iters, void* scratch, long long scratch_bytes, void* stream) {
  ISHAP_REQUIRE(rest && tris && out && scratch && nverts > 0 && ntris > 0 && ncons >= 0 && max_iter >= 0, "arap arguments");
  ISHAP_REQUIRE(ncons == 0 || (cons_ids && cons_pos), "arap: constraint ids and positions");
  ISHAP_REQUIRE(max_iter == 0 || (energy && cg_iters), "arap: energy[max_iter] and cg_iters[max_iter]");
  ISHAP_REQUIRE(ncons <= nverts, "arap: more constraints than vertices");
  ISHAP_REQUIRE(tol >= 0.0, "arap: tol >= 0");
  ISHAP_REQUIRE(max_cg < (1ll << 31), "arap: max_cg < 2^31 (<= 0: 4 free vertices + 100)");
  ISHAP_REQUIRE(nverts < (1ll << 31) && 6 * ntris < (1ll << 32), "arap: 32-bit vertex indices and list offsets");
  ISHAP_REQUIRE(scratch_bytes >= ishap_arap_scratch_bytes(nverts, ntris, ncons),
                "arap: scratch smaller than ishap_arap_scratch_bytes(nverts, ntris, ncons)");
  hipStream_t s = (hipStream_t)stream;
  const ArapLayout L = arap_layout(scratch, nverts, ntris);
  ArapState* st = L.st;
  unsigned *vt_off = L.vt_off, *vt_cur = L.vt_cur, *row = L.row, *totals = L.totals, *vt_list = L.vt_list, *cand = L.cand, *col = L.col;
  int *ccount = L.ccount, *has = L.has, *label = L.label, *role = L.role;
  double *w = L.w, *diag = L.diag, *x = L.x, *r = L.r, *z = L.z, *q = L.q, *R = L.R, *part = L.part;
  double* const* pbuf = L.pbuf;
  const int nv = (int)nverts, nc = (int)ncons, nb = (int)L.nb;
  const unsigned vb = (unsigned)L.nb, tb = (unsigned)((ntris + AB - 1) / AB);
  const unsigned t3b = (unsigned)((3 * ntris + AB - 1) / AB), cb = (unsigned)((ncons + AB - 1) / AB);

  // ---- ids in range and distinct, checked on the device before any kernel indexes with them
  ISHAP_CHECK_HIP(hipMemsetAsync(scratch, 0, (size_t)L.zero_end, s));
  hipLaunchKernelGGL(arap_check_tris_kernel, dim3(t3b), dim3(AB), 0, s, tris, 3 * ntris, nv, st);
  if (nc) hipLaunchKernelGGL(arap_check_cons_kernel, dim3(cb), dim3(AB), 0, s, cons_ids, nc, nv, ccount, st);
  ISHAP_CHECK_HIP(hipGetLastError());
  ArapState h;
  if (int e = read_state(st, h, s)) return e;
  ISHAP_REQUIRE(!(h.bad & 1), "arap: a triangle index outside [0, nverts)");
  ISHAP_REQUIRE(!(h.bad & 2), "arap: a constraint id outside [0, nverts)");
  ISHAP_REQUIRE(!(h.bad & 4), "arap: a repeated constraint id");

  // ---- adjacency and weights
  count_triangle_corners(tris, ntris, 1u, vt_off, s);
  scan_exclusive_u32(vt_off, nverts + 1, totals, nullptr, s);
  hipLaunchKernelGGL(arap_vt_fill_kernel, dim3(tb), dim3(AB), 0, s, tris, ntris, (const unsigned*)vt_off, vt_cur, vt_list);
  hipLaunchKernelGGL(arap_rows_kernel, dim3(vb), dim3(AB), 0, s, tris, nv, (const unsigned*)vt_off, vt_list, cand, row);
  scan_exclusive_u32(row, nverts + 1, totals, nullptr, s);
  hipLaunchKernelGGL(arap_weights_kernel, dim3(vb), dim3(AB), 0, s, rest, tris, nv, (const unsigned*)vt_off,
                     (const unsigned*)vt_list, (const unsigned*)cand, (const unsigned*)row, col, w, diag);

  // ---- components: rounds of four hook + jump sweeps until a round changes nothing (labels only decrease: it ends)
  hipLaunchKernelGGL(arap_label_init_kernel, dim3(vb), dim3(AB), 0, s, nv, label);
  for (;;) {
    ISHAP_CHECK_HIP(hipMemsetAsync(&st->changed, 0, sizeof(int), s));
    for (int k = 0; k < 4; ++k) {
      hipLaunchKernelGGL(arap_label_sweep_kernel, dim3(vb), dim3(AB), 0, s, nv, (const unsigned*)row, (const unsigned*)col,
                         (const double*)w, label, st);
      hipLaunchKernelGGL(arap_label_jump_kernel, dim3(vb), dim3(AB), 0, s, nv, label);
    }
    ISHAP_CHECK_HIP(hipGetLastError());
    if (int e = read_state(st, h, s)) return e;
    if (!h.changed) break;
  }
  if (nc) hipLaunchKernelGGL(arap_mark_kernel, dim3(cb), dim3(AB), 0, s, cons_ids, nc, (const int*)label, has);
  hipLaunchKernelGGL(arap_roles_kernel, dim3(vb), dim3(AB), 0, s, rest, nv, (const int*)ccount, (const int*)label,
                     (const int*)has, role, x, st);
  if (nc) hipLaunchKernelGGL(arap_targets_kernel, dim3(cb), dim3(AB), 0, s, cons_ids, cons_pos, nc, x);
  ISHAP_CHECK_HIP(hipGetLastError());
  if (int e = read_state(st, h, s)) return e;
  const long long dflt = 4ll * h.nfree + 100, cap = max_cg > 0 ? max_cg : (dflt < (1ll << 31) ? dflt : (1ll << 31) - 1);

  // ---- alternation
  for (int k = 0; k < max_iter; ++k) {
    hipLaunchKernelGGL(arap_local_kernel, dim3(vb), dim3(AB), 0, s, rest, nv, (const unsigned*)row, (const unsigned*)col,
                       (const double*)w, (const double*)x, R, part);
    hipLaunchKernelGGL(arap_energy_kernel, dim3(1), dim3(AB), 0, s, (const double*)part, nb, energy + k);
    hipLaunchKernelGGL(arap_rhs_kernel, dim3(vb), dim3(AB), 0, s, rest, nv, (const unsigned*)row, (const unsigned*)col,
                       (const double*)w, (const double*)diag, (const int*)role, (const double*)R, (const double*)x, r, z, pbuf[0],
                       part);
    hipLaunchKernelGGL(arap_cg_init_kernel, dim3(1), dim3(AB), 0, s, (const double*)part, nb, tol, st);
    ISHAP_CHECK_HIP(hipGetLastError());
    if (int e = read_state(st, h, s)) return e;
    int cur = 0;
    for (long long done_its = 0; !h.done && done_its < cap; done_its += ARAP_CHUNK) {
      for (int c = 0; c < ARAP_CHUNK; ++c) {
        hipLaunchKernelGGL(arap_cg_spmv_kernel, dim3(vb), dim3(AB), 0, s, nv, (const unsigned*)row, (const unsigned*)col,
                           (const double*)w, (const double*)diag, (const int*)role, (const double*)z, (const double*)pbuf[cur],
                           pbuf[cur ^ 1], q, (const ArapState*)st, part);
        hipLaunchKernelGGL(arap_cg_alpha_kernel, dim3(1), dim3(AB), 0, s, (const double*)part, nb, st);
        hipLaunchKernelGGL(arap_cg_update_kernel, dim3(vb), dim3(AB), 0, s, nv, (const double*)diag, (const int*)role,
                           (const double*)pbuf[cur ^ 1], (const double*)q, x, r, z, (const ArapState*)st, part);
        hipLaunchKernelGGL(arap_cg_beta_kernel, dim3(1), dim3(AB), 0, s, (const double*)part, nb, tol, (int)cap, st);
        cur ^= 1;
      }
      ISHAP_CHECK_HIP(hipGetLastError());
      if (int e = read_state(st, h, s)) return e;
    }
    hipLaunchKernelGGL(arap_cg_record_kernel, dim3(1), dim3(64), 0, s, (const ArapState*)st, cg_iters + k);
  }
  hipLaunchKernelGGL(arap_output_kernel, dim3(vb), dim3(AB), 0, s, (const double*)x, nv, out);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

extern "C" int ishap_nearest_vertices(const float* verts, long long nverts, const float* pts, long long npts, int* idx, void* stream) {
  ISHAP_REQUIRE(verts && pts && idx && nverts > 0 && npts > 0, "nearest_vertices arguments");
  ISHAP_REQUIRE(nverts < (1ll << 31), "nearest_vertices: vertex indices must fit 31 bits");
  hipLaunchKernelGGL(nearest_vertex_kernel, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pts, npts, verts,
                     nverts, idx);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
