// Shadows of 3-D regions on the three triplane planes, and the weight map the drag loss's mask term reads (regions.h).
//
// Marks: one byte per plane texel, [3][W][W] indexed [plane][row][col] like the drag kernels' `touched`; bit 0 = in the shadow of
// the keep region, bit 1 = in the shadow of the free region.  Plane axes as plane_axes() of drag.hip: plane 0 col = x, row = y;
// plane 1 col = y, row = z; plane 2 col = x, row = z.
//   1. region_prim_kernel: a thread per texel evaluates the primitives (a small device array) at the texel centre, in double, and
//      stores its byte (plain store: every byte of the map is written, so the scratch needs no memset).
//   2. region_vox_*_kernel: a voxel grid [D][D][D] bytes, z fastest, is OR-reduced along the missing axis of each plane; the
//      fastest volume axis runs across lanes in all three.  A set voxel marks the texel NEAREST to it, by the integer map
//      t = (2 i (W - 1) + (D - 1)) / (2 (D - 1)): no float ties, and no holes because D >= W.  Byte-wide marks go through a 32-bit
//      atomicOr as drag_touch_one's do.
//   3. region_compose_kernel: Chebyshev dilation by d texels (clipped at the map), then keep / free / 1 -> the float map; counts
//      the undilated shadow texels for the caller's "empty region" check.
//   4. region_compose_marks_kernel: the same dilation, the marks themselves out (ishap_region_plane_marks); and
//      region_feather_kernel: from the squared distances to the two dilated shadows (edt.hip on the marks, one transform per
//      bit, axes = 6: three independent planes) and a host-built table of doubles to the feathered map
//      (ishap_region_plane_feather).
// Once per edit; nothing here is on the per-step path.
#include "regions.h"
#include "edt.h"

__device__ __forceinline__ int vox_to_texel(int i, int D, int W) { return (2 * i * (W - 1) + (D - 1)) / (2 * (D - 1)); }

__device__ __forceinline__ void region_mark(unsigned char* marks, int W, int p, int row, int col, unsigned bit) {
  const long long o = ((long long)p * W + row) * W + col;       // row, col in [0, W): vox_to_texel(D - 1) = W - 1
  atomicOr(reinterpret_cast<unsigned*>(marks + (o & ~3ll)), bit << (8 * (o & 3)));
}

__global__ void region_prim_kernel(const RegionPrim* __restrict__ prims, int n_prims, int W, unsigned char* __restrict__ marks) {
#pragma clang fp contract(off)      // the comparisons below are the statement's, operation by operation
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 3 * W * W) return;
  const int p = idx / (W * W), rem = idx - p * W * W, row = rem / W, col = rem - row * W;
  const int ac = (p == 1) ? 1 : 0, ar = (p == 0) ? 1 : 2;
  const double u = 2.0 * (double)col / (double)(W - 1) - 1.0, v = 2.0 * (double)row / (double)(W - 1) - 1.0;
  unsigned m = 0;
  for (int i = 0; i < n_prims; ++i) {
    const RegionPrim q = prims[i];
    bool in;
    if (q.kind == 0) {
      in = u >= q.a[ac] && u <= q.b[ac] && v >= q.a[ar] && v <= q.b[ar];
    } else {
      const double du = u - q.a[ac], dv = v - q.a[ar];
      in = du * du + dv * dv <= q.b[0] * q.b[0];
    }
    if (in) m |= q.role ? 2u : 1u;
  }
  marks[idx] = (unsigned char)m;
}

// plane 0 (col = x, row = y): OR over z.  A wave per z column, lanes over z.
__global__ __launch_bounds__(256) void region_vox_xy_kernel(const unsigned char* __restrict__ vox, int D, int W, unsigned bit,
                                                            unsigned char* __restrict__ marks) {
  const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (wave >= (long long)D * D) return;                           // wave-uniform
  const unsigned char* colp = vox + wave * D;
  unsigned any = 0;
  for (int z = lane; z < D; z += 64) any |= colp[z];
  if (__ballot(any != 0) != 0ull && lane == 0) {
    const int ix = (int)(wave / D), iy = (int)(wave - (long long)ix * D);
    region_mark(marks, W, 0, vox_to_texel(iy, D, W), vox_to_texel(ix, D, W), bit);
  }
}

// planes 1 (col = y, row = z: OR over x) and 2 (col = x, row = z: OR over y).  Lanes over z; a thread ORs VOX_RUN voxels along
// the missing axis (the run keeps enough threads in flight at D = 256) and marks once.
constexpr int VOX_RUN = 16;
__global__ __launch_bounds__(256) void region_vox_z_kernel(const unsigned char* __restrict__ vox, int D, int W, int plane, unsigned bit,
                                                           unsigned char* __restrict__ marks) {
  const int runs = (D + VOX_RUN - 1) / VOX_RUN;
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)runs * D * D) return;
  const int iz = (int)(idx % D);
  const int k = (int)((idx / D) % D);                 // the axis that stays: y for plane 1, x for plane 2
  const int run = (int)(idx / ((long long)D * D));
  const long long stride = plane == 1 ? (long long)D * D : (long long)D;          // step along the reduced axis (x / y)
  const long long base = (plane == 1 ? (long long)k * D : (long long)k * D * D) + iz;
  unsigned any = 0;
  const int j0 = run * VOX_RUN, j1 = min(j0 + VOX_RUN, D);
  for (int j = j0; j < j1; ++j) any |= vox[base + j * stride];
  if (any) region_mark(marks, W, plane, vox_to_texel(iz, D, W), vox_to_texel(k, D, W), bit);
}

__global__ __launch_bounds__(256) void region_compose_kernel(const unsigned char* __restrict__ marks, int W, int dilate, float keep_weight,
                                                             float free_weight, float* __restrict__ out, int* __restrict__ counts) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = idx < 3 * W * W;
  unsigned own = 0, m = 0;
  if (live) {
    const int p = idx / (W * W), rem = idx - p * W * W, row = rem / W, col = rem - row * W;
    own = marks[idx];
    const int r0 = max(row - dilate, 0), r1 = min(row + dilate, W - 1), c0 = max(col - dilate, 0), c1 = min(col + dilate, W - 1);
    for (int r = r0; r <= r1; ++r)
      for (int c = c0; c <= c1; ++c) m |= marks[(p * W + r) * W + c];
    out[idx] = (m & 1u) ? keep_weight : (m & 2u) ? free_weight : 1.f;       // keep overrides free
  }
  if (counts) {
    const int nk = __popcll(__ballot(own & 1u)), nf = __popcll(__ballot(own & 2u));
    if ((threadIdx.x & 63) == 0) {
      if (nk) atomicAdd(counts + 0, nk);
      if (nf) atomicAdd(counts + 1, nf);
    }
  }
}

long long region_scratch_bytes(int W) {
  if (W < 2) return -1;
  Carve c{nullptr};
  c.take<unsigned char>((size_t)3 * W * W);                    // the marks; the tail keeps the last 32-bit atomicOr inside
  return c.total();
}

int region_plane_weights_launch(const RegionPrim* prims, int n_prims, const unsigned char* keep_vox, const unsigned char* free_vox,
                                int D, int W, int dilate, float keep_weight, float free_weight, float* weights_out, int* counts,
                                void* scratch, hipStream_t s) {
  unsigned char* marks = (unsigned char*)scratch;
  const int ntex = 3 * W * W;
  if (counts) ISHAP_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int), s));
  hipLaunchKernelGGL(region_prim_kernel, dim3(ceil_div(ntex, 256)), dim3(256), 0, s, prims, n_prims, W, marks);
  const unsigned char* vox[2] = {keep_vox, free_vox};
  for (int role = 0; role < 2; ++role) {
    if (!vox[role]) continue;
    const unsigned bit = role ? 2u : 1u;
    const long long waves = (long long)D * D;
    hipLaunchKernelGGL(region_vox_xy_kernel, dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0, s, vox[role], D, W, bit, marks);
    const long long nthr = (long long)((D + VOX_RUN - 1) / VOX_RUN) * D * D;
    for (int plane = 1; plane <= 2; ++plane)
      hipLaunchKernelGGL(region_vox_z_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, vox[role], D, W, plane, bit, marks);
  }
  hipLaunchKernelGGL(region_compose_kernel, dim3(ceil_div(ntex, 256)), dim3(256), 0, s, (const unsigned char*)marks, W, dilate,
                     keep_weight, free_weight, weights_out, counts);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

// ---- the marks after dilation, and the feathered map (ABI 23)
__global__ __launch_bounds__(256) void region_compose_marks_kernel(const unsigned char* __restrict__ marks, int W, int dilate,
                                                                   unsigned char* __restrict__ out, int* __restrict__ counts) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = idx < 3 * W * W;
  unsigned own = 0, m = 0;
  if (live) {
    const int p = idx / (W * W), rem = idx - p * W * W, row = rem / W, col = rem - row * W;
    own = marks[idx];
    const int r0 = max(row - dilate, 0), r1 = min(row + dilate, W - 1), c0 = max(col - dilate, 0), c1 = min(col + dilate, W - 1);
    for (int r = r0; r <= r1; ++r)
      for (int c = c0; c <= c1; ++c) m |= marks[(p * W + r) * W + c];
    out[idx] = (unsigned char)(m & 3u);
  }
  if (counts) {
    const int nk = __popcll(__ballot(own & 1u)), nf = __popcll(__ballot(own & 2u));
    if ((threadIdx.x & 63) == 0) {
      if (nk) atomicAdd(counts + 0, nk);
      if (nf) atomicAdd(counts + 1, nf);
    }
  }
}

// dk, df: squared texel distances to the keep / free shadow (EDT_INF: the plane has none).  table[d2], d2 < table_len, is
// A = max(0, 1 - sqrt(d2) / falloff) in double from the host; beyond the table A = 0.  The blend is formed in double as
// written, operation by operation, and rounded once.
__global__ __launch_bounds__(256) void region_feather_kernel(const int* __restrict__ dk, const int* __restrict__ df,
                                                             const double* __restrict__ table, int table_len, int ntex, float keep_weight,
                                                             float free_weight, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= ntex) return;
  const int k2 = dk[idx], f2 = df[idx];
  const double ak = k2 < table_len ? table[k2] : 0.0, af = f2 < table_len ? table[f2] : 0.0;
  float w;
  if (ak == 1.0) w = keep_weight;
  else if (ak == 0.0 && af == 1.0) w = free_weight;
  else if (ak == 0.0 && af == 0.0) w = 1.f;
  else {
    const double hold = 1.0 + ((double)keep_weight - 1.0) * ak;
    const double loose = (((double)free_weight - 1.0) * af) * (1.0 - ak);
    w = (float)(hold + loose);
  }
  out[idx] = w;
}

// the shadows of region_plane_weights_launch, undilated, into `raw`
static void region_shadows_launch(const RegionPrim* prims, int n_prims, const unsigned char* keep_vox, const unsigned char* free_vox, int D,
                                  int W, unsigned char* raw, hipStream_t s) {
  const int ntex = 3 * W * W;
  hipLaunchKernelGGL(region_prim_kernel, dim3(ceil_div(ntex, 256)), dim3(256), 0, s, prims, n_prims, W, raw);
  const unsigned char* vox[2] = {keep_vox, free_vox};
  for (int role = 0; role < 2; ++role) {
    if (!vox[role]) continue;
    const unsigned bit = role ? 2u : 1u;
    const long long waves = (long long)D * D;
    hipLaunchKernelGGL(region_vox_xy_kernel, dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0, s, vox[role], D, W, bit, raw);
    const long long nthr = (long long)((D + VOX_RUN - 1) / VOX_RUN) * D * D;
    for (int plane = 1; plane <= 2; ++plane)
      hipLaunchKernelGGL(region_vox_z_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, vox[role], D, W, plane, bit, raw);
  }
}

int region_plane_marks_launch(const RegionPrim* prims, int n_prims, const unsigned char* keep_vox, const unsigned char* free_vox, int D,
                              int W, int dilate, unsigned char* marks_out, int* counts, void* scratch, hipStream_t s) {
  unsigned char* raw = (unsigned char*)scratch;
  if (counts) ISHAP_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int), s));
  region_shadows_launch(prims, n_prims, keep_vox, free_vox, D, W, raw, s);
  hipLaunchKernelGGL(region_compose_marks_kernel, dim3(ceil_div(3 * W * W, 256)), dim3(256), 0, s, (const unsigned char*)raw, W, dilate,
                     marks_out, counts);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

// scratch: raw marks | dilated marks | dk int[3 W W] | df int[3 W W] | the transform's own scratch
namespace {
struct FeatherLayout { void* raw; unsigned char* marks; int *dk, *df; void* edt; long long bytes; };
FeatherLayout feather_layout(void* base, int W) {
  Carve c{(char*)base};
  const long long ntex = 3ll * W * W;
  return {c.bytes(region_scratch_bytes(W)), c.take<unsigned char>(ntex), c.take<int>(ntex), c.take<int>(ntex),
          c.bytes(edt_scratch_bytes(3, W, W, 6)), c.total()};
}
}  // namespace

long long region_feather_scratch_bytes(int W) {
  if (W < 2 || W > EDT_MAX_AXIS) return -1;
  return feather_layout(nullptr, W).bytes;
}

int region_plane_feather_launch(const RegionPrim* prims, int n_prims, const unsigned char* keep_vox, const unsigned char* free_vox, int D,
                                int W, int dilate, float keep_weight, float free_weight, const double* table, int table_len,
                                float* weights_out, int* counts, void* scratch, hipStream_t s) {
  const FeatherLayout L = feather_layout(scratch, W);
  unsigned char* marks = L.marks;
  int *dk = L.dk, *df = L.df;
  ISHAP_TRY(region_plane_marks_launch(prims, n_prims, keep_vox, free_vox, D, W, dilate, marks, counts, L.raw, s));
  ISHAP_TRY(edt_launch(marks, 1u, 3, W, W, 6, 0, dk, L.edt, s));
  ISHAP_TRY(edt_launch(marks, 2u, 3, W, W, 6, 0, df, L.edt, s));
  const int ntex = 3 * W * W;
  hipLaunchKernelGGL(region_feather_kernel, dim3(ceil_div(ntex, 256)), dim3(256), 0, s, (const int*)dk, (const int*)df, table, table_len,
                     ntex, keep_weight, free_weight, weights_out);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
