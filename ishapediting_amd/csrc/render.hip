// Headless mesh rendering: colour, depth and triangle id per pixel (include/ishap.h: ishap_render_mesh, ishap_unproject).
//
// The reference shows and picks shapes through Open3D's scene widget (main.py:345-360 render_to_image / render_to_depth_image,
// :492-507 camera.unproject, :539-590 markers, :611-612 setup_camera); Open3D's renderer (Filament) is not a dependency here.
// This is a visibility-buffer rasteriser with its OWN statement of projection, coverage, depth and shading -- parity with
// Open3D's pictures is unpinned (as for surface.hip); what is pinned is the fp64 statement in tests/render_ref.py.
//
//   vertex pass   world -> view -> window in fp64, one thread per vertex.  x_win = W/2 + f x_v / z_v, y_win = H/2 - f y_v / z_v
//                 (row 0 is the top of the picture), f = (H/2) / tan(fov_y/2), z_v > 0 in front of the eye.  The window
//                 position is kept as integers in units of 2^-14 pixel, with 1/z_v as fp32.
//   raster pass   coverage at pixel centres (x + 0.5, y + 0.5) from 64-bit integer edge functions of those integers: exact,
//                 so the two triangles of a shared edge never both claim, and never both drop, a pixel (top-left fill rule:
//                 a centre exactly on an edge belongs to the triangle whose interior lies towards +x, or towards +y for a
//                 horizontal edge).  Both windings are drawn.  1/z is affine on the screen: interpolated with the screen
//                 barycentrics it is perspective-correct.  depth d = far/(far-near) (1 - near/z_v), fp32 in [0, 1); a pixel
//                 whose d reaches 1 (beyond `far`) is dropped.  Every covered pixel does ONE agent-scope 64-bit atomicMin of
//                 (bits(d) << 32 | triangle id): d >= 0 orders like its bits, ties go to the lowest id, arrival order is
//                 immaterial -- the picture is bitwise repeatable and independent of the triangle order.
//   resolve pass  one thread per pixel: unpack, recompute the barycentrics of the winning triangle, shade.
//
// Triangles that are SKIPPED (they draw nothing): any vertex nearer than `near` (z_v < near; there is no near-plane
// clipping -- a triangle that crosses the near plane disappears whole), any vertex further than 65536 pixels from the
// window origin (the guard band of the integer edge functions: beyond an 89.8 degree view angle at near = 0.1), zero screen
// area, a bounding box that holds no pixel centre of the picture, a vertex index outside [0, nverts).
//
// Work shape.  Small triangles (bounding box up to 16 x 16 pixels: the ~300 k triangles of a 256^3 surface are a few pixels
// each) take one lane each, straight after their setup.  Larger ones are appended to a list and drawn by a second launch of
// one workgroup per 64 x 16 pixel screen tile: the workgroup scans the list 256 entries at a time, keeps the entries whose
// box meets its tile, and draws each with all four waves, ONE WAVE PER PIXEL ROW of the tile -- a wave's atomic instruction
// covers 64 consecutive pixels, 512 contiguous bytes of the visibility buffer, the access shape atomics run fastest at,
// and no lane ever walks a large box alone (two screen-filling triangles at 1024^2: 1024 workgroups, 8 pixels per lane).
#include "render.h"
#include <cmath>

namespace {

constexpr int SUB_BITS = 14;                       // window positions in units of 2^-14 pixel
constexpr long long SUB_ONE = 1ll << SUB_BITS;
constexpr double GUARD_PX = 65536.0;               // |x_win|, |y_win| < 2^16 px: |X| < 2^30, every edge function < 2^63
constexpr int SMALL_BOX = 16;
constexpr int TILE_W = 64, TILE_H = 16;
constexpr unsigned long long VIS_EMPTY = 0x3F800000FFFFFFFFull;   // depth 1.0f, triangle -1

struct VRec {          // one vertex after the vertex pass, 16 bytes
  int X, Y;            // window position, units of 2^-14 pixel
  float w;             // 1 / z_view
  int ok;              // 0: nearer than `near`, outside the guard band, or not finite
};
struct LargeRec { int tri, xy0, xy1, pad; };   // a large triangle and its pixel box (x | y << 16)

struct Tri {
  // edge i is opposite vertex i; all three are scaled by the sign of the area, so inside is E > 0
  long long dx0, dy0, dx1, dy1, dx2, dy2;   // direction of edge i (b - a), sub-pixel units
  int xa0, ya0, xa1, ya1, xa2, ya2;         // start vertex of edge i
  float inv_area, w0, dw1, dw2;
  int bx0, by0, bx1, by1;                   // pixels whose centres lie inside the bounding box, clipped to the picture
};

__device__ __forceinline__ bool tri_setup(const VRec& a, const VRec& b, const VRec& c, int W, int H, Tri& t) {
  if (!(a.ok & b.ok & c.ok)) return false;
  const long long area = (long long)(b.X - a.X) * (c.Y - a.Y) - (long long)(b.Y - a.Y) * (c.X - a.X);
  if (area == 0) return false;
  const long long s = area > 0 ? 1 : -1;
  const int mnx = min(a.X, min(b.X, c.X)), mxx = max(a.X, max(b.X, c.X));
  const int mny = min(a.Y, min(b.Y, c.Y)), mxy = max(a.Y, max(b.Y, c.Y));
  const int half = (int)(SUB_ONE / 2);
  // pixel p's centre is (2p + 1) * half: inside [mn, mx] for ceil((mn - half) / one) <= p <= floor((mx - half) / one)
  t.bx0 = max((mnx - half + (int)SUB_ONE - 1) >> SUB_BITS, 0);
  t.by0 = max((mny - half + (int)SUB_ONE - 1) >> SUB_BITS, 0);
  t.bx1 = min((mxx - half) >> SUB_BITS, W - 1);
  t.by1 = min((mxy - half) >> SUB_BITS, H - 1);
  if (t.bx0 > t.bx1 || t.by0 > t.by1) return false;
  t.dx0 = s * (c.X - b.X); t.dy0 = s * (c.Y - b.Y); t.xa0 = b.X; t.ya0 = b.Y;
  t.dx1 = s * (a.X - c.X); t.dy1 = s * (a.Y - c.Y); t.xa1 = c.X; t.ya1 = c.Y;
  t.dx2 = s * (b.X - a.X); t.dy2 = s * (b.Y - a.Y); t.xa2 = a.X; t.ya2 = a.Y;
  t.inv_area = 1.f / (float)(s * area);
  t.w0 = a.w; t.dw1 = b.w - a.w; t.dw2 = c.w - a.w;
  return true;
}

// edge function of the centre of pixel (px, py): exact (|factor| < 2^31 each, the difference of the products < 2^63)
__device__ __forceinline__ long long edge_at(long long dx, long long dy, int xa, int ya, int px, int py) {
  const long long cxp = (2ll * px + 1) * (SUB_ONE / 2), cyp = (2ll * py + 1) * (SUB_ONE / 2);
  return dx * (cyp - ya) - dy * (cxp - xa);
}
// top-left rule: E rises by -dy per step in x and by dx per step in y
__device__ __forceinline__ bool edge_in(long long e, long long dx, long long dy) {
  return e > 0 || (e == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

struct DepthConst { float kf, near; };   // d = kf (1 - near w)

__device__ __forceinline__ void plot(const Tri& t, long long e0, long long e1, long long e2, DepthConst dc, unsigned tri,
                                     unsigned long long* px) {
  if (!(edge_in(e0, t.dx0, t.dy0) && edge_in(e1, t.dx1, t.dy1) && edge_in(e2, t.dx2, t.dy2))) return;
  const float b1 = (float)e1 * t.inv_area, b2 = (float)e2 * t.inv_area;
  const float w = fmaf(b2, t.dw2, fmaf(b1, t.dw1, t.w0));
  float d = dc.kf * (1.f - dc.near * w);
  d = d > 0.f ? d : 0.f;
  if (!(d < 1.f)) return;
  atomicMin(px, ((unsigned long long)__float_as_uint(d) << 32) | tri);   // agent scope: workgroups on every XCD meet here
}

__global__ __launch_bounds__(256) void render_clear_kernel(unsigned long long* vis, long long npix, unsigned* counter) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < npix) vis[i] = VIS_EMPTY;
  if (i == 0) *counter = 0;
}

__global__ __launch_bounds__(256) void render_vertex_kernel(const float* __restrict__ verts, long long nverts, RenderCam cam,
                                                            VRec* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nverts) return;
  const double px = (double)verts[3 * i] - cam.eye[0], py = (double)verts[3 * i + 1] - cam.eye[1],
               pz = (double)verts[3 * i + 2] - cam.eye[2];
  const double xv = px * cam.right[0] + py * cam.right[1] + pz * cam.right[2];
  const double yv = px * cam.upv[0] + py * cam.upv[1] + pz * cam.upv[2];
  const double zv = px * cam.fwd[0] + py * cam.fwd[1] + pz * cam.fwd[2];
  VRec r;
  r.X = 0; r.Y = 0; r.w = 0.f; r.ok = 0;
  if (zv >= cam.near) {                         // false for NaN too
    const double iz = 1.0 / zv;
    const double xw = cam.cx + cam.focal * xv * iz, yw = cam.cy - cam.focal * yv * iz;
    if (fabs(xw) < GUARD_PX && fabs(yw) < GUARD_PX) {
      r.X = (int)llrint(xw * (double)SUB_ONE);
      r.Y = (int)llrint(yw * (double)SUB_ONE);
      r.w = (float)iz;
      r.ok = 1;
    }
  }
  out[i] = r;
}

__device__ __forceinline__ bool load_tri(const int* __restrict__ tris, long long t, long long nverts, const VRec* __restrict__ vr,
                                         int W, int H, Tri& tri) {
  const int i0 = tris[3 * t], i1 = tris[3 * t + 1], i2 = tris[3 * t + 2];
  if ((unsigned)i0 >= (unsigned long long)nverts || (unsigned)i1 >= (unsigned long long)nverts ||
      (unsigned)i2 >= (unsigned long long)nverts)
    return false;
  return tri_setup(vr[i0], vr[i1], vr[i2], W, H, tri);
}

// setup of every triangle; the small ones are drawn here, one lane each, the rest go on the list
__global__ __launch_bounds__(256) void render_small_kernel(const int* __restrict__ tris, long long ntris, long long nverts,
                                                           const VRec* __restrict__ vr, int W, int H, DepthConst dc,
                                                           unsigned long long* __restrict__ vis, LargeRec* __restrict__ list,
                                                           unsigned* __restrict__ counter) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntris) return;
  Tri tri;
  if (!load_tri(tris, t, nverts, vr, W, H, tri)) return;
  if (tri.bx1 - tri.bx0 >= SMALL_BOX || tri.by1 - tri.by0 >= SMALL_BOX) {
    const unsigned slot = atomicAdd(counter, 1u);
    LargeRec r;
    r.tri = (int)t; r.xy0 = tri.bx0 | (tri.by0 << 16); r.xy1 = tri.bx1 | (tri.by1 << 16); r.pad = 0;
    list[slot] = r;
    return;
  }
  long long r0 = edge_at(tri.dx0, tri.dy0, tri.xa0, tri.ya0, tri.bx0, tri.by0);
  long long r1 = edge_at(tri.dx1, tri.dy1, tri.xa1, tri.ya1, tri.bx0, tri.by0);
  long long r2 = edge_at(tri.dx2, tri.dy2, tri.xa2, tri.ya2, tri.bx0, tri.by0);
  for (int y = tri.by0; y <= tri.by1; ++y) {
    long long e0 = r0, e1 = r1, e2 = r2;
    unsigned long long* row = vis + (long long)y * W;
    for (int x = tri.bx0; x <= tri.bx1; ++x) {
      plot(tri, e0, e1, e2, dc, (unsigned)t, row + x);
      e0 -= tri.dy0 * SUB_ONE; e1 -= tri.dy1 * SUB_ONE; e2 -= tri.dy2 * SUB_ONE;
    }
    r0 += tri.dx0 * SUB_ONE; r1 += tri.dx1 * SUB_ONE; r2 += tri.dx2 * SUB_ONE;
  }
}

// one workgroup per 64 x 16 pixel tile; wave v draws rows v, v + 4, v + 8, v + 12 of the tile, lane l column l
__global__ __launch_bounds__(256) void render_large_kernel(const int* __restrict__ tris, long long nverts,
                                                           const VRec* __restrict__ vr, int W, int H, DepthConst dc,
                                                           unsigned long long* __restrict__ vis, const LargeRec* __restrict__ list,
                                                           const unsigned* __restrict__ counter) {
  __shared__ int hits[256];
  __shared__ int nhit;
  const int tid = threadIdx.x;
  const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
  const int tx1 = min(tx0 + TILE_W, W) - 1, ty1 = min(ty0 + TILE_H, H) - 1;
  const int x = tx0 + (tid & 63), yrow = ty0 + (tid >> 6);
  const unsigned nlarge = *counter;
  if (tid == 0) nhit = 0;
  __syncthreads();
  for (unsigned base = 0; base < nlarge; base += 256) {
    if (base + tid < nlarge) {
      const LargeRec r = list[base + tid];
      const int bx0 = r.xy0 & 0xffff, by0 = r.xy0 >> 16, bx1 = r.xy1 & 0xffff, by1 = r.xy1 >> 16;
      if (bx0 <= tx1 && bx1 >= tx0 && by0 <= ty1 && by1 >= ty0) hits[atomicAdd(&nhit, 1)] = r.tri;
    }
    __syncthreads();
    const int n = nhit;
    for (int h = 0; h < n; ++h) {
      const int t = hits[h];
      Tri tri;
      if (!load_tri(tris, t, nverts, vr, W, H, tri)) continue;      // uniform over the workgroup
      if (x < tri.bx0 || x > tri.bx1) continue;
#pragma unroll
      for (int i = 0; i < TILE_H / 4; ++i) {
        const int y = yrow + 4 * i;
        if (y < tri.by0 || y > tri.by1) continue;
        plot(tri, edge_at(tri.dx0, tri.dy0, tri.xa0, tri.ya0, x, y), edge_at(tri.dx1, tri.dy1, tri.xa1, tri.ya1, x, y),
             edge_at(tri.dx2, tri.dy2, tri.xa2, tri.ya2, x, y), dc, (unsigned)t, vis + (long long)y * W + x);
      }
    }
    __syncthreads();
    if (tid == 0) nhit = 0;
    __syncthreads();
  }
}

struct ShadeCam { float eye[3]; };

__global__ __launch_bounds__(256) void render_resolve_kernel(const unsigned long long* __restrict__ vis, int W, int H,
                                                             const float* __restrict__ verts, const int* __restrict__ tris,
                                                             long long nverts, const float* __restrict__ normals,
                                                             const int* __restrict__ tri_part, const float* __restrict__ parts,
                                                             int nparts, const VRec* __restrict__ vr, ShadeCam sc,
                                                             unsigned char* __restrict__ rgb, float* __restrict__ depth,
                                                             int* __restrict__ tri_id) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)W * H) return;
  const unsigned long long key = vis[p];
  const int id = (int)(unsigned)(key & 0xffffffffull);
  if (depth) depth[p] = __uint_as_float((unsigned)(key >> 32));
  if (tri_id) tri_id[p] = id;
  if (!rgb) return;
  float cr = 0.f, cg = 0.f, cb = 0.f;
  Tri tri;
  if (id >= 0 && load_tri(tris, id, nverts, vr, W, H, tri)) {
    const int px = (int)(p % W), py = (int)(p / W);
    const int i0 = tris[3 * (long long)id], i1 = tris[3 * (long long)id + 1], i2 = tris[3 * (long long)id + 2];
    const float b1 = (float)edge_at(tri.dx1, tri.dy1, tri.xa1, tri.ya1, px, py) * tri.inv_area;
    const float b2 = (float)edge_at(tri.dx2, tri.dy2, tri.xa2, tri.ya2, px, py) * tri.inv_area;
    const float b0 = 1.f - b1 - b2;
    // perspective-correct weights of the vertex attributes: b_i w_i / sum
    const float q0 = b0 * tri.w0, q1 = b1 * (tri.w0 + tri.dw1), q2 = b2 * (tri.w0 + tri.dw2);
    const float iq = 1.f / (q0 + q1 + q2);
    const float g0 = q0 * iq, g1 = q1 * iq, g2 = q2 * iq;
    int part = tri_part ? tri_part[id] : 0;
    part = min(max(part, 0), nparts - 1);
    const float pr = parts[4 * part], pg = parts[4 * part + 1], pb = parts[4 * part + 2];
    float shade = 1.f;
    if (parts[4 * part + 3] != 0.f) {
      const float ax = verts[3 * (long long)i0], ay = verts[3 * (long long)i0 + 1], az = verts[3 * (long long)i0 + 2];
      const float bx = verts[3 * (long long)i1], by = verts[3 * (long long)i1 + 1], bz = verts[3 * (long long)i1 + 2];
      const float cx = verts[3 * (long long)i2], cy = verts[3 * (long long)i2 + 1], cz = verts[3 * (long long)i2 + 2];
      float nx, ny, nz;
      if (normals) {
        nx = g0 * normals[3 * (long long)i0] + g1 * normals[3 * (long long)i1] + g2 * normals[3 * (long long)i2];
        ny = g0 * normals[3 * (long long)i0 + 1] + g1 * normals[3 * (long long)i1 + 1] + g2 * normals[3 * (long long)i2 + 1];
        nz = g0 * normals[3 * (long long)i0 + 2] + g1 * normals[3 * (long long)i1 + 2] + g2 * normals[3 * (long long)i2 + 2];
      } else {
        const float ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
        nx = uy * vz - uz * vy; ny = uz * vx - ux * vz; nz = ux * vy - uy * vx;
      }
      const float ex = sc.eye[0] - (g0 * ax + g1 * bx + g2 * cx), ey = sc.eye[1] - (g0 * ay + g1 * by + g2 * cy),
                  ez = sc.eye[2] - (g0 * az + g1 * bz + g2 * cz);
      const float nn = nx * nx + ny * ny + nz * nz, ee = ex * ex + ey * ey + ez * ez;
      const float c = nn > 0.f && ee > 0.f ? fabsf(nx * ex + ny * ey + nz * ez) / sqrtf(nn * ee) : 0.f;
      shade = 0.25f + 0.75f * fminf(c, 1.f);
    }
    cr = pr * shade; cg = pg * shade; cb = pb * shade;
  }
  rgb[3 * p] = (unsigned char)rintf(fminf(fmaxf(cr, 0.f), 1.f) * 255.f);
  rgb[3 * p + 1] = (unsigned char)rintf(fminf(fmaxf(cg, 0.f), 1.f) * 255.f);
  rgb[3 * p + 2] = (unsigned char)rintf(fminf(fmaxf(cb, 0.f), 1.f) * 255.f);
}

__global__ __launch_bounds__(256) void render_unproject_kernel(RenderCam cam, const float* __restrict__ xyd, long long n,
                                                               float* __restrict__ world) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double xw = (double)xyd[3 * i] + 0.5, yw = (double)xyd[3 * i + 1] + 0.5, d = (double)xyd[3 * i + 2];
  const double zv = cam.near / (1.0 - d * (cam.far - cam.near) / cam.far);
  const double xv = (xw - cam.cx) * zv / cam.focal, yv = -(yw - cam.cy) * zv / cam.focal;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    world[3 * i + k] = (float)(cam.eye[k] + xv * cam.right[k] + yv * cam.upv[k] + zv * cam.fwd[k]);
}

// scratch layout: visibility keys u64[width height] | VRec[nverts] | LargeRec[ntris] | the list counter (16 bytes), each on a 16-byte boundary
struct RenderScratch { unsigned long long* vis; VRec* vr; LargeRec* list; unsigned* counter; long long bytes; };
RenderScratch render_scratch(void* base, long long nverts, long long ntris, int width, int height) {
  Carve c{(char*)base};
  return {c.take<unsigned long long>((long long)width * height, 16), c.take<VRec>(nverts, 16), c.take<LargeRec>(ntris, 16),
          c.take<unsigned>(4, 16), c.total(16)};
}

}  // namespace

long long render_scratch_bytes(long long nverts, long long ntris, int width, int height) {
  if (nverts < 0 || ntris < 0 || nverts >= (1ll << 31) || ntris >= (1ll << 31) || width < 1 || height < 1 ||
      width > RENDER_MAX_SIDE || height > RENDER_MAX_SIDE)
    return -1;
  return render_scratch(nullptr, nverts, ntris, width, height).bytes;
}

int render_camera(const float* eye, const float* centre, const float* up, float fov_y_deg, float near, float far, int width,
                  int height, RenderCam& out) {
  ISHAP_REQUIRE(width >= 1 && height >= 1 && width <= RENDER_MAX_SIDE && height <= RENDER_MAX_SIDE, "render: picture side in [1, 16384]");
  ISHAP_REQUIRE(fov_y_deg > 0.f && fov_y_deg < 180.f, "camera: fov_y_deg in (0, 180)");
  ISHAP_REQUIRE(near > 0.f && far > near, "camera: 0 < near < far");
  double f[3], r[3], u[3];
  for (int k = 0; k < 3; ++k) f[k] = (double)centre[k] - (double)eye[k];
  const double fl = std::sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  ISHAP_REQUIRE(fl > 0.0 && std::isfinite(fl), "camera: eye and centre coincide");
  for (int k = 0; k < 3; ++k) f[k] /= fl;
  r[0] = f[1] * up[2] - f[2] * up[1]; r[1] = f[2] * up[0] - f[0] * up[2]; r[2] = f[0] * up[1] - f[1] * up[0];
  const double rl = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  ISHAP_REQUIRE(rl > 0.0 && std::isfinite(rl), "camera: up is parallel to the view direction");
  for (int k = 0; k < 3; ++k) r[k] /= rl;
  u[0] = r[1] * f[2] - r[2] * f[1]; u[1] = r[2] * f[0] - r[0] * f[2]; u[2] = r[0] * f[1] - r[1] * f[0];
  for (int k = 0; k < 3; ++k) { out.eye[k] = eye[k]; out.right[k] = r[k]; out.upv[k] = u[k]; out.fwd[k] = f[k]; }
  out.focal = 0.5 * height / std::tan(0.5 * (double)fov_y_deg * 3.14159265358979323846 / 180.0);
  out.cx = 0.5 * width; out.cy = 0.5 * height;
  out.near = near; out.far = far;
  return 0;
}

int render_mesh_launch(const RenderArgs& a, hipStream_t s) {
  const long long npix = (long long)a.width * a.height;
  const RenderScratch S = render_scratch(a.scratch, a.nverts, a.ntris, a.width, a.height);
  unsigned long long* vis = S.vis;
  VRec* vr = S.vr; LargeRec* list = S.list; unsigned* counter = S.counter;
  const unsigned pb = (unsigned)((npix + 255) / 256);
  DepthConst dc;
  dc.kf = (float)(a.cam.far / (a.cam.far - a.cam.near)); dc.near = (float)a.cam.near;
  hipLaunchKernelGGL(render_clear_kernel, dim3(pb), dim3(256), 0, s, vis, npix, counter);
  if (a.nverts > 0 && a.ntris > 0) {
    hipLaunchKernelGGL(render_vertex_kernel, dim3((unsigned)((a.nverts + 255) / 256)), dim3(256), 0, s, a.verts, a.nverts, a.cam, vr);
    hipLaunchKernelGGL(render_small_kernel, dim3((unsigned)((a.ntris + 255) / 256)), dim3(256), 0, s, a.tris, a.ntris, a.nverts,
                       (const VRec*)vr, a.width, a.height, dc, vis, list, counter);
    hipLaunchKernelGGL(render_large_kernel, dim3((a.width + TILE_W - 1) / TILE_W, (a.height + TILE_H - 1) / TILE_H), dim3(256), 0, s,
                       a.tris, a.nverts, (const VRec*)vr, a.width, a.height, dc, vis, (const LargeRec*)list, (const unsigned*)counter);
  }
  ShadeCam sc;
  for (int k = 0; k < 3; ++k) sc.eye[k] = (float)a.cam.eye[k];
  hipLaunchKernelGGL(render_resolve_kernel, dim3(pb), dim3(256), 0, s, (const unsigned long long*)vis, a.width, a.height, a.verts,
                     a.tris, a.nverts, a.normals, a.tri_part, a.parts, a.nparts, (const VRec*)vr, sc, a.rgb, a.depth, a.tri_id);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

int render_unproject_launch(const RenderCam& cam, const float* xyd, long long n, float* world, hipStream_t s) {
  hipLaunchKernelGGL(render_unproject_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cam, xyd, n, world);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
