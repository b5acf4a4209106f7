// GroupNorm32 (+ SiLU) and its input gradient as stand-alone C-ABI calls, with the statistics route selectable.
// Reference: guided_diffusion/nn.py:16-18,92-99 (GroupNorm32: 32 groups, eps 1e-5, computed on x.float()) followed by
// nn.SiLU (unet.py:179-183), and what autograd derives for them (drag_utils.py:383).
// The UNet executor picks a route per map size; these entry points run ANY route on a caller-given tensor so that the
// reference's own primitive fixtures (golden G3b / G15: group means up to 1000x the group spread) reach every one of them:
//   1  two-pass statistics (gn_partial / gn_finalize, double) + the full-map apply kernel
//   2  group-local kernel, one workgroup per (image, group)
//   3  group-local kernel, several workgroups per (image, group) meeting in the in-launch rendezvous
//   4  statistics as 64-bit fixed-point per-channel sums gathered in an implicit-GEMM epilogue (an identity 1x1
//      convolution stands in for the producing layer) + the apply kernel's finalise prologue  -- the route of the 128^2 / 64^2 maps
//   0  what the executor would pick for this map
#include "../../include/ishap.h"
#include "norm.h"
#include <cstring>

namespace {

struct Carve {
  char* base;
  size_t off = 0;
  template <typename T>
  T* take(size_t count) {
    off = align_up(off, 256);
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += count * sizeof(T);
    return p;
  }
};
struct Scratch {
  unsigned long long* rec;
  long long* csums;
  size_t zero_bytes;       // rec + csums: zeroed per call
  float* partial;
  half_t* ident;
  half_t* copy;
  size_t total;
};
Scratch carve(void* base, int N, int HW, int C) {
  Carve c{(char*)base};
  Scratch s;
  s.rec = c.take<unsigned long long>((size_t)N * 32 * GN_REC_STRIDE);
  s.csums = c.take<long long>((size_t)N * C * 2);
  s.zero_bytes = align_up(c.off, 256);
  s.partial = c.take<float>(gn_partial_floats(N, HW, C) + 64);
  s.ident = c.take<half_t>((size_t)align_up((size_t)C, 128) * C);
  s.copy = c.take<half_t>((size_t)N * HW * C);
  s.total = align_up(c.off, 256);
  return s;
}

__global__ void identity_fill_kernel(half_t* w, int C, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows * C) w[i] = (i / C == i % C) ? (half_t)1.f : (half_t)0.f;
}

// route 0: what the executor picks for this map (gn_route; ISHAP_LOCAL_GN=0 included)
int resolve_route(int route, int HW, int C, bool backward) {
  if (route != 0) return route;
  return gn_route(HW, C, GB_SAME, backward) == GnRoute::local ? 3 : (backward ? 1 : 4);
}

}  // namespace

extern "C" {

long long ishap_group_norm32_scratch_bytes(int N, int HW, int C) {
  if (N < 1 || HW < 1 || C < 32) return 0;
  return (long long)carve(nullptr, N, HW, C).total;
}

int ishap_group_norm32(const void* x_nhwc_f16, const float* gamma, const float* beta, int N, int H, int W, int C, int silu,
                       int route, void* y_nhwc_f16, float* stats, void* scratch, void* stream) {
  ISHAP_REQUIRE(x_nhwc_f16 && gamma && beta && y_nhwc_f16 && stats && scratch, "null argument");
  ISHAP_REQUIRE(N >= 1 && N <= 16 && H >= 1 && W >= 1 && C % 32 == 0, "GroupNorm32 dims");
  ISHAP_REQUIRE(route >= 0 && route <= 4, "route 0..4");
  ISHAP_TRY(ishap_check_status());
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  const Scratch sc = carve(scratch, N, HW, C);
  ISHAP_CHECK_HIP(hipMemsetAsync(scratch, 0, sc.zero_bytes, s));
  route = resolve_route(route, HW, C, false);
  GnApplyArgs g;
  g.x = (const half_t*)x_nhwc_f16; g.out = (half_t*)y_nhwc_f16; g.gamma = gamma; g.beta = beta;
  g.N = N; g.H = H; g.W = W; g.C = C; g.act = silu;
  if (route == 2 || route == 3) {
    // route 3 (several workgroups per group meeting inside the launch) needs the device's rendezvous tenancy (common.h);
    // while another context / stream of the process holds it the call degrades to one workgroup per group (route 2)
    TenancyScope tenancy(nullptr, s, false, route == 3);
    g.stats_out = stats;
    return gn_local_launch(gn_local_fill(g, SlabSrc{}, tenancy.granted ? sc.rec : nullptr), s);
  }
  if (route == 1) {
    ISHAP_TRY(gn_stats_launch(g.x, sc.partial, stats, N, HW, C, s));
    g.stats = stats;
  } else {
    // producer stand-in: copy = x * I through the implicit-GEMM kernel, whose epilogue gathers the per-channel sums
    // the epilogue credits a tile's sums to ONE image (n_img = m0 / HW): a tile must not straddle images.  The launcher only
    // takes 128-row tiles when H*W % 128 == 0 (igemm.hip), so 64-row tiles are what has to divide an image here
    ISHAP_REQUIRE(C % 64 == 0 && ((long long)N * HW) % 64 == 0 && (N == 1 || HW % 64 == 0), "route 4: C % 64 == 0, N*H*W % 64 == 0, and H*W % 64 == 0 at batch > 1");
    const int rows = (int)align_up((size_t)C, 128);
    hipLaunchKernelGGL(identity_fill_kernel, dim3((rows * C + 255) / 256), dim3(256), 0, s, sc.ident, C, rows);
    ISHAP_CHECK_HIP(hipGetLastError());
    IgemmArgs a;
    a.X = g.x; a.Wt = sc.ident; a.out = sc.copy; a.M = N * HW; a.N = C; a.K = C; a.conv3 = 0; a.Cin = C;
    a.ldx = C; a.ldw = C; a.ldo = C; a.H = H; a.W = W; a.out_mode = IG_OUT_F16; a.ksplit = 1;
    a.stat_out = sc.csums;
    ISHAP_TRY(igemm_launch(a, s));
    g.x = sc.copy; g.sums = sc.csums; g.stats_out = stats;
  }
  return gn_apply_launch(g, s);
}

int ishap_group_norm32_backward(const void* g_nhwc_f16, const void* x_nhwc_f16, const float* stats, const float* gamma,
                                const float* beta, int N, int H, int W, int C, int silu, int route, void* dx_nhwc_f16,
                                void* scratch, void* stream) {
  ISHAP_REQUIRE(g_nhwc_f16 && x_nhwc_f16 && stats && gamma && beta && dx_nhwc_f16 && scratch, "null argument");
  ISHAP_REQUIRE(N >= 1 && N <= 16 && H >= 1 && W >= 1 && C % 32 == 0, "GroupNorm32 dims");
  ISHAP_REQUIRE(route >= 0 && route <= 3, "backward route 0..3");
  ISHAP_TRY(ishap_check_status());
  hipStream_t s = (hipStream_t)stream;
  const int HW = H * W;
  const Scratch sc = carve(scratch, N, HW, C);
  ISHAP_CHECK_HIP(hipMemsetAsync(scratch, 0, sc.zero_bytes, s));
  route = resolve_route(route, HW, C, true);
  GnBwdArgs a;
  a.g = (const half_t*)g_nhwc_f16; a.x = (const half_t*)x_nhwc_f16; a.dx = (half_t*)dx_nhwc_f16;
  a.stats = stats; a.gamma = gamma; a.beta = beta; a.N = N; a.H = H; a.W = W; a.C = C; a.film = 0; a.act = silu;
  a.gmode = GB_SAME;
  if (route == 2 || route == 3) {
    TenancyScope tenancy(nullptr, s, false, route == 3);
    return gn_bwd_local_launch(gn_bwd_local_fill(a, SlabSrc{}, tenancy.granted ? sc.rec : nullptr), s);
  }
  a.csums = sc.csums;
  return gn_backward_launch(a, s);
}

/* CPU view of the plan (include/ishap.h): the route, kernel and launch geometry one GroupNorm pass of this shape gets */
int ishap_group_norm32_plan(int N, int H, int W, int C, int backward, int pending, int film, int act, int pool, int gmode, int route,
                            int* route_out, int* parts, int* vec, int* threads, int* grid_x, int* grid_y, int* lds_bytes,
                            int* xcd, char* kernel, int kernel_cap) {
  ISHAP_REQUIRE(N >= 1 && H >= 1 && W >= 1 && C >= 32 && C % 32 == 0, "GroupNorm32 dims");
  ISHAP_REQUIRE(route >= 0 && route <= (backward ? 3 : 4), "route 0..4 (backward: 0..3)");
  ISHAP_REQUIRE(gmode == GB_SAME || (backward && (gmode == GB_UNPOOL || gmode == GB_SUM4)), "gmode: a backward pass's GB_*");
  ISHAP_REQUIRE(!pool || (!backward && !film && act && H % 2 == 0 && W % 2 == 0), "pool variant: forward, SiLU, no FiLM");
  ISHAP_REQUIRE(!film || act, "FiLM is followed by SiLU");
  const int HW = H * W;
  if (route == 0) route = gn_route(HW, C, gmode, backward != 0) == GnRoute::local ? 3 : (backward ? 1 : 4);
  GnLocalPlan p;
  GnLaunchInfo full;
  const bool local = route == 2 || route == 3;
  if (local) {
    ISHAP_REQUIRE(backward ? gn_bwd_local_fits(HW, C, gmode) : gn_local_fits(HW, C), "group does not fit in LDS");
    GnLocalShape q;
    q.N = N; q.H = H; q.W = W; q.C = C; q.backward = backward != 0; q.pending = pending != 0; q.have_rec = route == 3;
    q.film = film; q.act = act; q.pool = pool; q.gmode = gmode;
    p = gn_local_plan(q);
  } else if (backward) {
    GnBwdArgs a;
    a.N = N; a.H = H; a.W = W; a.C = C; a.film = film; a.act = act; a.gmode = gmode;
    ISHAP_TRY(gn_backward_launch(a, nullptr, &full));
  } else {
    static const long long sums = 0;               // the launcher only asks whether the producer gathered the sums (route 4)
    GnApplyArgs a;
    a.N = N; a.H = H; a.W = W; a.C = C; a.film = film; a.act = act; a.pool = pool; a.sums = route == 4 ? &sums : nullptr;
    ISHAP_TRY(gn_apply_launch(a, nullptr, &full));
  }
  const std::string name = local ? gn_local_kernel_name(p) : full.kernel;
  if (route_out) *route_out = route;
  if (parts) *parts = local ? p.parts : 0;         // 0: not a group-local launch
  if (vec) *vec = local ? p.vec : 8;
  if (threads) *threads = local ? p.threads : full.threads;
  if (grid_x) *grid_x = local ? 32 * p.parts : full.grid_x;
  if (grid_y) *grid_y = local ? N : 1;
  if (lds_bytes) *lds_bytes = local ? p.lds_bytes : 0;
  if (xcd) *xcd = local ? p.xcd : 0;
  if (kernel) {
    if ((int)name.size() + 1 > kernel_cap) return -2;
    memcpy(kernel, name.c_str(), name.size() + 1);
  }
  return 0;
}

}  // extern "C"
