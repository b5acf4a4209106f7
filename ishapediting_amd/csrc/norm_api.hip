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
  s.zero_bytes = c.total();
  s.partial = c.take<float>(gn_partial_floats(N, HW, C) + 64);
  s.ident = c.take<half_t>((size_t)align_up((size_t)C, 128) * C);
  s.copy = c.take<half_t>((size_t)N * HW * C);
  s.total = c.total();
  return s;
}

__global__ void identity_fill_kernel(half_t* w, int C, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows * C) w[i] = (i / C == i % C) ? (half_t)1.f : (half_t)0.f;
}

}  // namespace

extern "C" {

long long ishap_group_norm32_scratch_bytes(int N, int HW, int C) {
  if (N < 1 || HW < 1 || C < 32) return 0;
  return (long long)carve(nullptr, N, HW, C).total;
}

// One GroupNorm launch, described by the caller field by field (include/ishap.h): the descriptor is checked against the contract of
// the kernels it would reach before any HIP call, turned into the GnApplyArgs / GnBwdArgs (+ SlabSrc) the executor builds
// (gn_forward_op in unet.hip, conv_gn_norm in backward.hip) and handed to the launchers the executor calls.  launch == 0 stops
// after the plan: route, parts and kernel name, no HIP call.
int ishap_group_norm32_run(const ishap_group_norm_desc* d, int launch, void* stream, int* route_out, int* parts_out, char* kernel,
                           int kernel_cap) {
  ISHAP_REQUIRE(d != nullptr, "descriptor");
  ISHAP_REQUIRE(d->backward == 0 || d->backward == 1, "backward: 0 forward, 1 input gradient");
  const bool bwd = d->backward != 0;
  const int N = d->N, H = d->H, W = d->W, C = d->C;
  ISHAP_REQUIRE(N >= 1 && N <= 16 && H >= 1 && W >= 1 && C % 32 == 0, "GroupNorm32 dims");
  ISHAP_REQUIRE(C >= 32 && H <= 4096 && W <= 4096 && (long long)N * H * W * (C / 8) < (1ll << 31), "GroupNorm32 dims: 32-bit vector index");
  ISHAP_REQUIRE(d->route >= 0 && d->route <= (bwd ? 3 : 4), bwd ? "backward route 0..3" : "route 0..4");
  ISHAP_REQUIRE(!bwd || (d->gmode >= GB_SAME && d->gmode <= GB_SUM4), "gmode: 0 same, 1 unpool, 2 sum of four");
  ISHAP_REQUIRE(d->gamma && d->beta && d->scratch, "null argument");
  ISHAP_REQUIRE(!d->film || d->act, "FiLM is followed by SiLU");
  ISHAP_REQUIRE(!d->film || (d->emb && d->emb_ld >= 2 * C), "FiLM rows: emb with emb_ld >= 2 C");
  const int HW = H * W, gmode = bwd ? d->gmode : GB_SAME;
  int route = d->route;
  if (route == 0) route = (!d->split && gn_route(HW, C, gmode, bwd) == GnRoute::local) ? 3 : (bwd ? 1 : 4);
  const bool local = route == 2 || route == 3;
  ISHAP_REQUIRE(local || route == 4 || C <= 2048, "two-pass routes: at most 2048 channels");
  const bool pending = d->nslab != 0 || d->ws != nullptr;
  SlabSrc slab;
  if (pending) {
    ISHAP_REQUIRE(local, "a pending source is added up by the group-local kernels only (routes 2, 3)");
    const int ld = bwd ? C : (d->x2 ? d->csplit : C);
    const long long rows = (long long)N * (gmode == GB_UNPOOL ? HW / 4 : gmode == GB_SUM4 ? HW * 4 : HW);
    ISHAP_REQUIRE(d->ws && d->nslab >= 1 && d->nslab <= 64 && d->zstride >= rows * ld, "pending source: ws, 1..64 slices, zstride >= rows * channels");
    ISHAP_REQUIRE(!bwd || (!d->bias && !d->bias2 && !d->res), "a pending gradient has neither bias nor residual");
    ISHAP_REQUIRE(!d->res || d->ldr >= ld, "pending residual: ldr >= channels");
    ISHAP_REQUIRE(d->res ? (!d->res_ups || (H % 2 == 0 && W % 2 == 0)) : !d->res_ups, "res_ups: a residual at (H/2, W/2), even H and W");
    slab.ws = d->ws; slab.nslab = d->nslab; slab.zstride = d->zstride; slab.bias = d->bias; slab.bias2 = d->bias2;
    slab.res = (const half_t*)d->res; slab.ldr = d->ldr; slab.res_ups = d->res_ups;
  } else {
    ISHAP_REQUIRE(!d->bias && !d->bias2 && !d->res && !d->ya, "bias, bias2, res and ya belong to a pending source");
  }
  ISHAP_REQUIRE(d->csplit >= 0 && d->csplit < C && d->csplit % 8 == 0, "csplit: a multiple of 8 below C");
  ISHAP_REQUIRE(!local || d->csplit % 32 == 0, "csplit on a group-local route: a multiple of 32");
  const Scratch sc = carve(d->scratch, N, HW, C);
  hipStream_t s = (hipStream_t)stream;
  std::string name;
  int parts = 0;
  auto report = [&]() -> int {
    if (route_out) *route_out = route;
    if (parts_out) *parts_out = parts;
    if (kernel) {
      ISHAP_REQUIRE((int)name.size() < kernel_cap, "kernel: name buffer too small");
      memcpy(kernel, name.c_str(), name.size() + 1);
    }
    return 0;
  };
  auto begin = [&]() -> int {          // every launching path: an earlier launch's device-side failure surfaces, the scratch is zeroed
    ISHAP_TRY(ishap_check_status());
    ISHAP_CHECK_HIP(hipMemsetAsync(d->scratch, 0, sc.zero_bytes, s));
    return 0;
  };

  if (!bwd) {
    ISHAP_REQUIRE(d->out != nullptr, "null argument: out");
    ISHAP_REQUIRE(pending ? (!d->x && d->ya) : d->x != nullptr, "input: x, or pending slices with ya and no x");
    ISHAP_REQUIRE((d->x2 != nullptr) == (d->csplit != 0) && (d->x2 != nullptr) == (d->xcopy != nullptr),
                  "lazy concatenation: x2, csplit and xcopy go together");
    ISHAP_REQUIRE(!d->pool || (H % 2 == 0 && W % 2 == 0), "pool: even H and W");
    ISHAP_REQUIRE(!d->pool || (d->act && !d->film), "pool variant: SiLU, no FiLM");
    ISHAP_REQUIRE(d->pool || !d->xpool, "xpool belongs to the pool variant");
    ISHAP_REQUIRE(!d->split || !local, "the split form has no group-local kernel");
    ISHAP_REQUIRE(!d->split || (d->act && !d->film && !d->pool), "split variant: SiLU, no FiLM, no pool");
    ISHAP_REQUIRE(!d->x2 || (!d->pool && !d->split), "lazy concatenation: plain variant only");
    ISHAP_REQUIRE(!d->x2 || local || (route == 4 && d->sums && d->sums2), "lazy concatenation on the full map: route 4 with sums and sums2");
    ISHAP_REQUIRE((!d->sums && !d->sums2) || route == 4, "sums: route 4 only");
    ISHAP_REQUIRE(!d->sums2 || (d->sums && d->x2), "sums2: the second source's, beside sums");
    ISHAP_REQUIRE(route != 1 || d->stats_out, "route 1: stats_out receives the two-pass statistics");
    ISHAP_REQUIRE(!local || gn_local_fits(HW, C), "group does not fit in LDS");
    const bool stand_in = route == 4 && !d->sums;
    // the stand-in producer's epilogue credits a tile's sums to ONE image (n_img = m0 / HW): a tile must not straddle images.  The
    // launcher only takes 128-row tiles when H*W % 128 == 0 (igemm.hip), so 64-row tiles are what has to divide an image here
    ISHAP_REQUIRE(!stand_in || (C % 64 == 0 && ((long long)N * HW) % 64 == 0 && (N == 1 || HW % 64 == 0)),
                  "route 4: C % 64 == 0, N*H*W % 64 == 0, and H*W % 64 == 0 at batch > 1");
    GnApplyArgs g;
    g.x = (const half_t*)(pending ? d->ya : d->x); g.out = (half_t*)d->out; g.xpool = (half_t*)d->xpool; g.stats_out = d->stats_out;
    g.gamma = d->gamma; g.beta = d->beta; g.emb = d->film ? d->emb : nullptr; g.emb_ld = d->film ? d->emb_ld : 0;
    g.N = N; g.H = H; g.W = W; g.C = C; g.film = d->film; g.act = d->act; g.pool = d->pool; g.split = d->split;
    g.x2 = (const half_t*)d->x2; g.csplit = d->csplit; g.xcopy = (half_t*)d->xcopy;
    if (local) {
      // route 3 (several workgroups per group meeting inside the launch) needs the device's rendezvous tenancy (common.h);
      // while another context / stream of the process holds it the call degrades to one workgroup per group (route 2)
      if (launch) ISHAP_TRY(begin());
      TenancyScope tenancy(nullptr, s, !launch, route == 3);
      const bool rec = launch ? tenancy.granted : route == 3;
      const GnLocalArgs la = gn_local_fill(g, slab, rec ? sc.rec : nullptr);
      const GnLocalPlan p = gn_local_plan(gn_local_shape(la));
      name = gn_local_kernel_name(p);
      parts = p.parts;
      ISHAP_TRY(report());
      return launch ? gn_local_launch(la, s) : 0;
    }
    g.sums = route == 4 ? (d->sums ? d->sums : sc.csums) : nullptr;
    g.sums2 = d->sums2;
    GnLaunchInfo info;
    ISHAP_TRY(gn_apply_launch(g, nullptr, &info));
    name = info.kernel;
    ISHAP_TRY(report());
    if (!launch) return 0;
    ISHAP_TRY(begin());
    if (route == 1) {
      ISHAP_TRY(gn_stats_launch(g.x, sc.partial, d->stats_out, N, HW, C, s));
      g.stats = d->stats_out;
      g.stats_out = nullptr;
    } else if (stand_in) {
      // producer stand-in: copy = x * I through the implicit-GEMM kernel, whose epilogue gathers the per-channel sums
      const int rows = (int)align_up((size_t)C, 128);
      hipLaunchKernelGGL(identity_fill_kernel, dim3((rows * C + 255) / 256), dim3(256), 0, s, sc.ident, C, rows);
      ISHAP_CHECK_HIP(hipGetLastError());
      IgemmArgs a;
      a.X = g.x; a.Wt = sc.ident; a.out = sc.copy; a.M = N * HW; a.N = C; a.K = C; a.conv3 = 0; a.Cin = C;
      a.ldx = C; a.ldw = C; a.ldo = C; a.H = H; a.W = W; a.out_mode = IG_OUT_F16; a.ksplit = 1;
      a.stat_out = sc.csums;
      ISHAP_TRY(igemm_launch(a, s));
      g.x = sc.copy;
    }
    return gn_apply_launch(g, s);
  }

  ISHAP_REQUIRE(d->x && d->stats && d->dx, "null argument: x, stats, dx");
  ISHAP_REQUIRE(pending ? !d->g : d->g != nullptr, "upstream gradient: g, or pending slices and no g");
  ISHAP_REQUIRE(!d->pool && !d->split, "pool and split are forward options");
  ISHAP_REQUIRE(gmode != GB_UNPOOL || (H % 2 == 0 && W % 2 == 0), "GB_UNPOOL: even H and W");
  ISHAP_REQUIRE((d->csplit != 0) == (d->dx2 != nullptr), "split output: dx2 and csplit go together");
  ISHAP_REQUIRE(d->sums_ready ? (!local && d->csums) : !d->csums, "sums_ready: the caller's csums, full-map route only");
  ISHAP_REQUIRE(!local || gn_bwd_local_fits(HW, C, gmode), "group does not fit in LDS");
  GnBwdArgs a;
  a.g = (const half_t*)d->g; a.x = (const half_t*)d->x; a.add = (const half_t*)d->add; a.add2 = (const half_t*)d->add2;
  a.dx = (half_t*)d->dx; a.dx2 = (half_t*)d->dx2; a.csplit = d->csplit;
  a.stats = d->stats; a.gamma = d->gamma; a.beta = d->beta; a.emb = d->film ? d->emb : nullptr; a.emb_ld = d->film ? d->emb_ld : 0;
  a.N = N; a.H = H; a.W = W; a.C = C; a.film = d->film; a.act = d->act; a.gmode = gmode;
  if (local) {
    if (launch) ISHAP_TRY(begin());
    TenancyScope tenancy(nullptr, s, !launch, route == 3);
    const bool rec = launch ? tenancy.granted : route == 3;
    const GnBwdLocalArgs la = gn_bwd_local_fill(a, slab, rec ? sc.rec : nullptr);
    const GnLocalPlan p = gn_local_plan(gn_bwd_local_shape(la));
    name = gn_local_kernel_name(p);
    parts = p.parts;
    ISHAP_TRY(report());
    return launch ? gn_bwd_local_launch(la, s) : 0;
  }
  a.sums_ready = d->sums_ready;
  a.csums = d->sums_ready ? d->csums : sc.csums;
  GnLaunchInfo info;
  ISHAP_TRY(gn_backward_launch(a, nullptr, &info));
  name = info.kernel;
  ISHAP_TRY(report());
  if (!launch) return 0;
  ISHAP_TRY(begin());
  return gn_backward_launch(a, s);
}

// y = act(GN(x)) and its input gradient on a chosen route: the plain forms of the call above
int ishap_group_norm32(const void* x_nhwc_f16, const float* gamma, const float* beta, int N, int H, int W, int C, int silu,
                       int route, void* y_nhwc_f16, float* stats, void* scratch, void* stream) {
  ISHAP_REQUIRE(x_nhwc_f16 && gamma && beta && y_nhwc_f16 && stats && scratch, "null argument");
  ishap_group_norm_desc d = {};
  d.N = N; d.H = H; d.W = W; d.C = C; d.route = route; d.act = silu;
  d.gamma = gamma; d.beta = beta; d.scratch = scratch; d.x = x_nhwc_f16; d.out = y_nhwc_f16; d.stats_out = stats;
  return ishap_group_norm32_run(&d, 1, stream, nullptr, nullptr, nullptr, 0);
}

int ishap_group_norm32_backward(const void* g_nhwc_f16, const void* x_nhwc_f16, const float* stats, const float* gamma,
                                const float* beta, int N, int H, int W, int C, int silu, int route, void* dx_nhwc_f16,
                                void* scratch, void* stream) {
  ISHAP_REQUIRE(g_nhwc_f16 && x_nhwc_f16 && stats && gamma && beta && dx_nhwc_f16 && scratch, "null argument");
  ishap_group_norm_desc d = {};
  d.backward = 1; d.N = N; d.H = H; d.W = W; d.C = C; d.route = route; d.act = silu; d.gmode = GB_SAME;
  d.gamma = gamma; d.beta = beta; d.scratch = scratch; d.g = g_nhwc_f16; d.x = x_nhwc_f16; d.stats = stats; d.dx = dx_nhwc_f16;
  return ishap_group_norm32_run(&d, 1, stream, nullptr, nullptr, nullptr, 0);
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
