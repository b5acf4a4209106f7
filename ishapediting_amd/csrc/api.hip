// C-ABI wrappers for the step / drag / decode kernels (declarations and reference citations: include/ishap.h).
#include "../../include/ishap.h"
#include "common.h"
#include "ddpm.h"
#include "decode.h"
#include "constrain.h"
#include "drag.h"
#include "track.h"
#include "retarget.h"
#include "regions.h"
#include "render.h"

static thread_local std::string g_err;
void ishap_set_error(const std::string& msg) { g_err = msg; }

#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
static std::atomic<unsigned*> g_status{nullptr};
static std::mutex g_status_mu;
unsigned* ishap_status_word() {
  unsigned* p = g_status.load(std::memory_order_acquire);
  if (p) return p;
  std::lock_guard<std::mutex> lk(g_status_mu);
  p = g_status.load(std::memory_order_relaxed);
  if (p) return p;
  void* h = nullptr;
  if (hipHostMalloc(&h, 64, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess) return nullptr;
  *(volatile unsigned*)h = 0u;
  g_status.store((unsigned*)h, std::memory_order_release);
  return (unsigned*)h;
}
static const char* status_text(unsigned code) {
  switch (code) {
    case ISHAP_DEV_GN_RENDEZVOUS:
      return "device-side failure: a group-local GroupNorm rendezvous timed out (its workgroups were not co-resident); the "
             "affected launch wrote NaN -- results since then are invalid";
    case ISHAP_DEV_CHAIN_TIMEOUT:
      return "device-side failure: a small-map chain kernel gave up waiting for another workgroup; the affected launch "
             "wrote NaN -- results since then are invalid";
    default: return "device-side failure: unknown status code";
  }
}
int ishap_check_status() {
  unsigned* p = g_status.load(std::memory_order_acquire);
  if (!p) return 0;
  const unsigned code = *(volatile unsigned*)p;
  if (code == 0u) return 0;
  *(volatile unsigned*)p = 0u;
  ishap_set_error(std::string(status_text(code)) + " (code " + std::to_string(code) + ")");
  return -3;
}
int ishap_cu_count() {
  static std::atomic<int> cached[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int v = cached[dev].load(std::memory_order_relaxed);
  if (v > 0) return v;
  int n = 0;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  cached[dev].store(n, std::memory_order_relaxed);
  return n;
}

namespace {
struct Tenant {
  std::mutex mu;
  const void* owner = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t done = nullptr;      // recorded when the tenant's last sequence was enqueued completely
  bool have = false, open = false, recorded = false;
  bool denied = false;            // another context / stream asked while this tenant held the device (read and cleared by the tenant)
};
Tenant g_tenant[64];
}  // namespace

// ---- the runtime switches: every environment variable the library reads (the Python package reads three more of its own:
//      ISHAP_FUSED_UPDATE, ISHAP_OVERLAP_TAIL, ISHAP_STEP_RNG) ----
static const struct { const char* name; int dflt; const char* meaning; } kSwitches[] = {
    {"ISHAP_IGEMM4", 2, "3x3 convolutions on igemm4: 0 = never, 1 = its 128x128 tiles only, 2 = every shape it takes"},
    {"ISHAP_IG4_TEAMS", 2, "igemm4 forms: 2 = two-team and 128x64 tiles, 1 = 128x64 tiles only, 0 = neither"},
    {"ISHAP_IG4_HALO", 1, "0 = no igemm4 halo tiles"},
    {"ISHAP_HALVES", 2, "2 = igemm2's two-team form"},
    {"ISHAP_SKINNY", 1, "0 = the tiled kernel + reduce instead of the skinny kernel"},
    {"ISHAP_G1_SLICES", 1, "0 = no sliced 1x1 GEMMs on the 8x8 maps"},
    {"ISHAP_BIG_MIN", 192, "128x128 workgroups from which the 128-tile is taken"},
    {"ISHAP_IG4_NOUTER", 2, "igemm4 tile order within an XCD: 0 = n-tiles fastest, 1 = m-tiles fastest, 2 = by estimated L2 traffic"},
    {"ISHAP_GN_PARTS", 8, "most workgroups per (image, group) of the group-local GroupNorm kernels"},
    {"ISHAP_GN_SPIN_LIMIT", 0, "polls before a rendezvous (group-local GroupNorm, fused 8x8 attention) gives up; <= 0 = the built-in limit"},
    {"ISHAP_GN_XCD", 1, "group-local GroupNorm: 0 = no XCD-local dealing, 1 = dealing + local record copy, 2 = also pre-touch the copy"},
    {"ISHAP_TAIL_MID", -1, "backward blocks before a deferred forward tail starts: k > 0 = after k, 0 = at the fork, < 0 = first map <= 16x16"},
    {"ISHAP_LOCAL_GN", 1, "0 = the two-pass GroupNorm route on the small maps too"},
    {"ISHAP_TAIL_DEFER_WGS", 128, "most tiles per launch of the overlapped forward tail's 3x3 convolutions"},
    {"ISHAP_BWD_MARKS", 0, "non-zero = a context records the backward pass's per-block events (read when the context is created)"},
    {"ISHAP_ATTN_XCD", 1, "0 = no XCD-local placement of an attention head's workgroups (any non-zero value = 1)"},
    {"ISHAP_ATTN8", 1, "0 = no fused attention kernel on the 8x8 maps"},
    {"ISHAP_EVENT_FENCE", 0, "non-zero = the library's ordering events keep the default system-scope fence"},
};
int ishap_switch(const char* name, int fallback) {
  for (const auto& s : kSwitches)
    if (!strcmp(s.name, name) && s.dflt == fallback) {
      const char* e = getenv(name);
      return e ? atoi(e) : fallback;
    }
  fprintf(stderr, "ishap_switch: %s (default %d) is not a row of kSwitches\n", name, fallback);
  abort();
}

unsigned ishap_event_flags() {
  static const unsigned f = ishap_switch("ISHAP_EVENT_FENCE", 0) ? (unsigned)hipEventDisableTiming
                                                                 : (unsigned)(hipEventDisableTiming | hipEventDisableSystemFence);
  return f;
}

bool ishap_rendezvous_begin(const void* owner, hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  Tenant& t = g_tenant[dev];
  std::lock_guard<std::mutex> lk(t.mu);
  if (t.have && t.owner == owner && t.stream == s) {
    if (t.open) return false;                   // re-entered from another thread on the same (owner, stream): do not share
    t.open = true;                              // same in-order stream: the earlier sequence precedes this one on the device
    return true;
  }
  if (t.have) {
    if (t.open) { t.denied = true; return false; }                   // another sequence is being enqueued right now
    if (t.recorded && hipEventQuery(t.done) != hipSuccess) { t.denied = true; return false; }   // ... or is still running
  }
  if (!t.done && hipEventCreateWithFlags(&t.done, ishap_event_flags()) != hipSuccess) { t.done = nullptr; return false; }
  t.owner = owner; t.stream = s; t.have = true; t.open = true; t.recorded = false; t.denied = false;
  return true;
}

// true once after another context / stream was refused the tenancy while `owner` held it: the device is being shared, and work
// that only pays when ONE sequence has the chip to itself (the overlapped forward tail) should not be started
bool ishap_rendezvous_contended(const void* owner, hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return true;
  Tenant& t = g_tenant[dev];
  std::lock_guard<std::mutex> lk(t.mu);
  if (!t.have || t.owner != owner || t.stream != s) return true;
  const bool d = t.denied;
  t.denied = false;
  return d;
}

void ishap_rendezvous_end(const void* owner, hipStream_t s, bool granted) {
  if (!granted) return;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return;
  Tenant& t = g_tenant[dev];
  std::lock_guard<std::mutex> lk(t.mu);
  if (!t.have || t.owner != owner || t.stream != s) return;
  t.recorded = hipEventRecord(t.done, s) == hipSuccess;
  t.open = false;
  if (!t.recorded) t.have = false;
}

extern "C" int ishap_rendezvous_would_grant(const void* owner, void* stream) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  Tenant& t = g_tenant[dev];
  std::lock_guard<std::mutex> lk(t.mu);
  if (!t.have) return 1;
  if (t.owner == owner && t.stream == (hipStream_t)stream) return t.open ? 0 : 1;
  if (t.open) return 0;
  return (!t.recorded || hipEventQuery(t.done) == hipSuccess) ? 1 : 0;
}

extern "C" {

const char* ishap_last_error(void) { return g_err.c_str(); }

int ishap_device_status(void) { return ishap_check_status(); }

int ishap_ddpm_step(const float* x, const float* model_out, const float* noise, const float* variance_in,
                    const ishap_step_coefs* k, int N, int C, int HW, float* sample, float* pred_xstart,
                    float* variance, float* mean, void* stream) {
  ISHAP_REQUIRE(x && model_out && k, "null argument");
  ISHAP_REQUIRE(k->mode >= 0 && k->mode <= 3, "mode");
  ISHAP_REQUIRE(k->mode != 2 || noise, "mode 2 needs variance_noise in `noise`");
  DdpmStepArgs a;
  a.x = x; a.model_out = model_out; a.noise = noise; a.variance_in = variance_in;
  a.sample = sample; a.pred_xstart = pred_xstart; a.variance = variance; a.mean = mean;
  a.N = N; a.C = C; a.HW = HW;
  a.min_log = k->min_log; a.max_log = k->max_log; a.sqrt_recip = k->sqrt_recip; a.sqrt_recipm1 = k->sqrt_recipm1;
  a.coef1 = k->coef1; a.coef2 = k->coef2; a.nonzero = k->nonzero; a.clip = k->clip_denoised; a.mode = k->mode;
  a.ddim_a = k->ddim_a; a.ddim_b = k->ddim_b; a.ddim_sigma = k->ddim_sigma;
  a.rng = k->rng; a.rng_seed = k->rng_seed; a.rng_offset = k->rng_offset; a.noise_out = k->noise_out;
  return ddpm_step_launch(a, (hipStream_t)stream);
}

int ishap_ddpm_step_guided(const float* x, const float* model_out, const float* noise, const float* variance_in,
                           const ishap_step_coefs* k, int N, int C, int HW, const float* grad, float scale,
                           const float* grad_mul_dev, float* guided, float* sample, float* variance, void* stream) {
  ISHAP_REQUIRE(x && model_out && k && grad && guided, "null argument");
  ISHAP_REQUIRE(k->mode == 0, "the guided step is p_sample_guidance's sqrt(variance) form (mode 0)");
  DdpmStepArgs a;
  a.x = x; a.model_out = model_out; a.noise = noise; a.variance_in = variance_in;
  a.sample = sample; a.variance = variance;
  a.N = N; a.C = C; a.HW = HW;
  a.min_log = k->min_log; a.max_log = k->max_log; a.sqrt_recip = k->sqrt_recip; a.sqrt_recipm1 = k->sqrt_recipm1;
  a.coef1 = k->coef1; a.coef2 = k->coef2; a.nonzero = k->nonzero; a.clip = k->clip_denoised; a.mode = k->mode;
  a.guide_grad = grad; a.guide_scale = scale; a.guide_mul = grad_mul_dev; a.guided = guided;
  a.rng = k->rng; a.rng_seed = k->rng_seed; a.rng_offset = k->rng_offset; a.noise_out = k->noise_out;
  return ddpm_step_launch(a, (hipStream_t)stream);
}

int ishap_ddpm_step_guided_scales(const float* x, const float* model_out, const float* noise, const float* variance_in,
                                  const ishap_step_coefs* k, int N, int C, int HW, const float* grad, const float* scales,
                                  const float* grad_mul_dev, float* guided, float* sample, float* variance, void* stream) {
  ISHAP_REQUIRE(x && model_out && k && grad && scales && guided, "null argument");
  ISHAP_REQUIRE(k->mode == 0, "the guided step is p_sample_guidance's sqrt(variance) form (mode 0)");
  DdpmStepArgs a;
  a.x = x; a.model_out = model_out; a.noise = noise; a.variance_in = variance_in;
  a.sample = sample; a.variance = variance;
  a.N = N; a.C = C; a.HW = HW;
  a.min_log = k->min_log; a.max_log = k->max_log; a.sqrt_recip = k->sqrt_recip; a.sqrt_recipm1 = k->sqrt_recipm1;
  a.coef1 = k->coef1; a.coef2 = k->coef2; a.nonzero = k->nonzero; a.clip = k->clip_denoised; a.mode = k->mode;
  a.guide_grad = grad; a.guide_scales = scales; a.guide_mul = grad_mul_dev; a.guided = guided;
  a.rng = k->rng; a.rng_seed = k->rng_seed; a.rng_offset = k->rng_offset; a.noise_out = k->noise_out;
  return ddpm_step_launch(a, (hipStream_t)stream);
}

int ishap_guided_update(const float* sample, const float* variance, const float* grad, float scale,
                        const float* grad_mul_dev, long long numel, float* out, void* stream) {
  ISHAP_REQUIRE(sample && variance && grad && out, "null argument");
  return guided_update_launch(sample, variance, grad, out, scale, grad_mul_dev, numel, (hipStream_t)stream);
}

int ishap_axpby(const float* x, const float* y, float a, float b, long long numel, float* out, void* stream) {
  ISHAP_REQUIRE(x && y && out, "null argument");
  return axpby_launch(x, y, out, a, b, numel, (hipStream_t)stream);
}

// ---- drag loss: one set of launches (csrc/drag.hip) that takes E edits (one edit is E = 1); the shape requirements are checked
// there.  One scratch buffer, carved as [grad_fx E*W*W*ld int64][acc E*2 int64][nmask E int32][touched E*3*W*W][chan_weight 3*ld],
// every part starting on a 256-byte boundary
struct DragBatchScratch { long long *gfx, *acc; int* nmask; unsigned char *touched, *chw; long long bytes; };
static DragBatchScratch drag_batch_carve(void* base, int E, int W, int ld) {
  Carve c{(char*)base};
  return {c.take<long long>((long long)E * W * W * ld), c.take<long long>(2ll * E), c.take<int>(E),
          c.take<unsigned char>(3ll * E * W * W), c.take<unsigned char>(3ll * ld), c.total()};
}

long long ishap_drag_batch_scratch_bytes(int E, int W, int ld) {
  if (E < 1 || W < 2 || ld < 1) return -1;
  return drag_batch_carve(nullptr, E, W, ld).bytes;
}

static int fill_drag_batch(const ishap_drag_batch_args* a, DragBatchArgs& d) {
  ISHAP_REQUIRE(a && a->chmap && a->sources && a->targets && a->handle_offsets && a->cof && a->scratch, "null argument");
  ISHAP_REQUIRE(a->E >= 1 && a->E <= DRAG_MAX_EDITS, "drag batch: E must be in 1..32");      // hoff / cof below hold that many
  ISHAP_REQUIRE(a->W > 1 && a->r >= 0 && a->Cc >= 1 && a->ld >= 1 && a->orig_stride >= 0, "drag dims");
  ISHAP_REQUIRE(!a->weights || a->weights_stride >= 0, "drag batch: negative weights_stride");
  const DragBatchScratch S = drag_batch_carve(a->scratch, a->E, a->W, a->ld);
  ISHAP_REQUIRE(a->scratch_bytes >= S.bytes, "drag batch: scratch smaller than ishap_drag_batch_scratch_bytes(E, W, ld)");
  ISHAP_REQUIRE(((unsigned long long)a->scratch & 15ull) == 0, "drag batch: scratch must be 16-byte aligned");
  DragArgs& b = d.base;
  b.W = a->W; b.ld = a->ld; b.Cc = a->Cc; b.chmap = a->chmap; b.sources = a->sources; b.targets = a->targets;
  b.r = a->r; b.voxel = a->voxel; b.l1 = a->l1;
  b.gfx = S.gfx; b.acc = S.acc; b.nmask = S.nmask; b.touched = S.touched; b.chw = S.chw;
  d.E = a->E;
  d.orig_stride = a->orig_stride;
  for (int e = 0; e <= a->E; ++e) d.hoff[e] = a->handle_offsets[e];
  for (int e = 0; e < a->E; ++e) d.cof[e] = a->cof[e];
  return 0;
}

// the per-call pointers of a loss call (nullptr for a setup call, which reads none of them)
static void fill_drag_call(DragBatchArgs& d, const void* edit, const void* orig, float* grad, float* loss) {
  d.base.edit = (const half_t*)edit; d.base.orig = (const half_t*)orig; d.base.grad = grad; d.base.loss = loss;
}

int ishap_drag_batch_setup(const ishap_drag_batch_args* a, void* stream) {
  DragBatchArgs d;
  ISHAP_TRY(fill_drag_batch(a, d));
  return drag_batch_setup_launch(d, (hipStream_t)stream);
}

int ishap_drag_batch_loss_grad(const ishap_drag_batch_args* a, const void* edit, const void* orig, float* grad, float* loss,
                               void* stream) {
  DragBatchArgs d;
  ISHAP_TRY(fill_drag_batch(a, d));
  ISHAP_REQUIRE(edit && orig && grad && loss, "null argument");
  fill_drag_call(d, edit, orig, grad, loss);
  return drag_batch_loss_launch(d, nullptr, nullptr, nullptr, a->weights, a->weights_stride, (hipStream_t)stream);
}

int ishap_drag_batch_loss_cotangent(const ishap_drag_batch_args* a, const void* edit, const void* orig, float* grad,
                                    float* loss, void* cot_f16, unsigned* bits, float* scale2, void* stream) {
  DragBatchArgs d;
  ISHAP_TRY(fill_drag_batch(a, d));
  ISHAP_REQUIRE(edit && orig && grad && loss && cot_f16 && bits && scale2, "null argument");
  fill_drag_call(d, edit, orig, grad, loss);
  return drag_batch_loss_launch(d, (half_t*)cot_f16, bits, scale2, a->weights, a->weights_stride, (hipStream_t)stream);
}

// ---- handle tracking (csrc/track.hip): every range is checked before anything is launched
long long ishap_drag_track_scratch_bytes(int E, int Btot, int R, int rp, int Cc) {
  if (E < 1 || E > DRAG_MAX_EDITS || Btot < E) return -1;
  return track_scratch_bytes(Btot, R, rp, Cc);
}

int ishap_drag_track(const void* edit, const void* orig, long long orig_stride, int W, int ld, int Cc, const int* chmap,
                     const float* sources, const int* handle_offsets, int E, float voxel, int R, int rp, const int* K_in, int* K_out,
                     float* dist, float* dist0, float* volume, void* scratch, long long scratch_bytes, void* stream) {
  ISHAP_REQUIRE(edit && orig && chmap && sources && handle_offsets && K_in && K_out && dist && dist0 && scratch, "null argument");
  ISHAP_REQUIRE(E >= 1 && E <= DRAG_MAX_EDITS, "drag track: E must be in 1..32");      // hoff below holds that many
  TrackArgs t;
  t.edit = (const half_t*)edit; t.orig = (const half_t*)orig; t.orig_stride = orig_stride;
  t.W = W; t.ld = ld; t.Cc = Cc; t.chmap = chmap; t.sources = sources; t.E = E;
  for (int e = 0; e <= E; ++e) t.hoff[e] = handle_offsets[e];
  t.voxel = voxel; t.R = R; t.rp = rp; t.K_in = K_in; t.K_out = K_out; t.dist = dist; t.dist0 = dist0; t.volume = volume;
  t.partial = (float*)scratch;
  const long long need = ishap_drag_track_scratch_bytes(E, t.hoff[E], R, rp, Cc);
  ISHAP_REQUIRE(need >= 0, "drag track: R must be in 0..8, rp in 0..4, Cc >= 1 and every edit needs a handle");
  ISHAP_REQUIRE(scratch_bytes >= need, "drag track: scratch smaller than ishap_drag_track_scratch_bytes(E, Btot, R, rp, Cc)");
  ISHAP_REQUIRE(((unsigned long long)scratch & 15ull) == 0, "drag track: scratch must be 16-byte aligned");
  return track_launch(t, (hipStream_t)stream);
}

// ---- closed-loop drag (csrc/retarget.hip): the arguments a drag call does not already check are checked here and in
// drag_retarget_launch, before anything is launched.  `a->targets` is the goals buffer the call writes.
static int retarget_call(const ishap_drag_batch_args* a, const float* final_targets, const int* K, const float* steps,
                         const float* arrives, float step, float arrive, float* remaining, int* arrived, int* done, void* stream) {
  ISHAP_REQUIRE(a && final_targets && K && remaining && arrived && done, "null argument");
  ISHAP_REQUIRE(a->W > 1 && 3ll * a->W * a->W <= RETARGET_LDS_BYTES, "drag retarget: 3*W*W must not exceed 65536 (the LDS bitmaps)");
  DragBatchArgs d;
  ISHAP_TRY(fill_drag_batch(a, d));
  RetargetArgs q;
  q.final_targets = final_targets; q.K = K; q.goals = const_cast<float*>(d.base.targets);
  q.remaining = remaining; q.arrived = arrived; q.done = done;
  for (int e = 0; e < d.E; ++e) { q.step[e] = steps ? steps[e] : step; q.arrive[e] = arrives ? arrives[e] : arrive; }
  return drag_retarget_launch(d, q, (hipStream_t)stream);
}

int ishap_drag_batch_retarget(const ishap_drag_batch_args* a, const float* final_targets, const int* K, float step, float arrive,
                              float* remaining, int* arrived, int* done, void* stream) {
  return retarget_call(a, final_targets, K, nullptr, nullptr, step, arrive, remaining, arrived, done, stream);
}

int ishap_drag_batch_retarget_each(const ishap_drag_batch_args* a, const float* final_targets, const int* K, const float* steps,
                                   const float* arrives, float* remaining, int* arrived, int* done, void* stream) {
  ISHAP_REQUIRE(steps && arrives, "null argument");
  return retarget_call(a, final_targets, K, steps, arrives, 0.f, 0.f, remaining, arrived, done, stream);
}

// ---- region weights of the drag loss's mask term (csrc/regions.hip)
long long ishap_region_plane_weights_scratch_bytes(int W) { return W > 4096 ? -1 : region_scratch_bytes(W); }

int ishap_region_plane_weights(const ishap_region_prim* prims, int n_prims, const unsigned char* keep_voxels,
                               const unsigned char* free_voxels, int D, int W, int dilate, float keep_weight, float free_weight,
                               float* weights_out, int* shadow_counts, void* scratch, long long scratch_bytes, void* stream) {
  static_assert(sizeof(ishap_region_prim) == sizeof(RegionPrim) && sizeof(RegionPrim) == 56, "ishap_region_prim layout");
  ISHAP_REQUIRE(W >= 2 && W <= 4096, "region weights: W must be in 2..4096");
  ISHAP_REQUIRE(n_prims >= 0 && (prims || n_prims == 0), "region weights: null primitives");
  if (keep_voxels || free_voxels) ISHAP_REQUIRE(D >= W && D <= REGION_MAX_D, "region weights: a voxel grid needs W <= D <= 4096");
  ISHAP_REQUIRE(dilate >= 0, "region weights: negative dilate");
  ISHAP_REQUIRE(std::isfinite(keep_weight) && std::isfinite(free_weight) && keep_weight >= 0.f && free_weight >= 0.f,
                "region weights: keep_weight and free_weight must be finite and >= 0");
  ISHAP_REQUIRE(weights_out && scratch, "null argument");
  ISHAP_REQUIRE(scratch_bytes >= region_scratch_bytes(W), "region weights: scratch smaller than ishap_region_plane_weights_scratch_bytes(W)");
  ISHAP_REQUIRE(((unsigned long long)scratch & 15ull) == 0, "region weights: scratch must be 16-byte aligned");
  return region_plane_weights_launch((const RegionPrim*)prims, n_prims, keep_voxels, free_voxels, D, W, dilate, keep_weight, free_weight,
                                     weights_out, shadow_counts, scratch, (hipStream_t)stream);
}

// the checks the three region map calls share
static int region_args_check(const ishap_region_prim* prims, int n_prims, const unsigned char* keep_voxels, const unsigned char* free_voxels,
                             int D, int W, int dilate, const void* out, const void* scratch) {
  ISHAP_REQUIRE(W >= 2 && W <= 4096, "region weights: W must be in 2..4096");
  ISHAP_REQUIRE(n_prims >= 0 && (prims || n_prims == 0), "region weights: null primitives");
  if (keep_voxels || free_voxels) ISHAP_REQUIRE(D >= W && D <= REGION_MAX_D, "region weights: a voxel grid needs W <= D <= 4096");
  ISHAP_REQUIRE(dilate >= 0, "region weights: negative dilate");
  ISHAP_REQUIRE(out && scratch, "null argument");
  ISHAP_REQUIRE(((unsigned long long)scratch & 15ull) == 0, "region weights: scratch must be 16-byte aligned");
  return 0;
}

int ishap_region_plane_marks(const ishap_region_prim* prims, int n_prims, const unsigned char* keep_voxels,
                             const unsigned char* free_voxels, int D, int W, int dilate, unsigned char* marks_out, int* shadow_counts,
                             void* scratch, long long scratch_bytes, void* stream) {
  ISHAP_TRY(region_args_check(prims, n_prims, keep_voxels, free_voxels, D, W, dilate, marks_out, scratch));
  ISHAP_REQUIRE(scratch_bytes >= region_scratch_bytes(W), "region marks: scratch smaller than ishap_region_plane_weights_scratch_bytes(W)");
  ISHAP_REQUIRE((void*)marks_out != scratch, "region marks: marks_out must not be the scratch");
  return region_plane_marks_launch((const RegionPrim*)prims, n_prims, keep_voxels, free_voxels, D, W, dilate, marks_out, shadow_counts,
                                   scratch, (hipStream_t)stream);
}

long long ishap_region_plane_feather_scratch_bytes(int W) { return region_feather_scratch_bytes(W); }

int ishap_region_plane_feather(const ishap_region_prim* prims, int n_prims, const unsigned char* keep_voxels,
                               const unsigned char* free_voxels, int D, int W, int dilate, float keep_weight, float free_weight,
                               const double* table, int table_len, float* weights_out, int* shadow_counts, void* scratch,
                               long long scratch_bytes, void* stream) {
  ISHAP_TRY(region_args_check(prims, n_prims, keep_voxels, free_voxels, D, W, dilate, weights_out, scratch));
  ISHAP_REQUIRE(W <= 1024, "region feather: W must be in 2..1024");
  ISHAP_REQUIRE(std::isfinite(keep_weight) && std::isfinite(free_weight) && keep_weight >= 0.f && free_weight >= 0.f,
                "region weights: keep_weight and free_weight must be finite and >= 0");
  ISHAP_REQUIRE(table && table_len >= 1 && table_len <= 4096, "region feather: the table holds 1..4096 entries (falloff <= 64 texels)");
  ISHAP_REQUIRE(scratch_bytes >= region_feather_scratch_bytes(W), "region feather: scratch smaller than ishap_region_plane_feather_scratch_bytes(W)");
  return region_plane_feather_launch((const RegionPrim*)prims, n_prims, keep_voxels, free_voxels, D, W, dilate, keep_weight, free_weight,
                                     table, table_len, weights_out, shadow_counts, scratch, (hipStream_t)stream);
}

int ishap_grad_to_scaled_f16(const float* grad, void* out_f16, unsigned* bits, float* scale2, long long numel,
                             void* stream) {
  ISHAP_REQUIRE(grad && out_f16 && bits && scale2, "null argument");
  return grad_to_scaled_f16_launch(grad, (half_t*)out_f16, bits, scale2, numel, (hipStream_t)stream);
}

int ishap_planes_prepare(const float* latent, const float* range, const float* middle, int S, float* planes,
                         void* stream) {
  ISHAP_REQUIRE(latent && planes, "null argument");
  return planes_prepare_launch(latent, range, middle, planes, S, (hipStream_t)stream);
}

static int fill_dec(const ishap_decoder_weights* w, DecodeArgs& d) {
  ISHAP_REQUIRE(w && w->B && w->W1 && w->b1 && w->W2 && w->b2 && w->w3 && w->b3, "null decoder weights");
  d.B = w->B; d.W1 = w->W1; d.b1 = w->b1; d.W2 = w->W2; d.b2 = w->b2; d.w3 = w->w3; d.b3 = w->b3;
  return 0;
}

int ishap_triplane_decode_points(const float* planes, int S, const ishap_decoder_weights* w, const float* coords,
                                 long long npts, float* logits, void* stream) {
  DecodeArgs d;
  ISHAP_TRY(fill_dec(w, d));
  ISHAP_REQUIRE(planes && coords && logits, "null argument");
  d.planes = planes; d.S = S; d.coords = coords; d.npts = npts; d.out = logits;
  return triplane_decode_launch(d, (hipStream_t)stream);
}

int ishap_triplane_points_loss_grad(const float* planes, int S, const ishap_decoder_weights* w, const float* W1T,
                                    const float* W2T, const float* coords, const float* gt, long long npts,
                                    float* dplanes, float* loss, float* logits, void* stream) {
  DecodeArgs d;
  ISHAP_TRY(fill_dec(w, d));
  ISHAP_REQUIRE(planes && W1T && W2T && coords && gt && dplanes && loss, "null argument");
  DecBwdArgs b;
  b.planes = planes; b.S = S; b.B = d.B; b.W1 = d.W1; b.b1 = d.b1; b.W2 = d.W2; b.b2 = d.b2; b.w3 = d.w3; b.b3 = d.b3;
  b.W1T = W1T; b.W2T = W2T; b.coords = coords; b.gt = gt; b.npts = npts; b.dplanes = dplanes; b.loss = loss; b.logits = logits;
  return decode_points_bwd_launch(b, (hipStream_t)stream);
}

long long ishap_constraint_setup_scratch_bytes(long long M, int S) { return constraint_setup_scratch_bytes(M, S); }

int ishap_constraint_setup(const float* coords, long long M, int S, int* row_start, int* entry, float* entry_w, void* scratch,
                           long long scratch_bytes, void* stream) {
  ConstraintSetupArgs a;
  a.coords = coords; a.M = M; a.S = S; a.row_start = row_start; a.entry = entry; a.entry_w = entry_w; a.scratch = scratch;
  a.scratch_bytes = scratch_bytes;
  return constraint_setup_launch(a, (hipStream_t)stream);
}

int ishap_constraint_loss_grad(const float* planes, int S, const ishap_decoder_weights* w, const float* coords,
                               const float* targets, const float* weights, long long M, double wsum, const int* row_start,
                               const int* entry, const float* entry_w, float* dfeat, float* partials, float* dplanes,
                               float* loss, float* logits, void* stream) {
  DecodeArgs d;
  ISHAP_TRY(fill_dec(w, d));
  ConstraintArgs c;
  c.B = d.B; c.W1 = d.W1; c.b1 = d.b1; c.W2 = d.W2; c.b2 = d.b2; c.w3 = d.w3; c.b3 = d.b3;
  c.planes = planes; c.S = S; c.coords = coords; c.gt = targets; c.pw = weights; c.npts = M; c.wsum = (float)wsum;
  c.row_start = row_start; c.entry = entry; c.entry_w = entry_w; c.dfeat = dfeat; c.partials = partials; c.dplanes = dplanes;
  c.loss = loss; c.logits = logits;
  return constraint_loss_grad_launch(c, (hipStream_t)stream);
}

int ishap_triplane_fit_loss_grad(const float* planes, int S, const ishap_decoder_weights* w, const float* coords,
                                 const float* gt, const int* idx, long long nbatch, const float* rand_coords,
                                 const float* rand_noise, long long nrand, float pair_w, float* dplanes, float* loss_parts,
                                 void* stream) {
  DecodeArgs d;
  ISHAP_TRY(fill_dec(w, d));
  ISHAP_REQUIRE(planes && dplanes && loss_parts, "null argument");
  ISHAP_REQUIRE(nbatch == 0 || (coords && gt && idx), "null batch");
  ISHAP_REQUIRE(nrand == 0 || (rand_coords && rand_noise), "null random pairs");
  FitArgs f;
  f.planes = planes; f.S = S; f.B = d.B; f.W1 = d.W1; f.b1 = d.b1; f.W2 = d.W2; f.b2 = d.b2; f.w3 = d.w3; f.b3 = d.b3;
  f.coords = coords; f.gt = gt; f.idx = idx; f.nbatch = nbatch; f.rcoords = rand_coords; f.rnoise = rand_noise;
  f.nrand = nrand; f.pair_w = pair_w; f.dplanes = dplanes; f.loss_parts = loss_parts;
  return triplane_fit_loss_grad_launch(f, (hipStream_t)stream);
}

static void fill_field(const DecodeArgs& d, FieldArgs& f) {
  f.B = d.B; f.W1 = d.W1; f.b1 = d.b1; f.W2 = d.W2; f.b2 = d.b2; f.w3 = d.w3; f.b3 = d.b3;
}

int ishap_triplane_field_grad(const float* planes, int S, const ishap_decoder_weights* w, const float* coords,
                              long long npts, float* logits, float* grad, void* stream) {
  DecodeArgs d;
  ISHAP_TRY(fill_dec(w, d));
  FieldArgs f;
  fill_field(d, f);
  f.planes = planes; f.S = S; f.coords = coords; f.npts = npts; f.logits = logits; f.grad = grad;
  return triplane_field_grad_launch(f, (hipStream_t)stream);
}

int ishap_triplane_project(const float* planes, int S, const ishap_decoder_weights* w, const float* coords, long long npts,
                           int iterations, float step_max, float max_move, float tol, float gmin, float* x_out,
                           float* z_out, float* normal_out, int* accepted_out, void* stream) {
  DecodeArgs d;
  ISHAP_TRY(fill_dec(w, d));
  FieldArgs f;
  fill_field(d, f);
  f.planes = planes; f.S = S; f.coords = coords; f.npts = npts; f.logits = z_out; f.iterations = iterations;
  f.step_max = step_max; f.max_move = max_move; f.tol = tol; f.gmin = gmin; f.x_out = x_out; f.normal_out = normal_out;
  f.accepted_out = accepted_out;
  return triplane_project_launch(f, (hipStream_t)stream);
}

int ishap_triplane_reg_adam_step(const float* planes, float* planes_out, float* m, float* v, float* dplanes, int S, int* step,
                                 double lr, double beta1, double beta2, double eps, float l2_w, float tv_w, double* ws,
                                 float* reg_parts, void* stream) {
  static_assert(ISHAP_TRIPLANE_REG_WS == 3 * TRIPLANE_REG_BLOCKS * 3, "workspace size");
  ISHAP_REQUIRE(planes_out && m && v && dplanes && step, "null argument");
  RegAdamArgs r;
  r.planes = planes; r.S = S; r.ws = ws; r.reg_parts = reg_parts; r.planes_out = planes_out; r.m = m; r.v = v;
  r.dplanes = dplanes; r.step = step; r.lr = lr; r.beta1 = beta1; r.beta2 = beta2; r.eps = eps; r.l2_w = l2_w; r.tv_w = tv_w;
  return triplane_reg_adam_launch(r, (hipStream_t)stream);
}

int ishap_triplane_reg_values(const float* planes, int S, double* ws, float* reg_parts, void* stream) {
  ISHAP_REQUIRE(reg_parts, "null argument");
  RegAdamArgs r;
  r.planes = planes; r.S = S; r.ws = ws; r.reg_parts = reg_parts;
  return triplane_reg_adam_launch(r, (hipStream_t)stream);
}

int ishap_x0_grad_to_cotangent(const float* dplanes, const float* range, const float* x, const float* model_out,
                               float sqrt_recip, float sqrt_recipm1, int clip_denoised, int S, float* g_direct,
                               float* cot_out, void* stream) {
  ISHAP_REQUIRE(dplanes && x && model_out && g_direct && cot_out, "null argument");
  return x0_grad_launch(dplanes, range, x, model_out, sqrt_recip, sqrt_recipm1, clip_denoised, S, g_direct, cot_out,
                        (hipStream_t)stream);
}

int ishap_triplane_decode_grid(const float* planes, int S, const ishap_decoder_weights* w, const float* axis, int res,
                               float* volume, void* stream) {
  DecodeArgs d;
  ISHAP_TRY(fill_dec(w, d));
  ISHAP_REQUIRE(planes && axis && volume && res > 0, "null argument");
  d.planes = planes; d.S = S; d.lin = axis; d.res = res; d.npts = (long long)res * res * res; d.out = volume;
  return triplane_decode_launch(d, (hipStream_t)stream);
}

int ishap_triplane_decode_bricks(const float* planes, int S, const ishap_decoder_weights* w, const float* axis, int res,
                                 const int* bricks, long long nbricks, float* values, void* stream) {
  DecodeArgs d;
  ISHAP_TRY(fill_dec(w, d));
  ISHAP_REQUIRE(planes && axis && bricks && values, "null argument");
  ISHAP_REQUIRE(nbricks >= 1 && nbricks <= (1ll << 21), "decode bricks: 1 <= bricks <= 2^21");
  d.planes = planes; d.S = S; d.lin = axis; d.res = res; d.npts = 729 * nbricks; d.out = values;
  return triplane_decode_bricks_launch(d, bricks, nbricks, (hipStream_t)stream);
}

// ---- headless rendering (csrc/render.hip) ----
long long ishap_render_scratch_bytes(long long nverts, long long ntris, int width, int height) {
  return render_scratch_bytes(nverts, ntris, width, height);
}

int ishap_render_mesh(const float* verts, long long nverts, const int* tris, long long ntris, const float* normals,
                      const int* tri_part, const float* parts, int nparts, const ishap_camera* camera, int width, int height,
                      void* scratch, long long scratch_bytes, unsigned char* rgb, float* depth, int* tri_id, void* stream) {
  ISHAP_REQUIRE(camera, "render_mesh: null camera");
  RenderArgs a;
  ISHAP_TRY(render_camera(camera->eye, camera->centre, camera->up, camera->fov_y_deg, camera->near, camera->far, width, height, a.cam));
  const long long need = render_scratch_bytes(nverts, ntris, width, height);
  ISHAP_REQUIRE(need > 0, "render_mesh: 0 <= nverts, ntris < 2^31");
  ISHAP_REQUIRE(scratch && scratch_bytes >= need, "render_mesh: scratch smaller than ishap_render_scratch_bytes(nverts, ntris, width, height)");
  ISHAP_REQUIRE(((uintptr_t)scratch & 15) == 0, "render_mesh: scratch must be 16-byte aligned");
  ISHAP_REQUIRE(ntris == 0 || nverts == 0 || (verts && tris), "render_mesh: null verts / tris");
  ISHAP_REQUIRE(!rgb || (parts && nparts > 0), "render_mesh: rgb needs at least one part");
  a.verts = verts; a.tris = tris; a.normals = normals; a.tri_part = tri_part; a.parts = parts;
  a.nverts = nverts; a.ntris = ntris; a.nparts = nparts; a.width = width; a.height = height;
  a.scratch = scratch; a.rgb = rgb; a.depth = depth; a.tri_id = tri_id;
  return render_mesh_launch(a, (hipStream_t)stream);
}

int ishap_unproject(const ishap_camera* camera, int width, int height, const float* xyd, long long n, float* world, void* stream) {
  ISHAP_REQUIRE(camera && n >= 0 && (n == 0 || (xyd && world)), "unproject arguments");
  RenderCam cam;
  ISHAP_TRY(render_camera(camera->eye, camera->centre, camera->up, camera->fov_y_deg, camera->near, camera->far, width, height, cam));
  if (n == 0) return 0;
  return render_unproject_launch(cam, xyd, n, world, (hipStream_t)stream);
}

}  // extern "C"
