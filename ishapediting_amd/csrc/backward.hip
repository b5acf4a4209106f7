// UNet input-gradient pass: d(sum(tap * cot)) / dx, hand-derived, layer by layer in reverse.
// Reference: loss.backward() at drag_utils.py:383 (autograd through guided_diffusion/unet.py:634-671 from
// the tapped output block back to x) and :458 (full depth, from the model output).  Only what the path
// needs is computed: gradients w.r.t. activations.  Weight gradients (which the reference computes and
// throws away, its parameters keep requires_grad=True) and the attention checkpoint's second forward
// (unet.py:297) have no counterpart here: activations needed for derivatives are recomputed inside the
// elementwise kernels from the saved GN inputs and statistics.
// Every convolution's input gradient is the same implicit-GEMM kernel run on the gradient map with the
// tap-flipped, transposed weight operand packed at load time (ConvW::wT).
#include "unet.h"

#include "attention.h"
#include "misc.h"
#include "norm.h"

static int gn_bwd_op(Exec& e, GnBwdArgs g) {
  if (!g.sums_ready) ISHAP_SALLOC(g.csums, e, (size_t)g.N * g.C * 2);     // zeroed with the rest of the stats arena at the start of the forward
  ISHAP_REQUIRE(g.csums != nullptr, "stats arena exhausted");
  return e.launch([g](hipStream_t s) { return gn_backward_launch(g, s); });
}

// dY [N,H,W,cout] -> dX [N,H,W,rows of wT] through the transposed / flipped operand
// `gb`: the GroupNorm whose activation this gradient arrives at, at the same resolution (GB_SAME) -- its per-channel
// backward sums are then accumulated in this launch's epilogue (gb->csums allocated here, gb->sums_ready set).
// `may_pend`: the only reader of dx_out is a group-local GroupNorm-backward pass, which adds up split-K slices itself.
static int dgrad_op(Exec& e, const ConvW& c, const Tensor& dy, Flow& dx_out, int n_out, GnBwdArgs* gb = nullptr,
                    bool may_pend = false) {
  dx_out = Flow{shaped(dy, n_out)};
  ISHAP_ALLOC(dx_out.t.p, e, dx_out.t.numel());
  if (gb) {
    ISHAP_SALLOC(gb->csums, e, (size_t)gb->N * gb->C * 2);
    gb->sums_ready = 1;
    ISHAP_REQUIRE(gb->C == n_out && gb->gmode == GB_SAME, "fused GroupNorm-backward sums need the gradient at the GN resolution");
  }
  ConvLaunch k = conv_launch(dy, c, dx_out.t);
  k.Wt = c.wT; k.kpad = c.cout_pad; k.cout = n_out; k.bias = nullptr;      // the transposed operand: dy's channels are its K
  k.gb = gb; k.pend_out = may_pend ? &dx_out.pend : nullptr;
  return conv_op(e, k);
}
// the same for a reader that is no GroupNorm-backward pass (`who`: the skip convolution, proj_out, the stem): a finished tensor
static int dgrad_tensor(Exec& e, const ConvW& c, const Tensor& dy, Tensor& dx_out, int n_out, const char* who) {
  Flow f;
  ISHAP_TRY(dgrad_op(e, c, dy, f, n_out));
  return finished(f, who, dx_out);
}

// group-local input gradient of act(film(GN(x))) on a small map; the upstream gradient `up` (g.g) may still be pending (norm_local.hip)
static int gn_bwd_local_op(Exec& e, const GnBwdArgs& g, Flow& up) {
  const SlabSrc slab = up.take();
  long long* rec = nullptr;
  ISHAP_SALLOC(rec, e, (size_t)g.N * 32 * GN_REC_STRIDE);       // zeroed with the rest of the statistics arena
  const GnBwdLocalArgs a = gn_bwd_local_fill(g, slab, exec_is_solo(e) ? reinterpret_cast<unsigned long long*>(rec) : nullptr);   // see gn_local_op
  return e.launch([a](hipStream_t s) { return gn_bwd_local_launch(a, s); });
}
static bool local_gn_bwd(const GnBwdArgs& g) { return gn_route(g.H * g.W, g.C, g.gmode, true) == GnRoute::local; }

// The input gradient of a convolution `c` that reads act(film(GN(x))), in two parts; `g` describes the GroupNorm (x, stats,
// weights, FiLM row, shape, gmode).  The route is a function of g's shape alone, so both parts (and a dry run) take the same one.
// Dgrad part: dy -> dact, the gradient arriving at the activation.  Group-local route: dact may stay pending (the norm part adds
// the slices up); else, with the gradient at the GroupNorm's own resolution, the launch gathers the backward sums in its epilogue.
static int conv_gn_dgrad(Exec& e, const ConvW& c, const Tensor& dy, GnBwdArgs& g, Flow& dact) {
  const bool loc = local_gn_bwd(g);
  return dgrad_op(e, c, dy, dact, g.C, (!loc && g.gmode == GB_SAME) ? &g : nullptr, loc);
}
// Norm part: dact -> g.dx (allocated by the caller between the two parts, with g.add / add2 / dx2 / csplit as it needs them)
static int conv_gn_norm(Exec& e, GnBwdArgs& g, Flow& dact) {
  g.g = dact.t.p;
  if (local_gn_bwd(g)) return gn_bwd_local_op(e, g, dact);
  ISHAP_REQUIRE(!dact.pending(), "the full-map GroupNorm backward reads a gradient that is still the split-K slices of its dgrad");
  return gn_bwd_op(e, g);
}
// both parts with the plain result between them: dx (its shape set by the caller) is allocated here
static int conv_gn_backward(Exec& e, const ConvW& c, const Tensor& dy, GnBwdArgs g, Tensor& dx) {
  Flow dact;
  ISHAP_TRY(conv_gn_dgrad(e, c, dy, g, dact));
  ISHAP_ALLOC(dx.p, e, dx.numel());
  g.dx = dx.p;
  return conv_gn_norm(e, g, dact);
}

// `split` > 0: the block input was a skip concatenation [h | skip]; its gradient is written as two dense tensors
// (dx = first `split` channels, *dx2 = the rest) so no slicing pass is needed afterwards.
// `add2`: a gradient map of the block input's shape (the skip-connection gradient of an input block) added to the result.
static int res_backward(Exec& e, const ResL& L, const ResSaved& sv, const Tensor& dy, Tensor& dx, int split = 0, Tensor* dx2 = nullptr,
                        const half_t* add2 = nullptr) {
  const KeptForward& k = e.u->kept;
  const Tensor& x = sv.x;
  const Tensor& h1 = sv.h1;
  ISHAP_REQUIRE(dy.C == L.cout && dy.H == h1.H && dy.N == x.N, "ResBlock gradient shape");
  // out_layers: conv2 <- SiLU <- FiLM <- GN2
  Tensor dh1 = shaped(h1);
  GnBwdArgs g2;
  g2.x = h1.p; g2.stats = sv.stats2; g2.gamma = L.n2.gamma; g2.beta = L.n2.beta;
  g2.emb = k.film + L.emb_off; g2.emb_ld = k.film_ld;
  g2.N = h1.N; g2.H = h1.H; g2.W = h1.W; g2.C = L.cout; g2.film = 1; g2.act = 1; g2.gmode = GB_SAME;
  ISHAP_TRY(conv_gn_backward(e, L.c2, dy, g2, dh1));
  // in_layers: conv1 <- (up/down sample) <- SiLU <- GN1
  GnBwdArgs g1;
  g1.x = x.p; g1.stats = sv.stats1; g1.gamma = L.n1.gamma; g1.beta = L.n1.beta;
  g1.N = x.N; g1.H = x.H; g1.W = x.W; g1.C = L.cin; g1.film = 0; g1.act = 1;
  g1.gmode = L.down ? GB_UNPOOL : (L.up ? GB_SUM4 : GB_SAME);
  Flow da;
  ISHAP_TRY(conv_gn_dgrad(e, L.c1, dh1, g1, da));
  const half_t* add = dy.p;     // identity skip: gradient of `x_upd(x)` (unet.py:241,256)
  if (L.has_skip) {
    Tensor dxs;
    ISHAP_TRY(dgrad_tensor(e, L.skip, dy, dxs, L.cin, "the sum with the skip convolution's input gradient"));
    add = dxs.p;
  }
  dx = shaped(x, split);        // split 0: all of x's channels
  ISHAP_ALLOC(dx.p, e, dx.numel());
  if (split > 0) {
    *dx2 = shaped(x, x.C - split);
    ISHAP_ALLOC(dx2->p, e, dx2->numel());
    g1.dx2 = dx2->p; g1.csplit = split;
  }
  g1.add = add; g1.dx = dx.p; g1.add2 = add2;
  return conv_gn_norm(e, g1, da);
}

static int attn_backward(Exec& e, const AttnL& L, const AttnSaved& sv, const Tensor& dy, Tensor& dx) {
  ishap_unet* u = e.u;
  const Tensor& x = sv.x;
  const int N = x.N, T = x.H * x.W, C = L.C, heads = L.heads, d = C / heads;
  const float alpha = 1.f / sqrtf((float)d);
  Tensor dA;
  ISHAP_TRY(dgrad_tensor(e, L.proj, dy, dA, C, "the attention backward"));
  Tensor dqkv{nullptr, N, x.H, x.W, 3 * C};
  ISHAP_ALLOC(dqkv.p, e, dqkv.numel());
  const size_t d_need = (size_t)N * heads * T;
  if (e.dry && d_need > u->attn_D_floats) u->attn_D_floats = d_need;
  AttnArgs ga;
  ga.qkv = sv.qkv.p; ga.out = sv.a.p; ga.dout = dA.p; ga.dqkv = dqkv.p; ga.lse = sv.lse; ga.Dbuf = u->attn_D;
  ga.N = N; ga.T = T; ga.C = C; ga.heads = heads; ga.d = d; ga.alpha = alpha; ga.xcd_map = attn_xcd_setting();
  ISHAP_TRY(e.launch([ga](hipStream_t s) { return attn_backward_launch(ga, s); }));
  dx = shaped(x);
  GnBwdArgs g;
  g.x = x.p; g.stats = sv.stats; g.gamma = L.n.gamma; g.beta = L.n.beta;
  g.N = N; g.H = x.H; g.W = x.W; g.C = C; g.film = 0; g.act = 0; g.gmode = GB_SAME;
  g.add = dy.p;
  return conv_gn_backward(e, L.qkv, dqkv, g, dx);
}

static int block_backward(Exec& e, BlockL& b, Tensor g, Tensor& out, int split = 0, Tensor* out2 = nullptr,
                          const half_t* add2 = nullptr, bool* add2_done = nullptr) {
  ishap_unet* u = e.u;
  for (int i = (int)b.layers.size() - 1; i >= 0; --i) {
    const LayerRef& l = b.layers[i];
    Tensor dx;
    if (l.kind == 0) {
      ISHAP_TRY(dgrad_tensor(e, u->stem, g, dx, u->in_pad, "the input gradient's read-out"));
    } else if (l.kind == 1) {
      if (i == 0 && split > 0) ISHAP_TRY(res_backward(e, u->res[l.idx], u->kept.res[l.idx], g, dx, split, out2, nullptr));
      else if (i == 0 && add2) { ISHAP_TRY(res_backward(e, u->res[l.idx], u->kept.res[l.idx], g, dx, 0, nullptr, add2)); *add2_done = true; }
      else ISHAP_TRY(res_backward(e, u->res[l.idx], u->kept.res[l.idx], g, dx, 0, nullptr, nullptr));
    } else {
      ISHAP_TRY(attn_backward(e, u->attn[l.idx], u->kept.attn[l.idx], g, dx));
    }
    g = dx;
  }
  out = g;
  return 0;
}

// ISHAP_BWD_MARKS=1: a timing event on the backward's stream, tagged (0 start, 100 + i after output block i, 200 after the middle
// block, 300 + i after input block i, 999 end); read back by ishap_unet_marks
static int bwd_mark(ishap_unet* u, hipStream_t s, int tag, bool dry) {
  if (dry || !u->marks_on) return 0;
  if (tag == 0) { u->marks_n = 0; u->mark_tail_set = false; }
  if ((size_t)u->marks_n == u->marks.size()) {
    hipEvent_t ev;
    ISHAP_CHECK_HIP(hipEventCreate(&ev));
    u->marks.push_back(ev);
    u->mark_tags.push_back(0);
  }
  u->mark_tags[u->marks_n] = tag;
  ISHAP_CHECK_HIP(hipEventRecord(u->marks[u->marks_n++], s));
  return 0;
}

int unet_backward_impl(ishap_unet* u, const half_t* cot_tap, const void* cot_out, int cot_out_f16, const float* scale2,
                       float* dx, hipStream_t s, bool dry) {
  Exec e{u, s, dry};
  TenancyScope tenancy(u, s, dry);
  e.tenant = tenancy.granted;
  KeptForward& k = u->kept;
  u->arena.off = k.fwd_mark;
  u->stat_off = k.stat_fwd_mark;
  u->seq++;                     // the scratch above fwd_mark is reused from here on: the previous pass's gradient maps are gone
  if (!dry) {
    ISHAP_REQUIRE(k.have_saved, "backward needs a preceding forward with keep_for_backward=1");
    if (k.bwd_since_fwd++ > 0 && u->stat_cap > k.stat_fwd_mark)   // a second backward on the same forward: fresh zeros
      ISHAP_CHECK_HIP(hipMemsetAsync(u->stat_base + k.stat_fwd_mark, 0, (u->stat_cap - k.stat_fwd_mark) * sizeof(long long), s));
  }
  ISHAP_TRY(bwd_mark(u, s, 0, dry));
  const ishap_unet_config& cfg = u->cfg;
  const int N = k.N;            // dry runs follow a dry forward of the same batch size
  const int n_in = (int)u->in_blocks.size(), n_out = (int)u->out_blocks.size();
  int F;
  Tensor g;
  if (cot_out) {
    ISHAP_REQUIRE(dry || !k.restored_partial, "the restored snapshot holds the network up to the tap only: no full-depth backward on it");
    if (!dry) ISHAP_TRY(unet_join_tail(u, s));    // full depth: needs the blocks an overlapped forward put on the side stream
    // head backward: out = conv3x3(silu(gn(h)))  (unet.py:612-616,667-669)
    F = n_out - 1;
    const int S = cfg.image_size, opad = u->head.cout_pad;
    Tensor dout{nullptr, N, S, S, opad};
    ISHAP_ALLOC(dout.p, e, dout.numel());
    ISHAP_TRY(e.launch([=](hipStream_t s) { return nchw_to_nhwc_f16_scaled(cot_out, cot_out_f16 ? 0 : 1, dout.p, N, u->cfg.out_channels, S * S, opad, 1.f, s); }));
    GnBwdArgs a;
    a.x = k.h_final.p; a.stats = k.head_stats; a.gamma = u->head_norm.gamma;
    a.beta = u->head_norm.beta; a.N = N; a.H = S; a.W = S; a.C = u->final_ch; a.act = 1;
    g = Tensor{nullptr, N, S, S, u->final_ch};      // k.h_final's shape (dry runs follow a dry forward of the same batch size)
    ISHAP_TRY(conv_gn_backward(e, u->head, dout, a, g));
  } else {
    F = dry ? n_out - 1 : k.feat;
    ISHAP_REQUIRE(F >= 0, "the last forward had no tap (feat_layer < 0)");
    g = shaped(k.out[u->out_blocks[F].slot]);
    g.p = const_cast<half_t*>(cot_tap);
  }
  std::vector<Tensor> skipgrad(n_in);
  for (int i = F; i >= 0; --i) {
    BlockL& b = u->out_blocks[i];
    const int Cs = b.skip_ch, Ch = b.cin - Cs;
    ISHAP_REQUIRE(b.layers[0].kind == 1 && Ch % 8 == 0, "an output block starts with a ResBlock on the concatenation");
    b.gout = g;
    ISHAP_TRY(block_backward(e, b, g, b.gh, Ch, &b.gs));   // the first ResBlock writes d/d[h | skip] as two tensors
    skipgrad[n_in - 1 - i] = b.gs;   // hs.pop() order (unet.py:663)
    g = b.gh;
    ISHAP_TRY(bwd_mark(u, s, 100 + i, dry));
    // a deferred forward tail starts behind this point: the backward's first (chip-filling) blocks have the GPU to themselves.
    // Default: once the first output block on a map of at most 16 x 16 pixels has been differentiated (the real model: after
    // out8 ... out5, i.e. four blocks -- in-situ sweep of the count, profiles/round5_overlap_tail_ab.txt 7); ISHAP_TAIL_MID=k: after
    // k blocks, 0: never (the tail then starts at the fork)
    static const int mid_k = ishap_switch("ISHAP_TAIL_MID", -1);
    const bool here = mid_k > 0 ? F - i + 1 == mid_k : (mid_k < 0 && b.res_in <= 16);
    if (!dry && u->tail_deferred && !u->mid_recorded && here) {
      ISHAP_CHECK_HIP(hipEventRecord(u->ev_mid, s));
      u->mid_recorded = true;
    }
  }
  // The gradient entering input block i is (gradient from the block after it) + (its skip-connection gradient).  When the
  // block after it ends its backward with a ResBlock (always, except the stem), that ResBlock's last kernel adds the skip
  // gradient itself; `pending` is the addend still owed when that was not possible.
  auto run = [&](BlockL& blk, const half_t* owed_next, const half_t*& pending) -> int {
    bool done = false;
    blk.gout = g;
    ISHAP_TRY(block_backward(e, blk, g, g, 0, nullptr, owed_next, &done));
    pending = (owed_next && !done) ? owed_next : nullptr;
    return 0;
  };
  const half_t* pending = nullptr;
  ISHAP_TRY(run(u->mid, n_in > 0 ? skipgrad[n_in - 1].p : nullptr, pending));
  ISHAP_TRY(bwd_mark(u, s, 200, dry));
  for (int i = n_in - 1; i >= 0; --i) {
    // build_spec / unet_build accept the resblock_updown variant only: the middle block and every input block but the stem begin
    // with a ResBlock, which takes the owed addend as add2 (tests/test_unet_ref_host.py walks the specs)
    ISHAP_REQUIRE(!pending, "a skip gradient is still owed: the block before this one did not begin with a ResBlock");
    ISHAP_TRY(run(u->in_blocks[i], i > 0 ? skipgrad[i - 1].p : nullptr, pending));
    ISHAP_TRY(bwd_mark(u, s, 300 + i, dry));
  }
  ISHAP_TRY(e.launch([=](hipStream_t s) {
    return nhwc_f16_to_nchw_f32_scaled(g.p, dx, N, u->cfg.in_channels, u->cfg.image_size * u->cfg.image_size, u->in_pad,
                                       scale2 ? scale2 + 1 : nullptr, s);
  }));
  ISHAP_TRY(bwd_mark(u, s, 999, dry));
  if (!dry) { u->grad_seq = u->seq; u->grad_F = F; }
  return 0;
}

// elapsed milliseconds from the start mark of the last backward to each of its marks, and to the begin / end of the forward tail
// that ran beside it on the side stream (-1: no deferred tail ran).  Synchronises with the device.
extern "C" int ishap_unet_marks(ishap_unet* u, int* tags, float* ms, int cap, float* tail_begin_ms, float* tail_end_ms) {
  ISHAP_REQUIRE(u && tags && ms && cap > 0, "null argument");
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  if (tail_begin_ms) *tail_begin_ms = -1.f;
  if (tail_end_ms) *tail_end_ms = -1.f;
  if (u->marks_n == 0) return 0;
  ISHAP_CHECK_HIP(hipDeviceSynchronize());
  const int n = u->marks_n < cap ? u->marks_n : cap;
  for (int k = 0; k < n; ++k) {
    tags[k] = u->mark_tags[k];
    ISHAP_CHECK_HIP(hipEventElapsedTime(&ms[k], u->marks[0], u->marks[k]));
  }
  if (u->mark_tail_set) {
    if (tail_begin_ms) ISHAP_CHECK_HIP(hipEventElapsedTime(tail_begin_ms, u->marks[0], u->mark_tail_begin));
    if (tail_end_ms) ISHAP_CHECK_HIP(hipEventElapsedTime(tail_end_ms, u->marks[0], u->mark_tail_end));
  }
  return n;
}

extern "C" int ishap_unet_backward_input(ishap_unet* u, const void* cot, const float* scale2, float* dx, void* stream) {
  ISHAP_REQUIRE(u && cot && dx, "null argument");
  ISHAP_TRY(ishap_check_status());
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  return unet_backward_impl(u, (const half_t*)cot, nullptr, 0, scale2, dx, (hipStream_t)stream, false);
}
extern "C" int ishap_unet_backward_from_output(ishap_unet* u, const void* cot_out, int cot_is_f16, const float* scale2,
                                               float* dx, void* stream) {
  ISHAP_REQUIRE(u && cot_out && dx, "null argument");
  ISHAP_TRY(ishap_check_status());
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  return unet_backward_impl(u, nullptr, cot_out, cot_is_f16, scale2, dx, (hipStream_t)stream, false);
}
