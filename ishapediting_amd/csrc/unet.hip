// UNet graph construction, parameter loading and the forward executor.
// Reference structure: guided_diffusion/unet.py:427-616 (constructor), :634-671 (forward),
// :236-256 (ResBlock), :299-305 + :337-354 (AttentionBlock, legacy qkv order).
// One C call runs the whole network: ~500 kernel launches on the caller's stream, no host sync.
#include "unet.h"

#include <cstring>

#include "attention.h"
#include "decode.h"
#include "misc.h"
#include "norm.h"

static int round_up(int a, int b) { return (a + b - 1) / b * b; }

// ------------------------------------------------------------------------------------------------
// graph
// ------------------------------------------------------------------------------------------------
static void init_conv(ConvW& c, const std::string& path, int cin, int cout, int taps) {
  c.path = path; c.cin = cin; c.cout = cout; c.taps = taps;
  c.kpad = round_up(cin, 32);
  c.cout_pad = round_up(cout, 32);
}

int unet_build(ishap_unet* u) {
  const ishap_unet_config& cfg = u->cfg;
  const int mc = cfg.model_channels;
  u->ted = mc * 4;
  // stem input channels padded with zeros: to 64-wide K-steps when that is cheap (96 -> 128: the LDS-DMA kernel), else to 32
  u->in_pad = cfg.in_channels >= 64 ? round_up(cfg.in_channels, 64) : round_up(cfg.in_channels, 32);
  auto has_att = [&](int ds) {
    for (int i = 0; i < cfg.n_att; ++i) if (cfg.attention_ds[i] == ds) return true;
    return false;
  };
  auto heads_of = [&](int ch) { return ch / cfg.num_head_channels; };
  // count layers first so the vectors never reallocate (ParamSlot keeps pointers into them)
  u->res.reserve(256);
  u->attn.reserve(64);
  int film = 0;
  auto add_res = [&](const std::string& path, int cin, int cout, bool up, bool down) {
    ResL r;
    r.path = path; r.cin = cin; r.cout = cout; r.up = up; r.down = down;
    r.n1.C = cin; r.n2.C = cout;
    init_conv(r.c1, path + ".in_layers.2", cin, cout, 9);
    init_conv(r.c2, path + ".out_layers.3", cout, cout, 9);
    r.has_skip = cin != cout;
    if (r.has_skip) init_conv(r.skip, path + ".skip_connection", cin, cout, 1);
    r.emb_off = film;
    film += 2 * cout;
    u->res.push_back(r);
    return (int)u->res.size() - 1;
  };
  auto add_attn = [&](const std::string& path, int ch) {
    AttnL a;
    a.path = path; a.C = ch; a.heads = heads_of(ch);
    a.n.C = ch;
    init_conv(a.qkv, path + ".qkv", ch, 3 * ch, 1);
    init_conv(a.proj, path + ".proj_out", ch, ch, 1);
    u->attn.push_back(a);
    return (int)u->attn.size() - 1;
  };

  int ch = cfg.channel_mult[0] * mc;
  int res = cfg.image_size;
  init_conv(u->stem, "input_blocks.0.0", cfg.in_channels, ch, 9);
  u->stem.kpad = u->in_pad;
  {
    BlockL b;
    b.name = "input_blocks.0";
    b.layers.push_back({0, 0});
    b.cin = cfg.in_channels; b.cout = ch; b.res_in = b.res_out = res;
    u->in_blocks.push_back(b);
  }
  std::vector<int> chans{ch};
  int ds = 1;
  for (int level = 0; level < cfg.n_mult; ++level) {
    for (int k = 0; k < cfg.num_res_blocks; ++k) {
      BlockL b;
      b.name = "input_blocks." + std::to_string(u->in_blocks.size());
      int cout = cfg.channel_mult[level] * mc;
      b.layers.push_back({1, add_res(b.name + ".0", ch, cout, false, false)});
      b.cin = ch; ch = cout; b.cout = ch; b.res_in = b.res_out = res;
      if (has_att(ds)) b.layers.push_back({2, add_attn(b.name + ".1", ch)});
      u->in_blocks.push_back(b);
      chans.push_back(ch);
    }
    if (level != cfg.n_mult - 1) {
      BlockL b;
      b.name = "input_blocks." + std::to_string(u->in_blocks.size());
      b.layers.push_back({1, add_res(b.name + ".0", ch, ch, false, true)});
      b.cin = b.cout = ch; b.res_in = res; b.res_out = res / 2;
      u->in_blocks.push_back(b);
      chans.push_back(ch);
      ds *= 2;
      res /= 2;
    }
  }
  u->mid.name = "middle_block";
  u->mid.layers.push_back({1, add_res("middle_block.0", ch, ch, false, false)});
  u->mid.layers.push_back({2, add_attn("middle_block.1", ch)});
  u->mid.layers.push_back({1, add_res("middle_block.2", ch, ch, false, false)});
  u->mid.cin = u->mid.cout = ch; u->mid.res_in = u->mid.res_out = res;
  for (int level = cfg.n_mult - 1; level >= 0; --level) {
    for (int i = 0; i < cfg.num_res_blocks + 1; ++i) {
      int ich = chans.back();
      chans.pop_back();
      BlockL b;
      b.name = "output_blocks." + std::to_string(u->out_blocks.size());
      int cout = mc * cfg.channel_mult[level];
      b.layers.push_back({1, add_res(b.name + ".0", ch + ich, cout, false, false)});
      b.cin = ch + ich; b.skip_ch = ich; ch = cout; b.cout = ch; b.res_in = res;
      if (has_att(ds)) b.layers.push_back({2, add_attn(b.name + "." + std::to_string(b.layers.size()), ch)});
      if (level && i == cfg.num_res_blocks) {
        b.layers.push_back({1, add_res(b.name + "." + std::to_string(b.layers.size()), ch, ch, true, false)});
        ds /= 2;
        res *= 2;
      }
      b.res_out = res;
      u->out_blocks.push_back(b);
    }
  }
  int slot = 0;
  for (auto& b : u->in_blocks) b.slot = slot++;
  u->mid.slot = slot++;
  for (auto& b : u->out_blocks) b.slot = slot++;
  u->kept.out.resize(slot); u->kept.cat.resize(slot);
  u->kept.res.resize(u->res.size()); u->kept.attn.resize(u->attn.size());
  u->final_ch = ch;
  u->film_rows = film;
  u->head_norm.C = ch;
  init_conv(u->head, "out.2", ch, cfg.out_channels, 9);
  u->head.split = true;
  u->head.kpad = 3 * ch;

  // ---- parameter table (torch state_dict names, gd/unet.py module tree) ----
  auto reg = [&](const std::string& name, std::initializer_list<long long> shape, int kind, ConvW* conv, float** dst,
                 long long off) {
    ParamSlot p;
    p.name = name; p.ndim = (int)shape.size();
    int i = 0;
    for (long long v : shape) p.shape[i++] = v;
    p.kind = kind; p.conv = conv; p.dst_off = off;
    p.dst = dst ? *dst : nullptr;
    u->param_index[name] = (int)u->params.size();
    u->params.push_back(p);
  };
  // device buffers for plain fp32 parameters
  auto dalloc = [&](float** p, size_t n) -> int {
    ISHAP_CHECK_HIP(hipMalloc((void**)p, n * sizeof(float)));
    ISHAP_CHECK_HIP(hipMemset(*p, 0, n * sizeof(float)));
    return 0;
  };
  auto conv_alloc = [&](ConvW& c) -> int {
    size_t wn = (size_t)round_up(c.cout, 128) * c.taps * c.kpad;
    ISHAP_CHECK_HIP(hipMalloc((void**)&c.w, wn * sizeof(half_t)));
    ISHAP_CHECK_HIP(hipMemset(c.w, 0, wn * sizeof(half_t)));
    size_t tn = (size_t)round_up(round_up(c.cin, 32), 128) * c.taps * c.cout_pad;
    ISHAP_CHECK_HIP(hipMalloc((void**)&c.wT, tn * sizeof(half_t)));
    ISHAP_CHECK_HIP(hipMemset(c.wT, 0, tn * sizeof(half_t)));
    ISHAP_TRY(dalloc(&c.bias, round_up(c.cout, 4)));
    return 0;
  };
  // conv2d: a 1x1 Conv2d weight [O,I,1,1] (the skip connections); the attention blocks' 1x1 convs are Conv1d [O,I,1]
  auto reg_conv = [&](ConvW& c, bool conv2d = false) -> int {
    ISHAP_TRY(conv_alloc(c));
    if (c.taps == 9) reg(c.path + ".weight", {c.cout, c.cin, 3, 3}, 0, &c, nullptr, 0);
    else if (conv2d) reg(c.path + ".weight", {c.cout, c.cin, 1, 1}, 0, &c, nullptr, 0);
    else reg(c.path + ".weight", {c.cout, c.cin, 1}, 0, &c, nullptr, 0);
    reg(c.path + ".bias", {c.cout}, 1, &c, nullptr, 0);
    return 0;
  };
  auto reg_norm = [&](NormW& n, const std::string& path) -> int {
    ISHAP_TRY(dalloc(&n.gamma, n.C));
    ISHAP_TRY(dalloc(&n.beta, n.C));
    reg(path + ".weight", {n.C}, 2, nullptr, &n.gamma, 0);
    reg(path + ".bias", {n.C}, 2, nullptr, &n.beta, 0);
    return 0;
  };
  const int ted = u->ted;
  ISHAP_TRY(dalloc(&u->te_w0, (size_t)ted * mc));
  ISHAP_TRY(dalloc(&u->te_b0, ted));
  ISHAP_TRY(dalloc(&u->te_w2, (size_t)ted * ted));
  ISHAP_TRY(dalloc(&u->te_b2, ted));
  ISHAP_TRY(dalloc(&u->emb_w, (size_t)film * ted));
  ISHAP_TRY(dalloc(&u->emb_b, film));
  reg("time_embed.0.weight", {ted, mc}, 2, nullptr, &u->te_w0, 0);
  reg("time_embed.0.bias", {ted}, 2, nullptr, &u->te_b0, 0);
  reg("time_embed.2.weight", {ted, ted}, 2, nullptr, &u->te_w2, 0);
  reg("time_embed.2.bias", {ted}, 2, nullptr, &u->te_b2, 0);
  ISHAP_TRY(reg_conv(u->stem));
  for (auto& r : u->res) {
    ISHAP_TRY(reg_norm(r.n1, r.path + ".in_layers.0"));
    ISHAP_TRY(reg_conv(r.c1));
    reg(r.path + ".emb_layers.1.weight", {2 * r.cout, ted}, 2, nullptr, &u->emb_w, (long long)r.emb_off * ted);
    reg(r.path + ".emb_layers.1.bias", {2 * r.cout}, 2, nullptr, &u->emb_b, r.emb_off);
    ISHAP_TRY(reg_norm(r.n2, r.path + ".out_layers.0"));
    ISHAP_TRY(reg_conv(r.c2));
    if (r.has_skip) {
      ISHAP_TRY(reg_conv(r.skip, true));
      if (!r.down && !r.up && r.c2.kpad % 64 == 0 && r.skip.kpad % 64 == 0) {
        // forward operand [c2 (9 taps) | skip (1x1)] concatenated along K: both convolutions in one launch
        const int ld = 9 * r.c2.kpad + r.skip.kpad;
        const size_t n = (size_t)round_up(r.cout, 128) * ld;
        ISHAP_CHECK_HIP(hipMalloc((void**)&r.c2.cat, n * sizeof(half_t)));
        ISHAP_CHECK_HIP(hipMemset(r.c2.cat, 0, n * sizeof(half_t)));
        r.c2.cat_ld = ld; r.c2.cat_off = 0;
        r.skip.cat = r.c2.cat; r.skip.cat_ld = ld; r.skip.cat_off = 9 * r.c2.kpad;
      }
    }
  }
  for (auto& a : u->attn) {
    ISHAP_TRY(reg_norm(a.n, a.path + ".norm"));
    ISHAP_TRY(reg_conv(a.qkv));
    ISHAP_TRY(reg_conv(a.proj));
  }
  ISHAP_TRY(reg_norm(u->head_norm, "out.0"));
  ISHAP_TRY(reg_conv(u->head));

  const int NB = cfg.max_batch;
  ISHAP_TRY(dalloc(&u->d_temb, (size_t)NB * mc));
  ISHAP_TRY(dalloc(&u->d_e1, (size_t)NB * ted));
  ISHAP_TRY(dalloc(&u->d_emb, (size_t)NB * ted));
  ISHAP_TRY(dalloc(&u->d_film, (size_t)NB * film));
  return 0;
}

// ------------------------------------------------------------------------------------------------
// parameter loading
// ------------------------------------------------------------------------------------------------
static int load_param(ishap_unet* u, ParamSlot& p, const float* data, hipStream_t s) {
  const long long n = p.numel();
  if (p.kind == 0) {
    ConvW& c = *p.conv;
    if (c.split) {
      ISHAP_TRY(pack_conv_weight_split(data, c.w, c.cout, c.cin, c.taps, round_up(c.cout, 128), s));
    } else {
      ISHAP_TRY(pack_conv_weight(data, c.w, c.cout, c.cin, c.taps, round_up(c.cout, 128), c.kpad, 0, s));
      if (c.cat) ISHAP_TRY(pack_conv_weight(data, c.cat, c.cout, c.cin, c.taps, round_up(c.cout, 128), c.kpad, 0, s, c.cat_ld, c.cat_off));
    }
    ISHAP_TRY(pack_conv_weight(data, c.wT, c.cout, c.cin, c.taps, round_up(round_up(c.cin, 32), 128), c.cout_pad, 1, s));
  } else if (p.kind == 1) {
    ConvW& c = *p.conv;
    if (c.split) ISHAP_CHECK_HIP(hipMemcpyAsync(c.bias, data, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    else ISHAP_TRY(round_through_f16(data, c.bias, n, s));   // torso conv bias is half in the reference (fp16_util.py:19-21)
  } else {
    ISHAP_CHECK_HIP(hipMemcpyAsync(p.dst + p.dst_off, data, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// op helpers
// ------------------------------------------------------------------------------------------------
long long* salloc(Exec& e, size_t count) {
  ishap_unet* u = e.u;
  size_t o = (u->stat_off + 63) / 64 * 64;
  u->stat_off = o + count;
  if (u->stat_off > u->stat_high) u->stat_high = u->stat_off;
  if (e.dry) return (long long*)(uintptr_t)(0x1000 + o * 8);
  return u->stat_off <= u->stat_cap ? u->stat_base + o : nullptr;
}

// In-launch rendezvous (several workgroups per GroupNorm group) is allowed on a sequence that holds the device's tenancy and is
// not the overlapped forward tail itself.  A tail still running on the side stream does not forbid it (round 4; it used to):
// the tail never launches rendezvous grids (exec_is_solo is false for it), and kernels that wait for nobody cannot starve a
// grid that does -- they finish and free their compute units (the same argument as for tenants, common.h).
bool exec_is_solo(const Exec& e) {
  return e.dry || (e.tenant && (e.u->side == nullptr || e.s != e.u->side));
}

static bool local_gn(int HW, int C) { return gn_route(HW, C, GB_SAME, false) == GnRoute::local; }

ConvLaunch conv_launch(const Tensor& x, const ConvW& w, const Tensor& y) {
  ConvLaunch c;
  c.X = x.p; c.N = y.N; c.H = y.H; c.W = y.W; c.ldx = x.C;
  c.Wt = w.w; c.kpad = w.kpad; c.taps = w.taps; c.cout = w.cout; c.bias = w.bias;
  c.out = y.p; c.ldo = y.C; c.stat_out = y.sums;
  return c;
}

int conv_op(Exec& e, const ConvLaunch& c) {
  if (c.pend_out) *c.pend_out = SlabSrc{};
  IgemmArgs a;
  ISHAP_TRY(igemm_fill(c, e.chunk_tiles, a));
  a.flops_scale = (c.Wt == e.u->head.w) ? 1.f / 3.f : 1.f;    // profiling weight of the hi/lo-split head; the executor's own, not part of the shared fill
  const size_t need = a.ksplit > 1 ? (size_t)a.ksplit * a.M * a.N : 0;
  if (a.defer_reduce) {
    // the consumer adds the slices up itself: they live in the arena until it has run
    ISHAP_ALLOC(a.ws, e, need);
    SlabSrc& p = *c.pend_out;
    p.ws = a.ws; p.nslab = a.ksplit; p.zstride = (long long)a.M * a.N;
    p.bias = c.bias; p.bias2 = c.bias2; p.res = c.res; p.ldr = c.ldr; p.res_ups = c.res_ups;
  } else {
    if (e.dry && need > e.u->ws_floats) e.u->ws_floats = need;
    ISHAP_REQUIRE(need <= e.u->ws_floats, "split-K workspace too small");
    a.ws = e.ws ? e.ws : e.u->ws;
  }
  return e.launch([a](hipStream_t s) { return igemm_launch(a, s); });
}

int finished(const Flow& f, const char* who, Tensor& out) {
  ISHAP_REQUIRE(!f.pending(), std::string(who) + " reads a tensor that is still the split-K slices of its producer");
  ISHAP_REQUIRE(f.cat.a == nullptr, std::string(who) + " reads a skip concatenation that nobody has written yet");
  out = f.t;
  return 0;
}

// A pending flow whose next consumer cannot add the slices up itself: the stand-alone reduce (bias, residual, fp16).
int slab_materialize(Exec& e, Flow& f) {
  if (!f.pending()) return 0;
  ISHAP_REQUIRE(f.cat.a == nullptr, "only the group-local GroupNorm pass adds up the pending half of a lazy concatenation");
  const IgemmArgs a = igemm_reduce_fill(f.take(), (int)f.t.rows(), f.t.C, f.t.H, f.t.W, f.t.p, f.t.C);
  return e.launch([a](hipStream_t s) { return igemm_reduce_launch(a, s); });
}

int gn_stats_op(Exec& e, const Tensor& x, float* stats) {
  size_t need = gn_partial_floats(x.N, x.H * x.W, x.C);
  if (e.dry && need > e.u->gn_partial_floats) e.u->gn_partial_floats = need;
  ISHAP_REQUIRE(need <= e.u->gn_partial_floats, "GroupNorm statistics scratch too small");
  float* part = e.gn_partial ? e.gn_partial : e.u->gn_partial;
  return e.launch([=](hipStream_t s) { return gn_stats_launch(x.p, part, stats, x.N, x.H * x.W, x.C, s); });
}

// The GroupNorm pass `g` on a small map: one group-local launch that also adds up `x` when it is still pending (and its first
// half when x is a lazy skip concatenation), see norm_local.hip
static int gn_local_op(Exec& e, Flow& x, const GnApplyArgs& g) {
  const SlabSrc slab = x.take();
  long long* rec = nullptr;
  ISHAP_SALLOC(rec, e, (size_t)x.t.N * 32 * GN_REC_STRIDE);     // zeroed with the statistics arena at the start of the forward
  // several workgroups per group rendezvous inside the launch: only while this launch sequence is the context's only one
  // (beside an overlapped forward tail two half-resident rendezvous grids could wait on each other's compute units)
  const GnLocalArgs a = gn_local_fill(g, slab, exec_is_solo(e) ? reinterpret_cast<unsigned long long*>(rec) : nullptr);
  return e.launch([a](hipStream_t s) { return gn_local_launch(a, s); });
}

// out = act(film(GN(x))) (+ 2x2 pool with the pooled raw input in xpool | the head's hi/lo split); `stats` receives (mean, rstd)
// for the backward pass; emb: the FiLM row (null without film).  THE forward consumer of a Flow: f may be pending or a lazy skip
// concatenation and is finished once this pass has run.  Route: a small map takes ONE group-local launch; else pending slices are
// added up by the stand-alone reduce, the statistics pass runs unless the producer(s) gathered the sums, and the apply kernel
// finalises those sums into `stats` itself.  The split form has no group-local kernel (the head's map is full-size anyway).
static int gn_forward_op(Exec& e, Flow& f, const NormW& nw, half_t* out, half_t* xpool, float* stats, const float* emb,
                         int film, int act, int pool, int split = 0) {
  const Tensor& x = f.t;
  const LazyCat cat = f.cat;
  const bool lazy_cat = cat.a != nullptr;
  GnApplyArgs g;
  g.x = x.p; g.out = out; g.xpool = xpool; g.stats_out = stats;
  g.gamma = nw.gamma; g.beta = nw.beta; g.emb = emb; g.emb_ld = emb ? e.u->kept.film_ld : 0;
  g.N = x.N; g.H = x.H; g.W = x.W; g.C = x.C; g.film = film; g.act = act; g.pool = pool; g.split = split;
  if (lazy_cat) { g.x = cat.a; g.x2 = cat.b; g.csplit = cat.ca; g.xcopy = x.p; }
  const bool local = !split && local_gn(x.H * x.W, x.C);
  ISHAP_REQUIRE(local || !lazy_cat || (cat.sa && cat.sb), "a lazy concatenation on a large map carries the producers' sums");
  ISHAP_TRY(local ? gn_local_op(e, f, g) : slab_materialize(e, f));
  f.cat = LazyCat{};           // either route writes the concatenation into x.p as it goes
  if (local) return 0;
  const bool summed = x.sums || lazy_cat;
  if (!summed) ISHAP_TRY(gn_stats_op(e, x, stats));
  g.stats = stats; g.sums = x.sums;
  if (lazy_cat) { g.sums = cat.sa; g.sums2 = cat.sb; }
  if (!summed) g.stats_out = nullptr;
  return e.launch([g](hipStream_t s) { return gn_apply_launch(g, s); });
}

static int res_forward(Exec& e, const ResL& L, ResSaved& sv, Flow x, Flow& y) {
  ishap_unet* u = e.u;
  const int N = x.t.N, H = x.t.H, W = x.t.W;
  const int Ho = L.down ? H / 2 : (L.up ? H * 2 : H), Wo = L.down ? W / 2 : (L.up ? W * 2 : W);
  ISHAP_REQUIRE(x.t.C == L.cin, "ResBlock input channels");
  float* st1 = nullptr; ISHAP_ALLOC(st1, e, (size_t)N * 64);
  float* st2 = nullptr; ISHAP_ALLOC(st2, e, (size_t)N * 64);
  ISHAP_REQUIRE(x.cat.a == nullptr || (!L.down && !L.up), "a skip concatenation feeds a plain ResBlock");
  const bool loc_out = local_gn(Ho * Wo, L.cout);     // conv1 may then leave its split-K slices to the second GroupNorm
  const bool nosum_out = small_map(Ho * Wo);      // the consumers of an activation on a small map gather their own statistics
  Tensor a{nullptr, N, L.down ? Ho : H, L.down ? Wo : W, L.cin};
  ISHAP_ALLOC(a.p, e, a.numel());
  Tensor xs = filled_by_next_gn(x);      // the skip path reads x after the pass below -- or the pooled x that pass writes
  if (L.down) { xs = a; ISHAP_ALLOC(xs.p, e, a.numel()); }
  ISHAP_TRY(gn_forward_op(e, x, L.n1, a.p, L.down ? xs.p : nullptr, st1, nullptr, 0, 1, L.down));
  Flow h1{Tensor{nullptr, N, Ho, Wo, L.cout}};
  ISHAP_ALLOC(h1.t.p, e, h1.t.numel());
  if (!nosum_out) ISHAP_SALLOC(h1.t.sums, e, (size_t)N * L.cout * 2);
  Tensor c = shaped(h1.t);
  ISHAP_ALLOC(c.p, e, c.numel());
  ConvLaunch k1 = conv_launch(a, L.c1, h1.t);
  k1.ups = L.up; k1.pend_out = loc_out ? &h1.pend : nullptr;
  ISHAP_TRY(conv_op(e, k1));
  ISHAP_TRY(gn_forward_op(e, h1, L.n2, c.p, nullptr, st2, u->kept.film + L.emb_off, 1, 1, 0));
  y = Flow{shaped(h1.t)};
  ISHAP_ALLOC(y.t.p, e, y.t.numel());
  if (!nosum_out) ISHAP_SALLOC(y.t.sums, e, (size_t)N * L.cout * 2);
  // the block output's next reader is always a GroupNorm pass (the next ResBlock's, an attention block's, the head's):
  // on a small map it may stay pending
  SlabSrc* ypend = small_map(Ho * Wo) ? &y.pend : nullptr;
  ConvLaunch k2 = conv_launch(c, L.c2, y.t);
  if (L.has_skip && L.c2.cat) {
    // y = conv2(c) + skip(x) as ONE launch: the 1x1 skip convolution is L.cin more K columns read from x
    k2.Wt = L.c2.cat; k2.ldw = L.c2.cat_ld; k2.X2 = xs.p; k2.ldx2 = L.cin; k2.K2 = L.skip.kpad; k2.bias2 = L.skip.bias;
    k2.pend_out = ypend;
  } else if (L.has_skip) {
    ConvLaunch ks = conv_launch(xs, L.skip, y.t);
    ks.stat_out = nullptr;              // y is complete, and its sums gathered, only after conv2 below
    ISHAP_TRY(conv_op(e, ks));
    k2.res = y.t.p; k2.ldr = L.cout;
  } else {
    k2.res = xs.p; k2.ldr = L.cin; k2.res_ups = L.up; k2.pend_out = ypend;
  }
  ISHAP_TRY(conv_op(e, k2));
  sv.stats1 = st1; sv.stats2 = st2;
  ISHAP_TRY(finished(x, "the record of a ResBlock's input", sv.x));
  return finished(h1, "the record of a ResBlock's conv1 output", sv.h1);
}

static int attn_forward(Exec& e, const AttnL& L, AttnSaved& sv, Flow in, Flow& y) {
  const int N = in.t.N, T = in.t.H * in.t.W, C = L.C, heads = L.heads, d = C / heads;
  ISHAP_REQUIRE(in.t.C == C, "attention channels");
  ISHAP_REQUIRE(d % 32 == 0, "head width must be a multiple of 32");
  float* st = nullptr; ISHAP_ALLOC(st, e, (size_t)N * 64);
  float* lse = nullptr; ISHAP_ALLOC(lse, e, (size_t)N * heads * T);
  Tensor nrm = shaped(in.t);
  ISHAP_ALLOC(nrm.p, e, nrm.numel());
  ISHAP_TRY(gn_forward_op(e, in, L.n, nrm.p, nullptr, st, nullptr, 0, 0, 0));
  Tensor x;                             // the residual and the backward read the input the pass above completed
  ISHAP_TRY(finished(in, "the attention block's residual", x));
  Tensor qkv{nullptr, N, x.H, x.W, 3 * C};
  ISHAP_ALLOC(qkv.p, e, qkv.numel());
  Tensor a = shaped(x);                 // ahead of the plain route's qkv conv_op, which allocates nothing (no pend_out): the arena order holds
  ISHAP_ALLOC(a.p, e, a.numel());
  sv = AttnSaved{x, qkv, a, st, lse};
  if (attn8_applicable(N, T, C, d) && L.qkv.kpad == C && L.proj.kpad == C && small_map(T)) {
    // 8x8 map: qkv GEMM + attention + proj_out in ONE launch (attention.hip, attn8_fused_kernel); proj_out leaves as per-head
    // K slices that the next GroupNorm pass adds up with its bias and the residual x (ISHAP_ATTN8=1).  The route depends on the
    // shape only: a sequence without the rendezvous tenancy (a second context, the deferred forward tail's replay) makes the same
    // allocations and runs the same kernel as two launches -- the same bits (round 6)
    float* slices = nullptr; ISHAP_ALLOC(slices, e, (size_t)heads * N * T * C);
    long long* fl = nullptr; ISHAP_SALLOC(fl, e, (size_t)N * heads * 8);   // 16 flags of 4 bytes per (image, head), zeroed with the statistics arena
    y = Flow{shaped(x)};
    ISHAP_ALLOC(y.t.p, e, x.numel());
    y.pend.ws = slices; y.pend.nslab = heads; y.pend.zstride = (long long)N * T * C;
    y.pend.bias = L.proj.bias; y.pend.res = x.p; y.pend.ldr = C;
    Attn8Args g;
    g.xn = nrm.p; g.wqkv = L.qkv.w; g.bqkv = L.qkv.bias; g.wproj = L.proj.w; g.qkv = qkv.p; g.aout = a.p; g.lse = lse;
    g.slices = slices; g.flags = reinterpret_cast<unsigned*>(fl);
    g.N = N; g.C = C; g.heads = heads; g.alpha = 1.f / sqrtf((float)d);
    return e.launch([g, solo = exec_is_solo(e)](hipStream_t s) mutable {
      g.status = ishap_status_word();        // looked up at the launch: a dry run allocates nothing
      ISHAP_REQUIRE(g.status != nullptr, "device status word");
      return attn8_fused_launch(g, s, solo);
    });
  }
  ISHAP_TRY(conv_op(e, conv_launch(nrm, L.qkv, qkv)));
  // fused flash-style attention: w = softmax((q*s)^T (k*s)), a = w v   (unet.py:347-353)
  AttnArgs g;
  g.qkv = qkv.p; g.out = a.p; g.lse = lse; g.N = N; g.T = T; g.C = C; g.heads = heads; g.d = d;
  g.alpha = 1.f / sqrtf((float)d);
  g.xcd_map = attn_xcd_setting();
  ISHAP_TRY(e.launch([g](hipStream_t s) { return attn_forward_launch(g, s); }));
  y = Flow{shaped(x)};
  ISHAP_ALLOC(y.t.p, e, x.numel());
  const bool nosum = small_map(T);
  if (!nosum) ISHAP_SALLOC(y.t.sums, e, (size_t)N * C * 2);
  ConvLaunch kp = conv_launch(a, L.proj, y.t);
  kp.res = x.p; kp.ldr = C; kp.pend_out = nosum ? &y.pend : nullptr;
  return conv_op(e, kp);
}

static int block_forward(Exec& e, BlockL& b, Flow h, Flow& out) {
  ishap_unet* u = e.u;
  for (auto& l : b.layers) {
    Flow y;
    if (l.kind == 0) {
      Tensor x;
      ISHAP_TRY(finished(h, "the stem convolution", x));
      y.t = shaped(x, u->stem.cout);
      ISHAP_ALLOC(y.t.p, e, y.t.numel());
      if (!small_map(x.H * x.W)) ISHAP_SALLOC(y.t.sums, e, (size_t)x.N * u->stem.cout * 2);
      ISHAP_TRY(conv_op(e, conv_launch(x, u->stem, y.t)));
    } else if (l.kind == 1) {
      ISHAP_TRY(res_forward(e, u->res[l.idx], u->kept.res[l.idx], h, y));
    } else {
      ISHAP_TRY(attn_forward(e, u->attn[l.idx], u->kept.attn[l.idx], h, y));
    }
    h = y;
  }
  out = h;
  u->kept.out[b.slot] = filled_by_next_gn(h);
  return 0;
}

// order `s` behind a forward tail that is still running on the context's side stream (no-op when there is none)
int unet_run_tail(ishap_unet* u);
int unet_join_tail(ishap_unet* u, hipStream_t s) {
  if (u->tail_deferred) ISHAP_TRY(unet_run_tail(u));     // planned but never enqueued: enqueue it now
  if (!u->tail_pending) return 0;
  ISHAP_CHECK_HIP(hipStreamWaitEvent(s, u->ev_tail, 0));
  u->tail_pending = false;
  return 0;
}

// the launch-sequence settings of the forward tail on the context's side stream
static void tail_exec(Exec& e, ishap_unet* u) {
  e.s = u->side;
  e.ws = u->ws_side;
  e.gn_partial = u->gn_partial_side;
  // the tail's 3x3 convolutions as launches of at most P tiles: it then holds the LDS of at most P compute units at a time and
  // the backward chain on the caller's stream keeps the rest.  In-situ sweep with the start point (profiles/round5_overlap_tail_ab.txt):
  // 96 / 112 / 128 / 144 / 160 / 192 / 256 tiles -> 0.1706 / 0.1707 / 0.1682 / 0.1707 / 0.1714 / 0.1727 / 0.1785 s per edit
  static const int wgs = ishap_switch("ISHAP_TAIL_DEFER_WGS", 128);
  e.chunk_tiles = wgs;
}

// output blocks [i0, i1): skip concatenation + block (gd/unet.py:661-664); records the tap after block `feat_layer`
static int out_blocks_range(Exec& e, ishap_unet* u, size_t i0, size_t i1, Flow& h, std::vector<Tensor>& hs, int feat_layer) {
  for (size_t i = i0; i < i1; ++i) {
    BlockL& b = u->out_blocks[i];
    const Tensor skip = hs.back();
    hs.pop_back();
    Flow cat{shaped(h.t, h.t.C + skip.C)};
    Tensor& c = cat.t;
    ISHAP_REQUIRE(skip.H == c.H && c.C == b.cin, "skip connection shape");
    ISHAP_ALLOC(c.p, e, c.numel());
    const bool first_is_res = b.layers[0].kind == 1;
    if (first_is_res && local_gn(c.H * c.W, c.C)) {
      // no copy pass: the ResBlock's first (group-local) GroupNorm reads both halves -- adding up h if it is still
      // pending -- and writes the concatenation as it goes
      cat.cat = LazyCat{h.t.p, skip.p, nullptr, nullptr, h.t.C};
      cat.cat_pend = h.take();
    } else {
      ISHAP_TRY(slab_materialize(e, h));
      Tensor a;
      ISHAP_TRY(finished(h, "the skip concatenation of a large map", a));
      if (first_is_res && a.sums && skip.sums && a.C % 8 == 0) {
        cat.cat = LazyCat{a.p, skip.p, a.sums, skip.sums, a.C};     // no copy pass either: the apply kernel reads both halves and their sums
      } else {
        c.sums = (a.sums && skip.sums) ? salloc(e, (size_t)c.N * c.C * 2) : nullptr;
        ISHAP_TRY(e.launch([=](hipStream_t s) { return concat2(a.p, skip.p, c.p, c.rows(), a.C, skip.C, s, a.sums, skip.sums, c.sums, c.N); }));
      }
    }
    u->kept.cat[b.slot] = filled_by_next_gn(cat);
    ISHAP_TRY(block_forward(e, b, cat, h));
    if ((int)i == feat_layer) u->kept.tap = filled_by_next_gn(h);
  }
  return 0;
}

// ---- head in fp32 (unet.py:667-669): GroupNorm, SiLU, 3x3 conv with fp32 weights.  The fp32 products are
//      formed on the fp16 MFMA from hi/lo splits of both operands (3 partial products, fp32 accumulate). ----
static int forward_head(Exec& e, ishap_unet* u, Flow h, int N, float* out) {
  const int S = u->cfg.image_size;
  ISHAP_ALLOC(u->kept.head_stats, e, (size_t)N * 64);
  half_t* hsplit = nullptr; ISHAP_ALLOC(hsplit, e, (size_t)h.t.numel() * 3);
  ISHAP_TRY(gn_forward_op(e, h, u->head_norm, hsplit, nullptr, u->kept.head_stats, nullptr, 0, 1, 0, 1));
  ISHAP_TRY(finished(h, "the record of the head's input", u->kept.h_final));
  ConvLaunch c = conv_launch(Tensor{hsplit, N, S, S, 3 * h.t.C}, u->head, Tensor{nullptr, N, S, S, 0});
  c.out = out; c.out_mode = IG_OUT_NCHW_F32;      // NCHW fp32: no row stride
  return conv_op(e, c);
}

// the deferred forward tail (ISHAP_TAIL_DEFER): the launches unet_forward_impl recorded, on the side stream, behind the event the
// backward recorded after its first blocks (or behind the fork when it recorded none)
int unet_run_tail(ishap_unet* u) {
  if (!u->tail_deferred) return 0;
  u->tail_deferred = false;
  const bool marks = u->marks_on && u->marks_n > 0;      // diagnostic marks (unet.h): the tail's span on the side stream
  auto body = [&]() -> int {
    ISHAP_CHECK_HIP(hipStreamWaitEvent(u->side, u->mid_recorded ? u->ev_mid : u->ev_fork, 0));
    if (marks) {
      if (!u->mark_tail_begin) { ISHAP_CHECK_HIP(hipEventCreate(&u->mark_tail_begin)); ISHAP_CHECK_HIP(hipEventCreate(&u->mark_tail_end)); }
      ISHAP_CHECK_HIP(hipEventRecord(u->mark_tail_begin, u->side));
    }
    for (auto& launch : u->tail_tape) ISHAP_TRY(launch(u->side));
    if (marks) {
      ISHAP_CHECK_HIP(hipEventRecord(u->mark_tail_end, u->side));
      u->mark_tail_set = true;
    }
    return 0;
  };
  const int r = body();
  // on EVERY exit path: whatever was enqueued on the side stream before a failure is closed by ev_tail, so that the next join
  // (forward, full-depth backward, read-out) still orders behind it before the arena or `out` is reused
  if (hipEventRecord(u->ev_tail, u->side) == hipSuccess) u->tail_pending = true;
  else if (r == 0) { ishap_set_error("hipEventRecord(ev_tail) failed after the deferred forward tail"); return -1; }
  return r;
}

int unet_forward_impl(ishap_unet* u, const float* x, const float* ts, int N, int feat_layer, float* out,
                      void* inter_feat, int keep, hipStream_t s, bool dry) {
  const ishap_unet_config& cfg = u->cfg;
  ISHAP_REQUIRE(N >= 1 && N <= cfg.max_batch && N <= 16, "batch size outside [1, max_batch]");
  ISHAP_REQUIRE(feat_layer < (int)u->out_blocks.size(), "feat_layer out of range");
  Exec e{u, s, dry};
  TenancyScope tenancy(u, s, dry);       // in-launch rendezvous only while no other context / stream of the process runs such grids here
  e.tenant = tenancy.granted;
  KeptForward& k = u->kept;
  // the overlapped tail fills what ONE edit leaves idle; when another context / stream of the process is running sequences on the
  // device (no tenancy: common.h) the chip is shared already and a second stream per edit only oversubscribes the hardware
  // queues (three interleaved edits: 0.120 s/shape in the plain sequence, 0.248 with three overlapped tails, 0.143 with the
  // tenant's alone): also not while anyone else has asked for the device since this context's last sequence
  const bool overlap = (keep & 2) != 0 && !dry && feat_layer >= 0 && feat_layer + 1 < (int)u->out_blocks.size() && tenancy.granted &&
                       !ishap_rendezvous_contended(u, s);
  if (!dry) ISHAP_TRY(unet_join_tail(u, s));       // the previous forward's tail still owns the arena it is about to reuse
  if (!dry && u->snap.valid && (u->snap.kept.N != N || u->snap.kept.feat != feat_layer)) u->snap.valid = false;   // another shape of call
  if (overlap && !u->side) {
    // lowest priority: the tail is throughput work that should fill what the latency-bound chain on the caller's stream
    // leaves idle, not compete with it for compute units
    int prio_least = 0, prio_greatest = 0;
    ISHAP_CHECK_HIP(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    ISHAP_CHECK_HIP(hipStreamCreateWithPriority(&u->side, hipStreamNonBlocking, prio_least));
    ISHAP_CHECK_HIP(hipEventCreateWithFlags(&u->ev_fork, ishap_event_flags()));
    ISHAP_CHECK_HIP(hipEventCreateWithFlags(&u->ev_tail, ishap_event_flags()));
    ISHAP_CHECK_HIP(hipEventCreateWithFlags(&u->ev_mid, ishap_event_flags()));
    if (u->ws_floats) ISHAP_CHECK_HIP(hipMalloc((void**)&u->ws_side, u->ws_floats * sizeof(float)));
    ISHAP_CHECK_HIP(hipMalloc((void**)&u->gn_partial_side, std::max<size_t>(u->gn_partial_floats, 64) * sizeof(float)));
  }
  u->arena.reset();
  u->stat_off = 0;
  u->seq++;                     // the arena is reused from here on: the last backward's gradient maps are gone
  // the statistics arena is zeroed by the layout conversion below (its first use comes after it)
  const bool zero_in_convert = (u->stat_cap % 2 == 0) && (reinterpret_cast<uintptr_t>(u->stat_base) & 15) == 0;
  if (!dry && u->stat_cap && !zero_in_convert) ISHAP_CHECK_HIP(hipMemsetAsync(u->stat_base, 0, u->stat_cap * sizeof(long long), s));
  k.have_saved = false;
  k.restored_partial = false;
  const int S = cfg.image_size, HW = S * S;
  // ---- timestep embedding -> emb -> every ResBlock's (scale | shift)   (unet.py:651, :245-250) ----
  k.film = u->d_film;
  k.film_ld = u->film_rows;
  bool prepared = false;
  if (!dry && !u->film_cache_ts.empty()) {
    bool same = true;
    for (int i = 1; i < N; ++i) same = same && ts[i] == ts[0];
    if (same)
      for (size_t i = 0; i < u->film_cache_ts.size() && !prepared; ++i)
        if (u->film_cache_ts[i] == ts[0]) {
          k.film = u->film_cache + i * (size_t)u->film_rows;
          k.film_ld = 0;
          prepared = true;
        }
  }
  if (!prepared) {
    TsArg ta;
    for (int i = 0; i < 16; ++i) ta.t[i] = i < N ? ts[i] : 0.f;
    ISHAP_TRY(e.launch([=](hipStream_t s) {
      ISHAP_TRY(timestep_embedding(ta, u->d_temb, N, u->cfg.model_channels, s));
      ISHAP_TRY(gemv_f32(u->te_w0, u->te_b0, u->d_temb, u->d_e1, u->ted, u->cfg.model_channels, N, 0, s));
      ISHAP_TRY(gemv_f32(u->te_w2, u->te_b2, u->d_e1, u->d_emb, u->ted, u->ted, N, 1, s));
      return gemv_f32(u->emb_w, u->emb_b, u->d_emb, u->d_film, u->film_rows, u->ted, N, 1, s);
    }));
  }
  // ---- x: NCHW fp32 -> NHWC fp16 (h = x.type(self.dtype), unet.py:657) ----
  k.x0 = Tensor{nullptr, N, S, S, u->in_pad};
  ISHAP_ALLOC(k.x0.p, e, k.x0.numel());
  ISHAP_TRY(e.launch([=, x0 = k.x0.p](hipStream_t s) {
    return nchw_f32_to_nhwc_f16(x, x0, N, u->cfg.in_channels, HW, u->in_pad, s, zero_in_convert ? u->stat_base : nullptr,
                                zero_in_convert ? u->stat_cap * sizeof(long long) : 0);
  }));
  Flow h{k.x0};
  std::vector<Tensor> hs;
  for (auto& b : u->in_blocks) {
    ISHAP_TRY(block_forward(e, b, h, h));
    hs.push_back(filled_by_next_gn(h));
  }
  ISHAP_TRY(block_forward(e, u->mid, h, h));
  k.tap = Tensor{};
  const size_t n_out = u->out_blocks.size();
  const size_t split = overlap ? (size_t)feat_layer + 1 : n_out;
  ISHAP_TRY(out_blocks_range(e, u, 0, split, h, hs, feat_layer));
  if (overlap) {
    // everything after the tap needs only what exists now; whatever the caller enqueues on `s` after this call (loss,
    // backward) needs nothing of what follows: fork
    ISHAP_TRY(slab_materialize(e, h));             // the tap is complete on the caller's stream
    ISHAP_TRY(finished(h, "the tap at the fork", k.tap));
    ISHAP_CHECK_HIP(hipEventRecord(u->ev_fork, s));
    // DEFERRED tail (round 5: -2.2 % against a tail enqueued here, at the tap; that form was removed in round 6): the rest is
    // allocated now -- so that the caller's backward gets its scratch above the whole forward -- and its launches are recorded
    // once, with the settings they run under; ishap_unet_run_tail enqueues them later, behind an event the backward records
    // after its first blocks (the tail then runs beside the backward's latency-bound middle, not beside its chip-filling first
    // and last launches)
    k.tail_arena_off = u->arena.off;
    k.tail_stat_off = u->stat_off;
    u->tail_tape.clear();
    Exec rec{u, u->side, false};
    rec.tenant = false;
    rec.tape = &u->tail_tape;
    tail_exec(rec, u);
    ISHAP_TRY(out_blocks_range(rec, u, split, n_out, h, hs, feat_layer));
    ISHAP_TRY(forward_head(rec, u, h, N, out));
    u->tail_deferred = true;
    u->mid_recorded = false;
  } else {
    ISHAP_TRY(forward_head(e, u, h, N, out));
  }
  if (feat_layer >= 0 && inter_feat)
    ISHAP_TRY(e.launch([=, t = k.tap](hipStream_t s) { return nhwc_f16_to_nchw(t.p, inter_feat, 0, N, t.C, t.H * t.W, t.C, s); }));
  k.N = N;
  k.feat = feat_layer;
  k.tail_planned = overlap;
  k.have_saved = (keep & 1) != 0 && !dry;
  k.fwd_mark = u->arena.off;
  k.stat_fwd_mark = u->stat_off;
  k.bwd_since_fwd = 0;
  return 0;
}

// ---- helper of the snapshot calls below ----
template <typename T>
static int snap_reserve(T** buf, size_t* cap, size_t need) {
  if (need <= *cap) return 0;
  if (*buf) ISHAP_CHECK_HIP(hipFree(*buf));         // hipFree waits for work that may still read it
  *buf = nullptr;
  *cap = 0;
  ISHAP_CHECK_HIP(hipMalloc((void**)buf, need * sizeof(T)));
  *cap = need;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int ishap_version(void) { return 27; }  // 2: ishap_mesh_smooth takes the scratch size; 3: ishap_step_coefs carries the rng fields;
                                        // 4: batched drag edits (ishap_drag_batch_*, ishap_ddpm_step_guided_scales);
                                        // 5: one implicit-GEMM launch through the ABI (ishap_igemm_run, ishap_igemm_reduce);
                                        // 6: direct triplane fitting (ishap_triplane_fit_loss_grad, ishap_triplane_reg_*)
                                        // 7: mesh metrics (ishap_mesh_distance, ishap_hausdorff, ishap_group_field_stats)
                                        // 8: ARAP deformation (ishap_arap, ishap_arap_scratch_bytes, ishap_nearest_vertices)
                                        // 9: one attention launch through the ABI (ishap_attention_run, ishap_attention8_run)
                                        // 10: ishap_group_norm32_plan replaces ishap_group_norm32_parts
                                        // 11: headless rendering (ishap_render_mesh, ishap_render_scratch_bytes, ishap_unproject)
                                        // 12: winding numbers (ishap_mesh_winding, ishap_cloud_winding, ishap_cloud_areas,
                                        //     ishap_winding_scratch_bytes) and ishap_mesh_distance's sdf == 2 / sdf == -2 (sign by winding number,
                                        //     counter-clockwise / clockwise mesh; before 12 both meant parity, as any other non-zero value still does)
                                        // 13: one GroupNorm launch through the ABI (ishap_group_norm32_run)
                                        // 14: clouds without normals (ishap_cloud_knn, ishap_cloud_normals, ishap_cloud_orient,
                                        //     ishap_cloud_orient_scratch_bytes)
                                        // 15: snapshot of a kept forward (ishap_unet_snapshot_save / _restore / _drop / _bytes)
                                        // 16: connected components of a volume (ishap_volume_label, ishap_volume_components_*,
                                        //     ishap_volume_flip; components.hip)
                                        // 17: region weights of the drag loss (weights fields of the drag structs,
                                        //     ishap_region_plane_weights; regions.hip)
                                        // 18: the decoder's field in space (ishap_triplane_field_grad, ishap_triplane_project;
                                        //     decode_field.hip)
                                        // 19: part edits (ishap_region_select, ishap_region_handles, ishap_region_handles_scratch_bytes,
                                        //     ishap_region_transform; parts.hip)
                                        // 20: per-block gradients of the last backward (ishap_unet_block_grad)
                                        // 21: handle tracking (ishap_drag_track, ishap_drag_track_scratch_bytes; track.hip)
                                        // 22: closed-loop drag (ishap_drag_batch_retarget, ishap_drag_batch_retarget_each; retarget.hip)
                                        // 23: exact distance transform (ishap_edt, ishap_edt_scratch_bytes; edt.hip) and the regions' marks and
                                        //     feathered map (ishap_region_plane_marks, ishap_region_plane_feather[_scratch_bytes]; regions.hip)
                                        // 24: volume constraints (ishap_constraint_setup[_scratch_bytes], ishap_constraint_loss_grad;
                                        //     constrain.hip)
                                        // 25: sparse high-resolution surface (ishap_triplane_decode_bricks, ishap_sparse_*;
                                        //     sparse_surface.hip, decode.hip)
                                        // 26: quadric vertex clustering (ishap_mesh_simplify_scratch_bytes / _count / _emit; simplify.hip)
                                        // 27: the single-edit drag interface is removed (ishap_drag_args, ishap_drag_setup, ishap_drag_loss_grad,
                                        //     ishap_drag_loss_cotangent, ishap_drag_retarget): one edit is the ishap_drag_batch_* entry of the same
                                        //     name with E = 1

int ishap_unet_create(const ishap_unet_config* cfg, int device, ishap_unet** out) {
  ISHAP_REQUIRE(cfg && out, "null argument");
  ISHAP_REQUIRE(cfg->n_mult >= 1 && cfg->n_mult <= 8 && cfg->n_att <= 8, "config arrays");
  ISHAP_REQUIRE(cfg->model_channels % 32 == 0, "model_channels must be a multiple of 32 (GroupNorm32)");
  ISHAP_REQUIRE(cfg->num_head_channels > 0 && cfg->num_head_channels % 32 == 0, "num_head_channels % 32");
  ISHAP_REQUIRE(cfg->out_channels % 4 == 0, "out_channels % 4");
  ISHAP_REQUIRE(cfg->max_batch >= 1 && cfg->max_batch <= 16, "max_batch in [1,16]");
  int minres = cfg->image_size >> (cfg->n_mult - 1);
  ISHAP_REQUIRE(minres * minres >= 64 && (cfg->image_size & (cfg->image_size - 1)) == 0,
                "image_size: power of two with at least 8x8 at the deepest level");
  ISHAP_CHECK_HIP(hipSetDevice(device));
  ishap_unet* u = new ishap_unet();
  u->cfg = *cfg;
  u->marks_on = ishap_switch("ISHAP_BWD_MARKS", 0) != 0;
  u->device = device;
  int r = unet_build(u);
  if (r) { delete u; return r; }
  // size the arena / workspaces with dry runs of forward + backward at EVERY batch size a call may use: the split-K
  // policy depends on M = N*H*W, so a smaller batch can need a larger fp32 partial workspace than max_batch does
  u->arena.dry = true;
  std::vector<float> ts(cfg->max_batch, 0.f);
  for (int nb = 1; nb <= cfg->max_batch && !r; ++nb) {
    r = unet_forward_impl(u, nullptr, ts.data(), nb, (int)u->out_blocks.size() - 1, nullptr, nullptr, 1, 0, true);
    if (!r) r = unet_backward_impl(u, nullptr, (const void*)0x1000, 0, nullptr, nullptr, 0, true);   // on top of the kept forward state
  }
  if (r) { delete u; return r; }
  u->arena.dry = false;
  u->arena.cap = align_up(u->arena.high + (1 << 20), 1 << 20);
  ISHAP_CHECK_HIP(hipMalloc((void**)&u->arena.base, u->arena.cap));
  if (u->ws_floats) ISHAP_CHECK_HIP(hipMalloc((void**)&u->ws, u->ws_floats * sizeof(float)));
  ISHAP_CHECK_HIP(hipMalloc((void**)&u->gn_partial, std::max<size_t>(u->gn_partial_floats, 64) * sizeof(float)));
  u->stat_cap = (u->stat_high + 1023) / 1024 * 1024;
  ISHAP_CHECK_HIP(hipMalloc((void**)&u->stat_base, std::max<size_t>(u->stat_cap, 1024) * sizeof(long long)));
  if (u->attn_D_floats) ISHAP_CHECK_HIP(hipMalloc((void**)&u->attn_D, u->attn_D_floats * sizeof(float)));
  u->kept.have_saved = false;
  *out = u;
  return 0;
}

void ishap_unet_destroy(ishap_unet* u) {
  if (!u) return;
  auto fr = [](void* p) { if (p) (void)hipFree(p); };
  auto frc = [&](ConvW& c) { fr(c.w); fr(c.wT); fr(c.bias); if (c.cat && c.cat_off == 0) fr(c.cat); };
  frc(u->stem); frc(u->head);
  fr(u->head_norm.gamma); fr(u->head_norm.beta);
  for (auto& r : u->res) {
    frc(r.c1); frc(r.c2); if (r.has_skip) frc(r.skip);
    fr(r.n1.gamma); fr(r.n1.beta); fr(r.n2.gamma); fr(r.n2.beta);
  }
  for (auto& a : u->attn) { frc(a.qkv); frc(a.proj); fr(a.n.gamma); fr(a.n.beta); }
  fr(u->te_w0); fr(u->te_b0); fr(u->te_w2); fr(u->te_b2); fr(u->emb_w); fr(u->emb_b);
  fr(u->d_temb); fr(u->d_e1); fr(u->d_emb); fr(u->d_film);
  fr(u->film_cache); fr(u->pc_temb); fr(u->pc_e1); fr(u->pc_emb);
  fr(u->ws_side); fr(u->gn_partial_side);
  fr(u->snap.arena); fr(u->snap.stat); fr(u->snap.film);
  if (u->side) (void)hipStreamDestroy(u->side);
  if (u->ev_fork) (void)hipEventDestroy(u->ev_fork);
  if (u->ev_tail) (void)hipEventDestroy(u->ev_tail);
  if (u->ev_mid) (void)hipEventDestroy(u->ev_mid);
  for (hipEvent_t ev : u->marks) (void)hipEventDestroy(ev);
  if (u->mark_tail_begin) (void)hipEventDestroy(u->mark_tail_begin);
  if (u->mark_tail_end) (void)hipEventDestroy(u->mark_tail_end);
  fr(u->arena.base); fr(u->ws); fr(u->gn_partial); fr(u->attn_D); fr(u->stat_base);
  delete u;
}

int ishap_unet_num_params(const ishap_unet* u) { return u ? (int)u->params.size() : 0; }

int ishap_unet_param_info(const ishap_unet* u, int index, char* name, int name_cap, int* ndim, long long* shape) {
  ISHAP_REQUIRE(u && index >= 0 && index < (int)u->params.size(), "param index");
  const ParamSlot& p = u->params[index];
  if (name && name_cap > 0) {
    std::strncpy(name, p.name.c_str(), name_cap - 1);
    name[name_cap - 1] = 0;
  }
  if (ndim) *ndim = p.ndim;
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = p.shape[i];
  return 0;
}

int ishap_unet_load_param(ishap_unet* u, const char* name, const float* data, long long numel, void* stream) {
  ISHAP_REQUIRE(u && name && data, "null argument");
  auto it = u->param_index.find(name);
  ISHAP_REQUIRE(it != u->param_index.end(), std::string("unexpected key in state_dict: ") + name);
  ParamSlot& p = u->params[it->second];
  ISHAP_REQUIRE(p.numel() == numel, std::string("size mismatch for ") + name);
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  ISHAP_TRY(load_param(u, p, data, (hipStream_t)stream));
  if (!p.loaded) { p.loaded = true; u->n_loaded++; }
  u->film_cache_ts.clear();            // rows prepared from the previous weights are stale
  u->snap.valid = false;               // and so is a snapshot of a forward through them
  return 0;
}

// (scale | shift) rows of all ResBlocks for n timesteps, computed once ahead of a sampling loop: forwards at these
// timesteps then skip timestep_embedding + time_embed + the emb_layers GEMV (gd/unet.py:651 and :245-250 do not depend on
// x).  n = 0 drops the prepared rows.  Same kernels as the in-forward path, so the values are bit-identical.
int ishap_unet_prepare_timesteps(ishap_unet* u, const float* ts, int n, void* stream) {
  ISHAP_REQUIRE(u && (ts || n == 0) && n >= 0 && n <= 4096, "prepare_timesteps arguments");
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  hipStream_t s = (hipStream_t)stream;
  u->film_cache_ts.clear();
  // a kept forward may be reading a prepared row (its backward needs the FiLM values again): the rows are about to be
  // rewritten, so that forward can no longer be differentiated
  if (u->kept.film != u->d_film) { u->kept.have_saved = false; u->kept.film = u->d_film; u->kept.film_ld = u->film_rows; }
  if (n == 0) return 0;
  ISHAP_REQUIRE(u->n_loaded == (int)u->params.size(), "prepare_timesteps before all parameters are loaded");
  const int mc = u->cfg.model_channels;
  if ((size_t)n > u->film_cache_rows) {
    if (u->film_cache) ISHAP_CHECK_HIP(hipFree(u->film_cache));      // hipFree waits for work that may still read it
    u->film_cache = nullptr;
    u->film_cache_rows = 0;
    ISHAP_CHECK_HIP(hipMalloc((void**)&u->film_cache, (size_t)n * u->film_rows * sizeof(float)));
    u->film_cache_rows = (size_t)n;
  }
  if (!u->pc_temb) {
    ISHAP_CHECK_HIP(hipMalloc((void**)&u->pc_temb, (size_t)16 * mc * sizeof(float)));
    ISHAP_CHECK_HIP(hipMalloc((void**)&u->pc_e1, (size_t)16 * u->ted * sizeof(float)));
    ISHAP_CHECK_HIP(hipMalloc((void**)&u->pc_emb, (size_t)16 * u->ted * sizeof(float)));
  }
  for (int c0 = 0; c0 < n; c0 += 16) {
    const int m = std::min(16, n - c0);
    TsArg ta;
    for (int i = 0; i < 16; ++i) ta.t[i] = i < m ? ts[c0 + i] : 0.f;
    ISHAP_TRY(timestep_embedding(ta, u->pc_temb, m, mc, s));
    ISHAP_TRY(gemv_f32(u->te_w0, u->te_b0, u->pc_temb, u->pc_e1, u->ted, mc, m, 0, s));
    ISHAP_TRY(gemv_f32(u->te_w2, u->te_b2, u->pc_e1, u->pc_emb, u->ted, u->ted, m, 1, s));
    ISHAP_TRY(gemv_f32(u->emb_w, u->emb_b, u->pc_emb, u->film_cache + (size_t)c0 * u->film_rows, u->film_rows, u->ted, m, 1, s));
  }
  u->film_cache_ts.assign(ts, ts + n);
  return 0;
}

int ishap_unet_params_loaded(const ishap_unet* u) { return u ? u->n_loaded : 0; }

int ishap_unet_join_tail(ishap_unet* u, void* stream) {
  ISHAP_REQUIRE(u, "null argument");
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  return unet_join_tail(u, (hipStream_t)stream);
}

int ishap_unet_run_tail(ishap_unet* u) {
  ISHAP_REQUIRE(u, "null argument");
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  return unet_run_tail(u);
}

int ishap_unet_forward(ishap_unet* u, const float* x, const float* timesteps, int N, int feat_layer, float* out,
                       void* inter_feat, int keep_for_backward, void* stream) {
  ISHAP_REQUIRE(u && x && timesteps && out, "null argument");
  ISHAP_REQUIRE(u->n_loaded == (int)u->params.size(), "missing keys: not every state_dict tensor has been loaded");
  ISHAP_TRY(ishap_check_status());          // an earlier launch's device-side failure surfaces here
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  return unet_forward_impl(u, x, timesteps, N, feat_layer, out, inter_feat, keep_for_backward, (hipStream_t)stream, false);
}

int ishap_unet_tap_shape(const ishap_unet* u, int feat_layer, int* channels, int* size) {
  ISHAP_REQUIRE(u && feat_layer >= 0 && feat_layer < (int)u->out_blocks.size(), "feat_layer out of range");
  if (channels) *channels = u->out_blocks[feat_layer].cout;
  if (size) *size = u->out_blocks[feat_layer].res_out;
  return 0;
}

const void* ishap_unet_tap_ptr(const ishap_unet* u) { return u ? u->kept.tap.p : nullptr; }

long long ishap_unet_workspace_bytes(const ishap_unet* u) {
  if (!u) return 0;
  return (long long)(u->arena.cap + u->ws_floats * sizeof(float) + u->gn_partial_floats * sizeof(float) +
                     u->stat_cap * sizeof(long long) + u->attn_D_floats * sizeof(float) + u->snap.bytes());
}

int ishap_unet_block_output(const ishap_unet* u, int group, int index, int* channels, int* size, void* dst_nchw_f16,
                            void* stream) {
  ISHAP_REQUIRE(u && group >= 0 && group <= 2, "group: 0 input_blocks, 1 middle_block, 2 output_blocks");
  const BlockL* b = nullptr;
  if (group == 0) { ISHAP_REQUIRE(index >= 0 && index < (int)u->in_blocks.size(), "input block index"); b = &u->in_blocks[index]; }
  else if (group == 1) b = &u->mid;
  else { ISHAP_REQUIRE(index >= 0 && index < (int)u->out_blocks.size(), "output block index"); b = &u->out_blocks[index]; }
  if (channels) *channels = b->cout;
  if (size) *size = b->res_out;
  if (!dst_nchw_f16) return 0;
  const Tensor& t = u->kept.out[b->slot];
  ISHAP_REQUIRE(u->kept.have_saved && t.p, "block outputs stay resident only after a forward with keep_for_backward=1");
  ISHAP_REQUIRE(!(u->kept.restored_partial && group == 2 && index > u->kept.feat), "the restored snapshot holds the network up to the tap only");
  ISHAP_TRY(ishap_check_status());
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  ISHAP_TRY(unet_join_tail(const_cast<ishap_unet*>(u), (hipStream_t)stream));
  return nhwc_f16_to_nchw(t.p, dst_nchw_f16, 0, t.N, t.C, t.H * t.W, t.C, (hipStream_t)stream);
}

int ishap_unet_block_grad(const ishap_unet* u, int group, int index, int part, int* channels, int* size, void* dst_nchw_f16,
                          void* stream) {
  ISHAP_REQUIRE(u && group >= 0 && group <= 2, "group: 0 input_blocks, 1 middle_block, 2 output_blocks");
  ISHAP_REQUIRE(part >= 0 && part <= 2, "part: 0 gradient w.r.t. the block output, 1 / 2 w.r.t. the h / skip half of an output block's input");
  ISHAP_REQUIRE(part == 0 || group == 2, "parts 1 and 2 (the [h | skip] halves) exist for output blocks only");
  const BlockL* b = nullptr;
  if (group == 0) { ISHAP_REQUIRE(index >= 0 && index < (int)u->in_blocks.size(), "input block index"); b = &u->in_blocks[index]; }
  else if (group == 1) b = &u->mid;
  else { ISHAP_REQUIRE(index >= 0 && index < (int)u->out_blocks.size(), "output block index"); b = &u->out_blocks[index]; }
  if (channels) *channels = part == 0 ? b->cout : (part == 1 ? b->cin - b->skip_ch : b->skip_ch);
  if (size) *size = part == 0 ? b->res_out : b->res_in;
  if (!dst_nchw_f16) return 0;
  ISHAP_REQUIRE(u->grad_seq != 0, "block gradients exist only after a backward pass on this context");
  ISHAP_REQUIRE(u->grad_seq == u->seq, "stale block gradients: a forward, a backward or a snapshot restore ran after the pass that wrote them");
  ISHAP_REQUIRE(!(u->kept.restored_partial && group == 2 && index > u->kept.feat), "the restored snapshot holds the network up to the tap only");
  ISHAP_REQUIRE(!(group == 2 && index > u->grad_F), "the last backward started below this output block: it has no gradient");
  const Tensor& t = part == 0 ? b->gout : (part == 1 ? b->gh : b->gs);
  ISHAP_REQUIRE(t.p != nullptr, "no gradient was recorded for this block");
  ISHAP_TRY(ishap_check_status());
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  return nhwc_f16_to_nchw(t.p, dst_nchw_f16, 0, t.N, t.C, t.H * t.W, t.C, (hipStream_t)stream);
}

int ishap_unet_copy_tap(const ishap_unet* u, void* dst, void* stream) {
  ISHAP_REQUIRE(u && dst && u->kept.tap.p, "no resident tap (run a forward with feat_layer >= 0 first)");
  ISHAP_CHECK_HIP(hipMemcpyAsync(dst, u->kept.tap.p, (size_t)u->kept.tap.numel() * sizeof(half_t), hipMemcpyDeviceToDevice,
                                 (hipStream_t)stream));
  return 0;
}

// ---- snapshot of a kept forward: the drag loop's first guided step has the same input, timestep and weights in every edit of
//      a loaded shape, so its forward is run once and put back for the later edits (two device copies instead of the launches
//      up to the tap and the tail) ----
int ishap_unet_snapshot_save(ishap_unet* u, void* stream) {
  ISHAP_REQUIRE(u, "null argument");
  ISHAP_REQUIRE(u->kept.have_saved, "a snapshot needs a preceding forward with keep_for_backward=1");
  if (ishap_profile_recording()) return 1;         // unavailable: the recorded edit runs (and counts) every forward
  if (u->snap.film && u->kept.film == u->snap.film) {       // the kept state IS the restored snapshot
    ISHAP_REQUIRE(u->snap.valid, "the kept state came from a snapshot that is no longer valid");
    return 0;
  }
  ISHAP_TRY(ishap_check_status());
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  hipStream_t s = (hipStream_t)stream;
  ISHAP_TRY(unet_join_tail(u, s));
  UnetSnapshot& sn = u->snap;
  sn.valid = false;
  const KeptForward& k = u->kept;
  sn.partial = k.tail_planned;
  sn.arena_bytes = sn.partial ? k.tail_arena_off : k.fwd_mark;
  sn.stat_count = sn.partial ? k.tail_stat_off : k.stat_fwd_mark;
  sn.film_floats = (size_t)u->film_rows * (k.film_ld ? (size_t)k.N : 1);
  ISHAP_REQUIRE(sn.arena_bytes <= u->arena.cap && sn.stat_count <= u->stat_cap, "forward marks beyond the arenas");
  ISHAP_TRY(snap_reserve(&sn.arena, &sn.arena_cap, sn.arena_bytes));
  ISHAP_TRY(snap_reserve(&sn.stat, &sn.stat_cap, sn.stat_count));
  ISHAP_TRY(snap_reserve(&sn.film, &sn.film_cap, sn.film_floats));
  if (sn.arena_bytes) ISHAP_CHECK_HIP(hipMemcpyAsync(sn.arena, u->arena.base, sn.arena_bytes, hipMemcpyDeviceToDevice, s));
  if (sn.stat_count) ISHAP_CHECK_HIP(hipMemcpyAsync(sn.stat, u->stat_base, sn.stat_count * sizeof(long long), hipMemcpyDeviceToDevice, s));
  ISHAP_CHECK_HIP(hipMemcpyAsync(sn.film, k.film, sn.film_floats * sizeof(float), hipMemcpyDeviceToDevice, s));
  sn.kept = k;
  sn.valid = true;
  return 0;
}

int ishap_unet_snapshot_restore(ishap_unet* u, void* stream) {
  ISHAP_REQUIRE(u, "null argument");
  UnetSnapshot& sn = u->snap;
  ISHAP_REQUIRE(sn.valid, "no valid snapshot (none saved, or the weights / the batch size / the tapped block changed since)");
  if (ishap_profile_recording()) return 1;         // unavailable: the caller runs the ordinary forward
  ISHAP_TRY(ishap_check_status());
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  hipStream_t s = (hipStream_t)stream;
  ISHAP_TRY(unet_join_tail(u, s));                 // a tail still in flight reads (and owns) the arena about to be overwritten
  u->kept.have_saved = false;
  u->seq++;                                        // the gradient maps of a backward before this restore belong to another forward
  if (sn.arena_bytes) ISHAP_CHECK_HIP(hipMemcpyAsync(u->arena.base, sn.arena, sn.arena_bytes, hipMemcpyDeviceToDevice, s));
  if (sn.stat_count) ISHAP_CHECK_HIP(hipMemcpyAsync(u->stat_base, sn.stat, sn.stat_count * sizeof(long long), hipMemcpyDeviceToDevice, s));
  u->kept = sn.kept;                               // have_saved comes back with it: a snapshot is only taken of a kept forward
  u->arena.off = u->kept.fwd_mark; u->stat_off = u->kept.stat_fwd_mark;
  u->kept.film = sn.film;                          // the snapshot's own rows: a later prepare_timesteps may rewrite the cache
  u->kept.tail_planned = false;                    // no tail is planned or deferred: the snapshot holds none
  u->tail_deferred = false;
  u->mid_recorded = false;
  u->kept.restored_partial = sn.partial;
  u->kept.bwd_since_fwd = 1;                       // the statistics scratch above the mark is whatever the last backward left:
  return 0;                                        // the next backward zeroes it, as a second backward on one forward does
}

int ishap_unet_snapshot_drop(ishap_unet* u) {
  ISHAP_REQUIRE(u, "null argument");
  ISHAP_CHECK_HIP(hipSetDevice(u->device));
  UnetSnapshot& sn = u->snap;
  sn.valid = false;
  if (u->kept.restored_partial || u->kept.film == sn.film) u->kept.have_saved = false;    // the kept state reads the rows about to be freed
  if (u->kept.film == sn.film) { u->kept.film = u->d_film; u->kept.film_ld = u->film_rows; }
  if (sn.arena) ISHAP_CHECK_HIP(hipFree(sn.arena));
  sn.arena = nullptr; sn.arena_cap = 0;
  if (sn.stat) ISHAP_CHECK_HIP(hipFree(sn.stat));
  sn.stat = nullptr; sn.stat_cap = 0;
  if (sn.film) ISHAP_CHECK_HIP(hipFree(sn.film));
  sn.film = nullptr; sn.film_cap = 0;
  return 0;
}

long long ishap_unet_snapshot_bytes(const ishap_unet* u) { return u ? (long long)u->snap.bytes() : 0; }

}  // extern "C"
