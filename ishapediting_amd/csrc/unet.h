// UNet graph + executor (host side).  Structure mirrors guided_diffusion/unet.py:427-616.
#pragma once
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/ishap.h"
#include "common.h"

// A finished activation, or the buffer it will be in once the op being built has run.  Everything kept for later readers is one.
struct Tensor {
  half_t* p = nullptr;
  int N = 0, H = 0, W = 0, C = 0;
  long long* sums = nullptr;   // [N][C][2] per-channel (sum, sum of squares), fixed point, gathered by the producer; or null
  long long rows() const { return (long long)N * H * W; }
  long long numel() const { return rows() * C; }
};
// a tensor of t's shape, with C channels when given: no buffer, no sums (new tensors are made from shapes, never from copies)
inline Tensor shaped(const Tensor& t, int C = 0) { return Tensor{nullptr, t.N, t.H, t.W, C > 0 ? C : t.C}; }

// a skip concatenation nobody has written yet: the first consumer (the ResBlock's GroupNorm pass) fills the Flow's t.p while it
// reads the two halves (a: the first ca channels, with the sums sa; b: the rest, with the sums sb)
struct LazyCat { const half_t *a = nullptr, *b = nullptr; const long long *sa = nullptr, *sb = nullptr; int ca = 0; };
// The value that walks from layer to layer: a Tensor plus the state that exists only between a producer and its first consumer.
// Read t's shape and allocate its buffer freely; t as a VALUE leaves a Flow through finished() or filled_by_next_gn() only.
struct Flow {
  Tensor t;
  // t is still the split-K slices of its producer (common.h SlabSrc): t.p is where the fp16 values go once the consumer has added
  // them up; cat_pend: the same for cat.a.  Writers: conv_op (ConvLaunch::pend_out) and the fused 8x8 attention block, no one else
  SlabSrc pend, cat_pend;
  LazyCat cat;
  bool pending() const { return pend.pending() || cat_pend.pending(); }
  // THE hand-over of the pending source to the one consumer that adds the slices up (gn_local_op, gn_bwd_local_op,
  // slab_materialize; a lazy concatenation taking over its first half): nothing is pending afterwards
  SlabSrc take() { const SlabSrc s = cat.a ? cat_pend : pend; pend = cat_pend = SlabSrc{}; return s; }
};
int finished(const Flow& f, const char* who, Tensor& out);   // f as a finished Tensor; fails, naming the reader `who`, otherwise
// The one exception: a record of f for readers that come only after the next GroupNorm pass (which adds up a pending f, or
// writes a lazy concatenation into t.p) has run: block outputs and concatenations kept for the backward and the read-outs, the
// skip stack (read again only after the next block's first GroupNorm), the tap of a plain sequence
inline Tensor filled_by_next_gn(const Flow& f) { return f.t; }

struct Arena {
  char* base = nullptr;
  size_t cap = 0, off = 0, high = 0;
  bool dry = false;
  void reset() { off = 0; }
  void* alloc(size_t bytes) {
    size_t o = align_up(off, 256);
    off = o + bytes;
    if (off > high) high = off;
    if (dry) return (void*)(uintptr_t)(0x1000 + o);
    if (off > cap) return nullptr;
    return base + o;
  }
};

struct ConvW {
  std::string path;
  int cin = 0, cout = 0, taps = 9;
  int kpad = 0;        // channels per tap in the packed forward operand
  half_t* w = nullptr;   // [rows_pad(cout)][taps*kpad]
  half_t* wT = nullptr;  // [rows_pad(cin)][taps*cout_pad]  (input-gradient operand)
  int cout_pad = 0;
  float* bias = nullptr;
  bool split = false;    // fp32 head: [hi|hi|lo] packing, kpad = 3*cin
  // K-concatenated forward operand shared with another conv of the same ResBlock ([c2 3x3 | skip 1x1]): this weight is
  // also packed into cat at column cat_off (row stride cat_ld)
  half_t* cat = nullptr;
  int cat_ld = 0, cat_off = 0;
};
struct NormW {
  float* gamma = nullptr;
  float* beta = nullptr;
  int C = 0;
};

struct ResSaved {   // what the backward pass re-reads
  Tensor x, h1;         // block input, conv1 output
  float* stats1 = nullptr;
  float* stats2 = nullptr;
};
struct AttnSaved {
  Tensor x, qkv, a;
  float* stats = nullptr;
  float* lse = nullptr;
};

struct ResL {
  std::string path;
  int cin = 0, cout = 0;
  bool up = false, down = false;
  NormW n1, n2;
  ConvW c1, c2, skip;
  bool has_skip = false;
  int emb_off = 0;     // row offset into the concatenated emb_layers matrix (2*cout rows)
};
struct AttnL {
  std::string path;
  int C = 0, heads = 0;
  NormW n;
  ConvW qkv, proj;
};
struct LayerRef { int kind; int idx; };   // 0 conv(stem) 1 res 2 attn
struct BlockL {
  std::string name;
  std::vector<LayerRef> layers;
  int cin = 0, cout = 0, res_in = 0, res_out = 0, skip_ch = 0;
  int slot = 0;     // index into KeptForward::out / ::cat: the input blocks, the middle block, the output blocks
  // Read-out of the last backward (ishap_unet_block_grad): the backward scratch is bump-allocated above fwd_mark and never reused
  // within one pass, so every gradient map stays where it was written until the next forward / backward / restore on the context.
  // gout: the dense gradient w.r.t. this block's output, summed over its consumers; gh, gs (output blocks): what the first
  // ResBlock wrote for d/d[h | skip].  Valid only while ishap_unet::grad_seq == ishap_unet::seq.
  Tensor gout, gh, gs;
};

struct ParamSlot {
  std::string name;
  int ndim = 0;
  long long shape[4] = {0, 0, 0, 0};
  int kind = 0;     // 0 conv weight, 1 conv bias, 2 plain fp32 vector / matrix copied to dst + dst_off
  ConvW* conv = nullptr;
  float* dst = nullptr;
  long long dst_off = 0;
  bool loaded = false;
  long long numel() const {
    long long n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    return n;
  }
};

// Everything a kept forward leaves for later readers (the backward, the block read-outs, the snapshot): the forward writes it,
// nobody else does except a snapshot restore, which puts a saved one back.
struct KeptForward {
  int N = 0, feat = -1;              // batch size, tapped output block
  bool have_saved = false;           // the forward ran with keep_for_backward: a backward may read this record
  Tensor tap, x0, h_final;
  float* head_stats = nullptr;
  size_t fwd_mark = 0, stat_fwd_mark = 0;   // arena offsets after the forward (backward scratch goes above them)
  const float* film = nullptr;       // FiLM rows the forward / backward reads: d_film (stride film_rows) or a prepared row (stride 0)
  int film_ld = 0;
  bool tail_planned = false;         // the blocks after the tap and the head went to the deferred tail, which allocated
  size_t tail_arena_off = 0, tail_stat_off = 0;   // from these offsets up to the marks
  bool restored_partial = false;     // put back from a snapshot without the tail's blocks: no full-depth backward on it
  int bwd_since_fwd = 0;
  std::vector<ResSaved> res;         // indexed like ishap_unet::res / ::attn
  std::vector<AttnSaved> attn;
  std::vector<Tensor> out, cat;      // by BlockL::slot: block output; concat input (output blocks)
};

// A copy of what ishap_unet_backward_input reads of one kept forward (ishap_unet_snapshot_save): the bytes of the activation and
// statistics arenas below the forward's marks (below the planned tail's when one was planned: the backward from the tap reads
// nothing of the tail's blocks), the FiLM rows, and the record that points into them.  Restoring copies the bytes back to
// the same offsets, so the recorded pointers hold again.
struct UnetSnapshot {
  bool valid = false;
  bool partial = false;         // taken of a forward with a planned tail: the blocks after the tap and the head are not in it
  char* arena = nullptr;      size_t arena_cap = 0, arena_bytes = 0;
  long long* stat = nullptr;  size_t stat_cap = 0, stat_count = 0;
  float* film = nullptr;      size_t film_cap = 0, film_floats = 0;
  KeptForward kept;
  size_t bytes() const { return arena_cap + stat_cap * sizeof(long long) + film_cap * sizeof(float); }
};

struct ishap_unet {
  ishap_unet_config cfg;
  int device = 0;
  int ted = 0;                 // time_embed_dim
  int in_pad = 0;              // padded input channels of the stem
  ConvW stem, head;
  NormW head_norm;
  std::vector<ResL> res;
  std::vector<AttnL> attn;
  std::vector<BlockL> in_blocks, out_blocks;
  BlockL mid;
  int final_ch = 0;
  // embeddings
  float *te_w0 = nullptr, *te_b0 = nullptr, *te_w2 = nullptr, *te_b2 = nullptr;
  float *emb_w = nullptr, *emb_b = nullptr;   // concatenated emb_layers [film_rows][ted]
  int film_rows = 0;
  float *d_temb = nullptr, *d_e1 = nullptr, *d_emb = nullptr, *d_film = nullptr;
  // FiLM rows of timesteps prepared ahead of a sampling loop (ishap_unet_prepare_timesteps): a forward whose timesteps
  // all equal one prepared value reads its row (stride 0 over the batch) and skips the four embedding launches, among
  // them the GEMV that streams the 168 MB of emb_layers weights
  float* film_cache = nullptr;
  size_t film_cache_rows = 0;
  std::vector<float> film_cache_ts;
  float *pc_temb = nullptr, *pc_e1 = nullptr, *pc_emb = nullptr;     // 16-row scratch of the prepare call
  // parameter table
  std::vector<ParamSlot> params;
  std::map<std::string, int> param_index;
  int n_loaded = 0;
  // memory
  Arena arena;
  float* ws = nullptr;          size_t ws_floats = 0;       // split-K partials
  float* gn_partial = nullptr;  size_t gn_partial_floats = 0;
  KeptForward kept;                 // the last forward
  long long* stat_base = nullptr;   // arena of per-channel GroupNorm sums, zeroed once per forward
  size_t stat_cap = 0, stat_off = 0, stat_high = 0;
  // every forward, backward (dry runs included) and snapshot restore counts here; a backward that ran to its end leaves its count
  // in grad_seq, with the output block it started from (grad_F) -- BlockL::gout / gh / gs may be read while the two agree
  unsigned long long seq = 0, grad_seq = 0;
  int grad_F = -1;
  // Overlapped forward tail (keep_for_backward bit 1): the output blocks after the tap and the head are enqueued on a
  // stream of the context's own, forked from the caller's stream at the tap, so that they run beside the loss and the
  // backward pass the caller enqueues next (those need nothing after the tap).  ishap_unet_join_tail orders a stream
  // behind them; the next forward / a full-depth backward / a block read-out joins by itself.
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_tail = nullptr, ev_mid = nullptr;
  // diagnostic time marks (ISHAP_BWD_MARKS=1; include/ishap.h, ishap_unet_marks): timing events after every block of the backward
  // pass and around the deferred forward tail on the side stream -- un-traced per-segment durations of the overlapped step
  bool marks_on = false;
  std::vector<hipEvent_t> marks;
  std::vector<int> mark_tags;
  int marks_n = 0;
  hipEvent_t mark_tail_begin = nullptr, mark_tail_end = nullptr;
  bool mark_tail_set = false;
  bool tail_pending = false;
  // deferred tail (ISHAP_TAIL_DEFER): the forward records the tail's launches once, with the settings they run under;
  // ishap_unet_run_tail enqueues them behind ev_mid (recorded by the backward after its first output blocks)
  std::vector<std::function<int(hipStream_t)>> tail_tape;
  bool tail_deferred = false, mid_recorded = false;
  float* ws_side = nullptr;          // the side stream's own copies of the shared scratch buffers
  float* gn_partial_side = nullptr;
  float* attn_D = nullptr;      // backward attention row sums
  size_t attn_D_floats = 0;
  UnetSnapshot snap;
};

struct Exec {
  ishap_unet* u;
  hipStream_t s;
  bool dry;
  float* ws = nullptr;          // split-K / GroupNorm-statistics scratch of this launch sequence (null: the context's)
  float* gn_partial = nullptr;
  int chunk_tiles = 0;          // > 0: the dx-reuse convolutions of this sequence run as launches of at most that many tiles (the overlapped forward tail)
  bool tenant = true;           // this sequence holds the device's rendezvous tenancy (common.h ishap_rendezvous_begin)
  std::vector<std::function<int(hipStream_t)>>* tape = nullptr;   // set: launches are recorded here, not made (the deferred tail)
  // THE gate of every device launch of the forward and backward walks; f(stream) makes the launch and captures its arguments by value
  template <class F> int launch(F&& f) {
    if (tape) { tape->emplace_back(std::forward<F>(f)); return 0; }
    return dry ? 0 : f(s);
  }
};
// Arena allocation that FAILS THE CALL when the arena sized by the create-time dry runs is exceeded (a null pointer
// must never reach a kernel): ISHAP_ALLOC(ptr, e, count) inside any function returning an int status.
template <typename T>
static inline int aalloc_checked(Exec& e, size_t count, T** out) {
  *out = (T*)e.u->arena.alloc(count * sizeof(T));
  ISHAP_REQUIRE(*out != nullptr, "activation arena exhausted (shape beyond what ishap_unet_create sized for)");
  return 0;
}
#define ISHAP_ALLOC(ptr, e, count) ISHAP_TRY(aalloc_checked((e), (size_t)(count), &(ptr)))
#define ISHAP_SALLOC(ptr, e, count)                                                                   \
  do {                                                                                                \
    (ptr) = salloc((e), (size_t)(count));                                                             \
    ISHAP_REQUIRE((ptr) != nullptr, "GroupNorm statistics arena exhausted");                          \
  } while (0)
// One convolution launch (ConvLaunch, common.h): picks split-K and uses the context workspace.  With c.pend_out (the consumer is a
// group-local GroupNorm pass) a split launch leaves its slices in an arena buffer described by *c.pend_out: no reduce kernel
int conv_op(Exec& e, const ConvLaunch& c);
// the launch y = w (*) x with w's bias, gathering the sums y carries; call sites add what else they use (x: finished data)
ConvLaunch conv_launch(const Tensor& x, const ConvW& w, const Tensor& y);
int unet_join_tail(ishap_unet* u, hipStream_t s);
bool ishap_profile_recording();     // between ishap_profile_begin and ishap_profile_end (igemm.hip)
bool exec_is_solo(const Exec& e);   // no other stream of this context has work in flight (in-launch rendezvous allowed)
int slab_materialize(Exec& e, Flow& f);      // add up a pending flow with the stand-alone reduce kernel (consumers that cannot)
long long* salloc(Exec& e, size_t count);   // from the stats arena
int gn_stats_op(Exec& e, const Tensor& x, float* stats);

int unet_build(ishap_unet* u);
int unet_forward_impl(ishap_unet* u, const float* x, const float* ts, int N, int feat_layer, float* out,
                      void* inter_feat, int keep, hipStream_t s, bool dry);
int unet_backward_impl(ishap_unet* u, const half_t* cot_tap, const void* cot_out, int cot_out_f16, const float* scale2,
                       float* dx, hipStream_t s, bool dry);
