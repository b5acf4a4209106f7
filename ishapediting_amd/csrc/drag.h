#pragma once
#include "common.h"
#include <algorithm>

// ---- the sampling the drag loss (drag.hip) and the handle tracker (track.hip) share: one definition, the same bits in both ----
__device__ __forceinline__ void plane_axes(int p, int& a_col, int& a_row) {
  // grid[...,0] indexes W (columns), grid[...,1] indexes H (rows); drag_utils.py:318-321
  a_col = (p == 1) ? 1 : 0;
  a_row = (p == 0) ? 1 : 2;
}

// Lattice coordinate s + voxel * k as the reference forms it (drag_utils.py:314-316: the product rounded, then the sum).  Not
// contracted into a fused multiply-add: every call site, and the reference's float32 lattice, get the same bits.
__device__ __forceinline__ float lattice(float s, float voxel, int k) {
#pragma clang fp contract(off)
  const float o = voxel * (float)k;
  return s + o;
}

struct Bilin { int x0, y0; float w[4]; };
__device__ __forceinline__ Bilin bilin_setup(float u, float v, int W) {
#pragma clang fp contract(off)      // the same (u, v) must give the same weights at every call site (zero loss at zero displacement)
  // Texel coordinates and weights in double, rounded to float once.  In float, ix = (u + 1) / 2 * (W - 1) carries up to 2^-21 of
  // a texel of rounding that is the SAME for every channel of a position (and, at a pitch of one texel, for every position of a
  // lattice row): it does not average out, and moved the loss by 1e-7 to 2e-7 against the float64 statement of the same lattice
  // (two units in the last place of the float it is returned as).  A dozen wave-uniform operations per position.
  Bilin b;
  const double ix = (((double)u + 1.0) / 2.0) * (double)(W - 1);
  const double iy = (((double)v + 1.0) / 2.0) * (double)(W - 1);
  const double fx = floor(ix), fy = floor(iy);
  b.x0 = (int)fx; b.y0 = (int)fy;
  const double wx1 = ix - fx, wx0 = 1.0 - wx1, wy1 = iy - fy, wy0 = 1.0 - wy1;
  b.w[0] = (float)(wx0 * wy0); b.w[1] = (float)(wx1 * wy0); b.w[2] = (float)(wx0 * wy1); b.w[3] = (float)(wx1 * wy1);
  return b;
}

// one edit: what the device bodies of drag.hip work on (drag_edit_args cuts it out of a DragBatchArgs)
struct DragArgs {
  const half_t* edit = nullptr;    // current tap, NHWC fp16 [W*W][ld]
  const half_t* orig = nullptr;    // cached guidance tap, same layout
  int W = 0, ld = 0;               // feature-map side, channels of the tap
  int Cc = 0;                      // channels per plane after resize_feat_align (170 for a 512-ch tap)
  const int* chmap = nullptr;      // [3][Cc] -> channel of the tap
  const float* sources = nullptr;  // [B][3]
  const float* targets = nullptr;  // [B][3]
  int B = 0, r = 0;
  float voxel = 0.f, cof = 0.f;
  int l1 = 0;
  unsigned char* touched = nullptr;  // [3][W][W]
  int* nmask = nullptr;              // [1]
  unsigned char* chw = nullptr;      // [3][ld]: (plane, c) pairs mapped onto each tap channel (set up by drag_batch_setup_launch)
  float* grad = nullptr;             // fp32 [W*W][ld] (d loss / d tap)
  long long* gfx = nullptr;          // scratch [W*W][ld]: the scatter accumulates here in 64-bit fixed point (DRAG_FX_SCALE)
  long long* acc = nullptr;          // [2] loss sums, 64-bit fixed point (DRAG_ACC_SCALE)
  float* loss = nullptr;             // [1]
};
// ---- the touched-texel rule the setup (drag.hip, marks in global memory) and the per-step retarget (retarget.hip, marks in LDS)
// share: one definition.  touched[p][row][col] is marked where a rounded lattice texel of any source / target point lands
// (drag_utils.py:322-334).  `put(o, bit)` receives the byte offset o = (p * W + row) * W + col of a texel INSIDE the map.
template <class Mark>
__device__ __forceinline__ void drag_touch_marks(const DragArgs& a, int p, int b, int st, int i, int j, Mark&& put) {
  int ac, ar;
  plane_axes(p, ac, ar);
  const float* pt = st ? a.targets : a.sources;
  float u = lattice(pt[b * 3 + ac], a.voxel, i - a.r);
  float v = lattice(pt[b * 3 + ar], a.voxel, j - a.r);
  // th.round((p + 1) * (W - 1) / 2).type(int16): round-half-even, then wrap to int16
  int col = (int)(short)rintf((u + 1.f) * (float)(a.W - 1) / 2.f);
  int row = (int)(short)rintf((v + 1.f) * (float)(a.W - 1) / 2.f);
  // bit 0: the reference's rounded-texel sets; bit 1: texels the motion scatter can reach (the four bilinear corners of a
  // target position) -- the gather pass reads the scatter buffer only there.
  auto mark = [&](int r_, int c_, unsigned bit) {
    if (c_ < 0 || c_ >= a.W || r_ < 0 || r_ >= a.W) return;
    const long long o = ((long long)p * a.W + r_) * a.W + c_;
    put(o, bit);
  };
  mark(row, col, 1u);
  if (st) {
    const Bilin bt = bilin_setup(u, v, a.W);
    // one texel of slack around the 2x2 corners: the scatter recomputes u, v and a differently contracted
    // multiply-add must not put a corner outside the marked set
    for (int dy = -1; dy <= 2; ++dy)
      for (int dx = -1; dx <= 2; ++dx) mark(bt.y0 + dy, bt.x0 + dx, 2u);
  }
}
// Integer atomics commute, so the scattered gradient and the loss are bitwise reproducible (fp32 atomics are not).
constexpr float DRAG_FX_SCALE = 17592186044416.f;    // 2^44: |sum| < 5e5, resolution 6e-14
constexpr float DRAG_ACC_SCALE = 16777216.f;         // 2^24
int grad_to_scaled_f16_launch(const float* g, half_t* o, unsigned* bits, float* scale2, long long n, hipStream_t s);

// ---- the launches: E edits per call (include/ishap.h, ishap_drag_batch_*), each pass one launch whose grid covers all of them;
// one edit is E = 1 ----
constexpr int DRAG_MAX_EDITS = 32;
struct DragBatchArgs {
  // the shared fields (W, ld, Cc, chmap, chw, r, voxel, l1) and the BASE of every per-edit array: edit e reads edit + e*W*W*ld,
  // orig + e*orig_stride, sources / targets + 3*hoff[e], and owns slice e of touched [E][3*W*W], nmask [E], acc [E][2],
  // gfx / grad [E][W*W*ld] and loss [E]; base.B and base.cof are unused
  DragArgs base;
  int E = 0;
  long long orig_stride = 0;         // halfs between the guidance slices of consecutive edits; 0: one guidance feature for all
  int hoff[DRAG_MAX_EDITS + 1] = {};  // handle CSR offsets into sources / targets
  int tblk[DRAG_MAX_EDITS + 1] = {};  // first workgroup of each edit in the terms pass (filled by the launcher)
  float cof[DRAG_MAX_EDITS] = {};
};
// edit e's slice of a batch
__device__ __forceinline__ DragArgs drag_edit_args(const DragBatchArgs& b, int e) {
  DragArgs a = b.base;
  const long long n = (long long)a.W * a.W * a.ld;
  const int h0 = b.hoff[e];
  a.edit += e * n;
  a.orig += e * b.orig_stride;
  a.sources += 3 * h0;
  a.targets += 3 * h0;
  a.B = b.hoff[e + 1] - h0;
  a.cof = b.cof[e];
  a.touched += (long long)e * 3 * a.W * a.W;
  a.nmask += e;
  a.grad += e * n;
  a.gfx += e * n;
  a.acc += 2 * e;
  a.loss += e;
  return a;
}
int drag_batch_check(const DragBatchArgs& a);                     // the shape requirements of every drag call
int drag_batch_setup_launch(DragBatchArgs& a, hipStream_t s);     // touched bitmaps + mask counts + channel weights (once per set of edits)
// losses + fp32 gradients; with `cot` (then `bits` and `scale2` too) also the fp16 cotangent under one loss scale; `weights`:
// the region weight maps [E][3][W][W] of the mask term (edit e at + e * wstride floats), nullptr for the unweighted pass
int drag_batch_loss_launch(DragBatchArgs& a, half_t* cot, unsigned* bits, float* scale2, const float* weights, long long wstride,
                           hipStream_t s);
