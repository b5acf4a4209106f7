#pragma once
#include "common.h"
#include <algorithm>

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
// Integer atomics commute, so the scattered gradient and the loss are bitwise reproducible (fp32 atomics are not).
constexpr float DRAG_FX_SCALE = 17592186044416.f;    // 2^44: |sum| < 5e5, resolution 6e-14
constexpr float DRAG_ACC_SCALE = 16777216.f;         // 2^24
int grad_to_scaled_f16_launch(const float* g, half_t* o, unsigned* bits, float* scale2, long long n, hipStream_t s);

// ---- the launches: E edits per call (include/ishap.h, ishap_drag_batch_*), each pass one launch whose grid covers all of them;
// the solo ABI (ishap_drag_setup / _loss_grad / _loss_cotangent) is E = 1 with `base` pointing at the caller's own buffers ----
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
int drag_batch_setup_launch(DragBatchArgs& a, hipStream_t s);     // touched bitmaps + mask counts + channel weights (once per set of edits)
// losses + fp32 gradients; with `cot` (then `bits` and `scale2` too) also the fp16 cotangent under one loss scale; `weights`:
// the region weight maps [E][3][W][W] of the mask term (edit e at + e * wstride floats), nullptr for the unweighted pass
int drag_batch_loss_launch(DragBatchArgs& a, half_t* cot, unsigned* bits, float* scale2, const float* weights, long long wstride,
                           hipStream_t s);
