#pragma once
#include "drag.h"

// Closed-loop drag (include/ishap.h, ishap_drag_batch_retarget): per tracked step, re-aim every handle's goal from
// its tracked offset and rebuild what the loss derives from its targets (touched bitmaps, mask counts), one launch for E edits.
constexpr int RETARGET_THREADS = 1024;
constexpr int RETARGET_LDS_BYTES = 65536;   // the three plane bitmaps of one edit, 3*W*W bytes, must fit
struct RetargetArgs {
  const float* final_targets = nullptr;   // [Btot][3]: where each handle is to end
  const int* K = nullptr;                 // [Btot][3]: tracked integer voxel offsets from the sources
  float* goals = nullptr;                 // [Btot][3]: written; the buffer the loss kernels read as `targets`
  float* remaining = nullptr;             // [Btot]
  int* arrived = nullptr;                 // [Btot]
  int* done = nullptr;                    // [E]
  float step[DRAG_MAX_EDITS] = {};        // the lead of each edit in voxels, > 0, may be +inf
  float arrive[DRAG_MAX_EDITS] = {};      // >= 0
};
// `a`: as for drag_batch_setup_launch (a.base.targets is ignored: the goals are q.goals); every check precedes the launch
int drag_retarget_launch(DragBatchArgs& a, const RetargetArgs& q, hipStream_t s);
