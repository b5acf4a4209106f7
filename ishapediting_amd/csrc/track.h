#pragma once
#include "drag.h"

// Handle tracking (include/ishap.h, ishap_drag_track): where did each drag handle go, in feature space.
// E edits per call with the handle CSR offsets of DragBatchArgs; the solo call is E = 1.
constexpr int TRACK_MAX_R = 8;         // search radius: candidates k in [-R, R]^3
constexpr int TRACK_MAX_RP = 4;        // patch radius: (2 rp + 1)^2 positions per plane
constexpr int TRACK_LDS_BYTES = 65536;  // the staged samples of one workgroup (two workgroups share a CU's 160 KB)
struct TrackArgs {
  const half_t* edit = nullptr;    // [E][W*W][ld] current taps, NHWC fp16
  const half_t* orig = nullptr;    // guidance taps, edit e at + e * orig_stride halfs (0: one tap for all edits)
  long long orig_stride = 0;
  int W = 0, ld = 0, Cc = 0;
  const int* chmap = nullptr;      // [3][Cc]
  const float* sources = nullptr;  // [Btot][3]
  int E = 0;
  int hoff[DRAG_MAX_EDITS + 1] = {};
  float voxel = 0.f;
  int R = 0, rp = 0;
  const int* K_in = nullptr;       // [Btot][3]
  int* K_out = nullptr;            // [Btot][3]; may be K_in
  float* dist = nullptr;           // [Btot]
  float* dist0 = nullptr;          // [Btot]
  float* volume = nullptr;         // [Btot][side^3] or nullptr
  float* partial = nullptr;        // scratch [Btot][3][nchunk][side^2]
};
// channels a workgroup stages at once: the widest of 64 / 32 / 16 whose fp32 samples fit TRACK_LDS_BYTES
int track_chunk_width(int R, int rp);
long long track_scratch_bytes(int Btot, int R, int rp, int Cc);    // -1 on arguments outside the ranges above
int track_launch(const TrackArgs& a, hipStream_t s);
