// Volume constraints of a drag edit (csrc/constrain.hip): a weighted occupancy loss at FIXED points, differentiated onto the
// planes without float atomics.  The points do not change during an edit, so the scatter of their bilinear taps is built
// once as a gather list (constraint_setup_launch) and every step sums it in a fixed order (constraint_loss_grad_launch).
#pragma once
#include "decode.h"

#define CONSTRAINT_MAX_POINTS (1ll << 20)
#define CONSTRAINT_MAX_S 1024

struct ConstraintSetupArgs {
  const float* coords = nullptr;   // [M][3]
  long long M = 0;
  int S = 0;
  int* row_start = nullptr;        // [3 S S + 1] first entry of texel row (p S + y) S + x; the last word is the entry count
  int* entry = nullptr;            // [<= 12 M] 4 j + q (point j, tap q of mlp_cell), ascending within a row
  float* entry_w = nullptr;        // [<= 12 M] the tap's bilinear weight wx[q & 1] * wy[q >> 1]
  void* scratch = nullptr;
  long long scratch_bytes = 0;
};
long long constraint_setup_scratch_bytes(long long M, int S);
int constraint_setup_launch(const ConstraintSetupArgs& a, hipStream_t s);

struct ConstraintArgs {
  const float* planes = nullptr;   // [3][S][S][32] un-normalised, channels-last
  int S = 0;
  const float *B = nullptr, *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
  const float* coords = nullptr;   // [npts][3]
  const float* gt = nullptr;       // [npts] targets in {0, 1}
  const float* pw = nullptr;       // [npts] weights >= 0
  long long npts = 0;
  float wsum = 0.f;                // sum of the weights (> 0), summed in double by the caller
  const int* row_start = nullptr;  // the gather list of constraint_setup_launch for these coords and this S
  const int* entry = nullptr;
  const float* entry_w = nullptr;
  float* dfeat = nullptr;          // [npts][32] scratch: the feature cotangent of every point
  float* partials = nullptr;       // [ceil(npts / 32)] scratch: sum of w * bce over each tile
  float* dplanes = nullptr;        // [3][S][S][32] d L / d planes, every texel written
  float* loss = nullptr;           // [1] L = -(1 / wsum) sum w * BCEWithLogits
  float* logits = nullptr;         // optional [npts]
};
int constraint_loss_grad_launch(const ConstraintArgs& a, hipStream_t s);
