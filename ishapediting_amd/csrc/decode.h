#pragma once
#include "common.h"
#include <algorithm>

// accumulator register s of lane-half h of a 32x32 MFMA tile holds row kmap(s, h) (cdna_hip_programming.md, C/D layout)
__device__ __forceinline__ int kmap(int s, int h) { return (s & 3) + 8 * (s >> 2) + 4 * h; }

// sin/cos of an fp32 angle: 3-term Cody-Waite reduction by pi/2 (exact for |x| < ~1e4, far above the Fourier
// phases seen here) + the classic single-precision minimax polynomials on [-pi/4, pi/4]; ~1e-7 absolute.
// (ocml's sincosf inlines its huge-argument path 64 times per tile and blows the register budget.)
__device__ __forceinline__ void sincos_cw(float x, float& s, float& c) {
  const float k = rintf(x * 0.63661977236758134f);
  float r = fmaf(-k, 1.5703125f, x);
  r = fmaf(-k, 4.837512969970703125e-4f, r);
  r = fmaf(-k, 7.54978995489188e-8f, r);
  const float z = r * r;
  const float sp = fmaf(r * z, fmaf(z, fmaf(z, -1.9515295891e-4f, 8.3321608736e-3f), -1.6666654611e-1f), r);
  const float cp = fmaf(z * z, fmaf(z, fmaf(z, 2.443315711809948e-5f, -1.388731625493765e-3f), 4.166664568298827e-2f),
                        fmaf(z, -0.5f, 1.f));
  const int q = (int)k & 3;
  const float s1 = (q & 1) ? cp : sp;
  const float c1 = (q & 1) ? sp : cp;
  s = (q & 2) ? -s1 : s1;
  c = ((q + 1) & 2) ? -c1 : c1;
}

struct DecodeArgs {
  const float* planes = nullptr;   // [3][S][S][32] un-normalised, channels-last
  int S = 0;
  const float* B = nullptr;        // net.0._B [32][64]
  const float* W1 = nullptr;       // net.1.weight [128][128]
  const float* b1 = nullptr;
  const float* W2 = nullptr;       // net.3.weight
  const float* b2 = nullptr;
  const float* w3 = nullptr;       // net.5.weight [1][128]
  const float* b3 = nullptr;       // [1]
  const float* coords = nullptr;   // [npts][3] or null for the dense grid
  const float* lin = nullptr;      // grid axis values [res]
  int res = 0;
  long long npts = 0;
  float* out = nullptr;            // [npts] logits
};
int triplane_decode_launch(const DecodeArgs& a, hipStream_t s);
// the 9^3 sample nodes of `nbricks` bricks of the fine grid a.lin [a.res] (brick ids (bx nb + by) nb + bz, nb = ceil((res - 1) / 8))
// into a.out [nbricks][9][9][9]; a.npts = 729 nbricks, a.coords unused
int triplane_decode_bricks_launch(const DecodeArgs& a, const int* bricks, long long nbricks, hipStream_t s);

struct DecBwdArgs {
  const float* planes = nullptr;   // [3][S][S][32]
  int S = 0;
  const float *B = nullptr, *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
  const float *W1T = nullptr, *W2T = nullptr;   // transposed copies (coalesced forward mat-vecs)
  const float* coords = nullptr;   // [npts][3]
  const float* gt = nullptr;       // [npts] occupancy targets
  long long npts = 0;
  float* dplanes = nullptr;        // [3][S][S][32] d(-BCE)/d planes (zeroed by the launch)
  float* loss = nullptr;           // [1] = -BCEWithLogits mean
  float* logits = nullptr;         // optional [npts]
};
int decode_points_bwd_launch(const DecBwdArgs& a, hipStream_t s);
int x0_grad_launch(const float* dplanes, const float* rng, const float* x, const float* model_out, float sr, float srm1,
                   int clip, int S, float* g_direct, float* cot_out, hipStream_t s);
int planes_prepare_launch(const float* latent, const float* rng, const float* mid, float* planes, int S, hipStream_t s);

// Direct triplane fitting (reference: drag_utils.py:473-550, train_triplane_opt), csrc/decode_fit.hip.
struct FitArgs {
  const float* planes = nullptr;   // [3][S][S][32] un-normalised, channels-last
  int S = 0;
  const float *B = nullptr, *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
  const float* coords = nullptr;   // [P][3] occupancy samples
  const float* gt = nullptr;       // [P]
  const int* idx = nullptr;        // [nbatch] this step's batch: coords[idx[i]], gt[idx[i]]
  long long nbatch = 0;
  const float* rcoords = nullptr;  // [nrand][3] r = rand*2-1
  const float* rnoise = nullptr;   // [nrand][3] randn; the pair partner is r + 0.01 * noise
  long long nrand = 0;
  float pair_w = 0.f;              // weight of the pair mse (0.3)
  float* dplanes = nullptr;        // [3][S][S][32] += d(BCE + pair_w * mse)/d planes
  float* loss_parts = nullptr;     // [2] += {BCE mean, mse}
};
int triplane_fit_loss_grad_launch(const FitArgs& a, hipStream_t s);

#define TRIPLANE_REG_BLOCKS 64     // partial-sum blocks per plane of the regulariser reduction
struct RegAdamArgs {
  const float* planes = nullptr;   // [3][S][S][32] this step's planes
  int S = 0;
  double* ws = nullptr;            // [3][TRIPLANE_REG_BLOCKS][3] partial sums
  float* reg_parts = nullptr;      // [2] = {l2reg, tvreg} of `planes` (may be null when stepping)
  // Adam (all null: the regulariser values alone)
  float* planes_out = nullptr;     // the stepped planes (must not alias `planes`)
  float *m = nullptr, *v = nullptr;
  float* dplanes = nullptr;        // read, then zeroed
  int* step = nullptr;             // device step counter, incremented by the launch
  double lr = 0.0, beta1 = 0.0, beta2 = 0.0, eps = 0.0;   // double as torch's Python scalars (1 - 0.999f is not 0.001f)
  float l2_w = 0.f, tv_w = 0.f;
};
int triplane_reg_adam_launch(const RegAdamArgs& a, hipStream_t s);

// The decoder's field in space (extends axisnetworks.py:537-562), csrc/decode_field.hip: logit and d logit / d coordinate at
// points, and the projection of points onto the zero level set.
struct FieldArgs {
  const float* planes = nullptr;   // [3][S][S][32] un-normalised, channels-last
  int S = 0;
  const float *B = nullptr, *W1 = nullptr, *b1 = nullptr, *W2 = nullptr, *b2 = nullptr, *w3 = nullptr, *b3 = nullptr;
  const float* coords = nullptr;   // [npts][3]
  long long npts = 0;
  float* logits = nullptr;         // [npts] (project: the logit at x_out)
  float* grad = nullptr;           // [npts][3] d logit / d coordinate (field_grad only)
  // projection only
  int iterations = 0;
  float step_max = 0.f, max_move = 0.f, tol = 0.f, gmin = 0.f;
  float* x_out = nullptr;          // [npts][3]
  float* normal_out = nullptr;     // [npts][3] -g / |g| (outward), 0 where |g|^2 < gmin
  int* accepted_out = nullptr;     // [npts] accepted steps
};
int triplane_field_grad_launch(const FieldArgs& a, hipStream_t s);
int triplane_project_launch(const FieldArgs& a, hipStream_t s);
