// Direct triplane fitting (reference: drag_utils.py:473-550, train_triplane_opt): per Adam step
//   loss = BCEWithLogits(decoder(coord), gt) + 0.3 * mse(decoder(r), decoder(r + 0.01 * randn)) + 0.001 * l2reg + 0.01 * tvreg
// (l2reg / tvreg: axisnetworks.py:564-575), gradient on the three planes only, the MLP frozen.
//
// triplane_fit_kernel: forward AND backward of the decoder (axisnetworks.py:526-562) for the data batch and the random pairs
// in one launch on the fp32-MFMA tile scheme of decode_mlp.h (one wave owns a 32-point tile; mlp_forward / mlp_backward
// with FUSED = true).  Between a tile's forward and its backward only the two ReLU masks and the logit stay in registers.
// The backward ends in the feature cotangent as [point][channel]: register r holds, across the 32 lanes of a half, the 32
// channels of ONE point -- each bilinear tap's gradient is one global_atomic_add_f32 instruction over two 128-byte texel
// rows (cdna_hip_programming.md, Guideline 12).
// A random pair (r, r + delta) is one work item: the same lane of two tiles in the same wave, so the pair's difference and
// its cotangents +-2 * 0.3 * d / N never leave registers.  Float atomics: not bitwise repeatable (as decode_bwd.hip).
//
// triplane_reg_partials_kernel + triplane_reg_adam_kernel: sum e^2, (D_H e)^2, (D_W e)^2 per plane in double in a fixed
// order (first launch: fixed per-block partials; second launch: every block re-sums the partials in the same order), then
// the regulariser gradients 0.001 e / |e| + 0.01 D^T (D e) / |D e| are added to dplanes and torch's Adam step
// (torch/optim/adam.py, single-tensor form) is applied into a second planes buffer; dplanes is left zeroed.
// Given the same dplanes these two launches are bitwise repeatable.
#include "decode_mlp.h"

#define FIT_WAVES 4

namespace {

// what the backward of one 32-point tile keeps in registers between its forward and its backward
struct FitTile {
  unsigned long long m1, m2;     // ReLU masks (mlp_forward)
  float z;                       // logit of this lane's point
};

// point i of a tile: kind 0 = data (coords[idx[i]]), 1 = r, 2 = r + 0.01 * noise (drag_utils.py:533-534)
__device__ __forceinline__ void fit_point(const FitArgs& a, int kind, long long i, float& cx, float& cy, float& cz) {
  if (kind == 0) {
    const long long j = a.idx[i];
    cx = a.coords[j * 3]; cy = a.coords[j * 3 + 1]; cz = a.coords[j * 3 + 2];
    return;
  }
  cx = a.rcoords[i * 3]; cy = a.rcoords[i * 3 + 1]; cz = a.rcoords[i * 3 + 2];
  if (kind == 2) {      // rounded as the reference: randn * 1e-2, then the add
    cx = __fadd_rn(cx, __fmul_rn(a.rnoise[i * 3], 0.01f));
    cy = __fadd_rn(cy, __fmul_rn(a.rnoise[i * 3 + 1], 0.01f));
    cz = __fadd_rn(cz, __fmul_rn(a.rnoise[i * 3 + 2], 0.01f));
  }
}

// dz: d loss / d logit of this lane's point (0 for padding lanes).  Scatters d loss / d planes with float atomics.
__device__ __forceinline__ void fit_backward(const FitArgs& a, const MlpLds& L, const FitTile& t, float dz, int kind,
                                             long long tile0, long long n, float cx, float cy, float cz, int l31, int h) {
  f32x16 df;
  mlp_backward<true>(a.planes, a.S, L, t.m1, t.m2, dz, cx, cy, cz, h, df);
  // ---- scatter: register r = channel l31 of point kmap(r, h); one instruction = two 128-byte texel rows ----
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long i = tile0 + kmap(r, h);
    if (i < n) {
      float px, py, pz;
      fit_point(a, kind, i, px, py, pz);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        int tex[4];
        float wx[2], wy[2];
        mlp_cell(p, px, py, pz, a.S, tex, wx, wy);
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (tex[q] >= 0) atomicAdd(a.dplanes + (long long)tex[q] * 32 + l31, (wx[q & 1] * wy[q >> 1]) * df[r]);
      }
    }
  }
}

}  // namespace

__global__ __launch_bounds__(64 * FIT_WAVES) void triplane_fit_kernel(FitArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const MlpLds L = mlp_fill_lds<64 * FIT_WAVES>(a, lds, tid);
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const float b3 = a.b3[0];
  const long long npair = (a.nrand + 31) / 32, ndata = (a.nbatch + 31) / 32;
  float bce_sum = 0.f, mse_sum = 0.f;
  // the pair items (two tiles each) first, so that the lighter data items fill the tail
  for (long long item = (long long)blockIdx.x * FIT_WAVES + wave; item < npair + ndata;
       item += (long long)gridDim.x * FIT_WAVES) {
    // one code instance of the forward and of the backward (not one per tile kind: the unrolled bodies are large), looped
    // over the item's tiles: data item = one tile (kind 0); pair item = r (kind 1) and r + delta (kind 2)
    const bool pair = item < npair;
    const long long n = pair ? a.nrand : a.nbatch;
    const long long tile0 = (pair ? item : item - npair) * 32, i = tile0 + l31;
    const bool valid = i < n;
    const long long ii = valid ? i : n - 1;
    const int ntiles = pair ? 2 : 1;
    FitTile ta, tb;
#pragma nounroll
    for (int k = 0; k < ntiles; ++k) {
      float cx, cy, cz;
      fit_point(a, pair ? 1 + k : 0, ii, cx, cy, cz);
      FitTile t;
      mlp_forward<true>(a.planes, a.S, L, b3, cx, cy, cz, h, t.m1, t.m2, t.z);
      if (k == 0) ta = t; else tb = t;
    }
    float dza, dzb = 0.f;
    if (pair) {
      const float d = ta.z - tb.z;
      if (valid && h == 0) mse_sum += d * d;
      dza = valid ? 2.f * a.pair_w * d / (float)a.nrand : 0.f;
      dzb = -dza;
    } else {
      const float gt = a.gt[a.idx[ii]];
      const float z = ta.z;
      if (valid && h == 0) bce_sum += fmaxf(z, 0.f) - z * gt + log1pf(expf(-fabsf(z)));
      const float sig = 1.f / (1.f + expf(-z));
      dza = valid ? (sig - gt) / (float)a.nbatch : 0.f;
    }
#pragma nounroll
    for (int k = 0; k < ntiles; ++k) {
      float cx, cy, cz;
      fit_point(a, pair ? 1 + k : 0, ii, cx, cy, cz);
      fit_backward(a, L, k == 0 ? ta : tb, k == 0 ? dza : dzb, pair ? 1 + k : 0, tile0, n, cx, cy, cz, l31, h);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    bce_sum += __shfl_xor(bce_sum, o);
    mse_sum += __shfl_xor(mse_sum, o);
  }
  if (lane == 0) {
    if (a.nbatch > 0) atomicAdd(a.loss_parts, bce_sum / (float)a.nbatch);
    if (a.nrand > 0) atomicAdd(a.loss_parts + 1, mse_sum / (float)a.nrand);
  }
}

int triplane_fit_loss_grad_launch(const FitArgs& a, hipStream_t s) {
  ISHAP_REQUIRE(a.nbatch >= 0 && a.nrand >= 0 && a.nbatch + a.nrand > 0, "no points");
  ISHAP_REQUIRE(a.S >= 2, "triplane fit_loss_grad: plane size");
  ISHAP_TRY(ishap_set_max_lds((const void*)triplane_fit_kernel, (int)MLP_SMEM));
  const long long items = (a.nrand + 31) / 32 + (a.nbatch + 31) / 32;
  const int blocks = (int)std::min<long long>((items + FIT_WAVES - 1) / FIT_WAVES, 256);
  hipLaunchKernelGGL(triplane_fit_kernel, dim3(blocks), dim3(64 * FIT_WAVES), MLP_SMEM, s, a);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ regularisers and Adam
// ws[(p * TRIPLANE_REG_BLOCKS + b) * 3 + {0,1,2}] = block b's share of sum e^2, sum (D_H e)^2, sum (D_W e)^2 of plane p.
// D_H e = e[y+1][x] - e[y][x] (the reference's embed[:, :, 1:] - embed[:, :, :-1]), D_W along x; planes [p][y][x][c].
__global__ __launch_bounds__(256) void triplane_reg_partials_kernel(const float* __restrict__ planes, int S, double* ws,
                                                                    int* step) {
  __shared__ double red[3][256];
  const int p = blockIdx.y, b = blockIdx.x, tid = threadIdx.x;
  const long long n = (long long)S * S * 32;
  const long long chunk = (n + TRIPLANE_REG_BLOCKS - 1) / TRIPLANE_REG_BLOCKS;
  const long long i0 = b * chunk, i1 = std::min(n, i0 + chunk);
  const float* pl = planes + p * n;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long i = i0 + tid; i < i1; i += 256) {
    const float e = pl[i];
    const long long pix = i >> 5;
    const int x = (int)(pix % S), y = (int)(pix / S);
    s0 += (double)e * e;
    if (y + 1 < S) { const float d = pl[i + 32 * S] - e; s1 += (double)d * d; }
    if (x + 1 < S) { const float d = pl[i + 32] - e; s2 += (double)d * d; }
  }
  red[0][tid] = s0; red[1][tid] = s1; red[2][tid] = s2;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o)
      for (int k = 0; k < 3; ++k) red[k][tid] += red[k][tid + o];
    __syncthreads();
  }
  if (tid < 3) ws[(p * TRIPLANE_REG_BLOCKS + b) * 3 + tid] = red[tid][0];
  if (step && p == 0 && b == 0 && tid == 0) *step += 1;
}

__global__ __launch_bounds__(256) void triplane_reg_adam_kernel(RegAdamArgs a) {
  __shared__ double nrm[3][3];
  const int tid = threadIdx.x;
  if (tid < 9) {          // fixed order: every block gets the same bits
    const int p = tid / 3, k = tid % 3;
    double s = 0.0;
    for (int b = 0; b < TRIPLANE_REG_BLOCKS; ++b) s += a.ws[(p * TRIPLANE_REG_BLOCKS + b) * 3 + k];
    nrm[p][k] = sqrt(s);
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0 && a.reg_parts) {
    a.reg_parts[0] = (float)((nrm[0][0] + nrm[1][0]) + nrm[2][0]);
    a.reg_parts[1] = (float)(((nrm[0][1] + nrm[0][2]) + (nrm[1][1] + nrm[1][2])) + (nrm[2][1] + nrm[2][2]));
  }
  if (!a.planes_out) return;
  const int S = a.S;
  const long long n = (long long)S * S * 32;
  const int t = *a.step;
  const double bc1 = 1.0 - pow(a.beta1, (double)t), bc2 = 1.0 - pow(a.beta2, (double)t);
  const float step_size = (float)(a.lr / bc1), bc2_sqrt = (float)sqrt(bc2);
  const float omb1 = (float)(1.0 - a.beta1), b2 = (float)a.beta2, omb2 = (float)(1.0 - a.beta2), eps = (float)a.eps;
  for (long long i = (long long)blockIdx.x * blockDim.x + tid; i < 3 * n; i += (long long)gridDim.x * blockDim.x) {
    const int p = (int)(i / n);
    const long long j = i - p * n, pix = j >> 5;
    const int x = (int)(pix % S), y = (int)(pix / S);
    const float* pl = a.planes + p * n;
    const float e = pl[j];
    // D^T (D e) at this element: (e - e[prev]) - (e[next] - e), each term where it exists
    float gh = 0.f, gw = 0.f;
    if (y > 0) gh += e - pl[j - 32 * S];
    if (y + 1 < S) gh -= pl[j + 32 * S] - e;
    if (x > 0) gw += e - pl[j - 32];
    if (x + 1 < S) gw -= pl[j + 32] - e;
    const float i0 = nrm[p][0] > 0.0 ? (float)(1.0 / nrm[p][0]) : 0.f;
    const float i1 = nrm[p][1] > 0.0 ? (float)(1.0 / nrm[p][1]) : 0.f;
    const float i2 = nrm[p][2] > 0.0 ? (float)(1.0 / nrm[p][2]) : 0.f;
    const float g = a.dplanes[i] + a.l2_w * (e * i0) + a.tv_w * (gh * i1 + gw * i2);
    float m = a.m[i], v = a.v[i];
    m = m + omb1 * (g - m);                 // exp_avg.lerp_(grad, 1 - beta1)
    v = v * b2 + omb2 * (g * g);            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    a.m[i] = m;
    a.v[i] = v;
    a.planes_out[i] = e - step_size * (m / denom);
    a.dplanes[i] = 0.f;
  }
}

int triplane_reg_adam_launch(const RegAdamArgs& a, hipStream_t s) {
  ISHAP_REQUIRE(a.S >= 2 && a.planes && a.ws, "null argument");
  const bool adam = a.planes_out != nullptr;
  ISHAP_REQUIRE(!adam || (a.m && a.v && a.dplanes && a.step), "null Adam state");
  ISHAP_REQUIRE(adam || a.reg_parts, "nothing to write");
  ISHAP_REQUIRE(a.planes_out != a.planes, "planes_out must not alias planes");
  hipLaunchKernelGGL(triplane_reg_partials_kernel, dim3(TRIPLANE_REG_BLOCKS, 3), dim3(256), 0, s, a.planes, a.S, a.ws,
                     adam ? a.step : nullptr);
  ISHAP_CHECK_HIP(hipGetLastError());
  const long long total = 3LL * a.S * a.S * 32;
  const int blocks = adam ? (int)std::min<long long>((total + 255) / 256, 1024) : 1;
  hipLaunchKernelGGL(triplane_reg_adam_kernel, dim3(blocks), dim3(256), 0, s, a);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
