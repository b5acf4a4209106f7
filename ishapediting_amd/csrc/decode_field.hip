// The decoder's occupancy field differentiated in SPACE (extends MultiTriplane.forward, axisnetworks.py:537-562): the logit
// and d logit / d coordinate at arbitrary points, and a projection of points onto the zero level set along that gradient.
//
// triplane_field_kernel: coords [npts][3] -> logits [npts], grad [npts][3].  The tile scheme of decode_fit.hip: one wave owns
// 32 points (lane & 31 = point, lane >> 5 = K slot), fp32 copies of W1, W2 and _B in LDS, every matrix product on the
// exact-fp32 matrix cores (v_mfma_f32_32x32x2_f32).  The forward is MultiTriplane.forward; the backward starts from
// d logit = 1, goes through the two ReLU layers (masks h > 0 kept as 64-bit words), the sin / cos features (phases
// recomputed) and _B to the 32-channel feature cotangent df.  The last product swaps its operands so that the accumulator is
// [point][channel]: register r of lane (l31, h) = channel l31 of point kmap(r, h).  For plane p with axes (a, b) the bilinear
// slopes of that channel
//   sx = (t_ne - t_nw) wy0 + (t_se - t_sw) wy1,   sy = (t_sw - t_nw) wx0 + (t_se - t_ne) wx1     (out-of-range texels read 0)
// are formed lane-locally (one 128-byte texel row per tap and half wave), multiplied by df and summed over the 32 channels
// by a fixed xor butterfly;  grad[a] = (S - 1) / 2 * sum_c df[c] (sx of the two planes that sample a), likewise grad[b].
// On a cell boundary floor() decides the cell, so the gradient is the RIGHT-SIDED derivative there.  No atomics: the
// outputs are bitwise repeatable.  A padding lane of a tail tile evaluates a stand-in point (the last one) and stores nothing.
//
// triplane_project_kernel: the same evaluation 1 + iterations times per tile (wave-collective, so every lane runs every
// evaluation and the updates are lane-masked).  Per point: x = x0, (z, g) = field(x), scale = 1; then `iterations` times: a
// lane with |z| <= tol or |g|^2 < gmin no longer updates; the others try d = -scale z g / max(|g|^2, gmin), |d| clipped to
// step_max, x + d clipped into the ball of radius max_move around x0; the trial is taken (x, z, g, scale = 1) when it lowers
// |z|, otherwise scale halves.  |z_out| <= |z_start| holds exactly.  The ball is enforced on the ROUNDED fp32 position: the clip
// aims 8 u inside the radius, the position is then stepped an ulp at a time towards x0 while the fp32 sum of squares of
// x - x0 exceeds the fp32 max_move^2, and a trial that is still outside after four steps is dropped.  Every position taken
// therefore passes that fp32 test, whose own roundings (the three differences, squares and sums, and max_move^2) leave
// |x_out - x0| <= max_move (1 + 4 u) in exact arithmetic -- that, not the bare max_move, is what the kernel guarantees.
// Outputs x, z, the unit normal -g / |g| (the direction of decreasing logit: logits are positive inside, so it points
// OUTWARD; exactly 0 where |g|^2 < gmin) and the count of accepted steps.  iterations = 0: logit and normal at the points.
//
// Contraction is off in this file: the two kernels inline the same evaluation, and a mul + add that one of them fused and the
// other did not would break "iterations = 0 returns triplane_field_kernel's logits bit for bit".
#include "decode.h"

#pragma clang fp contract(off)

#define FLD 132   // row stride (floats) of W1 / W2 in LDS: 528 B = 16 B mod 256 -> conflict-free ds_read_b128 (decode_fit.hip)
#define BLD 68    // row stride (floats) of _B [32][64] in LDS
#define FIELD_WAVES 4
#define FIELD_MAX_BLOCKS 256

namespace {

// this lane's base pointers into the LDS images: every read is base + a compile-time offset (decode_fit.hip, FitLds)
struct FieldLds {
  const float *W1r, *W2r;   // row reads W[32qo + l31][k + 4h]
  const float *W1c, *W2c;   // column reads W[k + 4h][32qo + l31]
  const float *Bf, *Bb;     // _B[c + 4h][32q + l31] and _B[l31][k + 4h]
  const float *b1, *b2, *w3;   // + 4h
};

// bilinear cell of plane p (xy, yz, xz; align_corners, zero padding): the four texel indices (nw ne sw se, -1 = out of
// range) and the axis weights.  The same arithmetic as decode_fit.hip's fit_taps.
__device__ __forceinline__ void field_cell(int p, float cx, float cy, float cz, int S, int (&tex)[4], float (&wx)[2],
                                           float (&wy)[2]) {
  const float u = (p == 1) ? cy : cx;
  const float v = (p == 0) ? cy : cz;
  const float ix = ((u + 1.f) / 2.f) * (float)(S - 1);
  const float iy = ((v + 1.f) / 2.f) * (float)(S - 1);
  const float fx = floorf(ix), fy = floorf(iy);
  // a coordinate beyond +-2^30 texels has no tap in range either way: keep the conversion defined
  const int x0 = (int)fminf(fmaxf(fx, -2.f), 1073741824.f), y0 = (int)fminf(fmaxf(fy, -2.f), 1073741824.f);
  wx[1] = ix - fx; wx[0] = (fx + 1.f) - ix;
  wy[1] = iy - fy; wy[0] = (fy + 1.f) - iy;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int xx = x0 + (q & 1), yy = y0 + (q >> 1);
    tex[q] = (xx >= 0 && xx < S && yy >= 0 && yy < S) ? (p * S + yy) * S + xx : -1;
  }
}

// features (three bilinear samples, summed) and phases y = f @ _B of this lane's point: y[q][r] = phase 32q + kmap(r, h)
__device__ __forceinline__ void field_phases(const float* __restrict__ planes, int S, const FieldLds& L, float cx, float cy,
                                             float cz, int h, f32x16 (&y)[2]) {
  f32x4 f[4];       // this lane's 16 channels {8g + 4h + e}
#pragma unroll
  for (int g = 0; g < 4; ++g) f[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    int tex[4];
    float wx[2], wy[2];
    field_cell(p, cx, cy, cz, S, tex, wx, wy);
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (tex[q] >= 0) {
        const float w = wx[q & 1] * wy[q >> 1];
        const float* tp = planes + (long long)tex[q] * 32 + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] += w * *reinterpret_cast<const f32x4*>(tp + 8 * g);
      }
#pragma unroll
    for (int g = 0; g < 4; ++g) f[g] += acc[g];
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int r = 0; r < 16; ++r) y[q][r] = 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        y[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(L.Bf[(8 * g + e) * BLD + 32 * q], f[g][e], y[q], 0, 0, 0);
  }
}

// logit z and gradient (gx, gy, gz) of this lane's point (cx, cy, cz); both lane halves return the same bits.
// Wave-collective: all 64 lanes must call it.
__device__ __forceinline__ void field_eval(const float* __restrict__ planes, int S, const FieldLds& L, float b3, float cx,
                                           float cy, float cz, int l31, int h, float& z, float& gx, float& gy, float& gz) {
  const float two_pi = 6.2831855f;      // float32(2*np.pi), axisnetworks.py:89
  unsigned long long m1 = 0ull, m2 = 0ull;      // ReLU masks: bit 16q + r = neuron 32q + kmap(r, h)
  {
    f32x16 y[2];
    field_phases(planes, S, L, cx, cy, cz, h, y);
    f32x16 x1[4];       // Fourier features: blocks 0,1 = sin, 2,3 = cos
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float s, c;
        sincos_cw(two_pi * y[q][r], s, c);
        x1[q][r] = s;
        x1[2 + q][r] = c;
      }
    // ---- layer 1 ----
    f32x16 x2[4];
#pragma unroll
    for (int qo = 0; qo < 4; ++qo) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(L.W1r + 32 * qo * FLD + 32 * q + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[e], x1[q][4 * g + e], acc, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);      // keep the weight reads next to their MFMAs (hoisted, they spill)
        }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[r] + L.b1[32 * qo + kmap(r, 0)];
        if (v > 0.f) m1 |= 1ull << (16 * qo + r);
        x2[qo][r] = fmaxf(v, 0.f);
      }
    }
    // ---- layer 2 and the output layer ----
    float partial = 0.f;
#pragma unroll
    for (int qo = 0; qo < 4; ++qo) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(L.W2r + 32 * qo * FLD + 32 * q + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[e], x2[q][4 * g + e], acc, 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int n = 32 * qo + kmap(r, 0);
        const float v = acc[r] + L.b2[n];
        if (v > 0.f) {
          m2 |= 1ull << (16 * qo + r);
          partial = fmaf(L.w3[n], v, partial);
        }
      }
    }
    z = (partial + __shfl_xor(partial, 32)) + b3;
  }
  // ---- d h1 = W2^T (w3 * relu'(h2)), masked by relu'(h1) ----
  f32x16 g1[4];
#pragma unroll
  for (int qo = 0; qo < 4; ++qo) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 w3v = *reinterpret_cast<const f32x4*>(L.w3 + 32 * q + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * g + e;
          const float bv = ((m2 >> (16 * q + r)) & 1ull) ? w3v[e] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(L.W2c[(32 * q + kmap(r, 0)) * FLD + 32 * qo], bv, acc, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) g1[qo][r] = ((m1 >> (16 * qo + r)) & 1ull) ? acc[r] : 0.f;
  }
  // ---- d Fourier features = W1^T g1 ----
  f32x16 dff[4];
#pragma unroll
  for (int qo = 0; qo < 4; ++qo) {
#pragma unroll
    for (int r = 0; r < 16; ++r) dff[qo][r] = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          dff[qo] = __builtin_amdgcn_mfma_f32_32x32x2f32(L.W1c[(32 * q + 8 * g + e) * FLD + 32 * qo], g1[q][4 * g + e],
                                                         dff[qo], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      }
  }
  // ---- d phases: 2 pi (d sin * cos - d cos * sin), the phases recomputed ----
  f32x16 y[2], dy[2];
  field_phases(planes, S, L, cx, cy, cz, h, y);
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float s, c;
      sincos_cw(two_pi * y[q][r], s, c);
      dy[q][r] = two_pi * (dff[q][r] * c - dff[2 + q][r] * s);
    }
  // ---- d features^T [point][channel] = dy^T _B^T: A = dy (point rows), B = _B rows (channel columns) ----
  f32x16 df;
#pragma unroll
  for (int r = 0; r < 16; ++r) df[r] = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 bv = *reinterpret_cast<const f32x4*>(L.Bb + 32 * q + 8 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) df = __builtin_amdgcn_mfma_f32_32x32x2f32(dy[q][4 * g + e], bv[e], df, 0, 0, 0);
    }
  // ---- slopes: register r = channel l31 of point kmap(r, h) (lane kmap(r, h) of half 0 holds its coordinates) ----
  const float half_sm1 = 0.5f * (float)(S - 1);
  const int ro = (l31 & 3) + 4 * (l31 >> 3), ho = (l31 >> 2) & 1;     // this lane's own point: register ro of half ho
  gx = gy = gz = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int src = kmap(r, h);
    const float px = __shfl(cx, src), py = __shfl(cy, src), pz = __shfl(cz, src);
    float a[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      int tex[4];
      float wx[2], wy[2], t[4];
      field_cell(p, px, py, pz, S, tex, wx, wy);
#pragma unroll
      for (int q = 0; q < 4; ++q) t[q] = tex[q] >= 0 ? planes[(long long)tex[q] * 32 + l31] : 0.f;
      const float sx = (t[1] - t[0]) * wy[0] + (t[3] - t[2]) * wy[1];
      const float sy = (t[2] - t[0]) * wx[0] + (t[3] - t[1]) * wx[1];
      a[p == 1 ? 1 : 0] += df[r] * sx;      // u axis: x, y, x
      a[p == 0 ? 1 : 2] += df[r] * sy;      // v axis: y, z, z
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) a[k] += __shfl_xor(a[k], o);     // over the 32 channels of this half
      a[k] *= half_sm1;
    }
    if (r == ro) { gx = a[0]; gy = a[1]; gz = a[2]; }
  }
  const float ox = __shfl_xor(gx, 32), oy = __shfl_xor(gy, 32), oz = __shfl_xor(gz, 32);
  if (h != ho) { gx = ox; gy = oy; gz = oz; }
}

__device__ __forceinline__ FieldLds field_fill_lds(const FieldArgs& a, float* lds, int tid) {
  float* sW1 = lds;                       // [128][FLD] W1[out][in]
  float* sW2 = sW1 + 128 * FLD;
  float* sB = sW2 + 128 * FLD;            // [32][BLD]  _B[channel][phase]
  float* sb1 = sB + 32 * BLD;
  float* sb2 = sb1 + 128;
  float* sw3 = sb2 + 128;
  for (int i = tid; i < 128 * 128; i += 64 * FIELD_WAVES) {
    const int r = i >> 7, k = i & 127;
    sW1[r * FLD + k] = a.W1[i];
    sW2[r * FLD + k] = a.W2[i];
  }
  for (int i = tid; i < 32 * 64; i += 64 * FIELD_WAVES) sB[(i >> 6) * BLD + (i & 63)] = a.B[i];
  if (tid < 128) { sb1[tid] = a.b1[tid]; sb2[tid] = a.b2[tid]; sw3[tid] = a.w3[tid]; }
  __syncthreads();
  const int l31 = tid & 31, h = (tid >> 5) & 1;
  return FieldLds{sW1 + l31 * FLD + 4 * h, sW2 + l31 * FLD + 4 * h, sW1 + 4 * h * FLD + l31, sW2 + 4 * h * FLD + l31,
                  sB + 4 * h * BLD + l31, sB + l31 * BLD + 4 * h, sb1 + 4 * h, sb2 + 4 * h, sw3 + 4 * h};
}

// the next fp32 value from v towards `to` (v itself when they are equal); finite inputs
__device__ __forceinline__ float step_towards(float v, float to) {
  if (v == to) return v;
  if (v == 0.f) return to > 0.f ? __int_as_float(1) : __int_as_float(0x80000001);
  const int b = __float_as_int(v);
  return __int_as_float(((v < to) == (v > 0.f)) ? b + 1 : b - 1);
}

}  // namespace

#define FIELD_SMEM ((size_t)(2 * 128 * FLD + 32 * BLD + 3 * 128) * sizeof(float))

__global__ __launch_bounds__(64 * FIELD_WAVES) void triplane_field_kernel(FieldArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const FieldLds L = field_fill_lds(a, lds, tid);
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const float b3 = a.b3[0];
  const long long ntiles = (a.npts + 31) / 32;
  for (long long tile = (long long)blockIdx.x * FIELD_WAVES + wave; tile < ntiles; tile += (long long)gridDim.x * FIELD_WAVES) {
    const long long i = tile * 32 + l31;
    const bool valid = i < a.npts;
    const long long ii = valid ? i : a.npts - 1;
    const float cx = a.coords[ii * 3], cy = a.coords[ii * 3 + 1], cz = a.coords[ii * 3 + 2];
    float z, gx, gy, gz;
    field_eval(a.planes, a.S, L, b3, cx, cy, cz, l31, h, z, gx, gy, gz);
    if (valid && h == 0) {
      a.logits[i] = z;
      a.grad[i * 3] = gx; a.grad[i * 3 + 1] = gy; a.grad[i * 3 + 2] = gz;
    }
  }
}

__global__ __launch_bounds__(64 * FIELD_WAVES) void triplane_project_kernel(FieldArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const FieldLds L = field_fill_lds(a, lds, tid);
  const int lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const float b3 = a.b3[0];
  const float r_clip = a.max_move * (1.f - 4.76837158203125e-7f);      // 8 u inside the ball
  const float mm2 = a.max_move * a.max_move;
  const long long ntiles = (a.npts + 31) / 32;
  for (long long tile = (long long)blockIdx.x * FIELD_WAVES + wave; tile < ntiles; tile += (long long)gridDim.x * FIELD_WAVES) {
    const long long i = tile * 32 + l31;
    const bool valid = i < a.npts;
    const long long ii = valid ? i : a.npts - 1;
    const float x0 = a.coords[ii * 3], y0 = a.coords[ii * 3 + 1], z0 = a.coords[ii * 3 + 2];
    float x = x0, y = y0, zc = z0;                 // the point; v = its logit, (gx, gy, gz) its gradient
    float v = 0.f, gx = 0.f, gy = 0.f, gz = 0.f, g2 = 0.f, scale = 1.f;
    int accepted = 0;
    // one code instance of the evaluation: pass 0 evaluates x0 itself and is always taken
#pragma nounroll
    for (int it = 0; it <= a.iterations; ++it) {
      float tx = x, ty = y, tz = zc;
      const bool active = it > 0 && !(fabsf(v) <= a.tol) && !(g2 < a.gmin);
      if (active) {
        const float s = -scale * v / fmaxf(g2, a.gmin);
        float dx = s * gx, dy = s * gy, dz = s * gz;
        const float dn = sqrtf(dx * dx + dy * dy + dz * dz);
        if (dn > a.step_max) { const float k = a.step_max / dn; dx *= k; dy *= k; dz *= k; }
        tx = x + dx; ty = y + dy; tz = zc + dz;
        float ex = tx - x0, ey = ty - y0, ez = tz - z0;
        const float en = sqrtf(ex * ex + ey * ey + ez * ez);
        if (en > r_clip) {
          const float k = r_clip / en;
          tx = x0 + ex * k; ty = y0 + ey * k; tz = z0 + ez * k;
        }
        // the ROUNDED position: one ulp towards x0 while it measures outside the ball (the clip leaves it within a rounding
        // of the radius, so one step is the rule); a position that four steps do not bring inside is given up for the
        // current point, which is inside by induction and as a trial changes nothing
        bool outside = true;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
          ex = tx - x0; ey = ty - y0; ez = tz - z0;
          outside = ex * ex + ey * ey + ez * ez > mm2;
          if (outside && k < 4) { tx = step_towards(tx, x0); ty = step_towards(ty, y0); tz = step_towards(tz, z0); }
        }
        if (outside) { tx = x; ty = y; tz = zc; }
      }
      float tv, tgx, tgy, tgz;
      field_eval(a.planes, a.S, L, b3, tx, ty, tz, l31, h, tv, tgx, tgy, tgz);
      if (it == 0 || (active && fabsf(tv) < fabsf(v))) {
        x = tx; y = ty; zc = tz; v = tv; gx = tgx; gy = tgy; gz = tgz;
        g2 = gx * gx + gy * gy + gz * gz;
        scale = 1.f;
        accepted += it > 0;
      } else if (active) {
        scale *= 0.5f;
      }
    }
    if (valid && h == 0) {
      a.x_out[i * 3] = x; a.x_out[i * 3 + 1] = y; a.x_out[i * 3 + 2] = zc;
      a.logits[i] = v;
      float nx = 0.f, ny = 0.f, nz = 0.f;
      if (!(g2 < a.gmin)) {      // normalised in double: one rounding per component
        const double n = sqrt((double)gx * gx + (double)gy * gy + (double)gz * gz);
        if (n > 0.0) { nx = (float)(-(double)gx / n); ny = (float)(-(double)gy / n); nz = (float)(-(double)gz / n); }
      }
      a.normal_out[i * 3] = nx; a.normal_out[i * 3 + 1] = ny; a.normal_out[i * 3 + 2] = nz;
      a.accepted_out[i] = accepted;
    }
  }
}

static int field_check(const FieldArgs& a) {
  ISHAP_REQUIRE(a.S >= 2, "triplane field: plane size");
  ISHAP_REQUIRE(a.npts >= 1, "triplane field: no points");
  ISHAP_REQUIRE(a.planes && a.coords && a.logits, "null argument");
  return 0;
}

static int field_blocks(long long npts) {
  const long long tiles = (npts + 31) / 32;
  return (int)std::min<long long>((tiles + FIELD_WAVES - 1) / FIELD_WAVES, FIELD_MAX_BLOCKS);
}

int triplane_field_grad_launch(const FieldArgs& a, hipStream_t s) {
  ISHAP_TRY(field_check(a));
  ISHAP_REQUIRE(a.grad, "null argument");
  ISHAP_TRY(ishap_set_max_lds((const void*)triplane_field_kernel, (int)FIELD_SMEM));
  hipLaunchKernelGGL(triplane_field_kernel, dim3(field_blocks(a.npts)), dim3(64 * FIELD_WAVES), FIELD_SMEM, s, a);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

int triplane_project_launch(const FieldArgs& a, hipStream_t s) {
  ISHAP_TRY(field_check(a));
  ISHAP_REQUIRE(a.x_out && a.normal_out && a.accepted_out, "null argument");
  ISHAP_REQUIRE(a.iterations >= 0 && a.iterations <= 64, "triplane project: iterations must be in 0..64");
  ISHAP_REQUIRE(a.step_max > 0.f && a.gmin > 0.f && a.max_move >= 0.f && a.tol >= 0.f,
                "triplane project: step_max, gmin > 0 and max_move, tol >= 0");
  ISHAP_TRY(ishap_set_max_lds((const void*)triplane_project_kernel, (int)FIELD_SMEM));
  hipLaunchKernelGGL(triplane_project_kernel, dim3(field_blocks(a.npts)), dim3(64 * FIELD_WAVES), FIELD_SMEM, s, a);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
