// The decoder's occupancy field differentiated in SPACE (extends MultiTriplane.forward, axisnetworks.py:537-562): the logit
// and d logit / d coordinate at arbitrary points, and a projection of points onto the zero level set along that gradient.
//
// triplane_field_kernel: coords [npts][3] -> logits [npts], grad [npts][3].  The fp32-MFMA tile scheme of
// decode_mlp.h: one wave owns 32 points; mlp_forward is MultiTriplane.forward, and mlp_backward from d logit = 1 gives the
// 32-channel feature cotangent df as [point][channel]: register r of lane (l31, h) = channel l31 of point kmap(r, h)
// (both with FUSED = false).  For plane p with axes (a, b) the bilinear slopes of that channel
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
// Contraction is off in this file, as it is inside decode_mlp.h: the two kernels inline the same evaluation, and a mul + add
// that one of them fused and the other did not would break "iterations = 0 returns triplane_field_kernel's logits bit for bit".
#include "decode_mlp.h"

#pragma clang fp contract(off)

#define FIELD_WAVES 4
#define FIELD_MAX_BLOCKS 256

namespace {

// logit z and gradient (gx, gy, gz) of this lane's point (cx, cy, cz); both lane halves return the same bits.
// Wave-collective: all 64 lanes must call it.
__device__ __forceinline__ void field_eval(const float* __restrict__ planes, int S, const MlpLds& L, float b3, float cx,
                                           float cy, float cz, int l31, int h, float& z, float& gx, float& gy, float& gz) {
  unsigned long long m1, m2;
  mlp_forward<false>(planes, S, L, b3, cx, cy, cz, h, m1, m2, z);
  f32x16 df;      // the feature cotangent of d logit = 1
  mlp_backward<false>(planes, S, L, m1, m2, 1.f, cx, cy, cz, h, df);
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
      mlp_cell(p, px, py, pz, S, tex, wx, wy);
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

// the next fp32 value from v towards `to` (v itself when they are equal); finite inputs
__device__ __forceinline__ float step_towards(float v, float to) {
  if (v == to) return v;
  if (v == 0.f) return to > 0.f ? __int_as_float(1) : __int_as_float(0x80000001);
  const int b = __float_as_int(v);
  return __int_as_float(((v < to) == (v > 0.f)) ? b + 1 : b - 1);
}

}  // namespace

__global__ __launch_bounds__(64 * FIELD_WAVES) void triplane_field_kernel(FieldArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const MlpLds L = mlp_fill_lds<64 * FIELD_WAVES>(a, lds, tid);
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
  const MlpLds L = mlp_fill_lds<64 * FIELD_WAVES>(a, lds, tid);
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
  ISHAP_TRY(ishap_set_max_lds((const void*)triplane_field_kernel, (int)MLP_SMEM));
  hipLaunchKernelGGL(triplane_field_kernel, dim3(field_blocks(a.npts)), dim3(64 * FIELD_WAVES), MLP_SMEM, s, a);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

int triplane_project_launch(const FieldArgs& a, hipStream_t s) {
  ISHAP_TRY(field_check(a));
  ISHAP_REQUIRE(a.x_out && a.normal_out && a.accepted_out, "null argument");
  ISHAP_REQUIRE(a.iterations >= 0 && a.iterations <= 64, "triplane project: iterations must be in 0..64");
  ISHAP_REQUIRE(a.step_max > 0.f && a.gmin > 0.f && a.max_move >= 0.f && a.tol >= 0.f,
                "triplane project: step_max, gmin > 0 and max_move, tol >= 0");
  ISHAP_TRY(ishap_set_max_lds((const void*)triplane_project_kernel, (int)MLP_SMEM));
  hipLaunchKernelGGL(triplane_project_kernel, dim3(field_blocks(a.npts)), dim3(64 * FIELD_WAVES), MLP_SMEM, s, a);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}
