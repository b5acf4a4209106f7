// Persistent-kernel prototype for the 8x8 level ("measure, not cite").
// HISTORICAL (rounds 3-5): form (A) launches csrc/igemm_small3.hip, which round 6 removed from the library together with the other
// measured-loser kernel families -- this file builds against the round-5 tree (git show 3dbab91:ishapediting_amd/csrc/igemm_small3.hip);
// its results are in profiles/round3_persistent_chain.txt and the GN_STAMP table in DESIGN.md.
//
// Chain of L layers on a 64-pixel x 1024-channel map at batch 1, each layer = what half a ResBlock of the middle block
// does (guided_diffusion/unet.py:236-256):   x_l = x_{l-1} + conv3x3( SiLU( GroupNorm32(x_{l-1}) ) ) + bias
// measured two ways on the same data:
//   (A) the product's launches: gn_local_launch (adds up the previous conv's pending K slices) + igemm_small3_launch with
//       4 K slices left pending -- 2 launches per layer, exactly what unet.hip enqueues on these maps;
//   (B) ONE persistent launch of 256 workgroups (one per CU, 512 threads) that walks all L layers.  Workgroup =
//       (16 output channels, one of 4 K slices of 256 input channels).  Per layer: wait for the previous layer's
//       activation -> load its own 64 x 256 slice (sc1 loads), GroupNorm statistics of its 8 groups in registers, normalise
//       + SiLU into a zero-haloed LDS tile -> 288 MFMAs against weights that were DMA'd into LDS while it waited ->
//       fp32 partial tile to global (sc1) + arrival count -> each of the 4 slice-workgroups adds up a quarter of the rows,
//       bias, residual, fp16 (sc1) + arrival count for the next layer.  Cross-workgroup hand-offs follow
//       cdna_hip_programming.md Guideline 16 (sc1 payload, every storing wave drains, one lane signals, relaxed sc1 polls,
//       bounded spins that raise an error word).
// Output: per-layer time of both forms and the relative difference of the final activations.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -w tools/experiments/persist_chain.hip -o build/persist_chain && ./build/persist_chain [L]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../ishapediting_amd/csrc/igemm_small3.hip"
#include "../ishapediting_amd/csrc/norm_local.hip"
#include "experiments/conv8.hip"

hipEvent_t g_igemm_prof_start = nullptr, g_igemm_prof_stop = nullptr;
#ifdef C8_STAMPS
__device__ unsigned long long* g_c8_stamps;
#endif
#ifdef ISHAP_STAMPS
__device__ unsigned long long* g_gn_stamps;
#endif
void ishap_set_error(const std::string& m) { fprintf(stderr, "ERR %s\n", m.c_str()); }
static unsigned* g_status_host = nullptr;
unsigned* ishap_status_word() {
  if (!g_status_host) { hipHostMalloc((void**)&g_status_host, 64, hipHostMallocMapped); *g_status_host = 0; }
  return g_status_host;
}
int ishap_check_status() { return 0; }
int ishap_cu_count() { return 256; }

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

namespace pc {
constexpr int C = 1024, HWP = 64, NT = 16, KS = 4, KSL = C / KS;        // 16 couts per workgroup, 4 K slices of 256 channels
constexpr int NTILES = C / NT;                                           // 64
constexpr int WGS = NTILES * KS;                                         // 256
constexpr int T = 512;
constexpr int W_BYTES = NT * 9 * KSL * 2;                                // 73 728: one (ntile, kslice) weight block
constexpr int XP = 100;                                                  // padded 10 x 10 pixels
constexpr int X_BYTES = XP * KSL * 2;                                    // 51 200
constexpr int RED_BYTES = 8 * 4 * 64 * 16;                               // 32 768
constexpr int LDS_BYTES = W_BYTES + X_BYTES + RED_BYTES + 1024;
constexpr int SPIN_LIMIT = 1 << 18;

struct Args {
  const half_t* W;        // [L][NTILES][KS][9 taps][8 ksteps][64 lanes][8 halfs]  (fragment order: a k-step is one linear KiB)
  const float* gamma;     // [L][C]
  const float* beta;      // [L][C]
  const float* bias;      // [L][C]
  half_t* X;              // [L + 1][64][C]  activations, X[0] = input
  float* part;            // [L][NTILES][KS][64][16] fp32 partial tiles
  unsigned* cnt_part;     // [L][NTILES]   arrivals of partial tiles (4 each)
  unsigned* cnt_act;      // [L + 1][KS]   arrivals of finished activation quarters per channel slice (64 each); layer 0: preset
  unsigned* err;          // error word: non-zero = a wait gave up
  int L;
  unsigned long long* stamps;   // [WGS][L][8] s_memtime of thread 0 at the phase boundaries (diagnostic)
};
#define PC_STAMP(k)                                                                                   \
  do {                                                                                                \
    if (t == 0 && a.stamps) {                                                                         \
      unsigned long long t_;                                                                          \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                     \
      a.stamps[((size_t)blockIdx.x * a.L + l) * 8 + (k)] = t_;                                        \
    }                                                                                                 \
  } while (0)

typedef __attribute__((address_space(3))) void lds_v;
typedef __attribute__((address_space(1))) unsigned gu32;

__device__ __forceinline__ half8 ld_sc1_b128(const void* p) {
  half8 v;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
  return v;
}
__device__ __forceinline__ void st_sc1_b128(void* p, f32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void st_sc1_b64(void* p, unsigned long long v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one lane polls a counter until it reaches `want`; bounded; returns false (and raises the error word) on give-up
__device__ __forceinline__ bool wait_count(unsigned* cnt, unsigned want, unsigned* err, unsigned code) {
  bool ok = true;
  if (threadIdx.x == 0) {
    int spins = 0;
    if (__hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) return false;   // someone gave up: drain quickly
    while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want) {
      if (++spins > SPIN_LIMIT) { ok = false; __hip_atomic_store(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
      __builtin_amdgcn_s_sleep(2);
    }
  }
  return ok;   // only thread 0's value matters; callers only use it to stop waiting later
}

__global__ __launch_bounds__(T) void chain_kernel(Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* const Wb = smem;
  char* const Xb = smem + W_BYTES;
  float* const red = reinterpret_cast<float*>(smem + W_BYTES + X_BYTES);
  float* const gsc = reinterpret_cast<float*>(smem + W_BYTES + X_BYTES + RED_BYTES);     // [8 waves][8 groups][2] + [8][2] stats
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int ntile = blockIdx.x / KS, ks = blockIdx.x % KS;
  const int c_lo = ks * KSL;
  // zero the halo (whole tile once; the interior is rewritten every layer)
  for (int i = t; i < X_BYTES / 16; i += T) reinterpret_cast<f32x4*>(Xb)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // waves 4-7 own the weight DMA (18 KiB-instructions each): waves 0-3 do the sc1 hand-off traffic, whose vmcnt(0) drains
  // would otherwise wait for the DMA as well (one in-order counter) and put the prefetch back on the critical path
  auto issue_weights = [&](int l) {
    if (wave < 4) return;
    const char* src = reinterpret_cast<const char*>(a.W) + ((size_t)(l * NTILES + ntile) * KS + ks) * W_BYTES;
    for (int i = wave - 4; i < W_BYTES / 1024; i += 4)
      __builtin_amdgcn_global_load_lds(src + i * 1024 + lane * 16, (lds_v*)(Wb + i * 1024), 16, 0, 0);
  };
  issue_weights(0);
  // this thread in the activation stage: pixel p, group g of the slice (32 consecutive channels)
  const int p = t >> 3, g = t & 7;
  const int py = p >> 3, px = p & 7, pp = (py + 1) * 10 + (px + 1);
  for (int l = 0; l < a.L; ++l) {
    const half_t* Xin = a.X + (size_t)l * HWP * C;
    half_t* Xout = a.X + (size_t)(l + 1) * HWP * C;
    // affine operands of this thread's 32 channels: issued before the wait, so their round trip hides under it
    f32x4 gam4[8], bet4[8];
    {
      const f32x4* gp = reinterpret_cast<const f32x4*>(a.gamma + (size_t)l * C + c_lo + g * 32);
      const f32x4* bp = reinterpret_cast<const f32x4*>(a.beta + (size_t)l * C + c_lo + g * 32);
#pragma unroll
      for (int k = 0; k < 8; ++k) { gam4[k] = gp[k]; bet4[k] = bp[k]; }
    }
    PC_STAMP(0);
    // ---- 1. previous layer's activation: our own channel slice, and the slice our residual lives in ----
    wait_count(a.cnt_act + l * KS + ks, 64, a.err, 1);
    wait_count(a.cnt_act + l * KS + ntile / (KSL / NT), 64, a.err, 2);
    __syncthreads();
    PC_STAMP(1);
    float v[32];
    {
      const half_t* src = Xin + (size_t)p * C + c_lo + g * 32;
      half8 h[4];
      asm volatile("global_load_dwordx4 %0, %4, off sc1\n\tglobal_load_dwordx4 %1, %4, off offset:16 sc1\n\t"
                   "global_load_dwordx4 %2, %4, off offset:32 sc1\n\tglobal_load_dwordx4 %3, %4, off offset:48 sc1\n\t"
                   "s_waitcnt vmcnt(0)"
                   : "=&v"(h[0]), "=&v"(h[1]), "=&v"(h[2]), "=&v"(h[3]) : "v"(src) : "memory");
#pragma unroll
      for (int i = 0; i < 32; ++i) v[i] = (float)h[i >> 3][i & 7];
    }
    PC_STAMP(2);
    // ---- 2. GroupNorm32 statistics of the 8 groups of this slice (64 pixels x 32 channels each), about a pivot ----
    const float pv = __shfl(v[0], g);        // lane g of wave 0..: pixel (wave*8), group g -> same pivot for a group within a wave
    float s = 0.f, q = 0.f;
#pragma unroll
    for (int i = 0; i < 32; ++i) { const float d = v[i] - pv; s += d; q = fmaf(d, d, q); }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) { s += __shfl_xor(s, o); q += __shfl_xor(q, o); }
    if (lane < 8) { gsc[(wave * 8 + lane) * 4 + 0] = s; gsc[(wave * 8 + lane) * 4 + 1] = q; gsc[(wave * 8 + lane) * 4 + 2] = pv; }
    __syncthreads();
    float mean, rstd;
    {
      double S = 0.0, Q = 0.0;
#pragma unroll
      for (int w = 0; w < 8; ++w) {      // to pivot 0 per wave (pivots differ between waves), in double
        const double sw = gsc[(w * 8 + g) * 4], qw = gsc[(w * 8 + g) * 4 + 1], P = gsc[(w * 8 + g) * 4 + 2];
        S += sw + 256.0 * P;
        Q += qw + P * (2.0 * sw + 256.0 * P);
      }
      const double md = S / 2048.0;
      double vd = Q / 2048.0 - md * md;
      vd = vd < 0.0 ? 0.0 : vd;
      mean = (float)md;
      rstd = (float)(1.0 / sqrt(vd + 1e-5));
    }
    // ---- 3. normalise + SiLU -> LDS tile [padded pixel][256 ch], 16-byte chunks XOR-swizzled by ((y&1)<<3 | x&7) ----
    {
      const int key = (((py + 1) & 1) << 3) | ((px + 1) & 7);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        half8 o;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int e = k * 8 + i;
          float y = (float)(half_t)((v[e] - mean) * rstd * gam4[e >> 2][e & 3] + bet4[e >> 2][e & 3]);
          y = __fdividef(y, 1.f + __expf(-y));
          o[i] = (half_t)y;
        }
        const int chunk = g * 4 + k;
        *reinterpret_cast<half8*>(Xb + pp * (KSL * 2) + ((chunk ^ key) & 31) * 16) = o;
      }
    }
    PC_STAMP(3);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's weight DMA has landed
    __syncthreads();
    PC_STAMP(4);
    // ---- 4. 288 MFMAs: wave w owns k-step w (32 channels) of every tap, all four 16-pixel blocks ----
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
      const int col = lane & 15, gg = lane >> 4;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        const half8 wf = *reinterpret_cast<const half8*>(Wb + ((tap * 8 + wave) * 64 + lane) * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int pix = j * 16 + col, y = pix >> 3, x = pix & 7;
          const int yy = y + 1 + dy, xx = x + 1 + dx;
          const int key = ((yy & 1) << 3) | (xx & 7);
          const int chunk = wave * 4 + gg;
          const half8 xf = *reinterpret_cast<const half8*>(Xb + (yy * 10 + xx) * (KSL * 2) + ((chunk ^ key) & 31) * 16);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf, acc[j], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(red + ((wave * 4 + j) * 64 + lane) * 4) = acc[j];
    __syncthreads();
    PC_STAMP(5);
    if (l + 1 < a.L) issue_weights(l + 1);                 // the weight tile is free: next layer's DMA runs under the hand-offs
    // ---- 5. partial tile of this K slice -> global (fp32, sc1), arrival ----
    float* mypart = a.part + ((size_t)(l * NTILES + ntile) * KS + ks) * (HWP * NT);
    if (t < 256) {
      const int j = t >> 6, ln = t & 63;
      f32x4 sum = *reinterpret_cast<const f32x4*>(red + ((0 * 4 + j) * 64 + ln) * 4);
#pragma unroll
      for (int w = 1; w < 8; ++w) sum += *reinterpret_cast<const f32x4*>(red + ((w * 4 + j) * 64 + ln) * 4);
      // lane ln of block j holds pixel j*16 + (ln & 15), couts (ln >> 4) * 4 .. +3
      st_sc1_b128(mypart + (j * 16 + (ln & 15)) * NT + (ln >> 4) * 4, sum);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // every STORING wave drains before the workgroup signals
    }
    __syncthreads();
    if (t == 0) __hip_atomic_fetch_add(a.cnt_part + l * NTILES + ntile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    PC_STAMP(6);
    // ---- 6. this workgroup finishes rows [16 ks, 16 ks + 16) of the tile: 4 slices in slice order, bias, residual ----
    wait_count(a.cnt_part + l * NTILES + ntile, KS, a.err, 3);
    __syncthreads();
    PC_STAMP(7);
    if (t < 64) {
      const int r = ks * 16 + (t >> 2), c4 = (t & 3) * 4;
      const float* base = a.part + (size_t)(l * NTILES + ntile) * KS * (HWP * NT) + r * NT + c4;
      f32x4 sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int z = 0; z < KS; ++z) {
        f32x4 pz;
        asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(pz) : "v"(base + z * (HWP * NT)) : "memory");
        sum += pz;
      }
      const int n = ntile * NT + c4;
      const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + (size_t)l * C + n);
      sum += b;
      unsigned long long rbits;
      asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(rbits) : "v"(Xin + (size_t)r * C + n) : "memory");
      const half4 rh4 = __builtin_bit_cast(half4, rbits);
      half4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (half_t)(sum[i] + (float)rh4[i]);
      st_sc1_b64(Xout + (size_t)r * C + n, __builtin_bit_cast(unsigned long long, o));
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (t == 0) __hip_atomic_fetch_add(a.cnt_act + (l + 1) * KS + ntile / (KSL / NT), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}
}  // namespace pc

int main(int argc, char** argv) {
  using namespace pc;
  const int L = argc > 1 ? atoi(argv[1]) : 6;
  srand(1);
  // ---- data ----
  std::vector<half_t> hW((size_t)L * C * 9 * C);          // reference layout [L][cout][tap][cin]
  for (auto& w : hW) w = (half_t)(((rand() % 2001) - 1000) / 1000.f * (1.7f / 96.f));   // ~N(0, 1/sqrt(9216)) scale
  std::vector<float> hg((size_t)L * C), hb((size_t)L * C), hbias((size_t)L * C);
  for (auto& v : hg) v = 1.f + ((rand() % 2001) - 1000) / 10000.f;
  for (auto& v : hb) v = ((rand() % 2001) - 1000) / 10000.f;
  for (auto& v : hbias) v = ((rand() % 2001) - 1000) / 50000.f;
  std::vector<half_t> hx((size_t)HWP * C);
  for (auto& v : hx) v = (half_t)(((rand() % 2001) - 1000) / 500.f);
  // persistent layout: [L][ntile][ks][tap][kstep][lane][8]: lane (r = lane & 15 -> cout, g = lane >> 4), k = kstep*32 + g*8 + j
  std::vector<half_t> hWp(hW.size());
  for (int l = 0; l < L; ++l)
    for (int nt = 0; nt < NTILES; ++nt)
      for (int ks = 0; ks < KS; ++ks)
        for (int tap = 0; tap < 9; ++tap)
          for (int kst = 0; kst < 8; ++kst)
            for (int lane = 0; lane < 64; ++lane)
              for (int j = 0; j < 8; ++j) {
                const int co = nt * NT + (lane & 15), ci = ks * KSL + kst * 32 + (lane >> 4) * 8 + j;
                hWp[((((((size_t)l * NTILES + nt) * KS + ks) * 9 + tap) * 8 + kst) * 64 + lane) * 8 + j] =
                    hW[(((size_t)l * C + co) * 9 + tap) * C + ci];
              }
  half_t *dW, *dWp, *dX, *dXref, *dA;
  float *dg, *db, *dbias, *dpart, *dslab, *dstats;
  unsigned *dcnt, *derr;
  unsigned long long* drec;
  CK(hipMalloc(&dW, hW.size() * 2)); CK(hipMalloc(&dWp, hW.size() * 2));
  CK(hipMemcpy(dW, hW.data(), hW.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(dWp, hWp.data(), hW.size() * 2, hipMemcpyHostToDevice));
  CK(hipMalloc(&dg, hg.size() * 4)); CK(hipMalloc(&db, hb.size() * 4)); CK(hipMalloc(&dbias, hbias.size() * 4));
  CK(hipMemcpy(dg, hg.data(), hg.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(db, hb.data(), hb.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dbias, hbias.data(), hbias.size() * 4, hipMemcpyHostToDevice));
  CK(hipMalloc(&dX, (size_t)(L + 1) * HWP * C * 2)); CK(hipMalloc(&dXref, (size_t)(L + 1) * HWP * C * 2));
  CK(hipMalloc(&dA, (size_t)HWP * C * 2));
  CK(hipMemcpy(dX, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
  CK(hipMemcpy(dXref, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
  CK(hipMalloc(&dpart, (size_t)L * NTILES * KS * HWP * NT * 4));
  CK(hipMalloc(&dslab, (size_t)L * 4 * HWP * C * 4));
  CK(hipMalloc(&dstats, 64 * 4));
  const size_t ncnt = (size_t)L * NTILES + (size_t)(L + 1) * KS + 16;
  CK(hipMalloc(&dcnt, ncnt * 4)); CK(hipMalloc(&derr, 64));
  CK(hipMalloc(&drec, (size_t)L * 32 * GN_REC_STRIDE * 8));
  hipStream_t s; CK(hipStreamCreate(&s));
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));

  // ---- (A) the product's launches: GroupNorm (adds up pending slices) + sliced small-map conv, 2 launches per layer ----
  auto run_launches = [&]() {
    CK(hipMemsetAsync(drec, 0, (size_t)L * 32 * GN_REC_STRIDE * 8, s));
    SlabSrc pend;
    for (int l = 0; l < L; ++l) {
      GnLocalArgs g;
      g.xa = dXref + (size_t)l * HWP * C; g.slab = pend; g.ya = pend.pending() ? dXref + (size_t)l * HWP * C : nullptr; g.Ca = C;
      g.out = dA; g.stats_out = dstats; g.gamma = dg + (size_t)l * C; g.beta = db + (size_t)l * C;
      g.N = 1; g.H = 8; g.W = 8; g.C = C; g.film = 0; g.act = 1; g.pool = 0;
      g.rec = drec + (size_t)l * 32 * GN_REC_STRIDE;
      if (gn_local_launch(g, s)) exit(1);
      IgemmArgs a;
      a.X = dA; a.Wt = dW + (size_t)l * C * 9 * C; a.out = dXref + (size_t)(l + 1) * HWP * C; a.M = HWP; a.N = C; a.K = 9 * C;
      a.conv3 = 1; a.Cin = C; a.ldx = C; a.ldw = 9 * C; a.ldo = C; a.H = 8; a.W = 8; a.out_mode = IG_OUT_F16;
      a.ksplit = 4; a.ws = dslab + (size_t)l * 4 * HWP * C; a.defer_reduce = 1;
      if (igemm_small3_launch(a, 0, s)) exit(1);
      pend = SlabSrc{};
      pend.ws = a.ws; pend.nslab = 4; pend.zstride = (long long)HWP * C; pend.bias = dbias + (size_t)l * C;
      pend.res = dXref + (size_t)l * HWP * C; pend.ldr = C;
    }
    // materialise the last output the way the next GroupNorm would (one more pass, outside the per-layer count)
    GnLocalArgs g;
    g.xa = dXref + (size_t)L * HWP * C; g.slab = pend; g.ya = dXref + (size_t)L * HWP * C; g.Ca = C; g.out = dA; g.stats_out = dstats;
    g.gamma = dg; g.beta = db; g.N = 1; g.H = 8; g.W = 8; g.C = C; g.act = 1;
    if (gn_local_launch(g, s)) exit(1);
  };
#ifdef ISHAP_STAMPS
  unsigned long long* dstg; CK(hipMalloc(&dstg, 512 * 8 * 8)); CK(hipMemset(dstg, 0, 512 * 8 * 8));
  CK(hipMemcpyToSymbol(HIP_SYMBOL(g_gn_stamps), &dstg, sizeof(dstg)));
#endif
  for (int i = 0; i < 3; ++i) run_launches();
  CK(hipStreamSynchronize(s));
#ifdef ISHAP_STAMPS
  {
    // the last GroupNorm launch of run_launches is the final materialise (parts = 1); re-run ONE mid-chain GroupNorm for the stamps
    CK(hipMemset(dstg, 0, 512 * 8 * 8));
    CK(hipMemsetAsync(drec, 0, (size_t)L * 32 * GN_REC_STRIDE * 8, s));
    SlabSrc pend; pend.ws = dslab; pend.nslab = 4; pend.zstride = (long long)HWP * C; pend.bias = dbias; pend.res = dXref; pend.ldr = C;
    GnLocalArgs g;
    g.xa = dXref + (size_t)1 * HWP * C; g.slab = pend; g.ya = dXref + (size_t)1 * HWP * C; g.Ca = C; g.out = dA; g.stats_out = dstats;
    g.gamma = dg; g.beta = db; g.N = 1; g.H = 8; g.W = 8; g.C = C; g.act = 1; g.rec = drec;
    if (gn_local_launch(g, s)) exit(1);
    CK(hipStreamSynchronize(s));
    std::vector<unsigned long long> h(512 * 8);
    CK(hipMemcpy(h.data(), dstg, h.size() * 8, hipMemcpyDeviceToHost));
    const char* nm[4] = {"slices summed (+bias, residual), fp16 stored, staged in LDS", "workgroup sums (block_sum2)", "rendezvous with the group's other parts",
                         "normalise + SiLU + store"};
    printf("  gn_local_kernel on a pending 8x8 x 1024 map (4 slices), phases (shader cycles, median over workgroups):\n");
    for (int k = 0; k < 4; ++k) {
      std::vector<double> d;
      for (int w = 0; w < 512; ++w) if (h[w * 8 + k] && h[w * 8 + k + 1] > h[w * 8 + k]) d.push_back((double)(h[w * 8 + k + 1] - h[w * 8 + k]));
      if (d.empty()) continue;
      std::sort(d.begin(), d.end());
      printf("    %-62s %7.0f   (p10 %7.0f  p90 %7.0f)  [%zu workgroups]\n", nm[k], d[d.size() / 2], d[d.size() / 10], d[d.size() * 9 / 10], d.size());
    }
  }
#endif
  float best_a = 1e9;
  for (int rep = 0; rep < 10; ++rep) {
    CK(hipEventRecord(e0, s));
    run_launches();
    CK(hipEventRecord(e1, s));
    CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    if (ms < best_a) best_a = ms;
  }
  // ---- (C) fused launches: ONE conv8 launch per layer (conv + bias + residual + the next layer's GroupNorm + SiLU) ----
  half_t *dW8, *dXc, *dAc;
  unsigned long long* drec8;
  float best_c = 1e9;
  {
    const size_t per = conv8_packed_halfs(C, C, 0, 9);
    CK(hipMalloc(&dW8, (size_t)L * per * 2));
    for (int l = 0; l < L; ++l)
      if (conv8_pack(dW + (size_t)l * C * 9 * C, 9 * C, C, C, 0, 9, dW8 + (size_t)l * per, s)) exit(1);
    CK(hipMalloc(&dXc, (size_t)(L + 1) * HWP * C * 2)); CK(hipMalloc(&dAc, (size_t)(L + 1) * HWP * C * 2));
    CK(hipMemcpy(dXc, hx.data(), hx.size() * 2, hipMemcpyHostToDevice));
    CK(hipMalloc(&drec8, (size_t)(L + 1) * 32 * GN_REC_STRIDE * 8));
#ifdef C8_STAMPS
    unsigned long long* dst8; CK(hipMalloc(&dst8, 256 * 8 * 8)); CK(hipMemset(dst8, 0, 256 * 8 * 8));
    CK(hipMemcpyToSymbol(HIP_SYMBOL(g_c8_stamps), &dst8, sizeof(dst8)));
#endif
    auto run_fused = [&]() {
      CK(hipMemsetAsync(drec8, 0, (size_t)(L + 1) * 32 * GN_REC_STRIDE * 8, s));
      GnLocalArgs g;                                  // chain start: a_0 = SiLU(GN_0(x_0)) by the ordinary kernel
      g.xa = dXc; g.Ca = C; g.out = dAc; g.stats_out = dstats; g.gamma = dg; g.beta = db; g.N = 1; g.H = 8; g.W = 8; g.C = C; g.act = 1;
      g.rec = drec8 + (size_t)L * 32 * GN_REC_STRIDE;
      if (gn_local_launch(g, s)) exit(1);
      for (int l = 0; l < L; ++l) {
        Conv8Args a;
        a.X = dAc + (size_t)l * HWP * C; a.W8 = dW8 + (size_t)l * per; a.Cin = C; a.Cout = C; a.taps = 9; a.ldx = C; a.N = 1;
        a.bias = dbias + (size_t)l * C; a.res = dXc + (size_t)l * HWP * C; a.ldr = C;
        a.y = dXc + (size_t)(l + 1) * HWP * C; a.ldy = C;
        const int ln = l + 1 < L ? l + 1 : 0;          // the last layer normalises with layer 0's parameters (same work)
        a.gamma = dg + (size_t)ln * C; a.beta = db + (size_t)ln * C; a.act = 1; a.cpg = 32; a.norm_C = C;
        a.a_out = dAc + (size_t)(l + 1) * HWP * C; a.lda = C; a.stats_out = dstats;
        a.rec = drec8 + (size_t)l * 32 * GN_REC_STRIDE;
        if (conv8_launch(a, s)) exit(1);
      }
    };
    for (int i = 0; i < 3; ++i) run_fused();
    CK(hipStreamSynchronize(s));
    for (int rep = 0; rep < 10; ++rep) {
      CK(hipEventRecord(e0, s));
      run_fused();
      CK(hipEventRecord(e1, s));
      CK(hipEventSynchronize(e1));
      float ms; CK(hipEventElapsedTime(&ms, e0, e1));
      if (ms < best_c) best_c = ms;
    }
#ifdef C8_STAMPS
    {
      std::vector<unsigned long long> h(256 * 8);
      CK(hipMemcpy(h.data(), dst8, h.size() * 8, hipMemcpyDeviceToHost));
      const char* nm[7] = {"zero the tiles + barrier", "chunk 0 landed (ring fill)", "K loop (chunks 1..)", "8-wave sum, bias, residual, y stored",
                           "tile statistics", "rendezvous with the group's other workgroups", "normalise + SiLU + store"};
      printf("  conv8 phases of the last launch (shader cycles, median over its 256 workgroups):\n");
      for (int k = 0; k < 7; ++k) {
        std::vector<double> d;
        for (int w = 0; w < 256; ++w) if (h[w * 8 + k] && h[w * 8 + k + 1] > h[w * 8 + k]) d.push_back((double)(h[w * 8 + k + 1] - h[w * 8 + k]));
        if (d.empty()) continue;
        std::sort(d.begin(), d.end());
        printf("    %-50s %7.0f   (p10 %7.0f  p90 %7.0f)\n", nm[k], d[d.size() / 2], d[d.size() / 10], d[d.size() * 9 / 10]);
      }
    }
#endif
    std::vector<half_t> ya((size_t)HWP * C), yc((size_t)HWP * C);
    CK(hipMemcpy(ya.data(), dXref + (size_t)L * HWP * C, ya.size() * 2, hipMemcpyDeviceToHost));
    CK(hipMemcpy(yc.data(), dXc + (size_t)L * HWP * C, yc.size() * 2, hipMemcpyDeviceToHost));
    double num = 0, den = 0, mx = 0;
    for (size_t i = 0; i < ya.size(); ++i) { const double d = (double)yc[i] - (double)ya[i]; num += d * d; den += (double)ya[i] * (double)ya[i]; mx = fmax(mx, fabs(d)); }
    printf("  fused launches (conv8: conv + next GroupNorm, 1 per layer + 1):    %8.2f us total, %6.2f us per layer;  vs launches: rel L2 diff %.3e, max abs %.4g, status %u\n",
           best_c * 1e3, best_c * 1e3 / L, sqrt(num / (den + 1e-30)), mx, *ishap_status_word());
  }
  // ---- (B) the persistent launch ----
  Args pa;
  pa.W = dWp; pa.gamma = dg; pa.beta = db; pa.bias = dbias; pa.X = dX; pa.part = dpart;
  pa.cnt_part = dcnt; pa.cnt_act = dcnt + (size_t)L * NTILES; pa.err = derr; pa.L = L; pa.stamps = nullptr;
  CK(hipFuncSetAttribute((const void*)chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_BYTES));
  std::vector<unsigned> hcnt(ncnt, 0u);
  for (int k = 0; k < KS; ++k) hcnt[(size_t)L * NTILES + k] = 64;        // layer 0's input is there
  unsigned* hcnt_dev_init; CK(hipMalloc(&hcnt_dev_init, ncnt * 4));
  CK(hipMemcpy(hcnt_dev_init, hcnt.data(), ncnt * 4, hipMemcpyHostToDevice));
  auto run_persist = [&]() {
    CK(hipMemcpyAsync(dcnt, hcnt_dev_init, ncnt * 4, hipMemcpyDeviceToDevice, s));
    CK(hipMemsetAsync(derr, 0, 64, s));
    hipLaunchKernelGGL(chain_kernel, dim3(WGS), dim3(T), LDS_BYTES, s, pa);
  };
  for (int i = 0; i < 3; ++i) run_persist();
  CK(hipStreamSynchronize(s));
  unsigned herr = 0; CK(hipMemcpy(&herr, derr, 4, hipMemcpyDeviceToHost));
  float best_b = 1e9;
  for (int rep = 0; rep < 10; ++rep) {
    CK(hipEventRecord(e0, s));
    run_persist();
    CK(hipEventRecord(e1, s));
    CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    if (ms < best_b) best_b = ms;
  }
  CK(hipMemcpy(&herr, derr, 4, hipMemcpyDeviceToHost));
  {   // one more run with stamps: median over workgroups of each phase of the middle layers
    unsigned long long* dst; CK(hipMalloc(&dst, (size_t)WGS * L * 8 * 8)); CK(hipMemset(dst, 0, (size_t)WGS * L * 8 * 8));
    pa.stamps = dst;
    run_persist();
    CK(hipStreamSynchronize(s));
    pa.stamps = nullptr;
    std::vector<unsigned long long> h((size_t)WGS * L * 8);
    CK(hipMemcpy(h.data(), dst, h.size() * 8, hipMemcpyDeviceToHost));
    const char* nm[8] = {"wait for activation (+ barrier)", "activation slice loaded (sc1)", "GN statistics + normalise + SiLU -> LDS",
                         "weight DMA landed + barrier", "288 MFMAs + wave partials to LDS", "8-wave sum, partial tile stored (sc1), drained, signalled",
                         "wait for the 4 slices (+ barrier)", "(next layer's top: quarter rows summed, stored, signalled)"};
    printf("  persistent kernel, phases of layers 1..%d (shader cycles, median over workgroups and layers):\n", L - 1);
    for (int k = 0; k < 8; ++k) {
      std::vector<double> d;
      for (int w = 0; w < WGS; ++w)
        for (int l = 1; l < L; ++l) {
          const unsigned long long* r = &h[((size_t)w * L + l) * 8];
          const unsigned long long nxt = k < 7 ? r[k + 1] : (l + 1 < L ? h[((size_t)w * L + l + 1) * 8] : 0);
          if (r[k] && nxt > r[k]) d.push_back((double)(nxt - r[k]));
        }
      if (d.empty()) continue;
      std::sort(d.begin(), d.end());
      printf("    %-62s %7.0f   (p10 %7.0f  p90 %7.0f)\n", nm[k], d[d.size() / 2], d[d.size() / 10], d[d.size() * 9 / 10]);
    }
  }
  // ---- compare the final activations ----
  std::vector<half_t> ya((size_t)HWP * C), yb((size_t)HWP * C);
  CK(hipMemcpy(ya.data(), dXref + (size_t)L * HWP * C, ya.size() * 2, hipMemcpyDeviceToHost));
  CK(hipMemcpy(yb.data(), dX + (size_t)L * HWP * C, yb.size() * 2, hipMemcpyDeviceToHost));
  double num = 0, den = 0, mx = 0;
  for (size_t i = 0; i < ya.size(); ++i) {
    const double d = (double)yb[i] - (double)ya[i];
    num += d * d; den += (double)ya[i] * (double)ya[i]; mx = fmax(mx, fabs(d));
  }
  printf("chain of %d layers (GroupNorm32 + SiLU + 3x3 conv 1024->1024 + bias + residual) on an 8x8 map, 18.9 MB of weights each\n", L);
  printf("  launches (gn_local + conv3_small x 4 slices, 2 per layer): %8.2f us total, %6.2f us per layer\n", best_a * 1e3, best_a * 1e3 / L);
  printf("  one persistent launch (256 workgroups):                    %8.2f us total, %6.2f us per layer (incl. %s)\n",
         best_b * 1e3, best_b * 1e3 / L, "counter reset memcpy + launch");
  printf("  persistent / launches = %.2fx;  error word %u;  final activation: rel L2 diff %.3e, max abs diff %.4g (|x| rms %.3g)\n",
         best_b / best_a, herr, sqrt(num / (den + 1e-30)), mx, sqrt(den / ya.size()));
  return 0;
}
