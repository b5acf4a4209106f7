// Implicit-GEMM on the CDNA4 matrix cores: every 3x3 / 1x1 convolution of the UNet
// (reference: guided_diffusion/unet.py:185,211,222,286,294,482,615 -- all stock
// torch conv ops there) and every attention matmul (unet.py:349-353) runs through
// this one kernel family.
//
//   D[n][m] = sum_k Wt[n][k] * X(m,k)        (fp16 operands, fp32 accumulate)
//
// m = output pixel (NHWC row), n = output channel, k = tap*Cin + c.  The weight tile is
// the MFMA "A" operand and the pixel tile the "B" operand, so each lane ends up holding
// 4 consecutive output channels of one pixel: an 8-byte NHWC store, no shuffle.
//
// Block = 256 threads = 4 waves (WM x WN).  Tiles are staged global -> registers -> LDS
// (double-buffered, one barrier per K-step); the 16-byte chunk index is XOR-swizzled with
// (row>>1) so both the ds_write_b128 and the ds_read_b128 fragment reads are
// bank-conflict free (lane-group table of the gfx950 LDS).
#include "common.h"
#include "igemm_epilogue.h"
#include "gn_bwd_terms.h"
#include "norm.h"
#include "../../include/ishap.h"

template <int BM, int BN, int BK, int WM, int WN, bool CONV3>
__global__ __launch_bounds__(256) void igemm_kernel(IgemmArgs a) {
  constexpr int CPR = BK / 8;               // 16-byte chunks per tile row
  constexpr int XL = BM * CPR / 256;        // chunks per thread, X tile
  constexpr int WL = BN * CPR / 256;
  constexpr int TMW = BM / WM, TNW = BN / WN;
  constexpr int MT = TMW / 16, NT = TNW / 16;
  static_assert(XL >= 1 && WL >= 1, "tile too small for 256 threads");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  half_t* sX = reinterpret_cast<half_t*>(smem_raw);          // [2][BM*BK]
  half_t* sW = sX + 2 * BM * BK;                             // [2][BN*BK]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int m0 = blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const int batch = blockIdx.z / a.ksplit;
  const int ks_id = blockIdx.z % a.ksplit;

  const half_t* X = a.X + (long long)batch * a.bsx;
  const half_t* Wt = a.Wt + (long long)batch * a.bsw;

  const int KS = a.K / BK;
  const int per = (KS + a.ksplit - 1) / a.ksplit;
  const int ks0 = ks_id * per;
  const int ks1 = min(KS, ks0 + per);
  const int steps_per_tap = CONV3 ? a.Cin / BK : KS;
  const int HW = a.H * a.W;

  // per-thread loader coordinates
  int xrow[XL], xch[XL], xn[XL], xy[XL], xx[XL];
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    int idx = tid + i * 256;
    xrow[i] = idx / CPR;
    xch[i] = idx % CPR;
    int m = m0 + xrow[i];
    if (CONV3) {
      xn[i] = m / HW;
      int p = m - xn[i] * HW;
      xy[i] = p / a.W;
      xx[i] = p - xy[i] * a.W;
    } else {
      xn[i] = m; xy[i] = 0; xx[i] = 0;
    }
  }
  int wrow[WL], wch[WL];
#pragma unroll
  for (int i = 0; i < WL; ++i) {
    int idx = tid + i * 256;
    wrow[i] = idx / CPR;
    wch[i] = idx % CPR;
  }

  half8 rx[XL], rw[WL];
  auto load_tiles = [&](int ks) {
    int tap = 0, c0;
    if (CONV3) { tap = ks / steps_per_tap; c0 = (ks - tap * steps_per_tap) * BK; }
    else c0 = ks * BK;
    const int dy = CONV3 ? tap / 3 - 1 : 0;
    const int dx = CONV3 ? tap % 3 - 1 : 0;
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      half8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (CONV3) {
        int yy = xy[i] + dy, xc = xx[i] + dx;
        if (yy >= 0 && yy < a.H && xc >= 0 && xc < a.W) {
          long long src;
          if (a.ups) src = (long long)xn[i] * (HW >> 2) + (yy >> 1) * (a.W >> 1) + (xc >> 1);
          else src = (long long)xn[i] * HW + yy * a.W + xc;
          v = *reinterpret_cast<const half8*>(X + src * a.ldx + c0 + xch[i] * 8);
        }
      } else {
        v = *reinterpret_cast<const half8*>(X + (long long)xn[i] * a.ldx + c0 + xch[i] * 8);
      }
      rx[i] = v;
    }
    const int kofs = CONV3 ? tap * a.Cin + c0 : c0;
#pragma unroll
    for (int i = 0; i < WL; ++i)
      rw[i] = *reinterpret_cast<const half8*>(Wt + (long long)(n0 + wrow[i]) * a.ldw + kofs + wch[i] * 8);
  };
  auto store_tiles = [&](int buf) {
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      int ph = xch[i] ^ ((xrow[i] >> 1) & (CPR - 1));
      *reinterpret_cast<half8*>(sX + buf * BM * BK + xrow[i] * BK + ph * 8) = rx[i];
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      int ph = wch[i] ^ ((wrow[i] >> 1) & (CPR - 1));
      *reinterpret_cast<half8*>(sW + buf * BN * BK + wrow[i] * BK + ph * 8) = rw[i];
    }
  };

  f32x4 acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (ks0 < ks1) {
    load_tiles(ks0);
    store_tiles(0);
    __syncthreads();
    int buf = 0;
    for (int ks = ks0; ks < ks1; ++ks) {
      const bool more = ks + 1 < ks1;
      if (more) load_tiles(ks + 1);
      const half_t* bx = sX + buf * BM * BK;
      const half_t* bw = sW + buf * BN * BK;
#pragma unroll
      for (int kk = 0; kk < BK / 32; ++kk) {
        half8 xf[MT], wf[NT];
        const int ch = (lane >> 4) + 4 * kk;
#pragma unroll
        for (int j = 0; j < MT; ++j) {
          int row = wm * TMW + j * 16 + (lane & 15);
          xf[j] = *reinterpret_cast<const half8*>(bx + row * BK + ((ch ^ ((row >> 1) & (CPR - 1))) * 8));
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          int row = wn * TNW + i * 16 + (lane & 15);
          wf[i] = *reinterpret_cast<const half8*>(bw + row * BK + ((ch ^ ((row >> 1) & (CPR - 1))) * 8));
        }
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
          for (int j = 0; j < MT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], xf[j], acc[i][j], 0, 0, 0);
      }
      if (more) store_tiles(buf ^ 1);
      __syncthreads();
      buf ^= 1;
    }
  }

  igemm_epilogue<MT, NT, TMW, TNW, BN>(a, acc, m0, n0, wm, wn, lane, batch, ks_id, reinterpret_cast<float*>(smem_raw));
}

// out = alpha * sum_z ws[z] (+bias)(+res).  Block = 16 rows x 64 channels (thread = one row, 4 channels); when
// `stat_out` is set the block also adds its per-channel (sum, sum of squares) of the stored fp16 values.
__global__ __launch_bounds__(256) void igemm_splitk_reduce(IgemmArgs a) {
  __shared__ float red[16][64][2];
  const int nq = (a.N + 63) / 64;                 // channel groups of 64
  const int rb = a.M / 16;                        // row blocks
  const int bid = blockIdx.x;
  const int cg = bid % nq;
  const int rbi = (bid / nq) % rb;
  const int batch = bid / (nq * rb);
  const int r = threadIdx.x >> 4, qd = threadIdx.x & 15;
  const int m = rbi * 16 + r;
  const int n = cg * 64 + qd * 4;
  const bool ok = n < a.N;
  const int HW = a.H * a.W;
  half4 o = {0, 0, 0, 0};
  if (ok) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const float* wp = a.ws + ((long long)batch * a.M + m) * a.N + n;
    const long long zs = (long long)a.nbatch * a.M * a.N;
    int z = 0;
    for (; z + 4 <= a.ksplit; z += 4) {             // four slices in flight; summed in slice order
      const f32x4 p0 = *reinterpret_cast<const f32x4*>(wp + (z + 0) * zs), p1 = *reinterpret_cast<const f32x4*>(wp + (z + 1) * zs);
      const f32x4 p2 = *reinterpret_cast<const f32x4*>(wp + (z + 2) * zs), p3 = *reinterpret_cast<const f32x4*>(wp + (z + 3) * zs);
      v += p0; v += p1; v += p2; v += p3;
    }
    for (; z < a.ksplit; ++z) v += *reinterpret_cast<const f32x4*>(wp + z * zs);
    v *= a.alpha;
    if (a.bias) v += *reinterpret_cast<const f32x4*>(a.bias + n);
    if (a.bias2) v += *reinterpret_cast<const f32x4*>(a.bias2 + n);
    int n_img = 0, py = 0, px = 0;
    if (a.res_ups || a.out_mode == IG_OUT_NCHW_F32) {
      n_img = m / HW;
      int p = m - n_img * HW;
      py = p / a.W;
      px = p - py * a.W;
    }
    if (a.res) {
      long long rrow = a.res_ups ? ((long long)n_img * (HW >> 2) + (py >> 1) * (a.W >> 1) + (px >> 1)) : m;
      half4 rr = *reinterpret_cast<const half4*>(a.res + rrow * a.ldr + n);
      v[0] += (float)rr[0]; v[1] += (float)rr[1]; v[2] += (float)rr[2]; v[3] += (float)rr[3];
    }
    if (a.out_mode == IG_OUT_F16) {
      o = (half4){(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
      *reinterpret_cast<half4*>((half_t*)a.out + (long long)batch * a.bso + (long long)m * a.ldo + n) = o;
    } else if (a.out_mode == IG_OUT_F32) {
      *reinterpret_cast<f32x4*>((float*)a.out + (long long)batch * a.bso + (long long)m * a.ldo + n) = v;
    } else {
      float* op = (float*)a.out + ((long long)n_img * a.N + n) * HW + (py * a.W + px);
      for (int k = 0; k < 4; ++k) op[(long long)k * HW] = v[k];
    }
  }
  if (a.stat_out || a.gb_x) {
    long long* const sdst = a.gb_x ? a.gb_csums : a.stat_out;
    const float scale_q = a.gb_x ? STAT_SCALE_SUM : STAT_SCALE_SQ;
    if (a.gb_x) {                              // GroupNorm-backward sums of the stored gradient (see common.h)
      const int n_img = m / HW, cpg = a.N / 32;
      half4 xv = {0, 0, 0, 0};
      if (ok) xv = *reinterpret_cast<const half4*>(a.gb_x + (long long)m * a.N + n);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float dyh = 0.f, xhat = 0.f;
        if (ok) {
          const int g = (n + c) / cpg;
          gn_bwd_term((float)o[c], (float)xv[c], a.gb_stats[(n_img * 32 + g) * 2], a.gb_stats[(n_img * 32 + g) * 2 + 1],
                      a.gb_gamma[n + c], a.gb_beta[n + c], a.gb_film ? a.gb_emb[(long long)n_img * a.gb_emb_ld + n + c] : 0.f,
                      a.gb_film ? a.gb_emb[(long long)n_img * a.gb_emb_ld + a.N + n + c] : 0.f, a.gb_film != 0, a.gb_act != 0, dyh, xhat);
        }
        red[r][qd * 4 + c][0] = dyh;
        red[r][qd * 4 + c][1] = dyh * xhat;
      }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float f = (float)o[c];
        red[r][qd * 4 + c][0] = f;
        red[r][qd * 4 + c][1] = f * f;
      }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 128) {
      const int ch = t >> 1, k = t & 1;
      // double: f and f*f of an fp16 value are exact, and so is their sum -- an fp32 sum of 16 squares at |mean| >> std
      // already loses the variance (see igemm_epilogue.h)
      double acc = 0.0;
#pragma unroll
      for (int rr = 0; rr < 16; ++rr) acc += (double)red[rr][ch][k];
      const int nn = cg * 64 + ch;
      if (nn < a.N)
        atomicAdd(reinterpret_cast<unsigned long long*>(sdst + ((long long)((rbi * 16) / HW) * a.N + nn) * 2 + k),
                  (unsigned long long)__double2ll_rn(acc * (double)(k ? scale_q : STAT_SCALE_SUM)));
    }
  }
}

// ---- optional per-launch timing (bench.py's roofline leg): HIP events on the launch stream around the main kernel ----
#include <vector>
struct ProfRec { hipEvent_t a, b, c; double flops; int variant; int M, N, K, conv3, big, ksplit; };
static bool g_prof_on = false;
hipEvent_t g_igemm_prof_start = nullptr, g_igemm_prof_stop = nullptr;
static std::vector<ProfRec> g_prof;
static std::vector<hipEvent_t> g_prof_pool;
static hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}
bool ishap_profile_recording() { return g_prof_on; }
extern "C" int ishap_profile_begin(void) {
  for (auto& r : g_prof) { g_prof_pool.push_back(r.a); g_prof_pool.push_back(r.b); if (r.c) g_prof_pool.push_back(r.c); }
  g_prof.clear();
  g_prof_on = true;
  return 0;
}
// out[v*3 + {0,1,2}] = {launches, total milliseconds, algorithmic FLOPs} for variant v (igemm_prof_slot):
//   0 / 1 igemm2 conv3x3 128x128 / 64x64 tile, 2 / 3 igemm2 GEMM 128x128 / 64x64 tile, 4 igemm2 conv3x3 64x64 two-team,
//   5 small-map (skinny) kernel, 6 register-staged (BK = 32) kernel, 7 igemm4's 128x32 halo tiles (igemm4_halo_kernel),
//   8 / 9 / 10 igemm4 128x128 tile / 64x64 tile (either ring) / 64x64 two-team, 11 igemm4's sliced launches on the 8x8 maps,
//   12 igemm4's 128x64 tiles
extern "C" int ishap_profile_end(double* out, int nvar) {
  g_prof_on = false;
  for (int i = 0; i < nvar * 3; ++i) out[i] = 0.0;
  for (auto& r : g_prof) {
    if (hipEventSynchronize(r.b) != hipSuccess) return -1;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return -1;
    if (r.variant < nvar) { out[r.variant * 3] += 1.0; out[r.variant * 3 + 1] += ms; out[r.variant * 3 + 2] += r.flops; }
  }
  return 0;
}

// Per-shape breakdown of the launches recorded since ishap_profile_begin (call before ishap_profile_end resets
// nothing; both may be called): CSV lines "M,N,K,conv3,tile,ksplit,launches,main_ms,reduce_ms,gflop" into buf.
#include <map>
#include <cstring>
#include <array>
#include <string>
extern "C" int ishap_profile_shapes(char* buf, int cap) {
  std::map<std::array<int, 6>, std::array<double, 4>> agg;
  for (auto& r : g_prof) {
    if (hipEventSynchronize(r.c ? r.c : r.b) != hipSuccess) return -1;
    float ms = 0.f, ms2 = 0.f;
    if (hipEventElapsedTime(&ms, r.a, r.b) != hipSuccess) return -1;
    if (r.c && hipEventElapsedTime(&ms2, r.b, r.c) != hipSuccess) return -1;
    auto& v = agg[{r.M, r.N, r.K, r.conv3, r.big ? 128 : 64, r.ksplit}];
    v[0] += 1.0; v[1] += ms; v[2] += ms2; v[3] += r.flops * 1e-9;
  }
  std::string out;
  char line[160];
  for (auto& kv : agg) {
    snprintf(line, sizeof line, "%d,%d,%d,%d,%d,%d,%.0f,%.4f,%.4f,%.3f\n", kv.first[0], kv.first[1], kv.first[2], kv.first[3],
             kv.first[4], kv.first[5], kv.second[0], kv.second[1], kv.second[2], kv.second[3]);
    out += line;
  }
  if ((int)out.size() + 1 > cap) return -2;
  memcpy(buf, out.c_str(), out.size() + 1);
  return (int)agg.size();
}

// ---- the launch plan: K slices and kernel form of every implicit-GEMM launch (no HIP runtime call) ----
const IgemmSwitches& igemm_switches() {
  static const IgemmSwitches sw = [] {
    return IgemmSwitches{ishap_switch("ISHAP_IGEMM4", 2), ishap_switch("ISHAP_IG4_TEAMS", 2), ishap_switch("ISHAP_IG4_HALO", 1),
                         ishap_switch("ISHAP_HALVES", 2), ishap_switch("ISHAP_SKINNY", 1), ishap_switch("ISHAP_G1_SLICES", 1),
                         ishap_switch("ISHAP_BIG_MIN", 192)};
  }();
  return sw;
}

// Tile and split-K policy.  256 CUs: prefer the 128x128 tile when it alone yields >= ~200 workgroups, otherwise the
// 64x64 tile; split K while the grid stays below ~224 workgroups (the small-map, weight-streaming layers),
// keeping >= 6 K-steps of 64 per slice so the fp32 partial traffic stays below the weight traffic.
static bool use_big(const IgemmArgs& a, const IgemmSwitches& sw) {
  if (a.M % 128 != 0 || a.N < 128) return false;
  return (long long)(a.M / 128) * ceil_div(a.N, 128) * a.nbatch >= sw.big_min;
}

int igemm_plan_ksplit(const IgemmArgs& a, bool pending, const IgemmSwitches& sw) {
  const bool big = use_big(a, sw);
  const int bm = big ? 128 : 64, bn = big ? 128 : 64;
  const long long blocks = (long long)(a.M / bm) * ceil_div(a.N, bn) * a.nbatch;
  const int ks = a.K / 64;
  // policy constants, each swept in situ (profiles/round4_env_ab_pending_split.txt,
  // profiles/round5_ab_policy_resweep.txt: all flat within +-0.5 % around these values)
  constexpr int nosplit = 36;       // K-steps below which a launch followed by a reduce launch is not split (24 / 48: +0.5 %)
  constexpr int fill = 224;         // split while the grid stays below this many workgroups (plateau 208 .. 256)
  constexpr int minsteps = 6;       // K-steps left per slice at least
  // slices whose consumer adds them up cost no reduce launch: thresholds of their own (12 / 3 against 36 / 6: 0.1783 -> 0.1777 s/shape)
  constexpr int p_nosplit = 12, p_minsteps = 3;
  int split = 1;
  if (ks >= (pending ? p_nosplit : nosplit))        // below ~36 K-steps the extra reduce launch (~5.5 us) costs more than the split saves (harness sweep: ~48; in situ: 36)
    while (blocks * split < fill && ks / (split * 2) >= (pending ? p_minsteps : minsteps) && split < 32) split *= 2;
  if (!a.conv3 && a.M <= 64 && a.K % 64 == 0) {
    // 1x1 GEMMs on the 8x8 maps: the one-launch small-map kernel (10.7 vs 16.2 us at K = 3072) -- unless the consumer adds K
    // slices up and K is long: then the tiled kernel with 8-16 slices left pending (harness, K = 3072 -> 1024: 5.0 us against
    // the skinny kernel's 8.1; at K = 1024 the two tie, profiles/round4_gemm1x1_slices_probe.txt).  ISHAP_G1_SLICES=0: off
    split = (sw.g1_slices && pending && a.K >= 2048) ? (a.K >= 3072 ? 16 : 8) : 1;
  }
  if (sw.igemm4 > 1 && pending && a.conv3 && a.W == 8 && a.H == 8 && a.nbatch == 1 && a.Cin % 64 == 0 && a.M % 64 == 0 &&
      a.K == 9 * a.Cin + a.K2 && (!a.K2 || (a.K2 % 64 == 0 && a.K2 / 64 <= 127 && a.X2))) {
    // 3x3 on the 8x8 maps whose consumer adds K slices up: igemm4's 64x64 tiles (= one image) with enough slices for ~one
    // workgroup per CU: the harness has 16 x 16 workgroups at 8.1 us against 9.1 for the one-launch small-map kernel this replaced
    // (1024 -> 1024), 11.3 against 15.1 (2048 -> 1024), 11.1 against 16.4 (1024 -> 2048), 9.5 against 23.9 with the folded skip
    // (profiles/round4_igemm4_w8_probe.txt, _w8_k2_probe.txt).  Fewer than 2 slices: the generic split above
    constexpr int target = 256;        // workgroups (in-situ sweep 256 .. 640: flat)
    const int tiles = (a.M / 64) * ((a.N + 63) / 64), G = 3 * (a.Cin / 64);
    int s4 = (target + tiles / 2) / tiles;
    if (s4 > 16) s4 = 16;
    if (s4 > G) s4 = G;
    if (s4 >= 2) {
      const int per = (G + s4 - 1) / s4;
      split = (G + per - 1) / per;                   // no slice without 3x3 groups (the second source's chunks are dealt out likewise)
    }
  }
  return split;
}

IgemmPlan igemm_plan(const IgemmArgs& a, const IgemmSwitches& sw) {
  // 1x1 GEMMs on the 8x8 maps: the one-launch skinny kernel beats the tiled one there (measured in situ: 7.8 vs 11.4 us
  // at 64 x 1024 x 1024); in situ it wins at M = 64 (-3..5 us per launch) and loses at M = 256; for 3x3 layers it re-reads
  // the im2col fragments once per 16-channel tile and loses (L2-bound).  ISHAP_SKINNY=0: the tiled kernel + reduce instead
  if (sw.skinny && !a.conv3 && a.M <= 64 && igemm_skinny_applicable(a)) return {IgemmForm::skinny, false};
  // K not a multiple of 64 (tiny configurations; the full model's stem is padded to 128 channels): the register-staged kernel,
  // built with 64x64 tiles only
  if (a.conv3 ? a.Cin % 64 != 0 : a.K % 64 != 0) return {IgemmForm::reg32, false};
  // the statistics epilogues file a whole tile under image m0 / HW: a tile must not straddle two images
  const bool big = use_big(a, sw) && (!(a.stat_out || a.gb_x) || (a.H * a.W) % 128 == 0);
  // igemm4 takes 3x3 launches (optionally with the folded 1x1 second source) with Cin % 64 == 0, one image per tile, a tile =
  // whole image rows of a map 16 / 32 / 64 / 128 pixels wide.  ISHAP_IGEMM4: 0 = never, 1 = 128x128 tiles only, 2 = all of these
  auto igemm4_takes = [&] {
    const int BM = big ? 128 : 64;
    if (!sw.igemm4 || (sw.igemm4 == 1 && !big)) return false;
    if (!a.conv3 || a.nbatch != 1 || a.Cin % 64 != 0 || a.K != 9 * a.Cin + a.K2) return false;
    if (a.K2 && (a.K2 % 64 != 0 || a.K2 / 64 > 127 || !a.X2)) return false;
    // the folded second source runs with a short lookahead (one slab per step, NSTX - 1 ahead): worth it on the 128-tiles
    // (-11 %), a loss on the 64-tiles (+4..18 %, profiles/round4_igemm4_probe_v4.txt) -- those stay with igemm2
    // (the sliced launches on the 8x8 maps excepted: 9.5 us against 23.9 for the one-launch kernel they replaced, round 4)
    const bool w8 = !big && a.W == 8 && a.H == 8 && a.ksplit > 1;
    if (a.K2 && !big && !w8) return false;
    // (128-pixel tiles on maps narrower than 128: several image rows per tile -- the batched generate path, where M = batch * H * W
    // fills the chip with 128x128 tiles on the 64^2 ... 16^2 maps)
    if (big ? (a.W != 128 && a.W != 64 && a.W != 32 && a.W != 16) : (a.W != 16 && a.W != 32 && a.W != 64 && !w8)) return false;
    return BM % a.W == 0 && (a.H * a.W) % BM == 0 && a.M % BM == 0;
  };
  if (!igemm4_takes()) {
    if (big) return {IgemmForm::ig2_128, true};
    // one workgroup per CU at most and a K slice long enough to split: the two-team variant of the 64x64 conv kernel
    // (measured: +4..16 % there, a loss on short slices and 1x1).  ISHAP_HALVES=1: one team
    const long long tiles = (long long)(a.M / 64) * ((a.N + 63) / 64) * a.nbatch * a.ksplit;
    const int steps = (a.K / 64 + a.ksplit - 1) / a.ksplit;
    if (sw.halves == 2 && a.conv3 && tiles <= 256 && steps >= 16) return {IgemmForm::ig2_teams, false};
    return {IgemmForm::ig2_64, false};
  }
  if (big) return {IgemmForm::ig4_128, true};
  const int nc = a.Cin / 64;                                   // 64-channel chunks
  const int groups = (3 * nc + a.ksplit - 1) / a.ksplit;       // (chunk, dy) groups of 3 K-steps per slice
  // 128-pixel x 32-channel halo tiles where the 64x64 tiles of the same launch are 224 ... 256 workgroups (the same count: same
  // tile area) and the K slices are whole 64-channel chunks, at least two of them (a one-chunk slice pays a whole slab fill before
  // its first MFMA).  ISHAP_IG4_HALO=0: the 64x64 / 128x64 choices below everywhere
  if (sw.ig4_halo && a.K2 == 0 && (a.W == 64 || a.W == 32 || a.W == 16) && a.M % 128 == 0 && (a.H * a.W) % 128 == 0 && a.N % 32 == 0 &&
      nc % a.ksplit == 0 && nc / a.ksplit >= 2) {
    const long long tiles = (long long)(a.M / 128) * (a.N / 32) * a.ksplit;
    if (tiles >= 224 && tiles <= 256) return {IgemmForm::ig4_halo, false};
  }
  // 128-pixel x 64-channel tiles (two image rows of a 64-wide map): for the 64^2 layers with >= 512 output channels the grid still
  // fills the chip (32 x 8 = 256 workgroups) and a K-step stages 13.3 KB for twice the FLOPs of a 64x64 tile's 10.7 KB; with only 128
  // such tiles (the 64^2 256->256 layers) it loses (0.1804 -> 0.182 s/shape): at least 224 tiles.  ISHAP_IG4_TEAMS=0: off
  if (sw.ig4_teams && a.W == 64 && a.K2 == 0 && a.ksplit == 1 && a.M % 128 == 0 && (a.H * a.W) % 128 == 0) {
    const long long tiles = (long long)(a.M / 128) * ((a.N + 63) / 64);
    if (tiles >= 224 && tiles <= 512) return {IgemmForm::ig4_tall, false};
  }
  // the 8x8 maps' sliced launches, whether or not the two-team test below would pass (no two-team instance for them)
  if (a.W == 8) return {IgemmForm::ig4_w8, false};
  // two teams: one workgroup per CU at most (<= 256 tiles) and a K slice long enough to halve (measured break-even: ~40 steps).
  // ISHAP_IG4_TEAMS other than 2: one team
  const long long tiles = (long long)(a.M / 64) * ((a.N + 63) / 64) * a.ksplit;
  if (sw.ig4_teams == 2 && tiles <= 256 && 3 * groups + a.K2 / 64 >= 48) return {IgemmForm::ig4_teams, false};
  // slices of 9-12 K-steps: too short for the 6-slot ring's compile-time loader path (13 steps), long enough for the 4-slot
  // ring's (9) -- -13 % per launch there (16^2 512->512 in 8 slices 7.7 -> 6.7 us, 32^2 256->512 in 4 slices 9.9 -> 8.6;
  // profiles/round4_igemm4_ring_by_slice_length_probe.txt); longer slices keep the deeper ring (+5 % at 36 steps with 4 slots)
  if (a.K2 == 0 && 3 * groups >= 9 && 3 * groups <= 12) return {IgemmForm::ig4_64_ring4, false};
  return {IgemmForm::ig4_64, false};
}

int igemm_prof_slot(const IgemmPlan& p, bool conv3) {
  // [form][conv3], forms in IgemmForm's order: skinny, reg32, ig2_128, ig2_64, ig2_teams, ig4_128, ig4_64, ig4_64_ring4, ig4_teams,
  // ig4_w8, ig4_tall, ig4_halo (the slot layout at ishap_profile_end)
  static const int slot[][2] = {{5, 5}, {6, 6}, {2, 0}, {3, 1}, {4, 4}, {8, 8}, {9, 9}, {9, 9}, {10, 10}, {11, 11}, {12, 12}, {7, 7}};
  static_assert(sizeof slot / sizeof slot[0] == (int)IgemmForm::ig4_halo + 1, "one row per form");
  return slot[(int)p.form][conv3];
}

template <bool CONV3>
static int launch_reg32(const IgemmArgs& a, hipStream_t s, std::string* name) {
  constexpr int BM = 64, BN = 64, BK = 32;
  if (name) { *name = igemm_kernel_name("igemm_kernel<%d, %d, %d, 2, 2, %s>", BM, BN, BK, CONV3 ? "true" : "false"); return 0; }
  constexpr size_t smem = 2 * (size_t)(BM + BN) * BK * sizeof(half_t);
  auto kern = igemm_kernel<BM, BN, BK, 2, 2, CONV3>;
  ISHAP_TRY(ishap_set_max_lds((const void*)kern, (int)smem));
  const dim3 grid(a.M / BM, ceil_div(a.N, BN), a.nbatch * a.ksplit);
  if (g_igemm_prof_start) hipExtLaunchKernelGGL(kern, grid, dim3(256), smem, s, g_igemm_prof_start, g_igemm_prof_stop, 0, a);
  else hipLaunchKernelGGL(kern, grid, dim3(256), smem, s, a);
  return 0;
}

int igemm_launch_main(const IgemmArgs& a, const IgemmPlan& p, hipStream_t s, std::string* name) {
  switch (p.form) {
    case IgemmForm::skinny: return igemm_skinny_launch(a, 0, s, name);
    case IgemmForm::reg32: return a.conv3 ? launch_reg32<true>(a, s, name) : launch_reg32<false>(a, s, name);
    case IgemmForm::ig2_128: case IgemmForm::ig2_64: case IgemmForm::ig2_teams: return igemm2_launch(a, p.form, s, name);
    default: return igemm4_launch(a, p.form, s, name);
  }
}

// the stand-alone reduce of deferred split-K slices (a.ws, a.ksplit, bias / residual / output fields as in the main launch)
int igemm_reduce_launch(const IgemmArgs& a, hipStream_t s) {
  ISHAP_REQUIRE(a.ksplit > 1 && a.ws && a.M % 16 == 0 && a.N % 4 == 0, "reduce: split-K slices of a finished launch");
  const unsigned rblocks = (unsigned)((long long)a.nbatch * (a.M / 16) * ((a.N + 63) / 64));
  hipLaunchKernelGGL(igemm_splitk_reduce, dim3(rblocks), dim3(256), 0, s, a);
  ISHAP_CHECK_HIP(hipGetLastError());
  return 0;
}

// what every launch must satisfy before it reaches a kernel (no HIP runtime call)
static int igemm_check(const IgemmArgs& a, const IgemmPlan& p) {
  ISHAP_REQUIRE(a.M % 64 == 0, "M must be a multiple of 64");
  ISHAP_REQUIRE(a.N % 4 == 0, "N must be a multiple of 4");
  ISHAP_REQUIRE(a.K % 32 == 0, "K must be a multiple of 32");
  ISHAP_REQUIRE(!a.conv3 || (a.Cin % 32 == 0 && a.K == 9 * a.Cin + a.K2), "conv3: K = 9*Cin (+ K2), Cin % 32 == 0");
  ISHAP_REQUIRE(a.K2 == 0 || (a.conv3 && a.X2 && a.K2 % 64 == 0 && a.Cin % 64 == 0 && a.ldx2 % 8 == 0 && a.nbatch == 1),
                "folded 1x1 source: 3x3 launch, 64-wide K-steps");
  ISHAP_REQUIRE(a.ksplit == 1 || a.ws != nullptr, "split-K needs a workspace");
  ISHAP_REQUIRE(!a.gb_x || (!a.stat_out && a.out_mode == IG_OUT_F16 && a.ldo == a.N && a.N % 32 == 0 && a.nbatch == 1 && a.gb_csums &&
                            a.gb_stats && a.gb_gamma && a.gb_beta && (!a.gb_film || a.gb_emb)),
                "fused GroupNorm-backward sums: fp16 dense output, N % 32 == 0, no forward statistics");
  ISHAP_REQUIRE(a.ldx % 8 == 0 && a.ldw % 8 == 0, "row strides must keep 16-byte alignment");
  ISHAP_REQUIRE(p.form == IgemmForm::skinny || !(a.stat_out || a.gb_x) || (a.H * a.W > 0 && (a.H * a.W) % 64 == 0),
                "fused GroupNorm sums need H*W to be a multiple of the 64-row tile");
  return 0;
}

int igemm_launch(const IgemmArgs& a, hipStream_t s) {
  const IgemmPlan p = igemm_plan(a);
  ISHAP_TRY(igemm_check(a, p));
  int prof_slot = -1;
  if (g_prof_on) {
    ProfRec r;
    r.a = prof_event(); r.b = prof_event(); r.c = nullptr;
    r.flops = 2.0 * a.M * a.N * a.K * a.nbatch * a.flops_scale;
    r.variant = igemm_prof_slot(p, a.conv3);
    r.M = a.M * a.nbatch; r.N = a.N; r.K = a.K; r.conv3 = a.conv3 != 0; r.big = p.big;
    r.ksplit = p.form == IgemmForm::skinny ? 0 : a.ksplit;    // ksplit 0 marks the skinny kernel
    g_igemm_prof_start = r.a; g_igemm_prof_stop = r.b;      // attached to the dispatch: kernel begin / end timestamps
    const int rc = igemm_launch_main(a, p, s);
    g_igemm_prof_start = nullptr; g_igemm_prof_stop = nullptr;
    if (rc) return rc;
    prof_slot = (int)g_prof.size();
    g_prof.push_back(r);
  } else {
    ISHAP_TRY(igemm_launch_main(a, p, s));
  }
  ISHAP_CHECK_HIP(hipGetLastError());
  if (a.ksplit > 1 && !a.defer_reduce) {
    ISHAP_TRY(igemm_reduce_launch(a, s));
    if (prof_slot >= 0) {
      g_prof[prof_slot].c = prof_event();
      (void)hipEventRecord(g_prof[prof_slot].c, s);
    }
  }
  return 0;
}

// CPU view of the plan (include/ishap.h): the K split conv_op picks and the kernel igemm_launch runs for one shape
extern "C" int ishap_igemm_plan(int M, int cin, int cout, int taps, int K2, int H, int W, int nbatch, int pending, int epilogue_sums,
                                int* ksplit, int* prof_slot, char* kernel, int kernel_cap) {
  static const half_t second_source = 0;         // the planner only asks whether a folded source is there
  static long long sums = 0;
  IgemmArgs a;
  a.M = M; a.N = cout; a.Cin = cin; a.K = taps * cin + K2; a.conv3 = taps == 9; a.K2 = K2; a.X2 = K2 ? &second_source : nullptr;
  a.H = H; a.W = W; a.nbatch = nbatch; a.stat_out = epilogue_sums ? &sums : nullptr;
  a.ksplit = igemm_plan_ksplit(a, pending != 0);
  const IgemmPlan p = igemm_plan(a);
  std::string name;
  ISHAP_TRY(igemm_launch_main(a, p, nullptr, &name));
  if (ksplit) *ksplit = a.ksplit;
  if (prof_slot) *prof_slot = igemm_prof_slot(p, a.conv3);
  if (kernel) {
    if ((int)name.size() + 1 > kernel_cap) return -2;
    memcpy(kernel, name.c_str(), name.size() + 1);
  }
  return 0;
}

// ---- a layer's launch as IgemmArgs: the one place the fields are filled, for the executor (unet.hip conv_op) and for the
// single-launch ABI below alike ----
int igemm_fill(const ConvLaunch& c, int chunk_tiles, IgemmArgs& a) {
  a = IgemmArgs{};
  a.stat_out = c.stat_out;
  if (const GnBwdArgs* gb = c.gb) {       // accumulate the GroupNorm-backward sums in this launch's epilogue
    a.gb_x = gb->x; a.gb_stats = gb->stats; a.gb_gamma = gb->gamma; a.gb_beta = gb->beta; a.gb_emb = gb->emb;
    a.gb_emb_ld = gb->emb_ld; a.gb_film = gb->film; a.gb_act = gb->act; a.gb_csums = gb->csums;
  }
  a.X = c.X; a.Wt = c.Wt; a.out = c.out; a.bias = c.bias; a.res = c.res;
  a.M = c.N * c.H * c.W; a.N = c.cout; a.K = c.taps * c.kpad + c.K2;
  a.X2 = c.X2; a.ldx2 = c.ldx2; a.K2 = c.K2; a.bias2 = c.bias2;
  a.conv3 = c.taps == 9; a.Cin = c.kpad;
  a.ldx = c.ldx; a.ldw = c.ldw ? c.ldw : c.taps * c.kpad; a.ldo = c.ldo; a.ldr = c.ldr;
  a.H = c.H; a.W = c.W; a.ups = c.ups; a.res_ups = c.res_ups;
  a.out_mode = c.out_mode; a.chunk_tiles = chunk_tiles;
  a.ksplit = igemm_plan_ksplit(a, c.pend_out != nullptr);
  if (c.pend_out && a.ksplit > 1) {
    ISHAP_REQUIRE(c.out_mode == IG_OUT_F16 && c.ldo == c.cout && !c.stat_out && !c.gb, "deferred reduce: dense fp16 output, no epilogue sums");
    a.defer_reduce = 1;
  }
  return 0;
}

IgemmArgs igemm_reduce_fill(const SlabSrc& p, int M, int N, int H, int W, void* out, int ldo) {
  IgemmArgs a;
  a.ws = const_cast<float*>(p.ws); a.ksplit = p.nslab; a.M = M; a.N = N; a.K = 64;
  a.bias = p.bias; a.bias2 = p.bias2; a.res = p.res; a.ldr = p.ldr; a.res_ups = p.res_ups;
  a.H = H; a.W = W; a.out = out; a.ldo = ldo; a.out_mode = IG_OUT_F16;
  return a;
}

// ---- one launch through the C ABI (include/ishap.h, ishap_igemm_run): the descriptor checked against the caller's buffer
// sizes, then the same fill, plan and launch a layer goes through ----

static bool desc_fits(const ishap_buf& b, long long bytes, int align) {
  return bytes <= 0 || (b.ptr && b.bytes >= bytes && ((unsigned long long)b.ptr % (unsigned)align) == 0);
}
#define DESC_BUF(buf, need, align, what)                                                                             \
  ISHAP_REQUIRE(desc_fits(d->buf, (need), (align)), std::string(what) + ": needs " + std::to_string((long long)(need)) + \
                " bytes at " #align "-byte alignment, has " + std::to_string(d->buf.bytes))

// Every extent the launch touches checked against the caller's byte sizes; the fields and the K split are igemm_fill's
// (nbatch = 1, alpha = 1, fp16 or NCHW fp32 output).  No HIP runtime call.
static int igemm_desc_args(const ishap_igemm_desc* d, IgemmArgs& a) {
  ISHAP_REQUIRE(d != nullptr, "descriptor");
  constexpr long long LIM = 1ll << 31;           // the kernels index each operand with 32-bit element offsets
  ISHAP_REQUIRE(d->taps == 1 || d->taps == 9, "taps: 1 (1x1) or 9 (3x3)");
  ISHAP_REQUIRE(d->M > 0 && d->N > 0 && d->Cin > 0 && d->H > 0 && d->W > 0 && d->K2 >= 0 && d->M < LIM / 8 && d->N < 65536 &&
                    d->H < 65536 && d->W < 65536,
                "extents");
  const long long HW = (long long)d->H * d->W;
  ISHAP_REQUIRE(d->M % HW == 0, "M = images * H * W");
  const long long nimg = d->M / HW;
  ISHAP_REQUIRE(d->out_mode == IG_OUT_F16 || d->out_mode == IG_OUT_NCHW_F32, "out_mode: fp16 rows or NCHW fp32");
  ISHAP_REQUIRE(!d->ups || (d->taps == 9 && d->H % 2 == 0 && d->W % 2 == 0), "ups: a 3x3 launch on an even map");
  ISHAP_REQUIRE(!d->res_ups || (d->res.ptr && d->H % 2 == 0 && d->W % 2 == 0), "res_ups: a residual on an even map");
  ISHAP_REQUIRE(d->K2 == 0 || d->taps == 9, "a folded second source rides on a 3x3 launch");
  ISHAP_REQUIRE(d->ldx >= d->Cin && d->ldx % 8 == 0, "ldx: >= Cin, a multiple of 8");
  ISHAP_REQUIRE(d->K2 == 0 || (d->ldx2 >= d->K2 && d->ldx2 % 8 == 0), "ldx2: >= K2, a multiple of 8");
  const long long K = (long long)d->taps * d->Cin + d->K2;
  ISHAP_REQUIRE(d->ldw >= K && d->ldw % 8 == 0, "ldw: >= taps * Cin + K2, a multiple of 8");
  ISHAP_REQUIRE(d->out_mode != IG_OUT_F16 || (d->ldo >= d->N && d->ldo % 4 == 0), "ldo: >= N, a multiple of 4");
  ISHAP_REQUIRE(!d->res.ptr || (d->ldr >= d->N && d->ldr % 4 == 0), "ldr: >= N, a multiple of 4");
  ISHAP_REQUIRE(d->chunk_tiles >= 0 && d->chunk_tiles % 8 == 0, "chunk_tiles: 0 or a multiple of 8");
  ISHAP_REQUIRE(!(d->stat_out.ptr && d->gb_x.ptr), "forward statistics and GroupNorm-backward sums are exclusive");
  ISHAP_REQUIRE(d->out_mode == IG_OUT_F16 || !(d->stat_out.ptr || d->gb_x.ptr), "epilogue sums need fp16 output");

  ConvLaunch c; GnBwdArgs gb; SlabSrc pend;      // what c.gb / c.pend_out point to
  c.X = (const half_t*)d->X.ptr; c.N = (int)nimg; c.H = d->H; c.W = d->W; c.ldx = d->ldx;
  c.Wt = (const half_t*)d->Wt.ptr; c.kpad = d->Cin; c.taps = d->taps; c.ldw = d->ldw;
  c.cout = d->N; c.bias = (const float*)d->bias.ptr;
  c.res = (const half_t*)d->res.ptr; c.ldr = d->ldr; c.res_ups = d->res_ups != 0;
  c.out = d->out.ptr; c.ldo = d->ldo; c.out_mode = d->out_mode;
  c.ups = d->ups != 0; c.stat_out = (long long*)d->stat_out.ptr;
  if (d->gb_x.ptr) {
    gb.x = (const half_t*)d->gb_x.ptr; gb.stats = (const float*)d->gb_stats.ptr; gb.gamma = (const float*)d->gb_gamma.ptr;
    gb.beta = (const float*)d->gb_beta.ptr; gb.emb = (const float*)d->gb_emb.ptr; gb.emb_ld = d->gb_emb_ld;
    gb.film = d->gb_film != 0; gb.act = d->gb_act != 0; gb.csums = (long long*)d->gb_csums.ptr;
    c.gb = &gb;
  }
  c.X2 = (const half_t*)d->X2.ptr; c.ldx2 = d->ldx2; c.K2 = d->K2; c.bias2 = (const float*)d->bias2.ptr;
  c.pend_out = d->pending ? &pend : nullptr;
  ISHAP_TRY(igemm_fill(c, d->chunk_tiles, a));
  a.ws = (float*)d->ws.ptr;

  // every extent the launch touches, in bytes
  const long long xrows = d->ups ? d->M / 4 : d->M, rrows = d->res_ups ? d->M / 4 : d->M;
  const long long npad = (d->N + 127) / 128 * 128;
  const long long xe = (xrows - 1) * d->ldx + d->Cin, x2e = (long long)(d->M - 1) * d->ldx2 + d->K2, we = npad * d->ldw;
  const long long oe = d->out_mode == IG_OUT_F16 ? (long long)(d->M - 1) * d->ldo + d->N : (long long)d->M * d->N;
  const long long re = (rrows - 1) * d->ldr + d->N, wse = a.ksplit > 1 ? (long long)a.ksplit * d->M * d->N : 0;
  ISHAP_REQUIRE(xe < LIM && x2e < LIM && we < LIM && oe < LIM && re < LIM && wse < LIM, "an operand beyond 2^31 elements");
  DESC_BUF(X, xe * 2, 16, "X");
  if (d->K2) DESC_BUF(X2, x2e * 2, 16, "X2");
  DESC_BUF(Wt, we * 2, 16, "Wt ([round_up(N, 128)][ldw])");
  DESC_BUF(out, oe * (d->out_mode == IG_OUT_F16 ? 2 : 4), 8, "out");
  if (d->res.ptr) DESC_BUF(res, re * 2, 8, "res");
  if (d->bias.ptr) DESC_BUF(bias, (long long)d->N * 4, 16, "bias");
  if (d->bias2.ptr) DESC_BUF(bias2, (long long)d->N * 4, 16, "bias2");
  DESC_BUF(ws, wse * 4, 16, "ws (K slices x M x N floats)");
  if (d->stat_out.ptr) DESC_BUF(stat_out, nimg * d->N * 16, 8, "stat_out ([images][N][2] int64)");
  if (d->gb_x.ptr) {
    ISHAP_REQUIRE(!d->gb_film || d->gb_emb_ld >= 2 * d->N, "gb_emb_ld: >= 2 N (scale, shift)");
    DESC_BUF(gb_x, (long long)d->M * d->N * 2, 16, "gb_x ([M][N] fp16)");
    DESC_BUF(gb_stats, nimg * 32 * 2 * 4, 4, "gb_stats ([images][32][2] float)");
    DESC_BUF(gb_gamma, (long long)d->N * 4, 4, "gb_gamma");
    DESC_BUF(gb_beta, (long long)d->N * 4, 4, "gb_beta");
    if (d->gb_film) DESC_BUF(gb_emb, ((nimg - 1) * d->gb_emb_ld + 2 * d->N) * 4, 4, "gb_emb");
    DESC_BUF(gb_csums, nimg * d->N * 16, 8, "gb_csums ([images][N][2] int64)");
  }
  return igemm_check(a, igemm_plan(a));
}

extern "C" int ishap_igemm_run(const ishap_igemm_desc* d, int launch, void* stream, int* ksplit, char* kernel, int kernel_cap) {
  IgemmArgs a;
  ISHAP_TRY(igemm_desc_args(d, a));
  std::string name;
  ISHAP_TRY(igemm_launch_main(a, igemm_plan(a), nullptr, &name));
  if (ksplit) *ksplit = a.ksplit;
  if (kernel) {
    if ((int)name.size() + 1 > kernel_cap) return -2;
    memcpy(kernel, name.c_str(), name.size() + 1);
  }
  return launch ? igemm_launch(a, (hipStream_t)stream) : 0;
}

extern "C" int ishap_igemm_reduce(const ishap_igemm_desc* d, int nslab, int launch, void* stream) {
  ISHAP_REQUIRE(d != nullptr, "descriptor");
  ISHAP_REQUIRE(nslab >= 2 && nslab <= 64, "nslab: the K slices of a deferred launch (2 .. 64)");
  ISHAP_REQUIRE(d->M > 0 && d->N > 0 && d->H > 0 && d->W > 0 && d->M % 16 == 0 && d->N % 4 == 0 && d->M < (1 << 28) && d->N < 65536 &&
                    d->H < 65536 && d->W < 65536 && d->M % ((long long)d->H * d->W) == 0,
                "M = images * H * W, a multiple of 16; N a multiple of 4");
  ISHAP_REQUIRE(d->out_mode == IG_OUT_F16 && d->ldo >= d->N && d->ldo % 4 == 0, "fp16 output, ldo >= N, a multiple of 4");
  ISHAP_REQUIRE(!d->res.ptr || (d->ldr >= d->N && d->ldr % 4 == 0), "ldr: >= N, a multiple of 4");
  ISHAP_REQUIRE(!d->res_ups || (d->res.ptr && d->H % 2 == 0 && d->W % 2 == 0), "res_ups: a residual on an even map");
  ISHAP_REQUIRE(!d->stat_out.ptr && !d->gb_x.ptr, "the stand-alone reduce adds no epilogue sums");
  const long long rrows = d->res_ups ? d->M / 4 : d->M;
  const long long oe = (long long)(d->M - 1) * d->ldo + d->N, re = (rrows - 1) * d->ldr + d->N, wse = (long long)nslab * d->M * d->N;
  ISHAP_REQUIRE(oe < (1ll << 31) && re < (1ll << 31) && wse < (1ll << 31), "an operand beyond 2^31 elements");
  DESC_BUF(out, oe * 2, 8, "out");
  if (d->res.ptr) DESC_BUF(res, re * 2, 8, "res");
  if (d->bias.ptr) DESC_BUF(bias, (long long)d->N * 4, 16, "bias");
  if (d->bias2.ptr) DESC_BUF(bias2, (long long)d->N * 4, 16, "bias2");
  DESC_BUF(ws, wse * 4, 16, "ws (K slices x M x N floats)");
  SlabSrc p;
  p.ws = (const float*)d->ws.ptr; p.nslab = nslab; p.bias = (const float*)d->bias.ptr; p.bias2 = (const float*)d->bias2.ptr;
  p.res = (const half_t*)d->res.ptr; p.ldr = d->ldr; p.res_ups = d->res_ups != 0;
  const IgemmArgs a = igemm_reduce_fill(p, d->M, d->N, d->H, d->W, d->out.ptr, d->ldo);
  return launch ? igemm_reduce_launch(a, (hipStream_t)stream) : 0;
}
