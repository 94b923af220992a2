/*
 * zb_policy_train.hip — backward pass of the GRU actor / critic (include/zbot_policy.h "Training",
 * DESIGN.md §4m): what get_ppo_variables differentiates (train.py:1683-1729). The training forward is
 * policy_kernel<..., SAVE = true> in zb_policy.hip; this file holds
 *
 *   head_kernel    the actor's mixture head backward, one thread per (t, env, joint);
 *   bptt_kernel    d h_top from the head gradient + backpropagation through time, one workgroup of 8 waves per 32
 *                  envs, persistent over t = T-1 .. 0 with the layers D-1 .. 0 inside and the
 *                  time-direction dh of every layer in registers between steps;
 *   wgrad_kernel   the parameter gradient as split-K A^T B products on the matrix cores;
 *   wreduce_kernel the fixed-order tree over the split-K partials;
 *   pack_kernel    natural-layout parameters -> fragment packs, on the device (zb_policy_set_params).
 *
 * bptt_kernel keeps the forward's ownership map: wave w owns units 16 w .. 16 w + 15 of every layer
 * for both 16-env row tiles, lane l holds unit 16 w + (l & 15) of envs crow(et, v, l), which is also
 * the C / D map of v_mfma_f32_16x16x4_f32. Per layer, with dh' = dx from the layer above + dh from
 * step t + 1:
 *   dn = dh' (1 - z)   dz = dh' (h - n)   dh = dh' z
 *   da_n = dn (1 - n^2)   da_z = dz z (1 - z)   da_r = da_n (W_hn h + b_n) r (1 - r)
 *   dgi = [da_r, da_z, da_n]   dgh = [da_r, da_z, da_n r]
 *   dx = dgi W_ih (to the layer below)   dh += dgh W_hh (to step t - 1; zero where reset[t][e])
 * The four gradient rows (da_r, da_z, da_n, da_n r) go k-major into LDS ([512][env]) as the A operand
 * of the two transposed products (K = 384 each; the first 256 k are shared, so one LDS read feeds
 * both), and to the scratch plane dg for wgrad_kernel. B operands are fragment packs of W_ih^T and
 * W_hh^T, built with the forward's packs.
 *
 * Reduction order of the parameter gradient: include/zbot_policy.h.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include "zb_internal.h"
#include "zbot_fmath.h"

namespace zb {
namespace ptr {

constexpr int H = ZB_POL_HIDDEN;
constexpr int D = ZB_POL_DEPTH;
constexpr int MT = 16;
constexpr int NET = 2;
constexpr int M = MT * NET;  /* envs per workgroup */
constexpr int NWAVE = H / 16;
constexpr int NTHR = 64 * NWAVE;
constexpr int LDA = M + 1;
constexpr int NJ = ZB_POL_JOINTS;
constexpr int NMIX = ZB_POL_MIX;
constexpr int G3 = 3 * H / 16;               /* 4-step groups over K = 3H */
constexpr int RAWP = ZB_TR_RAW_LD;           /* 300 padded to a multiple of 16 */
constexpr size_t MATT = (size_t)NWAVE * G3 * 64; /* one packed [H][3H] transposed matrix, float4 */
static_assert(RAWP % 16 == 0 && RAWP >= ZB_POL_ACTOR_OUT, "padded head width");
static_assert(ZB_TR_DG_LD == 4 * H, "four gradient rows per unit");

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int crow(int et, int v, int l) { return MT * et + 4 * (l >> 4) + v; }
__device__ __forceinline__ f32x4 mma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float q4(const float4& v, int u) {
  return u == 0 ? v.x : (u == 1 ? v.y : (u == 2 ? v.z : v.w));
}

/* Head backward of one (env, joint) (train.py:952-965): with p = softmax(logits), v_m = log p_m +
   log N(act; mu_m, sd_m) and w = softmax(v) as in zbf_mix_log_prob,
     d lp / d logit_m = w_m - p_m     d lp / d mu_m = w_m (act - mu_m) / sd_m^2
     d lp / d sd_m = w_m (z_m^2 - 1) / sd_m,  d sd / d raw = sigmoid(raw) below the max_std clip, else 0.
   o: the env's 300 raw outputs; g: the upstream d_log_prob. Writes the 15 gradients to dr (the env's
   row of the d raw plane). It runs as a kernel of its own over every (t, env, joint) before
   bptt_kernel: the rows do not depend on each other, so the transcendentals stay off the persistent
   loop's critical path. */
__device__ __forceinline__ void mix_head_grad(const float* o, float mb, float g, float act, int j, float* dr) {
  float mu[NMIX], sd[NMIX], lg[NMIX], sraw[NMIX];
  bool open[NMIX];
#pragma unroll
  for (int m = 0; m < NMIX; ++m) {
    mu[m] = o[j * NMIX + m] + mb;
    sraw[m] = o[NJ * NMIX + j * NMIX + m];
    const float s = (zbf_softplus(sraw[m]) + 0.01f) * 1.0f;
    open[m] = s < 1.0f; /* below the max_std clip (train.py:961) */
    sd[m] = open[m] ? s : 1.0f;
    lg[m] = o[2 * NJ * NMIX + j * NMIX + m];
  }
  float mx = lg[0];
#pragma unroll
  for (int m = 1; m < NMIX; ++m) mx = lg[m] > mx ? lg[m] : mx;
  float pe[NMIX], Ssum = 0.f;
#pragma unroll
  for (int m = 0; m < NMIX; ++m) {
    pe[m] = zbf_exp(lg[m] - mx);
    Ssum = Ssum + pe[m];
  }
  const float logS = zbf_log(Ssum);
  float vv[NMIX], zz[NMIX], Mx = -3.0e38f;
#pragma unroll
  for (int m = 0; m < NMIX; ++m) {
    zz[m] = (act - mu[m]) / sd[m];
    const float lnm = ((-0.5f * zz[m]) * zz[m] - zbf_log(sd[m])) - ZBF_HALF_LOG_2PI;
    vv[m] = ((lg[m] - mx) - logS) + lnm;
    Mx = vv[m] > Mx ? vv[m] : Mx;
  }
  float we[NMIX], acc = 0.f;
#pragma unroll
  for (int m = 0; m < NMIX; ++m) {
    we[m] = zbf_exp(vv[m] - Mx);
    acc = acc + we[m];
  }
#pragma unroll
  for (int m = 0; m < NMIX; ++m) {
    const float wm = we[m] / acc;
    const float dlg = g * (wm - pe[m] / Ssum);
    const float dmu = g * (wm * (zz[m] / sd[m]));
    const float dsr = open[m] ? g * (wm * ((zz[m] * zz[m] - 1.0f) / sd[m])) * zbf_sigmoid(sraw[m]) : 0.f;
    dr[j * NMIX + m] = dmu;
    dr[NJ * NMIX + j * NMIX + m] = dsr;
    dr[2 * NJ * NMIX + j * NMIX + m] = dlg;
  }
}

__global__ __launch_bounds__(256) void head_kernel(PolicyBwdArgs a) {
#pragma clang fp contract(off)
  const TrainLayout tl = train_layout(ZB_POL_ACTOR, a.T, a.n);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= tl.K * NJ) return;
  const size_t row = i / NJ;
  const int j = (int)(i - row * NJ);
  const float* mean_bias = a.bias + H + (size_t)D * 4 * H + ZB_POL_ACTOR_OUT;
  mix_head_grad(a.scratch + tl.raw + row * RAWP, mean_bias[j], a.dout[i], a.actions[i], j,
                a.scratch + tl.draw + row * RAWP);
}

/* The same head backward over nm <= ZB_POL_MAX_MIX components (shaped handles): the operations and their
   order are mix_head_grad's with nm in place of NMIX, the loops run over the maximum behind a guard so
   that they unroll and the arrays stay in registers. At nm = 5 the bits are mix_head_grad's. */
__device__ __forceinline__ void mix_head_grad_n(const float* o, float mb, float g, float act, int j, int nm,
                                                float* dr) {
  constexpr int MM = ZB_POL_MAX_MIX;
  float mu[MM], sd[MM], lg[MM], sraw[MM];
  bool open[MM];
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    mu[m] = sd[m] = lg[m] = sraw[m] = 0.f;
    open[m] = false;
    if (m >= nm) continue;
    mu[m] = o[j * nm + m] + mb;
    sraw[m] = o[NJ * nm + j * nm + m];
    const float s = (zbf_softplus(sraw[m]) + 0.01f) * 1.0f;
    open[m] = s < 1.0f;
    sd[m] = open[m] ? s : 1.0f;
    lg[m] = o[2 * NJ * nm + j * nm + m];
  }
  float mx = lg[0];
#pragma unroll
  for (int m = 1; m < MM; ++m)
    if (m < nm) mx = lg[m] > mx ? lg[m] : mx;
  float pe[MM], Ssum = 0.f;
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    pe[m] = 0.f;
    if (m >= nm) continue;
    pe[m] = zbf_exp(lg[m] - mx);
    Ssum = Ssum + pe[m];
  }
  const float logS = zbf_log(Ssum);
  float vv[MM], zz[MM], Mx = -3.0e38f;
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    vv[m] = zz[m] = 0.f;
    if (m >= nm) continue;
    zz[m] = (act - mu[m]) / sd[m];
    const float lnm = ((-0.5f * zz[m]) * zz[m] - zbf_log(sd[m])) - ZBF_HALF_LOG_2PI;
    vv[m] = ((lg[m] - mx) - logS) + lnm;
    Mx = vv[m] > Mx ? vv[m] : Mx;
  }
  float we[MM], acc = 0.f;
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    we[m] = 0.f;
    if (m >= nm) continue;
    we[m] = zbf_exp(vv[m] - Mx);
    acc = acc + we[m];
  }
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    if (m >= nm) continue;
    const float wm = we[m] / acc;
    const float dlg = g * (wm - pe[m] / Ssum);
    const float dmu = g * (wm * (zz[m] / sd[m]));
    const float dsr = open[m] ? g * (wm * ((zz[m] * zz[m] - 1.0f) / sd[m])) * zbf_sigmoid(sraw[m]) : 0.f;
    dr[j * nm + m] = dmu;
    dr[NJ * nm + j * nm + m] = dsr;
    dr[2 * NJ * nm + j * nm + m] = dlg;
  }
}

__global__ __launch_bounds__(256) void head_kernel_n(PolicyBwdArgsG a) {
#pragma clang fp contract(off)
  const TrainLayout tl = train_layout_shaped(ZB_POL_ACTOR, a.depth, a.nmix, a.T, a.n);
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= tl.K * NJ) return;
  const size_t row = i / NJ;
  const int j = (int)(i - row * NJ);
  const int rawp = policy_raw_ld(a.nmix);
  const float* mean_bias = a.bias + H + (size_t)a.depth * 4 * H + 3 * NJ * a.nmix;
  mix_head_grad_n(a.scratch + tl.raw + row * rawp, mean_bias[j], a.dout[i], a.actions[i], j, a.nmix,
                  a.scratch + tl.draw + row * rawp);
}

/* GEN: the shape-generic instantiation (a.depth layers, a.nmix mixtures). It hands the time-direction
   gradient of every layer to step t - 1 through the scratch plane TrainLayout::dht, each thread reading
   back the 8 values it wrote, where GEN = false holds them in registers; the arithmetic is the same. */
template <bool GEN>
struct BArgs { typedef PolicyBwdArgs type; };
template <>
struct BArgs<true> { typedef PolicyBwdArgsG type; };
__device__ __forceinline__ constexpr int arg_depth(const PolicyBwdArgs&) { return D; }
__device__ __forceinline__ int arg_depth(const PolicyBwdArgsG& a) { return a.depth; }
__device__ __forceinline__ constexpr int arg_nmix(const PolicyBwdArgs&) { return NMIX; }
__device__ __forceinline__ int arg_nmix(const PolicyBwdArgsG& a) { return a.nmix; }

template <bool ACTOR, bool GEN = false>
__global__ __launch_bounds__(NTHR) void bptt_kernel(typename BArgs<GEN>::type a) {
  constexpr int NOUT = ACTOR ? ZB_POL_ACTOR_OUT : 1;
  const int Dn = arg_depth(a), nmix = arg_nmix(a);
  const int nout = GEN && ACTOR ? 3 * NJ * nmix : NOUT;
  const int rawp = GEN ? policy_raw_ld(nmix) : RAWP;
  const int go = rawp / 16;
  __shared__ float sg[4 * H * LDA];  /* [da_r | da_z | da_n | da_n r][unit][env]; first the actor's d raw [c][env] */
  __shared__ float sdx[H * LDA];     /* dx from the layer above [unit][env] */
  static_assert(RAWP <= 4 * H, "the head gradient tile fits the gate gradient tile");
  static_assert(3 * ZB_POL_JOINTS * ZB_POL_MAX_MIX <= 4 * H, "and so does the widest shaped head");

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c16 = lane & 15, k4 = lane >> 4;
  const int unit = 16 * w + c16;
  const int e0 = blockIdx.x * M;
  const TrainLayout tl = GEN ? train_layout_shaped(ACTOR ? ZB_POL_ACTOR : ZB_POL_CRITIC, Dn, nmix, a.T, a.n)
                             : train_layout(ACTOR ? ZB_POL_ACTOR : ZB_POL_CRITIC, a.T, a.n);
  const float4* wt4 = reinterpret_cast<const float4*>(a.wpack_t);
  const float* tail = a.bias + H + (size_t)Dn * 4 * H; /* output bias [nout], then head constants */
  float* S = a.scratch;

  constexpr int DR = GEN ? 1 : D;
  [[maybe_unused]] float dht[DR][NET][4]; /* d loss / d carry handed to step t - 1, per layer */
#pragma unroll
  for (int l = 0; l < DR; ++l)
#pragma unroll
    for (int et = 0; et < NET; ++et)
#pragma unroll
      for (int v = 0; v < 4; ++v) dht[l][et][v] = 0.f;

  for (int t = a.T - 1; t >= 0; --t) {
    const size_t row0 = (size_t)t * a.n + e0;
    /* 1. head backward -> sdx = d loss / d h_top [unit][env] */
    if constexpr (ACTOR) {
      /* the step's d raw rows (head_kernel) -> sg [c][env], zero past the 300 outputs and the last env */
#pragma unroll 1
      for (int i = tid; i < M * rawp; i += NTHR) {
        const int e = i / rawp, c = i - e * rawp;
        sg[c * LDA + e] = (e0 + e < a.n && c < nout) ? S[tl.draw + (row0 + e) * rawp + c] : 0.f;
      }
      __syncthreads();
      /* d h_top = d raw [32][300] W_out [300][128]: this wave's 16 units */
      {
        const float4* wo = wt4 + (size_t)Dn * 2 * MATT + (size_t)w * go * 64 + lane;
        f32x4 acc[NET];
#pragma unroll
        for (int et = 0; et < NET; ++et) acc[et] = f32x4{0.f, 0.f, 0.f, 0.f};
        float4 b = wo[0];
#pragma unroll 1
        for (int g = 0; g < go; ++g) {
          const float4 bn = wo[(size_t)(g + 1 < go ? g + 1 : g) * 64];
          const float* xp = sg + (16 * g + k4) * LDA + c16;
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int et = 0; et < NET; ++et) acc[et] = mma(xp[4 * u * LDA + MT * et], q4(b, u), acc[et]);
          b = bn;
        }
#pragma unroll
        for (int et = 0; et < NET; ++et)
#pragma unroll
          for (int v = 0; v < 4; ++v) sdx[unit * LDA + crow(et, v, lane)] = acc[et][v];
      }
    } else {
      const float wu = tail[nout + unit]; /* value head W_out [H] */
#pragma unroll
      for (int et = 0; et < NET; ++et)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int e = crow(et, v, lane);
          sdx[unit * LDA + e] = e0 + e < a.n ? a.dout[row0 + e] * wu : 0.f;
        }
    }
    __syncthreads(); /* the head's reads of sg are done; sdx is written by its own readers only */

    /* 2. layers D-1 .. 0 */
    /* not unrolled: five copies of the layer body cost the actor 16 to 23 spilled registers */
#pragma unroll 1
    for (int l = Dn - 1; l >= 0; --l) {
      float dhd[NET][4];
#pragma unroll
      for (int et = 0; et < NET; ++et)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int e = crow(et, v, lane);
          const bool live = e0 + e < a.n;
          float dt;
          if constexpr (GEN) {
            /* what this thread stored for (layer l, env, unit) at step t + 1; nothing comes from past the end */
            dt = (live && t < a.T - 1) ? S[tl.dht + ((size_t)l * a.n + e0 + e) * H + unit] : 0.f;
          } else {
            dt = dht[0][et][v];
#pragma unroll
            for (int k = 1; k < D; ++k) dt = l == k ? dht[k][et][v] : dt;
          }
          const float dhp = sdx[unit * LDA + e] + dt;
          float r = 0.f, z = 0.f, nn = 0.f, hn = 0.f, hp = 0.f;
          const size_t i = ((size_t)l * tl.K + row0 + e) * H + unit;
          if (live) {
            r = S[tl.r + i];
            z = S[tl.z + i];
            nn = S[tl.nn + i];
            hn = S[tl.hn + i];
            hp = S[tl.hp + i];
          }
          const float dn = dhp * (1.0f - z), dz = dhp * (hp - nn);
          dhd[et][v] = dhp * z;
          const float dan = dn * (1.0f - nn * nn);
          const float daz = dz * (z * (1.0f - z));
          const float dar = (dan * hn) * (r * (1.0f - r));
          const float danr = dan * r;
          sg[unit * LDA + e] = dar;
          sg[(H + unit) * LDA + e] = daz;
          sg[(2 * H + unit) * LDA + e] = dan;
          sg[(3 * H + unit) * LDA + e] = danr;
          if (live) {
            float* dg = S + tl.dg + ((size_t)l * tl.K + row0 + e) * ZB_TR_DG_LD + unit;
            dg[0] = dar;
            dg[H] = daz;
            dg[2 * H] = dan;
            dg[3 * H] = danr;
          }
        }
      __syncthreads();
      /* dx = dgi W_ih, dh = dgh W_hh for this wave's units: K = 3H, k < 2H shared */
      const float4* wih = wt4 + (size_t)l * 2 * MATT + (size_t)w * G3 * 64 + lane;
      const float4* whh = wih + MATT;
      f32x4 ax[NET], ah[NET];
#pragma unroll
      for (int et = 0; et < NET; ++et) ax[et] = ah[et] = f32x4{0.f, 0.f, 0.f, 0.f};
      float4 bi = wih[0], bh = whh[0];
      for (int g = 0; g < G3; ++g) {
        const size_t gn = (size_t)(g + 1 < G3 ? g + 1 : g) * 64;
        const float4 ni = wih[gn], nh = whh[gn];
        const float* xp = sg + (16 * g + k4) * LDA + c16;
        const float* hq = g < 2 * H / 16 ? xp : xp + H * LDA; /* da_n r sits one H block after da_n */
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int et = 0; et < NET; ++et) {
            ax[et] = mma(xp[4 * u * LDA + MT * et], q4(bi, u), ax[et]);
            ah[et] = mma(hq[4 * u * LDA + MT * et], q4(bh, u), ah[et]);
          }
        bi = ni;
        bh = nh;
      }
#pragma unroll
      for (int et = 0; et < NET; ++et)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int e = crow(et, v, lane), ge = e0 + e;
          if (l > 0)
            sdx[unit * LDA + e] = ax[et][v];
          else if (ge < a.n)
            S[tl.dx0 + (row0 + e) * H + unit] = ax[et][v];
          const bool cut = ge >= a.n || (a.reset && a.reset[(size_t)t * a.n + ge]);
          const float nd = cut ? 0.f : dhd[et][v] + ah[et][v];
          if constexpr (GEN) {
            if (ge < a.n) S[tl.dht + ((size_t)l * a.n + ge) * H + unit] = nd;
          } else {
#pragma unroll
            for (int k = 0; k < D; ++k) dht[k][et][v] = l == k ? nd : dht[k][et][v];
          }
        }
      __syncthreads(); /* sg is free for the next layer, sdx holds its upstream */
    }
  }
}

/* ---------------------------------------------------------------------------------------------
 * Parameter gradient: every weight gradient is C [Mr][Nc] = sum over rows k of A[k][Mr] (x) B[k][Nc]
 * with A a gradient plane and B the matching activation plane, and every bias gradient is a column
 * sum of A (a product against ones, accumulated in fp64: v_mfma_f64_16x16x4_f64). One wave computes one 64 x 64 tile of C for
 * one chunk of rows, 4 rows an MFMA step, straight from global memory (both operands are read along
 * their rows, 64 B per 16 lanes), and writes it at the parameter's natural-layout place in the
 * chunk's partial vector. A chunk longer than 512 rows is summed as sub-chains of 512 rows added in
 * order: at K = 204 800 one 6 400-row chain per chunk measured 10x the fp32 torch error against fp64
 * (1.6e-5 of the largest gradient entry), the chain length showing in the rounding.
 * ------------------------------------------------------------------------------------------- */
struct WJob {
  const float* A;
  const float* B;
  int lda, ldb, Mr, Nc;
  long long out;   /* offset of C[0][0] in the parameter vector (row stride Nc) */
  long long bias;  /* offset of the column sums of A, or -1 */
  int tile0, ntn;  /* first tile of this job, tiles along Nc */
};
constexpr int MAXJOB = 3 * D + 2;
constexpr int MAXJOB_GEN = 3 * ZB_POL_MAX_DEPTH + 2; /* the job list of the deepest shaped handle */
constexpr int WSUB = 512; /* rows of one fp32 chain (a multiple of 16) */
template <int MJ>
struct WArgsT {
  WJob job[MJ];
  int njob;
  long long K;
  int chunk_rows;
  long long pc;    /* parameter count */
  float* part;
};
typedef WArgsT<MAXJOB> WArgs;

/* MJ: the capacity of the job list passed by value: MAXJOB at the default shape, MAXJOB_GEN for shaped handles */
template <int MJ>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void wgrad_kernel(WArgsT<MJ> wa) {
  const int lane = threadIdx.x, c16 = lane & 15, k4 = lane >> 4;
  int ji = 0;
  for (int i = 1; i < wa.njob; ++i) ji = (int)blockIdx.x >= wa.job[i].tile0 ? i : ji;
  const WJob jb = wa.job[ji];
  const int tile = blockIdx.x - jb.tile0;
  const int m0 = 64 * (tile / jb.ntn), n0 = 64 * (tile % jb.ntn);
  const long long k0 = (long long)blockIdx.y * wa.chunk_rows;
  const long long k1 = k0 + wa.chunk_rows < wa.K ? k0 + wa.chunk_rows : wa.K;
  const bool with_bias = jb.bias >= 0 && n0 == 0;

  int ca[4], cb[4];
  bool va[4], vb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + 16 * i + c16, n = n0 + 16 * i + c16;
    va[i] = m < jb.Mr;
    vb[i] = n < jb.Nc;
    ca[i] = va[i] ? m : 0;
    cb[i] = vb[i] ? n : 0;
  }
  float* P = wa.part + (size_t)blockIdx.y * wa.pc;
  /* the chunk's rows in sub-chains of WSUB: each a chain from 0, their sums added in order into the
     chunk's partial (this wave's own elements), so no fp32 chain is longer than WSUB rows */
  long long ks = k0;
  bool first = true;
  /* column sums of A (the bias gradients): ones (x) A in fp64 on the matrix cores, one chain over the
     whole chunk. Every row of the product holds the sums, column c16 that of m0 + 16 i + c16. In fp32
     chains these sums of signed terms lost the most against their own size (9x the fp32 torch error
     at K = 16 500). */
  f64x4 accs[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) accs[i] = f64x4{0.0, 0.0, 0.0, 0.0};
  do {
  const long long ke = ks + WSUB < k1 ? ks + WSUB : k1;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long k = ks; k < ke; k += 16) {
    float av[4][4], bv[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long kr = k + 4 * u + k4;
      const bool vk = kr < ke;
      const long long kk = vk ? kr : k0; /* a row of this chunk: always in bounds */
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float x = jb.A[kk * jb.lda + ca[i]], y = jb.B[kk * jb.ldb + cb[i]];
        av[u][i] = vk && va[i] ? x : 0.f;
        bv[u][i] = vk && vb[i] ? y : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mma(av[u][i], bv[u][j], acc[i][j]);
      if (with_bias) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          accs[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(1.0, (double)av[u][i], accs[i], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = m0 + 16 * i + 4 * k4 + v;
      if (m >= jb.Mr) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + c16;
        if (n < jb.Nc) {
          float* q = P + jb.out + (long long)m * jb.Nc + n;
          *q = first ? acc[i][j][v] : *q + acc[i][j][v];
        }
      }
    }
  first = false;
  ks += WSUB;
  } while (ks < k1);
  if (with_bias && k4 == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (va[i]) P[jb.bias + m0 + 16 * i + c16] = (float)accs[i][0];
  }
}

/* grad[i] = the fixed tree over the chunk partials (include/zbot_policy.h); the constant tail is 0 */
__global__ __launch_bounds__(256) void wreduce_kernel(const float* part, int chunks, long long pc, long long nlive,
                                                      float* grad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pc) return;
  float p[ZB_TR_MAX_CHUNKS];
#pragma unroll
  for (int c = 0; c < ZB_TR_MAX_CHUNKS; ++c) p[c] = c < chunks && i < nlive ? part[(size_t)c * pc + i] : 0.f;
#pragma unroll
  for (int s = ZB_TR_MAX_CHUNKS / 2; s >= 1; s >>= 1)
#pragma unroll
    for (int c = 0; c < s; ++c) p[c] = p[c] + p[c + s];
  grad[i] = p[0];
}

/* out = B fragments of the logical matrix Bm [N][K] (zb_capi.cpp pack_b): Bm[row][k] = W[row * K + k], or
   for the transposed packs W[k * N + row] with W the natural [K][N] matrix */
__global__ __launch_bounds__(256) void pack_kernel(const float* W, int N, int K, int trans, float* out) {
  const int G = (K + 15) / 16, NT = (N + 15) / 16;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)NT * G * 256) return;
  const int u = (int)(i & 3), l = (int)((i >> 2) & 63);
  const long long tg = i >> 8;
  const int g = (int)(tg % G), t = (int)(tg / G);
  const int row = 16 * t + (l & 15), k = 16 * g + 4 * u + (l >> 4);
  float v = 0.f;
  if (row < N && k < K) v = trans ? W[(size_t)k * N + row] : W[(size_t)row * K + k];
  out[i] = v;
}

}  // namespace ptr

static size_t pack_words(int N, int K) { return (size_t)((N + 15) / 16) * ((K + 15) / 16) * 256; }

hipError_t launch_policy_pack(int kind, int depth, int nmix, const float* params, float* wpack, float* wpack_t,
                              float* bias, hipStream_t s) {
  const int H = ZB_POL_HIDDEN, D = depth;
  const int I = kind == ZB_POL_ACTOR ? ZB_POL_ACTOR_IN : ZB_POL_CRITIC_IN;
  const int O = kind == ZB_POL_ACTOR ? 3 * ZB_POL_JOINTS * nmix : 1;
  auto pack = [&](const float* W, int N, int K, int trans, float* out) {
    const size_t words = pack_words(N, K);
    hipLaunchKernelGGL(ptr::pack_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, W, N, K, trans, out);
    return words;
  };
  auto copy = [&](float* dst, const float* src, size_t nfl) {
    return hipMemcpyAsync(dst, src, nfl * sizeof(float), hipMemcpyDeviceToDevice, s);
  };
  hipError_t e = hipSuccess;
  const float* p = params;
  float *wp = wpack, *wt = wpack_t, *b = bias;
  wp += pack(p, H, I, 0, wp);
  p += (size_t)H * I;
  if ((e = copy(b, p, H)) != hipSuccess) return e;
  b += H, p += H;
  for (int l = 0; l < D; l++) {
    for (int m = 0; m < 2; m++) { /* weight_ih, weight_hh */
      wp += pack(p, 3 * H, H, 0, wp);
      wt += pack(p, H, 3 * H, 1, wt);
      p += (size_t)3 * H * H;
    }
    if ((e = copy(b, p, 4 * H)) != hipSuccess) return e;
    b += 4 * H, p += 4 * H;
  }
  const float* wout = p;
  p += (size_t)O * H;
  if ((e = copy(b, p, O)) != hipSuccess) return e;
  b += O, p += O;
  if (kind == ZB_POL_ACTOR) {
    pack(wout, O, H, 0, wp);
    pack(wout, H, O, 1, wt);
    e = copy(b, p, ZB_POL_JOINTS);
  } else {
    e = copy(b, wout, H);
  }
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

template <int MJ>
static hipError_t policy_backward(int kind, const PolicyBwdArgsG& a, hipStream_t s) {
  constexpr bool GEN = MJ != ptr::MAXJOB;
  const int H = ZB_POL_HIDDEN, D = GEN ? a.depth : ZB_POL_DEPTH;
  const int I = kind == ZB_POL_ACTOR ? ZB_POL_ACTOR_IN : ZB_POL_CRITIC_IN;
  const int O = kind == ZB_POL_ACTOR ? (GEN ? 3 * ZB_POL_JOINTS * a.nmix : ZB_POL_ACTOR_OUT) : 1;
  const int rawld = GEN ? policy_raw_ld(a.nmix) : ZB_TR_RAW_LD;
  const TrainLayout tl = GEN ? train_layout_shaped(kind, a.depth, a.nmix, a.T, a.n) : train_layout(kind, a.T, a.n);
  const int nblk = (a.n + ptr::M - 1) / ptr::M;
  if (kind == ZB_POL_ACTOR) {
    const size_t items = tl.K * ZB_POL_JOINTS;
    if (GEN)
      hipLaunchKernelGGL(ptr::head_kernel_n, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(ptr::head_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, (const PolicyBwdArgs&)a);
    hipLaunchKernelGGL((ptr::bptt_kernel<true, GEN>), dim3(nblk), dim3(ptr::NTHR), 0, s, (const typename ptr::BArgs<GEN>::type&)a);
  } else
    hipLaunchKernelGGL((ptr::bptt_kernel<false, GEN>), dim3(nblk), dim3(ptr::NTHR), 0, s, (const typename ptr::BArgs<GEN>::type&)a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;

  ptr::WArgsT<MJ> wa;
  memset(&wa, 0, sizeof wa);
  float* S = a.scratch;
  const size_t KH = tl.K * H;
  int nj = 0, tiles = 0;
  long long off = 0;
  auto add = [&](const float* A, int lda, const float* B, int ldb, int Mr, int Nc, long long out, long long bias) {
    ptr::WJob& j = wa.job[nj++];
    j.A = A, j.B = B, j.lda = lda, j.ldb = ldb, j.Mr = Mr, j.Nc = Nc, j.out = out, j.bias = bias;
    j.tile0 = tiles;
    j.ntn = (Nc + 63) / 64;
    tiles += ((Mr + 63) / 64) * j.ntn;
  };
  /* input_proj.weight [H][I], bias [H]: A = d x0, B = obs */
  add(S + tl.dx0, H, a.obs, I, H, I, off, off + (long long)H * I);
  off += (long long)H * I + H;
  for (int l = 0; l < D; l++) {
    const float* dg = S + tl.dg + (size_t)l * tl.K * ZB_TR_DG_LD;
    const float* x = l == 0 ? S + tl.x0 : S + tl.ho + (size_t)(l - 1) * KH;
    const float* hp = S + tl.hp + (size_t)l * KH;
    const long long wih = off, whh = off + 3LL * H * H, bo = off + 6LL * H * H;
    add(dg, ZB_TR_DG_LD, x, H, 3 * H, H, wih, bo);                                    /* weight_ih, bias = sum dgi */
    add(dg, ZB_TR_DG_LD, hp, H, 2 * H, H, whh, -1);                                   /* weight_hh rows r, z */
    add(dg + 3 * H, ZB_TR_DG_LD, hp, H, H, H, whh + 2LL * H * H, bo + 3 * H);         /* rows n; bias_n = sum da_n r */
    off += 6LL * H * H + 4 * H;
  }
  const float* top = S + tl.ho + (size_t)(D - 1) * KH;
  if (kind == ZB_POL_ACTOR)
    add(S + tl.draw, rawld, top, H, O, H, off, off + (long long)O * H);
  else
    add(a.dout, 1, top, H, 1, H, off, off + H);
  off += (long long)O * H + O;
  wa.njob = nj;
  wa.K = (long long)tl.K;
  wa.chunk_rows = tl.chunk_rows;
  wa.pc = (long long)(GEN ? policy_param_count_shaped(kind, a.depth, a.nmix) : policy_param_count(kind));
  wa.part = S + tl.part;
  hipLaunchKernelGGL(ptr::wgrad_kernel<MJ>, dim3(tiles, tl.chunks), dim3(64), 0, s, wa);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(ptr::wreduce_kernel, dim3((unsigned)((wa.pc + 255) / 256)), dim3(256), 0, s,
                     (const float*)wa.part, tl.chunks, wa.pc, off, a.grad);
  return hipGetLastError();
}

hipError_t launch_policy_backward(int kind, const PolicyBwdArgsG& a, hipStream_t s) {
  if (a.generic) return policy_backward<ptr::MAXJOB_GEN>(kind, a, s);
  return policy_backward<ptr::MAXJOB>(kind, a, s);
}

}  // namespace zb
