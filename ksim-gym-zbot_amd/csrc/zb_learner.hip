/*
 * zb_learner.hip — the three steps of a PPO optimizer step around the networks' backward pass:
 * loss seeds and sums, the squared gradient norm, and AdamW behind the global-norm clip.
 * C ABI: include/zbot_ppo.h "Learner". Element arithmetic: include/zbot_learner_math.h, shared
 * source-identical with the host twins in zb_host.cpp; results are bit-identical to them.
 *
 * All three are launch-latency bound (a few MB at train.py's minibatch), so the kernels are plain:
 *
 *   ppo_loss_kernel  one workgroup = 256 rows. The rows' 2 x 20 log-probs (80 contiguous bytes a
 *                    row) stream in as 16-B loads along the joint axis into LDS (row stride 21
 *                    words: a thread per row then reads conflict-free); one thread per row sums
 *                    its 20 joints in order, runs zbl_loss_row and writes d_value; all threads
 *                    stream d_log_prob back out with 16-B stores; the four fp64 sums of the 256
 *                    rows go through a pairwise tree in LDS to partials[block][4].
 *   sqnorm_kernel    grid-stride over chunks of 4096 elements: 16-B loads, squares in fp64, the
 *                    pairwise tree of a chunk (4 elements in registers, 1024 nodes in LDS) to
 *                    partials[chunk].
 *   tree_finish      one workgroup: the pairwise tree over the partials (groups of 1024, then
 *                    the group roots), zero-padded; root + 0.0 to the output.
 *   grad_combine_kernel  the gradient sum over ranks: sqnorm_kernel's chunks and first stage, with
 *                    each element first formed as the fp64 pairwise tree over the ranks' rows (in rank
 *                    order, a recursion with one accumulator per level) and stored as fp32; then
 *                    tree_finish, so the squared norm costs no second read of the gradient.
 *   adamw_kernel     grid-stride float4 stream over the live elements (count - frozen_tail), a
 *                    scalar tail; every thread forms the clip factor from the k squared norms.
 *
 * Trees: leaves in index order, adjacent pairs first, zero padding: whatever the workgroup size,
 * the same tree as zb_host.cpp's recursive tree_sum. No floating-point atomics.
 */
#include <hip/hip_runtime.h>

#include "zb_internal.h"
#include "zbot_learner_math.h"

namespace zb {

constexpr int LROWS = ZB_LOSS_ROWS_PER_BLOCK;    /* rows per workgroup = threads */
constexpr int LLD = ZBL_JOINTS + 1;              /* LDS row stride, words */
constexpr int SQ_CHUNK = ZB_SQNORM_ELEMS_PER_BLOCK;
constexpr int SQ_NODES = SQ_CHUNK / 4;           /* tree nodes of a chunk held in LDS */
constexpr int FTREE = 1024;                      /* leaves per level of the finishing tree */
constexpr int MAX_BLOCKS = 2048;                 /* 256 CUs x 8: grid-stride the rest */

/* Pairwise sum over a power-of-two LDS array, in place; the root lands in element 0. All threads
   of the workgroup participate. */
template <int N>
__device__ inline void tree1(double* s) {
#pragma unroll
  for (int st = 1; st < N; st <<= 1) {
    __syncthreads();
    for (int i = threadIdx.x * 2 * st; i < N; i += blockDim.x * 2 * st) s[i] = s[i] + s[i + st];
  }
  __syncthreads();
}

__global__ __launch_bounds__(LROWS) void ppo_loss_kernel(LossArgs a) {
#pragma clang fp contract(off)
  __shared__ float slp[LROWS * LLD];
  __shared__ float sold[LROWS * LLD];
  __shared__ float sg[LROWS];
  __shared__ double red[4][LROWS];

  const int tid = threadIdx.x;
  const size_t row0 = (size_t)blockIdx.x * LROWS;
  const int nrows = (int)(a.rows - row0 < (size_t)LROWS ? a.rows - row0 : (size_t)LROWS);
  const size_t base = row0 * ZBL_JOINTS; /* a multiple of 4 words */
  const int nq = nrows * (ZBL_JOINTS / 4); /* float4s of this workgroup's rows; 5 per row */

  if (a.vec) {
    const float4* p4 = reinterpret_cast<const float4*>(a.log_prob + base);
    const float4* o4 = reinterpret_cast<const float4*>(a.old_log_prob + base);
    for (int q = tid; q < nq; q += LROWS) {
      const float4 x = p4[q], y = o4[q];
      const int r = q / 5, j = 4 * (q - 5 * r);
      float* d = &slp[r * LLD + j];
      float* e = &sold[r * LLD + j];
      d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
      e[0] = y.x; e[1] = y.y; e[2] = y.z; e[3] = y.w;
    }
  } else {
    for (int i = tid; i < nrows * ZBL_JOINTS; i += LROWS) {
      const int r = i / ZBL_JOINTS, j = i - ZBL_JOINTS * r;
      slp[r * LLD + j] = a.log_prob[base + i];
      sold[r * LLD + j] = a.old_log_prob[base + i];
    }
  }
  __syncthreads();

  ZblLossRow o;
  o.d_log_prob = o.d_value = o.surrogate = o.value_term = o.clipped = o.kl = 0.0f;
  if (tid < nrows) {
    const size_t i = row0 + tid;
    const float s = zbl_joint_sum(&slp[tid * LLD]);
    const float s0 = zbl_joint_sum(&sold[tid * LLD]);
    zbl_loss_row(s, s0, a.advantages[i], a.values[i], a.old_values[i], a.value_targets[i], a.clip_param,
                 a.log_clip_value, a.value_loss_coef, a.inv, a.use_clipped_value_loss, &o);
    a.d_value[i] = o.d_value;
  }
  sg[tid] = o.d_log_prob;
  red[0][tid] = (double)o.surrogate; /* rows past the end are +0.0 leaves */
  red[1][tid] = (double)o.value_term;
  red[2][tid] = (double)o.clipped;
  red[3][tid] = (double)o.kl;
#pragma unroll
  for (int st = 1; st < LROWS; st <<= 1) {
    __syncthreads();
    for (int i = tid * 2 * st; i < LROWS; i += LROWS * 2 * st) {
#pragma unroll
      for (int c = 0; c < 4; ++c) red[c][i] = red[c][i] + red[c][i + st];
    }
  }
  __syncthreads(); /* sg and the roots are visible */

  if (a.vec) {
    float4* d4 = reinterpret_cast<float4*>(a.d_log_prob + base);
    for (int q = tid; q < nq; q += LROWS) {
      const float g = sg[q / 5];
      d4[q] = make_float4(g, g, g, g);
    }
  } else {
    for (int i = tid; i < nrows * ZBL_JOINTS; i += LROWS) a.d_log_prob[base + i] = sg[i / ZBL_JOINTS];
  }
  if (tid < 4) a.partials[4 * (size_t)blockIdx.x + tid] = red[tid][0];
}

/* One workgroup: for each of C interleaved components, the pairwise tree over k partials
   in[k][C], zero-padded (groups of FTREE leaves first, then the group roots: k <= FTREE^2);
   out[c] = root + 0.0. */
__global__ __launch_bounds__(FTREE) void tree_finish_kernel(const double* in, int k, int C, double* out) {
  __shared__ double leaf[FTREE];
  __shared__ double root[FTREE];
  const int tid = threadIdx.x;
  const int ngroups = (k + FTREE - 1) / FTREE;
  for (int c = 0; c < C; ++c) {
    root[tid] = 0.0;
    for (int g = 0; g < ngroups; ++g) {
      const int i = g * FTREE + tid;
      leaf[tid] = i < k ? in[(size_t)i * C + c] : 0.0;
      tree1<FTREE>(leaf);
      if (tid == 0) root[g] = leaf[0];
      __syncthreads();
    }
    if (ngroups > 1) tree1<FTREE>(root);
    if (tid == 0) out[c] = root[0] + 0.0;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void sqnorm_kernel(const float* g, size_t count, size_t nchunks, double* partials,
                                                     int vec) {
#pragma clang fp contract(off)
  __shared__ double node[SQ_NODES];
  const int tid = threadIdx.x;
  for (size_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const size_t base = ch * SQ_CHUNK;
#pragma unroll
    for (int j = 0; j < SQ_NODES / 256; ++j) {
      const int q = j * 256 + tid;
      const size_t e = base + 4 * (size_t)q;
      float x[4];
      if (vec && e + 4 <= count) {
        const float4 t = *reinterpret_cast<const float4*>(g + e);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = e + c < count ? g[e + c] : 0.0f;
      }
      const double d0 = (double)x[0], d1 = (double)x[1], d2 = (double)x[2], d3 = (double)x[3];
      const double q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3;
      const double lo = q0 + q1, hi = q2 + q3;
      node[q] = lo + hi;
    }
    tree1<SQ_NODES>(node);
    if (tid == 0) partials[ch] = node[0];
    __syncthreads(); /* node is rewritten by the next chunk */
  }
}

/* ---- zb_grad_combine: the rank tree of every element, and the squared norm of the result ---- */

struct Col4 {
  double v[4];
};

/* Elements e .. e + 3 of the row that `row` points into (at element e) as fp64 leaves; `row` then
   moves on to the next rank's row (the tree visits the rows in rank order, each once).
   MODE 2: one 16-byte load; 1: four 4-byte loads; 0: a chunk with a ragged end, where elements
   past `count` are +0.0 leaves (never stored). */
template <int MODE>
__device__ inline Col4 combine_leaf(const float*& row, size_t count, size_t e) {
  float x[4];
  if constexpr (MODE == 2) {
    const float4 t = *reinterpret_cast<const float4*>(row);
    x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
  } else if constexpr (MODE == 1) {
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = row[c];
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c) x[c] = e + c < count ? row[c] : 0.0f;
  }
  row += count;
  Col4 o;
#pragma unroll
  for (int c = 0; c < 4; ++c) o.v[c] = (double)x[c];
  return o;
}

/* The balanced pairwise tree over rows r0 .. r0 + LEN - 1 (LEN a power of two, r0 < world); rows at or
   past `world` are the zero padding, and adding +0.0 is exact, so an absent right half is skipped (the
   sign of an all-zero sum is settled by the caller's root + 0.0). `world` is uniform, so every branch
   is; the recursion keeps one accumulator per level live: log2(ZB_COMBINE_MAX_WORLD) + 1 = 7 per
   element, no world-sized array. Four whole rows are loaded together before they are added. */
template <int MODE, int LEN>
__device__ inline Col4 rank_tree(const float*& row, size_t count, int world, int r0, size_t e) {
#pragma clang fp contract(off)
  if constexpr (LEN == 1) {
    return combine_leaf<MODE>(row, count, e);
  } else {
    if constexpr (LEN == 4) {
      if (r0 + 4 <= world) {
        const Col4 a = combine_leaf<MODE>(row, count, e);
        const Col4 b = combine_leaf<MODE>(row, count, e);
        const Col4 c = combine_leaf<MODE>(row, count, e);
        const Col4 d = combine_leaf<MODE>(row, count, e);
        Col4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double lo = a.v[k] + b.v[k], hi = c.v[k] + d.v[k];
          o.v[k] = lo + hi;
        }
        return o;
      }
    }
    Col4 a = rank_tree<MODE, LEN / 2>(row, count, world, r0, e);
    if (r0 + LEN / 2 < world) {
      const Col4 b = rank_tree<MODE, LEN / 2>(row, count, world, r0 + LEN / 2, e);
#pragma unroll
      for (int k = 0; k < 4; ++k) a.v[k] = a.v[k] + b.v[k];
    }
    return a;
  }
}

/* One chunk: a thread owns the float4s q = j 256 + tid, j < 4, as in sqnorm_kernel; per float4 it
   streams the rows in rank order through rank_tree, rounds root + 0.0 to fp32 once, stores it, and
   leaves the square of the rounded value in node[q] exactly as sqnorm_kernel forms it. */
template <int MODE>
__device__ inline void combine_chunk(const float* parts, int world, size_t count, size_t base, float* grad,
                                     double* node) {
#pragma clang fp contract(off)
#pragma unroll 1
  for (int j = 0; j < SQ_NODES / 256; ++j) {
    const int q = j * 256 + (int)threadIdx.x;
    const size_t e = base + 4 * (size_t)q;
    double s = 0.0;
    if (MODE != 0 || e < count) { /* a float4 wholly past the end is a +0.0 node and touches no memory */
      const float* row = parts + e; /* this float4 in rank 0's row */
      /* keeps the tree's ~100 comparisons with `world` beside their branches: hoisted out of this
         loop, each would hold a scalar register pair across it, more than there are */
      int w = world;
      asm volatile("" : "+s"(w));
      const Col4 t = rank_tree<MODE, ZB_COMBINE_MAX_WORLD>(row, count, w, 0, e);
      float x[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) x[c] = (float)(t.v[c] + 0.0);
      if constexpr (MODE == 2) {
        *reinterpret_cast<float4*>(grad + e) = make_float4(x[0], x[1], x[2], x[3]);
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (MODE == 1 || e + c < count) grad[e + c] = x[c];
      }
      const double d0 = (double)x[0], d1 = (double)x[1], d2 = (double)x[2], d3 = (double)x[3];
      const double q0 = d0 * d0, q1 = d1 * d1, q2 = d2 * d2, q3 = d3 * d3;
      const double lo = q0 + q1, hi = q2 + q3;
      s = lo + hi;
    }
    node[q] = s;
  }
}

/* One workgroup per 4096-element chunk (grid-stride past MAX_BLOCKS). A chunk that lies wholly below
   `count` moves in 16-byte accesses (vec: parts, grad and the row stride allow it) or 4-byte ones;
   the last, ragged chunk in guarded 4-byte ones. Then the chunk's tree, the same tree1 over the
   same nodes as sqnorm_kernel: partials[chunk] is what zb_grad_sqnorm's first stage writes for
   this grad. */
__global__ __launch_bounds__(256) void grad_combine_kernel(const float* parts, int world, size_t count, size_t nchunks,
                                                           float* grad, double* partials, int vec) {
  __shared__ double node[SQ_NODES];
  for (size_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const size_t base = ch * SQ_CHUNK;
    if (base + SQ_CHUNK > count)
      combine_chunk<0>(parts, world, count, base, grad, node);
    else if (vec)
      combine_chunk<2>(parts, world, count, base, grad, node);
    else
      combine_chunk<1>(parts, world, count, base, grad, node);
    tree1<SQ_NODES>(node);
    if (threadIdx.x == 0) partials[ch] = node[0];
    __syncthreads(); /* node is rewritten by the next chunk */
  }
}

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a) {
#pragma clang fp contract(off)
  const float scale = zbl_clip_scale(a.sqnorms, a.k, a.max_grad_norm);
  const size_t live = a.count - a.frozen_tail;
  const size_t n4 = a.vec ? live / 4 : 0;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  float4* p4 = reinterpret_cast<float4*>(a.param);
  float4* m4 = reinterpret_cast<float4*>(a.m);
  float4* v4 = reinterpret_cast<float4*>(a.v);
  const float4* g4 = reinterpret_cast<const float4*>(a.grad);
  for (size_t i = t0; i < n4; i += stride) {
    float4 p = p4[i], m = m4[i], v = v4[i];
    const float4 g = g4[i];
    zbl_adamw(&p.x, &m.x, &v.x, g.x, scale, a.lr, a.c.beta1, a.c.omb1, a.c.beta2, a.c.omb2, a.c.bc1, a.c.bc2, a.eps, a.wd);
    zbl_adamw(&p.y, &m.y, &v.y, g.y, scale, a.lr, a.c.beta1, a.c.omb1, a.c.beta2, a.c.omb2, a.c.bc1, a.c.bc2, a.eps, a.wd);
    zbl_adamw(&p.z, &m.z, &v.z, g.z, scale, a.lr, a.c.beta1, a.c.omb1, a.c.beta2, a.c.omb2, a.c.bc1, a.c.bc2, a.eps, a.wd);
    zbl_adamw(&p.w, &m.w, &v.w, g.w, scale, a.lr, a.c.beta1, a.c.omb1, a.c.beta2, a.c.omb2, a.c.bc1, a.c.bc2, a.eps, a.wd);
    p4[i] = p;
    m4[i] = m;
    v4[i] = v;
  }
  /* the elements before the frozen tail that fill no whole float4 (all of them when unaligned) */
  for (size_t i = n4 * 4 + t0; i < live; i += stride)
    zbl_adamw(&a.param[i], &a.m[i], &a.v[i], a.grad[i], scale, a.lr, a.c.beta1, a.c.omb1, a.c.beta2, a.c.omb2, a.c.bc1, a.c.bc2, a.eps, a.wd);
}

static bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

hipError_t launch_ppo_loss(LossArgs a, double* sums_out, hipStream_t s) {
  const int nblk = (int)((a.rows + LROWS - 1) / LROWS);
  a.vec = al16(a.log_prob) && al16(a.old_log_prob) && al16(a.d_log_prob);
  hipLaunchKernelGGL(ppo_loss_kernel, dim3(nblk), dim3(LROWS), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tree_finish_kernel, dim3(1), dim3(FTREE), 0, s, a.partials, nblk, 4, sums_out);
  return hipGetLastError();
}

hipError_t launch_sqnorm(const float* grad, size_t count, double* partials, double* out, hipStream_t s) {
  const size_t nchunks = (count + SQ_CHUNK - 1) / SQ_CHUNK;
  const int blocks = (int)(nchunks < (size_t)MAX_BLOCKS ? nchunks : (size_t)MAX_BLOCKS);
  hipLaunchKernelGGL(sqnorm_kernel, dim3(blocks), dim3(256), 0, s, grad, count, nchunks, partials, al16(grad) ? 1 : 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tree_finish_kernel, dim3(1), dim3(FTREE), 0, s, partials, (int)nchunks, 1, out);
  return hipGetLastError();
}

hipError_t launch_grad_combine(const float* parts, int world, size_t count, float* grad, double* partials,
                               double* sq_out, bool vec, hipStream_t s) {
  const size_t nchunks = (count + SQ_CHUNK - 1) / SQ_CHUNK;
  const int blocks = (int)(nchunks < (size_t)MAX_BLOCKS ? nchunks : (size_t)MAX_BLOCKS);
  hipLaunchKernelGGL(grad_combine_kernel, dim3(blocks), dim3(256), 0, s, parts, world, count, nchunks, grad, partials,
                     vec ? 1 : 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(tree_finish_kernel, dim3(1), dim3(FTREE), 0, s, partials, (int)nchunks, 1, sq_out);
  return hipGetLastError();
}

hipError_t launch_adamw(AdamArgs a, hipStream_t s) {
  a.vec = al16(a.param) && al16(a.grad) && al16(a.m) && al16(a.v);
  const size_t live = a.count - a.frozen_tail;
  if (live == 0) return hipSuccess;
  const size_t work = a.vec ? (live + 3) / 4 : live;
  size_t blocks = (work + 255) / 256;
  if (blocks > (size_t)MAX_BLOCKS) blocks = MAX_BLOCKS;
  hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace zb
