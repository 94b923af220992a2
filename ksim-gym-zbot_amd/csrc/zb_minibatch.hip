/*
 * zb_minibatch.hip — the keyed minibatch permutation as an array, and the gather that cuts every
 * array of one minibatch out of a rollout in one launch. C ABI: include/zbot_ppo.h "Minibatches".
 * The permutation is include/zbot_fmath.h zbf_perm_index, integers only and shared source-identical
 * with the host twins in zb_host.cpp, so results are bit-identical to them; the gather moves bytes.
 *
 *   perm_kernel    one thread per index.
 *   gather_kernel  grid (env chunks of GJ, items, time rows). A workgroup first evaluates the
 *                  permutation for its GJ destination envs into LDS (GJ evaluations: 4 threefry
 *                  rounds per walk, about 2 walks each; nothing next to the rows it then moves),
 *                  then streams its rows: consecutive threads take consecutive units of an env's
 *                  row, so a wave reads and writes whole contiguous rows. The unit is the item's
 *                  access width (16, 8, 4 or 1 bytes, chosen on the host: check_gather_args), the
 *                  same for every thread of a workgroup, so the switch on it does not diverge.
 *                  The time rows of an item are strided over gridDim.z; items with fewer rows
 *                  than the launch's largest leave the extra workgroups with nothing to do.
 *                  gather_kernel<true> is zb_minibatch_gather_seq's: source row t = c L + l of an
 *                  item cut in chunks of L rows (C = rows / L of them) goes to destination row
 *                  l C + c, so dst [L][C count] holds chunk c of the workgroup's envs in columns
 *                  c count + j; only the row's base address differs, the row still moves as one
 *                  contiguous piece. gather_kernel<false> is the whole-sequence gather as it was.
 *
 * Bounds: a workgroup reads src rows p(lo + j) < n for j < count and t < rows, and writes dst rows
 * t' * count + j with t' = t, or for a cut item t' = l C + c < L C = rows (l < L, c < C; rows is a
 * multiple of L, checked before the launch): the same [rows][count] extent either way.
 * zbf_perm_index returns a value < n for an index < n, and lo + count <= n is checked before the
 * launch.
 */
#include <hip/hip_runtime.h>

#include "zb_internal.h"
#include "zbot_fmath.h"

namespace zb {

constexpr int GJ = 64;        /* destination envs per workgroup */
constexpr int GTHREADS = 256;
constexpr int GMAX_Z = 1024;  /* time rows across gridDim.z; more rows stride */

__global__ __launch_bounds__(256) void perm_kernel(uint64_t seed, uint32_t epoch, int n, int32_t* perm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) perm[i] = (int32_t)zbf_perm_index(seed, epoch, (uint32_t)n, (uint32_t)i);
}

template <typename V, bool SEQ>
__device__ inline void move_rows(const GatherItemDev& it, const uint32_t* sp, int j0, int jn, int count) {
  const int upr = it.row_bytes / (int)sizeof(V); /* units per row */
  const int units = jn * upr;
  V zero;
  __builtin_memset(&zero, 0, sizeof(V));
  for (int t = blockIdx.z; t < it.rows; t += gridDim.z) {
    const char* s = it.src ? it.src + (size_t)t * (size_t)it.stride : nullptr;
    int dt = t;
    if (SEQ && it.chunk) { /* uniform over the workgroup */
      const int c = t / it.chunk;
      dt = (t - c * it.chunk) * (it.rows / it.chunk) + c;
    }
    char* d = it.dst + ((size_t)dt * (size_t)count + (size_t)j0) * (size_t)it.row_bytes;
    for (int u = threadIdx.x; u < units; u += GTHREADS) {
      const int j = u / upr, k = u - j * upr;
      V x = zero;
      if (s) x = *reinterpret_cast<const V*>(s + (size_t)sp[j] * (size_t)it.row_bytes + (size_t)k * sizeof(V));
      *reinterpret_cast<V*>(d + (size_t)u * sizeof(V)) = x;
    }
  }
}

template <bool SEQ>
__global__ __launch_bounds__(GTHREADS) void gather_kernel(GatherArgs a) {
  __shared__ uint32_t sp[GJ];
  const GatherItemDev& it = a.it[blockIdx.y];
  if ((int)blockIdx.z >= it.rows) return; /* uniform over the workgroup */
  const int j0 = blockIdx.x * GJ;
  const int jn = a.count - j0 < GJ ? a.count - j0 : GJ;
  if ((int)threadIdx.x < jn) {
    const uint32_t i = (uint32_t)(a.lo + j0 + (int)threadIdx.x);
    sp[threadIdx.x] = a.shuffle ? zbf_perm_index(a.seed, a.epoch, (uint32_t)a.n, i) : i;
  }
  __syncthreads();
  switch (it.width) {
    case 16: move_rows<uint4, SEQ>(it, sp, j0, jn, a.count); break;
    case 8: move_rows<uint2, SEQ>(it, sp, j0, jn, a.count); break;
    case 4: move_rows<uint32_t, SEQ>(it, sp, j0, jn, a.count); break;
    default: move_rows<uint8_t, SEQ>(it, sp, j0, jn, a.count); break;
  }
}

hipError_t launch_minibatch_perm(uint64_t seed, uint32_t epoch, int n, int32_t* perm, hipStream_t s) {
  hipLaunchKernelGGL(perm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, seed, epoch, n, perm);
  return hipGetLastError();
}

hipError_t launch_minibatch_gather(const GatherArgs& a, hipStream_t s) {
  int rows = 1, seq = 0;
  for (int k = 0; k < a.n_items; k++) {
    rows = a.it[k].rows > rows ? a.it[k].rows : rows;
    seq |= a.it[k].chunk;
  }
  const dim3 grid((unsigned)((a.count + GJ - 1) / GJ), (unsigned)a.n_items, (unsigned)(rows < GMAX_Z ? rows : GMAX_Z));
  if (seq)
    hipLaunchKernelGGL(gather_kernel<true>, grid, dim3(GTHREADS), 0, s, a);
  else
    hipLaunchKernelGGL(gather_kernel<false>, grid, dim3(GTHREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace zb
