// cbg_vector.h -- what the vector products share (cbg_bfs.hip, cbg_spmv.hip; the fill also cbg_ewise.hip and
// cbg_prune.hip): a column's expansion unit, its search and plan, the fold of a grid row's blocks, the fill.
#pragma once
#include "cbg_device.h"
#include "cbg_internal.h"

namespace cbg {

constexpr int WAVES = 256 / WAVE;  // of a 256-thread block
// Entries of a column of a sparse vector that one expansion unit (one wave) takes: 4 trips.  A scale-20 hub
// column of 10^5 entries gives 400 waves, and the unit's search over the vector (20 steps) stays small
// against its 256 entries.  Reported by cbg_bfs_bounds()[0] and cbg_spmv_bounds()[2].
constexpr int EXPAND_UNIT = 256;

// The owner of unit u: the last k in [0, n) with start(k) <= u, start the exclusive scan of the units per
// entry.  An entry without units shares its start with the next one and is never the last.
template <class Start>
__device__ __forceinline__ int64_t unit_owner(int64_t n, int64_t u, Start&& start) {
  int64_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (start(mid) <= u) lo = mid;
    else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ int64_t unit_owner(const int64_t* __restrict__ start, int64_t n, int64_t u) {
  return unit_owner(n, u, [&](int64_t k) { return start[k]; });
}

// The expansion plan of the nf columns fl[] of a tile (device; len = tile_col_map's column lengths): ustart =
// the scan of ceil(len / EXPAND_UNIT) and, with `products`, pstart = the scan of the lengths; nf + 1 entries
// each.  The totals are read back behind ONE synchronization of s, which also covers what the caller queued.
struct ExpandPlan {
  DBuf<int64_t> buf;  // nu | ustart | plen | pstart
  int64_t *ustart = nullptr, *pstart = nullptr;
  int64_t units = 0, products = 0;
};
void expand_plan(const int32_t* fl, int64_t nf, const int64_t* len, bool products, ExpandPlan& pl, hipStream_t s);

// y[i] = op(... op(op(all[i], all[lm + i]), all[2 lm + i]) ...): the P blocks of a grid row folded in rank
// order, in exactly this association (the bits of a PlusTimes sum depend on it)
template <class T, class Op>
__global__ __launch_bounds__(256) void k_fold_blocks(T* __restrict__ y, const T* __restrict__ all, int P, int64_t lm, Op op) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= lm) return;
  T v = all[i];
  for (int q = 1; q < P; ++q) v = op(v, all[(int64_t)q * lm + i]);
  y[i] = v;
}
template <class T, class Op>
void fold_blocks(T* y, const T* all, int P, int64_t lm, Op op, hipStream_t s) {
  if (lm > 0) hipLaunchKernelGGL((k_fold_blocks<T, Op>), dim3(nblk(lm, 256)), dim3(256), 0, s, y, all, P, lm, op);
  CBG_HIP(hipGetLastError());
}

template <class T>
__global__ __launch_bounds__(256) void k_fill(T* __restrict__ d, int64_t n, T v) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) d[i] = v;
}
template <class T>
void fill_device(T* p, int64_t n, T v, hipStream_t s) {
  if (n > 0) hipLaunchKernelGGL(k_fill<T>, dim3(nblk(n, 256)), dim3(256), 0, s, p, n, v);
  CBG_HIP(hipGetLastError());
}

}  // namespace cbg
