// cbg_spmv.hip -- y = A x on PlusTimesSRing<double,double> and MinPlusSRing<double,double> for one device
// DCSC tile, with a dense x (dcsc_gespmv, Friends.h:63-78) and with a sparse one (SpMXSpV, SpImpl.cpp).
//
// THE ORDER OF A ROW'S SUM (restated in tests/spmv_ref.py) depends only on the number L of its products,
// which are listed in ascending column order and rounded on their own (this file is built with
// -ffp-contract=off):
//   L <= 16     16 lanes      lane l starts at Sem<SR>::identity() and folds products l, l + G, l + 2G, ...
//   L <= 4096   64 lanes      one after another; the lanes are combined by the xor tree over distances
//                             1, 2, 4, ... with Sem<SR>::add
//   longer      chunks of 4096 products (the last one shorter), each reduced as a 64-lane row by a wave of
//               its own; the chunk results are folded one after another in chunk order.  A hub row does
//               not serialise on one workgroup.
// No atomics take part, so the result has the same bits in every run.
//
//   dense   pull over At = cbg_tile_transpose(A): column p of At is row At.jc[p] of A with the column ids
//           ascending.  A 16-lane group per stored row reduces the short ones and writes the class of the
//           others; one scan of the classes queues the rows of up to 4096 entries for a wave each and
//           gives the unit list (row, chunk) of the longer ones.  Each lane loads At.ir (4 B) and At.val (8 B) coalesced and gathers
//           x[ir].  y is filled with SR::id() first, and a stored row writes add(SR::id(), r).
//   sparse  x's columns go through A's column map; a unit is (column of x, chunk of at most EXPAND_UNIT of
//           its entries), one wave each, and writes key = row, value = mul(a, x[j]) at the column's
//           product offset: the products in ascending (j, i) order.  A stable radix sort by row keeps the
//           products of a row in ascending j; the run heads give the segments, which the same three
//           classes reduce.  The result keeps r itself (not folded with id): a cancelled sum is a stored 0.0.
#include <algorithm>
#include <cfloat>
#include <cstring>

#include "cbg_vector.h"

namespace cbg {

namespace {
constexpr int SPMV_GROUP = 16;     // the longest row of a 16-lane group
constexpr int SPMV_WAVE = 4096;    // the longest row of one wave, and the chunk of the longer ones
constexpr int GROUPS = 256 / SPMV_GROUP;

// add(SR::id(), r) with the reference's id (0.0, DBL_MAX): what the dense product stores
template <int SR>
__device__ __forceinline__ double fold_id(double r) {
  if constexpr (SR == 0) return 0.0 + r;
  else return r < DBL_MAX ? r : DBL_MAX;
}
template <int SR>
__device__ __forceinline__ double ref_id() {
  return SR == 0 ? 0.0 : DBL_MAX;
}

// G lanes (lane l of them) fold the products [k0, k1): every lane returns the result.  Every lane of the
// wave calls it (an idle group with k1 == k0), so the cross-lane moves see a full wave.
template <int SR, int G, class S>
__device__ __forceinline__ double lanes_reduce(const S& src, int64_t k0, int64_t k1, int l) {
  double acc = Sem<SR>::identity();
  int64_t k = k0 + l;
  for (; k + 3 * G < k1; k += 4 * G) {  // four gathers in flight, folded in order
    const double p0 = src.prod(k), p1 = src.prod(k + G), p2 = src.prod(k + 2 * G), p3 = src.prod(k + 3 * G);
    acc = Sem<SR>::add(Sem<SR>::add(Sem<SR>::add(Sem<SR>::add(acc, p0), p1), p2), p3);
  }
  for (; k < k1; k += G) acc = Sem<SR>::add(acc, src.prod(k));
#pragma unroll
  for (int d = 1; d < G; d <<= 1) acc = Sem<SR>::add(acc, __shfl_xor(acc, d, WAVE));
  return acc;
}

// rows of the dense product: the stored columns of At
template <int SR>
struct DenseRows {
  int64_t nrows;
  const int64_t* __restrict__ cp;
  const int32_t* __restrict__ jc;
  const int32_t* __restrict__ ir;
  const double* __restrict__ val;
  const double* __restrict__ x;
  double* __restrict__ y;
  __device__ __forceinline__ int64_t begin(int64_t p) const { return cp[p]; }
  __device__ __forceinline__ int64_t end(int64_t p) const { return cp[p + 1]; }
  __device__ __forceinline__ double prod(int64_t k) const { return Sem<SR>::mul(ld_stream(val + k), x[ld_stream(ir + k)]); }
  __device__ __forceinline__ void out(int64_t p, double r) const { y[jc[p]] = fold_id<SR>(r); }
};
// rows of the sparse product: the runs of equal keys of the sorted products
template <int SR>
struct SortedRows {
  int64_t nrows;
  const int64_t* __restrict__ start;
  const uint32_t* __restrict__ key;
  const double* __restrict__ pv;
  uint32_t* __restrict__ yind;
  double* __restrict__ yval;
  __device__ __forceinline__ int64_t begin(int64_t p) const { return start[p]; }
  __device__ __forceinline__ int64_t end(int64_t p) const { return start[p + 1]; }
  __device__ __forceinline__ double prod(int64_t k) const { return ld_stream(pv + k); }
  __device__ __forceinline__ void out(int64_t p, double r) const {
    yind[p] = key[start[p]];
    yval[p] = r;
  }
};

// A row's class as one scan element: bit 32 set for a row queued for a wave, the low word the chunks of a
// long row.  One exclusive scan of these gives the queue positions and the (row, chunk) unit starts.
constexpr int64_t CHUNK_MASK = 0xffffffffll;

// A 16-lane group per row: reduces a short row; cls[p] = the class word of the others.  No atomics: one per
// wave on a shared counter took 0.5 ms at scale 18, and a block looping over many rows to share one pays
// the rows' load latencies one after another.
template <int SR, class S>
__global__ __launch_bounds__(256) void k_spmv_group(S src, int64_t* __restrict__ cls) {
  const int64_t p = (int64_t)blockIdx.x * GROUPS + threadIdx.x / SPMV_GROUP;
  const int l = threadIdx.x & (SPMV_GROUP - 1);
  const bool valid = p < src.nrows;
  const int64_t b = valid ? src.begin(p) : 0, len = valid ? src.end(p) - b : 0;
  const bool small = valid && len <= SPMV_GROUP;
  const double r = lanes_reduce<SR, SPMV_GROUP>(src, b, small ? b + len : b, l);
  if (l == 0 && valid) {
    if (small) src.out(p, r);
    cls[p] = small ? 0 : len <= SPMV_WAVE ? (1ll << 32) : (len + SPMV_WAVE - 1) / SPMV_WAVE;
  }
}

// pre = the scan of cls: the wave rows into their queue (ascending), and the counts
// stat: 1 rows queued for a wave, 2 long rows, 3 chunks (the rows of the group class are the rest)
__global__ __launch_bounds__(256) void k_spmv_queue(int64_t nrows, const int64_t* __restrict__ cls, const int64_t* __restrict__ pre,
                                                    int32_t* __restrict__ waveq, u64* __restrict__ stat) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool big = false;
  if (p < nrows) {
    const int64_t v = cls[p];
    if (v >> 32) waveq[pre[p] >> 32] = (int32_t)p;
    big = (v & CHUNK_MASK) != 0;
  }
  const u64 mb = __ballot(big);  // long rows are few: an atomic only from the waves that hold one
  if (lane_id() == 0 && mb) atomicAdd(stat + 2, (unsigned long long)__popcll(mb));
  if (p == 0) {
    stat[1] = (u64)(pre[nrows] >> 32);
    stat[3] = (u64)(pre[nrows] & CHUNK_MASK);
  }
}

// one wave per queued row, the waves striding over the queue
template <int SR, class S>
__global__ __launch_bounds__(256) void k_spmv_wave(S src, const int32_t* __restrict__ waveq, const u64* __restrict__ stat) {
  const int64_t nq = (int64_t)stat[1];
  const int lane = lane_id();
  const int64_t w0 = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  for (int64_t q = w0; q < nq; q += (int64_t)gridDim.x * WAVES) {
    const int64_t p = waveq[q];
    const double r = lanes_reduce<SR, WAVE>(src, src.begin(p), src.end(p), lane);
    if (lane == 0) src.out(p, r);
  }
}

// one wave per (long row, chunk): the low words of pre are the rows' unit starts
template <int SR, class S>
__global__ __launch_bounds__(256) void k_spmv_chunk(S src, const int64_t* __restrict__ pre, double* __restrict__ partial) {
  const int64_t units = pre[src.nrows] & CHUNK_MASK;
  const int lane = lane_id();
  const int64_t w0 = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  for (int64_t u = w0; u < units; u += (int64_t)gridDim.x * WAVES) {
    // the unit's row: the starts are the low words of pre
    const int64_t lo = unit_owner(src.nrows, u, [&](int64_t p) { return pre[p] & CHUNK_MASK; });
    const int64_t k0 = src.begin(lo) + (u - (pre[lo] & CHUNK_MASK)) * SPMV_WAVE, k1 = min(k0 + SPMV_WAVE, src.end(lo));
    const double r = lanes_reduce<SR, WAVE>(src, k0, k1, lane);
    if (lane == 0) partial[u] = r;
  }
}

// a long row's chunk results, one after another in chunk order
template <int SR, class S>
__global__ __launch_bounds__(256) void k_spmv_long_fold(S src, const int64_t* __restrict__ pre,
                                                        const double* __restrict__ partial) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= src.nrows) return;
  const int64_t u0 = pre[p] & CHUNK_MASK, u1 = pre[p + 1] & CHUNK_MASK;
  if (u1 == u0) return;
  double acc = partial[u0];
  for (int64_t u = u0 + 1; u < u1; ++u) acc = Sem<SR>::add(acc, partial[u]);
  src.out(p, acc);
}

// ---- the sparse product's expansion (its plan: expand_plan, cbg_vector.h) ----
// one wave per unit
template <int SR>
__global__ __launch_bounds__(256) void k_spmspv_expand(int64_t nx, const int32_t* __restrict__ fl, const double* __restrict__ xv,
                                                       const int32_t* __restrict__ pos, const int64_t* __restrict__ cp,
                                                       const int32_t* __restrict__ ir, const double* __restrict__ val,
                                                       const int64_t* __restrict__ ustart, const int64_t* __restrict__ pstart,
                                                       int64_t units, uint32_t* __restrict__ key, double* __restrict__ pv) {
  const int64_t u = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (u >= units) return;
  const int64_t lo = unit_owner(ustart, nx, u);  // the unit's entry of x
  const int32_t p = pos[fl[lo]];
  if (p < 0) return;  // not stored: it has no unit, so this is never taken
  const int64_t off = (u - ustart[lo]) * EXPAND_UNIT;
  const int64_t a0 = cp[p] + off, a1 = min(a0 + EXPAND_UNIT, cp[p + 1]), o0 = pstart[lo] + off;
  const double xj = xv[lo];
  for (int64_t t = lane_id(); a0 + t < a1; t += WAVE) {
    key[o0 + t] = (uint32_t)ld_stream(ir + a0 + t);
    pv[o0 + t] = Sem<SR>::mul(ld_stream(val + a0 + t), xj);
  }
}

__global__ __launch_bounds__(256) void k_spmspv_heads(const uint32_t* __restrict__ key, int64_t n, int32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}
// seg = the scan of head: start[seg[i]] = i at the heads, start[seg[n]] = n
__global__ __launch_bounds__(256) void k_spmspv_starts(const uint32_t* __restrict__ key, int64_t n, const int64_t* __restrict__ seg,
                                                       int64_t* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  if (i == n || i == 0 || key[i] != key[i - 1]) start[seg[i]] = i;
}

template <int SR>
struct SemAdd {
  __device__ __forceinline__ double operator()(double a, double b) const { return Sem<SR>::add(a, b); }
};

// the calling thread's state between an asynchronous product and the reading of its statistics
struct Pending {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  u64* host = nullptr;  // pinned: the call's stat words
  bool waiting = false;
  int64_t rows = 0;  // the rows the call's reductions ran over
  std::vector<void*> blocks;  // the call's temporaries, back to the pool once it has finished
};
Pending& pending() {
  static thread_local Pending p;
  return p;
}
SpmvStats& raw_stats() {
  static thread_local SpmvStats s;
  return s;
}
void pending_resolve() {
  Pending& pd = pending();
  if (pd.waiting) {
    pd.waiting = false;
    const hipError_t e = hipEventSynchronize(pd.e1);
    for (void* q : pd.blocks) pool().free(q);
    pd.blocks.clear();
    if (e != hipSuccess) throw HipError(std::string("spmv: ") + hipGetErrorString(e), CBG_ERR_HIP);
    SpmvStats& st = raw_stats();
    st.counts[CBG_SPMV_ROWS_GROUP] += pd.rows - (int64_t)pd.host[1] - (int64_t)pd.host[2];
    pd.rows = 0;
    st.counts[CBG_SPMV_ROWS_WAVE] += (int64_t)pd.host[1];
    st.counts[CBG_SPMV_ROWS_LONG] += (int64_t)pd.host[2];
    st.counts[CBG_SPMV_CHUNKS] += (int64_t)pd.host[3];
    float ms = 0;
    if (hipEventElapsedTime(&ms, pd.e0, pd.e1) == hipSuccess) st.ms += ms;
  }
}
template <class T>
void keep(Pending& pd, DBuf<T>& b) {
  if (b.p) pd.blocks.push_back(b.detach());
}

// the three classes over the rows of src; everything is queued on s, the temporaries go to pd
template <int SR, class S>
void reduce_rows(const S& src, int64_t entries, u64* stat, Pending& pd, hipStream_t s) {
  const int64_t nrows = src.nrows;
  if (nrows <= 0) return;
  DBuf<int32_t> waveq(nrows);
  DBuf<int64_t> cls(nrows + 1), pre(nrows + 2);
  // chunks: sum of ceil(L / 4096) over the rows of L > 4096 <= entries / 4096 + entries / 4097
  DBuf<double> partial(2 * (entries / SPMV_WAVE) + 2);
  hipLaunchKernelGGL((k_spmv_group<SR, S>), dim3(nblk(nrows, GROUPS)), dim3(256), 0, s, src, cls.p);
  pd.rows += nrows;
  DeferredFree df;
  exclusive_scan_i64(cls.p, pre.p, nrows, s, &df);
  for (void* q : df.ptrs) pd.blocks.push_back(q);
  df.ptrs.clear();
  hipLaunchKernelGGL(k_spmv_queue, dim3(nblk(nrows, 256)), dim3(256), 0, s, nrows, cls.p, pre.p, waveq.p, stat);
  // enough waves to fill the device; a queue of fewer rows leaves the others idle
  hipLaunchKernelGGL((k_spmv_wave<SR, S>), dim3(nblk(std::min<int64_t>(nrows, 16384), WAVES)), dim3(256), 0, s, src, waveq.p,
                     stat);
  if (entries > SPMV_WAVE) {  // else no row is long
    const int64_t cw = std::min<int64_t>(2 * (entries / SPMV_WAVE) + 1, 16384);
    hipLaunchKernelGGL((k_spmv_chunk<SR, S>), dim3(nblk(cw, WAVES)), dim3(256), 0, s, src, pre.p, partial.p);
    hipLaunchKernelGGL((k_spmv_long_fold<SR, S>), dim3(nblk(nrows, 256)), dim3(256), 0, s, src, pre.p, partial.p);
  }
  CBG_HIP(hipGetLastError());
  keep(pd, waveq);
  keep(pd, cls);
  keep(pd, pre);
  keep(pd, partial);
}

// events and the stat words around `body`; the call's statistics are read when they are asked for
template <class F>
void timed(hipStream_t s, F&& body) {
  pending_resolve();
  Pending& pd = pending();
  if (!pd.e0) {
    CBG_HIP(hipEventCreate(&pd.e0));
    CBG_HIP(hipEventCreate(&pd.e1));
    CBG_HIP(hipHostMalloc(reinterpret_cast<void**>(&pd.host), sizeof(u64) * 4, hipHostMallocDefault));
  }
  DBuf<u64> stat(4);
  CBG_HIP(hipMemsetAsync(stat.p, 0, sizeof(u64) * 4, s));
  CBG_HIP(hipEventRecord(pd.e0, s));
  pd.waiting = true;  // from here on the blocks are released through pending_resolve
  pd.rows = 0;
  pd.host[0] = pd.host[1] = pd.host[2] = pd.host[3] = 0;
  try {
    body(stat.p, pd);
  } catch (...) {
    (void)hipStreamSynchronize(s);
    keep(pd, stat);
    (void)hipEventRecord(pd.e1, s);
    try {
      pending_resolve();
    } catch (...) {
    }
    throw;
  }
  // the event the statistics wait for comes after the copy of the stat words
  CBG_HIP(hipMemcpyAsync(pd.host, stat.p, sizeof(u64) * 4, hipMemcpyDeviceToHost, s));
  CBG_HIP(hipEventRecord(pd.e1, s));
  keep(pd, stat);
}
}  // namespace

SpmvStats& spmv_stats() {
  pending_resolve();
  return raw_stats();
}
void spmv_stats_reset() {
  pending_resolve();
  raw_stats() = SpmvStats{};
}

int spmv_bounds(int64_t* bounds, int n) {
  const int64_t b[3] = {SPMV_GROUP, SPMV_WAVE, EXPAND_UNIT};
  for (int i = 0; bounds && i < n && i < 3; ++i) bounds[i] = b[i];
  return 3;
}

double spmv_identity(int sr) { return sr == CBG_MIN_PLUS ? DBL_MAX : 0.0; }

// y (device, At.n doubles) = A x with x (device, At.m doubles); queued on s, nothing waits
void tile_spmv_device(const cbg_tile& At, int sr, const double* x, double* y, hipStream_t s) {
  timed(s, [&](u64* stat, Pending& pd) {
    fill_device(y, At.n, spmv_identity(sr), s);
    if (At.nnz <= 0 || At.nzc <= 0) return;
    if (sr == CBG_MIN_PLUS)
      reduce_rows<1>(DenseRows<1>{At.nzc, At.cp, At.jc, At.ir, At.val, x, y}, At.nnz, stat, pd, s);
    else
      reduce_rows<0>(DenseRows<0>{At.nzc, At.cp, At.jc, At.ir, At.val, x, y}, At.nnz, stat, pd, s);
  });
}

void spmv_combine_device(double* y, const double* all, int P, int64_t lm, int sr, hipStream_t s) {
  if (sr == CBG_MIN_PLUS) fold_blocks(y, all, P, lm, SemAdd<1>{}, s);
  else fold_blocks(y, all, P, lm, SemAdd<0>{}, s);
}

// the sparse product: host vectors in and out; synchronizes s
void tile_spmspv(const cbg_tile& A, int sr, const int64_t* xind, const double* xval, int64_t nx, int64_t* yind, double* yval,
                 int64_t* ny, hipStream_t s) {
  *ny = 0;
  if (nx <= 0 || A.nnz <= 0 || A.nzc <= 0 || A.m <= 0) return;
  std::vector<int32_t> fl_h((size_t)nx);
  for (int64_t k = 0; k < nx; ++k) fl_h[k] = (int32_t)xind[k];
  const int64_t n1 = std::max<int64_t>(A.n, 1);
  DBuf<int32_t> pos(n1), fl(nx);
  DBuf<int64_t> len(n1);
  DBuf<double> xv(nx);
  ExpandPlan plan;
  int64_t nseg = 0;
  std::vector<uint32_t> yi;
  bool ran = false;
  timed(s, [&](u64* stat, Pending& pd) {
    DBuf<uint32_t> key, oi;
    DBuf<double> pv, ov;
    DBuf<int32_t> head;
    DBuf<int64_t> seg, start;
    DeferredFree df2;
    WaitOnThrow wait{s};  // declared after the buffers, so it runs first
    tile_col_map(A, pos.p, len.p, s);
    CBG_HIP(hipMemcpyAsync(fl.p, fl_h.data(), sizeof(int32_t) * nx, hipMemcpyHostToDevice, s));
    CBG_HIP(hipMemcpyAsync(xv.p, xval, sizeof(double) * nx, hipMemcpyHostToDevice, s));
    expand_plan(fl.p, nx, len.p, true, plan, s);
    const int64_t products = plan.products;
    if (products <= 0) {
      wait.done = true;
      return;
    }
    key.reset(products);
    pv.reset(products);
    if (sr == CBG_MIN_PLUS)
      hipLaunchKernelGGL(k_spmspv_expand<1>, dim3(nblk(plan.units, WAVES)), dim3(256), 0, s, nx, fl.p, xv.p, pos.p, A.cp, A.ir,
                         A.val, plan.ustart, plan.pstart, plan.units, key.p, pv.p);
    else
      hipLaunchKernelGGL(k_spmspv_expand<0>, dim3(nblk(plan.units, WAVES)), dim3(256), 0, s, nx, fl.p, xv.p, pos.p, A.cp, A.ir,
                         A.val, plan.ustart, plan.pstart, plan.units, key.p, pv.p);
    CBG_HIP(hipGetLastError());
    radix_sort_pairs<uint32_t>(key, pv, products, low_bits(A.m - 1), s, &df2);
    head.reset(products + 1);
    seg.reset(products + 2);
    start.reset(std::min<int64_t>(products, A.m) + 2);
    hipLaunchKernelGGL(k_spmspv_heads, dim3(nblk(products, 256)), dim3(256), 0, s, key.p, products, head.p);
    exclusive_scan_i32_to_i64(head.p, seg.p, products, s, &df2);
    hipLaunchKernelGGL(k_spmspv_starts, dim3(nblk(products + 1, 256)), dim3(256), 0, s, key.p, products, seg.p, start.p);
    CBG_HIP(hipMemcpyAsync(&nseg, seg.p + products, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    CBG_HIP(hipStreamSynchronize(s));
    df2.synced = true;
    oi.reset(nseg);
    ov.reset(nseg);
    if (sr == CBG_MIN_PLUS)
      reduce_rows<1>(SortedRows<1>{nseg, start.p, key.p, pv.p, oi.p, ov.p}, products, stat, pd, s);
    else
      reduce_rows<0>(SortedRows<0>{nseg, start.p, key.p, pv.p, oi.p, ov.p}, products, stat, pd, s);
    yi.resize((size_t)nseg);
    CBG_HIP(hipMemcpyAsync(yi.data(), oi.p, sizeof(uint32_t) * nseg, hipMemcpyDeviceToHost, s));
    CBG_HIP(hipMemcpyAsync(yval, ov.p, sizeof(double) * nseg, hipMemcpyDeviceToHost, s));
    CBG_HIP(hipStreamSynchronize(s));
    ran = true;
    wait.done = true;
  });
  CBG_HIP(hipStreamSynchronize(s));
  SpmvStats& st = spmv_stats();
  st.counts[CBG_SPMV_UNITS] += plan.units;
  st.counts[CBG_SPMV_PRODUCTS] += plan.products;
  if (!ran) return;
  for (int64_t k = 0; k < nseg; ++k) yind[k] = yi[k];
  *ny = nseg;
  st.counts[CBG_SPMV_ENTRIES_OUT] += nseg;
}

// the partial entries of a grid row's ranks, concatenated in rank order (n of them, rows below m):
// stable sort by row and a sequential fold of each row's entries; host arrays; -> the entries out
int64_t spmspv_combine(const int64_t* ind, const double* val, int64_t n, int64_t m, int sr, int64_t* oind, double* oval,
                       hipStream_t s) {
  if (n <= 0) return 0;
  std::vector<uint32_t> k_h((size_t)n);
  for (int64_t i = 0; i < n; ++i) k_h[i] = (uint32_t)ind[i];
  DBuf<uint32_t> key(n), uk(n);
  DBuf<double> v(n), uv(n);
  CBG_HIP(hipMemcpyAsync(key.p, k_h.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, s));
  CBG_HIP(hipMemcpyAsync(v.p, val, sizeof(double) * n, hipMemcpyHostToDevice, s));
  radix_sort_pairs<uint32_t>(key, v, n, low_bits(m - 1), s);
  const int64_t runs = reduce_by_key<uint32_t>(key.p, v.p, n, sr, uk.p, uv.p, s);
  CBG_HIP(hipMemcpyAsync(k_h.data(), uk.p, sizeof(uint32_t) * runs, hipMemcpyDeviceToHost, s));
  CBG_HIP(hipMemcpyAsync(oval, uv.p, sizeof(double) * runs, hipMemcpyDeviceToHost, s));
  CBG_HIP(hipStreamSynchronize(s));
  for (int64_t i = 0; i < runs; ++i) oind[i] = k_h[i];
  return runs;
}

}  // namespace cbg
