// cbg_bfs.hip -- matrix x sparse vector with SelectMaxSRing<bool,int64> (Semirings.h:190-210, the local
// kernel SpImpl.cpp:168-221) on a device DCSC tile, pushing and pulling, and the dense-vector steps of
// the single-source breadth-first search built on it (TopDownBFS.cpp:427-443, DirOptBFS.cpp:360-445).
//
// ORIENTATION: y = A x as in the reference.  A stored A(i, j) is the edge j -> i: column j lists what j
// reaches.  This is the transpose of what cbg_grid_betwcent calls A.  Values are never read.
//
//   push   The frontier is an ascending list of local columns.  A unit is (frontier entry, chunk of at
//          most EXPAND_UNIT entries of its column), one wave each, found by a search in the scan of the
//          units per entry (cbg_vector.h): one hub column still fills the device.  Every entry does one vector
//          atomicMax(&cand[row], value) on the dense candidate array (-1: none).  The atomics execute at
//          the memory side, so cand is not cached across them and needs no ordering: max is idempotent.
//   pull   At is the tile's transpose: its column i is row i of A with the column ids ascending.  A row
//          without a parent scans its entries from the last one downward and tests bit coff + j of the
//          frontier bitmap; the first hit is the maximum.  Rows of at most BFS_PULL_LANE entries take one
//          lane each (64 rows per wave); longer rows are queued (one slot atomic per wave) and take a wave
//          each: 64 entries per step from the end, a ballot, the highest hitting lane.  Every row writes
//          its own cand[i]: no atomics on cand, and exactly the push's values.
//   update new = candidate and no parent yet; parent and level written; the new frontier's bits of the row
//          block from the wave's ballot; their count.
//   compaction  the bits of this rank's column block -> the ascending list of local columns (ballot,
//          popcount, scan), the units of each, and pred = the summed lengths of those columns.
#include <algorithm>
#include <climits>

#include "cbg_vector.h"

namespace cbg {

BfsStats& bfs_stats() {
  static thread_local BfsStats s;
  return s;
}

namespace {
// The longest row one lane scans.  Its reads are not coalesced, so only rows that fit a couple of cache
// lines of row ids stay here; the serial scan of a longer row would also hold its wave back.
constexpr int BFS_PULL_LANE = 16;

__device__ __forceinline__ bool bit_at(const u64* __restrict__ bits, int64_t g) { return (bits[g >> 6] >> (g & 63)) & 1ull; }

// nu[k] = the units of column fl[k]; plen[k] (plen may be NULL) = its stored length
__global__ __launch_bounds__(256) void k_expand_units(int64_t nf, const int32_t* __restrict__ fl,
                                                      const int64_t* __restrict__ len, int64_t* __restrict__ plen,
                                                      int64_t* __restrict__ nu) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= nf) return;
  const int64_t n = len[fl[k]];
  if (plen) plen[k] = n;
  nu[k] = (n + EXPAND_UNIT - 1) / EXPAND_UNIT;
}

__device__ __forceinline__ void atomic_max(int32_t* p, int32_t v) { atomicMax(p, v); }
__device__ __forceinline__ void atomic_max(int64_t* p, int64_t v) {
  atomicMax(reinterpret_cast<long long*>(p), (long long)v);
}

// one wave per unit; xv == NULL: the value is the column id
template <class V>
__global__ __launch_bounds__(256) void k_bfs_push(int64_t nf, const int32_t* __restrict__ fl, const V* __restrict__ xv,
                                                  const int32_t* __restrict__ pos, const int64_t* __restrict__ cp,
                                                  const int32_t* __restrict__ ir, const int64_t* __restrict__ ustart,
                                                  int64_t units, V* __restrict__ cand) {
  const int64_t u = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (u >= units) return;
  const int64_t lo = unit_owner(ustart, nf, u);  // the unit's frontier entry
  const int32_t j = fl[lo];
  const int32_t p = pos[j];
  if (p < 0) return;  // not stored: it has no unit, so this is never taken
  const int64_t a0 = cp[p] + (u - ustart[lo]) * EXPAND_UNIT, a1 = min(a0 + EXPAND_UNIT, cp[p + 1]);
  const V v = xv ? xv[lo] : (V)j;
  for (int64_t x = a0 + lane_id(); x < a1; x += WAVE) atomic_max(cand + ld_stream(ir + x), v);
}

// stat: 0 rows scanned, 1 entries read, 2 rows queued for k_bfs_pull_long
__global__ __launch_bounds__(256) void k_bfs_pull_rows(int64_t nzc, const int64_t* __restrict__ cp,
                                                       const int32_t* __restrict__ jc, const int32_t* __restrict__ ir,
                                                       const u64* __restrict__ bits, int64_t coff,
                                                       const int64_t* __restrict__ parent,
                                                       const uint8_t* __restrict__ skip, int32_t* __restrict__ cand,
                                                       int32_t* __restrict__ longq, u64* __restrict__ stat) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool active = false, queued = false;
  long long read = 0;
  if (p < nzc) {
    const int32_t i = jc[p];
    active = !(parent && parent[i] >= 0) && !(skip && skip[i]);
    if (active) {
      const int64_t lo = cp[p], hi = cp[p + 1];
      if (hi - lo <= BFS_PULL_LANE) {
        for (int64_t x = hi - 1; x >= lo; --x) {
          const int32_t j = ir[x];
          ++read;
          if (bit_at(bits, coff + j)) {
            cand[i] = j;
            break;
          }
        }
      } else {
        queued = true;
      }
    }
  }
  // every lane of the wave is here
  const u64 ma = __ballot(active), mq = __ballot(queued);
  const long long rsum = wave_sum64(read);
  const int lane = lane_id();
  unsigned long long base = 0;
  if (lane == 0) {
    if (ma) atomicAdd(stat + 0, (unsigned long long)__popcll(ma));
    if (rsum) atomicAdd(stat + 1, (unsigned long long)rsum);
    if (mq) base = atomicAdd(stat + 2, (unsigned long long)__popcll(mq));
  }
  base = __shfl(base, 0);
  if (queued) longq[base + __popcll(mq & ((1ull << lane) - 1ull))] = (int32_t)p;
}

// one wave per queued row, the waves striding over the queue
__global__ __launch_bounds__(256) void k_bfs_pull_long(const int64_t* __restrict__ cp, const int32_t* __restrict__ jc,
                                                       const int32_t* __restrict__ ir, const u64* __restrict__ bits,
                                                       int64_t coff, int32_t* __restrict__ cand,
                                                       const int32_t* __restrict__ longq, u64* __restrict__ stat) {
  const int64_t nq = (int64_t)stat[2];
  const int lane = lane_id();
  const int64_t w0 = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  long long read = 0;
  for (int64_t q = w0; q < nq; q += (int64_t)gridDim.x * WAVES) {
    const int32_t p = longq[q];
    const int64_t lo = cp[p], hi = cp[p + 1];
    for (int64_t e = hi; e > lo; e -= WAVE) {  // the wave's trip count: every lane votes
      const int64_t x = e - WAVE + lane;
      int32_t j = -1;
      bool hit = false;
      if (x >= lo) {
        j = ir[x];
        hit = bit_at(bits, coff + j);
      }
      const u64 m = __ballot(hit);
      if (m) {
        const int top = 63 - __clzll((long long)m);  // the highest hitting lane holds the largest column
        if (lane == top) cand[jc[p]] = j;
        read += WAVE - top;
        break;
      }
      read += min((int64_t)WAVE, e - lo);
    }
  }
  if (lane == 0 && read) atomicAdd(stat + 1, (unsigned long long)read);
}

__global__ __launch_bounds__(256) void k_bfs_cand_global(const int32_t* __restrict__ cand, int64_t lm, int64_t coff,
                                                         int64_t* __restrict__ candg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < lm) candg[i] = cand[i] < 0 ? -1 : coff + cand[i];
}

struct MaxI64 {
  __device__ __forceinline__ int64_t operator()(int64_t a, int64_t b) const { return max(a, b); }
};

// rowbits: wb words; the grid covers wb * 64 rows
__global__ __launch_bounds__(256) void k_bfs_update(int64_t lm, const int64_t* __restrict__ candg,
                                                    int64_t* __restrict__ parent, int64_t* __restrict__ level,
                                                    int64_t lev, u64* __restrict__ rowbits, int64_t wb,
                                                    u64* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool isnew = false;
  if (i < lm) {
    const int64_t c = candg[i];
    isnew = c >= 0 && parent[i] < 0;
    if (isnew) {
      parent[i] = c;
      level[i] = lev;
    }
  }
  const u64 m = __ballot(isnew);
  if (lane_id() == 0 && (i >> 6) < wb) {
    rowbits[i >> 6] = m;
    if (m) atomicAdd(count, (unsigned long long)__popcll(m));
  }
}

// the frontier over all gn vertices from the pr row blocks' words (wb each, block q starts at q * per)
__global__ __launch_bounds__(256) void k_bfs_assemble(const u64* __restrict__ all, int pr, int64_t per, int64_t wb,
                                                      int64_t gn, u64* __restrict__ bits, int64_t wg) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool b = false;
  if (v < gn) {
    const int64_t q = per > 0 ? min(v / per, (int64_t)pr - 1) : pr - 1;
    const int64_t i = v - q * per;
    b = bit_at(all + q * wb, i);
  }
  const u64 m = __ballot(b);
  if (lane_id() == 0 && (v >> 6) < wg) bits[v >> 6] = m;
}

__global__ __launch_bounds__(256) void k_bfs_front_count(int64_t ln, const u64* __restrict__ bits, int64_t coff,
                                                         int64_t* __restrict__ cnt, int64_t nw) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const u64 m = __ballot(j < ln && bit_at(bits, coff + j));
  if (lane_id() == 0 && (j >> 6) < nw) cnt[j >> 6] = __popcll(m);
}

// stat: 0 the list's length, 1 pred, 2 units
__global__ __launch_bounds__(256) void k_bfs_front_emit(int64_t ln, const u64* __restrict__ bits, int64_t coff,
                                                        const int64_t* __restrict__ off, int64_t nw,
                                                        const int64_t* __restrict__ len, int32_t* __restrict__ fl,
                                                        int64_t* __restrict__ nu, u64* __restrict__ stat) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = j < ln && bit_at(bits, coff + j);
  const u64 m = __ballot(in);
  const int lane = lane_id();
  long long l = 0, units = 0;
  if (in) {
    const int64_t at = off[j >> 6] + __popcll(m & ((1ull << lane) - 1ull));
    l = len[j];
    units = (l + EXPAND_UNIT - 1) / EXPAND_UNIT;
    fl[at] = (int32_t)j;
    nu[at] = units;
  }
  const long long ls = wave_sum64(l), us = wave_sum64(units);
  if (lane == 0) {
    if (ls) atomicAdd(stat + 1, (unsigned long long)ls);
    if (us) atomicAdd(stat + 2, (unsigned long long)us);
    if (j == 0) stat[0] = (u64)off[nw];
  }
}
}  // namespace

int bfs_bounds(int64_t* bounds, int n) {
  const int64_t b[2] = {EXPAND_UNIT, BFS_PULL_LANE};
  for (int i = 0; bounds && i < n && i < 2; ++i) bounds[i] = b[i];
  return 2;
}

template <class V>
static void push_launch(const cbg_tile& A, const int32_t* pos, const int32_t* fl, const V* xv, int64_t nf,
                        const int64_t* ustart, int64_t units, V* cand, hipStream_t s) {
  if (units <= 0 || nf <= 0) return;
  hipLaunchKernelGGL(k_bfs_push<V>, dim3(nblk(units, WAVES)), dim3(256), 0, s, nf, fl, xv, pos, A.cp, A.ir, ustart, units,
                     cand);
  CBG_HIP(hipGetLastError());
}

void bfs_push_device(const cbg_tile& A, const int32_t* pos, const int32_t* fl, int64_t nf, const int64_t* ustart,
                     int64_t units, int32_t* cand, hipStream_t s) {
  push_launch<int32_t>(A, pos, fl, nullptr, nf, ustart, units, cand, s);
}

void bfs_pull_device(const cbg_tile& At, const u64* bits, int64_t coff, const int64_t* parent, const uint8_t* skip,
                     int32_t* cand, int32_t* longq, u64* stat, hipStream_t s) {
  if (At.nzc <= 0 || At.nnz <= 0) return;
  hipLaunchKernelGGL(k_bfs_pull_rows, dim3(nblk(At.nzc, 256)), dim3(256), 0, s, At.nzc, At.cp, At.jc, At.ir, bits, coff,
                     parent, skip, cand, longq, stat);
  // enough waves to fill the device; a queue of fewer rows leaves the others idle
  const int64_t waves = std::min<int64_t>(At.nzc, 16384);
  hipLaunchKernelGGL(k_bfs_pull_long, dim3(nblk(waves, WAVES)), dim3(256), 0, s, At.cp, At.jc, At.ir, bits, coff, cand,
                     longq, stat);
  CBG_HIP(hipGetLastError());
}

void bfs_cand_global(const int32_t* cand, int64_t lm, int64_t coff, int64_t* candg, hipStream_t s) {
  if (lm > 0) hipLaunchKernelGGL(k_bfs_cand_global, dim3(nblk(lm, 256)), dim3(256), 0, s, cand, lm, coff, candg);
  CBG_HIP(hipGetLastError());
}
void bfs_cand_max(int64_t* candg, const int64_t* all, int P, int64_t lm, hipStream_t s) {
  fold_blocks(candg, all, P, lm, MaxI64{}, s);
}
void bfs_update(int64_t lm, const int64_t* candg, int64_t* parent, int64_t* level, int64_t lev, u64* rowbits, int64_t wb,
                u64* count, hipStream_t s) {
  if (wb > 0)
    hipLaunchKernelGGL(k_bfs_update, dim3(nblk(wb * WAVE, 256)), dim3(256), 0, s, lm, candg, parent, level, lev, rowbits,
                       wb, count);
  CBG_HIP(hipGetLastError());
}
void bfs_assemble_bits(const u64* all, int pr, int64_t per, int64_t wb, int64_t gn, u64* bits, hipStream_t s) {
  const int64_t wg = (gn + 63) / 64;
  if (wg > 0) hipLaunchKernelGGL(k_bfs_assemble, dim3(nblk(wg * WAVE, 256)), dim3(256), 0, s, all, pr, per, wb, gn, bits, wg);
  CBG_HIP(hipGetLastError());
}

// fl / nu: room for ln; scratch: 2 * (ceil(ln / 64) + 1) int64; stat: 3 words, zeroed here
void bfs_compact(const u64* bits, int64_t coff, int64_t ln, const int64_t* len, int32_t* fl, int64_t* nu,
                 int64_t* scratch, u64* stat, hipStream_t s, DeferredFree& df) {
  CBG_HIP(hipMemsetAsync(stat, 0, sizeof(u64) * 3, s));
  if (ln <= 0) return;
  const int64_t nw = (ln + 63) / 64;
  int64_t *cnt = scratch, *off = scratch + nw + 1;
  hipLaunchKernelGGL(k_bfs_front_count, dim3(nblk(nw * WAVE, 256)), dim3(256), 0, s, ln, bits, coff, cnt, nw);
  exclusive_scan_i64(cnt, off, nw, s, &df);
  hipLaunchKernelGGL(k_bfs_front_emit, dim3(nblk(nw * WAVE, 256)), dim3(256), 0, s, ln, bits, coff, off, nw, len, fl, nu,
                     stat);
  CBG_HIP(hipGetLastError());
}

void expand_plan(const int32_t* fl, int64_t nf, const int64_t* len, bool products, ExpandPlan& pl, hipStream_t s) {
  const int64_t n1 = nf + 1;
  pl.buf.reset((products ? 4 : 2) * n1);
  int64_t *nu = pl.buf.p, *plen = products ? nu + 2 * n1 : nullptr;
  pl.ustart = nu + n1, pl.pstart = products ? nu + 3 * n1 : nullptr;
  pl.units = pl.products = 0;
  DeferredFree df;
  hipLaunchKernelGGL(k_expand_units, dim3(nblk(nf, 256)), dim3(256), 0, s, nf, fl, len, plen, nu);
  exclusive_scan_i64(nu, pl.ustart, nf, s, &df);
  CBG_HIP(hipMemcpyAsync(&pl.units, pl.ustart + nf, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  if (products) {
    exclusive_scan_i64(plen, pl.pstart, nf, s, &df);
    CBG_HIP(hipMemcpyAsync(&pl.products, pl.pstart + nf, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  }
  CBG_HIP(hipStreamSynchronize(s));
  df.synced = true;
}

namespace {
template <class V>
void spmspv_run(const cbg_tile& A, const std::vector<int32_t>& fl_h, const int64_t* xval, V none, std::vector<V>& cand_h,
                hipStream_t s) {
  const int64_t nf = (int64_t)fl_h.size(), m1 = std::max<int64_t>(A.m, 1), n1 = std::max<int64_t>(A.n, 1);
  DBuf<V> cand(m1), xv;
  DBuf<int32_t> pos(n1), fl(std::max<int64_t>(nf, 1));
  DBuf<int64_t> len(n1);
  ExpandPlan plan;
  WaitOnThrow wait{s};  // after the buffers
  fill_device(cand.p, m1, none, s);
  if (nf > 0 && A.nnz > 0 && A.nzc > 0) {
    tile_col_map(A, pos.p, len.p, s);
    CBG_HIP(hipMemcpyAsync(fl.p, fl_h.data(), sizeof(int32_t) * nf, hipMemcpyHostToDevice, s));
    if (xval) {
      xv.reset(nf);
      CBG_HIP(hipMemcpyAsync(xv.p, xval, sizeof(V) * nf, hipMemcpyHostToDevice, s));
    }
    expand_plan(fl.p, nf, len.p, false, plan, s);
    push_launch<V>(A, pos.p, fl.p, xv.p, nf, plan.ustart, plan.units, cand.p, s);
  }
  cand_h.resize((size_t)m1);
  CBG_HIP(hipMemcpyAsync(cand_h.data(), cand.p, sizeof(V) * m1, hipMemcpyDeviceToHost, s));
  CBG_HIP(hipStreamSynchronize(s));
  CBG_HIP(hipGetLastError());
  wait.done = true;
  bfs_stats().counts[CBG_BFS_PUSH_UNITS] += plan.units;
}
}  // namespace

void bfs_spmspv_max(const cbg_tile& A, const int64_t* xind, const int64_t* xval, int64_t nx, int64_t* yind,
                    int64_t* yval, int64_t* ny, hipStream_t s) {
  std::vector<int32_t> fl((size_t)nx);
  for (int64_t k = 0; k < nx; ++k) fl[k] = (int32_t)xind[k];
  int64_t out = 0;
  if (xval) {  // any int64 above the smallest is a value
    std::vector<int64_t> c;
    spmspv_run<int64_t>(A, fl, xval, INT64_MIN, c, s);
    for (int64_t i = 0; i < A.m; ++i)
      if (c[i] != INT64_MIN) yind[out] = i, yval[out++] = c[i];
  } else {
    std::vector<int32_t> c;
    spmspv_run<int32_t>(A, fl, nullptr, -1, c, s);
    for (int64_t i = 0; i < A.m; ++i)
      if (c[i] >= 0) yind[out] = i, yval[out++] = c[i];
  }
  *ny = out;
}

void bfs_pull_max(const cbg_tile& At, const int64_t* xind, int64_t nx, const uint8_t* skip, int64_t* yind,
                  int64_t* yval, int64_t* ny, int64_t* entries_read, hipStream_t s) {
  const int64_t rows = At.n, cols = At.m;  // of the untransposed tile
  const int64_t wg = std::max<int64_t>((cols + 63) / 64, 1), r1 = std::max<int64_t>(rows, 1);
  std::vector<u64> bits_h((size_t)wg, 0);
  for (int64_t k = 0; k < nx; ++k) bits_h[xind[k] >> 6] |= 1ull << (xind[k] & 63);
  std::vector<int32_t> c((size_t)r1);
  u64 stat_h[3] = {0, 0, 0};
  {
    DBuf<u64> bits(wg), stat(3);
    DBuf<int32_t> cand(r1), longq(std::max<int64_t>(At.nzc, 1));
    DBuf<uint8_t> sk;
    WaitOnThrow wait{s};
    CBG_HIP(hipMemcpyAsync(bits.p, bits_h.data(), sizeof(u64) * wg, hipMemcpyHostToDevice, s));
    CBG_HIP(hipMemsetAsync(stat.p, 0, sizeof(u64) * 3, s));
    CBG_HIP(hipMemsetAsync(cand.p, 0xff, sizeof(int32_t) * r1, s));
    if (skip && rows > 0) {
      sk.reset(rows);
      CBG_HIP(hipMemcpyAsync(sk.p, skip, rows, hipMemcpyHostToDevice, s));
    }
    bfs_pull_device(At, bits.p, 0, nullptr, sk.p, cand.p, longq.p, stat.p, s);
    CBG_HIP(hipMemcpyAsync(c.data(), cand.p, sizeof(int32_t) * r1, hipMemcpyDeviceToHost, s));
    CBG_HIP(hipMemcpyAsync(stat_h, stat.p, sizeof(u64) * 3, hipMemcpyDeviceToHost, s));
    CBG_HIP(hipStreamSynchronize(s));
    CBG_HIP(hipGetLastError());
    wait.done = true;
  }
  int64_t out = 0;
  for (int64_t i = 0; i < rows; ++i)
    if (c[i] >= 0) yind[out] = i, yval[out++] = c[i];
  *ny = out;
  if (entries_read) *entries_read = (int64_t)stat_h[1];
  bfs_stats().counts[CBG_BFS_PULL_ROWS] += (int64_t)stat_h[0];
  bfs_stats().counts[CBG_BFS_PULL_ENTRIES] += (int64_t)stat_h[1];
}

}  // namespace cbg
