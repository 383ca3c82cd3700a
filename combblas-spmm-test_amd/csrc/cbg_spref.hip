// cbg_spref.hip -- sparse indexing B(i, j) = A(ri[i], ci[j]) on device DCSC tiles:
// SpDCCols::operator()(ri, ci) (SpDCCols.cpp:1355-1383) and the local work of
// SpParMat::SubsRef_SR (SpParMat.cpp:2026-2247).  The reference multiplies by two
// boolean selection matrices; here the entries are relabelled and moved, never
// computed with: every value keeps its bits.
//
//   column stage  column j of the result is column ci[j] of its owner: lengths of the
//                 requested columns, a scan, one copy per source tile (a column asked
//                 for k times is copied k times).  No sort.
//   row stage     the inverse of ri on this rank's new row block (for every old row the
//                 new rows that ask for it: a counting sort of ri), then every entry
//                 (a, j) emits (i, j) for each i of a's list: count per column, scan,
//                 scatter.
//   column sort   rows ascending in every column, values carried, in place, by column
//                 length: <= 256 one wave (4 keys per lane in registers, bitonic with
//                 cross-lane exchanges), <= 2048 one 256-thread block in LDS, longer
//                 ones together through radix_sort_pairs on (column, row) keys.
//                 Skipped when ri is strictly increasing: rows stay ascending.
//
// The grid-level logic (who broadcasts what, the agreements) is in cbg_grid_algos.cpp.
#include <algorithm>
#include <chrono>
#include <cstring>

#include "cbg_rebuild.h"

namespace cbg {

SprefStats& spref_stats() {
  static thread_local SprefStats s;
  return s;
}

namespace {
// A wave sorts 4 keys per lane: 12 VGPRs of payload, the whole network on the VALU.
constexpr int SORT_WAVE_MAX = 256;
// 2048 entries are 24 KiB of LDS (4-byte row ids, 8-byte values): six 256-thread blocks
// share a CU's 160 KiB, 24 waves per CU, enough to hide the column's load and store
// behind the other blocks' LDS passes.  4096 would halve that for columns R-MAT rarely has.
constexpr int SORT_LDS_MAX = 2048;
constexpr int PAD_KEY = 0x7FFFFFFF;  // sorts after every row id (local rows < 2^31 - 1)

// ---------------------------------------------------------------------------
// column stage
// ---------------------------------------------------------------------------
// owner of global column c in a communicator of np ranks with blocks of `per` (the last longer)
__device__ __forceinline__ int owner_of(int64_t c, int64_t per, int np, int64_t* local) {
  int q = per > 0 ? (int)min((int64_t)(np - 1), c / per) : np - 1;
  *local = c - (int64_t)q * per;
  return q;
}

// len[j] = stored length of global column sel[j]; cnt: np blocks of `stride` column counts
__global__ void k_sel_len(int64_t nsel, const int64_t* __restrict__ sel, const int32_t* __restrict__ cnt,
                          int64_t stride, int64_t per, int np, int64_t* __restrict__ len) {
  const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (j >= nsel) return;
  int64_t lc;
  const int q = owner_of(sel[j], per, np, &lc);
  len[j] = cnt[(int64_t)q * stride + lc];
}

// one wave per requested column: the columns that rank q owns are copied from its tile
__global__ __launch_bounds__(256) void k_sel_copy(int64_t nsel, const int64_t* __restrict__ sel, int q, int64_t per,
                                                  int np, const int32_t* __restrict__ pos,
                                                  const int64_t* __restrict__ cp, const int32_t* __restrict__ ir,
                                                  const double* __restrict__ val, const int64_t* __restrict__ ocp,
                                                  int32_t* __restrict__ oir, double* __restrict__ oval) {
  const int64_t j = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / WAVE;
  if (j >= nsel) return;
  int64_t lc;
  if (owner_of(sel[j], per, np, &lc) != q) return;
  const int32_t k = pos[lc];
  if (k < 0) return;
  const int64_t a = cp[k], len = cp[k + 1] - a, dst = ocp[j];
  for (int64_t i = lane_id(); i < len; i += WAVE) {
    st_stream(oir + dst + i, ld_stream(ir + a + i));
    st_stream(oval + dst + i, ld_stream(val + a + i));
  }
}

// ---------------------------------------------------------------------------
// row stage
// ---------------------------------------------------------------------------
__global__ void k_inv_count(int64_t n, const int64_t* __restrict__ ri, int32_t* __restrict__ cnt) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(cnt + ri[i], 1);
}
// the order inside a list is left to the atomics: the column sort orders the rows
// (a strictly increasing ri has lists of one entry)
__global__ void k_inv_fill(int64_t n, const int64_t* __restrict__ ri, const int64_t* __restrict__ start,
                           int32_t* __restrict__ fill, int32_t* __restrict__ list) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t r = ri[i];
  list[start[r] + atomicAdd(fill + r, 1)] = (int32_t)i;
}

// one wave per stored column: len[k] = new entries of column k
__global__ __launch_bounds__(256) void k_expand_count(int64_t nzc, const int64_t* __restrict__ cp,
                                                      const int32_t* __restrict__ ir, int64_t row0,
                                                      const int32_t* __restrict__ cnt, int64_t* __restrict__ len) {
  const int64_t k = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / WAVE;
  if (k >= nzc) return;
  const int64_t a = cp[k], b = cp[k + 1];
  long long s = 0;
  for (int64_t i = a + lane_id(); i < b; i += WAVE) s += cnt[row0 + ir[i]];
  s = wave_sum64(s);
  if (lane_id() == 0) len[k] = s;
}

// a wave per stored column: every entry writes its list's rows at the column's running offset
struct EmitExpanded {
  const int64_t* cp;
  const int32_t* ir;
  const double* val;
  int64_t row0;
  const int32_t* cnt;
  const int64_t* start;
  const int32_t* list;
  __device__ __forceinline__ void operator()(int64_t k, int64_t dst, int32_t* oir, double* oval) const {
    const int64_t a = cp[k], b = cp[k + 1];
    for (int64_t i0 = a; i0 < b; i0 += WAVE) {  // the trip count is the wave's: no lane leaves early
      const int64_t i = i0 + lane_id();
      int64_t r = 0;
      int c = 0;
      double v = 0.0;
      if (i < b) {
        r = row0 + ld_stream(ir + i);
        c = cnt[r];
        v = ld_stream(val + i);
      }
      const int incl = wave_incl_scan(c);
      const int64_t at = dst + (incl - c);
      const int64_t from = c ? start[r] : 0;
      for (int t = 0; t < c; ++t) {
        st_stream(oir + at + t, list[from + t]);
        st_stream(oval + at + t, v);
      }
      dst += wave_last(incl);
    }
  }
};

// ---------------------------------------------------------------------------
// column sort
// ---------------------------------------------------------------------------
// counts[c] += columns of class c (0 wave, 1 LDS, 2 long; fewer than 2 entries: none);
// the long columns' (position, length) pairs are appended to `longs`
__global__ void k_sort_classify(int64_t nzc, const int64_t* __restrict__ cp, unsigned long long* __restrict__ counts,
                                int64_t* __restrict__ longs) {
  const int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t len = k < nzc ? cp[k + 1] - cp[k] : 0;
  const int cls = len < 2 ? -1 : len <= SORT_WAVE_MAX ? 0 : len <= SORT_LDS_MAX ? 1 : 2;
  for (int c = 0; c < 2; ++c) {
    const unsigned long long m = __ballot(cls == c);
    if (lane_id() == 0 && m) atomicAdd(counts + c, (unsigned long long)__popcll(m));
  }
  if (cls == 2) {
    const unsigned long long at = atomicAdd(counts + 2, 1ull);
    longs[2 * at] = k;
    longs[2 * at + 1] = len;
  }
}

// ascending bitonic network over the 64 * R (key, value) pairs of a wave, element
// e = r * 64 + lane in register r; only the stages up to n2 (a power of two that
// covers the real elements, which fill a prefix) are run
template <int R>
__device__ __forceinline__ void wave_sort_regs(int (&key)[R], double (&val)[R], int lane, int n2) {
#pragma unroll
  for (int k = 2; k <= WAVE * R; k <<= 1) {
    if (k > n2) continue;  // the wave's decision; no early exit, so the loops unroll and the registers stay registers
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= WAVE) {
        const int jr = j / WAVE;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          if (r & jr) continue;
          const int p = r | jr;
          const bool up = ((r * WAVE + lane) & k) == 0;
          if ((key[r] > key[p]) == up) {
            const int tk = key[r];
            key[r] = key[p];
            key[p] = tk;
            const double tv = val[r];
            val[r] = val[p];
            val[p] = tv;
          }
        }
      } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int ok = xor_lane_d(key[r], j);
          const double ov = xor_lane_d(val[r], j);
          const bool up = ((r * WAVE + lane) & k) == 0;
          const bool lower = (lane & j) == 0;
          if (lower == up ? ok < key[r] : ok > key[r]) {
            key[r] = ok;
            val[r] = ov;
          }
        }
      }
    }
  }
}

template <int R>
__device__ __forceinline__ void wave_sort_column(int32_t* __restrict__ ir, double* __restrict__ val, int64_t a, int len,
                                                 int n2) {
  const int lane = lane_id();
  int key[R];
  double v[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = r * WAVE + lane;
    key[r] = e < len ? ld_stream(ir + a + e) : PAD_KEY;
    v[r] = e < len ? ld_stream(val + a + e) : 0.0;
  }
  wave_sort_regs<R>(key, v, lane, n2);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int e = r * WAVE + lane;
    if (e < len) {
      st_stream(ir + a + e, key[r]);
      st_stream(val + a + e, v[r]);
    }
  }
}

// one wave per column of 2 ... 256 entries; 1, 2 or 4 keys per lane by the length
__global__ __launch_bounds__(256) void k_sort_wave(int64_t nzc, const int64_t* __restrict__ cp, int32_t* __restrict__ ir,
                                                   double* __restrict__ val) {
  const int64_t k = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / WAVE;
  if (k >= nzc) return;
  const int64_t a = cp[k], len64 = cp[k + 1] - a;
  if (len64 < 2 || len64 > SORT_WAVE_MAX) return;
  const int len = (int)len64;
  int n2 = 2;
  while (n2 < len) n2 <<= 1;
  if (len <= WAVE)
    wave_sort_column<1>(ir, val, a, len, n2);
  else if (len <= 2 * WAVE)
    wave_sort_column<2>(ir, val, a, len, n2);
  else
    wave_sort_column<4>(ir, val, a, len, n2);
}

// one block per column of 257 ... 2048 entries, sorted in LDS
__global__ __launch_bounds__(256) void k_sort_lds(int64_t nzc, const int64_t* __restrict__ cp, int32_t* __restrict__ ir,
                                                  double* __restrict__ val) {
  __shared__ int keys[SORT_LDS_MAX];
  __shared__ double vals[SORT_LDS_MAX];
  const int64_t k = blockIdx.x;
  if (k >= nzc) return;
  const int64_t a = cp[k], len64 = cp[k + 1] - a;
  if (len64 <= SORT_WAVE_MAX || len64 > SORT_LDS_MAX) return;  // the block's decision: no barrier is split
  const int len = (int)len64, tid = threadIdx.x;
  int n2 = 512;
  while (n2 < len) n2 <<= 1;
  for (int e = tid; e < n2; e += 256) {
    keys[e] = e < len ? ld_stream(ir + a + e) : PAD_KEY;
    vals[e] = e < len ? ld_stream(val + a + e) : 0.0;
  }
  __syncthreads();
  for (int kk = 2; kk <= n2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int idx = tid; idx < n2 / 2; idx += 256) {
        const int i = 2 * idx - (idx & (j - 1)), l = i + j;
        const int ki = keys[i], kl = keys[l];
        const bool up = (i & kk) == 0;
        if ((ki > kl) == up) {
          keys[i] = kl;
          keys[l] = ki;
          const double t = vals[i];
          vals[i] = vals[l];
          vals[l] = t;
        }
      }
      __syncthreads();
    }
  }
  for (int e = tid; e < len; e += 256) {
    st_stream(ir + a + e, keys[e]);
    st_stream(val + a + e, vals[e]);
  }
}

// long columns: (index in the list << 32 | row) keys and values gathered end to end, and back
__global__ __launch_bounds__(256) void k_long_move(int64_t nlong, int64_t x0, const int64_t* __restrict__ longs,
                                                   const int64_t* __restrict__ off, const int64_t* __restrict__ cp,
                                                   int32_t* __restrict__ ir, double* __restrict__ val,
                                                   unsigned long long* __restrict__ keys, double* __restrict__ kv,
                                                   int back) {
  const int64_t x = x0 + blockIdx.y;
  if (x >= nlong) return;
  const int64_t a = cp[longs[2 * x]], len = longs[2 * x + 1], o = off[x];
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < len; e += (int64_t)gridDim.x * blockDim.x) {
    if (back) {
      st_stream(ir + a + e, (int32_t)(keys[o + e] & 0xffffffffull));
      st_stream(val + a + e, kv[o + e]);
    } else {
      keys[o + e] = ((unsigned long long)x << 32) | (unsigned)ld_stream(ir + a + e);
      kv[o + e] = ld_stream(val + a + e);
    }
  }
}

struct EvTimer {  // device ms between two points of a stream
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t s;
  explicit EvTimer(hipStream_t st) : s(st) {
    CBG_HIP(hipEventCreate(&e0));
    CBG_HIP(hipEventCreate(&e1));
    CBG_HIP(hipEventRecord(e0, s));
  }
  double stop() {
    float ms = 0;
    CBG_HIP(hipEventRecord(e1, s));
    CBG_HIP(hipEventSynchronize(e1));
    CBG_HIP(hipEventElapsedTime(&ms, e0, e1));
    return ms;
  }
  ~EvTimer() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};
}  // namespace

int spref_sort_bounds(int64_t* bounds, int n) {
  const int64_t b[2] = {SORT_WAVE_MAX, SORT_LDS_MAX};
  for (int i = 0; bounds && i < n && i < 2; ++i) bounds[i] = b[i];
  return 2;
}

void spref_sel_lengths(const int64_t* sel, int64_t nsel, const int32_t* cnt, int64_t stride, int64_t per, int np,
                       int64_t* len, hipStream_t s) {
  if (nsel > 0)
    hipLaunchKernelGGL(k_sel_len, dim3(nblk(nsel, 256)), dim3(256), 0, s, nsel, sel, cnt, stride, per, np, len);
}

void spref_sel_copy(const cbg_tile& src, int q, int64_t per, int np, const int64_t* sel, int64_t nsel,
                    const int64_t* ocp, int32_t* oir, double* oval, hipStream_t s) {
  if (nsel == 0 || src.nzc == 0) return;
  DBuf<int32_t> pos(std::max<int64_t>(src.n, 1));
  tile_col_map(src, pos.p, nullptr, s);
  hipLaunchKernelGGL(k_sel_copy, dim3(nblk(nsel * WAVE, 256)), dim3(256), 0, s, nsel, sel, q, per, np, pos.p, src.cp,
                     src.ir, src.val, ocp, oir, oval);
  CBG_HIP(hipStreamSynchronize(s));  // pos is released
}

// out takes over ir and val (nnz entries laid out by the dense offsets cp[0 .. ncols]);
// ids: the column ids of the ncols offsets (NULL: 0, 1, ...)
void spref_compact(int64_t m, int64_t n, const int32_t* ids, int64_t ncols, const int64_t* cp, DBuf<int32_t>& ir,
                   DBuf<double>& val, int64_t nnz, cbg_tile& out, hipStream_t s) {
  if (ir.n == 0) ir.reset(1);
  if (val.n == 0) val.reset(1);
  DeferredFree df;
  TileGuard o;
  compact_columns(m, n, nnz, ncols, ids, cp, o.t, s, df);
  CBG_HIP(hipStreamSynchronize(s));
  df.synced = true;
  o.t.ir = ir.detach();
  o.t.val = val.detach();
  out = o.release();
}

// the requested columns sel[0 .. nsel) (device, global ids) of ONE tile that holds them all
void spref_select_cols(const cbg_tile& T, const int64_t* sel_host, int64_t nsel, cbg_tile& out, hipStream_t s) {
  DBuf<int64_t> sel(std::max<int64_t>(nsel, 1)), len(nsel + 1), ocp(nsel + 1);
  DBuf<int32_t> cnt(std::max<int64_t>(T.n, 1));
  if (nsel) CBG_HIP(hipMemcpyAsync(sel.p, sel_host, sizeof(int64_t) * nsel, hipMemcpyHostToDevice, s));
  tile_counts_device(T, 0, cnt.p, std::max<int64_t>(T.n, 1), s);
  spref_sel_lengths(sel.p, nsel, cnt.p, T.n, T.n, 1, len.p, s);
  exclusive_scan_i64(len.p, ocp.p, nsel, s);
  int64_t nnz = 0;
  CBG_HIP(hipMemcpyAsync(&nnz, ocp.p + nsel, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  CBG_HIP(hipStreamSynchronize(s));
  DBuf<int32_t> oir(std::max<int64_t>(nnz, 1));
  DBuf<double> oval(std::max<int64_t>(nnz, 1));
  spref_sel_copy(T, 0, T.n, 1, sel.p, nsel, ocp.p, oir.p, oval.p, s);
  spref_compact(T.m, nsel, nullptr, nsel, ocp.p, oir, oval, nnz, out, s);
}

// ri[0 .. n): the old GLOBAL rows (all below gm) that the rank's new rows 0 .. n-1 ask for
void spref_build_inverse(const int64_t* ri_host, int64_t n, int64_t gm, RowInverse& inv, hipStream_t s) {
  DBuf<int64_t> ri(std::max<int64_t>(n, 1));
  DBuf<int32_t> fill(gm + 1);
  inv.cnt.reset(gm + 1);
  inv.start.reset(gm + 1);
  inv.list.reset(std::max<int64_t>(n, 1));
  CBG_HIP(hipMemsetAsync(inv.cnt.p, 0, sizeof(int32_t) * (gm + 1), s));
  CBG_HIP(hipMemsetAsync(fill.p, 0, sizeof(int32_t) * (gm + 1), s));
  if (n) {
    CBG_HIP(hipMemcpyAsync(ri.p, ri_host, sizeof(int64_t) * n, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_inv_count, dim3(nblk(n, 256)), dim3(256), 0, s, n, ri.p, inv.cnt.p);
  }
  exclusive_scan_i32_to_i64(inv.cnt.p, inv.start.p, gm, s);
  if (n) hipLaunchKernelGGL(k_inv_fill, dim3(nblk(n, 256)), dim3(256), 0, s, n, ri.p, inv.start.p, fill.p, inv.list.p);
  CBG_HIP(hipStreamSynchronize(s));
}

// X's rows are the old global rows row0 ... row0 + X.m - 1; out has new_m rows, unsorted columns
void spref_expand_rows(const cbg_tile& X, int64_t row0, const RowInverse& inv, int64_t new_m, cbg_tile& out,
                       hipStream_t s) {
  const int64_t nzc = X.nzc;
  DBuf<int64_t> len(nzc + 1);
  if (nzc)
    hipLaunchKernelGGL(k_expand_count, dim3(nblk(nzc * WAVE, 256)), dim3(256), 0, s, nzc, X.cp, X.ir, row0, inv.cnt.p,
                       len.p);
  tile_from_columns(new_m, X.n, nzc, X.jc, len.p,
                    EmitExpanded{X.cp, X.ir, X.val, row0, inv.cnt.p, inv.start.p, inv.list.p}, out, s);
}

// rows ascending in every column of t, values carried, in place
void spref_sort_columns(cbg_tile& t, hipStream_t s) {
  SprefStats& st = spref_stats();
  if (t.nzc == 0 || t.nnz < 2) return;
  EvTimer tm(s);
  const int64_t cap = t.nnz / (SORT_LDS_MAX + 1) + 1;
  DBuf<unsigned long long> counts(3);
  DBuf<int64_t> longs(2 * cap);
  CBG_HIP(hipMemsetAsync(counts.p, 0, sizeof(unsigned long long) * 3, s));
  hipLaunchKernelGGL(k_sort_classify, dim3(nblk(t.nzc, 256)), dim3(256), 0, s, t.nzc, t.cp, counts.p, longs.p);
  unsigned long long c[3] = {0, 0, 0};
  CBG_HIP(hipMemcpyAsync(c, counts.p, sizeof(c), hipMemcpyDeviceToHost, s));
  CBG_HIP(hipStreamSynchronize(s));
  if (c[0]) hipLaunchKernelGGL(k_sort_wave, dim3(nblk(t.nzc * WAVE, 256)), dim3(256), 0, s, t.nzc, t.cp, t.ir, t.val);
  if (c[1]) {
    // one block per stored column, in launches of at most 2^30 blocks
    for (int64_t k0 = 0; k0 < t.nzc; k0 += (int64_t)1 << 30) {
      const int64_t nb = std::min<int64_t>(t.nzc - k0, (int64_t)1 << 30);
      hipLaunchKernelGGL(k_sort_lds, dim3((unsigned)nb), dim3(256), 0, s, nb, t.cp + k0, t.ir, t.val);
    }
  }
  if (c[2]) {
    const int64_t nlong = (int64_t)c[2];
    if (nlong > cap) throw HipError("spref sort: long-column list overflow", CBG_ERR_HIP);
    std::vector<int64_t> h((size_t)2 * nlong), off((size_t)nlong + 1);
    CBG_HIP(hipMemcpy(h.data(), longs.p, sizeof(int64_t) * 2 * nlong, hipMemcpyDeviceToHost));
    std::vector<std::pair<int64_t, int64_t>> pl((size_t)nlong);
    for (int64_t i = 0; i < nlong; ++i) pl[i] = {h[2 * i], h[2 * i + 1]};
    std::sort(pl.begin(), pl.end());
    int64_t total = 0, longest = 0;
    for (int64_t i = 0; i < nlong; ++i) {
      h[2 * i] = pl[i].first;
      h[2 * i + 1] = pl[i].second;
      off[i] = total;
      total += pl[i].second;
      longest = std::max(longest, pl[i].second);
    }
    off[nlong] = total;
    DBuf<int64_t> doff(nlong + 1);
    CBG_HIP(hipMemcpyAsync(longs.p, h.data(), sizeof(int64_t) * 2 * nlong, hipMemcpyHostToDevice, s));
    CBG_HIP(hipMemcpyAsync(doff.p, off.data(), sizeof(int64_t) * (nlong + 1), hipMemcpyHostToDevice, s));
    DBuf<unsigned long long> keys(total);
    DBuf<double> kv(total);
    const unsigned bx = (unsigned)std::min<int64_t>((longest + 255) / 256, 1024);
    auto move = [&](int back) {  // the grid's y extent is 65535 at the most
      for (int64_t x0 = 0; x0 < nlong; x0 += 65535)
        hipLaunchKernelGGL(k_long_move, dim3(bx, (unsigned)std::min<int64_t>(nlong - x0, 65535)), dim3(256), 0, s,
                           nlong, x0, longs.p, doff.p, t.cp, t.ir, t.val, keys.p, kv.p, back);
    };
    move(0);
    // stable LSD passes over the bits the list index and the rows use: the columns stay end to end
    radix_sort_pairs<unsigned long long>(keys, kv, total, (low_bits(nlong - 1) << 32) | low_bits(t.m - 1), s);
    move(1);
    CBG_HIP(hipStreamSynchronize(s));  // h, off and the sort's buffers are released
  }
  st.ms[CBG_SPREF_MS_SORT] += tm.stop();
  CBG_HIP(hipStreamSynchronize(s));
  for (int i = 0; i < 3; ++i) st.counts[CBG_SPREF_SORT_CLASS0 + i] += (int64_t)c[i];
}

bool spref_strictly_increasing(const int64_t* v, int64_t n) {
  for (int64_t i = 1; i < n; ++i)
    if (v[i] <= v[i - 1]) return false;
  return true;
}

// SpDCCols::operator()(ri, ci) on one tile (ri / ci NULL: all, in order)
void tile_spref(const cbg_tile& T, const int64_t* ri, int64_t nri, const int64_t* ci, int64_t nci, cbg_tile& out,
                hipStream_t s) {
  SprefStats& st = spref_stats();
  st.counts[CBG_SPREF_ENTRIES_IN] += T.nnz;
  TileGuard X;
  {
    EvTimer tm(s);
    if (ci)
      spref_select_cols(T, ci, nci, X.t, s);
    else if (!ri)
      tile_slice_cols(T, 0, T.n, X.t, s);
    st.ms[CBG_SPREF_MS_COL] += tm.stop();
  }
  if (ri) {
    EvTimer tm(s);
    RowInverse inv;
    spref_build_inverse(ri, nri, T.m, inv, s);
    TileGuard Y;
    spref_expand_rows(ci ? X.t : T, 0, inv, nri, Y.t, s);
    X = std::move(Y);
    st.ms[CBG_SPREF_MS_ROW] += tm.stop();
    if (spref_strictly_increasing(ri, nri))
      st.counts[CBG_SPREF_COLS_MONOTONE] += X.t.nzc;
    else
      spref_sort_columns(X.t, s);
  }
  CBG_HIP(hipStreamSynchronize(s));
  CBG_HIP(hipGetLastError());  // a refused launch is this call's failure, not a later one's
  st.counts[CBG_SPREF_ENTRIES_OUT] += X.t.nnz;
  out = X.release();
}

}  // namespace cbg
