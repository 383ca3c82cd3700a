// cbg_ewise.hip -- sparse element-wise ops of two device DCSC tiles of equal shape:
// EWiseMult / SetDifference (Friends.h:744-1030, SpDCCols.cpp:631-690, SpParMat.cpp:2781-2812).
//
//   CBG_EWISE_MULT     stored in both, value a * b
//   CBG_EWISE_FIRST    stored in both, value a (b is a mask)
//   CBG_EWISE_EXCLUDE  stored in a and not in b, value a
//
// The operands of BetwCent are a few hundred columns that may each hold the tile's whole
// row count, so a column is not the work unit: a unit is (stored column of a, chunk of at
// most EWISE_CHUNK of its entries), one wave each.  The unit looks its column up in b.jc,
// then searches b's column for the chunk's first row and for its last row plus one (a
// 64-bit bound): only that range of b can match.  By the range's length the unit
//   class 0  has nothing to match (no such column in b, or an empty range),
//   class 1  stages the range's row ids in its wave's LDS and searches there,
//   class 2  searches the range in global memory, entry by entry.
// b's values are read on a hit under MULT only.
//
// Frame: units per column -> scan (first unit of every column) -> count per unit, the kept
// entries of every 64 remembered as a ballot word -> ONE scan over the units' counts, which
// gives the entry offset of every unit and, read at the columns' first units, the dense
// column offsets -> compact_columns (cbg_rebuild.h, layer a; its readback also carries the
// totals and the class counts) -> emit per unit from the ballot words, in order.
#include <algorithm>

#include "cbg_rebuild.h"
#include "cbg_vector.h"

namespace cbg {

EwiseStats& ewise_stats() {
  static thread_local EwiseStats s;
  return s;
}

namespace {
// A unit's a-entries: 8 trips of a wave.  Long enough that the three searches a unit makes
// (its column, b's column, b's range) are noise, short enough that a scale-20 frontier column
// of 10^5 entries still gives 200 waves.
constexpr int EWISE_CHUNK = 512;
// The longest b range matched in LDS: 1280 row ids are 5 KiB per wave, 20 KiB per 256-thread
// block, so 8 blocks fill a CU's 160 KiB with 32 waves, the CU's whole wave count.  A range
// this long is a b 2.5 times denser than a over the chunk's rows; denser still goes to class 2.
constexpr int EWISE_LDS_RANGE = 1280;
constexpr int WORDS = EWISE_CHUNK / WAVE;  // ballot words per unit

struct Ew {
  int64_t anzc, bnzc;
  const int64_t *acp, *bcp;
  const int32_t *ajc, *bjc, *air, *bir;
  const double *aval, *bval;
  int op;
  int64_t umax;           // units launched: an upper bound of the real ones
  const int64_t* ustart;  // [anzc + 1] first unit of every stored column of a
  int64_t* cnt;           // [umax] kept entries of the unit
  int32_t* ucol;          // [umax] the unit's column (position in a.jc)
  int64_t *blo, *bhi;     // [umax] the unit's range of b
  u64* mask;              // [umax * WORDS] kept entries of every 64
  int64_t* stat;          // 0 nnz out, 1 .. 3 units of class 0 .. 2, 4 units
};

// first position in [lo, hi) of the ascending a[] that holds key or more (key may be 2^31 - 1)
__device__ __forceinline__ int64_t lower_row(const int32_t* __restrict__ a, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if ((int64_t)a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ void k_ewise_units(int64_t nzc, const int64_t* __restrict__ cp, int64_t* __restrict__ nu) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i < nzc) nu[i] = (cp[i + 1] - cp[i] + EWISE_CHUNK - 1) / EWISE_CHUNK;
}

// one wave per unit
__global__ __launch_bounds__(256) void k_ewise_count(Ew p) {
  __shared__ int32_t rows[WAVES][EWISE_LDS_RANGE];
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int64_t u = (int64_t)blockIdx.x * WAVES + w;
  if (u >= p.umax) return;
  const int lane = lane_id();
  if (u >= p.ustart[p.anzc]) {  // the scan runs over all umax counts
    if (lane == 0) p.cnt[u] = 0;
    return;
  }
  // the unit's column: the last i with ustart[i] <= u (written out: unit_owner costs this kernel 6 SGPRs)
  int64_t lo = 0, hi = p.anzc;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (p.ustart[mid] <= u) lo = mid;
    else hi = mid;
  }
  const int64_t i = lo;
  const int64_t a0 = p.acp[i] + (u - p.ustart[i]) * EWISE_CHUNK, a1 = min(a0 + EWISE_CHUNK, p.acp[i + 1]);
  // its column in b, and the range of it that the chunk's rows span
  const int32_t col = p.ajc[i];
  int64_t k = 0, kh = p.bnzc;
  while (k < kh) {
    const int64_t mid = k + (kh - k) / 2;
    if (p.bjc[mid] < col) k = mid + 1;
    else kh = mid;
  }
  int64_t blo = 0, bhi = 0;
  if (k < p.bnzc && p.bjc[k] == col) {
    const int64_t c1 = p.bcp[k + 1];
    blo = lower_row(p.bir, p.bcp[k], c1, (int64_t)p.air[a0]);
    bhi = lower_row(p.bir, blo, c1, (int64_t)p.air[a1 - 1] + 1);
  }
  const int64_t blen = bhi - blo;
  const int cls = blen == 0 ? 0 : blen <= EWISE_LDS_RANGE ? 1 : 2;
  if (cls == 1) {
    for (int q = lane; q < (int)blen; q += WAVE) rows[w][q] = p.bir[blo + q];
    wave_sync();
  }
  const bool exclude = p.op == CBG_EWISE_EXCLUDE;
  int64_t total = 0;
  int word = 0;
  for (int64_t x0 = a0; x0 < a1; x0 += WAVE, ++word) {  // the trip count is the wave's: every lane votes
    const int64_t x = x0 + lane;
    bool keep = false;
    if (x < a1) {
      bool hit = false;
      if (cls == 1) {
        const int32_t r = p.air[x];
        int l = 0, h = (int)blen;
        while (l < h) {
          const int mid = (l + h) >> 1;
          if (rows[w][mid] < r) l = mid + 1;
          else h = mid;
        }
        hit = l < (int)blen && rows[w][l] == r;
      } else if (cls == 2) {
        const int32_t r = p.air[x];
        const int64_t at = lower_row(p.bir, blo, bhi, (int64_t)r);
        hit = at < bhi && p.bir[at] == r;
      }
      keep = hit != exclude;
    }
    const u64 m = __ballot(keep);
    if (lane == 0) p.mask[u * WORDS + word] = m;
    total += __popcll(m);
  }
  if (lane == 0) {
    p.cnt[u] = total;
    p.ucol[u] = (int32_t)i;
    p.blo[u] = blo;
    p.bhi[u] = bhi;
    atomicAdd(reinterpret_cast<u64*>(p.stat) + 1 + cls, 1ull);
  }
}

// coloff[i] = the offset of column i's first unit, i <= nzc: the dense column offsets
__global__ void k_ewise_coloff(int64_t nzc, const int64_t* __restrict__ ustart, const int64_t* __restrict__ off,
                               int64_t* __restrict__ coloff, int64_t* __restrict__ stat) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i > nzc) return;
  const int64_t o = off[ustart[i]];
  coloff[i] = o;
  if (i == nzc) {
    stat[0] = o;
    stat[4] = ustart[nzc];
  }
}

// one wave per unit: the kept entries, in order, at the unit's offset
__global__ __launch_bounds__(256) void k_ewise_emit(Ew p, const int64_t* __restrict__ off, int32_t* __restrict__ oir,
                                                    double* __restrict__ oval) {
  const int64_t u = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (u >= p.umax || u >= p.ustart[p.anzc]) return;
  int64_t dst = off[u];
  if (off[u + 1] == dst) return;
  const int64_t i = p.ucol[u];
  const int64_t a0 = p.acp[i] + (u - p.ustart[i]) * EWISE_CHUNK, a1 = min(a0 + EWISE_CHUNK, p.acp[i + 1]);
  const int64_t blo = p.blo[u], bhi = p.bhi[u];
  const int lane = lane_id();
  int word = 0;
  for (int64_t x0 = a0; x0 < a1; x0 += WAVE, ++word) {
    const u64 m = p.mask[u * WORDS + word];
    if ((m >> lane) & 1ull) {
      const int64_t x = x0 + lane, at = dst + __popcll(m & ((1ull << lane) - 1ull));
      const int32_t r = ld_stream(p.air + x);
      double v = ld_stream(p.aval + x);
      if (p.op == CBG_EWISE_MULT) v = v * p.bval[lower_row(p.bir, blo, bhi, (int64_t)r)];  // a kept entry is a hit
      st_stream(oir + at, r);
      st_stream(oval + at, v);
    }
    dst += __popcll(m);
  }
}
}  // namespace

int ewise_bounds(int64_t* bounds, int n) {
  const int64_t b[2] = {EWISE_CHUNK, EWISE_LDS_RANGE};
  for (int i = 0; bounds && i < n && i < 2; ++i) bounds[i] = b[i];
  return 2;
}

// b == NULL: the empty tile
void tile_ewise(const cbg_tile& a, const cbg_tile* b, int op, cbg_tile& out, hipStream_t s) {
  EwiseStats& st = ewise_stats();
  st.counts[CBG_EWISE_ENTRIES_A] += a.nnz;
  st.counts[CBG_EWISE_ENTRIES_B] += b ? b->nnz : 0;
  if (a.nnz == 0 || a.nzc == 0 || ((!b || b->nnz == 0 || b->nzc == 0) && op != CBG_EWISE_EXCLUDE)) {
    tile_alloc_device(out, a.m, a.n, 0, 0);
    return;
  }
  if (!b || b->nnz == 0 || b->nzc == 0) {  // nothing to exclude (SpDCCols.cpp:631-690): a copy
    tile_slice_cols(a, 0, a.n, out, s);
    st.counts[CBG_EWISE_ENTRIES_OUT] += out.nnz;
    return;
  }
  struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } ev;
  CBG_HIP(hipEventCreate(&ev.e0));
  CBG_HIP(hipEventCreate(&ev.e1));
  const int64_t nzc = a.nzc;
  // sum of ceil(len / CHUNK) over the columns <= nnz / CHUNK + nzc
  const int64_t umax = a.nnz / EWISE_CHUNK + nzc;
  TileGuard o;
  DBuf<int64_t> cols(3 * (nzc + 1));  // nu | ustart | coloff
  DBuf<int64_t> units(4 * umax + 1);  // cnt | blo | bhi | off[0 .. umax]
  DBuf<int32_t> ucol(umax);
  DBuf<u64> mask(umax * WORDS);
  DBuf<int64_t> stat(5);
  DeferredFree df;
  WaitOnThrow wait{s};  // declared last, so it runs first: before the output and the buffers go
  int64_t *nu = cols.p, *ustart = cols.p + (nzc + 1), *coloff = cols.p + 2 * (nzc + 1);
  int64_t* off = units.p + 3 * umax;
  Ew p{};
  p.anzc = nzc, p.bnzc = b->nzc;
  p.acp = a.cp, p.ajc = a.jc, p.air = a.ir, p.aval = a.val;
  p.bcp = b->cp, p.bjc = b->jc, p.bir = b->ir, p.bval = b->val;
  p.op = op, p.umax = umax, p.ustart = ustart;
  p.cnt = units.p, p.blo = units.p + umax, p.bhi = units.p + 2 * umax;
  p.ucol = ucol.p, p.mask = mask.p, p.stat = stat.p;
  CBG_HIP(hipEventRecord(ev.e0, s));
  CBG_HIP(hipMemsetAsync(stat.p, 0, sizeof(int64_t) * 5, s));
  hipLaunchKernelGGL(k_ewise_units, dim3(nblk(nzc, 256)), dim3(256), 0, s, nzc, a.cp, nu);
  exclusive_scan_i64(nu, ustart, nzc, s, &df);
  hipLaunchKernelGGL(k_ewise_count, dim3(nblk(umax, WAVES)), dim3(256), 0, s, p);
  exclusive_scan_i64(p.cnt, off, umax, s, &df);
  hipLaunchKernelGGL(k_ewise_coloff, dim3(nblk(nzc + 1, 256)), dim3(256), 0, s, nzc, ustart, off, coloff, stat.p);
  CBG_HIP(hipGetLastError());
  int64_t tot[5] = {0, 0, 0, 0, 0};
  compact_columns(a.m, a.n, 0, nzc, a.jc, coloff, o.t, s, df, stat.p, tot, 5);  // the one readback
  o.t.nnz = tot[0];
  o.t.ir = static_cast<int32_t*>(pool().alloc(sizeof(int32_t) * std::max<int64_t>(tot[0], 1)));
  o.t.val = static_cast<double*>(pool().alloc(sizeof(double) * std::max<int64_t>(tot[0], 1)));
  if (tot[0] > 0) hipLaunchKernelGGL(k_ewise_emit, dim3(nblk(umax, WAVES)), dim3(256), 0, s, p, off, o.t.ir, o.t.val);
  CBG_HIP(hipGetLastError());
  CBG_HIP(hipEventRecord(ev.e1, s));
  CBG_HIP(hipStreamSynchronize(s));  // the temporaries go back to the pool
  df.synced = true;
  wait.done = true;
  float ms = 0;
  CBG_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  st.ms += ms;
  st.counts[CBG_EWISE_ENTRIES_OUT] += tot[0];
  st.counts[CBG_EWISE_UNITS] += tot[4];
  for (int c = 0; c < 3; ++c) st.counts[CBG_EWISE_CLASS0 + c] += tot[1 + c];
  out = o.release();
}

// ---------------------------------------------------------------------------
// SpParMat::Apply: v <- arg (the unit-valued copy a bool matrix is), v <- arg / v
// ---------------------------------------------------------------------------
namespace {
template <bool RDIV>
__global__ __launch_bounds__(256) void k_apply_value(double* __restrict__ val, int64_t nnz, double arg) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < nnz) val[i] = RDIV ? arg / val[i] : arg;
}
}  // namespace

void tile_apply_set(cbg_tile& t, double arg, hipStream_t s) {
  if (t.nnz <= 0) return;
  hipLaunchKernelGGL(k_apply_value<false>, dim3(nblk(t.nnz, 256)), dim3(256), 0, s, t.val, t.nnz, arg);
  CBG_HIP(hipGetLastError());
}
void tile_apply_rdiv(cbg_tile& t, double arg, hipStream_t s) {
  if (t.nnz <= 0) return;
  hipLaunchKernelGGL(k_apply_value<true>, dim3(nblk(t.nnz, 256)), dim3(256), 0, s, t.val, t.nnz, arg);
  CBG_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------
// BetwCent's dense block (BetwCent.cpp:186-204): bcu is column-major, lm rows per column,
// one column per local root of the batch.  A tile's positions are distinct, so the
// update needs no atomics.
// ---------------------------------------------------------------------------
namespace {
template <bool ADD>
__global__ __launch_bounds__(256) void k_dense_tile(int64_t nzc, const int64_t* __restrict__ cp,
                                                    const int32_t* __restrict__ jc, const int32_t* __restrict__ ir,
                                                    double* __restrict__ val, double* __restrict__ bcu, int64_t lm) {
  const int64_t i = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / WAVE;
  if (i >= nzc) return;
  double* col = bcu + (int64_t)jc[i] * lm;
  for (int64_t q = cp[i] + lane_id(); q < cp[i + 1]; q += WAVE) {
    if (ADD) col[ir[q]] += val[q];
    else val[q] *= col[ir[q]];
  }
}
// out[i] = bcu(i, 0) + bcu(i, 1) + ... in that order; consecutive lanes read consecutive rows
__global__ __launch_bounds__(256) void k_dense_row_sums(const double* __restrict__ bcu, int64_t lm, int64_t ln,
                                                        double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= lm) return;
  double s = 0.0;
  for (int64_t j = 0; j < ln; ++j) s += bcu[i + j * lm];
  out[i] = s;
}
}  // namespace

void dense_fill(double* d, int64_t n, double v, hipStream_t s) { fill_device(d, n, v, s); }
void dense_scale_tile(cbg_tile& t, const double* bcu, int64_t lm, hipStream_t s) {
  if (t.nzc > 0)
    hipLaunchKernelGGL(k_dense_tile<false>, dim3(nblk(t.nzc * WAVE, 256)), dim3(256), 0, s, t.nzc, t.cp, t.jc, t.ir,
                       t.val, const_cast<double*>(bcu), lm);
  CBG_HIP(hipGetLastError());
}
void dense_add_tile(const cbg_tile& t, double* bcu, int64_t lm, hipStream_t s) {
  if (t.nzc > 0)
    hipLaunchKernelGGL(k_dense_tile<true>, dim3(nblk(t.nzc * WAVE, 256)), dim3(256), 0, s, t.nzc, t.cp, t.jc, t.ir,
                       t.val, bcu, lm);
  CBG_HIP(hipGetLastError());
}
void dense_row_sums(const double* bcu, int64_t lm, int64_t ln, double* out, hipStream_t s) {
  if (lm > 0) hipLaunchKernelGGL(k_dense_row_sums, dim3(nblk(lm, 256)), dim3(256), 0, s, bcu, lm, ln, out);
  CBG_HIP(hipGetLastError());
}

}  // namespace cbg
