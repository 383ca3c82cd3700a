// cbg_prune.hip -- Markov-clustering pruning of a DCSC tile on device
// (MCLPruneRecoverySelect, ParFriends.h:186-353): column statistics under a
// per-column threshold, an exact k-th largest value per column (radix select
// on the order-preserving 64-bit key of the double) and the column-threshold
// compaction.  All per-column arrays are dense over the tile's n columns, so
// the ranks of a grid column index them alike whatever columns are empty on
// one of them.  NaN values are not ordered by the key the way operator< sees
// them: the result for a column that holds a NaN is unspecified.
#include <algorithm>
#include <cstring>
#include <tuple>

#include "cbg_rebuild.h"
#include "cbg_vector.h"

namespace cbg {

namespace {
// k-select length classes (cbg_mcl_kselect_bounds): a wave's registers (8 keys
// per lane), a block's LDS at 32 KiB and at 128 KiB of keys, longer: streamed
constexpr int KSEL_WAVE_MAX = 512;
constexpr int KSEL_LDS_SMALL = 4096;
constexpr int KSEL_LDS_MAX = 16384;
constexpr int KSEL_STREAM_BLOCKS = 16;   // at most this many blocks share one streamed column ...
constexpr int KSEL_STREAM_CHUNK = 4096;  // ... in chunks of this many entries
// column statistics: 16 lanes per column up to 16 entries, a wave up to 4096, a block above
constexpr int STAT_GROUP_MAX = 16;
constexpr int STAT_WAVE_MAX = 4096;

// order-preserving key: a < b  <=>  key(a) < key(b); -0.0 and +0.0 share a key
__device__ inline u64 key_of(double v) {
  v = v == 0.0 ? 0.0 : v;
  const u64 u = (u64)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ inline int64_t imin(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ inline double val_of(u64 k) {
  const u64 u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)u);
}

// ---------------------------------------------------------------------------
// k_col_stats: count and sum of the kept values of every nonempty column, one
// streaming pass over val.  strict keeps v > thr, else !(v < thr).  The order
// of a column's sum depends on its length alone: columns of <= 16 entries one
// entry per lane of a 16-lane group (four columns to a wave), up to 4096
// entries lane-strided partials of a wave, longer ones thread-strided partials
// of a 256-thread block; then a fixed xor tree (1, 2, 4, ...), and for the
// block the four wave sums added in wave order.  No atomics: bit-reproducible.
// dense: results at the column's id (else at its position in jc).
// ---------------------------------------------------------------------------
template <int G, bool SUM>
__global__ __launch_bounds__(256) void k_col_stats(const int64_t* __restrict__ cp, const int32_t* __restrict__ jc,
                                                   const double* __restrict__ val, int64_t nzc,
                                                   const double* __restrict__ thr, int strict, int64_t lo,
                                                   int64_t hi, int dense, int64_t* __restrict__ cnt,
                                                   double* __restrict__ sum) {
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int l = threadIdx.x % G;
  if (p >= nzc) return;
  const int64_t b = cp[p], len = cp[p + 1] - b;
  if (len <= lo || len > hi) return;
  const int32_t j = jc[p];
  const double t = thr[j];
  int64_t c = 0;
  double s = 0.0;
  for (int64_t i = l; i < len; i += G) {
    const double v = val[b + i];
    const bool keep = strict ? v > t : !(v < t);
    if (keep) {
      ++c;
      if (SUM) s += v;
    }
  }
#pragma unroll
  for (int d = 1; d < G; d <<= 1) {
    c += __shfl_xor(c, d, WAVE);
    if (SUM) s += __shfl_xor(s, d, WAVE);
  }
  if (l == 0) {
    const int64_t o = dense ? j : p;
    cnt[o] = c;
    if (SUM) sum[o] = s;
  }
}

template <bool SUM>
__global__ __launch_bounds__(256) void k_col_stats_block(const int64_t* __restrict__ cp,
                                                         const int32_t* __restrict__ jc,
                                                         const double* __restrict__ val, int64_t nzc,
                                                         const double* __restrict__ thr, int strict, int64_t lo,
                                                         int dense, int64_t* __restrict__ cnt,
                                                         double* __restrict__ sum) {
  __shared__ int64_t sc[4];
  __shared__ double ss[4];
  const int64_t p = blockIdx.x;
  const int64_t b = cp[p], len = cp[p + 1] - b;
  if (len <= lo) return;
  const int32_t j = jc[p];
  const double t = thr[j];
  int64_t c = 0;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < len; i += 256) {
    const double v = val[b + i];
    const bool keep = strict ? v > t : !(v < t);
    if (keep) {
      ++c;
      if (SUM) s += v;
    }
  }
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    c += __shfl_xor(c, d, WAVE);
    if (SUM) s += __shfl_xor(s, d, WAVE);
  }
  if ((threadIdx.x & 63) == 0) {
    sc[threadIdx.x >> 6] = c;
    ss[threadIdx.x >> 6] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int64_t o = dense ? j : p;
    cnt[o] = ((sc[0] + sc[1]) + sc[2]) + sc[3];
    if (SUM) sum[o] = ((ss[0] + ss[1]) + ss[2]) + ss[3];
  }
}

// column statistics of the P ranks of a grid column summed in rank order:
// buf = P records of [cnt(n) | sum(n) | all(n)]
__global__ void k_stats_combine(const int64_t* buf, int P, int64_t n, int64_t* cnt, double* sum, int64_t* all) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int64_t c = 0, a = 0;
  double s = 0.0;
  for (int r = 0; r < P; ++r) {
    const int64_t* rec = buf + (size_t)r * 3 * n;
    c += rec[j];
    const double x = reinterpret_cast<const double*>(rec + n)[j];
    s = r == 0 ? x : s + x;
    a += rec[2 * n + j];
  }
  cnt[j] = c;
  sum[j] = s;
  all[j] = a;
}

// ---------------------------------------------------------------------------
// column sets (recover / select / recover after selection) as 0/1 flags
// ---------------------------------------------------------------------------
__global__ void k_flag_recover(const int64_t* cnt0, const double* sum0, const int64_t* all, int64_t n, int64_t R,
                               double q, int32_t* f) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) f[j] = (cnt0[j] < R && all[j] > cnt0[j] && sum0[j] < q) ? 1 : 0;
}
__global__ void k_flag_select(const int64_t* cnt0, const int32_t* inR, int64_t n, int64_t S, int32_t* f) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) f[j] = ((!inR || !inR[j]) && cnt0[j] > S) ? 1 : 0;
}
__global__ void k_flag_recover2(const int64_t* cnt1, const double* sum1, const int32_t* inS, int64_t n, int64_t R,
                                double q, int32_t* f) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) f[j] = (inS[j] && cnt1[j] < R && sum1[j] < q) ? 1 : 0;
}
__global__ void k_compact_list(const int32_t* f, const int64_t* off, int64_t n, int32_t* list) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n && f[j]) list[off[j]] = (int32_t)j;
}
__global__ void k_scatter_thr(const int32_t* list, const double* kth, int64_t L, double* thr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < L) thr[list[i]] = kth[i];
}
// the listed columns as segments [beg, end) of val; sz = min(k, length) (may be NULL)
__global__ void k_segments(const int64_t* cp, const int32_t* pos, const int32_t* list, int64_t L, int64_t k,
                           int64_t* beg, int64_t* end, int64_t* sz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  const int32_t p = pos[list[i]];
  const int64_t b = p < 0 ? 0 : cp[p], e = p < 0 ? 0 : cp[p + 1];
  beg[i] = b;
  end[i] = e;
  if (sz) sz[i] = imin(k, e - b);
}

// ---------------------------------------------------------------------------
// k-select.  Segment i of val is [beg[i], end[i]); out[i] = its min(k, len)-th
// largest value (0.0 for an empty segment).  st: device counters, st[c] =
// segments of class c (0 wave, 1 / 2 LDS, 3 streamed).
// ---------------------------------------------------------------------------
// class 0: one wave per segment, 8 keys per lane in registers, the key built
// bit by bit from the top: the largest candidate that >= k keys reach.  The
// kernel visits every segment and appends the longer ones to their class's
// list (lists[(c - 1) * L + ...], st[c] the cursor), so that the other classes
// run on exactly their segments.
__global__ __launch_bounds__(256) void k_kselect_wave(const double* __restrict__ val, const int64_t* __restrict__ beg,
                                                      const int64_t* __restrict__ end, int64_t L, int64_t k,
                                                      double* __restrict__ out, u64* st, int32_t* lists,
                                                      u64* lprefix, int64_t* lkk, int64_t cap) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= L) return;
  const int64_t b = beg[i], len = end[i] - b;
  if (len > KSEL_WAVE_MAX) {
    if (lane == 0) {
      const int c = len > KSEL_LDS_MAX ? 3 : len > KSEL_LDS_SMALL ? 2 : 1;
      const u64 slot = atomicAdd(&st[c], 1ull);
      lists[(int64_t)(c - 1) * L + (int64_t)slot] = (int32_t)i;  // slot < L: every segment is appended once
      if (c == 3 && slot < (u64)cap) {  // cap: an upper bound for disjoint segments
        lprefix[slot] = 0;
        lkk[slot] = imin(k, len);
      }
    }
    return;
  }
  if (len <= 0) {
    if (lane == 0) out[i] = 0.0;
    return;
  }
  u64 key[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const int idx = lane + WAVE * r;
    key[r] = idx < len ? key_of(val[b + idx]) : 0ull;  // 0 never reaches a candidate (>= 1)
  }
  const int kk = (int)imin(k, len);
  u64 cand = 0;
  for (int bit = 63; bit >= 0; --bit) {
    const u64 trial = cand | (1ull << bit);
    int c = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r) c += __popcll(__ballot(key[r] >= trial));
    if (c >= kk) cand = trial;
  }
  if (lane == 0) {
    out[i] = val_of(cand);
    atomicAdd(&st[0], 1ull);
  }
}

// One wave picks the digit of a 256-bin histogram where the count from the top
// reaches kk: lane l sums bins 255-4l ... 252-4l, a prefix scan over the lanes
// finds the lane, which walks its four bins.  above = entries in higher bins.
__device__ inline void wave_pick(const unsigned int* h, long long kk, int lane, int& digit, long long& above) {
  const unsigned int c0 = h[255 - 4 * lane], c1 = h[254 - 4 * lane], c2 = h[253 - 4 * lane], c3 = h[252 - 4 * lane];
  const long long s = (long long)c0 + c1 + c2 + c3;
  long long incl = s;
  for (int d = 1; d < WAVE; d <<= 1) {
    const long long t = __shfl_up(incl, d, WAVE);
    if (lane >= d) incl += t;
  }
  const long long excl = incl - s;
  const bool mine = excl < kk && kk <= incl;
  int dg = 0;
  long long ab = 0;
  if (mine) {
    long long a = excl;
    dg = 255 - 4 * lane;
    if (a + c0 < kk) {
      a += c0;
      --dg;
      if (a + c1 < kk) {
        a += c1;
        --dg;
        if (a + c2 < kk) {
          a += c2;
          --dg;
        }
      }
    }
    ab = a;
  }
  const u64 m = __ballot(mine);
  const int src = m ? __ffsll((long long)m) - 1 : 0;
  digit = __shfl(dg, src, WAVE);
  above = __shfl(ab, src, WAVE);
}

// classes 1 and 2: one block per segment, its keys in LDS, 8 digit passes
template <int CAP>
__global__ __launch_bounds__(512) void k_kselect_lds(const double* __restrict__ val, const int64_t* __restrict__ beg,
                                                     const int64_t* __restrict__ end,
                                                     const int32_t* __restrict__ list, int64_t k,
                                                     double* __restrict__ out) {
  extern __shared__ u64 keys[];
  __shared__ unsigned int hist[256];
  __shared__ u64 s_prefix;
  __shared__ long long s_kk;
  const int64_t i = list[blockIdx.x];
  const int64_t b = beg[i];
  const int len = (int)imin(end[i] - b, (int64_t)CAP);
  for (int x = threadIdx.x; x < len; x += 512) keys[x] = key_of(val[b + x]);
  if (threadIdx.x == 0) {
    s_prefix = 0;
    s_kk = imin(k, (int64_t)len);
  }
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    if (threadIdx.x < 256) hist[threadIdx.x] = 0;
    __syncthreads();
    const u64 prefix = s_prefix;
    const long long kk = s_kk;
    for (int x = threadIdx.x; x < len; x += 512) {
      const u64 key = keys[x];
      if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (threadIdx.x < WAVE) {
      int digit;
      long long above;
      wave_pick(hist, kk, threadIdx.x, digit, above);
      if (threadIdx.x == 0) {
        s_prefix = prefix | ((u64)digit << shift);
        s_kk = kk - above;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[i] = val_of(s_prefix);
}

// class 3: streamed from HBM, one digit per pass.  Up to KSEL_STREAM_BLOCKS
// blocks share a segment in chunks of KSEL_STREAM_CHUNK entries (a block
// without a chunk leaves at once); integer atomics only: the histogram is exact.
__global__ __launch_bounds__(256) void k_kselect_stream_hist(const double* __restrict__ val,
                                                             const int64_t* __restrict__ beg,
                                                             const int64_t* __restrict__ end,
                                                             const int32_t* __restrict__ longlist,
                                                             const u64* __restrict__ lprefix, int pass,
                                                             unsigned int* hist) {
  __shared__ unsigned int h[256];
  const int64_t slot = blockIdx.x;
  const int32_t i = longlist[slot];
  const int64_t b = beg[i], len = end[i] - b;
  if ((int64_t)blockIdx.y * KSEL_STREAM_CHUNK >= len) return;
  h[threadIdx.x] = 0;
  __syncthreads();
  const u64 prefix = lprefix[slot];
  const int shift = 56 - 8 * pass;
  for (int64_t c0 = (int64_t)blockIdx.y * KSEL_STREAM_CHUNK; c0 < len; c0 += (int64_t)gridDim.y * KSEL_STREAM_CHUNK) {
    const int64_t c1 = imin(c0 + KSEL_STREAM_CHUNK, len);
    for (int64_t x = c0 + threadIdx.x; x < c1; x += 256) {
      const u64 key = key_of(val[b + x]);
      if (pass == 0 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&h[(key >> shift) & 255], 1u);
    }
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[slot * 256 + threadIdx.x], h[threadIdx.x]);
}
__global__ __launch_bounds__(64) void k_kselect_stream_pick(const int32_t* __restrict__ longlist, u64* lprefix,
                                                            int64_t* lkk, int pass, unsigned int* hist,
                                                            double* __restrict__ out) {
  const int64_t slot = blockIdx.x;
  unsigned int* h = hist + slot * 256;
  int digit;
  long long above;
  wave_pick(h, lkk[slot], threadIdx.x, digit, above);
  for (int x = threadIdx.x; x < 256; x += WAVE) h[x] = 0;  // every lane has read its bins in wave_pick
  if (threadIdx.x == 0) {
    const u64 prefix = lprefix[slot] | ((u64)digit << (56 - 8 * pass));
    lprefix[slot] = prefix;
    lkk[slot] -= above;
    if (pass == 7) out[longlist[slot]] = val_of(prefix);
  }
}

// ---------------------------------------------------------------------------
// grid columns of several ranks: a rank's top-min(k, len) multiset of a
// segment (the values above its local k-th and copies of it up to sz), and the
// union of the ranks' multisets laid out segment by segment
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_extract_top(const double* __restrict__ val, const int64_t* __restrict__ beg,
                                                     const int64_t* __restrict__ end, const double* __restrict__ lk,
                                                     const int64_t* __restrict__ ooff, double* __restrict__ obuf) {
  __shared__ unsigned long long n_above;
  const int64_t i = blockIdx.x;
  const int64_t b = beg[i], len = end[i] - b;
  const int64_t o = ooff[i], sz = ooff[i + 1] - o;
  if (sz <= 0) return;
  if (threadIdx.x == 0) n_above = 0;
  __syncthreads();
  const double t = lk[i];
  const u64 tk = key_of(t);
  for (int64_t x = threadIdx.x; x < len; x += 256) {
    const double v = val[b + x];
    if (key_of(v) > tk) obuf[o + (int64_t)atomicAdd(&n_above, 1ull)] = v;
  }
  __syncthreads();
  for (int64_t x = (int64_t)n_above + threadIdx.x; x < sz; x += 256) obuf[o + x] = t;
}
// tot[i] = sum over the ranks of SZ[r][i]
__global__ void k_union_sizes(const int64_t* SZ, int P, int64_t L, int64_t* tot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  int64_t s = 0;
  for (int r = 0; r < P; ++r) s += SZ[(size_t)r * L + i];
  tot[i] = s;
}
// roff: P exclusive scans of SZ's rows ((L + 1) entries each); ALL: P buffers of `stride` values
__global__ __launch_bounds__(256) void k_union_gather(const int64_t* SZ, const int64_t* roff, const double* ALL, int P,
                                                      int64_t L, int64_t stride, const int64_t* ubeg, double* u,
                                                      int64_t* uend) {
  const int64_t i = blockIdx.x;
  int64_t o = ubeg[i];
  for (int r = 0; r < P; ++r) {
    const int64_t n = SZ[(size_t)r * L + i];
    const double* src = ALL + (size_t)r * stride + roff[(size_t)r * (L + 1) + i];
    for (int64_t x = threadIdx.x; x < n; x += 256) u[o + x] = src[x];
    o += n;
  }
  if (threadIdx.x == 0) uend[i] = o;
}

// ---------------------------------------------------------------------------
// compaction: the count is k_col_stats without the sums (kept entries per stored
// column, non-strict); the emit copies a surviving column's kept entries in
// order, values untouched
// ---------------------------------------------------------------------------
struct EmitKept {
  const int64_t* cp;
  const int32_t *jc, *ir;
  const double *val, *thr;
  struct Keep {
    static constexpr bool by_row = false;
    double t;
    __device__ __forceinline__ bool operator()(int32_t, double v) const { return !(v < t); }
  };
  __device__ __forceinline__ void operator()(int64_t p, int64_t dst, int32_t* oir, double* oval) const {
    copy_filtered(ir, val, cp[p], cp[p + 1] - cp[p], Keep{thr[jc[p]]}, RowSame(), oir, oval, dst);
  }
};

// device time of the prune's stages (events read after the call's last sync)
struct StageClock {
  hipStream_t s;
  std::vector<std::tuple<int, hipEvent_t, hipEvent_t>> ev;
  explicit StageClock(hipStream_t st) : s(st) {}
  void begin(int stage) {
    hipEvent_t a = nullptr, b = nullptr;
    CBG_HIP(hipEventCreate(&a));
    ev.emplace_back(stage, a, b);
    CBG_HIP(hipEventCreate(&std::get<2>(ev.back())));
    CBG_HIP(hipEventRecord(a, s));
  }
  void end() { CBG_HIP(hipEventRecord(std::get<2>(ev.back()), s)); }
  void collect(double* ms) {
    for (auto& e : ev) {
      float t = 0.f;
      if (hipEventSynchronize(std::get<2>(e)) == hipSuccess &&
          hipEventElapsedTime(&t, std::get<1>(e), std::get<2>(e)) == hipSuccess)
        ms[std::get<0>(e)] += t;
      else
        (void)hipGetLastError();
    }
  }
  ~StageClock() {
    for (auto& e : ev) {
      if (std::get<1>(e)) (void)hipEventDestroy(std::get<1>(e));
      if (std::get<2>(e)) (void)hipEventDestroy(std::get<2>(e));
    }
  }
};

// st: 5 zeroed device counters (see above), read into sth after the wave kernel (one
// stream synchronization: the other classes are launched on their exact counts);
// total = entries of val
void seg_kselect(const double* val, int64_t total, const int64_t* beg, const int64_t* end, int64_t L, int64_t k,
                 double* out, u64* st, u64* sth, hipStream_t s, DeferredFree& df) {
  if (L <= 0) return;
  const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(L, total / (KSEL_LDS_MAX + 1)));
  DBuf<int32_t> lists((size_t)3 * L);
  DBuf<u64> lprefix(cap);
  DBuf<int64_t> lkk(cap);
  hipLaunchKernelGGL(k_kselect_wave, dim3(nblk(L, 4)), dim3(256), 0, s, val, beg, end, L, k, out, st, lists.p,
                     lprefix.p, lkk.p, cap);
  CBG_HIP(hipGetLastError());
  CBG_HIP(hipMemcpyAsync(sth, st, sizeof(u64) * 5, hipMemcpyDeviceToHost, s));
  CBG_HIP(hipStreamSynchronize(s));
  const int64_t n1 = (int64_t)sth[1], n2 = (int64_t)sth[2], n3 = std::min<int64_t>((int64_t)sth[3], cap);
  if (n1 > 0)
    hipLaunchKernelGGL(k_kselect_lds<KSEL_LDS_SMALL>, dim3((unsigned)n1), dim3(512), sizeof(u64) * KSEL_LDS_SMALL, s, val,
                       beg, end, lists.p, k, out);
  if (n2 > 0) {
    set_lds(k_kselect_lds<KSEL_LDS_MAX>, sizeof(u64) * KSEL_LDS_MAX);
    hipLaunchKernelGGL(k_kselect_lds<KSEL_LDS_MAX>, dim3((unsigned)n2), dim3(512), sizeof(u64) * KSEL_LDS_MAX, s, val, beg,
                       end, lists.p + L, k, out);
  }
  if (n3 > 0) {
    DBuf<unsigned int> hist((size_t)n3 * 256);
    CBG_HIP(hipMemsetAsync(hist.p, 0, sizeof(unsigned int) * n3 * 256, s));
    for (int pass = 0; pass < 8; ++pass) {
      hipLaunchKernelGGL(k_kselect_stream_hist, dim3((unsigned)n3, KSEL_STREAM_BLOCKS), dim3(256), 0, s, val, beg, end,
                         lists.p + 2 * L, lprefix.p, pass, hist.p);
      hipLaunchKernelGGL(k_kselect_stream_pick, dim3((unsigned)n3), dim3(64), 0, s, lists.p + 2 * L, lprefix.p, lkk.p,
                         pass, hist.p, out);
    }
    df.take(hist);
  }
  CBG_HIP(hipGetLastError());
  df.take(lists);
  df.take(lprefix);
  df.take(lkk);
}

template <bool SUM>
void col_stats_launch(const cbg_tile& t, const double* thr, int strict, int dense, int64_t* cnt, double* sum,
                      hipStream_t s) {
  if (t.nzc <= 0) return;
  hipLaunchKernelGGL((k_col_stats<STAT_GROUP_MAX, SUM>), dim3(nblk(t.nzc * STAT_GROUP_MAX, 256)), dim3(256), 0, s, t.cp,
                     t.jc, t.val, t.nzc, thr, strict, (int64_t)0, (int64_t)STAT_GROUP_MAX, dense, cnt, sum);
  if (t.nnz > STAT_GROUP_MAX)
    hipLaunchKernelGGL((k_col_stats<WAVE, SUM>), dim3(nblk(t.nzc * WAVE, 256)), dim3(256), 0, s, t.cp, t.jc, t.val,
                       t.nzc, thr, strict, (int64_t)STAT_GROUP_MAX, (int64_t)STAT_WAVE_MAX, dense, cnt, sum);
  if (t.nnz > STAT_WAVE_MAX)
    hipLaunchKernelGGL(k_col_stats_block<SUM>, dim3((unsigned)t.nzc), dim3(256), 0, s, t.cp, t.jc, t.val, t.nzc, thr,
                       strict, (int64_t)STAT_WAVE_MAX, dense, cnt, sum);
  CBG_HIP(hipGetLastError());
}

void add_class_counts(const u64* st_host) {
  MclStats& m = mcl_stats();
  for (int c = 0; c < 4; ++c) m.counts[CBG_MCL_KSELECT_CLASS0 + c] += (int64_t)st_host[c];
}
}  // namespace

MclStats& mcl_stats() {
  static thread_local MclStats m;
  return m;
}

int mcl_kselect_bounds(int64_t* bounds, int n) {
  const int64_t b[3] = {KSEL_WAVE_MAX, KSEL_LDS_SMALL, KSEL_LDS_MAX};
  for (int i = 0; bounds && i < n && i < 3; ++i) bounds[i] = b[i];
  return 3;
}

// dense count / sum of the kept values per column (zero for empty columns); thr: device, n entries
void tile_col_stats_device(const cbg_tile& t, const double* thr, int strict, int64_t* cnt, double* sum,
                           hipStream_t s) {
  if (t.n <= 0) return;
  CBG_HIP(hipMemsetAsync(cnt, 0, sizeof(int64_t) * t.n, s));
  CBG_HIP(hipMemsetAsync(sum, 0, sizeof(double) * t.n, s));
  col_stats_launch<true>(t, thr, strict, 1, cnt, sum, s);
}

// SpParMat::PruneColumn with less<>: keep v iff !(v < thr[column]); thr: device, n entries
void tile_prune_column_device(const cbg_tile& t, const double* thr, cbg_tile& out, hipStream_t s) {
  if (t.nzc <= 0 || t.nnz <= 0) {
    tile_alloc_device(out, t.m, t.n, 0, 0);
    return;
  }
  DBuf<int64_t> kept(t.nzc + 1);
  col_stats_launch<false>(t, thr, 0, 0, kept.p, nullptr, s);
  tile_from_columns(t.m, t.n, t.nzc, t.jc, kept.p, EmitKept{t.cp, t.jc, t.ir, t.val, thr}, out, s);
}

namespace {
// k-th largest of the listed columns over the ranks of a grid column; out: L device values.
// With several ranks the sequence of collectives does not depend on the data (an
// empty list or empty multisets exchange one dummy element): grid columns whose
// lists differ stay in step on a transport that serializes the world's collectives.
int col_kselect(const ColComm& cc, const cbg_tile& T, const int32_t* pos, const int32_t* list, int64_t L, int64_t k,
                double* out, hipStream_t s) {
  DeferredFree df;
  DBuf<int64_t> beg, end, sz, ooff;
  DBuf<u64> st;
  DBuf<double> lk, obuf;
  u64 sth[5] = {};
  int64_t total = 0;
  const int64_t L1 = std::max<int64_t>(L, 1);
  int rc = step([&] {
    beg.reset(L1);
    end.reset(L1);
    st.reset(5);
    CBG_HIP(hipMemsetAsync(st.p, 0, sizeof(u64) * 5, s));
    if (cc.P > 1) {
      sz.reset(L1 + 1);
      ooff.reset(L1 + 1);
      lk.reset(L1);
      CBG_HIP(hipMemsetAsync(sz.p, 0, sizeof(int64_t) * (L1 + 1), s));
      CBG_HIP(hipMemsetAsync(ooff.p, 0, sizeof(int64_t) * (L1 + 1), s));
    }
    if (L > 0) {
      hipLaunchKernelGGL(k_segments, dim3(nblk(L, 256)), dim3(256), 0, s, T.cp, pos, list, L, k, beg.p, end.p, sz.p);
      seg_kselect(T.val, T.nnz, beg.p, end.p, L, k, cc.P > 1 ? lk.p : out, st.p, sth, s, df);
      if (cc.P > 1) {
        exclusive_scan_i64(sz.p, ooff.p, L, s, &df);
        CBG_HIP(hipMemcpyAsync(&total, ooff.p + L, sizeof(int64_t), hipMemcpyDeviceToHost, s));
      }
    }
    CBG_HIP(hipStreamSynchronize(s));
    df.synced = true;
    if (cc.P == 1) add_class_counts(sth);
  });
  if (cc.P == 1) return rc;
  // counts first: the largest multiset total sizes every rank's send buffer
  std::vector<int64_t> tots(cc.P);
  if ((rc = cc.agree_vals(rc, &total, 1, tots.data()))) return rc;
  const int64_t stride = std::max<int64_t>(1, *std::max_element(tots.begin(), tots.end()));
  DBuf<int64_t> SZ, roff, tot, ubeg, uend;
  DBuf<double> ALL, u;
  int64_t utotal = 0;
  for (auto t : tots) utotal += t;
  rc = step([&] {
    obuf.reset(stride);
    SZ.reset((size_t)cc.P * L1);
    roff.reset((size_t)cc.P * (L1 + 1));
    tot.reset(L1 + 1);
    ubeg.reset(L1 + 1);
    uend.reset(L1);
    ALL.reset((size_t)cc.P * stride);
    u.reset(std::max<int64_t>(utotal, 1));
    CBG_HIP(hipMemsetAsync(obuf.p, 0, sizeof(double) * stride, s));
    if (L > 0)
      hipLaunchKernelGGL(k_extract_top, dim3((unsigned)L), dim3(256), 0, s, T.val, beg.p, end.p, lk.p, ooff.p, obuf.p);
    CBG_HIP(hipGetLastError());
    CBG_HIP(hipStreamSynchronize(s));
  });
  if ((rc = cc.agree_vals(rc, nullptr, 0, nullptr))) return rc;
  return step([&] {
    DeferredFree df2;
    cc.allgather_dev(sz.p, SZ.p, sizeof(int64_t) * L1);
    cc.allgather_dev(obuf.p, ALL.p, sizeof(double) * stride);
    if (L <= 0) return;
    hipLaunchKernelGGL(k_union_sizes, dim3(nblk(L, 256)), dim3(256), 0, s, SZ.p, cc.P, L, tot.p);
    exclusive_scan_i64(tot.p, ubeg.p, L, s, &df2);
    for (int r = 0; r < cc.P; ++r)
      exclusive_scan_i64(SZ.p + (size_t)r * L, roff.p + (size_t)r * (L + 1), L, s, &df2);
    hipLaunchKernelGGL(k_union_gather, dim3((unsigned)L), dim3(256), 0, s, SZ.p, roff.p, ALL.p, cc.P, L, stride, ubeg.p,
                       u.p, uend.p);
    CBG_HIP(hipMemsetAsync(st.p, 0, sizeof(u64) * 5, s));
    seg_kselect(u.p, utotal, ubeg.p, uend.p, L, k, out, st.p, sth, s, df2);
    CBG_HIP(hipStreamSynchronize(s));
    df2.synced = true;
    add_class_counts(sth);
  });
}

// 0/1 flags -> ascending list of the flagged columns; returns their number (one readback)
int64_t build_list(const int32_t* f, int64_t n, int64_t* off, int32_t* list, hipStream_t s) {
  DeferredFree df;
  exclusive_scan_i32_to_i64(f, off, n, s, &df);
  hipLaunchKernelGGL(k_compact_list, dim3(nblk(n, 256)), dim3(256), 0, s, f, off, n, list);
  int64_t L = 0;
  CBG_HIP(hipMemcpyAsync(&L, off + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  CBG_HIP(hipStreamSynchronize(s));
  df.synced = true;
  return L;
}
}  // namespace

int grid_kselect_cols(const ColComm& cc, const cbg_tile& T, const int32_t* cols_host, int64_t ncols, int64_t k,
                      double* kth_host, hipStream_t s) {
  DBuf<int32_t> pos, list;
  DBuf<double> out;
  int bad = 0;  // ids inside the tile, each listed once
  std::vector<char> seen((size_t)std::max<int64_t>(T.n, 1), 0);
  for (int64_t i = 0; i < ncols && !bad; ++i) {
    bad = cols_host[i] < 0 || cols_host[i] >= T.n || seen[cols_host[i]];
    if (!bad) seen[cols_host[i]] = 1;
  }
  int rc = bad ? (int)CBG_ERR_INVALIDPARAMS : step([&] {
    pos.reset(std::max<int64_t>(T.n, 1));
    list.reset(std::max<int64_t>(ncols, 1));
    out.reset(std::max<int64_t>(ncols, 1));
    tile_col_map(T, pos.p, nullptr, s);
    if (ncols) CBG_HIP(hipMemcpyAsync(list.p, cols_host, sizeof(int32_t) * ncols, hipMemcpyHostToDevice, s));
    CBG_HIP(hipStreamSynchronize(s));
  });
  // every rank of the grid column lists the same columns
  std::vector<int64_t> ns(cc.P);
  int64_t mine = ncols;
  if ((rc = cc.agree_vals(rc, &mine, 1, ns.data()))) return rc;
  for (auto x : ns)
    if (x != ncols) rc = CBG_ERR_INVALIDPARAMS;
  if ((rc = cc.agree_vals(rc, nullptr, 0, nullptr))) return rc;
  if (ncols == 0 && cc.P == 1) return CBG_OK;
  rc = col_kselect(cc, T, pos.p, list.p, ncols, k, out.p, s);
  if (!rc && ncols)
    rc = step([&] { CBG_HIP(hipMemcpy(kth_host, out.p, sizeof(double) * ncols, hipMemcpyDeviceToHost)); });
  return cc.agree_vals(rc, nullptr, 0, nullptr);
}

// MCLPruneRecoverySelect of one column piece, collective along the grid
// column.  Every decision point is an agree_vals along the column: a rank that
// failed says so there, and the list sizes that decide the next stage are the
// same on every rank (they come from the summed statistics).  On one rank a
// stage whose column set is empty is skipped; with several ranks it runs on the
// empty list, so that the collectives of a piece depend on the parameters only.
int mcl_prune_piece(const ColComm& cc, const cbg_tile& T, const cbg_mcl_params& P, cbg_tile& out, hipStream_t s,
                    int pend0) {
  const int64_t n = std::max<int64_t>(T.n, 1);
  const int64_t R = P.recover_num, S = P.select_num;
  const double h = P.hard_threshold, q = P.recover_pct;
  MclStats& ms = mcl_stats();
  ms.counts[CBG_MCL_PIECES] += 1;
  ms.counts[CBG_MCL_ENTRIES_IN] += T.nnz;
  StageClock clock(s);
  DBuf<double> thr, sum0, sum1, kth;
  DBuf<int64_t> cnt0, cnt1, all, off, pack, packs;
  DBuf<int32_t> pos, inR, inS, f2, list;
  auto agree = [&](int rc, int64_t* v) {
    std::vector<int64_t> a(cc.P);
    if ((rc = cc.agree_vals(rc, v, v ? 1 : 0, v ? a.data() : nullptr))) return rc;
    if (v) *v = *std::max_element(a.begin(), a.end());
    return 0;
  };
  // statistics of the whole grid column (summed in rank order); pend: this rank's failure so far
  auto stats = [&](int pend, int strict, int64_t* cnt, double* sum) {
    if (!pend) pend = step([&] {
      clock.begin(CBG_MCL_MS_STATS);
      tile_col_stats_device(T, thr.p, strict, cnt, sum, s);
      if (cc.P > 1) {
        CBG_HIP(hipMemcpyAsync(pack.p, cnt, 8 * n, hipMemcpyDeviceToDevice, s));
        CBG_HIP(hipMemcpyAsync(pack.p + n, sum, 8 * n, hipMemcpyDeviceToDevice, s));
        CBG_HIP(hipMemcpyAsync(pack.p + 2 * n, all.p, 8 * n, hipMemcpyDeviceToDevice, s));
        CBG_HIP(hipStreamSynchronize(s));
      }
      clock.end();
    });
    if (cc.P == 1) return pend;
    if (int rc = agree(pend, nullptr)) return rc;
    return step([&] {
      cc.allgather_dev(pack.p, packs.p, (size_t)24 * n);
      hipLaunchKernelGGL(k_stats_combine, dim3(nblk(n, 256)), dim3(256), 0, s, packs.p, cc.P, n, cnt, sum,
                         strict ? all.p : off.p);  // `all` is combined once (off: scratch)
      CBG_HIP(hipGetLastError());
    });
  };
  auto select_into_thr = [&](int64_t L, int64_t k) {
    clock.begin(CBG_MCL_MS_KSELECT);
    int rc = col_kselect(cc, T, pos.p, list.p, L, k, kth.p, s);
    if (!rc) rc = step([&] {
      if (L > 0) hipLaunchKernelGGL(k_scatter_thr, dim3(nblk(L, 256)), dim3(256), 0, s, list.p, kth.p, L, thr.p);
      CBG_HIP(hipGetLastError());
      clock.end();
    });
    return rc;
  };

  int pend = pend0 ? pend0 : step([&] {
    thr.reset(n), sum0.reset(n), sum1.reset(n), kth.reset(n);
    cnt0.reset(n), cnt1.reset(n), all.reset(n), off.reset(n + 1);
    pos.reset(n), inR.reset(n), inS.reset(n), f2.reset(n), list.reset(n);
    if (cc.P > 1) pack.reset(3 * n), packs.reset((size_t)3 * n * cc.P);
    fill_device(thr.p, n, h, s);
    tile_col_map(T, pos.p, all.p, s);
  });
  pend = stats(pend, 1, cnt0.p, sum0.p);
  int rc = 0;
  int64_t nR = 0, nS = 0, n2 = 0;
  if (R > 0) {  // recovery
    if (!pend) pend = step([&] {
      hipLaunchKernelGGL(k_flag_recover, dim3(nblk(n, 256)), dim3(256), 0, s, cnt0.p, sum0.p, all.p, T.n, R, q, inR.p);
      nR = build_list(inR.p, T.n, off.p, list.p, s);
    });
    if ((rc = agree(pend, &nR))) return rc;
    if (nR > 0 || cc.P > 1) pend = select_into_thr(nR, R);
  }
  if (S > 0) {  // selection, then recovery of what selection cut too far
    if (!pend) pend = step([&] {
      hipLaunchKernelGGL(k_flag_select, dim3(nblk(n, 256)), dim3(256), 0, s, cnt0.p, R > 0 ? inR.p : (int32_t*)nullptr,
                         T.n, S, inS.p);
      nS = build_list(inS.p, T.n, off.p, list.p, s);
    });
    if ((rc = agree(pend, &nS))) return rc;
    if (nS > 0 || cc.P > 1) {
      pend = select_into_thr(nS, S);
      if (R > 0) {
        pend = stats(pend, 0, cnt1.p, sum1.p);
        if (!pend) pend = step([&] {
          hipLaunchKernelGGL(k_flag_recover2, dim3(nblk(n, 256)), dim3(256), 0, s, cnt1.p, sum1.p, inS.p, T.n, R, q,
                             f2.p);
          n2 = build_list(f2.p, T.n, off.p, list.p, s);
        });
        if ((rc = agree(pend, &n2))) return rc;
        if (n2 > 0 || cc.P > 1) pend = select_into_thr(n2, R);
      }
    }
  }
  TileGuard o;
  if (!pend) pend = step([&] {
    clock.begin(CBG_MCL_MS_COMPACT);
    tile_prune_column_device(T, thr.p, o.t, s);
    clock.end();
    CBG_HIP(hipStreamSynchronize(s));
    clock.collect(ms.ms);
  });
  if ((rc = agree(pend, nullptr))) return rc;
  ms.counts[CBG_MCL_COLS_RECOVERED] += nR;
  ms.counts[CBG_MCL_COLS_SELECTED] += nS;
  ms.counts[CBG_MCL_COLS_RECOVERED_AFTER] += n2;
  ms.counts[CBG_MCL_ENTRIES_OUT] += o.t.nnz;
  out = o.release();
  return CBG_OK;
}

}  // namespace cbg
