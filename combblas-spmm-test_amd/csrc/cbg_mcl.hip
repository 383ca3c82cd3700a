// cbg_mcl.hip -- the Markov-clustering iteration around the pruned product
// (Applications/MCL.cpp: MakeColStochastic :390-395, Chaos :408-421, Inflate
// :447-450, AdjustLoops :464-474, Interpret :373-386) on a DCSC tile on device:
// column moments (sum, sum of squares, max, count in one pass), the column
// scaling, the fused inflation pass, loops on the diagonal and the label
// kernels of the connected components.  The grid-level logic (combining the
// ranks of a grid column, the world's label vector) is in cbg_grid_algos.cpp.
//
// Sum order: exactly k_col_stats' (cbg_prune.hip).  Columns of <= 16 entries one
// entry per lane of a 16-lane group, up to 4096 entries lane-strided partials
// of a wave, longer ones thread-strided partials of a 256-thread block; a fixed
// xor tree (1, 2, 4, ...), the block's four wave sums added in wave order.  No
// atomics.  The reduce pass and the fused inflation pass are one template, so a
// column's sum has the same bits in both.  Floating-point contraction is off in
// this file: v * v and s + w are rounded separately, as the host computes them.
#include <algorithm>
#include <cfloat>
#include <cmath>

#include "cbg_rebuild.h"

#pragma clang fp contract(off)

namespace cbg {

namespace {
constexpr int MOM_GROUP_MAX = 16;
constexpr int MOM_WAVE_MAX = 4096;

// what a pass over a column does with its values
enum {
  PASS_REDUCE = 0,   // moments of val
  PASS_SCALE = 1,    // val <- val * inv[column]
  PASS_INFLATE = 2   // v = val * inv[column]; sq, mx, cnt of v; val <- w = pow(v, power); sum of w
};

struct Mom {
  double sum = 0.0, sq = 0.0, mx = -__builtin_inf(), cnt = 0.0;
};

__device__ __forceinline__ double pow_arg(double v, double power, int square) {
  return square ? v * v : pow(v, power);
}

// one value of the column: the pass's element step
template <int PASS>
__device__ __forceinline__ void mom_step(double* __restrict__ val, int64_t at, double inv, double power, int square,
                                         Mom& a) {
  double v = ld_stream(val + at);
  if (PASS == PASS_SCALE) {
    st_stream(val + at, v * inv);
    return;
  }
  double w = v;
  if (PASS == PASS_INFLATE) {
    v = v * inv;
    w = pow_arg(v, power, square);
    st_stream(val + at, w);
  }
  a.sum = a.sum + w;
  a.sq = a.sq + v * v;
  a.mx = v > a.mx ? v : a.mx;
  a.cnt = a.cnt + 1.0;
}

template <int G>
__device__ __forceinline__ void mom_tree(Mom& a) {
#pragma unroll
  for (int d = 1; d < G; d <<= 1) {
    a.sum = a.sum + __shfl_xor(a.sum, d, WAVE);
    a.sq = a.sq + __shfl_xor(a.sq, d, WAVE);
    const double o = __shfl_xor(a.mx, d, WAVE);
    a.mx = o > a.mx ? o : a.mx;
    a.cnt = a.cnt + __shfl_xor(a.cnt, d, WAVE);
  }
}

// mom: four dense arrays of n doubles, [sum | sq | mx | cnt], at the column's id
__device__ __forceinline__ void mom_store(double* __restrict__ mom, int64_t n, int32_t j, const Mom& a) {
  mom[j] = a.sum;
  mom[n + j] = a.sq;
  mom[2 * n + j] = a.mx;
  mom[3 * n + j] = a.cnt;
}

// ---------------------------------------------------------------------------
// k_col_moments: one streaming pass over val, columns of length in (lo, hi],
// G lanes per column
// ---------------------------------------------------------------------------
template <int G, int PASS>
__global__ __launch_bounds__(256) void k_col_moments(const int64_t* __restrict__ cp, const int32_t* __restrict__ jc,
                                                     double* __restrict__ val, int64_t nzc, int64_t n,
                                                     const double* __restrict__ inv, double power, int square,
                                                     int64_t lo, int64_t hi, double* __restrict__ mom) {
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int l = threadIdx.x % G;
  if (p >= nzc) return;
  const int64_t b = cp[p], len = cp[p + 1] - b;
  if (len <= lo || len > hi) return;
  const int32_t j = jc[p];
  const double s = PASS == PASS_REDUCE ? 1.0 : inv[j];
  Mom a;
  for (int64_t i = l; i < len; i += G) mom_step<PASS>(val, b + i, s, power, square, a);
  if (PASS == PASS_SCALE) return;
  mom_tree<G>(a);
  if (l == 0) mom_store(mom, n, j, a);
}

template <int PASS>
__global__ __launch_bounds__(256) void k_col_moments_block(const int64_t* __restrict__ cp,
                                                           const int32_t* __restrict__ jc, double* __restrict__ val,
                                                           int64_t nzc, int64_t n, const double* __restrict__ inv,
                                                           double power, int square, int64_t lo,
                                                           double* __restrict__ mom) {
  __shared__ double sh[4][4];
  const int64_t p = blockIdx.x;
  const int64_t b = cp[p], len = cp[p + 1] - b;
  if (len <= lo) return;
  const int32_t j = jc[p];
  const double s = PASS == PASS_REDUCE ? 1.0 : inv[j];
  Mom a;
  for (int64_t i = threadIdx.x; i < len; i += 256) mom_step<PASS>(val, b + i, s, power, square, a);
  if (PASS == PASS_SCALE) return;
  mom_tree<WAVE>(a);
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    sh[0][w] = a.sum;
    sh[1][w] = a.sq;
    sh[2][w] = a.mx;
    sh[3][w] = a.cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Mom r;
    r.sum = ((sh[0][0] + sh[0][1]) + sh[0][2]) + sh[0][3];
    r.sq = ((sh[1][0] + sh[1][1]) + sh[1][2]) + sh[1][3];
    r.mx = fmax(fmax(sh[2][0], sh[2][1]), fmax(sh[2][2], sh[2][3]));
    r.cnt = ((sh[3][0] + sh[3][1]) + sh[3][2]) + sh[3][3];
    mom_store(mom, n, j, r);
  }
}

// the moments of a column nobody holds: sums 0, max -inf, count 0
__global__ void k_mom_preset(double* mom, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 4 * n) mom[i] = (i >= 2 * n && i < 3 * n) ? -__builtin_inf() : 0.0;
}

// the P ranks' moments of a grid column combined in rank order: buf = P records of 4n doubles
__global__ void k_mom_combine(const double* __restrict__ buf, int P, int64_t n, double* __restrict__ mom) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  Mom a;
  for (int r = 0; r < P; ++r) {
    const double* rec = buf + (size_t)r * 4 * n;
    a.sum = r == 0 ? rec[j] : a.sum + rec[j];
    a.sq = r == 0 ? rec[n + j] : a.sq + rec[n + j];
    a.mx = rec[2 * n + j] > a.mx ? rec[2 * n + j] : a.mx;
    a.cnt = a.cnt + rec[3 * n + j];
  }
  mom_store(mom, n, (int32_t)j, a);
}

// safemultinv (Operations.h:103-110) of the column sums
__global__ void k_safe_inv(const double* __restrict__ sum, int64_t n, double* __restrict__ inv) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) inv[j] = sum[j] == 0.0 ? DBL_MAX : 1.0 / sum[j];
}

// Reduce's result of one kind from the combined moments
__global__ void k_mom_pick(const double* __restrict__ mom, int64_t n, int what, double identity,
                           double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double r = identity;
  if (mom[3 * n + j] > 0.0) {
    const int slot = what == CBG_RED_SUM ? 0 : what == CBG_RED_SUMSQ ? 1 : what == CBG_RED_MAX ? 2 : 3;
    const double x = mom[(int64_t)slot * n + j];
    r = what == CBG_RED_MAX ? (x > identity ? x : identity) : x;
  }
  out[j] = r;
}

// Chaos (MCL.cpp:408-421): max over the columns of (max(0, values) - sumsq) * count, folded
// from 0; part[block] = the block's maximum (a maximum does not depend on the order)
__global__ __launch_bounds__(256) void k_chaos(const double* __restrict__ mom, int64_t n, double* __restrict__ part) {
  __shared__ double sh[4];
  double c = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (int64_t)gridDim.x * 256) {
    const double mx = mom[2 * n + j] > 0.0 ? mom[2 * n + j] : 0.0;
    const double x = (mx - mom[n + j]) * mom[3 * n + j];
    c = x > c ? x : c;
  }
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const double o = __shfl_xor(c, d, WAVE);
    c = o > c ? o : c;
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// SpParMat::Apply(bind2nd(exponentiate(), power)): 16 bytes per lane from the first 16-byte
// boundary (head = 1: val starts 8 bytes before one), the odd ends one value each
__global__ __launch_bounds__(256) void k_apply_pow(double* __restrict__ val, int64_t nnz, double power, int square,
                                                   int head) {
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (head && tid == 0) val[0] = pow_arg(val[0], power, square);
  const int64_t i = head + tid * 2;
  if (i + 1 < nnz) {
    double2 v = *reinterpret_cast<double2*>(val + i);
    v.x = pow_arg(v.x, power, square);
    v.y = pow_arg(v.y, power, square);
    *reinterpret_cast<double2*>(val + i) = v;
  } else if (i < nnz) {
    val[i] = pow_arg(val[i], power, square);
  }
}

template <int PASS>
void moments_launch(const cbg_tile& t, const double* inv, double power, double* mom, hipStream_t s) {
  if (t.nzc <= 0) return;
  const int square = power == 2.0 ? 1 : 0;
  hipLaunchKernelGGL((k_col_moments<MOM_GROUP_MAX, PASS>), dim3(nblk(t.nzc * MOM_GROUP_MAX, 256)), dim3(256), 0, s, t.cp,
                     t.jc, t.val, t.nzc, t.n, inv, power, square, (int64_t)0, (int64_t)MOM_GROUP_MAX, mom);
  if (t.nnz > MOM_GROUP_MAX)
    hipLaunchKernelGGL((k_col_moments<WAVE, PASS>), dim3(nblk(t.nzc * WAVE, 256)), dim3(256), 0, s, t.cp, t.jc, t.val,
                       t.nzc, t.n, inv, power, square, (int64_t)MOM_GROUP_MAX, (int64_t)MOM_WAVE_MAX, mom);
  if (t.nnz > MOM_WAVE_MAX)
    hipLaunchKernelGGL(k_col_moments_block<PASS>, dim3((unsigned)t.nzc), dim3(256), 0, s, t.cp, t.jc, t.val, t.nzc, t.n,
                       inv, power, square, (int64_t)MOM_WAVE_MAX, mom);
  CBG_HIP(hipGetLastError());
}

// One pass over the tile and the combine along the grid column: mom (4n device doubles)
// ends as the moments of the whole columns, the same bits on every rank of the column.
// pend: this rank's failure so far (reported at the agreement).
template <int PASS>
int col_pass(const ColComm& cc, const cbg_tile& T, const double* inv, double power, double* mom, hipStream_t s,
             int pend) {
  const int64_t n = std::max<int64_t>(T.n, 1);
  if (!pend) pend = step([&] {
    hipLaunchKernelGGL(k_mom_preset, dim3(nblk(4 * n, 256)), dim3(256), 0, s, mom, n);
    // the arrays are laid out for T.n columns: n == T.n but for an empty tile, whose kernels do not run
    moments_launch<PASS>(T, inv, power, mom, s);
    CBG_HIP(hipStreamSynchronize(s));
  });
  if (cc.P == 1) return pend;
  // every rank holds its receive buffer before anyone posts the gather
  DBuf<double> all;
  if (!pend) pend = step([&] { all.reset((size_t)4 * n * cc.P); });
  if (int rc = cc.agree_vals(pend, nullptr, 0, nullptr)) return rc;
  const int rc = step([&] {
    cc.allgather_dev(mom, all.p, sizeof(double) * 4 * n);
    hipLaunchKernelGGL(k_mom_combine, dim3(nblk(n, 256)), dim3(256), 0, s, all.p, cc.P, n, mom);
    CBG_HIP(hipGetLastError());
    CBG_HIP(hipStreamSynchronize(s));
  });
  // the combine's code is agreed too: a caller with a second pass makes the same collectives on every rank
  return cc.agree_vals(rc, nullptr, 0, nullptr);
}

double chaos_of(const double* mom, int64_t n, hipStream_t s) {
  const unsigned nb = std::min<unsigned>(1024, nblk(n, 256));
  DBuf<double> part(nb);
  std::vector<double> h(nb);
  hipLaunchKernelGGL(k_chaos, dim3(nb), dim3(256), 0, s, mom, n, part.p);
  CBG_HIP(hipGetLastError());
  CBG_HIP(hipMemcpyAsync(h.data(), part.p, sizeof(double) * nb, hipMemcpyDeviceToHost, s));
  CBG_HIP(hipStreamSynchronize(s));
  double c = 0.0;
  for (double x : h) c = x > c ? x : c;
  return c;
}

void scale_launch(const cbg_tile& T, const double* inv, hipStream_t s) {
  moments_launch<PASS_SCALE>(T, inv, 1.0, nullptr, s);
}
}  // namespace

HipMclStats& hipmcl_stats() {
  static thread_local HipMclStats m;
  return m;
}

int mcl_moment_bounds(int64_t* bounds, int n) {
  const int64_t b[2] = {MOM_GROUP_MAX, MOM_WAVE_MAX};
  for (int i = 0; bounds && i < n && i < 2; ++i) bounds[i] = b[i];
  return 2;
}

void tile_apply_pow(cbg_tile& t, double power, hipStream_t s) {
  if (t.nnz <= 0) return;
  const int head = (reinterpret_cast<uintptr_t>(t.val) & 15) ? 1 : 0;
  hipLaunchKernelGGL(k_apply_pow, dim3(nblk(t.nnz / 2 + 1, 256)), dim3(256), 0, s, t.val, t.nnz, power,
                     power == 2.0 ? 1 : 0, head);
  CBG_HIP(hipGetLastError());
}

int grid_reduce_cols_device(const ColComm& cc, const cbg_tile& T, int what, double identity, double* out_host,
                            hipStream_t s) {
  const int64_t n = std::max<int64_t>(T.n, 1);
  DBuf<double> mom, out;
  int pend = step([&] {
    mom.reset(4 * n);
    out.reset(n);
  });
  // a reduce pass leaves val as it is
  int rc = col_pass<PASS_REDUCE>(cc, T, nullptr, 1.0, mom.p, s, pend);
  if (!rc) rc = step([&] {
    hipLaunchKernelGGL(k_mom_pick, dim3(nblk(n, 256)), dim3(256), 0, s, mom.p, n, what, identity, out.p);
    CBG_HIP(hipGetLastError());
    if (T.n > 0) CBG_HIP(hipMemcpyAsync(out_host, out.p, sizeof(double) * T.n, hipMemcpyDeviceToHost, s));
    CBG_HIP(hipStreamSynchronize(s));
  });
  return cc.agree_vals(rc, nullptr, 0, nullptr);
}

int grid_make_col_stochastic_device(const ColComm& cc, cbg_tile& T, hipStream_t s) {
  const int64_t n = std::max<int64_t>(T.n, 1);
  DBuf<double> mom, inv;
  int pend = step([&] {
    mom.reset(4 * n);
    inv.reset(n);
  });
  int rc = col_pass<PASS_REDUCE>(cc, T, nullptr, 1.0, mom.p, s, pend);
  if (!rc) rc = step([&] {
    hipLaunchKernelGGL(k_safe_inv, dim3(nblk(n, 256)), dim3(256), 0, s, mom.p, n, inv.p);
    scale_launch(T, inv.p, s);
    CBG_HIP(hipStreamSynchronize(s));
  });
  return cc.agree_vals(rc, nullptr, 0, nullptr);
}

// the local maximum; the caller takes the maximum over the grid
int grid_chaos_device(const ColComm& cc, const cbg_tile& T, double* chaos, hipStream_t s) {
  const int64_t n = std::max<int64_t>(T.n, 1);
  DBuf<double> mom;
  int pend = step([&] { mom.reset(4 * n); });
  int rc = col_pass<PASS_REDUCE>(cc, T, nullptr, 1.0, mom.p, s, pend);
  if (!rc) rc = step([&] { *chaos = chaos_of(mom.p, n, s); });
  return cc.agree_vals(rc, nullptr, 0, nullptr);
}

// MCL.cpp:591-611 in three passes over val; ms (may be NULL): device ms of the three passes
int grid_inflate_device(const ColComm& cc, cbg_tile& T, double power, double* chaos, hipStream_t s, double* ms) {
  const int64_t n = std::max<int64_t>(T.n, 1);
  DBuf<double> mom, inv;
  hipEvent_t ev[6] = {};
  auto mark = [&](int i) {
    if (ms) CBG_HIP(hipEventRecord(ev[i], s));
  };
  int pend = step([&] {
    mom.reset(4 * n);
    inv.reset(n);
    for (int i = 0; ms && i < 6; ++i) CBG_HIP(hipEventCreate(&ev[i]));
    mark(0);
  });
  int rc = col_pass<PASS_REDUCE>(cc, T, nullptr, 1.0, mom.p, s, pend);  // 1: column sums
  if (!rc) pend = step([&] {
    mark(1);
    hipLaunchKernelGGL(k_safe_inv, dim3(nblk(n, 256)), dim3(256), 0, s, mom.p, n, inv.p);
    mark(2);
  });
  if (!rc) rc = col_pass<PASS_INFLATE>(cc, T, inv.p, power, mom.p, s, pend);  // 2: scale, chaos moments, pow, sums
  if (!rc) rc = step([&] {
    mark(3);
    *chaos = chaos_of(mom.p, n, s);
    hipLaunchKernelGGL(k_safe_inv, dim3(nblk(n, 256)), dim3(256), 0, s, mom.p, n, inv.p);
    mark(4);
    scale_launch(T, inv.p, s);  // 3: scale
    mark(5);
    CBG_HIP(hipStreamSynchronize(s));
    for (int i = 0; ms && i < 3; ++i) {
      float t = 0.f;
      CBG_HIP(hipEventElapsedTime(&t, ev[2 * i], ev[2 * i + 1]));
      ms[i] = t;
    }
  });
  for (hipEvent_t e : ev)
    if (e) (void)hipEventDestroy(e);
  return cc.agree_vals(rc, nullptr, 0, nullptr);
}

// ---------------------------------------------------------------------------
// Loops on the diagonal (SpParMat.cpp:3257-3335).  Local column j of the tile is
// global column coff + j; its diagonal entry is local row coff + j - roff, inside
// the tile when that is in [0, m).
//   k_loop_count: per dense column its new length, where the diagonal row sorts
//                 into it and whether it is there;
//   EmitLoops:    a wave copies the column, shifted by the removed or inserted
//                 entry (rows stay ascending).
// ---------------------------------------------------------------------------
namespace {
enum { LOOP_REMOVE = 0, LOOP_ADD = 1 };
enum { DIAG_HERE = 1, DIAG_STORED = 2 };

__global__ void k_loop_count(const int64_t* __restrict__ cp, const int32_t* __restrict__ ir,
                             const int32_t* __restrict__ pos, int64_t m, int64_t n, int64_t diag_off, int mode,
                             int64_t* __restrict__ nlen, int32_t* __restrict__ code, int32_t* __restrict__ at,
                             u64* __restrict__ nfound) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int32_t p = pos[j];
  const int64_t b = p < 0 ? 0 : cp[p], e = p < 0 ? 0 : cp[p + 1];
  const int64_t r = j + diag_off;
  int c = 0;
  int64_t k = 0;
  if (r >= 0 && r < m) {
    c = DIAG_HERE;
    k = lower_bound_g64(ir, b, e, (int)r);
    if (k < e && ir[k] == (int32_t)r) c |= DIAG_STORED;
    k -= b;
  }
  int64_t len = e - b;
  if (c & DIAG_HERE) {
    if (mode == LOOP_REMOVE && (c & DIAG_STORED)) --len;
    if (mode == LOOP_ADD && !(c & DIAG_STORED)) ++len;
  }
  if (c & DIAG_STORED) atomicAdd(nfound, 1ull);
  nlen[j] = len;
  code[j] = c;
  at[j] = (int32_t)k;
}

struct EmitLoops {
  const int64_t* cp;
  const int32_t* ir;
  const double* val;
  const int32_t* pos;
  int64_t diag_off;
  int mode, replace, fix_min;
  const double* loopval;
  const int32_t *code, *at;
  __device__ __forceinline__ void operator()(int64_t j, int64_t o, int32_t* oir, double* oval) const {
    const int lane = lane_id();
    const int32_t p = pos[j];
    const int64_t b = p < 0 ? 0 : cp[p], len = p < 0 ? 0 : cp[p + 1] - b;
    const int c = code[j];
    const int64_t k = at[j];
    const bool here = c & DIAG_HERE, stored = c & DIAG_STORED;
    const bool drop = mode == LOOP_REMOVE && stored, insert = mode == LOOP_ADD && here && !stored;
    for (int64_t i = lane; i < len; i += WAVE) {
      if (drop && i == k) continue;
      double v = val[b + i];
      if (fix_min && v == DBL_MIN) v = 1.0;  // AdjustLoops' Apply (MCL.cpp:469)
      if (mode == LOOP_ADD && stored && replace && i == k) v = loopval[j];
      const int64_t d = o + i - (drop && i > k ? 1 : 0) + (insert && i >= k ? 1 : 0);
      oir[d] = ir[b + i];
      oval[d] = v;
    }
    if (insert && lane == 0) {
      oir[o + k] = (int32_t)(j + diag_off);
      oval[o + k] = loopval[j];
    }
  }
};
}  // namespace

// mode LOOP_REMOVE / LOOP_ADD on one tile; loopval: device, n entries (ADD); found: the
// diagonal entries the tile stored before the call
void tile_edit_loops_device(const cbg_tile& T, int64_t diag_off, int mode, int replace, int fix_min,
                            const double* loopval, cbg_tile& out, int64_t* found, hipStream_t s) {
  const int64_t n = T.n;
  if (n <= 0) {
    tile_alloc_device(out, T.m, T.n, 0, 0);
    if (found) *found = 0;
    return;
  }
  DBuf<int64_t> nlen(n + 1);
  DBuf<int32_t> pos(n), code(n), at(n);
  DBuf<u64> nf(1);
  CBG_HIP(hipMemsetAsync(nf.p, 0, sizeof(u64), s));
  tile_col_map(T, pos.p, nullptr, s);
  hipLaunchKernelGGL(k_loop_count, dim3(nblk(n, 256)), dim3(256), 0, s, T.cp, T.ir, pos.p, T.m, n, diag_off, mode, nlen.p,
                     code.p, at.p, nf.p);
  int64_t nfound = 0;  // read back with the totals
  tile_from_columns(T.m, T.n, n, nullptr, nlen.p,
                    EmitLoops{T.cp, T.ir, T.val, pos.p, diag_off, mode, replace, fix_min, loopval, code.p, at.p}, out, s,
                    reinterpret_cast<const int64_t*>(nf.p), &nfound);
  if (found) *found = nfound;
}

// ---------------------------------------------------------------------------
// Connected components: a dense label vector L over the gn vertices (L[v] <= v,
// a vertex of v's component).  Every stored entry (i, j) is an undirected edge.
//   k_cc_hook: m = min(L[i], L[j]) goes to i, j and their labels' entries by
//              atomicMin (vector atomics); *changed counts the lowered labels;
//   k_cc_jump: every vertex follows the labels down to a fixed point.
// ---------------------------------------------------------------------------
namespace {
__global__ void k_cc_init(u64* L, int64_t n) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) L[v] = (u64)v;
}

__global__ __launch_bounds__(256) void k_cc_hook(const int64_t* __restrict__ cp, const int32_t* __restrict__ jc,
                                                 const int32_t* __restrict__ ir, int64_t nzc, int64_t roff,
                                                 int64_t coff, int64_t gn, u64* L, u64* changed) {
  const int64_t p = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (p >= nzc) return;
  const u64 v = (u64)(coff + jc[p]);
  unsigned lowered = 0;
  for (int64_t q = cp[p] + lane_id(); q < cp[p + 1]; q += WAVE) {
    const u64 u = (u64)(roff + ir[q]);
    if (u >= (u64)gn || v >= (u64)gn) continue;  // (a rectangular tile's rows beyond the vertices)
    const u64 lu = L[u], lv = L[v];
    if (lu == lv) continue;
    const u64 lo = lu < lv ? lu : lv, hi = lu < lv ? lv : lu;  // hi <= max(u, v) < gn
    lowered += atomicMin(&L[hi], lo) > lo;
    lowered += atomicMin(lu < lv ? &L[v] : &L[u], lo) > lo;
  }
  if (lowered) atomicAdd(changed, 1ull);
}

__global__ void k_cc_jump(u64* L, int64_t n) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  u64 l = L[v];
  for (u64 nx = L[l]; nx < l; nx = L[l]) l = nx;  // strictly down: ends at a vertex that labels itself
  L[v] = l;
}

__global__ void k_cc_min(u64* __restrict__ L, const u64* __restrict__ all, int P, int64_t n, u64* changed) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  u64 l = L[v];
  const u64 mine = l;
  for (int r = 0; r < P; ++r) l = all[(size_t)r * n + v] < l ? all[(size_t)r * n + v] : l;
  if (l < mine) {
    L[v] = l;
    atomicAdd(changed, 1ull);
  }
}
}  // namespace

void cc_init_device(uint64_t* L, int64_t gn, hipStream_t s) {
  if (gn > 0) hipLaunchKernelGGL(k_cc_init, dim3(nblk(gn, 256)), dim3(256), 0, s, (u64*)L, gn);
  CBG_HIP(hipGetLastError());
}
// one round on this rank's tile: hook, then jump; *changed (device counter) is raised by lowered labels
void cc_round_device(const cbg_tile& T, int64_t roff, int64_t coff, uint64_t* L, int64_t gn, uint64_t* changed,
                     hipStream_t s) {
  if (gn <= 0) return;
  if (T.nzc > 0)
    hipLaunchKernelGGL(k_cc_hook, dim3(nblk(T.nzc * WAVE, 256)), dim3(256), 0, s, T.cp, T.jc, T.ir, T.nzc, roff, coff, gn,
                       (u64*)L, (u64*)changed);
  hipLaunchKernelGGL(k_cc_jump, dim3(nblk(gn, 256)), dim3(256), 0, s, (u64*)L, gn);
  CBG_HIP(hipGetLastError());
}
// L = elementwise minimum of L and the P gathered vectors
void cc_min_device(uint64_t* L, const uint64_t* all, int P, int64_t gn, uint64_t* changed, hipStream_t s) {
  if (gn <= 0) return;
  hipLaunchKernelGGL(k_cc_min, dim3(nblk(gn, 256)), dim3(256), 0, s, (u64*)L, (const u64*)all, P, gn, (u64*)changed);
  hipLaunchKernelGGL(k_cc_jump, dim3(nblk(gn, 256)), dim3(256), 0, s, (u64*)L, gn);
  CBG_HIP(hipGetLastError());
}

}  // namespace cbg
