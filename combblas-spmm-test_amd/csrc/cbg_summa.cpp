// cbg_summa.cpp -- 2D Sparse SUMMA over RCCL (xGMI), one process per GPU.
//
// Replaces, for the SpGEMM path:
//   CommGrid (reference src/CommGrid.cpp:37-75; rank -> (rank / cols, rank % cols),
//             row/col communicators by MPI_Comm_split)       -> ncclCommInitRank + ncclCommSplit
//   ProductGrid (CommGrid.cpp:164-180)                        -> grid reuse (no per-call dup)
//   SpParHelper::GetSetSizes (SpParHelper.cpp:797-809)        -> one allgather of {m,n,nnz,nzc}
//   SpParHelper::BCastMatrix (SpParHelper.cpp:582-600)        -> 4 x ncclBroadcast in a group
//   Mult_AnXBn_DoubleBuff / Mult_AnXBn_Synch (ParFriends.h:798-1108)
//
// Two execution modes with identical results (up to fp summation order):
//   PANEL  : every rank gathers its A block row and B block column (the same
//            broadcasts as the SUMMA stages, issued back to back on the comm
//            stream), concatenates them in HBM and runs ONE local multiply.
//            No partial products, no merge (the reference's dominant cost,
//            69 % of DoubleBuff at 1x1).  Works on any pr x pc grid because
//            the inner coordinates are global.
//            The B block column arrives in column pieces: the broadcast of
//            piece p+1 runs on the comm stream while piece p multiplies on
//            the compute stream (double buffering), and the pieces' C entries
//            are written end to end into one growable arena (no copy).
//   STAGED : the reference's stage structure (sqrt(P) stages for Synch,
//            2 sqrt(P) half-tile stages for DoubleBuff on square grids),
//            generalized to pr x pc grids by cutting the inner dimension at
//            the union of A's column-block and B's row-block boundaries; the
//            broadcast of stage s+1 runs on the comm stream while stage s
//            multiplies on the compute stream; partial products are merged
//            on device (cbg_merge.hip, 64-bit entry counts).
//
// Failure semantics.  The reference MPI_Aborts the whole job on a failed
// check (ParFriends.h:160-183, SpDefs.h:69-76).  Here every collective entry
// point agrees on a return code: after each local step the ranks take the
// maximum of their codes over the world (agree()), so a rank-local failure
// (an OOM inside the local multiply, a receive buffer that cannot be
// allocated, a HIP error) makes every rank leave the call with that code,
// after the collectives already posted have drained, instead of the others
// blocking in the next broadcast.  Communicator failures (an RCCL async
// error, or no progress for CBG_COMM_TIMEOUT_S seconds, default 600) abort
// the grid's communicators (ncclCommAbort); the grid is then unusable and
// every later call returns CBG_ERR_RCCL.
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <thread>

#include "cbg_internal.h"

namespace cbg {

struct RcclError : std::runtime_error {
  explicit RcclError(const std::string& s) : std::runtime_error(s) {}
};
#define CBG_NCCL(x)                                                                                   \
  do {                                                                                                \
    ncclResult_t r_ = (x);                                                                            \
    if (r_ != ncclSuccess)                                                                            \
      throw ::cbg::HipError(std::string(#x) + ": " + ncclGetErrorString(r_), CBG_ERR_RCCL);           \
  } while (0)

}  // namespace cbg

struct cbg_grid {
  int rank = 0, nranks = 1, pr = 1, pc = 1, prow = 0, pcol = 0;
  bool host_mode = false;
  cbg_host_comm hc{};
  ncclComm_t world = nullptr, row = nullptr, col = nullptr;
  hipStream_t compute = nullptr, comm = nullptr;
  hipEvent_t ev_comm = nullptr;
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;  // timing of the first piece's broadcast
  bool broken = false;  // communicators aborted: every later collective fails
  int64_t calls = 0;    // SUMMA calls made on this grid (fault-injection index)
  int64_t redist_calls = 0;  // Transpose / BlockSplit calls (CBG_FAULT_INJECT_REDIST index)
  bool fault_armed = false;
};

namespace cbg {

enum { COMM_WORLD = 0, COMM_ROW = 1, COMM_COL = 2 };

static ncclComm_t pick(cbg_grid* g, int which) {
  return which == COMM_ROW ? g->row : which == COMM_COL ? g->col : g->world;
}
static int comm_size(cbg_grid* g, int which) { return which == COMM_ROW ? g->pc : which == COMM_COL ? g->pr : g->nranks; }
static int comm_rank(cbg_grid* g, int which) { return which == COMM_ROW ? g->pcol : which == COMM_COL ? g->prow : g->rank; }

void grid_setup_streams(cbg_grid* g) {
  CBG_HIP(hipStreamCreateWithFlags(&g->compute, hipStreamNonBlocking));
  CBG_HIP(hipStreamCreateWithFlags(&g->comm, hipStreamNonBlocking));
  CBG_HIP(hipEventCreateWithFlags(&g->ev_comm, hipEventDisableTiming));
  CBG_HIP(hipEventCreate(&g->ev_t0));
  CBG_HIP(hipEventCreate(&g->ev_t1));
}

int grid_shape(int nranks, int& rows, int& cols) {
  if (rows == 0 && cols == 0) {  // CommGrid.cpp:44-53: square or NOTSQUARE
    int r = 1;
    while ((r + 1) * (r + 1) <= nranks) ++r;
    if (r * r != nranks) return CBG_ERR_NOTSQUARE;
    rows = cols = r;
  }
  if (rows <= 0 || cols <= 0 || rows * cols != nranks) return CBG_ERR_INVALIDPARAMS;
  return CBG_OK;
}

cbg_grid* grid_create_rccl(int rank, int nranks, int rows, int cols, const void* uid) {
  std::unique_ptr<cbg_grid> g(new cbg_grid());
  g->rank = rank;
  g->nranks = nranks;
  g->pr = rows;
  g->pc = cols;
  g->prow = rank / cols;
  g->pcol = rank % cols;
  grid_setup_streams(g.get());
  ncclUniqueId id;
  std::memcpy(&id, uid, sizeof(id));
  CBG_NCCL(ncclCommInitRank(&g->world, nranks, id, rank));
  CBG_NCCL(ncclCommSplit(g->world, g->prow, g->pcol, &g->row, nullptr));  // row comm: rank = pcol
  CBG_NCCL(ncclCommSplit(g->world, g->pcol, g->prow, &g->col, nullptr));  // col comm: rank = prow
  return g.release();
}

cbg_grid* grid_create_host(int rank, int nranks, int rows, int cols, const cbg_host_comm* hc) {
  std::unique_ptr<cbg_grid> g(new cbg_grid());
  g->rank = rank;
  g->nranks = nranks;
  g->pr = rows;
  g->pc = cols;
  g->prow = rank / cols;
  g->pcol = rank % cols;
  g->host_mode = true;
  g->hc = *hc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
    grid_setup_streams(g.get());
  } else {
    (void)hipGetLastError();  // no device: only the host collectives (agree, barrier) are usable
  }
  return g.release();
}

void grid_destroy(cbg_grid* g) {
  if (!g) return;
  if (g->row) ncclCommDestroy(g->row);
  if (g->col) ncclCommDestroy(g->col);
  if (g->world) ncclCommDestroy(g->world);
  if (g->compute) (void)hipStreamDestroy(g->compute);
  if (g->comm) (void)hipStreamDestroy(g->comm);
  if (g->ev_comm) (void)hipEventDestroy(g->ev_comm);
  if (g->ev_t0) (void)hipEventDestroy(g->ev_t0);
  if (g->ev_t1) (void)hipEventDestroy(g->ev_t1);
  delete g;
}

// ---------------------------------------------------------------------------
// collectives
// ---------------------------------------------------------------------------
static void host_check(cbg_grid* g, int rc, const char* what) {
  if (rc != 0) {
    g->broken = true;  // a peer is gone or the transport failed: no later call can agree
    throw HipError(std::string("host transport ") + what + " failed", CBG_ERR_RCCL);
  }
}

static double comm_timeout_s() {
  static const char* e = getenv("CBG_COMM_TIMEOUT_S");
  const double t = e ? atof(e) : 600.0;
  return t > 0 ? t : 600.0;
}

// ncclCommAbort on every communicator of the grid (pending operations are
// cancelled); the grid is unusable afterwards
static void abort_comms(cbg_grid* g) {
  for (ncclComm_t* c : {&g->row, &g->col, &g->world})
    if (*c) {
      (void)ncclCommAbort(*c);
      *c = nullptr;
    }
  g->broken = true;
}

static void check_usable(cbg_grid* g) {
  if (g->broken) throw HipError("grid communicators were aborted after an earlier failure", CBG_ERR_RCCL);
}

// Wait for the comm stream (the caller's collectives) with a watchdog:
// an RCCL async error on any communicator, or no completion within
// CBG_COMM_TIMEOUT_S, aborts the communicators instead of hanging.
static void wait_comm(cbg_grid* g) {
  if (g->host_mode) {
    CBG_HIP(hipStreamSynchronize(g->comm));
    return;
  }
  const auto t0 = std::chrono::steady_clock::now();
  const double limit = comm_timeout_s();
  int spins = 0;
  for (;;) {
    hipError_t q = hipStreamQuery(g->comm);
    if (q == hipSuccess) return;
    if (q != hipErrorNotReady) {
      (void)hipGetLastError();
      abort_comms(g);
      throw HipError(std::string("comm stream: ") + hipGetErrorString(q), CBG_ERR_HIP);
    }
    for (ncclComm_t c : {g->world, g->row, g->col}) {
      ncclResult_t ae = ncclSuccess;
      if (c && ncclCommGetAsyncError(c, &ae) == ncclSuccess && ae != ncclSuccess && ae != ncclInProgress) {
        abort_comms(g);
        throw HipError(std::string("RCCL async error: ") + ncclGetErrorString(ae), CBG_ERR_RCCL);
      }
    }
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (el > limit) {
      abort_comms(g);
      throw HipError("collective made no progress for " + std::to_string((int)limit) +
                         " s (CBG_COMM_TIMEOUT_S); communicators aborted",
                     CBG_ERR_RCCL);
    }
    if (++spins > 64) std::this_thread::sleep_for(std::chrono::microseconds(spins > 4096 ? 200 : 20));
  }
}

// allgather of n int64 per rank (host buffers)
void allgather_i64(cbg_grid* g, int which, const int64_t* in, int64_t* out, int n) {
  check_usable(g);
  const int P = comm_size(g, which);
  if (g->host_mode) {
    if (P == 1) {
      std::memcpy(out, in, sizeof(int64_t) * n);
      return;
    }
    host_check(g, g->hc.allgather(g->hc.user, which, in, out, sizeof(int64_t) * n), "allgather");
    return;
  }
  // RCCL: executed for one-rank communicators too (a 1x1 RCCL grid runs the same calls)
  DBuf<int64_t> d(P * n + n);
  CBG_HIP(hipMemcpyAsync(d.p + P * n, in, sizeof(int64_t) * n, hipMemcpyHostToDevice, g->comm));
  CBG_NCCL(ncclAllGather(d.p + P * n, d.p, n, ncclInt64, pick(g, which), g->comm));
  CBG_HIP(hipMemcpyAsync(out, d.p, sizeof(int64_t) * P * n, hipMemcpyDeviceToHost, g->comm));
  wait_comm(g);
}

// allgather of `bytes` bytes per rank (host buffers)
static void allgather_bytes(cbg_grid* g, int which, const void* in, void* out, size_t bytes) {
  check_usable(g);
  const int P = comm_size(g, which);
  if (bytes == 0) return;
  if (g->host_mode) {
    if (P == 1) {
      std::memcpy(out, in, bytes);
      return;
    }
    host_check(g, g->hc.allgather(g->hc.user, which, in, out, bytes), "allgather");
    return;
  }
  DBuf<char> d((size_t)(P + 1) * bytes);
  CBG_HIP(hipMemcpyAsync(d.p + P * bytes, in, bytes, hipMemcpyHostToDevice, g->comm));
  CBG_NCCL(ncclAllGather(d.p + P * bytes, d.p, bytes, ncclInt8, pick(g, which), g->comm));
  CBG_HIP(hipMemcpyAsync(out, d.p, (size_t)P * bytes, hipMemcpyDeviceToHost, g->comm));
  wait_comm(g);
}

// allgather of `bytes` bytes per rank of DEVICE buffers (stream-ordered on the
// comm stream and waited for); the host transport stages through host memory
static void allgather_device(cbg_grid* g, int which, const void* in, void* out, size_t bytes) {
  check_usable(g);
  if (bytes == 0) return;
  const int P = comm_size(g, which);
  if (P == 1) {
    CBG_HIP(hipMemcpy(out, in, bytes, hipMemcpyDeviceToDevice));
    return;
  }
  if (g->host_mode) {
    std::vector<char> h(bytes), all((size_t)P * bytes);
    CBG_HIP(hipMemcpy(h.data(), in, bytes, hipMemcpyDeviceToHost));
    allgather_bytes(g, which, h.data(), all.data(), bytes);
    CBG_HIP(hipMemcpy(out, all.data(), all.size(), hipMemcpyHostToDevice));
    return;
  }
  CBG_NCCL(ncclAllGather(in, out, bytes, ncclInt8, pick(g, which), g->comm));
  wait_comm(g);
}

void allreduce_f64(cbg_grid* g, double* v, bool max) {
  check_usable(g);
  if (g->host_mode) {
    if (g->nranks == 1) return;
    std::vector<double> all(g->nranks);
    host_check(g, g->hc.allgather(g->hc.user, COMM_WORLD, v, all.data(), sizeof(double)), "allgather");
    double r = all[0];
    for (double x : all) r = max ? std::max(r, x) : r + x;
    *v = r;
    return;
  }
  DBuf<double> d(1);
  CBG_HIP(hipMemcpyAsync(d.p, v, sizeof(double), hipMemcpyHostToDevice, g->comm));
  CBG_NCCL(ncclAllReduce(d.p, d.p, 1, ncclFloat64, max ? ncclMax : ncclSum, g->world, g->comm));
  CBG_HIP(hipMemcpyAsync(v, d.p, sizeof(double), hipMemcpyDeviceToHost, g->comm));
  wait_comm(g);
}

void allreduce_sum_i64(cbg_grid* g, int64_t* v) {
  std::vector<int64_t> all(g->nranks);
  allgather_i64(g, COMM_WORLD, v, all.data(), 1);
  int64_t s = 0;
  for (auto x : all) s += x;
  *v = s;
}

void barrier(cbg_grid* g) {
  double z = 0;
  allreduce_f64(g, &z, true);
}

// The agreed code of a collective step: max over the world of the ranks'
// local codes (0 = success).  Every rank calls it at the same points, so a
// failed rank never leaves its peers blocked in a broadcast it skipped.
int agree(cbg_grid* g, int rc) {
  int64_t v = rc, w = 0;
  std::vector<int64_t> all(g->nranks);
  allgather_i64(g, COMM_WORLD, &v, all.data(), 1);
  for (auto x : all) w = std::max(w, x);
  return (int)w;
}
// agree() that also reduces one value over the world: *vmin / *vmax receive
// its minimum / maximum (one allgather, the same point of the protocol)
static int agree_val(cbg_grid* g, int rc, int64_t val, int64_t* vmin, int64_t* vmax) {
  int64_t v[2] = {rc, val};
  std::vector<int64_t> all((size_t)2 * g->nranks);
  allgather_i64(g, COMM_WORLD, v, all.data(), 2);
  int64_t w = 0, lo = val, hi = val;
  for (int r = 0; r < g->nranks; ++r) {
    w = std::max(w, all[2 * r]);
    lo = std::min(lo, all[2 * r + 1]);
    hi = std::max(hi, all[2 * r + 1]);
  }
  if (vmin) *vmin = lo;
  if (vmax) *vmax = hi;
  return (int)w;
}

// Test hook (CBG_FAULT_INJECT="rank:k1,k2,..."): in the listed SUMMA calls
// that rank `rank` makes on a grid (counted from 0 over the grid's life), the
// first local multiply fails as an out-of-memory would.
static void arm_fault(cbg_grid* g) {
  static const char* e = getenv("CBG_FAULT_INJECT");
  const int64_t k = g->calls++;
  g->fault_armed = false;
  if (!e) return;
  const char* c = strchr(e, ':');
  if (!c || atoi(e) != g->rank) return;
  for (const char* q = c + 1; *q;) {
    char* end = nullptr;
    const long long at = strtoll(q, &end, 10);
    if (end == q) break;
    if (at == k) g->fault_armed = true;
    q = *end == ',' ? end + 1 : end;
  }
}
static void maybe_inject_fault(cbg_grid* g) {
  if (!g->fault_armed) return;
  g->fault_armed = false;
  throw HipError("injected fault (CBG_FAULT_INJECT) in SUMMA call " + std::to_string(g->calls - 1), CBG_ERR_OOM);
}
// the same for the redistributions (Transpose, BlockSplit):
// CBG_FAULT_INJECT_REDIST="rank:k1,k2,..." counts their calls on a grid, and
// the listed calls of that rank fail their receive-buffer allocation as an
// out-of-memory would
static bool redist_fault(cbg_grid* g) {
  static const char* e = getenv("CBG_FAULT_INJECT_REDIST");
  const int64_t k = g->redist_calls++;
  if (!e) return false;
  const char* c = strchr(e, ':');
  if (!c || atoi(e) != g->rank) return false;
  for (const char* q = c + 1; *q;) {
    char* end = nullptr;
    const long long at = strtoll(q, &end, 10);
    if (end == q) break;
    if (at == k) return true;
    q = *end == ',' ? end + 1 : end;
  }
  return false;
}

std::string& step_error() {  // see step() in cbg_internal.h
  static thread_local std::string m;
  return m;
}

// Broadcast a tile within a row/col communicator (BCastMatrix: the essentials
// {m,n,nnz,nzc} are known from the allgather; Create(ess) then 4 broadcasts).
// `t` is the root's tile on the root and an allocated receive tile elsewhere.
// RCCL: enqueued on g->comm (callers group the broadcasts of one step and
// order the consumer with g->ev_comm); host transport: synchronous.
static void bcast_tile(cbg_grid* g, int which, int root, const int64_t ess[4], cbg_tile& t, bool mine) {
  const int64_t nnz = ess[2], nzc = ess[3];
  if (g->host_mode) {
    if (comm_size(g, which) == 1) return;
    CBG_HIP(hipStreamSynchronize(g->comm));
    auto hb = [&](void* dptr, size_t bytes) {
      if (bytes == 0) {
        // the host transport's collectives are synchronous over the WORLD: an empty tile in
        // one grid row (column) must not skip an exchange that the other rows (columns) make
        char none = 0;
        host_check(g, g->hc.bcast(g->hc.user, which, &none, 1, root), "bcast");
        return;
      }
      std::vector<char> h(bytes);
      if (mine) CBG_HIP(hipMemcpy(h.data(), dptr, bytes, hipMemcpyDeviceToHost));
      host_check(g, g->hc.bcast(g->hc.user, which, h.data(), bytes, root), "bcast");
      if (!mine) CBG_HIP(hipMemcpy(dptr, h.data(), bytes, hipMemcpyHostToDevice));
    };
    hb(t.cp, sizeof(int64_t) * (nzc + 1));
    hb(t.jc, sizeof(int32_t) * nzc);
    hb(t.ir, sizeof(int32_t) * nnz);
    hb(t.val, sizeof(double) * nnz);
    return;
  }
  // RCCL, one-rank communicators included
  ncclComm_t c = pick(g, which);
  CBG_NCCL(ncclBroadcast(t.cp, t.cp, nzc + 1, ncclInt64, root, c, g->comm));
  if (nzc) CBG_NCCL(ncclBroadcast(t.jc, t.jc, nzc, ncclInt32, root, c, g->comm));
  if (nnz) {
    CBG_NCCL(ncclBroadcast(t.ir, t.ir, nnz, ncclInt32, root, c, g->comm));
    CBG_NCCL(ncclBroadcast(t.val, t.val, nnz, ncclFloat64, root, c, g->comm));
  }
}

// one step's broadcasts as one RCCL group
template <class F>
static void bcast_group(cbg_grid* g, F&& f) {
  if (!g->host_mode) CBG_NCCL(ncclGroupStart());
  try {
    f();
  } catch (...) {
    if (!g->host_mode) (void)ncclGroupEnd();
    throw;
  }
  if (!g->host_mode) CBG_NCCL(ncclGroupEnd());
}

static void tile_ess(const cbg_tile& t, int64_t e[4]) {
  e[0] = t.m;
  e[1] = t.n;
  e[2] = t.nnz;
  e[3] = t.nzc;
}

static void alloc_like(cbg_tile& t, const int64_t e[4]) { tile_alloc_device(t, e[0], e[1], e[2], e[3]); }

// ---------------------------------------------------------------------------
// PANEL (pipelined): Mult_AnXBn_DoubleBuff / _Synch as ONE local multiply of
// the A block row by the B block column (ParFriends.h:845-964 computes the
// same sum of stage products), the B block column arriving in column pieces
// cuts[0] = 0 < cuts[1] < ... < cuts[np] = B.n.  Comm stream, every rank in
// the same order: [A row broadcasts][piece 0][agree][piece 1][agree]...;
// the compute stream multiplies piece p while piece p+1 is broadcast.
// fn != NULL: each piece's C goes to fn and is freed (MemEfficientSpGEMM
// phases); else the pieces' entries go end to end into one EntryArena and C
// is their column concatenation (ColConcatenate without a copy).
// ---------------------------------------------------------------------------
static int64_t tile_bytes(const int64_t e[4]) { return 8 * (e[3] + 1) + 4 * e[3] + 12 * e[2]; }

SummaInfo& summa_info() {
  static thread_local SummaInfo s;
  return s;
}

// extra local multiply an additional pipeline piece costs (CBG_PIPELINE_MIN_MS):
// measured 2.5-3.0 ms on scale-22 rank tiles of 2x2 and 4x2 grids (68-132 ms)
static double pipeline_min_ms() {
  static const char* e = getenv("CBG_PIPELINE_MIN_MS");
  return e ? atof(e) : 3.0;
}
// ... and on larger tiles a share of the rank's multiply (CBG_PIPELINE_COST_FRAC,
// default 0.04: 1-7 % measured on the scale-22 2x1 rank tiles of 258 ms), taken
// from this thread's previous adaptive PANEL call (the same product repeated)
static thread_local double g_last_panel_ms = 0.0;
static double pipeline_cost_ms() {
  static const char* e = getenv("CBG_PIPELINE_COST_FRAC");
  static const double frac = e ? atof(e) : 0.04;
  return std::max(pipeline_min_ms(), frac * g_last_panel_ms);
}

// One phase's local multiply handed to fn (MemEfficientSpGEMM with a phase
// consumer).  A phase whose C does not fit the device -- the multiply learns
// nnz(C) from its symbolic pass and its allocation fails with CBG_ERR_OOM
// before any output is written -- is computed as two column halves of its B
// piece, each handed to fn with the same phase index and its own column
// offset, so an underestimated phase count costs a repeated symbolic pass, not
// the job.  The split is local: the piece's B columns are already on this rank.
static void multiply_to_fn(const cbg_tile& A, const cbg_tile& B, int sr, hipStream_t cs, int p, int64_t off,
                           cbg_phase_fn fn, void* user, int& cb_rc, double& ms, int depth) {
  TileGuard Cp;
  LocalStats ls;
  try {
    local_spgemm(A, B, sr, Cp.t, cs, &ls, nullptr);
  } catch (const HipError& e) {
    if (e.code != CBG_ERR_OOM || B.n < 2 || depth >= 12) throw;
    pool().trim();
    summa_info().oom_splits++;
    const int64_t h = B.n / 2;
    for (int k = 0; k < 2; ++k) {
      TileGuard half;
      tile_slice_cols(B, k ? h : 0, k ? B.n : h, half.t, cs);
      multiply_to_fn(A, half.t, sr, cs, p, off + (k ? h : 0), fn, user, cb_rc, ms, depth + 1);
    }
    return;
  }
  ms += ls.ms_symbolic + ls.ms_numeric;
  CBG_HIP(hipStreamSynchronize(cs));
  const int r = fn(user, p, off, &Cp.t);
  if (r && !cb_rc) cb_rc = r;
}

// CUs the persistent slab kernels leave free while a broadcast is in flight
static int comm_reserve_default() { return 8; }

// one_phase: the cuts are pipeline pieces of ONE phase (fn gets phase 0 for
// each of them, at its column offset), else piece p is phase p
static int summa_panel(cbg_grid* g, const cbg_tile& A, const cbg_tile& B, int64_t A_gncol, int64_t B_gnrow, int sr,
                       const std::vector<int64_t>& cuts_in, cbg_phase_fn fn, void* user, cbg_tile* C,
                       bool adaptive = false, bool one_phase = false) {
  std::vector<int64_t> cuts = cuts_in;
  int np = (int)cuts.size() - 1;
  const int pr = g->pr, pc = g->pc;
  hipStream_t cs = g->compute;
  // my B pieces (column slices; the whole tile when np == 1)
  std::vector<TileGuard> own(np);
  std::vector<cbg_tile> piece(np);
  int rc = step([&] {
    for (int p = 0; p < np; ++p) {
      if (np == 1) {
        piece[p] = B;
      } else {
        tile_slice_cols(B, cuts[p], cuts[p + 1], own[p].t, cs);
        piece[p] = own[p].t;
      }
    }
  });
  if ((rc = agree(g, rc))) return rc;
  // GetSetSizes: A tiles along my grid row, every piece of the B tiles along my grid column
  int64_t ea[4];
  tile_ess(A, ea);
  std::vector<int64_t> eb((size_t)4 * np);
  for (int p = 0; p < np; ++p) tile_ess(piece[p], &eb[4 * p]);
  std::vector<int64_t> EA((size_t)4 * pc), EB((size_t)4 * np * pr);
  allgather_i64(g, COMM_ROW, ea, EA.data(), 4);
  allgather_i64(g, COMM_COL, eb.data(), EB.data(), 4 * np);
  auto eB = [&](int s, int p) { return &EB[(size_t)4 * (s * np + p)]; };
  int64_t kA = 0, kB = 0;
  for (int s = 0; s < pc; ++s) kA += EA[4 * s + 1];
  for (int s = 0; s < pr; ++s) kB += eB(s, 0)[0];
  if ((rc = agree(g, (kA != A_gncol || kB != B_gnrow) ? CBG_ERR_DIMMISMATCH : CBG_OK))) return rc;
  std::vector<int64_t> aoff(pc + 1, 0), boff(pr + 1, 0);
  for (int s = 0; s < pc; ++s) aoff[s + 1] = aoff[s] + EA[4 * s + 1];
  for (int s = 0; s < pr; ++s) boff[s + 1] = boff[s] + eB(s, 0)[0];

  std::vector<TileGuard> Ar(pc);
  std::vector<std::vector<TileGuard>> Bc(np);
  for (auto& v : Bc) v.resize(pr);
  auto alloc_piece = [&](int p) {
    for (int s = 0; s < pr; ++s)
      if (s != g->prow) alloc_like(Bc[p][s].t, eB(s, p));
  };
  auto post_piece = [&](int p) {
    bcast_group(g, [&] {
      for (int s = 0; s < pr; ++s)
        bcast_tile(g, COMM_COL, s, eB(s, p), s == g->prow ? piece[p] : Bc[p][s].t, s == g->prow);
    });
    CBG_HIP(hipEventRecord(g->ev_comm, g->comm));
  };
  rc = step([&] {
    for (int s = 0; s < pc; ++s)
      if (s != g->pcol) alloc_like(Ar[s].t, &EA[4 * s]);
    alloc_piece(0);
  });
  if ((rc = agree(g, rc))) return rc;
  // from here on every rank has posted the same broadcasts: errors are
  // recorded, agreed on at the next step, and the comm stream is drained
  SummaInfo& info = summa_info();
  info = SummaInfo{};
  info.pieces = np;
  // bytes this rank receives: the remote A tiles of its grid row and the remote
  // B tiles (all pieces) of its grid column
  int64_t bytes_a = 0, bytes_b0 = 0, bytes_b1 = 0;
  for (int s = 0; s < pc; ++s)
    if (s != g->pcol) bytes_a += tile_bytes(&EA[4 * s]);
  for (int s = 0; s < pr; ++s)
    if (s != g->prow)
      for (int p = 0; p < np; ++p) (p == 0 ? bytes_b0 : bytes_b1) += tile_bytes(eB(s, p));
  info.bytes_recv = bytes_a + bytes_b0 + bytes_b1;
  double host_ms0 = 0.0;
  // the A block row's gather and B piece 0 in ONE broadcast group (their
  // transfers overlap on the row and column links); piece 0's multiply waits
  // for both
  int local = step([&] {
    CBG_HIP(hipEventRecord(g->ev_t0, g->comm));
    const auto h0 = std::chrono::steady_clock::now();
    bcast_group(g, [&] {
      for (int s = 0; s < pc; ++s) {
        cbg_tile& t = s == g->pcol ? const_cast<cbg_tile&>(A) : Ar[s].t;
        bcast_tile(g, COMM_ROW, s, &EA[4 * s], t, s == g->pcol);
      }
      for (int s = 0; s < pr; ++s)
        bcast_tile(g, COMM_COL, s, eB(s, 0), s == g->prow ? piece[0] : Bc[0][s].t, s == g->prow);
    });
    CBG_HIP(hipEventRecord(g->ev_comm, g->comm));
    CBG_HIP(hipEventRecord(g->ev_t1, g->comm));
    host_ms0 = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
  });
  // Double buffering (PANEL with the default two pieces on a grid).  On RCCL
  // grids whose B block column has more than one remote tile (pr >= 3) piece 1
  // is always broadcast while piece 0 multiplies (rule 1).  Otherwise
  // (one remote B tile, or the host transport) adaptively: the first group's
  // measured time (A gather + piece 0, 1/8 of B's columns), scaled to the
  // rest's bytes, is the transfer that pipelining would hide behind piece 0's
  // multiply; an extra piece costs about pipeline_cost_ms() of compute, so the
  // ranks keep the two pieces only when the hidden transfer is larger (rule 2,
  // agreed over the grid: every rank cuts its B tile alike); otherwise the
  // rest is broadcast at once and the pieces are rejoined into one multiply
  // (rule 3).
  if (np == 2 && adaptive && !g->host_mode && pr >= 3) info.rule = 1;
  // several pieces without the adaptive decision (CBG_PIPELINE, or the phases
  // of MemEfficientSpGEMM given as pieces): a fixed pipeline (rule 4)
  if (np > 1 && !adaptive) info.rule = 4;
  if (adaptive && np == 2 && !local && info.rule == 0) {
    float ms0 = 0.f;
    local = step([&] {
      wait_comm(g);
      if (g->host_mode) ms0 = (float)host_ms0;
      else CBG_HIP(hipEventElapsedTime(&ms0, g->ev_t0, g->ev_t1));
    });
    const int64_t b0 = bytes_a + bytes_b0, b1 = bytes_b1;
    const double hidden = b0 > 0 ? ms0 * (double)b1 / (double)b0 : 0.0;
    info.bcast_ms_piece0 = ms0;
    info.est_hidden_ms = hidden;
    info.piece_cost_ms = pipeline_cost_ms();
    const int want = hidden > info.piece_cost_ms ? 1 : 0;
    const int dec = agree(g, local ? local : want);  // codes >= 3001 are failures
    info.rule = dec == 1 ? 2 : 3;
    if (dec > 1) {
      rc = dec;
    } else if (dec == 0) {
      local = step([&] { alloc_piece(1); });
      if (!(rc = agree(g, local))) {
        local = step([&] {
          post_piece(1);
          wait_comm(g);  // the rest arrives now (its transfer is cheaper than a piece)
          for (int s = 0; s < pr; ++s) {
            const bool me = s == g->prow;
            std::vector<cbg_tile> parts = {me ? piece[0] : Bc[0][s].t, me ? piece[1] : Bc[1][s].t};
            TileGuard joined;
            tile_concat_cols(parts, {0, cuts[1]}, eB(s, 0)[0], cuts[2], joined.t, cs);
            if (me) {
              own[0] = std::move(joined);
              piece[0] = own[0].t;
              tile_free_device(own[1].t);
            } else {
              Bc[0][s] = std::move(joined);
              tile_free_device(Bc[1][s].t);
            }
          }
          CBG_HIP(hipEventRecord(g->ev_comm, g->comm));
        });
        np = 1;
        cuts = {0, cuts[2]};
        info.pieces = 1;
      }
    }
  }
  APrepScope aprep_scope;  // every piece multiplies the same A panel: keep its column maps
  std::unique_ptr<EntryArena> arena;
  if (!fn && np > 1) arena.reset(new EntryArena());
  std::vector<TileGuard> outs;
  std::vector<cbg_tile> outv;
  TileGuard Apanel;
  const cbg_tile* Ause = &A;
  int cb_rc = 0;
  double panel_ms = 0.0;
  // exposed communication: the compute stream's wait for each piece's broadcast
  // (an event before and after the wait; ~0 when the broadcast finished first)
  std::vector<hipEvent_t> wev;
  struct EvFree {
    std::vector<hipEvent_t>& v;
    ~EvFree() {
      for (auto e : v) (void)hipEventDestroy(e);
    }
  } wev_free{wev};
  for (int p = 0; p < np && !rc; ++p) {
    local = std::max(local, step([&] {
      hipEvent_t e0 = nullptr, e1 = nullptr;
      CBG_HIP(hipEventCreate(&e0));
      wev.push_back(e0);
      CBG_HIP(hipEventCreate(&e1));
      wev.push_back(e1);
      CBG_HIP(hipEventRecord(e0, cs));
      CBG_HIP(hipStreamWaitEvent(cs, g->ev_comm, 0));
      CBG_HIP(hipEventRecord(e1, cs));
    }));
    if (p + 1 < np) {
      // every rank holds piece p+1's receive buffers before anyone posts it
      local = std::max(local, step([&] { alloc_piece(p + 1); }));
      if ((rc = agree(g, local))) break;
      local = std::max(local, step([&] { post_piece(p + 1); }));
    }
    if (local) continue;  // agreed at the next step
    local = step([&] {
      maybe_inject_fault(g);
      // piece p+1's broadcast runs on the comm stream during this multiply:
      // the persistent kernels leave comm_reserve_default() (8) CUs to it
      CommReserve reserve(p + 1 < np && !g->host_mode ? comm_reserve_default() : 0);
      if (p == 0 && pc > 1) {
        std::vector<cbg_tile> parts(pc);
        for (int s = 0; s < pc; ++s) parts[s] = s == g->pcol ? A : Ar[s].t;
        tile_concat_cols(parts, std::vector<int64_t>(aoff.begin(), aoff.end() - 1), A.m, A_gncol, Apanel.t, cs);
        for (auto& t : Ar) tile_free_device(t.t);
        Ause = &Apanel.t;
      }
      TileGuard Bp;
      const cbg_tile* Buse = &piece[p];
      if (pr > 1) {
        std::vector<cbg_tile> parts(pr);
        for (int s = 0; s < pr; ++s) parts[s] = s == g->prow ? piece[p] : Bc[p][s].t;
        tile_concat_rows(parts, std::vector<int64_t>(boff.begin(), boff.end() - 1), B_gnrow, cuts[p + 1] - cuts[p],
                         Bp.t, cs);
        Buse = &Bp.t;
      }
      if (fn) {
        multiply_to_fn(*Ause, *Buse, sr, cs, one_phase ? 0 : p, cuts[p], fn, user, cb_rc, panel_ms, 0);
        for (auto& t : Bc[p]) tile_free_device(t.t);
        tile_free_device(own[p].t);
      } else {
        TileGuard Cp;
        LocalStats ls;
        local_spgemm(*Ause, *Buse, sr, Cp.t, cs, &ls, arena.get());
        panel_ms += ls.ms_symbolic + ls.ms_numeric;
        for (auto& t : Bc[p]) tile_free_device(t.t);
        tile_free_device(own[p].t);
        outv.push_back(Cp.t);
        outs.push_back(std::move(Cp));
      }
    });
  }
  if (!rc) rc = agree(g, local);
  if (!rc && adaptive) g_last_panel_ms = panel_ms;
  if (!rc) {
    double exposed = 0.0;
    for (size_t k = 0; k + 1 < wev.size(); k += 2) {
      float ms = 0.f;
      if (hipEventSynchronize(wev[k + 1]) == hipSuccess && hipEventElapsedTime(&ms, wev[k], wev[k + 1]) == hipSuccess)
        exposed += ms;
      else
        (void)hipGetLastError();
    }
    info.exposed_comm_ms = exposed;
  }
  if (rc) {
    if (!g->broken) wait_comm(g);  // posted broadcasts complete before their buffers are released
    return rc;
  }
  if (fn) return agree(g, cb_rc ? CBG_ERR_INVALIDPARAMS : CBG_OK);
  rc = step([&] {
    if (np == 1) {
      *C = outs[0].release();
    } else {
      std::vector<int64_t> off(cuts.begin(), cuts.end() - 1);
      tile_assemble_cols(outv, off, A.m, B.n, *arena, *C, cs);
    }
  });
  return agree(g, rc);
}

// ---------------------------------------------------------------------------
// STAGED: the reference's stages (ParFriends.h:845-964 DoubleBuff: A split by
// columns at n/2 and B by rows at m/2, 2 sqrt(P) stages; :1004-1108 Synch:
// sqrt(P) stages), generalized to pr x pc grids: the inner dimension is cut
// at the union of A's column-block and B's row-block boundaries (lcm(pr, pc)
// ranges for power-of-two grids), DoubleBuff halves every range and runs all
// first halves before all second halves.  Stage s+1's broadcasts are posted
// before stage s multiplies; the partials are merged on device (MergeAll /
// MultiwayMerge, 64-bit entry counts).  On square grids the stages, their
// roots and their pieces are exactly the reference's.
// ---------------------------------------------------------------------------
static int summa_staged(cbg_grid* g, const cbg_tile& A, const cbg_tile& B, int64_t A_gncol, int64_t B_gnrow, int sr,
                        int algo, cbg_tile& C) {
  const int pr = g->pr, pc = g->pc;
  hipStream_t cs = g->compute;
  const int64_t K = A_gncol;
  auto blk = [](int64_t ext, int np_, int i) {  // SpParMat::Owner block start
    return i >= np_ ? ext : (int64_t)i * (ext / np_);
  };
  std::vector<int64_t> bnd;
  for (int s = 0; s <= pc; ++s) bnd.push_back(blk(K, pc, s));
  for (int s = 0; s <= pr; ++s) bnd.push_back(blk(K, pr, s));
  std::sort(bnd.begin(), bnd.end());
  bnd.erase(std::unique(bnd.begin(), bnd.end()), bnd.end());
  struct Stage {
    int64_t lo, hi;
    int sa, sb;
  };
  auto owner = [&](int64_t k, int np_) {  // block of inner index k
    int s = (int)std::min<int64_t>(np_ - 1, K / np_ ? k / (K / np_) : np_ - 1);
    while (s > 0 && blk(K, np_, s) > k) --s;
    while (s + 1 < np_ && blk(K, np_, s + 1) <= k) ++s;
    return s;
  };
  std::vector<Stage> st;
  for (int half = 0; half < (algo == CBG_DOUBLEBUFF ? 2 : 1); ++half)
    for (size_t j = 0; j + 1 < bnd.size(); ++j) {
      int64_t lo = bnd[j], hi = bnd[j + 1];
      if (hi <= lo) continue;
      const int sa = owner(lo, pc), sb = owner(lo, pr);
      if (algo == CBG_DOUBLEBUFF) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (half == 0) hi = mid; else lo = mid;
      }
      st.push_back({lo, hi, sa, sb});
    }
  const int S = (int)st.size();
  // the stage slices below assume the block layout (SpParMat::Owner): my A
  // tile holds inner columns blk(K, pc, pcol) .. blk(K, pc, pcol + 1) and my
  // B tile the same rows of B's row blocks; a tile of another width would be
  // cut past its end or lose columns, so it is a dimension mismatch (agreed)
  const bool layout_ok = A.n == blk(K, pc, g->pcol + 1) - blk(K, pc, g->pcol) &&
                         B.m == blk(K, pr, g->prow + 1) - blk(K, pr, g->prow);
  int rc = agree(g, layout_ok ? CBG_OK : CBG_ERR_DIMMISMATCH);
  if (rc) return rc;
  // my pieces: A columns of the stages rooted at my grid column, B rows of those rooted at my grid row
  std::vector<TileGuard> myA(S), myB(S);
  rc = step([&] {
    for (int s = 0; s < S; ++s) {
      if (st[s].sa == g->pcol) {
        const int64_t o = blk(K, pc, st[s].sa);
        tile_slice_cols(A, st[s].lo - o, st[s].hi - o, myA[s].t, cs);
      }
      if (st[s].sb == g->prow) {
        const int64_t o = blk(K, pr, st[s].sb);
        tile_slice_rows(B, st[s].lo - o, st[s].hi - o, myB[s].t, cs);
      }
    }
  });
  if ((rc = agree(g, rc))) return rc;
  std::vector<int64_t> ea((size_t)4 * S, 0), eb((size_t)4 * S, 0);
  for (int s = 0; s < S; ++s) {
    tile_ess(myA[s].t, &ea[4 * s]);
    tile_ess(myB[s].t, &eb[4 * s]);
  }
  std::vector<int64_t> EA((size_t)4 * S * pc), EB((size_t)4 * S * pr);
  allgather_i64(g, COMM_ROW, ea.data(), EA.data(), 4 * S);  // GetSetSizes (ParFriends.h:834-835 / :1025-1026)
  allgather_i64(g, COMM_COL, eb.data(), EB.data(), 4 * S);
  auto eA = [&](int s) { return &EA[(size_t)4 * (st[s].sa * S + s)]; };
  auto eB = [&](int s) { return &EB[(size_t)4 * (st[s].sb * S + s)]; };
  int64_t kA = 0, kB = 0;
  for (int s = 0; s < S; ++s) {
    kA += eA(s)[1];
    kB += eB(s)[0];
  }
  if ((rc = agree(g, (kA != A_gncol || kB != B_gnrow) ? CBG_ERR_DIMMISMATCH : CBG_OK))) return rc;
  std::vector<TileGuard> Ar(S), Bc(S);
  auto alloc_stage = [&](int s) {
    if (st[s].sa != g->pcol) alloc_like(Ar[s].t, eA(s));
    if (st[s].sb != g->prow) alloc_like(Bc[s].t, eB(s));
  };
  auto post = [&](int s) {
    bcast_group(g, [&] {
      bcast_tile(g, COMM_ROW, st[s].sa, eA(s), st[s].sa == g->pcol ? myA[s].t : Ar[s].t, st[s].sa == g->pcol);
      bcast_tile(g, COMM_COL, st[s].sb, eB(s), st[s].sb == g->prow ? myB[s].t : Bc[s].t, st[s].sb == g->prow);
    });
    CBG_HIP(hipEventRecord(g->ev_comm, g->comm));
  };
  rc = step([&] { alloc_stage(0); });
  if ((rc = agree(g, rc))) return rc;
  int local = step([&] { post(0); });
  std::vector<TileGuard> partials;
  std::vector<cbg_tile> pv;
  for (int s = 0; s < S && !rc; ++s) {
    local = std::max(local, step([&] { CBG_HIP(hipStreamWaitEvent(cs, g->ev_comm, 0)); }));
    if (s + 1 < S) {
      local = std::max(local, step([&] { alloc_stage(s + 1); }));
      if ((rc = agree(g, local))) break;
      local = std::max(local, step([&] { post(s + 1); }));
    }
    if (local) continue;
    local = step([&] {
      maybe_inject_fault(g);
      CommReserve reserve(s + 1 < S && !g->host_mode ? comm_reserve_default() : 0);
      const cbg_tile& a = st[s].sa == g->pcol ? myA[s].t : Ar[s].t;
      const cbg_tile& b = st[s].sb == g->prow ? myB[s].t : Bc[s].t;
      TileGuard P;
      local_spgemm(a, b, sr, P.t, cs, nullptr);  // LocalHybridSpGEMM (ParFriends.h:888-891)
      tile_free_device(Ar[s].t);
      tile_free_device(Bc[s].t);
      tile_free_device(myA[s].t);
      tile_free_device(myB[s].t);
      if (P.t.nnz > 0) {
        pv.push_back(P.t);
        partials.push_back(std::move(P));
      }
    });
  }
  if (!rc) rc = agree(g, local);
  if (rc) {
    if (!g->broken) wait_comm(g);
    return rc;
  }
  // MergeAll (DoubleBuff, Friends.h:657-741) / MultiwayMerge (Synch, MultiwayMerge.h:409-526)
  rc = step([&] {
    if (pv.size() == 1) {
      C = partials[0].release();
    } else {
      merge_tiles(pv, A.m, B.n, sr, C, cs);
    }
  });
  return agree(g, rc);
}

// pieces of the pipelined PANEL multiply when C stays resident: the first
// piece small (its broadcast is exposed), the rest behind its multiply.
// CBG_PIPELINE=k: k equal pieces (1 = no pipelining); CBG_PIPELINE=1/d: two
// pieces, the first 1/d of B's columns; default: 1 piece without
// communication (one grid cell), else 1/8.
// The piece COUNT is a collective property (one broadcast group and one
// agree() per piece), so it is chosen from n_min, the narrowest B tile of the
// world (agreed by the caller): every rank cuts its own B tile into the same
// number of nonempty pieces, whatever the widths of the grid's column blocks.
static std::vector<int64_t> pipeline_cuts(cbg_grid* g, int64_t n, int64_t n_min) {
  static const char* e = getenv("CBG_PIPELINE");
  const bool comm = g->pr > 1;  // B tiles are broadcast only along grid columns of >1 rank
  if (n_min < 16) return {0, n};
  if (!e) return comm ? std::vector<int64_t>{0, n / 8, n} : std::vector<int64_t>{0, n};
  if (!strncmp(e, "1/", 2)) {
    const int64_t d = std::min<int64_t>(std::max(2, atoi(e + 2)), n_min);
    return {0, n / d, n};
  }
  int k = atoi(e);
  if (k <= 1) return {0, n};
  k = (int)std::min<int64_t>(k, n_min);
  std::vector<int64_t> c;
  for (int i = 0; i <= k; ++i) c.push_back((int64_t)i * n / k);
  return c;
}

// ---------------------------------------------------------------------------
// Mult_AnXBn_{DoubleBuff,Synch}
// ---------------------------------------------------------------------------
int summa_spgemm(cbg_grid* g, const cbg_tile& A, const cbg_tile& B, int64_t A_gncol, int64_t B_gnrow, int sr, int algo,
                 int exec, cbg_tile& C) {
  check_usable(g);
  arm_fault(g);
  // CheckSpGEMMCompliance (ParFriends.h:160-183), agreed over the grid, with
  // the narrowest B tile of the world (the pipeline's piece count)
  int rc = A_gncol != B_gnrow ? CBG_ERR_DIMMISMATCH
           : (&A == &B || (A.ir == B.ir && A.nnz > 0)) ? CBG_ERR_MATRIXALIAS
           : CBG_OK;
  int64_t n_min = 0;
  if ((rc = agree_val(g, rc, B.n, &n_min, nullptr))) return rc;
  if (exec == CBG_EXEC_PANEL) {
    const bool adaptive = !getenv("CBG_PIPELINE") && g->pr * g->pc > 1;
    return summa_panel(g, A, B, A_gncol, B_gnrow, sr, pipeline_cuts(g, B.n, n_min), nullptr, nullptr, &C, adaptive);
  }
  return summa_staged(g, A, B, A_gncol, B_gnrow, sr, algo, C);
}

// ---------------------------------------------------------------------------
// MemEfficientSpGEMM's phase count from memory (ParFriends.h:482-535, with
// EstPerProcessNnzSUMMA :1243-1341).  The reference estimates this rank's
// unmerged nnz(C) by a symbolic SUMMA (every tile broadcast once more) and
// divides the memory left after the inputs.  Here:
//  * flops of this rank's product C(prow, pcol) = sum over the inner index k
//    of nnz(A(:,k) in my grid row) * nnz(B(k,:) in my grid column), from the
//    column counts of A's tiles (allgathered along the grid row) and the row
//    counts of B's tiles (along the grid column): count vectors, not tiles;
//  * nnz(C) <= flops; the compression nnz/flops is measured by an exact
//    symbolic of a sample of the product (one rank: every 256th column of B, ~1/256
//    of a symbolic pass; a grid: every 8th row of the A block row times every
//    16th column of the B block column, gathered like the SUMMA's tiles) and the
//    estimate is flops x ratio x 1.1 -- only where the flops bound alone asks for
//    more than one phase on some rank;
//  * the C bytes a phase may take: CBG_PHASE_MEM_FRAC (0.6) of the memory left
//    after the tiles the SUMMA gathers -- perProcessMemory (GB, like the
//    reference) when given, else the device's free memory plus libcbg's pool
//    cache -- which leaves room for the symbolic bitmaps (<= 1/4 of the free
//    memory) and the per-column arrays;
//  * phases = ceil(12 B x nnz_est / budget), the maximum over the world (the
//    pieces are broadcast collectively), at most the narrowest B tile's width.
// A phase that still does not fit is split in column halves by multiply_to_fn.
// ---------------------------------------------------------------------------
PhasePlan& phase_plan() {
  static thread_local PhasePlan p;
  return p;
}

static double phase_mem_frac() {
  static const char* e = getenv("CBG_PHASE_MEM_FRAC");
  const double f = e ? atof(e) : 0.6;
  return f > 0 && f <= 1 ? f : 0.6;
}

static int plan_phases(cbg_grid* g, const cbg_tile& A, const cbg_tile& B, int64_t K, int64_t mem_gb, int64_t n_min,
                       int fallback, int& phases) {
  hipStream_t cs = g->compute;
  static const bool dbg = getenv("CBG_DEBUG_PLAN") != nullptr;
  const auto t_start = std::chrono::steady_clock::now();
  auto mark = [&](const char* what) {
    if (dbg)
      std::fprintf(stderr, "[cbg plan] %s at %.2f ms\n", what,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
  };
  const int pr = g->pr, pc = g->pc;
  // widths of A's tiles along my grid row and heights of B's along my grid column
  std::vector<int64_t> WA(pc), HB(pr);
  allgather_i64(g, COMM_ROW, &A.n, WA.data(), 1);
  allgather_i64(g, COMM_COL, &B.m, HB.data(), 1);
  int64_t wmax = 0, hmax = 0, sa = 0, sb = 0;
  for (auto w : WA) wmax = std::max(wmax, w), sa += w;
  for (auto h : HB) hmax = std::max(hmax, h), sb += h;
  int rc = agree(g, (sa != K || sb != K) ? CBG_ERR_DIMMISMATCH : CBG_OK);
  if (rc) return rc;
  int64_t flops = 0;
  if (g->nranks == 1) {
    // one rank: the flops straight from A's column counts and B's entries
    DBuf<int32_t> ca(std::max<int64_t>(A.n, 1));
    rc = agree(g, step([&] {
      tile_counts_device(A, 0, ca.p, A.n, cs);
      flops = entry_sum_device(B, ca.p, cs);
    }));
  } else {
    // the count vectors, padded to the widest tile, gathered on the device
    DBuf<int32_t> ca(std::max<int64_t>(wmax, 1)), rb(std::max<int64_t>(hmax, 1));
    DBuf<int32_t> CA(std::max<int64_t>(wmax * pc, 1)), RB(std::max<int64_t>(hmax * pr, 1));
    rc = agree(g, step([&] { tile_counts_device(A, 0, ca.p, wmax, cs), tile_counts_device(B, 1, rb.p, hmax, cs); }));
    if (rc) return rc;
    mark("counts");
    allgather_device(g, COMM_ROW, ca.p, CA.p, sizeof(int32_t) * wmax);
    allgather_device(g, COMM_COL, rb.p, RB.p, sizeof(int32_t) * hmax);
    mark("count allgathers");
    rc = agree(g, step([&] {
      std::vector<int64_t> aoff(pc + 1, 0), boff(pr + 1, 0);
      for (int s = 0; s < pc; ++s) aoff[s + 1] = aoff[s] + WA[s];
      for (int s = 0; s < pr; ++s) boff[s + 1] = boff[s] + HB[s];
      flops = blocked_dot_device(CA.p, wmax, aoff, RB.p, hmax, boff, K, cs);
    }));
  }
  if (rc) return rc;
  mark("flops");
  // compression nnz/flops of a sample of this rank's product: one rank: every
  // 256th column of B; a grid: every 8th row of the A block row
  // times every 16th column of the B block column, the samples broadcast like
  // the SUMMA's tiles (1/8 and 1/16 of their bytes); ids, not positions, so the
  // tiles of a grid row / column sample the same rows / columns
  // (skipped, agreed, where the flops bound alone leaves one phase on every rank)
  auto tbytes = [](const cbg_tile& t) { return (double)(8 * (t.nzc + 1) + 4 * t.nzc + 12 * t.nnz); };
  const double gathered = (pc - 1) * tbytes(A) + (pr - 1) * tbytes(B);
  double avail;
  if (mem_gb > 0) {
    avail = (double)mem_gb * 1e9 - tbytes(A) - tbytes(B) - gathered;
  } else {
    size_t fr = 0, tot = 0;
    CBG_HIP(hipMemGetInfo(&fr, &tot));
    avail = (double)fr + (double)pool().bytes_cached() - gathered;
  }
  const double budget = phase_mem_frac() * avail;
  int64_t need_sample = 0;
  if ((rc = agree_val(g, CBG_OK, flops > 0 && 12.0 * (double)flops > budget ? 1 : 0, nullptr, &need_sample)))
    return rc;
  double ratio = 1.0;
  if (need_sample) {
    const int cstride = g->nranks == 1 ? 256 : 16;
    const int rstride = g->nranks == 1 ? 1 : 8;
    TileGuard As, Bs;
    rc = agree(g, step([&] {
      if (rstride > 1) tile_sample_rows(A, rstride, As.t, cs);
      tile_sample_cols(B, cstride, Bs.t, cs);
    }));
    if (rc) return rc;
    const cbg_tile& Amine = rstride > 1 ? As.t : A;
    int64_t ea[4], eb[4];
    tile_ess(Amine, ea);
    tile_ess(Bs.t, eb);
    std::vector<int64_t> EA((size_t)4 * pc), EB((size_t)4 * pr);
    allgather_i64(g, COMM_ROW, ea, EA.data(), 4);
    allgather_i64(g, COMM_COL, eb, EB.data(), 4);
    std::vector<TileGuard> Ar(pc), Bc(pr);
    rc = agree(g, step([&] {
      for (int q = 0; q < pc; ++q)
        if (q != g->pcol) alloc_like(Ar[q].t, &EA[4 * q]);
      for (int q = 0; q < pr; ++q)
        if (q != g->prow) alloc_like(Bc[q].t, &EB[4 * q]);
    }));
    if (rc) return rc;
    int64_t fs = 0, zs = 0;
    rc = agree(g, step([&] {
      bcast_group(g, [&] {
        for (int q = 0; q < pc; ++q)
          bcast_tile(g, COMM_ROW, q, &EA[4 * q], q == g->pcol ? const_cast<cbg_tile&>(Amine) : Ar[q].t, q == g->pcol);
      });
      bcast_group(g, [&] {
        for (int q = 0; q < pr; ++q) bcast_tile(g, COMM_COL, q, &EB[4 * q], q == g->prow ? Bs.t : Bc[q].t, q == g->prow);
      });
      wait_comm(g);
      TileGuard Ap, Bp;
      const cbg_tile* Au = &Amine;
      const cbg_tile* Bu = &Bs.t;
      if (pc > 1) {
        std::vector<cbg_tile> parts(pc);
        std::vector<int64_t> off(pc, 0);
        for (int q = 0; q < pc; ++q) {
          parts[q] = q == g->pcol ? Amine : Ar[q].t;
          if (q) off[q] = off[q - 1] + WA[q - 1];
        }
        tile_concat_cols(parts, off, Amine.m, K, Ap.t, cs);
        Au = &Ap.t;
      }
      if (pr > 1) {
        std::vector<cbg_tile> parts(pr);
        std::vector<int64_t> off(pr, 0);
        for (int q = 0; q < pr; ++q) {
          parts[q] = q == g->prow ? Bs.t : Bc[q].t;
          if (q) off[q] = off[q - 1] + HB[q - 1];
        }
        tile_concat_rows(parts, off, K, B.n, Bp.t, cs);
        Bu = &Bp.t;
      }
      local_symbolic(*Au, *Bu, cs, &fs, &zs);
    }));
    if (rc) return rc;
    if (fs > 0) ratio = std::min(1.0, 1.1 * (double)zs / (double)fs);
    mark("sample symbolic");
  }
  const double need = 12.0 * ratio * (double)flops;
  int64_t want = budget > 0 ? (int64_t)std::ceil(need / budget) : fallback;  // the reference keeps the given phases
  want = std::max<int64_t>(1, std::min<int64_t>(want, std::max<int64_t>(1, n_min)));
  int64_t agreed = 0;
  if ((rc = agree_val(g, CBG_OK, want, nullptr, &agreed))) return rc;
  phases = (int)agreed;
  PhasePlan& pp = phase_plan();
  pp.automatic = 1;
  pp.flops = flops;
  pp.nnz_est = (int64_t)(ratio * (double)flops);
  pp.c_budget_bytes = budget;
  pp.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
  mark("planned");
  return CBG_OK;
}

// ---------------------------------------------------------------------------
// MemEfficientSpGEMM (ParFriends.h:449-730) minus its Markov-clustering pruning:
// B's local tile is cut into `phases` column pieces like SpDCCols::ColSplit
// (SpDCCols.cpp:936-970), each piece goes through the SUMMA, and the phase
// results are streamed to `fn` or column-concatenated (ColConcatenate,
// ParFriends.h:724-725).  Column pieces keep every C column's products inside
// one phase, so the result is identical to the unphased product.  PANEL: the
// phases are the pipeline's pieces (A's row panel is gathered once, phase
// p+1's B pieces are broadcast while phase p multiplies); STAGED: one staged
// SUMMA per phase.  phases <= 0 or mem_gb > 0: the count comes from
// plan_phases (perProcessMemory, ParFriends.h:482-535).
// ---------------------------------------------------------------------------
int summa_spgemm_phased(cbg_grid* g, const cbg_tile& A, const cbg_tile& B, int64_t A_gncol, int64_t B_gnrow, int sr,
                        int algo, int exec, int phases, int64_t mem_gb, cbg_phase_fn fn, void* user, cbg_tile* C) {
  check_usable(g);
  arm_fault(g);
  phase_plan() = PhasePlan{};
  summa_info() = SummaInfo{};
  // PANEL: every local multiply of this call (the plan's sample included on
  // one rank) multiplies the same A, so its column maps are built once.  Not
  // for STAGED, whose stages multiply different A slices.
  std::unique_ptr<APrepScope> aprep_scope;
  if (exec == CBG_EXEC_PANEL) aprep_scope.reset(new APrepScope());
  // phases == CBG_PHASES_AUTO or a memory budget: the count comes from memory;
  // otherwise phases < 1 or >= A_gncol is "Resetting to 1" (ParFriends.h:468-473)
  const bool automatic = phases == CBG_PHASES_AUTO || mem_gb > 0;
  if (!automatic && (phases < 1 || phases >= A_gncol)) phases = 1;
  int rc = A_gncol != B_gnrow ? CBG_ERR_DIMMISMATCH : CBG_OK;
  int64_t n_min = 0;
  if ((rc = agree_val(g, rc, B.n, &n_min, nullptr))) return rc;
  if (automatic && (rc = plan_phases(g, A, B, A_gncol, mem_gb, n_min, std::max(1, phases), phases))) return rc;
  phase_plan().phases = phases;
  if ((rc = agree(g, B.n < phases ? CBG_ERR_INVALIDPARAMS : CBG_OK))) return rc;  // ColSplit: "Matrix is too small to be splitted"
  hipStream_t cs = g->compute;
  const int64_t w = B.n / phases;
  std::vector<int64_t> cuts;
  for (int p = 0; p < phases; ++p) cuts.push_back((int64_t)p * w);
  cuts.push_back(B.n);
  if (exec == CBG_EXEC_PANEL) {
    // the reference copies B first, so A and B may alias here (ParFriends.h:547-549);
    // the copy is a step of every rank (a no-op where they do not alias), so
    // an empty tile on one rank cannot skip an agree() its peers make
    const bool alias = (&A == &B) || (A.ir == B.ir && A.nnz > 0);
    TileGuard Bcopy;
    rc = step([&] {
      if (alias) tile_slice_cols(B, 0, B.n, Bcopy.t, cs);
    });
    if ((rc = agree(g, rc))) return rc;
    const cbg_tile& Bu = alias ? Bcopy.t : B;
    if (phases == 1) {
      // one phase is Mult_AnXBn_DoubleBuff: B's block column arrives in the
      // (adaptive) pipeline's pieces, each handed to fn as phase 0 at its column offset
      const bool adaptive = !getenv("CBG_PIPELINE") && g->pr * g->pc > 1;
      return summa_panel(g, A, Bu, A_gncol, B_gnrow, sr, pipeline_cuts(g, Bu.n, n_min), fn, user, C, adaptive,
                         true);
    }
    return summa_panel(g, A, Bu, A_gncol, B_gnrow, sr, cuts, fn, user, C);
  }
  std::vector<TileGuard> parts;
  std::vector<cbg_tile> pv;
  int cb_rc = 0;
  for (int p = 0; p < phases; ++p) {
    TileGuard piece, Cp;
    rc = step([&] { tile_slice_cols(B, cuts[p], cuts[p + 1], piece.t, cs); });
    if ((rc = agree(g, rc))) return rc;
    rc = summa_staged(g, A, piece.t, A_gncol, B_gnrow, sr, algo, Cp.t);
    if (rc) return rc;
    if (fn) {
      rc = step([&] {
        CBG_HIP(hipStreamSynchronize(cs));
        const int r = fn(user, p, cuts[p], &Cp.t);
        if (r && !cb_rc) cb_rc = r;
      });
      if ((rc = agree(g, rc))) return rc;
    } else {
      pv.push_back(Cp.t);
      parts.push_back(std::move(Cp));
    }
  }
  if (fn) return agree(g, cb_rc ? CBG_ERR_INVALIDPARAMS : CBG_OK);
  rc = step([&] {
    if (pv.size() == 1) {
      *C = parts[0].release();
    } else {
      std::vector<int64_t> off(cuts.begin(), cuts.end() - 1);
      tile_concat_cols(pv, off, A.m, B.n, *C, cs);
    }
  });
  return agree(g, rc);
}

// ---------------------------------------------------------------------------
// SpParMat::Transpose (SpParMat.cpp:3528-3590) on a square grid: a diagonal
// rank transposes its tile; rank (r,c) transposes the tile of its complement
// (c,r) (GetComplementRank), received over RCCL send/recv (host transport:
// world broadcasts, test only).  `out` is this rank's tile of the transpose.
// ---------------------------------------------------------------------------
int grid_transpose(cbg_grid* g, const cbg_tile& T, cbg_tile& out) {
  check_usable(g);
  if (g->pr != g->pc) return CBG_ERR_NOTSQUARE;  // the grid's shape: the same answer on every rank
  hipStream_t cs = g->compute;
  const bool inject = redist_fault(g);
  // essentials of every rank's tile (world allgather: collective, diagonal ranks too)
  int64_t e[4] = {T.m, T.n, T.nnz, T.nzc};
  std::vector<int64_t> E((size_t)4 * g->nranks);
  allgather_i64(g, COMM_WORLD, e, E.data(), 4);
  const bool diag = g->prow == g->pcol;
  const int peer = g->pcol * g->pc + g->prow;
  const int64_t* pe = &E[4 * (size_t)peer];
  // every rank holds its receive buffer before anyone sends (agreed)
  TileGuard R;
  int rc = step([&] {
    if (inject) throw HipError("injected fault (CBG_FAULT_INJECT_REDIST) in Transpose", CBG_ERR_OOM);
    if (!diag) tile_alloc_device(R.t, pe[0], pe[1], pe[2], pe[3]);
  });
  if ((rc = agree(g, rc))) return rc;
  int local = step([&] {
    if (g->host_mode && g->nranks > 1) {
      // every off-diagonal rank broadcasts its tile over the world communicator
      for (int q = 0; q < g->nranks; ++q) {
        const int qr = q / g->pc, qc = q % g->pc;
        if (qr == qc) continue;
        const int64_t* qe = &E[4 * (size_t)q];
        const bool mine = q == g->rank, keep = !diag && q == peer;
        auto hb = [&](void* dst, const void* src, size_t bytes) {
          if (bytes == 0) return;
          std::vector<char> h(bytes);
          if (mine) CBG_HIP(hipMemcpy(h.data(), src, bytes, hipMemcpyDeviceToHost));
          host_check(g, g->hc.bcast(g->hc.user, COMM_WORLD, h.data(), bytes, q), "transpose bcast");
          if (keep) CBG_HIP(hipMemcpy(dst, h.data(), bytes, hipMemcpyHostToDevice));
        };
        hb(R.t.cp, T.cp, sizeof(int64_t) * (qe[3] + 1));
        hb(R.t.jc, T.jc, sizeof(int32_t) * qe[3]);
        hb(R.t.ir, T.ir, sizeof(int32_t) * qe[2]);
        hb(R.t.val, T.val, sizeof(double) * qe[2]);
      }
    } else if (!diag) {
      ncclComm_t c = g->world;
      CBG_NCCL(ncclGroupStart());
      CBG_NCCL(ncclSend(T.cp, T.nzc + 1, ncclInt64, peer, c, g->comm));
      CBG_NCCL(ncclRecv(R.t.cp, pe[3] + 1, ncclInt64, peer, c, g->comm));
      if (T.nzc) CBG_NCCL(ncclSend(T.jc, T.nzc, ncclInt32, peer, c, g->comm));
      if (pe[3]) CBG_NCCL(ncclRecv(R.t.jc, pe[3], ncclInt32, peer, c, g->comm));
      if (T.nnz) {
        CBG_NCCL(ncclSend(T.ir, T.nnz, ncclInt32, peer, c, g->comm));
        CBG_NCCL(ncclSend(T.val, T.nnz, ncclFloat64, peer, c, g->comm));
      }
      if (pe[2]) {
        CBG_NCCL(ncclRecv(R.t.ir, pe[2], ncclInt32, peer, c, g->comm));
        CBG_NCCL(ncclRecv(R.t.val, pe[2], ncclFloat64, peer, c, g->comm));
      }
      CBG_NCCL(ncclGroupEnd());
      wait_comm(g);
    }
  });
  // the local transpose (SpDCCols::Transpose) only where the exchange worked
  TileGuard O;
  if (!local) local = step([&] { tile_transpose(diag ? T : R.t, O.t, cs); });
  if ((rc = agree(g, local))) return rc;
  out = O.release();
  return CBG_OK;
}

// ---------------------------------------------------------------------------
// SpParMat::BlockSplit (SpParMat.cpp:2974-3058) for the splits BlockSpGEMM
// uses (bi = 1, BlockSpGEMM.h:39-45): global rows [lo, hi) of a distributed
// matrix (dim 0) or columns [lo, hi) (dim 1) as a distributed matrix of its
// own on the same grid, in the standard block layout (Owner,
// SpParMat.cpp:5068-5097).  Rows only move inside a grid column (columns
// inside a grid row): every rank broadcasts its slice of the range to its
// column (row) communicator and keeps the part of each slice that falls in
// its new block.  Collective steps agree on a code like the SUMMA's: a rank
// that cannot allocate a receive buffer makes every rank return the code
// before any of them posts the broadcast it would have skipped.
// ---------------------------------------------------------------------------
int grid_block_extract(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, int dim, int64_t lo, int64_t hi,
                       cbg_tile& out) {
  check_usable(g);
  if (dim != 0 && dim != 1) return CBG_ERR_INVALIDPARAMS;
  const int64_t gext = dim == 0 ? gm : gn;
  if (lo < 0 || hi < lo || hi > gext) return CBG_ERR_INVALIDPARAMS;
  hipStream_t cs = g->compute;
  const bool inject = redist_fault(g);
  const int which = dim == 0 ? COMM_COL : COMM_ROW;
  const int np = comm_size(g, which), me = comm_rank(g, which);
  // my old range [S0, S1) along dim and my new range [lo + T0, lo + T1)
  auto span = [](int64_t ext, int np_, int i, int64_t& a, int64_t& b) {
    const int64_t per = ext / np_;
    a = (int64_t)i * per;
    b = i == np_ - 1 ? ext : a + per;
  };
  int64_t S0, S1, T0, T1;
  span(gext, np, me, S0, S1);
  span(hi - lo, np, me, T0, T1);
  T0 += lo;
  T1 += lo;
  auto cut = [&](const cbg_tile& X, int64_t a, int64_t b, cbg_tile& piece) {  // local range [a, b) of X
    if (dim == 0)
      tile_slice_rows(X, a, b, piece, cs);
    else
      tile_slice_cols(X, a, b, piece, cs);
  };
  // my slice of [lo, hi)
  const int64_t x0 = std::max(S0, lo), x1 = std::max(x0, std::min(S1, hi));
  TileGuard mine;
  int rc = step([&] { cut(T, x0 - S0, x1 - S0, mine.t); });
  int64_t e[4] = {mine.t.m, mine.t.n, mine.t.nnz, mine.t.nzc};
  if (rc) e[0] = e[1] = e[2] = e[3] = 0;
  if ((rc = agree(g, rc))) return rc;
  std::vector<int64_t> E((size_t)4 * np);
  allgather_i64(g, which, e, E.data(), 4);
  std::vector<TileGuard> parts;
  std::vector<int64_t> offs;
  int local = CBG_OK;
  for (int q = 0; q < np; ++q) {
    int64_t Q0, Q1;
    span(gext, np, q, Q0, Q1);
    const int64_t y0 = std::max(Q0, lo), y1 = std::max(y0, std::min(Q1, hi));  // slice of rank q
    TileGuard recv;
    rc = step([&] {
      if (inject && q == (me + 1) % np) throw HipError("injected fault (CBG_FAULT_INJECT_REDIST) in BlockSplit", CBG_ERR_OOM);
      if (q != me) alloc_like(recv.t, &E[4 * (size_t)q]);
    });
    if ((rc = agree(g, rc))) return rc;  // every receive buffer of this broadcast exists
    cbg_tile& sl = q == me ? mine.t : recv.t;
    local = std::max(local, step([&] {
      bcast_group(g, [&] { bcast_tile(g, which, q, &E[4 * (size_t)q], sl, q == me); });
      wait_comm(g);
    }));
    const int64_t z0 = std::max(y0, T0), z1 = std::min(y1, T1);  // the part of it in my new range
    if (!local && z1 > z0)
      local = step([&] {
        TileGuard piece;
        cut(sl, z0 - y0, z1 - y0, piece.t);
        parts.push_back(std::move(piece));
        offs.push_back(z0 - T0);
      });
  }
  mine = TileGuard();
  const int64_t om = dim == 0 ? T1 - T0 : T.m, on = dim == 0 ? T.n : T1 - T0;
  TileGuard O;
  if (!local)
    local = step([&] {
      std::vector<cbg_tile> pv;
      for (auto& t : parts) pv.push_back(t.t);
      if (pv.empty()) {
        tile_alloc_device(O.t, om, on, 0, 0);
      } else if (dim == 0) {
        tile_concat_rows(pv, offs, om, on, O.t, cs);
      } else {
        tile_concat_cols(pv, offs, om, on, O.t, cs);
      }
      CBG_HIP(hipStreamSynchronize(cs));
    });
  if ((rc = agree(g, local))) return rc;
  out = O.release();
  return CBG_OK;
}

// ---------------------------------------------------------------------------
// Markov-clustering pruning (MCLPruneRecoverySelect, ParFriends.h:186-353; the
// kernels and the per-piece logic are in cbg_prune.hip).  All of its
// collectives run along the grid column; the world only agrees on the result.
// ---------------------------------------------------------------------------
static ColComm col_comm(cbg_grid* g) {
  ColComm cc;
  cc.P = g->pr;
  cc.agree_vals = [g](int rc, const int64_t* vals, int n, int64_t* all) {
    const int P = g->pr;
    if (P == 1) {
      for (int i = 0; i < n; ++i) all[i] = vals[i];
      return rc;
    }
    std::vector<int64_t> in((size_t)n + 1), out((size_t)P * (n + 1));
    in[0] = rc;
    for (int i = 0; i < n; ++i) in[i + 1] = vals[i];
    allgather_i64(g, COMM_COL, in.data(), out.data(), n + 1);
    int64_t w = 0;
    for (int r = 0; r < P; ++r) {
      w = std::max(w, out[(size_t)r * (n + 1)]);
      for (int i = 0; i < n; ++i) all[(size_t)r * n + i] = out[(size_t)r * (n + 1) + 1 + i];
    }
    return (int)w;
  };
  cc.allgather_dev = [g](const void* in, void* out, size_t bytes) { allgather_device(g, COMM_COL, in, out, bytes); };
  return cc;
}

int grid_mcl_prune(cbg_grid* g, const cbg_tile& T, const cbg_mcl_params* p, cbg_tile& out) {
  check_usable(g);
  hipStream_t cs = g->compute;
  int rc = CBG_OK;
  const int local = step([&] {
    if (!p) {
      tile_slice_cols(T, 0, T.n, out, cs);
      CBG_HIP(hipStreamSynchronize(cs));
    } else {
      rc = mcl_prune_piece(col_comm(g), T, *p, out, cs);
    }
  });
  return agree(g, std::max(local, rc));
}

int grid_kselect(cbg_grid* g, const cbg_tile& T, const int32_t* cols, int64_t ncols, int64_t k, double* kth) {
  check_usable(g);
  int rc = CBG_OK;
  const int local = step([&] { rc = grid_kselect_cols(col_comm(g), T, cols, ncols, k, kth, g->compute); });
  return agree(g, std::max(local, rc));
}

// The phased driver's consumer for the pruned product.  Pruning is per column,
// so any column piece can be pruned on its own -- if the ranks of a grid column
// prune the same columns at the same time.  Their B tiles have the same width,
// so the phase cuts and the pipeline's cuts (functions of that width, the
// world's narrowest tile and the environment; the adaptive decision is agreed
// over the world) are the same; only the out-of-memory split of
// multiply_to_fn is a rank's own decision.  So the ranks of a column first
// allgather the width they hold and prune the narrowest (halves nest, every
// rank reaches the end of the delivered piece at the same column), slicing
// their piece where a peer holds a half.
struct MclPhase {
  cbg_grid* g;
  cbg_mcl_params p;
  cbg_phase_fn fn;
  void* user;
  ColComm cc;
  std::vector<TileGuard> parts;
  std::vector<int64_t> offs;
  int rc = 0;     // a pruning failure, agreed along the grid column: no collective after it
  int cb_rc = 0;  // the caller's fn failed
};
static int mcl_phase_fn(void* user, int phase, int64_t off, const cbg_tile* Cp) {
  MclPhase& c = *static_cast<MclPhase*>(user);
  if (c.rc) return c.rc;
  hipStream_t cs = c.g->compute;
  for (int64_t done = 0; done < Cp->n || (Cp->n == 0 && done == 0);) {
    int64_t w = Cp->n - done;
    if (c.cc.P > 1) {
      std::vector<int64_t> all(c.cc.P);
      if ((c.rc = c.cc.agree_vals(CBG_OK, &w, 1, all.data()))) return c.rc;
      w = *std::min_element(all.begin(), all.end());
    }
    TileGuard slice, pruned;
    int pend = CBG_OK;
    const bool whole = done == 0 && w == Cp->n;
    if (!whole) pend = step([&] { tile_slice_cols(*Cp, done, done + w, slice.t, cs); });
    if (pend && c.cc.P == 1) return c.rc = pend;
    int rc = CBG_OK;
    const int local = step([&] { rc = mcl_prune_piece(c.cc, whole ? *Cp : slice.t, c.p, pruned.t, cs, pend); });
    if ((c.rc = std::max(local, rc))) return c.rc;
    if (c.fn) {
      const int r = c.fn(c.user, phase, off + done, &pruned.t);
      if (r && !c.cb_rc) c.cb_rc = r;
    } else {
      c.offs.push_back(off + done);
      c.parts.push_back(std::move(pruned));
    }
    done += std::max<int64_t>(w, 1);
  }
  return CBG_OK;
}

int summa_spgemm_mcl(cbg_grid* g, const cbg_tile& A, const cbg_tile& B, int64_t A_gncol, int64_t B_gnrow, int sr,
                     int algo, int exec, int phases, int64_t mem_gb, cbg_phase_fn fn, void* user, cbg_tile* C,
                     const cbg_mcl_params& p) {
  MclPhase c{g, p, fn, user, col_comm(g)};
  int rc = summa_spgemm_phased(g, A, B, A_gncol, B_gnrow, sr, algo, exec, phases, mem_gb, mcl_phase_fn, &c, nullptr);
  // the driver reports a consumer's failure as INVALIDPARAMS: the pruning's own code instead
  if (rc == CBG_OK || rc == CBG_ERR_INVALIDPARAMS) {
    const int mine = c.rc ? c.rc : c.cb_rc ? (int)CBG_ERR_INVALIDPARAMS : (int)CBG_OK;
    const int a = agree(g, mine);
    if (a) return a;
  }
  if (rc || fn) return rc;
  rc = step([&] {
    if (c.parts.size() == 1 && c.parts[0].t.n == B.n) {
      *C = c.parts[0].release();
    } else {
      std::vector<cbg_tile> pv;
      for (auto& t : c.parts) pv.push_back(t.t);
      tile_concat_cols(pv, c.offs, A.m, B.n, *C, g->compute);
      CBG_HIP(hipStreamSynchronize(g->compute));
    }
  });
  return agree(g, rc);
}

// ---------------------------------------------------------------------------
// The HipMCL iteration (Applications/MCL.cpp:515-647; kernels and the
// grid-column logic in cbg_mcl.hip).  Column reductions are collective along
// the grid column; the world agrees on every step's code.
// ---------------------------------------------------------------------------
int grid_reduce_cols(cbg_grid* g, const cbg_tile& T, int what, double identity, double* out) {
  check_usable(g);
  int rc = CBG_OK;
  const int local = step([&] { rc = grid_reduce_cols_device(col_comm(g), T, what, identity, out, g->compute); });
  return agree(g, std::max(local, rc));
}

int grid_make_col_stochastic(cbg_grid* g, cbg_tile& T) {
  check_usable(g);
  int rc = CBG_OK;
  const int local = step([&] { rc = grid_make_col_stochastic_device(col_comm(g), T, g->compute); });
  return agree(g, std::max(local, rc));
}

// the grid column's chaos -> the world's
static int world_chaos(cbg_grid* g, int rc, double* chaos) {
  if ((rc = agree(g, rc))) return rc;
  return agree(g, step([&] { allreduce_f64(g, chaos, true); }));
}

int grid_chaos(cbg_grid* g, const cbg_tile& T, double* chaos) {
  check_usable(g);
  int rc = CBG_OK;
  const int local = step([&] { rc = grid_chaos_device(col_comm(g), T, chaos, g->compute); });
  return world_chaos(g, std::max(local, rc), chaos);
}

int grid_inflate(cbg_grid* g, cbg_tile& T, double power, double* chaos) {
  check_usable(g);
  int rc = CBG_OK;
  HipMclStats& hs = hipmcl_stats();
  hs.inflate_nnz = T.nnz;
  const int local = step([&] { rc = grid_inflate_device(col_comm(g), T, power, chaos, g->compute, hs.inflate_ms); });
  return world_chaos(g, std::max(local, rc), chaos);
}

// the tile's offsets in the gm x gn matrix (SpParMat::Owner, SpParMat.cpp:5068-5097: blocks of
// ext / np, the last one longer), or false when the tile's shape is not that block's
static bool tile_place(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, int64_t* roff, int64_t* coff) {
  *roff = (int64_t)g->prow * (gm / g->pr);
  *coff = (int64_t)g->pcol * (gn / g->pc);
  const int64_t m = g->prow == g->pr - 1 ? gm - *roff : gm / g->pr;
  const int64_t n = g->pcol == g->pc - 1 ? gn - *coff : gn / g->pc;
  return T.m == m && T.n == n;
}

// mode 0: RemoveLoops, 1: AddLoops (fix_min: as AdjustLoops calls it)
static int grid_edit_loops(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, int mode, int replace, int fix_min,
                           const double* loopvals, cbg_tile& out, int64_t* found) {
  check_usable(g);
  int64_t roff = 0, coff = 0;
  int rc = gm != gn || !tile_place(g, T, gm, gn, &roff, &coff) ? CBG_ERR_DIMMISMATCH : CBG_OK;
  if ((rc = agree(g, rc))) return rc;
  hipStream_t cs = g->compute;
  TileGuard o;
  int64_t nf = 0;
  rc = step([&] {
    DBuf<double> lv;
    if (mode == 1) {
      lv.reset(std::max<int64_t>(T.n, 1));
      if (T.n) CBG_HIP(hipMemcpyAsync(lv.p, loopvals, sizeof(double) * T.n, hipMemcpyHostToDevice, cs));
    }
    tile_edit_loops_device(T, coff - roff, mode, replace, fix_min, lv.p, o.t, &nf, cs);
    CBG_HIP(hipStreamSynchronize(cs));
  });
  if ((rc = agree(g, rc))) return rc;
  if (found) {
    if ((rc = agree(g, step([&] { allreduce_sum_i64(g, &nf); })))) return rc;
    *found = nf;
  }
  out = o.release();
  return CBG_OK;
}

int grid_remove_loops(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, cbg_tile& out, int64_t* removed) {
  return grid_edit_loops(g, T, gm, gn, 0, 0, 0, nullptr, out, removed);
}
int grid_add_loops(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, const double* loopvals, int replace,
                   cbg_tile& out) {
  return grid_edit_loops(g, T, gm, gn, 1, replace, 0, loopvals, out, nullptr);
}
int grid_adjust_loops(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, cbg_tile& out) {
  TileGuard noloops;
  int rc = grid_edit_loops(g, T, gm, gn, 0, 0, 0, nullptr, noloops.t, nullptr);
  if (rc) return rc;
  std::vector<double> colmax;
  rc = agree(g, step([&] { colmax.resize((size_t)std::max<int64_t>(T.n, 1)); }));
  if (rc) return rc;
  if ((rc = grid_reduce_cols(g, noloops.t, CBG_RED_MAX, std::numeric_limits<double>::min(), colmax.data()))) return rc;
  return grid_edit_loops(g, noloops.t, gm, gn, 1, 0, 1, colmax.data(), out, nullptr);
}

// Interpret's connected components: see include/cbg.h.  At the start of a round every
// rank holds the same labels; a round hooks over the rank's entries, jumps, and takes
// the minimum over the world.  A round in which no rank lowered a label ends the loop.
int grid_connected_components(cbg_grid* g, const cbg_tile& T, int64_t gn, int64_t* labels, int64_t* ncomp) {
  check_usable(g);
  int64_t roff = 0, coff = 0;
  int rc = gn < 0 || !tile_place(g, T, gn, gn, &roff, &coff) ? CBG_ERR_DIMMISMATCH : CBG_OK;
  if ((rc = agree(g, rc))) return rc;
  hipStream_t cs = g->compute;
  const int P = g->nranks;
  const int64_t n1 = std::max<int64_t>(gn, 1);
  DBuf<uint64_t> L, all, changed;
  rc = step([&] {
    L.reset(n1);
    changed.reset(1);
    if (P > 1) all.reset(g->host_mode ? (size_t)n1 * P : (size_t)n1);
    cc_init_device(L.p, gn, cs);
    CBG_HIP(hipStreamSynchronize(cs));
  });
  if ((rc = agree(g, rc))) return rc;
  for (int64_t round = 0;; ++round) {
    uint64_t ch = 0;
    rc = round > gn ? (int)CBG_ERR_NOTSUPPORTED : step([&] {
      CBG_HIP(hipMemsetAsync(changed.p, 0, sizeof(uint64_t), cs));
      cc_round_device(T, roff, coff, L.p, gn, changed.p, cs);
      CBG_HIP(hipStreamSynchronize(cs));
      if (P > 1 && gn > 0) {
        if (g->host_mode) {
          allgather_device(g, COMM_WORLD, L.p, all.p, sizeof(uint64_t) * gn);
          cc_min_device(L.p, all.p, P, gn, changed.p, cs);
        } else {
          CBG_HIP(hipMemcpyAsync(all.p, L.p, sizeof(uint64_t) * gn, hipMemcpyDeviceToDevice, g->comm));
          CBG_NCCL(ncclAllReduce(all.p, all.p, (size_t)gn, ncclUint64, ncclMin, g->world, g->comm));
          wait_comm(g);
          cc_min_device(L.p, all.p, 1, gn, changed.p, cs);
        }
      }
      CBG_HIP(hipMemcpyAsync(&ch, changed.p, sizeof(uint64_t), hipMemcpyDeviceToHost, cs));
      CBG_HIP(hipStreamSynchronize(cs));
    });
    int64_t any = 0;
    if ((rc = agree_val(g, rc, ch ? 1 : 0, nullptr, &any))) return rc;
    if (!any) break;
  }
  // canonical labels: the rank of the component's smallest vertex among the smallest vertices
  int64_t nc = 0;
  rc = step([&] {
    std::vector<uint64_t> h((size_t)n1);
    std::vector<int64_t> rank_of((size_t)n1);
    if (gn > 0) CBG_HIP(hipMemcpy(h.data(), L.p, sizeof(uint64_t) * gn, hipMemcpyDeviceToHost));
    for (int64_t v = 0; v < gn; ++v)
      if (h[v] == (uint64_t)v) rank_of[v] = nc++;
    for (int64_t v = 0; labels && v < gn; ++v) labels[v] = rank_of[h[v]];
  });
  if ((rc = agree(g, rc))) return rc;
  if (ncomp) *ncomp = nc;
  return CBG_OK;
}

int grid_hipmcl(cbg_grid* g, const cbg_tile& A, int64_t gn, const cbg_hipmcl_params& P, cbg_hipmcl_iter_fn fn,
                void* user, cbg_tile* final_local, int64_t* labels, int64_t* nclusters, int64_t* iterations) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  HipMclStats& hs = hipmcl_stats();
  hs = HipMclStats{};
  hipStream_t cs = g->compute;
  const double eps = P.eps > 0 ? P.eps : 1e-4;
  const cbg_mcl_params& pp = P.prune;
  const bool pruning = pp.hard_threshold > 0 || pp.select_num > 0 || pp.recover_num > 0 || pp.recover_pct > 0;
  TileGuard cur;
  int rc = grid_adjust_loops(g, A, gn, gn, cur.t);
  if (rc) return rc;
  if ((rc = grid_make_col_stochastic(g, cur.t))) return rc;
  int64_t nnz = cur.t.nnz;
  if ((rc = agree(g, step([&] { allreduce_sum_i64(g, &nnz); })))) return rc;
  bool pre = P.preprune > 0;
  if (P.preprune < 0) pre = gn > 0 && nnz / gn > std::max(pp.select_num, pp.recover_num);  // MCL.cpp:531-538
  if (pre && pruning) {
    TileGuard pruned;
    if ((rc = grid_mcl_prune(g, cur.t, &pp, pruned.t))) return rc;
    cur = std::move(pruned);
  }
  double chaos = 1.0;
  int64_t it = 0;
  while (chaos > eps && (P.max_iterations == 0 || it < P.max_iterations)) {
    // the squaring multiplies A by a copy: the SUMMA refuses aliased operands
    TileGuard B, C;
    if ((rc = agree(g, step([&] {
           tile_slice_cols(cur.t, 0, cur.t.n, B.t, cs);
           CBG_HIP(hipStreamSynchronize(cs));
         }))))
      return rc;
    double prune0 = 0;
    for (double x : mcl_stats().ms) prune0 += x;
    const auto t0 = clk::now();
    rc = pruning ? summa_spgemm_mcl(g, cur.t, B.t, gn, gn, CBG_PLUS_TIMES, P.algo, P.exec, P.phases,
                                    P.per_process_memory_gb, nullptr, nullptr, &C.t, pp)
                 : summa_spgemm_phased(g, cur.t, B.t, gn, gn, CBG_PLUS_TIMES, P.algo, P.exec, P.phases,
                                       P.per_process_memory_gb, nullptr, nullptr, &C.t);
    if (rc) return rc;
    const double ms_expand = ms_since(t0);
    double ms_prune = -prune0;
    for (double x : mcl_stats().ms) ms_prune += x;
    B = TileGuard();
    cur = std::move(C);
    const auto t1 = clk::now();
    if ((rc = grid_inflate(g, cur.t, P.inflation, &chaos))) return rc;
    const double ms_inflate = ms_since(t1);
    nnz = cur.t.nnz;
    if ((rc = agree(g, step([&] { allreduce_sum_i64(g, &nnz); })))) return rc;
    ++it;
    hs.iterations = it;
    hs.chaos = chaos;
    hs.final_nnz = nnz;
    hs.ms_expand += ms_expand;
    hs.ms_prune += ms_prune;
    hs.ms_inflate += ms_inflate;
    if (fn) fn(user, it, chaos, nnz, ms_expand, ms_prune, ms_inflate);
  }
  hs.final_nnz = nnz;
  hs.chaos = chaos;
  if (iterations) *iterations = it;
  if (labels || nclusters)
    if ((rc = grid_connected_components(g, cur.t, gn, labels, nclusters))) return rc;
  if (final_local) *final_local = cur.release();
  return CBG_OK;
}

// ---------------------------------------------------------------------------
// SpParMat::SubsRef_SR (SpParMat.cpp:2026-2247): B(i, j) = A(ri[i], ci[j]) of a
// distributed matrix (kernels in cbg_spref.hip).  The reference multiplies by
// two selection matrices; here the entries move.  Columns first, along the grid
// row: whole stored columns are copied, nothing is sorted, and an indexing that
// shrinks the matrix shrinks it before the row stage, which touches every entry
// and sorts.  Every rank broadcasts its tile to its grid row; the receiver
// copies the columns it asked that rank for straight to their final place (the
// lengths come from an allgather of the column counts, so one tile is held at a
// time).  Then the rows, along the grid column: every rank broadcasts its
// column-stage tile, the receiver expands it through the inverse of its slice
// of ri, the parts are concatenated per column and the columns sorted (not when
// the slice of ri is strictly increasing: the parts' row ranges ascend).  The
// column-stage tile is freed before the concatenation: the peak is the gathered
// block column plus the output.  Agreements as in grid_block_extract.
// ---------------------------------------------------------------------------
static void block_span(int64_t ext, int np, int i, int64_t& a, int64_t& b) {
  const int64_t per = ext / np;
  a = (int64_t)i * per;
  b = i == np - 1 ? ext : a + per;
}

int grid_spref(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, const int64_t* ri, int64_t nri,
               const int64_t* ci, int64_t nci, cbg_tile& out) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  check_usable(g);
  hipStream_t cs = g->compute;
  SprefStats& st = spref_stats();
  // the indices themselves were checked by the caller (cbg_grid_spref; RemoveIsolated and RandPermute build valid ones)
  int64_t roff = 0, coff = 0;
  int rc = CBG_OK;
  auto bad = [&](const char* why) {
    if (step_error().empty()) step_error() = why;
    return (int)CBG_ERR_INVALIDPARAMS;
  };
  if (gm < 0 || gn < 0 || !tile_place(g, T, gm, gn, &roff, &coff)) rc = bad("gm x gn does not fit the tile's place in the grid");
  if (!rc && ((ri && nri < 0) || (ci && nci < 0))) rc = bad("a negative index count");
  const int64_t new_m = ri ? nri : gm, new_n = ci ? nci : gn;
  int64_t U0 = 0, U1 = 0, V0 = 0, V1 = 0;
  if (!rc) {
    block_span(new_m, g->pr, g->prow, U0, U1);
    block_span(new_n, g->pc, g->pcol, V0, V1);
    // the last blocks are the longest
    if (new_m - (int64_t)(g->pr - 1) * (new_m / g->pr) >= INT32_MAX || new_n - (int64_t)(g->pc - 1) * (new_n / g->pc) >= INT32_MAX) {
      if (step_error().empty()) step_error() = "a new local block has 2^31 or more rows or columns";
      rc = CBG_ERR_NOTSUPPORTED;
    }
  }
  if ((rc = agree(g, rc))) return rc;
  const bool inject = redist_fault(g);
  st.counts[CBG_SPREF_ENTRIES_IN] += T.nnz;

  // ---- column stage: X = A(:, ci[V0:V1)) restricted to this rank's old row block
  TileGuard X;
  const cbg_tile* src = &T;
  if (ci) {
    const auto t0 = clk::now();
    const int np = g->pc, me = g->pcol;
    const int64_t per = gn / np, maxn = gn - (int64_t)(np - 1) * per, nsel = V1 - V0;
    DBuf<int64_t> sel, len, ocp;
    DBuf<int32_t> mycnt, allcnt, oir;
    DBuf<double> oval;
    int64_t nnzX = 0;
    rc = step([&] {
      sel.reset(std::max<int64_t>(nsel, 1));
      len.reset(nsel + 1);
      ocp.reset(nsel + 1);
      mycnt.reset(std::max<int64_t>(maxn, 1));
      allcnt.reset(std::max<int64_t>(maxn, 1) * np);
      if (nsel) CBG_HIP(hipMemcpyAsync(sel.p, ci + V0, sizeof(int64_t) * nsel, hipMemcpyHostToDevice, cs));
      tile_counts_device(T, 0, mycnt.p, maxn, cs);
    });
    if ((rc = agree(g, rc))) return rc;
    rc = step([&] {
      // one rank in the grid row: its own counts (allgather_device would copy them on the null stream,
      // which the compute stream does not wait for)
      if (np > 1) allgather_device(g, COMM_ROW, mycnt.p, allcnt.p, sizeof(int32_t) * maxn);
      spref_sel_lengths(sel.p, nsel, np > 1 ? allcnt.p : mycnt.p, maxn, per, np, len.p, cs);
      exclusive_scan_i64(len.p, ocp.p, nsel, cs);
      CBG_HIP(hipMemcpyAsync(&nnzX, ocp.p + nsel, sizeof(int64_t), hipMemcpyDeviceToHost, cs));
      CBG_HIP(hipStreamSynchronize(cs));
      oir.reset(std::max<int64_t>(nnzX, 1));
      oval.reset(std::max<int64_t>(nnzX, 1));
    });
    if ((rc = agree(g, rc))) return rc;
    int64_t e[4];
    tile_ess(T, e);
    std::vector<int64_t> E((size_t)4 * np);
    allgather_i64(g, COMM_ROW, e, E.data(), 4);
    int local = CBG_OK;
    for (int q = 0; q < np; ++q) {
      TileGuard recv;
      rc = step([&] {
        if (inject && q == (me + 1) % np) throw HipError("injected fault (CBG_FAULT_INJECT_REDIST) in SubsRef", CBG_ERR_OOM);
        if (q != me) alloc_like(recv.t, &E[4 * (size_t)q]);
      });
      if ((rc = agree(g, rc))) return rc;  // every receive buffer of this broadcast exists
      cbg_tile bt = T;                     // the root's own tile (bcast_tile does not write it)
      cbg_tile& sl = q == me ? bt : recv.t;
      if (q != me) st.counts[CBG_SPREF_BYTES_RECV] += tile_bytes(&E[4 * (size_t)q]);
      local = std::max(local, step([&] {
        bcast_group(g, [&] { bcast_tile(g, COMM_ROW, q, &E[4 * (size_t)q], sl, q == me); });
        wait_comm(g);
      }));
      if (!local) local = step([&] { spref_sel_copy(sl, q, per, np, sel.p, nsel, ocp.p, oir.p, oval.p, cs); });
    }
    if (!local)
      local = step([&] {
        spref_compact(T.m, nsel, nullptr, nsel, ocp.p, oir, oval, nnzX, X.t, cs);
        CBG_HIP(hipGetLastError());
      });
    if ((rc = agree(g, local))) return rc;
    src = &X.t;
    st.ms[CBG_SPREF_MS_COL] += ms_since(t0);
  }

  // ---- row stage: out = X(ri[U0:U1), :) over the grid column's row blocks
  TileGuard O;
  if (ri) {
    const auto t0 = clk::now();
    const int np = g->pr, me = g->prow;
    const int64_t per = gm / np, nloc = U1 - U0, ncols = src->n;
    const bool monotone = spref_strictly_increasing(ri + U0, nloc);
    RowInverse inv;
    rc = step([&] { spref_build_inverse(ri + U0, nloc, gm, inv, cs); });
    if ((rc = agree(g, rc))) return rc;
    int64_t e[4];
    tile_ess(*src, e);
    std::vector<int64_t> E((size_t)4 * np);
    allgather_i64(g, COMM_COL, e, E.data(), 4);
    std::vector<TileGuard> parts;
    int local = CBG_OK;
    for (int q = 0; q < np; ++q) {
      TileGuard recv;
      rc = step([&] {
        if (inject && !ci && q == (me + 1) % np) throw HipError("injected fault (CBG_FAULT_INJECT_REDIST) in SubsRef", CBG_ERR_OOM);
        if (q != me) alloc_like(recv.t, &E[4 * (size_t)q]);
      });
      if ((rc = agree(g, rc))) return rc;
      cbg_tile bt = *src;
      cbg_tile& sl = q == me ? bt : recv.t;
      if (q != me) st.counts[CBG_SPREF_BYTES_RECV] += tile_bytes(&E[4 * (size_t)q]);
      local = std::max(local, step([&] {
        bcast_group(g, [&] { bcast_tile(g, COMM_COL, q, &E[4 * (size_t)q], sl, q == me); });
        wait_comm(g);
      }));
      if (!local)
        local = step([&] {
          TileGuard piece;
          spref_expand_rows(sl, (int64_t)q * per, inv, nloc, piece.t, cs);
          parts.push_back(std::move(piece));
        });
    }
    X = TileGuard();  // the gathered block column goes before the output is built
    if (!local)
      local = step([&] {
        int64_t total = 0;
        for (auto& t : parts) total += t.t.nnz;
        if (parts.size() == 1) {
          O = std::move(parts[0]);
        } else if (total == 0) {  // also a block of no columns, which tile_concat_rows has no launch for
          tile_alloc_device(O.t, nloc, ncols, 0, 0);
        } else {
          std::vector<cbg_tile> pv;
          for (auto& t : parts) pv.push_back(t.t);
          tile_concat_rows(pv, std::vector<int64_t>(pv.size(), 0), nloc, ncols, O.t, cs);
        }
        parts.clear();
        st.ms[CBG_SPREF_MS_ROW] += ms_since(t0);
        if (monotone)
          st.counts[CBG_SPREF_COLS_MONOTONE] += O.t.nzc;
        else
          spref_sort_columns(O.t, cs);
        CBG_HIP(hipStreamSynchronize(cs));
        CBG_HIP(hipGetLastError());  // a refused launch is this call's failure, not a later one's
      });
    if ((rc = agree(g, local))) return rc;
  } else if (ci) {
    O = std::move(X);
  } else {
    rc = step([&] {
      tile_slice_cols(T, 0, T.n, O.t, cs);
      CBG_HIP(hipStreamSynchronize(cs));
    });
    if ((rc = agree(g, rc))) return rc;
  }
  st.counts[CBG_SPREF_ENTRIES_OUT] += O.t.nnz;
  out = O.release();
  return CBG_OK;
}

// this library's RandPerm: see include/cbg.h
static uint64_t mix64_host(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
void rand_perm(int64_t n, uint64_t seed, int64_t* p) {
  std::vector<uint64_t> key((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    key[i] = mix64_host(seed ^ ((uint64_t)i * 0x9E3779B97F4A7C15ULL));
    p[i] = i;
  }
  std::stable_sort(p, p + n, [&](int64_t a, int64_t b) { return key[a] < key[b]; });
}

// nonisov of RemoveIsolated (MCL.cpp:476-486): the column sums are the same bits on every rank of
// a grid column; the slices of a grid row, in rank order, are the global list
int grid_nonisolated(cbg_grid* g, const cbg_tile& A, int64_t gn, std::vector<int64_t>& ids) {
  check_usable(g);
  int64_t roff = 0, coff = 0;
  int rc = !tile_place(g, A, gn, gn, &roff, &coff) ? CBG_ERR_DIMMISMATCH : CBG_OK;
  if ((rc = agree(g, rc))) return rc;
  std::vector<double> colsum;
  rc = step([&] { colsum.resize((size_t)std::max<int64_t>(A.n, 1)); });
  if ((rc = agree(g, rc))) return rc;
  if ((rc = grid_reduce_cols(g, A, CBG_RED_SUM, 0.0, colsum.data()))) return rc;
  const int np = g->pc;
  std::vector<int64_t> mine, cnts((size_t)np), all;
  int64_t most = 1;
  rc = step([&] {
    for (int64_t j = 0; j < A.n; ++j)
      if (colsum[j] > 0) mine.push_back(coff + j);
  });
  if ((rc = agree(g, rc))) return rc;
  int64_t cnt = (int64_t)mine.size();
  allgather_i64(g, COMM_ROW, &cnt, cnts.data(), 1);
  most = std::max<int64_t>(1, *std::max_element(cnts.begin(), cnts.end()));
  rc = step([&] {
    mine.resize((size_t)most, -1);
    all.resize((size_t)most * np);
  });
  if ((rc = agree(g, rc))) return rc;  // every rank holds its buffers before the exchange
  rc = step([&] {
    allgather_bytes(g, COMM_ROW, mine.data(), all.data(), sizeof(int64_t) * (size_t)most);
    ids.clear();
    for (int q = 0; q < np; ++q)
      ids.insert(ids.end(), all.begin() + (size_t)q * most, all.begin() + (size_t)q * most + cnts[q]);
  });
  return agree(g, rc);
}

// HipMCL() with its first two steps (MCL.cpp:517-521): RemoveIsolated (:476-493), RandPermute (:496-512)
int grid_hipmcl_prepared(cbg_grid* g, const cbg_tile& A, int64_t gn, const cbg_hipmcl_params& P,
                         const cbg_hipmcl_prep& prep, cbg_hipmcl_iter_fn fn, void* user, cbg_tile* final_local,
                         int64_t* labels, int64_t* nclusters, int64_t* iterations, int64_t* work_ids, int64_t* n_work) {
  check_usable(g);
  int64_t roff = 0, coff = 0;
  int rc = !tile_place(g, A, gn, gn, &roff, &coff) ? CBG_ERR_DIMMISMATCH : CBG_OK;
  if ((rc = agree(g, rc))) return rc;
  std::vector<int64_t> ids;  // ids[k] = the original vertex of working vertex k
  TileGuard W;
  const cbg_tile* cur = &A;
  int64_t nw = gn;
  rc = step([&] {
    ids.resize((size_t)gn);
    for (int64_t v = 0; v < gn; ++v) ids[v] = v;
  });
  if ((rc = agree(g, rc))) return rc;
  if (prep.remove_isolated) {
    if ((rc = grid_nonisolated(g, A, gn, ids))) return rc;
    nw = (int64_t)ids.size();
    const int64_t none = 0;  // an empty list is an extent of 0, a NULL pointer would be "all"
    const int64_t* ip = nw ? ids.data() : &none;
    TileGuard B;
    if ((rc = grid_spref(g, *cur, gn, gn, ip, nw, ip, nw, B.t))) return rc;
    W = std::move(B);
    cur = &W.t;
  }
  if (prep.randpermute) {
    std::vector<int64_t> p, pid;
    rc = step([&] {
      p.resize((size_t)std::max<int64_t>(nw, 1));
      pid.resize((size_t)nw);
      rand_perm(nw, prep.perm_seed, p.data());
      for (int64_t k = 0; k < nw; ++k) pid[k] = ids[p[k]];
    });
    if ((rc = agree(g, rc))) return rc;
    TileGuard B;
    if ((rc = grid_spref(g, *cur, nw, nw, p.data(), nw, p.data(), nw, B.t))) return rc;
    W = std::move(B);
    cur = &W.t;
    ids.swap(pid);
  }
  std::vector<int64_t> wl;
  const bool want = labels || nclusters;
  rc = step([&] { wl.resize((size_t)std::max<int64_t>(nw, 1)); });
  if ((rc = agree(g, rc))) return rc;
  int64_t nc_work = 0;
  if ((rc = grid_hipmcl(g, *cur, nw, P, fn, user, final_local, want ? wl.data() : nullptr, want ? &nc_work : nullptr,
                        iterations)))
    return rc;
  if (want) {
    // back to the original numbering: a working component keeps its vertices, a removed vertex is
    // a cluster of its own, and the clusters are numbered by their smallest original vertex
    rc = step([&] {
      std::vector<int64_t> comp((size_t)std::max<int64_t>(gn, 1), -1), newid((size_t)std::max<int64_t>(nc_work, 1), -1);
      for (int64_t k = 0; k < nw; ++k) comp[ids[k]] = wl[k];
      int64_t nc = 0;
      for (int64_t v = 0; v < gn; ++v) {
        int64_t l;
        if (comp[v] < 0) {
          l = nc++;
        } else {
          if (newid[comp[v]] < 0) newid[comp[v]] = nc++;
          l = newid[comp[v]];
        }
        if (labels) labels[v] = l;
      }
      if (nclusters) *nclusters = nc;
    });
    if ((rc = agree(g, rc))) return rc;
  }
  if (work_ids) std::copy(ids.begin(), ids.end(), work_ids);
  if (n_work) *n_work = nw;
  return CBG_OK;
}

// ---------------------------------------------------------------------------
// Batched betweenness centrality (Applications/BetwCent.cpp:148-217): see include/cbg.h.
// The multiplies are the SUMMA's, the fringe comes from grid_spref, nsp grows through
// merge_tiles, and the masks are tile_ewise; the dense block and its three kernels are in
// cbg_ewise.hip.  Every local step ends in an agreement, like the collectives it sits between.
// ---------------------------------------------------------------------------
BetwcentStats& betwcent_stats() {
  static thread_local BetwcentStats s;
  return s;
}

int grid_betwcent(cbg_grid* g, const cbg_tile& A, const cbg_tile* AT, int64_t gn, const int64_t* roots, int64_t nroots,
                  const cbg_betwcent_params& P, cbg_betwcent_level_fn fn, void* user, double* bc) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  check_usable(g);
  BetwcentStats& st = betwcent_stats();
  st = BetwcentStats{};
  const auto t_all = clk::now();
  hipStream_t cs = g->compute;
  int64_t roff = 0, coff = 0;
  int rc = !tile_place(g, A, gn, gn, &roff, &coff) || (AT && !tile_place(g, *AT, gn, gn, &roff, &coff))
               ? (int)CBG_ERR_DIMMISMATCH
           : (!AT && g->pr != g->pc) ? (int)CBG_ERR_NOTSQUARE
                                     : (int)CBG_OK;
  if ((rc = agree(g, rc))) return rc;
  // a local step: timed into st.ms[what], its code agreed
  auto local = [&](int what, const std::function<void()>& f) {
    const auto t0 = clk::now();
    const int r = step([&] {
      f();
      CBG_HIP(hipStreamSynchronize(cs));
    });
    if (what >= 0) st.ms[what] += ms_since(t0);
    return agree(g, r);
  };
  // every stored entry is `true`: unit-valued copies without loops
  auto unit_noloops = [&](const cbg_tile& X, cbg_tile& out) {
    TileGuard c;
    const int r = local(-1, [&] {
      tile_slice_cols(X, 0, X.n, c.t, cs);
      tile_apply_set(c.t, 1.0, cs);
    });
    return r ? r : grid_remove_loops(g, c.t, gn, gn, out, nullptr);
  };
  TileGuard Au, ATu;
  if ((rc = unit_noloops(A, Au.t))) return rc;
  if (AT) {
    if ((rc = unit_noloops(*AT, ATu.t))) return rc;
  } else if ((rc = grid_transpose(g, Au.t, ATu.t))) {
    return rc;
  }
  int64_t r0 = 0, r1 = 0;
  block_span(gn, g->pr, g->prow, r0, r1);
  const int64_t lm = r1 - r0, lmax = gn - (int64_t)(g->pr - 1) * (gn / g->pr);  // the last block is the longest
  std::vector<double> acc;
  if ((rc = agree(g, step([&] { acc.assign((size_t)std::max<int64_t>(gn, 1), 0.0); })))) return rc;

  for (int64_t b0 = 0, bi = 0; b0 < nroots; b0 += P.batch, ++bi) {
    const int64_t nb = std::min<int64_t>(P.batch, nroots - b0);
    int64_t c0 = 0, c1 = 0;
    block_span(nb, g->pc, g->pcol, c0, c1);
    const int64_t ln = c1 - c0;
    // fringe = AT(:, batch); nsp = 1 at (root k, column k)
    TileGuard fringe, nsp;
    if ((rc = grid_spref(g, ATu.t, gn, gn, nullptr, 0, roots + b0, nb, fringe.t))) return rc;
    rc = local(-1, [&] {
      std::vector<int64_t> cp{0};
      std::vector<int32_t> jc, ir;
      for (int64_t k = c0; k < c1; ++k)
        if (roots[b0 + k] >= r0 && roots[b0 + k] < r1) {
          jc.push_back((int32_t)(k - c0));
          ir.push_back((int32_t)(roots[b0 + k] - r0));
          cp.push_back((int64_t)jc.size());
        }
      const std::vector<double> one(jc.size(), 1.0);
      const int64_t e = (int64_t)jc.size();
      tile_alloc_device(nsp.t, lm, ln, e, e);
      if (e) {
        CBG_HIP(hipMemcpyAsync(nsp.t.cp, cp.data(), sizeof(int64_t) * (e + 1), hipMemcpyHostToDevice, cs));
        CBG_HIP(hipMemcpyAsync(nsp.t.jc, jc.data(), sizeof(int32_t) * e, hipMemcpyHostToDevice, cs));
        CBG_HIP(hipMemcpyAsync(nsp.t.ir, ir.data(), sizeof(int32_t) * e, hipMemcpyHostToDevice, cs));
        CBG_HIP(hipMemcpyAsync(nsp.t.val, one.data(), sizeof(double) * e, hipMemcpyHostToDevice, cs));
        CBG_HIP(hipStreamSynchronize(cs));  // the host vectors end with this step
      }
    });
    if (rc) return rc;

    // ---- forward: the levels of the breadth-first search, path counts as values
    std::vector<TileGuard> levels;
    for (int64_t level = 1;; ++level) {
      int64_t fnnz = fringe.t.nnz;
      if ((rc = agree(g, step([&] { allreduce_sum_i64(g, &fnnz); })))) return rc;
      if (fnnz == 0) break;
      st.counts[CBG_BC_LEVELS] += 1;
      st.counts[CBG_BC_DEEPEST] = std::max(st.counts[CBG_BC_DEEPEST], level);
      st.counts[CBG_BC_FRINGE_ENTRIES] += fnnz;
      if (fn) fn(user, bi, level, fnnz);
      rc = local(CBG_BC_MS_EWISE, [&] {  // nsp += fringe: the fringe holds none of nsp's positions
        if (fringe.t.nnz == 0) return;
        TileGuard sum;
        if (nsp.t.nnz == 0) tile_slice_cols(fringe.t, 0, fringe.t.n, sum.t, cs);
        else merge_tiles({nsp.t, fringe.t}, lm, ln, CBG_PLUS_TIMES, sum.t, cs);
        nsp = std::move(sum);
      });
      if (rc) return rc;
      levels.push_back(std::move(fringe));
      TileGuard prod;
      const auto t0 = clk::now();
      if ((rc = summa_spgemm(g, ATu.t, levels.back().t, gn, gn, CBG_PLUS_TIMES, P.algo, P.exec, prod.t))) return rc;
      st.ms[CBG_BC_MS_FORWARD] += ms_since(t0);
      if ((rc = local(CBG_BC_MS_EWISE, [&] { tile_ewise(prod.t, &nsp.t, CBG_EWISE_EXCLUDE, fringe.t, cs); }))) return rc;
    }

    // ---- backward: the dependencies, from the last level down to level 1
    TileGuard inv;
    DBuf<double> bcu, rs;
    rc = local(CBG_BC_MS_DENSE, [&] {
      tile_slice_cols(nsp.t, 0, nsp.t.n, inv.t, cs);
      tile_apply_rdiv(inv.t, 1.0, cs);
      bcu.reset((size_t)std::max<int64_t>(lm * ln, 1));
      rs.reset((size_t)std::max<int64_t>(lm, 1));
      dense_fill(bcu.p, lm * ln, 1.0, cs);
    });
    if (rc) return rc;
    for (int64_t j = (int64_t)levels.size() - 1; j >= 1; --j) {
      TileGuard w, prod;
      if ((rc = local(CBG_BC_MS_EWISE, [&] { tile_ewise(inv.t, &levels[j].t, CBG_EWISE_FIRST, w.t, cs); }))) return rc;
      if ((rc = local(CBG_BC_MS_DENSE, [&] { dense_scale_tile(w.t, bcu.p, lm, cs); }))) return rc;
      const auto t0 = clk::now();
      if ((rc = summa_spgemm(g, Au.t, w.t, gn, gn, CBG_PLUS_TIMES, P.algo, P.exec, prod.t))) return rc;
      st.ms[CBG_BC_MS_BACKWARD] += ms_since(t0);
      TileGuard scaled;
      rc = local(CBG_BC_MS_EWISE, [&] {
        TileGuard masked;
        tile_ewise(prod.t, &levels[j - 1].t, CBG_EWISE_FIRST, masked.t, cs);
        tile_ewise(masked.t, &nsp.t, CBG_EWISE_MULT, scaled.t, cs);
      });
      if (rc) return rc;
      if ((rc = local(CBG_BC_MS_DENSE, [&] { dense_add_tile(scaled.t, bcu.p, lm, cs); }))) return rc;
    }

    // ---- bc += row sums of bcu: this rank's columns, then the grid row's ranks in rank order,
    // then every grid row's block to every rank
    rc = local(CBG_BC_MS_DENSE, [&] {
      std::vector<double> part((size_t)std::max<int64_t>(lmax, 1), 0.0);
      dense_row_sums(bcu.p, lm, ln, rs.p, cs);
      if (lm) CBG_HIP(hipMemcpyAsync(part.data(), rs.p, sizeof(double) * lm, hipMemcpyDeviceToHost, cs));
      CBG_HIP(hipStreamSynchronize(cs));
      std::vector<double> row((size_t)g->pc * part.size()), col((size_t)g->pr * part.size());
      allgather_bytes(g, COMM_ROW, part.data(), row.data(), sizeof(double) * lmax);
      for (int64_t i = 0; i < lmax; ++i) {
        double s = 0.0;
        for (int q = 0; q < g->pc; ++q) s += row[(size_t)q * lmax + i];
        part[i] = s;
      }
      allgather_bytes(g, COMM_COL, part.data(), col.data(), sizeof(double) * lmax);
      for (int q = 0; q < g->pr; ++q) {
        int64_t a = 0, b = 0;
        block_span(gn, g->pr, q, a, b);
        for (int64_t i = a; i < b; ++i) acc[i] += col[(size_t)q * lmax + (i - a)];
      }
    });
    if (rc) return rc;
    st.counts[CBG_BC_BATCHES] += 1;
  }
  for (int64_t v = 0; v < gn; ++v) bc[v] = acc[v] - (double)nroots;
  st.ms[CBG_BC_MS_TOTAL] = ms_since(t_all);
  return CBG_OK;
}

// ---------------------------------------------------------------------------
// Single-source breadth-first search (include/cbg.h): the loop of TopDownBFS.cpp:427-443 with the
// direction rule of DirOptBFS.cpp:364-365, 388, 409.  The vector steps are in cbg_bfs.hip.
// State on the device: parents and levels of this rank's row block (equal on the ranks of a grid row),
// the frontier as a bitmap over all gn vertices (equal on every rank), and this rank's column block of
// it as a list.  Every step ends in one agreement that also sums the frontier and its pred.
// ---------------------------------------------------------------------------
int grid_bfs(cbg_grid* g, const cbg_tile& A, int64_t gn, int64_t root, const cbg_bfs_params& P, cbg_bfs_level_fn fn,
             void* user, int64_t* parents, int64_t* levels) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
  check_usable(g);
  BfsStats& st = bfs_stats();
  st = BfsStats{};
  const auto t_all = clk::now();
  hipStream_t cs = g->compute;
  int64_t roff = 0, coff = 0, toff = 0, tcoff = 0;
  int rc = !tile_place(g, A, gn, gn, &roff, &coff) ||
                   (P.At_local && (P.At_local->m != A.n || P.At_local->n != A.m || !P.At_local->on_device))
               ? (int)CBG_ERR_DIMMISMATCH
               : (int)CBG_OK;
  if ((rc = agree(g, rc))) return rc;
  const int64_t lm = A.m, ln = A.n, per = gn / g->pr;
  const int64_t lmax = gn - (int64_t)(g->pr - 1) * per;  // the last row block is the longest
  const int64_t wb = (lmax + 63) / 64, wg = (gn + 63) / 64, nw = (ln + 63) / 64;
  // stored entries over the grid: the cut-offs
  int64_t nnz = A.nnz;
  if ((rc = agree(g, step([&] { allreduce_sum_i64(g, &nnz); })))) return rc;
  const int64_t up = P.up_cutoff >= 0 ? P.up_cutoff : nnz / 20;
  const int64_t down = P.down_cutoff >= 0 ? P.down_cutoff
                       : nnz > 0          ? (int64_t)((double)gn * (double)gn / ((double)nnz * 12.0))
                                          : 0;

  DBuf<int64_t> parent, level, candg, all_cand, len, nu, scratch;
  DBuf<int32_t> cand, pos, fl, longq;
  DBuf<u64> bits, rowbits, all_bits, stat;
  TileGuard at_own;
  const cbg_tile* At = P.At_local;
  u64 sh[8] = {};  // stat's host copy: 0 new, 1 pull rows, 2 pull entries, 3 queued, 4 list length, 5 pred, 6 units
  // this rank's part of the current frontier, and the sums over the grid
  int64_t nf = 0, units = 0, frontier = 0, pred = 0;
  // compaction of the current bits, then the agreement that sums the frontier and pred over the grid
  auto compact_and_agree = [&](int code) {
    int r = code ? code : step([&] {
      DeferredFree df;
      bfs_compact(bits.p, coff, ln, len.p, fl.p, nu.p, scratch.p, stat.p + 4, cs, df);
      CBG_HIP(hipMemcpyAsync(sh + 4, stat.p + 4, sizeof(u64) * 3, hipMemcpyDeviceToHost, cs));
      CBG_HIP(hipStreamSynchronize(cs));
      nf = (int64_t)sh[4];
      units = (int64_t)sh[6];
      if (nf > 0) exclusive_scan_i64(nu.p, nu.p + ln + 1, nf, cs, &df);  // ustart
      CBG_HIP(hipStreamSynchronize(cs));
      df.synced = true;
    });
    int64_t v[3] = {r, r ? 0 : nf, r ? 0 : (int64_t)sh[5]};
    std::vector<int64_t> all((size_t)3 * g->nranks);
    const int rr = step([&] { allgather_i64(g, COMM_WORLD, v, all.data(), 3); });
    if (rr) return rr;
    int64_t w = 0, f = 0, pd = 0;
    for (int q = 0; q < g->nranks; ++q) w = std::max(w, all[3 * q]), f += all[3 * q + 1], pd += all[3 * q + 2];
    frontier = f / g->pr;  // every grid row lists the whole frontier once
    pred = pd;
    return (int)w;
  };

  rc = step([&] {
    parent.reset(std::max<int64_t>(lm, 1));
    level.reset(std::max<int64_t>(lm, 1));
    candg.reset(std::max<int64_t>(lm, 1));
    cand.reset(std::max<int64_t>(lm, 1));
    if (g->pc > 1 && g->host_mode) all_cand.reset((size_t)std::max<int64_t>(lm, 1) * g->pc);
    pos.reset(std::max<int64_t>(ln, 1));
    len.reset(std::max<int64_t>(ln, 1));
    fl.reset(std::max<int64_t>(ln, 1));
    nu.reset(2 * ln + 2);
    scratch.reset(2 * (nw + 1));
    bits.reset(std::max<int64_t>(wg, 1));
    rowbits.reset(std::max<int64_t>(wb, 1));
    all_bits.reset((size_t)std::max<int64_t>(wb, 1) * g->pr);
    stat.reset(8);
    CBG_HIP(hipMemsetAsync(parent.p, 0xff, sizeof(int64_t) * std::max<int64_t>(lm, 1), cs));
    CBG_HIP(hipMemsetAsync(level.p, 0xff, sizeof(int64_t) * std::max<int64_t>(lm, 1), cs));
    CBG_HIP(hipMemsetAsync(bits.p, 0, sizeof(u64) * std::max<int64_t>(wg, 1), cs));
    CBG_HIP(hipMemsetAsync(rowbits.p, 0, sizeof(u64) * std::max<int64_t>(wb, 1), cs));
    tile_col_map(A, pos.p, len.p, cs);
    const u64 one = 1ull << (root & 63);
    const int64_t zero = 0;
    CBG_HIP(hipMemcpyAsync(bits.p + (root >> 6), &one, sizeof(u64), hipMemcpyHostToDevice, cs));
    if (root >= roff && root < roff + lm) {  // as DirOptBFS.cpp:371
      CBG_HIP(hipMemcpyAsync(parent.p + (root - roff), &root, sizeof(int64_t), hipMemcpyHostToDevice, cs));
      CBG_HIP(hipMemcpyAsync(level.p + (root - roff), &zero, sizeof(int64_t), hipMemcpyHostToDevice, cs));
    }
    CBG_HIP(hipStreamSynchronize(cs));
  });
  if ((rc = compact_and_agree(rc))) return rc;

  bool pulling = P.direction == CBG_BFS_BOTTOMUP;
  int64_t last = 0;
  st.counts[CBG_BFS_REACHED] = 1;
  for (int64_t lev = 1; frontier > 0; ++lev) {
    if (P.direction == CBG_BFS_AUTO && !pulling && pred > up && last < frontier) pulling = true;
    if (fn) fn(user, lev, pulling ? CBG_BFS_BOTTOMUP : CBG_BFS_TOPDOWN, frontier, pred);
    st.counts[CBG_BFS_EDGES] += pred;
    st.counts[pulling ? CBG_BFS_PULL_STEPS : CBG_BFS_PUSH_STEPS] += 1;
    if (pulling && !At) {  // the local tile's transpose: no grid transpose, so any grid shape
      const auto t0 = clk::now();
      rc = step([&] {
        tile_transpose(A, at_own.t, cs);
        CBG_HIP(hipStreamSynchronize(cs));
      });
      st.ms[CBG_BFS_MS_PULL] += ms_since(t0);
      if ((rc = agree(g, rc))) return rc;
      At = &at_own.t;
    }
    // 1. push or pull into cand, as global ids
    auto t0 = clk::now();
    rc = step([&] {
      CBG_HIP(hipMemsetAsync(stat.p, 0, sizeof(u64) * 4, cs));
      CBG_HIP(hipMemsetAsync(cand.p, 0xff, sizeof(int32_t) * std::max<int64_t>(lm, 1), cs));
      if (pulling) {
        if (!longq.p) longq.reset(std::max<int64_t>(At->nzc, 1));
        bfs_pull_device(*At, bits.p, coff, parent.p, nullptr, cand.p, longq.p, stat.p + 1, cs);
      } else {
        bfs_push_device(A, pos.p, fl.p, nf, nu.p + ln + 1, units, cand.p, cs);
      }
      bfs_cand_global(cand.p, lm, coff, candg.p, cs);
      CBG_HIP(hipStreamSynchronize(cs));
    });
    st.ms[pulling ? CBG_BFS_MS_PULL : CBG_BFS_MS_PUSH] += ms_since(t0);
    if ((rc = agree(g, rc))) return rc;
    // 2. the maximum over the grid row
    t0 = clk::now();
    rc = step([&] {
      if (g->pc == 1 || lm == 0) return;
      if (g->host_mode) {
        allgather_device(g, COMM_ROW, candg.p, all_cand.p, sizeof(int64_t) * lm);
        bfs_cand_max(candg.p, all_cand.p, g->pc, lm, cs);
        CBG_HIP(hipStreamSynchronize(cs));
      } else {
        CBG_NCCL(ncclAllReduce(candg.p, candg.p, (size_t)lm, ncclInt64, ncclMax, g->row, g->comm));
        wait_comm(g);
      }
    });
    st.ms[CBG_BFS_MS_COMM] += ms_since(t0);
    if ((rc = agree(g, rc))) return rc;
    // 3. the update of the row block
    t0 = clk::now();
    rc = step([&] {
      bfs_update(lm, candg.p, parent.p, level.p, lev, rowbits.p, wb, stat.p, cs);
      CBG_HIP(hipMemcpyAsync(sh, stat.p, sizeof(u64) * 4, hipMemcpyDeviceToHost, cs));
      CBG_HIP(hipStreamSynchronize(cs));
    });
    st.ms[CBG_BFS_MS_UPDATE] += ms_since(t0);
    if ((rc = agree(g, rc))) return rc;
    // 4. the row blocks' bits along the grid column -> the frontier over all vertices
    t0 = clk::now();
    rc = step([&] {
      if (wb == 0) return;
      if (g->pr > 1) allgather_device(g, COMM_COL, rowbits.p, all_bits.p, sizeof(u64) * wb);
      bfs_assemble_bits(g->pr > 1 ? all_bits.p : rowbits.p, g->pr, per, wb, gn, bits.p, cs);
      CBG_HIP(hipStreamSynchronize(cs));
    });
    st.ms[CBG_BFS_MS_COMM] += ms_since(t0);
    // 5. the new frontier's list, size and pred (the agreement of step 4 is this one)
    if (!pulling) st.counts[CBG_BFS_PUSH_UNITS] += units;
    else st.counts[CBG_BFS_PULL_ROWS] += (int64_t)sh[1], st.counts[CBG_BFS_PULL_ENTRIES] += (int64_t)sh[2];
    last = frontier;
    t0 = clk::now();
    if ((rc = compact_and_agree(rc))) return rc;
    st.ms[CBG_BFS_MS_UPDATE] += ms_since(t0);
    st.counts[CBG_BFS_REACHED] += frontier;
    if (frontier > 0) st.counts[CBG_BFS_LEVELS] = lev;
    if (P.direction == CBG_BFS_AUTO && pulling && frontier < down && last > frontier) pulling = false;
  }
  // units, rows and entries over the grid
  rc = step([&] {
    int64_t v[3] = {st.counts[CBG_BFS_PUSH_UNITS], st.counts[CBG_BFS_PULL_ROWS], st.counts[CBG_BFS_PULL_ENTRIES]};
    std::vector<int64_t> all((size_t)3 * g->nranks);
    allgather_i64(g, COMM_WORLD, v, all.data(), 3);
    for (int k = 0; k < 3; ++k) {
      int64_t s = 0;
      for (int q = 0; q < g->nranks; ++q) s += all[3 * q + k];
      st.counts[CBG_BFS_PUSH_UNITS + k] = s;
    }
  });
  if ((rc = agree(g, rc))) return rc;
  // every row block to every rank
  rc = step([&] {
    if (g->pr == 1) {  // the one row block is the whole vector: straight into the caller's arrays
      if (lm) CBG_HIP(hipMemcpy(parents, parent.p, sizeof(int64_t) * lm, hipMemcpyDeviceToHost));
      if (lm && levels) CBG_HIP(hipMemcpy(levels, level.p, sizeof(int64_t) * lm, hipMemcpyDeviceToHost));
      return;
    }
    const int64_t l1 = std::max<int64_t>(lmax, 1);
    std::vector<int64_t> mine((size_t)2 * l1, -1), col((size_t)2 * l1 * g->pr);
    if (lm) CBG_HIP(hipMemcpy(mine.data(), parent.p, sizeof(int64_t) * lm, hipMemcpyDeviceToHost));
    if (lm) CBG_HIP(hipMemcpy(mine.data() + l1, level.p, sizeof(int64_t) * lm, hipMemcpyDeviceToHost));
    allgather_bytes(g, COMM_COL, mine.data(), col.data(), sizeof(int64_t) * 2 * l1);
    for (int q = 0; q < g->pr; ++q) {
      int64_t a = 0, b = 0;
      block_span(gn, g->pr, q, a, b);
      for (int64_t i = a; i < b; ++i) {
        parents[i] = col[(size_t)q * 2 * l1 + (i - a)];
        if (levels) levels[i] = col[(size_t)q * 2 * l1 + l1 + (i - a)];
      }
    }
  });
  if ((rc = agree(g, rc))) return rc;
  st.ms[CBG_BFS_MS_TOTAL] = ms_since(t_all);
  return CBG_OK;
}

// ---------------------------------------------------------------------------
// SpMV<SR> over a dense or a sparse vector (ParFriends.h:1860-1990), any pr x pc grid.  The vectors are
// replicated: every rank holds x and receives y.  A rank multiplies its tile by its column block's slice of
// x (cbg_spmv.hip); the results of a grid row's ranks are combined with SR::add in grid-column order, and the
// row blocks are gathered along the grid column.  The reference's dense SpMV exchanges the vector with the
// complement rank of a square grid; here nothing is exchanged before the product.
// ---------------------------------------------------------------------------
int grid_spmv(cbg_grid* g, const cbg_tile* A, const cbg_tile* At, int64_t gm, int64_t gn, int sr, const double* x,
              double* y) {
  check_usable(g);
  spmv_stats_reset();
  hipStream_t cs = g->compute;
  cbg_tile shape{};
  shape.m = A ? A->m : At->n;
  shape.n = A ? A->n : At->m;
  int64_t roff = 0, coff = 0;
  int rc = tile_place(g, shape, gm, gn, &roff, &coff) ? (int)CBG_OK : (int)CBG_ERR_DIMMISMATCH;
  if ((rc = agree(g, rc))) return rc;
  const int64_t lm = shape.m, ln = shape.n, per = gm / g->pr;
  const int64_t lmax = gm - (int64_t)(g->pr - 1) * per;  // the last row block is the longest
  TileGuard own;
  DBuf<double> dx, dy, all;
  // 1. the tile product into lm doubles
  rc = step([&] {
    dx.reset(std::max<int64_t>(ln, 1));
    dy.reset(std::max<int64_t>(lm, 1));
    if ((At ? At->nnz : A->nnz) == 0) {  // an empty tile: id everywhere, no kernel
      std::vector<double> id((size_t)std::max<int64_t>(lm, 1), spmv_identity(sr));
      CBG_HIP(hipMemcpy(dy.p, id.data(), sizeof(double) * id.size(), hipMemcpyHostToDevice));
      return;
    }
    if (ln) CBG_HIP(hipMemcpyAsync(dx.p, x + coff, sizeof(double) * ln, hipMemcpyHostToDevice, cs));
    if (!At) {
      tile_transpose(*A, own.t, cs);
      CBG_HIP(hipStreamSynchronize(cs));
      At = &own.t;
    }
    tile_spmv_device(*At, sr, dx.p, dy.p, cs);
    CBG_HIP(hipStreamSynchronize(cs));
    (void)spmv_stats();
  });
  if ((rc = agree(g, rc))) return rc;
  // 2. the grid row's results in grid-column order
  rc = step([&] {
    if (g->pc == 1 || lm == 0) return;
    all.reset((size_t)lm * g->pc);
    allgather_device(g, COMM_ROW, dy.p, all.p, sizeof(double) * lm);
    spmv_combine_device(dy.p, all.p, g->pc, lm, sr, cs);
    CBG_HIP(hipStreamSynchronize(cs));
  });
  if ((rc = agree(g, rc))) return rc;
  // 3. every row block to every rank
  rc = step([&] {
    if (g->pr == 1) {
      if (lm) CBG_HIP(hipMemcpy(y, dy.p, sizeof(double) * lm, hipMemcpyDeviceToHost));
      return;
    }
    const int64_t l1 = std::max<int64_t>(lmax, 1);
    std::vector<double> mine((size_t)l1, 0.0), col((size_t)l1 * g->pr);
    if (lm) CBG_HIP(hipMemcpy(mine.data(), dy.p, sizeof(double) * lm, hipMemcpyDeviceToHost));
    allgather_bytes(g, COMM_COL, mine.data(), col.data(), sizeof(double) * l1);
    for (int q = 0; q < g->pr; ++q) {
      int64_t a = 0, b = 0;
      block_span(gm, g->pr, q, a, b);
      if (b > a) std::memcpy(y + a, col.data() + (size_t)q * l1, sizeof(double) * (b - a));
    }
  });
  if ((rc = agree(g, rc))) return rc;
  return CBG_OK;
}

// variable-length (id, value) lists of a communicator's ranks, concatenated in rank order
static void allgather_entries(cbg_grid* g, int which, const std::vector<int64_t>& ind, const std::vector<double>& val,
                              std::vector<int64_t>& cnt, std::vector<int64_t>& oind, std::vector<double>& oval) {
  const int P = which == COMM_ROW ? g->pc : g->pr;
  const int64_t mine = (int64_t)ind.size();
  cnt.assign((size_t)P, 0);
  allgather_i64(g, which, &mine, cnt.data(), 1);
  const int64_t mx = std::max<int64_t>(*std::max_element(cnt.begin(), cnt.end()), 1);
  std::vector<int64_t> pi((size_t)mx, 0), ai((size_t)mx * P);
  std::vector<double> pv((size_t)mx, 0.0), av((size_t)mx * P);
  std::copy(ind.begin(), ind.end(), pi.begin());
  std::copy(val.begin(), val.end(), pv.begin());
  allgather_bytes(g, which, pi.data(), ai.data(), sizeof(int64_t) * mx);
  allgather_bytes(g, which, pv.data(), av.data(), sizeof(double) * mx);
  oind.clear();
  oval.clear();
  for (int q = 0; q < P; ++q) {
    oind.insert(oind.end(), ai.begin() + (size_t)q * mx, ai.begin() + (size_t)q * mx + cnt[q]);
    oval.insert(oval.end(), av.begin() + (size_t)q * mx, av.begin() + (size_t)q * mx + cnt[q]);
  }
}

int grid_spmspv(cbg_grid* g, const cbg_tile& A, int64_t gm, int64_t gn, int sr, const int64_t* xind, const double* xval,
                int64_t nx, int64_t* yind, double* yval, int64_t* ny) {
  check_usable(g);
  spmv_stats_reset();
  hipStream_t cs = g->compute;
  int64_t roff = 0, coff = 0;
  int rc = tile_place(g, A, gm, gn, &roff, &coff) ? (int)CBG_OK : (int)CBG_ERR_DIMMISMATCH;
  if ((rc = agree(g, rc))) return rc;
  const int64_t lm = A.m, ln = A.n;
  std::vector<int64_t> li, ci;
  std::vector<double> lv, cv;
  // 1. the tile product with the column block's slice of x
  rc = step([&] {
    const int64_t* lo = std::lower_bound(xind, xind + nx, coff);
    const int64_t* hi = std::lower_bound(lo, xind + nx, coff + ln);
    std::vector<int64_t> lx(lo, hi);
    for (auto& j : lx) j -= coff;
    li.assign((size_t)std::max<int64_t>(lm, 1), 0);
    lv.assign((size_t)std::max<int64_t>(lm, 1), 0.0);
    int64_t lny = 0;
    tile_spmspv(A, sr, lx.data(), xval + (lo - xind), (int64_t)lx.size(), li.data(), lv.data(), &lny, cs);
    li.resize((size_t)lny);
    lv.resize((size_t)lny);
  });
  if ((rc = agree(g, rc))) return rc;
  // 2. the grid row's entries in grid-column order: stable sort by row, each row's entries folded in that order
  rc = step([&] {
    if (g->pc == 1) return;
    std::vector<int64_t> cnt;
    allgather_entries(g, COMM_ROW, li, lv, cnt, ci, cv);
    li.assign(ci.size() + 1, 0);
    lv.assign(cv.size() + 1, 0.0);
    const int64_t runs = spmspv_combine(ci.data(), cv.data(), (int64_t)ci.size(), lm, sr, li.data(), lv.data(), cs);
    li.resize((size_t)runs);
    lv.resize((size_t)runs);
  });
  if ((rc = agree(g, rc))) return rc;
  // 3. every row block's entries to every rank, as global rows
  rc = step([&] {
    for (auto& i : li) i += roff;
    if (g->pr > 1) {
      std::vector<int64_t> cnt;
      allgather_entries(g, COMM_COL, li, lv, cnt, ci, cv);
      li.swap(ci);
      lv.swap(cv);
    }
    std::copy(li.begin(), li.end(), yind);
    std::copy(lv.begin(), lv.end(), yval);
    *ny = (int64_t)li.size();
  });
  if ((rc = agree(g, rc))) return rc;
  return CBG_OK;
}

}  // namespace cbg

extern "C" int cbg_get_unique_id(void* id) {
  if (!id) return CBG_ERR_INVALIDPARAMS;
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return CBG_ERR_RCCL;
  std::memcpy(id, &u, sizeof(u));
  return CBG_OK;
}

extern "C" int cbg_grid_info(const cbg_grid* g, int* rank, int* nranks, int* rows, int* cols, int* prow, int* pcol) {
  if (!g) return CBG_ERR_INVALIDPARAMS;
  if (rank) *rank = g->rank;
  if (nranks) *nranks = g->nranks;
  if (rows) *rows = g->pr;
  if (cols) *cols = g->pc;
  if (prow) *prow = g->prow;
  if (pcol) *pcol = g->pcol;
  return CBG_OK;
}
