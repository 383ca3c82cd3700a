// cbg_internal.h -- host-side internals of the MI355X SpGEMM library (libcbg).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/cbg.h"

namespace cbg {

struct HipError : std::runtime_error {
  int code;
  HipError(const std::string& s, int c) : std::runtime_error(s), code(c) {}
};

#define CBG_HIP(x)                                                                                  \
  do {                                                                                              \
    hipError_t e_ = (x);                                                                            \
    if (e_ != hipSuccess)                                                                           \
      throw ::cbg::HipError(std::string(#x) + ": " + hipGetErrorString(e_) + " @" + __FILE__ + ":" + \
                                std::to_string(__LINE__),                                           \
                            CBG_ERR_HIP);                                                           \
  } while (0)

typedef unsigned long long u64;

// code of a failure inside a collective step (the step's exception is not
// rethrown: the caller must still reach the next agreement); the first message
// of the calling thread is kept for cbg_last_error() (cbg_summa.cpp)
std::string& step_error();
template <class F>
int step(F&& f) {
  try {
    f();
    return CBG_OK;
  } catch (const HipError& e) {
    if (std::getenv("CBG_DEBUG_ERRORS")) std::fprintf(stderr, "[cbg] %s\n", e.what());
    if (step_error().empty()) step_error() = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    if (step_error().empty()) step_error() = "host allocation failed";
    return CBG_ERR_OOM;
  } catch (const std::exception& e) {  // anything else still reaches the next agreement
    if (step_error().empty()) step_error() = e.what();
    return CBG_ERR_HIP;
  }
}

// mask of the bits of values in [0, maxval] (the digits a radix sort has to visit)
inline u64 low_bits(int64_t maxval) {
  u64 m = 0;
  while ((u64)(maxval > 0 ? maxval : 0) > m) m = (m << 1) | 1ull;
  return m;
}

// Caching device allocator: blocks are rounded up (>= 2 MiB granules for big
// requests) and recycled by size so that repeated multiplies never touch
// hipMalloc/hipFree in steady state (cdna_hip_programming.md Guideline 9).
//
// Growable arrays (reserve_growable/grow) are a reserved virtual range whose
// physical pages are mapped on demand (hipMemAddressReserve + hipMemCreate +
// hipMemMap): a C tile assembled from several multiplies (pipeline pieces,
// merge chunks) is written in place, with no concatenation copy, and holds
// only the memory it uses.  A freed growable block stays mapped in the cache
// (like the hipMalloc blocks) and is handed out again, so steady-state calls
// map nothing; trim() (also run before an allocation is retried on OOM)
// unmaps and releases them.
class DevicePool {
 public:
  void* alloc(size_t bytes);
  void free(void* p);
  void trim();  // release every cached block
  bool release_largest_cached();  // hipFree the largest cached (non-growable) block; false if none
  void* reserve_growable(size_t max_bytes);
  void grow(void* base, size_t bytes);  // map [base, base + bytes)
  size_t bytes_in_use() const { return in_use_; }
  // allocation serial of the live block that contains p (a block handed out
  // again gets a new one); 0 if p is not in a live pool block
  uint64_t serial_of(const void* p);
  size_t bytes_cached() const { return cached_; }
  // Debug mode (CBG_POOL_QUARANTINE=1, read once): a freed block is poisoned at
  // once on a stream of its own (0xff bytes: row ids -1, values NaN), racing any
  // kernel that may still use it, and is not handed out again before
  // quarantine_release() (a device synchronization; every local multiply's end),
  // so a buffer released while a kernel can still read it shows up as a wrong
  // result, not as a rare race with the block's next owner.
  bool quarantine() const { return quarantine_; }
  void quarantine_release();
  DevicePool();
  ~DevicePool() { trim(); }

 private:
  struct Growable {
    size_t reserved = 0, mapped = 0;
    std::vector<std::pair<hipMemGenericAllocationHandle_t, size_t>> chunks;
  };
  void release_growable(void* base, Growable& g);
  std::mutex mu_;
  std::multimap<size_t, void*> free_;
  std::map<void*, size_t> live_;
  std::map<void*, Growable> grow_;        // growable blocks in use
  std::map<void*, Growable> grow_cache_;  // freed growable blocks, still mapped, reused first
  std::map<void*, uint64_t> serial_;      // live blocks (regular and growable) -> allocation serial
  uint64_t next_serial_ = 0;
  size_t in_use_ = 0, cached_ = 0;
  bool quarantine_ = false;
  std::vector<std::pair<void*, size_t>> quar_;  // freed, poisoned, not yet reusable
  hipStream_t poison_ = nullptr;
};
DevicePool& pool();

// cbg_tile.reserved bit: ir/val point into memory the tile does not own (an
// EntryArena's ranges); tile_free_device then frees only cp and jc
constexpr int32_t TILE_BORROWED_ENTRIES = 1;

// where a local multiply puts C's row ids and values (default: fresh pool blocks)
struct OutSink {
  virtual void place(int64_t nnz, int32_t** ir, double** val) = 0;
  virtual ~OutSink() = default;
};
// C entries of consecutive multiplies laid end to end in two growable arrays
struct EntryArena : OutSink {
  int32_t* ir = nullptr;
  double* val = nullptr;
  int64_t used = 0;
  EntryArena();
  ~EntryArena() override;
  void place(int64_t nnz, int32_t** pir, double** pval) override;
  void detach() { ir = nullptr; val = nullptr; used = 0; }
  EntryArena(const EntryArena&) = delete;
  EntryArena& operator=(const EntryArena&) = delete;
};

// RAII device buffer from the pool
template <class T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  DBuf() = default;
  explicit DBuf(size_t count) { reset(count); }
  void reset(size_t count) {
    release();
    n = count;
    if (count) p = static_cast<T*>(pool().alloc(count * sizeof(T)));
  }
  void release() {
    if (p) pool().free(p);
    p = nullptr;
    n = 0;
  }
  T* detach() {
    T* q = p;
    p = nullptr;
    n = 0;
    return q;
  }
  ~DBuf() { release(); }
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
};

// pool blocks whose release waits until the owner's streams are joined and
// synchronized (buffers of kernels running on a side stream)
struct DeferredFree {
  std::vector<void*> ptrs;
  bool synced = false;  // set by the owner after its streams are synchronized
  template <class T>
  void take(DBuf<T>& b) {
    if (b.p) ptrs.push_back(b.detach());
  }
  ~DeferredFree() {
    // an error path leaves without the owner's final sync: kernels may still
    // use the buffers, so wait before they can be handed out again
    if (!synced && !ptrs.empty()) (void)hipDeviceSynchronize();
    for (void* q : ptrs) pool().free(q);
    if (pool().quarantine()) pool().quarantine_release();
  }
};

// A throw out of a frame with kernels running on s waits for them first.  Declare it AFTER every buffer, tile
// guard and DeferredFree they use (destructors run in reverse order); set done after the frame's own last sync.
struct WaitOnThrow {
  hipStream_t s;
  bool done = false;
  ~WaitOnThrow() {
    if (!done) (void)hipStreamSynchronize(s);
  }
};

// blocks of `per` items that cover n items; at least one (a grid of 0 blocks is refused)
inline unsigned nblk(int64_t n, int per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }
// kernels that take more than 64 KiB of dynamic LDS have to say so
template <class K>
void set_lds(K kernel, size_t bytes) {
  if (bytes > 65536)
    CBG_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
}

// local SpGEMM (cbg_local.hip)
struct LocalStats {
  int64_t flops = 0;
  int64_t nnz = 0;
  int64_t n_big = 0, n_slabs = 0;
  double ms_symbolic = 0, ms_numeric = 0;
  int64_t work[CBG_WORK_N] = {};  // cbg_last_work_stats
};
// Every call accumulates into the calling thread's stats (reset by the C ABI
// at the start of each public entry point); `st` optionally receives this call's.
// sink: where C's entries go (C.reserved gets TILE_BORROWED_ENTRIES).
void local_spgemm(const cbg_tile& A, const cbg_tile& B, int semiring, cbg_tile& C, hipStream_t s,
                  LocalStats* st = nullptr, OutSink* sink = nullptr);
LocalStats& thread_stats();
// CUs the persistent slab kernels leave free for communication (cbg_local.hip)
int& comm_reserve_cus();
struct CommReserve {  // scope of a local multiply that runs while a broadcast is in flight
  int prev;
  explicit CommReserve(int cus) : prev(comm_reserve_cus()) { comm_reserve_cus() = cus; }
  ~CommReserve() { comm_reserve_cus() = prev; }
};
// merges run as products (cbg_merge.hip) but are not SpGEMM work: their
// multiplies are kept out of thread_stats() and summed here instead
struct MergeStats {
  int64_t entries_in = 0, entries_out = 0;
  double ms = 0;
};
MergeStats& merge_stats();
// the last PANEL SUMMA's pipelining: pieces multiplied, measured broadcast
// time of the first piece, and the transfer of the rest it estimated
struct SummaInfo {
  int pieces = 0;
  double bcast_ms_piece0 = 0, est_hidden_ms = 0, piece_cost_ms = 0;
  int oom_splits = 0;  // phases computed as column halves after an out-of-memory
  // 0: one piece, no decision; 1: pipelined (RCCL, > 1 remote B tile);
  // 2: adaptive, kept two pieces; 3: adaptive, rejoined into one
  int rule = 0;
  int64_t bytes_recv = 0;      // A and B tile bytes this rank received
  double exposed_comm_ms = 0;  // compute-stream waits for the broadcasts (events)
};
// the last MemEfficientSpGEMM call's phase plan: phases run, and when they
// were chosen from memory, this rank's product flops, estimated nnz(C) and
// the C bytes a phase may take
struct PhasePlan {
  int phases = 0, automatic = 0;
  int64_t flops = 0, nnz_est = 0;
  double c_budget_bytes = 0;
  double ms = 0;  // host time of the planning (collectives and sample included)
};
PhasePlan& phase_plan();
SummaInfo& summa_info();
// A-side preparation (column maps of A) kept across the local multiplies of
// one MemEfficientSpGEMM call, whose phases all multiply the same A: between
// aprep_begin() and aprep_end() on a thread, a local multiply whose A has the
// same arrays, the same pool allocations of them (DevicePool::serial_of: a
// freed and re-allocated block at the same address is a different A) and the
// same sizes as the previous one reuses its maps.
void aprep_begin();
void aprep_end();
struct APrepScope {
  APrepScope() { aprep_begin(); }
  ~APrepScope() { aprep_end(); }
};
// the preparation's thresholds (cbg_local_aprep_bounds): the entries factor of the
// private panel map and the flops factor of the (row, f64) records
int local_aprep_bounds(int64_t* bounds, int n);
// the bitmap slab classes' caps (cbg_local_slab_caps): small, large for f64 sums, then for int32 sums
int local_slab_caps(int out[4]);

// device exclusive scan of n int64 values -> out[0..n], returns nothing (total at out[n]).
// df: the scan's temporaries are released with df (no host synchronization);
// without it the scan synchronizes the stream before returning them.
void exclusive_scan_i64(const int64_t* in, int64_t* out, int64_t n, hipStream_t s, DeferredFree* df = nullptr);
void exclusive_scan_i32_to_i64(const int32_t* in, int64_t* out, int64_t n, hipStream_t s, DeferredFree* df = nullptr);

// thin big columns of the local multiply (cbg_thin.hip): the n columns perm[]
// (fthin products in all) expanded, sorted and reduced into tir/tval[base ...];
// cnt[col] = their nnz, tslot[col] = their first temporary position
// (E = their B entries); thin_copy moves them to C after the column scan
// (ainl: optional inline records of A's columns, see k_inline_cols)
void thin_columns(const int32_t* perm, int n, int64_t E, int64_t fthin, const cbg_tile& A, const cbg_tile& B,
                  const int2* cmap, const int4* ainl, int semiring, int32_t* cnt, int64_t* tslot, int32_t* tir,
                  double* tval, int64_t base, hipStream_t s, DeferredFree& df);
void thin_copy(const int32_t* perm, int n, const int64_t* tslot, const int32_t* cnt, const int64_t* colptr,
               const int32_t* tir, const double* tval, int32_t* out_ir, double* out_val, hipStream_t s);

// radix sort of (key, value) pairs (cbg_sort.hip): LSD over the 8-bit digits
// that `varying` marks as possibly nonzero, stable, 64-bit counts; the sorted
// pairs end in `keys` / `vals` (the DBufs may be swapped with temporaries).
// With df the temporaries are handed to it (no host synchronization: the
// caller's stream sync releases them), else the call synchronizes the stream.
template <typename K>
void radix_sort_pairs(DBuf<K>& keys, DBuf<double>& vals, int64_t n, unsigned long long varying, hipStream_t s,
                      DeferredFree* df = nullptr);
// equal consecutive keys combined with the semiring's add (in order); returns the
// runs (one readback: a host synchronization; temporaries to df when given)
template <typename K>
int64_t reduce_by_key(const K* keys, const double* vals, int64_t n, int semiring, K* ukeys, double* uvals,
                      hipStream_t s, DeferredFree* df = nullptr);

// multiway merge of column-sorted partial tiles (cbg_merge.hip)
// int64 entry counts: column chunks of < 2^30 stacked entries (CBG_MERGE_CHUNK
// overrides) each run as one product into an EntryArena
void merge_tiles(const std::vector<cbg_tile>& parts, int64_t m, int64_t n, int semiring, cbg_tile& C,
                 hipStream_t s);

// tile helpers (cbg_tile.hip)
void tile_free_device(cbg_tile& t);
void tile_alloc_device(cbg_tile& t, int64_t m, int64_t n, int64_t nnz, int64_t nzc);
// owner of a device tile inside host loops: freed on scope exit (exceptions included)
struct TileGuard {
  cbg_tile t{};
  TileGuard() = default;
  explicit TileGuard(const cbg_tile& x) : t(x) {}
  ~TileGuard();
  cbg_tile release() {
    cbg_tile r = t;
    t = cbg_tile{};
    return r;
  }
  TileGuard(TileGuard&& o) noexcept : t(o.release()) {}
  TileGuard& operator=(TileGuard&& o) noexcept;
  TileGuard(const TileGuard&) = delete;
  TileGuard& operator=(const TileGuard&) = delete;
};
void tile_split_cols(const cbg_tile& T, int64_t cut, cbg_tile& L, cbg_tile& R, hipStream_t s);
// columns [a, b) / rows [a, b) of T as a new tile (re-based), one copy
void tile_slice_cols(const cbg_tile& T, int64_t a, int64_t b, cbg_tile& out, hipStream_t s);
void tile_slice_rows(const cbg_tile& T, int64_t a, int64_t b, cbg_tile& out, hipStream_t s);
// column concatenation of tiles whose entries already lie end to end in
// `arena` (parts[k].ir == arena.ir + sum of the earlier parts' nnz): only cp
// and jc are built; `out` takes over the arena's arrays
void tile_assemble_cols(const std::vector<cbg_tile>& parts, const std::vector<int64_t>& col_off, int64_t m,
                        int64_t n, EntryArena& arena, cbg_tile& out, hipStream_t s);
void tile_split_rows(const cbg_tile& T, int64_t cut, cbg_tile& Top, cbg_tile& Bot, hipStream_t s);
void tile_concat_cols(const std::vector<cbg_tile>& parts, const std::vector<int64_t>& col_off, int64_t m,
                      int64_t n, cbg_tile& out, hipStream_t s);
void tile_concat_rows(const std::vector<cbg_tile>& parts, const std::vector<int64_t>& row_off, int64_t m,
                      int64_t n, cbg_tile& out, hipStream_t s);
bool tile_equal(const cbg_tile& a, const cbg_tile& b, double eps, hipStream_t s);
void tile_digest(const cbg_tile& t, int64_t roff, int64_t coff, uint64_t* hs, uint64_t* hv, double* vsum,
                 uint64_t* unsorted, hipStream_t s);
// this rank's tile of the R-MAT test matrix (cbg_rmat.hip)
void rmat_tile(int scale, int ef, uint64_t userseed, int pr, int pc, int prow, int pcol, cbg_tile& out, hipStream_t s);
// phase planning: dim 0 = nonzeros per column (length n), 1 = per row (length m),
// into the device array d zero-padded to `padded` entries (stream synchronized)
void tile_counts_device(const cbg_tile& t, int dim, int32_t* d, int64_t padded, hipStream_t s);
// dense column map (max(n, 1) entries each, queued on s): pos[j] = position of column j in
// jc, -1 where it stores nothing; len (may be NULL) = its length, 0 there
void tile_col_map(const cbg_tile& t, int32_t* pos, int64_t* len, hipStream_t s);
// sum over B's entries (k, j) of a[k] (device array of B.m values): A*B's flops for A's column counts
int64_t entry_sum_device(const cbg_tile& B, const int32_t* a, hipStream_t s);
// sum_k a[k] * b[k] over k < K with a, b stored as blocks (see cbg_tile.hip)
int64_t blocked_dot_device(const int32_t* a, int64_t astride, const std::vector<int64_t>& aoff, const int32_t* b,
                           int64_t bstride, const std::vector<int64_t>& boff, int64_t K, hipStream_t s);
// the columns of T whose id is a multiple of stride (same shape and ids), and
// the rows whose id is (renumbered row / stride: ceil(m / stride) rows)
void tile_sample_cols(const cbg_tile& T, int stride, cbg_tile& out, hipStream_t s);
void tile_sample_rows(const cbg_tile& T, int stride, cbg_tile& out, hipStream_t s);
// estimateFLOP + estimateNNZ_Hash totals of A*B without the numeric phase
void local_symbolic(const cbg_tile& A, const cbg_tile& B, hipStream_t s, int64_t* flops, int64_t* nnz);

// Galerkin path operations (cbg_ops.hip)
void tile_transpose(const cbg_tile& T, cbg_tile& out, hipStream_t s);
void tile_dim_apply(cbg_tile& t, int dim, const double* vec_host, int op, hipStream_t s);
void restriction_tile(int scale, int order, uint64_t seed, int pr, int pc, int prow, int pcol, cbg_tile& out,
                      hipStream_t s);
// values U[-1, 1) from a hash of (seed, global column, global row) (test inputs)
void tile_random_values(cbg_tile& t, uint64_t seed, int64_t roff, int64_t coff, hipStream_t s);

// Markov-clustering pruning (cbg_prune.hip)
struct MclStats {
  int64_t counts[CBG_MCL_N] = {};
  double ms[CBG_MCL_MS_N] = {};
};
MclStats& mcl_stats();  // the calling thread's; reset by the C ABI's pruning entry points
// the column communicator of a grid as the pruning sees it: agree_vals
// allgathers (rc, vals[0..n)) over its P ranks into all[r * n + i] and returns
// the largest rc; allgather_dev gathers device buffers of equal size
struct ColComm {
  int P = 1;
  std::function<int(int rc, const int64_t* vals, int n, int64_t* all)> agree_vals;
  std::function<void(const void* in, void* out, size_t bytes)> allgather_dev;
};
int mcl_kselect_bounds(int64_t* bounds, int n);
void tile_col_stats_device(const cbg_tile& t, const double* thr, int strict, int64_t* cnt, double* sum,
                           hipStream_t s);
void tile_prune_column_device(const cbg_tile& t, const double* thr, cbg_tile& out, hipStream_t s);
int grid_kselect_cols(const ColComm& cc, const cbg_tile& T, const int32_t* cols_host, int64_t ncols, int64_t k,
                      double* kth_host, hipStream_t s);
// pend: a failure of this rank from before the call (reported at the piece's first agreement)
int mcl_prune_piece(const ColComm& cc, const cbg_tile& T, const cbg_mcl_params& P, cbg_tile& out, hipStream_t s,
                    int pend = 0);

// the Markov-clustering iteration (cbg_mcl.hip); the *_device entry points are
// collective along the grid column `cc` and end with an agreement on their code
int mcl_moment_bounds(int64_t* bounds, int n);
void tile_apply_pow(cbg_tile& t, double power, hipStream_t s);
int grid_reduce_cols_device(const ColComm& cc, const cbg_tile& T, int what, double identity, double* out_host,
                            hipStream_t s);
int grid_make_col_stochastic_device(const ColComm& cc, cbg_tile& T, hipStream_t s);
int grid_chaos_device(const ColComm& cc, const cbg_tile& T, double* chaos, hipStream_t s);  // the grid column's
int grid_inflate_device(const ColComm& cc, cbg_tile& T, double power, double* chaos, hipStream_t s, double* ms3);
// mode 0 removes the stored diagonal entries, 1 adds loopval[j] (device, n values) where
// none is stored (replace: also over the stored ones); diag_off = the tile's column
// offset minus its row offset; fix_min: AdjustLoops' Apply; found: diagonal entries stored
void tile_edit_loops_device(const cbg_tile& T, int64_t diag_off, int mode, int replace, int fix_min,
                            const double* loopval, cbg_tile& out, int64_t* found, hipStream_t s);
void cc_init_device(uint64_t* L, int64_t gn, hipStream_t s);
void cc_round_device(const cbg_tile& T, int64_t roff, int64_t coff, uint64_t* L, int64_t gn, uint64_t* changed,
                     hipStream_t s);
void cc_min_device(uint64_t* L, const uint64_t* all, int P, int64_t gn, uint64_t* changed, hipStream_t s);
struct HipMclStats {
  int64_t iterations = 0, final_nnz = 0;
  double chaos = 0, ms_expand = 0, ms_prune = 0, ms_inflate = 0;
  double inflate_ms[3] = {};  // the last cbg_grid_inflate's passes
  int64_t inflate_nnz = 0;
};
HipMclStats& hipmcl_stats();

// sparse indexing B(i, j) = A(ri[i], ci[j]) (cbg_spref.hip)
struct SprefStats {
  int64_t counts[CBG_SPREF_N] = {};
  double ms[CBG_SPREF_MS_N] = {};
};
SprefStats& spref_stats();  // the calling thread's; reset by the C ABI's indexing entry points
int spref_sort_bounds(int64_t* bounds, int n);
bool spref_strictly_increasing(const int64_t* v, int64_t n);
// column stage: len[j] = the stored length of global column sel[j] (device ids), from np
// blocks of `stride` column counts (blocks of `per` columns, the last longer); then the
// columns rank q owns copied from its tile to the offsets ocp[j]
void spref_sel_lengths(const int64_t* sel, int64_t nsel, const int32_t* cnt, int64_t stride, int64_t per, int np,
                       int64_t* len, hipStream_t s);
void spref_sel_copy(const cbg_tile& src, int q, int64_t per, int np, const int64_t* sel, int64_t nsel,
                    const int64_t* ocp, int32_t* oir, double* oval, hipStream_t s);
// dense offsets cp[0 .. ncols] of the columns ids[] (NULL: 0, 1, ...) -> a DCSC tile that takes over ir and val
void spref_compact(int64_t m, int64_t n, const int32_t* ids, int64_t ncols, const int64_t* cp, DBuf<int32_t>& ir,
                   DBuf<double>& val, int64_t nnz, cbg_tile& out, hipStream_t s);
// row stage: the inverse of ri (HOST, n new rows asking for old global rows < gm), and a tile whose
// rows are the old rows row0 ... expanded to the new rows (new_m of them), columns left unsorted
struct RowInverse {
  DBuf<int32_t> cnt, list;
  DBuf<int64_t> start;
};
void spref_build_inverse(const int64_t* ri_host, int64_t n, int64_t gm, RowInverse& inv, hipStream_t s);
void spref_expand_rows(const cbg_tile& X, int64_t row0, const RowInverse& inv, int64_t new_m, cbg_tile& out,
                       hipStream_t s);
void spref_sort_columns(cbg_tile& t, hipStream_t s);  // rows ascending in every column, in place
void tile_spref(const cbg_tile& T, const int64_t* ri, int64_t nri, const int64_t* ci, int64_t nci, cbg_tile& out,
                hipStream_t s);

// sparse element-wise ops (cbg_ewise.hip)
struct EwiseStats {
  int64_t counts[CBG_EWISE_N] = {};
  double ms = 0;
};
EwiseStats& ewise_stats();  // the calling thread's; reset by cbg_tile_ewise
int ewise_bounds(int64_t* bounds, int n);
// b == NULL counts as the empty tile; a and b device tiles of equal shape (a == b allowed)
void tile_ewise(const cbg_tile& a, const cbg_tile* b, int op, cbg_tile& out, hipStream_t s);
// SpParMat::Apply's value functors beside the power (cbg_ewise.hip): v <- arg, v <- arg / v
void tile_apply_set(cbg_tile& t, double arg, hipStream_t s);
void tile_apply_rdiv(cbg_tile& t, double arg, hipStream_t s);

// BetwCent's dense block (cbg_ewise.hip): column-major, lm rows per column; t's columns index it
void dense_fill(double* d, int64_t n, double v, hipStream_t s);
void dense_scale_tile(cbg_tile& t, const double* bcu, int64_t lm, hipStream_t s);       // t(i, j) *= bcu(i, j)
void dense_add_tile(const cbg_tile& t, double* bcu, int64_t lm, hipStream_t s);         // bcu(i, j) += t(i, j)
void dense_row_sums(const double* bcu, int64_t lm, int64_t ln, double* out, hipStream_t s);
struct BetwcentStats {
  int64_t counts[CBG_BC_N] = {};
  double ms[CBG_BC_MS_N] = {};
};
BetwcentStats& betwcent_stats();

// SelectMax matrix x sparse vector and the breadth-first search's vector steps (cbg_bfs.hip)
struct BfsStats {
  int64_t counts[CBG_BFS_N] = {};
  double ms[CBG_BFS_MS_N] = {};
};
BfsStats& bfs_stats();  // the calling thread's; reset by the C ABI's entry points
int bfs_bounds(int64_t* bounds, int n);
void bfs_spmspv_max(const cbg_tile& A, const int64_t* xind, const int64_t* xval, int64_t nx, int64_t* yind,
                    int64_t* yval, int64_t* ny, hipStream_t s);
void bfs_pull_max(const cbg_tile& At, const int64_t* xind, int64_t nx, const uint8_t* skip, int64_t* yind,
                  int64_t* yval, int64_t* ny, int64_t* entries_read, hipStream_t s);
// push: pos = A's column map; fl[nf] the frontier's local columns, ustart the scan of their units; cand: -1 = none
void bfs_push_device(const cbg_tile& A, const int32_t* pos, const int32_t* fl, int64_t nf, const int64_t* ustart,
                     int64_t units, int32_t* cand, hipStream_t s);
// pull: bits = the frontier over the global columns, coff = At's row offset in them; parent / skip may be
// NULL; longq: At.nzc slots; stat (3 words, zeroed by the caller): rows scanned, entries read, rows queued
void bfs_pull_device(const cbg_tile& At, const u64* bits, int64_t coff, const int64_t* parent, const uint8_t* skip,
                     int32_t* cand, int32_t* longq, u64* stat, hipStream_t s);
void bfs_cand_global(const int32_t* cand, int64_t lm, int64_t coff, int64_t* candg, hipStream_t s);
void bfs_cand_max(int64_t* candg, const int64_t* all, int P, int64_t lm, hipStream_t s);  // all: P blocks of lm
// rowbits: wb words of the row block's new frontier (rewritten); *count += their number
void bfs_update(int64_t lm, const int64_t* candg, int64_t* parent, int64_t* level, int64_t lev, u64* rowbits, int64_t wb,
                u64* count, hipStream_t s);
// all: pr blocks of wb words, block q the rows from q * per -> bits over gn vertices
void bfs_assemble_bits(const u64* all, int pr, int64_t per, int64_t wb, int64_t gn, u64* bits, hipStream_t s);
// the set bits of [coff, coff + ln) -> fl (ascending local ids), nu (their units); stat (3 words, zeroed
// here): the list's length, pred, units; scratch: 2 * (ceil(ln / 64) + 1) int64; fl / nu: room for ln
void bfs_compact(const u64* bits, int64_t coff, int64_t ln, const int64_t* len, int32_t* fl, int64_t* nu,
                 int64_t* scratch, u64* stat, hipStream_t s, DeferredFree& df);

// y = A x on PlusTimes and MinPlus over a dense or a sparse vector (cbg_spmv.hip)
struct SpmvStats {
  int64_t counts[CBG_SPMV_N] = {};
  double ms = 0;
};
SpmvStats& spmv_stats();  // the calling thread's, summed since the last reset; waits for a product still running
void spmv_stats_reset();
int spmv_bounds(int64_t* bounds, int n);
double spmv_identity(int sr);  // the reference's SR::id(): 0.0, DBL_MAX
// y (device, At.n) = A x with At = A's transpose and x (device, At.m): queued on s, nothing waits.  The
// call's temporaries return to the pool when the thread's next product starts or its statistics are read.
void tile_spmv_device(const cbg_tile& At, int sr, const double* x, double* y, hipStream_t s);
// y[i] = all[i] + all[lm + i] + ... over the P blocks in order (SR::add)
void spmv_combine_device(double* y, const double* all, int P, int64_t lm, int sr, hipStream_t s);
// host vectors in and out; synchronizes s
void tile_spmspv(const cbg_tile& A, int sr, const int64_t* xind, const double* xval, int64_t nx, int64_t* yind,
                 double* yval, int64_t* ny, hipStream_t s);
// n partial entries (rows below m) concatenated in rank order -> one entry per row, the row's entries folded in
// that order; host arrays; returns the entries out
int64_t spmspv_combine(const int64_t* ind, const double* val, int64_t n, int64_t m, int sr, int64_t* oind, double* oval,
                       hipStream_t s);

// measured HBM bandwidth: 16-B-per-lane device copy (cbg_ops.hip)
double hbm_copy_gbps(int64_t bytes, int reps);
void store_probe(int64_t bytes, int width);

}  // namespace cbg
