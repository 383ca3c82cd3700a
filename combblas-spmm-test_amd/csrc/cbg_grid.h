// cbg_grid.h -- the grid layer's private interface: the grid, the block partition, the communication helpers of
// cbg_summa.cpp that cbg_grid_algos.cpp builds on, and every grid-level entry the C ABI (cbg_capi.cpp) calls.
#pragma once
#include <rccl/rccl.h>

#include "cbg_internal.h"

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

struct RcclError : std::runtime_error {
  explicit RcclError(const std::string& s) : std::runtime_error(s) {}
};
#define CBG_NCCL(x)                                                                                   \
  do {                                                                                                \
    ncclResult_t r_ = (x);                                                                            \
    if (r_ != ncclSuccess)                                                                            \
      throw ::cbg::HipError(std::string(#x) + ": " + ncclGetErrorString(r_), CBG_ERR_RCCL);           \
  } while (0)

enum { COMM_WORLD = 0, COMM_ROW = 1, COMM_COL = 2 };

// The block partition of `ext` rows or columns over the `np` ranks of a grid dimension, as
// SpParMat::Owner lays it out (SpParMat.cpp:5068-5097).  The only place that spells the rule; start(np) is the end.
struct Blocks {
  int64_t ext;
  int np;
  int64_t per() const { return ext / np; }  // Owner: every block but the last holds ext / np
  int64_t start(int i) const { return i >= np ? ext : (int64_t)i * per(); }  // Owner: block i starts at i * per
  int64_t len(int i) const { return start(i + 1) - start(i); }  // Owner: per, but the last to the end
  int64_t longest() const { return len(np - 1); }  // Owner: the last block takes the remainder
  void span(int i, int64_t& a, int64_t& b) const { a = start(i), b = start(i + 1); }  // Owner: block i is [a, b)
};

// ---- the communication layer (cbg_summa.cpp) ----
void check_usable(cbg_grid* g);  // throws once the communicators were aborted
void wait_comm(cbg_grid* g);     // the comm stream, under the watchdog
void allgather_i64(cbg_grid* g, int which, const int64_t* in, int64_t* out, int n);
void allgather_bytes(cbg_grid* g, int which, const void* in, void* out, size_t bytes);
void allgather_device(cbg_grid* g, int which, const void* in, void* out, size_t bytes);
void allreduce_f64(cbg_grid* g, double* v, bool max);
void allreduce_sum_i64(cbg_grid* g, int64_t* v);
void barrier(cbg_grid* g);
int agree(cbg_grid* g, int rc);
int agree_val(cbg_grid* g, int rc, int64_t val, int64_t* vmin, int64_t* vmax);
bool redist_fault(cbg_grid* g);
void bcast_tile(cbg_grid* g, int which, int root, const int64_t ess[4], cbg_tile& t, bool mine);
// one step's broadcasts as one RCCL group
template <class F>
void bcast_group(cbg_grid* g, F&& f) {
  if (!g->host_mode) CBG_NCCL(ncclGroupStart());
  try {
    f();
  } catch (...) {
    if (!g->host_mode) (void)ncclGroupEnd();
    throw;
  }
  if (!g->host_mode) CBG_NCCL(ncclGroupEnd());
}
void tile_ess(const cbg_tile& t, int64_t e[4]);  // {m, n, nnz, nzc}
void alloc_like(cbg_tile& t, const int64_t e[4]);
int64_t tile_bytes(const int64_t e[4]);
ColComm col_comm(cbg_grid* g);  // the grid column as the pruning and the MCL iteration see it
// the tile's offsets in the gm x gn matrix, or false when the tile's shape is not its block's
bool tile_place(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, int64_t* roff, int64_t* coff);

// ---- grids, SUMMA and redistributions (cbg_summa.cpp) ----
int grid_shape(int nranks, int& rows, int& cols);
cbg_grid* grid_create_rccl(int rank, int nranks, int rows, int cols, const void* uid);
cbg_grid* grid_create_host(int rank, int nranks, int rows, int cols, const cbg_host_comm* hc);
void grid_destroy(cbg_grid* g);
int summa_spgemm(cbg_grid* g, const cbg_tile& A, const cbg_tile& B, int64_t A_gncol, int64_t B_gnrow, int sr, int algo,
                 int exec, cbg_tile& C);
int summa_spgemm_phased(cbg_grid* g, const cbg_tile& A, const cbg_tile& B, int64_t A_gncol, int64_t B_gnrow, int sr,
                        int algo, int exec, int phases, int64_t mem_gb, cbg_phase_fn fn, void* user, cbg_tile* C);
int grid_transpose(cbg_grid* g, const cbg_tile& T, cbg_tile& out);
int grid_block_extract(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, int dim, int64_t lo, int64_t hi,
                       cbg_tile& out);

// ---- the algorithms on a grid (cbg_grid_algos.cpp) ----
int grid_mcl_prune(cbg_grid* g, const cbg_tile& T, const cbg_mcl_params* p, cbg_tile& out);
int grid_kselect(cbg_grid* g, const cbg_tile& T, const int32_t* cols, int64_t ncols, int64_t k, double* kth);
int summa_spgemm_mcl(cbg_grid* g, const cbg_tile& A, const cbg_tile& B, int64_t A_gncol, int64_t B_gnrow, int sr,
                     int algo, int exec, int phases, int64_t mem_gb, cbg_phase_fn fn, void* user, cbg_tile* C,
                     const cbg_mcl_params& p);
int grid_reduce_cols(cbg_grid* g, const cbg_tile& T, int what, double identity, double* out);
int grid_make_col_stochastic(cbg_grid* g, cbg_tile& T);
int grid_chaos(cbg_grid* g, const cbg_tile& T, double* chaos);
int grid_inflate(cbg_grid* g, cbg_tile& T, double power, double* chaos);
int grid_remove_loops(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, cbg_tile& out, int64_t* removed);
int grid_add_loops(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, const double* loopvals, int replace,
                   cbg_tile& out);
int grid_adjust_loops(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, cbg_tile& out);
int grid_connected_components(cbg_grid* g, const cbg_tile& T, int64_t gn, int64_t* labels, int64_t* ncomp);
int grid_hipmcl(cbg_grid* g, const cbg_tile& A, int64_t gn, const cbg_hipmcl_params& P, cbg_hipmcl_iter_fn fn,
                void* user, cbg_tile* final_local, int64_t* labels, int64_t* nclusters, int64_t* iterations);
int grid_spref(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, const int64_t* ri, int64_t nri,
               const int64_t* ci, int64_t nci, cbg_tile& out);
void rand_perm(int64_t n, uint64_t seed, int64_t* p);
int grid_nonisolated(cbg_grid* g, const cbg_tile& A, int64_t gn, std::vector<int64_t>& ids);
int grid_hipmcl_prepared(cbg_grid* g, const cbg_tile& A, int64_t gn, const cbg_hipmcl_params& P,
                         const cbg_hipmcl_prep& prep, cbg_hipmcl_iter_fn fn, void* user, cbg_tile* final_local,
                         int64_t* labels, int64_t* nclusters, int64_t* iterations, int64_t* work_ids, int64_t* n_work);
int grid_betwcent(cbg_grid* g, const cbg_tile& A, const cbg_tile* AT, int64_t gn, const int64_t* roots, int64_t nroots,
                  const cbg_betwcent_params& P, cbg_betwcent_level_fn fn, void* user, double* bc);
int grid_bfs(cbg_grid* g, const cbg_tile& A, int64_t gn, int64_t root, const cbg_bfs_params& P, cbg_bfs_level_fn fn,
             void* user, int64_t* parents, int64_t* levels);
int grid_spmv(cbg_grid* g, const cbg_tile* A, const cbg_tile* At, int64_t gm, int64_t gn, int sr, const double* x,
              double* y);
int grid_spmspv(cbg_grid* g, const cbg_tile& A, int64_t gm, int64_t gn, int sr, const int64_t* xind, const double* xval,
                int64_t nx, int64_t* yind, double* yval, int64_t* ny);

}  // namespace cbg
