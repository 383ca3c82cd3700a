// cbg_capi.cpp -- extern "C" boundary of libcbg (declared in include/cbg.h).
// Every entry point catches exceptions and returns the reference's abort code
// (SpDefs.h:69-76) or a >= 3100 runtime code; cbg_last_error() has the text.
#include <cfloat>
#include <cstring>

#include "cbg_grid.h"

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

template <class F>
int guard(F&& f) {
  try {
    g_err.clear();
    return f();
  } catch (const cbg::HipError& e) {
    return fail(e.code, e.what());
  } catch (const std::exception& e) {
    return fail(CBG_ERR_HIP, e.what());
  } catch (...) {
    return fail(CBG_ERR_HIP, "unknown error");
  }
}

hipStream_t default_stream() {
  static thread_local hipStream_t s = nullptr;
  if (!s) CBG_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return s;
}
hipStream_t as_stream(void* p) { return p ? static_cast<hipStream_t>(p) : default_stream(); }

int check_tile(const cbg_tile* t, bool need_device, const char* name) {
  if (!t) return fail(CBG_ERR_INVALIDPARAMS, std::string(name) + " is NULL");
  if (need_device && !t->on_device) return fail(CBG_ERR_INVALIDPARAMS, std::string(name) + " is not a device tile");
  if (t->m < 0 || t->n < 0 || t->nnz < 0 || t->nzc < 0 || t->nzc > t->n)
    return fail(CBG_ERR_INVALIDPARAMS, std::string(name) + " has inconsistent sizes");
  if (t->m >= INT32_MAX || t->n >= INT32_MAX)
    return fail(CBG_ERR_INVALIDPARAMS, std::string(name) + ": local dimensions must fit int32");
  return CBG_OK;
}
}  // namespace

extern "C" {

const char* cbg_version(void) { return "libcbg 0.1 (gfx950)"; }
const char* cbg_last_error(void) { return g_err.c_str(); }

int cbg_set_device(int device) {
  return guard([&] {
    CBG_HIP(hipSetDevice(device));
    return CBG_OK;
  });
}
int cbg_device_count(int* count) {
  return guard([&] {
    CBG_HIP(hipGetDeviceCount(count));
    return CBG_OK;
  });
}
int cbg_pool_stats(size_t* in_use, size_t* cached) {
  if (in_use) *in_use = cbg::pool().bytes_in_use();
  if (cached) *cached = cbg::pool().bytes_cached();
  return CBG_OK;
}
int cbg_pool_trim(void) {
  return guard([&] {
    cbg::pool().trim();
    return CBG_OK;
  });
}
int cbg_hbm_copy_bandwidth(int64_t bytes, int reps, double* gbps) {
  if (!gbps || bytes <= 0 || reps <= 0) return fail(CBG_ERR_INVALIDPARAMS, "cbg_hbm_copy_bandwidth: bad arguments");
  return guard([&] {
    *gbps = cbg::hbm_copy_gbps(bytes, reps);
    return CBG_OK;
  });
}

int cbg_store_probe(int64_t bytes, int width) {
  if (bytes <= 0 || bytes % 256 || (width != 4 && width != 8))
    return fail(CBG_ERR_INVALIDPARAMS, "cbg_store_probe: bytes a positive multiple of 256, width 4 or 8");
  return guard([&] {
    cbg::store_probe(bytes, width);
    return CBG_OK;
  });
}

int cbg_synchronize(void) {
  return guard([&] {
    CBG_HIP(hipDeviceSynchronize());
    return CBG_OK;
  });
}

int cbg_tile_upload(const cbg_tile* h, cbg_tile* d) {
  if (int rc = check_tile(h, false, "host tile")) return rc;
  if (!d) return fail(CBG_ERR_INVALIDPARAMS, "dst is NULL");
  return guard([&] {
    cbg_tile t{};
    cbg::tile_alloc_device(t, h->m, h->n, h->nnz, h->nzc);
    hipStream_t s = default_stream();
    CBG_HIP(hipMemcpyAsync(t.cp, h->cp, sizeof(int64_t) * (h->nzc + 1), hipMemcpyHostToDevice, s));
    if (h->nzc) CBG_HIP(hipMemcpyAsync(t.jc, h->jc, sizeof(int32_t) * h->nzc, hipMemcpyHostToDevice, s));
    if (h->nnz) {
      CBG_HIP(hipMemcpyAsync(t.ir, h->ir, sizeof(int32_t) * h->nnz, hipMemcpyHostToDevice, s));
      CBG_HIP(hipMemcpyAsync(t.val, h->val, sizeof(double) * h->nnz, hipMemcpyHostToDevice, s));
    }
    CBG_HIP(hipStreamSynchronize(s));
    *d = t;
    return CBG_OK;
  });
}

int cbg_tile_download(const cbg_tile* d, cbg_tile* h) {
  if (int rc = check_tile(d, true, "device tile")) return rc;
  if (!h || !h->cp || (d->nzc && !h->jc) || (d->nnz && (!h->ir || !h->val)))
    return fail(CBG_ERR_INVALIDPARAMS, "host arrays missing");
  return guard([&] {
    hipStream_t s = default_stream();
    CBG_HIP(hipMemcpyAsync(h->cp, d->cp, sizeof(int64_t) * (d->nzc + 1), hipMemcpyDeviceToHost, s));
    if (d->nzc) CBG_HIP(hipMemcpyAsync(h->jc, d->jc, sizeof(int32_t) * d->nzc, hipMemcpyDeviceToHost, s));
    if (d->nnz) {
      CBG_HIP(hipMemcpyAsync(h->ir, d->ir, sizeof(int32_t) * d->nnz, hipMemcpyDeviceToHost, s));
      CBG_HIP(hipMemcpyAsync(h->val, d->val, sizeof(double) * d->nnz, hipMemcpyDeviceToHost, s));
    }
    CBG_HIP(hipStreamSynchronize(s));
    h->m = d->m;
    h->n = d->n;
    h->nnz = d->nnz;
    h->nzc = d->nzc;
    h->on_device = 0;
    return CBG_OK;
  });
}

int cbg_tile_free(cbg_tile* t) {
  if (!t) return CBG_OK;
  return guard([&] {
    if (t->on_device) cbg::tile_free_device(*t);
    return CBG_OK;
  });
}

int cbg_tile_alloc(int64_t m, int64_t n, int64_t nnz, int64_t nzc, cbg_tile* out) {
  if (!out || m < 0 || n < 0 || nnz < 0 || nzc < 0 || nzc > n || (nzc == 0) != (nnz == 0))
    return fail(CBG_ERR_INVALIDPARAMS, "bad tile sizes");
  return guard([&] {
    cbg_tile t{};
    cbg::tile_alloc_device(t, m, n, nnz, nzc);
    if (nzc > 0) CBG_HIP(hipMemset(t.cp, 0, sizeof(int64_t)));
    *out = t;
    return CBG_OK;
  });
}

int cbg_tile_concat_cols(const cbg_tile* parts, int nparts, cbg_tile* out) {
  if (!parts || nparts <= 0 || !out) return fail(CBG_ERR_INVALIDPARAMS, "no parts");
  int64_t n = 0;
  std::vector<int64_t> off;
  for (int i = 0; i < nparts; ++i) {
    if (int rc = check_tile(&parts[i], true, "part")) return rc;
    if (parts[i].m != parts[0].m) return fail(CBG_ERR_DIMMISMATCH, "parts differ in row count");
    off.push_back(n);
    n += parts[i].n;
  }
  if (n >= INT32_MAX) return fail(CBG_ERR_INVALIDPARAMS, "local dimensions must fit int32");
  return guard([&] {
    std::vector<cbg_tile> v(parts, parts + nparts);
    cbg::tile_concat_cols(v, off, parts[0].m, n, *out, default_stream());
    return CBG_OK;
  });
}

int cbg_device_memory(size_t* free_bytes, size_t* total_bytes) {
  return guard([&] {
    size_t f = 0, t = 0;
    CBG_HIP(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    return CBG_OK;
  });
}

int cbg_tile_split_cols(const cbg_tile* t, int64_t cut, cbg_tile* l, cbg_tile* r) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if (cut < 0 || cut > t->n) return fail(CBG_ERR_INVALIDPARAMS, "cut out of range");
  return guard([&] {
    cbg::tile_split_cols(*t, cut, *l, *r, default_stream());
    return CBG_OK;
  });
}

int cbg_tile_split_rows(const cbg_tile* t, int64_t cut, cbg_tile* top, cbg_tile* bot) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if (cut < 0 || cut > t->m) return fail(CBG_ERR_INVALIDPARAMS, "cut out of range");
  return guard([&] {
    cbg::tile_split_rows(*t, cut, *top, *bot, default_stream());
    return CBG_OK;
  });
}

int cbg_tile_digest(const cbg_tile* t, int64_t roff, int64_t coff, uint64_t* hs, uint64_t* hv, double* vsum,
                    uint64_t* unsorted) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if (!hs || !hv || !vsum) return fail(CBG_ERR_INVALIDPARAMS, "digest outputs missing");
  return guard([&] {
    cbg::tile_digest(*t, roff, coff, hs, hv, vsum, unsorted, default_stream());
    return CBG_OK;
  });
}

int cbg_tile_equal(const cbg_tile* a, const cbg_tile* b, double epsilon, int* equal) {
  if (int rc = check_tile(a, true, "a")) return rc;
  if (int rc = check_tile(b, true, "b")) return rc;
  if (!equal || !(epsilon >= 0)) return fail(CBG_ERR_INVALIDPARAMS, "bad equality parameters");
  return guard([&] {
    *equal = cbg::tile_equal(*a, *b, epsilon, default_stream()) ? 1 : 0;
    return CBG_OK;
  });
}

int cbg_tile_transpose(const cbg_tile* t, cbg_tile* out) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if (!out) return fail(CBG_ERR_INVALIDPARAMS, "out is NULL");
  return guard([&] {
    cbg::tile_transpose(*t, *out, default_stream());
    return CBG_OK;
  });
}

int cbg_tile_dim_apply(cbg_tile* t, int dim, const double* vec, int op) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if ((dim != CBG_DIM_COLUMN && dim != CBG_DIM_ROW) || op < CBG_OP_MULTIPLIES || op > CBG_OP_MAX ||
      (!vec && (dim == CBG_DIM_COLUMN ? t->n : t->m) > 0))
    return fail(CBG_ERR_INVALIDPARAMS, "bad DimApply parameters");
  return guard([&] {
    cbg::tile_dim_apply(*t, dim, vec, op, default_stream());
    return CBG_OK;
  });
}

int cbg_restriction_tile(int scale, int order, uint64_t seed, int pr, int pc, int prow, int pcol, cbg_tile* out) {
  if (scale < 1 || scale > 30 || order < 1 || ((int64_t)1 << scale) / order < 1 || pr < 1 || pc < 1 || prow < 0 ||
      prow >= pr || pcol < 0 || pcol >= pc || !out)
    return fail(CBG_ERR_INVALIDPARAMS, "bad restriction parameters");
  return guard([&] {
    cbg::restriction_tile(scale, order, seed, pr, pc, prow, pcol, *out, default_stream());
    return CBG_OK;
  });
}

int cbg_tile_random_values(cbg_tile* t, uint64_t seed, int64_t row_off, int64_t col_off) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if (row_off < 0 || col_off < 0) return fail(CBG_ERR_INVALIDPARAMS, "negative offsets");
  return guard([&] {
    cbg::tile_random_values(*t, seed, row_off, col_off, default_stream());
    return CBG_OK;
  });
}

static const char* summa_msg(int rc);

int cbg_grid_transpose(cbg_grid* g, const cbg_tile* local, cbg_tile* out) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  if (int rc = check_tile(local, true, "tile")) return rc;
  if (!out) return fail(CBG_ERR_INVALIDPARAMS, "out is NULL");
  return guard([&]() -> int {
    CBG_HIP(hipDeviceSynchronize());
    cbg::step_error().clear();
    int rc = cbg::grid_transpose(g, *local, *out);
    if (rc == CBG_ERR_NOTSQUARE) return fail(rc, "SpParMat::Transpose needs a square grid");
    if (rc) return fail(rc, cbg::step_error().empty() ? summa_msg(rc) : "this rank: " + cbg::step_error());
    return CBG_OK;
  });
}

int cbg_grid_block_extract(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, int dim, int64_t lo,
                           int64_t hi, cbg_tile* out) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  if (int rc = check_tile(local, true, "tile")) return rc;
  if (!out) return fail(CBG_ERR_INVALIDPARAMS, "out is NULL");
  return guard([&]() -> int {
    CBG_HIP(hipDeviceSynchronize());
    cbg::step_error().clear();
    int rc = cbg::grid_block_extract(g, *local, gm, gn, dim, lo, hi, *out);
    if (rc == CBG_ERR_INVALIDPARAMS && cbg::step_error().empty())
      return fail(rc, "block range outside the matrix or bad dim");
    if (rc) return fail(rc, cbg::step_error().empty() ? summa_msg(rc) : "this rank: " + cbg::step_error());
    return CBG_OK;
  });
}

int cbg_rmat_tile(int scale, int ef, uint64_t seed, int pr, int pc, int prow, int pcol, cbg_tile* out) {
  if (scale < 1 || scale > 30 || ef < 1 || pr < 1 || pc < 1 || prow < 0 || prow >= pr || pcol < 0 || pcol >= pc || !out)
    return fail(CBG_ERR_INVALIDPARAMS, "bad R-MAT parameters");
  if (((int64_t)1 << scale) * ef >= ((int64_t)1 << 31))
    return fail(CBG_ERR_NOTSUPPORTED, "edge count must stay below 2^31");
  return guard([&] {
    cbg::rmat_tile(scale, ef, seed, pr, pc, prow, pcol, *out, default_stream());
    return CBG_OK;
  });
}

int cbg_local_spgemm(const cbg_tile* A, const cbg_tile* B, int sr, cbg_tile* C, void* stream) {
  if (int rc = check_tile(A, true, "A")) return rc;
  if (int rc = check_tile(B, true, "B")) return rc;
  if (!C) return fail(CBG_ERR_INVALIDPARAMS, "C is NULL");
  if (sr != CBG_PLUS_TIMES && sr != CBG_MIN_PLUS) return fail(CBG_ERR_INVALIDPARAMS, "unknown semiring");
  if (A->n != B->m) return fail(CBG_ERR_DIMMISMATCH, "A.ncol != B.nrow");
  if (A->nnz >= INT32_MAX || B->nnz >= INT32_MAX) return fail(CBG_ERR_NOTSUPPORTED, "A/B tiles need nnz < 2^31");
  return guard([&] {
    cbg::thread_stats() = cbg::LocalStats{};
    cbg::local_spgemm(*A, *B, sr, *C, as_stream(stream));
    return CBG_OK;
  });
}

int cbg_local_symbolic(const cbg_tile* A, const cbg_tile* B, int64_t* flops, int64_t* nnz, void* stream) {
  if (int rc = check_tile(A, true, "A")) return rc;
  if (int rc = check_tile(B, true, "B")) return rc;
  if (A->n != B->m) return fail(CBG_ERR_DIMMISMATCH, "A.ncol != B.nrow");
  if (A->nnz >= INT32_MAX || B->nnz >= INT32_MAX) return fail(CBG_ERR_NOTSUPPORTED, "A/B tiles need nnz < 2^31");
  // the multiply's flops and symbolic kernels only: no C is formed
  return guard([&] {
    cbg::local_symbolic(*A, *B, as_stream(stream), flops, nnz);
    return CBG_OK;
  });
}

int cbg_merge(const cbg_tile* parts, int nparts, int sr, cbg_tile* C, void* stream) {
  if (nparts <= 0 || !parts || !C) return fail(CBG_ERR_INVALIDPARAMS, "no parts");
  for (int i = 0; i < nparts; ++i) {
    if (int rc = check_tile(&parts[i], true, "part")) return rc;
    if (parts[i].m != parts[0].m || parts[i].n != parts[0].n)
      return fail(CBG_ERR_DIMMISMATCH, "Dimensions do not match on MergeAll()");  // Friends.h:672-678
  }
  return guard([&] {
    cbg::thread_stats() = cbg::LocalStats{};
    cbg::merge_stats() = cbg::MergeStats{};
    std::vector<cbg_tile> v(parts, parts + nparts);
    cbg::merge_tiles(v, parts[0].m, parts[0].n, sr, *C, as_stream(stream));
    return CBG_OK;
  });
}

int cbg_last_stats(int64_t* flops, int64_t* nnz, double* ms_sym, double* ms_num, int64_t* n_big, int64_t* n_slabs) {
  const cbg::LocalStats& g_stats = cbg::thread_stats();
  if (flops) *flops = g_stats.flops;
  if (nnz) *nnz = g_stats.nnz;
  if (ms_sym) *ms_sym = g_stats.ms_symbolic;
  if (ms_num) *ms_num = g_stats.ms_numeric;
  if (n_big) *n_big = g_stats.n_big;
  if (n_slabs) *n_slabs = g_stats.n_slabs;
  return CBG_OK;
}

int cbg_last_work_stats(int64_t* counts, int n) {
  const cbg::LocalStats& g_stats = cbg::thread_stats();
  for (int i = 0; counts && i < n && i < CBG_WORK_N; ++i) counts[i] = g_stats.work[i];
  return CBG_WORK_N;
}

int cbg_local_aprep_bounds(int64_t* bounds, int n) { return cbg::local_aprep_bounds(bounds, n); }
int cbg_local_slab_caps(int out[4]) { return cbg::local_slab_caps(out); }

// ---------------- grid ----------------
int cbg_get_unique_id(void* id);  // cbg_summa_id.cpp

int cbg_grid_create(int rank, int nranks, int rows, int cols, const void* uid, cbg_grid** out) {
  if (!out || !uid || rank < 0 || rank >= nranks) return fail(CBG_ERR_INVALIDPARAMS, "bad grid parameters");
  if (int rc = cbg::grid_shape(nranks, rows, cols))
    return fail(rc, rc == CBG_ERR_NOTSQUARE ? "This version only works on a square logical processor grid"
                                            : "grid rows*cols != nranks");
  return guard([&] {
    *out = cbg::grid_create_rccl(rank, nranks, rows, cols, uid);
    return CBG_OK;
  });
}

int cbg_grid_create_host(int rank, int nranks, int rows, int cols, const cbg_host_comm* hc, cbg_grid** out) {
  if (!out || !hc || !hc->bcast || !hc->allgather || rank < 0 || rank >= nranks)
    return fail(CBG_ERR_INVALIDPARAMS, "bad grid parameters");
  if (int rc = cbg::grid_shape(nranks, rows, cols)) return fail(rc, "grid shape");
  return guard([&] {
    *out = cbg::grid_create_host(rank, nranks, rows, cols, hc);
    return CBG_OK;
  });
}

int cbg_grid_destroy(cbg_grid* g) {
  return guard([&] {
    cbg::grid_destroy(g);
    return CBG_OK;
  });
}

int cbg_grid_barrier(cbg_grid* g) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  return guard([&] {
    cbg::barrier(g);
    return CBG_OK;
  });
}
int cbg_grid_allreduce_max(cbg_grid* g, double* v) {
  if (!g || !v) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  return guard([&] {
    cbg::allreduce_f64(g, v, true);
    return CBG_OK;
  });
}
int cbg_grid_allreduce_sum_i64(cbg_grid* g, int64_t* v) {
  if (!g || !v) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  return guard([&] {
    cbg::allreduce_sum_i64(g, v);
    return CBG_OK;
  });
}

// Collective entry points: a check that fails on some ranks only is agreed on
// over the grid before returning, so every rank returns the code (the
// reference MPI_Aborts every rank, SpDefs.h:69-76).
static const char* summa_msg(int rc) {
  return rc == CBG_ERR_DIMMISMATCH   ? "Can not multiply, dimensions does not match"
         : rc == CBG_ERR_MATRIXALIAS ? "Can not multiply, inputs alias"
         : rc == CBG_ERR_NOTSQUARE   ? "needs a square grid"
         : rc == CBG_ERR_INVALIDPARAMS
             ? "bad parameters (a B tile with fewer columns than phases, or a phase callback failed)"
         : rc == CBG_ERR_OOM ? "device memory exhausted on a rank of the grid"
         : rc == CBG_ERR_RCCL ? "communication failure on the grid"
                              : "failed on a rank of the grid";
}

static int summa_args(const cbg_tile* A, const cbg_tile* B, int sr, int algo, int exec) {
  if (int rc = check_tile(A, true, "A")) return rc;
  if (int rc = check_tile(B, true, "B")) return rc;
  if ((sr != CBG_PLUS_TIMES && sr != CBG_MIN_PLUS) || (algo != CBG_DOUBLEBUFF && algo != CBG_SYNCH) ||
      (exec != CBG_EXEC_PANEL && exec != CBG_EXEC_STAGED))
    return fail(CBG_ERR_INVALIDPARAMS, "bad summa parameters");
  if (A->nnz >= INT32_MAX || B->nnz >= INT32_MAX) return fail(CBG_ERR_NOTSUPPORTED, "A/B tiles need nnz < 2^31");
  return CBG_OK;
}

int cbg_summa_spgemm(cbg_grid* g, const cbg_tile* A, const cbg_tile* B, int64_t A_gncol, int64_t B_gnrow, int sr,
                     int algo, int exec, cbg_tile* C) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = summa_args(A, B, sr, algo, exec);
  if (!arg && !C) arg = fail(CBG_ERR_INVALIDPARAMS, "C is NULL");
  if (!arg && A == B) arg = fail(CBG_ERR_MATRIXALIAS, "inputs alias (make a temporary copy of one of them first)");
  const std::string why = g_err;
  return guard([&]() -> int {
    cbg::thread_stats() = cbg::LocalStats{};
    cbg::merge_stats() = cbg::MergeStats{};
    if (arg) return fail(cbg::agree(g, arg), why);  // before any device call: peers must not block
    CBG_HIP(hipDeviceSynchronize());
    cbg::step_error().clear();
    int rc = cbg::summa_spgemm(g, *A, *B, A_gncol, B_gnrow, sr, algo, exec, *C);
    if (rc) return fail(rc, cbg::step_error().empty() ? summa_msg(rc) : "this rank: " + cbg::step_error());
    return CBG_OK;
  });
}

int cbg_summa_spgemm_memeff(cbg_grid* g, const cbg_tile* A, const cbg_tile* B, int64_t A_gncol, int64_t B_gnrow,
                            int sr, int algo, int exec, int phases, int64_t per_process_memory_gb, cbg_phase_fn fn,
                            void* user, cbg_tile* C) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  // A and B may alias: B is copied (ParFriends.h:547-549)
  int arg = summa_args(A, B, sr, algo, exec);
  if (!arg && !C && !fn) arg = fail(CBG_ERR_INVALIDPARAMS, "neither C nor a phase callback");
  const std::string why = g_err;
  return guard([&]() -> int {
    cbg::thread_stats() = cbg::LocalStats{};
    cbg::merge_stats() = cbg::MergeStats{};
    if (arg) return fail(cbg::agree(g, arg), why);  // before any device call: peers must not block
    CBG_HIP(hipDeviceSynchronize());
    cbg::step_error().clear();
    int rc = cbg::summa_spgemm_phased(g, *A, *B, A_gncol, B_gnrow, sr, algo, exec, phases, per_process_memory_gb, fn,
                                      user, C);
    if (rc) return fail(rc, cbg::step_error().empty() ? summa_msg(rc) : "this rank: " + cbg::step_error());
    return CBG_OK;
  });
}

int cbg_summa_spgemm_phased(cbg_grid* g, const cbg_tile* A, const cbg_tile* B, int64_t A_gncol, int64_t B_gnrow,
                            int sr, int algo, int exec, int phases, cbg_phase_fn fn, void* user, cbg_tile* C) {
  return cbg_summa_spgemm_memeff(g, A, B, A_gncol, B_gnrow, sr, algo, exec, phases, 0, fn, user, C);
}

// ---------------- Markov-clustering pruning ----------------
// *active: some parameter asks for pruning (p == NULL or all <= 0: none)
static int mcl_params(const cbg_mcl_params* p, bool* active) {
  *active = false;
  if (!p) return CBG_OK;
  if (p->hard_threshold != p->hard_threshold || p->recover_pct != p->recover_pct)
    return fail(CBG_ERR_INVALIDPARAMS, "MCL pruning: a parameter is NaN");
  if (p->select_num < 0 || p->recover_num < 0)
    return fail(CBG_ERR_INVALIDPARAMS, "MCL pruning: selectNum and recoverNum must not be negative");
  *active = p->hard_threshold > 0 || p->select_num > 0 || p->recover_num > 0 || p->recover_pct > 0;
  return CBG_OK;
}

// a host array of n per-column values on device
static void upload_cols(cbg::DBuf<double>& d, const double* h, int64_t n, hipStream_t s) {
  d.reset((size_t)std::max<int64_t>(n, 1));
  if (n) CBG_HIP(hipMemcpyAsync(d.p, h, sizeof(double) * n, hipMemcpyHostToDevice, s));
}

int cbg_tile_col_stats(const cbg_tile* t, const double* thr, int strict, int64_t* cnt, double* sum) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if (t->n > 0 && (!thr || !cnt || !sum)) return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_col_stats: an array is NULL");
  if (strict != 0 && strict != 1) return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_col_stats: strict is 0 or 1");
  return guard([&] {
    hipStream_t s = default_stream();
    cbg::DBuf<double> dthr, dsum((size_t)std::max<int64_t>(t->n, 1));
    cbg::DBuf<int64_t> dcnt((size_t)std::max<int64_t>(t->n, 1));
    upload_cols(dthr, thr, t->n, s);
    cbg::tile_col_stats_device(*t, dthr.p, strict, dcnt.p, dsum.p, s);
    if (t->n) {
      CBG_HIP(hipMemcpyAsync(cnt, dcnt.p, sizeof(int64_t) * t->n, hipMemcpyDeviceToHost, s));
      CBG_HIP(hipMemcpyAsync(sum, dsum.p, sizeof(double) * t->n, hipMemcpyDeviceToHost, s));
    }
    CBG_HIP(hipStreamSynchronize(s));
    return CBG_OK;
  });
}

int cbg_tile_prune_column(const cbg_tile* t, const double* thr, cbg_tile* out) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if (!out || (t->n > 0 && !thr)) return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_prune_column: thr or out is NULL");
  return guard([&] {
    hipStream_t s = default_stream();
    cbg::DBuf<double> dthr;
    upload_cols(dthr, thr, t->n, s);
    cbg::tile_prune_column_device(*t, dthr.p, *out, s);
    CBG_HIP(hipStreamSynchronize(s));
    return CBG_OK;
  });
}

int cbg_grid_kselect(cbg_grid* g, const cbg_tile* local, const int32_t* cols, int64_t ncols, int64_t k, double* kth) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(local, true, "tile");
  if (!arg && (ncols < 0 || k < 1 || (ncols > 0 && (!cols || !kth))))
    arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_kselect: k >= 1, ncols >= 0 and the arrays are needed");
  const std::string why = g_err;
  return guard([&]() -> int {
    cbg::mcl_stats() = cbg::MclStats{};
    if (arg) return fail(cbg::agree(g, arg), why);
    CBG_HIP(hipDeviceSynchronize());
    cbg::step_error().clear();
    int rc = cbg::grid_kselect(g, *local, cols, ncols, k, kth);
    if (rc == CBG_ERR_INVALIDPARAMS && cbg::step_error().empty())
      return fail(rc, "cbg_grid_kselect: column ids outside the tile, listed twice, or lists that differ along the grid column");
    if (rc) return fail(rc, cbg::step_error().empty() ? summa_msg(rc) : "this rank: " + cbg::step_error());
    return CBG_OK;
  });
}

int cbg_grid_mcl_prune(cbg_grid* g, const cbg_tile* local, const cbg_mcl_params* p, cbg_tile* out) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(local, true, "tile");
  if (!arg && !out) arg = fail(CBG_ERR_INVALIDPARAMS, "out is NULL");
  bool active = false;
  if (!arg) arg = mcl_params(p, &active);
  const std::string why = g_err;
  return guard([&]() -> int {
    cbg::mcl_stats() = cbg::MclStats{};
    if (arg) return fail(cbg::agree(g, arg), why);
    CBG_HIP(hipDeviceSynchronize());
    cbg::step_error().clear();
    int rc = cbg::grid_mcl_prune(g, *local, active ? p : nullptr, *out);
    if (rc) return fail(rc, cbg::step_error().empty() ? summa_msg(rc) : "this rank: " + cbg::step_error());
    return CBG_OK;
  });
}

int cbg_summa_spgemm_mcl(cbg_grid* g, const cbg_tile* A, const cbg_tile* B, int64_t A_gncol, int64_t B_gnrow, int sr,
                         int algo, int exec, int phases, int64_t per_process_memory_gb, cbg_phase_fn fn, void* user,
                         cbg_tile* C, const cbg_mcl_params* p) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = summa_args(A, B, sr, algo, exec);
  if (!arg && !C && !fn) arg = fail(CBG_ERR_INVALIDPARAMS, "neither C nor a phase callback");
  bool active = false;
  if (!arg) arg = mcl_params(p, &active);
  const std::string why = g_err;
  return guard([&]() -> int {
    cbg::thread_stats() = cbg::LocalStats{};
    cbg::merge_stats() = cbg::MergeStats{};
    cbg::mcl_stats() = cbg::MclStats{};
    if (arg) return fail(cbg::agree(g, arg), why);
    CBG_HIP(hipDeviceSynchronize());
    cbg::step_error().clear();
    int rc = active ? cbg::summa_spgemm_mcl(g, *A, *B, A_gncol, B_gnrow, sr, algo, exec, phases,
                                            per_process_memory_gb, fn, user, C, *p)
                    : cbg::summa_spgemm_phased(g, *A, *B, A_gncol, B_gnrow, sr, algo, exec, phases,
                                               per_process_memory_gb, fn, user, C);
    if (rc) return fail(rc, cbg::step_error().empty() ? summa_msg(rc) : "this rank: " + cbg::step_error());
    return CBG_OK;
  });
}

int cbg_mcl_kselect_bounds(int64_t* bounds, int n) { return cbg::mcl_kselect_bounds(bounds, n); }

int cbg_last_mcl_stats(int64_t* counts, int n, double* ms) {
  const cbg::MclStats& m = cbg::mcl_stats();
  for (int i = 0; counts && i < n && i < CBG_MCL_N; ++i) counts[i] = m.counts[i];
  for (int i = 0; ms && i < CBG_MCL_MS_N; ++i) ms[i] = m.ms[i];
  return CBG_MCL_N;
}

// ---------------- HipMCL iteration ----------------
// a collective entry point's frame: the argument error (if any) is agreed before any device work
extern "C++" template <class F>
static int grid_call(cbg_grid* g, int arg, F&& f) {
  const std::string why = g_err;
  return guard([&]() -> int {
    if (arg) return fail(cbg::agree(g, arg), why);
    CBG_HIP(hipDeviceSynchronize());
    cbg::step_error().clear();
    const int rc = f();
    if (rc == CBG_ERR_DIMMISMATCH && cbg::step_error().empty())
      return fail(rc, "the matrix is not square, or the tile is not this rank's block of it");
    if (rc == CBG_ERR_NOTSUPPORTED && cbg::step_error().empty())
      return fail(rc, "connected components: no fixed point within gn rounds");
    if (rc) return fail(rc, cbg::step_error().empty() ? summa_msg(rc) : "this rank: " + cbg::step_error());
    return CBG_OK;
  });
}

int cbg_grid_reduce_cols(cbg_grid* g, const cbg_tile* local, int what, double identity, double* out) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(local, true, "tile");
  if (!arg && (what < CBG_RED_SUM || what > CBG_RED_COUNT || identity != identity || (local->n > 0 && !out)))
    arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_reduce_cols: what is CBG_RED_*, identity a number, out is needed");
  return grid_call(g, arg, [&] { return cbg::grid_reduce_cols(g, *local, what, identity, out); });
}

int cbg_mcl_moment_bounds(int64_t* bounds, int n) { return cbg::mcl_moment_bounds(bounds, n); }

int cbg_tile_apply(cbg_tile* t, int op, double arg) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if (op < CBG_APPLY_POW || op > CBG_APPLY_RDIV || arg != arg)
    return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_apply: op is CBG_APPLY_POW, _SET or _RDIV, arg a number");
  // a compatibility rule (include/cbg.h): op 1 was an unknown op once, and callers probed it with a tile struct
  // without arrays; the two new functors still answer those calls with INVALIDPARAMS.  Every device tile
  // libcbg makes holds cp, an empty one too (cp[0] = 0), and val where it has entries
  if (op != CBG_APPLY_POW && (!t->cp || (t->nnz > 0 && !t->val)))
    return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_apply: the tile has no arrays (cp, or val of a tile with entries, is NULL)");
  return guard([&] {
    hipStream_t s = default_stream();
    if (op == CBG_APPLY_POW) cbg::tile_apply_pow(*t, arg, s);
    else if (op == CBG_APPLY_SET) cbg::tile_apply_set(*t, arg, s);
    else cbg::tile_apply_rdiv(*t, arg, s);
    CBG_HIP(hipStreamSynchronize(s));
    return CBG_OK;
  });
}

int cbg_grid_make_col_stochastic(cbg_grid* g, cbg_tile* local) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  return grid_call(g, check_tile(local, true, "tile"), [&] { return cbg::grid_make_col_stochastic(g, *local); });
}

int cbg_grid_chaos(cbg_grid* g, const cbg_tile* local, double* chaos) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(local, true, "tile");
  if (!arg && !chaos) arg = fail(CBG_ERR_INVALIDPARAMS, "chaos is NULL");
  return grid_call(g, arg, [&] { return cbg::grid_chaos(g, *local, chaos); });
}

static int inflation_arg(double power) {
  if (!(power > 0) || power > DBL_MAX) return fail(CBG_ERR_INVALIDPARAMS, "the inflation must be a positive finite number");
  return CBG_OK;
}

int cbg_grid_inflate(cbg_grid* g, cbg_tile* local, double power, double* chaos) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(local, true, "tile");
  if (!arg && !chaos) arg = fail(CBG_ERR_INVALIDPARAMS, "chaos is NULL");
  if (!arg) arg = inflation_arg(power);
  return grid_call(g, arg, [&] { return cbg::grid_inflate(g, *local, power, chaos); });
}

int cbg_last_inflate_stats(double* ms3, int64_t* nnz) {
  const cbg::HipMclStats& h = cbg::hipmcl_stats();
  for (int i = 0; ms3 && i < 3; ++i) ms3[i] = h.inflate_ms[i];
  if (nnz) *nnz = h.inflate_nnz;
  return CBG_OK;
}

// gm != gn is refused here, before any device work (and again, agreed, with the tile's shape)
static int loops_args(const cbg_tile* local, int64_t gm, int64_t gn, const void* out) {
  if (int rc = check_tile(local, true, "tile")) return rc;
  if (!out) return fail(CBG_ERR_INVALIDPARAMS, "out is NULL");
  if (gm != gn) return fail(CBG_ERR_DIMMISMATCH, "loops need a square matrix");
  return CBG_OK;
}

int cbg_grid_remove_loops(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, cbg_tile* out, int64_t* removed) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  return grid_call(g, loops_args(local, gm, gn, out),
                   [&] { return cbg::grid_remove_loops(g, *local, gm, gn, *out, removed); });
}

int cbg_grid_add_loops(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, const double* loopvals,
                       int replace_existing, cbg_tile* out) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = loops_args(local, gm, gn, out);
  if (!arg && local->n > 0 && !loopvals) arg = fail(CBG_ERR_INVALIDPARAMS, "loopvals is NULL");
  return grid_call(g, arg, [&] { return cbg::grid_add_loops(g, *local, gm, gn, loopvals, replace_existing != 0, *out); });
}

int cbg_grid_adjust_loops(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, cbg_tile* out) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  return grid_call(g, loops_args(local, gm, gn, out), [&] { return cbg::grid_adjust_loops(g, *local, gm, gn, *out); });
}

int cbg_grid_connected_components(cbg_grid* g, const cbg_tile* local, int64_t gn, int64_t* labels, int64_t* ncomponents) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(local, true, "tile");
  if (!arg && gn < 0) arg = fail(CBG_ERR_INVALIDPARAMS, "gn is negative");
  return grid_call(g, arg, [&] { return cbg::grid_connected_components(g, *local, gn, labels, ncomponents); });
}

// the argument checks of cbg_grid_hipmcl (and cbg_grid_hipmcl_prepared), before any device work
static int hipmcl_args(const cbg_tile* A_local, int64_t gn, const cbg_hipmcl_params* params) {
  int arg = check_tile(A_local, true, "A");
  if (!arg && !params) arg = fail(CBG_ERR_INVALIDPARAMS, "params is NULL");
  if (!arg && gn < 0) arg = fail(CBG_ERR_INVALIDPARAMS, "gn is negative");
  if (!arg) arg = inflation_arg(params->inflation);
  bool active = false;
  if (!arg) arg = mcl_params(&params->prune, &active);
  if (!arg && params->max_iterations < 0) arg = fail(CBG_ERR_INVALIDPARAMS, "max_iterations is negative");
  if (!arg && (params->eps != params->eps || params->preprune < -1 || params->preprune > 1 ||
               (params->algo != CBG_DOUBLEBUFF && params->algo != CBG_SYNCH) ||
               (params->exec != CBG_EXEC_PANEL && params->exec != CBG_EXEC_STAGED)))
    arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_hipmcl: eps is NaN, or preprune, algo or exec is out of range");
  if (!arg && A_local->nnz + A_local->n >= INT32_MAX) arg = fail(CBG_ERR_NOTSUPPORTED, "A tiles need nnz < 2^31");
  return arg;
}

int cbg_grid_hipmcl(cbg_grid* g, const cbg_tile* A_local, int64_t gn, const cbg_hipmcl_params* params,
                    cbg_hipmcl_iter_fn fn, void* user, cbg_tile* final_local, int64_t* labels, int64_t* nclusters,
                    int64_t* iterations) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = hipmcl_args(A_local, gn, params);
  return grid_call(g, arg, [&] {
    cbg::thread_stats() = cbg::LocalStats{};
    cbg::merge_stats() = cbg::MergeStats{};
    cbg::mcl_stats() = cbg::MclStats{};
    return cbg::grid_hipmcl(g, *A_local, gn, *params, fn, user, final_local, labels, nclusters, iterations);
  });
}

// ---------------- sparse indexing ----------------
static int index_args(const char* what, const int64_t* idx, int64_t n, int64_t ext) {
  if (!idx) return CBG_OK;
  if (n < 0) return fail(CBG_ERR_INVALIDPARAMS, std::string("a negative number of ") + what + " indices");
  for (int64_t i = 0; i < n; ++i)
    if (idx[i] < 0 || idx[i] >= ext) return fail(CBG_ERR_INVALIDPARAMS, std::string("a ") + what + " index outside the matrix");
  return CBG_OK;
}

int cbg_tile_spref(const cbg_tile* t, const int64_t* ri, int64_t nri, const int64_t* ci, int64_t nci, cbg_tile* out) {
  if (int rc = check_tile(t, true, "tile")) return rc;
  if (!out) return fail(CBG_ERR_INVALIDPARAMS, "out is NULL");
  if (int rc = index_args("row", ri, nri, t->m)) return rc;
  if (int rc = index_args("column", ci, nci, t->n)) return rc;
  if ((ri && nri >= INT32_MAX) || (ci && nci >= INT32_MAX))
    return fail(CBG_ERR_NOTSUPPORTED, "the new tile has 2^31 or more rows or columns");
  return guard([&] {
    cbg::spref_stats() = cbg::SprefStats{};
    cbg::tile_spref(*t, ri, nri, ci, nci, *out, default_stream());
    return CBG_OK;
  });
}

int cbg_grid_spref(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, const int64_t* ri, int64_t nri,
                   const int64_t* ci, int64_t nci, cbg_tile* out) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(local, true, "tile");
  if (!arg && !out) arg = fail(CBG_ERR_INVALIDPARAMS, "out is NULL");
  if (!arg && (gm < 0 || gn < 0)) arg = fail(CBG_ERR_INVALIDPARAMS, "gm or gn is negative");
  if (!arg) {  // the tile's place (Blocks)
    int pr = 1, pc = 1, prow = 0, pcol = 0;
    cbg_grid_info(g, nullptr, nullptr, &pr, &pc, &prow, &pcol);
    if (local->m != cbg::Blocks{gm, pr}.len(prow) || local->n != cbg::Blocks{gn, pc}.len(pcol))
      arg = fail(CBG_ERR_INVALIDPARAMS, "gm x gn does not fit the tile's place in the grid");
    const int64_t nm = ri ? nri : gm, nn = ci ? nci : gn;
    if (!arg) arg = index_args("row", ri, nri, gm);
    if (!arg) arg = index_args("column", ci, nci, gn);
    if (!arg && (cbg::Blocks{nm, pr}.longest() >= INT32_MAX || cbg::Blocks{nn, pc}.longest() >= INT32_MAX))
      arg = fail(CBG_ERR_NOTSUPPORTED, "a new local block has 2^31 or more rows or columns");
  }
  // every check above precedes any device work; the code is agreed over the grid
  return grid_call(g, arg, [&] {
    cbg::spref_stats() = cbg::SprefStats{};
    return cbg::grid_spref(g, *local, gm, gn, ri, nri, ci, nci, *out);
  });
}

// ---------------- sparse element-wise ops ----------------
int cbg_tile_ewise(const cbg_tile* a, const cbg_tile* b, int op, cbg_tile* out) {
  if (int rc = check_tile(a, true, "a")) return rc;
  if (!out) return fail(CBG_ERR_INVALIDPARAMS, "out is NULL");
  if (op < CBG_EWISE_MULT || op > CBG_EWISE_EXCLUDE)
    return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_ewise: op is CBG_EWISE_MULT, _FIRST or _EXCLUDE");
  if (b) {
    if (int rc = check_tile(b, true, "b")) return rc;
    if (a->m != b->m || a->n != b->n) return fail(CBG_ERR_DIMMISMATCH, "cbg_tile_ewise: a and b differ in shape");
  }
  return guard([&] {
    cbg::ewise_stats() = cbg::EwiseStats{};
    cbg::TileGuard o;
    hipStream_t s = default_stream();
    cbg::tile_ewise(*a, b, op, o.t, s);
    CBG_HIP(hipStreamSynchronize(s));
    CBG_HIP(hipGetLastError());  // a refused launch is this call's failure, not a later one's
    *out = o.release();
    return CBG_OK;
  });
}

int cbg_ewise_bounds(int64_t* bounds, int n) { return cbg::ewise_bounds(bounds, n); }

int cbg_last_ewise_stats(int64_t* counts, int n, double* ms) {
  const cbg::EwiseStats& e = cbg::ewise_stats();
  for (int i = 0; counts && i < n && i < CBG_EWISE_N; ++i) counts[i] = e.counts[i];
  if (ms) *ms = e.ms;
  return CBG_EWISE_N;
}

// ---------------- batched betweenness centrality ----------------
int cbg_grid_betwcent(cbg_grid* g, const cbg_tile* A_local, const cbg_tile* AT_local, int64_t gn, const int64_t* roots,
                      int64_t nroots, const cbg_betwcent_params* p, cbg_betwcent_level_fn fn, void* user, double* bc) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(A_local, true, "A");
  if (!arg && AT_local) arg = check_tile(AT_local, true, "AT");
  if (!arg && (!p || gn < 0 || nroots < 0 || (nroots > 0 && !roots) || (gn > 0 && !bc)))
    arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_betwcent: params, roots and bc are needed, gn and nroots >= 0");
  if (!arg && (p->batch < 1 || (p->algo != CBG_DOUBLEBUFF && p->algo != CBG_SYNCH) ||
               (p->exec != CBG_EXEC_PANEL && p->exec != CBG_EXEC_STAGED)))
    arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_betwcent: batch >= 1, algo and exec as the SUMMA's");
  if (!arg) {  // distinct and in range
    std::vector<int64_t> r(roots, roots + nroots);
    std::sort(r.begin(), r.end());
    if (nroots && (r.front() < 0 || r.back() >= gn || std::adjacent_find(r.begin(), r.end()) != r.end()))
      arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_betwcent: the roots are distinct vertices below gn");
  }
  if (!arg && (A_local->nnz >= INT32_MAX || (AT_local && AT_local->nnz >= INT32_MAX)))
    arg = fail(CBG_ERR_NOTSUPPORTED, "A tiles need nnz < 2^31");
  int pr = 1, pc = 1;
  cbg_grid_info(g, nullptr, nullptr, &pr, &pc, nullptr, nullptr);
  if (!arg && !AT_local && pr != pc)
    arg = fail(CBG_ERR_NOTSQUARE, "cbg_grid_betwcent: without AT the grid has to be square (the transpose)");
  if (!arg && nroots > 0) {
    // the batch's columns are spread over the grid's columns: every grid column needs one, so that no rank
    // runs the SUMMA on a block of no columns.  The last batch is the narrowest.
    const int64_t last = nroots % p->batch ? nroots % p->batch : std::min<int64_t>(p->batch, nroots);
    if (last < pc)
      arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_betwcent: a batch (the last one: nroots % batch roots) has fewer roots "
                                        "than the grid has columns");
  }
  // every check above precedes any device work; the code is agreed over the grid
  return grid_call(g, arg, [&] {
    cbg::thread_stats() = cbg::LocalStats{};
    cbg::merge_stats() = cbg::MergeStats{};
    cbg::spref_stats() = cbg::SprefStats{};
    cbg::ewise_stats() = cbg::EwiseStats{};
    return cbg::grid_betwcent(g, *A_local, AT_local, gn, roots, nroots, *p, fn, user, bc);
  });
}

int cbg_last_betwcent_stats(int64_t* counts, int n, double* ms) {
  const cbg::BetwcentStats& b = cbg::betwcent_stats();
  for (int i = 0; counts && i < n && i < CBG_BC_N; ++i) counts[i] = b.counts[i];
  for (int i = 0; ms && i < CBG_BC_MS_N; ++i) ms[i] = b.ms[i];
  return CBG_BC_N;
}

// ---------------- single-source breadth-first search ----------------
// ascending, distinct, inside [0, n)
static bool bfs_index_ok(const int64_t* x, int64_t nx, int64_t n) {
  if (nx < 0 || (nx > 0 && !x)) return false;
  for (int64_t k = 0; k < nx; ++k)
    if (x[k] < 0 || x[k] >= n || (k > 0 && x[k] <= x[k - 1])) return false;
  return true;
}

int cbg_tile_spmspv_max(const cbg_tile* A, const int64_t* xind, const int64_t* xval, int64_t nx, int64_t* yind,
                        int64_t* yval, int64_t* ny) {
  if (int rc = check_tile(A, true, "A")) return rc;
  if (!ny || (A->m > 0 && (!yind || !yval))) return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_spmspv_max: an output is NULL");
  if (!bfs_index_ok(xind, nx, A->n))
    return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_spmspv_max: xind holds nx >= 0 distinct ascending columns below A->n");
  return guard([&] {
    cbg::bfs_stats() = cbg::BfsStats{};
    cbg::bfs_spmspv_max(*A, xind, xval, nx, yind, yval, ny, default_stream());
    return CBG_OK;
  });
}

int cbg_tile_pull_max(const cbg_tile* At, const int64_t* xind, int64_t nx, const uint8_t* skip, int64_t* yind,
                      int64_t* yval, int64_t* ny, int64_t* entries_read) {
  if (int rc = check_tile(At, true, "At")) return rc;
  if (!ny || (At->n > 0 && (!yind || !yval))) return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_pull_max: an output is NULL");
  if (!bfs_index_ok(xind, nx, At->m))
    return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_pull_max: xind holds nx >= 0 distinct ascending columns below At->m");
  return guard([&] {
    cbg::bfs_stats() = cbg::BfsStats{};
    cbg::bfs_pull_max(*At, xind, nx, skip, yind, yval, ny, entries_read, default_stream());
    return CBG_OK;
  });
}

int cbg_bfs_bounds(int64_t* bounds, int n) { return cbg::bfs_bounds(bounds, n); }

int cbg_grid_bfs(cbg_grid* g, const cbg_tile* A_local, int64_t gn, int64_t root, const cbg_bfs_params* p,
                 cbg_bfs_level_fn fn, void* user, int64_t* parents, int64_t* levels) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(A_local, true, "A");
  if (!arg && p && p->At_local) arg = check_tile(p->At_local, true, "At");
  if (!arg && (!p || !parents)) arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_bfs: params and parents are needed");
  if (!arg && (p->direction < CBG_BFS_AUTO || p->direction > CBG_BFS_BOTTOMUP))
    arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_bfs: direction is CBG_BFS_AUTO, _TOPDOWN or _BOTTOMUP");
  if (!arg && (root < 0 || root >= gn)) arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_bfs: the root is a vertex below gn");
  // every check above precedes any device work; the code is agreed over the grid
  return grid_call(g, arg, [&] { return cbg::grid_bfs(g, *A_local, gn, root, *p, fn, user, parents, levels); });
}

int cbg_last_bfs_stats(int64_t* counts, int n, double* ms) {
  const cbg::BfsStats& b = cbg::bfs_stats();
  for (int i = 0; counts && i < n && i < CBG_BFS_N; ++i) counts[i] = b.counts[i];
  for (int i = 0; ms && i < CBG_BFS_MS_N; ++i) ms[i] = b.ms[i];
  return CBG_BFS_N;
}

// ---------------- matrix x vector on PlusTimes and MinPlus ----------------
static bool spmv_sr_ok(int sr) { return sr == CBG_PLUS_TIMES || sr == CBG_MIN_PLUS; }
// the checks the tile and the grid product share; 0 or the code (the message is set)
static int spmv_dense_args(const cbg_tile* A, const cbg_tile* At, int sr, const double* x, double* y) {
  if (!A && !At) return fail(CBG_ERR_INVALIDPARAMS, "spmv: A and At are both NULL");
  if (A)
    if (int rc = check_tile(A, true, "A")) return rc;
  if (At)
    if (int rc = check_tile(At, true, "At")) return rc;
  if (!spmv_sr_ok(sr)) return fail(CBG_ERR_INVALIDPARAMS, "spmv: the semiring is CBG_PLUS_TIMES or CBG_MIN_PLUS");
  const int64_t m = A ? A->m : At->n, n = A ? A->n : At->m;
  if ((m > 0 && !y) || (n > 0 && !x)) return fail(CBG_ERR_INVALIDPARAMS, "spmv: x or y is NULL");
  if (A && At && (At->m != A->n || At->n != A->m))
    return fail(CBG_ERR_DIMMISMATCH, "spmv: At does not have the shape of A's transpose");
  return CBG_OK;
}

int cbg_tile_spmv(const cbg_tile* A, const cbg_tile* At, int semiring, const double* x, double* y, int on_device,
                  void* hip_stream) {
  if (int rc = spmv_dense_args(A, At, semiring, x, y)) return rc;
  return guard([&] {
    cbg::spmv_stats_reset();
    const int64_t m = A ? A->m : At->n, n = A ? A->n : At->m;
    const int64_t nnz = At ? At->nnz : A->nnz;
    hipStream_t s = as_stream(hip_stream);
    if (nnz == 0 && !on_device) {  // an empty tile: id everywhere, no kernel
      for (int64_t i = 0; i < m; ++i) y[i] = cbg::spmv_identity(semiring);
      return (int)CBG_OK;
    }
    cbg::TileGuard own;
    if (!At) {
      cbg::tile_transpose(*A, own.t, s);
      CBG_HIP(hipStreamSynchronize(s));
      At = &own.t;
    }
    if (on_device) {
      cbg::tile_spmv_device(*At, semiring, x, y, s);
      if (own.t.cp) (void)cbg::spmv_stats();  // the transpose made here is freed on return: wait for the product
      return (int)CBG_OK;
    }
    cbg::DBuf<double> dx(std::max<int64_t>(n, 1)), dy(std::max<int64_t>(m, 1));
    struct Wait {  // declared after the buffers, so it runs first
      hipStream_t s;
      ~Wait() { (void)hipStreamSynchronize(s); }
    } wait{s};
    if (n > 0) CBG_HIP(hipMemcpyAsync(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice, s));
    cbg::tile_spmv_device(*At, semiring, dx.p, dy.p, s);
    if (m > 0) CBG_HIP(hipMemcpyAsync(y, dy.p, sizeof(double) * m, hipMemcpyDeviceToHost, s));
    CBG_HIP(hipStreamSynchronize(s));
    (void)cbg::spmv_stats();
    return (int)CBG_OK;
  });
}

int cbg_tile_spmspv(const cbg_tile* A, int semiring, const int64_t* xind, const double* xval, int64_t nx,
                    int64_t* yind, double* yval, int64_t* ny) {
  if (int rc = check_tile(A, true, "A")) return rc;
  if (!spmv_sr_ok(semiring)) return fail(CBG_ERR_INVALIDPARAMS, "spmspv: the semiring is CBG_PLUS_TIMES or CBG_MIN_PLUS");
  if (!ny || (A->m > 0 && (!yind || !yval))) return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_spmspv: an output is NULL");
  if (!bfs_index_ok(xind, nx, A->n) || (nx > 0 && !xval))
    return fail(CBG_ERR_INVALIDPARAMS, "cbg_tile_spmspv: xind holds nx >= 0 distinct ascending columns below A->n, xval their values");
  return guard([&] {
    cbg::spmv_stats_reset();
    cbg::tile_spmspv(*A, semiring, xind, xval, nx, yind, yval, ny, default_stream());
    return CBG_OK;
  });
}

int cbg_grid_spmv(cbg_grid* g, const cbg_tile* A_local, const cbg_tile* At_local, int64_t gm, int64_t gn, int semiring,
                  const double* x, double* y) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = spmv_dense_args(A_local, At_local, semiring, x, y);
  if (!arg && (gm < 0 || gn < 0 || (gm > 0 && !y) || (gn > 0 && !x)))
    arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_spmv: gm, gn >= 0, x and y are needed");
  return grid_call(g, arg, [&] { return cbg::grid_spmv(g, A_local, At_local, gm, gn, semiring, x, y); });
}

int cbg_grid_spmspv(cbg_grid* g, const cbg_tile* A_local, int64_t gm, int64_t gn, int semiring, const int64_t* xind,
                    const double* xval, int64_t nx, int64_t* yind, double* yval, int64_t* ny) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(A_local, true, "A");
  if (!arg && !spmv_sr_ok(semiring))
    arg = fail(CBG_ERR_INVALIDPARAMS, "spmspv: the semiring is CBG_PLUS_TIMES or CBG_MIN_PLUS");
  if (!arg && (gm < 0 || gn < 0 || !ny || (gm > 0 && (!yind || !yval))))
    arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_spmspv: gm, gn >= 0 and the outputs are needed");
  if (!arg && (!bfs_index_ok(xind, nx, gn) || (nx > 0 && !xval)))
    arg = fail(CBG_ERR_INVALIDPARAMS, "cbg_grid_spmspv: xind holds nx >= 0 distinct ascending ids below gn, xval their values");
  return grid_call(g, arg, [&] {
    return cbg::grid_spmspv(g, *A_local, gm, gn, semiring, xind, xval, nx, yind, yval, ny);
  });
}

int cbg_spmv_bounds(int64_t* bounds, int n) { return cbg::spmv_bounds(bounds, n); }

int cbg_last_spmv_stats(int64_t* counts, int n, double* ms) {
  return guard([&] {
    const cbg::SpmvStats& b = cbg::spmv_stats();
    for (int i = 0; counts && i < n && i < CBG_SPMV_N; ++i) counts[i] = b.counts[i];
    if (ms) *ms = b.ms;
    return (int)CBG_SPMV_N;
  });
}

int cbg_rand_perm(int64_t n, uint64_t seed, int64_t* p) {
  if (n < 0 || (n > 0 && !p)) return fail(CBG_ERR_INVALIDPARAMS, "cbg_rand_perm: n >= 0 and p is needed");
  return guard([&] {
    cbg::rand_perm(n, seed, p);
    return CBG_OK;
  });
}

int cbg_spref_sort_bounds(int64_t* bounds, int n) { return cbg::spref_sort_bounds(bounds, n); }

int cbg_last_spref_stats(int64_t* counts, int n, double* ms) {
  const cbg::SprefStats& m = cbg::spref_stats();
  for (int i = 0; counts && i < n && i < CBG_SPREF_N; ++i) counts[i] = m.counts[i];
  for (int i = 0; ms && i < CBG_SPREF_MS_N; ++i) ms[i] = m.ms[i];
  return CBG_SPREF_N;
}

int cbg_grid_nonisolated(cbg_grid* g, const cbg_tile* local, int64_t gn, int64_t* ids, int64_t* n) {
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = check_tile(local, true, "tile");
  if (!arg && (gn < 0 || !n || (gn > 0 && !ids))) arg = fail(CBG_ERR_INVALIDPARAMS, "gn >= 0, ids and n are needed");
  return grid_call(g, arg, [&] {
    std::vector<int64_t> v;
    const int rc = cbg::grid_nonisolated(g, *local, gn, v);
    if (rc) return rc;
    std::copy(v.begin(), v.end(), ids);
    *n = (int64_t)v.size();
    return (int)CBG_OK;
  });
}

int cbg_grid_hipmcl_prepared(cbg_grid* g, const cbg_tile* A_local, int64_t gn, const cbg_hipmcl_params* params,
                             const cbg_hipmcl_prep* prep, cbg_hipmcl_iter_fn fn, void* user, cbg_tile* final_local,
                             int64_t* labels, int64_t* nclusters, int64_t* iterations, int64_t* work_ids,
                             int64_t* n_work) {
  if (!prep || (!prep->remove_isolated && !prep->randpermute)) {
    const int rc = cbg_grid_hipmcl(g, A_local, gn, params, fn, user, final_local, labels, nclusters, iterations);
    if (rc == CBG_OK) {
      for (int64_t v = 0; work_ids && v < gn; ++v) work_ids[v] = v;
      if (n_work) *n_work = gn;
    }
    return rc;
  }
  if (!g) return fail(CBG_ERR_INVALIDPARAMS, "grid is NULL");
  int arg = hipmcl_args(A_local, gn, params);
  return grid_call(g, arg, [&] {
    cbg::thread_stats() = cbg::LocalStats{};
    cbg::merge_stats() = cbg::MergeStats{};
    cbg::mcl_stats() = cbg::MclStats{};
    cbg::spref_stats() = cbg::SprefStats{};
    return cbg::grid_hipmcl_prepared(g, *A_local, gn, *params, *prep, fn, user, final_local, labels, nclusters,
                                     iterations, work_ids, n_work);
  });
}

int cbg_last_hipmcl_stats(int64_t* iterations, double* chaos, int64_t* final_nnz, double* ms_expand, double* ms_prune,
                          double* ms_inflate) {
  const cbg::HipMclStats& h = cbg::hipmcl_stats();
  if (iterations) *iterations = h.iterations;
  if (chaos) *chaos = h.chaos;
  if (final_nnz) *final_nnz = h.final_nnz;
  if (ms_expand) *ms_expand = h.ms_expand;
  if (ms_prune) *ms_prune = h.ms_prune;
  if (ms_inflate) *ms_inflate = h.ms_inflate;
  return CBG_OK;
}

int cbg_last_phase_plan(int* phases, int* automatic, int64_t* flops, int64_t* nnz_est, double* c_budget_bytes,
                        int* oom_splits, double* plan_ms) {
  const cbg::PhasePlan& p = cbg::phase_plan();
  if (phases) *phases = p.phases;
  if (automatic) *automatic = p.automatic;
  if (flops) *flops = p.flops;
  if (nnz_est) *nnz_est = p.nnz_est;
  if (c_budget_bytes) *c_budget_bytes = p.c_budget_bytes;
  if (oom_splits) *oom_splits = cbg::summa_info().oom_splits;
  if (plan_ms) *plan_ms = p.ms;
  return CBG_OK;
}

int cbg_grid_agree(cbg_grid* g, int local_rc, int* agreed) {
  if (!g || !agreed) return fail(CBG_ERR_INVALIDPARAMS, "grid or output is NULL");
  return guard([&] {
    *agreed = cbg::agree(g, local_rc);
    return CBG_OK;
  });
}

int cbg_last_summa_info(int* pieces, double* bcast_ms_piece0, double* est_hidden_ms, double* piece_cost_ms) {
  const cbg::SummaInfo& i = cbg::summa_info();
  if (pieces) *pieces = i.pieces;
  if (bcast_ms_piece0) *bcast_ms_piece0 = i.bcast_ms_piece0;
  if (est_hidden_ms) *est_hidden_ms = i.est_hidden_ms;
  if (piece_cost_ms) *piece_cost_ms = i.piece_cost_ms;
  return CBG_OK;
}

int cbg_last_summa_comm(int* rule, int64_t* bytes_recv, double* exposed_comm_ms) {
  const cbg::SummaInfo& i = cbg::summa_info();
  if (rule) *rule = i.rule;
  if (bytes_recv) *bytes_recv = i.bytes_recv;
  if (exposed_comm_ms) *exposed_comm_ms = i.exposed_comm_ms;
  return CBG_OK;
}

int cbg_merge_stats(int64_t* entries_in, int64_t* entries_out, double* ms) {
  const cbg::MergeStats& m = cbg::merge_stats();
  if (entries_in) *entries_in = m.entries_in;
  if (entries_out) *entries_out = m.entries_out;
  if (ms) *ms = m.ms;
  return CBG_OK;
}

}  // extern "C"
