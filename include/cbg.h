/* cbg.h -- C ABI of libcbg, the MI355X-native CombBLAS 2D-SUMMA SpGEMM hot path.
 *
 * Plain C types only (pointers + sizes): this is the drop-in boundary that a
 * CombBLAS build (C++ shim: combblas-spmm-test_amd/include/combblas_amd/) or
 * any FFI (ctypes stub in INTEGRATION.md) binds.  Each entry point names the
 * reference interface it replaces (paths relative to the reference root).
 *
 * Tiles are DCSC, the reference's Dcsc<IT,NT> (include/CombBLAS/dcsc.h:85-91):
 *   cp[nzc+1] column pointers (int64 here: C tiles exceed 2^31 nnz at scale>=20),
 *   jc[nzc]   ids of the nonempty columns (ascending),
 *   ir[nnz]   row ids, ascending inside each column,
 *   val[nnz]  fp64 values.
 * Local indices are int32 (SpDCCols<int32_t,double>, MultTiming.cpp:18-23);
 * A and B tiles need nnz < 2^31.
 *
 * Error model: the reference MPI_Aborts with SpDefs.h:69-76 codes; libcbg
 * returns the same code instead (3001 GRIDMISMATCH, 3002 DIMMISMATCH,
 * 3003 NOTSQUARE, 3005 MATRIXALIAS, 3007 INVALIDPARAMS) and >= 3100 for
 * device/runtime failures.  cbg_last_error() gives the message.
 */
#ifndef CBG_H
#define CBG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cbg_tile {
  int64_t m, n, nnz, nzc;
  int64_t* cp;
  int32_t* jc;
  int32_t* ir;
  double* val;
  int32_t on_device; /* 1: arrays are device memory (owned by libcbg when produced by it) */
  int32_t reserved;
} cbg_tile;

/* semirings: PlusTimesSRing<double,double> Semirings.h:212-233,
 *            MinPlusSRing<double,double>   Semirings.h:235-255 */
enum { CBG_PLUS_TIMES = 0, CBG_MIN_PLUS = 1 };

/* SUMMA variants */
enum {
  CBG_DOUBLEBUFF = 0, /* Mult_AnXBn_DoubleBuff ParFriends.h:798-997 */
  CBG_SYNCH = 1       /* Mult_AnXBn_Synch      ParFriends.h:1004-1108 (PSpGEMM SpParMat.h:454-467) */
};
/* how the stages are executed on device (identical results up to fp order) */
enum {
  CBG_EXEC_PANEL = 0, /* gather the A block-row, receive the B block-column in column pieces
                         (piece p+1 broadcast while piece p multiplies), one local multiply per
                         piece, C entries written end to end: no partial products, no merge */
  CBG_EXEC_STAGED = 1 /* the reference's stages (any pr x pc grid: inner dimension cut at the union
                         of A's column-block and B's row-block boundaries), stage s+1 broadcast while
                         stage s multiplies, then an on-device multiway merge of the partials */
};

enum {
  CBG_OK = 0,
  CBG_ERR_GRIDMISMATCH = 3001,
  CBG_ERR_DIMMISMATCH = 3002,
  CBG_ERR_NOTSQUARE = 3003,
  CBG_ERR_MATRIXALIAS = 3005,
  CBG_ERR_INVALIDPARAMS = 3007,
  CBG_ERR_HIP = 3100,
  CBG_ERR_RCCL = 3101,
  CBG_ERR_OOM = 3102,
  CBG_ERR_NOTSUPPORTED = 3103,
  CBG_ERR_INTERNAL = 3104 /* a check of the library on its own state failed */
};

/* ---------------- library ---------------- */
const char* cbg_version(void);
const char* cbg_last_error(void);
/* select the HIP device for the calling thread (default: current device) */
int cbg_set_device(int device);
int cbg_device_count(int* count);
/* device memory of libcbg's caching pool (bytes) */
int cbg_pool_stats(size_t* in_use, size_t* cached);
int cbg_pool_trim(void);
int cbg_synchronize(void);
/* measured side of the HBM roofline (no reference counterpart): a 16-byte-per-lane
 * device copy of `bytes` run `reps` times; *gbps = 2 * bytes * reps / time (GB/s) */
int cbg_hbm_copy_bandwidth(int64_t bytes, int reps, double* gbps);
/* known-bytes store probe for the PMC traffic calibration (tools/traffic.py, no
 * reference counterpart): writes exactly `bytes` (a multiple of 256) of a scratch
 * buffer with `width`-byte stores (4 or 8) per lane -- the SpGEMM kernels' C row
 * ids and values -- consecutive lanes at consecutive addresses (k_store_probe<W>) */
int cbg_store_probe(int64_t bytes, int width);

/* ---------------- tiles ---------------- */
/* host -> device copy (arrays of *dst are allocated by libcbg) */
int cbg_tile_upload(const cbg_tile* host, cbg_tile* dst);
/* device -> host into caller-provided arrays sized from dev->nnz/nzc */
int cbg_tile_download(const cbg_tile* dev, cbg_tile* host);
/* frees a device tile produced by libcbg (no-op for host tiles) */
int cbg_tile_free(cbg_tile* t);
/* SpDCCols::CreateImpl(essentials) (SpDCCols.cpp:733-745): an uninitialised device
 * tile of the given sizes (cp[0] = 0), e.g. the receive buffers of BCastMatrix */
int cbg_tile_alloc(int64_t m, int64_t n, int64_t nnz, int64_t nzc, cbg_tile* out);
/* SpDCCols::ColConcatenate / Merge (SpDCCols.cpp:1194-1223, ParFriends.h:724-725):
 * parts side by side (part k's columns shifted by the widths of parts 0..k-1),
 * all with the same row count; device tiles */
int cbg_tile_concat_cols(const cbg_tile* parts, int nparts, cbg_tile* out);
/* device memory: free and total bytes (hipMemGetInfo) */
int cbg_device_memory(size_t* free_bytes, size_t* total_bytes);
/* SpDCCols::Split (SpDCCols.cpp:905-930): columns [0,cut) and [cut,n) (device) */
int cbg_tile_split_cols(const cbg_tile* t, int64_t cut, cbg_tile* left, cbg_tile* right);
/* row split of B as DoubleBuff does with Transpose/Split/Transpose (ParFriends.h:824-829), no transposes */
int cbg_tile_split_rows(const cbg_tile* t, int64_t cut, cbg_tile* top, cbg_tile* bottom);
/* structural + value digest (same definition as tests/golden/make_golden.py), device tile.
 * unsorted (may be NULL) receives the number of DCSC order violations: a row id not
 * strictly above its predecessor in its column, a column id not strictly above the
 * previous one, an empty column, cp[0] != 0 or cp[nzc] != nnz (0 for a valid tile). */
int cbg_tile_digest(const cbg_tile* t, int64_t row_off, int64_t col_off, uint64_t* hs, uint64_t* hv, double* vsum,
                    uint64_t* unsorted);
/* SpDCCols::operator== (SpDCCols.h:74-81, Dcsc::operator== dcsc.cpp:472-510):
 * two empty tiles are equal; else m, n, nnz, nzc, cp, jc, ir must match and
 * values be ErrorTolerantEqual (Compare.h:47-65: equal, or absolute or
 * relative difference < epsilon; the reference's EPSILON is 0.01, SpDefs.h:64).
 * Device tiles; *equal receives 1 or 0. */
int cbg_tile_equal(const cbg_tile* a, const cbg_tile* b, double epsilon, int* equal);

/* ---------------- Galerkin triple-product path (GalerkinNew.cpp:96-153) ---------------- */
/* SpDCCols::Transpose (SpDCCols.cpp:853-873): out = t^T as a device DCSC tile */
int cbg_tile_transpose(const cbg_tile* t, cbg_tile* out);
/* SpParMat::DimApply (SpParMat.cpp:801): dim CBG_DIM_COLUMN: x(i,j) = op(x(i,j), vec[j]);
 * CBG_DIM_ROW: x(i,j) = op(x(i,j), vec[i]); vec is HOST memory of t->n (t->m) values,
 * the tile's slice of the distributed dense vector.  In place.
 * CBG_OP_MIN and CBG_OP_MAX are the reference's minimum and maximum (Operations.h:153-179):
 * x < v ? x : v and x < v ? v : x with x the matrix value and v the vector's, not fmin / fmax.
 * Where the comparison is false -- either side NaN, +0.0 against -0.0 -- MIN returns the
 * vector's value and MAX the matrix value, bit for bit. */
enum { CBG_DIM_COLUMN = 0, CBG_DIM_ROW = 1 };
enum { CBG_OP_MULTIPLIES = 0, CBG_OP_PLUS = 1, CBG_OP_MIN = 2, CBG_OP_MAX = 3 };
int cbg_tile_dim_apply(cbg_tile* t, int dim, const double* vec, int op);
/* Restriction operator of the Galerkin driver (mfiles/genrestrict.m:11,
 * sprand(n, n/order, order/n)): n x n/order, Poisson(1) nonzeros per fine row
 * (~37 % of the rows empty) in uniform coarse columns (Poisson(order) per
 * column), values in (0,1]; counts, columns and values from a counter-based
 * hash of (seed, row), a column drawn twice in a row summed, so every grid
 * shape sees the same global T.  Tile (prow,pcol) of the pr x pc block
 * distribution. */
int cbg_restriction_tile(int scale, int order, uint64_t seed, int pr, int pc, int prow, int pcol, cbg_tile* out);
/* Test inputs with random values: every nonzero (i, j) of the
 * tile, at global row i + row_off and column j + col_off, gets a value
 * U[-1, 1) from a counter hash of (seed, column, row) (exact in double; the
 * structure is kept).  In place. */
int cbg_tile_random_values(cbg_tile* t, uint64_t seed, int64_t row_off, int64_t col_off);

/* ---------------- generator ---------------- */
/* Graph500 Kronecker R-MAT as DistEdgeList::GenGraph500Data(packed, scrambled)
 * (DistEdgeList.cpp:223-280, RefGen21.h:73-318) -> SpParMat(DEL,false)
 * (SpParMat.cpp:3140-3254) -> RemoveLoops (SpParMat.cpp:3257-3272), on device.
 * Produces the tile of grid cell (prow,pcol) of a pr x pc grid (1x1: whole matrix). */
int cbg_rmat_tile(int scale, int edgefactor, uint64_t userseed, int pr, int pc, int prow, int pcol,
                  cbg_tile* out);

/* ---------------- local multiply ---------------- */
/* LocalHybridSpGEMM (mtSpGEMM.h:212-460) + SpDCCols(SpTuples) (SpDCCols.cpp:108-190):
 * C = A*B on the semiring, C as a device DCSC tile (columns where C has nonzeros,
 * rows ascending, explicit zeros kept).  A, B device tiles.  stream may be NULL. */
int cbg_local_spgemm(const cbg_tile* A, const cbg_tile* B, int semiring, cbg_tile* C, void* hip_stream);
/* estimateFLOP + estimateNNZ_Hash (mtSpGEMM.h:1056-1134, 805-933): totals only */
int cbg_local_symbolic(const cbg_tile* A, const cbg_tile* B, int64_t* flops, int64_t* nnz, void* hip_stream);
/* MergeAll / MultiwayMerge (Friends.h:657-741, MultiwayMerge.h:409-526) of
 * column-sorted device tiles of equal shape, summing duplicates with SR::add. */
int cbg_merge(const cbg_tile* parts, int nparts, int semiring, cbg_tile* C, void* hip_stream);
/* last call's local-multiply statistics (summed over its multiplies): flops, nnz,
 * per-phase device ms, big columns, slabs.  Merges are not counted here. */
int cbg_last_stats(int64_t* flops, int64_t* nnz, double* ms_symbolic, double* ms_numeric, int64_t* n_big,
                   int64_t* n_slabs);
/* ... and the work of each kernel family (summed over the call's multiplies), so a
 * test can prove which code paths ran: numeric slabs per launch class (bitmap
 * slabs with kept symbolic bitmaps / with the marking pass, hash slabs by table
 * size 512 ... 8192, rank slabs of <= 1024 / 2048 / 4096 nonzeros), symbolic
 * (column, panel) units and panel-group units, group units run panel by panel,
 * columns of the one-pass small-column kernels, thin columns, entries of the
 * single-entry big columns, columns of the numeric hash / wave bins, and the
 * multiplies whose slab kernels accumulated exact integers in int32 (A's and B's
 * values integers of magnitude <= 2^24 whose sums stay below 2^31), and the flops
 * above which a column took the big-column path.
 * counts[i] for i < min(n, CBG_WORK_N); returns CBG_WORK_N. */
enum {
  CBG_WORK_BITMAP_SMALL_KEPT = 0,
  CBG_WORK_BITMAP_SMALL_MARK = 1,
  CBG_WORK_BITMAP_LARGE_KEPT = 2,
  CBG_WORK_BITMAP_LARGE_MARK = 3,
  CBG_WORK_HASH0 = 4, /* + k: tables of 512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192 slots */
  CBG_WORK_RANK0 = 13, /* + k: rank slabs of <= 1024, 2048, 4096 nonzeros */
  CBG_WORK_SYM_PANEL_UNITS = 16,
  CBG_WORK_SYM_GROUP_UNITS = 17,
  CBG_WORK_SYM_DEFERRED_UNITS = 18,
  CBG_WORK_ESC_COLUMNS = 19,
  CBG_WORK_THIN_COLUMNS = 20,
  CBG_WORK_SINGLE_BIG_ENTRIES = 21,
  CBG_WORK_HASH_BIN_COLUMNS = 22,
  CBG_WORK_WAVE_BIN_COLUMNS = 23,
  CBG_WORK_IACC = 24, /* multiplies whose slabs accumulated exact integers in int32 */
  CBG_WORK_GRANK0 = 25, /* + k: panel-group rank slabs of <= 2048, 4096 nonzeros */
  CBG_WORK_BIG_CUT = 27, /* the big-column cut in flops (4096, or 1024 where the multiply's rule or
                          * CBG_BIG_FLOPS lowered it): not summed, the call's last multiply's */
  /* The A-side preparation one MemEfficientSpGEMM / PANEL SUMMA call keeps for its
   * multiplies (all of the same A): which of them each multiply took from that cache
   * and which it built.  Each counts multiplies. */
  CBG_WORK_AMAP_REUSED = 28,  /* reused the cached column map of A */
  CBG_WORK_PMAP_REUSED = 29,  /* reused the cached panel map */
  CBG_WORK_PMAP_BUILT = 30,   /* built the full panel map (kept for the call's later multiplies) */
  CBG_WORK_PMAP_ENTRIES = 31, /* built a private panel map of the A columns their big columns reference */
  CBG_WORK_AVALS_REUSED = 32, /* had big columns and took A's value verdicts and copies from the cache */
  CBG_WORK_RVD_BUILT = 33,    /* packed A's (row, f64) records */
  CBG_WORK_RVD_USED = 34,     /* had slab kernels read the (row, f64) records (packed now or cached) */
  /* Staged runs: the big columns' symbolic writes every B entry's run of A(:,k) inside each
   * panel of its bitmap-mode (column, panel) pairs, and the numeric's bitmap slabs read them
   * instead of hopping through A's panel map (all or nothing per multiply; CBG_STAGE_RUNS=0
   * keeps the hops). */
  CBG_WORK_STAGED_MULTIPLIES = 35, /* multiplies that used staged runs */
  CBG_WORK_STAGED_ENTRIES = 36,    /* B entries x panels of the pairs whose bitmap slabs read them */
  /* bitmap slabs the symbolic planned beyond the cap of the slab kernels the numeric was about
   * to launch: the library's own check, always 0 (a multiply that counts one fails with
   * CBG_ERR_INTERNAL before any slab kernel starts) */
  CBG_WORK_SLAB_OVER_CAP = 37,
  CBG_WORK_N = 38
};
int cbg_last_work_stats(int64_t* counts, int n);
/* The two thresholds of that preparation: bounds[0] = E, a multiply maps only the A
 * columns its big columns reference when their B entries x E < A's nonempty columns;
 * bounds[1] = F, the (row, f64) records are packed by the first multiply whose big
 * columns carry >= F x nnz(A) flops.  Writes min(n, 2) values, returns 2. */
int cbg_local_aprep_bounds(int64_t* bounds, int n);
/* The most nonzeros of a bitmap slab in its two launch classes: out[0], out[1] the small
 * and the large class where the slabs accumulate f64 values, out[2], out[3] where they
 * accumulate exact integers in int32 (CBG_WORK_IACC).  Returns 0. */
int cbg_local_slab_caps(int out[4]);
/* last call's multiway merges (MergeAll / MultiwayMerge): partial entries in,
 * merged entries out, device ms */
int cbg_merge_stats(int64_t* entries_in, int64_t* entries_out, double* ms);
/* last PANEL SUMMA call's double buffering: B-column pieces multiplied (1 = the
 * broadcast was not pipelined), measured broadcast ms of the first piece, the
 * estimated broadcast ms of the rest that pipelining would hide, and the ms an
 * extra piece is taken to cost: max(CBG_PIPELINE_MIN_MS (3), CBG_PIPELINE_COST_FRAC
 * (0.04) x the previous such call's local multiply ms); pipelined when the
 * hidden ms exceed the cost on some rank */
int cbg_last_summa_info(int* pieces, double* bcast_ms_piece0, double* est_hidden_ms, double* piece_cost_ms);
/* ... and its communication: the double-buffering rule applied (0 one piece,
 * 1 pipelined because the B block column has > 1 remote tile on an RCCL grid,
 * 2 adaptive and pipelined, 3 adaptive and rejoined, 4 a fixed pipeline of
 * several pieces: CBG_PIPELINE or phases given as pieces), the bytes of the remote
 * A and B tiles this rank received, and the exposed communication: the summed
 * ms the compute stream waited for broadcasts (HIP events around each wait) */
int cbg_last_summa_comm(int* rule, int64_t* bytes_recv, double* exposed_comm_ms);

/* ---------------- 2D SUMMA over RCCL ---------------- */
typedef struct cbg_grid cbg_grid;
#define CBG_UNIQUE_ID_BYTES 128
/* ncclGetUniqueId: called by rank 0, bytes shipped to the others by the host */
int cbg_get_unique_id(void* id);
/* CommGrid(MPI_COMM_WORLD, rows, cols) (CommGrid.cpp:37-75): rows=cols=0 => square
 * grid or CBG_ERR_NOTSQUARE; rank r -> (r / cols, r % cols); row/col
 * communicators via ncclCommSplit.  One process (rank) per GPU. */
int cbg_grid_create(int rank, int nranks, int grid_rows, int grid_cols, const void* unique_id, cbg_grid** out);
/* host-transport grid for testing the SUMMA logic with several processes on
 * one GPU: collectives are delegated to host callbacks (e.g. gloo). */
typedef struct cbg_host_comm {
  /* comm: 0 = world, 1 = row communicator, 2 = column communicator; root is the
   * rank inside that communicator; buf is HOST memory */
  int (*bcast)(void* user, int comm, void* buf, size_t bytes, int root);
  int (*allgather)(void* user, int comm, const void* in, void* out, size_t bytes_each);
  void* user;
} cbg_host_comm;
int cbg_grid_create_host(int rank, int nranks, int grid_rows, int grid_cols, const cbg_host_comm* comm,
                         cbg_grid** out);
int cbg_grid_destroy(cbg_grid* g);
int cbg_grid_info(const cbg_grid* g, int* rank, int* nranks, int* grid_rows, int* grid_cols, int* prow, int* pcol);
/* world-communicator helpers used by drivers for barrier + max-over-ranks timing */
int cbg_grid_barrier(cbg_grid* g);
/* collective error agreement (no reference counterpart: the reference MPI_Aborts,
 * SpDefs.h:69-76): *agreed = max over the grid's ranks of local_rc.  Every
 * collective entry point below runs it after each of its steps, so a failure on
 * one rank (CBG_ERR_OOM in its local multiply, a bad argument) is returned by
 * every rank instead of leaving the others blocked in a broadcast.  An RCCL
 * async error, or no progress for CBG_COMM_TIMEOUT_S seconds (default 600),
 * aborts the grid's communicators (ncclCommAbort): later calls on that grid
 * return CBG_ERR_RCCL. */
int cbg_grid_agree(cbg_grid* g, int local_rc, int* agreed);
int cbg_grid_allreduce_max(cbg_grid* g, double* value);
int cbg_grid_allreduce_sum_i64(cbg_grid* g, int64_t* value);

/* Mult_AnXBn_DoubleBuff / Mult_AnXBn_Synch (ParFriends.h:798-1108):
 * collective over the grid; A_local/B_local are this rank's device tiles of
 * the block distribution (SpParMat::Owner, SpParMat.cpp:5068-5097).
 * A_gncol/B_gnrow are the global inner dimensions (CheckSpGEMMCompliance).
 * A and B are left unchanged (the reference mutates and restores them).
 * C_local receives this rank's tile C(prow,pcol). */
int cbg_summa_spgemm(cbg_grid* g, const cbg_tile* A_local, const cbg_tile* B_local, int64_t A_gncol,
                     int64_t B_gnrow, int semiring, int algo, int exec, cbg_tile* C_local);

/* MemEfficientSpGEMM (ParFriends.h:449-730) without its Markov-clustering
 * pruning (with it: cbg_summa_spgemm_mcl below): this rank's B tile is cut into `phases` column pieces
 * (SpDCCols::ColSplit, SpDCCols.cpp:936-970: cuts at (i+1)*(n/phases)), each
 * piece goes through the SUMMA above, and the phase results are
 *   fn == NULL: column-concatenated on device into C_local
 *               (SpDCCols::ColConcatenate, ParFriends.h:724-725);
 *   fn != NULL: handed to fn(user, phase, col_offset, C_phase) one at a time
 *               and freed after the call (C streamed when it does not fit HBM;
 *               C_local may be NULL).  fn runs on every rank between the
 *               collectives; a nonzero return is reported after all phases.
 *               fn may be called SEVERAL times per phase, each time with a
 *               column piece of that phase's C at its own col_offset: with
 *               phases == 1 and EXEC_PANEL the SUMMA's pipeline pieces are
 *               handed over one by one (phase 0 each), and with EXEC_PANEL a
 *               phase whose C does not fit the device after all is computed as
 *               column halves of its B piece (same phase index).  With
 *               EXEC_STAGED such a phase fails with CBG_ERR_OOM.
 * phases < 1 or >= A_gncol is reset to 1 (ParFriends.h:468-473).  Every rank needs
 * B_local->n >= phases (CBG_ERR_INVALIDPARAMS otherwise, collectively). */
typedef int (*cbg_phase_fn)(void* user, int phase, int64_t col_offset, const cbg_tile* C_phase);
int cbg_summa_spgemm_phased(cbg_grid* g, const cbg_tile* A_local, const cbg_tile* B_local, int64_t A_gncol,
                            int64_t B_gnrow, int semiring, int algo, int exec, int phases, cbg_phase_fn fn,
                            void* user, cbg_tile* C_local);
/* The same with MemEfficientSpGEMM's perProcessMemory (GB, ParFriends.h:482-535):
 * when per_process_memory_gb > 0, or phases == CBG_PHASES_AUTO (this library's
 * extension: the device's free memory), the phase count comes from memory: the flops of this rank's product (from the column counts of A's tiles
 * and the row counts of B's tiles, allgathered along the grid row / column), an
 * nnz(C) estimate (flops, times the compression of an exact symbolic of a sample
 * of the product when the flops bound asks for more than one phase), and 60 % of
 * the memory left after the tiles the SUMMA gathers -- perProcessMemory, or the device's free memory when it is 0;
 * the maximum over the grid.  If that memory is already taken by the inputs the
 * given phases are kept, like the reference. */
#define CBG_PHASES_AUTO (-1)
int cbg_summa_spgemm_memeff(cbg_grid* g, const cbg_tile* A_local, const cbg_tile* B_local, int64_t A_gncol,
                            int64_t B_gnrow, int semiring, int algo, int exec, int phases,
                            int64_t per_process_memory_gb, cbg_phase_fn fn, void* user, cbg_tile* C_local);
/* the last (memeff / phased) call's phase plan: phases run, whether they were
 * chosen from memory, this rank's product flops and estimated nnz(C), the C bytes
 * a phase was allowed, phases split in halves after an out-of-memory, and the
 * host ms the planning took */
int cbg_last_phase_plan(int* phases, int* automatic, int64_t* flops, int64_t* nnz_est, double* c_budget_bytes,
                        int* oom_splits, double* plan_ms);

/* ---------------- Markov-clustering pruning (HipMCL) ---------------- */
/* MCLPruneRecoverySelect (ParFriends.h:186-353) on device.  Every decision is per
 * GLOBAL column j of the distributed matrix, over the row blocks of its grid column:
 *   1. cnt0[j] = #{v > h}, sum0[j] = their sum, all[j] = nnz of the column; thr[j] = h;
 *   2. recovery: columns with cnt0 < R, all > cnt0 and sum0 < q get thr = kth(j, R);
 *   3. if S > 0: the other columns with cnt0 > S get thr = kth(j, S); if also R > 0,
 *      those of them whose count and sum of the kept values (!(v < thr)) are < R and
 *      < q get thr = kth(j, R);
 *   4. v is kept iff !(v < thr[j]); emptied columns leave jc.
 * kth(j, k) is the k-th largest value of the unpruned column, duplicates counted
 * (SpParMat::Kselect1, SpParMat.cpp:1413-1739), its smallest value when it has fewer
 * than k entries: ties with the k-th value are all kept.  -0.0 and +0.0 compare equal
 * (a k-th value of zero is returned as +0.0); the result for a column that holds a
 * NaN is unspecified.  kselectVersion has no counterpart (one exact algorithm). */
typedef struct cbg_mcl_params {
  double hard_threshold;
  int64_t select_num, recover_num;
  double recover_pct;
} cbg_mcl_params;
/* Column statistics of a device tile: cnt[j] / sum[j] = number / sum of the values of
 * local column j kept under thr[j] (strict: 1 keeps v > thr, 0 keeps !(v < thr)); 0 for
 * empty columns.  thr, cnt, sum are HOST arrays of t->n entries.  The order of a
 * column's sum depends on its length alone (bit-reproducible). */
int cbg_tile_col_stats(const cbg_tile* t, const double* thr, int strict, int64_t* cnt, double* sum);
/* SpParMat::PruneColumn(pvals, less<>) (SpParMat.cpp) on one tile: out keeps the
 * entries with !(v < thr[column]), values copied; thr: HOST array of t->n entries */
int cbg_tile_prune_column(const cbg_tile* t, const double* thr, cbg_tile* out);
/* SpParMat::Kselect1, collective along the grid column (every rank of the grid calls
 * it; the ranks of a grid column list the same columns): kth[i] = the k-th largest
 * value of local column cols[i] over the grid column's row blocks (the smallest when
 * the column has fewer than k entries, 0.0 when it is empty).  cols: distinct local
 * column ids (HOST), kth: HOST out.  k >= 1. */
int cbg_grid_kselect(cbg_grid* g, const cbg_tile* local, const int32_t* cols, int64_t ncols, int64_t k, double* kth);
/* MCLPruneRecoverySelect of the distributed matrix whose tile is `local`; out = this
 * rank's pruned tile.  select_num < 0, recover_num < 0 or a NaN parameter:
 * CBG_ERR_INVALIDPARAMS.  p == NULL or every parameter <= 0: out is a copy. */
int cbg_grid_mcl_prune(cbg_grid* g, const cbg_tile* local, const cbg_mcl_params* p, cbg_tile* out);
/* cbg_summa_spgemm_memeff with every delivered column piece of C pruned
 * (MCLPruneRecoverySelect, ParFriends.h:698) before it is concatenated or handed to
 * fn (same phase and col_offset).  p == NULL or every parameter <= 0: no pruning,
 * the result of cbg_summa_spgemm_memeff (the reference would drop negative values
 * at a zero threshold). */
int cbg_summa_spgemm_mcl(cbg_grid* g, const cbg_tile* A_local, const cbg_tile* B_local, int64_t A_gncol,
                         int64_t B_gnrow, int semiring, int algo, int exec, int phases,
                         int64_t per_process_memory_gb, cbg_phase_fn fn, void* user, cbg_tile* C_local,
                         const cbg_mcl_params* p);
/* upper column length of each k-select kernel class but the last (a wave's registers,
 * a block's LDS in two sizes; longer columns are streamed): bounds[i] for
 * i < min(n, 3); returns 3 */
int cbg_mcl_kselect_bounds(int64_t* bounds, int n);
/* the last pruning call's work, summed over its pieces: entries in / out, columns
 * recovered, selected, recovered after selection, pieces pruned, columns run by each
 * k-select class (for grid columns of several ranks: of the union pass).
 * counts[i] for i < min(n, CBG_MCL_N); ms (may be NULL): CBG_MCL_MS_N device times
 * (statistics, k-select, compaction).  Returns CBG_MCL_N. */
enum {
  CBG_MCL_ENTRIES_IN = 0,
  CBG_MCL_ENTRIES_OUT = 1,
  CBG_MCL_COLS_RECOVERED = 2,
  CBG_MCL_COLS_SELECTED = 3,
  CBG_MCL_COLS_RECOVERED_AFTER = 4,
  CBG_MCL_PIECES = 5,
  CBG_MCL_KSELECT_CLASS0 = 6, /* + c: wave, LDS small, LDS large, streamed */
  CBG_MCL_N = 10
};
enum { CBG_MCL_MS_STATS = 0, CBG_MCL_MS_KSELECT = 1, CBG_MCL_MS_COMPACT = 2, CBG_MCL_MS_N = 3 };
int cbg_last_mcl_stats(int64_t* counts, int n, double* ms);

/* ---------------- HipMCL iteration (Applications/MCL.cpp:515-647) ---------------- */
/* SpParMat::Reduce(Column, op, id[, unop]) (SpParMat.cpp, as MCL.cpp:392-417 uses it),
 * collective along the grid column: out[j] (HOST, local->n doubles) = the sum, maximum,
 * sum of squares or count of local column j over the row blocks of its grid column.
 * An empty column gives `identity`; CBG_RED_MAX gives max(identity, values), as the
 * reference folds from id (the sums' id is 0.0 in every reference call: it only fills
 * empty columns here).  One pass over val yields all four (k_col_moments); a column's
 * sums depend on its length alone (the order of cbg_tile_col_stats) and the ranks'
 * partial results are added in rank order: the same bits in every run and on every
 * rank of the grid column.  The sums start from +0.0 (idle lanes add +0.0), so a column
 * whose values are all -0.0 sums to +0.0, where a host sum of its values gives -0.0. */
enum { CBG_RED_SUM = 0, CBG_RED_MAX = 1, CBG_RED_SUMSQ = 2, CBG_RED_COUNT = 3 };
int cbg_grid_reduce_cols(cbg_grid* g, const cbg_tile* local, int what, double identity, double* out);
/* upper column length of each column-moment kernel class but the last (16 lanes, a
 * wave; longer columns: a block): bounds[i] for i < min(n, 2); returns 2 */
int cbg_mcl_moment_bounds(int64_t* bounds, int n);
/* SpParMat::Apply (SpParMat.h Apply(unop)), in place on a device tile.  CBG_APPLY_POW is
 * exponentiate (Operations.h:140-143): arg == 2.0 is computed as v * v (exact; HipMCL's
 * default inflation), any other arg through the device pow. */
enum {
  CBG_APPLY_POW = 0,
  CBG_APPLY_SET = 1, /* v <- arg: the unit-valued copy that a bool matrix is in the reference (arg 1.0) */
  CBG_APPLY_RDIV = 2 /* v <- arg / v: bind1st(divides<double>(), arg) (BetwCent.cpp:192); arg / 0 = inf */
};
/* any other op, or a NaN arg: CBG_ERR_INVALIDPARAMS.  A compatibility rule: CBG_APPLY_SET and CBG_APPLY_RDIV
 * also refuse, with the same code and before any device work, a tile struct without its arrays (cp NULL, or
 * val NULL with nnz > 0).  Ops 1 and 2 were unknown before these functors existed, and callers that probed
 * "an unknown op" with such a struct keep their answer; CBG_APPLY_POW and the other entry points take the
 * struct as before.  Every device tile libcbg produces holds cp, an empty one too. */
int cbg_tile_apply(cbg_tile* t, int op, double arg);
/* MakeColStochastic (MCL.cpp:390-395), in place, collective along the grid column:
 * inv = (sum == 0) ? DBL_MAX : 1.0 / sum (safemultinv, Operations.h:103-110), then
 * v * inv: two roundings, like the reference (not v / sum). */
int cbg_grid_make_col_stochastic(cbg_grid* g, cbg_tile* local);
/* Chaos (MCL.cpp:408-421): the maximum over the columns of (max(0, values) - sumsq) *
 * count, folded from 0, then the maximum over the grid.  Collective over the grid. */
int cbg_grid_chaos(cbg_grid* g, const cbg_tile* local, double* chaos);
/* The iteration's step after the expansion (MCL.cpp:591-611: MakeColStochastic, Chaos,
 * Inflate, MakeColStochastic) in three passes over val: 1. column sums; 2. v <- v * inv,
 * the chaos moments of the scaled values, w = pow(v, power) written back and the column
 * sums of w; 3. w <- w * inv2; one grid-column combine of the per-column arrays after
 * passes 1 and 2.  The tile and *chaos are bit-identical to cbg_grid_make_col_stochastic,
 * cbg_grid_chaos, cbg_tile_apply(CBG_APPLY_POW, power), cbg_grid_make_col_stochastic. */
int cbg_grid_inflate(cbg_grid* g, cbg_tile* local, double power, double* chaos);
/* device ms of the last cbg_grid_inflate's three passes on this rank (with several
 * ranks in a grid column, passes 1 and 2 include the combine) and the entries they ran over */
int cbg_last_inflate_stats(double* ms3, int64_t* nnz);

/* SpParMat::RemoveLoops / AddLoops(FullyDistVec, replaceExisting) (SpParMat.cpp:3257-3335,
 * SpTuples.h:113-228) of the gm x gn distributed matrix whose tile is `local`; out = this
 * rank's new tile (rows ascending, columns that become nonempty enter jc, emptied ones
 * leave).  The tile's place comes from the grid (SpParMat::Owner, SpParMat.cpp:5068-5097),
 * so on a non-square grid the off-diagonal tiles the diagonal crosses are handled too
 * (the reference touches the diagonal processors only).  gm != gn: CBG_ERR_DIMMISMATCH.
 * *removed (may be NULL): the loops removed over the whole grid.  loopvals: HOST array of
 * local->n values, the loop of each local column; replace_existing as the reference's. */
int cbg_grid_remove_loops(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, cbg_tile* out,
                          int64_t* removed);
int cbg_grid_add_loops(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, const double* loopvals,
                       int replace_existing, cbg_tile* out);
/* AdjustLoops (MCL.cpp:464-474): RemoveLoops, colmaxs = Reduce(Column, max,
 * numeric_limits<double>::min()), AddLoops(colmaxs).  The reference's quirk is kept: the
 * Apply at :469 that would turn the isolated vertices' numeric_limits::min() into 1.0
 * acts on A (where it changes a stored value equal to min() only), not on colmaxs, so
 * the loop of an empty column is numeric_limits<double>::min(); MakeColStochastic then
 * makes it 1.0 (min() * (1 / min()) is exact). */
int cbg_grid_adjust_loops(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, cbg_tile* out);

/* Interpret (MCL.cpp:373-386) with the reference's CC: the connected components of the
 * gn x gn distributed matrix, every stored entry (i, j) an undirected edge (the
 * components of A + A^T without building it).  Min-label hooking over the tile's
 * entries and pointer jumping on a dense label vector of gn entries per rank, one
 * grid-wide minimum per round, until a round changes nothing (more than gn rounds:
 * CBG_ERR_NOTSUPPORTED).  labels (HOST, gn int64, the same on every rank): labels[v] =
 * the rank of v's component when the components are ordered by their smallest vertex
 * (this library's convention: the reference's numbering follows LACC's internals).
 * *ncomponents (may be NULL) their number. */
int cbg_grid_connected_components(cbg_grid* g, const cbg_tile* local, int64_t gn, int64_t* labels,
                                  int64_t* ncomponents);

/* HipMCL() (MCL.cpp:515-647), one layer: AdjustLoops, MakeColStochastic, the optional
 * pre-pruning (MCLPruneRecoverySelect), then while chaos > eps: A <- A * A with every
 * piece pruned (cbg_summa_spgemm_mcl), cbg_grid_inflate; finally the connected
 * components.  A stays on the device throughout.  RemoveIsolated and RandPermute
 * (MCL.cpp:477-512) run before it in cbg_grid_hipmcl_prepared below; the 3D layers need a
 * third grid dimension: out of scope.  The squaring multiplies A by a device copy of
 * itself (one copy per iteration): the public SUMMA's refusal of aliased operands stays. */
typedef struct cbg_hipmcl_params {
  double inflation;        /* > 0 */
  cbg_mcl_params prune;    /* hardThreshold, selectNum, recoverNum, recoverPct */
  int32_t phases;          /* as cbg_summa_spgemm_memeff */
  int32_t algo, exec;      /* CBG_DOUBLEBUFF / CBG_SYNCH, CBG_EXEC_PANEL / CBG_EXEC_STAGED */
  int32_t preprune;        /* -1: the reference's rule nnz / nv > max(S, R) (MCL.cpp:531-538); 0, 1: forced */
  int64_t per_process_memory_gb;
  double eps;              /* <= 0: 1e-4 (EPS, MCL.cpp:55) */
  int64_t max_iterations;  /* this library's extension; 0: unlimited, like the reference.  At the cap the
                              call returns CBG_OK: *iterations and the last chaos tell */
} cbg_hipmcl_params;
/* called once per iteration on every rank, after its inflation */
typedef void (*cbg_hipmcl_iter_fn)(void* user, int64_t iter, double chaos, int64_t nnz, double ms_expand,
                                   double ms_prune, double ms_inflate);
/* final_local (may be NULL): this rank's tile of the converged matrix; labels (may be
 * NULL), *nclusters, *iterations (may be NULL): as cbg_grid_connected_components.
 * A NaN or non-positive inflation, negative max_iterations or pruning parameters:
 * CBG_ERR_INVALIDPARAMS before any device work. */
int cbg_grid_hipmcl(cbg_grid* g, const cbg_tile* A_local, int64_t gn, const cbg_hipmcl_params* params,
                    cbg_hipmcl_iter_fn fn, void* user, cbg_tile* final_local, int64_t* labels, int64_t* nclusters,
                    int64_t* iterations);
/* the last cbg_grid_hipmcl: iterations, the last chaos, the global nnz of the final
 * matrix, and this rank's summed ms of the expansions (multiply and pruning), of the
 * pruning inside them (device ms) and of the inflations */
int cbg_last_hipmcl_stats(int64_t* iterations, double* chaos, int64_t* final_nnz, double* ms_expand,
                          double* ms_prune, double* ms_inflate);

/* ---------------- sparse indexing (SpRef) ---------------- */
/* SpDCCols::operator()(ri, ci) (SpDCCols.cpp:1355-1383) on one device tile:
 * out is nri x nci, out(i, j) = t(ri[i], ci[j]); stored entries only, values copied bit for bit
 * (explicit zeros, -0.0, NaN payloads kept), rows ascending in every column, empty columns not in jc.
 * ri / ci: HOST int64 arrays; indices may repeat and may be left out.
 * ri == NULL: all rows in order (nri ignored); ci == NULL likewise.
 * (The reference spells "all" as an empty vector; here a non-NULL vector of length 0 gives an extent of 0.)
 * An index outside the tile or a negative count: CBG_ERR_INVALIDPARAMS before any device work. */
int cbg_tile_spref(const cbg_tile* t, const int64_t* ri, int64_t nri, const int64_t* ci, int64_t nci, cbg_tile* out);

/* SpParMat::SubsRef_SR (SpParMat.cpp:2026-2247), collective over the grid, any pr x pc:
 * the gm x gn distributed matrix whose tile is `local` -> this rank's tile of the nri x nci matrix
 * B(i, j) = A(ri[i], ci[j]) in the standard block layout (SpParMat::Owner).
 * ri / ci: HOST, GLOBAL indices, the same arrays on every rank (as `labels` of
 * cbg_grid_connected_components); NULL = all.
 * The reference multiplies by two boolean selection matrices (P * A * Q); here the entries
 * are moved: the requested columns are gathered along the grid row first (whole columns, no
 * sort), then the rows are relabelled along the grid column through the inverse of ri and
 * every column is sorted by row -- not at all when ri is strictly increasing.
 * An index below 0 or at or above its extent (the reference's own check, SpParMat.cpp:2051,
 * lets the extent itself pass), a negative count, a NULL out, or gm / gn that do not fit the
 * tile's place in the grid: CBG_ERR_INVALIDPARAMS on every rank before any device work.
 * A new local block of 2^31 or more rows or columns: CBG_ERR_NOTSUPPORTED. */
int cbg_grid_spref(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, const int64_t* ri, int64_t nri,
                   const int64_t* ci, int64_t nci, cbg_tile* out);

/* ---------------- sparse element-wise ops ---------------- */
/* EWiseMult / SetDifference of two tiles (Friends.h:744-1030, SpDCCols.cpp:631-690; SpParMat's
 * EWiseMult, SpParMat.cpp:2781-2812, is this on every rank's pair of tiles). */
enum {
  CBG_EWISE_MULT = 0,   /* EWiseMult(A, B, false): stored in both; value a * b (one rounding) */
  CBG_EWISE_FIRST = 1,  /* the same structure; value a, bit for bit (B is a mask: the reference's
                           EWiseMult with a bool-valued B, as BetwCent uses its bfs levels) */
  CBG_EWISE_EXCLUDE = 2 /* SetDifference / EWiseMult(A, B, true): stored in A and not in B;
                           value a, bit for bit */
};
/* a, b: device tiles of equal m x n (else CBG_ERR_DIMMISMATCH); a == b is allowed.  An unknown
 * op, or a NULL a or out: CBG_ERR_INVALIDPARAMS before any device work.  b == NULL or an empty b:
 * the empty tile for MULT / FIRST, a copy of a for EXCLUDE.  out is valid DCSC (rows ascending, a
 * column left with no entry leaves jc, 64-bit offsets); explicit zeros, -0.0 and NaN payloads of
 * a survive FIRST and EXCLUDE unchanged.
 * The work unit is a (stored column of a, chunk of at most C of its entries), so a few very
 * long columns still fill the device.  A unit searches b's column for the rows its chunk
 * spans and matches inside that range: in LDS where the range holds at most L row ids, else by
 * a binary search per entry in global memory. */
int cbg_tile_ewise(const cbg_tile* a, const cbg_tile* b, int op, cbg_tile* out);
/* bounds[0] = C, bounds[1] = L for i < min(n, 2); returns 2 */
int cbg_ewise_bounds(int64_t* bounds, int n);
/* the last cbg_tile_ewise on this thread: entries of a, of b and of out, units, and the units of
 * each matching class (nothing of b in the chunk's rows, matched in LDS, matched in global
 * memory).  counts[i] for i < min(n, CBG_EWISE_N); *ms (may be NULL): ms between two device events
 * around the call's kernels.  That span holds the one host readback in the middle (the totals, before
 * the output is allocated), so it is the op's time on the stream, not the sum of its kernels' times.
 * A call answered without a kernel (an empty operand) has no units.  After cbg_grid_betwcent the
 * figures are SUMS over all the element-wise calls that run made (it resets them at its start).
 * Returns CBG_EWISE_N. */
enum {
  CBG_EWISE_ENTRIES_A = 0,
  CBG_EWISE_ENTRIES_B = 1,
  CBG_EWISE_ENTRIES_OUT = 2,
  CBG_EWISE_UNITS = 3,
  CBG_EWISE_CLASS0 = 4, /* + c: no range, LDS, global */
  CBG_EWISE_N = 7
};
int cbg_last_ewise_stats(int64_t* counts, int n, double* ms);

/* ---------------- batched betweenness centrality (Applications/BetwCent.cpp:148-217) ---------------- */
/* Brandes' algorithm as a breadth-first search over a matrix of frontiers, `batch` roots at a time
 * (the last batch may be shorter, down to the number of the grid's columns; the reference rounds the
 * count instead).  A(i, j) stored = an edge
 * i -> j of the gn-vertex graph; stored values are ignored (every stored entry is `true`): the loop
 * works on unit-valued copies without loops (CBG_APPLY_SET, cbg_grid_remove_loops).  Dropping the
 * loops is this library's deviation: the reference lets a root's loop put the root into its own
 * first fringe.  AT_local: A's transpose in the same layout; NULL on a square grid: cbg_grid_transpose;
 * NULL on any other grid: CBG_ERR_NOTSQUARE.  roots: HOST, nroots distinct global vertex ids below gn,
 * the same on every rank; a repeated or outside one, batch < 1, a bad algo / exec or a NULL bc:
 * CBG_ERR_INVALIDPARAMS on every rank before any device work.  A batch's columns are spread over the
 * grid's columns, and every grid column needs at least one: a batch with fewer roots than the grid has
 * columns -- the last one, of nroots % batch roots, is the narrowest -- is refused the same way (on a
 * 1 x 1 or pr x 1 grid every batch passes; on a grid of pc columns choose nroots % batch == 0 or >= pc).
 * Per batch: fringe = AT(:, batch) (cbg_grid_spref); nsp = 1 at (root k, column k); while the fringe
 * is non-empty over the grid: nsp += fringe, the fringe is kept as that level, fringe = AT * fringe
 * (the SUMMA, CBG_PLUS_TIMES), fringe = fringe without nsp's positions (CBG_EWISE_EXCLUDE).  Then
 * nspInv = 1 / nsp, a dense block bcu of ones, and from the last level down to level 1:
 * w = nspInv at that level's positions times bcu there, product = A * w masked by the level before
 * and multiplied by nsp, bcu += product.  bc += row sums of bcu (summed along the batch in column
 * order, the partial sums of a grid row's ranks added in rank order); after the last batch
 * bc -= nroots.  Path counts are doubles: exact below 2^53 (the reference's int overflows at 2^31).
 * fn (may be NULL): called on every rank once per level with the batch's index, the level (from 1)
 * and the fringe's entries over the whole grid.  bc: HOST, gn doubles, the same on every rank. */
typedef struct cbg_betwcent_params {
  int64_t batch;
  int32_t algo, exec;
} cbg_betwcent_params;
typedef void (*cbg_betwcent_level_fn)(void* user, int64_t batch, int64_t level, int64_t fringe_nnz);
int cbg_grid_betwcent(cbg_grid* g, const cbg_tile* A_local, const cbg_tile* AT_local, int64_t gn,
                      const int64_t* roots, int64_t nroots, const cbg_betwcent_params* p, cbg_betwcent_level_fn fn,
                      void* user, double* bc);
/* the last cbg_grid_betwcent on this rank: batches, levels (summed over the batches), the deepest
 * level, fringe entries (over the grid, summed over the levels); ms (may be NULL, CBG_BC_MS_N host
 * times): forward multiplies, element-wise ops, backward multiplies, dense ops, total.
 * counts[i] for i < min(n, CBG_BC_N); returns CBG_BC_N. */
enum { CBG_BC_BATCHES = 0, CBG_BC_LEVELS = 1, CBG_BC_DEEPEST = 2, CBG_BC_FRINGE_ENTRIES = 3, CBG_BC_N = 4 };
enum { CBG_BC_MS_FORWARD = 0, CBG_BC_MS_EWISE = 1, CBG_BC_MS_BACKWARD = 2, CBG_BC_MS_DENSE = 3, CBG_BC_MS_TOTAL = 4,
       CBG_BC_MS_N = 5 };
int cbg_last_betwcent_stats(int64_t* counts, int n, double* ms);

/* ---------------- single-source breadth-first search ----------------
 * Applications/TopDownBFS.cpp:427-443 and DirOptBFS.cpp:360-445: the parent tree of a search from one root
 * with SpMV<SelectMaxSRing<bool,int64>> (Semirings.h:190-210), pushing (top-down) or pulling (bottom-up).
 *
 * ORIENTATION: the reference's y = A x.  A stored A(i, j) is the edge j -> i, and column j lists what j
 * reaches.  This is the TRANSPOSE of what cbg_grid_betwcent calls A (there a stored A(i, j) is i -> j).
 * Stored values are ignored: every stored entry, an explicit zero included, is `true`.
 *
 * SpMXSpV with SelectMaxSRing<bool,int64> (SpImpl.cpp:168-221) on one device tile: xind HOST, nx distinct
 * local column ids, ascending; xval HOST or NULL (NULL: indexisvalue, the value is the id).  yind / yval: HOST,
 * room for A->m; *ny entries, yind ascending.  y[i] = max over stored A(i, j), j in xind, of x[j].
 * An unsorted, repeated or outside xind, a negative count or a NULL output: CBG_ERR_INVALIDPARAMS before any
 * device work. */
int cbg_tile_spmspv_max(const cbg_tile* A, const int64_t* xind, const int64_t* xval, int64_t nx,
                        int64_t* yind, int64_t* yval, int64_t* ny);
/* the same product with xval == NULL, by pulling: At = cbg_tile_transpose(A); skip (HOST, At->n bytes, may be
 * NULL): rows with skip[i] != 0 are left out of y.  *entries_read (may be NULL): entries a serial descending scan
 * reads, the hit included (a row without a hit: its length). */
int cbg_tile_pull_max(const cbg_tile* At, const int64_t* xind, int64_t nx, const uint8_t* skip,
                      int64_t* yind, int64_t* yval, int64_t* ny, int64_t* entries_read);
/* bounds[0] = C, the entries of a frontier column one push unit takes; bounds[1] = the longest row the pull
 * scans with one lane (longer rows take a wave each, 64 entries per step from the end).
 * bounds[i] for i < min(n, 2); returns 2 */
int cbg_bfs_bounds(int64_t* bounds, int n);

/* The search, collective over any pr x pc grid.  A_local: this rank's tile of the gn x gn matrix.
 * parents / levels (levels may be NULL): HOST, gn int64, the same on every rank: parents[root] = root (as
 * DirOptBFS.cpp:371), parents[v] = the largest u of the level before with A(v, u) stored, -1 where the root
 * does not reach; levels[root] = 0, -1 where unreached.  max is exact and order-free: the same bits in
 * either direction, on every grid and transport.
 * Per step: push the frontier's columns of the local tile (atomic max per entry) or pull over the local
 * transpose (every parentless row scans its columns downward and stops at the first one in the frontier) into
 * a dense candidate array; maximum of the candidates, as global ids, over the grid row; new = candidate and no
 * parent yet; the new frontier's bits allgathered along the grid column.
 * direction CBG_BFS_AUTO, the reference's rule with nnz the stored entries over the grid: start pushing;
 * before a step, if pushing and pred > up_cutoff and the frontier grew, pull; after a pull step, if the new
 * frontier is smaller than down_cutoff and shrank, push.  pred = the summed column lengths of the frontier.
 * up_cutoff / down_cutoff < 0: nnz / 20 and (int64)(double(gn) * gn / (nnz * 12.0)) (0 when nnz = 0).
 * fn (may be NULL): called on every rank before every step with the step (from 1), the direction taken
 * (CBG_BFS_TOPDOWN or _BOTTOMUP), the frontier's size and its pred.  The last step finds nothing.
 * root outside [0, gn), a bad direction or a NULL parents: CBG_ERR_INVALIDPARAMS; a tile that is not this
 * rank's block of gn x gn (or an At_local that is not its transpose's shape): CBG_ERR_DIMMISMATCH; on every
 * rank before any device work. */
enum { CBG_BFS_AUTO = 0, CBG_BFS_TOPDOWN = 1, CBG_BFS_BOTTOMUP = 2 };
typedef struct cbg_bfs_params {
  int32_t direction;
  int64_t up_cutoff, down_cutoff; /* < 0: the reference's rule */
  const cbg_tile* At_local;       /* cbg_tile_transpose of A_local, or NULL: made at the first pull step, freed at the end */
} cbg_bfs_params;
typedef void (*cbg_bfs_level_fn)(void* user, int64_t level, int direction, int64_t frontier, int64_t pred);
int cbg_grid_bfs(cbg_grid* g, const cbg_tile* A_local, int64_t gn, int64_t root, const cbg_bfs_params* p,
                 cbg_bfs_level_fn fn, void* user, int64_t* parents, int64_t* levels);
/* the last cbg_grid_bfs on this rank.  counts: the tree's depth (the largest level; steps run = depth + 1),
 * reached vertices (the root included), edges traversed (the summed column lengths of the reached vertices,
 * TopDownBFS.cpp:448-452), push steps, pull steps, push units, pull rows scanned, pull entries read (as
 * cbg_tile_pull_max counts them); the last three are sums over the grid.  ms (may be NULL, CBG_BFS_MS_N host
 * times): push, pull, update, communication, total.  counts[i] for i < min(n, CBG_BFS_N); returns CBG_BFS_N. */
enum { CBG_BFS_LEVELS = 0, CBG_BFS_REACHED = 1, CBG_BFS_EDGES = 2, CBG_BFS_PUSH_STEPS = 3, CBG_BFS_PULL_STEPS = 4,
       CBG_BFS_PUSH_UNITS = 5, CBG_BFS_PULL_ROWS = 6, CBG_BFS_PULL_ENTRIES = 7, CBG_BFS_N = 8 };
enum { CBG_BFS_MS_PUSH = 0, CBG_BFS_MS_PULL = 1, CBG_BFS_MS_UPDATE = 2, CBG_BFS_MS_COMM = 3, CBG_BFS_MS_TOTAL = 4,
       CBG_BFS_MS_N = 5 };
int cbg_last_bfs_stats(int64_t* counts, int n, double* ms);

/* ---------------- matrix x vector on PlusTimes and MinPlus ----------------
 * SpMV<SR> (ParFriends.h:1860-1990, the local kernels dcsc_gespmv Friends.h:63-78 and SpMXSpV SpImpl.cpp) for
 * SR = CBG_PLUS_TIMES or CBG_MIN_PLUS over doubles, with a dense or a sparse x.
 *
 * The products of row i are mul(a(i, j), x[j]) for the stored (i, j) whose j takes part, in ascending j, each
 * rounded on its own (no fused multiply-add).  With a dense x every stored column takes part (a stored entry
 * times x[j] = 0 is still a product); with a sparse x exactly the columns of xind.  mul of MinPlus is inf_plus
 * (DBL_MAX if either side is DBL_MAX, else a + b), its add is b < a ? b : a.
 * The order of a row's sum depends on the number L of its products alone: L <= 16: 16 lanes, L <= 4096:
 * 64 lanes; lane l starts at the identity (-0.0, +inf) and folds products l, l + G, ... one after another, then
 * the lanes are combined by the xor tree over distances 1, 2, 4, ...  A longer list is cut into chunks of 4096
 * products (the last one shorter), each reduced as a 64-lane row, and the chunk results are folded one after
 * another.  tests/spmv_ref.py restates it.  r_i is that sum.
 *   dense result   y[i] = add(SR::id(), r_i) with the reference's id, 0.0 and DBL_MAX; a row without a stored
 *                  entry gives id (ParFriends.h:1960-1968).  A row whose products are all -0.0 gives +0.0.
 *   sparse result  one entry per row with at least one product, rows ascending, value r_i itself: a cancelled
 *                  sum stays as a stored 0.0 and a row of -0.0 products gives -0.0 (the reference's first insert).
 * On a grid each rank computes this on its tile and its slice of x, and the results of a grid row's ranks are
 * combined with SR::add in grid-column order 0, 1, ...; a rank without the row contributes nothing (sparse) or
 * id (dense).  No atomics: the same bits in every run, on every rank and on either transport.
 * A NaN in A or x, and for MinPlus a sum whose minimum is a zero that occurs with both signs, give an
 * unspecified result.
 *
 * Refusals, before any device work (collectively on a grid): CBG_ERR_INVALIDPARAMS for an unknown semiring, an
 * xind that is unsorted, repeated or outside, a negative count, a NULL output, or A and At both NULL;
 * CBG_ERR_DIMMISMATCH for an At that is not A's transpose shape, or a tile that is not this rank's block of
 * gm x gn.  An empty tile answers without a kernel.
 *
 * y = A x, dense.  At = cbg_tile_transpose(A) or NULL (made from A for this call and freed, which waits);
 * A may be NULL when At is given.  x: n doubles, y: m doubles; on_device != 0: both are device memory and the
 * call is asynchronous on `stream` (the tile and the vectors must stay until it has run), else HOST. */
int cbg_tile_spmv(const cbg_tile* A, const cbg_tile* At, int semiring, const double* x, double* y, int on_device,
                  void* hip_stream);
/* y = A x, sparse.  xind: nx distinct local column ids, ascending; xval: nx doubles;
 * yind / yval: room for A->m; *ny entries, yind ascending.  HOST arrays. */
int cbg_tile_spmspv(const cbg_tile* A, int semiring, const int64_t* xind, const double* xval, int64_t nx,
                    int64_t* yind, double* yval, int64_t* ny);
/* collective over any pr x pc grid (the reference's dense SpMV needs a square one); x (HOST, gn doubles) and
 * y (HOST, gm doubles) the same on every rank, as `parents` of cbg_grid_bfs.  At_local: the local tile's
 * transpose or NULL. */
int cbg_grid_spmv(cbg_grid* g, const cbg_tile* A_local, const cbg_tile* At_local, int64_t gm, int64_t gn,
                  int semiring, const double* x, double* y);
/* x as (global ids ascending, values), the same on every rank; y likewise (room for gm) */
int cbg_grid_spmspv(cbg_grid* g, const cbg_tile* A_local, int64_t gm, int64_t gn, int semiring, const int64_t* xind,
                    const double* xval, int64_t nx, int64_t* yind, double* yval, int64_t* ny);
/* bounds[0] = 16 and bounds[1] = 4096, the longest rows of the 16-lane and the wave class (4096 is also the
 * chunk of the longer ones); bounds[2] = C, the entries of a column of x one expansion unit of the sparse
 * product takes.  bounds[i] for i < min(n, 3); returns 3 */
int cbg_spmv_bounds(int64_t* bounds, int n);
/* the last product on this thread (a grid call: this rank's tile product): rows run by the 16-lane, the wave and
 * the chunked class, chunks; sparse: units, products expanded, entries out.  counts[i] for i < min(n, CBG_SPMV_N);
 * *ms (may be NULL): ms between two device events around the call's kernels (the sparse product's span holds
 * its two host readbacks).  Waits for an asynchronous product.  Returns CBG_SPMV_N. */
enum {
  CBG_SPMV_ROWS_GROUP = 0,
  CBG_SPMV_ROWS_WAVE = 1,
  CBG_SPMV_ROWS_LONG = 2,
  CBG_SPMV_CHUNKS = 3,
  CBG_SPMV_UNITS = 4,
  CBG_SPMV_PRODUCTS = 5,
  CBG_SPMV_ENTRIES_OUT = 6,
  CBG_SPMV_N = 7
};
int cbg_last_spmv_stats(int64_t* counts, int n, double* ms);

/* p (HOST, n int64) = the stable argsort of key[i] = mix64(seed ^ (i * 0x9E3779B97F4A7C15)), i = 0..n-1
 * (mix64: the finalizer of cbg_tile_digest).  Equal keys keep index order.  Computed on the host.
 * This library's RandPerm (FullyDistVec::RandPerm as MCL.cpp:496-512 uses it): the
 * reference's draws from MTRand and cannot be reproduced. */
int cbg_rand_perm(int64_t n, uint64_t seed, int64_t* p);

/* upper column length of each class of the indexing's column sort but the last (a wave's
 * registers, a block's LDS; longer columns go through the radix sort): bounds[i] for
 * i < min(n, 2); returns 2 */
int cbg_spref_sort_bounds(int64_t* bounds, int n);
/* the last indexing call's work on this rank (cbg_grid_hipmcl_prepared: summed over its
 * two indexings): entries in / out, columns sorted by each class (columns of fewer than
 * two entries are not counted), stored columns left unsorted because ri was strictly
 * increasing, bytes of the remote tiles received.  counts[i] for i < min(n, CBG_SPREF_N);
 * ms (may be NULL): CBG_SPREF_MS_N times in ms (column stage, row stage, sort): the sort's
 * between device events, the stages' between stream-synchronized points (uploads of the index
 * slices and waits for the broadcasts included).  Returns CBG_SPREF_N. */
enum {
  CBG_SPREF_ENTRIES_IN = 0,
  CBG_SPREF_ENTRIES_OUT = 1,
  CBG_SPREF_SORT_CLASS0 = 2, /* + c: wave, LDS, radix */
  CBG_SPREF_COLS_MONOTONE = 5,
  CBG_SPREF_BYTES_RECV = 6,
  CBG_SPREF_N = 7
};
enum { CBG_SPREF_MS_COL = 0, CBG_SPREF_MS_ROW = 1, CBG_SPREF_MS_SORT = 2, CBG_SPREF_MS_N = 3 };
int cbg_last_spref_stats(int64_t* counts, int n, double* ms);

/* nonisov of RemoveIsolated (MCL.cpp:476-486), collective over the grid: the vertices of the
 * gn x gn distributed matrix whose column sum (cbg_grid_reduce_cols(CBG_RED_SUM, 0.0): the same
 * bits on every rank of a grid column) is > 0, ascending; each rank's slice allgathered along
 * its grid row.  ids: HOST, gn int64; *n their number.  The same list on every rank. */
int cbg_grid_nonisolated(cbg_grid* g, const cbg_tile* local, int64_t gn, int64_t* ids, int64_t* n);

typedef struct cbg_hipmcl_prep {
  int32_t remove_isolated, randpermute;
  uint64_t perm_seed;
} cbg_hipmcl_prep;
/* cbg_grid_hipmcl preceded by RemoveIsolated (MCL.cpp:476-493: A(nonisov, nonisov) with nonisov
 * the vertices whose column sum is > 0) and / or RandPermute (MCL.cpp:496-512: A(p, p) with
 * p = cbg_rand_perm(n_work, perm_seed)), in that order (MCL.cpp:517-521).
 * prep == NULL or both flags 0: exactly cbg_grid_hipmcl.
 * labels (HOST, gn): in the ORIGINAL vertex numbering, canonical as before (components ordered by their
 *   smallest original vertex); every removed vertex is a cluster of its own.
 *   (The reference leaves "handle reordered cluster ids" as a TODO, MCL.cpp:495; this library maps back.)
 * work_ids (HOST, gn, may be NULL): work_ids[k] = the original vertex of working vertex k, k < *n_work.
 * n_work (may be NULL): the working matrix's dimension.
 * final_local: the converged matrix in the working numbering (n_work x n_work). */
int cbg_grid_hipmcl_prepared(cbg_grid* g, const cbg_tile* A_local, int64_t gn, const cbg_hipmcl_params* params,
                             const cbg_hipmcl_prep* prep, cbg_hipmcl_iter_fn fn, void* user, cbg_tile* final_local,
                             int64_t* labels, int64_t* nclusters, int64_t* iterations, int64_t* work_ids,
                             int64_t* n_work);

/* SpParMat::Transpose (SpParMat.cpp:3528-3590), collective over a square grid:
 * out = this rank's tile of the transposed matrix (the transpose of the
 * complement rank's tile, exchanged with RCCL send/recv).  CBG_ERR_NOTSQUARE
 * on non-square grids, like the reference. */
int cbg_grid_transpose(cbg_grid* g, const cbg_tile* local, cbg_tile* out);

/* SpParMat::BlockSplit (SpParMat.cpp:2974-3058) as BlockSpGEMM uses it
 * (BlockSpGEMM.h:39-45, bi = 1), collective over the grid: the global rows
 * [lo, hi) (dim 0) or columns [lo, hi) (dim 1) of the gm x gn distributed
 * matrix whose local tile is `local`, as a distributed matrix of their own on
 * the same grid (standard block layout, SpParMat::Owner SpParMat.cpp:5068);
 * out = this rank's tile of it. */
int cbg_grid_block_extract(cbg_grid* g, const cbg_tile* local, int64_t gm, int64_t gn, int dim, int64_t lo,
                           int64_t hi, cbg_tile* out);

#ifdef __cplusplus
}
#endif
#endif /* CBG_H */
