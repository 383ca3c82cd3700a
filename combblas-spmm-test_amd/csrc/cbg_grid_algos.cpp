// cbg_grid_algos.cpp -- the algorithms on a grid, on top of the communication layer, the SUMMA and the
// redistributions of cbg_summa.cpp (cbg_grid.h): MCL pruning, the HipMCL iteration, loops, connected components,
// sparse indexing with RemoveIsolated / RandPermute, BetwCent, BFS, SpMV / SpMSpV.  Every entry agrees on
// its return code as the SUMMA does: a local step's failure is carried to the next agree(), never thrown past it.
#include <algorithm>
#include <chrono>
#include <limits>

#include "cbg_grid.h"

namespace cbg {

using clk = std::chrono::steady_clock;
static double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// "Every row block to every rank": the blocks of a vector distributed by rows are padded to the longest,
// gathered along the grid column in ONE allgather whatever the number of fields, and un-padded here:
// item i - start(q) of block q of `col` (blocks `stride` items apart) is item i of the vector
template <class T, class Put>
static void unpad_blocks(const Blocks& rows, const T* col, size_t stride, Put&& put) {
  for (int q = 0; q < rows.np; ++q) {
    int64_t a = 0, b = 0;
    rows.span(q, a, b);
    for (int64_t i = a; i < b; ++i) put(i, col[(size_t)q * stride + (i - a)]);
  }
}
// a field: {this rank's block (lm items on the device), the caller's rows.ext host items or NULL (not stored)}
template <class T>
static void gather_row_blocks(cbg_grid* g, const Blocks& rows, int64_t lm,
                              std::initializer_list<std::pair<const T*, T*>> fields) {
  if (rows.np == 1) {  // the one row block is the whole vector: no collective, straight into the caller's arrays
    for (const auto& f : fields)
      if (lm && f.second) CBG_HIP(hipMemcpy(f.second, f.first, sizeof(T) * lm, hipMemcpyDeviceToHost));
    return;
  }
  const size_t l1 = (size_t)std::max<int64_t>(rows.longest(), 1), k = fields.size();
  std::vector<T> mine(k * l1), col(k * l1 * rows.np);
  const auto* fd = fields.begin();
  for (size_t f = 0; f < k && lm; ++f)
    CBG_HIP(hipMemcpy(mine.data() + f * l1, fd[f].first, sizeof(T) * lm, hipMemcpyDeviceToHost));
  allgather_bytes(g, COMM_COL, mine.data(), col.data(), sizeof(T) * k * l1);
  for (size_t f = 0; f < k; ++f)
    if (T* whole = fd[f].second) unpad_blocks(rows, col.data() + f * l1, k * l1, [&](int64_t i, T v) { whole[i] = v; });
}

// ---------------------------------------------------------------------------
// Markov-clustering pruning (MCLPruneRecoverySelect, ParFriends.h:186-353; the
// kernels and the per-piece logic are in cbg_prune.hip).  All of its
// collectives run along the grid column; the world only agrees on the result.
// ---------------------------------------------------------------------------
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
int grid_spref(cbg_grid* g, const cbg_tile& T, int64_t gm, int64_t gn, const int64_t* ri, int64_t nri,
               const int64_t* ci, int64_t nci, cbg_tile& out) {
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
    const Blocks new_rows{new_m, g->pr}, new_cols{new_n, g->pc};
    new_rows.span(g->prow, U0, U1);
    new_cols.span(g->pcol, V0, V1);
    if (new_rows.longest() >= INT32_MAX || new_cols.longest() >= INT32_MAX) {
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
    const int64_t per = Blocks{gn, np}.per(), maxn = Blocks{gn, np}.longest(), nsel = V1 - V0;
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
    const int64_t nloc = U1 - U0, ncols = src->n;
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
          spref_expand_rows(sl, Blocks{gm, np}.start(q), inv, nloc, piece.t, cs);
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
  const Blocks rows{gn, g->pr};
  rows.span(g->prow, r0, r1);
  const int64_t lm = r1 - r0, lmax = rows.longest();
  std::vector<double> acc;
  if ((rc = agree(g, step([&] { acc.assign((size_t)std::max<int64_t>(gn, 1), 0.0); })))) return rc;

  for (int64_t b0 = 0, bi = 0; b0 < nroots; b0 += P.batch, ++bi) {
    const int64_t nb = std::min<int64_t>(P.batch, nroots - b0);
    int64_t c0 = 0, c1 = 0;
    Blocks{nb, g->pc}.span(g->pcol, c0, c1);
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
      unpad_blocks(rows, col.data(), (size_t)lmax, [&](int64_t i, double v) { acc[i] += v; });
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
  const Blocks rows{gn, g->pr};
  const int64_t lm = A.m, ln = A.n, per = rows.per(), lmax = rows.longest();
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
  rc = step([&] { gather_row_blocks<int64_t>(g, rows, lm, {{parent.p, parents}, {level.p, levels}}); });
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
  const int64_t lm = shape.m, ln = shape.n;
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
  rc = step([&] { gather_row_blocks<double>(g, Blocks{gm, g->pr}, lm, {{dy.p, y}}); });
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
