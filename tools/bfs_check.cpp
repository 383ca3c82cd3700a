// bfs_check.cpp -- single-source breadth-first search on the MI355X path, written against the
// C++ mirror header combblas_amd/CombBLAS.h, with the `Input` command line of the reference's
// Applications/TopDownBFS.cpp:
//
//   mpirun -n P ./bfs_check Input <file.mtx>
//
// The file's matrix is symmetrised (A += A^T, TopDownBFS.cpp:84-93), the roots are the first four
// vertices of nonzero degree, and every tree is searched under the reference's direction rule and
// once more top-down only (the same bits), then checked by the Graph500 rules: the root is its own
// parent; every other reached vertex has a stored edge from its parent; level[v] =
// level[parent[v]] + 1; no stored edge leaves the reached set; no stored edge spans more than one
// level forward.  Every rank checks the entries of its own tile.  Prints per root
// "root <r> levels <depth> reached <count> trace <d|u per step>" and at the end BFSCHECK OK.
#include <mpi.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "combblas_amd/CombBLAS.h"

using namespace combblas_amd;
typedef SpDCCols<int, double> DCCols;
typedef SpParMat<int, double, DCCols> PMat;

int main(int argc, char* argv[]) {
  MPI_Init(&argc, &argv);
  int myrank;
  MPI_Comm_rank(MPI_COMM_WORLD, &myrank);
  if (argc < 3 || std::string(argv[1]) != "Input") {
    if (myrank == 0) std::printf("Usage: ./bfs_check Input <Matrix Market file>\n");
    MPI_Finalize();
    return -1;
  }
  int64_t failures = 0;
  {
    auto fullWorld = std::make_shared<CommGrid>(MPI_COMM_WORLD, 0, 0);
    PMat A(fullWorld), AT(fullWorld);
    A.ParallelReadMM(argv[2], true, maximum<double>());
    AT.ParallelReadMM(argv[2], true, maximum<double>());
    AT.Transpose();
    A += AT;  // the union: an entry stored both ways is stored once
    A.ApplySet(1.0);
    const int64_t n = A.getncol();
    // this rank's entries on the host, as global ids
    const cbg_tile* t = A.spSeq->tile();
    std::vector<int64_t> cp((size_t)t->nzc + 1);
    std::vector<int32_t> jc((size_t)std::max<int64_t>(t->nzc, 1)), ir((size_t)std::max<int64_t>(t->nnz, 1));
    std::vector<double> val((size_t)std::max<int64_t>(t->nnz, 1));
    cbg_tile h{};
    h.cp = cp.data(), h.jc = jc.data(), h.ir = ir.data(), h.val = val.data();
    cbg_abort_on(cbg_tile_download(t, &h), "download");
    const int64_t roff = (int64_t)fullWorld->GetRankInProcCol() * (n / fullWorld->GetGridRows());
    const int64_t coff = (int64_t)fullWorld->GetRankInProcRow() * (n / fullWorld->GetGridCols());
    // roots: the first vertices whose column stores something
    std::vector<int64_t> ids((size_t)std::max<int64_t>(n, 1));
    int64_t nids = 0;
    cbg_abort_on(cbg_grid_nonisolated(fullWorld->handle(), t, n, ids.data(), &nids), "roots");
    cbg_tile At{};
    cbg_abort_on(cbg_tile_transpose(t, &At), "transpose");  // made once for all the roots
    for (int64_t k = 0; k < std::min<int64_t>(nids, 4); ++k) {
      const int root = (int)ids[k];
      const BFSResult r = BFS(A, root, CBG_BFS_AUTO, &At), td = BFS(A, root, CBG_BFS_TOPDOWN);
      int64_t bad = r.parents != td.parents || r.levels != td.levels ? 1 : 0;
      const std::vector<int64_t>&p = r.parents, &lv = r.levels;
      int64_t reached = 0, depth = 0, parent_edges = 0;
      if (p[root] != root || lv[root] != 0) ++bad;
      for (int64_t v = 0; v < n; ++v) {
        if ((p[v] >= 0) != (lv[v] >= 0)) ++bad;
        if (p[v] < 0) continue;
        ++reached;
        depth = std::max(depth, lv[v]);
        if (v != root && (p[v] >= n || lv[p[v]] < 0 || lv[v] != lv[p[v]] + 1)) ++bad;
      }
      for (int64_t c = 0; c < t->nzc; ++c)
        for (int64_t x = cp[c]; x < cp[c + 1]; ++x) {
          const int64_t j = coff + jc[c], i = roff + ir[x];  // the edge j -> i
          if (lv[j] >= 0 && (lv[i] < 0 || lv[i] > lv[j] + 1)) ++bad;
          if (i != root && p[i] == j) ++parent_edges;
        }
      cbg_abort_on(cbg_grid_allreduce_sum_i64(fullWorld->handle(), &parent_edges), "allreduce");
      cbg_abort_on(cbg_grid_allreduce_sum_i64(fullWorld->handle(), &bad), "allreduce");
      if (parent_edges != reached - 1) ++bad;  // every reached vertex but the root: its parent's edge is stored
      if (myrank == 0)
        std::printf("root %d levels %lld reached %lld trace %s%s\n", root, (long long)depth, (long long)reached, r.trace.c_str(),
                    bad ? "  ERROR" : "");
      failures += bad;
    }
    cbg_tile_free(&At);
  }
  if (myrank == 0 && failures == 0) std::printf("BFSCHECK OK\n");
  MPI_Finalize();
  return failures ? 1 : 0;
}
