// mcl_check.cpp -- the Markov-clustering pruning on the MI355X path, written
// against the C++ mirror header combblas_amd/CombBLAS.h.
//
//   mpirun -n P ./mcl_check <Matrix.mtx> <hardThreshold> <selectNum> <recoverNum> <recoverPct>
//
// Reads A with ParallelReadMM, forms A*A with MemEfficientSpGEMM (3 phases) once
// with the pruning arguments and once without, prunes the unpruned product with
// MCLPruneRecoverySelect and checks that both ways agree (operator==, then the
// exact digests); then SpParMat::Kselect and SpParMat::PruneColumn: pruning every
// column at its own largest value keeps at least one entry of each nonempty column
// and nothing below it.  Prints the pruned product's digest (global coordinates).
#include <mpi.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "combblas_amd/CombBLAS.h"

using namespace combblas_amd;
typedef SpDCCols<int, double> DCCols;
typedef SpParMat<int, double, DCCols> PMat;
typedef PlusTimesSRing<double, double> PTDOUBLEDOUBLE;

struct Digest {
  int64_t nnz, hs, hv;
  bool operator==(const Digest& o) const { return nnz == o.nnz && hs == o.hs && hv == o.hv; }
};

static Digest digest(const PMat& M) {
  auto g = M.getcommgrid();
  const int64_t roff = (int64_t)g->GetRankInProcCol() * (M.getnrow() / g->GetGridRows());
  const int64_t coff = (int64_t)g->GetRankInProcRow() * (M.getncol() / g->GetGridCols());
  uint64_t hs = 0, hv = 0, unsorted = 0;
  double vsum = 0;
  cbg_abort_on(cbg_tile_digest(M.seq().tile(), roff, coff, &hs, &hv, &vsum, &unsorted), "digest");
  int64_t v[4] = {M.seq().tile()->nnz, (int64_t)hs, (int64_t)hv, (int64_t)unsorted};
  for (auto& x : v) cbg_abort_on(cbg_grid_allreduce_sum_i64(g->handle(), &x), "allreduce");  // wraps mod 2^64
  if (v[3] != 0) cbg_abort_on(CBG_ERR_INVALIDPARAMS, "a pruned tile is not a valid DCSC tile");
  return Digest{v[0], v[1], v[2]};
}

int main(int argc, char* argv[]) {
  MPI_Init(&argc, &argv);
  int myrank;
  MPI_Comm_rank(MPI_COMM_WORLD, &myrank);
  if (argc < 6) {
    if (myrank == 0) std::printf("Usage: ./mcl_check <Matrix> <hardThreshold> <selectNum> <recoverNum> <recoverPct>\n");
    MPI_Finalize();
    return -1;
  }
  int failures = 0;
  {
    const double h = atof(argv[2]), q = atof(argv[5]);
    const int S = atoi(argv[3]), R = atoi(argv[4]);
    auto fullWorld = std::make_shared<CommGrid>(MPI_COMM_WORLD, 0, 0);
    PMat A(fullWorld), B(fullWorld);
    A.ParallelReadMM(argv[1], true, maximum<double>());
    B.ParallelReadMM(argv[1], true, maximum<double>());
    auto report = [&](bool ok, const char* what) {
      if (myrank == 0) std::printf("%s: %s\n", what, ok ? "ok" : "ERROR");
      failures += ok ? 0 : 1;
    };
    PMat C = MemEfficientSpGEMM<PTDOUBLEDOUBLE, double, DCCols>(A, B, 3, h, S, R, q, 1, 1, 0);
    PMat U = MemEfficientSpGEMM<PTDOUBLEDOUBLE, double, DCCols>(A, B, 3, 0.0, 0, 0, 0.0, 1, 1, 0);
    const int64_t unpruned = U.getnnz();
    const Digest dc = digest(C);
    if (myrank == 0)
      std::printf("pruned product: nnz %lld hs %016llx hv %016llx (unpruned nnz %lld)\n", (long long)dc.nnz,
                  (unsigned long long)dc.hs, (unsigned long long)dc.hv, (long long)unpruned);
    report(dc.nnz <= unpruned, "pruning removes entries only");
    MCLPruneRecoverySelect(U, h, S, R, q, 1);
    report(U == C, "MCLPruneRecoverySelect of the product == the pruned product (operator==)");
    report(digest(U) == dc, "... and by digest (bit-exact)");
    // Kselect + PruneColumn: every local column pruned at its own largest value
    const int64_t nloc = C.seq().tile()->n;
    std::vector<int32_t> cols((size_t)nloc);
    for (int64_t j = 0; j < nloc; ++j) cols[j] = (int32_t)j;
    const std::vector<double> top = C.Kselect(cols, 1);
    const std::vector<double> low = C.Kselect(cols, 1 << 30);  // fewer entries than k: the smallest
    bool ordered = true;
    for (int64_t j = 0; j < nloc; ++j) ordered = ordered && !(top[j] < low[j]);
    report(ordered, "Kselect: largest >= smallest in every column");
    PMat T = C.PruneColumn(top);
    PMat L = C.PruneColumn(low);
    report(digest(L) == dc, "PruneColumn at the smallest value keeps everything");
    const int64_t kept = T.getnnz();
    report(kept > 0 && kept <= dc.nnz, "PruneColumn at the largest value keeps the maxima only");
  }
  if (myrank == 0 && failures == 0) std::printf("MCLCHECK OK\n");
  MPI_Finalize();
  return failures;
}
