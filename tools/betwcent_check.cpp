// betwcent_check.cpp -- batched betweenness centrality on the MI355X path, written against
// the C++ mirror header combblas_amd/CombBLAS.h, with the command line of the reference's
// Applications/BetwCent.cpp:
//
//   mpirun -n P ./betwcent_check <BASEADDRESS> <K4APPROX> <BATCHSIZE> [output file]
//
// <BASEADDRESS>/input.mtx holds AT, the transpose of the graph's matrix (BetwCent.cpp:98-100);
// the roots are the first 2^K4APPROX vertices whose column of AT stores something; the output
// file is written the way FullyDistVec::SaveGathered writes bc: "n 1 n", then "index 1 value"
// from index 1 on, 21 significant digits.  A shorter last batch is allowed as long as it holds at
// least as many roots as the grid has columns (the reference rounds the number of roots to a
// multiple of the batch instead).  Also checks the element-wise
// ops on the way: A .* A^T and A \ A^T are disjoint and have A's entries between them.
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
  if (argc < 4) {
    if (myrank == 0) std::printf("Usage: ./betwcent_check <BASEADDRESS> <K4APPROX> <BATCHSIZE> <output file - optional>\n");
    MPI_Finalize();
    return -1;
  }
  int failures = 0;
  {
    const std::string file = std::string(argv[1]) + "/input.mtx";
    const int64_t want = (int64_t)1 << atoi(argv[2]), batch = atoll(argv[3]);
    auto fullWorld = std::make_shared<CommGrid>(MPI_COMM_WORLD, 0, 0);
    PMat A(fullWorld), AT(fullWorld);
    AT.ParallelReadMM(file, true, maximum<double>());
    A.ParallelReadMM(file, true, maximum<double>());
    A.Transpose();
    // the candidates: vertices with a nonempty column of AT.  Every stored entry is `true` (the reference reads
    // a bool matrix), so AT is made unit-valued in place: its column sums are > 0 exactly where it stores something
    AT.ApplySet(1.0);
    std::vector<int64_t> ids((size_t)std::max<int64_t>(AT.getncol(), 1));
    int64_t nids = 0;
    cbg_abort_on(cbg_grid_nonisolated(AT.commGrid->handle(), AT.spSeq->tile(), AT.getncol(), ids.data(), &nids), "candidates");
    const std::vector<int> roots(ids.begin(), ids.begin() + std::min(nids, want));
    // the element-wise ops on their own
    const PMat both = EWiseMult(A, AT, false), only = SetDifference(A, AT);
    const bool split = both.getnnz() + only.getnnz() == A.getnnz() && EWiseMult(both, only, false).getnnz() == 0;
    if (myrank == 0) std::printf("EWiseMult + SetDifference: %s\n", split ? "ok" : "ERROR");
    failures += split ? 0 : 1;
    std::vector<int64_t> levels;
    const std::vector<double> bc = BetwCent(A, roots, batch, &AT, &levels);
    if (myrank == 0) {
      std::printf("roots %zu batches %lld levels %zu\n", roots.size(), (long long)((roots.size() + batch - 1) / batch),
                  levels.size());
      if (argc > 4) {
        FILE* f = std::fopen(argv[4], "w");
        if (!f) {
          std::printf("cannot write %s\n", argv[4]);
          ++failures;
        } else {
          std::fprintf(f, "%zu\t1\t%zu\n", bc.size(), bc.size());
          for (size_t i = 0; i < bc.size(); ++i) std::fprintf(f, "%zu\t1\t%.21g\n", i + 1, bc[i]);
          std::fclose(f);
        }
      }
    }
  }
  if (myrank == 0 && failures == 0) std::printf("BETWCENTCHECK OK\n");
  MPI_Finalize();
  return failures;
}
