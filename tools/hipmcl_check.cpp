// hipmcl_check.cpp -- the whole HipMCL loop on the MI355X path, written against the
// C++ mirror header combblas_amd/CombBLAS.h.
//
//   mpirun -n P ./hipmcl_check <Matrix.mtx> [inflation hardThreshold selectNum recoverNum recoverPct [max_iterations]]
//                              [remove_isolated] [randpermute [seed]]
//
// The trailing words switch on HipMCL's preparation steps (MCL.cpp:517-521); with them the
// working matrix's dimension is printed too ("n_work <n>"), and RemoveIsolated / RandPermute
// are checked on their own (SubsRef_SR keeps the nonzero count of a permutation).
// Reads A with ParallelReadMM, runs HipMCL (Applications/MCL.cpp:515-647) and prints
// the iteration count, the chaos of every iteration, the number of clusters and a
// digest of the labels (FNV-1a over the 64-bit labels in vertex order; the labels are
// canonical, so equal partitions have equal digests).  Also checks the step functions
// against the loop: AdjustLoops + MakeColStochastic leave every column summing to 1.
#include <mpi.h>

#include <cctype>
#include <cmath>
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
  if (argc < 2) {
    if (myrank == 0) std::printf("Usage: ./hipmcl_check <Matrix> [inflation h S R q [max_iterations]]\n");
    MPI_Finalize();
    return -1;
  }
  int failures = 0;
  {
    auto fullWorld = std::make_shared<CommGrid>(MPI_COMM_WORLD, 0, 0);
    PMat A(fullWorld), B(fullWorld);
    A.ParallelReadMM(argv[1], true, maximum<double>());
    B.ParallelReadMM(argv[1], true, maximum<double>());
    HipMCLParam param;
    if (argc >= 7) {
      param.inflation = atof(argv[2]);
      param.prunelimit = atof(argv[3]);
      param.select = atoll(argv[4]);
      param.recover_num = atoll(argv[5]);
      param.recover_pct = atof(argv[6]);
    }
    int at = 7;
    if (argc > at && std::isdigit((unsigned char)argv[at][0])) param.max_iterations = atoll(argv[at++]);
    for (; at < argc; ++at) {
      const std::string w = argv[at];
      if (w == "remove_isolated") {
        param.remove_isolated = true;
      } else if (w == "randpermute") {
        param.randpermute = true;
        if (at + 1 < argc && std::isdigit((unsigned char)argv[at + 1][0])) param.perm_seed = strtoull(argv[++at], nullptr, 0);
      } else {
        if (myrank == 0) std::printf("unknown argument %s\n", w.c_str());
        MPI_Finalize();
        return -1;
      }
    }
    // the steps on their own: a stochastic matrix has column sums 1
    AdjustLoops(B);
    MakeColStochastic(B);
    bool stochastic = true;
    for (double s : B.Reduce(Column, CBG_RED_SUM, 0.0)) stochastic = stochastic && std::fabs(s - 1.0) < 1e-12;
    if (myrank == 0) std::printf("AdjustLoops + MakeColStochastic: %s\n", stochastic ? "ok" : "ERROR");
    failures += stochastic ? 0 : 1;
    if (param.remove_isolated || param.randpermute) {
      // the steps on their own: a permutation keeps every entry, a removal drops whole rows and columns
      PMat C(fullWorld);
      C.ParallelReadMM(argv[1], true, maximum<double>());
      const int64_t nnz0 = C.getnnz();
      bool ok = true;
      if (param.remove_isolated) {
        const std::vector<int> nonisov = RemoveIsolated(C);
        ok = ok && C.getnrow() == (int)nonisov.size() && C.getncol() == (int)nonisov.size() && C.getnnz() <= nnz0;
      }
      if (param.randpermute) {
        const int64_t nnz1 = C.getnnz();
        const std::vector<int> p = RandPermute(C, param.perm_seed);
        ok = ok && (int)p.size() == C.getncol() && C.getnnz() == nnz1;
      }
      if (myrank == 0) std::printf("RemoveIsolated / RandPermute: %s\n", ok ? "ok" : "ERROR");
      failures += ok ? 0 : 1;
    }
    const std::vector<int> labels = HipMCL(A, param);
    uint64_t h = 0xcbf29ce484222325ULL;
    int64_t nclusters = 0;
    for (int l : labels) {
      const uint64_t v = (uint64_t)(int64_t)l;
      for (int b = 0; b < 8; ++b) h = (h ^ ((v >> (8 * b)) & 0xff)) * 0x100000001b3ULL;
      nclusters = std::max<int64_t>(nclusters, (int64_t)l + 1);
    }
    if (myrank == 0) {
      std::printf("iterations %d\n", param.iterations);
      for (size_t i = 0; i < param.chaos.size(); ++i) std::printf("chaos %zu %.17g\n", i + 1, param.chaos[i]);
      std::printf("clusters %lld labels %016llx\n", (long long)nclusters, (unsigned long long)h);
      if (param.remove_isolated || param.randpermute) std::printf("n_work %lld\n", (long long)param.n_work);
    }
  }
  if (myrank == 0 && failures == 0) std::printf("HIPMCLCHECK OK\n");
  MPI_Finalize();
  return failures;
}
