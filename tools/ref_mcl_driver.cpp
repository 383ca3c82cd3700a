// ref_mcl_driver.cpp -- TEST INFRASTRUCTURE ONLY (fixture generator, never built
// by build() and never on the product path).
//
// Our own driver that links the reference CombBLAS and runs ITS
// MCLPruneRecoverySelect (ParFriends.h:186-353) on a Matrix Market file, so that
// the tests/golden/mcl_*.npz fixtures come from the reference's own run
// (tests/golden/make_mcl_golden.py calls it).
//
//   ref_mcl_driver <in.mtx> <hardThreshold> <selectNum> <recoverNum> <recoverPct> <out.txt>
//
// Every rank appends nothing: rank r writes <out.txt>.r<r> with one
// "global_row global_col value(%.17g)" line per surviving entry (0-based).
//
// Compile (the flags oracle/Makefile uses for ref_driver; REF = the reference's
// root, MPI = the MPICH prefix, OBJ = oracle/_ref after `make -C oracle ref`):
//   g++ -O3 -fopenmp -DTHREADED -std=c++14 -w -I$REF/include -I$REF/include/CombBLAS \
//       -I$REF/psort-1.0/include -I$REF/usort/include -I$REF/graph500-1.2/generator/include \
//       -I$MPI/include tools/ref_mcl_driver.cpp $OBJ/CommGrid.o $OBJ/MPIType.o $OBJ/MPIOp.o \
//       $OBJ/MemoryPool.o $OBJ/hash.o $OBJ/mmio.o $OBJ/gen_*.o -o ref_mcl_driver \
//       -L$MPI/lib -Wl,-rpath,$MPI/lib -lmpicxx -lmpi -lm
#include <mpi.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "CombBLAS/CombBLAS.h"

using namespace combblas;

typedef SpDCCols<int64_t, double> DCCols;
typedef SpParMat<int64_t, double, DCCols> PMat;

int main(int argc, char* argv[]) {
  MPI_Init(&argc, &argv);
  int rank;
  MPI_Comm_rank(MPI_COMM_WORLD, &rank);
  if (argc < 7) {
    if (rank == 0) fprintf(stderr, "usage: see the header of ref_mcl_driver.cpp\n");
    MPI_Finalize();
    return 1;
  }
  {
    auto grid = std::make_shared<CommGrid>(MPI_COMM_WORLD, 0, 0);
    PMat A(grid);
    A.ParallelReadMM(argv[1], true, maximum<double>());
    const double h = atof(argv[2]), q = atof(argv[5]);
    const int64_t S = atoll(argv[3]), R = atoll(argv[4]);
    MCLPruneRecoverySelect(A, h, S, R, q, 1);
    // the tile's place in the global matrix (SpParMat::GetPlaceInGlobalGrid's arithmetic)
    const int64_t roff = grid->GetRankInProcCol() * (A.getnrow() / grid->GetGridRows());
    const int64_t coff = grid->GetRankInProcRow() * (A.getncol() / grid->GetGridCols());
    const std::string path = std::string(argv[6]) + ".r" + std::to_string(rank);
    FILE* f = fopen(path.c_str(), "w");
    if (!f) MPI_Abort(MPI_COMM_WORLD, 1);
    const DCCols& T = A.seq();
    if (T.getnnz() > 0) {
      Dcsc<int64_t, double>* dc = T.GetDCSC();
      for (int64_t i = 0; i < dc->nzc; ++i)
        for (int64_t p = dc->cp[i]; p < dc->cp[i + 1]; ++p)
          fprintf(f, "%lld %lld %.17g\n", (long long)(dc->ir[p] + roff), (long long)(dc->jc[i] + coff), dc->numx[p]);
    }
    fclose(f);
  }
  MPI_Finalize();
  return 0;
}
