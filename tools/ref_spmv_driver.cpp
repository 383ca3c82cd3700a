// ref_spmv_driver.cpp -- TEST INFRASTRUCTURE ONLY (fixture generator, never built by
// build() and never on the product path).
//
// Our own driver that links the reference CombBLAS and runs ITS matrix x vector products --
// SpMV<PlusTimesSRing<double,double>> and SpMV<MinPlusSRing<double,double>> with a dense vector
// (ParFriends.h:1922-1990) and with a sparse one (ParFriends.h:1892-1897) -- on a Matrix Market
// file and two vector files, so that the tests/golden/spmv_*.npz fixtures come from the
// reference's own run (tests/golden/make_spmv_golden.py calls it).  Nothing is copied from the
// reference.
//
//   ref_spmv_driver <A.mtx> <x_dense.txt> <x_sparse.txt> <out>
//
// The vector files are what ReadDistribute takes: "n 1 nnz", then "i 1 value" lines (1-based).
// Rank 0 writes <out>: one line "<kind> <row> <bits>" per result entry, kind one of pt_dense,
// mp_dense (every row), pt_sparse, mp_sparse (the stored entries), row 0-based, bits the value's
// 64 bits in hex.
//
// Compile (the flags oracle/Makefile uses for ref_driver; REF = the reference's root,
// MPI = the MPICH prefix, OBJ = oracle/_ref after `make -C oracle ref`):
//   g++ -O3 -fopenmp -DTHREADED -std=c++14 -w -I$REF/include -I$REF/include/CombBLAS \
//       -I$REF/psort-1.0/include -I$REF/usort/include -I$REF/graph500-1.2/generator/include \
//       -I$MPI/include tools/ref_spmv_driver.cpp $OBJ/CommGrid.o $OBJ/MPIType.o \
//       $OBJ/MPIOp.o $OBJ/MemoryPool.o $OBJ/hash.o $OBJ/mmio.o $OBJ/gen_*.o -o ref_spmv_driver \
//       -Wl,-rpath,$MPI/lib $MPI/lib/libmpicxx.so $MPI/lib/libmpi.so -lm
#include <mpi.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>

#include "CombBLAS/CombBLAS.h"

using namespace combblas;

typedef SpParMat<int64_t, double, SpDCCols<int64_t, double>> PMat;
typedef PlusTimesSRing<double, double> PT;
typedef MinPlusSRing<double, double> MP;

static unsigned long long bits_of(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}

template <class SR>
static void run(PMat& A, FullyDistVec<int64_t, double>& x, FullyDistSpVec<int64_t, double>& spx, const char* name, FILE* f,
                int rank) {
  const int64_t m = A.getnrow();
  FullyDistVec<int64_t, double> y = SpMV<SR>(A, x);
  for (int64_t i = 0; i < m; ++i) {
    const double v = y.GetElement(i);  // collective
    if (rank == 0) fprintf(f, "%s_dense %lld %016llx\n", name, (long long)i, bits_of(v));
  }
  FullyDistSpVec<int64_t, double> spy(spx.getcommgrid(), m);
  SpMV<SR>(A, spx, spy, false);
  for (int64_t i = 0; i < m; ++i) {
    const double v = spy[i];  // collective
    if (spy.WasFound() && rank == 0) fprintf(f, "%s_sparse %lld %016llx\n", name, (long long)i, bits_of(v));
  }
}

int main(int argc, char* argv[]) {
  int provided;
  MPI_Init_thread(&argc, &argv, MPI_THREAD_SERIALIZED, &provided);
  int rank;
  MPI_Comm_rank(MPI_COMM_WORLD, &rank);
  if (argc < 5) {
    if (rank == 0) fprintf(stderr, "usage: see the header of ref_spmv_driver.cpp\n");
    MPI_Finalize();
    return 1;
  }
  {
    auto grid = std::make_shared<CommGrid>(MPI_COMM_WORLD, 0, 0);
    PMat A(grid);
    A.ParallelReadMM(argv[1], true, maximum<double>());
    FullyDistVec<int64_t, double> x(grid);
    FullyDistSpVec<int64_t, double> spx(grid);
    std::ifstream fx(argv[2]), fs(argv[3]);
    x.ReadDistribute(fx, 0);
    spx.ReadDistribute(fs, 0);
    FILE* f = nullptr;
    if (rank == 0 && !(f = fopen(argv[4], "w"))) MPI_Abort(MPI_COMM_WORLD, 1);
    run<PT>(A, x, spx, "pt", f, rank);
    run<MP>(A, x, spx, "mp", f, rank);
    if (f) fclose(f);
  }
  MPI_Finalize();
  return 0;
}
