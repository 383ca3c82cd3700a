// ref_spref_driver.cpp -- TEST INFRASTRUCTURE ONLY (fixture generator, never built by
// build() and never on the product path).
//
// Our own driver that links the reference CombBLAS and runs ITS sparse indexing,
// SpParMat::operator()(ri, ci) (SubsRef_SR, SpParMat.cpp:2026-2247), on a Matrix Market
// file, so that the tests/golden/spref_*.npz fixtures come from the reference's own run
// (tests/golden/make_spref_golden.py calls it).  Nothing is copied from the reference.
//
//   ref_spref_driver <in.mtx> <ri.txt> <ci.txt> <symmetric 0|1> <out>
//
// ri.txt / ci.txt: the number of indices, then the 0-based indices.  symmetric 1 passes
// the SAME vector object for rows and columns (the reference's symmetric-permutation path,
// SpParMat.cpp:2141); ci.txt is then ignored.  Rank r writes <out>.r<r> with one
// "global_row global_col value(%.17g)" line per entry of the result (0-based).
//
// Compile (the flags oracle/Makefile uses for ref_driver; REF = the reference's root,
// MPI = the MPICH prefix, OBJ = oracle/_ref after `make -C oracle ref`):
//   g++ -O3 -fopenmp -DTHREADED -std=c++14 -w -I$REF/include -I$REF/include/CombBLAS \
//       -I$REF/psort-1.0/include -I$REF/usort/include -I$REF/graph500-1.2/generator/include \
//       -I$MPI/include tools/ref_spref_driver.cpp $OBJ/CommGrid.o $OBJ/MPIType.o \
//       $OBJ/MPIOp.o $OBJ/MemoryPool.o $OBJ/hash.o $OBJ/mmio.o $OBJ/gen_*.o -o ref_spref_driver \
//       -Wl,-rpath,$MPI/lib $MPI/lib/libmpicxx.so $MPI/lib/libmpi.so -lm
#include <mpi.h>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "CombBLAS/CombBLAS.h"

using namespace combblas;

typedef SpDCCols<int64_t, double> DCCols;
typedef SpParMat<int64_t, double, DCCols> PMat;
typedef FullyDistVec<int64_t, int64_t> IVec;

static std::vector<int64_t> read_indices(const char* path) {
  std::ifstream f(path);
  long long n = 0;
  f >> n;
  std::vector<int64_t> v((size_t)n);
  for (long long i = 0; i < n; ++i) {
    long long x;
    f >> x;
    v[i] = x;
  }
  if (!f) MPI_Abort(MPI_COMM_WORLD, 2);
  return v;
}

static void fill(IVec& v, const std::vector<int64_t>& idx) {
  for (size_t i = 0; i < idx.size(); ++i) v.SetElement((int64_t)i, idx[i]);  // the owner stores it
}

int main(int argc, char* argv[]) {
  int provided;
  MPI_Init_thread(&argc, &argv, MPI_THREAD_SERIALIZED, &provided);
  int rank;
  MPI_Comm_rank(MPI_COMM_WORLD, &rank);
  if (argc < 6) {
    if (rank == 0) fprintf(stderr, "usage: see the header of ref_spref_driver.cpp\n");
    MPI_Finalize();
    return 1;
  }
  {
    auto grid = std::make_shared<CommGrid>(MPI_COMM_WORLD, 0, 0);
    PMat A(grid);
    A.ParallelReadMM(argv[1], true, maximum<double>());
    const std::vector<int64_t> r = read_indices(argv[2]), c = read_indices(argv[3]);
    const bool symmetric = atoi(argv[4]) != 0;
    IVec ri(grid, (int64_t)r.size(), 0), ci(grid, (int64_t)c.size(), 0);
    fill(ri, r);
    fill(ci, c);
    PMat B = symmetric ? A(ri, ri) : A(ri, ci);
    const int64_t roff = grid->GetRankInProcCol() * (B.getnrow() / grid->GetGridRows());
    const int64_t coff = grid->GetRankInProcRow() * (B.getncol() / grid->GetGridCols());
    const std::string path = std::string(argv[5]) + ".r" + std::to_string(rank);
    FILE* f = fopen(path.c_str(), "w");
    if (!f) MPI_Abort(MPI_COMM_WORLD, 1);
    const DCCols& T = B.seq();
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
