// ref_bfs_driver.cpp -- TEST INFRASTRUCTURE ONLY (fixture generator, never built by
// build() and never on the product path).
//
// Our own driver that links the reference CombBLAS and runs ITS top-down breadth-first
// search -- the loop of Applications/TopDownBFS.cpp:427-443: setNumToInd,
// SpMV<SelectMaxSRing<bool,int64_t>> with the values sent (ParFriends.h:1909-1918, local kernel
// SpImpl.cpp:168-221), EWiseMult against the parents, Set --
// on a Matrix Market file, so that the tests/golden/bfs_*.npz fixtures come from the
// reference's own run (tests/golden/make_bfs_golden.py calls it).  Nothing is copied from
// the reference.  The file is taken as it is (no symmetrisation): a line "i j" is the
// stored A(i, j), the edge j -> i.
//
//   ref_bfs_driver <in.mtx> <out> <root> [<root> ...]
//
// Rank 0 writes <out>: per root one line "root <r> iterations <k>" and then n lines
// "vertex parent" (0-based, -1: not reached).  As in TopDownBFS the root's own parent is
// whatever an edge back to it gives, -1 without one.
//
// Compile (the flags oracle/Makefile uses for ref_driver; REF = the reference's root,
// MPI = the MPICH prefix, OBJ = oracle/_ref after `make -C oracle ref`):
//   g++ -O3 -fopenmp -DTHREADED -std=c++14 -w -I$REF/include -I$REF/include/CombBLAS \
//       -I$REF/psort-1.0/include -I$REF/usort/include -I$REF/graph500-1.2/generator/include \
//       -I$MPI/include tools/ref_bfs_driver.cpp $OBJ/CommGrid.o $OBJ/MPIType.o \
//       $OBJ/MPIOp.o $OBJ/MemoryPool.o $OBJ/hash.o $OBJ/mmio.o $OBJ/gen_*.o -o ref_bfs_driver \
//       -Wl,-rpath,$MPI/lib $MPI/lib/libmpicxx.so $MPI/lib/libmpi.so -lm
#include <mpi.h>

#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

#include "CombBLAS/CombBLAS.h"

using namespace combblas;

typedef SpParMat<int64_t, double, SpDCCols<int64_t, double>> PMatD;
typedef SpParMat<int64_t, bool, SpDCCols<int64_t, bool>> PMatB;
typedef SpParMat<int64_t, bool, SpDCCols<int32_t, bool>> PMatB32;  // TopDownBFS's Aeff

int main(int argc, char* argv[]) {
  int provided;
  MPI_Init_thread(&argc, &argv, MPI_THREAD_SERIALIZED, &provided);
  int rank;
  MPI_Comm_rank(MPI_COMM_WORLD, &rank);
  if (argc < 4) {
    if (rank == 0) fprintf(stderr, "usage: see the header of ref_bfs_driver.cpp\n");
    MPI_Finalize();
    return 1;
  }
  {
    auto grid = std::make_shared<CommGrid>(MPI_COMM_WORLD, 0, 0);
    PMatD Ad(grid);
    Ad.ParallelReadMM(argv[1], true, maximum<double>());
    PMatB A = Ad;
    PMatB32 Aeff = PMatB32(A);
    typedef SelectMaxSRing<bool, int64_t> SR;
    OptBuf<int32_t, int64_t> optbuf;  // not optimised: the semiring path (TopDownBFS's buffers need OptimizeForGraph500)
    const int64_t n = Aeff.getncol();
    const int64_t nnz = Aeff.getnnz();
    if (rank == 0) printf("ref_bfs_driver: %lld vertices, %lld stored entries\n", (long long)n, (long long)nnz);
    FILE* f = nullptr;
    if (rank == 0 && !(f = fopen(argv[2], "w"))) MPI_Abort(MPI_COMM_WORLD, 1);
    for (int a = 3; a < argc; ++a) {
      const int64_t root = atoll(argv[a]);
      FullyDistVec<int64_t, int64_t> parents(Aeff.getcommgrid(), n, (int64_t)-1);
      FullyDistSpVec<int64_t, int64_t> fringe(Aeff.getcommgrid(), n);
      fringe.SetElement(root, root);
      int iterations = 0;
      while (fringe.getnnz() > 0) {
        fringe.setNumToInd();
        // indexisvalue = false: the values setNumToInd wrote travel with the indices.  With true this
        // overload hands the local kernel a value array it never gathered (SpImpl.cpp:185 reads it).
        fringe = SpMV<SR>(Aeff, fringe, false, optbuf);
        fringe = EWiseMult(fringe, parents, true, (int64_t)-1);
        parents.Set(fringe);
        iterations++;
      }
      if (rank == 0) fprintf(f, "root %lld iterations %d\n", (long long)root, iterations);
      for (int64_t v = 0; v < n; ++v) {
        const int64_t p = parents.GetElement(v);  // collective
        if (rank == 0) fprintf(f, "%lld %lld\n", (long long)v, (long long)p);
      }
    }
    if (f) fclose(f);
  }
  MPI_Finalize();
  return 0;
}
