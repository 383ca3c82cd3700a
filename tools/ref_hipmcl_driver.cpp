// ref_hipmcl_driver.cpp -- TEST INFRASTRUCTURE ONLY (fixture generator, never built
// by build() and never on the product path).
//
// Our own driver that links the reference CombBLAS and runs ITS HipMCL pieces
// (Applications/MCL.cpp) on a Matrix Market file, so that the
// tests/golden/hipmcl_*.npz fixtures come from the reference's own run
// (tests/golden/make_hipmcl_golden.py calls it).  The reference's functions are
// reached by including its MCL.cpp with `main` renamed; nothing is copied from it.
//
//   ref_hipmcl_driver <in.mtx> <inflation> <hardThreshold> <selectNum> <recoverNum> <recoverPct> <out>
//
// Rank r writes, with one "global_row global_col value(%.17g)" line per entry (0-based):
//   <out>.adjust.r<r>    AdjustLoops(A)
//   <out>.stoch.r<r>     MakeColStochastic of that
//   <out>.inflate.r<r>   Inflate(power) of that (no renormalisation)
// and, one "vertex label" line per local element of the label vector:
//   <out>.interpret.r<r> Interpret(A)
//   <out>.hipmcl.r<r>    HipMCL(A, param)
// Rank 0 writes <out>.scalars: "chaos <%.17g>" = Chaos of the stochastic matrix.
// HipMCL's own "Iteration# ... chaos: ..." lines go to stdout (the generator parses them).
//
// Compile (the flags oracle/Makefile uses for ref_driver; REF = the reference's
// root, MPI = the MPICH prefix, OBJ = oracle/_ref after `make -C oracle ref`):
//   g++ -O3 -fopenmp -DTHREADED -std=c++14 -w -I$REF/include -I$REF/include/CombBLAS \
//       -I$REF/psort-1.0/include -I$REF/usort/include -I$REF/graph500-1.2/generator/include \
//       -I$REF/Applications -I$MPI/include tools/ref_hipmcl_driver.cpp $OBJ/CommGrid.o $OBJ/MPIType.o \
//       $OBJ/MPIOp.o $OBJ/MemoryPool.o $OBJ/hash.o $OBJ/mmio.o $OBJ/gen_*.o -o ref_hipmcl_driver \
//       -Wl,-rpath,$MPI/lib $MPI/lib/libmpicxx.so $MPI/lib/libmpi.so -lm
// (the MPI libraries by path, as oracle/Makefile's adapter target links them: -L$MPI/lib
// would also pick up that prefix's older libstdc++)
#define main reference_hipmcl_main
#include "MCL.cpp"
#undef main

#include <cstdio>
#include <cstdlib>

typedef SpDCCols<int64_t, double> DCCols;
typedef SpParMat<int64_t, double, DCCols> PMat;

static void dump_matrix(PMat& A, const std::string& out, const char* what, int rank) {
  auto grid = A.getcommgrid();
  const int64_t roff = grid->GetRankInProcCol() * (A.getnrow() / grid->GetGridRows());
  const int64_t coff = grid->GetRankInProcRow() * (A.getncol() / grid->GetGridCols());
  const std::string path = out + "." + what + ".r" + std::to_string(rank);
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

static void dump_labels(FullyDistVec<int64_t, int64_t>& v, const std::string& out, const char* what, int rank) {
  long long n = v.LocArrSize(), before = 0;
  MPI_Exscan(&n, &before, 1, MPI_LONG_LONG, MPI_SUM, MPI_COMM_WORLD);
  if (rank == 0) before = 0;
  const std::string path = out + "." + what + ".r" + std::to_string(rank);
  FILE* f = fopen(path.c_str(), "w");
  if (!f) MPI_Abort(MPI_COMM_WORLD, 1);
  const int64_t* a = v.GetLocArr();
  for (long long i = 0; i < n; ++i) fprintf(f, "%lld %lld\n", before + i, (long long)a[i]);
  fclose(f);
}

int main(int argc, char* argv[]) {
  int provided;
  MPI_Init_thread(&argc, &argv, MPI_THREAD_SERIALIZED, &provided);
  int rank;
  MPI_Comm_rank(MPI_COMM_WORLD, &rank);
  if (argc < 8) {
    if (rank == 0) fprintf(stderr, "usage: see the header of ref_hipmcl_driver.cpp\n");
    MPI_Finalize();
    return 1;
  }
  {
    const std::string out = argv[7];
    HipMCLParam param;
    InitParam(param);
    param.inflation = atof(argv[2]);
    param.prunelimit = atof(argv[3]);
    param.select = atoll(argv[4]);
    param.recover_num = atoll(argv[5]);
    param.recover_pct = atof(argv[6]);
    auto grid = std::make_shared<CommGrid>(MPI_COMM_WORLD, 0, 0);
    PMat A(grid);
    A.ParallelReadMM(argv[1], true, maximum<double>());
    {
      PMat B(A);
      AdjustLoops(B);
      dump_matrix(B, out, "adjust", rank);
      MakeColStochastic(B);
      dump_matrix(B, out, "stoch", rank);
      const double chaos = Chaos(B);
      if (rank == 0) {
        FILE* f = fopen((out + ".scalars").c_str(), "w");
        if (!f) MPI_Abort(MPI_COMM_WORLD, 1);
        fprintf(f, "chaos %.17g\n", chaos);
        fclose(f);
      }
      Inflate(B, param.inflation);
      dump_matrix(B, out, "inflate", rank);
    }
    {
      PMat C(A);
      FullyDistVec<int64_t, int64_t> lab = Interpret(C);
      dump_labels(lab, out, "interpret", rank);
    }
    {
      PMat D(A);
      FullyDistVec<int64_t, int64_t> lab = HipMCL(D, param);
      dump_labels(lab, out, "hipmcl", rank);
    }
  }
  MPI_Finalize();
  return 0;
}
