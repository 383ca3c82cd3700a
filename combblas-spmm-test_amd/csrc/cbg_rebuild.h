// cbg_rebuild.h -- one place where a DCSC tile is built from per-column counts.
//
// Every op that keeps, drops, shifts or moves the entries of a tile (row slices
// and splits, the samples, row concatenation, the MCL prune and loops, the row
// stage of A(ri, ci)) has the same frame around the one kernel that is its own:
// count per column, scan, read the totals, allocate, write jc/cp and the
// entries, close cp.  The frame lives here, in two layers.
//
//   compact_columns    dense exclusive offsets off[0 .. nslots] -> nzc, jc, cp of the
//                      slots with off[i + 1] > off[i] (callers that lay the entries
//                      out themselves: tile_concat_rows, spref_compact)
//   tile_from_columns  per-slot lengths + an emit functor -> the whole tile
//
// A slot is a candidate column: a stored column of the input (ids = its jc) or a
// dense column id (ids = NULL: slot i is column i).  What both layers guarantee:
//   - offsets and positions are 64-bit: a tile may hold 2^31 or more entries;
//   - a slot's entries keep the order its emit writes them in: the primitive never
//     reorders inside a column, and slots keep their order;
//   - a slot of length 0 leaves no column: jc holds survivors only.  The survivors'
//     positions are a scan of "off[i + 1] > off[i]" read straight from the offsets
//     (k_scan_tile's ScanStep load), not of a flag array.  Every caller used to flag
//     "the input column is kept", which equals "length > 0" for a valid DCSC input;
//     a stored EMPTY column of an invalid input tile is now dropped, not copied;
//   - the output is owned by a TileGuard until it is complete: a throw frees it;
//   - one readback (the two totals, gathered side by side, in one copy) and one final
//     synchronisation, after which the
//     caller's temporaries may return to the pool; the scans' temporaries go
//     through a DeferredFree, so a scan level costs no synchronisation;
//   - cp[nzc] is written on the device by the last slot's wave (or thread);
//   - nslots == 0 or no entry at all: the empty tile of tile_alloc_device.
//
// Nothing here knows its callers: they differ in their count kernel and in the
// Emit functor they pass.
#pragma once
#include <algorithm>

#include "cbg_device.h"
#include "cbg_internal.h"

namespace cbg {

// ---------------------------------------------------------------------------
// device pieces
// ---------------------------------------------------------------------------
// slot i's column header if it survives; the last slot closes cp
__device__ __forceinline__ void put_column(int64_t i, int64_t nslots, const int32_t* __restrict__ ids,
                                           const int64_t* __restrict__ off, const int64_t* __restrict__ pos,
                                           int32_t* __restrict__ jc, int64_t* __restrict__ cp) {
  if (i == nslots - 1) cp[pos[nslots]] = off[nslots];
  if (off[i + 1] > off[i]) {
    jc[pos[i]] = ids ? ids[i] : (int32_t)i;
    cp[pos[i]] = off[i];
  }
}

// a wave copies the len entries from position b to oir/oval[dst ...], rows re-based by `sub`
__device__ __forceinline__ void copy_range(const int32_t* __restrict__ ir, const double* __restrict__ val, int64_t b,
                                           int64_t len, int sub, int32_t* __restrict__ oir,
                                           double* __restrict__ oval, int64_t dst) {
  for (int64_t q = lane_id(); q < len; q += WAVE) {
    oir[dst + q] = ir[b + q] - sub;
    oval[dst + q] = val[b + q];
  }
}

// a wave copies those of the len entries from position b that keep() accepts to
// oir/oval[dst ...], in order (ballot ranks), rows mapped by row().
// Keep::by_row: keep(r) looks at the row alone and a dropped entry's value is never
// loaded; else keep(r, v).
template <class Keep, class Row>
__device__ __forceinline__ void copy_filtered(const int32_t* __restrict__ ir, const double* __restrict__ val,
                                              int64_t b, int64_t len, Keep keep, Row row,
                                              int32_t* __restrict__ oir, double* __restrict__ oval, int64_t dst) {
  const int lane = lane_id();
  for (int64_t x0 = 0; x0 < len; x0 += WAVE) {  // the trip count is the wave's: every lane votes
    const int64_t x = x0 + lane;
    int32_t r = 0;
    double v = 0.0;
    bool k = false;
    if (x < len) {
      r = ir[b + x];
      if constexpr (Keep::by_row) {
        k = keep(r);
      } else {
        v = val[b + x];
        k = keep(r, v);
      }
    }
    const unsigned long long m = __ballot(k);
    if (k) {
      const int64_t at = dst + __popcll(m & ((1ull << lane) - 1ull));
      if constexpr (Keep::by_row) v = val[b + x];
      oir[at] = row(r);
      oval[at] = v;
    }
    dst += __popcll(m);
  }
}
struct RowSame {
  __device__ __forceinline__ int32_t operator()(int32_t r) const { return r; }
};

// one wave per slot: lane 0 writes the column header, the wave emits the entries
template <class Emit>
__global__ __launch_bounds__(256) void k_emit_columns(int64_t nslots, const int32_t* __restrict__ ids,
                                                      const int64_t* __restrict__ off,
                                                      const int64_t* __restrict__ pos, Emit emit,
                                                      int32_t* __restrict__ jc, int64_t* __restrict__ cp,
                                                      int32_t* __restrict__ oir, double* __restrict__ oval) {
  // the slot is the wave's: held in a scalar register, so its offsets and the emit's per-slot reads are scalar loads
  const int64_t i = (int64_t)blockIdx.x * (256 / WAVE) + __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  if (i >= nslots) return;
  if (lane_id() == 0) put_column(i, nslots, ids, off, pos, jc, cp);
  const int64_t dst = off[i];
  if (off[i + 1] > dst) emit(i, dst, oir, oval);
}

// ---------------------------------------------------------------------------
// host layers
// ---------------------------------------------------------------------------
// pos[0 .. n] = exclusive scan of (off[i + 1] > off[i]), i < n (cbg_tile.hip)
void scan_nonempty(const int64_t* off, int64_t* pos, int64_t n, hipStream_t s, DeferredFree* df);
// the device words *a, *b and *c (c may be NULL: 0) laid side by side in dev3 and read into host3
// by one copy; the stream is synchronised (cbg_tile.hip)
void read_words(const int64_t* a, const int64_t* b, const int64_t* c, int64_t* dev3, int64_t* host3, hipStream_t s);

// Layer a.  t.nzc, t.jc, t.cp from the offsets (device); m, n and nnz as given; t.ir and
// t.val stay NULL for the caller, who owns t (a TileGuard).  The stream is synchronised
// for the readback of nzc; the kernel that fills jc and cp is then queued on s, and its
// temporaries wait in df: the caller synchronises s and sets df.synced.
// extra (may be NULL): nextra more device words that land in extra_host with that readback
// (a caller that lays the entries out itself reads its nnz here: one copy, one wait).
void compact_columns(int64_t m, int64_t n, int64_t nnz, int64_t nslots, const int32_t* ids, const int64_t* off,
                     cbg_tile& t, hipStream_t s, DeferredFree& df, const int64_t* extra = nullptr,
                     int64_t* extra_host = nullptr, int nextra = 0);

// Layer b.  len[i] (device, nslots values) = the entries slot i will hold;
// emit(i, dst, oir, oval) is called by all 64 lanes of slot i's wave when len[i] > 0 and
// writes exactly len[i] entries at oir/oval[dst ...].  extra (may be NULL): one more device
// word, written by the caller's count kernel, that lands in *extra_host with the totals.
// A throw on the way waits for the stream first: the caller's count kernel may still be
// running on buffers that the caller's frame is about to release.
template <class Emit>
void tile_from_columns(int64_t m, int64_t n, int64_t nslots, const int32_t* ids, const int64_t* len, Emit emit,
                       cbg_tile& out, hipStream_t s, const int64_t* extra = nullptr, int64_t* extra_host = nullptr) {
  if (nslots <= 0) {
    tile_alloc_device(out, m, n, 0, 0);
    return;
  }
  TileGuard o;
  DBuf<int64_t> buf;  // off[0 .. nslots] | pos[0 .. nslots] | the three words read back
  DeferredFree df;
  WaitOnThrow wait{s};  // declared last, so it runs first: before the output and the buffers go
  buf.reset(2 * (nslots + 1) + 3);
  int64_t *off = buf.p, *pos = buf.p + nslots + 1, *words = buf.p + 2 * (nslots + 1);
  exclusive_scan_i64(len, off, nslots, s, &df);
  scan_nonempty(off, pos, nslots, s, &df);
  int64_t tot[3] = {0, 0, 0};
  read_words(off + nslots, pos + nslots, extra, words, tot, s);  // one copy, one wait
  df.synced = true;
  if (extra_host) *extra_host = tot[2];
  tile_alloc_device(o.t, m, n, tot[0], tot[1]);
  if (tot[0] > 0) {
    hipLaunchKernelGGL(k_emit_columns<Emit>, dim3(nblk(nslots, 256 / WAVE)), dim3(256), 0, s, nslots, ids, off, pos, emit,
                       o.t.jc, o.t.cp, o.t.ir, o.t.val);
    CBG_HIP(hipGetLastError());
    CBG_HIP(hipStreamSynchronize(s));  // the temporaries (the caller's too) go back to the pool
  }
  wait.done = true;
  out = o.release();
}

}  // namespace cbg
