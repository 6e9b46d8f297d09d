// census_rows.hpp — the tail the scan-placed censuses share (stage_l.hip --shareGraph, stage_p.hip listShare, stage_q.hip rowLinks). Each stage
// gathers keys slot << lowBits | other into the buffer keys() hands it; rows() does the rest (census_rows.hip): sort, runs of at least T equal
// keys, a scan that places them behind the rows of the batches before, the rows per slot.
#pragma once
#include "common.hpp"
#include "prim.hpp"

namespace h10x {

static constexpr u64 ROWS_DEFAULT_BUDGET = 1ull << 26;     // gathered entries per batch (stage_f.hip's NB_DEFAULT_BUDGET)
static constexpr unsigned ROWS_EMIT_GRID = 2048;          // the grid's limit for a kernel that ends in one atomic per workgroup

// dst holds at least `need` elements; the first `used` are kept (grown by doubling)
template <typename T>
int reserve_keep(Ctx *c, DevBuf<T> &dst, u64 used, u64 need) {
  if (need <= dst.n && dst.p) return 0;
  DevBuf<T> b;
  H10X_HIP(c, b.alloc(hmax<u64>(need, 2 * (u64)dst.n)));
  if (used) H10X_HIP(c, hipMemcpyAsync(b.p, dst.p, (size_t)used * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
  dst.swap(b);
  H10X_HIP(c, hipStreamSynchronize(c->stream));               // the old block goes back to the cache behind the copy
  return 0;
}

struct RowTail {
  Ctx *c = nullptr; KeptRows *kept = nullptr;               // the rows go behind kept->a / kept->b [rows], the offsets to kept->offsets
  u32 T = 1, nSlots = 0; bool siblings = false;             // siblings: a run of slots (2s, 2s + 1) is no row (stage_q.hip)
  DevBuf<u32> keys32, keys32s, flag, cnt, pos, oSlot, rowCnt, maxCount; DevBuf<u64> keys64, keys64s;
  PrimTemp pt;
  u64 rows = 0, entries = 0, nKeys = 0; u32 batches = 0, windows = 0, wide = 0;

  int begin(Ctx *c_, KeptRows *kept_, u32 T_, u32 nSlots_, bool siblings_ = false);   // rowCnt[nSlots + 1] and the maxCount word, zeroed
  // one batch of the cutter: its counters, then the places of its units = the exclusive sum of cnt[0 .. units] (cnt[units] = 0) and their total
  void batch(bool full) { if (!full) { c->nbStats[3] += 1; ++windows; } c->nbStats[2] += 1; ++batches; }
  int places(const u32 *unitCnt, u64 *place, u64 units, u64 *n);
  void gathered(u64 total, u64 n) { c->nbStats[0] += total; c->nbStats[1] += n; entries += total; nKeys += n; }
  // the buffer for n keys the stage's gather fills: keys64.p if wide, else keys32.p
  int keys(u64 n, bool wide);
  // the n gathered keys, slot << lowBits | other on endBit bits, slots [slot0, slot0 + nq) of the command's: sort, run, scan, total, reserve, emit, row count
  int emit(u64 n, int lowBits, int endBit, u32 slot0, u32 nq);
  int finish(u32 *maxCountOut);                             // kept->offsets = the exclusive sum of the rows per slot; the largest count (queued read-backs ride along)

 private:
  template <typename K> int emitKeys(const K *sorted, u64 n, int lowBits, u32 slot0, u32 nq);
};

}  // namespace h10x
