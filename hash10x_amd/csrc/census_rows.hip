// census_rows.hip — from a batch's gathered keys to rows: the tail of stage_l.hip, stage_p.hip and stage_q.hip (census_rows.hpp).
//   sort     prim_sort_keys_u32 / _u64 on the bits in use;
//   runs     a run of equal keys is one (slot, other) with count = its length (runs.hpp: a galloping search from the run's head); only runs of
//            length >= T are flagged, and in the sibling form no run of slots (2s, 2s + 1);
//   rows     a scan of the flags places the rows (other, count) behind those of the batches before, in the kept result's arrays. Rows per slot
//            = two binary searches in the batch's slot column; their exclusive sum over the command's slots is offsets[].
// Sub-threshold runs never leave the device, and nothing but the run total of a batch comes back to the host.
#include "census_rows.hpp"
#include "runs.hpp"
#include "wave.hpp"

namespace h10x {

// what the sibling test of the run kernel needs: the batch's first slot and the low field's width. Nothing where the test is compiled out
template <bool SIB> struct Siblings {};
template <> struct Siblings<true> { u32 q0; int lb; };

// flag[i] = 1 at the head of a run of at least T equal keys (SIB: that is no sibling pair), cnt[i] = its length there
template <typename K, bool SIB>
__global__ void rows_run_kernel(const K *__restrict__ keys, u64 n, u32 T, Siblings<SIB> sib, u32 *__restrict__ flag, u32 *__restrict__ cnt) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const K k = keys[i];
    u32 f = 0;
    if (!i || keys[i - 1] != k) {
      const u64 c = run_end(keys, n, i, [](K v) { return v; }) - i;
      bool row = c >= T;
      if constexpr (SIB) {
        const u32 a = sib.q0 + (u32)((u64)k >> sib.lb), b = (u32)((u64)k & (((u64)1 << sib.lb) - 1));
        row = row && (a >> 1) != (b >> 1);
      }
      if (row) { f = 1; cnt[i] = (u32)c; }
    }
    flag[i] = f;
  }
}

// the rows of the flagged runs at oOther / oCount [pos[i]] (the caller passes the arrays at the batch's first row; p < runs bounds the stores), their
// slot at oSlot[pos[i]], and the largest count: one atomic per workgroup of a grid of at most ROWS_EMIT_GRID (one per wave of 16384 workgroups, all on
// one word, was 0.75 of the kernel's 0.78 ms per batch on the yeast-like set). The loop is wave-uniform: i0 steps by whole workgroups
template <typename K>
__global__ __launch_bounds__(256) void rows_emit_kernel(const K *__restrict__ keys, u64 n, int lowBits, const u32 *__restrict__ flag, const u32 *__restrict__ cnt,
                                                        const u32 *__restrict__ pos, u64 runs, u32 *__restrict__ oOther, u32 *__restrict__ oCount,
                                                        u32 *__restrict__ oSlot, u32 *__restrict__ maxCount) {
  __shared__ u32 sMax[256 / WAVE];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  u32 mx = 0;
  for (u64 i0 = (u64)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
    const u64 i = i0 + threadIdx.x;
    if (i < n && flag[i]) {
      const K k = keys[i]; const u32 p = pos[i], c = cnt[i];
      if (p < runs) { oOther[p] = (u32)(k & (((K)1 << lowBits) - 1)); oCount[p] = c; oSlot[p] = (u32)(k >> lowBits); }
      mx = mx > c ? mx : c;
    }
  }
  mx = wg_max(mx, sMax);
  if (threadIdx.x == 0 && mx) atomicMax(maxCount, mx);
}

// rowCnt[q] += rows of the batch with slot q (oSlot ascends). A windowed slot comes here once per window, one launch after the other
__global__ void rows_count_kernel(const u32 *__restrict__ oSlot, u64 runs, u32 nq, u32 *__restrict__ rowCnt) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const u64 s = lower_bound(oSlot, (u64)0, runs, q);
  rowCnt[q] += (u32)(upper_bound(oSlot, s, runs, q) - s);
}

int RowTail::begin(Ctx *c_, KeptRows *kept_, u32 T_, u32 nSlots_, bool siblings_) {
  c = c_; kept = kept_; T = T_; nSlots = nSlots_; siblings = siblings_;
  H10X_HIP(c, rowCnt.alloc((size_t)nSlots + 1)); H10X_HIP(c, hipMemsetAsync(rowCnt.p, 0, ((size_t)nSlots + 1) * 4, c->stream));   // (the last stays 0)
  H10X_HIP(c, maxCount.alloc(1)); H10X_HIP(c, hipMemsetAsync(maxCount.p, 0, 4, c->stream));
  return 0;
}

int RowTail::places(const u32 *unitCnt, u64 *place, u64 units, u64 *n) {
  H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, unitCnt, place, units + 1));
  unsigned long long v = 0;
  H10X_TRY(c->readback(&v, place + units, 8)); H10X_TRY(c->syncReadbacks());
  *n = v;
  return 0;
}

int RowTail::keys(u64 n, bool isWide) {
  if (isWide) { ++wide; if (keys64.n < n) { H10X_HIP(c, keys64.alloc(n)); H10X_HIP(c, keys64s.alloc(n)); } }
  else if (keys32.n < n) { H10X_HIP(c, keys32.alloc(n)); H10X_HIP(c, keys32s.alloc(n)); }
  return 0;
}

int RowTail::emit(u64 n, int lowBits, int endBit, u32 slot0, u32 nq) {
  if (endBit <= 32) { H10X_TRY(prim_sort_keys_u32(c, pt, keys32.p, keys32s.p, n, 0, endBit)); return emitKeys(keys32s.p, n, lowBits, slot0, nq); }
  H10X_TRY(prim_sort_keys_u64(c, pt, keys64.p, keys64s.p, n, 0, endBit));
  return emitKeys(keys64s.p, n, lowBits, slot0, nq);
}

template <typename K>
int RowTail::emitKeys(const K *sorted, u64 n, int lowBits, u32 slot0, u32 nq) {
  hipStream_t st = c->stream;
  if (flag.n < n) { H10X_HIP(c, flag.alloc(n)); H10X_HIP(c, cnt.alloc(n)); H10X_HIP(c, pos.alloc(n)); }
  const unsigned gr = (unsigned)hmin<u64>(divUp(n, 256), 16384);
  if (siblings) rows_run_kernel<K, true><<<gr, 256, 0, st>>>(sorted, n, T, Siblings<true>{slot0, lowBits}, flag.p, cnt.p);
  else rows_run_kernel<K, false><<<gr, 256, 0, st>>>(sorted, n, T, Siblings<false>{}, flag.p, cnt.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, pos.p, n));
  u32 lastPos = 0, lastFlag = 0;
  H10X_TRY(c->readback(&lastPos, pos.p + (n - 1), 4)); H10X_TRY(c->readback(&lastFlag, flag.p + (n - 1), 4)); H10X_TRY(c->syncReadbacks());
  const u64 runs = (u64)lastPos + lastFlag;
  if (!runs) return 0;
  H10X_TRY(reserve_keep(c, kept->a, rows, rows + runs)); H10X_TRY(reserve_keep(c, kept->b, rows, rows + runs));
  if (oSlot.n < runs) H10X_HIP(c, oSlot.alloc(runs));
  rows_emit_kernel<K><<<hmin<unsigned>(gr, ROWS_EMIT_GRID), 256, 0, st>>>(sorted, n, lowBits, flag.p, cnt.p, pos.p, runs, kept->a.p + rows, kept->b.p + rows, oSlot.p,
                                                                        maxCount.p);
  H10X_HIP(c, hipGetLastError());
  rows_count_kernel<<<divUp(nq, 256), 256, 0, st>>>(oSlot.p, runs, nq, rowCnt.p + slot0);
  H10X_HIP(c, hipGetLastError());
  rows += runs;
  return 0;
}

int RowTail::finish(u32 *maxCountOut) {
  H10X_HIP(c, kept->offsets.alloc((size_t)nSlots + 1));
  H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, rowCnt.p, kept->offsets.p, (size_t)nSlots + 1));
  H10X_TRY(c->readback(maxCountOut, maxCount.p, 4));
  return c->syncReadbacks();
}

}  // namespace h10x
