// stage_l.hip — the share graph behind --shareGraph: for every block c of a range the blocks d that share at least T good hashes with it.
//
// countShare_c[d] is stage_f.hip's barcode census (codeExplore, hash10x.c:1371-1382): the number of entries d != c in the barcode lists of c's
// good hashes g[0 .. n), repeats as the lists hold them. --codeExplore asks for one barcode and wants every count and the rank that met each
// barcode first; the graph asks for ALL blocks and only for the counts that reach a threshold. So the census runs here in another form:
//   sizes    one wave per block: the entries of its lists in the window (the batches are cut by these), then per LIST the entries that stay
//            (those != c; the lists ascend, so the c's of a list are found by two binary searches);
//   scan     the exclusive sum of the per-list counts is every list's place in the key array: no reservation, and a fixed output order;
//   gather   one wave per list: key = (c - c0) << cbits | d, no rank below it. 32-bit keys where slot and barcode fit, else 64-bit;
//   sort     prim_sort_keys_u32 / _u64 on the bits in use;
//   runs     a run of equal keys is one (c, d) with countShare = its length (found by a galloping search from the run's head); only runs of
//            length >= T are flagged;
//   rows     a scan of the flags places the rows (d, count) behind those of the batches before, in the context's result arrays. Rows per block
//            = two binary searches in the batch's slot column; their exclusive sum over the range is offsets[].
// Sub-threshold runs never leave the device, and nothing but the rows and the offsets is ever copied out. Batches are cut by list entries
// against "neighbour_budget"; a block above it runs alone in windows of barcode index (whole runs each: the lists ascend), as in stage_f.hip.
#include "common.hpp"
#include "prim.hpp"
#include "wave.hpp"

namespace h10x {

static constexpr u64 SG_DEFAULT_BUDGET = 1ull << 26;       // list entries per batch (stage_f.hip's NB_DEFAULT_BUDGET)

// one wave per block c0 + q: size[q] = entries of its good hashes' lists in the window (the block's own included)
__global__ void sg_size_kernel(u32 c0, u32 nq, const u32 *__restrict__ nGood, const u64 *__restrict__ blockOff, const u64 *__restrict__ goodRow,
                               const u32 *__restrict__ rows, u32 rowShift, u32 lo, u32 hi, int full, u64 *__restrict__ size) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u32 q = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (q >= nq) return;
  u32 n; const u64 s = good_list_entries(c0 + q, nGood, blockOff, goodRow, rows, rowShift, lo, hi, full != 0, n);
  if (lane == 0) size[q] = s;
}

// one wave per block c0 + q, a lane per good rank: listCnt[unit] = entries != c of that list in the window. unitBase[q] = first unit of
// block c0 + q (units = good ranks of the batch's blocks in order; unitBase[0] is the batch's base)
__global__ void sg_list_kernel(u32 c0, u32 nq, const u64 *__restrict__ unitBase, const u64 *__restrict__ blockOff, const u64 *__restrict__ goodRow,
                               const u32 *__restrict__ rows, u32 rowShift, u32 lo, u32 hi, int full, u32 *__restrict__ listCnt) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u32 q = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  if (q >= nq) return;
  const u32 code = c0 + q; const u64 o = blockOff[code], u0 = unitBase[q] - unitBase[0];
  const u32 n = (u32)(unitBase[q + 1] - unitBase[q]);
  for (u32 i = lane; i < n; i += WAVE) {
    u64 a, b; list_window(rows, goodRow[o + i], rowShift, lo, hi, full != 0, a, b);
    const u64 s = lower_bound(rows, a, b, code), e = upper_bound(rows, s, b, code);   // the list's own entries of `code`: [s, e)
    listCnt[u0 + i] = (u32)((b - a) - (e - s));
  }
}

// one wave per unit; the list's keys go to [listPos[unit], listPos[unit + 1]) in list order. cap = listPos[units]: a miscount stays in bounds
template <typename K>
__global__ __launch_bounds__(256) void sg_gather_kernel(u32 c0, u32 nq, const u64 *__restrict__ unitBase, const u64 *__restrict__ blockOff,
                                                        const u64 *__restrict__ goodRow, const u32 *__restrict__ rows, u32 rowShift, u32 lo, u32 hi,
                                                        int full, int cbits, const u64 *__restrict__ listPos, u64 cap, K *__restrict__ keys) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u64 base = unitBase[0], units = unitBase[nq] - base;
  const u64 w0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / WAVE, wStride = ((u64)gridDim.x * blockDim.x) / WAVE;
  for (u64 u = w0; u < units; u += wStride) {
    const u32 q = last_le(unitBase, nq, base + u), code = c0 + q, rank = (u32)(u - (unitBase[q] - base));   // (unitBase[0] = base)
    u64 a, b; list_window(rows, goodRow[blockOff[code] + rank], rowShift, lo, hi, full != 0, a, b);
    const K tag = (K)q << cbits;
    u64 p0 = listPos[u];
    for (u64 e = a; e < b; e += WAVE) {                       // wave-uniform trip counts around the ballot
      const u64 j = e + lane;
      u32 cj = 0; bool keep = false;
      if (j < b) { cj = rows[j]; keep = cj != code; }
      const u64 p = wave_place(keep, p0);
      if (keep && p < cap) keys[p] = tag | (K)cj;
    }
  }
}

// flag[i] = 1 at the head of a run of at least T equal keys, cnt[i] = its length there. The run's end is searched for in doubling steps and
// then by bisection (most runs are a few keys long, some thousands: a walk would leave 63 lanes waiting for the longest)
template <typename K>
__global__ void sg_run_kernel(const K *__restrict__ keys, u64 n, u32 T, u32 *__restrict__ flag, u32 *__restrict__ cnt) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const K k = keys[i];
    u32 f = 0;
    if (!i || keys[i - 1] != k) {
      u64 l = i, step = 1;                                    // keys[l] == k; the first r > l with r == n or keys[r] != k
      u64 r = i + 1;
      while (r < n && keys[r] == k) { l = r; step <<= 1; r = l + step; }
      if (r > n) r = n;
      while (r - l > 1) { const u64 m = (l + r) >> 1; if (keys[m] == k) l = m; else r = m; }
      const u64 c = r - i;
      if (c >= T) { f = 1; cnt[i] = (u32)c; }
    }
    flag[i] = f;
  }
}

// the rows of the flagged runs at oBlock / oCount [pos[i]] (the caller passes the arrays at the batch's first row), their slot at oSlot[pos[i]],
// and the largest count: one atomic per workgroup of a grid of at most SG_EMIT_GRID (one per wave of 16384 workgroups, all on one word, was
// 0.75 of the kernel's 0.78 ms per batch on the yeast-like set). The loop is wave-uniform: i0 steps by whole workgroups
static constexpr unsigned SG_EMIT_GRID = 2048;
template <typename K>
__global__ __launch_bounds__(256) void sg_emit_kernel(const K *__restrict__ keys, u64 n, int cbits, const u32 *__restrict__ flag, const u32 *__restrict__ cnt,
                                                      const u32 *__restrict__ pos, u32 *__restrict__ oBlock, u32 *__restrict__ oCount, u32 *__restrict__ oSlot,
                                                      u32 *__restrict__ maxCount) {
  __shared__ u32 sMax[256 / WAVE];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  u32 mx = 0;
  for (u64 i0 = (u64)blockIdx.x * blockDim.x; i0 < n; i0 += stride) {
    const u64 i = i0 + threadIdx.x;
    if (i < n && flag[i]) {
      const K k = keys[i]; const u32 p = pos[i], c = cnt[i];
      oBlock[p] = (u32)(k & (((K)1 << cbits) - 1)); oCount[p] = c; oSlot[p] = (u32)(k >> cbits);
      mx = mx > c ? mx : c;
    }
  }
  mx = wg_max(mx, sMax);
  if (threadIdx.x == 0 && mx) atomicMax(maxCount, mx);
}

// rowCnt[q] += rows of the batch with slot q (oSlot ascends). A windowed block comes here once per window, one launch after the other
__global__ void sg_rowcount_kernel(const u32 *__restrict__ oSlot, u64 runs, u32 nq, u32 *__restrict__ rowCnt) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const u64 s = lower_bound(oSlot, (u64)0, runs, q);
  rowCnt[q] += (u32)(upper_bound(oSlot, s, runs, q) - s);
}

// ---------------------------------------------------------------------------------------------------------- driver
namespace {
struct ShareGraph {
  Ctx *c; u32 T, codeMin, nB; u64 budget;
  std::vector<u64> size; std::vector<u32> nGood;           // per block of the range: list entries, good ranks
  DevBuf<u64> unitBase;                                     // nB + 1: exclusive sum of nGood over the range
  DevBuf<u32> rowCnt;                                       // nB + 1 (the last stays 0)
  DevBuf<u32> maxCount;
  DevBuf<u64> keys64, keys64s, listPos, dSize; DevBuf<u32> keys32, keys32s, listCnt, flag, cnt, pos, oSlot;
  PrimTemp pt;
  u64 rows = 0, entries = 0, nKeys = 0; u32 batches = 0, windows = 0;

  int sizes(u32 c0, u32 nq, u32 lo, u32 hi, bool full, u64 *hSize) {
    hipStream_t st = c->stream;
    H10X_HIP(c, dSize.alloc(nq));
    sg_size_kernel<<<divUp((u64)nq * WAVE, 256), 256, 0, st>>>(c0, nq, c->nGood.p, c->blockOff.p, c->goodRow.p, c->rows.p, (u32)c->rowShift, lo, hi, full ? 1 : 0, dSize.p);
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipMemcpyAsync(hSize, dSize.p, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    return 0;
  }

  // the result arrays hold at least `need` rows (grown by doubling; the rows so far are kept)
  int reserve(u64 need) {
    if (need <= c->sgBlock.n && c->sgBlock.p) return 0;
    const u64 cap = hmax<u64>(need, 2 * (u64)c->sgBlock.n);
    DevBuf<u32> b, k;
    H10X_HIP(c, b.alloc(cap)); H10X_HIP(c, k.alloc(cap));
    if (rows) {
      H10X_HIP(c, hipMemcpyAsync(b.p, c->sgBlock.p, (size_t)rows * 4, hipMemcpyDeviceToDevice, c->stream));
      H10X_HIP(c, hipMemcpyAsync(k.p, c->sgCount.p, (size_t)rows * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    c->sgBlock.swap(b); c->sgCount.swap(k);
    return 0;
  }

  template <typename K>
  int sortAndEmit(DevBuf<K> &keys, DevBuf<K> &keysS, u32 c0, u32 nq, u32 lo, u32 hi, bool full, int cbits, int endBit, u64 units, u64 n) {
    hipStream_t st = c->stream;
    if (keys.n < n) { H10X_HIP(c, keys.alloc(n)); H10X_HIP(c, keysS.alloc(n)); }
    const u64 *ub = unitBase.p + (c0 - codeMin);
    sg_gather_kernel<K><<<(unsigned)hmin<u64>(divUp(units, 4), 65536), 256, 0, st>>>(c0, nq, ub, c->blockOff.p, c->goodRow.p, c->rows.p, (u32)c->rowShift, lo, hi,
                                                                                  full ? 1 : 0, cbits, listPos.p, n, keys.p);
    H10X_HIP(c, hipGetLastError());
    if (sizeof(K) == 4) H10X_TRY(prim_sort_keys_u32(c, pt, (const u32 *)keys.p, (u32 *)keysS.p, n, 0, endBit));
    else H10X_TRY(prim_sort_keys_u64(c, pt, (const u64 *)keys.p, (u64 *)keysS.p, n, 0, endBit));
    if (flag.n < n) { H10X_HIP(c, flag.alloc(n)); H10X_HIP(c, cnt.alloc(n)); H10X_HIP(c, pos.alloc(n)); }
    const unsigned gr = (unsigned)hmin<u64>(divUp(n, 256), 16384);
    sg_run_kernel<K><<<gr, 256, 0, st>>>(keysS.p, n, T, flag.p, cnt.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, pos.p, n));
    u32 lastPos = 0, lastFlag = 0;
    H10X_TRY(c->readback(&lastPos, pos.p + (n - 1), 4)); H10X_TRY(c->readback(&lastFlag, flag.p + (n - 1), 4)); H10X_TRY(c->syncReadbacks());
    const u64 runs = (u64)lastPos + lastFlag;
    if (!runs) return 0;
    H10X_TRY(reserve(rows + runs));
    if (oSlot.n < runs) H10X_HIP(c, oSlot.alloc(runs));
    sg_emit_kernel<K><<<hmin<unsigned>(gr, SG_EMIT_GRID), 256, 0, st>>>(keysS.p, n, cbits, flag.p, cnt.p, pos.p, c->sgBlock.p + rows, c->sgCount.p + rows, oSlot.p, maxCount.p);
    sg_rowcount_kernel<<<divUp(nq, 256), 256, 0, st>>>(oSlot.p, runs, nq, rowCnt.p + (c0 - codeMin));
    H10X_HIP(c, hipGetLastError());
    rows += runs;
    return 0;
  }

  // blocks [c0, c0 + nq) in the window [lo, hi); total = list entries gathered
  int batch(u32 c0, u32 nq, u32 lo, u32 hi, bool full, u64 total) {
    hipStream_t st = c->stream;
    if (!full) { c->nbStats[3] += 1; ++windows; }             // one window of a block above the budget
    c->nbStats[2] += 1; ++batches;
    if (!total) return 0;
    if (total >= 0xFFFFFFFFull) return c->fail("shareGraph: %llu list entries in one batch, beyond 2^32 (block %u alone)", (u64)total, c0);
    u64 units = 0; for (u32 q = 0; q < nq; ++q) units += nGood[c0 - codeMin + q];
    const u64 *ub = unitBase.p + (c0 - codeMin);
    if (listCnt.n < units + 1) { H10X_HIP(c, listCnt.alloc(units + 1)); H10X_HIP(c, listPos.alloc(units + 1)); }
    H10X_HIP(c, hipMemsetAsync(listCnt.p + units, 0, 4, st));
    sg_list_kernel<<<divUp((u64)nq * WAVE, 256), 256, 0, st>>>(c0, nq, ub, c->blockOff.p, c->goodRow.p, c->rows.p, (u32)c->rowShift, lo, hi, full ? 1 : 0, listCnt.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, listCnt.p, listPos.p, units + 1));
    unsigned long long n = 0;
    H10X_TRY(c->readback(&n, listPos.p + units, 8)); H10X_TRY(c->syncReadbacks());
    if (n > total) return c->fail("shareGraph: %llu keys of %llu list entries", n, (u64)total);
    c->nbStats[0] += total; c->nbStats[1] += n; entries += total; nKeys += n;
    if (!n) return 0;
    const int cbits = keyBits(c->nBlocks), endBit = cbits + keyBits(nq - 1);
    if (endBit <= 32) return sortAndEmit<u32>(keys32, keys32s, c0, nq, lo, hi, full, cbits, endBit, units, n);
    return sortAndEmit<u64>(keys64, keys64s, c0, nq, lo, hi, full, cbits, endBit, units, n);
  }

  int run() {
    hipStream_t st = c->stream;
    size.resize(nB); nGood.resize(nB);
    H10X_TRY(sizes(codeMin, nB, 0, c->nBlocks, true, size.data()));
    H10X_HIP(c, hipMemcpyAsync(nGood.data(), c->nGood.p + codeMin, (size_t)nB * 4, hipMemcpyDeviceToHost, st));
    // unitBase: nGood of the range with a zero behind it, summed
    DevBuf<u32> g; H10X_HIP(c, g.alloc((size_t)nB + 1)); H10X_HIP(c, unitBase.alloc((size_t)nB + 1));
    H10X_HIP(c, hipMemcpyAsync(g.p, c->nGood.p + codeMin, (size_t)nB * 4, hipMemcpyDeviceToDevice, st));
    H10X_HIP(c, hipMemsetAsync(g.p + nB, 0, 4, st));
    H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, g.p, unitBase.p, (size_t)nB + 1));
    H10X_HIP(c, rowCnt.alloc((size_t)nB + 1)); H10X_HIP(c, hipMemsetAsync(rowCnt.p, 0, ((size_t)nB + 1) * 4, st));
    H10X_HIP(c, maxCount.alloc(1)); H10X_HIP(c, hipMemsetAsync(maxCount.p, 0, 4, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    H10X_TRY(cut_batches(size.data(), nB, c->nBlocks, budget,
                         [&](u32 q, u32 lo, u32 hi, u64 *records) { return sizes(codeMin + q, 1, lo, hi, false, records); },
                         [&](u32 q0, u32 n, u32 lo, u32 hi, bool full, u64 total) { return batch(codeMin + q0, n, lo, hi, full, total); }));
    H10X_HIP(c, c->sgOffsets.alloc((size_t)nB + 1));
    return prim_exclusive_scan_u32_u64(c, pt, rowCnt.p, c->sgOffsets.p, (size_t)nB + 1);
  }
};
}  // namespace

void stageL_release(Ctx *c) {
  c->haveShareGraph = false; c->sgRows = 0; c->sgCodeMin = c->sgCodeMax = 0;
  c->sgBlock.release(); c->sgCount.release(); c->sgOffsets.release();
}

int stageL_run(Ctx *c, int64_t minShare, u32 codeMin, u32 codeMax, h10x_share_graph_info *info) {
  stageL_release(c);
  H10X_TRY(ce_check(c, "shareGraph", minShare));
  if (codeMax > c->nBlocks) return c->fail("!! shareGraph codeMax %u beyond nBlocks %u", codeMax, c->nBlocks);
  if (!codeMax) codeMax = c->nBlocks;                         // as --cluster 1 0
  if (codeMin > codeMax) codeMin = codeMax;                   // an empty graph
  memset(info, 0, sizeof *info);
  info->codeMin = codeMin; info->codeMax = codeMax; info->nBlocks = c->nBlocks;
  ShareGraph g; g.c = c; g.T = (u32)hmin<int64_t>(minShare, 0xFFFFFFFFll); g.codeMin = codeMin; g.nB = codeMax - codeMin;
  g.budget = c->optNbBudget > 0 ? (u64)c->optNbBudget : SG_DEFAULT_BUDGET;
  if (!g.nB) {
    H10X_HIP(c, c->sgOffsets.alloc(1)); H10X_HIP(c, hipMemsetAsync(c->sgOffsets.p, 0, 8, c->stream));
  } else {
    const int rc = g.run();
    if (rc) { stageL_release(c); return rc; }
    u32 mx = 0;
    H10X_TRY(c->readback(&mx, g.maxCount.p, 4)); H10X_TRY(c->syncReadbacks());
    info->maxCount = mx;
  }
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  c->haveShareGraph = true; c->sgRows = g.rows; c->sgCodeMin = codeMin; c->sgCodeMax = codeMax;
  info->rows = g.rows; info->listEntries = g.nKeys; info->entriesRead = g.entries; info->batches = g.batches; info->windows = g.windows;
  return 0;
}

// offsets[codeMax - codeMin + 1] and the first min(cap, rows) rows of the kept graph, to host (toDevice = 0) or device memory; any may be null
int stageL_get(Ctx *c, u64 *offsets, u32 *block, u32 *count, u64 cap, int toDevice) {
  if (!c->haveShareGraph) return c->fail("shareGraph: no graph is kept (run it first; a new range, --clusterSplit and a new state release it)");
  const hipMemcpyKind kind = toDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t m = (size_t)hmin<u64>(cap, c->sgRows);
  if (offsets) H10X_HIP(c, hipMemcpyAsync(offsets, c->sgOffsets.p, ((size_t)(c->sgCodeMax - c->sgCodeMin) + 1) * 8, kind, c->stream));
  if (m && block) H10X_HIP(c, hipMemcpyAsync(block, c->sgBlock.p, m * 4, kind, c->stream));
  if (m && count) H10X_HIP(c, hipMemcpyAsync(count, c->sgCount.p, m * 4, kind, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace h10x
