// stage_l.hip — the share graph behind --shareGraph: for every block c of a range the blocks d that share at least T good hashes with it.
//
// countShare_c[d] is stage_f.hip's barcode census (codeExplore, hash10x.c:1371-1382): the number of entries d != c in the barcode lists of c's
// good hashes g[0 .. n), repeats as the lists hold them. --codeExplore asks for one barcode and wants every count and the rank that met each
// barcode first; the graph asks for ALL blocks and only for the counts that reach a threshold. So the census runs here in another form:
//   sizes    one wave per block: the entries of its lists in the window (the batches are cut by these), then per LIST the entries that stay
//            (those != c; the lists ascend, so the c's of a list are found by two binary searches);
//   scan     the exclusive sum of the per-list counts is every list's place in the key array: no reservation, and a fixed output order;
//   gather   one wave per list: key = (c - c0) << cbits | d, no rank below it. 32-bit keys where slot and barcode fit, else 64-bit;
//   tail     census_rows.hip: the keys sorted, a run of equal keys is one (c, d) with countShare = its length, the runs of length >= T placed by a
//            scan as rows (d, count) behind those of the batches before in the context's result arrays, the rows per block summed to offsets[].
// Sub-threshold runs never leave the device, and nothing but the rows and the offsets is ever copied out. Batches are cut by list entries
// against "neighbour_budget"; a block above it runs alone in windows of barcode index (whole runs each: the lists ascend), as in stage_f.hip.
#include "census_rows.hpp"
#include "wave.hpp"

namespace h10x {

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

// ---------------------------------------------------------------------------------------------------------- driver
namespace {
struct ShareGraph {
  Ctx *c; u32 codeMin, nB; u64 budget;
  std::vector<u64> size; std::vector<u32> nGood;           // per block of the range: list entries, good ranks
  DevBuf<u64> unitBase;                                     // nB + 1: exclusive sum of nGood over the range
  DevBuf<u64> listPos, dSize; DevBuf<u32> listCnt;
  RowTail tail;

  int sizes(u32 c0, u32 nq, u32 lo, u32 hi, bool full, u64 *hSize) {
    hipStream_t st = c->stream;
    H10X_HIP(c, dSize.alloc(nq));
    sg_size_kernel<<<divUp((u64)nq * WAVE, 256), 256, 0, st>>>(c0, nq, c->nGood.p, c->blockOff.p, c->goodRow.p, c->rows.p, (u32)c->rowShift, lo, hi, full ? 1 : 0, dSize.p);
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipMemcpyAsync(hSize, dSize.p, (size_t)nq * 8, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    return 0;
  }

  template <typename K>
  int gather(K *keys, u32 c0, u32 nq, u32 lo, u32 hi, bool full, int cbits, u64 units, u64 n) {
    sg_gather_kernel<K><<<(unsigned)hmin<u64>(divUp(units, 4), 65536), 256, 0, c->stream>>>(c0, nq, unitBase.p + (c0 - codeMin), c->blockOff.p, c->goodRow.p, c->rows.p,
                                                                                         (u32)c->rowShift, lo, hi, full ? 1 : 0, cbits, listPos.p, n, keys);
    H10X_HIP(c, hipGetLastError());
    return 0;
  }

  // blocks [c0, c0 + nq) in the window [lo, hi); total = list entries gathered
  int batch(u32 c0, u32 nq, u32 lo, u32 hi, bool full, u64 total) {
    hipStream_t st = c->stream;
    tail.batch(full);                                         // (a window: of a block above the budget)
    if (!total) return 0;
    if (total >= 0xFFFFFFFFull) return c->fail("shareGraph: %llu list entries in one batch, beyond 2^32 (block %u alone)", (u64)total, c0);
    u64 units = 0; for (u32 q = 0; q < nq; ++q) units += nGood[c0 - codeMin + q];
    if (listCnt.n < units + 1) { H10X_HIP(c, listCnt.alloc(units + 1)); H10X_HIP(c, listPos.alloc(units + 1)); }
    H10X_HIP(c, hipMemsetAsync(listCnt.p + units, 0, 4, st));
    sg_list_kernel<<<divUp((u64)nq * WAVE, 256), 256, 0, st>>>(c0, nq, unitBase.p + (c0 - codeMin), c->blockOff.p, c->goodRow.p, c->rows.p, (u32)c->rowShift, lo, hi,
                                                              full ? 1 : 0, listCnt.p);
    H10X_HIP(c, hipGetLastError());
    u64 n = 0;
    H10X_TRY(tail.places(listCnt.p, listPos.p, units, &n));
    if (n > total) return c->fail("shareGraph: %llu keys of %llu list entries", n, (u64)total);
    tail.gathered(total, n);
    if (!n) return 0;
    const int cbits = keyBits(c->nBlocks), endBit = cbits + keyBits(nq - 1);
    H10X_TRY(tail.keys(n, endBit > 32));
    H10X_TRY(endBit > 32 ? gather(tail.keys64.p, c0, nq, lo, hi, full, cbits, units, n) : gather(tail.keys32.p, c0, nq, lo, hi, full, cbits, units, n));
    return tail.emit(n, cbits, endBit, c0 - codeMin, nq);
  }

  int run(u32 T, u32 *maxCount) {
    hipStream_t st = c->stream;
    size.resize(nB); nGood.resize(nB);
    H10X_TRY(sizes(codeMin, nB, 0, c->nBlocks, true, size.data()));
    H10X_HIP(c, hipMemcpyAsync(nGood.data(), c->nGood.p + codeMin, (size_t)nB * 4, hipMemcpyDeviceToHost, st));
    // unitBase: nGood of the range with a zero behind it, summed
    DevBuf<u32> g; H10X_HIP(c, g.alloc((size_t)nB + 1)); H10X_HIP(c, unitBase.alloc((size_t)nB + 1));
    H10X_HIP(c, hipMemcpyAsync(g.p, c->nGood.p + codeMin, (size_t)nB * 4, hipMemcpyDeviceToDevice, st));
    H10X_HIP(c, hipMemsetAsync(g.p + nB, 0, 4, st));
    H10X_TRY(prim_exclusive_scan_u32_u64(c, tail.pt, g.p, unitBase.p, (size_t)nB + 1));
    H10X_TRY(tail.begin(c, &c->sg, T, nB));
    H10X_HIP(c, hipStreamSynchronize(st));
    H10X_TRY(cut_batches(size.data(), nB, c->nBlocks, budget,
                         [&](u32 q, u32 lo, u32 hi, u64 *records) { return sizes(codeMin + q, 1, lo, hi, false, records); },
                         [&](u32 q0, u32 n, u32 lo, u32 hi, bool full, u64 total) { return batch(codeMin + q0, n, lo, hi, full, total); }));
    return tail.finish(maxCount);
  }
};
}  // namespace

void stageL_release(Ctx *c) { c->sg.release(); c->sgCodeMin = c->sgCodeMax = 0; }

int stageL_run(Ctx *c, int64_t minShare, u32 codeMin, u32 codeMax, h10x_share_graph_info *info) {
  stageL_release(c);
  H10X_TRY(ce_check(c, "shareGraph", minShare));
  if (codeMax > c->nBlocks) return c->fail("!! shareGraph codeMax %u beyond nBlocks %u", codeMax, c->nBlocks);
  if (!codeMax) codeMax = c->nBlocks;                         // as --cluster 1 0
  if (codeMin > codeMax) codeMin = codeMax;                   // an empty graph
  memset(info, 0, sizeof *info);
  info->codeMin = codeMin; info->codeMax = codeMax; info->nBlocks = c->nBlocks;
  ShareGraph g; g.c = c; g.codeMin = codeMin; g.nB = codeMax - codeMin;
  g.budget = c->optNbBudget > 0 ? (u64)c->optNbBudget : ROWS_DEFAULT_BUDGET;
  if (!g.nB) {
    H10X_HIP(c, c->sg.offsets.alloc(1)); H10X_HIP(c, hipMemsetAsync(c->sg.offsets.p, 0, 8, c->stream));
  } else {
    u32 mx = 0;
    const int rc = g.run((u32)hmin<int64_t>(minShare, 0xFFFFFFFFll), &mx);
    if (rc) { stageL_release(c); return rc; }
    info->maxCount = mx;
  }
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  c->sg.have = true; c->sg.rows = g.tail.rows; c->sg.lists = g.nB; c->sgCodeMin = codeMin; c->sgCodeMax = codeMax;
  info->rows = g.tail.rows; info->listEntries = g.tail.nKeys; info->entriesRead = g.tail.entries; info->batches = g.tail.batches; info->windows = g.tail.windows;
  return 0;
}

int stageL_get(Ctx *c, u64 *offsets, u32 *block, u32 *count, u64 cap, int toDevice) {
  return c->sg.get(c, offsets, block, count, cap, toDevice, "shareGraph: no graph is kept (run it first; a new range, --clusterSplit and a new state release it)");
}

}  // namespace h10x
