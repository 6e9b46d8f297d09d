// stage_c_host.hip — the host driver of --cluster: stands for the OMP loop over barcodes (hash10x.c:1241-1261) around codeClusterFind
// and codeClusterReadMerge (hash10x.c:770-868).
//
// stageC_cluster walks the context's block segments; per contiguous range cluster_local_range chooses the placement of first[]
// (dense, ranked, translated, dense on an HBM slot), sorts the blocks into launch classes by working-set size
// (cluster_classify_kernel), sizes the grids, handle slots and scratch, runs the classes side by side on forked streams (the
// whole-CU class resident before the main launch, a second wind behind it), re-runs the blocks whose tables overflowed in the next
// larger class, and hands the result words to the tail. The kernels themselves live in stage_c.hip, which launches them
// (stageC_launchCluster, stageC_clusterTail); --hashDepthRange is stage_c_good.hip, --clusterSplit stage_c_split.hip.
#include "cluster.hpp"
#include <chrono>

namespace h10x {

constexpr int CL_THREADS_SMALL = 1024;                     // <= 79 KB working sets, two workgroups per CU
constexpr int CL_THREADS_HUGE = 1024;                      // the whole LDS of a CU, one workgroup per CU
constexpr u32 RES_COUNT_MAX = (1u << 24) - 1;               // list lengths beyond this do not fit the word: refused by stageC_cluster
constexpr u32 RANKED_FIRST_PER_RANK = 6;                    // ranked placement: first[] entries budgeted per rank when a block is classified
                                                           // (3-7 barcodes present per rank on the synthetic sets); the kernel then takes
                                                           // whatever the budget leaves, and a block that still overflows is re-run with
                                                           // first[] on an HBM slot
__host__ __device__ inline u32 rankedFirstEstimate(u32 nBarcodes, u32 n) { const u64 e = (u64)RANKED_FIRST_PER_RANK * n; return e < nBarcodes ? (u32)e : nBarcodes; }
// … and, where the entries of the block's lists are known (classification): a seventh of them (6-8 % on the yeast-like
// sets, more on deeper ones), whichever is larger. Erring low is cheap: the ranked kernel knows the true number right
// after its bitmap pass and hands the block on before the list loop.
__host__ __device__ inline u32 rankedFirstEstimateE(u32 nBarcodes, u32 n, u32 entries, u32 div = 7) { const u32 a = rankedFirstEstimate(nBarcodes, n), b = entries / div; const u32 m = a > b ? a : b; return m < nBarcodes ? m : nBarcodes; }
__host__ __device__ inline bool translatedFits(u32 S, u32 S2, u32 est, u32 entries, u32 nBarcodes) {      // classification: do the tables hold the barcodes expected in the block's lists?
  if (!S) return false;
  if ((size_t)S >= 2 * (size_t)(entries < nBarcodes ? entries : nBarcodes)) return true;
  const size_t capacity = S2 ? (size_t)(S - S / 8) + (S2 - S2 / 8) : (size_t)S - S / 8;
  return capacity >= (size_t)est + est / 8;
}

// launch classes by working-set size: 0 = half a CU's LDS (barcodes with many ranks run their list loop on fewer waves:
// histWaves), 2 = the whole LDS of a CU, 3 = HBM scratch (class 1 is no longer used)
__global__ void cluster_classify_kernel(const h10x_block *__restrict__ blocks, const u32 *__restrict__ nGood, const u32 *__restrict__ entries, u32 codeMin, u32 codeMax,
                                        u32 nBlocks /* LDS entries of first[] (ranked, translated: barcodes of the data set) */, int ranked /* 1 ranked, 3 translated */, u32 hashMinSlots, u32 maxTrRanks, u32 firstCap, u32 bmWords, u32 waves0, size_t budget0, size_t budgetSmall, size_t budgetBig, u32 bigRanks, u32 estDiv /* translated placement: a block's barcodes are taken to be this fraction of its list entries */,
                                        u32 *__restrict__ list0, u32 *__restrict__ list1, u32 *__restrict__ list2, u32 *__restrict__ list3,
                                        u32 *__restrict__ listBig /* blocks with more ranks than the small replay class holds: counts[9] */, u32 *__restrict__ counts, unsigned long long *__restrict__ work,
                                        u32 *__restrict__ raw /* Ctx::clusterRaw: the two words of every block of the range start at zero (blocks without good hashes say nothing) */) {
  const u32 c = codeMin + blockIdx.x * blockDim.x + threadIdx.x;
  if (c < codeMax) { raw[2 * (size_t)c] = 0; raw[2 * (size_t)c + 1] = 0; }
  const int lane = threadIdx.x & (WAVE - 1);
  const u32 n = c < codeMax ? nGood[c] : 0;
  int cls = -1; u32 nRead = 0;
  if (n) {
    nRead = blocks[c].nRead;
    if (ranked == 3) {                             // translated placement: the table of pass A must hold the barcodes expected in the block's lists
      u32 S, S2, nW; bool compact;
      translatedShape(n, waves0, budget0, hashMinSlots, entries[c], nBlocks, firstCap, S, S2, nW, compact);
      if (n > maxTrRanks) cls = 3;                       // (its handles would not fit the workgroup's HBM slot)
      // (a sixth of the entries, not a seventh as in the ranked placement: the blocks in between would run in the half-CU class on a second table and
      //  with few list-loop waves — they are faster with a CU to themselves: full configs[2] 583 -> 567 ms, 17 % of the blocks in the whole-CU class
      //  instead of 8 %; at a fifth the whole-CU class holds more than half of the CUs and the launches no longer overlap: 890 ms)
      else if (translatedFits(S, S2, rankedFirstEstimateE(nBlocks, n, entries[c], estDiv), entries[c], nBlocks)) cls = 0;
      else { translatedShape(n, CL_THREADS_HUGE / WAVE, budgetBig, hashMinSlots, entries[c], nBlocks, firstCap, S, S2, nW, compact); cls = S ? 2 : 3; }
    }
    else if (histWaves(ranked ? rankedFirstEstimateE(nBlocks, n, entries[c]) : nBlocks, n, waves0, bmWords, budget0)) cls = 0;
    else if (histWaves(ranked ? rankedFirstEstimate(nBlocks, n) : nBlocks, n, CL_THREADS_HUGE / WAVE, bmWords, budgetBig)) cls = 2;
    else cls = 3;
  }
  // the largest barcodes of the main class go to the front of its work queue (list1, handed out before list0): the launch
  // then does not end on a workgroup that drew a big one last. (Ordering the WHOLE queue by size was measured 17 % slower:
  // like-sized workgroups run their phases in step.)
  if (cls == 0 && n > bigRanks) cls = 1;
  if (!n && c < codeMax && blocks[c].nSubCluster) nRead = blocks[c].nRead;   // no good hashes, but clusters in its file: the read merge still runs on it (hash10x.c:1252)
  for (int s = 32; s; s >>= 1) nRead = max(nRead, (u32)__shfl_xor((int)nRead, s));
  if (lane == 0 && nRead) atomicMax(&counts[8], nRead);
  {                                                          // most ranks of a block per LDS class: the translated placement sizes its handle slots by them
    u32 n0 = (cls == 0 || cls == 1) ? n : 0u, n2 = cls == 2 ? n : 0u;
    for (int s = 32; s; s >>= 1) { n0 = max(n0, (u32)__shfl_xor((int)n0, s)); n2 = max(n2, (u32)__shfl_xor((int)n2, s)); }
    if (lane == 0) { if (n0) atomicMax(&counts[12], n0); if (n2) atomicMax(&counts[13], n2); }
  }
  if (work) {                                            // work of the half-CU classes and of the whole-CU class (list entries + a charge per rank): the launches split the CUs by it
    unsigned long long w0 = (cls == 0 || cls == 1) ? (unsigned long long)entries[c] + 64ull * n : 0ull, w2 = cls == 2 ? (unsigned long long)entries[c] + 64ull * n : 0ull;
    for (int s = 32; s; s >>= 1) { w0 += __shfl_xor(w0, s); w2 += __shfl_xor(w2, s); }
    if (lane == 0) { if (w0) atomicAdd(&work[0], w0); if (w2) atomicAdd(&work[1], w2); }
  }
  {
    const u64 bal = __ballot(n > REPLAY_SMALL);
    if (bal) {
      u32 base = 0;
      if (lane == 0) base = atomicAdd(&counts[9], (u32)__popcll(bal));
      base = (u32)__shfl((int)base, 0);
      if (n > REPLAY_SMALL) listBig[base + (u32)__popcll(bal & ((1ULL << lane) - 1))] = c;
    }
  }
  u32 *const lists[4] = {list0, list1, list2, list3};
#pragma unroll
  for (int k = 0; k < 4; ++k) {                              // one atomic per wave and class
    const u64 bal = __ballot(cls == k);
    if (!bal) continue;
    u32 base = 0;
    if (lane == 0) base = atomicAdd(&counts[k], (u32)__popcll(bal));
    base = (u32)__shfl((int)base, 0);
    if (cls == k) lists[k][base + (u32)__popcll(bal & ((1ULL << lane) - 1))] = c;
  }
}

// one contiguous range of LOCAL block numbers; `more` = a further range of the same command has run before (counters add up)
static int cluster_local_range(Ctx *c, int codeMin, int codeMax, int threshold, bool more) {
  hipStream_t st = c->stream;
  const u32 nGlobal = c->sharded ? c->nBlocksGlobal : c->nBlocks;
  c->tstart(T_CLUSTER);
  const u32 span = (u32)(codeMax - codeMin);
  DevBuf<u32> list0, list1, list2, list3, listBig; DevBuf<u64> term;
  H10X_HIP(c, list0.alloc(span)); H10X_HIP(c, list1.alloc(span)); H10X_HIP(c, list2.alloc(span)); H10X_HIP(c, list3.alloc(span)); H10X_HIP(c, listBig.alloc(span));
  // every small counter of the command in one range of the zeroed arena (Ctx::zeros): counts[0..3] class sizes, [4] [6] [7] work
  // queue positions, [8] largest nRead, [10] [11] overflowed blocks (lists A, B); stats[0..7] the work counters
  ZeroScope zeroScope(c); H10X_TRY(zeroScope.rc);
  struct { u64 *p; } zeroed{(u64 *)c->zeros(2 * (8 + 8 + 2))}; if (!zeroed.p) return -1;
  H10X_HIP(c, term.alloc(c->nEntries));                      // (+ work of the half-CU and the whole-CU classes)
  // the --verbose figures of every block: cleared as a whole when first used on these blocks, per range by the classification below
  if (c->clusterRaw.n != 2 * (size_t)c->nBlocks) { c->haveClusterRaw = false; H10X_HIP(c, c->clusterRaw.alloc(2 * (size_t)c->nBlocks)); H10X_HIP(c, hipMemsetAsync(c->clusterRaw.p, 0, 8 * (size_t)c->nBlocks, st)); }
  struct { u32 *p; } counts{(u32 *)zeroed.p}; struct { u64 *p; } stats{zeroed.p + 8};   // counts[12] [13]: most ranks of a block in the half-CU classes / the whole-CU class (sizes the handle slots)
  const size_t budgetSmall = c->optClusterLds > 0 ? (size_t)c->optClusterLds : 80 * 1024 - 1024;
  const size_t budgetBig = c->optClusterLds > 0 ? (size_t)c->optClusterLds : 160 * 1024 - 1024;
  const int threads0 = c->optClusterThreads0 == 512 ? 512 : (c->optClusterThreads0 == 768 ? 768 : 1024);   // tuning knobs for class 0
  const size_t budget0 = c->optClusterLds > 0 ? (size_t)c->optClusterLds : (c->optClusterBudget0 > 0 ? (size_t)c->optClusterBudget0 : budgetSmall);
  // Placement of first[] (FirstDense / FirstRanked / SlotTable + FirstSlots): dense in LDS while 2 B per barcode of the data set is
  // small; ranked in LDS while the presence bitmap + prefix (3/16 B per barcode) leaves room for the rest; translated (handles
  // into a table in LDS) up to 2^22 barcodes (beyond that the 10-bit tag needs more slots than LDS has); dense on a per-workgroup
  // HBM slot (L2/MALL resident, atomics + L1-bypassing loads) as the last resort and for blocks whose LDS tables filled up twice.
  const u32 bmWordsAll = (nGlobal + 31) / 32;
  int hashBits = 1; while (hashBits < 32 && (1ull << hashBits) < (unsigned long long)nGlobal) ++hashBits;
  const u32 hashMinSlots = hashBits > 10 ? 4u << (hashBits - 10) : 0u;       // 10-bit tag: buckets >= 2^(b-10)
  // The ranked form reads the lists twice but needs no probing (100 k-barcode set: 39 ms against 56 translated), so it is TRIED wherever the
  // bitmap + prefix leave the whole-CU class any room (up to 100 KB of them: 546 k barcodes) and kept unless the classification then
  // sends more than a few blocks to the HBM-scratch class; up to 48 KB (262 k barcodes) it is taken as before.
  const bool rankedSure = (size_t)bmWordsAll * 6 <= 48 * 1024, rankedTry = !rankedSure && (size_t)bmWordsAll * 6 <= 100 * 1024 && hashBits <= 22;
  int firstMode = (size_t)nGlobal * 2 <= 48 * 1024 ? 0 : (rankedSure || rankedTry ? 1 : (hashBits <= 22 ? 4 : 2));
  if (c->optFirstGlobal == 1) firstMode = 2; else if (c->optFirstGlobal == 2) firstMode = 1;                                          // test knobs
  else if ((c->optFirstGlobal == 3 || c->optFirstGlobal == 4) && hashBits <= 22) firstMode = 4;                                        // (3: round 3's one-pass hashed table, replaced by the translated placement)
  // translated placement: u16 per list on a workgroup's handle slot (a multiple of 64 that holds the longest list), ranks per slot
  u32 hStride = 64; while (hStride < c->maxGoodDepth && hStride < (1u << 24)) hStride <<= 1;   // (a power of two: a handle's position tells its rank)
  const size_t trSlotCapBytes = (size_t)32 << 20;
  const u32 maxTrRanks = (u32)hmin<size_t>(0xFFFFFFFFu, trSlotCapBytes / ((size_t)hStride * 2));
  const bool packed = c->optTrPacked != 0;                   // translated placement: the packed form (several lists per wave instruction, round 5) unless the knob says 0
  // a workgroup's handle slot: the handles of its largest block (ranks x the slot's list stride; + 256: the packed form's class regions start at multiples of 64), then the waves' queues.
  // Sized per launch class by the largest block THAT class holds and by its waves (round 4 took the context's largest block and 16 waves for every class: tens of GB on sets
  // with a few giant barcodes that never run here); blocks handed on by the half-CU class run in the whole-CU class, whose slots therefore cover both
  auto trSlotFor = [&](u32 maxRanks, u32 waves) { return (size_t)hmin<u32>(hmax<u32>(maxRanks, 1u), maxTrRanks) * hStride + 256 + (size_t)waves * TR_QUEUE * 4; };
  const u32 firstCap = c->optFirstCap > 0 ? (u32)c->optFirstCap : 0u;      // test knob only
  u32 hc[14]; u64 hw[2] = {0, 0}; u32 nFirstLds = 0, bmWords = 0;
  for (int attempt = 0; attempt < 2; ++attempt) {
    nFirstLds = firstMode == 0 ? nGlobal : 0;
    bmWords = firstMode == 1 ? bmWordsAll : 0;
    cluster_classify_kernel<<<divUp(span, 256), 256, 0, st>>>(c->blocks.p, c->nGood.p, c->goodEntries.p, (u32)codeMin, (u32)codeMax,
                                                            firstMode == 1 || firstMode >= 3 ? nGlobal : nFirstLds, firstMode == 1 ? 1 : (firstMode == 4 ? 3 : 0), hashMinSlots, maxTrRanks, firstCap,
                                                            bmWords, (u32)threads0 / WAVE, budget0, budgetSmall, budgetBig, c->optBigRanks > 0 ? (u32)c->optBigRanks : c->meanGood + c->meanGood / 2, c->optTrEstDiv > 0 ? (u32)c->optTrEstDiv : 6u,
                                                            list0.p, list1.p, list2.p, list3.p, listBig.p, counts.p, (unsigned long long *)(zeroed.p + 16), c->clusterRaw.p);
    H10X_TRY(c->readback(hc, counts.p, 56));
    H10X_TRY(c->readback(hw, zeroed.p + 16, 16));
    H10X_TRY(c->syncReadbacks());
    const u32 classified = hc[0] + hc[1] + hc[2] + hc[3];
    if (attempt || !rankedTry || c->optFirstGlobal || firstMode != 1 || hc[3] <= 16 + classified / 200) break;
    firstMode = 4;                                           // too many blocks without room beside the bitmap: the translated placement after all
    H10X_HIP(c, hipMemsetAsync(counts.p, 0, 16, st));        // the four class sizes
    H10X_HIP(c, hipMemsetAsync(counts.p + 9, 0, 4, st));
    H10X_HIP(c, hipMemsetAsync(zeroed.p + 16, 0, 16, st));
    H10X_HIP(c, hipMemsetAsync(counts.p + 12, 0, 8, st));
  }
  // (the work queue hands barcodes out in the order the classification appended them, i.e. mixed sizes: sorting the
  // queue by descending rank count was measured 17 % SLOWER — workgroups of like size run their phases in step and
  // contend for the same unit at the same time)
  ClusterArgs a{};
  a.blocks = c->blocks.p; a.blockOff = c->blockOff.p; a.clusHash = c->clusHash.p; a.goodPos = c->goodPos.p; a.nGood = c->nGood.p;
  a.goodRow = c->goodRow.p; a.rows = c->rows.p; a.nBlocks = c->nBlocks; a.threshold = threshold;
  a.segs = c->segs; a.nBlocksFirst = nGlobal; a.rowShift = (u32)c->rowShift;
  if (c->sharded && c->optRowsFakeBase) a.rows = c->rows.p - (size_t)c->optRowsFakeBase;   // test knob: rowStart[] carries the same offset (shard_exchangeRows)
  a.narrowFirst = (u32)c->optNarrowFirst; a.tpClassT = c->optTrClassT != 0 ? 1u : 0u;
  a.maxGood = c->maxGood; a.stats = stats.p; a.res = term.p; a.entries = c->goodEntries.p;
  a.firstCap = firstCap; a.hashMinSlots = hashMinSlots;
  a.hashBits = (u32)hashBits; a.hStride = hStride;
  const size_t trStride[3] = {trSlotFor(hc[12], (u32)threads0 / WAVE), trSlotFor(hmax<u32>(hc[12], hc[13]), CL_THREADS_HUGE / WAVE), trSlotFor(hmax<u32>(hc[12], hc[13]), CL_THREADS_HUGE / WAVE)};   // [1]: the whole-CU class's second launch
  // ranked / translated placement: blocks whose table was too small are re-run — those of the half-CU class (list A) with the
  // whole LDS of a CU, those that fail there as well (list B) with first[] dense on an HBM slot
  DevBuf<u32> ovfA, ovfB; H10X_HIP(c, ovfA.alloc(span)); H10X_HIP(c, ovfB.alloc(span));
  u32 *const ovfCountA = counts.p + 10, *const ovfCountB = counts.p + 11;
  DevBuf<u64> phase;
  if (c->optStamps) { H10X_HIP(c, phase.alloc(8)); H10X_HIP(c, hipMemsetAsync(phase.p, 0, 64, st)); a.phase = phase.p; }
  // HBM working set per workgroup (class 3): first[] + per-rank arrays for the largest barcode
  DevBuf<unsigned char> scratch;
  size_t stride = 0; u32 grid3 = 0;
  if (hc[3]) {
    stride = (workBytes(nGlobal, c->maxGood, CL_THREADS_SMALL / WAVE, 0) + 255) & ~(size_t)255;
    grid3 = hmin<u32>(hc[3], (u32)c->numCU);
    H10X_HIP(c, scratch.alloc(stride * grid3));
    H10X_HIP(c, hipMemsetAsync(scratch.p, 0xFF, stride * grid3, st));    // first[] = unseen everywhere
  }
  // hybrid placement: one first[] slot per resident workgroup of each LDS class
  DevBuf<unsigned char> firstSlots[3];
  const size_t firstStride = (((size_t)nGlobal * 2 + 255) & ~(size_t)255);
  u32 gridOf[3] = {hmin<u32>(hc[0] + hc[1], (u32)c->numCU * (u32)hmax<size_t>(1, (160 * 1024) / (budget0 + 1024))), hmin<u32>(hc[1], (u32)c->numCU * 2), hmin<u32>(hc[2], (u32)c->numCU)};   // class 1 unused
  // Both LDS classes are persistent launches that stay on the CUs they get: a whole-CU workgroup keeps two half-CU workgroups out. Where both have
  // enough blocks to fill the chip, the CUs are split by the classes' work (the whole-CU class does a list entry at ~0.8 x the rate per CU: measured
  // on the million-barcode set, where it used to finish 100 ms behind the main launch), so that the two launches end together.
  u32 secondWind = 0;
  if (firstMode == 4 && gridOf[2] && gridOf[0] >= (u32)c->numCU && hw[0] + hw[1]) {
    const double share2 = 1.25 * (double)hw[1] / (1.25 * (double)hw[1] + (double)hw[0]);
    // (+ 4 CUs: the blocks of that class are the ones with many ranks, which the work figure flatters; its CUs are not lost when it ends early —
    // while it is the smaller side, the main launch brings two workgroups for EVERY CU, and those that find no room wait in the dispatcher
    // for the whole-CU workgroups to leave: 3 Gb set, 2 169 such blocks: 657 ms on one CU behind a main launch of 510 ms before this)
    // Whichever side the split errs on corrects itself: the main launch always brings two workgroups for every CU (they take over the whole-CU class's
    // CUs when that ends first), and behind the main launch, on its stream, the whole-CU class is launched a SECOND time on the same work queue
    // (secondWind): workgroups for every CU, which find the queue empty — or the CUs the main launch has just left free. (Before this the main launch
    // was held to the CUs the split gave it once the whole-CU class had more than half of them: 890 ms instead of 570 on a set classified that way.)
    // (round 6: never fewer than an eighth of the CUs, 32 of 256, while the class has the blocks: where it is a side show — 2 169 blocks of the 3 Gb set, ~130 of a rank's
    // eighth of it — five CUs made it a 2 ms tail whenever the two launches do not run side by side, e.g. when their streams share a hardware queue (seen with eight ranks'
    // forty streams in one process: the rank's --cluster 19.5 instead of 17.4 ms); with 32 CUs it is done in 0.3 ms, and the main launch's workgroups take the CUs over)
    const u32 cu2 = hmin<u32>((u32)c->numCU > 16 ? (u32)c->numCU - 8 : (u32)c->numCU - 1, hmax<u32>(hmax<u32>(1u, (u32)c->numCU / 8u), (u32)(share2 * c->numCU + 0.5) + 4u));
    gridOf[2] = hmin<u32>(hc[2], cu2);
    gridOf[0] = hmin<u32>(gridOf[0], 2 * (u32)c->numCU);
    secondWind = hc[2] > gridOf[2] ? hmin<u32>(hc[2] - gridOf[2], (u32)c->numCU) : 0u;
  }
  DevBuf<u16> trSlots[3];                                  // translated placement: one handle slot per resident workgroup of each LDS class
  // (no room for a class's slots: fewer workgroups — down to one — before giving up; the launches are persistent, a smaller grid is only slower)
  auto trAlloc = [&](int k, u32 &grid) -> int {
    for (;;) {
      if (trSlots[k].alloc(trStride[k] * grid) == hipSuccess) return 0;
      (void)hipGetLastError();
      if (grid <= 1) return c->fail("no device memory for the handle slots of the cluster kernel (%.1f MB per workgroup)", trStride[k] * 2 / 1e6);
      grid = (grid + 1) / 2;
    }
  };
  if (firstMode == 4) for (int k = 0; k < 3; k += 2) if (gridOf[k]) H10X_TRY(trAlloc(k, gridOf[k]));
  if (secondWind) H10X_TRY(trAlloc(1, secondWind));
  if (firstMode == 2) for (int k = 0; k < 3; k += 2) if (gridOf[k]) {       // class 0 serves list 0 AND the front list (hc[1]); class 1 has no launch
    H10X_HIP(c, firstSlots[k].alloc(firstStride * gridOf[k]));
    H10X_HIP(c, hipMemsetAsync(firstSlots[k].p, 0xFF, firstStride * gridOf[k], st));
  }
  // The classes are independent: fork them onto side streams so that the few largest barcodes (long, low
  // parallelism) run beside the many small ones instead of in front of them. Every buffer they touch was
  // allocated before the fork and is released after the join, which is what the block cache requires.
  // a failure between here and the join must not let the buffers above go back to the block cache while a side stream
  // still runs a kernel on them (the cache orders reuse within ONE stream only)
  ForkGuard forkGuard(c);
  c->tstart(T_CLUSTER_K);
  H10X_TRY(c->forkStreams(3));
  if (hc[3]) {
    ClusterArgs g = a; g.list = list3.p; g.nList = hc[3]; g.workCounter = counts.p + 7; g.scratch = scratch.p; g.scratchStride = stride;
    H10X_TRY(stageC_launchCluster(c, 2, 0, CL_THREADS_SMALL, 0, grid3, c->aux[0], g));
  }
  // a launch of LDS class K (0 or 2) in the placement of this command, on the work queue counts[cnt] (`a` as it stands at the call)
  auto launchLds = [&](int K, int threads, size_t budget, hipStream_t stream, const u32 *list, u32 nList, u32 grid, int cnt, u32 *ovfCount, u32 *ovf) -> int {
    ClusterArgs g = a; g.list = list; g.nList = nList; g.workCounter = counts.p + cnt; g.ldsBudget = (u32)budget; g.overflow = ovf; g.overflowCount = ovfCount;
    if (firstMode == 4) { g.handles = trSlots[K].p; g.handleStride = trStride[K]; }
    else if (firstMode != 0 && firstMode != 1) { g.scratch = firstSlots[K].p; g.scratchStride = firstStride; }
    return stageC_launchCluster(c, firstMode == 4 ? (packed ? 5 : 4) : (firstMode == 0 || firstMode == 1 ? firstMode : 2), K, threads, budget, grid, stream, g);
  };
  if (hc[2]) {
    // The whole-CU class must be resident BEFORE the main launch: its workgroups need an empty CU, and once the main
    // launch's persistent workgroups sit on every CU they only get one when those retire — the two launches then run one
    // after the other instead of side by side (seen under rocprofv3: +0.15 ms). Its workgroups report in through pinned
    // host words; the host holds the main launch back until they have (some 10 us), with a time limit as a safeguard.
    if (!c->startFlags) H10X_HIP(c, hipHostMalloc((void **)&c->startFlags, 1024 * sizeof(u32), hipHostMallocDefault));
    memset(c->startFlags, 0, 1024 * sizeof(u32));
    // (only while that class is a side show: when it holds most of the barcodes its persistent workgroups would keep every
    // CU to themselves until their queue is empty, and the two launches share the chip better by racing for the CUs —
    // 1 M-barcode set: 2.20 s against 2.52 s)
    a.started = (gridOf[2] * 2 <= (u32)c->numCU || secondWind) && gridOf[2] <= 1024 ? c->startFlags : nullptr;
    H10X_TRY(launchLds(2, CL_THREADS_HUGE, budgetBig, c->aux[1], list2.p, hc[2], gridOf[2], 6, ovfCountB, ovfB.p));
    if (a.started) {
      const auto t0 = std::chrono::steady_clock::now();
      for (;;) {
        u32 up = 0;
        for (u32 i = 0; i < gridOf[2]; ++i) up += __atomic_load_n(&c->startFlags[i], __ATOMIC_RELAXED) ? 1u : 0u;
        if (up == gridOf[2] || std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(500)) break;
      }
    }
    a.started = nullptr;
  }
  // the main launch (class 0) counts its own work and has its own hipEvent bracket on its stream: that is the launch the
  // roofline figure of bench.py is quoted for, and what a rocprofv3 kernel trace reports as cluster_kernel<true, *, 1024, 0>
  if (hc[0] || hc[1]) {
    a.stats = stats.p + 4; a.front = list1.p; a.nFront = hc[1];
    c->tstart(T_CLUSTER_MAIN);
    H10X_TRY(launchLds(0, threads0, budget0, st, list0.p, hc[0], gridOf[0], 4, ovfCountA, ovfA.p));
    c->tstop(T_CLUSTER_MAIN);
    a.stats = stats.p; a.front = nullptr; a.nFront = 0;
  }
  if (secondWind) {                                          // (see the split above) same work queue, counters and overflow list as the first launch of the class; handle slots of its own
    ClusterArgs g = a; g.list = list2.p; g.nList = hc[2]; g.workCounter = counts.p + 6; g.ldsBudget = (u32)budgetBig;
    g.overflow = ovfB.p; g.overflowCount = ovfCountB; g.handles = trSlots[1].p; g.handleStride = trStride[1];
    H10X_TRY(stageC_launchCluster(c, packed ? 5 : 4, 2, CL_THREADS_HUGE, budgetBig, secondWind, st, g));
  }
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(c->faultAt(4));
  H10X_TRY(c->joinStreams(3));
  u32 nOverflow = 0;
  DevBuf<unsigned char> scratch2;
  if (firstMode == 1 || firstMode == 4) {
    u32 nA = 0, nB = 0;
    H10X_HIP(c, hipMemcpyAsync(&nA, ovfCountA, 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    if (nA) {                                                // half-CU tables that were too small: again with the whole LDS of a CU
      H10X_HIP(c, hipMemsetAsync(counts.p + 6, 0, 4, st));
      u32 gridA = hmin<u32>(nA, (u32)c->numCU);
      if (firstMode == 4 && trSlots[2].n < trStride[2] * gridA) H10X_TRY(trAlloc(2, gridA));
      H10X_TRY(launchLds(2, CL_THREADS_HUGE, budgetBig, st, ovfA.p, nA, gridA, 6, ovfCountB, ovfB.p));
      H10X_HIP(c, hipGetLastError());
    }
    H10X_HIP(c, hipMemcpyAsync(&nB, ovfCountB, 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    nOverflow = nA + nB;
    if (nB) {
      // last resort: first[] dense on a per-workgroup HBM slot and everything else in LDS (the hybrid form); a block that
      // got this far fits the whole-CU budget without its table
      const u32 grid = hmin<u32>(nB, (u32)c->numCU);
      H10X_HIP(c, scratch2.alloc(firstStride * grid));
      H10X_HIP(c, hipMemsetAsync(scratch2.p, 0xFF, firstStride * grid, st));
      H10X_HIP(c, hipMemsetAsync(counts.p + 7, 0, 4, st));
      ClusterArgs g = a; g.list = ovfB.p; g.nList = nB; g.workCounter = counts.p + 7; g.scratch = scratch2.p; g.scratchStride = firstStride;
      g.ldsBudget = (u32)budgetBig;
      H10X_TRY(stageC_launchCluster(c, 2, 3, CL_THREADS_HUGE, budgetBig, grid, st, g));
      H10X_HIP(c, hipGetLastError());
    }
  }
  // labels from the msBest column, then the ordered sums beside the read merges
  H10X_TRY(stageC_clusterTail(c, (u32)codeMin, (u32)codeMax, term.p, listBig.p, hc[9], hc[8]));
  c->haveClusterRaw = true;
  c->tstop(T_CLUSTER_K);
  u64 hs[8];
  H10X_TRY(c->readback(hs, stats.p, 64));
  H10X_TRY(c->syncReadbacks());
  c->tstop(T_CLUSTER);
  if (c->optStamps) { H10X_HIP(c, hipMemcpy(c->ctr.cluster_phase_ticks, phase.p, 64, hipMemcpyDeviceToHost)); }
  forkGuard.done();                                          // everything has been waited for
  if (!more) { memset(c->ctr.cluster_main, 0, sizeof c->ctr.cluster_main); memset(c->ctr.cluster_class_counts, 0, sizeof c->ctr.cluster_class_counts);
               c->ctr.sum_good = c->ctr.sum_good_depth = c->ctr.sum_hash_clustered = c->ctr.clustered_codes = c->ctr.cluster_overflow_blocks = 0; }
  for (int k = 0; k < 4; ++k) { c->ctr.cluster_main[k] += hs[4 + k]; hs[k] += hs[4 + k]; }   // re-runs of overflowed blocks count again (they did the work twice)
  c->ctr.sum_good += hs[0]; c->ctr.sum_good_depth += hs[1]; c->ctr.sum_hash_clustered += hs[2]; c->ctr.clustered_codes += span;
  c->ctr.cluster_first_mode = (uint64_t)firstMode; c->ctr.cluster_overflow_blocks += nOverflow;
  for (int k = 0; k < 4; ++k) c->ctr.cluster_class_counts[k] += hc[k];
  return 0;
}

// the --cluster loop over GLOBAL block numbers [codeMin, codeMax): every segment of this context runs its part
int stageC_cluster(Ctx *c, int codeMin, int codeMax, int threshold) {
  if (!c->haveGood) return c->fail("!! you must set hashDepthRange before cluster");          // hash10x.c:1258
  if (threshold < 1) return c->fail("clusterThreshold %d must be >= 1 (the reference reads an uninitialised msBest otherwise)", threshold);
  H10X_TRY(c->needGoodFigures());                                                               // maxGoodDepth, maxGood, meanGood: still on the device after an unsharded --hashDepthRange
  if (c->maxGoodDepth > RES_COUNT_MAX) return c->fail("a hash of the depth range lies in %u barcodes: beyond %u, the limit of this build", c->maxGoodDepth, RES_COUNT_MAX);
  const u32 nGlobal = c->sharded ? c->nBlocksGlobal : c->nBlocks;
  if (!codeMin) codeMin = 1;                                                                    // hash10x.c:1243-1244
  if (!codeMax) codeMax = (int)nGlobal;
  if (codeMin < 0 || codeMax > (int)nGlobal) return c->fail("cluster code range %d..%d outside 1..%u", codeMin, codeMax, nGlobal);
  bool any = false;
  for (int k = 0; k < c->segs.n; ++k) {
    const BlockSeg &sg = c->segs.s[k];
    const long first = (long)sg.localStart + (k == 0 ? 1 : 0);                                  // slot 0 of the first segment is nobody's block
    long lo = (long)codeMin - (long)sg.globalBase + (long)sg.localStart, hi = (long)codeMax - (long)sg.globalBase + (long)sg.localStart;
    if (lo < first) lo = first;
    if (hi > (long)sg.localStart + (long)sg.count) hi = (long)sg.localStart + (long)sg.count;
    if (hi <= lo) continue;
    H10X_TRY(cluster_local_range(c, (int)lo, (int)hi, threshold, any));
    any = true;
  }
  if (!any) { memset(c->ctr.cluster_class_counts, 0, sizeof c->ctr.cluster_class_counts); memset(c->ctr.cluster_main, 0, sizeof c->ctr.cluster_main);
              c->ctr.sum_good = c->ctr.sum_good_depth = c->ctr.sum_hash_clustered = c->ctr.clustered_codes = c->ctr.cluster_overflow_blocks = 0; }
  return 0;
}

__global__ void warm_stageCHost_kernel() {}
void warm_stageCHost(hipStream_t st) { warm_stageCHost_kernel<<<1, 1, 0, st>>>(); }

}  // namespace h10x
