// cluster.hpp — what the driver (stage_c_host.hip) and the kernels (stage_c.hip) of --cluster both need, and nothing else: the kernels'
// argument block (ClusterArgs), the sizes of a block's on-chip working set that the classification and the kernels must compute alike
// (workBytes, histWaves, translatedShape), the constants both name, and the two functions by which the driver reaches the launches.
// Stands for no code of the reference: codeClusterFind (hash10x.c:770-835) keeps all of this in calloc'ed arrays per barcode.
#pragma once
#include "common.hpp"

namespace h10x {

// ------------------------------------------------------------------------------------------ cluster kernel
struct ClusterArgs {
  h10x_block *blocks; const u64 *blockOff; h10x_clushash *clusHash;
  const u16 *goodPos; const u32 *nGood;
  const u64 *goodRow;                                       // per rank (slice of block c at blockOff[c]): low word = list offset in rows[] (>> rowShift), high word = list length = hashDepth
  const u32 *rows;
  const u32 *list; u32 nList; u32 *workCounter;
  u32 *started;                 // host-visible word per workgroup, set when the workgroup starts (whole-CU class only)
  const u32 *front; u32 nFront;                             // handed out before list[]: the largest barcodes of the launch
  u32 nBlocks; int threshold;
  SegMap segs;                                              // local block number -> global barcode number (what the lists hold); identity when unsharded
  u32 rowShift;                                             // rows[]: a list starts at entry (rs << rowShift) — sharded runs with more than 2^32 list entries
  u32 nBlocksFirst;                                         // size of first[]: barcodes of the whole data set + 1
  u32 firstCap;                                             // ranked placement, test knob: cap on the first[] entries of a block (0 = what the budget leaves)
  u32 hashMinSlots;                                         // translated placement: table slots below which the 10-bit tag is too narrow for the data set's barcode count
  u32 hashBits;                                             // b
  u16 *handles; size_t handleStride; u32 hStride;           // translated placement: HBM slot of the workgroup (handleStride u16 each), u16 per list (a power of two >= 64 that holds the longest list)
  const u32 *entries;                                       // per block: entries of its barcode lists (sum of depths of its good hashes)
  u32 *overflow, *overflowCount;                            // ranked / translated placement: blocks whose table was too small (re-run in the next larger placement)
  unsigned char *scratch; size_t scratchStride;             // global-mode working set per workgroup
  u32 maxGood;
  u32 ldsBudget;                                            // LDS bytes of the launch class (list loop: as many waves as have room for a histogram)
  u64 *res;                                                 // out, per rank (slice of block c at blockOff[c]): RES_PACK(msBest or NONE16 if msMax < threshold,
                                                            // minShareCount[clusterMin], msTot) — replay_kernel turns it into the rank's pointToMin term in place
  u64 *stats;                                               // [0] sum good, [1] sum good depth, [2] sum nHash, [3] codes
  u64 *phase;                                               // diagnostic per-phase ticks (null = off)
  u32 narrowFirst;                                          // test / A-B knob: keep first[] at 2 bytes per entry in every block
  u32 tpClassT;                                             // packed translated placement: class T (lists of 65 .. 96 entries, two to a unit of three chunks) in use
};

__host__ __device__ inline size_t pad16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ inline size_t workBytes(u32 nFirst, u32 n, u32 nWaves, u32 bmWords) {
  size_t b = pad16((size_t)nFirst * 2) + pad16((size_t)bmWords * 4) + pad16((size_t)bmWords * 2);
  b += pad16((size_t)n * 2);                                // root
  b += (size_t)nWaves * (((size_t)n + 3) / 4) * 4;          // hist (the list of unsettled ranks, 2 n bytes at most, overlays it after the loop: nWaves >= 5)
  return b + 16;
}
// waves of the workgroup that take part in the list loop of a barcode with n ranks: as many as have room for a private
// histogram in what the fixed part leaves of `budget` (0 = does not fit)
constexpr u32 MIN_HIST_WAVES = 5;
__host__ __device__ inline u32 histWaves(u32 nFirst, u32 n, u32 maxWaves, u32 bmWords, size_t budget) {
  const size_t fixed = workBytes(nFirst, n, 0, bmWords), per = (((size_t)n + 3) / 4) * 4;
  if (fixed + MIN_HIST_WAVES * per > budget) return 0;
  const size_t wv = (budget - fixed) / (per ? per : 1);
  return wv < maxWaves ? (u32)wv : maxWaves;
}

constexpr u32 TR_QUEUE = 16384;                              // entries of a wave's queue in pass A (8 bytes each, behind the handles on the workgroup's HBM slot)
constexpr u32 TR_MIN_SLOTS = 1024;                             // tables are not made smaller than this
constexpr u32 TR_MAX_SLOTS = 65532;                          // handles are 16 bits; slot S (<= 65532) is the handle of "no entry" and reads unseen
// slots of a block's table and what pass B then looks like: S = 0 if the block does not fit `budget`. The table gets every byte
// pass A can give it (the emptier, the shorter the probes) but no more than twice the entries of the block's lists — a table at
// most half full cannot overflow — and no more than pass B can keep at 2 bytes per slot beside root[] and five histograms.
// S2: slots of a SECOND table, should the first fill up (only then: it is "closed" at 7/8 and the barcodes that turn up afterwards
// are parked): it lives in the half of the first table's LDS that the compaction of its ranks frees, as far as pass B then still
// has room for 2 bytes per slot of both. 0 = none (the first table holds every barcode the lists can bring, or nothing is left).
__host__ __device__ inline void translatedShape(u32 n, u32 maxWaves, size_t budget, u32 minSlots, u32 entries, u32 nBarcodes, u32 cap /* test knob */,
                                                u32 &S, u32 &S2, u32 &nW, bool &compact) {
  const size_t per = (((size_t)n + 3) / 4) * 4, fixedB = pad16((size_t)n * 2) + 64;
  S = 0; S2 = 0; nW = 0; compact = false;
  if (fixedB + MIN_HIST_WAVES * per + 2 * 256 + 64 >= budget) return;
  const size_t sA = (budget - 64) / 4, sB = (budget - fixedB - MIN_HIST_WAVES * per) / 2 - 16;
  size_t s = sA < sB ? sA : sB;
  if (s > TR_MAX_SLOTS) s = TR_MAX_SLOTS;
  size_t useful = 2 * (size_t)(entries < nBarcodes ? entries : nBarcodes) + 64;
  if (useful < TR_MIN_SLOTS) useful = TR_MIN_SLOTS;
  if (useful < minSlots) useful = minSlots;                  // (the tag's width asks for this many: a block with few entries still gets them)
  const bool all = s >= useful;                              // holds whatever the lists bring
  if (all) s = useful;
  if (cap && s > cap) s = cap;
  s &= ~(size_t)3;
  if (s < 64 || s < minSlots) return;                        // (16 buckets at least: the probe stride is below that)
  S = (u32)s;
  if (!all || cap) {
    const long a2 = ((long)budget - (long)pad16(2 * (s + 8)) - 64) / 4, b2 = ((long)budget - (long)fixedB - (long)(MIN_HIST_WAVES * per) - 2 * (long)(s + 8) - 64) / 2;
    long s2 = a2 < b2 ? a2 : b2;
    if (s2 > (long)TR_MAX_SLOTS - (long)s - 4) s2 = (long)TR_MAX_SLOTS - (long)s - 4;
    if (cap && s2 > (long)cap) s2 = (long)cap;
    s2 &= ~3L;
    if (s2 >= 64 && s2 >= (long)minSlots) S2 = (u32)s2;
  }
  if (pad16(4 * (s + 4)) + fixedB + (size_t)maxWaves * per <= budget) { nW = maxWaves; return; }   // the table stays as it is: every wave has its histogram anyway
  compact = true;
  const size_t wv = (budget - fixedB - pad16(2 * (s + 8))) / (per ? per : 1);
  nW = wv < maxWaves ? (u32)wv : maxWaves;
}
constexpr u32 REPLAY_SMALL = 2040, REPLAY_MID = 16376;       // rank counts up to which a block's replay runs in 16 KB / 128 KB of LDS

// ---- a kernel is launched from the unit that defines it: what stage_c_host.hip calls in stage_c.hip
// one cluster_kernel launch. placement = FIRST_MODE (0 dense in LDS, 1 ranked, 2 first[] on an HBM slot, 4 translated, 5 translated packed),
// klass = the kernel's launch class (0 half a CU, 2 a whole CU, 3 the last resort behind both), ldsBytes = its dynamic LDS (0: the working set on g.scratch)
int stageC_launchCluster(Ctx *c, int placement, int klass, int lanes, size_t ldsBytes, u32 grid, hipStream_t st, const ClusterArgs &g);
// replay, ordered sums and read merges of blocks [codeMin, codeMax) from the result words in res[]; listBig: the nBig blocks with more than REPLAY_SMALL ranks
int stageC_clusterTail(Ctx *c, u32 codeMin, u32 codeMax, u64 *res, const u32 *listBig, u32 nBig, u32 maxReads);
}  // namespace h10x
