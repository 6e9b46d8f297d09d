// mosh.hpp — the mosh set object shared by stage_g.hip (moshutils) and stage_h.hip (moshasm's readsets over a set)
#pragma once
#include "common.hpp"
#include "seq_scan.hpp"

namespace h10x {

constexpr u64 MOSH_SLAB_DEFAULT = (u64)1 << 26;              // bases per batch
constexpr u64 RS_CHUNK_ENTRIES_DEFAULT = (u64)1 << 26;       // expanded (x, y) entries per chunk of queries of a readset's overlap table (stage_h.hip)
constexpr u32 RS_CHUNK_READS_MAX = 65536;                    // queries per chunk: a read's place in its chunk travels in 16 bits

struct Mosh {
  Ctx c;                                                     // stream, error text, block cache scope; c.hashIndex = index[], c.hashValue = value[]
  int B = 0, k = 0, w = 0; u64 factor1 = 0, factor2 = 0;
  u32 size = 0, max = 0;                                     // ms->size (capacity of the per-index arrays: max stays below it), ms->max
  DevBuf<u16> depth; DevBuf<u8> info; DevBuf<u32> acc;
  u64 slab = MOSH_SLAB_DEFAULT;
  u64 overlapChunk = RS_CHUNK_ENTRIES_DEFAULT; u32 overlapChunkReads = RS_CHUNK_READS_MAX;   // options "overlap_chunk", "overlap_chunk_reads": read when a readset's table is built
};

static inline int moshEnter(Mosh *m) {
  Ctx &c = m->c;
  if (hipSetDevice(c.device) != hipSuccess) return c.fail("hipSetDevice(%d) failed", c.device);
  AllocScope::stream() = c.stream; AllocScope::device() = c.device;
  DevCache::noteStream(c.device, c.stream);
  c.pendingReads.clear(); c.mailUsed = 0; c.mailDirect = false;
  return 0;
}

// batches = as many whole sequences as fit the slab; a longer sequence goes alone
template <typename F> static int moshBatches(Mosh *m, const u64 *seqStart, u32 nSeq, F &&f) {
  u32 s = 0;
  while (s < nSeq) {
    u32 e = s + 1;
    while (e < nSeq && seqStart[e + 1] - seqStart[s] <= m->slab) ++e;
    H10X_TRY(f(s, e - s));
    s = e;
  }
  return 0;
}

// what a driver outside stage_g.hip builds a set with (stage_o.hip): an empty object on a stream of its own, its arrays (zeroed, `size` entries per
// index), and the table entries of the new indices [max + 1, max + 1 + D) whose value[] is written
int moshOpen(Mosh **out, int B, int k, int w, u64 factor1, u64 factor2, int device, char *err, int errlen);
int moshAllocSet(Mosh *m, u32 size);
int moshPlace(Mosh *m, u32 D);
int moshFold(Mosh *m);                                       // depth = min(65535, depth + acc), acc = 0: the end of a batch of -a / -x and of a readset's -f

// one uploaded batch and the list its scan left (stage_g.hip)
struct MoshBatch : SeqBatch { DevBuf<u64> tallies, outHash; DevBuf<u32> outOrd; u64 nRuns = 0, total = 0, listed = 0, found = 0; };
// the scan of one batch with a hasher given as arguments, on the stream of any context: acc = null lists every mosh in b.outHash / b.outOrd (in no
// order; b.listed of them), else the moshes found in c's table count in acc[accSize] and only the others are listed (stage_g.hip; stage_p.hip)
int moshScanWith(Ctx *c, int k, int w, u64 factor1, int B, u32 *acc, u32 accSize, MoshBatch &b, const u8 *codes, const u64 *seqStart, u32 nSeq, int skipOdd,
                 u64 seqBase);
int moshIota(Mosh *m, u32 *v, u64 n);
int moshScanOrdered(Mosh *m, MoshBatch &b, DevBuf<u64> &sh, DevBuf<u32> &so, const u8 *codes, const u64 *seqStart, u32 nSeq, int skipOdd, u64 seqBase);

}  // namespace h10x
