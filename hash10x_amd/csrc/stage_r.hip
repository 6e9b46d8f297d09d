// stage_r.hip — sequence spans, behind --seqSpans: where on a sequence each block's hits lie (extents) and how many kept extents span each window boundary
// (include/h10x.h "sequence spans"). Per slab of whole sequences:
//   scan     stage_g's mosh_scan_kernel<0> with the CONTEXT's hasher: every mosh occurrence as (hash, ordinal of its k-mer in the slab);
//   look-up  one lane per occurrence: the probe of sp_lookup_kernel, the key ordinal << 2 | class (0 absent, 1 found out of range, 2 counting) with the index
//            as value; a sort by ordinal puts the occurrences in (sequence, position) order;
//   figures  two flag scans (found, counting); one lane per sequence: two searches in the sorted keys give moshes, the scans' values there found, inRange
//            and the sequence's first unit. No atomic: every figure is a difference of positions;
//   units    one unit per counting occurrence (index, ordinal), compacted by the scan; per batch one lane per unit counts the entries of its barcode list in
//            the block window, and their exclusive sum is every unit's place;
//   gather   one wave per unit: key = block << ob | ordinal, ob = keyBits(bases of the slab). 64-bit keys: the ordinal is a u32 and so is the block;
//   sort     prim_sort_keys_u64 on the bits in use: a block's hits ascend by ordinal, that is by (sequence, position);
//   extents  key i is a head when it is the first, its block or its sequence differs from key i - 1's, or the ordinals lie more than maxGap apart (maxGap > 0);
//            a scan numbers the extents; the head writes first and its index, the key before the next head last and its index, hits = the difference + 1;
//            a second flag, scan and compact keeps those of at least minShare hits. An extent may cross any wave or workgroup edge: nothing here is per wave;
//   regroup  the kept extents come out by (block, sequence, first); a stable sort on the sequence makes it (sequence; block, first), the row order; the rows
//            per sequence are two searches;
//   cover    one lane per kept extent: +1 at boundary first / W + 1, -1 behind boundary last / W in a difference array with one spare slot per sequence
//            (scattered addresses, integer adds: any order gives the same words); an inclusive scan; the spare slots dropped.
// Batches inside a slab are cut by hits against "neighbour_budget" over whole sequences; a sequence above it runs alone in windows of block index. The block
// is the key's high field, so a window holds whole extents, and windows in ascending block order append in row order.
#include "census_rows.hpp"
#include "mosh.hpp"
#include "wave.hpp"

namespace h10x {

__global__ __launch_bounds__(256) void sr_lookup_kernel(const u64 *__restrict__ hash, const u32 *__restrict__ ord, u64 n, const u32 *__restrict__ table,
                                                        const u64 *__restrict__ hashValue, int B, const u8 *__restrict__ within, u32 U1, u64 *__restrict__ key,
                                                        u32 *__restrict__ xs) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u32 x = probe_find(table, hashValue, B, hash[i]);
    if (x >= U1) x = 0;                                       // (a table entry beyond hashNumber is no index of this state)
    key[i] = (u64)ord[i] << 2 | (!x ? 0u : within[x] ? 2u : 1u);
    xs[i] = x;
  }
}

// fFound[i] / fCount[i] = occurrence i is found / counts; entry n of both = 0 (the scans' last entries are the totals)
__global__ void sr_class_kernel(const u64 *__restrict__ key, u64 n, u32 *__restrict__ fFound, u32 *__restrict__ fCount) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  const u32 cls = i < n ? (u32)(key[i] & 3) : 0;
  fFound[i] = cls >= 1; fCount[i] = cls == 2;
}

// one lane per sequence s <= ns: a = the first sorted occurrence at or behind its start; uOff[s] = the counting occurrences before a = its first unit;
// s < ns: fig[3 s ..] = {moshes, found, inRange}
__global__ void sr_figures_kernel(const u64 *__restrict__ key, u64 n, const u64 *__restrict__ seqRel, u32 ns, const u32 *__restrict__ pFound,
                                  const u32 *__restrict__ pCount, u32 *__restrict__ fig, u64 *__restrict__ uOff) {
  const u32 s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s > ns) return;
  const u64 a = lower_bound(key, (u64)0, n, seqRel[s] << 2);
  uOff[s] = pCount[a];
  if (s == ns) return;
  const u64 e = lower_bound(key, a, n, seqRel[s + 1] << 2);
  fig[3 * (size_t)s] = (u32)(e - a); fig[3 * (size_t)s + 1] = pFound[e] - pFound[a]; fig[3 * (size_t)s + 2] = pCount[e] - pCount[a];
}

__global__ void sr_units_kernel(const u64 *__restrict__ key, const u32 *__restrict__ xs, const u32 *__restrict__ fCount, const u32 *__restrict__ pCount, u64 n,
                                u32 cap, u32 *__restrict__ uX, u32 *__restrict__ uOrd) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !fCount[i]) return;
  const u32 p = pCount[i];
  if (p < cap) { uX[p] = xs[i]; uOrd[p] = (u32)(key[i] >> 2); }
}

// one wave per sequence q0 + q: size[q] = the entries of its units' barcode lists in the window = its hits there
__global__ void sr_size_kernel(u32 nq, const u64 *__restrict__ uOff /* at q0 */, const u32 *__restrict__ uX, const u64 *__restrict__ rowStart,
                               const u32 *__restrict__ hashDepth, const u32 *__restrict__ rows, u32 lo, u32 hi, int full, u64 *__restrict__ size) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u32 q = (u32)(((u64)blockIdx.x * blockDim.x + threadIdx.x) / WAVE);
  if (q >= nq) return;                                        // whole waves leave: the fold below sees all 64 lanes
  u64 s = 0;
  for (u64 j = uOff[q] + lane; j < uOff[q + 1]; j += WAVE) { u64 a, b; sp_window(rows, rowStart, hashDepth, uX[j], lo, hi, full != 0, a, b); s += b - a; }
  s = wave_sum(s);
  if (lane == 0) size[q] = s;
}

// one lane per unit u0 + u: cnt[u] = entries of its list in the window; cnt[units] = 0
__global__ void sr_unit_count_kernel(u64 u0, u64 units, const u32 *__restrict__ uX, const u64 *__restrict__ rowStart, const u32 *__restrict__ hashDepth,
                                     const u32 *__restrict__ rows, u32 lo, u32 hi, int full, u32 *__restrict__ cnt) {
  const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (u > units) return;
  u32 n = 0;
  if (u < units) { u64 a, b; sp_window(rows, rowStart, hashDepth, uX[u0 + u], lo, hi, full != 0, a, b); n = (u32)(b - a); }
  cnt[u] = n;
}

// one wave per unit; its keys go to [place[u], place[u + 1]) in list order. cap = place[units]: a miscount stays in bounds
__global__ __launch_bounds__(256) void sr_gather_kernel(u64 u0, u64 units, const u32 *__restrict__ uX, const u32 *__restrict__ uOrd, const u64 *__restrict__ rowStart,
                                                        const u32 *__restrict__ hashDepth, const u32 *__restrict__ rows, u32 lo, u32 hi, int full, int ob,
                                                        const u64 *__restrict__ place, u64 cap, u64 *__restrict__ keys) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u64 w0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / WAVE, wStride = ((u64)gridDim.x * blockDim.x) / WAVE;
  for (u64 u = w0; u < units; u += wStride) {
    u64 a, b; sp_window(rows, rowStart, hashDepth, uX[u0 + u], lo, hi, full != 0, a, b);
    const u64 low = uOrd[u0 + u], p0 = place[u];
    for (u64 j = a + lane; j < b; j += WAVE) {
      const u64 p = p0 + (j - a);
      if (p < cap) keys[p] = (u64)rows[j] << ob | low;
    }
  }
}

// flag[i] = key i starts an extent; flag[n] = 0
__global__ void sr_heads_kernel(const u64 *__restrict__ key, u64 n, int ob, const u64 *__restrict__ seqRel, u32 ns, u32 G, u32 *__restrict__ flag) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  u32 f = 0;
  if (i < n) {
    f = 1;
    if (i) {
      const u64 k = key[i], p = key[i - 1], mask = ((u64)1 << ob) - 1, o = k & mask, po = p & mask;   // same block: po <= o
      if ((k >> ob) == (p >> ob) && !(G && o - po > G)) f = o >= seqRel[last_le(seqRel, ns, po) + 1];
    }
  }
  flag[i] = f;
}

// extent e = pos[i] + flag[i] - 1 of key i. Its head writes sequence, block, first and its own index; its last key (the next is a head, or there is none) last and its index
__global__ void sr_ends_kernel(const u64 *__restrict__ key, const u32 *__restrict__ flag, const u32 *__restrict__ pos, u64 n, int ob, const u64 *__restrict__ seqRel,
                               u32 ns, u32 nExt, u32 *__restrict__ eSeq, u32 *__restrict__ eBlock, u32 *__restrict__ eFirst, u32 *__restrict__ eLast,
                               u32 *__restrict__ eStart, u32 *__restrict__ eEnd) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 head = flag[i], tail = flag[i + 1] || i + 1 == n;
  if (!head && !tail) return;
  const u32 e = pos[i] + head - 1;
  if (e >= nExt) return;
  const u64 k = key[i], o = k & (((u64)1 << ob) - 1);
  const u32 s = last_le(seqRel, ns, o), p = (u32)(o - seqRel[s]);
  if (head) { eSeq[e] = s; eBlock[e] = (u32)(k >> ob); eFirst[e] = p; eStart[e] = (u32)i; }
  if (tail) { eLast[e] = p; eEnd[e] = (u32)i; }
}

// keep[e] = extent e has at least T hits; keep[nExt] = 0
__global__ void sr_keep_kernel(const u32 *__restrict__ eStart, const u32 *__restrict__ eEnd, u32 nExt, u32 T, u32 *__restrict__ keep) {
  const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e > nExt) return;
  keep[e] = e < nExt && eEnd[e] - eStart[e] + 1 >= T;
}

// the kept extents back to back: their sequence in the batch and their number
__global__ void sr_compact_kernel(const u32 *__restrict__ keep, const u32 *__restrict__ kpos, const u32 *__restrict__ eSeq, u32 nExt, u32 q0, u32 nKept,
                                  u32 *__restrict__ cSeq, u32 *__restrict__ cIdx) {
  const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nExt || !keep[e]) return;
  const u32 j = kpos[e];
  if (j < nKept) { cSeq[j] = eSeq[e] - q0; cIdx[j] = e; }
}

// row j of the batch = extent idx[j] (the caller passes the columns at the batch's first row)
__global__ void sr_rows_kernel(const u32 *__restrict__ idx, u32 nKept, const u32 *__restrict__ eBlock, const u32 *__restrict__ eFirst, const u32 *__restrict__ eLast,
                               const u32 *__restrict__ eStart, const u32 *__restrict__ eEnd, u32 *__restrict__ oBlock, u32 *__restrict__ oFirst,
                               u32 *__restrict__ oLast, u32 *__restrict__ oHits) {
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nKept) return;
  const u32 e = idx[j];
  oBlock[j] = eBlock[e]; oFirst[j] = eFirst[e]; oLast[j] = eLast[e]; oHits[j] = eEnd[e] - eStart[e] + 1;
}

// rowCnt[q] += rows of the batch in sequence q of it (seq ascends). A windowed sequence comes here once per window, one launch after the other
__global__ void sr_row_count_kernel(const u32 *__restrict__ seq, u32 nKept, u32 nq, u32 *__restrict__ rowCnt) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const u32 s = lower_bound(seq, 0u, nKept, q);
  rowCnt[q] += upper_bound(seq, s, nKept, q) - s;
}

// one lane per kept extent j of the slab, in sequence s = the row that holds it: +1 at its first spanned boundary, -1 behind its last, in the
// sequence's stretch of diff[] at cOff[s] + s (one spare slot each). last <= L - 1, so last / W is at most the spare slot
__global__ void sr_cover_kernel(const u32 *__restrict__ first, const u32 *__restrict__ last, u64 nRows, const u64 *__restrict__ rowOff, const u64 *__restrict__ cOff,
                                u32 ns, u32 W, u32 *__restrict__ diff) {
  const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nRows) return;
  const u32 j0 = first[j] / W + 1, j1 = last[j] / W;
  if (j0 > j1) return;
  const u32 s = last_le(rowOff, ns, j);
  u32 *d = diff + cOff[s] + s;
  atomicAdd(d + (j0 - 1), 1u); atomicAdd(d + j1, 0xFFFFFFFFu);
}

// cover[t] = the scanned difference array without the spare slots
__global__ void sr_cover_out_kernel(const u32 *__restrict__ scanned, u64 nB, const u64 *__restrict__ cOff, u32 ns, u32 *__restrict__ cover) {
  const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < nB) cover[t] = scanned[t + last_le(cOff, ns, t)];
}

__global__ void sr_span_kernel(const u32 *__restrict__ first, const u32 *__restrict__ last, u64 n, u32 *__restrict__ span) {
  const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) span[j] = last[j] - first[j];
}

namespace {

struct SeqSpans {
  Ctx *c; u32 T, G, W; u64 budget;
  h10x_seq_spans_info *info;
  PrimTemp pt;
  // the slab: its sequences' starts and units on the device, the rows per sequence
  const u64 *seqRel = nullptr; u32 ns = 0; int ob = 1;
  DevBuf<u64> uOff, dSize, place, keys, keysS, rowOff, cOff; DevBuf<u32> uX, uOrd, unitCnt, flag, pos, rowCnt;
  DevBuf<u32> eSeq, eBlock, eFirst, eLast, eStart, eEnd, keep, kpos, cSeq, cIdx, sSeq, sIdx;
  std::vector<u64> hUOff;
  u64 rows = 0, covered = 0;                                  // extents and boundaries kept so far

  int sizes(u32 q0, u32 n, u32 lo, u32 hi, bool full, u64 *hSize) {
    hipStream_t st = c->stream;
    H10X_HIP(c, dSize.alloc(n));
    sr_size_kernel<<<divUp((u64)n * WAVE, 256), 256, 0, st>>>(n, uOff.p + q0, uX.p, c->rowStart.p, c->hashDepth.p, c->rows.p, lo, hi, full ? 1 : 0, dSize.p);
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipMemcpyAsync(hSize, dSize.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    return 0;
  }

  // sequences [q0, q0 + n) of the slab in the block window [lo, hi); total = their hits there
  int batch(u32 q0, u32 n, u32 lo, u32 hi, bool full, u64 total) {
    hipStream_t st = c->stream;
    if (!full) { c->nbStats[3] += 1; ++info->windows; }
    c->nbStats[2] += 1; ++info->batches;
    if (!total) return 0;
    if (total >= 0xFFFFFFFFull) return c->fail("seqSpans: %llu hits in one batch, beyond 2^32 (sequence %u of its slab alone)", total, q0);
    const u64 u0 = hUOff[q0], units = hUOff[q0 + n] - u0;
    if (unitCnt.n < units + 1) { H10X_HIP(c, unitCnt.alloc(units + 1)); H10X_HIP(c, place.alloc(units + 1)); }
    sr_unit_count_kernel<<<divUp(units + 1, 256), 256, 0, st>>>(u0, units, uX.p, c->rowStart.p, c->hashDepth.p, c->rows.p, lo, hi, full ? 1 : 0, unitCnt.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, unitCnt.p, place.p, units + 1));
    unsigned long long nKeys = 0;
    H10X_TRY(c->readback(&nKeys, place.p + units, 8)); H10X_TRY(c->syncReadbacks());
    if (nKeys != total) return c->fail("seqSpans: %llu keys of %llu hits", nKeys, total);
    c->nbStats[0] += total; c->nbStats[1] += nKeys; info->hits += nKeys;
    // the two fields of a key: the ordinal is a u32 (ob <= 32) and so is the block, so they always fit 64 bits; a slab that broke this is refused all the same
    const int endBit = ob + keyBits(hi - 1);
    if (endBit > 64) return c->fail("seqSpans: %d bits of ordinal and %u blocks do not fit a 64-bit key", ob, hi);
    if (keys.n < nKeys) { H10X_HIP(c, keys.alloc(nKeys)); H10X_HIP(c, keysS.alloc(nKeys)); }
    if (flag.n < nKeys + 1) { H10X_HIP(c, flag.alloc(nKeys + 1)); H10X_HIP(c, pos.alloc(nKeys + 1)); }
    sr_gather_kernel<<<(unsigned)hmin<u64>(divUp(units, 4), 65536), 256, 0, st>>>(u0, units, uX.p, uOrd.p, c->rowStart.p, c->hashDepth.p, c->rows.p, lo, hi,
                                                                                  full ? 1 : 0, ob, place.p, nKeys, keys.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_sort_keys_u64(c, pt, keys.p, keysS.p, nKeys, 0, endBit));
    sr_heads_kernel<<<divUp(nKeys + 1, 256), 256, 0, st>>>(keysS.p, nKeys, ob, seqRel, ns, G, flag.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, pos.p, nKeys + 1));
    u32 nExt = 0;
    H10X_TRY(c->readback(&nExt, pos.p + nKeys, 4)); H10X_TRY(c->syncReadbacks());
    info->extentsAll += nExt;
    if (eSeq.n < nExt) for (DevBuf<u32> *b : {&eSeq, &eBlock, &eFirst, &eLast, &eStart, &eEnd}) H10X_HIP(c, b->alloc(nExt));
    if (keep.n < (size_t)nExt + 1) { H10X_HIP(c, keep.alloc((size_t)nExt + 1)); H10X_HIP(c, kpos.alloc((size_t)nExt + 1)); }
    sr_ends_kernel<<<divUp(nKeys, 256), 256, 0, st>>>(keysS.p, flag.p, pos.p, nKeys, ob, seqRel, ns, nExt, eSeq.p, eBlock.p, eFirst.p, eLast.p, eStart.p, eEnd.p);
    H10X_HIP(c, hipGetLastError());
    sr_keep_kernel<<<divUp((u64)nExt + 1, 256), 256, 0, st>>>(eStart.p, eEnd.p, nExt, T, keep.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_exclusive_scan_u32(c, pt, keep.p, kpos.p, (size_t)nExt + 1));
    u32 nKept = 0;
    H10X_TRY(c->readback(&nKept, kpos.p + nExt, 4)); H10X_TRY(c->syncReadbacks());
    if (!nKept) return 0;
    if (cSeq.n < nKept) for (DevBuf<u32> *b : {&cSeq, &cIdx, &sSeq, &sIdx}) H10X_HIP(c, b->alloc(nKept));
    sr_compact_kernel<<<divUp(nExt, 256), 256, 0, st>>>(keep.p, kpos.p, eSeq.p, nExt, q0, nKept, cSeq.p, cIdx.p);
    H10X_HIP(c, hipGetLastError());
    const u32 *seq = cSeq.p, *idx = cIdx.p;                   // one sequence: (block, first) is the row order already
    if (n > 1) { H10X_TRY(prim_sort_pairs_u32_u32(c, pt, cSeq.p, sSeq.p, cIdx.p, sIdx.p, nKept, 0, keyBits(n - 1))); seq = sSeq.p; idx = sIdx.p; }
    for (DevBuf<u32> *b : {&c->ssBlock, &c->ssFirst, &c->ssLast, &c->ssHits}) H10X_TRY(reserve_keep(c, *b, rows, rows + nKept));
    sr_rows_kernel<<<divUp(nKept, 256), 256, 0, st>>>(idx, nKept, eBlock.p, eFirst.p, eLast.p, eStart.p, eEnd.p, c->ssBlock.p + rows, c->ssFirst.p + rows,
                                                      c->ssLast.p + rows, c->ssHits.p + rows);
    H10X_HIP(c, hipGetLastError());
    sr_row_count_kernel<<<divUp(n, 256), 256, 0, st>>>(seq, nKept, n, rowCnt.p + q0);
    H10X_HIP(c, hipGetLastError());
    rows += nKept;
    return 0;
  }

  // the coverage of the slab's rows [row0, rows), whose offsets per sequence are in rowOff
  int cover(u64 row0, const u64 *slabStart, u64 *coverOff /* the command's, at the slab's first sequence: [0] is set */) {
    hipStream_t st = c->stream;
    std::vector<u64> h((size_t)ns + 1, 0);
    for (u32 s = 0; s < ns; ++s) { const u64 L = slabStart[s + 1] - slabStart[s]; h[s + 1] = h[s] + (W && L ? (L - 1) / W : 0); coverOff[s + 1] = coverOff[0] + h[s + 1]; }
    const u64 nB = h[ns], slabRows = rows - row0;
    if (!nB) return 0;
    StreamWait wait{st};                                      // (the upload reads h)
    DevBuf<u32> diff, scanned;
    H10X_HIP(c, cOff.alloc((size_t)ns + 1)); H10X_HIP(c, diff.alloc(nB + ns)); H10X_HIP(c, scanned.alloc(nB + ns));
    H10X_HIP(c, hipMemcpyAsync(cOff.p, h.data(), ((size_t)ns + 1) * 8, hipMemcpyHostToDevice, st));
    H10X_HIP(c, hipMemsetAsync(diff.p, 0, (nB + ns) * 4, st));
    if (slabRows) {
      sr_cover_kernel<<<divUp(slabRows, 256), 256, 0, st>>>(c->ssFirst.p + row0, c->ssLast.p + row0, slabRows, rowOff.p, cOff.p, ns, W, diff.p);
      H10X_HIP(c, hipGetLastError());
    }
    H10X_TRY(prim_inclusive_scan_u32(c, pt, diff.p, scanned.p, nB + ns));
    H10X_TRY(reserve_keep(c, c->ssCover, covered, covered + nB));
    sr_cover_out_kernel<<<divUp(nB, 256), 256, 0, st>>>(scanned.p, nB, cOff.p, ns, c->ssCover.p + covered);
    H10X_HIP(c, hipGetLastError());
    covered += nB;
    return 0;
  }

  // one slab: sequences [0, ns_) from slabStart; fig (may be null) and the command's offsets at the slab's first sequence
  int slab(const u8 *codes, const u64 *slabStart, u32 ns_, h10x_seq_span_figures *fig, u64 *offsets, u64 *coverOff) {
    hipStream_t st = c->stream;
    ns = ns_;
    const u32 U1 = c->hashNumber;
    MoshBatch b;
    H10X_TRY(moshScanWith(c, c->prm.k, c->prm.w, c->prm.factor1, c->prm.B, nullptr, 0, b, codes, slabStart, ns, 0, 0));
    const u64 n = b.listed, bases = slabStart[ns] - slabStart[0], row0 = rows;
    if (n > 0xFFFFFFFEull) return c->fail("seqSpans: %llu moshes in one batch", n);
    seqRel = b.seq.p; ob = keyBits(bases);
    std::vector<u32> hFig((size_t)3 * ns, 0);
    std::vector<u64> hRowOff((size_t)ns + 1, 0);
    hUOff.assign((size_t)ns + 1, 0);
    StreamWait wait{st};                                      // (the copies below write these vectors)
    H10X_HIP(c, rowCnt.alloc((size_t)ns + 1)); H10X_HIP(c, hipMemsetAsync(rowCnt.p, 0, ((size_t)ns + 1) * 4, st));   // (the last stays 0)
    H10X_HIP(c, rowOff.alloc((size_t)ns + 1));
    u32 units = 0;
    if (n) {
      if (ob > 32) return c->fail("seqSpans: a slab of %llu bases: the ordinal of a k-mer does not fit 32 bits", bases);
      DevBuf<u64> key, keyS; DevBuf<u32> xs, xsS, fFound, fCount, pFound, pCount, dFig;
      H10X_HIP(c, key.alloc(n)); H10X_HIP(c, keyS.alloc(n)); H10X_HIP(c, xs.alloc(n)); H10X_HIP(c, xsS.alloc(n)); H10X_HIP(c, dFig.alloc((size_t)3 * ns));
      for (DevBuf<u32> *f : {&fFound, &fCount, &pFound, &pCount}) H10X_HIP(c, f->alloc(n + 1));
      H10X_HIP(c, uOff.alloc((size_t)ns + 1));
      sr_lookup_kernel<<<(unsigned)hmin<u64>(divUp(n, 256), 16384), 256, 0, st>>>(b.outHash.p, b.outOrd.p, n, c->hashIndex.p, c->hashValue.p, c->prm.B, c->within.p, U1,
                                                                                   key.p, xs.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_sort_pairs_u64_u32(c, pt, key.p, keyS.p, xs.p, xsS.p, n, 2, 2 + ob));   // by ordinal: at most one mosh per k-mer start
      sr_class_kernel<<<divUp(n + 1, 256), 256, 0, st>>>(keyS.p, n, fFound.p, fCount.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_exclusive_scan_u32(c, pt, fFound.p, pFound.p, n + 1)); H10X_TRY(prim_exclusive_scan_u32(c, pt, fCount.p, pCount.p, n + 1));
      H10X_TRY(c->readback(&units, pCount.p + n, 4)); H10X_TRY(c->syncReadbacks());
      sr_figures_kernel<<<divUp((u64)ns + 1, 256), 256, 0, st>>>(keyS.p, n, seqRel, ns, pFound.p, pCount.p, dFig.p, uOff.p);
      H10X_HIP(c, hipGetLastError());
      H10X_HIP(c, uX.alloc(hmax<u32>(units, 1))); H10X_HIP(c, uOrd.alloc(hmax<u32>(units, 1)));
      if (units) {
        sr_units_kernel<<<divUp(n, 256), 256, 0, st>>>(keyS.p, xsS.p, fCount.p, pCount.p, n, units, uX.p, uOrd.p);
        H10X_HIP(c, hipGetLastError());
      }
      H10X_HIP(c, hipMemcpyAsync(hFig.data(), dFig.p, (size_t)12 * ns, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipMemcpyAsync(hUOff.data(), uOff.p, ((size_t)ns + 1) * 8, hipMemcpyDeviceToHost, st));
      H10X_HIP(c, hipStreamSynchronize(st));                  // (the slab's temporaries go back to the cache behind finished work)
    }
    if (units) {
      std::vector<u64> size(ns);
      H10X_TRY(sizes(0, ns, 0, c->nBlocks, true, size.data()));
      H10X_TRY(cut_batches(size.data(), ns, c->nBlocks, budget,
                           [&](u32 q, u32 lo, u32 hi, u64 *records) { return sizes(q, 1, lo, hi, false, records); },
                           [&](u32 q0, u32 m, u32 lo, u32 hi, bool full, u64 total) { return batch(q0, m, lo, hi, full, total); }));
    }
    H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, rowCnt.p, rowOff.p, (size_t)ns + 1));
    H10X_HIP(c, hipMemcpyAsync(hRowOff.data(), rowOff.p, ((size_t)ns + 1) * 8, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    if (hRowOff[ns] != rows - row0) return c->fail("seqSpans: %llu extents kept and %llu in the rows", rows - row0, hRowOff[ns]);
    H10X_TRY(cover(row0, slabStart, coverOff));
    for (u32 s = 0; s < ns; ++s) {
      const u32 *f = hFig.data() + (size_t)3 * s;
      offsets[s + 1] = offsets[0] + hRowOff[s + 1];
      if (fig) { h10x_seq_span_figures &o = fig[s]; o.len = slabStart[s + 1] - slabStart[s]; o.moshes = f[0]; o.found = f[1]; o.inRange = f[2]; o.extents = (u32)(hRowOff[s + 1] - hRowOff[s]); }
      info->moshes += f[0]; info->found += f[1]; info->inRange += f[2];
    }
    info->bases += bases;
    return 0;
  }

  int run(const u8 *codes, const u64 *seqStart, u32 nSeq, h10x_seq_span_figures *fig) {
    const u64 slabBases = c->optSeqSlab > 0 ? (u64)c->optSeqSlab : MOSH_SLAB_DEFAULT;
    for (u32 s = 0; s < nSeq; ++s)                              // the scan trusts the lengths
      if (seqStart[s + 1] < seqStart[s]) return c->fail("seqSpans: the sequence starts do not ascend at sequence %u", s);
    c->ssHostOff.assign((size_t)nSeq + 1, 0); c->ssHostCoverOff.assign((size_t)nSeq + 1, 0);
    for (u32 s0 = 0; s0 < nSeq;) {
      u32 s1 = s0 + 1;                                          // as many whole sequences as fit the slab; a longer one goes alone (moshBatches)
      while (s1 < nSeq && seqStart[s1 + 1] - seqStart[s0] <= slabBases) ++s1;
      H10X_TRY(slab(codes, seqStart + s0, s1 - s0, fig ? fig + s0 : nullptr, c->ssHostOff.data() + s0, c->ssHostCoverOff.data() + s0));
      s0 = s1;
    }
    for (DevBuf<u32> *b : {&c->ssBlock, &c->ssFirst, &c->ssLast, &c->ssHits, &c->ssCover}) if (!b->p) H10X_HIP(c, b->alloc(1));
    info->extents = rows; info->boundaries = covered;
    if (rows) {                                               // the three figures of the summary line
      hipStream_t st = c->stream;
      DevBuf<u32> span, mx; DevBuf<u64> sum;
      H10X_HIP(c, span.alloc(rows)); H10X_HIP(c, mx.alloc(2)); H10X_HIP(c, sum.alloc(1));
      sr_span_kernel<<<divUp(rows, 256), 256, 0, st>>>(c->ssFirst.p, c->ssLast.p, rows, span.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_reduce_max_u32(c, pt, c->ssHits.p, mx.p, rows)); H10X_TRY(prim_reduce_max_u32(c, pt, span.p, mx.p + 1, rows));
      H10X_TRY(prim_reduce_sum_u32_u64(c, pt, span.p, sum.p, rows));
      u32 m[2] = {0, 0}; unsigned long long total = 0;
      H10X_TRY(c->readback(m, mx.p, 8)); H10X_TRY(c->readback(&total, sum.p, 8)); H10X_TRY(c->syncReadbacks());
      info->maxHits = m[0]; info->maxSpan = m[1]; info->sumSpan = total;
    }
    H10X_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
  }
};

const char *const SS_NONE = "seqSpans: no extents are kept (run it first; a new range, --clusterSplit and a new state release them)";
}  // namespace

void stageR_release(Ctx *c) {
  c->haveSeqSpans = false; c->ssExtents = 0; c->ssBoundaries = 0; c->ssSeqs = 0; c->ssHostOff.clear(); c->ssHostCoverOff.clear();
  for (DevBuf<u32> *b : {&c->ssBlock, &c->ssFirst, &c->ssLast, &c->ssHits, &c->ssCover}) b->release();
}

int stageR_run(Ctx *c, int64_t minShare, int64_t maxGap, int64_t window, const u8 *codes, const u64 *seqStart, u32 nSeq, h10x_seq_span_figures *fig,
               h10x_seq_spans_info *info) {
  stageR_release(c);
  H10X_TRY(sp_check(c, "seqSpans", minShare, true));
  if (maxGap < 0) return c->fail("!! seqSpans maxGap %lld must be >= 0", (long long)maxGap);
  if (window < 0) return c->fail("!! seqSpans window %lld must be >= 0", (long long)window);
  if (nSeq && (!codes || !seqStart)) return c->fail("seqSpans: null argument");
  memset(info, 0, sizeof *info);
  info->sequences = nSeq; info->nBlocks = c->nBlocks;
  SeqSpans g; g.c = c; g.info = info;
  // a position is a u32: a threshold, gap or window beyond it acts as the largest u32 does
  g.T = (u32)hmin<int64_t>(minShare, 0xFFFFFFFFll); g.G = (u32)hmin<int64_t>(maxGap, 0xFFFFFFFFll); g.W = (u32)hmin<int64_t>(window, 0xFFFFFFFFll);
  g.budget = c->optNbBudget > 0 ? (u64)c->optNbBudget : ROWS_DEFAULT_BUDGET;
  const u64 zero = 0;
  const int rc = g.run(codes, nSeq ? seqStart : &zero, nSeq, fig);
  if (rc) { (void)hipStreamSynchronize(c->stream); stageR_release(c); return rc; }
  c->ssExtents = g.rows; c->ssBoundaries = g.covered; c->ssSeqs = nSeq; c->haveSeqSpans = true;
  return 0;
}

int stageR_getRange(Ctx *c, u64 firstRow, u64 count, u32 *block, u32 *first, u32 *last, u32 *hits) {
  if (!c->haveSeqSpans) return c->fail("%s", SS_NONE);
  if (firstRow > c->ssExtents || count > c->ssExtents - firstRow) return c->fail("seqSpans: rows %llu .. %llu of %llu", firstRow, firstRow + count, c->ssExtents);
  u32 *const dst[4] = {block, first, last, hits}; const u32 *const src[4] = {c->ssBlock.p, c->ssFirst.p, c->ssLast.p, c->ssHits.p};
  for (int k = 0; k < 4; ++k)
    if (count && dst[k]) H10X_HIP(c, hipMemcpyAsync(dst[k], src[k] + firstRow, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int stageR_get(Ctx *c, u64 *offsets, u32 *block, u32 *first, u32 *last, u32 *hits, u64 cap) {
  if (!c->haveSeqSpans) return c->fail("%s", SS_NONE);
  if (offsets) memcpy(offsets, c->ssHostOff.data(), ((size_t)c->ssSeqs + 1) * 8);
  return stageR_getRange(c, 0, hmin<u64>(cap, c->ssExtents), block, first, last, hits);
}

int stageR_coverGet(Ctx *c, u64 *coverOffsets, u32 *cover, u64 cap) {
  if (!c->haveSeqSpans) return c->fail("%s", SS_NONE);
  if (coverOffsets) memcpy(coverOffsets, c->ssHostCoverOff.data(), ((size_t)c->ssSeqs + 1) * 8);
  const size_t m = (size_t)hmin<u64>(cap, c->ssBoundaries);
  if (m && cover) H10X_HIP(c, hipMemcpyAsync(cover, c->ssCover.p, m * 4, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace h10x
