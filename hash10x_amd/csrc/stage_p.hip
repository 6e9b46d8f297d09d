// stage_p.hip — from sequences to blocks, behind --seqBlocks: which blocks' barcode lists hold the hashes of a sequence (include/h10x.h "from a
// sequence to its blocks"). Two layers.
//
// Layer 1, sequence -> query list, per slab of whole sequences:
//   scan     stage_g's mosh_scan_kernel<0> with the CONTEXT's hasher (k, w, factor1): every mosh occurrence as (hash, ordinal of its k-mer in the slab);
//   look-up  one lane per occurrence: its sequence by a search in the slab's sequence starts, its index x by hashIndexFind's slot and stride in the
//            state's own table, and the key (sequence in slab) << keyBits(hashNumber) | f with f = 0 absent, x in range, hashNumber found but out of
//            range (no index has that value);
//   sort     prim_sort_keys_u64 on the bits in use;
//   heads    flag = first key of a run whose f is an in-range index; a scan of the flags numbers them, compact writes the indices back to back
//            behind those of the slabs before: per sequence ascending, each once;
//   figures  one wave per sequence: four searches in the sorted keys give moshes, found and the ends of the in-range stretch, the scan gives query and
//            the list's place, and the wave sums hashDepth[] over the list (entries). No atomic anywhere: every figure is a difference of positions.
// Layer 2, query lists -> rows (the list census): stage_l.hip's scan-placed form with a hash list given from outside instead of a block's good ranks.
//   sizes    one wave per list: the entries of its hashes' barcode lists in the window (the batches are cut by these);
//   units    one lane per (list, hash) unit: the entries of that barcode list in the window; their exclusive sum is every unit's place;
//   gather   one wave per unit: key = (list - first of batch) << keyBits(nBlocks) | d. Nothing is left out (no own block here), so a lane's place is
//            the unit's place + its position in the list and there is no ballot. 32-bit keys where slot and block fit, else 64-bit;
//   tail     census_rows.hip: the keys sorted, a run of equal keys is one (list, d) with count = its length, the runs of length >= T placed by a scan
//            as rows (d, count) behind those of the batches before, the rows per list summed to offsets[].
// Batches are cut by list entries against "neighbour_budget"; a list above it runs alone in windows of block index (whole runs each: the lists ascend).
#include "census_rows.hpp"
#include "mosh.hpp"
#include "wave.hpp"

namespace h10x {

// ------------------------------------------------------------------------------------------------ layer 1
// occurrence i of the slab -> key[i]. seqRel[0 .. ns] = the slab's sequence starts (seqRel[0] = 0), ord[i] = the ordinal of the k-mer in the slab
__global__ __launch_bounds__(256) void sp_lookup_kernel(const u64 *__restrict__ hash, const u32 *__restrict__ ord, u64 n, const u64 *__restrict__ seqRel, u32 ns,
                                                        const u32 *__restrict__ table, const u64 *__restrict__ hashValue, int B, const u8 *__restrict__ within,
                                                        u32 U1, int hb, u64 *__restrict__ key) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const u32 s = last_le(seqRel, ns, (u64)ord[i]);
    u32 x = probe_find(table, hashValue, B, hash[i]);
    if (x >= U1) x = 0;                                       // (a table entry beyond hashNumber is no index of this state)
    const u32 f = !x ? 0u : within[x] ? x : U1;
    key[i] = (u64)s << hb | (u64)f;
  }
}

// flag[i] = 1 at the first key of a run whose low field is an in-range index; flag[n] = 0 (the scan's last entry is their number)
__global__ void sp_heads_kernel(const u64 *__restrict__ key, u64 n, u32 U1, int hb, u32 *__restrict__ flag) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  u32 f = 0;
  if (i < n) {
    const u64 k = key[i]; const u32 x = (u32)(k & (((u64)1 << hb) - 1));
    f = (x >= 1 && x < U1 && (!i || key[i - 1] != k)) ? 1u : 0u;
  }
  flag[i] = f;
}

__global__ void sp_compact_kernel(const u64 *__restrict__ key, const u32 *__restrict__ flag, const u32 *__restrict__ pos, u64 n, int hb, u32 cap,
                                  u32 *__restrict__ out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const u32 p = pos[i];
  if (p < cap) out[p] = (u32)(key[i] & (((u64)1 << hb) - 1));
}

// one wave per sequence s of the slab: fig[s] = {moshes, found, query, 0, entries lo, entries hi}; list = the slab's compacted indices
__global__ __launch_bounds__(256) void sp_figures_kernel(const u64 *__restrict__ key, u64 n, const u32 *__restrict__ pos, const u32 *__restrict__ list, u32 ns,
                                                         u32 U1, int hb, const u32 *__restrict__ hashDepth, u32 *__restrict__ fig) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u32 s = (u32)(((u64)blockIdx.x * blockDim.x + threadIdx.x) / WAVE);
  if (s >= ns) return;                                        // whole waves leave: the fold below sees all 64 lanes
  const u64 k0 = (u64)s << hb;
  const u64 a = lower_bound(key, (u64)0, n, k0), z = lower_bound(key, a, n, k0 | 1), o = lower_bound(key, z, n, k0 | (u64)U1);
  const u64 e = lower_bound(key, o, n, ((u64)s + 1) << hb);
  const u32 q0 = pos[z], q1 = pos[o];
  u64 sum = 0;
  for (u32 j = q0 + lane; j < q1; j += WAVE) sum += hashDepth[list[j]];
  sum = wave_sum(sum);
  if (lane == 0) {
    u32 *f = fig + (size_t)6 * s;
    f[0] = (u32)(e - a); f[1] = (u32)(e - z); f[2] = q1 - q0; f[3] = 0; f[4] = (u32)sum; f[5] = (u32)(sum >> 32);
  }
}

// ------------------------------------------------------------------------------------------------ layer 2
// (sp_window, the entries of a hash's barcode list in the window: wave.hpp)
// one wave per list q0 + q: size[q] = entries of its hashes' lists in the window
__global__ void sp_size_kernel(u32 nq, const u64 *__restrict__ qOff /* at q0 */, const u32 *__restrict__ qHash, const u64 *__restrict__ rowStart,
                               const u32 *__restrict__ hashDepth, const u32 *__restrict__ rows, u32 lo, u32 hi, int full, u64 *__restrict__ size) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u32 q = (u32)(((u64)blockIdx.x * blockDim.x + threadIdx.x) / WAVE);
  if (q >= nq) return;
  u64 s = 0;
  for (u64 j = qOff[q] + lane; j < qOff[q + 1]; j += WAVE) { u64 a, b; sp_window(rows, rowStart, hashDepth, qHash[j], lo, hi, full != 0, a, b); s += b - a; }
  s = wave_sum(s);
  if (lane == 0) size[q] = s;
}

// one lane per unit u0 + u: listCnt[u] = entries of its list in the window; listCnt[units] = 0
__global__ void sp_unit_kernel(u64 u0, u64 units, const u32 *__restrict__ qHash, const u64 *__restrict__ rowStart, const u32 *__restrict__ hashDepth,
                               const u32 *__restrict__ rows, u32 lo, u32 hi, int full, u32 *__restrict__ listCnt) {
  const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (u > units) return;
  u32 n = 0;
  if (u < units) { u64 a, b; sp_window(rows, rowStart, hashDepth, qHash[u0 + u], lo, hi, full != 0, a, b); n = (u32)(b - a); }
  listCnt[u] = n;
}

// one wave per unit; the list's keys go to [listPos[u], listPos[u + 1]) in list order. cap = listPos[units]: a miscount stays in bounds
template <typename K>
__global__ __launch_bounds__(256) void sp_gather_kernel(u32 nq, const u64 *__restrict__ qOff /* at q0 */, const u32 *__restrict__ qHash,
                                                        const u64 *__restrict__ rowStart, const u32 *__restrict__ hashDepth, const u32 *__restrict__ rows, u32 lo,
                                                        u32 hi, int full, int cbits, const u64 *__restrict__ listPos, u64 cap, K *__restrict__ keys) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u64 base = qOff[0], units = qOff[nq] - base;
  const u64 w0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / WAVE, wStride = ((u64)gridDim.x * blockDim.x) / WAVE;
  for (u64 u = w0; u < units; u += wStride) {
    const u32 q = last_le(qOff, nq, base + u);
    u64 a, b; sp_window(rows, rowStart, hashDepth, qHash[base + u], lo, hi, full != 0, a, b);
    const K tag = (K)q << cbits;
    const u64 p0 = listPos[u];
    for (u64 j = a + lane; j < b; j += WAVE) {
      const u64 p = p0 + (j - a);
      if (p < cap) keys[p] = tag | (K)rows[j];
    }
  }
}

// ------------------------------------------------------------------------------------------------ drivers
// the refusals both layers share (and stage_r.hip); the hasher's seed as h10x_mosh_from_state takes it
int sp_check(Ctx *c, const char *cmd, int64_t minShare, bool hasher) {
  H10X_TRY(ce_check(c, cmd, minShare));
  if (!c->haveRange) return c->fail("!! you must set hashDepthRange before %s", cmd);
  return hasher ? sp_check_hasher(c, cmd) : 0;
}

// the two checks of the hasher alone, for a command that needs no range (stage_s.hip)
int sp_check_hasher(Ctx *c, const char *cmd) {
  if (!c->haveSeed) return c->fail("%s: the context does not know the seed of its hasher: set option seqhash_seed to the -r value", cmd);
  u64 f1 = 0, f2 = 0; h10x_factors_from_seed(c->seed, (uint64_t *)&f1, (uint64_t *)&f2);
  if (f1 != c->prm.factor1) return c->fail("%s: option seqhash_seed %d does not give the context's hash multiplier", cmd, c->seed);
  return 0;
}

namespace {

void release_lists(Ctx *c) { c->haveSeqHashes = false; c->sqSeqs = 0; c->sqEntries = 0; c->sqHash.release(); c->sqOffsets.release(); c->sqHostOff.clear(); }

// ---- layer 1: the lists of sequences [0, nSeq) into c->sqHash / sqOffsets, the figures to fig[nSeq] (host)
int seq_lists(Ctx *c, const u8 *codes, const u64 *seqStart, u32 nSeq, h10x_seq_figures *fig) {
  hipStream_t st = c->stream; PrimTemp pt;
  const u32 U1 = c->hashNumber; const int hb = keyBits(U1);
  const u64 slab = c->optSeqSlab > 0 ? (u64)c->optSeqSlab : MOSH_SLAB_DEFAULT;
  for (u32 s = 0; s < nSeq; ++s)                              // the scan trusts the lengths
    if (seqStart[s + 1] < seqStart[s]) return c->fail("seqHashes: the sequence starts do not ascend at sequence %u", s);
  c->sqHostOff.assign((size_t)nSeq + 1, 0);
  u64 used = 0;
  DevBuf<u64> key, keyS; DevBuf<u32> flag, pos, dFig, part;
  std::vector<u32> hFig;
  for (u32 s0 = 0; s0 < nSeq;) {
    u32 s1 = s0 + 1;                                          // as many whole sequences as fit the slab; a longer one goes alone (moshBatches)
    while (s1 < nSeq && seqStart[s1 + 1] - seqStart[s0] <= slab) ++s1;
    const u32 ns = s1 - s0;
    MoshBatch b;
    H10X_TRY(moshScanWith(c, c->prm.k, c->prm.w, c->prm.factor1, c->prm.B, nullptr, 0, b, codes, seqStart + s0, ns, 0, 0));
    const u64 n = b.listed;
    if (n > 0xFFFFFFFEull) return c->fail("seqHashes: %llu moshes in one batch", n);
    u32 kept = 0;
    hFig.assign((size_t)6 * ns, 0);
    if (n) {
      const int endBit = hb + keyBits(ns - 1);
      if (endBit > 63) return c->fail("seqHashes: %u sequences in one batch with %u hashes", ns, U1);
      H10X_HIP(c, key.alloc(n)); H10X_HIP(c, keyS.alloc(n)); H10X_HIP(c, flag.alloc(n + 1)); H10X_HIP(c, pos.alloc(n + 1)); H10X_HIP(c, dFig.alloc((size_t)6 * ns));
      sp_lookup_kernel<<<(unsigned)hmin<u64>(divUp(n, 256), 16384), 256, 0, st>>>(b.outHash.p, b.outOrd.p, n, b.seq.p, ns, c->hashIndex.p, c->hashValue.p, c->prm.B,
                                                                                   c->within.p, U1, hb, key.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_sort_keys_u64(c, pt, key.p, keyS.p, n, 0, endBit));
      sp_heads_kernel<<<divUp(n + 1, 256), 256, 0, st>>>(keyS.p, n, U1, hb, flag.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, pos.p, n + 1));
      H10X_TRY(c->readback(&kept, pos.p + n, 4)); H10X_TRY(c->syncReadbacks());
      H10X_HIP(c, part.alloc(hmax<u32>(kept, 1)));
      if (kept) {
        sp_compact_kernel<<<divUp(n, 256), 256, 0, st>>>(keyS.p, flag.p, pos.p, n, hb, kept, part.p);
        H10X_HIP(c, hipGetLastError());
      }
      sp_figures_kernel<<<divUp((u64)ns * WAVE, 256), 256, 0, st>>>(keyS.p, n, pos.p, part.p, ns, U1, hb, c->hashDepth.p, dFig.p);
      H10X_HIP(c, hipGetLastError());
      H10X_HIP(c, hipMemcpyAsync(hFig.data(), dFig.p, (size_t)24 * ns, hipMemcpyDeviceToHost, st));
      if (kept) {
        H10X_TRY(reserve_keep(c, c->sqHash, used, used + kept));
        H10X_HIP(c, hipMemcpyAsync(c->sqHash.p + used, part.p, (size_t)kept * 4, hipMemcpyDeviceToDevice, st));
      }
      H10X_HIP(c, hipStreamSynchronize(st));
    }
    u64 sum = 0;
    for (u32 s = 0; s < ns; ++s) {
      const u32 *f = hFig.data() + (size_t)6 * s;
      if (fig) { h10x_seq_figures &o = fig[s0 + s]; o.moshes = f[0]; o.found = f[1]; o.query = f[2]; o.reserved = 0; o.entries = (u64)f[4] | (u64)f[5] << 32; }
      sum += f[2];
      c->sqHostOff[(size_t)s0 + s + 1] = used + sum;
    }
    if (sum != kept) return c->fail("seqHashes: %u indices kept at the scan and %llu in the figures", kept, sum);
    used += kept;
    s0 = s1;
  }
  H10X_HIP(c, c->sqOffsets.alloc((size_t)nSeq + 1));
  H10X_HIP(c, hipMemcpyAsync(c->sqOffsets.p, c->sqHostOff.data(), ((size_t)nSeq + 1) * 8, hipMemcpyHostToDevice, st));
  if (!c->sqHash.p) H10X_HIP(c, c->sqHash.alloc(1));
  H10X_HIP(c, hipStreamSynchronize(st));
  c->sqSeqs = nSeq; c->sqEntries = used; c->haveSeqHashes = true;
  return 0;
}

// ---- layer 2
struct ListShare {
  Ctx *c; u32 nq; u64 budget;
  const u64 *hOff; const u64 *dOff; const u32 *dHash;       // the lists: offsets on the host and the device, indices on the device
  std::vector<u64> size;
  DevBuf<u64> listPos, dSize; DevBuf<u32> listCnt;
  RowTail tail;

  int sizes(u32 q0, u32 n, u32 lo, u32 hi, bool full, u64 *hSize) {
    hipStream_t st = c->stream;
    H10X_HIP(c, dSize.alloc(n));
    sp_size_kernel<<<divUp((u64)n * WAVE, 256), 256, 0, st>>>(n, dOff + q0, dHash, c->rowStart.p, c->hashDepth.p, c->rows.p, lo, hi, full ? 1 : 0, dSize.p);
    H10X_HIP(c, hipGetLastError());
    H10X_HIP(c, hipMemcpyAsync(hSize, dSize.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    return 0;
  }

  template <typename K>
  int gather(K *keys, u32 q0, u32 n, u32 lo, u32 hi, bool full, int cbits, u64 units, u64 nKeys) {
    sp_gather_kernel<K><<<(unsigned)hmin<u64>(divUp(units, 4), 65536), 256, 0, c->stream>>>(n, dOff + q0, dHash, c->rowStart.p, c->hashDepth.p, c->rows.p, lo, hi,
                                                                                         full ? 1 : 0, cbits, listPos.p, nKeys, keys);
    H10X_HIP(c, hipGetLastError());
    return 0;
  }

  // lists [q0, q0 + n) in the window [lo, hi); total = list entries gathered
  int batch(u32 q0, u32 n, u32 lo, u32 hi, bool full, u64 total) {
    tail.batch(full);                                         // (a window: of a list above the budget)
    if (!total) return 0;
    if (total >= 0xFFFFFFFFull) return c->fail("listShare: %llu list entries in one batch, beyond 2^32 (list %u alone)", total, q0);
    const u64 u0 = hOff[q0], units = hOff[q0 + n] - u0;
    if (listCnt.n < units + 1) { H10X_HIP(c, listCnt.alloc(units + 1)); H10X_HIP(c, listPos.alloc(units + 1)); }
    sp_unit_kernel<<<divUp(units + 1, 256), 256, 0, c->stream>>>(u0, units, dHash, c->rowStart.p, c->hashDepth.p, c->rows.p, lo, hi, full ? 1 : 0, listCnt.p);
    H10X_HIP(c, hipGetLastError());
    u64 nKeys = 0;
    H10X_TRY(tail.places(listCnt.p, listPos.p, units, &nKeys));
    if (nKeys != total) return c->fail("listShare: %llu keys of %llu list entries", nKeys, total);
    tail.gathered(total, nKeys);
    const int cbits = keyBits(c->nBlocks), endBit = cbits + keyBits(n - 1);
    H10X_TRY(tail.keys(nKeys, endBit > 32));
    H10X_TRY(endBit > 32 ? gather(tail.keys64.p, q0, n, lo, hi, full, cbits, units, nKeys) : gather(tail.keys32.p, q0, n, lo, hi, full, cbits, units, nKeys));
    return tail.emit(nKeys, cbits, endBit, q0, n);
  }

  int run(u32 T, u32 *maxCount) {
    size.resize(nq);
    H10X_TRY(sizes(0, nq, 0, c->nBlocks, true, size.data()));
    H10X_TRY(tail.begin(c, &c->sb, T, nq));
    H10X_TRY(cut_batches(size.data(), nq, c->nBlocks, budget,
                         [&](u32 q, u32 lo, u32 hi, u64 *records) { return sizes(q, 1, lo, hi, false, records); },
                         [&](u32 q0, u32 n, u32 lo, u32 hi, bool full, u64 total) { return batch(q0, n, lo, hi, full, total); }));
    return tail.finish(maxCount);
  }
};

// the census over lists already on the device (hOff = the same offsets on the host); the checks are the caller's
int list_share(Ctx *c, int64_t minShare, const u64 *hOff, const u64 *dOff, const u32 *dHash, u32 nq, h10x_list_share_info *info) {
  memset(info, 0, sizeof *info);
  info->nBlocks = c->nBlocks; info->lists = nq; info->listHashes = nq ? hOff[nq] : 0;
  ListShare g; g.c = c; g.nq = nq; g.hOff = hOff; g.dOff = dOff; g.dHash = dHash;
  g.budget = c->optNbBudget > 0 ? (u64)c->optNbBudget : ROWS_DEFAULT_BUDGET;
  if (!nq) {
    H10X_HIP(c, c->sb.offsets.alloc(1)); H10X_HIP(c, hipMemsetAsync(c->sb.offsets.p, 0, 8, c->stream));
  } else {
    u32 mx = 0;
    const int rc = g.run((u32)hmin<int64_t>(minShare, 0xFFFFFFFFll), &mx);
    if (rc) { (void)hipStreamSynchronize(c->stream); c->sb.release(); return rc; }
    info->maxCount = mx;
  }
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  c->sb.have = true; c->sb.rows = g.tail.rows; c->sb.lists = nq;
  info->rows = g.tail.rows; info->listEntries = g.tail.entries; info->batches = g.tail.batches; info->windows = g.tail.windows; info->wideBatches = g.tail.wide;
  return 0;
}
}  // namespace

void stageP_release(Ctx *c) { release_lists(c); c->sb.release(); }

int stageP_seqHashes(Ctx *c, const u8 *codes, const u64 *seqStart, u32 nSeq, h10x_seq_figures *fig) {
  release_lists(c);
  H10X_TRY(sp_check(c, "seqHashes", 1, true));
  if (nSeq && (!codes || !seqStart)) return c->fail("seqHashes: null argument");
  const u64 zero = 0;
  const int rc = seq_lists(c, codes, nSeq ? seqStart : &zero, nSeq, fig);
  if (rc) { (void)hipStreamSynchronize(c->stream); release_lists(c); }
  return rc;
}

// offsets[nSeq + 1] and the first min(cap, entries) indices of the kept lists, to host memory; either may be null
int stageP_seqHashesGet(Ctx *c, u64 *offsets, u32 *hashes, u64 cap) {
  if (!c->haveSeqHashes) return c->fail("seqHashes: no lists are kept (run it first; a new range, --clusterSplit and a new state release them)");
  if (offsets) memcpy(offsets, c->sqHostOff.data(), ((size_t)c->sqSeqs + 1) * 8);
  const size_t m = (size_t)hmin<u64>(cap, c->sqEntries);
  if (m && hashes) H10X_HIP(c, hipMemcpyAsync(hashes, c->sqHash.p, m * 4, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int stageP_listShare(Ctx *c, int64_t minShare, const u64 *offsets, const u32 *hashes, u32 nq, h10x_list_share_info *info) {
  c->sb.release();
  H10X_TRY(sp_check(c, "listShare", minShare, false));
  if (nq && (!offsets || (offsets[nq] && !hashes))) return c->fail("listShare: null argument");
  const u64 zero = 0;
  if (!nq) offsets = &zero;
  if (offsets[0]) return c->fail("!! listShare offsets must start at 0");
  for (u32 q = 0; q < nq; ++q) {
    if (offsets[q + 1] < offsets[q]) return c->fail("!! listShare offsets descend at list %u", q);
    for (u64 j = offsets[q]; j < offsets[q + 1]; ++j)
      if (hashes[j] < 1 || hashes[j] >= c->hashNumber)
        return c->fail("!! listShare list %u entry %llu: hash index %u is not in 1 .. %u", q, j - offsets[q], hashes[j], c->hashNumber - 1);
  }
  hipStream_t st = c->stream;
  const u64 total = offsets[nq];
  DevBuf<u64> dOff; DevBuf<u32> dHash;
  H10X_HIP(c, dOff.alloc((size_t)nq + 1)); H10X_HIP(c, dHash.alloc(hmax<u64>(total, 1)));
  H10X_HIP(c, hipMemcpyAsync(dOff.p, offsets, ((size_t)nq + 1) * 8, hipMemcpyHostToDevice, st));
  if (total) H10X_HIP(c, hipMemcpyAsync(dHash.p, hashes, (size_t)total * 4, hipMemcpyHostToDevice, st));
  const int rc = list_share(c, minShare, offsets, dOff.p, dHash.p, nq, info);
  (void)hipStreamSynchronize(st);                             // the uploads and the temporaries go back to the block cache behind finished work
  return rc;
}

int stageP_seqBlocks(Ctx *c, int64_t minShare, const u8 *codes, const u64 *seqStart, u32 nSeq, h10x_seq_figures *fig, h10x_list_share_info *info) {
  stageP_release(c);
  H10X_TRY(sp_check(c, "seqBlocks", minShare, true));
  if (nSeq && (!codes || !seqStart)) return c->fail("seqBlocks: null argument");
  const u64 zero = 0;
  int rc = seq_lists(c, codes, nSeq ? seqStart : &zero, nSeq, fig);
  if (!rc) rc = list_share(c, minShare, c->sqHostOff.data(), c->sqOffsets.p, c->sqHash.p, nSeq, info);
  if (rc) { (void)hipStreamSynchronize(c->stream); stageP_release(c); }
  return rc;
}

int stageP_get(Ctx *c, u64 *offsets, u32 *block, u32 *count, u64 cap, int toDevice) {
  return c->sb.get(c, offsets, block, count, cap, toDevice, "seqBlocks: no rows are kept (run it first; a new range, --clusterSplit and a new state release them)");
}

}  // namespace h10x
