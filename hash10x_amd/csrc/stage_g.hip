// stage_g.hip — mosh sets: the object behind moshutils (moshset.c, moshutils.c:19-76 of the reference).
//
// A set is index[2^B] (the probe table of moshsetIndexFind, moshset.c:45-61: hashIndexFind's geometry) and per index
// 1 .. max value (u64 hash), depth (u16), info (u8, low two bits = copy class). Three facts make a parallel build exact:
//   1. index order = order of a hash's FIRST occurrence (sequence order of the file, then position);
//   2. the table is a fixed point: a hash sits in the first slot of its probe sequence not held by a LOWER index, so
//      inserting a batch of new (higher) indices by compare-and-evict ends in the table the sequential loop builds
//      and nothing already placed moves ("Index build");
//   3. depth = min(65535, depth + occurrences) (moshutils.c:26: ++depth, a wrap to 0 becomes 65535), so occurrences may
//      be counted in any order.
// -a / -x, per batch of whole sequences: scan (one lane per run of k-mer start positions, the one walk of seq_scan.hpp;
// a hit adds 1 to a 32-bit accumulator of its index, a miss appends (hash, ordinal) to a list whose space is reserved
// once per wave step: wave_append) -> sort the misses by hash -> per distinct hash its count and lowest ordinal
// -> sort those by ordinal -> index = max + 1 + rank -> insert -> fold the accumulators into depth[].
#include "common.hpp"
#include "prim.hpp"
#include "mosh.hpp"
#include <new>

namespace h10x {

// ------------------------------------------------------------------------------------------------ kernels
// The batch as its SeqPlan lays it out (seqStart = rel[], runStart; skipOdd and seqBase = its SeqSkip).
// ADD = 0: every mosh goes to the list; ADD = 1: a mosh found in the table counts in acc[], the others go to the list.
// Both loops have the same trip count in every lane of a wave: the ballots of wave_append see all 64 lanes.
template <int ADD>
__global__ __launch_bounds__(256)
void mosh_scan_kernel(const u8 *__restrict__ codes, const u64 *__restrict__ seqStart, const u64 *__restrict__ runStart, u32 nSeq,
                      int skipOdd, u64 seqBase, int k, int w, u64 factor1,
                      const u32 *__restrict__ table, const u64 *__restrict__ value, int B, u32 *__restrict__ acc,
                      u64 *__restrict__ outHash, u32 *__restrict__ outOrd, u64 cap, u64 *__restrict__ tallies /* listed, found */) {
  const u64 nRuns = runStart[nSeq];
  const u64 T = (u64)gridDim.x * blockDim.x, iters = (nRuns + T - 1) / T;
  const int lane = threadIdx.x & (WAVE - 1);
  u64 found = 0;
  for (u64 it = 0; it < iters; ++it) {
    const u64 run = it * T + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    KmerRun r = {0, 0, 0, 0, codes}; KmerRoll roll(k, factor1);   // (a lane beyond the last run walks nothing and takes part in the ballots)
    if (run < nRuns) { r = KmerRun::open(codes, seqStart, runStart, nSeq, run, k, SeqSkip{skipOdd, seqBase}); roll.prime(r.b); }
    for (int j = 0; j < SEQ_RUN; ++j) {
      bool emit = false; u64 h = 0;
      if (j < r.cnt) {
        h = roll.next(r.b[k - 1 + j]);
        if (h % (u64)w == 0) {
          if (ADD) {
            const u32 ix = probe_find(table, value, B, h);
            if (ix) { atomicAdd(&acc[ix], 1u); ++found; } else emit = true;
          } else emit = true;
        }
      }
      const u64 at = wave_append(emit, &tallies[0]);
      if (emit && at < cap) { outHash[at] = h; outOrd[at] = (u32)(r.ord0 + (u64)j); }
    }
  }
  for (int o = 32; o; o >>= 1) found += __shfl_down(found, o);
  if (lane == 0 && found) atomicAdd((unsigned long long *)&tallies[1], (unsigned long long)found);
}

__global__ void mosh_heads_kernel(const u64 *__restrict__ key, u64 n, u32 *__restrict__ flag) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}
// runs of equal hash in the sorted miss list: run r = before[i] + flag[i] - 1
__global__ void mosh_runs_kernel(const u64 *__restrict__ key, const u32 *__restrict__ ord, const u32 *__restrict__ flag, const u32 *__restrict__ before, u64 n,
                                 u64 *__restrict__ runHash, u32 *__restrict__ runFirst, u32 *__restrict__ runMinOrd) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 r = before[i] + flag[i] - 1;
  if (flag[i]) { runHash[r] = key[i]; runFirst[r] = (u32)i; }
  atomicMin(&runMinOrd[r], ord[i]);
}
// rank j of the distinct new hashes in first-appearance order -> index first + j
__global__ void mosh_assign_kernel(const u32 *__restrict__ rankRun, u32 D, u64 nMiss, const u64 *__restrict__ runHash, const u32 *__restrict__ runFirst,
                                   u32 first, u64 *__restrict__ value, u16 *__restrict__ depth, u8 *__restrict__ info, u32 *__restrict__ acc) {
  const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= D) return;
  const u32 r = rankRun[j], ix = first + (u32)j;
  const u32 end = r + 1 < D ? runFirst[r + 1] : (u32)nMiss;
  value[ix] = runHash[r]; depth[ix] = 0; info[ix] = 0; acc[ix] = end - runFirst[r];
}
// moshsetIndexFind(.., TRUE) for indices [first, first + count) whose value[] is written: table entry 0 = empty. An index
// takes the first slot of its probe sequence that is empty or held by a HIGHER index; the one it displaces walks on
// from there with its own stride. Indices below `first` are never displaced.
__global__ void mosh_insert_kernel(const u64 *__restrict__ value, u32 first, u32 count, int B, u32 *__restrict__ table) {
  const u64 mask = ((u64)1 << B) - 1;
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (u64)gridDim.x * blockDim.x) {
    u32 cur = first + (u32)t;
    u64 h = value[cur];
    u64 slot = h & mask, step = ((h >> B) & mask) | 1;
    for (;;) {
      u32 old = __hip_atomic_load(&table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == 0) { old = atomicCAS(&table[slot], 0u, cur); if (old == 0) break; }
      if (old > cur) {
        if (atomicCAS(&table[slot], old, cur) != old) continue;   // changed under us: look at the slot again
        cur = old; h = value[cur]; step = ((h >> B) & mask) | 1;
      }
      slot = (slot + step) & mask;
    }
  }
}
__global__ void mosh_fold_kernel(u16 *__restrict__ depth, u32 *__restrict__ acc, u32 n1) {   // moshutils.c:26, moshasm.c:148: ++depth, a wrap to 0 becomes 65535
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // 64-bit: a set may hold up to 2^32 - 2 entries (B = 34)
  if (i == 0 || i >= n1) return;
  const u32 a = acc[i];
  if (a) { const u32 d = (u32)depth[i] + a; depth[i] = (u16)(d > 65535u || d < a ? 65535u : d); acc[i] = 0; }
}

// moshsetMerge (moshset.c:112-118) in three steps: find, number + place the misses, apply
__global__ void mosh_merge_find_kernel(const u64 *__restrict__ v2, u32 n1 /* max2 + 1 */, const u32 *__restrict__ table, const u64 *__restrict__ value, int B,
                                       u32 *__restrict__ target, u32 *__restrict__ miss) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // 64-bit: a set may hold up to 2^32 - 2 entries (B = 34)
  if (i >= n1) return;
  u32 ix = 0;
  if (i) ix = probe_find(table, value, B, v2[i]);
  target[i] = ix; miss[i] = (i && !ix) ? 1u : 0u;
}
__global__ void mosh_merge_new_kernel(const u64 *__restrict__ v2, u32 n1, const u32 *__restrict__ miss, const u32 *__restrict__ before, u32 first,
                                      u32 *__restrict__ target, u64 *__restrict__ value, u16 *__restrict__ depth, u8 *__restrict__ info) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // 64-bit: a set may hold up to 2^32 - 2 entries (B = 34)
  if (i >= n1 || !miss[i]) return;
  const u32 ix = first + before[i];
  target[i] = ix; value[ix] = v2[i]; depth[ix] = 0; info[ix] = 0;
}
__global__ void mosh_merge_apply_kernel(const u16 *__restrict__ d2, const u8 *__restrict__ i2, u32 n1, const u32 *__restrict__ target,
                                        u16 *__restrict__ depth, u8 *__restrict__ info) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // 64-bit: a set may hold up to 2^32 - 2 entries (B = 34)
  if (i == 0 || i >= n1) return;
  const u32 ix = target[i];                                  // distinct values of the other set -> distinct indices: no two lanes share one
  const u32 d = (u32)depth[ix] + (u32)d2[i];
  depth[ix] = (u16)(d > 65535u ? 65535u : d);
  u32 cc = (u32)(info[ix] & 3) + (u32)(i2[i] & 3); if (cc > 3) cc = 3;
  info[ix] = (u8)((info[ix] & 3) | cc);                      // moshset.c:117: the old copy bits stay and the sum is OR-ed in
}

// moshsetDepthPrune (moshset.c:63-76)
__global__ void mosh_keep_kernel(const u16 *__restrict__ depth, u32 n1, int mn, int mx, u32 *__restrict__ keep) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // 64-bit: a set may hold up to 2^32 - 2 entries (B = 34)
  if (i >= n1) return;
  const int d = depth[i];
  keep[i] = (i && d >= mn && (!mx || d < mx)) ? 1u : 0u;
}
__global__ void mosh_compact_kernel(const u32 *__restrict__ keep, const u32 *__restrict__ before, u32 n1,
                                    const u64 *__restrict__ v, const u16 *__restrict__ d, const u8 *__restrict__ f,
                                    u64 *__restrict__ vo, u16 *__restrict__ dn, u8 *__restrict__ fo) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // 64-bit: a set may hold up to 2^32 - 2 entries (B = 34)
  if (i >= n1 || !keep[i]) return;
  const u32 o = 1 + before[i];
  vo[o] = v[i]; dn[o] = d[i]; fo[o] = f[i];
}
// -s (moshutils.c:170-178) / -sM (moshutils.c:181-184)
__global__ void mosh_setcopy_kernel(const u16 *__restrict__ depth, u8 *__restrict__ info, u32 n1, int c1, int c2, int cM, int onlyM) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // 64-bit: a set may hold up to 2^32 - 2 entries (B = 34)
  if (i == 0 || i >= n1) return;
  const int d = depth[i]; u8 f = info[i];
  if (onlyM) { if (d >= cM) f |= 3; }
  else if (d < c1) f &= 0xfc;
  else if (d < c2) f = (u8)((f & 0xfc) | 1);
  else if (d < cM) f = (u8)((f & 0xfc) | 2);
  else f |= 3;
  info[i] = f;
}
// depth histogram (65536 bins) + the four copy counts: the lanes of a wave that hold the same depth post ONE add
__global__ __launch_bounds__(256)
void mosh_summary_kernel(const u16 *__restrict__ depth, const u8 *__restrict__ info, u32 n1, u32 *__restrict__ hist, u32 *__restrict__ copy) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // 64-bit: a set may hold up to 2^32 - 2 entries (B = 34)
  const int lane = threadIdx.x & (WAVE - 1);
  const bool on = i > 0 && i < n1;
  const u32 d = on ? depth[i] : 0, cc = on ? (info[i] & 3) : 0;
  u64 todo = __ballot(on);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const u32 d0 = __shfl(d, leader);
    const u64 same = __ballot(on && d == d0) & todo;
    if (lane == leader) atomicAdd(&hist[d0], (u32)__popcll(same));
    todo &= ~same;
  }
  for (u32 q = 0; q < 4; ++q) {
    const u64 m = __ballot(on && cc == q);
    if (m && lane == __ffsll((long long)m) - 1) atomicAdd(&copy[q], (u32)__popcll(m));
  }
}
__global__ void mosh_lookup_kernel(const u64 *__restrict__ q, u64 n, const u32 *__restrict__ table, const u64 *__restrict__ value, const u16 *__restrict__ depth, int B,
                                   u32 *__restrict__ index, u16 *__restrict__ dout) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u32 ix = probe_find(table, value, B, q[i]);
  index[i] = ix; dout[i] = ix ? depth[ix] : (u16)0;
}
__global__ void mosh_gather_kernel(const u32 *__restrict__ pos, const u64 *__restrict__ in, u64 n, u64 *__restrict__ out) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[pos[i]];
}
__global__ void mosh_iota_kernel(u32 *__restrict__ v, u64 n) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (u32)i;
}

// ------------------------------------------------------------------------------------------------ drivers
int moshAllocSet(Mosh *m, u32 size) {
  Ctx *c = &m->c; hipStream_t st = c->stream;
  const u64 T = (u64)1 << m->B;
  const u64 bytes = T * 4 + (u64)size * (8 + 2 + 1 + 4);
  hipError_t e = c->hashIndex.alloc(T);
  if (e == hipSuccess) e = c->hashValue.alloc(size);
  if (e == hipSuccess) e = m->depth.alloc(size);
  if (e == hipSuccess) e = m->info.alloc(size);
  if (e == hipSuccess) e = m->acc.alloc(size);
  if (e != hipSuccess) { (void)hipGetLastError(); return c->fail("mosh set with %d table bits does not fit the device: %llu bytes asked for", m->B, bytes); }
  m->size = size;
  H10X_HIP(c, hipMemsetAsync(c->hashIndex.p, 0, T * 4, st));
  H10X_HIP(c, hipMemsetAsync(c->hashValue.p, 0, (size_t)size * 8, st));     // value[0] is uninitialised heap in the reference: 0 here
  H10X_HIP(c, hipMemsetAsync(m->depth.p, 0, (size_t)size * 2, st));
  H10X_HIP(c, hipMemsetAsync(m->info.p, 0, (size_t)size, st));
  H10X_HIP(c, hipMemsetAsync(m->acc.p, 0, (size_t)size * 4, st));
  return 0;
}

__attribute__((format(printf, 3, 4))) static int moshBad(char *err, int errlen, const char *fmt, ...) {
  if (err && errlen > 0) { va_list ap; va_start(ap, fmt); vsnprintf(err, (size_t)errlen, fmt, ap); va_end(ap); }
  return -1;
}
#define bad(...) moshBad(err, errlen, __VA_ARGS__)
int moshOpen(Mosh **out, int B, int k, int w, u64 factor1, u64 factor2, int device, char *err, int errlen) {
  *out = nullptr;
  if (k < 1 || k >= 32) return bad("seqhash k %d must be between 1 and 32\n", k);            // seqhash.c:24-25
  if (w < 1) return bad("seqhash w %d must be positive\n", w);
  if (B < 20 || B > 34) return bad("table bits %d must be between 20 and 34", B);           // moshset.c:17
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return bad("no HIP device available: libh10x_hip has no CPU fallback");
  if (device < 0 || device >= n) return bad("HIP device %d out of range 0..%d", device, n - 1);
  if (hipSetDevice(device) != hipSuccess) return bad("hipSetDevice(%d) failed", device);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return bad("hipGetDeviceProperties failed");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return bad("device %d is %s: this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
  Mosh *m = new (std::nothrow) Mosh();
  if (!m) return bad("out of host memory");
  m->B = B; m->k = k; m->w = w; m->factor1 = factor1; m->factor2 = factor2;
  m->c.device = device; m->c.numCU = prop.multiProcessorCount;
  m->c.prm.k = k; m->c.prm.w = w; m->c.prm.B = B; m->c.prm.factor1 = factor1;
  if (hipStreamCreateWithFlags(&m->c.stream, hipStreamNonBlocking) != hipSuccess) { delete m; return bad("hipStreamCreate failed"); }
  m->c.ownStream = true;
  *out = m;
  return 0;
}
#undef bad

void stageG_destroy(Mosh *m) {
  if (!m) return;
  (void)moshEnter(m);
  (void)hipStreamSynchronize(m->c.stream);
  if (m->c.mail) (void)hipHostFree(m->c.mail);
  const hipStream_t used = m->c.stream; const int dev = m->c.device;
  delete m;
  DevCache::retireStream(dev, used);
  (void)hipStreamDestroy(used);
}
const char *stageG_error(const Mosh *m) { return m ? m->c.err.c_str() : "null mosh set"; }

int stageG_create(Mosh **out, int B, int k, int w, u64 factor1, u64 factor2, int device, char *err, int errlen) {
  H10X_TRY(moshOpen(out, B, k, w, factor1, factor2, device, err, errlen));
  Mosh *m = *out;
  int rc = moshEnter(m);
  if (!rc) rc = moshAllocSet(m, (u32)((((u64)1 << B) >> 2) - 1));                            // moshset.c:26
  if (!rc && hipStreamSynchronize(m->c.stream) != hipSuccess) rc = m->c.fail("hipStreamSynchronize failed");
  if (rc) { if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", m->c.err.c_str()); stageG_destroy(m); *out = nullptr; }
  return rc;
}

// moshsetRead's state (moshset.c:89-103): the arrays are sized to the file's max + 1, so the set is FULL
int stageG_load(Mosh **out, int B, int k, int w, u64 factor1, u64 factor2, const u32 *index, const u64 *value, const u16 *depth, const u8 *info, u32 size,
                int device, char *err, int errlen) {
  *out = nullptr;
  if (size < 1 || (u64)size >= (((u64)1 << (B < 20 || B > 34 ? 20 : B)) >> 2)) { if (err && errlen > 0) snprintf(err, (size_t)errlen, "Moshset size %u is too big for %d bits", size, B); return -1; }   // moshset.c:24
  H10X_TRY(moshOpen(out, B, k, w, factor1, factor2, device, err, errlen));
  Mosh *m = *out; Ctx *c = &m->c; hipStream_t st = c->stream;
  auto body = [&]() -> int {
    H10X_TRY(moshEnter(m));
    H10X_TRY(moshAllocSet(m, size));
    H10X_HIP(c, hipMemcpyAsync(c->hashIndex.p, index, ((size_t)1 << B) * 4, hipMemcpyHostToDevice, st));
    H10X_HIP(c, hipMemcpyAsync(c->hashValue.p, value, (size_t)size * 8, hipMemcpyHostToDevice, st));
    H10X_HIP(c, hipMemcpyAsync(m->depth.p, depth, (size_t)size * 2, hipMemcpyHostToDevice, st));
    H10X_HIP(c, hipMemcpyAsync(m->info.p, info, (size_t)size, hipMemcpyHostToDevice, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    m->max = size - 1;
    return 0;
  };
  const int rc = body();
  if (rc) { if (err && errlen > 0) snprintf(err, (size_t)errlen, "%s", c->err.c_str()); stageG_destroy(m); *out = nullptr; }
  return rc;
}

int stageG_setOption(Mosh *m, const char *name, int64_t v) {
  if (!strcmp(name, "mosh_slab")) { m->slab = v > 0 ? (u64)v : MOSH_SLAB_DEFAULT; return 0; }
  if (!strcmp(name, "overlap_chunk")) { m->overlapChunk = v > 0 ? (u64)v : RS_CHUNK_ENTRIES_DEFAULT; return 0; }
  if (!strcmp(name, "overlap_chunk_reads")) {                // the 16-bit xl field of rs_order_kernel (stage_h.hip) holds a read's place in its chunk
    if (v > (int64_t)RS_CHUNK_READS_MAX) return -1;
    m->overlapChunkReads = v > 0 ? (u32)v : RS_CHUNK_READS_MAX;
    return 0;
  }
  return -1;
}
void stageG_counters(const Mosh *m, h10x_mosh_counters_t *out) { memset(out, 0, sizeof *out); out->scan_retries = m->c.scanRetries; }

// new indices [first, first + D) have their value[]: the die of moshset.c:57, then the table
int moshPlace(Mosh *m, u32 D) {
  Ctx *c = &m->c;
  if (!D) return 0;
  if ((u64)m->max + D >= (u64)m->size) return c->fail("hashTableSize %u is too small for %u", m->size, m->size);
  mosh_insert_kernel<<<hmin<u32>(divUp(D, 256), 16384), 256, 0, c->stream>>>(c->hashValue.p, m->max + 1, D, m->B, c->hashIndex.p);
  H10X_HIP(c, hipGetLastError());
  m->max += D;
  return 0;
}

// upload a batch and run the scan; the list is sized by an estimate and the scan repeated with the exact size if it was too small
// (the hasher and the table are arguments: stage_p.hip scans with a context's hasher and no set; acc = null lists every mosh)
int moshScanWith(Ctx *c, int k, int w, u64 factor1, int B, u32 *acc, u32 accSize, MoshBatch &b, const u8 *codes, const u64 *seqStart, u32 nSeq, int skipOdd,
                 u64 seqBase) {
  hipStream_t st = c->stream; const bool add = acc != nullptr;
  const SeqPlan plan(seqStart, nSeq, k, SeqSkip{skipOdd, seqBase}); StreamWait wait{st};
  if (plan.tooShort < nSeq) return c->fail("10x sequence %llu has %llu bases: the first read of a pair needs at least %d", seqBase + plan.tooShort + 1, plan.len(plan.tooShort), MOSH_X_SKIP);
  b.total = plan.total; b.nRuns = plan.nRuns; b.listed = b.found = 0;
  if (b.total > 0xFFFFFFFFull) return c->fail("a batch of %llu bases: at most 2^32 - 1 are supported per call", b.total);
  if (!b.nRuns) return 0;
  H10X_TRY(b.upload(c, plan, codes + seqStart[0])); H10X_HIP(c, b.tallies.alloc(2));
  const unsigned grid = (unsigned)hmin<u64>(divUp(b.nRuns, 256), (u64)c->numCU * 16);
  u64 ht[2] = {0, 0};
  const int rc = seqScanTwice(c, plan.cap(w), b.tallies.p, ht, 2, "mosh scan: the list overflowed twice", [&](u64 cap) -> int {
    H10X_HIP(c, b.outHash.alloc(cap)); H10X_HIP(c, b.outOrd.alloc(cap));
    H10X_HIP(c, hipMemsetAsync(b.tallies.p, 0, 16, st));
    if (add) mosh_scan_kernel<1><<<grid, 256, 0, st>>>(b.codes.p, b.seq.p, b.run.p, nSeq, skipOdd, seqBase, k, w, factor1, c->hashIndex.p, c->hashValue.p, B,
                                                       acc, b.outHash.p, b.outOrd.p, cap, b.tallies.p);
    else mosh_scan_kernel<0><<<grid, 256, 0, st>>>(b.codes.p, b.seq.p, b.run.p, nSeq, skipOdd, seqBase, k, w, factor1, nullptr, nullptr, B,
                                                   nullptr, b.outHash.p, b.outOrd.p, cap, b.tallies.p);
    return 0;
  }, [&]() -> int { if (add) H10X_HIP(c, hipMemsetAsync(acc, 0, (size_t)accSize * 4, st)); return 0; });   // (acc[] is all zero between batches)
  b.listed = ht[0]; b.found = ht[1];
  return rc;
}

static int moshScanBatch(Mosh *m, MoshBatch &b, const u8 *codes, const u64 *seqStart, u32 nSeq, int skipOdd, u64 seqBase, bool add) {
  return moshScanWith(&m->c, m->k, m->w, m->factor1, m->B, add ? m->acc.p : nullptr, m->size, b, codes, seqStart, nSeq, skipOdd, seqBase);
}

int moshFold(Mosh *m) {                                      // depth[] takes what the scans counted in acc[], which is all zero again
  mosh_fold_kernel<<<divUp((u64)m->max + 1, 256), 256, 0, m->c.stream>>>(m->depth.p, m->acc.p, m->max + 1);
  H10X_HIP(&m->c, hipGetLastError()); return 0;
}

// addSequence over a batch of whole sequences (moshutils.c:19-30, 41-45)
static int moshAddBatch(Mosh *m, const u8 *codes, const u64 *seqStart, u32 nSeq, int skipOdd, u64 seqBase, u64 *nHashes) {
  Ctx *c = &m->c; hipStream_t st = c->stream; PrimTemp pt; MoshBatch b;
  H10X_TRY(moshScanBatch(m, b, codes, seqStart, nSeq, skipOdd, seqBase, true));
  *nHashes += b.listed + b.found;
  const u64 n = b.listed;
  u32 D = 0;
  if (n) {
    if (n > 0xFFFFFFFFull) return c->fail("mosh add: %llu new occurrences in one batch", n);
    DevBuf<u64> sh, runHash; DevBuf<u32> so, flag, before, runFirst, runMin, rankKey, rankRun, iota;
    H10X_HIP(c, sh.alloc(n)); H10X_HIP(c, so.alloc(n)); H10X_HIP(c, flag.alloc(n)); H10X_HIP(c, before.alloc(n));
    H10X_TRY(prim_sort_pairs_u64_u32(c, pt, b.outHash.p, sh.p, b.outOrd.p, so.p, n, 0, 2 * m->k));
    mosh_heads_kernel<<<divUp(n, 256), 256, 0, st>>>(sh.p, n, flag.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, before.p, n));
    u32 tail[2];
    H10X_HIP(c, hipMemcpyAsync(&tail[0], before.p + (n - 1), 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipMemcpyAsync(&tail[1], flag.p + (n - 1), 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    D = tail[0] + tail[1];
    if ((u64)m->max + D >= (u64)m->size) return c->fail("hashTableSize %u is too small for %u", m->size, m->size);
    H10X_HIP(c, runHash.alloc(D)); H10X_HIP(c, runFirst.alloc(D)); H10X_HIP(c, runMin.alloc(D)); H10X_HIP(c, rankKey.alloc(D)); H10X_HIP(c, rankRun.alloc(D)); H10X_HIP(c, iota.alloc(D));
    H10X_HIP(c, hipMemsetAsync(runMin.p, 0xFF, (size_t)D * 4, st));
    mosh_runs_kernel<<<divUp(n, 256), 256, 0, st>>>(sh.p, so.p, flag.p, before.p, n, runHash.p, runFirst.p, runMin.p);
    H10X_HIP(c, hipGetLastError());
    mosh_iota_kernel<<<divUp(D, 256), 256, 0, st>>>(iota.p, D);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(prim_sort_pairs_u32_u32(c, pt, runMin.p, rankKey.p, iota.p, rankRun.p, D, 0, 32));
    mosh_assign_kernel<<<divUp(D, 256), 256, 0, st>>>(rankRun.p, D, n, runHash.p, runFirst.p, m->max + 1, c->hashValue.p, m->depth.p, m->info.p, m->acc.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(moshPlace(m, D));
  }
  if (b.nRuns) H10X_TRY(moshFold(m));
  H10X_HIP(c, hipStreamSynchronize(st));                    // temporaries of this batch go back to the block cache behind finished work
  return 0;
}

int stageG_add(Mosh *m, const u8 *codes, const u64 *seqStart, u32 nSeq, int skipOdd, u64 seqBase, u64 *nHashes) {
  H10X_TRY(moshEnter(m));
  if (nSeq && (!codes || !seqStart)) return m->c.fail("h10x_mosh_add: null argument");
  u64 total = 0;
  const int rc = moshBatches(m, seqStart, nSeq, [&](u32 s, u32 n) { return moshAddBatch(m, codes, seqStart + s, n, skipOdd, seqBase + s, &total); });
  if (rc) {                                                  // leave a usable object: no half-counted batch
    (void)hipStreamSynchronize(m->c.stream);
    (void)hipMemsetAsync(m->acc.p, 0, (size_t)m->size * 4, m->c.stream);
    (void)hipStreamSynchronize(m->c.stream);
  }
  if (nHashes) *nHashes = total;
  return rc;
}

int moshIota(Mosh *m, u32 *v, u64 n) {                       // v[i] = i
  if (!n) return 0;
  mosh_iota_kernel<<<divUp(n, 256), 256, 0, m->c.stream>>>(v, n);
  H10X_HIP(&m->c, hipGetLastError());
  return 0;
}

// every mosh of one batch in order, on the device: sh[i] = hash, so[i] = ordinal of its k-mer in the batch, i < b.listed; b.seq = the
// batch's sequence starts. What stageG_scan copies out, and what stage_i.hip looks up.
int moshScanOrdered(Mosh *m, MoshBatch &b, DevBuf<u64> &sh, DevBuf<u32> &so, const u8 *codes, const u64 *seqStart, u32 nSeq, int skipOdd, u64 seqBase) {
  Ctx *c = &m->c; hipStream_t st = c->stream; PrimTemp pt;
  H10X_TRY(moshScanBatch(m, b, codes, seqStart, nSeq, skipOdd, seqBase, false));
  const u64 n = b.listed;
  if (!n) return 0;
  if (n > 0xFFFFFFFFull) return c->fail("mosh scan: %llu moshes in one batch", n);
  DevBuf<u32> iota, sp;
  H10X_HIP(c, iota.alloc(n)); H10X_HIP(c, so.alloc(n)); H10X_HIP(c, sp.alloc(n)); H10X_HIP(c, sh.alloc(n));
  H10X_TRY(moshIota(m, iota.p, n));
  H10X_TRY(prim_sort_pairs_u32_u32(c, pt, b.outOrd.p, so.p, iota.p, sp.p, n, 0, 32));
  mosh_gather_kernel<<<divUp(n, 256), 256, 0, st>>>(sp.p, b.outHash.p, n, sh.p);
  H10X_HIP(c, hipGetLastError());
  H10X_HIP(c, hipStreamSynchronize(st));                     // the temporaries above go back to the block cache behind finished work
  return 0;
}

// every mosh of the sequences in order: (hash, sequence, position of the k-mer in the sequence as moshRCnext reports it)
int stageG_scan(Mosh *m, const u8 *codes, const u64 *seqStart, u32 nSeq, int skipOdd, u64 seqBase, u64 *hash, u32 *seq, u32 *pos, u64 cap, u64 *nOut) {
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c; hipStream_t st = c->stream;
  if (nSeq && (!codes || !seqStart)) return c->fail("h10x_mosh_scan: null argument");
  u64 done = 0;
  const int rc = moshBatches(m, seqStart, nSeq, [&](u32 s0, u32 ns) -> int {
    MoshBatch b; DevBuf<u32> so; DevBuf<u64> sh;
    H10X_TRY(moshScanOrdered(m, b, sh, so, codes, seqStart + s0, ns, skipOdd, seqBase + s0));
    const u64 n = b.listed;
    if (!n) return 0;
    std::vector<u64> hh(n); std::vector<u32> oo(n);
    H10X_HIP(c, hipMemcpyAsync(hh.data(), sh.p, n * 8, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipMemcpyAsync(oo.data(), so.p, n * 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    const u64 base = seqStart[s0]; const SeqSkip skip{skipOdd, seqBase + s0};
    u32 s = 0;
    for (u64 i = 0; i < n; ++i, ++done) {
      const u64 o = base + oo[i];
      while (seqStart[s0 + s + 1] <= o) ++s;
      if (done >= cap) continue;
      if (hash) hash[done] = hh[i];
      if (seq) seq[done] = s0 + s;
      if (pos) pos[done] = (u32)(o - seqStart[s0 + s] - skip.of(s));
    }
    return 0;
  });
  if (nOut) *nOut = done;
  return rc;
}

int stageG_merge(Mosh *m, int k2, int w2, u64 factor12, const u64 *value2, const u16 *depth2, const u8 *info2, u32 size2, int *merged) {
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c; hipStream_t st = c->stream; PrimTemp pt;
  if (merged) *merged = 0;
  if (k2 != m->k || w2 != m->w || factor12 != m->factor1) return 0;           // moshset.c:110: the caller prints "incompatible"
  if (merged) *merged = 1;
  if (size2 <= 1) return 0;
  if (!value2 || !depth2 || !info2) return c->fail("h10x_mosh_merge: null argument");
  DevBuf<u64> v2; DevBuf<u16> d2; DevBuf<u8> i2; DevBuf<u32> target, miss, before;
  H10X_HIP(c, v2.alloc(size2)); H10X_HIP(c, d2.alloc(size2)); H10X_HIP(c, i2.alloc(size2));
  H10X_HIP(c, target.alloc(size2)); H10X_HIP(c, miss.alloc(size2)); H10X_HIP(c, before.alloc(size2));
  H10X_HIP(c, hipMemcpyAsync(v2.p, value2, (size_t)size2 * 8, hipMemcpyHostToDevice, st));
  H10X_HIP(c, hipMemcpyAsync(d2.p, depth2, (size_t)size2 * 2, hipMemcpyHostToDevice, st));
  H10X_HIP(c, hipMemcpyAsync(i2.p, info2, (size_t)size2, hipMemcpyHostToDevice, st));
  const unsigned g = divUp(size2, 256);
  mosh_merge_find_kernel<<<g, 256, 0, st>>>(v2.p, size2, c->hashIndex.p, c->hashValue.p, m->B, target.p, miss.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, miss.p, before.p, size2));
  u32 tail[2];
  H10X_HIP(c, hipMemcpyAsync(&tail[0], before.p + (size2 - 1), 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(&tail[1], miss.p + (size2 - 1), 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  const u32 D = tail[0] + tail[1];
  if (D) {
    if ((u64)m->max + D >= (u64)m->size) return c->fail("hashTableSize %u is too small for %u", m->size, m->size);
    mosh_merge_new_kernel<<<g, 256, 0, st>>>(v2.p, size2, miss.p, before.p, m->max + 1, target.p, c->hashValue.p, m->depth.p, m->info.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(moshPlace(m, D));
  }
  mosh_merge_apply_kernel<<<g, 256, 0, st>>>(d2.p, i2.p, size2, target.p, m->depth.p, m->info.p);
  H10X_HIP(c, hipGetLastError());
  H10X_HIP(c, hipStreamSynchronize(st));
  return 0;
}

int stageG_prune(Mosh *m, int mn, int mx, u32 *before_, u32 *after_) {
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c; hipStream_t st = c->stream; PrimTemp pt;
  const u32 n1 = m->max + 1;
  if (before_) *before_ = m->max;
  DevBuf<u32> keep, before; DevBuf<u64> vo; DevBuf<u16> dn; DevBuf<u8> fo;
  H10X_HIP(c, keep.alloc(n1)); H10X_HIP(c, before.alloc(n1));
  H10X_HIP(c, vo.alloc(m->size)); H10X_HIP(c, dn.alloc(m->size)); H10X_HIP(c, fo.alloc(m->size));
  H10X_HIP(c, hipMemsetAsync(vo.p, 0, (size_t)m->size * 8, st)); H10X_HIP(c, hipMemsetAsync(dn.p, 0, (size_t)m->size * 2, st)); H10X_HIP(c, hipMemsetAsync(fo.p, 0, (size_t)m->size, st));
  mosh_keep_kernel<<<divUp(n1, 256), 256, 0, st>>>(m->depth.p, n1, mn, mx, keep.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, keep.p, before.p, n1));
  u32 tail[2];
  H10X_HIP(c, hipMemcpyAsync(&tail[0], before.p + (n1 - 1), 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(&tail[1], keep.p + (n1 - 1), 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  const u32 M = tail[0] + tail[1];
  mosh_compact_kernel<<<divUp(n1, 256), 256, 0, st>>>(keep.p, before.p, n1, c->hashValue.p, m->depth.p, m->info.p, vo.p, dn.p, fo.p);
  H10X_HIP(c, hipGetLastError());
  c->hashValue.swap(vo); m->depth.swap(dn); m->info.swap(fo);
  H10X_HIP(c, hipMemsetAsync(c->hashIndex.p, 0, ((size_t)1 << m->B) * 4, st));
  m->max = 0;
  H10X_TRY(moshPlace(m, M));
  H10X_HIP(c, hipStreamSynchronize(st));
  if (after_) *after_ = m->max;
  return 0;
}

int stageG_setCopy(Mosh *m, int c1, int c2, int cM, int onlyM) {
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c;
  mosh_setcopy_kernel<<<divUp((u64)m->max + 1, 256), 256, 0, c->stream>>>(m->depth.p, m->info.p, m->max + 1, c1, c2, cM, onlyM);
  H10X_HIP(c, hipGetLastError());
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int stageG_summary(Mosh *m, u32 *hist65536, u32 *copy4) {
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c; hipStream_t st = c->stream;
  DevBuf<u32> d; H10X_HIP(c, d.alloc(65536 + 4));
  H10X_HIP(c, hipMemsetAsync(d.p, 0, (65536 + 4) * 4, st));
  mosh_summary_kernel<<<divUp((u64)m->max + 1, 256), 256, 0, st>>>(m->depth.p, m->info.p, m->max + 1, d.p, d.p + 65536);
  H10X_HIP(c, hipGetLastError());
  if (hist65536) H10X_HIP(c, hipMemcpyAsync(hist65536, d.p, 65536 * 4, hipMemcpyDeviceToHost, st));
  if (copy4) H10X_HIP(c, hipMemcpyAsync(copy4, d.p + 65536, 16, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  return 0;
}

void stageG_info(const Mosh *m, int *B, int *k, int *w, u64 *factor1, u64 *factor2, u32 *max, u32 *size) {
  if (B) *B = m->B; if (k) *k = m->k; if (w) *w = m->w; if (factor1) *factor1 = m->factor1; if (factor2) *factor2 = m->factor2;
  if (max) *max = m->max; if (size) *size = m->size;
}

int stageG_export(Mosh *m, u64 indexFirst, u64 indexCount, u32 *index, u64 *value, u16 *depth, u8 *info) {
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c; hipStream_t st = c->stream;
  const u64 T = (u64)1 << m->B; const size_t n1 = (size_t)m->max + 1;
  if (index && indexCount) {
    if (indexFirst > T || indexCount > T - indexFirst) return c->fail("h10x_mosh_export: index slice outside the table");
    H10X_HIP(c, hipMemcpyAsync(index, c->hashIndex.p + indexFirst, indexCount * 4, hipMemcpyDeviceToHost, st));
  }
  if (value) H10X_HIP(c, hipMemcpyAsync(value, c->hashValue.p, n1 * 8, hipMemcpyDeviceToHost, st));
  if (depth) H10X_HIP(c, hipMemcpyAsync(depth, m->depth.p, n1 * 2, hipMemcpyDeviceToHost, st));
  if (info) H10X_HIP(c, hipMemcpyAsync(info, m->info.p, n1, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  return 0;
}

int stageG_lookup(Mosh *m, const u64 *hashes, u64 n, u32 *index, u16 *depth) {
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c; hipStream_t st = c->stream;
  if (!n) return 0;
  if (!hashes) return c->fail("h10x_mosh_lookup: null argument");
  DevBuf<u64> q; DevBuf<u32> ix; DevBuf<u16> d;
  H10X_HIP(c, q.alloc(n)); H10X_HIP(c, ix.alloc(n)); H10X_HIP(c, d.alloc(n));
  H10X_HIP(c, hipMemcpyAsync(q.p, hashes, n * 8, hipMemcpyHostToDevice, st));
  mosh_lookup_kernel<<<divUp(n, 256), 256, 0, st>>>(q.p, n, c->hashIndex.p, c->hashValue.p, m->depth.p, m->B, ix.p, d.p);
  H10X_HIP(c, hipGetLastError());
  if (index) H10X_HIP(c, hipMemcpyAsync(index, ix.p, n * 4, hipMemcpyDeviceToHost, st));
  if (depth) H10X_HIP(c, hipMemcpyAsync(depth, d.p, n * 2, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  return 0;
}

}  // namespace h10x
