// stage_i.hip — reference maps: the Reference object behind moshmap (moshmap.c of the reference) over a mosh set of stage_g.hip.
//
// A reference map is, per mosh hit of the reference sequences in file order, (index, offset, id) = (set index, position of the k-mer,
// sequence number); per set index a 32-bit depth; and after packing loc[] (exclusive scan of depth) and rev[] (the hit ordinals of each
// index, ascending: a stable sort of the ordinals by index). The host keeps a copy of the six arrays (they are what -w stores and what
// the M lines and the verbose lines read); the device keeps id, rev and loc for the query pass.
//
// The query pass, per slab of whole queries:
//   scan     every mosh in order (moshScanOrdered of stage_g.hip)
//   seed     one lane per mosh: find-only look-up, copy class, loc / loc2 = its first two entries of rev, and their ids: the random
//            reads of the pass, all issued here
//   count    one wave per query: missed / copy 1 / copy 2 / multi, and the bound on its M records
//   block    one wave per query: the block automaton of queryProcess (moshmap.c:211-272) over the seeds that have an index and are
//            not copy M, staged 64 at a time through LDS; records go to a region reserved per query
//   compact  the regions to one list
// No float leaves the device: the host formats every figure from these integers.
#include "common.hpp"
#include "prim.hpp"
#include "mosh.hpp"
#include <memory>
#include <new>

namespace h10x {

constexpr u32 RM_CLASS_SHIFT = 30, RM_ID_MASK = (1u << RM_CLASS_SHIFT) - 1;
static_assert(sizeof(h10x_mapseed_t) == 16 && sizeof(h10x_maprec_t) == 28, "the records of include/h10x.h");

struct RefMap {
  Mosh *m = nullptr;
  u32 size = 0, max = 0;                                     // ref->size (the append that makes max + 1 reach it dies), ref->max
  bool packed = false, loaded = false;
  DevBuf<u32> dDepth, dIndex, dId, dRev, dLoc;               // dDepth (ms->size entries) and dIndex (every hit so far) while adding; the other three after packing
  std::vector<u32> index, offset, id, depth, rev, loc;       // the arrays of the .ref file
  // what the last query call found: per query four counts and its records; the seeds when asked for
  std::vector<u32> qCounts, seedPos; std::vector<u64> recStart, seedStart; std::vector<h10x_maprec_t> recs; std::vector<h10x_mapseed_t> seeds;
};

// ------------------------------------------------------------------------------------------------ kernels: build
// the -f loop behind the find-or-add (moshmap.c:106-115): every mosh of the batch is in the set by now
__global__ void rm_hit_kernel(const u64 *__restrict__ hash, const u32 *__restrict__ ord, u64 n, const u64 *__restrict__ seqStart, u32 nSeq, u32 idBase,
                              const u32 *__restrict__ table, const u64 *__restrict__ value, int B,
                              u32 *__restrict__ index, u32 *__restrict__ offset, u32 *__restrict__ id, u32 *__restrict__ depth, u32 *__restrict__ absent) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 o = ord[i];
  const u32 lo = last_le(seqStart, nSeq, o);                 // (an empty sequence never wins: the next one starts there too)
  const u32 ix = probe_find(table, value, B, hash[i]);
  index[i] = ix; offset[i] = (u32)(o - seqStart[lo]); id[i] = idBase + lo;
  if (ix) atomicAdd(&depth[ix], 1u); else *absent = 1;
}
// copy classes from the 32-bit depth (moshmap.c:124-128); counts[0..2] = copy 1, copy 2, multiple
__global__ __launch_bounds__(256)
void rm_class_kernel(const u32 *__restrict__ depth, u8 *__restrict__ info, u32 n1, u32 *__restrict__ counts) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & (WAVE - 1);
  const bool on = i > 0 && i < n1;
  u32 cc = 0;
  if (on) {
    const u32 d = depth[i];
    cc = d == 1 ? 1u : d == 2 ? 2u : 3u;
    info[i] = cc == 3 ? (u8)(info[i] | 3) : (u8)((info[i] & 0xfc) | cc);
  }
  for (u32 q = 1; q < 4; ++q) {
    const u64 mk = __ballot(on && cc == q);
    if (mk && lane == __ffsll((long long)mk) - 1) atomicAdd(&counts[q - 1], (u32)__popcll(mk));
  }
}
// what a loaded pair of files must satisfy: every index has a copy class, as after -f (class 0 would be counted in no figure of the Q line and
// walked as copy 2 by the reference), and the query pass stays inside rev[]: a copy-1 index has one entry, a copy-2 index two
__global__ void rm_classcheck_kernel(const u32 *__restrict__ depth, const u8 *__restrict__ info, u32 n1, u32 *__restrict__ bad) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 || i >= n1) return;
  const u32 cc = info[i] & 3, d = depth[i];
  if (cc == 0 || (cc == 1 && d < 1) || (cc == 2 && d < 2)) atomicMin(bad, (u32)i);
}
// the first index whose 16-bit depth is not 0 (a reference is built over a set as moshsetCreate leaves it)
__global__ void rm_depthzero_kernel(const u16 *__restrict__ depth, u32 n1, u32 *__restrict__ bad) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n1 && depth[i]) atomicMin(bad, (u32)i);
}

// ------------------------------------------------------------------------------------------------ kernels: query
__global__ void rm_seed_kernel(const u64 *__restrict__ hash, const u32 *__restrict__ ord, u64 n, const u64 *__restrict__ seqStart, u32 nSeq,
                               const u32 *__restrict__ table, const u64 *__restrict__ value, int B, const u8 *__restrict__ info,
                               const u32 *__restrict__ loc, const u32 *__restrict__ rev, const u32 *__restrict__ id,
                               h10x_mapseed_t *__restrict__ seeds, u32 *__restrict__ pos) {
  const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const u64 o = ord[i];
  const u32 lo = last_le(seqStart, nSeq, o);
  pos[i] = (u32)(o - seqStart[lo]);
  h10x_mapseed_t r = {0, 0, 0, 0};
  const u32 ix = probe_find(table, value, B, hash[i]);
  if (ix) {
    const u32 cc = info[ix] & 3;
    if (cc == 1 || cc == 2) {
      const u32 l = loc[ix];
      r.loc = rev[l]; r.idClass = id[r.loc] | (cc << RM_CLASS_SHIFT);
      if (cc == 2) { r.loc2 = rev[l + 1]; r.id2 = id[r.loc2]; }
    } else r.idClass = 3u << RM_CLASS_SHIFT;                 // copy M (class 0 is refused when a set is loaded, and -f leaves none)
  }
  ((uint4 *)seeds)[i] = make_uint4(r.loc, r.loc2, r.idClass, r.id2);
}
// seedStart[q] = the first seed at or after the start of query q (nSeq + 1 entries)
__global__ void rm_bounds_kernel(const u32 *__restrict__ ord, u32 n, const u64 *__restrict__ seqStart, u32 nSeq, u32 *__restrict__ seedStart) {
  const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > nSeq) return;
  const u64 s = seqStart[q];
  u32 lo = 0, hi = n;
  while (lo < hi) { const u32 mid = lo + (hi - lo) / 2; if ((u64)ord[mid] < s) lo = mid + 1; else hi = mid; }
  seedStart[q] = lo;
}
// one wave per query: counts[4 q ..] = missed, copy 1, copy 2, multi (the Q line, moshmap.c:198-209); bound[q] = the most M records it can
// emit: every record but the closing one needs n1 > 2, that is three qualifying seeds of its own
__global__ __launch_bounds__(WAVE)
void rm_count_kernel(const h10x_mapseed_t *__restrict__ seeds, const u32 *__restrict__ seedStart, u32 nSeq, u32 *__restrict__ counts, u32 *__restrict__ bound) {
  const u32 q = blockIdx.x; const int lane = threadIdx.x;
  if (q >= nSeq) return;
  const u32 s0 = seedStart[q], s1 = seedStart[q + 1];
  u32 c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (u32 i = s0 + lane; i < s1; i += WAVE) {
    const u32 ic = seeds[i].idClass, cc = ic >> RM_CLASS_SHIFT;
    c0 += ic == 0; c1 += cc == 1; c2 += cc == 2; c3 += cc == 3;
  }
  for (int o = 32; o; o >>= 1) { c0 += __shfl_down(c0, o); c1 += __shfl_down(c1, o); c2 += __shfl_down(c2, o); c3 += __shfl_down(c3, o); }
  if (lane == 0) { counts[4 * q] = c0; counts[4 * q + 1] = c1; counts[4 * q + 2] = c2; counts[4 * q + 3] = c3; bound[q] = (c1 + c2) / 3 + 1; }
  if (lane == 0 && q == 0) bound[nSeq] = 0;
}
// The block automaton of queryProcess (moshmap.c:211-272), one wave per query. A tile of 64 seed records is loaded with one coalesced read;
// the qualifying ones (an index, not copy M) are packed into LDS in order with their ordinal i among ALL seeds of the query; then every lane
// steps the same state machine over them (the LDS reads are broadcasts) and lane 0 writes the records. The state is the reference's:
// loc0 == 0 means "no open block" also when the block began on hit 0 of the reference; the arithmetic of d is 32-bit unsigned cast to int.
struct RmState { u32 loc0, locN, i0, iN, id0; int n1, n2; };
__device__ __forceinline__ bool rm_ends(const RmState &s, u32 loc, u32 idl) {
  if (idl != s.id0) return true;
  bool end = false;
  if (s.loc0 < s.locN) { if (loc < s.locN) end = true; const int d = (int)(s.locN - s.loc0 - s.iN + s.i0); if (d > 50 || d < -50) end = true; }
  else if (s.loc0 > s.locN) { if (loc > s.locN) end = true; const int d = (int)(s.loc0 - s.locN - s.iN + s.i0); if (d > 50 || d < -50) end = true; }
  return end;
}
__global__ __launch_bounds__(WAVE)
void rm_block_kernel(const h10x_mapseed_t *__restrict__ seeds, const u32 *__restrict__ pos, const u32 *__restrict__ seedStart, u32 nSeq, u32 queryBase,
                     const u32 *__restrict__ regStart, h10x_maprec_t *__restrict__ region, u32 *__restrict__ nRec) {
  __shared__ uint4 sRec[WAVE];
  __shared__ u32 sI[WAVE];
  const u32 q = blockIdx.x; const int lane = threadIdx.x;
  if (q >= nSeq) return;
  const u32 s0 = seedStart[q], s1 = seedStart[q + 1], r0 = regStart[q], room = regStart[q + 1] - r0;
  RmState s = {0, 0, 0, 0, 0, 0, 0};
  u32 nOut = 0;
  auto emit = [&]() {
    if (lane == 0 && nOut < room) {
      h10x_maprec_t r = {pos[s0 + s.i0], pos[s0 + s.iN], s.loc0, s.locN, (u32)s.n1, (u32)s.n2, queryBase + q};
      region[r0 + nOut] = r;
    }
    ++nOut;
  };
  for (u32 base = s0; base < s1; base += WAVE) {              // the same trip count in every lane: one block is one wave
    const u32 i = base + lane;
    uint4 r = make_uint4(0, 0, 0, 0); bool qual = false;
    if (i < s1) { r = ((const uint4 *)seeds)[i]; const u32 cc = r.z >> RM_CLASS_SHIFT; qual = cc == 1 || cc == 2; }
    const u64 mk = __ballot(qual);
    if (qual) { const int at = __popcll(mk & (((u64)1 << lane) - 1)); sRec[at] = r; sI[at] = i - s0; }
    __syncthreads();
    const int cnt = __popcll(mk);
    for (int j = 0; j < cnt; ++j) {
      const uint4 e = sRec[j]; const u32 ii = sI[j];
      const bool is1 = (e.z >> RM_CLASS_SHIFT) == 1;
      u32 loc = e.x, idl = e.z & RM_ID_MASK;
      bool end = !s.loc0 || rm_ends(s, loc, idl);
      if (end && s.loc0 && !is1) { loc = e.y; idl = e.w; end = rm_ends(s, loc, idl); }          // try the second loc (moshmap.c:240-252)
      if (end) {
        if (s.n1 > 2) emit();
        s.n1 = 0; s.n2 = 0; s.loc0 = loc; s.id0 = idl; s.i0 = ii;
      }
      if (is1) ++s.n1; else ++s.n2;
      s.locN = loc; s.iN = ii;
    }
    __syncthreads();
  }
  if (s.n2 > 2) emit();                                      // the closing flush tests n2 (moshmap.c:266)
  if (lane == 0) nRec[q] = nOut < room ? nOut : room;
}
__global__ __launch_bounds__(WAVE)
void rm_compact_kernel(const h10x_maprec_t *__restrict__ region, const u32 *__restrict__ regStart, const u32 *__restrict__ nRec, const u32 *__restrict__ recStart, u32 nSeq,
                       h10x_maprec_t *__restrict__ out) {
  const u32 q = blockIdx.x;
  if (q >= nSeq) return;
  for (u32 t = threadIdx.x; t < nRec[q]; t += WAVE) out[recStart[q] + t] = region[regStart[q] + t];
}

// ------------------------------------------------------------------------------------------------ drivers
// -f puts the set's 16-bit depth[] back to 0 after the find-or-add: that is only right for a set whose depths were 0
static int rmDepthsZero(Mosh *m) {
  Ctx *c = &m->c; hipStream_t st = c->stream;
  DevBuf<u32> bad; u32 b = 0;
  H10X_HIP(c, bad.alloc(1));
  H10X_HIP(c, hipMemsetAsync(bad.p, 0xFF, 4, st));
  rm_depthzero_kernel<<<divUp((u64)m->max + 1, 256), 256, 0, st>>>(m->depth.p, m->max + 1, bad.p);
  H10X_HIP(c, hipGetLastError());
  H10X_HIP(c, hipMemcpyAsync(&b, bad.p, 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  if (b != 0xFFFFFFFFu) return c->fail("mosh index %u has a depth: a reference is built over a set whose depths are all 0, as moshsetCreate leaves it", b);
  return 0;
}

int stageI_create(RefMap **out, Mosh *m, u32 size) {
  *out = nullptr;
  if (!m) return -1;
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c;
  if (!m->size) return c->fail("moshset must be initialised before reference");               // moshmap.c:50-51
  if (!size) return c->fail("refCreate must have size > 0");
  H10X_TRY(rmDepthsZero(m));
  std::unique_ptr<RefMap> rm(new (std::nothrow) RefMap());
  if (!rm) return c->fail("out of host memory");
  rm->m = m; rm->size = size;
  H10X_HIP(c, rm->dDepth.alloc(m->size));
  H10X_HIP(c, hipMemsetAsync(rm->dDepth.p, 0, (size_t)m->size * 4, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  *out = rm.release();
  return 0;
}
void stageI_destroy(RefMap *rm) {
  if (!rm) return;
  (void)moshEnter(rm->m);
  (void)hipStreamSynchronize(rm->m->c.stream);
  delete rm;
}
const char *stageI_error(const RefMap *rm) { return rm ? rm->m->c.err.c_str() : "null reference map"; }
Mosh *stageI_set(RefMap *rm) { return rm ? rm->m : nullptr; }
void stageI_info(const RefMap *rm, h10x_refmap_info_t *out) { out->size = rm->size; out->max = rm->max; out->setMax = rm->m->max; out->packed = rm->packed; }

static int rmAddBatch(RefMap *rm, const u8 *codes, const u64 *seqStart, u32 nSeq, u32 idBase) {
  Mosh *m = rm->m; Ctx *c = &m->c; hipStream_t st = c->stream;
  MoshBatch b; DevBuf<u64> sh; DevBuf<u32> so;
  H10X_TRY(moshScanOrdered(m, b, sh, so, codes, seqStart, nSeq, 0, 0));
  const u64 n = b.listed;
  if (!n) return 0;
  if ((u64)rm->max + n >= (u64)rm->size) return c->fail("reference size overflow");           // moshmap.c:109: the append that finds max + 1 >= size
  DevBuf<u32> dIx, dOff, dId, dAbsent;
  H10X_HIP(c, dIx.alloc(n)); H10X_HIP(c, dOff.alloc(n)); H10X_HIP(c, dId.alloc(n)); H10X_HIP(c, dAbsent.alloc(1));
  H10X_HIP(c, hipMemsetAsync(dAbsent.p, 0, 4, st));
  rm_hit_kernel<<<divUp(n, 256), 256, 0, st>>>(sh.p, so.p, n, b.seq.p, nSeq, idBase, c->hashIndex.p, c->hashValue.p, m->B, dIx.p, dOff.p, dId.p, rm->dDepth.p, dAbsent.p);
  H10X_HIP(c, hipGetLastError());
  const size_t at = rm->index.size();
  rm->index.resize(at + n); rm->offset.resize(at + n); rm->id.resize(at + n);
  u32 absent = 0;
  H10X_HIP(c, hipMemcpyAsync(rm->index.data() + at, dIx.p, n * 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(rm->offset.data() + at, dOff.p, n * 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(rm->id.data() + at, dId.p, n * 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(&absent, dAbsent.p, 4, hipMemcpyDeviceToHost, st));
  if ((size_t)rm->max + n > rm->dIndex.n) {                  // the index column stays on the device for the sort of the packing
    DevBuf<u32> grown;
    H10X_HIP(c, grown.alloc(hmax<size_t>((size_t)rm->max + n, 2 * rm->dIndex.n)));
    if (rm->max) H10X_HIP(c, hipMemcpyAsync(grown.p, rm->dIndex.p, (size_t)rm->max * 4, hipMemcpyDeviceToDevice, st));
    rm->dIndex.swap(grown);
    H10X_HIP(c, hipStreamSynchronize(st));                   // (the old block goes back to the cache behind the copy)
  }
  H10X_HIP(c, hipMemcpyAsync(rm->dIndex.p + rm->max, dIx.p, n * 4, hipMemcpyDeviceToDevice, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  if (absent) return c->fail("reference add: a mosh of the batch is not in the set after the find-or-add");
  rm->max += (u32)n;
  return 0;
}

int stageI_add(RefMap *rm, const u8 *codes, const u64 *seqStart, u32 nSeq, u32 idBase, u64 *nHits) {
  Mosh *m = rm->m;
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c;
  if (rm->packed || rm->loaded) return c->fail("h10x_refmap_add: the reference is packed");
  if (nSeq && (!codes || !seqStart)) return c->fail("h10x_refmap_add: null argument");
  if ((u64)idBase + nSeq > RM_ID_MASK) return c->fail("reference of 2^30 sequences or more is not supported");
  // moshsetIndexFind(.., TRUE) in file order: the exact first-appearance numbering and table of h10x_mosh_add. That loop also counts in the
  // set's 16-bit depth[], which the reference's moshmap never touches (moshmap.c:107-111): it is all 0 before (moshsetCreate) and is put back to 0
  u64 total = 0;
  H10X_TRY(rmDepthsZero(m));
  H10X_TRY(stageG_add(m, codes, seqStart, nSeq, 0, 0, &total));
  H10X_HIP(c, hipMemsetAsync(m->depth.p, 0, (size_t)m->size * 2, c->stream));
  const u32 before = rm->max;
  H10X_TRY(moshBatches(m, seqStart, nSeq, [&](u32 s, u32 n) { return rmAddBatch(rm, codes, seqStart + s, n, idBase + s); }));
  if (nHits) *nHits = rm->max - before;
  return 0;
}

// the device side of a loaded reference: id, rev, loc
static int rmUpload(RefMap *rm) {
  Mosh *m = rm->m; Ctx *c = &m->c; hipStream_t st = c->stream;
  const size_t n = rm->max, n1 = (size_t)m->max + 1;
  H10X_HIP(c, rm->dId.alloc(n ? n : 1)); H10X_HIP(c, rm->dRev.alloc(n ? n : 1)); H10X_HIP(c, rm->dLoc.alloc(n1));
  if (n) {
    H10X_HIP(c, hipMemcpyAsync(rm->dId.p, rm->id.data(), n * 4, hipMemcpyHostToDevice, st));
    H10X_HIP(c, hipMemcpyAsync(rm->dRev.p, rm->rev.data(), n * 4, hipMemcpyHostToDevice, st));
  }
  H10X_HIP(c, hipMemcpyAsync(rm->dLoc.p, rm->loc.data(), n1 * 4, hipMemcpyHostToDevice, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  return 0;
}

// the end of referenceFastaRead and referencePack (moshmap.c:73-90, 124-132)
int stageI_pack(RefMap *rm, u32 *n1out, u32 *n2out, u32 *nMout) {
  Mosh *m = rm->m;
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c; hipStream_t st = c->stream; PrimTemp pt;
  if (rm->packed || rm->loaded) return c->fail("h10x_refmap_pack: the reference is packed");
  const u32 n1 = m->max + 1, n = rm->max;
  DevBuf<u32> counts, dLoc, dIxS, iota, dRev;
  H10X_HIP(c, counts.alloc(3)); H10X_HIP(c, dLoc.alloc(n1));
  H10X_HIP(c, hipMemsetAsync(counts.p, 0, 12, st));
  rm_class_kernel<<<divUp(n1, 256), 256, 0, st>>>(rm->dDepth.p, m->info.p, n1, counts.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, rm->dDepth.p, dLoc.p, n1));                         // depth[0] = 0: loc[i] = depth[1] + .. + depth[i - 1]
  rm->depth.resize(n1); rm->loc.resize(n1); rm->rev.resize(n);
  u32 cnt[3];
  H10X_HIP(c, hipMemcpyAsync(cnt, counts.p, 12, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(rm->depth.data(), rm->dDepth.p, (size_t)n1 * 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(rm->loc.data(), dLoc.p, (size_t)n1 * 4, hipMemcpyDeviceToHost, st));
  if (n) {                                                   // rev: the hit ordinals sorted by index, stable: ascending within an index
    H10X_HIP(c, dIxS.alloc(n)); H10X_HIP(c, iota.alloc(n)); H10X_HIP(c, dRev.alloc(n));
    H10X_TRY(moshIota(m, iota.p, n));
    H10X_TRY(prim_sort_pairs_u32_u32(c, pt, rm->dIndex.p, dIxS.p, iota.p, dRev.p, n, 0, 32));
    H10X_HIP(c, hipMemcpyAsync(rm->rev.data(), dRev.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
  }
  H10X_HIP(c, hipStreamSynchronize(st));
  if (n1out) *n1out = cnt[0]; if (n2out) *n2out = cnt[1]; if (nMout) *nMout = cnt[2];
  rm->size = rm->max;                                        // moshmap.c:79
  rm->dDepth.release(); rm->dIndex.release();
  rm->dLoc.swap(dLoc); rm->dRev.swap(dRev);                  // loc and rev stay where they were made; id comes from the host copy
  H10X_HIP(c, rm->dId.alloc(n ? n : 1));
  if (!n) H10X_HIP(c, rm->dRev.alloc(1));
  if (n) H10X_HIP(c, hipMemcpyAsync(rm->dId.p, rm->id.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  rm->packed = true;
  return 0;
}

// referenceRead's state (moshmap.c:157-181) from the arrays of a parsed RFMSHv1 file (host/map_host.c has checked them against each other)
int stageI_load(RefMap **out, Mosh *m, const u32 *index, const u32 *offset, const u32 *id, const u32 *depth, const u32 *rev, const u32 *loc, u32 max, u32 nIds) {
  *out = nullptr;
  if (!m) return -1;
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c; hipStream_t st = c->stream;
  if (!depth || !loc || (max && (!index || !offset || !id || !rev))) return c->fail("h10x_refmap_load: null argument");
  if (nIds > RM_ID_MASK) return c->fail("reference of 2^30 sequences or more is not supported");
  const u32 n1 = m->max + 1;
  u32 run = 0;
  for (u32 i = 0; i < n1; ++i) {                             // the checks the device's reads rest on, whoever parsed the file
    if (loc[i] != run) return c->fail("reference loc[%u] is %u, the depths before it sum to %u", i, loc[i], run);
    if (depth[i] > max - run) return c->fail("reference depths sum to more than its %u hits", max);
    if (i) run += depth[i];
  }
  for (u32 i = 0; i < max; ++i) {
    if (index[i] > m->max) return c->fail("reference hit %u holds mosh index %u beyond %u", i, index[i], m->max);
    if (id[i] >= nIds) return c->fail("reference hit %u is on sequence %u of %u", i, id[i], nIds);
    if (rev[i] >= max) return c->fail("reference rev[%u] is %u beyond its %u hits", i, rev[i], max);
  }
  std::unique_ptr<RefMap> rm(new (std::nothrow) RefMap());
  if (!rm) return c->fail("out of host memory");
  rm->m = m; rm->size = rm->max = max; rm->loaded = rm->packed = true;
  rm->index.assign(index, index + max); rm->offset.assign(offset, offset + max); rm->id.assign(id, id + max);
  rm->depth.assign(depth, depth + n1); rm->rev.assign(rev, rev + max); rm->loc.assign(loc, loc + n1);
  DevBuf<u32> dDepth, bad;
  H10X_HIP(c, dDepth.alloc(n1)); H10X_HIP(c, bad.alloc(1));
  H10X_HIP(c, hipMemcpyAsync(dDepth.p, depth, (size_t)n1 * 4, hipMemcpyHostToDevice, st));
  H10X_HIP(c, hipMemsetAsync(bad.p, 0xFF, 4, st));
  rm_classcheck_kernel<<<divUp(n1, 256), 256, 0, st>>>(dDepth.p, m->info.p, n1, bad.p);
  H10X_HIP(c, hipGetLastError());
  u32 b = 0;
  H10X_HIP(c, hipMemcpyAsync(&b, bad.p, 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  if (b != 0xFFFFFFFFu) return c->fail("mosh index %u: its copy class in the set is 0 or asks for more hits than the reference holds for it", b);
  H10X_TRY(rmUpload(rm.get()));
  *out = rm.release();
  return 0;
}

int stageI_export(RefMap *rm, const u32 **index, const u32 **offset, const u32 **id, const u32 **depth, const u32 **rev, const u32 **loc) {
  if (!rm->packed) return rm->m->c.fail("h10x_refmap_export: the reference is not packed");
  if (index) *index = rm->index.data(); if (offset) *offset = rm->offset.data(); if (id) *id = rm->id.data();
  if (depth) *depth = rm->depth.data(); if (rev) *rev = rm->rev.data(); if (loc) *loc = rm->loc.data();
  return 0;
}

static int rmQueryBatch(RefMap *rm, const u8 *codes, const u64 *seqStart, u32 nSeq, u32 queryBase, bool wantSeeds) {
  Mosh *m = rm->m; Ctx *c = &m->c; hipStream_t st = c->stream; PrimTemp pt;
  MoshBatch b; DevBuf<u64> sh; DevBuf<u32> so;
  H10X_TRY(moshScanOrdered(m, b, sh, so, codes, seqStart, nSeq, 0, 0));
  const u64 n = b.listed;
  const size_t q0 = rm->recStart.size() - 1;
  rm->qCounts.resize((q0 + nSeq) * 4, 0); rm->recStart.resize(q0 + nSeq + 1, rm->recStart.back());
  if (wantSeeds) rm->seedStart.resize(q0 + nSeq + 1, rm->seedStart.back());
  if (!n) return 0;                                          // no seed anywhere: every count 0, no record
  DevBuf<h10x_mapseed_t> dSeeds; DevBuf<h10x_maprec_t> region, dRecs; DevBuf<u32> dPos, dStart, dCounts, dBound, dReg, dNRec, dRecStart;
  H10X_HIP(c, dSeeds.alloc(n)); H10X_HIP(c, dPos.alloc(n)); H10X_HIP(c, dStart.alloc((size_t)nSeq + 1)); H10X_HIP(c, dCounts.alloc((size_t)nSeq * 4));
  H10X_HIP(c, dBound.alloc((size_t)nSeq + 1)); H10X_HIP(c, dReg.alloc((size_t)nSeq + 1)); H10X_HIP(c, dNRec.alloc((size_t)nSeq + 1)); H10X_HIP(c, dRecStart.alloc((size_t)nSeq + 1));
  rm_seed_kernel<<<divUp(n, 256), 256, 0, st>>>(sh.p, so.p, n, b.seq.p, nSeq, c->hashIndex.p, c->hashValue.p, m->B, m->info.p, rm->dLoc.p, rm->dRev.p, rm->dId.p, dSeeds.p, dPos.p);
  H10X_HIP(c, hipGetLastError());
  rm_bounds_kernel<<<divUp((u64)nSeq + 1, 256), 256, 0, st>>>(so.p, (u32)n, b.seq.p, nSeq, dStart.p);
  H10X_HIP(c, hipGetLastError());
  rm_count_kernel<<<nSeq, WAVE, 0, st>>>(dSeeds.p, dStart.p, nSeq, dCounts.p, dBound.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, dBound.p, dReg.p, (size_t)nSeq + 1));
  u32 roomTotal = 0;
  H10X_HIP(c, hipMemcpyAsync(&roomTotal, dReg.p + nSeq, 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  H10X_HIP(c, region.alloc(roomTotal));
  H10X_HIP(c, hipMemsetAsync(dNRec.p, 0, ((size_t)nSeq + 1) * 4, st));
  rm_block_kernel<<<nSeq, WAVE, 0, st>>>(dSeeds.p, dPos.p, dStart.p, nSeq, queryBase, dReg.p, region.p, dNRec.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, dNRec.p, dRecStart.p, (size_t)nSeq + 1));
  std::vector<u32> recStart((size_t)nSeq + 1), seedStart;
  H10X_HIP(c, hipMemcpyAsync(recStart.data(), dRecStart.p, ((size_t)nSeq + 1) * 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(rm->qCounts.data() + q0 * 4, dCounts.p, (size_t)nSeq * 16, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  const u32 nRecs = recStart[nSeq];
  const size_t r0 = rm->recs.size();
  if (nRecs) {
    H10X_HIP(c, dRecs.alloc(nRecs));
    rm_compact_kernel<<<nSeq, WAVE, 0, st>>>(region.p, dReg.p, dNRec.p, dRecStart.p, nSeq, dRecs.p);
    H10X_HIP(c, hipGetLastError());
    rm->recs.resize(r0 + nRecs);
    H10X_HIP(c, hipMemcpyAsync(rm->recs.data() + r0, dRecs.p, (size_t)nRecs * sizeof(h10x_maprec_t), hipMemcpyDeviceToHost, st));
  }
  if (wantSeeds) {
    const size_t p0 = rm->seeds.size();
    rm->seeds.resize(p0 + n); rm->seedPos.resize(p0 + n); seedStart.resize((size_t)nSeq + 1);
    H10X_HIP(c, hipMemcpyAsync(rm->seeds.data() + p0, dSeeds.p, n * sizeof(h10x_mapseed_t), hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipMemcpyAsync(rm->seedPos.data() + p0, dPos.p, n * 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipMemcpyAsync(seedStart.data(), dStart.p, ((size_t)nSeq + 1) * 4, hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    for (u32 q = 0; q <= nSeq; ++q) rm->seedStart[q0 + q] = p0 + seedStart[q];
  }
  H10X_HIP(c, hipStreamSynchronize(st));
  for (u32 q = 0; q <= nSeq; ++q) rm->recStart[q0 + q] = r0 + recStart[q];
  return 0;
}

// queryProcess (moshmap.c:187-278) over sequences as for h10x_mosh_add; the results stay in the object until the next call
int stageI_query(RefMap *rm, const u8 *codes, const u64 *seqStart, u32 nSeq, int wantSeeds) {
  Mosh *m = rm->m;
  H10X_TRY(moshEnter(m));
  Ctx *c = &m->c;
  if (!rm->packed) return c->fail("h10x_refmap_query: the reference is not packed");
  if (nSeq && (!codes || !seqStart)) return c->fail("h10x_refmap_query: null argument");
  rm->qCounts.clear(); rm->recs.clear(); rm->seeds.clear(); rm->seedPos.clear();
  rm->recStart.assign(1, 0); rm->seedStart.assign(1, 0);
  return moshBatches(m, seqStart, nSeq, [&](u32 s, u32 n) { return rmQueryBatch(rm, codes, seqStart + s, n, s, wantSeeds != 0); });
}
int stageI_results(RefMap *rm, u32 *nQueries, const u32 **counts4, const u64 **recStart, const h10x_maprec_t **recs, const u64 **seedStart,
                   const h10x_mapseed_t **seeds, const u32 **seedPos) {
  if (rm->recStart.empty()) return rm->m->c.fail("h10x_refmap_results: no query has run");
  if (nQueries) *nQueries = (u32)(rm->recStart.size() - 1);
  if (counts4) *counts4 = rm->qCounts.data(); if (recStart) *recStart = rm->recStart.data(); if (recs) *recs = rm->recs.data();
  if (seedStart) *seedStart = rm->seedStart.data(); if (seeds) *seeds = rm->seeds.data(); if (seedPos) *seedPos = rm->seedPos.data();
  return 0;
}

}  // namespace h10x
