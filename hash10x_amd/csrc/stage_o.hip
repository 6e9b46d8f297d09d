// stage_o.hip — the state's in-range hashes as a classed mosh set, behind --writeMosh (include/h10x.h "the state as a mosh set").
//
// hash10x and moshutils -c make the same hasher from (k, w, seed), take their hashes from the same iterator and keep them in the same probe
// table (hashIndexFind, hash10x.c:139-152 = moshsetIndexFind, moshset.c:45-61), so a state is a mosh set that lacks the 16-bit depths and the
// info byte. The kept hashes are the x >= 1 with within[x], in ascending x; the k-th gets set index k (moshsetDepthPrune's renumbering,
// moshset.c:63-76). The class is moshutils -s over the saturated depth (moshutils.c:173-177) and, where a --hashCopies result is kept
// (stage_n.hip), second >= 2 makes it M and largest < 2 makes it 0.
//   classify  one lane per hash index: within[x] (1 B), hashDepth[x] (4 B), the 8-byte --hashCopies record as one load, cribType[x] with a
//             crib. Writes the keep flag and the class byte; the tallies by ballots per wave, one atomic per workgroup and counter.
//   number    prim_exclusive_scan_u32 over the flags; the total and the tallies come back in one read-back.
//   compact   value, depth (saturating) and info of the kept hashes to 1 + their rank, on the set's stream.
//   place     stage_g's moshPlace: an index takes the first slot of its probe sequence that is empty or held by a higher index, so the table
//             is the one sequential insertion in set-index order builds.
// No per-hash array passes through the host.
#include "common.hpp"
#include "prim.hpp"
#include "mosh.hpp"
#include "wave.hpp"

namespace h10x {

static constexpr unsigned SO_GRID = 2048;                     // workgroups of the classify kernel, at most: it ends in one atomic per counter
// the counters: [0 .. 4) kept per class, 4 raised to M by linkage, 5 lowered to 0 by linkage, 6 depths saturated, [8 .. 28) crib type x class
static constexpr int SO_TOM = 4, SO_TO0 = 5, SO_SAT = 6, SO_CRIB = 8, SO_COUNTERS = 28, SO_WORDS = 32;

// flag[x] = 1 for the kept hashes (flag[U1] = 0: the scan's last entry is their number), cls[x] = their class. hc = the kept --hashCopies
// records {distinct | groups << 16, largest | second << 16} or null (depth only); cribType = null without a crib
template <bool CRIB>
__global__ __launch_bounds__(256) void so_classify_kernel(const u8 *__restrict__ within, const u32 *__restrict__ hashDepth, const uint2 *__restrict__ hc,
                                                          const u8 *__restrict__ cribType, u32 U1, int c1, int c2, int cM, u32 *__restrict__ flag,
                                                          u8 *__restrict__ cls, unsigned long long *__restrict__ counts) {
  __shared__ u32 sCnt[256 / WAVE][SO_WORDS];
  const u64 stride = (u64)gridDim.x * blockDim.x;
  const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  u32 n[SO_COUNTERS];
#pragma unroll
  for (int k = 0; k < SO_COUNTERS; ++k) n[k] = 0;
  for (u64 x0 = (u64)blockIdx.x * blockDim.x; x0 <= U1; x0 += stride) {   // wave-uniform: whole workgroups
    const u64 x = x0 + threadIdx.x;
    bool keep = false, toM = false, to0 = false, sat = false; u32 q = 0, t = 0;
    if (x >= 1 && x < U1 && within[x]) {
      keep = true;
      u32 d = hashDepth[x];
      if (d > 65535u) { d = 65535u; sat = true; }
      const int di = (int)d;
      const u32 base = di < c1 ? 0u : di < c2 ? 1u : di < cM ? 2u : 3u;                 // moshutils.c:173-177
      q = base;
      if (hc) {
        const uint2 r = hc[x];
        const u32 largest = r.y & 0xFFFFu, second = r.y >> 16;
        if (second >= 2) q = 3; else if (largest < 2) q = 0;
        toM = q == 3 && base != 3; to0 = q == 0 && base != 0;
      }
      if (CRIB) { t = cribType[x]; if (t > 4) t = 0; }
    }
    if (x <= U1) { flag[x] = keep ? 1u : 0u; if (x < U1) cls[x] = (u8)q; }
#pragma unroll
    for (u32 k = 0; k < 4; ++k) n[k] += (u32)__popcll(__ballot(keep && q == k));
    n[SO_TOM] += (u32)__popcll(__ballot(toM)); n[SO_TO0] += (u32)__popcll(__ballot(to0)); n[SO_SAT] += (u32)__popcll(__ballot(sat));
    if (CRIB) {
#pragma unroll
      for (u32 k = 0; k < 20; ++k) n[SO_CRIB + k] += (u32)__popcll(__ballot(keep && t == k / 4 && q == k % 4));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < SO_COUNTERS; ++k) sCnt[wave][k] = n[k];
  }
  __syncthreads();
  if (threadIdx.x < SO_COUNTERS) {
    const u32 k = threadIdx.x;
    u32 v = sCnt[0][k];
    for (u32 w = 1; w < blockDim.x / WAVE; ++w) v += sCnt[w][k];
    if (v) atomicAdd(counts + k, (unsigned long long)v);
  }
}

// the kept hashes to their set indices: 1 + the kept hashes below x
__global__ void so_compact_kernel(const u32 *__restrict__ flag, const u32 *__restrict__ before, const u8 *__restrict__ cls, const u64 *__restrict__ hashValue,
                                  const u32 *__restrict__ hashDepth, u32 U1, u32 kept, u64 *__restrict__ value, u16 *__restrict__ depth, u8 *__restrict__ info) {
  const u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // 64-bit, as stage_g's loops over a set's entries
  if (x >= U1 || !flag[x]) return;
  const u32 r = before[x];
  if (r >= kept) return;                                     // (the arrays hold kept + 1 entries)
  const u32 o = 1 + r, d = hashDepth[x];
  value[o] = hashValue[x]; depth[o] = (u16)(d > 65535u ? 65535u : d); info[o] = cls[x];
}

int stageO_run(Ctx *c, int bits, int c1, int c2, int cM, Mosh **out, h10x_state_mosh_info *info) {
  *out = nullptr;
  if (!c->haveState) return c->fail("no hash state loaded: use readFQB or readHash first");
  if (c->sharded) return c->fail("writeMosh: not available on a sharded context (one rank holds only its own barcodes)");
  if (!c->haveRange || !c->haveGood) return c->fail("!! you must set hashDepthRange before writeMosh");   // after --clusterSplit too, as for the census commands
  if (c1 < 0 || c2 < c1 || cM < c2) return c->fail("!! writeMosh needs 0 <= copy1min <= copy2min <= copyMmin");
  if (bits != 0 && (bits < 20 || bits > 34)) return c->fail("!! writeMosh bits %d must be 0 or 20 .. 34", bits);
  if (!c->haveSeed) return c->fail("writeMosh: the context does not know the seed of its hasher: set option seqhash_seed to the -r value");
  u64 f1 = 0, f2 = 0; h10x_factors_from_seed(c->seed, (uint64_t *)&f1, (uint64_t *)&f2);
  if (f1 != c->prm.factor1) return c->fail("writeMosh: option seqhash_seed %d does not give the context's hash multiplier", c->seed);
  const int B = bits ? bits : c->prm.B;
  const u32 U1 = c->hashNumber;
  hipStream_t st = c->stream;
  const bool linked = c->haveHashCopies && c->hcHashes == U1;
  PrimTemp pt; DevBuf<u32> flag, pos; DevBuf<u8> cls; DevBuf<unsigned long long> counts;
  H10X_HIP(c, flag.alloc((size_t)U1 + 1)); H10X_HIP(c, pos.alloc((size_t)U1 + 1)); H10X_HIP(c, cls.alloc(U1)); H10X_HIP(c, counts.alloc(SO_WORDS));
  H10X_HIP(c, hipMemsetAsync(counts.p, 0, SO_WORDS * 8, st));
  const unsigned grid = (unsigned)hmin<u64>(divUp((u64)U1 + 1, 256), SO_GRID);
  const uint2 *hc = linked ? (const uint2 *)c->hcOut.p : nullptr;
  if (c->haveCrib) so_classify_kernel<true><<<grid, 256, 0, st>>>(c->within.p, c->hashDepth.p, hc, c->cribType.p, U1, c1, c2, cM, flag.p, cls.p, counts.p);
  else so_classify_kernel<false><<<grid, 256, 0, st>>>(c->within.p, c->hashDepth.p, hc, nullptr, U1, c1, c2, cM, flag.p, cls.p, counts.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32(c, pt, flag.p, pos.p, (size_t)U1 + 1));
  u32 kept = 0; u64 tl[SO_WORDS];
  H10X_TRY(c->readback(&kept, pos.p + U1, 4)); H10X_TRY(c->readback(tl, counts.p, SO_WORDS * 8)); H10X_TRY(c->syncReadbacks());
  H10X_HIP(c, hipStreamSynchronize(st));                      // the set's stream reads the context's arrays and the temporaries above from here
  if (tl[0] + tl[1] + tl[2] + tl[3] != kept) return c->fail("writeMosh: %u hashes kept at the scan and %llu at the tallies", kept, tl[0] + tl[1] + tl[2] + tl[3]);
  if ((u64)kept + 1 >= (((u64)1 << B) >> 2)) return c->fail("Moshset size %u is too big for %d bits", kept + 1, B);   // moshset.c:24

  char err[512] = "";
  Mosh *m = nullptr;
  if (moshOpen(&m, B, c->prm.k, c->prm.w, f1, f2, c->device, err, (int)sizeof err)) return c->fail("%s", err);
  auto body = [&]() -> int {
    Ctx *mc = &m->c; hipStream_t ms = mc->stream;
    H10X_TRY(moshEnter(m));
    H10X_TRY(moshAllocSet(m, kept + 1));                      // full, as after h10x_mosh_load
    if (kept) {
      so_compact_kernel<<<divUp(U1, 256), 256, 0, ms>>>(flag.p, pos.p, cls.p, c->hashValue.p, c->hashDepth.p, U1, kept, mc->hashValue.p, m->depth.p, m->info.p);
      H10X_HIP(mc, hipGetLastError());
      H10X_TRY(moshPlace(m, kept));
    }
    H10X_HIP(mc, hipStreamSynchronize(ms));                   // the temporaries go back to the context's block cache behind finished work
    return 0;
  };
  const int rc = body();
  AllocScope::stream() = c->stream; AllocScope::device() = c->device;   // (moshEnter pointed the allocations at the set's stream)
  if (rc) { c->fail("%s", m->c.err.c_str()); (void)hipStreamSynchronize(m->c.stream); stageG_destroy(m); AllocScope::stream() = c->stream; AllocScope::device() = c->device; return -1; }
  if (info) {
    memset(info, 0, sizeof *info);
    info->kept = kept;
    for (int q = 0; q < 4; ++q) info->copy[q] = tl[q];
    info->toM = tl[SO_TOM]; info->to0 = tl[SO_TO0]; info->saturated = tl[SO_SAT];
    for (int t = 0; t < 5; ++t) for (int q = 0; q < 4; ++q) info->crib[t][q] = tl[SO_CRIB + 4 * t + q];
    info->hashNumber = U1; info->bits = (u32)B; info->minShare = linked ? c->hcInfo.minShare : 0;
  }
  *out = m;
  return 0;
}

}  // namespace h10x
