// stage_k.hip — the molecule of every read pair (--moleculeMap) and the records in molecule order (--splitFQB). The reference stops at
// the hash level: --clusterReport counts the reads of a cluster (hash10x.c:897-920) and --clusterSplit renumbers the reads of each new
// block (hash10x.c:979-989), but neither says which records of the .fqb those reads are. Both follow from the state after --cluster:
//
//   nCodes = nBlocks (slot 0 unused), base[c] = records of blocks 1 .. c-1, R = base[nCodes]: record base[c] + r is read pair r of block c.
//   A ClusterHash record of block c is clustered with label cl = subCluster when 1 <= subCluster <= nSubCluster[c] (split_move_kernel's
//   guard, stage_c_split.hip) and its read lies inside the block. A read's label L is that of its FIRST clustered record in block order, its
//   slot the number of clustered reads of the block with the same label whose first clustered record lies earlier — the order of the
//   reference's ++new2[clus].nRead —, its molecule nCodes - 1 + subBefore[c] + L, the block number --clusterSplit gives the cluster.
//   An unclustered read keeps mol = c, slot = r. Split order: record -> start[mol] + slot for a molecule, start[c] + (unclustered records
//   of c in front of it) for what stays in a parent; start[] = exclusive sum of the records per post-split block.
//
//   aux      per block: records, sub-clusters, scratch words; the lowest block that has a parent / is clustered with more than 65536 reads
//   map      one wave per block. Pass 1: first[read] = min position of a clustered record (LDS where the block's reads fit, else the
//            block's own slice of a scratch array in HBM: integer min either way). Pass 2 over the positions in order, 64 a step: a
//            position counts if it is its read's first; its rank = the label's running counter + the counting lanes of the same label
//            in front of it in the step (ballot / leader loop as nb_hist_kernel, stage_f.hip); the counters live in LDS, one wave owns
//            them: no atomics. Pass 3 over the reads: the unclustered ones keep their block, numbered by a running ballot count.
//            Blocks without clusters are a streaming fill.
//   check    blocks whose records do not all carry word 0 of the block's first record (unless that is 0, the all-A barcode, the only
//            one that can swallow a following run: hash10x.c:212, replayChunks): the file is not the one the state was read from
//   move     idx[start[mol] + rank] = record, then one lane per dword as gather_records_kernel (stage_a.hip): 120-byte reads, coalesced writes
#include "prim.hpp"

namespace h10x {

constexpr u32 MOL_LDS_READS = 2048;                          // reads of a block whose first[] lives in LDS (8 KiB + 1 KiB of counters per wave)
constexpr u32 MOL_NONE = 0xFFFFFFFFu;
constexpr u32 MOL_MAX_READS = 65536;                         // ClusterHash.read is 16 bits (hash10x.c:37, 180): beyond, a read's records are not its own

static inline unsigned gridFor(u64 items, unsigned cap) { return (unsigned)hmax<u64>(1, hmin<u64>(divUp(items, 256), cap)); }

// entries 0 .. nCodes (the last one 0, for the scans); bad[0] / bad[1] = lowest block with a parent / clustered with too many reads
__global__ void molmap_aux_kernel(const h10x_block *__restrict__ blocks, u32 nCodes, u32 ldsReads, u32 *__restrict__ nRead, u32 *__restrict__ nSub,
                                  u32 *__restrict__ need, u32 *bad) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > nCodes) return;
  u32 r = 0, s = 0, w = 0;
  if (i < nCodes) {
    const h10x_block b = blocks[i];
    s = b.nSubCluster;
    if (i) {
      r = b.nRead;
      if (s && r > ldsReads) w = r;
      if (b.clusterParent) atomicMin(&bad[0], i);            // (error path only)
      if (s && r > MOL_MAX_READS) atomicMin(&bad[1], i);
    }
  }
  nRead[i] = r; nSub[i] = s; need[i] = w;
}

__device__ __forceinline__ u32 mol_label(u64 e, u32 nSub, u32 nRead, u32 &read) {
  read = (u32)(e >> 32) & 0xFFFFu;
  const u32 s = (u32)(e >> 48) & 0xFFu;
  return (s && s <= nSub && read < nRead) ? s : 0u;
}
template <bool LDS> __device__ __forceinline__ u32 mol_first(const u32 *first, u32 r) {
  if (LDS) return first[r];
  return __hip_atomic_load(first + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // written by atomics: read where they landed
}

// one clustered block on one wave; first[] holds MOL_NONE in its nR entries on entry (LDS: set here; HBM: set by the driver), seen[] is cleared here
template <bool LDS>
__device__ __forceinline__ void mol_block(u32 *first, u32 *seen, const u64 *__restrict__ e, u64 nH, u32 nR, u32 nS, u32 c, u32 ext, u64 r0,
                                          u32 *__restrict__ mol, u32 *__restrict__ slot, u32 *__restrict__ rank, u32 *__restrict__ cnt) {
  const u32 lane = threadIdx.x;
  const u64 below = ((u64)1 << lane) - 1;
  if (LDS) for (u32 r = lane; r < nR; r += WAVE) first[r] = MOL_NONE;
  for (u32 j = lane; j < 256; j += WAVE) seen[j] = 0;
  __syncthreads();
  for (u64 p = lane; p < nH; p += WAVE) {                    // pass 1: the first clustered position of every read
    u32 rd; if (mol_label(e[p], nS, nR, rd)) atomicMin(&first[rd], (u32)p);
  }
  if (!LDS) __threadfence();
  __syncthreads();
  for (u64 p0 = 0; p0 < nH; p0 += WAVE) {                    // pass 2: number the reads of every label in order of those positions
    const u64 p = p0 + lane;
    u32 cl = 0, rd = 0, my = 0;
    if (p < nH) { cl = mol_label(e[p], nS, nR, rd); if (cl && mol_first<LDS>(first, rd) != (u32)p) cl = 0; }
    u64 pending = __ballot(cl != 0);
    while (pending) {                                        // wave-uniform: one turn per distinct label of the step
      const int leader = __ffsll((unsigned long long)pending) - 1;
      const u32 la = __shfl(cl, leader);
      const u64 same = __ballot(cl == la);
      const u32 before = seen[la];
      if (cl == la) my = before + (u32)__popcll(same & below);
      __syncthreads();
      if ((int)lane == leader) seen[la] = before + (u32)__popcll(same);
      __syncthreads();
      pending &= ~same;
    }
    if (cl) {
      const u64 i = r0 + rd;
      if (mol) mol[i] = ext + cl;
      if (slot) slot[i] = my;
      if (rank) rank[i] = my;
    }
  }
  u32 run = 0;
  for (u32 q0 = 0; q0 < nR; q0 += WAVE) {                    // pass 3: what stays in the parent, in file order
    const u32 r = q0 + lane;
    const bool un = r < nR && mol_first<LDS>(first, r) == MOL_NONE;
    const u64 m = __ballot(un);
    if (un) {
      const u64 i = r0 + r;
      if (mol) mol[i] = c;
      if (slot) slot[i] = r;
      if (rank) rank[i] = run + (u32)__popcll(m & below);
    }
    run += (u32)__popcll(m);
  }
  if (lane == 0) cnt[c] = run;
  for (u32 j = 1 + lane; j <= nS && j < 256; j += WAVE) cnt[ext + j] = seen[j];
  __syncthreads();                                           // first[] / seen[] are the next block's
}

// cnt[0 .. nCodes + M) = records per post-split block (zeroed by the driver); mol / slot / rank may each be null
__global__ void __launch_bounds__(WAVE) molmap_kernel(const h10x_block *__restrict__ blocks, const u64 *__restrict__ blockOff, const h10x_clushash *__restrict__ ch,
                                                      u32 nCodes, const u64 *__restrict__ base, const u32 *__restrict__ subBefore, const u64 *__restrict__ scrOff,
                                                      u32 *scratch, u32 ldsReads, u32 *__restrict__ mol, u32 *__restrict__ slot, u32 *__restrict__ rank,
                                                      u32 *__restrict__ cnt) {
  __shared__ u32 firstL[MOL_LDS_READS];
  __shared__ u32 seen[256];
  const u32 lane = threadIdx.x;
  for (u32 c = blockIdx.x + 1; c < nCodes; c += gridDim.x) {
    const h10x_block b = blocks[c];
    const u32 nR = b.nRead, nS = b.nSubCluster; const u64 r0 = base[c];
    if (!nS) {
      for (u32 r = lane; r < nR; r += WAVE) {
        const u64 i = r0 + r;
        if (mol) mol[i] = c;
        if (slot) slot[i] = r;
        if (rank) rank[i] = r;
      }
      if (lane == 0) cnt[c] = nR;
      continue;
    }
    const u64 *e = reinterpret_cast<const u64 *>(ch + blockOff[c]);
    const u32 ext = nCodes - 1 + subBefore[c];
    if (nR <= ldsReads) mol_block<true>(firstL, seen, e, b.nHash, nR, nS, c, ext, r0, mol, slot, rank, cnt);
    else mol_block<false>(scratch + scrOff[c], seen, e, b.nHash, nR, nS, c, ext, r0, mol, slot, rank, cnt);
  }
}

__global__ void __launch_bounds__(WAVE) molmap_barcode_kernel(const u32 *__restrict__ rec, const h10x_block *__restrict__ blocks, const u64 *__restrict__ base,
                                                              u32 nCodes, u32 *bad /* [0] blocks, [1] the lowest */) {
  const u32 lane = threadIdx.x;
  for (u32 c = blockIdx.x + 1; c < nCodes; c += gridDim.x) {
    const u32 nR = blocks[c].nRead; if (!nR) continue;
    const u64 r0 = base[c];
    const u32 w0 = rec[r0 * 30]; if (!w0) continue;
    bool diff = false;
    for (u32 r = lane; r < nR; r += WAVE) diff |= rec[(r0 + r) * 30] != w0;
    if (__ballot(diff) && lane == 0) { atomicAdd(&bad[0], 1u); atomicMin(&bad[1], c); }   // (error path only)
  }
}

__global__ void molmap_index_kernel(const u32 *__restrict__ mol, const u32 *__restrict__ rank, const u64 *__restrict__ start, u64 n, u32 *__restrict__ idx) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) idx[start[mol[i]] + rank[i]] = (u32)i;
}
__global__ void molmap_move_kernel(const u32 *__restrict__ rec, const u32 *__restrict__ idx, u64 n, u32 *__restrict__ out) {
  const u64 stride = (u64)gridDim.x * blockDim.x, total = n * 30;
  for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) { const u64 j = t / 30; const u32 w = (u32)(t - j * 30); out[t] = rec[(u64)idx[j] * 30 + w]; }
}

struct MolPlan {
  DevBuf<u64> base, scrOff; DevBuf<u32> subBefore, scratch, cnt;
  u64 R = 0, scrWords = 0; u32 M = 0, nCodes = 0, ldsReads = MOL_LDS_READS;
};

// the refusals and the per-block offsets
static int mol_prepare(Ctx *c, const char *what, MolPlan &pl) {
  if (!c->haveState) return c->fail("%s: no hash state loaded: use readFQB or readHash first", what);
  if (c->sharded) return c->fail("%s does not run on a sharded context: each rank holds only its own barcodes, and the new blocks' numbers are given over all ranks", what);
  hipStream_t st = c->stream; PrimTemp pt;
  const u32 nCodes = pl.nCodes = c->nBlocks;
  pl.ldsReads = c->optMolGlobal ? 0 : MOL_LDS_READS;
  DevBuf<u32> nRead, nSub, need, bad;
  const size_t n1 = (size_t)nCodes + 1;
  H10X_HIP(c, nRead.alloc(n1)); H10X_HIP(c, nSub.alloc(n1)); H10X_HIP(c, need.alloc(n1)); H10X_HIP(c, bad.alloc(2));
  H10X_HIP(c, pl.base.alloc(n1)); H10X_HIP(c, pl.subBefore.alloc(n1)); H10X_HIP(c, pl.scrOff.alloc(n1));
  H10X_HIP(c, hipMemsetAsync(bad.p, 0xFF, 8, st));
  molmap_aux_kernel<<<divUp(n1, 256), 256, 0, st>>>(c->blocks.p, nCodes, pl.ldsReads, nRead.p, nSub.p, need.p, bad.p);
  H10X_HIP(c, hipGetLastError());
  H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, nRead.p, pl.base.p, n1));
  H10X_TRY(prim_exclusive_scan_u32(c, pt, nSub.p, pl.subBefore.p, n1));
  H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, need.p, pl.scrOff.p, n1));
  u32 hb[2] = {0, 0};
  H10X_TRY(c->readback(&pl.R, pl.base.p + nCodes, 8)); H10X_TRY(c->readback(&pl.M, pl.subBefore.p + nCodes, 4));
  H10X_TRY(c->readback(&pl.scrWords, pl.scrOff.p + nCodes, 8)); H10X_TRY(c->readback(hb, bad.p, 8));
  H10X_TRY(c->syncReadbacks());
  if (hb[0] != MOL_NONE) return c->fail("%s: block %u was made by --clusterSplit: the map needs the file's own barcodes, run it before --clusterSplit", what, hb[0]);
  if (hb[1] != MOL_NONE) return c->fail("%s: block %u is clustered and holds more than %u read pairs: their 16-bit read numbers wrap (hash10x.c:180), the molecule of such a read is not recoverable", what, hb[1], MOL_MAX_READS);
  if (pl.R >= ((u64)1 << 32)) return c->fail("%s: %llu records exceed this build's 2^32 limit", what, pl.R);
  if ((u64)nCodes + pl.M >= ((u64)1 << 31)) return c->fail("%s: %llu barcode blocks after the split", what, (u64)nCodes + pl.M);
  return 0;
}

// mol / slot / rank: device arrays of R entries or null; pl.cnt = records per post-split block, one more entry (0) for the scan
static int mol_run(Ctx *c, MolPlan &pl, u32 *dMol, u32 *dSlot, u32 *dRank) {
  hipStream_t st = c->stream;
  const size_t nOut = (size_t)pl.nCodes + pl.M + 1;
  H10X_HIP(c, pl.cnt.alloc(nOut));
  H10X_HIP(c, hipMemsetAsync(pl.cnt.p, 0, nOut * 4, st));
  H10X_HIP(c, pl.scratch.alloc(pl.scrWords));
  if (pl.scrWords) H10X_HIP(c, hipMemsetAsync(pl.scratch.p, 0xFF, pl.scrWords * 4, st));
  if (pl.nCodes > 1) {
    const unsigned grid = (unsigned)hmin<u64>(pl.nCodes - 1, (u64)c->numCU * 64);
    molmap_kernel<<<grid, WAVE, 0, st>>>(c->blocks.p, c->blockOff.p, c->clusHash.p, pl.nCodes, pl.base.p, pl.subBefore.p, pl.scrOff.p, pl.scratch.p,
                                         pl.ldsReads, dMol, dSlot, dRank, pl.cnt.p);
    H10X_HIP(c, hipGetLastError());
  }
  return 0;
}

int stageK_map(Ctx *c, u32 *dMol, u32 *dSlot, u64 cap, h10x_molmap_info *info) {
  MolPlan pl; PrimTemp pt;
  H10X_TRY(mol_prepare(c, "moleculeMap", pl));
  if ((dMol || dSlot) && cap < pl.R) return c->fail("moleculeMap: room for %llu entries, the state holds %llu records", cap, pl.R);
  H10X_TRY(mol_run(c, pl, dMol, dSlot, nullptr));
  u64 inMol = 0;
  if (pl.M) {
    DevBuf<u64> sum; H10X_HIP(c, sum.alloc(1));
    H10X_TRY(prim_reduce_sum_u32_u64(c, pt, pl.cnt.p + pl.nCodes, sum.p, pl.M));
    H10X_TRY(c->readback(&inMol, sum.p, 8)); H10X_TRY(c->syncReadbacks());
  }
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  if (info) { info->nRecords = pl.R; info->nClustered = inMol; info->nBlocks = pl.nCodes; info->nMolecules = pl.M; }
  return 0;
}

int stageK_records(Ctx *c, u64 *nRecords) {                  // R alone, with the refusals (the host forms size their buffers with it)
  MolPlan pl;
  H10X_TRY(mol_prepare(c, "splitFQB", pl));
  *nRecords = pl.R;
  return 0;
}

int stageK_split(Ctx *c, const u32 *dIn, u64 n, u32 *dOut, u64 *hostStart, u64 startCap) {
  MolPlan pl; PrimTemp pt; hipStream_t st = c->stream;
  H10X_TRY(mol_prepare(c, "splitFQB", pl));
  if (n != pl.R) return c->fail("splitFQB: %llu records given, the state was read from %llu", n, pl.R);
  const u64 nOut = (u64)pl.nCodes + pl.M + 1;
  if (!hostStart || startCap < nOut) return c->fail("splitFQB: room for %llu block starts, %llu needed", hostStart ? startCap : 0, nOut);
  if (n) {
    const uintptr_t a = (uintptr_t)dIn, b = (uintptr_t)dOut;
    if (a < b + n * 120 && b < a + n * 120) return c->fail("splitFQB: the input and output buffers overlap");
    DevBuf<u32> bad; H10X_HIP(c, bad.alloc(2));
    u32 init[2] = {0, MOL_NONE}, hb[2] = {0, 0};
    H10X_HIP(c, hipMemcpyAsync(bad.p, init, 8, hipMemcpyHostToDevice, st));
    molmap_barcode_kernel<<<(unsigned)hmax<u64>(1, hmin<u64>(pl.nCodes, (u64)c->numCU * 64)), WAVE, 0, st>>>(dIn, c->blocks.p, pl.base.p, pl.nCodes, bad.p);
    H10X_HIP(c, hipGetLastError());
    H10X_TRY(c->readback(hb, bad.p, 8)); H10X_TRY(c->syncReadbacks());
    if (hb[0]) return c->fail("splitFQB: the record image is not the file this state was read from: block %u holds more than one barcode (%u such blocks)", hb[1], hb[0]);
  }
  DevBuf<u32> mol, rank, idx; DevBuf<u64> start;
  H10X_HIP(c, mol.alloc(n)); H10X_HIP(c, rank.alloc(n)); H10X_HIP(c, idx.alloc(n)); H10X_HIP(c, start.alloc(nOut));
  H10X_TRY(mol_run(c, pl, mol.p, nullptr, rank.p));
  H10X_TRY(prim_exclusive_scan_u32_u64(c, pt, pl.cnt.p, start.p, nOut));
  if (n) {
    molmap_index_kernel<<<gridFor(n, 65535u * 4), 256, 0, st>>>(mol.p, rank.p, start.p, n, idx.p);
    molmap_move_kernel<<<gridFor(n * 30, 65535u * 16), 256, 0, st>>>(dIn, idx.p, n, dOut);
    H10X_HIP(c, hipGetLastError());
  }
  H10X_HIP(c, hipMemcpyAsync(hostStart, start.p, nOut * 8, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  return 0;
}

}  // namespace h10x
