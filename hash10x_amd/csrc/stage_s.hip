// stage_s.hip — sequence spectrum, behind --seqSpectrum: the moshes of sequences classed by the read depth of their hash, per sequence and per window, the
// number of times the sequences hold every hash of the state, and the depth x copies matrix (include/h10x.h "sequence spectrum").
// Per slab of whole sequences:
//   scan     stage_g's mosh_scan_kernel<0> with the CONTEXT's hasher: every mosh occurrence as (hash, ordinal of its k-mer in the slab);
//   look-up  one lane per occurrence: the probe of sr_lookup_kernel, the key ordinal << 3 | class (0 absent, 1 .. 4 = depth class 0, 1, 2, M) with the index
//            as value, and +1 on copies[index] for a found one;
//   order    a sort by ordinal puts the occurrences in (sequence, position) order;
//   tally    one wave per segment, a window or a whole sequence: two searches in the sorted keys bound it, the lanes stride over its occurrences, wave_sum folds
//            the class counts and the depth sum and lane 0 stores the record. No atomic: a segment is a stretch of the sorted keys. The kernel runs once over the windows and once
//            over the sequences.
// At the end one pass over the hashes bins (depth, copies) in a workgroup's LDS and flushes the bins in use.
#include "census_rows.hpp"
#include "mosh.hpp"
#include "wave.hpp"

namespace h10x {

static constexpr u32 SS_DEPTH_BINS = H10X_SPECTRUM_DEPTH_BINS, SS_COPY_BINS = H10X_SPECTRUM_COPY_BINS, SS_BINS = SS_DEPTH_BINS * SS_COPY_BINS;

// depth class of a hash by the three thresholds (u64: a threshold beyond any u32 depth is never reached)
__device__ __forceinline__ u32 ss_class(u32 d, u64 c1, u64 c2, u64 cM) { return d < c1 ? 0u : d < c2 ? 1u : d < cM ? 2u : 3u; }

// The copies: one integer add per found occurrence on the word of its hash. The words are scattered over hashNumber (a hash repeats only where the sequences do),
// so there is nothing to fold per wave or workgroup first, and integer adds give the same array in any order.
__global__ __launch_bounds__(256) void ss_lookup_kernel(const u64 *__restrict__ hash, const u32 *__restrict__ ord, u64 n, const u32 *__restrict__ table,
                                                        const u64 *__restrict__ hashValue, int B, const u32 *__restrict__ hashDepth, u32 U1, u64 c1, u64 c2, u64 cM,
                                                        u64 *__restrict__ key, u32 *__restrict__ xs, u32 *__restrict__ copies) {
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    u32 x = probe_find(table, hashValue, B, hash[i]);
    if (x >= U1) x = 0;                                       // (a table entry beyond hashNumber is no index of this state)
    key[i] = (u64)ord[i] << 3 | (x ? 1u + ss_class(hashDepth[x], c1, c2, cM) : 0u);
    xs[i] = x;
    if (x) atomicAdd(&copies[x], 1u);
  }
}

// One wave per segment g < nSeg of the slab. W >= 1: g is a window, of sequence s = the last with winOff[s] <= g, and holds the ordinals
// [seqRel[s] + j W, min(seqRel[s] + (j + 1) W, seqRel[s + 1])), j = g - winOff[s]. W = 0: g is a sequence, whole. A segment of any length (0, 1, 65, hundreds of
// occurrences) is one wave's: nothing is per workgroup
__global__ __launch_bounds__(256) void ss_tally_kernel(const u64 *__restrict__ key, const u32 *__restrict__ xs, u64 n, const u64 *__restrict__ seqRel, u32 ns,
                                                       const u64 *__restrict__ winOff, u64 nSeg, u32 W, const u32 *__restrict__ hashDepth,
                                                       h10x_seq_spectrum_window *__restrict__ out) {
  const u32 lane = threadIdx.x & (WAVE - 1);
  const u64 w0 = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / WAVE, wStride = ((u64)gridDim.x * blockDim.x) / WAVE;
  for (u64 g = w0; g < nSeg; g += wStride) {                  // (wave-uniform: the folds below see all 64 lanes)
    u64 lo, hi;
    if (W) {
      const u32 s = last_le(winOff, ns, g);
      lo = seqRel[s] + (g - winOff[s]) * W; hi = lo + W < seqRel[s + 1] ? lo + W : seqRel[s + 1];
    } else { lo = seqRel[g]; hi = seqRel[g + 1]; }
    const u64 a = lower_bound(key, (u64)0, n, lo << 3), e = lower_bound(key, a, n, hi << 3);
    u32 cnt[5] = {0, 0, 0, 0, 0}; u64 sum = 0;
    for (u64 i = a + lane; i < e; i += WAVE) {
      const u32 cls = (u32)(key[i] & 7);
#pragma unroll
      for (u32 q = 0; q < 5; ++q) cnt[q] += cls == q;
      if (cls) sum += hashDepth[xs[i]];
    }
#pragma unroll
    for (u32 q = 0; q < 5; ++q) cnt[q] = wave_sum(cnt[q]);
    sum = wave_sum(sum);
    if (lane == 0) {
      h10x_seq_spectrum_window r;
      r.moshes = (u32)(e - a); r.absent = cnt[0]; r.n0 = cnt[1]; r.n1 = cnt[2]; r.n2 = cnt[3]; r.nM = cnt[4]; r.depthSum = sum;
      out[g] = r;
    }
  }
}

// Every hash x = 1 .. U1 - 1 once: S[min(depth, 1023)][min(copies, 7)] += 1, totals[class] += 1, totals[4 + class] += copies >= 1, *maxCopies = max.
// The workgroup bins into its own LDS matrix of u32 and adds the bins in use to the global u64 matrix at its end, once. No LDS counter can wrap: a workgroup bins
// at most U1 - 1 < 2^32 hashes in all (hashNumber is a u32), so it needs no flush in between. The eight totals are folded per wave, gathered per workgroup in LDS
// and added once per workgroup.
__global__ __launch_bounds__(256) void ss_spectrum_kernel(const u32 *__restrict__ hashDepth, const u32 *__restrict__ copies, u32 U1, u64 c1, u64 c2, u64 cM,
                                                          u64 *__restrict__ S, u64 *__restrict__ totals, u32 *__restrict__ maxCopies) {
  __shared__ u32 hist[SS_BINS];
  __shared__ u32 wg[9];
  for (u32 b = threadIdx.x; b < SS_BINS; b += blockDim.x) hist[b] = 0;
  if (threadIdx.x < 9) wg[threadIdx.x] = 0;
  __syncthreads();
  u32 t[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mx = 0;
  const u64 stride = (u64)gridDim.x * blockDim.x;
  for (u64 x = 1 + (u64)blockIdx.x * blockDim.x + threadIdx.x; x < U1; x += stride) {
    const u32 d = hashDepth[x], cp = copies[x], q = ss_class(d, c1, c2, cM);
#pragma unroll
    for (u32 k = 0; k < 4; ++k) { t[k] += q == k; t[4 + k] += (q == k) & (cp != 0); }
    mx = cp > mx ? cp : mx;
    atomicAdd(&hist[(d < SS_DEPTH_BINS - 1 ? d : SS_DEPTH_BINS - 1) * SS_COPY_BINS + (cp < SS_COPY_BINS - 1 ? cp : SS_COPY_BINS - 1)], 1u);
  }
#pragma unroll
  for (u32 k = 0; k < 8; ++k) t[k] = wave_sum(t[k]);
  mx = wave_max(mx);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
    for (u32 k = 0; k < 8; ++k) if (t[k]) atomicAdd(&wg[k], t[k]);
    atomicMax(&wg[8], mx);
  }
  __syncthreads();
  for (u32 b = threadIdx.x; b < SS_BINS; b += blockDim.x) { const u32 v = hist[b]; if (v) atomicAdd((unsigned long long *)&S[b], (unsigned long long)v); }
  if (threadIdx.x < 8 && wg[threadIdx.x]) atomicAdd((unsigned long long *)&totals[threadIdx.x], (unsigned long long)wg[threadIdx.x]);
  if (threadIdx.x == 8 && wg[8]) atomicMax(maxCopies, wg[8]);
}

namespace {

inline u64 ss_windows(u64 L, u32 W) { return W ? L / W + (L % W != 0) : 0; }   // ceil(L / W) in 64 bits; none at W = 0

const char *const SS_NO_RUN = "seqSpectrum: no run is open (h10x_seq_spectrum_begin opens one, h10x_seq_spectrum_finish closes it)";
const char *const SS_NONE = "seqSpectrum: no result is kept (begin a run first; --clusterSplit and a new state release it)";

struct SeqSpectrum {
  Ctx *c; h10x_seq_spectrum_info *info; PrimTemp pt;
  u64 used = 0;                                               // window records of this call so far

  int tally(const u64 *key, const u32 *xs, u64 n, const u64 *seqRel, u32 ns, const u64 *winOff, u64 nSeg, u32 W, h10x_seq_spectrum_window *out) {
    if (!nSeg) return 0;
    if (!n) { H10X_HIP(c, hipMemsetAsync(out, 0, (size_t)nSeg * sizeof *out, c->stream)); return 0; }   // (no occurrence: no scan ran, every record is zero)
    ss_tally_kernel<<<(unsigned)hmin<u64>((nSeg + 256 / WAVE - 1) / (256 / WAVE), 65536), 256, 0, c->stream>>>(key, xs, n, seqRel, ns, winOff, nSeg, W, c->hashDepth.p, out);
    H10X_HIP(c, hipGetLastError());
    return 0;
  }

  // one slab: sequences [0, ns) from slabStart; fig (may be null) and the call's window offsets at the slab's first sequence
  int slab(const u8 *codes, const u64 *slabStart, u32 ns, h10x_seq_spectrum_figures *fig, u64 *winOffsets) {
    hipStream_t st = c->stream;
    const u32 W = c->spW;
    std::vector<u64> hWin((size_t)ns + 1, 0);
    std::vector<h10x_seq_spectrum_window> hRec(ns);
    for (u32 s = 0; s < ns; ++s) { hWin[s + 1] = hWin[s] + ss_windows(slabStart[s + 1] - slabStart[s], W); winOffsets[s + 1] = winOffsets[0] + hWin[s + 1]; }
    const u64 nW = hWin[ns], bases = slabStart[ns] - slabStart[0];
    MoshBatch b;
    H10X_TRY(moshScanWith(c, c->prm.k, c->prm.w, c->prm.factor1, c->prm.B, nullptr, 0, b, codes, slabStart, ns, 0, 0));
    const u64 n = b.listed;
    if (n > 0xFFFFFFFEull) return c->fail("seqSpectrum: %llu moshes in one batch", n);
    const int ob = keyBits(bases);
    if (n && ob > 32) return c->fail("seqSpectrum: a slab of %llu bases: the ordinal of a k-mer does not fit 32 bits", bases);
    StreamWait wait{st};                                      // (the copies below read and write these vectors)
    DevBuf<u64> key, keyS, dWin; DevBuf<u32> xs, xsS; DevBuf<h10x_seq_spectrum_window> dRec;
    H10X_HIP(c, dRec.alloc(ns));
    if (nW) {
      H10X_TRY(reserve_keep(c, c->spWin, used, used + nW));
      H10X_HIP(c, dWin.alloc((size_t)ns + 1));
      H10X_HIP(c, hipMemcpyAsync(dWin.p, hWin.data(), ((size_t)ns + 1) * 8, hipMemcpyHostToDevice, st));
    }
    if (n) {
      H10X_HIP(c, key.alloc(n)); H10X_HIP(c, keyS.alloc(n)); H10X_HIP(c, xs.alloc(n)); H10X_HIP(c, xsS.alloc(n));
      ss_lookup_kernel<<<(unsigned)hmin<u64>(divUp(n, 256), 16384), 256, 0, st>>>(b.outHash.p, b.outOrd.p, n, c->hashIndex.p, c->hashValue.p, c->prm.B, c->hashDepth.p,
                                                                                   c->hashNumber, c->spThr[0], c->spThr[1], c->spThr[2], key.p, xs.p, c->spCopies.p);
      H10X_HIP(c, hipGetLastError());
      H10X_TRY(prim_sort_pairs_u64_u32(c, pt, key.p, keyS.p, xs.p, xsS.p, n, 3, 3 + ob));   // by ordinal: at most one mosh per k-mer start
    }
    if (nW) H10X_TRY(tally(keyS.p, xsS.p, n, b.seq.p, ns, dWin.p, nW, W, c->spWin.p + used));
    H10X_TRY(tally(keyS.p, xsS.p, n, b.seq.p, ns, nullptr, ns, 0, dRec.p));
    H10X_HIP(c, hipMemcpyAsync(hRec.data(), dRec.p, (size_t)ns * sizeof(h10x_seq_spectrum_window), hipMemcpyDeviceToHost, st));
    H10X_HIP(c, hipStreamSynchronize(st));
    for (u32 s = 0; s < ns; ++s) {
      const h10x_seq_spectrum_window &r = hRec[s];
      if (fig) { h10x_seq_spectrum_figures &o = fig[s]; o.len = slabStart[s + 1] - slabStart[s]; o.moshes = r.moshes; o.absent = r.absent; o.n0 = r.n0; o.n1 = r.n1; o.n2 = r.n2; o.nM = r.nM; o.depthSum = r.depthSum; }
      info->moshes += r.moshes; info->absent += r.absent; info->n0 += r.n0; info->n1 += r.n1; info->n2 += r.n2; info->nM += r.nM; info->depthSum += r.depthSum;
    }
    info->bases += bases; info->windows += nW; used += nW;
    return 0;
  }

  int run(const u8 *codes, const u64 *seqStart, u32 nSeq, h10x_seq_spectrum_figures *fig) {
    const u64 slabBases = c->optSeqSlab > 0 ? (u64)c->optSeqSlab : MOSH_SLAB_DEFAULT;
    for (u32 s = 0; s < nSeq; ++s) {                            // the scan trusts the lengths
      if (seqStart[s + 1] < seqStart[s]) return c->fail("seqSpectrum: the sequence starts do not ascend at sequence %u", s);
      const u64 L = seqStart[s + 1] - seqStart[s];
      if (ss_windows(L, c->spW) > 0xFFFFFFFFull) return c->fail("seqSpectrum: sequence %u of %llu bases has more than 2^32 - 1 windows of %u", s, L, c->spW);
    }
    c->spHostWinOff.assign((size_t)nSeq + 1, 0);
    for (u32 s0 = 0; s0 < nSeq;) {
      u32 s1 = s0 + 1;                                          // as many whole sequences as fit the slab; a longer one goes alone (moshBatches)
      while (s1 < nSeq && seqStart[s1 + 1] - seqStart[s0] <= slabBases) ++s1;
      H10X_TRY(slab(codes, seqStart + s0, s1 - s0, fig ? fig + s0 : nullptr, c->spHostWinOff.data() + s0));
      s0 = s1;
    }
    return 0;
  }
};

}  // namespace

void stageS_release(Ctx *c) {
  c->haveSpectrum = c->spOpen = false; c->spWindows = 0; c->spSeqs = 0; c->spHostWinOff.clear(); c->spCopies.release(); c->spWin.release();
  memset(&c->spRun, 0, sizeof c->spRun);
}

int stageS_begin(Ctx *c, int64_t copy1min, int64_t copy2min, int64_t copyMmin, int64_t window) {
  stageS_release(c);
  if (!c->haveState) return c->fail("no hash state loaded: use readFQB or readHash first");
  if (c->sharded) return c->fail("seqSpectrum: not available on a sharded context (one rank holds only its own barcodes)");
  if (copy1min < 0 || copy2min < copy1min || copyMmin < copy2min) return c->fail("!! seqSpectrum needs 0 <= copy1min <= copy2min <= copyMmin");
  if (window < 0) return c->fail("!! seqSpectrum window %lld must be >= 0", (long long)window);
  H10X_TRY(sp_check_hasher(c, "seqSpectrum"));
  // a position is a u32: a window beyond it acts as the largest u32 does; a depth is a u32: the thresholds stay 64 bits wide, one beyond it is never reached
  c->spThr[0] = (u64)copy1min; c->spThr[1] = (u64)copy2min; c->spThr[2] = (u64)copyMmin;
  c->spW = (u32)hmin<int64_t>(window, 0xFFFFFFFFll);
  H10X_HIP(c, c->spCopies.alloc(c->hashNumber));
  H10X_HIP(c, hipMemsetAsync(c->spCopies.p, 0, (size_t)c->hashNumber * 4, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  c->spRun.hashNumber = c->hashNumber;
  c->haveSpectrum = c->spOpen = true;
  return 0;
}

int stageS_add(Ctx *c, const u8 *codes, const u64 *seqStart, u32 nSeq, h10x_seq_spectrum_figures *fig, h10x_seq_spectrum_info *info) {
  if (!c->spOpen) return c->fail("%s", SS_NO_RUN);
  if (nSeq && (!codes || !seqStart)) return c->fail("seqSpectrum: null argument");
  memset(info, 0, sizeof *info);
  info->sequences = nSeq; info->hashNumber = c->hashNumber;
  c->spWindows = 0; c->spSeqs = 0;
  SeqSpectrum g; g.c = c; g.info = info;
  const u64 zero = 0;
  const int rc = g.run(codes, nSeq ? seqStart : &zero, nSeq, fig);
  if (rc) { (void)hipStreamSynchronize(c->stream); stageS_release(c); return rc; }   // (copies[] holds a part of this call: the run is over)
  c->spWindows = g.used; c->spSeqs = nSeq;
  h10x_seq_spectrum_info &t = c->spRun;
  t.sequences += nSeq; t.bases += info->bases; t.moshes += info->moshes; t.absent += info->absent; t.n0 += info->n0; t.n1 += info->n1; t.n2 += info->n2;
  t.nM += info->nM; t.depthSum += info->depthSum; t.windows += info->windows;
  return 0;
}

int stageS_windowsGet(Ctx *c, u64 *winOffsets, h10x_seq_spectrum_window *records, u64 cap) {
  if (!c->haveSpectrum) return c->fail("%s", SS_NONE);
  if (winOffsets) { if (c->spHostWinOff.empty()) winOffsets[0] = 0; else memcpy(winOffsets, c->spHostWinOff.data(), ((size_t)c->spSeqs + 1) * 8); }
  const size_t m = (size_t)hmin<u64>(cap, c->spWindows);
  if (m && records) H10X_HIP(c, hipMemcpyAsync(records, c->spWin.p, m * sizeof *records, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int stageS_finish(Ctx *c, u64 *spectrum, u64 *totals, h10x_seq_spectrum_info *info) {
  if (!c->spOpen) return c->fail("%s", SS_NO_RUN);
  hipStream_t st = c->stream;
  DevBuf<u64> dS; DevBuf<u32> dMax;
  H10X_HIP(c, dS.alloc(SS_BINS + 8)); H10X_HIP(c, dMax.alloc(1));
  H10X_HIP(c, hipMemsetAsync(dS.p, 0, (size_t)(SS_BINS + 8) * 8, st)); H10X_HIP(c, hipMemsetAsync(dMax.p, 0, 4, st));
  const u32 U1 = c->hashNumber;
  if (U1 > 1) {
    // every workgroup ends in up to SS_BINS adds on the global matrix: few workgroups with many hashes each
    ss_spectrum_kernel<<<(unsigned)hmin<u64>(divUp((u64)U1, 256 * 64), (u64)c->numCU * 2), 256, 0, st>>>(c->hashDepth.p, c->spCopies.p, U1, c->spThr[0], c->spThr[1],
                                                                                                         c->spThr[2], dS.p, dS.p + SS_BINS, dMax.p);
    H10X_HIP(c, hipGetLastError());
  }
  u32 mx = 0;
  if (spectrum) H10X_HIP(c, hipMemcpyAsync(spectrum, dS.p, (size_t)SS_BINS * 8, hipMemcpyDeviceToHost, st));
  if (totals) H10X_HIP(c, hipMemcpyAsync(totals, dS.p + SS_BINS, 64, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipMemcpyAsync(&mx, dMax.p, 4, hipMemcpyDeviceToHost, st));
  H10X_HIP(c, hipStreamSynchronize(st));
  c->spRun.maxCopies = mx; c->spRun.hashNumber = U1;
  *info = c->spRun;
  c->spOpen = false;
  return 0;
}

int stageS_copiesGet(Ctx *c, u64 first, u64 count, u32 *out) {
  if (!c->haveSpectrum) return c->fail("%s", SS_NONE);
  if (first > c->hashNumber || count > c->hashNumber - first) return c->fail("seqSpectrum: copies %llu .. %llu of %u hashes", first, first + count, c->hashNumber);
  if (count && out) H10X_HIP(c, hipMemcpyAsync(out, c->spCopies.p + first, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
  H10X_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace h10x
