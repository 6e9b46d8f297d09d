// seq_plan.hpp — the one k-mer walk behind the sequence scans (crib_scan_kernel of stage_d.hip, mosh_scan_kernel of stage_g.hip, rs_scan_kernel of stage_h.hip) and the
// plan of a batch: which lane run walks which k-mer starts. The same text runs on the device, in the drivers and in the host model of tests/seq_plan_model.cpp
// (under AddressSanitizer against the plain definitions). The header needs no HIP header.
#pragma once
#include <cstdint>
#include <vector>

#ifdef __HIPCC__
#define SEQ_FN __host__ __device__ __forceinline__
#else
#define SEQ_FN inline
#endif

namespace h10x {
typedef unsigned long long u64; typedef uint32_t u32; typedef uint8_t u8;      // (as in common.hpp)

constexpr int SEQ_RUN = 64;                                  // k-mer start positions per lane
constexpr int MOSH_X_SKIP = 23;                              // moshutils.c:43: barcode + spacer of the first read of a 10x pair

// the per-sequence offset rule: with odd set, the 1st, 3rd, ... sequence of the FILE (base = its sequences before this batch) starts MOSH_X_SKIP bases in
struct SeqSkip { int odd; u64 base; SEQ_FN u64 of(u32 s) const { return (odd && ((base + s + 1) & 1)) ? MOSH_X_SKIP : 0; } };

// the rolling forward and reverse-complement words of one walk and the mosh hash of each k-mer: the arithmetic of mosh_lds_kernel (seqhash.c:58-80, 154-195)
struct KmerRoll {
  int k, k2, shift1; u64 mask, factor1, f = 0, rc = 0, hf = 0, hr = 0;
  SEQ_FN KmerRoll(int k_, u64 factor1_) : k(k_), k2(2 * k_), shift1(64 - 2 * k_), mask(2 * k_ == 64 ? ~0ULL : ((1ULL << (2 * k_)) - 1)), factor1(factor1_) {}
  SEQ_FN void prime(const u8 *b) {                           // the first k - 1 bases of the walk
    for (int j = 0; j < k - 1; ++j) { const u64 x = b[j] & 3; f = (f << 2) | x; rc = (rc >> 2) | ((3 - x) << (k2 - 2)); }
  }
  SEQ_FN u64 next(u8 code) {                                 // the hash of the k-mer that this base ends
    const u64 x = code & 3;
    f = ((f << 2) | x) & mask; rc = (rc >> 2) | ((3 - x) << (k2 - 2));          // seqhash.c:72-76
    hf = (f * factor1) >> shift1; hr = (rc * factor1) >> shift1;                // seqhash.c:58-59
    return fwd() ? hf : hr;
  }
  SEQ_FN bool fwd() const { return hf < hr; }                // the forward strand of the last k-mer won: a tie is reverse (seqhash.c:67)
};

// A batch of nSeq whole sequences, bases [seqStart[s], seqStart[s + 1]). rel[] = the starts rebased to the batch's first base; runStart[s] = lane runs of SEQ_RUN
// k-mer starts in the sequences before s: a sequence with fewer than k bases behind its skip has none (seqhash.c:162); nK = k-mers in all; tooShort = the first
// sequence that is shorter than its skip, nSeq if there is none. The plan states facts: the callers word their errors
struct SeqPlan {
  std::vector<u64> rel, runStart; u64 nK = 0, total = 0, nRuns = 0; u32 tooShort;
  SeqPlan(const u64 *seqStart, u32 nSeq, int k, SeqSkip skip = SeqSkip{0, 0}) : rel((size_t)nSeq + 1), runStart((size_t)nSeq + 1, 0), tooShort(nSeq) {
    for (u32 s = 0; s <= nSeq; ++s) rel[s] = seqStart[s] - seqStart[0];
    for (u32 s = 0; s < nSeq; ++s) {
      const u64 off = skip.of(s); u64 n = len(s);
      if (n < off && tooShort == nSeq) tooShort = s;
      n = n >= off + (u64)k ? n - off - (u64)k + 1 : 0;
      nK += n; runStart[s + 1] = runStart[s] + (n + SEQ_RUN - 1) / SEQ_RUN;
    }
    total = rel[nSeq]; nRuns = runStart[nSeq];
  }
  u64 len(u32 s) const { return rel[s + 1] - rel[s]; }
  u64 cap(int w) const { const u64 e = 2 * (nK / (u64)w) + ((u64)1 << 16); return nK < e ? nK : e; }   // a scan's list at first: about nK / w moshes, never above nK
};

}  // namespace h10x
