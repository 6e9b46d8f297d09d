/* h10x_host.h — host side of the hash10x command surface, in C, above the C ABI of include/h10x.h.
 *
 * A session holds what the reference keeps in globals (hash10x.c:25-33, 85-104): the latched
 * parameters, the device context, and the Array bookkeeping (dim/max of hashDepth and
 * clusterBlocks, array.c:144-170) that decides bytes of the .hash file. Each function is one
 * command of the reference's argv loop (hash10x.c:1200-1269); hash10x_main.c is that loop.
 * All compute goes through libh10x_hip.so — there is no CPU path here.
 *
 * The h10x_host_write_* functions and the whitelist functions write and read the project's own formats from host arrays and
 * callbacks; they live in files_host.c, which needs no device library. Each writes <path>.part and renames it when it is whole.
 */
#ifndef H10X_HOST_H
#define H10X_HOST_H
#include <stdint.h>
#include <stdio.h>
#include "../../include/h10x.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct h10x_session h10x_session;

h10x_session *h10x_session_new(void);                 /* defaults of hash10x.c:1131-1137 */
void h10x_session_free(h10x_session *s);
/* -k -w -r -B -N -c -ct (hash10x.c:1174-1179,1239) plus "device" (HIP ordinal); latched until the
   next readFQB/readHash like the reference */
int  h10x_session_set(h10x_session *s, const char *name, int value);
int  h10x_session_get(const h10x_session *s, const char *name);
const char *h10x_session_error(const h10x_session *s);
h10x_ctx *h10x_session_ctx(h10x_session *s);

int  h10x_session_readFQB(h10x_session *s, const char *path);                         /* hash10x.c:1200-1205 */
int  h10x_session_begin(h10x_session *s);                 /* initialise() with the latched parameters (callers that use the C ABI directly) */
int  h10x_session_after_read(h10x_session *s);            /* Array dims as a finished --readFQB leaves them */
int  h10x_session_readFQB_mem(h10x_session *s, const uint32_t *records, uint64_t nRecords);
int  h10x_session_readFQB_dev(h10x_session *s, const uint32_t *devRecords, uint64_t nRecords);  /* records already in HBM */
int  h10x_session_readHash(h10x_session *s, const char *path);                        /* hash10x.c:1206-1211 */
int  h10x_session_writeHash(h10x_session *s, const char *path);                       /* hash10x.c:1212-1215 */
int  h10x_session_hashDepthRange(h10x_session *s, int min, int max);                  /* hash10x.c:1216-1219 */
int  h10x_session_cluster(h10x_session *s, int codeMin, int codeMax);                 /* hash10x.c:1241-1261 */
int  h10x_session_clusterSplit(h10x_session *s);                                      /* hash10x.c:1267 */

/* --hashStats / --codeStats (hash10x.c:351-402): the reference's histogram reports; the histograms are filled on the
   device (h10x_report_histogram), the text is the reference's, including its Array dim: hashDepth is histogrammed over
   arrayMax entries, index 0 included. f = NULL: take part without printing (ranks > 0 of a sharded session). */
int  h10x_session_hashStats(h10x_session *s, FILE *f);
int  h10x_session_codeStats(h10x_session *s, FILE *f);

/* --cribBuild <genome1.fa> <genome2.fa>, --clusterReport <codeMin> <codeMax>, --cribSummary (hash10x.c:470-521, 870-952,
   1017-1061): truth labels from two haplotype FASTAs (hashed and looked up on the device) and the reference's text
   reports. printTables = the --tables flag (CRIB_TABLE lines). The per-cluster figures come from the device
   (h10x_cluster_report); out = NULL: take part without printing (ranks > 0 of a sharded session). */
int  h10x_session_cribBuild(h10x_session *s, const char *fa1, const char *fa2, FILE *out, int printTables);
int  h10x_session_clusterReport(h10x_session *s, int codeMin, int codeMax, FILE *out);
/* after h10x_session_cluster(codeMin, codeMax): the reference's --verbose lines of those blocks (hash10x.c:827-834, 867) to out, its "too many clusters" notes
   (hash10x.c:813) to err; either may be null. Collective when sharded (rank 0 prints). */
int  h10x_session_clusterVerbose(h10x_session *s, int codeMin, int codeMax, FILE *out, FILE *err);
int  h10x_session_cribSummary(h10x_session *s, FILE *out);

/* the neighbour commands (hash10x.c:512-521, 541-718, 1220-1225, 1271-1272): --hashInfo <start> <end> <skip>, --hashExplore <hash>,
   --doubleShared <hash1> <hash2> print to out; --errorFix <hashMin> <hashMax> prints to out (the reference's stdout) and fails with
   "need to set crib" without one; --shareScan <countMin> <countMax> prints to out. The census runs on the device (h10x_neighbours /
   _max / _hist) in batches of bounded memory. Without --hashDepthRange each prints the reference's "<name> called without
   hashDepthRange" to err and returns 0; where the reference is undefined (ranges beyond hashNumber, skip <= 0, ...) they fail with a
   "!! ..." message. Single-GPU sessions only. */
int  h10x_session_hashInfo(h10x_session *s, int hMin, int hMax, int skip, FILE *out, FILE *err);
int  h10x_session_hashExplore(h10x_session *s, int x, FILE *out, FILE *err);
int  h10x_session_doubleShared(h10x_session *s, int x1, int x2, FILE *out, FILE *err);
int  h10x_session_errorFix(h10x_session *s, int hashMin, int hashMax, FILE *out, FILE *err);
int  h10x_session_shareScan(h10x_session *s, int countMin, int countMax, FILE *out, FILE *err);
/* --codeExplore <code> (hash10x.c:1226-1232, 1351-1470) with the session's -ct: re-clusters the barcode's good hashes on the device
   (h10x_code_explore), then prints its line, the COUNT_SHARE histogram, codeClusterReport's lines of the barcode and the SHARE lines
   to out, and the "too many clusters" note to err. Fails with "!! ..." before --hashDepthRange, for a code outside 0 .. nBlocks - 1,
   for -ct < 1, and — after everything else is printed and the state changed — without a crib. Single-GPU sessions only. */
int  h10x_session_codeExplore(h10x_session *s, int code, FILE *out, FILE *err);

/* --sortFQB <in.fqb> <out.fqb> (addition): the record sort the reference leaves to `bsort -k 4 -r 120` (README.md:26),
   on the device: records ordered by their first 4 bytes, stably */
int  h10x_session_sortFQB(h10x_session *s, const char *inPath, const char *outPath);

/* the barcode step between fq2b and --sortFQB, on the packed file and on the device (additions; include/h10x.h "barcode census"):
   --codeCensus <thresh> <in.fqb> <goodcodes> writes the barcodes (record word 0) that occur at least thresh times, one 16-letter line
   each, ascending by packed word — the README's `gzip -dc | perl | sort | uniq -c | awk` (README.md:44) — and one line of counts to out;
   --fixFQB <goodcodes> <in.fqb> <out.fqb> does to the records what `fq2b -10x <goodcodes>` does to the reads (fq2b.c:71-104, 157):
   drops those without a whitelist barcode within one substitution, corrects the others to the candidate of the latest whitelist
   line, and prints fq2b's lines to err; --fixFQBThresh <thresh> <in.fqb> <out.fqb> is both in one (README.md:62's `fq2b -10xThresh`),
   the whitelist never leaving the device. The file passes through in batches of "fqb_slab" records (h10x_session_set; 0 = 2^20):
   the host holds one batch. They fail for a size that is no multiple of 120, 2^32 or more records, thresh < 1, and a threshold no
   barcode reaches (or an empty whitelist: the reference reads an unallocated table then). out / err may be NULL. */
int  h10x_session_codeCensus(h10x_session *s, int thresh, const char *inPath, const char *goodPath, FILE *out);
int  h10x_session_fixFQB(h10x_session *s, const char *goodPath, const char *inPath, const char *outPath, FILE *err);
int  h10x_session_fixFQBThresh(h10x_session *s, int thresh, const char *inPath, const char *outPath, FILE *err);
/* the whitelist text without a device: the reader of fq2b-amd (blank-separated words of 16 characters; anything but ACGTacgt packs as A;
   codes in line order, to be freed with h10x_host_whitelist_free; -1 with "bad barcode line %d in %s: %s" or "failed to open 10x
   whitelist file %s" in err), the writer (one 16-letter line per code), and the line a barcode is looked up under — the LAST line
   that holds it, 0 = absent — which is what the device's set keeps (h10x_whitelist_set). The writer writes <path>.part and renames it when whole. */
int  h10x_host_whitelist_read(const char *path, uint32_t **codes, uint64_t *n, char *err, int errlen);
void h10x_host_whitelist_free(uint32_t *codes);
int  h10x_host_whitelist_write(const char *path, const uint32_t *codes, uint64_t n, char *err, int errlen);
int  h10x_host_whitelist_lines(const uint32_t *codes, uint64_t n, const uint32_t *query, uint64_t nq, uint32_t *lines);

/* the molecule of every read pair (additions; include/h10x.h "the molecule of every read pair"), after --cluster and before --clusterSplit:
   --moleculeMap <out.mol> writes a 32-byte header (magic "10XM", u32 version 1, u64 nRecords, u32 nBlocks, u32 nMolecules, u64 nClustered) and nRecords
   pairs {u32 mol, u32 slot} in the order of the sorted file the state was read from, and one line of counts to out;
   --splitFQB <in.fqb> <out.fqb> writes the records of in.fqb — that file — in split order (the whole image at once, as --sortFQB) and <out.fqb>.idx: magic
   "10XS", u32 version 1, u32 nBlocks, u32 nMolecules, then nBlocks + nMolecules + 1 u64 starts: the records of post-split block m are [start[m],
   start[m + 1]). A file with fewer records than the state was read from fails; records beyond them (a -N cut) are left out, with one line to out
   saying how many. Both fail without a state, on a sharded session and after --clusterSplit. All values little-endian. out may be NULL.
   h10x_host_write_molmap / _split_index write the two formats from arrays and never touch the GPU (-1 with the message in err). The .mol file and the
   .idx file are each written as <name>.part and renamed when whole: a failure leaves neither the file nor a .part. */
int  h10x_session_moleculeMap(h10x_session *s, const char *outPath, FILE *out);
int  h10x_session_splitFQB(h10x_session *s, const char *inPath, const char *outPath, FILE *out);
int  h10x_host_write_molmap(const char *path, const uint32_t *mol, const uint32_t *slot, const h10x_molmap_info *info, char *err, int errlen);
int  h10x_host_write_split_index(const char *path, const uint64_t *start, uint32_t nBlocks, uint32_t nMolecules, char *err, int errlen);

/* --shareGraph <minShare> <out.sg> (addition; include/h10x.h "the share graph"): for every block the blocks that share at least minShare of its
   good hashes, with the counts. The file, little-endian: magic "10XG", u32 version 1, u32 nBlocks, u32 minShare, u64 rows, nBlocks + 1 u64 offsets,
   then rows pairs {u32 block, u32 count}: the row of block c is pairs [offsets[c], offsets[c + 1]), ascending in block. The blocks are walked in
   ranges of "share_graph_blocks" (h10x_session_set; 0 = 8192) and the file is written range by range, so neither the host nor the device holds all
   rows; the result does not depend on it. One line of counts to out (may be NULL). Fails with "!! ..." (the command then does nothing) before
   --hashDepthRange, after --clusterSplit until a new range is set, and for minShare < 1; single-GPU sessions only. The file is written as <out.sg>.part
   and renamed when whole: in every failure no file is written and no .part is left behind.
   h10x_host_write_share_graph is the writer alone (no device): it asks the callback for the block ranges [c0, c1) of rangeBlocks blocks (0 = 8192) in
   ascending order; the callback yields the range's rows {blk, cnt} and part[0 .. c1 - c0], the row offsets of its blocks from 0 (0 = done, else failed).
   It returns -2 when the callback failed (err untouched), -1 with err set for its own failures; *rows (may be NULL) = all rows. */
typedef struct { const uint64_t *part; const uint32_t *blk, *cnt; uint64_t rows; } h10x_share_graph_range;
typedef int (*h10x_share_graph_range_fn)(void *user, uint32_t c0, uint32_t c1, h10x_share_graph_range *range);
int  h10x_session_shareGraph(h10x_session *s, int minShare, const char *outPath, FILE *out);
int  h10x_host_write_share_graph(const char *path, uint32_t nBlocks, uint32_t minShare, uint32_t rangeBlocks, h10x_share_graph_range_fn range, void *user,
                                 uint64_t *rows, char *err, int errlen);

/* --shareComponents <minShare> <out.sc> (addition; include/h10x.h "the components of the share graph"): the connected components of the share graph at
   minShare over all blocks — which blocks (after --clusterSplit: molecules) hang together through shared good hashes. The file, little-endian: magic
   "10XC", u32 version 1, u32 nBlocks, u32 minShare, u32 nComponents, u32 largest, u64 rows, then comp[nBlocks] as u32, then nComponents + 1 entries
   {u32 root, u32 blocks, u64 records} (entry 0 all zero). The blocks are walked in ranges of "share_graph_blocks" as --shareGraph walks them; each
   range's rows are folded into the labels on the device and never leave it; the result does not depend on the ranges. One line of counts to out (may
   be NULL). Fails with "!! ..." (the command then does nothing, no file is written) before --hashDepthRange, after --clusterSplit until a new range is
   set, and for minShare < 1; single-GPU sessions only.
   h10x_session_shareComponentsRun is the walk alone: the result stays in the context for h10x_share_components_get.
   h10x_host_write_share_components writes the file from host arrays (no device), as <out.sc>.part, renamed when whole: a failure leaves neither. */
int  h10x_session_shareComponents(h10x_session *s, int minShare, const char *outPath, FILE *out);
int  h10x_session_shareComponentsRun(h10x_session *s, int minShare, h10x_share_components_info *info);
int  h10x_host_write_share_components(const char *path, const h10x_share_components_info *info, const uint32_t *comp, const uint32_t *rootOf,
                                      const uint32_t *blocks, const uint64_t *records, char *err, int errlen);

/* --hashCopies <minShare> <out.hc> (addition; include/h10x.h "the per-hash linkage groups"): for every hash in the depth range the linkage groups of the
   blocks that hold it — one group for a hash at one locus, two that do not link for a hash at two. The file, little-endian: magic "10XK", u32 version 1,
   u32 hashNumber, u32 minShare, u64 inRange, u64 rows, then hashNumber records {u16 distinct, u16 groups, u16 largest, u16 second} (zeros outside the
   range and at index 0), written in slabs of 2^22 hashes. One line of counts to out (may be NULL) and, with a crib, five lines
   "HASH_COPIES  <err|htA|htB|hom|mul> n <in range> one <groups == 1> split <second >= 2>". Fails with "!! ..." (the command then does nothing, no file
   is written) before --hashDepthRange, after --clusterSplit until a new range is set, for minShare < 1 and when an in-range hash is deeper than 4096;
   single-GPU sessions only.
   h10x_session_hashCopiesRun is the run alone: the result stays in the context for h10x_hash_copies_get.
   h10x_host_write_hash_copies writes the file from a callback that fills records [first, first + count) (no device); slabHashes = 0: 2^22. It returns
   -2 when the callback failed (err untouched), -1 with err set for its own failures. The file is written as <out.hc>.part and renamed when whole: in
   every failure no file is written and no .part is left behind. */
typedef int (*h10x_hash_copies_slab_fn)(void *user, uint16_t *out, uint64_t first, uint64_t count);
int  h10x_session_hashCopies(h10x_session *s, int minShare, const char *outPath, FILE *out);
int  h10x_session_hashCopiesRun(h10x_session *s, int minShare, h10x_hash_copies_info *info);
int  h10x_host_write_hash_copies(const char *path, const h10x_hash_copies_info *info, h10x_hash_copies_slab_fn slab, void *user, uint64_t slabHashes,
                                 char *err, int errlen);

/* --seqBlocks <minShare> <seqfile> <out.sb> (addition; include/h10x.h "from a sequence to its blocks"): per sequence of a FASTA / FASTQ file (gzip or
   plain) the blocks that stand at least minShare times in the barcode lists of its in-range hashes. The file is read through h10x_seq_next_named in
   slabs of "seq_slab" bases (h10x_session_set; 0 = 2^26; a longer sequence goes alone), each slab runs through h10x_seq_blocks_run and its rows are
   appended to the file at once, so neither the host nor the device holds all rows; the per-sequence table and the names stay on the host until the end.
   The file is written as <out.sb>.part and renamed when whole. Little-endian: "10XQ", u32 version 1, u32 nBlocks, u32 minShare, u64 nSeq, u64 rows,
   u64 nameBytes (filled in at the end); rows pairs {u32 block, u32 count}; nSeq records {u64 len, u32 moshes, u32 found, u32 query, u32 0};
   nSeq + 1 u64 offsets; nSeq + 1 u64 name offsets; the names, NUL-terminated, cut at the first blank or tab.
   out gets one line of counts; verbose != 0 adds one SEQ_BLOCKS line per sequence: name, len, moshes, found, query, rows, the block of the largest
   count (lowest on ties; 0 without rows) and that count. Soft errors as --shareGraph: no state or no range ("!! you must set hashDepthRange before
   seqBlocks"), "!! seqBlocks minShare 0 must be >= 1"; a sequence file or an output path that cannot be opened fails without "!!". In every failure no
   file is written and no .part is left behind.
   h10x_host_write_seq_blocks is the writer alone, fed by a callback that yields one slab after the other (1 = a slab, 0 = no more, < 0 = failed); it
   returns -2 when the callback failed (err untouched), -1 with err set for its own failures. */
typedef struct {
  uint32_t nSeq;
  const uint64_t *seqStart;                  /* nSeq + 1: sequence s has seqStart[s + 1] - seqStart[s] bases */
  const h10x_seq_figures *fig;               /* nSeq */
  const uint64_t *rowOff;                    /* nSeq + 1: the slab's rows, from 0 */
  const uint32_t *block, *count;             /* rowOff[nSeq] each */
  const char *names; const uint64_t *nameOff;   /* sequence s is called names + nameOff[s] */
} h10x_seq_blocks_slab;
typedef struct { uint64_t nSeq, bases, moshes, found, query, rows, withRows; uint32_t maxCount, reserved; } h10x_seq_blocks_totals;
typedef int (*h10x_seq_blocks_slab_fn)(void *user, h10x_seq_blocks_slab *slab);
int  h10x_host_write_seq_blocks(const char *path, uint32_t nBlocks, uint32_t minShare, h10x_seq_blocks_slab_fn next, void *user, FILE *verbose,
                                h10x_seq_blocks_totals *totals, char *err, int errlen);
int  h10x_session_seqBlocks(h10x_session *s, int minShare, const char *seqPath, const char *outPath, FILE *out, int verbose);

/* --seqLinks <minShare> <minBlocks> <endLen> <maxEnds> <seqfile> <out.sl> (addition; include/h10x.h "row links"): which ends of the sequences of a FASTA /
   FASTQ file are covered by the same blocks: after --clusterSplit and a new range, by the same molecules. Sequence s (0-based, file order) gives end 2s, its
   first min(len, endLen) bases, and end 2s + 1, its last min(len, endLen) bases, each hashed as a sequence of its own; endLen 0 makes end 2s the whole
   sequence and end 2s + 1 empty. The row of an end is its --seqBlocks row at minShare; ends e < f are linked when they share at least minBlocks blocks that
   stand in at most maxEnds ends (0 = no cap); the two ends of one sequence are never linked. The file is read in slabs of "seq_slab" bases; a slab of ends
   runs through h10x_seq_blocks_run and h10x_row_links_add_kept, so the rows never reach the host: the device holds 8 bytes per row entry of the whole
   file, the host per sequence its length, its two row counts and its name. h10x_row_links_finish runs once at the end and the links come back in pieces.
   The file is written as <out.sl>.part and renamed when whole. Little-endian: "10XL", u32 version 1, u32 nBlocks, u32 minShare, u32 minBlocks, u32 endLen,
   u32 maxEnds, u32 0, u64 nSeq, u64 links, u64 skippedBlocks, u64 nameBytes; nSeq records {u64 len, u32 headRows, u32 tailRows}; 2 nSeq + 1 u64 offsets;
   links pairs {u32 end, u32 shared}: the row of end e at [offsets[e], offsets[e + 1]), ends f > e ascending; nSeq + 1 u64 name offsets; the names,
   NUL-terminated, cut at the first blank or tab.
   out gets one line of counts; verbose != 0 adds one line per link, "SEQ_LINKS  <nameA> <H|T> <nameB> <H|T> shared c". Soft errors as --seqBlocks: no state
   or no range ("!! you must set hashDepthRange before seqLinks"), "!! seqLinks minShare 0 must be >= 1" and likewise minBlocks (>= 1), endLen and maxEnds
   (>= 0); a sequence file or an output path that cannot be opened fails without "!!"; 2^31 or more sequences are refused. In every failure no file is
   written and no .part is left behind.
   h10x_host_write_seq_links is the writer alone: the tables come ready in the head, the links through a callback that fills other[] / shared[] with links
   [first, first + count) (0 = done, < 0 = failed), at most pieceLinks at a time (0 = 2^20). It returns -2 when the callback failed (err untouched), -1
   with err set for its own failures. */
typedef struct { uint64_t len; uint32_t headRows, tailRows; } h10x_seq_links_rec;
typedef struct {
  uint32_t nBlocks, minShare, minBlocks, endLen, maxEnds;
  uint64_t nSeq, links, skippedBlocks;
  const h10x_seq_links_rec *table;           /* nSeq */
  const uint64_t *offsets;                   /* 2 nSeq + 1, from 0 to links */
  const char *names; const uint64_t *nameOff;   /* nSeq + 1: sequence s is called names + nameOff[s], nameOff[nSeq] = the bytes of all names */
} h10x_seq_links_head;
typedef struct { uint64_t nSeq, links, withLinks, pieces; uint32_t maxShared, reserved; } h10x_seq_links_totals;
typedef int (*h10x_seq_links_piece_fn)(void *user, uint64_t first, uint64_t count, uint32_t *other, uint32_t *shared);
int  h10x_host_write_seq_links(const char *path, const h10x_seq_links_head *head, h10x_seq_links_piece_fn piece, void *user, uint64_t pieceLinks, FILE *verbose,
                               h10x_seq_links_totals *totals, char *err, int errlen);
int  h10x_session_seqLinks(h10x_session *s, int minShare, int minBlocks, int endLen, int maxEnds, const char *seqPath, const char *outPath, FILE *out, int verbose);

/* --seqSpans <minShare> <maxGap> <window> <minCover> <seqfile> <out.ss> (addition; include/h10x.h "sequence spans"): per sequence of a FASTA / FASTQ file the
   extents {block, first, last, hits} of the blocks on it (hits of one block no more than maxGap apart, maxGap 0: one extent per block; kept at minShare hits)
   and, for window >= 1, the number of kept extents that span each boundary j * window: after --clusterSplit and a new range, the molecules over each position.
   A boundary with cover < minCover is weak. The file is read in slabs of "seq_slab" bases as --seqBlocks reads it; each slab runs through h10x_seq_spans_run
   and its extents are appended to the file at once; the host keeps per sequence a record, the name and the coverage (4 bytes per boundary) until the end.
   The file is written as <out.ss>.part and renamed when whole. Little-endian: "10XE", u32 version 1, u32 nBlocks, u32 minShare, u32 maxGap, u32 window,
   u32 minCover, u32 0, u64 nSeq, u64 extents, u64 boundaries, u64 nameBytes (filled in at the end); extents records {u32 block, u32 first, u32 last, u32 hits};
   nSeq records {u64 len, u32 moshes, u32 found, u32 inRange, u32 weak}; nSeq + 1 u64 offsets; nSeq + 1 u64 cover offsets; boundaries u32 cover; nSeq + 1 u64
   name offsets; the names, NUL-terminated, cut at the first blank or tab.
   out gets one line of counts; verbose != 0 adds per sequence "SEQ_SPANS  <name> len l moshes m found f inRange q extents e boundaries B weak w" and, per
   maximal run of consecutive weak boundaries, "SEQ_WEAK  <name> from <first position> to <last position> min <lowest cover>". Soft errors as --seqBlocks: no
   state or no range ("!! you must set hashDepthRange before seqSpans"), "!! seqSpans minShare 0 must be >= 1", and maxGap, window and minCover "must be >= 0";
   a sequence file or an output path that cannot be opened fails without "!!". In every failure no file is written and no .part is left behind.
   h10x_host_write_seq_spans is the writer alone, fed by a callback as h10x_host_write_seq_blocks is, with the same return values. */
typedef struct { uint32_t nBlocks, minShare, maxGap, window, minCover; } h10x_seq_spans_head;
typedef struct {
  uint32_t nSeq;
  const uint64_t *seqStart;                  /* nSeq + 1: sequence s has seqStart[s + 1] - seqStart[s] bases */
  const h10x_seq_span_figures *fig;          /* nSeq */
  const uint64_t *rowOff;                    /* nSeq + 1: the slab's extents, from 0 */
  const uint32_t *block, *first, *last, *hits;   /* rowOff[nSeq] each */
  const uint64_t *coverOff;                  /* nSeq + 1: the slab's boundaries, from 0 */
  const uint32_t *cover;                     /* coverOff[nSeq] */
  uint64_t gathered;                         /* the hits the slab's run gathered (the summary line) */
  const char *names; const uint64_t *nameOff;   /* sequence s is called names + nameOff[s] */
} h10x_seq_spans_slab;
typedef struct { uint64_t nSeq, bases, moshes, found, inRange, hits, extents, sumSpan, boundaries, weak; uint32_t maxSpan, maxHits; } h10x_seq_spans_totals;
typedef int (*h10x_seq_spans_slab_fn)(void *user, h10x_seq_spans_slab *slab);
int  h10x_host_write_seq_spans(const char *path, const h10x_seq_spans_head *head, h10x_seq_spans_slab_fn next, void *user, FILE *verbose,
                               h10x_seq_spans_totals *totals, char *err, int errlen);
int  h10x_session_seqSpans(h10x_session *s, int minShare, int maxGap, int window, int minCover, const char *seqPath, const char *outPath, FILE *out, int verbose);

/* --seqSpectrum <copy1min> <copy2min> <copyMmin> <window> <seqfile> <out.sp> (addition; include/h10x.h "sequence spectrum"): the moshes of every sequence of a
   FASTA / FASTQ file classed by the read depth of their hash (absent; copy0 below copy1min; copy1; copy2; copyM from copyMmin), per sequence and, for window >= 1,
   per window of that many bases; how many times the sequences hold every hash of the state; and the depth x copies matrix with the hashes of each class that the
   sequences hold at all. It needs no depth range. The file is read in slabs of "seq_slab" bases as --seqBlocks reads it; each slab runs through
   h10x_seq_spectrum_add and its window records are appended to the file at once; the host keeps per sequence the 40-byte record, one offset and the name.
   The file is written as <out.sp>.part and renamed when whole. Little-endian: "10XP", u32 version 1, u32 hashNumber, u32 copy1min, u32 copy2min, u32 copyMmin,
   u32 window, u32 depthBins (1024), u32 copyBins (8), u32 0, u64 nSeq, u64 windows, u64 nameBytes (filled in at the end); windows records {u32 moshes, absent,
   n0, n1, n2, nM; u64 depthSum}; nSeq records {u64 len; u32 moshes, absent, n0, n1, n2, nM; u64 depthSum}; nSeq + 1 u64 window offsets; 8 u64 totals
   (total[4], present[4]); depthBins x copyBins u64 spectrum, row = depth bin; hashNumber bytes min(copies[x], 255), byte 0 = 0; nSeq + 1 u64 name offsets; the
   names, NUL-terminated, cut at the first blank or tab.
   out gets "  seq spectrum at copy1min a copy2min b copyMmin c, window W: n sequences, b bases, m moshes, x absent, copy0 p copy1 q copy2 r copyM s, QV v,
   present h1 of t1 copy1, h2 of t2 copy2, hM of tM copyM, completeness z %"; QV = h10x_host_qv(moshes, absent + copy0, k), completeness = 100 (h1 + h2 + hM) /
   (t1 + t2 + tM), 0 without such hashes. verbose != 0 adds per sequence "SEQ_SPECTRUM  <name> len l moshes m absent x copy0 p copy1 q copy2 r copyM s meanDepth
   %.1f QV %.2f" (meanDepth over the found occurrences, 0.0 without any). Soft errors: no state ("!! seqSpectrum: no hash state loaded ..."), "!! seqSpectrum
   needs 0 <= copy1min <= copy2min <= copyMmin", "!! seqSpectrum window -1 must be >= 0"; a sequence file or an output path that cannot be opened fails without
   "!!". In every failure no file is written and no .part is left behind.
   h10x_host_write_seq_spectrum is the writer alone: `next` gives one slab per call (1, 0 at the end, < 0 on its own error), `end` the totals and the spectrum
   once the last slab is in, `copies` copies[first .. first + count) in pieces of at most 2^22; 0, -1 with err set, or -2 when a callback failed (err untouched).
   h10x_host_qv: -10 log10(1 - (1 - unsupported / moshes)^(1 / k)); infinity when nothing is unsupported, 0 without moshes. */
typedef struct { uint32_t hashNumber, copy1min, copy2min, copyMmin, window; int k; } h10x_seq_spectrum_head;
typedef struct {
  uint32_t nSeq;
  const h10x_seq_spectrum_figures *fig;      /* nSeq */
  const uint64_t *winOff;                    /* nSeq + 1: the slab's windows, from 0 */
  const h10x_seq_spectrum_window *win;       /* winOff[nSeq] */
  const char *names; const uint64_t *nameOff;   /* sequence s is called names + nameOff[s] */
} h10x_seq_spectrum_slab;
typedef struct { uint64_t nSeq, bases, moshes, absent, n0, n1, n2, nM, depthSum, windows, total[4], present[4]; } h10x_seq_spectrum_totals;
typedef int (*h10x_seq_spectrum_slab_fn)(void *user, h10x_seq_spectrum_slab *slab);
typedef int (*h10x_seq_spectrum_end_fn)(void *user, uint64_t *spectrum, uint64_t *totals);
typedef int (*h10x_seq_spectrum_copies_fn)(void *user, uint64_t first, uint64_t count, uint32_t *out);
double h10x_host_qv(uint64_t moshes, uint64_t unsupported, int k);
int  h10x_host_write_seq_spectrum(const char *path, const h10x_seq_spectrum_head *head, h10x_seq_spectrum_slab_fn next, h10x_seq_spectrum_end_fn end,
                                  h10x_seq_spectrum_copies_fn copies, void *user, FILE *verbose, h10x_seq_spectrum_totals *totals, char *err, int errlen);
int  h10x_session_seqSpectrum(h10x_session *s, int copy1min, int copy2min, int copyMmin, int window, const char *seqPath, const char *outPath, FILE *out, int verbose);

/* --writeMosh <bits> <copy1min> <copy2min> <copyMmin> <out.mosh> (addition; include/h10x.h "the state as a mosh set"): the in-range hashes of the state as
   an MSHSTv1 file that moshutils, moshasm and moshmap read: the state's hash values, depths saturated to 16 bits, copy classes from depth by the three
   thresholds of moshutils -s and, where a --hashCopies result is kept, corrected by linkage. bits = the table bits of the set, 0 = the state's -B. The file
   is written as <out.mosh>.part and renamed when it is whole. The figures of the set to info (may be NULL), one line to out (may be NULL),
     "  mosh set of N hashes in range, bits B: copy0 a copy1 b copy2 c copyM d, by linkage at minShare T: x to M, y to 0"   (or ", by depth only"),
   with ", n depths cut to 65535" when depths saturated, and with a crib five lines "WRITE_MOSH  <err|htA|htB|hom|mul> copy0 a copy1 b copy2 c copyM d".
   Fails with "!! ..." (the command then does nothing, no file is written) before --hashDepthRange, after --clusterSplit until a new range is set, for
   thresholds that do not ascend and for bits outside 0, 20 .. 34; single-GPU sessions only.
   h10x_session_moshSet is the build alone: *set is the caller's to use and destroy. h10x_host_print_state_mosh prints the lines (no device). */
int  h10x_session_writeMosh(h10x_session *s, int bits, int copy1min, int copy2min, int copyMmin, const char *outPath, FILE *out, h10x_state_mosh_info *info);
int  h10x_session_moshSet(h10x_session *s, int bits, int copy1min, int copy2min, int copyMmin, h10x_mosh **set, h10x_state_mosh_info *info);
void h10x_host_print_state_mosh(FILE *out, const h10x_state_mosh_info *info, int withCrib);

/* multi-GPU (include/h10x.h "multi-GPU"): one session per rank, each holding a contiguous barcode range of the sorted file
   (cut with h10x_host_partition / _partition_file; -N is applied by the launcher before cutting). Every command of a
   sharded session is collective: all ranks call it with the same arguments; the text commands print on the rank whose
   FILE* is not NULL (rank 0) and only take part on the others. --writeHash, --clusterSplit, --cribBuild and the reports
   work on the shards as they are (no gather): see h10x.h. _file streams this rank's records [first, first + n) of the
   file into HBM and applies the reference's chunk semantics (-c) over the whole file. shardGather turns rank 0 into a
   single-GPU session holding everything (for continuing on one GPU). */
int  h10x_session_shardReadFQB_mem(h10x_session *s, h10x_comm *comm, const uint32_t *shardRecords, uint64_t nRecords);
int  h10x_session_shardReadFQB_dev(h10x_session *s, h10x_comm *comm, const uint32_t *devShardRecords, uint64_t nRecords);
int  h10x_session_shardReadFQB_file(h10x_session *s, h10x_comm *comm, const char *path, uint64_t firstRecord, uint64_t nRecords);
int  h10x_session_shardReadHash(h10x_session *s, h10x_comm *comm, const char *path);      /* --readHash: every rank reads its cut of the blocks */
int  h10x_session_shardGather(h10x_session *s);

/* dimension the reference's Array reaches when elements are first touched in ascending order up to
   lastIndex, starting from initialDim (array.c:144-185) */
int  h10x_host_array_dim(int initialDim, int elemSize, int64_t lastIndex);
/* test hook: what the reference's HASH object (hash.c) counts after hashAdd(HASH_INT(key)) of these keys — the restatement behind --cribSummary's second figures */
int  h10x_host_refhash_count(const int32_t *keys, uint64_t n);
/* readFQB's chunk loop (hash10x.c:202-223) replayed on the barcode column: returns the number of
   records it would consume (honours -N), or -1 with "chunkSize too small" in err */
int64_t h10x_host_check_chunks(const uint32_t *records, uint64_t nRecords, int N, int chunkSize, char *err, int errlen);

/* contiguous barcode-range shards for nParts GPUs: cut[g] = first record of shard g, always on a
   barcode-run boundary, balanced by record count; cut[nParts] = nRecords. Returns 0. */
int  h10x_host_partition(const uint32_t *records, uint64_t nRecords, int nParts, uint64_t *cut);
/* the same cuts for the first nRecords records of a file, reading only the barcode words around each cut */
int  h10x_host_partition_file(const char *path, uint64_t nRecords, int nParts, uint64_t *cut, char *err, int errlen);

/* starts loading the library's device code for `device` on a thread of its own (once per process and device; --readFQB joins it before its first kernels) */
void h10x_host_warm_start(int device);
/* ---- moshutils-amd (mosh_host.c): sequence files, MSHSTv1 files and the file-level commands over h10x_mosh_* ----
   Sequence reader (seqio.c:15-190 for FASTA / FASTQ, gzip or plain; needs no device). h10x_seq_open: NULL on failure with msg = the
   reference's stderr line ("sequence file %s unreadable or empty", "... is unknown type"; empty when the file cannot be opened) and
   *fatal = 1 where this program stops instead (seqio's binary format). h10x_seq_next reads whole sequences until slabBases bases are
   in (0 = 2^26): codes = one byte per base (A C G T N, either case -> 0 1 2 3 0), sequence s = codes[seqStart[s] .. seqStart[s+1]);
   1 = sequences delivered, 0 = end of file, -1 = fatal (h10x_seq_error: the reference's die texts, "bad base 0x.. in FASTQ line n").
   The arrays of one call stay valid until the call after the next returns. h10x_seq_warning: "incomplete sequence record line n" once
   the file has ended inside a record (that record is dropped, seqio.c:91-95). */
typedef struct h10x_seqreader h10x_seqreader;
h10x_seqreader *h10x_seq_open(const char *path, char *msg, int msglen, int *fatal);
int  h10x_seq_next(h10x_seqreader *r, uint64_t slabBases, const uint8_t **codes, const uint64_t **seqStart, uint32_t *nSeq);
/* the same with the names: sequence s is called names + nameOff[s], the header up to its first blank or tab (readseq.c:82-88) */
int  h10x_seq_next_named(h10x_seqreader *r, uint64_t slabBases, const uint8_t **codes, const uint64_t **seqStart, uint32_t *nSeq, const char **names, const uint64_t **nameOff);
const char *h10x_seq_error(const h10x_seqreader *r);
const char *h10x_seq_warning(const h10x_seqreader *r);
void h10x_seq_totals(const h10x_seqreader *r, uint64_t *nSeq, uint64_t *bases);
void h10x_seq_close(h10x_seqreader *r);
/* == Seqhash as seqhashWrite stores it (seqhash.h:15-22, 72 bytes, no padding holes) */
typedef struct { int32_t k, w; uint64_t mask; int32_t shift1, shift2; uint64_t factor1, factor2, patternRC[4]; } h10x_seqhash_rec;
/* a parsed MSHSTv1 file (moshset.c:78-103): index 2^B entries, value / depth / info `size` = max + 1 entries. The reader refuses a
   file whose entries are not each found through their own probe walk (so the values are distinct: h10x_mosh_merge relies on it). */
typedef struct { int32_t B; uint32_t size; h10x_seqhash_rec sh; uint32_t *index; uint64_t *value; uint16_t *depth; uint8_t *info; } h10x_moshfile;
int  h10x_moshfile_read(const char *path, h10x_moshfile *out, char *err, int errlen);
void h10x_moshfile_free(h10x_moshfile *m);
void h10x_moshfile_counts(const h10x_moshfile *m, uint32_t *hist65536, uint32_t copy4[4]);
/* moshsetSummary's text (moshset.c:122-144) from the counts; with max = 0 the line ends without a newline, as in the reference */
void h10x_mosh_summary_print(FILE *f, int k, int w, int B, uint32_t max, const uint32_t *hist65536, const uint32_t *copy4);
int  h10x_mosh_set_summary(h10x_mosh *set, FILE *f);
int  h10x_mosh_set_write(h10x_mosh *set, const char *path, char *err, int errlen);                     /* moshsetWrite */
/* addSequenceFile (moshutils.c:32-50): 0 = done, 1 = the file could not be opened (msg = line for stderr, may be empty), -1 = fatal */
int  h10x_mosh_set_add_file(h10x_mosh *set, const char *path, int is10x, uint64_t slabBases, uint64_t *nSeq, uint64_t *totLen, uint64_t *totHash,
                            char *msg, int msglen, char *warn, int warnlen);
/* ---- moshasm-amd (asm_host.c): the RSMSHv2 file, the text reports and the file-level commands over h10x_readset_* ----
   a parsed RSMSHv2 file (moshasm.c:84-123): `max` records, hit / dx of all reads back to back. The reader checks the header, the record
   size, max <= dim, that the hit counts fit the file and that every mosh index lies in 1 .. setMax; it fails with a message. */
typedef struct { uint64_t totHit; uint32_t dim, max; h10x_read_t *reads; uint32_t *hit; uint16_t *dx; } h10x_readsetfile;
int  h10x_readsetfile_read(const char *path, uint32_t setMax, h10x_readsetfile *out, char *err, int errlen);
void h10x_readsetfile_free(h10x_readsetfile *r);
int  h10x_readsetfile_write(const char *path, uint64_t totHit, uint32_t dim, const h10x_read_t *reads, uint32_t nReads, const uint64_t *hitStart,
                            const uint32_t *hit, const uint16_t *dx, char *err, int errlen);
int  h10x_readset_write_file(h10x_readset *rs, const char *path, char *err, int errlen);                /* the .readset half of readsetWrite */
/* the loop of readsetFileRead: 0 = done, 1 = the file could not be opened (msg = line for stderr, may be empty), -1 = fatal */
int  h10x_readset_add_file(h10x_readset *rs, const char *path, uint64_t slabBases, char *msg, int msglen, char *warn, int warnlen);
int  h10x_readset_print_stats(h10x_readset *rs, h10x_mosh *set, FILE *f, char *err, int errlen);        /* 1 = empty readset */
int  h10x_readset_print_overlaps(h10x_readset *rs, uint32_t ix, int level, FILE *f, h10x_overlap_t **olap, uint32_t *nOlap, char *err, int errlen);
int  h10x_readset_print_pair(h10x_readset *rs, h10x_mosh *set, uint32_t ix, uint32_t iy, FILE *f, char *err, int errlen);
int  h10x_readset_print_assembly(h10x_readset *rs, h10x_mosh *set, uint32_t ix, FILE *f, FILE *fstd, char *err, int errlen);
/* ---- moshmap-amd (map_host.c): the name dictionary, the RFMSHv1 file, the Q / M / -v texts and the file-level commands over h10x_refmap_* ----
   h10x_namedict: the reference's DICT (dict.c): names numbered from 0 in order of arrival behind a probe table of 2^dim entries that
   doubles when max > 0.3 * size. table[] holds index + 1; names[1 .. max]. */
typedef struct { int32_t dim, max, size; int32_t *table; char **names; } h10x_namedict;
h10x_namedict *h10x_namedict_create(int size);
void h10x_namedict_destroy(h10x_namedict *d);
int  h10x_namedict_add(h10x_namedict *d, const char *s, int *ip);           /* 1 = added, 0 = already there, -1 = out of memory */
int  h10x_namedict_find(const h10x_namedict *d, const char *s, int *ip);
const char *h10x_namedict_name(const h10x_namedict *d, uint32_t i);
/* a parsed RFMSHv1 file (moshmap.c:135-181): index / offset / id / rev of max entries, depth / loc of setMax + 1, the lengths (an Array of
   lenDim entries, lenMax used) and the names. The reader fails with a message unless: the header is right, size == max, every array fits
   the file, index <= setMax, id < names, loc is the running sum of depth and ends within max, rev < max, the dict's dim is 10 .. 30 and
   holds its names, every name fits the file. */
typedef struct { uint32_t max, setMax; uint32_t *index, *offset, *id, *depth, *rev, *loc; int32_t lenDim, lenMax; uint32_t *len; h10x_namedict *dict; } h10x_reffile;
int  h10x_reffile_read(const char *path, uint32_t setMax, h10x_reffile *out, char *err, int errlen);
int  h10x_reffile_write(const char *path, const h10x_reffile *r, char *err, int errlen);
int  h10x_reffile_set_len(h10x_reffile *r, uint32_t id, uint32_t len);        /* array(ref->len, id, int) = len with arrayExtend's growth */
void h10x_reffile_free(h10x_reffile *r);
void h10x_map_print_q(FILE *f, const char *name, int len, const uint32_t counts4[4]);
void h10x_map_print_m(FILE *f, const char *name, int len, const h10x_maprec_t *m, const char *refName, uint32_t off0, uint32_t offN, uint32_t copy1);
void h10x_map_print_seed(FILE *f, uint32_t pos, int copyClass, const char *name1, uint32_t off1, const char *name2, uint32_t off2);
/* a Reference on the device with its names and lengths */
typedef struct { h10x_refmap *rm; h10x_namedict *dict; uint32_t *len; int32_t lenDim, lenMax; } h10x_mapref;
int  h10x_mapref_from_fasta(h10x_mapref **out, h10x_mosh *set, uint32_t size, const char *path, uint64_t slabBases, FILE *outFile, char *msg, int msglen);
int  h10x_mapref_from_file(h10x_mapref **out, h10x_mosh *set, h10x_reffile *rf, char *msg, int msglen);   /* takes rf's names and lengths */
int  h10x_mapref_write_file(h10x_mapref *r, const char *path, char *err, int errlen);
int  h10x_mapref_query_file(h10x_mapref *r, const char *path, uint64_t slabBases, int verbose, FILE *f, FILE *fverbose, char *msg, int msglen);
void h10x_mapref_destroy(h10x_mapref *r);

#ifdef __cplusplus
}
#endif
#endif
