/* h10x.h — C ABI of libh10x_hip.so: the MI355X (gfx950) implementation of hash10x's
 * mosh-construction + per-barcode clustering path.
 *
 * The reference (richarddurbin/hash10x) has no library/FFI boundary: its seams are global-state C
 * functions called from main()'s argv loop (hash10x.c:1158-1279). Each entry point below replaces
 * one of those seams and cites it. A maintainer of the reference would call these from the same
 * places in hash10x.c (see INTEGRATION.md for the exact stub); our own C host program
 * (hash10x_amd/host/hash10x_main.c) does exactly that behind the reference's command surface.
 *
 * Conventions: every function returns 0 on success, non-zero on failure; h10x_last_error() then
 * returns the message — the reference's own die() text (utils.c:18-29) where the reference would
 * have died (e.g. "hashTableSize is too small"). Plain pointers and sizes only; host pointers are
 * caller-owned; device memory is owned by the context. One host thread per context (the reference
 * is single-threaded at this boundary; its OMP loop lives inside --cluster, as our kernels do).
 * There is NO CPU fallback: without a HIP device h10x_create() fails.
 */
#ifndef H10X_H
#define H10X_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): h10x_warm, h10x_alloc_stats, h10x_pinned_*, h10x_ingest_fqb_async / _wait, H10X_TABLE_CLUSTER_RAW, the exchange counters of
   h10x_counters; option "cluster_dbg_skip" gone.
   3: h10x_counters.shard_reply_path, options "shard_reply_sort" 2 .. 4 and "shard_owner_cut". Entry points added since (the census, share graph, components,
   hash copies, mosh sets, readsets, reference maps, h10x_mosh_from_state, h10x_seq_hashes / h10x_list_share_* / h10x_seq_blocks_run, h10x_row_links_*,
   h10x_mosh_counters, h10x_get_scan_retries, h10x_readset_chunks) change no existing struct or table and leave the version alone.
   libh10x_host.so and the Python loader refuse a libh10x_hip.so of another version. */
#define H10X_ABI_VERSION 3

typedef struct h10x_ctx h10x_ctx;

/* hasher + table parameters latched by -k -w -r -B (hash10x.c:1131-1134, 1174-1177) */
typedef struct {
  int32_t  k;          /* k-mer length, 1..31                      (seqhash.c:24)            */
  int32_t  w;          /* mosh modulus, >= 1                       (seqhash.c:25) */
  int32_t  B;          /* hash index table bits, 20..30            (hash10x.c:1107-1108)     */
  int32_t  reserved;
  uint64_t factor1;    /* multiplier of hashFunc (seqhash.c:29,58-59): h10x_factor1_from_seed(r) */
} h10x_params;

/* == ClusterBlock (hash10x.c:62-70), 32 bytes; clusHash is a heap pointer in the reference and is
   always written as 0 by this library (canonical form) */
typedef struct {
  uint32_t nRead, nHash, nSubCluster, clusterParent;
  uint64_t clusHash;
  double   pointToMin;
} h10x_block;

/* == ClusterHash (hash10x.c:35-43), 8 bytes */
typedef struct {
  uint32_t hash;        /* hash INDEX (1-based, first-appearance order) */
  uint16_t read;
  uint8_t  subCluster;
  uint8_t  flags;       /* isHet:1 isHom:1 isErr:1 isSure:1 — never set on this path */
} h10x_clushash;

typedef struct {
  int32_t  B;
  uint32_t hashNumber;  /* number of distinct hashes + 1 (index 0 unused)   (hash10x.c:90)  */
  uint32_t nBlocks;     /* arrayMax(clusterBlocks) = barcodes + 1           (hash10x.c:96)  */
  uint32_t reserved;
  uint64_t nClusHash;   /* sum of nHash over blocks                                          */
  uint64_t nRecords;    /* read pairs consumed by the last read_fqb                          */
} h10x_sizes;

/* srandom(seed); (random() << 32) | random() | 1 — glibc, as seqhashCreate draws it after
   initialise() seeds the generator (hash10x.c:1101, seqhash.c:29). Host-side helper. */
uint64_t h10x_factor1_from_seed(int32_t seed);

int  h10x_abi_version(void);
/* "src:<first 16 hex digits of the sha256 over the .hip and .hpp files of csrc (sorted by name) and this header>": what this library
   was built from (measurements record it; tests compare it with the sources of the tree they run in) */
const char *h10x_build_id(void);
/* number of HIP devices visible (0 if none / no driver); never initialises a context */
int  h10x_device_count(void);

/* replaces initialise() (hash10x.c:1099-1118). device = HIP ordinal; stream = hipStream_t to launch
   on, or NULL for the device's default stream. Fails (no fallback) if the device is unusable or the
   parameters would make the reference die. err/errlen receive the message when *ctx stays NULL. */
int  h10x_create(h10x_ctx **ctx, const h10x_params *p, int device, void *stream, char *err, int errlen);
void h10x_destroy(h10x_ctx *ctx);
const char *h10x_last_error(const h10x_ctx *ctx);

/* replaces readFQB() + fillHashTable() (hash10x.c:188-236, 317-347) for a whole sorted .fqb image:
   n_records records of 30 uint32 (fq2b.c:142-160). Barcode blocks are runs of equal word 0; the
   block still open at the end is kept with nHash = 0 (hash10x.c:209). The caller applies
   -N (pass only the first N records). The side effects of the reference's chunked fread loop (hash10x.c:202-223:
   die("chunkSize too small") for a barcode of chunkSize or more pairs, and the all-A barcode swallowing the next run
   when its own run ends at a chunk boundary, hash10x.c:212) are replayed from the barcode run starts when
   h10x_set_option(ctx, "chunk_size", c) was called with c > 0 (the session layer passes -c); 0 = no chunk semantics.
   _device: records already resident in device memory (HBM). */
/* Both return once the last launches are queued (every size the host needs has been read back by then): the next call on the
   context waits for them, and a device fault in them is reported there. */
int  h10x_read_fqb(h10x_ctx *ctx, const uint32_t *host_records, uint64_t n_records);
/* The same in chunks, as the reference's loop reads the file (hash10x.c:202-223: fread of chunkSize records at a time): every call
   appends n_records records to the context's record image ON THE DEVICE (the chunk buffer is the caller's again when the call returns;
   barcode runs may straddle chunks in any way, the runs are found over the whole image); the call with final_chunk != 0 (n_records may
   be 0) hashes the image exactly as h10x_read_fqb_device and releases it. The host never holds more than one chunk. h10x_ingest_reserve
   (optional, before the first chunk) announces the total so that the image is allocated once instead of growing geometrically.
   The chunk semantics of "chunk_size" apply to the whole image as above. A failed call drops the image; h10x_ingest_reserve(ctx, 0)
   gives up an ingest that will not be closed. */
int  h10x_ingest_reserve(h10x_ctx *ctx, uint64_t n_records_total);
int  h10x_ingest_fqb(h10x_ctx *ctx, const uint32_t *host_records, uint64_t n_records, int final_chunk);
/* The same as a pipeline (round 4): the chunk lies in page-locked memory from h10x_pinned_alloc and its upload is only QUEUED — the call returns
   while the DMA runs, so the caller reads the next chunk of the file into another buffer meanwhile (hash10x.c:202-209's fread loop, with the file
   read and the PCIe transfer side by side). The buffer must not be touched until h10x_ingest_wait(ctx, slot) has returned for the slot (0..7)
   the chunk was queued under. The ingest is closed as before, by h10x_ingest_fqb / h10x_shard_ingest_fqb with final_chunk = 1 (which waits for
   every queued upload). */
/* Loads the library's device code on `device` ahead of its first use (HIP loads a code object when the first of its kernels is launched — some tens
   of milliseconds for this library, otherwise spent inside the first command). Thread-safe; meant to be called from a thread of its own while the
   caller opens and reads its input. 0 on success. No counterpart in the reference (a CPU program has no such step). */
int  h10x_warm(int device);
/* Device blocks this process has obtained from hipMalloc so far (count, bytes): the library keeps freed blocks and hands them out again, so a
   repeated command on one context should add nothing here — a measurement hook (tests/test_gpu_parity.py), no counterpart in the reference. */
void h10x_alloc_stats(uint64_t *calls, uint64_t *bytes);
void *h10x_pinned_alloc(size_t bytes);
void  h10x_pinned_free(void *p);
int  h10x_ingest_fqb_async(h10x_ctx *ctx, const uint32_t *pinned_records, uint64_t n_records, int slot);
int  h10x_ingest_wait(h10x_ctx *ctx, int slot);
int  h10x_read_fqb_device(h10x_ctx *ctx, const uint32_t *dev_records, uint64_t n_records);

/* replaces the external record sort between fq2b and hash10x (README.md:26 `bsort -k 4 -r 120 x.fqb`): orders the
   120-byte records by their first 4 bytes (byte 0 most significant), stably, so that equal barcodes are contiguous.
   in / out must not overlap. _device: both buffers in device memory. */
int  h10x_sort_fqb(h10x_ctx *ctx, const uint32_t *host_in, uint64_t n_records, uint32_t *host_out);
int  h10x_sort_fqb_device(h10x_ctx *ctx, const uint32_t *dev_in, uint64_t n_records, uint32_t *dev_out);

/* ---- barcode census and whitelist correction of unsorted .fqb records (csrc/stage_j.hip) ----
   The barcode step between fq2b and the record sort, on packed records instead of FASTQ text. A barcode is record word 0 as
   fq2b packs it (first base in the top two bits); whitelist order is the order of that packed value, no byte swap. Records come
   in batches, so neither the host nor the device ever holds the file: the census keeps 4 bytes per record between batches.
   h10x_census_begin / _add / _close replace the README's goodcodes pipeline (README.md:44, the wish of README.md:57-62: `gzip -dc | perl | sort | uniq -c |
   awk` over the FASTQ text) — begin opens a census (nRecordsHint > 0 reserves the key array once instead of growing it), add
   appends the barcodes of a batch, close(thresh) finds the distinct barcodes with their counts and makes the barcodes that occur
   at least thresh times the whitelist, in ascending order (line r + 1 = r-th good barcode). thresh < 1 fails. A census without a
   good barcode closes with nGood = 0 and leaves no whitelist. h10x_census_export copies out the distinct (goodOnly = 0) or good
   barcodes, ascending, with their counts (NULL = skip; at most cap entries).
   h10x_whitelist_set replaces read10xWhitelist (fq2b.c:71-94): codes in line order, a repeated code keeps its latest line.
   h10x_fix_fqb replaces find10xBarcode for a batch (fq2b.c:96-104, 157): per record the candidates are the barcode and its 48
   one-substitution neighbours that are in the whitelist; none: the record is dropped; otherwise the candidate of the latest line
   wins and replaces word 0. Kept records go to out in their input order (in / out must not overlap, out holds n records);
   *nKept = how many. acc (may be NULL) is ADDED to: dropped = nBad, corrected = nFixed, correctedAt[p] = nFixBase[p], p = position
   of the changed base counted from the first base. The host forms move the records through the device in batches of "fqb_slab"
   records (h10x_set_option; 0 = default 2^20); results do not depend on it. */
typedef struct { uint64_t nRecords, nDistinct, nGood, nGoodRecords; } h10x_census_t;
typedef struct { uint64_t dropped, corrected, correctedAt[16]; } h10x_fix_stats;
int  h10x_census_begin(h10x_ctx *ctx, uint64_t nRecordsHint);
int  h10x_census_add(h10x_ctx *ctx, const uint32_t *host_records, uint64_t n_records);
int  h10x_census_add_device(h10x_ctx *ctx, const uint32_t *dev_records, uint64_t n_records);
int  h10x_census_close(h10x_ctx *ctx, int64_t thresh, h10x_census_t *out);
int  h10x_census_export(h10x_ctx *ctx, int goodOnly, uint32_t *codes, uint32_t *counts, uint64_t cap);
int  h10x_whitelist_set(h10x_ctx *ctx, const uint32_t *host_codes, uint64_t n_codes);
int  h10x_fix_fqb(h10x_ctx *ctx, const uint32_t *host_in, uint64_t n_records, uint32_t *host_out, uint64_t *nKept, h10x_fix_stats *acc);
int  h10x_fix_fqb_device(h10x_ctx *ctx, const uint32_t *dev_in, uint64_t n_records, uint32_t *dev_out, uint64_t *nKept, h10x_fix_stats *acc);

/* ---- the molecule of every read pair, and the records in molecule order (csrc/stage_k.hip) ----
   The reference stops at the hash level: --clusterReport counts the reads of a cluster (hash10x.c:897-920) and --clusterSplit renumbers the
   reads of each new block (hash10x.c:979-989); neither result is written per read. Both calls work on the state after h10x_cluster and
   before h10x_cluster_split. nCodes = nBlocks (slot 0 unused); record base[c] + r of the sorted file the state was read from (base[c] =
   sum of nRead over blocks 1 .. c-1, R = base[nCodes] records) is read pair r of block c. A ClusterHash record of block c is clustered with
   label subCluster when 1 <= subCluster <= nSubCluster[c]; a read's label L is that of its first clustered record in block order.
   h10x_molecule_map: per record mol = nCodes - 1 + (sub-clusters of the blocks before c) + L, the block number h10x_cluster_split gives
     the cluster, and slot = the number of clustered reads of the block with the same label whose first clustered record lies earlier (the
     order of ++new2[clus].nRead, hash10x.c:984-985); an unclustered read has mol = c, slot = r. Arrays of at least R entries (cap says how
     many there are; either may be NULL, both NULL = info only). info: R, the reads with a molecule, nCodes and M = all sub-clusters.
   h10x_split_fqb: the records in split order: those of molecule m at start[m] + slot, those left in parent c at start[c] + (unclustered
     records of c in front), start[0 .. nBlocks + nMolecules] = exclusive sum of the records per post-split block (start[m + 1] - start[m] =
     nRead of block m after h10x_cluster_split, and its ClusterHash (hash, read r) refers to record start[m] + r). n_records must be R,
     startCap at least nBlocks + nMolecules + 1, in / out must not overlap. Before anything is written the records are checked against the
     state: a block whose records do not all carry word 0 of its first record (unless that is 0, the all-A barcode: hash10x.c:212) fails.
   All four fail without a state, on a sharded context, after h10x_cluster_split (a block with clusterParent != 0), for a clustered block
   of more than 65536 read pairs (the 16-bit read numbers wrap, hash10x.c:180) and for R >= 2^32. _device: arrays in device memory. */
typedef struct { uint64_t nRecords, nClustered; uint32_t nBlocks, nMolecules; } h10x_molmap_info;
int  h10x_molecule_map(h10x_ctx *ctx, uint32_t *mol, uint32_t *slot, uint64_t cap, h10x_molmap_info *info);
int  h10x_molecule_map_device(h10x_ctx *ctx, uint32_t *dev_mol, uint32_t *dev_slot, uint64_t cap, h10x_molmap_info *info);
int  h10x_split_fqb(h10x_ctx *ctx, const uint32_t *host_in, uint64_t n_records, uint32_t *host_out, uint64_t *start, uint64_t startCap);
int  h10x_split_fqb_device(h10x_ctx *ctx, const uint32_t *dev_in, uint64_t n_records, uint32_t *dev_out, uint64_t *start, uint64_t startCap);

/* replaces the state that readHashFile() + fillHashTable() leave behind (hash10x.c:269-315,
   317-347): uploads the tables of a parsed .hash file and rebuilds the hash->barcode lists.
   hashDepth has hashNumber entries, blocks has nBlocks entries (entry 0 unused), clusHash is the
   concatenation of blocks 1..nBlocks-1. */
int  h10x_load_state(h10x_ctx *ctx, const uint32_t *hashIndex, uint32_t hashNumber,
                     const uint64_t *hashValue, const uint32_t *hashDepth,
                     const h10x_block *blocks, uint32_t nBlocks, const h10x_clushash *clusHash);

/* replaces hashWithinRangeBuild() + goodHashesBuild() (hash10x.c:528-539, 738-766); ranges
   accumulate over calls exactly as in the reference. Returns once the work is queued on the context's stream (it has
   no host-side result); the next call on the context — h10x_cluster, an export — waits for it, and a device fault in
   it is reported there. */
int  h10x_depth_range(h10x_ctx *ctx, int32_t min, int32_t max);

/* replaces the --cluster loop: codeClusterFind() + codeClusterReadMerge() for code in
   [codeMin, codeMax) (hash10x.c:1241-1261, 770-868); 0,0 => 1..nBlocks. Fails with the reference's
   "!! you must set hashDepthRange before cluster" if no range was set. */
int  h10x_cluster(h10x_ctx *ctx, int32_t codeMin, int32_t codeMax, int32_t clusterThreshold);

/* replaces clusterSplitCodes() (hash10x.c:956-1013) */
int  h10x_cluster_split(h10x_ctx *ctx);

/* ---- crib: truth labels from two haplotype genomes (csrc/stage_d.hip) ----
   h10x_crib_genome replaces cribAddGenome() (hash10x.c:426-453) for one genome: `codes` holds one byte per base
   (0..3 as readSequence() yields them with dna2indexConv, 'N' -> 0: hash10x.c:432), all sequences concatenated,
   sequence s = codes[seqStart[s] .. seqStart[s+1]); which = 0 for the first .fa, 1 for the second. nPresent / nAbsent
   receive the "known" / "unknown" mosh counts the reference prints. h10x_crib_finish is the classification loop of
   cribBuild() (hash10x.c:476-494): cribType[], the merged crib[], and the four depth histograms (err, het, hom, mul). */
int  h10x_crib_genome(h10x_ctx *ctx, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq, int which,
                      uint64_t *nPresent, uint64_t *nAbsent);
int  h10x_crib_finish(h10x_ctx *ctx);
/* histDim = entries per depth histogram; arrayMax[4] = arrayMax() of the reference's aErr, aHet, aHom, aMul */
int  h10x_crib_sizes(h10x_ctx *ctx, uint32_t *histDim, uint32_t arrayMax[4]);
/* copy-out (NULL = skip): chr/pos/type have hashNumber entries (CribInfo.chr, CribInfo.pos, cribType), hist 4 * histDim */
int  h10x_crib_export(h10x_ctx *ctx, int16_t *chr, uint16_t *pos, uint8_t *type, uint32_t *hist);
/* per-block good-hash counts (nGoodHashes[], hash10x.c:723) for --clusterReport: nBlocks entries; fails before --hashDepthRange */
int  h10x_export_ngood(h10x_ctx *ctx, uint32_t *nGood);

/* what writeHashFile() needs (hash10x.c:244-267): sizes, then a copy-out of any subset of the
   tables (NULL = skip). hashIndex: 2^B, hashValue/hashDepth: hashNumber, blocks: nBlocks,
   clusHash: nClusHash entries. */
int  h10x_get_sizes(h10x_ctx *ctx, h10x_sizes *out);
int  h10x_export(h10x_ctx *ctx, uint32_t *hashIndex, uint64_t *hashValue, uint32_t *hashDepth,
                 h10x_block *blocks, h10x_clushash *clusHash);

/* ---- multi-GPU: barcodes sharded over N ranks, hashes owned by value range (csrc/shard.hip) ----
   The reference has no counterpart (its only parallelism is the OMP loop inside --cluster); the invariant is
   that N ranks produce exactly the bytes one rank produces. A communicator is either RCCL (one process per GPU:
   rank 0 calls h10x_comm_unique_id, ships the 128 bytes to the others by any means, every rank calls
   h10x_comm_create_rccl) or in-process (h10x_comm_create_local: N ranks driven by N threads of one process,
   used by the tests and by single-process multi-GPU hosts). */
typedef struct h10x_comm h10x_comm;
int  h10x_comm_unique_id(void *id128);
int  h10x_comm_create_rccl(h10x_comm **comm, int rank, int nranks, const void *id128, int device, char *err, int errlen);
int  h10x_comm_create_local(h10x_comm **comms /* nranks outputs */, int nranks);
/* RCCL communicators for N ranks of ONE process (ncclCommInitAll), rank r on devices[r]: what a single-process host — the C program's
   --gpus N — uses when the box has a GPU per rank; each communicator is then driven by its rank's thread. Distinct devices required. */
int  h10x_comm_create_rccl_all(h10x_comm **comms /* nranks outputs */, int nranks, const int *devices, char *err, int errlen);
/* peer access between every pair of the listed devices (best effort; ranks of an in-process communicator that sit on different
   devices then copy device to device directly instead of through the host) */
int  h10x_device_enable_peers(const int *devices, int n);
/* one process per rank like RCCL, but host-staged over TCP (rank r listens on basePort + r at addr): for exercising the
   multi-process launch path where RCCL cannot run — several ranks sharing one GPU on a test box. Not a production path. */
int  h10x_comm_create_socket(h10x_comm **comm, int rank, int nranks, const char *addr, int basePort, char *err, int errlen);
/* "Virtual ranks": the ranks of an in-process communicator share one device and take turns on it. With serialize on, a rank's thread computes only between
   h10x_comm_turn_begin and h10x_comm_turn_end (its caller brackets every command with them) and hands the device on inside every collective while it waits for the
   others — so its stage timers read as if it had the GPU to itself, and its exchange timers (h10x_exchange_get) hold all the waiting. A measuring device for
   `bench.py --virtual-ranks N` on one-GPU boxes; the results are those of any other N-rank run. -1 on a communicator that is not in-process. */
int  h10x_comm_local_serialize(h10x_comm *comm, int on);
int  h10x_comm_turn_begin(h10x_comm *comm);
int  h10x_comm_turn_end(h10x_comm *comm, int device);
void h10x_comm_destroy(h10x_comm *comm);
int  h10x_comm_rank(const h10x_comm *comm);
int  h10x_comm_size(const h10x_comm *comm);
/* bind a communicator to a context (collective calls below are made by every rank in the same order) */
int  h10x_shard_attach(h10x_ctx *ctx, h10x_comm *comm);
/* --readFQB on this rank's contiguous barcode range of the sorted file (cut with h10x_host_partition): stage A
   locally, then the hash-owner exchange; afterwards every rank holds hashDepth of the whole data set and
   blocks/clusHash of its own barcodes. h10x_depth_range / h10x_cluster / h10x_cluster_split / h10x_crib_* work as
   usual and are collective on a sharded context (global barcode numbers; --hashDepthRange also allgathers the barcode
   lists of the in-range hashes, --clusterSplit numbers the new blocks over all ranks and sends the entries' new block
   numbers back to the hash owners, the crib is computed on every rank against the whole table). hashValue / hashIndex of the whole
   set (only --writeHash and the crib read them) are built by h10x_shard_gather, not here. */
int  h10x_shard_read_fqb(h10x_ctx *ctx, const uint32_t *host_records, uint64_t n_records);
int  h10x_shard_read_fqb_device(h10x_ctx *ctx, const uint32_t *dev_records, uint64_t n_records);
/* h10x_ingest_fqb for this rank's record range of the file: chunks append, the closing call runs the sharded --readFQB (collective) */
int  h10x_shard_ingest_fqb(h10x_ctx *ctx, const uint32_t *host_records, uint64_t n_records, int final_chunk);
/* --readHash onto shards (collective): the replicated tables of the file (hashIndex, hashValue, hashDepth: whole data set) plus THIS
   rank's contiguous cut of the file's blocks — localBlocks[0] unused, localBlocks[1 ..] = blocks codeBase + 1 .. of the file, with
   their ClusterHash records concatenated. The hash owners' barcode lists are rebuilt by an exchange (ownership by index range);
   inconsistent files (entries of a hash != its depth) are refused there. */
int  h10x_shard_load_state(h10x_ctx *ctx, const uint32_t *hashIndex, uint32_t hashNumber, const uint64_t *hashValue,
                           const uint32_t *hashDepth, const h10x_block *localBlocks, uint32_t nLocalBlocks,
                           const h10x_clushash *localClusHash, uint32_t codeBase, uint32_t nBlocksGlobal);
/* collective: every rank builds hashValue / hashIndex of the whole set; rank 0 receives every rank's blocks and
   clusHash (in file order), rebuilds the barcode lists and from then on IS a single-GPU context (for continuing on one
   GPU; --writeHash and the reports work on the shards directly, see below) */
int  h10x_shard_gather(h10x_ctx *ctx);
/* ---- a sharded state without a gather ("each rank pwrites its slices") ----
   After --readFQB every rank owns one contiguous range of the file's barcode blocks; every --clusterSplit appends, for
   each range that held parents, a range of new blocks numbered behind ALL existing blocks (hash10x.c:961-1003). A
   segment = one such range on one rank. h10x_shard_segments lists the segments of all ranks in file order (ascending
   globalBase): blocks [localStart, localStart + count) of rank `rank` are blocks [globalBase, ...) of the data set and
   their `entries` ClusterHash records start at localEntryStart in that rank's clusHash (filled in for the caller's own
   segments) and at globalEntryStart in the file's. An unsharded context reports itself as one segment of rank 0.
   h10x_shard_prepare_export (collective) builds hashValue[] / hashIndex[] of the whole set on every rank;
   h10x_export_slice copies elements [first, first + count) of one table of THIS rank to the host. */
typedef struct {
  uint32_t rank, localStart, count, globalBase;
  uint64_t entries, localEntryStart, globalEntryStart;
} h10x_shard_seg;
typedef struct {
  int32_t  rank, nranks, B; uint32_t hashNumber;
  uint32_t nBlocksGlobal;      /* arrayMax(clusterBlocks) of the whole data set */
  uint32_t nSegs;              /* entries h10x_shard_segments will write */
  uint64_t nEntriesGlobal, nRecordsGlobal;
} h10x_shard_info_t;
enum { H10X_TABLE_HASHINDEX = 0, H10X_TABLE_HASHVALUE = 1, H10X_TABLE_HASHDEPTH = 2, H10X_TABLE_BLOCKS = 3, H10X_TABLE_CLUSHASH = 4,
       H10X_TABLE_NGOOD = 5,
       H10X_TABLE_CLUSTER_RAW = 6 /* per block, after h10x_cluster: u32 clusters before the read merge (bit 31: given up at the 256th, hash10x.c:810-816),
                                     u32 good hashes with a label — the figures of the reference's --verbose line (hash10x.c:827-834) */,
       H10X_TABLE_WITHIN = 7 /* hashWithinRange[] (hash10x.c:525-539): one byte per hash index, 1 = in a --hashDepthRange set so far; fails before the first */ };
int  h10x_shard_info(h10x_ctx *ctx, h10x_shard_info_t *out);
int  h10x_shard_segments(h10x_ctx *ctx, h10x_shard_seg *out, uint32_t cap);
int  h10x_shard_prepare_export(h10x_ctx *ctx);
int  h10x_export_slice(h10x_ctx *ctx, int table, uint64_t first, uint64_t count, void *dst);
/* collective plumbing for launchers: barrier, max over ranks of a host double (timing), sums / maxima of small host
   arrays (in place), and a gather of byte strings to rank 0 (recv = the strings in rank order, counts[r] = bytes of
   rank r; recv / cap are read on rank 0 only). On an unsharded context these are the identity. */
int  h10x_shard_barrier(h10x_ctx *ctx);
/* do all ranks of the attached communicator say ok? Works before a state is loaded (h10x_shard_allreduce_* are the identity then):
   a launcher whose rank failed on its own — a short read of its part of a file, no memory — reports it here, so that every rank
   leaves with the same verdict instead of waiting in the next collective. Without a communicator *allOk = ok. */
int  h10x_shard_agree(h10x_ctx *ctx, int ok, int *allOk);
int  h10x_shard_allreduce_max(h10x_ctx *ctx, double *value);
int  h10x_shard_allreduce_sum_u64(h10x_ctx *ctx, uint64_t *values, uint32_t n);
int  h10x_shard_allreduce_max_u64(h10x_ctx *ctx, uint64_t *values, uint32_t n);
int  h10x_shard_gather_bytes(h10x_ctx *ctx, const void *send, uint64_t nbytes, void *recv, uint64_t cap, uint64_t *counts);

/* ---- the text reports, reduced on the device (csrc/stage_e.hip): only these results cross PCIe, never clusHash ----
   h10x_report_max / h10x_report_histogram: what histogramReport() is fed with (hash10x.c:351-402): `which` = 0
   hashDepth[first .. first+count) (hashDepthHist), 1 nHash and 2 nSubCluster of this rank's blocks [first, first+count)
   (codeSizeHist); hist has `bins` entries, values >= bins are not counted.
   h10x_cluster_report: codeClusterReport()'s per-barcode and per-sub-cluster figures (hash10x.c:870-952) for this
   rank's blocks [firstBlock, firstBlock+nBlocks): one h10x_block_rep per block, and for block b its sub-clusters
   1 .. min(nSubCluster, 255) consecutively in `clusters` (in block order). Without a crib the crib fields are 0.
   h10x_crib_summary: cribSummary()'s tallies (hash10x.c:1017-1061) over this rank's blocks 1..: counts[0..4] entries
   per crib type in base blocks, [5..9] in blocks made by --clusterSplit, [10] / [11] the number of such blocks; the two
   bitmaps (bit = hash index, (hashNumber + 31) / 32 words) mark the hashes met in each kind. */
typedef struct { uint32_t nGood, nClusHash, nClusRead, reserved; } h10x_block_rep;
typedef struct {
  uint32_t n, nRead, nt[5];      /* hashes, reads, hashes per crib type (err htA htB hom mul) */
  uint32_t nBad;                 /* located hashes on another chromosome than the first located one ("OTHER") */
  int16_t  chr; uint16_t pMin, pMax, nOtherListed;
  uint32_t other[10];            /* hash indices of the last ten of those, in the reference's print order */
} h10x_cluster_rep;
int  h10x_report_max(h10x_ctx *ctx, int which, uint64_t first, uint64_t count, uint32_t *maxValue);
int  h10x_report_histogram(h10x_ctx *ctx, int which, uint64_t first, uint64_t count, uint32_t bins, uint64_t *hist);
int  h10x_cluster_report(h10x_ctx *ctx, uint32_t firstBlock, uint32_t nBlocks, h10x_block_rep *blocks,
                         h10x_cluster_rep *clusters, uint64_t clusterCap, uint64_t *nClusters);
int  h10x_crib_summary(h10x_ctx *ctx, uint64_t counts[12], uint32_t *seenBase, uint32_t *seenCluster);
/* cribSummary's walk over the blocks (hash10x.c:1030-1046) as one word per ClusterHash record [first, first + count) of THIS rank, in clusHash order: bit 31 = the
   record's block was made by --clusterSplit, bits 28-30 = cribType of its hash, bits 0-27 = the hash index. The second and third figure of every type in the
   reference's summary is hashCount() of a HASH object fed in exactly this order (hash.c) — and that count depends on the order once such an object has doubled
   (see RefHash in host/h10x_host.c) — so the host layer replays the words through a restatement of it. */
int  h10x_crib_words(h10x_ctx *ctx, uint64_t first, uint64_t count, uint32_t *words);

/* ---- neighbour census (csrc/stage_f.hip): the hashes that share barcode blocks with a query hash ----
   For a query x, N(x) = every hash h != x with hashWithinRange[h] in any block that holds x, and c_x(h) = the number of blocks
   holding both (hashNeighbours / countHashNeighbours, hash10x.c:541-586; the blocks are the current ones, --clusterSplit
   included). Each call fails before --hashDepthRange, on a sharded context, and for a query not below hashNumber.
   h10x_neighbours: the list of --hashInfo / --hashExplore / --doubleShared (hash10x.c:541-567, 588-647): *n = |N(x)|, and the
     first min(cap, *n) pairs ascending in h: hash[i], count[i] = c_x(hash[i]) (full count; the reference keeps it mod 2^16),
     firstCode[i] = the lowest barcode holding hash[i] (*arr(hashCodes, h, U32*), hash10x.c:620). Any array may be NULL; call
     again with a larger cap when *n > cap. A query of depth 0 gives *n = 0.
   h10x_neighbour_max: per query (repeats allowed) what --hashInfo prints (hash10x.c:631-647): maxKey[q] = the maximum over N(x) of
     (c_x(h) mod 2^16) << 32 | h — the last element after the reference's stable sort on the 16-bit count — and nNeighbours[q] = |N(x)|
     (0: maxKey[q] = 0).
   h10x_neighbour_hist: per query the histogram countHashNeighbours builds for --errorFix / --shareScan (hash10x.c:569-586, 651-718):
     hist[offsets[q] + k] = the number of h in N(x) with c_x(h) = k, full int counts. offsets has nq + 1 entries; region q is
     [offsets[q], offsets[q + 1]) and must hold depth(x) + 1 bins (c_x(h) <= depth(x)); bins above the top count are 0.
   Work is cut into batches of at most "neighbour_budget" gathered ClusterHash records (h10x_set_option); a larger query runs in
   windows of hash index. h10x_neighbour_stats: out[0] records gathered, out[1] in-range keys sorted, out[2] batches, out[3]
   windows, since the last call with reset != 0. */
int  h10x_neighbours(h10x_ctx *ctx, uint32_t x, uint32_t *hash, uint32_t *count, uint32_t *firstCode, uint64_t cap, uint64_t *n);
int  h10x_neighbour_max(h10x_ctx *ctx, const uint32_t *xs, uint32_t nq, uint64_t *maxKey, uint32_t *nNeighbours);
int  h10x_neighbour_hist(h10x_ctx *ctx, const uint32_t *xs, uint32_t nq, const uint64_t *offsets, uint32_t *hist);
int  h10x_neighbour_stats(h10x_ctx *ctx, uint64_t out[4], int reset);

/* ---- barcode census and --codeExplore (csrc/stage_f.hip, codeExplore: hash10x.c:1351-1470) ----
   For a barcode `code` with good hashes g[0 .. n) (the --hashDepthRange lists, ranks in depth order), every entry cj != code of the
   barcode list of hash(g[i]), i = 0 .. n-1 (repeats as the list holds them): countShare[cj] = the number of such entries,
   first[cj] = the lowest rank i whose list holds cj. Every call fails on a sharded context, before --hashDepthRange and after
   --clusterSplit until a new range is set ("!! you must set hashDepthRange before ..."), and for a barcode not below nBlocks.
   h10x_code_share: per query (repeats allowed) the rows (barcode, count = countShare, firstRank = first, firstHash = hash index
     at g[first]) of the barcodes with countShare > 0, ascending in barcode; rows of query q = [offsets[q], offsets[q + 1]) (offsets:
     nq + 1 entries, always filled). The first min(cap, offsets[nq]) rows are written (any array may be NULL): call with cap 0 for
     the sizes, then again. Batches and windows (of barcode index) as the neighbour census, counted in h10x_neighbour_stats.
   h10x_code_explore: codeExplore's state change for one barcode — the good hashes' labels wiped and re-clustered with i from 0 (not
     1 as in --cluster), clusters numbered in founding order, the 256th abandons the block (labels 0, nSubCluster 0, pointToMin
     keeps the partial sum: hash10x.c:1392-1397), pointToMin = the fp64 sum in rank order, then the read merge of --cluster. A
     barcode without good hashes is left as it is (rep: nHash, nGood only). Also fails for code < 0 ("!! codeExplore code ...
     outside 0 to nBlocks") and threshold < 1 ("!! clusterThreshold ... must be >= 1 ..."). The COUNT_SHARE histogram has
     histMax + 1 bins: bin 0 = nBlocks - nShare, bin k = rows of h10x_code_share with count k.
   h10x_code_crib_counts: per listed barcode the CRIB_HTA and CRIB_HTB records of its block (out[2 q], out[2 q + 1]: the htA / htB
     figures of the SHARE lines); fails without a crib ("!! codeExplore needs --cribBuild for its SHARE lines"). */
typedef struct {
  uint32_t nHash, nGood;   /* the block's records and good hashes */
  uint32_t clustered;      /* good hashes labelled before the read merge (0 when abandoned) */
  uint32_t raw;            /* clusters before the read merge (0 when abandoned) */
  uint32_t merged;         /* clusters after it: the block's nSubCluster */
  uint32_t abandoned;      /* 1 = the 256th cluster gave the block up */
  uint32_t histMax;        /* the largest countShare */
  uint32_t nShare;         /* barcodes with countShare > 0 */
} h10x_code_explore_rep;
int  h10x_code_share(h10x_ctx *ctx, const uint32_t *codes, uint32_t nq, uint64_t *offsets, uint32_t *barcode, uint32_t *count,
                     uint32_t *firstRank, uint32_t *firstHash, uint64_t cap);
int  h10x_code_explore(h10x_ctx *ctx, int32_t code, int32_t threshold, h10x_code_explore_rep *rep);
int  h10x_code_crib_counts(h10x_ctx *ctx, const uint32_t *codes, uint32_t n, uint32_t *out);

/* ---- the share graph (csrc/stage_l.hip): all pairs of blocks that share at least minShare good hashes ----
   The barcode census above for every block at once, thresholded on the device. For a block c, countShare_c[d] is the `count` column of
   h10x_code_share: the entries d != c in the barcode lists of c's good hashes, repeats as the lists hold them. It is a DIRECTED count: a block
   of more than 65535 records has no good hashes (hash10x.c:748), so its own row is empty, yet it appears in the rows of others. The graph at
   minShare = T >= 1 over blocks [codeMin, codeMax) is, per block c of the range, the row {(d, countShare_c[d]) : countShare_c[d] >= T}
   ascending in d, in CSR form: offsets[codeMax - codeMin + 1], and block[] / count[] with offsets[last] entries. At T = 1 these are the
   rows of h10x_code_share for the same codes. codeMax = 0 means nBlocks (as --cluster 1 0); codeMin >= codeMax is an empty graph (one
   offset, 0). The blocks are the current ones: after --clusterSplit and a new range they are the molecules.
   h10x_share_graph_run computes the graph with ONE census — per block and per list a size pass, keys (c - codeMin') << bits | d without a
     rank (32-bit where they fit), every list's place from a scan instead of a reservation, a sort, and a run pass that keeps only runs of
     length >= T — and keeps the rows in device memory of the context. Batches are cut by list entries against "neighbour_budget", a block
     above it runs alone in windows of barcode index; both are counted in h10x_neighbour_stats too. The result does not depend on the
     batching, and two calls give the same bytes. info: rows = offsets[last]; listEntries = the list entries d != c gathered and sorted
     (the sum of all counts at T = 1); entriesRead = list entries read, the blocks' own included; maxCount = the largest count of a row (0 without rows); batches, windows of this call; the range
     as it was taken, and nBlocks.
   h10x_share_graph_get / _get_device copy the kept graph out: the offsets and the first min(cap, rows) rows (any array may be NULL), to
     host or to device memory. The kept graph is released by the next run (also a failed one), h10x_depth_range, h10x_cluster_split, a new
     state and h10x_destroy; get without one fails.
   h10x_share_graph_run fails without a state, on a sharded context, before --hashDepthRange and after --clusterSplit until a new range is
   set ("!! you must set hashDepthRange before shareGraph"), for minShare < 1 ("!! shareGraph minShare ... must be >= 1") and for
   codeMax > nBlocks ("!! shareGraph codeMax ... beyond nBlocks ..."). */
typedef struct {
  uint64_t rows, listEntries, entriesRead;
  uint32_t maxCount, batches, windows;
  uint32_t codeMin, codeMax, nBlocks;
} h10x_share_graph_info;
int  h10x_share_graph_run(h10x_ctx *ctx, int64_t minShare, uint32_t codeMin, uint32_t codeMax, h10x_share_graph_info *info);
int  h10x_share_graph_get(h10x_ctx *ctx, uint64_t *offsets, uint32_t *block, uint32_t *count, uint64_t cap);
int  h10x_share_graph_get_device(h10x_ctx *ctx, uint64_t *dev_offsets, uint32_t *dev_block, uint32_t *dev_count, uint64_t cap);

/* ---- the components of the share graph (csrc/stage_m.hip): which blocks hang together through shared good hashes ----
   State: as for the share graph, an unsharded context with a --hashDepthRange in force.
   Graph: the share graph above at minShare = T >= 1 over ALL blocks. Every row entry (c, d) is an undirected edge {c, d}. A block of more
   than 65535 records has an empty row of its own, yet it stands in the rows of others: such entries join it all the same.
   Per block and per component:
     root[c]   = the smallest block number in c's connected component; root[0] = 0.
     The components of blocks 1 .. nBlocks-1 are numbered 1 .. nComponents in ascending order of their root.
     comp[c]   = that number; comp[0] = 0.
     For each component k: blocks[k] = its member count (u32), records[k] = the sum of nHash over its members (u64), rootOf[k] = its root.
     Entry 0 of the three is all zero. A block without edges is a component of one; empty blocks count.
   The result depends on none of "neighbour_budget", the ranges the blocks are added in, the order in which atomics land, or the run: two
   calls give the same bytes.
   h10x_share_components_begin starts a run: parent[nBlocks], one label per block, is set up on the device as the identity.
   h10x_share_components_add(ctx, codeMin, codeMax) runs the census of h10x_share_graph_run over blocks [codeMin, codeMax) (codeMax = 0:
     nBlocks) and folds that range's rows into parent[] where they were made: a hook kernel, one thread per row, joins the two ends by
     lock-free union by smaller root; a check kernel counts the rows whose ends still differ, and the hook runs again while there are any
     (bounded; running out of rounds is an error). The caller adds ranges that cover blocks 1 .. nBlocks-1, each block once, in any order. The
     census uses the share graph's result arrays: a share graph kept from h10x_share_graph_run is dropped by a components run.
   h10x_share_components_finish computes the five arrays and keeps them in device memory of the context. info: nBlocks, minShare, rows =
     the rows of all ranges, listEntries as in h10x_share_graph_info, nComponents, largest = the largest member count, singletons = the
     components of one block, batches and windows of the censuses, hookRounds = hook launches over all ranges (one per range that has rows,
     unless a check asked for more).
   h10x_share_components_get copies the first min(capBlocks, nBlocks) entries of comp / root and the first min(capComps, nComponents + 1) of
     rootOf / blocks / records to host memory; any array may be NULL. With all NULL it returns 0 when a result is kept, non-zero otherwise.
   The kept result (and a run in progress) is released by the next begin (also a failed one), h10x_depth_range, h10x_cluster_split, a new
   state and h10x_destroy. begin fails without a state, on a sharded context, before --hashDepthRange and after --clusterSplit until a new
   range is set ("!! you must set hashDepthRange before shareComponents") and for minShare < 1 ("!! shareComponents minShare ... must be
   >= 1"); add and finish fail without a begin. */
typedef struct {
  uint64_t rows, listEntries;
  uint32_t nBlocks, minShare, nComponents, largest, singletons, batches, windows, hookRounds;
} h10x_share_components_info;
int  h10x_share_components_begin(h10x_ctx *ctx, int64_t minShare);
int  h10x_share_components_add(h10x_ctx *ctx, uint32_t codeMin, uint32_t codeMax);
int  h10x_share_components_finish(h10x_ctx *ctx, h10x_share_components_info *info);
int  h10x_share_components_get(h10x_ctx *ctx, uint32_t *comp, uint32_t *root, uint32_t *rootOf, uint32_t *blocks, uint64_t *records,
                               uint64_t capBlocks, uint64_t capComps);

/* ---- the per-hash linkage groups (csrc/stage_n.hip): at how many places of the genome does a hash sit ----
   State: as for the share graph, an unsharded context with a --hashDepthRange in force. T = minShare >= 1.
   For a hash index x >= 1 with hashWithinRange[x] set:
     L(x) = its barcode list: one entry per ClusterHash record of x, ascending, a block as often as it holds x.
     D(x) = the distinct blocks of L(x), m = |D(x)|.
     Graph on D(x): a and b (a != b) are joined when countShare_a[b] >= T or countShare_b[a] >= T, countShare as the share graph above
     defines it. x itself counts: every pair of D(x) shares at least x. Either direction joins, as for the components: a block of more
     than 65535 records has an empty row of its own and is joined through the rows of the others.
     distinct = m, groups = the connected components of that graph, largest = the member count of the largest component, second = that of
     the second largest (0 with one group). Four u16 values per hash; hashes outside the range, and index 0, get four zeros.
   So at T = 1 a hash whose blocks are not all above 65535 records has groups = 1 and largest = m; at T = 2^31 - 1 groups = m, largest = 1
   and second = 1 if m > 1; groups does not fall as T rises. A hash at one locus tends to one group, a hash at two loci to two that do not
   link: thresholds on second / largest are the caller's.
   The result depends on none of "neighbour_budget", the order in which atomics land, or the run: two calls give the same bytes.
   A list of more than 4096 entries in range is refused for the whole call ("!! hashCopies needs every hash in range to have depth <= 4096
   (deepest N)"): a wave's working set then has a fixed bound in LDS and u16 holds every figure.
   h10x_hash_copies_run runs the census of h10x_share_graph_run over all blocks at T (the rows stay on the device and are dropped at the
     end; a share graph or components kept from an earlier call are dropped too), then one wave per in-range hash: the list deduped into LDS,
     each member's row streamed and looked up there, the hits hooked by union by smaller label in LDS until a pass hooks nothing (bounded;
     running out of passes is an error), the members per root counted. info: hashNumber, minShare, inRange = the hashes x >= 1 in range,
     rows / listEntries / batches / windows of the census, deepest = the longest in-range list, oneGroup = hashes with groups = 1, split =
     hashes with second >= 2.
   h10x_hash_copies_get copies records [first, first + count) (4 x u16 each) to host memory, _get_device to device memory. out = NULL asks
     whether a result is kept: 0 if so.
   h10x_hash_copies_tally: counts[t][0 .. 2] = in-range hashes, those with groups = 1, those with second >= 2, per crib type t (err, htA, htB,
     hom, mul; everything under 0 when no crib was built at the time of the run).
   The kept result is released by the next run (also a refused one), h10x_depth_range, h10x_cluster_split, a new state and h10x_destroy.
   The run fails without a state, on a sharded context, before --hashDepthRange and after --clusterSplit until a new range is set ("!! you
   must set hashDepthRange before hashCopies"), for minShare < 1 ("!! hashCopies minShare ... must be >= 1") and above the depth cap. */
typedef struct {
  uint64_t inRange, rows, listEntries, oneGroup, split;
  uint32_t hashNumber, minShare, deepest, batches, windows, reserved;
} h10x_hash_copies_info;
int  h10x_hash_copies_run(h10x_ctx *ctx, int64_t minShare, h10x_hash_copies_info *info);
int  h10x_hash_copies_get(h10x_ctx *ctx, uint16_t *out, uint64_t first, uint64_t count);
int  h10x_hash_copies_get_device(h10x_ctx *ctx, uint16_t *dev_out, uint64_t first, uint64_t count);
int  h10x_hash_copies_tally(h10x_ctx *ctx, uint64_t counts[5][3]);

/* ---- mosh sets (csrc/stage_g.hip): the Moshset object of the reference's moshutils (moshset.h, moshset.c, moshutils.c) ----
   A second opaque handle beside the context. A set is the probe table index[2^B] (moshsetIndexFind, moshset.c:45-61) and, per index
   1 .. max in order of first appearance, value (the hash), depth (saturating at 65535) and info (low two bits = copy class 0, 1, 2, M).
   Every function returns 0 on success; h10x_mosh_error() then holds the message otherwise — the reference's die() text where it
   would have died ("hashTableSize %u is too small for %u", moshset.c:57). One host thread per set. No CPU fallback. */
typedef struct h10x_mosh h10x_mosh;
typedef struct {
  int32_t  B, k, w, reserved;
  uint64_t factor1, factor2;    /* seqhashCreate's two multipliers (seqhash.c:29-31); only factor1 hashes, factor2 goes into the file */
  uint32_t max;                 /* ms->max: number of entries */
  uint32_t size;                /* ms->size: the per-index arrays hold this many; the entry that makes max reach it dies */
} h10x_mosh_info_t;
/* srandom(seed); seqhashCreate: factor1 then factor2, two random() draws each (moshutils.c:150-151, seqhash.c:29-31).
   factor1 is h10x_factor1_from_seed(seed). */
void h10x_factors_from_seed(int32_t seed, uint64_t *factor1, uint64_t *factor2);
/* moshsetCreate(seqhashCreate(k, w), B, 0) after srandom(seed) (moshutils.c:150-152, moshset.c:15-31): an empty set that holds up to
   2^(B-2) - 2 hashes. B 20..34; a set that does not fit the device fails with the bytes it asked for. */
int  h10x_mosh_create(h10x_mosh **set, int32_t B, int32_t k, int32_t w, int32_t seed, int device, char *err, int errlen);
/* the state moshsetRead leaves (moshset.c:89-103) from the arrays of a parsed MSHSTv1 file: index 2^B entries, value / depth / info
   `size` = max + 1 entries. The set is FULL, as in the reference (its arrays are sized to the file): the first new hash dies. */
int  h10x_mosh_load(h10x_mosh **set, int32_t B, int32_t k, int32_t w, uint64_t factor1, uint64_t factor2, const uint32_t *index,
                    const uint64_t *value, const uint16_t *depth, const uint8_t *info, uint32_t size, int device, char *err, int errlen);
void h10x_mosh_destroy(h10x_mosh *set);
const char *h10x_mosh_error(const h10x_mosh *set);
int  h10x_mosh_info(const h10x_mosh *set, h10x_mosh_info_t *out);
/* "mosh_slab": bases per device batch of h10x_mosh_add / h10x_mosh_scan (0 = default 2^26; a longer sequence goes alone).
   "overlap_chunk", "overlap_chunk_reads": the overlap table of a readset over this set (below) is built for chunks of queries; a chunk
   ends before the read that would take its expanded entries past overlap_chunk (0 = default 2^26; a read with more goes alone) and
   holds at most overlap_chunk_reads reads (0 = default and upper limit 65536: a read's place in its chunk travels in 16 bits; a larger
   value is refused with -1). Both are read when the table is built, i.e. by the first call after h10x_readset_add / _load that needs
   it; h10x_readset_chunks reports how many chunks it took. Results depend on none of the three. Unknown name: -1. */
int  h10x_mosh_set_option(h10x_mosh *set, const char *name, int64_t value);
/* scan_retries = the device batches, since the set was made, whose list of moshes (h10x_mosh_add, h10x_mosh_scan, h10x_refmap_add,
   h10x_refmap_query) or of hits (h10x_readset_add) overflowed the size estimated for it, 2 * (k-mers / w) + 65536, and were scanned a
   second time at the exact size: long runs of N or of one base, low-complexity reads. h10x_refmap_add scans every batch twice (find-or-add,
   then the ordered list), so such a batch counts twice there. Results do not depend on it. */
typedef struct { uint64_t scan_retries, reserved[3]; } h10x_mosh_counters_t;
int  h10x_mosh_counters(const h10x_mosh *set, h10x_mosh_counters_t *out);
/* addSequence over sequences (moshutils.c:19-30, 41-45): codes = one byte per base (0..3, N -> 0), sequence s =
   codes[seqStart[s] .. seqStart[s+1]). Every mosh occurrence is found or added in file order and its depth incremented.
   skipOdd23 != 0 is -x: the 1st, 3rd, ... sequence (counting seqBase sequences before this call) starts 23 bases in; one shorter
   than 23 fails (the reference aborts on an assert). *nHashes = occurrences. */
int  h10x_mosh_add(h10x_mosh *set, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq, int skipOdd23, uint64_t seqBase,
                   uint64_t *nHashes);
/* the moshes themselves, as moshRCiterator / moshRCnext yield them (seqhash.c:154-195), in order: hash, sequence number (0-based),
   position of the k-mer. The set is not changed. *n = how many there are; the first min(cap, *n) are written (NULL = skip). */
int  h10x_mosh_scan(h10x_mosh *set, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq, int skipOdd23, uint64_t seqBase,
                    uint64_t *hash, uint32_t *seq, uint32_t *pos, uint64_t cap, uint64_t *n);
/* moshsetMerge (moshset.c:105-120) of another set given by its per-index arrays (size2 = its max + 1 entries, entry 0 unused):
   *merged = 0 and nothing done if k, w or factor1 differ (the caller prints the reference's "incompatible" line). value2[1 ..] must be
   distinct, as they are in any set (h10x_moshfile_read checks a file's); repeated values are undefined here. */
int  h10x_mosh_merge(h10x_mosh *set, int32_t k2, int32_t w2, uint64_t factor1_2, const uint64_t *value2, const uint16_t *depth2,
                     const uint8_t *info2, uint32_t size2, int *merged);
/* moshsetDepthPrune (moshset.c:63-76): keeps depth >= min && (!max || depth < max), renumbers, rebuilds the table */
int  h10x_mosh_prune(h10x_mosh *set, int32_t min, int32_t max, uint32_t *nBefore, uint32_t *nAfter);
/* -s (moshutils.c:170-178) and -sM (moshutils.c:181-184) */
int  h10x_mosh_set_copy(h10x_mosh *set, int32_t copy1min, int32_t copy2min, int32_t copyMmin);
int  h10x_mosh_set_copy_m(h10x_mosh *set, int32_t copyMmin);
/* what moshsetSummary and depthHistogram count (moshset.c:127-133, moshutils.c:52-62): hist[65536] by depth, copy[4] by class */
int  h10x_mosh_summary(h10x_mosh *set, uint32_t *hist65536, uint32_t *copy4);
/* copy-out for moshsetWrite (moshset.c:78-87): entries [indexFirst, indexFirst + indexCount) of the table, and value / depth / info
   with max + 1 entries each (NULL = skip). value[0] is 0 (uninitialised heap in the reference). */
int  h10x_mosh_export(h10x_mosh *set, uint64_t indexFirst, uint64_t indexCount, uint32_t *index, uint64_t *value, uint16_t *depth,
                      uint8_t *info);
/* moshsetIndexFind(ms, hash, FALSE) per hash (reportDepths, moshutils.c:64-76): index (0 = absent) and depth (0 when absent) */
int  h10x_mosh_lookup(h10x_mosh *set, const uint64_t *hashes, uint64_t n, uint32_t *index, uint16_t *depth);

/* ---- the state as a mosh set (csrc/stage_o.hip): the in-range hashes of a context as a classed set, behind --writeMosh ----
   hash10x (hash10x.c:1099-1104) and moshutils -c (moshutils.c:150-151) both call srandom(seed); seqhashCreate(k, w), take their hashes from
   moshRCiterator and keep them in the same probe table (hashIndexFind, hash10x.c:139-152 = moshsetIndexFind, moshset.c:45-61), so a state with
   -k K -w W -r R is a mosh set with hasher (K, W, seed R) that lacks the 16-bit depths and the info byte.
   State: a loaded, unsharded context with a --hashDepthRange in force; --cluster / --clusterSplit may or may not have run before.
   Parameters: bits = the table bits of the set (0 = the state's B, otherwise 20 .. 34); copy1min <= copy2min <= copyMmin, the thresholds of moshutils -s.
   Kept hashes: the indices x >= 1 with hashWithinRange[x], ascending; the k-th kept hash gets set index k from 1 (what moshsetDepthPrune does
   with the survivors of a set, moshset.c:63-76). Per kept hash: value = hashValue[x]; depth = min(hashDepth[x], 65535); info = the class in its
   low two bits, nothing else:
     1. the base class from the saturated depth d as moshutils.c:173-177: d < copy1min -> 0, d < copy2min -> 1, d < copyMmin -> 2, otherwise 3 (M);
     2. if a --hashCopies result is kept for this state, x's record (distinct, groups, largest, second) overrides it: second >= 2 -> 3 (the hash's
        molecules fall into two real groups: multicopy whatever its depth), otherwise largest < 2 -> 0 (no two blocks that hold it link at that
        minShare), otherwise the base class stays;
     3. without a kept result the base class stands ("depth only").
   Table: index[2^bits] is what moshsetIndexFind(ms, value, TRUE) builds when the kept hashes are inserted in set-index order into an empty table.
   Header: k, w and the two multipliers of the context's hasher. The context learns its -r value through option "seqhash_seed" (the session layer
   sets it; the call fails without it, or if it does not give the context's factor1). For a state from --readHash these are trusted as the reference
   trusts them: a .hash file does not store them. value[0] is 0.
   The result depends on nothing but the state, the kept --hashCopies result and the five parameters: two calls give the same bytes. The call neither
   releases nor changes the kept --hashCopies result.
   info: kept; copy[q] = kept hashes of class q; toM / to0 = kept hashes whose class the linkage changed to M / to 0 (a hash whose depth had put it
   there already does not count); saturated = kept hashes with hashDepth > 65535; crib[t][q] = kept hashes of crib type t (err, htA, htB, hom, mul)
   and class q, all 0 without a crib; hashNumber; bits = the table bits used; minShare = that of the kept --hashCopies result, 0 = depth only.
   *set is an ordinary h10x_mosh, full as after h10x_mosh_load; every h10x_mosh_* call works on it and the caller destroys it. On failure *set = NULL
   and h10x_last_error(ctx) holds the text: no state; a sharded context; before --hashDepthRange and after --clusterSplit until a new range ("!! you
   must set hashDepthRange before writeMosh"); "!! writeMosh needs 0 <= copy1min <= copy2min <= copyMmin"; "!! writeMosh bits N must be 0 or
   20 .. 34"; kept + 1 >= 2^(bits-2): moshsetCreate's "Moshset size %u is too big for %d bits" (moshset.c:24). */
typedef struct {
  uint64_t kept, copy[4], toM, to0, saturated, crib[5][4];
  uint32_t hashNumber, bits, minShare /* 0 = depth only */, reserved;
} h10x_state_mosh_info;
int  h10x_mosh_from_state(h10x_ctx *ctx, int32_t bits, int32_t copy1min, int32_t copy2min, int32_t copyMmin, h10x_mosh **set, h10x_state_mosh_info *info);

/* ---- from a sequence to its blocks (csrc/stage_p.hip): which blocks' barcode lists hold the hashes of a contig or a long read ----
   State: a loaded, unsharded context with a --hashDepthRange in force; --cluster / --clusterSplit may or may not have run. The blocks are the
   current ones: after --clusterSplit and a new range they are the molecules.
   Hasher: the context's k, w and the seed it learnt through option "seqhash_seed", exactly as h10x_mosh_from_state takes them (the calls that
   hash fail without the seed, or if it does not give the context's factor1).
   Layer 1, sequence -> query list. A sequence s is one byte per base, 0..3, N -> 0 (what h10x_seq_next yields). Its moshes are what
   moshRCiterator / moshRCnext give (seqhash.c:154-195), as h10x_mosh_scan yields them. Each is looked up as hashIndexFind(hash, FALSE)
   (hash10x.c:139-152) in the state's own table: index x, or 0 if absent. Per sequence (h10x_seq_figures): moshes = occurrences; found =
   occurrences with x >= 1, in range or not; query = |Q(s)|, Q(s) = the distinct x >= 1 with hashWithinRange[x], ascending (a mosh that occurs
   twice in s counts once); entries = the sum over Q(s) of hashDepth[x]. A sequence shorter than one window, one of only out-of-range hashes and
   one with no found hash all have an empty Q(s).
   Layer 2, query lists -> rows (the list census). Input: nq lists of hash indices in CSR form (offsets[nq + 1], hashes[]); every index must be
   >= 1 and < hashNumber ("!! listShare list Q entry E: hash index X is not in 1 .. N"). hashWithinRange is NOT applied here: the caller decides
   which hashes go in. count_q[d] = the number of entries d in the barcode lists of the list's hashes, repeats as the lists hold them, a hash given
   twice counted twice. No block is left out: a block of more than 65535 records stands in the lists and so in the rows. The result at minShare =
   T >= 1 is, per list, the row {(d, count_q[d]) : count_q[d] >= T} ascending in d, in CSR form like the share graph. With the good hashes of
   block c as the list (any order) the row is row c of the share graph at T plus the entry (c, sum over x of G[c,x] M[c,x]) if that reaches T; at
   T = 1 the counts of a row sum to the list's entries.
   h10x_seq_hashes is layer 1 for sequences [seqStart[s], seqStart[s + 1]) of codes, s < nSeq, in slabs of option "seq_slab" bases (whole
     sequences; a longer one goes alone); figures[nSeq] may be NULL. The lists stay on the device; h10x_seq_hashes_get copies out offsets[nSeq + 1]
     and the first min(cap, offsets[nSeq]) indices (either may be NULL).
   h10x_list_share_run is layer 2 from host lists: keys (list - first of batch) << bits | d, every (list, hash) unit's place from a scan of the
     unit sizes, a sort on the bits in use (32-bit keys where list and block fit, else 64-bit) and a run pass that keeps runs of length >= T.
     Batches are cut by list entries against "neighbour_budget", a list above it runs alone in windows of block index; both are counted in
     h10x_neighbour_stats. info: rows; listEntries = the entries gathered (the sum of all counts at T = 1); maxCount (0 without rows); batches,
     windows, and wideBatches = the batches that took 64-bit keys; nBlocks; lists = nq; listHashes = offsets[nq].
   h10x_seq_blocks_run is both layers, the lists never leaving the device: row s is the row of Q(s). It keeps the lists as h10x_seq_hashes does
     and the rows as h10x_list_share_run does. figures may be NULL.
   h10x_list_share_get / _get_device copy the kept rows out as h10x_share_graph_get does: offsets[lists + 1] and the first min(cap, rows) rows.
   The result depends on none of "seq_slab", "neighbour_budget", the order in which anything lands, or the run: two calls give the same bytes.
   The kept lists and rows are released by the next run of their kind (also a refused one), h10x_depth_range, h10x_cluster_split, a new state
   and h10x_destroy; get without them fails. These calls neither release nor change a kept share graph, components or --hashCopies result.
   They fail without a state, on a sharded context, before --hashDepthRange and after --clusterSplit until a new range ("!! you must set
   hashDepthRange before seqBlocks" / "listShare" / "seqHashes") and for minShare < 1 ("!! seqBlocks minShare 0 must be >= 1"). */
typedef struct {
  uint32_t moshes, found, query, reserved;
  uint64_t entries;
} h10x_seq_figures;
typedef struct {
  uint64_t rows, listEntries, listHashes;
  uint32_t maxCount, batches, windows, wideBatches, nBlocks, lists;
} h10x_list_share_info;
int  h10x_seq_hashes(h10x_ctx *ctx, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq, h10x_seq_figures *figures);
int  h10x_seq_hashes_get(h10x_ctx *ctx, uint64_t *offsets, uint32_t *hashes, uint64_t cap);
int  h10x_list_share_run(h10x_ctx *ctx, int64_t minShare, const uint64_t *offsets, const uint32_t *hashes, uint32_t nq, h10x_list_share_info *info);
int  h10x_seq_blocks_run(h10x_ctx *ctx, int64_t minShare, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq, h10x_seq_figures *figures,
                         h10x_list_share_info *info);
int  h10x_list_share_get(h10x_ctx *ctx, uint64_t *offsets, uint32_t *block, uint32_t *count, uint64_t cap);
int  h10x_list_share_get_device(h10x_ctx *ctx, uint64_t *dev_offsets, uint32_t *dev_block, uint32_t *dev_count, uint64_t cap);

/* ---- row links (csrc/stage_q.hip): which lists of block numbers share blocks; with the --seqBlocks rows of sequence ends as the lists, which
   contig or long-read ends are covered by the same molecules (--seqLinks) ----
   Input: lists of block numbers in CSR form (offsets[nLists + 1] from 0, block[]), each strictly ascending, every block < nBlocks. They are
   accumulated on the device, numbered 0, 1, .. in the order they are added, however they are cut into calls.
   ends(d) = the number of lists that hold block d. A block is used when maxLists == 0 or ends(d) <= maxLists (the multiplicity cap of the
   linked-read scaffolders: a block in every list would cost ends(d)^2 pairs and says nothing). For lists e < f, shared(e, f) = the number of
   used blocks in both. With siblings != 0 lists 2s and 2s + 1 (the two ends of sequence s) are never linked. The result at minBlocks = M >= 1 is,
   per list e, the row {(f, shared(e, f)) : f > e, shared >= M} ascending in f, in CSR form like the share graph: the upper triangle only.
   h10x_row_links_begin starts an accumulator for blocks < nBlocks and drops an earlier one with its links.
   h10x_row_links_add appends nLists host rows. A list that does not ascend strictly or holds an entry >= nBlocks is refused ("!! rowLinks list Q
     entry E: block X is not ascending" / "... is not below N", Q counted over all lists added) and the call appends nothing.
   h10x_row_links_add_kept appends the rows kept by the last h10x_list_share_run / h10x_seq_blocks_run straight from device memory (their blocks
     ascend and are below the state's nBlocks, which must not exceed the accumulator's); it needs a state with a range in force and kept rows.
   h10x_row_links_finish: every row entry is a key block << listBits | list; a sort makes a block's run the ascending list of its ends; per row
     entry, in (list, block) order, the later members of its block's run are its partners, and the exclusive sum of their numbers places every
     unit (no atomics); one lane per pair writes the key (e - first list of batch) << listBits | f, 32-bit where it fits; a sort and a run pass keep
     the runs of length >= M. Batches are cut by list against "neighbour_budget" (pairs), a list above it runs alone in windows of f; both are
     counted in h10x_neighbour_stats. info: lists, rowEntries, blocksUsed and skippedBlocks (blocks with ends(d) >= 1, by the cap), pairs = the
     keys gathered, links = the result's entries, maxShared (0 without links), batches, windows, wideBatches = the batches that took 64-bit keys.
     It may be called again with other arguments: the accumulator stays. minBlocks < 1: "!! seqLinks minBlocks 0 must be >= 1"; more than
     2^32 - 1 lists (or 2^32 - 2 row entries) are refused.
   h10x_row_links_get / _get_device copy the kept links out as h10x_share_graph_get does: offsets[lists + 1] and the first min(cap, links) entries.
   The result depends on none of the cut into add calls, "neighbour_budget", "seq_slab", the order in which anything lands, or the run: two
   calls give the same bytes. The accumulator and the kept links are released by the next begin (also a refused one), h10x_depth_range,
   h10x_cluster_split, a new state and h10x_destroy. These calls neither release nor change a kept share graph, components, --hashCopies result
   or the lists and rows of h10x_seq_blocks_run. begin, add and finish need a context, not a state; all are refused on a sharded context. */
typedef struct {
  uint64_t lists, rowEntries, blocksUsed, skippedBlocks, pairs, links;
  uint32_t maxShared, batches, windows, wideBatches;
} h10x_row_links_info;
int  h10x_row_links_begin(h10x_ctx *ctx, uint32_t nBlocks);
int  h10x_row_links_add(h10x_ctx *ctx, const uint64_t *offsets, const uint32_t *block, uint64_t nLists);
int  h10x_row_links_add_kept(h10x_ctx *ctx);
int  h10x_row_links_finish(h10x_ctx *ctx, int64_t minBlocks, int64_t maxLists, int32_t siblings, h10x_row_links_info *info);
int  h10x_row_links_get(h10x_ctx *ctx, uint64_t *offsets, uint32_t *other, uint32_t *shared, uint64_t cap);
int  h10x_row_links_get_device(h10x_ctx *ctx, uint64_t *dev_offsets, uint32_t *dev_other, uint32_t *dev_shared, uint64_t cap);
/* links [first, first + count) of the kept result to host memory (either array may be NULL): a writer takes the links in pieces */
int  h10x_row_links_get_range(h10x_ctx *ctx, uint64_t first, uint64_t count, uint32_t *other, uint32_t *shared);

/* ---- sequence spans (csrc/stage_r.hip): where on a sequence each block lies, and how many blocks span each position (--seqSpans) ----
   There is no reference function: hash10x.c knows no sequences beside the crib's. State and hasher as "from a sequence to its blocks" above;
   after --clusterSplit and a new range the blocks are the molecules, and an extent is a molecule's footprint on a contig.
   Hits. The mosh occurrences of sequence s (length L) are those of layer 1 above; occurrence i has position p_i, the 0-based start of its
   k-mer in s. It counts when its hash is found at an index x_i with hashWithinRange[x_i]. Every counting occurrence gives one hit (d, p_i)
   per entry d of the barcode list of x_i, repeats as the list holds them; no block is left out; a hash that occurs twice in s gives hits at
   both positions.
   Extents. Per (s, d) the hits sorted by position: a new extent starts at the first hit and wherever p[j + 1] - p[j] > maxGap (maxGap = 0
   never splits; equal positions never split). An extent is {block, first, last, hits}, kept when hits >= minShare. Row s = its kept extents
   ascending by (block, first); the result is in CSR form, offsets[nSeq + 1] and four uint32 columns.
   Spanning coverage (window W >= 1). The boundaries of s are b_j = j W, j = 1 .. (L - 1) / W (none for L <= W); cover_s[j - 1] = the number
   of kept extents of s with first < b_j <= last: coverOffsets[nSeq + 1] and cover[]. W = 0: no coverage, every offset 0.
   h10x_seq_spans_run: per slab of "seq_slab" bases (whole sequences; a longer one goes alone) a scan, one look-up per occurrence, one unit
     per counting occurrence placed by a scan, a gather of keys block << bits | ordinal in the slab, a sort, head flags where block or sequence
     change or the gap is exceeded, a scan that numbers the extents, a second one that keeps those of minShare hits, a stable sort on the
     sequence and a +1 / -1 difference array over the boundaries with an inclusive scan. Batches are cut by hits against "neighbour_budget", a
     sequence above it runs alone in windows of block index; a batch of 2^32 - 1 hits or more is refused. figures[nSeq] may be NULL:
     inRange = the counting occurrences (not distinct hashes), extents = the row's length. info: sequences, bases, moshes, found, inRange,
     hits = the keys gathered, extentsAll / extents = before / after the threshold, maxHits, maxSpan and sumSpan over last - first of the kept
     extents, boundaries, batches, windows, nBlocks.
   h10x_seq_spans_get copies out offsets[nSeq + 1] and the first min(cap, extents) entries of each column, h10x_seq_spans_get_range rows
     [firstRow, firstRow + count) of the columns, h10x_seq_spans_cover_get coverOffsets[nSeq + 1] and the first min(cap, boundaries) counts; any
     pointer may be NULL.
   The result depends on none of "seq_slab", "neighbour_budget", the order in which anything lands, or the run: two calls give the same bytes.
   The kept result is released by the next run (also a refused one), h10x_depth_range, h10x_cluster_split, a new state and h10x_destroy; get
   without it fails. Refused without a state, on a sharded context, before --hashDepthRange ("!! you must set hashDepthRange before seqSpans"),
   for "!! seqSpans minShare 0 must be >= 1", "!! seqSpans maxGap -1 must be >= 0", "!! seqSpans window -1 must be >= 0", and without the
   hasher's seed as h10x_seq_hashes is. */
typedef struct {
  uint64_t len;
  uint32_t moshes, found, inRange, extents;
} h10x_seq_span_figures;
typedef struct {
  uint64_t sequences, bases, moshes, found, inRange, hits, extentsAll, extents, sumSpan, boundaries;
  uint32_t maxHits, maxSpan, batches, windows, nBlocks, reserved;
} h10x_seq_spans_info;
int  h10x_seq_spans_run(h10x_ctx *ctx, int64_t minShare, int64_t maxGap, int64_t window, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq,
                        h10x_seq_span_figures *figures, h10x_seq_spans_info *info);
int  h10x_seq_spans_get(h10x_ctx *ctx, uint64_t *offsets, uint32_t *block, uint32_t *first, uint32_t *last, uint32_t *hits, uint64_t cap);
int  h10x_seq_spans_get_range(h10x_ctx *ctx, uint64_t firstRow, uint64_t count, uint32_t *block, uint32_t *first, uint32_t *last, uint32_t *hits);
int  h10x_seq_spans_cover_get(h10x_ctx *ctx, uint64_t *coverOffsets, uint32_t *cover, uint64_t cap);

/* ---- sequence spectrum (csrc/stage_s.hip): the hashes of sequences against the read depths of the state (--seqSpectrum) ----
   There is no reference function. State: a loaded, unsharded context, with or without a depth range, before or after --cluster /
   --clusterSplit: only hashDepth[] and the probe table are read. Hasher as "from a sequence to its blocks" above.
   Parameters 0 <= copy1min <= copy2min <= copyMmin and window W >= 0.
   Occurrences. Occurrence i of the moshes of sequence s (length L) has position p_i, the 0-based start of its k-mer, and the index x_i of
   its hash in the state (0: absent; a table entry >= hashNumber counts as absent). Class of an occurrence: absent, or by d = hashDepth[x_i]
   class 0 (d < copy1min), 1 (d < copy2min), 2 (d < copyMmin), else M.
   Per sequence {len; moshes, absent, n0, n1, n2, nM; depthSum = the sum of d over its found occurrences}.
   Windows (W >= 1): window j = 0 .. ceil(L / W) - 1 of s holds the occurrences with p_i / W == j; one record {moshes, absent, n0, n1, n2,
   nM, depthSum} each, in CSR form over the sequences: winOffsets[nSeq + 1]. L = 0 and W = 0 give no windows. The windows of a sequence sum
   field by field to its figures.
   Copies: copies[x], x = 1 .. hashNumber - 1, = the found occurrences with x_i = x over ALL sequences between one begin and its finish.
   Spectrum: S[min(hashDepth[x], H10X_SPECTRUM_DEPTH_BINS - 1)][min(copies[x], H10X_SPECTRUM_COPY_BINS - 1)] counts the hashes x >= 1;
   totals[q] = the hashes of class q = 0, 1, 2, M by the same thresholds, totals[4 + q] = those of them with copies >= 1.
   h10x_seq_spectrum_begin releases a kept result, checks (a refused begin keeps nothing) and zeroes copies[] on the device.
   h10x_seq_spectrum_add: per slab of "seq_slab" bases (whole sequences; a longer one goes alone) the scan, one look-up per occurrence
     (which also adds 1 to copies[x]), a sort by ordinal, and one wave per window and per sequence that finds its occurrences by two searches
     and folds them; no atomic in the tally. figures[nSeq] may be NULL; info = the sums of THIS call. The windows of this call stay on the
     device until the next add; h10x_seq_spectrum_windows_get copies out winOffsets[nSeq + 1] (from 0) and the first min(cap, windows) records.
   h10x_seq_spectrum_finish bins every hash into spectrum[DEPTH_BINS * COPY_BINS] (row = depth bin) and totals[8], closes the run (a later
     add needs a new begin) and fills info with the sums of the whole run and the largest copies[] value. Any pointer but info may be NULL.
   h10x_seq_spectrum_copies_get: copies[first .. first + count) as uint32, from begin until the kept result is released.
   The result depends on none of "seq_slab", how the sequences are split over add calls, the order in which anything lands, or the run.
   The kept result is released by the next begin (also a refused one), h10x_cluster_split, a new state and h10x_destroy; a new depth range
   keeps it. It neither releases nor changes the kept results of the other sequence and share commands. Refused without a state, on a sharded
   context, for "!! seqSpectrum needs 0 <= copy1min <= copy2min <= copyMmin", "!! seqSpectrum window -1 must be >= 0", without the hasher's
   seed as h10x_seq_hashes is; add / windows_get / finish / copies_get without a begin fail, and so does a sequence of more than 2^32 - 1
   windows. */
#define H10X_SPECTRUM_DEPTH_BINS 1024
#define H10X_SPECTRUM_COPY_BINS 8
typedef struct {
  uint64_t len;
  uint32_t moshes, absent, n0, n1, n2, nM;
  uint64_t depthSum;
} h10x_seq_spectrum_figures;                  /* 40 bytes */
typedef struct {
  uint32_t moshes, absent, n0, n1, n2, nM;
  uint64_t depthSum;
} h10x_seq_spectrum_window;                   /* 32 bytes */
typedef struct {
  uint64_t sequences, bases, moshes, absent, n0, n1, n2, nM, depthSum, windows;
  uint32_t hashNumber, maxCopies;
} h10x_seq_spectrum_info;
int  h10x_seq_spectrum_begin(h10x_ctx *ctx, int64_t copy1min, int64_t copy2min, int64_t copyMmin, int64_t window);
int  h10x_seq_spectrum_add(h10x_ctx *ctx, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq, h10x_seq_spectrum_figures *figures,
                           h10x_seq_spectrum_info *info);
int  h10x_seq_spectrum_windows_get(h10x_ctx *ctx, uint64_t *winOffsets, h10x_seq_spectrum_window *records, uint64_t cap);
int  h10x_seq_spectrum_finish(h10x_ctx *ctx, uint64_t *spectrum, uint64_t *totals, h10x_seq_spectrum_info *info);
int  h10x_seq_spectrum_copies_get(h10x_ctx *ctx, uint64_t first, uint64_t count, uint32_t *out);

/* ---- readsets (csrc/stage_h.hip): the Readset object of the reference's moshasm (moshasm.c) over a mosh set ----
   Long reads kept as their mosh hits only: per read the set indices hit, in position order (top bit = the forward hash was strictly
   the smaller, seqhash.c:67), and the 16-bit distance of each hit to the one before it. Read 0 is the reference's burned entry. The
   readset borrows the set: the set must outlive it and must not be changed by other calls while the readset lives. The pairwise
   classification of findOverlaps (moshasm.c:286-365) is computed once per readset, for every directed pair of reads that share a
   first-occurrence copy-1 mosh, and kept on the device; the calls below that depend on the bad flags (moshasm.c:325, 367-371) resolve
   them in read order on the host. Every function returns 0 on success; h10x_readset_error() holds the message otherwise. */
typedef struct h10x_readset h10x_readset;
typedef struct {              /* the 72-byte Read of moshasm.c:31-53 as readsetWrite stores it; the two pointers are always 0 here */
  int32_t  len, nHit;
  uint64_t hitPtr, dxPtr;
  uint8_t  bad, otherFlags;   /* bad: bit 0 repeat, 1 order10, 2 order1, 3 no_match, 4 low_hit, 5 low_copy1 */
  uint16_t pad1;
  int32_t  nMiss, contained;
  int32_t  nCopy[4];
  uint32_t pad2[4];
  uint32_t tail;
} h10x_read_t;
typedef struct {              /* one Overlap of findOverlaps' array (moshasm.c:264-270) with what its RH line prints */
  uint32_t iy; int32_t nHit, offset;
  uint8_t  isPlus, isBad, visited, pad;   /* visited = 0: y was bad when x was looked at, or nHit < 3 (the array's last entry) */
  int32_t  nPlus, nMinus;
  double   d, sd;             /* d /= nHit ; sqrt(d2 / nHit - d * d) (moshasm.c:355) from the device's integer sums */
  int64_t  sumZ, sumZ2;
} h10x_overlap_t;
typedef struct { uint32_t nReads /* arrayMax: read 0 included */, dim /* of the reference's reads array */; uint64_t totHit; } h10x_readset_info_t;
/* readsetCreate + the start of readsetFileRead (moshasm.c:65-73, 132): an empty readset; the set's depth[] is zeroed, to be rebuilt
   from the sequences added */
int  h10x_readset_create(h10x_readset **rs, h10x_mosh *set);
/* the loop of readsetFileRead (moshasm.c:135-160) over sequences as for h10x_mosh_add; a read with more than 65534 hits is refused */
int  h10x_readset_add(h10x_readset *rs, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq);
/* readsetRead's state (moshasm.c:102-123) from the arrays of a parsed RSMSHv2 file: nReads records, hit / dx of all reads back to
   back in read order. The set's depth[] is kept and must be the one this readset gave it: checked (invBuild, moshasm.c:232-260) */
int  h10x_readset_load(h10x_readset **rs, h10x_mosh *set, const h10x_read_t *reads, uint32_t nReads, uint32_t dim, const uint32_t *hit,
                       const uint16_t *dx);
void h10x_readset_destroy(h10x_readset *rs);                                         /* readsetDestroy (moshasm.c:75-82) */
const char *h10x_readset_error(const h10x_readset *rs);
int  h10x_readset_info(h10x_readset *rs, h10x_readset_info_t *out);
/* the number of chunks of queries the overlap table was built in (options "overlap_chunk", "overlap_chunk_reads" of the set); 0 while
   the readset has no table (before the first overlaps / mark_bad / mark_contained call, and again after h10x_readset_add). A chunk
   of reads that meet no inverse-list entry is not counted: it holds nothing. */
int  h10x_readset_chunks(h10x_readset *rs, uint32_t *nChunks);
/* what readsetWrite stores (moshasm.c:84-100), nCopy as invBuild leaves it: pointers into the object, valid until the next call that
   changes it; hitStart[i] .. hitStart[i + 1] are read i's entries of hit / dx */
int  h10x_readset_export(h10x_readset *rs, const h10x_read_t **reads, const uint64_t **hitStart, const uint32_t **hit, const uint16_t **dx);
/* findOverlaps (rs, read ix, ..) (moshasm.c:286-384): its side effects on the flags of read ix, the array it returns (at most
   h10x_readset_overlap_cap(rs, ix) entries, sorted by descending nHit, ties in the order first met) and nRepeat, nGood, nBad */
int  h10x_readset_overlap_cap(h10x_readset *rs, uint32_t ix, uint32_t *cap);
int  h10x_readset_overlaps(h10x_readset *rs, uint32_t ix, h10x_overlap_t *out, uint32_t cap, uint32_t *n, int32_t counts3[3]);
/* markBadReads (moshasm.c:436-461): found3 = the reads each of the three passes marks */
int  h10x_readset_mark_bad(h10x_readset *rs, int32_t found3[3]);
/* markContained (moshasm.c:471-497) */
int  h10x_readset_mark_contained(h10x_readset *rs, int32_t *nContained, int32_t *nNotContained, uint64_t *totLenNotContained);
/* the per-class sums of readsetStats' last line (moshasm.c:216-224): nCopy[4], hitCopy[4], hit2Copy[4], depthCopy[4] */
int  h10x_readset_stats_sums(h10x_readset *rs, uint64_t out16[16]);

/* ---- reference maps (csrc/stage_i.hip): the Reference object of the reference's moshmap (moshmap.c) over a mosh set ----
   Reference sequences kept as their mosh hits: per hit in file order index (the set index), offset (position of the k-mer) and id
   (sequence number); per set index a 32-bit depth; once packed, loc[] (where an index's hits start in rev[]) and rev[] (the hit
   ordinals of each index, ascending). The map borrows the set, as a readset does. Sequence names and lengths are the caller's
   (host/map_host.c keeps the reference's DICT). Every function returns 0 on success; h10x_refmap_error() holds the message otherwise —
   the reference's die() text where it would have died ("reference size overflow", moshmap.c:109). */
typedef struct h10x_refmap h10x_refmap;
typedef struct { uint32_t size /* ref->size */, max /* ref->max: hits */, setMax /* ms->max */; int32_t packed; } h10x_refmap_info_t;
typedef struct {              /* one seed of a query, resolved: class = idClass >> 30 (0 = not in the set, 1, 2, 3 = M); for class 1 and 2 */
  uint32_t loc, loc2;         /* loc = rev[loc[index]], and for class 2 loc2 = rev[loc[index] + 1] (moshmap.c:217, 224)                 */
  uint32_t idClass, id2;      /* idClass & 0x3fffffff = id[loc]; id2 = id[loc2]                                                       */
} h10x_mapseed_t;
typedef struct {              /* what one M line is printed from (moshmap.c:255-260, 267-272)                                          */
  uint32_t pos0, posN;        /* positions in the query of seeds i0 and iN                                                           */
  uint32_t loc0, locN, n1, n2, query;
} h10x_maprec_t;
/* referenceCreate (moshmap.c:48-63) over a set that moshsetCreate left: its 16-bit depths must all be 0 (checked here and by every
   h10x_refmap_add, which fail otherwise); the program passes size = 1 << 26. Destroy the map before its set. */
int  h10x_refmap_create(h10x_refmap **rm, h10x_mosh *set, uint32_t size);
/* the loop of referenceFastaRead (moshmap.c:99-119) over sequences as for h10x_mosh_add: every mosh is found or added in file order
   (the numbering and the table of h10x_mosh_add), appended as (index, position, idBase + sequence number) and counted in the 32-bit
   depth. The set's own 16-bit depth[] stays 0. *nHits = hits appended by this call. */
int  h10x_refmap_add(h10x_refmap *rm, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq, uint32_t idBase, uint64_t *nHits);
/* the rest of referenceFastaRead and referencePack (moshmap.c:73-90, 124-132): copy classes from the 32-bit depth (1, 2, else M)
   into the set's info, loc[], rev[] */
int  h10x_refmap_pack(h10x_refmap *rm, uint32_t *n1, uint32_t *n2, uint32_t *nM);
/* referenceRead's state (moshmap.c:157-181) from the arrays of a parsed RFMSHv1 file: index / offset / id / rev of max entries, depth /
   loc of the set's max + 1. Checked again here: loc is the running sum of depth and ends within max, every index within the set,
   id < nIds, rev < max, and no index of the set with copy class 0 (-f leaves none; the reference would walk it as copy 2) or copy-1 /
   copy-2 with fewer than 1 / 2 hits. */
int  h10x_refmap_load(h10x_refmap **rm, h10x_mosh *set, const uint32_t *index, const uint32_t *offset, const uint32_t *id, const uint32_t *depth, const uint32_t *rev,
                      const uint32_t *loc, uint32_t max, uint32_t nIds);
void h10x_refmap_destroy(h10x_refmap *rm);
const char *h10x_refmap_error(const h10x_refmap *rm);
int  h10x_refmap_info(const h10x_refmap *rm, h10x_refmap_info_t *out);
/* what referenceWrite stores (moshmap.c:143-150) of a packed map: pointers into the object, valid while it lives */
int  h10x_refmap_export(h10x_refmap *rm, const uint32_t **index, const uint32_t **offset, const uint32_t **id, const uint32_t **depth, const uint32_t **rev, const uint32_t **loc);
/* queryProcess (moshmap.c:187-278) over query sequences as for h10x_mosh_add. The results stay in the object until the next query:
   counts4[4 q ..] = missed, copy 1, copy 2, multi of query q; recs[recStart[q] .. recStart[q + 1]) its M records in the order the
   reference prints them; with wantSeeds != 0 also seeds / seedPos [seedStart[q] .. seedStart[q + 1]), every mosh of q in order (the -v
   lines, moshmap.c:219-229). */
int  h10x_refmap_query(h10x_refmap *rm, const uint8_t *codes, const uint64_t *seqStart, uint32_t nSeq, int wantSeeds);
int  h10x_refmap_results(h10x_refmap *rm, uint32_t *nQueries, const uint32_t **counts4, const uint64_t **recStart, const h10x_maprec_t **recs, const uint64_t **seedStart,
                         const h10x_mapseed_t **seeds, const uint32_t **seedPos);

/* ---- device memory plumbing for callers that keep the input resident in HBM (bench, pipelines) ----
   plain hipMalloc / hipMemcpy / hipDeviceSynchronize on `device`; return NULL / non-zero on failure */
void *h10x_device_malloc(int device, uint64_t bytes);
/* free and total bytes of the device's memory as the driver sees them (hipMemGetInfo; blocks parked in the library's cache count as used) */
int   h10x_device_mem_info(int device, uint64_t *freeBytes, uint64_t *totalBytes);
int   h10x_device_free(int device, void *ptr);
int   h10x_device_upload(int device, void *dst, const void *src, uint64_t bytes);
int   h10x_device_download(int device, void *dst, const void *src, uint64_t bytes);
int   h10x_device_synchronize(int device);

/* ---- measurement hooks (not part of the reference surface) ----
   Per-kernel device timings collected with hipEvents on the context's stream when enabled.
   names: "mosh_extract", "sort_by_hash", ..., "good_hashes", "cluster" (whole command), "cluster_kernel" (all device work of
   --cluster), "cluster_main" (the main cluster_kernel launch alone) ... (h10x_timing_name(i)). */
int  h10x_timing_enable(h10x_ctx *ctx, int on);
int  h10x_timing_count(const h10x_ctx *ctx);
const char *h10x_timing_name(const h10x_ctx *ctx, int i);
int  h10x_timing_get(h10x_ctx *ctx, int i, double *total_ms, uint64_t *launches);
int  h10x_timing_reset(h10x_ctx *ctx);
/* The exchanges of a sharded context, per kind of collective (names: h10x_exchange_name(i), i < h10x_exchange_count()): calls; bytes this rank sent to and received
   from OTHER ranks; maxPeerOut = the sum over the calls of the largest share one peer received (grouped point-to-point sends: what one xGMI link carried); ms = from
   each call to its completion on the context's stream, waits for slower ranks included (collected while timing is enabled; a rank's compute is its stage timers less
   these). Cleared by h10x_timing_reset. What `bench.py --scaling strong` and `--virtual-ranks` print so that a scaling curve can be read. */
/* sharded contexts: the part of stage timer i (h10x_timing_name) spent inside exchanges — waiting for other ranks and moving bytes; the stage's own compute is the rest */
int  h10x_timing_wait_get(h10x_ctx *ctx, int i, double *ms);
int  h10x_exchange_count(void);
const char *h10x_exchange_name(int i);
int  h10x_exchange_get(h10x_ctx *ctx, int i, uint64_t *calls, uint64_t *bytesOut, uint64_t *bytesIn, uint64_t *maxPeerOut, double *ms, double *msInStages);
/* the stage timer (index for h10x_timing_name) whose kernels ran on the main stream while exchange kind i was on the context's exchange stream, -1 if it ran on the main
   stream with nothing beside it (option "shard_overlap" 0: always) */
int  h10x_exchange_beside(h10x_ctx *ctx, int i);
/* algorithmic work counters of the last commands: see DESIGN.md */
typedef struct {
  uint64_t pairs;            /* read pairs hashed                                   */
  uint64_t kmers;            /* k-mers hashed (237 per pair at k=21)                */
  uint64_t entries;          /* H = sum nHash                                       */
  uint64_t distinct;         /* U = hashNumber - 1                                  */
  uint64_t clustered_codes;  /* barcodes visited by the last h10x_cluster           */
  uint64_t sum_good;         /* sum of good hashes over those barcodes              */
  uint64_t sum_good_depth;   /* sum over good hashes of depth (gathered row entries)*/
  uint64_t sum_hash_clustered; /* sum nHash over barcodes with good hashes          */
  uint64_t fallback_blocks;  /* barcodes that took the global-memory path in stage A */
  uint64_t cluster_class_counts[4]; /* barcodes clustered in: half-CU LDS with 1024 lanes, half-CU LDS with 512 lanes, full-CU LDS (512 lanes), HBM scratch */
  uint64_t cluster_first_mode;     /* placement of the first[] table: 0 dense in LDS, 1 ranked (bitmap) in LDS, 2 per-workgroup HBM slot, 4 translated (16-bit handles into a table in LDS) */
  uint64_t cluster_overflow_blocks; /* ranked placement: barcodes re-run on the HBM path because too many barcodes were present */
  uint64_t cluster_main[4];        /* work of the main cluster launch alone (timer "cluster_main"): good hashes, gathered list entries, nHash, barcodes */
  uint64_t cluster_phase_ticks[8]; /* diagnostic (option "cluster_stamps"): 100 MHz ticks per phase summed over workgroups:
                                      [0] init (+ bitmap), [1] list loop, [2] barrier, [3] replay, [4] quotient, [5] output */
  uint64_t list_words[2];          /* sharded --hashDepthRange: 32-bit words of in-range barcode lists this rank received, [0] as plain
                                      numbers, [1] as they travelled (delta-coded: option "shard_delta_lists"); 0 0 if sent plain */
  uint64_t index_table_form;       /* single-GPU index build, the look-up table behind the ClusterHash records: 0 = hashIndex[] + hashValue[] (or the library's private table: option
                                      "index_priv_table"), 1 = the wide table, entry = index | hash / w, 2 = the wide table in the probed format (index | hash >> B | probe number:
                                      -B 29 / 30 at k = 21), 3 = the probed table failed and the round-5 pair was built (option "index_probed_table") */
  uint64_t shard_reply_path;       /* sharded --readFQB, how this hash owner answered its entries: 0 nothing to answer, 1 by look-up, 2 by scatter, 3 by scatter after a look-up
                                      that failed or did not fit (option "shard_reply_sort") */
} h10x_counters;
int  h10x_get_counters(h10x_ctx *ctx, h10x_counters *out);
/* the device batches of h10x_seq_hashes / h10x_seq_blocks_run, since the context was made, whose list of moshes overflowed its estimated size
   and were scanned a second time at the exact size (h10x_mosh_counters_t.scan_retries for a context) */
int  h10x_get_scan_retries(h10x_ctx *ctx, uint64_t *out);
/* test / tuning knobs (none changes a result): "stage_a_max_slots" caps the LDS hash-set slots per barcode in stage A (0 =
   default) so that the global-memory fallback can be exercised on small inputs; "chunk_size" (above); "index_no_pack" 1 = index
   build with separate key / block arrays even where the packed one-word entries fit; "index_probed_table" 0 default = the wide look-up table takes the probed entry format
   (index | hash >> B | probe number, in the reference's own geometry: hashIndex[] is its index column) where index | hash / w does not fit 64 bits, 1 = always, 2 = never (two
   tables, as round 5 built them), 3 = always and with one bit of probe number (exercises the fall-back; h10x_counters.index_table_form says what was built); "index_priv_table" 1 = the entry look-ups of the
   index build through the library's own one-read table also where the reference-shaped 64-bit table fits (default 0: only where it
   does not, i.e. -B 29 / 30 at k = 21), 2 = never, 3 = always and undersized (exercises its fall-back); "cluster_narrow_first" 1 = first[] of the
   cluster kernel at 2 bytes per entry in every block, w >= 2 = 4 bytes down to w list-loop waves (default 0: 4 bytes where that
   costs no wave); "cluster_tr_packed" (translated placement of first[]: -1 / 1 = several lists per wave instruction, the default; 0 = round 4's
   one list per wave instruction), "cluster_tr_class_t" (packed form: -1 / 1 = lists of 65 .. 96 entries run two to a unit of three chunks, the default; 0 = one to a
   unit of two chunks like the lists of 97 .. 128), "cluster_lds_budget", "cluster_first_global", "cluster_first_cap", "cluster_big_ranks", "cluster_threads0",
   "cluster_budget0" (placement and launch-class overrides of the tests), "cluster_stamps" (phase stamps into h10x_counters),
   "shard_reply_sort" (sharded index build: 0 default = a hash owner answers by look-up in a table of its distinct hashes, 1 = by scattering from its sorted order; tests of the
   fall-back, reported in h10x_counters.shard_reply_path: 2 = look up, then scatter all the same, 3 = a look-up table that fails, 4 = one that does not fit),
   "shard_overlap" (1 default = the exchanges whose result a later stage needs — the in-range barcode lists, hashDepth[] of the other owners — run on an exchange stream beside
   the main stream's kernels; 0 = every exchange on the main stream),
   "shard_owner_cut" (0 default = hash owners' value ranges cut at the quantiles of the canonical-hash density, equal shares; 1 = equal value ranges),
   "shard_row_shift", "shard_rows_fake_base" (sharded list offsets beyond 32 bits on small inputs), "shard_delta_lists" (-1 default:
   the in-range barcode lists travel delta-coded where bytes are dear — more than one rank on the host-staged TCP backend, not over xGMI; 0 never; 1 always),
   "neighbour_budget" (gathered ClusterHash records per batch of the neighbour census; 0 = default 2^26; small values force batches and hash-index windows),
   "molmap_global" (1 = the molecule map keeps the first-clustered-position table of every clustered block in device memory, also where it fits LDS: tests of that form),
   "fqb_slab" (records per device batch of h10x_census_add / h10x_fix_fqb and of the session's --codeCensus / --fixFQB / --fixFQBThresh; 0 = default 2^20),
   "seq_slab" (bases per device batch of h10x_seq_hashes / h10x_seq_blocks_run; 0 = default 2^26; results do not depend on it).
   Not a knob: "seqhash_seed" = the -r value params.factor1 was drawn from (h10x_factor1_from_seed); h10x_mosh_from_state needs it for the second multiplier of the
   set's header, and the session layer sets it. Unknown name: -1. */
int  h10x_set_option(h10x_ctx *ctx, const char *name, int64_t value);

#ifdef __cplusplus
}
#endif
#endif /* H10X_H */
