/* files_host.c — the files of the project's own formats, written from host arrays and callbacks: .mol, .idx, .sg, .sc, .hc, .sb, .sl and the whitelist text
   (layouts: h10x_host.h). Nothing here touches a h10x_ctx or a session and nothing needs the device library, so all of it runs under sanitizers on a machine
   without a GPU (the *_asan_driver.c programs). Every writer goes through OutFile: an output appears under its name only when it is whole. */
#define _GNU_SOURCE
#include "files_host.h"
#include <math.h>
#include <stdlib.h>
#include <string.h>

const char *const cribTypeName[5] = {"err", "htA", "htB", "hom", "mul"};

/* ---- OutFile (files_host.h): the one place that builds the .part name ---- */
static int out_fail(const OutFile *o, const char *fmt) { if (o->err) snprintf(o->err, (size_t)o->errlen, fmt, o->path); return -1; }
int h10x_out_open(OutFile *o, const char *path, char *err, int errlen) {
  memset(o, 0, sizeof *o); o->path = path; o->err = err; o->errlen = errlen;
  const size_t n = strlen(path);
  if ((o->tmp = (char *)malloc(n + 6))) { memcpy(o->tmp, path, n); memcpy(o->tmp + n, ".part", 6); o->f = fopen(o->tmp, "wb"); }
  if (o->f) return 0;
  free(o->tmp); o->tmp = 0;                                                          /* nothing was created: nothing for abort to remove */
  return out_fail(o, "failed to open output file %s");
}
int h10x_out_probe(OutFile *o, const char *path, char *err, int errlen) {
  if (h10x_out_open(o, path, err, errlen)) return -1;
  fclose(o->f); o->f = 0;
  return 0;
}
int h10x_out_write(OutFile *o, const void *p, size_t size, size_t n) { return !n || fwrite(p, size, n, o->f) == n ? 0 : out_fail(o, "failed to write %s"); }
int h10x_out_rewrite(OutFile *o, const void *p, size_t n) { return !fseeko(o->f, 0, SEEK_SET) && fwrite(p, 1, n, o->f) == n ? 0 : out_fail(o, "failed to write %s"); }
void h10x_out_abort(OutFile *o) {
  if (o->f) { fclose(o->f); o->f = 0; }
  if (o->tmp) { remove(o->tmp); free(o->tmp); o->tmp = 0; }
}
int h10x_out_commit(OutFile *o) {
  int ok = o->tmp != 0;
  if (o->f) { if (fclose(o->f)) ok = 0; o->f = 0; }                                    /* (buffered bytes that do not fit the disk fail here) */
  if (ok && rename(o->tmp, o->path)) ok = 0;
  if (!ok) { h10x_out_abort(o); return out_fail(o, "failed to write %s"); }
  free(o->tmp); o->tmp = 0;
  return 0;
}

/* ---- the small shared pieces ---- */
int h10x_grow(void **p, size_t *cap, size_t need, size_t elt) {
  if (need <= *cap) return 0;
  size_t n = *cap ? *cap : 64; while (n < need) n *= 2;
  void *q = realloc(*p, n * elt); if (!q) return -1;
  *p = q; *cap = n;
  return 0;
}
int h10x_names_add(NameTable *t, const char *name) {
  const size_t nl = strlen(name) + 1;
  if (h10x_grow((void **)&t->off, &t->capOff, (size_t)t->n + 2, 8) || h10x_grow((void **)&t->bytes, &t->capBytes, (size_t)t->nBytes + nl, 1)) return -1;
  memcpy(t->bytes + t->nBytes, name, nl);
  t->off[t->n] = t->nBytes; t->nBytes += nl; t->off[++t->n] = t->nBytes;
  return 0;
}
void h10x_names_free(NameTable *t) { free(t->bytes); free(t->off); memset(t, 0, sizeof *t); }
static void interleave_u32(uint32_t *pair, const uint32_t *a, const uint32_t *b, uint64_t n) { for (uint64_t i = 0; i < n; ++i) { pair[2 * i] = a[i]; pair[2 * i + 1] = b[i]; } }
/* a header under construction: every format starts with its four letters and u32 version 1, all values little-endian */
typedef struct { unsigned char *p; size_t n; } Head;
static void put_u32(Head *h, uint32_t v) { memcpy(h->p + h->n, &v, 4); h->n += 4; }
static void put_u64(Head *h, uint64_t v) { memcpy(h->p + h->n, &v, 8); h->n += 8; }
static Head head_start(unsigned char *p, const char *magic) { Head h = {p, 4}; memcpy(p, magic, 4); put_u32(&h, 1); return h; }
static int put_err(char *err, int errlen, const char *fmt, unsigned long long v) { if (err) snprintf(err, (size_t)errlen, fmt, v); return -1; }
static const uint64_t zero64 = 0;                                                      /* the offsets of no sequences */

/* ---- .mol and .idx: --moleculeMap, --splitFQB ---- */
int h10x_host_write_molmap(const char *path, const uint32_t *mol, const uint32_t *slot, const h10x_molmap_info *info, char *err, int errlen) {
  enum { RUN = 1 << 16 };
  OutFile o; unsigned char head[32]; Head h = head_start(head, "10XM");
  put_u64(&h, info->nRecords); put_u32(&h, info->nBlocks); put_u32(&h, info->nMolecules); put_u64(&h, info->nClustered);
  if (h10x_out_open(&o, path, err, errlen)) return -1;
  uint32_t *pair = (uint32_t *)malloc((size_t)RUN * 8);
  int rc = pair ? h10x_out_write(&o, head, 1, h.n) : out_fail(&o, "out of host memory writing %s");
  for (uint64_t at = 0; !rc && at < info->nRecords; at += RUN) {
    const uint64_t m = info->nRecords - at < RUN ? info->nRecords - at : RUN;
    interleave_u32(pair, mol + at, slot + at, m);
    rc = h10x_out_write(&o, pair, 8, (size_t)m);
  }
  if (!rc) rc = h10x_out_commit(&o);
  h10x_out_abort(&o); free(pair);
  return rc;
}
int h10x_host_write_split_index(const char *path, const uint64_t *start, uint32_t nBlocks, uint32_t nMolecules, char *err, int errlen) {
  OutFile o; unsigned char head[16]; Head h = head_start(head, "10XS");
  put_u32(&h, nBlocks); put_u32(&h, nMolecules);
  if (h10x_out_open(&o, path, err, errlen)) return -1;
  const int rc = h10x_out_write(&o, head, 1, h.n) || h10x_out_write(&o, start, 8, (size_t)nBlocks + nMolecules + 1) || h10x_out_commit(&o) ? -1 : 0;
  h10x_out_abort(&o);
  return rc;
}

/* ---- the whitelist text as fq2b-amd reads it (read10xWhitelist, fq2b.c:71-94): blank-separated words of 16 characters in line order ---- */
int h10x_host_whitelist_read(const char *path, uint32_t **codes, uint64_t *n, char *err, int errlen) {
  uint8_t sym[256]; memset(sym, 0, 256); sym['c'] = sym['C'] = 1; sym['g'] = sym['G'] = 2; sym['t'] = sym['T'] = 3;   /* a, A, N, anything else: 0 (fq2b.c:27-28) */
  *codes = 0; *n = 0;
  FILE *f = fopen(path, "r");
  if (!f) { if (err) snprintf(err, (size_t)errlen, "failed to open 10x whitelist file %s\n", path); return -1; }
  size_t cap = 1 << 16, m = 0; uint32_t *c = (uint32_t *)malloc(cap * 4);
  char word[64]; int rc = 0;
  while (c && fscanf(f, "%63s", word) == 1) {
    if (strlen(word) != 16) { if (err) snprintf(err, (size_t)errlen, "bad barcode line %d in %s: %s", (int)m + 1, path, word); rc = -1; break; }
    if (m == cap) { cap *= 2; uint32_t *c2 = (uint32_t *)realloc(c, cap * 4); if (!c2) { free(c); c = 0; break; } c = c2; }
    uint32_t v = 0; for (int i = 0; i < 16; ++i) v = (v << 2) | sym[(unsigned char)word[i]];
    c[m++] = v;
  }
  fclose(f);
  if (!c) { if (err) snprintf(err, (size_t)errlen, "out of host memory for the whitelist"); return -1; }
  if (rc) { free(c); return rc; }
  *codes = c; *n = m;
  return 0;
}
void h10x_host_whitelist_free(uint32_t *codes) { free(codes); }
int h10x_host_whitelist_write(const char *path, const uint32_t *codes, uint64_t n, char *err, int errlen) {
  OutFile o; if (h10x_out_open(&o, path, err, errlen)) return -1;
  char line[17]; line[16] = '\n'; int rc = 0;
  for (uint64_t i = 0; !rc && i < n; ++i) {
    for (int b = 0; b < 16; ++b) line[15 - b] = "ACGT"[(codes[i] >> (2 * b)) & 3];     /* uSeq (fq2b.c:44-50) */
    rc = h10x_out_write(&o, line, 1, 17);
  }
  if (!rc) rc = h10x_out_commit(&o);
  h10x_out_abort(&o);
  return rc;
}
/* the line a barcode is looked up under: the LAST line that holds it (later lines overwrite earlier ones in the reference's byte table, fq2b.c:89), 0 = absent */
static int cmp_u64(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return x < y ? -1 : x > y; }
int h10x_host_whitelist_lines(const uint32_t *codes, uint64_t n, const uint32_t *query, uint64_t nq, uint32_t *lines) {
  uint64_t *k = (uint64_t *)malloc((n ? n : 1) * 8);
  if (!k) return -1;
  for (uint64_t i = 0; i < n; ++i) k[i] = (uint64_t)codes[i] << 32 | (uint32_t)(i + 1);
  qsort(k, n, 8, cmp_u64);
  for (uint64_t q = 0; q < nq; ++q) {                                                 /* the last entry of the barcode's run = its largest line */
    const uint64_t top = (uint64_t)query[q] << 32 | 0xFFFFFFFFu;
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (k[mid] <= top) lo = mid + 1; else hi = mid; }
    lines[q] = lo && (uint32_t)(k[lo - 1] >> 32) == query[q] ? (uint32_t)k[lo - 1] : 0;
  }
  free(k);
  return 0;
}

/* ---- .sg: --shareGraph. The rows come range by range, so nobody holds them all: the header and the offsets are left blank first and filled in at the end. ---- */
int h10x_host_write_share_graph(const char *path, uint32_t nBlocks, uint32_t minShare, uint32_t rangeBlocks, h10x_share_graph_range_fn range, void *user,
                                uint64_t *rowsOut, char *err, int errlen) {
  const uint32_t step = rangeBlocks ? rangeBlocks : 8192u; const size_t nOff = (size_t)nBlocks + 1;
  uint64_t *offsets = (uint64_t *)calloc(nOff, 8); uint32_t *pair = 0; size_t capPair = 0; uint64_t rows = 0;
  if (!offsets) return put_err(err, errlen, "out of host memory for the offsets of %llu blocks", nBlocks);
  OutFile o; unsigned char head[24]; memset(head, 0, sizeof head);
  if (h10x_out_open(&o, path, err, errlen)) { free(offsets); return -1; }
  int rc = h10x_out_write(&o, head, 1, sizeof head) || h10x_out_write(&o, offsets, 8, nOff) ? -1 : 0;
  for (uint32_t c0 = 0; !rc && c0 < nBlocks; c0 += step) {             /* (block 0 is unused: its row is empty) */
    const uint32_t c1 = nBlocks - c0 < step ? nBlocks : c0 + step;
    h10x_share_graph_range r; memset(&r, 0, sizeof r);
    if (range(user, c0, c1, &r)) { rc = -2; break; }                   /* the callback's own error stands */
    if (h10x_grow((void **)&pair, &capPair, (size_t)r.rows, 8)) { rc = put_err(err, errlen, "out of host memory for %llu rows", r.rows); break; }
    for (uint32_t q = 0; q <= c1 - c0; ++q) offsets[c0 + q] = rows + r.part[q];
    interleave_u32(pair, r.blk, r.cnt, r.rows);
    rc = h10x_out_write(&o, pair, 8, (size_t)r.rows);
    rows += r.rows;
  }
  Head h = head_start(head, "10XG"); put_u32(&h, nBlocks); put_u32(&h, minShare); put_u64(&h, rows);
  if (!rc) rc = h10x_out_rewrite(&o, head, h.n) || h10x_out_write(&o, offsets, 8, nOff) || h10x_out_commit(&o) ? -1 : 0;
  h10x_out_abort(&o); free(offsets); free(pair);
  if (!rc && rowsOut) *rowsOut = rows;
  return rc;
}

/* ---- .sc: --shareComponents ---- */
int h10x_host_write_share_components(const char *path, const h10x_share_components_info *info, const uint32_t *comp, const uint32_t *rootOf,
                                     const uint32_t *blocks, const uint64_t *records, char *err, int errlen) {
  OutFile o; unsigned char head[32]; Head h = head_start(head, "10XC");
  put_u32(&h, info->nBlocks); put_u32(&h, info->minShare); put_u32(&h, info->nComponents); put_u32(&h, info->largest); put_u64(&h, info->rows);
  if (h10x_out_open(&o, path, err, errlen)) return -1;
  int rc = h10x_out_write(&o, head, 1, h.n) || h10x_out_write(&o, comp, 4, info->nBlocks) ? -1 : 0;
  for (uint32_t k = 0; !rc && k <= info->nComponents; ++k) {
    unsigned char entry[16]; Head e = {entry, 0};
    put_u32(&e, rootOf[k]); put_u32(&e, blocks[k]); put_u64(&e, records[k]);
    rc = h10x_out_write(&o, entry, 1, e.n);
  }
  if (!rc) rc = h10x_out_commit(&o);
  h10x_out_abort(&o);
  return rc;
}

/* ---- .hc: --hashCopies. The table is fetched and written in slabs, so the host never holds it. ---- */
int h10x_host_write_hash_copies(const char *path, const h10x_hash_copies_info *info, h10x_hash_copies_slab_fn slab, void *user, uint64_t slabHashes,
                                char *err, int errlen) {
  if (!slabHashes) slabHashes = (uint64_t)1 << 22;
  const uint64_t n = info->hashNumber, cap = n < slabHashes ? (n ? n : 1) : slabHashes;
  uint16_t *buf = (uint16_t *)malloc((size_t)cap * 8);
  if (!buf) return put_err(err, errlen, "out of host memory for a slab of %llu hashes", cap);
  OutFile o; unsigned char head[32]; Head h = head_start(head, "10XK");
  put_u32(&h, info->hashNumber); put_u32(&h, info->minShare); put_u64(&h, info->inRange); put_u64(&h, info->rows);
  if (h10x_out_open(&o, path, err, errlen)) { free(buf); return -1; }
  int rc = h10x_out_write(&o, head, 1, h.n);
  for (uint64_t first = 0; !rc && first < n; first += cap) {
    const uint64_t count = n - first < cap ? n - first : cap;
    if (slab(user, buf, first, count)) rc = -2;                       /* the callback's own error stands */
    else rc = h10x_out_write(&o, buf, 8, (size_t)count);
  }
  if (!rc) rc = h10x_out_commit(&o);
  h10x_out_abort(&o); free(buf);
  return rc;
}

/* ---- .sb: --seqBlocks. Three parts: the rows of each slab go to the file as they come; the per-sequence table, the offsets and the names are kept on the
   host and written at the end, with the header. ---- */
int h10x_host_write_seq_blocks(const char *path, uint32_t nBlocks, uint32_t minShare, h10x_seq_blocks_slab_fn next, void *user, FILE *verbose,
                               h10x_seq_blocks_totals *totals, char *err, int errlen) {
  typedef struct { uint64_t len; uint32_t moshes, found, query, reserved; } Rec;
  h10x_seq_blocks_totals t; memset(&t, 0, sizeof t);
  Rec *table = 0; uint64_t *offsets = 0; uint32_t *pair = 0; NameTable names; memset(&names, 0, sizeof names);
  size_t capTable = 0, capOff = 0, capPair = 0;
  OutFile o; unsigned char head[40]; memset(head, 0, sizeof head);
  if (h10x_out_open(&o, path, err, errlen)) return -1;
  int rc = h10x_out_write(&o, head, 1, sizeof head);
  while (!rc) {
    h10x_seq_blocks_slab b; memset(&b, 0, sizeof b);
    const int got = next(user, &b);
    if (got < 0) { rc = -2; break; }                                  /* the callback's own error stands */
    if (!got) break;
    const uint64_t rows = b.nSeq ? b.rowOff[b.nSeq] : 0;
    if (h10x_grow((void **)&table, &capTable, (size_t)(t.nSeq + b.nSeq), sizeof(Rec)) || h10x_grow((void **)&offsets, &capOff, (size_t)(t.nSeq + b.nSeq + 1), 8) ||
        h10x_grow((void **)&pair, &capPair, (size_t)rows, 8)) goto no_memory;
    offsets[0] = 0;
    interleave_u32(pair, b.block, b.count, rows);
    if ((rc = h10x_out_write(&o, pair, 8, (size_t)rows))) break;
    for (uint32_t q = 0; q < b.nSeq; ++q) {
      const uint64_t at = t.nSeq + q, len = b.seqStart[q + 1] - b.seqStart[q], r0 = b.rowOff[q], r1 = b.rowOff[q + 1];
      const h10x_seq_figures *g = b.fig + q;
      Rec rec = {len, g->moshes, g->found, g->query, 0};
      table[at] = rec;
      offsets[at + 1] = t.rows + r1;
      const char *name = b.names + b.nameOff[q];
      if (h10x_names_add(&names, name)) goto no_memory;
      uint32_t best = 0, bestCount = 0;
      for (uint64_t i = r0; i < r1; ++i) if (b.count[i] > bestCount) { bestCount = b.count[i]; best = b.block[i]; }
      if (verbose) fprintf(verbose, "SEQ_BLOCKS  %s len %llu moshes %u found %u query %u rows %llu best %u count %u\n", name, (unsigned long long)len,
                           g->moshes, g->found, g->query, (unsigned long long)(r1 - r0), best, bestCount);
      t.bases += len; t.moshes += g->moshes; t.found += g->found; t.query += g->query;
      if (r1 > r0) ++t.withRows;
      if (bestCount > t.maxCount) t.maxCount = bestCount;
    }
    t.nSeq += b.nSeq; t.rows += rows;
  }
  if (!rc) {
    Head h = head_start(head, "10XQ"); put_u32(&h, nBlocks); put_u32(&h, minShare); put_u64(&h, t.nSeq); put_u64(&h, t.rows); put_u64(&h, names.nBytes);
    rc = h10x_out_write(&o, table, sizeof(Rec), (size_t)t.nSeq) || h10x_out_write(&o, offsets ? offsets : &zero64, 8, (size_t)t.nSeq + 1) ||
         h10x_out_write(&o, names.off ? names.off : &zero64, 8, (size_t)t.nSeq + 1) || h10x_out_write(&o, names.bytes, 1, (size_t)names.nBytes) ||
         h10x_out_rewrite(&o, head, h.n) || h10x_out_commit(&o) ? -1 : 0;
  }
  if (!rc && totals) *totals = t;
  goto done;
no_memory:
  rc = put_err(err, errlen, "out of host memory for the table of %llu sequences", t.nSeq);
done:
  h10x_out_abort(&o); free(table); free(offsets); free(pair); h10x_names_free(&names);
  return rc;
}

/* ---- .ss: --seqSpans. As .sb: the extents of each slab go to the file as they come; the per-sequence table, the offsets, the coverage (4 bytes per boundary)
   and the names are kept on the host and written at the end, with the header. The weak boundaries are found here, from cover[]. ---- */
int h10x_host_write_seq_spans(const char *path, const h10x_seq_spans_head *hd, h10x_seq_spans_slab_fn next, void *user, FILE *verbose,
                              h10x_seq_spans_totals *totals, char *err, int errlen) {
  typedef struct { uint64_t len; uint32_t moshes, found, inRange, weak; } Rec;
  h10x_seq_spans_totals t; memset(&t, 0, sizeof t);
  Rec *table = 0; uint64_t *offsets = 0, *coverOff = 0; uint32_t *quad = 0, *cover = 0; NameTable names; memset(&names, 0, sizeof names);
  size_t capTable = 0, capOff = 0, capCoverOff = 0, capQuad = 0, capCover = 0;
  OutFile o; unsigned char head[64]; memset(head, 0, sizeof head);
  if (h10x_out_open(&o, path, err, errlen)) return -1;
  int rc = h10x_out_write(&o, head, 1, sizeof head);
  while (!rc) {
    h10x_seq_spans_slab b; memset(&b, 0, sizeof b);
    const int got = next(user, &b);
    if (got < 0) { rc = -2; break; }                                  /* the callback's own error stands */
    if (!got) break;
    const uint64_t rows = b.nSeq ? b.rowOff[b.nSeq] : 0, bounds = b.nSeq ? b.coverOff[b.nSeq] : 0;
    if (h10x_grow((void **)&table, &capTable, (size_t)(t.nSeq + b.nSeq), sizeof(Rec)) || h10x_grow((void **)&offsets, &capOff, (size_t)(t.nSeq + b.nSeq + 1), 8) ||
        h10x_grow((void **)&coverOff, &capCoverOff, (size_t)(t.nSeq + b.nSeq + 1), 8) || h10x_grow((void **)&quad, &capQuad, (size_t)rows, 16) ||
        h10x_grow((void **)&cover, &capCover, (size_t)(t.boundaries + bounds), 4)) goto no_memory;
    offsets[0] = 0; coverOff[0] = 0;
    for (uint64_t i = 0; i < rows; ++i) {
      quad[4 * i] = b.block[i]; quad[4 * i + 1] = b.first[i]; quad[4 * i + 2] = b.last[i]; quad[4 * i + 3] = b.hits[i];
      const uint32_t span = b.last[i] - b.first[i];
      t.sumSpan += span;
      if (span > t.maxSpan) t.maxSpan = span;
      if (b.hits[i] > t.maxHits) t.maxHits = b.hits[i];
    }
    if ((rc = h10x_out_write(&o, quad, 16, (size_t)rows))) break;
    if (bounds) memcpy(cover + t.boundaries, b.cover, (size_t)bounds * 4);
    for (uint32_t q = 0; q < b.nSeq; ++q) {
      const uint64_t at = t.nSeq + q, len = b.seqStart[q + 1] - b.seqStart[q], c0 = b.coverOff[q], c1 = b.coverOff[q + 1];
      const h10x_seq_span_figures *g = b.fig + q;
      const char *name = b.names + b.nameOff[q];
      if (h10x_names_add(&names, name)) goto no_memory;
      uint32_t weak = 0;
      for (uint64_t j = c0; j < c1; ++j) weak += b.cover[j] < hd->minCover;
      Rec rec = {len, g->moshes, g->found, g->inRange, weak};
      table[at] = rec;
      offsets[at + 1] = t.extents + b.rowOff[q + 1]; coverOff[at + 1] = t.boundaries + c1;
      if (verbose) {
        fprintf(verbose, "SEQ_SPANS  %s len %llu moshes %u found %u inRange %u extents %llu boundaries %llu weak %u\n", name, (unsigned long long)len, g->moshes,
                g->found, g->inRange, (unsigned long long)(b.rowOff[q + 1] - b.rowOff[q]), (unsigned long long)(c1 - c0), weak);
        for (uint64_t j = c0; j < c1;) {                                /* the maximal runs of boundaries below minCover; boundary j - c0 + 1 stands at (j - c0 + 1) W */
          if (b.cover[j] >= hd->minCover) { ++j; continue; }
          uint64_t e = j; uint32_t low = b.cover[j];
          while (e + 1 < c1 && b.cover[e + 1] < hd->minCover) { ++e; if (b.cover[e] < low) low = b.cover[e]; }
          fprintf(verbose, "SEQ_WEAK  %s from %llu to %llu min %u\n", name, (unsigned long long)((j - c0 + 1) * hd->window),
                  (unsigned long long)((e - c0 + 1) * hd->window), low);
          j = e + 1;
        }
      }
      t.bases += len; t.moshes += g->moshes; t.found += g->found; t.inRange += g->inRange; t.weak += weak;
    }
    t.nSeq += b.nSeq; t.extents += rows; t.boundaries += bounds; t.hits += b.gathered;
  }
  if (!rc) {
    Head h = head_start(head, "10XE"); put_u32(&h, hd->nBlocks); put_u32(&h, hd->minShare); put_u32(&h, hd->maxGap); put_u32(&h, hd->window); put_u32(&h, hd->minCover);
    put_u32(&h, 0); put_u64(&h, t.nSeq); put_u64(&h, t.extents); put_u64(&h, t.boundaries); put_u64(&h, names.nBytes);
    rc = h10x_out_write(&o, table, sizeof(Rec), (size_t)t.nSeq) || h10x_out_write(&o, offsets ? offsets : &zero64, 8, (size_t)t.nSeq + 1) ||
         h10x_out_write(&o, coverOff ? coverOff : &zero64, 8, (size_t)t.nSeq + 1) || h10x_out_write(&o, cover, 4, (size_t)t.boundaries) ||
         h10x_out_write(&o, names.off ? names.off : &zero64, 8, (size_t)t.nSeq + 1) || h10x_out_write(&o, names.bytes, 1, (size_t)names.nBytes) ||
         h10x_out_rewrite(&o, head, h.n) || h10x_out_commit(&o) ? -1 : 0;
  }
  if (!rc && totals) *totals = t;
  goto done;
no_memory:
  rc = put_err(err, errlen, "out of host memory for the table of %llu sequences", t.nSeq);
done:
  h10x_out_abort(&o); free(table); free(offsets); free(coverOff); free(quad); free(cover); h10x_names_free(&names);
  return rc;
}

/* ---- .sp: --seqSpectrum. As .ss: the window records of each slab go to the file as they come; the per-sequence records, the window offsets and the names are
   kept on the host; the totals, the spectrum and the copies are asked for when the last slab is in, the copies in pieces of 2^22 hashes. ---- */
double h10x_host_qv(uint64_t moshes, uint64_t unsupported, int k) {
  if (!moshes) return 0.0;
  if (!unsupported) return INFINITY;
  return -10.0 * log10(1.0 - pow(1.0 - (double)unsupported / (double)moshes, 1.0 / (double)k)) + 0.0;   /* (+ 0.0: every mosh unsupported gives 0.00, not -0.00) */
}

int h10x_host_write_seq_spectrum(const char *path, const h10x_seq_spectrum_head *hd, h10x_seq_spectrum_slab_fn next, h10x_seq_spectrum_end_fn end,
                                 h10x_seq_spectrum_copies_fn copies, void *user, FILE *verbose, h10x_seq_spectrum_totals *totals, char *err, int errlen) {
  enum { PIECE = 1 << 22, BINS = H10X_SPECTRUM_DEPTH_BINS * H10X_SPECTRUM_COPY_BINS };
  h10x_seq_spectrum_totals t; memset(&t, 0, sizeof t);
  h10x_seq_spectrum_figures *table = 0; uint64_t *offsets = 0, *spectrum = 0; uint32_t *piece = 0; unsigned char *bytes = 0; NameTable names; memset(&names, 0, sizeof names);
  size_t capTable = 0, capOff = 0;
  OutFile o; unsigned char head[64]; memset(head, 0, sizeof head);
  if (h10x_out_open(&o, path, err, errlen)) return -1;
  int rc = h10x_out_write(&o, head, 1, sizeof head);
  while (!rc) {
    h10x_seq_spectrum_slab b; memset(&b, 0, sizeof b);
    const int got = next(user, &b);
    if (got < 0) { rc = -2; break; }                                  /* the callback's own error stands */
    if (!got) break;
    const uint64_t wins = b.nSeq ? b.winOff[b.nSeq] : 0;
    if (h10x_grow((void **)&table, &capTable, (size_t)(t.nSeq + b.nSeq), sizeof *table) || h10x_grow((void **)&offsets, &capOff, (size_t)(t.nSeq + b.nSeq + 1), 8)) goto no_memory;
    offsets[0] = 0;
    if ((rc = h10x_out_write(&o, b.win, sizeof *b.win, (size_t)wins))) break;
    for (uint32_t q = 0; q < b.nSeq; ++q) {
      const uint64_t at = t.nSeq + q;
      const h10x_seq_spectrum_figures *g = b.fig + q;
      const char *name = b.names + b.nameOff[q];
      if (h10x_names_add(&names, name)) goto no_memory;
      table[at] = *g;
      offsets[at + 1] = t.windows + b.winOff[q + 1];
      const uint32_t found = g->moshes - g->absent;
      if (verbose)
        fprintf(verbose, "SEQ_SPECTRUM  %s len %llu moshes %u absent %u copy0 %u copy1 %u copy2 %u copyM %u meanDepth %.1f QV %.2f\n", name, (unsigned long long)g->len,
                g->moshes, g->absent, g->n0, g->n1, g->n2, g->nM, found ? (double)g->depthSum / (double)found : 0.0,
                h10x_host_qv(g->moshes, (uint64_t)g->absent + g->n0, hd->k));
      t.bases += g->len; t.moshes += g->moshes; t.absent += g->absent; t.n0 += g->n0; t.n1 += g->n1; t.n2 += g->n2; t.nM += g->nM; t.depthSum += g->depthSum;
    }
    t.nSeq += b.nSeq; t.windows += wins;
  }
  if (!rc) {
    const size_t pieceLen = hd->hashNumber < PIECE ? (hd->hashNumber ? hd->hashNumber : 1) : PIECE;
    spectrum = (uint64_t *)calloc((size_t)BINS + 8, 8); piece = (uint32_t *)malloc(pieceLen * 4); bytes = (unsigned char *)malloc(pieceLen);
    if (!spectrum || !piece || !bytes) goto no_memory;
    if (end(user, spectrum + 8, spectrum) < 0) rc = -2;               /* (the totals stand before the spectrum in the file) */
  }
  if (!rc) {
    for (int q = 0; q < 4; ++q) { t.total[q] = spectrum[q]; t.present[q] = spectrum[4 + q]; }
    rc = h10x_out_write(&o, table, sizeof *table, (size_t)t.nSeq) || h10x_out_write(&o, offsets ? offsets : &zero64, 8, (size_t)t.nSeq + 1) ||
         h10x_out_write(&o, spectrum, 8, (size_t)BINS + 8) ? -1 : 0;
  }
  for (uint64_t at = 0; !rc && at < hd->hashNumber; at += PIECE) {
    const uint64_t m = hd->hashNumber - at < PIECE ? hd->hashNumber - at : PIECE;
    if (copies(user, at, m, piece) < 0) { rc = -2; break; }
    for (uint64_t i = 0; i < m; ++i) bytes[i] = (unsigned char)(piece[i] < 255 ? piece[i] : 255);
    if (!at) bytes[0] = 0;                                            /* (index 0 is no hash) */
    rc = h10x_out_write(&o, bytes, 1, (size_t)m);
  }
  if (!rc) {
    Head h = head_start(head, "10XP"); put_u32(&h, hd->hashNumber); put_u32(&h, hd->copy1min); put_u32(&h, hd->copy2min); put_u32(&h, hd->copyMmin); put_u32(&h, hd->window);
    put_u32(&h, H10X_SPECTRUM_DEPTH_BINS); put_u32(&h, H10X_SPECTRUM_COPY_BINS); put_u32(&h, 0); put_u64(&h, t.nSeq); put_u64(&h, t.windows); put_u64(&h, names.nBytes);
    rc = h10x_out_write(&o, names.off ? names.off : &zero64, 8, (size_t)t.nSeq + 1) || h10x_out_write(&o, names.bytes, 1, (size_t)names.nBytes) ||
         h10x_out_rewrite(&o, head, h.n) || h10x_out_commit(&o) ? -1 : 0;
  }
  if (!rc && totals) *totals = t;
  goto done;
no_memory:
  rc = put_err(err, errlen, "out of host memory for the table of %llu sequences", t.nSeq);
done:
  h10x_out_abort(&o); free(table); free(offsets); free(spectrum); free(piece); free(bytes); h10x_names_free(&names);
  return rc;
}

/* ---- .sl: --seqLinks. The tables come ready in the head; the links come back in pieces. ---- */
int h10x_host_write_seq_links(const char *path, const h10x_seq_links_head *h, h10x_seq_links_piece_fn piece, void *user, uint64_t pieceLinks, FILE *verbose,
                              h10x_seq_links_totals *totals, char *err, int errlen) {
  h10x_seq_links_totals t; memset(&t, 0, sizeof t);
  const uint64_t nEnds = 2 * h->nSeq, nameBytes = h->nSeq ? h->nameOff[h->nSeq] : 0;
  if (!pieceLinks) pieceLinks = (uint64_t)1 << 20;
  const uint64_t cap = h->links < pieceLinks ? h->links : pieceLinks;
  if (h->offsets[0] != 0 || h->offsets[nEnds] != h->links) return put_err(err, errlen, "seqLinks: the offsets do not end at the %llu links", h->links);
  OutFile o; if (h10x_out_open(&o, path, err, errlen)) return -1;
  uint32_t *other = (uint32_t *)malloc((size_t)(cap + 1) * 4), *shared = (uint32_t *)malloc((size_t)(cap + 1) * 4), *pair = (uint32_t *)malloc((size_t)(cap + 1) * 8);
  unsigned char *seen = (unsigned char *)calloc((size_t)h->nSeq + 1, 1);
  unsigned char head[64]; Head hd = head_start(head, "10XL");
  put_u32(&hd, h->nBlocks); put_u32(&hd, h->minShare); put_u32(&hd, h->minBlocks); put_u32(&hd, h->endLen); put_u32(&hd, h->maxEnds); put_u32(&hd, 0);
  put_u64(&hd, h->nSeq); put_u64(&hd, h->links); put_u64(&hd, h->skippedBlocks); put_u64(&hd, nameBytes);
  int rc = 0;
  if (!other || !shared || !pair || !seen) rc = put_err(err, errlen, "out of host memory for the links of %llu sequences", h->nSeq);
  else if (h10x_out_write(&o, head, 1, hd.n) || h10x_out_write(&o, h->table, sizeof(h10x_seq_links_rec), (size_t)h->nSeq) || h10x_out_write(&o, h->offsets, 8, (size_t)nEnds + 1)) rc = -1;
  uint64_t e = 0;                                                      /* the end whose row holds the link at hand */
  for (uint64_t first = 0; !rc && first < h->links; first += cap) {
    const uint64_t m = h->links - first < cap ? h->links - first : cap;
    if (piece(user, first, m, other, shared) < 0) { rc = -2; break; }   /* the callback's own error stands */
    for (uint64_t i = 0; i < m; ++i) {
      while (h->offsets[e + 1] <= first + i) ++e;
      const uint64_t g = other[i];
      if (g >= nEnds || g <= e) { if (err) snprintf(err, (size_t)errlen, "seqLinks: link %llu of end %llu names end %llu", (unsigned long long)(first + i), (unsigned long long)e, (unsigned long long)g); rc = -1; break; }
      seen[e >> 1] = 1; seen[g >> 1] = 1;
      if (shared[i] > t.maxShared) t.maxShared = shared[i];
      if (verbose) fprintf(verbose, "SEQ_LINKS  %s %c %s %c shared %u\n", h->names + h->nameOff[e >> 1], e & 1 ? 'T' : 'H', h->names + h->nameOff[g >> 1],
                           g & 1 ? 'T' : 'H', shared[i]);
    }
    if (rc) break;
    interleave_u32(pair, other, shared, m);
    rc = h10x_out_write(&o, pair, 8, (size_t)m);
    ++t.pieces;
  }
  if (!rc) rc = h10x_out_write(&o, h->nSeq ? h->nameOff : &zero64, 8, (size_t)h->nSeq + 1) || h10x_out_write(&o, h->names, 1, (size_t)nameBytes) || h10x_out_commit(&o) ? -1 : 0;
  for (uint64_t q = 0; q < h->nSeq && seen; ++q) t.withLinks += seen[q];
  t.nSeq = h->nSeq; t.links = h->links;
  if (!rc && totals) *totals = t;
  h10x_out_abort(&o); free(other); free(shared); free(pair); free(seen);
  return rc;
}

/* ---- the lines of --writeMosh (the .mosh file itself is mosh_host.c's, written through h10x_out_probe / _commit in h10x_host.c) ---- */
void h10x_host_print_state_mosh(FILE *out, const h10x_state_mosh_info *z, int withCrib) {
  fprintf(out, "  mosh set of %llu hashes in range, bits %u: copy0 %llu copy1 %llu copy2 %llu copyM %llu", (unsigned long long)z->kept, z->bits,
          (unsigned long long)z->copy[0], (unsigned long long)z->copy[1], (unsigned long long)z->copy[2], (unsigned long long)z->copy[3]);
  if (z->minShare) fprintf(out, ", by linkage at minShare %u: %llu to M, %llu to 0", z->minShare, (unsigned long long)z->toM, (unsigned long long)z->to0);
  else fprintf(out, ", by depth only");
  if (z->saturated) fprintf(out, ", %llu depths cut to 65535", (unsigned long long)z->saturated);
  fputc('\n', out);
  if (withCrib)
    for (int t = 0; t < 5; ++t)
      fprintf(out, "WRITE_MOSH  %s copy0 %llu copy1 %llu copy2 %llu copyM %llu\n", cribTypeName[t], (unsigned long long)z->crib[t][0],
              (unsigned long long)z->crib[t][1], (unsigned long long)z->crib[t][2], (unsigned long long)z->crib[t][3]);
}
