/* mosh_host.c — host side of moshutils-amd: the sequence-file reader (seqio.c:15-190 of the reference for FASTA / FASTQ,
 * gzip or plain), the MSHSTv1 file (moshset.c:78-103, seqhash.c:39-51), the summary text (moshset.c:122-144) and the
 * file-level commands over the h10x_mosh_* entry points of include/h10x.h. The reader and the file code touch no device.
 */
#define _GNU_SOURCE
#include "h10x_host.h"
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <pthread.h>
#include <zlib.h>

/* ------------------------------------------------------------------------------------------------ sequence reader */
enum { SEQ_FASTA = 1, SEQ_FASTQ = 2 };
enum { RD_BUF = 1 << 20 };
typedef struct { uint8_t *codes; uint64_t nCodes, capCodes; uint64_t *start; uint32_t nSeq, capSeq; char *names; uint64_t nNames, capNames, *nameOff; } SeqSlab;
struct h10x_seqreader {
  gzFile f; int type; int line; int done;
  unsigned char *buf; int pos, n; int eof;                  /* buf[pos] is the current byte while !eof */
  SeqSlab slab[2]; int which;                               /* the slab of call N stays valid until call N + 2 returns */
  uint64_t nSeqTotal, basesTotal;
  char warn[256], err[256];
};

static int set_msg(char *dst, int len, const char *fmt, ...) {
  va_list ap; va_start(ap, fmt); if (dst && len > 0) vsnprintf(dst, (size_t)len, fmt, ap); va_end(ap);
  return -1;
}
/* dna2indexConv with moshutils' N -> 0 (seqio.c:274-283, moshutils.c:38): A C G T N in either case, everything else < 0 */
static int base_code(unsigned c) {
  switch (c) {
    case 'A': case 'a': case 'N': case 'n': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return -2;
  }
}
static void rd_fill(h10x_seqreader *r) {
  int n = gzread(r->f, r->buf, RD_BUF);
  r->pos = 0; r->n = n > 0 ? n : 0;
  if (r->n == 0) r->eof = 1;
}
static inline int rd_cur(const h10x_seqreader *r) { return r->buf[r->pos]; }
static inline void rd_adv(h10x_seqreader *r) { if (++r->pos >= r->n) rd_fill(r); }   /* afterwards r->eof says whether a byte is there */

h10x_seqreader *h10x_seq_open(const char *path, char *msg, int msglen, int *fatal) {
  if (fatal) *fatal = 0;
  if (msg && msglen > 0) msg[0] = 0;
  gzFile f = gzopen(path, "r");
  if (!f) return 0;                                          /* seqio.c:20: the caller says "failed to open sequence file" */
  h10x_seqreader *r = (h10x_seqreader *)calloc(1, sizeof *r);
  if (!r) { gzclose(f); set_msg(msg, msglen, "out of host memory"); if (fatal) *fatal = 1; return 0; }
  r->f = f; r->buf = (unsigned char *)malloc(RD_BUF); r->line = 1;
  if (!r->buf) { h10x_seq_close(r); set_msg(msg, msglen, "out of host memory"); if (fatal) *fatal = 1; return 0; }
  gzbuffer(f, 1 << 18);
  rd_fill(r);
  if (r->eof) { h10x_seq_close(r); set_msg(msg, msglen, "sequence file %s unreadable or empty", path); return 0; }              /* seqio.c:26-30 */
  if (rd_cur(r) == '>') r->type = SEQ_FASTA;
  else if (rd_cur(r) == '@') r->type = SEQ_FASTQ;
  else if (rd_cur(r) == 'B') { h10x_seq_close(r); set_msg(msg, msglen, "sequence file %s is in seqio's binary format, which is not supported", path); if (fatal) *fatal = 1; return 0; }
  else { h10x_seq_close(r); set_msg(msg, msglen, "sequence file %s is unknown type", path); return 0; }                         /* seqio.c:45-49 */
  return r;
}
void h10x_seq_close(h10x_seqreader *r) {
  if (!r) return;
  if (r->f) gzclose(r->f);
  free(r->buf);
  for (int i = 0; i < 2; ++i) { free(r->slab[i].codes); free(r->slab[i].start); free(r->slab[i].names); free(r->slab[i].nameOff); }
  free(r);
}
const char *h10x_seq_error(const h10x_seqreader *r) { return r ? r->err : "null reader"; }
const char *h10x_seq_warning(const h10x_seqreader *r) { return r ? r->warn : ""; }
void h10x_seq_totals(const h10x_seqreader *r, uint64_t *nSeq, uint64_t *bases) { if (nSeq) *nSeq = r->nSeqTotal; if (bases) *bases = r->basesTotal; }

static int slab_push(h10x_seqreader *r, SeqSlab *s, int code) {
  if (s->nCodes == s->capCodes) {
    uint64_t cap = s->capCodes ? s->capCodes * 2 : (1u << 20);
    uint8_t *p = (uint8_t *)realloc(s->codes, cap);
    if (!p) return set_msg(r->err, sizeof r->err, "out of host memory for %llu bases", (unsigned long long)cap);
    s->codes = p; s->capCodes = cap;
  }
  s->codes[s->nCodes++] = (uint8_t)code;
  return 0;
}
/* the record's name: the header up to the first blank or tab, as readSequence cuts it (readseq.c:82-88) */
static int name_push(h10x_seqreader *r, SeqSlab *s, int ch) {
  if (s->nNames == s->capNames) {
    uint64_t cap = s->capNames ? s->capNames * 2 : (1u << 12);
    char *p = (char *)realloc(s->names, cap);
    if (!p) return set_msg(r->err, sizeof r->err, "out of host memory for %llu bytes of names", (unsigned long long)cap);
    s->names = p; s->capNames = cap;
  }
  s->names[s->nNames++] = (char)ch;
  return 0;
}
static int slab_close_seq(h10x_seqreader *r, SeqSlab *s, uint64_t nameAt) {   /* start[nSeq] = end of the sequence just read */
  if (s->nSeq + 2 > s->capSeq) {
    uint32_t cap = s->capSeq ? s->capSeq * 2 : 1024;
    uint64_t *p = (uint64_t *)realloc(s->start, (size_t)cap * sizeof *p);
    if (!p) return set_msg(r->err, sizeof r->err, "out of host memory for %u sequences", cap);
    s->start = p;
    p = (uint64_t *)realloc(s->nameOff, (size_t)cap * sizeof *p);
    if (!p) return set_msg(r->err, sizeof r->err, "out of host memory for %u sequences", cap);
    s->nameOff = p; s->capSeq = cap;
  }
  s->nameOff[s->nSeq] = nameAt;
  if (s->nSeq == 0) s->start[0] = 0;
  const uint64_t len = s->nCodes - s->start[s->nSeq];
  if (len >= (1ull << 31)) return set_msg(r->err, sizeof r->err, "sequence %llu has %llu bases: 2^31 or more are not supported", (unsigned long long)(r->nSeqTotal + 1), (unsigned long long)len);
  s->start[++s->nSeq] = s->nCodes;
  ++r->nSeqTotal; r->basesTotal += len;
  return 0;
}

/* seqio.c:91-95: a record that the file ends inside is dropped with this line, and reading stops */
#define ADV_IN(r) do { rd_adv(r); if ((r)->eof) { snprintf((r)->warn, sizeof (r)->warn, "incomplete sequence record line %d", (r)->line); return 0; } } while (0)

/* one record (seqio.c:142-188): 1 = read, 0 = none (end of file, or the file ended inside it), -1 = fatal (r->err) */
static int read_record(h10x_seqreader *r, SeqSlab *s) {
  if (r->eof) return 0;
  if (r->type == SEQ_FASTA) {
    if (rd_cur(r) != '>') return set_msg(r->err, sizeof r->err, "no initial > for FASTA record line %d", r->line);
    ADV_IN(r);
    for (int inName = 1; rd_cur(r) != '\n'; ) {              /* identifier and description */
      if (rd_cur(r) == ' ' || rd_cur(r) == '\t') inName = 0;
      if (inName && name_push(r, s, rd_cur(r))) return -1;
      ADV_IN(r);
    }
    if (name_push(r, s, 0)) return -1;
    ++r->line; ADV_IN(r);
    while (!r->eof && rd_cur(r) != '>') {                    /* a record runs to the next LINE that starts with '>' */
      while (rd_cur(r) != '\n') {
        const unsigned c = (unsigned)rd_cur(r);
        if (c >= 0x80) return set_msg(r->err, sizeof r->err, "bad base 0x%02x in FASTA line %d", c, r->line);
        const int b = base_code(c);
        if (b >= 0 && slab_push(r, s, b)) return -1;         /* every other byte is dropped (seqio.c:165) */
        ADV_IN(r);
      }
      ++r->line; rd_adv(r);
    }
  } else {
    if (rd_cur(r) != '@') return set_msg(r->err, sizeof r->err, "no initial @ for FASTQ record line %d", r->line);
    ADV_IN(r);
    for (int inName = 1; rd_cur(r) != '\n'; ) {
      if (rd_cur(r) == ' ' || rd_cur(r) == '\t') inName = 0;
      if (inName && name_push(r, s, rd_cur(r))) return -1;
      ADV_IN(r);
    }
    if (name_push(r, s, 0)) return -1;
    ++r->line; ADV_IN(r);
    uint64_t len = 0, qlen = 0;
    while (rd_cur(r) != '\n') {                              /* the sequence line is taken whole */
      const unsigned c = (unsigned)rd_cur(r);
      const int b = c >= 0x80 ? -2 : base_code(c);
      if (b < 0) return set_msg(r->err, sizeof r->err, "bad base 0x%02x in FASTQ line %d", c, r->line);
      if (slab_push(r, s, b)) return -1;
      ++len; ADV_IN(r);
    }
    ++r->line; ADV_IN(r);
    if (rd_cur(r) != '+') return set_msg(r->err, sizeof r->err, "missing + FASTQ line %d", r->line);
    while (rd_cur(r) != '\n') ADV_IN(r);
    ++r->line; ADV_IN(r);
    while (rd_cur(r) != '\n') { ++qlen; ADV_IN(r); }
    if (qlen != len) return set_msg(r->err, sizeof r->err, "qual not same length as seq line %d", r->line);
    ++r->line; rd_adv(r);
  }
  return 1;
}

int h10x_seq_next(h10x_seqreader *r, uint64_t slabBases, const uint8_t **codes, const uint64_t **seqStart, uint32_t *nSeq) {
  return h10x_seq_next_named(r, slabBases, codes, seqStart, nSeq, 0, 0);
}
int h10x_seq_next_named(h10x_seqreader *r, uint64_t slabBases, const uint8_t **codes, const uint64_t **seqStart, uint32_t *nSeq, const char **names, const uint64_t **nameOff) {
  if (!r) return -1;
  SeqSlab *s = &r->slab[r->which]; r->which ^= 1;
  s->nCodes = 0; s->nSeq = 0; s->nNames = 0;
  if (!slabBases) slabBases = 1ull << 26;
  while (!r->done && (s->nSeq == 0 || s->nCodes < slabBases) && s->nSeq < 0x7FFFFFFFu) {
    const uint64_t mark = s->nCodes, nameMark = s->nNames;
    const int rc = read_record(r, s);
    if (rc < 0) { r->done = 1; return -1; }
    if (rc == 0) { s->nCodes = mark; s->nNames = nameMark; r->done = 1; break; }   /* (a record the file ended in leaves nothing behind) */
    if (slab_close_seq(r, s, nameMark)) { r->done = 1; return -1; }
  }
  if (codes) *codes = s->codes;
  if (seqStart) *seqStart = s->start;
  if (nSeq) *nSeq = s->nSeq;
  if (names) *names = s->names;
  if (nameOff) *nameOff = s->nameOff;
  return s->nSeq ? 1 : 0;
}

/* ------------------------------------------------------------------------------------------------ MSHSTv1 */
void h10x_moshfile_free(h10x_moshfile *m) {
  if (!m) return;
  free(m->index); free(m->value); free(m->depth); free(m->info);
  m->index = 0; m->value = 0; m->depth = 0; m->info = 0;
}
/* moshsetRead + seqhashRead (moshset.c:89-103, seqhash.c:44-51) with the reference's texts, plus what a file from outside
   needs and the reference does not check: the seqhash fields, the file's length, the table entries */
int h10x_moshfile_read(const char *path, h10x_moshfile *m, char *err, int errlen) {
  memset(m, 0, sizeof *m);
  FILE *f = fopen(path, "rb");
  if (!f) return set_msg(err, errlen, "failed to open mosh file %s", path);
  char name[8]; int rc = -1;
#define FAIL(...) do { set_msg(err, errlen, __VA_ARGS__); goto out; } while (0)
  if (fread(name, 8, 1, f) != 1) FAIL("failed to read moshset header");
  if (memcmp(name, "MSHSTv1", 8)) FAIL("bad reference header");
  if (fread(&m->B, 4, 1, f) != 1) FAIL("failed to read bits");
  if (fread(&m->size, 4, 1, f) != 1) FAIL("failed to read size");
  if (fread(name, 8, 1, f) != 1) FAIL("failed to read seqhash header");
  if (memcmp(name, "SQHSHv1", 8)) FAIL("seqhash read mismatch");
  if (fread(&m->sh, sizeof m->sh, 1, f) != 1) FAIL("failed to read seqhash");
  if (m->B < 20 || m->B > 34) FAIL("table bits %d must be between 20 and 34", m->B);
  const uint64_t T = 1ull << m->B;
  if (m->size >= (T >> 2)) FAIL("Moshset size %u is too big for %d bits", m->size, m->B);
  if (m->size < 1) FAIL("mosh file %s: size 0 (a set holds at least the unused entry 0)", path);
  if (m->sh.k < 1 || m->sh.k >= 32 || m->sh.w < 1) FAIL("mosh file %s: seqhash k %d w %d out of range", path, m->sh.k, m->sh.w);
  {
    const long long at = ftello(f);
    if (fseeko(f, 0, SEEK_END)) FAIL("mosh file %s: cannot seek", path);
    const long long end = ftello(f), want = at + (long long)(T * 4 + (uint64_t)m->size * 11);
    if (end < want) {                                        /* the reference's texts, by the array the file ends in */
      const long long have = end - at;
      if (have < (long long)(T * 4)) FAIL("failed read index");
      if (have < (long long)(T * 4 + (uint64_t)m->size * 8)) FAIL("failed to read value");
      if (have < (long long)(T * 4 + (uint64_t)m->size * 10)) FAIL("failed to read depth");
      FAIL("failed to read info");
    }
    if (end > want) FAIL("mosh file %s holds %lld bytes more than its header implies", path, end - want);
    fseeko(f, at, SEEK_SET);
  }
  m->index = (uint32_t *)malloc(T * 4); m->value = (uint64_t *)malloc((size_t)m->size * 8);
  m->depth = (uint16_t *)malloc((size_t)m->size * 2); m->info = (uint8_t *)malloc(m->size);
  if (!m->index || !m->value || !m->depth || !m->info) FAIL("out of host memory for mosh file %s", path);
  if (fread(m->index, 4, T, f) != T) FAIL("failed read index");
  if (fread(m->value, 8, m->size, f) != m->size) FAIL("failed to read value");
  if (fread(m->depth, 2, m->size, f) != m->size) FAIL("failed to read depth");
  if (fread(m->info, 1, m->size, f) != m->size) FAIL("failed to read info");
  {
    uint64_t used = 0;
    for (uint64_t i = 0; i < T; ++i) {
      if (m->index[i] >= m->size) FAIL("mosh file %s: table entry %u at slot %llu is beyond max %u", path, m->index[i], (unsigned long long)i, m->size - 1);
      used += m->index[i] != 0;
    }
    if (used != m->size - 1) FAIL("mosh file %s: %llu table entries for %u hashes", path, (unsigned long long)used, m->size - 1);
    /* every entry is found through its own probe walk: the values are distinct and the table is the one moshsetIndexFind reads
       (a repeated value would be met at its first index; the merge relies on distinct values giving distinct targets) */
    const uint64_t mask = T - 1;
    for (uint32_t i = 1; i < m->size; ++i) {
      const uint64_t h = m->value[i], step = ((h >> m->B) & mask) | 1;
      uint64_t slot = h & mask; uint32_t ix;
      while ((ix = m->index[slot]) && m->value[ix] != h) slot = (slot + step) & mask;
      if (ix != i) FAIL("mosh file %s: entry %u (hash %llx) is not where its probe walk ends (found %u): repeated value or foreign table", path, i, (unsigned long long)h, ix);
    }
  }
  rc = 0;
out:
#undef FAIL
  fclose(f);
  if (rc) h10x_moshfile_free(m);
  return rc;
}

/* moshsetSummary (moshset.c:122-144) from the counts: hist[65536] by depth, copy[4] */
void h10x_mosh_summary_print(FILE *f, int k, int w, int B, uint32_t max, const uint32_t *hist, const uint32_t *copy) {
  fprintf(f, "SH k %d  w %d\n", k, w);                       /* seqhashReport (seqhash.c:53-54) */
  fprintf(f, "MS table size %llu number of entries %u", 1ull << B, max);
  if (!max) return;                                          /* no newline: moshset.c:126 */
  uint32_t top = 0, i;
  for (i = 0; i < 65536; ++i) if (hist[i]) top = i + 1;       /* arrayMax(h) */
  uint64_t sum = 0, tot = 0;
  for (i = 0; i < top; ++i) { sum += hist[i]; tot += (uint64_t)(uint32_t)(i * hist[i]); }   /* i * arr(h,i,U32) is a 32-bit product */
  int64_t htot = (int64_t)(tot / 2);
  for (i = 0; i < top; ++i) { htot -= (uint32_t)(i * hist[i]); if (htot < 0) break; }
  fprintf(f, " total count %llu\nMS average depth %.1f N50 depth %u", (unsigned long long)tot, tot / (double)sum, i);
  if (copy[0] < max) fprintf(f, " copy0 %u copy1 %u copy2 %u copyM %u", copy[0], copy[1], copy[2], copy[3]);
  fputc('\n', f);
}
void h10x_moshfile_counts(const h10x_moshfile *m, uint32_t *hist65536, uint32_t copy4[4]) {
  memset(hist65536, 0, 65536 * 4); memset(copy4, 0, 16);
  for (uint32_t i = 1; i < m->size; ++i) { ++hist65536[m->depth[i]]; ++copy4[m->info[i] & 3]; }
}

/* ------------------------------------------------------------------------------------------------ commands over a device set */
int h10x_mosh_set_summary(h10x_mosh *set, FILE *f) {
  h10x_mosh_info_t in; uint32_t *hist = (uint32_t *)malloc(65536 * 4), copy[4];
  if (!hist) return -1;
  int rc = h10x_mosh_info(set, &in);
  if (!rc) rc = h10x_mosh_summary(set, hist, copy);
  if (!rc) h10x_mosh_summary_print(f, in.k, in.w, in.B, in.max, hist, copy);
  free(hist);
  return rc;
}

/* moshsetWrite (moshset.c:78-87): the table leaves the device in slices */
int h10x_mosh_set_write(h10x_mosh *set, const char *path, char *err, int errlen) {
  h10x_mosh_info_t in;
  if (h10x_mosh_info(set, &in)) return set_msg(err, errlen, "bad mosh set");
  FILE *f = fopen(path, "wb");
  if (!f) return set_msg(err, errlen, "failed to open mosh file %s", path);
  int rc = -1;
  const uint64_t T = 1ull << in.B, SL = 1ull << 24; const uint32_t n1 = in.max + 1;
  uint32_t *ix = (uint32_t *)malloc((T < SL ? T : SL) * 4);
  uint64_t *v = (uint64_t *)malloc((size_t)n1 * 8); uint16_t *d = (uint16_t *)malloc((size_t)n1 * 2); uint8_t *fl = (uint8_t *)malloc(n1);
#define FAIL(...) do { set_msg(err, errlen, __VA_ARGS__); goto out; } while (0)
  if (!ix || !v || !d || !fl) FAIL("out of host memory writing %s", path);
  h10x_seqhash_rec sh; memset(&sh, 0, sizeof sh);
  sh.k = in.k; sh.w = in.w; sh.mask = (1ull << (2 * in.k)) - 1; sh.shift1 = 64 - 2 * in.k; sh.shift2 = 2 * in.k;      /* seqhash.c:24-33 */
  sh.factor1 = in.factor1; sh.factor2 = in.factor2;
  for (int i = 0; i < 4; ++i) sh.patternRC[i] = (uint64_t)(3 - i) << (2 * (in.k - 1));
  if (fwrite("MSHSTv1", 8, 1, f) != 1) FAIL("failed to write moshset header");
  if (fwrite(&in.B, 4, 1, f) != 1) FAIL("failed to write bits");
  if (fwrite(&n1, 4, 1, f) != 1) FAIL("failed to write size");
  if (fwrite("SQHSHv1", 8, 1, f) != 1) FAIL("failed to write seqhash header");
  if (fwrite(&sh, sizeof sh, 1, f) != 1) FAIL("failed to write seqhash");
  for (uint64_t at = 0; at < T; at += SL) {
    const uint64_t n = T - at < SL ? T - at : SL;
    if (h10x_mosh_export(set, at, n, ix, 0, 0, 0)) FAIL("%s", h10x_mosh_error(set));
    if (fwrite(ix, 4, n, f) != n) FAIL("fail write index");
  }
  if (h10x_mosh_export(set, 0, 0, 0, v, d, fl)) FAIL("%s", h10x_mosh_error(set));
  if (fwrite(v, 8, n1, f) != n1) FAIL("failed to write value");
  if (fwrite(d, 2, n1, f) != n1) FAIL("failed to write depth");
  if (fwrite(fl, 1, n1, f) != n1) FAIL("failed to write info");
  rc = 0;
out:
#undef FAIL
  free(ix); free(v); free(d); free(fl);
  if (fclose(f) && !rc) rc = set_msg(err, errlen, "failed to write mosh file %s", path);
  return rc;
}

/* addSequenceFile (moshutils.c:32-50): the reader fills the next slab on a thread of its own while the device works on this one.
   0 = done (counts filled), 1 = the file could not be opened (msg = the line for stderr, may be empty), -1 = fatal (msg) */
typedef struct { h10x_seqreader *r; uint64_t slab; const uint8_t *codes; const uint64_t *start; uint32_t nSeq; int rc; } NextCall;
static void *next_thread(void *p) { NextCall *c = (NextCall *)p; c->rc = h10x_seq_next(c->r, c->slab, &c->codes, &c->start, &c->nSeq); return 0; }
int h10x_mosh_set_add_file(h10x_mosh *set, const char *path, int is10x, uint64_t slabBases, uint64_t *nSeq, uint64_t *totLen, uint64_t *totHash,
                           char *msg, int msglen, char *warn, int warnlen) {
  int fatal = 0;
  if (warn && warnlen > 0) warn[0] = 0;
  h10x_seqreader *r = h10x_seq_open(path, msg, msglen, &fatal);
  if (!r) return fatal ? -1 : 1;
  uint64_t base = 0, hashes = 0; int rc = 0;
  NextCall cur = {r, slabBases, 0, 0, 0, 0}, nxt = cur;
  next_thread(&cur);
  while (cur.rc == 1) {
    pthread_t th; int threaded = pthread_create(&th, 0, next_thread, &nxt) == 0;
    uint64_t h = 0;
    const int arc = h10x_mosh_add(set, cur.codes, cur.start, cur.nSeq, is10x, base, &h);
    if (threaded) pthread_join(th, 0); else next_thread(&nxt);
    if (arc) { rc = set_msg(msg, msglen, "%s", h10x_mosh_error(set)); break; }
    hashes += h; base += cur.nSeq;
    cur = nxt;
  }
  if (!rc && cur.rc < 0) rc = set_msg(msg, msglen, "%s", h10x_seq_error(r));
  if (warn && warnlen > 0) snprintf(warn, (size_t)warnlen, "%s", h10x_seq_warning(r));
  h10x_seq_totals(r, nSeq, totLen);
  if (totHash) *totHash = hashes;
  h10x_seq_close(r);
  return rc;
}
