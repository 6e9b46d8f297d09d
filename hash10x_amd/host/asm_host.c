/* asm_host.c — host side of moshasm-amd: the RSMSHv2 file (readsetWrite / readsetRead, moshasm.c:84-123, over arrayWrite's layout,
 * array.c:213-218), the RS / RR / RH / RO / AR / AH texts (moshasm.c:167-230, 359-380, 386-416, 514-579) and the file-level commands
 * over the h10x_readset_* entry points of include/h10x.h. The file code touches no device.
 */
#define _GNU_SOURCE
#include "h10x_host.h"
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <pthread.h>
#include <sys/stat.h>

enum { ARRAY_MAGIC = 8918274, READ_SIZE = 72, MAX_HITS = 65534 };
#define TOPBIT 0x80000000u
#define TOPMASK 0x7fffffffu
typedef struct { int32_t magic, pad0; uint64_t base; int32_t dim, size, max, pad1; } ArrayHead;   /* struct ArrayStruct (array.h:41-50) */
_Static_assert(sizeof(h10x_read_t) == READ_SIZE, "the Read record of the file");
_Static_assert(sizeof(ArrayHead) == 32, "the ArrayStruct of the file");

static int set_msg(char *dst, int len, const char *fmt, ...) {
  va_list ap; va_start(ap, fmt); if (dst && len > 0) vsnprintf(dst, (size_t)len, fmt, ap); va_end(ap);
  return -1;
}

/* ------------------------------------------------------------------------------------------------ RSMSHv2 */
void h10x_readsetfile_free(h10x_readsetfile *r) {
  if (!r) return;
  free(r->reads); free(r->hit); free(r->dx);
  r->reads = 0; r->hit = 0; r->dx = 0;
}
/* readsetRead's file half with what a file from outside needs: the header, size == 72, max <= dim, hit counts that fit the file,
   every index within 1 .. setMax */
int h10x_readsetfile_read(const char *path, uint32_t setMax, h10x_readsetfile *r, char *err, int errlen) {
  memset(r, 0, sizeof *r);
  FILE *f = fopen(path, "rb");
  if (!f) return set_msg(err, errlen, "can't open file %s", path);
  int rc = -1; char name[8]; ArrayHead a; struct stat sb;
#define FAIL(...) do { set_msg(err, errlen, __VA_ARGS__); goto out; } while (0)
  if (fstat(fileno(f), &sb)) FAIL("can't stat file %s", path);
  const uint64_t fileSize = (uint64_t)sb.st_size;
  if (fread(name, 8, 1, f) != 1) FAIL("failed to read readset header");
  if (memcmp(name, "RSMSHv2", 8)) FAIL("bad readset header %.8s != RSMSHv2", name);
  if (fread(&r->totHit, 8, 1, f) != 1) FAIL("failed to read totHit");
  if (fread(&a, sizeof a, 1, f) != 1) FAIL("failed to read the reads array");
  if (a.size != READ_SIZE) FAIL("readset record size %d != %d", a.size, READ_SIZE);
  if (a.max < 1 || a.max > a.dim) FAIL("readset max %d outside 1 .. dim %d", a.max, a.dim);
  if (fileSize < 48 + (uint64_t)READ_SIZE * (uint64_t)a.dim) FAIL("failed to read the reads array");
  r->dim = (uint32_t)a.dim; r->max = (uint32_t)a.max;
  r->reads = (h10x_read_t *)malloc((size_t)a.max * READ_SIZE);
  if (!r->reads) FAIL("out of host memory for %d reads", a.max);
  if (fread(r->reads, READ_SIZE, (size_t)a.max, f) != (size_t)a.max) FAIL("failed to read the reads array");
  if (fseeko(f, (off_t)(48 + (uint64_t)READ_SIZE * (uint64_t)a.dim), SEEK_SET)) FAIL("failed to read the reads array");
  uint64_t tot = 0;
  for (uint32_t i = 0; i < r->max; ++i) {
    const int32_t n = r->reads[i].nHit;
    if (n < 0 || n > MAX_HITS) FAIL("read %u has %d hits: more than %d are not supported", i, n, MAX_HITS);
    tot += (uint64_t)n; r->reads[i].hitPtr = r->reads[i].dxPtr = 0;
  }
  if (tot != r->totHit) FAIL("readset totHit %llu but the reads hold %llu hits", (unsigned long long)r->totHit, (unsigned long long)tot);
  uint64_t have = fileSize - (48 + (uint64_t)READ_SIZE * (uint64_t)a.dim);
  const uint64_t cap = have / 4 < tot ? have / 4 : tot;       /* never more than the file can hold */
  r->hit = (uint32_t *)malloc((size_t)(cap ? cap : 1) * 4); r->dx = (uint16_t *)malloc((size_t)(cap ? cap : 1) * 2);
  if (!r->hit || !r->dx) FAIL("out of host memory for %llu hits", (unsigned long long)tot);
  uint64_t at = 0;
  for (uint32_t i = 0; i < r->max; ++i) {
    const uint64_t n = (uint64_t)r->reads[i].nHit;
    if (!n) continue;
    if (have < n * 4 || fread(r->hit + at, 4, n, f) != n) FAIL("failed read hits");
    have -= n * 4;
    if (have < n * 2 || fread(r->dx + at, 2, n, f) != n) FAIL("failed read dx");
    have -= n * 2;
    uint32_t top = 0, low = 0xFFFFFFFFu;
    for (uint64_t p = at; p < at + n; ++p) { const uint32_t y = r->hit[p] & TOPMASK; if (y > top) top = y; if (y < low) low = y; }
    if (top > setMax || low == 0) FAIL("read %u holds mosh index %u outside 1 .. %u", i, top > setMax ? top : 0, setMax);
    at += n;
  }
  rc = 0;
out:
#undef FAIL
  fclose(f);
  if (rc) h10x_readsetfile_free(r);
  return rc;
}

int h10x_readsetfile_write(const char *path, uint64_t totHit, uint32_t dim, const h10x_read_t *reads, uint32_t nReads, const uint64_t *hitStart,
                           const uint32_t *hit, const uint16_t *dx, char *err, int errlen) {
  if (nReads < 1 || nReads > dim) return set_msg(err, errlen, "readset max %u outside 1 .. dim %u", nReads, dim);
  FILE *f = fopen(path, "wb");
  if (!f) return set_msg(err, errlen, "can't open file %s", path);
  int rc = -1;
#define FAIL(...) do { set_msg(err, errlen, __VA_ARGS__); goto out; } while (0)
  ArrayHead a; memset(&a, 0, sizeof a);
  a.magic = ARRAY_MAGIC; a.dim = (int32_t)dim; a.size = READ_SIZE; a.max = (int32_t)nReads;
  if (fwrite("RSMSHv2", 8, 1, f) != 1) FAIL("failed to write readset header");
  if (fwrite(&totHit, 8, 1, f) != 1) FAIL("failed to write totHit");
  if (fwrite(&a, sizeof a, 1, f) != 1 || fwrite(reads, READ_SIZE, nReads, f) != nReads) FAIL("failed to write the reads array");
  {
    static const char zero[READ_SIZE * 64];
    for (uint64_t left = (uint64_t)dim - nReads; left; ) {
      const size_t n = left < 64 ? (size_t)left : 64;
      if (fwrite(zero, READ_SIZE, n, f) != n) FAIL("failed to write the reads array");
      left -= n;
    }
  }
  for (uint32_t i = 0; i < nReads; ++i) {
    const size_t n = (size_t)(hitStart[i + 1] - hitStart[i]);
    if (!n) continue;
    if (fwrite(hit + hitStart[i], 4, n, f) != n) FAIL("failed write hits %d", (int)n);
    if (fwrite(dx + hitStart[i], 2, n, f) != n) FAIL("failed write dx %d", (int)n);
  }
  rc = 0;
out:
#undef FAIL
  if (fclose(f) && !rc) rc = set_msg(err, errlen, "failed to write readset file %s", path);
  return rc;
}

/* ------------------------------------------------------------------------------------------------ commands over a device readset */
int h10x_readset_write_file(h10x_readset *rs, const char *path, char *err, int errlen) {
  h10x_readset_info_t in; const h10x_read_t *reads; const uint64_t *hs; const uint32_t *hit; const uint16_t *dx;
  if (h10x_readset_info(rs, &in) || h10x_readset_export(rs, &reads, &hs, &hit, &dx)) return set_msg(err, errlen, "%s", h10x_readset_error(rs));
  return h10x_readsetfile_write(path, in.totHit, in.dim, reads, in.nReads, hs, hit, dx, err, errlen);
}

typedef struct { h10x_seqreader *r; uint64_t slab; const uint8_t *codes; const uint64_t *start; uint32_t nSeq; int rc; } NextCall;
static void *next_thread(void *p) { NextCall *c = (NextCall *)p; c->rc = h10x_seq_next(c->r, c->slab, &c->codes, &c->start, &c->nSeq); return 0; }
/* the loop of readsetFileRead: 0 = done, 1 = the file could not be opened (msg = the line for stderr, may be empty), -1 = fatal (msg) */
int h10x_readset_add_file(h10x_readset *rs, const char *path, uint64_t slabBases, char *msg, int msglen, char *warn, int warnlen) {
  int fatal = 0;
  if (warn && warnlen > 0) warn[0] = 0;
  h10x_seqreader *r = h10x_seq_open(path, msg, msglen, &fatal);
  if (!r) return fatal ? -1 : 1;
  int rc = 0;
  NextCall cur = {r, slabBases, 0, 0, 0, 0}, nxt = cur;
  next_thread(&cur);
  while (cur.rc == 1) {
    pthread_t th; int threaded = pthread_create(&th, 0, next_thread, &nxt) == 0;
    const int arc = h10x_readset_add(rs, cur.codes, cur.start, cur.nSeq);
    if (threaded) pthread_join(th, 0); else next_thread(&nxt);
    if (arc) { rc = set_msg(msg, msglen, "%s", h10x_readset_error(rs)); break; }
    cur = nxt;
  }
  if (!rc && cur.rc < 0) rc = set_msg(msg, msglen, "%s", h10x_seq_error(r));
  if (warn && warnlen > 0) snprintf(warn, (size_t)warnlen, "%s", h10x_seq_warning(r));
  h10x_seq_close(r);
  return rc;
}

#define RS_FAIL(rs) return set_msg(err, errlen, "%s", h10x_readset_error(rs))

/* readsetStats (moshasm.c:167-230); 1 = empty readset (the caller prints the reference's line on stderr) */
int h10x_readset_print_stats(h10x_readset *rs, h10x_mosh *set, FILE *f, char *err, int errlen) {
  h10x_readset_info_t in; const h10x_read_t *reads; uint64_t sums[16];
  if (h10x_readset_info(rs, &in)) RS_FAIL(rs);
  const uint32_t n = in.nReads - 1;
  if (!n) return 1;
  if (h10x_readset_export(rs, &reads, 0, 0, 0) || h10x_readset_stats_sums(rs, sums)) RS_FAIL(rs);
  if (h10x_mosh_set_summary(set, f)) return set_msg(err, errlen, "%s", h10x_mosh_error(set));
  int nUnique0 = 0, nUnique1 = 0;
  uint64_t totLen = 0, totMiss = 0, lenUnique0 = 0, lenUnique1 = 0, totCopy[4] = {0, 0, 0, 0};
  uint32_t nBad = 0, nb[6] = {0, 0, 0, 0, 0, 0};
  for (uint32_t i = 1; i <= n; ++i) {
    const h10x_read_t *r = &reads[i];
    totLen += (uint64_t)r->len; totMiss += (uint64_t)r->nMiss;
    for (int j = 0; j < 4; ++j) totCopy[j] += (uint64_t)r->nCopy[j];
    if (r->nCopy[1] == 0) { ++nUnique0; lenUnique0 += (uint64_t)r->len; }
    else if (r->nCopy[1] == 1) { ++nUnique1; lenUnique1 += (uint64_t)r->len; }
    if (r->bad) { ++nBad; for (int b = 0; b < 6; ++b) nb[b] += (r->bad >> b) & 1; }
  }
  const uint64_t totHit = in.totHit;
  fprintf(f, "RS %d sequences, total length %llu (av %.1f)\n", (int)n, (unsigned long long)totLen, totLen / (double)n);
  fprintf(f, "RS %llu mosh hits, %.1f bp/hit, frac hit %.2f, av hits/read %.1f\n", (unsigned long long)totHit, totLen / (double)totHit,
          totHit / (double)(totMiss + totHit), totHit / (double)n);
  fprintf(f, "RS hit distribution %.2f copy0, %.2f copy1, %.2f copy2, %.2f copyM\n", totCopy[0] / (double)totHit, totCopy[1] / (double)totHit,
          totCopy[2] / (double)totHit, totCopy[3] / (double)totHit);
  const uint32_t nUniqueMulti = n - (uint32_t)nUnique0 - (uint32_t)nUnique1;
  fprintf(f, "RS num reads and av_len with 0 copy1 hits %d %.1f with 1 copy1 hits %d %.1f >1 copy1 hits %d %.1f av copy1 hits %.1f\n",
          nUnique0, lenUnique0 / (double)nUnique0, nUnique1, lenUnique1 / (double)nUnique1, (int)nUniqueMulti,
          (totLen - lenUnique0 - lenUnique1) / (double)nUniqueMulti, (totCopy[1] - (uint64_t)nUnique1) / (double)nUniqueMulti);
  fprintf(f, "RS bad %u : %u repeat, %u order10, %u order1, %u no_match, %u low_hit, %u low_copy1\n", nBad, nb[0], nb[1], nb[2], nb[3], nb[4], nb[5]);
  static const char *const cls[4] = {"copy0", "copy1", "copy2", "copyM"};
  fprintf(f, "RS mosh frac hit hit>1 av:");
  for (int j = 0; j < 4; ++j)
    fprintf(f, " %s %.3f %.3f %.1f", cls[j], (uint32_t)sums[4 + j] / (double)(uint32_t)sums[j], (uint32_t)sums[8 + j] / (double)(uint32_t)sums[j], sums[12 + j] / (double)(uint32_t)sums[8 + j]);
  fputc('\n', f);
  return 0;
}

/* findOverlaps with reportLevel 1 (RR) or 2 (RH + RR) (moshasm.c:359-380); *olap / *nOlap get the array when asked for (free it) */
int h10x_readset_print_overlaps(h10x_readset *rs, uint32_t ix, int level, FILE *f, h10x_overlap_t **olap, uint32_t *nOlap, char *err, int errlen) {
  uint32_t cap = 0, n = 0; int32_t cnt[3]; const h10x_read_t *reads;
  const int want = level > 1 || olap;
  h10x_overlap_t *o = 0;
  if (want) {
    if (h10x_readset_overlap_cap(rs, ix, &cap)) RS_FAIL(rs);
    o = (h10x_overlap_t *)malloc((size_t)cap * sizeof *o);
    if (!o) return set_msg(err, errlen, "out of host memory");
  }
  if (h10x_readset_overlaps(rs, ix, o, cap, &n, cnt) || h10x_readset_export(rs, &reads, 0, 0, 0)) { free(o); RS_FAIL(rs); }
  if (level > 1)
    for (uint32_t i = 0; i < n; ++i)
      if (o[i].visited)
        fprintf(f, "RH\t%u\tlen %d\t%s\tnPlus %d\tnMinus %d\toffset %.1f\tsd %.1f\n", o[i].iy, reads[o[i].iy].len, o[i].isBad ? "BAD" : "GOOD", o[i].nPlus, o[i].nMinus, o[i].d, o[i].sd);
  if (level > 0) {
    const h10x_read_t *x = &reads[ix];
    fprintf(f, "RR %6u\tlen %d\tnHit %3d\tnMiss %3d\tnCpy %d %d %d %d\tnRepeatMosh %d\tnGood %4d\tnBad %4d\n", ix, x->len, x->nHit, x->nMiss,
            x->nCopy[0], x->nCopy[1], x->nCopy[2], x->nCopy[3], cnt[0], cnt[1], cnt[2]);
  }
  if (olap) { *olap = o; *nOlap = n; } else free(o);
  return 0;
}

typedef struct { uint64_t *value; uint16_t *depth; uint8_t *info; uint32_t max; } SetCopy;
static int set_copy_get(h10x_mosh *set, SetCopy *s, char *err, int errlen) {
  h10x_mosh_info_t in; memset(s, 0, sizeof *s);
  if (h10x_mosh_info(set, &in)) return set_msg(err, errlen, "bad mosh set");
  s->max = in.max;
  s->value = (uint64_t *)malloc(((size_t)in.max + 1) * 8); s->depth = (uint16_t *)malloc(((size_t)in.max + 1) * 2); s->info = (uint8_t *)malloc((size_t)in.max + 1);
  if (!s->value || !s->depth || !s->info) { free(s->value); free(s->depth); free(s->info); return set_msg(err, errlen, "out of host memory"); }
  if (h10x_mosh_export(set, 0, 0, 0, s->value, s->depth, s->info)) { free(s->value); free(s->depth); free(s->info); return set_msg(err, errlen, "%s", h10x_mosh_error(set)); }
  return 0;
}
static void set_copy_free(SetCopy *s) { free(s->value); free(s->depth); free(s->info); }

/* printOverlap (moshasm.c:386-416) as written: hx is never advanced, so every turn of the outer loop looks at x's FIRST hit, and
   yPos adds y->dx[0] each time */
int h10x_readset_print_pair(h10x_readset *rs, h10x_mosh *set, uint32_t ix, uint32_t iy, FILE *f, char *err, int errlen) {
  h10x_readset_info_t in; const h10x_read_t *reads; const uint64_t *hs; const uint32_t *hit; const uint16_t *dx; SetCopy sc;
  if (h10x_readset_info(rs, &in) || h10x_readset_export(rs, &reads, &hs, &hit, &dx)) RS_FAIL(rs);
  if (ix >= in.nReads || iy >= in.nReads) return set_msg(err, errlen, "read %u is outside the readset of %u reads", ix >= in.nReads ? ix : iy, in.nReads - 1);
  if (set_copy_get(set, &sc, err, errlen)) return -1;
  const h10x_read_t *x = &reads[ix], *y = &reads[iy];
  fprintf(f, "RR overlaps_for %u\tlen %d\tnHit %d\tnMiss %d\tnCopy %d %d %d %d\n", ix, x->len, x->nHit, x->nMiss, x->nCopy[0], x->nCopy[1], x->nCopy[2], x->nCopy[3]);
  fprintf(f, "RR overlaps_for %u\tlen %d\tnHit %d\tnMiss %d\tnCopy %d %d %d %d\n", iy, y->len, y->nHit, y->nMiss, y->nCopy[0], y->nCopy[1], y->nCopy[2], y->nCopy[3]);
  int xPos = 0;
  for (int j = 0; j < x->nHit; ++j) {
    const uint32_t hx = hit[hs[ix]], hxx = hx & TOPMASK;
    xPos += dx[hs[ix] + (uint64_t)j];
    if ((sc.info[hxx] & 3) != 1) continue;
    int yPos = 0;
    for (int k = 0; k < y->nHit; ++k) {
      const uint32_t hy = hit[hs[iy] + (uint64_t)k];
      yPos += dx[hs[iy]];
      if (hxx == (hy & TOPMASK))
        fprintf(f, "RO\t%8x %5d %c\t%u %u %c\t%u %u %c\n", hxx, sc.depth[hxx], (hx & TOPBIT) == (hy & TOPBIT) ? '+' : '-', ix, xPos, (hx & TOPBIT) ? 'F' : 'R',
                iy, yPos, (hy & TOPBIT) ? 'F' : 'R');
    }
  }
  set_copy_free(&sc);
  return 0;
}

/* assembleFromRead's report (moshasm.c:514-579): RR to f, AR / AH to fstd. hashAdd numbers the distinct hits from 1 in the order met,
   and the reporting loop runs over 1 .. hashCount - 1 */
int h10x_readset_print_assembly(h10x_readset *rs, h10x_mosh *set, uint32_t ix, FILE *f, FILE *fstd, char *err, int errlen) {
  h10x_overlap_t *o = 0; uint32_t nO = 0; const h10x_read_t *reads; const uint64_t *hs; const uint32_t *hit; const uint16_t *dx; SetCopy sc;
  if (h10x_readset_print_overlaps(rs, ix, 1, f, &o, &nO, err, errlen)) return -1;
  if (h10x_readset_export(rs, &reads, &hs, &hit, &dx)) { free(o); RS_FAIL(rs); }
  if (set_copy_get(set, &sc, err, errlen)) { free(o); return -1; }
  typedef struct { uint32_t hit, count; int pos; } AHit;
  uint32_t *slot = (uint32_t *)calloc((size_t)sc.max + 1, 4); AHit *ah = 0; uint32_t nA = 0, capA = 0; int rc = -1;
  if (!slot) { set_msg(err, errlen, "out of host memory"); goto out; }
  for (uint32_t io = 0; io < nO; ++io) {
    const h10x_read_t *y = &reads[o[io].iy];
    int yPos = 0;
    for (int i = 0; i < y->nHit; ++i) {
      const uint32_t h = hit[hs[o[io].iy] + (uint64_t)i] & TOPMASK;
      yPos += dx[hs[o[io].iy] + (uint64_t)i];
      if (!slot[h]) {
        if (nA == capA) { capA = capA ? capA * 2 : 1024; AHit *p = (AHit *)realloc(ah, (size_t)capA * sizeof *p); if (!p) { set_msg(err, errlen, "out of host memory"); goto out; } ah = p; }
        ah[nA].hit = h; ah[nA].count = 0; ah[nA].pos = 0; slot[h] = ++nA;
      }
      AHit *a = &ah[slot[h] - 1];
      ++a->count;
      a->pos += o[io].isPlus ? o[io].offset + yPos : o[io].offset - yPos;
    }
  }
  {
    double totCount = 0.; int countA[20][20], countB[20][20]; int i, j;
    memset(countA, 0, sizeof countA); memset(countB, 0, sizeof countB);
    for (uint32_t ih = 1; ih < nA; ++ih) {
      const AHit *a = &ah[ih - 1];
      totCount += a->count;
      if ((sc.info[a->hit] & 3) != 1) continue;
      i = (int)a->count; if (i > 19) i = 19;
      j = sc.depth[a->hit]; if (j > 19) j = 19; ++countA[i][j];
      j = (int)((10 * a->count - 1) / sc.depth[a->hit]); if (j > 19) j = 19; ++countB[i][j];
    }
    totCount /= (int)nA;
    fprintf(fstd, "AR  %d total hits - mean count %.1f\n", (int)nA, totCount);
    for (i = 0; i < 20; ++i) {
      fprintf(fstd, "AH  %2d\t", i);
      for (j = 0; j < 20; ++j) if (j < i) fprintf(fstd, "    "); else fprintf(fstd, "%4d", countA[i][j]);
      fprintf(fstd, "    ");
      for (j = 0; j < 10; ++j) fprintf(fstd, "%4d", countB[i][j]);
      fputc('\n', fstd);
    }
  }
  rc = 0;
out:
  free(slot); free(ah); free(o); set_copy_free(&sc);
  return rc;
}
