/* The .ss writer of files_host.c (h10x_host_write_seq_spans) behind a main of its own, for the AddressSanitizer + UBSan build
   (tests/test_seq_spans_cpu.py): it needs no device.   ss_asan_driver <out.ss> <nSeq> <seqsPerSlab>
   Sequence q is called "s<q>", has 10 q + 1 bases, q % 4 extents {block q + i + 1, first i, last i + q, hits 2 q + i + 1} and, at window 4, (len - 1) / 4
   boundaries with cover (q + j) % 3; its figures are moshes q % 11, found q % 7, inRange q % 3. minCover is 2. The slabs hold seqsPerSlab sequences each
   (0: all in one). Then the callback fails in its last slab over a file that stood there before, and a path that cannot be opened is tried: neither may
   leave a .part behind, and the old file keeps its bytes. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include "h10x_host.h"

enum { WINDOW = 4, MIN_COVER = 2 };

typedef struct {
  uint64_t next, n, per, calls, failAt;
  uint64_t *seqStart, *rowOff, *coverOff, *nameOff; h10x_seq_span_figures *fig; uint32_t *col[4], *cover; char *names;
} Feed;

static void feed_free(Feed *f) {
  free(f->seqStart); free(f->rowOff); free(f->coverOff); free(f->nameOff); free(f->fig); free(f->cover); free(f->names);
  for (int k = 0; k < 4; ++k) free(f->col[k]);
}

static int feed(void *user, h10x_seq_spans_slab *b) {
  Feed *f = (Feed *)user;
  if (f->calls == f->failAt) return -1;
  if (f->next >= f->n) return 0;
  const uint64_t per = f->per ? f->per : f->n, m = f->n - f->next < per ? f->n - f->next : per;
  uint64_t bounds = 0;
  for (uint64_t i = 0; i < m; ++i) bounds += 10 * (f->next + i) / WINDOW;
  feed_free(f);
  f->seqStart = (uint64_t *)calloc(m + 1, 8); f->rowOff = (uint64_t *)calloc(m + 1, 8); f->coverOff = (uint64_t *)calloc(m + 1, 8); f->nameOff = (uint64_t *)calloc(m + 1, 8);
  f->fig = (h10x_seq_span_figures *)calloc(m, sizeof *f->fig); f->cover = (uint32_t *)calloc(bounds + 1, 4); f->names = (char *)calloc(m, 24);
  for (int k = 0; k < 4; ++k) f->col[k] = (uint32_t *)calloc(3 * m + 1, 4);
  if (!f->seqStart || !f->rowOff || !f->coverOff || !f->nameOff || !f->fig || !f->cover || !f->names || !f->col[0] || !f->col[1] || !f->col[2] || !f->col[3]) return -1;
  uint64_t nameAt = 0;
  for (uint64_t i = 0; i < m; ++i) {
    const uint64_t q = f->next + i, len = 10 * q + 1;
    f->seqStart[i + 1] = f->seqStart[i] + len;
    f->fig[i].len = len; f->fig[i].moshes = (uint32_t)(q % 11); f->fig[i].found = (uint32_t)(q % 7); f->fig[i].inRange = (uint32_t)(q % 3); f->fig[i].extents = (uint32_t)(q % 4);
    uint64_t r = f->rowOff[i];
    for (uint64_t k = 0; k < q % 4; ++k, ++r) { f->col[0][r] = (uint32_t)(q + k + 1); f->col[1][r] = (uint32_t)k; f->col[2][r] = (uint32_t)(k + q); f->col[3][r] = (uint32_t)(2 * q + k + 1); }
    f->rowOff[i + 1] = r;
    uint64_t c = f->coverOff[i];
    for (uint64_t j = 0; j < (len - 1) / WINDOW; ++j, ++c) f->cover[c] = (uint32_t)((q + j) % 3);
    f->coverOff[i + 1] = c;
    f->nameOff[i] = nameAt;
    nameAt += (uint64_t)snprintf(f->names + nameAt, 24, "s%llu", (unsigned long long)q) + 1;
  }
  b->nSeq = (uint32_t)m; b->seqStart = f->seqStart; b->fig = f->fig; b->rowOff = f->rowOff; b->block = f->col[0]; b->first = f->col[1]; b->last = f->col[2];
  b->hits = f->col[3]; b->coverOff = f->coverOff; b->cover = f->cover; b->gathered = 5 * m; b->names = f->names; b->nameOff = f->nameOff;
  f->next += m; ++f->calls;
  return 1;
}

static int exists(const char *p) { struct stat st; return stat(p, &st) == 0; }

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: ss_asan_driver <out.ss> <nSeq> <seqsPerSlab>\n"); return 2; }
  const uint64_t n = strtoull(argv[2], 0, 10), per = strtoull(argv[3], 0, 10);
  char err[256] = "", part[1200]; snprintf(part, sizeof part, "%s.part", argv[1]);
  const h10x_seq_spans_head head = {1000000, 3, 7, WINDOW, MIN_COVER};
  h10x_seq_spans_totals t;
  Feed f; memset(&f, 0, sizeof f); f.n = n; f.per = per; f.failAt = UINT64_MAX;
  int rc = h10x_host_write_seq_spans(argv[1], &head, feed, &f, stdout, &t, err, (int)sizeof err);
  feed_free(&f);
  if (rc) { fprintf(stderr, "%s\n", err); return 4; }
  if (f.next != n || t.nSeq != n || exists(part) || !exists(argv[1])) { fprintf(stderr, "the slabs do not tile the %llu sequences\n", (unsigned long long)n); return 5; }
  printf("%llu slabs, %llu extents, %llu boundaries, %llu weak, %llu hits, sum span %llu, max span %u, max hits %u\n", (unsigned long long)f.calls,
         (unsigned long long)t.extents, (unsigned long long)t.boundaries, (unsigned long long)t.weak, (unsigned long long)t.hits, (unsigned long long)t.sumSpan, t.maxSpan,
         t.maxHits);
  if (n) {                                                    /* a failing callback over the file just written: -2, err untouched, no .part, the old bytes kept */
    struct stat before, after;
    if (stat(argv[1], &before)) return 6;
    Feed g; memset(&g, 0, sizeof g); g.n = n; g.per = per; g.failAt = f.calls - 1;
    strcpy(err, "untouched");
    rc = h10x_host_write_seq_spans(argv[1], &head, feed, &g, 0, &t, err, (int)sizeof err);
    feed_free(&g);
    if (rc != -2 || strcmp(err, "untouched") || exists(part) || stat(argv[1], &after) || after.st_size != before.st_size || after.st_ino != before.st_ino) return 6;
    char other[1200], otherPart[1300]; snprintf(other, sizeof other, "%s.fail", argv[1]); snprintf(otherPart, sizeof otherPart, "%s.part", other);
    Feed g2; memset(&g2, 0, sizeof g2); g2.n = n; g2.per = per; g2.failAt = 0;
    rc = h10x_host_write_seq_spans(other, &head, feed, &g2, 0, &t, err, (int)sizeof err);
    feed_free(&g2);
    if (rc != -2 || exists(other) || exists(otherPart)) return 6;
  }
  char bad[1200]; snprintf(bad, sizeof bad, "%s.dir/does/not/exist.ss", argv[1]);
  Feed h; memset(&h, 0, sizeof h); h.n = n; h.per = per; h.failAt = UINT64_MAX;
  rc = h10x_host_write_seq_spans(bad, &head, feed, &h, 0, &t, err, (int)sizeof err);
  feed_free(&h);
  if (rc != -1 || strncmp(err, "failed to open output file", 26) || h.calls) return 7;
  printf("%s\n", err);
  return 0;
}
