/* The .sb writer of files_host.c (h10x_host_write_seq_blocks) behind a main of its own, for the AddressSanitizer + UBSan build
   (tests/test_seq_blocks_cpu.py): it needs no device.   sb_asan_driver <out.sb> <nSeq> <seqsPerSlab>
   Sequence q is called "s<q>", has q % 5 + 1 bases and q % 4 rows {block q + i + 1, count 2 q + i + 1}; its figures are moshes q % 11, found q % 7,
   query q % 3. The slabs hold seqsPerSlab sequences each (0: all in one). Then the
   callback fails in its last slab, and a path that cannot be opened is tried: neither may leave a .part behind. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include "h10x_host.h"

typedef struct {
  uint64_t next, n, per, calls, failAt;
  uint64_t *seqStart, *rowOff, *nameOff; h10x_seq_figures *fig; uint32_t *block, *count; char *names;
} Feed;

static int feed(void *user, h10x_seq_blocks_slab *b) {
  Feed *f = (Feed *)user;
  if (f->calls == f->failAt) return -1;
  if (f->next >= f->n) return 0;
  const uint64_t per = f->per ? f->per : f->n, m = f->n - f->next < per ? f->n - f->next : per;
  free(f->seqStart); free(f->rowOff); free(f->nameOff); free(f->fig); free(f->block); free(f->count); free(f->names);
  f->seqStart = (uint64_t *)calloc(m + 1, 8); f->rowOff = (uint64_t *)calloc(m + 1, 8); f->nameOff = (uint64_t *)calloc(m + 1, 8);
  f->fig = (h10x_seq_figures *)calloc(m, sizeof *f->fig); f->block = (uint32_t *)calloc(3 * m + 1, 4); f->count = (uint32_t *)calloc(3 * m + 1, 4);
  f->names = (char *)calloc(m, 24);
  if (!f->seqStart || !f->rowOff || !f->nameOff || !f->fig || !f->block || !f->count || !f->names) return -1;
  uint64_t nameAt = 0;
  for (uint64_t i = 0; i < m; ++i) {
    const uint64_t q = f->next + i;
    f->seqStart[i + 1] = f->seqStart[i] + q % 5 + 1;
    f->fig[i].moshes = (uint32_t)(q % 11); f->fig[i].found = (uint32_t)(q % 7); f->fig[i].query = (uint32_t)(q % 3); f->fig[i].entries = q;
    uint64_t r = f->rowOff[i];
    for (uint64_t k = 0; k < q % 4; ++k, ++r) { f->block[r] = (uint32_t)(q + k + 1); f->count[r] = (uint32_t)(2 * q + k + 1); }
    f->rowOff[i + 1] = r;
    f->nameOff[i] = nameAt;
    nameAt += (uint64_t)snprintf(f->names + nameAt, 24, "s%llu", (unsigned long long)q) + 1;
  }
  b->nSeq = (uint32_t)m; b->seqStart = f->seqStart; b->fig = f->fig; b->rowOff = f->rowOff; b->block = f->block; b->count = f->count;
  b->names = f->names; b->nameOff = f->nameOff;
  f->next += m; ++f->calls;
  return 1;
}

static void feed_free(Feed *f) { free(f->seqStart); free(f->rowOff); free(f->nameOff); free(f->fig); free(f->block); free(f->count); free(f->names); }
static int exists(const char *p) { struct stat st; return stat(p, &st) == 0; }

int main(int argc, char **argv) {
  if (argc != 4) { fprintf(stderr, "usage: sb_asan_driver <out.sb> <nSeq> <seqsPerSlab>\n"); return 2; }
  const uint64_t n = strtoull(argv[2], 0, 10), per = strtoull(argv[3], 0, 10);
  char err[256] = "", part[1200]; snprintf(part, sizeof part, "%s.part", argv[1]);
  h10x_seq_blocks_totals t;
  Feed f; memset(&f, 0, sizeof f); f.n = n; f.per = per; f.failAt = UINT64_MAX;
  int rc = h10x_host_write_seq_blocks(argv[1], 1000000, 3, feed, &f, 0, &t, err, (int)sizeof err);
  feed_free(&f);
  if (rc) { fprintf(stderr, "%s\n", err); return 4; }
  if (f.next != n || t.nSeq != n || exists(part) || !exists(argv[1])) { fprintf(stderr, "the slabs do not tile the %llu sequences\n", (unsigned long long)n); return 5; }
  printf("%llu slabs, %llu rows, %llu with rows, max count %u\n", (unsigned long long)f.calls, (unsigned long long)t.rows, (unsigned long long)t.withRows, t.maxCount);
  if (n) {                                                    /* a failing callback: -2, err untouched, nothing left behind */
    char other[1200], otherPart[1300]; snprintf(other, sizeof other, "%s.fail", argv[1]); snprintf(otherPart, sizeof otherPart, "%s.part", other);
    Feed g; memset(&g, 0, sizeof g); g.n = n; g.per = per; g.failAt = f.calls - 1;
    strcpy(err, "untouched");
    rc = h10x_host_write_seq_blocks(other, 1000000, 3, feed, &g, 0, &t, err, (int)sizeof err);
    feed_free(&g);
    if (rc != -2 || strcmp(err, "untouched") || exists(other) || exists(otherPart)) return 6;
  }
  char bad[1200]; snprintf(bad, sizeof bad, "%s.dir/does/not/exist.sb", argv[1]);
  Feed h; memset(&h, 0, sizeof h); h.n = n; h.per = per; h.failAt = UINT64_MAX;
  rc = h10x_host_write_seq_blocks(bad, 1000000, 3, feed, &h, 0, &t, err, (int)sizeof err);
  feed_free(&h);
  if (rc != -1 || strncmp(err, "failed to open output file", 26) || h.calls) return 7;
  printf("%s\n", err);
  return 0;
}
