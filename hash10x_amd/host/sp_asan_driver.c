/* The .sp writer of files_host.c (h10x_host_write_seq_spectrum) behind a main of its own, for the AddressSanitizer + UBSan build
   (tests/test_seq_spectrum_cpu.py): it needs no device.   sp_asan_driver <out.sp> <nSeq> <seqsPerSlab> <hashNumber>
   Thresholds 2, 4, 6, window 4, k 21. Sequence q is called "s<q>" and has 10 q + 1 bases, so ceil(len / 4) windows; window j of it has absent (q + j) % 2,
   n0 (q + j) % 3, n1 j % 2, n2 q % 2, nM (q j) % 2 (all but absent 0 when hashNumber is 1: a state without hashes finds nothing), moshes their sum and depthSum 3 x
   found; the sequence's figures are the sums of its windows. Hash x = 1 .. hashNumber - 1 has depth x % 9, or 2000 where x % 500 == 499, and the F found
   occurrences of all sequences are dealt to the hashes evenly, the first F % (hashNumber - 1) hashes one more: that is copies[]. The spectrum and the totals
   follow from depth and copies. The slabs hold seqsPerSlab sequences each (0: all in one). Then each of the three callbacks fails once over the file that stands
   there, and a path that cannot be opened is tried: none may leave a .part behind, and the old file keeps its bytes. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include "h10x_host.h"

enum { WINDOW = 4, C1 = 2, C2 = 4, CM = 6, K = 21 };

typedef struct {
  uint64_t next, n, per, calls, failAt, hashNumber, found; int failEnd, failCopies, ended; uint64_t copyCalls;
  uint64_t *winOff, *nameOff; h10x_seq_spectrum_figures *fig; h10x_seq_spectrum_window *win; char *names;
} Feed;

static void feed_free(Feed *f) { free(f->winOff); free(f->nameOff); free(f->fig); free(f->win); free(f->names); f->winOff = f->nameOff = 0; f->fig = 0; f->win = 0; f->names = 0; }

static h10x_seq_spectrum_window window_of(uint64_t q, uint64_t j, uint64_t hashNumber) {
  h10x_seq_spectrum_window w; memset(&w, 0, sizeof w);
  w.absent = (uint32_t)((q + j) % 2);
  if (hashNumber > 1) { w.n0 = (uint32_t)((q + j) % 3); w.n1 = (uint32_t)(j % 2); w.n2 = (uint32_t)(q % 2); w.nM = (uint32_t)((q * j) % 2); }
  w.moshes = w.absent + w.n0 + w.n1 + w.n2 + w.nM; w.depthSum = 3ull * (w.moshes - w.absent);
  return w;
}
static uint64_t windows_of(uint64_t q) { return (10 * q + 1 + WINDOW - 1) / WINDOW; }
static uint64_t found_of_all(uint64_t n, uint64_t hashNumber) {
  uint64_t f = 0;
  for (uint64_t q = 0; q < n; ++q) for (uint64_t j = 0; j < windows_of(q); ++j) { const h10x_seq_spectrum_window w = window_of(q, j, hashNumber); f += w.moshes - w.absent; }
  return f;
}
static uint32_t depth_of(uint64_t x) { return x % 500 == 499 ? 2000u : (uint32_t)(x % 9); }
static uint32_t copies_of(const Feed *f, uint64_t x) {
  if (!x || f->hashNumber < 2) return 0;
  const uint64_t m = f->hashNumber - 1;
  return (uint32_t)(f->found / m + (x <= f->found % m));
}

static int feed(void *user, h10x_seq_spectrum_slab *b) {
  Feed *f = (Feed *)user;
  if (f->calls == f->failAt) return -1;
  if (f->next >= f->n) return 0;
  const uint64_t per = f->per ? f->per : f->n, m = f->n - f->next < per ? f->n - f->next : per;
  uint64_t wins = 0;
  for (uint64_t i = 0; i < m; ++i) wins += windows_of(f->next + i);
  feed_free(f);
  f->winOff = (uint64_t *)calloc(m + 1, 8); f->nameOff = (uint64_t *)calloc(m + 1, 8); f->fig = (h10x_seq_spectrum_figures *)calloc(m, sizeof *f->fig);
  f->win = (h10x_seq_spectrum_window *)calloc(wins + 1, sizeof *f->win); f->names = (char *)calloc(m, 24);
  if (!f->winOff || !f->nameOff || !f->fig || !f->win || !f->names) return -1;
  uint64_t nameAt = 0;
  for (uint64_t i = 0; i < m; ++i) {
    const uint64_t q = f->next + i;
    h10x_seq_spectrum_figures *g = f->fig + i; g->len = 10 * q + 1;
    uint64_t at = f->winOff[i];
    for (uint64_t j = 0; j < windows_of(q); ++j, ++at) {
      const h10x_seq_spectrum_window w = window_of(q, j, f->hashNumber);
      f->win[at] = w;
      g->moshes += w.moshes; g->absent += w.absent; g->n0 += w.n0; g->n1 += w.n1; g->n2 += w.n2; g->nM += w.nM; g->depthSum += w.depthSum;
    }
    f->winOff[i + 1] = at;
    f->nameOff[i] = nameAt;
    nameAt += (uint64_t)snprintf(f->names + nameAt, 24, "s%llu", (unsigned long long)q) + 1;
  }
  b->nSeq = (uint32_t)m; b->fig = f->fig; b->winOff = f->winOff; b->win = f->win; b->names = f->names; b->nameOff = f->nameOff;
  f->next += m; ++f->calls;
  return 1;
}

static int feed_end(void *user, uint64_t *spectrum, uint64_t *totals) {
  Feed *f = (Feed *)user;
  if (f->failEnd) return -1;
  f->ended = 1;
  for (uint64_t x = 1; x < f->hashNumber; ++x) {
    const uint32_t d = depth_of(x), c = copies_of(f, x), q = d < C1 ? 0 : d < C2 ? 1 : d < CM ? 2 : 3;
    ++spectrum[(uint64_t)(d < H10X_SPECTRUM_DEPTH_BINS - 1 ? d : H10X_SPECTRUM_DEPTH_BINS - 1) * H10X_SPECTRUM_COPY_BINS + (c < H10X_SPECTRUM_COPY_BINS - 1 ? c : H10X_SPECTRUM_COPY_BINS - 1)];
    ++totals[q]; totals[4 + q] += c >= 1;
  }
  return 0;
}

static int feed_copies(void *user, uint64_t first, uint64_t count, uint32_t *out) {
  Feed *f = (Feed *)user;
  if (f->failCopies || !f->ended || first + count > f->hashNumber || count > (1u << 22)) return -1;
  for (uint64_t i = 0; i < count; ++i) out[i] = first + i ? copies_of(f, first + i) : 77;   /* (the writer owes byte 0 = 0 whatever it is given) */
  ++f->copyCalls;
  return 0;
}

static int exists(const char *p) { struct stat st; return stat(p, &st) == 0; }
static Feed feed_new(uint64_t n, uint64_t per, uint64_t hashNumber) {
  Feed f; memset(&f, 0, sizeof f); f.n = n; f.per = per; f.hashNumber = hashNumber; f.failAt = UINT64_MAX; f.found = found_of_all(n, hashNumber);
  return f;
}

int main(int argc, char **argv) {
  if (argc != 5) { fprintf(stderr, "usage: sp_asan_driver <out.sp> <nSeq> <seqsPerSlab> <hashNumber>\n"); return 2; }
  const uint64_t n = strtoull(argv[2], 0, 10), per = strtoull(argv[3], 0, 10), hashNumber = strtoull(argv[4], 0, 10);
  if (!hashNumber || hashNumber > 0xFFFFFFFFull) return 2;
  char err[256] = "", part[1200]; snprintf(part, sizeof part, "%s.part", argv[1]);
  const h10x_seq_spectrum_head head = {(uint32_t)hashNumber, C1, C2, CM, WINDOW, K};
  h10x_seq_spectrum_totals t;
  Feed f = feed_new(n, per, hashNumber);
  int rc = h10x_host_write_seq_spectrum(argv[1], &head, feed, feed_end, feed_copies, &f, stdout, &t, err, (int)sizeof err);
  feed_free(&f);
  if (rc) { fprintf(stderr, "%s\n", err); return 4; }
  if (f.next != n || t.nSeq != n || exists(part) || !exists(argv[1])) { fprintf(stderr, "the slabs do not tile the %llu sequences\n", (unsigned long long)n); return 5; }
  if (f.copyCalls != (hashNumber + (1u << 22) - 1) >> 22) { fprintf(stderr, "%llu pieces of copies\n", (unsigned long long)f.copyCalls); return 5; }
  printf("%llu slabs, %llu windows, %llu moshes, %llu absent, %llu found, present %llu of %llu, QV %.2f\n", (unsigned long long)f.calls, (unsigned long long)t.windows,
         (unsigned long long)t.moshes, (unsigned long long)t.absent, (unsigned long long)f.found,
         (unsigned long long)(t.present[0] + t.present[1] + t.present[2] + t.present[3]), (unsigned long long)(t.total[0] + t.total[1] + t.total[2] + t.total[3]),
         h10x_host_qv(t.moshes, t.absent + t.n0, K));
  struct stat before, after;
  if (stat(argv[1], &before)) return 6;
  for (int what = 0; what < 3; ++what) {                      /* a failing callback over the file just written: -2, err untouched, no .part, the old bytes kept */
    if (what == 0 && !n) continue;
    Feed g = feed_new(n, per, hashNumber);
    if (what == 0) g.failAt = f.calls - 1; else if (what == 1) g.failEnd = 1; else g.failCopies = 1;
    strcpy(err, "untouched");
    rc = h10x_host_write_seq_spectrum(argv[1], &head, feed, feed_end, feed_copies, &g, 0, &t, err, (int)sizeof err);
    feed_free(&g);
    if (rc != -2 || strcmp(err, "untouched") || exists(part) || stat(argv[1], &after) || after.st_size != before.st_size || after.st_ino != before.st_ino) return 6;
  }
  {
    char other[1200], otherPart[1300]; snprintf(other, sizeof other, "%s.fail", argv[1]); snprintf(otherPart, sizeof otherPart, "%s.part", other);
    Feed g2 = feed_new(n, per, hashNumber); g2.failEnd = 1;
    rc = h10x_host_write_seq_spectrum(other, &head, feed, feed_end, feed_copies, &g2, 0, &t, err, (int)sizeof err);
    feed_free(&g2);
    if (rc != -2 || exists(other) || exists(otherPart)) return 6;
  }
  char bad[1200]; snprintf(bad, sizeof bad, "%s.dir/does/not/exist.sp", argv[1]);
  Feed h = feed_new(n, per, hashNumber);
  rc = h10x_host_write_seq_spectrum(bad, &head, feed, feed_end, feed_copies, &h, 0, &t, err, (int)sizeof err);
  feed_free(&h);
  if (rc != -1 || strncmp(err, "failed to open output file", 26) || h.calls) return 7;
  printf("%s\n", err);
  return 0;
}
