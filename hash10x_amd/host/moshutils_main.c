/* moshutils_main.c — `moshutils-amd`: the reference's moshutils command loop (moshutils.c:106-233) over mosh sets that live on
 * one MI355X (csrc/stage_g.hip). Commands run strictly left to right; each is echoed as "COMMAND ..." on stderr and followed by a
 * resource line; -c / -r only while no set exists, everything from -w on only when one does, otherwise "unknown command".
 * Fatal conditions print "FATAL ERROR: <message>" and exit(-1) like die() (utils.c:18-29). The device is opened by -c / -r, not
 * before: usage, unknown commands and bad files behave the same on a machine without a GPU.
 * Additions: --device <n>, --slab <bases> (bases per device batch; results do not depend on it), --check <sequence file> (the
 * reader alone, no device); the resource line also carries
 * wall-clock seconds.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <time.h>
#include <sys/resource.h>
#include "h10x_host.h"

static FILE *outFile;

static void die(const char *fmt, ...) {
  va_list ap; va_start(ap, fmt);
  fflush(stdout); if (outFile && outFile != stdout) fflush(outFile);
  fprintf(stderr, "FATAL ERROR: "); vfprintf(stderr, fmt, ap); fprintf(stderr, "\n");
  va_end(ap);
  exit(-1);
}

static double wallNow(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
static void timeUpdate(FILE *f, int total) {                 /* utils.c:122-150 */
  static int first = 1; static struct rusage rOld, rFirst; static double wOld, wFirst;
  struct rusage rNew; getrusage(RUSAGE_SELF, &rNew); double wNew = wallNow();
  if (first) { rFirst = rNew; wFirst = wNew; first = 0; rOld = rNew; wOld = wNew; return; }
  const struct rusage *r0 = total ? &rFirst : &rOld; double w0 = total ? wFirst : wOld;
  long us = (rNew.ru_utime.tv_sec - r0->ru_utime.tv_sec) * 1000000L + (rNew.ru_utime.tv_usec - r0->ru_utime.tv_usec);
  long ss = (rNew.ru_stime.tv_sec - r0->ru_stime.tv_sec) * 1000000L + (rNew.ru_stime.tv_usec - r0->ru_stime.tv_usec);
  fprintf(f, "user\t%ld.%06ld\tsystem\t%ld.%06ld\tmax_RSS\t%ld\twall\t%.6f\n", us / 1000000, us % 1000000, ss / 1000000, ss % 1000000,
          rNew.ru_maxrss - r0->ru_maxrss, wNew - w0);
  rOld = rNew; wOld = wNew;
}

static void usage(void) {
  fprintf(stderr, "Usage: moshutils-amd <commands>\n");
  fprintf(stderr, "Builds, merges, prunes and reports sets of sampled k-mer hashes (\"moshes\") on one MI355X.\n");
  fprintf(stderr, "Commands run in the order given, so set things up before the command that needs them:\n");
  fprintf(stderr, "  -v  | --verbose                         toggle verbose mode\n");
  fprintf(stderr, "  -o  | --output <file>                   where the text goes from here on; '-' is stdout\n");
  fprintf(stderr, "  --device <n>                            HIP device for the set (default 0); before -c / -r\n");
  fprintf(stderr, "  --slab <bases>                          bases per device batch (default 2^26); results do not depend on it\n");
  fprintf(stderr, "  --check <sequence file>                 parse a sequence file as -a would and print its totals; needs no device\n");
  fprintf(stderr, "  -c  | --create [B [k [w [seed]]]]       new empty set; defaults 28 19 31 17, trailing values may be left out\n");
  fprintf(stderr, "  -r  | --read <mosh file>                set from a file; such a set is full and takes no new hashes\n");
  fprintf(stderr, "  -w  | --write <mosh file>\n");
  fprintf(stderr, "  -a  | --add <sequence file>             count the moshes of a FASTA / FASTQ file, gzipped or not\n");
  fprintf(stderr, "  -x  | --add10x <sequence file>          the same for 10x reads: the first 23 bases of reads 1, 3, 5 ... are skipped\n");
  fprintf(stderr, "  -m  | --merge <mosh file>               add the entries and depths of another set\n");
  fprintf(stderr, "  -p  | --prune <min> <max>               keep min <= depth < max (max 0: no upper limit)\n");
  fprintf(stderr, "  -s  | --setcopy <c1min> <c2min> <cMmin> copy class of every entry from its depth\n");
  fprintf(stderr, "  -sM | --setcopyM <cMmin>                class M where depth >= cMmin\n");
  fprintf(stderr, "  -H  | --hist <file>                     depth histogram\n");
  fprintf(stderr, "  -d  | --depths <file> [mosh files...]   per entry: hash, copy class, depth, and its depth in each further set\n");
  fprintf(stderr, "One of -c and -r must come first; it may come only once.\n");
  fprintf(stderr, "To take the union of two files start from an empty set: -c 30 19 31 17 -m X.mosh -m Y.mosh -w XY.mosh\n");
}

static int device = 0;
static uint64_t slab = 0;

static void summary(h10x_mosh *ms, const char *tag) {
  fprintf(outFile, "%s", tag);
  if (h10x_mosh_set_summary(ms, outFile)) die("%s", h10x_mosh_error(ms));
}
static void file_summary(const h10x_moshfile *m, const char *tag) {
  uint32_t *hist = (uint32_t *)malloc(65536 * 4), copy[4];
  if (!hist) die("out of host memory");
  h10x_moshfile_counts(m, hist, copy);
  fprintf(outFile, "%s", tag);
  h10x_mosh_summary_print(outFile, m->sh.k, m->sh.w, m->B, m->size - 1, hist, copy);
  free(hist);
}
static void read_file(const char *path, h10x_moshfile *m) {
  char err[512];
  if (h10x_moshfile_read(path, m, err, (int)sizeof err)) die("%s", err);
}
static h10x_mosh *load_set(const h10x_moshfile *m) {
  char err[512]; h10x_mosh *ms = 0;
  if (h10x_mosh_load(&ms, m->B, m->sh.k, m->sh.w, m->sh.factor1, m->sh.factor2, m->index, m->value, m->depth, m->info, m->size, device, err, (int)sizeof err)) die("%s", err);
  return ms;
}

static void add_file(h10x_mosh *ms, const char *path, int is10x) {
  char msg[512], warn[256]; uint64_t nSeq = 0, totLen = 0, totHash = 0;
  const int rc = h10x_mosh_set_add_file(ms, path, is10x, slab, &nSeq, &totLen, &totHash, msg, (int)sizeof msg, warn, (int)sizeof warn);
  if (rc > 0) { if (msg[0]) fprintf(stderr, "%s\n", msg); die("failed to open sequence file %s", path); }
  if (warn[0]) fprintf(stderr, "%s\n", warn);
  if (rc < 0) die("%s", msg);
  h10x_mosh_info_t in; h10x_mosh_info(ms, &in);
  fprintf(outFile, "added %llu sequences total length %llu total hashes %llu, new max %u\n",
          (unsigned long long)nSeq, (unsigned long long)totLen, (unsigned long long)totHash, in.max);
  summary(ms, is10x ? "add10x " : "add ");
}

/* --check: the sequence reader alone (no device): what -a would be given */
static void check_file(const char *path) {
  char msg[512]; int fatal = 0;
  h10x_seqreader *r = h10x_seq_open(path, msg, (int)sizeof msg, &fatal);
  if (!r) { if (fatal) die("%s", msg); if (msg[0]) fprintf(stderr, "%s\n", msg); die("failed to open sequence file %s", path); }
  int rc; uint64_t nSeq = 0, bases = 0;
  while ((rc = h10x_seq_next(r, slab, 0, 0, 0)) > 0) { }
  if (h10x_seq_warning(r)[0]) fprintf(stderr, "%s\n", h10x_seq_warning(r));
  if (rc < 0) { snprintf(msg, sizeof msg, "%s", h10x_seq_error(r)); h10x_seq_close(r); die("%s", msg); }
  h10x_seq_totals(r, &nSeq, &bases);
  h10x_seq_close(r);
  fprintf(outFile, "checked %llu sequences total length %llu\n", (unsigned long long)nSeq, (unsigned long long)bases);
}

static void report_depths(h10x_mosh *ms, h10x_mosh **others, int nOthers, FILE *f) {   /* moshutils.c:64-76 */
  h10x_mosh_info_t in; h10x_mosh_info(ms, &in);
  const uint32_t n1 = in.max + 1;
  uint64_t *v = (uint64_t *)malloc((size_t)n1 * 8); uint16_t *d = (uint16_t *)malloc((size_t)n1 * 2); uint8_t *fl = (uint8_t *)malloc(n1);
  uint16_t **od = (uint16_t **)calloc((size_t)nOthers + 1, sizeof *od);
  if (!v || !d || !fl || !od) die("out of host memory");
  if (h10x_mosh_export(ms, 0, 0, 0, v, d, fl)) die("%s", h10x_mosh_error(ms));
  for (int j = 0; j < nOthers; ++j) {
    od[j] = (uint16_t *)malloc((size_t)n1 * 2);
    if (!od[j]) die("out of host memory");
    if (h10x_mosh_lookup(others[j], v, n1, 0, od[j])) die("%s", h10x_mosh_error(others[j]));
  }
  for (uint32_t i = 1; i < n1; ++i) {
    fprintf(f, "MH\t%llx\t%d\t%u", (unsigned long long)v[i], fl[i] & 3, d[i]);
    for (int j = 0; j < nOthers; ++j) fprintf(f, "\t%u", od[j][i]);
    fputc('\n', f);
  }
  for (int j = 0; j < nOthers; ++j) free(od[j]);
  free(od); free(v); free(d); free(fl);
}

int main(int argc, char *argv[]) {
  --argc; ++argv;
  if (!argc) usage();
  outFile = stdout;
  timeUpdate(stdout, 0);

  h10x_mosh *ms = 0;
  int i; FILE *f;

  while (argc) {
    if (**argv != '-') die("option/command %s does not start with '-': run without arguments for usage", *argv);
    fprintf(stderr, "COMMAND %s", *argv);
    for (i = 1; i < argc && *argv[i] != '-'; ++i) fprintf(stderr, " %s", argv[i]);
    fputc('\n', stderr);

#define ARGMATCH(x, y, n) ((!strcmp(*argv, x) || !strcmp(*argv, y)) && argc >= n && (argc -= n, argv += n))
    if (ARGMATCH("-v", "--verbose", 1)) { }
    else if (ARGMATCH("-o", "--output", 2)) {
      if (!strcmp(argv[-1], "-")) outFile = stdout;
      else if (!(outFile = fopen(argv[-1], "w"))) { fprintf(stderr, "can't open output file %s - resetting to stdout\n", argv[-1]); outFile = stdout; }
    }
    else if (!ms && ARGMATCH("--device", "--device", 2)) device = atoi(argv[-1]);
    else if (ARGMATCH("--slab", "--slab", 2)) {
      char *end = 0;
      slab = strtoull(argv[-1], &end, 10);
      if (*argv[-1] == 0 || *end || slab < 1 || slab > 0xFFFFFFFFull) die("bad slab %s: 1 to 4294967295 bases", argv[-1]);
      if (ms) h10x_mosh_set_option(ms, "mosh_slab", (int64_t)slab);
    }
    else if (ARGMATCH("--check", "--check", 2)) check_file(argv[-1]);
    else if (!ms && ARGMATCH("-c", "--create", 1)) {         /* moshutils.c:135-153, accept / reject as it does */
      int B = 28, k = 19, w = 31, s = 17;
      if (argc && **argv != '-') {
        if (!(B = atoi(*argv)) || B < 20 || B > 34) die("bad moshbuild B %s", *argv);
        if (--argc && **++argv != '-') {
          if (!(k = atoi(*argv)) || k < 1) die("bad moshbuild k %s", *argv);
          if (--argc && **++argv != '-') {
            if (!(w = atoi(*argv)) || k < 1) die("bad moshbuild w %s", *argv);
            if (--argc && **++argv != '-') {
              if (!(s = atoi(*argv))) die("bad moshbuild w %s", *argv);
              --argc; ++argv;
            }
          }
        }
      }
      char err[512];
      if (h10x_mosh_create(&ms, B, k, w, s, device, err, (int)sizeof err)) die("%s", err);
      if (slab) h10x_mosh_set_option(ms, "mosh_slab", (int64_t)slab);
    }
    else if (!ms && ARGMATCH("-r", "--read", 2)) {
      h10x_moshfile m; read_file(argv[-1], &m);
      ms = load_set(&m);
      h10x_moshfile_free(&m);
      if (slab) h10x_mosh_set_option(ms, "mosh_slab", (int64_t)slab);
      h10x_mosh_info_t in; h10x_mosh_info(ms, &in);
      fprintf(outFile, "SH k %d  w %d\n", in.k, in.w);
      summary(ms, "read ");
    }
    else if (ms && ARGMATCH("-w", "--write", 2)) {
      char err[512];
      if (h10x_mosh_set_write(ms, argv[-1], err, (int)sizeof err)) die("%s", err);
    }
    else if (ms && ARGMATCH("-p", "--prune", 3)) {
      uint32_t n0 = 0, n1 = 0; const int mn = atoi(argv[-2]), mx = atoi(argv[-1]);
      if (h10x_mosh_prune(ms, mn, mx, &n0, &n1)) die("%s", h10x_mosh_error(ms));
      fprintf(stderr, "  pruned Moshset from %d to %d with min %d <= depth < max %d\n", (int)n0, (int)n1, mn, mx);
      summary(ms, "prune ");
    }
    else if (ms && ARGMATCH("-s", "--setcopy", 4)) {
      if (h10x_mosh_set_copy(ms, atoi(argv[-3]), atoi(argv[-2]), atoi(argv[-1]))) die("%s", h10x_mosh_error(ms));
      summary(ms, "setcopy ");
    }
    else if (ms && ARGMATCH("-sM", "--setcopyM", 2)) {
      if (h10x_mosh_set_copy_m(ms, atoi(argv[-1]))) die("%s", h10x_mosh_error(ms));
      summary(ms, "setcopyM ");
    }
    else if (ms && ARGMATCH("-a", "--add", 2)) add_file(ms, argv[-1], 0);
    else if (ms && ARGMATCH("-x", "--add10x", 2)) add_file(ms, argv[-1], 1);
    else if (ms && ARGMATCH("-m", "--merge", 2)) {
      h10x_moshfile m; read_file(argv[-1], &m);
      file_summary(&m, "read ");
      int merged = 0;
      if (h10x_mosh_merge(ms, m.sh.k, m.sh.w, m.sh.factor1, m.value, m.depth, m.info, m.size, &merged)) die("%s", h10x_mosh_error(ms));
      if (!merged) fprintf(stderr, "moshset %s incompatible with current - unable to merge\n", argv[-1]);
      h10x_moshfile_free(&m);
      summary(ms, "merge ");
    }
    else if (ms && ARGMATCH("-H", "--hist", 2)) {
      if (!(f = fopen(argv[-1], "w"))) die("failed to open histogram file %s", argv[-1]);
      uint32_t *hist = (uint32_t *)malloc(65536 * 4);
      if (!hist) die("out of host memory");
      if (h10x_mosh_summary(ms, hist, 0)) die("%s", h10x_mosh_error(ms));
      for (uint32_t d = 0; d < 65536; ++d) if (hist[d]) fprintf(f, "DP\t%u\t%u\n", d, hist[d]);   /* moshutils.c:52-62 */
      free(hist); fclose(f);
    }
    else if (ms && ARGMATCH("-d", "--depths", 2)) {
      FILE *fd;
      if (!(fd = fopen(argv[-1], "w"))) die("failed to open depths file %s", argv[-1]);
      h10x_mosh *others[64]; int nOthers = 0;
      while (argc && **argv != '-') {
        if (nOthers == 64) die("-d takes at most 64 further mosh files");
        h10x_moshfile m; read_file(*argv, &m);
        file_summary(&m, "read ");
        others[nOthers++] = load_set(&m);
        h10x_moshfile_free(&m);
        --argc; ++argv;
      }
      report_depths(ms, others, nOthers, fd);
      for (i = 0; i < nOthers; ++i) h10x_mosh_destroy(others[i]);
      fclose(fd);
    }
    else die("unknown command %s - run without arguments for usage", *argv);

    timeUpdate(outFile, 0);
  }

  fprintf(outFile, "total resources used: "); timeUpdate(outFile, 1);
  if (outFile != stdout) { printf("total resources used: "); timeUpdate(stdout, 1); fclose(outFile); }
  if (ms) h10x_mosh_destroy(ms);
  return 0;
}
