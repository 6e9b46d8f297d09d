/* moshmap_main.c — `moshmap-amd`: the reference's moshmap command loop (moshmap.c:298-383) over a Reference that lives on one MI355X
 * (csrc/stage_i.hip) beside its mosh set (csrc/stage_g.hip). Commands run strictly left to right; each is echoed as "COMMAND ..." on
 * stderr and followed by a resource line. Fatal conditions print "FATAL ERROR: <message>" and exit(-1) like die() (utils.c:18-29); -w
 * before any reference, where the reference reads a null pointer, ends the same way with a plain message. The device is opened by -f / -r,
 * not before: usage, unknown commands and bad files behave the same on a machine without a GPU.
 * Additions: --device <n>, --slab <bases> (bases per device batch; results do not depend on it); the resource line also carries
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

static struct { int k, w, s, B; } params = {19, 31, 17, 28};

static void usage(void) {
  fprintf(stderr, "Usage: moshmap-amd <commands>\n");
  fprintf(stderr, "A reference indexed by its moshes, and query sequences placed on it, on one MI355X.\n");
  fprintf(stderr, "Commands are executed in order - set parameters before using them!\n");
  fprintf(stderr, "  -K | --kmer <kmer size> [%d]\n", params.k);
  fprintf(stderr, "  -W | --window <window> [%d]\n", params.w);
  fprintf(stderr, "  -S | --seed <random number seed> [%d]\n", params.s);
  fprintf(stderr, "  -B | --tableBits <hash index table bitcount> [%d]\n", params.B);
  fprintf(stderr, "  -v | --verbose : toggle verbose mode\n");
  fprintf(stderr, "  -t | --threads <n> : accepted; the work is on the device\n");
  fprintf(stderr, "  -o | --output <output filename> : '-' for stdout\n");
  fprintf(stderr, "  --device <n> : HIP device (default 0); before -f / -r\n");
  fprintf(stderr, "  --slab <bases> : bases per device batch (default 2^26); results do not depend on it\n");
  fprintf(stderr, "  -f | --referenceFasta <reference fasta file>\n");
  fprintf(stderr, "  -w | --referenceWrite <file stem> : writes <stem>.mosh and <stem>.ref\n");
  fprintf(stderr, "  -r | --referenceRead <file stem> : reads them\n");
  fprintf(stderr, "  -q | --query <query fasta file>\n");
}

static int device = 0;
static uint64_t slab = 0;
static h10x_mosh *ms = 0;
static h10x_mapref *ref = 0;

static void drop_reference(void) {                           /* a reference does not outlive its set */
  if (ref) { h10x_mapref_destroy(ref); ref = 0; }
  if (ms) { h10x_mosh_destroy(ms); ms = 0; }
}
static char *tagged(const char *stem, const char *tag) {
  char *path = (char *)malloc(strlen(stem) + strlen(tag) + 2);
  if (!path) die("out of host memory");
  sprintf(path, "%s.%s", stem, tag);
  return path;
}

int main(int argc, char *argv[]) {
  --argc; ++argv;
  outFile = stdout;
  timeUpdate(stdout, 0);
  if (!argc) usage();

  int i, isVerbose = 0; char err[512];

  while (argc) {
    if (**argv != '-') die("option/command %s does not start with '-': run without arguments for usage", *argv);
    fprintf(stderr, "COMMAND %s", *argv);
    for (i = 1; i < argc && *argv[i] != '-'; ++i) fprintf(stderr, " %s", argv[i]);
    fputc('\n', stderr);

#define ARGMATCH(x, y, n) ((!strcmp(*argv, x) || !strcmp(*argv, y)) && argc >= n && (argc -= n, argv += n))
    if (ARGMATCH("-K", "--kmer", 2)) params.k = atoi(argv[-1]);
    else if (ARGMATCH("-W", "--window", 2)) params.w = atoi(argv[-1]);
    else if (ARGMATCH("-S", "--seed", 2)) params.s = atoi(argv[-1]);
    else if (ARGMATCH("-B", "--tableBits", 2)) params.B = atoi(argv[-1]);
    else if (ARGMATCH("-t", "--threads", 2)) fprintf(stderr, "  can't set thread number - not compiled with OMP\n");
    else if (ARGMATCH("-v", "--verbose", 1)) isVerbose = !isVerbose;
    else if (ARGMATCH("-o", "--output", 2)) {
      if (!strcmp(argv[-1], "-")) outFile = stdout;
      else if (!(outFile = fopen(argv[-1], "w"))) { fprintf(stderr, "can't open output file %s - resetting to stdout\n", argv[-1]); outFile = stdout; }
    }
    else if (ARGMATCH("--device", "--device", 2)) { if (ms) die("--device comes before -f / -r"); device = atoi(argv[-1]); }
    else if (ARGMATCH("--slab", "--slab", 2)) {
      char *end = 0;
      slab = strtoull(argv[-1], &end, 10);
      if (*argv[-1] == 0 || *end || slab < 1 || slab > 0xFFFFFFFFull) die("bad slab %s: 1 to 4294967295 bases", argv[-1]);
      if (ms) h10x_mosh_set_option(ms, "mosh_slab", (int64_t)slab);
    }
    else if (ARGMATCH("-f", "--referenceFasta", 2)) {
      { FILE *t = fopen(argv[-1], "r"); if (!t) die("failed to open fasta file %s", argv[-1]); fclose(t); }
      if (params.k <= 0 || params.w <= 0) die("k %d, w %d must be > 0", params.k, params.w);
      if (params.k >= 32) die("seqhash k %d must be between 1 and 32\n", params.k);           /* seqhash.c:24 */
      fprintf(outFile, "  moshmap initialised with k = %d, w = %d, random seed = %d\n", params.k, params.w, params.s);
      drop_reference();
      if (h10x_mosh_create(&ms, params.B, params.k, params.w, params.s, device, err, (int)sizeof err)) die("%s", err);
      if (slab) h10x_mosh_set_option(ms, "mosh_slab", (int64_t)slab);
      if (h10x_mapref_from_fasta(&ref, ms, 1u << 26, argv[-1], slab, outFile, err, (int)sizeof err)) die("%s", err);
    }
    else if (ARGMATCH("-q", "--query", 2)) {
      if (!ref) die("need to read a reference before processing query sequences");
      { FILE *t = fopen(argv[-1], "r"); if (!t) die("failed to open query file %s", argv[-1]); fclose(t); }
      if (h10x_mapref_query_file(ref, argv[-1], slab, isVerbose, outFile, stdout, err, (int)sizeof err)) die("%s", err);
    }
    else if (ARGMATCH("-r", "--referenceRead", 2)) {
      char *path = tagged(argv[-1], "mosh");
      { FILE *t = fopen(path, "r"); if (!t) die("failed to open %s.mosh to read", argv[-1]); fclose(t); }
      h10x_moshfile m; h10x_reffile rf;                       /* both files are parsed before the device is opened */
      if (h10x_moshfile_read(path, &m, err, (int)sizeof err)) die("%s", err);
      free(path); path = tagged(argv[-1], "ref");
      { FILE *t = fopen(path, "r"); if (!t) die("failed to open %s.ref to read", argv[-1]); fclose(t); }
      if (h10x_reffile_read(path, m.size - 1, &rf, err, (int)sizeof err)) die("%s", err);
      free(path);
      drop_reference();
      if (h10x_mosh_load(&ms, m.B, m.sh.k, m.sh.w, m.sh.factor1, m.sh.factor2, m.index, m.value, m.depth, m.info, m.size, device, err, (int)sizeof err)) die("%s", err);
      h10x_moshfile_free(&m);
      if (slab) h10x_mosh_set_option(ms, "mosh_slab", (int64_t)slab);
      if (h10x_mapref_from_file(&ref, ms, &rf, err, (int)sizeof err)) die("%s", err);
      h10x_reffile_free(&rf);
    }
    else if (ARGMATCH("-w", "--referenceWrite", 2)) {
      if (!ref) die("-w needs a reference: give -f or -r first");
      char *path = tagged(argv[-1], "mosh");
      if (h10x_mosh_set_write(ms, path, err, (int)sizeof err)) die("failed to open %s.mosh to write", argv[-1]);
      free(path); path = tagged(argv[-1], "ref");
      { FILE *t = fopen(path, "w"); if (!t) die("failed to open %s.ref to write", argv[-1]); fclose(t); }
      if (h10x_mapref_write_file(ref, path, err, (int)sizeof err)) die("%s", err);
      free(path);
    }
    else die("unkown command %s - run without arguments for usage", *argv);

    timeUpdate(outFile, 0);
  }

  fprintf(outFile, "total resources used: "); timeUpdate(outFile, 1);
  if (outFile != stdout) { printf("total resources used: "); timeUpdate(stdout, 1); fclose(outFile); }
  drop_reference();
  return 0;
}
