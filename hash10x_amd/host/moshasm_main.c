/* moshasm_main.c — `moshasm-amd`: the reference's moshasm command loop (moshasm.c:583-695) over a readset that lives on one MI355X
 * (csrc/stage_h.hip) beside its mosh set (csrc/stage_g.hip). Commands run strictly left to right; each is echoed as "COMMAND ..." on
 * stderr and followed by a resource line. Fatal conditions print "FATAL ERROR: <message>" and exit(-1) like die() (utils.c:18-29);
 * where the reference would read freed or null memory, that is what happens here too, with a plain message. The device is opened
 * by -m / -r, not before: usage, unknown commands and bad files behave the same on a machine without a GPU.
 * Additions: --device <n>, --slab <bases> (bases per device batch; results do not depend on it), --chunk <entries> (expanded entries
 * per chunk of queries of the overlap table; results do not depend on it); the resource line also carries wall-clock seconds.
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
  fprintf(stderr, "Usage: moshasm-amd <commands>\n");
  fprintf(stderr, "Long reads as lists of mosh hits, their overlaps, bad and contained reads, on one MI355X.\n");
  fprintf(stderr, "Commands run in the order given, so set things up before the command that needs them:\n");
  fprintf(stderr, "  -v  | --verbose                    toggle verbose mode\n");
  fprintf(stderr, "  -t  | --threads <n>                accepted; the work is on the device\n");
  fprintf(stderr, "  -o  | --output <file>              where the text goes from here on; '-' is stdout\n");
  fprintf(stderr, "  --device <n>                       HIP device (default 0); before -m / -r\n");
  fprintf(stderr, "  --slab <bases>                     bases per device batch of -f (default 2^26); results do not depend on it\n");
  fprintf(stderr, "  --chunk <entries>                  inverse-list entries per chunk of the overlap table (default 2^26); results do not depend on it\n");
  fprintf(stderr, "  -m  | --moshset <mosh file>        the set, with copy classes (moshutils-amd -s)\n");
  fprintf(stderr, "  -f  | --seqfile <sequence file>    build the readset: FASTA / FASTQ, gzipped or not; once per -m\n");
  fprintf(stderr, "  -w  | --write <stem>               writes <stem>.mosh and <stem>.readset\n");
  fprintf(stderr, "  -r  | --read <stem>                reads them\n");
  fprintf(stderr, "  -S  | --stats                      readset statistics\n");
  fprintf(stderr, "  -o1 | --overlaps1 <read>           the overlaps of one read\n");
  fprintf(stderr, "  -o2 | --overlaps2 <k>              overlap counts of every k'th read\n");
  fprintf(stderr, "  -o3 | --overlap <read1> <read2>    the shared copy-1 hits of two reads\n");
  fprintf(stderr, "  -b  | --markBadReads               find and classify bad reads\n");
  fprintf(stderr, "  -c  | --markContained              find contained reads\n");
  fprintf(stderr, "  -a1 | --assemble1 <read>           hit census of the reads that overlap one read\n");
}

static int device = 0;
static uint64_t slab = 0, chunk = 0;
static h10x_mosh *ms = 0;
static h10x_readset *rs = 0;

static void parse_set(const char *path, h10x_moshfile *m) {
  char err[512];
  if (h10x_moshfile_read(path, m, err, (int)sizeof err)) die("%s", err);
  if (m->size - 1 >= 0x80000000u) die("too many entries in moshset");                         /* moshasm.c:652 */
}
static void device_set(h10x_moshfile *m) {
  char err[512];
  if (rs) { h10x_readset_destroy(rs); rs = 0; }              /* a readset does not outlive its set */
  if (ms) { h10x_mosh_destroy(ms); ms = 0; }
  if (h10x_mosh_load(&ms, m->B, m->sh.k, m->sh.w, m->sh.factor1, m->sh.factor2, m->index, m->value, m->depth, m->info, m->size, device, err, (int)sizeof err)) die("%s", err);
  h10x_moshfile_free(m);
  if (slab) h10x_mosh_set_option(ms, "mosh_slab", (int64_t)slab);
  if (chunk) h10x_mosh_set_option(ms, "overlap_chunk", (int64_t)chunk);
}
static void need_rs(const char *cmd) { if (!rs) die("%s needs a readset: give -f or -r first", cmd); }
static uint32_t read_ix(const char *s) {
  const uint32_t ix = (uint32_t)atoi(s);
  h10x_readset_info_t in; h10x_readset_info(rs, &in);
  if (ix >= in.nReads) die("read %u is outside the readset of %u reads", ix, in.nReads - 1);
  return ix;
}

int main(int argc, char *argv[]) {
  --argc; ++argv;
  outFile = stdout;
  timeUpdate(stdout, 0);
  if (!argc) usage();

  int i, fOpen = 0, fromRead = 0; char err[512];

  while (argc) {
    if (**argv != '-') die("option/command %s does not start with '-': run without arguments for usage", *argv);
    fprintf(stderr, "COMMAND %s", *argv);
    for (i = 1; i < argc && *argv[i] != '-'; ++i) fprintf(stderr, " %s", argv[i]);
    fputc('\n', stderr);
    const char *cmd = *argv;

#define ARGMATCH(x, y, n) ((!strcmp(*argv, x) || !strcmp(*argv, y)) && argc >= n && (argc -= n, argv += n))
    if (ARGMATCH("-t", "--threads", 2)) fprintf(stderr, "  can't set thread number - not compiled with OMP\n");
    else if (ARGMATCH("-v", "--verbose", 1)) { }
    else if (ARGMATCH("-o", "--output", 2)) {
      if (!strcmp(argv[-1], "-")) outFile = stdout;
      else if (!(outFile = fopen(argv[-1], "w"))) { fprintf(stderr, "can't open output file %s - resetting to stdout\n", argv[-1]); outFile = stdout; }
    }
    else if (ARGMATCH("--device", "--device", 2)) { if (ms) die("--device comes before -m / -r"); device = atoi(argv[-1]); }
    else if (ARGMATCH("--slab", "--slab", 2)) {
      char *end = 0;
      slab = strtoull(argv[-1], &end, 10);
      if (*argv[-1] == 0 || *end || slab < 1 || slab > 0xFFFFFFFFull) die("bad slab %s: 1 to 4294967295 bases", argv[-1]);
      if (ms) h10x_mosh_set_option(ms, "mosh_slab", (int64_t)slab);
    }
    else if (ARGMATCH("--chunk", "--chunk", 2)) {            /* read when the table is built: before the first -o1 / -o2 / -b / -c of a readset */
      char *end = 0;
      chunk = strtoull(argv[-1], &end, 10);
      if (*argv[-1] == 0 || *end || chunk < 1 || chunk > 0x7FFFFFFFull) die("bad chunk %s: 1 to 2147483647 entries", argv[-1]);
      if (ms) h10x_mosh_set_option(ms, "overlap_chunk", (int64_t)chunk);
    }
    else if (ARGMATCH("-m", "--moshset", 2)) {
      h10x_moshfile m; parse_set(argv[-1], &m); device_set(&m);
      fOpen = 1; fromRead = 0;
      if (h10x_mosh_set_summary(ms, outFile)) die("%s", h10x_mosh_error(ms));
    }
    else if (ARGMATCH("-f", "--seqfile", 2)) {
      if (!ms) fprintf(stderr, "** need to read a moshset before a sequence file\n");
      else {
        if (!fOpen && fromRead) die("-f after -r needs a new -m first (the reference closes a mosh file here that -r never opened)");
        if (!fOpen) die("a second -f needs a new -m first (the reference closes the mosh file twice here)");
        if (rs) { h10x_readset_destroy(rs); rs = 0; }
        if (h10x_readset_create(&rs, ms)) die("%s", h10x_mosh_error(ms));
        char msg[512], warn[256];
        const int rc = h10x_readset_add_file(rs, argv[-1], slab, msg, (int)sizeof msg, warn, (int)sizeof warn);
        if (rc > 0) { if (msg[0]) fprintf(stderr, "%s\n", msg); die("failed to open sequence file %s", argv[-1]); }
        if (rc < 0) die("%s", msg);
        if (warn[0]) fprintf(stderr, "%s\n", warn);
        fOpen = 0;
      }
    }
    else if (ARGMATCH("-r", "--read", 2)) {
      char *path = (char *)malloc(strlen(argv[-1]) + 32);
      if (!path) die("out of host memory");
      sprintf(path, "%s.mosh", argv[-1]);
      { FILE *t = fopen(path, "r"); if (!t) die("can't open file %s.mosh", argv[-1]); fclose(t); }
      h10x_moshfile m; parse_set(path, &m);                    /* both files are parsed before the device is opened */
      sprintf(path, "%s.readset", argv[-1]);
      { FILE *t = fopen(path, "r"); if (!t) die("can't open file %s.readset", argv[-1]); fclose(t); }
      h10x_readsetfile rf;
      if (h10x_readsetfile_read(path, m.size - 1, &rf, err, (int)sizeof err)) die("%s", err);
      device_set(&m);
      fOpen = 0; fromRead = 1;
      if (h10x_readset_load(&rs, ms, rf.reads, rf.max, rf.dim, rf.hit, rf.dx)) die("%s", h10x_mosh_error(ms));
      h10x_readsetfile_free(&rf);
      const h10x_read_t *reads;
      if (h10x_readset_export(rs, &reads, 0, 0, 0)) die("%s", h10x_readset_error(rs));        /* invBuild: the set's depths must be this readset's */
      free(path);
    }
    else if (ARGMATCH("-w", "--write", 2)) {
      need_rs(cmd);
      char *path = (char *)malloc(strlen(argv[-1]) + 32);
      if (!path) die("out of host memory");
      sprintf(path, "%s.mosh", argv[-1]);
      if (h10x_mosh_set_write(ms, path, err, (int)sizeof err)) die("can't open file %s.mosh", argv[-1]);
      sprintf(path, "%s.readset", argv[-1]);
      if (h10x_readset_write_file(rs, path, err, (int)sizeof err)) die("%s", err);
      free(path);
    }
    else if (ARGMATCH("-S", "--stats", 1)) {
      need_rs(cmd);
      const int rc = h10x_readset_print_stats(rs, ms, outFile, err, (int)sizeof err);
      if (rc < 0) die("%s", err);
      if (rc > 0) fprintf(stderr, "stats called on empty readset\n");
    }
    else if (ARGMATCH("-o1", "--overlaps1", 2)) {
      need_rs(cmd);
      if (h10x_readset_print_overlaps(rs, read_ix(argv[-1]), 2, outFile, 0, 0, err, (int)sizeof err)) die("%s", err);
    }
    else if (ARGMATCH("-o2", "--overlaps2", 2)) {
      need_rs(cmd);
      const int d = atoi(argv[-1]);
      if (d < 1) die("-o2 needs a step of at least 1");
      h10x_readset_info_t in; h10x_readset_info(rs, &in);
      for (uint64_t ix = (uint64_t)d; ix < in.nReads; ix += (uint64_t)d)
        if (h10x_readset_print_overlaps(rs, (uint32_t)ix, 1, outFile, 0, 0, err, (int)sizeof err)) die("%s", err);
    }
    else if (ARGMATCH("-o3", "--overlap", 3)) {
      need_rs(cmd);
      const uint32_t a = read_ix(argv[-2]), b = read_ix(argv[-1]);
      if (h10x_readset_print_pair(rs, ms, a, b, outFile, err, (int)sizeof err)) die("%s", err);
    }
    else if (ARGMATCH("-b", "--markBadReads", 1)) {
      need_rs(cmd);
      int32_t found[3];
      if (h10x_readset_mark_bad(rs, found)) die("%s", h10x_readset_error(rs));
      printf("MB  %d with >=10 bad overlaps\n", found[0]);
      printf("MB  %d with multiple bad overlaps\n", found[1]);
      printf("MB  %d with single bad overlaps\n", found[2]);
    }
    else if (ARGMATCH("-c", "--markContained", 1)) {
      need_rs(cmd);
      int32_t nC = 0, nN = 0; uint64_t tot = 0;
      if (h10x_readset_mark_contained(rs, &nC, &nN, &tot)) die("%s", h10x_readset_error(rs));
      printf("MC  found %d contained reads, leaving %d not contained, av length %.1f\n", nC, nN, nN ? tot / (double)nN : 0.);
    }
    else if (ARGMATCH("-a1", "--assemble1", 2)) {
      need_rs(cmd);
      if (h10x_readset_print_assembly(rs, ms, read_ix(argv[-1]), outFile, stdout, err, (int)sizeof err)) die("%s", err);
    }
    else die("unkown command %s - run without arguments for usage", *argv);

    timeUpdate(outFile, 0);
  }

  fprintf(outFile, "total resources used: "); timeUpdate(outFile, 1);
  if (outFile != stdout) { printf("total resources used: "); timeUpdate(stdout, 1); fclose(outFile); }
  if (rs) h10x_readset_destroy(rs);
  if (ms) h10x_mosh_destroy(ms);
  return 0;
}
