/* map_host.c — host side of moshmap-amd: the name dictionary (a restatement of dict.c of the reference: its hash, its probing, its
 * doubling and its file layout), the RFMSHv1 file (referenceWrite / referenceRead, moshmap.c:135-181, over arrayWrite's and dictWrite's
 * layouts), the Q / M / verbose texts (moshmap.c:207-209, 219-229, 255-260) and the file-level commands over the h10x_refmap_* entry
 * points of include/h10x.h. The dictionary, the file code and the formatters touch no device.
 */
#define _GNU_SOURCE
#include "h10x_host.h"
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <sys/stat.h>

enum { ARRAY_MAGIC = 8918274 };
typedef struct { int32_t magic, pad0; uint64_t base; int32_t dim, size, max, pad1; } ArrayHead;   /* struct ArrayStruct (array.h:41-50) */
_Static_assert(sizeof(ArrayHead) == 32, "the ArrayStruct of the file");

static int set_msg(char *dst, int len, const char *fmt, ...) {
  va_list ap; va_start(ap, fmt); if (dst && len > 0) vsnprintf(dst, (size_t)len, fmt, ap); va_end(ap);
  return -1;
}

/* ------------------------------------------------------------------------------------------------ the name dictionary */
/* hashString (dict.c:45-63): a rotate-and-xor over the bytes as signed chars, folded to `bits` bits; its second loop never runs for
   bits >= 4. The stride of the probe walk is the same with another rotation, made odd. */
static uint32_t name_hash(const char *s, int bits, int stride) {
  const int rot = stride ? 21 : 13;
  uint32_t x = 0;
  for (; *s; ++s) x = (uint32_t)(int32_t)(signed char)*s ^ ((x >> (32 - rot)) | (x << rot));
  x &= (1u << bits) - 1;
  return stride ? x | 1 : x;
}
h10x_namedict *h10x_namedict_create(int size) {              /* dictCreate (dict.c:67-75) */
  h10x_namedict *d = (h10x_namedict *)calloc(1, sizeof *d);
  if (!d) return 0;
  for (d->dim = 10, d->size = 1024; d->size < size; ++d->dim, d->size *= 2) ;
  d->table = (int32_t *)calloc((size_t)d->size, 4);
  d->names = (char **)calloc((size_t)d->size / 2, sizeof(char *));
  if (!d->table || !d->names) { h10x_namedict_destroy(d); return 0; }
  return d;
}
void h10x_namedict_destroy(h10x_namedict *d) {
  if (!d) return;
  if (d->names) for (int i = 1; i <= d->max; ++i) free(d->names[i]);
  free(d->names); free(d->table); free(d);
}
/* the slot a name sits in (*found = its index from 1), or the empty slot its walk ends at (*found = 0); compare = 0 walks to the empty slot */
static uint32_t dict_slot(const h10x_namedict *d, const int32_t *table, const char *s, int compare, int *found) {
  uint32_t x = name_hash(s, d->dim, 0), step = 0;
  *found = 0;
  for (;;) {
    const int32_t i = table[x];
    if (!i) return x;
    if (compare && !strcmp(s, d->names[i])) { *found = i; return x; }
    if (!step) step = name_hash(s, d->dim, 1);
    x = (x + step) & ((1u << d->dim) - 1);
  }
}
int h10x_namedict_find(const h10x_namedict *d, const char *s, int *ip) {
  int found;
  dict_slot(d, d->table, s, 1, &found);
  if (found && ip) *ip = found - 1;
  return found != 0;
}
/* dictAdd (dict.c:160-195): 1 = added, 0 = already there, -1 = out of memory; *ip = index from 0 */
int h10x_namedict_add(h10x_namedict *d, const char *s, int *ip) {
  int found;
  const uint32_t at = dict_slot(d, d->table, s, 1, &found);
  if (found) { if (ip) *ip = found - 1; return 0; }
  char *copy = strdup(s);
  if (!copy) return -1;
  const int i = ++d->max;
  d->table[at] = i; d->names[i] = copy;
  if (ip) *ip = i - 1;
  if (d->max > 0.3 * d->size) {                              /* double the table and place every name again, in index order */
    int32_t *nt = (int32_t *)calloc((size_t)d->size * 2, 4);
    char **nn = (char **)realloc(d->names, (size_t)d->size * sizeof(char *));
    if (nn) { memset(nn + d->size / 2, 0, (size_t)(d->size - d->size / 2) * sizeof(char *)); d->names = nn; }
    if (!nt || !nn) { free(nt); return -1; }
    ++d->dim; d->size *= 2;
    for (int j = 1; j <= d->max; ++j) nt[dict_slot(d, nt, d->names[j], 0, &found)] = j;
    free(d->table); d->table = nt;
  }
  return 1;
}
const char *h10x_namedict_name(const h10x_namedict *d, uint32_t i) { return i < (uint32_t)d->max ? d->names[i + 1] : "?"; }

/* ------------------------------------------------------------------------------------------------ RFMSHv1 */
void h10x_reffile_free(h10x_reffile *r) {
  if (!r) return;
  free(r->index); free(r->offset); free(r->id); free(r->depth); free(r->rev); free(r->loc); free(r->len);
  h10x_namedict_destroy(r->dict);
  memset(r, 0, sizeof *r);
}
/* referenceRead's file half (moshmap.c:163-179) with what a file from outside needs; the reference checks the header only */
int h10x_reffile_read(const char *path, uint32_t setMax, h10x_reffile *r, char *err, int errlen) {
  memset(r, 0, sizeof *r);
  FILE *f = fopen(path, "rb");
  if (!f) return set_msg(err, errlen, "failed to open %s to read", path);
  int rc = -1; char name[8]; ArrayHead a; struct stat sb; uint32_t size;
#define FAIL(...) do { set_msg(err, errlen, __VA_ARGS__); goto out; } while (0)
  if (fstat(fileno(f), &sb)) FAIL("can't stat file %s", path);
  uint64_t left = (uint64_t)sb.st_size;
#define TAKE(ptr, bytes, what) do { if (left < (uint64_t)(bytes) || fread(ptr, 1, (size_t)(bytes), f) != (size_t)(bytes)) FAIL(what); left -= (uint64_t)(bytes); } while (0)
  TAKE(name, 8, "failed to read reference header");
  if (memcmp(name, "RFMSHv1", 8)) FAIL("bad reference header");
  TAKE(&size, 4, "failed to read size");
  TAKE(&r->max, 4, "failed to read max");
  if (size != r->max) FAIL("reference file %s: size %u differs from max %u", path, size, r->max);
  r->setMax = setMax;
  const uint64_t nb = (uint64_t)r->max * 4, sb1 = ((uint64_t)setMax + 1) * 4;
  if (left < 4 * nb + 2 * sb1) FAIL("reference file %s: %u hits over a set of %u do not fit its %llu bytes", path, r->max, setMax, (unsigned long long)sb.st_size);
  r->index = (uint32_t *)malloc(nb + 4); r->offset = (uint32_t *)malloc(nb + 4); r->id = (uint32_t *)malloc(nb + 4); r->rev = (uint32_t *)malloc(nb + 4);
  r->depth = (uint32_t *)malloc(sb1); r->loc = (uint32_t *)malloc(sb1);
  if (!r->index || !r->offset || !r->id || !r->rev || !r->depth || !r->loc) FAIL("out of host memory for reference file %s", path);
  TAKE(r->index, nb, "failed read ref index");
  TAKE(r->offset, nb, "failed read ref offset");
  TAKE(r->id, nb, "failed read ref id");
  TAKE(r->depth, sb1, "fail depth");                         /* max + 1 entries: the reference reads them into an array of max */
  TAKE(r->rev, nb, "fail rev");
  TAKE(r->loc, sb1, "fail loc");
  TAKE(&a, sizeof a, "failed read ref len");
  if (a.size != 4 || a.max < 0 || a.dim < a.max || left < (uint64_t)a.dim * 4) FAIL("failed read ref len");
  r->lenDim = a.dim; r->lenMax = a.max;
  r->len = (uint32_t *)calloc((size_t)a.dim + 1, 4);
  if (!r->len) FAIL("out of host memory for reference file %s", path);
  TAKE(r->len, (uint64_t)a.dim * 4, "failed read ref len");
  {
    int32_t dim, dmax;
    TAKE(&dim, 4, "failed read ref dict");
    TAKE(&dmax, 4, "failed read ref dict");
    if (dim < 10 || dim > 30) FAIL("reference file %s: dict dim %d outside 10 .. 30", path, dim);
    const uint64_t tsize = 1ull << dim;
    if (dmax < 0 || (uint64_t)dmax >= tsize / 2) FAIL("reference file %s: %d names do not fit a dict of dim %d", path, dmax, dim);
    if (left < tsize * 4 + ((uint64_t)dmax + 1) * 8) FAIL("reference file %s: dict of dim %d with %d names does not fit the file", path, dim, dmax);
    if (!(r->dict = h10x_namedict_create((int)tsize))) FAIL("out of host memory for reference file %s", path);
    TAKE(r->dict->table, tsize * 4, "failed read ref dict");
    for (uint64_t i = 0; i < tsize; ++i) if (r->dict->table[i] < 0 || r->dict->table[i] > dmax) FAIL("reference file %s: dict table entry %d beyond its %d names", path, r->dict->table[i], dmax);
    if (fseeko(f, ((off_t)dmax + 1) * 8, SEEK_CUR)) FAIL("failed read ref dict");           /* the reference's heap pointers */
    left -= ((uint64_t)dmax + 1) * 8;
    for (int i = 1; i <= dmax; ++i) {
      int32_t n;
      TAKE(&n, 4, "failed read ref dict");
      if (n < 0 || (uint64_t)n > left) FAIL("reference file %s: name %d of %d bytes runs past the end of the file", path, i, n);
      if (!(r->dict->names[i] = (char *)calloc((size_t)n + 1, 1))) FAIL("out of host memory for reference file %s", path);
      r->dict->max = i;
      TAKE(r->dict->names[i], n, "failed read ref dict");
    }
    if (a.max < dmax) FAIL("reference file %s: %d lengths for %d names", path, a.max, dmax);
  }
  {
    uint32_t run = 0;
    for (uint32_t i = 0; i <= setMax; ++i) {
      if (r->loc[i] != run) FAIL("reference file %s: loc[%u] is %u, the depths before it sum to %u", path, i, r->loc[i], run);
      if (r->depth[i] > r->max - run) FAIL("reference file %s: its depths sum to more than its %u hits", path, r->max);
      if (i) run += r->depth[i];
    }
    for (uint32_t i = 0; i < r->max; ++i) {
      if (r->index[i] > setMax) FAIL("reference file %s: hit %u holds mosh index %u beyond %u", path, i, r->index[i], setMax);
      if (r->id[i] >= (uint32_t)r->dict->max) FAIL("reference file %s: hit %u is on sequence %u of %d", path, i, r->id[i], r->dict->max);
      if (r->rev[i] >= r->max) FAIL("reference file %s: rev[%u] is %u beyond its %u hits", path, i, r->rev[i], r->max);
    }
  }
  rc = 0;
out:
#undef TAKE
#undef FAIL
  fclose(f);
  if (rc) h10x_reffile_free(r);
  return rc;
}

/* the .ref half of referenceWrite (moshmap.c:141-154): the pointer fields of the reference's structures (ArrayStruct.base, the dict's
   names[]) are written as 0 */
int h10x_reffile_write(const char *path, const h10x_reffile *r, char *err, int errlen) {
  FILE *f = fopen(path, "wb");
  if (!f) return set_msg(err, errlen, "failed to open %s to write", path);
  int rc = -1;
#define PUT(ptr, size, n, what) do { if ((n) && fwrite(ptr, size, (size_t)(n), f) != (size_t)(n)) { set_msg(err, errlen, what); goto out; } } while (0)
  const uint32_t n1 = r->setMax + 1;
  ArrayHead a; memset(&a, 0, sizeof a);
  a.magic = ARRAY_MAGIC; a.dim = r->lenDim; a.size = 4; a.max = r->lenMax;
  PUT("RFMSHv1", 8, 1, "failed to write reference header");
  PUT(&r->max, 4, 1, "failed to write size");
  PUT(&r->max, 4, 1, "failed to write max");
  PUT(r->index, 4, r->max, "failed write ref index");
  PUT(r->offset, 4, r->max, "failed write ref offset");
  PUT(r->id, 4, r->max, "failed write ref id");
  PUT(r->depth, 4, n1, "fail depth");
  PUT(r->rev, 4, r->max, "fail rev");
  PUT(r->loc, 4, n1, "fail loc");
  PUT(&a, sizeof a, 1, "failed write ref len");
  PUT(r->len, 4, r->lenDim, "failed write ref len");
  PUT(&r->dict->dim, 4, 1, "failed write ref dict");
  PUT(&r->dict->max, 4, 1, "failed write ref dict");
  PUT(r->dict->table, 4, r->dict->size, "failed write ref dict");
  for (int i = 0; i <= r->dict->max; ++i) { const uint64_t zero = 0; PUT(&zero, 8, 1, "failed write ref dict"); }
  for (int i = 1; i <= r->dict->max; ++i) {
    const int32_t n = (int32_t)strlen(r->dict->names[i]);
    PUT(&n, 4, 1, "failed write ref dict");
    PUT(r->dict->names[i], 1, n, "failed write ref dict");
  }
  rc = 0;
out:
#undef PUT
  if (fclose(f) && !rc) rc = set_msg(err, errlen, "failed to write reference file %s", path);
  return rc;
}

/* array(ref->len, id, int) = len (moshmap.c:102) with arrayExtend's growth (array.c:144-170) */
int h10x_reffile_set_len(h10x_reffile *r, uint32_t id, uint32_t len) {
  if (!r->len) { r->lenDim = 1024; if (!(r->len = (uint32_t *)calloc(1024, 4))) return -1; }
  if ((int64_t)id >= r->lenDim) {
    int64_t dim = r->lenDim;
    if (dim * 4 < (1 << 23)) dim *= 2; else dim += 1024 + ((1 << 23) / 4);
    if ((int64_t)id >= dim) dim = (int64_t)id + 1;
    if (dim > 0x7fffffff) return -1;
    uint32_t *p = (uint32_t *)calloc((size_t)dim, 4);
    if (!p) return -1;
    memcpy(p, r->len, (size_t)r->lenMax * 4);
    free(r->len); r->len = p; r->lenDim = (int32_t)dim;
  }
  if ((int32_t)id >= r->lenMax) r->lenMax = (int32_t)id + 1;
  r->len[id] = len;
  return 0;
}

/* ------------------------------------------------------------------------------------------------ texts */
void h10x_map_print_q(FILE *f, const char *name, int len, const uint32_t c[4]) {              /* moshmap.c:207-209 */
  const int missed = (int)c[0], n = (int)(c[0] + c[1] + c[2] + c[3]);
  fprintf(f, "Q\t%s\t%d\t%d miss, %d copy1, %d copy2, %d multi, %.2f hit\n", name, len, missed, (int)c[1], (int)c[2], (int)c[3], (n - missed) / (double)n);
}
void h10x_map_print_m(FILE *f, const char *name, int len, const h10x_maprec_t *m, const char *refName, uint32_t off0, uint32_t offN, uint32_t copy1) {   /* moshmap.c:255-260 */
  const int n1 = (int)m->n1, n2 = (int)m->n2;
  fprintf(f, "M\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d %d\t%.2f\t%.2f\n", name, (int)m->pos0, (int)m->posN, len, refName, (int)off0, (int)offN, n1, n2,
          (n1 + n2) / (double)(m->locN > m->loc0 ? m->locN - m->loc0 : m->loc0 - m->locN), n1 / (double)(int)copy1);
}
void h10x_map_print_seed(FILE *f, uint32_t pos, int class, const char *name1, uint32_t off1, const char *name2, uint32_t off2) {   /* moshmap.c:219-229 */
  if (class == 1) fprintf(f, "  %6d\t%s %d\n", (int)pos, name1, (int)off1);
  else fprintf(f, "  %6d\t%s %d\t%s %d\n", (int)pos, name1, (int)off1, name2, (int)off2);
}

/* ------------------------------------------------------------------------------------------------ commands over a device map */
#ifndef H10X_MAP_NO_DEVICE                                   /* (the sanitizer driver links what is above this line, and nothing of the device) */
void h10x_mapref_destroy(h10x_mapref *r) {
  if (!r) return;
  if (r->rm) h10x_refmap_destroy(r->rm);
  free(r->len);
  h10x_namedict_destroy(r->dict);
  free(r);
}

/* referenceFastaRead (moshmap.c:92-133) after referenceCreate: 0 = done, -1 = fatal (msg). A sequence without bases ends the file, as
   readSequence's return value does (readseq.c:157, moshmap.c:99). */
int h10x_mapref_from_fasta(h10x_mapref **out, h10x_mosh *set, uint32_t size, const char *path, uint64_t slabBases, FILE *outFile, char *msg, int msglen) {
  *out = 0;
  h10x_mapref *r = (h10x_mapref *)calloc(1, sizeof *r);
  if (!r) return set_msg(msg, msglen, "out of host memory");
  int rc = -1, fatal = 0; h10x_seqreader *rd = 0; h10x_reffile lens; memset(&lens, 0, sizeof lens);
#define FAIL(...) do { set_msg(msg, msglen, __VA_ARGS__); goto out; } while (0)
  if (h10x_refmap_create(&r->rm, set, size)) FAIL("%s", h10x_mosh_error(set));
  if (!(r->dict = h10x_namedict_create(1024))) FAIL("out of host memory");
  if (h10x_reffile_set_len(&lens, 0, 0)) FAIL("out of host memory");
  lens.lenMax = 0;
  rd = h10x_seq_open(path, msg, msglen, &fatal);
  if (!rd && fatal) goto out;
  uint64_t totLen = 0; int stop = 0;
  while (rd && !stop) {
    const uint8_t *codes; const uint64_t *start, *nameOff; const char *names; uint32_t nSeq;
    const int nrc = h10x_seq_next_named(rd, slabBases, &codes, &start, &nSeq, &names, &nameOff);
    if (nrc < 0) FAIL("%s", h10x_seq_error(rd));
    if (nrc == 0) break;
    const uint32_t idBase = (uint32_t)r->dict->max;
    for (uint32_t s = 0; s < nSeq; ++s) {
      if (start[s + 1] == start[s]) { nSeq = s; stop = 1; break; }
      int id;
      const int arc = h10x_namedict_add(r->dict, names + nameOff[s], &id);
      if (arc < 0) FAIL("out of host memory");
      if (!arc) FAIL("duplicate ref sequence name %s", names + nameOff[s]);
      if (h10x_reffile_set_len(&lens, (uint32_t)id, (uint32_t)(start[s + 1] - start[s]))) FAIL("out of host memory");
      totLen += start[s + 1] - start[s];
    }
    if (nSeq && h10x_refmap_add(r->rm, codes, start, nSeq, idBase, 0)) FAIL("%s", h10x_refmap_error(r->rm));
  }
  r->len = lens.len; r->lenDim = lens.lenDim; r->lenMax = lens.lenMax; lens.len = 0;
  h10x_refmap_info_t in; h10x_refmap_info(r->rm, &in);
  fprintf(outFile, "  %d hashes from %d reference sequences, total length %lld\n", (int)in.max, r->dict->max, (long long)totLen);
  uint32_t n1, n2, nM;
  if (h10x_refmap_pack(r->rm, &n1, &n2, &nM)) FAIL("%s", h10x_refmap_error(r->rm));
  fprintf(outFile, "  %d copy 1, %d copy 2, %d multiple\n", (int)n1, (int)n2, (int)nM);
  rc = 0;
out:
#undef FAIL
  free(lens.len);
  if (rd) h10x_seq_close(rd);
  if (rc) h10x_mapref_destroy(r); else *out = r;
  return rc;
}

/* the device half of referenceRead: takes the names and lengths out of the parsed file */
int h10x_mapref_from_file(h10x_mapref **out, h10x_mosh *set, h10x_reffile *rf, char *msg, int msglen) {
  *out = 0;
  h10x_mapref *r = (h10x_mapref *)calloc(1, sizeof *r);
  if (!r) return set_msg(msg, msglen, "out of host memory");
  if (h10x_refmap_load(&r->rm, set, rf->index, rf->offset, rf->id, rf->depth, rf->rev, rf->loc, rf->max, (uint32_t)rf->dict->max)) {
    free(r);
    return set_msg(msg, msglen, "%s", h10x_mosh_error(set));
  }
  r->dict = rf->dict; r->len = rf->len; r->lenDim = rf->lenDim; r->lenMax = rf->lenMax;
  rf->dict = 0; rf->len = 0;
  *out = r;
  return 0;
}

int h10x_mapref_write_file(h10x_mapref *r, const char *path, char *err, int errlen) {
  h10x_reffile rf; h10x_refmap_info_t in; memset(&rf, 0, sizeof rf);
  if (h10x_refmap_info(r->rm, &in) ||
      h10x_refmap_export(r->rm, (const uint32_t **)&rf.index, (const uint32_t **)&rf.offset, (const uint32_t **)&rf.id, (const uint32_t **)&rf.depth,
                         (const uint32_t **)&rf.rev, (const uint32_t **)&rf.loc))
    return set_msg(err, errlen, "%s", h10x_refmap_error(r->rm));
  rf.max = in.max; rf.setMax = in.setMax; rf.len = r->len; rf.lenDim = r->lenDim; rf.lenMax = r->lenMax; rf.dict = r->dict;
  return h10x_reffile_write(path, &rf, err, errlen);
}

/* queryProcess (moshmap.c:187-278) over a file: the Q and M lines to f, the -v lines to fverbose (stdout in the program, moshmap.c:221),
   in the reference's order: an M line follows the verbose line of the seed that ended its block */
int h10x_mapref_query_file(h10x_mapref *r, const char *path, uint64_t slabBases, int verbose, FILE *f, FILE *fverbose, char *msg, int msglen) {
  int fatal = 0, rc = -1, stop = 0;
  h10x_seqreader *rd = h10x_seq_open(path, msg, msglen, &fatal);
  if (!rd) return fatal ? -1 : 0;                            /* an empty file holds no query */
  const uint32_t *offset, *id;
  if (h10x_refmap_export(r->rm, 0, &offset, &id, 0, 0, 0)) { set_msg(msg, msglen, "%s", h10x_refmap_error(r->rm)); goto out; }
  while (!stop) {
    const uint8_t *codes; const uint64_t *start, *nameOff; const char *names; uint32_t nSeq, nq;
    const int nrc = h10x_seq_next_named(rd, slabBases, &codes, &start, &nSeq, &names, &nameOff);
    if (nrc < 0) { set_msg(msg, msglen, "%s", h10x_seq_error(rd)); goto out; }
    if (nrc == 0) break;
    for (uint32_t s = 0; s < nSeq; ++s) if (start[s + 1] == start[s]) { nSeq = s; stop = 1; break; }
    if (!nSeq) break;
    const uint32_t *counts, *seedPos; const uint64_t *recStart, *seedStart; const h10x_maprec_t *recs; const h10x_mapseed_t *seeds;
    if (h10x_refmap_query(r->rm, codes, start, nSeq, verbose) || h10x_refmap_results(r->rm, &nq, &counts, &recStart, &recs, &seedStart, &seeds, &seedPos)) {
      set_msg(msg, msglen, "%s", h10x_refmap_error(r->rm)); goto out;
    }
    for (uint32_t q = 0; q < nSeq; ++q) {
      const char *name = names + nameOff[q]; const int len = (int)(start[q + 1] - start[q]);
      h10x_map_print_q(f, name, len, counts + 4 * (size_t)q);
      uint64_t k = recStart[q];
#define PRINT_M(rec) h10x_map_print_m(f, name, len, rec, h10x_namedict_name(r->dict, id[(rec)->loc0]), offset[(rec)->loc0], offset[(rec)->locN], counts[4 * (size_t)q + 1])
      if (verbose)
        for (uint64_t p = seedStart[q]; p < seedStart[q + 1]; ++p) {
          const int class = (int)(seeds[p].idClass >> 30);
          if (class != 1 && class != 2) continue;
          h10x_map_print_seed(fverbose, seedPos[p], class, h10x_namedict_name(r->dict, seeds[p].idClass & 0x3fffffffu), offset[seeds[p].loc],
                              class == 2 ? h10x_namedict_name(r->dict, seeds[p].id2) : "", class == 2 ? offset[seeds[p].loc2] : 0);
          if (k < recStart[q + 1] && seedPos[p] > recs[k].posN) { PRINT_M(&recs[k]); ++k; }      /* this seed ended the block of record k */
        }
      for (; k < recStart[q + 1]; ++k) PRINT_M(&recs[k]);
#undef PRINT_M
    }
  }
  rc = 0;
out:
  h10x_seq_close(rd);
  return rc;
}
#endif
