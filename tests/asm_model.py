"""A plain Python model of the reference's moshasm (moshasm.c) on top of mosh_model.py: the readset of long reads as lists of
mosh hits, its inverse index, findOverlaps with the order glibc's stable qsort gives, markBadReads, markContained, the reports,
the RSMSHv2 file and the command loop. Pinned to the reference byte for byte by the fixtures of tests/golden/asm
(tests/test_moshasm_cpu.py)."""
import gzip
import hashlib
import json
import math
import os
import struct

import numpy as np

import mosh_model as mm
import orc
from mosh_model import ModelDie

TOPBIT, TOPMASK, U16MAX = 0x80000000, 0x7FFFFFFF, 65535
ARRAY_MAGIC = 8918274
READ_SIZE = 72
BAD_REPEAT, BAD_ORDER10, BAD_ORDER1, BAD_NOMATCH, BAD_LOWHIT, BAD_LOWCOPY1 = 1, 2, 4, 8, 16, 32
MAX_HITS = 65534


def fdiv(a, b):
    """a / (double) b as C gives it, as text pieces for %.Nf: 0/0 is the x86 default NaN, which prints as -nan"""
    if b:
        return a / float(b)
    return float("inf") if a > 0 else float("-nan") if a == 0 else float("-inf")


def ffmt(v, nd):
    if v != v:
        return "-nan"
    return "%.*f" % (nd, v)


class Read:
    __slots__ = ("len", "hit", "dx", "bad", "other", "pad1", "nMiss", "contained", "nCopy", "pad2")

    def __init__(self):
        self.len = 0; self.hit = []; self.dx = []; self.bad = 0; self.other = 0; self.pad1 = 0; self.nMiss = 0; self.contained = 0
        self.nCopy = [0, 0, 0, 0]; self.pad2 = (0, 0, 0, 0)

    @property
    def nHit(self):
        return len(self.hit)


def grow_dim(dim, n):
    """arrayExtend (array.c:144-170) for 72-byte elements: called with index n >= dim"""
    if dim * READ_SIZE < 1 << 23:
        dim *= 2
    else:
        dim += 1024 + ((1 << 23) // READ_SIZE)
    if n >= dim:
        dim = n + 1
    return dim


class ReadsetModel:
    def __init__(self, ms, dim=1 << 16):
        self.ms = ms
        self.reads = [Read()]                                   # read 0 is burned
        self.dim = dim
        self.totHit = 0
        self.inv = {}

    # ---- readsetFileRead (moshasm.c:125-165)
    def add(self, seqs):
        ms = self.ms
        ms.depth = [0] * len(ms.depth)
        k = ms.k
        shift1 = 64 - 2 * k
        M64 = (1 << 64) - 1
        for s in seqs:
            r = Read()
            r.len = len(s)
            n = len(self.reads)
            if n >= self.dim:
                self.dim = grow_dim(self.dim, n)
            self.reads.append(r)
            hs, ps = ms.moshes(s)
            last = 0
            for h, p in zip(hs.tolist(), ps.tolist()):
                i = ms.ix.get(h, 0)
                if not i:
                    r.nMiss += 1
                    continue
                f = 0
                for c in s[p:p + k].tolist():
                    f = (f << 2) | c
                fwd = ((f * ms.factor1) & M64) >> shift1 == h
                if fwd:                                           # a tie is reverse (seqhash.c:67)
                    rc = 0
                    for c in s[p:p + k].tolist()[::-1]:
                        rc = (rc << 2) | (3 - c)
                    fwd = ((rc * ms.factor1) & M64) >> shift1 != h
                r.hit.append(i | TOPBIT if fwd else i)
                r.dx.append((p - last) & 0xFFFF)
                last = p
                ms.depth[i] = min(U16MAX, ms.depth[i] + 1)
            if r.nHit > MAX_HITS:
                raise ModelDie("FATAL ERROR: read %d has %d hits: more than %d are not supported" % (n, r.nHit, MAX_HITS))
            self.totHit += r.nHit
        self.inv_build()

    # ---- invBuild (moshasm.c:232-260)
    def inv_build(self):
        ms = self.ms
        self.inv = {}
        for i, r in enumerate(self.reads):
            if not i:
                continue
            r.nCopy = [0, 0, 0, 0]
            for h in r.hit:
                y = h & TOPMASK
                r.nCopy[ms.info[y] & 3] += 1
                if ms.depth[y] < U16MAX:
                    self.inv.setdefault(y, []).append(i)
        for y, lst in self.inv.items():
            if len(lst) != ms.depth[y]:
                raise ModelDie("FATAL ERROR: the readset does not match the depths of its mosh set")

    # ---- the RSMSHv2 file (moshasm.c:84-123, array.c:213-218)
    def to_bytes(self):
        out = [b"RSMSHv2\0", struct.pack("<Q", self.totHit), struct.pack("<iiQiiii", ARRAY_MAGIC, 0, 0, self.dim, READ_SIZE, len(self.reads), 0)]
        for r in self.reads:
            out.append(struct.pack("<iiQQBBHii4i4Ii", r.len, r.nHit, 0, 0, r.bad, r.other, r.pad1, r.nMiss, r.contained, *r.nCopy, *r.pad2, 0))
        out.append(b"\0" * (READ_SIZE * (self.dim - len(self.reads))))
        for r in self.reads:
            if r.nHit:
                out.append(np.array(r.hit, "<u4").tobytes() + np.array(r.dx, "<u2").tobytes())
        return b"".join(out)

    @classmethod
    def from_bytes(cls, ms, data):
        if len(data) < 8:
            raise ModelDie("FATAL ERROR: failed to read readset header")
        if data[:8] != b"RSMSHv2\0":
            raise ModelDie("FATAL ERROR: bad readset header %s != RSMSHv2" % data[:8].split(b"\0")[0].decode(errors="replace"))
        if len(data) < 16:
            raise ModelDie("FATAL ERROR: failed to read totHit")
        rs = cls(ms)
        rs.totHit = struct.unpack_from("<Q", data, 8)[0]
        if len(data) < 48:
            raise ModelDie("FATAL ERROR: failed to read the reads array")
        magic, _, _, dim, size, mx, _ = struct.unpack_from("<iiQiiii", data, 16)
        if size != READ_SIZE:
            raise ModelDie("FATAL ERROR: readset record size %d != %d" % (size, READ_SIZE))
        if mx < 1 or mx > dim:
            raise ModelDie("FATAL ERROR: readset max %d outside 1 .. dim %d" % (mx, dim))
        if len(data) < 48 + READ_SIZE * dim:
            raise ModelDie("FATAL ERROR: failed to read the reads array")
        rs.dim = dim
        rs.reads = []
        off = 48 + READ_SIZE * dim
        nh = []
        for i in range(mx):
            f = struct.unpack_from("<iiQQBBHii4i4I", data, 48 + READ_SIZE * i)
            r = Read()
            r.len, n, _, _, r.bad, r.other, r.pad1, r.nMiss, r.contained = f[:9]
            r.nCopy = list(f[9:13]); r.pad2 = tuple(f[13:17])
            if n < 0 or n > MAX_HITS:
                raise ModelDie("FATAL ERROR: read %d has %d hits: more than %d are not supported" % (i, n, MAX_HITS))
            nh.append(n)
            rs.reads.append(r)
        if sum(nh) != rs.totHit:
            raise ModelDie("FATAL ERROR: readset totHit %d but the reads hold %d hits" % (rs.totHit, sum(nh)))
        for i, r in enumerate(rs.reads):
            n = nh[i]
            if n:
                if len(data) < off + 4 * n:
                    raise ModelDie("FATAL ERROR: failed read hits")
                r.hit = np.frombuffer(data, "<u4", n, off).tolist()
                off += 4 * n
                if len(data) < off + 2 * n:
                    raise ModelDie("FATAL ERROR: failed read dx")
                r.dx = np.frombuffer(data, "<u2", n, off).tolist()
                off += 2 * n
                top = max(h & TOPMASK for h in r.hit)
                if top > ms.max or min(h & TOPMASK for h in r.hit) == 0:
                    raise ModelDie("FATAL ERROR: read %d holds mosh index %d outside 1 .. %d" % (i, top if top > ms.max else 0, ms.max))
        rs.inv_build()
        return rs

    # ---- findOverlaps (moshasm.c:286-384); returns the Overlap array as lists [iy, nHit, offset, isPlus, isBad]
    def find_overlaps(self, ix, report, emit):
        ms, x = self.ms, self.reads[ix]
        hmap, cand, nRepeat = {}, {}, 0
        xPos = [0]
        for j, h in enumerate(x.hit):
            hxx = h & TOPMASK
            xPos.append((xPos[-1] + x.dx[j]) & 0xFFFFFFFF)
            if (ms.info[hxx] & 3) == 1:
                if hxx in hmap:
                    nRepeat += 1
                    x.bad |= BAD_REPEAT
                    continue
                hmap[hxx] = j + 1
                if ms.depth[hxx] >= U16MAX:
                    raise ModelDie("FATAL ERROR: copy-1 mosh %x has depth 65535: it has no inverse list" % ms.value[hxx])
                for r in self.inv.get(hxx, ()):
                    cand[r] = cand.get(r, 0) + 1
        olap = [[0, 0, 0, 0, 0]] + [[iy, n, 0, 0, 0] for iy, n in cand.items()]
        olap.sort(key=lambda o: -o[1])                          # stable, as glibc's merge sort is
        nGood = nBad = 0
        k = 1
        while k < len(olap):
            o = olap[k - 1]
            if o[1] < 3:
                break
            k += 1
            y = self.reads[o[0]]
            if y.bad:
                continue
            nPlus = nMinus = 0
            for h in y.hit:
                i = hmap.get(h & TOPMASK, 0)
                if i:
                    if (h & TOPBIT) == (x.hit[i - 1] & TOPBIT):
                        nPlus += 1
                    else:
                        nMinus += 1
            d = d2 = 0.0
            yPos = 0.0
            if nPlus and not nMinus:
                o[3] = 1
                last = 0
                for j, h in enumerate(y.hit):
                    yPos += y.dx[j]
                    i = hmap.get(h & TOPMASK, 0)
                    if i:
                        if i < last:
                            o[4] = 1; nPlus -= 1
                        last = i
                        z = xPos[i] - yPos; d += z; d2 += z * z
            elif nMinus and not nPlus:
                last = x.nHit
                for j, h in enumerate(y.hit):
                    yPos += y.dx[j]
                    i = hmap.get(h & TOPMASK, 0)
                    if i:
                        if i > last:
                            o[4] = 1; nMinus -= 1
                        last = i
                        z = xPos[i] + yPos; d += z; d2 += z * z
            if nPlus and nMinus:
                o[4] = 1
            d /= o[1]
            v = d2 / o[1] - d * d
            d2 = math.sqrt(v) if v >= 0 else float("nan")
            o[2] = int(d)
            if o[4]:
                nBad += 1
            else:
                nGood += 1
            if report > 1:
                emit("RH\t%u\tlen %d\t%s\tnPlus %d\tnMinus %d\toffset %s\tsd %s\n" % (o[0], y.len, "BAD" if o[4] else "GOOD", nPlus, nMinus, ffmt(d, 1), ffmt(d2, 1)))
        del olap[k:]
        if not nGood and not nBad:
            x.bad |= BAD_NOMATCH
            if x.nHit < 10:
                x.bad |= BAD_LOWHIT
            elif x.nCopy[1] < 10:
                x.bad |= BAD_LOWCOPY1
        if report > 0:
            emit("RR %6u\tlen %d\tnHit %3d\tnMiss %3d\tnCpy %d %d %d %d\tnRepeatMosh %d\tnGood %4d\tnBad %4d\n" % (
                ix, x.len, x.nHit, x.nMiss, x.nCopy[0], x.nCopy[1], x.nCopy[2], x.nCopy[3], nRepeat, nGood, nBad))
        return olap

    def bad_overlaps(self, ix):
        return sum(o[4] for o in self.find_overlaps(ix, 0, None))

    # ---- markBadReads (moshasm.c:436-461): the MB lines go to stdout
    def mark_bad(self):
        lines = []
        for r in self.reads:
            r.bad = 0
        n = 0
        for ix, x in enumerate(self.reads):
            if self.bad_overlaps(ix) >= 10:
                x.bad |= BAD_ORDER10; n += 1
        lines.append("MB  %d with >=10 bad overlaps\n" % n)
        n = 0
        for ix, x in enumerate(self.reads):
            if self.bad_overlaps(ix) > 1 and not x.bad & BAD_ORDER10:
                x.bad |= BAD_ORDER1; n += 1
        lines.append("MB  %d with multiple bad overlaps\n" % n)
        n = 0
        for ix, x in enumerate(self.reads):
            if self.bad_overlaps(ix) > 0 and not x.bad & BAD_ORDER10:
                x.bad |= BAD_ORDER1; n += 1
        lines.append("MB  %d with single bad overlaps\n" % n)
        return "".join(lines)

    # ---- markContained (moshasm.c:471-497); ties = reads whose choice a tie in nHit decided (for the fixture conditions)
    def mark_contained(self):
        nC = nN = tot = 0
        self.ties = 0
        for ix, x in enumerate(self.reads):
            if x.bad:
                continue
            maxHit, tie = 0, False
            for iy, nHit, offset, isPlus, _ in self.find_overlaps(ix, 0, None):
                y = self.reads[iy]
                if iy == ix or y.len < x.len:
                    continue
                ok = not ((isPlus and (offset > 0 or offset + y.len < x.len)) or (not isPlus and (offset < x.len or offset - y.len > 0)))
                if nHit <= maxHit:
                    tie = tie or (ok and nHit == maxHit)
                    continue
                if not ok:
                    continue
                x.contained = iy; maxHit = nHit
            self.ties += tie
            if x.contained:
                nC += 1
            else:
                nN += 1; tot += x.len
        return "MC  found %d contained reads, leaving %d not contained, av length %.1f\n" % (nC, nN, tot / float(nN) if nN else 0.)

    # ---- readsetStats (moshasm.c:167-230)
    def stats(self, emit, err):
        n = len(self.reads) - 1
        if not n:
            err("stats called on empty readset\n")
            return
        ms = self.ms
        emit(ms.summary())
        totLen = totMiss = len0 = len1 = n0 = n1 = 0
        totCopy = [0] * 4
        nb = [0] * 7
        for r in self.reads[1:]:
            totLen += r.len; totMiss += r.nMiss
            for j in range(4):
                totCopy[j] += r.nCopy[j]
            if r.nCopy[1] == 0:
                n0 += 1; len0 += r.len
            elif r.nCopy[1] == 1:
                n1 += 1; len1 += r.len
            if r.bad:
                nb[0] += 1
                for b in range(6):
                    nb[b + 1] += (r.bad >> b) & 1
        th = self.totHit
        emit("RS %d sequences, total length %d (av %s)\n" % (n, totLen, ffmt(fdiv(totLen, n), 1)))
        emit("RS %d mosh hits, %s bp/hit, frac hit %s, av hits/read %s\n" % (th, ffmt(fdiv(totLen, th), 1), ffmt(fdiv(th, totMiss + th), 2), ffmt(fdiv(th, n), 1)))
        emit("RS hit distribution %s copy0, %s copy1, %s copy2, %s copyM\n" % tuple(ffmt(fdiv(totCopy[j], th), 2) for j in range(4)))
        nm = (n - n0 - n1) & 0xFFFFFFFF
        emit("RS num reads and av_len with 0 copy1 hits %d %s with 1 copy1 hits %d %s >1 copy1 hits %d %s av copy1 hits %s\n" % (
            n0, ffmt(fdiv(len0, n0), 1), n1, ffmt(fdiv(len1, n1), 1), nm & 0x7FFFFFFF if nm < 2 ** 31 else nm - 2 ** 32,
            ffmt(fdiv(totLen - len0 - len1, nm), 1), ffmt(fdiv(totCopy[1] - n1, nm), 1)))
        emit("RS bad %u : %u repeat, %u order10, %u order1, %u no_match, %u low_hit, %u low_copy1\n" % tuple(nb))
        nc, hc, h2, dc = [0] * 4, [0] * 4, [0] * 4, [0] * 4
        for i in range(1, ms.max + 1):
            j = ms.info[i] & 3
            nc[j] += 1
            if ms.depth[i] > 0:
                hc[j] += 1
            if ms.depth[i] > 1:
                h2[j] += 1; dc[j] += ms.depth[i]
        parts = []
        for j, nm_ in enumerate(("copy0", "copy1", "copy2", "copyM")):
            parts.append("%s %s %s %s" % (nm_, ffmt(fdiv(hc[j], nc[j]), 3), ffmt(fdiv(h2[j], nc[j]), 3), ffmt(fdiv(dc[j], h2[j]), 1)))
        emit("RS mosh frac hit hit>1 av: " + " ".join(parts) + "\n")

    # ---- printOverlap (moshasm.c:386-416), yPos += y->dx[0] as written
    def print_overlap(self, ix, iy, emit):
        ms = self.ms
        for i in (ix, iy):
            r = self.reads[i]
            emit("RR overlaps_for %u\tlen %d\tnHit %d\tnMiss %d\tnCopy %d %d %d %d\n" % (i, r.len, r.nHit, r.nMiss, *r.nCopy))
        x, y = self.reads[ix], self.reads[iy]
        xPos = 0
        for j in range(x.nHit):
            hx = x.hit[0]                                        # hx is never advanced in the reference: every turn looks at x's first hit
            hxx = hx & TOPMASK
            xPos += x.dx[j]
            if (ms.info[hxx] & 3) == 1:
                yPos = 0
                for hy in y.hit:
                    yPos += y.dx[0]
                    if hxx == hy & TOPMASK:
                        emit("RO\t%8x %5d %c\t%u %u %c\t%u %u %c\n" % (hxx, ms.depth[hxx], "+" if (hx & TOPBIT) == (hy & TOPBIT) else "-",
                                                                     ix, xPos, "F" if hx & TOPBIT else "R", iy, yPos, "F" if hy & TOPBIT else "R"))

    # ---- assembleFromRead's report (moshasm.c:514-579): RR to the output, AR / AH to stdout
    def assemble(self, ix, emit):
        ms = self.ms
        order, ah = {}, []                                      # hashAdd numbers keys from 1 in insertion order
        for iy, nHit, offset, isPlus, _ in self.find_overlaps(ix, 1, emit):
            y = self.reads[iy]
            yPos = 0
            for j, h in enumerate(y.hit):
                hit = h & TOPMASK
                yPos += y.dx[j]
                ih = order.get(hit)
                if ih is None:
                    ih = order[hit] = len(ah)
                    ah.append([hit, 0, 0])
                a = ah[ih]
                a[1] += 1
                a[2] += offset + yPos if isPlus else offset - yPos
        cnt = len(ah)
        A = [[0] * 20 for _ in range(20)]; Bm = [[0] * 20 for _ in range(20)]
        tot = 0.0
        for hit, c, _ in ah[:max(cnt - 1, 0)]:                  # for (ih = 1 ; ih < hashCount ; ++ih): the last one is left out
            tot += c
            if (ms.info[hit] & 3) != 1:
                continue
            i = min(c, 19)
            A[i][min(ms.depth[hit], 19)] += 1
            Bm[i][(10 * c - 1) // ms.depth[hit]] += 1
        out = ["AR  %d total hits - mean count %s\n" % (cnt, ffmt(fdiv(tot, cnt), 1))]
        for i in range(20):
            out.append("AH  %2d\t" % i + "".join("    " if j < i else "%4d" % A[i][j] for j in range(20)) + "    " + "".join("%4d" % Bm[i][j] for j in range(10)) + "\n")
        return "".join(out)


# ---- masks and the command loop (moshasm.c:602-695) -----------------------------------------------------------------------
def mask_readset(data):
    """the heap pointers the reference leaks into the file: ArrayStruct.base, Read.hit and Read.dx of every record"""
    if len(data) < 48 or data[:8] != b"RSMSHv2\0":
        return data
    b = bytearray(data)
    b[24:32] = b"\0" * 8
    dim = struct.unpack_from("<i", data, 32)[0]
    a = np.frombuffer(b, np.uint8, READ_SIZE * dim, 48).reshape(dim, READ_SIZE)
    a[:, 8:24] = 0
    return bytes(b)


def mask_file(name, data):
    if name.endswith(".mosh"):
        return mm.mask_mosh(data)
    if name.endswith(".readset"):
        return mask_readset(data)
    return "\n".join(mm.mask_lines(data)).encode()


def _atoi(s):
    import re
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group()) if m else 0


def run_commands(args, cwd):
    """returns (status, stdout text, stderr text); files are written under cwd"""
    out, err, ofile, files = [], [], [None], []
    RES = "user\t\n"

    def emit(s):
        (out if ofile[0] is None else ofile[0]).append(s)

    def path(p):
        return os.path.join(cwd, p)

    def finish(status):
        for lst, p in files:
            with open(path(p), "w") as f:
                f.write("".join(lst))
        return status, "".join(out), "".join(err)

    def need_rs(c):
        if rs is None:
            raise ModelDie("FATAL ERROR: %s needs a readset: give -f or -r first" % c)

    def read_ix(s):
        i = _atoi(s) & 0xFFFFFFFF
        if i >= len(rs.reads):
            raise ModelDie("FATAL ERROR: read %u is outside the readset of %d reads" % (i, len(rs.reads) - 1))
        return i

    ms = rs = None
    fopen = from_read = False
    a = list(args)
    try:
        while a:
            if not a[0].startswith("-"):
                raise ModelDie("FATAL ERROR: option/command %s does not start with '-': run without arguments for usage" % a[0])
            j = 1
            while j < len(a) and not a[j].startswith("-"):
                j += 1
            err.append("COMMAND " + " ".join(a[:j]) + "\n")
            c = a[0]

            def match(names, n):
                return c in names and len(a) >= n

            if match(("-t", "--threads"), 2):
                err.append("  can't set thread number - not compiled with OMP\n"); a = a[2:]
            elif match(("-v", "--verbose"), 1):
                a = a[1:]
            elif match(("-o", "--output"), 2):
                if a[1] == "-":
                    ofile[0] = None
                else:
                    try:
                        open(path(a[1]), "w").close()
                        ofile[0] = []
                        files.append((ofile[0], a[1]))
                    except OSError:
                        err.append("can't open output file %s - resetting to stdout\n" % a[1])
                        ofile[0] = None
                a = a[2:]
            elif match(("-m", "--moshset"), 2):
                try:
                    with open(path(a[1]), "rb") as f:
                        data = f.read()
                except OSError:
                    raise ModelDie("FATAL ERROR: failed to open mosh file %s" % a[1])
                ms = mm.MoshModel.from_bytes(data); rs = None; fopen = True; from_read = False
                emit(ms.summary())
                a = a[2:]
            elif match(("-f", "--seqfile"), 2):
                if ms is None:
                    err.append("** need to read a moshset before a sequence file\n")
                else:
                    if not fopen and from_read:
                        raise ModelDie("FATAL ERROR: -f after -r needs a new -m first (the reference closes a mosh file here that -r never opened)")
                    if not fopen:
                        raise ModelDie("FATAL ERROR: a second -f needs a new -m first (the reference closes the mosh file twice here)")
                    try:
                        data = mm.read_maybe_gz(path(a[1]))
                    except OSError:
                        raise ModelDie("FATAL ERROR: failed to open sequence file %s" % a[1])
                    seqs, warn = mm.parse_seq_bytes(data, a[1])
                    rs = ReadsetModel(ms)
                    rs.add(seqs)
                    err.extend(w + "\n" for w in warn)
                    fopen = False
                a = a[2:]
            elif match(("-r", "--read"), 2):
                try:
                    with open(path(a[1] + ".mosh"), "rb") as f:
                        ms = mm.MoshModel.from_bytes(f.read())
                except OSError:
                    raise ModelDie("FATAL ERROR: can't open file %s.mosh" % a[1])
                try:
                    with open(path(a[1] + ".readset"), "rb") as f:
                        data = f.read()
                except OSError:
                    raise ModelDie("FATAL ERROR: can't open file %s.readset" % a[1])
                rs = ReadsetModel.from_bytes(ms, data)
                fopen = False; from_read = True
                a = a[2:]
            elif match(("-w", "--write"), 2):
                need_rs(c)
                with open(path(a[1] + ".mosh"), "wb") as f:
                    f.write(ms.to_bytes())
                with open(path(a[1] + ".readset"), "wb") as f:
                    f.write(rs.to_bytes())
                a = a[2:]
            elif match(("-S", "--stats"), 1):
                need_rs(c)
                rs.stats(emit, err.append); a = a[1:]
            elif match(("-o1", "--overlaps1"), 2):
                need_rs(c)
                rs.find_overlaps(read_ix(a[1]), 2, emit); a = a[2:]
            elif match(("-o2", "--overlaps2"), 2):
                need_rs(c)
                d = _atoi(a[1])
                if d < 1:
                    raise ModelDie("FATAL ERROR: -o2 needs a step of at least 1")
                for ix in range(d, len(rs.reads), d):
                    rs.find_overlaps(ix, 1, emit)
                a = a[2:]
            elif match(("-o3", "--overlap"), 3):
                need_rs(c)
                rs.print_overlap(read_ix(a[1]), read_ix(a[2]), emit); a = a[3:]
            elif match(("-b", "--markBadReads"), 1):
                need_rs(c)
                out.append(rs.mark_bad()); a = a[1:]
            elif match(("-c", "--markContained"), 1):
                need_rs(c)
                out.append(rs.mark_contained()); a = a[1:]
            elif match(("-a1", "--assemble1"), 2):
                need_rs(c)
                out.append(rs.assemble(read_ix(a[1]), emit)); a = a[2:]
            else:
                raise ModelDie("FATAL ERROR: unkown command %s - run without arguments for usage" % c)
            emit(RES)
    except ModelDie as e:
        err.append(str(e) + "\n")
        return finish(255)
    emit("total resources used: " + RES)
    if ofile[0] is not None:
        out.append("total resources used: " + RES)
    return finish(0)


# ---- the golden fixtures of tests/golden/make_asm_golden.py ------------------------------------------------------------------
GOLD = os.path.join(orc.GOLDEN, "asm")
MANIFEST = os.path.join(orc.GOLDEN, "asm_manifest.json")


def manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def gold(name):
    with open(os.path.join(GOLD, name + ".gz"), "rb") as f:
        return gzip.decompress(f.read())


def stage_case(man, case, d):
    os.makedirs(d, exist_ok=True)
    for n in man["inputs"]:
        with open(os.path.join(d, n), "wb") as f:
            f.write(gold("in/" + n))
    for n in case["needs"]:
        with open(os.path.join(d, os.path.basename(n)), "wb") as f:
            f.write(gold(n.replace("/", ".")))
    return set(os.listdir(d))


def check_case(case, d, before, status, stdout, stderr):
    assert mm.mask_lines(stderr) == case["stderr"]
    assert mm.mask_lines(stdout) == case["stdout"]
    assert status == case["status"]
    made = sorted(set(os.listdir(d)) - before)
    assert made == sorted(case["outputs"]), (made, sorted(case["outputs"]))
    for n in made:
        with open(os.path.join(d, n), "rb") as f:
            got = mask_file(n, f.read())
        if hashlib.sha256(got).hexdigest() != case["outputs"][n]:
            exp = gold("%s.%s" % (case["name"], n))
            first = next((i for i in range(min(len(got), len(exp))) if got[i] != exp[i]), min(len(got), len(exp)))
            raise AssertionError("%s of case %s differs from the reference's: sizes %d / %d, first difference at byte %d" % (n, case["name"], len(got), len(exp), first))
