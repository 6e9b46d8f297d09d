"""A plain NumPy / Python model of the reference's mosh sets (moshset.c, moshutils.c, seqio.c's FASTA / FASTQ rules): set
semantics, the MSHSTv1 bytes including the probe table, the texts and the command loop. The hashes come from
orc.Oracle(k, w, seed, B).mosh(), which the existing tests pin to the reference; everything else is restated here and pinned
to the reference by the golden fixtures of tests/golden/mosh (tests/test_moshutils_cpu.py)."""
import gzip
import os
import re
import struct

import numpy as np

import orc

U16MAX = 65535


# ---- glibc random(): TYPE_3 additive feedback generator (r[i] = r[i-3] + r[i-31], output >> 1) ----------------------------
def glibc_random(seed, n):
    r = [0] * (344 + n)
    r[0] = seed if seed else 1
    for i in range(1, 31):
        hi, lo = divmod(r[i - 1] if r[i - 1] < 2 ** 31 else r[i - 1] - 2 ** 32, 127773)
        v = 16807 * lo - 2836 * hi
        r[i] = (v + 2147483647 if v < 0 else v) & 0xFFFFFFFF
    for i in range(31, 34):
        r[i] = r[i - 31]
    for i in range(34, 344 + n):
        r[i] = (r[i - 31] + r[i - 3]) & 0xFFFFFFFF
    return [r[344 + i] >> 1 for i in range(n)]


def factors(seed):
    """srandom(seed); seqhashCreate: factor1, factor2 (seqhash.c:29-31)"""
    a, b, c, d = glibc_random(seed & 0xFFFFFFFF, 4)
    return ((a << 32) | b | 1) & (2 ** 64 - 1), ((c << 32) | d | 1) & (2 ** 64 - 1)


# ---- sequence files (seqio.c:15-190 with dna2indexConv, N -> 0) -----------------------------------------------------------
_CODE = {ord(c): v for c, v in zip("ACGTNacgtn", (0, 1, 2, 3, 0, 0, 1, 2, 3, 0))}


class ModelDie(Exception):
    pass


def parse_seq_bytes(data, name="file"):
    """returns (list of uint8 code arrays, stderr lines); raises ModelDie with the die() text"""
    err = []
    if not data:
        err.append("sequence file %s unreadable or empty" % name)
        raise ModelDie("\n".join(err + ["FATAL ERROR: failed to open sequence file %s" % name]))
    if data[:1] not in (b">", b"@"):
        if data[:1] == b"B":
            raise ModelDie("FATAL ERROR: sequence file %s is in seqio's binary format, which is not supported" % name)
        err.append("sequence file %s is unknown type" % name)
        raise ModelDie("\n".join(err + ["FATAL ERROR: failed to open sequence file %s" % name]))
    fasta = data[:1] == b">"
    seqs, pos, line, n = [], 0, 1, len(data)

    def to_newline(p):          # index of the next '\n' at or after p, or -1 when the file ends first (bufAdvanceInRecord)
        q = data.find(b"\n", p)
        return q

    while pos < n:
        if fasta:
            if data[pos:pos + 1] != b">":
                raise ModelDie("FATAL ERROR: no initial > for FASTA record line %d" % line)
            q = to_newline(pos)
            if q < 0 or q + 1 >= n:
                err.append("incomplete sequence record line %d" % (line if q < 0 else line + 1))
                break
            line += 1
            pos = q + 1
            chunks, bad = [], False
            while pos < n and data[pos:pos + 1] != b">":
                q = to_newline(pos)
                if q < 0:
                    bad = True
                    break
                chunks.append(data[pos:q])
                line += 1
                pos = q + 1
            if bad:
                err.append("incomplete sequence record line %d" % line)
                break
            raw = b"".join(chunks)
            hi = [c for c in raw if c >= 0x80]
            if hi:
                raise ModelDie("FATAL ERROR: bad base 0x%02x in FASTA" % hi[0])
            seqs.append(np.array([_CODE[c] for c in raw if c in _CODE], dtype=np.uint8))
        else:
            if data[pos:pos + 1] != b"@":
                raise ModelDie("FATAL ERROR: no initial @ for FASTQ record line %d" % line)
            q = to_newline(pos)
            if q < 0 or q + 1 >= n:
                err.append("incomplete sequence record line %d" % (line if q < 0 else line + 1))
                break
            line += 1
            s0 = q + 1
            q = to_newline(s0)
            seq = data[s0:q] if q >= 0 else data[s0:]
            for c in seq:
                if c not in _CODE:
                    raise ModelDie("FATAL ERROR: bad base 0x%02x in FASTQ line %d" % (c, line))
            if q < 0 or q + 1 >= n:
                err.append("incomplete sequence record line %d" % (line if q < 0 else line + 1))
                break
            line += 1
            p0 = q + 1
            if data[p0:p0 + 1] != b"+":
                raise ModelDie("FATAL ERROR: missing + FASTQ line %d" % line)
            q = to_newline(p0)
            if q < 0 or q + 1 >= n:
                err.append("incomplete sequence record line %d" % (line if q < 0 else line + 1))
                break
            line += 1
            q0 = q + 1
            q = to_newline(q0)
            if q < 0:
                err.append("incomplete sequence record line %d" % line)
                break
            if q - q0 != len(seq):
                raise ModelDie("FATAL ERROR: qual not same length as seq line %d" % line)
            line += 1
            pos = q + 1
            seqs.append(np.array([_CODE[c] for c in seq], dtype=np.uint8))
    return seqs, err


def read_maybe_gz(path):
    with open(path, "rb") as f:
        data = f.read()
    return gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data


def flatten(seqs):
    start = np.zeros(len(seqs) + 1, np.uint64)
    if seqs:
        start[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)), start


# ---- the set ----------------------------------------------------------------------------------------------------------
class MoshModel:
    def __init__(self, B=28, k=19, w=31, seed=17, _empty=False):
        self.B, self.k, self.w = B, k, w
        if not _empty:
            if not 1 <= k < 32:
                raise ModelDie("FATAL ERROR: seqhash k %d must be between 1 and 32\n" % k)
            self.factor1, self.factor2 = factors(seed)
            self.seed = seed
            self.size = (1 << B >> 2) - 1
        self.value, self.depth, self.info = [0], [0], [0]
        self.ix = {}
        self._orc = None

    @property
    def max(self):
        return len(self.value) - 1

    @classmethod
    def from_bytes(cls, data):
        """moshsetRead: the set is FULL (size = max + 1)"""
        if len(data) < 8:
            raise ModelDie("FATAL ERROR: failed to read moshset header")
        if data[:8] != b"MSHSTv1\0":
            raise ModelDie("FATAL ERROR: bad reference header")
        B, size = struct.unpack_from("<iI", data, 8)
        assert data[16:24] == b"SQHSHv1\0"
        k, w, mask, s1, s2, f1, f2 = struct.unpack_from("<iiQiiQQ", data, 24)
        m = cls(B, k, w, _empty=True)
        m.factor1, m.factor2, m.seed, m.size = f1, f2, None, size
        off = 96 + 4 * (1 << B)
        m.value = [int(x) for x in np.frombuffer(data, "<u8", size, off)]
        m.depth = [int(x) for x in np.frombuffer(data, "<u2", size, off + 8 * size)]
        m.info = [int(x) for x in np.frombuffer(data, "u1", size, off + 10 * size)]
        assert len(data) == off + 11 * size
        m.ix = {v: i for i, v in enumerate(m.value) if i}
        m.file_index = np.frombuffer(data, "<u4", 1 << B, 96)
        return m

    def _find_add(self, h):
        i = self.ix.get(h)
        if i is None:
            i = len(self.value)
            if i >= self.size:
                raise ModelDie("FATAL ERROR: hashTableSize %d is too small for %d" % (self.size, i))
            self.ix[h] = i
            self.value.append(h); self.depth.append(0); self.info.append(0)
        return i

    def moshes(self, seq):
        if self._orc is None:
            if self.seed is None:                            # a set from a file: the oracle hashes by seed, the file holds factor1
                self.seed = next((sd for sd in range(1, 65) if factors(sd)[0] == self.factor1), None)
            assert self.seed is not None, "hashing needs the seed: no seed 1..64 gives this file's factor1"
            self._orc = orc.Oracle(self.k, self.w, self.seed, 20)
            assert orc.lib().orc_factor1_from_seed(self.seed) == self.factor1
        return self._orc.mosh(seq)

    def add(self, seqs, is10x=False, seq_base=0):
        """addSequenceFile's loop (moshutils.c:41-45); returns (nSeq, totLen, totHash)"""
        tot = nh = 0
        for n, s in enumerate(seqs):
            tot += len(s)
            if is10x and ((seq_base + n + 1) & 1):
                if len(s) < 23:
                    raise ModelDie("FATAL ERROR: 10x sequence %d has %d bases: the first read of a pair needs at least 23" % (seq_base + n + 1, len(s)))
                s = s[23:]
            hs, _ = self.moshes(s)
            for h in hs:
                i = self._find_add(int(h))
                self.depth[i] = min(U16MAX, self.depth[i] + 1)
            nh += len(hs)
        return len(seqs), tot, nh

    def merge(self, o):
        if (self.k, self.w, self.factor1) != (o.k, o.w, o.factor1):
            return False
        for i in range(1, o.max + 1):
            j = self._find_add(o.value[i])
            self.depth[j] = min(U16MAX, self.depth[j] + o.depth[i])
            self.info[j] = (self.info[j] & 3) | min(3, (self.info[j] & 3) + (o.info[i] & 3))       # moshset.c:116-117
        return True

    def prune(self, lo, hi):
        n0 = self.max
        keep = [i for i in range(1, n0 + 1) if self.depth[i] >= lo and (not hi or self.depth[i] < hi)]
        self.value = [0] + [self.value[i] for i in keep]
        self.depth = [0] + [self.depth[i] for i in keep]
        self.info = [0] + [self.info[i] for i in keep]
        self.ix = {v: i for i, v in enumerate(self.value) if i}
        return n0, self.max

    def set_copy(self, c1, c2, cM):
        for i in range(1, self.max + 1):
            d = self.depth[i]
            if d < c1:
                self.info[i] &= 0xFC
            elif d < c2:
                self.info[i] = (self.info[i] & 0xFC) | 1
            elif d < cM:
                self.info[i] = (self.info[i] & 0xFC) | 2
            else:
                self.info[i] |= 3

    def set_copy_m(self, cM):
        for i in range(1, self.max + 1):
            if self.depth[i] >= cM:
                self.info[i] |= 3

    def table(self):
        """sequential moshsetIndexFind insertion in index order"""
        mask = (1 << self.B) - 1
        t = np.zeros(1 << self.B, np.uint32)
        for i in range(1, self.max + 1):
            h = self.value[i]
            slot, step = h & mask, ((h >> self.B) & mask) | 1
            while t[slot]:
                slot = (slot + step) & mask
            t[slot] = i
        return t

    def hist(self):
        return np.bincount(np.array(self.depth[1:], np.int64), minlength=1) if self.max else np.zeros(1, np.int64)

    def summary(self):
        s = "SH k %d  w %d\nMS table size %d number of entries %d" % (self.k, self.w, 1 << self.B, self.max)
        if not self.max:
            return s
        h = self.hist()
        tot = int(sum(i * int(c) for i, c in enumerate(h)))
        htot, n50 = tot // 2, len(h)
        for i, c in enumerate(h):
            htot -= i * int(c)
            if htot < 0:
                n50 = i
                break
        s += " total count %d\nMS average depth %.1f N50 depth %d" % (tot, tot / float(int(h.sum())), n50)
        copy = np.bincount(np.array(self.info[1:], np.int64) & 3, minlength=4)
        if copy[0] < self.max:
            s += " copy0 %d copy1 %d copy2 %d copyM %d" % tuple(int(x) for x in copy)
        return s + "\n"

    def hist_text(self):
        return "".join("DP\t%d\t%d\n" % (i, c) for i, c in enumerate(self.hist()) if c) if self.max else ""

    def depths_text(self, others=()):
        out = []
        for i in range(1, self.max + 1):
            row = "MH\t%x\t%d\t%d" % (self.value[i], self.info[i] & 3, self.depth[i])
            for o in others:
                j = o.ix.get(self.value[i])
                row += "\t%d" % (o.depth[j] if j else 0)
            out.append(row + "\n")
        return "".join(out)

    def to_bytes(self):
        k = self.k
        head = b"MSHSTv1\0" + struct.pack("<iI", self.B, self.max + 1) + b"SQHSHv1\0" + struct.pack(
            "<iiQiiQQ4Q", k, self.w, (1 << (2 * k)) - 1, 64 - 2 * k, 2 * k, self.factor1, self.factor2, *[(3 - i) << (2 * (k - 1)) for i in range(4)])
        assert len(head) == 96
        return (head + self.table().tobytes() + np.array(self.value, "<u8").tobytes() + np.array(self.depth, "<u2").tobytes() +
                np.array(self.info, "u1").tobytes())


def mask_mosh(data):
    """value[0] is uninitialised heap in a set the reference created: parity = equality after zeroing those 8 bytes"""
    B = struct.unpack_from("<i", data, 8)[0]
    off = 96 + 4 * (1 << B)
    return data[:off] + b"\0" * 8 + data[off + 8:]


def mask_lines(b):
    """text of a run with the resource figures masked"""
    return [re.sub(r"user\t.*", "user", ln) for ln in b.decode(errors="replace").splitlines()]


# ---- the command loop (moshutils.c:106-233) ---------------------------------------------------------------------------------
def run_commands(args, cwd):
    """returns (status, stdout text, stderr text); files are written under cwd"""
    out, err, ofile = [], [], [None]
    RES = "user\t\n"

    def emit(s):
        (out if ofile[0] is None else ofile[0]).append(s)

    def path(p):
        return os.path.join(cwd, p)

    def load(p):
        try:
            with open(path(p), "rb") as f:
                return MoshModel.from_bytes(f.read())
        except OSError:
            raise ModelDie("FATAL ERROR: failed to open mosh file %s" % p)

    def finish(status):
        for lst, p in files:
            with open(path(p), "w") as f:
                f.write("".join(lst))
        return status, "".join(out), "".join(err)

    files = []
    ms = None
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

            if match(("-v", "--verbose"), 1):
                a = a[1:]
            elif match(("-o", "--output"), 2):
                if a[1] == "-":
                    ofile[0] = None
                else:
                    ofile[0] = []
                    files.append((ofile[0], a[1]))
                a = a[2:]
            elif ms is None and match(("-c", "--create"), 1):
                vals, a = [28, 19, 31, 17], a[1:]
                names = ["B", "k", "w", "w"]
                for q in range(4):
                    if not a or a[0].startswith("-"):
                        break
                    m = re.match(r"\s*[+-]?\d+", a[0])
                    v = int(m.group()) if m else 0
                    if not v or (q == 0 and not 20 <= v <= 34) or (q == 1 and v < 1):
                        raise ModelDie("FATAL ERROR: bad moshbuild %s %s" % (names[q], a[0]))
                    vals[q] = v
                    a = a[1:]
                ms = MoshModel(*vals)
            elif ms is None and match(("-r", "--read"), 2):
                ms = load(a[1])
                emit("SH k %d  w %d\n" % (ms.k, ms.w))
                emit("read " + ms.summary())
                a = a[2:]
            elif ms is not None and match(("-w", "--write"), 2):
                with open(path(a[1]), "wb") as f:
                    f.write(ms.to_bytes())
                a = a[2:]
            elif ms is not None and match(("-p", "--prune"), 3):
                lo, hi = int(a[1]), int(a[2])
                n0, n1 = ms.prune(lo, hi)
                err.append("  pruned Moshset from %d to %d with min %d <= depth < max %d\n" % (n0, n1, lo, hi))
                emit("prune " + ms.summary())
                a = a[3:]
            elif ms is not None and match(("-s", "--setcopy"), 4):
                ms.set_copy(int(a[1]), int(a[2]), int(a[3]))
                emit("setcopy " + ms.summary())
                a = a[4:]
            elif ms is not None and match(("-sM", "--setcopyM"), 2):
                ms.set_copy_m(int(a[1]))
                emit("setcopyM " + ms.summary())
                a = a[2:]
            elif ms is not None and (match(("-a", "--add"), 2) or match(("-x", "--add10x"), 2)):
                is10x = c in ("-x", "--add10x")
                try:
                    data = read_maybe_gz(path(a[1]))
                except OSError:
                    raise ModelDie("FATAL ERROR: failed to open sequence file %s" % a[1])
                seqs, warn = parse_seq_bytes(data, a[1])
                err.extend(w + "\n" for w in warn)
                n, tot, nh = ms.add(seqs, is10x)
                emit("added %d sequences total length %d total hashes %d, new max %d\n" % (n, tot, nh, ms.max))
                emit(("add10x " if is10x else "add ") + ms.summary())
                a = a[2:]
            elif ms is not None and match(("-m", "--merge"), 2):
                o = load(a[1])
                emit("read " + o.summary())
                if not ms.merge(o):
                    err.append("moshset %s incompatible with current - unable to merge\n" % a[1])
                emit("merge " + ms.summary())
                a = a[2:]
            elif ms is not None and match(("-H", "--hist"), 2):
                with open(path(a[1]), "w") as f:
                    f.write(ms.hist_text())
                a = a[2:]
            elif ms is not None and match(("-d", "--depths"), 2):
                target, a, others = a[1], a[2:], []
                while a and not a[0].startswith("-"):
                    others.append(load(a[0]))
                    emit("read " + others[-1].summary())
                    a = a[1:]
                with open(path(target), "w") as f:
                    f.write(ms.depths_text(others))
            else:
                raise ModelDie("FATAL ERROR: unknown command %s - run without arguments for usage" % c)
            emit(RES)
    except ModelDie as e:
        err.append(str(e) + "\n")
        return finish(255)
    emit("total resources used: " + RES)
    if ofile[0] is not None:
        out.append("total resources used: " + RES)
    return finish(0)


# ---- the golden fixtures of tests/golden/make_mosh_golden.py ----------------------------------------------------------------
GOLD = os.path.join(orc.GOLDEN, "mosh")
MANIFEST = os.path.join(orc.GOLDEN, "mosh_manifest.json")


def manifest():
    import json
    with open(MANIFEST) as f:
        return json.load(f)


def stage_case(man, case, d):
    """the inputs of a case as the generator laid them out: every input plain, g.fa.gz, and the .mosh files it needs"""
    os.makedirs(d, exist_ok=True)
    for n in man["inputs"]:
        with open(os.path.join(d, n), "wb") as f:
            f.write(read_maybe_gz(os.path.join(GOLD, "in", n + ".gz")))
    with open(os.path.join(GOLD, "in", "g.fa.gz"), "rb") as f, open(os.path.join(d, "g.fa.gz"), "wb") as g:
        g.write(f.read())
    for n in case["needs"]:
        with open(os.path.join(d, os.path.basename(n)), "wb") as f:
            f.write(read_maybe_gz(os.path.join(GOLD, n.replace("/", ".") + ".gz")))
    return set(os.listdir(d))


def check_case(case, d, before, status, stdout, stderr):
    """exit status, stdout / stderr lines and every output file of a run in d against the reference's"""
    import hashlib
    assert mask_lines(stderr) == case["stderr"]
    assert mask_lines(stdout) == case["stdout"]
    assert status == case["status"]
    made = sorted(set(os.listdir(d)) - before)
    assert made == sorted(case["outputs"]), (made, sorted(case["outputs"]))
    for n in made:
        with open(os.path.join(d, n), "rb") as f:
            data = f.read()
        got = mask_mosh(data) if n.endswith(".mosh") else "\n".join(mask_lines(data)).encode()
        if hashlib.sha256(got).hexdigest() != case["outputs"][n]:
            exp = read_maybe_gz(os.path.join(GOLD, "%s.%s.gz" % (case["name"], n)))
            raise AssertionError("%s of case %s differs from the reference's: %s" % (n, case["name"], orc.describe_diff(got, exp)))
