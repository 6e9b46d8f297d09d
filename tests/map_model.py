"""A plain NumPy / Python model of the reference's moshmap (moshmap.c with dict.c, array.c and readSequence's name cut): the Reference
object, the RFMSHv1 bytes, the Q / M / verbose texts and the command loop. The set and the hashes come from tests/mosh_model.py;
everything else is restated here and pinned to the reference by the golden fixtures of tests/golden/map (tests/test_moshmap_cpu.py)."""
import gzip
import hashlib
import json
import os
import struct

import numpy as np

import mosh_model as mm
from mosh_model import ModelDie

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "map")
MANIFEST = os.path.join(HERE, "golden", "map_manifest.json")
ARRAY_MAGIC = 8918274
M32 = 0xFFFFFFFF


# ---- dict.c ---------------------------------------------------------------------------------------------------------------------
def hash_string(s, bits, stride):
    rot = 21 if stride else 13
    x = 0
    for c in s.encode("latin-1"):
        c = c - 256 if c > 127 else c                          # char is signed
        x = (c ^ ((x >> (32 - rot)) | (x << rot))) & M32
    x &= (1 << bits) - 1
    return x | 1 if stride else x


class DictModel:
    def __init__(self, size=1024):
        self.dim, self.size = 10, 1024
        while self.size < size:
            self.dim += 1
            self.size *= 2
        self.table = [0] * self.size
        self.names = [None]

    @property
    def max(self):
        return len(self.names) - 1

    def _slot(self, table, s, compare):
        x, d = hash_string(s, self.dim, 0), None
        while True:
            i = table[x]
            if not i:
                return x, 0
            if compare and self.names[i] == s:
                return x, i
            if d is None:
                d = hash_string(s, self.dim, 1)
            x = (x + d) & ((1 << self.dim) - 1)

    def add(self, s):
        """(added, index from 0)"""
        x, i = self._slot(self.table, s, True)
        if i:
            return False, i - 1
        self.names.append(s)
        self.table[x] = self.max
        if self.max > 0.3 * self.size:
            self.dim += 1
            self.size *= 2
            t = [0] * self.size
            for j in range(1, self.max + 1):
                t[self._slot(t, self.names[j], False)[0]] = j
            self.table = t
        return True, self.max - 1

    def to_bytes(self):
        out = [struct.pack("<ii", self.dim, self.max), np.array(self.table, "<i4").tobytes(), b"\0" * 8 * (self.max + 1)]
        for n in self.names[1:]:
            b = n.encode("latin-1")
            out.append(struct.pack("<i", len(b)) + b)
        return b"".join(out)


# ---- the Reference ----------------------------------------------------------------------------------------------------------------
def c_ratio(a, b):
    """what printf("%.2f", a / (double) b) prints for integers"""
    if b == 0:
        return "-nan" if a == 0 else ("inf" if a > 0 else "-inf")
    return "%.2f" % (a / float(b))


def parse_fasta(data, name="file"):
    """(names, code arrays) as the reader delivers them; both loops of moshmap stop at the first sequence without bases"""
    if not data or data[:1] != b">":
        return [], []
    seqs, _ = mm.parse_seq_bytes(data, name)
    names = [ln[1:].split(b" ")[0].split(b"\t")[0].decode("latin-1") for ln in data.split(b"\n") if ln[:1] == b">"][:len(seqs)]
    for i, s in enumerate(seqs):
        if len(s) == 0:
            return names[:i], seqs[:i]
    return names, seqs


def array_dim_after(ids):
    """dim of array(ref->len, id, int) after ids 0 .. ids - 1 (array.c:144-170)"""
    dim = 1024
    for i in range(ids):
        if i >= dim:
            dim = dim * 2 if dim * 4 < (1 << 23) else dim + 1024 + (1 << 23) // 4
            if i >= dim:
                dim = i + 1
    return dim


class RefModel:
    def __init__(self, ms, size=1 << 26):
        self.ms, self.size = ms, size
        self.index, self.offset, self.id = [], [], []
        self.depth = {}
        self.dict, self.len, self.len_dim = DictModel(1024), [], 1024
        self.rev = self.loc = None

    @property
    def max(self):
        return len(self.index)

    def add_fasta(self, names, seqs):
        """referenceFastaRead's loop; returns totLen"""
        tot = 0
        for name, s in zip(names, seqs):
            added, i = self.dict.add(name)
            if not added:
                raise ModelDie("FATAL ERROR: duplicate ref sequence name %s" % name)
            self.len.append(len(s))
            tot += len(s)
            hs, ps = self.ms.moshes(s)
            for h, p in zip(hs, ps):
                ix = self.ms._find_add(int(h))
                if self.max + 1 >= self.size:
                    raise ModelDie("FATAL ERROR: reference size overflow")
                self.index.append(ix); self.offset.append(int(p)); self.id.append(i)
                self.depth[ix] = self.depth.get(ix, 0) + 1
        self.len_dim = array_dim_after(len(self.len))
        return tot

    def pack(self):
        """copy classes, then referencePack; returns (n1, n2, nM)"""
        n = [0, 0, 0]
        ms = self.ms
        for i in range(1, ms.max + 1):
            d = self.depth.get(i, 0)
            c = 1 if d == 1 else 2 if d == 2 else 3
            ms.info[i] = (ms.info[i] | 3) if c == 3 else ((ms.info[i] & 0xFC) | c)
            n[c - 1] += 1
        dep = [self.depth.get(i, 0) for i in range(ms.max + 1)]
        self.depth_arr = dep
        self.loc = [0] * (ms.max + 1)
        for i in range(1, ms.max + 1):
            self.loc[i] = self.loc[i - 1] + dep[i - 1]
        fill = [0] * (ms.max + 1)
        self.rev = [0] * self.max
        for i, ix in enumerate(self.index):
            self.rev[self.loc[ix] + fill[ix]] = i
            fill[ix] += 1
        self.size = self.max
        return tuple(n)

    def to_bytes(self):
        u = lambda v: np.array(v, "<u4").tobytes()
        lens = self.len + [0] * (self.len_dim - len(self.len))
        return (b"RFMSHv1\0" + struct.pack("<II", self.max, self.max) + u(self.index) + u(self.offset) + u(self.id) + u(self.depth_arr) + u(self.rev) + u(self.loc) +
                struct.pack("<iiQiiii", ARRAY_MAGIC, 0, 0, self.len_dim, 4, len(self.len), 0) + u(lens) + self.dict.to_bytes())

    @classmethod
    def from_bytes(cls, ms, data):
        """referenceRead of a well-formed file"""
        assert data[:8] == b"RFMSHv1\0"
        size, mx = struct.unpack_from("<II", data, 8)
        r = cls(ms, size)
        n1, off = ms.max + 1, 16

        def take(n):
            nonlocal off
            v = [int(x) for x in np.frombuffer(data, "<u4", n, off)]
            off += 4 * n
            return v
        r.index, r.offset, r.id = take(mx), take(mx), take(mx)
        r.depth_arr = take(n1); r.rev = take(mx); r.loc = take(n1)
        r.depth = {i: d for i, d in enumerate(r.depth_arr) if d}
        _, _, _, dim, _, amax, _ = struct.unpack_from("<iiQiiii", data, off)
        off += 32
        r.len_dim = dim
        r.len = take(dim)[:amax]
        ddim, dmax = struct.unpack_from("<ii", data, off)
        off += 8
        d = DictModel(1 << ddim)
        d.table = [int(x) for x in np.frombuffer(data, "<i4", d.size, off)]
        off += 4 * d.size + 8 * (dmax + 1)
        for _ in range(dmax):
            n = struct.unpack_from("<i", data, off)[0]
            d.names.append(data[off + 4:off + 4 + n].decode("latin-1"))
            off += 4 + n
        assert off == len(data)
        r.dict = d
        return r

    def query(self, name, s, verbose):
        """queryProcess for one sequence: a list of ("o" | "v", line): outFile and printf"""
        ms = self.ms
        hs, ps = ms.moshes(s)
        seeds = [(ms.ix.get(int(h), 0), int(p)) for h, p in zip(hs, ps)]
        copy, missed = [0, 0, 0, 0], 0
        for ix, _ in seeds:
            if ix:
                copy[ms.info[ix] & 3] += 1
            else:
                missed += 1
        L = len(s)
        ev = [("o", "Q\t%s\t%d\t%d miss, %d copy1, %d copy2, %d multi, %s hit\n" % (name, L, missed, copy[1], copy[2], copy[3], c_ratio(len(seeds) - missed, len(seeds))))]
        nm = lambda loc: self.dict.names[self.id[loc] + 1]

        def m_line():
            return ("o", "M\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d %d\t%s\t%s\n" % (name, seeds[i0][1], seeds[iN][1], L, nm(loc0), self.offset[loc0], self.offset[locN], n1, n2,
                                                                           c_ratio(n1 + n2, abs(locN - loc0)), c_ratio(n1, copy[1])))

        def ends(loc):
            if self.id[loc] != self.id[loc0]:
                return True
            end = False
            if loc0 < locN:
                d = (locN - loc0 - iN + i0) & M32
                end = loc < locN or not -50 <= (d - (1 << 32) if d >> 31 else d) <= 50
            elif loc0 > locN:
                d = (loc0 - locN - iN + i0) & M32
                end = loc > locN or not -50 <= (d - (1 << 32) if d >> 31 else d) <= 50
            return end
        loc0 = locN = i0 = iN = n1 = n2 = 0
        for i, (ix, pos) in enumerate(seeds):
            if not ix or (ms.info[ix] & 3) == 3:
                continue
            loc = self.rev[self.loc[ix]]
            is1 = (ms.info[ix] & 3) == 1
            if verbose:
                if is1:
                    ev.append(("v", "  %6d\t%s %d\n" % (pos, nm(loc), self.offset[loc])))
                else:
                    l2 = self.rev[self.loc[ix] + 1]
                    ev.append(("v", "  %6d\t%s %d\t%s %d\n" % (pos, nm(loc), self.offset[loc], nm(l2), self.offset[l2])))
            end = not loc0 or ends(loc)
            if end and loc0 and not is1:
                loc = self.rev[self.loc[ix] + 1]
                end = ends(loc)
            if end:
                if n1 > 2:
                    ev.append(m_line())
                n1 = n2 = 0
                loc0, i0 = loc, i
            if is1:
                n1 += 1
            else:
                n2 += 1
            locN, iN = loc, i
        if n2 > 2:
            ev.append(m_line())
        return ev


def _ref_tail(data, off):
    """(start of the dict's pointers, names) if an ArrayStruct at off and the dict behind it end exactly with the file"""
    if off + 32 > len(data):
        return None
    magic, _, _, dim, size, amax, _ = struct.unpack_from("<iiQiiii", data, off)
    if magic != ARRAY_MAGIC or size != 4 or not 0 <= amax <= dim or off + 32 + 4 * dim + 8 > len(data):
        return None
    d0 = off + 32 + 4 * dim
    ddim, dmax = struct.unpack_from("<ii", data, d0)
    if not 10 <= ddim <= 30 or dmax < 0:
        return None
    p0 = d0 + 8 + 4 * (1 << ddim)
    q = p0 + 8 * (dmax + 1)
    for _ in range(dmax):
        if q + 4 > len(data):
            return None
        q += 4 + struct.unpack_from("<i", data, q)[0]
    return (p0, dmax) if q == len(data) else None


def mask_ref(data):
    """ArrayStruct.base of len and the dict's name pointers are heap addresses in a file the reference wrote: parity = equality after
    zeroing them. The file does not say how long depth[] and loc[] are (the set's max + 1 each): the ArrayStruct behind them is found as
    the one from which the rest of the file parses to its last byte."""
    mx = struct.unpack_from("<I", data, 12)[0]
    off = 16 + 16 * mx + 8
    while off < len(data):
        tail = _ref_tail(data, off)
        if tail:
            p0, dmax = tail
            return data[:off + 8] + b"\0" * 8 + data[off + 16:p0] + b"\0" * 8 * (dmax + 1) + data[p0 + 8 * (dmax + 1):]
        off += 8
    raise AssertionError("no ArrayStruct found in the .ref bytes")


def mask_file(name, data):
    if name.endswith(".mosh"):
        return mm.mask_mosh(data)
    if name.endswith(".ref"):
        return mask_ref(data)
    return "\n".join(mm.mask_lines(data)).encode()


def _atoi(s):
    import re
    m = re.match(r"\s*[+-]?\d+", s)
    return int(m.group()) if m else 0


# ---- the command loop (moshmap.c:298-383) ---------------------------------------------------------------------------------------------
def run_commands(args, cwd):
    """returns (status, stdout text, stderr text); files are written under cwd"""
    out, err, ofile, files = [], [], [None], []
    RES = "user\t\n"
    k, w, seed, B = 19, 31, 17, 28
    verbose, ref = False, None

    def emit(s):
        (out if ofile[0] is None else ofile[0]).append(s)

    def path(p):
        return os.path.join(cwd, p)

    def finish(status):
        for lst, p in files:
            with open(path(p), "w") as f:
                f.write("".join(lst))
        return status, "".join(out), "".join(err)

    args = [str(a) for a in args]
    i = 0
    try:
        while i < len(args):
            a = args[i]
            if not a.startswith("-"):
                raise ModelDie("FATAL ERROR: option/command %s does not start with '-': run without arguments for usage" % a)
            j = i + 1
            while j < len(args) and not args[j].startswith("-"):
                j += 1
            err.append("COMMAND " + " ".join(args[i:j]) + "\n")
            left = len(args) - i

            def match(x, y, n):
                return a in (x, y) and left >= n
            if match("-K", "--kmer", 2):
                k = _atoi(args[i + 1]); i += 2
            elif match("-W", "--window", 2):
                w = _atoi(args[i + 1]); i += 2
            elif match("-S", "--seed", 2):
                seed = _atoi(args[i + 1]); i += 2
            elif match("-B", "--tableBits", 2):
                B = _atoi(args[i + 1]); i += 2
            elif match("-t", "--threads", 2):
                err.append("  can't set thread number - not compiled with OMP\n"); i += 2
            elif match("-v", "--verbose", 1):
                verbose = not verbose; i += 1
            elif match("-o", "--output", 2):
                p = args[i + 1]; i += 2
                if p == "-":
                    ofile[0] = None
                elif os.path.isdir(os.path.dirname(path(p)) or "."):
                    ofile[0] = []
                    files.append((ofile[0], p))
                else:
                    err.append("can't open output file %s - resetting to stdout\n" % p)
                    ofile[0] = None
            elif match("--slab", "--slab", 2) or match("--device", "--device", 2):
                i += 2
            elif match("-f", "--referenceFasta", 2):
                p = args[i + 1]; i += 2
                if not os.path.exists(path(p)):
                    raise ModelDie("FATAL ERROR: failed to open fasta file %s" % p)
                if k <= 0 or w <= 0:
                    raise ModelDie("FATAL ERROR: k %d, w %d must be > 0" % (k, w))
                if k >= 32:
                    raise ModelDie("FATAL ERROR: seqhash k %d must be between 1 and 32\n" % k)
                emit("  moshmap initialised with k = %d, w = %d, random seed = %d\n" % (k, w, seed))
                if not 20 <= B <= 34:
                    raise ModelDie("FATAL ERROR: table bits %d must be between 20 and 34" % B)
                ref = RefModel(mm.MoshModel(B, k, w, seed))
                with open(path(p), "rb") as f:
                    names, seqs = parse_fasta(f.read(), p)
                tot = ref.add_fasta(names, seqs)
                emit("  %d hashes from %d reference sequences, total length %d\n" % (ref.max, ref.dict.max, tot))
                emit("  %d copy 1, %d copy 2, %d multiple\n" % ref.pack())
            elif match("-q", "--query", 2):
                p = args[i + 1]; i += 2
                if ref is None:
                    raise ModelDie("FATAL ERROR: need to read a reference before processing query sequences")
                if not os.path.exists(path(p)):
                    raise ModelDie("FATAL ERROR: failed to open query file %s" % p)
                with open(path(p), "rb") as f:
                    names, seqs = parse_fasta(f.read(), p)
                for name, s in zip(names, seqs):
                    for stream, line in ref.query(name, s, verbose):
                        if stream == "v":
                            out.append(line)
                        else:
                            emit(line)
            elif match("-r", "--referenceRead", 2):
                p = args[i + 1]; i += 2
                for tag in ("mosh", "ref"):
                    if not os.path.exists(path(p + "." + tag)):
                        raise ModelDie("FATAL ERROR: failed to open %s.%s to read" % (p, tag))
                with open(path(p + ".mosh"), "rb") as f:
                    ms = mm.MoshModel.from_bytes(f.read())
                with open(path(p + ".ref"), "rb") as f:
                    ref = RefModel.from_bytes(ms, f.read())
            elif match("-w", "--referenceWrite", 2):
                p = args[i + 1]; i += 2
                if ref is None:
                    raise ModelDie("FATAL ERROR: -w needs a reference: give -f or -r first")
                with open(path(p + ".mosh"), "wb") as f:
                    f.write(ref.ms.to_bytes())
                with open(path(p + ".ref"), "wb") as f:
                    f.write(ref.to_bytes())
            else:
                raise ModelDie("FATAL ERROR: unkown command %s - run without arguments for usage" % a)
            emit(RES)
    except ModelDie as e:
        err.append(str(e) + "\n")
        return finish(255)
    emit("total resources used: " + RES)
    if ofile[0] is not None:
        out.append("total resources used: " + RES)
    return finish(0)


# ---- fixtures -------------------------------------------------------------------------------------------------------------------------
def manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def gold(name):
    with open(os.path.join(GOLD, name + ".gz"), "rb") as f:
        return gzip.decompress(f.read())


def stage_case(man, case, d):
    os.makedirs(d, exist_ok=True)
    for n in case["inputs"]:
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


# ---- malformed .ref files ---------------------------------------------------------------------------------------------------------------
def ref_offsets():
    """byte offsets of the parts of the golden idx.ref"""
    data = gold("build.idx.ref")
    n1 = struct.unpack_from("<I", gold("build.idx.mosh"), 12)[0]
    mx = struct.unpack_from("<I", data, 12)[0]
    o = {"index": 16, "offset": 16 + 4 * mx, "id": 16 + 8 * mx, "depth": 16 + 12 * mx}
    o["rev"] = o["depth"] + 4 * n1; o["loc"] = o["rev"] + 4 * mx; o["len"] = o["loc"] + 4 * n1
    dim = struct.unpack_from("<i", data, o["len"] + 16)[0]
    o["dict"] = o["len"] + 32 + 4 * dim
    ddim, dmax = struct.unpack_from("<ii", data, o["dict"])
    o["names"] = o["dict"] + 8 + 4 * (1 << ddim) + 8 * (dmax + 1)
    return data, o, mx


def put(data, at, value):
    return data[:at] + struct.pack("<I", value) + data[at + 4:]


def bad_refs():
    """the golden idx.ref broken in one place per rule of the reader: (name, bytes, part of the message)"""
    data, o, mx = ref_offsets()
    return [("header", b"RFMSHv2\0" + data[8:], "bad reference header"),
            ("size_not_max", put(data, 8, mx + 1), "size %d differs from max %d" % (mx + 1, mx)),
            ("cut_in_arrays", data[:o["rev"]], "do not fit its"),
            ("max_too_large", put(put(data, 8, 1 << 30), 12, 1 << 30), "do not fit its"),
            ("index_beyond_set", put(data, o["index"] + 40, 0xFFFFFFF0), "holds mosh index 4294967280 beyond"),
            ("id_beyond_names", put(data, o["id"], 2), "hit 0 is on sequence 2 of 2"),
            ("loc_not_the_sum", put(data, o["loc"] + 20, 77777), "loc[5] is 77777, the depths before it sum to"),
            ("depth_too_large", put(data, o["depth"] + 4, mx + 5), "its depths sum to more than its %d hits" % mx),
            ("rev_beyond_max", put(data, o["rev"] + 8, mx), "rev[2] is %d beyond its %d hits" % (mx, mx)),
            ("len_record_size", put(data, o["len"] + 20, 8), "failed read ref len"),
            ("len_dim", put(data, o["len"] + 16, 1 << 28), "failed read ref len"),
            ("dict_dim", put(data, o["dict"], 9), "dict dim 9 outside 10 .. 30"),
            ("dict_dim_past_file", put(data, o["dict"], 12), "does not fit the file"),
            ("dict_entry", put(data, o["dict"] + 8 + 4 * int(np.flatnonzero(np.frombuffer(data, "<i4", 1024, o["dict"] + 8))[0]), 9), "dict table entry 9 beyond its 2 names"),
            ("name_length", put(data, o["names"], 1 << 20), "name 1 of 1048576 bytes runs past the end of the file"),
            ("cut_in_names", data[:-2], "runs past the end of the file")]
