"""The crib and the reports that hang on it, restated in plain Python from the reference (hash10x.c): cribAddGenome (426-456), the classification
loop of cribBuild (479-492), codeClusterReport (891-943), clusterSplitCodes (956-996) and cribSummary's walk (1029-1047), with the text of the
lines the command-line tests compare. Checked against the reference binary's recorded output (tests/golden/crib/) and, on the GPU, against
crib_scan_kernel / crib_classify_kernel (csrc/stage_d.hip) and cluster_report_kernel / crib_summary_kernel / crib_words_kernel (csrc/stage_e.hip).

Everything is written the way the reference walks: one update per occurrence in file order, a 16-bit chr that is stepped and wrapped, a linked list
of disagreeing hashes — never the closed forms the kernels use, so that the two stay independent.

TEST INFRASTRUCTURE — plain Python and numpy, never imported by hash10x_amd/."""
import numpy as np

import orc

ERR, HTA, HTB, HOM, MUL = range(5)
TYPE_NAME = ("err", "htA", "htB", "hom", "mul")
NAN = "-nan"                                                 # what printf("%.1f") makes of 0.0 / 0 on x86-64 glibc: the quotient's sign bit is set
CHUNK = 1 << 22


def moshes(hasher, codes):
    """(hashes, k-mer start positions) of one sequence through orc.Oracle.mosh, in pieces of CHUNK k-mer starts: whether a k-mer is a mosh depends on
    the k-mer alone (seqhash.c:171-173, 187-191), so pieces that overlap by k - 1 bases give the sequence's moshes exactly"""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    k = hasher.k
    for at in range(0, max(len(codes) - k + 1, 0), CHUNK):
        hs, ps = hasher.mosh(codes[at:at + CHUNK + k - 1])
        yield hs, ps.astype(np.int64) + at


def add_genome(state, seqs):
    """cribAddGenome: state.values[i] = hash value of index i (slot 0 unused), state.hasher() = the Oracle of the state's k, w, seed.
    Returns (chr int16[], pos uint16[], known, unknown, count[]): the CribInfo array of one genome and the two figures of its line of text; count
    (occurrences per index) is for the cases' own checks only."""
    values = np.asarray(state.values, dtype=np.uint64)
    index = {int(v): i for i, v in enumerate(values.tolist()) if i}
    assert len(index) == len(values) - 1, "hash values of a state are distinct"
    member = np.sort(values[1:])
    chrom, pos, count = [0] * len(values), [0] * len(values), [0] * len(values)
    known = unknown = 0
    hasher = state.hasher()
    for number, s in enumerate(seqs, start=1):               # ++chr for every sequence, also one shorter than k
        for hs, ps in moshes(hasher, s):
            hit = np.isin(hs, member)
            unknown += int(hs.size - np.count_nonzero(hit))
            for h, p in zip(hs[hit].tolist(), ps[hit].tolist()):
                i = index[h]
                if chrom[i] == 0:
                    chrom[i] = number; pos[i] = (p >> 10) & 0xFFFF      # U16 pos = pos >> 10
                elif chrom[i] > 0:
                    chrom[i] = -1
                else:
                    chrom[i] -= 1
                    if chrom[i] < -32768:                    # --c->chr on an I16
                        chrom[i] += 65536
                count[i] += 1
                known += 1
    hasher.close()
    return np.array(chrom, dtype=np.int16), np.array(pos, dtype=np.uint16), known, unknown, np.array(count, dtype=np.int64)


class Crib:
    """what cribBuild leaves: type[], the merged chr[] / pos[], the depth histograms err, het, hom, mul as the reference's Arrays (hist[s] is arrayMax[s] long)"""

    def __init__(self, typ, chrom, pos, hist, depth):
        self.type, self.chr, self.pos, self.hist, self.depth = typ, chrom, pos, hist, depth
        self.array_max = [len(h) for h in hist]


def classify(crib_a, crib_b, depth):
    """hash10x.c:479-492 over (chr, pos) of the two genomes and hashDepth[]. Histogram slots: 0 err, 1 het, 2 hom, 3 mul."""
    ca, pa = [int(x) for x in crib_a[0]], [int(x) for x in crib_a[1]]
    cb, pb = [int(x) for x in crib_b[0]], [int(x) for x in crib_b[1]]
    n = len(ca)
    typ = [0] * n
    hist = [[], [], [], []]

    def bump(a, d):                                          # ++array(a, d, int): the Array grows to d + 1
        if len(a) <= d:
            a.extend([0] * (d + 1 - len(a)))
        a[d] += 1
    for i in range(1, n):
        d = int(depth[i])
        if ca[i] == 0 and cb[i] == 0:
            typ[i] = ERR; bump(hist[0], d)
        elif ca[i] > 0 and cb[i] > 0:
            typ[i] = HOM; bump(hist[2], d)
        elif ca[i] < 0 or cb[i] < 0:
            typ[i] = MUL; bump(hist[3], d)
            if cb[i] < ca[i]:
                ca[i] = cb[i]
        else:
            typ[i] = HTA if ca[i] else HTB
            bump(hist[1], d)
            if not ca[i]:
                ca[i] = cb[i]; pa[i] = pb[i]
    return Crib(np.array(typ, dtype=np.uint8), np.array(ca, dtype=np.int16), np.array(pa, dtype=np.uint16), hist, np.asarray(depth))


def n_good(rec, depth, lo, hi):
    """nGoodHashes[] of one block (hash10x.c:746-761)"""
    if len(rec) > 65535:
        return 0
    d = np.asarray(depth)[rec["hash"].astype(np.int64)]
    return int(np.count_nonzero((d >= lo) & (d < hi)))


def cluster_report(blocks, crib):
    """codeClusterReport's loop (hash10x.c:891-943) over blocks = [(records, nRead, nSubCluster, ...)]. Per block a dict: nClusHash, nClusRead and
    clusters = per label 1 .. nSubCluster {n, nRead, nt[5], chr, pMin, pMax, nBad, other: the hash indices of the OTHER list in print order}.
    info[] lives across the blocks and is cleared up to nSubCluster only (arrayReCreate, array.c:84-106), as in the reference: a label above nSubCluster
    counts in nClusHash / nClusRead and writes to a slot nobody prints before it is cleared."""
    fresh = lambda: {"n": 0, "nRead": 0, "nt": [0] * 5, "chr": 0, "pMin": 0, "pMax": 0, "nBad": 0, "bad": 0}
    info = [fresh() for _ in range(256)]
    out = []
    for blk in blocks:
        rec, n_read, n_sub = blk[0], blk[1], blk[2]
        for j in range(n_sub + 1):
            info[j] = fresh()
        read_clus = [0] * max(n_read, 1)
        bad_link = [0] * max(len(rec), 1)
        n_clus_hash = 0
        hashes, reads, labels = rec["hash"].tolist(), rec["read"].tolist(), rec["subCluster"].tolist()
        for i in range(len(rec)):
            c = labels[i]
            if not c:
                continue
            n_clus_hash += 1
            read_clus[reads[i]] = c
            r = info[c]
            r["n"] += 1
            bh = hashes[i]
            if crib is not None:
                t = int(crib.type[bh])
                r["nt"][t] += 1
                if ERR < t < MUL:
                    ch, ps = int(crib.chr[bh]), int(crib.pos[bh])
                    if not r["chr"]:
                        r["chr"] = ch; r["pMin"] = r["pMax"] = ps
                    elif ch == r["chr"]:
                        r["pMin"] = min(r["pMin"], ps); r["pMax"] = max(r["pMax"], ps)
                    else:
                        r["nBad"] += 1; bad_link[i] = r["bad"]; r["bad"] = i
        n_clus_read = 0
        for i in range(n_read):
            c = read_clus[i]
            if c:
                info[c]["nRead"] += 1; n_clus_read += 1
        clusters = []
        for j in range(1, n_sub + 1):
            r = dict(info[j]); r["nt"] = list(r["nt"])
            other, x, left = [], r["bad"], 10
            while x and left:
                left -= 1
                other.append(hashes[x]); x = bad_link[x]
            r["other"] = other
            clusters.append(r)
        out.append({"nClusHash": n_clus_hash, "nClusRead": n_clus_read, "clusters": clusters})
    return out


def cluster_split(blocks):
    """clusterSplitCodes (hash10x.c:956-996): blocks = [(records, nRead, nSubCluster, pointToMin)] of codes 1 ..; returns the new list as
    (records, nRead, nSubCluster, pointToMin, clusterParent): the old codes without their labelled records, then one block per sub-cluster. Only for
    states whose labels stay within nSubCluster (the reference indexes its new blocks by the label)."""
    base, made = [], []
    for code, (rec, n_read, n_sub, ptm) in enumerate(blocks, start=1):
        if not n_sub:
            base.append((rec.copy(), n_read, n_sub, ptm, 0))
            continue
        assert int(rec["subCluster"].max(initial=0)) <= n_sub
        keep, parts, read_map = [], [[] for _ in range(n_sub + 1)], {}
        n_reads = [0] * (n_sub + 1)
        for e in rec:
            e = e.copy()
            clus = int(e["subCluster"]); e["subCluster"] = 0
            if clus:
                rd = int(e["read"])
                if rd not in read_map:
                    n_reads[clus] += 1; read_map[rd] = n_reads[clus]
                e["read"] = read_map[rd] - 1
                parts[clus].append(e)
            else:
                keep.append(e)
        as_rec = lambda es: np.array(es, dtype=orc.CLUSHASH) if es else np.zeros(0, dtype=orc.CLUSHASH)
        base.append((as_rec(keep), n_read, 0, 0.0, 0))       # new1 is a zeroed block: only clusHash, nHash and nRead are set
        for j in range(1, n_sub + 1):
            made.append((as_rec(parts[j]), n_reads[j], 0, 0.0, code + 1))
    return base + made


def crib_summary(blocks, typ):
    """cribSummary's walk (hash10x.c:1029-1047) over blocks = [(records, ..., clusterParent)] of codes 1 .. (block 0 is a base code without records).
    Returns (countBase[5], countCluster[5], nBaseCode, nSubClusterCode, seenBase, seenCluster: the sets of hash indices met)."""
    base, clus, n_base, n_clus, seen_b, seen_c = [0] * 5, [0] * 5, 1, 0, set(), set()
    for blk in blocks:
        parent = blk[4] if len(blk) > 4 else 0
        hs = blk[0]["hash"].tolist()
        if parent:
            n_clus += 1
            for h in hs:
                clus[int(typ[h])] += 1; seen_c.add(h)
        else:
            n_base += 1
            for h in hs:
                base[int(typ[h])] += 1; seen_b.add(h)
    return base, clus, n_base, n_clus, seen_b, seen_c


def crib_words(blocks, typ):
    """the records of codes 1 .. in file order as h10x_crib_words packs them: bit 31 = a block --clusterSplit made, 28-30 the crib type, 0-27 the hash index"""
    out = []
    for blk in blocks:
        kind = 0x80000000 if (len(blk) > 4 and blk[4]) else 0
        out.extend(kind | (int(typ[h]) << 28) | h for h in blk[0]["hash"].tolist())
    return np.array(out, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------ text
def genome_line(known, unknown, n_seq):
    return "  read %d known and %d unknown hashes from %d sequences in crib genome" % (known, unknown, n_seq)


def _array_stats(a):
    """printArrayStats (hash10x.c:458-468)"""
    total = sum(a)
    mn = next((i for i, v in enumerate(a) if v), -1)
    weighted = float(sum(v * i for i, v in enumerate(a)))
    mean = ("%.1f" % (weighted / total)) if total else NAN
    return "  %d mean %s min %d max %d" % (total, mean, mn, len(a) - 1)


def crib_lines(crib, tables=True):
    err, het, hom, mul = crib.hist
    out = ["  crib matches", "    hom  " + _array_stats(hom), "    het  " + _array_stats(het), "    mul " + _array_stats(mul), "    err " + _array_stats(err)]
    if tables:
        out.append("CRIB_TABLE      i   err         het          hom         mul")
        at = lambda a, i: a[i] if len(a) > i else 0
        for i in range(1, 256):
            out.append("CRIB_TABLE      %4d%12d%12d%12d%12d" % (i, at(err, i), at(het, i), at(hom, i), at(mul, i)))
    return out


def crib_text(crib, x):
    """cribText (hash10x.c:512-521)"""
    t = int(crib.type[x])
    s = "%d:%s" % (x, TYPE_NAME[t])
    if ERR < t < MUL:
        s += "_%d.%d" % (int(crib.chr[x]), int(crib.pos[x]))
    return s + "-%d" % int(crib.depth[x])


def report_lines(blocks, crib, lo, hi, code_min, code_max):
    """--clusterReport codeMin codeMax after --hashDepthRange lo hi; code 0 is the empty block in front"""
    if not code_max:
        code_max = len(blocks) + 1
    rep = cluster_report(blocks[max(code_min, 1) - 1:code_max - 1], crib)
    out, total_good, total_ptm = [], 0, 0.0
    for code in range(code_min, code_max):
        if code == 0:
            out.append("  CLUSTER_SUMMARY 0 nRead 0 nHash 0 nGoodHash 0 nClusHash 0 nClusRead 0 nSubCluster 0")
            continue
        rec, n_read, n_sub, ptm = blocks[code - 1][:4]
        good = n_good(rec, crib.depth, lo, hi)
        r = rep[code - max(code_min, 1)]
        out.append("  CLUSTER_SUMMARY %d nRead %d nHash %d nGoodHash %d nClusHash %d nClusRead %d nSubCluster %d" % (code, n_read, len(rec), good, r["nClusHash"], r["nClusRead"], n_sub))
        for j, c in enumerate(r["clusters"], start=1):
            if not c["n"]:
                continue
            nt = c["nt"]
            ln = "    CODE_CLUSTER %d %d : %d reads %d hashes %d hom, %d htA, %d htB, %d mul, %d err" % (code, j, c["nRead"], c["n"], nt[HOM], nt[HTA], nt[HTB], nt[MUL], nt[ERR])
            if c["chr"]:
                ln += "  chr %d pos %d %d" % (c["chr"], c["pMin"], c["pMax"] - c["pMin"] + 1)
            if c["nBad"]:
                ln += "  OTHER %d" % c["nBad"] + "".join(" " + crib_text(crib, x) for x in c["other"])
            out.append(ln)
        total_good += good
        total_ptm += float(ptm)
    if total_good:
        out.append("  MIN_POINT_DENSITY %.3f" % (total_ptm / total_good))
    return out


def summary_lines(blocks, typ):
    """--cribSummary; the second figure of a type is the number of distinct hash indices (the reference's hashCount() runs ahead of it only after its table
    doubles, beyond 524 288 keys: tests/test_host_cpu.py)"""
    base, clus, n_base, n_clus, seen_b, seen_c = crib_summary(blocks, typ)

    def part(counts, seen):
        s = ""
        for t in range(5):
            distinct = sum(1 for h in seen if int(typ[h]) == t)
            s += " %s %d %d %s" % (TYPE_NAME[t], counts[t], distinct, ("%.1f" % (counts[t] / distinct)) if distinct else NAN)
        return s
    return ["  %d base codes " % n_base + part(base, seen_b), "  %d cluster codes " % n_clus + part(clus, seen_c)]


KEEP = ("  crib matches", "    hom", "    het", "    mul", "    err", "CRIB_TABLE", "  CLUSTER_SUMMARY", "    CODE_CLUSTER", "  MIN_POINT_DENSITY")


def report(text):
    """the lines of a program's stdout that the model restates"""
    if isinstance(text, bytes):
        text = text.decode(errors="replace")
    return [ln for ln in text.splitlines() if ln.startswith(KEEP) or " base codes " in ln or " cluster codes " in ln or " in crib genome" in ln]
