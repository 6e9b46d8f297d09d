"""Hand-built `.hash` states at the exact boundaries of the tail of --cluster (replay_kernel, point_sum_kernel, read_merge_kernel in
hash10x_amd/csrc/stage_c.hip; codeClusterFind and codeClusterReadMerge, hash10x.c:770-868), and the registry of cases the CPU and the GPU
tests run (test_cluster_states_cpu.py, test_cluster_states_gpu.py).

`image` generalises orc.hash_image: the per-block input is a CLUSHASH array, so hash, read and the file's subCluster are free, and the
table's nRead, nSubCluster and pointToMin are set per block. Everything else is hash_image's: version 2, an empty index table,
hashValue = 31 * index, depth = number of records that hold the index.

A `Subject` is a block under test, described by its good hashes IN RANK ORDER and by the companion blocks that hold them. What
codeClusterFind makes of a rank follows from the companions alone (hash10x.c:794-806): a companion belongs to the first rank >= 1 that
holds it (its owner), and rank i counts, per earlier owner, the companions it holds. The builder therefore knows every rank's msBest,
msMax and msTot, replays the serial labelling, the cut at the 256th cluster and the read merge in plain Python (`Subject.expect`), and a
case's check compares that with the oracle's output before anything runs on the GPU: a changed builder cannot empty a case unnoticed.

A list is ascending in barcode number and block numbers are barcode numbers, so where a companion lies in the file decides which entry of a
rank's list it is. A companion lies behind every subject of the file unless it is made with front=True: then it lies directly in front of
its subject, in the order made. `Subject.lay` writes a whole list entry by entry — own entry, counted entries and fillers at stated
indices — and `Subject.lists` states, per rank, what the list loop is given and must find (`Rank`): the cases of tests/list_cases.py, a
registry of its own (REGISTRIES), are built on the two. A case carries its own --hashDepthRange (Case.lo, Case.hi).

TEST INFRASTRUCTURE — plain Python and numpy, never imported by hash10x_amd/."""
import collections
import functools

import numpy as np

from orc import BLOCK, CLUSHASH

LO, HI = 2, 100                                              # --hashDepthRange of a case that states none: a hash is good when 2 .. 99 records hold it
REPLAY_SMALL, REPLAY_MID = 2040, 16376                       # cluster.hpp
MERGE_SMALL_READS, MERGE_KEPT = 4096, 2048                   # stage_c.hip: read_merge_kernel's BIG form; records it keeps in registers


def image(blocks, B=20, values=None, table=None):
    """bytes of a version 2 .hash file (hash10x.c:244-267). blocks[i] = (records: CLUSHASH array, nRead, nSubCluster, pointToMin) of block
    i + 1. Asserts what the reference relies on without checking: every read below nRead, at most 255 clusters in a file's block.
    values: hashValue[] (slot 0 unused) in place of 31 * index, and with it the number of hash indices; table: hashIndex[2^B] in place of
    the empty one (tests/crib_cases.py: real hash values and the probe table that finds them)."""
    n_blocks = len(blocks) + 1
    block_table = np.zeros(n_blocks, dtype=BLOCK)
    for i, (rec, n_read, n_sub, ptm) in enumerate(blocks, start=1):
        assert rec.dtype == CLUSHASH and n_sub <= 255
        assert len(rec) == 0 or int(rec["read"].max()) < n_read, "block %d: a read beyond nRead (readMap[] is nRead long, hash10x.c:842)" % i
        block_table[i] = (n_read, len(rec), n_sub, 0, 0, ptm)
    hashes = np.concatenate([rec["hash"] for rec, _, _, _ in blocks]).astype(np.int64)
    n_index = int(hashes.max()) + 1 if values is None else len(values)
    assert hashes.size == 0 or int(hashes.max()) < n_index
    depth = np.bincount(hashes, minlength=n_index).astype("<u4")
    values = np.arange(n_index, dtype="<u8") * 31 if values is None else np.asarray(values, dtype="<u8")
    table = bytes(4 << B) if table is None else np.asarray(table, dtype="<u4").tobytes()
    assert len(table) == 4 << B

    def array_header(n, size):
        return np.array([(8918274, 0, 0, n, size, n, 0)], dtype="<i4,<i4,<u8,<i4,<i4,<i4,<i4").tobytes()

    u16, u32 = (lambda v: int(v).to_bytes(2, "little")), (lambda v: int(v).to_bytes(4, "little"))
    head = b"10XH" + u32(2) + u16(8) + u16(32) + u32(B) + table + u32(n_index) + values.tobytes()
    return b"".join([head, array_header(n_index, 4), depth.tobytes(), array_header(n_blocks, 32), block_table.tobytes()] + [rec.tobytes() for rec, _, _, _ in blocks])


def plain_image(blocks, B=20):
    """orc.hash_image through `image` (same bytes): blocks[i] = the hash indices of block i + 1, every read 0, nRead 1."""
    out = []
    for b in blocks:
        rec = np.zeros(len(b), dtype=CLUSHASH)
        rec["hash"] = np.asarray(b, dtype=np.int64)
        out.append((rec, 1, 0, 0.0))
    return image(out, B)


Rank = collections.namedtuple("Rank", "d own best mx tot q at codes")
# one rank's list as the list loop sees it (Subject.lists): d entries, ascending in barcode number, the block's own among them at index `own`;
# msBest (None: no counted entry), msMax and msTot of hash10x.c:801-806; q = minShareCount[clusterMin[label]] of an active rank (hash10x.c:821), else 0;
# at = {owner: indices of its entries in the list} (an entry's chunk is index // 64); codes = the barcode number of every entry (after State.build)

Expect = collections.namedtuple("Expect", "n raw abandoned stop labelled terms all_terms ptm nsub labels")
# n good hashes; raw clusters of codeClusterFind (0 if abandoned); stop = the abandoning turn; labelled = good hashes with a label before the merge;
# terms = [(rank, a, b)] of the pointToMin quotients a / b added up to the stop, all_terms = the same without the cut at 255 clusters;
# ptm, nsub, labels (per record, file order) = the block as --cluster leaves it


class Subject:
    """One block under test. Records in file order: front extras, the good hashes in rank order, back extras. An extra is a record whose hash
    only this block holds (depth 1: outside the range), with any read and any stale label."""

    def __init__(self, n_read=None, n_sub=0, ptm=0.0, raw=None):
        self.read, self.label = [], []                       # per rank: read, label in the file (wiped by codeClusterFind)
        self.comps = []                                      # companion blocks: the ranks whose hashes each holds
        self.comp_front = []                                 # per companion: it lies in front of the subject in the file (a lower barcode number), else behind every subject
        self.comp_code = []                                  # per companion: its barcode number (State.build)
        self.owned = {}                                      # rank -> the companions made for it by own()
        self.front, self.back = [], []                       # extras: (read, label)
        self.n_read, self.n_sub, self.ptm = n_read, n_sub, ptm
        self.raw = raw                                       # declared raw cluster count where extras carry labels (checked against the replay)
        self.code = None
        self.in_range = True                                 # False: --cluster does not reach the block

    # ---- construction
    def rank(self, read=None, label=0):
        """a further good hash, on a read of its own unless one is given"""
        self.read.append(len(self.read) if read is None else read); self.label.append(label)
        return len(self.read) - 1

    def ranks(self, k, label=0):
        first = len(self.read)
        self.read.extend(range(first, first + k)); self.label.extend([label] * k)
        return range(first, first + k)

    def comp(self, members, front=False):
        self.comps.append(members if isinstance(members, range) else list(members)); self.comp_front.append(front)

    def extra(self, read=0, label=0, front=False, k=1):
        (self.front if front else self.back).extend([(read, label)] * k)

    def start(self):
        """rank 0, which is never processed (hash10x.c:789)"""
        if not self.read:
            self.rank()

    def pair(self, k):
        """k clusters of two: C_m founds cluster m on R_m, term 1/1 (at -ct 1). Returns [(R_m, C_m)]."""
        self.start()
        out = []
        for _ in range(k):
            r, c = self.rank(), self.rank()
            self.comp([r, c])
            out.append((r, c))
        return out

    def pad(self, m):
        """m further ranks, all held by one companion: one more cluster, every rank pointing at the first of them"""
        self.start()
        r = self.ranks(m)
        self.comp(r)
        return r

    def chain(self, m):
        """m further ranks, each sharing a companion with the one before: every rank points at the rank before it, the longest msBest chain there
        is; the second founds a cluster on the first (term 1/1), every later term is 0/1"""
        r = self.ranks(m)
        for i in r[:-1]:
            self.comp([i, i + 1])
        return r

    def own(self, f, k, front=False):
        """k companions that rank f owns (held by f alone until a child() joins them)"""
        for _ in range(k):
            c = [f]
            self.comps.append(c); self.comp_front.append(front)   # (the list itself: child() appends to it)
            self.owned.setdefault(f, []).append(c)

    def child(self, shares):
        """a further rank that holds shares[f] of the companions rank f owns (own())"""
        i = self.rank()
        for f, a in shares.items():
            assert len(self.owned.get(f, [])) >= a, "rank %d owns fewer than %d companions" % (f, a)
            for c in (self.owned[f][:a] if a >= 0 else self.owned[f][a:]):   # (a < 0: the LAST -a of them)
                c.append(i)
        return i

    def fill(self, i, k, front=False):
        """k fillers of rank i — companions that hold it alone and count for nobody — at this place of the file order"""
        for _ in range(k):
            self.comp([i], front)

    def lay(self, i, d, own_at, counted):
        """the whole list of rank i, entry by entry: d entries, the block's own at index own_at, counted[index] = the earlier rank that owns the entry
        there (a companion of its own, held by the two), a filler everywhere else. Call once per rank, ranks in ascending order."""
        assert 0 <= own_at < d and own_at not in counted and all(0 <= j < d and 1 <= f < i for j, f in counted.items())
        for j in range(d):
            if j != own_at:
                self.comp([counted[j], i] if j in counted else [i], front=j < own_at)

    # ---- what the reference makes of it
    def _level(self, lo=LO, hi=HI):
        """fillers — companions that hold one rank alone: they count for nobody — until the depths are >= 2 and never fall along the ranks, so that the
        order of the ranks is the order written here (goodHashes are sorted by depth, ties keep their position: hash10x.c:758)"""
        n = len(self.read)
        d = np.ones(n, dtype=np.int64)
        for c in self.comps:
            d[np.asarray(c, dtype=np.int64)] += 1
        need = np.maximum(np.maximum.accumulate(np.maximum(d, lo)) - d, 0)
        for i in np.flatnonzero(need):
            self.fill(int(i), int(need[i]))
        d += need
        assert n == 0 or (d.min() >= lo and d.max() < hi and np.all(np.diff(d) >= 0))

    def lists(self, ct):
        """per rank, what the list loop is given and what it must find (Rank above); after State.build, which adds the levelling fillers and numbers the companions"""
        n = len(self.read)
        assert len(self.comp_code) == len(self.comps) == len(self.comp_front), "State.build first"
        order = sorted(range(len(self.comps)), key=lambda k: self.comp_code[k])
        ent = [[] for _ in range(n)]                         # per rank: (barcode number, owner or None) ascending
        for k in order:
            a = [int(x) for x in self.comps[k]]
            live = [x for x in a if x >= 1]
            f = min(live) if live else None
            for i in a:
                ent[i].append((self.comp_code[k], f if f is not None and i > f else None))
        q = {i: a for i, a, _ in self.replay(ct, cap=False)[4]}
        out = []
        for i in range(n):
            e = sorted(ent[i] + [(self.code, None)])
            assert [c for c, _ in e] == sorted({c for c, _ in e}), "rank %d: a companion twice" % i
            at = collections.OrderedDict()
            for j, (_, f) in enumerate(e):
                if f is not None and i >= 1:
                    at.setdefault(f, []).append(j)
            mx = max((len(v) for v in at.values()), default=0)
            best = min((f for f, v in at.items() if len(v) == mx), default=None)
            out.append(Rank(len(e), [c for c, _ in e].index(self.code), best, mx, sum(len(v) for v in at.values()), q.get(i, 0), at, [c for c, _ in e]))
        return out

    def replay(self, ct, cap=True):
        """codeClusterFind (hash10x.c:789-823) from the companions: labels per rank, raw clusters, abandoning turn, terms"""
        n = len(self.read)
        owners = [[] for _ in range(n)]
        for c in self.comps:
            a = np.asarray(c, dtype=np.int64)
            live = a[a >= 1]
            if live.size:
                f = int(live.min())
                for i in live.tolist():
                    if i > f:
                        owners[i].append(f)
        label, nsub, founder, terms, stop = [0] * n, 0, {}, [], None
        for i in range(1, n):
            if not owners[i]:
                continue
            cnt = collections.Counter(owners[i])
            tot, mx = len(owners[i]), max(cnt.values())
            best = min(j for j, v in cnt.items() if v == mx)
            if mx < ct:
                continue
            if not label[best]:
                nsub += 1
                if cap and nsub > 255:
                    return [0] * n, 0, True, i, terms
                label[best] = nsub; founder[nsub] = best
            label[i] = label[best]
            terms.append((i, cnt.get(founder[label[i]], 0), tot))
        return label, nsub, False, stop, terms

    def expect(self, ct):
        n_hash = len(self.front) + len(self.read) + len(self.back)
        n = len(self.read) if n_hash <= 65535 else 0         # hash10x.c:748: a block of more than 65535 records has no good hashes
        file_labels = [l for _, l in self.front] + list(self.label) + [l for _, l in self.back]
        reads = [r for r, _ in self.front] + list(self.read) + [r for r, _ in self.back]
        if not self.in_range:
            return Expect(n, None, False, None, 0, [], [], self.ptm, self.n_sub, file_labels)
        if n:
            lab, raw, abandoned, stop, terms = self.replay(ct)
            all_terms = self.replay(ct, cap=False)[4] if abandoned else terms
            ptm = 0.0
            for _, a, b in terms:
                ptm += a / b
            labels = [l for _, l in self.front] + lab + [l for _, l in self.back]
            if self.raw is not None:
                assert raw == self.raw, "declared %d raw clusters, the replay gives %d" % (self.raw, raw)
        else:
            raw, abandoned, stop, terms, all_terms, ptm, labels = self.n_sub, False, None, [], [], self.ptm, file_labels
        labelled = sum(1 for l in labels[len(self.front):len(self.front) + len(self.read)] if l) if n else 0
        # the rule the reference relies on (trueCluster[] is nSubCluster + 1 long, hash10x.c:842-846): no label beyond the count the merge sees
        assert raw == 0 or max(labels, default=0) <= raw, "a label beyond the %d clusters the read merge sees" % raw
        nsub = raw
        if raw:                                              # codeClusterReadMerge: components of labels sharing a read, numbered by ascending minimum
            parent = list(range(raw + 1))

            def find(x):
                while parent[x] != x:
                    parent[x] = parent[parent[x]]; x = parent[x]
                return x
            rep = {}
            for l, r in zip(labels, reads):
                if l:
                    r &= 0xFFFF
                    if r in rep:
                        a, b = find(l), find(rep[r])
                        if a != b:
                            parent[max(a, b)] = min(a, b)
                    else:
                        rep[r] = l
            mins = sorted({find(l) for l in range(1, raw + 1)})
            new = {m: k + 1 for k, m in enumerate(mins)}
            labels = [new[find(l)] if l else 0 for l in labels]
            nsub = len(mins)
        return Expect(n, raw, abandoned, stop, labelled, terms, all_terms, ptm, nsub, labels)


class State:
    """the blocks of one file: subjects and plain blocks in the order they are added, the subjects' companions behind them"""

    def __init__(self):
        self.items = []

    def subject(self, **kw):
        s = Subject(**kw)
        self.items.append(s)
        return s

    def plain(self, k=1):
        """a block of k records nobody shares (no good hashes, no labels)"""
        s = Subject()
        s.extra(k=k)
        self.items.append(s)
        return s

    @property
    def subjects(self):
        return self.items

    def build(self, crange=(1, 0), lo=LO, hi=HI):
        nxt = [1]                                            # hash indices from 1 on

        def fresh(k):
            a = np.arange(nxt[0], nxt[0] + k, dtype=np.int64); nxt[0] += k
            return a
        blocks, companions, behind = [], [], []
        for s in self.items:
            s._level(lo, hi)
            s.code = len(blocks) + 1 + sum(s.comp_front)      # its companions in front of it come first
            s.comp_code = [0] * len(s.comps)
            hf, hr, hb = fresh(len(s.front)), fresh(len(s.read)), fresh(len(s.back))
            rec = np.zeros(len(hf) + len(hr) + len(hb), dtype=CLUSHASH)
            rec["hash"] = np.concatenate([hf, hr, hb])
            reads = [r for r, _ in s.front] + list(s.read) + [r for r, _ in s.back]
            rec["read"] = np.asarray(reads, dtype=np.int64) & 0xFFFF
            rec["subCluster"] = [l for _, l in s.front] + list(s.label) + [l for _, l in s.back]
            n_read = s.n_read if s.n_read is not None else max(reads, default=0) + 1
            assert all(r < n_read for r in reads) and (n_read <= 65536 or max(reads, default=0) < 65536)
            for k, c in enumerate(s.comps):
                r2 = np.zeros(len(c), dtype=CLUSHASH)
                r2["hash"] = hr[np.asarray(c, dtype=np.int64)]
                if s.comp_front[k]:
                    blocks.append((r2, 1, 0, 0.0)); s.comp_code[k] = len(blocks)
                else:
                    companions.append((r2, 1, 0, 0.0)); behind.append((s, k))
            blocks.append((rec, n_read, s.n_sub, s.ptm))
            assert len(blocks) == s.code
        for j, (s, k) in enumerate(behind):
            s.comp_code[k] = len(blocks) + 1 + j
        n_codes = self.n_codes = len(blocks) + len(companions) + 1   # barcode numbers 1 .. n_codes - 1
        c_lo, c_hi = (crange[0] or 1), (crange[1] or n_codes)
        for s in self.items:
            s.in_range = c_lo <= s.code < c_hi
        assert not companions or len(self.items) == 1 or c_hi == n_codes, "companions lie behind the subjects: cluster to the end of the file"
        return image(blocks + companions)


Case = collections.namedtuple("Case", "name make ct crange heavy lo hi")   # lo, hi: the case's --hashDepthRange
CASES = collections.OrderedDict()
REGISTRIES = [CASES]                                         # every registry of cases (tests/list_cases.py adds its own): names are unique over all of them


def case(name, ct=1, crange=(1, 0), heavy=False, lo=LO, hi=HI, registry=CASES):
    def deco(f):
        assert not any(name in r for r in REGISTRIES)
        registry[name] = Case(name, f, ct, crange, heavy, lo, hi)
        return f
    return deco


def find(name):
    for r in REGISTRIES:
        if name in r:
            return r[name]
    raise KeyError("no case named %r in any registry" % (name,))


@functools.lru_cache(maxsize=None)
def built(name):
    """(the file's bytes, State, the case's own check) — made once per process"""
    c = find(name)
    st, where = c.make()
    data = st.build(c.crange, c.lo, c.hi)
    return data, st, where


def args(name, inp, out):
    """the command line of a case, for the reference binary and for tests/driver.run_commands"""
    c = find(name)
    return ["-B", 20, "-ct", c.ct, "--readHash", inp, "--hashDepthRange", c.lo, c.hi, "--cluster", c.crange[0], c.crange[1], "--writeHash", out]


def check(name, hf, n_good):
    """hf: orc.HashFile of the oracle's output, n_good: {code: good hashes} from the oracle. Every subject equals the builder's own replay — labels,
    cluster count, pointToMin bit for bit — and the case still sits where it is meant to (its own `where`)."""
    _, st, where = built(name)
    ct = find(name).ct
    ex = []
    for s in st.subjects:
        e = s.expect(ct)
        blk = hf.blocks[s.code]
        tag = "%s, block %d: " % (name, s.code)
        assert n_good[s.code] == e.n, tag + "%d good hashes, %d built" % (n_good[s.code], e.n)
        assert int(blk["nSubCluster"]) == e.nsub, tag + "nSubCluster %d, replay %d" % (blk["nSubCluster"], e.nsub)
        assert hf.block_clushash(s.code)["subCluster"].tolist() == e.labels, tag + "labels differ from the replay"
        assert np.float64(blk["pointToMin"]).tobytes() == np.float64(e.ptm).tobytes(), tag + "pointToMin %r, serial sum of the built terms %r" % (float(blk["pointToMin"]), e.ptm)
        ex.append(e)
    where(*ex)


def order_matters(e):
    """the serial sum of the terms differs from the sum in reversed order (a case for which it does not is rejected)"""
    fwd = rev = 0.0
    for _, a, b in e.terms:
        fwd += a / b
    for _, a, b in reversed(e.terms):
        rev += a / b
    assert fwd == e.ptm
    return fwd != rev


# ------------------------------------------------------------------------------------------------ replay classes by rank count
def _one_cluster(n):
    st = State(); s = st.subject()
    s.comp(s.ranks(n))

    def where(e):
        assert e.n == n and e.raw == 1 and e.labelled == n - 1 and e.ptm == float(n - 2)
    return st, where


def _chain(n):
    st = State(); s = st.subject()
    s.chain(n)

    def where(e):
        assert e.n == n and e.raw == 1 and e.labelled == n - 1 and e.ptm == 1.0
        assert all(a == 0 and b == 1 for _, a, b in e.terms[1:]) and len(e.terms) == n - 2
    return st, where


@case("n1")
def _():
    """one good hash: the loop never runs; the file's label, nSubCluster and pointToMin are reset"""
    st = State(); s = st.subject(n_sub=3, ptm=2.5)
    s.rank(label=2)
    return st, lambda e: (e.n, e.nsub, e.ptm, e.labels) == (1, 0, 0.0, [0]) or moved()


@case("n2")
def _():
    st = State(); s = st.subject(n_sub=1, ptm=1.0)
    s.comp([s.rank(label=1), s.rank(label=1)])
    return st, lambda e: (e.n, e.raw, e.labelled) == (2, 0, 0) or moved()


@case("n3")
def _():
    st = State(); s = st.subject()
    s.pair(1)
    return st, lambda e: (e.n, e.raw, e.labelled, e.ptm) == (3, 1, 2, 1.0) or moved()


def moved():
    raise AssertionError("the case no longer sits where it is meant to")


for _n in (REPLAY_SMALL, REPLAY_SMALL + 1, REPLAY_MID, REPLAY_MID + 1):
    case("one_%d" % _n, heavy=_n > REPLAY_MID - 1)(functools.partial(_one_cluster, _n))
    case("chain_%d" % _n, heavy=_n > REPLAY_MID - 1)(functools.partial(_chain, _n))
case("one_65535", heavy=True)(functools.partial(_one_cluster, 65535))   # every record of a block of 65535 good: the largest block there is


# ------------------------------------------------------------------------------------------------ 255 / 256 clusters
def _pairs(k, pad=0, file_labels=False):
    def make():
        st = State(); s = st.subject(n_sub=9 if file_labels else 0, ptm=3.5 if file_labels else 0.0)
        s.pair(k)
        if pad:
            s.pad(pad)
        if file_labels:
            s.label = [1 + i % 9 for i in range(len(s.label))]
        n = 1 + 2 * k + pad
        clusters = k + (1 if pad else 0)

        def where(e):
            assert e.n == n
            if clusters > 255:
                assert e.abandoned and e.nsub == 0 and e.ptm == 255.0 and not any(e.labels) and e.stop == 2 * 256
            else:
                assert not e.abandoned and e.raw == clusters == e.nsub and e.labelled == n - 1
        return st, where
    return make


case("pair255")(_pairs(255))
case("pair256")(_pairs(256))                                  # the abandoning turn is the last rank of the block
case("pair300")(_pairs(300))
case("pair256_file_labels")(_pairs(256, file_labels=True))       # labels and a cluster count in the file of a block that is given up: all wiped
case("pair254_pad1600")(_pairs(254, 1600))                     # 2109 ranks: the middle class
case("pair255_pad1600")(_pairs(255, 1600))
case("pair254_pad16000", heavy=True)(_pairs(254, 16000))       # 16509 ranks: the HBM-scratch class
case("pair255_pad16000", heavy=True)(_pairs(255, 16000))


@case("abandon_second_stripe")
def _():
    """the abandoning turn at a rank in 1024 .. 2047: the second stripe of 4 x 256 threads of the small class"""
    st = State(); s = st.subject()
    s.pair(255); s.ranks(600); s.pair(1); s.pair(3)

    def where(e):
        assert e.abandoned and 1024 <= e.stop < 2048 and e.n <= REPLAY_SMALL and e.ptm == 255.0 and e.stop < e.n - 1
    return st, where


@case("abandon_second_stripe_mid")
def _():
    """the same in the middle class: a rank in 4096 .. 8191, the second stripe of 4 x 1024 threads"""
    st = State(); s = st.subject()
    s.pair(254); s.pad(4000); s.pair(2)

    def where(e):
        assert e.abandoned and 4096 <= e.stop < 8192 and REPLAY_SMALL < e.n <= REPLAY_MID and e.ptm == 254.0 + 3999.0
    return st, where


@case("abandon_terms_both_sides")
def _():
    """active ranks with uneven terms before AND after the abandoning turn: pointToMin keeps exactly the terms of the turns before it"""
    st = State(); s = st.subject()
    s.start()
    a, b = s.rank(), s.rank()
    s.own(a, 5); s.own(b, 5)
    for x, y in ((2, 1), (1, 2), (3, 4), (5, 2), (1, 5), (2, 3)):
        s.child({a: x, b: y})
    s.pair(253)                                              # clusters 3 .. 255
    s.pair(1)                                                # the 256th
    for x, y in ((1, 2), (4, 3), (2, 5), (3, 1)):
        s.child({a: x, b: y})

    def where(e):
        full = 0.0
        for _, p, q in e.all_terms:
            full += p / q
        assert e.abandoned and e.nsub == 0 and len(e.all_terms) == len(e.terms) + 5 and full != e.ptm
        assert any(p != q for _, p, q in e.terms) and any(p != q and p for _, p, q in e.all_terms[len(e.terms):])
    return st, where


# ------------------------------------------------------------------------------------------------ the ordered sum
FRACTIONS = ((1, 1, 1), (2, 1, 0), (1, 3, 3), (2, 5, 0), (1, 0, 6), (3, 2, 2), (1, 0, 0), (4, 1, 2), (1, 1, 0), (2, 2, 1), (1, 2, 0), (3, 1, 1))


def _fractions(n, hole=False, shift=0):
    """three roots and children that share x, y and z companions with them: terms thirds, sevenths, max / (x + y + z). hole: a chain stretch
    in the middle whose terms are all 0/1, over at least one aligned group of 64 ranks"""
    def make():
        st = State(); s = st.subject()
        s.start()
        roots = (s.rank(), s.rank(), s.rank())
        for f in roots:
            s.own(f, 6)
        k = shift
        while len(s.read) < (70 if hole else n):
            s.child(dict(zip(roots, FRACTIONS[k % len(FRACTIONS)]))); k += 1
        if hole:
            s.chain(150)
            while len(s.read) < n:
                s.child(dict(zip(roots, FRACTIONS[k % len(FRACTIONS)]))); k += 1

        def where(e):
            assert e.n == n and not e.abandoned and order_matters(e)
            assert {(1, 3), (2, 3), (3, 7), (4, 7), (5, 7), (6, 7), (2, 5)} <= {(p, q) for _, p, q in e.terms}
            if hole:
                t = np.zeros(e.n)
                for i, p, q in e.terms:
                    t[i] = p / q
                g = [bool(np.any(t[j:j + 64])) for j in range(0, e.n, 64)]
                assert any(not g[j] and any(g[:j]) and any(g[j + 1:]) for j in range(len(g))), "no all-zero group of 64 terms between non-zero ones"
        return st, where
    return make


for _n in (63, 64, 65, 128, 129):
    case("sum_%d" % _n)(_fractions(_n, shift=1))               # (shift 1: of the twelve rotations of FRACTIONS the one for which the order of addition matters at all six sizes)
case("sum_300_zero_group")(_fractions(300, hole=True, shift=1))


# ------------------------------------------------------------------------------------------------ the threshold's edge
def _threshold(ct):
    def make():
        st = State(); s = st.subject()
        s.start()
        a = s.rank()
        s.own(a, ct)
        at = s.child({a: ct})                                # msMax == ct: active
        below = s.child({a: ct - 1})                         # msMax == ct - 1: not

        def where(e):
            lab = e.labels
            assert e.raw == 1 and lab[a] == 1 and lab[at] == 1 and lab[below] == 0 and e.terms == [(at, ct, ct)]
        return st, where
    return make


case("threshold_2", ct=2)(_threshold(2))
case("threshold_3", ct=3)(_threshold(3))


@case("tie", ct=2)
def _():
    """rank 3 shares two companions with rank 1 and two with rank 2: msBest is rank 1 (strict >), the term 2/4"""
    st = State(); s = st.subject()
    s.start()
    a, b = s.rank(), s.rank()
    s.own(a, 2); s.own(b, 2)
    c = s.child({a: 2, b: 2})
    return st, lambda e: (e.terms == [(c, 2, 4)] and e.labels[a] == 1 and e.labels[b] == 0 and e.raw == 1) or moved()


@case("best_in_other_cluster")
def _():
    """a rank whose msBest is an ACTIVE rank of a cluster founded elsewhere: it takes the label of that chain's root, its term is 0 / msTot"""
    st = State(); s = st.subject()
    s.start()
    a, d = s.rank(), s.rank()
    s.own(a, 1); s.own(d, 2)
    e1 = s.child({d: 1})                                     # founds cluster 1 on d
    b = s.child({a: 1})                                      # founds cluster 2 on a
    s.own(b, 2)
    c = s.child({b: 2, d: 1})                                # msBest b (2 > 1): label of a's cluster, 0 / 3

    def where(e):
        assert e.labels[d] == e.labels[e1] == 1 and e.labels[a] == e.labels[b] == e.labels[c] == 2 and e.terms[-1] == (c, 0, 3) and e.raw == 2
    return st, where


# ------------------------------------------------------------------------------------------------ the read merge
def _path(order):
    """pair(255) with the clusters joined into one path in the given order of labels: C of one and R of the next on one read"""
    def make():
        st = State(); s = st.subject(n_read=256)
        p = s.pair(255)
        seq = order(255)
        assert sorted(seq) == list(range(1, 256))
        s.read[p[seq[0] - 1][0]] = 0
        for t in range(254):
            s.read[p[seq[t] - 1][1]] = t + 1
            s.read[p[seq[t + 1] - 1][0]] = t + 1
        s.read[p[seq[-1] - 1][1]] = 255
        s.read[0] = 255
        return st, lambda e: (e.raw == 255 and e.nsub == 1 and e.labelled == 510) or moved()
    return make


def _interleaved(k):
    out = []
    for i in range((k + 1) // 2):
        out.append(1 + i)
        if k - i != 1 + i:
            out.append(k - i)
    return out


case("path255")(_path(lambda k: list(range(1, k + 1))))
case("path255_reversed")(_path(lambda k: list(range(k, 0, -1))))
case("path255_interleaved")(_path(_interleaved))             # 1 - 255 - 2 - 254 - ...


@case("merge_127_pairs")
def _():
    """255 clusters joined two by two, m with 256 - m, and 128 alone: 128 components, numbered by ascending minimum"""
    st = State(); s = st.subject(n_read=600)
    p = s.pair(255)
    nxt = 1
    for r, c in p:
        s.read[r], s.read[c] = nxt, nxt + 1; nxt += 2
    for m in range(1, 128):
        s.read[p[256 - m - 1][0]] = s.read[p[m - 1][1]]

    def where(e):
        assert e.raw == 255 and e.nsub == 128
        for m in range(1, 128):
            assert e.labels[p[m - 1][0]] == e.labels[p[256 - m - 1][1]] == m
        assert e.labels[p[127][0]] == 128
    return st, where


def _link_on_last_read(n_read, front=0, n_hash=None):
    """two clusters whose only link lies on the last read the block can store; `front` extras ahead of them"""
    def make():
        st = State(); s = st.subject(n_read=n_read)
        (r1, c1), (r2, c2) = s.pair(2)
        last = min(n_read, 65536) - 1
        s.read[0], s.read[r1], s.read[c1], s.read[r2], s.read[c2] = 2, 0, last, 1, last
        s.extra(read=3, front=True, k=front)
        return st, lambda e: (e.raw == 2 and e.nsub == 1 and e.labelled == 4 and (n_hash is None or len(e.labels) == n_hash)) or moved()
    return make


case("reads_4096")(_link_on_last_read(MERGE_SMALL_READS))
case("reads_4097")(_link_on_last_read(MERGE_SMALL_READS + 1))
case("reads_65535")(_link_on_last_read(65535))               # (the link on read 65534: the last one such a block has)
case("reads_65536")(_link_on_last_read(65536))
case("reads_70000")(_link_on_last_read(70000))               # reads are stored modulo 2^16: the link on read 65535
case("hashes_2048")(_link_on_last_read(8, front=MERGE_KEPT - 5, n_hash=MERGE_KEPT))       # the linking records at positions 2045 and 2047: the last ones kept in registers
case("hashes_2049")(_link_on_last_read(8, front=MERGE_KEPT - 4, n_hash=MERGE_KEPT + 1))   # ... at 2046 and 2048: one kept, one re-read


@case("stale_link")
def _():
    """2100 extras in front; five good hashes carry the file's label 7 and are wiped; an extra BEHIND position 2048 carries the stale label 2 on the
    read of cluster 1's child: the two clusters merge through a record that is no good hash"""
    st = State(); s = st.subject(n_sub=9, ptm=3.5, raw=2, n_read=16)
    (r1, c1), (r2, c2) = s.pair(2)
    s.label = [7] * 5
    s.read[0], s.read[r1], s.read[c1], s.read[r2], s.read[c2] = 9, 1, 2, 3, 4
    s.extra(read=10, front=True, k=2100)
    s.extra(read=2, label=2)

    def where(e):
        assert e.nsub == 1 and e.ptm == 2.0 and [l for l in e.labels if l] == [1] * 5 and len(e.labels) == 2106
    return st, where


@case("unlabelled_on_shared_read")
def _():
    """a read shared by a labelled and an unlabelled record does not merge: 1 - (0) - 2 is no path"""
    st = State(); s = st.subject(n_read=8)
    (r1, c1), (r2, c2) = s.pair(2)
    u = s.rank(read=5)                                       # never active: label 0
    s.read[0], s.read[r1], s.read[c1], s.read[r2], s.read[c2] = 5, 1, 5, 3, 5 + 1
    s.extra(read=6, label=0); s.extra(read=5, label=0)
    return st, lambda e: (e.raw == 2 and e.nsub == 2 and e.labels[u] == 0) or moved()


@case("stale_label_renumbered")
def _():
    """an extra with a valid stale label is renumbered with its cluster: 1 and 3 merge, the extra's 3 becomes 1, 2 stays"""
    st = State(); s = st.subject(n_read=16, raw=3, n_sub=3)
    (r1, c1), (r2, c2), (r3, c3) = s.pair(3)
    for i, r in enumerate((0, r1, c1, r2, c2, r3, c3)):
        s.read[r] = i
    s.read[r3] = s.read[c1]
    s.extra(read=12, label=3); s.extra(read=13, label=2, front=True)
    return st, lambda e: (e.nsub == 2 and e.labels[-1] == 1 and e.labels[0] == 2) or moved()


# ------------------------------------------------------------------------------------------------ blocks the clustering does not enter
def _no_good(st, labels, reads, n_sub, ptm=1.5, n_read=None, k_tail=0):
    s = st.subject(n_sub=n_sub, ptm=ptm, n_read=n_read)
    for l, r in zip(labels, reads):
        s.extra(read=r, label=l)
    if k_tail:
        s.extra(k=k_tail)
    return s


@case("nogood_unmerged")
def _():
    """no good hashes, nSubCluster 2, labels 1, 2, 2, the first two records on one read: codeClusterReadMerge runs all the same (hash10x.c:1250-1253)"""
    st = State()
    _no_good(st, (1, 2, 2), (0, 0, 1), 2)
    st.plain()
    return st, lambda e, _: (e.n == 0 and e.nsub == 1 and e.labels == [1, 1, 1] and e.ptm == 1.5) or moved()


@case("nogood_merged")
def _():
    st = State()
    _no_good(st, (1, 2, 2), (0, 1, 2), 2)
    st.plain()
    return st, lambda e, _: (e.n == 0 and e.nsub == 2 and e.labels == [1, 2, 2]) or moved()


@case("nogood_many_reads")
def _():
    """the same with more than 4096 reads and the link on the last one: the BIG form of the merge, for a block that has no good hashes"""
    st = State()
    _no_good(st, (1, 2, 3, 3), (0, 4999, 4999, 7), 3, n_read=5000)
    st.plain()
    return st, lambda e, _: (e.n == 0 and e.nsub == 2 and e.labels == [1, 2, 2, 2]) or moved()


@case("nogood_65536_records", heavy=True)
def _():
    """a block of more than 65535 records — ignored by the clustering even where its hashes are in range (hash10x.c:748) — with unmerged labels"""
    st = State()
    s = st.subject(n_sub=3, ptm=0.5, n_read=5000)
    x, y = s.rank(read=1, label=1), s.rank(read=4999, label=3)
    s.comp([x, y])                                           # in range: depth 2
    s.extra(read=4999, label=2); s.extra(read=9, label=3)
    s.extra(read=11, k=65536)
    st.plain()
    return st, lambda e, _: (e.n == 0 and len(e.labels) > 65535 and e.nsub == 2 and e.labels[:4] == [1, 2, 2, 2]) or moved()


@case("nogood_range_3_5", crange=(3, 5))
def _():
    """--cluster 3 5 on eight blocks that all carry unmerged labels: blocks 3 and 4 are merged, the others stay byte for byte"""
    st = State()
    for k in range(8):
        _no_good(st, (1, 2, 3, 2 + k % 2), (0, 0, 1 + k % 2, 2), 3, ptm=0.25 * k)

    def where(*ex):
        assert [e.nsub for e in ex] == [3, 3, 2, 2, 3, 3, 3, 3]
        assert ex[2].labels == [1, 1, 2, 1] and ex[3].labels == [1, 1, 2, 2] and ex[4].labels == [1, 2, 3, 2]
    return st, where


# ------------------------------------------------------------------------------------------------ the file of the command-line case
@case("cli_mix")
def _():
    """a 255-cluster block, a block given up at the 256th, a block without good hashes that carries unmerged labels, a block of one good hash"""
    st = State()
    st.subject().pair(255)
    st.subject().pair(256)
    _no_good(st, (1, 2, 2), (0, 0, 1), 2)
    st.subject(n_sub=3, ptm=2.5).rank(label=2)

    def where(a, b, c, d):
        assert a.raw == a.nsub == 255 and b.abandoned and (c.n, c.nsub, c.labels) == (0, 1, [1, 1, 1]) and (d.n, d.nsub) == (1, 0)
    return st, where


def run_oracle(name, cwd):
    """the case through the CPU oracle in directory cwd: (bytes of its .hash, {code: good hashes of the subjects}); leaves NAME.in.hash there"""
    import os
    import orc
    from driver import run_commands
    data, st, _ = built(name)
    with open(os.path.join(cwd, name + ".in.hash"), "wb") as f:
        f.write(data)
    o = run_commands(lambda k, w, r, b: orc.Oracle(k, w, r, b), args(name, name + ".in.hash", name + ".orc.hash"), cwd)
    n_good = {s.code: len(o.good_hashes(s.code)) for s in st.subjects}
    o.close()
    with open(os.path.join(cwd, name + ".orc.hash"), "rb") as f:
        return f.read(), n_good
