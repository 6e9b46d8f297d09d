"""Hand-built states and truth genomes at the boundaries of the crib kernels (crib_scan_kernel, crib_classify_kernel: csrc/stage_d.hip) and of the
kernels behind the crib's reports (cluster_report_kernel, crib_summary_kernel, crib_words_kernel: csrc/stage_e.hip), and the registry of cases the
CPU and the GPU tests run (test_crib_report_cpu.py, test_crib_report_gpu.py).

A state is a `.hash` image (cluster_states.image) with REAL hash values and the probe table that sequential insertion in index order leaves
(hashIndexFind, hash10x.c:139-152): the reference and crib_scan_kernel both look the genomes' moshes up in it. A case takes designed sequences, takes
their moshes from the model hasher (orc.Oracle.mosh, pinned to the reference), chooses which become members of the state and lays them into blocks
with hand-set read, subCluster, nRead, nSubCluster and pointToMin. With -k 21 -w 1 -r 3 every k-mer is a mosh, which gives full control; the
hash-value-0 case runs at -k 21 -w 31 -r 17. -B 20 throughout.

Every case carries its own check (`where`), made from the model's results alone, that it still hits what it is named for — "hash x occurs 32770
times in genome A", "the only occurrence starts at 1023" — so that a changed builder cannot empty a case unnoticed.

TEST INFRASTRUCTURE — plain Python and numpy, never imported by hash10x_amd/."""
import collections
import functools

import numpy as np

import cluster_states as cs
import crib_model as cm
import orc

K, B = 21, 20
RUN = 64                                                     # SEQ_RUN of csrc/seq_plan.hpp: k-mer starts per lane
REP_THREADS = 256                                            # stage_e.hip: threads of cluster_report_kernel
LO, HI = 1, 100000                                           # --hashDepthRange of every case: every hash a record holds is good


def rc(codes):
    return (3 - np.asarray(codes, dtype=np.uint8))[::-1].copy()


def probe_table(values, bits=B):
    """hashIndex[] after hashIndexFind(value, TRUE) of values[1], values[2], ... in that order (hash10x.c:139-152)"""
    mask = (1 << bits) - 1
    t = np.zeros(1 << bits, dtype=np.uint32)
    for i in range(1, len(values)):
        h = int(values[i])
        off, diff = h & mask, ((h >> bits) & mask) | 1
        while t[off]:
            assert int(values[int(t[off])]) != h, "hash values of a state are distinct"
            off = (off + diff) & mask
        t[off] = i
    return t


def records(hashes, reads=None, labels=None):
    rec = np.zeros(len(hashes), dtype=orc.CLUSHASH)
    rec["hash"] = np.asarray(hashes, dtype=np.int64)
    if reads is not None:
        rec["read"] = np.asarray(reads, dtype=np.int64)
    if labels is not None:
        rec["subCluster"] = np.asarray(labels, dtype=np.int64)
    return rec


class State:
    """the members of a state by name, the genomes, the blocks"""

    def __init__(self, w=1, seed=3, rng=1):
        self.k, self.w, self.seed, self.B = K, w, seed, B
        self.rs = np.random.RandomState(rng)
        self.names, self._values = {}, [0]
        self.genome = ([], [])                               # sequences of genome A, of genome B: code arrays
        self.text = ({}, {})                                 # per genome {sequence number from 0: the FASTA text of a sequence written otherwise than in ACGT}
        self.blocks = []                                     # (records, nRead, nSubCluster, pointToMin) of codes 1 ..
        self.ranges = [(0, 0)]                               # the --clusterReport commands of the command line
        self.split = False                                   # --clusterSplit --cribSummary behind them
        self._h = None

    def hasher(self):
        return orc.Oracle(self.k, self.w, self.seed, self.B)

    @property
    def values(self):
        return np.array(self._values, dtype=np.uint64)

    def rand(self, n):
        return self.rs.randint(0, 4, n).astype(np.uint8)

    def hash_of(self, kmer):
        """the hash of one k-mer (it must be a mosh: any k-mer at w = 1)"""
        if self._h is None:
            self._h = self.hasher()
        hs, ps = self._h.mosh(np.asarray(kmer, dtype=np.uint8))
        assert len(kmer) == self.k and hs.size == 1 and ps[0] == 0
        return int(hs[0])

    def member(self, name, kmer=None, value=None):
        """a further hash index: the hash of a k-mer, or a value given outright"""
        v = self.hash_of(kmer) if value is None else value
        assert name not in self.names and v not in self._values[1:], "member %s: the value is in the state already" % name
        self._values.append(v)
        self.names[name] = len(self._values) - 1
        return self.names[name]

    def at(self, g, s, start):
        return self.genome[g][s][start:start + self.k]

    def seq(self, g, codes, text=None):
        self.genome[g].append(np.asarray(codes, dtype=np.uint8))
        if text is not None:
            self.text[g][len(self.genome[g]) - 1] = text
        return len(self.genome[g]) - 1

    def depth_blocks(self, depths=None, label=True):
        """block 1 holds every index once, all on read 0 and (label) in cluster 1; blocks 2 .. hold the indices that are to be deeper"""
        n = len(self._values)
        depths = depths or {}
        self.blocks.append((records(range(1, n), labels=[1 if label else 0] * (n - 1)), 1, 1 if label else 0, 0.5))
        for d in range(2, max(depths.values(), default=1) + 1):
            self.blocks.append((records([i for i, v in sorted(depths.items()) if v >= d]), 1, 0, 0.0))

    def image(self):
        return cs.image(self.blocks, B=self.B, values=self.values, table=probe_table(self.values, self.B))

    def fasta(self, g):
        out = []
        for i, s in enumerate(self.genome[g]):
            t = self.text[g].get(i)
            if t is None:
                t = np.frombuffer(b"ACGT", dtype=np.uint8)[s].tobytes().decode()
            out.append(">s%d\n" % (i + 1) + "".join(t[a:a + 60000] + "\n" for a in range(0, len(t), 60000)))
        return "".join(out)


Model = collections.namedtuple("Model", "a b crib reports summary words split_blocks split_summary split_words")
# a, b = add_genome's (chr, pos, known, unknown, count); crib = classify's; reports = cluster_report over codes 1 ..; summary / words of the file's
# blocks; the same after cluster_split where the case splits


Case = collections.namedtuple("Case", "name make text heavy")
CASES = collections.OrderedDict()


def case(name, text=True, heavy=False):
    def deco(f):
        assert name not in CASES
        CASES[name] = Case(name, f, text, heavy)
        return f
    return deco


@functools.lru_cache(maxsize=None)
def built(name):
    """(State, Model, the file's bytes) of a case, after the case's own check — made once per process"""
    st, where = CASES[name].make()
    a, b = cm.add_genome(st, st.genome[0]), cm.add_genome(st, st.genome[1])
    data = st.image()
    depth = orc.HashFile(data).hash_depth
    crib = cm.classify(a[:2], b[:2], depth)
    reports = cm.cluster_report(st.blocks, crib)
    summary, words = cm.crib_summary(st.blocks, crib.type), cm.crib_words(st.blocks, crib.type)
    sb = ss = sw = None
    if st.split:
        sb = cm.cluster_split(st.blocks)
        ss, sw = cm.crib_summary(sb, crib.type), cm.crib_words(sb, crib.type)
    m = Model(a, b, crib, reports, summary, words, sb, ss, sw)
    where(st, m)
    return st, m, data


def args(name, inp, fa, fb):
    """the command line of a case, for the reference binary and for bin/hash10x-amd"""
    st = built(name)[0]
    out = ["-k", st.k, "-w", st.w, "-r", st.seed, "-B", st.B, "--readHash", inp, "--tables", "--cribBuild", fa, fb, "--hashDepthRange", LO, HI]
    for a, b in st.ranges:
        out += ["--clusterReport", a, b]
    out += ["--cribSummary"]
    if st.split:
        out += ["--clusterSplit", "--cribSummary"]
    return [str(x) for x in out]


def model_text(name):
    """the lines cm.report keeps of the reference's stdout for args(name), from the model"""
    st, m, _ = built(name)
    out = []
    for g, r in enumerate((m.a, m.b)):
        out.append(cm.genome_line(r[2], r[3], len(st.genome[g])))
    out += cm.crib_lines(m.crib)
    for a, b in st.ranges:
        out += cm.report_lines(st.blocks, m.crib, LO, HI, a, b)
    out += cm.summary_lines(st.blocks, m.crib.type)
    if st.split:
        out += cm.summary_lines(m.split_blocks, m.crib.type)
    return out


def golden(name):
    """the recorded lines of the reference binary for args(name): tests/golden/crib/NAME.txt.gz (tests/golden/make_crib_golden.py)"""
    import os
    return orc.read_maybe_gz(os.path.join(orc.GOLDEN, "crib", name + ".txt.gz")).decode().splitlines()


def write_files(name, d):
    """NAME.hash, NAME.A.fa, NAME.B.fa in directory d; returns the three file names"""
    import os
    st, _, data = built(name)
    names = [name + ".hash", name + ".A.fa", name + ".B.fa"]
    with open(os.path.join(d, names[0]), "wb") as f:
        f.write(data)
    for g in range(2):
        with open(os.path.join(d, names[1 + g]), "w") as f:
            f.write(st.fasta(g))
    return names


def got(m, st, name):
    """(type, chr, pos, count in A, count in B) of a member"""
    i = st.names[name]
    return int(m.crib.type[i]), int(m.crib.chr[i]), int(m.crib.pos[i]), int(m.a[4][i]), int(m.b[4][i])


def each(m, st, expect):
    for name, e in expect.items():
        g = got(m, st, name)
        assert g == e, "%s: (type, chr, pos, nA, nB) = %r, built for %r" % (name, g, e)


# ------------------------------------------------------------------------------------------------ S1: sequence lengths and run seams
@case("S1_seams")
def _():
    st = State(rng=101)
    lens = [K - 1, K, K + 62, K + 63, 1, K - 1, K + 64, K + 127, K + 128, K + 200, 3]
    for n in lens:
        st.seq(0, st.rand(n))
    x = st.rand(K)                                           # genome A holds its reverse complement only
    st.genome[0][9][50:50 + K] = rc(x)
    spots = {"only_kmer": (1, 0), "last_slot62": (2, 62), "last_slot63": (3, 63), "run_end": (6, 63), "run_start_last": (6, 64), "first": (7, 0),
             "second_run_end_last": (7, 127), "r9_64": (8, 64), "r9_127": (8, 127), "r9_128_last": (8, 128)}
    for name, (s, p) in spots.items():
        st.member(name, st.at(0, s, p))
    st.member("rc_only", x)
    st.seq(1, st.rand(2))                                    # genome B: short sequences first and in the middle as well
    st.seq(1, st.genome[0][6].copy())
    st.seq(1, st.rand(K - 1))
    st.seq(1, st.rand(K + 64))
    st.member("b_run_start_last", st.at(1, 3, 64))
    st.member("b_run_end", st.at(1, 3, 63))
    st.member("nowhere", st.rand(K))
    st.depth_blocks()

    def where(st, m):
        e = {name: (cm.HTA, s + 1, 0, 1, 0) for name, (s, p) in spots.items()}
        e["run_end"] = e["run_start_last"] = (cm.HOM, 7, 0, 1, 1)
        e.update(rc_only=(cm.HTA, 10, 0, 1, 0), b_run_start_last=(cm.HTB, 4, 0, 0, 1), b_run_end=(cm.HTB, 4, 0, 0, 1), nowhere=(cm.ERR, 0, 0, 0, 0))
        each(m, st, e)
        assert st.hash_of(rc(x)) == st.hash_of(x) and not np.array_equal(rc(x), x)
        for s, p in spots.values():                          # the spots are what their names say
            assert p <= lens[s] - K
        assert [lens[s] - K for s in (1, 2, 3, 6, 7, 8)] == [0, 62, 63, 64, 127, 128] and RUN == 64
        assert m.a[2] == len(spots) + 1 and m.a[2] + m.a[3] == sum(max(n - K + 1, 0) for n in lens)
    return st, where


# ------------------------------------------------------------------------------------------------ S2: bin edges
@case("S2_bins")
def _():
    st = State(rng=102)
    st.seq(0, st.rand(65 * 1024 + K + 5))
    starts = {"a1023": 1023, "a1024": 1024, "a66559": 65 * 1024 - 1, "a66560": 65 * 1024}
    for name, p in starts.items():
        st.member(name, st.at(0, 0, p))
    st.seq(1, st.rand(5))
    st.seq(1, np.concatenate([st.rand(7), st.genome[0][0][:3000]]))      # the first two again, both in bin 1 of genome B: hom keeps genome A's position
    st.seq(1, st.rand(1100))
    st.member("b1023", st.at(1, 2, 1023))
    st.member("b1024", st.at(1, 2, 1024))
    st.depth_blocks()

    def where(st, m):
        each(m, st, {"a1023": (cm.HOM, 1, 0, 1, 1), "a1024": (cm.HOM, 1, 1, 1, 1), "a66559": (cm.HTA, 1, 64, 1, 0), "a66560": (cm.HTA, 1, 65, 1, 0),
                     "b1023": (cm.HTB, 3, 0, 0, 1), "b1024": (cm.HTB, 3, 1, 0, 1)})
        assert [int(m.b[1][st.names[n]]) for n in ("a1023", "a1024")] == [1, 1]
    return st, where


# ------------------------------------------------------------------------------------------------ S3: a sequence of more than 2^26 bases
@case("S3_long", heavy=True)
def _():
    st = State(rng=103)
    n = (1 << 26) + 3000
    s = np.ones(n, dtype=np.uint8)                           # C: its k-mer is no member
    stretch = st.rand(80)
    s[(1 << 26) - 30:(1 << 26) + 50] = stretch
    st.seq(0, s)
    st.member("last_bin", st.at(0, 0, (1 << 26) - 1))
    st.member("wrapped", st.at(0, 0, 1 << 26))
    st.seq(1, stretch[:50].copy())                           # k-mers 0 .. 29 of the stretch: the first member, not the second
    st.depth_blocks()

    def where(st, m):
        each(m, st, {"last_bin": (cm.HOM, 1, 65535, 1, 1), "wrapped": (cm.HTA, 1, 0, 1, 0)})
        assert m.a[2] == 2 and m.a[3] == n - K + 1 - 2 and st.hash_of(np.ones(K, dtype=np.uint8)) not in st.values.tolist()
    return st, where


# ------------------------------------------------------------------------------------------------ S4: occurrence counts and the 16-bit chr
def _run(st, unit, kmers, brk):
    """1100 random bases that end on base brk (which the run read backwards would not hold), then a run of the repeated unit with `kmers` k-mer starts"""
    pre = st.rand(1100)
    pre[-1] = brk
    n = kmers + K - 1
    return np.concatenate([pre, np.resize(np.asarray(unit, dtype=np.uint8), n)])


@case("S4_counts")
def _():
    st = State(rng=104)
    A, C, G, T = 0, 1, 2, 3
    runs = [((A,), 32769, G), ((C,), 32770, T), ((A, T), 32771, C), ((C, G), 65539, A), ((A, C), 65539, T), ((A, G), 5, T)]
    for unit, kmers, brk in runs:
        st.seq(0, _run(st, unit, kmers, brk))
    st.seq(0, st.rand(100))
    for name, s, p in (("polyA", 0, 1100), ("polyC", 1, 1100), ("AT", 2, 1100), ("CG", 3, 1100), ("ACA", 4, 1100), ("CAC", 4, 1101), ("AGA", 5, 1100), ("GAG", 5, 1101),
                       ("once", 6, 40), ("twice_b", 6, 41), ("thrice_b", 6, 42)):
        st.member(name, st.at(0, s, p))
    once = st.genome[0][6]
    st.seq(1, np.concatenate([st.rand(30), [A], np.resize([C, G], K), [A], st.rand(10)]))                       # CG once
    st.seq(1, np.concatenate([st.rand(30), [T], np.resize([A, C], K + 2), [T], st.rand(10)]))                   # ACA twice, CAC once
    st.seq(1, np.concatenate([st.rand(30), [G], np.resize([A], K + 1), [C], np.resize([A, G], K), [T]]))       # polyA twice, AGA once
    st.seq(1, np.concatenate([once[40:40 + K + 2], [(once[40] + 1) % 4], once[41:41 + K + 1], [(once[41] + 1) % 4], once[42:42 + K]]))   # (a base that does not restore the k-mer in front)
    n = len(st._values)
    # block 1: a cluster whose chromosome is the wrapped +32767 (polyC first, CG agrees with it), `once` disagrees; block 2: the rest, unlabelled
    first = [st.names[x] for x in ("polyA", "polyC", "CG", "once", "ACA")]
    st.blocks.append((records(first, reads=[0, 0, 1, 1, 2], labels=[1] * 5), 3, 1, 1.25))
    st.blocks.append((records([i for i in range(1, n) if i not in first]), 1, 0, 0.0))

    def where(st, m):
        each(m, st, {"polyA": (cm.MUL, -32768, 1, 32769, 2), "polyC": (cm.HTA, 32767, 1, 32770, 0), "AT": (cm.MUL, -1, 1, 32771, 0),
                     "CG": (cm.HOM, 32767, 1, 65539, 1), "ACA": (cm.MUL, -1, 1, 32770, 2), "CAC": (cm.MUL, -32768, 1, 32769, 1),
                     "AGA": (cm.MUL, -2, 1, 3, 1), "GAG": (cm.MUL, -1, 1, 2, 0), "once": (cm.HOM, 7, 0, 1, 1), "twice_b": (cm.MUL, -1, 0, 1, 2),
                     "thrice_b": (cm.MUL, -2, 0, 1, 3)})
        assert int(m.a[0][st.names["ACA"]]) == 32767 and int(m.a[0][st.names["CG"]]) == 32767       # genome A alone: the wrapped, positive chr
        c = m.reports[0]["clusters"][0]
        assert (c["chr"], c["nBad"], c["other"], c["nt"]) == (32767, 1, [st.names["once"]], [0, 1, 0, 2, 2])
    return st, where


@case("S4_value0_w31")
def _():
    """-w 31: A^k hashes to 0, which is a mosh for every w; 32770 of it in genome A (+32767), two in genome B (-1): mul with chr -1"""
    st = State(w=31, seed=17, rng=105)
    pre = st.rand(1100); pre[-1] = 2
    st.seq(0, np.concatenate([pre, np.zeros(32770 + K - 1, dtype=np.uint8)]))
    st.seq(1, np.concatenate([[1], np.zeros(K + 1, dtype=np.uint8), [1], pre[:600]]))
    h = st.hasher()
    hs, ps = h.mosh(pre)
    h.close()
    st.member("zero", value=0)
    for j in (0, 1, int(np.searchsorted(ps, 600))):
        st.member("mosh%d" % j, value=int(hs[j]))
    late = "mosh%d" % int(np.searchsorted(ps, 600))
    st.depth_blocks()

    def where(st, m):
        each(m, st, {"zero": (cm.MUL, -1, 1, 32770, 2)})
        assert int(m.a[0][st.names["zero"]]) == 32767 and got(m, st, "mosh0")[0] == cm.HOM and got(m, st, late)[0] == cm.HTA
        assert m.a[3] > 0 and m.a[2] == 32770 + 3
    return st, where


# ------------------------------------------------------------------------------------------------ S5: order under atomics
@case("S5_order")
def _():
    st = State(rng=106)
    s1, s2, s3 = st.rand(2500), st.rand(3200), st.rand(100)
    s1[2100:2100 + K] = s1[100:100 + K]
    s3[5:5 + K] = s2[3000:3000 + K]
    for s in (s1, s2, s3):
        st.seq(0, s)
    st.member("late_seq_low_pos", st.at(0, 2, 5))
    st.member("twice_in_one", st.at(0, 0, 100))
    st.member("plain", st.at(0, 1, 2048))
    st.seq(1, st.rand(30))
    st.depth_blocks()

    def where(st, m):
        each(m, st, {"late_seq_low_pos": (cm.MUL, -1, 2, 2, 0), "twice_in_one": (cm.MUL, -1, 0, 2, 0), "plain": (cm.HTA, 2, 2, 1, 0)})
    return st, where


# ------------------------------------------------------------------------------------------------ S6: the nine pairs of the two genomes
PAIRS = ((0, 0), (0, 1), (0, 3), (1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2), (2, 3), (2, 1), (1, 1), (0, 0), (0, 1))
DEPTHS = (300, 255, 1, 256, 256, 300, 1, 255, 300, 1, 256, 1, 1, 300)


def _pairs(drop=None):
    def make():
        st = State(rng=107)
        parts = ([st.rand(1500)], [st.rand(1100)])
        kmers = [st.rand(K) for _ in PAIRS]
        for q, mult in zip(kmers, PAIRS):
            for g in range(2):
                for _ in range(mult[g]):
                    parts[g].extend([q, st.rand(37)])
        st.seq(0, np.concatenate(parts[0]))
        st.seq(1, st.rand(K - 1))
        st.seq(1, np.concatenate(parts[1]))
        kept, depths = [], {}
        for j, (q, mult) in enumerate(zip(kmers, PAIRS)):
            t = "err" if mult == (0, 0) else "hom" if mult == (1, 1) else "mul" if max(mult) > 1 else "het"
            if t != drop:
                depths[st.member("p%d" % j, q)] = DEPTHS[j]
                kept.append(j)
        st.depth_blocks(depths)

        def chr_of(n, number):
            return 0 if n == 0 else number if n == 1 else -(n - 1)

        def where(st, m):
            for j in kept:
                na, nb = PAIRS[j]
                a, b = chr_of(na, 1), chr_of(nb, 2)
                t, c = got(m, st, "p%d" % j)[:2]
                if PAIRS[j] == (0, 0):
                    assert (t, c) == (cm.ERR, 0)
                elif PAIRS[j] == (1, 1):
                    assert (t, c) == (cm.HOM, 1)
                elif max(PAIRS[j]) > 1:
                    assert (t, c) == (cm.MUL, min(a, b) if b < a else a)
                else:
                    assert (t, c) == ((cm.HTA, 1) if na else (cm.HTB, 2))
                assert got(m, st, "p%d" % j)[3:] == PAIRS[j]
            if "p1" in st.names:                             # het from genome B comes with B's position: its sequence starts with 1100 bases of filler
                assert got(m, st, "p1")[2] == int(m.b[1][st.names["p1"]]) == 1 and int(m.a[1][st.names["p1"]]) == 0
            assert {(1, 2), (2, 3), (0, 3)} <= set(PAIRS)       # b < a among the mul pairs, and the other way round
            assert tuple(m.crib.array_max) == {None: (301, 301, 257, 301), "err": (0, 301, 257, 301), "hom": (301, 301, 0, 301)}[drop], m.crib.array_max
        return st, where
    return make


case("S6_pairs")(_pairs())
case("S6_no_hom")(_pairs("hom"))                             # "hom" and "err" of `crib matches` divide 0 by 0
case("S6_no_err")(_pairs("err"))


# ------------------------------------------------------------------------------------------------ S7: 32767 sequences
@case("S7_32767_sequences")
def _():
    st = State(rng=108)
    for _ in range(32767):
        st.seq(0, st.rand(K))
    st.member("in_last", st.genome[0][32766])
    st.member("in_first", st.genome[0][0])
    st.member("in_32766th", st.genome[0][32765])
    st.seq(1, st.rand(K + 3))
    st.depth_blocks()

    def where(st, m):
        each(m, st, {"in_last": (cm.HTA, 32767, 0, 1, 0), "in_first": (cm.HTA, 1, 0, 1, 0), "in_32766th": (cm.HTA, 32766, 0, 1, 0)})
        assert m.reports[0]["clusters"][0]["chr"] == 32767
    return st, where


# ------------------------------------------------------------------------------------------------ S8: N and lower case
@case("S8_n_and_lower_case")
def _():
    st = State(rng=109)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    s = st.rand(90)
    s[40 + 7] = 0                                            # an A of the member's k-mer is written N
    t = bytearray(letters[s].tobytes().lower())
    t[47:48] = b"N"
    st.seq(0, s, text=t.decode())
    s2 = st.rand(60)
    s2[[3, 30]] = 0
    t2 = bytearray(letters[s2].tobytes())
    t2[3:4] = b"n"; t2[30:31] = b"N"; t2[10:20] = bytes(t2[10:20]).lower()
    st.seq(1, s2, text=t2.decode())
    st.member("with_N", st.at(0, 0, 40))
    st.member("b_with_n", st.at(1, 0, 0))
    st.member("b_with_N_lower", st.at(1, 0, 12))
    st.depth_blocks()

    def where(st, m):
        each(m, st, {"with_N": (cm.HTA, 1, 0, 1, 0), "b_with_n": (cm.HTB, 1, 0, 0, 1), "b_with_N_lower": (cm.HTB, 1, 0, 0, 1)})
        assert "N" in st.fasta(0) and "n" in st.fasta(1) and st.fasta(0).splitlines()[1][:40].islower()
    return st, where


# ------------------------------------------------------------------------------------------------ the report cases: one pair of genomes, pools of members by class
def _pools(st):
    """three chromosomes in genome A, three in genome B; members by crib class and chromosome, each pool in the order of the positions"""
    r1, r2, r3, r4 = st.rand(2100), st.rand(2100), st.rand(600), st.rand(2100)
    for s in (r1, r2, np.concatenate([r3, r3[:100]])):
        st.seq(0, s)
    for s in (r1, r4, r2[:1000]):
        st.seq(1, s)
    spots = {"hom1": (0, 0, range(0, 2079, 3)), "hta2": (0, 1, range(1050, 2050, 50)), "hom2": (0, 1, range(0, 960, 50)), "htb2": (1, 1, range(0, 2000, 50)),
             "hta3": (0, 2, range(120, 520, 40)), "mul": (0, 2, range(0, 80, 10))}
    pool = {}
    for name, (g, s, starts) in spots.items():
        pool[name] = [st.member("%s_%d" % (name, p), st.at(g, s, p)) for p in starts]
    pool["err"] = [st.member("err_%d" % j, st.rand(K)) for j in range(30)]
    return pool


def _check_pools(st, m, pool):
    want = {"hom1": (cm.HOM, 1), "hta2": (cm.HTA, 2), "hom2": (cm.HOM, 2), "htb2": (cm.HTB, 2), "hta3": (cm.HTA, 3), "mul": (cm.MUL, -1), "err": (cm.ERR, 0)}
    for name, (t, c) in want.items():
        assert all(int(m.crib.type[i]) == t and int(m.crib.chr[i]) == c for i in pool[name]), name
    assert {int(m.crib.pos[i]) for i in pool["hom1"]} == {0, 1, 2}


def _mixed(pool, n, start=0):
    """n hash indices that cycle through the classes"""
    order = ("hom1", "err", "hta2", "mul", "htb2", "hom1", "hta3", "hom2")
    return [pool[order[(start + j) % 8]][((start + j) // 8) % len(pool[order[(start + j) % 8]])] for j in range(n)]


@case("R1_sizes")
def _():
    """blocks of 0, 1, 255, 256, 257 and 600 records; nRead 1, 256, 257; nSubCluster 0, 1, 255; labels above nSubCluster. The --clusterReport ranges of R5 run on
    this state: all, from 0, one block, up to the last block; MIN_POINT_DENSITY from the hand-set pointToMin."""
    st = State(rng=110)
    pool = _pools(st)
    st.blocks.append((records([]), 1, 0, 0.0))
    st.blocks.append((records(_mixed(pool, 1), labels=[1]), 1, 1, 0.75))
    st.blocks.append((records(_mixed(pool, 255, 3), reads=range(255), labels=range(1, 256)), 256, 255, 2.5))
    st.blocks.append((records(_mixed(pool, 256, 1), reads=range(256), labels=[1] * 256), 256, 1, 0.125))
    st.blocks.append((records(_mixed(pool, 257, 5), reads=range(257), labels=[1 + i % 255 for i in range(257)]), 257, 255, 1.0))
    lab = [(0, 1, 2, 3, 4, 200, 255)[i % 7] for i in range(600)]
    st.blocks.append((records(_mixed(pool, 600, 2), reads=[i % 257 for i in range(600)], labels=lab), 257, 3, 3.0))
    st.blocks.append((records(_mixed(pool, 40, 4), reads=[i % 5 for i in range(40)], labels=[(0, 7)[i % 2] for i in range(40)]), 5, 0, 0.5))
    st.ranges = [(0, 0), (0, 3), (4, 5), (5, 8)]

    def where(st, m):
        _check_pools(st, m, pool)
        assert [len(b[0]) for b in st.blocks] == [0, 1, 255, REP_THREADS, REP_THREADS + 1, 600, 40]
        r = m.reports
        assert r[5]["nClusHash"] == 600 - 86 and sum(c["n"] for c in r[5]["clusters"]) == 86 * 3 and len(r[5]["clusters"]) == 3
        assert r[6]["nClusHash"] == 20 and r[6]["nClusRead"] == 5 and r[6]["clusters"] == []
        assert all(c["n"] == 1 for c in r[2]["clusters"]) and r[4]["clusters"][0]["n"] == 2 and r[4]["clusters"][2]["n"] == 1
    return st, where


@case("R2_read_labels")
def _():
    """a read whose records carry the labels 2, 1, 0 in that order (the result is 1); a read without a labelled record; a read in records 255 and 256"""
    st = State(rng=111)
    pool = _pools(st)
    n = 300
    reads, lab = [i % 4 for i in range(n)], [3] * n
    for i, l in ((10, 2), (20, 1), (30, 0)):
        reads[i], lab[i] = 5, l
    for i in (40, 50, 270):
        reads[i], lab[i] = 6, 0
    reads[255], lab[255] = 7, 1
    reads[256], lab[256] = 7, 2
    st.blocks.append((records(_mixed(pool, n), reads=reads, labels=lab), 9, 3, 1.0))

    def where(st, m):
        _check_pools(st, m, pool)
        c = m.reports[0]["clusters"]
        assert [x["nRead"] for x in c] == [1, 1, 4] and [x["n"] for x in c] == [2, 2, n - 8] and m.reports[0]["nClusRead"] == 6
    return st, where


@case("R3_first_located")
def _():
    st = State(rng=112)
    pool = _pools(st)
    p = pool
    blocks = [
        [p["hom1"][690], p["hom1"][0], p["hta2"][0], p["hom1"][350]],                                          # located at record 0; hom; positions 2, 0, 1
        [p["err"][0], p["mul"][0]] * 5 + [p["hta2"][3], p["hom1"][1], p["hta2"][19], p["hom2"][2], p["htb2"][30]],   # late, behind err / mul; htA; hom2 and htb2 share its chromosome
        [p["err"][1], p["htb2"][25], p["hta2"][0], p["hom1"][5], p["htb2"][0]],                                # htB
    ]
    for hs in blocks:
        st.blocks.append((records(hs, reads=range(len(hs)), labels=[1] * len(hs)), len(hs), 1, 0.0))
    # two labels: label 2's first located record stands before label 1's
    hs = [p["err"][2], p["hom1"][9], p["mul"][1], p["hta3"][0], p["hta3"][1], p["hom1"][10]]
    st.blocks.append((records(hs, reads=range(6), labels=[1, 2, 1, 1, 2, 1]), 6, 2, 0.0))

    def where(st, m):
        _check_pools(st, m, pool)
        c = [b["clusters"] for b in m.reports]
        assert (c[0][0]["chr"], c[0][0]["pMin"], c[0][0]["pMax"], c[0][0]["nBad"]) == (1, 0, 2, 1)
        assert (c[1][0]["chr"], c[1][0]["nBad"], c[1][0]["nt"]) == (2, 1, [5, 2, 1, 2, 5]) and c[1][0]["pMin"] == 0
        assert (c[2][0]["chr"], c[2][0]["nBad"]) == (2, 1) and int(m.crib.type[blocks[2][1]]) == cm.HTB
        assert (c[3][0]["chr"], c[3][0]["nBad"], c[3][1]["chr"], c[3][1]["nBad"]) == (3, 1, 1, 1)
    return st, where


NBAD = (0, 1, 10, 11, 25)


@case("R4_other_lists")
def _():
    """five labels whose records alternate through a block of 600: 0, 1, 10, 11 and 25 disagreeing hashes, spread over the strides of 256"""
    st = State(rng=113)
    pool = _pools(st)
    per = 120
    hs, lab = [0] * (5 * per), [0] * (5 * per)
    for l, nb in enumerate(NBAD):
        bad_at = set(np.linspace(3, per - 1, nb).astype(int).tolist()) if nb else set()
        assert len(bad_at) == nb
        other = pool["hta2"] + pool["hta3"] + pool["htb2"]
        k = 0
        for j in range(per):
            e = j * 5 + l
            lab[e] = l + 1
            if j in bad_at:
                hs[e] = other[(k + 7 * l) % len(other)]; k += 1
            elif j % 4 == 1:
                hs[e] = (pool["err"] + pool["mul"])[(j + l) % 38]
            else:
                hs[e] = pool["hom1"][(j * 5 + l) % len(pool["hom1"])]
    st.blocks.append((records(hs, reads=[e % 50 for e in range(600)], labels=lab), 50, 5, 4.0))

    def where(st, m):
        _check_pools(st, m, pool)
        c = m.reports[0]["clusters"]
        assert [x["nBad"] for x in c] == list(NBAD) and [len(x["other"]) for x in c] == [0, 1, 10, 10, 10] and all(x["chr"] == 1 for x in c)
        entries = [e for e in range(600) if lab[e] == 5 and int(m.crib.chr[hs[e]]) not in (0, 1, -1)]
        assert c[4]["other"] == [hs[e] for e in sorted(entries, reverse=True)[:10]] and len(entries) == 25
        assert min(entries) < REP_THREADS < 2 * REP_THREADS < max(entries)
    return st, where


@case("R6_split")
def _():
    """a state --clusterSplit can take (no label above nSubCluster): --cribSummary before and after it"""
    st = State(rng=114)
    pool = _pools(st)
    st.blocks.append((records(_mixed(pool, 70), reads=[i % 9 for i in range(70)], labels=[(0, 1, 2, 1)[i % 9 % 4] for i in range(70)]), 9, 2, 1.0))
    st.blocks.append((records(_mixed(pool, 30, 3), reads=[0] * 30), 1, 0, 0.0))
    st.blocks.append((records(_mixed(pool, 33, 5), reads=[i % 3 for i in range(33)], labels=[(1, 0, 1)[i % 3] for i in range(33)]), 3, 1, 0.5))
    st.split = True

    def where(st, m):
        _check_pools(st, m, pool)
        assert m.summary[2:4] == (4, 0) and m.split_summary[2:4] == (4, 3) and [b[4] for b in m.split_blocks] == [0, 0, 0, 2, 2, 4]
        assert sum(m.split_summary[0]) + sum(m.split_summary[1]) == 133 and sum(m.split_summary[1]) == sum(1 for b in st.blocks for l in b[0]["subCluster"] if l)
    return st, where
