"""Scripted states for --seqSpans, shared by test_seq_spans_cpu.py and test_seq_spans_gpu.py. Random sequences; the oracle lists their moshes as
(value, position); those values become the state's hashValue[] (with the probe table that finds them) and a script says which blocks hold which of
them, so that every edge of the definition lies where its case says. One state holds all cases: a case is the sequences it names, the parameters it
runs at and the claim it asserts from the model. k = 21, w = 31, seed 17."""
import numpy as np

import cluster_states
import crib_cases
import orc
import seqblocks_model as sbm
import seqspans_model as ssm

K, W, R = 21, 31, 17
RANGE = (1, 400)                                               # a hash counts when 1 .. 399 records hold it
HEAVY_RECORDS = 65540                                          # the block of more than 65535 records (test_seq_blocks_gpu.py's hand-made state)

_oracle = []


def moshes(seq):
    if not _oracle:
        _oracle.append(orc.Oracle(k=K, w=W, seed=R, B=20))
    hs, ps = _oracle[0].mosh(np.asarray(seq, dtype=np.uint8))
    return [int(v) for v in hs], [int(p) for p in ps]


def random_seq(n, seed):
    return np.random.RandomState(seed).randint(0, 4, n).astype(np.uint8)


def trimmed(n, seed):
    """a random sequence cut so that its first mosh starts at position 0 and its last at L - k"""
    s = random_seq(n, seed)
    _, ps = moshes(s)
    order = sorted(ps)
    out = s[order[0]:order[-1] + K].copy()
    got = sorted(moshes(out)[1])
    assert got[0] == 0 and got[-1] == len(out) - K
    return out


def with_unit_gap(n, seed0):
    """the first random sequence (seeds seed0, seed0 + 1, ..) two of whose neighbouring moshes start one base apart"""
    for seed in range(seed0, seed0 + 400):
        s = random_seq(n, seed)
        ps = sorted(moshes(s)[1])
        if 1 in np.diff(ps).tolist():
            return s
    raise AssertionError("no sequence with two moshes one base apart")


class Script:
    """sequences by name, their occurrences in position order, and which block holds which hash how often"""

    def __init__(self):
        self.names, self.seqs, self.occ = [], {}, {}          # occ[name] = [(position, value)] ascending in position
        self.values = [0]                                      # hashValue[]: slot 0 unused
        self.index = {}
        self.holds = {}                                        # block -> [hash index, ..]

    def add(self, name, seq):
        hs, ps = moshes(seq)
        self.names.append(name); self.seqs[name] = seq
        self.occ[name] = sorted(zip(ps, hs))
        return self.occ[name]

    def x(self, value):
        if value not in self.index:
            self.index[value] = len(self.values); self.values.append(value)
        return self.index[value]

    def hold(self, block, name, which, times=1):
        """block holds the hashes of occurrences `which` (indices in position order) of sequence `name`, `times` records each"""
        for i in which:
            self.holds.setdefault(block, []).extend([self.x(self.occ[name][i][1])] * times)

    def pos(self, name, i):
        return self.occ[name][i][0]

    def image(self):
        n_blocks = max(self.holds)
        heavy = self.holds[n_blocks]
        base = len(self.values)
        filler = [31 * ((1 << 40) + i) for i in range(HEAVY_RECORDS - len(heavy))]     # values no sequence has
        assert not set(filler) & set(self.values)
        values = np.array(self.values + filler, dtype=np.uint64)
        blocks = []
        for b in range(1, n_blocks + 1):
            h = list(self.holds.get(b, []))
            if b == n_blocks:
                h += list(range(base, base + len(filler)))
            blocks.append((crib_cases.records(h), 1, 0, 0.0))
        return cluster_states.image(blocks, B=20, values=values, table=crib_cases.probe_table(values, 20)), values


# the blocks of the script
(B_GAP, B_ENDS, B_UNIT, B_T3, B_T4, B_SPLIT, B_LONE, B_TWICE, B_257, B_64, B_65, B_256, B_257D, B_DEEP, B_DUP, B_EDGE, B_NEIGH, B_COVER,
 B_HEAVY) = range(1, 20)

_built = []


def script():
    """the one scripted state: (Script, image bytes, model)"""
    if _built:
        return _built[0]
    z = Script()
    main = z.add("main", with_unit_gap(3001, 100))             # L = 2 W + 1 at W = 1500
    assert len(main) > 70
    z.hold(B_GAP, "main", (4, 5))                              # two hits G apart / G + 1 apart, by the choice of G
    z.hold(B_ENDS, "main", (0, len(main) - 1))                 # G = 0 with hits at both ends: one extent
    d = np.diff([p for p, _ in main]).tolist()
    u = d.index(1)
    assert 0 < u < len(main) - 2 and d[u + 1] > 1
    z.hold(B_UNIT, "main", (u, u + 1, u + 2))                  # G = 1: {u, u + 1} stay together, u + 2 is its own extent
    z.hold(B_T3, "main", (10, 11, 12)); z.hold(B_T4, "main", (20, 21, 22, 23))   # T = 4: T - 1 and T hits
    z.hold(B_SPLIT, "main", (30, 31, 32, 33, 60))              # one kept and one dropped extent at T = 2 and a gap between the inner and the outer distance
    z.hold(B_TWICE, "main", (40,), times=2)                    # two hits at one position
    z.hold(B_257, "main", (41,), times=257)                    # 257 equal keys
    lone = z.add("lone", random_seq(600, 7))
    z.hold(B_LONE, "lone", (1,))                               # a row with no kept extent at T = 2
    long_ = z.add("long", random_seq(9500, 11))
    assert len(long_) >= 257
    for b, n in ((B_64, 64), (B_65, 65), (B_256, 256), (B_257D, 257)):
        z.hold(b, "long", range(n))                            # extents of exactly 64, 65, 256 and 257 hits at distinct positions
    deep = z.add("deep", random_seq(300, 13))
    assert deep
    z.hold(B_DEEP, "deep", (0,), times=RANGE[1])               # found, and held by too many records: no counting occurrence
    r = random_seq(1500, 17)
    dup = z.add("dup", np.concatenate([r, r[200:500]]))       # a duplicated segment: the same hash at two positions
    twice = [i for i, (p, v) in enumerate(dup) if [w for _, w in dup].count(v) == 2 and p < 1500]
    assert twice
    z.dup = (twice[0], [i for i, (_, v) in enumerate(dup) if v == dup[twice[0]][1]][1])
    z.hold(B_DUP, "dup", (twice[0],))
    e1 = z.add("edge1", trimmed(900, 19))                      # hits at position 0 and at L - k
    z.hold(B_EDGE, "edge1", (0, len(e1) - 1))
    z.hold(B_NEIGH, "edge1", (len(e1) - 1,))                   # the block's last hit in edge1 ..
    z.add("empty", random_seq(0, 1)); z.add("k-1", random_seq(K - 1, 2)); z.add("k", random_seq(K, 3))
    assert not z.occ["empty"] and not z.occ["k-1"]
    e2 = z.add("edge2", trimmed(900, 23))
    z.hold(B_NEIGH, "edge2", (0,))                             # .. and its first in edge2: 3 k - 1 apart in slab ordinals
    assert len(e2) > 3
    cov = z.add("cover", random_seq(2000, 29))                 # one block, one extent: from occurrence 2 to occurrence 9
    z.hold(B_COVER, "cover", (2, 9))
    assert len(cov) > 9 and z.pos("cover", 2) >= 1
    z.add("absent", random_seq(700, 31))                       # moshes, none of them in the state
    z.hold(B_HEAVY, "main", (50, 51))
    data, values = z.image()
    hf = orc.HashFile(data)
    model = ssm.SeqSpansModel(sbm.SeqBlocksModel.from_hash_file(hf, [RANGE], K, W, R))
    _built.append((z, data, model))
    return _built[0]


def sequences(z):
    return [z.seqs[n] for n in z.names]


def gap_of(z, name, i):
    return z.pos(name, i + 1) - z.pos(name, i)


def params(z):
    """every (T, G, W) a case runs at"""
    g = gap_of(z, "main", 4)
    inner = max(gap_of(z, "main", i) for i in (30, 31, 32))
    d2 = z.pos("dup", z.dup[1]) - z.pos("dup", z.dup[0])
    f, l = z.pos("cover", 2), z.pos("cover", 9)
    out = [(1, 0, 0), (1, g, 0), (1, g - 1, 0), (1, 1, 0), (4, 0, 0), (2, inner, 1000), (1, d2 - 1, 0), (1, d2, 0), (1, 100, 0), (2, 0, 700),
           (257, 0, 0), (258, 0, 0), (64, 40, 0), (2 ** 31 - 1, 0, 100)]
    out += [(1, 0, w) for w in (f + 1, f, l, l + 1, 2000, 1999, 1000, 1500, 1, 10 ** 6)]
    return out
