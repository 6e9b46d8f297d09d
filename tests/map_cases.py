"""Scripted seed streams at the edges of the moshmap block walk (rm_block_kernel, csrc/stage_i.hip; queryProcess, moshmap.c:211-272), and the
registry of cases the CPU and the GPU tests run (test_moshmap_blocks_cpu.py, test_moshmap_blocks_gpu.py).

What a seed gives the walk is its copy class, `loc` (the first hit ordinal of its set index), `loc2` / `id2` for copy 2 and `id[loc]`. In a
hand-built reference all of these are the caller's: a case is a random query (its moshes come from the model hasher, mosh_model.MoshModel.moshes)
and a script with one entry per mosh of the query, in order:

    None             the set does not hold it (a miss)
    ('M',)           a multi-copy seed
    (1, loc)         copy 1 on hit ordinal loc
    (2, loc, loc2)   copy 2, loc < loc2

build() puts the scripted hashes into a set (-B 20 -K 19 -W 31 -S 17) and lays the hit arrays of a reference out so that RefModel.pack() derives
exactly the scripted classes and locs: index[loc] = the seed's set index at the scripted ordinals, one filler index (a hash no query holds) on
every other hit, id[h] = h // SEQ and offset[h] = (h % SEQ) * 31. Every case owns R = 3 * SEQ hit ordinals, that is three reference sequences
"a", "b" and "c"; a script names them by LOCAL ordinals 0 .. R - 1 (a: 0 .. 999, b: 1000 .. 1999, c: 2000 .. 2999). Hit 0 of the reference
opens no block, so the case that scripts local ordinal 0 is the first of its group, and each hit-0 case has a group (a set and a reference)
of its own. The three hits a copy-M seed needs lie behind the last case's range.

blocks() restates the walk over integers, apart from RefModel.query, which formats text; VARIANTS are the wrong walks a change to the kernel
would plausibly make, and CATCHES names a case that tells each from the right one.

Every case states what the reference prints for it: `expect`, the (n1, n2) of its M records in order, and `starts`, the local ordinal each
record's block began on. tests/golden/make_map_blocks_golden.py refuses a fixture in which the reference's own lines say otherwise.

TEST INFRASTRUCTURE — plain Python and numpy, never imported by hash10x_amd/."""
import collections
import zlib

import numpy as np

import map_model as mp
import mosh_model as mm

B, K, W, SEED = 20, 19, 31, 17
SEQ = 1000                                                   # hit ordinals per reference sequence
R = 3 * SEQ                                                  # hit ordinals per case
QLEN = 12000                                                 # bases of a query: 12000 / 31, some 390 moshes
TILE = 64                                                    # seeds rm_block_kernel stages at a time: consecutive seed ordinals, misses and copy M included
M32 = 0xFFFFFFFF
A0, B0, C0 = 0, SEQ, 2 * SEQ                                 # the first local ordinal of the case's three sequences
FILLER_SEED = 999331                                         # rng of the sequence the filler hash is taken from


class Sc:
    """a script under construction"""

    def __init__(self):
        self.e = []

    def miss(self, n=1):
        self.e += [None] * n
        return self

    def multi(self, n=1):
        self.e += [("M",)] * n
        return self

    def gap(self, n):
        """n seeds that do not qualify, misses and copy-M seeds in turn"""
        self.e += [None if j & 1 else ("M",) for j in range(n)]
        return self

    def one(self, *locs):
        self.e += [(1, l) for l in locs]
        return self

    def run(self, start, n, step=1):
        return self.one(*[start + step * j for j in range(n)])

    def two(self, loc, loc2):
        assert loc < loc2
        self.e.append((2, loc, loc2))
        return self

    def upto(self, i):
        """misses until the next entry is seed ordinal i"""
        assert len(self.e) <= i
        return self.miss(i - len(self.e))


Case = collections.namedtuple("Case", "name family script expect starts kind cut repeat group")


def case(name, family, sc, expect, starts=None, kind="random", cut=None, repeat=None, group="x"):
    assert starts is None or len(starts) == len(expect)
    return Case(name, family, list(sc.e) if sc else None, [tuple(p) for p in expect], starts, kind, cut, repeat, group)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
def _cases():
    out = []
    add = lambda *a, **k: out.append(case(*a, **k))

    # -- hit 0 (each first in a group of its own: local ordinal 0 is hit 0 of that reference) ------------------------------------------------
    # a copy-1 seed on hit 0 opens nothing: the block of 0, 1, 2, 3, 4 starts on hit 1
    add("hit0_first_seed", "hit0", Sc().run(0, 5).one(C0 + 7), [(4, 0)], [1])
    # copy 2 with first loc 0 while no block is open: no retry (its second loc, on another sequence, would open a block), the next seed opens it
    add("hit0_copy2_no_retry", "hit0", Sc().two(0, B0 + 5).run(B0 + 6, 3).one(C0 + 7), [(3, 0)], [B0 + 6], group="h2")
    # a descending block may arrive at hit 0; the forward step behind it ends it like any other
    add("hit0_descending_arrives", "hit0", Sc().run(3, 4, -1).run(10, 3, -1).one(C0 + 7), [(4, 0), (3, 0)], [3, 10], group="h3")

    # -- drift thresholds: 49 and 50 keep the block, 51 ends it at the seed behind the one that brought the drift -------------------------------
    for d in (49, 50, 51):
        exp, two = ([(10, 0)], d > 50) if d <= 50 else ([(6, 0), (4, 0)], True)
        # d > 0: the hit ordinals jump by d more than the seed ordinals
        add("drift_asc_pos_%d" % d, "drift", Sc().run(10, 5).run(15 + d, 5).one(C0 + 7), exp, [10, 16 + d] if two else [10])
        add("drift_desc_pos_%d" % d, "drift", Sc().run(900, 5, -1).run(895 - d, 5, -1).one(C0 + 7), exp, [900, 894 - d] if two else [900])
        # d < 0: d seeds that do not qualify (misses and copy M in turn) between consecutive hits
        add("drift_asc_neg_%d" % d, "drift", Sc().run(10, 5).gap(d).run(15, 5).one(C0 + 7), exp, [10, 16] if two else [10])
        add("drift_desc_neg_%d" % d, "drift", Sc().run(900, 5, -1).gap(d).run(895, 5, -1).one(C0 + 7), exp, [900, 894] if two else [900])

    # -- direction -----------------------------------------------------------------------------------------------------------------------------
    # the second seed makes the block descending: 30 is then a forward step and ends it
    add("dir_second_seed_decides", "direction", Sc().one(10, 9, 8, 7).run(30, 3, -1).one(C0 + 7), [(4, 0), (3, 0)], [10, 30])
    add("dir_backwards_ends_ascending", "direction", Sc().run(10, 4).run(5, 4).one(C0 + 7), [(4, 0), (4, 0)], [10, 5])
    add("dir_forwards_ends_descending", "direction", Sc().run(500, 4, -1).run(600, 4, -1).one(C0 + 7), [(4, 0), (4, 0)], [500, 600])
    # a forward jump of 27 in an ascending block (a backward one in a descending block) is drift, not direction
    add("dir_forward_jump_stays", "direction", Sc().run(10, 3).run(40, 3).one(C0 + 7), [(6, 0)], [10])
    add("dir_backward_jump_stays_descending", "direction", Sc().run(500, 3, -1).run(470, 3, -1).one(C0 + 7), [(6, 0)], [500])
    # the same mosh twice in a row (the query repeats a k-mer): loc == locN is no backwards step
    add("dir_equal_loc_stays", "direction", None, [(6, 0)], [10], repeat=True)

    # -- sequence change: the id ends the block, whatever the loc -------------------------------------------------------------------------------
    add("seq_change_up", "sequence", Sc().run(10, 3).run(B0 + 13, 3).one(C0 + 7), [(3, 0), (3, 0)], [10, B0 + 13])
    add("seq_change_down", "sequence", Sc().run(B0 + 10, 3).run(13, 3).one(C0 + 7), [(3, 0), (3, 0)], [B0 + 10, 13])

    # -- the second loc of a copy-2 seed --------------------------------------------------------------------------------------------------------
    # first loc backwards, second the next hit: the block goes on
    add("retry_ascending", "retry", Sc().run(10, 3).two(5, 13).one(14, 15).one(C0 + 7), [(5, 1)], [10])
    # in a descending block the first loc (the smaller) can only end it by its sequence
    add("retry_descending", "retry", Sc().run(B0 + 500, 3, -1).two(20, B0 + 497).one(B0 + 496, B0 + 495).one(C0 + 7), [(5, 1)], [B0 + 500])
    # both backwards: the new block opens on the SECOND loc
    add("retry_both_end", "retry", Sc().run(10, 3).two(3, 5).run(6, 3).one(C0 + 7), [(3, 0), (3, 1)], [10, 5])
    # second loc on another sequence: the new block opens there, with id2, and the seeds behind it continue it
    add("retry_second_other_sequence", "retry", Sc().run(10, 3).two(3, B0 + 5).run(B0 + 6, 3).one(C0 + 7), [(3, 0), (3, 1)], [10, B0 + 5])
    # first loc continues: the second (which would jump by 60) is not looked at
    add("retry_first_continues", "retry", Sc().run(10, 3).two(13, 74).run(14, 6).one(C0 + 7), [(9, 1)], [10])

    # -- flushes: every flush but the closing one tests n1 > 2, the closing one n2 > 2 ------------------------------------------------------------
    add("flush_final_2_3", "flush", Sc().miss(3).one(10, 11).two(12, C0 + 1).two(13, C0 + 2).two(14, C0 + 3), [(2, 3)], [10])
    add("flush_2_3_then_elsewhere", "flush", Sc().miss(3).one(10, 11).two(12, C0 + 1).two(13, C0 + 2).two(14, C0 + 3).one(B0 + 7), [], [])
    add("flush_final_5_2", "flush", Sc().run(10, 5).two(15, C0 + 1).two(16, C0 + 2), [], [])
    add("flush_copy2_only", "flush", Sc().two(10, C0 + 1).two(11, C0 + 2).two(12, C0 + 3).two(13, C0 + 4), [(0, 4)], [10])

    # -- tiles: an event on the last seeds of a tile and the first of the next ----------------------------------------------------------------------
    for p in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130):
        # seed p ends the block by the drift seed p - 1 brought
        add("tile_drift_%d" % p, "tile", Sc().run(10, p - 1).run(10 + p - 1 + 51, 11).one(C0 + 7), [(p, 0), (10, 0)], [10, 10 + p + 51])
        add("tile_sequence_%d" % p, "tile", Sc().run(10, p).run(B0 + 10, 10).one(C0 + 7), [(p, 0), (10, 0)], [10, B0 + 10])
        add("tile_second_loc_%d" % p, "tile", Sc().run(10, p).two(3, 10 + p).run(11 + p, 10).one(C0 + 7), [(p + 10, 1)], [10])
    add("tile_block_of_200", "tile", Sc().run(10, 200).one(C0 + 7), [(200, 0)], [10])
    # seeds 60 .. 199 do not qualify (all of tile 64 .. 127): with the hits jumping as far d stays 0, without it is -140
    add("tile_empty_compensated", "tile", Sc().run(10, 60).gap(140).run(210, 10).one(C0 + 7), [(70, 0)], [10])
    add("tile_empty_drifts", "tile", Sc().run(10, 60).gap(140).run(70, 10).one(C0 + 7), [(61, 0), (9, 0)], [10, 71])
    # the query ends behind its 64th, 65th, 128th mosh, in a block only the closing flush writes
    for n in (64, 65, 128):
        add("tile_cut_%d" % n, "tile", Sc().run(10, n - 3).two(B0 + 1, C0 + 1).two(B0 + 2, C0 + 2).two(B0 + 3, C0 + 3), [(n - 3, 0), (0, 3)], [10, C0 + 1], cut=n)

    # -- record room: 71 records (more than one pass of rm_compact_kernel's 64 lanes) against a bound of (210 + 3) / 3 + 1 = 72 ------------------------
    sc = Sc()
    for j in range(70):
        sc.run(900 - 10 * j, 3)                                   # each block a backwards step from the one before
    sc.two(B0 + 1, C0 + 1).two(B0 + 2, C0 + 2).two(B0 + 3, C0 + 3)
    add("room_71_records", "room", sc, [(3, 0)] * 70 + [(0, 3)], [900 - 10 * j for j in range(70)] + [C0 + 1])

    # -- nothing to walk ----------------------------------------------------------------------------------------------------------------------------
    add("none_shorter_than_k", "nothing", Sc(), [], [], kind="short")
    add("none_no_mosh_in_set", "nothing", Sc(), [], [])
    add("none_copyM_only", "nothing", Sc(), [], [], kind="allM")
    add("none_empty", "nothing", Sc(), [], [], kind="empty")        # last: both loops of moshmap stop reading at a sequence without bases
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GROUPS = collections.OrderedDict((g, [c for c in CASES if c.group == g]) for g in ("x", "h2", "h3"))
FAMILIES = ("hit0", "drift", "direction", "sequence", "retry", "flush", "tile", "room", "nothing")
assert sum(c.family == "drift" for c in CASES) == 12 and {c.family for c in CASES} == set(FAMILIES)


# ---- the builder --------------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def query_codes(ms, c):
    """(codes, script) of a case: a random query of QLEN bases, cut or with one k-mer repeated where the case asks for it"""
    rs = _rng(c.name)
    if c.kind == "empty":
        return np.zeros(0, np.uint8), []
    if c.kind == "short":
        return rs.randint(0, 4, 12).astype(np.uint8), []
    s = rs.randint(0, 4, QLEN).astype(np.uint8)
    script = c.script
    if c.repeat:
        # s[:p + K] + s[p:] holds the k-mer of mosh j twice; the first j at which no mosh arises on the seam makes seeds j and j + 1 the same mosh.
        # Script: an ascending block 10, 11, 12, [12], 13, 14 whose fourth seed is that repeat
        _, ps = ms.moshes(s)
        for j in range(3, len(ps)):
            t = np.concatenate([s[:int(ps[j]) + K], s[int(ps[j]):]])
            hs, _ = ms.moshes(t)
            if hs[j] == hs[j + 1]:
                break
        else:
            raise AssertionError("no mosh of the query repeats without a mosh on the seam")
        s = t
        script = Sc().upto(j - 2).run(10, 3).one(12).one(13, 14).one(C0 + 7).e
    if c.cut:
        _, ps = ms.moshes(s)
        s = s[:int(ps[c.cut - 1]) + K]
    if c.kind == "allM":
        script = [("M",)] * len(ms.moshes(s)[0])
    return s, script


def bases(cases):
    """{case name: its first hit ordinal}: the case that scripts local ordinal 0 comes first, the others follow in order"""
    first = [c for c in cases if any(e and e[0] in (1, 2) and 0 in e[1:] for e in (c.script or []))]
    assert len(first) <= 1, "hit 0 can be scripted once in a reference"
    return {c.name: R * n for n, c in enumerate(first + [c for c in cases if c not in first])}


def build(cases):
    """(MoshModel, RefModel, [query codes], [script]) for several queries over one set and one reference. The scripts come back per mosh of their
    query (padded with misses) and in GLOBAL hit ordinals."""
    ms = mm.MoshModel(B, K, W, SEED)
    base = bases(cases)
    at, multi, seen = {}, [], {}                                 # hit ordinal -> set index; the copy-M indices; hash -> (case, seed)
    queries, scripts = [], []
    for c in cases:
        s, local = query_codes(ms, c)
        hs, _ = ms.moshes(s)
        assert len(local) <= len(hs), "%s: %d entries for %d moshes" % (c.name, len(local), len(hs))
        if c.cut:
            assert len(hs) == c.cut
        script = []
        for i, h in enumerate(int(h) for h in hs):
            e = local[i] if i < len(local) else None
            if e is not None and e[0] != "M":
                assert all(0 <= l < R for l in e[1:])
                e = (e[0],) + tuple(base[c.name] + l for l in e[1:])
            if h in seen:                                        # the one repeat a case asks for; every other mosh of every query is distinct
                assert c.repeat and seen[h] == (c.name, i - 1) and e == script[i - 1], "%s: mosh %d is mosh %d of %s" % ((c.name, i) + seen[h][::-1])
                script.append(e)
                continue
            seen[h] = (c.name, i)
            script.append(e)
            if e is None:
                continue
            ix = ms._find_add(h)
            if e[0] == "M":
                multi.append(ix)
                continue
            for l in e[1:]:
                assert l not in at, "%s: hit ordinal %d is scripted twice" % (c.name, l)
                at[l] = ix
        queries.append(s)
        scripts.append(script)
    fh, _ = ms.moshes(np.random.RandomState(FILLER_SEED).randint(0, 4, 2000).astype(np.uint8))
    assert int(fh[0]) not in seen
    filler = ms._find_add(int(fh[0]))
    nh = R * len(cases) + 3 * len(multi)
    nh += -nh % SEQ
    ref = mp.RefModel(ms, nh)
    ref.index = [filler] * nh
    for l, ix in at.items():
        ref.index[l] = ix
    for j, ix in enumerate(multi):
        for t in range(3):
            ref.index[R * len(cases) + 3 * j + t] = ix
    ref.offset = [(h % SEQ) * W for h in range(nh)]
    ref.id = [h // SEQ for h in range(nh)]
    ref.depth = dict(collections.Counter(ref.index))
    assert ref.depth[filler] > 2
    for i in range(nh // SEQ):
        ref.dict.add("s%d" % i)
        ref.len.append(SEQ * W + K)
    ref.len_dim = mp.array_dim_after(len(ref.len))
    ref.pack()
    for c, s, script in zip(cases, queries, scripts):            # every scripted class and loc comes out of pack() as scripted
        got = seeds_of(ms, ref, s)
        assert got == expected_seeds(script), "%s: pack() does not give the scripted seeds" % c.name
    return ms, ref, queries, scripts


def expected_seeds(script):
    """(class, loc, loc2, id, id2) per seed as the script has it: class 0 a miss, 3 copy M"""
    out = []
    for e in script:
        if e is None:
            out.append((0, 0, 0, 0, 0))
        elif e[0] == "M":
            out.append((3, 0, 0, 0, 0))
        elif e[0] == 1:
            out.append((1, e[1], 0, e[1] // SEQ, 0))
        else:
            out.append((2, e[1], e[2], e[1] // SEQ, e[2] // SEQ))
    return out


def seeds_of(ms, ref, s):
    """the same from the packed reference: what rm_seed_kernel reads"""
    out = []
    for h in ms.moshes(s)[0]:
        ix = ms.ix.get(int(h), 0)
        cc = ms.info[ix] & 3 if ix else 0
        if cc in (1, 2):
            l = ref.rev[ref.loc[ix]]
            l2 = ref.rev[ref.loc[ix] + 1] if cc == 2 else 0
            out.append((cc, l, l2, ref.id[l], ref.id[l2] if cc == 2 else 0))
        else:
            out.append((cc, 0, 0, 0, 0))
    return out


# ---- the walk, restated ---------------------------------------------------------------------------------------------------------------------
VARIANTS = ("drift_ge_50", "drift_le_minus_50", "backwards_not_strict", "no_retry", "retry_without_block", "closing_flush_on_n1",
            "flush_on_n1_plus_n2", "hit0_opens_block", "ordinal_over_qualifying", "failed_retry_opens_on_first")
# a case whose records each wrong walk changes (test_moshmap_blocks_cpu.py holds every entry to it)
CATCHES = {"drift_ge_50": "drift_asc_pos_50", "drift_le_minus_50": "drift_desc_neg_50", "backwards_not_strict": "dir_equal_loc_stays",
           "no_retry": "retry_ascending", "retry_without_block": "hit0_copy2_no_retry", "closing_flush_on_n1": "flush_final_5_2",
           "flush_on_n1_plus_n2": "flush_2_3_then_elsewhere", "hit0_opens_block": "hit0_first_seed", "ordinal_over_qualifying": "drift_asc_neg_51",
           "failed_retry_opens_on_first": "retry_both_end"}


def blocks(seeds, variant=None):
    """the records (i0, iN, loc0, locN, n1, n2) of queryProcess over (class, loc, loc2, id, id2) per seed; variant names a wrong walk"""
    assert variant is None or variant in VARIANTS
    v = lambda name: variant == name
    hi, lo = (49 if v("drift_ge_50") else 50), (-49 if v("drift_le_minus_50") else -50)
    opened = False                                               # the reference has no such flag: loc0 == 0 is "no block"
    loc0 = locN = i0 = iN = id0 = n1 = n2 = 0
    recs = []

    def ends(loc, idl):
        if idl != id0:
            return True
        if loc0 == locN:
            return False
        asc = loc0 < locN
        d = ((locN - loc0 if asc else loc0 - locN) - iN + i0) & M32    # U32 arithmetic, read as int
        d = d - (1 << 32) if d >> 31 else d
        if v("backwards_not_strict"):
            back = loc <= locN if asc else loc >= locN
        else:
            back = loc < locN if asc else loc > locN
        return back or d > hi or d < lo

    i = -1
    for cc, loc, loc2, idl, id2 in seeds:
        if v("ordinal_over_qualifying"):
            i += cc in (1, 2)
        else:
            i += 1
        if cc not in (1, 2):
            continue
        is_open = opened if v("hit0_opens_block") else loc0 != 0
        end = not is_open or ends(loc, idl)
        if end and cc == 2 and (is_open or v("retry_without_block")) and not v("no_retry"):
            end = ends(loc2, id2)
            if not (end and v("failed_retry_opens_on_first")):
                loc, idl = loc2, id2
        if end:
            if (n1 + n2 if v("flush_on_n1_plus_n2") else n1) > 2:
                recs.append((i0, iN, loc0, locN, n1, n2))
            n1 = n2 = 0
            loc0, id0, i0, opened = loc, idl, i, True
        if cc == 1:
            n1 += 1
        else:
            n2 += 1
        locN, iN = loc, i
    if (n1 if v("closing_flush_on_n1") else n2) > 2:
        recs.append((i0, iN, loc0, locN, n1, n2))
    return recs


# ---- texts, files and the fixture -------------------------------------------------------------------------------------------------------------
def m_lines(ref, name, s, recs, copy1):
    """the M lines of the records, formatted as the reference does"""
    _, ps = ref.ms.moshes(s)
    nm = lambda loc: ref.dict.names[ref.id[loc] + 1]
    return ["M\t%s\t%d\t%d\t%d\t%s\t%d\t%d\t%d %d\t%s\t%s" % (name, ps[i0], ps[iN], len(s), nm(l0), ref.offset[l0], ref.offset[lN], n1, n2,
                                                             mp.c_ratio(n1 + n2, abs(lN - l0)), mp.c_ratio(n1, copy1)) for i0, iN, l0, lN, n1, n2 in recs]


def fasta(names, seqs, width=100):
    out = []
    for n, s in zip(names, seqs):
        t = "".join("ACGT"[c] for c in s)
        out.append(">%s\n" % n + "".join(t[i:i + width] + "\n" for i in range(0, len(t), width)))
    return "".join(out).encode()


def pairs_and_starts(lines, base):
    """(n1, n2) and the local ordinal of loc0 of every M line: the sequence name is s<id> and the offset (loc % SEQ) * 31"""
    pairs, starts = [], []
    for ln in lines:
        f = ln.split("\t")
        if f[0] == "M":
            pairs.append(tuple(int(x) for x in f[8].split()))
            starts.append(int(f[5][1:]) * SEQ + int(f[6]) // W - base)
    return pairs, starts


def split_queries(lines):
    """the lines of a -q run per query: {name: [its Q line and what follows it]}"""
    out, cur = collections.OrderedDict(), None
    for ln in lines:
        if ln.startswith("Q\t"):
            cur = out.setdefault(ln.split("\t")[1], [])
        if cur is not None and (ln[:2] in ("Q\t", "M\t") or ln.startswith("  ")):
            cur.append(ln)
    return out


_built = {}


def built(group):
    """build() of a group with its file bytes, once per process: dict of ms, ref, queries, scripts, cases, base and files {name: bytes}"""
    if group not in _built:
        cases = GROUPS[group]
        ms, ref, queries, scripts = build(cases)
        files = {"x.mosh": ms.to_bytes(), "x.ref": ref.to_bytes(), "all.fa": fasta([c.name for c in cases], queries)}
        for c, s in zip(cases, queries):
            files[c.name + ".fa"] = fasta([c.name], [s])
        _built[group] = dict(ms=ms, ref=ref, queries=queries, scripts=scripts, cases=cases, base=bases(cases), files=files)
    return _built[group]
