"""Hand-built `.hash` states at the exact numbers the list loop of --cluster switches on (cluster_kernel in hash10x_amd/csrc/stage_c.hip:
row_mode_hist<…, 1 | 2 | RCHUNK>, row_mode_long, short_round, the settle phase behind the loop, the placements of first[] and the length classes
of the packed translated placement), and the registry of cases test_list_loop_cpu.py and test_list_loop_gpu.py run. The builder is
tests/cluster_states.py; the cases here use what it states about a rank's list (Subject.lay, Subject.lists): its length d as the kernel sees it
(the block's own entry included), the index of the own entry, the index of every counted entry, msBest / msMax / msTot and the count of the pointToMin term.
Every case's `where` asserts from these that the case sits where its name says, and cluster_states.check compares the builder's replay with the oracle
before anything runs on the GPU.

A subject is small: rank 0, the ranks that own companions (roots), and the ranks whose lists decide. An owner's list length grows with what it
owns, and the ranks of a block ascend in length, so deciding ranks of very different lengths get a subject each; many subjects share a file.

Families (FAMILY[name]): a length seams of the one-list bodies; b counts across chunks, ties, owners that share a histogram word; c the threshold in every
body; d rounds and the settle phase; e position of the own entry, first and last barcode of the file, bitmap word edges; f class census of the packed
translated placement; g table edges of the translated placement.

TEST INFRASTRUCTURE — plain Python, never imported by hash10x_amd/."""
import collections

import cluster_states as cs
from cluster_states import State

HI = 600                                                     # --hashDepthRange 2 600 (1 600 where a list of one entry is wanted): lists of up to 599 entries
LIST_CASES = collections.OrderedDict()
cs.REGISTRIES.append(LIST_CASES)
FAMILY = {}
FAMILIES = "abcdefg"


def case(name, family, ct=1, lo=2, hi=HI):
    FAMILY[name] = family
    return cs.case(name, ct=ct, lo=lo, hi=hi, registry=LIST_CASES)


class Claims:
    """what each subject of a file must show: fn(L, e) with L = Subject.lists(ct), e = its Expect; `where` runs them all and refuses an empty file"""

    def __init__(self, st, ct):
        self.st, self.ct, self.items = st, ct, []

    def add(self, s, fn):
        self.items.append((s, fn))

    def where(self, *ex):
        assert self.items and len(ex) == len(self.st.items)
        assert self.st.n_codes < 20000, "%d blocks: the dense placement ends at 24576 barcodes" % self.st.n_codes
        for s, fn in self.items:
            fn(s.lists(self.ct), ex[self.st.items.index(s)])


def decider(st, d, own_at, counted, roots=None, idle=0):
    """a subject of rank 0, `idle` ranks nobody shares, the owners named in counted (numbered from 1 in counted, placed behind the idle ranks) and ONE deciding rank
    whose list is laid out entry by entry (Subject.lay). Returns (subject, deciding rank, {owner number: rank})."""
    s = st.subject()
    s.start()
    if idle:
        s.ranks(idle)
    k = roots if roots is not None else max(counted.values(), default=0)
    rk = {f: s.rank() for f in range(1, k + 1)}
    i = s.rank()
    s.lay(i, d, own_at, {j: rk[f] for j, f in counted.items()})
    return s, i, rk


def free_index(d, taken, start):
    return next(j for j in list(range(start, d)) + list(range(start)) if j not in taken)


def spread(d, x, y):
    """x entries of owner 1 and y of owner 2 in a list of d: the first at index 0 and at the last index, the second at index 1 and the last but one, the others on both
    sides of the chunk boundaries the list has"""
    seen, u = set(), []
    for p in [0, d - 1, 1, d - 2] + [p for p in (63, 64, 127, 128, 191, 192, 255, 256) if 2 <= p < d - 2] + list(range(2, max(d - 2, 2))):
        if 0 <= p < d and p not in seen:
            seen.add(p); u.append(p)
    a = [u[k] for k in (0, 1, 4, 6, 8, 10)[:x]]
    b = [u[k] for k in (2, 3, 5, 7, 9, 11)[:y]]
    out = {j: 1 for j in a}
    out.update({j: 2 for j in b})
    assert len(out) == x + y
    return out


# ------------------------------------------------------------------------------------------------ a. length seams of the one-list bodies
SEAMS = (2, 16, 17, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 191, 192, 193, 254, 255, 256, 257, 320)


@case("a_lengths", "a")
def _():
    """one subject per length: 4 entries of rank 1 and 3 of rank 2 (term 4/7), one at index 0, one at the last index, the own entry in the middle. d = 2: the one companion is
    rank 1's (term 1/1)"""
    st = State(); cl = Claims(st, 1)
    for d in SEAMS:
        counted = {1: 1} if d == 2 else spread(d, 4, 3)
        own = 0 if d == 2 else free_index(d, counted, d // 2)
        s, i, rk = decider(st, d, own, counted)

        def claim(L, e, d=d, i=i, rk=rk, own=own):
            r = L[i]
            assert r.d == d and r.own == own and r.best == rk[1]
            if d == 2:
                assert (r.mx, r.tot, r.q) == (1, 1, 1) and r.at[rk[1]] == [1]
            else:
                assert (r.mx, r.tot, r.q) == (4, 7, 4) and 0 in r.at[rk[1]] and d - 1 in r.at[rk[1]] and 1 in r.at[rk[2]] and e.terms[-1] == (i, 4, 7)
        cl.add(s, claim)
    return st, cl.where


@case("a_length1", "a", lo=1)
def _():
    """--hashDepthRange 1 600: a block whose three good hashes nobody shares (d = 1: the own entry alone, every rank inactive) beside one whose ranks 1 and 2 share a companion"""
    st = State(); cl = Claims(st, 1)
    s = st.subject(); s.ranks(3)
    cl.add(s, lambda L, e: all(r.d == 1 and r.own == 0 and r.tot == 0 for r in L) and e.raw == 0 or cs.moved())
    s2 = st.subject(); s2.ranks(2); t = s2.rank(); s2.comp([1, t])
    cl.add(s2, lambda L, e: ([r.d for r in L] == [1, 2, 2] and L[t].best == 1 and e.terms == [(t, 1, 1)]) or cs.moved())
    return st, cl.where


@case("a_full", "a", ct=254)
def _():
    """one owner holds every entry but the own one: 254, 255 and 256 of one value at -ct 254. The byte histogram counts 254 (d = 255: the longest list it is given),
    row_mode_long takes over at d = 256. The own entry first, in the middle, last."""
    st = State(); cl = Claims(st, 254)
    for d, own in ((255, 0), (255, 254), (255, 128), (256, 0), (256, 255), (257, 64), (257, 256)):
        s, i, rk = decider(st, d, own, {j: 1 for j in range(d) if j != own})

        def claim(L, e, d=d, i=i, own=own):
            r = L[i]
            assert (r.d, r.own, r.mx, r.tot, r.q, r.best) == (d, own, d - 1, d - 1, d - 1, 1) and e.terms == [(i, d - 1, d - 1)] and e.raw == 1
        cl.add(s, claim)
    # the other side of the threshold: 253 of one value and a second owner beside it — inactive at -ct 254
    s, i, rk = decider(st, 255, 100, {j: (1 if j < 254 else 2) for j in range(255) if j != 100})
    cl.add(s, lambda L, e, i=i: ((L[i].d, L[i].mx, L[i].tot) == (255, 253, 254) and e.raw == 0) or cs.moved())
    return st, cl.where


# ------------------------------------------------------------------------------------------------ b. counts across chunks
@case("b_four_chunks", "b")
def _():
    """the winner has one entry in each of the four chunks, the runner-up all of its three in one; d = 250, 200 and 193 (the fourth chunk holds one entry)"""
    st = State(); cl = Claims(st, 1)
    for d, win, lose, own in ((250, (10, 70, 140, 249), (80, 81, 82), 100), (200, (63, 64, 128, 192), (129, 130, 131), 0), (193, (0, 64, 128, 192), (1, 2, 3), 100)):
        counted = {j: 2 for j in win}                      # the winner is the HIGHER rank: a count decides, not the order
        counted.update({j: 1 for j in lose})
        s, i, rk = decider(st, d, own, counted)

        def claim(L, e, d=d, i=i, rk=rk):
            r = L[i]
            assert r.d == d and r.best == rk[2] and (r.mx, r.tot, r.q) == (4, 7, 4)
            assert sorted(j // 64 for j in r.at[rk[2]]) == [0, 1, 2, 3] and len({j // 64 for j in r.at[rk[1]]}) == 1
        cl.add(s, claim)
    return st, cl.where


TIES = (("c0", 40, (5, 6, 7), (1, 2, 3), 20), ("c0_2chunks", 100, (5, 6, 7), (1, 2, 3), 64), ("c0_4chunks", 200, (50, 51, 52), (1, 2, 3), 128),
        ("last_first_2", 128, (125, 126, 127), (0, 1, 2), 64), ("last_first_4", 200, (193, 195, 199), (0, 2, 63), 64), ("last_first_255", 255, (192, 253, 254), (0, 1, 63), 191),
        ("long_c0", 300, (40, 41, 42), (1, 2, 3), 0), ("long_last_first", 300, (256, 298, 299), (0, 1, 2), 150), ("long_256", 256, (193, 254, 255), (0, 63, 64), 100),
        # the lower rank's value met FIRST: a loop that lets the later of two equal counts win is wrong only here
        ("low_first_c0", 40, (1, 2, 3), (5, 6, 7), 20), ("low_first_4", 200, (0, 2, 63), (193, 195, 199), 64), ("long_low_first_c0", 300, (1, 2, 3), (40, 41, 42), 0),
        ("long_low_first", 300, (0, 1, 63), (256, 298, 299), 150), ("long_low_first_256", 256, (0, 63, 64), (193, 254, 255), 100))


@case("b_ties", "b")
def _():
    """equal counts, the lower rank must win (hash10x.c:804: strict >): both values inside chunk 0; the lower rank's entries only in the last chunk and the higher rank's only
    in the first; the same on lists of 256 entries and more, where row_mode_long meets the HIGHER rank's value first"""
    st = State(); cl = Claims(st, 1)
    for tag, d, low, high, own in TIES:
        counted = {j: 1 for j in low}
        counted.update({j: 2 for j in high})
        s, i, rk = decider(st, d, own, counted)

        def claim(L, e, d=d, i=i, rk=rk, tag=tag):
            r = L[i]
            assert r.d == d and r.best == rk[1] and (r.mx, r.tot, r.q) == (3, 6, 3) and len(r.at[rk[2]]) == 3
            assert e.labels[rk[1]] == 1 and e.labels[rk[2]] == 0 and e.labels[i] == 1
            if "last_first" in tag:
                assert {j // 64 for j in r.at[rk[1]]} == {(d - 1) // 64} and {j // 64 for j in r.at[rk[2]]} <= {0, 1} and min(r.at[rk[2]]) == 0
            elif "low_first" in tag:
                assert max(r.at[rk[1]]) < min(r.at[rk[2]]) and (tag.endswith("c0") or {j // 64 for j in r.at[rk[2]]} == {(d - 1) // 64})
            else:
                assert max(r.at[rk[1]] + r.at[rk[2]]) < 64 or d == 256
        cl.add(s, claim)
    return st, cl.where


@case("b_stale_counts", "b")
def _():
    """two lists that one wave counts one after the other in its histogram (ranks 8 and 9: one group of four). In the first, rank 1's two entries lie only in the list's
    LAST chunk and rank 4 wins with three; in the second rank 1 has two again and rank 4 three. Counts of the first list left standing — cleared for the values of chunk 0
    alone — make rank 1 the second list's mode. Lists of two chunks, of four, and of 300 entries."""
    st = State(); cl = Claims(st, 1)
    for d in (100, 128, 200, 255, 300):
        s = st.subject(); s.start()
        a = s.rank(); s.ranks(2)
        b = s.rank(); s.ranks(3)                             # ranks 1 and 4: their counts lie in two histogram words, so clearing the one does not clear the other
        t1, t2 = s.rank(), s.rank()
        s.lay(t1, d, 10, {d - 1: a, d - 2: a, 0: b, 1: b, 2: b})
        s.lay(t2, d, 11, {d - 1: a, 3: a, 0: b, 1: b, 70: b})

        def claim(L, e, d=d, a=a, b=b, t1=t1, t2=t2):
            assert (a, b, t1, t2) == (1, 4, 8, 9) and L[t1].d == L[t2].d == d
            for t in (t1, t2):
                assert (L[t].best, L[t].mx, L[t].tot, L[t].q) == (b, 3, 5, 3) and len(L[t].at[a]) == 2
            assert {j // 64 for j in L[t1].at[a]} == {(d - 1) // 64} and (d - 1) // 64 >= 1 and max(L[t1].at[b]) < 64
            assert e.terms == [(t1, 3, 5), (t2, 3, 5)] and e.labels[b] == 1 and e.labels[a] == 0
        cl.add(s, claim)
    return st, cl.where


@case("b_shared_word", "b")
def _():
    """owners whose ranks share one histogram word (4k .. 4k + 3), large unequal counts: two and four of them, on one chunk, two chunks and four"""
    st = State(); cl = Claims(st, 1)
    for counts, d in (((15, 17, 16, 14), 63), ((15, 17, 16, 14), 64), ((30, 33, 31, 29), 124), ((30, 33, 31, 29), 130), ((40, 37), 128), ((0, 0, 60, 61), 200), ((62, 63, 61, 60), 255)):
        order = [f + 1 for f, c in enumerate(counts) for _ in range(c)]
        tot = len(order)
        cand = [j for j in range(d) if j != d // 2]
        idx = [cand[(k * len(cand)) // tot] for k in range(tot)]     # spread over the whole list
        assert len(set(idx)) == tot and tot % 5
        counted = {j: order[(5 * k) % tot] for k, j in enumerate(idx)}   # the owners interleaved: 5 is coprime to every total here
        s, i, rk = decider(st, d, d // 2, counted, roots=4, idle=3)      # the owners are ranks 4, 5, 6, 7

        def claim(L, e, d=d, i=i, rk=rk, counts=counts):
            r = L[i]
            assert [rk[f] for f in (1, 2, 3, 4)] == [4, 5, 6, 7] and r.d == d
            assert [len(r.at.get(rk[f + 1], [])) for f in range(len(counts))] == list(counts)
            w = rk[1 + counts.index(max(counts))]
            assert r.best == w and r.mx == max(counts) and r.tot == sum(counts) and r.q == max(counts)
        cl.add(s, claim)
    return st, cl.where


@case("b_far_words", "b")
def _():
    """owners at ranks 255, 256, 257 and 1023, 1024: the last byte of one histogram word and the first of the next, behind 254 and 765 inactive ranks"""
    st = State(); cl = Claims(st, 1)
    s = st.subject(); s.start()
    s.ranks(254)
    o = [s.rank(), s.rank(), s.rank()]
    s.ranks(765)
    o += [s.rank(), s.rank()]
    i = s.rank()
    counts = (3, 4, 2, 6, 5)
    counted, j = {}, 0
    for f, c in zip(o, counts):
        for _ in range(c):
            counted[j if j < 10 else j + 1] = f; j += 1
    s.lay(i, 21, 10, counted)

    def claim(L, e):
        assert o == [255, 256, 257, 1023, 1024] and i == 1025 and L[i].d == 21
        assert (L[i].best, L[i].mx, L[i].tot, L[i].q) == (1023, 6, 20, 6) and e.terms == [(i, 6, 20)]
        assert all(r.tot == 0 for r in L[:i])
    cl.add(s, claim)
    # the same owners, the winner now rank 256 and a tie between 255 and 1024 behind it
    s2 = st.subject(); s2.start(); s2.ranks(254)
    o2 = [s2.rank(), s2.rank(), s2.rank()]; s2.ranks(765); o2 += [s2.rank(), s2.rank()]
    i2 = s2.rank()
    counted, j = {}, 0
    for f, c in zip(o2, (4, 5, 1, 2, 4)):
        for _ in range(c):
            counted[j + 1] = f; j += 1
    s2.lay(i2, 17, 0, counted)
    cl.add(s2, lambda L, e: ((L[i2].best, L[i2].mx, L[i2].tot, L[i2].d) == (256, 5, 16, 17) and o2 == o) or cs.moved())
    return st, cl.where


# ------------------------------------------------------------------------------------------------ c. the threshold in every body
def _threshold(ct):
    def make():
        st = State(); cl = Claims(st, ct)
        for d in (50, 64, 100, 128, 200, 255, 256, 300):
            cand = [j for j in range(1, d) if j != d // 2 + 1]
            pos = lambda m: sorted({cand[len(cand) - 1 - (k * (len(cand) - 1)) // max(m - 1, 1)] for k in range(m)})   # m indices from the last down to 1, the own entry's left out
            variants = {
                "tot_below": ([ct - 1], False),              # msTot == ct - 1
                "tot_at": ([ct], True),                      # msTot == ct, one owner: ct / ct
                "max_below": ([ct - 1] * 4, False),          # msTot large, msMax == ct - 1
                "max_at": ([ct, ct - 1], True),              # msMax == ct exactly: ct / (2 ct - 1)
                "max_at_second": ([ct - 1, ct], True),       # ... held by the higher rank
            }
            for tag, (counts, active) in variants.items():
                m = sum(counts)
                idx = pos(m)
                assert len(idx) == m, (d, m, idx)
                owners = [f + 1 for f, c in enumerate(counts) for _ in range(c)]
                counted = {j: owners[(3 * k) % m] if m % 3 else owners[k] for k, j in enumerate(idx)}
                s, i, rk = decider(st, d, d // 2 + 1, counted)

                def claim(L, e, d=d, i=i, rk=rk, counts=counts, active=active):
                    r = L[i]
                    assert r.d == d and r.mx == max(counts) and r.tot == sum(counts) and (r.mx >= ct) == active
                    assert d - 1 in [j for v in r.at.values() for j in v]
                    if active:
                        assert r.mx == ct and e.terms == [(i, ct, sum(counts))] and e.labels[i] == 1
                    else:
                        assert r.mx == ct - 1 and e.terms == [] and e.raw == 0 and not any(e.labels)
                cl.add(s, claim)
        return st, cl.where
    return make


case("c_ct3", "c", ct=3)(_threshold(3))
case("c_ct5", "c", ct=5)(_threshold(5))


# ------------------------------------------------------------------------------------------------ d. rounds and the settle phase
ROUND = 64                                                   # ranks of a round at 1024 lanes and the default budget (nW * RIF); lds_24k, lds_2k and cluster_threads0=512 change it
RELATIONS = collections.OrderedDict([
    ("prev_in_group", lambda i: i - 1 if i % 4 else None),                         # same wave, same round
    ("other_wave", lambda i: i - 5 if (i - 5) // ROUND == i // ROUND else None),   # same round, another group of four
    ("last_of_prev_round", lambda i: i // ROUND * ROUND - 1 if i >= ROUND else None),
    ("first_of_round", lambda i: i // ROUND * ROUND if i % ROUND and i >= ROUND else None),   # (rank 0 owns nothing)
])


def _rounds(rel):
    def make():
        st = State(); cl = Claims(st, 1)
        for n in (132, 133, 134, 135):
            s = st.subject(); s.ranks(n)
            pairs = []
            for i in (63, 64, 65, 127, 128, n - 1):
                b = RELATIONS[rel](i)
                if b is None:
                    continue
                s.comp([b, i], front=True); s.comp([b, i]); s.comp([1, i])    # two entries of msBest on both sides of the own entry, one of rank 1
                pairs.append((i, b))

            def claim(L, e, n=n, pairs=pairs):
                assert e.n == n and len(pairs) >= 2
                for i, b in pairs:
                    assert L[i].best == b and L[i].mx == 2 and L[i].tot == 3 and e.labels[i] == e.labels[b] != 0
                    if rel != "last_of_prev_round":
                        assert b // ROUND == i // ROUND
                    else:
                        assert b // ROUND == i // ROUND - 1 and b % ROUND == ROUND - 1
                assert {q for _, q, _ in e.terms} >= {2}
            cl.add(s, claim)
        return st, cl.where
    return make


for _rel in RELATIONS:
    case("d_" + _rel, "d")(_rounds(_rel))


def _settle(idle):
    """Ranks the loop leaves open BY CONSTRUCTION, and long lists hung on them. A rank is left open when root[msBest] is not on record as its list is worked through. The
    straight-line round of the dense placement (short_round) and a unit of class Q of the packed translated placement store the roots of their four lists together, so in
    the chain c0 .. c0 + 3 — c0 a multiple of four and inactive (its own root), every list of at most 16 entries, each rank's msBest the rank before it — the ranks c0 + 1,
    c0 + 2 and c0 + 3 are open there whatever the waves' timing; and a rank whose msBest is open stays open in EVERY form. Per length 64, 65, 128, 129, 200, 300 a rank t
    whose msBest (three entries at the list's start and middle) is one of c0 + 1 .. c0 + 3 and whose two entries for the root c0 lie at the list's end — behind index 128 on
    the lists of 200 and 300 entries: the settle phase's own loop over the entries beyond two chunks. In the forms that store a root per list (2-byte dense, ranked, HBM
    slot, HBM scratch, unpacked translated) the chain is settled inside the loop, and so are these ranks: nothing but a race between waves leaves a rank open there.
    idle: inactive ranks in front (2080: the block is in the middle replay class)."""
    def make():
        st = State(); cl = Claims(st, 1)
        s = st.subject(); s.start()
        s.ranks(idle)
        s.ranks(-len(s.read) % 4)
        c0 = len(s.read)
        s.chain(4)
        marks = []
        for k, d in enumerate((64, 65, 128, 129, 200, 300)):
            b = c0 + 1 + k // 2
            t = s.rank()
            own = d // 2
            s.lay(t, d, own, {0: b, 1: b, min(own - 1, 70): b, d - 1: c0, d - 3: c0})
            marks.append((d, b, t))

        def claim(L, e):
            assert e.n == len(s.read) and (idle < 2080 or cs.REPLAY_SMALL < e.n <= cs.REPLAY_MID)
            assert c0 % 4 == 0 and L[c0].tot == 0 and [L[c0 + k].best for k in (1, 2, 3)] == [c0, c0 + 1, c0 + 2] and all(L[c0 + k].d <= 16 for k in range(4))
            assert e.labels[c0] == e.labels[c0 + 3] != 0
            assert {b for _, b, _ in marks} == {c0 + 1, c0 + 2, c0 + 3}
            for d, b, t in marks:
                r = L[t]
                assert r.d == d and r.best == b and (r.mx, r.tot, r.q) == (3, 5, 2) and e.labels[t] == e.labels[c0]
                assert r.at[c0] == [d - 3, d - 1] and (d < 200 or min(r.at[c0]) > 128) and max(r.at[b]) < 2 * 64
                assert (t, 2, 5) in e.terms
        cl.add(s, claim)
        return st, cl.where
    return make


case("d_settle", "d")(_settle(0))
case("d_settle_2100", "d")(_settle(2080))


# ------------------------------------------------------------------------------------------------ e. position of the own entry, first and last barcode, bitmap words
@case("e_own_entry", "e")
def _():
    """the block's own barcode at entry 0, 63, 64, 127, 128 and last, the entries before and behind it counted ones. The first subject's list begins with barcode 1 and
    holds counted companions at barcodes 31, 32, 33, 63, 64 and 65; a subject with ONE companion in front of it, at the last bit of a bitmap word its lists name nothing
    else of; the file's last barcode is a counted entry of the last subject."""
    st = State(); cl = Claims(st, 1)
    s, i, rk = decider(st, 130, 127, {0: 1, 31: 1, 62: 1, 63: 1, 126: 1, 128: 1, 30: 2, 32: 2, 64: 2})

    def first(L, e):
        r = L[i]
        assert r.d == 130 and r.own == 127 and r.codes[:127] == list(range(1, 128)) and (r.mx, r.tot, r.q) == (6, 9, 6)
        assert {r.codes[j] for v in r.at.values() for j in v} >= {1, 31, 32, 33, 63, 64, 65}
    cl.add(s, first)
    for d, own in ((130, 0), (130, 63), (130, 64), (130, 128), (130, 129), (64, 0), (64, 63), (65, 64), (129, 128), (300, 128), (300, 299), (256, 255)):
        near = [j for j in (own - 1, own + 1) if 0 <= j < d]
        far = [j for j in (0, 5, d - 1, d - 2) if j != own and j not in near]
        counted = {j: 1 for j in near + far[:1]}
        counted.update({j: 2 for j in far[1:1 + len(near)]})
        s, i, rk = decider(st, d, own, counted)

        def claim(L, e, d=d, own=own, i=i, near=near, rk=rk):
            r = L[i]
            assert (r.d, r.own) == (d, own) and all(j in r.at[rk[1]] for j in near) and r.best == rk[1] and r.tot > r.mx and r.q == r.mx == len(near) + 1, (d, own, r.at, r.q, r.mx, r.best)
        cl.add(s, claim)
    # one companion in front, at barcode 32 w + 31; the 31 barcodes in front of it in its word belong to nobody's lists here, the own barcode opens the next word
    made = sum(1 + sum(x.comp_front) for x in st.items)
    for _ in range((30 - made) % 32 + 32):
        st.plain()
    s = st.subject(); s.start(); a = s.rank(); t = s.rank()
    s.comp([a, t], front=True)
    s.fill(0, 1); s.comp([a, t])
    lone = s

    def word(L, e):
        c = L[t].codes[0]
        assert c % 32 == 31 and lone.code == c + 1 and L[t].own == 1 and L[t].at[a] == [0, 2]
        assert not [x for r in L for x in r.codes if x // 32 == c // 32 and x != c]
    cl.add(s, word)
    for _ in range(32):
        st.plain()
    # last subject: nothing is levelled, so its last companion — a counted one — is the file's last barcode
    s = st.subject(); s.start(); s.fill(0, 1, front=True); a = s.rank(); t = s.rank()
    s.lay(t, 3, 0, {1: a, 2: a})
    cl.add(s, lambda L, e: (L[t].codes[-1] == st.n_codes - 1 and L[t].at[a] == [1, 2] and [r.d for r in L] == [2, 3, 3]) or cs.moved())
    return st, cl.where


# ------------------------------------------------------------------------------------------------ f. class census of the packed translated placement
SHARES = ((1, 2), (2, 1), (3, 4), (4, 3), (1, 4), (5, 2), (2, 5), (6, 1), (1, 6), (3, 2), (2, 3), (5, 6), (6, 5), (4, 1), (1, 0), (0, 3))
CLASS_TOP = (("Q", 16), ("H", 32), ("F", 64), ("T", 96), ("D", 128), ("X", 1 << 30))


def klass(d):
    return next(k for k, top in CLASS_TOP if d <= top)


def census(st, cl, lengths, shift=0):
    """a subject whose ACTIVE lists have these lengths (ascending), each with a term of its own: ranks 1 and 2 own six companions each — rank 1's in front of the block,
    rank 2's behind it — and list k holds x of the one and y of the other, SHARES[k], and fillers in front of and behind the own entry. Rank 0 and the two owners are lists as
    well, never active: they get the lowest length of the first list's class (at least 8), so no class in front of it is used."""
    s = st.subject(); s.start()
    a, b = s.rank(), s.rank()
    s.own(a, 6, front=True); s.own(b, 6)
    low = max(8, {"Q": 8, "H": 17, "F": 33, "T": 65, "D": 97, "X": 129}[klass(lengths[0])])
    assert list(lengths) == sorted(lengths) and lengths[0] >= low
    s.fill(0, low - 1, front=True)
    s.fill(a, low - 7); s.fill(b, low - 7, front=True)
    rows = []
    for k, d in enumerate(lengths):
        x, y = SHARES[(k + shift) % len(SHARES)]
        i = s.child({a: x, b: -y} if y else {a: x})
        free = d - 1 - x - y
        ff = (0, free // 2, free)[k % 3]
        s.fill(i, ff, front=True); s.fill(i, free - ff)
        rows.append((i, d, x, y, x + ff))

    def claim(L, e):
        assert [r.d for r in L[:3]] == [low] * 3 and len(L) == 3 + len(lengths)
        for i, d, x, y, own in rows:
            r = L[i]
            assert (r.d, r.own, r.tot, r.mx) == (d, own, x + y, max(x, y)) and e.labels[i] != 0
            assert r.at.get(a, []) == list(range(x)) and r.at.get(b, []) == list(range(own + 1, own + 1 + y))
        assert len(e.terms) == len(lengths)
    cl.add(s, claim)
    return s


def spaced(lo, hi, k):
    return [lo + (hi - lo) * j // max(k - 1, 1) for j in range(k)] if k > 1 else [hi] * k


ROWS = collections.OrderedDict()
for _r in range(4):
    ROWS["q%d" % (8 + _r)] = spaced(8, 16, 8 + _r)                                   # four lists to an instruction: 4k + r
for _r in range(2):
    ROWS["h%d" % (4 + _r)] = spaced(17, 32, 4 + _r)                                  # two lists to an instruction
ROWS["t1"] = [96]; ROWS["t1_65"] = [65]; ROWS["t2"] = [65, 96]; ROWS["t3"] = [65, 65, 96]
ROWS["t8"] = [65, 65, 65, 66, 80, 96, 96, 96]; ROWS["t9"] = [65, 65, 65, 65, 66, 95, 96, 96, 96]   # tails of 1 and of 32 entries in both halves of the shared chunk
ROWS["each"] = [16, 32, 64, 96, 128, 129]
ROWS["x3"] = [129, 200, 300]
ROWS["q3_t3"] = [8, 12, 16, 65, 80, 96]
for _m in (64, 65, 128, 129, 256, 257):
    ROWS["max%d" % _m] = [16, 40, _m]                                              # unpacked: hStride is the power of two that holds the longest list
MIX = [8, 10, 12, 16, 16, 17, 24, 32, 33, 64, 65, 80, 96, 97, 128, 129, 255, 256, 300]   # 5 3 2 3 2 and X with 129, 255, 256, 300; every class edge on consecutive ranks


def seen_census(lengths):
    """the lists per class as the kernel sees them: the named ones and, in the first used class, rank 0 and the two owners"""
    c = collections.Counter(klass(d) for d in lengths)
    c[klass(lengths[0])] += 3
    return [c.get(k, 0) for k, _ in CLASS_TOP]


def _census_claims(cl, s, lengths, want):
    def claim(L, e):
        got = collections.Counter(klass(r.d) for r in L[3:])
        assert [got.get(k, 0) for k, _ in CLASS_TOP] == list(want), got
        real = collections.Counter(klass(r.d) for r in L)
        assert [real.get(k, 0) for k, _ in CLASS_TOP] == seen_census(lengths), real
    cl.add(s, claim)


@case("f_rows", "f")
def _():
    st = State(); cl = Claims(st, 1)
    for k, (tag, lengths) in enumerate(ROWS.items()):
        s = census(st, cl, lengths, shift=k)
        want = collections.Counter(klass(d) for d in lengths)
        _census_claims(cl, s, lengths, [want.get(c, 0) for c, _ in CLASS_TOP])
    # every remainder of a unit occurs among the rows AS THE KERNEL SEES THEM (each row's count is held to seen_census above): four lists of class Q to an instruction,
    # two of class H, two of class T to a unit of three chunks
    seen = [seen_census(v) for v in ROWS.values()]
    assert {q % 4 for q, *_ in seen if q} == {0, 1, 2, 3} and {h % 2 for _, h, *_ in seen if h} == {0, 1} and {t % 2 for _, _, _, t, _, _ in seen if t} == {0, 1}
    assert {(0, 0, 0, 0, 0, 6), (6, 0, 0, 3, 0, 0), (4, 1, 1, 1, 1, 1)} <= {tuple(v) for v in seen}    # only the per-list loop; an empty class between two used ones; every class
    return st, cl.where


@case("f_mix", "f")
def _():
    st = State(); cl = Claims(st, 1)
    s = census(st, cl, MIX)
    _census_claims(cl, s, MIX, (5, 3, 2, 3, 2, 4))
    cl.add(s, lambda L, e: all((p, q) in {(L[i].d, L[i + 1].d) for i in range(3, len(L) - 1)} for p, q in ((16, 17), (32, 33), (64, 65), (96, 97), (128, 129))) or cs.moved())
    return st, cl.where


# ------------------------------------------------------------------------------------------------ g. table edges of the translated placement
TABLE_CAP = 1024                                             # cluster_first_cap: S = S2 = 1024 slots, the first table closed at S - S / 8 = 896 inserts
TABLE_M = (895, 896, 897, 1500, 2100)


def _table(m):
    """one subject whose lists name exactly m distinct companions. Ranks 1 and 2 own six each (rank 1's the file's first barcodes, rank 2's behind the block); every later rank
    holds seven of those, three of the companions the rank before it brought in (so first[] values of late inserts are read too) and fillers of its own, up to 560 a rank."""
    def make():
        st = State(); cl = Claims(st, 1)
        s = st.subject(); s.start()
        a, b = s.rank(), s.rank()
        s.own(a, 6, front=True); s.own(b, 6)
        s.owned[a][0].append(0)                              # rank 0's list names nothing the others do not
        left = m - 12
        sizes = []
        size = 60
        while left:
            k = min(left, size, 560); sizes.append(k); left -= k; size += 110
        sizes.sort()
        prev, k = None, 0
        for f in sizes:
            x, y = ((1, 6), (2, 5), (3, 4), (4, 3), (5, 2), (6, 1))[k % 6]; k += 1
            i = s.child({a: x, b: -y})
            if prev is not None:
                for c in prev[-3:]:
                    c.append(i)
            mine = [[i] for _ in range(f)]
            half = f // 2
            for j, c in enumerate(mine):
                s.comps.append(c); s.comp_front.append(j < half)
            prev = mine

        def claim(L, e):
            assert len(s.comps) == m and len({c for r in L for c in r.codes} - {s.code}) == m, "levelling added a companion"
            assert max(r.d for r in L) < HI and e.raw >= 1 and len(e.terms) == len(sizes)
            assert sum(1 for r in L[4:] if len(r.at) == 3) == len(sizes) - 1
        cl.add(s, claim)
        return st, cl.where
    return make


for _m in TABLE_M:
    case("g_table_%d" % _m, "g")(_table(_m))
