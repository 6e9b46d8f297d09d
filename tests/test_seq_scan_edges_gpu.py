"""The one k-mer walk of csrc/seq_plan.hpp / seq_scan.hpp under the mosh-set and readset scan kernels (mosh_scan_kernel of stage_g.hip, rs_scan_kernel of
stage_h.hip) at the boundaries of a lane's run of 64 k-mer starts. Every comparison is exact equality; the expected values come from the models of
tests/mosh_model.py and tests/asm_model.py (orc.Oracle's hasher, pinned to the reference). The crib kernel has these lengths in crib_cases.py.

k = 16, B = 20. The sequence lengths 0, 1, k - 1, k, k + 62 .. k + 64, k + 127 .. k + 129 put the last k-mer of a sequence at the end of a run, at the start of
the next and one further: a lane whose run starts inside a sequence primes from the bases before its first k-mer. 30 rounds of them, rotated, so that every length
falls on odd and even file ordinals, and the runs fill more than one workgroup. With w = 1 every k-mer is a mosh: every slot of every run is observed, and the
list's estimate is the number of k-mers, so no batch is scanned twice (w = 3: the estimate is still above what is listed). Palindromic 16-mers are planted: their
two strands tie, and a tie is reverse."""
import numpy as np
import pytest

import asm_model as am
import mosh_model as mm

pytestmark = pytest.mark.gpu
K, B, SEED = 16, 20, 5
LENS = [0, 1, K - 1, K, K + 62, K + 63, K + 64, K + 127, K + 128, K + 129]
ROUNDS = 30


def _sequences():
    rs = np.random.RandomState(1604)
    seqs = []
    for rep in range(ROUNDS):
        for n in LENS[rep % len(LENS):] + LENS[:rep % len(LENS)]:
            s = rs.randint(0, 4, n).astype(np.uint8)
            if n >= K and rep % 3 == 0:                         # its own reverse complement: the strands tie
                s[K // 2:K] = (3 - s[:K // 2])[::-1]
            seqs.append(s)
    return seqs


SEQS = _sequences()
HALF = SEQS[:len(SEQS) // 2]


@pytest.fixture(scope="module", params=[1, 3], ids=["w1", "w3"])
def case(request):
    """w, and the model's moshes of every sequence (computed once)"""
    w = request.param
    model = mm.MoshModel(B, K, w, SEED)
    per_seq = [model.moshes(s) for s in SEQS]
    ties = 0
    for s, (hs, ps) in zip(SEQS, per_seq):
        ties += len(s) >= K and bool((s[K // 2:K] == (3 - s[:K // 2])[::-1]).all()) and 0 in ps.tolist()
    assert ties >= ROUNDS // 3 * (1 if w > 1 else 7)            # planted palindromes that are moshes (w = 1: all of them)
    return w, per_seq


def test_lengths_cover_the_run_boundaries():
    starts = sorted({max(0, n - K + 1) for n in LENS})
    assert starts == [0, 1, 63, 64, 65, 128, 129, 130] and sum(-(-max(0, n - K + 1) // 64) for n in LENS) * ROUNDS > 256


def test_scan_lists_every_mosh(case):
    import hash10x_amd
    w, per_seq = case
    exp = [(int(h), s, int(p)) for s, (hs, ps) in enumerate(per_seq) for h, p in zip(hs.tolist(), ps.tolist())]
    if w == 1:
        assert len(exp) == sum(max(0, len(s) - K + 1) for s in SEQS)
    codes, start = mm.flatten(SEQS)
    h, q, p = hash10x_amd.mosh_scan(codes, start, K, w, SEED)
    assert list(zip(h.tolist(), q.tolist(), p.tolist())) == exp
    ms = hash10x_amd.MoshSet(B=B, k=K, w=w, seed=SEED)
    h, q, p = ms.scan(codes, start)
    assert list(zip(h.tolist(), q.tolist(), p.tolist())) == exp and ms.counters()["scan_retries"] == 0
    ms.close()


@pytest.mark.parametrize("is10x,seq_base", [(False, 0), (True, 0), (True, 1)], ids=["plain", "10x", "10x-odd-base"])
def test_add_values_depths_and_order(case, is10x, seq_base):
    """the set after -a / -x in two calls (the second finds the first's hashes in the table): values in order of first appearance, depths, the table"""
    import hash10x_amd
    w, _ = case
    rs = np.random.RandomState(23)
    seqs = [np.concatenate([rs.randint(0, 4, 23).astype(np.uint8), s]) if is10x and ((seq_base + i + 1) & 1) else s for i, s in enumerate(SEQS)]
    model = mm.MoshModel(B, K, w, SEED)
    ms = hash10x_amd.MoshSet(B=B, k=K, w=w, seed=SEED)
    cut = len(seqs) // 2 + 1                                     # (odd: the second call's first sequence has the other parity than its index)
    for part, base in ((seqs[:cut], seq_base), (seqs[cut:], seq_base + cut)):
        _, _, n = model.add(part, is10x, base)
        assert ms.add(*mm.flatten(part), is10x=is10x, seq_base=base) == n
    ix, v, dep, info = ms.export()
    assert v.tolist() == model.value and dep.tolist() == model.depth and not info.any()
    assert np.array_equal(ix, model.table())
    assert ms.counters()["scan_retries"] == 0
    ms.close()


def test_readset_hits_strands_and_misses(case):
    """-f over a set that holds the moshes of the first half of the sequences: hits with their strand bit, dx, nMiss per read, the set's depths"""
    import hash10x_amd
    w, _ = case
    model = mm.MoshModel(B, K, w, SEED)
    model.add(HALF)
    ms = hash10x_amd.MoshSet(B=B, k=K, w=w, seed=SEED)
    ms.add(*mm.flatten(HALF))
    rm = am.ReadsetModel(model)
    rm.add(SEQS)
    rs = hash10x_amd.ReadSet(ms)
    rs.add(*mm.flatten(SEQS))
    reads, hs, hit, dx = rs.export()
    exp = rm.reads[1:]
    assert len(reads) == len(rm.reads)
    assert reads["len"][1:].tolist() == [r.len for r in exp] and reads["nMiss"][1:].tolist() == [r.nMiss for r in exp]
    assert reads["nHit"][1:].tolist() == [r.nHit for r in exp] and np.diff(hs.astype(np.int64))[1:].tolist() == [r.nHit for r in exp]
    assert hit.tolist() == [x for r in exp for x in r.hit] and dx.tolist() == [x for r in exp for x in r.dx]
    top = [x >> 31 for r in exp for x in r.hit]
    assert 0 in top and 1 in top and sum(r.nMiss for r in exp) > 0
    assert ms.export(index=False)[2].tolist() == model.depth
    assert ms.counters()["scan_retries"] == 0
    rs.close(); ms.close()
