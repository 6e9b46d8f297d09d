"""The hand-built list-loop states of tests/list_cases.py through the CPU oracle and the REAL reference binary: every case still sits at the length, chunk, class
or table edge it is named for (its own `where`, from what the builder states about each rank's list), the oracle's labels, cluster counts and pointToMin equal the
builder's replay bit for bit (cluster_states.check), and where oracle/_ref exists the reference binary's canonical bytes equal the oracle's. The builder's own
statements — list length, index of the own entry and of every counted entry, barcode numbers — are checked against a file read back, and the images of the older
cases are pinned by digest: the builder was generalised under them."""
import collections
import json
import os

import pytest

import cluster_states as cs
import list_cases as lc
import orc


@pytest.mark.parametrize("name", list(lc.LIST_CASES))
def test_case_sits_where_it_says(tmp_path, name):
    got, n_good = cs.run_oracle(name, str(tmp_path))
    cs.check(name, orc.HashFile(got), n_good)


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", list(lc.LIST_CASES))
def test_oracle_matches_reference(tmp_path, name):
    cwd = str(tmp_path)
    got, _ = cs.run_oracle(name, cwd)
    r = orc.run_ref(cs.args(name, name + ".in.hash", "ref.hash"), cwd)
    assert r.returncode == 0, r.stderr.decode()
    ref = orc.canonical_hash_bytes(open(os.path.join(cwd, "ref.hash"), "rb").read())
    assert got == ref, orc.describe_diff(got, ref)


def test_registry_holds_every_family():
    """a family cannot be dropped unnoticed, nor the members the GPU tests name"""
    per = collections.Counter(lc.FAMILY[n] for n in lc.LIST_CASES)
    assert set(per) == set(lc.FAMILIES) and set(lc.FAMILY) == set(lc.LIST_CASES), per
    assert per["a"] >= 3 and per["b"] >= 5 and per["c"] >= 2 and per["d"] >= 6 and per["f"] >= 2 and per["g"] == len(lc.TABLE_M) == 5
    assert set(lc.SEAMS) | {1} == {1, 2, 16, 17, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 191, 192, 193, 254, 255, 256, 257, 320}
    assert {"f_mix", "e_own_entry", "d_settle_2100"} <= set(lc.LIST_CASES) and lc.TABLE_M == (895, 896, 897, 1500, 2100)
    assert not set(lc.LIST_CASES) & set(cs.CASES)


def test_depth_range_is_the_case_s_own():
    assert cs.args("tie", "i", "o")[6:9] == ["--hashDepthRange", 2, 100]
    assert cs.args("a_length1", "i", "o")[6:9] == ["--hashDepthRange", 1, 600] and cs.args("f_mix", "i", "o")[6:9] == ["--hashDepthRange", 2, 600]
    st = cs.State(); s = st.subject(); s.start(); a = s.rank(); t = s.rank()
    s.lay(t, 100, 3, {0: a})
    with pytest.raises(AssertionError):
        st.build()                                           # a list of 100 entries under --hashDepthRange 2 100
    st = cs.State(); s = st.subject(); s.start(); a = s.rank(); t = s.rank()
    s.lay(t, 100, 3, {0: a})
    st.build(hi=101)


def test_builder_states_the_lists_the_file_holds():
    """Subject.lists against the file itself: for every rank of a subject with companions on both sides, the blocks that hold the rank's hash, in file order, are the
    barcode numbers stated; the own entry and every counted entry lie at the stated index; the owner of a counted entry is the lowest rank >= 1 its block holds"""
    st = cs.State()
    st.plain()
    s = st.subject(); s.start(); a, b = s.rank(), s.rank()
    t = s.rank()
    s.lay(t, 9, 4, {0: a, 3: b, 5: a, 8: b})
    u = s.rank()
    s.lay(u, 12, 2, {10: t, 0: a})                         # (the companion it shares with t lies behind the block: t's list grows at its end)
    hf = orc.HashFile(st.build())
    L = s.lists(1)
    own_hashes = hf.block_clushash(s.code)["hash"].tolist()
    holders = collections.defaultdict(list)
    for code in range(1, st.n_codes):
        for h in hf.block_clushash(code)["hash"].tolist():
            holders[h].append(code)
    for i, r in enumerate(L):
        assert r.codes == holders[own_hashes[i]] and r.d == len(r.codes) and r.codes[r.own] == s.code
        for f, idx in r.at.items():
            for j in idx:
                others = hf.block_clushash(r.codes[j])["hash"].tolist()
                assert min(k for k in range(1, len(L)) if own_hashes[k] in others) == f < i
    assert (L[t].d, L[t].own, dict(L[t].at), L[t].best, L[t].mx, L[t].tot, L[t].q) == (10, 4, {a: [0, 5], b: [3, 8]}, a, 2, 4, 2)
    assert (L[u].d, L[u].own, dict(L[u].at), L[u].best, L[u].mx, L[u].tot) == (12, 2, {a: [0], t: [10]}, a, 1, 2)
    assert s.code == 2 + 4 + 2 and [r.d for r in L] == sorted(r.d for r in L)


def test_images_of_the_older_cases_are_unchanged():
    """sha256 of built(name)[0] for every case of cluster_states.CASES, recorded before the builder learnt depth ranges per case and companions in front of a subject"""
    with open(os.path.join(orc.GOLDEN, "cluster_states_sha256.json")) as f:
        want = json.load(f)
    assert set(want) == set(cs.CASES)
    for name in cs.CASES:
        assert orc.sha256(cs.built(name)[0]) == want[name], name
