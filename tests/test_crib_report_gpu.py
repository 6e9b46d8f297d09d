"""The cases of tests/crib_cases.py on the GPU. Arrays: Hash10x.read_hash of the case's state, crib_sequences of its genomes, then crib_export
(crib_scan_kernel, crib_classify_kernel), cluster_report_raw (cluster_report_kernel), crib_summary_raw and crib_words (crib_summary_kernel,
crib_words_kernel) compared entry for entry with tests/crib_model.py — the fields no text shows among them: chr / pos of `mul` hashes, the
position kept under atomics, the histograms beyond depth 255. Text: bin/hash10x-amd on the case's files against the reference binary's recorded
lines (tests/golden/crib/), on one GPU and, for two cases, on 2 and 3 shards. Needs a real MI355X: `pytest -m gpu`."""
import os
import subprocess

import numpy as np
import pytest

import crib_cases as cc
import crib_model as cm
import orc

pytestmark = pytest.mark.gpu

NAMES = list(cc.CASES)
CLI = [n for n, c in cc.CASES.items() if not c.heavy]        # S3_long goes through the C ABI as a code array only: no 67 MB FASTA here


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return str(tmp_path_factory.mktemp("crib_cases"))


def _load(name, root):
    import hash10x_amd
    st, m, data = cc.built(name)
    path = os.path.join(root, name + ".hash")
    if not os.path.exists(path):
        with open(path, "wb") as f:
            f.write(data)
    h = hash10x_amd.Hash10x(k=st.k, w=st.w, r=st.seed, B=st.B)
    h.read_hash(path)
    return h, st, m


def _check_report(tag, brep, crep, blocks, rep, depth):
    """the raw records of h10x_cluster_report over `blocks` (None = block 0) against cluster_report's dicts"""
    at = 0
    for j, (blk, r) in enumerate(zip(blocks, rep)):
        b = brep[j]
        if blk is None:
            assert (int(b["nGood"]), int(b["nClusHash"]), int(b["nClusRead"])) == (0, 0, 0), tag + "block 0"
            continue
        want = (cm.n_good(blk[0], depth, cc.LO, cc.HI), r["nClusHash"], r["nClusRead"])
        assert (int(b["nGood"]), int(b["nClusHash"]), int(b["nClusRead"])) == want, "%sblock %d of the range: (nGood, nClusHash, nClusRead) %r, model %r" % (tag, j, b, want)
        for l, c in enumerate(r["clusters"], start=1):
            g = crep[at]; at += 1
            got = {"n": int(g["n"]), "nRead": int(g["nRead"]), "nt": g["nt"].tolist(), "chr": int(g["chr"]), "pMin": int(g["pMin"]), "pMax": int(g["pMax"]), "nBad": int(g["nBad"]),
                   "other": g["other"][:int(g["nOtherListed"])].tolist()}
            exp = {f: c[f] for f in got}
            assert got == exp, "%sblock %d of the range, label %d:\n  gpu   %r\n  model %r" % (tag, j, l, got, exp)
    assert at == len(crep), tag + "%d cluster records, %d looked at" % (len(crep), at)


def _check_summary(tag, h, blocks, summary, words):
    counts, seen_b, seen_c = h.crib_summary_raw()
    base, clus, n_base, n_clus, set_b, set_c = summary
    assert counts[:5].tolist() == base and counts[5:10].tolist() == clus and (int(counts[10]) + 1, int(counts[11])) == (n_base, n_clus), tag + "counts %r, model %r" % (counts, summary[:4])
    assert np.flatnonzero(seen_b).tolist() == sorted(set_b) and np.flatnonzero(seen_c).tolist() == sorted(set_c), tag + "seen sets"
    total = len(words)
    assert h.sizes()["nClusHash"] == total
    edges = np.cumsum([len(b[0]) for b in blocks])
    cut = next((int(e0 + (e1 - e0) // 2) for e0, e1 in zip(np.r_[0, edges[:-1]], edges) if e1 - e0 >= 2), 0)      # inside the first block of two records or more
    for first, count in ((0, total), (cut, total - cut), (0, cut), (cut, 1), (total - 1, 1), (cut, min(300, total - cut)), (total, 0)):
        got = h.crib_words(first, count)
        assert np.array_equal(got, words[first:first + count]), tag + "crib_words(%d, %d)" % (first, count)


@pytest.mark.parametrize("name", NAMES)
def test_arrays_match_the_model(root, name):
    h, st, m = _load(name, root)
    got = h.crib_sequences(st.genome[0], st.genome[1])
    assert got == [(m.a[2], m.a[3]), (m.b[2], m.b[3])], "known / unknown moshes %r, model %r" % (got, [m.a[2:4], m.b[2:4]])
    x = h.crib_export()
    for f, want in (("type", m.crib.type), ("chr", m.crib.chr), ("pos", m.crib.pos)):
        d = np.flatnonzero(x[f] != want)
        names = {i: n for n, i in st.names.items()}
        assert d.size == 0, "crib %s differs at %d indices, first %d (%s): gpu %d, model %d" % (f, d.size, d[0], names.get(int(d[0])), x[f][d[0]], want[d[0]])
    assert x["arrayMax"].tolist() == m.crib.array_max
    dim = x["hist"].shape[1]
    assert dim == int(m.crib.depth.max()) + 1
    for s in range(4):
        want = np.zeros(dim, dtype=np.uint32); want[:len(m.crib.hist[s])] = m.crib.hist[s]
        assert np.array_equal(x["hist"][s], want), "depth histogram %d" % s
    h.depth_range(cc.LO, cc.HI)
    n = len(st.blocks)
    _check_report("all blocks: ", *h.cluster_report_raw(1, n), st.blocks, m.reports, m.crib.depth)
    for a, b in st.ranges:                                   # the ranges of the command line, block 0 included where they start there
        b = b or n + 1
        blocks = [None if c == 0 else st.blocks[c - 1] for c in range(a, b)]
        rep = ([None] if a == 0 else []) + cm.cluster_report(st.blocks[max(a, 1) - 1:b - 1], m.crib)
        _check_report("blocks %d .. %d: " % (a, b), *h.cluster_report_raw(a, b - a), blocks, rep, m.crib.depth)
    _check_summary("", h, st.blocks, m.summary, m.words)
    if st.split:
        h.cluster_split()
        assert h.export_blocks()["clusterParent"].tolist() == [0] + [b[4] for b in m.split_blocks]
        _check_summary("after the split: ", h, m.split_blocks, m.split_summary, m.split_words)
    h.close()


def test_report_range_outside_the_blocks_is_refused(root):
    import hash10x_amd
    h, st, m = _load("R3_first_located", root)
    n = len(st.blocks) + 1
    with pytest.raises(hash10x_amd.Hash10xError, match="outside"):
        h.cluster_report_raw(2, n - 1)
    with pytest.raises(hash10x_amd.Hash10xError, match="outside"):
        h.cluster_report(0, n + 1)
    assert len(h.cluster_report_raw(n, 0)[0]) == 0
    h.close()


def test_32768_sequences_are_refused(root):
    """one sequence more than a 16-bit chr can number: the refusal of stageD_cribGenome, and the state keeps no half-made crib"""
    import hash10x_amd
    h, st, m = _load("S7_32767_sequences", root)
    with pytest.raises(hash10x_amd.Hash10xError, match="at most 32767"):
        h.crib_sequences(st.genome[0] + [st.genome[0][0]], st.genome[1])
    with pytest.raises(hash10x_amd.Hash10xError, match="no crib"):
        h.crib_export()
    h.close()


def _cli(name, root, gpus=1):
    files = cc.write_files(name, root)
    g = subprocess.run([os.path.join(orc.REPO, "bin", "hash10x-amd")] + (["--gpus", str(gpus)] if gpus > 1 else []) + cc.args(name, *files), cwd=root,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert g.returncode == 0, g.stderr.decode(errors="replace")[-2000:]
    ref = cc.golden(name)
    got = cm.report(g.stdout)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a == b, "%s, --gpus %d, line %d:\n  hip: %s\n  ref: %s" % (name, gpus, i, a, b)
    assert len(got) == len(ref)


@pytest.mark.parametrize("name", CLI)
def test_cli_text_matches_recorded_reference(root, name):
    _cli(name, root)


@pytest.mark.parametrize("gpus", [2, 3])
@pytest.mark.parametrize("name", ["S6_pairs", "R1_sizes"])
def test_cli_text_on_shards(root, name, gpus):
    _cli(name, root, gpus)
