"""The dense list loop of --cluster (first[] dense in LDS, cluster_kernel<true, 0, ...>) on sets whose rounds fall into its
paths: straight-line rounds (the four lists of a wave's round all within one chunk of 64 entries), rounds of two-chunk lists,
rounds that mix length classes, and lists of three and four chunks. Every case compares the whole canonical .hash byte for
byte with the CPU oracle's, under the options that move blocks between the 4-byte and the 2-byte form of first[] and that
change how many waves share a block's ranks. Needs a real MI355X: `pytest -m gpu`."""
import os

import numpy as np
import pytest

import orc
from driver import run_commands

pytestmark = pytest.mark.gpu

K, W, R, B = 21, 31, 17, 20

# set: (gen_fqb arguments, depth range, classes of list lengths that must occur (<= 64, 65-128, 129-255), mixed groups expected)
SETS = {
    "A": ((60000, 300, 400000, 0.003, 43, 4.0, 150, 6000), (4, 300), (True, False, False), False),
    "B": ((120000, 300, 120000, 0.003, 45, 10.0, 150, 3000), (30, 300), (True, True, False), True),
    "C": ((40000, 300, 25000, 0.003, 48, 4.0, 150, 6000), (30, 300), (True, True, True), True),
}
DEFAULT_CT = {"A": 3, "B": 4, "C": 5}


def _list_classes(o):
    """Lists of the good hashes by length class, and the groups of four consecutive ranks of a block that mix classes —
    from the oracle's own arrays."""
    depth, _, _ = o.hash_depth()
    blocks, _, mx = o.blocks()
    counts = np.zeros(4, dtype=np.int64)
    mixed = 0
    for code in range(1, mx):
        good = o.good_hashes(code)
        if len(good) < 2:
            continue
        d = depth[o.clushash(code)["hash"][good]].astype(np.int64)
        cls = np.digitize(d, [65, 129, 256])                 # 0: <= 64, 1: 65-128, 2: 129-255, 3: longer
        cls[0] = -1                                          # rank 0 is never processed
        counts += np.bincount(cls[1:], minlength=4)
        pad = np.full((-len(cls)) % 4, -1, dtype=cls.dtype)
        g = np.concatenate([cls, pad]).reshape(-1, 4)
        hi = g.max(axis=1)
        lo = np.where(g < 0, 99, g).min(axis=1)
        mixed += int(np.count_nonzero((hi >= 0) & (lo != hi)))
    return counts, mixed


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    """Per (set, clusterThreshold): the set's records on disk, the oracle's .hash and the set's list classes — made once."""
    root = tmp_path_factory.mktemp("dense_rounds")
    made = {}

    def get(name, ct):
        if (name, ct) not in made:
            gen, (lo, hi), _, _ = SETS[name]
            fqb = os.path.join(str(root), name + ".fqb")
            if not os.path.exists(fqb):
                orc.gen_fqb(fqb, *gen)
            out = "orc_%s_%d.hash" % (name, ct)
            o = run_commands(lambda k, w, r, b: orc.Oracle(k, w, r, b),
                             ["-k", K, "-w", W, "-r", R, "-B", B, "-ct", ct, "--readFQB", name + ".fqb", "--hashDepthRange", lo, hi, "--cluster", 1, 0,
                              "--writeHash", out], str(root))
            counts, mixed = _list_classes(o)
            o.close()
            made[(name, ct)] = (str(root), open(os.path.join(str(root), out), "rb").read(), counts, mixed)
        return made[(name, ct)]
    return get


def _check(reference, name, ct, **opts):
    import hash10x_amd
    cwd, exp, counts, mixed = reference(name, ct)
    _, (lo, hi), classes, want_mixed = SETS[name]
    # the set still has the lists this case is about (a changed generator must not empty the test)
    for c, wanted in enumerate(classes):
        assert (counts[c] > 0) == wanted, "set %s: %d lists in length class %d" % (name, counts[c], c)
    assert counts[3] == 0, "set %s: lists of 256 entries and more" % name
    assert (mixed > 0) == want_mixed, "set %s: %d groups of four ranks mix length classes" % (name, mixed)

    h = hash10x_amd.Hash10x(k=K, w=W, r=R, B=B)
    for n, v in opts.items():
        h.set_option(n, v)
    h.read_fqb(np.fromfile(os.path.join(cwd, name + ".fqb"), dtype=np.uint32), 0, 100000)
    h.depth_range(lo, hi)
    h.cluster(1, 0, ct)
    assert h.counters()["cluster_first_mode"] == 0
    out = os.path.join(cwd, "hip_%s.hash" % name)
    h.write_hash(out)
    h.close()
    got = open(out, "rb").read()
    assert got == exp, orc.describe_diff(got, exp)
    return orc.HashFile(got)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_dense_rounds_default(reference, name):
    hf = _check(reference, name, DEFAULT_CT[name])
    assert hf.blocks["nSubCluster"].sum() > 0


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_dense_rounds_narrow_first(reference, name):
    """first[] at 2 bytes per entry in every block: the CAS-min form of the loop."""
    _check(reference, name, DEFAULT_CT[name], cluster_narrow_first=1)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_dense_rounds_small_lds_budget(reference, name):
    """40 KB of LDS per workgroup: fewer list-loop waves per block, so the rounds fall differently."""
    _check(reference, name, DEFAULT_CT[name], cluster_lds_budget=40 * 1024)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_dense_rounds_512_threads(reference, name):
    _check(reference, name, DEFAULT_CT[name], cluster_threads0=512)


def test_dense_rounds_every_list_active(reference):
    """clusterThreshold 1: a rank with any usable entry is active."""
    _check(reference, "A", 1)


def test_dense_rounds_no_list_active(reference):
    """clusterThreshold 50: no rank is active, every result word says so."""
    hf = _check(reference, "A", 50)
    assert hf.blocks["nSubCluster"].sum() == 0
