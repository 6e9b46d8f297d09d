"""The neighbour commands (--hashInfo, --hashExplore, --doubleShared, --errorFix, --shareScan; hash10x.c:541-718) on the GPU:
the census ABI against an independent NumPy restatement, and the command line against the reference binary."""
import os
import re
import subprocess

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")


_hx, _budget = orc.hx, orc.set_budget


# ------------------------------------------------------------------------------------ NumPy restatement of the census
class Census:
    """c_x(h) from the exported blocks + ClusterHash records and hashWithinRange."""

    def __init__(self, h):
        blocks = h.export_blocks(); ch = h.export_clushash()
        n = int(blocks["nHash"].sum())
        self.hash = ch["hash"][:n].astype(np.int64)
        self.block = np.repeat(np.arange(len(blocks)), blocks["nHash"].astype(np.int64))
        self.within = h.export_within().astype(bool)
        self.depth = h.export_depth()

    def pairs(self, x):
        blk = self.block[self.hash == x]
        m = np.isin(self.block, blk) & (self.hash != x) & self.within[self.hash]
        return np.unique(self.hash[m], return_counts=True)

    def first_code(self, hs):
        order = np.lexsort((self.block, self.hash))
        hsorted, bsorted = self.hash[order], self.block[order]
        return bsorted[np.searchsorted(hsorted, hs)]


def _queries(cs, rng):
    """random in-range and out-of-range hashes of every depth class, the deepest hash, one with an empty N(x), repeats"""
    d = cs.depth.astype(np.int64)
    qs = []
    for lo, hi in ((1, 2), (2, 3), (3, 5), (5, 10), (10, 30), (30, 1 << 30)):
        idx = np.nonzero((d >= lo) & (d < hi))[0]
        if len(idx):
            qs += list(rng.choice(idx, size=min(4, len(idx)), replace=False))
    qs.append(int(np.argmax(d)))
    empty = [x for x in np.nonzero(d > 0)[0][:2000] if len(cs.pairs(x)[0]) == 0]
    qs += empty[:1]                                # (test_census_empty covers an empty N(x) where the data has none)
    qs += qs[:3]
    return [int(q) for q in qs]


def _check(h, cs, qs):
    mk, nn = h.neighbour_max(qs)
    hists = h.neighbour_hist(qs, cs.depth)
    for i, x in enumerate(qs):
        eh, ec = cs.pairs(x)
        gh, gc, gf = h.neighbours(x)
        assert np.array_equal(gh, eh) and np.array_equal(gc, ec), "list of %d" % x
        if len(eh):
            assert np.array_equal(gf, cs.first_code(eh)), "first codes of %d" % x
        assert nn[i] == len(eh), "|N(%d)|" % x
        exp = max(((int(c) & 0xFFFF) << 32) | int(hh) for hh, c in zip(eh, ec)) if len(eh) else 0
        assert int(mk[i]) == exp, "max of %d" % x
        eh_hist = np.bincount(ec, minlength=int(cs.depth[x]) + 1) if len(ec) else np.zeros(int(cs.depth[x]) + 1, np.int64)
        assert np.array_equal(hists[i], eh_hist), "histogram of %d" % x


def _both_budgets(h, cs, qs):
    _check(h, cs, qs)
    h.neighbour_stats(reset=True)
    _budget(h, 64)                                 # far below the deepest query: many batches, and windows of hash index
    _check(h, cs, qs)
    st = h.neighbour_stats(reset=True)
    assert st["windows"] > 0 and st["batches"] > len(set(qs)), st
    _budget(h, 0)


def _small(tmpdir_path=None):
    recs = np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32)
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    return h


def test_census_small_golden():
    h = _small()
    h.depth_range(3, 14)
    cs = Census(h)
    qs = _queries(cs, np.random.default_rng(1))
    _both_budgets(h, cs, qs)
    h.close()


def test_census_empty():
    """nothing in range: every N(x) is empty (the list has no entry, max 0 with |N| = 0, an all-zero histogram)"""
    h = _small()
    d = h.export_depth()
    h.depth_range(int(d.max()) + 1, int(d.max()) + 2)
    cs = Census(h)
    qs = [int(np.argmax(d)), 1, 2, 1]
    _check(h, cs, qs)
    mk, nn = h.neighbour_max(qs)
    assert not nn.any() and not mk.any()
    h.close()


def test_census_generated_split_and_hash_file(tmp_path):
    path = str(tmp_path / "g.fqb")
    recs = orc.gen_fqb(path, 6000, 30, 60000, 0.003, 7, 4.0, 150, 6000)
    h = _hx().Hash10x(B=21)
    h.read_fqb(recs)
    h.depth_range(2, 40)
    cs = Census(h)
    qs = _queries(cs, np.random.default_rng(2))
    _both_budgets(h, cs, qs)
    h.cluster(1, 0, 3)
    h.cluster_split()                              # the split blocks, hashCodes rebuilt
    cs = Census(h)
    _both_budgets(h, cs, qs)
    hp = str(tmp_path / "g.hash")
    h.write_hash(hp)
    h.close()
    h2 = _hx().Hash10x(B=21)
    h2.read_hash(hp)
    h2.depth_range(2, 40)
    cs2 = Census(h2)
    _both_budgets(h2, cs2, qs)
    h2.close()


def test_census_needs_depth_range():
    h = _small()
    with pytest.raises(_hx().Hash10xError, match="without hashDepthRange"):
        h.neighbour_max([5])
    h.depth_range(3, 14)
    with pytest.raises(_hx().Hash10xError, match="not below hashNumber"):
        h.neighbour_max([h.sizes()["hashNumber"]])
    h.close()


# ------------------------------------------------------------------------------------ command line vs the reference binary
# The lines of the five commands. The other commands' lines are compared by their own tests (the reading commands word their
# progress lines differently here, tests/soak_cli.py), and so is the command echo, which the reference writes to the -o file with
# the previous command's arguments in front of it. Resource lines are masked.
NB_LINE = re.compile(r"^(HASH_INFO  |  \d+ hashes sharing codes with |    \d+ sharing \d+ codes|  hash \d+ +code |SHARE_SCAN |"
                     r"  \d+\S* count \d+ max \d+ score |  (err|htA|htB|hom|mul) low \d+ n |.*called without hashDepthRange|FATAL ERROR)")


def _mask(b):
    return [re.sub(r"user\t.*", "user", ln).replace("out.hip", "OUT").replace("out.ref", "OUT")
            for ln in b.decode(errors="replace").splitlines() if NB_LINE.match(ln)]


def _run_both(d, args, with_o=False):
    a_ref = ["-o", "out.ref"] + args if with_o else args
    a_hip = ["-o", "out.hip"] + args if with_o else args
    ref = orc.run_ref(a_ref, d)
    hip = subprocess.run([EXE] + [str(a) for a in a_hip], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert hip.returncode == ref.returncode, (args, hip.stderr[-400:], ref.stderr[-400:])
    got, exp = _mask(hip.stdout), _mask(ref.stdout)
    assert got == exp, (args, next(((a, b) for a, b in zip(got, exp) if a != b), (len(got), len(exp))))
    assert _mask(hip.stderr) == _mask(ref.stderr), args
    if with_o:
        assert _mask(open(os.path.join(d, "out.hip"), "rb").read()) == _mask(open(os.path.join(d, "out.ref"), "rb").read()), args
    return hip


@pytest.fixture(scope="module")
def gen_set(tmp_path_factory):
    if not orc.have_ref():
        pytest.fail("reference binary missing: build() makes oracle/_ref")
    d = str(tmp_path_factory.mktemp("nbcli"))
    recs = orc.gen_fqb(os.path.join(d, "x.fqb"), 5000, 24, 40000, 0.003, 11, 4.0, 150, 5000, fa=os.path.join(d, "x"))
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(3, 30)
    z = h.sizes()
    d_ = h.export_depth()
    within = h.export_within()
    ins = np.nonzero(within)[0]
    deep = int(ins[np.argmax(d_[ins])])
    mk, nn = h.neighbour_max([deep])
    partner = int(mk[0] & 0xFFFFFFFF)
    h.close()
    return dict(dir=d, hashNumber=z["hashNumber"], deep=deep, partner=partner, mid=int(ins[len(ins) // 2]))


def test_cli_hash_info_explore_double(gen_set):
    d, n = gen_set["dir"], gen_set["hashNumber"]
    base = ["-B", 20, "--readFQB", "x.fqb", "--hashDepthRange", 3, 30]
    for with_o in (False, True):
        _run_both(d, base + ["--hashInfo", 1, n, 7], with_o)
        _run_both(d, base + ["--hashExplore", gen_set["deep"], "--hashExplore", gen_set["mid"], "--hashExplore", 1,
                             "--doubleShared", gen_set["deep"], gen_set["partner"], "--doubleShared", gen_set["mid"], gen_set["deep"]], with_o)


def test_cli_crib_error_fix_share_scan(gen_set):
    d, n = gen_set["dir"], gen_set["hashNumber"]
    base = ["-B", 20, "--readFQB", "x.fqb", "--hashDepthRange", 3, 30, "--cribBuild", "x.A.fa", "x.B.fa"]
    for with_o in (False, True):
        _run_both(d, base + ["--hashInfo", 1, min(n, 4000), 13, "--hashExplore", gen_set["deep"], "--errorFix", 1, n, "--shareScan", 3, 30], with_o)
    _run_both(d, base + ["--cluster", 1, 0, "--clusterSplit", "--hashInfo", 1, n, 11, "--hashExplore", gen_set["deep"],
                         "--doubleShared", gen_set["deep"], gen_set["partner"], "--errorFix", 1, n, "--shareScan", 3, 30], True)


def test_cli_reference_messages(gen_set):
    d = gen_set["dir"]
    base = ["-B", 20, "--readFQB", "x.fqb"]
    _run_both(d, base + ["--hashInfo", 1, 10, 1, "--hashExplore", 5, "--doubleShared", 5, 6])
    hip = _run_both(d, base + ["--hashDepthRange", 3, 30, "--errorFix", 1, 100])
    assert hip.returncode == 255 and b"FATAL ERROR: need to set crib" in hip.stderr


def test_cli_undefined_cases_and_shards(gen_set):
    d, n = gen_set["dir"], gen_set["hashNumber"]
    base = [EXE, "-B", 20, "--readFQB", "x.fqb"]

    def run(*args):
        p = subprocess.run([str(a) for a in base + list(args)], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        return p.returncode, p.stdout.decode(), p.stderr.decode()

    rc, out, err = run("--errorFix", 1, 10, "--shareScan", 3, 5)                      # no crib: the reference dies first
    assert rc == 255 and "FATAL ERROR: need to set crib" in err
    rc, out, err = run("--shareScan", 3, 5)                                             # no range: the reference dereferences NULL
    assert rc == 0 and "shareScan called without hashDepthRange\n" in err
    rc, out, err = run("--hashDepthRange", 3, 30, "--cribBuild", "x.A.fa", "x.B.fa", "--errorFix", 1, n + 5, "--hashInfo", 0, n + 1, 1,
                       "--hashInfo", 1, 5, 0, "--hashExplore", n, "--doubleShared", -1, 3, "--shareScan", 0, 5, "--shareScan", 5, 5)
    assert rc == 0, err
    for msg in ("!! errorFix range 1 to %d outside 0 to %d" % (n + 5, n), "!! hashInfo range 0 to %d outside 0 to %d" % (n + 1, n),
                "!! hashInfo skip 0 must be positive", "!! hashExplore hash %d outside 0 to %d" % (n, n),
                "!! doubleShared hashes -1 3 outside 0 to %d" % n, "!! shareScan needs 0 < countMin < countMax, not 0 5",
                "!! shareScan needs 0 < countMin < countMax, not 5 5"):
        assert msg + "\n" in out, msg
    assert "HASH_INFO" not in out
    # a depth-0 hash inside the range (--hashDepthRange 0 ...): its line carries no census
    rc, out, err = run("--hashDepthRange", 0, 30, "--hashInfo", 0, 1, 1)
    assert rc == 0 and "HASH_INFO  0-0\n" in out
    p = subprocess.run([EXE, "--gpus", "2", "-B", "20", "--readFQB", "x.fqb", "--hashDepthRange", "3", "30", "--hashInfo", "1", "5", "1"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 255 and "FATAL ERROR: --hashInfo does not run on a sharded session (--gpus 2)" in p.stderr.decode()
