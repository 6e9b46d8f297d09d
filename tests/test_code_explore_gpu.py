"""--codeExplore (codeExplore, hash10x.c:1351-1470) on the GPU: the barcode census (h10x_code_share) and the one-code re-clustering
(h10x_code_explore) against literal NumPy restatements, and the command line against the reference binary."""
import os
import re
import subprocess

import numpy as np
import pytest

import orc

pytestmark = pytest.mark.gpu

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")


_hx, _budget = orc.hx, orc.set_budget


# ------------------------------------------------------------------------------------ NumPy restatement
class State:
    """blocks, ClusterHash records, hashWithinRange and hashDepth as exported; hashCodes[x] = the blocks of x's records, ascending."""

    def __init__(self, h):
        self.blocks = h.export_blocks()
        self.ch = h.export_clushash()
        nh = self.blocks["nHash"].astype(np.int64)
        self.off = np.concatenate([[0], np.cumsum(nh)])
        self.hash = self.ch["hash"].astype(np.int64)
        self.within = h.export_within().astype(bool)
        self.depth = h.export_depth().astype(np.int64)
        blk = np.repeat(np.arange(len(nh)), nh)
        order = np.argsort(self.hash, kind="stable")         # records are in block order: each hash's blocks ascending
        self.hs, self.bs = self.hash[order], blk[order]

    def good(self, code):
        """goodHashesBuild (hash10x.c:738-766): positions of the in-range hashes, by depth, ties by position"""
        a, b = self.off[code], self.off[code + 1]
        if b - a > 65535:
            return np.zeros(0, np.int64)
        pos = np.nonzero(self.within[self.hash[a:b]])[0]
        return pos[np.argsort(self.depth[self.hash[a + pos]], kind="stable")]

    def lists(self, code):
        g = self.good(code)
        xs = self.hash[self.off[code] + g]
        lo, hi = np.searchsorted(self.hs, xs, "left"), np.searchsorted(self.hs, xs, "right")
        return g, xs, [self.bs[l:r] for l, r in zip(lo, hi)]

    def share(self, code):
        """countShare[cj] > 0 and first[cj] (hash10x.c:1371-1382), ascending in cj, with the hash at rank first[cj]"""
        g, xs, L = self.lists(code)
        if not len(g):
            return [np.zeros(0, np.int64)] * 4
        ranks = np.repeat(np.arange(len(g)), [len(l) for l in L])
        cj = np.concatenate(L)
        keep = cj != code
        ranks, cj = ranks[keep], cj[keep]
        u, inv, cnt = np.unique(cj, return_inverse=True, return_counts=True)
        first = np.full(len(u), 1 << 30, np.int64)
        np.minimum.at(first, inv, ranks)
        return u, cnt, first, xs[first]


def read_merge(lab, reads, n_sub):
    """codeClusterReadMerge (hash10x.c:837-868) restated literally; labels above nSubCluster (stale, of an earlier clustering) stay
    out of it and as they are, as --cluster keeps them"""
    read_map = {}
    true = list(range(n_sub + 1))
    dead = [0] * (n_sub + 1)
    for i in range(len(lab)):
        L = int(lab[i])
        if L > n_sub:
            continue
        hc = true[L]
        if not hc:
            continue
        r = int(reads[i])
        rc = true[read_map.get(r, 0)]
        if hc == rc:
            continue
        if not rc:
            read_map[r] = hc
        else:
            if hc > rc:
                hc, rc = rc, hc
            for j in range(1, n_sub + 1):
                if true[j] == rc:
                    true[j] = hc
            dead[rc] = 1
    for j in range(1, n_sub + 1):
        dead[j] = dead[j - 1] + 1 - dead[j]
    for j in range(1, n_sub + 1):
        true[j] = dead[true[j]]
    out = lab.copy()
    for i in range(len(lab)):
        if lab[i] <= n_sub:
            out[i] = true[int(lab[i])]
    return out, dead[n_sub]


def explore(st, code, thr):
    """steps 1-4 of codeExplore (hash10x.c:1361-1436): (labels of the block's records, nSubCluster, pointToMin, clustered, raw,
    abandoned), or None for a barcode without good hashes (nothing changes)"""
    g, xs, L = st.lists(code)
    n = len(g)
    if not n:
        return None
    a = st.off[code]
    lab = st.ch["subCluster"][a:st.off[code + 1]].astype(np.int64).copy()
    lab[g] = 0
    first = np.full(len(st.blocks), -1, np.int64)
    rank_lab = np.zeros(n, np.int64)
    n_sub, clustered, p, abandoned, cmin = 0, 0, 0.0, False, {}
    for i in range(n):
        l = L[i][L[i] != code]
        first[l[first[l] < 0]] = i
        msc = np.bincount(first[l], minlength=i + 1)
        if i == 0:
            continue
        c = msc[:i]
        if int(c.max()) < thr:
            continue
        best, tot = int(np.argmax(c)), int(c.sum())
        if not rank_lab[best]:
            n_sub += 1
            if n_sub > 255:
                n_sub, clustered, abandoned = 0, 0, True
                rank_lab[:] = 0
                break
            rank_lab[best] = n_sub
            cmin[n_sub] = best
            clustered += 1
        rank_lab[i] = rank_lab[best]
        clustered += 1
        p += int(msc[cmin[int(rank_lab[i])]]) / float(tot)
    lab[g] = rank_lab
    raw = n_sub
    if n_sub:
        lab, n_sub = read_merge(lab, st.ch["read"][a:st.off[code + 1]], n_sub)
    return lab, n_sub, p, clustered, raw, abandoned


# ------------------------------------------------------------------------------------ the census
def _check_share(h, st, codes):
    got = h.code_share(codes)
    for code, r in zip(codes, got):
        u, cnt, first, fh = st.share(code)
        assert np.array_equal(r["barcode"], u), code
        assert np.array_equal(r["count"], cnt), code
        assert np.array_equal(r["firstRank"], first), code
        assert np.array_equal(r["firstHash"], fh), code


def _both_budgets(h, st):
    codes = list(range(len(st.blocks))) + [1, 1]                # every barcode (block 0 too), and a repeat
    _check_share(h, st, codes)
    h.neighbour_stats(reset=True)
    _budget(h, 64)                                             # far below the largest barcode: many batches, and windows of barcode index
    _check_share(h, st, codes)
    s = h.neighbour_stats(reset=True)
    assert s["windows"] > 0 and s["batches"] > 2, s
    _budget(h, 0)


def _small():
    recs = np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32)
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    return h


def test_share_small_golden():
    h = _small()
    h.depth_range(3, 14)
    _both_budgets(h, State(h))
    h.close()


def test_share_generated(tmp_path):
    recs = orc.gen_fqb(str(tmp_path / "g.fqb"), 6000, 30, 60000, 0.003, 7, 4.0, 150, 6000)
    h = _hx().Hash10x(B=21)
    h.read_fqb(recs)
    h.depth_range(2, 40)
    _both_budgets(h, State(h))
    h.close()


# ------------------------------------------------------------------------------------ the re-clustering
def _check_explore(h, code, thr):
    st = State(h)
    exp = explore(st, code, thr)
    rep = h.code_explore(code, thr)
    after = State(h)
    others = np.ones(len(st.ch), bool)
    others[st.off[code]:st.off[code + 1]] = False
    assert np.array_equal(after.ch["subCluster"][others], st.ch["subCluster"][others]), "labels outside block %d" % code
    bo = np.arange(len(st.blocks)) != code
    assert np.array_equal(after.blocks[bo], st.blocks[bo]), "other blocks"
    assert rep["nGood"] == len(st.good(code)) and rep["nHash"] == int(st.blocks["nHash"][code])
    if exp is None:
        assert np.array_equal(after.ch, st.ch) and np.array_equal(after.blocks.view(np.uint8), st.blocks.view(np.uint8)), code
        return rep
    lab, n_sub, p, clustered, raw, abandoned = exp
    got = after.ch["subCluster"][st.off[code]:st.off[code + 1]]
    assert np.array_equal(got, lab), (code, thr, np.nonzero(got != lab)[0][:10])
    assert int(after.blocks["nSubCluster"][code]) == n_sub == rep["merged"], (code, thr)
    assert np.float64(after.blocks["pointToMin"][code]).tobytes() == np.float64(p).tobytes(), (code, thr, after.blocks["pointToMin"][code], p)
    assert (rep["clustered"], rep["raw"], rep["abandoned"]) == (clustered, raw, int(abandoned)), (code, thr, rep)
    u, cnt, _, _ = st.share(code)
    assert rep["nShare"] == len(u) and rep["histMax"] == (int(cnt.max()) if len(cnt) else 0)
    return rep


def test_explore_generated(tmp_path):
    recs = orc.gen_fqb(str(tmp_path / "g.fqb"), 5000, 24, 40000, 0.003, 11, 4.0, 150, 5000)
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(3, 30)
    st = State(h)
    ngood = np.array([len(st.good(c)) for c in range(len(st.blocks))])
    largest = int(np.argmax(st.blocks["nHash"]))
    assert ngood[0] == 0
    seen = set()
    for thr in (2, 5, 9):
        for code in (0, 1, largest, 5, 17):
            rep = _check_explore(h, code, thr)
            seen.add(rep["raw"] > 0)
    assert seen == {True, False}
    # after --cluster of every barcode and a second range (ranges accumulate): the explored block's earlier labels are replaced
    h.cluster(1, 0, 3)
    h.depth_range(10, 20)
    for code in (1, largest, 9):
        _check_explore(h, code, 3)
    h.close()


def test_explore_budget_and_abandon(tmp_path):
    p = str(tmp_path / "a.hash")
    with open(p, "wb") as f:
        f.write(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "abort255.in.hash.gz")))
    h = _hx().Hash10x(B=20)
    h.read_hash(p)
    h.depth_range(2, 100)
    _budget(h, 64)                                             # the pairs of a windowed census
    rep = _check_explore(h, 1, 5)
    assert rep["abandoned"] == 1 and rep["merged"] == 0
    assert h.export_blocks()["pointToMin"][1] > 0                # the partial sum stands
    h.close()


def test_explore_errors():
    h = _small()
    err = _hx().Hash10xError
    with pytest.raises(err, match="!! you must set hashDepthRange before codeExplore"):
        h.code_explore(1)
    with pytest.raises(err, match="before codeShare"):
        h.code_share([1])
    h.depth_range(3, 14)
    nb = h.sizes()["nBlocks"]
    with pytest.raises(err, match="!! codeExplore code %d outside 0 to %d" % (nb, nb)):
        h.code_explore(nb)
    with pytest.raises(err, match="!! codeExplore code -1 outside"):
        h.code_explore(-1)
    with pytest.raises(err, match=r"!! clusterThreshold 0 must be >= 1"):
        h.code_explore(1, 0)
    with pytest.raises(err, match="not below nBlocks"):
        h.code_share([nb])
    with pytest.raises(err, match="needs --cribBuild"):
        h.code_crib_counts([1])
    h.cluster(1, 0, 3)
    h.cluster_split()
    with pytest.raises(err, match="!! you must set hashDepthRange before codeExplore"):
        h.code_explore(1)
    h.close()


# ------------------------------------------------------------------------------------ command line vs the reference binary
# The lines of the command and of the commands whose state it changes; the reading commands word their progress lines differently
# here (tests/soak_cli.py), and the resource lines are masked.
CE_LINE = re.compile(r"^(  code \d+ with |COUNT_SHARE_|  CLUSTER_SUMMARY |    CODE_CLUSTER |  MIN_POINT_DENSITY |  SHARE code |"
                     r"CODE_(SIZE|CLUSTER)_|!! |    code \d+ with \d+ good hashes has too many|FATAL ERROR| then \d+ merged)")


def _mask(b):
    return [ln for ln in b.decode(errors="replace").splitlines() if CE_LINE.match(ln)]


def _run_both(d, args, with_o=False, hash_out=None):
    a_ref = (["-o", "out.ref"] if with_o else []) + args + (["--writeHash", "ref.hash"] if hash_out else [])
    a_hip = (["-o", "out.hip"] if with_o else []) + args + (["--writeHash", "hip.hash"] if hash_out else [])
    ref = orc.run_ref(a_ref, d)
    hip = subprocess.run([EXE] + [str(a) for a in a_hip], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert hip.returncode == ref.returncode, (args, hip.stderr[-400:], ref.stderr[-400:])
    got, exp = _mask(hip.stdout), _mask(ref.stdout)
    assert got == exp, (args, next(((a, b) for a, b in zip(got, exp) if a != b), (len(got), len(exp))))
    assert _mask(hip.stderr) == _mask(ref.stderr), (args, _mask(hip.stderr), _mask(ref.stderr))
    if with_o:
        g, e = _mask(open(os.path.join(d, "out.hip"), "rb").read()), _mask(open(os.path.join(d, "out.ref"), "rb").read())
        assert g == e, (args, next(((a, b) for a, b in zip(g, e) if a != b), (len(g), len(e))))
    if hash_out:
        gh = orc.canonical_hash_bytes(open(os.path.join(d, "hip.hash"), "rb").read())
        rh = orc.canonical_hash_bytes(open(os.path.join(d, "ref.hash"), "rb").read())
        assert gh == rh, (args, orc.describe_diff(gh, rh))
    return hip, ref


@pytest.fixture(scope="module")
def gen_set(tmp_path_factory):
    if not orc.have_ref():
        pytest.fail("reference binary missing: build() makes oracle/_ref")
    d = str(tmp_path_factory.mktemp("cecli"))
    recs = orc.gen_fqb(os.path.join(d, "x.fqb"), 5000, 24, 40000, 0.003, 11, 4.0, 150, 5000, fa=os.path.join(d, "x"))
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    largest = int(np.argmax(h.export_blocks()["nHash"]))
    nb = h.sizes()["nBlocks"]
    h.close()
    return dict(dir=d, largest=largest, nBlocks=nb)


def test_cli_explore(gen_set):
    d, big = gen_set["dir"], gen_set["largest"]
    base = ["-B", 20, "--readFQB", "x.fqb", "--hashDepthRange", 3, 30, "--cribBuild", "x.A.fa", "x.B.fa"]
    for with_o in (False, True):
        hip, _ = _run_both(d, base + ["-ct", 2, "--codeExplore", 1, "--codeExplore", 5, "--codeExplore", big, "--codeExplore", 0,
                                      "-ct", 5, "--codeExplore", 17, "--clusterReport", 0, 0, "--codeStats"], with_o, hash_out=True)
        assert b"SHARE code" in (open(os.path.join(d, "out.hip"), "rb").read() if with_o else hip.stdout)
    _run_both(d, base + ["-ct", 3, "--cluster", 1, 0, "--codeExplore", 1, "--codeExplore", 9, "--clusterReport", 1, 0], True, hash_out=True)
    _run_both(d, ["-B", 20, "--readFQB", "x.fqb", "--codeExplore", 3], True)              # before any range: the reference's message
    _run_both(d, ["-B", 20, "-ct", 2] + base[2:] + ["--codeExplore", 1, "--clusterSplit", "--hashDepthRange", 3, 30, "--cluster", 1, 0], hash_out=True)


def test_cli_abandon(tmp_path):
    if not orc.have_ref():
        pytest.fail("reference binary missing: build() makes oracle/_ref")
    d = str(tmp_path)
    with open(os.path.join(d, "abort255.hash"), "wb") as f:
        f.write(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "abort255.in.hash.gz")))
    hip, ref = _run_both(d, ["-B", 20, "--readHash", "abort255.hash", "--hashDepthRange", 2, 100, "--codeExplore", 1], hash_out=True)
    assert b"code 1 with 600 good hashes has too many clusters" in ref.stderr


def test_cli_undefined_cases_and_shards(gen_set):
    d, nb = gen_set["dir"], gen_set["nBlocks"]
    base = [EXE, "-B", 20, "--readFQB", "x.fqb"]

    def run(*args):
        p = subprocess.run([str(a) for a in base + list(args)], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        return p.returncode, p.stdout.decode(), p.stderr.decode()

    rc, out, err = run("--hashDepthRange", 3, 30, "--cribBuild", "x.A.fa", "x.B.fa", "--codeExplore", nb, "--codeExplore", -1, "-ct", 0, "--codeExplore", 1)
    assert rc == 0, err
    for msg in ("!! codeExplore code %d outside 0 to %d" % (nb, nb), "!! codeExplore code -1 outside 0 to %d" % nb,
                "!! clusterThreshold 0 must be >= 1 (the reference reads an uninitialised msBest otherwise)"):
        assert msg + "\n" in out, msg
    assert "  code " not in out
    # no crib: everything before the SHARE lines, then the message; the state change stands
    rc, out, err = run("-ct", 2, "--hashDepthRange", 3, 30, "--codeExplore", 1, "--writeHash", "nocrib.hash")
    assert rc == 0, err
    lines = out.splitlines()
    i = lines.index("!! codeExplore needs --cribBuild for its SHARE lines")
    assert lines[i - 1].startswith("  MIN_POINT_DENSITY") and "SHARE code" not in out
    ref = orc.run_ref(["-B", 20, "-ct", 2, "--readFQB", "x.fqb", "--hashDepthRange", 3, 30, "--cribBuild", "x.A.fa", "x.B.fa", "--codeExplore", 1,
                       "--writeHash", "crib.hash"], d)
    assert ref.returncode == 0
    assert orc.canonical_hash_bytes(open(os.path.join(d, "nocrib.hash"), "rb").read()) == \
        orc.canonical_hash_bytes(open(os.path.join(d, "crib.hash"), "rb").read())
    # after --clusterSplit until a new range
    rc, out, err = run("-o", "split.out", "--hashDepthRange", 3, 30, "--cluster", 1, 0, "--clusterSplit", "--codeExplore", 1)
    assert rc == 0 and "!! you must set hashDepthRange before codeExplore\n" in err
    assert "!! you must set hashDepthRange before codeExplore\n" in open(os.path.join(d, "split.out")).read()
    p = subprocess.run([EXE, "--gpus", "2", "-B", "20", "--readFQB", "x.fqb", "--hashDepthRange", "3", "30", "--codeExplore", "1"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 255 and "FATAL ERROR: --codeExplore does not run on a sharded session (--gpus 2)" in p.stderr.decode()


def test_cli_interactive(gen_set):
    d = gen_set["dir"]
    script = b"readFQB x.fqb\ncodeExplore 1\nhashDepthRange 3 30\ncribBuild x.A.fa x.B.fa\ncodeExplore 1\nclusterThreshold 2\ncodeExplore 1\ncodeExplore 7\nquit\n"
    env = dict(os.environ, MALLOC_PERTURB_="255", GLIBC_TUNABLES="glibc.malloc.tcache_count=0")
    args = ["-B", "20", "--interactive"]
    ref = subprocess.run([os.path.join(orc.REF_DIR, "hash10x")] + args, input=script, cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    hip = subprocess.run([EXE] + args, input=script, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert hip.returncode == ref.returncode == 0
    got, exp = _mask(hip.stdout), _mask(ref.stdout)
    assert got == exp and any(ln.startswith("  SHARE code") for ln in got), next(((a, b) for a, b in zip(got, exp) if a != b), (len(got), len(exp)))
    assert _mask(hip.stderr) == _mask(ref.stderr)
