"""--shareComponents on the GPU (csrc/stage_m.hip): Hash10x.share_components against the plain-Python model of the definition
(tests/comp_model.py over tests/share_model.py), over thresholds, budgets and block ranges, on a split state, an unsplit one and hand-made
blocks; the refusals; the .sc file and the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import comp_model
import orc

pytestmark = pytest.mark.gpu

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
NAMES = ("comp", "root", "rootOf", "blocks", "records")
TOP = 2 ** 31 - 1


_hx, _budget, _molecules, _load_image, GEN = orc.hx, orc.set_budget, orc.molecules, orc.load_image, orc.GEN_MOLECULES


def _same(got, exp, what):
    assert len(got) == len(exp) == 5
    for g, e, name in zip(got, exp, NAMES):
        assert g.dtype == e.dtype and np.array_equal(g, e), (what, name, g.tolist(), e.tolist())


def _bytes(res):
    return b"".join(a.tobytes() for a in res)


def _kept(h):
    return h._hip.h10x_share_components_get(h._ctx(), None, None, None, None, None, 0, 0) == 0


def _check_info(h, res, rows, t):
    info = h.share_components_info
    n, largest, single, _ = comp_model.figures(res)
    assert (info["nBlocks"], info["minShare"], info["rows"]) == (len(res[0]), t, rows), info
    assert (info["nComponents"], info["largest"], info["singletons"]) == (n, largest, single), info
    assert info["hookRounds"] >= (1 if rows else 0) and info["batches"] >= 1


# ------------------------------------------------------------------------------------ the inputs, loaded once, with their models
@pytest.fixture(scope="module")
def gen_recs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sc"))
    return d, orc.gen_fqb(os.path.join(d, "x.fqb"), *GEN)


@pytest.fixture(scope="module")
def generated(gen_recs):
    """the molecules of the generated set (the state of the CPU test's reference run) and the model's answers, computed once"""
    d, recs = gen_recs
    h = _molecules(recs)
    h.depth_range(2, 40)
    cm = comp_model.CompModel.from_state(h)
    exp = {t: cm.components(t) for t in (1, 50, 100, TOP)}
    yield h, cm, exp, d
    h.close()


@pytest.fixture(scope="module")
def small():
    recs = np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32)
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(3, 14)
    yield h, comp_model.CompModel.from_state(h)
    h.close()


# ------------------------------------------------------------------------------------ agreement with the model
def test_generated_set(generated):
    h, cm, exp, _ = generated
    assert cm.n_blocks == 31 == h.sizes()["nBlocks"]
    # the figures of the CPU test, which come from the reference binary's state
    table = {1: (158, 3, 28, 2, 1), 50: (66, 6, 25, 5, 1), 100: (38, 15, 9, 11, 4), TOP: (0, 30, 1, 30, 0)}
    for t, figs in table.items():
        assert (cm.rows(t),) + comp_model.figures(exp[t]) == figs, t
    images = {}
    for budget in (0, 64):
        _budget(h, budget)
        for step in (4, 7, 0):
            h.set_option("share_graph_blocks", step)
            for t in (1, 50, 100, TOP):
                got = h.share_components(t)
                _same(got, exp[t], (budget, step, t))
                _check_info(h, got, cm.rows(t), t)
                if budget:                                     # far below the largest block: windows of barcode index inside the ranges
                    assert h.share_components_info["windows"] > 0
                images.setdefault(t, set()).add(_bytes(got))
                if step == 0:
                    assert _bytes(h.share_components(t)) == _bytes(got), ("a second identical call", budget, t)
    _budget(h, 0)
    assert all(len(v) == 1 for v in images.values())           # every combination: the same bytes
    comp, root, root_of, blocks, records = exp[100]
    assert 1 < len(blocks) - 1 < cm.n_blocks - 1 and int((blocks[1:] >= 3).sum()) >= 2   # neither everything joined nor nothing
    assert np.array_equal(exp[TOP][0], np.arange(cm.n_blocks)) and np.array_equal(exp[TOP][3][1:], np.ones(cm.n_blocks - 1))


def test_unsplit_small(small):
    h, cm = small
    assert cm.n_blocks == 41
    seen = set()
    for t in (1, 50, 200):
        exp = cm.components(t)
        seen.add(len(exp[3]))
        for budget, step in ((0, 0), (64, 4), (0, 7)):
            _budget(h, budget)
            h.set_option("share_graph_blocks", step)
            got = h.share_components(t)
            _same(got, exp, (t, budget, step))
            _check_info(h, got, cm.rows(t), t)
    _budget(h, 0)
    h.set_option("share_graph_blocks", 0)
    assert len(seen) > 1                                       # the thresholds cut the graph differently


# ------------------------------------------------------------------------------------ hand-made states
def test_chain(tmp_path):
    """300 blocks in a chain; link i - (i + 1) is two private hashes for even i, one for odd i. Block numbers are a fixed permutation of the
    chain positions: neighbours lie in different ranges, and the smaller root is often the far end. At 4 blocks a range, components meet
    only through later ranges."""
    n = 300
    number = np.random.RandomState(20240).permutation(n) + 1   # block number of chain position i
    blocks = [[] for _ in range(n)]
    share = np.zeros((n + 1, n + 1), dtype=np.int64)
    nxt = 1
    for i in range(n - 1):
        for _ in range(2 if i % 2 == 0 else 1):
            blocks[number[i] - 1].append(nxt)
            blocks[number[i + 1] - 1].append(nxt)
            nxt += 1
        share[number[i], number[i + 1]] = share[number[i + 1], number[i]] = 2 if i % 2 == 0 else 1
    n_hash = [0] + [len(b) for b in blocks]
    h = _load_image(tmp_path, blocks)
    exp1, exp2 = comp_model.components(share, n_hash, 1), comp_model.components(share, n_hash, 2)
    assert exp1[3].tolist() == [0, 300] and exp1[2].tolist() == [0, 1] and not (exp1[1][1:] != 1).any()
    assert exp2[3].tolist() == [0] + [2] * 150 and sorted(set(exp2[1][1:].tolist())) == exp2[2][1:].tolist()
    for step in (4, 0):
        h.set_option("share_graph_blocks", step)
        got = h.share_components(1)
        _same(got, exp1, ("chain, T = 1", step))
        _check_info(h, got, 2 * (n - 1), 1)
        assert h.share_components_info["largest"] == 300 and h.share_components_info["singletons"] == 0
        if step:
            assert h.share_components_info["batches"] >= 75    # 301 blocks, 4 a range
        got = h.share_components(2)
        _same(got, exp2, ("chain, T = 2", step))
        _check_info(h, got, 2 * (n // 2), 2)
        assert h.share_components_info["nComponents"] == 150 and h.share_components_info["largest"] == 2
    h.close()


def test_directed_only_link(tmp_path):
    """Block 1 has 65540 records — hash 1, hash 2 and filler of depth 1 — so it has no good hashes and its own row is empty (hash10x.c:748).
    Block 2 holds hash 1, block 3 holds hash 2; 2 and 3 share nothing. Block 1 stands in the rows of 2 and 3, and those entries alone join all
    three under root 1."""
    filler = np.arange(10, 10 + 65538)
    blocks = [np.concatenate([[1, 2], filler]), [1, 7], [2, 8]]
    h = _load_image(tmp_path, blocks)
    off, blk, cnt = h.share_graph(1)
    assert off.tolist() == [0, 0, 1, 2] and blk.tolist() == [1, 1]      # an empty row for block 1, block 1 in both others
    for step in (0, 1):
        h.set_option("share_graph_blocks", step)
        comp, root, root_of, members, records = h.share_components(1)
        assert comp.tolist() == [0, 1, 1, 1] and root.tolist() == [0, 1, 1, 1]
        assert root_of.tolist() == [0, 1] and members.tolist() == [0, 3] and records.tolist() == [0, 65540 + 2 + 2]
        assert records.dtype == np.uint64 and comp.dtype == root.dtype == root_of.dtype == members.dtype == np.uint32
        assert h.share_components_info["rows"] == 2
    comp, root, root_of, members, records = h.share_components(2)
    assert comp.tolist() == [0, 1, 2, 3] and members.tolist() == [0, 1, 1, 1] and records.tolist() == [0, 65540, 2, 2]
    h.close()


def test_star(tmp_path):
    """a hub (block 101) shares one private hash with each of 200 leaves: one component of 201, and every hook contends on one word"""
    hub = 101
    leaves = [c for c in range(1, 202) if c != hub]
    blocks = [[] for _ in range(201)]
    for x, c in enumerate(leaves, start=1):
        blocks[c - 1].append(x)
        blocks[hub - 1].append(x)
    h = _load_image(tmp_path, blocks)
    for step in (0, 7):
        h.set_option("share_graph_blocks", step)
        comp, root, root_of, members, records = h.share_components(1)
        assert comp.tolist() == [0] + [1] * 201 and root.tolist() == [0] + [1] * 201
        assert root_of.tolist() == [0, 1] and members.tolist() == [0, 201] and records.tolist() == [0, 400]
        assert h.share_components_info["rows"] == 400 and h.share_components_info["largest"] == 201
    comp = h.share_components(2)[0]
    assert comp.tolist() == list(range(202))
    h.close()


def test_singletons_and_an_empty_block(tmp_path):
    """Blocks 1, 2, 3 hold hashes of depth 1 only (none in range), block 6 has no records at all: each is a component of its own, the empty one
    with 0 records. Blocks 4 and 5 share a hash, so the state has a good hash at all."""
    blocks = [[1, 2], [3], [4, 5, 6], [7, 8], [7, 9], []]
    h = _load_image(tmp_path, blocks)
    comp, root, root_of, members, records = h.share_components(1)
    assert comp.tolist() == [0, 1, 2, 3, 4, 4, 5] and root.tolist() == [0, 1, 2, 3, 4, 4, 6]
    assert root_of.tolist() == [0, 1, 2, 3, 4, 6] and members.tolist() == [0, 1, 1, 1, 2, 1] and records.tolist() == [0, 2, 1, 3, 4, 0]
    info = h.share_components_info
    assert (info["nComponents"], info["largest"], info["singletons"], info["rows"]) == (5, 2, 4, 2)
    h.close()


# ------------------------------------------------------------------------------------ refusals
def test_refusals(small, gen_recs):
    err = _hx().Hash10xError
    h = _hx().Hash10x(B=20)
    with pytest.raises(err, match="no hash state loaded"):
        h.share_components(5)
    h.close()
    recs = np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32)
    h2 = _hx().Hash10x(B=20)
    h2.read_fqb(recs)
    with pytest.raises(err, match="!! you must set hashDepthRange before shareComponents"):
        h2.share_components(5)
    assert not _kept(h2)
    h2.close()
    h, _ = small
    h.share_components(5)
    assert _kept(h)
    for bad in (0, -3):
        with pytest.raises(err, match="!! shareComponents minShare %d must be >= 1" % bad):
            h.share_components(bad)
        assert not _kept(h)                                    # a refused run keeps no result behind, nor an earlier one
        h.share_components(5)
        assert _kept(h)
    h.depth_range(3, 14)                                       # a new range releases it
    assert not _kept(h)
    # after --clusterSplit the lists are of the old blocks until a new range is set
    h3 = _hx().Hash10x(B=21)
    h3.read_fqb(gen_recs[1])
    h3.depth_range(2, 40)
    h3.share_components(5)
    assert _kept(h3)
    h3.cluster(1, 0, 3)
    h3.cluster_split()
    assert not _kept(h3)
    with pytest.raises(err, match="!! you must set hashDepthRange before shareComponents"):
        h3.share_components(5)
    assert not _kept(h3)
    h3.depth_range(2, 40)
    h3.share_components(5)
    assert _kept(h3)
    # the pieces of the C ABI out of order
    ctx = h3._ctx()
    assert h3._hip.h10x_share_components_begin(ctx, 5) == 0 and not _kept(h3)
    assert h3._hip.h10x_share_components_add(ctx, 1, 0) == 0
    z = np.zeros(16, dtype=np.uint64)
    assert h3._hip.h10x_share_components_finish(ctx, z.ctypes.data) == 0 and _kept(h3)
    assert h3._hip.h10x_share_components_add(ctx, 1, 0) != 0 and b"add without begin" in h3._hip.h10x_last_error(ctx)
    assert h3._hip.h10x_share_components_finish(ctx, z.ctypes.data) != 0
    h3.close()


# ------------------------------------------------------------------------------------ the file and the command line
SUMMARY = re.compile(r"^  share components at minShare (\d+): (\d+) blocks, (\d+) rows, (\d+) components, largest (\d+) blocks, (\d+) singletons$", re.M)


def test_written_file_in_ranges(generated):
    """the session's walk over block ranges, at 4 and 7 blocks a range and in one piece: the same file, and what share_components returns"""
    h, cm, exp, d = generated
    images = []
    for step in (4, 7, 0):
        h.set_option("share_graph_blocks", step)
        p = os.path.join(d, "walk%d.sc" % step)
        h.write_share_components(100, p, out=os.path.join(d, "walk%d.out" % step))
        info, comp, root_of, blocks, records = _hx().read_share_components(p)
        assert info == {"version": 1, "nBlocks": 31, "minShare": 100, "nComponents": 15, "largest": 9, "rows": 38}
        got = h.share_components(100)
        _same((comp, got[1], root_of, blocks, records), got, step)
        _same(got, exp[100], step)
        m = SUMMARY.search(open(os.path.join(d, "walk%d.out" % step)).read())
        assert m and [int(v) for v in m.groups()] == [100, 31, 38, 15, 9, 11]
        z = h.share_components_info
        assert [int(v) for v in m.groups()] == [z["minShare"], z["nBlocks"], z["rows"], z["nComponents"], z["largest"], z["singletons"]]
        images.append(open(p, "rb").read())
    assert images[0] == images[1] == images[2]


def test_cli(generated):
    h, cm, exp, d = generated
    base = [EXE, "-B", "21", "-ct", "3", "--readFQB", "x.fqb"]
    mol = ["--hashDepthRange", 2, 40, "--cluster", 1, 0, "--clusterSplit", "--hashDepthRange", 2, 40]

    def run(*args):
        p = subprocess.run(base + [str(a) for a in args], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        return p.returncode, p.stdout.decode(), p.stderr.decode()

    rc, out, err = run(*mol, "--shareComponents", 100, "x.sc")
    assert rc == 0, err
    info, comp, root_of, blocks, records = _hx().read_share_components(os.path.join(d, "x.sc"))
    e = exp[100]
    _same((comp, e[1], root_of, blocks, records), e, "cli")
    m = SUMMARY.search(out)
    assert m and [int(v) for v in m.groups()] == [100, 31, 38, 15, 9, 11]
    assert (info["nBlocks"], info["rows"], info["nComponents"], info["largest"]) == (31, 38, 15, 9)
    assert out[m.end():].lstrip("\n").startswith("  user")      # the resource line follows
    # with -o the summary line goes to the file (behind the echo of the command's arguments, which ends without a newline: hash10x.c:1166-1171)
    rc, out, err = run("-o", "sc.out", *mol, "--shareComponents", 100, "y.sc")
    assert rc == 0 and "share components at minShare" not in out
    assert " 100 y.sc" + m.group(0) + "\n" in open(os.path.join(d, "sc.out")).read()
    assert open(os.path.join(d, "y.sc"), "rb").read() == open(os.path.join(d, "x.sc"), "rb").read()
    # soft errors: the message, nothing done, no file, exit status 0
    rc, out, err = run("--shareComponents", 50, "early.sc")
    assert rc == 0 and "!! you must set hashDepthRange before shareComponents\n" in out and not os.path.exists(os.path.join(d, "early.sc"))
    p = subprocess.run([EXE, "-B", "21", "--shareComponents", "50", "nostate.sc"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and b"!! you must set hashDepthRange before shareComponents\n" in p.stdout and not os.path.exists(os.path.join(d, "nostate.sc"))
    rc, out, err = run("-o", "soft.out", "--hashDepthRange", 2, 40, "--shareComponents", 0, "zero.sc", "--cluster", 1, 0, "--clusterSplit", "--shareComponents", 5, "late.sc")
    assert rc == 0, err
    for msg in ("!! shareComponents minShare 0 must be >= 1\n", "!! you must set hashDepthRange before shareComponents\n"):
        assert msg in err and msg in open(os.path.join(d, "soft.out")).read()
    assert not os.path.exists(os.path.join(d, "zero.sc")) and not os.path.exists(os.path.join(d, "late.sc"))
    # --interactive takes it too
    script = b"readFQB x.fqb\nhashDepthRange 2 40\ncluster 1 0\nclusterSplit\nhashDepthRange 2 40\nshareComponents 100 i.sc\nquit\n"
    p = subprocess.run(base[:5] + ["--interactive"], input=script, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and open(os.path.join(d, "i.sc"), "rb").read() == open(os.path.join(d, "x.sc"), "rb").read()
    p = subprocess.run([EXE, "--gpus", "2", "-B", "21", "--readFQB", "x.fqb", "--hashDepthRange", "2", "40", "--shareComponents", "50", "s.sc"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 255 and "FATAL ERROR: --shareComponents does not run on a sharded session (--gpus 2)" in p.stderr.decode()
    assert not os.path.exists(os.path.join(d, "s.sc"))
