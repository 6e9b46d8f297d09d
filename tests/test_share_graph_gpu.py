"""--shareGraph on the GPU (csrc/stage_l.hip): Hash10x.share_graph against the NumPy model of the definition (tests/share_model.py) and
against the existing barcode census (code_share), over thresholds, budgets, sub-ranges, a split state and hand-made blocks; the refusals;
the command line and the .sg file."""
import os
import re
import subprocess

import numpy as np
import pytest

import orc
import share_model

pytestmark = pytest.mark.gpu

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
THRESHOLDS = (1, 50, 200, 2 ** 31 - 1)


_hx, _budget = orc.hx, orc.set_budget


def _same(got, exp, what):
    for g, e, name in zip(got, exp, ("offsets", "block", "count")):
        assert g.dtype == e.dtype and np.array_equal(g, e), (what, name)


# ------------------------------------------------------------------------------------ the inputs, loaded once, with their models
def _load(recs, B, lo, hi):
    h = _hx().Hash10x(B=B)
    h.read_fqb(recs)
    h.depth_range(lo, hi)
    return h


@pytest.fixture(scope="module")
def small():
    recs = np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32)
    h = _load(recs, 20, 3, 14)
    yield h, share_model.ShareModel.from_state(h), (41, 37582, 734, 308, 12, 258), recs
    h.close()


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    recs = orc.gen_fqb(str(tmp_path_factory.mktemp("sg") / "g.fqb"), 6000, 30, 60000, 0.003, 7, 4.0, 150, 6000)
    h = _load(recs, 21, 2, 40)
    yield h, share_model.ShareModel.from_state(h), (31, 100672, 656, 486, 166, 951), recs
    h.close()


# ------------------------------------------------------------------------------------ agreement with the model and the census
def _agreement(h, model, figures, _recs):
    n_blocks, entries, rows1, rows50, rows200, max_count = figures
    assert model.n_blocks == n_blocks == h.sizes()["nBlocks"]
    assert int(model.list_entries[1:].sum()) == entries and int(model.share.max()) == max_count
    census = h.code_share(list(range(1, n_blocks)))
    results = {}
    for budget in (0, 64):
        _budget(h, budget)
        h.neighbour_stats(reset=True)
        for t in THRESHOLDS:
            got = h.share_graph(t)
            info = h.share_graph_info
            _same(got, model.graph(t), (budget, t))
            _same(h.share_graph(t), got, ("a second identical call", budget, t))
            assert info["rows"] == len(got[1]) == int(got[0][-1]) and info["listEntries"] == entries and info["nBlocks"] == n_blocks
            assert info["maxCount"] == (int(got[2].max()) if len(got[2]) else 0)
            assert (info["codeMin"], info["codeMax"]) == (1, n_blocks)
            results[(budget, t)] = got
            if t == 1:                                         # the rows of h10x_code_share for the same codes
                assert np.array_equal(got[1], np.concatenate([r["barcode"] for r in census]))
                assert np.array_equal(got[2], np.concatenate([r["count"] for r in census]))
                assert np.array_equal(np.diff(got[0].astype(np.int64)), [len(r["barcode"]) for r in census])
                assert info["maxCount"] == max_count
        s = h.neighbour_stats(reset=True)
        if budget:                                             # far below the largest block: many batches, and windows of barcode index
            assert s["windows"] > 0 and s["batches"] > 2, s
            assert h.share_graph_info["windows"] > 0 and h.share_graph_info["batches"] > 2
        else:
            assert s["windows"] == 0 and s["batches"] == 2 * len(THRESHOLDS), s   # one batch a call, two calls a threshold
    _budget(h, 0)
    for t in THRESHOLDS:
        _same(results[(64, t)], results[(0, t)], t)
    n1, n50, n200, ntop = (len(results[(0, t)][1]) for t in THRESHOLDS)
    assert (n1, n50, n200, ntop) == (rows1, rows50, rows200, 0)
    assert 0 < n200 < n50 < n1                                 # a filter that keeps everything, or nothing, cannot pass
    assert not results[(0, THRESHOLDS[-1])][0].any()           # T = 2^31 - 1: all-zero offsets
    assert len(results[(0, THRESHOLDS[-1])][0]) == n_blocks


def test_agreement_small(small):
    _agreement(*small)


def test_agreement_generated(generated):
    _agreement(*generated)


def test_sub_ranges(small):
    h, model, _, _ = small
    nb = model.n_blocks
    for t in (1, 50):
        for lo, hi in ((5, 9), (nb - 1, nb), (7, 7), (1, 0), (5, 0), (0, 3), (9, 5)):
            got = h.share_graph(t, lo, hi)
            _same(got, model.graph(t, lo, hi), (t, lo, hi))
            assert len(got[0]) == max((hi or nb) - lo, 0) + 1
    got = h.share_graph(1, 7, 7)
    assert got[0].tolist() == [0] and len(got[1]) == 0 and len(got[2]) == 0
    _budget(h, 64)
    _same(h.share_graph(50, 5, 9), model.graph(50, 5, 9), "windowed sub-range")
    _budget(h, 0)


def test_after_cluster_split(generated):
    """the molecule graph: after --cluster and --clusterSplit the lists are of the old blocks until a new range is set"""
    h0, _, _, recs = generated
    before = h0.sizes()["nBlocks"]
    h = _load(recs, 21, 2, 40)                                 # a context of its own: the shared one stays as it is
    h.cluster(1, 0, 3)
    h.cluster_split()
    with pytest.raises(_hx().Hash10xError, match="!! you must set hashDepthRange before shareGraph"):
        h.share_graph(5)
    h.depth_range(2, 40)
    assert h.sizes()["nBlocks"] > before
    model = share_model.ShareModel.from_state(h)
    assert model.n_blocks == h.sizes()["nBlocks"]
    rows = []
    for t in (1, 5, 50):
        got = h.share_graph(t)
        _same(got, model.graph(t), t)
        rows.append(len(got[1]))
    assert rows[0] > rows[1] > rows[2] > 0
    _budget(h, 64)
    _same(h.share_graph(5), model.graph(5), "budget 64")
    h.close()


# ------------------------------------------------------------------------------------ a hand-made state
def test_hand_made_state(tmp_path):
    """Block 1 holds hash 1 twice: its lists are walked twice, and every list holds block 1 twice. Block 3 has 65540 records: no good
    hashes of its own (hash10x.c:748), so its row is empty, yet it stands in the rows of blocks 1 and 2. Hashes 1 and 2 have 4 records
    each (the range 2 .. 100), every other hash one."""
    filler = np.arange(10, 10 + 65538)
    blocks = [[1, 1, 2, 3], [1, 2, 2, 4], np.concatenate([[1, 2], filler])]
    p = tmp_path / "state.hash"
    p.write_bytes(orc.hash_image(blocks))
    h = _hx().Hash10x(B=20)
    h.read_hash(str(p))
    h.depth_range(2, 100)
    assert h.export_blocks()["nHash"].tolist() == [0, 4, 4, 65540]
    # by hand: block 1's good records are 1, 1, 2; list of hash 1 = [1, 1, 2, 3], of hash 2 = [1, 2, 2, 3]
    off, blk, cnt = h.share_graph(1)
    assert off.tolist() == [0, 2, 4, 4]
    assert blk.tolist() == [2, 3, 1, 3] and cnt.tolist() == [4, 3, 4, 3]
    model = share_model.ShareModel.from_state(h)
    assert model.share[3].sum() == 0 and model.share[1, 3] == 3
    for t in (1, 4, 5):
        _same(h.share_graph(t), model.graph(t), t)
    assert h.share_graph(4)[1].tolist() == [2, 1]
    census = h.code_share([1, 2, 3])
    assert [r["count"].tolist() for r in census] == [[4, 3], [4, 3], []]
    h.close()


def test_wide_keys(tmp_path):
    """65540 blocks in one batch: keyBits(nBlocks) = 17 and keyBits(nq - 1) = 17, 34 bits, so the tail runs on 64-bit keys. Block b holds hashes b and
    b + 1, so blocks b and b + 1 share hash b + 1 once; a block of DOUBLED holds hash b + 1 twice, which makes that count 2 in both rows. Hash X stands 60
    times in block HEAVY and 30 times in block PARTNER: 1800 in both rows, and HEAVY's lists hold 5404 entries, above the budget of the second pass, so it
    runs alone in windows while the other blocks run some 250 to a batch. The expected rows are stated here, not taken from the dense model."""
    n, doubled, heavy, partner = 65540, (3, 1000, 32768, 65000), 20000, 50000
    x = n + 2
    blocks = [[b, b + 1] + [b + 1] * (b in doubled) for b in range(1, n + 1)]
    blocks[heavy - 1] += [x] * 60
    blocks[partner - 1] += [x] * 30
    h = orc.load_image(tmp_path, blocks, 2, 100)
    assert h.sizes()["nBlocks"] == n + 1 and (n + 1).bit_length() + (n - 1).bit_length() == 34
    # every (row, block, count): neighbours b and b + 1 both ways, HEAVY and PARTNER both ways
    b = np.arange(1, n, dtype=np.int64)
    m = np.where(np.isin(b, doubled), 2, 1)
    row = np.concatenate([b, b + 1, [heavy, partner]])
    other = np.concatenate([b + 1, b, [partner, heavy]])
    count = np.concatenate([m, m, [1800, 1800]])
    order = np.lexsort((other, row))
    row, other, count = row[order], other[order], count[order]
    for budget in (0, 4000):
        _budget(h, budget)
        for t in (1, 2, 3):
            keep = count >= t
            off = np.concatenate([[0], np.cumsum(np.bincount(row[keep] - 1, minlength=n))]).astype(np.uint64)
            _same(h.share_graph(t), (off, other[keep].astype(np.uint32), count[keep].astype(np.uint32)), (budget, t))
            info = h.share_graph_info
            assert info["rows"] == int(keep.sum()) == (2 * (n - 1) + 2, 2 * len(doubled) + 2, 2)[t - 1]
            assert info["listEntries"] == int(count.sum()) and info["maxCount"] == 1800 and (info["codeMin"], info["codeMax"]) == (1, n + 1)
            if budget:
                assert info["windows"] >= 2 and info["batches"] > 60, info
            else:
                assert (info["batches"], info["windows"]) == (1, 0), info
    _budget(h, 0)
    h.close()


# ------------------------------------------------------------------------------------ refusals
def test_refusals(small):
    err = _hx().Hash10xError
    h = _hx().Hash10x(B=20)
    with pytest.raises(err, match="no hash state loaded"):
        h.share_graph(5)
    h.close()
    h, model, _, _ = small
    with pytest.raises(err, match="!! shareGraph minShare 0 must be >= 1"):
        h.share_graph(0)
    with pytest.raises(err, match="!! shareGraph minShare -3 must be >= 1"):
        h.share_graph(-3)
    nb = model.n_blocks
    with pytest.raises(err, match="!! shareGraph codeMax %d beyond nBlocks %d" % (nb + 1, nb)):
        h.share_graph(5, 1, nb + 1)
    # a refused run keeps no graph behind; neither does a new range
    assert h._hip.h10x_share_graph_get(h._ctx(), None, None, None, 0) != 0
    h.share_graph(5)
    assert h._hip.h10x_share_graph_get(h._ctx(), None, None, None, 0) == 0
    h.depth_range(3, 14)
    assert h._hip.h10x_share_graph_get(h._ctx(), None, None, None, 0) != 0
    recs = np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32)
    h2 = _hx().Hash10x(B=20)
    h2.read_fqb(recs)
    with pytest.raises(err, match="!! you must set hashDepthRange before shareGraph"):
        h2.share_graph(5)
    h2.close()


# ------------------------------------------------------------------------------------ the file and the command line
SUMMARY = re.compile(r"^  share graph at minShare (\d+): (\d+) blocks, (\d+) rows, (\d+) list entries, max count (\d+)$", re.M)


@pytest.fixture(scope="module")
def third(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sgcli"))
    recs = orc.gen_fqb(os.path.join(d, "x.fqb"), 5000, 24, 40000, 0.003, 11, 4.0, 150, 5000)
    h = _load(recs, 20, 3, 30)
    yield d, h
    h.close()


def test_written_file_in_ranges(third):
    """the session's walk over block ranges, at 4 and 7 blocks a range and in one piece: the same file"""
    d, h = third
    exp = h.share_graph(50, 0, 0)
    assert (len(exp[0]), len(exp[1]), int(exp[2].max())) == (26, 416, 726)
    images = []
    for step in (4, 7, 0):
        h.set_option("share_graph_blocks", step)
        p = os.path.join(d, "walk%d.sg" % step)
        h.write_share_graph(50, p, out=os.path.join(d, "walk%d.out" % step))
        info, off, blk, cnt = _hx().read_share_graph(p)
        assert info == {"version": 1, "nBlocks": 25, "minShare": 50, "rows": 416}
        _same((off, blk, cnt), exp, step)
        m = SUMMARY.search(open(os.path.join(d, "walk%d.out" % step)).read())
        assert m and [int(v) for v in m.groups()] == [50, 25, 416, 100686, 726]
        images.append(open(p, "rb").read())
    assert images[0] == images[1] == images[2]


def test_cli(third):
    d, h = third
    exp = h.share_graph(50, 0, 0)
    base = [EXE, "-B", "20", "--readFQB", "x.fqb"]

    def run(*args):
        p = subprocess.run(base + [str(a) for a in args], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        return p.returncode, p.stdout.decode(), p.stderr.decode()

    rc, out, err = run("--hashDepthRange", 3, 30, "--shareGraph", 50, "x.sg")
    assert rc == 0, err
    info, off, blk, cnt = _hx().read_share_graph(os.path.join(d, "x.sg"))
    _same((off, blk, cnt), exp, "cli")
    m = SUMMARY.search(out)
    assert m and [int(v) for v in m.groups()] == [50, info["nBlocks"], info["rows"], h.share_graph_info["listEntries"], int(exp[2].max())]
    assert [int(v) for v in m.groups()] == [50, 25, 416, 100686, 726]
    assert out[m.end():].lstrip("\n").startswith("  user")      # the resource line follows
    # with -o the summary line goes to the file (behind the echo of the command's arguments, which ends without a newline: hash10x.c:1166-1171)
    rc, out, err = run("-o", "sg.out", "--hashDepthRange", 3, 30, "--shareGraph", 50, "y.sg")
    assert rc == 0 and "share graph at minShare" not in out
    assert " 50 y.sg" + m.group(0) + "\n" in open(os.path.join(d, "sg.out")).read()
    assert open(os.path.join(d, "y.sg"), "rb").read() == open(os.path.join(d, "x.sg"), "rb").read()
    # soft errors: the message, nothing done, exit status 0
    rc, out, err = run("--shareGraph", 50, "early.sg")
    assert rc == 0 and "!! you must set hashDepthRange before shareGraph\n" in out and not os.path.exists(os.path.join(d, "early.sg"))
    rc, out, err = run("-o", "soft.out", "--hashDepthRange", 3, 30, "--shareGraph", 0, "zero.sg", "--cluster", 1, 0, "--clusterSplit", "--shareGraph", 5, "late.sg")
    assert rc == 0, err
    for msg in ("!! shareGraph minShare 0 must be >= 1\n", "!! you must set hashDepthRange before shareGraph\n"):
        assert msg in err and msg in open(os.path.join(d, "soft.out")).read()
    assert not os.path.exists(os.path.join(d, "zero.sg")) and not os.path.exists(os.path.join(d, "late.sg"))
    # --interactive takes it too
    p = subprocess.run(base[:3] + ["--interactive"], input=b"readFQB x.fqb\nhashDepthRange 3 30\nshareGraph 50 i.sg\nquit\n", cwd=d,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and open(os.path.join(d, "i.sg"), "rb").read() == open(os.path.join(d, "x.sg"), "rb").read()
    p = subprocess.run([EXE, "--gpus", "2", "-B", "20", "--readFQB", "x.fqb", "--hashDepthRange", "3", "30", "--shareGraph", "50", "s.sg"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 255 and "FATAL ERROR: --shareGraph does not run on a sharded session (--gpus 2)" in p.stderr.decode()
