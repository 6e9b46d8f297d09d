"""--hashCopies on the GPU (csrc/stage_n.hip): Hash10x.hash_copies against the plain-Python model of the definition (tests/copies_model.py
over tests/share_model.py), over thresholds and budgets, on a split state, an unsplit one and hand-made blocks; the refusals; the .hc file
and the command line."""
import os
import re
import subprocess

import numpy as np
import pytest

import copies_model
import orc

pytestmark = pytest.mark.gpu

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
TOP = 2 ** 31 - 1


_hx, _budget, _molecules, _load_image, GEN = orc.hx, orc.set_budget, orc.molecules, orc.load_image, orc.GEN_MOLECULES


def _same(got, exp, what):
    assert got.dtype == exp.dtype == np.uint16 and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        bad = np.flatnonzero((got != exp).any(axis=1))
        raise AssertionError((what, len(bad), [(int(x), got[x].tolist(), exp[x].tolist()) for x in bad[:8]]))


def _kept(h):
    return h._hip.h10x_hash_copies_get(h._ctx(), None, 0, 0) == 0


def _check_info(h, cm, table, t):
    info = h.hash_copies_info
    in_range, one, split, deepest = cm.tallies(table)
    assert (info["hashNumber"], info["minShare"], info["rows"]) == (cm.hash_number, t, cm.rows(t)), info
    assert (info["inRange"], info["oneGroup"], info["split"], info["deepest"]) == (in_range, one, split, deepest), info
    assert info["batches"] >= 1
    tally = h.hash_copies_tally()                                # no crib: everything under class 0
    assert tally.dtype == np.uint64 and tally.tolist() == [[in_range, one, split]] + [[0, 0, 0]] * 4


# ------------------------------------------------------------------------------------ the inputs, loaded once, with their models
@pytest.fixture(scope="module")
def gen_recs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("hc"))
    return d, orc.gen_fqb(os.path.join(d, "x.fqb"), *GEN, fa=os.path.join(d, "x"))   # (the two haplotypes beside it, for --cribBuild)


@pytest.fixture(scope="module")
def generated(gen_recs):
    """the molecules of the generated set (the state of the CPU test's reference run) and the model's answers, computed once"""
    d, recs = gen_recs
    h = _molecules(recs)
    h.depth_range(2, 40)
    cm = copies_model.CopiesModel.from_state(h)
    exp = {t: cm.table(t) for t in (1, 50, 100, TOP)}
    yield h, cm, exp, d
    h.close()


def _against_model(h, cm, exp, what):
    for budget in (0, 64):
        _budget(h, budget)
        for t, e in exp.items():
            got = h.hash_copies(t)
            _same(got, e, (what, budget, t))
            _check_info(h, cm, e, t)
            if budget:                                         # far below the largest block: windows of barcode index inside the census
                assert h.hash_copies_info["windows"] > 0
            assert h.hash_copies(t).tobytes() == got.tobytes(), ("a second identical call", what, budget, t)
    _budget(h, 0)


def test_generated_set(generated):
    h, cm, exp, _ = generated
    assert cm.model.n_blocks == 31 == h.sizes()["nBlocks"]
    # the tallies of the CPU test, which come from the reference binary's state
    pinned = {1: (3433, 3433, 0, 5), 50: (3433, 2675, 0, 5), 100: (3433, 1898, 0, 5), TOP: (3433, 0, 0, 5)}
    for t, figs in pinned.items():
        assert cm.tallies(exp[t]) == figs, t
    _against_model(h, cm, exp, "generated")


def test_unsplit_small():
    recs = np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32)
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    h.depth_range(3, 14)
    cm = copies_model.CopiesModel.from_state(h)
    assert cm.model.n_blocks == 41
    exp = {t: cm.table(t) for t in (1, 50, 100, TOP)}
    assert len({e.tobytes() for e in exp.values()}) > 2        # the thresholds cut the lists differently
    _against_model(h, cm, exp, "small")
    h.close()


# ------------------------------------------------------------------------------------ hand-made states
def _model_of(blocks, lo=2, hi=100):
    hashes = np.concatenate([np.asarray(b, dtype=np.int64) for b in blocks])
    depth = np.bincount(hashes)
    return copies_model.CopiesModel([0] + [len(b) for b in blocks], hashes, (depth >= lo) & (depth < hi))


def test_two_loci(tmp_path):
    """Blocks 1-3 hold hashes 10, 11, 12, blocks 4-6 hold 20, 21, 22, all six hold hash 1 (block 1 also hash 30, of depth 1). Inside a locus
    two blocks share 4, across the loci only hash 1."""
    blocks = [[1, 10, 11, 12, 30]] + [[1, 10, 11, 12]] * 2 + [[1, 20, 21, 22]] * 3
    h, cm = _load_image(tmp_path, blocks), _model_of(blocks)
    t1, t2, t5 = h.hash_copies(1), h.hash_copies(2), h.hash_copies(5)
    assert t1.shape == (31, 4) and t1[1].tolist() == [6, 1, 6, 0]
    assert t2[1].tolist() == [6, 2, 3, 3] and t2[10].tolist() == [3, 1, 3, 0] and t2[22].tolist() == [3, 1, 3, 0]
    assert t5[1].tolist() == [6, 6, 1, 1] and t5[10].tolist() == [3, 3, 1, 1]
    for got, t in ((t1, 1), (t2, 2), (t5, 5)):
        assert not got[30].any() and not got[0].any() and not got[2:10].any()     # depth 1, index 0, no records
        _same(got, cm.table(t), ("two loci", t))
    _check_info(h, cm, t5, 5)
    assert (h.hash_copies_info["inRange"], h.hash_copies_info["oneGroup"], h.hash_copies_info["split"], h.hash_copies_info["deepest"]) == (7, 0, 0, 6)
    h.hash_copies(2)
    assert (h.hash_copies_info["oneGroup"], h.hash_copies_info["split"]) == (6, 1)
    h.close()


@pytest.mark.parametrize("n", [130, 64, 65])
def test_chain_longer_than_a_wave(tmp_path, n):
    """n blocks under a fixed permutation of block numbers all hold hash 1, chain neighbours share two private hashes more: at T = 3 one
    group of n (the smallest label crosses lanes and takes many hooks), at T = 4 n groups."""
    number = np.random.RandomState(20241).permutation(n) + 1   # block number of chain position i
    blocks = [[1] for _ in range(n)]
    nxt = 2
    for i in range(n - 1):
        for _ in range(2):
            blocks[number[i] - 1].append(nxt)
            blocks[number[i + 1] - 1].append(nxt)
            nxt += 1
    h, cm = _load_image(tmp_path, blocks, 2, 200), _model_of(blocks, 2, 200)
    t3, t4 = h.hash_copies(3), h.hash_copies(4)
    assert t3[1].tolist() == [n, 1, n, 0] and t4[1].tolist() == [n, n, 1, 1]
    assert h.hash_copies(1)[1].tolist() == [n, 1, n, 0]
    _same(t3, cm.table(3), ("chain", n, 3))
    _same(t4, cm.table(4), ("chain", n, 4))
    assert t3[2].tolist() == [2, 1, 2, 0] and t4[2].tolist() == [2, 2, 1, 1]      # a private hash: its two blocks share 3
    h.close()


def test_long_rows_beside_a_short_list(tmp_path):
    """Blocks 1 and 2 hold hash 1. Block 1 also shares hashes 2 and 3 with blocks 3 .. 302, block 2 hashes 4 and 5 with blocks 303 .. 602,
    none of which holds hash 1: the rows of 1 and 2 are 300 entries and more, all misses but one at T = 1 and all misses at T = 2."""
    blocks = [[1, 2, 3], [1, 4, 5]] + [[2, 3]] * 300 + [[4, 5]] * 300
    h, cm = _load_image(tmp_path, blocks, 2, 1000), _model_of(blocks, 2, 1000)
    t1, t2, t3 = h.hash_copies(1), h.hash_copies(2), h.hash_copies(3)
    assert t1[1].tolist() == [2, 1, 2, 0] and t2[1].tolist() == [2, 2, 1, 1]
    assert t2[2].tolist() == [301, 1, 301, 0] and t3[4].tolist() == [301, 301, 1, 1]   # the holders of a private pair share exactly those two
    for got, t in ((t1, 1), (t2, 2), (t3, 3)):
        _same(got, cm.table(t), ("long rows", t))
    off, blk, cnt = h.share_graph(2)
    assert int(off[1] - off[0]) == 300 and int(off[2] - off[1]) == 300 and 2 not in blk[:300].tolist()
    h.close()


def test_repeats(tmp_path):
    """Block 1 holds hash 1 twice: the list of hash 1 has 4 entries and 3 distinct blocks, and the repeat counts twice in the shares."""
    blocks = [[1, 1, 5], [1, 5], [1, 6], [6, 7], [7, 5]]
    h, cm = _load_image(tmp_path, blocks), _model_of(blocks)
    assert cm.lists[0].tolist() == [1, 1, 2, 3] and cm.deepest == 4
    assert cm.model.share[1, 2] == 3 and cm.model.share[2, 1] == 3 and cm.model.share[1, 3] == 2     # 2 x hash 1 + hash 5; 2 x hash 1
    for t in (1, 2, 3, 4):
        got = h.hash_copies(t)
        _same(got, cm.table(t), ("repeats", t))
        assert got[1, 0] == 3
        _check_info(h, cm, got, t)
    assert h.hash_copies(3)[1].tolist() == [3, 2, 2, 1] and h.hash_copies(4)[1].tolist() == [3, 3, 1, 1]
    h.close()


def test_a_block_above_65535_records(tmp_path):
    """Block 1 has 65540 records (hashes 1, 2, 3 and filler of depth 1): no good hashes, an empty row of its own (hash10x.c:748). Block 2 holds
    hash 1, block 3 hash 2: block 1 stands in their rows and is joined through them. Block 4 is as large and holds hash 3: the list of hash 3 has
    only such blocks, nothing joins them, also at T = 1."""
    blocks = [np.concatenate([[1, 2, 3], np.arange(10, 10 + 65537)]), [1, 7], [2, 8], np.concatenate([[3], np.arange(70000, 70000 + 65539)])]
    assert len(blocks[0]) == len(blocks[3]) == 65540
    h = _load_image(tmp_path, blocks)
    off, blk, cnt = h.share_graph(1)
    assert off.tolist() == [0, 0, 1, 2, 2] and blk.tolist() == [1, 1]
    t1 = h.hash_copies(1)
    assert t1[1].tolist() == [2, 1, 2, 0] and t1[2].tolist() == [2, 1, 2, 0] and t1[3].tolist() == [2, 2, 1, 1]
    assert not t1[4:].any() and not t1[0].any()
    info = h.hash_copies_info
    assert (info["inRange"], info["oneGroup"], info["split"], info["deepest"], info["rows"]) == (3, 2, 0, 2, 2)
    assert h.hash_copies(2)[1].tolist() == [2, 2, 1, 1]
    _same(t1, _model_of(blocks).table(1), "a large block")
    h.close()


# ------------------------------------------------------------------------------------ refusals
def test_depth_cap(tmp_path):
    """Hash 1 in 4097 blocks, hash 2 in 4096 of them, hash 3 in two. With hash 1 in range the whole command is refused; with the range cut
    below it the same image runs, and hash 2 fills a wave's LDS to the limit."""
    blocks = [[1, 2, 3], [1, 2, 3]] + [[1, 2]] * 4094 + [[1]]
    err = _hx().Hash10xError
    h = _load_image(tmp_path, blocks, 2, 5000)
    with pytest.raises(err, match=r"!! hashCopies needs every hash in range to have depth <= 4096 \(deepest 4097\)"):
        h.hash_copies(1)
    assert not _kept(h)
    h.read_hash(str(tmp_path / "state.hash"))                  # (ranges add up, hash10x.c:528-539: a narrower one needs the state anew)
    h.depth_range(2, 4097)
    t1 = h.hash_copies(1)
    assert _kept(h) and h.hash_copies_info["deepest"] == 4096 and h.hash_copies_info["inRange"] == 2
    assert not t1[1].any() and t1[2].tolist() == [4096, 1, 4096, 0] and t1[3].tolist() == [2, 1, 2, 0]
    t2 = h.hash_copies(2)                                       # only blocks 1 and 2 share two
    assert t2[2].tolist() == [4096, 4095, 2, 1] and t2[3].tolist() == [2, 1, 2, 0]
    assert h.hash_copies_info["rows"] == 2
    h.close()


def test_refusals(gen_recs):
    err = _hx().Hash10xError
    h = _hx().Hash10x(B=20)
    with pytest.raises(err, match="no hash state loaded"):
        h.hash_copies(5)
    with pytest.raises(err, match="no hash state loaded"):
        h.hash_copies_tally()
    h.close()
    recs = np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32)
    h = _hx().Hash10x(B=20)
    h.read_fqb(recs)
    with pytest.raises(err, match="!! you must set hashDepthRange before hashCopies"):
        h.hash_copies(5)
    assert not _kept(h)
    with pytest.raises(err, match="no result is kept"):
        h.hash_copies_tally()
    h.depth_range(3, 14)
    first = h.hash_copies(5)
    assert _kept(h)
    # the slabs of the C ABI: any piece of the kept table, and nothing beyond it
    n = h.hash_copies_info["hashNumber"]
    piece = np.zeros((7, 4), dtype=np.uint16)
    assert h._hip.h10x_hash_copies_get(h._ctx(), piece.ctypes.data, n - 7, 7) == 0 and np.array_equal(piece, first[n - 7:])
    assert h._hip.h10x_hash_copies_get(h._ctx(), piece.ctypes.data, n - 6, 7) != 0 and b"beyond" in h._hip.h10x_last_error(h._ctx())
    for bad in (0, -3):
        with pytest.raises(err, match="!! hashCopies minShare %d must be >= 1" % bad):
            h.hash_copies(bad)
        assert not _kept(h)                                    # a refused run keeps no result behind, nor an earlier one
        h.hash_copies(5)
        assert _kept(h)
    h.share_graph(5)                                           # a kept share graph is dropped by the run, as a components run drops it
    h.hash_copies(5)
    with pytest.raises(err, match="no graph is kept"):
        h._chk_ctx(h._hip.h10x_share_graph_get(h._ctx(), None, None, None, 0))
    h.depth_range(3, 14)                                       # a new range releases it
    assert not _kept(h)
    h.hash_copies(5)
    assert _kept(h)
    h.read_fqb(recs)                                           # a new state too
    assert not _kept(h)
    h.close()
    # after --clusterSplit the lists are of the old blocks until a new range is set
    h3 = _hx().Hash10x(B=21)
    h3.read_fqb(gen_recs[1])
    h3.depth_range(2, 40)
    h3.hash_copies(5)
    assert _kept(h3)
    h3.cluster(1, 0, 3)
    h3.cluster_split()
    assert not _kept(h3)
    with pytest.raises(err, match="!! you must set hashDepthRange before hashCopies"):
        h3.hash_copies(5)
    assert not _kept(h3)
    h3.depth_range(2, 40)
    h3.hash_copies(5)
    assert _kept(h3)
    h3.close()


# ------------------------------------------------------------------------------------ the file and the command line
SUMMARY = re.compile(r"^  hash copies at minShare (\d+): (\d+) hashes in range, (\d+) rows, (\d+) in one group, (\d+) split, deepest list (\d+)$", re.M)
CRIB = re.compile(r"^HASH_COPIES  (err|htA|htB|hom|mul) n (\d+) one (\d+) split (\d+)$", re.M)


def test_written_file(generated):
    h, cm, exp, d = generated
    p = os.path.join(d, "w.hc")
    h.write_hash_copies(100, p, out=os.path.join(d, "w.out"))
    info, table = _hx().read_hash_copies(p)
    assert info == {"version": 1, "hashNumber": cm.hash_number, "minShare": 100, "inRange": 3433, "rows": cm.rows(100)}
    _same(table, exp[100], "file")
    _same(h.hash_copies(100), table, "file against the call")
    text = open(os.path.join(d, "w.out")).read()
    m = SUMMARY.search(text)
    assert m and [int(v) for v in m.groups()] == [100, 3433, cm.rows(100), 1898, 0, 5] and "HASH_COPIES" not in text   # no crib: no lines by type


def test_cli(generated):
    h, cm, exp, d = generated
    base = [EXE, "-B", "21", "-ct", "3", "--readFQB", "x.fqb"]
    mol = ["--hashDepthRange", 2, 40, "--cluster", 1, 0, "--clusterSplit", "--hashDepthRange", 2, 40]

    def run(*args):
        p = subprocess.run(base + [str(a) for a in args], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        return p.returncode, p.stdout.decode(), p.stderr.decode()

    rc, out, err = run(*mol, "--hashCopies", 100, "x.hc")
    assert rc == 0, err
    info, table = _hx().read_hash_copies(os.path.join(d, "x.hc"))
    _same(table, exp[100], "cli")
    m = SUMMARY.search(out)
    assert m and [int(v) for v in m.groups()] == [100, 3433, cm.rows(100), 1898, 0, 5] and "HASH_COPIES" not in out
    assert (info["hashNumber"], info["minShare"], info["inRange"], info["rows"]) == (cm.hash_number, 100, 3433, cm.rows(100))
    assert out[m.end():].lstrip("\n").startswith("  user")      # the resource line follows
    # with -o the summary line goes to the file (behind the echo of the command's arguments, which ends without a newline: hash10x.c:1166-1171)
    rc, out, err = run("-o", "hc.out", *mol, "--hashCopies", 100, "y.hc")
    assert rc == 0 and "hash copies at minShare" not in out
    assert " 100 y.hc" + m.group(0) + "\n" in open(os.path.join(d, "hc.out")).read()
    assert open(os.path.join(d, "y.hc"), "rb").read() == open(os.path.join(d, "x.hc"), "rb").read()
    # soft errors: the message, nothing done, no file, exit status 0
    rc, out, err = run("--hashCopies", 50, "early.hc")
    assert rc == 0 and "!! you must set hashDepthRange before hashCopies\n" in out and not os.path.exists(os.path.join(d, "early.hc"))
    p = subprocess.run([EXE, "-B", "21", "--hashCopies", "50", "nostate.hc"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and b"!! you must set hashDepthRange before hashCopies\n" in p.stdout and not os.path.exists(os.path.join(d, "nostate.hc"))
    rc, out, err = run("-o", "soft.out", "--hashDepthRange", 2, 40, "--hashCopies", 0, "zero.hc", "--cluster", 1, 0, "--clusterSplit", "--hashCopies", 5, "late.hc")
    assert rc == 0, err
    for msg in ("!! hashCopies minShare 0 must be >= 1\n", "!! you must set hashDepthRange before hashCopies\n"):
        assert msg in err and msg in open(os.path.join(d, "soft.out")).read()
    assert not os.path.exists(os.path.join(d, "zero.hc")) and not os.path.exists(os.path.join(d, "late.hc"))
    # --interactive takes it too
    script = b"readFQB x.fqb\nhashDepthRange 2 40\ncluster 1 0\nclusterSplit\nhashDepthRange 2 40\nhashCopies 100 i.hc\nquit\n"
    p = subprocess.run(base[:5] + ["--interactive"], input=script, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and open(os.path.join(d, "i.hc"), "rb").read() == open(os.path.join(d, "x.hc"), "rb").read()
    p = subprocess.run([EXE, "--gpus", "2", "-B", "21", "--readFQB", "x.fqb", "--hashDepthRange", "2", "40", "--hashCopies", "50", "s.hc"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 255 and "FATAL ERROR: --hashCopies does not run on a sharded session (--gpus 2)" in p.stderr.decode()
    assert not os.path.exists(os.path.join(d, "s.hc"))


def test_cli_depth_cap(tmp_path):
    """the depth cap from the command line: the message on the output, no file, exit status 0; the state read anew (ranges add up) with the
    range cut below the deep hash runs"""
    blocks = [[1, 2], [1, 2]] + [[1]] * 4095
    (tmp_path / "deep.hash").write_bytes(orc.hash_image(blocks))
    p = subprocess.run([EXE, "-B", "20", "--readHash", "deep.hash", "--hashDepthRange", "2", "5000", "--hashCopies", "1", "deep.hc",
                        "--readHash", "deep.hash", "--hashDepthRange", "2", "4097", "--hashCopies", "1", "cut.hc"], cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    assert b"!! hashCopies needs every hash in range to have depth <= 4096 (deepest 4097)\n" in p.stdout and not (tmp_path / "deep.hc").exists()
    info, table = _hx().read_hash_copies(str(tmp_path / "cut.hc"))
    assert info["inRange"] == 1 and table[2].tolist() == [2, 1, 2, 0] and not table[1].any()


def test_cli_with_crib(gen_recs):
    """with --cribBuild the five HASH_COPIES lines: a numpy tally of the returned array over the crib's types"""
    d, recs = gen_recs
    h = _molecules(recs, crib=os.path.join(d, "x"))
    h.depth_range(2, 40)
    table = h.hash_copies(5)
    types, within = h.export_crib_type(), h.export_within().astype(bool)
    within[0] = False
    exp = [[int((within & (types == t)).sum()), int((within & (types == t) & (table[:, 1] == 1)).sum()), int((within & (types == t) & (table[:, 3] >= 2)).sum())]
           for t in range(5)]
    assert h.hash_copies_tally().tolist() == exp and sum(e[0] for e in exp) == h.hash_copies_info["inRange"] and sum(1 for e in exp if e[0]) >= 2
    h.close()
    p = subprocess.run([EXE, "-B", "21", "-ct", "3", "--readFQB", "x.fqb", "--cribBuild", "x.A.fa", "x.B.fa", "--hashDepthRange", "2", "40", "--cluster", "1", "0",
                        "--clusterSplit", "--hashDepthRange", "2", "40", "--hashCopies", "5", "crib.hc"], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    out = p.stdout.decode()
    lines = CRIB.findall(out)
    assert [l[0] for l in lines] == ["err", "htA", "htB", "hom", "mul"] and [[int(v) for v in l[1:]] for l in lines] == exp
    m = SUMMARY.search(out)
    assert m and int(m.group(2)) == sum(e[0] for e in exp) and int(m.group(4)) == sum(e[1] for e in exp) and int(m.group(5)) == sum(e[2] for e in exp)
    _same(_hx().read_hash_copies(os.path.join(d, "crib.hc"))[1], table, "the file with a crib")
