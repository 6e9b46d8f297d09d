"""--hashCopies without a GPU: the plain-Python model of its definition (tests/copies_model.py) by hand and on a generated set that went
through the reference binary, the usage text, the reader of the .hc file, and the .hc writer under AddressSanitizer + UBSan behind a
main of its own."""
import os
import struct
import subprocess

import numpy as np
import pytest

import copies_model
import orc

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
TOP = 2 ** 31 - 1
GEN = orc.GEN_MOLECULES                                         # the generated set of test_share_components_cpu.py


def test_model_by_hand():
    """Two loci. Blocks 1-3 hold hashes 10, 11, 12, blocks 4-6 hold 20, 21, 22, all six hold hash 1; range 2 .. 99. Inside a locus two blocks
    share 4 hashes (hash 1 included), across the loci only hash 1."""
    blocks = [[1, 10, 11, 12]] * 3 + [[1, 20, 21, 22]] * 3
    n_hash = [0] + [len(b) for b in blocks]
    hashes = np.concatenate(blocks)
    depth = np.bincount(hashes, minlength=23)
    cm = copies_model.CopiesModel(n_hash, hashes, (depth >= 2) & (depth < 100))
    assert cm.xs.tolist() == [1, 10, 11, 12, 20, 21, 22] and cm.deepest == 6
    t1, t2, t5 = cm.table(1), cm.table(2), cm.table(5)
    assert t1.dtype == np.uint16 and t1.shape == (23, 4)
    assert t1[1].tolist() == [6, 1, 6, 0] and t2[1].tolist() == [6, 2, 3, 3] and t5[1].tolist() == [6, 6, 1, 1]
    assert t2[10].tolist() == [3, 1, 3, 0] and t5[10].tolist() == [3, 3, 1, 1]
    assert not t1[0].any() and not t1[2:10].any() and not t1[13:20].any()
    assert cm.tallies(t1) == (7, 7, 0, 6) and cm.tallies(t2) == (7, 6, 1, 6) and cm.tallies(t5) == (7, 0, 0, 6)
    assert copies_model.groups_of(np.zeros((4, 4), dtype=bool), [1, 2, 3]) == (3, 1, 1)
    assert copies_model.groups_of(np.ones((4, 4), dtype=bool), [2]) == (1, 1, 0)


def test_model_on_generated_set_through_reference(tmp_path):
    """The molecules of the generated set as the reference binary cuts them (-B 21 -ct 3, range 2 40, --cluster 1 0 --clusterSplit
    --writeHash), the model on the written state in the range 2 .. 40: the tallies (inRange, oneGroup, split, deepest) are pinned, and the
    consequences of the definition hold."""
    if not orc.have_ref():
        pytest.fail("reference binary missing: build() makes oracle/_ref")
    d = str(tmp_path)
    orc.gen_fqb(os.path.join(d, "x.fqb"), *GEN)
    r = orc.run_ref(["-B", 21, "-ct", 3, "--readFQB", "x.fqb", "--hashDepthRange", 2, 40, "--cluster", 1, 0, "--clusterSplit", "--writeHash", "x.hash"], d)
    assert r.returncode == 0, r.stderr[-400:]
    hf = orc.HashFile(open(os.path.join(d, "x.hash"), "rb").read())
    cm = copies_model.CopiesModel.from_hash_file(hf, [(2, 40)])
    assert cm.model.n_blocks == 31 and cm.hash_number == 17181
    pinned = {1: (3433, 3433, 0, 5), 50: (3433, 2675, 0, 5), 100: (3433, 1898, 0, 5), TOP: (3433, 0, 0, 5)}
    tables = {t: cm.table(t) for t in pinned}
    for t, exp in pinned.items():
        assert cm.tallies(tables[t]) == exp, t
    xs = cm.xs
    outside = np.ones(cm.hash_number, dtype=bool)
    outside[xs] = False
    for t, tab in tables.items():
        assert not tab[outside].any(), t                         # zeros outside the range and at index 0
        m = tab[xs, 0].astype(int)
        assert np.array_equal(m, [len(np.unique(l)) for l in cm.lists])
        assert np.all(tab[xs, 1] >= 1) and np.all(tab[xs, 1] <= m) and np.all(tab[xs, 2].astype(int) + tab[xs, 3] <= m) and np.all(tab[xs, 3] <= tab[xs, 2])
    # T = 1: no block of this state is above 65535 records, so every in-range hash is one group of all its blocks
    assert int(cm.model.share.max()) == 259
    assert np.all(tables[1][xs, 1] == 1) and np.array_equal(tables[1][xs, 2], tables[1][xs, 0]) and not tables[1][xs, 3].any()
    # T = 2^31 - 1: every block alone
    top = tables[TOP][xs]
    assert np.array_equal(top[:, 1], top[:, 0]) and np.all(top[:, 2] == 1) and np.array_equal(top[:, 3], (top[:, 0] > 1).astype(np.uint16))
    # groups does not fall as T rises
    order = sorted(tables)
    for lo, hi in zip(order, order[1:]):
        assert np.all(tables[lo][:, 1] <= tables[hi][:, 1]), (lo, hi)
    # an intermediate T tells hashes apart: at 50 and at 100 some sit in one group and some in several
    for t in (50, 100):
        g = tables[t][xs, 1]
        assert (g == 1).any() and (g > 1).any(), t


def test_usage_names_hash_copies():
    p = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--hashCopies <minShare> <hc output>" in p.stderr


def _write(path, magic=b"10XK", version=1, n_hash=4, min_share=3, in_range=2, rows=9, table=((0, 0, 0, 0), (6, 2, 3, 3), (0, 0, 0, 0), (3, 1, 3, 0)), tail=b""):
    with open(path, "wb") as f:
        f.write(magic + struct.pack("<IIIQQ", version, n_hash, min_share, in_range, rows))
        f.write(np.asarray(table, dtype="<u2").tobytes())
        f.write(tail)


def test_read_hash_copies(tmp_path):
    import hash10x_amd
    err = hash10x_amd.Hash10xError
    p = str(tmp_path / "t.hc")
    _write(p)
    info, table = hash10x_amd.read_hash_copies(p)
    assert info == {"version": 1, "hashNumber": 4, "minShare": 3, "inRange": 2, "rows": 9}
    assert table.dtype == np.uint16 and table.tolist() == [[0, 0, 0, 0], [6, 2, 3, 3], [0, 0, 0, 0], [3, 1, 3, 0]]
    _write(p, n_hash=0, in_range=0, rows=0, table=())
    info, table = hash10x_amd.read_hash_copies(p)
    assert info["hashNumber"] == 0 and table.shape == (0, 4)
    _write(p, magic=b"10XC")
    with pytest.raises(err, match="not a hash copies file"):
        hash10x_amd.read_hash_copies(p)
    _write(p, version=2)
    with pytest.raises(err, match="version 2"):
        hash10x_amd.read_hash_copies(p)
    _write(p, n_hash=5)                                        # truncated: shorter than its header says
    with pytest.raises(err, match="bytes"):
        hash10x_amd.read_hash_copies(p)
    _write(p, tail=b"\0\0")                                    # longer than its header says
    with pytest.raises(err, match="bytes"):
        hash10x_amd.read_hash_copies(p)
    with open(p, "wb") as f:
        f.write(b"10XK" + bytes(20))                           # cut inside the header
    with pytest.raises(err, match="not a hash copies file"):
        hash10x_amd.read_hash_copies(p)


# ------------------------------------------------------------------------------------ the .hc writer under ASan + UBSan (a program of its own, on the CPU)
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="halt_on_error=1:exitcode=67")   # (the HIP runtime, linked in, keeps its own allocations)


@pytest.mark.parametrize("n_hash, slab, slabs", [(0, 0, 0), (1, 0, 1), (1000, 64, 16), (1024, 64, 16), (5, 1, 5), (300, 0, 1)])
def test_hc_writer_under_sanitizers(tmp_path, n_hash, slab, slabs):
    import hash10x_amd
    drv = os.path.join(orc.REPO, "build", "hc-host-asan")
    if not os.path.exists(drv):
        subprocess.run(["make", "-C", os.path.join(orc.REPO, "hash10x_amd", "host"), "asan"], check=True, stdout=subprocess.DEVNULL)
    p = str(tmp_path / "w.hc")
    r = subprocess.run([drv, p, str(n_hash), str(slab)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode not in (66, 67) and b"ERROR: AddressSanitizer" not in r.stderr and b"runtime error:" not in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    assert r.returncode == 0 and b"failed to open output file" in r.stdout and r.stdout.startswith(b"%d slabs\n" % slabs), (r.stdout, r.stderr)
    assert not os.path.exists(p + ".part")
    info, table = hash10x_amd.read_hash_copies(p)
    assert info == {"version": 1, "hashNumber": n_hash, "minShare": 5, "inRange": max(n_hash - 1, 0), "rows": 3 * n_hash}
    x = np.arange(n_hash)
    assert np.array_equal(table, np.stack([x % 7, x % 3, x % 5, x % 2], axis=1).astype(np.uint16).reshape(-1, 4))
