"""--shareComponents without a GPU: the plain-Python model of its definition (tests/comp_model.py) on hand-made share matrices and on a
generated set that went through the reference binary, the usage text, and the reader of the .sc file."""
import os
import struct
import subprocess

import numpy as np
import pytest

import comp_model
import orc
import share_model

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")


def _lists(result):
    return [a.tolist() for a in result]


def test_model_by_hand():
    """Blocks 0 .. 5. 1 and 3 share 2 either way; 4 holds 5 entries of 2 in its lists while 2's own row is empty (a directed entry joins all
    the same); 5 shares nothing. Records 10, 20, 30, 0, 7: block 4 is an empty block, and still a member."""
    share = np.zeros((6, 6), dtype=np.int64)
    share[1, 3] = share[3, 1] = 2
    share[4, 2] = 5
    n_hash = [0, 10, 20, 30, 0, 7]
    # T = 1: {1, 3}, {2, 4}, {5}
    assert _lists(comp_model.components(share, n_hash, 1)) == [[0, 1, 2, 1, 2, 3], [0, 1, 2, 1, 2, 5], [0, 1, 2, 5], [0, 2, 2, 1], [0, 40, 20, 7]]
    # T = 3: the edge 1 - 3 is gone
    assert _lists(comp_model.components(share, n_hash, 3)) == [[0, 1, 2, 3, 2, 4], [0, 1, 2, 3, 2, 5], [0, 1, 2, 3, 5], [0, 1, 2, 1, 1], [0, 10, 20, 30, 7]]
    # T = 6: every block alone
    got = comp_model.components(share, n_hash, 6)
    assert _lists(got) == [[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0, 1, 1, 1, 1, 1], [0, 10, 20, 30, 0, 7]]
    assert got[0].dtype == got[1].dtype == got[2].dtype == got[3].dtype == np.uint32 and got[4].dtype == np.uint64
    assert comp_model.figures(got) == (5, 1, 5, 0)


def test_model_by_hand_far_root():
    """A chain 5 - 4 - 3 - 1 given from its far end, and 2 alone between them: the smallest number becomes the root of all four, whatever
    the order of the edges, and the numbering goes by root: {1, 3, 4, 5} is 1, {2} is 2."""
    share = np.zeros((6, 6), dtype=np.int64)
    share[5, 4] = 1
    share[4, 3] = 7
    share[3, 1] = 1
    n_hash = [0, 1, 2, 3, 4, 5]
    assert _lists(comp_model.components(share, n_hash, 1)) == [[0, 1, 2, 1, 1, 1], [0, 1, 2, 1, 1, 1], [0, 1, 2], [0, 4, 1], [0, 13, 2]]
    # T = 2: only 4 - 3
    assert _lists(comp_model.components(share, n_hash, 2)) == [[0, 1, 2, 3, 3, 4], [0, 1, 2, 3, 3, 5], [0, 1, 2, 3, 5], [0, 1, 1, 2, 1], [0, 1, 2, 7, 5]]
    # nothing but block 0
    assert _lists(comp_model.components(np.zeros((1, 1), dtype=np.int64), [0], 1)) == [[0], [0], [0], [0], [0]]


def test_model_on_generated_set_through_reference(tmp_path):
    """The molecules of a generated set as the reference binary cuts them (--cluster 1 0 at -ct 3, --clusterSplit, --writeHash), the share
    matrix of the written state in the range 2 .. 40, and its components at three thresholds: the figures are pinned."""
    if not orc.have_ref():
        pytest.fail("reference binary missing: build() makes oracle/_ref")
    d = str(tmp_path)
    orc.gen_fqb(os.path.join(d, "x.fqb"), *orc.GEN_MOLECULES)
    r = orc.run_ref(["-B", 21, "-ct", 3, "--readFQB", "x.fqb", "--hashDepthRange", 2, 40, "--cluster", 1, 0, "--clusterSplit", "--writeHash", "x.hash"], d)
    assert r.returncode == 0, r.stderr[-400:]
    hf = orc.HashFile(open(os.path.join(d, "x.hash"), "rb").read())
    model = share_model.ShareModel.from_hash_file(hf, [(2, 40)])
    n_hash = np.asarray(hf.blocks["nHash"][:hf.blocks_max], dtype=np.int64).copy()
    n_hash[0] = 0
    cm = comp_model.CompModel(model, n_hash)
    assert model.n_blocks == 31 and int(model.share.max()) == 259
    table = {1: (158, 3, 28, 2, 1), 50: (66, 6, 25, 5, 1), 100: (38, 15, 9, 11, 4)}
    for t, exp in table.items():
        res = cm.components(t)
        comp, root, root_of, blocks, records = res
        assert (cm.rows(t),) + comp_model.figures(res) == exp, t
        assert int(blocks.sum()) == model.n_blocks - 1 and int(records.sum()) == int(n_hash.sum())
        assert np.array_equal(root_of[comp], root) and np.all(root <= np.arange(model.n_blocks))
        assert np.all(np.diff(root_of.astype(np.int64)) > 0)
    # every block alone above the largest count
    assert comp_model.figures(cm.components(260)) == (30, 1, 30, 0)


def test_usage_names_share_components():
    p = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--shareComponents <minShare> <sc output>" in p.stderr


def _write(path, magic=b"10XC", version=1, n_blocks=6, min_share=3, n_comp=3, largest=2, rows=3, comp=(0, 1, 2, 1, 2, 3),
           entries=((0, 0, 0), (1, 2, 40), (2, 2, 20), (5, 1, 7)), tail=b""):
    with open(path, "wb") as f:
        f.write(magic + struct.pack("<IIIIIQ", version, n_blocks, min_share, n_comp, largest, rows))
        f.write(np.asarray(comp, dtype="<u4").tobytes())
        for e in entries:
            f.write(struct.pack("<IIQ", *e))
        f.write(tail)


def test_read_share_components_round_trip(tmp_path):
    import hash10x_amd
    p = str(tmp_path / "g.sc")
    _write(p)
    info, comp, root_of, blocks, records = hash10x_amd.read_share_components(p)
    assert info == {"version": 1, "nBlocks": 6, "minShare": 3, "nComponents": 3, "largest": 2, "rows": 3}
    assert comp.dtype == np.uint32 and comp.tolist() == [0, 1, 2, 1, 2, 3]
    assert root_of.dtype == np.uint32 and root_of.tolist() == [0, 1, 2, 5]
    assert blocks.dtype == np.uint32 and blocks.tolist() == [0, 2, 2, 1]
    assert records.dtype == np.uint64 and records.tolist() == [0, 40, 20, 7]
    _write(p, n_blocks=1, n_comp=0, largest=0, rows=0, comp=(0,), entries=((0, 0, 0),))
    info, comp, root_of, blocks, records = hash10x_amd.read_share_components(p)
    assert info["nComponents"] == 0 and comp.tolist() == [0] and root_of.tolist() == [0] and blocks.tolist() == [0] and records.tolist() == [0]


def test_read_share_components_rejects(tmp_path):
    import hash10x_amd
    err = hash10x_amd.Hash10xError
    p = str(tmp_path / "g.sc")
    _write(p, magic=b"10XG")
    with pytest.raises(err, match="not a share components file"):
        hash10x_amd.read_share_components(p)
    _write(p, version=2)
    with pytest.raises(err, match="version 2"):
        hash10x_amd.read_share_components(p)
    _write(p, tail=b"\0\0\0\0")                                  # longer than its header says
    with pytest.raises(err, match="bytes"):
        hash10x_amd.read_share_components(p)
    _write(p, n_comp=4)                                        # shorter than its header says
    with pytest.raises(err, match="bytes"):
        hash10x_amd.read_share_components(p)
    _write(p, comp=(0, 1, 2, 1, 2, 4))                          # comp < nComponents + 1
    with pytest.raises(err, match="beyond the 3 components"):
        hash10x_amd.read_share_components(p)
    _write(p, entries=((0, 0, 0), (1, 2, 40), (2, 2, 20), (5, 2, 7)))   # the member counts sum to nBlocks - 1
    with pytest.raises(err, match="do not sum to the 5 blocks"):
        hash10x_amd.read_share_components(p)
    _write(p, entries=((0, 0, 0), (2, 2, 40), (1, 2, 20), (5, 1, 7)))   # rootOf ascends
    with pytest.raises(err, match="roots do not ascend"):
        hash10x_amd.read_share_components(p)
    _write(p, entries=((0, 0, 0), (1, 2, 40), (2, 2, 20), (2, 1, 7)))   # (strictly)
    with pytest.raises(err, match="roots do not ascend"):
        hash10x_amd.read_share_components(p)
