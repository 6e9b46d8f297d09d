"""--shareGraph without a GPU: the NumPy model of its definition (tests/share_model.py) against the SHARE lines of the reference binary's
--codeExplore, the usage text, and the reader of the .sg file."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import orc
import share_model

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
T = 50
CT = 2


def test_model_against_reference(tmp_path):
    """Every block's SHARE lines with shared_hashes >= 50 are row c of the model at T = 50. The reference prints the lines by descending
    count down to and including the first one below -ct (hash10x.c:1454-1465), but only for a block whose good hashes form a cluster at
    that -ct (hash10x.c:1414) — at -ct 50 none of this input does, so the run is made at -ct 2, where every barcode clusters and every
    line down to count 2 is printed: the lines >= 50 are compared as asked, and all lines >= 2 with the model at T = 2 as well."""
    if not orc.have_ref():
        pytest.fail("reference binary missing: build() makes oracle/_ref")
    d = str(tmp_path)
    orc.gen_fqb(os.path.join(d, "x.fqb"), 5000, 24, 40000, 0.003, 11, 4.0, 150, 5000, fa=os.path.join(d, "x"))
    r = orc.run_ref(["-B", 20, "--readFQB", "x.fqb", "--writeHash", "x.hash"], d)
    assert r.returncode == 0, r.stderr[-400:]
    hf = orc.HashFile(open(os.path.join(d, "x.hash"), "rb").read())
    model = share_model.ShareModel.from_hash_file(hf, [(3, 30)])
    assert model.n_blocks == 25
    args = ["-B", 20, "-ct", CT, "--readFQB", "x.fqb", "--hashDepthRange", 3, 30, "--cribBuild", "x.A.fa", "x.B.fa"]
    for c in range(model.n_blocks):
        args += ["--codeExplore", c]
    r = orc.run_ref(args, d)
    assert r.returncode == 0, r.stderr[-400:]
    share, low = {}, {}
    code = None
    for ln in r.stdout.decode(errors="replace").splitlines():
        m = re.match(r"COMMAND --codeExplore (\d+)$", ln)
        if m:
            code = int(m.group(1))
            continue
        m = re.match(r"  SHARE code (\d+) shared_hashes (\d+) ", ln)
        if m:
            share.setdefault(code, set())
            low.setdefault(code, set())
            if int(m.group(2)) >= T:
                share[code].add((int(m.group(1)), int(m.group(2))))
            if int(m.group(2)) >= CT:                          # (the trailing line below -ct is left out)
                low[code].add((int(m.group(1)), int(m.group(2))))
    # every barcode with records clusters at -ct 2 (block 0 is unused, and the block still open at the end of the file is kept empty: hash10x.c:209)
    assert sorted(share) == [c for c in range(1, model.n_blocks) if hf.blocks["nHash"][c]] and len(share) == 23, sorted(share)
    rows = 0
    for c in range(model.n_blocks):
        blk, cnt = model.row(c, T)
        assert share.get(c, set()) == set(zip(blk.tolist(), cnt.tolist())), c
        blk, cnt = model.row(c, CT)
        assert low.get(c, set()) == set(zip(blk.tolist(), cnt.tolist())), c
        rows += len(share.get(c, ()))
    assert rows == 416
    off, blk, cnt = model.graph(T)
    assert (int(off[-1]), int(model.graph(1)[0][-1]), int(model.graph(200)[0][-1]), int(model.share.max())) == (416, 474, 212, 726)
    assert int(model.list_entries.sum()) == 100686


def test_usage_names_share_graph():
    p = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--shareGraph <minShare> <sg output>" in p.stderr


def _write(path, magic=b"10XG", version=1, n_blocks=4, min_share=3, offsets=(0, 0, 2, 2, 3), rows=((2, 7), (3, 9), (1, 4)), n_rows=None):
    with open(path, "wb") as f:
        f.write(magic + struct.pack("<IIIQ", version, n_blocks, min_share, len(rows) if n_rows is None else n_rows))
        f.write(np.asarray(offsets, dtype="<u8").tobytes())
        f.write(np.asarray(rows, dtype="<u4").tobytes())


def test_read_share_graph_round_trip(tmp_path):
    import hash10x_amd
    p = str(tmp_path / "g.sg")
    _write(p)
    info, off, blk, cnt = hash10x_amd.read_share_graph(p)
    assert info == {"version": 1, "nBlocks": 4, "minShare": 3, "rows": 3}
    assert off.dtype == np.uint64 and off.tolist() == [0, 0, 2, 2, 3]
    assert blk.dtype == np.uint32 and blk.tolist() == [2, 3, 1] and cnt.dtype == np.uint32 and cnt.tolist() == [7, 9, 4]
    _write(p, n_blocks=0, offsets=(0,), rows=())
    info, off, blk, cnt = hash10x_amd.read_share_graph(p)
    assert info["rows"] == 0 and off.tolist() == [0] and len(blk) == 0 and len(cnt) == 0


def test_read_share_graph_rejects(tmp_path):
    import hash10x_amd
    p = str(tmp_path / "g.sg")
    _write(p, magic=b"10XM")
    with pytest.raises(hash10x_amd.Hash10xError, match="not a share graph file"):
        hash10x_amd.read_share_graph(p)
    _write(p, version=2)
    with pytest.raises(hash10x_amd.Hash10xError, match="version 2"):
        hash10x_amd.read_share_graph(p)
    _write(p, offsets=(0, 2, 1, 2, 3))
    with pytest.raises(hash10x_amd.Hash10xError, match="offsets do not ascend"):
        hash10x_amd.read_share_graph(p)
    _write(p, offsets=(0, 0, 2, 2, 2))                          # the last offset is not the row count
    with pytest.raises(hash10x_amd.Hash10xError, match="offsets do not ascend"):
        hash10x_amd.read_share_graph(p)
    _write(p, n_rows=5)                                        # shorter than its header says
    with pytest.raises(hash10x_amd.Hash10xError, match="bytes"):
        hash10x_amd.read_share_graph(p)
