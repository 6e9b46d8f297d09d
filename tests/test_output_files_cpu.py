"""The writers of files_host.c that had no driver of their own — .mm, .idx, .sg and the whitelist text — under AddressSanitizer + UBSan in a
stand-alone program (host/files_asan_driver.c, no device): the program itself checks the whitelist round trip and that a writer that fails — an
unopenable path, a failing callback, a disk full after 4096 bytes — leaves neither a file nor a .part and keeps an older file's bytes; here its
good files go through the package's readers."""
import os
import subprocess

import numpy as np
import pytest

import orc
from test_sanitizers import ENV

REPO = orc.REPO


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    drv = os.path.join(REPO, "build", "files-host-asan")
    if not os.path.exists(drv):
        subprocess.run(["make", "-C", os.path.join(REPO, "hash10x_amd", "host"), "../../build/files-host-asan"], check=True, stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("files")
    r = subprocess.run([drv, str(d)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode not in (66, 67) and b"ERROR: AddressSanitizer" not in r.stderr and b"runtime error:" not in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    assert r.returncode == 0 and r.stdout == b"4 writers, 3 failures each: nothing left behind\n", (r.returncode, r.stdout, r.stderr[-1000:])
    return d


def test_driver_leaves_only_whole_files(written):
    assert sorted(os.listdir(written)) == ["idx_0.idx", "idx_7.idx", "mm_0.mm", "mm_1.mm", "mm_65539.mm", "sg_1.sg", "sg_3.sg", "sg_8192.sg", "sg_none.sg"]


@pytest.mark.parametrize("n", [0, 1, (1 << 16) + 3])
def test_molecule_map_reads_back(written, n):
    import hash10x_amd
    mol, slot, info = hash10x_amd.read_molecule_map(str(written / ("mm_%d.mm" % n)))
    assert info == {"nRecords": n, "nClustered": n // 2, "nBlocks": 11, "nMolecules": 23}
    i = np.arange(n, dtype=np.uint64)
    assert mol.dtype == np.uint32 and np.array_equal(mol, 7 * i + 1) and np.array_equal(slot, i % 5)


@pytest.mark.parametrize("n_blocks, n_mol", [(0, 0), (3, 4)])
def test_split_index_reads_back(written, n_blocks, n_mol):
    import hash10x_amd
    start, b, m = hash10x_amd.read_split_index(str(written / ("idx_%d.idx" % (n_blocks + n_mol))))
    assert (b, m) == (n_blocks, n_mol) and np.array_equal(start, 10 * np.arange(n_blocks + n_mol + 1))


@pytest.mark.parametrize("step", [1, 3, 8192])
def test_share_graph_reads_back_whatever_the_ranges(written, step):
    """10 blocks, the row of block c holds c % 3 pairs {c + 1 + k, 2 c + k + 1}: the same bytes from ranges of 1, 3 and 8192 blocks"""
    import hash10x_amd
    info, off, blk, cnt = hash10x_amd.read_share_graph(str(written / ("sg_%d.sg" % step)))
    c = np.arange(10)
    assert info == {"version": 1, "nBlocks": 10, "minShare": 4, "rows": 9}
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(c % 3)]))
    exp = [(b + 1 + k, 2 * b + k + 1) for b in range(10) for k in range(b % 3)]
    assert list(zip(blk.tolist(), cnt.tolist())) == exp
    assert (written / ("sg_%d.sg" % step)).read_bytes() == (written / "sg_1.sg").read_bytes()
    info, off, blk, cnt = hash10x_amd.read_share_graph(str(written / "sg_none.sg"))
    assert info["nBlocks"] == 0 and info["rows"] == 0 and off.tolist() == [0] and blk.size == 0
