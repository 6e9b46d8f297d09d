"""--moleculeMap / --splitFQB without a device: the numpy model of tests/mol_model.py against the .hash files the reference wrote
(tests/golden), and the two small file formats: the C writers of libh10x_host.so against the model's bytes, the Python readers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import mol_model
import orc

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")

# golden -> (records, blocks incl. slot 0, molecules, clustered read pairs): measured with the model on the reference's files
PINNED = {
    "small.c_3_14_2": (4000, 41, 88, 1391),
    "small.recluster": (4000, 41, 31, 246),
    "small.c_3_12_3": (4000, 41, 31, 244),
    "small.c_2_14_5": (4000, 41, 1, 3),
    "small.accum": (4000, 41, 62, 734),
    "tiny.c": (16, 9, 2, 2),
    "abort255.out": (2100, 1502, 0, 0),
}


@pytest.fixture(scope="module")
def native():
    import hash10x_amd
    return hash10x_amd.load_native()


@pytest.fixture(scope="module")
def small():
    return mol_model.load("small.c_3_14_2.hash.gz")


@pytest.mark.parametrize("name", sorted(PINNED))
def test_model_on_goldens(name):
    m = mol_model.load(name + ".hash.gz")
    assert (m.R, m.n_codes, m.M, m.n_clustered) == PINNED[name]
    assert m.mol.size == m.slot.size == m.R
    inside = m.mol >= m.n_codes
    assert int(inside.sum()) == m.n_clustered and (m.mol[inside] < m.n_codes + m.M).all()
    # a molecule's slots are 0 .. count - 1, each once
    for mm in np.unique(m.mol[inside]).tolist():
        assert np.array_equal(np.sort(m.slot[m.mol == mm]), np.arange(m.count[mm]))
    if m.M == 0:                                             # identity map
        assert np.array_equal(m.dest, np.arange(m.R))


def test_no_read_of_a_golden_carries_two_labels():
    for name in PINNED:
        hf = orc.HashFile(orc.read_maybe_gz(os.path.join(orc.GOLDEN, name + ".hash.gz")))
        for c in range(1, hf.blocks_max):
            ns = int(hf.blocks["nSubCluster"][c])
            ch = hf.block_clushash(c)
            ok = (ch["subCluster"] >= 1) & (ch["subCluster"] <= ns)
            key = np.unique(ch["read"][ok].astype(np.int64) * 256 + ch["subCluster"][ok])
            assert np.unique(key // 256).size == key.size, (name, c)


def test_model_matches_the_reference_split(small):
    """the per-molecule counts are nRead of blocks 41 .. 128 of the reference's state after --clusterSplit, the parents match, and
    every ClusterHash record there points at a record of its parent's barcode in the split file"""
    sp = orc.HashFile(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.split.hash.gz")))
    assert sp.blocks_max == 129
    small.check_against_split(sp)
    recs = np.frombuffer(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.fqb.gz")), dtype=np.uint32).reshape(-1, 30)
    mol_model.split_refs(small, sp, small.split(recs), recs)


def _info(hip_info_cls, m):
    z = hip_info_cls()
    z.nRecords, z.nClustered, z.nBlocks, z.nMolecules = m.R, m.n_clustered, m.n_codes, m.M
    return z


@pytest.mark.parametrize("name", ["small.c_3_14_2", "tiny.c", "abort255.out"])
def test_c_writers_equal_the_model_and_readers_round_trip(native, tmp_path, name):
    import hash10x_amd
    _, host = native
    m = mol_model.load(name + ".hash.gz")
    err = ctypes.create_string_buffer(512)
    z = _info(hash10x_amd._MolInfo, m)
    p, q = str(tmp_path / "x.mol"), str(tmp_path / "x.fqb.idx")
    assert host.h10x_host_write_molmap(os.fsencode(p), m.mol.ctypes.data, m.slot.ctypes.data, ctypes.byref(z), err, 512) == 0, err.value
    assert open(p, "rb").read() == m.mol_bytes()
    assert host.h10x_host_write_split_index(os.fsencode(q), m.start.ctypes.data, m.n_codes, m.M, err, 512) == 0, err.value
    assert open(q, "rb").read() == m.idx_bytes()
    mol, slot, info = hash10x_amd.read_molecule_map(p)
    assert np.array_equal(mol, m.mol) and np.array_equal(slot, m.slot) and info == m.info
    start, nb, nm = hash10x_amd.read_split_index(q)
    assert np.array_equal(start, m.start) and (nb, nm) == (m.n_codes, m.M)
    assert host.h10x_host_write_molmap(os.fsencode(str(tmp_path / "no" / "x.mol")), m.mol.ctypes.data, m.slot.ctypes.data, ctypes.byref(z), err, 512) != 0
    assert b"failed to open output file" in err.value


def test_readers_refuse_bad_files(small, tmp_path):
    import hash10x_amd
    good_mol, good_idx = small.mol_bytes(), small.idx_bytes()
    cases = [(hash10x_amd.read_molecule_map, b"10XS" + good_mol[4:], "magic"), (hash10x_amd.read_molecule_map, good_mol[:4] + (2).to_bytes(4, "little") + good_mol[8:], "version"),
             (hash10x_amd.read_molecule_map, good_mol[:-4], "bytes"), (hash10x_amd.read_molecule_map, good_mol[:20], "magic"),
             (hash10x_amd.read_split_index, b"10XM" + good_idx[4:], "magic"), (hash10x_amd.read_split_index, good_idx[:4] + (0).to_bytes(4, "little") + good_idx[8:], "version"),
             (hash10x_amd.read_split_index, good_idx[:-8], "bytes"), (hash10x_amd.read_split_index, good_idx + bytes(8), "bytes")]
    for k, (reader, data, word) in enumerate(cases):
        p = tmp_path / ("bad%d" % k)
        p.write_bytes(data)
        with pytest.raises(hash10x_amd.Hash10xError, match=word):
            reader(str(p))


def test_usage_lists_the_commands(native):
    r = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0
    for line in (b"   --moleculeMap <mol output>", b"   --splitFQB <sorted fqb input> <split fqb output>"):
        assert line in r.stderr
