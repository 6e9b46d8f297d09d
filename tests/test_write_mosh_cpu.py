"""--writeMosh without a GPU: the plain-Python model of its definition (tests/statemosh_model.py) by hand, the model's probe table against
the table of a state the reference wrote, and the usage text."""
import os
import subprocess

import numpy as np
import pytest

import copies_model
import mosh_model
import orc
import statemosh_model as sm

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
K, W, SEED = 21, 31, 17


def _two_loci():
    """the state of test_hash_copies_cpu.test_model_by_hand: blocks 1-3 hold {1, 10, 11, 12}, blocks 4-6 hold {1, 20, 21, 22}; range 2 .. 99"""
    blocks = [[1, 10, 11, 12]] * 3 + [[1, 20, 21, 22]] * 3
    hashes = np.concatenate(blocks)
    depth = np.bincount(hashes, minlength=23)
    within = (depth >= 2) & (depth < 100)
    cm = copies_model.CopiesModel([0] + [len(b) for b in blocks], hashes, within)
    value = np.arange(23, dtype=np.uint64) * 31
    return value, depth, within, cm


def test_model_by_hand():
    value, depth, within, cm = _two_loci()
    xs = [1, 10, 11, 12, 20, 21, 22]
    assert depth[1] == 6 and all(depth[x] == 3 for x in xs[1:])
    thr = (2, 5, 100)

    def run(table=None, t=0):
        m, info = sm.state_mosh(value, depth, within, *thr, 20, K, W, SEED, table=table, min_share=t)
        assert m.max == 7 and m.value[1:] == [31 * x for x in xs]          # set indices 1 .. 7 in ascending hash index
        assert m.depth[1:] == [6, 3, 3, 3, 3, 3, 3] and m.value[0] == 0 and m.depth[0] == 0 and m.info[0] == 0
        assert info["kept"] == 7 and info["hashNumber"] == 23 and info["bits"] == 20 and info["saturated"] == 0
        assert info["copy"] == np.bincount(m.info[1:], minlength=4).tolist()
        return m, info

    m0, i0 = run()
    assert m0.info[1:] == [2, 1, 1, 1, 1, 1, 1] and (i0["toM"], i0["to0"], i0["minShare"]) == (0, 0, 0)
    t2 = cm.table(2)
    assert t2[1].tolist() == [6, 2, 3, 3]
    m2, i2 = run(t2, 2)
    assert m2.info[1:] == [3, 1, 1, 1, 1, 1, 1] and (i2["toM"], i2["to0"], i2["minShare"]) == (1, 0, 2)
    t5 = cm.table(5)
    assert all(t5[x].tolist() == [depth[x], depth[x], 1, 1] for x in xs)
    m5, i5 = run(t5, 5)
    assert m5.info[1:] == [0] * 7 and (i5["toM"], i5["to0"], i5["minShare"]) == (0, 7, 5)
    m1, i1 = run(cm.table(1), 1)
    assert m1.info == m0.info and (i1["toM"], i1["to0"], i1["minShare"]) == (0, 0, 1)
    assert m1.to_bytes() == m0.to_bytes() and m2.to_bytes() != m0.to_bytes()
    # the table is what sequential insertion in set-index order builds, and every kept hash is found through its own probe walk
    t = m0.table()
    mask = (1 << 20) - 1
    for i in range(1, 8):
        h = m0.value[i]
        slot, step = h & mask, ((h >> 20) & mask) | 1
        while t[slot] != i:
            assert t[slot] != 0
            slot = (slot + step) & mask
    assert int((t != 0).sum()) == 7
    # the file: header, table, then 11 bytes per index, index 0 included
    assert len(m0.to_bytes()) == 8 + 4 + 4 + 80 + 4 * (1 << 20) + 8 * 11


def test_model_saturation_and_capacity():
    value, depth, within, _ = _two_loci()
    depth = depth.copy()
    depth[1] = 70000
    within = (depth >= 2) & (depth < 100000)
    m, info = sm.state_mosh(value, depth, within, 2, 5, 65536, 20, K, W, SEED)
    assert m.depth[1] == 65535 and m.info[1] == 2 and info["saturated"] == 1            # classed by 65535, below copyMmin 65536
    m, info = sm.state_mosh(value, depth, within, 2, 5, 65535, 20, K, W, SEED)
    assert m.depth[1] == 65535 and m.info[1] == 3 and info["copy"] == [0, 6, 0, 1]
    # the capacity rule of moshsetCreate: kept + 1 >= 2^(bits - 2) is too big (bits below 20 only here, to keep the model small)
    n = (1 << 8) - 1
    v = np.arange(n + 1, dtype=np.uint64) * 31
    d = np.full(n + 1, 3)
    with pytest.raises(mosh_model.ModelDie, match="Moshset size %d is too big for 10 bits" % (n + 1)):
        sm.state_mosh(v, d, d > 0, 1, 2, 3, 10, K, W, SEED)
    m, info = sm.state_mosh(v[:-1], d[:-1], d[:-1] > 0, 1, 2, 3, 10, K, W, SEED)
    assert info["kept"] == n - 1 and m.max == n - 1


def test_model_table_is_the_reference_states_table():
    """hashIndex / hashValue / hashDepth of a state the reference wrote: with a range over everything and bits = the file's B the model's
    table is the file's hashIndex word for word, since both tables are built by the same insertion in the same order"""
    hf = orc.HashFile(orc.read_maybe_gz(os.path.join(orc.GOLDEN, "small.hash.gz")))
    n = hf.hash_number
    value, depth = hf.hash_value[:n], hf.hash_depth[:n]
    assert n == 5039 and hf.B == 20
    m, info = sm.state_mosh(value, depth, np.ones(n, dtype=bool), 2, 5, 100, hf.B, K, W, SEED)
    assert info["kept"] == n - 1 and m.max == n - 1
    assert np.array_equal(m.table(), hf.hash_index)
    assert m.value[1:] == [int(v) for v in value[1:]] and m.depth[1:] == [int(x) for x in depth[1:]]
    assert info["copy"] == np.bincount(np.where(depth[1:] < 2, 0, np.where(depth[1:] < 5, 1, 2)), minlength=4).tolist()


def test_usage_names_write_mosh():
    p = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--writeMosh <bits> <copy1min> <copy2min> <copyMmin> <mosh output>" in p.stderr
