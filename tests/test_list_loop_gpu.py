"""The hand-built list-loop states of tests/list_cases.py on the GPU: Hash10x.read_hash, depth_range, cluster, write_hash, the whole file compared byte for byte
with the CPU oracle's. A wrong msBest, msTot or minShareCount[clusterMin] of one rank shows as a wrong label or as a pointToMin that differs in its last bit. Every
case runs under the ten forms of test_cluster_states_gpu.py and at 512 lanes (another round size); the class census and the table edges of the translated
placement also under the options that choose its units and the size of its tables. Two files go through bin/hash10x-amd --gpus 2 and 3: a sharded list holds
global barcode numbers. Needs a real MI355X: `pytest -m gpu`."""
import os
import subprocess

import pytest

import cluster_states as cs
import list_cases as lc
import orc
from test_cluster_states_gpu import FORMS

pytestmark = pytest.mark.gpu

LOOP_FORMS = dict(FORMS, threads0_512=({"cluster_threads0": 512}, 0))
# the packed translated placement's units (class T on and off) and the unpacked one, whose handle stride is the power of two that holds the longest list
CENSUS_FORMS = {"tr_packed%d_class_t%d" % (p, t): ({"cluster_first_global": 4, "cluster_tr_packed": p, "cluster_tr_class_t": t}, 4) for p in (1, 0) for t in (1, 0)}
# cluster_first_cap = c: the translated placement's tables have S = S2 = c slots, the ranked first[] c entries
TABLE_FORMS = {
    "tr_packed_cap": ({"cluster_first_global": 4, "cluster_tr_packed": 1, "cluster_first_cap": lc.TABLE_CAP}, 4),
    "tr_unpacked_cap": ({"cluster_first_global": 4, "cluster_tr_packed": 0, "cluster_first_cap": lc.TABLE_CAP}, 4),
    "ranked_cap": ({"cluster_first_global": 2, "cluster_tr_packed": 1, "cluster_first_cap": lc.TABLE_CAP}, 1),
}
RUNS = [(name, form) for name in lc.LIST_CASES for form in LOOP_FORMS]
OWN_RUNS = [(name, form) for name in lc.LIST_CASES if lc.FAMILY[name] == "f" for form in CENSUS_FORMS] + \
           [(name, form) for name in lc.LIST_CASES if lc.FAMILY[name] == "g" for form in TABLE_FORMS]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """per case, made once: the directory with the case's file, the oracle's .hash bytes (after the case's own check of where it sits)"""
    root = str(tmp_path_factory.mktemp("list_loop"))
    made = {}

    def get(name):
        if name not in made:
            exp, n_good = cs.run_oracle(name, root)
            cs.check(name, orc.HashFile(exp), n_good)
            made[name] = exp
        return root, made[name]
    return get


def _cluster(root, name, opts, mode):
    """(the .hash the GPU writes, its counters)"""
    import hash10x_amd
    c = cs.find(name)
    h = hash10x_amd.Hash10x(B=20)
    for k, v in opts.items():
        h.set_option(k, v)
    h.read_hash(os.path.join(root, name + ".in.hash"))
    h.depth_range(c.lo, c.hi)
    h.cluster(c.crange[0], c.crange[1], c.ct)
    ctr = dict(h.counters())
    assert ctr["cluster_first_mode"] == mode
    out = os.path.join(root, name + ".hip.hash")
    h.write_hash(out)
    with open(out, "rb") as f:
        got = f.read()
    os.remove(out)
    h.close()
    return got, ctr


@pytest.mark.parametrize("name,form", RUNS)
def test_state(oracle, name, form):
    root, exp = oracle(name)
    got, _ = _cluster(root, name, *LOOP_FORMS[form])
    assert got == exp, orc.describe_diff(got, exp)


@pytest.mark.parametrize("name,form", OWN_RUNS)
def test_state_under_its_own_options(oracle, name, form):
    root, exp = oracle(name)
    got, ctr = _cluster(root, name, *dict(CENSUS_FORMS, **TABLE_FORMS)[form])
    assert got == exp, orc.describe_diff(got, exp)
    if name == "g_table_%d" % lc.TABLE_M[-1]:
        # more distinct companions than two tables of 1024 slots (or a ranked first[] of 1024 entries) hold: the block is handed on, and finished all the same
        assert ctr["cluster_overflow_blocks"] >= 1


@pytest.mark.parametrize("gpus", [2, 3])
@pytest.mark.parametrize("name", ["f_mix", "e_own_entry"])
def test_cli_sharded(oracle, name, gpus):
    """bin/hash10x-amd --gpus N --readHash: every rank clusters its own blocks, whose lists hold the barcode numbers of the whole file"""
    root, exp = oracle(name)
    out = "%s.gpus%d.hash" % (name, gpus)
    args = [str(a) for a in ["--gpus", gpus] + cs.args(name, name + ".in.hash", out)]
    g = subprocess.run([os.path.join(orc.REPO, "bin", "hash10x-amd")] + args, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert g.returncode == 0, g.stderr.decode()[-2000:]
    with open(os.path.join(root, out), "rb") as f:
        got = f.read()
    os.remove(os.path.join(root, out))
    assert got == exp, orc.describe_diff(got, exp)
