"""The hand-built states of tests/cluster_states.py on the GPU: Hash10x.read_hash, depth_range, cluster, write_hash, the file compared byte
for byte with the CPU oracle's. Every case runs under the forms of the list loop that write the result words differently, because the tail
(replay_kernel, point_sum_kernel, read_merge_kernel) reads those words. The cases with 16 k ranks and more and the block of more than
65535 records (`heavy` in the registry) take the default and two further forms only: the translated placement (cluster_first_global=4) and
the 24 KB budget, which sends their blocks to the HBM-scratch class of the list loop. Needs a real MI355X: `pytest -m gpu`."""
import os
import subprocess

import pytest

import cluster_states as cs
import orc

pytestmark = pytest.mark.gpu

# name -> (options, cluster_first_mode the run must report)
FORMS = {
    "default": ({}, 0),
    "narrow_first": ({"cluster_narrow_first": 1}, 0),
    "hbm_slot": ({"cluster_first_global": 1, "cluster_tr_packed": 1}, 2),
    "hbm_slot_unpacked": ({"cluster_first_global": 1, "cluster_tr_packed": 0}, 2),
    "ranked": ({"cluster_first_global": 2, "cluster_tr_packed": 1}, 1),
    "ranked_unpacked": ({"cluster_first_global": 2, "cluster_tr_packed": 0}, 1),
    "translated": ({"cluster_first_global": 4, "cluster_tr_packed": 1}, 4),
    "translated_unpacked": ({"cluster_first_global": 4, "cluster_tr_packed": 0}, 4),
    "lds_24k": ({"cluster_lds_budget": 24 * 1024}, 0),
    "lds_2k": ({"cluster_lds_budget": 2048}, 0),             # blocks with more than a few hundred ranks, or in files of many blocks: the HBM-scratch class
}
HEAVY_FORMS = ("default", "translated", "lds_24k")
RUNS = [(name, form) for name, c in cs.CASES.items() for form in (HEAVY_FORMS if c.heavy else FORMS)]


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """per case, made once: the directory with the case's file, the oracle's .hash bytes (after the case's own check of where it sits)"""
    root = str(tmp_path_factory.mktemp("cluster_states"))
    made = {}

    def get(name):
        if name not in made:
            exp, n_good = cs.run_oracle(name, root)
            cs.check(name, orc.HashFile(exp), n_good)
            made[name] = exp
        return root, made[name]
    return get


def _cluster(root, name, opts, mode, times=1):
    import hash10x_amd
    c = cs.find(name)
    h = hash10x_amd.Hash10x(B=20)
    for k, v in opts.items():
        h.set_option(k, v)
    h.read_hash(os.path.join(root, name + ".in.hash"))
    h.depth_range(c.lo, c.hi)
    outs = []
    for t in range(times):
        h.cluster(c.crange[0], c.crange[1], c.ct)
        assert h.counters()["cluster_first_mode"] == mode
        out = os.path.join(root, "%s.hip%d.hash" % (name, t))
        h.write_hash(out)
        with open(out, "rb") as f:
            outs.append(f.read())
        os.remove(out)
    classes = list(h.counters()["cluster_class_counts"])
    h.close()
    return outs, classes


@pytest.mark.parametrize("name,form", RUNS)
def test_state(oracle, name, form):
    root, exp = oracle(name)
    (got,), _ = _cluster(root, name, *FORMS[form])
    assert got == exp, orc.describe_diff(got, exp)


def test_small_budget_reaches_the_hbm_scratch_class(oracle):
    root, exp = oracle("pair255_pad1600")
    (got,), classes = _cluster(root, "pair255_pad1600", *FORMS["lds_2k"])
    assert classes[3] > 0 and got == exp


@pytest.mark.parametrize("name", ["pair254_pad1600", "pair255_pad16000"])
def test_cluster_twice_on_one_context(oracle, name):
    """the scratch of the replay and the clusterRaw slots are reused by the second command: same bytes (the states carry no stale labels, so the
    second clustering starts from what the first one started from)"""
    root, exp = oracle(name)
    outs, _ = _cluster(root, name, {}, 0, times=2)
    assert outs[0] == exp, orc.describe_diff(outs[0], exp)
    assert outs[1] == outs[0], orc.describe_diff(outs[1], outs[0])


def _lines(b):
    """the lines --verbose --cluster is about, as test_cli_verbose_cluster_lines_match_reference takes them: the per-barcode lines of codeClusterFind and
    codeClusterReadMerge and the command's closing line (the resource lines and the two programs' own wording of what --readHash read are left out)"""
    return [ln for ln in b.decode(errors="replace").splitlines() if ln.startswith(("  code ", " then ", "  clustered codes "))]


def _notes(b):
    return [ln for ln in b.decode(errors="replace").splitlines() if "too many clusters" in ln or ln.startswith("ignoring barcode")]


def test_cli_verbose_lines_of_built_blocks_match_reference(oracle):
    """bin/hash10x-amd --verbose and the reference binary on a file that holds a 255-cluster block, a block given up at the 256th cluster, a block
    without good hashes that carries unmerged labels and a block of one good hash: the lines of stdout that --verbose --cluster writes, one by one and in
    order, and the notes on stderr — the `raw`, `then N merged` and `too many clusters` lines among them."""
    if not orc.have_ref():
        pytest.fail("reference binary missing: build() makes oracle/_ref")
    root, exp = oracle("cli_mix")
    args = [str(a) for a in ["-B", 20, "-ct", 1, "--verbose", "--readHash", "cli_mix.in.hash", "--hashDepthRange", cs.LO, cs.HI, "--cluster", 1, 0, "--writeHash", "OUT"]]
    r = orc.run_ref([a if a != "OUT" else "cli.ref.hash" for a in args], root)
    assert r.returncode == 0, r.stderr.decode()
    g = subprocess.run([os.path.join(orc.REPO, "bin", "hash10x-amd")] + [a if a != "OUT" else "cli.hip.hash" for a in args], cwd=root, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert g.returncode == 0, g.stderr.decode()
    for got, ref in ((_lines(g.stdout), _lines(r.stdout)), (_notes(g.stderr), _notes(r.stderr))):
        assert got == ref, next(((a, b) for a, b in zip(got, ref) if a != b), (len(got), len(ref)))
    out = _lines(r.stdout)
    assert len(out) == 519 and out[-1] == "  clustered codes 1 to 519"
    assert out[0].endswith("510 cluster into 255 raw then 255 merged clusters") and out[1].endswith("513 good hashes, 0 clusters") and out[2] == " then 1 merged clusters"
    assert out[3] == "  code 4 with 1 reads 1 hashes, 1 good hashes, 0 clusters"
    assert _notes(r.stderr) == ["    code 2 with 513 good hashes has too many clusters"]
    got = open(os.path.join(root, "cli.hip.hash"), "rb").read()
    assert got == exp, orc.describe_diff(got, exp)
