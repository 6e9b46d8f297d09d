"""rm_block_kernel (csrc/stage_i.hip) on the scripted seed streams of tests/map_cases.py: per case through hash10x_amd.RefMap, all cases as the
queries of one call at three slab sizes, and bin/moshmap-amd against the lines the reference's moshmap printed (tests/golden/map_blocks.json).
Expected values come from the script itself and from map_cases.blocks(), which tests/test_moshmap_blocks_cpu.py holds to the reference and to
map_model.RefModel.query. Every comparison is exact equality."""
import json
import os
import subprocess

import numpy as np
import pytest

import map_cases as mc
import mosh_model as mm
import orc

pytestmark = pytest.mark.gpu
EXE = os.path.join(orc.REPO, "bin", "moshmap-amd")
with open(os.path.join(orc.GOLDEN, "map_blocks.json")) as f:
    GOLD = json.load(f)
CLASS_SHIFT = 30
REC_FIELDS = ("pos0", "posN", "loc0", "locN", "n1", "n2")


class Loaded:
    """a group's set and reference on the device, through the same doors as -r"""

    def __init__(self, group):
        import hash10x_amd
        self.b = b = mc.built(group)
        ms, ref = b["ms"], b["ref"]
        self.ms = hash10x_amd.MoshSet.from_arrays(mc.B, mc.K, mc.W, ms.factor1, ms.factor2, ms.table(), np.array(ms.value, np.uint64),
                                                  np.array(ms.depth, np.uint16), np.array(ms.info, np.uint8))
        self.rm = hash10x_amd.RefMap.from_arrays(self.ms, ref.index, ref.offset, ref.id, ref.depth_arr, ref.rev, ref.loc, n_ids=len(ref.len))
        self._single = {}

    def expected(self, n):
        """(seeds n x 5, positions, counts, records n x 6) of case n from its script and blocks()"""
        s, script = self.b["queries"][n], self.b["scripts"][n]
        seeds = mc.expected_seeds(script)
        _, ps = self.b["ms"].moshes(s)
        recs = [(int(ps[i0]), int(ps[iN]), l0, lN, n1, n2) for i0, iN, l0, lN, n1, n2 in mc.blocks(seeds)]
        return seeds, [int(p) for p in ps], [sum(x[0] == k for x in seeds) for k in range(4)], recs

    def single(self, n):
        """case n as the only query of a call, at the default slab: run once"""
        if n not in self._single:
            res = self.rm.query(*mm.flatten([self.b["queries"][n]]), seeds=True)
            self._single[n] = {k: np.array(v) for k, v in res.items()}
        return self._single[n]

    def close(self):
        self.rm.close(); self.ms.close()


@pytest.fixture(scope="module")
def loaded():
    groups = {}

    def get(g):
        if g not in groups:
            groups[g] = Loaded(g)
        return groups[g]
    yield get
    for x in groups.values():
        x.close()


def rec_rows(recs):
    return [tuple(int(r[k]) for k in REC_FIELDS) for r in recs]


def seed_rows(seeds):
    """(class, loc, loc2, id, id2) per device seed record: a miss is all 0, copy M only its class"""
    return [(int(s["idClass"]) >> CLASS_SHIFT, int(s["loc"]), int(s["loc2"]), int(s["idClass"]) & ((1 << CLASS_SHIFT) - 1), int(s["id2"])) for s in seeds]


# ---- per case ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", mc.CASES, ids=[c.name for c in mc.CASES])
def test_case_through_refmap(c, loaded):
    L = loaded(c.group)
    n = L.b["cases"].index(c)
    seeds, pos, counts, recs = L.expected(n)
    assert [(r[4], r[5]) for r in recs] == c.expect                                    # (the case still is what it is named for)
    res = L.single(n)
    assert [int(x) for x in res["seed_start"]] == [0, len(seeds)]
    assert seed_rows(res["seeds"]) == seeds
    assert [int(p) for p in res["seed_pos"]] == pos
    assert [int(x) for x in res["counts"].reshape(-1)] == counts
    assert [int(x) for x in res["rec_start"]] == [0, len(recs)]
    assert rec_rows(res["recs"]) == recs
    assert (res["recs"]["query"] == 0).all()


# ---- all cases as the queries of one call -------------------------------------------------------------------------------------------------------
def call_order(cases):
    """the cases with the empty and the seedless queries spread between the others"""
    bare = [c for c in cases if c.family == "nothing"]
    rest = [c for c in cases if c.family != "nothing"]
    step = len(rest) // (len(bare) + 1) + 1
    out = []
    for i, c in enumerate(rest):
        out.append(c)
        if bare and i % step == step - 1:
            out.append(bare.pop(0))
    return out + bare


@pytest.mark.parametrize("slab", [0, 40000, 3000], ids=["default_slab", "a_few_queries_a_batch", "every_query_alone"])
@pytest.mark.parametrize("group", list(mc.GROUPS))
def test_all_cases_in_one_call(group, slab, loaded):
    L = loaded(group)
    order = call_order(L.b["cases"])
    assert sorted(c.name for c in order) == sorted(c.name for c in L.b["cases"])
    if group == "x":
        at = [order.index(c) for c in order if c.family == "nothing"]
        assert 0 < at[0] and at[-1] < len(order) - 1 and all(b - a > 1 for a, b in zip(at, at[1:])), "the seedless queries lie between the others"
    idx = [L.b["cases"].index(c) for c in order]
    L.ms.set_option("mosh_slab", slab)                           # 0: the default
    try:
        res = L.rm.query(*mm.flatten([L.b["queries"][n] for n in idx]), seeds=True)
    finally:
        L.ms.set_option("mosh_slab", 0)
    assert len(res["counts"]) == len(order) and len(res["rec_start"]) == len(order) + 1
    for q, (c, n) in enumerate(zip(order, idx)):
        seeds, pos, counts, recs = L.expected(n)
        assert [int(x) for x in res["counts"][q]] == counts, c.name
        got = res["recs"][int(res["rec_start"][q]):int(res["rec_start"][q + 1])]
        assert rec_rows(got) == recs, c.name
        one = L.single(n)                                        # its single run
        assert np.array_equal(res["counts"][q], one["counts"][0]) and rec_rows(got) == rec_rows(one["recs"]), c.name
        assert (got["query"] == q).all(), c.name
        a, e = int(res["seed_start"][q]), int(res["seed_start"][q + 1])
        assert seed_rows(res["seeds"][a:e]) == seeds and [int(p) for p in res["seed_pos"][a:e]] == pos, c.name
    assert int(res["rec_start"][-1]) == len(res["recs"]) and int(res["seed_start"][-1]) == len(res["seeds"])


# ---- the program ----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """x.mosh, x.ref and all.fa of every group, written once"""
    dirs = {}
    for g in mc.GROUPS:
        d = str(tmp_path_factory.mktemp("blocks_" + g))
        for n in ("x.mosh", "x.ref", "all.fa"):
            with open(os.path.join(d, n), "wb") as f:
                f.write(mc.built(g)["files"][n])
        dirs[g] = d
    return dirs


RUNS = [(g, v, 0) for g in mc.GROUPS for v in (False, True)] + [("x", v, 3000) for v in (False, True)]      # --slab 3000: every query of all.fa goes alone


@pytest.mark.parametrize("group,verbose,slab", RUNS, ids=["%s_%s_slab%d" % (g, "verbose" if v else "plain", s) for g, v, s in RUNS])
def test_program_matches_the_reference(group, verbose, slab, staged):
    if not os.path.exists(EXE):
        pytest.fail("bin/moshmap-amd is missing: run build()")
    args = (["--slab", str(slab)] if slab else []) + ["-r", "x"] + (["-v"] if verbose else []) + ["-q", "all.fa"]
    r = subprocess.run([EXE] + args, cwd=staged[group], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    out, err = mm.mask_lines(r.stdout), mm.mask_lines(r.stderr)
    if slab:
        out.remove("user")
        err = [ln for ln in err if not ln.startswith("COMMAND --slab")]
    g = GOLD["groups"][group]
    assert out == g["all_verbose" if verbose else "all_plain"]
    assert [ln for ln in err if not ln.startswith("COMMAND -v")] == g["all_stderr"]
