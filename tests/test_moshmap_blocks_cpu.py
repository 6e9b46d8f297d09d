"""The scripted seed streams of tests/map_cases.py without a device: per case the integer walk blocks(), the text model RefModel.query and the
lines the reference's moshmap printed (tests/golden/map_blocks.json, tests/golden/make_map_blocks_golden.py) agree; the generated files are the
ones the reference ran on; and every wrong walk of VARIANTS is told from the right one by a named case. Every comparison is exact."""
import hashlib
import json
import os

import pytest

import map_cases as mc
import orc

with open(os.path.join(orc.GOLDEN, "map_blocks.json")) as f:
    GOLD = json.load(f)
IDS = [c.name for c in mc.CASES]


def test_fixture_holds_these_cases():
    assert list(GOLD["groups"]) == list(mc.GROUPS)
    for g, cases in mc.GROUPS.items():
        assert sorted(GOLD["groups"][g]["cases"]) == sorted(c.name for c in cases if c.kind != "empty")
    fam = {f: [len(c.expect) for c in mc.CASES if c.family == f] for f in mc.FAMILIES}
    assert GOLD["records_per_family"] == fam


@pytest.mark.parametrize("group", list(mc.GROUPS))
def test_generated_files_are_the_fixtures(group):
    """a drift of the builder, the hasher or the file writers: the recorded lines would no longer belong to these bytes"""
    b = mc.built(group)
    assert {n: hashlib.sha256(d).hexdigest() for n, d in b["files"].items()} == GOLD["groups"][group]["sha256"]


@pytest.mark.parametrize("c", mc.CASES, ids=IDS)
def test_walk_model_and_reference_agree(c):
    b = mc.built(c.group)
    n = b["cases"].index(c)
    s, script = b["queries"][n], b["scripts"][n]
    seeds = mc.expected_seeds(script)
    assert mc.seeds_of(b["ms"], b["ref"], s) == seeds
    recs = mc.blocks(seeds)
    # what the case is for, as its author wrote it down
    assert [(r[4], r[5]) for r in recs] == c.expect
    assert [r[2] - b["base"][c.name] for r in recs] == list(c.starts)
    assert len(recs) <= (sum(x[0] in (1, 2) for x in seeds)) // 3 + 1                 # the room rm_count_kernel reserves
    # the text model
    ev = b["ref"].query(c.name, s, False)
    model = [ln.rstrip("\n") for _, ln in ev]
    assert model[1:] == mc.m_lines(b["ref"], c.name, s, recs, sum(x[0] == 1 for x in seeds))
    counts = [sum(x[0] == k for x in seeds) for k in range(4)]
    assert model[0] == "Q\t%s\t%d\t%d miss, %d copy1, %d copy2, %d multi, %s hit" % (c.name, len(s), counts[0], counts[1], counts[2], counts[3],
                                                                                    mc.mp.c_ratio(len(seeds) - counts[0], len(seeds)))
    # the reference: its own run, and its lines in the runs over all.fa
    g = GOLD["groups"][c.group]
    plain, verbose = mc.split_queries(g["all_plain"]), mc.split_queries(g["all_verbose"])
    if c.kind == "empty":                                        # reading stops at a sequence without bases: no line at all
        assert c.name not in plain and c.name not in verbose and c.name not in g["cases"]
        return
    assert g["cases"][c.name]["status"] == 0
    assert [ln for ln in g["cases"][c.name]["stdout"] if ln[:2] in ("Q\t", "M\t")] == model
    assert plain[c.name] == model
    assert verbose[c.name] == [ln.rstrip("\n") for _, ln in b["ref"].query(c.name, s, True)]


def test_queries_are_what_the_cases_say():
    b = mc.built("x")
    n = {c.name: len(sc) for c, sc in zip(b["cases"], b["scripts"])}
    assert all(340 <= n[c.name] <= 440 for c in b["cases"] if c.kind == "random" and not c.cut and not c.repeat), n
    assert (n["tile_cut_64"], n["tile_cut_65"], n["tile_cut_128"], n["none_empty"], n["none_shorter_than_k"]) == (64, 65, 128, 0, 0)
    rep = b["scripts"][[c.name for c in b["cases"]].index("dir_equal_loc_stays")]
    assert sum(rep[i] is not None and rep[i] == rep[i + 1] for i in range(len(rep) - 1)) == 1
    room = mc.expected_seeds(b["scripts"][[c.name for c in b["cases"]].index("room_71_records")])
    assert (sum(x[0] == 1 for x in room) + sum(x[0] == 2 for x in room)) // 3 + 1 == 72 and len(mc.BY_NAME["room_71_records"].expect) == 71 > mc.TILE


@pytest.mark.parametrize("variant", mc.VARIANTS)
def test_every_wrong_walk_is_caught_by_its_named_case(variant):
    """a case list thinned later fails here: the variant's records must differ on the case CATCHES names for it"""
    c = mc.BY_NAME[mc.CATCHES[variant]]
    b = mc.built(c.group)
    seeds = mc.expected_seeds(b["scripts"][b["cases"].index(c)])
    assert mc.blocks(seeds, variant) != mc.blocks(seeds), "%s does not tell %s from the reference's walk" % (c.name, variant)


def test_builder_refuses_what_would_blur_a_script():
    a = mc.case("a", "drift", mc.Sc().one(10, 11), [], [])
    with pytest.raises(AssertionError, match="scripted twice"):
        mc.build([a._replace(script=[(1, 10), (2, 5, 10)])])
    with pytest.raises(AssertionError, match="is mosh 0 of a"):                         # the same query twice: its moshes are no longer distinct
        mc.build([a, a])
