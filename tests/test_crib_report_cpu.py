"""The cases of tests/crib_cases.py without a GPU: every case's own check of where it sits, the model's text (tests/crib_model.py) against the
reference binary's recorded output (tests/golden/crib/, made by tests/golden/make_crib_golden.py) and, where oracle/_ref exists, against the
reference binary run then and there on the same files. Pins the model that test_crib_report_gpu.py compares the kernels with."""
import os

import numpy as np
import pytest

import cluster_states as cs
import crib_cases as cc
import crib_model as cm
import orc

NAMES = list(cc.CASES)


def test_image_defaults_give_the_bytes_of_before():
    """cluster_states.image with its new arguments left out, and with the old contents passed in, is orc.hash_image"""
    blocks = [[3, 1, 2], [], [2, 3, 7, 7]]
    recs = []
    for b in blocks:
        rec = np.zeros(len(b), dtype=orc.CLUSHASH)
        rec["hash"] = b
        recs.append((rec, 1, 0, 0.0))
    old = orc.hash_image(blocks)
    assert cs.image(recs) == old and cs.plain_image(blocks) == old
    assert cs.image(recs, values=np.arange(8, dtype=np.uint64) * 31, table=np.zeros(1 << 20, dtype=np.uint32)) == old


def test_probe_table_finds_every_member():
    """the table of a case is what hashIndexFind walks: every value is found at its index, also where two values share their first slot"""
    values = np.array([0, 5, 5 + (1 << 20), 5 + (2 << 20), 0, 7 << 40], dtype=np.uint64)
    t = cc.probe_table(values)
    mask = (1 << 20) - 1
    for i in range(1, len(values)):
        h = int(values[i]); off, diff = h & mask, ((h >> 20) & mask) | 1
        while int(values[int(t[off])]) != h:
            assert t[off]
            off = (off + diff) & mask
        assert t[off] == i
    assert np.count_nonzero(t) == 5 and t[5] == 1 and t[0] == 4
    st = cc.built("S4_value0_w31")[0]
    hf = orc.HashFile(cc.built("S4_value0_w31")[2])
    assert hf.hash_value[st.names["zero"]] == 0 and hf.hash_index[0] == st.names["zero"] and hf.hash_number == len(st.values)


@pytest.mark.parametrize("name", NAMES)
def test_case_sits_where_it_is_built_for(name):
    cc.built(name)                                           # runs the case's own check


@pytest.mark.parametrize("name", NAMES)
def test_model_text_matches_recorded_reference(name):
    ref = cc.golden(name)
    got = cc.model_text(name)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a == b, "%s, line %d:\n  model: %s\n  ref:   %s" % (name, i, a, b)
    assert len(got) == len(ref) and len(ref) >= 269


def test_recorded_text_shows_what_the_cases_are_about():
    """the reference's own lines at the edges: 0 / 0 as -nan, the wrapped chr, the wrapped position bin, ten OTHER hashes of 25"""
    text = {n: "\n".join(cc.golden(n)) + "\n" for n in NAMES}
    assert "    hom    0 mean -nan min -1 max -1\n" in text["S6_no_hom"] and "    err   0 mean -nan min -1 max -1\n" in text["S6_no_err"]
    assert "  0 cluster codes  err 0 0 -nan htA 0 0 -nan htB 0 0 -nan hom 0 0 -nan mul 0 0 -nan\n" in text["R1_sizes"]
    assert " chr 32767 pos 1 1  OTHER 1 " in text["S4_counts"] and " chr 32767 pos 0 1" in text["S7_32767_sequences"]
    assert " chr 1 pos 0 65536" in text["S3_long"]                       # bins 65535 and (wrapped) 0 in one cluster
    assert "CRIB_TABLE       255" in text["S6_pairs"] and "CRIB_TABLE       256" not in text["S6_pairs"]
    other = [ln for ln in text["R4_other_lists"].splitlines() if " OTHER 25 " in ln]
    assert len(other) == 1 and len(other[0].split(" OTHER 25 ")[1].split()) == 10
    assert text["R1_sizes"].count("  MIN_POINT_DENSITY ") == 4 and text["R1_sizes"].count("  CLUSTER_SUMMARY 0 ") == 2


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", NAMES)
def test_model_text_matches_reference_binary(tmp_path, name):
    files = cc.write_files(name, str(tmp_path))
    r = orc.run_ref(cc.args(name, *files), str(tmp_path))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    ref, got = cm.report(r.stdout), cc.model_text(name)
    for i, (a, b) in enumerate(zip(got, ref)):
        assert a == b, "%s, line %d:\n  model: %s\n  ref:   %s" % (name, i, a, b)
    assert len(got) == len(ref)
    for p in files:                                          # (67 MB for S3_long)
        os.remove(os.path.join(str(tmp_path), p))
