"""The model of tests/map_model.py against the reference's moshmap, byte for byte, on the golden fixtures of tests/golden/map
(tests/golden/make_map_golden.py): what makes the model usable as the expected result on fresh inputs where the reference is not at hand."""
import pytest

import map_model as mp

MAN = mp.manifest()


@pytest.mark.parametrize("case", MAN["cases"], ids=[c["name"] for c in MAN["cases"]])
def test_model_matches_reference_golden(case, tmp_path):
    d = str(tmp_path)
    before = mp.stage_case(MAN, case, d)
    status, out, err = mp.run_commands(case["args"], d)
    mp.check_case(case, d, before, status, out.encode(), err.encode())


def test_dict_doubles_past_307_names():
    """dict.c:172: the table of 1024 doubles when max > 0.3 * size, that is with the 308th name; the golden `many` case holds 310"""
    d = mp.DictModel(1024)
    for i in range(307):
        d.add("s%d" % i)
    assert (d.dim, d.size) == (10, 1024)
    d.add("s307")
    assert (d.dim, d.size) == (11, 2048)
    ref = mp.gold("many.many.ref")
    assert mp.mask_ref(ref) == ref
    assert mp.RefModel.from_bytes(mp.mm.MoshModel.from_bytes(mp.gold("many.many.mosh")), ref).dict.dim == 11
