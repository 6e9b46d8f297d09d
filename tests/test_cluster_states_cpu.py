"""The hand-built states of tests/cluster_states.py through the CPU oracle and the REAL reference binary: canonical bytes equal, and every case
still sits at the boundary it was built for (cluster_states.check: the oracle's labels, cluster counts and pointToMin equal the builder's own replay
of codeClusterFind and codeClusterReadMerge, bit for bit). Pins the oracle on shapes no generated set gives it; runs where oracle/_ref exists."""
import os

import numpy as np
import pytest

import cluster_states as cs
import orc


def test_plain_image_is_hash_image():
    blocks = [[3, 1, 2], [], [2, 3, 7, 7]]
    assert cs.plain_image(blocks) == orc.hash_image(blocks)


def test_builder_refuses_what_the_reference_would_read_out_of_bounds():
    rec = np.zeros(2, dtype=orc.CLUSHASH)
    rec["hash"] = [1, 2]; rec["read"] = [0, 3]
    with pytest.raises(AssertionError):
        cs.image([(rec, 3, 0, 0.0)])                         # a read beyond nRead
    with pytest.raises(AssertionError):
        cs.image([(rec, 4, 256, 0.0)])                       # more than 255 clusters in the file
    st = cs.State(); s = st.subject(n_sub=2)
    s.extra(label=3)
    st.build()
    with pytest.raises(AssertionError):
        s.expect(1)                                          # a label beyond the clusters the read merge sees


@pytest.mark.skipif(not orc.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", list(cs.CASES))
def test_oracle_matches_reference(tmp_path, name):
    cwd = str(tmp_path)
    got, n_good = cs.run_oracle(name, cwd)
    r = orc.run_ref(cs.args(name, name + ".in.hash", "ref.hash"), cwd)
    assert r.returncode == 0, r.stderr.decode()
    ref = orc.canonical_hash_bytes(open(os.path.join(cwd, "ref.hash"), "rb").read())
    assert got == ref, orc.describe_diff(got, ref)
    cs.check(name, orc.HashFile(got), n_good)
