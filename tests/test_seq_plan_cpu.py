"""The k-mer walk and the batch plan of hash10x_amd/csrc/seq_plan.hpp (the text the crib, mosh-set and readset scan kernels and their drivers run) against
the plain definitions, as a host program under AddressSanitizer and UBSan: tests/seq_plan_model.cpp, a stand-alone program built and run here. The list
estimate it prints is compared with gap_cases.scan_cap, which the GPU tests of the second attempt size their inputs by."""
import os
import subprocess

from gap_cases import scan_cap

HERE = os.path.dirname(os.path.abspath(__file__))


def test_seq_plan_model_under_asan(tmp_path):
    exe = str(tmp_path / "seq_plan_model")
    b = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", os.path.join(HERE, "seq_plan_model.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0, b.stdout.decode(errors="replace")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0, out + err
    assert "AddressSanitizer" not in err and "runtime error" not in err, err
    lines = out.splitlines()
    assert lines[-1] == "ok" and sum(ln.startswith("roll k") for ln in lines) == 7 and "plan: 42 batches" in lines
    caps = [ln for ln in lines if ln.startswith("cap ")]
    assert len(caps) == 10
    seen = set()
    for ln in caps:
        head, _, lens = ln.partition(":")
        _, k, w, value = head.split()
        lens = [int(x) for x in lens.split()]
        exp = scan_cap(lens, int(k), int(w))
        assert int(value) == exp, ln
        seen.add(exp == sum(max(0, n - int(k) + 1) for n in lens))
    assert seen == {True, False}                                 # both arms of the minimum
    assert "cap 19 31 74566 : 140000" in caps                   # the figure the second-attempt tests assert
