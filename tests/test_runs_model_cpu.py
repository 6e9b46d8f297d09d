"""The galloping run search of hash10x_amd/csrc/runs.hpp (the text the census tail's run kernel and stage_q.hip's block-run kernels run on the
device) against a linear walk, as a host program under AddressSanitizer and UBSan: tests/runs_model.cpp, a stand-alone program built and run here."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_run_end_model_under_asan(tmp_path):
    exe = str(tmp_path / "runs_model")
    b = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-std=c++17", os.path.join(HERE, "runs_model.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0, b.stdout.decode(errors="replace")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out, err = r.stdout.decode(errors="replace"), r.stderr.decode(errors="replace")
    assert r.returncode == 0, out + err
    assert "ok" in out.split() and out.count("cases") == 5
    assert "AddressSanitizer" not in err and "runtime error" not in err, err
