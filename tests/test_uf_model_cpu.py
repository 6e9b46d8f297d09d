"""The lock-free union by smaller label of hash10x_amd/csrc/unionfind.hpp (the text stage_m.hip and stage_n.hip run on the device) as a host
program on std::atomic, 16 threads, under ThreadSanitizer: tests/uf_model.cpp, a stand-alone program built and run here."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_union_find_model_under_tsan(tmp_path):
    exe = str(tmp_path / "uf_model")
    b = subprocess.run(["g++", "-O1", "-g", "-fsanitize=thread", "-std=c++17", "-pthread", os.path.join(HERE, "uf_model.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b.returncode == 0, b.stdout.decode(errors="replace")
    r = subprocess.run([exe, "60"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)   # 60 graphs of up to 3000 blocks, 16 threads
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0, r.stdout.decode(errors="replace") + err
    assert "ok" in r.stdout.decode().split()
    assert "WARNING: ThreadSanitizer" not in err, err
