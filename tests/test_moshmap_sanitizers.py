"""The device-free parts of host/map_host.c (the RFMSHv1 reader and writer, the name dictionary, the Q / M / -v formatters) under
AddressSanitizer + UndefinedBehaviorSanitizer, through the stand-alone driver host/map_asan_driver.c (`make asan`). Nothing sanitized is
loaded into Python."""
import os
import struct
import subprocess

import pytest

import map_model as mp
import orc

REPO = orc.REPO
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="halt_on_error=1:exitcode=67")
DRV = os.path.join(REPO, "build", "map-host-asan")


@pytest.fixture(scope="module")
def drv():
    if not os.path.exists(DRV):
        subprocess.run(["make", "-C", os.path.join(REPO, "hash10x_amd", "host"), "asan"], check=True, stdout=subprocess.DEVNULL)
    return DRV


def go(drv, args, cwd):
    r = subprocess.run([drv] + [str(a) for a in args], cwd=str(cwd), env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode not in (66, 67) and b"ERROR: AddressSanitizer" not in r.stderr and b"runtime error:" not in r.stderr, r.stderr.decode(errors="replace")[-2000:]
    return r


@pytest.mark.parametrize("stem", ["build.idx", "many.many", "params.p"])
def test_golden_ref_files_round_trip(drv, stem, tmp_path):
    """read with every check, every name found through the table, written back: the same bytes"""
    data = mp.gold(stem + ".ref")
    set_max = struct.unpack_from("<I", mp.gold(stem + ".mosh"), 12)[0] - 1
    (tmp_path / "in.ref").write_bytes(data)
    r = go(drv, ["ref", "in.ref", set_max, "out.ref"], tmp_path)
    assert r.returncode == 0, r.stderr.decode()
    assert (tmp_path / "out.ref").read_bytes() == data


@pytest.mark.parametrize("name,data,message", mp.bad_refs(), ids=[b[0] for b in mp.bad_refs()])
def test_malformed_ref_files_end_with_a_message(drv, name, data, message, tmp_path):
    set_max = struct.unpack_from("<I", mp.gold("build.idx.mosh"), 12)[0] - 1
    (tmp_path / "bad.ref").write_bytes(data)
    r = go(drv, ["ref", "bad.ref", set_max, "out.ref"], tmp_path)
    assert r.returncode == 3 and message in r.stderr.decode(), r.stderr.decode()


def test_dict_and_formatters(drv, tmp_path):
    r = go(drv, ["dict", 400], tmp_path)
    d = mp.DictModel(1024)
    for i in range(400):
        d.add("s%d" % i)
    assert r.returncode == 0 and r.stdout.decode().startswith("dim %d max %d " % (d.dim, d.max)) and r.stdout.decode().rstrip().endswith("lenDim 1024 lenMax 400")
    r = go(drv, ["dict", 5000], tmp_path)
    assert r.returncode == 0 and " lenDim %d lenMax 5000" % mp.array_dim_after(5000) in r.stdout.decode()
    r = go(drv, ["fmt"], tmp_path)
    assert r.returncode == 0
    assert r.stdout.decode().splitlines() == ["Q\tshort\t12\t0 miss, 0 copy1, 0 copy2, 0 multi, -nan hit", "Q\tq\t4000\t3 miss, 150 copy1, 2 copy2, 1 multi, 0.98 hit",
                                              "M\tdup\t92\t2947\t3000\tchrA\t10592\t13447\t0 96\t1.00\t-nan", "M\tflat\t5\t5\t100\tchrB\t1\t1\t3 0\tinf\t1.00",
                                              "      17\tchrA 5", "      18\tchrA 5\tchrB 6"]
