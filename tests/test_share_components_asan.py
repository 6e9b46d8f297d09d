"""The host code of --shareComponents under AddressSanitizer + UBSan, in stand-alone programs (no device): the .sc writer behind a main of
its own, whose files read_share_components must accept, and the sanitized hash10x-amd refusing the command before any state is loaded."""
import os
import subprocess

import numpy as np
import pytest

import orc

REPO = orc.REPO
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=66", UBSAN_OPTIONS="halt_on_error=1:exitcode=67")   # (the HIP runtime, linked in, keeps its own allocations)


def _built(name):
    path = os.path.join(REPO, "build", name)
    if not os.path.exists(path):
        subprocess.run(["make", "-C", os.path.join(REPO, "hash10x_amd", "host"), "asan"], check=True, stdout=subprocess.DEVNULL)
    return path


def _clean(r):
    assert r.returncode not in (66, 67) and b"ERROR: AddressSanitizer" not in r.stderr and b"runtime error:" not in r.stderr, r.stderr.decode(errors="replace")[-2000:]


@pytest.mark.parametrize("n_blocks", [0, 1, 2, 6, 1001])
def test_sc_writer_under_sanitizers(tmp_path, n_blocks):
    import hash10x_amd
    drv = _built("sc-host-asan")
    p = str(tmp_path / "w.sc")
    r = subprocess.run([drv, p, str(n_blocks)], env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    _clean(r)
    assert r.returncode == 0 and b"failed to open output file" in r.stdout, r.stderr.decode()
    members = max(n_blocks - 1, 0)
    n_comp = (members + 1) // 2
    assert os.path.getsize(p) == 32 + 4 * n_blocks + 16 * (n_comp + 1)
    if n_blocks == 0:
        return                                                 # (a header and entry 0 alone: no block 0 for the reader to place)
    info, comp, root_of, blocks, records = hash10x_amd.read_share_components(p)
    assert info == {"version": 1, "nBlocks": n_blocks, "minShare": 5, "nComponents": n_comp, "largest": min(members, 2), "rows": 2 * (members // 2)}
    c = np.arange(n_blocks)
    assert np.array_equal(comp, (c + 1) // 2) and np.array_equal(root_of[1:], np.arange(1, n_blocks, 2))
    assert int(blocks.sum()) == members and int(records.sum()) == 1000 * int(c.sum())


def test_cli_refuses_under_sanitizers(tmp_path):
    exe = _built("hash10x-amd-asan")
    r = subprocess.run([exe, "-B", "20", "--shareComponents", "5", "x.sc"], cwd=tmp_path, env=ENV, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    _clean(r)
    assert r.returncode == 0 and b"!! you must set hashDepthRange before shareComponents\n" in r.stdout and not (tmp_path / "x.sc").exists()
