"""--codeExplore without a loaded state (no GPU needed): the reference's "!! you must set hashDepthRange before codeExplore"
(hash10x.c:1226-1232), on the command line and in --interactive, against the reference binary."""
import os
import subprocess

import pytest

import orc

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")


def _mask(b):
    """the command's own lines (the resource lines of the other commands are compared by tests/test_interactive_cpu.py)"""
    return [ln for ln in b.decode(errors="replace").replace("> ", "").splitlines() if ln.startswith(("!!", "  unknown", "COMMAND"))]


def _both(args, tmp_path, script=None):
    if not orc.have_ref() or not os.path.exists(EXE):
        pytest.fail("build() first: needs bin/hash10x-amd and oracle/_ref/hash10x")
    env = dict(os.environ, MALLOC_PERTURB_="255", GLIBC_TUNABLES="glibc.malloc.tcache_count=0")
    ref = subprocess.run([os.path.join(orc.REF_DIR, "hash10x")] + args, input=script, cwd=str(tmp_path), env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    hip = subprocess.run([EXE] + args, input=script, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert hip.returncode == ref.returncode == 0
    assert _mask(hip.stdout) == _mask(ref.stdout)
    assert _mask(hip.stderr) == _mask(ref.stderr)
    return hip


def test_code_explore_before_range(tmp_path):
    hip = _both(["-k", "21", "--codeExplore", "5", "-o", "out", "--codeExplore", "2"], tmp_path)
    assert b"!! you must set hashDepthRange before codeExplore\n" in hip.stdout
    assert b"!! you must set hashDepthRange before codeExplore\n" in hip.stderr           # under -o: the file and stderr
    assert open(os.path.join(str(tmp_path), "out"), "rb").read().count(b"!! you must set hashDepthRange before codeExplore\n") == 1


def test_code_explore_interactive(tmp_path):
    hip = _both(["-k", "21", "--interactive"], tmp_path, b"codeExplore 5\ncodeExplore\nclusterThreshold 2\ncodeExplore 0\nquit\n")
    assert hip.stdout.count(b"!! you must set hashDepthRange before codeExplore\n") == 2


def test_code_explore_usage():
    p = subprocess.run([EXE, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert b"--codeExplore <code>" in p.stderr
