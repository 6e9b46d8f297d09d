"""--interactive (hash10x.c:1281-1300) against the reference binary, without loading data (no GPU needed): the same stdin script
gives the same stdout and stderr. Masked: resource lines, and the usage text that --help (an empty line) prints, whose option list is
this program's own."""
import os
import re
import subprocess

import pytest

import orc

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
USAGE = ("Usage:", "Commands can", "Be sure", "   ")


def _mask_out(b):
    return [re.sub(r"user\t.*", "user", ln) for ln in b.decode(errors="replace").splitlines()]


def _mask_err(b):
    return [ln for ln in b.decode(errors="replace").splitlines() if not ln.startswith(USAGE)]


SCRIPTS = [
    b"\n  hashExplore 5\nfoo 1 2\n-k 19\nhashInfo 1 2\nhashInfo 1 2 3\ndoubleShared 4 5\nquit\nhelp\n",   # ends at quit
    b"k 19\n\n   \nbogus\ncodeStats\nhashExplore",                                                       # end of input inside a line
    b"shareScan 3 5\nexit\n",
    b"",
]


@pytest.mark.parametrize("i", range(len(SCRIPTS)))
def test_interactive_matches_reference(tmp_path, i):
    if not orc.have_ref() or not os.path.exists(EXE):
        pytest.fail("build() first: needs bin/hash10x-amd and oracle/_ref/hash10x")
    args = ["-k", "21", "--interactive", "-w", "5"]
    env = dict(os.environ, MALLOC_PERTURB_="255", GLIBC_TUNABLES="glibc.malloc.tcache_count=0")
    ref = subprocess.run([os.path.join(orc.REF_DIR, "hash10x")] + args, input=SCRIPTS[i], cwd=str(tmp_path), env=env,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    hip = subprocess.run([EXE] + args, input=SCRIPTS[i], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert hip.returncode == ref.returncode
    assert _mask_out(hip.stdout) == _mask_out(ref.stdout)
    assert _mask_err(hip.stderr) == _mask_err(ref.stderr)
    assert b"> " in hip.stdout


def test_interactive_no_command_echo():
    p = subprocess.run([EXE, "--interactive"], input=b"k 19\nquit\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    out = p.stdout.decode()
    assert out.count("COMMAND") == 1 and "COMMAND --interactive" in out and out.count("> ") == 2
