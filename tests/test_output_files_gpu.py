"""An output stands under its name only when it is whole: the commands that write the project's own formats, through bin/hash10x-amd on the
golden small set (-B 20, -ct 2, depth range 3 .. 14, clustered: the command line of test_cli_whole_command_line_under_sanitizers). Per command
three fresh processes: a good run leaves the file and no .part; a path inside a missing directory dies with "failed to open output file <path>"
and leaves nothing; a refused run over the good file leaves its bytes alone. The refused form is minShare 0 where the command refuses that, and
otherwise the command ahead of --hashDepthRange: --writeMosh right behind --readFQB, and --moleculeMap at the head of the line, ahead of the
state itself, because behind --readFQB it has an answer (every read pair unclustered) and is not refused."""
import glob
import os
import subprocess

import pytest

import orc

pytestmark = pytest.mark.gpu

EXE = os.path.join(orc.REPO, "bin", "hash10x-amd")
READ = ["--readFQB", "small.fqb"]
STATE = READ + ["--hashDepthRange", "3", "14", "--cluster", "1", "0"]

# name: (arguments in front of the path, extension, the refused command line for an output path, its exit code, its message)
COMMANDS = {
    "moleculeMap": (["--moleculeMap"], "mol", lambda p: ["--moleculeMap", p], 255, "FATAL ERROR: moleculeMap: no hash state loaded: use readFQB or readHash first"),
    "shareGraph": (["--shareGraph", "2"], "sg", lambda p: STATE + ["--shareGraph", "0", p], 0, "!! shareGraph minShare 0 must be >= 1"),
    "shareComponents": (["--shareComponents", "2"], "sc", lambda p: STATE + ["--shareComponents", "0", p], 0, "!! shareComponents minShare 0 must be >= 1"),
    "hashCopies": (["--hashCopies", "2"], "hc", lambda p: STATE + ["--hashCopies", "0", p], 0, "!! hashCopies minShare 0 must be >= 1"),
    "writeMosh": (["--writeMosh", "0", "4", "7", "10"], "mosh", lambda p: READ + ["--writeMosh", "0", "4", "7", "10", p] + STATE[2:], 0, "!! you must set hashDepthRange before writeMosh"),
}


def _run(d, args):
    p = subprocess.run([EXE, "-B", "20", "-ct", "2"] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p.returncode, p.stdout.decode() + p.stderr.decode()


def _read(name, path):
    import hash10x_amd
    return {"moleculeMap": hash10x_amd.read_molecule_map, "shareGraph": hash10x_amd.read_share_graph, "shareComponents": hash10x_amd.read_share_components,
            "hashCopies": hash10x_amd.read_hash_copies, "writeMosh": hash10x_amd.read_mosh_file}[name](path)


@pytest.mark.parametrize("name", list(COMMANDS))
def test_output_appears_only_when_whole(workdir, name):
    head, ext, refused, refused_rc, refused_text = COMMANDS[name]
    d = workdir.path
    workdir.need("small.fqb.gz")
    out = "good." + ext
    # 1. a good run: the file, whole, and no .part
    rc, text = _run(d, STATE + head + [out])
    assert rc == 0, text[-1000:]
    assert os.path.exists(os.path.join(d, out)) and not glob.glob(os.path.join(d, "*.part"))
    _read(name, os.path.join(d, out))
    good = open(os.path.join(d, out), "rb").read()
    # 2. a path that cannot be opened: the message as it always was, nothing left
    bad = "nodir/x." + ext
    rc, text = _run(d, STATE + head + [bad])
    assert rc == 255 and "FATAL ERROR: failed to open output file %s\n" % bad in text, (rc, text[-1000:])
    assert not os.path.exists(os.path.join(d, "nodir")) and not glob.glob(os.path.join(d, "*.part"))
    # 3. a refused run over the good file: its bytes stay
    rc, text = _run(d, refused(out))
    assert rc == refused_rc and refused_text + "\n" in text, (rc, text[-1000:])
    assert open(os.path.join(d, out), "rb").read() == good and not glob.glob(os.path.join(d, "*.part"))
