"""Are the kernels of csrc/stage_a.hip, stage_b.hip and stage_c*.hip the same, instruction for instruction, as those of another revision? (no GPU needed)
   python scratch/kdiff.py <rev>          e.g. the commit before a change that only moves code between files
Builds the device assembly of every stage_[abc]*.hip of <rev> and of the working tree with the Makefile's flags for those objects, cuts it into
functions, drops comments, takes the numbers off the local labels and compares, per kernel, the instruction list and the .amdhsa_ descriptor
lines (registers, LDS, scratch, waves). Kernels only the working tree has are listed; exit status 1 if a kernel of <rev> differs or is missing."""
import glob, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def compile_line(csrc, src):
    """the command the directory's own Makefile builds the unit's object with (make -n), turned into one that writes device assembly"""
    obj = os.path.basename(src)[:-4] + ".o"
    out = subprocess.run(["make", "-n", "-B", "-C", csrc, obj], stdout=subprocess.PIPE, check=True).stdout.decode()
    cmd = next(l for l in out.splitlines() if " -c " in l and obj in l).split()
    return [w for w in cmd[:cmd.index("-o")] if w != "-c"] + ["--cuda-device-only", "-S"]

def kernels(csrc, out):
    """{demangled name: (instruction lines, descriptor lines)} over every stage_[abc]*.hip of the directory"""
    found = {}
    for src in sorted(glob.glob(os.path.join(csrc, "stage_[abc]*.hip"))):
        asm = os.path.join(out, os.path.basename(src) + ".s")
        r = subprocess.run(compile_line(csrc, src) + ["-o", asm], cwd=csrc, stderr=subprocess.PIPE)
        if r.returncode: sys.exit("%s does not compile:\n%s" % (src, r.stderr.decode()))
        body, desc, cur, inDesc, pending = {}, {}, None, None, "?"
        for line in open(asm):
            line = re.sub(r"\.L(BB|tmp|func_begin|JTI)\d+", r".L\1", line.split(";")[0].rstrip())
            if not line.strip(): continue
            m = re.match(r"\s*\.type\s+(\w+),@function", line)
            if m: pending = m.group(1); continue
            if line == pending + ":": cur = pending; body[cur] = []; continue
            if line.startswith(".Lfunc_end"): cur = None; continue
            m = re.match(r"\s*\.amdhsa_kernel\s+(\w+)", line)
            if m: inDesc = m.group(1); desc[inDesc] = []; continue
            if line.strip() == ".end_amdhsa_kernel": inDesc = None; continue
            if inDesc is not None: desc[inDesc].append(line.strip())
            elif cur is not None: body[cur].append(line.strip())
        for sym in desc:                                          # kernels: the functions that have a descriptor
            name = subprocess.run(["c++filt", sym], stdout=subprocess.PIPE).stdout.decode().strip().replace("h10x::", "")
            found[name] = (body[sym], desc[sym], os.path.basename(src))
    return found

rev = sys.argv[1]
with tempfile.TemporaryDirectory() as tmp:
    os.makedirs(os.path.join(tmp, "old")); os.makedirs(os.path.join(tmp, "new"))
    tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "hash10x_amd/csrc", "include"], stdout=subprocess.PIPE, check=True).stdout
    subprocess.run(["tar", "-x", "-C", os.path.join(tmp, "old")], input=tar, check=True)
    oldDir = os.path.join(tmp, "old", "hash10x_amd", "csrc")
    open(os.path.join(oldDir, "build_id.h"), "w").write('#define H10X_BUILD_ID "kdiff"\n')
    old, new = kernels(oldDir, os.path.join(tmp, "old")), kernels(os.path.join(ROOT, "hash10x_amd", "csrc"), os.path.join(tmp, "new"))
bad = 0
print("%-58s %-20s %7s %7s  %s" % ("kernel", "now in", "lines", "before", "verdict"))
for name in sorted(old):
    if name not in new: print("%-58s %-20s %7s %7d  MISSING" % (name[:58], "-", "-", len(old[name][0]))); bad += 1; continue
    same = old[name][0] == new[name][0], old[name][1] == new[name][1]
    bad += not all(same)
    print("%-58s %-20s %7d %7d  %s" % (name[:58], new[name][2], len(new[name][0]), len(old[name][0]),
                                       "identical" if all(same) else ("INSTRUCTIONS DIFFER" if not same[0] else "DESCRIPTOR DIFFERS")))
for name in sorted(set(new) - set(old)): print("%-58s %-20s %7d %7s  new" % (name[:58], new[name][2], len(new[name][0]), "-"))
print("%d kernels of %s, %d differ or are missing" % (len(old), rev, bad))
sys.exit(1 if bad else 0)
