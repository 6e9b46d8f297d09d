"""the links between the ends of sequences on the molecule state of the yeast-like workload (after --cluster 1 0 --clusterSplit and
the range again). The sequences are the generator's two haplotypes cut into 20 kb pieces; ends of END_LEN bases, rows at minShare T, links at minBlocks M,
no cap. Two ways in one process, in alternation: (a) Hash10x.seq_blocks of the ends to the host plus the numpy join of tests/seqlinks_model.py;
(b) Hash10x.seq_links. Call times by the host clock around calls that end in a synchronise and include the copy-out, six rounds, the first dropped.
SL_UNDER_PROF=1 (for a run under rocprofv3 --kernel-trace --stats): three rounds of (b) only. The records come from build/gen_fqb with the workload's
parameters and seed 1 (it writes the haplotypes beside them) and are checked against bench.generate's."""
import json, os, subprocess, sys, tempfile, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import bench, hash10x_amd
import seqlinks_model as slm

T, M, END_LEN, PIECE = 5, 3, 5000, 20000
PROF = bool(os.environ.get("SL_UNDER_PROF"))
wl = bench.WORKLOADS["yeast-like-2.5M"]
tmp = tempfile.mkdtemp(prefix="sl_measure_")
fqb, fa = os.path.join(tmp, "x.fqb"), os.path.join(tmp, "x")
subprocess.run([os.path.join(REPO, "build", "gen_fqb"), "-o", fqb, "-P", str(wl["pairs"]), "-C", str(wl["barcodes"]), "-G", str(wl["genome"]), "-e", str(wl["err"]),
                "-s", "1", "-m", str(wl["mol"]), "-S", str(wl["snp"]), "-L", str(wl["mol_len"]), "-fa", fa], check=True, stderr=subprocess.DEVNULL)
recs = np.fromfile(fqb, dtype=np.uint32)
same_records = bool(np.array_equal(recs, bench.generate(wl, seed=1)))
pairs = recs.size // 30


def haplotype(path):
    text = b"".join(ln.strip() for ln in open(path, "rb") if not ln.startswith(b">"))
    return hash10x_amd.Hash10x._flatten_seqs([text])[0]


pieces = []
for name in (fa + ".A.fa", fa + ".B.fa"):
    codes = haplotype(name)
    pieces += [codes[a:a + PIECE] for a in range(0, len(codes), PIECE)]
d = hash10x_amd.DeviceRecords(recs)
h = hash10x_amd.Hash10x(B=wl["B"])
h.read_fqb_device(d.ptr, pairs)
h.depth_range(wl["lo"], wl["hi"]); h.cluster(1, 0, wl["ct"]); h.cluster_split(); h.depth_range(wl["lo"], wl["hi"])
hash10x_amd.synchronize(0)
for f in (fqb, fa + ".A.fa", fa + ".B.fa"):
    os.remove(f)
os.rmdir(tmp)
ends = slm.cut_ends(pieces, END_LEN)

res = {"build_id": hash10x_amd.build_id(), "workload": "yeast-like-2.5M (gen_fqb seed 1 with its haplotypes), after --cluster 1 0 --clusterSplit, range again",
       "records_equal_bench_generate": same_records, "pairs": pairs, "nBlocks": h.sizes()["nBlocks"], "minShare": T, "minBlocks": M, "endLen": END_LEN, "maxEnds": 0,
       "pieces": len(pieces), "end_bases": int(sum(len(e) for e in ends)), "host_route_ms": [], "seq_links_ms": []}


def host_route():
    """the rows of the ends to the host, then the join in numpy"""
    off, blk, _, _ = h.seq_blocks(ends, T)
    return slm.row_links(off, blk, M, 0, True)[:3]


for rep in range(3 if PROF else 6):
    if not PROF:
        t0 = time.perf_counter()
        a = host_route()
        res["host_route_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    t0 = time.perf_counter()
    b = h.seq_links(pieces, T, M, END_LEN)
    res["seq_links_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    if rep == 0:
        res["info"] = dict(h.seq_links_info)
        if not PROF:
            res["equal"] = bool(all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b)))
            # the algorithmic bytes of the pair gather: per pair one place searched (8 B at least), one partner key read (8 B) and one key written (K B);
            # per row entry 8 B of its own key, 8 B of place and 4 B of source
            K = 8 if res["info"]["wideBatches"] else 4
            res["gather_kernel_bytes"] = {"partners": 8 * res["info"]["pairs"], "keys": K * res["info"]["pairs"], "units": 20 * res["info"]["rowEntries"]}
if not PROF:
    for k in ("host_route_ms", "seq_links_ms"):
        v = res[k][1:]
        res[k + "_median_min_max"] = [round(float(np.median(v)), 3), min(v), max(v)]
print(json.dumps(res))
