"""seq_spectrum(30, 55, 100, 1000) next to seq_hashes on the same sequences, on the state of the yeast-like workload with its range
set. The sequences are the generator's haplotype A cut into 20 kb pieces. seq_hashes runs the same scan, look-up and one sort, so the difference is the
tally, the copy atomics and the finish. The two alternate in one process; call times by the host clock around calls that end in a synchronise, six rounds,
the first dropped. SP_UNDER_PROF=1 (for a run under rocprofv3 --kernel-trace --stats): three rounds of seq_spectrum only. The records come from build/gen_fqb
with the workload's parameters and seed 1 (it writes the haplotypes beside them) and are checked against bench.generate's."""
import json, os, subprocess, sys, tempfile, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench, hash10x_amd

PRM, PIECE = (30, 55, 100, 1000), 20000
PROF = bool(os.environ.get("SP_UNDER_PROF"))
wl = bench.WORKLOADS["yeast-like-2.5M"]
tmp = tempfile.mkdtemp(prefix="sp_measure_")
fqb, fa = os.path.join(tmp, "x.fqb"), os.path.join(tmp, "x")
subprocess.run([os.path.join(REPO, "build", "gen_fqb"), "-o", fqb, "-P", str(wl["pairs"]), "-C", str(wl["barcodes"]), "-G", str(wl["genome"]), "-e", str(wl["err"]),
                "-s", "1", "-m", str(wl["mol"]), "-S", str(wl["snp"]), "-L", str(wl["mol_len"]), "-fa", fa], check=True, stderr=subprocess.DEVNULL)
recs = np.fromfile(fqb, dtype=np.uint32)
same_records = bool(np.array_equal(recs, bench.generate(wl, seed=1)))
pairs = recs.size // 30
text = b"".join(ln.strip() for ln in open(fa + ".A.fa", "rb") if not ln.startswith(b">"))
codes = hash10x_amd.Hash10x._flatten_seqs([text])[0]
pieces = [codes[a:a + PIECE] for a in range(0, len(codes), PIECE)]
d = hash10x_amd.DeviceRecords(recs)
h = hash10x_amd.Hash10x(B=wl["B"])
h.read_fqb_device(d.ptr, pairs)
h.depth_range(wl["lo"], wl["hi"])
hash10x_amd.synchronize(0)
for f in (fqb, fa + ".A.fa", fa + ".B.fa"):
    os.remove(f)
os.rmdir(tmp)

res = {"build_id": hash10x_amd.build_id(), "workload": "yeast-like-2.5M (gen_fqb seed 1), haplotype A in 20 kb pieces", "records_equal_bench_generate": same_records,
       "pairs": pairs, "hashNumber": h.sizes()["hashNumber"], "params": PRM, "pieces": len(pieces), "bases": int(len(codes)), "seq_hashes_ms": [], "seq_spectrum_ms": []}
for rep in range(3 if PROF else 6):
    if not PROF:
        t0 = time.perf_counter()
        a = h.seq_hashes(pieces)
        res["seq_hashes_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    t0 = time.perf_counter()
    b = h.seq_spectrum(pieces, *PRM)
    res["seq_spectrum_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
    if rep == 0:
        res["info"] = dict(h.seq_spectrum_info)
        res["totals"] = b[4].tolist()
        if not PROF:
            fig = a[2]
            res["same_moshes_and_found"] = bool(np.array_equal(fig["moshes"], b[0]["moshes"]) and np.array_equal(fig["found"], b[0]["moshes"] - b[0]["absent"]))
if not PROF:
    for k in ("seq_hashes_ms", "seq_spectrum_ms"):
        v = res[k][1:]
        res[k + "_median_min_max"] = [round(float(np.median(v)), 3), min(v), max(v)]
print(json.dumps(res))
