"""the molecule map and the split on the yeast-like workload through the C ABI on device arrays; call times by the host clock around
calls that end in a synchronise. MOL_UNDER_PROF=1 (for a run under rocprofv3 --kernel-trace --stats): the default form only."""
import ctypes, json, os, sys, time
import numpy as np
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench, hash10x_amd

wl = bench.WORKLOADS["yeast-like-2.5M"]
recs = bench.generate(wl, seed=1)
pairs = recs.size // 30
hip, host = hash10x_amd.load_native()
d = hash10x_amd.DeviceRecords(recs)
h = hash10x_amd.Hash10x(B=wl["B"])
h.read_fqb_device(d.ptr, pairs); h.depth_range(wl["lo"], wl["hi"]); h.cluster(1, 0, wl["ct"])
hash10x_amd.synchronize(0)
z = h.sizes()
ctx = h._ctx()
info = hash10x_amd._MolInfo()
assert hip.h10x_molecule_map(ctx, None, None, 0, ctypes.byref(info)) == 0, hip.h10x_last_error(ctx)
R = int(info.nRecords)
dmol, dslot = hip.h10x_device_malloc(0, 4 * R), hip.h10x_device_malloc(0, 4 * R)
out = hash10x_amd.DeviceRecords(np.zeros(0, dtype=np.uint32), 0, _words=R * 30)
start = np.zeros(int(info.nBlocks) + int(info.nMolecules) + 1, dtype=np.uint64)
res = {"build_id": hash10x_amd.build_id(), "workload": "yeast-like-2.5M (bench.py, gen_fqb seed 1)", "pairs": pairs, "R": R, "H": z["nClusHash"], "nBlocks": int(info.nBlocks),
       "nMolecules": int(info.nMolecules), "nClustered": int(info.nClustered), "map_ms": [], "info_ms": [], "split_ms": []}
PROF = bool(os.environ.get("MOL_UNDER_PROF"))
for form in ((0,) if PROF else (0, 1)):
    h.set_option("molmap_global", form)
    key = "" if form == 0 else "_global"
    res["map_ms" + key], res["split_ms" + key] = [], []
    for rep in range(6):
        t0 = time.perf_counter()
        assert hip.h10x_molecule_map_device(ctx, dmol, dslot, R, ctypes.byref(info)) == 0, hip.h10x_last_error(ctx)
        t1 = time.perf_counter()
        assert hip.h10x_split_fqb_device(ctx, d.ptr, R, out.ptr, start.ctypes.data, start.size) == 0, hip.h10x_last_error(ctx)
        t2 = time.perf_counter()
        res["map_ms" + key].append(round(1e3 * (t1 - t0), 3)); res["split_ms" + key].append(round(1e3 * (t2 - t1), 3))
h.set_option("molmap_global", 0)
for rep in range(0 if PROF else 4):
    t0 = time.perf_counter()
    assert hip.h10x_molecule_map(ctx, None, None, 0, ctypes.byref(info)) == 0
    res["info_ms"].append(round(1e3 * (time.perf_counter() - t0), 3))
# the split file against the map, on the host: every record where the map says
mol, slot = np.zeros(R, dtype=np.uint32), np.zeros(R, dtype=np.uint32)
assert hip.h10x_device_download(0, mol.ctypes.data, dmol, 4 * R) == 0 and hip.h10x_device_download(0, slot.ctypes.data, dslot, 4 * R) == 0
out.n_records = R
o = out.download()
r30 = recs.reshape(-1, 30)
clustered = mol >= int(info.nBlocks)
dest = start[mol[clustered]].astype(np.int64) + slot[clustered]
res["split_matches_map_on_clustered"] = bool(np.array_equal(o[dest], r30[:R][clustered]))
res["start_last"] = int(start[-1])
print(json.dumps(res))
