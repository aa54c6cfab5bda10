"""Host path (kamd_index_load + kamd_index_upload) against device path (kamd_index_load_deferred + kamd_index_upload, the k-mer table built on the
GPU) on config #3's index, alternating within one process (run on a GPU box).  usage: python scratch/ixbuild_timing.py [--genes N] [--reps R] [--out FILE.json]"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench, kallisto_amd as ka
ap = argparse.ArgumentParser()
ap.add_argument("--genes", type=int, default=20000)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--out", default=None, help="also write the rows to this JSON file")
a = ap.parse_args()
cat, tl, idx = bench.prepare_workload("human", a.genes, True)
ctx = ka.Context(0)
rows = []
for rep in range(a.reps):
    for deferred in (False, True):
        t = time.time(); ix = ka.Index(idx, a.threads, deferred=deferred); t1 = time.time() - t
        torch.cuda.synchronize(); t = time.time(); ctx.upload(ix); torch.cuda.synchronize(); t2 = time.time() - t
        info = ctx.table_info()
        row = {"path": "device" if deferred else "host", "load_s": round(t1, 3), "upload_s": round(t2, 3), "total_s": round(t1 + t2, 3),
               **{k: round(v, 3) for k, v in info.items() if k.startswith("build_") and k != "build_rounds"}, "n_buckets": info["n_buckets"], "layout": info["table_layout"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del ix
if a.out:
    json.dump({"genes": a.genes, "threads": a.threads, "rows": rows}, open(a.out, "w"), indent=1)
