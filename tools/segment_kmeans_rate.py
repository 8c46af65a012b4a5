#!/usr/bin/env python3
"""Measured cost of the device k-means behind the diversity statistic (tools/diverse_select_rate.py's pattern: the GPU run is a child
process under its own time limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

ONE child process times one launch of `ops.segment_kmeans` with k = 20, D = 61, iters = 100 at three shapes -- O = 1, M = 65 536 (the
paper-style check of a whole bench batch); O = 1, M = 1200; O = 164, M = 100 (ho3d: one segment per object) -- from evenly spaced
starting rows: device events around trains of calls, one untimed warm-up train, then `--trains` timed trains; the best train counts.
The parent then times the reference's own path on the same rows and the same starting rows on this machine's CPUs:
`scipy.cluster.vq.kmeans(x, guess)` + `vq` in float64, one segment after the other (ONE start, as the kernel; the paper protocol of 20
random starts costs twenty times that).  scipy stops on a distortion threshold, the kernel when no assignment changes or at the limit,
so the iteration counts differ: both are recorded.

    python tools/segment_kmeans_rate.py [--trains 5] [--limit 300] [--out profiles/segment_kmeans_rate.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, D, ITERS = 20, 61, 100
SHAPES = ((1, 65536), (1, 1200), (164, 100))
CALLS = {65536: 2, 1200: 20, 100: 20}                  # calls per timed train


def rows_of(O, M):
    """The rows of a shape: Gaussian noise around 40 centres, so that Lloyd has something to find; the same in child and parent."""
    rng = np.random.default_rng([O, M])
    blobs = rng.standard_normal((40, D)).astype(np.float32)
    return (rng.standard_normal((O * M, D)).astype(np.float32) * np.float32(0.5) + blobs[rng.integers(0, 40, O * M)]).astype(np.float32)


def spaced(M):
    return np.asarray([j * M // K for j in range(K)], dtype=np.int64)


def child(trains):
    sys.path.insert(0, ROOT)
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import diversity, ops
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "k": K, "D": D, "iters": ITERS, "trains": trains, "cases": {}}
    for O, M in SHAPES:
        feat = torch.from_numpy(rows_of(O, M)).to(dev)
        init = diversity.kmeans_init(O, M, K, "spaced", device=dev)
        n = CALLS[M]

        def train():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                r = ops.segment_kmeans(feat, init, O, M, ITERS)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / n, r

        _, r = train()                                                   # untimed warm-up train
        ms = [round(train()[0], 4) for _ in range(trains)]
        used = r[4].cpu().numpy()
        stat = diversity.device_diversity(feat, O, M, cls_num=K, iters=ITERS)
        out["cases"][f"{O}x{M}"] = {"O": O, "M": M, "calls_per_train": n, "ms_per_call": ms, "best_ms": min(ms),
                                    "spread": round((max(ms) - min(ms)) / max(ms), 4), "iters_used_min": int(used.min()),
                                    "iters_used_max": int(used.max()), "entropy_first_segment": stat[0]["entropy"],
                                    "mean_dist_first_segment": stat[0]["mean_dist"]}
        print(f"[kernel] O={O} M={M}: {min(ms):.3f} ms per launch, {int(used.min())}-{int(used.max())} iterations", file=sys.stderr, flush=True)
        del feat, r
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))
    return 0


def scipy_path(O, M):
    import scipy.cluster.vq
    from scipy.stats import entropy
    x = rows_of(O, M).astype(np.float64)
    guess = spaced(M)
    t0 = time.perf_counter()
    first = None
    for o in range(O):
        seg = x[o * M:(o + 1) * M]
        codes, _ = scipy.cluster.vq.kmeans(seg, seg[guess])
        labels, dist = scipy.cluster.vq.vq(seg, codes)
        if first is None:
            first = (float(entropy(np.histogram(labels, len(codes))[0])), float(dist.mean()))
    return {"seconds": round(time.perf_counter() - t0, 4), "entropy_first_segment": first[0], "mean_dist_first_segment": first[1]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_kmeans_rate.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.trains)
    doc = {"what": "tools/segment_kmeans_rate.py: one launch of ops.segment_kmeans (k = 20, D = 61, iters = 100, device events, best of the "
                   "timed trains) against scipy.cluster.vq.kmeans(x, guess) + vq from the same starting rows on the host's CPUs; one MI355X"}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--trains", str(args.trains)]
    rc = 0
    try:
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.limit)
        if p.returncode != 0:
            raise RuntimeError(f"exit status {p.returncode}\n{p.stdout[-2000:]}")
        doc["kernel"] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        doc["cpus"] = len(os.sched_getaffinity(0))
        doc["scipy"] = {}
        for O, M in SHAPES:
            doc["scipy"][f"{O}x{M}"] = s = scipy_path(O, M)
            ms = doc["kernel"]["cases"][f"{O}x{M}"]["best_ms"]
            s["scipy_over_kernel"] = round(s["seconds"] * 1e3 / ms, 1)
            print(f"O={O} M={M}: kernel {ms:.3f} ms, scipy {s['seconds'] * 1e3:.1f} ms ({s['scipy_over_kernel']} x)", flush=True)
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        print(f"segment_kmeans_rate: stopped: {e}", file=sys.stderr)
        doc["stopped"] = str(e)[:600]
        rc = 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
