#!/usr/bin/env python3
"""Measured cost of best-of-M grasp selection (tools/entry_point_rate.py's pattern: every GPU run is a child process under its own
time limit, the tool itself never opens the GPU; the first non-zero exit ends the measurement).

  kernels      ONE child process times, on identical inputs and alternating, the fused `contact.grasp_scores` against the composed
               `contact.grasp_proxies` (vertex normals + nearest neighbour + interior test + three torch reductions: the code of the
               commit before the fused kernel, unchanged since) at B = 16 384 grasps, V = 778, N in {1024, 3000}: device events
               around trains of calls, one untimed warm-up train each, then `--trains` timed trains per path, A B A B ...
               The hand is the MANO template of tests/golden/g9_mano_right.pkl.xz under a per-grasp offset, the cloud a
               channel-first [B,4,N] tensor read in place, as the generation path holds it.
  entry point  the ho3d script at `--candidates 400 --num_grasp 100` against plain `--num_grasp 400` (the same generation work,
               so the difference is scoring + selection): one untimed warm-up each, then plain, best-of, plain, best-of; the
               synchronised time of the generation calls from the closing `rank 0:` line.

    python tools/grasp_score_rate.py [--only kernels|entry] [--objects 128] [--out profiles/grasp_score_rate.json]
"""
import argparse
import json
import lzma
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g9_mano_right.pkl.xz")
GEN_LINE = re.compile(r"^rank 0: (\d+) grasps in ([0-9.]+) s")
B, V, SIZES = 16384, 778, (1024, 3000)


class RunFailed(RuntimeError):
    pass


def child(cmd, limit):
    try:
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        raise RunFailed(f"time limit of {limit} s: {' '.join(cmd)}\n{(e.stdout or '')[-2000:]}")
    if p.returncode != 0:
        raise RunFailed(f"exit status {p.returncode}: {' '.join(cmd)}\n{p.stdout[-2000:]}")
    return p.stdout


def spread(xs):
    return round((max(xs) - min(xs)) / max(xs), 4)


# ------------------------------------------------------------------------------------------------ the child of `kernels`
def kernels_child(mano_path, trains, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import contact, mano as dmano
    dev = torch.device("cuda", 0)
    arrays = dmano.read_mano_pkl(mano_path)
    topo = contact.HandTopology(arrays["faces"], V, dev)
    g = torch.Generator().manual_seed(5)
    template = torch.from_numpy(np.asarray(arrays["v_template"], np.float32))
    centre = template.mean(0)
    offset = torch.randn(B, 1, 3, generator=g) * 0.2
    hand = (template[None] + offset + torch.randn(B, V, 3, generator=g) * 0.001).to(dev).contiguous()
    out = {"B": B, "V": V, "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0), "cases": {}}
    for N in SIZES:
        cloud = torch.empty(B, 4, N)
        cloud[:, :3] = (centre[None, None] + offset + torch.randn(B, N, 3, generator=g) * 0.03).transpose(1, 2)   # around the hand
        cloud[:, 3] = 0.2
        cloud = cloud.to(dev)
        obj = cloud[:, :3].transpose(1, 2)
        paths = {"fused": lambda: contact.grasp_scores(topo, hand, obj), "composed": lambda: contact.grasp_proxies(topo, hand, obj)}

        def train(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                r = fn()
            b.record()
            b.synchronize()
            del r
            return a.elapsed_time(b) / calls

        f, c = paths["fused"](), paths["composed"]()
        same = bool(torch.equal(f["n_interior"].long(), c["n_interior"]) and torch.equal(f["n_contact"].long(), c["n_contact"])
                    and torch.allclose(f["penetration"], c["penetration"], rtol=1e-5, atol=0))
        rec = {"results_agree": same, "interior_share": round(float(c["n_interior"].float().mean()) / N, 4),
               "ms_per_call": {k: [] for k in paths}}
        del f, c
        for k in paths:                                              # untimed warm-up train of each path
            train(paths[k])
        for _ in range(trains):                                      # A B A B ...
            for k in paths:
                rec["ms_per_call"][k].append(round(train(paths[k]), 4))
        ms = rec["ms_per_call"]
        best = {k: min(v) for k, v in ms.items()}
        rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()},
                   composed_over_fused=round(best["composed"] / best["fused"], 3),
                   # per (point, vertex) pair 3 subtractions, 1 product, 2 fmas = 8 FLOPs; the fused kernel reads the hand and the
                   # cloud once and writes 12 B per grasp; the composed path also writes and re-reads the [B,N] intermediates
                   flops=8.0 * B * N * V, fused_bytes=B * ((V + N) * 12 + 12), composed_extra_bytes=13 * B * N,
                   fused_tflops=round(8.0 * B * N * V / (best["fused"] * 1e-3) / 1e12, 2))
        out["cases"][str(N)] = rec
        print(f"[kernels] N={N}: fused {best['fused']:.3f} ms, composed {best['composed']:.3f} ms per {B} grasps "
              f"(spread {rec['spread']}), agree={same}", file=sys.stderr, flush=True)
        del cloud, obj
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))
    return 0 if all(c["results_agree"] for c in out["cases"].values()) else 1


# ------------------------------------------------------------------------------------------------ the entry point
def entry_run(mano_path, objects, flags, limit):
    out_dir = tempfile.mkdtemp(prefix="grasp_score_rate_")
    cmd = [sys.executable, os.path.join(ROOT, "d-vqvae_amd", "gen_diverse_grasp_ho3d.py"), "--num_objects", str(objects), "--points", "3000",
           "--checkpoint", "/nonexistent", "--mano_model", mano_path, "--out_dir", out_dir] + flags
    t0 = time.time()
    try:
        text = child(cmd, limit)
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)
    for line in text.splitlines():
        m = GEN_LINE.match(line)
        if m:
            return {"grasps_kept": int(m.group(1)), "gen_s": float(m.group(2)), "process_s": round(time.time() - t0, 2)}
    raise RunFailed(f"no closing `rank 0:` line: {' '.join(cmd)}\n{text[-2000:]}")


def entry_point(mano_path, objects, limit):
    cases = {"plain_400": ["--num_grasp", "400"], "best_100_of_400": ["--num_grasp", "100", "--candidates", "400"]}
    rec = {"dataset": "ho3d", "objects": objects, "points": 3000, "rows_generated": 400 * objects, "flags": cases,
           "runs": {k: [] for k in cases}}
    for k, flags in cases.items():                                   # untimed warm-up of each
        entry_run(mano_path, objects, flags, limit)
    for _ in range(2):                                               # plain, best-of, plain, best-of
        for k, flags in cases.items():
            r = entry_run(mano_path, objects, flags, limit)
            print(f"[entry] {k}: {r['gen_s']} s in the generation calls", flush=True)
            rec["runs"][k].append(r)
    gen = {k: [r["gen_s"] for r in v] for k, v in rec["runs"].items()}
    rec["gen_s"] = gen
    rec["spread"] = {k: spread(v) for k, v in gen.items()}
    rec["selection_share_of_generation"] = round((min(gen["best_100_of_400"]) - min(gen["plain_400"])) / min(gen["plain_400"]), 4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["kernels", "entry"], default=None)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed train")
    ap.add_argument("--objects", type=int, default=128, help="objects of the entry-point runs (400 rows each)")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grasp_score_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="grasp_score_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["what"] = ("tools/grasp_score_rate.py: fused contact.grasp_scores against the composed contact.grasp_proxies (alternating trains, "
                   "device events, one process), and the ho3d entry point with and without best-of-M selection (child processes); one MI355X")
    rc = 0
    try:
        if args.only in (None, "kernels"):
            text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", mano_path, "--trains", str(args.trains),
                          "--calls", str(args.calls)], args.limit)
            doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
            print(json.dumps({N: {k: c[k] for k in ("best_ms", "spread", "composed_over_fused")} for N, c in doc["kernels"]["cases"].items()}))
        if args.only in (None, "entry"):
            doc["entry_point"] = entry_point(mano_path, args.objects, args.limit)
            print(json.dumps({k: doc["entry_point"][k] for k in ("gen_s", "spread", "selection_share_of_generation")}))
    except RunFailed as e:
        print(f"grasp_score_rate: stopped at the first failing run: {e}", file=sys.stderr)
        doc["stopped"] = str(e)[:600]
        rc = 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
