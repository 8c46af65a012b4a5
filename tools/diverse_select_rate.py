#!/usr/bin/env python3
"""Measured cost of the diverse selection (tools/grasp_score_rate.py's pattern: every GPU run is a child process under its own time
limit, the tool itself never opens the GPU; the first non-zero exit ends the measurement).

  kernels      ONE child process times `ops.segment_diverse` at ho3d's shape (O = 163 objects, M = P = 400, keep = 100), once over
               D = 61 parameters (rows resident in LDS) and once over D = 2334 vertex coordinates (rows streamed), against the same
               selection composed from torch ops on the same inputs, all objects batched: per step `torch.cdist` of the pick against
               the pool, `minimum`, `argmax` -- what a user would write without the kernel.  Device events around trains of calls,
               one untimed warm-up train each, then `--trains` timed trains per path, A B A B ...  The composed path rounds in
               another order, so its picks may differ where two gaps nearly tie: the share of equal picks is recorded, not required.
  entry point  the ho3d script at `--candidates 400 --num_grasp 100` with and without `--diverse_pool 400` (the same generation,
               scoring and ranking work, so the difference is the farthest-point selection): one untimed warm-up each, then
               without, with, without, with; the synchronised time of the generation calls from the closing `rank 0:` line.

    python tools/diverse_select_rate.py [--only kernels|entry] [--objects 163] [--out profiles/diverse_select_rate.json]
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
O, M, P, KEEP, SIZES = 163, 400, 400, 100, (61, 2334)


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
def kernels_child(trains, calls):
    sys.path.insert(0, ROOT)
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    pool = torch.stack([torch.randperm(M, generator=g)[:P] for _ in range(O)]).to(dev)
    rows = (pool + torch.arange(O, device=dev)[:, None] * M).reshape(-1)
    ar = torch.arange(O, device=dev)
    out = {"O": O, "M": M, "P": P, "keep": KEEP, "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0),
           "cases": {}}
    for D in SIZES:
        feat = torch.randn(O * M, D, generator=g).to(dev)

        def composed():
            x = feat.index_select(0, rows).view(O, P, D)                 # the pooled rows, gathered once
            pick = torch.zeros(O, dtype=torch.int64, device=dev)
            mind = torch.full((O, P), float("inf"), device=dev)
            picks = [pick]
            for _ in range(KEEP - 1):
                d = torch.cdist(x[ar, pick].unsqueeze(1), x).squeeze(1) ** 2
                mind = torch.minimum(mind, d)
                mind[ar, pick] = -1.0
                pick = torch.argmax(mind, dim=1)
                picks.append(pick)
            return pool.gather(1, torch.stack(picks, 1))

        paths = {"kernel": lambda: ops.segment_diverse(feat, pool, O, M, KEEP)[0], "composed": composed}

        def train(fn, n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(n):
                r = fn()
            b.record()
            b.synchronize()
            del r
            return a.elapsed_time(b) / n

        n_calls = {"kernel": calls, "composed": max(1, calls // 10)}      # ~600 launches per composed call
        k, c = paths["kernel"](), paths["composed"]()
        rec = {"lds_resident": bool(ops.segment_diverse_lds_resident(P, D)), "picks_equal_share": round(float((k == c).float().mean()), 4),
               "calls_per_train": n_calls, "ms_per_call": {name: [] for name in paths}}
        del k, c
        for name in paths:                                               # untimed warm-up train of each path
            train(paths[name], n_calls[name])
        for _ in range(trains):                                          # A B A B ...
            for name in paths:
                rec["ms_per_call"][name].append(round(train(paths[name], n_calls[name]), 4))
        ms = rec["ms_per_call"]
        best = {name: min(v) for name, v in ms.items()}
        # 3 FLOPs per feature and (step, pooled row) pair; the resident path reads every pooled row once, the streaming path once
        # per step (and once to validate them)
        flops = 3.0 * O * KEEP * P * D
        rec.update(best_ms=best, spread={name: spread(v) for name, v in ms.items()},
                   composed_over_kernel=round(best["composed"] / best["kernel"], 2), flops=flops,
                   kernel_bytes=O * P * D * 4 * (1 if rec["lds_resident"] else KEEP),
                   kernel_gflops=round(flops / (best["kernel"] * 1e-3) / 1e9, 1), us_per_step=round(best["kernel"] * 1e3 / KEEP, 2))
        out["cases"][str(D)] = rec
        print(f"[kernels] D={D}: kernel {best['kernel']:.3f} ms, composed {best['composed']:.3f} ms per {O} objects "
              f"(spread {rec['spread']}), equal picks {rec['picks_equal_share']}", file=sys.stderr, flush=True)
        del feat
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))
    return 0


# ------------------------------------------------------------------------------------------------ the entry point
def entry_run(mano_path, objects, flags, limit):
    out_dir = tempfile.mkdtemp(prefix="diverse_select_rate_")
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
    base = ["--num_grasp", str(KEEP), "--candidates", str(M)]
    cases = {"best_100_of_400": base, "diverse_100_of_400": base + ["--diverse_pool", str(P)]}
    rec = {"dataset": "ho3d", "objects": objects, "points": 3000, "rows_generated": M * objects, "flags": cases,
           "runs": {k: [] for k in cases}}
    for k, flags in cases.items():                                   # untimed warm-up of each
        entry_run(mano_path, objects, flags, limit)
    for _ in range(2):                                               # without, with, without, with
        for k, flags in cases.items():
            r = entry_run(mano_path, objects, flags, limit)
            print(f"[entry] {k}: {r['gen_s']} s in the generation calls", flush=True)
            rec["runs"][k].append(r)
    gen = {k: [r["gen_s"] for r in v] for k, v in rec["runs"].items()}
    rec["gen_s"] = gen
    rec["spread"] = {k: spread(v) for k, v in gen.items()}
    rec["diverse_share_of_generation"] = round((min(gen["diverse_100_of_400"]) - min(gen["best_100_of_400"])) / min(gen["best_100_of_400"]), 4)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["kernels", "entry"], default=None)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed train of the kernel (a tenth of it for the composed path)")
    ap.add_argument("--objects", type=int, default=O, help="objects of the entry-point runs (400 candidates each)")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diverse_select_rate.json"))
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="diverse_select_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc["what"] = ("tools/diverse_select_rate.py: ops.segment_diverse against the same selection composed from torch ops (alternating "
                   "trains, device events, one process), and the ho3d entry point at best-of-M with and without --diverse_pool (child "
                   "processes); one MI355X")
    rc = 0
    try:
        if args.only in (None, "kernels"):
            text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", "--trains", str(args.trains),
                          "--calls", str(args.calls)], args.limit)
            doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
            print(json.dumps({D: {k: c[k] for k in ("best_ms", "spread", "composed_over_kernel", "us_per_step")}
                              for D, c in doc["kernels"]["cases"].items()}))
        if args.only in (None, "entry"):
            doc["entry_point"] = entry_point(mano_path, args.objects, args.limit)
            print(json.dumps({k: doc["entry_point"][k] for k in ("gen_s", "spread", "diverse_share_of_generation")}))
    except RunFailed as e:
        print(f"diverse_select_rate: stopped at the first failing run: {e}", file=sys.stderr)
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
