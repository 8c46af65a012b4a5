#!/usr/bin/env python3
"""Measured rates of the gen_diverse_grasp_* entry points: this tree against a checkout of its parent commit.

Every run is a fresh child process (`python <root>/d-vqvae_amd/gen_diverse_grasp_<dataset>.py ...`) under its own time limit;
the tool itself never opens the GPU.  It uses the command line and the closing lines of a run only,

    rank 0: G grasps in T s (... grasps/s incl. first-call packing)      <- synchronised time of the generation calls
    rank 0: wall time W s incl. JSON writing (...)                       <- absent before --rows_per_call existed: recorded as null

so it runs unchanged against an older tree (`git archive <parent> | tar -x -C <dir>`, built there).  Per case: one untimed
warm-up run of each tree, then baseline, branch, baseline, branch; then the branch once with twice the objects, which separates
the fixed part of a run (first-call weight packing, allocator growth) from its rate: marginal = G / (T(2G) - T(G)).
The first non-zero exit ends the measurement.  Synthetic weights and objects (--checkpoint / --mano_model name no file).

    python tools/entry_point_rate.py --baseline-root <parent checkout> [--cases obman1024 ho3d ...] [--out profiles/entry_point_rate.json]

`--trace CASE` instead runs that case once per tree under `rocprofv3 --kernel-trace --stats` (a run of its own, no timing
taken from it) and records calls / total / average of the cloud-transform kernels with their algorithmic bytes per second."""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRASPS = {"obman": 1, "ho3d": 100, "grab": 20, "FHAB": 49}
CASES = {                         # name -> (dataset, objects, points, seconds allowed per run)
    "obman1024": ("obman", 16384, 1024, 600),
    "obman3000": ("obman", 16384, 3000, 600),
    "ho3d": ("ho3d", 512, 3000, 300),
    "grab": ("grab", 512, 3000, 300),
    "FHAB": ("FHAB", 512, 3000, 300),
}
GEN_LINE = re.compile(r"^rank 0: (\d+) grasps in ([0-9.]+) s \(([0-9.]+) grasps/s")
WALL_LINE = re.compile(r"^rank 0: wall time ([0-9.]+) s")


class RunFailed(RuntimeError):
    pass


def command(root, dataset, objects, points, out_dir):
    return [sys.executable, os.path.join(root, "d-vqvae_amd", f"gen_diverse_grasp_{dataset}.py"), "--num_objects", str(objects),
            "--points", str(points), "--checkpoint", "/nonexistent", "--mano_model", "/nonexistent", "--out_dir", out_dir]


def run_once(root, dataset, objects, points, limit, prefix=()):
    """One child process; returns the parsed closing lines.  The JSON files go to a scratch directory that is removed."""
    out_dir = tempfile.mkdtemp(prefix="entry_point_rate_")
    cmd = list(prefix) + command(root, dataset, objects, points, out_dir)
    t0 = time.time()
    try:
        p = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        raise RunFailed(f"time limit of {limit} s: {' '.join(cmd)}\n{(e.stdout or '')[-2000:]}")
    finally:
        files = len(glob.glob(os.path.join(out_dir, "*.json")))
        shutil.rmtree(out_dir, ignore_errors=True)
    if p.returncode != 0:
        raise RunFailed(f"exit status {p.returncode}: {' '.join(cmd)}\n{p.stdout[-2000:]}")
    rec = {"process_s": round(time.time() - t0, 3), "files": files, "grasps": None, "gen_s": None, "gen_grasps_per_s": None,
           "wall_s": None, "wall_grasps_per_s": None, "calls": sum(1 for l in p.stdout.splitlines() if l.startswith("gen_time:"))}
    for line in p.stdout.splitlines():
        m = GEN_LINE.match(line)
        if m:
            rec.update(grasps=int(m.group(1)), gen_s=float(m.group(2)), gen_grasps_per_s=float(m.group(3)))
        m = WALL_LINE.match(line)
        if m:
            rec["wall_s"] = float(m.group(1))
    if rec["grasps"] is None:
        raise RunFailed(f"no closing `rank 0:` line: {' '.join(cmd)}\n{p.stdout[-2000:]}")
    if rec["wall_s"]:
        rec["wall_grasps_per_s"] = round(rec["grasps"] / rec["wall_s"], 1)
    return rec


def spread(a, b):
    return None if a is None or b is None else round(abs(a - b) / max(a, b), 4)


def measure(name, roots, warmup_objects):
    dataset, objects, points, limit = CASES[name]
    rec = {"dataset": dataset, "objects": objects, "points": points, "grasps_per_object": GRASPS[dataset], "runs": {k: [] for k in roots}}
    for k, root in roots.items():                                   # untimed warm-up of each tree
        w = run_once(root, dataset, min(objects, warmup_objects) if warmup_objects else objects, points, limit)
        rec.setdefault("warmup", {})[k] = {"objects": w["grasps"] // GRASPS[dataset], "process_s": w["process_s"]}
    for _ in range(2):                                              # baseline, branch, baseline, branch
        for k, root in roots.items():
            r = run_once(root, dataset, objects, points, limit)
            print(f"[{name}] {k}: {r['gen_grasps_per_s']} grasps/s in the generation calls, wall {r['wall_grasps_per_s']}", flush=True)
            rec["runs"][k].append(r)
    for k, runs in rec["runs"].items():
        rec[k] = {"gen_grasps_per_s": [r["gen_grasps_per_s"] for r in runs], "wall_grasps_per_s": [r["wall_grasps_per_s"] for r in runs],
                  "gen_spread": spread(runs[0]["gen_grasps_per_s"], runs[1]["gen_grasps_per_s"]),
                  "wall_spread": spread(runs[0]["wall_grasps_per_s"], runs[1]["wall_grasps_per_s"])}
    if "branch" in roots:                                           # twice the objects: the fixed part of a run against its rate
        d = run_once(roots["branch"], dataset, 2 * objects, points, 2 * limit)
        one = min(r["gen_s"] for r in rec["runs"]["branch"])
        rec["branch_twice_the_objects"] = d
        if d["gen_s"] > one:
            rec["branch"]["marginal_gen_grasps_per_s"] = round((d["grasps"] - rec["runs"]["branch"][0]["grasps"]) / (d["gen_s"] - one), 1)
            rec["branch"]["fixed_share_of_gen_s"] = round(max(0.0, 1.0 - (d["gen_s"] - one) / one), 4)
        if "baseline" in roots:
            rec["speedup_gen"] = round(max(rec["branch"]["gen_grasps_per_s"]) / max(rec["baseline"]["gen_grasps_per_s"]), 2)
    return rec


def trace(name, roots):
    """One run per tree under rocprofv3 --kernel-trace --stats; the cloud-transform kernels' rows of the statistics."""
    dataset, objects, points, limit = CASES[name]
    G, C = GRASPS[dataset], 4
    rec = {"dataset": dataset, "objects": objects, "points": points, "command": "rocprofv3 --kernel-trace --stats -- <entry point>"}
    for k, root in roots.items():
        d = tempfile.mkdtemp(prefix="entry_point_trace_")
        try:
            r = run_once(root, dataset, objects, points, 2 * limit,
                         prefix=["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "t", "--output-format", "csv", "--"])
            rows = []
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                rows += list(csv.DictReader(open(path)))
        finally:
            shutil.rmtree(d, ignore_errors=True)
        total = sum(float(x["TotalDurationNs"]) for x in rows)
        out = {"gen_s_under_the_profiler": r["gen_s"], "kernel_time_ms": round(total / 1e6, 3), "calls_of_gen": r["calls"],
               "top": [{"name": x["Name"][:100], "calls": int(x["Calls"]), "total_ms": round(float(x["TotalDurationNs"]) / 1e6, 3)}
                       for x in sorted(rows, key=lambda x: -float(x["TotalDurationNs"]))[:12]]}
        for x in rows:
            if "transform_cloud" in x["Name"]:
                calls, tot = int(x["Calls"]), float(x["TotalDurationNs"])
                written = objects * G * C * points * 4                           # every row of every call, once
                read = objects * C * points * 4                                  # every object's cloud, once (re-reads stay in L2)
                out["transform"] = {"kernel": x["Name"][:100], "calls": calls, "total_ms": round(tot / 1e6, 3),
                                    "average_us": round(tot / calls / 1e3, 2), "algorithmic_bytes": written + read,
                                    "bytes_per_s": round((written + read) / (tot * 1e-9), 1)}
        rec[k] = out
        print(f"[trace {name}] {k}: {json.dumps(out.get('transform'))}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--branch-root", default=ROOT)
    ap.add_argument("--baseline-root", default=None, help="a built checkout of the parent commit (per-object loop)")
    ap.add_argument("--cases", nargs="*", default=list(CASES), choices=list(CASES))
    ap.add_argument("--warmup-objects", type=int, default=0, help="objects of the untimed warm-up runs (0 = the case's own count)")
    ap.add_argument("--trace", default=None, choices=list(CASES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entry_point_rate.json"))
    args = ap.parse_args()
    roots = {}
    if args.baseline_root:
        roots["baseline"] = os.path.abspath(args.baseline_root)
    roots["branch"] = os.path.abspath(args.branch_root)
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc.setdefault("what", "tools/entry_point_rate.py: entry-point scripts as child processes, synthetic weights and objects, one MI355X; "
                           "baseline = the parent commit's per-object loop, branch = grouped calls (--rows_per_call 16384)")
    rc = 0
    try:
        if args.trace:
            doc.setdefault("trace", {})[args.trace] = trace(args.trace, roots)
        else:
            for name in args.cases:
                doc.setdefault("cases", {})[name] = measure(name, roots, args.warmup_objects)
                with open(args.out, "w") as f:                     # after every case: a later failure keeps the earlier ones
                    json.dump(doc, f, indent=1)
    except RunFailed as e:
        print(f"entry_point_rate: stopped at the first failing run: {e}", file=sys.stderr)
        doc["stopped"] = str(e)[:600]
        rc = 1
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
