#!/usr/bin/env python3
"""Measured cost of hand-side contact (tools/grasp_wrench_rate.py's pattern: the GPU run is a child process under its own time
limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

  ONE child process times, on identical inputs and alternating, `contact.grasp_parts` (dvq_grasp_parts: every hand vertex against
  the cloud, the per-part minima and counts and the mask; the per-vertex outputs are not asked for, as on the generation path)
  against `contact.grasp_scores` (dvq_grasp_scores: every cloud point against the hand -- the yardstick: the same pairs, the roles
  swapped) at B = 16 384 grasps, V = 778, N in {1024, 3000}: device events around trains of calls, one untimed warm-up train each,
  then `--trains` timed trains per path, A B A B ...  The hand is the MANO template of tests/golden/g9_mano_right.pkl.xz under a
  per-grasp offset, the cloud a channel-first [B,4,N] tensor read in place, as the generation path holds it.  The parts kernel
  scans 1024 vertex slots (four per thread) for 778 vertices: 1.32 x the pairs of the scores kernel.  The mean number of fingers
  in contact at the default 5 mm is reported, and the kernel's per-vertex outputs are checked against ops.nn_points once.

    python tools/grasp_parts_rate.py [--trains 5] [--calls 20] [--out profiles/grasp_parts_rate.json]
"""
import argparse
import json
import lzma
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "g9_mano_right.pkl.xz")
B, V, SIZES = 16384, 778, (1024, 3000)
SLOTS = 1024                     # vertex slots of a pass of the parts kernel: 256 threads x 4


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


def kernels_child(mano_path, trains, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import contact, mano as dmano, ops
    dev = torch.device("cuda", 0)
    arrays = dmano.read_mano_pkl(mano_path)
    topo = contact.HandTopology(arrays["faces"], V, dev)
    parts = contact.HandParts.from_json(device=dev)
    g = torch.Generator().manual_seed(5)
    template = torch.from_numpy(np.asarray(arrays["v_template"], np.float32))
    centre = template.mean(0)
    offset = torch.randn(B, 1, 3, generator=g) * 0.2
    hand = (template[None] + offset + torch.randn(B, V, 3, generator=g) * 0.001).to(dev).contiguous()
    out = {"B": B, "V": V, "tile": ops.GRASP_PARTS_TILE, "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0), "cases": {}}
    for N in SIZES:
        cloud = torch.empty(B, 4, N)
        cloud[:, :3] = (centre[None, None] + offset + torch.randn(B, N, 3, generator=g) * 0.03).transpose(1, 2)   # around the hand
        cloud[:, 3] = 0.2
        cloud = cloud.to(dev)
        obj = cloud[:, :3].transpose(1, 2)
        paths = {"parts": lambda: contact.grasp_parts(parts, hand, obj), "scores": lambda: contact.grasp_scores(topo, hand, obj)}

        def train(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                r = fn()
            b.record()
            b.synchronize()
            del r
            return a.elapsed_time(b) / calls

        rows = slice(0, 256)                                         # the per-vertex outputs against nn_points, on a slice of the rows
        w = contact.grasp_parts(parts, hand[rows], obj[rows], want_verts=True)
        d, idx = ops.nn_points(hand[rows], obj[rows])
        same = bool(torch.equal(w["vert_dist"].view(torch.int32), d.view(torch.int32)) and torch.equal(w["vert_idx"].long(), idx))
        w = paths["parts"]()
        fingers = (w["part_count"][:, :5] >= 1).sum(dim=1).float()
        rec = {"nn_points_agree": same, "mean_fingers_in_contact": round(float(fingers.mean()), 4),
               "rows_with_a_figure": round(float((w["status"] == 0).float().mean()), 4), "ms_per_call": {k: [] for k in paths}}
        del w, d, idx, fingers
        for k in paths:                                              # untimed warm-up train of each path
            train(paths[k])
        for _ in range(trains):                                      # A B A B ...
            for k in paths:
                rec["ms_per_call"][k].append(round(train(paths[k]), 4))
        ms = rec["ms_per_call"]
        best = {k: min(v) for k, v in ms.items()}
        rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()}, parts_over_scores=round(best["parts"] / best["scores"], 3),
                   # the scan's 8 FLOPs per pair: the scores kernel does N x V of them, the parts kernel N x 1024 vertex slots
                   scores_flops=8.0 * B * N * V, parts_flops=8.0 * B * N * SLOTS, pair_ratio=round(SLOTS / V, 3),
                   parts_tflops=round(8.0 * B * N * SLOTS / (best["parts"] * 1e-3) / 1e12, 2),
                   scores_tflops=round(8.0 * B * N * V / (best["scores"] * 1e-3) / 1e12, 2))
        out["cases"][str(N)] = rec
        print(f"[kernels] N={N}: parts {best['parts']:.3f} ms, scores {best['scores']:.3f} ms per {B} grasps "
              f"(spread {rec['spread']}), fingers {rec['mean_fingers_in_contact']}, agree={same}", file=sys.stderr, flush=True)
        del cloud, obj
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))
    return 0 if all(c["nn_points_agree"] for c in out["cases"].values()) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed train")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grasp_parts_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="grasp_parts_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": "tools/grasp_parts_rate.py: contact.grasp_parts (dvq_grasp_parts) against contact.grasp_scores (dvq_grasp_scores) "
                   "on identical inputs (alternating trains, device events, one process); one MI355X"}
    rc = 0
    try:
        text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", mano_path, "--trains", str(args.trains),
                      "--calls", str(args.calls)], args.limit)
        doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({N: {k: c[k] for k in ("best_ms", "spread", "parts_over_scores", "mean_fingers_in_contact")}
                          for N, c in doc["kernels"]["cases"].items()}))
    except RunFailed as e:
        print(f"grasp_parts_rate: stopped at the failing run: {e}", file=sys.stderr)
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
