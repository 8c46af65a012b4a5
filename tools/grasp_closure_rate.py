#!/usr/bin/env python3
"""Measured cost of the force-closure quality with friction (tools/grasp_wrench_rate.py's pattern: the GPU run is a child process
under its own time limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

  ONE child process times, on identical inputs and alternating, `contact.grasp_closure` (dvq_grasp_closure) at D = 64, 256 and 1024
  sampled directions against `contact.grasp_stability` (dvq_grasp_wrench: the frictionless proxy it stands beside, the same scan and
  the same centre pass -- the baseline) at B = 16 384 grasps, V = 778, N in {1024, 3000}: device events around trains of calls, one
  untimed warm-up train each, then `--trains` timed trains per path, A B C D A B C D ...  The hand is the MANO template of
  tests/golden/g9_mano_right.pkl.xz under a per-grasp offset, the cloud a channel-first [B,4,N] tensor read in place, as the
  generation path holds it.  The share of points in contact is reported: the work per direction is done for those only, about 30
  FLOPs per (contact, direction).

    python tools/grasp_closure_rate.py [--trains 5] [--calls 10] [--out profiles/grasp_closure_rate.json]
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
B, V, SIZES, DIRS, MU = 16384, 778, (1024, 3000), (64, 256, 1024), 0.5


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
    from dvqvae_amd import contact, mano as dmano
    dev = torch.device("cuda", 0)
    arrays = dmano.read_mano_pkl(mano_path)
    topo = contact.HandTopology(arrays["faces"], V, dev)
    g = torch.Generator().manual_seed(5)
    template = torch.from_numpy(np.asarray(arrays["v_template"], np.float32))
    centre = template.mean(0)
    offset = torch.randn(B, 1, 3, generator=g) * 0.2
    hand = (template[None] + offset + torch.randn(B, V, 3, generator=g) * 0.001).to(dev).contiguous()
    out = {"B": B, "V": V, "friction": MU, "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0), "cases": {}}
    for N in SIZES:
        cloud = torch.empty(B, 4, N)
        cloud[:, :3] = (centre[None, None] + offset + torch.randn(B, N, 3, generator=g) * 0.03).transpose(1, 2)   # around the hand
        cloud[:, 3] = 0.2
        cloud = cloud.to(dev)
        obj = cloud[:, :3].transpose(1, 2)
        paths = {"wrench": lambda: contact.grasp_stability(topo, hand, obj)}
        for D in DIRS:
            paths[f"closure{D}"] = lambda D=D: contact.grasp_closure(topo, hand, obj, friction=MU, dirs=D)

        def train(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                r = fn()
            b.record()
            b.synchronize()
            del r
            return a.elapsed_time(b) / calls

        w, c = paths["wrench"](), paths[f"closure{DIRS[-1]}"]()
        # the count and the centre the two kernels share, bit for bit
        same = bool(torch.equal(w["n_contact"], c["n_contact"])) and bool(torch.equal(w["centre"].view(torch.int32), c["centre"].view(torch.int32)))
        n_ct = float(c["n_contact"].float().mean())
        rec = {"shared_outputs_agree": same, "contact_share": round(n_ct / N, 4), "mean_contacts": round(n_ct, 1),
               "status0_share": round(float((c["status"] == 0).float().mean()), 4),
               "share_not_refuted": round(float((c["quality"] > 0).float().mean()), 4), "ms_per_call": {k: [] for k in paths}}
        del w, c
        for k in paths:                                              # untimed warm-up train of each path
            train(paths[k])
        for _ in range(trains):                                      # A B C D A B C D ...
            for k in paths:
                rec["ms_per_call"][k].append(round(train(paths[k]), 4))
        ms = rec["ms_per_call"]
        best = {k: min(v) for k, v in ms.items()}
        rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()},
                   closure_over_wrench={k: round(best[k] / best["wrench"], 3) for k in best if k != "wrench"},
                   # the scan's 8 FLOPs per (point, vertex) pair, which every path does, and what the directions add: about 30 FLOPs
                   # per (contact, direction), with the measured mean contact count
                   scan_flops=8.0 * B * N * V, direction_flops={str(D): 30.0 * B * n_ct * D for D in DIRS},
                   closure_tflops={str(D): round((8.0 * B * N * V + 30.0 * B * n_ct * D) / (best[f"closure{D}"] * 1e-3) / 1e12, 2) for D in DIRS},
                   wrench_tflops=round(8.0 * B * N * V / (best["wrench"] * 1e-3) / 1e12, 2))
        out["cases"][str(N)] = rec
        print(f"[kernels] N={N}: " + ", ".join(f"{k} {v:.3f} ms" for k, v in best.items()) + f" per {B} grasps (spread {rec['spread']}), "
              f"contact share {rec['contact_share']}, agree={same}", file=sys.stderr, flush=True)
        del cloud, obj
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))
    return 0 if all(c["shared_outputs_agree"] for c in out["cases"].values()) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed train")
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grasp_closure_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="grasp_closure_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": "tools/grasp_closure_rate.py: contact.grasp_closure (dvq_grasp_closure) at 64 / 256 / 1024 directions against "
                   "contact.grasp_stability (dvq_grasp_wrench) on identical inputs (alternating trains, device events, one process); one MI355X"}
    rc = 0
    try:
        text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", mano_path, "--trains", str(args.trains),
                      "--calls", str(args.calls)], args.limit)
        doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({N: {k: c[k] for k in ("best_ms", "spread", "closure_over_wrench", "contact_share")}
                          for N, c in doc["kernels"]["cases"].items()}))
    except RunFailed as e:
        print(f"grasp_closure_rate: stopped at the failing run: {e}", file=sys.stderr)
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
