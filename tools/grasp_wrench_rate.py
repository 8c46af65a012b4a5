#!/usr/bin/env python3
"""Measured cost of the grasp stability proxy (tools/grasp_score_rate.py's pattern: the GPU run is a child process under its own
time limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

  ONE child process times, on identical inputs and alternating, `contact.grasp_stability` (dvq_grasp_wrench: the three scores, the
  centre, the 27 contact-wrench sums and the key) against `contact.grasp_scores` (dvq_grasp_scores: the three scores, the kernel the
  selection path launches without the stability flags -- the baseline) at B = 16 384 grasps, V = 778, N in {1024, 3000}: device
  events around trains of calls, one untimed warm-up train each, then `--trains` timed trains per path, A B A B ...  The hand is the
  MANO template of tests/golden/g9_mano_right.pkl.xz under a per-grasp offset, the cloud a channel-first [B,4,N] tensor read in
  place, as the generation path holds it.  The share of points in contact is reported: the wrench work is done for those only.

    python tools/grasp_wrench_rate.py [--trains 5] [--calls 20] [--out profiles/grasp_wrench_rate.json]
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
    out = {"B": B, "V": V, "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0), "cases": {}}
    for N in SIZES:
        cloud = torch.empty(B, 4, N)
        cloud[:, :3] = (centre[None, None] + offset + torch.randn(B, N, 3, generator=g) * 0.03).transpose(1, 2)   # around the hand
        cloud[:, 3] = 0.2
        cloud = cloud.to(dev)
        obj = cloud[:, :3].transpose(1, 2)
        paths = {"wrench": lambda: contact.grasp_stability(topo, hand, obj), "scores": lambda: contact.grasp_scores(topo, hand, obj)}

        def train(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                r = fn()
            b.record()
            b.synchronize()
            del r
            return a.elapsed_time(b) / calls

        w, s = paths["wrench"](), paths["scores"]()
        same = all(bool(torch.equal(w[k].view(torch.int32), s[k].view(torch.int32))) for k in s)       # the three scores, bit for bit
        rec = {"scores_agree": same, "contact_share": round(float(s["n_contact"].float().mean()) / N, 4),
               "finite_keys": round(float(torch.isfinite(w["key"]).float().mean()), 4), "ms_per_call": {k: [] for k in paths}}
        del w, s
        for k in paths:                                              # untimed warm-up train of each path
            train(paths[k])
        for _ in range(trains):                                      # A B A B ...
            for k in paths:
                rec["ms_per_call"][k].append(round(train(paths[k]), 4))
        ms = rec["ms_per_call"]
        best = {k: min(v) for k, v in ms.items()}
        rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()}, wrench_over_scores=round(best["wrench"] / best["scores"], 3),
                   # the scan's 8 FLOPs per (point, vertex) pair, which both kernels do; the wrench kernel reads the cloud twice and
                   # writes 136 B per grasp instead of 12
                   flops=8.0 * B * N * V, scores_bytes=B * ((V + N) * 12 + 12), wrench_bytes=B * ((V + 2 * N) * 12 + 136),
                   wrench_tflops=round(8.0 * B * N * V / (best["wrench"] * 1e-3) / 1e12, 2),
                   scores_tflops=round(8.0 * B * N * V / (best["scores"] * 1e-3) / 1e12, 2))
        out["cases"][str(N)] = rec
        print(f"[kernels] N={N}: wrench {best['wrench']:.3f} ms, scores {best['scores']:.3f} ms per {B} grasps "
              f"(spread {rec['spread']}), contact share {rec['contact_share']}, agree={same}", file=sys.stderr, flush=True)
        del cloud, obj
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))
    return 0 if all(c["scores_agree"] for c in out["cases"].values()) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed train")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grasp_wrench_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="grasp_wrench_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": "tools/grasp_wrench_rate.py: contact.grasp_stability (dvq_grasp_wrench) against contact.grasp_scores (dvq_grasp_scores) "
                   "on identical inputs (alternating trains, device events, one process); one MI355X"}
    rc = 0
    try:
        text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", mano_path, "--trains", str(args.trains),
                      "--calls", str(args.calls)], args.limit)
        doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({N: {k: c[k] for k in ("best_ms", "spread", "wrench_over_scores", "contact_share")}
                          for N, c in doc["kernels"]["cases"].items()}))
    except RunFailed as e:
        print(f"grasp_wrench_rate: stopped at the failing run: {e}", file=sys.stderr)
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
