#!/usr/bin/env python3
"""Measured cost of the test-time-loss kernel and of one step of the gradient refinement (tools/grasp_self_rate.py's pattern: every
GPU step is a child process under its own time limit, the tool itself never opens the GPU; the steps are chained, and a non-zero
exit ends the measurement).

  One child per cloud size (N = 1024 and N = 3000): 16 384 hands of the real hand model (tests/golden/g9_mano_right.pkl.xz posed on
  the device) against clouds of N points around them, channel-first and read in place.  Timed, alternating, in ONE process:
    scores   contact.grasp_scores            (dvq_grasp_scores: the yardstick, the same scan without the second minimum)
    forward  contact.ttt_terms, grad off     (dvq_grasp_ttt, the scan phase and the reductions)
    grad     contact.ttt_value_and_grad      (dvq_grasp_ttt with the gather phase: the loss and its gradient at the vertices)
    step     one step of contact.refine_ttt  (MANO forward, grad, dvq_mano_backward, the SGD update, keep_best bookkeeping):
             (refine_ttt(steps = S) - refine_ttt(steps = 0)) / S
  Device events around trains of calls, one untimed warm-up train each, then `--trains` timed trains per path, A B C D A B C D ...

    python tools/grasp_ttt_rate.py [--trains 5] [--calls 10] [--out profiles/grasp_ttt_rate.json]
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
B, V = 16384, 778
SIZES = (1024, 3000)
STEPS = 4                        # of the timed refine_ttt call


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


def kernels_child(mano_path, N, trains, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import contact, mano as dmano
    dev = torch.device("cuda", 0)
    layer = dmano.load(model_path=mano_path, model_type="mano", use_pca=True, num_pca_comps=45, flat_hand_mean=True).to(dev)
    topo = contact.HandTopology(np.asarray(layer.faces), V, dev)
    g = torch.Generator().manual_seed(6)
    params = torch.cat([torch.randn(B, 10, generator=g), torch.randn(B, 3, generator=g), torch.randn(B, 45, generator=g) * 0.3,
                        torch.randn(B, 3, generator=g) * 0.2], dim=1).to(dev)
    with torch.no_grad():
        hands = layer(betas=params[:, :10], global_orient=params[:, 10:13], hand_pose=params[:, 13:58], transl=params[:, 58:61]).vertices.contiguous()
    g = torch.Generator().manual_seed(7)
    cloud = torch.empty(B, 4, N, device=dev)
    for lo in range(0, B, 2048):                                     # in slabs: the host copy of 16 384 x 3000 points is 750 MB
        cloud[lo:lo + 2048, :3] = (torch.randn(2048, N, 3, generator=g) * 0.03).transpose(1, 2).to(dev)
    cloud[:, 3] = 0.2
    cloud[:, :3] += hands.mean(dim=1)[:, :, None]                    # around the hand
    obj = cloud[:, :3].transpose(1, 2)                               # channel-first, read in place, as the generation path holds it

    def forward():
        with torch.no_grad():
            return contact.ttt_terms(topo, hands, obj)

    paths = {"scores": lambda: contact.grasp_scores(topo, hands, obj), "forward": forward,
             "grad": lambda: contact.ttt_value_and_grad(topo, hands, obj),
             "refine0": lambda: contact.refine_ttt(layer, topo, params, obj, 0),
             "refineS": lambda: contact.refine_ttt(layer, topo, params, obj, STEPS)}

    def train(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            r = fn()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b) / n

    n_of = {k: (max(1, calls // STEPS) if k == "refineS" else calls) for k in paths}
    rec = {"B": B, "V": V, "N": N, "trains": trains, "calls_per_train": n_of, "refine_steps": STEPS, "device": torch.cuda.get_device_name(0),
           "ms_per_call": {k: [] for k in paths}}
    for k in paths:                                                  # untimed warm-up train of each path
        train(paths[k], 2)
    for _ in range(trains):
        for k in paths:
            rec["ms_per_call"][k].append(round(train(paths[k], n_of[k]), 4))
    ms = rec["ms_per_call"]
    best = {k: min(v) for k, v in ms.items()}
    best["step"] = round((best["refineS"] - best["refine0"]) / STEPS, 4)
    out = contact.ttt_terms(topo, hands, obj)
    rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()},
               over_scores={k: round(best[k] / best["scores"], 3) for k in ("forward", "grad", "step")},
               gather_share_of_grad=round((best["grad"] - best["forward"]) / best["grad"], 3),
               scan_tflops={k: round(8.0 * B * N * V / (best[k] * 1e-3) / 1e12, 2) for k in ("scores", "forward", "grad")},
               mean_n_interior=round(float(out["n_interior"].float().mean()), 1), mean_n_contact=round(float(out["n_contact"].float().mean()), 1))
    print(f"[N={N}] scores {best['scores']:.3f} forward {best['forward']:.3f} grad {best['grad']:.3f} step {best['step']:.3f} ms per {B} grasps",
          file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(rec))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed train")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed for each child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grasp_ttt_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--points", type=int, default=SIZES[0], help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.points, args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="grasp_ttt_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": "tools/grasp_ttt_rate.py: contact.ttt_terms / ttt_value_and_grad (dvq_grasp_ttt) and one step of contact.refine_ttt "
                   "on 16 384 posed hands of the real hand model against contact.grasp_scores (dvq_grasp_scores) on the same inputs "
                   "(alternating trains, device events, one process per cloud size); one MI355X"}
    rc = 0
    me = [sys.executable, os.path.abspath(__file__)]
    try:                                                             # chained: the second size starts only after the first ended well
        for N in SIZES:
            text = child(me + ["--kernels-child", mano_path, "--points", str(N), "--trains", str(args.trains), "--calls", str(args.calls)],
                         args.limit)
            doc[f"N{N}"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({f"N{N}": {k: doc[f"N{N}"][k] for k in ("best_ms", "over_scores", "gather_share_of_grad")} for N in SIZES}))
    except RunFailed as e:
        print(f"grasp_ttt_rate: stopped at the failing run: {e}", file=sys.stderr)
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
