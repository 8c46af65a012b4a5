#!/usr/bin/env python3
"""Measured cost of the self-collision kernel (tools/grasp_parts_rate.py's pattern: every GPU step is a child process under its own
time limit, the tool itself never opens the GPU; the steps are chained, and a non-zero exit ends the measurement).

  Step "figures": 16 384 hands of the real hand model (tests/golden/g9_mano_right.pkl.xz posed on the device: betas ~ N(0,1), PCA
  pose ~ N(0, 0.3^2), the distribution of the calibration) through `contact.grasp_self` at the defaults -- the share of hands with
  a penetrating vertex (every one is a false alarm: these hands do not collide), the counts' histogram and the smallest clearance.

  Step "kernels": ONE child process times, on the same hands and alternating, `contact.grasp_self` (dvq_grasp_self: 1024 source
  slots against the hand's 778 vertices) against `contact.grasp_scores` (dvq_grasp_scores: a cloud of N = 1024 points against the
  hand -- the yardstick) at B = 16 384: device events around trains of calls, one untimed warm-up train each, then `--trains` timed
  trains per path, A B A B ...  The self kernel's pairs are 1024 x 778 per grasp against 1024 x 778 of the scores kernel at N = 1024
  when the idle slots are counted, 778 x 778 = 0.76 x when they are not: a ratio far above 1 is a finding to explain.

    python tools/grasp_self_rate.py [--trains 5] [--calls 20] [--out profiles/grasp_self_rate.json]
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
B, V, N = 16384, 778, 1024
SLOTS = 1024                     # source slots of a pass of the self kernel: 256 threads x 4


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


def _hands(mano_path):
    """(topology, table, hands [B,778,3]) on the device."""
    import numpy as np
    import torch
    from dvqvae_amd import contact, mano as dmano
    dev = torch.device("cuda", 0)
    layer = dmano.load(model_path=mano_path, model_type="mano", use_pca=True, num_pca_comps=45, flat_hand_mean=True).to(dev)
    faces = np.asarray(layer.faces)
    topo = contact.HandTopology(faces, V, dev)
    table = contact.SelfTable(contact.HandParts.from_json(), faces, device=dev)
    g = torch.Generator().manual_seed(6)
    betas = torch.randn(B, 10, generator=g)
    betas[0] = 0.0
    pose = torch.randn(B, 45, generator=g) * 0.3
    orient = torch.randn(B, 3, generator=g)
    transl = torch.randn(B, 3, generator=g) * 0.2
    with torch.no_grad():
        hands = layer(betas=betas.to(dev), global_orient=orient.to(dev), hand_pose=pose.to(dev), transl=transl.to(dev)).vertices.contiguous()
    return topo, table, hands


def figures_child(mano_path):
    sys.path.insert(0, ROOT)
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import contact
    topo, table, hands = _hands(mano_path)
    out = contact.grasp_self(topo, table, hands)
    total = out["pen_count"].sum(dim=1).cpu()
    gap = out["gap_min"].min(dim=1).values.cpu().double().sqrt() * 100.0
    rec = {"B": B, "V": V, "seam_vertices": table.n_seam, "reach": contact.SELF_REACH, "margin": contact.SELF_MARGIN,
           "rows_with_a_figure": round(float((out["status"] == 0).float().mean()), 4),
           "share_penetrating": round(float((total > 0).float().mean()), 6), "mean_penetrating": round(float(total.float().mean()), 6),
           "count_histogram_0_to_9_and_more": [int((total == k).sum()) for k in range(10)] + [int((total >= 10).sum())],
           "min_clearance_cm": round(float(gap.min()), 4), "device": torch.cuda.get_device_name(0)}
    print("RESULT " + json.dumps(rec))
    return 0


def kernels_child(mano_path, trains, calls):
    sys.path.insert(0, ROOT)
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import contact
    topo, table, hands = _hands(mano_path)
    dev = hands.device
    g = torch.Generator().manual_seed(7)
    cloud = torch.empty(B, 4, N)
    cloud[:, :3] = (torch.randn(B, N, 3, generator=g) * 0.03).transpose(1, 2)
    cloud[:, 3] = 0.2
    cloud = cloud.to(dev)
    cloud[:, :3] += hands.mean(dim=1)[:, :, None]                    # around the hand
    obj = cloud[:, :3].transpose(1, 2)                               # channel-first, read in place, as the generation path holds it
    paths = {"self": lambda: contact.grasp_self(topo, table, hands), "scores": lambda: contact.grasp_scores(topo, hands, obj)}

    def train(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            r = fn()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b) / calls

    rec = {"B": B, "V": V, "N": N, "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0),
           "ms_per_call": {k: [] for k in paths}}
    for k in paths:                                                  # untimed warm-up train of each path
        train(paths[k])
    for _ in range(trains):                                          # A B A B ...
        for k in paths:
            rec["ms_per_call"][k].append(round(train(paths[k]), 4))
    ms = rec["ms_per_call"]
    best = {k: min(v) for k, v in ms.items()}
    rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()}, self_over_scores=round(best["self"] / best["scores"], 3),
               # the scan's 8 FLOPs per pair: the scores kernel does N x V of them, the self kernel 1024 source slots x V
               scores_flops=8.0 * B * N * V, self_flops=8.0 * B * SLOTS * V, pair_ratio_counting_idle_slots=round(SLOTS / N, 3),
               pair_ratio_of_real_vertices=round(V / N, 3),
               self_tflops=round(8.0 * B * SLOTS * V / (best["self"] * 1e-3) / 1e12, 2),
               scores_tflops=round(8.0 * B * N * V / (best["scores"] * 1e-3) / 1e12, 2))
    print(f"[kernels] self {best['self']:.3f} ms, scores {best['scores']:.3f} ms per {B} grasps (spread {rec['spread']})",
          file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(rec))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed train")
    ap.add_argument("--limit", type=int, default=180, help="seconds allowed for each child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grasp_self_rate.json"))
    ap.add_argument("--figures-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.figures_child:
        return figures_child(args.figures_child)
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="grasp_self_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": "tools/grasp_self_rate.py: contact.grasp_self (dvq_grasp_self) on 16 384 posed hands of the real hand model, its "
                   "figures and its time against contact.grasp_scores (dvq_grasp_scores, N = 1024) on the same hands (alternating "
                   "trains, device events, one process); one MI355X"}
    rc = 0
    me = [sys.executable, os.path.abspath(__file__)]
    try:                                                             # chained: the second step starts only after the first ended well
        for step, cmd in (("figures", me + ["--figures-child", mano_path]),
                          ("kernels", me + ["--kernels-child", mano_path, "--trains", str(args.trains), "--calls", str(args.calls)])):
            text = child(cmd, args.limit)
            doc[step] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({"figures": {k: doc["figures"][k] for k in ("share_penetrating", "mean_penetrating", "min_clearance_cm")},
                          "kernels": {k: doc["kernels"][k] for k in ("best_ms", "spread", "self_over_scores")}}))
    except RunFailed as e:
        print(f"grasp_self_rate: stopped at the failing run: {e}", file=sys.stderr)
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
