#!/usr/bin/env python3
"""Measured cost of the fused articulated push-out (tools/grasp_refine_rigid_rate.py's pattern: the GPU run is a child process under
its own time limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

  ONE child process times, on identical inputs and alternating, `contact.refine_fingers` at steps = 8, spin = 1, curl = 1 (ONE launch
  of dvq_grasp_refine_fingers: 21 + 40 sums per scan in three rounds of the tree, the hand's planes and normals rebuilt after every
  step that curls a finger) against `contact.refine_rigid` at steps = 8, spin = 1 (ONE launch of dvq_grasp_refine_rigid).  The new
  kernel has no earlier version to compare with, so the rigid kernel on the same inputs is the yardstick; it is not the code under
  test, and no target is fixed.  B = 16 384 grasps, V = 778, N in {1024, 3000}: device events around trains of calls, one untimed
  warm-up train each, then `--trains` timed trains per path, A B A B ...  The hand is the MANO template of
  tests/golden/g9_mano_right.pkl.xz under a per-grasp offset, the pivot its root joint, the knuckles its five knuckle joints, the rig
  `contact.FingerRig.from_mano`, the cloud a channel-first [B,4,N] tensor read in place, as the generation path holds it.  The two
  kernels take different paths through the iterates, so the record also holds the share of grasps that kept a later iterate, the mean
  iterate kept, and the share with a curled finger.  A third path, the fingers kernel at curl = 0, walks exactly the rigid kernel's
  iterates (its outputs are checked to be the same bits): its ratio is the cost of the kernel's larger register file alone.

    python tools/grasp_refine_fingers_rate.py [--trains 5] [--calls 5] [--out profiles/grasp_refine_fingers_rate.json]
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
B, V, SIZES, STEPS = 16384, 778, (1024, 3000), 8


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
    rig = contact.FingerRig.from_mano(dmano.load(model_path=mano_path), dev)
    g = torch.Generator().manual_seed(5)
    template = torch.from_numpy(np.asarray(arrays["v_template"], np.float32))
    centre = template.mean(0)
    offset = torch.randn(B, 1, 3, generator=g) * 0.2
    hand = (template[None] + offset + torch.randn(B, V, 3, generator=g) * 0.001).to(dev).contiguous()
    joints = torch.from_numpy(np.asarray(arrays["J_regressor"], np.float32)) @ template                        # the template's joints [16,3]
    pivot = (joints[None, 0] + offset[:, 0]).to(dev).contiguous()
    knuckles = (joints[rig.joints][None] + offset).to(dev).contiguous()                                         # [B,5,3]
    out = {"B": B, "V": V, "steps": STEPS, "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0), "cases": {}}
    for N in SIZES:
        cloud = torch.empty(B, 4, N)
        cloud[:, :3] = (centre[None, None] + offset + torch.randn(B, N, 3, generator=g) * 0.03).transpose(1, 2)   # around the hand
        cloud[:, 3] = 0.2
        cloud = cloud.to(dev)
        obj = cloud[:, :3].transpose(1, 2)

        paths = {"fingers": lambda: contact.refine_fingers(topo, rig, hand, obj, pivot, knuckles, STEPS, spin=1.0, curl=1.0),
                 "rigid": lambda: contact.refine_rigid(topo, hand, obj, pivot, STEPS, spin=1.0),
                 "fingers_curl0": lambda: contact.refine_fingers(topo, rig, hand, obj, pivot, knuckles, STEPS, spin=1.0, curl=0.0)}

        def train(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                r = fn()
            b.record()
            b.synchronize()
            del r
            return a.elapsed_time(b) / calls

        f, s = paths["fingers"](), paths["rigid"]()
        zero = paths["fingers_curl0"]()
        same = bool(all(torch.equal(zero[k], s[k]) for k in ("offset", "quat", "iter", "n_interior", "n_contact"))
                    and torch.equal(zero["penetration"].view(torch.int32), s["penetration"].view(torch.int32)))
        before = contact.grasp_scores(topo, hand, obj)["penetration"].double().sum()
        rec = {"curl0_equals_rigid": same, "ms_per_call": {k: [] for k in paths}}
        for k, r in (("fingers", f), ("rigid", s)):
            rec[k] = {"moved_share": round(float((r["iter"] > 0).float().mean()), 4), "mean_iter_kept": round(float(r["iter"].float().mean()), 3),
                      "penetration_after_over_before": round(float(r["penetration"].double().sum() / before), 4)}
        rec["fingers"]["curled_share"] = round(float((f["finger_quat"][..., 0] != 1).any(dim=1).float().mean()), 4)
        del f, s, zero, before
        for k in paths:                                              # untimed warm-up train of each path
            train(paths[k])
        for _ in range(trains):                                      # A B A B ...
            for k in paths:
                rec["ms_per_call"][k].append(round(train(paths[k]), 4))
        ms = rec["ms_per_call"]
        best = {k: min(v) for k, v in ms.items()}
        ratio = best["fingers"] / best["rigid"]
        rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()}, fingers_over_rigid=round(ratio, 3),
                   fingers_curl0_over_rigid=round(best["fingers_curl0"] / best["rigid"], 3),
                   # per (point, vertex) pair 3 subtractions, 1 product, 2 fmas = 8 FLOPs, nine scans at most
                   flops_at_most=8.0 * B * N * V * (STEPS + 1))
        out["cases"][str(N)] = rec
        print(f"[kernels] N={N}: fingers {best['fingers']:.3f} ms, rigid {best['rigid']:.3f} ms per {B} grasps "
              f"(ratio {ratio:.3f}, spread {rec['spread']}), curl0_equals_rigid={same}", file=sys.stderr, flush=True)
        del cloud, obj
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))
    return 0 if all(c["curl0_equals_rigid"] for c in out["cases"].values()) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed train")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grasp_refine_fingers_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="grasp_refine_fingers_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": (f"tools/grasp_refine_fingers_rate.py: ONE launch of dvq_grasp_refine_fingers at steps = {STEPS}, spin = 1, curl = 1 against "
                    "ONE launch of dvq_grasp_refine_rigid on the same inputs (alternating trains, device events, one process); one MI355X")}
    rc = 0
    try:
        text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", mano_path, "--trains", str(args.trains),
                      "--calls", str(args.calls)], args.limit)
        doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({N: {k: c[k] for k in ("best_ms", "spread", "fingers_over_rigid", "fingers_curl0_over_rigid")}
                          for N, c in doc["kernels"]["cases"].items()}))
    except RunFailed as e:
        print(f"grasp_refine_fingers_rate: stopped at the failing run: {e}", file=sys.stderr)
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
