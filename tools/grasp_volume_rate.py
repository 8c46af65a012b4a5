#!/usr/bin/env python3
"""Measured cost of the penetration-volume kernel (tools/grasp_wrench_rate.py's pattern: the GPU run is a child process under its own
time limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

  ONE child process times `contact.grasp_volume` (dvq_grasp_volume) at B = 16 384 grasps of the real MANO hand (the template of
  tests/golden/g9_mano_right.pkl.xz under a per-grasp shift of about a centimetre and a millimetre of roughness, sealed at the wrist)
  for `res` in {0.001, 0.0025} and hulls of about 200 and about 2000 planes -- half-spaces tangent to a sphere of 4 cm about the palm
  in pseudo-random directions, built analytically: no scipy -- against `contact.grasp_scores` (dvq_grasp_scores) at N = 1024 points
  on the same hands: device events around trains of calls, one untimed warm-up train each, then `--trains` timed trains per path,
  alternating.  No target is fixed; the mean voxel count and the share of grasps with a figure are reported with the times.

    python tools/grasp_volume_rate.py [--trains 3] [--calls 5] [--out profiles/grasp_volume_rate.json]
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
RESOLUTIONS, PLANES = (0.001, 0.0025), (200, 2000)
HULL_RADIUS = 0.04


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
    hand = (template[None] + torch.randn(B, 1, 3, generator=g) * 0.01 + torch.randn(B, V, 3, generator=g) * 0.001).to(dev).contiguous()
    cloud = torch.empty(B, 4, N)
    cloud[:, :3] = (centre[None, None] + torch.randn(B, N, 3, generator=g) * 0.03).transpose(1, 2)
    cloud[:, 3] = 0.2
    obj = cloud.to(dev)[:, :3].transpose(1, 2)
    rows = torch.zeros(B, dtype=torch.int64, device=dev)
    out = {"B": B, "V": V, "N_scores": N, "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0), "cases": {}}

    def train(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            r = fn()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b) / calls

    scores = lambda: contact.grasp_scores(topo, hand, obj)
    train(scores)
    for n_planes in PLANES:
        n = torch.randn(n_planes, 3, generator=g, dtype=torch.float64)
        n = n / n.norm(dim=1, keepdim=True)
        planes = torch.cat([n, (HULL_RADIUS + n @ centre.double())[:, None]], dim=1).float().to(dev).contiguous()
        plane_off = torch.tensor([0, n_planes], dtype=torch.int32, device=dev)
        for res in RESOLUTIONS:
            volume = lambda: contact.grasp_volume(topo, hand, planes, plane_off, rows, res=res)
            first = volume()
            rec = {"mean_voxels": round(float(first["count"].clamp(min=0).float().mean()), 1),
                   "with_a_figure": round(float((first["count"] >= 0).float().mean()), 4),
                   "mean_volume_cm3": round(float(first["count"].clamp(min=0).double().mean()) * res ** 3 * 1e6, 3),
                   "ms_per_call": {"volume": [], "scores": []}}
            del first
            train(volume)                                            # untimed warm-up train
            for _ in range(trains):                                  # A B A B ...
                rec["ms_per_call"]["volume"].append(round(train(volume), 4))
                rec["ms_per_call"]["scores"].append(round(train(scores), 4))
            ms = rec["ms_per_call"]
            best = {k: min(v) for k, v in ms.items()}
            rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()}, volume_over_scores=round(best["volume"] / best["scores"], 3))
            out["cases"][f"res={res},planes={n_planes}"] = rec
            print(f"[kernels] res={res} planes={n_planes}: volume {best['volume']:.3f} ms, scores {best['scores']:.3f} ms per {B} grasps "
                  f"(spread {rec['spread']}), mean voxels {rec['mean_voxels']}", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed train")
    ap.add_argument("--limit", type=int, default=300, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grasp_volume_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="grasp_volume_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": "tools/grasp_volume_rate.py: contact.grasp_volume (dvq_grasp_volume) against contact.grasp_scores (dvq_grasp_scores, "
                   "N = 1024) on the same hands (alternating trains, device events, one process); one MI355X"}
    rc = 0
    try:
        text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", mano_path, "--trains", str(args.trains),
                      "--calls", str(args.calls)], args.limit)
        doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({k: {x: c[x] for x in ("best_ms", "spread", "volume_over_scores", "mean_voxels")}
                          for k, c in doc["kernels"]["cases"].items()}))
    except RunFailed as e:
        print(f"grasp_volume_rate: stopped at the failing run: {e}", file=sys.stderr)
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
