#!/usr/bin/env python3
"""Measured cost of the mesh penetration-volume kernel (the pattern of tools/grasp_volume_rate.py and tools/grasp_mesh_rate.py: the GPU
run is a child process under its own time limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

  ONE child process times `contact.grasp_mesh_volume` (dvq_grasp_mesh_volume) at B = 16 384 grasps of the real MANO hand (the template
  of tests/golden/g9_mano_right.pkl.xz under a per-grasp shift of about a centimetre and a millimetre of roughness, sealed at the
  wrist) against closed tori (major radius 5 cm, minor 2 cm) of 256, 4 096 and 65 536 faces with the palm sunk into the tube, at voxel
  sizes of 1 mm and 2.5 mm.  The 256-face torus fits the kernel's cull list; the two larger ones overflow it, so every tile walks all
  their faces.  For scale, on the same hands: `contact.grasp_volume` (dvq_grasp_volume) at 200 planes and both voxel sizes, and
  `contact.grasp_mesh` (dvq_grasp_mesh) against the same tori.  Device events around trains of calls, one untimed warm-up train each,
  then `--trains` timed trains per path.  No target is fixed; the mean voxel count is reported with the times.

    python tools/grasp_mesh_volume_rate.py [--trains 3] [--out profiles/grasp_mesh_volume_rate.json]
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
B, V, PLANES = 16384, 778, 200
TORI = ((16, 8, 5), (64, 32, 2), (256, 128, 1))          # n, m (2 n m faces), calls per train
RES = (0.001, 0.0025)
MAJOR, MINOR = 0.05, 0.02


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


def torus(n, m):
    import numpy as np
    u, w = np.meshgrid(2 * np.pi * np.arange(n) / n, 2 * np.pi * np.arange(m) / m, indexing="ij")
    ring = MAJOR + MINOR * np.cos(w)
    v = np.stack([ring * np.cos(u), ring * np.sin(u), MINOR * np.sin(w)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    idx = lambda a, b: ((a % n) * m + (b % m)).reshape(-1)
    a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
    return v, np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3)


def kernels_child(mano_path, trains):
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
    rough = template[None] - centre + torch.randn(B, 1, 3, generator=g) * 0.01 + torch.randn(B, V, 3, generator=g) * 0.001
    sunk = (rough + torch.tensor([MAJOR, 0.0, 0.0])).to(dev).contiguous()           # the palm on the tube's centre circle
    rows = torch.zeros(B, dtype=torch.int64, device=dev)
    n = torch.randn(PLANES, 3, generator=g, dtype=torch.float64)
    n = n / n.norm(dim=1, keepdim=True)
    planes = torch.cat([n, (0.04 + n @ torch.tensor([MAJOR, 0.0, 0.0], dtype=torch.float64))[:, None]], dim=1).float().to(dev).contiguous()
    plane_off = torch.tensor([0, PLANES], dtype=torch.int32, device=dev)
    out = {"B": B, "V": V, "planes_volume": PLANES, "trains": trains, "device": torch.cuda.get_device_name(0), "hull": {}, "cases": {}}

    def train(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            r = fn()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b) / calls

    for res in RES:                                                 # for scale: the hull kernel at the same voxel sizes
        fn = lambda: contact.grasp_volume(topo, sunk, planes, plane_off, rows, res=res)
        train(fn, 5)
        t = [round(train(fn, 5), 4) for _ in range(trains)]
        out["hull"][f"res={res}"] = {"ms_per_call": t, "best_ms": min(t), "spread": spread(t)}
        print(f"[kernels] grasp_volume, {PLANES} planes, res {res}: {min(t):.3f} ms per {B} grasps", file=sys.stderr, flush=True)
    for nn, mm, calls in TORI:
        meshes = contact.ObjectMeshes([torus(nn, mm)], device=dev)
        assert meshes.closed == [True]
        rec = {"faces": 2 * nn * mm, "calls_per_train": calls}
        fn = lambda: contact.grasp_mesh(meshes, sunk, rows)         # for scale: the depth against the same mesh
        train(fn, calls)
        t = [round(train(fn, calls), 4) for _ in range(trains)]
        rec["grasp_mesh"] = {"ms_per_call": t, "best_ms": min(t), "spread": spread(t)}
        for res in RES:
            fn = lambda: contact.grasp_mesh_volume(topo, meshes, sunk, rows, res=res)
            first = fn()
            voxels = float(first["count"].float().mean())
            assert int(first["status"].max()) == 0 and voxels > 0.0
            del first
            train(fn, calls)                                        # untimed warm-up train
            t = [round(train(fn, calls), 4) for _ in range(trains)]
            rec[f"res={res}"] = {"mean_voxels": round(voxels, 1), "mean_cm3": round(voxels * res ** 3 * 1e6, 3), "ms_per_call": t,
                                 "best_ms": min(t), "spread": spread(t),
                                 "over_grasp_volume": round(min(t) / out["hull"][f"res={res}"]["best_ms"], 2),
                                 "over_grasp_mesh": round(min(t) / rec["grasp_mesh"]["best_ms"], 2)}
            print(f"[kernels] {rec['faces']} faces, res {res}: {min(t):.3f} ms per {B} grasps (spread {spread(t)}), mean voxels {voxels:.1f}",
                  file=sys.stderr, flush=True)
        out["cases"][f"faces={rec['faces']}"] = rec
    print("RESULT " + json.dumps(out))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=3)
    ap.add_argument("--limit", type=int, default=540, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grasp_mesh_volume_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains)
    tmp = tempfile.mkdtemp(prefix="grasp_mesh_volume_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": "tools/grasp_mesh_volume_rate.py: contact.grasp_mesh_volume (dvq_grasp_mesh_volume) against closed tori of 256, 4 096 and "
                   "65 536 faces with the palm sunk into the tube, at 1 mm and 2.5 mm voxels, with contact.grasp_volume (200 planes, the same "
                   "voxel sizes) and contact.grasp_mesh (the same tori) on the same hands for scale (device events, one process); one MI355X"}
    rc = 0
    try:
        text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", mano_path, "--trains", str(args.trains)], args.limit)
        doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({"hull": {k: v["best_ms"] for k, v in doc["kernels"]["hull"].items()},
                          **{k: {r: (c[r]["best_ms"], c[r]["over_grasp_volume"], c[r]["over_grasp_mesh"]) for r in c if r.startswith("res=")}
                             for k, c in doc["kernels"]["cases"].items()}}))
    except RunFailed as e:
        print(f"grasp_mesh_volume_rate: stopped at the failing run: {e}", file=sys.stderr)
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
