#!/usr/bin/env python3
"""Measured cost of making object clouds from meshes on the device (tools/segment_contact_rate.py's pattern: the GPU run is a child
process under its own time limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

  ONE child process times, alternating, each kernel path against a torch restatement on the same device and the same inputs:
    `ops.mesh_sample` (dvq_mesh_sample: one workgroup per object for the integer weights and their prefix sum, then one thread per
        sample) at S = 3000 and 12 000 over 256 objects of 4 096 and of 65 536 faces, against face areas by `torch.linalg.cross`,
        `torch.multinomial(areas, S, replacement=True)`, a gather of the three vertices and the folded barycentric point;
    `ops.cloud_fps` (dvq_cloud_fps: one workgroup of 1024 threads per object, the pool in registers) 12 000 -> 3 000 over 1, 256 and
        1 024 objects, against a `keep`-step loop of `torch.cdist` to the last pick, `torch.minimum` and `argmax` over the whole batch.
  Device events around trains of calls, one untimed warm-up train each, then `--trains` timed trains per path, A B A B ...; the number of
  calls of a train is set per case so that a train runs for about `--train_ms` (at least one call).  The meshes are height fields over
  a jittered grid (2 n m faces), the pools the kernel's own samples of them.  Every case is checked once: status 0 everywhere, faces
  inside the object, `keep` distinct picks, and the two paths' smallest kept separation side by side (the restatement rounds its
  distances differently, so its picks may part from the kernel's).

    python tools/mesh_sample_rate.py [--trains 5] [--train_ms 300] [--out profiles/mesh_sample_rate.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJECTS, GRIDS, SAMPLES = 256, ((32, 64), (128, 256)), (3000, 12000)          # 2 n m = 4 096 and 65 536 faces
FPS_POOL, FPS_KEEP, FPS_OBJECTS = 12000, 3000, (1, 256, 1024)


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


def kernels_child(trains, train_ms):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import ops
    dev = torch.device("cuda", 0)
    out = {"trains": trains, "train_ms": train_ms, "device": torch.cuda.get_device_name(0),
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "cases": {}}

    def train(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            r = fn()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b) / calls

    def measure(name, paths, rec):
        for k in paths:                                              # an untimed call sizes the trains; then one untimed warm-up train
            once = train(paths[k], 1)
            rec["calls_per_train"][k] = int(min(200, max(1, round(train_ms / max(once, 1e-3)))))
            train(paths[k], rec["calls_per_train"][k])
        for _ in range(trains):                                      # A B A B ...
            for k in paths:
                rec["ms_per_call"][k].append(round(train(paths[k], rec["calls_per_train"][k]), 4))
        best = {k: min(v) for k, v in rec["ms_per_call"].items()}
        rec.update(best_ms=best, spread={k: spread(v) for k, v in rec["ms_per_call"].items()},
                   torch_over_kernel=round(best["torch"] / best["kernel"], 2))
        out["cases"][name] = rec
        print(f"[kernels] {name}: kernel {best['kernel']:.3f} ms, torch {best['torch']:.3f} ms per call (spread {rec['spread']}), "
              f"checks {rec['checks']}", file=sys.stderr, flush=True)

    ok = True
    g = torch.Generator().manual_seed(5)
    pools = None
    for n, m in GRIDS:
        nf, nv = 2 * n * m, (n + 1) * (m + 1)
        u, w = np.meshgrid(np.arange(n + 1), np.arange(m + 1), indexing="ij")
        idx = lambda i, j: i * (m + 1) + j
        quads = [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)) for i in range(n) for j in range(m)]
        faces1 = np.asarray([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
        grid = torch.from_numpy(np.stack([u / n * 0.2, w / m * 0.1, np.zeros_like(u, float)], -1).reshape(-1, 3).astype(np.float32))
        verts = (grid[None] + torch.randn(OBJECTS, nv, 3, generator=g) * torch.tensor([0.1 / n, 0.05 / m, 0.01])).to(dev)
        faces = torch.from_numpy(faces1).to(dev)
        flat_v, flat_f = verts.reshape(-1, 3).contiguous(), faces.repeat(OBJECTS, 1).contiguous()
        vert_off = (torch.arange(OBJECTS + 1, dtype=torch.int64) * nv).to(torch.int32).to(dev)
        face_off = (torch.arange(OBJECTS + 1, dtype=torch.int64) * nf).to(torch.int32).to(dev)
        ids = torch.arange(OBJECTS, dtype=torch.int64, device=dev)
        fl = faces.long()
        for S in SAMPLES:
            def kernel():
                return ops.mesh_sample(flat_v, vert_off, flat_f, face_off, S, 7, ids)

            def restated():
                a, b, c = verts[:, fl[:, 0]], verts[:, fl[:, 1]], verts[:, fl[:, 2]]
                area = torch.linalg.cross(b - a, c - a).norm(dim=2)
                f = torch.multinomial(area, S, replacement=True)
                pick = lambda x: torch.gather(x, 1, f[:, :, None].expand(-1, -1, 3))
                r = torch.rand(OBJECTS, S, 2, device=dev)
                r = torch.where((r.sum(2, keepdim=True) > 1), 1 - r, r)
                pa = pick(a)
                return pa + r[:, :, :1] * (pick(b) - pa) + r[:, :, 1:] * (pick(c) - pa), f

            points, face, status, _ = kernel()
            checks = {"status_zero": bool((status == 0).all()), "faces_in_range": bool(((face >= 0) & (face < nf)).all()),
                      "finite": bool(torch.isfinite(points).all())}
            ok &= all(checks.values())
            if (n, m) == GRIDS[0] and S == FPS_POOL:
                pools = points.clone()                               # the farthest-point cases' pools: the kernel's own samples
            rec = {"O": OBJECTS, "faces": nf, "S": S, "checks": checks, "calls_per_train": {}, "ms_per_call": {"kernel": [], "torch": []}}
            del points, face, status
            measure(f"mesh_sample:{nf}:{S}", {"kernel": kernel, "torch": restated}, rec)
        del verts, flat_v, flat_f, faces, fl
        torch.cuda.empty_cache()

    for O in FPS_OBJECTS:
        pool = pools.repeat((O + OBJECTS - 1) // OBJECTS, 1, 1)[:O].contiguous()
        if O > OBJECTS:                                              # distinct pools: the repeats get a jitter of their own
            pool = (pool + torch.randn(O, 1, 3, generator=g).to(dev) * 1e-3).contiguous()

        def kernel():
            return ops.cloud_fps(pool, FPS_KEEP)

        def restated():
            mind = torch.full((O, FPS_POOL), float("inf"), device=dev)
            sel = torch.zeros(O, FPS_KEEP, dtype=torch.int64, device=dev)
            last = sel[:, 0]
            rows = torch.arange(O, device=dev)
            for r in range(1, FPS_KEEP):
                d = torch.cdist(pool, pool[rows, last][:, None, :]).squeeze(2)
                mind = torch.minimum(mind, d * d)
                last = mind.argmax(1)                                # (a picked point has distance 0 to itself: never the largest again)
                sel[:, r] = last
            return sel, mind

        def separation(sel):                                         # the smallest distance between two kept points of object 0, mm
            kept = pool[0, sel[0].long()].double()
            d = torch.cdist(kept, kept) + torch.eye(len(kept), device=dev, dtype=torch.float64)
            return round(float(d.min()) * 1e3, 4)

        sel, gap, status = kernel()
        tsel, _ = restated()
        checks = {"status_zero": bool((status == 0).all()), "distinct": bool((sel.long().sort(1).values.diff(dim=1) > 0).all()),
                  "min_separation_mm": {"kernel": separation(sel), "torch": separation(tsel), "first_keep_samples": separation(
                      torch.arange(FPS_KEEP, device=dev)[None])},
                  "same_picks_object0": int((sel[0].long() == tsel[0]).sum())}
        ok &= checks["status_zero"] and checks["distinct"]
        rec = {"O": O, "P": FPS_POOL, "keep": FPS_KEEP, "checks": checks, "calls_per_train": {}, "ms_per_call": {"kernel": [], "torch": []}}
        del sel, gap, status, tsel
        measure(f"cloud_fps:{O}", {"kernel": kernel, "torch": restated}, rec)
        rec["us_per_pick"] = round(rec["best_ms"]["kernel"] * 1e3 / (FPS_KEEP - 1), 3)
    print("RESULT " + json.dumps(out))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--train_ms", type=float, default=300.0, help="the length of a timed train: the calls per train are set from it")
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_sample_rate.json"))
    ap.add_argument("--kernels-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.trains, args.train_ms)
    doc = {"what": "tools/mesh_sample_rate.py: ops.mesh_sample (dvq_mesh_sample) and ops.cloud_fps (dvq_cloud_fps) against torch "
                   "restatements on the same device and inputs (alternating trains, device events, one process); one MI355X"}
    rc = 0
    try:
        text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", "--trains", str(args.trains), "--train_ms",
                      str(args.train_ms)], args.limit)
        doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({name: {k: c[k] for k in ("best_ms", "spread", "torch_over_kernel")} for name, c in doc["kernels"]["cases"].items()}))
    except RunFailed as e:
        print(f"mesh_sample_rate: stopped at the failing run: {e}", file=sys.stderr)
        doc["stopped"] = str(e)[:600]
        rc = 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
