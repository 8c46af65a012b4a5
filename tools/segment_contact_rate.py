#!/usr/bin/env python3
"""Measured cost of the object-side contact map (tools/grasp_parts_rate.py's pattern: the GPU run is a child process under its own
time limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

  ONE child process times, on identical rows and alternating, `contact.object_contact` (dvq_segment_contact: a workgroup holds 1024
  object points still and walks the segment's rows) against `contact.grasp_scores` (dvq_grasp_scores: a workgroup holds a hand still
  and walks the object points -- the yardstick: the same (row, point, vertex) pairs, the loops swapped) on 16 384 real-model hands
  (16 400 for the grouping of 100), V = 778, N in {1024, 3000}, for the groupings O x K = 16 384 x 1, 164 x 100 and 16 x 1024: device
  events around trains of calls, one untimed warm-up train each, then `--trains` timed trains per path, A B A B ...  The number of
  calls of a train is set per case so that a train runs for about `--train_ms`.  The hand is the MANO template of
  tests/golden/g9_mano_right.pkl.xz under a per-grasp offset, the cloud a channel-first [B,4,N] tensor read in place, as the
  generation path holds it.  At N = 3000 the map kernel scans 3 x 1024 point slots for 3000 points and rebuilds the normals three
  times per row.  Every case is checked once: the column sums of touch / inside against the per-grasp n_contact / n_interior.

    python tools/segment_contact_rate.py [--trains 5] [--train_ms 300] [--out profiles/segment_contact_rate.json]
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
V, SIZES = 778, (1024, 3000)
GROUPINGS = ((16384, 1), (164, 100), (16, 1024))
B = max(o * k for o, k in GROUPINGS)                     # 16 400: every grouping takes the first O * K rows
TILE = 1024                                              # point slots of a workgroup of the map kernel: 256 threads x 4


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


def kernels_child(mano_path, trains, train_ms):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import contact, mano as dmano, ops
    assert ops.SEGMENT_CONTACT_TILE == TILE
    dev = torch.device("cuda", 0)
    arrays = dmano.read_mano_pkl(mano_path)
    topo = contact.HandTopology(arrays["faces"], V, dev)
    g = torch.Generator().manual_seed(5)
    template = torch.from_numpy(np.asarray(arrays["v_template"], np.float32))
    centre = template.mean(0)
    offset = torch.randn(B, 1, 3, generator=g) * 0.2
    hand_all = (template[None] + offset + torch.randn(B, V, 3, generator=g) * 0.001).to(dev).contiguous()
    out = {"B": B, "V": V, "tile": TILE, "trains": trains, "train_ms": train_ms, "device": torch.cuda.get_device_name(0),
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

    ok = True
    for N in SIZES:
        cloud_all = torch.empty(B, 4, N)
        cloud_all[:, :3] = (centre[None, None] + offset + torch.randn(B, N, 3, generator=g) * 0.03).transpose(1, 2)   # around the hand
        cloud_all[:, 3] = 0.2
        cloud_all = cloud_all.to(dev)
        tiles = (N + TILE - 1) // TILE
        for O, K in GROUPINGS:
            hand, obj = hand_all[:O * K], cloud_all[:O * K, :3].transpose(1, 2)
            paths = {"map": lambda: contact.object_contact(topo, hand, obj, O, K), "scores": lambda: contact.grasp_scores(topo, hand, obj)}
            m, s = paths["map"](), paths["scores"]()
            same = bool(torch.equal(m["touch"].sum(1), s["n_contact"].view(O, K).sum(1))
                        and torch.equal(m["inside"].sum(1), s["n_interior"].view(O, K).sum(1)) and int(m["n_valid"].sum()) == O * K)
            ok &= same
            rec = {"O": O, "K": K, "N": N, "workgroups": O * tiles, "sums_agree": same,
                   "touched_share": round(float((m["touch"] > 0).float().mean()), 4), "calls_per_train": {}, "ms_per_call": {k: [] for k in paths}}
            del m, s
            for k in paths:                                          # an untimed call sizes the trains; then one untimed warm-up train
                once = train(paths[k], 1)
                rec["calls_per_train"][k] = int(min(200, max(2, round(train_ms / max(once, 1e-3)))))
                train(paths[k], rec["calls_per_train"][k])
            for _ in range(trains):                                  # A B A B ...
                for k in paths:
                    rec["ms_per_call"][k].append(round(train(paths[k], rec["calls_per_train"][k]), 4))
            ms = rec["ms_per_call"]
            best = {k: min(v) for k, v in ms.items()}
            rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()}, map_over_scores=round(best["map"] / best["scores"], 3),
                       # the scan's 8 FLOPs per pair: the scores kernel does N x V of them per row, the map kernel tiles x 1024 point slots x V
                       scores_flops=8.0 * O * K * N * V, map_flops=8.0 * O * K * tiles * TILE * V, pair_ratio=round(tiles * TILE / N, 3),
                       map_tflops=round(8.0 * O * K * tiles * TILE * V / (best["map"] * 1e-3) / 1e12, 2),
                       scores_tflops=round(8.0 * O * K * N * V / (best["scores"] * 1e-3) / 1e12, 2))
            out["cases"][f"{N}:{O}x{K}"] = rec
            print(f"[kernels] N={N} {O}x{K}: map {best['map']:.3f} ms, scores {best['scores']:.3f} ms per {O * K} rows "
                  f"(spread {rec['spread']}, {rec['workgroups']} workgroups), sums agree={same}", file=sys.stderr, flush=True)
        del cloud_all, hand, obj
        torch.cuda.empty_cache()
    print("RESULT " + json.dumps(out))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--train_ms", type=float, default=300.0, help="the length of a timed train: the calls per train are set from it")
    ap.add_argument("--limit", type=int, default=420, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "segment_contact_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains, args.train_ms)
    tmp = tempfile.mkdtemp(prefix="segment_contact_rate_mano_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": "tools/segment_contact_rate.py: contact.object_contact (dvq_segment_contact) against contact.grasp_scores "
                   "(dvq_grasp_scores) on identical rows (alternating trains, device events, one process); one MI355X"}
    rc = 0
    try:
        text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", mano_path, "--trains", str(args.trains),
                      "--train_ms", str(args.train_ms)], args.limit)
        doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({name: {k: c[k] for k in ("best_ms", "spread", "map_over_scores", "workgroups")}
                          for name, c in doc["kernels"]["cases"].items()}))
    except RunFailed as e:
        print(f"segment_contact_rate: stopped at the failing run: {e}", file=sys.stderr)
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
