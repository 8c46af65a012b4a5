#!/usr/bin/env python3
"""Measured cost of the MANO layer's backward pass (tools/grasp_self_rate.py's pattern: the GPU step is a child process under its
own time limit, the tool itself never opens the GPU; a non-zero exit ends the measurement).

  ONE child process times, at B = 16 384 hands of the real hand model (tests/golden/g9_mano_right.pkl.xz; betas ~ N(0,1), PCA pose
  ~ N(0, 0.3^2), random orientation and translation) and alternating:
    "forward"        the layer with no input requiring grad (dvq_mano_forward: today's three launches);
    "forward+back"   the layer with all four inputs requiring grad, loss = <vertices, gv> + <joints, gj>, loss.backward()
                     (dvq_mano_forward, then dvq_mano_backward: the forward state recomputed, three more launches);
    "torch"          forward + backward of tests/mano_grad_ref.py in float32 on the same device: what a user without the fused
                     backward would write.
  Device events around trains of calls, one untimed warm-up train each, then `--trains` timed trains per path, A B C A B C ...  The
  library's per-launch events (dvq_prof_*) give the backward's kernel-by-kernel split in a run of their own afterwards.

    python tools/mano_backward_rate.py [--trains 5] [--calls 10] [--out profiles/mano_backward_rate.json]
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
B = 16384


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
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import _lib, mano as dmano, ops
    import mano_grad_ref
    import mano_ref
    dev = torch.device("cuda", 0)
    arrays = dmano.read_mano_pkl(mano_path)
    layer = dmano.ManoLayer(arrays, flat_hand_mean=True).to(dev)
    restated = mano_grad_ref.ManoTorch(mano_ref.device_arrays(arrays), flat_hand_mean=True, dtype=torch.float32, device=dev)
    g = torch.Generator().manual_seed(6)
    ins = [torch.randn(B, 10, generator=g), torch.randn(B, 45, generator=g) * 0.3, torch.randn(B, 3, generator=g),
           torch.randn(B, 3, generator=g) * 0.2]
    betas, pose, orient, transl = (t.to(dev) for t in ins)
    gv, gj = torch.randn(B, 778, 3, generator=g).to(dev), torch.randn(B, 16, 3, generator=g).to(dev)
    leaf = [t.clone().requires_grad_(True) for t in (betas, pose, orient, transl)]

    def forward():
        return layer(betas=betas, global_orient=orient, hand_pose=pose, transl=transl).vertices

    def forward_back():
        for t in leaf:
            t.grad = None
        out = layer(betas=leaf[0], global_orient=leaf[2], hand_pose=leaf[1], transl=leaf[3])
        ((out.vertices * gv).sum() + (out.joints * gj).sum()).backward()
        return leaf[0].grad

    def torch_path():
        for t in leaf:
            t.grad = None
        v, j = restated(leaf[0], leaf[1], leaf[2], leaf[3])
        ((v * gv).sum() + (j * gj).sum()).backward()
        return leaf[0].grad

    paths = {"forward": forward, "forward+back": forward_back, "torch": torch_path}
    a = [t.clone() for t in (forward_back(), leaf[1].grad, leaf[2].grad, leaf[3].grad)]
    b = [t.clone() for t in (torch_path(), leaf[1].grad, leaf[2].grad, leaf[3].grad)]
    agree = [round(float((x - y).abs().max()), 9) for x, y in zip(a, b)]      # the two paths compute the same thing

    def train(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            r = fn()
        e1.record()
        e1.synchronize()
        del r
        return e0.elapsed_time(e1) / calls

    rec = {"B": B, "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0),
           "max_abs_difference_layer_vs_torch": dict(zip(("betas", "pose", "orient", "transl"), agree)),
           "ms_per_call": {k: [] for k in paths}}
    for k in paths:                                                  # untimed warm-up train of each path
        train(paths[k])
    for _ in range(trains):                                          # A B C A B C ...
        for k in paths:
            rec["ms_per_call"][k].append(round(train(paths[k]), 4))
    ms = rec["ms_per_call"]
    best = {k: min(v) for k, v in ms.items()}
    rec.update(best_ms=best, spread={k: spread(v) for k, v in ms.items()},
               forward_back_over_forward=round(best["forward+back"] / best["forward"], 3),
               torch_over_forward_back=round(best["torch"] / best["forward+back"], 3))
    # kernel by kernel: the library's own events around every launch of a few forward+backward calls
    lib = _lib.load()
    torch.cuda.synchronize(dev)
    lib.dvq_prof_reset()
    lib.dvq_prof_enable(1)
    for _ in range(calls):
        forward_back()
    torch.cuda.synchronize(dev)
    lib.dvq_prof_enable(0)
    buf = (_lib.ProfEntry * 64)()
    n = lib.dvq_prof_read(buf, 64)
    rec["launches_ms_per_call"] = {buf[i].name.decode(): round(float(buf[i].ms) / calls, 4) for i in range(min(n, 64))}
    lib.dvq_prof_reset()
    ops.release_workspaces()
    print(f"[kernels] forward {best['forward']:.3f} ms, forward+back {best['forward+back']:.3f} ms, torch {best['torch']:.3f} ms per {B} hands "
          f"(spread {rec['spread']})", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(rec))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed train")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed for the child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mano_backward_rate.json"))
    ap.add_argument("--kernels-child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels_child:
        return kernels_child(args.kernels_child, args.trains, args.calls)
    tmp = tempfile.mkdtemp(prefix="mano_backward_rate_")
    mano_path = os.path.join(tmp, "MANO_RIGHT.pkl")
    with open(FIXTURE, "rb") as f, open(mano_path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    doc = {"what": "tools/mano_backward_rate.py: the MANO layer at B = 16 384 real-model hands -- forward alone, forward + backward through "
                   "the layer (dvq_mano_forward + dvq_mano_backward), forward + backward of the float32 torch restatement "
                   "(tests/mano_grad_ref.py) on the same device; alternating trains, device events, one process; one MI355X"}
    rc = 0
    try:
        text = child([sys.executable, os.path.abspath(__file__), "--kernels-child", mano_path, "--trains", str(args.trains),
                      "--calls", str(args.calls)], args.limit)
        doc["kernels"] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({k: doc["kernels"][k] for k in ("best_ms", "spread", "forward_back_over_forward", "torch_over_forward_back",
                                                         "launches_ms_per_call")}))
    except RunFailed as e:
        print(f"mano_backward_rate: stopped at the failing run: {e}", file=sys.stderr)
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
