#!/usr/bin/env python3
"""Measured cost of the beam search over the prior (tools/grasp_self_rate.py's pattern: every GPU step is a child process under
its own time limit, the tool itself never opens the GPU; the steps are chained, and a non-zero exit ends the measurement).

  Step "prior": the full prior (512 tokens, dim 512, 15 layers, 128 classes, synthetic weights) in ONE child process.  For
  S x W = 16 x 1024, 160 x 100 and 2048 x 8: `ops.pixelcnn_beam` (dvq_pixelcnn_beam) on S seeded labels against
  `ops.pixelcnn_sample` (dvq_pixelcnn_sample) on the same labels repeated to S * W rows -- device events around trains of calls,
  one untimed warm-up train each, then `--trains` timed trains per path, A B A B ...  Afterwards, in a run of its own, the
  library's per-launch events (dvq_prof_*) split one search by kernel: the share of beam_expand_kernel and of the score pass.

  Step "gen": `GenNet.gen_beam` on S clouds against `GenNet.gen` on the same clouds repeated W times (what best-of-M does today),
  160 x 100 at `--points` points per cloud, timed the same way: this is where encoding each cloud once shows.

    python tools/pixelcnn_beam_rate.py [--trains 5] [--calls 3] [--points 1024] [--out profiles/pixelcnn_beam_rate.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((16, 1024), (160, 100), (2048, 8))
GEN_SHAPE = (160, 100)


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


def _net():
    import torch
    from dvqvae_amd import mano as dmano, synth
    from dvqvae_amd.network.gen_net import GenNet
    dev = torch.device("cuda", 0)
    net = GenNet()
    sd = synth.synthetic_state_dict(net.state_dict(), 1234)
    sd["GatedPixelCNN.output_conv.2.bias"][128:] = -1e4                # codes inside the 128-row codebooks, as generate.load_model
    net.load_state_dict(sd)
    net.eval().to(dev)
    net.set_rh_mano(dmano.ManoLayer(dmano.synthetic_mano_arrays()).to(dev))
    return net, dev


def _trains(paths, trains, calls):
    """Alternating trains of ``calls`` calls per path, device events: {path: [ms per call]}."""
    import torch

    def train(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            r = fn()
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b) / calls

    ms = {k: [] for k in paths}
    for k in paths:                                                  # untimed warm-up train of each path
        train(paths[k])
    for _ in range(trains):                                          # A B A B ...
        for k in paths:
            ms[k].append(round(train(paths[k]), 4))
    return ms


def prior_child(trains, calls):
    sys.path.insert(0, ROOT)
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import _lib, ops
    net, dev = _net()
    pk = net.GatedPixelCNN.packed()
    lib = _lib.load()
    rec = {"prior": [512, 512, 15, 128], "trains": trains, "calls_per_train": calls, "device": torch.cuda.get_device_name(0), "shapes": []}
    for S, W in SHAPES:
        g = torch.Generator().manual_seed(S + W)
        lab = torch.randint(0, 128, (S,), generator=g).to(dev)
        rows = lab.repeat_interleave(W).contiguous()
        q = ops.exp1_noise(S * W, 9 * 512, 7, 0, 0, device=dev).view(S * W, 9, 512)
        err = ops.new_err_flag(dev)
        paths = {"beam": lambda: ops.pixelcnn_beam(pk, lab, W, err=err), "sample": lambda: ops.pixelcnn_sample(pk, rows, q, err=err)}
        ms = _trains(paths, trains, calls)
        best = {k: min(v) for k, v in ms.items()}
        codes, score, n_live = ops.pixelcnn_beam(pk, lab, W)
        lib.dvq_prof_reset()
        lib.dvq_prof_enable(1)
        ops.pixelcnn_beam(pk, lab, W, err=err)
        torch.cuda.synchronize()
        lib.dvq_prof_enable(0)
        buf = (_lib.ProfEntry * 64)()
        n = lib.dvq_prof_read(buf, 64)
        kern = {buf[i].name.decode(): round(buf[i].ms, 4) for i in range(n)}
        lib.dvq_prof_reset()
        total = sum(kern.values())
        shape = {"S": S, "W": W, "rows": S * W, "ms_per_call": ms, "best_ms": best, "spread": {k: spread(v) for k, v in ms.items()},
                 "beam_over_sample": round(best["beam"] / best["sample"], 3), "n_live_min": int(n_live.min()),
                 "best_log_prob_mean": round(float(score[:, 0].mean()), 4), "kernel_ms_one_search": kern,
                 "expand_share": round(kern.get("pixelcnn_beam_expand", 0.0) / total, 4) if total else None,
                 "score_share": round(kern.get("pixelcnn_beam_score", 0.0) / total, 4) if total else None}
        rec["shapes"].append(shape)
        print(f"[prior] {S} x {W}: beam {best['beam']:.2f} ms, sample {best['sample']:.2f} ms, expand share {shape['expand_share']}",
              file=sys.stderr, flush=True)
        del q, rows
    print("RESULT " + json.dumps(rec))
    return 0


def gen_child(trains, calls, points):
    sys.path.insert(0, ROOT)
    import torch
    import dvqvae_amd  # noqa: F401
    from dvqvae_amd import synth
    net, dev = _net()
    S, W = GEN_SHAPE
    obj = synth.synthetic_clouds(S, points, seed=5).to(dev)
    rep = obj.repeat_interleave(W, 0).contiguous()
    net.set_noise_seed(3)
    paths = {"gen_beam": lambda: net.gen_beam(obj, W), "gen": lambda: net.gen(rep)}
    ms = _trains(paths, trains, calls)
    best = {k: min(v) for k, v in ms.items()}
    rec = {"S": S, "W": W, "rows": S * W, "points": points, "trains": trains, "calls_per_train": calls,
           "device": torch.cuda.get_device_name(0), "ms_per_call": ms, "best_ms": best, "spread": {k: spread(v) for k, v in ms.items()},
           "gen_beam_over_gen": round(best["gen_beam"] / best["gen"], 3)}
    print(f"[gen] {S} x {W}: gen_beam {best['gen_beam']:.2f} ms, gen {best['gen']:.2f} ms", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(rec))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--trains", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed train")
    ap.add_argument("--points", type=int, default=1024, help="points per cloud of the gen step")
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed for each child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixelcnn_beam_rate.json"))
    ap.add_argument("--prior-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--gen-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.prior_child:
        return prior_child(args.trains, args.calls)
    if args.gen_child:
        return gen_child(args.trains, args.calls, args.points)
    doc = {"what": "tools/pixelcnn_beam_rate.py: ops.pixelcnn_beam (dvq_pixelcnn_beam) against ops.pixelcnn_sample on the same labels "
                   "repeated to S * W rows, and GenNet.gen_beam against GenNet.gen on the clouds repeated (alternating trains, device "
                   "events, one process per step); one MI355X"}
    rc = 0
    me = [sys.executable, os.path.abspath(__file__), "--trains", str(args.trains), "--calls", str(args.calls), "--points", str(args.points)]
    try:                                                             # chained: the second step starts only after the first ended well
        for step, flag in (("prior", "--prior-child"), ("gen", "--gen-child")):
            text = child(me + [flag], args.limit)
            doc[step] = json.loads([l for l in text.splitlines() if l.startswith("RESULT ")][-1][7:])
        print(json.dumps({"prior": [{k: s[k] for k in ("S", "W", "best_ms", "beam_over_sample", "expand_share")} for s in doc["prior"]["shapes"]],
                          "gen": {k: doc["gen"][k] for k in ("best_ms", "spread", "gen_beam_over_gen")}}))
    except RunFailed as e:
        print(f"pixelcnn_beam_rate: stopped at the failing run: {e}", file=sys.stderr)
        doc["stopped"] = str(e)[:600]
        rc = 1
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    return rc


if __name__ == "__main__":
    sys.exit(main())
