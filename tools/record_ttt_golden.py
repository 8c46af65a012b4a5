#!/usr/bin/env python3
"""Record the reference's hand-centric contact term (utils/loss.py: Contact_loss) for tests/test_grasp_ttt.py by RUNNING the
reference on the CPU -- the reference source is not read, and nothing of its text is written here.

    python tools/record_ttt_golden.py --reference /path/to/the/reference/checkout

The reference imports pytorch3d, which is not needed for this function beyond ``knn_points``: stand-in modules are placed in
``sys.modules`` before the import -- a brute-force float64 ``knn_points`` (differentiable: the distance of the nearest target) and
empty shells for the rest.  ``Contact_loss`` selects a subset of the hand's vertices through a list literal; the list is recorded by
spying on the tensor indexing.  Two float64 cases, each one posed hand of the committed MANO model (778 vertices), a cloud of 64
points around it and the mask the reference's TTT_loss would pass (nearest-vertex distance below 0.02 ** 2); recorded are the
inputs, the loss and its autograd gradient with respect to the hand.

Writes tests/golden/g10_ttt_contact.npz (data only: prior_idx int16 [204]; per case k: hand{k} [778,3], obj{k} [64,3], mask{k}
[64], loss{k}, grad{k} [778,3] float64).  Runs on the CPU only."""
import argparse
import lzma
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def knn_points(p1, p2, lengths1=None, lengths2=None, K=1, **_):
    assert K == 1
    d = ((p1[:, :, None, :] - p2[:, None, :, :]) ** 2).sum(-1)
    dists, idx = d.min(dim=-1)
    return types.SimpleNamespace(dists=dists[..., None], idx=idx[..., None])


def install_stand_ins():
    shell = lambda name, **attrs: sys.modules.setdefault(name, types.SimpleNamespace(__name__=name, __path__=[], **attrs))
    refuse = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("stand-in: not available"))
    shell("pytorch3d")
    shell("pytorch3d.loss", chamfer_distance=refuse)
    shell("pytorch3d.ops")
    shell("pytorch3d.ops.knn", knn_points=knn_points, knn_gather=refuse)
    shell("pytorch3d.structures", Meshes=refuse)
    shell("pytorch3d.structures.pointclouds", Pointclouds=refuse)


def cases():
    """Two posed hands of the committed hand model and 64 points scattered around each (float64)."""
    import mano_ref
    from dvqvae_amd import mano as dmano
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "MANO_RIGHT.pkl")
        with open(os.path.join(ROOT, "tests", "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
        arrays = mano_ref.device_arrays(dmano.read_mano_pkl(path))
    rng = np.random.default_rng(20240610)
    for k in range(2):
        betas, pose = rng.normal(0, 1.0, (1, 10)), rng.normal(0, 0.8, (1, 45))
        go, tr = rng.normal(0, 1.0, (1, 3)), rng.normal(0, 0.3, (1, 3))
        hand = np.asarray(mano_ref.mano_ref(arrays, betas, pose, go, tr)[0], np.float64)[0]
        near = hand[rng.choice(778, 64, replace=False)] + rng.normal(0, 0.012, (64, 3))
        yield hand, near


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="a checkout of the reference (the directory that holds utils/loss.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g10_ttt_contact.npz"))
    args = ap.parse_args()
    install_stand_ins()
    sys.path.insert(0, os.path.abspath(args.reference))
    from utils import loss as ref_loss                     # the reference, as it is

    seen = []
    orig = torch.Tensor.__getitem__

    def spy(self, idx):
        if isinstance(idx, tuple) and len(idx) == 3 and isinstance(idx[1], list):
            seen.append([int(i) for i in idx[1]])
        return orig(self, idx)

    out = {}
    for k, (hand, obj) in enumerate(cases()):
        h = torch.from_numpy(hand)[None].clone().requires_grad_(True)
        o = torch.from_numpy(obj)[None]
        with torch.no_grad():
            mask = knn_points(o, h).dists[..., 0] < 0.02 ** 2
        assert int(mask.sum()) >= 8 and not bool(mask.all()), int(mask.sum())
        torch.Tensor.__getitem__ = spy
        try:
            value = ref_loss.Contact_loss(o, h, mask)
        finally:
            torch.Tensor.__getitem__ = orig
        grad, = torch.autograd.grad(value, h)
        out.update({f"hand{k}": hand, f"obj{k}": obj, f"mask{k}": mask[0].numpy(), f"loss{k}": np.float64(value.item()),
                    f"grad{k}": grad[0].numpy()})
        print(f"case {k}: {int(mask.sum())} of 64 points in the mask, loss {value.item():.6e}, max|grad| {grad.abs().max().item():.3e}")
    lists = [s for s in seen if len(s) > 8]
    assert len(lists) == 2 and lists[0] == lists[1], [len(s) for s in seen]
    prior = np.asarray(lists[0], np.int16)
    assert prior.min() >= 0 and prior.max() < 778 and len(set(prior.tolist())) == len(prior)
    np.savez_compressed(args.out, prior_idx=prior, **out)
    print(f"wrote {args.out}: {len(prior)} prior vertices, {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
