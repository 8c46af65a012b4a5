"""GPU check of pn_exact_kernel's pruning rules (the CPU model of the decision is tests/test_pointnet_exact_prune.py):
on clouds built to stress them the filtered trunk must give the bits of the exhaustive evaluation (DVQ_PN_EXHAUSTIVE=1: exact_dot of
every point) with both run-time consistency counters at zero, and with a fault injected into the trunk kernel (diagnostics build)
the same bits with the counters NOT at zero."""
import json
import os
import subprocess
import sys

import pytest
import torch

from dvqvae_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(C, N) for N in (1024, 778, 3000) for C in (3, 4)]


def _deal(N):
    """Tiles the points are dealt to (pn_geometry of csrc/pn_filter.h)."""
    tiles = (N + 255) // 256
    over = N - 256 * (tiles - 1)
    return tiles - 1 if tiles >= 2 and over <= 32 else tiles


def _point_of_slot(tile, slot, deal):
    return ((slot * 67) & 255) * deal + tile


def adversarial_clouds(C, N):
    """[6, C, N]: two plain clouds; a tiny-spread cloud; a cloud with an outlier point in tile 0 and eight near-duplicates of it,
    a little closer in, that share a residue modulo the dealt tiles (one tile, not the best one); a cloud whose outlier has two
    near-duplicates in its own 16-point group (slots 0, 1, 2 of tile 0: the group's third is hidden and beats the tile's c5); the
    same with the three in different groups of one tile."""
    g = torch.Generator().manual_seed(1000 * C + N)
    x = synth.synthetic_clouds(6, N, seed=70 + N + C, channels=C).clone()
    deal = _deal(N)
    x[2] = x[2, :, :1] + 1e-4 * x[2]
    far = 3.0 * x[3, :, 0]
    x[3, :, 0] = far
    for i in range(8):
        x[3, :, 1 + deal * (7 * i + 3)] = far * 0.9995 * (1 + 1e-5 * torch.randn(C, generator=g))
    for cloud, slots in ((4, (0, 1, 2)), (5, (0, 4, 64))):
        far = 3.0 * x[cloud, :, 0]
        for s in slots:
            x[cloud, :, _point_of_slot(0, s, deal)] = far * (1 + 1e-5 * torch.randn(C, generator=g))
    return x.contiguous()


def _encoder(C):
    from dvqvae_amd.network.pointnet_encoder import PointNetEncoder
    from util import load_synth
    net = PointNetEncoder(channel=C)
    load_synth(net, 40 + C)
    return net.eval().to(DEV)


def _run(net, x, **env):
    """(features, STN transforms, fault counters) of one pass with library knobs set."""
    from dvqvae_amd import _lib, ops
    env = dict(env, DVQ_PN_FILTER="2")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    _lib.load().dvq_reload_env()
    try:
        ops.pointnet_fault_counters(reset=True)
        feat, trans, _ = net(x)
        torch.cuda.synchronize()
        return feat, trans, tuple(ops.pointnet_fault_counters(reset=True))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        _lib.load().dvq_reload_env()


@pytest.mark.parametrize("C,N", CASES)
def test_pruned_filter_equals_exhaustive_on_adversarial_clouds(C, N):
    net = _encoder(C)
    x = adversarial_clouds(C, N).to(DEV)
    feat, trans, counters = _run(net, x)
    feat_all, trans_all, _ = _run(net, x, DVQ_PN_EXHAUSTIVE="1")
    assert torch.isfinite(feat).all()
    assert torch.equal(trans, trans_all), "STN trunk: filtered != exhaustive"
    bad = (feat != feat_all).nonzero()[:6].tolist()
    assert torch.equal(feat, feat_all), f"main trunk: filtered != exhaustive at (cloud, channel) {bad}"
    assert counters == (0, 0), "the records must be consistent with the exact maxima"


_CHILD = r"""
import os, sys, json, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import dvqvae_amd
import test_pointnet_exact_prune_gpu as T
out = []
for C, N in T.CASES:
    net = T._encoder(C)
    x = T.adversarial_clouds(C, N).to(T.DEV)
    abl = os.environ.pop("DVQ_PN_ABL")
    f_ref, tr_ref, _ = T._run(net, x, DVQ_PN_EXHAUSTIVE="1")
    os.environ["DVQ_PN_ABL"] = abl
    f, tr, c = T._run(net, x)
    out.append({"C": C, "N": N, "equal": bool(torch.equal(f, f_ref) and torch.equal(tr, tr_ref)), "counters": list(c)})
print(json.dumps(out))
"""


@pytest.mark.parametrize("abl,counter", [(32768, 1), (65536, 0)], ids=["inject_lie", "inject_lost"])
def test_pruned_filter_repairs_injected_faults(abl, counter):
    """PN_ABL_INJECT_LIE: a record whose top score lies about its tile raises the lower bound -- the interval check must still catch
    it; PN_ABL_INJECT_LOST: a suspect record must still have every group expanded.  Diagnostics build, a child process."""
    from dvqvae_amd import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    diag = os.path.join(root, "tools", "diag", "libdvq_hip_diag.so")
    if not os.path.exists(diag):
        r = subprocess.run(["make", "-C", os.path.join(root, "d-vqvae_amd", "csrc"), "-j", "8", "diag"], capture_output=True, text=True)
        assert r.returncode == 0 and os.path.exists(diag), r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, DVQ_DIAG_LIB="1", DVQ_PN_ABL=str(abl))
    r = subprocess.run([sys.executable, "-c", _CHILD, root], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    for case in json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("[")][-1]):
        assert case["equal"], f"an injected fault must not change a feature: {case}"
        assert case["counters"][counter] > 0, case
    assert ops.pointnet_fault_counters() == (0, 0), "the product library must not have seen an inconsistency"
