"""The fp16 weight image in K-tile order (csrc/gemm_f16x2.hip: f16x2_split_kernel writes it, the tiled, the small-batch and the
gate-group kernels read it): inside every [N][K] block of a plane, element (n, k) stands at (k // 32) * N * 32 + n * 32 + k % 32.

  * the image itself, element by element, against a numpy restatement of the split -- the values, their places and the row scales;
  * the tiled and the small-batch kernel on it against float64, with a ragged last row tile and a ragged last column tile;
  * tiled == small-batch bit for bit on the same rows, for the launcher's own tile width and (a child process) the other one;
  * a small prior: the codes of a batch equal the codes of its chunks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from util import load_synth
from dvqvae_amd import ops, packing, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BK = 32


def _distinct(shape, seed):
    """float32 weights, no two equal: odd integers (a permutation) times a power of two per output row, so that the rows' scales differ"""
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    w = (2 * torch.randperm(n, generator=g) + 1).float().reshape(shape)
    rows = torch.exp2((torch.arange(shape[-2]) % 5).float() - 9).reshape(-1, 1)
    return w * rows


def _numpy_split(w):
    """(plane 1, plane 2, row scales) of w [outer, N, K] in natural order: float16 of w * 2^t, then float16((w~ - w1) * 2048)"""
    amax = np.abs(w).max(axis=(0, 2))
    _, e = np.frexp(amax)                                   # amax = f * 2^e, f in [0.5, 1): the largest t with amax * 2^t < 2^15 is 15 - e
    t = (15 - e).astype(np.int32)
    ws = np.ldexp(w, t[None, :, None]).astype(np.float32)
    w1 = ws.astype(np.float16)
    w2 = ((ws - w1.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return w1, w2, np.ldexp(np.float32(1.0), -t).astype(np.float32)


def _ktile_index(outer, N, K):
    """flat index inside a plane of element (o, n, k): every [N][K] block laid out on its own"""
    o, n, k = np.meshgrid(np.arange(outer), np.arange(N), np.arange(K), indexing="ij")
    return o * N * K + (k // BK) * N * BK + n * BK + k % BK


@pytest.mark.parametrize("shape", [(40, 64), (3, 72, 96)], ids=lambda s: "x".join(map(str, s)))
def test_image_layout_values_and_row_scales(shape):
    w = _distinct(shape, 11 + len(shape))
    assert torch.unique(w).numel() == w.numel()
    pl = packing.split_f16x2([w.to(DEV)])[0]
    assert tuple(pl.planes.shape) == (2,) + tuple(shape) and pl.planes.dtype == torch.int16
    w3 = w.numpy().reshape((-1,) + tuple(shape[-2:]))
    outer, N, K = w3.shape
    w1, w2, scale = _numpy_split(w3)
    idx = _ktile_index(outer, N, K)
    assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(outer * N * K))       # a permutation of the plane
    got = pl.planes.cpu().numpy().view(np.float16).reshape(2, -1)
    for p, want in enumerate((w1, w2)):
        at = got[p][idx]                                    # [outer, N, K]: what stands where element (o, n, k) belongs
        bad = np.argwhere(at.view(np.uint16) != want.view(np.uint16))
        assert bad.size == 0, f"plane {p}: {len(bad)} elements differ, first (o, n, k) = {bad[0].tolist()}"
    assert np.array_equal(pl.scale.cpu().numpy(), scale)


KS = (32, 64, 96)
N_OUT, M_TILED, M_SKINNY = 72, 300, 40


def _problem():
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(M_TILED, k, generator=g).to(DEV) for k in KS]
    ws = [(torch.randn(N_OUT, k, generator=g) / np.sqrt(sum(KS))).to(DEV) for k in KS]
    b = torch.randn(N_OUT, generator=g).to(DEV)
    return xs, ws, b


@pytest.fixture(scope="module")
def outputs():
    """(inputs, the M = 300 call on the tiled kernel, the M = 40 call on the small-batch kernel): computed once"""
    xs, ws, b = _problem()
    pls = packing.split_f16x2(ws)
    big = ops.linear_multi(list(zip(xs, ws)), b, planes=pls)
    small = ops.linear_multi([(x[:M_SKINNY], w) for x, w in zip(xs, ws)], b, planes=pls)
    return xs, ws, b, big, small


def test_three_sources_against_float64(outputs):
    """K = 32, 64, 96 into N = 72: the last row tile (300 = 2 x 128 + 44) and the only column tile are ragged; the bound is the
    project's for its fp32-class GEMMs (test_linear_fuzz_shapes_planes_and_batch_invariance)."""
    xs, ws, b, big, small = outputs
    ref = sum(x.double() @ w.double().t() for x, w in zip(xs, ws)) + b.double()
    scale = sum(x.double().abs() @ w.double().abs().t() for x, w in zip(xs, ws)) + b.double().abs()
    for name, y, rows in (("tiled", big, M_TILED), ("small-batch", small, M_SKINNY)):
        err = (y.double() - ref[:rows]).abs()
        bound = 4e-6 * scale[:rows].max(dim=0, keepdim=True).values + 1e-30
        print(f"{name}: max error / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), name


def test_tiled_equals_small_batch_bitwise(outputs):
    _, _, _, big, small = outputs
    assert torch.equal(big[:M_SKINNY], small)


_CHILD = r"""
import os, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import dvqvae_amd
from dvqvae_amd import ops, packing
import test_gemm_f16x2_wimage_gpu as t
xs, ws, b = t._problem()
pls = packing.split_f16x2(ws)
big = ops.linear_multi(list(zip(xs, ws)), b, planes=pls)
small = ops.linear_multi([(x[:t.M_SKINNY], w) for x, w in zip(xs, ws)], b, planes=pls)
want = torch.load(sys.argv[2])
assert torch.equal(big[:t.M_SKINNY], small), "128 x 256 tiles: rows 0..39 differ from the small-batch kernel's"
assert torch.equal(big.cpu(), want), "128 x 256 tiles differ from the launcher's own choice"
print("child ok")
"""


def test_tiled_equals_small_batch_bitwise_on_the_wide_tile(outputs, tmp_path):
    """DVQ_GEMM_TN=256 in a fresh process: the 128 x 256 tile (N = 72: three of its four waves' weight rows are clamped)"""
    _, _, _, big, _ = outputs
    path = str(tmp_path / "big.pt")
    torch.save(big.cpu(), path)
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=dict(os.environ, DVQ_GEMM_TN="256"), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_small_prior_batch_equals_its_chunks():
    from dvqvae_amd.network.pixelcnn.models import GatedPixelCNN
    cfg = (32, 64, 3, 16)
    net = GatedPixelCNN(*cfg)
    load_synth(net, 77 + cfg[0])
    net = net.to(DEV)
    B = 300
    g = torch.Generator().manual_seed(B)
    lab = torch.randint(0, cfg[3], (B,), generator=g).to(DEV)
    q = synth.exp1_noise(B, 9, cfg[0], seed=B).to(DEV)
    pk = net.packed()
    whole = ops.pixelcnn_sample(pk, lab, q)
    parts = torch.cat([ops.pixelcnn_sample(pk, lab[r:r + 100], q[r:r + 100].contiguous()) for r in range(0, B, 100)])
    assert len(torch.unique(whole)) > 4
    assert torch.equal(whole, parts)
