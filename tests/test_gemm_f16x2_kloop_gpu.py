"""The K loop of the tiled fp16-plane GEMM kernel (csrc/gemm_f16x2.hip, gemm_f16x2_pp_kernel): a prologue that stages three K-tiles, a
steady state that feeds the pipeline without a bounds test (tiles 0 .. T - 4), the last three K-tiles peeled, and two cursors that
switch sources from registers filled long before (the descriptor of the next source, the row index of a source read through arow).

Yardstick, as in tests/test_gemm_f16x2_edges_gpu.py: the small-batch ("skinny") kernels, which serve M <= 256 by default and issue the
same MFMA sequence and the same arithmetic per element.  DVQ_GEMM_SKINNY=0 with DVQ_GEMM_TN=128 / 256 forces the tiled kernel's two
tile widths on the same inputs; batches beyond 256 rows are compared with their chunks of at most 256 rows (batched == loop,
bitwise).  Every comparison is torch.equal.

Shapes: T = 1 .. 7 K-tiles is prologue only (1 .. 3), every length of the peeled tail with an empty steady state, and one to four
steady-state trips; sources of K = 32 switch at every K-tile, up to the eight sources a launch holds; two sources over nine K-tiles
put the switch on every tile of the prologue, on the first, second and third tile behind it and on each peeled tile; M = 1 .. 257
and N = 128 .. 512 put whole, ragged and 4-byte-row blocks side by side.  The launcher tells no 32-bit from 64-bit offsets (every
launch addresses per lane in 64 bits, as before), so there is no case for that distinction; a strided-row case checks the row
stride through a source switch instead."""
import pytest
import torch

from util import load_synth
from dvqvae_amd import ops, packing, synth
from dvqvae_amd._lib import DVQ_MAX_SRC
from test_gpu_parity import _with_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MS = (1, 65, 129, 200, 257)
NS = (128, 260, 258, 512)
TNS = ("128", "256")
SKINNY_MAX_M = 256


def _tiled(fn, tn):
    return _with_env("DVQ_GEMM_SKINNY", "0", lambda: _with_env("DVQ_GEMM_TN", tn, fn))


def _problem(M, N, ks, seed, pads=None):
    """Sources of K = ks with a shared plane group; pads: source i's activation rows are slices of rows pads[i] floats longer."""
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(M, k + (pads[i] if pads else 0), generator=g).to(DEV)[:, :k] for i, k in enumerate(ks)]
    ws = [(torch.randn(N, k, generator=g) * 0.05).to(DEV) for k in ks]
    b = torch.randn(N, generator=g).to(DEV)
    return xs, ws, b, packing.split_f16x2(ws)


def _run(xs, ws, b, pls, rows=slice(None)):
    return ops.linear_multi([(x[rows], w) for x, w in zip(xs, ws)], b, planes=pls)


def _check(M, N, ks, seed, pads=None):
    xs, ws, b, pls = _problem(M, N, ks, seed, pads)
    ref = torch.cat([_run(xs, ws, b, pls, slice(r, min(M, r + SKINNY_MAX_M))) for r in range(0, M, SKINNY_MAX_M)])
    assert bool(torch.isfinite(ref).all())
    for tn in TNS:
        got = _tiled(lambda: _run(xs, ws, b, pls), tn)
        assert torch.equal(ref, got), f"M={M} N={N} K={ks} tile {tn}: tiled kernel != skinny kernel"


@pytest.mark.parametrize("M", MS)
def test_one_to_seven_ktiles(M):
    """One source of T K-tiles: T <= 3 never enters the loop, T = 4 .. 7 runs one to four steady-state trips before the peeled tail."""
    for N in NS:
        for T in range(1, 8):
            _check(M, N, (32 * T,), 1000 * M + N + T)


@pytest.mark.parametrize("M", MS)
def test_a_switch_at_every_ktile(M):
    """Sources of one K-tile each, two up to the most a launch holds: both cursors switch in every load phase (and three times in the
    prologue), every descriptor fetched one compute phase before it is used."""
    for N in NS:
        for ns in range(2, DVQ_MAX_SRC + 1):
            _check(M, N, (32,) * ns, 2000 * M + N + ns)


@pytest.mark.parametrize("M", (65, 257))
def test_a_switch_on_each_ktile_of_nine(M):
    """Nine K-tiles in two sources, the second starting at tile 1 .. 8: inside the prologue (1, 2), on the first three tiles the
    steady state loads (3, 4, 5) and on each peeled tile (6, 7, 8); then three sources whose switches are one and two tiles apart."""
    for N in (128, 260):
        for first in range(1, 9):
            _check(M, N, (32 * first, 32 * (9 - first)), 3000 * M + N + first)
        for ks in ((96, 32, 160), (64, 64, 32, 128), (128, 32, 32, 32, 64)):
            _check(M, N, ks, 4000 * M + N + len(ks))


def test_strided_rows_through_a_switch():
    """Activation rows that are slices of longer rows, a different stride per source."""
    for M in (129, 257):
        _check(M, 260, (64, 96, 32), 77 + M, pads=(4, 8, 12))


# ---------------------------------------------------------------------------------------------------------------- the prior
CFGS = [(32, 64, 3, 16), (64, 128, 4, 8)]


def _prior(cfg):
    from dvqvae_amd.network.pixelcnn.models import GatedPixelCNN
    net = GatedPixelCNN(*cfg)
    load_synth(net, 77 + cfg[0])
    return net.to(DEV)


def _inputs(cfg, B):
    g = torch.Generator().manual_seed(B * 31 + cfg[0])
    x = torch.randint(0, cfg[0], (B, 3, 3), generator=g).to(DEV)
    lab = torch.randint(0, cfg[3], (B,), generator=g).to(DEV)
    return x, lab, synth.exp1_noise(B, 9, cfg[0], seed=B).to(DEV)


def _prior_outputs(net, x, lab, q):
    """codes + logits of the sampler, teacher-forced logits, log-likelihood of x: everything the prior's three entry points give"""
    pk = net.packed()
    codes, logits = ops.pixelcnn_sample(pk, lab, q, return_logits=True)
    return codes, logits, ops.pixelcnn_forward(pk, x, lab), net.log_prob(x, lab)


def _chunked(net, x, lab, q):
    """the batch as chunks the small-batch kernels serve, joined: computed once per (configuration, batch, tables)"""
    parts = [_prior_outputs(net, x[r:r + SKINNY_MAX_M], lab[r:r + SKINNY_MAX_M], q[r:r + SKINNY_MAX_M].contiguous())
             for r in range(0, x.shape[0], SKINNY_MAX_M)]
    return tuple(torch.cat(p) for p in zip(*parts))


@pytest.mark.parametrize("B", [300, 600])
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "x".join(map(str, c)))
def test_prior_tiled_equals_skinny_with_and_without_class_tables(cfg, B):
    """B >= 2 x classes: with the class tables on, the leading sources of a gated launch are read through arow on the table's rows and
    the launches on the batch continue a stored accumulator state; DVQ_PIXELCNN_TABLES=0 computes every row from zero.  Sample,
    forward and log_prob: the tiled kernels equal the small-batch kernels under either setting, and the two settings equal each other."""
    net = _prior(cfg)
    x, lab, q = _inputs(cfg, B)
    names = ("codes", "logits", "forward", "log_prob")
    outs = {}
    for tables in ("1", "0"):
        ref = _with_env("DVQ_PIXELCNN_TABLES", tables, lambda: _chunked(net, x, lab, q))
        assert all(bool(torch.isfinite(r).all()) for r in ref[1:])
        outs[tables] = ref
        for tn in TNS:
            got = _with_env("DVQ_PIXELCNN_TABLES", tables, lambda: _tiled(lambda: _prior_outputs(net, x, lab, q), tn))
            for n, r, t in zip(names, ref, got):
                assert torch.equal(r, t), f"tables {tables} tile {tn}: {n} on the tiled kernels != small-batch kernels"
        whole = _with_env("DVQ_PIXELCNN_TABLES", tables, lambda: _prior_outputs(net, x, lab, q))
        for n, r, t in zip(names, ref, whole):
            assert torch.equal(r, t), f"tables {tables}: {n} of the whole batch (launcher's own choice) != its chunks"
    for n, a, b in zip(names, outs["1"], outs["0"]):
        assert torch.equal(a, b), f"{n}: class tables on != off"
