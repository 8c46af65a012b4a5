"""The tiled fp16-plane GEMM kernel (csrc/gemm_f16x2.hip, gemm_f16x2_pp_kernel) around its K loop: the prologue that stages the first
three K-tiles, the accumulator state it may start from, and the epilogues.  A wave whose 64 x 64 block lies inside the output loads
every operand before its first store; blocks on a ragged edge, and rows that are not 16-byte multiples, keep the block-by-block code.

Yardstick: the small-batch ("skinny") kernels, which serve M <= 256 by default and issue the same MFMA sequence and the same
arithmetic per element.  DVQ_GEMM_SKINNY=0 forces the tiled kernel on the same inputs; every comparison is torch.equal.
Shapes: M = 64 / 65 / 129 / 200 put whole and ragged 64-row wave blocks side by side, N = 260 ends in a ragged column tile, N = 258
is not a multiple of four (4-byte path), K = 32 .. 160 is one to five K-tiles, and the two-source cases end a source inside the
three tiles of the prologue."""
import pytest
import torch

from util import load_synth
from dvqvae_amd import ops, packing, synth
from test_gpu_parity import _with_env

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (128, 256, 260, 258, 512)
KS = ((32,), (64,), (96,), (160,), (32, 64), (64, 32))


def _tiled(fn, tn):
    """fn() on the tiled kernel with its 128 x 128 (tn = "128") or 128 x 256 (tn = "256") tile: the launcher's own choice between the two
    takes the wide one only from a few thousand rows on."""
    return _with_env("DVQ_GEMM_SKINNY", "0", lambda: _with_env("DVQ_GEMM_TN", tn, fn))


TNS = ("128", "256")


def _linear_cases(M):
    out = {}
    for N in NS:
        for ks in KS:
            g = torch.Generator().manual_seed(M * 100003 + N * 17 + sum(ks) + len(ks))
            xs = [torch.randn(M, k, generator=g).to(DEV) for k in ks]
            ws = [(torch.randn(N, k, generator=g) * 0.05).to(DEV) for k in ks]
            b = torch.randn(N, generator=g).to(DEV)
            pls = packing.split_f16x2(ws)
            hot = [x.clone() for x in xs]
            hot[-1][M // 2, 3] = 7.0e4                      # beyond fp16: this row, and only this row, must come out NaN
            for bias in (b, None):
                for relu in (False, True):
                    key = f"N{N} K{ks} bias{bias is not None} relu{relu}"
                    if len(ks) == 1:
                        out[key] = ops.linear(xs[0], ws[0], bias, relu=relu, planes=pls[0])
                    else:
                        out[key] = ops.linear_multi(list(zip(xs, ws)), bias, relu=relu, planes=pls)
                    with ops.no_range_check():              # ops.linear would run a NaN result again on the six-product images
                        out[key + " hot"] = ops.linear_multi(list(zip(hot, ws)), bias, relu=relu, planes=pls)
    return out


@pytest.mark.parametrize("M", [1, 17, 64, 65, 129, 200])
def test_linear_tiled_equals_skinny(M):
    """Bias / no bias, ReLU on / off, one and two sources, T = 1, 2, 3, 5 K-tiles, ragged and 4-byte widths; and the NaN row of an
    out-of-range activation, which must leave every other row as it was."""
    ref = _linear_cases(M)
    assert len(ref) == len(NS) * len(KS) * 4 * 2
    hot_row = M // 2
    others = [i for i in range(M) if i != hot_row]
    for tn in TNS:
        got = _tiled(lambda: _linear_cases(M), tn)
        for key, r in ref.items():
            assert torch.equal(r.nan_to_num(nan=-7.0), got[key].nan_to_num(nan=-7.0)), f"M={M} tile {tn} {key}: tiled kernel != skinny kernel"
        for key, t in got.items():
            if key.endswith(" hot"):
                assert bool(torch.isnan(t[hot_row]).all()), f"M={M} tile {tn} {key}: the out-of-range row is not all NaN"
                assert torch.equal(t[others], got[key[:-4]][others]), f"M={M} tile {tn} {key}: the out-of-range row changed other rows"
            else:
                assert bool(torch.isfinite(t).all()), f"M={M} tile {tn} {key}"


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


CFGS = [(32, 64, 3, 16), (64, 128, 4, 8)]


@pytest.mark.parametrize("B", [37, 200])
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "x".join(map(str, c)))
def test_pixelcnn_forward_tiled_equals_skinny_and_rows(cfg, B):
    """Residual, gate, pre-gate output and class rows: the teacher-forced logits on the tiled kernels equal the default run, and
    the batch equals its rows run one by one."""
    net = _prior(cfg)
    pk = net.packed()
    x, lab, _ = _inputs(cfg, B)
    ref = ops.pixelcnn_forward(pk, x, lab)
    assert bool(torch.isfinite(ref).all())
    rows = torch.cat([ops.pixelcnn_forward(pk, x[i:i + 1], lab[i:i + 1]) for i in range(B)])
    for tn in TNS:
        got = _tiled(lambda: ops.pixelcnn_forward(pk, x, lab), tn)
        assert torch.equal(ref, got), f"tile {tn}: tiled kernels != default run"
        assert torch.equal(rows, got), f"tile {tn}: batch on the tiled kernels != its rows one by one"


@pytest.mark.parametrize("B", [40, 200])
@pytest.mark.parametrize("cfg", CFGS, ids=lambda c: "x".join(map(str, c)))
def test_pixelcnn_sample_tiled_equals_skinny_and_rows(cfg, B):
    """The sampler with fixed noise: codes and the logits they were drawn from."""
    net = _prior(cfg)
    pk = net.packed()
    _, lab, q = _inputs(cfg, B)
    rc, rl = ops.pixelcnn_sample(pk, lab, q, return_logits=True)
    one = [ops.pixelcnn_sample(pk, lab[i:i + 1], q[i:i + 1].contiguous(), return_logits=True) for i in range(B)]
    for tn in TNS:
        gc, gl = _tiled(lambda: ops.pixelcnn_sample(pk, lab, q, return_logits=True), tn)
        assert torch.equal(rc, gc) and torch.equal(rl, gl), f"tile {tn}: tiled kernels != default run"
        assert torch.equal(torch.cat([c for c, _ in one]), gc) and torch.equal(torch.cat([l for _, l in one]), gl), \
            f"tile {tn}: batch on the tiled kernels != its rows one by one"


@pytest.mark.parametrize("cfg", [(32, 64, 3, 16), (64, 128, 4, 16)], ids=lambda c: "x".join(map(str, c)))
def test_accumulator_state_equals_per_row_evaluation(cfg):
    """B = 300 >= 2 x 16 classes: the class tables are on and the tiled gated launches continue a stored accumulator state (two
    whole 128-row tiles and a ragged one).  DVQ_PIXELCNN_TABLES=0 computes every row from zero: the same codes and logits."""
    B = 300
    net = _prior(cfg)
    pk = net.packed()
    _, lab, q = _inputs(cfg, B)
    ac, al = ops.pixelcnn_sample(pk, lab, q, return_logits=True)
    bc, bl = _with_env("DVQ_PIXELCNN_TABLES", "0", lambda: ops.pixelcnn_sample(pk, lab, q, return_logits=True))
    assert bool(torch.isfinite(al).all())
    assert torch.equal(ac, bc) and torch.equal(al, bl), "accumulator state != per-row evaluation"
