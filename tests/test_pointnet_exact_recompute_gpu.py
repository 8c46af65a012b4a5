"""GPU check of the exact stage's on-demand conv2 rows (DVQ_PN_RECOMPUTE): with the knob on, pn_trunk_filter_kernel spills no
row and pn_exact_kernel produces the rows it reads with the trunk's own conv1 / conv2 code.  Every case compares the encoder's
features and STN transforms (the STN trunk: no input transform, ReLU head; the main trunk: transform, no ReLU) with recompute on
against recompute off (spilled rows) and against the exhaustive evaluation (DVQ_PN_EXHAUSTIVE=1, always on spilled rows), BITWISE,
with both run-time consistency counters at zero.  Before every recompute run the scratch rows are overwritten with the rows of OTHER
clouds (a spill pass on different inputs): a row the exact stage failed to produce would be read as a wrong one, not as a stale right one."""
import os

import pytest
import torch

from dvqvae_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _encoder(C):
    from dvqvae_amd.network.pointnet_encoder import PointNetEncoder
    from util import load_synth
    net = PointNetEncoder(channel=C)
    load_synth(net, 50 + C)
    return net.eval().to(DEV)


def _run(net, x, **env):
    """(features, STN transforms, fault counters) of one pass with library knobs set."""
    from dvqvae_amd import _lib, ops
    env = dict({"DVQ_PN_FILTER": "2"}, **env)
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


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Bitwise equality (a NaN equals the same NaN)."""
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _three_ways(net, x, **env):
    """recompute on (over poisoned scratch rows) == recompute off == exhaustive, counters zero; returns the recompute-on result."""
    poison = torch.nan_to_num(torch.roll(x, 1, dims=2).flip(0)) * 1.25 + 0.01
    _run(net, poison, DVQ_PN_RECOMPUTE="0", **env)
    f_on, t_on, c_on = _run(net, x, DVQ_PN_RECOMPUTE="1", **env)
    f_off, t_off, c_off = _run(net, x, DVQ_PN_RECOMPUTE="0", **env)
    f_all, t_all, c_all = _run(net, x, DVQ_PN_RECOMPUTE="1", DVQ_PN_EXHAUSTIVE="1", **env)
    assert _same(t_on, t_off), "STN trunk: recomputed rows != spilled rows"
    bad = (_bits(f_on) != _bits(f_off)).nonzero()[:6].tolist()
    assert _same(f_on, f_off), f"main trunk: recomputed rows != spilled rows at (cloud, channel) {bad}"
    assert _same(t_on, t_all), "STN trunk: recompute != exhaustive"
    bad = (_bits(f_on) != _bits(f_all)).nonzero()[:6].tolist()
    assert _same(f_on, f_all), f"main trunk: recompute != exhaustive at (cloud, channel) {bad}"
    assert c_on == (0, 0) and c_off == (0, 0) and c_all == (0, 0), (c_on, c_off, c_all)
    return f_on, t_on


# N = 1 024: four full tiles; 778: three tiles + the tail tile; 40: one tile, mostly padding slots that repeat points; 3 000: twelve
# tiles, points 1 024 apart share a slot range of the point sort
@pytest.mark.parametrize("C,N,B", [(4, 1024, 5), (3, 778, 5), (3, 40, 3), (4, 40, 3), (4, 3000, 3)])
def test_recomputed_rows_equal_spilled_rows(C, N, B):
    net = _encoder(C)
    x = synth.synthetic_clouds(B, N, seed=300 + N + C, channels=C).to(DEV)
    f, _ = _three_ways(net, x)
    assert torch.isfinite(f).all()


@pytest.mark.parametrize("C,N", [(3, 512), (4, 778)])
def test_recompute_cloud_of_equal_points(C, N):
    """All points equal: every score of a channel ties, every group is flagged, the lists overflow -- the "everything" path, which
    produces every row of the cloud."""
    net = _encoder(C)
    x = synth.synthetic_clouds(3, N, seed=410 + N, channels=C).clone()
    x[1] = x[1, :, :1]
    f, _ = _three_ways(net, x.contiguous().to(DEV))
    assert torch.isfinite(f).all()


def test_recompute_nan_cloud_next_to_healthy_clouds():
    """One NaN coordinate: that cloud's features are NaN (the exact stage returns before it needs a row), its neighbours' are what
    they are without it."""
    C, N = 4, 778
    net = _encoder(C)
    x = synth.synthetic_clouds(3, N, seed=520, channels=C).clone()
    healthy = x.clone()
    x[1, 1, 5] = float("nan")
    f, t = _three_ways(net, x.contiguous().to(DEV))
    f_ok, t_ok, c_ok = _run(net, healthy.to(DEV), DVQ_PN_RECOMPUTE="1")
    assert torch.isnan(f[1]).all() and torch.isfinite(f[[0, 2]]).all()
    assert _same(f[[0, 2]], f_ok[[0, 2]]) and _same(t[[0, 2]], t_ok[[0, 2]]), "a NaN cloud changed its neighbours"
    assert c_ok == (0, 0)


def test_recompute_two_streams_equal_one_stream():
    """9 000 clouds of 64 points: the smallest batch that takes more than one launch, so the exact stage of a launch (which now reads
    the launch's clouds and transforms) runs on the second stream beside the next launch's trunk kernel."""
    C, N, B = 4, 64, 9000
    net = _encoder(C)
    x = synth.synthetic_clouds(B, N, seed=630, channels=C).to(DEV)
    f2, t2 = _three_ways(net, x)
    f1, t1, c1 = _run(net, x, DVQ_PN_RECOMPUTE="1", DVQ_PN_STREAMS="0")
    assert _same(t2, t1) and _same(f2, f1), "two streams != one stream"
    assert c1 == (0, 0)
    assert torch.isfinite(f2).all()
