"""The PointNet encoder against a float64 reference (tests/pointnet_ref.py) under trained-like weights and clouds of several kinds.

Weights (``pointnet_ref.weights``), all from ``synth``'s Philox streams on top of ``synthetic_state_dict``:
  base    unchanged: the control (the goldens' weights)
  wide    every BatchNorm: running_var log-uniform in [1e-4, 1e2], gamma ~ N(0, 1), running_mean and beta ~ N(0, 0.5)
  dead    wide, gamma exactly 0 on about 6 % of every BatchNorm's channels (zero conv1 / conv3 rows, constant conv2 channels), and one
          conv3 row with a single non-zero weight
  rows    base, every conv / fc weight row times 2^k, k uniform in -6 .. 6
  sparse  base, conv1's BatchNorm beta = -3 |folded row|_1 max|x|: every conv1 activation of every point is zero (|w.x| <= |w|_1 max|x|),
          the conv2 rows are one constant row, the centred rows are zero and all points tie in every channel
Clouds (``pointnet_ref.clouds``): offset (``synth.synthetic_clouds``), unit (centred, times 10), two (two points alternating), line.

One number per case: the error ratio u = max |y - ref| / S with S the reference's condition scale.  ``golden/pointnet_u32.json`` records
the fp32 oracle's own u per family (CPU tests below); the device may have 16 times that: conv2's fp16 split keeps 22 of fp32's 24
significand bits (4 x), and another 4 x allows for an accumulation order different from torch's.  Never above 4e-6, the constant of the
GEMM fuzz.  The feature is compared with the reference run on the DEVICE's transforms, so an STN difference does not compound.

Not covered: the STN trunk's own 1 024 features (only the transforms leave the library), so the "feature of a zero row is its folded
bias" check of family dead is made on the main trunk.  Family sparse ties all points by construction and is, like the two-point and
line clouds, outside the argmax test's gap rule; the bitwise three-way test covers it.

Measured on the MI355X (u / u32 of the family, maximum over cloud kinds, N, C and the four paths; feat, trans): base 1.12, 3.98;
wide 1.00, 2.61; dead 1.50, 5.19; rows 0.86, 3.80; sparse 0.89, 3.49 -- against the 16 allowed (table by path: DESIGN 3.3, "measured
kernel error ratio").  What the tests found: family dead, fault counters (0, 127) per cloud -- a zero conv3 row has E_t = 0 and its
records' interval did not cover the id bits of a zero score (fixed: E_ID_FLOOR in csrc/pointnet_filter.hip).
"""
import functools
import json
import os

import pytest
import torch

from conftest import GOLDEN, SEED
import pointnet_ref as R
from dvqvae_amd import synth

DEV = "cuda:0"
U32_FILE = os.path.join(GOLDEN, "pointnet_u32.json")
CEILING = 4e-6                       # the GEMM fuzz's constant: |err| <= 4e-6 sum |a| |w|
FACTOR = 16.0                        # 4 (fp16 split: 22 of 24 bits) x 4 (accumulation order)
CAP = 0.10                           # argmax test: channels the gap rule may set aside per case
CPU_SHAPES = ((3, 1), (3, 40), (3, 257), (3, 778))          # (B, N) of the recorded oracle ratios
GPU_B, GPU_NS = 5, (1, 40, 257, 778, 1030)                  # one point; a padded tile; a tile + tail; MANO; four tiles + 6 points
PATHS = {"default": {"DVQ_PN_FILTER": None, "DVQ_PN_RECOMPUTE": None},
         "filter2": {"DVQ_PN_FILTER": "2", "DVQ_PN_RECOMPUTE": None},
         "filter0": {"DVQ_PN_FILTER": "0", "DVQ_PN_RECOMPUTE": None},
         "filter2_spill": {"DVQ_PN_FILTER": "2", "DVQ_PN_RECOMPUTE": "0"}}
CASES = [(f, k, C) for f in R.FAMILIES for k in R.KINDS for C in (3, 4)]
GAP_CASES = [(f, k, C) for f, k, C in CASES if k in ("offset", "unit") and f != "sparse"]


def _cloud_seed(N, C):
    return 700 + N + C


def _inputs(family, kind, C, B, N):
    x = R.clouds(kind, B, N, C, seed=_cloud_seed(N, C))
    return x, R.weights(family, C, xmax=float(x.abs().max()))


def _u32():
    with open(U32_FILE) as f:
        return json.load(f)


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("C,N,B", [(4, 64, 4), (4, 1024, 1), (4, 1024, 4), (4, 3000, 1), (3, 778, 4), (3, 100, 2)])
def test_reference_reproduces_goldens(golden, C, N, B):
    """Pins the float64 reference to the real reference's output, within the goldens' own 1e-5."""
    g = golden("g1_pointnet")
    sd = R.weights("base", C, seed=SEED)
    x = synth.synthetic_clouds(B, N, seed=100 + N, channels=C)
    tag = f"C{C}_N{N}_B{B}"
    t = R.stn(sd, x)
    f = R.encode(sd, x)
    assert float((t.value - torch.from_numpy(g[tag + "_trans"]).double()).abs().max()) <= 1e-5
    assert float((f.value - torch.from_numpy(g[tag + "_feat"]).double()).abs().max()) <= 1e-5


@functools.lru_cache(maxsize=None)
def _oracle_ratios(family):
    """The fp32 oracle against the float64 reference: (max u(feat), max u(trans), largest |reference value|, worst share of channels
    the argmax test's gap rule would set aside with the committed ratios) over cloud kinds, C and CPU_SHAPES."""
    from oracle import dvq_oracle as O
    uf = ut = big = aside = 0.0
    try:
        recorded = _u32()[family]["feat"]
    except (OSError, KeyError):
        recorded = None              # first generation of the file
    for kind in R.KINDS:
        for C in (3, 4):
            for B, N in CPU_SHAPES:
                x, sd = _inputs(family, kind, C, B, N)
                of, ot = O.pointnet_encode(sd, "", x)
                rt, rf = R.stn(sd, x), R.encode(sd, x, trans=ot)
                uf, ut = max(uf, R.error_ratio(of, rf)), max(ut, R.error_ratio(ot, rt))
                vals = torch.cat([rt.value.reshape(-1), rf.value.reshape(-1)])
                big = max(big, float(vals.abs().max())) if bool(torch.isfinite(vals).all()) else float("inf")
                if recorded is not None and (family, kind, C) in GAP_CASES:
                    own = R.encode(sd, x, trans=rt.value)
                    aside = max(aside, float((own.gap <= 2 * FACTOR * recorded * own.S).double().mean()))
    return uf, ut, big, aside


@pytest.mark.parametrize("family", R.FAMILIES)
def test_oracle_error_ratio(family):
    uf, ut, big, aside = _oracle_ratios(family)
    print(f"pn64 oracle {family}: u32 feat {uf:.3e} trans {ut:.3e}, max |ref| {big:.3e}, set aside by the gap rule {aside:.3f}")
    assert big < 1e30, "a reference value is too close to fp32's range (or not finite)"
    assert uf < CEILING and ut < CEILING
    assert aside <= CAP, "the reference alone sets too many channels aside for the argmax test"


@pytest.mark.parametrize("family", R.FAMILIES)
def test_recorded_ratios_reproduce(family):
    """golden/pointnet_u32.json is what the test above measures, within a factor of 2 (torch's summation order varies between builds).
    Regenerate with ``python tests/test_pointnet_fp64.py``."""
    uf, ut, _, _ = _oracle_ratios(family)
    rec = _u32()[family]
    assert rec["feat"] / 2 <= uf <= rec["feat"] * 2, (uf, rec)
    assert rec["trans"] / 2 <= ut <= rec["trans"] * 2, (ut, rec)


# ------------------------------------------------------------------------------------------------------------------- GPU
def _net(sd, C):
    from dvqvae_amd.network.pointnet_encoder import PointNetEncoder
    net = PointNetEncoder(channel=C)
    net.load_state_dict(sd, strict=True)
    return net.eval().to(DEV)


def _run(net, x, env):
    """(features, transforms, fault counters) of one pass; env: knob -> value, None = unset."""
    from dvqvae_amd import _lib, ops
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.load().dvq_reload_env()
        ops.pointnet_fault_counters(reset=True)
        feat, trans, _ = net(x)
        torch.cuda.synchronize()
        return feat, trans, tuple(ops.pointnet_fault_counters(reset=True))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _lib.load().dvq_reload_env()


@functools.lru_cache(maxsize=None)
def _device_case(family, kind, C):
    """Every path and N of one (family, cloud kind, C): a list of records with the error ratios, the counters and the argmax figures.
    The float64 reference runs on the device (torch float64); the STN reference once per N, shared by the paths."""
    u32 = _u32()[family]
    out = []
    for N in GPU_NS:
        x, sd = _inputs(family, kind, C, GPU_B, N)
        net, xd = _net(sd, C), x.to(DEV)
        sdd = {k: v.to(DEV) for k, v in sd.items()}
        rt = R.stn(sdd, xd)
        for path, env in PATHS.items():
            feat, trans, counters = _run(net, xd, env)
            rf = R.encode(sdd, xd, trans=trans)
            m = 2 * FACTOR * u32["feat"] * rf.S
            clear = rf.gap > m
            off = ((feat.double() - rf.value).abs() > m) & clear
            out.append(dict(N=N, path=path, u_feat=R.error_ratio(feat, rf), u_trans=R.error_ratio(trans, rt), counters=counters,
                            finite=bool(torch.isfinite(feat).all() and torch.isfinite(trans).all()),
                            aside=float((~clear).double().mean()), off=int(off.sum()), off_at=off.nonzero()[:4].tolist()))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("family,kind,C", CASES)
def test_accuracy_against_float64(family, kind, C):
    u32, bad = _u32()[family], []
    for r in _device_case(family, kind, C):
        print(f"pn64 device {family} {kind} C{C} N{r['N']} {r['path']}: u feat {r['u_feat']:.3e} ({r['u_feat'] / u32['feat']:.2f} x u32) "
              f"trans {r['u_trans']:.3e} ({r['u_trans'] / u32['trans']:.2f} x u32) counters {r['counters']}")
        where = f"N={r['N']} {r['path']}"
        if not r["finite"]:
            bad.append(f"{where}: non-finite output")
        if r["counters"] != (0, 0):
            bad.append(f"{where}: fault counters {r['counters']}")
        for what in ("feat", "trans"):
            u = r["u_" + what]
            if not u <= FACTOR * u32[what]:
                bad.append(f"{where}: u({what}) = {u:.3e} > 16 x {u32[what]:.3e}")
            if not u <= CEILING:
                bad.append(f"{where}: u({what}) = {u:.3e} > {CEILING}")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("family,kind,C", GAP_CASES)
def test_argmax_faithful(family, kind, C):
    """Where the float64 top-two gap over the points exceeds 2 x 16 u32 S, the device's feature lies within that margin of the
    reference's maximum: it is not the runner-up.  At most 10 % of a case's channels may fall under the gap rule."""
    bad = []
    for r in _device_case(family, kind, C):
        print(f"pn64 argmax {family} {kind} C{C} N{r['N']} {r['path']}: set aside {r['aside']:.3f}, off the maximum {r['off']}")
        if r["off"]:
            bad.append(f"N={r['N']} {r['path']}: {r['off']} features off the reference maximum, first (cloud, channel) {r['off_at']}")
        if r["aside"] > CAP:
            bad.append(f"N={r['N']} {r['path']}: {r['aside']:.3f} of the channels set aside by the gap rule")
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("family,kind,C", CASES)
def test_filter_guarantee(family, kind, C):
    """Filtered trunk: DVQ_PN_FILTER=2 alone == with DVQ_PN_EXHAUSTIVE=1 == with DVQ_PN_RECOMPUTE=0, bitwise, over poisoned scratch rows,
    counters zero.  Family dead: a zero conv3 row's feature is its folded bias."""
    import test_pointnet_exact_recompute_gpu as RC
    for N in GPU_NS:
        x, sd = _inputs(family, kind, C, GPU_B, N)
        net, xd = _net(sd, C), x.to(DEV)
        f, t = RC._three_ways(net, xd)
        f0, t0, c0 = RC._run(net, xd)
        assert RC._same(f, f0) and RC._same(t, t0), f"N={N}: DVQ_PN_FILTER=2 alone differs from the three-way result"
        assert c0 == (0, 0), (N, c0)
        assert torch.isfinite(f).all() and torch.isfinite(t).all(), f"N={N}: non-finite output"
        if family == "dead":
            dead = R.dead_channels(sd, "bn3")
            assert 30 <= len(dead) <= 100, len(dead)
            fold = sd["bn3.bias"].double()[dead]            # (b - mean) * 0 / sqrt(var + eps) + beta
            torch.testing.assert_close(f[:, dead].double().cpu(), fold.expand(GPU_B, -1), rtol=1e-6, atol=0.0,
                                       msg=lambda s: f"N={N}: zero conv3 rows' features are not their folded bias\n{s}")


if __name__ == "__main__":           # regenerate golden/pointnet_u32.json
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    table = {}
    for fam in R.FAMILIES:
        uf, ut, big, _ = _oracle_ratios(fam)
        assert big < 1e30 and uf < CEILING and ut < CEILING, (fam, uf, ut, big)
        table[fam] = {"feat": uf, "trans": ut}
    with open(U32_FILE, "w") as fh:
        json.dump(table, fh, indent=1)
        fh.write("\n")
    print(json.dumps(table, indent=1))
