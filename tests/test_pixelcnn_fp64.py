"""The gated PixelCNN prior against a float64 reference (tests/pixelcnn_ref.py) under trained-like weights.

Weights (``pixelcnn_ref.weights``), all from ``synth``'s Philox streams on top of ``synthetic_state_dict``:
  base       unchanged: the control (the goldens' weights at the goldens' seeds for the two golden sizes)
  hot        every class embedding ~ N(0, 3), every bias ~ N(0, 1), vert_stack / horiz_stack / vert_to_horiz weights times 4: gates
             saturate on both sides, the logits span about 30 at the full size
  dead       about 6 % of the rows of every weight (token and class embeddings included) exactly zero, for half of them the bias too:
             zero token embeddings and class rows, gate channels whose tanh or sigmoid half is constant, zero head rows, rows whose
             f16x2 scale comes from an absmax of 0.  output_conv.2 rows 3 (zero bias) and 5 (live bias) are always among them
  grow       every horiz_resid weight times 4: the residual stream grows with depth, logits reach about 28 at 15 layers
  gauge      base under an exact reparametrisation by powers of two that leaves the function unchanged: the residual stream's channel c
             times 2^k_c, k_c in -6 .. 10 (horiz_resid rows up, horiz_stack columns of layers >= 1 and output_conv.0 columns down), the
             head's hidden unit n times 2^k_n, k_n in -10 .. 10 (output_conv.0 rows up, output_conv.2 columns down), the token
             embedding's channel c times 2^k_c, k_c in -8 .. 8 (layer 0's two stacks' columns down).  Float64 reference and fp32 oracle
             are bit-identical to base's (asserted below), the device sees activations from 2^-8 to 2^10 per channel and weight columns
             of 16 octaves inside one f16x2 row scale
  gauge_far  gauge with the residual exponents 8 higher (2 .. 18): channels of the stream pass 65 520, the f16x2 forward returns
             non-finite logits under ``ops.no_range_check()`` (asserted), and the checked calls answer through their bf16x3 re-run

Tolerance.  There is no usable worst-case bound for this network (module docstring of pixelcnn_ref.py), so it comes from the reference
side, as in tests/test_mano.py: per case e32 = max |oracle32 - ref| over the compared logits, oracle32 being
``oracle.dvq_oracle.pixelcnn_forward`` in float32 on the CPU on the same weights, codes and labels.  The device may have FACTOR = 16 times
that: 4 x because the fp16 split keeps 22 of fp32's 24 significand bits, 4 x for an accumulation order and a tanhf / expf different from
torch's (the figure of tests/test_pointnet_fp64.py; reasoned, not measured).  A log-probability moves by at most twice the largest logit
error: 2 x 16 x e32.  The families themselves are held to e32 <= 2e-5 max(1, max |ref|) on the CPU, so that the tolerance stays sharp.

Sizes (n_in, dim, n_layers, n_classes): (32, 64, 3, 16) and (512, 512, 15, 128) are the goldens', (100, 64, 2, 8) has an n_in that is
no multiple of 32, (64, 128, 4, 8) a second width: a depth series of 2, 3, 4 and 15 layers.  Batches: the horizontal stack and the head
multiply B rows per position, the vertical stack 3 B rows per grid row, and csrc/gemm_f16x2.hip takes its skinny kernel up to
SKINNY_MAX_M = 256 rows and its 128-row tiles (TM) beyond: B = 1 (one row, served by the class tables), 40 (skinny kernels, 40 and 120
rows), 100 (horizontal rows skinny, 300 vertical rows tiled), 300 (tiled: 300 = 128 + 128 + 44, a ragged last tile).  The class tables
(csrc/pixelcnn.hip, make_plan) are the packer's own for fp16 planes and serve every batch size; a call builds them itself only from
B >= 2 n_classes on; DVQ_PIXELCNN_TABLES=0 evaluates per row (one case per family below).  At the full size beyond 40 rows the device
runs all rows and the reference and the oracle 32 of them: both ends of every 128-row block and rows spread between
(``pixelcnn_ref.rows_of``).  On a GPU the float64 reference runs as torch float64 on the device; the CPU group pins the same code.

Draws.  The device's code must win the reference's race argmax(logit - log q); where it does not, the reference's margin between its
winner and its runner-up must be <= 2 x 16 x e32 (and the device's code within that margin of the winner): such a draw is set aside and
later positions are still compared, since the reference is teacher-forced on the device's codes.  At most 5 % of the draws pooled over
a family's batches at one size may be set aside.

Not covered: grids other than 3 x 3 and batches beyond one 16 384-row chunk (both covered bitwise in tests/test_gpu_parity.py).
"""
import functools
import os

import pytest
import torch

import pixelcnn_ref as R
from dvqvae_amd import synth

DEV = "cuda:0"
FACTOR = 16.0                        # 4 (fp16 split: 22 of 24 bits) x 4 (accumulation order, tanhf / expf)
CONDITION = 2e-5                     # families: e32 <= CONDITION max(1, max |ref|)
CAP = 0.05                           # draws set aside per (family, size), pooled over the batches
BATCHES = (1, 40, 100, 300)
DRY_B = 16                           # oracle-only dry run of the draw rule: 144 draws per (family, size)
SIZES = tuple(R.SIZES)
SMALL = (32, 64, 3, 16)
F16_LIMIT = 65520.0
CASES = [(f, s, B) for f in R.FAMILIES for s in SIZES for B in BATCHES]
KIND_B = 40


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _oracle32(sd, x, label):
    from oracle import dvq_oracle as O
    return O.pixelcnn_forward({k: v.cpu() for k, v in sd.items()}, "", x.cpu(), label.cpu())


def _ratio(err, e32):
    return err / e32 if e32 > 0 else (0.0 if err == 0 else float("inf"))


def _noise(size, B):
    return synth.exp1_noise(B, 9, size[0], seed=7 * size[0] + B)


def _draws(codes, ref, q, tol):
    """codes [R, 9], ref / q [R, 9, n]: (draws set aside, draws off the reference beyond the margin, their first places)."""
    race = R.race(ref, q.to(ref.device))
    top = torch.topk(race, 2, dim=-1)
    lost = codes.to(ref.device) != top.indices[..., 0]
    margin = top.values[..., 0] - top.values[..., 1]
    behind = top.values[..., 0] - race.gather(-1, codes.to(ref.device)[..., None])[..., 0]
    aside = lost & (margin <= tol) & (behind <= tol)
    bad = lost & ~aside
    return int(aside.sum()), int(bad.sum()), bad.nonzero()[:4].tolist()


def _rows_last(logits):
    """[R, n, 3, 3] -> [R, 9, n]"""
    return logits.permute(0, 2, 3, 1).reshape(logits.shape[0], 9, logits.shape[1])


# ------------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("tag,size,atol", [("small", SMALL, 1e-5), ("full", R.FULL, 2e-5)])
def test_reference_reproduces_goldens(golden, tag, size, atol):
    """Pins the float64 reference to the real model's output, within the goldens' own tolerances."""
    g = golden("g4_pixelcnn")
    ref = R.forward(R.weights("base", size), torch.from_numpy(g[tag + "_x"]), torch.from_numpy(g[tag + "_label"]))
    assert float((ref - torch.from_numpy(g[tag + "_logits"]).double()).abs().max()) <= atol


@functools.lru_cache(maxsize=None)
def _cpu_case(family, size, B):
    """(reference, fp32 oracle, largest |residual stream|) on the compared rows of a case's random codes."""
    sd = R.weights(family, size)
    x, label = R.codes_and_labels(size, B)
    rows = R.rows_of(size, B)
    probe = {}
    ref = R.forward(sd, x[rows], label[rows], probe=probe)
    return ref, _oracle32(sd, x[rows], label[rows]), probe["stream"]


@pytest.mark.parametrize("size", SIZES, ids=_id)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_families_are_well_conditioned(family, size):
    """A condition on the families, not a measurement of the device: fp32 itself stays within 2e-5 max(1, max |ref|) of the reference."""
    for B in BATCHES:
        ref, o32, stream = _cpu_case(family, size, B)
        e32, big = float((o32.double() - ref).abs().max()), float(ref.abs().max())
        print(f"pcnn-e32 {family} {_id(size)} B{B}: e32 {e32:.3e} max |ref| {big:.3f} max |stream| {stream:.4g}")
        assert bool(torch.isfinite(ref).all()), f"B={B}: non-finite reference value"
        assert e32 <= CONDITION * max(1.0, big), f"B={B}: e32 {e32:.3e} > {CONDITION} x max(1, {big:.3f})"
        if family == "gauge":
            assert stream < F16_LIMIT, f"B={B}: family gauge is meant to stay inside fp16's range, stream reaches {stream:.4g}"
        if family == "gauge_far":
            assert stream > F16_LIMIT, f"B={B}: family gauge_far must pass fp16's range, stream reaches {stream:.4g}"


@pytest.mark.parametrize("size", SIZES, ids=_id)
@pytest.mark.parametrize("family", ("gauge", "gauge_far"))
def test_gauge_leaves_reference_and_oracle_unchanged(family, size):
    """The reparametrisation is exact: float64 reference and fp32 oracle are bit-identical to base's, so the reference does not move."""
    for B in BATCHES:
        ref, o32, _ = _cpu_case(family, size, B)
        ref0, o320, _ = _cpu_case("base", size, B)
        assert torch.equal(ref, ref0), f"B={B}: float64 reference moved by {float((ref - ref0).abs().max()):.3e}"
        assert torch.equal(o32, o320), f"B={B}: fp32 oracle moved by {float((o32 - o320).abs().max()):.3e}"


@pytest.mark.parametrize("size", SIZES, ids=_id)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_draw_rule_dry_run(family, size):
    """The draw rule of the gpu group with the fp32 oracle standing in for the device: the reference alone stays inside the cap."""
    from oracle import dvq_oracle as O
    sd = R.weights(family, size)
    _, label = R.codes_and_labels(size, DRY_B)
    q = _noise(size, DRY_B)
    codes = O.pixelcnn_generate(sd, "", label, q)
    ref = _rows_last(R.forward(sd, codes, label))
    e32 = float((_rows_last(_oracle32(sd, codes, label)).double() - ref).abs().max())
    aside, bad, where = _draws(codes.reshape(DRY_B, 9), ref, q, 2 * FACTOR * e32)
    print(f"pcnn-dry {family} {_id(size)}: e32 {e32:.3e}, set aside {aside} of {DRY_B * 9} draws")
    assert not bad, f"{bad} oracle draws off the reference beyond the margin, first (row, position) {where}"
    assert aside <= CAP * DRY_B * 9


# ------------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _net(family, size):
    from dvqvae_amd.network.pixelcnn.models import GatedPixelCNN
    sd = R.weights(family, size)
    net = GatedPixelCNN(*size)
    net.load_state_dict(sd, strict=True)
    return net.eval().to(DEV), sd, {k: v.to(DEV) for k, v in sd.items()}


def _compare(dev_rows, sd, sdd, x, label):
    """dev_rows [R, n, 3, 3] against the float64 reference (on the device) and the fp32 oracle (CPU) of the same rows."""
    ref = R.forward(sdd, x.to(DEV), label.to(DEV))
    e32 = float((_oracle32(sd, x, label).double().to(DEV) - ref).abs().max())
    err = (dev_rows.double() - ref).abs()
    err = float(err.max()) if bool(torch.isfinite(dev_rows).all()) else float("inf")
    return ref, e32, err


@functools.lru_cache(maxsize=None)
def _forward_case(family, size, B):
    """Teacher-forced logits of random codes: ``net(x, label)`` on all rows, compared on ``rows_of``."""
    net, sd, sdd = _net(family, size)
    x, label = R.codes_and_labels(size, B)
    rows = R.rows_of(size, B)
    logits = net(x.to(DEV), label.to(DEV))
    assert tuple(logits.shape) == (B, size[0], 3, 3)
    _, e32, err = _compare(logits[rows.to(DEV)], sd, sdd, x[rows], label[rows])
    return dict(logits=logits, e32=e32, err=err)


@functools.lru_cache(maxsize=None)
def _sample_case(family, size, B):
    """``net.generate`` on recorded noise and ``net.log_prob`` of its codes against the reference teacher-forced on those codes."""
    net, sd, sdd = _net(family, size)
    _, label = R.codes_and_labels(size, B)
    q = _noise(size, B)
    rows = R.rows_of(size, B)
    codes, slog = net.generate(None, label.to(DEV), batch_size=B, noise=q.to(DEV), return_logits=True)
    logp = net.log_prob(codes, label.to(DEV))
    assert tuple(codes.shape) == (B, 3, 3) and tuple(slog.shape) == (B, 9, size[0]) and tuple(logp.shape) == (B, 9)
    assert int(codes.min()) >= 0 and int(codes.max()) < size[0], "a drawn code is out of range"
    rd = rows.to(DEV)
    ref, e32, err = _compare(slog[rd].reshape(len(rows), 3, 3, -1).permute(0, 3, 1, 2), sd, sdd, codes[rd].cpu(), label[rows])
    ref = _rows_last(ref)
    c = codes[rd].reshape(len(rows), 9)
    aside, bad, where = _draws(c, ref, q[rows], 2 * FACTOR * e32)
    want = torch.log_softmax(ref, dim=-1).gather(-1, c[..., None])[..., 0]
    lp_err = float((logp[rd].double() - want).abs().max()) if bool(torch.isfinite(logp).all()) else float("inf")
    return dict(slog=slog, e32=e32, err=err, aside=aside, bad=bad, where=where, draws=c.numel(), lp_err=lp_err)


def _check(what, family, size, B, err, e32, factor=FACTOR):
    print(f"pcnn-ratio {what} {family} {_id(size)} B{B}: err {err:.3e} e32 {e32:.3e} ratio {_ratio(err, e32):.2f}")
    assert err <= factor * e32, f"{what}: device error {err:.3e} > {factor:g} x e32 = {factor * e32:.3e} ({_ratio(err, e32):.1f} x e32)"


@pytest.mark.gpu
@pytest.mark.parametrize("family,size,B", CASES, ids=_id)
def test_logits_against_float64(family, size, B):
    r = _forward_case(family, size, B)
    kind = os.environ.get("DVQ_GEMM")
    _check(f"forward[{kind}]" if kind else "forward", family, size, B, r["err"], r["e32"])


@pytest.mark.gpu
@pytest.mark.parametrize("family,size,B", CASES, ids=_id)
def test_sampler_logits_against_float64(family, size, B):
    """The cached sampler against the truth directly, not through its bitwise equality with the forward."""
    r = _sample_case(family, size, B)
    _check("sampler", family, size, B, r["err"], r["e32"])


@pytest.mark.gpu
@pytest.mark.parametrize("family,size,B", CASES, ids=_id)
def test_log_prob_against_float64(family, size, B):
    r = _sample_case(family, size, B)
    _check("logprob", family, size, B, r["lp_err"], r["e32"], 2 * FACTOR)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=_id)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_draws_win_the_reference_race(family, size):
    aside = draws = 0
    bad = []
    for B in BATCHES:
        r = _sample_case(family, size, B)
        aside, draws = aside + r["aside"], draws + r["draws"]
        if r["bad"]:
            bad.append(f"B={B}: {r['bad']} draws off the reference beyond 2 x 16 x e32, first (row, position) {r['where']}")
    print(f"pcnn-draws {family} {_id(size)}: set aside {aside} of {draws} ({aside / draws:.4f})")
    assert not bad, "\n".join(bad)
    assert aside <= CAP * draws, f"{aside} of {draws} draws set aside"


KIND_SELECT = "test_logits_against_float64 and (" + " or ".join(f"{_id(s)}-{KIND_B}]" for s in (SMALL, R.FULL)) + ")"


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("bf16x3", "fp32"))
def test_other_gemm_kinds(kind):
    """The GEMM kind is chosen when the library loads: a fresh process runs the B = 40 cases of test_logits_against_float64 at one
    reduced size and the full size on it.  No worse than the default: the same bound."""
    import subprocess
    import sys
    env = dict(os.environ, DVQ_GEMM=kind)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-k", KIND_SELECT,
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
    print("\n".join(ln[ln.index("pcnn-ratio"):] for ln in r.stdout.splitlines() if "pcnn-ratio" in ln))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{2 * len(R.FAMILIES)} passed" in r.stdout, r.stdout[-1000:]


@pytest.mark.gpu
@pytest.mark.parametrize("size,B", [(SMALL, 100), (R.FULL, 40)], ids=_id)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_per_row_evaluation_without_class_tables(family, size, B):
    """DVQ_PIXELCNN_TABLES=0: row 0 and position (0, 0) evaluated per row instead of read through the label.  The packer's tables
    serve every batch size, so this knob is the only way onto the per-row path: at a reduced size and at the product's."""
    from test_gpu_parity import _with_env
    f = _with_env("DVQ_PIXELCNN_TABLES", "0", lambda: _forward_case.__wrapped__(family, size, B))
    _check("forward[tables=0]", family, size, B, f["err"], f["e32"])
    s = _with_env("DVQ_PIXELCNN_TABLES", "0", lambda: _sample_case.__wrapped__(family, size, B))
    _check("sampler[tables=0]", family, size, B, s["err"], s["e32"])
    _check("logprob[tables=0]", family, size, B, s["lp_err"], s["e32"], 2 * FACTOR)
    assert not s["bad"], f"{s['bad']} draws off the reference beyond the margin, first (row, position) {s['where']}"


@pytest.mark.gpu
@pytest.mark.parametrize("size", (SMALL, (64, 128, 4, 8)), ids=_id)
def test_gauge_far_given_codes_return_finite_logits(size):
    """Given codes raise no flag where their logits are NaN: the op itself must notice, also when only the logits are asked for.
    Even rows are given whole, odd rows from position 5 on are drawn again from the same noise: the codes are those of the plain
    sampler, the logits are finite and within the tolerance of the reference; then the even rows alone, without noise."""
    B = 40
    net, sd, sdd = _net("gauge_far", size)
    _, label = R.codes_and_labels(size, B)
    q = _noise(size, B).to(DEV)
    codes, _ = net.generate(None, label.to(DEV), batch_size=B, noise=q, return_logits=True)
    given = codes.reshape(B, 9).clone()
    given[1::2, 5:] = -1
    c2, lg2 = net.generate(None, label.to(DEV), batch_size=B, noise=q, given=given, return_logits=True)
    assert torch.equal(c2, codes), "given + redrawn codes differ from the plain sampler's"
    _, e32, err = _compare(lg2.reshape(B, 3, 3, -1).permute(0, 3, 1, 2), sd, sdd, codes.cpu(), label)
    _check("sampler[given]", "gauge_far", size, B, err, e32)
    even = torch.arange(0, B, 2)
    c3, lg3 = net.generate(None, label[even].to(DEV), batch_size=len(even), noise=None, given=given[even.to(DEV)].contiguous(),
                           return_logits=True)
    assert torch.equal(c3, codes[even.to(DEV)])
    _, e32, err = _compare(lg3.reshape(len(even), 3, 3, -1).permute(0, 3, 1, 2), sd, sdd, codes[even.to(DEV)].cpu(), label[even])
    _check("sampler[all given]", "gauge_far", size, len(even), err, e32)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=_id)
def test_dead_head_rows_are_exact(size):
    """A logit whose output_conv.2 row and bias are zero is exactly 0.0; one whose row is zero under a live bias is that bias."""
    _, sd, _ = _net("dead", size)
    zero, live = R.dead_head_rows(sd)
    assert len(zero) >= 1 and len(live) >= 1
    bias = sd["output_conv.2.bias"][live].to(DEV)
    for B in BATCHES:
        lg = _forward_case("dead", size, B)["logits"]                      # [B, n, 3, 3]
        sl = _sample_case("dead", size, B)["slog"]                         # [B, 9, n]
        assert bool((lg[:, zero.to(DEV)] == 0).all()) and bool((sl[:, :, zero.to(DEV)] == 0).all()), f"B={B}: a dead logit is not 0.0"
        assert torch.equal(lg[:, live.to(DEV)], bias[None, :, None, None].expand(B, -1, 3, 3)), f"B={B}: forward: dead row != its bias"
        assert torch.equal(sl[:, :, live.to(DEV)], bias[None, None, :].expand(B, 9, -1)), f"B={B}: sampler: dead row != its bias"


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=_id)
def test_gauge_far_bites(size):
    """The case is what it claims: without the range check the fp16 split returns non-finite logits for family gauge_far (and finite
    ones for gauge), so the checked calls of the tests above went through their bf16x3 re-run."""
    from dvqvae_amd import _lib, ops, packing
    f16 = packing.gemm_kind() == _lib.PLANES_F16X2          # the other kinds have fp32's range: everything stays finite
    for B in BATCHES:
        x, label = R.codes_and_labels(size, B)
        with ops.no_range_check():
            far = _net("gauge_far", size)[0](x.to(DEV), label.to(DEV))
            near = _net("gauge", size)[0](x.to(DEV), label.to(DEV))
        assert bool(torch.isfinite(far).all()) != f16, f"B={B}: gauge_far stays inside fp16's range on the device"
        assert bool(torch.isfinite(near).all()), f"B={B}: gauge leaves fp16's range on the device"
        assert bool(torch.isfinite(_forward_case("gauge_far", size, B)["logits"]).all())
