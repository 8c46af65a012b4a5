"""Controls on the prior's draw -- temperature, top-k, given codes, log-probabilities (include/dvq.h: dvq_pixelcnn_sample_ctl,
DESIGN.md 3.4) -- against their float64 restatement (tests/prior_controls_ref.py), and the invariants GenNet.gen and the entry
points keep under them.  Bounds: codes equal except rows whose two best race scores lie within a relative 1e-4 (at most 0.1 % of
the rows); every drawn code inside the restatement's kept set; log-probabilities within 1e-5 absolute (the project's parity bar)."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import SEED
from util import load_synth
from dvqvae_amd import _lib, generate, ops, synth
from oracle import dvq_oracle as O
import prior_controls_ref as R

DEV = "cuda:0"
TOL = 1e-5
GAP, SET_ASIDE_CAP = 1e-4, 1e-3


# ------------------------------------------------------------------------------------------ no GPU
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_three_flags(dataset):
    p = generate.build_parser(dataset)
    a = p.parse_args([])
    assert a.temperature == 1.0 and a.top_k == 0 and a.log_prob == 0
    a = p.parse_args(["--temperature", "0.8", "--top_k", "40", "--log_prob", "1"])
    assert a.temperature == 0.8 and a.top_k == 40 and a.log_prob == 1
    assert generate._prior_controls(1.0, 0, False) == {}, "flags at their defaults: the call names no control"
    assert generate._prior_controls(0.8, 40, True) == dict(temperature=0.8, top_k=40, log_prob=True, return_aux=True)


def test_abi_10_gains_the_controlled_sampler():
    assert _lib.ABI_VERSION == 10
    assert "dvq_pixelcnn_sample_ctl" in _lib.SIGNATURES and "dvq_pixelcnn_sample" in _lib.SIGNATURES
    header = open(_lib.HEADER).read()
    assert "int dvq_pixelcnn_sample_ctl(" in header and "} dvq_pixelcnn_ctl;" in header and "models.py:186-196" in header
    assert "#define DVQ_ABI_VERSION 10\n" in header
    # the struct mirror follows the header's field order
    assert [f[0] for f in _lib.PixelcnnCtl._fields_] == ["temperature", "top_k", "given", "logp_model_out", "logp_draw_out"]
    assert hasattr(_lib.load(), "dvq_pixelcnn_sample_ctl")


def test_ops_refuse_bad_controls():
    """The controls are validated before anything touches a device."""
    lab, q = torch.zeros(4, dtype=torch.int64), torch.ones(4, 9, 32)
    for T in (0.0, -1.0, float("inf"), float("nan"), "1", None, True):
        with pytest.raises(RuntimeError, match="temperature"):
            ops.pixelcnn_sample(None, lab, q, temperature=T)
    for k in (-1, 1.5, "3", True):
        with pytest.raises(RuntimeError, match="top_k"):
            ops.pixelcnn_sample(None, lab, q, top_k=k)
    for g in (torch.zeros(4, 8, dtype=torch.int64), torch.zeros(3, 9, dtype=torch.int64), torch.zeros(4, 9, dtype=torch.int32),
              torch.zeros(4, 3, 3, 1, dtype=torch.int64), torch.zeros(4, 18, dtype=torch.int64)[:, ::2], [[0] * 9] * 4):
        with pytest.raises(RuntimeError, match="given"):
            ops.pixelcnn_sample(None, lab, q, given=g)
    with pytest.raises(RuntimeError, match="noise"):
        ops.pixelcnn_sample(None, lab, None)


def test_code_grid_places_part_codes_at_the_code_slots():
    from dvqvae_amd.network.gen_net import CODE_SLOTS, code_grid
    parts = torch.arange(12).view(2, 6) + 10
    g = code_grid(parts)
    assert g.dtype == torch.int64 and tuple(g.shape) == (2, 3, 3)
    assert g[:, :, 0].eq(-1).all(), "the context column is drawn"
    for k, (i, j) in enumerate(CODE_SLOTS):
        assert torch.equal(g[:, i, j], parts[:, k])
    with pytest.raises(RuntimeError):
        code_grid(torch.zeros(2, 5, dtype=torch.int64))


def test_restatement_definitions_on_hand_cases():
    l = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0, 0.0, -0.0, 0.5]])
    q = torch.ones(1, 8)
    assert R.kept_set(l, 2).tolist() == [[False, True, True, False, False, False, False, False]], "ties towards the lowest index"
    assert R.kept_set(l, 4).tolist() == [[True, True, True, False, True, False, False, False]]
    assert R.kept_set(l, 6).tolist() == [[True, True, True, False, True, True, False, True]], "-0 ties with +0"
    assert bool(R.kept_set(l, 0).all()) and bool(R.kept_set(l, 8).all()) and bool(R.kept_set(l, 99).all())
    r = R.draw(l, q, temperature=2.0, top_k=1)
    assert r.code.tolist() == [1] and r.logp_draw.tolist() == [0.0]
    assert abs(float(r.logp_model[0]) - float(torch.log_softmax(l.double(), 1)[0, 1])) < 1e-12
    r = R.draw(l, q, top_k=2, given=torch.tensor([4]))
    assert r.code.tolist() == [4] and r.logp_draw.tolist() == [float("-inf")] and np.isfinite(float(r.logp_model[0]))
    r = R.draw(l, q, top_k=2, given=torch.tensor([2]))
    assert abs(float(r.logp_draw[0]) - np.log(1.0 / 2.0)) < 1e-12, "two of the three 3.0 are kept"
    # noise decides among the kept codes only
    qq = torch.ones(1, 8)
    qq[0, 3] = 1e-30
    assert R.draw(l, qq).code.tolist() == [3] and R.draw(l, qq, top_k=5).code.tolist() == [1]
    # temperature 0.5 squares the odds
    r1, r2 = R.draw(l, q), R.draw(l, q, temperature=0.5, given=torch.tensor([7]))
    assert abs(float(r2.logp_draw[0]) - float(torch.log_softmax(2 * l.double(), 1)[0, 7])) < 1e-12
    assert float(r2.logp_model[0]) == float(R.draw(l, q, given=torch.tensor([7])).logp_model[0]), "logp_model ignores the controls"
    nan = l.clone()
    nan[0, 5] = float("nan")
    r = R.draw(torch.cat([l, nan]), torch.ones(2, 8), given=torch.tensor([-1, -1]))
    assert r.code.tolist() == [1, -1] and bool(torch.isnan(r.logp_model[1])) and bool(torch.isnan(r.logp_draw[1]))


def test_restatement_with_controls_off_is_the_oracle_sampler(golden):
    """The one point where the reference defines the draw: softmax of the logits, exponential race.  On the reduced prior of the
    G4 golden the restatement (T = 1, top_k = 0, nothing given) must draw the oracle's codes position by position, and the
    reference's recorded grid in the end."""
    from test_oracle_golden import pixelcnn_template
    g = golden("g4_pixelcnn")
    sd = synth.synthetic_state_dict(pixelcnn_template(32, 64, 3, 16), SEED + 1)
    lab = torch.from_numpy(g["small_label"])
    q = synth.exp1_noise(5, 9, 32, seed=5)
    x = torch.zeros(5, 3, 3, dtype=torch.int64)
    with torch.no_grad():
        for i in range(3):
            for j in range(3):
                logits = O.pixelcnn_forward(sd, "", x, lab)[:, :, i, j]
                r = R.draw(logits, q[:, i * 3 + j])
                assert torch.equal(r.code, O.sample_from_logits(logits, q[:, i * 3 + j]))
                assert bool(r.kept.all())
                np.testing.assert_allclose(r.logp_model.numpy(), torch.log_softmax(logits.double(), 1).gather(1, r.code[:, None])[:, 0].numpy(),
                                           atol=1e-12)
                assert torch.equal(r.logp_model, r.logp_draw)
                x[:, i, j] = r.code
    assert np.array_equal(x.numpy(), g["small_codes"])


def test_float32_arithmetic_stays_inside_the_bounds_the_device_is_held_to():
    """Where the bounds come from: the same restatement evaluated in float32 (what a device kernel can do at best) against float64
    on Gaussian logits of the golden prior's spread -- rows set aside by the 1e-4 race gap stay far below the 0.1 % cap, no other
    row disagrees, and the log-probabilities agree to 1e-6 (the tests allow the device 1e-5)."""
    gen = torch.Generator().manual_seed(11)
    B, n = 16384, 512
    l = torch.randn(B, n, generator=gen) * 3.0
    q = torch.empty(B, n).exponential_(generator=gen)
    for T in (0.5, 1.0, 2.0):
        for k in (0, 5, 40):
            a, b = R.draw(l, q, T, k), R.draw(l, q, T, k, dtype=torch.float32)
            aside = a.gap <= GAP
            assert float(aside.float().mean()) <= SET_ASIDE_CAP
            assert torch.equal(a.code[~aside], b.code[~aside])
            assert float((a.logp_model - b.logp_model.double()).abs().max()) < 2e-6
            assert float((a.logp_draw - b.logp_draw.double()).abs().max()) < 2e-6


# ------------------------------------------------------------------------------------------ GPU: the kernel through the C ABI
_PRIORS = {}


def _prior(cfg=(512, 512, 15, 128), seed=SEED + 2):
    from dvqvae_amd.network.pixelcnn.models import GatedPixelCNN
    if (cfg, seed) not in _PRIORS:
        net = GatedPixelCNN(*cfg)
        load_synth(net, seed)
        _PRIORS[(cfg, seed)] = net.to(DEV)
    return _PRIORS[(cfg, seed)]


def _inputs(B, n_tok, n_cls, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, n_cls, (B,), generator=g).to(DEV)
    q = ops.exp1_noise(B, 9 * n_tok, seed, 0, 0, device=torch.device(DEV)).view(B, 9, n_tok)
    return lab, q


def _check_against_restatement(codes, logits, q, lm, ld, T, k, given=None, what=""):
    """Every position of a call against the restatement on the exported logits and the same noise.  Returns the figures.
    A row of the restatement is one row of logits, i.e. one draw: a call of B rows holds nine sets of B draws, each evaluated on its
    own exported logits and independent of the others.  A draw is set aside -- that (row, position) alone, every other position of
    the row is still compared -- when the restatement's two best race scores lie within a relative 1e-4, and at EVERY position at
    most 0.1 % of the B rows may be set aside (float32 against float64 on Gaussian logits sets aside about 0.02 % of the draws,
    test_float32_arithmetic_stays_inside_the_bounds_the_device_is_held_to; the union over a row's nine draws is then about
    0.1 - 0.2 % of the rows whatever the device computes, so the cap is not applied to the union)."""
    B = codes.shape[0]
    codes = codes.view(B, 9)
    aside_rows = torch.zeros(B, dtype=torch.bool, device=codes.device)
    worst_m = worst_d = worst_frac = 0.0
    for pos in range(9):
        r = R.draw(logits[:, pos], q[:, pos], T, k, None if given is None else given[:, pos])
        c = codes[:, pos]
        assert bool((c >= 0).all()), f"{what} position {pos}: a draw from NaN logits"
        assert bool(r.kept.gather(1, c[:, None])[r.drawn].all()), f"{what} position {pos}: a drawn code outside the kept set"
        aside = r.drawn & (r.gap <= GAP)
        differ = (c != r.code) & ~aside
        assert not bool(differ.any()), f"{what} position {pos}: {int(differ.sum())} codes differ from the restatement beyond the race gap"
        aside_rows |= aside
        frac = float(aside.float().mean())
        worst_frac = max(worst_frac, frac)
        assert frac <= SET_ASIDE_CAP, f"{what} position {pos}: {100 * frac:.3f} % of the rows set aside by the race gap (cap 0.1 %)"
        # log-probabilities of the DEVICE's code (the restatement's own where they agree; evaluated for the device's otherwise)
        rr = R.draw(logits[:, pos], q[:, pos], T, k, c)
        fin = torch.isfinite(rr.logp_draw)
        assert bool(torch.isfinite(lm[:, pos]).all()) and torch.equal(torch.isfinite(ld[:, pos]), fin)
        assert torch.equal(ld[:, pos][~fin], rr.logp_draw[~fin].float()), "-inf exactly where the given code is outside the kept set"
        worst_m = max(worst_m, float((lm[:, pos].double() - rr.logp_model).abs().max()))
        if bool(fin.any()):
            worst_d = max(worst_d, float((ld[:, pos].double() - rr.logp_draw)[fin].abs().max()))
    frac = worst_frac
    print(f"{what} T={T} top_k={k}: draws set aside at the worst position {100 * frac:.4f} % of {B} rows (rows with any of their nine "
          f"draws set aside: {int(aside_rows.sum())}), no other code differs; worst |logp_model - fp64| {worst_m:.3e}, "
          f"worst |logp_draw - fp64| {worst_d:.3e}")
    assert worst_m <= TOL and worst_d <= TOL, f"{what}: log-probabilities off by {worst_m:.3e} / {worst_d:.3e}"
    return frac, worst_m, worst_d


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 100, 16385])
def test_defaults_equal_the_plain_sampler_bitwise(B):
    """dvq_pixelcnn_sample_ctl with T = 1, top_k = 0 and nothing given (reached through return_logp) against dvq_pixelcnn_sample:
    codes and exported logits bit for bit; and with everything at its default ops.pixelcnn_sample does not enter it at all."""
    net = _prior()
    pk = net.packed()
    lab, q = _inputs(B, 512, 128, 100 + B)
    lib = _lib.load()
    calls = []
    real = lib.dvq_pixelcnn_sample_ctl
    c0, l0 = ops.pixelcnn_sample(pk, lab, q, return_logits=True)
    try:
        lib.dvq_pixelcnn_sample_ctl = lambda *a: calls.append(1) or real(*a)
        c_def, l_def = ops.pixelcnn_sample(pk, lab, q, return_logits=True, temperature=1.0, top_k=0, given=None, return_logp=False)
        assert not calls, "all controls at their defaults: the plain entry point"
        c1, l1, lm, ld = ops.pixelcnn_sample(pk, lab, q, return_logits=True, return_logp=True)
        assert calls == [1]
    finally:
        lib.dvq_pixelcnn_sample_ctl = real
    assert torch.equal(c_def, c0) and torch.equal(l_def, l0)
    assert torch.equal(c1, c0), "codes of the controlled kernel at neutral controls != sample_kernel's"
    assert torch.equal(l1, l0)
    assert torch.equal(lm, ld), "T = 1 and no top-k: the two log-probabilities are one number"
    want = torch.log_softmax(l0.double(), dim=2).gather(2, c0.view(B, 9, 1))[:, :, 0]
    assert float((lm.double() - want).abs().max()) <= TOL
    # top_k >= n_in switches the selection off as 0 does
    c2 = ops.pixelcnn_sample(pk, lab, q, top_k=512)
    c3 = ops.pixelcnn_sample(pk, lab, q, top_k=100000)
    assert torch.equal(c2, c0) and torch.equal(c3, c0)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_top_k_one_is_the_argmax_whatever_the_noise(T):
    net = _prior()
    B = 4096
    lab, q = _inputs(B, 512, 128, 7)
    codes, logits, lm, ld = net.generate(None, lab, batch_size=B, noise=q, return_logits=True, temperature=T, top_k=1, return_logp=True)
    assert torch.equal(codes.view(B, 9), torch.argmax(logits, dim=2)), "top_k = 1 must draw the lowest-index argmax of its logits"
    assert bool((ld == 0).all()), "logp_draw of the only kept code is 0 exactly"
    q2 = _inputs(B, 512, 128, 8)[1]
    assert torch.equal(net.generate(None, lab, batch_size=B, noise=q2, temperature=T, top_k=1), codes)
    want = torch.log_softmax(logits.double(), dim=2).gather(2, codes.view(B, 9, 1))[:, :, 0]
    assert float((lm.double() - want).abs().max()) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("top_k", [0, 5, 40])
@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_draws_and_log_probabilities_against_the_float64_restatement(T, top_k):
    """65 536 rows of the full-size prior (n_in = 512), every position: codes, kept set, both log-probabilities."""
    net = _prior()
    B = 65536
    lab, q = _inputs(B, 512, 128, 21)
    codes, logits, lm, ld = net.generate(None, lab, batch_size=B, noise=q, return_logits=True, temperature=T, top_k=top_k, return_logp=True)
    _check_against_restatement(codes, logits, q, lm, ld, T, top_k, what="full prior")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [(32, 64, 3, 16), (100, 64, 2, 8), (1024, 64, 2, 8), (1, 64, 2, 4)])
def test_any_token_count_and_exact_ties(cfg):
    """Token counts below a wave, not a multiple of 64, beyond the register-resident 512 (the kernel's second instantiation) and 1;
    and exact ties at the top-k boundary: the head's last layer is rounded so coarsely that logits repeat within a row."""
    net = _prior(cfg, SEED + 31)
    n_tok, n_cls = cfg[0], cfg[3]
    B = 3000
    lab, q = _inputs(B, n_tok, n_cls, 5)
    w, b = net.output_conv[2].weight, net.output_conv[2].bias
    saved = w.detach().clone(), b.detach().clone()
    try:
        for coarse in (False, True):
            if coarse:                       # logits on a coarse grid: many exact ties, signed zeros included
                with torch.no_grad():
                    w.zero_()
                    b.copy_((torch.arange(n_tok, device=DEV) % 7).float() - 3.0)
            for T, k in ((1.0, 0), (0.7, 3), (1.0, n_tok - 1), (3.0, 10), (0.5, 1)):
                if k >= n_tok and n_tok > 1:
                    k = n_tok - 1
                given = torch.full((B, 9), -1, dtype=torch.int64, device=DEV)
                given[::3, 4] = torch.arange(0, B, 3, device=DEV) % n_tok
                codes, logits, lm, ld = net.generate(None, lab, batch_size=B, noise=q, return_logits=True, temperature=T, top_k=k,
                                                     given=given, return_logp=True)
                if coarse:
                    assert int(torch.unique(logits[0, 0]).numel()) <= 7
                _check_against_restatement(codes, logits, q, lm, ld, T, k, given=given, what=f"{cfg} coarse={coarse}")
                assert torch.equal(codes.view(B, 9)[::3, 4], given[::3, 4])
    finally:
        with torch.no_grad():
            w.copy_(saved[0])
            b.copy_(saved[1])
        _PRIORS.pop((cfg, SEED + 31), None)


@pytest.mark.gpu
def test_given_codes():
    net = _prior()
    B = 64
    lab, q = _inputs(B, 512, 128, 33)
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, 512, (B, 3, 3), generator=g).to(DEV)
    # all nine given: the codes come back, log_prob is log_softmax of the teacher-forced logits at x
    codes, logits, lm, ld = net.generate(None, lab, batch_size=B, noise=q, return_logits=True, given=x, return_logp=True)
    assert torch.equal(codes, x)
    tf = net(x, lab).permute(0, 2, 3, 1).reshape(B, 9, 512)
    assert torch.equal(logits, tf), "all nine given: the logits are the teacher-forced forward's"
    want = torch.log_softmax(tf.double(), dim=2).gather(2, x.view(B, 9, 1))[:, :, 0]
    lp = net.log_prob(x, lab)
    assert tuple(lp.shape) == (B, 9) and lp.dtype == torch.float32
    assert float((lp.double() - want).abs().max()) <= TOL
    assert torch.equal(lp, lm) and torch.equal(lm, ld)
    assert torch.equal(net.log_prob(x.view(B, 9), lab), lp)
    # prefix replay: the first m positions of an unconstrained run given, same noise -> the run again, bit for bit
    for T, k in ((1.0, 0), (0.8, 40)):
        c0, l0, lm0, ld0 = net.generate(None, lab, batch_size=B, noise=q, return_logits=True, temperature=T, top_k=k, return_logp=True)
        for m in range(10):
            given = c0.view(B, 9).clone()
            given[:, m:] = -1
            c, l, lm_, ld_ = net.generate(None, lab, batch_size=B, noise=q, return_logits=True, temperature=T, top_k=k, given=given,
                                          return_logp=True)
            assert torch.equal(c, c0) and torch.equal(l, l0) and torch.equal(lm_, lm0), f"T={T} top_k={k}: prefix of {m} given"
            assert torch.equal(ld_, ld0), "a drawn code replayed as a given one lies in the kept set: the same logp_draw"
    # causality: a given code at a later position changes no earlier position's code (nor its logits)
    c0, l0 = net.generate(None, lab, batch_size=B, noise=q, return_logits=True, temperature=0.8, top_k=40)
    for p in (1, 4, 8):
        given = torch.full((B, 9), -1, dtype=torch.int64, device=DEV)
        given[:, p] = (c0.view(B, 9)[:, p] + 1 + torch.arange(B, device=DEV)) % 512
        c, l = net.generate(None, lab, batch_size=B, noise=q, return_logits=True, temperature=0.8, top_k=40, given=given)
        assert torch.equal(c.view(B, 9)[:, :p], c0.view(B, 9)[:, :p]) and torch.equal(l[:, :p + 1], l0[:, :p + 1])
        assert torch.equal(c.view(B, 9)[:, p], given[:, p])
        if p < 8:
            assert not torch.equal(l[:, p + 1:], l0[:, p + 1:]), "the given code must reach the later positions"
    # mixed rows: some rows fully given, some partly, some not at all
    given = torch.full((B, 9), -1, dtype=torch.int64, device=DEV)
    given[0::3] = x.view(B, 9)[0::3]
    given[1::3, 2::2] = x.view(B, 9)[1::3, 2::2]
    c, l, lm_, ld_ = net.generate(None, lab, batch_size=B, noise=q, return_logits=True, temperature=0.8, top_k=40, given=given, return_logp=True)
    assert torch.equal(c.view(B, 9)[given >= 0], given[given >= 0])
    _check_against_restatement(c, l, q, lm_, ld_, 0.8, 40, given=given, what="mixed given")
    assert bool(torch.isinf(ld_[given >= 0]).any()), "random given codes mostly fall outside the 40 kept: logp_draw = -inf there"
    for b in (0, 1, 2, 31):                                                     # ... and every row equals its own B = 1 call
        cb, lb = net.generate(None, lab[b:b + 1], batch_size=1, noise=q[b:b + 1].contiguous(), return_logits=True, temperature=0.8,
                              top_k=40, given=given[b:b + 1].contiguous())
        assert torch.equal(cb, c[b:b + 1]) and torch.equal(lb, l[b:b + 1])
    # out of range: bit 0
    bad = x.clone()
    bad[5, 1, 1] = 512
    with pytest.raises(RuntimeError, match="out of range"):
        net.generate(None, lab, batch_size=B, noise=q, given=bad)
    err = ops.new_err_flag(torch.device(DEV))
    ops.pixelcnn_sample(net.packed(), lab, q, given=bad.view(B, 9), err=err)
    assert int(err.item()) & 1
    with pytest.raises(RuntimeError, match="out of range"):                    # nothing to draw from: a negative entry without noise
        ops.pixelcnn_sample(net.packed(), lab, None, given=torch.full((B, 9), -1, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        net.log_prob(torch.full((B, 9), -1, dtype=torch.int64, device=DEV), lab)


@pytest.mark.gpu
def test_nan_logits_at_a_drawn_position():
    """A residual stream beyond fp16's range makes the later logits NaN (tests/test_gpu_parity.py, the range fallback): drawn
    positions report -1 and bit 2 as the plain sampler does, given ones keep their code, both log-probabilities are NaN there."""
    if os.environ.get("DVQ_GEMM", "").lower() in ("fp32", "bf16x3"):
        pytest.skip("the fp16 weight images are not in use")
    net = _gennet().GatedPixelCNN
    B = 6
    lab, q = _inputs(B, 512, 128, 3)
    given = torch.full((B, 9), -1, dtype=torch.int64, device=DEV)
    given[:, 7] = 3
    try:
        with torch.no_grad():
            net.layers[2].horiz_resid.weight.mul_(1.0e7)
        pk = net.packed()
        err = ops.new_err_flag(torch.device(DEV))
        c, logits, lm, ld = ops.pixelcnn_sample(pk, lab, q, return_logits=True, err=err, temperature=0.8, top_k=40, given=given, return_logp=True)
    finally:
        with torch.no_grad():
            net.layers[2].horiz_resid.weight.mul_(1.0e-7)
    nan_pos = torch.isnan(logits).any(dim=2)
    assert bool(nan_pos.any()), "the scaled weight must push the logits out of range"
    assert int(err.item()) & 4
    c = c.view(B, 9)
    drawn = given < 0
    assert bool((c[nan_pos & drawn] == -1).all()) and bool((c[~nan_pos] >= 0).all())
    assert torch.equal(c[:, 7], given[:, 7])
    assert bool(torch.isnan(lm[nan_pos]).all()) and bool(torch.isnan(ld[nan_pos]).all())
    assert bool(torch.isfinite(lm[~nan_pos]).all())


# ------------------------------------------------------------------------------------------ GPU: GenNet.gen
def _gennet():
    """The synthetic net of tests/test_gpu_parity.py::_gennet."""
    from conftest import GOLDEN, gen_state_dict
    from dvqvae_amd import mano as dmano
    from dvqvae_amd.network.gen_net import GenNet
    net = GenNet()
    sd = gen_state_dict(net.state_dict(), np.load(os.path.join(GOLDEN, "g7_gen.npz")))
    net.load_state_dict(sd, strict=True)
    net.eval().to(DEV)
    net.set_rh_mano(dmano.ManoLayer(dmano.synthetic_mano_arrays()).to(DEV))
    return net


CTL = dict(temperature=0.8, top_k=40)
_AUX = ("codes", "logp_model", "logp_draw")


def _some_given(B, seed=0):
    """[B,3,3]: a third of the rows hold given hand-part codes at some code slots, context column and the other rows drawn."""
    from dvqvae_amd.network.gen_net import code_grid
    g = torch.Generator().manual_seed(seed)
    parts = torch.randint(0, 128, (B, 6), generator=g)
    parts[torch.rand(B, 6, generator=g) < 0.5] = -1
    parts[torch.arange(B) % 3 != 0] = -1
    return code_grid(parts).to(DEV)


def _same(a, b, rows_a=None, rows_b=None, what=""):
    (ra, pa, xa), (rb, pb, xb) = a, b
    sa = (lambda t: t if rows_a is None else t[rows_a])
    sb = (lambda t: t if rows_b is None else t[rows_b])
    assert torch.equal(sa(ra), sb(rb)) and torch.equal(sa(pa), sb(pb)), f"{what}: parameters differ"
    for k in _AUX:
        assert torch.equal(sa(xa[k]), sb(xb[k])), f"{what}: aux[{k}] differs"


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 100, 16385])
def test_gen_defaults_run_the_plain_sampler_and_equal_the_controlled_kernel(B):
    """gen() with the controls at their defaults never enters the controlled entry point (the launches of the commit before the
    controls); and the controlled kernel at neutral controls (log_prob=True) returns the same parameters bit for bit, fixed seed."""
    net = _gennet()
    obj = synth.synthetic_clouds(min(B, 128), 256, seed=61).to(DEV)
    obj = obj[torch.arange(B, device=DEV) % obj.shape[0]].contiguous()
    lib = _lib.load()
    calls = []
    real = lib.dvq_pixelcnn_sample_ctl
    try:
        lib.dvq_pixelcnn_sample_ctl = lambda *a: calls.append(1) or real(*a)
        r0, p0, a0 = net.gen(obj, seed=9, row0=0, stream_id=1, return_aux=True)
        r1, p1, a1 = net.gen(obj, seed=9, row0=0, stream_id=1, return_aux=True, temperature=1.0, top_k=0, codes=None)
        assert not calls and "logp_model" not in a0 and "logp_model" not in a1
        r2, p2, a2 = net.gen(obj, seed=9, row0=0, stream_id=1, return_aux=True, log_prob=True)
        assert calls
    finally:
        lib.dvq_pixelcnn_sample_ctl = real
    for r, p, a in ((r1, p1, a1), (r2, p2, a2)):
        assert torch.equal(r, r0) and torch.equal(p, p0) and torch.equal(a["codes"], a0["codes"])
    assert tuple(a2["logp_model"].shape) == (B, 9) and torch.equal(a2["logp_model"], a2["logp_draw"])
    assert bool(torch.isfinite(a2["logp_model"]).all())


@pytest.mark.gpu
def test_gen_under_controls_batched_equals_single_calls():
    net = _gennet()
    B = 6
    obj = synth.synthetic_clouds(B, 512, seed=77).to(DEV)
    q = synth.exp1_noise(B, 9, 512, seed=78).to(DEV)
    codes = _some_given(B)
    whole = net.gen(obj, noise=q, return_aux=True, codes=codes, **CTL)
    assert bool((whole[2]["codes"][codes >= 0] == codes[codes >= 0]).all()) and bool((codes >= 0).any())
    for b in range(B):
        one = net.gen(obj[b:b + 1], noise=q[b:b + 1], return_aux=True, codes=codes[b:b + 1], **CTL)
        _same(one, whole, None, slice(b, b + 1), f"row {b}")
    # the same without a host synchronisation
    r, p, a = net.gen(obj, noise=q, return_aux=True, codes=codes, check=False, **CTL)
    _same((r, p, a), whole, what="check=False")
    assert int(a["err"].item()) == 0
    # the controls do something, and logp_model is the prior's view of the codes whatever they were drawn under
    plain = net.gen(obj, noise=q, return_aux=True, log_prob=True)
    lp = net.GatedPixelCNN.log_prob(whole[2]["codes"], whole[2]["idx6"][:, 0].contiguous())
    assert torch.equal(lp, whole[2]["logp_model"])
    assert not torch.equal(plain[2]["logp_draw"], whole[2]["logp_draw"])
    with pytest.raises(RuntimeError):
        net.gen(obj, noise=q, codes=codes[:-1])
    with pytest.raises(RuntimeError):
        net.gen(obj, noise=q, codes=codes.to(torch.int32))
    with pytest.raises(RuntimeError, match="temperature"):
        net.gen(obj, noise=q, temperature=0.0)


@pytest.mark.gpu
def test_gen_under_controls_sharded_sorted_and_keyed():
    from dvqvae_amd import dist
    net = _gennet()
    # shards by row0 == the whole call (700 rows: the whole call sorts by label, the shards of 4 do not)
    B = 700
    obj = synth.synthetic_clouds(B, 256, seed=505).to(DEV)
    codes = _some_given(B, 1)
    whole = net.gen(obj, seed=77, row0=1000, stream_id=5, return_aux=True, codes=codes, **CTL)
    assert len(set(whole[2]["idx6"].reshape(-1).tolist())) >= 2, "the inputs must exercise the label sort"
    for n_shards in (2, 4):
        for rank in range(n_shards):
            lo, hi = dist.shard_range(B, rank, n_shards)
            part = net.gen(obj[lo:hi], seed=77, row0=1000 + lo, stream_id=5, return_aux=True, codes=codes[lo:hi], **CTL)
            _same(part, whole, None, slice(lo, hi), f"{n_shards} shards, rank {rank}")
    # sorted by label == arrival order
    net.sort_by_label = False
    try:
        unsorted = net.gen(obj, seed=77, row0=1000, stream_id=5, return_aux=True, codes=codes, **CTL)
    finally:
        net.sort_by_label = True
    _same(unsorted, whole, what="label sort")
    # row_keys: a call that mixes the grasps of 8 objects == the objects' own calls
    n_obj, n_grasp = 8, 100
    B = n_obj * n_grasp
    clouds = synth.synthetic_clouds(B, 256, seed=77).to(DEV)
    given = _some_given(B, 2)
    order = torch.from_numpy(np.random.default_rng(3).permutation(B)).to(DEV)
    sid, rid = (order // n_grasp).contiguous(), (order % n_grasp).contiguous()
    mixed = net.gen(clouds[order].contiguous(), seed=41, row_keys=(sid, rid), return_aux=True, codes=given[order].contiguous(), **CTL)
    for o in range(n_obj):
        own = net.gen(clouds[o * n_grasp:(o + 1) * n_grasp].contiguous(), seed=41, row0=0, stream_id=o, return_aux=True,
                      codes=given[o * n_grasp:(o + 1) * n_grasp].contiguous(), **CTL)
        rows = (sid == o).nonzero().reshape(-1)
        _same(mixed, own, rows, rid[rows], f"object {o}")


@pytest.mark.gpu
def test_gen_range_fallback_under_controls():
    """The fixture of test_gen_range_fallback_regenerates_only_the_rows_that_need_it with the controls on: exactly the bad row is
    regenerated (same controls, same given codes, same noise key), every other row keeps its bits, its log-probabilities are finite."""
    from dvqvae_amd import packing
    if packing.gemm_kind() != _lib.PLANES_F16X2:
        pytest.skip("the fp16 weight images are not in use")
    net = _gennet()
    B, bad = 40, 17
    obj = synth.synthetic_clouds(B, 300, seed=91).to(DEV)
    clean = obj.clone()
    scale = None
    for s_try in (1.0e3, 1.0e4, 1.0e5, 1.0e6):                                   # the smallest scale that leaves fp16's range
        with torch.no_grad():
            f_bad, _, _ = net.obj_encoder_type(clean[bad:bad + 1] * s_try)
        if float(f_bad.abs().max()) > 7.0e4:
            scale = s_try
            break
    assert scale is not None, "no scale pushed the PointNet feature (a decoder input) beyond fp16's range"
    obj[bad] *= scale
    codes = _some_given(B, 3)
    codes[bad] = _some_given(3, 4)[0]                                            # the bad row holds given codes too
    assert bool((codes[bad] >= 0).any())
    key = dict(seed=5, row0=300, stream_id=2, return_aux=True, codes=codes, **CTL)
    n0, r0 = net.range_fallbacks, net.range_fallback_rows
    got = net.gen(obj, **key)
    assert net.range_fallbacks == n0 + 1 and net.range_fallback_rows == r0 + 1 and got[2]["fallback_rows"].tolist() == [bad]
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
    assert bool(torch.isfinite(got[2]["logp_model"][bad]).all()) and not bool(torch.isnan(got[2]["logp_draw"][bad]).any())
    assert bool((got[2]["codes"][bad][codes[bad] >= 0] == codes[bad][codes[bad] >= 0]).all())
    ref = net.gen(clean, **key)                                                  # no row out of range: no fallback
    assert net.range_fallbacks == n0 + 1
    keep = [i for i in range(B) if i != bad]
    _same(got, ref, keep, keep, "rows inside the range")
    from test_gpu_parity import _with_env
    six = _with_env("DVQ_GEMM", "bf16x3", lambda: net.gen(obj, **key))
    _same(got, six, slice(bad, bad + 1), slice(bad, bad + 1), "the regenerated row against the six-product result")


@pytest.mark.gpu
def test_temperature_moves_the_likelihood_of_the_draws():
    """16 384 rows, one seed: the mean log-likelihood (under the untempered prior) of the drawn grids falls strictly as T goes
    0.5 -> 1 -> 2, by far more than its standard error."""
    net = _gennet()
    B = 16384
    obj = synth.synthetic_clouds(64, 256, seed=12).to(DEV)
    obj = obj[torch.arange(B, device=DEV) % 64].contiguous()
    means, sems = [], []
    for T in (0.5, 1.0, 2.0):
        _, _, aux = net.gen(obj, seed=3, row0=0, stream_id=0, return_aux=True, temperature=T, log_prob=True)
        total = aux["logp_model"].double().sum(dim=1)
        means.append(float(total.mean()))
        sems.append(float(total.std() / np.sqrt(B)))
    print(f"mean grasp log-likelihood at T = 0.5 / 1 / 2: {means}, standard errors {sems}")
    assert means[0] > means[1] > means[2]
    assert means[0] - means[1] > 10 * max(sems) and means[1] - means[2] > 10 * max(sems)
    # top_k narrows the draw as well
    _, _, aux = net.gen(obj, seed=3, row0=0, stream_id=0, return_aux=True, top_k=5)
    assert float(aux["logp_model"].double().sum(dim=1).mean()) > means[1]


# ------------------------------------------------------------------------------------------ GPU: entry points
def _run_main(dataset, out_dir, extra):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent",
                                            "--mano_model", "/nonexistent"])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", ["obman", "ho3d"])
def test_entry_point_flags(tmp_path, dataset):
    base = ["--num_objects", "4", "--points", "256"]
    n0, b0 = _run_main(dataset, str(tmp_path / "plain"), base)
    n1, b1 = _run_main(dataset, str(tmp_path / "defaults"), base + ["--temperature", "1.0", "--top_k", "0", "--log_prob", "0"])
    assert n1 == n0 and b1 == b0, "the three flags at their defaults must not change a byte"
    ctl = ["--top_k", "40", "--temperature", "0.8", "--log_prob", "1"]
    names, ref = _run_main(dataset, str(tmp_path / "loop"), base + ctl + ["--rows_per_call", "0"])
    assert names == n0 and ref != b0
    for tag, extra in (("default", []), ("seven", ["--rows_per_call", "7"])):
        n, data = _run_main(dataset, str(tmp_path / tag), base + ctl + extra)
        assert n == names and data == ref, f"{tag}: the files depend on --rows_per_call"
    G = generate.DATASETS[dataset]["num_grasp"]
    for blob, plain in zip(ref, b0):
        doc = json.loads(blob)
        assert set(doc) == set(json.loads(plain)) | {"log_prob"}
        assert len(doc["log_prob"]) == G == len(doc["recon_params"]) and all(np.isfinite(v) and v < 0 for v in doc["log_prob"])


@pytest.mark.gpu
def test_generate_for_objects_log_prob_is_the_sum_of_the_positions():
    net = _gennet()
    seed, G = 9, 7
    objs = [synth.synthetic_clouds(1, n, seed=50 + i)[0] for i, n in enumerate((700, 300, 700))]
    indices = [5, 2, 11]
    want = [generate.generate_for_object(net, objs[i], G, False, np.random.default_rng([seed, indices[i]]), seed=seed,
                                         object_index=indices[i], log_prob=True, **CTL) for i in range(3)]
    for rows_per_call in (16384, 10, 1):
        got = generate.generate_for_objects(net, objs, G, False, seed, indices, rows_per_call=rows_per_call, log_prob=True, **CTL)
        for i in range(3):
            assert set(got[i]) == set(want[i]) and "log_prob" in got[i]
            assert torch.equal(got[i]["params"], want[i]["params"]) and torch.equal(got[i]["log_prob"], want[i]["log_prob"])
            assert got[i]["json"] == want[i]["json"]
    # against gen() itself: the batch generate_for_object builds without rotation is the cloud repeated
    for i in range(3):
        batch = ops.transform_cloud(objs[i].to(DEV).contiguous(), torch.eye(3, device=DEV).repeat(G, 1, 1), torch.zeros(3, device=DEV))
        _, _, aux = net.gen(batch, seed=seed, row0=0, stream_id=indices[i], return_aux=True, log_prob=True, **CTL)
        lp = want[i]["log_prob"]
        assert tuple(lp.shape) == (G,) and bool(torch.isfinite(lp).all())
        assert torch.equal(lp, generate.grasp_log_prob(aux["logp_model"]))
        assert float((lp.double() - aux["logp_model"].double().sum(dim=1)).abs().max()) <= 1e-5
        assert want[i]["json"]["log_prob"] == lp.cpu().numpy().tolist()
    plain = generate.generate_for_object(net, objs[0], G, False, np.random.default_rng([seed, 5]), seed=seed, object_index=5)
    assert "log_prob" not in plain and "log_prob" not in plain["json"]
