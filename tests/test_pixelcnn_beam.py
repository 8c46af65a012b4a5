"""Beam search over the prior (include/dvq.h: dvq_pixelcnn_beam) against its float64 restatement
(tests/pixelcnn_beam_ref.py), exhaustive enumeration on a three-token prior, and the project's standing contract that every path
computes the same bits per row (greedy decoding, replay through the controlled sampler and the teacher-forced forward).

Bounds.  The selection is compared step by step on the device's OWN traced logits and previous scores, so one step's difference
cannot compound: every survivor's float64 candidate score >= the W-th best - BAND and every candidate above the W-th best + BAND
survives, BAND = 1e-4 (GAP of tests/test_prior_controls.py, about 25 ulp of a score near -56); traced scores within TOL = 1e-5 of
float64 (the project's parity bar).  test_float32_selection_stays_inside_the_band shows float32 arithmetic fits both."""
import os

import numpy as np
import pytest
import torch

from conftest import SEED
from util import load_synth
from dvqvae_amd import _lib, generate, ops, synth
import pixelcnn_beam_ref as BR
import pixelcnn_ref as P

DEV = "cuda:0"
TOL = 1e-5
BAND = 1e-4
TINY = (3, 64, 2, 2)
SLOTS = (1, 2, 4, 5, 7, 8)                 # flat grid positions of gen_net.CODE_SLOTS


# ------------------------------------------------------------------------------------------ no GPU
@pytest.fixture(scope="module")
def tiny():
    """The three-token prior, every one of its 3^9 grids scored under label 1 (computed once, never changed)."""
    torch.manual_seed(0)
    sd = synth.synthetic_state_dict(P.template(TINY), SEED + 7)
    with torch.no_grad():
        codes, score = BR.enumerate_all(sd, 1, 3)
    return sd, codes, score


def test_restatement_equals_exhaustive_enumeration(tiny):
    sd, codes, score = tiny
    order = torch.argsort(-score, stable=True)
    with torch.no_grad():
        c, s, n = BR.beam(sd, torch.tensor([1]), 3 ** 8)
    assert int(n[0]) == 3 ** 8
    assert torch.equal(c[0, :50], codes[order[:50]]), "with W = 3^8 nothing is pruned before the last position: the search is exact"
    np.testing.assert_allclose(s[0, :50].numpy(), score[order[:50]].numpy(), rtol=0, atol=1e-12)
    with torch.no_grad():
        c, s, n = BR.beam(sd, torch.tensor([1]), 4)
    assert int(n[0]) == 4
    flat = sum(c[0, :, p] * 3 ** (8 - p) for p in range(9))
    np.testing.assert_allclose(s[0].numpy(), score[flat].numpy(), rtol=0, atol=1e-12)
    assert float(s[0].max()) <= float(score.max()) + 1e-12
    assert bool((s[0, :-1] >= s[0, 1:]).all())


def test_restatement_definitions_on_hand_cases():
    # ties go to the lower flat index b * n_in + k; -0 ties with +0
    cand = torch.tensor([[1.0, 3.0, 3.0], [3.0, -0.0, 0.0]], dtype=torch.float64)
    assert BR.select(cand, 2).tolist() == [1, 2] and BR.select(cand, 4).tolist() == [1, 2, 3, 0]
    assert BR.select(cand, 6).tolist() == [1, 2, 3, 0, 4, 5] and BR.select(cand, 99).numel() == 6
    # live counts at the early positions, -1 / -inf beyond them
    g = torch.Generator().manual_seed(3)
    table = torch.randn(9, 3, generator=g, dtype=torch.float64)
    codes, score, live, trace = BR.search(lambda pre, p: table[p][None, :].expand(pre.shape[0], 3), 3, 100)
    assert [t[0].numel() for t in trace] == [min(100, 3 ** (p + 1)) for p in range(9)] and live == 100
    codes, score, live, _ = BR.search(lambda pre, p: table[p][None, :].expand(pre.shape[0], 3) if p < 8 else torch.full((pre.shape[0], 3), float("nan")), 3, 5)
    assert live == 0 and bool((codes == -1).all()) and bool(torch.isinf(score).all())
    # a position-independent prior: the best grid takes the best token everywhere, its score is the sum
    codes, score, live, _ = BR.search(lambda pre, p: table[p][None, :].expand(pre.shape[0], 3), 3, 7)
    assert codes[0].tolist() == table.argmax(dim=1).tolist()
    assert abs(float(score[0]) - float(torch.log_softmax(table, 1).max(dim=1).values.sum())) < 1e-12
    # fewer grids than W: one-token prior
    codes, score, live, _ = BR.search(lambda pre, p: torch.zeros(pre.shape[0], 1, dtype=torch.float64), 1, 4)
    assert live == 1 and codes[0].tolist() == [0] * 9 and bool((codes[1:] == -1).all()) and score[1:].tolist() == [float("-inf")] * 3
    # a planted duplicate: beams 0 and 2 share the six hand codes and differ in the context column only
    c = torch.tensor([[[5, 1, 2, 6, 3, 4, 7, 5, 6], [5, 1, 2, 6, 3, 9, 7, 5, 6], [8, 1, 2, 8, 3, 4, 8, 5, 6], [5, 1, 2, 6, 3, 4, 7, 5, 6]]])
    assert BR.duplicate_of(c, torch.tensor([4]), SLOTS).tolist() == [[-1, -1, 0, 0]]
    assert BR.duplicate_of(c, torch.tensor([3]), SLOTS).tolist() == [[-1, -1, 0, -1]], "rows beyond n_live are nobody's duplicate"
    from dvqvae_amd.network.gen_net import CODE_SLOTS, GenNet
    assert tuple(i * 3 + j for i, j in CODE_SLOTS) == SLOTS
    assert GenNet.beam_duplicates(c, torch.tensor([4], dtype=torch.int32)).tolist() == [[-1, -1, 0, 0]]
    assert GenNet.beam_duplicates(c.view(1, 4, 3, 3), torch.tensor([3], dtype=torch.int32)).tolist() == [[-1, -1, 0, -1]]


def test_float32_selection_stays_inside_the_band():
    """Where the band comes from: the restatement's selection run with float32 scores, nine positions deep, against float64
    candidates recomputed from the float32 run's own previous scores (exactly what the device is held to below)."""
    gen = torch.Generator().manual_seed(17)
    n, W = 512, 64
    prev, worst = torch.zeros(1, dtype=torch.float32), 0.0
    for p in range(9):
        logits = torch.randn(prev.shape[0], n, generator=gen) * 3.0
        c32, c64 = BR.candidates(prev, logits, torch.float32), BR.candidates(prev, logits, torch.float64)
        idx = BR.select(c32, W)
        BR.band_check(c64, idx, W, BAND, f"position {p}")
        worst = max(worst, float((c32.double() - c64).abs().max()))
        prev = c32.reshape(-1)[idx]
    print(f"float32 against float64 candidate scores, sigma 3, n 512, W 64, nine positions: largest difference {worst:.3e}")
    assert worst <= TOL


@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_beam_flags(dataset):
    p = generate.build_parser(dataset)
    a = p.parse_args([])
    assert a.beam_width == 0 and a.beam_poses == 1
    a = p.parse_args(["--beam_width", "4", "--beam_poses", "2"])
    assert a.beam_width == 4 and a.beam_poses == 2


def test_parse_args_refuses_what_a_beam_cannot_do():
    base = ["--beam_width", "4", "--beam_poses", "2"]
    ok = generate.parse_args("ho3d", base + ["--num_grasp", "8"])
    assert ok.beam_width == 4 and ok.beam_poses == 2
    ok = generate.parse_args("grab", base + ["--num_grasp", "3", "--candidates", "8", "--select_by", "log_prob"])
    assert ok.candidates == 8
    for bad in (base + ["--num_grasp", "7"], base + ["--num_grasp", "3", "--candidates", "9"], base,
                base + ["--num_grasp", "8", "--temperature", "0.8"], base + ["--num_grasp", "8", "--top_k", "5"],
                ["--beam_width", "-1"], ["--beam_width", "2000", "--num_grasp", "2000"], ["--beam_poses", "2"],
                ["--beam_width", "4", "--beam_poses", "0", "--num_grasp", "4"]):
        with pytest.raises(SystemExit):
            generate.parse_args("ho3d", bad)
    assert not generate.DATASETS["obman"]["rotate"]
    with pytest.raises(SystemExit):
        generate.parse_args("obman", base + ["--num_grasp", "8"])         # a dataset that does not rotate takes one pose
    assert generate.parse_args("obman", ["--beam_width", "4", "--num_grasp", "4"]).beam_width == 4
    assert generate.parse_args("obman", []).beam_width == 0


def test_ops_refuse_bad_beams_before_touching_a_device():
    lab = torch.zeros(4, dtype=torch.int64)
    for w in (0, -1, 1025, 1.5, "3", True, None):
        with pytest.raises(RuntimeError, match="width"):
            ops.pixelcnn_beam(None, lab, w)
    with pytest.raises(RuntimeError, match="int64"):
        ops.pixelcnn_beam(None, lab.int(), 4)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.pixelcnn_beam(None, torch.zeros(4, 2, dtype=torch.int64), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.pixelcnn_beam(None, lab, 4)


def test_abi_10_gains_the_beam_search():
    assert _lib.ABI_VERSION == 10
    header = open(_lib.HEADER).read()
    assert "#define DVQ_ABI_VERSION 10\n" in header
    assert "int dvq_pixelcnn_beam(" in header
    assert "size_t dvq_pixelcnn_beam_workspace_bytes(" in header and "} dvq_pixelcnn_beam_trace;" in header
    assert "dvq_pixelcnn_beam" in _lib.SIGNATURES and "dvq_pixelcnn_beam_workspace_bytes" in _lib.SIGNATURES
    assert [f[0] for f in _lib.PixelcnnBeamTrace._fields_] == ["parent", "token", "score", "live", "logits"]
    lib = _lib.load()
    assert hasattr(lib, "dvq_pixelcnn_beam") and hasattr(lib, "dvq_pixelcnn_beam_workspace_bytes")


# ------------------------------------------------------------------------------------------ GPU: the kernel through the C ABI
_PRIORS = {}
SMALL = [(32, 64, 3, 16), (100, 64, 2, 8)]
FULL = (512, 512, 15, 128)


def _prior(cfg, seed=None):
    from dvqvae_amd.network.pixelcnn.models import GatedPixelCNN
    seed = P.SIZES[cfg] if seed is None else seed
    if (cfg, seed) not in _PRIORS:
        net = GatedPixelCNN(*cfg)
        load_synth(net, seed)
        _PRIORS[(cfg, seed)] = net.to(DEV)
    return _PRIORS[(cfg, seed)]


def _labels(cfg, S):
    g = torch.Generator().manual_seed(100 + cfg[0] + S)
    return torch.randint(0, cfg[3], (S,), generator=g).to(DEV)


def _fp16_only():
    if os.environ.get("DVQ_GEMM", "").lower() in ("fp32", "bf16x3"):
        pytest.skip("the beam search runs on the fp16 weight images only")


_RUNS = {}


def _run(cfg, S, W):
    """One traced search per case, shared by the tests that read it."""
    if (cfg, S, W) not in _RUNS:
        lab = _labels(cfg, S)
        codes, score, n_live, tr = ops.pixelcnn_beam(_prior(cfg).packed(), lab, W, trace=True)
        _RUNS[(cfg, S, W)] = (lab, codes, score, n_live, tr)
    return _RUNS[(cfg, S, W)]


CASES = [(cfg, 5, W) for cfg in SMALL for W in (1, 3, 64, 100)] + [(FULL, 3, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,S,W", CASES)
def test_every_step_against_the_restatement(cfg, S, W):
    _fp16_only()
    n_in = cfg[0]
    lab, codes, score, n_live, tr = _run(cfg, S, W)
    tr = {k: v.cpu() for k, v in tr.items()}
    worst = 0.0
    for s in range(S):
        live_prev, prev = 1, torch.zeros(1)
        for p in range(9):
            want_live = min(W, live_prev * n_in)
            got_live = int(tr["live"][p, s])
            assert got_live == want_live, f"segment {s} position {p}: n_live {got_live}, defined {want_live}"
            cand64 = BR.candidates(prev, tr["logits"][p, s, :live_prev])
            parent, token, sc = (tr[k][p, s, :got_live] for k in ("parent", "token", "score"))
            assert bool(((parent >= 0) & (parent < live_prev) & (token >= 0) & (token < n_in)).all())
            flat = parent.long() * n_in + token.long()
            BR.band_check(cand64, flat, W, BAND, f"segment {s} position {p}")
            diff = float((sc.double() - cand64.reshape(-1)[flat]).abs().max())
            worst = max(worst, diff)
            assert diff <= TOL, f"segment {s} position {p}: traced score {diff:.3e} from float64"
            # rank order on the device's own float32 scores: non-increasing, ties by flat index, exactly
            up = sc[1:] > sc[:-1]
            tie_bad = (sc[1:] == sc[:-1]) & (flat[1:] <= flat[:-1])
            assert not bool(up.any()) and not bool(tie_bad.any()), f"segment {s} position {p}: survivors out of rank order"
            assert bool((tr["token"][p, s, got_live:] == -1).all()) and bool(torch.isinf(tr["score"][p, s, got_live:]).all())
            live_prev, prev = got_live, sc
        assert int(n_live[s]) == live_prev
        assert torch.equal(score[s, :live_prev].cpu(), prev), "the returned score is the last position's"
        assert bool((codes[s, live_prev:] == -1).all()) and bool((score[s, live_prev:] == float("-inf")).all())
        assert bool((codes[s, :live_prev] >= 0).all())
        assert codes[s, :live_prev].reshape(live_prev, 9).unique(dim=0).shape[0] == live_prev, "beams are distinct grids"
    print(f"{cfg} S={S} W={W}: largest traced-score distance to float64 {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SMALL + [FULL])
def test_width_one_is_greedy_decoding(cfg):
    _fp16_only()
    S = 3 if cfg == FULL else 5
    lab = _labels(cfg, S)
    codes, score, n_live = ops.pixelcnn_beam(_prior(cfg).packed(), lab, 1)
    q = torch.ones(S, 9, cfg[0], device=DEV)
    c, lm, _ = ops.pixelcnn_sample(_prior(cfg).packed(), lab, q, top_k=1, return_logp=True)
    assert torch.equal(codes.view(S, 9), c.view(S, 9))
    assert torch.equal(score.view(S), BR.left_to_right_sum(lm))
    assert bool((n_live == 1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,S,W", [(SMALL[0], 5, 64), (SMALL[1], 5, 100), (SMALL[1], 5, 3), (FULL, 3, 8)])
def test_replay_gives_the_same_bits(cfg, S, W):
    """Every final beam through the controlled sampler (all nine codes given) and the teacher-forced forward."""
    _fp16_only()
    n_in = cfg[0]
    lab, codes, score, n_live, tr = _run(cfg, S, W)
    pk = _prior(cfg).packed()
    live = (torch.arange(W, device=DEV)[None, :] < n_live[:, None])
    rows = live.reshape(-1).nonzero().reshape(-1)
    grids = codes.view(S * W, 9)[rows]
    labs = lab.repeat_interleave(W)[rows]
    _, lm, _ = ops.pixelcnn_sample(pk, labs, None, given=grids, return_logp=True)
    assert torch.equal(BR.left_to_right_sum(lm), score.view(-1)[rows]), "a beam's score is its replayed logp_model summed left to right"
    fwd = ops.pixelcnn_forward(pk, grids.view(-1, 3, 3), labs).reshape(-1, n_in, 9)
    # the traced logits of a final beam at position p: its ancestor's row BEFORE p's selection, i.e. the parent rank at p
    seg, rank = rows // W, rows % W
    for p in range(8, -1, -1):
        rank = tr["parent"][p][seg, rank].long()
        assert torch.equal(tr["logits"][p][seg, rank], fwd[:, :, p]), f"position {p}: traced logits differ from pixelcnn_forward"


@pytest.mark.gpu
def test_segments_are_independent():
    """Alone, in a batch, with the chunk knob splitting the batch, and in permuted order: the same bits."""
    _fp16_only()
    from test_gpu_parity import _with_env
    cfg, S, W = SMALL[1], 5, 64
    lab, codes, score, n_live, _ = _run(cfg, S, W)
    pk = _prior(cfg).packed()
    for s in (0, 3):
        c, sc, n = ops.pixelcnn_beam(pk, lab[s:s + 1].contiguous(), W)
        assert torch.equal(c[0], codes[s]) and torch.equal(sc[0], score[s]) and int(n[0]) == int(n_live[s])
    for chunk in (str(2 * W), "1", str(3 * W + 5)):
        c, sc, n = _with_env("DVQ_PIXELCNN_CHUNK", chunk, lambda: ops.pixelcnn_beam(pk, lab, W))
        assert torch.equal(c, codes) and torch.equal(sc, score) and torch.equal(n, n_live), f"DVQ_PIXELCNN_CHUNK={chunk}"
    c, sc, n = _with_env("DVQ_PIXELCNN_TABLES", "0", lambda: ops.pixelcnn_beam(pk, lab, W))
    assert torch.equal(c, codes) and torch.equal(sc, score) and torch.equal(n, n_live), "without the class tables: row 0 evaluated per row"
    perm = torch.tensor([3, 0, 4, 2, 1], device=DEV)
    c, sc, n = ops.pixelcnn_beam(pk, lab[perm].contiguous(), W)
    assert torch.equal(c, codes[perm]) and torch.equal(sc, score[perm]) and torch.equal(n, n_live[perm])


@pytest.mark.gpu
def test_nan_logits_end_their_segment_alone():
    """A class whose conditional embedding holds a NaN row: the segments of that class come out with n_live = 0, every code -1 and
    bit 2 set; their neighbours keep the bits of the clean weights.  A label out of range sets bit 0 and searches label 0."""
    _fp16_only()
    from dvqvae_amd.network.pixelcnn.models import GatedPixelCNN
    cfg, W = SMALL[0], 8
    clean = _prior(cfg)
    sick = GatedPixelCNN(*cfg)
    load_synth(sick, P.SIZES[cfg])
    with torch.no_grad():
        sick.layers[1].class_cond_embedding.weight[5] = float("nan")
    sick = sick.to(DEV)
    lab = torch.tensor([2, 5, 7, 5, 0], device=DEV)
    err = ops.new_err_flag(torch.device(DEV))
    c, sc, n, tr = ops.pixelcnn_beam(sick.packed(), lab, W, trace=True, err=err)
    assert int(err.item()) == 4
    assert n.tolist()[1] == 0 and n.tolist()[3] == 0 and bool((c[[1, 3]] == -1).all()) and bool((sc[[1, 3]] == float("-inf")).all())
    c0, sc0, n0 = ops.pixelcnn_beam(clean.packed(), lab, W)
    keep = [0, 2, 4]
    assert torch.equal(c[keep], c0[keep]) and torch.equal(sc[keep], sc0[keep]) and torch.equal(n[keep], n0[keep]) and n[keep].tolist() == [W] * 3
    with pytest.raises(RuntimeError, match=r"segments \[1, 3\]"):
        ops.pixelcnn_beam(sick.packed(), lab, W)
    err = ops.new_err_flag(torch.device(DEV))
    bad = torch.tensor([cfg[3], 3], device=DEV)
    c, sc, n = ops.pixelcnn_beam(clean.packed(), bad, W, err=err)
    assert int(err.item()) == 1
    c1, sc1, _ = ops.pixelcnn_beam(clean.packed(), torch.tensor([0, 3], device=DEV), W)
    assert torch.equal(c, c1) and torch.equal(sc, sc1)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.pixelcnn_beam(clean.packed(), bad, W)
    assert tuple(clean.beam_search(lab, 3)[0].shape) == (5, 3, 3, 3)


# ------------------------------------------------------------------------------------------ GPU: GenNet.gen_beam
@pytest.mark.gpu
def test_gen_beam_equals_gen_on_the_beams_codes():
    _fp16_only()
    from test_prior_controls import _gennet
    net = _gennet()
    S, W = 3, 8
    obj = synth.synthetic_clouds(S, 1024, seed=21).to(DEV)
    recon, pos, aux = net.gen_beam(obj, W, return_aux=True)
    assert tuple(recon.shape) == (S * W, 55) and tuple(pos.shape) == (S * W, 6) and tuple(aux["codes"].shape) == (S * W, 3, 3)
    assert aux["n_live"].tolist() == [W] * S and bool(torch.isfinite(recon).all())
    r2, p2, aux2 = net.gen(obj.repeat_interleave(W, 0), codes=aux["codes"], return_aux=True)
    assert torch.equal(recon, r2) and torch.equal(pos, p2) and torch.equal(aux["verts"], aux2["verts"])
    assert torch.equal(aux["codes"], aux2["codes"])
    assert torch.equal(aux["log_prob"], BR.left_to_right_sum(aux2["logp_model"]))
    assert torch.equal(aux["idx6"].repeat_interleave(W, 0), aux2["idx6"])
    lp = aux["log_prob"].view(S, W)
    assert bool((lp[:, :-1] >= lp[:, 1:]).all()), "rank order"
    want = BR.duplicate_of(aux["codes"].view(S, W, 9).cpu(), aux["n_live"].cpu(), SLOTS)
    assert torch.equal(aux["duplicate_of"].cpu(), want)
    a, b = net.gen_beam(obj, W)
    assert torch.equal(a, recon) and torch.equal(b, pos), "deterministic: no noise key"
    with pytest.raises(RuntimeError, match="width"):
        net.gen_beam(obj, 0)


# ------------------------------------------------------------------------------------------ GPU: the entry points
def _run_main(dataset, out_dir, extra, mano="/nonexistent"):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano,
                                            "--num_objects", "2", "--points", "256"])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
@pytest.mark.parametrize("dataset,P", [("ho3d", 2), ("obman", 1)])
def test_entry_point_writes_the_same_bytes_for_every_grouping(tmp_path, dataset, P):
    """One dataset that rotates (two poses) and one that does not: the files do not depend on --rows_per_call."""
    _fp16_only()
    import json
    W = 4
    base = ["--beam_width", str(W), "--beam_poses", str(P), "--num_grasp", str(P * W)]
    names0, bytes0 = _run_main(dataset, str(tmp_path / "loop"), base + ["--rows_per_call", "0"])
    assert names0 == ["obj_id_synthetic_0.json", "obj_id_synthetic_1.json"]
    for rpc in ("7", "16384"):
        names, data = _run_main(dataset, str(tmp_path / rpc), base + ["--rows_per_call", rpc])
        assert names == names0 and data == bytes0, f"--rows_per_call {rpc}: the files differ"
    for data in bytes0:
        j = json.loads(data)
        assert {"recon_params", "R_list", "trans_list", "r_list", "log_prob", "beam_pose", "beam_rank", "beam_duplicate_of"} <= set(j)
        assert j["beam_pose"] == [p for p in range(P) for _ in range(W)] and j["beam_rank"] == list(range(W)) * P
        assert all(len(j[k]) == P * W for k in ("recon_params", "log_prob", "beam_duplicate_of"))
        for p in range(P):
            lp = j["log_prob"][p * W:(p + 1) * W]
            assert lp == sorted(lp, reverse=True), "rank order within a pose"
            assert len({tuple(r) for r in j["r_list"][p * W:(p + 1) * W]}) == 1, "one rotation per pose"
            assert all(-1 <= d < r for r, d in enumerate(j["beam_duplicate_of"][p * W:(p + 1) * W]))
        if P == 2:
            assert j["r_list"][0] != j["r_list"][W]


@pytest.mark.gpu
def test_beam_poses_are_the_first_rotations_and_width_zero_is_the_run_without_the_flag(tmp_path):
    _fp16_only()
    import json
    plain_names, plain = _run_main("ho3d", str(tmp_path / "plain"), ["--num_grasp", "8"])
    names, zero = _run_main("ho3d", str(tmp_path / "zero"), ["--num_grasp", "8", "--beam_width", "0", "--beam_poses", "1"])
    assert names == plain_names and zero == plain, "--beam_width 0: the bytes of the run without the flag"
    _, beam = _run_main("ho3d", str(tmp_path / "beam"), ["--num_grasp", "8", "--beam_width", "4", "--beam_poses", "2"])
    for a, b in zip(beam, plain):
        ja, jb = json.loads(a), json.loads(b)
        assert ja["r_list"][0] == jb["r_list"][0] and ja["r_list"][4] == jb["r_list"][1], "pose p takes the rotation of grasp row p"
        assert ja["R_list"][4] == jb["R_list"][1]


@pytest.mark.gpu
def test_selection_by_log_prob_keeps_rank_order_within_a_pose(tmp_path):
    _fp16_only()
    import json
    from test_grasp_select import mano_pkl
    _, data = _run_main("ho3d", str(tmp_path / "sel"), ["--num_grasp", "5", "--candidates", "8", "--select_by", "log_prob",
                                                      "--beam_width", "4", "--beam_poses", "2"], mano_pkl(tmp_path))
    for d in data:
        j = json.loads(d)
        assert len(j["candidate"]) == 5 and j["log_prob"] == sorted(j["log_prob"], reverse=True)
        assert j["beam_pose"] == [c // 4 for c in j["candidate"]] and j["beam_rank"] == [c % 4 for c in j["candidate"]]
        for p in range(2):
            ranks = [r for q, r in zip(j["beam_pose"], j["beam_rank"]) if q == p]
            assert ranks == list(range(len(ranks))), "a pose's kept grasps are its best ranks, in rank order"
