"""Grasp stability proxy: the fused contact-wrench kernel (dvq_grasp_wrench), its host API (ops.grasp_wrench, contact.grasp_stability,
contact.wrench_stats, select_keys("stability")) and the ``--select_by stability`` / ``--stability`` mode of the entry points.  The
reference is tests/grasp_wrench_ref.py (numpy over oracle/contact_oracle.py, the canonical reduction of tests/grasp_score_ref.py);
GPU results are compared with it bit for bit."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops, synth

import grasp_score_ref as score_ref
import grasp_wrench_ref as ref

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
LENGTH, THR = 0.1, 0.02 ** 2
FIELDS = ("force_residual", "torque_residual", "min_sv", "stability_key")
OUTPUTS = ("penetration", "n_interior", "n_contact", "centre", "sums", "key")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_stability_flags(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.select_by, a.stability, a.torque_length) == ("penetration", 0, 0.1) and a.max_penetration == INF
    a = generate.parse_args(dataset, ["--select_by", "stability", "--max_penetration", "0.002", "--torque_length", "0.05",
                                      "--stability", "1", "--candidates", "200", "--num_grasp", "100"])
    assert (a.select_by, a.max_penetration, a.torque_length, a.stability) == ("stability", 0.002, 0.05, 1)
    for bad in (["--torque_length", "0"], ["--torque_length", "inf"], ["--torque_length", "nan"], ["--max_penetration", "-1"],
                ["--max_penetration", "nan"]):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_grasp_wrench" in _lib.SIGNATURES and "int dvq_grasp_wrench(" in header and hasattr(lib, "dvq_grasp_wrench")
    assert "dvq_grasp_wrench" in re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert len(_lib.SIGNATURES["dvq_grasp_wrench"][1]) == 20                           # dvq_grasp_scores' 16 + inv_length + three outputs


def test_ops_refuse_bad_arguments_before_any_device_use():
    v, f = score_ref.sphere_mesh(4, 6)
    faces, off, vf = (torch.from_numpy(a) for a in contact.face_csr(f, len(v)))
    hand = torch.from_numpy(v)[None].contiguous()
    obj = torch.zeros(1, 5, 3)
    good = dict(hand=hand, faces=faces, vf_off=off, vf_face=vf, obj=obj, inv_length=10.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_wrench(**good)                                                     # well-formed, but not on a device
    for bad in (dict(hand=torch.zeros(1, 2049, 3), vf_off=torch.zeros(2050, dtype=torch.int32)),     # V > 2048
                dict(obj=torch.zeros(1, 0, 3)),                                                      # N = 0
                dict(hand=hand.transpose(1, 2)), dict(hand=hand.expand(2, -1, -1), obj=torch.zeros(2, 5, 3)),   # not contiguous
                dict(hand=hand.double()), dict(obj=obj.double()), dict(faces=faces.long()),                     # wrong dtype
                dict(hand=torch.zeros(1, 0, 3), vf_off=off[:1]), dict(vf_off=off[:-1]), dict(obj=torch.zeros(2, 5, 3)),
                dict(inv_length=0.0), dict(inv_length=INF), dict(inv_length=NAN)):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_wrench(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    topo = type("T", (), dict(faces=faces, vf_off=off, vf_face=vf))
    for length in (0.0, -0.1, INF, NAN):
        with pytest.raises(RuntimeError, match="length"):
            contact.grasp_stability(topo, hand, obj, length=length)


# ------------------------------------------------------------------------------------------------------ CPU: the reference itself
@pytest.fixture(scope="module")
def sphere_cases():
    """The closed sphere of radius 0.05 as the hand against 1000 points at radius 0.06: all of them, the cap z > 0.8, and the shell
    1 m away.  Computed once."""
    v, f = score_ref.sphere_mesh()
    dirs = ref.unit_directions(1000, 0)
    shell = (0.06 * dirs).astype(np.float32)
    clouds = {"shell": shell, "cap": shell[dirs[:, 2] > 0.8], "far": (shell + np.float32(1.0)).astype(np.float32)}
    return {k: ref.grasp_wrench(v[None], f, o[None], 1.0 / LENGTH, THR) for k, o in clouds.items()}


def test_reference_on_the_closed_sphere(sphere_cases):
    shell, cap, far = (sphere_cases[k] for k in ("shell", "cap", "far"))
    assert shell["n_contact"].tolist() == [1000] and cap["n_contact"].tolist() == [96] and far["n_contact"].tolist() == [0]
    stats = {k: contact.wrench_stats(r["sums"], r["n_contact"]) for k, r in sphere_cases.items()}
    print({k: (s, sphere_cases[k]["key"]) for k, s in stats.items()})
    assert stats["shell"]["force_residual"][0] < 0.15                   # contacts all round: the unit forces cancel (measured 0.057)
    assert stats["cap"]["force_residual"][0] > 0.7                      # contacts on one side: they add up (measured 0.89)
    assert shell["key"][0] < cap["key"][0] < INF                        # ... and the enclosing hand ranks first
    assert all(0.0 <= s["force_residual"][0] <= 1.0 for s in (stats["shell"], stats["cap"]))
    assert all(stats["far"][k] == [None] for k in FIELDS[:3]) and far["key"][0] == INF and bits(far["sums"]).max() == 0
    # the net force of the key is the float64 statistic squared, up to fp32 rounding; the torque part is the rest
    for r, s in ((shell, stats["shell"]), (cap, stats["cap"])):
        assert math.isclose(float(r["key"][0]), s["force_residual"][0] ** 2 + s["torque_residual"][0] ** 2, rel_tol=1e-5)


def test_wrench_stats_equal_an_independent_float64_computation(sphere_cases):
    rng = np.random.default_rng(5)
    w = rng.normal(size=(4, 40, 6))
    w[3, :, 3:] *= 1e-4                                                 # near-zero torque rows: a tiny smallest eigenvalue
    n = np.asarray([40, 7, 1, 40])
    sums = np.zeros((6, 27))
    for b in range(4):
        x = w[b, :n[b]]
        sums[b, :6] = x.sum(0)
        sums[b, 6:] = [np.sum(x[:, a] * x[:, e]) for a, e in ref.PAIRS]
    sums[4] = sphere_cases["shell"]["sums"][0]
    sums[5] = sphere_cases["cap"]["sums"][0]
    n = np.concatenate([n, [1000, 96]])
    sums, n = np.concatenate([sums, np.ones((1, 27))]), np.concatenate([n, [0]])      # and a grasp that touches nothing
    got = contact.wrench_stats(torch.from_numpy(sums.astype(np.float32)), torch.from_numpy(n.astype(np.int32)))
    want = ref.wrench_stats(sums.astype(np.float32), n)
    assert [len(got[k]) for k in FIELDS[:3]] == [7, 7, 7]
    for b, wb in enumerate(want):
        if wb is None:
            assert all(got[k][b] is None for k in FIELDS[:3])
            continue
        force, torque, lam, trace = wb
        assert abs(got["force_residual"][b] - force) <= 1e-12 * force and abs(got["torque_residual"][b] - torque) <= 1e-12 * torque
        # lambda_min to the float64 backward error of a symmetric 6x6 eigenproblem: 1e-12 * trace(G / n), absolute
        lam_got = got["min_sv"][b] ** 2
        print(b, lam_got, lam, trace)
        assert abs(lam_got - max(lam, 0.0)) <= 1e-12 * trace
    assert json.loads(json.dumps(got))["min_sv"][6] is None            # json: null
    assert contact.wrench_stats(np.full((1, 27), NAN), [3]) == {k: [None] for k in FIELDS[:3]}


def test_select_keys_by_stability():
    scores = {"penetration": torch.tensor([0.5, 0.0, NAN, 0.25, 2.0, 0.0, 1.0, 0.0]),
              "n_interior": torch.zeros(8, dtype=torch.int32),
              "n_contact": torch.tensor([3, 0, 9, 2, 2, 1, 7, 4], dtype=torch.int32),
              "key": torch.tensor([0.3, INF, NAN, 0.1, 0.0, 0.1, 0.2, 0.9])}
    cls, key = contact.select_keys(scores, "stability", 1)
    assert cls.dtype == torch.int32 and key.dtype == torch.float32 and torch.equal(key.isnan(), scores["key"].isnan())
    assert cls.tolist() == [0, 1, 2, 0, 0, 0, 0, 0]                     # the three classes; max_penetration defaults to +inf
    assert score_ref.segment_topk(cls.numpy(), key.numpy(), 1, 8, 8)[0].tolist() == [4, 3, 5, 6, 0, 7, 1, 2]
    cls, _ = contact.select_keys(scores, "stability", 3)               # min_contact = 3: candidates 3, 4, 5 drop a class
    assert cls.tolist() == [0, 1, 2, 1, 1, 1, 0, 0]
    cls, key = contact.select_keys(scores, "stability", 1, max_penetration=0.5)      # 0.5 itself passes; 2.0 and 1.0 do not
    assert cls.tolist() == [0, 1, 2, 0, 1, 0, 1, 0]
    assert score_ref.segment_topk(cls.numpy(), key.numpy(), 1, 8, 8)[0].tolist() == [3, 5, 0, 7, 4, 6, 1, 2]
    cls, _ = contact.select_keys(scores, "stability", 1, max_penetration=0.0)
    assert cls.tolist() == [1, 1, 2, 1, 1, 0, 1, 0]
    # the other modes return what they returned: max_penetration is not theirs
    pen_cls, pen_key = contact.select_keys(scores, "penetration", 1, max_penetration=0.0)
    assert pen_cls.tolist() == [0, 1, 2, 0, 0, 0, 0, 0] and pen_key is scores["penetration"]
    lp = torch.tensor([-3.0, -1.0, NAN, -1.0])
    lp_cls, lp_key = contact.select_keys({}, "log_prob", 1, log_prob=lp)
    assert lp_cls.tolist() == [0, 0, 2, 0] and torch.equal(lp_key[[0, 1, 3]], -lp[[0, 1, 3]])
    assert contact.SELECT_BY == ("penetration", "log_prob", "stability")
    with pytest.raises(RuntimeError):
        contact.select_keys(scores, "volume", 1)


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def wrench_case(name, tmp_path):
    """(hand [B,V,3], faces, obj [B,N,3]) numpy fp32, built as tests/test_grasp_select.py builds score_case: points on both sides
    of the surface, some within the contact threshold, some not."""
    from test_grasp_select import mano_faces
    rng = lambda tag, shape, scale: synth.synthetic_normal(shape, 41, f"wrench/{name}/{tag}", scale).numpy()
    B, N, V = (int(x) for x in name.split("x"))
    if name == "1x1x1":                                                  # one vertex, one degenerate face (its normal is 0), one point in contact
        hand = rng("h", (1, 1, 3), 0.1)
        return hand, np.zeros((1, 3), np.int64), (hand + rng("o", (1, 1, 3), 0.005)).astype(np.float32)
    if V == 776:
        v, f = score_ref.sphere_mesh()
        scale = np.linspace(0.8, 1.2, B).astype(np.float32)[:, None, None]
        hand = (v[None] * scale + rng("h", (B, len(v), 3), 0.002)).astype(np.float32)
        return hand, f, rng("o", (B, N, 3), 0.04)
    f, v = mano_faces(tmp_path)                                           # the MANO template itself, the cloud about its centre
    hand = (v[None] + rng("h", (B, 778, 3), 0.001)).astype(np.float32)
    return hand, f, (v.mean(0, keepdims=True)[None] + rng("o", (B, N, 3), 0.03)).astype(np.float32)


def run_wrench(hand, faces, obj_dev, length=LENGTH, thr=THR):
    topo = contact.HandTopology(faces, hand.shape[1], DEV)
    out = contact.grasp_stability(topo, gpu(hand), obj_dev, length, thr)
    assert tuple(out) == OUTPUTS
    B = hand.shape[0]
    assert tuple(out["centre"].shape) == (B, 3) and tuple(out["sums"].shape) == (B, 27) and tuple(out["key"].shape) == (B,)
    assert all(out[k].dtype == (torch.int32 if k.startswith("n_") else torch.float32) for k in OUTPUTS)
    return topo, {k: v.cpu().numpy() for k, v in out.items()}


def assert_same_bits(got, want, rows=None, what=""):
    """Every number bit for bit; a NaN is a NaN (its payload is nobody's contract)."""
    for k in OUTPUTS:
        g, w = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        if k.startswith("n_"):
            assert np.array_equal(g, w), (what, k, g, w)
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, k, g, w)
        assert np.array_equal(bits(g)[~nan], bits(w)[~nan]), (what, k, g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1x1", "3x255x776", "3x256x776", "2x257x778", "2x1000x778"])
def test_grasp_wrench_equals_the_reference_bit_for_bit(name, tmp_path):
    hand, faces, obj = wrench_case(name, tmp_path)
    N = obj.shape[1]
    topo, got = run_wrench(hand, faces, gpu(obj))
    want = ref.grasp_wrench(hand, faces, obj, 1.0 / LENGTH, THR)
    print("n_contact", got["n_contact"], want["n_contact"], "key", got["key"], want["key"], "sums", got["sums"][0], want["sums"][0])
    assert_same_bits(got, want, what=name)
    if name == "1x1x1":
        assert want["n_contact"].tolist() == [1] and want["key"].tolist() == [0.0]    # N = 1 leaves no room for 0 < n < N
    else:
        assert ((0 < want["n_contact"]) & (want["n_contact"] < N)).any(), "no row has some points in contact and some not"
        assert (want["n_interior"] > 0).any() and (want["n_interior"] < N).any() and np.abs(want["sums"]).min(axis=0).max() > 0
        assert np.isfinite(want["key"]).all() and (want["key"] > 0).all()
    # the three scores carry the bits of dvq_grasp_scores on the same inputs
    scores = contact.grasp_scores(topo, gpu(hand), gpu(obj), THR)
    for k in ("penetration", "n_interior", "n_contact"):
        assert np.array_equal(scores[k].cpu().numpy().view(np.uint32), got[k].view(np.uint32)), k
    # and the float64 statistics of the kernel's sums are those of the reference's
    assert contact.wrench_stats(got["sums"], got["n_contact"]) == contact.wrench_stats(want["sums"], want["n_contact"])


@pytest.mark.gpu
def test_grasp_wrench_reads_a_channel_first_view_in_place():
    v, f = score_ref.sphere_mesh()
    B, N = 3, 500
    cloud = synth.synthetic_normal((B, 4, N), 42, "wrench/cf", 0.04)                    # [B,4,N] as the generation path holds it
    hand = (v[None] * np.asarray([1.0, 0.9, 1.1], np.float32)[:, None, None]).astype(np.float32)
    view = gpu(cloud)[:, :3].transpose(1, 2)                                             # strides (4N, 1, N)
    assert not view.is_contiguous()
    _, got = run_wrench(hand, f, view)
    _, copy = run_wrench(hand, f, view.contiguous())
    obj = cloud[:, :3].transpose(1, 2).contiguous().numpy()
    want = ref.grasp_wrench(hand, f, obj, 1.0 / LENGTH, THR)
    assert ((0 < want["n_contact"]) & (want["n_contact"] < N)).any()
    assert_same_bits(got, want, what="view")
    assert_same_bits(got, copy, what="view against its contiguous copy")


@pytest.mark.gpu
def test_grasp_wrench_with_a_nan_row_and_rows_alone():
    v, f = score_ref.sphere_mesh()
    B, N = 4, 300
    hand = (v[None] * np.linspace(0.9, 1.1, B).astype(np.float32)[:, None, None]).astype(np.float32)
    obj = synth.synthetic_normal((B, N, 3), 43, "wrench/nan", 0.04).numpy()
    _, clean = run_wrench(hand, f, gpu(obj))
    assert ((0 < clean["n_contact"]) & (clean["n_contact"] < N)).all() and np.isfinite(clean["key"]).all()
    bad = obj.copy()
    bad[1, 17, 2] = np.nan                                                               # a NaN object coordinate: row 1
    _, got = run_wrench(hand, f, gpu(bad))
    assert np.isnan(got["key"][1]) and np.isnan(got["penetration"][1])
    cls, key = contact.select_keys({k: torch.from_numpy(x) for k, x in got.items()}, "stability", 1)
    assert cls.tolist() == [0, 2, 0, 0] and np.isnan(key[1].item())
    assert_same_bits(got, clean, rows=[0, 2, 3], what="the rows beside the NaN row")
    assert_same_bits(got, ref.grasp_wrench(hand, f, bad, 1.0 / LENGTH, THR), what="nan")
    assert contact.wrench_stats(got["sums"], got["n_contact"])["force_residual"][1] is None
    for b in range(B):                                                                   # a row alone gives the bits it has inside the batch
        _, one = run_wrench(hand[b:b + 1], f, gpu(bad[b:b + 1]))
        assert_same_bits(one, {k: x[b:b + 1] for k, x in got.items()}, what=f"row {b} alone")
    # another length scales the torques and leaves the forces alone
    _, short = run_wrench(hand, f, gpu(obj), length=0.05)
    assert np.array_equal(bits(short["sums"][:, :3]), bits(clean["sums"][:, :3])) and not np.array_equal(short["sums"][:, 3:6], clean["sums"][:, 3:6])


@pytest.mark.gpu
def test_grasp_wrench_across_the_chunk_seam():
    """B = 65 537 grasps in two launches (65 535 + 2): the rows at the seam equal the reference."""
    B, rows = 65537, [0, 65534, 65535, 65536]
    tetra = np.asarray([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.05, 0.0], [0.0, 0.0, 0.05]], np.float32)
    faces = np.asarray([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)
    hand = (tetra[None] + synth.synthetic_normal((B, 4, 3), 44, "wrench/seam/h", 0.005).numpy()).astype(np.float32)
    near = hand[np.arange(B), np.arange(B) % 4][:, None]                                 # row b's point sits at its vertex b mod 4
    obj = (near + synth.synthetic_normal((B, 1, 3), 44, "wrench/seam/o", 0.005).numpy()).astype(np.float32)
    _, got = run_wrench(hand, faces, gpu(obj))
    want = ref.grasp_wrench(hand[rows], faces, obj[rows], 1.0 / LENGTH, THR)
    assert want["n_contact"].tolist() == [1, 1, 1, 1] and (want["key"] > 0.5).all() and len({x.tobytes() for x in want["sums"]}) == 4
    assert_same_bits({k: x[rows] for k, x in got.items()}, want, what="seam")
    assert set(np.unique(got["n_contact"]).tolist()) <= {0, 1} and got["n_contact"].mean() > 0.9    # N = 1; a 4-sigma offset misses
    assert np.array_equal(np.isinf(got["key"]), got["n_contact"] == 0)
    topo = contact.HandTopology(faces, 4, DEV)
    empty = contact.grasp_stability(topo, gpu(hand)[:0].contiguous(), gpu(obj)[:0].contiguous())
    assert [tuple(empty[k].shape) for k in OUTPUTS] == [(0,), (0,), (0,), (0, 3), (0, 27), (0,)]


@pytest.mark.gpu
def test_grasp_wrench_refuses_what_the_kernel_cannot_hold():
    v, f = score_ref.sphere_mesh(4, 6)
    topo = contact.HandTopology(f, len(v), DEV)
    hand = gpu(v)[None].contiguous()
    with pytest.raises(RuntimeError):
        contact.grasp_stability(topo, hand, torch.zeros(1, 0, 3, device=DEV))
    with pytest.raises(RuntimeError):
        contact.grasp_stability(topo, hand, torch.zeros(2, 4, 3, device=DEV))
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL, nothing launched
    one = torch.full((32,), 7.0, device=DEV)
    for V, N, B in ((2049, 4, 1), (0, 4, 1), (5, 0, 1), (5, 4, -1)):
        rc = lib.dvq_grasp_wrench(one.data_ptr(), topo.faces.data_ptr(), topo.vf_off.data_ptr(), topo.vf_face.data_ptr(), V,
                                  one.data_ptr(), 0, 3, 1, B, N, 0.0004, 10.0, one.data_ptr(), one.data_ptr(), one.data_ptr(),
                                  one.data_ptr(), one.data_ptr(), one.data_ptr(), None)
        assert rc == 1, (V, N, B)
    assert (one == 7.0).all()                                           # nothing was written


# ------------------------------------------------------------------------------------------------------ GPU: end to end
E2E_SEED, E2E_M, E2E_K = 9, 8, 3
E2E_INDICES = [5, 2, 11, 7]


def e2e_clouds():
    """Four small [N,3] clouds of two point counts: three cubes of points about the place where the synthetic weights put every hand
    (tests/test_grasp_select.py: e2e_objects), and one a metre away, which no hand touches."""
    centre = np.asarray([-0.08, -0.09, 0.13])
    clouds = [synth.synthetic_uniform((n, 3), 80 + i, "wrench/e2e", -0.1, 0.1).numpy().astype(np.float64) + centre
              for i, n in enumerate((300, 200, 300, 200))]
    clouds[3] = clouds[3] + 1.0
    return clouds


@pytest.mark.gpu
def test_best_of_m_by_stability_keeps_the_reference_order(tmp_path):
    from test_grasp_select import _gennet
    net = _gennet(tmp_path)
    objs = [generate.object_tensor(c) for c in e2e_clouds()]
    M, k = E2E_M, E2E_K
    plain = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES)
    faces = np.asarray(net.rh_mano.faces)
    dumped, varied, beyond = {}, False, False
    for rows_per_call in (16384, 8, 1):
        got = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, rows_per_call=rows_per_call, candidates=M,
                                            select_by="stability", min_contact=1)
        for i, (g, p) in enumerate(zip(got, plain)):
            c = g["candidate"].cpu().numpy()
            scores = {name: t.cpu() for name, t in g["scores"].items()}
            assert set(scores) == set(OUTPUTS) and tuple(scores["sums"].shape) == (M, 27)
            cls, key = contact.select_keys(scores, "stability", 1)
            assert np.array_equal(c, score_ref.segment_topk(cls.numpy(), key.numpy(), 1, M, k)[0]), f"object {i}: order"
            assert torch.equal(g["params"], p["params"][g["candidate"]]) and torch.equal(g["vertices"], p["vertices"][g["candidate"]])
            if rows_per_call == 16384:                                  # the keys are the reference's on the plain run's hands
                want = ref.grasp_wrench(p["vertices"].cpu().numpy(), faces, np.repeat(objs[i][:3].T.numpy()[None], M, 0), 1.0 / LENGTH, THR)
                assert_same_bits({name: t.numpy() for name, t in scores.items()}, want, what=f"object {i}")
            j = g["json"]
            assert list(j)[-7:] == ["penetration", "n_interior", "n_contact"] + list(FIELDS) and all(len(j[f]) == k for f in FIELDS)
            stats = contact.wrench_stats(scores["sums"][c], scores["n_contact"][c])
            for f in FIELDS[:3]:
                assert j[f] == stats[f]
            assert j["stability_key"] == [float(x) if math.isfinite(x) else None for x in scores["key"][c].tolist()]
            for r in range(k):                                          # null exactly where the hand touches nothing
                assert all((j[f][r] is None) == (j["n_contact"][r] == 0) for f in FIELDS)
            assert torch.equal(g["wrench_sums"].cpu(), scores["sums"][c]) and torch.equal(g["stability_key"].cpu(), scores["key"][c])
            varied |= len(set(key.tolist())) >= 3
            beyond |= bool((c >= k).any())
            print(f"rows_per_call {rows_per_call} object {i}: kept {c.tolist()} keys {key.tolist()} n_contact {scores['n_contact'].tolist()}")
        text = [json.dumps(g["json"]) for g in got]
        assert "Infinity" not in "".join(text) and "NaN" not in "".join(text)
        dumped[rows_per_call] = text
    assert dumped[8] == dumped[16384] and dumped[1] == dumped[16384]
    assert "null" in dumped[16384][3] and "null" not in "".join(dumped[16384][:3]), "the far object's hands touch nothing, the others' do"
    assert varied and beyond, "the selection is not exercised"
    # stability=True writes the figures without selecting by them: the grasps of the penetration run, plus the four fields ...
    by_pen = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, candidates=M)
    both = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, candidates=M, stability=True)
    for g, p in zip(both, by_pen):
        j, q = g["json"], p["json"]
        assert {f: j[f] for f in q} == q and list(j)[len(q):] == list(FIELDS) and torch.equal(g["params"], p["params"])
        assert set(p["scores"]) == {"penetration", "n_interior", "n_contact"} and "wrench_sums" not in p
    # ... and without candidates: every grasp generated, with the three scores and the four fields
    figures = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES, stability=True, torque_length=LENGTH)
    for i, (g, p) in enumerate(zip(figures, plain)):
        j, q = g["json"], p["json"]
        assert {f: j[f] for f in q} == q and list(j)[len(q):] == ["penetration", "n_interior", "n_contact"] + list(FIELDS)
        assert torch.equal(g["params"], p["params"]) and tuple(g["wrench_sums"].shape) == (M, 27)
        full = got[i]["scores"]                                         # of the last best-of-M run above: all M candidates
        assert torch.equal(g["wrench_sums"], full["sums"]) and torch.equal(g["stability_key"].isinf(), full["key"].isinf())
        assert j["n_contact"] == full["n_contact"].tolist() and all((j[f][r] is None) == (j["n_contact"][r] == 0) for f in FIELDS for r in range(M))
    # max_penetration moves candidates to class 1: the kept set changes where a kept candidate penetrates more than the limit
    g0 = generate.generate_for_objects(net, objs[:1], k, False, E2E_SEED, E2E_INDICES[:1], candidates=M, select_by="stability")[0]
    pen = g0["scores"]["penetration"].cpu()
    limit = float(pen.median())
    g1 = generate.generate_for_objects(net, objs[:1], k, False, E2E_SEED, E2E_INDICES[:1], candidates=M, select_by="stability",
                                       max_penetration=limit)[0]
    cls, key = contact.select_keys({n: t.cpu() for n, t in g1["scores"].items()}, "stability", 1, max_penetration=limit)
    assert set(cls.tolist()) == {0, 1}
    assert np.array_equal(g1["candidate"].cpu().numpy(), score_ref.segment_topk(cls.numpy(), key.numpy(), 1, M, k)[0])


def _run_main(dataset, out_dir, extra, mano):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
def test_entry_point_writes_the_stability_fields(tmp_path):
    from test_grasp_select import mano_pkl
    mano = mano_pkl(tmp_path)
    files = []
    for i, c in enumerate(e2e_clouds()):
        files.append(str(tmp_path / f"cloud{i}.npy"))
        np.save(files[-1], c)
    base = ["--objects"] + files + ["--num_grasp", str(E2E_K), "--candidates", str(E2E_M)]
    stab = base + ["--select_by", "stability"]
    names0, bytes0 = _run_main("obman", str(tmp_path / "s16384"), stab + ["--rows_per_call", "16384"], mano)
    assert names0 == [f"obj_id_cloud{i}.json" for i in range(4)]
    for tag in ("0", "8"):
        names, data = _run_main("obman", str(tmp_path / f"s{tag}"), stab + ["--rows_per_call", tag], mano)
        assert names == names0 and data == bytes0, f"--rows_per_call {tag}: the files differ"
    for i, data in enumerate(bytes0):
        j = json.loads(data)                                            # strict JSON: no Infinity, no NaN
        assert b"Infinity" not in data and b"NaN" not in data
        assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact", *FIELDS}
        assert all(len(j[f]) == E2E_K for f in FIELDS)
        assert all((j[f][r] is None) == (j["n_contact"][r] == 0) for f in FIELDS for r in range(E2E_K))
        keys = [INF if x is None else x for x in j["stability_key"]]
        assert keys == sorted(keys) and ((i == 3) == (j["n_contact"] == [0] * E2E_K))


@pytest.mark.gpu
def test_entry_point_without_the_flags_writes_the_parents_bytes(tmp_path):
    """``--stability 0 --select_by penetration`` (and values for the two dependent flags) against a run that omits them all: the
    code path of the parent commit, the same bytes."""
    from test_grasp_select import mano_pkl
    mano = mano_pkl(tmp_path)
    files = []
    for i, c in enumerate(e2e_clouds()):
        files.append(str(tmp_path / f"cloud{i}.npy"))
        np.save(files[-1], c)
    base = ["--objects"] + files + ["--num_grasp", str(E2E_K), "--candidates", str(E2E_M)]
    names0, plain = _run_main("obman", str(tmp_path / "plain"), base, mano)
    names, off = _run_main("obman", str(tmp_path / "off"), base + ["--stability", "0", "--select_by", "penetration", "--max_penetration", "0.5",
                                                                   "--torque_length", "0.3"], mano)
    assert names == names0 and off == plain
    assert all(set(json.loads(d)) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact"}
               for d in plain)
