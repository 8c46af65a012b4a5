"""Gradient refinement of grasps: the fused loss-and-gradient kernel (dvq_grasp_ttt), its host API (ops.grasp_ttt,
contact.ContactTargets / ttt_terms / ttt_loss / ttt_value_and_grad / refine_ttt) and the ``--ttt_*`` flags of the entry points.

Two restatements in tests/grasp_ttt_ref.py: numpy fp32 over oracle/contact_oracle (device results are compared with it bit for bit)
and a torch float64 one of the published loss, differentiated by autograd, which the CPU group pins to the values recorded from the
reference (tests/golden/g10_ttt_contact.npz, tools/record_ttt_golden.py) and to central differences.

End to end through the MANO layer the tolerance follows tests/test_mano_backward.py: ``e32`` is the error of the float32 CPU
restatement's gradient against the float64 one under the same frozen masks, pooled over the rows; the device must be within
``8 * e32``.  The comparison prints a ``ttt-grad-ratio`` line; DESIGN.md records the worst."""
import functools
import json
import lzma
import os
import re
import types

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, mano as dmano, ops, synth

import grasp_score_ref as score_ref
import grasp_ttt_ref as ref
import mano_grad_ref as gref
import mano_ref

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
gpu = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24
FACTOR = 8.0
W_PEN, W_CON = 840.0, 7500.0
GROUPS = (("betas", slice(0, 10)), ("orient", slice(10, 13)), ("pose", slice(13, 58)), ("transl", slice(58, 61)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, what=""):
    """Every number bit for bit; a NaN is a NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype != np.float32:
        assert np.array_equal(got, want), (what, got, want)
        return
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, got, want)
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), (what, np.abs(got[~nan] - want[~nan]).max())


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(HERE, "golden", "g10_ttt_contact.npz")) as z:
        return {k: z[k] for k in z.files}


def prior():
    """The reference's contact vertices, ascending."""
    return np.sort(golden()["prior_idx"].astype(np.int64))


@functools.lru_cache(maxsize=None)
def mano_arrays():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "MANO_RIGHT.pkl")
        with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
        return dmano.read_mano_pkl(path)


def mano_faces():
    return np.asarray(mano_arrays()["faces"], np.int64)


def params61(B, tag):
    """[B,61] fp32: betas | global_orient | hand_pose | transl of plausible hands."""
    return torch.cat([synth.synthetic_normal((B, 10), 91, f"ttt/{tag}/betas", 1.0), synth.synthetic_normal((B, 3), 91, f"ttt/{tag}/go", 1.0),
                      synth.synthetic_normal((B, 45), 91, f"ttt/{tag}/pose", 0.6), synth.synthetic_normal((B, 3), 91, f"ttt/{tag}/tr", 0.2)], 1)


def posed(p):
    """float64 [B,778,3]: the float64 reference of tests/mano_ref.py on parameters [B,61]."""
    p = p.double().numpy()
    return mano_ref.mano_ref(mano_ref.device_arrays(mano_arrays()), p[:, :10], p[:, 13:58], p[:, 10:13], p[:, 58:61])[0]


def cloud_near(hand, N, tag, sigma=0.01):
    """[B,N,3] fp32: hand vertices drawn at random, moved by N(0, sigma^2): about half of the points behind the surface, most within 2 cm."""
    B, V = hand.shape[:2]
    rng = np.random.default_rng([92, N, V, sum(map(ord, tag))])
    pick = rng.integers(0, V, size=(B, N))
    return (np.take_along_axis(np.asarray(hand, np.float64), pick[..., None], 1) + rng.normal(0, sigma, (B, N, 3))).astype(f32)


def bipyramid():
    """A closed mesh of 5 vertices and 6 faces, outward winding: three on the equator, two apexes."""
    v = np.asarray([[0.03, 0.0, 0.0], [-0.015, 0.026, 0.0], [-0.015, -0.026, 0.0], [0.0, 0.0, 0.04], [0.0, 0.0, -0.04]], f32)
    f = np.asarray([[0, 1, 3], [1, 2, 3], [2, 0, 3], [1, 0, 4], [2, 1, 4], [0, 2, 4]], np.int64)
    return v, f


@functools.lru_cache(maxsize=None)
def mesh(V):
    if V == 5:
        return bipyramid()
    if V == 776:
        return score_ref.sphere_mesh()
    if V == 2048:
        return score_ref.sphere_mesh(31, 66)
    raise AssertionError(V)


def hands_of(V, B, tag):
    """[B,V,3] fp32 and the faces: the mesh of V vertices under B small random distortions, or B posed hands of the real model."""
    if V == 778:
        return posed(params61(B, tag)).astype(f32), mano_faces()
    v, f = mesh(V)
    assert v.shape[0] == V
    jitter = synth.synthetic_normal((B, V, 3), 93, f"ttt/{tag}/{V}", 0.002).numpy()
    return (v[None] + jitter).astype(f32), f


# ========================================================================================== CPU group
def test_f64_restatement_equals_the_recorded_reference():
    """The reference's Contact_loss (recorded, float64) is 3000 * contact_sum / (B * n) of the restatement under the recorded mask."""
    g = golden()
    assert g["prior_idx"].shape == (204,) and len(set(g["prior_idx"].tolist())) == 204 and os.path.getsize(os.path.join(HERE, "golden", "g10_ttt_contact.npz")) < 100 * 1024
    for k in (0, 1):
        hand = torch.from_numpy(g[f"hand{k}"])[None].clone().requires_grad_(True)
        obj, mask = torch.from_numpy(g[f"obj{k}"])[None], g[f"mask{k}"]
        assert hand.dtype == torch.float64 and tuple(hand.shape) == (1, 778, 3) and tuple(obj.shape) == (1, 64, 3) and mask.sum() >= 8
        _, con, n = ref.ttt_terms_t(hand, mano_faces(), obj, prior(), frozen={"contact": mask[None]})
        assert int(n) == int(mask.sum())
        loss = 3000.0 * con[0] / (1 * n[0])
        grad, = torch.autograd.grad(loss, hand)
        want, wgrad = float(g[f"loss{k}"]), g[f"grad{k}"]
        assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want), (float(loss.detach()), want)
        err = float(np.abs(grad[0].numpy() - wgrad).max())
        assert np.abs(wgrad).max() > 1.0 and err <= 1e-12 * np.abs(wgrad).max(), err
        # the mask the reference's TTT_loss would pass is the restatement's own
        assert np.array_equal(ref.masks_t(hand.detach(), mano_faces(), obj, prior())["contact"][0].numpy(), mask)


def _tie_free_case():
    """Two distorted coarse spheres (V = 26) with 40 points each, none within 1e-5 of a Voronoi boundary (of all vertices or of the
    targets), of its nearest vertex's tangent plane, or of the contact threshold."""
    v, faces = score_ref.sphere_mesh(4, 6)
    V, B, N = v.shape[0], 2, 40
    rng = np.random.default_rng(94)
    hand = v[None].astype(np.float64) + rng.normal(0, 0.003, (B, V, 3))
    targets = np.arange(0, V, 2)
    objs = []
    for b in range(B):
        cand = rng.normal(size=(200, 3))
        cand = cand / np.linalg.norm(cand, axis=1, keepdims=True) * rng.uniform(0.03, 0.07, (200, 1))
        h, o = torch.from_numpy(hand[b:b + 1]), torch.from_numpy(cand[None])
        dist = ((o[:, :, None] - h[:, None]) ** 2).sum(-1).sqrt()[0]
        two, dt = dist.sort(dim=1)[0][:, :2], dist[:, targets].sort(dim=1)[0][:, :2]
        m = ref.masks_t(h, faces, o, targets)
        n = ref.vertex_normals_t(h, faces)[0]
        dot = ((h[0][m["j"][0]] - o[0]) * n[m["j"][0]]).sum(-1)
        ok = ((two[:, 1] - two[:, 0] > 1e-5) & (dt[:, 1] - dt[:, 0] > 1e-5) & (dot.abs() > 1e-5) & ((two[:, 0] - 0.02).abs() > 1e-5)).numpy()
        assert ok.sum() >= N
        objs.append(cand[ok][:N])
    return hand, faces, np.stack(objs), targets


def test_f64_gradient_equals_central_differences():
    """h = 1e-6 on every coordinate of both hands (the rows are independent: one evaluation moves both).  With the masks fixed the
    loss is quadratic in the hand, so the central difference has no truncation error; its rounding, 2^-52 |loss| / h, is below 1e-8.
    The masks are recomputed in every evaluation: away from the boundaries they are constants, which is what the gradient assumes."""
    hand, faces, obj, targets = _tie_free_case()
    o = torch.from_numpy(obj)
    x = torch.from_numpy(hand).clone().requires_grad_(True)
    loss = ref.ttt_loss_t(x, faces, o, targets)
    m0 = ref.masks_t(x.detach(), faces, o, targets)
    assert m0["inside"].any(1).all() and m0["contact"].any(1).all() and not m0["contact"].all() and not m0["inside"].all()
    grad, = torch.autograd.grad(loss.sum(), x)
    grad = grad.numpy()
    h, fd = 1e-6, np.zeros_like(hand)
    with torch.no_grad():
        for v in range(hand.shape[1]):
            for c in range(3):
                hi, lo = hand.copy(), hand.copy()
                hi[:, v, c] += h
                lo[:, v, c] -= h
                fd[:, v, c] = ((ref.ttt_loss_t(torch.from_numpy(hi), faces, o, targets) - ref.ttt_loss_t(torch.from_numpy(lo), faces, o, targets)) / (2 * h)).numpy()
    err, mag = np.abs(grad - fd).max(), np.abs(grad).max()
    print(f"ttt-grad-fd: {err:.2e} on {mag:.2e}")
    assert mag > 1.0 and err <= 1e-6 * max(1.0, mag), (err, mag)


def _rounding_bound(hand, obj, m, n_ct, w_pen, w_con):
    """Per component: 2 |w| (n + 2) 2^-24 sum |hand - obj| over the n contributing points, for each of the two terms.  (Every
    difference is rounded once, the running sum n - 1 times, the product a * Gp and the final fma once each, the division of the
    contact weight once.)"""
    B, V = hand.shape[:2]
    bound = np.zeros(hand.shape)
    for b in range(B):
        for flag, index, w in ((m["inside"][b], m["j"][b], w_pen), (m["contact"][b], m["jc"][b], w_con / max(int(n_ct[b]), 1))):
            S, n = np.zeros((V, 3)), np.zeros(V)
            for p in np.flatnonzero(flag):
                S[index[p]] += np.abs(hand[b, index[p]].astype(np.float64) - obj[b, p].astype(np.float64))
                n[index[p]] += 1
            bound[b] += 2 * abs(w) * (n[:, None] + 2) * U * S
    return bound


@pytest.mark.parametrize("case", ("real", "sphere"))
def test_f32_restatement_is_within_the_rounding_bound(case):
    if case == "real":
        g = golden()
        hand, faces, targets = np.stack([g["hand0"], g["hand1"]]).astype(f32), mano_faces(), prior()
        obj = np.stack([g["obj0"], g["obj1"]]).astype(f32)
    else:
        hand, faces = hands_of(776, 2, "bound")
        targets, obj = np.arange(0, 776, 3), cloud_near(hand, 300, "bound")
    B = hand.shape[0]
    r = ref.grasp_ttt(hand, faces, obj, targets, np.full(B, W_PEN, f32), np.full(B, W_CON, f32), mean_contact=True)
    x = torch.from_numpy(hand.astype(np.float64)).requires_grad_(True)
    loss = ref.ttt_loss_t(x, faces, torch.from_numpy(obj.astype(np.float64)), targets, W_PEN, W_CON, frozen={k: r[k] for k in ("j", "inside", "jc", "contact")})
    g64, = torch.autograd.grad(loss.sum(), x)
    err = np.abs(r["grad"].astype(np.float64) - g64.numpy())
    bound = _rounding_bound(hand, obj, r, r["n_contact"], W_PEN, W_CON)
    assert r["inside"].any() and r["contact"].any() and np.abs(g64.numpy()).max() > 1.0
    assert (err <= bound).all(), float((err - bound).max())
    assert (r["grad"][bound == 0] == 0).all()                        # a vertex no point names has a zero gradient
    # and the loss itself: the combination of the restatement's bits against the float64 value
    l32 = ref.combine(r["penetration"], r["contact_sum"], r["n_contact"], W_PEN, W_CON)
    assert np.abs(l32 - loss.detach().numpy()).max() <= 1e-5 * np.abs(loss.detach().numpy()).max()


def test_refine_ttt_update_is_torch_sgd(monkeypatch):
    """The two device ops replaced by recording CPU stubs (a smooth loss of the vertices, a linear map back to the 61 columns): the
    iterates of refine_ttt are those of torch.optim.SGD(lr, momentum) fed the same gradients, to the bit."""
    B, lr, mom, steps = 4, 0.05, 0.8, 6
    A = synth.synthetic_normal((61, 12), 95, "ttt/sgd/A", 0.3)
    Bt = synth.synthetic_normal((12, 61), 95, "ttt/sgd/B", 0.3)
    calls = []

    def layer(betas, global_orient, hand_pose, transl):
        p = torch.cat([betas, global_orient, hand_pose, transl], 1)
        return types.SimpleNamespace(vertices=(p @ A).reshape(-1, 4, 3))
    layer._packed = "packed"

    def value_and_grad(topology, hand_xyz, obj_xyz, targets=None, w_pen=W_PEN, w_con=W_CON, contact_threshold=0.02 ** 2, want_grad=True):
        calls.append(("ttt", topology, targets, w_pen, w_con, want_grad))
        return (hand_xyz ** 2).sum((1, 2)), (2 * hand_xyz if want_grad else None)

    def mano_backward(packed, betas, hand_pose, global_orient=None, transl=None, grad_verts=None, **_):
        calls.append(("bwd", packed))
        g = grad_verts.reshape(-1, 12) @ Bt                         # any fixed map will do: the update rule is what is under test
        return g[:, :10], g[:, 13:58], g[:, 10:13], g[:, 58:61]

    monkeypatch.setattr(contact, "ttt_value_and_grad", value_and_grad)
    monkeypatch.setattr(ops, "mano_backward", mano_backward)
    p0 = synth.synthetic_normal((B, 61), 95, "ttt/sgd/p", 1.0)
    out = contact.refine_ttt(layer, "topo", p0, None, steps, lr, mom, targets="T", w_pen=3.0, w_con=5.0, keep_best=False)
    assert [c[0] for c in calls] == ["ttt"] + ["bwd", "ttt"] * steps and calls[0][1:5] == ("topo", "T", 3.0, 5.0)
    assert [c[5] for c in calls if c[0] == "ttt"] == [True] * steps + [False] and calls[1][1] == "packed"
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([q], lr=lr, momentum=mom)
    losses = []
    for _ in range(steps):
        v = (q.detach() @ A).reshape(-1, 4, 3)
        losses.append((v ** 2).sum((1, 2)))
        q.grad = (2 * v).reshape(-1, 12) @ Bt
        opt.step()
    last = ((q.detach() @ A).reshape(-1, 4, 3) ** 2).sum((1, 2))
    assert torch.equal(out["params"], q.detach()) and torch.equal(out["loss0"], losses[0]) and torch.equal(out["loss"], last)
    assert out["iter"].tolist() == [steps] * B and out["iter"].dtype == torch.int32 and not torch.equal(q.detach(), p0)
    # keep_best: every row its best iterate, the earliest among equals; steps = 0: the input's bits
    best = contact.refine_ttt(layer, "topo", p0, None, steps, lr, mom, keep_best=True)
    every = torch.stack(losses + [last])
    assert best["iter"].tolist() == every.argmin(0).tolist() and torch.equal(best["loss"], every.min(0)[0])
    for k in set(best["iter"].tolist()):
        rows = best["iter"] == k
        assert torch.equal(best["params"][rows], contact.refine_ttt(layer, "topo", p0, None, k, lr, mom, keep_best=False)["params"][rows])
    zero = contact.refine_ttt(layer, "topo", p0, None, 0)
    assert torch.equal(zero["params"], p0) and zero["iter"].tolist() == [0] * B and torch.equal(zero["loss"], zero["loss0"])
    bad = p0.clone()
    bad[1, 7] = float("nan")
    got = contact.refine_ttt(layer, "topo", bad, None, 3, lr, mom)
    assert got["iter"][1] == 0 and torch.equal(got["params"][[0, 2, 3]], contact.refine_ttt(layer, "topo", p0, None, 3, lr, mom)["params"][[0, 2, 3]])
    assert np.array_equal(got["params"][1].numpy().view(np.uint32), bad[1].numpy().view(np.uint32))
    for kw in (dict(steps=-1), dict(steps=1001), dict(lr=float("inf")), dict(lr=-1.0), dict(momentum=1.0), dict(momentum=-0.1)):
        with pytest.raises(RuntimeError):
            contact.refine_ttt(layer, "topo", p0, None, **{"steps": 1, **kw})
    with pytest.raises(RuntimeError):
        contact.refine_ttt(layer, "topo", p0[:, :60], None, 1)


@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_ttt_flags(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.ttt_steps, a.ttt_lr, a.ttt_momentum, a.ttt_w_pen, a.ttt_w_con, a.ttt_prior, a.ttt_keep_best) == (0, 6.25e-6, 0.8, 840.0, 7500.0, None, 1)
    a = generate.parse_args(dataset, ["--ttt_steps", "300", "--ttt_lr", "1e-5", "--ttt_momentum", "0", "--ttt_w_pen", "1", "--ttt_w_con", "0",
                                      "--ttt_prior", "list.json", "--ttt_keep_best", "0"])
    assert (a.ttt_steps, a.ttt_lr, a.ttt_momentum, a.ttt_w_pen, a.ttt_w_con, a.ttt_prior, a.ttt_keep_best) == (300, 1e-5, 0.0, 1.0, 0.0, "list.json", 0)
    assert generate.parse_args(dataset, ["--ttt_steps", "1000"]).ttt_steps == 1000
    for bad in (["--ttt_steps", "-1"], ["--ttt_steps", "1001"], ["--ttt_steps", "x"], ["--ttt_lr", "-1"], ["--ttt_lr", "inf"], ["--ttt_lr", "nan"],
                ["--ttt_momentum", "1"], ["--ttt_momentum", "-0.1"], ["--ttt_momentum", "nan"], ["--ttt_w_pen", "-1"], ["--ttt_w_pen", "inf"],
                ["--ttt_w_con", "nan"], ["--ttt_keep_best", "2"], ["--ttt_prior", "list.json"]):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_generate_for_objects_refuses_bad_ttt_arguments():
    net = types.SimpleNamespace()
    for kw in (dict(ttt_steps=-1), dict(ttt_steps=1001), dict(ttt_steps=3, ttt_lr=-1.0), dict(ttt_steps=3, ttt_lr=float("nan")),
               dict(ttt_steps=3, ttt_momentum=1.0), dict(ttt_steps=3, ttt_w_pen=-1.0), dict(ttt_steps=3, ttt_w_con=float("inf")),
               dict(ttt_prior="list.json")):
        with pytest.raises(RuntimeError, match="ttt_"):
            generate.generate_for_objects(net, [], 1, False, 0, [], **kw)


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_grasp_ttt" in _lib.SIGNATURES and "int dvq_grasp_ttt(" in header and hasattr(lib, "dvq_grasp_ttt")
    assert "dvq_grasp_ttt" in re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert len(_lib.SIGNATURES["dvq_grasp_ttt"][1]) == 22 and lib.dvq_abi_version() == 10
    assert re.search(r"^#define DVQ_GRASP_TTT_MAX_N 16384$", header, re.M) and ops.GRASP_TTT_MAX_N == 16384
    assert contact.TTT_MAX_STEPS == generate.TTT_MAX_STEPS == 1000
    assert (contact.TTT_W_PEN, contact.TTT_W_CON, contact.TTT_LR, contact.TTT_MOMENTUM) == (7 * 120.0, 1 * 2.5 * 3000.0, 6.25e-6, 0.8)


def test_contact_targets_and_argument_checks_need_no_device(tmp_path):
    t = contact.ContactTargets([4, 1, 1, 3], n_verts=6)
    assert t.indices.tolist() == [1, 3, 4] and t.flags.tolist() == [0, 1, 0, 1, 1, 0] and t.flags.dtype == np.int32 and t.n_verts == 6
    assert contact.ContactTargets(np.asarray([False, True, False, True, True, False]), n_verts=6).flags.tolist() == t.flags.tolist()
    assert contact.ContactTargets(torch.tensor([1, 3, 4]), n_verts=6).flags.tolist() == t.flags.tolist()
    assert t.on("cpu") is t.on("cpu") and t.on("cpu").dtype == torch.int32 and t.on("cpu").tolist() == t.flags.tolist()
    path = str(tmp_path / "prior.json")
    json.dump(prior().tolist(), open(path, "w"))
    assert contact.ContactTargets.from_json(path).indices.tolist() == prior().tolist() and contact.ContactTargets.from_json(path).n_verts == 778
    for bad in ([], np.zeros(6, bool), [6], [-1], [[1, 2]], [0.5], np.ones(5, bool)):
        with pytest.raises(RuntimeError):
            contact.ContactTargets(bad, n_verts=6)
    for text in ('{"a": 1}', "[1.5]", "[true]", "[]"):
        open(path, "w").write(text)
        with pytest.raises(RuntimeError):
            contact.ContactTargets.from_json(path)
    V = 6
    faces, vf_off, vf_face = (torch.from_numpy(x) for x in contact.face_csr([[0, 1, 2], [3, 4, 5]], V))
    hand, obj = torch.zeros(2, V, 3), torch.zeros(2, 9, 3)
    good = dict(hand=hand, faces=faces, vf_off=vf_off, vf_face=vf_face, obj=obj, targets=t.on("cpu"), w_pen=torch.ones(2), w_con=torch.ones(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_ttt(**good)
    for bad in (dict(obj=torch.zeros(2, ops.GRASP_TTT_MAX_N + 1, 3)), dict(obj=torch.zeros(2, 0, 3)), dict(obj=torch.zeros(3, 9, 3)),
                dict(targets=t.on("cpu").long()), dict(targets=t.on("cpu")[:5]), dict(targets=torch.zeros(12, dtype=torch.int32)[::2]),
                dict(targets=t.flags), dict(w_pen=torch.ones(3)), dict(w_con=torch.ones(2).double()), dict(w_pen=1.0),
                dict(hand=hand.double()), dict(hand=torch.zeros(2, 3, V).transpose(1, 2)), dict(vf_off=vf_off[:-1])):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_ttt(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    topo = contact.HandTopology(faces.numpy(), V, "cpu")
    with pytest.raises(RuntimeError, match="ContactTargets"):
        contact.ttt_terms(topo, hand, obj, targets=[1, 2])
    with pytest.raises(RuntimeError, match="778"):
        contact.ttt_loss(topo, hand, obj, targets=contact.ContactTargets([1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        contact.ttt_value_and_grad(topo, hand, obj, targets=t)


# ========================================================================================== GPU group: the kernel
def dev(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


OUT = ("penetration", "contact_sum", "n_interior", "n_contact", "grad")


def run_dev(hand, faces, obj, targets=None, w_pen=None, w_con=None, mean_contact=False, want_grad=True, channel_first=False):
    B, V = hand.shape[:2]
    topo = contact.HandTopology(faces, V, DEV)
    o = dev(np.ascontiguousarray(np.transpose(obj, (0, 2, 1)))).transpose(1, 2) if channel_first else dev(obj)
    assert o.is_contiguous() != channel_first or obj.shape[1] == 1
    flags = None if targets is None else contact.ContactTargets(targets, n_verts=V).on(DEV)
    w = lambda x: None if x is None else dev(np.asarray(x, f32))
    out = ops.grasp_ttt(dev(hand), topo.faces, topo.vf_off, topo.vf_face, o, flags, w(w_pen), w(w_con), mean_contact, want_grad)
    assert [None if x is None else tuple(x.shape) for x in out] == [(B,)] * 4 + [(B, V, 3) if want_grad else None]
    assert [x.dtype for x in out[:4]] == [torch.float32, torch.float32, torch.int32, torch.int32]
    return {k: None if x is None else x.cpu().numpy() for k, x in zip(OUT, out)}


def check_against_restatement(hand, faces, obj, targets, w_pen, w_con, mean_contact, what, channel_first=False):
    got = run_dev(hand, faces, obj, targets, w_pen, w_con, mean_contact, True, channel_first)
    want = ref.grasp_ttt(hand, faces, obj, targets, w_pen, w_con, mean_contact)
    for k in OUT:
        same_bits(got[k], want[k], f"{what}: {k}")
    topo = contact.HandTopology(faces, hand.shape[1], DEV)
    o = dev(obj)
    pen, n_in, n_ct = ops.grasp_scores(dev(hand), topo.faces, topo.vf_off, topo.vf_face, o)
    same_bits(got["penetration"], pen.cpu().numpy(), f"{what}: penetration against grasp_scores")
    assert np.array_equal(got["n_interior"], n_in.cpu().numpy()) and np.array_equal(got["n_contact"], n_ct.cpu().numpy())
    fwd = run_dev(hand, faces, obj, targets, want_grad=False, channel_first=channel_first)        # the forward-only launch: the same four
    for k in OUT[:4]:
        same_bits(fwd[k], got[k], f"{what}: forward-only {k}")
    again = run_dev(hand, faces, obj, targets, w_pen, w_con, mean_contact, True, channel_first)
    for k in OUT:
        same_bits(again[k], got[k], f"{what}: second run {k}")
    return got, want


def weights(B, tag):
    return (synth.synthetic_uniform((B,), 96, f"ttt/{tag}/wp", 0.5, 900.0).numpy(), synth.synthetic_uniform((B,), 96, f"ttt/{tag}/wc", 0.5, 8000.0).numpy())


@gpu
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_small_mesh_equals_the_restatement_bit_for_bit(N):
    """V = 5: the tail loop behind the sixteen-byte reads.  N around 256: a thread with no point, with one, the first with two."""
    hand, faces = hands_of(5, 3, f"small{N}")
    obj = cloud_near(hand, N, f"small{N}", sigma=0.012)
    wp, wc = weights(3, f"small{N}")
    for targets in (None, [2], [0, 3, 4]):
        for mean in (False, True):
            got, want = check_against_restatement(hand, faces, obj, targets, wp, wc, mean, f"V=5 N={N} targets={targets} mean={mean}")
        if targets is not None:
            assert np.isin(want["jc"], targets).all()
            assert (got["grad"][:, [v for v in range(5) if v not in targets]] == want["grad"][:, [v for v in range(5) if v not in targets]]).all()
    if N > 1:
        assert want["inside"].any() and want["contact"].any() and np.abs(want["grad"]).max() > 0


@gpu
@pytest.mark.parametrize("V,N,B,targets,channel_first", [(776, 1024, 3, "third", True), (778, 3000, 3, "prior", False),
                                                         (778, 1024, 1, None, True), (2048, 1024, 1, "third", False),
                                                         (2048, 257, 3, None, False)])
def test_model_shapes_equal_the_restatement_bit_for_bit(V, N, B, targets, channel_first):
    """The sphere of tests/test_contact.py, posed hands of the real model with the reference's contact vertices, and a finer sphere
    of 2048 vertices: the second walk of the gather phase, the largest planes."""
    hand, faces = hands_of(V, B, f"model{N}")
    obj = cloud_near(hand, N, f"model{V}")
    T = {"third": np.arange(1, V, 3), "prior": prior(), None: None}[targets]
    wp, wc = weights(B, f"model{V}")
    got, want = check_against_restatement(hand, faces, obj, T, wp, wc, True, f"V={V} N={N} B={B}", channel_first)
    named = np.unique(want["j"][want["inside"]]).size + np.unique(want["jc"][want["contact"]]).size
    print(f"V={V} N={N}: n_interior {want['n_interior'].tolist()} n_contact {want['n_contact'].tolist()} vertices named {named}")
    assert (want["n_interior"] > 0).all() and (want["n_contact"] > want["n_interior"]).all() and np.isfinite(want["grad"]).all()
    if V == 2048:
        assert (want["j"][want["inside"]] >= 1024).any() and (want["jc"][want["contact"]] >= 1024).any(), "no vertex of the second walk is named"


@gpu
def test_rows_of_a_batch_of_65_equal_the_rows_alone():
    hand, faces = hands_of(778, 65, "batch")
    obj = cloud_near(hand, 257, "batch")
    wp, wc = weights(65, "batch")
    got, _ = check_against_restatement(hand, faces, obj, prior(), wp, wc, True, "B=65")
    assert len({x.tobytes() for x in got["grad"]}) == 65
    for b in (0, 1, 31, 64):
        one = run_dev(hand[b:b + 1], faces, obj[b:b + 1], prior(), wp[b:b + 1], wc[b:b + 1], True)
        for k in OUT:
            same_bits(one[k], got[k][b:b + 1], f"row {b} alone: {k}")
    empty = run_dev(hand[:0], faces, obj[:0], prior(), wp[:0], wc[:0], True)
    assert all(x.shape[0] == 0 for x in empty.values())


@gpu
def test_ties_take_the_lowest_index():
    """Two coincident vertices (the lowest index wins both scans, also when only the higher one has faces), and a point at the same
    distance from two vertices."""
    v, faces = bipyramid()
    hand = np.concatenate([v, v[[3]], v[[0]]])[None].astype(f32)                 # vertex 5 = vertex 3, vertex 6 = vertex 0
    obj = np.asarray([[[0.0, 0.0, 0.045], [0.0, 0.0, 0.035], [0.031, 0.001, 0.0], [-0.015, 0.0, 0.0], [0.0, 0.0, -0.039]]], f32)
    assert np.array_equal(obj[0, 3] - hand[0, 1], (obj[0, 3] - hand[0, 2]) * np.asarray([1, -1, 1], f32))     # equidistant from 1 and 2
    for f, what in ((faces, "faces at the lower duplicate"), (np.where(faces == 3, 5, faces), "faces at the higher duplicate")):
        got, want = check_against_restatement(hand, f, obj, None, None, None, False, what)
        assert want["j"][0].tolist() == [3, 3, 0, 1, 4] and want["jc"][0].tolist() == [3, 3, 0, 1, 4]
        got, want = check_against_restatement(hand, f, obj, [2, 4, 5, 6], None, None, True, what + ", targets")
        assert want["j"][0].tolist() == [3, 3, 0, 1, 4] and want["jc"][0].tolist() == [5, 5, 6, 2, 4]
    # coordinates whose squares overflow: every distance is +inf, the lowest target attains it, nothing is in contact
    far = (hand * f32(1e30)).astype(f32)
    with np.errstate(all="ignore"):
        got, want = check_against_restatement(far, faces, obj, [2, 4], None, None, False, "overflow")
    assert np.isposinf(want["penetration"]).all() or want["n_interior"][0] == 0
    assert got["n_contact"].tolist() == [0] and bits(got["contact_sum"]).tolist() == [0]


@gpu
def test_non_finite_rows_stay_in_their_rows():
    hand, faces = hands_of(778, 5, "nan")
    obj = cloud_near(hand, 300, "nan")
    wp, wc = weights(5, "nan")
    clean = run_dev(hand, faces, obj, prior(), wp, wc, True)
    bad_h, bad_o = hand.copy(), obj.copy()
    bad_h[1, 777, 2] = np.nan
    bad_o[3, 299, 0] = np.inf
    got, want = check_against_restatement(bad_h, faces, bad_o, prior(), wp, wc, True, "non-finite rows")
    for b in (1, 3):
        assert np.isnan(got["contact_sum"][b]) and np.isnan(got["grad"][b]).all()
    assert np.isnan(got["penetration"][1]) and not np.isnan(got["penetration"][3])
    for k in OUT:
        same_bits(got[k][[0, 2, 4]], clean[k][[0, 2, 4]], f"the rows beside them: {k}")
    t = contact.ttt_loss(contact.HandTopology(faces, 778, DEV), dev(bad_h), dev(bad_o), contact.ContactTargets(prior()))
    assert torch.isnan(t[[1, 3]]).all() and torch.isfinite(t[[0, 2, 4]]).all()


@gpu
def test_refused_arguments_launch_nothing():
    """Refusals of arguments through the C ABI: an error return with valid device pointers behind it, never a launch."""
    lib = _lib.load()
    one = torch.full((65536,), 7.0, device=DEV)
    p = one.data_ptr()
    call = lambda V, N, B, mean=0, out=p, targets=p: lib.dvq_grasp_ttt(p, p, p, p, V, p, 3 * N, 3, 1, B, N, 4e-4, targets, None, None, mean, out, p, p, p,
                                                                         None, None)
    assert call(5, ops.GRASP_TTT_MAX_N + 1, 1) == 1 and b"grasp_ttt" in lib.dvq_last_error()
    assert call(2049, 16, 1) == 1 and call(0, 16, 1) == 1 and call(5, 0, 1) == 1 and call(5, 16, -1) == 1 and call(5, 16, 1, mean=2) == 1
    assert call(5, 16, 1, out=None) == 1 and b"null" in lib.dvq_last_error()
    assert call(5, 16, 0, out=None) == 0                                       # B = 0: nothing to do, no pointer is looked at
    torch.cuda.synchronize()
    assert bool((one == 7.0).all())
    hand, faces = hands_of(5, 1, "refuse")
    topo = contact.HandTopology(faces, 5, DEV)
    with pytest.raises(RuntimeError):
        ops.grasp_ttt(dev(hand), topo.faces, topo.vf_off, topo.vf_face, torch.zeros(1, ops.GRASP_TTT_MAX_N + 1, 3, device=DEV))
    with pytest.raises(RuntimeError, match="devices|HIP device"):
        ops.grasp_ttt(dev(hand), topo.faces, topo.vf_off, topo.vf_face, torch.zeros(1, 4, 3, device=DEV), w_pen=torch.ones(1))


@gpu
def test_the_largest_cloud_fits():
    """N = DVQ_GRASP_TTT_MAX_N at V = 2048: the largest LDS image the entry point accepts (bits against the restatement at the
    cheaper V = 5, the same word array)."""
    N = ops.GRASP_TTT_MAX_N
    hand, faces = hands_of(5, 1, "maxn")
    obj = cloud_near(hand, N, "maxn", sigma=0.012)
    check_against_restatement(hand, faces, obj, [1, 3], None, None, True, "N=16384 V=5")
    big, bf = hands_of(2048, 1, "maxn")
    o = cloud_near(big, N, "maxn2048")
    got = run_dev(big, bf, o, None, None, None, True)
    topo = contact.HandTopology(bf, 2048, DEV)
    pen, n_in, n_ct = ops.grasp_scores(dev(big), topo.faces, topo.vf_off, topo.vf_face, dev(o))
    same_bits(got["penetration"], pen.cpu().numpy())
    assert np.array_equal(got["n_contact"], n_ct.cpu().numpy()) and np.isfinite(got["grad"]).all() and np.abs(got["grad"]).max() > 0


# ========================================================================================== GPU group: autograd, the layer, the loop
@gpu
def test_autograd_equals_the_fused_launch(monkeypatch):
    hand, faces = hands_of(778, 3, "autograd")
    obj = dev(cloud_near(hand, 512, "autograd"))
    topo, T = contact.HandTopology(faces, 778, DEV), contact.ContactTargets(prior())
    x = dev(hand).requires_grad_(True)
    loss = contact.ttt_loss(topo, x, obj, T)
    assert loss.grad_fn is not None and tuple(loss.shape) == (3,)
    loss.sum().backward()
    value, grad = contact.ttt_value_and_grad(topo, x, obj, T)
    assert torch.equal(loss.detach(), value) and torch.equal(x.grad, grad) and value.grad_fn is None and float(grad.abs().max()) > 0
    want = ref.grasp_ttt(hand, faces, obj.cpu().numpy(), prior(), np.full(3, W_PEN, f32), np.full(3, W_CON, f32), True)
    same_bits(grad.cpu().numpy(), want["grad"], "value_and_grad against the restatement")
    same_bits(value.cpu().numpy(), ref.combine(want["penetration"], want["contact_sum"], want["n_contact"], W_PEN, W_CON), "loss")
    # an unused output contributes nothing: each term alone is the launch with the other weight 0
    one, zero = torch.ones(3, device=DEV), torch.zeros(3, device=DEV)
    for key, wp, wc in (("penetration", one, zero), ("contact_sum", zero, one)):
        y = dev(hand).requires_grad_(True)
        t = contact.ttt_terms(topo, y, obj, T)
        assert t["penetration"].grad_fn is not None and t["contact_sum"].grad_fn is not None and not t["n_contact"].requires_grad
        t[key].sum().backward()
        alone = ops.grasp_ttt(dev(hand), topo.faces, topo.vf_off, topo.vf_face, obj, T.on(DEV), wp, wc, want_grad=True)[4]
        assert torch.equal(y.grad, alone) and float(alone.abs().max()) > 0
    # under no_grad, and for a hand that does not require grad: the forward launch alone
    launches = []
    real = ops.grasp_ttt
    monkeypatch.setattr(ops, "grasp_ttt", lambda *a, **k: (launches.append(k.get("want_grad", a[9] if len(a) > 9 else False)), real(*a, **k))[1])
    with torch.no_grad():
        t = contact.ttt_terms(topo, x, obj, T)
    u = contact.ttt_terms(topo, dev(hand), obj, T)
    assert launches == [False, False] and sorted(t) == ["contact_sum", "n_contact", "n_interior", "penetration"]
    assert all(v.grad_fn is None and not v.requires_grad for v in list(t.values()) + list(u.values()))
    assert torch.equal(t["contact_sum"], u["contact_sum"]) and torch.equal(t["penetration"], contact.grasp_scores(topo, dev(hand), obj)["penetration"])
    y = dev(hand).requires_grad_(True)
    g, = torch.autograd.grad(contact.ttt_loss(topo, y, obj, T).sum(), y, create_graph=True)
    assert launches[-2:] == [False, True]
    with pytest.raises(RuntimeError):                                          # once differentiable
        g.sum().backward()


_layers = {}


def layer_on_device():
    if "real" not in _layers:
        _layers["real"] = dmano.ManoLayer(mano_arrays(), flat_hand_mean=True).to(DEV)
    return _layers["real"]


def pose(layer, p):
    return layer(betas=p[:, :10], global_orient=p[:, 10:13], hand_pose=p[:, 13:58], transl=p[:, 58:61]).vertices


@gpu
def test_gradient_through_the_layer_against_float64():
    """Eight real-model rows, N = 512: d sum(ttt_loss(layer(p))) / d p on the device against the float64 restatement composed with
    tests/mano_grad_ref.ManoTorch, masks and indices frozen to the device's (the fp32 restatement on the device's vertices).
    Worst ttt-grad-ratio observed on an MI355X: 0.87 (betas)."""
    B, N = 8, 512
    p0 = params61(B, "layer")
    obj = cloud_near(posed(p0), N, "layer")
    layer, faces = layer_on_device(), mano_faces()
    topo, T = contact.HandTopology(faces, 778, DEV), contact.ContactTargets(prior())
    p = p0.to(DEV).requires_grad_(True)
    verts = pose(layer, p)
    contact.ttt_loss(topo, verts, dev(obj), T).sum().backward()
    got = p.grad.cpu().double().numpy()
    m = ref.grasp_ttt(verts.detach().cpu().numpy(), faces, obj, prior(), want_grad=False)
    frozen = {k: m[k] for k in ("j", "inside", "jc", "contact")}
    assert (m["n_interior"] > 0).all() and (m["n_contact"] > 0).all()
    grads = {}
    for dtype in (torch.float64, torch.float32):
        mt = gref.ManoTorch(mano_ref.device_arrays(mano_arrays()), flat_hand_mean=True, dtype=dtype)
        q = p0.to(dtype).requires_grad_(True)
        v = mt(q[:, :10], q[:, 13:58], q[:, 10:13], q[:, 58:61])[0]
        ref.ttt_loss_t(v, faces, torch.from_numpy(obj).to(dtype), prior(), W_PEN, W_CON, frozen=frozen).sum().backward()
        grads[dtype] = q.grad.double().numpy()
    line, worst = [], 0.0
    for name, cols in GROUPS:
        e32 = np.abs(grads[torch.float32][:, cols] - grads[torch.float64][:, cols]).max()
        err = np.abs(got[:, cols] - grads[torch.float64][:, cols]).max()
        line.append(f"{name} {err:.3e} / e32 {e32:.3e} = {err / e32:.2f} (|grad| {np.abs(grads[torch.float64][:, cols]).max():.2g})")
        worst = max(worst, err / e32)
        assert e32 > 0 and np.isfinite(err) and err <= FACTOR * e32, f"grad {name} differs from the float64 gradient by {err:.3e} > {FACTOR:g} x e32 = {FACTOR * e32:.3e}"
    print("ttt-grad-ratio B=8 N=512: " + "; ".join(line) + f"; worst {worst:.2f}")


def refine_case(B=6, N=512, tag="refine"):
    p0 = params61(B, tag)
    obj = dev(cloud_near(posed(p0), N, tag))
    layer = layer_on_device()
    return layer, contact.HandTopology(mano_faces(), 778, DEV), contact.ContactTargets(prior()), p0.to(DEV), obj


@gpu
def test_refine_ttt_equals_a_hand_written_sgd_loop():
    layer, topo, T, p0, obj = refine_case()
    zero = contact.refine_ttt(layer, topo, p0, obj, 0, targets=T)
    assert torch.equal(zero["params"], p0) and zero["iter"].tolist() == [0] * 6 and torch.equal(zero["loss"], zero["loss0"])
    assert torch.equal(zero["loss0"], contact.ttt_loss(topo, pose(layer, p0), obj, T))
    steps = 5
    out = contact.refine_ttt(layer, topo, p0, obj, steps, targets=T, keep_best=False)
    q = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([q], lr=contact.TTT_LR, momentum=contact.TTT_MOMENTUM)
    first = None
    for _ in range(steps):
        opt.zero_grad()
        loss = contact.ttt_loss(topo, pose(layer, q), obj, T)
        first = loss.detach() if first is None else first
        loss.sum().backward()
        opt.step()
    assert torch.equal(out["params"], q.detach()), float((out["params"] - q.detach()).abs().max())
    assert torch.equal(out["loss0"], first) and out["iter"].tolist() == [steps] * 6 and not torch.equal(out["params"], p0)
    with torch.no_grad():
        assert torch.equal(out["loss"], contact.ttt_loss(topo, pose(layer, q), obj, T))
    print("refine_ttt 5 steps: loss", out["loss0"].tolist(), "->", out["loss"].tolist())


@gpu
def test_refine_ttt_keeps_the_best_iterate():
    layer, topo, T, p0, obj = refine_case(tag="best")
    steps = 6
    p = p0.clone()
    p[4, 20] = float("nan")
    out = contact.refine_ttt(layer, topo, p, obj, steps, lr=4 * contact.TTT_LR, targets=T)        # four times the default rate
    ok = [0, 1, 2, 3, 5]
    assert bool((out["loss"][ok] <= out["loss0"][ok]).all()) and out["iter"].dtype == torch.int32
    assert out["iter"][4] == 0 and np.array_equal(out["params"][4].cpu().numpy().view(np.uint32), p[4].cpu().numpy().view(np.uint32))
    assert torch.isnan(out["loss"][4]) and torch.isnan(out["loss0"][4])
    iters = out["iter"].tolist()
    print("refine_ttt keep_best: iter", iters, "loss0", out["loss0"].tolist(), "loss", out["loss"].tolist())
    assert max(iters) > 0
    for k in sorted(set(iters[i] for i in ok)):
        at = contact.refine_ttt(layer, topo, p, obj, k, lr=4 * contact.TTT_LR, targets=T, keep_best=False)
        rows = [i for i in ok if iters[i] == k]
        assert torch.equal(at["params"][rows], out["params"][rows]) and torch.equal(at["loss"][rows], out["loss"][rows]), k
        later = [i for i in ok if iters[i] > k]
        assert bool((at["loss"][later] > out["loss"][later]).all()), "an earlier iterate with the same or a lower loss was passed over"


# ========================================================================================== GPU group: the entry point
def _run_main(out_dir, extra, mano):
    paths = generate.main("obman", extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@gpu
def test_entry_point_writes_the_same_files_for_every_grouping(tmp_path):
    """Synthetic weights on the real hand topology, four clouds: with --ttt_steps 3 the files do not depend on --rows_per_call and
    hold the parameters of contact.refine_ttt; with --ttt_steps 0 they are the files written without the flag."""
    from test_grasp_self import _cloud_files, _mano_pkl
    mano = _mano_pkl(tmp_path)
    files = _cloud_files(tmp_path)
    prior_json = str(tmp_path / "prior.json")
    json.dump(prior().tolist(), open(prior_json, "w"))
    base = ["--objects"] + files + ["--num_grasp", "4"]
    ttt = base + ["--ttt_steps", "3", "--ttt_prior", prior_json]
    names, data = _run_main(str(tmp_path / "t16384"), ttt + ["--rows_per_call", "16384"], mano)
    for rows in ("0", "7"):
        n2, d2 = _run_main(str(tmp_path / f"t{rows}"), ttt + ["--rows_per_call", rows], mano)
        assert n2 == names and d2 == data, f"--rows_per_call {rows}: the files differ"
    n0, d0 = _run_main(str(tmp_path / "plain"), base + ["--rows_per_call", "16384"], mano)
    n1, d1 = _run_main(str(tmp_path / "zero"), base + ["--rows_per_call", "16384", "--ttt_steps", "0"], mano)
    assert n1 == n0 == names and d1 == d0 and d0 != data and len(names) == len(files)
    layer = dmano.load(model_path=mano, model_type="mano", use_pca=True, num_pca_comps=45, flat_hand_mean=True).to(DEV)
    topo, T = contact.HandTopology(np.asarray(layer.faces), 778, DEV), contact.ContactTargets(prior())
    moved = 0
    for path, plain, tuned in zip(files, d0, data):
        assert b"NaN" not in tuned and b"Infinity" not in tuned
        j0, j1 = json.loads(plain), json.loads(tuned)
        assert set(j1) == set(j0) | {"ttt_loss0", "ttt_loss", "ttt_iter"} and "ttt_loss" not in j0
        p0 = torch.tensor(j0["recon_params"], dtype=torch.float32, device=DEV).reshape(4, 61)
        cloud = generate.object_tensor(np.load(path).astype(np.float64)).to(DEV)[:3].T.unsqueeze(0).expand(4, -1, -1)
        want = contact.refine_ttt(layer, topo, p0, cloud, 3, targets=T)
        assert np.array_equal(np.asarray(j1["recon_params"], f32).reshape(4, 61), want["params"].cpu().numpy())
        assert j1["ttt_iter"] == want["iter"].tolist() and np.array_equal(np.asarray(j1["ttt_loss"], f32), want["loss"].cpu().numpy())
        assert np.array_equal(np.asarray(j1["ttt_loss0"], f32), want["loss0"].cpu().numpy())
        assert all(a <= b for a, b in zip(j1["ttt_loss"], j1["ttt_loss0"]))
        moved += sum(j1["ttt_iter"])
    assert moved > 0, "no grasp was refined: the test cannot see the loop"
    # best-of-M ranks the refined candidates: the kept rows carry the figures of their own candidates
    sel = base + ["--candidates", "8", "--ttt_steps", "3", "--ttt_prior", prior_json]
    ns, ds = _run_main(str(tmp_path / "c16384"), sel + ["--rows_per_call", "16384"], mano)
    n7, d7 = _run_main(str(tmp_path / "c7"), sel + ["--rows_per_call", "7"], mano)
    assert n7 == ns and d7 == ds
    for plain_path, text in zip(files, ds):
        j = json.loads(text)
        assert len(j["ttt_loss"]) == 4 == len(j["candidate"]) and {"ttt_loss0", "ttt_iter", "penetration"} <= set(j)
