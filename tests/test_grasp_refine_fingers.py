"""Articulated push-out of generated grasps: the fused kernel (dvq_grasp_refine_fingers), its host API (ops.grasp_refine_fingers,
contact.FingerRig, contact.refine_fingers, contact.apply_fingers, contact.compose_finger_pose) and the ``refine_curl`` mode of
generate_for_objects / the entry points.  The reference is tests/grasp_refine_fingers_ref.py (numpy over oracle/contact_oracle.py and
grasp_score_ref.tree_sum, all fp32, one operation at a time); all ten GPU outputs are compared with it bit for bit.  Nothing here says
anything about real grasps: no real checkpoint exists in the tree."""
import json
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops, synth

import grasp_refine_fingers_ref as fref
import grasp_refine_ref as tref
import grasp_refine_rigid_ref as rref
import grasp_score_ref as ref
import mano_ref
import test_grasp_refine_rigid as rigid_tests                    # its inputs and helpers (a module, so nothing is collected twice)

DEV = "cuda:0"
THR = 0.02 ** 2
IDENTITY = np.asarray([1, 0, 0, 0], np.float32)
bits, gpu, mano_pkl = rigid_tests.bits, rigid_tests.gpu, rigid_tests.mano_pkl
NAMES = fref.NAMES


def hooked():
    """The prototype's hooked finger: a bar (an ellipsoid along x, the pivot at its -x end) whose last third is a finger hinged at
    x = 3 cm (the weights ramp from 0 to 1 over 2 cm).  The finger's tip is sunk in a small sphere; the bar's far side rests on a
    second, larger sphere just before the hinge, so a shift or a turn about the wrist that frees the tip loses that contact."""
    v, f = ref.sphere_mesh()
    hand = (v * np.asarray([1.6, 0.5, 0.5], np.float32)).astype(np.float32)
    w = np.clip((hand[:, 0].astype(np.float64) - 0.03) / 0.02, 0.0, 1.0).astype(np.float32)
    cloud = np.concatenate([tref.sphere_cloud(300, 0.01, (0.075, 0.01, 0.0)), tref.sphere_cloud(300, 0.03, (0.015, -0.0545, 0.0))])
    return dict(hand=hand[None], faces=f, obj=cloud[None], pivot=np.asarray([[-0.08, 0, 0]], np.float32), part=np.where(w > 0, 0, -1),
                w=w, knuckle=np.asarray([[[0.03, 0, 0]]], np.float32))


def run_ref(case, steps, traces=None, **kw):
    return fref.grasp_refine_fingers(case["hand"], case["faces"], case["obj"], case["pivot"], case["part"], case["w"], case["knuckle"], steps,
                                     traces=traces, **{**case.get("kw", {}), **kw})


def real_layer(tmp_path):
    from dvqvae_amd import mano as dmano
    return dmano.load(model_path=mano_pkl(tmp_path), model_type="mano", use_pca=True, num_pca_comps=45, flat_hand_mean=True)


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_curl_flags_and_the_abi_has_the_entry_point(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.refine_curl, a.refine_max_curl) == (0.0, 0.35)
    a = generate.parse_args(dataset, ["--refine_steps", "6", "--refine_curl", "0.5", "--refine_max_curl", "0.2"])
    assert (a.refine_steps, a.refine_curl, a.refine_max_curl, a.refine_spin) == (6, 0.5, 0.2, 0.0)
    a = generate.parse_args(dataset, ["--refine_steps", "6", "--refine_curl", "1", "--refine_spin", "1"])
    assert (a.refine_curl, a.refine_spin) == (1.0, 1.0)
    for bad in (["--refine_steps", "3", "--refine_curl", "-0.1"], ["--refine_steps", "3", "--refine_curl", "inf"],
                ["--refine_steps", "3", "--refine_curl", "nan"], ["--refine_curl", "1"],
                ["--refine_steps", "3", "--refine_curl", "1", "--refine_max_curl", "0"],
                ["--refine_steps", "3", "--refine_curl", "1", "--refine_max_curl", "3.2"],
                ["--refine_steps", "3", "--refine_curl", "1", "--refine_max_curl", "nan"]):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_grasp_refine_fingers" in _lib.SIGNATURES and len(_lib.SIGNATURES["dvq_grasp_refine_fingers"][1]) == 35
    assert "int dvq_grasp_refine_fingers(" in header and hasattr(lib, "dvq_grasp_refine_fingers")
    added = re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert "dvq_grasp_refine_fingers" in added


def test_bad_arguments_are_refused_before_any_device_use():
    v, f = ref.sphere_mesh(4, 6)
    V = len(v)
    faces, off, vf = (torch.from_numpy(a) for a in contact.face_csr(f, V))
    hand = torch.from_numpy(v)[None].contiguous()
    part, w = torch.zeros(V, dtype=torch.int32), torch.ones(V)
    good = dict(hand=hand, faces=faces, vf_off=off, vf_face=vf, vert_part=part, vert_w=w, n_fingers=2, obj=torch.zeros(1, 5, 3),
                pivot=torch.zeros(1, 3), knuckle=torch.zeros(1, 2, 3), steps=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_refine_fingers(**good)                                             # well-formed, but not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_refine_fingers(**{**good, "steps": 0, "curl": 0.0, "max_curl": np.pi})
    for bad in (dict(n_fingers=0), dict(n_fingers=6, knuckle=torch.zeros(1, 6, 3)), dict(vert_part=part + 2), dict(vert_part=part - 2),
                dict(vert_part=part.long()), dict(vert_part=part[:-1]), dict(vert_part=None), dict(vert_w=w * 1.5), dict(vert_w=-w),
                dict(vert_w=w * float("nan")), dict(vert_w=w.double()), dict(vert_w=w[:-1]), dict(knuckle=torch.zeros(1, 3, 3)),
                dict(knuckle=torch.zeros(2, 3)), dict(knuckle=torch.zeros(1, 2, 3, dtype=torch.float64)), dict(knuckle=None),
                dict(pivot=torch.zeros(3)), dict(pivot=None), dict(curl=-1.0), dict(curl=float("inf")), dict(curl=float("nan")),
                dict(spin=-1.0), dict(push=float("nan")), dict(pull=-0.5), dict(max_curl=0.0), dict(max_curl=-0.1), dict(max_curl=3.2),
                dict(max_curl=float("nan")), dict(steps=65), dict(steps=-1), dict(obj=torch.zeros(1, 0, 3)), dict(hand=hand.double())):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_refine_fingers(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    for bad in (dict(vert_part=np.full(V, 2)), dict(vert_w=np.full(V, 1.5)), dict(joints=[]), dict(joints=[1] * 6), dict(vert_w=np.ones(V - 1))):
        with pytest.raises(RuntimeError, match="FingerRig"):
            contact.FingerRig(**{**dict(vert_part=np.zeros(V, np.int64), vert_w=np.ones(V), joints=[1, 4]), **bad})
    for kw in (dict(refine_steps=2, refine_curl=-1.0), dict(refine_steps=2, refine_curl=float("inf")), dict(refine_curl=1.0)):
        with pytest.raises(RuntimeError, match="refine_curl"):
            generate.generate_for_objects(None, [torch.zeros(4, 8)], 5, True, 0, [0], **kw)
    for a in (0.0, 3.2, float("nan")):
        with pytest.raises(RuntimeError, match="refine_max_curl"):
            generate.generate_for_objects(None, [torch.zeros(4, 8)], 5, True, 0, [0], refine_steps=2, refine_curl=1.0, refine_max_curl=a)


# ------------------------------------------------------------------------------------------------------ CPU: the reference itself
def test_reference_without_curl_is_the_rigid_reference():
    hand, f, obj, pivot = rigid_tests.five_situations()
    rng = np.random.default_rng(3)
    part, w = rng.integers(-1, 3, hand.shape[1]), rng.random(hand.shape[1]).astype(np.float32)
    knuckle = rng.normal(0, 0.03, (len(hand), 3, 3)).astype(np.float32)
    for steps, spin in ((0, 1.0), (5, 1.0), (5, 0.0)):
        got = dict(zip(NAMES, fref.grasp_refine_fingers(hand, f, obj, pivot, part, w, knuckle, steps, spin=spin, curl=0.0)))
        want = rref.grasp_refine_rigid(hand, f, obj, pivot, steps, spin=spin)
        for k, x in zip(rigid_tests.NAMES, want):
            if k == "penetration":
                nan = np.isnan(x)
                assert np.array_equal(np.isnan(got[k]), nan) and np.array_equal(bits(got[k])[~nan], bits(x)[~nan])
            else:
                assert np.array_equal(got[k].view(np.uint32), x.view(np.uint32)), (steps, spin, k)
        assert np.array_equal(bits(got["finger_quat"]), bits(np.tile(IDENTITY, (len(hand), 3, 1))))
        scores = ref.grasp_scores(hand, f, obj)
        nan = np.isnan(scores[0])
        assert np.array_equal(bits(got["penetration0"])[~nan], bits(scores[0])[~nan]) and np.array_equal(np.isnan(got["penetration0"]), nan)
        assert np.array_equal(got["n_interior0"], scores[1]) and np.array_equal(got["n_contact0"], scores[2])


HOOK_KEPT = {0.0: 6.234e-4, 1.0: 5.552e-4}   # the kept penetration without and with the curl, of 2.242e-3 as given (this reference)


def test_reference_frees_the_hooked_finger_by_curling():
    """No rigid motion frees the tip without losing the bar's rest, the finger's own turn does: with the curl on the kept penetration
    is strictly below the one without, and both are no worse than the hand as given."""
    case, kept = hooked(), {}
    for curl in (0.0, 1.0):
        traces = []
        o = dict(zip(NAMES, run_ref(case, 8, traces, curl=curl)))
        kept[curl] = float(o["penetration"][0])
        angle = float(rref.quat_angle(o["finger_quat"][0])[0])
        print("curl", curl, "kept", int(o["iter"][0]), "pen", kept[curl], "of", float(o["penetration0"][0]), "finger angle (deg)",
              float(np.degrees(angle)), "wrist angle (deg)", float(np.degrees(rref.quat_angle(o["quat"])[0])))
        assert kept[curl] <= float(o["penetration0"][0]) and o["n_contact"][0] >= 1
        assert (curl > 0) == (angle > 0)
        assert abs(np.linalg.norm(o["finger_quat"][0, 0].astype(np.float64)) - 1.0) <= 1e-6
        assert abs(kept[curl] - HOOK_KEPT[curl]) <= 1e-3 * HOOK_KEPT[curl], "the figures quoted in DESIGN.md are stale"
    assert kept[1.0] < kept[0.0]


def refused_case():
    """The hooked finger with max_curl = 0.015 rad: the finger's first turn (0.0117 rad) is accepted, the second would exceed the
    limit and is refused, later ones (back towards the hand as given) are accepted again -- chosen by running the reference."""
    return {**hooked(), "kw": dict(max_curl=0.015)}


def test_reference_refuses_a_turn_beyond_max_curl_and_accepts_later_ones():
    traces = []
    o = dict(zip(NAMES, run_ref(refused_case(), 6, traces)))
    acc, refd = [x[7][0] for x in traces[0][:-1]], [x[8][0] for x in traces[0][:-1]]
    print("accepted", acc, "refused", refd, "angles", [float(rref.quat_angle(x[6][0])) for x in traces[0]])
    assert acc[0] and refd[1] and not acc[1] and any(acc[2:])
    assert np.array_equal(bits(traces[0][2][6]), bits(traces[0][1][6])), "a refused turn changed the finger's state"
    assert all(float(rref.quat_angle(x[6][0])) <= 0.015 + 1e-6 for x in traces[0])
    assert float(o["penetration"][0]) <= float(o["penetration0"][0])


# ------------------------------------------------------------------------------------------------------ CPU: the rig and the pose
def test_finger_rig_of_the_real_hand_model(tmp_path):
    layer = real_layer(tmp_path)
    rig = contact.FingerRig.from_mano(layer)
    parents = [int(p) for p in layer._packed.parents]
    assert parents == [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
    assert rig.joints == [1, 4, 7, 10, 13] and rig.n_fingers == 5 and rig.n_verts == 778
    from dvqvae_amd import mano as dmano
    weights = np.asarray(dmano.read_mano_pkl(mano_pkl(tmp_path))["weights"], np.float64)         # [778,16] as the file holds them
    chains = [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15]]
    sums = np.stack([weights[:, c].sum(1) for c in chains], 1)
    top = sums.max(1).astype(np.float32)
    assert np.array_equal(rig.vert_w, np.clip(top, 0, 1)) and rig.vert_w.dtype == np.float32 and rig.vert_part.dtype == np.int32
    assert np.array_equal(rig.vert_part, np.where(top > 0, sums.argmax(1), -1))
    counts = (int((rig.vert_w == 1).sum()), int(((rig.vert_w > 0) & (rig.vert_w < 1)).sum()), int((rig.vert_part < 0).sum()))
    second = np.sort(sums, 1)[:, -2].max()
    print("vertices with weight 1 / in between / of no finger:", counts, "largest second chain sum", second)
    assert counts == (349, 376, 53) and sum(counts) == 778
    assert second < 0.1901                                                           # 0.19 to two digits: no vertex hangs between two fingers
    part, w = rig.on("cpu")
    assert part.dtype == torch.int32 and w.dtype == torch.float32 and rig.on("cpu")[0] is part


FINGER_REF_ERR = 3.1e-10    # metres: the largest difference the float64 numpy restatement gives below (measured: 3.005e-10)


def _finger_turns(B, P, top):
    rnd = lambda tag, shape, scale: synth.synthetic_normal(shape, 78, f"fingers/helpers/{tag}", scale).numpy().astype(np.float64)
    axis = rnd("ax", (B, P, 3), 1.0)
    axis /= np.linalg.norm(axis, axis=2, keepdims=True)
    angle = np.linspace(0.0, top, B)[:, None] * np.ones((1, P))
    return np.concatenate([np.cos(0.5 * angle)[..., None], np.sin(0.5 * angle)[..., None] * axis], 2), angle


def test_compose_finger_pose_on_the_real_hand_model(tmp_path):
    """Turning finger f by D_f about its knuckle IS posing the hand with compose_finger_pose's hand_pose: the knuckles stay and every
    joint of the chain is D_f of the first pass's.  Both sides in float64 (tests/mano_ref.py on the real model).  As in the rigid
    test, the two do not agree to float64 rounding because the layer's Rodrigues formula takes the angle of ``r + 1e-8``: the numpy
    restatement differs by FINGER_REF_ERR, and the torch helper may differ by four times that."""
    from dvqvae_amd import mano as dmano
    layer = real_layer(tmp_path)
    rig = contact.FingerRig.from_mano(layer)
    arrays = mano_ref.device_arrays(dmano.read_mano_pkl(mano_pkl(tmp_path)))
    B, P = 24, 5
    rnd = lambda tag, shape, scale: synth.synthetic_normal(shape, 78, f"fingers/helpers/{tag}", scale).numpy().astype(np.float64)
    betas, pose, go, tr = rnd("b", (B, 10), 1.0), rnd("p", (B, 45), 0.5), rnd("g", (B, 3), 1.2), rnd("t", (B, 3), 0.1)
    q, angle = _finger_turns(B, P, 0.35)                                             # all five fingers at once, the identity row included
    q[2::3] *= -1.0                                                                  # either sign is the same turn
    q[5] *= 1.0 + 3e-8                                                               # unit only to fp32 rounding, as the kernel's
    _, joints0 = mano_ref.mano_ref(arrays, betas, pose, go, tr)
    comps = arrays["hands_components"][:45]
    assert np.linalg.cond(comps) < 100 and np.abs(comps @ comps.T - np.eye(45)).max() > 0.5      # invertible, not orthonormal
    chains = [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15]]
    R = rref.quat_matrix64(q)                                                        # [B,P,3,3]

    def chain_error(joints):
        worst = 0.0
        for f, chain in enumerate(chains):
            c = joints0[:, chain[0]][:, None]
            want = np.einsum("bij,bvj->bvi", R[:, f], joints0[:, chain] - c) + c
            worst = max(worst, float(np.abs(joints[:, chain] - want).max()))
        return max(worst, float(np.abs(joints[:, 0] - joints0[:, 0]).max()))

    pose_ref = fref.compose_finger_pose64(comps, np.zeros(45), go, pose, q, rig.joints)
    err_ref = chain_error(mano_ref.mano_ref(arrays, betas, pose_ref, go, tr)[1])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    got = contact.compose_finger_pose(layer, T(go), T(pose), T(q), rig)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, 45)
    err = chain_error(mano_ref.mano_ref(arrays, betas, got.numpy(), go, tr)[1])
    print(f"chain joints against D_f of the first pass: float64 reference {err_ref:.3e} m, torch helper {err:.3e} m; the two poses "
          f"differ by {np.abs(got.numpy() - pose_ref).max():.3e}")
    assert err_ref <= FINGER_REF_ERR, "the recorded figure of the reference is stale"
    assert err_ref >= FINGER_REF_ERR / 4, "the recorded figure of the reference is stale (too wide)"
    assert err <= 4 * FINGER_REF_ERR
    # dtype, the identity and the batch
    pose32, go32 = T(pose.astype(np.float32)), T(go.astype(np.float32))
    ident = torch.from_numpy(np.tile(IDENTITY, (B, P, 1)))
    assert contact.compose_finger_pose(layer, go32, pose32, T(q), rig).dtype == torch.float32
    assert torch.equal(contact.compose_finger_pose(layer, go32, pose32, ident, rig).view(torch.int32), pose32.view(torch.int32))
    assert torch.equal(got[0].view(torch.int64), T(pose)[0].view(torch.int64))       # row 0 turns nothing
    mixed = T(q).clone()
    mixed[3, 1:] = torch.from_numpy(np.tile(IDENTITY.astype(np.float64), (P - 1, 1)))            # one finger turned: not an identity row
    assert not torch.equal(contact.compose_finger_pose(layer, T(go), T(pose), mixed, rig)[3], T(pose)[3])
    for b in (0, 7, B - 1):                                                          # a row alone gives the row's bits
        assert torch.equal(contact.compose_finger_pose(layer, T(go[b:b + 1]), T(pose[b:b + 1]), T(q[b:b + 1]), rig), got[b:b + 1])


BLEND_ERR = {0.05: (4.4e-4, 2.72e-5), 0.2: (1.81e-3, 1.10e-4), 0.35: (3.24e-3, 1.94e-4)}   # angle: (max, mean) in metres, this test's own run


def test_apply_fingers_against_the_reposed_hand(tmp_path):
    """What the kernel searches with against what is written: contact.apply_fingers (the blend model) on the first pass's vertices
    against MANO posed with compose_finger_pose's parameters, float64, all five fingers turned by the same angle about random axes.
    The recorded figures are this test's own (printed below); they are asserted not to be stale: within 10 % from below, not above."""
    from dvqvae_amd import mano as dmano
    layer = real_layer(tmp_path)
    rig = contact.FingerRig.from_mano(layer)
    arrays = mano_ref.device_arrays(dmano.read_mano_pkl(mano_pkl(tmp_path)))
    B, P = 16, 5
    rnd = lambda tag, shape, scale: synth.synthetic_normal(shape, 79, f"fingers/blend/{tag}", scale).numpy().astype(np.float64)
    betas, pose, go, tr = rnd("b", (B, 10), 1.0), rnd("p", (B, 45), 0.5), rnd("g", (B, 3), 1.2), rnd("t", (B, 3), 0.1)
    axis = rnd("ax", (B, P, 3), 1.0)
    axis /= np.linalg.norm(axis, axis=2, keepdims=True)
    verts0, joints0 = mano_ref.mano_ref(arrays, betas, pose, go, tr)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    knuckles = joints0[:, rig.joints]
    figures = {}
    for angle in BLEND_ERR:
        q = np.concatenate([np.full((B, P, 1), np.cos(0.5 * angle)), np.sin(0.5 * angle) * axis], 2)
        model = contact.apply_fingers(T(verts0), rig, T(knuckles), T(q))
        assert model.dtype == torch.float64 and tuple(model.shape) == (B, 778, 3)
        want = fref.apply_fingers64(verts0, rig.vert_part, rig.vert_w, knuckles, q)
        assert np.abs(model.numpy() - want).max() <= 64 * np.finfo(np.float64).eps
        posed, _ = mano_ref.mano_ref(arrays, betas, contact.compose_finger_pose(layer, T(go), T(pose), T(q), rig).numpy(), go, tr)
        diff = np.linalg.norm(posed - model.numpy(), axis=2)
        moved = np.linalg.norm(posed - verts0, axis=2).max()
        solid = diff[:, rig.vert_w == 1].max()
        print(f"angle {angle} rad: max {diff.max() * 1e3:.3f} mm, mean {diff.mean() * 1e3:.4f} mm, largest true motion {moved * 1e3:.1f} mm, "
              f"vertices of weight 1: {solid * 1e3:.3f} mm")
        figures[angle] = (float(diff.max()), float(diff.mean()))
        free = rig.vert_part < 0
        assert torch.equal(model[:, free], T(verts0)[:, free])                       # a vertex of no finger keeps its bits
    for angle, (top, mean) in BLEND_ERR.items():                                     # after all three are printed
        assert 0.9 * top <= figures[angle][0] <= top and 0.9 * mean <= figures[angle][1] <= mean, "the recorded figures are stale"
    ident = torch.from_numpy(np.tile(IDENTITY.astype(np.float64), (B, P, 1)))
    v32 = T(verts0.astype(np.float32))
    assert torch.equal(contact.apply_fingers(v32, rig, T(knuckles.astype(np.float32)), ident.float()).view(torch.int32), v32.view(torch.int32))
    assert torch.equal(contact.apply_fingers(T(verts0[2:3]), rig, T(knuckles[2:3]), T(q[2:3])), model[2:3])   # a row alone


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def sectors(hand, P):
    """A rig laid over a blob: finger = the sector of the vertex's angle about z in the template, -1 near the axis."""
    v = hand[0]
    ang = np.arctan2(v[:, 1], v[:, 0])
    part = np.floor((ang + np.pi) / (2 * np.pi) * P).astype(np.int64).clip(0, P - 1)
    return np.where(np.hypot(v[:, 0], v[:, 1]) < 0.01, -1, part)


def finger_case(name, tmp_path):
    """hand [B,V,3], faces, obj [B,N,3], pivot [B,3], part [V], w [V], knuckle [B,P,3] (numpy) and keywords."""
    rng = lambda tag, shape, scale: synth.synthetic_normal(shape, 35, f"fingers/{name}/{tag}", scale).numpy().astype(np.float32)
    uni = lambda tag, shape, lo, hi: synth.synthetic_uniform(shape, 36, f"fingers/{name}/{tag}", lo, hi).numpy().astype(np.float32)
    if name == "hooked":
        return hooked()
    if name == "refused":
        return refused_case()
    if name == "pinch":                                                              # the rigid test's pinch, both ends of the bar hinged
        hand, f, cloud, pivot = rigid_tests.pinch()
        x = hand[:, 0].astype(np.float64)
        w = np.clip((np.abs(x) - 0.02) / 0.02, 0.0, 1.0).astype(np.float32)
        part = np.where(w > 0, np.where(x > 0, 0, 1), -1)
        return dict(hand=hand[None], faces=f, obj=cloud[None], pivot=pivot[None], part=part, w=w,
                    knuckle=np.asarray([[[0.02, 0, 0], [-0.02, 0, 0]]], np.float32))
    if name == "1x1x1":                                                              # one vertex, one degenerate face, one finger
        hand, f, obj, pivot = rigid_tests.rigid_case("1x1x1", tmp_path)
        return dict(hand=hand, faces=f, obj=obj, pivot=pivot, part=np.zeros(1, np.int64), w=np.ones(1, np.float32),
                    knuckle=(hand + rng("k", (1, 1, 3), 0.03)).astype(np.float32))
    if name == "2x1030x5":                                                           # the pyramid: V below one vector, two passes of points
        hand, f, obj, pivot = rigid_tests.rigid_case("2x1030x5", tmp_path)
        return dict(hand=hand, faces=f, obj=obj, pivot=pivot, part=np.asarray([0, 0, -1, 1, 1]), w=np.asarray([1, 0.5, 0, 0.25, 1], np.float32),
                    knuckle=rng("k", (2, 2, 3), 0.02))
    if name == "5x257x778":                                                          # the MANO template with the rig of the real model
        hand, f, obj, pivot = rigid_tests.rigid_case("5x257x778", tmp_path)
        layer = real_layer(tmp_path)
        rig = contact.FingerRig.from_mano(layer)
        joints = layer._packed.tensors["j_template"].numpy()[rig.joints]            # the template's knuckles
        return dict(hand=hand, faces=f, obj=obj, pivot=pivot, part=rig.vert_part.astype(np.int64), w=rig.vert_w,
                    knuckle=(joints[None] + rng("k", (5, 5, 3), 0.001)).astype(np.float32))
    if name in ("3x300x776_no_finger", "3x300x776_between"):
        hand, f, obj, pivot = rigid_tests.rigid_case("3x300x776", tmp_path)
        if name.endswith("no_finger"):                                               # every vertex of no finger: the rigid kernel's run
            part, w = np.full(776, -1), uni("w", (776,), 0.0, 1.0)
        else:                                                                        # every weight strictly between 0 and 1
            part, w = sectors(hand, 5), uni("w", (776,), 0.2, 0.8)
            assert ((w > 0) & (w < 1)).all() and set(part) == {-1, 0, 1, 2, 3, 4}
        return dict(hand=hand, faces=f, obj=obj, pivot=pivot, part=part, w=w, knuckle=rng("k", (3, 5, 3), 0.02))
    assert name == "5x257x776"                                                       # the five situations, a NaN row among them
    hand, f, obj, pivot = rigid_tests.five_situations()
    return dict(hand=hand, faces=f, obj=obj, pivot=pivot, part=sectors(hand, 4), w=uni("w", (776,), 0.0, 1.0), knuckle=rng("k", (5, 4, 3), 0.02))


def run_fingers(case, steps, obj_dev=None, **kw):
    hand = case["hand"]
    topo = contact.HandTopology(case["faces"], hand.shape[1], DEV)
    rig = contact.FingerRig(case["part"], case["w"], list(range(1, 1 + case["knuckle"].shape[1])), DEV)
    out = contact.refine_fingers(topo, rig, gpu(hand), gpu(case["obj"]) if obj_dev is None else obj_dev, gpu(case["pivot"]),
                                 gpu(case["knuckle"]), steps, **{**case.get("kw", {}), **kw})
    assert tuple(out) == NAMES
    B, P = hand.shape[0], case["knuckle"].shape[1]
    shapes = dict(offset=(B, 3), quat=(B, 4), finger_quat=(B, P, 4))
    for k, v in out.items():
        assert v.dtype == (torch.int32 if k.startswith(("iter", "n_")) else torch.float32) and tuple(v.shape) == shapes.get(k, (B,)), k
    return topo, rig, {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal_bits(got, want, tag=""):
    """All ten outputs bit for bit, no row exempted (a NaN is a NaN: its payload is nobody's contract)."""
    want = dict(zip(NAMES, want))
    print(tag, {k: got[k].tolist() for k in NAMES}, "reference", {k: want[k].tolist() for k in NAMES})
    for k in NAMES:
        g, w = got[k], want[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (tag, k)
        if g.dtype == np.float32:
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), (tag, k, g, w)
            assert np.array_equal(bits(g)[~nan], bits(w)[~nan]), (tag, k, g, w)
        else:
            assert np.array_equal(g, w), (tag, k, g, w)


CASES = [("hooked", 0), ("hooked", 1), ("hooked", 6), ("refused", 6), ("pinch", 6), ("1x1x1", 3), ("2x1030x5", 4), ("5x257x778", 1),
         ("5x257x778", 6), ("3x300x776_no_finger", 6), ("3x300x776_between", 6), ("5x257x776", 6)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,steps", CASES)
def test_grasp_refine_fingers_equals_the_reference_bit_for_bit(name, steps, tmp_path):
    case = finger_case(name, tmp_path)
    _, _, got = run_fingers(case, steps)
    traces = []
    want = run_ref(case, steps, traces)
    assert_equal_bits(got, want, f"{name} steps {steps}")
    B, P = case["knuckle"].shape[:2]
    accepted = [any(any(x[7]) for x in tr if x[7]) for tr in traces]
    if steps == 0:
        assert not got["iter"].any() and not bits(got["offset"]).any() and np.array_equal(got["finger_quat"], np.tile(IDENTITY, (B, P, 1)))
    elif name == "3x300x776_no_finger":
        assert not any(accepted) and np.array_equal(got["finger_quat"], np.tile(IDENTITY, (B, P, 1)))
        rigid = rref.grasp_refine_rigid(case["hand"], case["faces"], case["obj"], case["pivot"], steps)
        for k, x in zip(rigid_tests.NAMES, rigid):
            assert np.array_equal(got[k].view(np.uint32), x.view(np.uint32)), k
    elif name == "refused":
        assert any(any(x[8]) for x in traces[0] if x[8]) and accepted[0]
    elif name != "1x1x1":
        assert any(accepted), "no finger of the case turns: the curl is not exercised"
        if steps > 1:
            assert (got["finger_quat"][..., 0] != 1).any(), "no kept iterate has a curled finger"
    if name == "5x257x776":
        assert np.isnan(got["penetration"][4]) and np.isnan(got["penetration0"][4]) and got["iter"][4] == 0
        assert np.array_equal(got["finger_quat"][4], np.tile(IDENTITY, (P, 1))) and got["n_contact0"][3] == 0 and got["iter"][3] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["nan_in_the_hand", "inf_in_the_hand", "nan_in_the_cloud", "inf_in_the_cloud", "nan_in_a_knuckle",
                                  "inf_in_a_knuckle"])
def test_grasp_refine_fingers_on_a_coordinate_that_is_not_finite(what):
    """A NaN in the hand or the cloud makes iterate 0 of class 2, the only one.  An Inf in the hand or the cloud where it enters a sum
    makes the step not finite: the next iterate is of class 2, ends the loop and never replaces the iterate kept.  A knuckle that is
    not finite only stops its own finger: a NaN makes the finger's Q NaN (no turn), an Inf the candidate NaN (refused); the row goes
    on as the definition says, and the other finger still turns."""
    case = finger_case("pinch", None)
    hand, cloud, knuckle = case["hand"].copy(), case["obj"].copy(), case["knuckle"].copy()
    steps = 6
    bad = np.nan if what.startswith("nan") else np.inf
    if what.endswith("hand"):
        hand[0, 300, 1] = bad
    elif what == "nan_in_the_cloud":
        cloud[0, 17, 0] = bad
    elif what == "inf_in_the_cloud":
        from oracle import contact_oracle
        n0 = contact_oracle.vertex_normals(hand, case["faces"])[0, 0]                # the scan gives a point at infinity vertex 0
        axis = int(np.argmax(np.abs(n0)))
        cloud[0, 17, axis] = -np.inf if n0[axis] > 0 else np.inf                     # (hand[0] - p) . n0 = +inf: interior
    else:
        knuckle[0, 0, 1] = bad
    case = {**case, "hand": hand, "obj": cloud, "knuckle": knuckle}
    traces = []
    want = run_ref(case, steps, traces)
    _, _, got = run_fingers(case, steps)
    assert_equal_bits(got, want, what)
    trace = traces[0]
    if what.endswith("knuckle"):
        assert all(np.array_equal(x[6][0], IDENTITY) for x in trace), "the finger of the knuckle turned"
        assert any(x[7][1] for x in trace if x[7]), "the other finger does not turn"
        assert not np.isnan(got["penetration"][0]) and got["iter"][0] > 0
    else:
        assert trace[-1][2] == 2 and len(trace) <= 2 < steps + 1, "the loop did not end on the iterate of class 2"
        assert got["iter"][0] == 0 and not bits(got["offset"]).any() and np.array_equal(got["quat"][0], IDENTITY)
        assert np.array_equal(got["finger_quat"][0], np.tile(IDENTITY, (2, 1)))
        assert np.isnan(got["penetration"][0]) == what.startswith("nan")


@pytest.mark.gpu
def test_grasp_refine_fingers_without_curl_gives_the_bits_of_the_rigid_kernel(tmp_path):
    for name, steps, spin in (("5x257x776", 5, 1.0), ("5x257x778", 4, 1.0), ("5x257x776", 5, 0.0)):
        case = finger_case(name, tmp_path)
        topo, _, got = run_fingers(case, steps, curl=0.0, spin=spin)
        want = contact.refine_rigid(topo, gpu(case["hand"]), gpu(case["obj"]), gpu(case["pivot"]), steps, spin=spin)
        if spin == 0.0:
            shift = contact.refine_translation(topo, gpu(case["hand"]), gpu(case["obj"]), steps)
        for k in rigid_tests.NAMES:
            w = want[k].cpu().numpy()
            real = ~np.isnan(w) if k == "penetration" else np.ones(len(w), bool)     # a NaN is a NaN, whatever its payload
            assert np.array_equal(got[k][real].view(np.uint32), w[real].view(np.uint32)), (name, k)
            if spin == 0.0 and k != "quat":
                assert np.array_equal(got[k][real].view(np.uint32), shift[k].cpu().numpy()[real].view(np.uint32)), (name, k, "translation")
        assert np.array_equal(np.isnan(got["penetration"]), torch.isnan(want["penetration"]).cpu().numpy())
        assert np.array_equal(bits(got["finger_quat"]), bits(np.tile(IDENTITY, got["finger_quat"].shape[:2] + (1,))))
        assert (got["iter"] > 0).any()


@pytest.mark.gpu
def test_grasp_refine_fingers_with_no_steps_gives_the_bits_of_grasp_scores(tmp_path):
    for name, steps in (("5x257x776", 0), ("5x257x778", 0), ("5x257x778", 4)):
        case = finger_case(name, tmp_path)
        topo, _, got = run_fingers(case, steps)
        want = contact.grasp_scores(topo, gpu(case["hand"]), gpu(case["obj"]))
        pen = want["penetration"].cpu().numpy()
        for suffix in ("0",) + (("",) if steps == 0 else ()):                        # iterate 0 always; the kept one with no steps
            nan = np.isnan(got["penetration" + suffix])
            assert np.array_equal(nan, np.isnan(pen))
            assert np.array_equal(bits(got["penetration" + suffix])[~nan], bits(pen)[~nan])
            assert np.array_equal(got["n_interior" + suffix], want["n_interior"].cpu().numpy())
            assert np.array_equal(got["n_contact" + suffix], want["n_contact"].cpu().numpy())
        if steps == 0:
            assert not got["iter"].any() and not bits(got["offset"]).any() and np.array_equal(got["quat"], np.stack([IDENTITY] * len(pen)))


@pytest.mark.gpu
def test_grasp_refine_fingers_of_a_row_does_not_depend_on_the_batch(tmp_path):
    case = finger_case("5x257x776", tmp_path)
    topo = contact.HandTopology(case["faces"], 776, DEV)
    rig = contact.FingerRig(case["part"], case["w"], [1, 2, 3, 4], DEV)
    pick = torch.arange(8, device=DEV) % 5
    g = lambda k: gpu(case[k])
    big = contact.refine_fingers(topo, rig, g("hand")[pick].contiguous(), g("obj")[pick].contiguous(), g("pivot")[pick].contiguous(),
                                 g("knuckle")[pick].contiguous(), 5)
    for b in range(5):
        one = contact.refine_fingers(topo, rig, g("hand")[b:b + 1], g("obj")[b:b + 1], g("pivot")[b:b + 1], g("knuckle")[b:b + 1], 5)
        for k in NAMES:
            rows = big[k][pick == b].cpu().numpy()
            alone = one[k].cpu().numpy()
            assert np.array_equal(rows.view(np.uint32), np.repeat(alone, rows.shape[0], axis=0).view(np.uint32)), (k, b)
    assert (big["iter"] > 0).any() and (big["iter"] == 0).any()
    assert (big["finger_quat"][..., 0] != 1).any(), "no kept iterate has a curled finger"
    empty = contact.refine_fingers(topo, rig, g("hand")[:0].contiguous(), g("obj")[:0].contiguous(), g("pivot")[:0].contiguous(),
                                   g("knuckle")[:0].contiguous(), 5)
    assert tuple(empty["finger_quat"].shape) == (0, 4, 4) and tuple(empty["offset"].shape) == (0, 3) and empty["penetration0"].shape == (0,)


@pytest.mark.gpu
def test_grasp_refine_fingers_reads_a_channel_first_view_in_place():
    v, f = ref.sphere_mesh()
    B, N = 3, 500
    cloud = synth.synthetic_normal((B, 4, N), 32, "refine/cf", 0.02)                    # [B,4,N] as the generation path holds it
    cloud[:, 0] += 0.06                                                                  # across the hand's surface on the +x side
    hand = (v[None] * np.asarray([1.0, 0.9, 1.1], np.float32)[:, None, None]).astype(np.float32)
    x = v[:, 0].astype(np.float64)
    w = np.clip((x - 0.01) / 0.02, 0.0, 1.0).astype(np.float32)
    case = dict(hand=hand, faces=f, obj=cloud[:, :3].transpose(1, 2).contiguous().numpy(), part=np.where(w > 0, 0, -1), w=w,
                pivot=np.asarray([[-0.05, 0.0, 0.0], [-0.04, 0.01, 0.0], [-0.05, 0.0, 0.02]], np.float32),
                knuckle=np.asarray([[[0.01, 0, 0]], [[0.01, 0.005, 0]], [[0.012, 0, -0.004]]], np.float32))
    view = gpu(cloud)[:, :3].transpose(1, 2)                                             # strides (4N, 1, N)
    assert not view.is_contiguous()
    _, _, got = run_fingers(case, 4, obj_dev=view)
    _, _, copy = run_fingers(case, 4)
    for k in NAMES:
        assert np.array_equal(got[k].view(np.uint32), copy[k].view(np.uint32)), k
    assert_equal_bits(got, run_ref(case, 4), "channel-first")
    assert (got["iter"] > 0).any() and (got["finger_quat"][..., 0] != 1).any()


@pytest.mark.gpu
def test_grasp_refine_fingers_refuses_what_the_kernel_cannot_hold():
    v, f = ref.sphere_mesh(4, 6)
    topo = contact.HandTopology(f, len(v), DEV)
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL, nothing launched
    one = torch.zeros(64, device=DEV)
    p = one.data_ptr()
    ok = dict(V=5, P=2, N=4, B=1, steps=2, push=1.0, pull=0.25, spin=1.0, curl=1.0, min_w=0.98, knuckle=p, part=p, fquat=p, pen0=p)
    for bad in (dict(V=2049), dict(V=0), dict(N=0), dict(B=-1), dict(steps=-1), dict(steps=65), dict(P=0), dict(P=6), dict(curl=-1.0),
                dict(curl=float("inf")), dict(curl=float("nan")), dict(spin=float("nan")), dict(push=-1.0), dict(min_w=-0.1), dict(min_w=1.5),
                dict(min_w=float("nan")), dict(knuckle=None), dict(part=None), dict(fquat=None), dict(pen0=None)):
        a = {**ok, **bad}
        rc = lib.dvq_grasp_refine_fingers(p, topo.faces.data_ptr(), topo.vf_off.data_ptr(), topo.vf_face.data_ptr(), a["V"], a["part"], p,
                                          a["P"], p, 0, 3, 1, a["B"], a["N"], p, a["knuckle"], 0.0004, a["steps"], a["push"], a["pull"],
                                          a["spin"], a["curl"], a["min_w"], 1, p, p, a["fquat"], p, p, p, p, a["pen0"], p, p, None)
        assert rc == 1, bad
    torch.cuda.synchronize()
    assert not one.any(), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------------ GPU: end to end
E2E_SEED, E2E_M, E2E_K, E2E_STEPS = rigid_tests.E2E_SEED, rigid_tests.E2E_M, rigid_tests.E2E_K, rigid_tests.E2E_STEPS
E2E_INDICES = rigid_tests.E2E_INDICES
_mano = rigid_tests._mano


def _key(scores, min_contact=1):
    cls, key = contact.select_keys(scores, "penetration", min_contact)
    return cls.cpu().numpy(), key.cpu().numpy()


@pytest.mark.gpu
def test_best_of_m_with_curled_fingers_end_to_end(tmp_path):
    """Synthetic weights, the real MANO, M = 8, keep = 4, three steps, the curl on: some finger turns; the vertices written are MANO
    of the parameters written; the scores reported are those of the hands written; no written row has a worse key than the hand as
    generated, and a reverted row carries its generated parameters bit for bit; the JSON does not depend on rows_per_call."""
    net = rigid_tests._gennet(tmp_path)
    objs, M, k = rigid_tests.e2e_objects(), E2E_M, E2E_K
    plain = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES)            # all M rows, unrefined
    topo = contact.HandTopology(np.asarray(net.rh_mano.faces), 778, DEV)
    rig = contact.FingerRig.from_mano(net.rh_mano)
    first, curled, reverted = None, 0, 0
    for rows_per_call in (16384, 8):
        got = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, rows_per_call=rows_per_call, candidates=M,
                                            refine_steps=E2E_STEPS, refine_spin=1.0, refine_curl=1.0)
        for i, (g, p) in enumerate(zip(got, plain)):
            cand, j = g["candidate"], g["json"]
            old = p["params"][cand].contiguous()
            assert tuple(g["params"].shape) == (k, 61) and tuple(g["refine_curl"].shape) == (k, 5, 3) and g["refine_curl"].dtype == torch.float64
            assert tuple(g["refine_reverted"].shape) == (k,) and g["refine_reverted"].dtype == torch.int32
            assert torch.equal(g["params"][:, :10], old[:, :10])
            assert torch.equal(g["params"][:, 58:61], old[:, 58:61] + g["refine_offset"]), f"object {i}: translation"
            quats = contact.axis_angle_quat(g["refine_curl"].reshape(-1, 3)).reshape(k, 5, 4)
            want_pose = contact.compose_finger_pose(net.rh_mano, old[:, 10:13], old[:, 13:58], quats, rig)
            assert torch.allclose(g["params"][:, 13:58], want_pose, rtol=0, atol=1e-5), f"object {i}: hand_pose"
            new = _mano(net, g["params"].contiguous())
            assert torch.equal(new.vertices, g["vertices"]), f"object {i}: the vertices are not those of the parameters written"
            R = np.asarray(j["R_list"], np.float64)                                      # [k,3,4]: rotation | translation
            cloud = ops.transform_cloud(gpu(objs[i]).contiguous(), gpu(R[:, :, :3].astype(np.float32)).contiguous(),
                                        gpu(R[0, :, 3].astype(np.float32)).contiguous())[:, :3].transpose(1, 2)
            scores = contact.grasp_scores(topo, g["vertices"], cloud)
            pen = scores["penetration"].cpu().numpy()
            assert np.array_equal(bits(np.asarray(j["penetration"], np.float32)), bits(pen)), f"object {i}: JSON penetration"
            assert j["n_interior"] == scores["n_interior"].cpu().numpy().tolist()
            assert j["n_contact"] == scores["n_contact"].cpu().numpy().tolist()
            cls1, key1 = _key(scores)
            cls0, key0 = _key(contact.grasp_scores(topo, p["vertices"][cand].contiguous(), cloud))
            for r in range(k):                                                       # never worse than the hand as generated
                assert (cls1[r], key1[r]) <= (cls0[r], key0[r]) or (np.isnan(key1[r]) and np.isnan(key0[r])), (i, r, cls1[r], key1[r], cls0[r], key0[r])
            rev = g["refine_reverted"].cpu().numpy().astype(bool)
            assert j["refine_reverted"] == rev.astype(int).tolist()
            for r in np.nonzero(rev)[0]:                                             # a reverted row is the generated one, bit for bit
                assert torch.equal(g["params"][r], old[r]) and torch.equal(g["vertices"][r], p["vertices"][cand][r])
                assert not g["refine_offset"][r].any() and not g["refine_curl"][r].any() and not g["refine_rotation"][r].any()
                assert int(g["refine_iter"][r]) == 0
            written = np.asarray(j["recon_params"], np.float32)[:, 0]
            assert np.array_equal(bits(written), bits(g["params"].cpu().numpy()))
            assert j["refine_curl"] == g["refine_curl"].cpu().numpy().tolist()
            assert j["refine_rotation"] == g["refine_rotation"].cpu().numpy().tolist()
            assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact",
                              "refine_offset", "refine_iter", "refine_rotation", "refine_curl", "refine_reverted"}
            print(f"rows_per_call {rows_per_call} object {i}: kept {cand.tolist()} iter {j['refine_iter']} reverted {j['refine_reverted']} "
                  f"pen {j['penetration']} as generated {key0.tolist()} curl {j['refine_curl']}")
            curled += sum(1 for c in j["refine_curl"] if any(x != 0 for a in c for x in a))
            reverted += int(rev.sum())
        dumped = [json.dumps(g["json"]) for g in got]
        if first is None:
            first = dumped
        assert dumped == first, f"rows_per_call {rows_per_call}: the JSON differs from the 16384-row call's"
    print(f"grasps with a curled finger: {curled}; reverted: {reverted}")
    assert curled, "no finger was turned: the curl is not exercised"


def _force_worse(monkeypatch):
    """contact.grasp_scores, as generate sees it, wrapped: the next call after ``state["rows"]`` is set reports those rows without a
    contact and with an infinite penetration -- a worse key than any hand as generated that has one -- and disarms itself.  Every other
    call, and every other row, is the real one's.  ``state["calls"]`` counts the calls."""
    real, state = contact.grasp_scores, {"rows": None, "calls": 0}

    def forced(topology, hand_xyz, obj_xyz, *a, **k):
        out = dict(real(topology, hand_xyz, obj_xyz, *a, **k))
        state["calls"] += 1
        if state["rows"] is not None:
            rows, state["rows"] = torch.as_tensor(state["rows"], device=hand_xyz.device), None
            out["penetration"], out["n_contact"] = out["penetration"].clone(), out["n_contact"].clone()
            out["penetration"][rows] = float("inf")
            out["n_contact"][rows] = 0
        return out

    monkeypatch.setattr(contact, "grasp_scores", forced)
    return real, state


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.gpu
def test_rows_that_come_out_worse_are_reverted_bit_for_bit(tmp_path, monkeypatch):
    """The guard of the articulated push-out with rows that DO come out worse: the score of the re-posed hands is replaced, for chosen
    rows, by one that is worse than any hand as generated (the end-to-end test above reverts nothing on its inputs).  Exactly those
    rows (and the rows that a run without the replacement reverts) report ``reverted``; they carry the generated parameters, the
    first pass's vertices AND joints, a zero offset, identity turns, iterate 0 and the scores of the hand as generated, bit for bit;
    every other row is the unforced run's, bit for bit, and has moved.  First on generate._refine_fingers_call itself, then through
    generate_for_objects without and with candidates.  The merged scores make the call's second grasp_scores launch unnecessary:
    one call per generate call."""
    net = rigid_tests._gennet(tmp_path)
    objs, M, k = rigid_tests.e2e_objects(), E2E_M, E2E_K
    plain = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES)            # all M rows, unrefined
    topo = contact.HandTopology(np.asarray(net.rh_mano.faces), 778, DEV)
    real, state = _force_worse(monkeypatch)
    params = torch.cat([p["params"] for p in plain]).contiguous()                                # [2M,61]: the rows of one call
    eye, zero3 = torch.eye(3, device=DEV).expand(M, 3, 3).contiguous(), torch.zeros(3, device=DEV)
    cloud = torch.cat([ops.transform_cloud(gpu(o).contiguous(), eye, zero3) for o in objs])[:, :3].transpose(1, 2)
    first = _mano(net, params)
    assert torch.equal(first.vertices, torch.cat([p["vertices"] for p in plain]))
    call = lambda: generate._refine_fingers_call(net, topo, params.clone(), first, cloud, E2E_STEPS, 1.0, 0.25, 1.0, 1.0, 0.35, 1)
    p_t, hands_t, r_t = call()                                                                   # unforced
    rev_t = r_t["reverted"].cpu().numpy().astype(bool)
    free = np.nonzero(~rev_t)[0]
    assert len(free) >= 3, "nearly every row is reverted without being forced: the inputs do not exercise the push-out"
    chosen = free[[1, len(free) // 2, len(free) - 1]]                                            # no pattern a mix-up of axes keeps
    state["rows"], before = chosen.tolist(), state["calls"]
    p_f, hands_f, r_f = call()
    assert state["calls"] == before + 1 and state["rows"] is None, "the guard scores the re-posed hands exactly once"
    rev_f = r_f["reverted"].cpu().numpy().astype(bool)
    want = rev_t.copy()
    want[chosen] = True
    print("reverted unforced", np.nonzero(rev_t)[0].tolist(), "chosen", chosen.tolist(), "reverted forced", np.nonzero(rev_f)[0].tolist())
    assert r_f["reverted"].dtype == torch.int32 and np.array_equal(rev_f, want) and rev_f[chosen].all() and rev_f.sum() >= 3
    rev, keep_ = torch.from_numpy(rev_f).to(DEV), torch.from_numpy(~rev_f).to(DEV)
    scores0 = real(topo, first.vertices, cloud)                                                  # of the hands as generated
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV)
    # the reverted rows: the generated hand, bit for bit
    assert _same_bits(p_f[rev], params[rev]) and _same_bits(hands_f.vertices[rev], first.vertices[rev])
    assert _same_bits(hands_f.joints[rev], first.joints[rev])
    assert not r_f["offset"][rev].view(torch.int32).any() and not r_f["iter"][rev].any()
    assert _same_bits(r_f["quat"][rev], ident.expand(int(rev.sum()), 4)) and _same_bits(r_f["finger_quat"][rev], ident.expand(int(rev.sum()), 5, 4))
    assert not r_f["curl"][rev].view(torch.int64).any() and not r_f["rotation"][rev].view(torch.int64).any()
    for name in ("penetration", "n_interior", "n_contact"):
        assert _same_bits(r_f["scores"][name][rev], scores0[name][rev]), name
    # every other row: the unforced run's, and moved
    assert _same_bits(p_f[keep_], p_t[keep_]) and _same_bits(hands_f.vertices[keep_], hands_t.vertices[keep_])
    assert _same_bits(hands_f.joints[keep_], hands_t.joints[keep_])
    for name in ("offset", "iter", "quat", "finger_quat", "curl", "rotation"):
        assert _same_bits(r_f[name][keep_], r_t[name][keep_]), name
    written = real(topo, hands_f.vertices, cloud)
    for name in ("penetration", "n_interior", "n_contact"):
        assert _same_bits(r_f["scores"][name], written[name]), f"{name}: the merged scores are not grasp_scores of the hands written"
    moved = (p_t[chosen.tolist()] != params[chosen.tolist()]).any(dim=1)
    assert moved.all(), "a chosen row had not moved: reverting it shows nothing"
    assert (hands_t.joints[chosen.tolist()] != first.joints[chosen.tolist()]).flatten(1).any(dim=1).all()
    assert (p_f[keep_] != params[keep_]).any() and (r_f["finger_quat"][keep_][..., 0] != 1).any()

    # through generate_for_objects, every row returned (no candidates): row o * M + g is grasp g of object o
    state["rows"], before = chosen.tolist(), state["calls"]
    got = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES, refine_steps=E2E_STEPS, refine_spin=1.0, refine_curl=1.0)
    assert state["calls"] == before + 1, "the hands written were scored a second time"
    for i, (g, p) in enumerate(zip(got, plain)):
        r = rev_f[i * M:(i + 1) * M]
        j = g["json"]
        assert g["refine_reverted"].cpu().numpy().tolist() == r.astype(int).tolist() == j["refine_reverted"]
        assert _same_bits(g["params"], p_f[i * M:(i + 1) * M]) and _same_bits(g["vertices"], hands_f.vertices[i * M:(i + 1) * M])
        rr = torch.from_numpy(r).to(DEV)
        assert _same_bits(g["params"][rr], p["params"][rr]) and _same_bits(g["vertices"][rr], p["vertices"][rr])
        for name in ("refine_offset", "refine_curl", "refine_rotation", "refine_iter"):
            assert not np.asarray(j[name])[r].any(), name
        assert np.array_equal(bits(np.asarray(j["recon_params"], np.float32)[:, 0]), bits(g["params"].cpu().numpy()))
        for name in ("penetration", "n_interior", "n_contact"):
            assert np.array_equal(np.asarray(j[name], written[name].cpu().numpy().dtype).view(np.uint32),
                                  written[name][i * M:(i + 1) * M].cpu().numpy().view(np.uint32)), name

    # with candidates: every candidate of object 1 comes out worse, so its kept rows are reverted ones, ranked by the generated hands
    state["rows"] = list(range(M, 2 * M))
    best = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, candidates=M, refine_steps=E2E_STEPS, refine_spin=1.0,
                                         refine_curl=1.0)
    g, p = best[1], plain[1]
    cand = g["candidate"]
    assert g["json"]["refine_reverted"] == [1] * k and _same_bits(g["params"], p["params"][cand]) and _same_bits(g["vertices"], p["vertices"][cand])
    order = ref.segment_topk(*(x[M:].cpu().numpy() for x in contact.select_keys(scores0, "penetration", 1)), 1, M, k)[0]
    assert cand.cpu().numpy().tolist() == order.tolist(), "the reverted rows are not ranked by the scores of the hands as generated"
    assert np.array_equal(bits(np.asarray(g["json"]["penetration"], np.float32)), bits(scores0["penetration"][M:][cand].cpu().numpy()))
    g0 = best[0]                                                                                 # object 0 was not forced
    c0 = g0["candidate"]
    assert g0["json"]["refine_reverted"] == rev_t[:M][c0.cpu().numpy()].astype(int).tolist()
    assert _same_bits(g0["params"], p_t[:M][c0]) and _same_bits(g0["vertices"], hands_t.vertices[:M][c0])


BASE = rigid_tests.BASE
_run_main = rigid_tests._run_main


@pytest.mark.gpu
def test_entry_point_files_without_curl_are_those_of_a_run_without_the_flag(tmp_path):
    mano = mano_pkl(tmp_path)
    steps = BASE + ["--candidates", "8", "--refine_steps", "3", "--refine_spin", "1"]
    names1, bytes1 = _run_main("ho3d", str(tmp_path / "steps"), steps, mano)
    names2, bytes2 = _run_main("ho3d", str(tmp_path / "steps0"), steps + ["--refine_curl", "0", "--refine_max_curl", "0.2"], mano)
    assert names1 == names2 and bytes1 == bytes2, "--refine_curl 0: the files differ"
    assert sorted(os.listdir(tmp_path / "steps")) == sorted(os.listdir(tmp_path / "steps0"))
    assert "refine_curl" not in json.loads(bytes1[0]) and "refine_rotation" in json.loads(bytes1[0])
    names0, bytes0 = _run_main("ho3d", str(tmp_path / "plain"), BASE, mano)
    names3, bytes3 = _run_main("ho3d", str(tmp_path / "zero"), BASE + ["--refine_curl", "0"], mano)
    assert names3 == names0 and bytes3 == bytes0, "--refine_curl 0 must write the files of a run without the flag"


@pytest.mark.gpu
def test_entry_point_files_with_curl_do_not_depend_on_rows_per_call(tmp_path):
    mano = mano_pkl(tmp_path)
    curl = BASE + ["--candidates", "8", "--refine_steps", "3", "--refine_curl", "1"]
    runs = [_run_main("ho3d", str(tmp_path / f"rows{r}"), curl + ["--rows_per_call", str(r)], mano) for r in (0, 5, 16384)]
    assert runs[0] == runs[1] == runs[2], "--rows_per_call 0, 5, 16384: the files differ"
    meta = [open(tmp_path / f"rows{r}" / "refine_curl.json", "rb").read() for r in (0, 5, 16384)]
    assert meta[0] == meta[1] == meta[2]
    m = json.loads(meta[0])
    assert m["joints"] == [1, 4, 7, 10, 13] and m["grasps"] == 8 and m["refine_curl"] == 1.0 and m["refine_max_curl"] == 0.35
    j = json.loads(runs[0][1][0])
    assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact",
                      "refine_offset", "refine_iter", "refine_curl", "refine_reverted"}      # no spin: no "refine_rotation"
    assert all(len(j[f]) == 4 for f in j) and all(len(g) == 5 and all(len(a) == 3 for a in g) for g in j["refine_curl"])
    assert all(isinstance(x, float) for g in j["refine_curl"] for a in g for x in a) and all(r in (0, 1) for r in j["refine_reverted"])
    _, loop = _run_main("ho3d", str(tmp_path / "loop"), BASE + ["--refine_steps", "3", "--refine_curl", "1", "--refine_spin", "1",
                                                                 "--rows_per_call", "0"], mano)
    assert set(json.loads(loop[0])) == {"recon_params", "R_list", "trans_list", "r_list", "refine_offset", "refine_iter", "refine_rotation",
                                        "refine_curl", "refine_reverted", "penetration", "n_interior", "n_contact"}
