"""Rigid push-out of generated grasps: the fused kernel (dvq_grasp_refine_rigid), its host API (ops.grasp_refine_rigid,
contact.refine_rigid, contact.apply_rigid, contact.compose_orient) and the ``refine_spin`` mode of generate_for_objects / the entry
points.  The reference is tests/grasp_refine_rigid_ref.py (numpy over oracle/contact_oracle.py and grasp_score_ref.tree_sum, all
fp32, one operation at a time); all six GPU outputs are compared with it bit for bit.  Nothing here says anything about real grasps:
no real checkpoint exists in the tree."""
import json
import lzma
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops, synth

import grasp_refine_ref as tref
import grasp_refine_rigid_ref as rref
import grasp_score_ref as ref
import mano_ref

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
THR = 0.02 ** 2
IDENTITY = np.asarray([1, 0, 0, 0], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mano_pkl(tmp_path):
    """tests/golden/g9_mano_right.pkl.xz unpacked: the path of a MANO_RIGHT.pkl (real topology: 778 vertices, 1538 faces)."""
    path = str(tmp_path / "MANO_RIGHT.pkl")
    if not os.path.exists(path):
        with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
    return path


def pinch():
    """The prototype's pinch: a bar-shaped hand with the pivot at one end, pinched by two small spheres on opposite sides at opposite
    ends -- no shift frees both, a small turn does."""
    v, f = ref.sphere_mesh()
    hand = (v * np.asarray([1.6, 0.5, 0.5], np.float32)).astype(np.float32)
    cloud = np.concatenate([tref.sphere_cloud(300, 0.03, (0.06, 0.04, 0)), tref.sphere_cloud(300, 0.03, (-0.04, -0.045, 0))])
    return hand, f, cloud, np.asarray([-0.08, 0, 0], np.float32)


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_spin_flag_and_the_abi_has_the_entry_point(dataset):
    a = generate.parse_args(dataset, [])
    assert a.refine_spin == 0.0
    a = generate.parse_args(dataset, ["--refine_steps", "6", "--refine_spin", "0.5"])
    assert (a.refine_steps, a.refine_spin) == (6, 0.5)
    for bad in (["--refine_steps", "3", "--refine_spin", "-0.1"], ["--refine_steps", "3", "--refine_spin", "inf"],
                ["--refine_steps", "3", "--refine_spin", "nan"], ["--refine_spin", "1"]):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_grasp_refine_rigid" in _lib.SIGNATURES and len(_lib.SIGNATURES["dvq_grasp_refine_rigid"][1]) == 25
    assert "int dvq_grasp_refine_rigid(" in header and hasattr(lib, "dvq_grasp_refine_rigid")
    added = re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert "dvq_grasp_refine_rigid" in added


def test_bad_arguments_are_refused_before_any_device_use():
    v, f = ref.sphere_mesh(4, 6)
    faces, off, vf = (torch.from_numpy(a) for a in contact.face_csr(f, len(v)))
    hand = torch.from_numpy(v)[None].contiguous()
    good = dict(hand=hand, faces=faces, vf_off=off, vf_face=vf, obj=torch.zeros(1, 5, 3), pivot=torch.zeros(1, 3), steps=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_refine_rigid(**good)                                               # well-formed, but not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_refine_rigid(**{**good, "steps": 0, "spin": 0.0})
    for bad in (dict(spin=-1.0), dict(spin=float("inf")), dict(spin=float("nan")), dict(pivot=torch.zeros(3)), dict(pivot=torch.zeros(2, 3)),
                dict(pivot=torch.zeros(1, 4)), dict(pivot=torch.zeros(1, 3, dtype=torch.float64)), dict(pivot=None), dict(steps=65),
                dict(push=-1.0), dict(pull=float("nan")), dict(obj=torch.zeros(1, 0, 3)), dict(hand=hand.double())):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_refine_rigid(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    for kw in (dict(refine_steps=2, refine_spin=-1.0), dict(refine_steps=2, refine_spin=float("inf")), dict(refine_spin=1.0)):
        with pytest.raises(RuntimeError, match="refine_spin"):
            generate.generate_for_objects(None, [torch.zeros(4, 8)], 5, True, 0, [0], **kw)


# ------------------------------------------------------------------------------------------------------ CPU: the reference itself
def test_reference_without_spin_is_the_translation_reference():
    v, f = ref.sphere_mesh()
    hand = np.stack([v, 0.9 * v]).astype(np.float32)
    obj = np.stack([tref.sphere_cloud(300), tref.sphere_cloud(300, centre=(0.0, 0.06, 0.01))])
    obj[1, 7, 1] = np.nan
    pivot = np.asarray([[-0.05, 0.0, 0.01], [0.0, -0.04, 0.0]], np.float32)
    for steps in (0, 6):
        got = rref.grasp_refine_rigid(hand, f, obj, pivot, steps, spin=0.0)
        want = tref.grasp_refine(hand, f, obj, steps)
        off, quat, it, pen, n_in, n_ct = got
        assert np.array_equal(bits(off), bits(want[0])) and np.array_equal(it, want[1])
        assert np.isnan(pen[1]) and np.isnan(want[2][1]) and bits(pen)[0] == bits(want[2])[0]
        assert np.array_equal(n_in, want[3]) and np.array_equal(n_ct, want[4])
        assert np.array_equal(bits(quat), bits(np.stack([IDENTITY] * 2)))
    assert it[0] > 0, "the six-step case does not move"
    scores = ref.grasp_scores(hand, f, obj)
    zero = rref.grasp_refine_rigid(hand, f, obj, pivot, 0)                           # with the spin on: steps = 0 is the score reference
    assert bits(zero[3])[0] == bits(scores[0])[0] and np.array_equal(zero[4], scores[1]) and np.array_equal(zero[5], scores[2])


def test_reference_hardly_turns_a_sphere_pushed_out_of_a_sphere():
    """A pull field that a shift satisfies turns nothing: tau is taken after the field's mean is removed, so it does not depend on the
    pivot, and for a sphere against a sphere it vanishes by symmetry up to the sampling of the two surfaces and fp32.  Measured with
    this reference: the kept iterate (7 of 8) is turned by 1.68e-3 rad and no iterate by more than 2.11e-3 rad, while the pinch below
    is turned by 4.0e-2 rad; the bound is four times the kept figure."""
    v, f = ref.sphere_mesh()
    traces = []
    pivot = np.asarray([[-0.03, 0.02, 0.01]], np.float32)                            # off-centre
    off, quat, it, pen, n_in, n_ct = rref.grasp_refine_rigid(v[None], f, tref.sphere_cloud()[None], pivot, 8, traces=traces)
    angle = float(rref.quat_angle(quat)[0])
    print("kept", int(it[0]), "pen", float(pen[0]), "angle", angle, "angles", [float(rref.quat_angle(x[1])) for x in traces[0]])
    assert it[0] > 0 and float(pen[0]) * 10 <= float(traces[0][0][3])                # it is pushed out all the same
    assert angle < 4 * 1.68e-3


def test_reference_frees_the_pinch_by_turning():
    hand, f, cloud, pivot = pinch()
    kept = {}
    for spin in (0.0, 1.0):
        traces = []
        off, quat, it, pen, n_in, n_ct = rref.grasp_refine_rigid(hand[None], f, cloud[None], pivot[None], 8, spin=spin, traces=traces)
        kept[spin] = float(pen[0])
        pen0 = float(traces[0][0][3])
        print("spin", spin, "kept", int(it[0]), "pen", kept[spin], "of", pen0, "angle (deg)", float(np.degrees(rref.quat_angle(quat)[0])))
        assert kept[spin] < pen0
        assert abs(np.linalg.norm(quat[0].astype(np.float64)) - 1.0) <= 1e-6
        assert (spin > 0) == bool(rref.quat_angle(quat)[0] > 0)
    assert kept[1.0] < kept[0.0]                                                     # the float64 prototype: 6.1e-4 against 9.4e-4


# ------------------------------------------------------------------------------------------------------ CPU: the rigid-motion helpers
RIGID_REF_ERR = 8.4e-9      # metres: the largest difference the float64 numpy restatement gives below (measured: 8.382e-9)


def test_apply_rigid_and_compose_orient_on_the_real_hand_model(tmp_path):
    """Turning the posed hand about its root joint and shifting it IS posing it with global_orient <- log(Q exp(global_orient)) and
    transl + t.  Both sides in float64 (tests/mano_ref.py on the real model).  The two do not agree to float64 rounding because the
    layer's Rodrigues formula takes the angle of ``r + 1e-8`` (not an exact exponential): the numpy restatement of the two helpers
    differs by RIGID_REF_ERR (1e-8 rad on a hand of 0.2 m and more), and the torch helpers may differ by four times that.  Against
    the numpy restatement itself the helpers are held to float64 rounding: 64 eps of 1 m and of pi rad (measured: 5.6e-17 m and
    4.4e-16 rad)."""
    from dvqvae_amd import mano as dmano
    arrays = mano_ref.device_arrays(dmano.read_mano_pkl(mano_pkl(tmp_path)))
    B = 24
    rnd = lambda tag, shape, scale: synth.synthetic_normal(shape, 77, f"rigid/helpers/{tag}", scale).numpy().astype(np.float64)
    betas, pose, go, tr = rnd("b", (B, 10), 1.0), rnd("p", (B, 45), 0.5), rnd("g", (B, 3), 1.2), rnd("t", (B, 3), 0.1)
    t = rnd("dt", (B, 3), 0.02)
    axis = rnd("ax", (B, 3), 1.0)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    angle = np.linspace(0.0, 3.0, B)                                                 # turns of up to 3 rad, the identity included
    angle[1] = 1e-9
    q = np.concatenate([np.cos(0.5 * angle)[:, None], np.sin(0.5 * angle)[:, None] * axis], 1)
    q[2::3] *= -1.0                                                                  # either sign is the same turn
    q[5] *= 1.0 + 3e-8                                                               # unit only to fp32 rounding, as the kernel's
    verts0, joints0 = mano_ref.mano_ref(arrays, betas, pose, go, tr)
    c = joints0[:, 0]
    want_ref = rref.apply_rigid64(verts0, c, t, q)
    posed_ref, _ = mano_ref.mano_ref(arrays, betas, pose, rref.compose_orient64(go, q), tr + t)
    err_ref = np.abs(posed_ref - want_ref).max()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    go_new = contact.compose_orient(T(go), T(q))
    assert go_new.dtype == torch.float64
    posed, _ = mano_ref.mano_ref(arrays, betas, pose, go_new.numpy(), tr + t)
    got = contact.apply_rigid(T(verts0), T(c), T(t), T(q))
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, 778, 3)
    err = np.abs(posed - got.numpy()).max()
    print(f"float64 reference: {err_ref:.3e} m; torch helpers: {err:.3e} m; against each other: apply "
          f"{np.abs(got.numpy() - want_ref).max():.3e} m, orient {np.abs(go_new.numpy() - rref.compose_orient64(go, q)).max():.3e} rad")
    assert err_ref <= RIGID_REF_ERR, "the recorded figure of the reference is stale"
    assert err <= 4 * RIGID_REF_ERR
    eps = np.finfo(np.float64).eps
    assert np.abs(got.numpy() - want_ref).max() <= 64 * eps and np.abs(go_new.numpy() - rref.compose_orient64(go, q)).max() <= 64 * eps * np.pi
    assert np.abs(np.linalg.norm(go_new.numpy(), axis=1)).max() <= np.pi + 1e-12     # w >= 0: the angle is at most pi
    # dtype, the identity and the batch
    go32 = T(go.astype(np.float32))
    ident = torch.from_numpy(np.stack([IDENTITY] * B))
    big = torch.tensor([[4.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1e-12, 0.0, -1e-12]], dtype=torch.float32)
    assert contact.compose_orient(go32, T(q)).dtype == torch.float32
    assert torch.equal(contact.compose_orient(go32, ident).view(torch.int32), go32.view(torch.int32))
    assert torch.equal(contact.compose_orient(big, ident[:3]).view(torch.int32), big.view(torch.int32))
    assert not contact.compose_orient(torch.zeros(1, 3), ident[:1]).view(torch.int32).any()
    assert not contact.quat_axis_angle(ident).view(torch.int64).any()                # exact zeros for the identity
    tiny = contact.compose_orient(torch.zeros(2, 3, dtype=torch.float64), T(np.asarray([[1.0, 1e-12, 0, 0], [1.0, 0, 0, 1e-200]])))
    assert torch.isfinite(tiny).all() and abs(float(tiny[0, 0]) - 2e-12) < 1e-24 and abs(float(tiny[1, 2]) - 2e-200) < 1e-210
    for b in (0, 7, B - 1):                                                          # a row alone gives the row's bits
        assert torch.equal(contact.compose_orient(T(go[b:b + 1]), T(q[b:b + 1])), go_new[b:b + 1])
        assert torch.equal(contact.apply_rigid(T(verts0[b:b + 1]), T(c[b:b + 1]), T(t[b:b + 1]), T(q[b:b + 1])), got[b:b + 1])
    back = contact.quat_axis_angle(contact.axis_angle_quat(T(go)))                   # the two conversions invert each other
    folded = rref.compose_orient64(go, np.stack([IDENTITY.astype(np.float64)] * B))
    assert np.abs(back.numpy() - folded).max() <= 1e-14


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def mano_faces(tmp_path):
    from dvqvae_amd import mano as dmano
    arrays = dmano.read_mano_pkl(mano_pkl(tmp_path))
    return arrays["faces"], np.asarray(arrays["v_template"], np.float32)


def five_situations():
    """tests/test_grasp_refine.py's five situations (moderate overlap, deep, touching, out of reach, a NaN coordinate) with a pivot per
    row on the far side of each hand."""
    v, f = ref.sphere_mesh()
    B, N = 5, 257
    scale = np.linspace(0.9, 1.1, B).astype(np.float32)[:, None, None]
    hand = (v[None] * scale + synth.synthetic_normal((B, len(v), 3), 41, "refine/five/h", 0.0005).numpy()).astype(np.float32)
    obj = np.stack([tref.sphere_cloud(N, 0.04, (0.07, 0.01, 0.0)), tref.sphere_cloud(N, 0.02, (0.015, 0.0, 0.005)),
                    tref.sphere_cloud(N, 0.04, (0.0, 0.0, 0.1)), tref.sphere_cloud(N, 0.04, (0.3, 0.0, 0.0)),
                    tref.sphere_cloud(N, 0.04, (0.0, 0.08, 0.01))])
    obj[4, 100, 2] = np.nan
    pivot = np.asarray([[-0.05, 0.01, 0.0], [-0.04, 0.0, 0.02], [0.0, 0.01, -0.05], [-0.06, 0.0, 0.0], [0.0, -0.05, 0.0]], np.float32)
    return hand, f, obj.astype(np.float32), pivot


def rigid_case(name, tmp_path):
    """(hand [B,V,3], faces, obj [B,N,3], pivot [B,3]) numpy fp32."""
    rng = lambda tag, shape, scale: synth.synthetic_normal(shape, 31, f"scores/{name}/{tag}", scale).numpy()
    piv = lambda shape, scale: synth.synthetic_normal(shape, 33, f"rigid/{name}/c", scale).numpy().astype(np.float32)
    if name == "1x1x1":                                                              # one vertex, one degenerate face; Q may be 0
        return rng("h", (1, 1, 3), 0.1), np.zeros((1, 3), np.int64), rng("o", (1, 1, 3), 0.1), piv((1, 3), 0.05)
    if name == "1x1x1_on_the_pivot":                                                 # the point 1 cm from the vertex, the pivot ON it: Q = 0
        h = rng("h", (1, 1, 3), 0.1)
        return h, np.zeros((1, 3), np.int64), (h + np.asarray([0.006, -0.008, 0.0], np.float32)).astype(np.float32), h[0].copy()
    if name == "3x300x776":                                                          # tests/test_grasp_refine.py's inputs, plus a pivot per row
        B, N = 3, 300
        v, f = ref.sphere_mesh()
        scale = np.linspace(0.8, 1.2, B).astype(np.float32)[:, None, None]
        hand = (v[None] * scale + rng("h", (B, len(v), 3), 0.002)).astype(np.float32)
        return hand, f, rng("o", (B, N, 3), 0.04), (np.asarray([[-0.05, 0.0, 0.0]], np.float32) + piv((B, 3), 0.01)).astype(np.float32)
    if name == "5x257x778":                                                          # the MANO template: V = 778 is no multiple of four
        f, v = mano_faces(tmp_path)
        B, N = 5, 257
        hand = (v[None] + rng("h", (B, 778, 3), 0.001)).astype(np.float32)
        centre = v.mean(0, keepdims=True)[None]
        obj = (centre + np.linspace(0.0, 0.03, B).astype(np.float32)[:, None, None] + rng("o", (B, N, 3), 0.025)).astype(np.float32)
        return hand, f, obj, (v[None, 0] + piv((B, 3), 0.01)).astype(np.float32)
    if name == "2x1030x5":                                                           # a square pyramid: V below one vector, two passes of points
        apex = np.asarray([[0.03, 0.03, -0.02], [-0.03, 0.03, -0.02], [-0.03, -0.03, -0.02], [0.03, -0.03, -0.02], [0.0, 0.0, 0.04]], np.float32)
        f = np.asarray([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [1, 0, 2], [2, 0, 3]], np.int64)
        hand = (apex[None] + rng("h", (2, 5, 3), 0.002)).astype(np.float32)
        return hand, f, rng("o", (2, 1030, 3), 0.03), (np.asarray([[0.0, 0.0, -0.03]], np.float32) + piv((2, 3), 0.005)).astype(np.float32)
    assert name == "5x257x776"
    return five_situations()


NAMES = ("offset", "quat", "iter", "penetration", "n_interior", "n_contact")


def run_rigid(hand, faces, obj_dev, pivot, steps, **kw):
    topo = contact.HandTopology(faces, hand.shape[1], DEV)
    out = contact.refine_rigid(topo, gpu(hand), obj_dev, gpu(pivot), steps, **kw)
    assert set(out) == set(NAMES)
    B = hand.shape[0]
    assert out["offset"].dtype == torch.float32 and tuple(out["offset"].shape) == (B, 3)
    assert out["quat"].dtype == torch.float32 and tuple(out["quat"].shape) == (B, 4)
    assert out["penetration"].dtype == torch.float32 and all(out[k].dtype == torch.int32 for k in ("iter", "n_interior", "n_contact"))
    return topo, {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal_bits(got, want, tag=""):
    """All six outputs bit for bit (a NaN is a NaN: its payload is nobody's contract)."""
    want = dict(zip(NAMES, want))
    print(tag, {k: got[k].tolist() for k in NAMES}, "reference", {k: want[k].tolist() for k in NAMES})
    for k in ("iter", "n_interior", "n_contact"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    nan = np.isnan(want["penetration"])
    assert np.array_equal(np.isnan(got["penetration"]), nan), tag
    assert np.array_equal(bits(got["penetration"])[~nan], bits(want["penetration"])[~nan]), (tag, got["penetration"], want["penetration"])
    assert np.array_equal(bits(got["offset"]), bits(want["offset"])), (tag, got["offset"], want["offset"])
    assert np.array_equal(bits(got["quat"]), bits(want["quat"])), (tag, got["quat"], want["quat"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,steps", [("1x1x1", 3), ("1x1x1_on_the_pivot", 3), ("3x300x776", 0), ("3x300x776", 1), ("3x300x776", 6), ("5x257x778", 5),
                                        ("2x1030x5", 4), ("5x257x776", 5)])
def test_grasp_refine_rigid_equals_the_reference_bit_for_bit(name, steps, tmp_path):
    hand, faces, obj, pivot = rigid_case(name, tmp_path)
    _, got = run_rigid(hand, faces, gpu(obj), pivot, steps)
    traces = []
    want = rref.grasp_refine_rigid(hand, faces, obj, pivot, steps, traces=traces)
    assert_equal_bits(got, want, f"{name} steps {steps}")
    turned = [any(not np.array_equal(x[1], IDENTITY) for x in tr) for tr in traces]
    if steps == 0:
        assert not got["iter"].any() and not bits(got["offset"]).any() and np.array_equal(got["quat"], np.stack([IDENTITY] * len(hand)))
    elif name == "1x1x1_on_the_pivot":
        assert len(traces[0]) == steps + 1 and traces[0][1][0].any() and not any(turned)   # pulled closer, and Q = 0 turns nothing
    elif name != "1x1x1":
        assert any(turned), "no iterate of the case is turned: the rotation is not exercised"
    if steps > 1 and not name.startswith("1x1x1"):
        assert (want[2] > 1).any(), "no kept iterate comes after a turn"
    if name == "5x257x776":
        off, quat, it, pen, n_in, n_ct = want
        assert it[0] > 0 and it[3] == 0 and n_ct[3] == 0 and not bits(off[3]).any()                 # out of reach: untouched
        assert np.isnan(pen[4]) and it[4] == 0 and not bits(off[4]).any() and np.array_equal(quat[4], IDENTITY)   # the NaN row


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["nan_in_the_hand", "inf_in_the_cloud"])
def test_grasp_refine_rigid_ends_on_a_coordinate_that_is_not_finite(what):
    """A NaN coordinate of the hand makes every distance of the grasp NaN: iterate 0 is of class 2 and is the only one.  An Inf in the
    cloud is a point at infinity: where it counts as interior its pull is infinite, the state leaves the finite numbers with the first
    step and the next iterate is of class 2, which ends the loop and never replaces the iterate kept."""
    hand, f, cloud, pivot = pinch()
    hand, cloud = hand.copy(), cloud.copy()
    steps = 6
    if what == "nan_in_the_hand":
        hand[300, 1] = np.nan
    else:
        from oracle import contact_oracle
        n0 = contact_oracle.vertex_normals(hand[None], f)[0, 0]                      # the scan gives a point at infinity vertex 0
        axis = int(np.argmax(np.abs(n0)))
        cloud[17, axis] = -np.inf if n0[axis] > 0 else np.inf                        # (hand[0] - p) . n0 = +inf: interior
    traces = []
    want = rref.grasp_refine_rigid(hand[None], f, cloud[None], pivot[None], steps, traces=traces)
    _, got = run_rigid(hand[None], f, gpu(cloud[None]), pivot[None], steps)
    assert_equal_bits(got, want, what)
    trace = traces[0]
    assert trace[-1][2] == 2 and len(trace) <= 2 < steps + 1, "the loop did not end on the iterate of class 2"
    assert got["iter"][0] == 0 and not bits(got["offset"]).any() and np.array_equal(got["quat"][0], IDENTITY)
    assert np.isnan(got["penetration"][0]) == (what == "nan_in_the_hand")


@pytest.mark.gpu
def test_grasp_refine_rigid_without_spin_gives_the_bits_of_the_translation_kernel(tmp_path):
    for name, steps in (("5x257x776", 5), ("5x257x778", 4)):
        hand, faces, obj, pivot = rigid_case(name, tmp_path)
        topo, got = run_rigid(hand, faces, gpu(obj), pivot, steps, spin=0.0)
        want = contact.refine_translation(topo, gpu(hand), gpu(obj), steps)
        for k in ("offset", "iter", "penetration", "n_interior", "n_contact"):
            w = want[k].cpu().numpy()
            real = ~np.isnan(w) if k == "penetration" else np.ones(len(w), bool)     # a NaN is a NaN, whatever its payload
            assert np.array_equal(got[k][real].view(np.uint32), w[real].view(np.uint32)), (name, k)
        assert np.array_equal(np.isnan(got["penetration"]), torch.isnan(want["penetration"]).cpu().numpy())
        assert np.isnan(got["penetration"]).sum() == (1 if name == "5x257x776" else 0)
        assert np.array_equal(bits(got["quat"]), bits(np.stack([IDENTITY] * len(hand))))
        assert (got["iter"] > 0).any()


@pytest.mark.gpu
def test_grasp_refine_rigid_of_a_row_does_not_depend_on_the_batch():
    hand, faces, obj, pivot = five_situations()
    topo = contact.HandTopology(faces, hand.shape[1], DEV)
    pick = torch.arange(300, device=DEV) % 5
    big = contact.refine_rigid(topo, gpu(hand)[pick].contiguous(), gpu(obj)[pick].contiguous(), gpu(pivot)[pick].contiguous(), 5)
    for b in range(5):
        one = contact.refine_rigid(topo, gpu(hand[b:b + 1]), gpu(obj[b:b + 1]), gpu(pivot[b:b + 1]), 5)
        for k in NAMES:
            rows = big[k][pick == b].cpu().numpy()
            alone = one[k].cpu().numpy()
            assert np.array_equal(rows.view(np.uint32), np.repeat(alone, rows.shape[0], axis=0).view(np.uint32)), (k, b)
    assert (big["iter"] > 0).any() and (big["iter"] == 0).any()
    assert (big["quat"][:, 0] != 1).any(), "no kept iterate is turned"
    empty = contact.refine_rigid(topo, gpu(hand)[:0].contiguous(), gpu(obj)[:0].contiguous(), gpu(pivot)[:0].contiguous(), 5)
    assert tuple(empty["offset"].shape) == (0, 3) and tuple(empty["quat"].shape) == (0, 4)
    assert all(empty[k].shape == (0,) for k in NAMES[2:])


@pytest.mark.gpu
def test_grasp_refine_rigid_reads_a_channel_first_view_in_place():
    v, f = ref.sphere_mesh()
    B, N = 3, 500
    cloud = synth.synthetic_normal((B, 4, N), 32, "refine/cf", 0.02)                    # [B,4,N] as the generation path holds it
    cloud[:, 0] += 0.06                                                                  # across the hand's surface on the +x side
    hand = (v[None] * np.asarray([1.0, 0.9, 1.1], np.float32)[:, None, None]).astype(np.float32)
    pivot = np.asarray([[-0.05, 0.0, 0.0], [-0.04, 0.01, 0.0], [-0.05, 0.0, 0.02]], np.float32)
    view = gpu(cloud)[:, :3].transpose(1, 2)                                             # strides (4N, 1, N)
    assert not view.is_contiguous()
    _, got = run_rigid(hand, f, view, pivot, 4)
    obj = cloud[:, :3].transpose(1, 2).contiguous().numpy()
    _, copy = run_rigid(hand, f, gpu(obj), pivot, 4)
    for k in NAMES:
        assert np.array_equal(got[k].view(np.uint32), copy[k].view(np.uint32)), k
    assert_equal_bits(got, rref.grasp_refine_rigid(hand, f, obj, pivot, 4), "channel-first")
    assert (got["iter"] > 0).any() and (got["quat"][:, 0] != 1).any()


@pytest.mark.gpu
def test_grasp_refine_rigid_with_no_steps_gives_the_bits_of_grasp_scores(tmp_path):
    for name in ("5x257x776", "5x257x778"):
        hand, faces, obj, pivot = rigid_case(name, tmp_path)
        topo, got = run_rigid(hand, faces, gpu(obj), pivot, 0)
        want = contact.grasp_scores(topo, gpu(hand), gpu(obj))
        pen = want["penetration"].cpu().numpy()
        nan = np.isnan(got["penetration"])
        assert np.array_equal(nan, np.isnan(pen))
        assert np.array_equal(bits(got["penetration"])[~nan], bits(pen)[~nan])
        assert np.array_equal(got["n_interior"], want["n_interior"].cpu().numpy())
        assert np.array_equal(got["n_contact"], want["n_contact"].cpu().numpy())
        assert not got["iter"].any() and not bits(got["offset"]).any() and np.array_equal(got["quat"], np.stack([IDENTITY] * len(hand)))


@pytest.mark.gpu
def test_grasp_refine_rigid_refuses_what_the_kernel_cannot_hold():
    v, f = ref.sphere_mesh(4, 6)
    topo = contact.HandTopology(f, len(v), DEV)
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL, nothing launched
    one = torch.zeros(8, device=DEV)
    ok = dict(V=5, N=4, B=1, steps=2, push=1.0, pull=0.25, spin=1.0, pivot=one.data_ptr(), quat=one.data_ptr())
    for bad in (dict(V=2049), dict(V=0), dict(N=0), dict(B=-1), dict(steps=-1), dict(steps=65), dict(spin=-1.0), dict(spin=float("inf")),
                dict(spin=float("nan")), dict(push=-1.0), dict(pivot=None), dict(quat=None)):
        a = {**ok, **bad}
        rc = lib.dvq_grasp_refine_rigid(one.data_ptr(), topo.faces.data_ptr(), topo.vf_off.data_ptr(), topo.vf_face.data_ptr(), a["V"],
                                        one.data_ptr(), 0, 3, 1, a["B"], a["N"], a["pivot"], 0.0004, a["steps"], a["push"], a["pull"],
                                        a["spin"], 1, one.data_ptr(), a["quat"], one.data_ptr(), one.data_ptr(), one.data_ptr(),
                                        one.data_ptr(), None)
        assert rc == 1, bad
    torch.cuda.synchronize()
    assert not one.any(), "a refused call wrote something"


# ------------------------------------------------------------------------------------------------------ GPU: end to end
def _gennet(tmp_path):
    """The synthetic net of tests/test_generate_batched.py with the REAL MANO model of the fixture (the scores need its faces)."""
    from conftest import GOLDEN, gen_state_dict
    from dvqvae_amd import mano as dmano
    from dvqvae_amd.network.gen_net import GenNet
    net = GenNet()
    net.load_state_dict(gen_state_dict(net.state_dict(), np.load(os.path.join(GOLDEN, "g7_gen.npz"))), strict=True)
    net.eval().to(DEV)
    net.set_rh_mano(dmano.load(model_path=mano_pkl(tmp_path), model_type="mano", use_pca=True, num_pca_comps=45,
                               flat_hand_mean=True).to(DEV))
    return net


E2E_SEED, E2E_M, E2E_K, E2E_STEPS = 9, 8, 4, 3
E2E_INDICES = [5, 2]


def e2e_objects():
    """tests/test_grasp_refine.py's two clouds of 256 points around the place the synthetic weights put every hand."""
    centre = np.asarray([-0.08, -0.09, 0.13])
    return [generate.object_tensor(synth.synthetic_uniform((256, 3), 70 + i, "select/e2e", -0.1, 0.1).numpy().astype(np.float64) + centre)
            for i in range(2)]


def _mano(net, params):
    return net.rh_mano(betas=params[:, :10], global_orient=params[:, 10:13], hand_pose=params[:, 13:58], transl=params[:, 58:61])


def _mano64(arrays, params):
    p = params.cpu().numpy().astype(np.float64)
    return mano_ref.mano_ref(arrays, p[:, :10], p[:, 13:58], p[:, 10:13], p[:, 58:61])[0]


@pytest.mark.gpu
def test_rigidly_refined_best_of_m_end_to_end(tmp_path):
    """The hands written are the unrefined hands moved by the reported offset and rotation about their root joints.  Both sides carry
    the fp32 error of the MANO layer (one pose each); the tolerance is four times the largest difference between the layer and its
    float64 restatement on the parameters of this test."""
    from dvqvae_amd import mano as dmano
    net = _gennet(tmp_path)
    arrays = mano_ref.device_arrays(dmano.read_mano_pkl(mano_pkl(tmp_path)))
    objs, M, k = e2e_objects(), E2E_M, E2E_K
    plain = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES)            # all M rows, unrefined
    topo = contact.HandTopology(np.asarray(net.rh_mano.faces), 778, DEV)
    first, turned, worst, layer = None, False, 0.0, 0.0
    for rows_per_call in (16384, 8):
        got = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, rows_per_call=rows_per_call, candidates=M,
                                            refine_steps=E2E_STEPS, refine_spin=1.0)
        for i, (g, p) in enumerate(zip(got, plain)):
            cand, j = g["candidate"], g["json"]
            old = p["params"][cand].contiguous()
            assert tuple(g["params"].shape) == (k, 61) and tuple(g["refine_offset"].shape) == (k, 3) and tuple(g["refine_iter"].shape) == (k,)
            assert tuple(g["refine_rotation"].shape) == (k, 3) and g["refine_rotation"].dtype == torch.float64
            assert torch.equal(g["params"][:, :10], old[:, :10]) and torch.equal(g["params"][:, 13:58], old[:, 13:58])
            assert torch.equal(g["params"][:, 58:61], old[:, 58:61] + g["refine_offset"]), f"object {i}: translation"
            quat = contact.axis_angle_quat(g["refine_rotation"])
            assert torch.allclose(g["params"][:, 10:13].double(), contact.compose_orient(old[:, 10:13].double(), quat), rtol=0, atol=1e-6)
            new = _mano(net, g["params"].contiguous())
            assert torch.equal(new.vertices, g["vertices"]), f"object {i}: the vertices are not those of the parameters written"
            before = _mano(net, old)
            assert torch.equal(before.vertices, p["vertices"][cand])
            want = contact.apply_rigid(before.vertices, before.joints[:, 0], g["refine_offset"], quat)
            diff = float((want.double() - g["vertices"].double()).abs().max())
            err = max(float(np.abs(before.vertices.cpu().numpy() - _mano64(arrays, old)).max()),
                      float(np.abs(g["vertices"].cpu().numpy() - _mano64(arrays, g["params"])).max()))
            worst, layer = max(worst, diff), max(layer, err)
            written = np.asarray(j["recon_params"], np.float32)[:, 0]
            assert np.array_equal(bits(written), bits(g["params"].cpu().numpy()))
            assert np.array_equal(bits(np.asarray(j["refine_offset"], np.float32)), bits(g["refine_offset"].cpu().numpy()))
            assert j["refine_rotation"] == g["refine_rotation"].cpu().numpy().tolist()
            assert j["refine_iter"] == g["refine_iter"].cpu().numpy().tolist() and all(0 <= x <= E2E_STEPS for x in j["refine_iter"])
            R = np.asarray(j["R_list"], np.float64)                                      # [k,3,4]: rotation | translation
            cloud = ops.transform_cloud(gpu(objs[i]).contiguous(), gpu(R[:, :, :3].astype(np.float32)).contiguous(),
                                        gpu(R[0, :, 3].astype(np.float32)).contiguous())[:, :3].transpose(1, 2)
            scores = contact.grasp_scores(topo, g["vertices"], cloud)
            pen = scores["penetration"].cpu().numpy()
            assert np.array_equal(bits(np.asarray(j["penetration"], np.float32)), bits(pen)), f"object {i}: JSON penetration"
            assert j["n_interior"] == scores["n_interior"].cpu().numpy().tolist()
            assert j["n_contact"] == scores["n_contact"].cpu().numpy().tolist()
            assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact",
                              "refine_offset", "refine_iter", "refine_rotation"}
            print(f"rows_per_call {rows_per_call} object {i}: kept {cand.tolist()} iter {j['refine_iter']} rotation {j['refine_rotation']} "
                  f"pen {j['penetration']}; written against apply_rigid {diff:.3e} m, the layer against float64 {err:.3e} m")
            turned |= any(any(x != 0 for x in r) for r in j["refine_rotation"])
        dumped = [json.dumps(g["json"]) for g in got]
        if first is None:
            first = dumped
        assert dumped == first, f"rows_per_call {rows_per_call}: the JSON differs from the 16384-row call's"
    print(f"largest difference {worst:.3e} m; the MANO layer against float64 {layer:.3e} m; allowed {4 * layer:.3e} m")
    assert turned, "no grasp was turned: the rotation is not exercised"
    assert worst <= 4 * layer


def _run_main(dataset, out_dir, extra, mano="/nonexistent"):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


BASE = ["--num_objects", "2", "--points", "256", "--num_grasp", "4"]


@pytest.mark.gpu
def test_entry_point_files_without_spin_are_those_of_a_run_without_the_flag(tmp_path):
    mano = mano_pkl(tmp_path)
    names0, bytes0 = _run_main("ho3d", str(tmp_path / "plain"), BASE, mano)
    names, data = _run_main("ho3d", str(tmp_path / "zero"), BASE + ["--refine_spin", "0"], mano)
    assert names == names0 and data == bytes0, "--refine_spin 0 must write the files of a run without the flag"
    steps = BASE + ["--candidates", "8", "--refine_steps", "3"]
    names1, bytes1 = _run_main("ho3d", str(tmp_path / "steps"), steps, mano)
    names2, bytes2 = _run_main("ho3d", str(tmp_path / "steps0"), steps + ["--refine_spin", "0"], mano)
    assert names1 == names0 and names2 == names0 and bytes1 == bytes2, "--refine_steps 3 --refine_spin 0: the files differ"
    assert "refine_rotation" not in json.loads(bytes1[0]) and "refine_offset" in json.loads(bytes1[0])


@pytest.mark.gpu
def test_entry_point_files_with_spin_do_not_depend_on_rows_per_call(tmp_path):
    mano = mano_pkl(tmp_path)
    spin = BASE + ["--candidates", "8", "--refine_steps", "3", "--refine_spin", "1"]
    runs = [_run_main("ho3d", str(tmp_path / f"rows{r}"), spin + ["--rows_per_call", str(r)], mano) for r in (0, 5, 16384)]
    assert runs[0] == runs[1] == runs[2], "--rows_per_call 0, 5, 16384: the files differ"
    j = json.loads(runs[0][1][0])
    assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact",
                      "refine_offset", "refine_iter", "refine_rotation"}
    assert all(len(j[f]) == 4 for f in j) and all(len(o) == 3 for o in j["refine_rotation"])
    assert all(isinstance(x, float) for o in j["refine_rotation"] for x in o)        # (the end-to-end test above turns hands; these clouds
                                                                                     # need not touch theirs)
    _, loop = _run_main("ho3d", str(tmp_path / "loop"), BASE + ["--refine_steps", "3", "--refine_spin", "1", "--rows_per_call", "0"], mano)
    assert set(json.loads(loop[0])) == {"recon_params", "R_list", "trans_list", "r_list", "refine_offset", "refine_iter", "refine_rotation",
                                        "penetration", "n_interior", "n_contact"}
