"""Force-closure quality with friction: the fused kernel (dvq_grasp_closure), its host API (ops.grasp_closure, contact.grasp_closure,
contact.closure_directions, contact.closure_stats, contact.closure_class) and the ``--closure`` / ``--min_closure`` mode of the entry
points.  The reference is tests/grasp_closure_ref.py (numpy over oracle/contact_oracle.py, the canonical reduction of
tests/grasp_score_ref.py); GPU results are compared with it bit for bit."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops, synth

import grasp_closure_ref as ref
import grasp_score_ref as score_ref

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
LENGTH, THR = 0.1, 0.02 ** 2
FIELDS = ("closure_quality", "force_closure", "closure_direction")
OUTPUTS = ("quality", "worst_dir", "status", "n_contact", "centre")
MUS, DS = (0.0, 0.5), (12, 13, 256, 1024)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_closure_flags(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.closure, a.friction, a.closure_dirs, a.min_closure) == (0, 0.5, 256, -INF)
    a = generate.parse_args(dataset, ["--closure", "1", "--friction", "0.8", "--closure_dirs", "64", "--min_closure", "-0.25", "--candidates", "200",
                                      "--num_grasp", "100", "--torque_length", "0.05"])
    assert (a.closure, a.friction, a.closure_dirs, a.min_closure, a.torque_length) == (1, 0.8, 64, -0.25, 0.05)
    assert generate.parse_args(dataset, ["--min_closure", "0", "--candidates", "8", "--num_grasp", "4", "--friction", "0"]).friction == 0.0
    for bad in (["--closure", "2"], ["--closure", "1", "--friction", "-0.1"], ["--closure", "1", "--friction", "inf"],
                ["--closure", "1", "--friction", "nan"], ["--closure", "1", "--closure_dirs", "11"], ["--closure", "1", "--closure_dirs", "1025"],
                ["--min_closure", "nan", "--candidates", "8", "--num_grasp", "4"], ["--min_closure", "0.1"],      # a guard needs candidates
                ["--friction", "0.3"], ["--closure_dirs", "64"], ["--closure", "1", "--torque_length", "0"]):       # settings need the figure
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    assert re.search(r"^#define DVQ_GRASP_CLOSURE_MAX_DIRS 1024$", header, re.M) and ops.GRASP_CLOSURE_MAX_DIRS == 1024
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_grasp_closure" in _lib.SIGNATURES and "int dvq_grasp_closure(" in header and hasattr(lib, "dvq_grasp_closure")
    assert "dvq_grasp_closure" in re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert len(_lib.SIGNATURES["dvq_grasp_closure"][1]) == 23                         # dvq_grasp_wrench's first 13 + mu, dirs, D + six outputs + stream


def test_ops_refuse_bad_arguments_before_any_device_use():
    v, f = score_ref.sphere_mesh(4, 6)
    faces, off, vf = (torch.from_numpy(a) for a in contact.face_csr(f, len(v)))
    hand = torch.from_numpy(v)[None].contiguous()
    obj = torch.zeros(1, 5, 3)
    dirs = torch.from_numpy(contact.closure_directions(16).copy())
    good = dict(hand=hand, faces=faces, vf_off=off, vf_face=vf, obj=obj, inv_length=10.0, mu=0.5, dirs=dirs)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_closure(**good)                                                    # well-formed, but not on a device
    for bad in (dict(hand=torch.zeros(1, 2049, 3), vf_off=torch.zeros(2050, dtype=torch.int32)),     # V > 2048
                dict(obj=torch.zeros(1, 0, 3)),                                                      # N = 0
                dict(hand=hand.transpose(1, 2)), dict(hand=hand.expand(2, -1, -1), obj=torch.zeros(2, 5, 3)),   # not contiguous
                dict(hand=hand.double()), dict(obj=obj.double()), dict(faces=faces.long()),                     # wrong dtype
                dict(hand=torch.zeros(1, 0, 3), vf_off=off[:1]), dict(vf_off=off[:-1]), dict(obj=torch.zeros(2, 5, 3)),
                dict(inv_length=0.0), dict(inv_length=INF), dict(inv_length=NAN),
                dict(mu=-0.1), dict(mu=INF), dict(mu=NAN),
                dict(dirs=torch.zeros(0, 6)), dict(dirs=torch.zeros(1025, 6)), dict(dirs=torch.zeros(16, 5)), dict(dirs=dirs.double()),
                dict(dirs=torch.zeros(6, 16).t()), dict(dirs=dirs.numpy())):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_closure(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    topo = type("T", (), dict(faces=faces, vf_off=off, vf_face=vf))
    for length in (0.0, -0.1, INF, NAN):
        with pytest.raises(RuntimeError, match="length"):
            contact.grasp_closure(topo, hand, obj, length=length)
    for friction in (-0.1, INF, NAN):
        with pytest.raises(RuntimeError, match="friction"):
            contact.grasp_closure(topo, hand, obj, friction=friction)
    for D in (0, 1025):
        with pytest.raises(RuntimeError, match="1 <= D <= 1024"):
            contact.grasp_closure(topo, hand, obj, dirs=D)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        contact.grasp_closure(topo, hand, obj)


# ------------------------------------------------------------------------------------------------------ CPU: the direction table
def test_direction_table():
    full = contact.closure_directions(1024)
    assert full.dtype == np.float32 and full.shape == (1024, 6)
    axes = np.zeros((12, 6), np.float32)
    for a in range(6):
        axes[2 * a, a], axes[2 * a + 1, a] = 1.0, -1.0
    assert np.array_equal(full[:12], axes)                                           # +e_0, -e_0, ..., -e_5
    assert np.array_equal(full[1::2], -full[0::2])                                   # row 2m + 1 = -row 2m
    norm = np.sqrt((full.astype(np.float64) ** 2).sum(axis=1))
    assert np.abs(norm - 1.0).max() <= 2.0 ** -23, np.abs(norm - 1.0).max()
    assert len({row.tobytes() for row in full}) == 1024                              # no direction twice
    for D in (1, 12, 13, 256):
        t = contact.closure_directions(D)
        assert t.shape == (D, 6) and t.tobytes() == full[:D].tobytes()               # a shorter table is the head of a longer one
    odd = contact.closure_directions(13)
    assert np.array_equal(odd[12], full[12]) and not np.array_equal(odd[12], -odd[11])   # D = 13 cuts a pair: u without its -u
    assert contact.closure_directions(256).tobytes() == contact.closure_directions(256).tobytes()
    contact._CLOSURE_TABLES.clear()                                                  # and made again from nothing: the same bytes
    assert contact.closure_directions(1024).tobytes() == full.tobytes()
    assert full.tobytes() == ref.directions(1024).tobytes() and ref.directions(13).tobytes() == odd.tobytes()
    # the Halton rows are spread: the largest gap, the angle from any axis to its nearest row, is far below a right angle
    assert (full[12:] @ axes.T).max(axis=0).min() > 0.8
    for D in (0, 1025, -3):
        with pytest.raises(RuntimeError):
            contact.closure_directions(D)


# ------------------------------------------------------------------------------------------------------ CPU: analytic, contacts given
def close(a, b, scale=None):
    return abs(a - b) <= 1e-12 * (abs(b) if scale is None else scale)


def test_support64_on_contacts_given():
    R, L = 0.06, LENGTH
    p = R * ref.unit_directions(400, 1)                                              # contact points on a sphere about the origin
    n, r = p / R, p / L                                                              # radial normals: n_i = r_i * L / R
    dirs = np.zeros((14, 6))
    dirs[:12] = ref.directions(12)
    dirs[12, 3:] = np.asarray([1.0, 2.0, -2.0]) / 3.0                                # a torque axis that is no coordinate axis
    dirs[13, :3] = np.asarray([2.0, -1.0, 2.0]) / 3.0
    for mu in (0.0, 0.5, 1.3):
        h = ref.support64(n, r, dirs, mu)
        # a pure torque u = (0, e): a = e x r is normal to r and so to n, hence s = n . a = 0 and |n x a| = |a|: h = mu * max |e x r|
        for k in (6, 7, 8, 9, 10, 11, 12):
            e = dirs[k, 3:]
            assert close(h[k], mu * np.linalg.norm(np.cross(e, r), axis=1).max(), scale=np.linalg.norm(r, axis=1).max()), (mu, k, h[k])
        # a pure force u = (e, 0): a = e, s = n . e and |n x e| = sqrt(1 - (n . e)^2) for unit n and e
        for k in (0, 1, 2, 3, 4, 5, 13):
            ne = n @ dirs[k, :3]
            assert close(h[k], (ne + mu * np.sqrt(1.0 - ne * ne)).max()), (mu, k, h[k])
    assert np.abs(ref.support64(n, r, dirs[6:13], 0.0)).max() <= 1e-12 * R / L      # frictionless sphere: no torque is resisted
    # a one-sided set: n_z > mu / sqrt(1 + mu^2) for every contact  <=>  n_z^2 (1 + mu^2) > mu^2  <=>  n_z > mu sqrt(1 - n_z^2), so
    # every term of h(-e_z) = max(-n_z + mu sqrt(1 - n_z^2)) is negative: the cones cannot push along -z, no force closure
    for mu in (0.0, 0.5, 1.3):
        side = n[:, 2] > mu / math.sqrt(1.0 + mu * mu) + 1e-3
        assert 10 < side.sum() < 400
        h = ref.support64(n[side], r[side], dirs[:12], mu)
        nz = n[side, 2]
        assert h[5] < 0.0 and close(h[5], (-nz + mu * np.sqrt(1.0 - nz * nz)).max())
        assert ref.quality(h)[0] <= h[5] < 0.0
    # the issue's float64 figures with radial normals: the whole shell at mu = 0.5 is mu R / L at a torque axis, the cap's rim closes the form
    dirs = ref.directions(256).astype(np.float64)
    q, k = ref.quality(ref.support64(n, r, dirs, 0.5))
    assert k >= 6 and abs(q - 0.5 * R / L) < 2e-3, (q, k)                            # (400 points: the largest |e x r| is just below R / L)
    cap = n[:, 2] > 0.8
    for mu in (0.0, 0.5):
        q, k = ref.quality(ref.support64(n[cap], r[cap], dirs, mu))
        rim = n[cap, 2].min()
        assert k == 5 and close(q, -rim + mu * math.sqrt(1.0 - rim * rim)), (mu, q, k)


# ------------------------------------------------------------------------------------------------------ CPU: the reference itself
@pytest.fixture(scope="module")
def sphere_cases():
    """The closed sphere of radius 0.05 as the hand against 1000 points at radius 0.06 -- all of them, the cap z > 0.8, and the shell
    1 m away (tests/test_grasp_wrench.py's clouds) -- over 256 directions at mu = 0, 0.25, 0.5 and 1.  Computed once."""
    v, f = score_ref.sphere_mesh()
    pts = ref.unit_directions(1000, 0)
    shell = (0.06 * pts).astype(np.float32)
    clouds = {"shell": shell, "cap": shell[pts[:, 2] > 0.8], "far": (shell + np.float32(1.0)).astype(np.float32)}
    dirs = contact.closure_directions(256)
    return {(k, mu): ref.grasp_closure(v[None], f, o[None], 1.0 / LENGTH, mu, dirs, THR) for k, o in clouds.items() for mu in (0.0, 0.25, 0.5, 1.0)}


def test_reference_on_the_closed_sphere(sphere_cases):
    print({key: (float(r["quality"][0]), int(r["worst_dir"][0]), int(r["status"][0]), int(r["n_contact"][0])) for key, r in sphere_cases.items()})
    for mu in (0.0, 0.25, 0.5, 1.0):
        shell, cap, far = (sphere_cases[(k, mu)] for k in ("shell", "cap", "far"))
        assert shell["n_contact"].tolist() == [1000] and cap["n_contact"].tolist() == [96] and far["n_contact"].tolist() == [0]
        assert shell["status"].tolist() == [0] and cap["status"].tolist() == [0]
        assert far["status"].tolist() == [1] and far["quality"][0] == -INF and far["worst_dir"].tolist() == [-1] and np.isneginf(far["support"]).all()
        assert shell["quality"][0] > cap["quality"][0]                               # the enclosing hand is the better one at every mu
        assert shell["support"][0, shell["worst_dir"][0]] == shell["quality"][0] and (shell["support"][0] >= shell["quality"][0]).all()
    assert sphere_cases[("shell", 0.5)]["quality"][0] > 0.0                          # contacts all round, with friction: not refuted
    assert sphere_cases[("cap", 0.0)]["quality"][0] < 0.0 and sphere_cases[("cap", 0.5)]["quality"][0] < 0.0    # one side: certified open
    for k in ("shell", "cap"):                                                       # more friction never lowers a support
        q = [sphere_cases[(k, mu)]["quality"][0] for mu in (0.0, 0.25, 0.5, 1.0)]
        assert q == sorted(q), (k, q)
        for lo, hi in ((0.0, 0.25), (0.25, 0.5), (0.5, 1.0)):
            assert (sphere_cases[(k, hi)]["support"] >= sphere_cases[(k, lo)]["support"]).all()


def test_fp32_restatement_against_float64_on_the_same_contacts(sphere_cases):
    """|quality32 - quality64| <= 32 * 2^-24 * (1 + mu) * (1 + max|r|) on the SAME fp32 n, r and contact set.  One (contact, direction)
    pair's h goes through at most 16 roundings -- a: 2 products, a difference, a sum; s: 3; c: 2 products and a difference; dot(c, c): 3,
    the square root, the last fma -- each of relative size 2^-24 on a quantity bounded by (1 + mu) * |a| with |a| <= |uf| + |ut| |r| <=
    1 + |r| (n and u are unit to rounding; the roundings of a pass to s and to |c| with factors <= 1 and mu); first order, doubled.  Max
    over contacts and min over directions are 1-Lipschitz in the sup norm, so the pair bound carries to the quality."""
    worst = 0.0
    cases = []
    rng = np.random.default_rng(7)
    for C, scale, mu in ((1, 0.3, 0.0), (50, 0.6, 0.5), (200, 1.5, 1.0), (37, 3.0, 0.25), (500, 0.6, 2.0)):
        n = rng.normal(size=(C, 3))
        n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
        cases.append((f"random C={C}", n, (scale * rng.normal(size=(C, 3))).astype(np.float32), mu))
    for (k, mu), r in sphere_cases.items():
        if k != "far":
            c = r["contact"][0]
            cases.append((f"{k} mu={mu}", r["n"][0][c], r["r"][0][c], mu))
    dirs = contact.closure_directions(256)
    for name, n, r, mu in cases:
        s32 = ref.support32(n, r, dirs, mu)
        s64 = ref.support64(n, r, dirs, float(np.float32(mu)))
        q32, q64 = float(ref.quality(s32)[0]), float(ref.quality(s64)[0])
        bound = 32 * 2.0 ** -24 * (1 + mu) * (1 + float(np.linalg.norm(r.astype(np.float64), axis=1).max()))
        ratio = abs(q32 - q64) / bound
        sup_ratio = float(np.abs(s32.astype(np.float64) - s64).max()) / bound
        print(f"{name}: quality32 {q32!r} quality64 {q64!r} |diff| / bound {ratio:.4f}; worst support {sup_ratio:.4f}")
        worst = max(worst, ratio, sup_ratio)
        assert ratio <= 1.0 and sup_ratio <= 1.0, (name, ratio, sup_ratio)
    print(f"worst ratio {worst:.4f}")


def test_support32_never_takes_a_nan_and_has_no_negative_zero():
    dirs = contact.closure_directions(12)
    n = np.asarray([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]], np.float32)
    r = np.asarray([[np.inf, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)                # the first contact's 0 * inf: every h of it is NaN
    s = ref.support32(n, r, dirs, 0.5)
    assert not np.isnan(s).any() and s[4] == 1.0 and s[5] == -1.0
    z = ref.support32(np.zeros((1, 3), np.float32), r[1:], dirs, 0.0)                # a degenerate normal: every h is 0, and +0
    assert np.array_equal(bits(z), np.zeros(12, np.uint32))
    assert np.isneginf(ref.support32(n[:0], r[:0], dirs, 0.5)).all()


# ------------------------------------------------------------------------------------------------------ CPU: host statistics, the guard
def test_closure_stats_and_class():
    quality = torch.tensor([NAN, -INF, 0.0, 0.25, -0.5, 0.125, INF, -0.0])
    worst = torch.tensor([-1, -1, 7, 3, 5, 0, 0, 2], dtype=torch.int32)
    status = torch.tensor([2, 1, 0, 0, 0, 0, 0, 0], dtype=torch.int32)
    got = contact.closure_stats(quality, worst, status)
    assert list(got) == list(FIELDS)
    assert got["closure_quality"] == [None, None, 0.0, 0.25, -0.5, 0.125, None, -0.0]
    assert got["force_closure"] == [None, None, False, True, False, True, None, False]    # 0 is a certificate of NO closure
    assert got["closure_direction"] == [None, None, 7, 3, 5, 0, None, 2]
    assert all(type(x) in (float, type(None)) for x in got["closure_quality"]) and all(type(x) in (bool, type(None)) for x in got["force_closure"])
    text = json.dumps(got)
    assert "NaN" not in text and "Infinity" not in text and json.loads(text)["closure_quality"][:2] == [None, None]
    assert contact.closure_stats(quality.numpy(), worst.numpy(), status.numpy()) == got
    with pytest.raises(RuntimeError):
        contact.closure_stats(quality, worst[:3], status)
    out = {"quality": quality, "status": status}
    assert contact.closure_class(out, 0.125).tolist() == [2, 1, 1, 0, 1, 0, 0, 1]    # 0.125 itself passes; no contact is class 1, a NaN row class 2
    assert contact.closure_class(out, -INF).tolist() == [2, 1, 0, 0, 0, 0, 0, 0]
    assert contact.closure_class(out, 0.0).tolist() == [2, 1, 0, 0, 1, 0, 0, 0]      # -0.0 is not below 0
    cls = contact.closure_class(out, 0.2)
    assert cls.dtype == torch.int32 and cls.tolist() == [2, 1, 1, 0, 1, 1, 0, 1]
    with pytest.raises(RuntimeError):
        contact.closure_class(out, NAN)


# ------------------------------------------------------------------------------------------------------ CPU: the rule table, the keyword path
def test_rule_table_and_keyword_path():
    assert generate.RULES[-3:] == generate.VOLUME_MESH_RULES
    assert generate.RULES[-9:-3] == generate.CLOSURE_RULES and [r.only for r in generate.CLOSURE_RULES] == ["cli"] * 6
    assert generate._Closure not in generate.FIGURES and "closure" not in generate.GROUPS and generate.EXTRA_FIGURES == (generate._Closure,)
    objs = [torch.zeros(4, 8)]
    call = lambda **kw: generate.generate_with_closure(None, objs, 5, True, 0, [0], **kw)      # net = None: nothing may touch it
    for kw, text in ((dict(friction=-1.0), "friction must be finite and >= 0"), (dict(friction=NAN), "friction must be finite and >= 0"),
                     (dict(friction=INF), "friction must be finite and >= 0"),
                     (dict(closure_dirs=11), "closure_dirs must lie between 12 and 1024"), (dict(closure_dirs=1025), "closure_dirs must lie between 12 and 1024"),
                     (dict(min_closure=NAN, candidates=8), "min_closure must not be NaN"),
                     (dict(min_closure=0.0), "min_closure needs candidates"),
                     (dict(torque_length=0.0), "torque_length must be finite and positive"),
                     (dict(volume_mesh=3), "volume_mesh must be 0, 1 or 2"), (dict(candidates=3), "candidates must be 0 or at least num_grasp")):
        with pytest.raises(RuntimeError) as e:
            call(**kw)
        assert str(e.value).startswith("generate_for_objects: " + text) and "(got " in str(e.value) and "--" not in str(e.value), str(e.value)
    with pytest.raises(TypeError):
        generate.generate_for_objects(None, objs, 5, True, 0, [0], friction=0.3)    # the pinned signature has none of the four
    # the flag path: each rule with its own message
    for argv, text in ((["--closure", "3"], "--closure is 0 or 1"), (["--closure", "1", "--friction", "-1"], "--friction must be finite"),
                       (["--closure", "1", "--closure_dirs", "5"], "--closure_dirs must lie between 12 and 1024"),
                       (["--min_closure", "nan"], "--min_closure must not be NaN"), (["--min_closure", "0"], "--min_closure needs --candidates"),
                       (["--friction", "0.3"], "--closure_dirs and --friction away from their defaults need --closure")):
        rule = generate._broken_rule(generate.types.SimpleNamespace(**{**vars(generate.build_parser("ho3d").parse_args(argv)), "rotate": True}), cli=True)
        assert rule in generate.CLOSURE_RULES
        assert generate._rule_message(rule, generate.build_parser("ho3d").parse_args(argv), cli=True).startswith(text)


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


CASES = ["1x1x1", "3x255x776", "3x256x776", "2x257x778", "2x1025x778"]


def closure_case(name, tmp_path):
    """(hand [B,V,3], faces, obj [B,N,3]) numpy fp32, built as tests/test_grasp_wrench.py builds wrench_case -- points on both sides of
    the surface, some within the contact threshold, some not -- with the LAST row's cloud drawn together to a patch of a few
    millimetres at one hand vertex (normals within a narrow cone: certified open at both mu) while the rows before it are enclosed; and
    with 1025 points the one point of the second tile sits at that vertex too: contacts on both sides of the seam."""
    from test_grasp_wrench import wrench_case
    hand, faces, obj = wrench_case(name, tmp_path)
    if name == "1x1x1":
        return hand, faces, obj
    obj = obj.copy()
    at = hand[:, hand.shape[1] // 2][:, None]                                        # [B,1,3]: on the sphere a vertex near the equator, where the mesh is coarser than the noise
    obj[-1] = (at[-1] + np.float32(0.03) * (obj[-1] - obj[-1].mean(axis=0))).astype(np.float32)   # sigma 1 mm about the vertex
    if obj.shape[1] > 1024:
        obj[:, 1024] = (at[:, 0] + np.float32(0.003)).astype(np.float32)
    return hand, faces, obj


_REFERENCES = {}


def reference(name, mu, tmp_path):
    """The case and its reference over all 1024 directions, computed once per (case, mu); ref.cut gives the shorter tables."""
    if (name, mu) not in _REFERENCES:
        hand, faces, obj = closure_case(name, tmp_path)
        _REFERENCES[(name, mu)] = (hand, faces, obj, ref.grasp_closure(hand, faces, obj, 1.0 / LENGTH, mu, contact.closure_directions(1024), THR))
    return _REFERENCES[(name, mu)]


@pytest.mark.parametrize("name", CASES)
def test_the_cases_exercise_the_kernel(name, tmp_path):
    """On the REFERENCE, without a GPU: some row has some points in contact and some not, some quality is above 0 and some below."""
    for mu in MUS:
        hand, faces, obj, want = reference(name, mu, tmp_path)
        N = obj.shape[1]
        print(name, mu, {D: (ref.cut(want, D)["quality"].tolist(), ref.cut(want, D)["worst_dir"].tolist()) for D in DS}, want["n_contact"].tolist())
        if name == "1x1x1":                                                          # a degenerate normal: every h is 0, quality 0
            assert want["n_contact"].tolist() == [1] and want["status"].tolist() == [0]
            assert np.array_equal(bits(want["support"]), np.zeros((1, 1024), np.uint32)) and want["worst_dir"].tolist() == [0]
            continue
        assert (want["status"] == 0).all() and ((0 < want["n_contact"]) & (want["n_contact"] < N)).any()
        for D in DS:                                                                 # (twelve axes alone may miss the open row's gap)
            q = ref.cut(want, D)["quality"]
            assert (q < 0).any() or D < 256, (name, mu, D, q)
            assert (q > 0).any(), (name, mu, D, q)
        if N > 1024:
            assert want["contact"][:, 1024].all() and want["contact"][:, :1024].any(axis=1).all()


def run_closure(hand, faces, obj_dev, mu, D, length=LENGTH, thr=THR, want_support=True):
    topo = contact.HandTopology(faces, hand.shape[1], DEV)
    out = contact.grasp_closure(topo, gpu(hand), obj_dev, length, mu, D, thr, want_support)
    assert tuple(out) == OUTPUTS + (("support",) if want_support else ())
    B = hand.shape[0]
    assert [tuple(out[k].shape) for k in OUTPUTS] == [(B,), (B,), (B,), (B,), (B, 3)]
    assert [out[k].dtype for k in OUTPUTS] == [torch.float32, torch.int32, torch.int32, torch.int32, torch.float32]
    if want_support:
        assert tuple(out["support"].shape) == (B, D if isinstance(D, int) else D.shape[0]) and out["support"].dtype == torch.float32
    return topo, {k: v.cpu().numpy() for k, v in out.items()}


def assert_same_bits(got, want, rows=None, what="", keys=OUTPUTS + ("support",)):
    """Every number bit for bit; a NaN is a NaN (its payload is nobody's contract)."""
    for k in keys:
        g, w = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        if g.dtype != np.float32:
            assert np.array_equal(g, w), (what, k, g, w)
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, k, g, w)
        assert np.array_equal(bits(g)[~nan], bits(w)[~nan]), (what, k, g[~nan][bits(g)[~nan] != bits(w)[~nan]][:4], w[~nan][bits(g)[~nan] != bits(w)[~nan]][:4])


@pytest.mark.gpu
@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("name", CASES)
def test_grasp_closure_equals_the_reference_bit_for_bit(name, mu, tmp_path):
    hand, faces, obj, full = reference(name, mu, tmp_path)
    obj_dev = gpu(obj)
    for D in DS:
        want = ref.cut(full, D)
        topo, got = run_closure(hand, faces, obj_dev, mu, D)
        print(name, mu, D, "quality", got["quality"], want["quality"], "worst_dir", got["worst_dir"], want["worst_dir"], "n_contact", got["n_contact"])
        assert_same_bits(got, want, what=f"{name} mu={mu} D={D}")
        _, bare = run_closure(hand, faces, obj_dev, mu, D, want_support=False)       # support = NULL: the other outputs are the same
        assert_same_bits(bare, got, what=f"{name} mu={mu} D={D} without support", keys=OUTPUTS)
    # n_contact carries the bits of dvq_grasp_scores, centre those of dvq_grasp_wrench, on the same inputs
    scores = contact.grasp_scores(topo, gpu(hand), obj_dev, THR)
    assert np.array_equal(scores["n_contact"].cpu().numpy(), got["n_contact"])
    wrench = contact.grasp_stability(topo, gpu(hand), obj_dev, LENGTH, THR)
    assert np.array_equal(bits(wrench["centre"].cpu().numpy()), bits(got["centre"]))
    # and a table of the caller's own is read as the packaged one
    _, own = run_closure(hand, faces, obj_dev, mu, gpu(contact.closure_directions(DS[-1]).copy()))
    assert_same_bits(own, got, what="own table")


@pytest.mark.gpu
def test_grasp_closure_reads_a_channel_first_view_in_place():
    v, f = score_ref.sphere_mesh()
    B, N, D, mu = 3, 500, 256, 0.5
    cloud = synth.synthetic_normal((B, 4, N), 52, "closure/cf", 0.04)                    # [B,4,N] as the generation path holds it
    hand = (v[None] * np.asarray([1.0, 0.9, 1.1], np.float32)[:, None, None]).astype(np.float32)
    view = gpu(cloud)[:, :3].transpose(1, 2)                                             # strides (4N, 1, N)
    assert not view.is_contiguous()
    _, got = run_closure(hand, f, view, mu, D)
    _, copy = run_closure(hand, f, view.contiguous(), mu, D)
    obj = cloud[:, :3].transpose(1, 2).contiguous().numpy()
    want = ref.grasp_closure(hand, f, obj, 1.0 / LENGTH, mu, contact.closure_directions(D), THR)
    assert ((0 < want["n_contact"]) & (want["n_contact"] < N)).any() and (want["status"] == 0).all()
    assert_same_bits(got, want, what="view")
    assert_same_bits(got, copy, what="view against its contiguous copy")


@pytest.mark.gpu
def test_grasp_closure_with_a_nan_row_and_rows_alone():
    v, f = score_ref.sphere_mesh()
    B, N, D, mu = 4, 300, 64, 0.5
    hand = (v[None] * np.linspace(0.9, 1.1, B).astype(np.float32)[:, None, None]).astype(np.float32)
    obj = synth.synthetic_normal((B, N, 3), 53, "closure/nan", 0.04).numpy()
    _, clean = run_closure(hand, f, gpu(obj), mu, D)
    assert ((0 < clean["n_contact"]) & (clean["n_contact"] < N)).all() and (clean["status"] == 0).all() and np.isfinite(clean["quality"]).all()
    bad = obj.copy()
    bad[1, 17, 2] = np.nan                                                               # a NaN object coordinate: row 1
    _, got = run_closure(hand, f, gpu(bad), mu, D)
    assert got["status"].tolist() == [0, 2, 0, 0] and np.isnan(got["quality"][1]) and got["worst_dir"][1] == -1 and np.isnan(got["support"][1]).all()
    assert_same_bits(got, clean, rows=[0, 2, 3], what="the rows beside the NaN row")
    assert_same_bits(got, ref.grasp_closure(hand, f, bad, 1.0 / LENGTH, mu, contact.closure_directions(D), THR), what="nan")
    cls = contact.closure_class({k: torch.from_numpy(x) for k, x in got.items()}, -1.0)
    assert cls[1] == 2 and contact.closure_stats(got["quality"], got["worst_dir"], got["status"])["closure_quality"][1] is None
    broken = hand.copy()
    broken[2, 100, 0] = np.inf                                                           # and a hand coordinate that is not finite: row 2
    _, got_h = run_closure(broken, f, gpu(obj), mu, D)
    assert got_h["status"].tolist() == [0, 0, 2, 0]
    assert_same_bits(got_h, ref.grasp_closure(broken, f, obj, 1.0 / LENGTH, mu, contact.closure_directions(D), THR), what="inf in the hand")
    for b in range(B):                                                                   # a row alone gives the bits it has inside the batch
        _, one = run_closure(hand[b:b + 1], f, gpu(bad[b:b + 1]), mu, D)
        assert_same_bits(one, {k: x[b:b + 1] for k, x in got.items()}, what=f"row {b} alone")
    # another length scales the arms: the supports of the six pure-force axes do not see it, the torque rows do
    _, short = run_closure(hand, f, gpu(obj), mu, D, length=0.05)
    assert np.array_equal(bits(short["support"][:, :6]), bits(clean["support"][:, :6]))
    assert not np.array_equal(short["support"][:, 6:12], clean["support"][:, 6:12])
    far = (obj + np.float32(1.0)).astype(np.float32)                                     # and a cloud a metre away: status 1
    _, none = run_closure(hand, f, gpu(far), mu, D)
    assert none["status"].tolist() == [1] * B and np.isneginf(none["quality"]).all() and (none["worst_dir"] == -1).all() and np.isneginf(none["support"]).all()


@pytest.mark.gpu
def test_grasp_closure_across_the_chunk_seam():
    """B = 65 537 grasps in two launches (65 535 + 2): the rows at the seam equal the reference."""
    B, rows, D, mu = 65537, [0, 65534, 65535, 65536], 12, 0.5
    tetra = np.asarray([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.05, 0.0], [0.0, 0.0, 0.05]], np.float32)
    faces = np.asarray([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int64)
    hand = (tetra[None] + synth.synthetic_normal((B, 4, 3), 54, "closure/seam/h", 0.005).numpy()).astype(np.float32)
    near = hand[np.arange(B), np.arange(B) % 4][:, None]                                 # row b's point sits at its vertex b mod 4
    obj = (near + synth.synthetic_normal((B, 1, 3), 54, "closure/seam/o", 0.005).numpy()).astype(np.float32)
    _, got = run_closure(hand, faces, gpu(obj), mu, D)
    want = ref.grasp_closure(hand[rows], faces, obj[rows], 1.0 / LENGTH, mu, contact.closure_directions(D), THR)
    assert want["n_contact"].tolist() == [1, 1, 1, 1] and want["status"].tolist() == [0] * 4 and len({x.tobytes() for x in want["support"]}) == 4
    assert_same_bits({k: x[rows] for k, x in got.items()}, want, what="seam")
    assert set(np.unique(got["n_contact"]).tolist()) <= {0, 1} and got["n_contact"].mean() > 0.9    # N = 1; a 4-sigma offset misses
    assert np.array_equal(got["status"], 1 - got["n_contact"]) and np.array_equal(np.isneginf(got["quality"]), got["n_contact"] == 0)
    topo = contact.HandTopology(faces, 4, DEV)
    empty = contact.grasp_closure(topo, gpu(hand)[:0].contiguous(), gpu(obj)[:0].contiguous(), dirs=D, want_support=True)
    assert [tuple(empty[k].shape) for k in OUTPUTS + ("support",)] == [(0,), (0,), (0,), (0,), (0, 3), (0, D)]


@pytest.mark.gpu
def test_grasp_closure_refuses_what_the_kernel_cannot_hold():
    v, f = score_ref.sphere_mesh(4, 6)
    topo = contact.HandTopology(f, len(v), DEV)
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL, nothing launched
    one = torch.full((64,), 7.0, device=DEV)
    p = one.data_ptr()
    for V, N, B, D, mu in ((2049, 4, 1, 12, 0.5), (0, 4, 1, 12, 0.5), (5, 0, 1, 12, 0.5), (5, 4, -1, 12, 0.5), (5, 4, 1, 0, 0.5), (5, 4, 1, 1025, 0.5),
                           (5, 4, 1, 12, -0.5), (5, 4, 1, 12, INF), (5, 4, 1, 12, NAN)):
        rc = lib.dvq_grasp_closure(p, topo.faces.data_ptr(), topo.vf_off.data_ptr(), topo.vf_face.data_ptr(), V, p, 0, 3, 1, B, N, 0.0004, 10.0,
                                   mu, p, D, p, p, p, p, p, None, None)
        assert rc == 1, (V, N, B, D, mu)
    assert (one == 7.0).all()                                           # nothing was written


# ------------------------------------------------------------------------------------------------------ GPU: end to end
def _run_main(dataset, out_dir, extra, mano):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


def _cloud_files(tmp_path):
    from test_grasp_wrench import e2e_clouds
    files, clouds = [], e2e_clouds()
    for i, c in enumerate(clouds):
        files.append(str(tmp_path / f"cloud{i}.npy"))
        np.save(files[-1], c)
    return files, clouds


def _closure_of_the_written_hands(net, j, obj4n, mu, D):
    """contact.closure_stats of contact.grasp_closure on the hands re-posed from a JSON's parameters against the cloud re-posed from
    its rotations."""
    params = torch.tensor([p[0] for p in j["recon_params"]], dtype=torch.float32, device=DEV)
    Rt = np.asarray(j["R_list"])
    R = torch.as_tensor(Rt[:, :, :3], dtype=torch.float32, device=DEV).contiguous()
    t = torch.as_tensor(Rt[0, :, 3], dtype=torch.float32, device=DEV).contiguous()
    posed = ops.transform_cloud(obj4n.to(DEV).contiguous(), R, t)
    verts = generate._pose(net, params).vertices
    out = contact.grasp_closure(generate._hand_topology(net, verts.shape[1], torch.device(DEV)), verts, posed[:, :3].transpose(1, 2), LENGTH, mu, D)
    return contact.closure_stats(out["quality"], out["worst_dir"], out["status"]), out


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", ["ho3d", "obman"])
def test_entry_point_writes_the_closure_fields(dataset, tmp_path):
    """ho3d poses every object under its own rotation and the canonical offset, where the hands of the synthetic weights stand 0.8 m
    from the cloud: every figure is null there and every candidate is under the limit; obman leaves the clouds about the hands, where
    the figures are numbers."""
    from test_grasp_select import _gennet, mano_pkl
    from test_grasp_wrench import E2E_K as k, E2E_M as M
    mano = mano_pkl(tmp_path)
    files, clouds = _cloud_files(tmp_path)
    mu, D, limit = 0.7, 64, -0.2
    base = ["--objects"] + files + ["--num_grasp", str(k), "--candidates", str(M)]
    flags = base + ["--closure", "1", "--friction", str(mu), "--closure_dirs", str(D), "--min_closure", str(limit)]
    names0, bytes0 = _run_main(dataset, str(tmp_path / "c16384"), flags + ["--rows_per_call", "16384"], mano)
    summary0 = open(str(tmp_path / "c16384" / "closure.json"), "rb").read()
    names, data = _run_main(dataset, str(tmp_path / "c8"), flags + ["--rows_per_call", "8"], mano)
    assert names == names0 == [f"obj_id_cloud{i}.json" for i in range(4)] and data == bytes0, "--rows_per_call 8: the files differ"
    assert open(str(tmp_path / "c8" / "closure.json"), "rb").read() == summary0
    before = {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact"}
    if dataset == "ho3d":                                               # without the flags: the code path of before, the same bytes, no summary
        names_p, plain = _run_main(dataset, str(tmp_path / "plain"), base, mano)
        names_o, off = _run_main(dataset, str(tmp_path / "off"), base + ["--closure", "0", "--min_closure=-inf", "--friction", "0.5", "--closure_dirs", "256"],
                                 mano)
        assert names_p == names_o == names0 and off == plain and not os.path.exists(str(tmp_path / "off" / "closure.json"))
        assert all(set(json.loads(d)) == before for d in plain)
        assert all({f: v for f, v in json.loads(d).items() if f in before} == json.loads(p) for d, p in zip(bytes0, plain))
    net = _gennet(tmp_path)
    figures = []
    for i, (d, c) in enumerate(zip(bytes0, clouds)):
        assert b"Infinity" not in d and b"NaN" not in d                 # strict JSON
        j = json.loads(d)
        assert list(j)[-3:] == list(FIELDS) and set(j) == before | set(FIELDS) and all(len(j[f]) == k for f in FIELDS)
        want, out = _closure_of_the_written_hands(net, j, generate.object_tensor(c), mu, D)
        assert {f: j[f] for f in FIELDS} == want, (i, j, want)
        assert all((j[f][r] is None) == (j["n_contact"][r] == 0) for f in FIELDS for r in range(k))
        assert out["n_contact"].tolist() == j["n_contact"]
        figures += [q for q in j["closure_quality"] if q is not None]
        # candidates under the limit rank after all others: once a kept grasp is under it (or has no figure), so is every later one
        under = [q is None or q < limit for q in j["closure_quality"]]
        assert under == sorted(under), (i, j["closure_quality"])
    s = json.loads(summary0)
    assert list(s) == ["friction", "dirs", "torque_length", "grasps", "closure_ratio", "mean_quality"]
    assert (s["friction"], s["dirs"], s["torque_length"], s["grasps"]) == (mu, D, 0.1, len(figures))
    if dataset == "ho3d":
        assert figures == [] and s["closure_ratio"] is None and s["mean_quality"] is None
    else:
        assert len(figures) >= k and s["mean_quality"] == math.fsum(figures) / len(figures)
        assert s["closure_ratio"] == sum(1 for q in figures if q > 0) / len(figures)


@pytest.mark.gpu
def test_candidates_under_the_limit_rank_last(tmp_path):
    """The keyword path on clouds about the hands: the kept candidates are those of the reference order over the classes of
    contact.select_keys raised by contact.closure_class, whatever the grouping, and the limit moves the kept set."""
    from test_grasp_select import _gennet
    from test_grasp_wrench import E2E_INDICES, E2E_K as k, E2E_M as M, E2E_SEED, e2e_clouds
    net = _gennet(tmp_path)
    objs = [generate.object_tensor(c) for c in e2e_clouds()]
    mu, D = 0.5, 64
    free = generate.generate_with_closure(net, objs, k, False, E2E_SEED, E2E_INDICES, friction=mu, closure_dirs=D, candidates=M)
    plain = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, candidates=M)
    quality = torch.cat([g["closure_scores"]["quality"] for g in free[:3]]).cpu()
    quality = quality[torch.isfinite(quality)].sort().values
    assert len(set(quality.tolist())) > M, "the candidates' figures do not vary"
    moved = False
    # half of the candidates under the limit, then three quarters, the second time in calls of one object each
    for limit, rows_per_call in ((float(quality[len(quality) // 2]), 16384), (float(quality[3 * len(quality) // 4]), M)):
        got = generate.generate_with_closure(net, objs, k, False, E2E_SEED, E2E_INDICES, friction=mu, closure_dirs=D, min_closure=limit,
                                             candidates=M, rows_per_call=rows_per_call)
        for i, (g, f, p) in enumerate(zip(got, free, plain)):
            all_c = {n: t.cpu() for n, t in g["closure_scores"].items()}
            assert set(all_c) == {"quality", "worst_dir", "status"} and all(torch.equal(all_c[n], f["closure_scores"][n].cpu()) for n in all_c)
            assert {n: torch.equal(f[n], p[n]) for n in ("params", "vertices", "candidate")} == dict(params=True, vertices=True, candidate=True)
            cls, key = contact.select_keys({n: t.cpu() for n, t in g["scores"].items()}, "penetration", 1)
            cls = torch.maximum(cls, contact.closure_class(all_c, limit))
            want = score_ref.segment_topk(cls.numpy(), key.numpy(), 1, M, k)[0]
            c = g["candidate"].cpu().numpy()
            assert np.array_equal(c, want), (i, c, want)
            assert all(torch.equal(g["closure"][n].cpu(), all_c[n][c]) for n in all_c)
            assert g["json"]["closure_quality"] == contact.closure_stats(*(all_c[n][c] for n in ("quality", "worst_dir", "status")))["closure_quality"]
            moved |= not np.array_equal(c, f["candidate"].cpu().numpy())
            kept_cls = cls.numpy()[c]
            assert list(kept_cls) == sorted(kept_cls)
            print(f"rows_per_call {rows_per_call} object {i}: kept {c.tolist()} classes {kept_cls.tolist()} quality {all_c['quality'].tolist()}")
    assert moved, "the limit changes no kept set: the guard is not exercised"
