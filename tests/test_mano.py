"""The MANO layer (csrc/mano.hip, ops.mano_forward, packing.PackedMano, mano.ManoLayer) against tests/mano_ref.py, a float64
restatement of SURVEY.md Appendix E, on the real hand model (tests/golden/g9_mano_right.pkl.xz) and the synthetic one.

CPU group (unmarked): the reference itself is checked by properties that do not share its code path, the fp32 oracle is pinned
to it, and the packed tensors are shown to hold the same model.  GPU group (``gpu`` marker): the kernels against the reference.

Tolerance of every device comparison: ``e32`` is the max-abs error of the fp32 CPU oracle against the reference on the same
inputs; the device must be within ``8 * e32``, vertices and joints separately.  e32 comes from the reference side.  The factor 8
is not measured: it allows for the kernels' summation orders, the device's sinf / cosf and the two-plane fp16 blendshape image.
Each comparison prints a ``mano-ratio`` line (device error / e32); DESIGN.md records them."""
import ctypes as C
import lzma
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, ops, packing, synth
from dvqvae_amd import mano as dmano
from oracle import mano_oracle

import mano_ref as ref

DEV = "cuda:0"
gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = ("real", "synthetic")
FACTOR = 8.0


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """{"real": arrays of the committed MANO_RIGHT.pkl, "synthetic": synthetic_mano_arrays()} (float64 as stored)."""
    path = str(tmp_path_factory.mktemp("mano") / "MANO_RIGHT.pkl")
    with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    return {"real": dmano.read_mano_pkl(path), "synthetic": dmano.synthetic_mano_arrays()}


def _inputs(B, tag, pose_scale=0.8, betas_scale=1.0, go_scale=1.0, tr_scale=0.3):
    return (synth.synthetic_normal((B, 10), 61, f"tmano/{tag}/betas", betas_scale),
            synth.synthetic_normal((B, 45), 61, f"tmano/{tag}/pose", pose_scale),
            synth.synthetic_normal((B, 3), 61, f"tmano/{tag}/go", go_scale),
            synth.synthetic_normal((B, 3), 61, f"tmano/{tag}/tr", tr_scale))


def _oracle(arrays, flat, betas, pose, go=None, tr=None):
    v, j = mano_oracle.ManoOracle(arrays, flat_hand_mean=flat)(betas, pose, go, tr, return_joints=True)
    return v.double().numpy(), j.double().numpy()


def _maxabs(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    return float(np.abs(a - b).max())


# ========================================================================================== CPU group
def _stored(arrays):
    assert np.abs(np.asarray(arrays["weights"], np.float64).sum(1) - 1).max() <= 1e-15
    return arrays


@pytest.mark.parametrize("model", MODELS)
def test_ref_zero_pose_is_the_shaped_template(models, model):
    """On the model as stored (float64): its skinning weights sum to one to the last bit or two, the fp32-rounded ones only to
    4e-8, which moves a zero-pose vertex by 4e-9 -- on the device as well as here."""
    a = _stored(models[model])
    betas = synth.synthetic_normal((5, 10), 61, "tmano/zero/betas", 2.0).double().numpy()
    v, j = ref.mano_ref(a, betas, np.zeros((5, 45)))
    shaped = a["v_template"][None] + np.einsum("vkl,bl->bvk", a["shapedirs"], betas)
    assert np.abs(v - shaped).max() <= 1e-12
    assert np.abs(j - np.einsum("jv,bvk->bjk", a["J_regressor"], shaped)).max() <= 1e-12


@pytest.mark.parametrize("flat", (True, False))
@pytest.mark.parametrize("model", MODELS)
def test_ref_rigid_motion(models, model, flat):
    """verts(go, tr) = R(go) (verts(0, 0) - J0) + J0 + tr with J0 the shaped root joint, and the same for the joints: the global
    orientation and the translation move the posed hand rigidly about its root (exactly so when the skinning weights sum to one:
    the model as stored)."""
    a = _stored(models[model])
    betas, pose, go, tr = (t.double().numpy() for t in _inputs(6, "rigid"))
    v0, j0 = ref.mano_ref(a, betas, pose, flat_hand_mean=flat)
    v1, j1 = ref.mano_ref(a, betas, pose, go, tr, flat_hand_mean=flat)
    shaped = a["v_template"][None] + np.einsum("vkl,bl->bvk", a["shapedirs"], betas)
    root = np.einsum("v,bvk->bk", a["J_regressor"][0], shaped)[:, None]
    R = ref.rodrigues(go)
    for x0, x1 in ((v0, v1), (j0, j1)):
        want = np.einsum("bik,bnk->bni", R, x0 - root) + root + tr[:, None]
        assert np.abs(x1 - want).max() <= 1e-12
    assert np.abs(j0[:, 0] - root[:, 0]).max() <= 1e-12                 # zero orientation leaves the root where it was regressed


@pytest.mark.parametrize("model", MODELS)
def test_ref_bone_lengths_do_not_change(models, model):
    """|posed joint - posed parent| = |rest joint - rest parent|.  Relative bound 1e-7: with angle = ||r + 1e-8|| the axis r / angle
    is not exactly a unit vector (k = |r| / angle, |1 - k^2| <= 2 sqrt(3) 1e-8 / |r|), which stretches a rotation by at most
    (1 - cos a)^2 |1 - k^2| / 2 <= 2.3e-8 for any angle; at most four rotations act on a bone (root and three in a finger)."""
    a = ref.device_arrays(models[model])
    betas, pose, go, tr = (t.double().numpy() for t in _inputs(16, "bones", pose_scale=1.5))
    for flat in (True, False):
        o = ref.mano_ref_full(a, betas, pose, go, tr, flat_hand_mean=flat)
        for j, p in enumerate(a["parents"]):
            if p < 0:
                continue
            rest = np.linalg.norm(o["J"][:, j] - o["J"][:, p], axis=1)
            posed = np.linalg.norm(o["joints"][:, j] - o["joints"][:, p], axis=1)
            assert rest.min() > 1e-3 and np.abs(posed / rest - 1).max() <= 1e-7, (flat, j)


def test_ref_rotations_are_rotations():
    """Orthonormal, determinant 1, at the angles where Rodrigues goes wrong.  |R^T R - I| = (1 - cos a)^2 |1 - k^2| with k as in the
    bone-length test: at most 4 * 2 sqrt(3) 1e-8 / pi = 4.4e-8 (a = pi) for the angles >= 1, below 1e-14 for the angles <= 1e-4."""
    rng = np.random.default_rng(5)
    axes = np.concatenate([np.eye(3), -np.eye(3), rng.normal(size=(10, 3))])
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    for angle in (0.0, 1e-7, 1e-4, 1.0, np.pi - 1e-3, np.pi, 7.0):
        R = ref.rodrigues(axes * angle)
        tol = 1e-14 if angle <= 1e-4 else 1e-7
        assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= tol, angle
        assert np.abs(np.linalg.det(R) - 1).max() <= tol, angle
        # the rotation it should be: axis kept, a vector orthogonal to it turned by the angle
        assert np.abs((R @ axes[..., None])[..., 0] - axes).max() <= 1e-7
        perp = np.cross(axes, np.roll(axes, 1, axis=1) + 0.5)
        perp /= np.linalg.norm(perp, axis=1, keepdims=True)
        got = (R @ perp[..., None])[..., 0]
        assert np.abs((got * perp).sum(1) - np.cos(angle)).max() <= 1e-7
        assert np.abs((np.cross(perp, got) * axes).sum(1) - np.sin(angle)).max() <= 1e-7


# pose scale, betas scale: the four input scales of the measurement the 1e-6 rests on (max 3.5e-7, times three)
SCALES = ((0.0, 1.0), (1e-4, 1.0), (0.8, 1.0), (2.0, 3.0))


@pytest.mark.parametrize("flat", (True, False))
@pytest.mark.parametrize("model", MODELS)
def test_fp32_oracle_agrees_with_the_reference(models, model, flat):
    """Pins oracle/mano_oracle.ManoOracle, on which the golden files and the 1e-5 GPU contract rest."""
    a = ref.device_arrays(models[model])
    for ps, bs in SCALES:
        betas, pose, go, tr = _inputs(12, f"oracle/{ps}", pose_scale=max(ps, 1e-30), betas_scale=bs)
        if ps == 0.0:
            pose, go = torch.zeros_like(pose), torch.zeros_like(go)
        rv, rj = ref.mano_ref(a, betas, pose, go, tr, flat_hand_mean=flat)
        ov, oj = _oracle(models[model], flat, betas, pose, go, tr)
        ev, ej = np.abs(ov - rv).max(), np.abs(oj - rj).max()
        print(f"mano-oracle {model} flat={flat} pose={ps} betas={bs}: e32 verts {ev:.2e} joints {ej:.2e}")
        assert ev <= 1e-6 and ej <= 1e-6, (ps, bs, ev, ej)


@pytest.mark.parametrize("flat", (True, False))
@pytest.mark.parametrize("model", MODELS)
def test_packed_tensors_hold_the_same_model(models, model, flat):
    """PackedMano on the CPU (construction needs no device): the folded joint regressor and the [160]-wide blendshape operand
    reproduce the reference's rest joints and posed vertices; float64 arithmetic on the fp32 tensors, 1e-6."""
    t = {k: v.double().numpy() for k, v in packing.PackedMano(models[model], flat_hand_mean=flat).tensors.items()}
    betas, pose, go, tr = _inputs(9, "pack", betas_scale=2.0)
    o = ref.mano_ref_full(ref.device_arrays(models[model]), betas, pose, go, tr, flat_hand_mean=flat)
    b64 = betas.double().numpy()
    J = t["j_template"].reshape(16, 3)[None] + (b64 @ t["j_shapedirs"]).reshape(-1, 16, 3)
    assert np.abs(J - o["J"]).max() <= 1e-6
    X = np.concatenate([b64, o["pose_feature"], np.zeros((9, 15))], axis=1)
    assert t["blend_w"].shape == (2334, 160) and not t["blend_w"][:, 145:].any()
    V = X @ t["blend_w"].T + t["v_template"].reshape(-1)
    assert np.abs(V.reshape(9, 778, 3) - o["v_posed"]).max() <= 1e-6
    mean = np.zeros(45) if flat else ref.device_arrays(models[model])["hands_mean"]
    assert np.array_equal(t["pose_mean"], np.concatenate([np.zeros(3), mean]))
    assert np.array_equal(t["comps"], ref.device_arrays(models[model])["hands_components"][:45])
    assert np.array_equal(t["weights"], ref.device_arrays(models[model])["weights"])


@pytest.mark.parametrize("model", MODELS)
def test_from_module_packs_what_the_constructor_packs(models, model):
    """ManoLayer.from_module on a stand-in with smplx-style fp32 buffers == ManoLayer(the same fp32 numbers, flat_hand_mean=False)."""
    a = ref.device_arrays(models[model])
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    layer = types.SimpleNamespace(
        v_template=t32(a["v_template"]), shapedirs=t32(a["shapedirs"]),
        posedirs=t32(a["posedirs"].reshape(778 * 3, 135).T), J_regressor=t32(a["J_regressor"]),
        lbs_weights=t32(a["weights"]), hand_components=t32(a["hands_components"]),
        pose_mean=t32(np.concatenate([np.zeros(3), a["hands_mean"]])),
        parents=torch.from_numpy(np.asarray(a["parents"], dtype=np.int64)), faces=np.asarray(a["faces"]))
    assert tuple(layer.posedirs.shape) == (135, 2334) and float(layer.pose_mean[3:].abs().max()) > 0
    got, want = dmano.ManoLayer.from_module(layer)._packed, dmano.ManoLayer(a, flat_hand_mean=False)._packed
    assert sorted(got.tensors) == sorted(want.tensors)
    for k in want.tensors:
        assert got.tensors[k].dtype == want.tensors[k].dtype and torch.equal(got.tensors[k], want.tensors[k]), k
    assert got.parents == want.parents and got.parents[0] == -1
    assert np.array_equal(got.faces, want.faces)


# ========================================================================================== GPU group
_layers = {}


def _layer(models, model, flat):
    key = (model, flat, packing.gemm_kind())
    if key not in _layers:
        _layers[key] = dmano.ManoLayer(models[model], flat_hand_mean=flat).to(DEV)
    return _layers[key]


def _gemm_name():
    return os.environ.get("DVQ_GEMM", "").strip().lower() or "f16x2"


def _quant_term(models, model, flat, betas, pose, go):
    """max over the batch of 2^-21 sum_k |X_k| |blend_vk|: what the two-plane fp16 blendshape image may cost (reported only)."""
    o = ref.mano_ref_full(ref.device_arrays(models[model]), betas, pose, go, None, flat_hand_mean=flat)
    X = np.abs(np.concatenate([betas.double().numpy(), o["pose_feature"]], axis=1))
    W = np.abs(packing.PackedMano(models[model], flat_hand_mean=flat).tensors["blend_w"].double().numpy()[:, :145])
    return float((X @ W.T).max() * 2.0 ** -21)


def _compare(what, models, model, flat, betas, pose, go, tr, got_v, got_j=None, cm=False):
    """Device vertices ([B,778,3], or [B,3,778] with ``cm``) and joints against the reference, within FACTOR * e32."""
    a = ref.device_arrays(models[model])
    rv, rj = ref.mano_ref(a, betas, pose, go, tr, flat_hand_mean=flat)
    ov, oj = _oracle(models[model], flat, betas, pose, go, tr)
    e32v, e32j = float(np.abs(ov - rv).max()), float(np.abs(oj - rj).max())
    if cm:
        got_v = got_v.permute(0, 2, 1)
    dv = _maxabs(got_v, rv)
    dj = _maxabs(got_j, rj) if got_j is not None else 0.0
    print(f"mano-ratio {_gemm_name()} {model} flat={flat} {what}: verts {dv:.3e} / e32 {e32v:.3e} = {dv / e32v:.2f}"
          + (f"; joints {dj:.3e} / e32 {e32j:.3e} = {dj / e32j:.2f}" if got_j is not None else ""))
    assert e32v > 0 and e32j > 0
    assert dv <= FACTOR * e32v, f"{what}: vertices differ from the float64 reference by {dv:.3e} > {FACTOR:g} x e32 = {FACTOR * e32v:.3e}"
    assert dj <= FACTOR * e32j, f"{what}: joints differ from the float64 reference by {dj:.3e} > {FACTOR:g} x e32 = {FACTOR * e32j:.3e}"
    return dv / e32v, (dj / e32j if got_j is not None else 0.0)


BATCHES = (1, 2, 3, 4, 5, 7, 64, 65, 257)      # WPB = 4: one live lane with three dead ones, full blocks, a ragged last block


@gpu
@pytest.mark.parametrize("flat", (True, False))
@pytest.mark.parametrize("model", MODELS)
def test_parity_matrix(models, model, flat):
    layer = _layer(models, model, flat)
    worst = [0.0, 0.0, 0.0]
    for B in BATCHES:
        betas, pose, go, tr = _inputs(B, f"matrix/{model}/{flat}/{B}")
        out = layer(betas=betas.to(DEV), global_orient=go.to(DEV), hand_pose=pose.to(DEV), transl=tr.to(DEV))
        assert tuple(out.vertices.shape) == (B, 778, 3) and tuple(out.joints.shape) == (B, 16, 3)
        rv, rj = _compare(f"B={B}", models, model, flat, betas, pose, go, tr, out.vertices, out.joints)
        cm = layer.vertices_channel_major(betas.to(DEV), pose.to(DEV))
        assert tuple(cm.shape) == (B, 3, 778)
        rc, _ = _compare(f"B={B} channel-major", models, model, flat, betas, pose, None, None, cm, cm=True)
        worst = [max(w, r) for w, r in zip(worst, (rv, rj, rc))]
    print(f"mano-ratio-worst {_gemm_name()} {model} flat={flat}: verts {worst[0]:.2f} joints {worst[1]:.2f} channel-major {worst[2]:.2f}; "
          f"fp16-image term {_quant_term(models, model, flat, *_inputs(64, f'matrix/{model}/{flat}/64')[:3]):.2e}")


def _edge_inputs(case, arrays, flat):
    B = 8
    betas, pose, go, tr = _inputs(B, f"edge/{case}")
    if case == "zero":
        pose, go = torch.zeros_like(pose), torch.zeros_like(go)
    elif case in ("1e-7", "1e-4"):
        betas, pose, go, tr = _inputs(B, f"edge/{case}", pose_scale=float(case), go_scale=float(case))
    elif case == "large":
        betas, pose, go, tr = _inputs(B, "edge/large", pose_scale=2.0, betas_scale=3.0)
    elif case == "pi-and-7":
        g = go.double().numpy()
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        g[0], g[1] = (1.0, 0.0, 0.0), (0.0, 0.0, -1.0)
        g[0::2] *= np.pi                                # rows 0 2 4 6: |go| = pi (row 0 exactly fp32's pi on one axis)
        g[1::2] *= 7.0                                  # rows 1 3 5 7: |go| = 7 (row 1 exactly)
        go = torch.from_numpy(g.astype(np.float32))
    elif case == "one-joint-zero":
        # full pose = pose @ comps + mean: row b's joint 1 + b has a zero axis-angle, the other joints large ones
        target = synth.synthetic_normal((B, 45), 61, "tmano/edge/target", 1.5).double().numpy()
        for b in range(B):
            target[b, 3 * b: 3 * b + 3] = 0.0
        mean = np.zeros(45) if flat else np.asarray(arrays["hands_mean"], np.float64)
        comps = np.asarray(arrays["hands_components"], np.float64)[:45]
        pose = torch.from_numpy(np.linalg.solve(comps.T, (target - mean).T).T.astype(np.float32))
        back = pose.double().numpy() @ comps + mean
        assert all(np.abs(back[b, 3 * b: 3 * b + 3]).max() < 1e-5 for b in range(B)) and np.abs(back).max() > 1.0
    else:
        raise AssertionError(case)
    return betas, pose, go, tr


@gpu
@pytest.mark.parametrize("case", ("zero", "1e-7", "1e-4", "large", "pi-and-7", "one-joint-zero"))
def test_edge_poses(models, case):
    for flat in (True, False):
        betas, pose, go, tr = _edge_inputs(case, models["real"], flat)
        out = _layer(models, "real", flat)(betas=betas.to(DEV), global_orient=go.to(DEV), hand_pose=pose.to(DEV), transl=tr.to(DEV))
        _compare(f"edge {case}", models, "real", flat, betas, pose, go, tr, out.vertices, out.joints)


@gpu
@pytest.mark.parametrize("B", (1, 5))
def test_optional_arguments_equal_explicit_zeros(models, B):
    p = _layer(models, "real", False)._packed
    betas, pose, go, tr = (t.to(DEV) for t in _inputs(B, f"opt/{B}"))
    z = torch.zeros(B, 3, device=DEV)
    for cmaj in (False, True):
        f = lambda g, t, j=True: ops.mano_forward(p, betas, pose, g, t, channel_major=cmaj, want_joints=j)
        for (g0, t0), (g1, t1) in (((None, tr), (z, tr)), ((go, None), (go, z)), ((None, None), (z, z))):
            v0, j0 = f(g0, t0)
            v1, j1 = f(g1, t1)
            assert torch.equal(v0, v1) and torch.equal(j0, j1), (cmaj, g0 is None, t0 is None)
        vj, _ = f(go, tr)
        v = f(go, tr, False)
        assert torch.is_tensor(v) and torch.equal(v, vj)                # the vertices do not depend on whether joints are written
        assert torch.equal(f(None, None, False), f(z, z)[0])


@gpu
@pytest.mark.parametrize("B", (1, 5))
def test_strided_inputs_equal_contiguous_copies(models, B):
    """generate.py hands the layer column slices of its [B,61] rows, GenNet.gen slices of recon [B,55]: ldb / ldp / ldg / ldt
    are then the row strides of the wide tensor."""
    layer = _layer(models, "real", False)
    p = layer._packed
    row = synth.synthetic_normal((B, 61), 61, f"tmano/strided61/{B}", 0.7).to(DEV)
    betas, go, pose, tr = row[:, :10], row[:, 10:13], row[:, 13:58], row[:, 58:]
    assert not pose.is_contiguous() or B == 1
    for cmaj in (False, True):
        v, j = ops.mano_forward(p, betas, pose, go, tr, channel_major=cmaj, want_joints=True)
        vc, jc = ops.mano_forward(p, betas.contiguous(), pose.contiguous(), go.contiguous(), tr.contiguous(), channel_major=cmaj,
                                  want_joints=True)
        assert torch.equal(v, vc) and torch.equal(j, jc), cmaj
    _compare(f"strided [B,61] B={B}", models, "real", False, betas.cpu(), pose.cpu(), go.cpu(), tr.cpu(), vc.permute(0, 2, 1), jc)
    recon = synth.synthetic_normal((B, 55), 61, f"tmano/strided55/{B}", 0.7).to(DEV)
    cm = layer.vertices_channel_major(recon[:, :10], recon[:, 10:55])
    assert torch.equal(cm, layer.vertices_channel_major(recon[:, :10].contiguous(), recon[:, 10:55].contiguous()))
    _compare(f"strided [B,55] B={B}", models, "real", False, recon[:, :10].cpu(), recon[:, 10:55].cpu(), None, None, cm, cm=True)
    wide = torch.zeros(B, 90, device=DEV)
    for bad in ((wide[:, 0:20:2], pose), (betas, wide[:, 0:90:2])):     # right shapes, column stride 2
        with pytest.raises(RuntimeError):
            ops.mano_forward(p, *bad)
    with pytest.raises(RuntimeError):
        ops.mano_forward(p, betas, pose, wide[:, 0:6:2], None)
    with pytest.raises(RuntimeError):
        ops.mano_forward(p, betas, pose, None, wide[:, 0:6:2])


@gpu
def test_rows_do_not_depend_on_the_batch(models):
    """Both MANO kernels are per sample and the GEMM's accumulation order does not depend on the M tiling: a row of a batch of
    257 has the bits of the same row computed alone, and of the same row at another position of a batch of 6."""
    p = _layer(models, "real", False)._packed
    betas, pose, go, tr = (t.to(DEV) for t in _inputs(257, "rows"))
    for cmaj in (False, True):
        f = lambda s: ops.mano_forward(p, betas[s], pose[s], go[s], tr[s], channel_major=cmaj, want_joints=True)
        V, J = f(slice(None))
        for i in (0, 3, 4, 255, 256):
            v1, j1 = f(slice(i, i + 1))
            assert torch.equal(v1[0], V[i]) and torch.equal(j1[0], J[i]), f"row {i} alone differs (channel_major={cmaj})"
            idx = torch.tensor([100, 7, i, 200, 31, 64], device=DEV)
            v6, j6 = f(idx)
            assert torch.equal(v6[2], V[i]) and torch.equal(j6[2], J[i]), f"row {i} inside a batch of 6 differs (channel_major={cmaj})"


@gpu
def test_chunk_boundary(models):
    """B = 16384 + 3: the second pass of dvq_mano_forward's chunk loop (offsets b0*ldb, b0*48, b0*778*3).  64 distinct rows tiled;
    beyond the boundary the tiling is shifted by 29, so no row of the second chunk equals the row 16384 places before it."""
    CH = 16384
    B = CH + 3
    p = _layer(models, "real", False)._packed
    src = [t.to(DEV) for t in _inputs(64, "chunk")]
    idx = torch.arange(B, device=DEV) % 64
    idx[CH:] = (idx[CH:] + 29) % 64
    rows = torch.tensor([0, CH - 1, CH, CH + 2], device=DEV)
    assert len(set(idx[rows].tolist())) == 4 and int(idx[CH]) != int(idx[0])
    betas, pose, go, tr = (t[idx].contiguous() for t in src)
    small = [t[rows].contiguous() for t in (betas, pose, go, tr)]
    for cmaj in (False, True):
        V, J = ops.mano_forward(p, betas, pose, go, tr, channel_major=cmaj, want_joints=True)
        v4, j4 = ops.mano_forward(p, *small, channel_major=cmaj, want_joints=True)
        assert torch.equal(V[rows], v4) and torch.equal(J[rows], j4), f"rows at the chunk boundary differ (channel_major={cmaj})"
        assert bool(torch.isfinite(V).all())
        _compare(f"chunk boundary rows cm={cmaj}", models, "real", False, *(t.cpu() for t in small), V[rows], J[rows], cm=cmaj)
        del V, J, v4, j4
    del betas, pose, go, tr
    ops.release_workspaces()
    torch.cuda.empty_cache()


@gpu
def test_a_non_finite_row_stays_in_its_row(models):
    p = _layer(models, "real", False)._packed
    betas, pose, go, tr = (t.to(DEV) for t in _inputs(9, "nan"))
    bad = betas.clone()
    bad[4, 2] = float("nan")
    keep = torch.tensor([0, 1, 2, 3, 5, 6, 7, 8], device=DEV)
    with ops.no_range_check():
        v0, j0 = ops.mano_forward(p, betas, pose, go, tr, want_joints=True)
        v1, j1 = ops.mano_forward(p, bad, pose, go, tr, want_joints=True)
    assert torch.equal(v0[keep], v1[keep]) and torch.equal(j0[keep], j1[keep])
    assert not bool(torch.isfinite(v1[4]).any()) and not bool(torch.isfinite(j1[4]).any())
    # with the range check on, the default fp16 image's fallback runs the batch again on the six-product images
    v2, j2 = ops.mano_forward(p, bad, pose, go, tr, want_joints=True)
    assert not bool(torch.isfinite(v2[4]).any()) and bool(torch.isfinite(v2[keep]).all()) and bool(torch.isfinite(j2[keep]).all())
    k = keep.cpu()
    _compare("beside a NaN row", models, "real", False, betas.cpu()[k], pose.cpu()[k], go.cpu()[k], tr.cpu()[k], v2[keep], j2[keep])
    v3, j3 = ops.mano_forward(p, betas, pose, go, tr, want_joints=True)  # and the default images are back afterwards
    assert torch.equal(v3, v0) and torch.equal(j3, j0)


def _parity_matrix_in_a_child(kind):
    env = dict(os.environ, DVQ_GEMM=kind)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k", "test_parity_matrix",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("mano-ratio-worst")))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout and f"mano-ratio-worst {kind} " in r.stdout


@gpu
def test_fp32_gemm_branch_parity():
    """DVQ_GEMM=fp32 is chosen when the library loads: a fresh process runs test_parity_matrix on the fp32 matrix-core GEMM."""
    _parity_matrix_in_a_child("fp32")


@gpu
def test_bf16x3_gemm_branch_parity():
    """DVQ_GEMM=bf16x3: the blendshape image is the exact three-plane bf16 split (what the fp16 default falls back to)."""
    _parity_matrix_in_a_child("bf16x3")


def _abi_call(struct, B, betas, ldb, pose, ldp, verts, layout, ws, ws_bytes):
    return _lib.load().dvq_mano_forward(C.byref(struct), betas.data_ptr(), ldb, pose.data_ptr(), ldp, None, 0, None, 0, B,
                                        verts.data_ptr(), layout, None, ws.data_ptr(), ws_bytes,
                                        torch.cuda.current_stream().cuda_stream)


@gpu
def test_refusals(models):
    """Every refused call is an error return with valid device pointers behind it, never a launch."""
    lib = _lib.load()
    p = _layer(models, "real", True)._packed
    B = 3
    betas, pose, go, tr = (t.to(DEV) for t in _inputs(B, "refuse"))
    good = ops.mano_forward(p, betas, pose, go, tr)
    # through the wrapper
    with pytest.raises(RuntimeError):
        ops.mano_forward(p, betas[:, :9].contiguous(), pose)
    with pytest.raises(RuntimeError):
        ops.mano_forward(p, betas, torch.cat([pose, pose[:1]]))
    with pytest.raises(RuntimeError):
        ops.mano_forward(p, betas.cpu(), pose.cpu())
    with pytest.raises(RuntimeError):
        ops.mano_forward(p, betas, pose, go.cpu(), None)
    with pytest.raises(RuntimeError):
        ops.mano_forward(p, betas.double(), pose)
    for bad in (go[:, :2].contiguous(), torch.cat([go, go[:1]]), torch.zeros(B, 4, device=DEV), go[0]):
        with pytest.raises(RuntimeError):                               # the kernels read three floats per row of these
            ops.mano_forward(p, betas, pose, bad, None)
        with pytest.raises(RuntimeError):
            ops.mano_forward(p, betas, pose, None, bad)
    # through the ABI
    nws = lib.dvq_mano_workspace_bytes(B)
    ws = torch.empty(nws + 256, dtype=torch.uint8, device=DEV)
    verts = torch.full((B, 778, 3), -7.0, device=DEV)
    with torch.cuda.device(DEV):
        assert _abi_call(p.cstruct, B, betas, 10, pose, 45, verts, 0, ws, nws) == 0
        torch.cuda.synchronize()
        assert torch.equal(verts, ops.mano_forward(p, betas, pose))
        verts.fill_(-7.0)
        EINVAL, EWORKSPACE = 1, 2
        assert _abi_call(p.cstruct, B, betas, 9, pose, 45, verts, 0, ws, nws) == EINVAL              # betas rows of 9
        assert _abi_call(p.cstruct, B, betas, 10, pose, 44, verts, 0, ws, nws) == EINVAL             # pose rows of 44
        assert _abi_call(p.cstruct, B, betas, 10, pose, 45, verts, 2, ws, nws) == EINVAL and b"layout" in lib.dvq_last_error()
        assert _abi_call(p.cstruct, -1, betas, 10, pose, 45, verts, 0, ws, nws) == EINVAL
        assert _abi_call(p.cstruct, B, betas, 10, pose, 45, verts, 0, ws, nws - 1) == EWORKSPACE and b"workspace" in lib.dvq_last_error()
        for j, bad in ((3, 3), (5, 9), (0, 0), (15, 16)):
            s = _lib.ManoModel.from_buffer_copy(p.cstruct)                                           # never the shared struct
            s.parents[j] = bad
            assert _abi_call(s, B, betas, 10, pose, 45, verts, 0, ws, nws) == EINVAL and b"parents" in lib.dvq_last_error(), (j, bad)
        assert p.cstruct.parents[3] == 2
        torch.cuda.synchronize()
    assert bool((verts == -7.0).all())                                  # nothing was launched
    assert torch.equal(ops.mano_forward(p, betas, pose, go, tr), good)  # and the library still works
    # B = 0: empty results of the right shape
    e = lambda n: torch.empty(0, n, device=DEV)
    v, j = ops.mano_forward(p, e(10), e(45), e(3), e(3), want_joints=True)
    assert tuple(v.shape) == (0, 778, 3) and tuple(j.shape) == (0, 16, 3) and v.dtype == torch.float32 and v.device.type == "cuda"
    assert tuple(ops.mano_forward(p, e(10), e(45), channel_major=True).shape) == (0, 3, 778)
    out = _layer(models, "real", True)(betas=e(10), global_orient=e(3), hand_pose=e(45), transl=e(3))
    assert tuple(out.vertices.shape) == (0, 778, 3) and tuple(out.joints.shape) == (0, 16, 3)
