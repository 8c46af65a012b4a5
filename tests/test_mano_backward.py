"""The MANO layer's backward pass (csrc/mano_grad.hip, ops.mano_backward, the autograd Function of mano.ManoLayer) against
autograd through tests/mano_grad_ref.py, a torch restatement of tests/mano_ref.py.

CPU group (unmarked): the restatement's float64 forward is pinned to mano_ref, its float64 gradient to central differences of
mano_ref (a numpy path that shares no code with it), the packed ``blend_wt`` to ``blend_w``, and the layer's dispatch is checked
with the two ops replaced by recording stubs.  GPU group (``gpu`` marker): the kernels against the float64 gradient.

Tolerance of every device comparison, in the method of tests/test_mano.py: ``e32`` is the max-abs error of the float32 CPU
restatement's gradient against the float64 one, per output tensor over the POOLED rows of a test (all batches of a parity-matrix
variant, the eight rows of an edge case); the device must be within ``8 * e32``.  e32 comes from the reference side only.  Each
comparison prints a ``mano-grad-ratio`` line (device error / e32); DESIGN.md records the worst per output."""
import ctypes as C
import lzma
import os

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, ops, packing, synth
from dvqvae_amd import mano as dmano

import mano_ref as ref
import mano_grad_ref as gref

DEV = "cuda:0"
gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = ("real", "synthetic")
FACTOR = 8.0
NAMES = ("betas", "pose", "orient", "transl")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    """{"real": arrays of the committed MANO_RIGHT.pkl, "synthetic": synthetic_mano_arrays()} (float64 as stored)."""
    path = str(tmp_path_factory.mktemp("mano") / "MANO_RIGHT.pkl")
    with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
        out.write(lzma.decompress(f.read()))
    return {"real": dmano.read_mano_pkl(path), "synthetic": dmano.synthetic_mano_arrays()}


def _inputs(B, tag, pose_scale=0.8, betas_scale=1.0, go_scale=1.0, tr_scale=0.3):
    return (synth.synthetic_normal((B, 10), 61, f"tmanograd/{tag}/betas", betas_scale),
            synth.synthetic_normal((B, 45), 61, f"tmanograd/{tag}/pose", pose_scale),
            synth.synthetic_normal((B, 3), 61, f"tmanograd/{tag}/go", go_scale),
            synth.synthetic_normal((B, 3), 61, f"tmanograd/{tag}/tr", tr_scale))


def _upstream(B, tag):
    return (synth.synthetic_normal((B, 778, 3), 61, f"tmanograd/{tag}/gv", 1.0),
            synth.synthetic_normal((B, 16, 3), 61, f"tmanograd/{tag}/gj", 1.0))


_restatements = {}


def _restatement(models, model, flat, dtype):
    key = (model, flat, dtype)
    if key not in _restatements:
        _restatements[key] = gref.ManoTorch(ref.device_arrays(models[model]), flat_hand_mean=flat, dtype=dtype)
    return _restatements[key]


# ========================================================================================== CPU group
@pytest.mark.parametrize("flat", (True, False))
@pytest.mark.parametrize("model", MODELS)
def test_f64_forward_equals_mano_ref(models, model, flat):
    a = ref.device_arrays(models[model])
    betas, pose, go, tr = _inputs(6, "fwd")
    m = _restatement(models, model, flat, torch.float64)
    with torch.no_grad():
        v, j = m(*(t.double() for t in (betas, pose, go, tr)))
        v0, j0 = m(betas.double(), pose.double())
    rv, rj = ref.mano_ref(a, betas, pose, go, tr, flat_hand_mean=flat)
    rv0, rj0 = ref.mano_ref(a, betas, pose, flat_hand_mean=flat)
    assert np.abs(v.numpy() - rv).max() <= 1e-12 and np.abs(j.numpy() - rj).max() <= 1e-12
    assert np.abs(v0.numpy() - rv0).max() <= 1e-12 and np.abs(j0.numpy() - rj0).max() <= 1e-12


@pytest.mark.parametrize("flat", (True, False))
@pytest.mark.parametrize("model", MODELS)
def test_f64_vjp_equals_central_differences(models, model, flat):
    """d/dx of <verts, gv> + <joints, gj> by central differences (h = 1e-5) of mano_ref.mano_ref, every one of the 61 inputs of
    each of two rows (the rows are independent, so column k of both rows moves in one evaluation).  Truncation h^2 f''' / 6 and
    rounding 2^-52 |loss| / h are both below 1e-8 here; the bound is 1e-7 * max(1, max|grad|)."""
    a = ref.device_arrays(models[model])
    B, h = 2, 1e-5
    ins = [t.double().numpy() for t in _inputs(B, "fd")]
    gv, gj = (t.double().numpy() for t in _upstream(B, "fd"))
    got = _restatement(models, model, flat, torch.float64).vjp(*ins, gv, gj)

    def loss_rows(x):
        v, j = ref.mano_ref(a, x[0], x[1], x[2], x[3], flat_hand_mean=flat)
        return (v * gv).sum((1, 2)) + (j * gj).sum((1, 2))

    for i, name in enumerate(NAMES):
        fd = np.zeros_like(ins[i])
        for k in range(ins[i].shape[1]):
            hi, lo = [x.copy() for x in ins], [x.copy() for x in ins]
            hi[i][:, k] += h
            lo[i][:, k] -= h
            fd[:, k] = (loss_rows(hi) - loss_rows(lo)) / (2 * h)
        err, mag = np.abs(got[i] - fd).max(), np.abs(fd).max()
        print(f"mano-grad-fd {model} flat={flat} {name}: {err:.2e} on {mag:.2e}")
        assert mag > 0 and err <= 1e-7 * max(1.0, mag), (name, err, mag)


@pytest.mark.parametrize("model", MODELS)
def test_blend_wt_is_blend_w_transposed(models, model):
    t = packing.PackedMano(models[model], flat_hand_mean=False).tensors
    assert sorted(t) == sorted(["v_template", "blend_w", "blend_wt", "j_template", "j_shapedirs", "weights", "comps", "pose_mean"])
    bw, bt = t["blend_w"], t["blend_wt"]
    assert tuple(bw.shape) == (2334, 160) and tuple(bt.shape) == (160, 2336) and bt.dtype == torch.float32 and bt.is_contiguous()
    assert torch.equal(bt[:, :2334], bw.T) and not bool(bt[:, 2334:].any()) and not bool(bt[145:].any())
    # the forward's operand is what it was: [shapedirs | posedirs | 0] rounded once
    a = models[model]
    blend = np.zeros((2334, 160))
    blend[:, :10] = np.asarray(a["shapedirs"], np.float64)[:, :, :10].reshape(2334, 10)
    blend[:, 10:145] = np.asarray(a["posedirs"], np.float64).reshape(2334, 135)
    assert np.array_equal(bw.numpy(), blend.astype(np.float32))


def test_layer_dispatch_needs_no_device(models, monkeypatch):
    """With no input requiring grad, or under torch.no_grad(), ManoLayer calls ops.mano_forward exactly as before and never the
    autograd Function; with grad wanted the Function calls the two ops and hands back gradients for the inputs that want them."""
    layer = dmano.ManoLayer(models["synthetic"])
    calls = []

    def fwd(packed, betas, hand_pose, global_orient=None, transl=None, channel_major=False, want_joints=False):
        calls.append(("fwd", packed, betas, hand_pose, global_orient, transl, channel_major, want_joints))
        B = betas.shape[0]
        v = torch.zeros((B, 3, 778) if channel_major else (B, 778, 3))
        return (v, torch.zeros(B, 16, 3)) if want_joints else v

    def bwd(packed, betas, hand_pose, global_orient=None, transl=None, grad_verts=None, grad_joints=None, channel_major=False,
            needs=(True, True, True, True)):
        calls.append(("bwd", packed, betas, hand_pose, global_orient, transl, grad_verts, grad_joints, channel_major, tuple(needs)))
        B = betas.shape[0]
        return tuple(torch.full((B, n), float(i + 1)) if need else None for i, (n, need) in enumerate(zip((10, 45, 3, 3), needs)))

    monkeypatch.setattr(ops, "mano_forward", fwd)
    monkeypatch.setattr(ops, "mano_backward", bwd)
    real_apply = dmano._ManoFunction.apply
    applied = []
    monkeypatch.setattr(dmano._ManoFunction, "apply", staticmethod(lambda *a: (applied.append(a), real_apply(*a))[1]))
    betas, pose, go, tr = _inputs(3, "dispatch")
    # no input requires grad
    out = layer(betas=betas, global_orient=go, hand_pose=pose, transl=tr)
    assert not applied and len(calls) == 1 and calls[0][0] == "fwd" and calls[0][1] is layer._packed
    assert all(torch.equal(x, y) for x, y in zip(calls[0][2:6], (betas, pose, go, tr))) and calls[0][6:] == (False, True)
    assert out.vertices.grad_fn is None and out.joints.grad_fn is None
    layer(betas=betas, hand_pose=pose)
    assert not applied and calls[1][4] is None and calls[1][5] is None
    layer.vertices_channel_major(betas, pose)
    assert not applied and calls[2][0] == "fwd" and calls[2][6:] == (True, False)
    # requires grad, but under no_grad
    rb, rp = betas.clone().requires_grad_(True), pose.clone().requires_grad_(True)
    with torch.no_grad():
        out = layer(betas=rb, global_orient=go, hand_pose=rp, transl=tr)
        layer.vertices_channel_major(rb, rp)
    assert not applied and len(calls) == 5 and all(c[0] == "fwd" for c in calls) and out.vertices.grad_fn is None
    # grad wanted: through the Function; gradients only where they are required
    out = layer(betas=rb, global_orient=go, hand_pose=rp, transl=None)
    assert len(applied) == 1 and len(calls) == 6 and calls[5][0] == "fwd" and calls[5][5] is None and calls[5][6:] == (False, True)
    assert out.vertices.grad_fn is not None and out.joints.grad_fn is not None
    gv, gj = _upstream(3, "dispatch")
    ((out.vertices * gv).sum() + (out.joints * gj).sum()).backward()
    assert len(calls) == 7 and calls[6][0] == "bwd" and calls[6][9] == (True, True, False, False) and calls[6][8] is False
    assert torch.equal(calls[6][6], gv) and torch.equal(calls[6][7], gj) and calls[6][5] is None and torch.equal(calls[6][4], go)
    assert torch.equal(rb.grad, torch.full((3, 10), 1.0)) and torch.equal(rp.grad, torch.full((3, 45), 2.0))
    cm = layer.vertices_channel_major(rb, rp)
    cm.sum().backward()
    assert len(applied) == 2 and calls[8][0] == "bwd" and calls[8][8] is True and calls[8][7] is None and tuple(calls[8][6].shape) == (3, 3, 778)
    out = layer(betas=rb, hand_pose=rp)
    g, = torch.autograd.grad(out.vertices.sum(), rb, create_graph=True)
    with pytest.raises(RuntimeError):                                   # once_differentiable: the gradient cannot be differentiated again
        g.sum().backward()


# ========================================================================================== GPU group
_layers = {}


def _layer(models, model, flat):
    key = (model, flat, packing.gemm_kind())
    if key not in _layers:
        _layers[key] = dmano.ManoLayer(models[model], flat_hand_mean=flat).to(DEV)
    return _layers[key]


def _device_grads(packed, ins, gv, gj, cm=False):
    d = lambda t: None if t is None else t.contiguous().to(DEV)         # (the one-joint-zero case builds its pose transposed)
    gvd = None if gv is None else (gv.permute(0, 2, 1).contiguous() if cm else gv).to(DEV)
    return ops.mano_backward(packed, *(d(t) for t in ins), grad_verts=gvd, grad_joints=d(gj), channel_major=cm)


class _Pool:
    """Device gradients of one test against the float64 gradient: e32 per output over ALL rows handed to ``reference``, then every
    recorded device error against FACTOR * e32."""

    def __init__(self, models, model, flat, what):
        self.m64 = _restatement(models, model, flat, torch.float64)
        self.m32 = _restatement(models, model, flat, torch.float32)
        self.what, self.e32, self.mag, self.cases, self.r64 = f"{model} flat={flat} {what}", None, None, [], None

    def reference(self, ins, gv, gj):
        """float64 gradients of the pooled rows (kept: ``check`` slices them) and e32 over them."""
        self.r64 = self.m64.vjp(*ins, gv, gj)
        r32 = self.m32.vjp(*ins, gv, gj)
        self.e32 = [float(np.abs(a - b).max()) for a, b in zip(r32, self.r64)]
        self.mag = [float(np.abs(b).max()) for b in self.r64]
        return self.r64

    def check(self, label, got, rows):
        err = [float(np.abs(g.detach().cpu().double().numpy() - r[rows]).max()) for g, r in zip(got, self.r64)]
        self.cases.append((label, err))

    def finish(self):
        assert self.e32 is not None and all(e > 0 for e in self.e32), self.e32
        worst = [0.0] * 4
        for label, err in self.cases:
            ratio = [d / e for d, e in zip(err, self.e32)]
            worst = [max(a, b) for a, b in zip(worst, ratio)]
            print(f"mano-grad-ratio {self.what} {label}: " + "; ".join(f"{n} {d:.3e} / e32 {e:.3e} = {r:.2f}" for n, d, e, r in zip(NAMES, err, self.e32, ratio)))
        print(f"mano-grad-ratio-worst {self.what}: " + " ".join(f"{n} {r:.2f}" for n, r in zip(NAMES, worst))
              + "; |grad| " + " ".join(f"{m:.2g}" for m in self.mag))
        for label, err in self.cases:
            for n, d, e in zip(NAMES, err, self.e32):
                assert np.isfinite(d) and d <= FACTOR * e, f"{self.what} {label}: grad {n} differs from the float64 gradient by {d:.3e} > {FACTOR:g} x e32 = {FACTOR * e:.3e}"
        return worst


BATCHES = (1, 3, 4, 5, 65, 129, 257)   # one live wave beside three dead ones, a full pose block, a ragged last block, a second GEMM row tile


@gpu
@pytest.mark.parametrize("flat", (True, False))
@pytest.mark.parametrize("model", MODELS)
def test_parity_matrix(models, model, flat):
    packed = _layer(models, model, flat)._packed
    parts = [(_inputs(B, f"matrix/{model}/{flat}/{B}"), _upstream(B, f"matrix/{model}/{flat}/{B}")) for B in BATCHES]
    ins = [torch.cat([p[0][i] for p in parts]) for i in range(4)]
    gv, gj = torch.cat([p[1][0] for p in parts]), torch.cat([p[1][1] for p in parts])
    offs = np.concatenate([[0], np.cumsum(BATCHES)])
    for variant, ugv, ugj in (("verts+joints", gv, gj), ("verts", gv, None), ("joints", None, gj)):
        pool = _Pool(models, model, flat, variant)
        pool.reference(ins, ugv, ugj)
        for k, B in enumerate(BATCHES):
            rows = slice(int(offs[k]), int(offs[k + 1]))
            sub = [t[rows] for t in ins]
            for cm in ((False, True) if ugv is not None else (False,)):
                got = _device_grads(packed, sub, None if ugv is None else ugv[rows], None if ugj is None else ugj[rows], cm)
                assert [tuple(g.shape) for g in got] == [(B, 10), (B, 45), (B, 3), (B, 3)]
                pool.check(f"B={B}" + (" channel-major" if cm else ""), got, rows)
        pool.finish()


def _edge_inputs(case, arrays, flat):
    """The cases of tests/test_mano.py::test_edge_poses, restated."""
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
        target = synth.synthetic_normal((B, 45), 61, "tmanograd/edge/target", 1.5).double().numpy()
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
    gv, gj = _upstream(8, f"edge/{case}")
    for flat in (True, False):
        ins = _edge_inputs(case, models["real"], flat)
        pool = _Pool(models, "real", flat, f"edge {case}")
        pool.reference(ins, gv, gj)
        pool.check("B=8", _device_grads(_layer(models, "real", flat)._packed, ins, gv, gj), slice(None))
        pool.finish()


@gpu
def test_through_autograd(models):
    layer = _layer(models, "real", False)
    p = layer._packed
    B = 5
    ins = [t.to(DEV) for t in _inputs(B, "autograd")]
    gv, gj = (t.to(DEV) for t in _upstream(B, "autograd"))
    want = ops.mano_backward(p, *ins, grad_verts=gv, grad_joints=gj)

    def run(betas, go, pose, tr):
        out = layer(betas=betas, global_orient=go, hand_pose=pose, transl=tr)
        assert out.vertices.grad_fn is not None and out.joints.grad_fn is not None
        ((out.vertices * gv).sum() + (out.joints * gj).sum()).backward()
        return out

    leaf = [t.clone().requires_grad_(True) for t in ins]
    out = run(leaf[0], leaf[2], leaf[1], leaf[3])
    v0, j0 = ops.mano_forward(p, *ins, want_joints=True)
    assert torch.equal(out.vertices.detach(), v0) and torch.equal(out.joints.detach(), j0)
    for x, w, n in zip(leaf, want, NAMES):
        assert x.grad is not None and torch.equal(x.grad, w), n
    # an input that does not require grad gets none; the others get the same bits
    leaf = [t.clone().requires_grad_(i in (1, 3)) for i, t in enumerate(ins)]
    run(leaf[0], leaf[2], leaf[1], leaf[3])
    assert leaf[0].grad is None and leaf[2].grad is None
    assert torch.equal(leaf[1].grad, want[1]) and torch.equal(leaf[3].grad, want[3])
    # vertices alone, joints alone: what ops.mano_backward gives for that upstream gradient
    for use_v, use_j in ((True, False), (False, True)):
        leaf = [t.clone().requires_grad_(True) for t in ins]
        out = layer(betas=leaf[0], global_orient=leaf[2], hand_pose=leaf[1], transl=leaf[3])
        ((out.vertices * gv).sum() if use_v else (out.joints * gj).sum()).backward()
        w1 = ops.mano_backward(p, *ins, grad_verts=gv if use_v else None, grad_joints=gj if use_j else None)
        assert all(torch.equal(x.grad, w) for x, w in zip(leaf, w1)), (use_v, use_j)
    # global_orient=None / transl=None: the bits of explicit zeros
    z = torch.zeros(B, 3, device=DEV)
    for g, t in ((None, ins[3]), (ins[2], None), (None, None)):
        wz = ops.mano_backward(p, ins[0], ins[1], z if g is None else g, z if t is None else t, grad_verts=gv, grad_joints=gj)
        got = ops.mano_backward(p, ins[0], ins[1], g, t, grad_verts=gv, grad_joints=gj)
        assert all(torch.equal(a, b) for a, b in zip(got, wz)), (g is None, t is None)
        lb, lp = ins[0].clone().requires_grad_(True), ins[1].clone().requires_grad_(True)
        run(lb, g, lp, t)
        assert torch.equal(lb.grad, wz[0]) and torch.equal(lp.grad, wz[1])
    # channel-major vertices of the PointNet path
    lb, lp = ins[0].clone().requires_grad_(True), ins[1].clone().requires_grad_(True)
    cm = layer.vertices_channel_major(lb, lp)
    assert tuple(cm.shape) == (B, 3, 778) and cm.grad_fn is not None
    gcm = gv.permute(0, 2, 1).contiguous()
    (cm * gcm).sum().backward()
    wc = ops.mano_backward(p, ins[0], ins[1], grad_verts=gcm, channel_major=True, needs=(True, True, False, False))
    assert wc[2] is None and wc[3] is None and torch.equal(lb.grad, wc[0]) and torch.equal(lp.grad, wc[1])
    # strided column slices of a [B,61] row: the bits of contiguous copies, and row.grad in the right columns
    row = synth.synthetic_normal((B, 61), 61, "tmanograd/strided61", 0.7).to(DEV).requires_grad_(True)
    betas, go, pose, tr = row[:, :10], row[:, 10:13], row[:, 13:58], row[:, 58:]
    assert not pose.is_contiguous()
    run(betas, go, pose, tr)
    d = row.detach()
    ws = ops.mano_backward(p, d[:, :10], d[:, 13:58], d[:, 10:13], d[:, 58:], grad_verts=gv, grad_joints=gj)
    wc = ops.mano_backward(p, d[:, :10].contiguous(), d[:, 13:58].contiguous(), d[:, 10:13].contiguous(), d[:, 58:].contiguous(),
                           grad_verts=gv, grad_joints=gj)
    assert all(torch.equal(a, b) for a, b in zip(ws, wc))
    assert torch.equal(row.grad, torch.cat([wc[0], wc[2], wc[1], wc[3]], dim=1))


@gpu
def test_no_grad_path_is_unchanged(models):
    layer = _layer(models, "real", False)
    ins = [t.to(DEV) for t in _inputs(5, "nograd")]
    v0, j0 = ops.mano_forward(layer._packed, *ins, want_joints=True)
    out = layer(betas=ins[0], global_orient=ins[2], hand_pose=ins[1], transl=ins[3])
    assert torch.equal(out.vertices, v0) and torch.equal(out.joints, j0) and out.vertices.grad_fn is None and out.joints.grad_fn is None
    req = [t.clone().requires_grad_(True) for t in ins]
    with torch.no_grad():
        out = layer(betas=req[0], global_orient=req[2], hand_pose=req[1], transl=req[3])
        cm = layer.vertices_channel_major(req[0], req[1])
    assert torch.equal(out.vertices, v0) and torch.equal(out.joints, j0) and out.vertices.grad_fn is None and not out.vertices.requires_grad
    assert torch.equal(cm, ops.mano_forward(layer._packed, ins[0], ins[1], channel_major=True)) and cm.grad_fn is None


@gpu
def test_rows_do_not_depend_on_the_batch(models):
    """Both backward kernels are per sample and the GEMM's accumulation order does not depend on the M tiling: a row's gradient in
    a batch of 257 has the bits of the same row computed alone, and at another position of a batch of 6."""
    p = _layer(models, "real", False)._packed
    ins = [t.to(DEV) for t in _inputs(257, "rows")]
    gv, gj = (t.to(DEV) for t in _upstream(257, "rows"))
    for cm in (False, True):
        g = gv.permute(0, 2, 1).contiguous() if cm else gv
        f = lambda s: ops.mano_backward(p, *(t[s] for t in ins), grad_verts=g[s], grad_joints=gj[s], channel_major=cm)
        full = f(slice(None))
        for i in (0, 3, 4, 255, 256):
            one = f(slice(i, i + 1))
            six = f(torch.tensor([100, 7, i, 200, 31, 64], device=DEV))
            for n, a, b, c in zip(NAMES, full, one, six):
                assert torch.equal(b[0], a[i]), f"grad {n} of row {i} alone differs (channel_major={cm})"
                assert torch.equal(c[2], a[i]), f"grad {n} of row {i} inside a batch of 6 differs (channel_major={cm})"


@gpu
def test_chunk_boundary(models):
    """B = 16384 + 3: the second pass of dvq_mano_backward's chunk loop.  64 distinct rows tiled; beyond the boundary the tiling is
    shifted by 29, so no row of the second chunk equals the row 16384 places before it."""
    CH = 16384
    B = CH + 3
    p = _layer(models, "real", False)._packed
    src = [t.to(DEV) for t in _inputs(64, "chunk") + _upstream(64, "chunk")]
    idx = torch.arange(B, device=DEV) % 64
    idx[CH:] = (idx[CH:] + 29) % 64
    rows = torch.tensor([0, CH - 1, CH, CH + 2], device=DEV)
    assert len(set(idx[rows].tolist())) == 4 and int(idx[CH]) != int(idx[0])
    betas, pose, go, tr, gv, gj = (t[idx].contiguous() for t in src)
    small = [t[rows].contiguous() for t in (betas, pose, go, tr, gv, gj)]
    full = ops.mano_backward(p, betas, pose, go, tr, grad_verts=gv, grad_joints=gj)
    four = ops.mano_backward(p, *small[:4], grad_verts=small[4], grad_joints=small[5])
    for n, a, b in zip(NAMES, full, four):
        assert tuple(a.shape)[0] == B and torch.equal(a[rows], b), f"grad {n}: rows at the chunk boundary differ"
        assert bool(torch.isfinite(a).all()), n
    pool = _Pool(models, "real", False, "chunk boundary rows")
    pool.reference([t.cpu() for t in src[:4]], src[4].cpu(), src[5].cpu())
    pool.check("B=16387", [a[rows] for a in full], idx[rows].cpu().numpy())
    pool.finish()
    del full, four, betas, pose, go, tr, gv, gj, small
    ops.release_workspaces()
    torch.cuda.empty_cache()


@gpu
@pytest.mark.parametrize("where", ("grad_verts", "betas"))
def test_a_non_finite_row_stays_in_its_row(models, where):
    p = _layer(models, "real", False)._packed
    ins = [t.to(DEV) for t in _inputs(9, "nan")]
    gv, gj = (t.to(DEV) for t in _upstream(9, "nan"))
    bad_ins, bad_gv = list(ins), gv
    if where == "grad_verts":
        bad_gv = gv.clone()
        bad_gv[4, 100, 1] = float("nan")
    else:
        bad_ins[0] = ins[0].clone()
        bad_ins[0][4, 2] = float("nan")
    keep = torch.tensor([0, 1, 2, 3, 5, 6, 7, 8], device=DEV)
    with ops.no_range_check():
        g0 = ops.mano_backward(p, *ins, grad_verts=gv, grad_joints=gj)
        g1 = ops.mano_backward(p, *bad_ins, grad_verts=bad_gv, grad_joints=gj)
    for n, a, b in zip(NAMES, g0, g1):
        assert torch.equal(a[keep], b[keep]), f"grad {n}: a row beside the non-finite one changed"
        assert bool(torch.isfinite(a).all())
    # row 4 itself: every gradient is linear in grad_verts; the vertices are linear in betas and transl, so a NaN in betas reaches
    # the gradients of the pose and the orientation (through V and the rest joints) and neither grad_betas nor grad_transl
    hit = (0, 1, 2, 3) if where == "grad_verts" else (1, 2)
    assert all(not bool(torch.isfinite(g1[k][4]).all()) for k in hit), "row 4 must hold a non-finite value"
    # with the range check on (the fp16 image's fallback runs the batch again), the other rows stay finite and right
    g2 = ops.mano_backward(p, *bad_ins, grad_verts=bad_gv, grad_joints=gj)
    assert all(bool(torch.isfinite(b[keep]).all()) for b in g2) and not bool(torch.isfinite(g2[1][4]).all())
    g3 = ops.mano_backward(p, *ins, grad_verts=gv, grad_joints=gj)        # and the default images are back afterwards
    assert all(torch.equal(a, b) for a, b in zip(g0, g3))


def _abi_call(struct, blend_wt, B, betas, ldb, pose, ldp, gv, layout, gj, outs, ws, ws_bytes):
    ptr = lambda t: None if t is None else t.data_ptr()
    return _lib.load().dvq_mano_backward(C.byref(struct), ptr(blend_wt), betas.data_ptr(), ldb, pose.data_ptr(), ldp, None, 0, None, 0, B,
                                         ptr(gv), layout, ptr(gj), *[ptr(o) for o in outs], ptr(ws), ws_bytes,
                                         torch.cuda.current_stream().cuda_stream)


@gpu
def test_refusals(models):
    """Every refused call is an error return with valid device pointers behind it, never a launch."""
    lib = _lib.load()
    p = _layer(models, "real", True)._packed
    B = 3
    betas, pose, go, tr = (t.to(DEV) for t in _inputs(B, "refuse"))
    gv, gj = (t.to(DEV) for t in _upstream(B, "refuse"))
    good = ops.mano_backward(p, betas, pose, go, tr, grad_verts=gv, grad_joints=gj)
    # through the wrapper
    bw = lambda *a, **k: ops.mano_backward(p, *a, **k)
    for bad in (lambda: bw(betas[:, :9].contiguous(), pose, grad_verts=gv),
                lambda: bw(betas, torch.cat([pose, pose[:1]]), grad_verts=gv),
                lambda: bw(betas.cpu(), pose.cpu(), grad_verts=gv.cpu()),
                lambda: bw(betas, pose, go, tr, grad_verts=gv.cpu()),
                lambda: bw(betas, pose, go.cpu(), None, grad_verts=gv),
                lambda: bw(betas.double(), pose, grad_verts=gv),
                lambda: bw(betas, pose, grad_verts=gv.double()),
                lambda: bw(betas, pose, grad_joints=gj.double()),
                lambda: bw(betas, pose, go[:, :2].contiguous(), None, grad_verts=gv),
                lambda: bw(betas, pose, None, torch.zeros(B, 4, device=DEV), grad_verts=gv),
                lambda: bw(betas, pose),                                                    # both upstream gradients missing
                lambda: bw(betas, pose, grad_verts=gv.permute(0, 2, 1).contiguous()),       # [B,3,778] without channel_major
                lambda: bw(betas, pose, grad_verts=gv, channel_major=True),
                lambda: bw(betas, pose, grad_verts=gv[:2]),
                lambda: bw(betas, pose, grad_joints=gj[:, :15].contiguous()),
                lambda: bw(betas, pose, grad_verts=gv, needs=(True, True, True))):
        with pytest.raises(RuntimeError):
            bad()
    # through the ABI
    bt = p.tensors["blend_wt"]
    nws = lib.dvq_mano_backward_workspace_bytes(B)
    assert nws >= B * (2 * (160 + 2336 + 192) + 3) * 4 and nws == lib.dvq_mano_backward_workspace_bytes(B)
    ws = torch.empty(nws + 256, dtype=torch.uint8, device=DEV)
    outs = [torch.full((B, n), -7.0, device=DEV) for n in (10, 45, 3, 3)]
    with torch.cuda.device(DEV):
        assert _abi_call(p.cstruct, bt, B, betas, 10, pose, 45, gv, 0, gj, outs, ws, nws) == 0
        torch.cuda.synchronize()
        want = ops.mano_backward(p, betas, pose, grad_verts=gv, grad_joints=gj)
        assert all(torch.equal(a, b) for a, b in zip(outs, want))
        only = [outs[0], None, None, outs[3]]                                                        # null outputs: not wanted
        assert _abi_call(p.cstruct, bt, B, betas, 10, pose, 45, gv, 0, None, only, ws, nws) == 0
        torch.cuda.synchronize()
        w2 = ops.mano_backward(p, betas, pose, grad_verts=gv, needs=(True, False, False, True))
        assert w2[1] is None and w2[2] is None and torch.equal(outs[0], w2[0]) and torch.equal(outs[3], w2[3])
        assert torch.equal(outs[1], want[1]) and torch.equal(outs[2], want[2])                       # ... and not written
        for o in outs:
            o.fill_(-7.0)
        EINVAL, EWORKSPACE = 1, 2
        assert _abi_call(p.cstruct, bt, B, betas, 9, pose, 45, gv, 0, gj, outs, ws, nws) == EINVAL            # betas rows of 9
        assert _abi_call(p.cstruct, bt, B, betas, 10, pose, 44, gv, 0, gj, outs, ws, nws) == EINVAL           # pose rows of 44
        assert _abi_call(p.cstruct, bt, B, betas, 10, pose, 45, gv, 2, gj, outs, ws, nws) == EINVAL and b"layout" in lib.dvq_last_error()
        assert _abi_call(p.cstruct, bt, B, betas, 10, pose, 45, None, 0, None, outs, ws, nws) == EINVAL and b"both null" in lib.dvq_last_error()
        assert _abi_call(p.cstruct, bt, -1, betas, 10, pose, 45, gv, 0, gj, outs, ws, nws) == EINVAL
        assert _abi_call(p.cstruct, None, B, betas, 10, pose, 45, gv, 0, gj, outs, ws, nws) == EINVAL
        assert _abi_call(p.cstruct, bt, B, betas, 10, pose, 45, gv, 0, gj, outs, None, nws) == EINVAL and b"workspace" in lib.dvq_last_error()
        assert _abi_call(p.cstruct, bt, B, betas, 10, pose, 45, gv, 0, gj, outs, ws[4:], nws) == EINVAL       # unaligned workspace
        assert _abi_call(p.cstruct, bt, B, betas, 10, pose, 45, gv, 0, gj, outs, ws, nws - 1) == EWORKSPACE and b"workspace" in lib.dvq_last_error()
        for j, bad in ((3, 3), (5, 9), (0, 0), (15, 16)):
            s = _lib.ManoModel.from_buffer_copy(p.cstruct)                                           # never the shared struct
            s.parents[j] = bad
            assert _abi_call(s, bt, B, betas, 10, pose, 45, gv, 0, gj, outs, ws, nws) == EINVAL and b"parents" in lib.dvq_last_error(), (j, bad)
        assert p.cstruct.parents[3] == 2
        assert _abi_call(p.cstruct, bt, 0, betas, 10, pose, 45, gv, 0, gj, outs, None, 0) == 0        # B = 0: nothing to do
        torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)                   # nothing was launched
    again = ops.mano_backward(p, betas, pose, go, tr, grad_verts=gv, grad_joints=gj)
    assert all(torch.equal(a, b) for a, b in zip(again, good))          # and the library still works
    # B = 0: empty gradients of the right shape
    e = lambda *n: torch.empty(0, *n, device=DEV)
    g = ops.mano_backward(p, e(10), e(45), e(3), e(3), grad_verts=e(778, 3), grad_joints=e(16, 3))
    assert [tuple(x.shape) for x in g] == [(0, 10), (0, 45), (0, 3), (0, 3)] and all(x.dtype == torch.float32 and x.device.type == "cuda" for x in g)
    g = ops.mano_backward(p, e(10), e(45), grad_verts=e(3, 778), channel_major=True, needs=(False, True, False, False))
    assert g[0] is None and tuple(g[1].shape) == (0, 45)


DESCENT_STEPS, DESCENT_LR = 200, 0.05   # fixed on the CPU: the float32 restatement under the same optimiser ends at 3.6e-5 of its starting loss (9.87e-3 -> 3.55e-7; float64: the same four digits)


@gpu
def test_descent_works_end_to_end(models):
    """Adam on betas, hand_pose, global_orient and transl of four real-model hands towards vertices made from known parameters,
    loss = mean squared vertex distance.  The float32 restatement on the CPU, same optimiser, steps and rate, must reach 1 % of
    its starting loss; the layer on the device must end within twice the CPU run's final loss."""
    B = 4
    target_p = _inputs(B, "descent/target")
    start = [t + d for t, d in zip(target_p, _inputs(B, "descent/start", pose_scale=0.3, betas_scale=0.5, go_scale=0.2, tr_scale=0.05))]
    m32 = _restatement(models, "real", True, torch.float32)
    layer = _layer(models, "real", True)
    loss_of = lambda v, target: ((v - target) ** 2).sum(-1).mean()

    def descend(verts_of, dev):
        with torch.no_grad():
            target = verts_of(*(t.to(dev) for t in target_p))
        ps = [t.to(dev).clone().requires_grad_(True) for t in start]
        opt = torch.optim.Adam(ps, lr=DESCENT_LR)
        first = None
        for _ in range(DESCENT_STEPS):
            opt.zero_grad()
            loss = loss_of(verts_of(*ps), target)
            loss.backward()
            opt.step()
            first = float(loss.detach()) if first is None else first
        with torch.no_grad():
            return first, float(loss_of(verts_of(*ps), target))

    c0, c1 = descend(lambda b, p, g, t: m32(b, p, g, t)[0], "cpu")
    d0, d1 = descend(lambda b, p, g, t: layer(betas=b, global_orient=g, hand_pose=p, transl=t).vertices, DEV)
    print(f"mano-grad-descent: cpu {c0:.3e} -> {c1:.3e} ({c1 / c0:.2e}); device {d0:.3e} -> {d1:.3e} ({d1 / d0:.2e})")
    assert c1 <= 0.01 * c0, (c0, c1)
    assert abs(d0 - c0) <= 1e-3 * c0, (d0, c0)
    assert np.isfinite(d1) and d1 <= 2.0 * c1, (d1, c1)
