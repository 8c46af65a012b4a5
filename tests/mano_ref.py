"""float64 numpy restatement of the MANO hand layer -- test infrastructure.

Written from the published algorithm, step by step, and from nothing else: PCA pose plus mean, Rodrigues with
``angle = ||r + 1e-8||``, shape and pose blendshapes, regressed joints, the kinematic chain, linear blend skinning, ``transl``
added to vertices and joints.  Feed it ``device_arrays(arrays)`` (the model rounded to fp32 and widened again: the numbers the
device holds) and fp32 inputs, so that a difference to it measures arithmetic and not input rounding."""
import numpy as np

NV, NJ, NB, NP = 778, 16, 10, 45
_FLOAT_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "weights", "hands_components", "hands_mean")


def device_arrays(arrays):
    """The model as the device sees it: every float array rounded to fp32, then widened to float64."""
    out = dict(arrays)
    for k in _FLOAT_KEYS:
        out[k] = np.asarray(arrays[k], dtype=np.float64).astype(np.float32).astype(np.float64)
    out["parents"] = np.asarray(arrays["parents"]).astype(np.int64).reshape(-1)
    return out


def _f64(x):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def rodrigues(r):
    """Axis-angle [..., 3] -> rotation matrices [..., 3, 3].  ``1 - cos a`` is taken as ``2 sin^2(a/2)``: the same number, without
    the cancellation of the literal form at small angles."""
    r = _f64(r)
    e = r + 1e-8
    angle = np.sqrt((e * e).sum(-1))
    d = r / angle[..., None]
    K = np.zeros(r.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -d[..., 2], d[..., 1]
    K[..., 1, 0], K[..., 1, 2] = d[..., 2], -d[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -d[..., 1], d[..., 0]
    s = np.sin(angle)[..., None, None]
    c1 = (2.0 * np.sin(0.5 * angle) ** 2)[..., None, None]
    return np.eye(3) + s * K + c1 * (K @ K)


def mano_ref_full(arrays, betas, hand_pose, global_orient=None, transl=None, flat_hand_mean=True):
    """Every intermediate of the layer, as a dict of float64 arrays."""
    betas, hand_pose = _f64(betas), _f64(hand_pose)
    B = betas.shape[0]
    assert betas.shape == (B, NB) and hand_pose.shape == (B, NP)
    go = np.zeros((B, 3)) if global_orient is None else _f64(global_orient)
    tr = np.zeros((B, 3)) if transl is None else _f64(transl)
    vt, sd = _f64(arrays["v_template"]), _f64(arrays["shapedirs"])[:, :, :NB]
    pd = _f64(arrays["posedirs"]).reshape(NV * 3, 9 * (NJ - 1))
    jr, w = _f64(arrays["J_regressor"]), _f64(arrays["weights"])
    comps = _f64(arrays["hands_components"])[:NP]
    parents = [int(p) for p in np.asarray(arrays["parents"]).reshape(-1)]
    mean = np.zeros(NP) if flat_hand_mean else _f64(arrays["hands_mean"])

    # 1. PCA pose -> axis-angle, plus the mean pose
    full_pose = np.concatenate([go, hand_pose @ comps], axis=1) + np.concatenate([np.zeros(3), mean])
    # 2. shape blendshapes and the joints regressed from the shaped mesh
    v_shaped = vt[None] + (sd.reshape(NV * 3, NB) @ betas.T).T.reshape(B, NV, 3)
    J = np.stack([jr @ v_shaped[b] for b in range(B)]) if B else np.zeros((0, NJ, 3))
    # 3. joint rotations
    R = rodrigues(full_pose.reshape(B, NJ, 3))
    # 4. pose blendshapes
    pose_feature = (R[:, 1:] - np.eye(3)).reshape(B, 9 * (NJ - 1))
    v_posed = v_shaped + (pose_feature @ pd.T).reshape(B, NV, 3)
    # 5. kinematic chain: world rotation and translation of every joint
    Gr, Gt = np.zeros((B, NJ, 3, 3)), np.zeros((B, NJ, 3))
    for j in range(NJ):
        p = parents[j]
        if p < 0:
            Gr[:, j], Gt[:, j] = R[:, j], J[:, j]
        else:
            assert p < j
            Gr[:, j] = Gr[:, p] @ R[:, j]
            Gt[:, j] = (Gr[:, p] @ (J[:, j] - J[:, p])[..., None])[..., 0] + Gt[:, p]
    # the rest joint removed: x -> Gr (x - J) + Gt
    At = Gt - (Gr @ J[..., None])[..., 0]
    # 6. skinning
    Tr = np.einsum("vj,bjik->bvik", w, Gr)
    Tt = np.einsum("vj,bji->bvi", w, At)
    verts = (Tr @ v_posed[..., None])[..., 0] + Tt + tr[:, None]
    joints = Gt + tr[:, None]
    return dict(full_pose=full_pose, v_shaped=v_shaped, J=J, R=R, pose_feature=pose_feature, v_posed=v_posed, Gr=Gr, Gt=Gt,
                verts=verts, joints=joints)


def mano_ref(arrays, betas, hand_pose, global_orient=None, transl=None, flat_hand_mean=True):
    """-> (verts [B,778,3], joints [B,16,3]) in float64."""
    o = mano_ref_full(arrays, betas, hand_pose, global_orient, transl, flat_hand_mean)
    return o["verts"], o["joints"]
