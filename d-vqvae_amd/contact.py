"""Contact / penetration proxies on the device: mirrors of the reference's
``utils/utils_loss.py`` (``get_NN`` :7-24, ``get_interior`` :27-45) and of the penetration / contact terms of
``utils/loss.py`` ``TTT_loss`` (:144-160), batched over grasps.  The reference runs them through pytorch3d
(``knn_points``, ``Meshes.verts_normals_packed``), which is not available here: parity is pinned against
``oracle/contact_oracle.py`` (a numpy restatement of the published algorithms), not against pytorch3d output.
"""
import json
import math
import os

import numpy as np
import torch

from . import ops


def _host(x, dtype=None):
    """A tensor (on any device) or an array-like as a numpy array."""
    return np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=dtype)


class _DeviceTables:
    """Host tables that the kernels read from device copies, uploaded once per device.  A subclass names its numpy arrays in
    ``_tables`` and ends its ``__init__`` with ``_start_cache(device)``; ``on(device)`` returns the copies: a tuple in the order of
    ``_tables``, or the tensor itself when there is one table."""
    _tables = ()

    def _start_cache(self, device):
        self._dev = {}
        if device is not None:
            self.on(torch.device(device))

    def _upload(self, device):
        copies = tuple(torch.from_numpy(np.ascontiguousarray(getattr(self, name))).to(device) for name in self._tables)
        return copies if len(copies) > 1 else copies[0]

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self._upload(device)
        return self._dev[key]


def face_csr(faces, n_verts):
    """faces [F,3] (array-like) -> (faces int32 [F,3], vf_off int32 [V+1], vf_face int32 [3F]) numpy arrays: for each
    vertex the faces that contain it, ascending."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    vert = f.reshape(-1)
    face = np.repeat(np.arange(f.shape[0]), 3)
    order = np.lexsort((face, vert))
    counts = np.bincount(vert, minlength=n_verts)
    off = np.zeros(n_verts + 1, dtype=np.int64)
    off[1:] = np.cumsum(counts)
    return f.astype(np.int32), off.astype(np.int32), face[order].astype(np.int32)


def seal_faces(faces, n_verts):
    """faces [F,3] of an orientable mesh with holes -> ``(faces_sealed int32 [F + sum of loop lengths, 3], loop_off int32 [L+1],
    loop_vert int32)``: the open boundary loops, found from the topology alone (the directed edges whose reverse no face uses), each
    closed by a fan of triangles to a NEW centre vertex ``n_verts + l`` (``dvq_grasp_volume`` places it at the loop's mean), wound
    against the boundary edges so that the sealed mesh is closed and consistently oriented.  Loops are ordered by their lowest vertex
    and start there; a closed mesh gives no loop.  Raises if a directed edge is used twice (an edge used more than twice, or faces of
    inconsistent orientation) or if the boundary branches at a vertex."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= n_verts):
        raise RuntimeError(f"seal_faces: a face index is outside [0, {n_verts})")
    directed = {}
    for a, b in f[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2).tolist():
        if a == b or (a, b) in directed:
            raise RuntimeError(f"seal_faces: the directed edge ({a}, {b}) is degenerate or used twice (non-manifold or inconsistently oriented mesh)")
        directed[(a, b)] = True
    nxt = {}
    for a, b in directed:
        if (b, a) not in directed:                              # used by one face only: a boundary edge a -> b
            if a in nxt:
                raise RuntimeError(f"seal_faces: the boundary branches at vertex {a}")
            nxt[a] = b
    loops, seen = [], set()
    for start in sorted(nxt):
        if start in seen:
            continue
        loop, v = [], start
        while v not in seen:
            seen.add(v)
            loop.append(v)
            if v not in nxt:
                raise RuntimeError(f"seal_faces: the boundary does not close at vertex {v}")
            v = nxt[v]
        if v != start:
            raise RuntimeError(f"seal_faces: the boundary branches at vertex {v}")
        loops.append(loop)
    fan = [[b, a, n_verts + l] for l, loop in enumerate(loops) for a, b in zip(loop, loop[1:] + loop[:1])]
    sealed = np.concatenate([f, np.asarray(fan, np.int64).reshape(-1, 3)]).astype(np.int32)
    off = np.zeros(len(loops) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(loop) for loop in loops])
    return sealed, off, np.asarray([v for loop in loops for v in loop], dtype=np.int32)


class HandTopology:
    """Device copies of a mesh topology (MANO: 778 vertices, 1538 faces) for ``vertex_normals``; ``sealed()``: the closed face list
    and boundary loops of ``seal_faces`` for ``grasp_volume``, made on first use."""

    def __init__(self, faces, n_verts, device):
        f, off, vf = face_csr(faces, n_verts)
        self.n_verts = n_verts
        self.faces = torch.from_numpy(f).to(device)
        self.vf_off = torch.from_numpy(off).to(device)
        self.vf_face = torch.from_numpy(vf).to(device)
        self._host_faces, self._sealed = f, None

    def normals(self, verts):
        return ops.vertex_normals(verts.contiguous(), self.faces, self.vf_off, self.vf_face)

    def sealed(self):
        """(faces_sealed, loop_off, loop_vert) of ``seal_faces`` on the device."""
        if self._sealed is None:
            self._sealed = tuple(torch.from_numpy(a).to(self.faces.device) for a in seal_faces(self._host_faces, self.n_verts))
        return self._sealed


def get_NN(src_xyz, trg_xyz):
    """(nn_dists [B,N1] squared, nn_idx [B,N1]) -- utils_loss.get_NN with k=1."""
    return ops.nn_points(src_xyz, trg_xyz)


def get_interior(src_face_normal, src_xyz, trg_xyz, trg_NN_idx):
    """utils_loss.get_interior(hand normals, hand verts, object points, NN index of each object point in the hand)."""
    return ops.interior(src_face_normal.contiguous(), src_xyz.contiguous(), trg_xyz, trg_NN_idx.contiguous())


def grasp_proxies(topology, hand_xyz, obj_xyz, contact_threshold=0.02 ** 2):
    """Per-grasp proxies from TTT_loss (loss.py:154-164), unreduced so that callers can rank grasps:
    ``penetration`` [B] = sum of squared NN distances over interior object points (the reference reports
    120 * sum / B), ``n_interior`` [B], ``n_contact`` [B] = object points within 2 cm of the hand (the dynamic contact
    region ``nn_dist < 0.02**2``), plus the raw ``nn_dist``, ``nn_idx``, ``interior``.
    hand_xyz [B,778,3]; obj_xyz [B,N,3] (any strides, e.g. ``cloud[:, :3].transpose(1, 2)``)."""
    normals = topology.normals(hand_xyz)
    nn_dist, nn_idx = get_NN(obj_xyz, hand_xyz.contiguous())
    inside = get_interior(normals, hand_xyz, obj_xyz, nn_idx)
    zero = torch.zeros((), dtype=nn_dist.dtype, device=nn_dist.device)
    return {"penetration": torch.where(inside, nn_dist, zero).sum(dim=1), "n_interior": inside.sum(dim=1),
            "n_contact": (nn_dist < contact_threshold).sum(dim=1), "nn_dist": nn_dist, "nn_idx": nn_idx,
            "interior": inside, "normals": normals}


def grasp_scores(topology, hand_xyz, obj_xyz, contact_threshold=0.02 ** 2):
    """``penetration`` [B] f32, ``n_interior`` [B] i32, ``n_contact`` [B] i32 of ``grasp_proxies`` from ONE fused kernel
    (ops.grasp_scores): no [B,N] tensor is made.  Per object point the same bits; the sums in a fixed order (256 strided partial
    sums, then a binary tree), so a grasp's scores do not depend on the batch it is in -- ``grasp_proxies``' penetration is a
    torch reduction and agrees to rounding.  A grasp with a NaN distance reports NaN."""
    pen, n_in, n_ct = ops.grasp_scores(hand_xyz.contiguous(), topology.faces, topology.vf_off, topology.vf_face, obj_xyz,
                                       contact_threshold)
    return {"penetration": pen, "n_interior": n_in, "n_contact": n_ct}


def refine_translation(topology, hand_xyz, obj_xyz, steps, push=1.0, pull=0.25, min_contact=1, contact_threshold=0.02 ** 2):
    """Translation push-out from ONE fused kernel per call (ops.grasp_refine; the update rule is in include/dvq.h under
    dvq_grasp_refine): at most ``steps`` steps of descent on the scores of ``grasp_scores`` with respect to the hand's rigid
    translation -- object points inside the hand push it out by ``push`` times their mean pull vector, points within the contact
    threshold outside it pull it closer by ``pull`` times theirs -- and of the iterates 0 .. steps the best under the key of
    ``select_keys("penetration")`` (``min_contact``), the earliest among equals.  Returns ``offset`` [B,3] f32 (add it to the hand's
    translation: ``params[:, 58:61]``), ``iter`` [B] i32 (the iterate kept; 0 = the hand as given) and that iterate's ``penetration``,
    ``n_interior``, ``n_contact``.  ``steps = 0`` gives the scores of ``grasp_scores`` and a zero offset.

    The defaults are a numpy prototype's on a sphere against a sphere and are untuned; the effect on real grasps is NOT measured
    (no real checkpoint).  Known limit: an object lying deep inside the hand is pulled further in (its nearest-vertex distances
    shrink that way): the kept iterate is only "not worse under the proxy"."""
    offset, it, pen, n_in, n_ct = ops.grasp_refine(hand_xyz.contiguous(), topology.faces, topology.vf_off, topology.vf_face, obj_xyz,
                                                   steps, push, pull, min_contact, contact_threshold)
    return {"offset": offset, "iter": it, "penetration": pen, "n_interior": n_in, "n_contact": n_ct}


def refine_rigid(topology, hand_xyz, obj_xyz, pivot, steps, push=1.0, pull=0.25, spin=1.0, min_contact=1, contact_threshold=0.02 ** 2):
    """Rigid push-out from ONE fused kernel per call (ops.grasp_refine_rigid; the update rule is in include/dvq.h under
    dvq_grasp_refine_rigid): ``refine_translation`` whose hand may also TURN about ``pivot`` [B,3] (the wrist: the root joint's world
    position) -- a hand that sinks into the object with its fingertips while its palm stands off cannot be repaired by a shift.  Per
    step the turn is ``spin`` times the least-squares small rotation (isotropic inertia about the pivot) towards the pull field left
    after its mean, which the shift takes, is removed.  Returns ``refine_translation``'s dict plus ``quat`` [B,4] f32 (w, x, y, z):
    the refined hand is ``apply_rigid(hand_xyz, pivot, offset, quat)``, and for a MANO hand the parameters are ``transl + offset``
    and ``compose_orient(global_orient, quat)``.  ``spin = 0`` gives ``refine_translation``'s bits and the identity quaternion.

    The defaults are a numpy prototype's and are untuned; the effect on real grasps is NOT measured (no real checkpoint).  Known
    limits: the turn under-estimates when the contacts cluster far from the wrist; the pull term may turn the hand into the object;
    the kept iterate is only "not worse under the proxy"."""
    offset, quat, it, pen, n_in, n_ct = ops.grasp_refine_rigid(hand_xyz.contiguous(), topology.faces, topology.vf_off, topology.vf_face,
                                                               obj_xyz, pivot.contiguous(), steps, push, pull, spin, min_contact,
                                                               contact_threshold)
    return {"offset": offset, "quat": quat, "iter": it, "penetration": pen, "n_interior": n_in, "n_contact": n_ct}


def _quat_mul(a, b):
    """Hamilton product of (w, x, y, z) tuples of tensors, elementwise."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
            aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw)


def _quat_rows(quat):
    """(w, x, y, z) of quaternions [..., 4], float64, normalised."""
    w, x, y, z = quat.to(torch.float64).unbind(-1)
    n = torch.sqrt(w * w + x * x + y * y + z * z)
    return w / n, x / n, y / n, z / n


def _quat_matrix(w, x, y, z):
    """The rotation matrix of a unit quaternion: three rows of three entries, elementwise."""
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def _is_identity(quat):
    """True where a quaternion [..., 4] is exactly (1, 0, 0, 0)."""
    w, x, y, z = quat.to(torch.float64).unbind(-1)
    return (w == 1) & (x == 0) & (y == 0) & (z == 0)


def axis_angle_quat(axis_angle):
    """Axis-angle [B,3] -> the unit quaternion [B,4] (w, x, y, z) of the same rotation, float64, elementwise per row; safe at 0."""
    a = axis_angle.to(torch.float64)
    x, y, z = a.unbind(-1)
    th2 = x * x + y * y + z * z
    th = torch.sqrt(th2)
    small = th < 1e-6
    k = torch.where(small, 0.5 - th2 / 48.0, torch.sin(0.5 * th) / torch.where(small, torch.ones_like(th), th))   # sin(th/2) / th
    return torch.stack([torch.cos(0.5 * th), k * x, k * y, k * z], -1)


def _atan2_rowwise(y, x):
    """``torch.atan2`` whose result for an element does not depend on the tensor around it.  On the device every element is one
    thread's.  On the host torch's vectorised loop and its scalar tail round differently (seen: the last bit of 2 rows in 24), so host
    tensors go through numpy, whose loop treats every element alike."""
    if y.is_cuda:
        return torch.atan2(y, x)
    return torch.from_numpy(np.arctan2(y.detach().numpy(), x.detach().numpy()))


def quat_axis_angle(quat):
    """Quaternion [B,4] (w, x, y, z; any positive norm) -> the axis-angle [B,3] of its rotation, float64, elementwise per row: the sign
    is chosen so that w >= 0, the angle is ``2 atan2(|v|, w)`` (at most pi), and the identity gives exact zeros."""
    return _quat_axis_angle(quat, torch.atan2)


def _quat_axis_angle(quat, _atan2):
    """``quat_axis_angle`` with the arc tangent given: ``torch.atan2``, or ``_atan2_rowwise`` where a row's bits must not depend on its
    batch on the host either (``compose_finger_pose``)."""
    q = quat.to(torch.float64)
    w, x, y, z = q.unbind(-1)
    flip = w < 0
    w, x, y, z = (torch.where(flip, -c, c) for c in (w, x, y, z))
    n = torch.sqrt(x * x + y * y + z * z)
    small = n < 1e-9 * w                                        # angle / |v| -> 2 / w as |v| -> 0
    k = torch.where(small, 2.0 / torch.where(small, w, torch.ones_like(w)),
                    2.0 * _atan2(n, w) / torch.where(small, torch.ones_like(n), n))
    return torch.stack([k * x, k * y, k * z], -1)


def compose_orient(global_orient, quat):
    """The axis-angle [B,3] of ``Q * exp(global_orient)`` for ``quat`` [B,4] (w, x, y, z): the ``global_orient`` of a MANO hand turned by
    ``Q`` about its root joint (``refine_rigid``'s ``quat`` with the root joint's world position as pivot).  Through quaternions, in
    float64, elementwise per row (a row's result does not depend on the batch), returned in ``global_orient``'s dtype; a row whose
    ``quat`` is exactly (1, 0, 0, 0) returns its ``global_orient`` untouched."""
    qw, qx, qy, qz = quat.to(torch.float64).unbind(-1)
    out = quat_axis_angle(torch.stack(_quat_mul((qw, qx, qy, qz), axis_angle_quat(global_orient).unbind(-1)), -1)).to(global_orient.dtype)
    return torch.where(_is_identity(quat).unsqueeze(-1), global_orient, out)


def apply_rigid(hand_xyz, pivot, offset, quat):
    """``R (v - c) + c + t`` for hand_xyz [B,V,3], pivot c [B,3], offset t [B,3] and quat [B,4] (w, x, y, z; normalised here): the hand
    ``refine_rigid`` reports, in float64 inside and in ``hand_xyz``'s dtype outside, elementwise per row."""
    R = _quat_matrix(*_quat_rows(quat))
    c, t = pivot.to(torch.float64).unsqueeze(1), offset.to(torch.float64).unsqueeze(1)
    d = hand_xyz.to(torch.float64) - c
    dx, dy, dz = d.unbind(-1)
    rows = [R[i][0].unsqueeze(1) * dx + R[i][1].unsqueeze(1) * dy + R[i][2].unsqueeze(1) * dz for i in range(3)]
    return (torch.stack(rows, -1) + c + t).to(hand_xyz.dtype)


class FingerRig(_DeviceTables):
    """What the articulated push-out knows of the hand's fingers: ``vert_part`` int32 [V] (the finger of every vertex, -1 = none),
    ``vert_w`` float32 [V] (how far the vertex follows its finger's turn, in [0, 1]) and ``joints`` (per finger the index of its
    knuckle among the layer's joints: the pivot of the finger's turn).  Device copies are made once per device (``on``)."""
    _tables = ("vert_part", "vert_w")                         # on(device): (vert_part int32 [V], vert_w f32 [V])

    def __init__(self, vert_part, vert_w, joints, device=None):
        part = _host(vert_part)
        w = _host(vert_w, np.float64)
        self.joints = [int(j) for j in joints]
        if not 1 <= len(self.joints) <= ops.GRASP_FINGERS_MAX_P:
            raise RuntimeError(f"FingerRig: between 1 and {ops.GRASP_FINGERS_MAX_P} fingers (got {len(self.joints)})")
        if part.ndim != 1 or part.size < 1 or part.dtype.kind not in "iu" or w.shape != part.shape:
            raise RuntimeError("FingerRig: vert_part must be a non-empty 1-D integer array and vert_w one weight per vertex")
        part = part.astype(np.int64)
        if part.min() < -1 or part.max() >= len(self.joints):
            raise RuntimeError(f"FingerRig: vert_part must lie in [-1, {len(self.joints)}) (got {int(part.min())} .. {int(part.max())})")
        if not np.all((w >= 0.0) & (w <= 1.0)):
            raise RuntimeError("FingerRig: vert_w must lie in [0, 1]")
        self.vert_part, self.vert_w = part.astype(np.int32), w.astype(np.float32)
        self.n_verts, self.n_fingers = int(part.size), len(self.joints)
        self._start_cache(device)

    @classmethod
    def from_mano(cls, layer, device=None):
        """The rig of a MANO layer (``mano.ManoLayer``), from its kinematic tree and skinning weights: a finger is a child of the root
        joint with all its descendants, in joint order; a vertex belongs to the chain with the largest sum of skinning weights (the
        lowest chain on ties), that sum (float64 over the weights as loaded, rounded once to fp32 and clipped to [0, 1]) is its
        weight, and a vertex whose sum is 0 belongs to no finger."""
        packed = layer._packed
        parents = [int(p) for p in packed.parents]
        weights = np.asarray(packed.skin_weights, np.float64)                                   # [V,J], as loaded (not the fp32 copy)
        knuckles = [j for j, p in enumerate(parents) if p == 0]
        chain_of = [-1] * len(parents)
        for j in range(1, len(parents)):                          # parents precede their children in the tree
            chain_of[j] = knuckles.index(j) if parents[j] == 0 else chain_of[parents[j]]
        sums = np.stack([weights[:, [j for j, c in enumerate(chain_of) if c == f]].sum(axis=1) for f in range(len(knuckles))], 1)
        part = np.argmax(sums, axis=1)                            # the first of equal sums
        w = np.clip(sums[np.arange(len(part)), part].astype(np.float32), 0.0, 1.0)
        return cls(np.where(w > 0, part, -1), w, knuckles, device)


def refine_fingers(topology, rig, hand_xyz, obj_xyz, pivot, knuckles, steps, push=1.0, pull=0.25, spin=1.0, curl=1.0, max_curl=0.35,
                   min_contact=1, contact_threshold=0.02 ** 2):
    """Articulated push-out from ONE fused kernel per call (ops.grasp_refine_fingers; the update rule is in include/dvq.h under
    dvq_grasp_refine_fingers): ``refine_rigid`` whose fingers may also CURL, each by one rotation about its knuckle (``knuckles``
    [B,P,3]: the world positions of ``rig.joints`` in the hand as given) -- one fingertip buried in the object while the others sit
    well cannot be repaired by a rigid motion.  The kernel searches with a blend model of the hand (``apply_fingers``), not with MANO;
    per step a finger's turn is ``curl`` times the least-squares small rotation about its knuckle towards the pulls at its own
    vertices, and no finger turns further than ``max_curl`` radians from the hand as given.  Returns ``refine_rigid``'s dict plus
    ``finger_quat`` [B,P,4] f32 (w, x, y, z, in the frame of the hand as given) and ``penetration0`` / ``n_interior0`` /
    ``n_contact0`` [B], the scores of the hand as given (the bits of ``grasp_scores``).  The hand the kernel believed in is
    ``apply_rigid(apply_fingers(hand_xyz, rig, knuckles, finger_quat), pivot, offset, quat)``; for a MANO hand the pose parameters are
    ``compose_finger_pose(...)``.  ``curl = 0`` gives ``refine_rigid``'s bits and identity finger quaternions.

    The defaults are untuned; the effect on real grasps is NOT measured (no real checkpoint).  Known limits: the blend model differs
    from the re-posed MANO hand by up to 3.2 mm at 0.35 rad, so the kept iterate is the best only under that model --
    compare the re-posed hand's scores with ``penetration0`` / ``n_contact0`` before keeping it; no joint limits beyond ``max_curl``;
    no finger-to-finger collision test; shift, turn and curl answer the same contacts, so a step may overshoot."""
    if not torch.is_tensor(hand_xyz) or hand_xyz.dim() != 3 or hand_xyz.shape[1] != rig.n_verts:
        raise RuntimeError(f"refine_fingers: the rig has {rig.n_verts} vertices, the hand "
                           f"{tuple(hand_xyz.shape) if torch.is_tensor(hand_xyz) else type(hand_xyz)}")
    part, w = rig.on(hand_xyz.device)
    names = ("offset", "quat", "finger_quat", "iter", "penetration", "n_interior", "n_contact", "penetration0", "n_interior0", "n_contact0")
    out = ops.grasp_refine_fingers(hand_xyz.contiguous(), topology.faces, topology.vf_off, topology.vf_face, part, w, rig.n_fingers,
                                   obj_xyz, pivot.contiguous(), knuckles.contiguous(), steps, push, pull, spin, curl, max_curl,
                                   min_contact, contact_threshold)
    return dict(zip(names, out))


def apply_fingers(hand_xyz, rig, knuckles, finger_quat):
    """The blend model of ``refine_fingers``: a vertex v of finger f with weight w becomes ``v + w (R_f (v - c_f) + c_f - v)`` for
    hand_xyz [B,V,3], knuckles c [B,P,3] and finger_quat [B,P,4] (w, x, y, z; normalised here); a vertex of no finger, or of a finger
    whose quaternion is exactly (1, 0, 0, 0), keeps its bits.  Float64 inside, ``hand_xyz``'s dtype outside, elementwise per row.  It
    states what the kernel believed, NOT the MANO hand of the composed pose (DESIGN.md 3 has the difference); ``apply_rigid`` on top
    gives the world hand."""
    part, wv = rig.on(hand_xyz.device)
    part = part.to(torch.int64)
    v = hand_xyz.to(torch.float64)
    same = _is_identity(finger_quat)                                                # [B,P]
    R = _quat_matrix(*_quat_rows(finger_quat))
    idx = part.clamp(min=0)                                                         # [V]: finger per vertex (0 where none; masked below)
    c = knuckles.to(torch.float64).index_select(1, idx)                             # [B,V,3]
    d = v - c
    dx, dy, dz = d.unbind(-1)
    rows = [R[i][0].index_select(1, idx) * dx + R[i][1].index_select(1, idx) * dy + R[i][2].index_select(1, idx) * dz for i in range(3)]
    rot = torch.stack(rows, -1) + c
    out = v + wv.to(torch.float64).view(1, -1, 1) * (rot - v)
    keep = (part < 0).view(1, -1) | same.index_select(1, idx)                       # [B,V]
    return torch.where(keep.unsqueeze(-1), hand_xyz, out.to(hand_xyz.dtype))


def compose_finger_pose(layer, global_orient, hand_pose, finger_quat, rig):
    """The ``hand_pose`` [B,45] (PCA coefficients) of a MANO hand whose finger f has been turned by ``finger_quat[:, f]`` (w, x, y, z;
    expressed in the frame of the hand as generated) about its knuckle.  The knuckles are children of the root joint, so the turn D_f
    is exactly ``R_loc' = R0^T D_f R0 R_loc`` on the knuckle's local rotation, with ``R0 = exp(global_orient)`` -- ``global_orient``
    [B,3] is the one AS GENERATED, before ``compose_orient``.  Through quaternions, in float64: the full pose is ``hand_pose @ comps +
    mean``, the knuckles' axis-angles are replaced, the mean is subtracted and the result is multiplied by the inverse of ``comps``
    (taken once, in float64, on the host: the components are invertible but not orthonormal).  Both 45-term products are summed term
    by term in a fixed elementwise order, so a row's result does not depend on its batch.  Returned in ``hand_pose``'s dtype; a row
    whose finger quaternions are all exactly (1, 0, 0, 0) returns its ``hand_pose`` untouched.  No MANO backward pass is involved."""
    packed = layer._packed
    cache = getattr(packed, "_finger_pose_cache", None)
    if cache is None:
        comps = packed.tensors["comps"].detach().cpu().numpy().astype(np.float64)
        mean = packed.tensors["pose_mean"].detach().cpu().numpy().astype(np.float64)[3:]
        cache = {"host": (comps, np.linalg.inv(comps), mean)}
        packed._finger_pose_cache = cache
    key = str(hand_pose.device)
    if key not in cache:
        cache[key] = tuple(torch.from_numpy(a).to(hand_pose.device) for a in cache["host"])
    comps, inv, mean = cache[key]
    hp = hand_pose.to(torch.float64)
    acc = hp[:, 0:1] * comps[0]
    for k in range(1, 45):
        acc = acc + hp[:, k:k + 1] * comps[k]
    full = (acc + mean).clone()
    q0 = axis_angle_quat(global_orient).unbind(-1)
    q0c = (q0[0], -q0[1], -q0[2], -q0[3])
    fq = finger_quat.to(torch.float64)
    for f, j in enumerate(rig.joints):
        lo = 3 * (j - 1)
        loc = axis_angle_quat(full[:, lo:lo + 3]).unbind(-1)
        new = _quat_mul(_quat_mul(_quat_mul(q0c, _quat_rows(fq[:, f])), q0), loc)
        full[:, lo:lo + 3] = _quat_axis_angle(torch.stack(new, -1), _atan2_rowwise)
    z = full - mean
    acc = z[:, 0:1] * inv[0]
    for k in range(1, 45):
        acc = acc + z[:, k:k + 1] * inv[k]
    return torch.where(_is_identity(fq).all(dim=1, keepdim=True), hand_pose, acc.to(hand_pose.dtype))


def grasp_stability(topology, hand_xyz, obj_xyz, length=0.1, contact_threshold=0.02 ** 2):
    """A force-closure proxy from ONE fused kernel (ops.grasp_wrench; the definition is in include/dvq.h under dvq_grasp_wrench):
    every object point within the contact threshold of the hand pushes with a unit force along the normal of its nearest hand vertex
    (frictionless), and its torque is taken about the cloud's centre with the arm divided by ``length``.  Returns the three scores of
    ``grasp_scores`` (the same bits: the selection path launches this kernel INSTEAD of that one) plus ``centre`` [B,3], ``sums``
    [B,27] (the summed wrench, then the upper triangle of sum w w^T: ``wrench_stats`` turns them into figures) and ``key`` [B] =
    |sum of the wrenches|^2 / n_contact^2, +inf without a contact, NaN with a NaN penetration -- smaller means the unit contact
    forces cancel better.

    ``length`` is in metres; 0.1 is a hand-sized default and is UNTUNED, as is the unit-force model.  This is a proxy: it replaces no
    physics run, and its effect on real grasps is NOT measured (no real checkpoint)."""
    length = ops._positive("grasp_stability", "length", length)
    pen, n_in, n_ct, centre, sums, key = ops.grasp_wrench(hand_xyz.contiguous(), topology.faces, topology.vf_off, topology.vf_face,
                                                          obj_xyz, 1.0 / length, contact_threshold)
    return {"penetration": pen, "n_interior": n_in, "n_contact": n_ct, "centre": centre, "sums": sums, "key": key}


def wrench_stats(sums, n_contact):
    """Host side, float64: per grasp, from ``grasp_stability``'s ``sums`` [B,27] and ``n_contact`` [B] (arrays or tensors),
    ``force_residual`` = |S[0:3]| / n (in [0,1]: 0 = the unit forces cancel, 1 = they all point one way), ``torque_residual`` =
    |S[3:6]| / n and ``min_sv`` = sqrt(max(lambda_min(G / n), 0)) with G the symmetric 6x6 matrix of columns 6 .. 26 (the smallest
    singular value of the grasp matrix over sqrt(n): 0 = some wrench direction no contact resists).  Three lists of floats, ``None``
    where n == 0 or a sum is not finite (json writes null).  A sphere-like contact patch has near-zero torque rows, so ``min_sv`` is small there by
    construction."""
    s = _host(sums, np.float64).reshape(-1, 27)
    n = _host(n_contact, np.int64).reshape(-1)
    if n.shape[0] != s.shape[0]:
        raise RuntimeError("wrench_stats: one n_contact per row of sums")
    iu = np.triu_indices(6)
    force, torque, min_sv = [], [], []
    for row, k in zip(s, n):
        if k <= 0 or not np.isfinite(row).all():                # no contact, or a grasp with a NaN / inf in it: no figure
            force.append(None), torque.append(None), min_sv.append(None)
            continue
        g = np.zeros((6, 6))
        g[iu] = row[6:]
        g = g + np.triu(g, 1).T
        force.append(float(np.sqrt(np.sum(row[0:3] ** 2)) / k))
        torque.append(float(np.sqrt(np.sum(row[3:6] ** 2)) / k))
        min_sv.append(float(np.sqrt(max(float(np.linalg.eigvalsh(g / k)[0]), 0.0))))
    return {"force_residual": force, "torque_residual": torque, "min_sv": min_sv}


CLOSURE_BASES = (2, 3, 5, 7, 11, 13)   # the Halton bases of closure_directions, one per wrench component
CLOSURE_OUTPUTS = ("quality", "worst_dir", "status", "n_contact", "centre")


def _radical_inverse(i, b):
    f, r = 1.0, 0.0
    while i > 0:
        f /= b
        r += f * (i % b)
        i //= b
    return r


class _ClosureTable(_DeviceTables):
    """The direction table of ``closure_directions`` for one D, made once; its device copies are cached as every table's are."""
    _tables = ("dirs",)

    def __init__(self, D):
        rows = [[(1.0 if s == 0 else -1.0) if c == a else 0.0 for c in range(6)] for a in range(6) for s in range(2)]
        i = 0
        while len(rows) < D:
            i += 1
            x = [2.0 * _radical_inverse(i, b) - 1.0 for b in CLOSURE_BASES]
            q = 0.0
            for v in x:
                q += v * v
            if 0.01 <= q <= 1.0:
                n = math.sqrt(q)
                u = [v / n for v in x]
                rows += [u, [-v for v in u]]
        self.dirs = np.asarray(rows[:D], dtype=np.float64).astype(np.float32)
        self.shown = self.dirs.view()                                  # what callers get: read-only
        self.shown.setflags(write=False)
        self._start_cache(None)


_CLOSURE_TABLES = {}


def _closure_table(D):
    D = int(D)
    if not 1 <= D <= ops.GRASP_CLOSURE_MAX_DIRS:
        raise RuntimeError(f"closure_directions: need 1 <= D <= {ops.GRASP_CLOSURE_MAX_DIRS} (got {D})")
    if D not in _CLOSURE_TABLES:
        _CLOSURE_TABLES[D] = _ClosureTable(D)
    return _CLOSURE_TABLES[D]


def closure_directions(D):
    """The [D,6] float32 table of unit directions in wrench space that ``grasp_closure`` samples, deterministic and without a random
    generator: rows 0 .. 11 are +e_0, -e_0, +e_1, ..., -e_5; the rest come from the Halton points i = 1, 2, ... in the bases (2, 3, 5,
    7, 11, 13): x = 2 h - 1 in float64, accepted iff 0.01 <= |x|^2 <= 1 (|x|^2 summed left to right), u = x / sqrt(|x|^2), and u, then
    -u, are appended; the table is cut at D (an odd D cuts a pair).  The radical inverse is the plain float64 loop ``f /= b; r += f *
    (i % b); i //= b``.  A read-only numpy array, made once per D; the device copies are cached per (D, device)."""
    return _closure_table(D).shown


def grasp_closure(topology, hand_xyz, obj_xyz, length=0.1, friction=0.5, dirs=256, threshold=0.02 ** 2, want_support=False):
    """Force-closure quality with Coulomb friction from ONE fused kernel (ops.grasp_closure; the definition is in include/dvq.h under
    dvq_grasp_closure): every object point within the contact threshold of the hand is a point contact with the normal of its nearest
    hand vertex and the friction coefficient ``friction``; torques are taken about the cloud's centre with the arm divided by
    ``length``.  Per grasp ``quality`` [B] is the smallest value, over the ``dirs`` directions of ``closure_directions`` (an int D, or
    a [D,6] fp32 tensor of the caller's own on the device), of the support function of the contacts' friction cones: an UPPER BOUND of
    the L1 Ferrari-Canny quality, so ``quality <= 0`` certifies that the grasp is NOT in force closure, and a positive value certifies
    nothing.  Also ``worst_dir`` [B] (the lowest direction that attains it, -1 without a figure), ``status`` [B] (0; 1 = no contact:
    quality -inf; 2 = a coordinate is not finite: quality NaN), ``n_contact`` [B] (the bits of ``grasp_scores``), ``centre`` [B,3] (the
    bits of ``grasp_stability``) and with ``want_support`` ``support`` [B,D].

    No physics run and no soft contact; ``friction`` and ``length`` are UNTUNED; contacts are cloud points within ``threshold`` (a
    squared distance, the scores' 2 cm), penetrating ones included; the effect on real grasps is NOT measured."""
    length = ops._positive("grasp_closure", "length", length)
    friction = ops._non_negative("grasp_closure", "friction", friction)
    if not torch.is_tensor(dirs):
        table = _closure_table(dirs)
        if not torch.is_tensor(hand_xyz):
            raise RuntimeError("grasp_closure: hand_xyz must be a tensor")
        dirs = table.on(hand_xyz.device) if hand_xyz.is_cuda else torch.from_numpy(table.dirs)
    out = ops.grasp_closure(hand_xyz.contiguous(), topology.faces, topology.vf_off, topology.vf_face, obj_xyz, 1.0 / length, friction,
                            dirs, threshold, want_support)
    res = dict(zip(CLOSURE_OUTPUTS, out[:5]))
    if want_support:
        res["support"] = out[5]
    return res


def closure_stats(quality, worst_dir, status):
    """Host side, float64, row by row, from ``grasp_closure``'s outputs (tensors or arrays): ``closure_quality`` (the quality; ``None``
    where status != 0 or the value is not finite: json writes null), ``force_closure`` (quality > 0 -- False certifies that the grasp
    is not in force closure, True only says that no sampled direction refutes it -- or ``None``) and ``closure_direction`` (the row of
    ``closure_directions`` that attains the quality, or ``None``).  Three lists."""
    q = _host(quality, np.float64).reshape(-1)
    k = _host(worst_dir, np.int64).reshape(-1)
    st = _host(status, np.int64).reshape(-1)
    if not q.shape[0] == k.shape[0] == st.shape[0]:
        raise RuntimeError("closure_stats: one worst_dir and one status per quality")
    has = [int(s) == 0 and math.isfinite(x) for x, s in zip(q, st)]
    return {"closure_quality": [float(x) if ok else None for x, ok in zip(q, has)],
            "force_closure": [bool(x > 0.0) if ok else None for x, ok in zip(q, has)],
            "closure_direction": [int(d) if ok else None for d, ok in zip(k, has)]}


def closure_class(out, min_closure):
    """int32 [B] on the device for ``torch.maximum`` with the class of ``select_keys``: 2 where the row of ``grasp_closure``'s output
    has no figure because a coordinate is not finite (status 2), else 1 where the hand touches nothing (status 1) or the quality is
    below ``min_closure``, else 0.  One fp32 comparison per row, ``quality < fp32(min_closure)``: no sum, so nothing depends on which
    rows share the call."""
    quality, status = out["quality"], out["status"]
    limit = float(min_closure)
    if math.isnan(limit):
        raise RuntimeError("closure_class: min_closure is NaN")
    below = quality < torch.tensor(limit, dtype=torch.float64, device=quality.device).to(torch.float32)
    return _guard_class(status == 2, below | (status == 1))


def hull_planes(points_xyz):
    """[N,3] cloud -> fp32 [P,4] rows (n, d), |n| = 1, with n.x <= d for every x inside the cloud's convex hull: the unique rows of
    ``scipy.spatial.ConvexHull(points).equations`` (float64; qhull lists a plane once per triangle of a facet), normalised, in
    lexicographic order.  The hull of a sampled cloud lies inside the hull of the mesh it was sampled from."""
    try:
        from scipy.spatial import ConvexHull
    except ImportError as e:
        raise RuntimeError("hull_planes: scipy is needed to build a convex hull (scipy.spatial.ConvexHull) and is not installed") from e
    pts = np.asarray(points_xyz, dtype=np.float64).reshape(-1, 3)
    if pts.shape[0] < 4 or not np.isfinite(pts).all():
        raise RuntimeError(f"hull_planes: need at least four finite points (got {pts.shape[0]})")
    eq = ConvexHull(pts).equations                              # [n, off] with n.x + off <= 0 inside
    eq = eq / np.linalg.norm(eq[:, :3], axis=1, keepdims=True)
    rows = np.concatenate([eq[:, :3], -eq[:, 3:]], axis=1).astype(np.float32) + np.float32(0.0)      # (no -0.0)
    return np.unique(rows, axis=0)


def pack_planes(planes_per_object):
    """A list of [P_o,4] arrays -> ``(planes fp32 [sum P_o, 4], plane_off int32 [O+1])`` numpy arrays for ``grasp_volume``."""
    rows = [np.asarray(p, dtype=np.float32).reshape(-1, 4) for p in planes_per_object]
    for o, r in enumerate(rows):
        if r.shape[0] > ops.GRASP_VOLUME_MAX_PLANES:
            raise RuntimeError(f"pack_planes: object {o} has {r.shape[0]} planes, at most {ops.GRASP_VOLUME_MAX_PLANES} fit")
    off = np.zeros(len(rows) + 1, dtype=np.int64)
    off[1:] = np.cumsum([r.shape[0] for r in rows])
    if off[-1] >= 2 ** 31:
        raise RuntimeError("pack_planes: too many planes")
    return (np.concatenate(rows) if rows else np.zeros((0, 4), np.float32)).astype(np.float32).reshape(-1, 4), off.astype(np.int32)


def grasp_volume(topology, hand_xyz, planes, plane_off, obj_of_row, R=None, t=None, res=0.001, err=None):
    """Penetration volume from ONE fused kernel (ops.grasp_volume; the definition is in include/dvq.h under dvq_grasp_volume): the
    hand mesh of ``topology`` sealed at its open boundary (``seal_faces``) against the convex hull of each row's object, given as
    half-spaces (``hull_planes`` / ``pack_planes``, on the device), on a lattice of spacing ``res`` metres in the object's own frame
    (``R`` [B,3,3], ``t`` [3]: what ``ops.transform_clouds`` got, None for objects in place).  Returns ``count`` [B] i32 (voxels in
    both; -1 = no figure), ``depth`` [B] f32 (the deepest hand vertex inside the hull, metres) and ``status`` [B] i32 (0 fine, 1 the
    hand's box misses the hull or the object has no plane, 2 the box has more than 1024 cells on an axis, 3 a vertex is not finite).
    ``volume_stats`` turns them into the figures written.

    Against the reference's intersection_eval this is a LOWER bound when the planes come from a sampled cloud (its hull lies inside
    the mesh's), the lattice is the object's and not anchored at a box corner, and no igl / trimesh run pins parity."""
    faces, loop_off, loop_vert = topology.sealed()
    count, depth, status = ops.grasp_volume(hand_xyz.contiguous(), faces, loop_off, loop_vert, planes, plane_off, obj_of_row, R, t, res,
                                            err=err)
    return {"count": count, "depth": depth, "status": status}


def volume_stats(count, depth, res):
    """Host side, float64, row by row: ``penetration_volume`` = count * res^3 * 1e6 in cm^3 and ``penetration_depth`` = depth * 100 in
    cm from ``grasp_volume``'s ``count`` and ``depth`` (arrays or tensors); two lists of floats, ``None`` where count < 0 (json writes
    null)."""
    c = _host(count, np.int64).reshape(-1)
    d = _host(depth, np.float64).reshape(-1)
    if c.shape[0] != d.shape[0]:
        raise RuntimeError("volume_stats: one depth per count")
    res = ops._positive("volume_stats", "res", res)
    cell = res * res * res * 1e6
    return {"penetration_volume": [float(k) * cell if k >= 0 else None for k in c],
            "penetration_depth": [float(x) * 100.0 if k >= 0 else None for k, x in zip(c, d)]}


def volume_limit(max_volume, res):
    """``--max_volume`` X cm^3 as the largest voxel count allowed, floor(X / (res^3 * 1e6)) in float64; +inf -> 2^31 - 1 (no limit)."""
    x = float(max_volume) / (float(res) ** 3 * 1e6)
    return int(min(np.floor(x), 2 ** 31 - 1))


class ObjectMeshes(_DeviceTables):
    """The triangle meshes of a call's objects, packed for ``grasp_mesh``: a list of ``(verts [n,3], faces [m,3])`` -> ``verts`` fp32
    [sum n, 3], ``vert_off`` int32 [O+1], ``faces`` int32 [sum m, 3] (indices local to each object's vertices) and ``face_off`` int32
    [O+1] as numpy arrays, uploaded once per device by ``on``.  ``closed[o]``: every edge of object o is used by exactly two faces,
    once in each direction (computed here, on the host) -- only then is "inside" defined; an open mesh is NOT refused, as the
    reference does not refuse it either.  Refused: a face index outside the object's vertices, an object without a face, and more
    than ``ops.GRASP_MESH_MAX_FACES`` faces per object (decimate the mesh first)."""
    _tables = ("verts", "vert_off", "faces", "face_off")      # on(device): the four of them, in this order

    def __init__(self, meshes, device=None):
        vs, fs, self.closed = [], [], []
        for o, (v, f) in enumerate(meshes):
            v = _host(v)
            f = _host(f)
            if v.ndim != 2 or v.shape[1] != 3 or f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
                raise RuntimeError(f"ObjectMeshes: object {o}: verts must be [n,3] and faces an integer [m,3] (got {v.shape}, {f.dtype} {f.shape})")
            if f.shape[0] < 1:
                raise RuntimeError(f"ObjectMeshes: object {o} has no face")
            if f.shape[0] > ops.GRASP_MESH_MAX_FACES:
                raise RuntimeError(f"ObjectMeshes: object {o} has {f.shape[0]} faces, at most {ops.GRASP_MESH_MAX_FACES} fit: "
                                   "decimate the mesh first")
            f = f.astype(np.int64)
            if f.min() < 0 or f.max() >= v.shape[0]:
                raise RuntimeError(f"ObjectMeshes: object {o}: a face index is outside [0, {v.shape[0]})")
            vs.append(v.astype(np.float32))
            fs.append(f.astype(np.int32))
            self.closed.append(self._closed(f, v.shape[0]))
        self.n_objects = len(vs)
        self.vert_off, self.face_off = np.zeros(len(vs) + 1, np.int64), np.zeros(len(fs) + 1, np.int64)
        self.vert_off[1:], self.face_off[1:] = np.cumsum([len(v) for v in vs]), np.cumsum([len(f) for f in fs])
        if self.vert_off[-1] >= 2 ** 31 or self.face_off[-1] >= 2 ** 31:
            raise RuntimeError("ObjectMeshes: too many vertices or faces")
        self.vert_off, self.face_off = self.vert_off.astype(np.int32), self.face_off.astype(np.int32)
        self.verts = np.concatenate(vs).reshape(-1, 3) if vs else np.zeros((0, 3), np.float32)
        self.faces = np.concatenate(fs).reshape(-1, 3) if fs else np.zeros((0, 3), np.int32)
        self._start_cache(device)

    @staticmethod
    def _closed(f, n):
        """Every directed edge at most once, and its reverse exactly as often."""
        d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        if (d[:, 0] == d[:, 1]).any():
            return False
        fwd, rev = np.sort(d[:, 0] * n + d[:, 1]), np.sort(d[:, 1] * n + d[:, 0])
        return bool((np.diff(fwd) != 0).all() and np.array_equal(fwd, rev))


def load_mesh(path):
    """``(verts float64 [n,3], faces int64 [m,3])`` from a ``.npz`` with ``verts`` and ``faces``, or from a Wavefront ``.obj`` of
    ``v`` and ``f`` lines (other lines are skipped): polygons are fan-triangulated, the ``v/vt/vn`` index forms are accepted, indices
    are 1-based and negative ones count from the end, as the format says.  Nothing else is read (no trimesh)."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".npz":
        with np.load(path) as z:
            if "verts" not in z.files or "faces" not in z.files:
                raise RuntimeError(f"load_mesh: {path}: an .npz needs the arrays 'verts' and 'faces' (has {sorted(z.files)})")
            verts, faces = np.asarray(z["verts"], np.float64), np.asarray(z["faces"])
        if faces.dtype.kind not in "iu":
            raise RuntimeError(f"load_mesh: {path}: 'faces' must be integers (got {faces.dtype})")
        faces = faces.astype(np.int64)
    elif ext == ".obj":
        vs, fs = [], []
        with open(path) as f:
            for no, line in enumerate(f, 1):
                w = line.split("#", 1)[0].split()
                if not w:
                    continue
                try:
                    if w[0] == "v":
                        if len(w) < 4:
                            raise ValueError("a vertex needs three coordinates")
                        vs.append([float(w[1]), float(w[2]), float(w[3])])
                    elif w[0] == "f":
                        idx = [int(tok.split("/")[0]) for tok in w[1:]]
                        if len(idx) < 3 or 0 in idx:
                            raise ValueError("a face needs three or more non-zero indices")
                        idx = [i - 1 if i > 0 else len(vs) + i for i in idx]
                        fs.extend([idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1))
                except ValueError as e:
                    raise RuntimeError(f"load_mesh: {path}:{no}: {e}") from e
        verts, faces = np.asarray(vs, np.float64).reshape(-1, 3), np.asarray(fs, np.int64).reshape(-1, 3)
    else:
        raise RuntimeError(f"load_mesh: {path}: only .npz (verts, faces) and Wavefront .obj are read")
    if verts.ndim != 2 or verts.shape[1] != 3 or faces.ndim != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise RuntimeError(f"load_mesh: {path}: need verts [n,3] and at least one face [m,3] (got {verts.shape}, {faces.shape})")
    if faces.min() < 0 or faces.max() >= verts.shape[0]:
        raise RuntimeError(f"load_mesh: {path}: a face index is outside the file's {verts.shape[0]} vertices")
    return verts, faces


def sample_clouds(meshes, n_points, seed, object_indices, even=1, device=None):
    """Point clouds of a call's meshes, made on the device: ``meshes`` an ``ObjectMeshes``, ``object_indices`` every object's GLOBAL
    index (with ``seed`` and the sample index it fixes a draw, whatever else shares the call) -> ``points`` [O,n_points,3] f32 and
    ``face`` [O,n_points] i32 (the local face each point lies on).  ``even`` = 1: the first ``n_points`` area-weighted samples of
    ``ops.mesh_sample`` (the definition is in include/dvq.h under dvq_mesh_sample: the library's own Philox stream, NOT trimesh's).
    ``even`` = F > 1: F * n_points samples (at most ``ops.CLOUD_FPS_MAX_P``), of which ``ops.cloud_fps`` keeps the n_points most
    spread-out, in pick order from sample 0.  Raises on an object without a face with area (or with a range out of bounds), naming it."""
    if not isinstance(meshes, ObjectMeshes):
        raise RuntimeError("sample_clouds: meshes must be an ObjectMeshes")
    n, F, ids = int(n_points), int(even), [int(i) for i in object_indices]
    if len(ids) != meshes.n_objects:
        raise RuntimeError(f"sample_clouds: object_indices must hold one index per mesh (got {len(ids)} for {meshes.n_objects})")
    if n < 1 or F < 1 or n * F > (ops.CLOUD_FPS_MAX_P if F > 1 else ops.MESH_SAMPLE_MAX_S):
        raise RuntimeError(f"sample_clouds: need n_points >= 1, even >= 1 and n_points * even <= {ops.CLOUD_FPS_MAX_P} where even > 1 "
                           f"(<= {ops.MESH_SAMPLE_MAX_S} samples otherwise; got n_points={n} even={F})")
    device = torch.device("cuda" if device is None else device)
    verts, vert_off, faces, face_off = meshes.on(device)
    stream_ids = torch.tensor(ids, dtype=torch.int64, device=device)
    points, face, status, _ = ops.mesh_sample(verts, vert_off, faces, face_off, n * F, int(seed), stream_ids)
    if F > 1:
        sel, _, fps_status = ops.cloud_fps(points, n)
        status = torch.maximum(status, fps_status)
        sel = sel.clamp_(min=0).long()                                           # (a refused pool's -1: the status raises below)
        points, face = torch.gather(points, 1, sel[:, :, None].expand(-1, -1, 3)), torch.gather(face, 1, sel)
    bad = torch.nonzero(status).flatten().tolist()
    if bad:
        raise RuntimeError(f"sample_clouds: object {bad[0]} (global index {ids[bad[0]]}) has no face with area, or a coordinate that "
                           f"is not finite (status {int(status[bad[0]])})")
    return points.contiguous(), face.contiguous()


def _guard_class(no_figure, poor):
    """int32 [B] for ``torch.maximum`` with the class of ``select_keys``, from two boolean [B]: 2 where the row has no figure, else 1
    where it is poor, else 0."""
    zero = torch.zeros_like(no_figure, dtype=torch.int32)
    return torch.where(no_figure, torch.full_like(zero, 2), torch.where(poor, torch.ones_like(zero), zero))


MESH_OUTPUTS = ("n_inside", "depth", "deep_vertex", "deep_face", "mask", "status")


def grasp_mesh(meshes, hand_xyz, obj_of_row, R=None, t=None, want_verts=False, err=None):
    """Penetration depth against the object's MESH from ONE fused kernel (ops.grasp_mesh; the definition is in include/dvq.h under
    dvq_grasp_mesh): ``meshes`` an ``ObjectMeshes`` in the clouds' own frame, ``R`` [B,3,3] / ``t`` [3] what ``ops.transform_clouds``
    got (None for objects in place).  Returns ``n_inside`` [B] i32 (hand vertices inside the mesh; -1 = no figure), ``depth`` [B] f32
    (the largest distance of one of them to the surface, metres), ``deep_vertex`` / ``deep_face`` [B] i32 (that vertex and its nearest
    face, -1 without one), ``mask`` [B,W] i32 (bit v & 31 of word v >> 5: vertex v is inside) and ``status`` [B] i32 (0 fine, 1 the
    object has no face, 3 a hand coordinate is not finite, 4 the object index or its ranges are out of bounds); with ``want_verts``
    also ``vert_d2`` [B,V] f32 and ``vert_face`` [B,V] i32.  ``mesh_stats`` / ``mesh_class`` turn them into the figures written and
    into a selection guard.

    This is the reference's metric/penetration.py figure with a +z ray and a watertight tie rule in place of its oblique ray with
    strict inequalities.  On an open mesh (``meshes.closed[o]`` False) the parity, and with it every figure, is undefined."""
    if not isinstance(meshes, ObjectMeshes):
        raise RuntimeError("grasp_mesh: meshes must be an ObjectMeshes")
    if not torch.is_tensor(hand_xyz) or hand_xyz.dim() != 3:
        raise RuntimeError("grasp_mesh: hand_xyz must be a [B,V,3] tensor")
    verts, vert_off, faces, face_off = meshes.on(hand_xyz.device)
    out = ops.grasp_mesh(hand_xyz.contiguous(), verts, vert_off, faces, face_off, obj_of_row, R, t, want_verts, err=err)
    res = dict(zip(MESH_OUTPUTS, out[:6]))
    if want_verts:
        res.update(vert_d2=out[6], vert_face=out[7])
    return res


def grasp_mesh_volume(topology, meshes, hand_xyz, obj_of_row, R=None, t=None, res=0.001, err=None):
    """Penetration volume against the object's MESH from ONE fused kernel (ops.grasp_mesh_volume; the definition is in include/dvq.h
    under dvq_grasp_mesh_volume): the hand mesh of ``topology`` sealed at its open boundary (``seal_faces``) against the closed
    triangle mesh of each row's object (``meshes`` an ``ObjectMeshes`` in the clouds' own frame), on a lattice of spacing ``res``
    metres in the object's own frame (``R`` [B,3,3], ``t`` [3]: what ``ops.transform_clouds`` got, None for objects in place).  Returns
    ``count`` [B] i32 (voxels in both; -1 = no figure) and ``status`` [B] i32 (0 fine, 1 no voxel of the hand's box is in the object or
    the object has no face, 2 the box has more than 1024 cells on an axis, 3 a vertex is not finite, 4 the object index or its ranges
    are out of bounds).  No depth: the depth against the mesh is ``grasp_mesh``'s.  ``volume_stats`` turns the count into cm^3.

    The solid intersection on the object's own lattice -- a finger in the hollow of a cup shares nothing with the cup, where
    ``grasp_volume``'s hull counts it.  It is NOT the reference's metric/intersect.py figure (trimesh's surface voxels of the object
    inside the hand), no igl / trimesh run pins parity, and on an open mesh (``meshes.closed[o]`` False) it is undefined."""
    if not isinstance(meshes, ObjectMeshes):
        raise RuntimeError("grasp_mesh_volume: meshes must be an ObjectMeshes")
    if not torch.is_tensor(hand_xyz) or hand_xyz.dim() != 3:
        raise RuntimeError("grasp_mesh_volume: hand_xyz must be a [B,V,3] tensor")
    faces, loop_off, loop_vert = topology.sealed()
    verts, vert_off, mfaces, face_off = meshes.on(hand_xyz.device)
    count, status = ops.grasp_mesh_volume(hand_xyz.contiguous(), faces, loop_off, loop_vert, verts, vert_off, mfaces, face_off, obj_of_row,
                                          R, t, res, err=err)
    return {"count": count, "status": status}


def mesh_stats(out):
    """Host side, float64, row by row, from ``grasp_mesh``'s dict (tensors or arrays): ``mesh_depth`` = depth * 100 in cm and
    ``mesh_interior`` = n_inside; two lists, ``None`` where n_inside < 0 (json writes null)."""
    n = _host(out["n_inside"], np.int64).reshape(-1)
    d = _host(out["depth"], np.float64).reshape(-1)
    if n.shape[0] != d.shape[0]:
        raise RuntimeError("mesh_stats: one depth per count")
    return {"mesh_depth": [float(x) * 100.0 if k >= 0 else None for k, x in zip(n, d)],
            "mesh_interior": [int(k) if k >= 0 else None for k in n]}


def mesh_class(out, max_depth_cm):
    """int32 [B] on the device for ``torch.maximum`` with the class of ``select_keys``: 2 where the row of ``grasp_mesh``'s output has
    no figure (n_inside < 0), else 1 where the depth exceeds ``max_depth_cm`` centimetres, else 0.  One fp32 comparison per row,
    ``depth > fp32(max_depth_cm / 100)``: no sum, so nothing depends on which rows share the call."""
    n, depth = out["n_inside"], out["depth"]
    limit = float(max_depth_cm) / 100.0
    if math.isnan(limit) or limit < 0.0:
        raise RuntimeError(f"mesh_class: max_depth_cm must be >= 0 (got {max_depth_cm})")
    over = depth > torch.tensor(limit, dtype=torch.float64, device=depth.device).to(torch.float32) if limit < float("inf") \
        else torch.zeros_like(n, dtype=torch.bool)
    return _guard_class(n < 0, over)


HAND_PARTS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "network", "hand_parts.json")
PART_THRESHOLD = 0.005             # metres: the reference's hard-contact tolerance (penetration_tol, CMap_consistency_loss); untuned


class HandParts(_DeviceTables):
    """A partition of the hand's vertices into parts for ``grasp_parts``: ``labels`` [V] (the part of every vertex, -1 = no part),
    ``names`` (one per part, at most 32; by convention the fingers come first, the thumb as part 0) and the device the int32 label
    vector lives on (None: it follows the first hand it is used with)."""
    _tables = ("labels",)                                     # on(device): the int32 label vector

    def __init__(self, labels, names, device=None):
        lab = _host(labels)
        if lab.ndim != 1 or lab.size < 1 or lab.dtype.kind not in "iu":
            raise RuntimeError("HandParts: labels must be a non-empty 1-D integer array, one label per vertex")
        self.names = [str(n) for n in names]
        if not 1 <= len(self.names) <= ops.GRASP_PARTS_MAX_P:
            raise RuntimeError(f"HandParts: between 1 and {ops.GRASP_PARTS_MAX_P} parts (got {len(self.names)})")
        lab = lab.astype(np.int64)
        self.labels = np.where((lab >= 0) & (lab < len(self.names)), lab, -1).astype(np.int32)
        self.n_verts, self.n_parts = int(lab.size), len(self.names)
        self.sizes = np.bincount(self.labels[self.labels >= 0], minlength=self.n_parts).astype(np.int64)
        self._start_cache(device)

    @classmethod
    def from_json(cls, path=None, device=None):
        """A label table ``{"order": [names], "parts": [[vertex indices], ...]}``, the packaged ``network/hand_parts.json`` (MANO's 778
        vertices: thumb, four fingers, palm) by default, in the file's own order.  A vertex listed by two parts takes the first; the
        vertex count is the file's ``"n_verts"``, or one more than the largest index listed."""
        with open(path or HAND_PARTS_JSON) as f:
            table = json.load(f)
        names, parts = table["order"], table["parts"]
        if len(names) != len(parts):
            raise RuntimeError(f"HandParts.from_json: {len(names)} names for {len(parts)} parts")
        flat = [int(v) for p in parts for v in p]
        if not flat or min(flat) < 0:
            raise RuntimeError("HandParts.from_json: the parts list no vertex, or a negative one")
        n_verts = int(table.get("n_verts", max(flat) + 1))
        if max(flat) >= n_verts:
            raise RuntimeError(f"HandParts.from_json: vertex {max(flat)} of a table of {n_verts} vertices")
        labels = np.full(n_verts, -1, np.int64)
        for q in reversed(range(len(parts))):                   # the first part that lists a vertex is written last
            labels[np.asarray(parts[q], np.int64)] = q
        return cls(labels, names, device)


def grasp_parts(parts, hand_xyz, obj_xyz, threshold=PART_THRESHOLD, want_verts=False):
    """Which parts of the hand touch the object, from ONE fused kernel (ops.grasp_parts; the definition is in include/dvq.h under
    dvq_grasp_parts): every hand vertex finds its nearest object point, and a vertex closer than ``threshold`` METRES (squared once,
    here) touches.  Returns ``part_min`` [B,P] f32 (per part the smallest squared distance, +inf for a part without a vertex),
    ``part_count`` [B,P] i32 (its touching vertices), ``mask`` [B,W] i32 (bit v & 31 of word v >> 5: vertex v touches) and
    ``status`` [B] i32 (1: a coordinate of the row is not finite, and the row has no figure: NaN, -1, 0); with ``want_verts`` also
    ``vert_dist`` [B,V] f32 and ``vert_idx`` [B,V] i32, the bits of ``get_NN(hand_xyz, obj_xyz)``.  ``part_stats`` /
    ``contact_map`` / ``parts_class`` turn them into the figures written and into a selection guard.

    A proximity figure from the hand's side: no contact-force model.  The default threshold is the reference's 5 mm hard-contact
    tolerance and is UNTUNED; its effect on real grasps is NOT measured (no real checkpoint)."""
    threshold = ops._positive("grasp_parts", "threshold", threshold)
    if not torch.is_tensor(hand_xyz) or hand_xyz.dim() != 3 or hand_xyz.shape[1] != parts.n_verts:
        raise RuntimeError(f"grasp_parts: the label table has {parts.n_verts} vertices, the hand "
                           f"{tuple(hand_xyz.shape) if torch.is_tensor(hand_xyz) else type(hand_xyz)}")
    part_min, part_count, mask, status, vert_dist, vert_idx = ops.grasp_parts(hand_xyz.contiguous(), parts.on(hand_xyz.device),
                                                                              parts.n_parts, obj_xyz, threshold * threshold, want_verts)
    out = {"part_min": part_min, "part_count": part_count, "mask": mask, "status": status}
    if want_verts:
        out.update(vert_dist=vert_dist, vert_idx=vert_idx)
    return out


def part_stats(part_min, part_count, status, min_verts=1, n_fingers=5):
    """Host side, float64, row by row, from ``grasp_parts``' ``part_min`` [B,P], ``part_count`` [B,P] and ``status`` [B] (arrays or
    tensors): ``fingers_in_contact`` = how many of the first ``n_fingers`` parts have at least ``min_verts`` touching vertices,
    ``part_contact`` = the P counts, ``part_dist`` = sqrt(part_min) * 100, each part's smallest distance to the cloud in cm.  Three
    lists; ``None`` where the row has no figure (status != 0) and, in ``part_dist``, where the part has no vertex (json writes
    null)."""
    pm = _host(part_min, np.float64)
    pc = _host(part_count, np.int64)
    st = _host(status, np.int64).reshape(-1)
    if pm.ndim != 2 or pm.shape != pc.shape or st.shape[0] != pm.shape[0]:
        raise RuntimeError("part_stats: part_min and part_count [B,P], one status per row")
    min_verts, n_fingers = int(min_verts), int(n_fingers)
    if min_verts < 1 or not 0 <= n_fingers <= pm.shape[1]:
        raise RuntimeError(f"part_stats: min_verts >= 1 and 0 <= n_fingers <= {pm.shape[1]} (got {min_verts}, {n_fingers})")
    fingers, counts, dists = [], [], []
    for m, c, s in zip(pm, pc, st):
        if s != 0:
            fingers.append(None), counts.append(None), dists.append(None)
            continue
        fingers.append(int(np.sum(c[:n_fingers] >= min_verts)))
        counts.append([int(k) for k in c])
        dists.append([float(np.sqrt(x)) * 100.0 if np.isfinite(x) else None for x in m])
    return {"fingers_in_contact": fingers, "part_contact": counts, "part_dist": dists}


def contact_map(mask, n_verts):
    """int64 [V] (numpy): at every vertex, how many of the given rows of ``grasp_parts``' ``mask`` [B,W] touch there."""
    m = np.ascontiguousarray(_host(mask, np.int32)).view(np.uint32)
    n_verts = int(n_verts)
    if m.ndim != 2 or m.shape[1] != (n_verts + 31) // 32:
        raise RuntimeError(f"contact_map: mask must be [B,{(n_verts + 31) // 32}] for {n_verts} vertices (got {m.shape})")
    v = np.arange(n_verts)
    return ((m[:, v >> 5] >> (v & 31).astype(np.uint32)) & np.uint32(1)).astype(np.int64).sum(axis=0)


def parts_class(out, min_fingers, need_thumb, min_verts=1, n_fingers=5):
    """int32 [B] on the device, integer operations only, for ``torch.maximum`` with the class of ``select_keys``: 2 where the row of
    ``grasp_parts``' output has no figure (status != 0), else 1 where fewer than ``min_fingers`` of the first ``n_fingers`` parts have
    at least ``min_verts`` touching vertices, or where ``need_thumb`` is set and part 0 has not, else 0."""
    cnt, status = out["part_count"], out["status"]
    on = cnt[:, :int(n_fingers)] >= int(min_verts)
    poor = on.sum(dim=1) < int(min_fingers)
    if need_thumb:
        poor = poor | ~on[:, 0]
    return _guard_class(status != 0, poor)


OBJECT_CONTACT_OUTPUTS = ("touch", "inside", "dmin", "near_sum", "n_valid", "row_status")


def object_contact(topology, hand_xyz, obj_xyz, O, K, rows=None, contact_threshold=0.02 ** 2, err=None):
    """Where on the object its grasps land, from ONE fused kernel (ops.segment_contact; the definition is in include/dvq.h under
    dvq_segment_contact): object o's grasps are the ``K`` rows ``rows[o*K:(o+1)*K]`` of hand_xyz [B,V,3] / obj_xyz [B,N,3] (any strides,
    read in place; ``rows=None``: rows o*K .. o*K+K-1 of a batch of O*K), each row's cloud the object as that grasp sees it -- point p
    is point p of the object whatever the row's rotation.  Returns ``touch`` [O,N] i32 (the grasps whose hand comes closer to point p
    than the threshold, a SQUARED distance as in ``grasp_scores``), ``inside`` [O,N] i32 (the grasps with p inside the hand),
    ``dmin`` [O,N] f32 (the smallest squared distance), ``near_sum`` [O,N] f32 (the summed distances of the touching grasps),
    ``n_valid`` [O] i32 and ``row_status`` [O*K] i32 (1: a coordinate of the row is not finite; such a row takes part in nothing).
    ``object_contact_stats`` turns them into the figures written.

    A proximity figure at the scores' 2 cm threshold, which is UNTUNED; its effect on real grasps is NOT measured."""
    out = ops.segment_contact(hand_xyz.contiguous(), topology.faces, topology.vf_off, topology.vf_face, obj_xyz, O, K, rows,
                              contact_threshold, err)
    return dict(zip(OBJECT_CONTACT_OUTPUTS, out))


def object_contact_stats(touch, inside, dmin, near_sum, n_valid):
    """Host side, float64, object by object, from ``object_contact``'s ``touch``, ``inside``, ``dmin``, ``near_sum`` [O,N] and
    ``n_valid`` [O] (arrays or tensors) -> one dict per object: ``grasps`` = n_valid, ``coverage`` = the share of points at least one
    grasp touches, ``entropy`` = -sum q ln q over q = touch / sum(touch) (natural logarithm as diversity.py; None when nothing is
    touched), ``min_dist`` = 100 sqrt(dmin) per point in cm (None where the object has no valid grasp) and ``contact_dist`` =
    100 near_sum / touch per point in cm (None where touch == 0).  ``inside`` only has to match in shape."""
    tc, dm, ns = _host(touch, np.int64), _host(dmin, np.float64), _host(near_sum, np.float64)
    nv = _host(n_valid, np.int64).reshape(-1)
    if tc.ndim != 2 or not (tc.shape == _host(inside).shape == dm.shape == ns.shape) or nv.shape[0] != tc.shape[0]:
        raise RuntimeError("object_contact_stats: touch, inside, dmin and near_sum [O,N], one n_valid per object")
    out = []
    for t, d, s, n in zip(tc, dm, ns, nv):
        if n < 0:
            raise RuntimeError("object_contact_stats: an object without a figure (a rows entry was out of bounds)")
        total = int(t.sum())
        entropy = None
        if total > 0:
            q = t[t > 0].astype(np.float64) / float(total)
            entropy = float(-(q * np.log(q)).sum())
        out.append({"grasps": int(n), "coverage": float(np.count_nonzero(t >= 1)) / t.shape[0], "entropy": entropy,
                    "min_dist": [float(np.sqrt(x)) * 100.0 for x in d] if n > 0 else [None] * t.shape[0],
                    "contact_dist": [100.0 * float(x) / int(k) if k > 0 else None for x, k in zip(s, t)]})
    return out


def pseudo_cmap(d2):
    """The reference's 0-1 contact map (utils/utils.py get_pseudo_cmap: 1 - 2 (sigmoid(2 * 100 * distance) - 0.5)) of SQUARED
    distances in metres, e.g. ``object_contact``'s ``dmin``: float64 on the host, 1 at the hand and falling towards 0 away from it
    (+inf gives 0).  Not evaluated in the kernel: its bits would hang on an exp."""
    d = np.sqrt(_host(d2, np.float64)) * 100.0
    with np.errstate(over="ignore"):
        return 1.0 - 2.0 * (1.0 / (1.0 + np.exp(-2.0 * d)) - 0.5)


SELF_REACH, SELF_MARGIN, SELF_SEAM = 0.01, 0.001, 2    # metres, metres, edge rings: calibrated against false alarms only; untuned


class SelfTable(_DeviceTables):
    """What ``grasp_self`` tests a hand of ``parts`` (a ``HandParts``) against itself with: ``source`` int32 [V], 0 at the SEAM
    vertices -- parts of one hand are joined surfaces, and next to a join the vector to the nearest vertex of the other part is
    tangent to the surface, so the sign of the interior test is noise there: a vertex that an edge of ``faces`` joins to a vertex of
    a different label, or that lies within ``seam`` - 1 further edge rings of such a vertex, never counts as a source (it remains a
    target; ``seam`` = 0: no seam) -- and ``pairs``, P words: bit b of ``pairs[a]`` = part a's vertices are tested against part
    b's.  The first ``n_fingers`` parts are tested against one another and, with ``palm``, against every remaining part as well
    (the remaining parts are sources of nothing).  ``pairs=`` / ``source=`` replace the derived ones outright."""

    def __init__(self, parts, faces, seam=SELF_SEAM, palm=True, n_fingers=5, pairs=None, source=None, device=None):
        if not isinstance(parts, HandParts):
            raise RuntimeError("SelfTable: parts must be a HandParts")
        V, P = parts.n_verts, parts.n_parts
        seam, n_fingers = int(seam), int(n_fingers)
        if seam < 0 or n_fingers < 0:
            raise RuntimeError(f"SelfTable: seam >= 0 and n_fingers >= 0 (got {seam}, {n_fingers})")
        n_fingers = min(n_fingers, P)                           # a table of fewer parts: all of them are fingers
        self.parts, self.seam, self.palm, self.n_fingers = parts, seam, bool(palm), n_fingers
        if source is None:
            f = _host(faces, np.int64).reshape(-1, 3)
            if f.size and (f.min() < 0 or f.max() >= V):
                raise RuntimeError(f"SelfTable: a face index is outside [0, {V})")
            edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
            near = np.zeros(V, bool)
            if seam >= 1:
                cut = edges[parts.labels[edges[:, 0]] != parts.labels[edges[:, 1]]]
                near[cut.reshape(-1)] = True
                for _ in range(seam - 1):                       # one more edge ring
                    grow = near.copy()
                    grow[edges[near[edges[:, 1]], 0]] = True
                    grow[edges[near[edges[:, 0]], 1]] = True
                    near = grow
            src = (~near).astype(np.int32)
        else:
            src = _host(source)
            if src.shape != (V,) or src.dtype.kind not in "iub":
                raise RuntimeError(f"SelfTable: source must be an integer array [{V}] (got {src.dtype} {src.shape})")
            src = (src != 0).astype(np.int32)
        self.source = src
        self.n_seam = int(V - src.sum())
        if pairs is None:
            fingers = (1 << n_fingers) - 1
            rest = ((1 << P) - 1) & ~fingers if palm else 0
            words = [(fingers & ~(1 << a)) | rest if a < n_fingers else 0 for a in range(P)]
        else:
            words, a = ops._pair_words("SelfTable", pairs, P)
            if a is not None:
                raise RuntimeError(f"SelfTable: pairs[{a}] = {words[a]:#x} names a part at or above {P}, or part {a} itself")
        self.pairs = np.asarray(words, dtype=np.uint32)
        self._start_cache(device)

    def _upload(self, device):
        """(labels, source) int32 [V]; the labels are ``parts``' own copy."""
        return self.parts.on(device), torch.from_numpy(self.source).to(device)


def grasp_self(topology, table, hand_xyz, reach=SELF_REACH, margin=SELF_MARGIN):
    """Finger-to-finger (and finger-to-palm) collision of hands, from ONE fused kernel (ops.grasp_self; the definition is in
    include/dvq.h under dvq_grasp_self): every source vertex of ``table`` (a ``SelfTable``) finds its nearest vertex among the parts
    its own part is tested against, and PENETRATES when that vertex lies within ``reach`` METRES (squared once, here) and the source
    is more than ``margin`` metres behind its tangent plane.  Returns ``pen_count`` [B,P] i32, ``pen_depth`` [B,P] f32 (metres, +0.0
    without a penetrating vertex), ``gap_min`` [B,P] f32 (squared metres, +inf for a part without a source), ``pair_bits`` [B,P] i32
    (bit b: part b was hit), ``mask`` [B,W] i32 (bit v & 31 of word v >> 5: vertex v penetrates) and ``status`` [B] i32 (1: a
    coordinate of the row is not finite, and the row has no figure: -1, NaN, NaN, 0, 0).  ``self_stats`` / ``self_class`` turn them
    into the figures written and into a selection guard.

    A proximity figure in the style of ``get_interior``, not a mesh-mesh intersection: vertices only, so a thin crossing between
    vertices is missed.  The defaults are calibrated only against false alarms on 48 posed hands of the real hand model and are
    UNTUNED otherwise; the effect on real grasps is NOT measured (no real checkpoint)."""
    reach, margin = ops._positive("grasp_self", "reach", reach), ops._non_negative("grasp_self", "margin", margin)
    if not isinstance(table, SelfTable):
        raise RuntimeError("grasp_self: table must be a SelfTable")
    V = table.parts.n_verts
    if not torch.is_tensor(hand_xyz) or hand_xyz.dim() != 3 or hand_xyz.shape[1] != V or topology.n_verts != V:
        raise RuntimeError(f"grasp_self: the table has {V} vertices, the topology {topology.n_verts}, the hand "
                           f"{tuple(hand_xyz.shape) if torch.is_tensor(hand_xyz) else type(hand_xyz)}")
    labels, source = table.on(hand_xyz.device)
    out = ops.grasp_self(hand_xyz.contiguous(), topology.faces, topology.vf_off, topology.vf_face, labels, source, table.parts.n_parts,
                         table.pairs, reach * reach, margin)
    return dict(zip(SELF_OUTPUTS, out))


SELF_OUTPUTS = ("pen_count", "pen_depth", "gap_min", "pair_bits", "mask", "status")
SELF_FIELDS = ("self_penetrating", "self_part_penetrating", "self_depth", "self_pairs", "self_clearance")


def self_stats(out):
    """Host side, float64, row by row, from ``grasp_self``'s dict (tensors or arrays): ``self_penetrating`` = the row's penetrating
    vertices, ``self_part_penetrating`` = the P counts, ``self_depth`` = the largest depth over the parts in cm, ``self_pairs`` = the
    sorted [a, b] pairs "a vertex of part a penetrates part b", ``self_clearance`` = sqrt of the smallest ``gap_min`` in cm (None
    when no part has a source with a target).  Five lists; ``None`` where the row has no figure (status != 0)."""
    cnt, dep, gap = _host(out["pen_count"], np.int64), _host(out["pen_depth"], np.float64), _host(out["gap_min"], np.float64)
    bits = _host(out["pair_bits"], np.int64) & 0xffffffff
    st = _host(out["status"], np.int64).reshape(-1)
    if cnt.ndim != 2 or not (cnt.shape == dep.shape == gap.shape == bits.shape) or st.shape[0] != cnt.shape[0]:
        raise RuntimeError("self_stats: pen_count, pen_depth, gap_min and pair_bits [B,P], one status per row")
    P = cnt.shape[1]
    res = {k: [] for k in SELF_FIELDS}
    for c, d, g, w, s in zip(cnt, dep, gap, bits, st):
        if s != 0:
            for k in SELF_FIELDS:
                res[k].append(None)
            continue
        res["self_penetrating"].append(int(c.sum()))
        res["self_part_penetrating"].append([int(k) for k in c])
        res["self_depth"].append(float(d.max()) * 100.0)
        res["self_pairs"].append([[a, b] for a in range(P) for b in range(P) if (int(w[a]) >> b) & 1])
        low = float(g.min())
        res["self_clearance"].append(float(np.sqrt(low)) * 100.0 if np.isfinite(low) else None)
    return res


def self_class(out, max_verts):
    """int32 [B] on the device, integer operations only, for ``torch.maximum`` with the class of ``select_keys``: 2 where the row of
    ``grasp_self``'s output has no figure (status != 0), else 1 where more than ``max_verts`` vertices penetrate, else 0."""
    cnt, status = out["pen_count"], out["status"]
    over = cnt.sum(dim=1) > int(max_verts)
    return _guard_class(status != 0, over)


SELECT_BY = ("penetration", "log_prob", "stability")


def select_keys(scores, select_by, min_contact, log_prob=None, max_penetration=float("inf")):
    """(cls int32 [B], key f32 [B]) for ``ops.segment_topk`` -- smaller is better, row by row:
    ``"penetration"``: cls 2 where the penetration is NaN, else 1 where the hand touches fewer than ``min_contact`` object
    points (a hand far from the object penetrates nothing), else 0; key = penetration.
    ``"log_prob"``: cls 2 where it is NaN, else 0; key = -log_prob (likeliest first).
    ``"stability"`` (``scores`` of ``grasp_stability``): cls 2 where the penetration is NaN, else 1 where the hand touches fewer than
    ``min_contact`` object points or penetrates more than ``max_penetration``, else 0; key = the kernel's ``key``.  Ranking by
    stability alone rewards hands that wrap the object by sinking into it: ``max_penetration`` (default +inf: no limit) is the
    caller's guard against that."""
    if select_by == "stability":
        pen = scores["penetration"]
        poor = (scores["n_contact"] < int(min_contact)) | (pen > float(max_penetration))
        cls = torch.where(torch.isnan(pen), 2, torch.where(poor, 1, 0))
        return cls.to(torch.int32), scores["key"]
    if select_by == "penetration":
        pen = scores["penetration"]
        cls = torch.where(torch.isnan(pen), 2, torch.where(scores["n_contact"] < int(min_contact), 1, 0))
        return cls.to(torch.int32), pen
    if select_by == "log_prob":
        if log_prob is None:
            raise RuntimeError("select_keys: select_by='log_prob' needs the grasps' log_prob")
        return torch.where(torch.isnan(log_prob), 2, 0).to(torch.int32), -log_prob
    raise RuntimeError(f"select_keys: select_by must be one of {SELECT_BY} (got {select_by!r})")


# ------------------------------------------------------------------------------------------ gradient refinement (the reference's TTT loop)
TTT_W_PEN = 840.0                  # utils/loss.py TTT_loss and gen_diverse_grasp_obman.py:69-94: 7 * (120 * penetration)
TTT_W_CON = 7500.0                 # 1 * (2.5 * 3000 * contact); both are the reference's constants, untuned here
TTT_LR = 6.25e-6                   # SGD(lr=6.25e-6, momentum=0.8), 300 steps in the reference
TTT_MOMENTUM = 0.8
TTT_MAX_STEPS = 1000


class ContactTargets(_DeviceTables):
    """The hand vertices the contact term of ``ttt_terms`` measures distances to (the reference's ``prior_idx`` subset of
    ``Contact_loss``): built from a list of vertex indices or from a boolean mask of ``n_verts`` entries; ``from_json`` reads a JSON
    file that holds a list of indices.  ``on(device)`` is the int32 flag vector [n_verts] the kernel takes (uploaded once per device).
    An empty set is refused; "every vertex" is ``targets=None`` at the call, not an object of this class."""
    _tables = ("flags",)

    def __init__(self, spec, n_verts=778, device=None):
        a = _host(spec)
        n_verts = int(n_verts)
        if a.dtype == np.bool_:
            if a.ndim != 1 or a.size != n_verts:
                raise RuntimeError(f"ContactTargets: a mask must have {n_verts} entries (got shape {a.shape})")
            idx = np.flatnonzero(a)
        else:
            if a.ndim != 1 or (a.size and a.dtype.kind not in "iu"):
                raise RuntimeError("ContactTargets: expected a 1-D list of vertex indices or a boolean mask")
            idx = np.unique(a.astype(np.int64))
        if idx.size == 0:
            raise RuntimeError("ContactTargets: the set is empty (every vertex is targets=None)")
        if idx.min() < 0 or idx.max() >= n_verts:
            raise RuntimeError(f"ContactTargets: a vertex index lies outside [0, {n_verts})")
        self.n_verts = n_verts
        self.indices = idx.astype(np.int64)
        self.flags = np.zeros(n_verts, np.int32)
        self.flags[idx] = 1
        self._start_cache(device)

    @classmethod
    def from_json(cls, path, n_verts=778, device=None):
        """A JSON file holding a list of vertex indices."""
        with open(path) as f:
            table = json.load(f)
        if not isinstance(table, list) or not all(isinstance(v, int) and not isinstance(v, bool) for v in table):
            raise RuntimeError(f"ContactTargets.from_json: {path} must hold a list of vertex indices")
        return cls(np.asarray(table, np.int64), n_verts, device)


def _ttt_flags(what, targets, topology, hand_xyz):
    if targets is None:
        return None
    if not isinstance(targets, ContactTargets):
        raise RuntimeError(f"{what}: targets must be a ContactTargets or None")
    if targets.n_verts != topology.n_verts or hand_xyz.shape[1] != targets.n_verts:
        raise RuntimeError(f"{what}: the targets name {targets.n_verts} vertices, the topology {topology.n_verts}, the hand "
                           f"{hand_xyz.shape[1]}")
    return targets.on(hand_xyz.device)


class _TttFunction(torch.autograd.Function):
    """``ops.grasp_ttt`` as autograd sees it: the forward launch computes no gradient; the backward is a second launch with the
    upstream gradients as the two weights, which recomputes the forward from the hand and the cloud -- they are all that is saved.
    The masks and indices are constants (the reference indexes with booleans); no gradient for the cloud; no double backward."""

    @staticmethod
    def forward(ctx, topology, flags, threshold, hand_xyz, obj_xyz):
        ctx.topology, ctx.flags, ctx.threshold = topology, flags, threshold
        ctx.set_materialize_grads(False)                    # an output the loss does not use arrives as None: weight 0
        ctx.save_for_backward(hand_xyz, obj_xyz)
        pen, con, n_in, n_ct, _ = ops.grasp_ttt(hand_xyz, topology.faces, topology.vf_off, topology.vf_face, obj_xyz, flags,
                                                contact_threshold=threshold)
        ctx.mark_non_differentiable(n_in, n_ct)
        return pen, con, n_in, n_ct

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_pen, g_con, _g_in=None, _g_ct=None):
        if (g_pen is None and g_con is None) or not ctx.needs_input_grad[3]:
            return (None,) * 5
        hand_xyz, obj_xyz = ctx.saved_tensors
        B = hand_xyz.shape[0]
        weight = lambda g: (torch.zeros(B, dtype=torch.float32, device=hand_xyz.device) if g is None
                            else g.to(torch.float32).contiguous())
        topo = ctx.topology
        grad = ops.grasp_ttt(hand_xyz, topo.faces, topo.vf_off, topo.vf_face, obj_xyz, ctx.flags, weight(g_pen), weight(g_con),
                             want_grad=True, contact_threshold=ctx.threshold)[4]
        return None, None, None, grad, None


def ttt_terms(topology, hand_xyz, obj_xyz, targets=None, contact_threshold=0.02 ** 2):
    """The two terms of the reference's test-time loss (utils/loss.py: TTT_loss), unweighted and per grasp, from ONE fused kernel
    (ops.grasp_ttt; the definition is in include/dvq.h under dvq_grasp_ttt): ``penetration`` [B] f32, ``n_interior`` [B] i32 and
    ``n_contact`` [B] i32 are the bits of ``grasp_scores``; ``contact_sum`` [B] f32 is the sum, over the object points within the
    threshold of the hand, of the squared distance to the nearest vertex of ``targets`` (a ``ContactTargets``; None = every vertex) --
    the hand-centric ``Contact_loss`` before its mean.  When grad is enabled and ``hand_xyz`` requires it, ``penetration`` and
    ``contact_sum`` are differentiable with respect to the hand (once; the masks and nearest-vertex indices are constants, nothing
    flows to the cloud): the backward is a second launch of the kernel.  Otherwise only the forward launch runs."""
    flags = _ttt_flags("ttt_terms", targets, topology, hand_xyz)
    hand = hand_xyz.contiguous()
    if torch.is_grad_enabled() and hand.requires_grad:
        pen, con, n_in, n_ct = _TttFunction.apply(topology, flags, float(contact_threshold), hand, obj_xyz.detach())
    else:
        pen, con, n_in, n_ct, _ = ops.grasp_ttt(hand, topology.faces, topology.vf_off, topology.vf_face, obj_xyz, flags,
                                                contact_threshold=contact_threshold)
    return {"penetration": pen, "contact_sum": con, "n_interior": n_in, "n_contact": n_ct}


def _ttt_combine(pen, con, n_ct, w_pen, w_con):
    scale = torch.full_like(pen, float(w_con)) / n_ct.clamp(min=1).to(pen.dtype)       # fp32 division, row by row
    return pen * float(w_pen) + con * scale


def ttt_loss(topology, hand_xyz, obj_xyz, targets=None, w_pen=TTT_W_PEN, w_con=TTT_W_CON, contact_threshold=0.02 ** 2):
    """[B]: ``w_pen * penetration + w_con * contact_sum / max(n_contact, 1)`` of ``ttt_terms`` -- with the defaults (the reference's
    7 * 120 and 1 * 2.5 * 3000) and B = 1, the way the reference calls it, this is utils/loss.py's TTT_loss without the ContactNet
    term.  DEVIATION for B > 1: every row is normalised by its OWN contact count (the reference's mean runs over the batch's contact
    points and its penetration term divides by B), which keeps a grasp's loss and gradient independent of the batch it is in.  A row
    without a contact point has contact term 0 (the reference divides 0 by 0 there).  Differentiable through ``ttt_terms``."""
    t = ttt_terms(topology, hand_xyz, obj_xyz, targets, contact_threshold)
    return _ttt_combine(t["penetration"], t["contact_sum"], t["n_contact"], w_pen, w_con)


def ttt_value_and_grad(topology, hand_xyz, obj_xyz, targets=None, w_pen=TTT_W_PEN, w_con=TTT_W_CON, contact_threshold=0.02 ** 2,
                       want_grad=True):
    """``(ttt_loss [B], d sum(ttt_loss) / d hand_xyz [B,V,3])`` from ONE launch (the kernel divides the contact weight by the row's
    contact count itself): what ``refine_ttt`` calls per step.  The bits of ``ttt_loss`` and of its autograd gradient.  No graph is
    recorded.  ``want_grad=False`` skips the gradient phase and returns None for it."""
    flags = _ttt_flags("ttt_value_and_grad", targets, topology, hand_xyz)
    hand = hand_xyz.detach().contiguous()
    B = hand.shape[0]
    wp = torch.full((B,), float(w_pen), dtype=torch.float32, device=hand.device)
    wc = torch.full((B,), float(w_con), dtype=torch.float32, device=hand.device)
    pen, con, _, n_ct, grad = ops.grasp_ttt(hand, topology.faces, topology.vf_off, topology.vf_face, obj_xyz.detach(), flags, wp, wc,
                                            mean_contact=True, want_grad=want_grad, contact_threshold=contact_threshold)
    return _ttt_combine(pen, con, n_ct, w_pen, w_con), grad


def refine_ttt(layer, topology, params61, obj_xyz, steps, lr=TTT_LR, momentum=TTT_MOMENTUM, targets=None, w_pen=TTT_W_PEN,
               w_con=TTT_W_CON, keep_best=True):
    """Gradient refinement of grasps, the reference's test-time loop (gen_diverse_grasp_obman.py:69-94): ``steps`` steps of
    ``SGD(lr, momentum)`` on the [B,61] MANO parameters (betas 10 | global_orient 3 | hand_pose 45 | transl 3) down ``ttt_loss``.
    Per step: ``layer`` poses the hands, ``ttt_value_and_grad`` gives the loss and its gradient at the vertices in one launch,
    ``ops.mano_backward`` carries it to the 61 columns, and the update is torch.optim.SGD's (buf = g on the first step,
    buf = momentum * buf + g after it, p -= lr * buf).  Returns ``params`` [B,61], ``loss0`` [B] (iterate 0), ``loss`` [B] and
    ``iter`` [B] i32 (of the iterate returned).  With ``keep_best`` every row keeps its iterate of lowest loss among 0 .. steps, the
    earliest among equals; without it the last iterate is returned, as the reference does.  A row whose loss is NaN at iterate 0,
    or whose parameters become non-finite, comes back as given with ``iter = 0``.  ``steps = 0`` returns the input's bits.  Every
    row is refined on its own (``ttt_loss``'s per-row normalisation): the result does not depend on the batch.  The constants are
    the reference's and untuned here."""
    steps = int(steps)
    if not 0 <= steps <= TTT_MAX_STEPS:
        raise RuntimeError(f"refine_ttt: steps must lie between 0 and {TTT_MAX_STEPS} (got {steps})")
    lr, momentum = float(lr), float(momentum)
    if not (0.0 <= lr < float("inf") and 0.0 <= momentum < 1.0):
        raise RuntimeError(f"refine_ttt: lr must be finite and >= 0, momentum in [0, 1) (got {lr}, {momentum})")
    if params61.dim() != 2 or params61.shape[1] != 61 or params61.dtype != torch.float32:
        raise RuntimeError(f"refine_ttt: params61 must be float32 [B,61] (got {params61.dtype} {tuple(params61.shape)})")
    pose = lambda q: layer(betas=q[:, :10], global_orient=q[:, 10:13], hand_pose=q[:, 13:58], transl=q[:, 58:61]).vertices
    with torch.no_grad():
        given = params61.detach()
        p = given.clone()
        loss0, grad = ttt_value_and_grad(topology, pose(p), obj_xyz, targets, w_pen, w_con, want_grad=steps > 0)
        loss = loss0
        best_p, best_loss = p.clone(), loss0.clone()
        best_iter = torch.zeros(p.shape[0], dtype=torch.int32, device=p.device)
        buf = None
        for k in range(1, steps + 1):
            g_betas, g_pose, g_orient, g_transl = ops.mano_backward(layer._packed, p[:, :10], p[:, 13:58], p[:, 10:13], p[:, 58:61], grad)
            g = torch.cat((g_betas, g_orient, g_pose, g_transl), dim=1)          # the 61 columns' order
            if buf is None:
                buf = g.clone()
            else:
                buf.mul_(momentum).add_(g)
            p.add_(buf, alpha=-lr)
            loss, grad = ttt_value_and_grad(topology, pose(p), obj_xyz, targets, w_pen, w_con, want_grad=k < steps)
            if keep_best:
                better = loss < best_loss                   # strictly: the earliest among equals; never true against a NaN
                best_p = torch.where(better[:, None], p, best_p)
                best_loss = torch.where(better, loss, best_loss)
                best_iter = torch.where(better, torch.full_like(best_iter, k), best_iter)
        if not keep_best:
            best_p, best_loss, best_iter = p, loss, torch.full_like(best_iter, steps)
        lost = ~torch.isfinite(p).all(dim=1) | torch.isnan(loss0)
        best_p = torch.where(lost[:, None], given, best_p)
        best_loss = torch.where(lost, loss0, best_loss)
        best_iter = torch.where(lost, torch.zeros_like(best_iter), best_iter)
    return {"params": best_p, "loss0": loss0, "loss": best_loss, "iter": best_iter}

