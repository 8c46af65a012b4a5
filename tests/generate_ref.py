"""The pipeline of generate.generate_for_objects restated from the stage references -- test infrastructure.  ``compose`` takes the
tensors of a PLAIN run (no option on; with beam search: only ``beam_width`` / ``beam_poses`` on) and returns what the call must return
with the options on.  The thirteen options: best-of-M (``candidates``, ``select_by``), the diverse pool, the translation push-out,
diversity, stability, volume -- and the rigid push-out (``refine_spin``), the articulated push-out with its revert guard
(``refine_curl``, ``refine_max_curl``), gradient refinement (``ttt_*``), beam search (``beam_width``, ``beam_poses``), hand-side contact
(``parts``, ``min_fingers``, ``need_thumb``), self-collision (``self_collision``, ``max_self_verts``) and mesh depth (``mesh_depth``,
``max_mesh_depth``, ``object_meshes``).

The order is the one generate_for_objects' docstring promises:

    1 row clouds = R | t applied to the object (the ``transform`` given; ops.transform_cloud by default)
    2 push-out of ALL rows: grasp_refine_ref; with refine_spin grasp_refine_rigid_ref about the root joint of the first posed pass; with
      refine_curl grasp_refine_fingers_ref about the root joint and the rig's knuckles, the hands posed again, scored, and the rows that
      came out worse reverted (the guard, written out in ``push_out``)
    3 MANO again (the ``pose`` given)
    3b gradient refinement (the ``tune`` given) of the pushed-out parameters against the rows' own clouds, and MANO again
    4 scores or wrench sums of the final hands               5 the figures of the final hands: volume (hull of the UNROTATED cloud, the
      rows' R | t), parts (against the row's cloud), self-collision, mesh depth (the object's mesh in the cloud's own frame, R | t)
    6 classes and keys (contact.select_keys on CPU tensors; the guards of volume, parts, self and mesh joined by np.maximum)
    7 top-k, or the pool and its farthest-point picks          8 k-means of the kept parameters          9 the JSON, keys in order

What is checked against what.  INDEPENDENT, bit-exact CPU references: the three push-outs (tests/grasp_refine_ref, grasp_refine_rigid_ref,
grasp_refine_fingers_ref), the scores (grasp_score_ref), the wrench sums (grasp_wrench_ref), volume (grasp_volume_ref), parts
(grasp_parts_ref, with its contact_map and parts_class), self-collision (grasp_self_ref, with its seam_sources, default_pairs and
self_class), mesh depth (grasp_mesh_ref; the class rule is written out in ``mesh_class``), top-k and the diverse picks
(grasp_score_ref.segment_topk, diverse_select_ref), k-means (segment_kmeans_ref); the revert guard, the order of stages, rows, frames,
dict keys and JSON fields are written out here.  PLUMBING only, through the package's own host formulas (each has float64 twins and
tests of its own in its stage's test file): contact.select_keys, hull_planes, volume_limit, wrench_stats, volume_stats, part_stats,
self_stats, mesh_stats, diversity.kmeans_init, and the write-back of the two newer push-outs into the parameters --
contact.compose_orient, compose_finger_pose and quat_axis_angle, fed with the REFERENCE's quaternions on the device of the plain run
(so that a float64 sine is the same sine) -- exactly as wrench_stats is used: the right rows' quaternions must reach the formula and its
result the right columns.  PLUMBING through device-backed callables the test supplies: ``transform`` (step 1), ``pose`` (MANO, which has
its own float64 tests) and ``tune`` (contact.refine_ttt: the MANO backward has no bit-exact CPU restatement, tests/test_grasp_ttt.py
owns its arithmetic) -- compose checks that ``tune`` gets the pushed-out parameters and the row's own cloud, that everything after it
sees its output, that its three figures reach the dict and the JSON, and that after an articulated push-out the scores are those of
the tuned hands.  compose calls none of contact.grasp_scores, refine_translation, refine_rigid, refine_fingers, grasp_stability,
grasp_volume, grasp_parts, grasp_self, grasp_mesh, parts_class, self_class, mesh_class, contact_map, ops.segment_topk,
segment_diverse, segment_kmeans.

The JSON's field order, as generate.py builds it.  With candidates: recon_params, R_list, trans_list, r_list, candidate, penetration,
n_interior, n_contact, [log_prob], [force_residual, torque_residual, min_sv, stability_key], [rank, novelty], [refine_offset,
refine_iter, refine_rotation, refine_curl, refine_reverted], [diversity], [penetration_volume, penetration_depth, volume_voxels],
[fingers_in_contact, part_contact, part_dist, hand_contact_map], [the five self fields], [mesh_depth, mesh_interior, mesh_closed,
mesh_penetration_map], [ttt_loss0, ttt_loss, ttt_iter], [beam_pose, beam_rank, beam_duplicate_of].  Without: recon_params, R_list,
trans_list, r_list, [log_prob], [the refine fields], [penetration, n_interior, n_contact] (with a push-out or stability), [the four
stability fields], [the three volume fields], [diversity], [parts], [self], [mesh], [ttt], [beam]."""
import json

import numpy as np
import torch

from dvqvae_amd import contact, diversity, generate, synth

import diverse_select_ref as dref
import grasp_mesh_ref as mref
import grasp_parts_ref as pref
import grasp_refine_fingers_ref as fref
import grasp_refine_ref as rref
import grasp_refine_rigid_ref as gref_rigid
import grasp_score_ref as sref
import grasp_self_ref as cref
import grasp_volume_ref as vref
import grasp_wrench_ref as wref
import segment_kmeans_ref as kref

F32 = np.float32
INF = float("inf")

OFF = dict(num_grasp=None, rotate=False, proxies=False, rows_per_call=16384, temperature=1.0, top_k=0, log_prob=False, candidates=0,
           select_by="penetration", min_contact=1, diverse_pool=0, diverse_space="params", refine_steps=0, refine_push=1.0,
           refine_pull=0.25, diversity=0, stability=False, max_penetration=INF, torque_length=0.1, volume=False, volume_res=0.001,
           max_volume=INF, parts=False, part_threshold=0.005, part_min_verts=1, min_fingers=0, need_thumb=False, hand_parts=None,
           refine_spin=0.0, refine_curl=0.0, refine_max_curl=0.35, self_collision=False, self_reach=0.01, self_margin=0.001, self_seam=2,
           self_palm=True, max_self_verts=None, object_meshes=None, mesh_depth=False, max_mesh_depth=INF, ttt_steps=0, ttt_lr=6.25e-6,
           ttt_momentum=0.8, ttt_w_pen=840.0, ttt_w_con=7500.0, ttt_prior=None, ttt_keep_best=True, beam_width=0, beam_poses=1)
"""Every keyword of generate_for_objects at its documented "off" value; ``num_grasp`` (the rows kept per object) has none."""

STABILITY_FIELDS = ("force_residual", "torque_residual", "min_sv", "stability_key")
VOLUME_FIELDS = ("penetration_volume", "penetration_depth", "volume_voxels")
VOLUME_PIECES = ("count", "depth", "status")
PARTS_FIELDS = ("fingers_in_contact", "part_contact", "part_dist", "hand_contact_map")
PARTS_PIECES = ("part_min", "part_count", "mask", "status")
SELF_FIELDS = ("self_penetrating", "self_part_penetrating", "self_depth", "self_pairs", "self_clearance")
SELF_PIECES = ("pen_count", "pen_depth", "gap_min", "pair_bits", "mask", "status")
MESH_FIELDS = ("mesh_depth", "mesh_interior", "mesh_closed", "mesh_penetration_map")
MESH_PIECES = ("n_inside", "depth", "mask")
REFINE_PIECES = ("offset", "iter", "rotation", "curl", "reverted")           # the order of the dict keys and JSON fields "refine_" + name
TTT_PIECES = ("loss0", "loss", "iter")
BEAM_PIECES = ("beam_pose", "beam_rank", "beam_duplicate_of")
NESTED = ("scores", "volume", "volume_scores", "parts", "part_scores", "self", "self_scores", "mesh", "mesh_scores")
SCORE_NAMES = ("penetration", "n_interior", "n_contact")


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def api_keywords(options):
    """The keyword arguments of generate_for_objects for ``options`` (``num_grasp`` and ``rotate`` are positional there)."""
    return {k: v for k, v in options.items() if k not in ("num_grasp", "rotate")}


def device_transform(device):
    """Step 1 through ops.transform_cloud (its own numpy test: tests/test_gpu_parity.py), as
    test_grasp_select.py::test_best_of_m_scores_are_the_scores_of_the_plain_hands does it: obj [4,N], R [M,3,3], t [3] -> [M,N,3]."""
    from dvqvae_amd import ops

    def transform(obj4n, R, t):
        cloud = ops.transform_cloud(obj4n.to(device).contiguous(), torch.from_numpy(np.ascontiguousarray(R, F32)).to(device),
                                    torch.from_numpy(np.ascontiguousarray(t, F32)).to(device))
        return cloud[:, :3].transpose(1, 2).contiguous().cpu().numpy()
    return transform


class Hand:
    """What the seven newer options need of the hand model beside its faces: ``layer`` (the MANO layer, for contact.compose_finger_pose),
    ``rig`` (a contact.FingerRig: the fingers' vertices, weights and knuckle joints) and ``parts`` (a contact.HandParts: the label
    table of parts and self-collision).  The seam and the pair words of self-collision are NOT taken from contact.SelfTable: they come
    from grasp_self_ref.seam_sources / default_pairs."""

    def __init__(self, layer=None, rig=None, parts=None):
        self.layer, self.rig, self.parts = layer, rig, parts


def posed(pose, params):
    """``pose(params)`` in its two forms -- fp32 vertices [B,V,3], or (vertices, joints [B,J,3]) -- as (vertices, joints or None)."""
    out = pose(np.ascontiguousarray(params, F32))
    if isinstance(out, tuple):
        return np.ascontiguousarray(out[0], F32), np.ascontiguousarray(out[1], F32)
    return np.ascontiguousarray(out, F32), None


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def push_out(o, params0, verts0, obj, faces, pose, hand, device, forced=()):
    """Steps 2 and 3 for ALL rows of one object: (the dict below).  ``params0`` / ``verts0``: the hands as generated; ``forced``: rows
    whose re-posed hands the articulated guard must see as worse (tests/test_grasp_refine_fingers.py::_force_worse: no contact and an
    infinite penetration in the scores of the re-posed hands).

    The write-back of a turn into ``params[:, 10:13]`` and of the curls into ``params[:, 13:58]`` is contact.compose_orient /
    compose_finger_pose, and the axis-angles shown are contact.quat_axis_angle, of the REFERENCE's quaternions, on ``device`` -- the
    package's own host formulas, which tests/test_grasp_refine_rigid.py and test_grasp_refine_fingers.py check against float64 twins:
    here they check the plumbing only.  The guard's rule is written out: keys by contact.select_keys("penetration") of
    grasp_score_ref's scores of the re-posed hands against those of the hands as generated (the reference's iterate 0); a row with a
    worse (class, key) takes back its generated parameters and vertices, a zero offset, identity turns and iterate 0; the scores
    reported are the merged ones."""
    steps, push, pull, mc = int(o["refine_steps"]), o["refine_push"], o["refine_pull"], o["min_contact"]
    spin, curl = float(o["refine_spin"]), float(o["refine_curl"])
    out = {"kind": "curl" if curl else "spin" if spin else "translation", "pieces": ["offset", "iter"], "merged": None}
    if not (spin or curl):
        off, it, _, _, _ = rref.grasp_refine(verts0, faces, obj, steps, push, pull, mc)
        params = params0.copy()
        params[:, 58:61] = (params0[:, 58:61] + off).astype(F32)
        out.update(offset=off, iter=it, params=params)
        out["verts"], out["joints"] = posed(pose, params)
        return out
    v_first, joints0 = posed(pose, params0)
    assert joints0 is not None, "refine_spin and refine_curl need a pose that returns (vertices, joints): the pivots are joints"
    assert np.array_equal(bits(v_first), bits(verts0)), "the pose given does not reproduce the plain run's vertices"
    P0 = _dev(params0, device)
    new = P0.clone()
    if not curl:
        off, quat, it, _, _, _ = gref_rigid.grasp_refine_rigid(verts0, faces, obj, joints0[:, 0], steps, push, pull, spin, mc)
        new[:, 10:13] = contact.compose_orient(P0[:, 10:13], _dev(quat, device))
        new[:, 58:61] = P0[:, 58:61] + _dev(off, device)
        params = new.cpu().numpy()
        out.update(offset=off, iter=it, quat=quat, params=params, rotation=contact.quat_axis_angle(_dev(quat, device)).cpu().numpy())
        out["pieces"] = ["offset", "iter", "rotation"]
        out["verts"], out["joints"] = posed(pose, params)
        return out
    rig = hand.rig
    knuckle = joints0[:, rig.joints]
    r = dict(zip(fref.NAMES, fref.grasp_refine_fingers(verts0, faces, obj, joints0[:, 0], rig.vert_part, rig.vert_w, knuckle, steps, push, pull,
                                                       spin, curl, o["refine_max_curl"], mc)))
    new[:, 10:13] = contact.compose_orient(P0[:, 10:13], _dev(r["quat"], device))
    new[:, 13:58] = contact.compose_finger_pose(hand.layer, P0[:, 10:13], P0[:, 13:58], _dev(r["finger_quat"], device), rig)
    new[:, 58:61] = P0[:, 58:61] + _dev(r["offset"], device)
    new = new.cpu().numpy()
    v1, j1 = posed(pose, new)
    s1 = dict(zip(SCORE_NAMES, sref.grasp_scores(v1, faces, obj)))
    s1 = {k: np.array(v) for k, v in s1.items()}
    forced = np.asarray(sorted(forced), np.int64)
    s1["penetration"][forced], s1["n_contact"][forced] = INF, 0
    keys = lambda s: tuple(x.numpy() for x in contact.select_keys({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in s.items()},
                                                                  "penetration", mc))
    cls1, key1 = keys(s1)
    cls0, key0 = keys({"penetration": r["penetration0"], "n_contact": r["n_contact0"]})
    with np.errstate(invalid="ignore"):
        worse = (cls1 > cls0) | ((cls1 == cls0) & (key1 > key0))                    # a NaN key compares false: such a row never moved
    ident = np.zeros(4, F32)
    ident[0] = 1.0
    quat = np.where(worse[:, None], ident, r["quat"]).astype(F32)
    fquat = np.where(worse[:, None, None], ident, r["finger_quat"]).astype(F32)
    B, Pn = fquat.shape[:2]
    out.update(offset=np.where(worse[:, None], F32(0), r["offset"]).astype(F32), iter=np.where(worse, 0, r["iter"]).astype(np.int32),
               quat=quat, finger_quat=fquat, reverted=worse.astype(np.int32), unreverted=dict(r, params=new, verts=v1),
               curl=contact.quat_axis_angle(_dev(fquat, device).reshape(-1, 4)).reshape(B, Pn, 3).cpu().numpy(),
               merged={k: np.where(worse, r[k + "0"], s1[k]).astype(s1[k].dtype) for k in SCORE_NAMES},
               params=np.where(worse[:, None], params0, new).astype(F32), verts=np.where(worse[:, None, None], verts0, v1).astype(F32),
               joints=np.where(worse[:, None, None], joints0, j1).astype(F32))
    if spin:
        out["rotation"] = contact.quat_axis_angle(_dev(quat, device)).cpu().numpy()
    out["pieces"] = [k for k in REFINE_PIECES if k in out]
    return out


def mesh_class(n_inside, depth, max_depth_cm):
    """The rule of the docstring, written out: 2 without a figure (n_inside < 0), else 1 where the fp32 depth exceeds fp32(X / 100)
    metres, else 0."""
    limit = F32(float(max_depth_cm) / 100.0)
    return np.asarray([2 if int(n) < 0 else int(F32(d) > limit) for n, d in zip(n_inside, depth)], np.int32)


def want_figures(o):
    return {"volume": bool(o["volume"]) or float(o["max_volume"]) < INF,
            "parts": bool(o["parts"]) or bool(o["min_fingers"]) or bool(o["need_thumb"]),
            "self": bool(o["self_collision"]) or o["max_self_verts"] is not None,
            "mesh": bool(o["mesh_depth"]) or float(o["max_mesh_depth"]) < INF}


def stages(plain, obj4n, faces, sealed_topology, pose, transform, options, cache=None, cache_key=None, tune=None, hand=None, mesh=None,
           forced=()):
    """Steps 1 - 5 for ALL rows of one object: what they give depends on the refinements' and the kernels' own arguments only, so
    ``cache`` (a dict) with ``cache_key`` (naming the object and its plain run) shares them between the option sets of a test: the
    hands under (rotation, push-out settings and forced rows, ttt settings), every figure under its own settings beside them.
    Returns (base, scores, figures): ``figures`` maps volume / parts / self / mesh to the reference's dict of ALL rows."""
    o = options
    refine_key = ((o["refine_steps"], o["refine_push"], o["refine_pull"], o["min_contact"], float(o["refine_spin"]), float(o["refine_curl"]),
                   o["refine_max_curl"] if o["refine_curl"] else None, tuple(sorted(forced)) if o["refine_curl"] else ())
                  if o["refine_steps"] else None)
    ttt_key = ((o["ttt_steps"], o["ttt_lr"], o["ttt_momentum"], o["ttt_w_pen"], o["ttt_w_con"], bool(o["ttt_keep_best"]), repr(o["ttt_prior"]))
               if o["ttt_steps"] else None)
    caching = cache is not None and cache_key is not None
    pushed = cache.setdefault((cache_key, o["rotate"], refine_key), {}) if caching else {}      # steps 1 - 3, shared by the ttt settings
    store = cache.setdefault((cache_key, o["rotate"], refine_key, ttt_key), {}) if caching else {}
    Rt = np.asarray(plain["json"]["R_list"], np.float64)                               # [M,3,4]: rotation | translation
    R, t = Rt[:, :, :3].astype(F32), Rt[0, :, 3].astype(F32)
    if "base" not in store:
        if "pushed" not in pushed:
            params = plain["params"].detach().cpu().numpy().astype(F32)
            verts = plain["vertices"].detach().cpu().numpy().astype(F32)
            obj = np.ascontiguousarray(transform(obj4n, R, t), F32)                     # [M,N,3]
            base = {"obj": obj, "offset": None, "iter": None, "push": None, "ttt": None, "params0": params, "verts0": verts}
            if o["refine_steps"]:
                push = push_out(o, params, verts, obj, faces, pose, hand, plain["params"].device, forced)
                params, verts = push["params"], push["verts"]
                base.update(offset=push["offset"], iter=push["iter"], push=push)
            base.update(pushed_params=params, pushed_verts=verts)
            pushed["pushed"] = base
        base = dict(pushed["pushed"])
        params, verts, obj = base["pushed_params"], base["pushed_verts"], base["obj"]
        if o["ttt_steps"]:
            assert tune is not None, "ttt_steps needs the ``tune`` callable"
            tuned = {k: np.ascontiguousarray(v) for k, v in tune(params.copy(), obj.copy()).items()}
            params = np.ascontiguousarray(tuned["params"], F32)
            verts, _ = posed(pose, params)
            base["ttt"] = tuned
        base.update(params=params, verts=verts)
        store["base"] = base
    base = store["base"]
    want_stability = bool(o["stability"]) or (bool(o["candidates"]) and o["select_by"] == "stability")
    want_scores = bool(o["candidates"]) or bool(o["refine_steps"]) or want_stability
    scores = None
    if want_stability:
        k = ("wrench", float(o["torque_length"]))
        if k not in store:
            store[k] = wref.grasp_wrench(base["verts"], faces, base["obj"], 1.0 / float(o["torque_length"]))
        scores = dict(store[k])
    elif want_scores and base["push"] is not None and base["push"]["merged"] is not None and base["ttt"] is None:
        scores = dict(base["push"]["merged"])                 # the guard has scored the hands written; a ttt pass voids them
    elif want_scores:
        if "scores" not in store:
            store["scores"] = dict(zip(SCORE_NAMES, sref.grasp_scores(base["verts"], faces, base["obj"])))
        scores = dict(store["scores"])
    want, figs = want_figures(o), {}
    M = base["verts"].shape[0]
    frame = dict(R=R, t=t) if o["rotate"] else dict(R=None, t=None)
    if want["volume"]:
        k = ("volume", float(o["volume_res"]))
        if k not in store:
            sealed, loop_off, loop_vert = sealed_topology
            planes = contact.hull_planes(obj4n[:3].T.cpu().numpy().astype(np.float64))  # of the object's own UNROTATED cloud
            store[k] = vref.grasp_volume(base["verts"], sealed, loop_off, loop_vert, planes, [0, len(planes)], np.zeros(M, np.int64),
                                         h=float(o["volume_res"]), **frame)
        figs["volume"] = store[k]
    if want["parts"]:
        k = ("parts", float(o["part_threshold"]))
        if k not in store:
            thr = float(o["part_threshold"])
            store[k] = pref.grasp_parts(base["verts"], hand.parts.labels, hand.parts.n_parts, base["obj"], thr * thr)
        figs["parts"] = store[k]
    if want["self"]:
        k = ("self", float(o["self_reach"]), float(o["self_margin"]), int(o["self_seam"]), bool(o["self_palm"]))
        if k not in store:
            labels, n_parts = hand.parts.labels, hand.parts.n_parts
            source = cref.seam_sources(labels, faces, int(o["self_seam"]))
            pairs = cref.default_pairs(n_parts, bool(o["self_palm"]), min(5, n_parts))
            store[k] = cref.grasp_self(base["verts"], faces, labels, source, n_parts, pairs, float(o["self_reach"]) ** 2, float(o["self_margin"]))
        figs["self"] = store[k]
    if want["mesh"]:
        mv, mf = np.asarray(mesh[0], F32).reshape(-1, 3), np.asarray(mesh[1], np.int32).reshape(-1, 3)
        k = ("mesh", mv.tobytes(), mf.tobytes())
        if k not in store:
            store[k] = mref.grasp_mesh(base["verts"], mv, [0, len(mv)], mf, [0, len(mf)], np.zeros(M, np.int64), **frame)
            assert store[k]["err"] == 0
        figs["mesh"] = store[k]
    return base, scores, figs


def volume_class(count, max_volume, res):
    """The rule of the docstring, written out: 2 without a figure, else 1 above floor(X / (res^3 * 1e6)) voxels, else 0."""
    limit = contact.volume_limit(max_volume, res)
    return np.asarray([2 if int(c) < 0 else int(int(c) > limit) for c in count], np.int32)


def guard_classes(o, figs):
    """The classes the figures' guards raise, by figure name, in the order of generate.FIGURES: only the guards with a limit set."""
    out = {}
    if "volume" in figs and float(o["max_volume"]) < INF:
        out["volume"] = volume_class(figs["volume"]["count"], o["max_volume"], o["volume_res"])
    if "parts" in figs and (o["min_fingers"] or o["need_thumb"]):
        p = figs["parts"]
        out["parts"] = np.asarray(pref.parts_class(p["part_count"], p["status"], int(o["min_fingers"]), bool(o["need_thumb"]),
                                                   int(o["part_min_verts"])), np.int32)
    if "self" in figs and o["max_self_verts"] is not None:
        s = figs["self"]
        out["self"] = np.asarray(cref.self_class(s["pen_count"], s["status"], int(o["max_self_verts"])), np.int32)
    if "mesh" in figs and float(o["max_mesh_depth"]) < INF:
        out["mesh"] = mesh_class(figs["mesh"]["n_inside"], figs["mesh"]["depth"], o["max_mesh_depth"])
    return out


def diversity_entry(kept_params, clusters):
    """Step 8 for one object's kept parameters [keep,61]."""
    keep = kept_params.shape[0]
    init = diversity.kmeans_init(1, keep, clusters, "spaced").numpy()
    _, counts, _, dist, used = kref.segment_kmeans(kept_params, init, 1, keep, generate.DIVERSITY_ITERS)
    ent, mean = kref.statistics(counts[0], dist)
    return {"clusters": int(clusters), "entropy": ent, "mean_dist": mean, "iters": int(used[0]), "counts": counts[0].tolist()}


def stability_json(sums, n_contact, key):
    """The four stability fields of the rows given.  The three float64 figures are contact.wrench_stats itself -- the host formula the
    package uses, which tests/test_grasp_wrench.py checks against an independent float64 computation -- so for them the combined tests
    check the plumbing only (the right rows' sums and counts reach the formula, in the right order); the key's rule is written out:
    the float32 key as a Python float, null where it is +inf or NaN."""
    out = contact.wrench_stats(sums, n_contact)
    out["stability_key"] = [None if (k != k or k in (INF, -INF)) else k for k in (float(x) for x in np.asarray(key, F32))]
    return out


def volume_json(count, depth, res):
    """The three volume fields of the rows given: contact.volume_stats itself (the package's host formula, pinned by
    tests/test_grasp_volume.py) -- again a check of the plumbing, not of the formula -- and the count, null where it is negative."""
    out = contact.volume_stats(count, depth, res)
    out["volume_voxels"] = [None if int(k) < 0 else int(k) for k in count]
    return out


def parts_json(p, sel, o, n_parts, n_verts):
    """The four parts fields of the kept rows ``sel``: contact.part_stats itself (pinned by tests/test_grasp_parts.py against
    grasp_parts_ref.part_stats: plumbing only) and grasp_parts_ref.contact_map over the KEPT rows of THIS object."""
    out = contact.part_stats(p["part_min"][sel], p["part_count"][sel], p["status"][sel], int(o["part_min_verts"]), min(5, n_parts))
    out["hand_contact_map"] = [int(x) for x in pref.contact_map(p["mask"][sel], n_verts)]
    return out


def self_json(s, sel):
    """The five self-collision fields of the kept rows: contact.self_stats itself (pinned by tests/test_grasp_self.py: plumbing only)."""
    return contact.self_stats({k: s[k][sel] for k in SELF_PIECES})


def mesh_json(m, sel, closed, n_verts):
    """The four mesh fields of the kept rows: contact.mesh_stats itself (plumbing only), ``closed`` as the test decided it from the
    mesh it built, and grasp_parts_ref.contact_map over the kept rows' inside masks."""
    out = contact.mesh_stats({"n_inside": m["n_inside"][sel], "depth": m["depth"][sel]})
    out["mesh_closed"] = bool(closed)
    out["mesh_penetration_map"] = [int(x) for x in pref.contact_map(m["mask"][sel], n_verts)]
    return out


def compose_one(plain, obj4n, faces, sealed_topology, pose, transform, options, cache=None, cache_key=None, tune=None, hand=None, mesh=None,
                closed=None, forced=()):
    o = {**OFF, **options}
    M = plain["params"].shape[0]
    cand_mode = bool(o["candidates"])
    assert (o["candidates"] or o["num_grasp"]) == M, "the plain run must hold the rows of the call: candidates, or num_grasp without"
    beam = bool(o["beam_width"])
    assert not beam or (int(o["beam_width"]) * int(o["beam_poses"]) == M and all(k in plain for k in BEAM_PIECES)), "beam: the plain run is the beam run"
    keep = int(o["num_grasp"])
    base, scores, figs = stages(plain, obj4n, faces, sealed_topology, pose, transform, o, cache, cache_key, tune, hand, mesh, forced)
    vol = figs.get("volume")
    want_stability = bool(o["stability"]) or (cand_mode and o["select_by"] == "stability")
    with_logp = bool(o["log_prob"]) or beam or (cand_mode and o["select_by"] == "log_prob")
    logp = plain["log_prob"].detach().cpu().numpy().astype(F32) if with_logp else None
    pj = plain["json"]
    n_verts = base["verts"].shape[1]
    exp = {}
    if cand_mode:
        scores_all = dict(scores)
        if logp is not None:
            scores_all["log_prob"] = logp
        as_t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in scores_all.items()}
        cls, key = contact.select_keys(as_t, o["select_by"], o["min_contact"], log_prob=as_t.get("log_prob"),
                                       max_penetration=o["max_penetration"])
        cls, key = cls.numpy().astype(np.int32), key.numpy().astype(F32)
        exp["cls_ranking"], exp["guards"] = cls.copy(), guard_classes(o, figs)
        for g in exp["guards"].values():
            cls = np.maximum(cls, g)
        exp["cls"], exp["key"] = cls, key
        rank = gap = None
        if o["diverse_pool"]:
            pool = sref.segment_topk(cls, key, 1, M, int(o["diverse_pool"]))
            feat = base["params"] if o["diverse_space"] == "params" else base["verts"].reshape(M, -1)
            sel, rank, gap = dref.segment_diverse(feat, pool, 1, M, keep)
            sel, rank, gap = sel[0], rank[0], gap[0]
            exp["pool"] = pool[0]
        else:
            sel = sref.segment_topk(cls, key, 1, M, keep)[0]
        exp["best"] = sref.segment_topk(cls, key, 1, M, keep)[0]
    else:
        sel = np.arange(M)
        scores_all = None
    kept_p, kept_v = base["params"][sel], base["verts"][sel]
    j = {"recon_params": [[p] for p in kept_p.tolist()], "R_list": [pj["R_list"][c] for c in sel],
         "trans_list": pj["trans_list"][:keep], "r_list": [pj["r_list"][c] for c in sel]}
    keys = []
    div = diversity_entry(kept_p, o["diversity"]) if o["diversity"] else None
    stab = stability_json(scores["sums"][sel], scores["n_contact"][sel], scores["key"][sel]) if want_stability else {}
    # the figures after the volume, in the order of generate.FIGURES: (dict key, key of ALL candidates, pieces, the JSON fields)
    fig_rows = []
    if vol is not None:
        fig_rows.append(("volume", "volume_scores", vol, VOLUME_PIECES, volume_json(vol["count"][sel], vol["depth"][sel], o["volume_res"])))
    if "parts" in figs:
        fig_rows.append(("parts", "part_scores", figs["parts"], PARTS_PIECES, parts_json(figs["parts"], sel, o, hand.parts.n_parts, n_verts)))
    if "self" in figs:
        fig_rows.append(("self", "self_scores", figs["self"], SELF_PIECES, self_json(figs["self"], sel)))
    if "mesh" in figs:
        assert closed is not None, "mesh depth: the test says whether the mesh it built is closed"
        fig_rows.append(("mesh", "mesh_scores", figs["mesh"], MESH_PIECES, mesh_json(figs["mesh"], sel, closed, n_verts)))
    push = base["push"]
    refine_exp = {"refine_" + k: push[k][sel] for k in push["pieces"]} if push is not None else {}
    refine_json = {k: v.tolist() for k, v in refine_exp.items()}
    if cand_mode:
        j["candidate"] = sel.tolist()
        for k in SCORE_NAMES + (("log_prob",) if with_logp else ()):
            j[k] = scores_all[k][sel].tolist()
        j.update(stab)
        if with_logp:
            exp["log_prob"] = logp[sel]
            keys.append("log_prob")
        if want_stability:
            exp["wrench_sums"], exp["stability_key"] = scores["sums"][sel], scores["key"][sel]
            keys += ["wrench_sums", "stability_key"]
        if o["diverse_pool"]:
            exp["rank"], exp["novelty"] = rank, gap
            j.update(rank=rank.tolist(), novelty=gap.tolist())
            keys += ["rank", "novelty"]
        exp.update(refine_exp)
        j.update(refine_json)
        keys += list(refine_exp)
        if div is not None:
            exp["diversity"] = j["diversity"] = div
            keys.append("diversity")
        for name, all_name, d, pieces, fields in fig_rows:
            exp[name] = {k: d[k][sel] for k in pieces}
            exp[all_name] = {k: d[k] for k in pieces}
            j.update(fields)
            keys += [name, all_name]
        exp["candidate"], exp["scores"] = sel.astype(np.int64), scores_all
        keys += ["params", "vertices", "candidate", "scores", "json"]
    else:
        if with_logp:
            exp["log_prob"] = logp
            j["log_prob"] = logp.tolist()
            keys.append("log_prob")
        exp.update(refine_exp)
        j.update(refine_json)
        keys += list(refine_exp)
        if scores is not None:
            for k in SCORE_NAMES:
                exp[k] = scores[k]
                j[k] = scores[k].tolist()
                keys.append(k)
        if want_stability:
            exp["wrench_sums"], exp["stability_key"] = scores["sums"], scores["key"]
            j.update(stab)
            keys += ["wrench_sums", "stability_key"]
        for name, _, d, pieces, fields in fig_rows:                                # the diversity stands after the volume, before the rest
            if name != "volume" and div is not None and "diversity" not in keys:
                exp["diversity"] = j["diversity"] = div
                keys.append("diversity")
            exp[name] = {k: d[k] for k in pieces}
            j.update(fields)
            keys.append(name)
        if div is not None and "diversity" not in keys:
            exp["diversity"] = j["diversity"] = div
            keys.append("diversity")
        keys += ["params", "vertices", "json"]
    if base["ttt"] is not None:                                                    # attached after the call's dicts are built
        for k in TTT_PIECES:
            x = base["ttt"][k][sel]
            exp["ttt_" + k] = x
            j["ttt_" + k] = x.tolist() if k == "iter" else [float(v) if np.isfinite(v) else None for v in x]
            keys.append("ttt_" + k)
    if beam:                                                                       # the plain run's, carried through the selection
        for k in BEAM_PIECES:
            exp[k] = plain[k].detach().cpu().numpy().astype(np.int64)[sel]
            j[k] = exp[k].tolist()
            keys.append(k)
    exp.update(params=kept_p, vertices=kept_v, json=j, keys=keys, stage=base, stage_scores=scores, stage_volume=vol, stage_figures=figs)
    return exp


def compose(plain, clouds, faces, sealed_topology, pose, options, transform=None, cache=None, cache_keys=None, tune=None, hand=None,
            mesh_closed=None, forced=None):
    """What ``generate_for_objects(net, clouds, options["num_grasp"], options["rotate"], ...)`` must return with ``options`` on (the
    keys of OFF; missing ones are off), one dict per object.

    ``plain``: per object, the dict of a plain run of M rows (M = candidates, or num_grasp without candidates) with the same seed,
    object_indices, rotate, temperature, top_k and log_prob -- and the same ``beam_width`` / ``beam_poses``: nothing is drawn then, so
    the "plain" run of a beam case is the run with only those two on, whose rows compose treats as ordinary rows, carrying their
    ``log_prob`` (always present then), ``beam_pose``, ``beam_rank`` and ``beam_duplicate_of`` through the selection: ``params``
    [M,61], ``vertices`` [M,V,3], ``log_prob`` [M] where the options read it, and ``json`` with its ``R_list`` / ``r_list`` /
    ``trans_list``.  ``clouds``: the [4,N] object tensors.  ``faces`` [F,3]; ``sealed_topology`` = (sealed faces, loop_off, loop_vert)
    of contact.seal_faces, as numpy; ``pose``: fp32 params [B,61] -> fp32 vertices [B,V,3], or -> (vertices, joints [B,J,3]), which the
    rigid and the articulated push-out need for their pivots (the net's MANO layer, which has its own float64 tests).  ``transform``:
    step 1 (default: ops.transform_cloud on the device of the plain tensors).  ``tune``: ``(params [M,61], cloud_xyz [M,N,3]) -> dict``
    of ``params`` / ``loss0`` / ``loss`` / ``iter`` as numpy, backed by contact.refine_ttt with the options' ttt settings (a plumbing
    check: the arithmetic is tests/test_grasp_ttt.py's).  ``hand``: a ``Hand``.  ``options["object_meshes"]``: one (verts, faces) per
    object; ``mesh_closed``: per object, whether that mesh is closed, as the test knows it from building it.  ``forced``: per object,
    the rows the articulated guard must see as worse (``push_out``).  ``cache`` / ``cache_keys`` (one hashable per object, naming the
    object and its plain run): share steps 1 - 5 between calls.

    Each dict holds, as numpy arrays: ``params``, ``vertices``, ``candidate``, ``rank`` / ``novelty``, ``refine_offset`` / ``refine_iter``
    / ``refine_rotation`` / ``refine_curl`` (float64) / ``refine_reverted``, ``scores`` (all candidates), ``wrench_sums`` /
    ``stability_key``, ``volume`` / ``volume_scores``, ``parts`` / ``part_scores``, ``self`` / ``self_scores``, ``mesh`` /
    ``mesh_scores``, ``log_prob``, ``ttt_loss0`` / ``ttt_loss`` / ``ttt_iter``, the three beam entries, (without candidates)
    ``penetration`` / ``n_interior`` / ``n_contact``; the ``diversity`` dict; ``json`` with its keys in order; ``keys``: the returned
    dict's own keys in order; and for the tests' direct assertions ``cls`` / ``key`` / ``pool`` / ``best`` (the ``num_grasp``
    best-ranked), ``cls_ranking`` (the class before the figures' guards) and ``guards`` (each guard's class by figure), and ``stage`` /
    ``stage_scores`` / ``stage_volume`` / ``stage_figures`` (steps 1 - 5 of ALL rows; ``stage`` holds ``params0`` / ``verts0`` as
    generated, ``pushed_params`` / ``pushed_verts`` before the gradient refinement, ``push`` and ``ttt``)."""
    if transform is None:
        transform = device_transform(plain[0]["params"].device)
    o = {**OFF, **options}
    meshes = o["object_meshes"]
    return [compose_one(p, c, faces, sealed_topology, pose, transform, options, cache, None if cache_keys is None else cache_keys[i], tune, hand,
                        None if meshes is None else meshes[i], None if mesh_closed is None else mesh_closed[i],
                        () if forced is None else forced[i])
            for i, (p, c) in enumerate(zip(plain, clouds))]


# ------------------------------------------------------------------------------------------------------ comparisons
FLOAT64_KEYS = ("refine_rotation", "refine_curl")
"""The entries generate_for_objects documents as float64 (axis-angles computed in float64); every other float entry is float32."""


def same_bits(got, want, what, floats=np.float32):
    """``floats`` (fp32 unless the entry is one of FLOAT64_KEYS): bit for bit, a NaN is a NaN (the rule of every stage test);
    integers: equal.  A float entry of another width than ``floats``, on either side, fails."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.dtype.kind == "f":
        assert got.dtype == floats and want.dtype == floats, (what, got.dtype, want.dtype, floats)
        word = np.uint32 if floats == np.float32 else np.uint64
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, got, want)
        assert np.array_equal(np.ascontiguousarray(got).view(word)[~nan], np.ascontiguousarray(want).view(word)[~nan]), (what, got, want)
    else:
        assert got.dtype.kind in "iu" and np.array_equal(got, want), (what, got, want)


def assert_result(got, want, what=""):
    """One object's dict of generate_for_objects against compose's: the dict's keys in order, tensors bit for bit, the diversity dict
    and the JSON by ``==`` with its keys in order, the nested dicts of scores and figures name by name.  ``json.dumps`` of both must
    agree as well: a float32 value and its Python float have the same repr exactly when their bits agree, so this is the bit
    comparison of the float32 fields (and tells -0.0 from +0.0)."""
    assert list(got) == want["keys"], (what, list(got), want["keys"])
    for k in want["keys"]:
        if k == "json":
            assert list(got["json"]) == list(want["json"]), (what, list(got["json"]), list(want["json"]))
            for f in want["json"]:
                assert got["json"][f] == want["json"][f], (what, f, got["json"][f], want["json"][f])
            assert json.dumps(got["json"]) == json.dumps(want["json"]), what
        elif k == "diversity":
            assert got[k] == want[k] and list(got[k]) == list(want[k]), (what, got[k], want[k])
        elif k in NESTED:
            assert set(got[k]) == set(want[k]), (what, k, set(got[k]), set(want[k]))
            for name in want[k]:
                same_bits(got[k][name], want[k][name], f"{what} {k}[{name}]")
        else:
            same_bits(got[k], want[k], f"{what} {k}", np.float64 if k in FLOAT64_KEYS else np.float32)


# ------------------------------------------------------------------------------------------------------ inputs
CENTRE = (-0.6006, -0.1580, -0.1531)
"""Where the synthetic weights put the hands of a ROTATED run against the objects of rotated_contact_objects -- measured, see there."""
STILL_CENTRE = (-0.10, -0.085, 0.125)
POINTS, HALF, SIGMA = (64, 48, 64), 0.10, 0.05


SEED = 104
"""The run seed of the rotated tests: the first seed >= 0 at which, for the objects 0, 1, 2 and eight rows, no block of
rotated_contact_objects other than a row's own lands within 0.2 m of CENTRE (most seeds bring one of the 168 pairs that close)."""
STILL_SEED = 12
"""The run seed of the tests without rotation.  Changed from SEED: at seed 104 the four candidates of object 0 that ``max_volume``
demotes are exactly the four that ``max_penetration`` demotes, so neither guard acts alone; at seed 12 each demotes one the other
leaves."""


def block(seed, tag, n, centre, half, sigma=None):
    """n points in the cube of half-width ``half`` about ``centre``, float64 [n,3]: uniform, or with ``sigma`` normal draws of that
    deviation clipped to the cube (denser where the hand is)."""
    if sigma is None:
        d = synth.synthetic_uniform((n, 3), seed, tag, -half, half).numpy().astype(np.float64)
    else:
        d = np.clip(synth.synthetic_normal((n, 3), seed, tag, sigma).numpy().astype(np.float64), -half, half)
    return d + np.asarray(centre, np.float64)


def hand_clouds(centre=STILL_CENTRE, counts=(384, 256, 384), half=0.07, sigma=None, seed=170):
    """Unrotated [N,3] clouds at the hand, of two point counts, for calls with ``rotate=False``."""
    return [block(seed + i, "combined/still", n, centre, half, sigma) for i, n in enumerate(counts)]


def rotation_of(seed, index, M):
    """[M,3,3]: exactly what generate._generate_call draws for object ``index`` of a run with ``seed``."""
    return generate.rotation_xyz(np.random.default_rng([seed, int(index)]).random((M, 3)) * np.pi * 2)


def rotated_contact_objects(seed, object_indices, M, centre=CENTRE, points=POINTS, half=HALF, sigma=SIGMA):
    """Objects that meet the hand under the datasets' random rotations.  Row g of object i is generated against R_g x + t with
    R = rotation_of(seed, i, M) and t = CANONICAL_OFFSET, about 0.8 m from where the synthetic weights put every hand; so object i's
    cloud is the union over g < M of R_g^T (cube_g - t), cube_g = ``points[i]`` points in the cube of half-width ``half`` about
    ``centre`` (a draw of its own per (i, g)): under row g's transform block g lands on the hand and the other blocks elsewhere on the
    0.8 m sphere about t.  Returns (clouds: float64 [M * points[i], 3] per object, cubes: [M, points[i], 3] per object).

    ``centre``: the net has no CPU path, so the hand's place is measured on the MI355X, and it depends on the cloud the net sees (about
    (-0.14, -0.12, 0.09) against tests/test_grasp_select.py's synthetic clouds, elsewhere against these).  CENTRE is the fixed point:
    plain rotated runs (tests/test_grasp_select.py::_gennet, 8 rows, objects 0, 1, 2) against these objects built about (-0.14, -0.12,
    0.09), then about the mean vertex each run gave, gave mean vertices (-0.6196, -0.1574, -0.1706), (-0.6006, -0.1580, -0.1531) and
    (-0.5993, -0.1581, -0.1530) at seed 12; at SEED, built about CENTRE, (-0.6080, -0.1553, -0.1582) with the rows' own means within
    (-0.674 .. -0.541, -0.185 .. -0.111, -0.189 .. -0.093) -- inside the cube.  The entry points' own synthetic weights
    (generate.load_model) give the same place to 1 mm.  The tests that use it assert contact and penetration per object rather than
    trust the constant."""
    t = np.asarray(generate.CANONICAL_OFFSET, np.float64)
    clouds, cubes = [], []
    for i, index in enumerate(object_indices):
        R = rotation_of(seed, index, M)
        cube = np.stack([block(200 + int(index), f"combined/rotated/{g}", points[i], centre, half, sigma) for g in range(M)])
        clouds.append(np.concatenate([(cube[g] - t) @ R[g] for g in range(M)]))          # row vectors: (R^T v)^T = v^T R
        cubes.append(cube)
    return clouds, cubes


BOX_FACES = ((0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5))
"""The 12 outward triangles of ``box``.  The boxes' place and sizes were measured on the MI355X at SEED / STILL_SEED with the clouds
above (24 candidates per rotation and push-out kind, every option on, no guard): boxes of half-widths 0.04 .. 0.06 m about STILL_CENTRE
/ CENTRE hold vertices of every unrotated hand (up to 305) and of all but a few rotated ones (up to 432), at depths that differ per
candidate.  No row reverts in the articulated push-out unforced, so the tests force rows as tests/test_grasp_refine_fingers.py does.
tests/test_generate_combined.py::GUARD_RANKS records the sizes, settings and ranks the tests use and how they were found."""


def box(half, centre=STILL_CENTRE):
    """A closed box about ``centre``, 12 outward triangles (tests/test_grasp_mesh.py::cube, moved to the hand): (verts float64 [8,3],
    faces int64 [12,3]).  ``half``: one half-width, or one per axis."""
    v = np.asarray([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64) * np.asarray(half, np.float64) + np.asarray(centre)
    return v, np.asarray(BOX_FACES, np.int64)


def rotated_boxes(seed, index, M, half, centre=CENTRE):
    """The mesh of one object of rotated_contact_objects: the union over g < M of R_g^T (box about ``centre`` - t), a closed mesh of M
    components in the cloud's own frame -- under row g's transform component g lands on the hand.  A wrong frame leaves every hand
    outside every box."""
    t = np.asarray(generate.CANONICAL_OFFSET, np.float64)
    R = rotation_of(seed, index, M)
    v, f = box(half, centre)
    return np.concatenate([(v - t) @ R[g] for g in range(M)]), np.concatenate([f + 8 * g for g in range(M)])
