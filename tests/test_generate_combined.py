"""generate.generate_for_objects with its options TOGETHER, rotated too, on both paths (_select_call, and _generate_call without
candidates), and the entry points with every flag.  The thirteen options: best-of-M, the diverse pool, the translation push-out, the
k-means statistic, the wrench proxy, the voxel volume -- and the rigid push-out (refine_spin), the articulated push-out with its
revert guard (refine_curl), gradient refinement (ttt_*), beam search (beam_width x beam_poses), hand-side contact (parts, min_fingers,
need_thumb), self-collision (self_collision, max_self_verts) and mesh depth (mesh_depth, max_mesh_depth, object_meshes).  The order
of the stages: clouds posed, push-out of all rows, MANO again, gradient refinement, MANO again, scores and figures of the final hands,
classes (the five guards joined by maximum) and keys, top-k or pool and picks, k-means of the kept rows, the JSON.

The reference is tests/generate_ref.py::compose -- the pipeline restated from the stage references -- fed the tensors of a plain run
(for beam search: of the run with only the two beam keywords on); every comparison is the one the stage's own test uses (tensors bit
for bit, JSON by ``==``).  Checked against INDEPENDENT bit-exact CPU references: the three push-outs, the scores, the wrench sums,
volume, parts, self-collision, mesh depth, the selection, the k-means; the revert guard, the class rules, rows, frames and orders are
written out in generate_ref.py.  PLUMBING checks only: the package's own host formulas (select_keys, the *_stats, compose_orient,
compose_finger_pose, quat_axis_angle -- each pinned by its stage's tests) and the device-backed callables this file supplies (the
clouds' transform, MANO, and contact.refine_ttt, whose arithmetic is tests/test_grasp_ttt.py's)."""
import inspect
import itertools
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import contact, generate

import generate_ref as gref
import grasp_mesh_ref as mref
import grasp_parts_ref as pref
import grasp_refine_fingers_ref as fref
import grasp_score_ref as sref
import grasp_self_ref as cref
import grasp_volume_ref as vref
import grasp_wrench_ref as wref

DEV = "cuda:0"
F32 = np.float32
INF = float("inf")
SEED = gref.SEED                                        # rotated runs; gref.STILL_SEED for the runs without rotation
INDICES = [0, 1, 2]                                     # the entry points number their objects from 0: the same rotations there
M, KEEP, POOL, STEPS, CLUSTERS, RES = 8, 4, 6, 3, 2, 0.004
G = 4                                                   # rows per object without candidates
GROUPINGS = (16384, M, 1)                               # rows_per_call: the objects of a point count together; one object per call, twice
KINDS = {"translation": {}, "spin": dict(refine_spin=1.0), "curl": dict(refine_spin=1.0, refine_curl=1.0)}   # the three push-outs
TTT = 3                                                 # gradient steps
BOX_HALVES = {False: (0.045, 0.04, 0.04), True: (0.04, 0.04, 0.06)}     # the half-widths of the objects' boxes, metres
FIGURE_SETTINGS = {False: dict(part_threshold=0.01, self_reach=0.01, self_margin=0.0, self_seam=0),
                   True: dict(part_threshold=0.015, self_reach=0.02, self_margin=0.0, self_seam=0)}
PART_THRESHOLD = {(False, "translation"): 0.015, (False, "spin"): 0.015}   # the new full stack's, where it is not FIGURE_SETTINGS'
_ranks = lambda *r: dict(zip(("penetration", "volume", "fingers", "self", "mesh"), r))
GUARD_RANKS = {(False, "translation"): _ranks(4, 4, 0, 5, 4), (False, "spin"): _ranks(2, 1, 0, 5, 5), (False, "curl"): _ranks(5, 4, 0, 2, 2),
               (True, "translation"): _ranks(4, 4, 1, 2, 5), (True, "spin"): _ranks(5, 4, 1, 2, 7), (True, "curl"): _ranks(4, 4, 1, 4, 6)}
"""The inputs of the seven newer options: the boxes, the settings of parts and self-collision, and per rotation and push-out kind the
rank of object 0's sorted candidates at which each guard's limit is taken (Ctx.guard_limits).  How they were found: the final hands
of the new full stack with no guard (3 objects x 8 candidates, both rotations, the three push-outs) were measured on the MI355X at
SEED / STILL_SEED, and the figures of those hands were evaluated with the CPU references over box half-widths 0.04 .. 0.06 m per
object, part thresholds 7.5 .. 20 mm, (reach, margin, seam) = (1 cm, 0, 0), (2 cm, 0, 0), (1.5 cm, 0.5 mm, 1) and every rank, in that
order; these are the first that meet ALL the conditions of assert_stack_not_vacuous in all three push-out kinds of a rotation.  What
the search showed: at the call's defaults (5 mm, reach 1 cm, margin 1 mm, seam 2) no hand has a self-penetrating vertex and no thumb
of an unrotated hand touches; with seam 0 the vertices at the joins count -- their sign is noise, which serves a test of plumbing --
and every hand has 17 .. 47 of them.  The limits come from object 0 and hold for all objects, so boxes of one size are needed for a
mesh guard that does not demote another object wholesale.  Rotated, one threshold serves the three push-outs; unrotated the
articulated push-out needs 10 mm and the other two 15 mm (PART_THRESHOLD).  Every unrotated hand has its four fingers other than the
thumb on the object at every threshold searched, so there the two parts guards follow the thumb alone and neither demotes a row by
itself; that need_thumb and min_fingers each demote a row the other leaves is asserted for the rotated stacks, where fingers miss."""
ENTRY_RANKS = {False: dict(fingers=1, self=6, mesh=6, need_thumb=True), True: dict(fingers=1, self=6, mesh=7, need_thumb=False)}
"""The same for the three newer guards of test_entry_point_with_every_flag, whose net has synthetic weights of its own: the first ranks,
tried on the MI355X from those that demote fewest, at which that test's own conditions hold.  Its max_penetration and max_volume sit at
the medians of object 0, and a guard that leaves no candidate of any object in class 0 ranks them as no guard does.  For ho3d the two
medians leave only candidates 1, 4 and 7 of object 1, and their thumbs touch at no threshold from 10 to 30 mm: with need_thumb on no
rank changes a file, so ho3d passes --need_thumb 0 and obman --need_thumb 1."""


def seed_of(rotate):
    return gref.SEED if rotate else gref.STILL_SEED


# ------------------------------------------------------------------------------------------------------ CPU: _host_copy
def host_copy_pieces():
    return [torch.zeros(0, dtype=torch.int64), torch.tensor([1.5], dtype=torch.float32), torch.tensor([2 ** 40 + 3], dtype=torch.int64),
            torch.zeros((0, 3), dtype=torch.float32), torch.tensor([[-2 ** 62, 7], [5, -1]], dtype=torch.int64)[:, :1],
            torch.tensor([[1, -2, 3]], dtype=torch.int32), torch.tensor([float("nan"), -0.0, 3e38], dtype=torch.float32),
            torch.tensor([-9, 2 ** 63 - 1], dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
            torch.arange(12, dtype=torch.float32).reshape(3, 4).t(), torch.zeros((2, 0), dtype=torch.int64)]


def test_host_copy_returns_every_piece_in_any_order():
    """int64 pieces at byte offsets 4, 12 and 36 (not multiples of 8), zero-length pieces of every type and at both ends: every piece
    comes back equal to its own .cpu().numpy(), so the function needs no rule about the order of its pieces."""
    pieces = host_copy_pieces()
    offsets =np.cumsum([0] + [p.numel() * p.element_size() for p in pieces])
    assert [int(o) % 8 for o, p in zip(offsets, pieces) if p.dtype == torch.int64 and p.numel()] == [4, 4, 4]
    host = generate._host_copy(pieces)
    assert len(host) == len(pieces)
    for h, p in zip(host, pieces):
        want = p.cpu().numpy()
        assert h.dtype == want.dtype and h.shape == want.shape
        assert h.tobytes() == want.tobytes()                                             # bytes: a NaN and -0.0 compare too
    assert host[2].tolist() == [2 ** 40 + 3] and host[4].tolist() == [[-2 ** 62], [5]] and host[7].tolist() == [-9, 2 ** 63 - 1]
    assert [int(x) for x in host[4].reshape(-1)] == [-2 ** 62, 5] and int(host[7].sum()) == 2 ** 63 - 10
    assert generate._host_copy([torch.zeros(0)])[0].shape == (0,)


def test_host_groups_returns_every_group_under_its_own_name(monkeypatch):
    """The pieces above as named groups -- an empty group at the front, in the middle and at the end, and one of zero-length tensors
    only: every group comes back under its name, its arrays byte-equal to .cpu().numpy() of its pieces, whatever the order of the
    groups, through one ``.cpu()`` per call."""
    p = host_copy_pieces()
    wants = [x.cpu().numpy() for x in p]
    copies, cpu = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(1), cpu(self, *a, **k))[1])
    groups = {"front": [], "hollow": [p[0], p[3]], "params": [p[1], p[2], p[4]], "middle": [], "scores": p[5:8], "mesh": p[8:], "end": []}
    assert all(x.numel() == 0 for x in groups["hollow"]) and sum(len(g) for g in groups.values()) == len(p)
    orders = [list(groups), list(groups)[::-1], ["scores", "end", "hollow", "front", "mesh", "middle", "params"]]
    want_of = {id(x): w for x, w in zip(p, wants)}
    for n, order in enumerate(orders):
        host = generate._host_groups({name: groups[name] for name in order})
        assert list(host) == order and len(copies) == n + 1
        for name, pieces in groups.items():
            assert isinstance(host[name], list) and len(host[name]) == len(pieces), name
            for h, x in zip(host[name], pieces):
                want = want_of[id(x)]
                assert h.dtype == want.dtype and h.shape == want.shape and h.tobytes() == want.tobytes(), name
    assert host["params"][1].tolist() == [2 ** 40 + 3] and host["front"] == host["middle"] == host["end"] == []


# ------------------------------------------------------------------------------------------------------ CPU: the rotated objects
def test_rotated_objects_put_one_block_at_the_hand_per_row():
    t = np.asarray(generate.CANONICAL_OFFSET)
    centre = np.asarray(gref.CENTRE)
    clouds, cubes = gref.rotated_contact_objects(SEED, INDICES, M)
    assert [c.shape[0] for c in clouds] == [M * n for n in gref.POINTS] and len({c.shape[0] for c in clouds}) == 2
    assert len(generate.plan_calls([c.shape[0] for c in clouds], M, 16384)) == 2, "two point counts: the calls must split"
    nearest = []
    for i, index in enumerate(INDICES):
        R = gref.rotation_of(SEED, index, M)
        assert np.array_equal(R, generate.rotation_xyz(np.random.default_rng([SEED, index]).random((M, 3)) * np.pi * 2))
        xyz = generate.object_tensor(clouds[i])[:3].T.numpy().astype(np.float64)     # the cloud as the run holds it: fp32
        n = cubes[i].shape[1]
        for g in range(M):
            moved = xyz @ R[g].T + t                                                 # row g's transform of the whole object
            assert np.abs(moved[g * n:(g + 1) * n] - cubes[i][g]).max() <= 1e-6, (i, g)
            assert cubes[i][g].shape == (gref.POINTS[i], 3) and np.abs(cubes[i][g] - centre).max() <= gref.HALF + 1e-12
            others = np.delete(moved, np.s_[g * n:(g + 1) * n], axis=0)
            nearest.append(float(np.linalg.norm(others - centre, axis=1).min()))
    print(f"{M} rows: the nearest point of another block to the centre: {min(nearest):.3f} m")
    assert min(nearest) >= 0.2
    # the draws differ per object and per row
    assert not np.array_equal(cubes[0][0], cubes[0][1]) and not np.array_equal(cubes[0][0], cubes[2][0])


# ------------------------------------------------------------------------------------------------------ CPU: compose on a toy problem
TOY_M, TOY_KEEP = 6, 3


def toy_problem():
    """No net: a coarse sphere mesh of grasp_score_ref as the hand (closed: nothing to seal), pose = translate by params[:, 58:61], three
    clouds of two point counts in a shell about the sphere, hand-made parameters."""
    v, f = sref.sphere_mesh(9, 20)                                                     # 182 vertices, 360 faces: quick
    pose = lambda p: (v[None] + np.asarray(p, F32)[:, None, 58:61]).astype(F32)
    sealed = (f.astype(np.int32), np.zeros(1, np.int32), np.zeros(0, np.int32))
    transform = lambda obj4n, R, t: (np.einsum("mij,nj->mni", R.astype(np.float64), obj4n[:3].T.numpy().astype(np.float64)) + t).astype(F32)
    plain, clouds = [], []
    for i, n in enumerate((160, 120, 160)):
        rng = np.random.default_rng(40 + i)
        params = rng.normal(size=(TOY_M, 61)).astype(F32)
        params[:, 58:61] = rng.normal(scale=0.012, size=(TOY_M, 3)).astype(F32)
        d = rng.normal(size=(n, 3))
        pts = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.03, 0.065, size=(n, 1))
        clouds.append(generate.object_tensor(pts))
        eye = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
        plain.append({"params": torch.from_numpy(params), "vertices": torch.from_numpy(pose(params)),
                      "log_prob": torch.from_numpy(rng.normal(size=TOY_M).astype(F32)),
                      "json": {"recon_params": [[p] for p in params.tolist()], "R_list": [eye.tolist()] * TOY_M,
                               "trans_list": [np.zeros((3, 1)).tolist()] * TOY_M, "r_list": np.zeros((TOY_M, 3)).tolist()}})
    return plain, clouds, f, sealed, pose, transform


TOY_FULL = dict(num_grasp=TOY_KEEP, candidates=TOY_M, select_by="stability", diverse_pool=5, refine_steps=2, diversity=2, stability=True,
                log_prob=True, volume=True, volume_res=0.004)


def test_compose_with_every_option_off_is_the_input():
    plain, clouds, f, sealed, pose, transform = toy_problem()
    for options in (dict(num_grasp=TOY_M), dict(gref.OFF, num_grasp=TOY_M)):
        for p, e in zip(plain, gref.compose(plain, clouds, f, sealed, pose, options, transform=transform)):
            assert e["keys"] == ["params", "vertices", "json"]
            assert np.array_equal(gref.bits(e["params"]), gref.bits(p["params"].numpy()))
            assert np.array_equal(gref.bits(e["vertices"]), gref.bits(p["vertices"].numpy()))
            assert e["json"] == p["json"] and list(e["json"]) == ["recon_params", "R_list", "trans_list", "r_list"]
    # OFF names every keyword of generate_for_objects at the value the call has without it: api_keywords(OFF) is the plain call
    sig = inspect.signature(generate.generate_for_objects).parameters
    positional = ["net", "objs", "num_grasp", "rotate", "seed", "object_indices"]
    assert list(sig)[:6] == positional and set(gref.OFF) == set(sig) - {"net", "objs", "seed", "object_indices"}
    keywords = gref.api_keywords(gref.OFF)
    assert set(keywords) == set(sig) - set(positional)
    for name, value in keywords.items():
        default = sig[name].default
        assert type(value) is type(default) and value == default, (name, value, default)


def toy_hand_problem():
    """The toy problem for the seven newer options: its pose also returns joints (the centre as the root, five knuckles on the
    equator), a rig of five longitude sectors, a label table of those and a cap as the palm, a stand-in layer whose pose space is the
    identity (contact.compose_finger_pose reads nothing else of it), a closed box as every object's mesh."""
    plain, clouds, f, sealed, pose, transform = toy_problem()
    v, _ = sref.sphere_mesh(9, 20)
    sector = np.clip(((np.arctan2(v[:, 1], v[:, 0]) + np.pi) / (2 * np.pi) * 5).astype(np.int64), 0, 4)
    labels = np.where(v[:, 2] < -0.03, 5, sector)
    knuckles = [1, 4, 7, 10, 13]
    joints = np.zeros((16, 3), F32)
    for k, j in enumerate(knuckles):
        joints[j] = 0.05 * np.asarray([np.cos((k + 0.5) * 2 * np.pi / 5 - np.pi), np.sin((k + 0.5) * 2 * np.pi / 5 - np.pi), 0.0])
    with_joints = lambda p: (pose(p), (joints[None] + np.asarray(p, F32)[:, None, 58:61]).astype(F32))
    layer = types.SimpleNamespace(_packed=types.SimpleNamespace(tensors={"comps": torch.eye(45, dtype=torch.float64),
                                                                         "pose_mean": torch.zeros(48, dtype=torch.float64)}))
    hand = gref.Hand(layer=layer, rig=contact.FingerRig(np.where(labels < 5, labels, -1), np.where(labels < 5, 0.5 + 10.0 * np.clip(v[:, 2], -0.03, 0.05), 0.0),
                                                        knuckles),
                     parts=contact.HandParts(labels, ["thumb", "index", "middle", "ring", "little", "palm"]))
    meshes = [gref.box(h, (0.0, 0.0, 0.0)) for h in (0.04, 0.045, (0.05, 0.03, 0.04))]
    return plain, clouds, f, sealed, with_joints, transform, hand, meshes


TOY_STACK = dict(num_grasp=TOY_KEEP, candidates=TOY_M, refine_steps=2, refine_spin=1.0, refine_curl=1.0, ttt_steps=2, parts=True,
                 part_threshold=0.01, self_collision=True, mesh_depth=True, log_prob=True, diversity=2)
REFINE_FIELDS = ["refine_offset", "refine_iter", "refine_rotation", "refine_curl", "refine_reverted"]
TTT_FIELDS = ["ttt_loss0", "ttt_loss", "ttt_iter"]
BEAM_FIELDS = list(gref.BEAM_PIECES)


def recording_fakes(pose):
    """``pose`` and a ``tune`` that record what they are called with.  The tune moves every even row by 3 mm and reports iterate 1 for
    it; its loss is +inf for row 1 and NaN for row 2."""
    log = {"pose": [], "tune": []}

    def rec_pose(p):
        log["pose"].append(np.array(p, F32))
        return pose(p)

    def tune(params, cloud):
        log["tune"].append((np.array(params, F32), np.array(cloud, F32)))
        B = params.shape[0]
        even = (np.arange(B) % 2 == 0)
        out = np.array(params, F32)
        out[even, 58:61] = (out[even, 58:61] + F32(0.003)).astype(F32)
        loss = (np.arange(B) * 0.25).astype(F32)
        loss[1], loss[2] = np.inf, np.nan
        return {"params": out, "loss0": (loss + F32(1)).astype(F32), "loss": loss, "iter": even.astype(np.int32)}
    return rec_pose, tune, log


def test_compose_runs_push_out_tune_and_figures_in_the_stage_order():
    """The stage-order test for the newer steps, with recording fakes: the articulated push-out sees the hands as generated and the
    pivots of the first posed pass; ``tune`` gets the pushed-out parameters and each row's own cloud; the figures, the scores and the
    selection see its output; the three ttt figures reach the dict and the JSON (null for a loss that is not finite); the scores
    after push-out and tune are those of the tuned hands, without tune the guard's merged ones."""
    plain, clouds, f, sealed, pose, transform, hand, meshes = toy_hand_problem()
    rec_pose, tune, log = recording_fakes(pose)
    options = dict(TOY_STACK, object_meshes=meshes)
    exp = gref.compose(plain, clouds, f, sealed, rec_pose, options, transform=transform, tune=tune, hand=hand, mesh_closed=[True] * 3)
    assert len(log["tune"]) == 3 and len(log["pose"]) == 9, "per object: the first pass, the re-posed hands, the tuned hands"
    moved = curled = changed = 0
    for i, (e, p) in enumerate(zip(exp, plain)):
        st, push = e["stage"], e["stage"]["push"]
        raw = p["params"].numpy()
        obj = transform(clouds[i], np.tile(np.eye(3, dtype=F32), (TOY_M, 1, 1)), np.zeros(3, F32))
        # the push-out: the generated hands in, its pieces out, the write-back in the right columns
        assert np.array_equal(log["pose"][3 * i], raw) and np.array_equal(st["params0"], raw)
        _, joints0 = pose(raw)
        want = dict(zip(fref.NAMES, fref.grasp_refine_fingers(p["vertices"].numpy(), f, obj, joints0[:, 0], hand.rig.vert_part, hand.rig.vert_w,
                                                              joints0[:, hand.rig.joints], 2, 1.0, 0.25, 1.0, 1.0, 0.35, 1)))
        un = push["unreverted"]
        assert all(np.array_equal(un[k], want[k]) for k in fref.NAMES) and np.array_equal(log["pose"][3 * i + 1], un["params"])
        assert np.array_equal(un["params"][:, :10], raw[:, :10])
        assert np.array_equal(gref.bits(un["params"][:, 58:61]), gref.bits((raw[:, 58:61] + want["offset"]).astype(F32)))
        P0 = torch.from_numpy(raw)
        assert torch.equal(torch.from_numpy(un["params"][:, 10:13]), contact.compose_orient(P0[:, 10:13], torch.from_numpy(want["quat"])))
        assert torch.equal(torch.from_numpy(un["params"][:, 13:58]),
                           contact.compose_finger_pose(hand.layer, P0[:, 10:13], P0[:, 13:58], torch.from_numpy(want["finger_quat"]), hand.rig))
        rev = push["reverted"].astype(bool)
        assert np.array_equal(push["params"][rev], raw[rev]) and np.array_equal(push["params"][~rev], un["params"][~rev])
        moved += int((push["iter"] > 0).sum())
        curled += int((push["finger_quat"][..., 0] != 1).any(axis=1).sum())
        # tune: the pushed-out parameters and the row's own cloud in, everything after it on its output
        t_params, t_cloud = log["tune"][i]
        assert np.array_equal(gref.bits(t_params), gref.bits(push["params"])) and np.array_equal(gref.bits(t_cloud), gref.bits(obj))
        assert np.array_equal(gref.bits(st["pushed_params"]), gref.bits(push["params"]))
        tuned = tune(push["params"], obj)
        log["tune"].pop()
        assert np.array_equal(gref.bits(st["params"]), gref.bits(tuned["params"])) and np.array_equal(log["pose"][3 * i + 2], tuned["params"])
        assert np.array_equal(gref.bits(st["verts"]), gref.bits(pose(tuned["params"])[0]))
        changed += int((st["params"] != st["pushed_params"]).any(axis=1).sum())
        # the scores and the figures: the references on the FINAL hands, not on the pushed-out ones
        pen, n_in, n_ct = sref.grasp_scores(st["verts"], f, obj)
        assert np.array_equal(gref.bits(e["scores"]["penetration"]), gref.bits(pen)) and np.array_equal(e["scores"]["n_contact"], n_ct)
        parts = pref.grasp_parts(st["verts"], hand.parts.labels, 6, obj, 0.01 ** 2)
        before = pref.grasp_parts(st["pushed_verts"], hand.parts.labels, 6, obj, 0.01 ** 2)
        assert np.array_equal(gref.bits(e["part_scores"]["part_min"]), gref.bits(parts["part_min"]))
        assert not np.array_equal(gref.bits(parts["part_min"][0]), gref.bits(before["part_min"][0])), "row 0 was tuned: its distances move"
        mesh = mref.grasp_mesh(st["verts"], np.asarray(meshes[i][0], F32), [0, 8], meshes[i][1], [0, 12], np.zeros(TOY_M, np.int64))
        assert np.array_equal(e["mesh_scores"]["n_inside"], mesh["n_inside"]) and (mesh["n_inside"] > 0).any()
        source, pairs = cref.seam_sources(hand.parts.labels, f, 2), cref.default_pairs(6, True)
        own = cref.grasp_self(st["verts"], f, hand.parts.labels, source, 6, pairs, 0.01 ** 2, 0.001)
        assert np.array_equal(gref.bits(e["self_scores"]["gap_min"]), gref.bits(own["gap_min"]))
        # the selection and what it carries
        c, j = e["candidate"], e["json"]
        assert c.tolist() == sref.segment_topk(e["cls"], e["key"], 1, TOY_M, TOY_KEEP)[0].tolist() and np.array_equal(e["key"], pen)
        assert np.array_equal(e["params"], st["params"][c]) and np.array_equal(e["parts"]["mask"], parts["mask"][c])
        assert j["hand_contact_map"] == pref.contact_map(parts["mask"][c], 182) and j["mesh_closed"] is True
        assert j["mesh_penetration_map"] == pref.contact_map(mesh["mask"][c], 182)
        assert j["ttt_iter"] == [int(x % 2 == 0) for x in c] and np.array_equal(e["ttt_iter"], tuned["iter"][c])
        assert j["ttt_loss"] == [None if x in (1, 2) else x * 0.25 for x in c] and j["ttt_loss0"] == [None if x in (1, 2) else x * 0.25 + 1 for x in c]
        assert j["refine_reverted"] == push["reverted"][c].tolist() and j["refine_curl"] == push["curl"][c].tolist()
        assert e["refine_curl"].dtype == np.float64 and e["refine_curl"].shape == (TOY_KEEP, 5, 3) and e["refine_rotation"].shape == (TOY_KEEP, 3)
        assert list(j) == ["recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact", "log_prob",
                           *REFINE_FIELDS, "diversity", *gref.PARTS_FIELDS, *gref.SELF_FIELDS, *gref.MESH_FIELDS, *TTT_FIELDS]
        assert e["keys"] == ["log_prob", *REFINE_FIELDS, "diversity", "parts", "part_scores", "self", "self_scores", "mesh", "mesh_scores",
                             "params", "vertices", "candidate", "scores", "json", *TTT_FIELDS]
        assert "NaN" not in json.dumps(j) and "Infinity" not in json.dumps(j)
    print(f"toy: rows pushed {moved}, with a curled finger {curled}, changed by the tune {changed}")
    assert moved and changed == 9, "the toy push-out moves no row, or the tune's even rows are not all seen as changed"
    # without the tune the scores are the guard's merged ones: those of the hands written
    no_ttt = gref.compose(plain, clouds, f, sealed, pose, dict(options, ttt_steps=0), transform=transform, hand=hand, mesh_closed=[True] * 3)
    for i, e in enumerate(no_ttt):
        push, obj = e["stage"]["push"], e["stage"]["obj"]
        assert all(np.array_equal(e["scores"][k], push["merged"][k]) for k in gref.SCORE_NAMES)
        assert np.array_equal(gref.bits(e["scores"]["penetration"]), gref.bits(sref.grasp_scores(e["stage"]["verts"], f, obj)[0]))
        assert not any(k.startswith("ttt") for k in e["keys"]) and e["stage"]["ttt"] is None
    # without candidates: the documented order, the diversity between the volume and the rest
    flat = gref.compose(plain, clouds, f, sealed, pose, dict(options, num_grasp=TOY_M, candidates=0, volume=True, volume_res=0.004, stability=True),
                        transform=transform, tune=tune, hand=hand, mesh_closed=[True] * 3)
    for e in flat:
        assert list(e["json"]) == ["recon_params", "R_list", "trans_list", "r_list", "log_prob", *REFINE_FIELDS, "penetration", "n_interior",
                                   "n_contact", *gref.STABILITY_FIELDS, *gref.VOLUME_FIELDS, "diversity", *gref.PARTS_FIELDS, *gref.SELF_FIELDS,
                                   *gref.MESH_FIELDS, *TTT_FIELDS]
        assert e["keys"] == ["log_prob", *REFINE_FIELDS, "penetration", "n_interior", "n_contact", "wrench_sums", "stability_key", "volume",
                             "diversity", "parts", "self", "mesh", "params", "vertices", "json", *TTT_FIELDS]


def test_compose_reverts_the_rows_that_come_out_worse():
    """The revert guard as written-out cases: rows whose re-posed hand is forced to score worse (no contact, infinite penetration) take
    back the generated parameters and vertices, a zero offset, identity turns, iterate 0 and the scores of the hand as generated;
    every other row is the unforced run's; a forced row whose generated hand is itself without contact and infinitely deep would
    not be worse -- none is."""
    plain, clouds, f, sealed, pose, transform, hand, meshes = toy_hand_problem()
    options = dict(num_grasp=TOY_M, refine_steps=2, refine_spin=1.0, refine_curl=1.0)
    free = gref.compose(plain, clouds, f, sealed, pose, options, transform=transform, hand=hand)
    forced = [[1, 4], [], [0, 2, 5]]
    got = gref.compose(plain, clouds, f, sealed, pose, options, transform=transform, hand=hand, forced=forced)
    for i, (e, u, p) in enumerate(zip(got, free, plain)):
        rev, rev_free = e["refine_reverted"].astype(bool), u["refine_reverted"].astype(bool)
        want = rev_free.copy()
        want[forced[i]] = True
        assert np.array_equal(rev, want) and e["json"]["refine_reverted"] == want.astype(int).tolist()
        assert np.array_equal(gref.bits(e["params"][rev]), gref.bits(p["params"].numpy()[rev]))
        assert np.array_equal(gref.bits(e["vertices"][rev]), gref.bits(p["vertices"].numpy()[rev]))
        assert not e["refine_offset"][rev].any() and not e["refine_iter"][rev].any() and not e["refine_curl"][rev].any()
        assert not e["refine_rotation"][rev].any() and (e["stage"]["push"]["quat"][rev] == [1, 0, 0, 0]).all()
        for k in gref.SCORE_NAMES:
            assert np.array_equal(e[k][rev], e["stage"]["push"]["unreverted"][k + "0"][rev]), k
            assert np.array_equal(e[k][~rev], u[k][~rev]), k
        for k in ("params", "vertices", "refine_offset", "refine_iter", "refine_curl", "refine_rotation"):
            assert np.array_equal(e[k][~rev], u[k][~rev]), k
        pen = sref.grasp_scores(e["vertices"], f, e["stage"]["obj"])[0]
        assert np.array_equal(gref.bits(e["penetration"]), gref.bits(pen)), "the merged scores are not those of the hands written"
    assert any((u["refine_iter"][rows] > 0).any() for u, rows in zip(free, forced) if rows), "no forced row had moved: reverting it shows nothing"


def test_guard_classes_are_the_documented_rules_and_join_by_maximum():
    assert gref.mesh_class([0, 3, 3, -1, 5], np.asarray([0.0, 0.01, 0.0100001, np.nan, 1.0], F32), 1.0).tolist() == [0, 0, 1, 2, 1]
    assert gref.mesh_class([2], [F32(0.02)], 2.0).tolist() == [0] and gref.mesh_class([2], [np.nextafter(F32(0.02), F32(1))], 2.0).tolist() == [1]
    figs = {"volume": {"count": np.asarray([0, 20, -1, 3])},
            "parts": {"part_count": np.asarray([[1, 1, 0, 0, 0, 4], [0, 2, 2, 2, 0, 0], [1, 0, 0, 0, 0, 9], [-1] * 6]), "status": np.asarray([0, 0, 0, 1])},
            "self": {"pen_count": np.asarray([[0, 0, 0, 0, 0, 0], [2, 1, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [0, 0, 0, 3, 0, 0]]), "status": np.zeros(4, int)},
            "mesh": {"n_inside": np.asarray([4, 4, 0, -1]), "depth": np.asarray([0.02, 0.005, 0.0, np.nan], F32)}}
    off = dict(gref.OFF, volume_res=0.004)
    assert gref.guard_classes(off, figs) == {}
    on = dict(off, max_volume=1.0, min_fingers=2, need_thumb=True, max_self_verts=2, max_mesh_depth=1.0)
    got = gref.guard_classes(on, figs)
    assert list(got) == ["volume", "parts", "self", "mesh"] and {k: v.tolist() for k, v in got.items()} == {
        "volume": [0, 1, 2, 0], "parts": [0, 1, 1, 2], "self": [0, 1, 0, 1], "mesh": [1, 0, 0, 2]}
    assert gref.guard_classes(dict(off, need_thumb=True), figs)["parts"].tolist() == [0, 1, 0, 2]
    assert gref.guard_classes(dict(off, min_fingers=2), figs)["parts"].tolist() == [0, 0, 1, 2]
    # in compose: the class is the maximum of the ranking's and every guard's
    plain, clouds, f, sealed, pose, transform, hand, meshes = toy_hand_problem()
    options = dict(num_grasp=TOY_KEEP, candidates=TOY_M, parts=True, part_threshold=0.01, self_collision=True, mesh_depth=True, object_meshes=meshes,
                   volume=True, volume_res=0.004)
    e0 = gref.compose(plain, clouds, f, sealed, pose, options, transform=transform, hand=hand, mesh_closed=[True] * 3)[0]
    fingers = sorted(e0["stage_figures"]["parts"]["part_count"][:, :5].astype(bool).sum(1).tolist())
    limits = dict(min_fingers=fingers[TOY_M // 2], max_self_verts=0, max_mesh_depth=float(np.sort(e0["mesh_scores"]["depth"])[TOY_M // 2 - 1]) * 100.0,
                  max_volume=(int(np.sort(e0["volume_scores"]["count"])[TOY_M // 2 - 1]) + 0.5) * 0.004 ** 3 * 1e6)
    for e in gref.compose(plain, clouds, f, sealed, pose, dict(options, **limits), transform=transform, hand=hand, mesh_closed=[True] * 3):
        assert list(e["guards"]) == ["volume", "parts", "self", "mesh"]
        assert np.array_equal(e["cls"], np.maximum.reduce([e["cls_ranking"]] + list(e["guards"].values())))
        assert e["candidate"].tolist() == sref.segment_topk(e["cls"], e["key"], 1, TOY_M, TOY_KEEP)[0].tolist()
    print("toy guards of object 0:", {k: v.tolist() for k, v in e0["guards"].items()}, "limits", limits)


def test_compose_carries_the_beam_entries_through_the_selection():
    plain, clouds, f, sealed, pose, transform = toy_problem()
    for i, p in enumerate(plain):                                                      # a beam run's dicts: P = 2 poses of W = 3 ranks
        p.update(beam_pose=torch.arange(TOY_M) // 3, beam_rank=torch.arange(TOY_M) % 3, beam_duplicate_of=torch.tensor([-1, 0, -1, -1, -1, i - 1]))
    for e, p in zip(gref.compose(plain, clouds, f, sealed, pose, dict(num_grasp=TOY_KEEP, candidates=TOY_M, beam_width=3, beam_poses=2), transform=transform), plain):
        c = e["candidate"]
        assert e["keys"] == ["log_prob", "params", "vertices", "candidate", "scores", "json", *BEAM_FIELDS]
        assert list(e["json"])[-4:] == ["log_prob", *BEAM_FIELDS] and e["json"]["log_prob"] == p["log_prob"].numpy()[c].tolist()
        assert e["json"]["beam_pose"] == (c // 3).tolist() and e["json"]["beam_rank"] == (c % 3).tolist()
        assert e["beam_duplicate_of"].dtype == np.int64 and e["beam_duplicate_of"].tolist() == p["beam_duplicate_of"].numpy()[c].tolist()
    flat = gref.compose(plain, clouds, f, sealed, pose, dict(num_grasp=TOY_M, beam_width=3, beam_poses=2), transform=transform)
    assert all(e["keys"] == ["log_prob", "params", "vertices", "json", *BEAM_FIELDS] and e["json"]["beam_rank"] == [0, 1, 2] * 2 for e in flat)


def test_compose_does_not_depend_on_the_grouping_and_follows_the_stage_order():
    plain, clouds, f, sealed, pose, transform = toy_problem()
    full = dict(TOY_FULL)
    cache = {}
    both = gref.compose(plain, clouds, f, sealed, pose, full, transform=transform, cache=cache, cache_keys=[0, 1, 2])
    pen0 = np.sort(both[0]["scores"]["penetration"])
    cnt0 = np.sort(both[0]["volume_scores"]["count"])
    full.update(max_penetration=float(pen0[TOY_M - 2]), max_volume=(int(cnt0[TOY_M - 2]) + 0.5) * 0.004 ** 3 * 1e6)      # each demotes the worst one
    together = gref.compose(plain, clouds, f, sealed, pose, full, transform=transform, cache=cache, cache_keys=[0, 1, 2])
    for order in ([2, 0], [1]):                                                        # regrouped, and without the cache
        alone = gref.compose([plain[i] for i in order], [clouds[i] for i in order], f, sealed, pose, full, transform=transform)
        for i, e in zip(order, alone):
            assert json.dumps(e["json"]) == json.dumps(together[i]["json"]) and e["keys"] == together[i]["keys"]
            assert np.array_equal(e["candidate"], together[i]["candidate"])
    again = gref.compose(plain, clouds, f, sealed, pose, full, transform=transform, cache=cache, cache_keys=[0, 1, 2])
    assert [json.dumps(e["json"]) for e in again] == [json.dumps(e["json"]) for e in together], "the cache changes the result"
    moved = False
    for i, (e, p) in enumerate(zip(together, plain)):
        c, j = e["candidate"], e["json"]
        assert list(j) == ["recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact", "log_prob",
                           *gref.STABILITY_FIELDS, "rank", "novelty", "refine_offset", "refine_iter", "diversity", *gref.VOLUME_FIELDS]
        assert e["keys"] == ["log_prob", "wrench_sums", "stability_key", "rank", "novelty", "refine_offset", "refine_iter", "diversity",
                             "volume", "volume_scores", "params", "vertices", "candidate", "scores", "json"]
        assert len(set(c.tolist())) == TOY_KEEP and j["candidate"] == c.tolist() and "NaN" not in json.dumps(j)
        # 2, 3: parameters 0 .. 57 of the plain rows, the translation moved in fp32, the vertices those of the parameters
        raw = p["params"].numpy()[c]
        assert np.array_equal(e["params"][:, :58], raw[:, :58])
        assert np.array_equal(gref.bits(e["params"][:, 58:61]), gref.bits((raw[:, 58:61] + e["refine_offset"]).astype(F32)))
        assert np.array_equal(gref.bits(e["vertices"]), gref.bits(pose(e["params"])))
        moved |= bool((e["refine_iter"] > 0).any())
        # 4, 5: the figures of the re-posed hands
        want = wref.grasp_wrench(e["vertices"], f, np.repeat(clouds[i][:3].T.numpy()[None], TOY_KEEP, 0), 10.0)
        assert np.array_equal(gref.bits(e["wrench_sums"]), gref.bits(want["sums"])) and j["n_contact"] == want["n_contact"].tolist()
        vol = vref.grasp_volume(e["vertices"], *sealed, contact.hull_planes(clouds[i][:3].T.numpy().astype(np.float64)),
                                [0, len(contact.hull_planes(clouds[i][:3].T.numpy().astype(np.float64)))], np.zeros(TOY_KEEP, np.int64), h=0.004)
        assert j["volume_voxels"] == vol["count"].tolist() and (vol["count"] > 0).all()
        # 6, 7: the pool is the best of the classes and keys, the first pick its best, the picks a subset of it
        assert e["pool"].tolist() == sref.segment_topk(e["cls"], e["key"], 1, TOY_M, 5)[0].tolist()
        assert c[0] == e["pool"][0] and set(c.tolist()) <= set(e["pool"].tolist()) and e["rank"].tolist() == [e["pool"].tolist().index(x) for x in c]
        assert e["novelty"][0] == -1.0 and (e["novelty"][1:] > 0).all()
        # 8: the statistic of the kept parameters
        assert j["diversity"] == gref.diversity_entry(e["params"], 2) and sum(j["diversity"]["counts"]) == TOY_KEEP
    assert moved, "no toy hand was pushed: the refinement is not exercised"
    cls0 = together[0]["cls"]
    assert set(cls0.tolist()) == {0, 1}, "the two guards must demote some candidates of object 0 and not all"
    # without candidates: every row in order, the scores as fields of their own, the diversity last
    flat = gref.compose(plain, clouds, f, sealed, pose, dict(TOY_FULL, num_grasp=TOY_M, candidates=0, diverse_pool=0, select_by="penetration"),
                        transform=transform, cache=cache, cache_keys=[0, 1, 2])
    for e, t in zip(flat, together):
        assert list(e["json"]) == ["recon_params", "R_list", "trans_list", "r_list", "log_prob", "refine_offset", "refine_iter", "penetration",
                                   "n_interior", "n_contact", *gref.STABILITY_FIELDS, *gref.VOLUME_FIELDS, "diversity"]
        assert e["keys"] == ["log_prob", "refine_offset", "refine_iter", "penetration", "n_interior", "n_contact", "wrench_sums",
                             "stability_key", "volume", "diversity", "params", "vertices", "json"]
        assert np.array_equal(e["wrench_sums"], t["scores"]["sums"]) and np.array_equal(e["volume"]["count"], t["volume_scores"]["count"])
        assert np.array_equal(e["params"][t["candidate"]], t["params"])


def test_volume_class_is_the_documented_rule():
    cell = 0.004 ** 3 * 1e6
    assert gref.volume_class([0, 15, 16, -1, 2 ** 31 - 1], 1.0, 0.004).tolist() == [0, 0, 1, 2, 1]            # 1 cm^3 = 15.625 voxels
    assert gref.volume_class([15, 16], 15.5 * cell, 0.004).tolist() == [0, 1] and gref.volume_class([5, -1], INF, 0.004).tolist() == [0, 2]


# ------------------------------------------------------------------------------------------------------ GPU: shared state
class Ctx:
    """The net, its topology and what the tests share: plain runs, objects, and compose's steps 1 - 5 (computed once per object,
    rotation and refinement, as the stage references cost seconds)."""

    def __init__(self, net):
        self.net = net
        self.faces = np.asarray(net.rh_mano.faces)
        self.topo = generate._hand_topology(net, 778, torch.device(DEV))
        self.sealed = tuple(x.cpu().numpy() for x in self.topo.sealed())
        self.cache, self._plain, self._objs, self._limits, self._meshes = {}, {}, {}, {}, {}
        # the rig is the package's own (contact.FingerRig.from_mano, pinned by tests/test_grasp_refine_fingers.py), the label table the
        # packaged one: what the call itself uses without ``hand_parts``
        self.hand = gref.Hand(layer=net.rh_mano, rig=generate._finger_rig(net), parts=contact.HandParts.from_json())

    def pose_t(self, p):
        return self.net.rh_mano(betas=p[:, :10], global_orient=p[:, 10:13], hand_pose=p[:, 13:58], transl=p[:, 58:61]).vertices

    def pose(self, params):
        """compose's ``pose``: (vertices, joints) of the net's MANO layer."""
        p = torch.from_numpy(np.ascontiguousarray(params, F32)).to(DEV)
        with torch.no_grad():
            out = self.net.rh_mano(betas=p[:, :10], global_orient=p[:, 10:13], hand_pose=p[:, 13:58], transl=p[:, 58:61])
        return out.vertices.cpu().numpy(), out.joints.cpu().numpy()

    def tune_for(self, o):
        """compose's ``tune`` for the ttt settings of ``o``: contact.refine_ttt on the device, as the call runs it."""
        def tune(params, cloud):
            with torch.no_grad():
                out = contact.refine_ttt(self.net.rh_mano, self.topo, torch.from_numpy(np.ascontiguousarray(params, F32)).to(DEV),
                                         torch.from_numpy(np.ascontiguousarray(cloud, F32)).to(DEV), int(o["ttt_steps"]), o["ttt_lr"],
                                         o["ttt_momentum"], generate._ttt_targets(o["ttt_prior"]), o["ttt_w_pen"], o["ttt_w_con"],
                                         bool(o["ttt_keep_best"]))
            return {k: v.cpu().numpy() for k, v in out.items()}
        return tune

    def meshes(self, rotate):
        """One closed mesh of 12-triangle boxes per object, in the cloud's own frame: unrotated a box about STILL_CENTRE; rotated the
        union over the M blocks of the object, R_g^T (box about CENTRE - t), M closed components."""
        if rotate not in self._meshes:
            self._meshes[rotate] = [gref.rotated_boxes(SEED, i, M, h) if rotate else gref.box(h) for i, h in zip(INDICES, BOX_HALVES[rotate])]
        return self._meshes[rotate]

    def objects(self, rotate):
        """Three objects of two point counts that meet the hands of a run of at most M rows per object.  Rotated: always the objects of
        M blocks -- a run of fewer rows draws the first rotations of the M, its rows are rows of the M-row run, and the place the net
        puts a hand depends on the whole cloud it sees."""
        if rotate not in self._objs:
            clouds = gref.rotated_contact_objects(SEED, INDICES, M)[0] if rotate else gref.hand_clouds()
            assert len({c.shape[0] for c in clouds[:2]}) == 2
            self._objs[rotate] = [generate.object_tensor(c) for c in clouds]
        return self._objs[rotate]

    def plain(self, rotate, rows, log_prob, beam=None):
        """The plain run: no option on -- or, with ``beam`` = (poses, width), only those two (nothing is drawn then)."""
        if (rotate, rows, log_prob, beam) not in self._plain:
            kw = dict(beam_poses=beam[0], beam_width=beam[1]) if beam else dict(log_prob=log_prob)
            self._plain[rotate, rows, log_prob, beam] = generate.generate_for_objects(self.net, self.objects(rotate), rows, rotate,
                                                                                      seed_of(rotate), INDICES, **kw)
        return self._plain[rotate, rows, log_prob, beam]

    def expected(self, options, n_obj=3, forced=None):
        o = {**gref.OFF, **options}
        rows = o["candidates"] or o["num_grasp"]
        beam = (int(o["beam_poses"]), int(o["beam_width"])) if o["beam_width"] else None
        with_lp = not beam and (bool(o["log_prob"]) or (bool(o["candidates"]) and o["select_by"] == "log_prob"))
        if o["object_meshes"] is not None:
            o["object_meshes"] = o["object_meshes"][:n_obj]
        return gref.compose(self.plain(o["rotate"], rows, with_lp, beam)[:n_obj], self.objects(o["rotate"])[:n_obj], self.faces, self.sealed,
                            self.pose, o, cache=self.cache, cache_keys=[(o["rotate"], rows, beam, i) for i in range(n_obj)],
                            tune=self.tune_for(o) if o["ttt_steps"] else None, hand=self.hand, mesh_closed=[True] * n_obj,   # boxes: closed as built
                            forced=forced)

    def run(self, options, rows_per_call=16384, n_obj=3):
        o = {**gref.OFF, **options}
        keywords = {k: v for k, v in gref.api_keywords(options).items() if k != "rows_per_call"}
        if keywords.get("object_meshes") is not None:
            keywords["object_meshes"] = keywords["object_meshes"][:n_obj]
        return generate.generate_for_objects(self.net, self.objects(o["rotate"])[:n_obj], o["num_grasp"], o["rotate"],
                                             seed_of(o["rotate"]), INDICES[:n_obj], rows_per_call=rows_per_call, **keywords)

    def limits(self, rotate, refine_steps):
        """(max_penetration, max_volume) of the full stack: the median penetration of object 0's candidates as test_grasp_wrench.py
        takes it (torch's median: the lower middle), and (count + 0.5) * cell at the lower-half boundary of its voxel counts as
        test_grasp_volume.py does -- both from the stack itself with neither limit set."""
        if (rotate, refine_steps) not in self._limits:
            e = self.expected(dict(num_grasp=KEEP, rotate=rotate, candidates=M, select_by="stability", refine_steps=refine_steps, volume=True,
                                   volume_res=RES))[0]
            pen, cnt = np.sort(e["scores"]["penetration"]), np.sort(e["volume_scores"]["count"])
            limit = int(cnt[M // 2 - 1])
            X = (limit + 0.5) * RES ** 3 * 1e6
            assert contact.volume_limit(X, RES) == limit
            self._limits[rotate, refine_steps] = (float(pen[M // 2 - 1]), X)
        return self._limits[rotate, refine_steps]

    def stack(self, rotate, kind, guards=True, **changes):
        """The new full stack: all thirteen options but beam search, the push-out of ``kind``; with ``guards`` the five limits of
        guard_limits."""
        o = dict(num_grasp=KEEP, rotate=rotate, log_prob=True, candidates=M, select_by="stability", min_contact=1, diverse_pool=POOL,
                 diverse_space="params", refine_steps=STEPS, diversity=CLUSTERS, stability=True, torque_length=0.1, volume=True, volume_res=RES,
                 ttt_steps=TTT, parts=True, self_collision=True, mesh_depth=True, object_meshes=self.meshes(rotate), **FIGURE_SETTINGS[rotate],
                 **KINDS[kind])
        o["part_threshold"] = PART_THRESHOLD.get((rotate, kind), o["part_threshold"])
        if guards:
            o.update(self.guard_limits(rotate, kind))
        return {**o, **changes}

    def guard_limits(self, rotate, kind):
        """The five limits of the new full stack, each from the UNGUARDED composed reference of that stack at a rank statistic of object
        0's candidates (GUARD_RANKS): the penetration and the voxel count as ``limits`` takes them; min_fingers = the fingers in contact
        at that rank (fewer is demoted); max_self_verts = the self-penetrating vertices at that rank; max_mesh_depth = the depth at
        that rank, in cm (float64 of the fp32 depth times 100: dividing by 100 gives the fp32 back, so exactly the deeper rows are
        demoted).  need_thumb has no limit."""
        if ("guards", rotate, kind) not in self._limits:
            e = self.expected(self.stack(rotate, kind, guards=False))[0]
            rank, figs = GUARD_RANKS[rotate, kind], e["stage_figures"]
            limit = int(np.sort(e["volume_scores"]["count"])[rank["volume"]])
            X = (limit + 0.5) * RES ** 3 * 1e6
            assert contact.volume_limit(X, RES) == limit
            fingers = np.sort((figs["parts"]["part_count"][:, :5] >= 1).sum(axis=1))
            depth_cm = float(np.sort(figs["mesh"]["depth"])[rank["mesh"]]) * 100.0
            assert F32(depth_cm / 100.0) == np.sort(figs["mesh"]["depth"])[rank["mesh"]]
            self._limits["guards", rotate, kind] = dict(
                max_penetration=float(np.sort(e["scores"]["penetration"])[rank["penetration"]]), max_volume=X, min_fingers=int(fingers[rank["fingers"]]),
                need_thumb=True, max_self_verts=int(np.sort(figs["self"]["pen_count"].sum(axis=1))[rank["self"]]), max_mesh_depth=depth_cm)
        return self._limits["guards", rotate, kind]

    def full(self, rotate, select_by="stability", space="params", refine_steps=STEPS, **changes):
        max_pen, X = self.limits(rotate, refine_steps)
        return {**dict(num_grasp=KEEP, rotate=rotate, log_prob=True, candidates=M, select_by=select_by, min_contact=1, diverse_pool=POOL,
                       diverse_space=space, refine_steps=refine_steps, diversity=CLUSTERS, stability=True, max_penetration=max_pen,
                       torque_length=0.1, volume=True, volume_res=RES, max_volume=X), **changes}


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    import scipy.spatial  # noqa: F401  the hulls need it: a missing scipy is an error here, not a skip
    from test_grasp_select import _gennet
    return Ctx(_gennet(tmp_path_factory.mktemp("combined")))


def statuses(res):
    return [res[k]["status"] for k in ("volume", "volume_scores") if k in res]


def check_case(ctx, options, calls, n_obj=3, what=""):
    """The call at every ``rows_per_call`` of ``calls`` against compose, object by object; the JSON text the same for all of them and
    free of NaN; every volume status 0 (the error flags raise inside the call).  Returns (the first call's dicts, compose's)."""
    exp = ctx.expected(options, n_obj)
    first, text0 = None, None
    for rows_per_call in calls:
        got = ctx.run(options, rows_per_call, n_obj)
        assert len(got) == n_obj
        for i, (g, e) in enumerate(zip(got, exp)):
            gref.assert_result(g, e, f"{what} rows_per_call {rows_per_call} object {i}")
            assert all(int(s.abs().max()) == 0 for s in statuses(g)), "a volume status is not 0"
        text = [json.dumps(g["json"]) for g in got]
        assert "NaN" not in "".join(text)
        if first is None:
            first, text0 = got, text
        assert text == text0, f"{what} rows_per_call {rows_per_call}: the JSON differs from the first call's"
    return first, exp


def assert_contact(scores, what):
    """At least half of an object's candidates touch it, and at least half penetrate it."""
    n_ct, pen = np.asarray(scores["n_contact"]), np.asarray(scores["penetration"])
    print(f"{what}: n_contact {n_ct.tolist()} penetration {pen.tolist()}")
    assert 2 * int((n_ct >= 1).sum()) >= len(n_ct), f"{what}: fewer than half of the candidates touch the object"
    assert 2 * int((pen > 0).sum()) >= len(pen), f"{what}: fewer than half of the candidates penetrate the object"


def assert_inputs_not_vacuous(ctx, rotate):
    """The conditions on the inputs of the full stack, from compose's steps 1 - 5 (which every case compares the device with)."""
    options = ctx.full(rotate)
    exp = ctx.expected(options)
    raw = ctx.expected({**options, "refine_steps": 0})
    for i, e in enumerate(exp):
        assert_contact(e["scores"], f"rotate {rotate} object {i}")
    iters = np.concatenate([e["stage"]["iter"] for e in exp])
    moved = [int((e["stage_volume"]["count"] != r["stage_volume"]["count"]).sum()) for e, r in zip(exp, raw)]
    print(f"rotate {rotate}: refine_iter {iters.tolist()}, rows whose voxel count moves with the push-out, per object: {moved}")
    assert (iters > 0).any(), "no row was pushed"
    assert sum(moved) >= 1, "no row's voxel count differs between the refined and the unrefined hands"
    count, pen = exp[0]["volume_scores"]["count"], exp[0]["scores"]["penetration"]
    over = count > contact.volume_limit(options["max_volume"], RES)
    deep = pen > F32(options["max_penetration"])
    print(f"rotate {rotate} object 0: voxel counts {count.tolist()} over {over.astype(int).tolist()} deep {deep.astype(int).tolist()}")
    assert len(set(count.tolist())) >= 3 and (count >= 0).all()
    assert 0 < over.sum() < M, "max_volume must demote some candidates of object 0 and not all"
    assert 0 < deep.sum() < M, "max_penetration must demote some candidates of object 0 and not all"
    assert (over & ~deep).any() and (deep & ~over).any(), "each guard must demote a candidate the other leaves alone"
    assert all(int(np.abs(e["stage_volume"]["status"]).max()) == 0 for e in exp + raw)


def assert_selection_not_vacuous(exp, what):
    beyond = any((e["candidate"] >= KEEP).any() for e in exp)
    spread = [sorted(e["candidate"].tolist()) != sorted(e["best"].tolist()) for e in exp]
    print(f"{what}: kept {[e['candidate'].tolist() for e in exp]} best-ranked {[e['best'].tolist() for e in exp]}")
    assert beyond, f"{what}: only the first {KEEP} candidates were kept"
    assert any(spread), f"{what}: the farthest-point picks are the best-ranked candidates for every object"


# ------------------------------------------------------------------------------------------------------ GPU: the candidates path
@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("space", ["params", "verts"])
@pytest.mark.parametrize("select_by", ["penetration", "log_prob", "stability"])
def test_full_stack_equals_the_composed_reference(ctx, select_by, space, rotate):
    assert_inputs_not_vacuous(ctx, rotate)
    options = ctx.full(rotate, select_by, space)
    got, exp = check_case(ctx, options, GROUPINGS, what=f"{select_by}/{space}/rotate {rotate}")
    assert_selection_not_vacuous(exp, f"{select_by}/{space}/rotate {rotate}")
    for g in got:
        assert list(g["json"]) == ["recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact",
                                   "log_prob", *gref.STABILITY_FIELDS, "rank", "novelty", "refine_offset", "refine_iter", "diversity",
                                   *gref.VOLUME_FIELDS]


LEAVE_ONE_OUT = {"refine": dict(refine_steps=0), "diverse pool": dict(diverse_pool=0), "diversity": dict(diversity=0),
                 "stability figures": dict(select_by="penetration", stability=False), "volume": dict(volume=False, max_volume=INF),
                 "log_prob": dict(log_prob=False)}
LEFT_OUT_FIELDS = {"refine": ["refine_offset", "refine_iter"], "diverse pool": ["rank", "novelty"], "diversity": ["diversity"],
                   "stability figures": list(gref.STABILITY_FIELDS), "volume": list(gref.VOLUME_FIELDS), "log_prob": ["log_prob"]}


@pytest.mark.gpu
@pytest.mark.parametrize("left_out", list(LEAVE_ONE_OUT))
def test_full_stack_with_one_option_off(ctx, left_out):
    """The six lengths of _select_call's packed copy."""
    changes = LEAVE_ONE_OUT[left_out]
    options = ctx.full(False, refine_steps=changes.get("refine_steps", STEPS), **{k: v for k, v in changes.items() if k != "refine_steps"})
    got, exp = check_case(ctx, options, GROUPINGS, what=f"without {left_out}")
    full = list(ctx.expected(ctx.full(False))[0]["json"])
    for g in got:
        assert list(g["json"]) == [f for f in full if f not in LEFT_OUT_FIELDS[left_out]]


@pytest.mark.gpu
def test_figure_only_switches_add_fields_and_change_nothing(ctx):
    base_options = dict(num_grasp=KEEP, rotate=False, candidates=M)
    base, _ = check_case(ctx, base_options, GROUPINGS, what="best-of-M alone")
    added = {"stability": (dict(stability=True), list(gref.STABILITY_FIELDS)),
             "volume": (dict(volume=True, volume_res=RES, max_volume=INF), list(gref.VOLUME_FIELDS)),
             "diversity": (dict(diversity=CLUSTERS), ["diversity"]), "log_prob": (dict(log_prob=True), ["log_prob"])}
    everything = {k: v for switch, _ in added.values() for k, v in switch.items()}
    added["all"] = (everything, ["log_prob", *gref.STABILITY_FIELDS, "diversity", *gref.VOLUME_FIELDS])
    for name, (switch, fields) in added.items():
        got, _ = check_case(ctx, {**base_options, **switch}, GROUPINGS, what=f"best-of-M and {name}")
        for g, b in zip(got, base):
            assert torch.equal(g["candidate"], b["candidate"]) and torch.equal(g["params"], b["params"]) and torch.equal(g["vertices"], b["vertices"])
            assert list(g["json"]) == list(b["json"]) + fields, name
            assert {f: g["json"][f] for f in b["json"]} == b["json"], name
            assert json.dumps({f: g["json"][f] for f in b["json"]}) == json.dumps(b["json"]), name


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [False, True])
def test_stage_order_of_a_refined_call(ctx, rotate):
    """Directly, not through compose: the kept vertices are MANO of the kept parameters, and the wrench sums and the volume of a kept row
    are the references' on THOSE vertices -- not on the hands from before the push-out."""
    options = ctx.full(rotate)
    plain = ctx.plain(rotate, M, True)
    objs = ctx.objects(rotate)
    transform = gref.device_transform(torch.device(DEV))
    text = []
    for rows_per_call in GROUPINGS:
        got = ctx.run(options, rows_per_call)
        text.append([json.dumps(g["json"]) for g in got])
        assert text[-1] == text[0], f"rows_per_call {rows_per_call}: the JSON differs from the first call's"
        sums_differ = count_differ = depth_differ = 0
        for i, (g, p) in enumerate(zip(got, plain)):
            cand = g["candidate"]
            assert torch.equal(g["vertices"], ctx.pose_t(g["params"].contiguous())), f"object {i}: the vertices are not those of the parameters"
            assert torch.equal(g["params"][:, 58:61], p["params"][cand][:, 58:61] + g["refine_offset"])
            Rt = np.asarray(g["json"]["R_list"], np.float64)
            R, t = Rt[:, :, :3].astype(F32), Rt[0, :, 3].astype(F32)
            cloud = transform(objs[i], R, t)
            planes = contact.hull_planes(objs[i][:3].T.numpy().astype(np.float64))
            frame = dict(R=R, t=t) if rotate else {}
            figures = []
            for verts in (g["vertices"].cpu().numpy(), p["vertices"][cand].cpu().numpy()):       # the re-posed hands, the hands before
                w = wref.grasp_wrench(verts, ctx.faces, cloud, 10.0)
                v = vref.grasp_volume(verts, *ctx.sealed, planes, [0, len(planes)], np.zeros(KEEP, np.int64), h=RES, **frame)
                figures.append((w["sums"], v["count"], v["depth"]))
            (sums, count, depth), (sums0, count0, depth0) = figures
            gref.same_bits(g["wrench_sums"], sums, f"object {i} sums")
            gref.same_bits(g["volume"]["count"], count, f"object {i} count")
            gref.same_bits(g["volume"]["depth"], depth, f"object {i} depth")
            sums_differ += int((gref.bits(sums) != gref.bits(sums0)).any(axis=1).sum())
            count_differ += int((count != count0).sum())
            depth_differ += int((gref.bits(depth) != gref.bits(depth0)).sum())
        print(f"rotate {rotate} rows_per_call {rows_per_call}: kept rows whose sums / count / depth differ from the unrefined hands': "
              f"{sums_differ} / {count_differ} / {depth_differ}")
        assert sums_differ >= 1 and count_differ >= 1 and depth_differ >= 1


# ------------------------------------------------------------------------------------------------------ GPU: without candidates
def documented_refine(o):
    """The push-out's entries, dict keys and JSON fields alike, in the order generate.REFINE_PIECES documents."""
    if not o["refine_steps"]:
        return []
    return (["refine_offset", "refine_iter"] + (["refine_rotation"] if o.get("refine_spin") else [])
            + (["refine_curl", "refine_reverted"] if o.get("refine_curl") else []))


def documented_fields(o):
    """The JSON's fields without candidates, in the order generate.py documents: the diversity stands between the volume and the
    figures after it; the gradient refinement's and the beam's fields are attached last."""
    stab, refine = o["stability"], bool(o["refine_steps"])
    return (["recon_params", "R_list", "trans_list", "r_list"] + (["log_prob"] if o["log_prob"] or o.get("beam_width") else [])
            + documented_refine(o) + (["penetration", "n_interior", "n_contact"] if refine or stab else [])
            + (list(gref.STABILITY_FIELDS) if stab else []) + (list(gref.VOLUME_FIELDS) if o["volume"] else [])
            + (["diversity"] if o["diversity"] else []) + (list(gref.PARTS_FIELDS) if o.get("parts") else [])
            + (list(gref.SELF_FIELDS) if o.get("self_collision") else []) + (list(gref.MESH_FIELDS) if o.get("mesh_depth") else [])
            + (TTT_FIELDS if o.get("ttt_steps") else []) + (BEAM_FIELDS if o.get("beam_width") else []))


def documented_keys(o):
    stab, refine = o["stability"], bool(o["refine_steps"])
    return ((["log_prob"] if o["log_prob"] or o.get("beam_width") else []) + documented_refine(o)
            + (["penetration", "n_interior", "n_contact"] if refine or stab else []) + (["wrench_sums", "stability_key"] if stab else [])
            + (["volume"] if o["volume"] else []) + (["diversity"] if o["diversity"] else []) + (["parts"] if o.get("parts") else [])
            + (["self"] if o.get("self_collision") else []) + (["mesh"] if o.get("mesh_depth") else []) + ["params", "vertices", "json"]
            + (TTT_FIELDS if o.get("ttt_steps") else []) + (BEAM_FIELDS if o.get("beam_width") else []))


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("refine_steps", [0, STEPS])
def test_every_combination_without_candidates(ctx, refine_steps, rotate):
    """All 16 combinations of stability x volume x diversity x log_prob per refinement setting (rotated: the four with diversity and
    log_prob on), two objects of two point counts, G rows each: the three slicings of the packed copy in _generate_call."""
    seen = set()
    for stab, vol, div, lp in itertools.product([False, True], [False, True], [0, CLUSTERS], [False, True]):
        if rotate and not (div and lp):
            continue
        options = dict(num_grasp=G, rotate=rotate, refine_steps=refine_steps, stability=stab, volume=vol, volume_res=RES, diversity=div,
                       log_prob=lp)
        got, exp = check_case(ctx, options, (16384, 1), n_obj=2, what=f"refine {refine_steps} stability {stab} volume {vol} diversity {div} "
                                                                      f"log_prob {lp} rotate {rotate}")
        for g in got:
            assert list(g) == documented_keys(options) and list(g["json"]) == documented_fields(options)
            seen.add(len(g["json"]))
        if stab:
            for i, e in enumerate(exp):
                assert (e["n_contact"] >= 1).any() and (e["penetration"] > 0).any(), f"object {i}: no hand touches it"
        if refine_steps and stab and vol and div and lp:
            assert any((e["refine_iter"] > 0).any() for e in exp), "no row was pushed"
    print(f"refine {refine_steps} rotate {rotate}: JSON lengths seen {sorted(seen)}")


# ------------------------------------------------------------------------------------------------------ GPU: every figure together
def box(half, centre=gref.STILL_CENTRE):
    """A closed box about ``centre``, 12 outward triangles (tests/test_grasp_mesh.py::cube, moved to the hand)."""
    v = np.asarray([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64) * half + np.asarray(centre)
    f = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    return v, np.asarray(f, np.int64)


PARTS_FIELDS = ["fingers_in_contact", "part_contact", "part_dist", "hand_contact_map"]
MESH_FIELDS = ["mesh_depth", "mesh_interior", "mesh_closed", "mesh_penetration_map"]
SCORES = ["penetration", "n_interior", "n_contact"]
ALONE = {"stability": dict(stability=True), "volume": dict(volume=True, volume_res=RES), "parts": dict(parts=True),
         "self": dict(self_collision=True), "mesh": dict(mesh_depth=True), "diversity": dict(diversity=CLUSTERS), "log_prob": dict(log_prob=True)}
TOGETHER_KEYS = {0: ["log_prob", *SCORES, "wrench_sums", "stability_key", "volume", "diversity", "parts", "self", "mesh", "params", "vertices", "json"],
                 M: ["log_prob", "wrench_sums", "stability_key", "diversity", "volume", "volume_scores", "parts", "part_scores", "self",
                     "self_scores", "mesh", "mesh_scores", "params", "vertices", "candidate", "scores", "json"]}
TOGETHER_FIELDS = {0: ["recon_params", "R_list", "trans_list", "r_list", "log_prob", *SCORES, *gref.STABILITY_FIELDS, *gref.VOLUME_FIELDS,
                       "diversity", *PARTS_FIELDS, *contact.SELF_FIELDS, *MESH_FIELDS],
                   M: ["recon_params", "R_list", "trans_list", "r_list", "candidate", *SCORES, "log_prob", *gref.STABILITY_FIELDS, "diversity",
                       *gref.VOLUME_FIELDS, *PARTS_FIELDS, *contact.SELF_FIELDS, *MESH_FIELDS]}


def same_entry(got, want, what):
    """A dict entry of one run against the same entry of another: tensors byte for byte (so a NaN compares too), the tensors of a nested
    dict that the other run has as well, anything else by ``==``."""
    if torch.is_tensor(want):
        assert got.dtype == want.dtype and got.shape == want.shape, what
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), what
    elif isinstance(want, dict) and any(torch.is_tensor(v) for v in want.values()):
        assert set(want) <= set(got), (what, set(got), set(want))
        for k, v in want.items():
            same_entry(got[k], v, f"{what}[{k}]")
    else:
        assert got == want, what


@pytest.mark.gpu
@pytest.mark.parametrize("candidates", [0, M])
def test_every_figure_together_is_every_figure_alone(ctx, candidates):
    """Stability, volume, parts, self-collision, mesh depth, diversity and log_prob in ONE call, on both paths, with no guard limit: none
    of them changes a parameter, so every dict entry and every JSON field equals the same entry of the run with that switch alone (each
    pinned by its own stage test), and the keys and fields come in the documented order.  Parts, self-collision and mesh depth ride
    together in the call's one copy nowhere else."""
    base = dict(num_grasp=G, rotate=False, candidates=candidates, object_meshes=[box(0.05), box(0.06)])
    alone = {name: ctx.run({**base, **switch}, n_obj=2) for name, switch in ALONE.items()}
    everything = {**base, **{k: v for switch in ALONE.values() for k, v in switch.items()}}
    text0 = None
    for rows_per_call in (16384, 1):
        got = ctx.run(everything, rows_per_call, n_obj=2)
        for i, g in enumerate(got):
            assert list(g) == TOGETHER_KEYS[candidates] and list(g["json"]) == TOGETHER_FIELDS[candidates], (list(g), list(g["json"]))
            seen_keys, seen_fields = set(), set()
            for name, runs in alone.items():
                one = runs[i]
                for k in one:
                    if k != "json":
                        same_entry(g[k], one[k], f"rows_per_call {rows_per_call} object {i} {name} alone: {k}")
                for f in one["json"]:
                    assert g["json"][f] == one["json"][f], (rows_per_call, i, name, f)
                assert json.dumps({f: g["json"][f] for f in one["json"]}) == json.dumps(one["json"]), (rows_per_call, i, name)
                seen_keys |= set(one)
                seen_fields |= set(one["json"])
            assert seen_keys == set(g) and seen_fields == set(g["json"]), "an entry of the combined run has no run of its own"
        text = [json.dumps(g["json"]) for g in got]
        assert "NaN" not in "".join(text)
        text0 = text0 or text
        assert text == text0, f"rows_per_call {rows_per_call}: the JSON differs from the first call's"
    # the conditions on the inputs
    voxels = [g["json"]["volume_voxels"] for g in got]
    fingers = [g["json"]["fingers_in_contact"] for g in got]
    inside = [g["json"]["mesh_interior"] for g in got]
    print(f"candidates {candidates}: voxels {voxels} fingers in contact {fingers} vertices inside the boxes {inside} "
          f"self-penetrating {[g['json']['self_penetrating'] for g in got]}")
    assert all(any(v is not None and v > 0 for v in obj) for obj in voxels), "an object has no row with a positive voxel count"
    assert any(f is not None and f > 0 for obj in fingers for f in obj), "no finger is in contact"
    assert all(any(n is not None and n > 0 for n in obj) for obj in inside), "an object has no row with a vertex inside its box"
    assert all(g["json"]["mesh_closed"] is True for g in got)


# ------------------------------------------------------------------------------------------------------ GPU: the seven newer options
def guard_demotions(e, options):
    """Per guard, the candidates of one object it demotes, from compose's own stages: max_penetration (inside select_keys' class; its
    rule restated: penetration > fp32 limit), then the four figures' guards."""
    deep = e["scores"]["penetration"] > F32(options["max_penetration"])
    return {"max_penetration": deep, **{k: g > 0 for k, g in e["guards"].items()}}


def assert_stack_not_vacuous(ctx, rotate, kind):
    """The conditions on the inputs of the new full stack, from compose's own stages; the numbers are printed."""
    options = ctx.stack(rotate, kind)
    exp = ctx.expected(options)
    what = f"rotate {rotate} {kind}"
    demoted = [guard_demotions(e, options) for e in exp]
    names = list(demoted[0])
    assert names == ["max_penetration", "volume", "parts", "self", "mesh"], names
    for name in names:
        rows = [d[name].astype(int).tolist() for d in demoted]
        alone = [int((d[name] & ~np.any([d[k] for k in names if k != name], axis=0)).sum()) for d in demoted]
        print(f"{what}: {name} demotes {rows}, alone {alone}")
        assert any(0 < sum(r) < M for r in rows), f"{what}: {name} must demote some candidates of an object and not all"
        assert sum(alone) >= 1, f"{what}: {name} demotes no candidate that the other guards leave alone"
    counts = [e["stage_figures"]["parts"]["part_count"][:, :5] >= 1 for e in exp]
    few, no_thumb = [c.sum(axis=1) < options["min_fingers"] for c in counts], [~c[:, 0] for c in counts]
    only = [int((a & ~b).sum()) for a, b in zip(few, no_thumb)], [int((b & ~a).sum()) for a, b in zip(few, no_thumb)]
    print(f"{what}: min_fingers {options['min_fingers']} demotes alone {only[0]}, need_thumb alone {only[1]}")
    assert options["min_fingers"] >= 1, "min_fingers = 0 is the guard switched off"
    if rotate:                                                                         # unrotated: see GUARD_RANKS
        assert sum(only[0]) >= 1, "min_fingers changes no row's class that need_thumb leaves"
        assert sum(only[1]) >= 1, "need_thumb changes no row's class that min_fingers leaves"
    pushes = [e["stage"]["push"] for e in exp]
    iters = np.concatenate([p["iter"] for p in pushes])
    turned = np.concatenate([(p["quat"][:, 0] != 1) for p in pushes]) if kind != "translation" else None
    curled = np.concatenate([(p["finger_quat"][..., 0] != 1).any(axis=1) for p in pushes]) if kind == "curl" else None
    reverted = np.concatenate([p["reverted"] for p in pushes]) if kind == "curl" else None
    ttt_iter = np.concatenate([e["stage"]["ttt"]["iter"] for e in exp])
    tuned = np.concatenate([(e["stage"]["params"] != e["stage"]["pushed_params"]).any(axis=1) for e in exp])
    print(f"{what}: refine_iter {iters.tolist()} turned {None if turned is None else turned.astype(int).tolist()} curled "
          f"{None if curled is None else curled.astype(int).tolist()} reverted {None if reverted is None else reverted.tolist()} ttt_iter "
          f"{ttt_iter.tolist()} changed by ttt {tuned.astype(int).tolist()}")
    assert (iters > 0).any(), "no row was pushed"
    assert turned is None or turned.any(), "no row was turned"
    assert curled is None or curled.any(), "no finger was curled"
    assert ((ttt_iter > 0) & tuned).any(), "no row was changed by the gradient refinement"
    assert any((e["candidate"] >= KEEP).any() for e in exp), f"only the first {KEEP} candidates were kept"
    inside = [e["stage_figures"]["mesh"]["n_inside"].tolist() for e in exp]
    fingers = [(e["stage_figures"]["parts"]["part_count"][:, :5] >= 1).sum(axis=1).tolist() for e in exp]
    own = [e["stage_figures"]["self"]["pen_count"].sum(axis=1).tolist() for e in exp]
    print(f"{what}: vertices inside the mesh {inside} fingers in contact {fingers} self-penetrating {own}")
    assert all(max(x) > 0 for x in inside), "an object has no row with a vertex inside its mesh: a wrong frame, or a box off the hands"
    assert all(max(x) > 0 for x in fingers), "an object has no row with a finger in contact"
    assert any(max(x) > 0 for x in own), "no row has a self-penetrating vertex"
    assert all(int(np.abs(e["stage_volume"]["status"]).max()) == 0 and (e["stage_figures"]["mesh"]["status"] == 0).all() for e in exp)


def stack_refine(kind):
    return documented_refine(dict(refine_steps=STEPS, **KINDS[kind]))


def stack_fields(kind, beam=False):
    refine = stack_refine(kind)
    return ["recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact", "log_prob",
            *gref.STABILITY_FIELDS, "rank", "novelty", *refine, "diversity", *gref.VOLUME_FIELDS, *gref.PARTS_FIELDS, *gref.SELF_FIELDS,
            *gref.MESH_FIELDS, *TTT_FIELDS] + (BEAM_FIELDS if beam else [])


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_new_full_stack_equals_the_composed_reference(ctx, kind, rotate):
    """All thirteen options but beam search in ONE call, with all five guards limited, each push-out kind in turn, rotated too."""
    assert_stack_not_vacuous(ctx, rotate, kind)
    options = ctx.stack(rotate, kind)
    got, exp = check_case(ctx, options, GROUPINGS, what=f"{kind}/rotate {rotate}")
    for g in got:
        assert list(g["json"]) == stack_fields(kind) and g["json"]["mesh_closed"] is True
        assert list(g) == ["log_prob", "wrench_sums", "stability_key", "rank", "novelty", *stack_refine(kind), "diversity", "volume",
                           "volume_scores", "parts", "part_scores", "self", "self_scores", "mesh", "mesh_scores", "params", "vertices", "candidate",
                           "scores", "json", *TTT_FIELDS]


NEW_LEAVE_ONE_OUT = {"spin": dict(refine_spin=0.0), "curl": dict(refine_curl=0.0), "ttt": dict(ttt_steps=0),
                     "parts": dict(parts=False, min_fingers=0, need_thumb=False), "self": dict(self_collision=False, max_self_verts=None),
                     "mesh": dict(mesh_depth=False, max_mesh_depth=INF, object_meshes=None)}
NEW_LEFT_OUT_FIELDS = {"spin": ["refine_rotation"], "curl": ["refine_curl", "refine_reverted"], "ttt": TTT_FIELDS, "parts": list(gref.PARTS_FIELDS),
                       "self": list(gref.SELF_FIELDS), "mesh": list(gref.MESH_FIELDS)}


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("left_out", list(NEW_LEAVE_ONE_OUT))
def test_new_full_stack_with_one_option_off(ctx, left_out, rotate):
    """The new full stack (articulated push-out with the turn) without one of the newer options, rotated too; the limits stay the full
    stack's."""
    options = ctx.stack(rotate, "curl", **NEW_LEAVE_ONE_OUT[left_out])
    got, _ = check_case(ctx, options, GROUPINGS, what=f"without {left_out} rotate {rotate}")
    for g in got:
        assert list(g["json"]) == [f for f in stack_fields("curl") if f not in NEW_LEFT_OUT_FIELDS[left_out]]


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [False, True])
def test_newer_options_without_candidates(ctx, rotate):
    """_generate_call without candidates: every figure switch on with each push-out kind, gradient refinement after the articulated
    push-out, and gradient refinement alone; two objects of two point counts, G rows each."""
    figures = dict(stability=True, volume=True, volume_res=RES, diversity=CLUSTERS, log_prob=True, parts=True, self_collision=True, mesh_depth=True,
                   object_meshes=ctx.meshes(rotate), **FIGURE_SETTINGS[rotate])
    cases = {kind: dict(refine_steps=STEPS, **kw) for kind, kw in KINDS.items()}
    cases["ttt after curl"] = dict(refine_steps=STEPS, ttt_steps=TTT, **KINDS["curl"])
    cases["ttt after curl, no stability"] = dict(refine_steps=STEPS, ttt_steps=TTT, stability=False, **KINDS["curl"])
    cases["ttt alone"] = dict(ttt_steps=TTT)
    cases["ttt alone, no figure"] = dict(stability=False, volume=False, diversity=0, log_prob=False, parts=False, self_collision=False,
                                         mesh_depth=False, object_meshes=None, ttt_steps=TTT)
    for name, case in cases.items():
        options = {**dict(num_grasp=G, rotate=rotate), **figures, **case}
        got, exp = check_case(ctx, options, (16384, 1), n_obj=2, what=f"{name} rotate {rotate}")
        o = {**gref.OFF, **options}
        for g in got:
            assert list(g) == documented_keys(o) and list(g["json"]) == documented_fields(o), (name, list(g), list(g["json"]))
        if o["ttt_steps"]:
            assert any(((e["ttt_iter"] > 0) & (e["stage"]["params"] != e["stage"]["pushed_params"]).any(axis=1)).any() for e in exp), f"{name}: no row was tuned"
        if o["refine_curl"] and o["ttt_steps"] and not o["stability"]:                # the guard's scores must not survive the ttt pass
            differ = sum(int((gref.bits(e["penetration"]) != gref.bits(e["stage"]["push"]["merged"]["penetration"])).sum()) for e in exp)
            print(f"{name} rotate {rotate}: rows whose penetration differs from the push-out guard's: {differ}")
            assert differ >= 1, "every row's score after ttt equals the guard's: stale scores would pass"


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [False, True])
def test_figures_of_the_new_stack_are_those_of_the_hands_written(ctx, rotate):
    """Directly, not through compose: for the kept rows of the new full stack (articulated push-out, gradient refinement) the vertices
    are MANO of the parameters written, and the parts, self-collision and mesh figures are the references' on THOSE vertices -- and for
    at least one kept row they differ from the references' on the hands before the push-out, and on the hands before refine_ttt."""
    options = ctx.stack(rotate, "curl")
    plain = ctx.plain(rotate, M, True)
    before_ttt = ctx.run(dict(num_grasp=M, rotate=rotate, refine_steps=STEPS, **KINDS["curl"]))      # all M rows, pushed out, not tuned
    objs, meshes = ctx.objects(rotate), ctx.meshes(rotate)
    transform = gref.device_transform(torch.device(DEV))
    labels = ctx.hand.parts.labels
    source, pairs = cref.seam_sources(labels, ctx.faces, options["self_seam"]), cref.default_pairs(6, True)
    got = ctx.run(options)
    differ = {"push-out": [0, 0, 0], "ttt": [0, 0, 0]}
    for i, (g, p, b) in enumerate(zip(got, plain, before_ttt)):
        cand = g["candidate"]
        assert torch.equal(g["vertices"], ctx.pose_t(g["params"].contiguous())), f"object {i}: the vertices are not those of the parameters"
        assert np.array_equal(gref.bits(np.asarray(g["json"]["recon_params"], F32)[:, 0]), gref.bits(g["params"].cpu().numpy()))
        Rt = np.asarray(g["json"]["R_list"], np.float64)
        R, t = Rt[:, :, :3].astype(F32), Rt[0, :, 3].astype(F32)
        cloud = transform(objs[i], R, t)
        frame = dict(R=R, t=t) if rotate else {}
        mv, mf = np.asarray(meshes[i][0], F32), meshes[i][1]
        figures = []
        for verts in (g["vertices"], p["vertices"][cand], b["vertices"][cand]):                   # written, as generated, before ttt
            verts = verts.cpu().numpy()
            figures.append((pref.grasp_parts(verts, labels, 6, cloud, options["part_threshold"] ** 2),
                            cref.grasp_self(verts, ctx.faces, labels, source, 6, pairs, options["self_reach"] ** 2, options["self_margin"]),
                            mref.grasp_mesh(verts, mv, [0, len(mv)], mf, [0, len(mf)], np.zeros(KEEP, np.int64), **frame)))
        parts, own, mesh = figures[0]
        for k in gref.PARTS_PIECES:
            gref.same_bits(g["parts"][k], parts[k], f"object {i} parts[{k}]")
        for k in gref.SELF_PIECES:
            gref.same_bits(g["self"][k], own[k], f"object {i} self[{k}]")
        for k in gref.MESH_PIECES:
            gref.same_bits(g["mesh"][k], mesh[k], f"object {i} mesh[{k}]")
        assert g["json"]["hand_contact_map"] == pref.contact_map(parts["mask"], 778) and g["json"]["mesh_penetration_map"] == pref.contact_map(mesh["mask"], 778)
        for name, other in (("push-out", figures[1]), ("ttt", figures[2])):
            differ[name][0] += int((gref.bits(parts["part_min"]) != gref.bits(other[0]["part_min"])).any(axis=1).sum())
            differ[name][1] += int((gref.bits(own["gap_min"]) != gref.bits(other[1]["gap_min"])).any(axis=1).sum())
            differ[name][2] += int((gref.bits(mesh["depth"]) != gref.bits(other[2]["depth"])).sum())
    print(f"rotate {rotate}: kept rows whose parts / self / mesh figures differ from those of the hands before the push-out, before ttt: {differ}")
    assert all(n >= 1 for counts in differ.values() for n in counts)


FORCED = [[1, 6], [], [0, 3, 4]]                        # per object, the candidates whose re-posed hands are reported as worse


def force_worse(monkeypatch, queue):
    """contact.grasp_scores, as generate sees it, wrapped (tests/test_grasp_refine_fingers.py::_force_worse, for several calls): every
    call made by the articulated push-out's guard takes the next entry of ``queue`` -- the rows of that call it reports without a
    contact and with an infinite penetration.  Every other call, and every other row, is the real one's."""
    # the guard's call is told from the call's other launches by its caller's name: a private function of generate.py
    assert callable(getattr(generate, "_refine_fingers_call", None)), "generate._refine_fingers_call is gone: name the guard's new home here"
    real = contact.grasp_scores

    def forced(topology, hand_xyz, obj_xyz, *a, **k):
        out = dict(real(topology, hand_xyz, obj_xyz, *a, **k))
        if inspect.stack()[1].function == "_refine_fingers_call":
            rows = torch.as_tensor(queue.pop(0), dtype=torch.int64, device=hand_xyz.device)
            out["penetration"], out["n_contact"] = out["penetration"].clone(), out["n_contact"].clone()
            out["penetration"][rows] = float("inf")
            out["n_contact"][rows] = 0
        return out
    monkeypatch.setattr(contact, "grasp_scores", forced)


@pytest.mark.gpu
@pytest.mark.parametrize("candidates", [0, M])
def test_forced_reverts_are_composed(ctx, candidates, monkeypatch):
    """No row of these inputs reverts unforced, so the guard's revert branch is covered as tests/test_grasp_refine_fingers.py covers
    it, and compose is given the same forced rows: with candidates the new full stack (the reverted rows then go through the gradient
    refinement and every figure), without them the articulated push-out alone (the scores shown are the guard's merged ones)."""
    options = ctx.stack(False, "curl") if candidates else dict(num_grasp=M, rotate=False, refine_steps=STEPS, **KINDS["curl"])
    free = ctx.expected(options)
    exp = ctx.expected(options, forced=FORCED)
    for i, (e, u) in enumerate(zip(exp, free)):
        rev, before = e["stage"]["push"]["reverted"], u["stage"]["push"]["reverted"]
        print(f"object {i}: reverted unforced {before.tolist()} forced {rev.tolist()} iterate unforced {u['stage']['push']['iter'].tolist()}")
        assert rev[FORCED[i]].all() and np.array_equal(np.delete(rev, FORCED[i]), np.delete(before, FORCED[i]))
        assert (u["stage"]["push"]["iter"][FORCED[i]] > 0).all(), "a forced row had not moved: reverting it shows nothing"
        assert np.array_equal(e["stage"]["pushed_params"][FORCED[i]], e["stage"]["params0"][FORCED[i]])
    sizes = [o.shape[1] for o in ctx.objects(False)]
    text0 = None
    for rows_per_call in GROUPINGS:
        queue = [[k * M + c for k, pos in enumerate(call) for c in FORCED[pos]] for call in generate.plan_calls(sizes, M, rows_per_call)]
        force_worse(monkeypatch, queue)
        got = ctx.run(options, rows_per_call)
        monkeypatch.undo()
        assert not queue, "the guard scored fewer calls than the plan has"
        for i, (g, e) in enumerate(zip(got, exp)):
            gref.assert_result(g, e, f"forced, rows_per_call {rows_per_call} object {i}")
        text = [json.dumps(g["json"]) for g in got]
        text0 = text0 or text
        assert text == text0
    kept = [int(np.isin(e["candidate"], FORCED[i]).sum()) if candidates else len(FORCED[i]) for i, e in enumerate(exp)]
    print(f"candidates {candidates}: reverted rows among those written, per object: {kept}")
    assert sum(kept) >= 1, "no reverted row is written: the revert is composed but never compared"


BEAM = {False: (1, 8), True: (2, 4)}                   # (poses, width): W = 4 x P = 2 rotated; one pose of all M rows without rotation


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [False, True])
def test_beam_rows_carry_their_pose_and_its_rotation(ctx, rotate):
    """Independently of compose: row p * W + r of a beam run has the rotation the plain call draws for row p -- not the one it draws
    for row p * W + r -- and beam_pose = p, beam_rank = r."""
    P, W = BEAM[rotate]
    t = np.asarray(generate.CANONICAL_OFFSET if rotate else (0.0, 0.0, 0.0))
    for i, g in enumerate(ctx.plain(rotate, M, False, BEAM[rotate])):
        R = gref.rotation_of(seed_of(rotate), INDICES[i], P) if rotate else np.tile(np.eye(3), (P, 1, 1))
        j = g["json"]
        assert len(j["R_list"]) == P * W == M
        for p in range(P):
            for r in range(W):
                assert np.array_equal(np.asarray(j["R_list"][p * W + r]), np.concatenate([R[p], t.reshape(3, 1)], axis=1)), (i, p, r)
        if rotate:
            assert not np.array_equal(R[0], R[1]) and not np.array_equal(R[1], gref.rotation_of(seed_of(rotate), INDICES[i], M)[W])
        assert j["beam_pose"] == [p for p in range(P) for _ in range(W)] == g["beam_pose"].tolist()
        assert j["beam_rank"] == list(range(W)) * P == g["beam_rank"].tolist()
        assert all(-1 <= d < r for d, r in zip(j["beam_duplicate_of"], j["beam_rank"])) and "log_prob" in j


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [False, True])
@pytest.mark.parametrize("candidates", [0, M])
def test_beam_search_with_every_figure(ctx, candidates, rotate):
    P, W = BEAM[rotate]
    options = dict(num_grasp=KEEP if candidates else M, rotate=rotate, candidates=candidates, beam_width=W, beam_poses=P, stability=True, volume=True,
                   volume_res=RES, diversity=CLUSTERS, parts=True, self_collision=True, mesh_depth=True, object_meshes=ctx.meshes(rotate),
                   **FIGURE_SETTINGS[rotate])
    if candidates:
        options.update(select_by="stability", diverse_pool=POOL)
    got, exp = check_case(ctx, options, GROUPINGS, what=f"beam candidates {candidates} rotate {rotate}")
    for g, e in zip(got, exp):
        c = e["candidate"] if candidates else np.arange(M)
        assert list(g)[-3:] == BEAM_FIELDS and list(g["json"])[-3:] == BEAM_FIELDS and "log_prob" in g["json"]
        if not candidates:
            assert list(g) == documented_keys({**gref.OFF, **options}) and list(g["json"]) == documented_fields({**gref.OFF, **options})
        assert g["json"]["beam_pose"] == (c // W).tolist() and g["json"]["beam_rank"] == (c % W).tolist()
        assert [row[0][:3] for row in np.asarray(g["json"]["R_list"]).tolist()] == [row[0][:3] for row in np.asarray(e["json"]["R_list"]).tolist()]
    fingers = [(e["stage_figures"]["parts"]["part_count"][:, :5] >= 1).sum(axis=1).tolist() for e in exp]
    inside = [e["stage_figures"]["mesh"]["n_inside"].tolist() for e in exp]
    print(f"beam candidates {candidates} rotate {rotate}: fingers in contact {fingers} vertices inside the mesh {inside} "
          f"kept {[e['candidate'].tolist() for e in exp] if candidates else None}")
    assert all(max(x) > 0 for x in inside) and any(max(x) > 0 for x in fingers), "the beams' hands miss their objects"
    if candidates and rotate:
        assert any(len(set((e["candidate"] // W).tolist())) == P for e in exp), "every object's kept rows come from one pose"


@pytest.mark.gpu
def test_every_option_off_is_the_plain_call(ctx):
    plain = ctx.plain(False, G, False)
    got = ctx.run(dict(gref.OFF, num_grasp=G))
    for g, p in zip(got, plain):
        assert list(g) == list(p) == ["params", "vertices", "json"] and torch.equal(g["params"], p["params"]) and torch.equal(g["vertices"], p["vertices"])
        assert json.dumps(g["json"]) == json.dumps(p["json"])


# ------------------------------------------------------------------------------------------------------ GPU: the entry points
def _run_main(dataset, out_dir, extra, mano):
    seed = seed_of(generate.DATASETS[dataset]["rotate"])
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", str(seed), "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", ["ho3d", "obman"])
def test_entry_point_with_beam_search(dataset, tmp_path):
    """The entry points with --beam_width on (W = 4 x P = 2 for the rotated dataset, one pose of 8 beams for the other), best-of-M over
    the beams and every figure: the files equal ``json.dumps`` of the API's result, do not depend on --rows_per_call, and carry the
    beams' fields of the kept rows last.  Beam search draws nothing and excludes nothing but --temperature / --top_k, yet it replaces
    the candidates themselves, so it has a run of its own beside test_entry_point_with_every_flag."""
    from test_grasp_select import mano_pkl
    mano = mano_pkl(tmp_path)
    rotate = generate.DATASETS[dataset]["rotate"]
    seed, (P, W) = seed_of(rotate), BEAM[rotate]
    clouds = gref.rotated_contact_objects(SEED, INDICES, M)[0] if rotate else gref.hand_clouds()
    meshes = [gref.rotated_boxes(SEED, i, M, h) if rotate else gref.box(h) for i, h in zip(INDICES, BOX_HALVES[rotate])]
    files, mesh_files = [], []
    for i, (c, (v, f)) in enumerate(zip(clouds, meshes)):
        files.append(str(tmp_path / f"cloud{i}.npy"))
        np.save(files[-1], c)
        mesh_files.append(str(tmp_path / f"mesh{i}.npz"))
        np.savez(mesh_files[-1], verts=v, faces=f)
    settings = FIGURE_SETTINGS[rotate]
    flags = (["--objects"] + files + ["--num_grasp", str(KEEP), "--candidates", str(M), "--beam_width", str(W), "--beam_poses", str(P), "--select_by",
                                      "stability", "--diverse_pool", str(POOL), "--stability", "1", "--volume", "1", "--volume_res", str(RES),
                                      "--diversity", str(CLUSTERS), "--parts", "1", "--part_threshold", repr(settings["part_threshold"]),
                                      "--self_collision", "1", "--self_reach", repr(settings["self_reach"]), "--self_margin",
                                      repr(settings["self_margin"]), "--self_seam", str(settings["self_seam"]), "--object_meshes"]
             + mesh_files + ["--mesh_depth", "1"])
    args = generate.parse_args(dataset, flags + ["--checkpoint", "/nonexistent", "--mano_model", mano, "--seed", str(seed)])
    net = generate.load_model(args, torch.device(DEV))
    objs = [generate.object_tensor(np.load(p).astype(np.float64)) for p in files]
    api = generate.generate_for_objects(net, objs, KEEP, rotate, seed, INDICES, candidates=M, beam_width=W, beam_poses=P, select_by="stability",
                                        diverse_pool=POOL, stability=True, volume=True, volume_res=RES, diversity=CLUSTERS, parts=True,
                                        self_collision=True, mesh_depth=True, object_meshes=meshes, **settings)
    names0, bytes0 = _run_main(dataset, str(tmp_path / "r16384"), flags + ["--rows_per_call", "16384"], mano)
    assert names0 == [f"obj_id_cloud{i}.json" for i in range(3)]
    for tag in ("8", "0"):
        names, data = _run_main(dataset, str(tmp_path / f"r{tag}"), flags + ["--rows_per_call", tag], mano)
        assert names == names0 and data == bytes0, f"--rows_per_call {tag}: the files differ"
    poses = set()
    for i, (data, a) in enumerate(zip(bytes0, api)):
        assert data.decode() == json.dumps(a["json"]) and b"NaN" not in data
        j = json.loads(data)
        assert list(j) == ["recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact", "log_prob",
                           *gref.STABILITY_FIELDS, "rank", "novelty", "diversity", *gref.VOLUME_FIELDS, *gref.PARTS_FIELDS, *gref.SELF_FIELDS,
                           *gref.MESH_FIELDS, *BEAM_FIELDS]
        cand = np.asarray(j["candidate"])
        assert j["beam_pose"] == (cand // W).tolist() and j["beam_rank"] == (cand % W).tolist() and j["mesh_closed"] is True
        R = gref.rotation_of(seed, INDICES[i], P) if rotate else np.tile(np.eye(3), (P, 1, 1))
        assert all(np.array_equal(np.asarray(row)[:, :3], R[p]) for row, p in zip(j["R_list"], j["beam_pose"])), "a kept row's rotation is not its pose's"
        poses |= set(j["beam_pose"])
        print(f"{dataset} object {i}: kept {j['candidate']} fingers {j['fingers_in_contact']} inside {j['mesh_interior']}")
    assert poses == set(range(P)), "the kept rows come from one pose only"
    assert any(n > 0 for a in api for n in a["json"]["mesh_interior"]), "no kept beam has a vertex inside its mesh"


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", ["ho3d", "obman"])
def test_entry_point_with_every_flag(dataset, tmp_path):
    import scipy.spatial  # noqa: F401  the hulls need it: a missing scipy is an error here, not a skip
    from test_grasp_select import mano_pkl
    mano = mano_pkl(tmp_path)
    rotate = generate.DATASETS[dataset]["rotate"]
    seed = seed_of(rotate)
    clouds = gref.rotated_contact_objects(SEED, INDICES, M)[0] if rotate else gref.hand_clouds()
    files = []
    for i, c in enumerate(clouds):
        files.append(str(tmp_path / f"cloud{i}.npy"))
        np.save(files[-1], c)
    meshes = [gref.rotated_boxes(SEED, i, M, h) if rotate else gref.box(h) for i, h in zip(INDICES, BOX_HALVES[rotate])]
    mesh_files = []
    for i, (v, f) in enumerate(meshes):
        mesh_files.append(str(tmp_path / f"mesh{i}.npz"))
        np.savez(mesh_files[-1], verts=v, faces=f)
    base = ["--objects"] + files + ["--num_grasp", str(KEEP)]
    # the net of the entry point (synthetic weights of its own) and the objects as it reads them
    args = generate.parse_args(dataset, base + ["--checkpoint", "/nonexistent", "--mano_model", mano, "--seed", str(seed)])
    net = generate.load_model(args, torch.device(DEV))
    objs = [generate.object_tensor(np.load(p).astype(np.float64)) for p in files]
    stack = dict(candidates=M, select_by="stability", min_contact=1, diverse_pool=POOL, diverse_space="params", refine_steps=STEPS,
                 diversity=CLUSTERS, stability=True, torque_length=0.1, volume=True, volume_res=RES, log_prob=True,
                 # the newer options; beam search replaces the candidates themselves: test_entry_point_with_beam_search
                 ttt_steps=TTT, parts=True, self_collision=True, mesh_depth=True, object_meshes=meshes, **FIGURE_SETTINGS[rotate], **KINDS["curl"])
    unguarded = generate.generate_for_objects(net, objs, KEEP, rotate, seed, INDICES, **stack)
    pen, cnt = unguarded[0]["scores"]["penetration"].cpu(), np.sort(unguarded[0]["volume_scores"]["count"].cpu().numpy())
    max_pen = float(pen.median())                                                            # as test_grasp_wrench.py takes it
    limit = int(cnt[M // 2 - 1])
    X = (limit + 0.5) * RES ** 3 * 1e6                                                       # as test_grasp_volume.py takes it
    assert contact.volume_limit(X, RES) == limit and 0 < int((pen > max_pen).sum()) < M and 0 < int((cnt > limit).sum()) < M
    for i, g in enumerate(unguarded):
        assert_contact({k: v.cpu().numpy() for k, v in g["scores"].items()}, f"{dataset} object {i}")
    # the three newer guards: from the unguarded stack at ENTRY_RANKS of object 0's candidates, as Ctx.guard_limits takes them
    rank, u0 = ENTRY_RANKS[rotate], unguarded[0]
    fingers0 = np.sort((u0["part_scores"]["part_count"].cpu().numpy()[:, :5] >= 1).sum(axis=1))
    newer = dict(min_fingers=int(fingers0[rank["fingers"]]), need_thumb=rank["need_thumb"],
                 max_self_verts=int(np.sort(u0["self_scores"]["pen_count"].cpu().numpy().sum(axis=1))[rank["self"]]),
                 max_mesh_depth=float(np.sort(u0["mesh_scores"]["depth"].cpu().numpy())[rank["mesh"]]) * 100.0)
    assert newer["min_fingers"] >= 1, "min_fingers = 0 is the guard switched off"
    api = generate.generate_for_objects(net, objs, KEEP, rotate, seed, INDICES, max_penetration=max_pen, max_volume=X, **newer, **stack)
    no_pen = generate.generate_for_objects(net, objs, KEEP, rotate, seed, INDICES, max_volume=X, **newer, **stack)
    assert any(json.dumps(a["json"]) != json.dumps(b["json"]) for a, b in zip(api, no_pen)), "max_penetration changes no file"
    assert any(json.dumps(a["json"]) != json.dumps(b["json"]) for a, b in zip(api, unguarded)), "the two limits change no file"
    # the other conditions on the inputs, for THIS net: the entry point's synthetic weights are not those of the tests above
    count0 = api[0]["volume_scores"]["count"].cpu().numpy()
    over, deep = count0 > limit, (pen > max_pen).numpy()
    print(f"{dataset} object 0: voxel counts {count0.tolist()} over {over.astype(int).tolist()} deep {deep.astype(int).tolist()}")
    assert len(set(count0.tolist())) >= 3 and (count0 >= 0).all()
    assert (over & ~deep).any() and (deep & ~over).any(), "each guard must demote a candidate the other leaves alone"
    iters = [x for a in api for x in a["json"]["refine_iter"]]
    kept = [a["candidate"].cpu().numpy() for a in api]
    best = []
    for a in api:
        cls, key = contact.select_keys({k: v.cpu() for k, v in a["scores"].items()}, "stability", 1, max_penetration=max_pen)
        figs = {name: {k: v.cpu().numpy() for k, v in a[key].items()}
                for name, key in (("volume", "volume_scores"), ("parts", "part_scores"), ("self", "self_scores"), ("mesh", "mesh_scores"))}
        guards = gref.guard_classes({**gref.OFF, **stack, **newer, "max_volume": X}, figs)
        assert list(guards) == ["volume", "parts", "self", "mesh"]
        cls = np.maximum.reduce([cls.numpy()] + list(guards.values()))
        best.append(sref.segment_topk(cls, key.numpy(), 1, M, KEEP)[0])
    print(f"{dataset}: refine_iter of the kept rows {iters}, kept {[k.tolist() for k in kept]} best-ranked {[x.tolist() for x in best]}")
    assert any(x > 0 for x in iters), "no kept row was pushed"
    assert any((k >= KEEP).any() for k in kept), f"only the first {KEEP} candidates were kept"
    assert any(sorted(k.tolist()) != sorted(x.tolist()) for k, x in zip(kept, best)), "the picks are the best-ranked for every object"
    assert all(int(a[v]["status"].abs().max()) == 0 for a in api for v in ("volume", "volume_scores")), "a volume status is not 0"
    flags = base + ["--candidates", str(M), "--select_by", "stability", "--min_contact", "1", "--diverse_pool", str(POOL), "--diverse_space",
                    "params", "--refine_steps", str(STEPS), "--diversity", str(CLUSTERS), "--stability", "1", "--max_penetration",
                    repr(max_pen), "--torque_length", "0.1", "--volume", "1", "--volume_res", str(RES), "--max_volume", repr(X),
                    "--log_prob", "1", "--refine_spin", "1.0", "--refine_curl", "1.0", "--ttt_steps", str(TTT), "--parts", "1", "--part_threshold",
                    repr(stack["part_threshold"]), "--min_fingers", str(newer["min_fingers"]), "--need_thumb", str(int(newer["need_thumb"])), "--self_collision", "1",
                    "--self_reach", repr(stack["self_reach"]), "--self_margin", repr(stack["self_margin"]), "--self_seam", str(stack["self_seam"]),
                    "--max_self_verts", str(newer["max_self_verts"]), "--object_meshes"] + mesh_files + [
                    "--mesh_depth", "1", "--max_mesh_depth", repr(newer["max_mesh_depth"])]
    summaries = ("diversity.json", "penetration.json", "hand_contact.json", "self_collision.json", "mesh_penetration.json", "refine_curl.json")
    names0, bytes0 = _run_main(dataset, str(tmp_path / "r16384"), flags + ["--rows_per_call", "16384"], mano)
    assert names0 == [f"obj_id_cloud{i}.json" for i in range(3)]
    extras0 = [open(tmp_path / "r16384" / f, "rb").read() for f in summaries]
    for tag in ("8", "0"):
        names, data = _run_main(dataset, str(tmp_path / f"r{tag}"), flags + ["--rows_per_call", tag], mano)
        assert names == names0 and data == bytes0, f"--rows_per_call {tag}: the files differ"
        assert [open(tmp_path / f"r{tag}" / f, "rb").read() for f in summaries] == extras0
    kept, rows = [], []
    for data, a in zip(bytes0, api):
        assert data.decode() == json.dumps(a["json"]) and b"NaN" not in data
        j = json.loads(data)
        assert list(j) == stack_fields("curl") and j["mesh_closed"] is True
        kept.append(np.asarray(j["recon_params"], dtype=F32).reshape(KEEP, 61))
        rows += list(zip(j["volume_voxels"], j["penetration_volume"], j["penetration_depth"]))
    # diversity.json: test_segment_kmeans.py's rule; penetration.json: test_grasp_volume.py's
    assert json.loads(extras0[0]) == {**gref.diversity_entry(np.concatenate(kept), CLUSTERS), "grasps": 3 * KEEP}
    stat = json.loads(extras0[1])
    assert set(stat) == {"res", "grasps", "mean_volume_cm3", "mean_depth_cm", "contact_ratio"} and stat["res"] == RES
    assert stat["grasps"] == len(rows) == 3 * KEEP and all(r[0] is not None for r in rows)
    assert math.isclose(stat["mean_volume_cm3"], sum(r[1] for r in rows) / len(rows), rel_tol=1e-12)
    assert math.isclose(stat["mean_depth_cm"], sum(r[2] for r in rows) / len(rows), rel_tol=1e-12)
    assert stat["contact_ratio"] == sum(1 for r in rows if r[0] >= 1) / len(rows)
    # every flag at its documented "off" value: the bytes of a run without the flags, and neither extra file
    off = ["--candidates", "0", "--select_by", "penetration", "--diverse_pool", "0", "--refine_steps", "0", "--diversity", "0", "--stability", "0",
           "--max_penetration", "inf", "--volume", "0", "--max_volume", "inf", "--log_prob", "0", "--refine_spin", "0", "--refine_curl", "0",
           "--ttt_steps", "0", "--parts", "0", "--min_fingers", "0", "--need_thumb", "0", "--self_collision", "0", "--mesh_depth", "0",
           "--max_mesh_depth", "inf", "--beam_width", "0", "--beam_poses", "1", "--object_meshes"] + mesh_files
    names_p, plain = _run_main(dataset, str(tmp_path / "plain"), base, mano)
    names_o, offed = _run_main(dataset, str(tmp_path / "off"), base + off, mano)
    assert names_p == names_o == names0 and offed == plain
    assert all(list(json.loads(d)) == ["recon_params", "R_list", "trans_list", "r_list"] for d in plain)
    for tag in ("plain", "off"):
        assert not any(os.path.exists(tmp_path / tag / f) for f in summaries)
