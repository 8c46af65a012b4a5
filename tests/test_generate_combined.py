"""generate.generate_for_objects with its options TOGETHER, rotated too: best-of-M, the diverse pool, the push-out, the k-means
statistic, the wrench proxy and the voxel volume in one call, on both paths (_select_call, and _generate_call without candidates), and
the entry points with every flag.  The reference is tests/generate_ref.py::compose -- the pipeline restated from the stage references
-- fed the tensors of a plain run; every comparison is the one the stage's own test uses (tensors bit for bit, JSON by ``==``)."""
import itertools
import json
import math
import os

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import contact, generate

import generate_ref as gref
import grasp_score_ref as sref
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
        self.cache, self._plain, self._objs, self._limits = {}, {}, {}, {}

    def pose_t(self, p):
        return self.net.rh_mano(betas=p[:, :10], global_orient=p[:, 10:13], hand_pose=p[:, 13:58], transl=p[:, 58:61]).vertices

    def pose(self, params):
        return self.pose_t(torch.from_numpy(np.ascontiguousarray(params, F32)).to(DEV)).cpu().numpy()

    def objects(self, rotate):
        """Three objects of two point counts that meet the hands of a run of at most M rows per object.  Rotated: always the objects of
        M blocks -- a run of fewer rows draws the first rotations of the M, its rows are rows of the M-row run, and the place the net
        puts a hand depends on the whole cloud it sees."""
        if rotate not in self._objs:
            clouds = gref.rotated_contact_objects(SEED, INDICES, M)[0] if rotate else gref.hand_clouds()
            assert len({c.shape[0] for c in clouds[:2]}) == 2
            self._objs[rotate] = [generate.object_tensor(c) for c in clouds]
        return self._objs[rotate]

    def plain(self, rotate, rows, log_prob):
        if (rotate, rows, log_prob) not in self._plain:
            self._plain[rotate, rows, log_prob] = generate.generate_for_objects(self.net, self.objects(rotate), rows, rotate,
                                                                                seed_of(rotate), INDICES, log_prob=log_prob)
        return self._plain[rotate, rows, log_prob]

    def expected(self, options, n_obj=3):
        o = {**gref.OFF, **options}
        rows = o["candidates"] or o["num_grasp"]
        with_lp = bool(o["log_prob"]) or (bool(o["candidates"]) and o["select_by"] == "log_prob")
        return gref.compose(self.plain(o["rotate"], rows, with_lp)[:n_obj], self.objects(o["rotate"])[:n_obj], self.faces, self.sealed,
                            self.pose, o, cache=self.cache, cache_keys=[(o["rotate"], rows, i) for i in range(n_obj)])

    def run(self, options, rows_per_call=16384, n_obj=3):
        o = {**gref.OFF, **options}
        rows = o["candidates"] or o["num_grasp"]
        return generate.generate_for_objects(self.net, self.objects(o["rotate"])[:n_obj], o["num_grasp"], o["rotate"],
                                             seed_of(o["rotate"]), INDICES[:n_obj], rows_per_call=rows_per_call, **gref.api_keywords(options))

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
def documented_fields(o):
    """The JSON's fields without candidates, in the order generate.py documents."""
    stab, refine = o["stability"], bool(o["refine_steps"])
    return (["recon_params", "R_list", "trans_list", "r_list"] + (["log_prob"] if o["log_prob"] else [])
            + (["refine_offset", "refine_iter"] if refine else []) + (["penetration", "n_interior", "n_contact"] if refine or stab else [])
            + (list(gref.STABILITY_FIELDS) if stab else []) + (list(gref.VOLUME_FIELDS) if o["volume"] else [])
            + (["diversity"] if o["diversity"] else []))


def documented_keys(o):
    stab, refine = o["stability"], bool(o["refine_steps"])
    return ((["log_prob"] if o["log_prob"] else []) + (["refine_offset", "refine_iter"] if refine else [])
            + (["penetration", "n_interior", "n_contact"] if refine or stab else []) + (["wrench_sums", "stability_key"] if stab else [])
            + (["volume"] if o["volume"] else []) + (["diversity"] if o["diversity"] else []) + ["params", "vertices", "json"])


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


# ------------------------------------------------------------------------------------------------------ GPU: the entry points
def _run_main(dataset, out_dir, extra, mano):
    seed = seed_of(generate.DATASETS[dataset]["rotate"])
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", str(seed), "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


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
    base = ["--objects"] + files + ["--num_grasp", str(KEEP)]
    # the net of the entry point (synthetic weights of its own) and the objects as it reads them
    args = generate.parse_args(dataset, base + ["--checkpoint", "/nonexistent", "--mano_model", mano, "--seed", str(seed)])
    net = generate.load_model(args, torch.device(DEV))
    objs = [generate.object_tensor(np.load(p).astype(np.float64)) for p in files]
    stack = dict(candidates=M, select_by="stability", min_contact=1, diverse_pool=POOL, diverse_space="params", refine_steps=STEPS,
                 diversity=CLUSTERS, stability=True, torque_length=0.1, volume=True, volume_res=RES, log_prob=True)
    unguarded = generate.generate_for_objects(net, objs, KEEP, rotate, seed, INDICES, **stack)
    pen, cnt = unguarded[0]["scores"]["penetration"].cpu(), np.sort(unguarded[0]["volume_scores"]["count"].cpu().numpy())
    max_pen = float(pen.median())                                                            # as test_grasp_wrench.py takes it
    limit = int(cnt[M // 2 - 1])
    X = (limit + 0.5) * RES ** 3 * 1e6                                                       # as test_grasp_volume.py takes it
    assert contact.volume_limit(X, RES) == limit and 0 < int((pen > max_pen).sum()) < M and 0 < int((cnt > limit).sum()) < M
    for i, g in enumerate(unguarded):
        assert_contact({k: v.cpu().numpy() for k, v in g["scores"].items()}, f"{dataset} object {i}")
    api = generate.generate_for_objects(net, objs, KEEP, rotate, seed, INDICES, max_penetration=max_pen, max_volume=X, **stack)
    no_pen = generate.generate_for_objects(net, objs, KEEP, rotate, seed, INDICES, max_volume=X, **stack)
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
        cls = np.maximum(cls.numpy(), gref.volume_class(a["volume_scores"]["count"].cpu().numpy(), X, RES))
        best.append(sref.segment_topk(cls, key.numpy(), 1, M, KEEP)[0])
    print(f"{dataset}: refine_iter of the kept rows {iters}, kept {[k.tolist() for k in kept]} best-ranked {[x.tolist() for x in best]}")
    assert any(x > 0 for x in iters), "no kept row was pushed"
    assert any((k >= KEEP).any() for k in kept), f"only the first {KEEP} candidates were kept"
    assert any(sorted(k.tolist()) != sorted(x.tolist()) for k, x in zip(kept, best)), "the picks are the best-ranked for every object"
    assert all(int(a[v]["status"].abs().max()) == 0 for a in api for v in ("volume", "volume_scores")), "a volume status is not 0"
    flags = base + ["--candidates", str(M), "--select_by", "stability", "--min_contact", "1", "--diverse_pool", str(POOL), "--diverse_space",
                    "params", "--refine_steps", str(STEPS), "--diversity", str(CLUSTERS), "--stability", "1", "--max_penetration",
                    repr(max_pen), "--torque_length", "0.1", "--volume", "1", "--volume_res", str(RES), "--max_volume", repr(X),
                    "--log_prob", "1"]
    names0, bytes0 = _run_main(dataset, str(tmp_path / "r16384"), flags + ["--rows_per_call", "16384"], mano)
    assert names0 == [f"obj_id_cloud{i}.json" for i in range(3)]
    extras0 = [open(tmp_path / "r16384" / f, "rb").read() for f in ("diversity.json", "penetration.json")]
    for tag in ("8", "0"):
        names, data = _run_main(dataset, str(tmp_path / f"r{tag}"), flags + ["--rows_per_call", tag], mano)
        assert names == names0 and data == bytes0, f"--rows_per_call {tag}: the files differ"
        assert [open(tmp_path / f"r{tag}" / f, "rb").read() for f in ("diversity.json", "penetration.json")] == extras0
    kept, rows = [], []
    for data, a in zip(bytes0, api):
        assert data.decode() == json.dumps(a["json"]) and b"NaN" not in data
        j = json.loads(data)
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
           "--max_penetration", "inf", "--volume", "0", "--max_volume", "inf", "--log_prob", "0"]
    names_p, plain = _run_main(dataset, str(tmp_path / "plain"), base, mano)
    names_o, offed = _run_main(dataset, str(tmp_path / "off"), base + off, mano)
    assert names_p == names_o == names0 and offed == plain
    assert all(list(json.loads(d)) == ["recon_params", "R_list", "trans_list", "r_list"] for d in plain)
    for tag in ("plain", "off"):
        assert not os.path.exists(tmp_path / tag / "diversity.json") and not os.path.exists(tmp_path / tag / "penetration.json")
