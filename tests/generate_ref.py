"""The pipeline of generate.generate_for_objects restated from the stage references -- test infrastructure.  ``compose`` takes the
tensors of a PLAIN run (no option on) and returns what the call must return with the options on, built from tests/grasp_refine_ref,
grasp_score_ref, grasp_wrench_ref, grasp_volume_ref, diverse_select_ref and segment_kmeans_ref, numpy, and the float64 host formulas
of the package (contact.select_keys, hull_planes, volume_limit, wrench_stats, volume_stats, diversity.kmeans_init).  It calls none of
contact.grasp_scores, refine_translation, grasp_stability, grasp_volume, ops.segment_topk, segment_diverse, segment_kmeans.

The order is the one generate_for_objects' docstring promises:

    1 row clouds = R | t applied to the object (the ``transform`` given; ops.transform_cloud by default)
    2 push-out of ALL rows (grasp_refine_ref), params[:, 58:61] + offset in fp32
    3 MANO again (the ``pose`` given)
    4 scores or wrench sums of the re-posed hands             5 volume of the re-posed hands, hull of the UNROTATED cloud, the rows' R | t
    6 classes and keys (contact.select_keys on CPU tensors; the volume rule written out below)
    7 top-k, or the pool and its farthest-point picks          8 k-means of the kept parameters          9 the JSON, keys in order

The JSON's field order, as generate.py builds it.  With candidates: recon_params, R_list, trans_list, r_list, candidate, penetration,
n_interior, n_contact, [log_prob], [force_residual, torque_residual, min_sv, stability_key], [rank, novelty], [refine_offset,
refine_iter], [diversity], [penetration_volume, penetration_depth, volume_voxels].  Without: recon_params, R_list, trans_list, r_list,
[log_prob], [refine_offset, refine_iter], [penetration, n_interior, n_contact] (with refine or stability), [the four stability
fields], [the three volume fields], [diversity]."""
import json

import numpy as np
import torch

from dvqvae_amd import contact, diversity, generate, synth

import diverse_select_ref as dref
import grasp_refine_ref as rref
import grasp_score_ref as sref
import grasp_volume_ref as vref
import grasp_wrench_ref as wref
import segment_kmeans_ref as kref

F32 = np.float32
INF = float("inf")

OFF = dict(num_grasp=None, rotate=False, log_prob=False, candidates=0, select_by="penetration", min_contact=1, diverse_pool=0,
           diverse_space="params", refine_steps=0, refine_push=1.0, refine_pull=0.25, diversity=0, stability=False, max_penetration=INF,
           torque_length=0.1, volume=False, volume_res=0.001, max_volume=INF)
"""Every option of generate_for_objects at its documented "off" value; ``num_grasp`` (the rows kept per object) has none."""

STABILITY_FIELDS = ("force_residual", "torque_residual", "min_sv", "stability_key")
VOLUME_FIELDS = ("penetration_volume", "penetration_depth", "volume_voxels")
VOLUME_PIECES = ("count", "depth", "status")


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


def stages(plain, obj4n, faces, sealed_topology, pose, transform, options, cache=None, cache_key=None):
    """Steps 1 - 5 for ALL rows of one object: what they give depends on the refinement's and the two kernels' own arguments only, so
    ``cache`` (a dict) with ``cache_key`` (naming the object and its plain run) shares them between the option sets of a test."""
    o = options
    key = (cache_key, o["rotate"], o["refine_steps"], o["refine_push"], o["refine_pull"], o["min_contact"] if o["refine_steps"] else None)
    store = cache.setdefault(key, {}) if cache is not None and cache_key is not None else {}
    Rt = np.asarray(plain["json"]["R_list"], np.float64)                               # [M,3,4]: rotation | translation
    R, t = Rt[:, :, :3].astype(F32), Rt[0, :, 3].astype(F32)
    if "base" not in store:
        params = plain["params"].detach().cpu().numpy().astype(F32)
        verts = plain["vertices"].detach().cpu().numpy().astype(F32)
        obj = np.ascontiguousarray(transform(obj4n, R, t), F32)                         # [M,N,3]
        base = {"obj": obj, "offset": None, "iter": None}
        if o["refine_steps"]:
            off, it, _, _, _ = rref.grasp_refine(verts, faces, obj, o["refine_steps"], o["refine_push"], o["refine_pull"], o["min_contact"])
            params = params.copy()
            params[:, 58:61] = (params[:, 58:61] + off).astype(F32)
            verts = np.ascontiguousarray(pose(params), F32)
            base.update(offset=off, iter=it)
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
    elif want_scores:
        if "scores" not in store:
            store["scores"] = dict(zip(("penetration", "n_interior", "n_contact"), sref.grasp_scores(base["verts"], faces, base["obj"])))
        scores = dict(store["scores"])
    vol = None
    if o["volume"] or float(o["max_volume"]) < INF:
        k = ("volume", float(o["volume_res"]))
        if k not in store:
            sealed, loop_off, loop_vert = sealed_topology
            planes = contact.hull_planes(obj4n[:3].T.cpu().numpy().astype(np.float64))  # of the object's own UNROTATED cloud
            M = base["verts"].shape[0]
            store[k] = vref.grasp_volume(base["verts"], sealed, loop_off, loop_vert, planes, [0, len(planes)], np.zeros(M, np.int64),
                                         R=R if o["rotate"] else None, t=t if o["rotate"] else None, h=float(o["volume_res"]))
        vol = store[k]
    return base, scores, vol


def volume_class(count, max_volume, res):
    """The rule of the docstring, written out: 2 without a figure, else 1 above floor(X / (res^3 * 1e6)) voxels, else 0."""
    limit = contact.volume_limit(max_volume, res)
    return np.asarray([2 if int(c) < 0 else int(int(c) > limit) for c in count], np.int32)


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


def compose_one(plain, obj4n, faces, sealed_topology, pose, transform, options, cache=None, cache_key=None):
    o = {**OFF, **options}
    M = plain["params"].shape[0]
    cand_mode = bool(o["candidates"])
    assert (o["candidates"] or o["num_grasp"]) == M, "the plain run must hold the rows of the call: candidates, or num_grasp without"
    keep = int(o["num_grasp"])
    base, scores, vol = stages(plain, obj4n, faces, sealed_topology, pose, transform, o, cache, cache_key)
    want_stability = bool(o["stability"]) or (cand_mode and o["select_by"] == "stability")
    with_logp = bool(o["log_prob"]) or (cand_mode and o["select_by"] == "log_prob")
    logp = plain["log_prob"].detach().cpu().numpy().astype(F32) if with_logp else None
    pj = plain["json"]
    exp = {}
    if cand_mode:
        scores_all = dict(scores)
        if logp is not None:
            scores_all["log_prob"] = logp
        as_t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in scores_all.items()}
        cls, key = contact.select_keys(as_t, o["select_by"], o["min_contact"], log_prob=as_t.get("log_prob"),
                                       max_penetration=o["max_penetration"])
        cls, key = cls.numpy().astype(np.int32), key.numpy().astype(F32)
        if vol is not None and float(o["max_volume"]) < INF:
            cls = np.maximum(cls, volume_class(vol["count"], o["max_volume"], o["volume_res"]))
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
    volj = volume_json(vol["count"][sel], vol["depth"][sel], o["volume_res"]) if vol is not None else {}
    if cand_mode:
        j["candidate"] = sel.tolist()
        for k in ("penetration", "n_interior", "n_contact") + (("log_prob",) if with_logp else ()):
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
        if o["refine_steps"]:
            exp["refine_offset"], exp["refine_iter"] = base["offset"][sel], base["iter"][sel]
            j.update(refine_offset=exp["refine_offset"].tolist(), refine_iter=exp["refine_iter"].tolist())
            keys += ["refine_offset", "refine_iter"]
        if div is not None:
            exp["diversity"] = j["diversity"] = div
            keys.append("diversity")
        if vol is not None:
            exp["volume"] = {k: vol[k][sel] for k in VOLUME_PIECES}
            exp["volume_scores"] = {k: vol[k] for k in VOLUME_PIECES}
            j.update(volj)
            keys += ["volume", "volume_scores"]
        exp["candidate"], exp["scores"] = sel.astype(np.int64), scores_all
        keys += ["params", "vertices", "candidate", "scores", "json"]
    else:
        if with_logp:
            exp["log_prob"] = logp
            j["log_prob"] = logp.tolist()
            keys.append("log_prob")
        if o["refine_steps"]:
            exp["refine_offset"], exp["refine_iter"] = base["offset"], base["iter"]
            j.update(refine_offset=base["offset"].tolist(), refine_iter=base["iter"].tolist())
            keys += ["refine_offset", "refine_iter"]
        if scores is not None:
            for k in ("penetration", "n_interior", "n_contact"):
                exp[k] = scores[k]
                j[k] = scores[k].tolist()
                keys.append(k)
        if want_stability:
            exp["wrench_sums"], exp["stability_key"] = scores["sums"], scores["key"]
            j.update(stab)
            keys += ["wrench_sums", "stability_key"]
        if vol is not None:
            exp["volume"] = {k: vol[k] for k in VOLUME_PIECES}
            j.update(volj)
            keys.append("volume")
        if div is not None:
            exp["diversity"] = j["diversity"] = div
            keys.append("diversity")
        keys += ["params", "vertices", "json"]
    exp.update(params=kept_p, vertices=kept_v, json=j, keys=keys, stage=base, stage_scores=scores, stage_volume=vol)
    return exp


def compose(plain, clouds, faces, sealed_topology, pose, options, transform=None, cache=None, cache_keys=None):
    """What ``generate_for_objects(net, clouds, options["num_grasp"], options["rotate"], ...)`` must return with ``options`` on (the
    keys of OFF; missing ones are off), one dict per object.

    ``plain``: per object, the dict of a plain run of M rows (M = candidates, or num_grasp without candidates) with the same seed,
    object_indices, rotate, temperature, top_k and log_prob: ``params`` [M,61], ``vertices`` [M,V,3], ``log_prob`` [M] where the options
    read it, and ``json`` with its ``R_list`` / ``r_list`` / ``trans_list``.  ``clouds``: the [4,N] object tensors.  ``faces`` [F,3];
    ``sealed_topology`` = (sealed faces, loop_off, loop_vert) of contact.seal_faces, as numpy; ``pose``: fp32 params [B,61] -> fp32
    vertices [B,V,3] (the net's MANO layer, which has its own float64 tests).  ``transform``: step 1 (default: ops.transform_cloud on
    the device of the plain tensors).  ``cache`` / ``cache_keys`` (one hashable per object): share steps 1 - 5 between calls.

    Each dict holds, as numpy arrays: ``params``, ``vertices``, ``candidate``, ``rank`` / ``novelty``, ``refine_offset`` / ``refine_iter``,
    ``scores`` (all candidates), ``wrench_sums`` / ``stability_key``, ``volume`` / ``volume_scores``, ``log_prob``, (without candidates)
    ``penetration`` / ``n_interior`` / ``n_contact``; the ``diversity`` dict; ``json`` with its keys in order; ``keys``: the returned
    dict's own keys in order; and for the tests' direct assertions ``cls`` / ``key`` / ``pool`` / ``best`` (the ``num_grasp`` best-ranked)
    and ``stage`` / ``stage_scores`` / ``stage_volume`` (steps 1 - 5 of ALL rows)."""
    if transform is None:
        transform = device_transform(plain[0]["params"].device)
    return [compose_one(p, c, faces, sealed_topology, pose, transform, options, cache, None if cache_keys is None else cache_keys[i])
            for i, (p, c) in enumerate(zip(plain, clouds))]


# ------------------------------------------------------------------------------------------------------ comparisons
def same_bits(got, want, what):
    """fp32: bit for bit, a NaN is a NaN (the rule of every stage test); integers: equal."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if want.dtype.kind == "f":
        assert got.dtype == np.float32, (what, got.dtype)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, got, want)
        assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), (what, got, want)
    else:
        assert got.dtype.kind in "iu" and np.array_equal(got, want), (what, got, want)


def assert_result(got, want, what=""):
    """One object's dict of generate_for_objects against compose's: the dict's keys in order, tensors bit for bit, the diversity dict
    and the JSON by ``==`` with its keys in order.  ``json.dumps`` of both must agree as well: a float32 value and its Python float
    have the same repr exactly when their bits agree, so this is the bit comparison of the float32 fields (and tells -0.0 from +0.0)."""
    assert list(got) == want["keys"], (what, list(got), want["keys"])
    for k in want["keys"]:
        if k == "json":
            assert list(got["json"]) == list(want["json"]), (what, list(got["json"]), list(want["json"]))
            for f in want["json"]:
                assert got["json"][f] == want["json"][f], (what, f, got["json"][f], want["json"][f])
            assert json.dumps(got["json"]) == json.dumps(want["json"]), what
        elif k == "diversity":
            assert got[k] == want[k] and list(got[k]) == list(want[k]), (what, got[k], want[k])
        elif k in ("scores", "volume", "volume_scores"):
            assert set(got[k]) == set(want[k]), (what, k, set(got[k]), set(want[k]))
            for name in want[k]:
                same_bits(got[k][name], want[k][name], f"{what} {k}[{name}]")
        else:
            same_bits(got[k], want[k], f"{what} {k}")


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
