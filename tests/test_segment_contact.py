"""Object-side contact map: the fused per-object kernel (dvq_segment_contact), its host API (ops.segment_contact,
contact.object_contact, contact.object_contact_stats, contact.pseudo_cmap) and the ``--object_contact`` mode of the entry points.  The
reference is tests/segment_contact_ref.py (numpy over tests/grasp_score_ref.py's per-point bits, rules 1-5 of the header stated
literally); GPU results are compared with it bit for bit, every output, no row or point exempted; a NaN is a NaN."""
import functools
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops

import grasp_score_ref as score_ref
import segment_contact_ref as ref

DEV = "cuda:0"
F32 = np.float32
T = ops.SEGMENT_CONTACT_TILE
THR = 2.0 ** -12                        # (2^-6 m)^2 = (1.5625 cm)^2: a threshold a planted point can sit at exactly
OUTPUTS = ("touch", "inside", "dmin", "near_sum", "n_valid", "row_status")
FIELDS = ("object_contact_map", "object_interior_map", "object_min_dist", "object_contact")
DATASETS = ["obman", "ho3d", "grab", "FHAB"]


# ------------------------------------------------------------------------------------------------------ the cases
@functools.lru_cache(maxsize=None)
def case(O, K, N, V, plant=True):
    """hand [O*K,V,3], faces, obj [O*K,N,3] (row o*K+i: object o as its grasp i sees it -- the same points for every grasp of an object,
    the hand scaled and shifted per row), and the indices planted in object 0: hands on a 5 cm sphere, the clouds in a shell of 3 .. 9 cm
    about it, so that some points are inside the hands, some within the threshold and some beyond.  With ``plant`` (hands of >= 776
    vertices) point 0 of object 0 sits exactly at the threshold distance from the nearest vertex of row 0 -- it must not count there --
    and the points at the tile seam (T - 1, T) and the last point sit ON vertices of row 0: the last of the scan's blocks of four, the
    first of its tail and the last vertex.  Built once per shape and left unchanged."""
    v, f = ref.meshes(V)
    rng = np.random.default_rng([77, O, K, N, V])
    B = O * K
    hand = (v[None].astype(np.float64) * rng.uniform(0.9, 1.1, (B, 1, 1)) + rng.uniform(-0.01, 0.01, (B, 1, 3))).astype(F32)
    dirs = rng.normal(size=(O, N, 3))
    dirs /= np.linalg.norm(dirs, axis=2, keepdims=True)
    obj = np.repeat((dirs * rng.uniform(0.03, 0.09, (O, N, 1))).astype(F32), K, axis=0)
    planted = {}
    if plant and V >= 776:
        j = int(hand[0, :, 0].argmax())                                 # the outermost vertex along x: nothing else is nearer beyond it
        hand[0, j] = np.round(hand[0, j].astype(np.float64) * 4096.0) / 4096.0
        obj[:K, 0] = hand[0, j] + np.asarray([2.0 ** -6, 0.0, 0.0], F32)  # exact: multiples of 2^-12 below 1
        planted["threshold"] = 0
        V4 = V & ~3
        for p, u in zip((T - 1, T, N - 1), (V4 - 1, min(V4, V - 1), V - 1)):
            if 0 < p < N and p not in planted.values():
                obj[:K, p] = hand[0, u]
                planted[f"vertex {u}"] = p
    for a in (hand, obj):
        a.setflags(write=False)
    return hand, f, obj, planted


@functools.lru_cache(maxsize=None)
def want_of(O, K, N, V, thr=THR):
    hand, f, obj, _ = case(O, K, N, V)
    return ref.segment_contact(hand, f, obj, O, K, None, thr)


def topology(f, V):
    return contact.HandTopology(f, V, DEV)


def gpu(hand, f, obj, O, K, rows=None, thr=THR, err=None):
    hand_t, obj_t = torch.from_numpy(np.ascontiguousarray(hand)).to(DEV), torch.from_numpy(np.ascontiguousarray(obj)).to(DEV)
    rows_t = None if rows is None else torch.as_tensor(np.asarray(rows, np.int64).reshape(-1), device=DEV)
    out = contact.object_contact(topology(f, hand.shape[1]), hand_t, obj_t, O, K, rows_t, thr, err=err)
    assert tuple(out) == OUTPUTS
    return {k: x.cpu().numpy() for k, x in out.items()}


def assert_same_bits(got, want, what=""):
    for name in OUTPUTS:
        g, w = got[name], np.asarray(want[name])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float32:
            nan_g, nan_w = np.isnan(g), np.isnan(w)
            same = (nan_g & nan_w) | (~nan_g & ~nan_w & (g.view(np.uint32) == w.view(np.uint32)))
        else:
            same = g == w
        assert same.all(), f"{what}: {name} differs at {np.argwhere(~same)[:5].tolist()}: got {g[~same][:5]}, want {w[~same][:5]}"


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", DATASETS)
def test_parser_has_the_object_contact_flags(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.object_contact, a.object_contact_threshold) == (0, 0.02)
    a = generate.parse_args(dataset, ["--object_contact", "1", "--object_contact_threshold", "0.005"])
    assert (a.object_contact, a.object_contact_threshold) == (1, 0.005)
    for bad in (["--object_contact", "2"], ["--object_contact_threshold", "0"], ["--object_contact_threshold", "-0.01"],
                ["--object_contact_threshold", "inf"], ["--object_contact_threshold", "nan"]):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.dvq_abi_version() == 10
    assert "dvq_segment_contact" in _lib.SIGNATURES and "int dvq_segment_contact(" in header and hasattr(lib, "dvq_segment_contact")
    assert "dvq_segment_contact" in re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert len(_lib.SIGNATURES["dvq_segment_contact"][1]) == 23
    assert ops.SEGMENT_CONTACT_TILE == 1024
    src = open(os.path.join(_lib.CSRC, "segment_contact.hip")).read()
    assert "__syncthreads" not in src and "dvq_lds_barrier();" in src          # every barrier through the checked helper


def test_ops_refuse_bad_arguments_before_any_device_use():
    v, f = ref.meshes(5)
    faces, off, vf = (torch.from_numpy(a) for a in contact.face_csr(f, len(v)))
    hand = torch.from_numpy(v)[None].repeat(4, 1, 1).contiguous()
    obj = torch.zeros(4, 7, 3)
    rows = torch.arange(4)
    call = lambda *a, **k: ops.segment_contact(hand, faces, off, vf, obj, *a, **k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # a good call gets as far as the device check, no further
        call(2, 2, rows)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(2, 2)
    bad = [((2, 0), {}), ((4, 0), {}), ((2, 2, torch.arange(3)), {}), ((2, 2, torch.arange(5)), {}), ((2, 2, rows.to(torch.int32)), {}),
           ((2, 2, rows.view(2, 2)), {}), ((2, 2, [0, 1, 2, 3]), {}), ((3, 2), {}), ((2, 1), {}), ((-1, 2, torch.arange(0)), {}),
           ((2, 2), {"contact_threshold": 0.0}), ((2, 2), {"contact_threshold": -1.0}), ((2, 2), {"contact_threshold": math.inf}),
           ((2, 2), {"contact_threshold": math.nan}), ((2, 2), {"err": torch.zeros(1)}), ((2, 2), {"err": torch.zeros(2, dtype=torch.int32)}),
           ((1, ops.SEGMENT_CONTACT_MAX_K + 1, torch.zeros(ops.SEGMENT_CONTACT_MAX_K + 1, dtype=torch.int64)), {})]
    for args, kw in bad:
        with pytest.raises(RuntimeError, match="segment_contact") as e:
            call(*args, **kw)
        assert "no CPU fallback" not in str(e.value), (args, kw)
    big = torch.zeros(4, 2049, 3)                                           # V > 2048
    with pytest.raises(RuntimeError, match=r"segment_contact: need N >= 1 and 1 <= V <= 2048"):
        ops.segment_contact(big, faces, torch.zeros(2050, dtype=torch.int32), vf, obj, 2, 2)
    with pytest.raises(RuntimeError, match="segment_contact"):             # N = 0
        ops.segment_contact(hand, faces, off, vf, torch.zeros(4, 0, 3), 2, 2)
    with pytest.raises(RuntimeError, match="segment_contact"):             # the CSR of another mesh
        ops.segment_contact(hand, faces, off[:-1], vf, obj, 2, 2)


def test_restatement_agrees_with_the_per_grasp_scores():
    """Per object the column sums of touch / inside are the sums of grasp_score_ref.grasp_scores' n_contact / n_interior over the
    segment's rows, at the planted threshold and at the scores' own."""
    O, K, N, V = 2, 5, 40, 776
    hand, f, obj, _ = case(O, K, N, V)
    for thr in (THR, 0.02 ** 2):
        want = ref.segment_contact(hand, f, obj, O, K, None, thr)
        _, n_in, n_ct = score_ref.grasp_scores(hand, f, obj, thr)
        assert want["err"] == 0 and want["n_valid"].tolist() == [K] * O and not want["row_status"].any()
        assert want["touch"].sum(1).tolist() == n_ct.reshape(O, K).sum(1).tolist() and want["touch"].any()
        assert want["inside"].sum(1).tolist() == n_in.reshape(O, K).sum(1).tolist() and want["inside"].any()
    rows = [9, 8, 7, 6, 5, 0, 0, 3, 3, 1]                               # given rows: a reversed segment, rows that repeat
    want = ref.segment_contact(hand, f, obj, O, K, rows, THR)
    _, n_in, n_ct = score_ref.grasp_scores(hand[rows], f, obj[rows], THR)
    assert want["touch"].sum(1).tolist() == n_ct.reshape(O, K).sum(1).tolist()
    assert want["inside"].sum(1).tolist() == n_in.reshape(O, K).sum(1).tolist()


def test_restatement_agrees_with_a_float64_brute_force():
    O, K, N, V = 2, 5, 60, 776
    hand, f, obj, planted = case(O, K, N, V, plant=False)
    assert not planted
    want = ref.segment_contact(hand, f, obj, O, K, None, THR)
    touch, inside, dmin, rel_gap, dot_margin, tie_gap = ref.brute_force(hand, f, obj, O, K, THR)
    # the test's own inputs: no distance within a relative 1e-5 of the threshold, no interior test or nearest-vertex tie on the edge
    assert rel_gap > 1e-5 and dot_margin > 1e-7 and tie_gap > 1e-5, (rel_gap, dot_margin, tie_gap)
    assert np.array_equal(want["touch"], touch) and np.array_equal(want["inside"], inside) and touch.any() and inside.any()
    assert np.allclose(want["dmin"].astype(np.float64), dmin, rtol=1e-6, atol=0.0)
    assert want["n_valid"].tolist() == [K] * O


def test_restatement_rules_on_a_hand_made_segment():
    """Chains, validity and refusal on numbers small enough to check by hand: one vertex at the origin, three points on the x axis."""
    hand = np.zeros((6, 1, 3), F32)
    obj = np.zeros((6, 3, 3), F32)
    obj[:, :, 0] = np.asarray([0.25, 0.5, 2.0], F32)                    # d = 1/16, 1/4, 4 for every row
    hand[2, 0, 1] = np.nan                                              # position 2 is invalid: its chain (g = 2) stays +0.0
    f = np.asarray([[0, 0, 0]])
    out = ref.segment_contact(hand, f, obj, 1, 6, None, 1.0)
    assert out["n_valid"].tolist() == [5] and out["row_status"].tolist() == [0, 0, 1, 0, 0, 0]
    assert out["touch"].tolist() == [[5, 5, 0]] and out["inside"].tolist() == [[0, 0, 0]]
    assert out["dmin"].tolist() == [[0.0625, 0.25, 4.0]] and out["near_sum"].tolist() == [[1.25, 2.5, 0.0]]
    out = ref.segment_contact(hand, f, obj, 2, 3, [0, 1, 6, 3, 4, 5], 1.0)
    assert out["err"] == 1 and out["n_valid"].tolist() == [-1, 3] and out["row_status"].tolist() == [-1, -1, -1, 0, 0, 0]
    assert out["touch"].tolist() == [[-1, -1, -1], [3, 3, 0]] and np.isnan(out["dmin"][0]).all() and np.isnan(out["near_sum"][0]).all()


def test_object_contact_stats_and_pseudo_cmap():
    rng = np.random.default_rng(5)
    touch = rng.integers(0, 4, (4, 9)).astype(np.int32)
    touch[1] = 0                                                        # nothing touched: no entropy
    n_valid = np.asarray([3, 3, 0, 2], np.int32)
    touch[2] = 0
    dmin = rng.uniform(0.0, 0.01, (4, 9)).astype(F32)
    dmin[2] = np.inf
    near_sum = (touch * rng.uniform(0.001, 0.02, (4, 9))).astype(F32)
    got = contact.object_contact_stats(torch.from_numpy(touch), np.zeros_like(touch), dmin, near_sum, n_valid)
    want = ref.object_contact_stats(touch, dmin, near_sum, n_valid)
    assert len(got) == 4 and all(set(g) == {"grasps", "coverage", "entropy", "min_dist", "contact_dist"} for g in got)
    for g, w in zip(got, want):
        assert g["grasps"] == w["grasps"] and g["coverage"] == w["coverage"] and g["contact_dist"] == w["contact_dist"]
        assert (g["entropy"] is None) == (w["entropy"] is None) and (g["entropy"] is None or abs(g["entropy"] - w["entropy"]) < 1e-12)
        assert g["min_dist"] == w["min_dist"]
    assert got[1]["entropy"] is None and got[2]["min_dist"] == [None] * 9 and got[2]["grasps"] == 0 and got[0]["entropy"] > 0
    one = contact.object_contact_stats([[2, 2, 0, 0]], [[0] * 4], [[0.0001] * 4], [[0.02, 0.03, 0, 0]], [2])[0]
    assert one["coverage"] == 0.5 and abs(one["entropy"] - math.log(2)) < 1e-15 and one["contact_dist"] == [1.0, 1.5, None, None]
    assert one["min_dist"] == [100.0 * math.sqrt(0.0001)] * 4
    with pytest.raises(RuntimeError):
        contact.object_contact_stats(touch, touch, dmin, near_sum, n_valid[:3])
    with pytest.raises(RuntimeError):
        contact.object_contact_stats([[-1]], [[-1]], [[math.nan]], [[math.nan]], [-1])
    d2 = np.asarray([0.0, 0.0001, 0.0009, 1.0, np.inf])                 # 0, 1, 3, 100 cm, nothing
    cm = contact.pseudo_cmap(torch.from_numpy(d2))
    sig = lambda x: 1.0 / (1.0 + math.exp(-x))
    assert cm.dtype == np.float64 and cm[0] == 1.0 and cm[4] == 0.0
    assert all(abs(cm[i] - (1.0 - 2.0 * (sig(2.0 * 100.0 * math.sqrt(d2[i])) - 0.5))) < 1e-15 for i in range(4))
    assert 0.0 < cm[2] < cm[1] < 1.0 and cm[3] < 1e-80


# ------------------------------------------------------------------------------------------------------ GPU: the kernel
SHAPES = [(1, 1, 1, 1), (1, 2, 5, 5), (3, 3, T - 1, 776), (2, 4, T, 778), (2, 5, T + 1, 778), (1, 9, 2 * T + 1, 778)]


@pytest.mark.gpu
@pytest.mark.parametrize("O,K,N,V", SHAPES)
def test_kernel_matches_the_restatement(O, K, N, V):
    hand, f, obj, planted = case(O, K, N, V)
    want = want_of(O, K, N, V)
    if V >= 776:                                                        # the planting took: the case exercises what it is meant to
        d0, _, _ = score_ref.point_terms(hand[:1], f, obj[:1])
        assert d0[0, planted["threshold"]] == F32(THR), "the planted point is not exactly at the threshold"
        assert want["touch"].any() and want["inside"].any() and (want["touch"] < K).any(), "the hands are not near the clouds"
        on = [p for name, p in planted.items() if name != "threshold"]
        assert on and all(want["dmin"][0, p] == 0.0 and want["touch"][0, p] >= 1 for p in on)
        if N > T:
            assert T - 1 in on and T in on
    got = gpu(hand, f, obj, O, K)
    assert_same_bits(got, want, f"{O}x{K}x{N}x{V}")
    assert want["err"] == 0 and got["n_valid"].tolist() == [K] * O


@pytest.mark.gpu
def test_planted_threshold_point_does_not_count():
    """Row 0 alone as a segment: the point exactly at the threshold distance has touch 0 and adds nothing; just above it would."""
    O, K, N, V = 2, 4, T, 778
    hand, f, obj, planted = case(O, K, N, V)
    got = gpu(hand, f, obj, 1, 1, rows=[0])
    p = planted["threshold"]
    assert got["dmin"][0, p] == F32(THR) and got["touch"][0, p] == 0 and got["near_sum"][0, p] == 0.0
    above = gpu(hand, f, obj, 1, 1, rows=[0], thr=float(np.nextafter(F32(THR), F32(1.0))))
    assert above["touch"][0, p] == 1 and above["near_sum"][0, p] == F32(2.0 ** -6)


@pytest.mark.gpu
def test_rows_given_and_identity():
    O, K, N, V = 3, 3, T - 1, 776
    hand, f, obj, _ = case(O, K, N, V)
    same = gpu(hand, f, obj, O, K, rows=np.arange(O * K))               # rows=None against the identity list: the same bits
    assert_same_bits(same, want_of(O, K, N, V), "identity")
    assert_same_bits(same, gpu(hand, f, obj, O, K), "rows=None")
    # a permutation; a row in two objects (and twice in one); object 0's segment in reversed order
    rows = [4, 8, 0, 0, 5, 5, 0, 8, 4]
    want = ref.segment_contact(hand, f, obj, O, K, rows, THR)
    got = gpu(hand, f, obj, O, K, rows=rows)
    assert_same_bits(got, want, "rows")
    assert np.array_equal(got["touch"][0], got["touch"][2]) and np.array_equal(got["dmin"][0], got["dmin"][2])   # the same rows: order only moves the chains
    perm = np.random.default_rng(3).permutation(O * K)
    assert_same_bits(gpu(hand, f, obj, O, K, rows=perm), ref.segment_contact(hand, f, obj, O, K, perm, THR), "permutation")
    # four objects of two rows out of the nine, K = 2: O * K != B
    rows = [1, 2, 3, 4, 8, 7, 6, 5]
    assert_same_bits(gpu(hand, f, obj, 4, 2, rows=rows), ref.segment_contact(hand, f, obj, 4, 2, rows, THR), "O*K != B")


@pytest.mark.gpu
def test_reversed_segment_moves_the_chains():
    """Five touching rows of one point with distances whose four-chain fp32 sum depends on the order (3.0 forwards, the next float
    after it backwards): the kernel follows the segment order."""
    v, f = ref.meshes(1)
    hand = np.zeros((5, 1, 3), F32)
    obj = np.zeros((5, 2, 3), F32)
    obj[:, 0, 0] = np.asarray([1.0, 1.0, 1.0, 3 * 2.0 ** -25, 3 * 2.0 ** -25], F32)   # the distances: their squares and roots are exact
    obj[:, 1, 0] = 0.5
    fwd, rev = [0, 1, 2, 3, 4], [4, 3, 2, 1, 0]
    wf, wr = ref.segment_contact(hand, f, obj, 1, 5, fwd, 16.0), ref.segment_contact(hand, f, obj, 1, 5, rev, 16.0)
    assert wf["near_sum"][0, 0] != wr["near_sum"][0, 0], "the case does not tell the orders apart"
    assert_same_bits(gpu(hand, f, obj, 1, 5, rows=fwd, thr=16.0), wf, "forward")
    assert_same_bits(gpu(hand, f, obj, 1, 5, rows=rev, thr=16.0), wr, "reversed")


@pytest.mark.gpu
def test_bad_index_refuses_that_object_only():
    O, K, N, V = 3, 3, T - 1, 776
    hand, f, obj, _ = case(O, K, N, V)
    clean = want_of(O, K, N, V)
    for bad_value in (-1, O * K, 2 ** 40):
        rows = np.arange(O * K)
        rows[4] = bad_value                                             # in object 1
        err = ops.new_err_flag(torch.device(DEV))
        got = gpu(hand, f, obj, O, K, rows=rows, err=err)
        assert int(err.item()) == 1
        want = ref.segment_contact(hand, f, obj, O, K, rows, THR)
        assert want["err"] == 1 and (want["touch"][1] == -1).all() and np.isnan(want["dmin"][1]).all()
        assert_same_bits(got, want, f"bad index {bad_value}")
        for name in OUTPUTS[:4]:                                        # the other objects: the bits of the clean call
            assert np.array_equal(got[name][[0, 2]], clean[name][[0, 2]]), name
        assert got["n_valid"].tolist() == [K, -1, K] and got["row_status"].tolist() == [0] * 3 + [-1] * 3 + [0] * 3
    with pytest.raises(RuntimeError, match="out of bounds"):            # without a flag of the caller's the wrapper raises
        gpu(hand, f, obj, O, K, rows=rows)
    err = ops.new_err_flag(torch.device(DEV))                           # a clean call leaves the flag alone
    gpu(hand, f, obj, O, K, rows=np.arange(O * K), err=err)
    assert int(err.item()) == 0


@pytest.mark.gpu
def test_rows_that_are_not_finite_take_part_in_nothing():
    O, K, N, V = 2, 5, T + 1, 778
    hand0, f, obj0, _ = case(O, K, N, V)
    hand, obj = hand0.copy(), obj0.copy()
    hand[0, 777, 2] = np.nan                                            # a hand
    hand[1, 3, 0] = np.inf
    obj[2, 17, 1] = np.nan                                              # a cloud, inside tile 0 (outside the tile tile 1 reduces)
    obj[3, T, 0] = -np.inf                                              # a cloud, in tile 1 (outside the tile tile 0 reduces)
    for r in range(K, 2 * K):                                           # object 1: every row invalid, one way or another
        (hand if r % 2 else obj)[r, r, r % 3] = np.nan if r % 3 else np.inf
    want = ref.segment_contact(hand, f, obj, O, K, None, THR)
    assert want["row_status"].tolist() == [1, 1, 1, 1, 0] + [1] * K and want["n_valid"].tolist() == [1, 0]
    assert np.isinf(want["dmin"][1]).all() and not want["touch"][1].any() and not want["near_sum"][1].any()
    got = gpu(hand, f, obj, O, K)
    assert_same_bits(got, want, "non-finite rows")
    alone = gpu(hand0, f, obj0, 1, 1, rows=[4])                         # object 0 is its one valid row
    for name in OUTPUTS[:4]:
        assert np.array_equal(got[name][0], alone[name][0]), name


@pytest.mark.gpu
def test_channel_first_cloud_is_read_in_place():
    O, K, N, V = 2, 5, T + 1, 778
    hand, f, obj, _ = case(O, K, N, V)
    cloud = np.concatenate([obj.transpose(0, 2, 1), np.full((O * K, 1, N), 7.0, F32)], axis=1)       # [B,4,N]
    cloud_t = torch.from_numpy(cloud).to(DEV)
    view = cloud_t[:, :3].transpose(1, 2)
    assert not view.is_contiguous() and view.data_ptr() == cloud_t.data_ptr()
    out = contact.object_contact(topology(f, V), torch.from_numpy(hand).to(DEV), view, O, K, None, THR)
    assert_same_bits({k: x.cpu().numpy() for k, x in out.items()}, want_of(O, K, N, V), "channel-first")


@pytest.mark.gpu
def test_an_objects_map_does_not_depend_on_the_call():
    O, K, N, V = 3, 3, T - 1, 776
    hand, f, obj, _ = case(O, K, N, V)
    full = gpu(hand, f, obj, O, K)
    for o in range(O):                                                  # alone
        alone = gpu(hand[o * K:(o + 1) * K], f, obj[o * K:(o + 1) * K], 1, K)
        for name in OUTPUTS[:5]:
            assert np.array_equal(alone[name][0], full[name][o]), (o, name)
        assert np.array_equal(alone["row_status"], full["row_status"][o * K:(o + 1) * K])
    # its rows moved elsewhere in a larger B, among other rows, another object first in the call
    where = [11, 2, 7]
    big_h, big_o = np.repeat(hand[:1], 13, 0).copy(), np.repeat(obj[:1], 13, 0).copy()
    big_h[where], big_o[where] = hand[K:2 * K], obj[K:2 * K]
    moved = gpu(big_h, f, big_o, 2, K, rows=[0, 1, 3] + where)
    for name in OUTPUTS[:5]:
        assert np.array_equal(moved[name][1], full[name][1]), name


@pytest.mark.gpu
def test_cross_checks_against_the_shipped_kernels():
    """On the device, exact, at the scores' threshold: the column sums against ops.grasp_scores, the minimum against ops.nn_points."""
    O, K, N, V = 2, 5, T + 1, 778
    hand, f, obj, _ = case(O, K, N, V)
    topo = topology(f, V)
    hand_t, obj_t = torch.from_numpy(hand).to(DEV), torch.from_numpy(obj).to(DEV)
    out = contact.object_contact(topo, hand_t, obj_t, O, K)             # the default threshold: the scores'
    scores = contact.grasp_scores(topo, hand_t, obj_t)
    assert torch.equal(out["touch"].sum(1), scores["n_contact"].view(O, K).sum(1)) and int(out["touch"].sum()) > 0
    assert torch.equal(out["inside"].sum(1), scores["n_interior"].view(O, K).sum(1)) and int(out["inside"].sum()) > 0
    dist, _ = ops.nn_points(obj_t, hand_t)
    assert torch.equal(out["dmin"], dist.view(O, K, N).min(1).values)
    assert out["n_valid"].tolist() == [K] * O and not out["row_status"].any()
    assert_same_bits({k: x.cpu().numpy() for k, x in out.items()}, want_of(O, K, N, V, 0.02 ** 2), "default threshold")


@pytest.mark.gpu
def test_c_abi_refuses_sizes_out_of_range():
    v, f = ref.meshes(5)
    topo = topology(f, 5)
    lib = _lib.load()
    one = torch.full((64,), 7.0, device=DEV)
    p, q = one.data_ptr(), topo.faces.data_ptr()
    call = lambda V=5, B=4, N=4, rows=None, O=2, K=2, thr=0.0004, touch=p, err=p: lib.dvq_segment_contact(
        p, q, topo.vf_off.data_ptr(), topo.vf_face.data_ptr(), V, p, 12, 3, 1, B, N, rows, O, K, thr, touch, p, p, p, p, p, err, None)
    for kw in (dict(K=0), dict(K=ops.SEGMENT_CONTACT_MAX_K + 1), dict(V=2049), dict(V=0), dict(N=0), dict(O=-1), dict(thr=0.0),
               dict(thr=-1.0), dict(thr=math.inf), dict(thr=math.nan), dict(B=5), dict(touch=None), dict(err=None)):
        assert call(**kw) == 1, kw
    assert (one == 7.0).all()                                           # nothing was written
    assert lib.dvq_segment_contact(None, None, None, None, 5, None, 0, 0, 0, 0, 4, None, 0, 2, 0.0004, None, None, None, None, None,
                                   None, None, None) == 0               # O == 0: DVQ_OK before any pointer is looked at
    empty = ops.segment_contact(torch.zeros(0, 5, 3, device=DEV), topo.faces, topo.vf_off, topo.vf_face, torch.zeros(0, 4, 3, device=DEV), 0, 2)
    assert [tuple(x.shape) for x in empty] == [(0, 4)] * 4 + [(0,), (0,)]


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


def _check_fields(j, N, k):
    assert [len(j[f]) for f in FIELDS[:3]] == [N] * 3
    assert all(type(x) is int and 0 <= x <= k for f in FIELDS[:2] for x in j[f])
    assert all(type(x) is float and x >= 0.0 for x in j["object_min_dist"])
    oc = j["object_contact"]
    assert list(oc) == ["grasps", "coverage", "entropy", "threshold"] and oc["grasps"] == k and oc["threshold"] == 0.02
    assert oc["coverage"] == sum(1 for x in j["object_contact_map"] if x >= 1) / N
    total = sum(j["object_contact_map"])
    if total:
        want = -math.fsum(x / total * math.log(x / total) for x in j["object_contact_map"] if x)
        assert abs(oc["entropy"] - want) < 1e-12
    else:
        assert oc["entropy"] is None
    assert sum(j["object_contact_map"]) == sum(j["n_contact"]) and sum(j["object_interior_map"]) == sum(j["n_interior"])


@pytest.mark.gpu
@pytest.mark.parametrize("candidates", [True, False])
def test_entry_point_writes_the_object_contact_fields(candidates, tmp_path):
    from test_grasp_select import mano_pkl
    from test_grasp_wrench import E2E_K as k, E2E_M
    mano = mano_pkl(tmp_path)
    files, clouds = _cloud_files(tmp_path)
    # without --candidates the three scores are written with --stability 1, which leaves the hands as they are
    base = ["--objects"] + files + (["--num_grasp", str(k), "--candidates", str(E2E_M)] if candidates else ["--num_grasp", str(k), "--stability", "1"])
    _, plain = _run_main("obman", str(tmp_path / "plain"), base, mano)
    names, data = _run_main("obman", str(tmp_path / "oc"), base + ["--object_contact", "1"], mano)
    assert names == [f"obj_id_cloud{i}.json" for i in range(4)]
    touched = 0
    for i, (d, p) in enumerate(zip(data, plain)):
        assert b"Infinity" not in d and b"NaN" not in d                # strict JSON
        j, jp = json.loads(d), json.loads(p)
        assert list(j) == list(jp) + list(FIELDS) and {f: j[f] for f in jp} == jp
        _check_fields(j, clouds[i].shape[0], k)
        touched += sum(j["object_contact_map"])
        if i == 3:                                                      # the far object: no hand touches it
            assert j["object_contact_map"] == [0] * 200 and j["object_interior_map"] == [0] * 200
            assert j["object_contact"]["entropy"] is None and j["object_contact"]["coverage"] == 0.0 and min(j["object_min_dist"]) > 50.0
        else:
            assert sum(j["object_contact_map"]) > 0 and j["object_contact"]["entropy"] > 0.0
    summary = open(str(tmp_path / "oc" / "object_contact.json"), "rb").read()
    assert b"Infinity" not in summary and b"NaN" not in summary
    s = json.loads(summary)
    per = [json.loads(d)["object_contact"] for d in data]
    assert s["objects"] == 4 and s["grasps"] == 4 * k and s["threshold"] == 0.02 and s["share_untouched"] == 0.25
    assert abs(s["mean_coverage"] - sum(x["coverage"] for x in per) / 4) < 1e-12
    assert abs(s["mean_entropy"] - sum(x["entropy"] for x in per[:3]) / 3) < 1e-12
    assert touched > 0


@pytest.mark.gpu
def test_entry_point_files_do_not_depend_on_the_grouping(tmp_path):
    from test_grasp_select import mano_pkl
    from test_grasp_wrench import E2E_K as k, E2E_M
    mano = mano_pkl(tmp_path)
    files, _ = _cloud_files(tmp_path)
    flags = ["--objects"] + files + ["--num_grasp", str(k), "--candidates", str(E2E_M), "--object_contact", "1"]
    names0, bytes0 = _run_main("obman", str(tmp_path / "g16384"), flags + ["--rows_per_call", "16384"], mano)
    summary0 = open(str(tmp_path / "g16384" / "object_contact.json"), "rb").read()
    for tag in ("8", "0"):
        names, data = _run_main("obman", str(tmp_path / f"g{tag}"), flags + ["--rows_per_call", tag], mano)
        assert names == names0 and data == bytes0, f"--rows_per_call {tag}: the files differ"
        assert open(str(tmp_path / f"g{tag}" / "object_contact.json"), "rb").read() == summary0


@pytest.mark.gpu
def test_entry_point_without_the_flag_writes_the_parents_bytes(tmp_path):
    from test_grasp_select import mano_pkl
    from test_grasp_wrench import E2E_K as k, E2E_M
    mano = mano_pkl(tmp_path)
    files, _ = _cloud_files(tmp_path)
    base = ["--objects"] + files + ["--num_grasp", str(k), "--candidates", str(E2E_M)]
    names0, plain = _run_main("obman", str(tmp_path / "plain"), base, mano)
    names, off = _run_main("obman", str(tmp_path / "off"), base + ["--object_contact", "0", "--object_contact_threshold", "0.01"], mano)
    assert names == names0 and off == plain and not os.path.exists(str(tmp_path / "off" / "object_contact.json"))
    assert not os.path.exists(str(tmp_path / "plain" / "object_contact.json"))
    assert all(set(json.loads(d)) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact"}
               for d in plain)


@pytest.mark.gpu
def test_ho3d_map_is_indexed_by_the_files_point_order(tmp_path):
    """gen_diverse_grasp_ho3d: every grasp sees the object under its own rotation.  The entry point runs with the flag; and for the
    grouped call behind it, the map of an object is contact.object_contact of the returned vertices against the clouds re-posed from the
    object's own [4,N] tensor, in its point order, with the rotations the JSON lists -- the same bits.  The hands of the synthetic
    weights stand about 0.8 m from a rotated cloud, so the threshold is 1 m here."""
    from test_grasp_select import _gennet, mano_pkl
    from test_grasp_wrench import E2E_INDICES, E2E_SEED, e2e_clouds
    mano = mano_pkl(tmp_path)
    files, clouds = _cloud_files(tmp_path)
    G, thr = 4, 1.0
    names, data = _run_main("ho3d", str(tmp_path / "ho3d"), ["--objects"] + files + ["--num_grasp", str(G), "--object_contact", "1",
                                                                                   "--object_contact_threshold", str(thr)], mano)
    assert len(data) == 4 and os.path.exists(str(tmp_path / "ho3d" / "object_contact.json"))
    for d, c in zip(data, clouds):
        j = json.loads(d)
        assert [len(j[f]) for f in FIELDS[:3]] == [c.shape[0]] * 3 and j["object_contact"]["threshold"] == thr
        assert len({tuple(map(tuple, R)) for R in j["R_list"]}) == G, "the rows carry different rotations"
    net = _gennet(tmp_path)
    objs = [generate.object_tensor(c) for c in e2e_clouds()]
    topo = generate._hand_topology(net, 778, torch.device(DEV))
    for kw in ({}, {"candidates": 2 * G}):
        got = generate.generate_with_object_contact(net, objs, G, True, E2E_SEED, E2E_INDICES, object_contact_threshold=thr, **kw)
        varied = False
        for g, obj in zip(got, objs):
            Rt = np.asarray(g["json"]["R_list"])                           # [G,3,4]
            R = torch.as_tensor(Rt[:, :, :3], dtype=torch.float32, device=DEV).contiguous()
            t = torch.as_tensor(Rt[0, :, 3], dtype=torch.float32, device=DEV).contiguous()
            posed = ops.transform_cloud(obj.to(DEV).contiguous(), R, t)     # [G,4,N], the file's point order
            want = contact.object_contact(topo, g["vertices"], posed[:, :3].transpose(1, 2), 1, G, None, thr ** 2)
            for name in OUTPUTS[:5]:
                assert torch.equal(g["object_contact"][name], want[name][0]), name
            assert torch.equal(g["object_contact"]["row_status"], want["row_status"])
            j = g["json"]
            assert j["object_contact_map"] == want["touch"][0].tolist() and j["object_interior_map"] == want["inside"][0].tolist()
            assert j["object_min_dist"] == [100.0 * math.sqrt(x) for x in want["dmin"][0].double().tolist()]
            assert j["object_contact"]["grasps"] == G
            varied |= len(set(j["object_min_dist"])) > 1
            print("touch", sum(j["object_contact_map"]), "of", G * len(j["object_contact_map"]), "nearest", min(j["object_min_dist"]), "cm")
        assert varied, "every point has the same distance: the point order is not exercised"
