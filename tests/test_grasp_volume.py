"""Penetration volume: the fused hull-intersection voxel kernel (dvq_grasp_volume), its host API (ops.grasp_volume, contact.seal_faces,
hull_planes, pack_planes, grasp_volume, volume_stats) and the ``--volume`` / ``--max_volume`` mode of the entry points.  The references
are in tests/grasp_volume_ref.py: (a) the header's definition in numpy fp32, which GPU results equal exactly, and (b) an independent
float64 brute force that (a) is checked against on the CPU."""
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops, synth

import grasp_score_ref as score_ref
import grasp_volume_ref as ref

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
RADIUS = 0.04
NO_LOOPS = (np.zeros(1, np.int32), np.zeros(0, np.int32))
OUTPUTS = ("count", "depth", "status")
FIELDS = ("penetration_volume", "penetration_depth", "volume_voxels")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sphere():
    v, f = score_ref.sphere_mesh(radius=RADIUS)
    return v, f


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_volume_flags(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.volume, a.volume_res) == (0, 0.001) and a.max_volume == INF
    a = generate.parse_args(dataset, ["--volume", "1", "--volume_res", "0.0025", "--max_volume", "1.5", "--candidates", "200",
                                      "--num_grasp", "100"])
    assert (a.volume, a.volume_res, a.max_volume) == (1, 0.0025, 1.5)
    assert generate.parse_args(dataset, ["--volume", "1"]).candidates == 0          # the figure alone needs no candidates
    for bad in (["--volume_res", "0"], ["--volume_res", "-0.001"], ["--volume_res", "inf"], ["--volume_res", "nan"],
                ["--max_volume", "-1", "--candidates", "200", "--num_grasp", "100"],
                ["--max_volume", "nan", "--candidates", "200", "--num_grasp", "100"], ["--max_volume", "2"]):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)
    with pytest.raises(SystemExit):                                                  # ranking by volume is not a --select_by choice
        generate.parse_args(dataset, ["--select_by", "volume"])
    assert contact.SELECT_BY == ("penetration", "log_prob", "stability")


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_grasp_volume" in _lib.SIGNATURES and "int dvq_grasp_volume(" in header and hasattr(lib, "dvq_grasp_volume")
    assert "dvq_grasp_volume" in re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    # hand V | faces F | loop_off loop_vert L n_loop | planes n_planes plane_off O | obj_of_row R t B h | count depth status err | stream
    assert len(_lib.SIGNATURES["dvq_grasp_volume"][1]) == 22
    declared = re.search(r"int dvq_grasp_volume\((.*?)\);", header, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", declared, flags=re.S).split(",")) == 22


def volume_args(B=1):
    v, f = sphere()
    hand = torch.from_numpy(v)[None].repeat(B, 1, 1).contiguous()
    return dict(hand=hand, faces=torch.from_numpy(f.astype(np.int32)), loop_off=torch.zeros(1, dtype=torch.int32),
                loop_vert=torch.zeros(0, dtype=torch.int32), planes=torch.from_numpy(ref.SPHERE_PLANES),
                plane_off=torch.tensor([0, 7], dtype=torch.int32), obj_of_row=torch.zeros(B, dtype=torch.int64))


def test_ops_refuse_bad_arguments_before_any_device_use():
    good = volume_args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_volume(**good)                                                     # well-formed, but not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_volume(**good, R=torch.eye(3)[None].contiguous(), t=torch.zeros(3), res=0.004)
    hand, faces = good["hand"], good["faces"]
    for bad in (dict(hand=torch.zeros(1, 2049, 3)), dict(hand=torch.zeros(1, 0, 3)), dict(hand=hand.transpose(1, 2)),  # V, layout
                dict(hand=hand.double()), dict(faces=faces.long()), dict(faces=faces.reshape(-1)),                     # dtype, shape
                dict(faces=torch.zeros(8193, 3, dtype=torch.int32)), dict(loop_off=torch.zeros(66, dtype=torch.int32)),
                dict(loop_off=torch.zeros(0, dtype=torch.int32)), dict(loop_vert=torch.zeros(3, dtype=torch.int64)),
                dict(planes=torch.zeros(7, 3)), dict(planes=torch.zeros(7, 4, dtype=torch.float64)),
                dict(plane_off=torch.zeros(2, dtype=torch.int64)), dict(plane_off=torch.zeros(0, dtype=torch.int32)),
                dict(obj_of_row=torch.zeros(1, dtype=torch.int32)), dict(obj_of_row=torch.zeros(2, dtype=torch.int64)),
                dict(R=torch.zeros(2, 3, 3)), dict(R=torch.zeros(1, 3, 3, dtype=torch.float64)), dict(t=torch.zeros(3)),   # t without R
                dict(R=torch.eye(3)[None].contiguous(), t=torch.zeros(4)),
                dict(res=0.0), dict(res=-0.001), dict(res=INF), dict(res=NAN)):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_volume(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"


# ------------------------------------------------------------------------------------------------------ CPU: the host helpers
def test_seal_faces_on_the_real_hand_and_on_closed_meshes(tmp_path):
    from test_grasp_select import mano_faces
    faces, _ = mano_faces(tmp_path)
    sealed, off, loop = contact.seal_faces(faces, 778)
    assert off.tolist() == [0, 16] and sealed.shape == (1538 + 16, 3) and sealed.dtype == off.dtype == loop.dtype == np.int32
    assert set(loop.tolist()) == {38, 78, 79, 92, 108, 117, 118, 119, 120, 121, 122, 214, 215, 234, 239, 279}
    assert np.array_equal(sealed[:1538], faces) and set(sealed[1538:, 2].tolist()) == {778}
    directed = sealed[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2)
    pairs = {(a, b) for a, b in directed.tolist()}
    assert len(pairs) == len(directed), "a directed edge is used twice"
    assert all((b, a) in pairs for a, b in pairs), "the sealed mesh is not closed"
    # the boundary is walked along the faces' own direction: consecutive loop vertices are a directed edge of the open mesh
    open_pairs = {(a, b) for a, b in np.asarray(faces)[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2).tolist()}
    assert all((a, b) in open_pairs for a, b in zip(loop.tolist(), loop.tolist()[1:] + loop.tolist()[:1]))
    v, f = score_ref.sphere_mesh()
    closed, off, loop = contact.seal_faces(f, len(v))
    assert off.tolist() == [0] and loop.size == 0 and np.array_equal(closed, f)
    # a sphere with two faces removed far apart: two loops of three, lowest vertex first; sealing restores a closed mesh
    holes, off, loop = contact.seal_faces(np.delete(f, [200, 900], axis=0), len(v))
    assert off.tolist() == [0, 3, 6] and holes.shape[0] == len(f) - 2 + 6 and set(holes[-6:, 2].tolist()) == {len(v), len(v) + 1}
    pairs = {(a, b) for a, b in holes[:, [0, 1, 1, 2, 2, 0]].reshape(-1, 2).tolist()}
    assert len(pairs) == 3 * len(holes) and all((b, a) in pairs for a, b in pairs)
    assert {frozenset(loop[:3].tolist()), frozenset(loop[3:].tolist())} == {frozenset(f[200].tolist()), frozenset(f[900].tolist())}
    with pytest.raises(RuntimeError):
        contact.seal_faces(np.concatenate([f, f[:1]]), len(v))                       # a directed edge twice
    with pytest.raises(RuntimeError):
        contact.seal_faces(np.concatenate([f, f[:1, ::-1]]), len(v))                 # an edge used three times
    with pytest.raises(RuntimeError):
        contact.seal_faces(f, 10)                                                    # an index past the vertices


def test_hull_planes_of_a_cube_and_the_packing():
    pytest.importorskip("scipy")
    corners = np.asarray([[x, y, z] for x in (-0.1, 0.2) for y in (0.0, 0.3) for z in (-0.05, 0.05)])
    inner = synth.synthetic_uniform((60, 3), 3, "volume/cube", 0.0, 1.0).numpy().astype(np.float64) * [0.3, 0.3, 0.1] + [-0.1, 0.0, -0.05]
    planes = contact.hull_planes(np.concatenate([corners, inner]))
    assert planes.shape == (6, 4) and planes.dtype == np.float32
    want = {(-1, 0, 0, 0.1), (1, 0, 0, 0.2), (0, -1, 0, 0.0), (0, 1, 0, 0.3), (0, 0, -1, 0.05), (0, 0, 1, 0.05)}
    assert {tuple(np.round(p.astype(np.float64), 6).tolist()) for p in planes} == {tuple(float(x) for x in w) for w in want}
    pts = np.concatenate([corners, inner])
    assert (pts @ planes[:, :3].T.astype(np.float64) <= planes[:, 3] + 1e-6).all()   # n.x <= d inside
    packed, off = contact.pack_planes([planes, planes[:2], np.zeros((0, 4))])
    assert packed.shape == (8, 4) and packed.dtype == np.float32 and off.tolist() == [0, 6, 8, 8] and off.dtype == np.int32
    assert contact.pack_planes([])[1].tolist() == [0]
    with pytest.raises(RuntimeError):
        contact.pack_planes([np.zeros((8193, 4))])
    with pytest.raises(RuntimeError):
        contact.hull_planes(np.zeros((3, 3)))


def test_volume_stats_and_the_integer_limit():
    got = contact.volume_stats(torch.tensor([0, 1939, -1, 15159], dtype=torch.int32), torch.tensor([0.0, 0.0062, NAN, 0.011]), 0.004)
    assert got["penetration_volume"] == [0.0, 1939 * (0.004 * 0.004 * 0.004 * 1e6), None, 15159 * (0.004 * 0.004 * 0.004 * 1e6)]
    assert got["penetration_depth"][2] is None and got["penetration_depth"][0] == 0.0
    assert got["penetration_depth"][1] == float(np.float32(0.0062)) * 100.0
    assert math.isclose(got["penetration_volume"][1], 124.096, rel_tol=1e-12)       # cm^3
    assert json.loads(json.dumps(got))["penetration_volume"][2] is None
    assert contact.volume_stats(np.asarray([5]), np.asarray([0.01]), 0.001) == {"penetration_volume": [5 * (0.001 ** 3 * 1e6)],
                                                                                 "penetration_depth": [1.0]}
    for res in (0.0, -1.0, INF, NAN):
        with pytest.raises(RuntimeError):
            contact.volume_stats([1], [0.0], res)
    with pytest.raises(RuntimeError):
        contact.volume_stats([1, 2], [0.0], 0.001)
    # floor(X / (H^3 * 1e6)): 1 cm^3 at 4 mm voxels is 15.625 voxels
    assert contact.volume_limit(1.0, 0.004) == 15 and contact.volume_limit(0.0, 0.004) == 0
    assert contact.volume_limit(INF, 0.001) == 2 ** 31 - 1 and contact.volume_limit(1.0, 0.001) in (999, 1000)


# ------------------------------------------------------------------------------------------------------ CPU: the references
def test_reference_voxelises_the_sphere_to_its_volume():
    """Reference (a), all space as the hull: count * h^3 within 1 % of the mesh's own volume (signed tetrahedra, float64)."""
    v, f = sphere()
    h = 0.002
    lo, n = ref.box_of(v, h)
    inside, covers = ref.hand_voxels(v, f, lo, n, h)
    volume = ref.mesh_volume(v, f)
    print("voxels", int(inside.sum()), "mesh volume in voxels", volume / h ** 3, "round sphere", 4 / 3 * math.pi * RADIUS ** 3 / h ** 3)
    assert abs(inside.sum() * h ** 3 - volume) <= 0.01 * volume
    assert int(inside.sum()) == 33112
    assert (covers % 2 == 0).all(), "a column of a closed mesh is covered an odd number of times"


@pytest.mark.parametrize("h,voxels", [(0.002, 15159), (0.004, 1939)])
def test_reference_equals_the_float64_brute_force_up_to_uncertain_voxels(h, voxels):
    v, f = sphere()
    count, depth, status, both, lo, _ = ref.grasp_volume_one(v, f, *NO_LOOPS, ref.SPHERE_PLANES, h=h, voxels=True)
    brute, uncertain = ref.brute_force(v, f, *NO_LOOPS, ref.SPHERE_PLANES, lo, both.shape, h=h)
    differ = both ^ brute
    print("h", h, "count", count, "brute force", int(brute.sum()), "differ", int(differ.sum()), "uncertain", int(uncertain.sum()))
    assert status == 0 and count == int(both.sum()) == voxels
    assert not (differ & ~uncertain).any(), "a voxel differs that is not within 1e-6 m of a surface"
    assert uncertain.sum() <= 0.005 * count
    # the deepest vertex: against float64, to fp32 rounding of numbers of this size
    want = max(0.0, float(np.min(ref.SPHERE_PLANES[None, :, 3].astype(np.float64)
                                 - v.astype(np.float64) @ ref.SPHERE_PLANES[:, :3].T.astype(np.float64), axis=1).max()))
    assert abs(float(depth) - want) <= 4 * np.finfo(np.float32).eps * 0.1 and want > 0.005


def test_reference_keeps_the_parity_on_edges_and_vertices():
    """An octahedron placed so that columns run exactly through a silhouette edge, an inner edge and a vertex (every number a small
    multiple of a power of two: all edge values are exact): every column is covered an even number of times, and the count is the
    octahedron's up to its surface voxels."""
    h = 2.0 ** -9
    a = 4 * h
    c = np.asarray([0.5 * h, 0.5 * h, 0.0])
    v = (c + np.asarray([[a, 0, 0], [-a, 0, 0], [0, a, 0], [0, -a, 0], [0, 0, a], [0, 0, -a]])).astype(np.float32)
    f = np.asarray([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    assert ref.mesh_volume(v, f) > 0
    lo, n = ref.box_of(v, h)
    inside, covers = ref.hand_voxels(v, f, lo, n, h)
    x, y = ref.centres(lo[0] + np.arange(n[0]), h), ref.centres(lo[1] + np.arange(n[1]), h)
    on_edge = np.abs(x[:, None] - np.float32(c[0])) + np.abs(y[None, :] - np.float32(c[1])) == np.float32(a)     # the silhouette, exactly
    assert on_edge.sum() >= 12 and (covers % 2 == 0).all() and set(covers[on_edge].tolist()) <= {0, 2}
    assert covers[(x == v[4, 0]).argmax(), (y == v[4, 1]).argmax()] == 2             # the column through both apexes
    volume = ref.mesh_volume(v, f) / h ** 3                                            # 4/3 * 4^3 = 85.3 voxels
    assert abs(inside.sum() - volume) <= 0.5 * volume and inside.sum() > 0
    # mirrored in x the mesh changes every traversal and every sign of A: the columns' parity holds as well
    m = v.copy()
    m[:, 0] = np.float32(h) - m[:, 0]
    inside_m, covers_m = ref.hand_voxels(m, f[:, ::-1].copy(), *ref.box_of(m, h), h)
    assert (covers_m % 2 == 0).all() and inside_m.sum() > 0


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def run_volume(hand, faces, loops, planes, plane_off, obj_of_row, R=None, t=None, h=0.004, err=None):
    out = ops.grasp_volume(gpu(np.ascontiguousarray(hand, np.float32)), gpu(np.asarray(faces, np.int32)), gpu(loops[0]), gpu(loops[1]),
                           gpu(np.asarray(planes, np.float32).reshape(-1, 4)), gpu(np.asarray(plane_off, np.int32)),
                           gpu(np.asarray(obj_of_row, np.int64)), None if R is None else gpu(np.asarray(R, np.float32)),
                           None if t is None else gpu(np.asarray(t, np.float32)), h, err=err)
    B = hand.shape[0]
    assert all(tuple(o.shape) == (B,) for o in out) and [o.dtype for o in out] == [torch.int32, torch.float32, torch.int32]
    return dict(zip(OUTPUTS, (o.cpu().numpy() for o in out)))


def assert_same(got, want, rows=None, what=""):
    """Integers equal, the depth bit for bit; a NaN is a NaN."""
    for k in OUTPUTS:
        g, w = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        if k != "depth":
            assert np.array_equal(g, w), (what, k, g, w)
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g)[~nan], bits(w)[~nan]), (what, k, g, w)


def sphere_hands(B, tag):
    """B different hands: the sphere scaled, shifted and roughened a little (still closed, still near the planes)."""
    v, f = sphere()
    scale = np.linspace(0.9, 1.1, B).astype(np.float32)[:, None, None]
    shift = synth.synthetic_normal((B, 1, 3), 51, f"volume/{tag}/shift", 0.004).numpy()
    rough = synth.synthetic_normal((B, len(v), 3), 51, f"volume/{tag}/rough", 0.0003).numpy()
    return (v[None] * scale + shift + rough).astype(np.float32), f


@pytest.mark.gpu
def test_grasp_volume_equals_the_reference_exactly_and_ignores_the_batch():
    hand, f = sphere_hands(5, "plain")
    hand[4] = hand[0]                                                                # the same grasp at rows 0 and 4
    off, rows = [0, 7], np.zeros(5, np.int64)
    got = run_volume(hand, f, NO_LOOPS, ref.SPHERE_PLANES, off, rows)
    want = ref.grasp_volume(hand, f, *NO_LOOPS, ref.SPHERE_PLANES, off, rows, h=0.004)
    print("count", got["count"], want["count"], "depth", got["depth"], want["depth"])
    assert_same(got, want, what="sphere")
    assert (want["status"] == 0).all() and (want["count"] > 1000).all() and len(set(want["count"][:4].tolist())) == 4
    assert (want["depth"] > 0.003).all()
    assert got["count"][0] == got["count"][4] and bits(got["depth"])[0] == bits(got["depth"])[4]
    alone = run_volume(hand[:1], f, NO_LOOPS, ref.SPHERE_PLANES, off, rows[:1])
    assert_same(alone, {k: x[:1] for k, x in got.items()}, what="row 0 alone")
    # the plain sphere: the figure the CPU tests pin
    plain = run_volume(sphere()[0][None], f, NO_LOOPS, ref.SPHERE_PLANES, off, rows[:1])
    assert plain["count"].tolist() == [1939] and plain["status"].tolist() == [0]
    empty = run_volume(hand[:0], f, NO_LOOPS, ref.SPHERE_PLANES, off, rows[:0])
    assert [empty[k].shape for k in OUTPUTS] == [(0,)] * 3


@pytest.mark.gpu
def test_grasp_volume_in_the_rotated_rows_frame():
    """hand = R v + t as the entry points hold it (the object was moved by R, t): the kernel undoes it per row; checked against
    reference (a) fed the same R and t, and the counts stay near the unrotated ones (the lattice is the object's)."""
    base, f = sphere_hands(4, "rot")
    R = generate.rotation_xyz(synth.synthetic_uniform((4, 3), 52, "volume/rot/angles", 0.0, 2 * math.pi).numpy().astype(np.float64))
    t = np.asarray(generate.CANONICAL_OFFSET)
    hand = (np.einsum("bij,bvj->bvi", R, base.astype(np.float64)) + t).astype(np.float32)
    off, rows = [0, 7], np.zeros(4, np.int64)
    got = run_volume(hand, f, NO_LOOPS, ref.SPHERE_PLANES, off, rows, R=R, t=t)
    want = ref.grasp_volume(hand, f, *NO_LOOPS, ref.SPHERE_PLANES, off, rows, R=R.astype(np.float32), t=t.astype(np.float32), h=0.004)
    still = ref.grasp_volume(base, f, *NO_LOOPS, ref.SPHERE_PLANES, off, rows, h=0.004)
    print("count", got["count"], want["count"], still["count"])
    assert_same(got, want, what="rotated")
    assert (want["status"] == 0).all() and (np.abs(want["count"] - still["count"]) <= 0.02 * still["count"]).all()
    no_t = run_volume(hand, f, NO_LOOPS, ref.SPHERE_PLANES, off, rows, R=R)          # R alone: u = v
    assert_same(no_t, ref.grasp_volume(hand, f, *NO_LOOPS, ref.SPHERE_PLANES, off, rows, R=R.astype(np.float32), h=0.004), what="R alone")


@pytest.mark.gpu
def test_grasp_volume_with_two_objects_and_the_status_cases():
    hand, f = sphere_hands(6, "objects")
    box = ref.SPHERE_PLANES[:6].copy()
    box[:, 3] *= 0.5                                                                 # object 1: half the box, without the oblique plane
    far = ref.SPHERE_PLANES.copy()
    far[:, 3] += far[:, :3] @ np.asarray([0.0, 0.0, 1.0], np.float32)                # the same hull, 1 m up
    planes = np.concatenate([ref.SPHERE_PLANES, box, far])                          # objects 0 (7 planes), 1 (6), 2 (none), 3 (7, far)
    off = [0, 7, 13, 13, 20]
    rows = np.asarray([0, 1, 2, 3, 1, 0], np.int64)
    hand[1] = hand[0]                                                                # one hand against objects 0 and 1 ...
    hand[4] = hand[1]                                                                # ... and against object 1 twice
    want = ref.grasp_volume(hand, f, *NO_LOOPS, planes, off, rows, h=0.004)
    got = run_volume(hand, f, NO_LOOPS, planes, off, rows)
    print(got, want)
    assert_same(got, want, what="objects")
    assert want["status"].tolist() == [0, 0, 1, 1, 0, 0] and want["count"][2:4].tolist() == [0, 0] and bits(want["depth"][2:4]).tolist() == [0, 0]
    assert want["count"][0] > want["count"][1] > 0 and got["count"][1] == got["count"][4]        # each row sees its own object's planes
    # a NaN vertex: status 3, and the rows beside it untouched
    bad = hand.copy()
    bad[1, 300, 1] = np.nan
    bad[5, 0, 0] = np.inf
    nan = run_volume(bad, f, NO_LOOPS, planes, off, rows)
    assert_same(nan, ref.grasp_volume(bad, f, *NO_LOOPS, planes, off, rows, h=0.004), what="nan")
    assert nan["status"].tolist() == [0, 3, 1, 1, 0, 3] and nan["count"][[1, 5]].tolist() == [-1, -1] and np.isnan(nan["depth"][[1, 5]]).all()
    assert_same(nan, got, rows=[0, 2, 3, 4], what="beside the NaN rows")
    assert contact.volume_stats(nan["count"], nan["depth"], 0.004)["penetration_volume"][1] is None
    # a lattice too fine for the box: status 2, the depth still there
    fine = run_volume(hand[:2], f, NO_LOOPS, planes, off, rows[:2], h=1e-5)
    assert_same(fine, ref.grasp_volume(hand[:2], f, *NO_LOOPS, planes, off, rows[:2], h=1e-5), what="fine")
    assert fine["status"].tolist() == [2, 2] and fine["count"].tolist() == [-1, -1] and np.array_equal(bits(fine["depth"]), bits(got["depth"][:2]))
    # an object index out of range: the error bit, and the binding raises without a flag of the caller's
    err = ops.new_err_flag(torch.device(DEV))
    out = run_volume(hand[:3], f, NO_LOOPS, planes, off, np.asarray([0, 4, -1], np.int64), err=err)
    assert int(err.item()) == 1 and out["status"].tolist() == [0, 4, 4] and out["count"].tolist() == [int(got["count"][0]), -1, -1]
    with pytest.raises(RuntimeError, match="out of bounds"):
        run_volume(hand[:3], f, NO_LOOPS, planes, off, np.asarray([0, 4, 1], np.int64))
    lib = _lib.load()                                                                # straight through the C ABI: DVQ_EINVAL, nothing launched
    one = torch.full((64,), 7.0, device=DEV)
    p = one.data_ptr()
    for V, F, L, h, B in ((2049, 4, 0, 0.004, 1), (0, 4, 0, 0.004, 1), (5, 8193, 0, 0.004, 1), (5, 4, 65, 0.004, 1), (5, 4, 0, 0.0, 1),
                          (5, 4, 0, INF, 1), (5, 4, 0, NAN, 1), (5, 4, 0, 0.004, -1)):
        assert lib.dvq_grasp_volume(p, V, p, F, p, p, L, 0, p, 1, p, 1, p, None, None, B, h, p, p, p, p, None) == 1, (V, F, L, h, B)
    assert lib.dvq_grasp_volume(p, 5, p, 4, p, p, 0, 0, p, 1, p, 1, p, None, p, 1, 0.004, p, p, p, p, None) == 1      # t without R
    assert (one == 7.0).all()                                                        # nothing was written


def mano_hands(tmp_path, B):
    """B posed hands from the MANO layer on the real model, and the topology."""
    from test_grasp_select import mano_pkl
    from dvqvae_amd import mano as dmano
    layer = dmano.load(model_path=mano_pkl(tmp_path), model_type="mano", use_pca=True, num_pca_comps=45, flat_hand_mean=True).to(DEV)
    p = synth.synthetic_normal((B, 61), 53, "volume/mano", 0.4).to(DEV)
    out = layer(betas=p[:, :10].contiguous(), global_orient=p[:, 10:13].contiguous(), hand_pose=p[:, 13:58].contiguous(),
                transl=(0.05 * p[:, 58:61]).contiguous())
    return out.vertices, np.asarray(layer.faces)


def palm_planes(centre, half=(0.03, 0.025, 0.02)):
    """Twelve half-spaces about ``centre``: a box, cut by the four diagonals of its xy section and by two of its xz section."""
    n = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0.6, 0.8, 0], [-0.6, 0.8, 0], [0.6, -0.8, 0],
         [-0.6, -0.8, 0], [0.8, 0, 0.6], [-0.8, 0, -0.6]]
    d = [half[0], half[0], half[1], half[1], half[2], half[2]] + [0.0313] * 4 + [0.0287] * 2
    n = np.asarray(n, np.float64)
    return np.concatenate([n, (np.asarray(d) + n @ np.asarray(centre, np.float64))[:, None]], axis=1).astype(np.float32)


@pytest.mark.gpu
def test_grasp_volume_on_the_real_hand_sealed_at_the_wrist(tmp_path):
    verts, faces = mano_hands(tmp_path, 3)
    topo = contact.HandTopology(faces, 778, DEV)
    sealed, loop_off, loop_vert = (x.cpu().numpy() for x in topo.sealed())
    assert topo.sealed()[0] is topo.sealed()[0] and sealed.shape == (1554, 3) and loop_off.tolist() == [0, 16]
    hand = verts.cpu().numpy()
    palms = [palm_planes(hand[b][[95, 220, 110, 60]].mean(0)) for b in range(3)]     # about four palm vertices of each hand
    planes, plane_off = contact.pack_planes(palms)
    rows = np.arange(3)
    out = contact.grasp_volume(topo, verts, gpu(planes), gpu(plane_off), gpu(rows), res=0.004)
    assert tuple(out) == OUTPUTS
    got = {k: x.cpu().numpy() for k, x in out.items()}
    want = ref.grasp_volume(hand, sealed, loop_off, loop_vert, planes, plane_off, rows, h=0.004)
    print("count", got["count"], want["count"], "depth", got["depth"], want["depth"])
    assert_same(got, want, what="mano")
    assert (want["status"] == 0).all() and (want["count"] > 50).all() and (want["depth"] > 0.005).all()
    # the sealed hand is closed: every column of the box is covered an even number of times
    v0 = ref.object_frame(hand[0], loop_off, loop_vert, None, None)
    assert (ref.hand_voxels(v0, sealed, *ref.box_of(v0, 0.004), 0.004)[1] % 2 == 0).all()


@pytest.mark.gpu
def test_grasp_volume_across_bit_words_and_tiles():
    """The sphere stretched four times in z at 1 mm voxels: about 80 x 80 x 320 cells, so a column's cells span eleven 32-bit words
    and the box several tiles of columns."""
    v, f = sphere()
    hand = (v * np.asarray([1.0, 1.0, 4.0], np.float32))[None].astype(np.float32)
    planes = ref.SPHERE_PLANES.copy()
    planes[4:6, 3] = [0.1237, 0.0951]                                                # z from -0.0951 to 0.1237
    got = run_volume(hand, f, NO_LOOPS, planes, [0, 7], [0], h=0.001)
    want = ref.grasp_volume(hand, f, *NO_LOOPS, planes, [0, 7], [0], h=0.001)
    print(got, want)
    assert_same(got, want, what="tall")
    assert want["status"].tolist() == [0] and want["count"][0] > 400000


# ------------------------------------------------------------------------------------------------------ GPU: end to end
E2E_SEED, E2E_M, E2E_K, E2E_RES = 9, 8, 4, 0.004
E2E_INDICES = [5, 2]


def e2e_clouds():
    """Two [N,3] clouds of different point counts: cubes of points about the place where the synthetic weights put every hand
    (tests/test_grasp_select.py: e2e_objects), small enough to leave part of the hand outside their hulls."""
    centre = np.asarray([-0.12, -0.07, 0.13])
    return [synth.synthetic_uniform((n, 3), 90 + i, "volume/e2e", -w, w).numpy().astype(np.float64) + centre
            for i, (n, w) in enumerate(((300, 0.05), (200, 0.04)))]


def reference_of_json(net, j, cloud, topo):
    """volume_stats of reference (a) on MANO of the parameters a JSON holds."""
    p = torch.tensor(j["recon_params"], dtype=torch.float32, device=DEV).reshape(-1, 61)
    verts = net.rh_mano(betas=p[:, :10], global_orient=p[:, 10:13], hand_pose=p[:, 13:58], transl=p[:, 58:61]).vertices.cpu().numpy()
    sealed, loop_off, loop_vert = (x.cpu().numpy() for x in topo.sealed())
    planes = contact.hull_planes(cloud)
    want = ref.grasp_volume(verts, sealed, loop_off, loop_vert, planes, [0, len(planes)], np.zeros(len(verts), np.int64), h=E2E_RES)
    return want, contact.volume_stats(want["count"], want["depth"], E2E_RES)


def _run_main(dataset, out_dir, extra, mano):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
def test_entry_points_write_and_guard_by_the_volume(tmp_path):
    pytest.importorskip("scipy")
    from test_grasp_select import _gennet, mano_pkl
    net = _gennet(tmp_path)
    mano = mano_pkl(tmp_path)
    clouds = e2e_clouds()
    objs = [generate.object_tensor(c) for c in clouds]
    M, k = E2E_M, E2E_K
    topo = generate._hand_topology(net, 778, torch.device(DEV))
    # the candidates' counts, and a limit that demotes some of them and not all
    figures = generate.generate_for_objects(net, objs, M, False, 3, [0, 1], volume=True, volume_res=E2E_RES)
    counts = [g["volume"]["count"].cpu().numpy() for g in figures]
    print("counts of all candidates", [c.tolist() for c in counts])
    assert all((c >= 0).all() for c in counts) and len(set(counts[0].tolist())) >= 3
    cell = E2E_RES ** 3 * 1e6
    limit = int(np.sort(counts[0])[M // 2 - 1])                                      # object 0: its lower half passes
    X = (limit + 0.5) * cell
    assert contact.volume_limit(X, E2E_RES) == limit and (counts[0] > limit).any() and (counts[0] <= limit).any()
    for i, g in enumerate(figures):                                                  # without candidates: every grasp, the three fields last
        want, stats = reference_of_json(net, g["json"], objs[i][:3].T.numpy().astype(np.float64), topo)
        assert list(g["json"])[-3:] == list(FIELDS) and g["json"]["volume_voxels"] == want["count"].tolist()
        assert all(g["json"][f] == stats[f] for f in FIELDS[:2]) and (want["status"] == 0).all()
        assert np.array_equal(g["volume"]["count"].cpu().numpy(), want["count"]) and np.array_equal(bits(g["volume"]["depth"].cpu().numpy()), bits(want["depth"]))
    # best-of-M through the API: demoted candidates rank after the others, whatever the grouping of the calls
    demoted = False
    for rows_per_call in (16384, 8):
        got = generate.generate_for_objects(net, objs, k, False, 3, [0, 1], rows_per_call=rows_per_call, candidates=M, volume=True,
                                            volume_res=E2E_RES, max_volume=X)
        for i, g in enumerate(got):
            all_counts = g["volume_scores"]["count"].cpu()
            assert np.array_equal(all_counts.numpy(), figures[i]["volume"]["count"].cpu().numpy())   # candidate c is grasp c of the M-run
            cls, key = contact.select_keys({n: t.cpu() for n, t in g["scores"].items()}, "penetration", 1)
            cls = torch.maximum(cls, (all_counts > limit).to(torch.int32))
            order = score_ref.segment_topk(cls.numpy(), key.numpy(), 1, M, M)[0]
            c = g["candidate"].cpu().numpy()
            assert np.array_equal(c, order[:k]), (c, order, cls.tolist(), key.tolist())
            over = (all_counts > limit).numpy()
            ranks = {int(cand): r for r, cand in enumerate(order)}
            assert all(ranks[a] < ranks[b] for a in range(M) for b in range(M) if cls[a] == 0 and over[b]), "a demoted candidate ranks before a fit one"
            demoted |= 0 < over.sum() < M
            assert g["json"]["volume_voxels"] == all_counts.numpy()[c].tolist()
    assert demoted
    # the entry point: files, byte-identical for every --rows_per_call, and penetration.json consistent with them
    files = []
    for i, c in enumerate(clouds):
        files.append(str(tmp_path / f"cloud{i}.npy"))
        np.save(files[-1], c)
    base = ["--objects"] + files + ["--num_grasp", str(k), "--candidates", str(M)]
    vol = base + ["--volume", "1", "--volume_res", str(E2E_RES), "--max_volume", repr(X)]
    names0, bytes0 = _run_main("obman", str(tmp_path / "v16384"), vol + ["--rows_per_call", "16384"], mano)
    names8, bytes8 = _run_main("obman", str(tmp_path / "v8"), vol + ["--rows_per_call", "8"], mano)
    assert names0 == names8 == ["obj_id_cloud0.json", "obj_id_cloud1.json"] and bytes0 == bytes8
    pen0, pen8 = (open(str(tmp_path / d / "penetration.json"), "rb").read() for d in ("v16384", "v8"))
    assert pen0 == pen8
    rows = []
    for i, data in enumerate(bytes0):
        j = json.loads(data)
        assert b"NaN" not in data and list(j)[-3:] == list(FIELDS) and all(len(j[f]) == k for f in FIELDS)
        want, stats = reference_of_json(net, j, objs[i][:3].T.numpy().astype(np.float64), topo)   # the cloud as the run holds it: fp32
        assert j["volume_voxels"] == want["count"].tolist() and all(j[f] == stats[f] for f in FIELDS[:2])
        assert all(v <= limit for v in j["volume_voxels"]) or len([v for v in j["volume_voxels"] if v <= limit]) < k
        rows += list(zip(j["volume_voxels"], j["penetration_volume"], j["penetration_depth"]))
    pen = json.loads(pen0)
    assert set(pen) == {"res", "grasps", "mean_volume_cm3", "mean_depth_cm", "contact_ratio"} and pen["res"] == E2E_RES
    assert pen["grasps"] == len(rows) == 2 * k
    assert math.isclose(pen["mean_volume_cm3"], sum(r[1] for r in rows) / len(rows), rel_tol=1e-12)
    assert math.isclose(pen["mean_depth_cm"], sum(r[2] for r in rows) / len(rows), rel_tol=1e-12)
    assert pen["contact_ratio"] == sum(1 for r in rows if r[0] >= 1) / len(rows)
    # a run that omits the flags, or names their defaults, writes the bytes of the run before the feature and no penetration.json
    names_p, plain = _run_main("obman", str(tmp_path / "plain"), base, mano)
    names_o, off = _run_main("obman", str(tmp_path / "off"), base + ["--volume", "0", "--volume_res", "0.002"], mano)
    assert names_p == names_o == names0 and off == plain
    assert all(set(json.loads(d)) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact"}
               for d in plain)
    assert not os.path.exists(str(tmp_path / "plain" / "penetration.json")) and not os.path.exists(str(tmp_path / "off" / "penetration.json"))
    for i, data in enumerate(bytes0):                                                # the volume run adds fields; the shared ones of a kept candidate agree
        assert set(json.loads(data)) == set(json.loads(plain[i])) | set(FIELDS)
