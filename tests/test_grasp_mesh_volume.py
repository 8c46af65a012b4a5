"""dvq_grasp_mesh_volume: the voxels shared by the sealed hand and the object's MESH, and the ``--volume_mesh`` option of the entry
points.  CPU group (unmarked): reference (a) of tests/grasp_mesh_volume_ref.py -- the header's definition in fp32 -- against the
independent float64 brute force (b), the exact tie rule, hollow objects, the statuses and error bits of (a), and the host layers.  GPU
group: the kernel equals (a) exactly, integer for integer, and the entry points write what (a) gives."""
import inspect
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops, synth

import grasp_mesh_volume_ref as ref
import grasp_score_ref as score_ref
import grasp_volume_ref as vref

DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")
RADIUS = 0.04
NO_LOOPS = (np.zeros(1, np.int32), np.zeros(0, np.int32))
FIELDS = ("penetration_volume", "penetration_depth", "volume_voxels")
# the objects of the sphere tests, at offsets that are no multiples of either lattice spacing
TORUS = ref.torus(8, 8, R=0.03, r=0.012, centre=(0.0113, 0.0071, 0.0037))              # 128 faces
CUBE = ref.box((0.021, 0.017, 0.013), (0.0187, -0.0093, 0.0111))                       # 12 faces


def sphere():
    return score_ref.sphere_mesh(radius=RADIUS)


# ------------------------------------------------------------------------------------------------------ CPU: (a) against (b)
@pytest.mark.parametrize("name,h,voxels", [("torus", 0.004, 812), ("torus", 0.002, 6420), ("cube", 0.004, 520), ("cube", 0.002, 4072)])
def test_reference_equals_the_float64_brute_force_up_to_uncertain_voxels(name, h, voxels):
    v, f = sphere()
    mv, mf = {"torus": TORUS, "cube": CUBE}[name]
    assert all(abs(c / h - round(c / h)) > 0.01 and abs(c / h - 0.5 - round(c / h - 0.5)) > 0.01 for c in mv.min(0).tolist() + mv.max(0).tolist())
    count, status, bad, both, in_hand, in_obj, lo, _ = ref.grasp_mesh_volume_one(v, f, *NO_LOOPS, mv, mf, h=h, voxels=True)
    brute, uncertain = ref.brute_force(v, f, *NO_LOOPS, mv, mf, lo, both.shape, h=h)
    differ = both ^ brute
    print(name, "h", h, "count", count, "brute force", int(brute.sum()), "differ", int(differ.sum()), "uncertain", int(uncertain.sum()))
    assert status == 0 and not bad and count == int(both.sum()) == voxels
    assert not (differ & ~uncertain).any(), "a voxel differs that is not within 1e-6 m of a surface"
    assert uncertain.sum() <= 0.005 * count                                          # (b) alone stays within the cap off the lattice
    assert 0 < count < in_obj.sum() and count < in_hand.sum()                        # a proper intersection: part of the object is outside


# ------------------------------------------------------------------------------------------------------ CPU: the tie rule, exactly
TIE_H = 2.0 ** -9


def tie_box():
    """A box whose faces, edges and corners pass exactly through column centres and whose top and bottom lie exactly at cell centres
    (every coordinate a small odd multiple of h / 2): x from c(-4) to c(4), y from c(-3) to c(3), z from c(-2) to c(2).  The diagonal
    of its top and bottom faces runs through the column (0, 0)'s centre.  Inside by the tie rule: columns -4 .. 3 and -3 .. 2 (an
    edge belongs to the side the column would reach when moved by (eps, eps^2)), cells -2 .. 1 (a crossing must EXCEED the centre)."""
    h = TIE_H
    lo_, hi_ = np.asarray([-3.5, -2.5, -1.5]) * h, np.asarray([4.5, 3.5, 2.5]) * h
    return ref.box((hi_ - lo_) / 2, (hi_ + lo_) / 2), 8 * 6 * 4


def test_tie_rule_on_a_box_through_column_centres():
    (mv, mf), closed_form = tie_box()
    h = TIE_H
    assert np.array_equal(mv.astype(np.float64) / (h / 2), np.round(mv.astype(np.float64) / (h / 2)))     # exact in fp32
    v, f = sphere()
    count, status, bad, both, in_hand, in_obj, lo, _ = ref.grasp_mesh_volume_one(v, f, *NO_LOOPS, mv, mf, h=h, voxels=True)
    _, covers, _ = ref.object_voxels(mv, mf, lo, both.shape, h)
    x, y = vref.centres(lo[0] + np.arange(both.shape[0]), h), vref.centres(lo[1] + np.arange(both.shape[1]), h)
    on_edge = ((x[:, None] == mv[:, 0].min()) | (x[:, None] == mv[:, 0].max())) & (y[None, :] >= mv[:, 1].min()) & (y[None, :] <= mv[:, 1].max())
    on_edge |= ((y[None, :] == mv[:, 1].min()) | (y[None, :] == mv[:, 1].max())) & (x[:, None] >= mv[:, 0].min()) & (x[:, None] <= mv[:, 0].max())
    assert on_edge.sum() == 2 * 9 + 2 * 7 - 4 and (covers % 2 == 0).all() and set(covers[on_edge].tolist()) <= {0, 2}
    assert covers[(x == vref.centres(0, h)).argmax(), (y == vref.centres(0, h)).argmax()] == 2           # the column on the diagonal
    assert in_obj.sum() == closed_form and status == 0 and count == closed_form      # the sphere holds the whole box
    # mirrored in x every traversal and every sign of A changes: the parity holds, the columns inside move by one
    m = mv.copy()
    m[:, 0] = np.float32(h) - m[:, 0]
    obj_m, covers_m, _ = ref.object_voxels(m, mf[:, ::-1].copy(), lo, both.shape, h)
    assert (covers_m % 2 == 0).all() and obj_m.sum() == closed_form


# ------------------------------------------------------------------------------------------------------ CPU: hollow objects
def test_a_finger_through_the_hole_shares_nothing_with_the_torus_but_much_with_its_hull():
    pytest.importorskip("scipy")
    mv, mf = ref.torus(16, 8, R=0.03, r=0.01, centre=(0.0007, -0.0011, 0.0013))
    planes = contact.hull_planes(mv)
    h = 0.002
    through, ff = ref.box((0.0043, 0.0037, 0.03), (0.0011, 0.0003, 0.0007))          # a thin finger along z, threaded through the hole
    count, status, _ = ref.grasp_mesh_volume_one(through, ff, *NO_LOOPS, mv, mf, h=h)
    hull_count = vref.grasp_volume_one(through, ff, *NO_LOOPS, planes, h=h)[0]
    print("threaded: mesh", count, status, "hull", hull_count)
    assert (count, status) == (0, 1) and hull_count > 100                            # the hull swallows the hole
    sunk, _ = ref.box((0.0043, 0.0037, 0.03), (0.0311, 0.0003, 0.0007))              # the same finger sunk into the tube
    count, status, _ = ref.grasp_mesh_volume_one(sunk, ff, *NO_LOOPS, mv, mf, h=h)
    hull_count = vref.grasp_volume_one(sunk, ff, *NO_LOOPS, planes, h=h)[0]
    print("sunk: mesh", count, status, "hull", hull_count)
    assert status == 0 and 0 < count <= hull_count


# ------------------------------------------------------------------------------------------------------ CPU: statuses and error bits of (a)
def far_mesh():
    """The cube with faces far outside any hand's box added: a closed tetrahedron at 1e30, faces from the cube's corners to vertices
    at +-1e30 and at +inf, a face far above and one far below the box, and a face with a NaN height."""
    v, f = CUBE
    more = np.asarray([[1e30, 1e30, 1e30], [1.1e30, 1e30, 1e30], [1e30, 1.1e30, 1e30], [1e30, 1e30, 1.1e30],      # 8 .. 11
                       [-1e30, 3.0, 0.5], [np.inf, 0.0, 0.0], [0.01, 0.0, 7.0], [0.03, 0.01, 7.0], [0.01, 0.02, 7.0],   # 12 .. 16
                       [0.01, 0.0, -7.0], [0.03, 0.01, -7.0], [0.01, 0.02, -7.0], [0.02, 0.0, np.nan]], np.float32)  # 17 .. 20
    faces = [[8, 10, 9], [8, 9, 11], [9, 10, 11], [10, 8, 11], [0, 1, 12], [2, 12, 6], [0, 5, 13], [14, 15, 16], [17, 18, 19], [4, 5, 20]]
    return np.concatenate([v, more]).astype(np.float32), np.concatenate([f, np.asarray(faces, np.int64)])


def status_case():
    """Rows and objects for every status and both error bits: objects 0 torus, 1 cube, 2 the far mesh, 3 without a face, 4 the cube
    with a face index out of range, 5 the torus 1 m up."""
    v, f = sphere()
    hand = np.repeat(v[None], 8, axis=0).astype(np.float32)
    hand[6, 3, 1] = np.nan
    bad_cube = (CUBE[0], np.concatenate([CUBE[1], [[0, 1, 8]]]))
    up = (TORUS[0] + np.asarray([0, 0, 1], np.float32), TORUS[1])
    meshes = [TORUS, CUBE, far_mesh(), (CUBE[0], np.zeros((0, 3), np.int64)), bad_cube, up]
    rows = np.asarray([0, 1, 2, 3, 4, 5, 0, 0], np.int64)
    return hand, f, meshes, rows


def test_reference_statuses_error_bits_and_far_faces():
    hand, f, meshes, rows = status_case()
    packed = ref.pack(meshes)
    out = ref.grasp_mesh_volume(hand, f, *NO_LOOPS, *packed, rows, h=0.004)
    print(out)
    assert out["status"].tolist() == [0, 0, 0, 1, 0, 1, 3, 0] and out["err"] == 2     # (the face index of object 4)
    assert out["count"][3] == 0 and out["count"][5] == 0 and out["count"][6] == -1 and out["count"][7] == out["count"][0] == 812
    assert out["count"][4] == out["count"][1] == 520                                  # the bad face is skipped
    # the far mesh is open, so its count is defined by (a) alone; the faces at 1e30, at infinity and below the box change nothing,
    # the face above the box flips its columns, the NaN face covers nothing
    near = ref.grasp_mesh_volume_one(hand[0], f, *NO_LOOPS, *meshes[2], h=0.004)
    assert near[:2] == (int(out["count"][2]), 0) and near[0] != out["count"][1]
    keep = [i for i in range(len(meshes[2][1])) if i not in (12, 13, 14, 15, 18, 20, 21)]
    assert ref.grasp_mesh_volume_one(hand[0], f, *NO_LOOPS, meshes[2][0], meshes[2][1][keep], h=0.004)[:2] == near[:2]
    assert ref.grasp_mesh_volume_one(hand[0], f, *NO_LOOPS, meshes[2][0], meshes[2][1][[i for i in keep if i != 19]], h=0.004)[0] != near[0]
    # status 2: the box is refused as dvq_grasp_volume refuses it; status 4 and the two bits
    fine = ref.grasp_mesh_volume(hand[:1], f, *NO_LOOPS, *packed, rows[:1], h=1e-5)
    assert fine["status"].tolist() == [2] and fine["count"].tolist() == [-1]
    out = ref.grasp_mesh_volume(hand[:3], f, *NO_LOOPS, *packed, np.asarray([6, -1, 0]), h=0.004)
    assert out["status"].tolist() == [4, 4, 0] and out["count"].tolist() == [-1, -1, 812] and out["err"] == 1
    broken = list(packed)
    broken[3] = packed[3].copy()
    broken[3][2] = 9999                                                              # object 1's faces leave the array
    out = ref.grasp_mesh_volume(hand[:2], f, *NO_LOOPS, *broken, rows[:2], h=0.004)
    assert out["status"].tolist() == [0, 4] and out["err"] == 2


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops, options
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_flag(dataset):
    assert generate.parse_args(dataset, []).volume_mesh == 0
    files = ["--objects", "a.npy", "--object_meshes", "a.obj"]
    for k in (1, 2):
        a = generate.parse_args(dataset, files + ["--volume", "1", "--volume_mesh", str(k)])
        assert a.volume_mesh == k and a.mesh_depth == 0                              # the meshes without the mesh depth
    assert generate.parse_args(dataset, files + ["--max_volume", "2", "--candidates", "8", "--num_grasp", "4", "--volume_mesh", "2"]).volume_mesh == 2
    assert generate.parse_args(dataset, files + ["--volume_mesh", "0"]).volume_mesh == 0
    for bad in (files + ["--volume", "1", "--volume_mesh", "3"], files + ["--volume", "1", "--volume_mesh", "-1"],
                ["--volume", "1", "--volume_mesh", "1"], files + ["--volume_mesh", "2"]):          # a value, no meshes, no volume figure
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_keyword_path_checks_the_option_before_any_work():
    mesh = (np.zeros((4, 3)), np.asarray([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]]))
    objs = [torch.zeros(4, 8)]
    call = lambda **kw: generate.generate_with_volume_mesh(None, objs, 5, True, 0, [0], **kw)     # net = None: nothing may touch it
    with pytest.raises(RuntimeError, match="volume_mesh must be 0, 1 or 2"):
        call(volume_mesh=3, volume=True, object_meshes=[mesh])
    with pytest.raises(RuntimeError, match="volume_mesh needs object_meshes"):
        call(volume_mesh=2, volume=True)
    with pytest.raises(RuntimeError, match="volume_mesh needs object_meshes"):
        call(volume_mesh=1, volume=True, object_meshes=[mesh, mesh])
    with pytest.raises(RuntimeError, match="volume_mesh needs volume or max_volume"):
        call(volume_mesh=2, object_meshes=[mesh])
    with pytest.raises(RuntimeError, match="max_volume needs candidates"):           # the table's own rules still come first
        call(volume_mesh=2, max_volume=2.0, object_meshes=[mesh])
    sig = inspect.signature(generate.generate_with_volume_mesh).parameters
    assert sig["volume_mesh"].default == 0 and generate.build_parser("ho3d").parse_args([]).volume_mesh == 0
    assert [r.only for r in generate.VOLUME_MESH_RULES] == ["cli"] * 3 and generate.RULES[-3:] == generate.VOLUME_MESH_RULES


def test_option_0_leaves_the_settings_and_the_options_as_they_were(monkeypatch):
    base = dict(volume_res=0.004, max_volume=2.0)
    assert generate._Volume.settings(types.SimpleNamespace(**base), None) == dict(res=0.004, max_volume=2.0)
    assert generate._Volume.settings(types.SimpleNamespace(**base, volume_mesh=0), None) == dict(res=0.004, max_volume=2.0)
    assert generate._Volume.settings(types.SimpleNamespace(**base, volume_mesh=2), None) == dict(res=0.004, max_volume=2.0, mesh=2)
    assert generate._Volume.keywords == ("volume_res", "max_volume") and "volume_mesh" not in inspect.signature(generate.generate_for_objects).parameters
    made, packed = [], []
    monkeypatch.setattr(generate, "plan_calls", lambda counts, rows, rows_per_call: [])
    options = generate._Options

    class Spy(options):
        def __init__(self, **fields):
            options.__init__(self, **fields)
            made.append(self)
    monkeypatch.setattr(generate, "_Options", Spy)
    net = types.SimpleNamespace(rh_mano=types.SimpleNamespace(faces=np.asarray([[0, 1, 2]])))
    objs = [torch.zeros(4, 8)]
    mesh = (np.zeros((4, 3)), np.asarray([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]]))
    generate.generate_for_objects(net, objs, 5, True, 3, [0], volume=True)
    generate.generate_with_volume_mesh(net, objs, 5, True, 3, [0], volume=True, volume_mesh=0)
    generate.generate_with_volume_mesh(net, objs, 5, True, 3, [0], volume=True, volume_mesh=2, object_meshes=[mesh])
    assert made[0] == made[1] and made[0].figures == ((generate._Volume, dict(res=0.001, max_volume=INF)),)
    assert made[2].figures == ((generate._Volume, dict(res=0.001, max_volume=INF, mesh=2)),)
    # the meshes of a call are packed when only the volume asks for them
    monkeypatch.setattr(generate, "plan_calls", lambda counts, rows, rows_per_call: [[0]])
    monkeypatch.setattr(generate, "_generate_call", lambda net, opt, objs, indices, meshes=None: packed.append(meshes) or [None])
    generate.generate_with_volume_mesh(net, objs, 5, True, 3, [0], volume=True, volume_mesh=1, object_meshes=[mesh])
    generate.generate_for_objects(net, objs, 5, True, 3, [0], volume=True, object_meshes=[mesh])
    assert isinstance(packed[0], contact.ObjectMeshes) and packed[0].n_objects == 1 and packed[1] is None


def test_option_1_takes_the_hulls_of_the_mesh_vertices(monkeypatch):
    pytest.importorskip("scipy")
    seen = {}

    def fake_volume(topo, hand, planes, plane_off, obj_of_row, R, t, res, err=None):
        seen.update(planes=planes.numpy(), plane_off=plane_off.numpy(), res=res)
        return {"count": torch.zeros(2, dtype=torch.int32), "depth": torch.zeros(2), "status": torch.zeros(2, dtype=torch.int32)}
    monkeypatch.setattr(generate, "_hand_topology", lambda net, n, dev: None)
    monkeypatch.setattr(ops, "new_err_flag", lambda dev: torch.zeros(1, dtype=torch.int32))
    monkeypatch.setattr(contact, "grasp_volume", fake_volume)
    meshes = [TORUS, CUBE]
    cloud = generate.object_tensor(np.random.default_rng(0).normal(size=(40, 3)))
    call = types.SimpleNamespace(net=None, vertices=torch.zeros(2, 5, 3), objs=[cloud, cloud], obj_of_row=torch.arange(2), frame=(None, None),
                                 meshes=contact.ObjectMeshes(meshes), indices=[7, 9])
    out = generate._Volume.launch(dict(res=0.004, max_volume=INF, mesh=1), call)
    want = contact.pack_planes([contact.hull_planes(v.astype(np.float64)) for v, _ in meshes])
    assert np.array_equal(seen["planes"], want[0]) and np.array_equal(seen["plane_off"], want[1]) and set(out) == set(generate.VOLUME_PIECES)
    assert want[1].tolist()[1] > 6 and want[1].tolist()[2] - want[1].tolist()[1] == 6             # a torus' hull, then a box's six planes
    generate._Volume.launch(dict(res=0.004, max_volume=INF), call)                   # option 0: the cloud's hull, as before
    assert np.array_equal(seen["planes"], contact.pack_planes([contact.hull_planes(cloud[:3].T.numpy().astype(np.float64))] * 2)[0])
    monkeypatch.setattr(ops, "GRASP_VOLUME_MAX_PLANES", 6)
    with pytest.raises(RuntimeError, match="object 7 has"):
        generate._Volume.launch(dict(res=0.004, max_volume=INF, mesh=1), call)
    # what the lists and the summary say under option 2: no depth, never a NaN
    lists = generate._Volume.lists(dict(res=0.004, max_volume=INF, mesh=2),
                                   [np.asarray([3, -1], np.int32), np.full(2, np.nan, np.float32), np.zeros(2, np.int32), np.zeros(1, np.int32)])
    assert lists["penetration_depth"] == [None, None] and lists["volume_voxels"] == [3, None] and lists["penetration_volume"][1] is None
    rows = [generate._Volume.rows(lists)]
    for k, against in ((2, "mesh"), (1, "mesh_hull")):
        stat, _ = generate._Volume.summary(types.SimpleNamespace(volume_res=0.004, volume_mesh=k), None, rows)
        assert stat["against"] == against and stat["mean_depth_cm"] is None and stat["grasps"] == 1 and "NaN" not in json.dumps(stat)
    stat, _ = generate._Volume.summary(types.SimpleNamespace(volume_res=0.004, volume_mesh=0), None, [[(3, 0.1, 0.5)]])
    assert set(stat) == {"res", "grasps", "mean_volume_cm3", "mean_depth_cm", "contact_ratio"} and stat["mean_depth_cm"] == 0.5


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    name = "dvq_grasp_mesh_volume"
    assert name in _lib.SIGNATURES and f"int {name}(" in header and hasattr(lib, name)
    assert name in re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    # hand V | faces F | loop_off loop_vert L n_loop | mesh_verts n_mv vert_off | mesh_faces n_mf face_off | O obj_of_row R t B h |
    # count status err | stream
    assert len(_lib.SIGNATURES[name][1]) == 24
    declared = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
    assert len(re.sub(r"/\*.*?\*/", "", declared, flags=re.S).split(",")) == 24
    assert ops.GRASP_MESH_VOLUME_LIST == 2048


def volume_args(B=1):
    v, f = sphere()
    verts, vert_off, faces, face_off = (torch.from_numpy(x) for x in ref.pack([TORUS]))
    return dict(hand=torch.from_numpy(v)[None].repeat(B, 1, 1).contiguous(), faces=torch.from_numpy(f.astype(np.int32)),
                loop_off=torch.zeros(1, dtype=torch.int32), loop_vert=torch.zeros(0, dtype=torch.int32), mesh_verts=verts, vert_off=vert_off,
                mesh_faces=faces, face_off=face_off, obj_of_row=torch.zeros(B, dtype=torch.int64))


def test_ops_refuse_bad_arguments_before_any_device_use():
    good = volume_args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_mesh_volume(**good)                                                # well-formed, but not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_mesh_volume(**good, R=torch.eye(3)[None].contiguous(), t=torch.zeros(3), res=0.004)
    hand, faces = good["hand"], good["faces"]
    for bad in (dict(hand=torch.zeros(1, 2049, 3)), dict(hand=torch.zeros(1, 0, 3)), dict(hand=hand.transpose(1, 2)), dict(hand=hand.double()),
                dict(faces=faces.long()), dict(faces=faces.reshape(-1)), dict(faces=torch.zeros(8193, 3, dtype=torch.int32)),
                dict(loop_off=torch.zeros(66, dtype=torch.int32)), dict(loop_off=torch.zeros(0, dtype=torch.int32)),
                dict(loop_vert=torch.zeros(3, dtype=torch.int64)), dict(mesh_verts=torch.zeros(7, 4)),
                dict(mesh_verts=torch.zeros(7, 3, dtype=torch.float64)), dict(mesh_verts=torch.zeros(3, 7).t()),
                dict(mesh_faces=torch.zeros(4, 3, dtype=torch.int64)), dict(mesh_faces=torch.zeros(12, dtype=torch.int32)),
                dict(vert_off=torch.zeros(2, dtype=torch.int64)), dict(face_off=torch.zeros(3, dtype=torch.int32)),
                dict(vert_off=torch.zeros(0, dtype=torch.int32), face_off=torch.zeros(0, dtype=torch.int32)),
                dict(obj_of_row=torch.zeros(1, dtype=torch.int32)), dict(obj_of_row=torch.zeros(2, dtype=torch.int64)),
                dict(R=torch.zeros(2, 3, 3)), dict(R=torch.zeros(1, 3, 3, dtype=torch.float64)), dict(t=torch.zeros(3)),   # t without R
                dict(R=torch.eye(3)[None].contiguous(), t=torch.zeros(4)),
                dict(res=0.0), dict(res=-0.001), dict(res=INF), dict(res=NAN)):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_mesh_volume(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    with pytest.raises(RuntimeError, match="ObjectMeshes"):
        contact.grasp_mesh_volume(None, [TORUS], hand, good["obj_of_row"])


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def run(hand, faces, loops, packed, obj_of_row, R=None, t=None, h=0.004, err=None):
    out = ops.grasp_mesh_volume(gpu(np.ascontiguousarray(hand, np.float32)), gpu(np.asarray(faces, np.int32)), gpu(loops[0]), gpu(loops[1]),
                                *(gpu(x) for x in packed), gpu(np.asarray(obj_of_row, np.int64)),
                                None if R is None else gpu(np.asarray(R, np.float32)), None if t is None else gpu(np.asarray(t, np.float32)),
                                h, err=err)
    B = hand.shape[0]
    assert all(tuple(o.shape) == (B,) and o.dtype == torch.int32 for o in out) and len(out) == 2
    return {"count": out[0].cpu().numpy(), "status": out[1].cpu().numpy()}


def assert_same(got, want, what=""):
    for k in ("count", "status"):
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def sphere_hands(B, tag):
    """B different hands: the sphere scaled, shifted and roughened a little (still closed)."""
    v, f = sphere()
    scale = np.linspace(0.85, 1.1, B).astype(np.float32)[:, None, None]
    shift = synth.synthetic_normal((B, 1, 3), 61, f"mesh_volume/{tag}/shift", 0.006).numpy()
    rough = synth.synthetic_normal((B, len(v), 3), 61, f"mesh_volume/{tag}/rough", 0.0003).numpy()
    return (v[None] * scale + shift + rough).astype(np.float32), f


@pytest.mark.gpu
def test_kernel_equals_the_reference_on_two_objects_and_ignores_the_batch():
    hand, f = sphere_hands(16, "plain")
    packed = ref.pack([TORUS, CUBE])
    rows = np.asarray([0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1], np.int64)
    hand[9] = hand[2]                                                                # the same grasp of the same object at two rows
    got = run(hand, f, NO_LOOPS, packed, rows)
    want = ref.grasp_mesh_volume(hand, f, *NO_LOOPS, *packed, rows, h=0.004)
    print("count", got["count"], want["count"])
    assert_same(got, want, "two objects")
    assert want["err"] == 0 and (want["status"] == 0).all() and (want["count"] > 300).all() and len(set(want["count"].tolist())) >= 12
    assert got["count"][9] == got["count"][2]
    for b in range(16):                                                              # every row alone: neither B nor the row matters
        alone = run(hand[b:b + 1], f, NO_LOOPS, packed, rows[b:b + 1])
        assert alone["count"][0] == got["count"][b] and alone["status"][0] == got["status"][b], b
    plain = run(sphere()[0][None], f, NO_LOOPS, packed, [0])                         # the figures the CPU tests pin
    assert plain["count"].tolist() == [812] and run(sphere()[0][None], f, NO_LOOPS, packed, [1])["count"].tolist() == [520]
    assert run(sphere()[0][None], f, NO_LOOPS, packed, [0], h=0.002)["count"].tolist() == [6420]
    empty = run(hand[:0], f, NO_LOOPS, packed, rows[:0])
    assert empty["count"].shape == (0,) and empty["status"].shape == (0,)


@pytest.mark.gpu
def test_kernel_in_the_rotated_rows_frame():
    base, f = sphere_hands(16, "rot")
    packed = ref.pack([TORUS, CUBE])
    rows = (np.arange(16) % 2).astype(np.int64)
    R = generate.rotation_xyz(synth.synthetic_uniform((16, 3), 62, "mesh_volume/rot/angles", 0.0, 2 * math.pi).numpy().astype(np.float64))
    t = np.asarray(generate.CANONICAL_OFFSET)
    hand = (np.einsum("bij,bvj->bvi", R, base.astype(np.float64)) + t).astype(np.float32)
    got = run(hand, f, NO_LOOPS, packed, rows, R=R, t=t)
    want = ref.grasp_mesh_volume(hand, f, *NO_LOOPS, *packed, rows, R=R.astype(np.float32), t=t.astype(np.float32), h=0.004)
    still = ref.grasp_mesh_volume(base, f, *NO_LOOPS, *packed, rows, h=0.004)
    print("count", got["count"], want["count"], still["count"])
    assert_same(got, want, "rotated")
    assert (want["status"] == 0).all() and (np.abs(want["count"] - still["count"]) <= 0.05 * still["count"]).all()   # the lattice is the object's
    for b in (0, 7):
        alone = run(hand[b:b + 1], f, NO_LOOPS, packed, rows[b:b + 1], R=R[b:b + 1], t=t)
        assert alone["count"][0] == got["count"][b]
    no_t = run(hand[:4], f, NO_LOOPS, packed, rows[:4], R=R[:4])                     # R alone: u = v
    assert_same(no_t, ref.grasp_mesh_volume(hand[:4], f, *NO_LOOPS, *packed, rows[:4], R=R[:4].astype(np.float32), h=0.004), "R alone")


@pytest.mark.gpu
def test_kernel_on_the_real_hand_sealed_at_the_wrist(tmp_path):
    from test_grasp_volume import mano_hands
    verts, faces = mano_hands(tmp_path, 4)
    topo = contact.HandTopology(faces, 778, DEV)
    sealed, loop_off, loop_vert = (x.cpu().numpy() for x in topo.sealed())
    assert sealed.shape == (1554, 3) and loop_off.tolist() == [0, 16]               # L = 1
    hand = verts.cpu().numpy()
    meshes = [ref.torus(8, 8, R=0.025, r=0.012, centre=hand[b][[95, 220, 110, 60]].mean(0)) for b in range(4)]   # about each palm
    objects = contact.ObjectMeshes(meshes)
    out = contact.grasp_mesh_volume(topo, objects, verts, gpu(np.arange(4)), res=0.004)
    assert tuple(out) == ("count", "status")
    got = {k: x.cpu().numpy() for k, x in out.items()}
    want = ref.grasp_mesh_volume(hand, sealed, loop_off, loop_vert, *ref.pack(meshes), np.arange(4), h=0.004)
    print("count", got["count"], want["count"])
    assert_same(got, want, "mano")
    assert (want["status"] == 0).all() and (want["count"] > 20).all()
    fine = contact.grasp_mesh_volume(topo, objects, verts[:1], gpu(np.arange(1)), res=0.001)     # 1 mm: many tiles, several words
    want = ref.grasp_mesh_volume(hand[:1], sealed, loop_off, loop_vert, *ref.pack(meshes), np.arange(1), h=0.001)
    assert fine["count"].cpu().tolist() == want["count"].tolist() and want["count"][0] > 2000


@pytest.mark.gpu
def test_kernel_with_more_faces_than_the_cull_list_holds_and_with_fewer():
    v, f = sphere()
    fine = score_ref.sphere_mesh(40, 40, radius=0.021)                               # 3200 faces, all inside the hand's box: the list overflows
    coarse = score_ref.sphere_mesh(20, 20, radius=0.021)                             # 800 faces: they fit
    off = np.asarray([0.0037, -0.0041, 0.0053], np.float32)
    meshes = [(fine[0] + off, fine[1]), (coarse[0] + off, coarse[1]), TORUS]
    assert len(fine[1]) > ops.GRASP_MESH_VOLUME_LIST > len(coarse[1])
    packed = ref.pack(meshes)
    hand = np.repeat(v[None], 3, axis=0)
    got = run(hand, f, NO_LOOPS, packed, [0, 1, 2])
    want = ref.grasp_mesh_volume(hand, f, *NO_LOOPS, *packed, [0, 1, 2], h=0.004)
    print("count", got["count"], want["count"])
    assert_same(got, want, "cull list")
    assert (want["status"] == 0).all() and abs(int(want["count"][0]) - int(want["count"][1])) < 0.05 * want["count"][1] and want["count"][1] > 400
    # a hand much smaller than the object: most faces are culled and the rest fit, whatever the object's size
    small = (v * np.float32(0.25) + np.asarray([0.0, 0.0, 0.018], np.float32))[None]
    assert_same(run(small, f, NO_LOOPS, packed, [0], h=0.002), ref.grasp_mesh_volume(small, f, *NO_LOOPS, *packed, [0], h=0.002), "small hand")


@pytest.mark.gpu
def test_tie_rule_on_the_device():
    (mv, mf), closed_form = tie_box()
    v, f = sphere()
    got = run(v[None], f, NO_LOOPS, ref.pack([(mv, mf)]), [0], h=TIE_H)
    assert got["count"].tolist() == [closed_form] and got["status"].tolist() == [0]
    m = mv.copy()
    m[:, 0] = np.float32(TIE_H) - m[:, 0]
    got = run(v[None], f, NO_LOOPS, ref.pack([(m, mf[:, ::-1].copy())]), [0], h=TIE_H)
    assert got["count"].tolist() == [closed_form]


@pytest.mark.gpu
def test_statuses_error_bits_far_coordinates_and_an_open_mesh():
    hand, f, meshes, rows = status_case()
    open_torus = (TORUS[0], TORUS[1][5:])                                            # five faces removed: parity undefined, (a) still says what
    meshes = meshes + [open_torus]
    packed = ref.pack(meshes)
    rows = np.concatenate([rows, [6]])
    hand = np.concatenate([hand, hand[:1]])
    want = ref.grasp_mesh_volume(hand, f, *NO_LOOPS, *packed, rows, h=0.004)
    err = ops.new_err_flag(torch.device(DEV))
    got = run(hand, f, NO_LOOPS, packed, rows, err=err)
    print(got, want)
    assert_same(got, want, "statuses")
    assert int(err.item()) == want["err"] == 2 and want["status"].tolist() == [0, 0, 0, 1, 0, 1, 3, 0, 0]
    assert want["count"][8] != want["count"][0]
    with pytest.raises(RuntimeError, match="out of bounds"):                         # without a flag of the caller's the binding raises
        run(hand[4:5], f, NO_LOOPS, packed, rows[4:5])
    fine = run(hand[:2], f, NO_LOOPS, packed, rows[:2], h=1e-5)                      # status 2
    assert fine["status"].tolist() == [2, 2] and fine["count"].tolist() == [-1, -1]
    err = ops.new_err_flag(torch.device(DEV))
    out = run(hand[:3], f, NO_LOOPS, packed, np.asarray([7, -1, 0], np.int64), err=err)          # bit 0
    assert int(err.item()) == 1 and out["status"].tolist() == [4, 4, 0] and out["count"].tolist() == [-1, -1, int(want["count"][0])]
    broken = list(packed)
    broken[3] = packed[3].copy()
    broken[3][2] = 9999
    err = ops.new_err_flag(torch.device(DEV))
    out = run(hand[:2], f, NO_LOOPS, broken, rows[:2], err=err)                      # bit 1: a face range that leaves the array
    assert int(err.item()) == 2 and out["status"].tolist() == [0, 4] and out["count"].tolist() == [int(want["count"][0]), -1]
    lib = _lib.load()                                                                # straight through the C ABI: DVQ_EINVAL, nothing launched
    one = torch.full((64,), 7.0, device=DEV)
    p = one.data_ptr()
    for V, F, L, h, B in ((2049, 4, 0, 0.004, 1), (0, 4, 0, 0.004, 1), (5, 8193, 0, 0.004, 1), (5, 4, 65, 0.004, 1), (5, 4, 0, 0.0, 1),
                          (5, 4, 0, INF, 1), (5, 4, 0, NAN, 1), (5, 4, 0, 0.004, -1)):
        assert lib.dvq_grasp_mesh_volume(p, V, p, F, p, p, L, 0, p, 1, p, p, 1, p, 1, p, None, None, B, h, p, p, p, None) == 1, (V, F, L, h, B)
    assert lib.dvq_grasp_mesh_volume(p, 5, p, 4, p, p, 0, 0, p, 1, p, p, 1, p, 1, p, None, p, 1, 0.004, p, p, p, None) == 1   # t without R
    assert lib.dvq_grasp_mesh_volume(None, 5, None, 4, None, None, 0, 0, None, 1, None, None, 1, None, 1, None, None, None, 0, 0.004, None, None,
                                     None, None) == 0                                # B = 0: no pointer is looked at
    assert (one == 7.0).all()                                                        # nothing was written


# ------------------------------------------------------------------------------------------------------ GPU: end to end
E2E_K, E2E_RES = 4, 0.004
E2E_CENTRE = np.asarray([-0.12, -0.07, 0.13])                    # where the synthetic weights put every hand (tests/test_grasp_volume.py)


def e2e_objects():
    """Two closed meshes about the place of the hands, each with a cloud sampled from its surface: (meshes, clouds [N,3] float64)."""
    meshes = [ref.torus(16, 8, 0.05, 0.02, E2E_CENTRE), ref.box((0.04, 0.03, 0.035), E2E_CENTRE + [0.01, 0.0, -0.01])]
    clouds = []
    for i, ((v, f), n) in enumerate(zip(meshes, (300, 200))):
        rng = np.random.default_rng(70 + i)
        tri = v[f[rng.integers(0, len(f), n)]].astype(np.float64)
        clouds.append(np.einsum("nk,nkc->nc", rng.dirichlet(np.ones(3), n), tri))
    return meshes, clouds


def _run_main(dataset, out_dir, extra, mano):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
def test_entry_points_count_against_the_mesh_and_against_its_hull(tmp_path):
    pytest.importorskip("scipy")
    from test_grasp_select import mano_pkl
    mano = mano_pkl(tmp_path)
    net = generate.load_model(generate.parse_args("obman", ["--checkpoint", "/nonexistent", "--mano_model", mano]), torch.device(DEV))
    meshes, clouds = e2e_objects()
    objs = [generate.object_tensor(c) for c in clouds]
    k = E2E_K
    topo = generate._hand_topology(net, 778, torch.device(DEV))
    sealed, loop_off, loop_vert = (x.cpu().numpy() for x in topo.sealed())
    plain = generate.generate_for_objects(net, objs, k, False, 3, [0, 1], volume=True, volume_res=E2E_RES)
    zero = generate.generate_with_volume_mesh(net, objs, k, False, 3, [0, 1], volume=True, volume_res=E2E_RES, volume_mesh=0, object_meshes=meshes)
    assert [json.dumps(g["json"]) for g in zero] == [json.dumps(g["json"]) for g in plain]       # option 0: the call without the keyword
    seen = {}
    for option in (2, 1):
        per_grouping = []
        for rows_per_call in (16384, 1):
            got = generate.generate_with_volume_mesh(net, objs, k, False, 3, [0, 1], rows_per_call=rows_per_call, volume=True,
                                                     volume_res=E2E_RES, volume_mesh=option, object_meshes=meshes)
            per_grouping.append([g["json"] for g in got])
        assert per_grouping[0] == per_grouping[1]                                    # the lists do not depend on the grouping
        for i, g in enumerate(got):
            hand = g["vertices"].cpu().numpy()
            j = g["json"]
            assert list(j)[-3:] == list(FIELDS) and np.array_equal(g["params"].cpu().numpy(), plain[i]["params"].cpu().numpy())
            if option == 2:
                want = ref.grasp_mesh_volume(hand, sealed, loop_off, loop_vert, *ref.pack([meshes[i]]), np.zeros(k, np.int64), h=E2E_RES)
                assert j["penetration_depth"] == [None] * k and torch.isnan(g["volume"]["depth"]).all()
            else:
                planes = contact.hull_planes(meshes[i][0].astype(np.float64))
                want = vref.grasp_volume(hand, sealed, loop_off, loop_vert, planes, [0, len(planes)], np.zeros(k, np.int64), h=E2E_RES)
                assert j["penetration_depth"] == contact.volume_stats(want["count"], want["depth"], E2E_RES)["penetration_depth"]
            assert (want["status"] == 0).all() and j["volume_voxels"] == want["count"].tolist()
            assert j["penetration_volume"] == contact.volume_stats(want["count"], np.zeros(k), E2E_RES)["penetration_volume"]
            assert np.array_equal(g["volume"]["count"].cpu().numpy(), want["count"])
            seen[option, i] = want["count"]
    print("voxels against the mesh", [seen[2, i].tolist() for i in range(2)], "against its hull", [seen[1, i].tolist() for i in range(2)],
          "against the cloud's hull", [g["json"]["volume_voxels"] for g in plain])
    assert (seen[2, 0] <= seen[1, 0]).all() and (seen[2, 0] < seen[1, 0]).any() and sum(int(c.sum()) for c in seen.values()) > 0   # the torus' hole
    assert np.array_equal(seen[2, 1], seen[1, 1])                                    # a box is its own hull
    assert all((np.asarray(g["json"]["volume_voxels"]) <= seen[1, i]).all() for i, g in enumerate(plain))   # the cloud's hull lies inside
    # the entry point: files byte-identical for every --rows_per_call, null depths, "against" in penetration.json
    files, mesh_files = [], []
    for i, (c, (v, f)) in enumerate(zip(clouds, meshes)):
        files.append(str(tmp_path / f"cloud{i}.npy"))
        np.save(files[-1], c)
        mesh_files.append(str(tmp_path / f"mesh{i}.npz"))
        np.savez(mesh_files[-1], verts=v, faces=f)
    base = ["--objects"] + files + ["--num_grasp", str(k), "--volume", "1", "--volume_res", str(E2E_RES)]
    with_mesh = base + ["--object_meshes"] + mesh_files
    for option, against in ((2, "mesh"), (1, "mesh_hull")):
        names0, bytes0 = _run_main("obman", str(tmp_path / f"a{option}"), with_mesh + ["--volume_mesh", str(option), "--rows_per_call", "0"], mano)
        names1, bytes1 = _run_main("obman", str(tmp_path / f"b{option}"), with_mesh + ["--volume_mesh", str(option), "--rows_per_call", "16384"], mano)
        assert names0 == names1 == ["obj_id_cloud0.json", "obj_id_cloud1.json"] and bytes0 == bytes1
        pen0, pen1 = (open(str(tmp_path / d / "penetration.json"), "rb").read() for d in (f"a{option}", f"b{option}"))
        assert pen0 == pen1 and b"NaN" not in pen0
        pen = json.loads(pen0)
        assert pen["against"] == against and pen["grasps"] == 2 * k and (pen["mean_depth_cm"] is None) == (option == 2)
        for i, data in enumerate(bytes0):
            j = json.loads(data)
            assert b"NaN" not in data and j["volume_voxels"] == seen[option, i].tolist()
            assert (j["penetration_depth"] == [None] * k) == (option == 2)
        assert not os.path.exists(str(tmp_path / f"a{option}" / "mesh_penetration.json"))         # the meshes without the mesh depth
    # --volume_mesh 0 reproduces the bytes of a run without the flag
    names_p, bytes_p = _run_main("obman", str(tmp_path / "plain"), base, mano)
    names_o, bytes_o = _run_main("obman", str(tmp_path / "off"), with_mesh + ["--volume_mesh", "0"], mano)
    assert names_p == names_o and bytes_p == bytes_o
    assert open(str(tmp_path / "plain" / "penetration.json"), "rb").read() == open(str(tmp_path / "off" / "penetration.json"), "rb").read()
    assert "against" not in json.loads(open(str(tmp_path / "plain" / "penetration.json")).read())
    # --max_volume compares the count, as before
    figures = generate.generate_with_volume_mesh(net, objs, 8, False, 3, [0, 1], volume=True, volume_res=E2E_RES, volume_mesh=2, object_meshes=meshes)
    counts = figures[0]["volume"]["count"].cpu().numpy()
    limit = int(np.sort(counts)[3])
    X = (limit + 0.5) * E2E_RES ** 3 * 1e6
    kept = generate.generate_with_volume_mesh(net, objs, k, False, 3, [0, 1], candidates=8, volume=True, volume_res=E2E_RES, max_volume=X,
                                              volume_mesh=2, object_meshes=meshes)
    assert np.array_equal(kept[0]["volume_scores"]["count"].cpu().numpy(), counts)
    cls, key = contact.select_keys({n: t.cpu() for n, t in kept[0]["scores"].items()}, "penetration", 1)
    order = score_ref.segment_topk(torch.maximum(cls, torch.from_numpy((counts > limit).astype(np.int32))).numpy(), key.numpy(), 1, 8, 8)[0]
    assert np.array_equal(kept[0]["candidate"].cpu().numpy(), order[:k])
