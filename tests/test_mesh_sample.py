"""Object clouds from meshes on the device: the two kernels of csrc/mesh_sample.hip (dvq_mesh_sample, dvq_cloud_fps), their host API
(ops.mesh_sample, ops.cloud_fps, contact.sample_clouds) and the ``--mesh_points`` / ``--mesh_points_even`` mode of the entry points.
The reference is tests/mesh_sample_ref.py, the header's definition in numpy: the CPU part checks the restatement itself (face counts
against the areas, points on their faces, the farthest-point order against a float64 loop), the GPU part equals it bit for bit."""
import json
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops

import mesh_sample_ref as ref

DEV = "cuda:0"
SEED, STREAM, S_BIG = 1234, 7, 65536
CHUNK = ops.MESH_SAMPLE_CHUNK


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ procedural meshes
BOX = (0.2, 0.05, 0.01)             # metres: face areas 20 : 4 : 1


def box(size=BOX, centre=(0.0, 0.0, 0.0)):
    """12 triangles, outward; faces 0-3 are the two largest sides (+-z), 4-7 the middle ones (+-y), 8-11 the smallest (+-x)."""
    v = (np.asarray([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64) * 0.5 * np.asarray(size) + np.asarray(centre))
    f = [[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]]
    return v, np.asarray(f, np.int64)


def torus(n=24, m=22, major=0.05, minor=0.02, centre=(0.0, 0.0, 0.0)):
    """n x m quads split into 2 n m triangles about the z axis (tests/test_grasp_mesh.py's): 24 x 22 gives 1 056 faces, closed."""
    u, w = np.meshgrid(2 * np.pi * np.arange(n) / n, 2 * np.pi * np.arange(m) / m, indexing="ij")
    ring = major + minor * np.cos(w)
    v = np.stack([ring * np.cos(u), ring * np.sin(u), minor * np.sin(w)], axis=-1).reshape(-1, 3) + np.asarray(centre)
    idx = lambda i, j: (i % n) * m + (j % m)
    f = []
    for i in range(n):
        for j in range(m):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [[a, b, c], [a, c, d]]
    return v, np.asarray(f, np.int64)


def one_face():
    return np.asarray([[0.0, 0.0, 0.0], [0.03, 0.0, 0.01], [0.0, 0.02, 0.0]]), np.asarray([[0, 1, 2]], np.int64)


def flat():
    """Three faces without area: two on a line, one on a point."""
    v = np.asarray([[0.0, 0.0, 0.0], [0.01, 0.01, 0.01], [0.02, 0.02, 0.02], [0.5, 0.5, 0.5]])
    return v, np.asarray([[0, 1, 2], [2, 1, 0], [3, 3, 3]], np.int64)


def pool_of_four():
    objs = [box(), one_face(), torus(), flat()]
    assert [len(f) for _, f in objs] == [12, 1, CHUNK + 32, 3]
    return objs


def areas64(verts, faces):
    tri = np.asarray(verts, np.float32).astype(np.float64)[faces]
    return 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)


_BIG = {}


def big_sample():
    """The box under (SEED, STREAM), S_BIG samples: computed once."""
    if not _BIG:
        _BIG["out"] = ref.mesh_sample([box()], S_BIG, SEED, [STREAM])
    return _BIG["out"]


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_mesh_points_flags(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.mesh_points, a.mesh_points_even) == (0, 1)
    meshes = ["--object_meshes", "box.npz", "torus.obj"]
    a = generate.parse_args(dataset, meshes + ["--mesh_points", "256", "--mesh_points_even", "4"])
    assert (a.mesh_points, a.mesh_points_even, a.objects, a.object_meshes) == (256, 4, [], ["box.npz", "torus.obj"])
    assert generate.parse_args(dataset, meshes + ["--mesh_points", "3000"]).mesh_points_even == 1
    assert generate.parse_args(dataset, meshes + ["--mesh_points", "4096", "--mesh_points_even", "4"]).mesh_points == 4096      # N * F = 16 384
    assert generate.parse_args(dataset, meshes + ["--mesh_points", "100000"]).mesh_points == 100000                            # F = 1: no pool
    assert generate.parse_args(dataset, meshes + ["--mesh_points", "256", "--mesh_depth", "1"]).mesh_depth == 1              # one copy of the meshes
    for bad in (["--mesh_points", "256"],                                                                 # no meshes
                ["--objects", "a.npy", "b.npy"] + meshes + ["--mesh_points", "256"],                      # clouds given as well
                meshes + ["--mesh_points", "4097", "--mesh_points_even", "4"],                            # the pool of the even mode
                meshes + ["--mesh_points", "-1"], meshes + ["--mesh_points", str(2 ** 20 + 1)],
                meshes + ["--mesh_points", "256", "--mesh_points_even", "0"],
                meshes + ["--mesh_points_even", "4"], ["--mesh_points_even", "2"],                        # even without mesh_points
                meshes):                                                                                  # as before: one mesh per --objects file
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_the_old_rule_keeps_its_text(capsys):
    with pytest.raises(SystemExit):
        generate.parse_args("ho3d", ["--objects", "a.npy", "--object_meshes", "a.obj", "b.obj"])
    assert "--object_meshes needs one mesh per --objects file, in the same order" in capsys.readouterr().err


def test_abi_declares_and_exports_the_entry_points():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    added = re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    for name, n_args in (("dvq_mesh_sample", 16), ("dvq_cloud_fps", 8)):
        assert name in _lib.SIGNATURES and f"int {name}(" in header and hasattr(lib, name) and name in added
        assert len(_lib.SIGNATURES[name][1]) == n_args
        declared = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", declared, flags=re.S).split(",")) == n_args
    assert lib.dvq_abi_version() == 10
    assert "mesh_sample.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    source = open(os.path.join(_lib.CSRC, "mesh_sample.hip")).read()
    assert "__syncthreads" not in source and source.count("dvq_lds_barrier()") >= 3      # every barrier goes through the one helper
    assert (ops.MESH_SAMPLE_MAX_S, ops.CLOUD_FPS_MAX_P) == (2 ** 20, 16384)
    assert "#define DVQ_MESH_SAMPLE_MAX_S 1048576" in header and "#define DVQ_CLOUD_FPS_MAX_P 16384" in header


def sample_args(O=2):
    m = contact.ObjectMeshes([box(), torus()][:O])
    return dict(verts=torch.from_numpy(m.verts), vert_off=torch.from_numpy(m.vert_off), faces=torch.from_numpy(m.faces),
                face_off=torch.from_numpy(m.face_off), n_samples=16, seed=SEED, stream_ids=torch.arange(O, dtype=torch.int64))


def test_ops_refuse_bad_arguments_before_any_device_use():
    good = sample_args()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_sample(**good)                                                      # well-formed, but not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mesh_sample(**good, err=torch.zeros(1, dtype=torch.int32))
    for bad in (dict(verts=good["verts"].double()), dict(verts=good["verts"].reshape(-1)), dict(verts=None),
                dict(faces=good["faces"].long()), dict(faces=good["faces"].reshape(-1)), dict(vert_off=good["vert_off"].long()),
                dict(face_off=good["face_off"][:2]), dict(vert_off=torch.zeros(0, dtype=torch.int32)),
                dict(n_samples=0), dict(n_samples=2 ** 20 + 1), dict(stream_ids=torch.arange(2, dtype=torch.int32)),
                dict(stream_ids=torch.arange(3, dtype=torch.int64)), dict(stream_ids=[0, 1]), dict(err=torch.zeros(1)),
                dict(err=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(RuntimeError) as e:
            ops.mesh_sample(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    pts = torch.zeros(2, 100, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cloud_fps(pts, 10)
    for p, keep in ((pts, 0), (pts, 101), (pts.double(), 10), (pts[:, :, :2], 10), (pts.reshape(200, 3), 10), (pts.transpose(0, 1), 10),
                    (torch.zeros(1, 16385, 3), 10), (torch.zeros(1, 0, 3), 1), (None, 1)):
        with pytest.raises(RuntimeError) as e:
            ops.cloud_fps(p, keep)
        assert "no CPU fallback" not in str(e.value), (None if p is None else tuple(p.shape), keep)
    with pytest.raises(RuntimeError, match="ObjectMeshes"):
        contact.sample_clouds([box()], 16, SEED, [0])
    m = contact.ObjectMeshes([box(), torus()])
    for n, even, ids in ((16, 1, [0]), (0, 1, [0, 1]), (16, 0, [0, 1]), (4097, 4, [0, 1])):
        with pytest.raises(RuntimeError, match="sample_clouds") as e:
            contact.sample_clouds(m, n, SEED, ids, even=even, device="cpu")
        assert "no CPU fallback" not in str(e.value)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        contact.sample_clouds(m, 16, SEED, [0, 1], even=2, device="cpu")


# ------------------------------------------------------------------------------------------------------ CPU: the restatement itself
def test_face_counts_follow_the_areas():
    v, f = box()
    points, face, status, cdf, err = big_sample()
    assert status.tolist() == [0] and err == 0 and cdf.dtype == np.uint64 and len(cdf) == 12 and (np.diff(cdf.astype(np.int64)) > 0).all()
    area = areas64(v, f)
    share = area / area.sum()
    assert np.allclose(share * 50, np.repeat([10.0, 2.0, 0.5], 4), rtol=1e-6)                      # 20 : 4 : 1, two triangles a side
    count = np.bincount(face[0], minlength=12)
    sigma = np.abs(count - S_BIG * share) / np.sqrt(S_BIG * share * (1 - share))
    print("per-face counts", count.tolist(), "deviations in binomial sigmas", np.round(sigma, 2).tolist())
    assert count.sum() == S_BIG and sigma.max() <= 5.0


def test_points_lie_on_their_faces_and_inside_the_box():
    v, f = box()
    points, face, _, _, _ = big_sample()
    v32 = np.asarray(v, np.float32).astype(np.float64)
    p, tri = points[0].astype(np.float64), v32[f[face[0]]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    off = np.abs(np.einsum("nc,nc->n", n, p - tri[:, 0])) / np.linalg.norm(n, axis=1)
    # p = (a + r1 e1) + r2 e2: two products and two sums, each rounded by at most 2^-24 of a magnitude of at most 0.2 m (the box's
    # longest side; r1, r2 <= 1, r1 + r2 <= 1 + 2^-24), and e1, e2 themselves rounded once: six roundings in all
    bound = 6 * 2.0 ** -24 * 0.2
    out = np.maximum(v32.min(0) - p, p - v32.max(0)).max()
    print(f"largest distance to the face's plane {off.max():.3e} m, largest excursion out of the box {out:.3e} m, bound {bound:.3e} m")
    assert off.max() <= bound and out <= bound
    lam = np.linalg.solve(np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], n], axis=2), (p - tri[:, 0])[:, :, None])[:, :2, 0]
    assert lam.min() >= -1e-6 and lam.sum(1).max() <= 1 + 1e-6                                        # inside the triangle, not only its plane
    assert np.isfinite(points).all() and (points[0].std(0) > np.asarray(BOX) * 0.2).all()             # spread over the whole box


def test_a_face_without_area_is_never_drawn():
    v, f = box()
    f2 = np.concatenate([f[:5], [[0, 0, 1], [2, 2, 2]], f[5:]])                                       # two faces without area in the middle
    points, face, status, cdf, err = ref.mesh_sample([(v, f2)], 20000, SEED, [STREAM])
    assert status.tolist() == [0] and err == 0 and cdf[5] == cdf[4] == cdf[6] and set(face[0].tolist()) == set(range(14)) - {5, 6}
    # the same draws land on the same triangles as without the two faces
    _, face0, _, _, _ = ref.mesh_sample([(v, f)], 20000, SEED, [STREAM])
    assert np.array_equal(np.where(face[0] > 6, face[0] - 2, face[0]), face0[0])
    # an index out of range: weight 0, never drawn, err bit 1; no face with area at all: status 1, NaN, -1
    f3 = f.copy()
    f3[2] = [4, 5, 8]
    _, face3, status3, cdf3, err3 = ref.mesh_sample([(v, f3)], 5000, SEED, [STREAM])
    assert err3 == 2 and status3.tolist() == [0] and 2 not in face3[0] and cdf3[2] == cdf3[1]
    p4, face4, status4, cdf4, err4 = ref.mesh_sample([flat()], 7, SEED, [STREAM])
    assert status4.tolist() == [1] and err4 == 0 and np.isnan(p4).all() and (face4 == -1).all() and (cdf4 == 0).all()
    _, _, status5, _, err5 = ref.mesh_sample([box()], 7, SEED, [2 ** 32])
    assert status5.tolist() == [4] and err5 == 1


def test_the_largest_face_weighs_2_to_the_20():
    for verts, faces in pool_of_four()[:3]:
        cdf, bad = ref.face_cdf(verts, faces)
        q = np.diff(np.concatenate([[0], cdf.astype(np.int64)]))
        assert not bad and q.max() == 2 ** 20 and q.min() >= 1


def fps_pool():
    return big_sample()[0][0, :4096]


_FPS = {}


def fps_case():
    if not _FPS:
        _FPS["out"] = ref.cloud_fps(fps_pool(), 1024)
    return _FPS["out"]


def test_fps_picks_are_distinct_and_the_gaps_fall():
    p = fps_pool()
    sel, gap, status = fps_case()
    assert status == 0 and sel[0] == 0 and gap[0] == -1.0 and len(set(sel.tolist())) == 1024
    assert (np.diff(gap[1:]) <= 0).all() and gap[1:].min() > 0
    kept = p[sel]
    closest = min(np.delete(ref.dist2(kept, kept[i]), i).min() for i in range(len(kept)))
    assert bits(gap[1:].min()) == bits(closest)                                                       # the kept set's smallest pairwise distance
    cover = max(ref.dist2(kept, q).min() for q in p[::16])
    print(f"1024 of 4096: smallest separation {np.sqrt(gap[1:].min()) * 1e3:.2f} mm, the first 1024 samples "
          f"{np.sqrt(min(np.delete(ref.dist2(p[:1024], p[i]), i).min() for i in range(1024))) * 1e3:.3f} mm; covering radius about "
          f"{np.sqrt(cover) * 1e3:.2f} mm")


def test_fps_matches_a_float64_greedy_loop():
    p = fps_pool().astype(np.float64)
    sel, gap, _ = fps_case()
    mind = ((p - p[0]) ** 2).sum(1)
    mind[0] = -1.0
    for r in range(1, 1024):
        i = int(np.argmax(mind))
        assert i == sel[r], (r, i, sel[r])
        assert abs(mind[i] - gap[r]) <= 8 * 2.0 ** -24 * mind[i]              # three differences, three squares, two sums: under eight roundings
        mind = np.minimum(mind, ((p - p[i]) ** 2).sum(1))
        mind[sel[:r + 1]] = -1.0


def test_fps_edge_rules():
    p = np.random.default_rng(5).normal(0, 0.05, (40, 3)).astype(np.float32)
    p[7], p[30], p[31] = p[3], p[3], p[12]                                                            # exact duplicates
    sel, gap, status = ref.cloud_fps(p, 40)
    assert status == 0 and sorted(sel.tolist()) == list(range(40))
    zero = gap == 0
    assert zero.sum() == 3 and zero[-3:].all() and sel[-3:].tolist() == sorted(sel[-3:].tolist())      # last, in position order
    sel1, gap1, _ = ref.cloud_fps(p, 1)
    assert sel1.tolist() == [0] and gap1.tolist() == [-1.0]
    bad = p.copy()
    bad[11, 2] = np.inf
    sel, gap, status = ref.cloud_fps(bad, 5)
    assert status == 1 and sel.tolist() == [-1] * 5 and gap.tolist() == [-1.0] * 5


def assert_sample_equal(got, want, what=""):
    names = ("points", "face", "status", "cdf")
    for k, a, b in zip(names, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == np.float32:
            assert np.array_equal(np.isnan(a), np.isnan(b)), (what, k)
            a, b = bits(np.nan_to_num(a, nan=0.0)), bits(np.nan_to_num(b, nan=0.0))
        assert np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5].tolist())


def test_grouping_changes_no_byte():
    objs, ids = pool_of_four(), [7, 2 ** 32 - 1, 0, 3]
    together = ref.mesh_sample(objs, 300, SEED, ids)
    assert together[2].tolist() == [0, 0, 0, 1] and together[4] == 0
    off = np.concatenate([[0], np.cumsum([len(f) for _, f in objs])])
    for o, (obj, sid) in enumerate(zip(objs, ids)):
        alone = ref.mesh_sample([obj], 300, SEED, [sid])
        assert_sample_equal(alone[:4], (together[0][o:o + 1], together[1][o:o + 1], together[2][o:o + 1], together[3][off[o]:off[o + 1]]), o)
    longer = ref.mesh_sample(objs, 301, SEED, ids)                                                    # nor does S
    assert_sample_equal((longer[0][:, :300], longer[1][:, :300]), together[:2])
    other = ref.mesh_sample(objs[:1], 300, SEED, [8])
    assert not np.array_equal(other[1], together[1][:1])                                              # the stream id is the key


# ------------------------------------------------------------------------------------------------------ GPU: bit for bit
def pack(meshes):
    vs = [np.asarray(v, np.float32).reshape(-1, 3) for v, _ in meshes]
    fs = [np.asarray(f, np.int32).reshape(-1, 3) for _, f in meshes]
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
    return np.concatenate(vs), off(vs), np.concatenate(fs), off(fs)


def run_sample(meshes, S, seed, ids, err=None):
    v, ov, f, of = (torch.as_tensor(x, device=DEV) for x in pack(meshes))
    out = ops.mesh_sample(v, ov, f, of, S, seed, torch.as_tensor(np.asarray(ids, np.int64), device=DEV), err=err)
    torch.cuda.synchronize()
    points, face, status, cdf = (x.cpu().numpy() for x in out)
    return points, face, status, cdf.view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 255, 256, 257, 3000])
def test_mesh_sample_matches_the_definition(S):
    objs, ids = pool_of_four(), [7, 2 ** 32 - 1, 0, 3]
    want = ref.mesh_sample(objs, S, SEED, ids)
    assert want[2].tolist() == [0, 0, 0, 1]
    err = ops.new_err_flag(torch.device(DEV))
    got = run_sample(objs, S, SEED, ids, err=err)
    assert int(err.item()) == 0
    assert_sample_equal(got, want[:4], S)
    if S == 3000:                                                                                     # the same objects one per call
        off = np.concatenate([[0], np.cumsum([len(f) for _, f in objs])])
        for o, (obj, sid) in enumerate(zip(objs, ids)):
            alone = run_sample([obj], S, SEED, [sid], err=err)
            assert_sample_equal(alone, (got[0][o:o + 1], got[1][o:o + 1], got[2][o:o + 1], got[3][off[o]:off[o + 1]]), o)
        assert int(err.item()) == 0
        seed2 = (5 << 32) | 9                                                                         # both halves of the key
        assert_sample_equal(run_sample(objs[:3], 64, seed2, ids[:3]), ref.mesh_sample(objs[:3], 64, seed2, ids[:3])[:4], "seed")


@pytest.mark.gpu
def test_a_bad_face_index_sets_the_flag_and_is_never_drawn():
    v, f = torus()
    f = f.copy()
    f[[3, CHUNK - 1, CHUNK + 5]] = [[0, 1, len(v)], [-1, 2, 3], [5, 2 ** 31 - 1, 6]]
    objs = [box(), (v, f)]
    want = ref.mesh_sample(objs, 3000, SEED, [1, 2])
    assert want[4] == 2 and want[2].tolist() == [0, 0]
    err = ops.new_err_flag(torch.device(DEV))
    got = run_sample(objs, 3000, SEED, [1, 2], err=err)
    assert int(err.item()) == 2
    assert_sample_equal(got, want[:4])
    assert not set(got[1][1].tolist()) & {3, CHUNK - 1, CHUNK + 5}
    with pytest.raises(RuntimeError, match="face index"):
        run_sample(objs, 16, SEED, [1, 2])
    # a stream id that is no 32-bit key: bit 0, status 4, nothing sampled, the neighbour untouched
    err.zero_()
    got = run_sample([box(), box()], 16, SEED, [2 ** 32, 5], err=err)
    want = ref.mesh_sample([box(), box()], 16, SEED, [2 ** 32, 5])
    assert int(err.item()) == 1 == want[4] and got[2].tolist() == [4, 0]
    assert_sample_equal(got, want[:4])


def fps_points(P, seed):
    return np.random.default_rng(seed).normal(0.0, 0.05, (P, 3)).astype(np.float32)


_FPS_REF = {}


def fps_ref(P, o, keep):
    """The reference of pool ``o`` of size P at the largest keep of the test, once: a smaller keep is its prefix (the order is greedy)."""
    if (P, o) not in _FPS_REF:
        _FPS_REF[P, o] = ref.cloud_fps(fps_points(P, 100 * o + P % 97), min(P, 1024 if P == 16384 else P))
    sel, gap, status = _FPS_REF[P, o]
    return sel[:keep], gap[:keep], status


def run_fps(pools, keep):
    out = ops.cloud_fps(torch.as_tensor(np.stack(pools), device=DEV), keep)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2, 1023, 1024, 1025, 16384])
def test_cloud_fps_matches_the_definition(P):
    pools = [fps_points(P, 100 * o + P % 97) for o in range(2)]                                       # two workgroups
    for keep in sorted({1, min(64, P), min(P, 1024 if P == 16384 else P)}):
        sel, gap, status = run_fps(pools, keep)
        assert sel.dtype == np.int32 and gap.dtype == np.float32 and status.tolist() == [0, 0]
        for o in range(2):
            want_sel, want_gap, _ = fps_ref(P, o, keep)
            assert np.array_equal(sel[o], want_sel), (P, keep, o, np.argwhere(sel[o] != want_sel)[:3].tolist())
            assert np.array_equal(bits(gap[o]), bits(want_gap)), (P, keep, o)


@pytest.mark.gpu
def test_cloud_fps_duplicates_and_a_pool_that_is_not_finite():
    p = fps_points(1100, 3)
    p[7], p[1030], p[1031], p[0] = p[3], p[3], p[12], p[1099]                                         # duplicates across the slots, and of pick 0
    sel, gap, status = run_fps([p], 1100)
    want_sel, want_gap, _ = ref.cloud_fps(p, 1100)
    assert status.tolist() == [0] and np.array_equal(sel[0], want_sel) and np.array_equal(bits(gap[0]), bits(want_gap))
    assert (gap[0][-4:] == 0).all() and (gap[0][1:-4] > 0).all() and sel[0][-4:].tolist() == sorted(sel[0][-4:].tolist())
    good = fps_points(1100, 4)
    for value, at in ((np.nan, (1050, 1)), (np.inf, (0, 0)), (-np.inf, (1099, 2))):
        bad = good.copy()
        bad[at] = value
        sel, gap, status = run_fps([good, bad, good], 64)
        want = ref.cloud_fps(good, 64)
        assert status.tolist() == [0, 1, 0] and (sel[1] == -1).all() and (gap[1] == -1.0).all()
        for o in (0, 2):
            assert np.array_equal(sel[o], want[0]) and np.array_equal(bits(gap[o]), bits(want[1]))


@pytest.mark.gpu
def test_sample_clouds_is_the_two_kernels_in_a_row():
    objs = [box(), torus()]
    meshes = contact.ObjectMeshes(objs)
    points, face = contact.sample_clouds(meshes, 256, SEED, [4, 9], even=4, device=DEV)
    pool = ref.mesh_sample(objs, 1024, SEED, [4, 9])
    for o in range(2):
        sel, _, _ = ref.cloud_fps(pool[0][o], 256)
        assert np.array_equal(bits(points[o].cpu().numpy()), bits(pool[0][o][sel])) and np.array_equal(face[o].cpu().numpy(), pool[1][o][sel])
    plain, plain_face = contact.sample_clouds(meshes, 256, SEED, [4, 9], device=DEV)
    assert np.array_equal(bits(plain.cpu().numpy()), bits(pool[0][:, :256])) and np.array_equal(plain_face.cpu().numpy(), pool[1][:, :256])
    with pytest.raises(RuntimeError, match="object 1 .global index 9"):
        contact.sample_clouds(contact.ObjectMeshes([box(), flat()]), 16, SEED, [4, 9], device=DEV)


E2E_CENTRE = np.asarray([-0.12, -0.07, 0.13])                    # where the synthetic weights put every hand (tests/test_grasp_volume.py)


@pytest.mark.gpu
@pytest.mark.parametrize("rows_per_call", [0, 16384])
def test_entry_point_builds_its_clouds_from_the_meshes(tmp_path, rows_per_call):
    from test_grasp_select import mano_pkl
    mano = mano_pkl(tmp_path)
    objs = [box((0.08, 0.05, 0.03), E2E_CENTRE), torus(24, 22, 0.04, 0.018, E2E_CENTRE + [0.01, 0.0, -0.01])]
    mesh_files = [str(tmp_path / "box.npz"), str(tmp_path / "torus.npz")]
    for path, (v, f) in zip(mesh_files, objs):
        np.savez(path, verts=v, faces=f)
    common = ["--num_grasp", "4", "--object_contact", "1", "--rows_per_call", str(rows_per_call), "--seed", "3", "--checkpoint", "/nonexistent",
              "--mano_model", mano]
    dir_a, dir_b = str(tmp_path / "a"), str(tmp_path / "b")
    paths_a = generate.main("obman", ["--object_meshes"] + mesh_files + ["--mesh_points", "256", "--mesh_points_even", "4", "--out_dir", dir_a] + common)
    assert [os.path.basename(p) for p in paths_a] == ["obj_id_box.json", "obj_id_torus.json"]
    cloud_files = [os.path.join(dir_a, f"obj_cloud_{name}.npy") for name in ("box", "torus")]
    want, _ = contact.sample_clouds(contact.ObjectMeshes([contact.load_mesh(p) for p in mesh_files]), 256, 3, [0, 1], even=4, device=DEV)
    for o, path in enumerate(cloud_files):
        cloud = np.load(path)
        assert cloud.dtype == np.float32 and cloud.shape == (256, 3) and np.array_equal(bits(cloud), bits(want[o].cpu().numpy()))
    paths_b = generate.main("obman", ["--objects"] + cloud_files + ["--out_dir", dir_b] + common)
    assert [os.path.basename(p) for p in paths_b] == ["obj_id_obj_cloud_box.json", "obj_id_obj_cloud_torus.json"]
    for a, b in zip(paths_a, paths_b):
        data = open(a, "rb").read()
        assert data == open(b, "rb").read()
        j = json.loads(data)
        assert len(j["object_contact_map"]) == 256 and len(j["recon_params"]) == 4
    assert open(os.path.join(dir_a, "object_contact.json"), "rb").read() == open(os.path.join(dir_b, "object_contact.json"), "rb").read()
    assert not os.path.exists(os.path.join(dir_b, "obj_cloud_box.npy"))                               # without the flag nothing new is written
