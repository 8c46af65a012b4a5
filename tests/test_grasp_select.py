"""Best-of-M grasp selection: the fused per-grasp scores (dvq_grasp_scores), the per-object top-k (dvq_segment_topk), their host
API and the ``candidates`` mode of generate_for_objects / the entry points.  The reference is tests/grasp_score_ref.py (numpy over
oracle/contact_oracle.py plus the canonical reduction and total order); GPU results are compared with it bit for bit."""
import json
import lzma
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops, synth

import grasp_score_ref as ref

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
NAN = float("nan")


def mano_pkl(tmp_path):
    """tests/golden/g9_mano_right.pkl.xz unpacked: the path of a MANO_RIGHT.pkl (real topology: 778 vertices, 1538 faces)."""
    path = str(tmp_path / "MANO_RIGHT.pkl")
    if not os.path.exists(path):
        with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
    return path


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_selection_flags(dataset):
    a = generate.build_parser(dataset).parse_args([])
    assert (a.candidates, a.select_by, a.min_contact) == (0, "penetration", 1)
    a = generate.parse_args(dataset, [])
    assert (a.candidates, a.select_by, a.min_contact) == (0, "penetration", 1)
    a = generate.parse_args(dataset, ["--candidates", "400", "--select_by", "log_prob", "--min_contact", "5", "--num_grasp", "100"])
    assert (a.candidates, a.select_by, a.min_contact, a.num_grasp) == (400, "log_prob", 5, 100)
    assert generate.parse_args(dataset, ["--candidates", "7", "--num_grasp", "7"]).candidates == 7
    with pytest.raises(SystemExit):
        generate.build_parser(dataset).parse_args(["--select_by", "volume"])


@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_refuses_fewer_candidates_than_grasps(dataset):
    with pytest.raises(SystemExit):
        generate.parse_args(dataset, ["--candidates", "3", "--num_grasp", "4"])
    with pytest.raises(SystemExit):
        generate.parse_args(dataset, ["--candidates", "-1"])
    if generate.DATASETS[dataset]["num_grasp"] > 1:                 # against the dataset's own default count
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, ["--candidates", str(generate.DATASETS[dataset]["num_grasp"] - 1)])


def test_abi_declares_and_exports_both_entry_points():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    for name in ("dvq_grasp_scores", "dvq_segment_topk"):
        assert name in _lib.SIGNATURES
        assert f"int {name}(" in header
        assert hasattr(lib, name)
    added = re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert "dvq_grasp_scores" in added and "dvq_segment_topk" in added


def test_ops_refuse_bad_arguments_before_any_device_use():
    v, f = ref.sphere_mesh(4, 6)
    faces, off, vf = (torch.from_numpy(a) for a in contact.face_csr(f, len(v)))
    hand = torch.from_numpy(v)[None].contiguous()
    obj = torch.zeros(1, 5, 3)
    good = dict(hand=hand, faces=faces, vf_off=off, vf_face=vf, obj=obj)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_scores(**good)                                                     # well-formed, but not on a device
    for bad in (dict(hand=hand.double()), dict(obj=obj.double()), dict(faces=faces.long()), dict(vf_off=off[:-1]),
                dict(vf_face=vf[:-3]), dict(hand=hand[0]), dict(hand=hand.transpose(1, 2)), dict(obj=torch.zeros(2, 5, 3)),
                dict(obj=torch.zeros(1, 5, 4)), dict(obj=torch.zeros(1, 0, 3)), dict(hand=torch.zeros(1, 0, 3), vf_off=off[:1]),
                dict(hand=torch.zeros(1, 2049, 3), vf_off=torch.zeros(2050, dtype=torch.int32)),
                dict(hand=hand.expand(2, -1, -1), obj=torch.zeros(2, 5, 3)), dict(faces=faces.reshape(-1))):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_scores(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    cls, key = torch.zeros(6, dtype=torch.int32), torch.zeros(6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.segment_topk(cls, key, 2, 3, 2)
    for args in ((cls.long(), key, 2, 3, 2), (cls, key.double(), 2, 3, 2), (cls, key, 2, 3, 0), (cls, key, 2, 3, 4), (cls, key, 3, 3, 1),
                 (cls, key, -1, 3, 1), (cls.reshape(2, 3), key.reshape(2, 3), 2, 3, 1), (cls[::2], key[::2], 1, 3, 1),
                 (torch.zeros(4097, dtype=torch.int32), torch.zeros(4097), 1, 4097, 1)):
        with pytest.raises(RuntimeError) as e:
            ops.segment_topk(*args)
        assert "no CPU fallback" not in str(e.value)


# ------------------------------------------------------------------------------------------------------ CPU: the reference itself
def test_reference_scores_on_the_closed_sphere():
    v, f = ref.sphere_mesh()
    hand = np.repeat(v[None], 3, axis=0)
    pts = v[::7]
    obj = np.stack([0.5 * pts, 1.5 * pts, 0.5 * pts]).astype(np.float32)
    obj[2, 11, 1] = np.nan
    N = pts.shape[0]
    pen, n_in, n_ct = ref.grasp_scores(hand, f, obj)
    assert n_in[0] == N and pen[0] > 0                                  # every point at half the radius is inside
    assert n_in[1] == 0 and bits(pen[1]) == 0                           # none at 1.5 r: the sum is +0.0
    assert np.isnan(pen[2]) and n_in[2] == N - 1                        # one NaN coordinate: NaN penetration
    assert n_ct[0] == 0 and n_ct[1] == 0                                # 2.5 cm from the surface: beyond the 2 cm contact region
    assert ref.grasp_scores(hand, f, obj, contact_threshold=0.03 ** 2)[2].tolist() == [N, N, N - 1]
    d, inside, term = ref.point_terms(hand[:1], f, obj[:1])
    exact = float(term[0].astype(np.float64).sum())
    assert abs(float(pen[0]) - exact) <= 1e-6 * exact                   # the tree sum against a float64 sum
    rng = np.random.default_rng(0)                                      # ... and on 3000 terms spread over four decades
    terms = (10.0 ** rng.uniform(-6, -2, size=3000)).astype(np.float32)
    exact = float(terms.astype(np.float64).sum())
    assert abs(float(ref.tree_sum(terms)) - exact) <= 1e-6 * exact
    assert bits(ref.tree_sum(np.zeros(5, np.float32))) == 0 and ref.tree_sum(np.asarray([1.5], np.float32)) == 1.5


def test_select_keys_and_the_reference_order():
    scores = {"penetration": torch.tensor([0.5, 0.0, NAN, 0.25, 0.25, 0.0, 1.0, -0.0]),
              "n_interior": torch.zeros(8, dtype=torch.int32),
              "n_contact": torch.tensor([3, 0, 9, 2, 2, 1, 7, 4], dtype=torch.int32)}
    cls, key = contact.select_keys(scores, "penetration", 1)
    assert cls.dtype == torch.int32 and key.dtype == torch.float32
    assert cls.tolist() == [0, 1, 2, 0, 0, 0, 0, 0]
    order = ref.segment_topk(cls.numpy(), key.numpy(), 1, 8, 8)[0].tolist()
    # +0.0 (5) and -0.0 (7) tie: the lower index first; 0.25 twice: 3 before 4; the hand that touches nothing (1) after every
    # touching one although it penetrates least; NaN (2) last
    assert order == [5, 7, 3, 4, 0, 6, 1, 2]
    assert sorted(order) == list(range(8))                              # keep == M: a permutation
    assert ref.segment_topk(cls.numpy(), key.numpy(), 1, 8, 3)[0].tolist() == order[:3]
    cls3, _ = contact.select_keys(scores, "penetration", 3)             # min_contact = 3: candidates 3, 4, 5 drop a class
    assert cls3.tolist() == [0, 1, 2, 1, 1, 1, 0, 0]
    assert ref.segment_topk(cls3.numpy(), key.numpy(), 1, 8, 8)[0].tolist() == [7, 0, 6, 1, 5, 3, 4, 2]
    lp = torch.tensor([-3.0, -1.0, NAN, -1.0, -7.5, float("-inf")])
    cls, key = contact.select_keys({}, "log_prob", 1, log_prob=lp)
    assert cls.tolist() == [0, 0, 2, 0, 0, 0]
    assert ref.segment_topk(cls.numpy(), key.numpy(), 1, 6, 6)[0].tolist() == [1, 3, 0, 4, 5, 2]    # likeliest first, NaN last
    two = ref.segment_topk(np.asarray([0, 0, 1, 0]), np.asarray([2.0, 1.0, 0.0, 1.0], np.float32), 2, 2, 2)   # two objects of two
    assert two.tolist() == [[1, 0], [1, 0]]
    with pytest.raises(RuntimeError):
        contact.select_keys(scores, "log_prob", 1)
    with pytest.raises(RuntimeError):
        contact.select_keys(scores, "volume", 1)


def test_generate_for_objects_refuses_bad_candidate_counts():
    with pytest.raises(RuntimeError, match="candidates"):
        generate.generate_for_objects(None, [torch.zeros(4, 8)], 5, True, 0, [0], candidates=3)


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def mano_faces(tmp_path):
    from dvqvae_amd import mano as dmano
    arrays = dmano.read_mano_pkl(mano_pkl(tmp_path))
    return arrays["faces"], np.asarray(arrays["v_template"], np.float32)


def score_case(name, tmp_path):
    """(hand [B,V,3], faces, obj [B,N,3]) numpy fp32."""
    rng = lambda tag, shape, scale: synth.synthetic_normal(shape, 31, f"scores/{name}/{tag}", scale).numpy()
    if name == "1x1x1":
        return rng("h", (1, 1, 3), 0.1), np.zeros((1, 3), np.int64), rng("o", (1, 1, 3), 0.1)      # one vertex, one degenerate face
    if name in ("3x300x776", "5x257x776"):
        B, N = (3, 300) if name == "3x300x776" else (5, 257)
        v, f = ref.sphere_mesh()
        scale = np.linspace(0.8, 1.2, B).astype(np.float32)[:, None, None]
        hand = (v[None] * scale + rng("h", (B, len(v), 3), 0.002)).astype(np.float32)
        return hand, f, rng("o", (B, N, 3), 0.04)                                                    # points on both sides of the surface
    f, v = mano_faces(tmp_path)
    if name == "2x1024x778":
        return rng("h", (2, 778, 3), 0.05), f, rng("o", (2, 1024, 3), 0.05)                          # arbitrary vertices on the MANO topology
    assert name == "2x3000x778"
    hand = (v[None] + rng("h", (2, 778, 3), 0.001)).astype(np.float32)                               # the MANO template itself
    centre = v.mean(0, keepdims=True)[None]
    return hand, f, (centre + rng("o", (2, 3000, 3), 0.03)).astype(np.float32)


def run_scores(hand, faces, obj_dev, thr=0.02 ** 2):
    topo = contact.HandTopology(faces, hand.shape[1], DEV)
    out = contact.grasp_scores(topo, gpu(hand), obj_dev, thr)
    assert set(out) == {"penetration", "n_interior", "n_contact"}
    assert out["penetration"].dtype == torch.float32 and out["n_interior"].dtype == torch.int32 and out["n_contact"].dtype == torch.int32
    return topo, {k: v.cpu().numpy() for k, v in out.items()}


def assert_scores_equal_reference(got, hand, faces, obj, thr=0.02 ** 2):
    pen, n_in, n_ct = ref.grasp_scores(hand, faces, obj, thr)
    print("penetration", got["penetration"], "reference", pen, "n_interior", got["n_interior"], "n_contact", got["n_contact"])
    assert np.array_equal(got["n_interior"], n_in) and np.array_equal(got["n_contact"], n_ct)
    nan = np.isnan(pen)                                                 # a NaN is a NaN (its payload is nobody's contract); every number bit for bit
    assert np.array_equal(np.isnan(got["penetration"]), nan)
    assert np.array_equal(bits(got["penetration"])[~nan], bits(pen)[~nan]), (got["penetration"], pen)
    return pen, n_in, n_ct


def assert_scores_agree_with_proxies(got, topo, hand, obj_dev, skip_penetration_rows=()):
    """Against the composed path: counts exactly, penetration at rtol 1e-5 (torch's sum runs in another order)."""
    prox = contact.grasp_proxies(topo, gpu(hand), obj_dev)
    assert np.array_equal(got["n_interior"], prox["n_interior"].cpu().numpy())
    assert np.array_equal(got["n_contact"], prox["n_contact"].cpu().numpy())
    rows = [b for b in range(hand.shape[0]) if b not in skip_penetration_rows]
    assert np.allclose(got["penetration"][rows], prox["penetration"].cpu().numpy()[rows], rtol=1e-5, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1x1", "3x300x776", "2x1024x778", "2x3000x778", "5x257x776"])
def test_grasp_scores_equal_the_reference_bit_for_bit(name, tmp_path):
    hand, faces, obj = score_case(name, tmp_path)
    thr = 0.02 ** 2
    topo, got = run_scores(hand, faces, gpu(obj), thr)
    pen, n_in, n_ct = assert_scores_equal_reference(got, hand, faces, obj, thr)
    if name != "1x1x1":                                                 # the data must exercise all three outputs
        assert 0 < n_in.min() and n_in.max() < obj.shape[1] and (pen > 0).all() and n_ct.max() > 0
    assert_scores_agree_with_proxies(got, topo, hand, gpu(obj))


@pytest.mark.gpu
def test_grasp_scores_read_a_channel_first_view_in_place():
    v, f = ref.sphere_mesh()
    B, N = 3, 500
    cloud = synth.synthetic_normal((B, 4, N), 32, "scores/cf", 0.04)                    # [B,4,N] as the generation path holds it
    hand = (v[None] * np.asarray([1.0, 0.9, 1.1], np.float32)[:, None, None]).astype(np.float32)
    view = gpu(cloud)[:, :3].transpose(1, 2)                                             # strides (4N, 1, N)
    assert not view.is_contiguous()
    topo, got = run_scores(hand, f, view)
    obj = cloud[:, :3].transpose(1, 2).contiguous().numpy()
    _, n_in, _ = assert_scores_equal_reference(got, hand, f, obj)
    assert 0 < n_in.min() and n_in.max() < N
    assert_scores_agree_with_proxies(got, topo, hand, view)


@pytest.mark.gpu
def test_grasp_scores_with_a_nan_row():
    v, f = ref.sphere_mesh()
    B, N = 4, 300
    hand = np.repeat(v[None], B, axis=0).copy()
    obj = synth.synthetic_normal((B, N, 3), 33, "scores/nan", 0.04).numpy()
    obj[1, 17, 2] = np.nan                                                               # a NaN object point: row 1
    hand[3, 5, 0] = np.nan                                                               # a NaN hand vertex: row 3 (NaN wins every argmin)
    topo, got = run_scores(hand, f, gpu(obj))
    pen, n_in, n_ct = assert_scores_equal_reference(got, hand, f, obj)
    assert np.isnan(got["penetration"][[1, 3]]).all() and np.isfinite(got["penetration"][[0, 2]]).all()
    assert n_ct[3] == 0 and n_in[3] == 0
    # grasp_proxies drops a NaN distance from its sum (its interior test is false); the fused kernel reports the row as NaN
    assert_scores_agree_with_proxies(got, topo, hand, gpu(obj), skip_penetration_rows=(1, 3))


@pytest.mark.gpu
def test_grasp_scores_of_a_row_do_not_depend_on_the_batch(tmp_path):
    hand, faces, obj = score_case("5x257x776", tmp_path)
    topo, got = run_scores(hand, faces, gpu(obj))
    for b in range(hand.shape[0]):
        _, one = run_scores(hand[b:b + 1], faces, gpu(obj[b:b + 1]))
        for k in got:
            assert np.array_equal(one[k].view(np.uint32), got[k][b:b + 1].view(np.uint32)), (k, b)
    # a batch beyond one launch (65 535 grasps): row r holds grasp r % 5, and must score as that grasp alone
    B = 65535 + 70
    pick = torch.arange(B, device=DEV) % hand.shape[0]
    big = contact.grasp_scores(topo, gpu(hand)[pick].contiguous(), gpu(obj[:, :16])[pick].contiguous())
    small = contact.grasp_scores(topo, gpu(hand), gpu(obj[:, :16]).contiguous())
    for k in big:
        assert torch.equal(big[k], small[k][pick]), k
    empty = contact.grasp_scores(topo, gpu(hand)[:0].contiguous(), gpu(obj)[:0].contiguous())
    assert all(v.shape == (0,) for v in empty.values())


@pytest.mark.gpu
def test_grasp_scores_refuse_what_the_kernel_cannot_hold():
    v, f = ref.sphere_mesh(4, 6)
    topo = contact.HandTopology(f, len(v), DEV)
    hand = gpu(v)[None].contiguous()
    with pytest.raises(RuntimeError):
        contact.grasp_scores(topo, hand, torch.zeros(1, 0, 3, device=DEV))
    with pytest.raises(RuntimeError):
        contact.grasp_scores(topo, hand, torch.zeros(2, 4, 3, device=DEV))
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL, nothing launched
    one = torch.zeros(8, device=DEV)
    for V, N, B in ((2049, 4, 1), (0, 4, 1), (5, 0, 1), (5, 4, -1)):
        rc = lib.dvq_grasp_scores(one.data_ptr(), topo.faces.data_ptr(), topo.vf_off.data_ptr(), topo.vf_face.data_ptr(), V,
                                  one.data_ptr(), 0, 3, 1, B, N, 0.0004, one.data_ptr(), one.data_ptr(), one.data_ptr(), None)
        assert rc == 1, (V, N, B)


# ------------------------------------------------------------------------------------------------------ GPU: the selection
def topk_case(O, M, seed):
    rng = np.random.default_rng(seed)
    values = np.asarray([0.0, -0.0, 1.0, 1.0, -2.5, 3.0e-7, np.inf, -np.inf, NAN, 0.125, 7.0, -7.0], np.float32)
    key = values[rng.integers(0, len(values), size=O * M)]                              # heavy duplication, both zeros, NaN
    fresh = rng.random(O * M) < 0.3
    key[fresh] = rng.normal(size=int(fresh.sum())).astype(np.float32)                   # and values of their own
    cls = rng.integers(0, 3, size=O * M).astype(np.int32)                               # all three classes
    return cls, key


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 2, 100, 4096])
def test_segment_topk_equals_the_reference_order(M):
    O = 3
    cls, key = topk_case(O, M, 100 + M)
    if M >= 100:
        assert len(set(cls.tolist())) == 3 and np.isnan(key).any() and (bits(key) == 0x80000000).any() and (bits(key) == 0).any()
    for keep in sorted({1, M // 2, M}):
        if keep == 0:                                                                    # M = 1: M // 2 is out of range
            with pytest.raises(RuntimeError):
                ops.segment_topk(gpu(cls), gpu(key), O, M, 0)
            continue
        got = ops.segment_topk(gpu(cls), gpu(key), O, M, keep)
        assert got.dtype == torch.int64 and tuple(got.shape) == (O, keep)
        want = ref.segment_topk(cls, key, O, M, keep)
        assert np.array_equal(got.cpu().numpy(), want), (M, keep)
    # unique keys too (no tie to break), and a single class
    rng = np.random.default_rng(M)
    key = rng.permutation(O * M).astype(np.float32) - 5.0
    cls = np.zeros(O * M, np.int32)
    got = ops.segment_topk(gpu(cls), gpu(key), O, M, M)
    assert np.array_equal(got.cpu().numpy(), ref.segment_topk(cls, key, O, M, M))
    assert np.array_equal(np.sort(got.cpu().numpy(), axis=1), np.tile(np.arange(M), (O, 1)))


@pytest.mark.gpu
def test_segment_topk_refuses_sizes_out_of_range():
    cls, key = torch.zeros(8194, dtype=torch.int32, device=DEV), torch.zeros(8194, device=DEV)
    for O, M, keep in ((2, 4097, 1), (2, 4, 5), (2, 4, 0), (-1, 4, 1), (2, 0, 0)):
        with pytest.raises(RuntimeError):
            ops.segment_topk(cls[:max(O, 0) * M], key[:max(O, 0) * M], O, M, keep)
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL
    for O, M, keep in ((2, 4097, 1), (2, 4, 5), (2, 4, 0), (-1, 4, 1)):
        assert lib.dvq_segment_topk(cls.data_ptr(), key.data_ptr(), O, M, keep, key.data_ptr(), None) == 1, (O, M, keep)
    assert tuple(ops.segment_topk(cls[:0], key[:0], 0, 4, 2).shape) == (0, 2)


# ------------------------------------------------------------------------------------------------------ GPU: end to end
def _gennet(tmp_path):
    """The synthetic net of tests/test_generate_batched.py with the REAL MANO model of the fixture (the scores need its faces)."""
    from conftest import GOLDEN, gen_state_dict
    from dvqvae_amd import mano as dmano
    from dvqvae_amd.network.gen_net import GenNet
    net = GenNet()
    net.load_state_dict(gen_state_dict(net.state_dict(), np.load(os.path.join(GOLDEN, "g7_gen.npz"))), strict=True)
    net.eval().to(DEV)
    net.set_rh_mano(dmano.load(model_path=mano_pkl(tmp_path), model_type="mano", use_pca=True, num_pca_comps=45,
                               flat_hand_mean=True).to(DEV))
    return net


E2E_SEED, E2E_M, E2E_K = 9, 24, 5
E2E_INDICES = [5, 2, 11, 7]


def e2e_objects(at_the_hand=False):
    """Four clouds of two point counts.  The synthetic weights put every hand near (-0.14, -0.06, 0.13) whatever the object, about
    0.8 m from a cloud under the datasets' random rotation and canonical offset, where every candidate scores penetration +0.0 and no
    contact (the CPU oracle shows it).  ``at_the_hand``: 20 cm cubes of points around that place for calls without
    rotation, so that the candidates' penetration keys differ."""
    if not at_the_hand:
        return [synth.synthetic_clouds(1, n, seed=60 + i)[0] for i, n in enumerate((700, 300, 700, 300))]
    centre = np.asarray([-0.08, -0.09, 0.13])
    return [generate.object_tensor(synth.synthetic_uniform((n, 3), 70 + i, "select/e2e", -0.1, 0.1).numpy().astype(np.float64) + centre)
            for i, n in enumerate((700, 300, 700, 300))]


@pytest.mark.gpu
@pytest.mark.parametrize("select_by,rotate", [("penetration", False), ("log_prob", True)])
def test_best_of_m_keeps_rows_of_the_plain_run(select_by, rotate, tmp_path):
    net = _gennet(tmp_path)
    objs, M, k = e2e_objects(at_the_hand=not rotate), E2E_M, E2E_K
    with_lp = select_by == "log_prob"
    plain = generate.generate_for_objects(net, objs, M, rotate, E2E_SEED, E2E_INDICES, log_prob=with_lp)  # the parent's code path
    first = None
    varied, beyond = False, False
    for rows_per_call in (16384, M, 1):
        got = generate.generate_for_objects(net, objs, k, rotate, E2E_SEED, E2E_INDICES, rows_per_call=rows_per_call, candidates=M,
                                            select_by=select_by, min_contact=1)
        assert len(got) == len(objs)
        for i, (g, p) in enumerate(zip(got, plain)):
            cand = g["candidate"]
            assert cand.dtype == torch.int64 and tuple(cand.shape) == (k,)
            c = cand.cpu().numpy()
            assert len(set(c.tolist())) == k and c.min() >= 0 and c.max() < M
            assert tuple(g["params"].shape) == (k, 61) and tuple(g["vertices"].shape) == (k, 778, 3)
            assert torch.equal(g["params"], p["params"][cand]), f"object {i}: kept parameters are not rows of the plain run"
            assert torch.equal(g["vertices"], p["vertices"][cand]), f"object {i}: kept vertices"
            j = g["json"]
            assert j["candidate"] == c.tolist()
            assert j["recon_params"] == [p["json"]["recon_params"][x] for x in c]
            assert j["R_list"] == [p["json"]["R_list"][x] for x in c] and j["r_list"] == [p["json"]["r_list"][x] for x in c]
            assert j["trans_list"] == p["json"]["trans_list"][:k]
            scores = {name: t.cpu() for name, t in g["scores"].items()}
            assert all(tuple(t.shape) == (M,) for t in scores.values())
            assert {"penetration", "n_interior", "n_contact"} <= set(scores) and ("log_prob" in scores) == with_lp
            for name in ("penetration", "n_interior", "n_contact"):
                assert j[name] == scores[name].numpy()[c].tolist(), name
            if with_lp:
                assert torch.equal(g["scores"]["log_prob"], p["log_prob"]) and torch.equal(g["log_prob"], p["log_prob"][cand])
                assert j["log_prob"] == scores["log_prob"].numpy()[c].tolist()
            else:
                assert "log_prob" not in j and "log_prob" not in g
            # the scores of ALL candidates are those of the plain run's hands against their clouds, and the order is the reference's
            cls, key = contact.select_keys(scores, select_by, 1, log_prob=scores.get("log_prob"))
            assert np.array_equal(c, ref.segment_topk(cls.numpy(), key.numpy(), 1, M, k)[0]), f"object {i}: order"
            pairs = {(int(a), float(b)) for a, b in zip(cls.tolist(), key.tolist())}
            print(f"{select_by} rows_per_call {rows_per_call} object {i}: kept {c.tolist()}, {len(pairs)} distinct (cls, key), "
                  f"n_contact {scores['n_contact'].tolist()}")
            varied |= len(pairs) >= 2
            beyond |= bool((c >= k).any())
        dumped = [json.dumps(g["json"]) for g in got]
        if first is None:
            first = dumped
        assert dumped == first, f"rows_per_call {rows_per_call}: the JSON differs from the 16384-row call's"
    # against a vacuous pass: the candidates must differ in what ranks them, and the selection must reach beyond the first k
    assert varied, "every candidate has the same (cls, key): the selection is not exercised"
    assert beyond, "only the first k candidates were kept: the selection is not exercised"


@pytest.mark.gpu
def test_best_of_m_scores_are_the_scores_of_the_plain_hands(tmp_path):
    net = _gennet(tmp_path)
    objs, M, k = e2e_objects(at_the_hand=True)[:2], 8, 3
    plain = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES[:2])
    got = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES[:2], candidates=M)
    faces = np.asarray(net.rh_mano.faces)
    for i, (g, p) in enumerate(zip(got, plain)):
        R = np.asarray(p["json"]["R_list"], np.float64)                                  # [M,3,4]: rotation | translation
        xyz = objs[i][:3].numpy().astype(np.float64)
        cloud = ops.transform_cloud(gpu(objs[i]).contiguous(), gpu(R[:, :, :3].astype(np.float32)).contiguous(),
                                    gpu(R[0, :, 3].astype(np.float32)).contiguous())
        assert np.allclose(cloud[:, :3].cpu().numpy(), np.einsum("mij,jn->min", R[:, :, :3], xyz) + R[:, :, 3:], atol=1e-5)
        pen, n_in, n_ct = ref.grasp_scores(p["vertices"].cpu().numpy(), faces, cloud[:, :3].transpose(1, 2).cpu().numpy())
        assert np.array_equal(bits(g["scores"]["penetration"].cpu().numpy()), bits(pen))
        assert (pen > 0).all() and n_ct.min() > 0, "the clouds must sit at the hands"
        assert np.array_equal(g["scores"]["n_interior"].cpu().numpy(), n_in) and np.array_equal(g["scores"]["n_contact"].cpu().numpy(), n_ct)


@pytest.mark.gpu
def test_best_of_m_needs_a_face_list():
    from dvqvae_amd import mano as dmano
    from dvqvae_amd.network.gen_net import GenNet
    from conftest import GOLDEN, gen_state_dict
    net = GenNet()
    net.load_state_dict(gen_state_dict(net.state_dict(), np.load(os.path.join(GOLDEN, "g7_gen.npz"))), strict=True)
    net.eval().to(DEV)
    net.set_rh_mano(dmano.ManoLayer(dmano.synthetic_mano_arrays()).to(DEV))
    with pytest.raises(RuntimeError, match="no face list"):
        generate.generate_for_objects(net, e2e_objects()[:1], 2, True, 1, [0], candidates=4)
    with pytest.raises(RuntimeError, match="candidates"):
        generate.generate_for_objects(net, e2e_objects()[:1], 5, True, 1, [0], candidates=4)


def _run_main(dataset, out_dir, extra, mano="/nonexistent"):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
def test_ho3d_entry_point_writes_the_selected_grasps(tmp_path):
    mano = mano_pkl(tmp_path)
    M, k, n_obj = 12, 5, 3
    base = ["--num_objects", str(n_obj), "--points", "256", "--num_grasp", str(k), "--candidates", str(M)]
    names0, bytes0 = _run_main("ho3d", str(tmp_path / "default"), base, mano)
    assert names0 == [f"obj_id_synthetic_{i}.json" for i in range(n_obj)]
    _, plain = _run_main("ho3d", str(tmp_path / "plain"), ["--num_objects", str(n_obj), "--points", "256", "--num_grasp", str(M)], mano)
    for data, full in zip(bytes0, plain):
        j, p = json.loads(data), json.loads(full)
        assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact"}
        assert all(len(j[f]) == k for f in j)
        c = j["candidate"]
        assert len(set(c)) == k and all(0 <= x < M for x in c)
        assert j["recon_params"] == [p["recon_params"][x] for x in c] and j["R_list"] == [p["R_list"][x] for x in c]
        assert j["r_list"] == [p["r_list"][x] for x in c]
        assert all(isinstance(x, int) for x in j["n_interior"] + j["n_contact"]) and all(isinstance(x, float) for x in j["penetration"])
    for tag, extra in (("m", ["--rows_per_call", str(M)]), ("one", ["--rows_per_call", "1"]), ("loop", ["--rows_per_call", "0"])):
        names, data = _run_main("ho3d", str(tmp_path / tag), base + extra, mano)
        assert names == names0 and data == bytes0, f"--rows_per_call {extra[1]}: the files differ"
    _, by_lp = _run_main("ho3d", str(tmp_path / "lp"), base + ["--select_by", "log_prob"], mano)
    for data, full in zip(by_lp, plain):
        j = json.loads(data)
        assert len(j["log_prob"]) == k and j["log_prob"] == sorted(j["log_prob"], reverse=True)
        assert j["recon_params"] == [json.loads(full)["recon_params"][x] for x in j["candidate"]]
    _, with_lp = _run_main("ho3d", str(tmp_path / "pen_lp"), base + ["--log_prob", "1"], mano)
    for data, sel in zip(with_lp, bytes0):
        j, s = json.loads(data), json.loads(sel)
        assert len(j["log_prob"]) == k and {f: j[f] for f in s} == s


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", ["obman", "ho3d"])
def test_candidates_zero_writes_the_files_of_a_run_without_the_flags(tmp_path, dataset):
    base = ["--num_objects", "4", "--points", "256"]
    for tag, extra in (("grouped", []), ("loop", ["--rows_per_call", "0"])):
        names0, bytes0 = _run_main(dataset, str(tmp_path / f"{tag}_plain"), base + extra)
        names, data = _run_main(dataset, str(tmp_path / f"{tag}_zero"),
                                base + extra + ["--candidates", "0", "--select_by", "log_prob", "--min_contact", "9"])
        assert names == names0 and data == bytes0
        assert set(json.loads(data[0])) == {"recon_params", "R_list", "trans_list", "r_list"}
