"""Hand-side contact: the fused per-part kernel (dvq_grasp_parts), its host API (ops.grasp_parts, contact.HandParts / grasp_parts /
part_stats / contact_map / parts_class) and the ``--parts`` / ``--min_fingers`` / ``--need_thumb`` mode of the entry points.  The
reference is tests/grasp_parts_ref.py (numpy over oracle/contact_oracle.nn_points with the hand as the source); GPU results are
compared with it bit for bit."""
import json
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops, synth

import grasp_parts_ref as ref
import grasp_score_ref as score_ref

DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
THR = 0.005                                                              # metres: the default
OUTPUTS = ("part_min", "part_count", "mask", "status")
FIELDS = ("fingers_in_contact", "part_contact", "part_dist")
TILE = ops.GRASP_PARTS_TILE


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_parts_flags(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.parts, a.part_threshold, a.part_min_verts, a.min_fingers, a.need_thumb, a.hand_parts) == (0, 0.005, 1, 0, 0, None)
    a = generate.parse_args(dataset, ["--parts", "1", "--part_threshold", "0.01", "--part_min_verts", "3", "--min_fingers", "5",
                                      "--need_thumb", "1", "--hand_parts", "table.json", "--candidates", "200", "--num_grasp", "100"])
    assert (a.parts, a.part_threshold, a.part_min_verts, a.min_fingers, a.need_thumb, a.hand_parts) == (1, 0.01, 3, 5, 1, "table.json")
    assert generate.parse_args(dataset, ["--parts", "1"]).parts == 1                  # the figures alone need no candidates
    cand = ["--candidates", "200", "--num_grasp", "100"]
    for bad in (["--part_threshold", "0"], ["--part_threshold", "-0.01"], ["--part_threshold", "inf"], ["--part_threshold", "nan"],
                ["--min_fingers", "6"] + cand, ["--min_fingers", "-1"] + cand, ["--part_min_verts", "0"],
                ["--min_fingers", "2"], ["--need_thumb", "1"], ["--need_thumb", "2"] + cand):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_grasp_parts" in _lib.SIGNATURES and "int dvq_grasp_parts(" in header and hasattr(lib, "dvq_grasp_parts")
    assert "dvq_grasp_parts" in re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert len(_lib.SIGNATURES["dvq_grasp_parts"][1]) == 18
    assert lib.dvq_abi_version() == 10 and ops.GRASP_PARTS_TILE >= 256 and ops.GRASP_PARTS_TILE % 256 == 0


def test_ops_refuse_bad_arguments_before_any_device_use():
    hand = torch.zeros(1, 6, 3)
    labels = torch.zeros(6, dtype=torch.int32)
    obj = torch.zeros(1, 5, 3)
    good = dict(hand=hand, part_of_vertex=labels, n_parts=2, obj=obj, contact_threshold=1e-4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_parts(**good)                                                      # well-formed, but not on a device
    for bad in (dict(hand=torch.zeros(1, 2049, 3), part_of_vertex=torch.zeros(2049, dtype=torch.int32)),   # V > 2048
                dict(hand=torch.zeros(1, 0, 3), part_of_vertex=labels[:0]),                                # V = 0
                dict(obj=torch.zeros(1, 0, 3)),                                                            # N = 0
                dict(n_parts=0), dict(n_parts=33),                                                         # P outside 1 .. 32
                dict(hand=hand.double()), dict(obj=obj.double()), dict(part_of_vertex=labels.long()),      # wrong dtype
                dict(hand=torch.zeros(1, 3, 6).transpose(1, 2)),                                           # not contiguous
                dict(hand=hand.expand(2, -1, -1), obj=torch.zeros(2, 5, 3)),
                dict(part_of_vertex=labels[:5]), dict(part_of_vertex=torch.zeros(7, dtype=torch.int32)),   # a label vector of the wrong length
                dict(part_of_vertex=torch.zeros(12, dtype=torch.int32)[::2]),
                dict(obj=torch.zeros(2, 5, 3)), dict(obj=torch.zeros(1, 5, 4)), dict(contact_threshold=NAN)):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_parts(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    parts = contact.HandParts(np.zeros(6, np.int64), ["a", "b"])
    for thr in (0.0, -0.005, INF, NAN):
        with pytest.raises(RuntimeError, match="threshold"):
            contact.grasp_parts(parts, hand, obj, threshold=thr)
    with pytest.raises(RuntimeError, match="6 vertices"):                            # the table's vertex count and V disagree
        contact.grasp_parts(parts, torch.zeros(1, 7, 3), obj)


def test_hand_parts_tables(tmp_path):
    parts = contact.HandParts.from_json()
    assert parts.n_verts == 778 and parts.n_parts == 6 and len(parts.names) == 6 and parts.labels.dtype == np.int32
    assert parts.labels.min() == 0 and parts.labels.max() == 5 and parts.sizes.sum() == 778 and (parts.sizes > 0).all()
    table = json.load(open(contact.HAND_PARTS_JSON))
    assert parts.names == table["order"]                                             # the file's own order
    for q, listed in enumerate(table["parts"]):
        assert (parts.labels[listed] == q).all()                                     # disjoint: every listed vertex is its part's
    path = str(tmp_path / "table.json")
    json.dump({"order": ["thumb", "index", "rest"], "parts": [[4, 2, 2], [2, 3, 4, 0], [5, 0]], "n_verts": 8}, open(path, "w"))
    small = contact.HandParts.from_json(path)
    assert small.labels.tolist() == [1, -1, 0, 1, 0, 2, -1, -1] and small.names == ["thumb", "index", "rest"]   # the first part that lists a vertex
    assert small.sizes.tolist() == [2, 2, 1] and small.n_verts == 8
    assert contact.HandParts([0, 5, -3, 1], ["a", "b"]).labels.tolist() == [0, -1, -1, 1]      # outside [0, P): no part
    for labels, names in (([], ["a"]), ([0, 1], []), ([0], [str(i) for i in range(33)]), ([[0, 1]], ["a"]), ([0.5], ["a"])):
        with pytest.raises(RuntimeError):
            contact.HandParts(np.asarray(labels), names)


def test_host_statistics_equal_independent_code():
    rng = np.random.default_rng(11)
    B, P, V = 9, 6, 778
    part_count = rng.integers(0, 4, size=(B, P)).astype(np.int32)
    part_min = (rng.random((B, P)) * 1e-3).astype(np.float32)
    part_min[2, 4] = np.inf                                                          # an empty part
    status = np.zeros(B, np.int32)
    status[5] = 1
    part_min[5], part_count[5] = np.nan, -1
    for min_verts, n_fingers in ((1, 5), (2, 5), (3, 3)):
        got = contact.part_stats(torch.from_numpy(part_min), torch.from_numpy(part_count), torch.from_numpy(status), min_verts, n_fingers)
        want = ref.part_stats(part_min, part_count, status, min_verts, n_fingers)
        assert tuple(got) == FIELDS and all(len(got[k]) == B for k in FIELDS)
        for b, w in enumerate(want):
            if w is None:
                assert all(got[k][b] is None for k in FIELDS)
                continue
            assert got["fingers_in_contact"][b] == w[0] and got["part_contact"][b] == w[1]
            for g, x in zip(got["part_dist"][b], w[2]):
                assert (g is None) == (x is None) and (g is None or abs(g - x) <= 1e-15 * x)     # one float64 sqrt and one product
        assert len({f for f in got["fingers_in_contact"] if f is not None}) >= 2
    text = json.dumps(got)
    assert "NaN" not in text and "Infinity" not in text and json.loads(text)["part_dist"][2][4] is None
    assert json.loads(text)["fingers_in_contact"][5] is None
    mask = rng.integers(-2 ** 31, 2 ** 31, size=(B, 25)).astype(np.int32)           # the sign bit is vertex 31 of a word
    got_map = contact.contact_map(torch.from_numpy(mask), V)
    assert got_map.dtype == np.int64 and got_map.shape == (V,) and got_map.tolist() == ref.contact_map(mask, V)
    assert 0 <= got_map.min() < got_map.max() <= B and contact.contact_map(mask[:0], V).tolist() == [0] * V
    with pytest.raises(RuntimeError):
        contact.contact_map(mask, 900)
    out = {"part_count": torch.from_numpy(part_count), "status": torch.from_numpy(status)}
    seen = set()
    for min_fingers, need_thumb, min_verts in ((0, False, 1), (3, False, 1), (5, False, 1), (0, True, 1), (2, True, 2), (4, False, 3)):
        cls = contact.parts_class(out, min_fingers, need_thumb, min_verts)
        assert cls.dtype == torch.int32 and cls.tolist() == ref.parts_class(part_count, status, min_fingers, need_thumb, min_verts)
        seen |= set(cls.tolist())
    assert seen == {0, 1, 2} and contact.parts_class(out, 0, False, 1).tolist() == [0, 0, 0, 0, 0, 2, 0, 0, 0]
    assert contact.SELECT_BY == ("penetration", "log_prob", "stability")             # a guard only: nothing ranks by fingers


# ------------------------------------------------------------------------------------------------------ CPU: the reference itself
def mano_rows(tmp_path):
    """The MANO template plus 1 mm noise against clouds of 300 points, N(0, 2 cm) about the template's centre moved by -5 .. +5 cm
    along x: four rows whose contact differs."""
    from test_grasp_select import mano_faces
    _, v = mano_faces(tmp_path)
    B, N = 4, 300
    hand = (v[None] + synth.synthetic_normal((B, 778, 3), 51, "parts/mano/h", 0.001).numpy()).astype(np.float32)
    shift = np.zeros((B, 1, 3), np.float32)
    shift[:, 0, 0] = np.linspace(-0.05, 0.05, B)
    obj = (v.mean(0)[None, None] + shift + synth.synthetic_normal((B, N, 3), 51, "parts/mano/o", 0.02).numpy()).astype(np.float32)
    return hand, obj


def test_reference_on_the_mano_template(tmp_path):
    parts = contact.HandParts.from_json()
    hand, obj = mano_rows(tmp_path)
    want = ref.grasp_parts(hand, parts.labels, 6, obj, THR * THR)
    stats = contact.part_stats(want["part_min"], want["part_count"], want["status"])
    print(stats["fingers_in_contact"], want["part_count"].tolist(), stats["part_dist"])
    assert want["status"].tolist() == [0] * 4
    assert (want["part_count"][:, 0] == 0).any(), "no row without the thumb"
    assert len(set(stats["fingers_in_contact"])) >= 2, "every row has the same number of fingers in contact"
    assert ((0 < want["part_count"]) & (want["part_count"] < parts.sizes[None])).any(), "no part is partly in contact"
    assert (want["vert_idx"] != 0).any() and want["vert_idx"].min() >= 0 and want["vert_idx"].max() < 300
    # the outputs are consistent among themselves
    assert contact.contact_map(want["mask"], 778).sum() == want["part_count"].sum()          # the table covers every vertex
    assert np.array_equal(want["part_min"].min(axis=1), want["vert_dist"].min(axis=1))
    need = contact.parts_class({k: torch.from_numpy(x) for k, x in want.items()}, 0, True)
    assert need.tolist() == [int(c == 0) for c in want["part_count"][:, 0]]


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def parts_case(name, tmp_path):
    """(hand [B,V,3], labels [V], P, sizes [P], obj [B,N,3]) numpy."""
    rng = lambda tag, shape, scale: synth.synthetic_normal(shape, 52, f"parts/{name}/{tag}", scale).numpy()
    B, N, V = (int(x) for x in name.split("x"))
    if name == "1x1x1":                                                  # one vertex, one point within the threshold
        hand = rng("h", (1, 1, 3), 0.1)
        return hand, np.zeros(1, np.int64), 1, np.ones(1, np.int64), (hand + rng("o", (1, 1, 3), 0.001)).astype(np.float32)
    if V == 776:                                                         # the sphere, labelled by index band: 0 1 2 3 -1 5 and a tail of 9s
        v, _ = score_ref.sphere_mesh()
        scale = np.linspace(0.8, 1.2, B).astype(np.float32)[:, None, None]
        hand = (v[None] * scale + rng("h", (B, len(v), 3), 0.002)).astype(np.float32)
        labels = np.arange(V) // 130
        labels[labels == 4] = -1                                         # part 4 is empty
        labels[770:] = 9                                                 # outside [0, 6): no part
        sizes = np.bincount(labels[(labels >= 0) & (labels < 6)], minlength=6)
        assert sizes[4] == 0 and (labels < 0).any()
        return hand, labels, 6, sizes, rng("o", (B, N, 3), 0.04)
    parts = contact.HandParts.from_json()
    hand, obj = mano_rows(tmp_path)
    centre = hand[0].mean(0)[None, None]
    obj = (centre + rng("o", (B, N, 3), 0.03)).astype(np.float32)
    return hand[:B], parts.labels, 6, parts.sizes, obj


def run_parts(hand, labels, P, obj_dev, thr=THR, want_verts=True):
    parts = contact.HandParts(labels, [f"p{q}" for q in range(P)], DEV)
    out = contact.grasp_parts(parts, gpu(hand), obj_dev, thr, want_verts=want_verts)
    assert tuple(out) == OUTPUTS + (("vert_dist", "vert_idx") if want_verts else ())
    B, V = hand.shape[:2]
    assert [tuple(out[k].shape) for k in OUTPUTS] == [(B, P), (B, P), (B, (V + 31) // 32), (B,)]
    assert all(out[k].dtype == (torch.float32 if k in ("part_min", "vert_dist") else torch.int32) for k in out)
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same_bits(got, want, rows=None, what=""):
    """Every number bit for bit; a NaN is a NaN (its payload is nobody's contract)."""
    for k in got:
        g, w = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        if g.dtype != np.float32:
            assert np.array_equal(g, w), (what, k, g, w)
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, k, g, w)
        assert np.array_equal(bits(g)[~nan], bits(w)[~nan]), (what, k, g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["1x1x1", "3x255x776", "3x256x776", "2x257x778", "2x1000x778"])
def test_grasp_parts_equals_the_reference_bit_for_bit(name, tmp_path):
    hand, labels, P, sizes, obj = parts_case(name, tmp_path)
    got = run_parts(hand, labels, P, gpu(obj))
    want = ref.grasp_parts(hand, labels, P, obj, THR * THR)
    print("part_count", got["part_count"].tolist(), want["part_count"].tolist(), "part_min", got["part_min"].tolist())
    assert_same_bits(got, want, what=name)
    assert want["status"].tolist() == [0] * hand.shape[0]
    if name == "1x1x1":
        assert want["part_count"].tolist() == [[1]] and want["mask"].tolist() == [[1]] and want["vert_idx"].tolist() == [[0]]
    else:
        assert ((0 < want["part_count"]) & (want["part_count"] < sizes[None])).any(), "no part is partly in contact"
        assert (want["vert_idx"] != 0).any(), "every vertex's nearest point is point 0"
        assert np.array_equal(np.isinf(want["part_min"]), np.broadcast_to(sizes[None] == 0, want["part_min"].shape))
    # the per-vertex outputs are the bits of nn_points with the hand as the source, on the same device tensors
    h_dev, o_dev = gpu(hand), gpu(obj)
    parts = contact.HandParts(labels, [f"p{q}" for q in range(P)], DEV)
    full = contact.grasp_parts(parts, h_dev, o_dev, THR, want_verts=True)
    d, idx = ops.nn_points(h_dev, o_dev)
    assert torch.equal(full["vert_dist"].view(torch.int32), d.view(torch.int32)) and torch.equal(full["vert_idx"].long(), idx)
    # ... and passing NULL for both changes no other output
    lean = run_parts(hand, labels, P, o_dev, want_verts=False)
    assert_same_bits(lean, got, what=f"{name} without the per-vertex outputs")


SEAMS = {"one_past": (TILE + 1, [7, TILE - 1, TILE], []),
         "one_past_dup": (TILE + 1, [7, TILE - 1], [(7, TILE)]),
         "two_past": (2 * TILE + 3, [7, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 2 * TILE + 2], [(TILE - 1, 2 * TILE + 1), (7, TILE + 5)])}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(SEAMS))
def test_grasp_parts_across_the_tile_seam(case):
    """N = TILE + 1 and 2 * TILE + 3 with V = 8: vertex i's nearest point is planted at a chosen index -- in the first tile, at a
    tile's last index, at the next tile's first, at the last point -- and exact duplicates of a nearest point sit in a later tile:
    the lower index wins."""
    N, targets, dups = SEAMS[case]
    V = 8
    hand = (np.arange(V, dtype=np.float32)[:, None] * np.asarray([0.1, 0.0, 0.0], np.float32))[None]       # 10 cm apart along x
    obj = (synth.synthetic_uniform((1, N, 3), 53, f"parts/seam/{case}", -0.1, 0.1).numpy() + np.asarray([0.35, 1.0, 1.0], np.float32)).astype(np.float32)
    for i, p in enumerate(targets):                                      # 1 mm from vertex i: nearer than anything else
        obj[0, p] = hand[0, i] + np.asarray([0.0, 0.001, 0.0], np.float32)
    for src, at in dups:
        obj[0, at] = obj[0, src]
    labels = np.arange(V) % 3
    got = run_parts(hand, labels, 3, gpu(obj))
    want = ref.grasp_parts(hand, labels, 3, obj, THR * THR)
    assert want["vert_idx"][0, :len(targets)].tolist() == targets and want["mask"][0, 0] == (1 << len(targets)) - 1
    assert want["vert_idx"][0].max() < N and want["part_count"].sum() == len(targets)
    print(case, got["vert_idx"].tolist(), want["vert_idx"].tolist())
    assert_same_bits(got, want, what=case)


@pytest.mark.gpu
def test_grasp_parts_reads_a_channel_first_view_in_place(tmp_path):
    parts = contact.HandParts.from_json()
    hand, _ = mano_rows(tmp_path)
    B, N = 3, 500
    centre = hand[0].mean(0)
    cloud = synth.synthetic_normal((B, 4, N), 54, "parts/cf", 0.03)                      # [B,4,N] as the generation path holds it
    cloud[:, :3] += torch.from_numpy(centre)[None, :, None]
    view = gpu(cloud)[:, :3].transpose(1, 2)                                             # strides (4N, 1, N)
    assert not view.is_contiguous()
    got = run_parts(hand[:B], parts.labels, 6, view)
    copy = run_parts(hand[:B], parts.labels, 6, view.contiguous())
    want = ref.grasp_parts(hand[:B], parts.labels, 6, cloud[:, :3].transpose(1, 2).contiguous().numpy(), THR * THR)
    assert ((0 < want["part_count"]) & (want["part_count"] < parts.sizes[None])).any()
    assert_same_bits(got, want, what="view")
    assert_same_bits(got, copy, what="view against its contiguous copy")


@pytest.mark.gpu
def test_grasp_parts_with_nan_rows_and_rows_alone(tmp_path):
    hand, labels, P, sizes, obj = parts_case("3x255x776", tmp_path)
    hand, obj = np.concatenate([hand, hand[:2]]), np.concatenate([obj, obj[1:]])          # five rows
    B = 5
    clean = run_parts(hand, labels, P, gpu(obj))
    assert clean["status"].tolist() == [0] * B and (clean["part_count"].sum(axis=1) > 0).all()
    bad_h, bad_o = hand.copy(), obj.copy()
    bad_o[1, 17, 2] = np.nan                                                             # a NaN cloud coordinate: row 1
    bad_h[3, 700, 0] = np.nan                                                            # a NaN hand coordinate: row 3
    got = run_parts(bad_h, labels, P, gpu(bad_o))
    assert got["status"].tolist() == [0, 1, 0, 1, 0]
    for b in (1, 3):
        assert np.isnan(got["part_min"][b]).all() and np.isnan(got["vert_dist"][b]).all() and (got["mask"][b] == 0).all()
        assert (got["part_count"][b] == -1).all() and (got["vert_idx"][b] == -1).all()
    assert_same_bits(got, clean, rows=[0, 2, 4], what="the rows beside the NaN rows")
    assert_same_bits(got, ref.grasp_parts(bad_h, labels, P, bad_o, THR * THR), what="nan")
    out = {k: torch.from_numpy(x) for k, x in got.items()}
    assert contact.parts_class(out, 0, False).tolist() == [0, 2, 0, 2, 0]
    stats = contact.part_stats(got["part_min"], got["part_count"], got["status"])
    assert [f is None for f in stats["fingers_in_contact"]] == [False, True, False, True, False]
    for b in range(B):                                                                   # a row alone gives the bits it has inside the batch
        one = run_parts(bad_h[b:b + 1], labels, P, gpu(bad_o[b:b + 1]))
        assert_same_bits(one, {k: x[b:b + 1] for k, x in got.items()}, what=f"row {b} alone")
    inf_o = obj.copy()
    inf_o[0, 3, 1] = np.inf                                                              # an infinity is no figure either
    assert run_parts(hand, labels, P, gpu(inf_o))["status"].tolist() == [1, 0, 0, 0, 0]


@pytest.mark.gpu
def test_grasp_parts_across_the_chunk_seam():
    """B = 65 537 grasps in two launches (65 535 + 2): the rows at the seam equal the reference."""
    B, rows = 65537, [0, 65534, 65535, 65536]
    base = np.asarray([[0.0, 0.0, 0.0], [0.05, 0.0, 0.0], [0.0, 0.05, 0.0], [0.0, 0.0, 0.05]], np.float32)
    hand = (base[None] + synth.synthetic_normal((B, 4, 3), 55, "parts/seam/h", 0.005).numpy()).astype(np.float32)
    near = hand[np.arange(B), np.arange(B) % 4][:, None]                                 # row b's point sits at its vertex b mod 4
    obj = (near + synth.synthetic_normal((B, 1, 3), 55, "parts/seam/o", 0.002).numpy()).astype(np.float32)
    labels = np.asarray([0, 1, 1, 2])
    got = run_parts(hand, labels, 3, gpu(obj))
    want = ref.grasp_parts(hand[rows], labels, 3, obj[rows], THR * THR)
    assert want["mask"][:, 0].tolist() == [1, 4, 8, 1] and len({x.tobytes() for x in want["part_min"]}) == 4
    assert_same_bits({k: x[rows] for k, x in got.items()}, want, what="seam")
    assert (got["status"] == 0).all() and set(np.unique(got["mask"]).tolist()) <= {0, 1, 2, 4, 8} and (got["mask"] != 0).mean() > 0.7
    assert np.array_equal(got["part_count"].sum(axis=1), (got["mask"][:, 0] != 0).astype(np.int64))
    parts = contact.HandParts(labels, ["a", "b", "c"], DEV)
    empty = contact.grasp_parts(parts, gpu(hand)[:0].contiguous(), gpu(obj)[:0].contiguous(), want_verts=True)
    assert [tuple(empty[k].shape) for k in empty] == [(0, 3), (0, 3), (0, 1), (0,), (0, 4), (0, 4)]


@pytest.mark.gpu
def test_grasp_parts_refuses_what_the_kernel_cannot_hold():
    parts = contact.HandParts(np.zeros(5, np.int64), ["a"], DEV)
    hand = torch.zeros(1, 5, 3, device=DEV)
    with pytest.raises(RuntimeError):
        contact.grasp_parts(parts, hand, torch.zeros(1, 0, 3, device=DEV))
    with pytest.raises(RuntimeError):
        contact.grasp_parts(parts, hand, torch.zeros(2, 4, 3, device=DEV))
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL, nothing launched
    one = torch.full((8192,), 7.0, device=DEV)
    p = one.data_ptr()
    for V, N, P, B in ((2049, 4, 1, 1), (0, 4, 1, 1), (5, 0, 1, 1), (5, 4, 0, 1), (5, 4, 33, 1), (5, 4, 1, -1)):
        rc = lib.dvq_grasp_parts(p, p, V, P, p, 0, 3, 1, B, N, 2.5e-5, p, p, p, p, p, p, None)
        assert rc == 1, (V, N, P, B)
    assert lib.dvq_grasp_parts(p, p, 5, 1, p, 0, 3, 1, 1, 4, 2.5e-5, None, p, p, p, None, None, None) == 1      # a required pointer
    assert lib.dvq_grasp_parts(p, p, 5, 1, p, 0, 3, 1, 0, 4, 2.5e-5, p, p, p, p, None, None, None) == 0         # B = 0: nothing to do
    torch.cuda.synchronize()
    assert (one == 7.0).all()                                           # nothing was written


# ------------------------------------------------------------------------------------------------------ GPU: end to end
# metres, fingers: picked from the values the first run printed.  At 2 cm every candidate of the three near objects has all five
# fingers in contact and at 1 cm they still all agree; at the default 5 mm object 0's candidates have [5, 3, 5, 4, 4, 4, 5, 5], so K = 4
# moves candidate 1 out of the kept set [0, 6, 1] of the run without the guard
E2E_THR, E2E_K = 0.005, 4


@pytest.mark.gpu
def test_best_of_m_with_the_finger_guard_keeps_the_reference_order(tmp_path):
    from test_grasp_select import _gennet
    from test_grasp_wrench import E2E_INDICES, E2E_M, E2E_K as k, E2E_SEED, e2e_clouds
    net = _gennet(tmp_path)
    clouds = e2e_clouds()
    objs = [generate.object_tensor(c) for c in clouds]
    M = E2E_M
    table = contact.HandParts.from_json()
    plain = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES)
    by_pen = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, candidates=M)
    keys0 = set(by_pen[0]["scores"])
    dumped, varied, changed = {}, False, False
    for rows_per_call in (16384, 8, 1):
        got = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, rows_per_call=rows_per_call, candidates=M,
                                            min_fingers=E2E_K, part_threshold=E2E_THR)
        for i, (g, p) in enumerate(zip(got, plain)):
            c = g["candidate"].cpu().numpy()
            assert set(g["scores"]) == keys0                            # "scores" keeps its key set
            obj = np.repeat(objs[i][:3].T.numpy()[None], M, 0)
            want = ref.grasp_parts(p["vertices"].cpu().numpy(), table.labels, 6, obj, E2E_THR * E2E_THR)
            full = {name: t.cpu().numpy() for name, t in g["part_scores"].items()}
            assert tuple(full) == OUTPUTS
            assert_same_bits(full, {name: want[name] for name in OUTPUTS}, what=f"object {i}")
            cls, key = contact.select_keys({name: t.cpu() for name, t in g["scores"].items()}, "penetration", 1)
            cls = np.maximum(cls.numpy(), np.asarray(ref.parts_class(want["part_count"], want["status"], E2E_K, False), np.int32))
            assert np.array_equal(c, score_ref.segment_topk(cls, key.numpy(), 1, M, k)[0]), f"object {i}: order"
            assert torch.equal(g["params"], p["params"][g["candidate"]]) and torch.equal(g["vertices"], p["vertices"][g["candidate"]])
            stats = contact.part_stats(want["part_min"], want["part_count"], want["status"])
            j = g["json"]
            assert list(j)[-4:] == list(FIELDS) + ["hand_contact_map"]
            for f in FIELDS:
                assert j[f] == [stats[f][r] for r in c]
            assert j["hand_contact_map"] == ref.contact_map(want["mask"][c], 778) and len(j["hand_contact_map"]) == 778
            assert all(torch.equal(g["parts"][name].cpu(), g["part_scores"][name].cpu()[c]) for name in OUTPUTS)
            fingers = stats["fingers_in_contact"]
            print(f"rows_per_call {rows_per_call} object {i}: kept {c.tolist()} (without the guard {by_pen[i]['candidate'].tolist()}) "
                  f"fingers {fingers} cls {cls.tolist()} part_dist of candidate 0 {stats['part_dist'][0]}")
            varied |= len(set(fingers)) >= 2
            changed |= c.tolist() != by_pen[i]["candidate"].tolist()
            if i == 3:
                assert fingers == [0] * M and j["fingers_in_contact"] == [0] * k, "the far object's hands touch nothing"
        text = [json.dumps(g["json"]) for g in got]
        assert "Infinity" not in "".join(text) and "NaN" not in "".join(text)
        dumped[rows_per_call] = text
    assert dumped[8] == dumped[16384] and dumped[1] == dumped[16384]
    assert varied and changed, "the guard is not exercised"
    # parts=True without candidates: the fields for every grasp generated, and the parameters of the plain run
    figures = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES, parts=True, part_threshold=E2E_THR)
    for i, (g, p) in enumerate(zip(figures, plain)):
        j, q = g["json"], p["json"]
        assert {f: j[f] for f in q} == q and list(j)[len(q):] == list(FIELDS) + ["hand_contact_map"]
        assert torch.equal(g["params"], p["params"]) and torch.equal(g["vertices"], p["vertices"])
        full = got[i]["part_scores"]                                    # of the last best-of-M run above: all M candidates
        assert all(torch.equal(g["parts"][name], full[name]) for name in OUTPUTS) and "part_scores" not in g
        assert all(len(j[f]) == M for f in FIELDS) and sum(j["hand_contact_map"]) == int(full["part_count"].sum())


def _run_main(dataset, out_dir, extra, mano):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


def _cloud_files(tmp_path):
    from test_grasp_wrench import e2e_clouds
    files = []
    for i, c in enumerate(e2e_clouds()):
        files.append(str(tmp_path / f"cloud{i}.npy"))
        np.save(files[-1], c)
    return files


@pytest.mark.gpu
def test_entry_point_writes_the_parts_fields(tmp_path):
    from test_grasp_select import mano_pkl
    from test_grasp_wrench import E2E_K as k, E2E_M
    mano = mano_pkl(tmp_path)
    base = ["--objects"] + _cloud_files(tmp_path) + ["--num_grasp", str(k), "--candidates", str(E2E_M)]
    flags = base + ["--parts", "1", "--min_fingers", str(E2E_K), "--part_threshold", str(E2E_THR)]
    names0, bytes0 = _run_main("obman", str(tmp_path / "p16384"), flags + ["--rows_per_call", "16384"], mano)
    assert names0 == [f"obj_id_cloud{i}.json" for i in range(4)]
    pooled_text = open(str(tmp_path / "p16384" / "hand_contact.json"), "rb").read()
    for tag in ("0", "8"):
        names, data = _run_main("obman", str(tmp_path / f"p{tag}"), flags + ["--rows_per_call", tag], mano)
        assert names == names0 and data == bytes0, f"--rows_per_call {tag}: the files differ"
        assert open(str(tmp_path / f"p{tag}" / "hand_contact.json"), "rb").read() == pooled_text
    maps, fingers = [], []
    for i, data in enumerate(bytes0):
        j = json.loads(data)                                            # strict JSON: no Infinity, no NaN
        assert b"Infinity" not in data and b"NaN" not in data
        assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact",
                          *FIELDS, "hand_contact_map"}
        assert all(len(j[f]) == k for f in FIELDS) and all(len(row) == 6 for row in j["part_contact"] + j["part_dist"])
        assert len(j["hand_contact_map"]) == 778 and all(isinstance(x, int) and 0 <= x <= k for x in j["hand_contact_map"])
        assert sum(j["hand_contact_map"]) == sum(sum(row) for row in j["part_contact"])
        assert j["fingers_in_contact"] == [sum(1 for x in row[:5] if x >= 1) for row in j["part_contact"]]
        if i == 3:                                                      # the far object: no hand touches it
            assert j["fingers_in_contact"] == [0] * k and sum(j["hand_contact_map"]) == 0
        maps.append(j["hand_contact_map"])
        fingers += j["fingers_in_contact"]
    assert b"Infinity" not in pooled_text and b"NaN" not in pooled_text
    pooled = json.loads(pooled_text)
    assert pooled["parts"] == contact.HandParts.from_json().names and pooled["threshold"] == E2E_THR and pooled["grasps"] == 4 * k
    assert pooled["hand_contact_map"] == [sum(col) for col in zip(*maps)]
    assert pooled["fingers_histogram"] == [fingers.count(x) for x in range(6)] and sum(pooled["fingers_histogram"]) == 4 * k
    assert abs(pooled["mean_fingers_in_contact"] - sum(fingers) / len(fingers)) < 1e-12


@pytest.mark.gpu
def test_entry_point_without_the_flags_writes_the_parents_bytes(tmp_path):
    """``--parts 0 --min_fingers 0 --need_thumb 0`` (and a value for the dependent flag) against a run that omits them all: the code
    path of the parent commit, the same bytes, and no hand_contact.json."""
    from test_grasp_select import mano_pkl
    from test_grasp_wrench import E2E_K as k, E2E_M
    mano = mano_pkl(tmp_path)
    base = ["--objects"] + _cloud_files(tmp_path) + ["--num_grasp", str(k), "--candidates", str(E2E_M)]
    names0, plain = _run_main("obman", str(tmp_path / "plain"), base, mano)
    names, off = _run_main("obman", str(tmp_path / "off"), base + ["--parts", "0", "--min_fingers", "0", "--need_thumb", "0",
                                                                   "--part_threshold", "0.01"], mano)
    assert names == names0 and off == plain and not os.path.exists(str(tmp_path / "off" / "hand_contact.json"))
    assert all(set(json.loads(d)) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact"}
               for d in plain)
