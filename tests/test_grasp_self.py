"""Finger-to-finger collision: the fused kernel (dvq_grasp_self), its host API (ops.grasp_self, contact.SelfTable / grasp_self /
self_stats / self_class) and the ``--self_collision`` / ``--max_self_verts`` mode of the entry points.  The reference is
tests/grasp_self_ref.py (numpy over oracle/contact_oracle); GPU results are compared with it bit for bit, no tolerance anywhere."""
import functools
import json
import lzma
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, mano as dmano, ops, synth

import grasp_self_ref as ref
import grasp_score_ref as score_ref
import mano_ref

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
REACH, MARGIN = 0.01, 0.001                                              # metres: the defaults
OUTPUTS = ("pen_count", "pen_depth", "gap_min", "pair_bits", "mask", "status")
FIELDS = ("self_penetrating", "self_part_penetrating", "self_depth", "self_pairs", "self_clearance")
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_self_collision_flags(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.self_collision, a.self_reach, a.self_margin, a.self_seam, a.self_palm, a.max_self_verts) == (0, 0.01, 0.001, 2, 1, None)
    a = generate.parse_args(dataset, ["--self_collision", "1", "--self_reach", "0.006", "--self_margin", "0", "--self_seam", "0",
                                      "--self_palm", "0", "--max_self_verts", "0", "--candidates", "200", "--num_grasp", "100"])
    assert (a.self_collision, a.self_reach, a.self_margin, a.self_seam, a.self_palm, a.max_self_verts) == (1, 0.006, 0.0, 0, 0, 0)
    assert generate.parse_args(dataset, ["--self_collision", "1"]).self_collision == 1   # the figures alone need no candidates
    cand = ["--candidates", "200", "--num_grasp", "100"]
    for bad in (["--self_reach", "0"], ["--self_reach", "-0.01"], ["--self_reach", "inf"], ["--self_reach", "nan"],
                ["--self_margin", "-0.001"], ["--self_margin", "inf"], ["--self_margin", "nan"], ["--self_seam", "-1"],
                ["--self_collision", "2"], ["--self_palm", "2"], ["--max_self_verts", "-1"] + cand, ["--max_self_verts", "3"],
                ["--max_self_verts", "x"] + cand):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_grasp_self" in _lib.SIGNATURES and "int dvq_grasp_self(" in header and hasattr(lib, "dvq_grasp_self")
    assert "dvq_grasp_self" in re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert len(_lib.SIGNATURES["dvq_grasp_self"][1]) == 19
    assert lib.dvq_abi_version() == 10 and ops.GRASP_SELF_MAX_P == 32


def test_ops_refuse_bad_arguments_before_any_device_use():
    V = 6
    faces, vf_off, vf_face = (torch.from_numpy(x) for x in contact.face_csr([[0, 1, 2], [3, 4, 5]], V))
    hand = torch.zeros(1, V, 3)
    labels = torch.tensor([0, 0, 1, 1, 2, 2], dtype=torch.int32)
    source = torch.ones(V, dtype=torch.int32)
    good = dict(hand=hand, faces=faces, vf_off=vf_off, vf_face=vf_face, part_of_vertex=labels, source_of_vertex=source, n_parts=3,
                pairs=[0b110, 0b101, 0b000], reach2=1e-4, margin=1e-3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_self(**good)                                                        # well-formed, but not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_self(**{**good, "pairs": np.asarray([6, 5, 0], np.uint32), "margin": 0.0})
    big = 2049
    csr0 = [torch.from_numpy(x) for x in contact.face_csr(np.zeros((0, 3), np.int64), 0)]
    csr_big = [torch.from_numpy(x) for x in contact.face_csr([[0, 1, 2]], big)]
    for bad in (dict(hand=torch.zeros(1, big, 3), faces=csr_big[0], vf_off=csr_big[1], vf_face=csr_big[2],
                     part_of_vertex=torch.zeros(big, dtype=torch.int32), source_of_vertex=torch.ones(big, dtype=torch.int32)),   # V = 2049
                dict(hand=torch.zeros(1, 0, 3), faces=csr0[0], vf_off=csr0[1], vf_face=csr0[2], part_of_vertex=labels[:0],
                     source_of_vertex=source[:0]),                                                                            # V = 0
                dict(n_parts=0, pairs=[]), dict(n_parts=33, pairs=[0] * 33),                                                   # P outside 1 .. 32
                dict(pairs=[0b111, 0b101, 0]), dict(pairs=[0b110, 0b101, 0b100]),                                              # a part against itself
                dict(pairs=[0b1110, 0b101, 0]), dict(pairs=[0b110, 0b101, 1 << 31]), dict(pairs=[-2, 0, 0]),                   # a bit at or above P
                dict(pairs=[0b110, 0b101]), dict(pairs=[0b110, 0b101, 0, 0]),                                                  # wrong length
                dict(reach2=0.0), dict(reach2=-1e-4), dict(reach2=INF), dict(reach2=NAN),
                dict(margin=-1e-3), dict(margin=INF), dict(margin=NAN),
                dict(hand=hand.double()), dict(part_of_vertex=labels.long()), dict(source_of_vertex=source.long()),            # wrong dtype
                dict(source_of_vertex=source.bool()), dict(faces=faces.long()), dict(vf_off=vf_off.long()),
                dict(hand=torch.zeros(1, 3, V).transpose(1, 2)), dict(hand=hand.expand(2, -1, -1)),                            # not contiguous
                dict(part_of_vertex=torch.zeros(2 * V, dtype=torch.int32)[::2]), dict(source_of_vertex=torch.ones(2 * V, dtype=torch.int32)[::2]),
                dict(part_of_vertex=labels[:5]), dict(source_of_vertex=torch.ones(V + 1, dtype=torch.int32)),                  # wrong lengths
                dict(vf_off=vf_off[:-1]), dict(vf_face=vf_face[:-1]), dict(hand=torch.zeros(1, V, 4)), dict(hand=torch.zeros(V, 3))):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_self(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"
    parts = contact.HandParts(labels.numpy(), ["a", "b", "c"])
    table = contact.SelfTable(parts, faces.numpy(), seam=0, n_fingers=2)
    topo = contact.HandTopology(faces.numpy(), V, "cpu")
    for kw in (dict(reach=0.0), dict(reach=-0.01), dict(reach=INF), dict(reach=NAN), dict(margin=-0.001), dict(margin=INF), dict(margin=NAN)):
        with pytest.raises(RuntimeError, match="reach|margin"):
            contact.grasp_self(topo, table, hand, **kw)
    with pytest.raises(RuntimeError, match="6 vertices"):                             # the table's vertex count and V disagree
        contact.grasp_self(topo, table, torch.zeros(1, 7, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        contact.grasp_self(topo, table, hand)


@functools.lru_cache(maxsize=None)
def mano_arrays():
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "MANO_RIGHT.pkl")
        with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
        return dmano.read_mano_pkl(path)


def test_self_table_seams_and_pairs():
    parts = contact.HandParts.from_json()
    faces = np.asarray(mano_arrays()["faces"])
    for seam, n in ((0, 0), (1, 112), (2, 210), (3, 297)):
        table = contact.SelfTable(parts, faces, seam=seam)
        assert table.n_seam == n and int((table.source == 0).sum()) == n and table.source.dtype == np.int32
        assert table.source.tolist() == ref.seam_sources(parts.labels, faces, seam), seam
    assert contact.SelfTable(parts, faces, seam=0).source.tolist() == [1] * 778
    assert contact.SelfTable(parts, faces).seam == 2 and contact.SelfTable(parts, faces).n_seam == 210     # the default
    with_palm, without = contact.SelfTable(parts, faces), contact.SelfTable(parts, faces, palm=False)
    assert with_palm.pairs.dtype == np.uint32
    assert with_palm.pairs.tolist() == [0b111110, 0b111101, 0b111011, 0b110111, 0b101111, 0] == ref.default_pairs(6, True)
    assert without.pairs.tolist() == [0b011110, 0b011101, 0b011011, 0b010111, 0b001111, 0] == ref.default_pairs(6, False)
    # a hand-made table of 8 vertices: a strip of six triangles, three parts, vertex 7 unlabelled
    #   0 - 1 - 2 - 3        labels 0 0 1 1
    #   | / | / | / |
    #   4 - 5 - 6 - 7        labels 0 2 2 -
    strip = [[0, 4, 1], [1, 4, 5], [1, 5, 2], [2, 5, 6], [2, 6, 3], [3, 6, 7]]
    small = contact.HandParts([0, 0, 1, 1, 0, 2, 2, 9], ["a", "b", "c"])
    assert contact.SelfTable(small, strip, seam=1, n_fingers=2).source.tolist() == [1, 0, 0, 0, 0, 0, 0, 0]    # 3 - 7: an unlabelled vertex is another label
    assert contact.SelfTable(small, strip, seam=2, n_fingers=2).source.tolist() == [0] * 8
    assert contact.SelfTable(small, strip, seam=0, n_fingers=2).source.tolist() == [1] * 8
    for seam in (0, 1, 2):
        assert contact.SelfTable(small, strip, seam=seam, n_fingers=2).source.tolist() == ref.seam_sources(small.labels, strip, seam)
    assert contact.SelfTable(small, strip, n_fingers=2).pairs.tolist() == [0b110, 0b101, 0]
    assert contact.SelfTable(small, strip, n_fingers=2, palm=False).pairs.tolist() == [0b010, 0b001, 0]
    assert contact.SelfTable(small, strip, n_fingers=3).pairs.tolist() == [0b110, 0b101, 0b011]
    given = contact.SelfTable(small, strip, pairs=[0b100, 0, 0], source=[1, 1, 0, 0, 5, 0, 0, 1])               # passed outright
    assert given.pairs.tolist() == [4, 0, 0] and given.source.tolist() == [1, 1, 0, 0, 1, 0, 0, 1] and given.n_seam == 4
    for kw in (dict(seam=-1), dict(n_fingers=-1), dict(pairs=[1, 0, 0]), dict(pairs=[8, 0, 0]), dict(pairs=[2, 1]), dict(source=[1] * 7),
               dict(source=np.ones(8))):
        with pytest.raises(RuntimeError):
            contact.SelfTable(small, strip, **kw)
    with pytest.raises(RuntimeError):
        contact.SelfTable(small, [[0, 1, 8]])


def test_host_statistics_equal_independent_code():
    rng = np.random.default_rng(12)
    B, P = 9, 6
    out = {"pen_count": rng.integers(0, 3, size=(B, P)).astype(np.int32), "pen_depth": (rng.random((B, P)) * 5e-3).astype(f32),
           "gap_min": (rng.random((B, P)) * 1e-4).astype(f32), "pair_bits": rng.integers(0, 64, size=(B, P)).astype(np.int32),
           "status": np.zeros(B, np.int32)}
    out["pen_count"][1] = 0                                                           # a clean row
    out["pen_depth"][1], out["pair_bits"][1] = 0.0, 0
    out["gap_min"][2, 5] = np.inf                                                     # a part without a source
    out["gap_min"][3] = np.inf                                                        # a row without any
    out["status"][5] = 1
    out["pen_count"][5], out["pen_depth"][5], out["gap_min"][5], out["pair_bits"][5] = -1, np.nan, np.nan, 0
    got = contact.self_stats({k: torch.from_numpy(v) for k, v in out.items()})
    want = ref.self_stats(out)
    assert tuple(got) == FIELDS and all(len(got[k]) == B for k in FIELDS)
    for b, w in enumerate(want):
        if w is None:
            assert b == 5 and all(got[k][b] is None for k in FIELDS)
            continue
        assert got["self_penetrating"][b] == w[0] and got["self_part_penetrating"][b] == w[1] and got["self_pairs"][b] == w[3]
        assert abs(got["self_depth"][b] - w[2]) <= 1e-15 * w[2]                      # one float64 product
        assert (got["self_clearance"][b] is None) == (w[4] is None) and (w[4] is None or abs(got["self_clearance"][b] - w[4]) <= 1e-15 * w[4])
    assert got["self_penetrating"][1] == 0 and got["self_pairs"][1] == [] and got["self_depth"][1] == 0.0
    assert got["self_clearance"][3] is None and got["self_clearance"][2] is not None
    text = json.dumps(got)
    assert "NaN" not in text and "Infinity" not in text and json.loads(text)["self_penetrating"][5] is None
    wide = {k: np.zeros((1, 32), v.dtype) for k, v in out.items() if k != "status"}     # bit 31 of a word is the int32's sign
    wide["status"] = np.zeros(1, np.int32)
    wide["pair_bits"][0, 0] = -2 ** 31
    wide["pair_bits"][0, 31] = 1
    assert contact.self_stats(wide)["self_pairs"] == [[[0, 31], [31, 0]]] == [ref.self_stats(wide)[0][3]]
    dev = {k: torch.from_numpy(v) for k, v in out.items()}
    seen = set()
    for k in (0, 1, 3, 6, 100):
        cls = contact.self_class(dev, k)
        assert cls.dtype == torch.int32 and cls.tolist() == ref.self_class(out["pen_count"], out["status"], k)
        seen |= set(cls.tolist())
    assert seen == {0, 1, 2} and contact.self_class(dev, 100).tolist() == [0, 0, 0, 0, 0, 2, 0, 0, 0]
    assert contact.self_class(dev, 0)[1].item() == 0 and contact.SELECT_BY == ("penetration", "log_prob", "stability")   # a guard only


# ------------------------------------------------------------------------------------------------------ CPU: calibration on the real model
@functools.lru_cache(maxsize=None)
def calibration_hands():
    """The 48 hands of the calibration -- 12 shapes (betas ~ N(0,1), the first zero), each under the zero pose and under a PCA pose
    ~ N(0, 0.3^2), with flat_hand_mean on and off -- and the overlays: the flat hand with zero betas whose index finger is moved towards
    the middle finger by the whole and by half of the vector between the two parts' centroids.  fp32 [50,778,3], the float64
    reference of tests/mano_ref.py rounded once."""
    arrays = mano_ref.device_arrays(mano_arrays())
    betas = synth.synthetic_normal((12, 10), 71, "self/betas", 1.0).double().numpy()
    betas[0] = 0.0
    pose = synth.synthetic_normal((12, 45), 71, "self/pose", 0.3).double().numpy()
    hands = [mano_ref.mano_ref(arrays, betas, p, flat_hand_mean=flat)[0] for flat in (True, False) for p in (np.zeros_like(pose), pose)]
    labels = contact.HandParts.from_json().labels
    flat0 = hands[0][0]
    shift = flat0[labels == 2].mean(0) - flat0[labels == 1].mean(0)
    assert abs(np.linalg.norm(shift) - 0.0348) < 5e-4 and int((labels == 1).sum()) == 123
    for share in (1.0, 0.5):
        over = flat0.copy()
        over[labels == 1] += share * shift
        hands.append(over[None])
    out = np.concatenate(hands).astype(f32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def calibration_reference(seam, palm):
    parts = contact.HandParts.from_json()
    faces = np.asarray(mano_arrays()["faces"])
    table = contact.SelfTable(parts, faces, seam=seam, palm=palm)
    return ref.grasp_self(calibration_hands(), faces, parts.labels, table.source, 6, table.pairs, REACH * REACH, MARGIN)


def test_calibration_on_the_real_hand_model():
    """The two caps of the issue as conditions: no false alarm on the 48 hands at the defaults and at fingers-only with one seam ring;
    the whole and the half overlay of the index on the middle finger give at least 30 and at least 8 penetrating vertices at the
    defaults (47 and 11 were observed when the rule was chosen), with both parts in the pairs."""
    for seam, palm in ((2, True), (1, False)):
        want = calibration_reference(seam, palm)
        stats = contact.self_stats(want)
        print(f"seam {seam} palm {palm}: penetrating {stats['self_penetrating']} clearance (cm) min "
              f"{min(stats['self_clearance'][:48]):.3f} overlays depth (cm) {stats['self_depth'][48:]} pairs {stats['self_pairs'][48:]}")
        assert want["status"].tolist() == [0] * 50
        assert stats["self_penetrating"][:48] == [0] * 48, "a false alarm on a hand that does not collide"
        assert all(d == 0.0 and p == [] for d, p in zip(stats["self_depth"][:48], stats["self_pairs"][:48]))
        assert (want["mask"][:48] == 0).all()
    stats = contact.self_stats(calibration_reference(2, True))
    full, half = stats["self_penetrating"][48:]
    assert full >= 30 and half >= 8, (full, half)
    for b in (48, 49):
        hit = {a for ab in stats["self_pairs"][b] for a in ab}
        assert {1, 2} <= hit and stats["self_part_penetrating"][b][1] > 0 and stats["self_part_penetrating"][b][2] > 0
        assert stats["self_depth"][b] > 100.0 * MARGIN
        assert contact.contact_map(calibration_reference(2, True)["mask"][b:b + 1], 778).sum() == stats["self_penetrating"][b]


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.array(a))).to(DEV)


def scene(tag, B, V, P, F=None, box=0.012):
    """B random vertex sets in a box of 1.2 cm with F random triangles and labels v mod P: within a reach of 1 cm nearly every vertex has
    a target, and about half of them lie behind its tangent plane."""
    F = F if F is not None else 2 * V
    hand = synth.synthetic_uniform((B, V, 3), 72, f"self/{tag}/h", -box / 2, box / 2).numpy().astype(f32)
    rng = np.random.default_rng([72, V, F])
    faces = np.stack([rng.permutation(V)[:3] for _ in range(F)]).astype(np.int64) if V >= 3 else np.zeros((1, 3), np.int64)
    labels = (np.arange(V) % P).astype(np.int64)
    return hand, faces, labels


def ring_pairs(P):
    return [((1 << P) - 1) & ~(1 << a) for a in range(P)]


def run_self(hand, faces, labels, source, P, pairs, reach2=REACH * REACH, margin=MARGIN):
    V = hand.shape[1]
    topo = contact.HandTopology(faces, V, DEV)
    out = ops.grasp_self(gpu(hand), topo.faces, topo.vf_off, topo.vf_face, gpu(np.asarray(labels, np.int32)),
                         gpu(np.asarray(source, np.int32)), P, pairs, reach2, margin)
    out = dict(zip(OUTPUTS, out))
    B = hand.shape[0]
    assert [tuple(out[k].shape) for k in OUTPUTS] == [(B, P)] * 4 + [(B, (V + 31) // 32), (B,)]
    assert all(out[k].dtype == (torch.float32 if k in ("pen_depth", "gap_min") else torch.int32) for k in OUTPUTS)
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same_bits(got, want, rows=None, what=""):
    """Every number bit for bit; a NaN is a NaN (its payload is nobody's contract)."""
    for k in OUTPUTS:
        g, w = (got[k], want[k]) if rows is None else (got[k][rows], want[k][rows])
        if g.dtype != np.float32:
            assert np.array_equal(g, w), (what, k, g, w)
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, k, g, w)
        assert np.array_equal(bits(g)[~nan], bits(w)[~nan]), (what, k, g, w)


def both(hand, faces, labels, source, P, pairs, reach2=REACH * REACH, margin=MARGIN, what=""):
    got = run_self(hand, faces, labels, source, P, pairs, reach2, margin)
    want = ref.grasp_self(hand, faces, labels, source, P, pairs, reach2, margin)
    print(what, "pen_count", got["pen_count"].tolist(), "pair_bits", got["pair_bits"].tolist(), "mask", got["mask"].tolist()[:2])
    assert_same_bits(got, want, what=what)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("V", [4, 5, 6, 7, 33, 64, 65])
def test_grasp_self_equals_the_reference_bit_for_bit(V):
    """V = 4: one whole sixteen-byte block and no tail; 5, 6, 7: the tail behind the sixteen-byte reads and the padding of the one mask
    word; 33, 64, 65: a second mask word, a whole wave's ballot and one vertex past it."""
    P = 3
    hand, faces, labels = scene(f"small{V}", 3, V, P)
    got, want = both(hand, faces, labels, np.ones(V), P, ring_pairs(P), what=f"V={V}")
    assert want["status"].tolist() == [0] * 3 and want["pen_count"].sum() > 0 and (want["vert_idx"] >= 0).all()
    assert (want["pen_count"].sum(axis=1) < V).all(), "every vertex penetrates: the test cannot see a missed one"
    if V % 32:                                                           # the unused high bits of the last word are 0
        assert (got["mask"].view(np.uint32)[:, -1] >> np.uint32(V % 32) == 0).all()


@pytest.mark.gpu
def test_grasp_self_on_the_real_hand():
    """V = 778: the 48 hands of the calibration and the two overlays, on the packaged table, through contact.grasp_self."""
    parts = contact.HandParts.from_json()
    faces = np.asarray(mano_arrays()["faces"])
    topo = contact.HandTopology(faces, 778, DEV)
    hands = calibration_hands()
    for seam, palm in ((2, True), (1, False)):
        table = contact.SelfTable(parts, faces, seam=seam, palm=palm, device=DEV)
        out = contact.grasp_self(topo, table, gpu(hands))
        assert tuple(out) == OUTPUTS
        got = {k: v.cpu().numpy() for k, v in out.items()}
        want = calibration_reference(seam, palm)
        assert_same_bits(got, want, what=f"seam {seam} palm {palm}")
        stats = contact.self_stats(out)
        assert stats["self_penetrating"][:48] == [0] * 48 and contact.self_class(out, 0).tolist() == [0] * 48 + [1, 1]
    assert stats["self_penetrating"][48] >= 8 and min(stats["self_clearance"]) > 0.0


@pytest.mark.gpu
def test_grasp_self_at_the_maximum_size():
    """V = 2048, one grasp: the second pass over the planes, all 64 mask words, the largest LDS image."""
    V, P = 2048, 6
    hand, faces, labels = scene("max", 1, V, P, F=4000, box=0.05)
    labels[::7] = -1
    source = (np.arange(V) % 5 != 0).astype(np.int32)
    got, want = both(hand, faces, labels, source, P, contact.SelfTable(contact.HandParts(labels, list("abcdef")), faces, source=source).pairs,
                     what="V=2048")
    assert want["pen_count"][0, :5].min() > 0 and want["pen_count"][0, 5] == 0 and (want["mask"][0, 32:] != 0).any()
    assert (want["vert_idx"][0, 1024:] >= 1024).any() and (want["vert_idx"][0, 1024:] < 1024).any()


@pytest.mark.gpu
def test_grasp_self_small_batches_and_rows_alone():
    """B = 0 writes nothing; a row's outputs are the same alone, in a batch of 3, and with a NaN and an Inf row beside it."""
    V, P = 70, 4
    hand, faces, labels = scene("batch", 3, V, P)
    source, pairs = np.ones(V), ring_pairs(P)
    three, want = both(hand, faces, labels, source, P, pairs, what="B=3")
    assert len({x.tobytes() for x in three["pen_count"]}) == 3, "the three rows are alike"
    for b in range(3):
        one = run_self(hand[b:b + 1], faces, labels, source, P, pairs)
        assert_same_bits(one, {k: x[b:b + 1] for k, x in three.items()}, what=f"row {b} alone")
    bad = np.concatenate([hand, hand[:2]])
    bad[1, 69, 2] = np.nan
    bad[3, 0, 0] = np.inf
    got, _ = both(bad, faces, labels, source, P, pairs, what="non-finite rows")
    assert got["status"].tolist() == [0, 1, 0, 1, 0]
    for b in (1, 3):
        assert np.isnan(got["pen_depth"][b]).all() and np.isnan(got["gap_min"][b]).all() and (got["pen_count"][b] == -1).all()
        assert (got["pair_bits"][b] == 0).all() and (got["mask"][b] == 0).all()
    assert_same_bits(got, {k: np.concatenate([x, x[:2]]) for k, x in three.items()}, rows=[0, 2, 4], what="the rows beside them")
    out = {k: torch.from_numpy(x) for k, x in got.items()}
    assert contact.self_class(out, 10 ** 6).tolist() == [0, 2, 0, 2, 0]
    assert [s is None for s in contact.self_stats(out)["self_penetrating"]] == [False, True, False, True, False]
    # B = 0: the shapes, and nothing written through the C ABI
    empty = run_self(hand[:0], faces, labels, source, P, pairs)
    assert all(x.shape[0] == 0 for x in empty.values())
    lib = _lib.load()
    one = torch.full((8192,), 7.0, device=DEV)
    p = one.data_ptr()
    host = (np.asarray(pairs, np.uint32)).ctypes.data
    assert lib.dvq_grasp_self(p, p, p, p, 5, p, p, 4, host, 0, 1e-4, 1e-3, p, p, p, p, p, p, None) == 0
    for V_, P_, B_, r2, mg in ((2049, 4, 1, 1e-4, 1e-3), (0, 4, 1, 1e-4, 1e-3), (5, 0, 1, 1e-4, 1e-3), (5, 33, 1, 1e-4, 1e-3),
                               (5, 4, -1, 1e-4, 1e-3), (5, 4, 1, 0.0, 1e-3), (5, 4, 1, INF, 1e-3), (5, 4, 1, NAN, 1e-3),
                               (5, 4, 1, 1e-4, -1e-3), (5, 4, 1, 1e-4, NAN), (5, 4, 1, 1e-4, INF)):
        assert lib.dvq_grasp_self(p, p, p, p, V_, p, p, P_, host, B_, r2, mg, p, p, p, p, p, p, None) == 1, (V_, P_, B_, r2, mg)
    assert lib.dvq_grasp_self(p, p, p, p, 5, p, p, 4, host, 1, 1e-4, 1e-3, None, p, p, p, p, p, None) == 1       # a null pointer
    assert lib.dvq_grasp_self(p, p, p, p, 5, p, p, 4, None, 1, 1e-4, 1e-3, p, p, p, p, p, p, None) == 1
    for words in ([0b0001, 0, 0, 0], [0, 0, 0, 0b1000], [0b10000, 0, 0, 0]):                                      # itself; a bit at P
        assert lib.dvq_grasp_self(p, p, p, p, 5, p, p, 4, np.asarray(words, np.uint32).ctypes.data, 1, 1e-4, 1e-3, p, p, p, p, p, p, None) == 1
    torch.cuda.synchronize()
    assert (one == 7.0).all()                                           # nothing was written


def wedge(extra=0):
    """A triangle (u, p1, p2) in the plane z = 0 whose normal is +z, and a vertex v 3 mm below u: v lies behind u's tangent plane by
    exactly its distance to u.  Labels: v = 0, u = 1, the rest unlabelled; `extra` far vertices pad V."""
    pts = [[0.0, 0.0, -0.003], [0.0, 0.0, 0.0], [0.01, 0.0, 0.0], [0.0, 0.01, 0.0]] + [[1.0 + i, 1.0, 1.0] for i in range(extra)]
    return np.asarray([pts], f32), np.asarray([[1, 2, 3]]), np.asarray([0, 1, -1, -1] + [-1] * extra)


@pytest.mark.gpu
def test_grasp_self_ties_take_the_lowest_index():
    hand, faces, labels = wedge(extra=5)                                 # V = 9
    hand[0, 6] = hand[0, 1]                                              # duplicates of u further up: the same d, another normal (none)
    hand[0, 8] = hand[0, 1]
    labels[[6, 8]] = 1
    got, want = both(hand, faces, labels, np.ones(9), 2, [0b10, 0b01], what="ties")
    assert want["vert_idx"][0, 0] == 1 and want["pen_count"].tolist() == [[1, 0]] and want["mask"].tolist() == [[1]]
    assert 0.0029 < want["pen_depth"][0, 0] < 0.0031 and want["pair_bits"].tolist() == [[2, 0]]
    # the triangle moved to the duplicate at index 6: vertex 1, the lowest index, has no face (normal 0, depth 0) and still wins
    got2, want2 = both(hand, np.asarray([[6, 2, 3]]), labels, np.ones(9), 2, [0b10, 0b01], what="ties, the faceless duplicate first")
    assert want2["vert_idx"][0, 0] == 1 and want2["pen_count"].tolist() == [[0, 0]] and bits(want2["gap_min"])[0, 0] == bits(want["gap_min"])[0, 0]


@pytest.mark.gpu
def test_grasp_self_label_sets():
    """No targets (P = 1), the widest label set (P = 32), an empty part, unlabelled vertices, asymmetric pairs, no source at all."""
    V = 40
    hand, faces, _ = scene("labels", 2, V, 1)
    ones = np.ones(V)
    # P = 1: a part has nothing to be tested against
    got, want = both(hand, faces, np.zeros(V, np.int64), ones, 1, [0], what="P=1")
    assert np.isposinf(got["gap_min"]).all() and (want["vert_idx"] == -1).all() and (got["pen_count"] == 0).all()
    assert (got["mask"] == 0).all() and (got["pair_bits"] == 0).all() and (bits(got["pen_depth"]) == 0).all()
    # P = 32: part 0 against part 31 -- bit 31 comes back as the int32's sign
    wh, wf, wl = wedge(extra=3)
    wl[1] = 31
    got, want = both(wh, wf, wl, np.ones(7), 32, [1 << 31] + [0] * 31, what="P=32")
    assert got["pair_bits"][0, 0] == -2 ** 31 and got["pen_count"][0].tolist() == [1] + [0] * 31
    assert contact.self_stats(got)["self_pairs"] == [[[0, 31]]]
    labels32 = (np.arange(V) % 32).astype(np.int64)
    got, want = both(hand, faces, labels32, ones, 32, ring_pairs(32), what="P=32, every pair")
    assert want["pen_count"].sum() > 0
    # an empty part (2) and unlabelled vertices (labels 4 and -1 at P = 4... outside [0, P))
    labels = (np.arange(V) % 6).astype(np.int64)
    labels[labels == 2] = 7
    labels[labels == 5] = -1
    got, want = both(hand, faces, labels, ones, 5, ring_pairs(5), what="empty part, unlabelled vertices")
    assert got["pen_count"][:, 2].tolist() == [0, 0] and (bits(got["pen_depth"][:, 2]) == 0).all() and np.isposinf(got["gap_min"][:, 2]).all()
    assert (got["pair_bits"][:, 2] == 0).all() and (got["pair_bits"] & 0b100 == 0).all() and want["pen_count"].sum() > 0
    off = np.flatnonzero((labels < 0) | (labels >= 5))
    m = got["mask"].view(np.uint32)
    assert all(((m[:, v >> 5] >> np.uint32(v & 31)) & 1 == 0).all() for v in off), "an unlabelled vertex is no source"
    assert not np.isin(want["vert_idx"], off).any(), "an unlabelled vertex is no target"
    # asymmetric pairs: 0 against 1, not 1 against 0
    labels = (np.arange(V) % 2).astype(np.int64)
    got, want = both(hand, faces, labels, ones, 2, [0b10, 0], what="asymmetric")
    assert (got["pen_count"][:, 0] > 0).all() and (got["pen_count"][:, 1] == 0).all() and np.isposinf(got["gap_min"][:, 1]).all()
    assert np.isfinite(got["gap_min"][:, 0]).all() and (got["mask"].view(np.uint32) & np.uint32(0xaaaaaaaa) == 0).all()
    # every vertex a seam vertex
    got, want = both(hand, faces, labels, np.zeros(V), 2, [0b10, 0b01], what="all seam")
    assert (got["pen_count"] == 0).all() and np.isposinf(got["gap_min"]).all() and (got["mask"] == 0).all()
    # half of them: only sources count, all remain targets
    half = (np.arange(V) % 4 < 2).astype(np.int32)
    got, want = both(hand, faces, labels, half, 2, [0b10, 0b01], what="half seam")
    assert want["pen_count"].sum() > 0 and (half[want["vert_idx"][0][half != 0]] == 0).any(), "no seam vertex is a target"
    # coordinates whose squares overflow: every distance is +inf, the lowest target attains it, nothing is within reach
    far = (hand * f32(1e33)).astype(f32)
    got, want = both(far, faces, labels, ones, 2, [0b10, 0b01], what="overflow")
    assert np.isposinf(got["gap_min"]).all() and (got["pen_count"] == 0).all() and got["status"].tolist() == [0, 0]


@pytest.mark.gpu
def test_grasp_self_thresholds_are_strict():
    """d exactly reach2 and depth exactly margin do not count; one ulp to the generous side does."""
    hand, faces, labels = wedge(extra=1)                                 # V = 5
    src, pairs = np.ones(5), [0b10, 0]
    base = ref.grasp_self(hand, faces, labels, src, 2, pairs, 1.0, 0.0)
    d, depth = f32(base["vert_dist"][0, 0]), f32(base["vert_depth"][0, 0])
    assert d > 0 and depth > 0 and base["pen_count"].tolist() == [[1, 0]]
    up, down = np.nextafter(d, f32(np.inf)), np.nextafter(depth, f32(0))
    for reach2, margin, n in ((d, 0.0, 0), (up, 0.0, 1), (1.0, depth, 0), (1.0, down, 1), (d, down, 0), (up, depth, 0), (up, down, 1)):
        got, want = both(hand, faces, labels, src, 2, pairs, float(reach2), float(margin), what=f"reach2 {reach2!r} margin {margin!r}")
        assert got["pen_count"].tolist() == [[n, 0]] and got["mask"].tolist() == [[n]], (reach2, margin)
        assert bits(got["gap_min"])[0, 0] == bits(d) and bits(got["pen_depth"])[0, 0] == (bits(depth) if n else 0)


# ------------------------------------------------------------------------------------------------------ GPU: end to end
def _mano_pkl(tmp_path):
    path = str(tmp_path / "MANO_RIGHT.pkl")
    if not os.path.exists(path):
        with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
    return path


def _run_main(dataset, out_dir, extra, mano):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


PLAIN_KEYS = {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact"}


def _cloud_files(tmp_path):
    from test_grasp_wrench import e2e_clouds
    files = []
    for i, c in enumerate(e2e_clouds()):                                 # three clouds where the synthetic weights put the hands, one far away
        files.append(str(tmp_path / f"cloud{i}.npy"))
        np.save(files[-1], c)
    return files


@pytest.mark.gpu
def test_entry_point_writes_the_self_collision_fields(tmp_path):
    """One small run with synthetic weights on the real hand topology: the files do not depend on --rows_per_call, the fields are
    those of contact.grasp_self on the written parameters posed again, and guarded candidates come after the others."""
    mano = _mano_pkl(tmp_path)
    M, k = 8, 4
    files = _cloud_files(tmp_path)
    n_obj = len(files)
    base = ["--objects"] + files + ["--num_grasp", str(k), "--candidates", str(M)]
    flags = base + ["--self_collision", "1", "--max_self_verts", "0"]
    names0, bytes0 = _run_main("obman", str(tmp_path / "s16384"), flags + ["--rows_per_call", "16384"], mano)
    names1, bytes1 = _run_main("obman", str(tmp_path / "s8"), flags + ["--rows_per_call", "8"], mano)
    assert names1 == names0 and bytes1 == bytes0 and len(names0) == n_obj, "--rows_per_call 8: the files differ"
    pooled_text = open(str(tmp_path / "s16384" / "self_collision.json"), "rb").read()
    assert open(str(tmp_path / "s8" / "self_collision.json"), "rb").read() == pooled_text
    layer = dmano.load(model_path=mano, model_type="mano", use_pca=True, num_pca_comps=45, flat_hand_mean=True).to(DEV)
    faces = np.asarray(layer.faces)
    topo = contact.HandTopology(faces, 778, DEV)
    table = contact.SelfTable(contact.HandParts.from_json(), faces, device=DEV)
    counts, pairs = [], []
    for data in bytes0:
        assert b"Infinity" not in data and b"NaN" not in data
        j = json.loads(data)
        assert set(j) == PLAIN_KEYS | set(FIELDS) and list(j)[-5:] == list(FIELDS) and all(len(j[f]) == k for f in FIELDS)
        params = torch.tensor(np.asarray(j["recon_params"], np.float32).reshape(k, 61), device=DEV)
        posed = layer(betas=params[:, :10], global_orient=params[:, 10:13], hand_pose=params[:, 13:58], transl=params[:, 58:61])
        want = contact.self_stats(contact.grasp_self(topo, table, posed.vertices))
        assert {f: j[f] for f in FIELDS} == json.loads(json.dumps(want)), "the fields are not those of the hands written"
        # kept order: within the hands that touch the object, those within the guard come first
        touching = [c for c, n in zip(j["self_penetrating"], j["n_contact"]) if n >= 1]
        assert touching == sorted(touching, key=lambda c: c > 0), (j["self_penetrating"], j["n_contact"])
        counts += j["self_penetrating"]
        pairs += [tuple(ab) for g in j["self_pairs"] for ab in g]
    pooled = json.loads(pooled_text)
    assert pooled["grasps"] == n_obj * k and pooled["parts"] == table.parts.names and pooled["seam_vertices"] == 210
    assert (pooled["reach"], pooled["margin"], pooled["seam"], pooled["palm"]) == (0.01, 0.001, 2, 1)
    assert pooled["share_penetrating"] == sum(1 for c in counts if c > 0) / len(counts)
    assert abs(pooled["mean_penetrating"] - sum(counts) / len(counts)) < 1e-12
    assert pooled["pair_histogram"] == [[pairs.count((a, b)) for b in range(6)] for a in range(6)]
    print("self_penetrating of the kept grasps", counts, "pairs", sorted(set(pairs)))
    # the order of ALL candidates, from the tensors: maximum(class of the scores, class of the guard), then the key.  Once with the
    # run's settings, and once with no seam and no margin -- settings under which the calibration finds a dozen false alarms on any
    # hand -- and the guard at the median count of the candidates, so that it does move candidates
    net_args = generate.parse_args("obman", flags + ["--checkpoint", "/nonexistent", "--mano_model", mano])
    net = generate.load_model(net_args, torch.device(DEV))
    objs = [generate.object_tensor(np.load(f).astype(np.float64)) for f in files]
    idx = list(range(n_obj))
    free = generate.generate_for_objects(net, objs, k, False, 3, idx, candidates=M)
    loose = dict(self_seam=0, self_margin=0.0)
    seen = generate.generate_for_objects(net, objs, k, False, 3, idx, candidates=M, self_collision=True, **loose)
    totals = np.concatenate([g["self_scores"]["pen_count"].sum(dim=1).cpu().numpy() for g in seen[:3]])
    K = int(np.median(totals))
    print("self counts of all candidates without a seam and a margin", totals.tolist(), "guard at", K)
    assert totals.min() <= K < totals.max(), "the candidates do not straddle the guard"
    moved = False
    for settings, limit in ((dict(), 0), (loose, K)):
        guarded = generate.generate_for_objects(net, objs, k, False, 3, idx, candidates=M, self_collision=True, max_self_verts=limit, **settings)
        for i, (g, f, u) in enumerate(zip(guarded, free, seen)):
            assert tuple(g["self_scores"]) == OUTPUTS and "self_scores" not in f and set(g["scores"]) == set(f["scores"])
            full = {name: t.cpu().numpy() for name, t in g["self_scores"].items()}
            cls, key = contact.select_keys({name: t.cpu() for name, t in g["scores"].items()}, "penetration", 1)
            guard = np.asarray(ref.self_class(full["pen_count"], full["status"], limit), np.int32)
            c = g["candidate"].cpu().numpy()
            assert np.array_equal(c, score_ref.segment_topk(np.maximum(cls.numpy(), guard), key.numpy(), 1, M, k)[0]), f"object {i}: order"
            assert all(torch.equal(g["self"][name].cpu(), g["self_scores"][name].cpu()[c]) for name in OUTPUTS)
            assert g["json"]["self_penetrating"] == [int(full["pen_count"][r].sum()) for r in c]
            if settings:
                assert all(torch.equal(g["self_scores"][name], u["self_scores"][name]) for name in OUTPUTS)   # the guard changes no figure
                moved |= c.tolist() != f["candidate"].tolist()
            else:
                assert json.dumps(g["json"]).encode() == bytes0[i]
            print(f"guard {limit} object {i}: kept {c.tolist()} (without the guard {f['candidate'].tolist()}) self counts "
                  f"{full['pen_count'].sum(axis=1).tolist()} cls {cls.tolist()} guard {guard.tolist()}")
    assert moved, "the guard is not exercised"


@pytest.mark.gpu
def test_entry_point_without_the_flags_writes_the_parents_bytes(tmp_path):
    """``--self_collision 0`` (and values for the dependent flags) against a run that omits them all: the code path of the parent
    commit, the same bytes, and no self_collision.json; --self_collision 1 alone adds the five fields to the same grasps."""
    mano = _mano_pkl(tmp_path)
    base = ["--num_objects", "2", "--points", "256", "--num_grasp", "4", "--candidates", "8"]
    names0, plain = _run_main("obman", str(tmp_path / "plain"), base, mano)
    names, off = _run_main("obman", str(tmp_path / "off"), base + ["--self_collision", "0", "--self_reach", "0.02", "--self_margin", "0",
                                                                   "--self_seam", "1", "--self_palm", "0"], mano)
    assert names == names0 and off == plain and not os.path.exists(str(tmp_path / "off" / "self_collision.json"))
    assert all(set(json.loads(d)) == PLAIN_KEYS for d in plain)
    _, figures = _run_main("obman", str(tmp_path / "on"), base + ["--self_collision", "1"], mano)
    for a, b in zip(plain, figures):
        ja, jb = json.loads(a), json.loads(b)
        assert {f: jb[f] for f in ja} == ja and list(jb)[len(ja):] == list(FIELDS)
    assert os.path.exists(str(tmp_path / "on" / "self_collision.json"))


@pytest.mark.gpu
def test_self_collision_rides_with_every_other_option(tmp_path):
    """Without candidates the six tensors ride at the tail of each of _generate_call's three host copies, with candidates inside
    _select_call's one: beside every option that adds pieces of its own the other fields stay what they were, and the self_* fields
    are those of the vertices returned (after the push-out where there is one)."""
    mano = _mano_pkl(tmp_path)
    net = generate.load_model(generate.parse_args("obman", ["--checkpoint", "/nonexistent", "--mano_model", mano]), torch.device(DEV))
    objs = [generate.object_tensor(np.load(f).astype(np.float64)) for f in _cloud_files(tmp_path)[:3]]
    idx = [0, 1, 2]
    faces = np.asarray(net.rh_mano.faces)
    topo = contact.HandTopology(faces, 778, DEV)
    table = contact.SelfTable(contact.HandParts.from_json(), faces, seam=0, device=DEV)      # no seam, no margin: counts that differ
    loose = dict(self_collision=True, self_seam=0, self_margin=0.0)
    combos = [dict(), dict(refine_steps=2), dict(refine_steps=2, refine_spin=1.0, refine_curl=0.5), dict(parts=True), dict(volume=True),
              dict(parts=True, volume=True, refine_steps=2), dict(stability=True, diversity=2, log_prob=True),
              dict(candidates=8, parts=True, volume=True, diversity=2, refine_steps=2), dict(candidates=8, diverse_pool=6, stability=True)]
    counts = set()
    for combo in combos:
        for rows_per_call in (16384, 4):
            plain = generate.generate_for_objects(net, objs, 4, False, 3, idx, rows_per_call=rows_per_call, **combo)
            both_ = generate.generate_for_objects(net, objs, 4, False, 3, idx, rows_per_call=rows_per_call, **combo, **loose)
            for g, p in zip(both_, plain):
                j, q = g["json"], p["json"]
                assert {f: j[f] for f in q} == q and list(j)[len(q):] == list(FIELDS), combo
                assert torch.equal(g["params"], p["params"]) and torch.equal(g["vertices"], p["vertices"])
                out = contact.grasp_self(topo, table, g["vertices"], margin=0.0)
                assert all(torch.equal(g["self"][name], out[name]) for name in OUTPUTS), combo
                assert {f: j[f] for f in FIELDS} == json.loads(json.dumps(contact.self_stats(out))), combo
                assert ("self_scores" in g) == ("candidates" in combo)
                counts |= set(j["self_penetrating"])
    assert len(counts) >= 3, counts
