"""Diverse best-of-M: the farthest-point selection inside a quality pool (dvq_segment_diverse), its host API and the
``diverse_pool`` mode of generate_for_objects / the entry points.  The reference is tests/diverse_select_ref.py (numpy float32, one
rounding per operation); GPU results are compared with it on bits: sel and rank exactly, gap as uint32."""
import functools
import json
import lzma
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, diversity, generate, ops, synth

import diverse_select_ref as dref
import grasp_score_ref as sref

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
DATASETS = ["obman", "ho3d", "grab", "FHAB"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", DATASETS)
def test_parser_has_the_diverse_flags(dataset):
    a = generate.build_parser(dataset).parse_args([])
    assert (a.diverse_pool, a.diverse_space) == (0, "params")
    a = generate.parse_args(dataset, [])
    assert (a.diverse_pool, a.diverse_space) == (0, "params")
    a = generate.parse_args(dataset, ["--candidates", "400", "--num_grasp", "100", "--diverse_pool", "200", "--diverse_space", "verts"])
    assert (a.candidates, a.num_grasp, a.diverse_pool, a.diverse_space) == (400, 100, 200, "verts")
    for P in (100, 400):                                                # both ends of the range are allowed
        assert generate.parse_args(dataset, ["--candidates", "400", "--num_grasp", "100", "--diverse_pool", str(P)]).diverse_pool == P
    with pytest.raises(SystemExit):
        generate.build_parser(dataset).parse_args(["--diverse_space", "joints"])


@pytest.mark.parametrize("dataset", DATASETS)
def test_parser_refuses_a_pool_without_candidates_or_out_of_range(dataset):
    with pytest.raises(SystemExit):                                     # the flag needs --candidates
        generate.parse_args(dataset, ["--num_grasp", "1", "--diverse_pool", "4"])
    for P in ("99", "401", "-1"):                                       # num_grasp <= diverse_pool <= candidates
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, ["--candidates", "400", "--num_grasp", "100", "--diverse_pool", P])


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_segment_diverse" in _lib.SIGNATURES and len(_lib.SIGNATURES["dvq_segment_diverse"][1]) == 13
    assert "int dvq_segment_diverse(" in header and hasattr(lib, "dvq_segment_diverse")
    added = re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert all(n in added for n in ("dvq_pixelcnn_sample_ctl", "dvq_grasp_scores", "dvq_segment_topk", "dvq_segment_diverse"))
    assert lib.dvq_abi_version() == 10
    assert ops.SEGMENT_DIVERSE_MAX_D == 4096


def test_ops_refuse_bad_arguments_before_any_device_use():
    feat, pool = torch.zeros(6, 5), torch.tensor([[0, 1], [2, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.segment_diverse(feat, pool, 2, 3, 2)                                        # well-formed, but not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.segment_diverse(torch.zeros(6, 8)[:, 1:6], pool, 2, 3, 1)                   # a column slice is well-formed too
    wide = torch.zeros(6, 10)
    for args in ((feat.double(), pool, 2, 3, 2), (feat, pool.int(), 2, 3, 2), (feat, pool.float(), 2, 3, 2),
                 (wide[:, ::2], pool, 2, 3, 2),                                          # stride(1) != 1
                 (torch.zeros(1, 5).expand(6, 5), pool, 2, 3, 2),                        # ld = 0 < D
                 (torch.zeros(30).as_strided((6, 5), (4, 1)), pool, 2, 3, 2),            # ld = 4 < D: rows overlap
                 (feat, torch.zeros(2, 4, dtype=torch.int64), 2, 3, 2),                  # P > M
                 (feat, pool, 2, 3, 3),                                                  # keep > P
                 (feat, pool, 2, 3, 0),                                                  # keep = 0
                 (torch.zeros(4097, 2), torch.zeros(1, 2, dtype=torch.int64), 1, 4097, 1),   # M = 4097
                 (torch.zeros(3, 4097), torch.zeros(1, 2, dtype=torch.int64), 1, 3, 1),      # D = 4097
                 (torch.zeros(3, 0), torch.zeros(1, 2, dtype=torch.int64), 1, 3, 1),         # D = 0
                 (feat, pool.reshape(-1), 2, 3, 2), (feat, pool[:1], 2, 3, 2), (feat, pool.t(), 2, 3, 2),   # pool shape / layout
                 (feat[:5], pool, 2, 3, 2), (feat.reshape(-1), pool, 2, 3, 2),           # feat is not [O*M, D]
                 (feat, pool, -1, 3, 2), (feat, pool, 2, 3, 2, torch.zeros(1)),          # O < 0; an err flag of the wrong type
                 (None, pool, 2, 3, 2)):
        with pytest.raises(RuntimeError) as e:
            ops.segment_diverse(*args)
        assert "no CPU fallback" not in str(e.value), f"{args[2:]}: refused only for the device, not for the argument"


def test_the_lds_threshold_follows_the_documented_arithmetic():
    assert ops.SEGMENT_DIVERSE_LDS_FLOATS * 4 == 160 * 1024
    assert ops.segment_diverse_lds_resident(400, 61)                    # ho3d's defaults in parameter space
    assert not ops.segment_diverse_lds_resident(400, 2334) and not ops.segment_diverse_lds_resident(40, 2334)    # vertex space
    assert ops.segment_diverse_lds_resident(4096, 5) and ops.segment_diverse_lds_resident(1, 4096)
    P = lds_threshold_pool(61)
    assert 32 + (P + 3) // 4 * 4 + P * 61 <= ops.SEGMENT_DIVERSE_LDS_FLOATS < 32 + (P + 4) // 4 * 4 + (P + 1) * 61


def test_generate_for_objects_refuses_a_bad_pool_before_any_work():
    objs = [torch.zeros(4, 8)]
    for kw in (dict(diverse_pool=6), dict(candidates=8, diverse_pool=4), dict(candidates=8, diverse_pool=9),
               dict(candidates=8, diverse_pool=-1), dict(candidates=8, diverse_pool=6, diverse_space="joints")):
        with pytest.raises(RuntimeError, match="diverse_"):
            generate.generate_for_objects(None, objs, 5, True, 0, [0], **kw)             # no net: nothing may touch it


def test_coverage_is_the_nearest_neighbour_distance():
    x = np.asarray([[0.0, 0.0], [3.0, 4.0], [3.0, 5.0], [-6.0, 8.0]])
    lo, mean = diversity.coverage(x)
    assert lo == 1.0 and mean == pytest.approx((5.0 + 1.0 + 1.0 + 90.0 ** 0.5) / 4)
    assert diversity.coverage(np.concatenate([x, x[:1]]))[0] == 0.0      # a duplicate
    assert all(np.isnan(v) for v in diversity.coverage(x[:1]))
    assert diversity.coverage([[[1.0, 2.0]], [[1.0, 4.0]]]) == (2.0, 2.0)               # recon_params' [[61 floats]] nesting


# ------------------------------------------------------------------------------------------------------ the cases
def lds_threshold_pool(D):
    """The largest pool whose rows of D features the kernel keeps in LDS, from the constant ops exposes."""
    P = 1
    while ops.segment_diverse_lds_resident(P + 1, D):
        P += 1
    return P


@functools.lru_cache(maxsize=None)
def diverse_case(O, M, P, keep, D):
    """(feat [O*M,D], pool [O,P], specials): Gaussian rows; the pool is a prefix of a random permutation, so position != candidate.
    With P >= 6, per object: the row at pool position dup[0] is an exact copy of the one at dup[1], one pooled row has a NaN and one
    an Inf (positions > 0: pick 0 stays a valid row).  specials[o] = (dup pair, sorted invalid positions)."""
    rng = np.random.default_rng([O, M, P, keep, D])
    feat = rng.standard_normal((O * M, D)).astype(np.float32)
    pool = np.stack([rng.permutation(M)[:P] for _ in range(O)]).astype(np.int64)
    specials = []
    for o in range(O):
        if P < 6:
            specials.append(None)
            continue
        a, b, n, f = (int(x) for x in 1 + rng.permutation(P - 1)[:4])
        rows = o * M + pool[o]
        feat[rows[a]] = feat[rows[b]]
        feat[rows[n], int(rng.integers(D))] = np.nan
        feat[rows[f], int(rng.integers(D))] = np.inf if o % 2 == 0 else -np.inf
        specials.append(((a, b), sorted((n, f))))
    feat.setflags(write=False), pool.setflags(write=False)
    return feat, pool, tuple(specials)


@functools.lru_cache(maxsize=None)
def reference(O, M, P, keep, D):
    feat, pool, _ = diverse_case(O, M, P, keep, D)
    out = dref.segment_diverse(feat, pool, O, M, keep)
    for a in out:
        a.setflags(write=False)
    return out


def assert_the_reference_places_the_specials(O, M, P, D):
    """The whole pool in farthest-point order (keep = P): a permutation, non-increasing gaps, the duplicate after every distinct row,
    the two rows that are not finite last in pool order; min(gap) is the smallest pairwise distance of the valid rows."""
    feat, pool, specials = diverse_case(O, M, P, P, D)
    sel, rank, gap = reference(O, M, P, P, D)
    for o in range(O):
        (a, b), invalid = specials[o]
        rows = feat[o * M + pool[o]]
        assert np.array_equal(rows[a], rows[b]) and np.isnan(rows).any() and np.isinf(rows).any()
        assert (~np.isfinite(rows).all(axis=1)).sum() == 2
        assert sorted(rank[o].tolist()) == list(range(P)) and np.array_equal(sel[o], pool[o][rank[o]])
        assert rank[o, 0] == 0 and gap[o, 0] == -1.0
        assert rank[o, -2:].tolist() == invalid and (gap[o, -2:] == -1.0).all()
        assert bits(gap[o, -3]) == 0 and rank[o, -3] in (a, b) and ({a, b} - {int(rank[o, -3])}) <= set(rank[o, :-3].tolist())
        body = gap[o, 1:-2]
        assert (body[:-1] > 0).all() and (np.diff(body) <= 0).all()
        valid = rows[rank[o, :-2]]
        pair = np.stack([dref.dist2(valid, v) for v in valid])
        assert np.array_equal(bits(pair), bits(pair.T)), "d(a, b) != d(b, a)"
        pair[np.diag_indices(len(valid))] = np.inf
        assert bits(pair.min()) == bits(body.min()) == 0
        keep_valid = P - 3                                              # without the duplicate: the minimum is a real distance
        sub = pair[:keep_valid, :keep_valid]
        assert bits(sub.min()) == bits(gap[o, 1:keep_valid].min()) and sub.min() > 0


# ------------------------------------------------------------------------------------------------------ CPU: the reference itself
@pytest.mark.parametrize("P,D,keep", [(520, 61, 33), (4096, 5, 7), (40, 2334, 40), (70, 64, 70)])
def test_reference_properties(P, D, keep):
    O, M = 1, P + 3
    feat, pool, specials = diverse_case(O, M, P, keep, D)
    sel, rank, gap = reference(O, M, P, keep, D)
    assert len(set(sel[0].tolist())) == keep and np.array_equal(sel[0], pool[0][rank[0]])
    assert rank[0, 0] == 0 and gap[0, 0] == -1.0
    rows = feat[pool[0]]
    finite = np.isfinite(rows[rank[0]]).all(axis=1)
    body = gap[0, 1:][finite[1:]]
    assert (np.diff(body) <= 0).all(), "gap[1:] must be non-increasing over the valid picks"
    kept = rows[rank[0]][finite]
    pair = np.stack([dref.dist2(kept, v) for v in kept])
    assert np.array_equal(bits(pair), bits(pair.T)), "d(a, b) != d(b, a)"
    pair[np.diag_indices(len(kept))] = np.inf
    assert bits(pair.min()) == bits(body.min()), "min(gap[1:]) is the kept set's smallest pairwise distance"
    if keep < P:                                                        # greedy selection is incremental: a prefix of a longer run
        longer = dref.segment_diverse(feat, pool, O, M, min(P, keep + 5))
        assert np.array_equal(longer[0][:, :keep], sel) and np.array_equal(longer[1][:, :keep], rank)
        assert np.array_equal(bits(longer[2][:, :keep]), bits(gap))
    if P <= 520:
        assert_the_reference_places_the_specials(O, M, P, D)


def test_reference_with_an_invalid_first_row_and_tiny_pools():
    x = np.asarray([[np.nan, 0.0], [1.0, 1.0], [2.0, 2.0], [np.inf, 0.0]], np.float32)
    sel, rank, gap = dref.segment_diverse(x, np.asarray([[0, 1, 2, 3]]), 1, 4, 4)
    assert rank.tolist() == [[0, 1, 2, 3]] and (gap == -1.0).all()      # every distance to pick 0 is NaN: rank order, no distances
    x = np.asarray([[0.0], [3.0], [1.0], [3.0]], np.float32)
    sel, rank, gap = dref.segment_diverse(x, np.asarray([[2, 0, 3, 1]]), 1, 4, 4)       # rows 1, 0, 3, 3 in pool order
    assert rank.tolist() == [[0, 2, 1, 3]] and sel.tolist() == [[2, 3, 0, 1]] and gap.tolist() == [[-1.0, 4.0, 1.0, 0.0]]
    assert dref.segment_diverse(x, np.asarray([[3]]), 1, 4, 1)[0].tolist() == [[3]]


# ------------------------------------------------------------------------------------------------------ GPU: the kernel
def run(feat, pool, O, M, keep, **kw):
    sel, rank, gap = ops.segment_diverse(feat if torch.is_tensor(feat) else gpu(feat), gpu(pool), O, M, keep, **kw)
    assert sel.dtype == torch.int64 and rank.dtype == torch.int32 and gap.dtype == torch.float32
    assert tuple(sel.shape) == tuple(rank.shape) == tuple(gap.shape) == (O, keep)
    return sel.cpu().numpy(), rank.cpu().numpy(), gap.cpu().numpy()


def assert_equal_bits(got, want, what=""):
    for name, g, w in zip(("sel", "rank", "gap"), got, want):
        print(what, name, "got", g.reshape(-1)[:12], "reference", w.reshape(-1)[:12])
        if name == "gap":
            g, w = bits(g), bits(w)
        assert np.array_equal(g, w), f"{what}: {name} differs from the reference in {int((g != w).sum())} places"


def kernel_cases():
    P = lds_threshold_pool(61)
    return [(3, 1, 1, 1, 1), (2, 70, 70, 70, 64), (3, 600, 520, 33, 61), (1, 4096, 4096, 7, 5), (2, 300, 40, 40, 2334),
            (1, P + 40, P, 9, 61), (1, P + 40, P + 1, 9, 61)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(7))
def test_segment_diverse_equals_the_reference_bit_for_bit(case):
    O, M, P, keep, D = kernel_cases()[case]
    if case == 5:                                                       # on either side of the LDS threshold
        assert ops.segment_diverse_lds_resident(P, D) and not ops.segment_diverse_lds_resident(P + 1, D)
    if case == 6:
        assert ops.segment_diverse_lds_resident(P - 1, D) and not ops.segment_diverse_lds_resident(P, D)
    assert ops.segment_diverse_lds_resident(P, D) == (case not in (4, 6))
    feat, pool, specials = diverse_case(O, M, P, keep, D)
    assert any((pool[o] != np.arange(P)).any() for o in range(O)) or P == 1
    got = run(feat, pool, O, M, keep)
    assert_equal_bits(got, reference(O, M, P, keep, D), str((O, M, P, keep, D)))
    if P >= 6:
        for o in range(O):                                              # the data really holds what the case promises
            rows = feat[o * M + pool[o]]
            (a, b), invalid = specials[o]
            assert np.array_equal(rows[a], rows[b]) and np.isnan(rows[invalid]).any() and np.isinf(rows[invalid]).any()
        if keep == P:
            assert_the_reference_places_the_specials(O, M, P, D)
        elif P <= 520:                                                  # the same shape with the whole pool kept, device and reference
            whole = diverse_case(O, M, P, P, D)
            assert_equal_bits(run(whole[0], whole[1], O, M, P), reference(O, M, P, P, D), "keep = P")
            assert_the_reference_places_the_specials(O, M, P, D)


@pytest.mark.gpu
def test_segment_diverse_on_rows_at_the_edges_of_the_definition():
    """Four objects in one call: the best-ranked row itself not finite (every distance to pick 0 is NaN: rank order, no gaps);
    squared differences that overflow to +inf; every row the same (all gaps +0.0, rank order); ten copies of one row among the others."""
    O, M, D = 4, 40, 7
    rng = np.random.default_rng(11)
    feat = rng.standard_normal((O * M, D)).astype(np.float32)
    feat[0, 3] = np.nan
    feat[M + 5], feat[M + 6], feat[M + 7, 2] = 3e38, -3e38, -np.inf
    feat[2 * M:3 * M] = feat[2 * M]
    feat[3 * M + 10:3 * M + 20] = feat[3 * M + 4]
    pool = np.tile(np.arange(M), (O, 1))
    pool[1] = pool[1, ::-1]
    want = dref.segment_diverse(feat, pool, O, M, M)
    assert want[1][0].tolist() == list(range(M)) and (want[2][0] == -1.0).all()
    assert np.isinf(want[2][1]).sum() >= 2 and want[1][1, -1] == M - 1 - 7
    assert want[1][2].tolist() == list(range(M)) and (bits(want[2][2, 1:]) == 0).all()
    assert (bits(want[2][3, -10:]) == 0).all() and (want[2][3, 1:-10] > 0).all()             # eleven equal rows: one picked as new
    assert_equal_bits(run(feat, pool, O, M, M), want, "edge rows")
    assert_equal_bits(run(feat, pool, O, M, 1), [w[:, :1] for w in want], "keep = 1")


@pytest.mark.gpu
def test_segment_diverse_reads_strided_features_in_place():
    O, M, P, keep = 2, 30, 24, 9
    rng = np.random.default_rng(5)
    pool = np.stack([rng.permutation(M)[:P] for _ in range(O)])
    wide = gpu(rng.standard_normal((O * M, 80)).astype(np.float32))
    view = wide[:, 7:68]                                                # [O*M,61] of a wider tensor: ld = 80, an unaligned base
    assert view.stride() == (80, 1) and not view.is_contiguous()
    got = run(view, pool, O, M, keep)
    assert_equal_bits(got, run(view.contiguous(), pool, O, M, keep), "slice against its copy")
    assert_equal_bits(got, dref.segment_diverse(view.cpu().numpy(), pool, O, M, keep), "slice")
    verts = gpu(rng.standard_normal((O * M, 778, 3)).astype(np.float32))
    flat = verts.view(O * M, 2334)                                      # rows 8-byte aligned only
    want = dref.segment_diverse(flat.cpu().numpy(), pool, O, M, keep)
    assert_equal_bits(run(flat, pool, O, M, keep), want, "vertices viewed as [B,2334]")
    padded = torch.zeros(O * M, 2340, device=DEV)                       # the same rows at the three alignments the loads choose by
    for lo in (0, 1, 2):                                                # 16-byte rows, 4-byte rows, 8-byte rows
        padded[:, lo:lo + 2334] = flat
        assert_equal_bits(run(padded[:, lo:lo + 2334], pool, O, M, keep), want, f"ld = 2340, column offset {lo}")


@pytest.mark.gpu
def test_segment_diverse_of_an_object_does_not_depend_on_the_batch():
    for O, M, P, keep, D in ((3, 600, 520, 33, 61), (2, 300, 40, 40, 2334)):
        feat, pool, _ = diverse_case(O, M, P, keep, D)
        got = run(feat, pool, O, M, keep)
        for o in range(O):
            one = run(feat[o * M:(o + 1) * M], pool[o:o + 1], 1, M, keep)
            assert_equal_bits(one, [g[o:o + 1] for g in got], f"object {o} alone")
    O, M, P, keep, D = 700, 8, 8, 4, 61                                 # more workgroups than compute units
    feat, pool, _ = diverse_case(O, M, P, keep, D)
    got = run(feat, pool, O, M, keep)
    assert_equal_bits(got, reference(O, M, P, keep, D), "700 objects")
    f, p, err = gpu(feat), gpu(pool), ops.new_err_flag(torch.device(DEV))
    alone = [ops.segment_diverse(f[o * M:(o + 1) * M], p[o:o + 1], 1, M, keep, err=err) for o in range(O)]
    assert int(err.item()) == 0
    assert_equal_bits([torch.cat([a[k] for a in alone]).cpu().numpy() for k in range(3)], got, "700 objects alone")
    empty = ops.segment_diverse(f[:0], p[:0], 0, M, keep)
    assert all(tuple(e.shape) == (0, keep) for e in empty)


@pytest.mark.gpu
def test_segment_diverse_flags_a_pool_entry_out_of_range():
    O, M, P, keep, D = 3, 600, 520, 33, 61
    feat, pool, _ = diverse_case(O, M, P, keep, D)
    for value in (M, -1, 1 << 40):
        bad = pool.copy()
        bad[1, 300] = value
        with pytest.raises(RuntimeError, match="out of bounds"):
            ops.segment_diverse(gpu(feat), gpu(bad), O, M, keep)
        err = ops.new_err_flag(torch.device(DEV))
        sel, rank, gap = run(feat, bad, O, M, keep, err=err)            # the caller's flag: set, object 1 is -1, the others are right
        assert int(err.item()) == 1
        assert (sel[1] == -1).all() and (rank[1] == -1).all() and (gap[1] == -1.0).all()
        want = reference(O, M, P, keep, D)
        assert_equal_bits([g[[0, 2]] for g in (sel, rank, gap)], [w[[0, 2]] for w in want], "the other objects")
    err = ops.new_err_flag(torch.device(DEV))                           # the streaming path checks before it reads too
    assert not ops.segment_diverse_lds_resident(10, 4096)
    sel, _, _ = run(np.zeros((12, 4096), np.float32), np.asarray([[0, 1, 2, 3, 4, 5, 6, 7, 8, 12]]), 1, 12, 2, err=err)
    assert int(err.item()) == 1 and (sel == -1).all()
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL, nothing launched
    f, p, e = gpu(feat), gpu(pool), ops.new_err_flag(torch.device(DEV))
    out = torch.zeros(O * P, dtype=torch.int64, device=DEV)
    call = lambda ld, D, O, M, P, keep: lib.dvq_segment_diverse(f.data_ptr(), ld, D, p.data_ptr(), O, M, P, keep, out.data_ptr(),
                                                                out.data_ptr(), out.data_ptr(), e.data_ptr(), None)
    for args in ((61, 61, 3, 600, 520, 0), (61, 61, 3, 600, 520, 521), (61, 61, 3, 500, 520, 33), (61, 61, 1, 4097, 520, 33),
                 (61, 0, 3, 600, 520, 33), (4097, 4097, 1, 8, 4, 2), (60, 61, 3, 600, 520, 33), (61, 61, -1, 600, 520, 33)):
        assert call(*args) == 1, args
    assert lib.dvq_segment_diverse(None, 61, 61, p.data_ptr(), 3, 600, 520, 33, out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                   e.data_ptr(), None) == 1
    assert call(61, 61, 0, 600, 520, 33) == 0 and int(e.item()) == 0     # O = 0: a no-op


# ------------------------------------------------------------------------------------------------------ GPU: end to end
def mano_pkl(tmp_path):
    """tests/golden/g9_mano_right.pkl.xz unpacked: the path of a MANO_RIGHT.pkl (real topology: 778 vertices, 1538 faces)."""
    path = str(tmp_path / "MANO_RIGHT.pkl")
    if not os.path.exists(path):
        with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
    return path


def _gennet(tmp_path):
    """The synthetic net and the real MANO model of tests/test_grasp_select.py (the scores need the faces)."""
    from conftest import GOLDEN, gen_state_dict
    from dvqvae_amd import mano as dmano
    from dvqvae_amd.network.gen_net import GenNet
    net = GenNet()
    net.load_state_dict(gen_state_dict(net.state_dict(), np.load(os.path.join(GOLDEN, "g7_gen.npz"))), strict=True)
    net.eval().to(DEV)
    net.set_rh_mano(dmano.load(model_path=mano_pkl(tmp_path), model_type="mano", use_pca=True, num_pca_comps=45,
                               flat_hand_mean=True).to(DEV))
    return net


E2E_SEED, E2E_M, E2E_P, E2E_K = 9, 24, 12, 5
E2E_INDICES = [5, 2, 11, 7]


def e2e_objects(at_the_hand=False):
    """The four clouds of tests/test_grasp_select.py: two point counts; ``at_the_hand``: around the place the synthetic weights put
    every hand, for calls without rotation, so that the candidates' penetration keys differ."""
    if not at_the_hand:
        return [synth.synthetic_clouds(1, n, seed=60 + i)[0] for i, n in enumerate((700, 300, 700, 300))]
    centre = np.asarray([-0.08, -0.09, 0.13])
    return [generate.object_tensor(synth.synthetic_uniform((n, 3), 70 + i, "select/e2e", -0.1, 0.1).numpy().astype(np.float64) + centre)
            for i, n in enumerate((700, 300, 700, 300))]


def same_result(a, b):
    if set(a) != set(b) or json.dumps(a["json"]) != json.dumps(b["json"]):
        return False
    for k in a:
        if torch.is_tensor(a[k]) and not torch.equal(a[k], b[k]):
            return False
        if isinstance(a[k], dict) and k != "json" and not all(torch.equal(a[k][n], b[k][n]) for n in a[k]):
            return False
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("select_by,rotate,space", [("penetration", False, "params"), ("log_prob", True, "params"),
                                                    ("penetration", False, "verts")])
def test_diverse_pool_keeps_a_farthest_point_subset_of_the_best(select_by, rotate, space, tmp_path):
    net = _gennet(tmp_path)
    objs, M, P, k = e2e_objects(at_the_hand=not rotate), E2E_M, E2E_P, E2E_K
    with_lp = select_by == "log_prob"
    plain = generate.generate_for_objects(net, objs, M, rotate, E2E_SEED, E2E_INDICES, log_prob=with_lp)  # every candidate, unselected
    best = generate.generate_for_objects(net, objs, k, rotate, E2E_SEED, E2E_INDICES, candidates=M, select_by=select_by)
    zero = generate.generate_for_objects(net, objs, k, rotate, E2E_SEED, E2E_INDICES, candidates=M, select_by=select_by,
                                         diverse_pool=0, diverse_space="verts")
    assert all(same_result(z, b) and "rank" not in z and "novelty" not in z and "rank" not in z["json"] for z, b in zip(zero, best))
    first, differs = None, False
    for rows_per_call in (16384, M, 1):
        got = generate.generate_for_objects(net, objs, k, rotate, E2E_SEED, E2E_INDICES, rows_per_call=rows_per_call, candidates=M,
                                            select_by=select_by, diverse_pool=P, diverse_space=space)
        assert len(got) == len(objs)
        for i, (g, p, b) in enumerate(zip(got, plain, best)):
            cand, rank, nov = g["candidate"], g["rank"], g["novelty"]
            assert cand.dtype == torch.int64 and rank.dtype == torch.int32 and nov.dtype == torch.float32
            assert tuple(cand.shape) == tuple(rank.shape) == tuple(nov.shape) == (k,)
            c = cand.cpu().numpy()
            assert torch.equal(g["params"], p["params"][cand]), f"object {i}: kept parameters are not rows of the plain run"
            assert torch.equal(g["vertices"], p["vertices"][cand]), f"object {i}: kept vertices"
            scores = {name: t.cpu() for name, t in g["scores"].items()}
            assert all(torch.equal(g["scores"][n], b["scores"][n]) for n in b["scores"])
            cls, key = contact.select_keys(scores, select_by, 1, log_prob=scores.get("log_prob"))
            top = sref.segment_topk(cls.numpy(), key.numpy(), 1, M, P)
            assert np.array_equal(top[0, :k], b["candidate"].cpu().numpy())            # the ranking best-of-M keeps the head of
            assert set(c.tolist()) <= set(top[0].tolist()) and len(set(c.tolist())) == k
            assert int(rank[0]) == 0 and c[0] == top[0, 0], f"object {i}: pick 0 is not the best candidate"
            feat = (p["params"] if space == "params" else p["vertices"].reshape(M, -1)).cpu().numpy()
            want = dref.segment_diverse(feat, top, 1, M, k)
            assert_equal_bits((c[None], rank.cpu().numpy()[None], nov.cpu().numpy()[None]), want, f"object {i}")
            assert np.array_equal(top[0][rank.cpu().numpy()], c)
            j = g["json"]
            assert j["candidate"] == c.tolist() and j["rank"] == rank.tolist() and j["novelty"] == nov.cpu().numpy().tolist()
            assert list(j)[-2:] == ["rank", "novelty"] and list(j)[:len(b["json"])] == list(b["json"])
            assert all(isinstance(x, int) for x in j["rank"]) and all(isinstance(x, float) for x in j["novelty"])
            assert j["recon_params"] == [p["json"]["recon_params"][x] for x in c]
            assert j["R_list"] == [p["json"]["R_list"][x] for x in c] and j["r_list"] == [p["json"]["r_list"][x] for x in c]
            for name in ("penetration", "n_interior", "n_contact"):
                assert j[name] == scores[name].numpy()[c].tolist(), name
            if with_lp:
                assert torch.equal(g["log_prob"], p["log_prob"][cand]) and j["log_prob"] == scores["log_prob"].numpy()[c].tolist()
            nn_min, _ = diversity.coverage(feat[c])
            print(f"{select_by}/{space} rows_per_call {rows_per_call} object {i}: kept {c.tolist()} ranks {rank.tolist()} "
                  f"novelty {nov.tolist()}; nearest pair {nn_min:.5f} against {diversity.coverage(feat[top[0, :k]])[0]:.5f} of the top {k}")
            # the smallest gap is the kept set's closest pair: fp32 chains of at most 292 + 3 additions after a rounded difference and
            # product, (295 + 2) * 2^-24 = 1.8e-5 relative on the squared distance at worst, half of it on the root
            assert nn_min == pytest.approx(float(nov[1:].min()) ** 0.5, rel=2e-5, abs=1e-12)
            differs |= set(c.tolist()) != set(top[0, :k].tolist())
        if first is None:
            first = got
        assert all(same_result(a, b) for a, b in zip(got, first)), f"rows_per_call {rows_per_call}: differs from the 16384-row call"
    assert differs, "farthest-point order coincides with rank order on every object: the selection is not exercised"


def _run_main(dataset, out_dir, extra, mano):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", DATASETS)
def test_entry_points_write_the_same_files_for_every_grouping(dataset, tmp_path):
    mano = mano_pkl(tmp_path)
    M, P, k, n_obj = 8, 6, 3, 3
    base = ["--num_objects", str(n_obj), "--points", "256", "--num_grasp", str(k), "--candidates", str(M)]
    flags = base + ["--diverse_pool", str(P)]
    names0, bytes0 = _run_main(dataset, str(tmp_path / "default"), flags, mano)
    assert names0 == [f"obj_id_synthetic_{i}.json" for i in range(n_obj)]
    for tag, extra in (("m", ["--rows_per_call", str(M)]), ("loop", ["--rows_per_call", "0"])):
        names, data = _run_main(dataset, str(tmp_path / tag), flags + extra, mano)
        assert names == names0 and data == bytes0, f"--rows_per_call {extra[1]}: the files differ"
    _, best = _run_main(dataset, str(tmp_path / "best"), base, mano)                    # best-of-M without the flag ...
    _, zero = _run_main(dataset, str(tmp_path / "zero"), base + ["--diverse_pool", "0", "--diverse_space", "verts"], mano)
    assert zero == best                                                                 # ... is what the flag at its default writes
    for data, b in zip(bytes0, best):
        j, jb = json.loads(data), json.loads(b)
        assert list(j) == list(jb) + ["rank", "novelty"] and all(len(j[f]) == k for f in j)
        assert j["rank"][0] == 0 and j["novelty"][0] == -1.0 and j["candidate"][0] == jb["candidate"][0]
        assert len(set(j["rank"])) == k and all(0 <= r < P for r in j["rank"])
        assert all(a >= b_ >= 0 for a, b_ in zip(j["novelty"][1:], j["novelty"][2:]))
