"""The diversity statistic on the device: dvq_segment_kmeans (one fused Lloyd kernel, one workgroup per segment), its host API
(ops.segment_kmeans, diversity.kmeans_init / device_diversity) and the ``--diversity`` mode of generate_for_objects / the entry
points.  The reference is tests/segment_kmeans_ref.py (numpy float32, one rounding per operation): on the CPU it is compared with
the reference project's own scipy path, on the GPU every output of the kernel is compared with it bit for bit."""
import functools
import json
import lzma
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, diversity, generate, ops, synth

import diverse_select_ref as dref
import segment_kmeans_ref as kref

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
DATASETS = ["obman", "ho3d", "grab", "FHAB"]
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


# ------------------------------------------------------------------------------------------------------ CPU: restatement against scipy
def lloyd64(x, init, iters=100):
    """Plain float64 Lloyd from the same start (two-pass means): labels, centres, and the smallest relative gap between a row's two
    nearest centres seen in any iteration -- how close the run came to a tie that rounding could decide either way."""
    c = x[init].copy()
    gap, lab = np.inf, None
    for _ in range(iters + 1):
        d = ((x[:, None, :] - c[None]) ** 2).sum(axis=2)
        two = np.sort(d, axis=1)[:, :2] if c.shape[0] > 1 else np.concatenate([d, d + 1.0], axis=1)
        gap = min(gap, float(((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)).min()))
        new = d.argmin(axis=1)
        if lab is not None and np.array_equal(new, lab):
            break
        lab = new
        for j in range(c.shape[0]):
            if (lab == j).any():
                c[j] = x[lab == j].mean(axis=0)
    return lab, c, gap


@pytest.mark.parametrize("k,M,D", [(8, 300, 3), (20, 600, 61), (20, 300, 8)])
def test_restatement_equals_the_reference_scipy_path(k, M, D):
    """scipy.cluster.vq.kmeans(x, guess) + vq in float64 from the farthest-point start: the same number of centres, identical labels,
    equal entropy, centres within 1e-5, mean distance within 1e-6 relative.  A segment may be left out only when the float64 run came
    within 1e-6 (relative) of a tie between a row's two nearest centres; at most one of the twelve."""
    import scipy.cluster.vq
    from scipy.stats import entropy
    O = 12
    feat = np.random.default_rng(1).uniform(-1, 1, (O * M, D)).astype(F32)
    left_out = []
    for o in range(O):
        x = feat[o * M:(o + 1) * M]
        init = dref.select_one(x, k)[0].astype(np.int64)
        centres, counts, assign, dist, used = kref.kmeans_one(x, init, 100)
        x64 = x.astype(np.float64)
        codes, _ = scipy.cluster.vq.kmeans(x64, x64[init])
        labels, d = scipy.cluster.vq.vq(x64, codes)
        hist, _ = np.histogram(labels, len(codes))
        ent, mean = kref.statistics(counts, dist)
        lab64, c64, gap = lloyd64(x64, init)
        same = (len(codes) == k and np.array_equal(labels, assign) and np.array_equal(lab64, assign))
        print(f"segment {o}: {used} iterations, scipy centres {len(codes)}, labels equal {same}, smallest two-centre gap {gap:.3e}, "
              f"max centre difference {np.abs(codes - centres).max() if len(codes) == k else float('nan'):.2e}, "
              f"entropy {ent:.12f} scipy {float(entropy(hist)):.12f}, mean distance {mean:.9f} scipy {float(d.mean()):.9f}")
        if not same and gap < 1e-6:
            left_out.append(o)
            continue
        assert 0 < used < 100, f"segment {o}: the restatement did not converge"
        assert len(codes) == k, f"segment {o}: scipy kept {len(codes)} of {k} centres"
        assert np.array_equal(labels, assign), f"segment {o}: {int((labels != assign).sum())} labels differ from scipy's"
        assert np.array_equal(lab64, assign), f"segment {o}: labels differ from the float64 Lloyd run"
        assert np.array_equal(hist, counts) and ent == pytest.approx(float(entropy(hist)), rel=1e-12, abs=1e-12)
        assert np.abs(codes - centres).max() <= 1e-5 and np.abs(c64 - centres).max() <= 1e-5
        assert mean == pytest.approx(float(d.mean()), rel=1e-6)
    assert len(left_out) <= 1, f"segments left out as near-ties: {left_out}"


def test_statistics_helper_equals_scipy_entropy():
    from scipy.stats import entropy
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 50, 20)
    counts[[2, 7]] = 0
    assign = np.repeat(np.arange(20), counts)
    dist = rng.uniform(0, 4, assign.size).astype(F32)
    with_invalid = np.concatenate([dist, np.full(5, np.nan, F32)])           # five rows that took no part
    ent, mean, n = diversity.kmeans_statistics(counts, with_invalid)
    assert n == counts.sum() and ent == pytest.approx(float(entropy(counts)), rel=1e-13)
    assert mean == pytest.approx(float(np.sqrt(dist.astype(np.float64)).mean()), rel=1e-13)
    assert (ent, mean) == pytest.approx(kref.statistics(counts, with_invalid), rel=1e-13)
    assert diversity.kmeans_statistics([5, 0, 0], np.zeros(5, F32)) == (0.0, 0.0, 5)
    ent, mean, n = diversity.kmeans_statistics([0, 0], np.full(3, np.nan, F32))
    assert np.isnan(ent) and np.isnan(mean) and n == 0
    seg = diversity.segment_statistics(20, np.stack([counts, counts]), np.concatenate([with_invalid, with_invalid]), [4, 9])
    assert [s["iters"] for s in seg] == [4, 9] and seg[0]["counts"] == counts.tolist() and seg[0]["n_valid"] == n + counts.sum()
    assert seg[0]["entropy"] == seg[1]["entropy"] and seg[0]["clusters"] == 20 and all(isinstance(v, int) for v in seg[0]["counts"])
    assert json.loads(json.dumps(seg[0])) == seg[0]


def test_kmeans_init_spaced_and_its_errors():
    init = diversity.kmeans_init(3, 100, 20)
    assert init.dtype == torch.int64 and tuple(init.shape) == (3, 20) and init.is_contiguous()
    assert init[0].tolist() == [j * 100 // 20 for j in range(20)] and torch.equal(init[0], init[2])
    assert diversity.kmeans_init(1, 7, 3)[0].tolist() == [0, 2, 4] and diversity.kmeans_init(1, 5, 5)[0].tolist() == [0, 1, 2, 3, 4]
    assert tuple(diversity.kmeans_init(0, 5, 5).shape) == (0, 5)
    for M, k in ((65536, 20), (1200, 20), (101, 64)):
        pos = diversity.kmeans_init(1, M, k)[0].tolist()
        assert len(set(pos)) == k and pos[0] == 0 and max(pos) < M
    for args in ((1, 5, 6), (1, 5, 0), (-1, 5, 2), (1, 5, 2, "random")):
        with pytest.raises(RuntimeError, match="kmeans_init"):
            diversity.kmeans_init(*args)
    with pytest.raises(RuntimeError, match="spaced"):                   # beyond the selection kernel's cap: the message names the way out
        diversity.kmeans_init(1, ops.SEGMENT_DIVERSE_MAX_D + 1, 20, "farthest", params=torch.zeros(ops.SEGMENT_DIVERSE_MAX_D + 1, 3))
    with pytest.raises(RuntimeError, match="params"):
        diversity.kmeans_init(1, 50, 5, "farthest")


def test_ops_refuse_bad_arguments_before_any_device_use():
    feat, init = torch.zeros(6, 5), torch.tensor([[0, 1], [2, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.segment_kmeans(feat, init, 2, 3, 10)                                        # well-formed, but not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.segment_kmeans(torch.zeros(6, 8)[:, 1:6], init, 2, 3, 0)                    # a column slice is well-formed too
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        diversity.device_diversity(feat, 2, 3, cls_num=2)
    wide = torch.zeros(6, 10)
    big = ops.SEGMENT_KMEANS_MAX_M + 1
    assert ops.SEGMENT_KMEANS_MAX_M >= 65536
    for args in ((feat.double(), init, 2, 3, 1), (feat, init.int(), 2, 3, 1), (feat, init.float(), 2, 3, 1),
                 (wide[:, ::2], init, 2, 3, 1),                                          # stride(1) != 1
                 (torch.zeros(1, 5).expand(6, 5), init, 2, 3, 1),                        # ld = 0 < D
                 (torch.zeros(30).as_strided((6, 5), (4, 1)), init, 2, 3, 1),            # ld = 4 < D: rows overlap
                 (feat, torch.zeros(2, 4, dtype=torch.int64), 2, 3, 1),                  # k > M
                 (feat, torch.zeros(2, 0, dtype=torch.int64), 2, 3, 1),                  # k = 0
                 (torch.zeros(70, 2), torch.zeros(1, 65, dtype=torch.int64), 1, 70, 1),  # k = 65
                 (feat, init, 2, 3, -1),                                                 # iters < 0
                 (torch.zeros(3, 65), torch.zeros(1, 2, dtype=torch.int64), 1, 3, 1),    # D = 65
                 (torch.zeros(3, 2334), torch.zeros(1, 2, dtype=torch.int64), 1, 3, 1),  # vertex space
                 (torch.zeros(3, 0), torch.zeros(1, 2, dtype=torch.int64), 1, 3, 1),     # D = 0
                 (torch.zeros(1, 1).expand(big, 1), torch.zeros(1, 1, dtype=torch.int64), 1, big, 1),   # M beyond the cap
                 (feat, init.reshape(-1), 2, 3, 1), (feat, init[:1], 2, 3, 1), (feat, init.t(), 2, 3, 1),   # init shape / layout
                 (feat[:5], init, 2, 3, 1), (feat.reshape(-1), init, 2, 3, 1),           # feat is not [O*M, D]
                 (feat, init, -1, 3, 1), (feat, init, 2, 3, 1, torch.zeros(1)),          # O < 0; an err flag of the wrong type
                 (None, init, 2, 3, 1)):
        with pytest.raises(RuntimeError) as e:
            ops.segment_kmeans(*args)
        assert "no CPU fallback" not in str(e.value), f"{args[2:]}: refused only for the device, not for the argument"
    with pytest.raises(RuntimeError, match="init must be"):
        diversity.device_diversity(feat, 2, 3, cls_num=2, init=torch.zeros(2, 3, dtype=torch.int64))


@pytest.mark.parametrize("dataset", DATASETS)
def test_parser_has_the_diversity_flag(dataset):
    assert generate.build_parser(dataset).parse_args([]).diversity == 0 and generate.parse_args(dataset, []).diversity == 0
    a = generate.parse_args(dataset, ["--num_grasp", "100", "--diversity", "20"])
    assert (a.num_grasp, a.diversity) == (100, 20)
    assert generate.parse_args(dataset, ["--num_grasp", "20", "--diversity", "20"]).diversity == 20
    for bad in (["--num_grasp", "19", "--diversity", "20"], ["--num_grasp", "100", "--diversity", "-1"],
                ["--num_grasp", "100", "--diversity", "65"]):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_generate_for_objects_refuses_a_bad_cluster_count_before_any_work():
    for kw in (dict(diversity=6), dict(diversity=-1), dict(diversity=65)):
        with pytest.raises(RuntimeError, match="diversity"):
            generate.generate_for_objects(None, [torch.zeros(4, 8)], 5 if kw["diversity"] != 65 else 100, True, 0, [0], **kw)


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_segment_kmeans" in _lib.SIGNATURES and len(_lib.SIGNATURES["dvq_segment_kmeans"][1]) == 15
    assert "int dvq_segment_kmeans(" in header and hasattr(lib, "dvq_segment_kmeans") and lib.dvq_abi_version() == 10
    assert "dvq_segment_kmeans" in re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    text = " ".join(re.search(r"/\* Lloyd's k-means inside each segment.*?\*/", header, re.S).group(0).replace(" * ", " ").split())
    for phrase in ("a row is valid iff all D features are finite", "assign = -1 and dist = NaN",
                   "the eight-chain squared distance of dvq_segment_diverse", "((acc0 + acc1) + (acc2 + acc3)) + ((acc4 + acc5) + (acc6 + acc7))",
                   "centre j replaces best iff d_j < d_best, or d_best is NaN and d_j is not",
                   "chain g starts at +0.0f and adds x[i][j] over ascending segment positions i = g (mod 4) with assign[i] == c",
                   "S = (ch0 + ch1) + (ch2 + ch3)", "S / (float)count[c] by IEEE division", "A centre with count == 0 keeps its value",
                   "stop when no assignment changed, with iters_used = u", "iters = 0 gives 0",
                   "assign, dist and counts are always those of the centres returned", "a duplicate within a segment or an invalid row",
                   "no row of the segment is read through a bad index", "1 <= k <= 64, 1 <= D <= 64", "Vertex space (D = 2334) is out of scope"):
        assert phrase in text, phrase
    assert f"k <= M <= {ops.SEGMENT_KMEANS_MAX_M}" in text and (ops.SEGMENT_KMEANS_MAX_K, ops.SEGMENT_KMEANS_MAX_D) == (64, 64)
    source = open(os.path.join(_lib.CSRC, "kmeans.hip")).read()
    assert f"KM_MAX_M = {ops.SEGMENT_KMEANS_MAX_M};" in source and "kmeans.hip" in open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "__syncthreads" not in source and "atomic" not in source.replace("atomicOr(err, 1)", "") and "asm" not in source


# ------------------------------------------------------------------------------------------------------ GPU: the kernel
@functools.lru_cache(maxsize=None)
def kmeans_case(O, M, k, D, iters=100, clustered=True):
    """(feat [O*M,D], init [O,k], reference outputs): rows around 2k well-separated-ish blobs so that Lloyd moves for a while; the start
    is k distinct random positions."""
    rng = np.random.default_rng([O, M, k, D])
    feat = rng.standard_normal((O * M, D)).astype(F32)
    if clustered:
        blobs = (rng.standard_normal((2 * k, D)) * 1.5).astype(F32)
        feat = (feat * F32(0.7) + blobs[rng.integers(0, 2 * k, O * M)]).astype(F32)
    init = np.stack([rng.permutation(M)[:k] for _ in range(O)]).astype(np.int64)
    want = kref.segment_kmeans(feat, init, O, M, iters)
    for a in (feat, init) + want:
        a.setflags(write=False)
    return feat, init, want


def run(feat, init, O, M, iters, **kw):
    out = ops.segment_kmeans(feat if torch.is_tensor(feat) else gpu(feat), gpu(init), O, M, iters, **kw)
    k, D = init.shape[1], feat.shape[1]
    assert [t.dtype for t in out] == [torch.float32, torch.int32, torch.int32, torch.float32, torch.int32]
    assert [tuple(t.shape) for t in out] == [(O, k, D), (O, k), (O * M,), (O * M,), (O,)]
    return tuple(t.cpu().numpy() for t in out)


NAMES = ("centres", "counts", "assign", "dist", "iters_used")


def assert_equal_bits(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        print(what, name, "got", g.reshape(-1)[:10], "reference", w.reshape(-1)[:10])
        if g.dtype == F32:
            g, w = bits(g), bits(w)
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}: {name} differs from the reference in {int((g != w).sum())} places"


KERNEL_CASES = [(3, 300, 8, 3, 100), (1, 1, 1, 5, 100), (2, 257, 5, 7, 100), (2, 300, 6, 64, 100), (2, 300, 4, 1, 100),
                (2, 40, 40, 9, 100), (2, 64, 64, 33, 100), (1, 5000, 20, 61, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(KERNEL_CASES)))
def test_segment_kmeans_equals_the_reference_bit_for_bit(case):
    O, M, k, D, iters = KERNEL_CASES[case]
    feat, init, want = kmeans_case(O, M, k, D, iters)
    got = run(feat, init, O, M, iters)
    print("iterations", want[4], "counts", want[1][0])
    assert_equal_bits(got, want, str(KERNEL_CASES[case]))
    assert (want[1].sum(axis=1) == M).all() and (want[4] >= 0).all()
    if case == 0:
        assert (want[4] >= 3).all() and (want[4] < iters).all(), "the case must take several iterations and converge"
    if case == 7:
        assert M > ops.SEGMENT_TOPK_MAX_M and want[4][0] == iters                # the limit ends the loop


@pytest.mark.gpu
def test_segment_kmeans_reads_a_column_slice_in_place():
    O, M, k, D, iters = 2, 600, 20, 61, 100
    feat, init, want = kmeans_case(O, M, k, D, iters)
    wide = torch.full((O * M, 70), float("nan"), device=DEV)
    wide[:, 5:66] = gpu(feat)
    view = wide[:, 5:66]                                                # ld = 70, an unaligned base
    assert view.stride() == (70, 1) and not view.is_contiguous()
    assert_equal_bits(run(view, init, O, M, iters), want, "slice")
    assert_equal_bits(run(feat, init, O, M, iters), want, "contiguous")
    assert (want[4] >= 3).all() and (want[4] < iters).all()


@pytest.mark.gpu
def test_segment_kmeans_iteration_limits():
    O, M, k, D = 2, 500, 10, 16
    feat, init, conv = kmeans_case(O, M, k, D, 100)
    assert (conv[4] >= 6).all(), f"the data must need several iterations (took {conv[4]})"
    zero = kref.segment_kmeans(feat, init, O, M, 0)
    assert (zero[4] == 0).all() and np.array_equal(bits(zero[0]), bits(feat.reshape(O, M, D)[np.arange(O)[:, None], init]))
    assert_equal_bits(run(feat, init, O, M, 0), zero, "iters = 0")
    one = kref.segment_kmeans(feat, init, O, M, 1)
    assert (one[4] == 1).all() and not np.array_equal(one[2], conv[2]) and not np.array_equal(one[2], zero[2])
    assert_equal_bits(run(feat, init, O, M, 1), one, "iters = 1")
    assert_equal_bits(run(feat, init, O, M, 100), conv, "iters = 100")
    exact = kref.segment_kmeans(feat, init, O, M, int(conv[4].max()))                    # the limit and the convergence test meet
    assert_equal_bits(run(feat, init, O, M, int(conv[4].max())), exact, "iters = iterations needed")
    for o in range(O):                                                  # counts and dist belong to the centres returned
        x = feat[o * M:(o + 1) * M]
        a, d = kref.assign_rows(x, one[0][o], np.ones(M, bool))
        assert np.array_equal(a, one[2][o * M:(o + 1) * M]) and np.array_equal(np.bincount(a, minlength=k), one[1][o])


@pytest.mark.gpu
def test_segment_kmeans_with_rows_that_are_not_finite_and_empty_centres():
    O, M, k, D = 4, 300, 6, 9
    rng = np.random.default_rng(21)
    feat = rng.standard_normal((O * M, D)).astype(F32)
    init = np.stack([rng.permutation(M)[:k] for _ in range(O)]).astype(np.int64)
    for o in (0, 2):                                                    # NaN, +Inf and -Inf rows away from the starting rows
        free = np.setdiff1d(np.arange(M), init[o])
        rows = o * M + rng.permutation(free)[:30]
        feat[rows[:10], rng.integers(0, D, 10)] = np.nan
        feat[rows[10:20], rng.integers(0, D, 10)] = np.inf
        feat[rows[20:], rng.integers(0, D, 10)] = -np.inf
    feat[M:2 * M, 4] = np.nan                                           # segment 1: no valid row at all
    # segment 3: every row is a copy of one of three rows.  Equal rows always share a centre (ties go to the lowest index), so at
    # most three of the six centres hold rows at any time and the others end empty, keeping the value they had
    feat[3 * M:] = feat[3 * M:3 * M + 3][rng.integers(0, 3, M)]
    want = kref.segment_kmeans(feat, init, O, M, 100)
    assert (want[2][:M] == -1).sum() == 30 and np.isnan(want[3][:M]).sum() == 30 and want[1][0].sum() == M - 30
    assert (want[1][1] == -1).all() and (want[2][M:2 * M] == -1).all() and np.isnan(want[0][1]).all() and want[4][1] == -1
    assert (want[1][3] == 0).sum() >= 3 and want[1][3].sum() == M and np.isfinite(want[0][3]).all()
    err = ops.new_err_flag(torch.device(DEV))
    got = run(feat, init, O, M, 100, err=err)
    assert int(err.item()) == 1                                         # raised by the segment without a valid row
    assert_equal_bits(got, want, "rows that are not finite")
    sub = [0, 2, 3]                                                     # without that segment nothing is flagged
    f3 = np.concatenate([feat[o * M:(o + 1) * M] for o in sub])
    err = ops.new_err_flag(torch.device(DEV))
    got = run(f3, init[sub], 3, M, 100, err=err)
    assert int(err.item()) == 0
    assert_equal_bits(got, [want[0][sub], want[1][sub], want[2].reshape(O, M)[sub].reshape(-1), want[3].reshape(O, M)[sub].reshape(-1),
                            want[4][sub]], "the three other segments")


@pytest.mark.gpu
def test_segment_kmeans_flags_a_bad_init():
    O, M, k, D, iters = 3, 300, 8, 3, 100
    feat, init, want = kmeans_case(O, M, k, D, iters)
    nan_row = feat.copy()
    nan_row[M + init[1, 5], 1] = np.inf
    for what, f, entry in (("beyond the segment", feat, M), ("negative", feat, -1), ("far beyond", feat, 1 << 40),
                           ("a duplicate", feat, int(init[1, 0])), ("an invalid row", nan_row, int(init[1, 5]))):
        bad = init.copy()
        bad[1, 5] = entry
        assert kref.bad_init(f[M:2 * M], bad[1]) and not kref.bad_init(f[:M], bad[0])
        with pytest.raises(RuntimeError, match="segment_kmeans: init"):
            ops.segment_kmeans(gpu(f), gpu(bad), O, M, iters)
        err = ops.new_err_flag(torch.device(DEV))
        got = run(f, bad, O, M, iters, err=err)                         # the caller's flag: set, segment 1 is -1 / NaN, the others right
        assert int(err.item()) == 1, what
        assert (got[1][1] == -1).all() and (got[2][M:2 * M] == -1).all() and got[4][1] == -1, what
        assert np.isnan(got[0][1]).all() and np.isnan(got[3][M:2 * M]).all(), what
        assert_equal_bits(got, kref.segment_kmeans(f, bad, O, M, iters), what)
        assert_equal_bits([got[0][[0, 2]], got[1][[0, 2]], got[4][[0, 2]]], [want[0][[0, 2]], want[1][[0, 2]], want[4][[0, 2]]], what)
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL, nothing launched
    f, p, e = gpu(feat), gpu(init), ops.new_err_flag(torch.device(DEV))
    out = torch.zeros(O * M * 4, dtype=torch.int32, device=DEV)
    call = lambda ld, D, O, M, k, iters: lib.dvq_segment_kmeans(f.data_ptr(), ld, D, p.data_ptr(), O, M, k, iters, out.data_ptr(),
                                                                out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                                                e.data_ptr(), None)
    for args in ((3, 3, 3, 300, 0, 5), (3, 3, 3, 300, 65, 5), (3, 3, 3, 7, 8, 5), (3, 3, 1, ops.SEGMENT_KMEANS_MAX_M + 1, 8, 5),
                 (3, 0, 3, 300, 8, 5), (65, 65, 1, 8, 4, 5), (2, 3, 3, 300, 8, 5), (3, 3, -1, 300, 8, 5), (3, 3, 3, 300, 8, -1)):
        assert call(*args) == 1, args
    assert lib.dvq_segment_kmeans(None, 3, 3, p.data_ptr(), 3, 300, 8, 5, out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(),
                                  out.data_ptr(), e.data_ptr(), None) == 1
    assert call(3, 3, 0, 300, 8, 5) == 0 and int(e.item()) == 0 and int(out.abs().sum()) == 0     # O = 0: a no-op
    empty = ops.segment_kmeans(f[:0], p[:0], 0, M, iters)
    assert [tuple(t.shape) for t in empty] == [(0, k, D), (0, k), (0,), (0,), (0,)]


@pytest.mark.gpu
def test_segment_kmeans_of_a_segment_does_not_depend_on_the_batch():
    O, M, k, D, iters = 300, 8, 3, 61, 100                              # more workgroups than compute units
    feat, init, want = kmeans_case(O, M, k, D, iters, clustered=False)
    got = run(feat, init, O, M, iters)
    assert_equal_bits(got, want, "300 segments")
    f, p, err = gpu(feat), gpu(init), ops.new_err_flag(torch.device(DEV))
    alone = [ops.segment_kmeans(f[o * M:(o + 1) * M], p[o:o + 1], 1, M, iters, err=err) for o in range(O)]
    assert int(err.item()) == 0
    assert_equal_bits([torch.cat([a[i] for a in alone]).cpu().numpy() for i in range(5)], got, "300 segments alone")


@pytest.mark.gpu
def test_device_diversity_and_the_farthest_start():
    O, M, k, D = 3, 300, 8, 3
    feat, _, _ = kmeans_case(O, M, k, D, 100)
    f = gpu(feat)
    far = diversity.kmeans_init(O, M, k, "farthest", params=f)
    assert far.dtype == torch.int64 and tuple(far.shape) == (O, k)
    want_far = np.stack([dref.select_one(feat[o * M:(o + 1) * M], k)[0] for o in range(O)])
    assert np.array_equal(far.cpu().numpy(), want_far)
    for how, init in (("spaced", np.tile(np.arange(k) * M // k, (O, 1))), ("farthest", want_far), (far, want_far)):
        got = diversity.device_diversity(f, O, M, cls_num=k, iters=100, init=how)
        ref = kref.segment_kmeans(feat, init, O, M, 100)
        assert len(got) == O
        for o in range(O):
            ent, mean = kref.statistics(ref[1][o], ref[3][o * M:(o + 1) * M])
            assert got[o] == {"clusters": k, "entropy": ent, "mean_dist": mean, "iters": int(ref[4][o]), "counts": ref[1][o].tolist(),
                              "n_valid": M}
            alone = diversity.device_diversity(f[o * M:(o + 1) * M], 1, M, cls_num=k, iters=100,
                                               init=how if isinstance(how, str) else how[o:o + 1])
            assert alone[0] == got[o], "a segment's figures depend on the call it shares"
    assert diversity.device_diversity(f[:0], 0, M, cls_num=k) == []


# ------------------------------------------------------------------------------------------------------ GPU: end to end
def _gennet():
    """The synthetic net of tests/test_generate_batched.py::_gennet."""
    from conftest import GOLDEN, gen_state_dict
    from dvqvae_amd import mano as dmano
    from dvqvae_amd.network.gen_net import GenNet
    net = GenNet()
    net.load_state_dict(gen_state_dict(net.state_dict(), np.load(os.path.join(GOLDEN, "g7_gen.npz"))), strict=True)
    net.eval().to(DEV)
    net.set_rh_mano(dmano.ManoLayer(dmano.synthetic_mano_arrays()).to(DEV))
    return net


def expected_entry(params, clusters):
    """The "diversity" dict of one object from its kept parameters [G,61] (host), through the restatement."""
    G = params.shape[0]
    init = np.asarray([[j * G // clusters for j in range(clusters)]])
    _, counts, _, dist, used = kref.segment_kmeans(params, init, 1, G, generate.DIVERSITY_ITERS)
    ent, mean = kref.statistics(counts[0], dist)
    return {"clusters": clusters, "entropy": ent, "mean_dist": mean, "iters": int(used[0]), "counts": counts[0].tolist()}


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [True, False])
def test_generate_for_objects_reports_the_diversity_of_the_kept_grasps(rotate):
    net = _gennet()
    seed, G, K, indices = 9, 24, 5, [5, 2, 11, 7]
    objs = [synth.synthetic_clouds(1, n, seed=50 + i)[0] for i, n in enumerate((700, 300, 700, 300))]
    plain = generate.generate_for_objects(net, objs, G, rotate, seed, indices)
    zero = generate.generate_for_objects(net, objs, G, rotate, seed, indices, diversity=0)
    first = None
    for rows_per_call in (16384, 2 * G, 1):
        got = generate.generate_for_objects(net, objs, G, rotate, seed, indices, rows_per_call=rows_per_call, diversity=K)
        for i, (g, p, z) in enumerate(zip(got, plain, zero)):
            assert set(z) == set(p) and z["json"] == p["json"] and "diversity" not in z["json"]
            assert set(g) == set(p) | {"diversity"} and list(g["json"]) == list(p["json"]) + ["diversity"]
            assert torch.equal(g["params"], p["params"]) and torch.equal(g["vertices"], p["vertices"])
            assert {k: v for k, v in g["json"].items() if k != "diversity"} == p["json"]
            want = expected_entry(p["params"].cpu().numpy(), K)
            print(f"rows_per_call {rows_per_call} object {i}:", g["json"]["diversity"])
            assert g["diversity"] == want and g["json"]["diversity"] == want
            assert list(want) == ["clusters", "entropy", "mean_dist", "iters", "counts"] and sum(want["counts"]) == G
        if first is None:
            first = got
        assert [g["json"] for g in got] == [f["json"] for f in first], f"rows_per_call {rows_per_call}: differs from the 16384-row call"


def _run_main(dataset, out_dir, extra, mano="/nonexistent"):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", DATASETS)
def test_entry_points_write_the_same_diversity_for_every_grouping(dataset, tmp_path):
    G, K, n_obj = 12, 4, 5
    base = ["--num_objects", str(n_obj), "--points", "256", "--num_grasp", str(G)]
    flags = base + ["--diversity", str(K)]
    names0, bytes0 = _run_main(dataset, str(tmp_path / "default"), flags)
    assert names0 == [f"obj_id_synthetic_{i}.json" for i in range(n_obj)]
    pooled0 = open(tmp_path / "default" / "diversity.json", "rb").read()
    for tag, extra in (("loop", ["--rows_per_call", "0"]), ("thirty", ["--rows_per_call", "30"])):
        names, data = _run_main(dataset, str(tmp_path / tag), flags + extra)
        assert names == names0 and data == bytes0, f"--rows_per_call {extra[1]}: the files differ"
        assert open(tmp_path / tag / "diversity.json", "rb").read() == pooled0, f"--rows_per_call {extra[1]}: diversity.json differs"
    for tag, extra in (("plain", []), ("zero", ["--diversity", "0"])):
        _, plain = _run_main(dataset, str(tmp_path / tag), base + extra)
        assert not os.path.exists(tmp_path / tag / "diversity.json")
        if tag == "plain":
            first = plain
        assert plain == first, f"{tag}: --diversity 0 is not the run without the flag"
    kept = []
    for data, p in zip(bytes0, first):
        j, jp = json.loads(data), json.loads(p)
        assert list(j) == list(jp) + ["diversity"] and {k: v for k, v in j.items() if k != "diversity"} == jp
        params = np.asarray(jp["recon_params"], dtype=F32).reshape(G, 61)
        assert j["diversity"] == expected_entry(params, K)
        kept.append(params)
    pooled = json.loads(pooled0)
    want = expected_entry(np.concatenate(kept), K)
    print("pooled", pooled)
    assert pooled == {**want, "grasps": n_obj * G} and sum(pooled["counts"]) == n_obj * G


def mano_pkl(tmp_path):
    """tests/golden/g9_mano_right.pkl.xz unpacked: the path of a MANO_RIGHT.pkl (real topology: the scores need the faces)."""
    path = str(tmp_path / "MANO_RIGHT.pkl")
    if not os.path.exists(path):
        with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
    return path


@pytest.mark.gpu
def test_diversity_follows_selection_and_push_out(tmp_path):
    """The statistic is that of the grasps WRITTEN: after best-of-M, the diverse pool and the push-out, riding in the same copy."""
    mano = mano_pkl(tmp_path)
    G, K, n_obj = 6, 3, 3
    base = ["--num_objects", str(n_obj), "--points", "256", "--num_grasp", str(G)]
    for tag, extra in (("refine", ["--refine_steps", "2"]),
                       ("both", ["--candidates", "12", "--diverse_pool", "8", "--refine_steps", "2", "--log_prob", "1"])):
        _, plain = _run_main("ho3d", str(tmp_path / tag), base + extra, mano)
        names, data = _run_main("ho3d", str(tmp_path / (tag + "_k")), base + extra + ["--diversity", str(K)], mano)
        assert len(data) == n_obj
        if tag == "both":
            _, split = _run_main("ho3d", str(tmp_path / "both_k1"), base + extra + ["--diversity", str(K), "--rows_per_call", "1"], mano)
            assert split == data
        for d, p in zip(data, plain):
            j, jp = json.loads(d), json.loads(p)
            assert list(j) == list(jp) + ["diversity"] and {k: v for k, v in j.items() if k != "diversity"} == jp, tag
            assert j["diversity"] == expected_entry(np.asarray(jp["recon_params"], dtype=F32).reshape(G, 61), K), tag
