"""The seams of csrc/grasp_scan.h -- the hand in LDS and the nearest-vertex scan that dvq_grasp_scores, dvq_grasp_refine and
dvq_grasp_wrench share -- at sizes the MANO-sized cases of the other grasp tests do not reach: hands of 3, 5 and 7 vertices (no
four-vertex block at all; one block and a tail of one; one block and a tail of three) against clouds of 1, 257 and 1025 points (one
point; a second thread block of points; a second 4 x 256 pass with a single live point).  Every batch has a finite row, a row whose
hand holds a NaN (the whole row takes the exact scan) and a row whose last point holds an inf (only that thread's pass takes it).
The references are tests/grasp_score_ref.py, grasp_refine_ref.py and grasp_wrench_ref.py; everything is compared bit for bit.

The three levels of the push-out (csrc/grasp_refine.hip: translation, rigid, fingers) are one kernel text, so the two upper levels go
to the same sizes (``ladder``): the pivot at vertex 0, two fingers that share the rim vertices alternately with weights 1 and 0.5, their
knuckles at vertices 1 and 2, against tests/grasp_refine_rigid_ref.py and grasp_refine_fingers_ref.py.

dvq_grasp_ttt runs the header's vertex walk with a target flag per vertex (a packed byte plane: a word per four-vertex block, a byte
per tail vertex), so it goes to the same sizes with every odd vertex a target: at V = 5 the tail vertex is no target, at V = 7 the
tail holds both kinds.  Against tests/grasp_ttt_ref.py bit for bit, and its three scores against dvq_grasp_scores on the device."""
import functools
import hashlib

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import contact, ops, synth

import grasp_refine_fingers_ref as fingers_ref
import grasp_refine_ref as refine_ref
import grasp_refine_rigid_ref as rigid_ref
import grasp_score_ref as score_ref
import grasp_ttt_ref as ttt_ref
import grasp_wrench_ref as wrench_ref

DEV = "cuda:0"
THR, INV_LENGTH, STEPS = 0.02 ** 2, 10.0, 2
SIZES = [(V, N) for V in (3, 5, 7) for N in (1, 257, 1025)]
SCORES = ("penetration", "n_interior", "n_contact")
REFINE = ("offset", "iter") + SCORES
WRENCH = SCORES + ("centre", "sums", "key")
RIGID = ("offset", "quat", "iter") + SCORES
FINGERS = fingers_ref.NAMES
TTT = ("penetration", "contact_sum", "n_interior", "n_contact", "grad")
N_FINGERS, MAX_CURL = 2, 0.35
IDENTITY = np.asarray([1, 0, 0, 0], np.float32)


def fan(V):
    """A triangle fan about vertex 0: open for V = 3 (one face) and V = 5 (three faces), closed for V = 7 (six faces)."""
    rim = list(range(1, V))
    pairs = list(zip(rim, rim[1:])) + ([(rim[-1], rim[0])] if V == 7 else [])
    return np.asarray([(0, a, b) for a, b in pairs], np.int64)


@functools.lru_cache(maxsize=None)
def case(V, N):
    """(hand [3,V,3], faces, obj [3,N,3], the three references' outputs as dicts): computed once per size, never written to."""
    hand = synth.synthetic_normal((3, V, 3), 61, f"scan/{V}x{N}/h", 0.03).numpy()
    obj = synth.synthetic_normal((3, N, 3), 61, f"scan/{V}x{N}/o", 0.03).numpy()
    hand[1, V - 1, 1] = np.nan
    obj[2, N - 1, 0] = np.inf
    faces = fan(V)
    with np.errstate(all="ignore"):
        want = {"scores": dict(zip(SCORES, score_ref.grasp_scores(hand, faces, obj, THR))),
                "refine": dict(zip(REFINE, refine_ref.grasp_refine(hand, faces, obj, STEPS, contact_threshold=THR))),
                "wrench": wrench_ref.grasp_wrench(hand, faces, obj, INV_LENGTH, THR)}
    for a in [hand, faces, obj] + [x for d in want.values() for x in d.values()]:
        a.setflags(write=False)
    return hand, faces, obj, want


@functools.lru_cache(maxsize=None)
def ladder(V, N):
    """``case(V, N)``'s hand and cloud for the two upper levels: (pivot [3,3], vert_part [V], vert_w [V], knuckle [3,2,3], the rigid and
    the fingers reference's outputs with the turn on and off as dicts): computed once per size, never written to.  Steps, push, pull
    and min_contact are the translation case's; spin = curl = 1."""
    hand, faces, obj, _ = case(V, N)
    finite = lambda a: np.where(np.isfinite(a), a, np.float32(0.0)).astype(np.float32)
    pivot = finite(hand[:, 0])
    knuckle = finite(np.stack([hand[:, 1], hand[:, 2]], 1))
    vert_part = np.asarray([-1] + [i % 2 for i in range(V - 1)], np.int32)
    vert_w = np.asarray([0.0] + [1.0 if i % 2 == 0 else 0.5 for i in range(V - 1)], np.float32)
    rigid = lambda spin: dict(zip(RIGID, rigid_ref.grasp_refine_rigid(hand, faces, obj, pivot, STEPS, spin=spin, contact_threshold=THR)))
    fingers = lambda curl: dict(zip(FINGERS, fingers_ref.grasp_refine_fingers(hand, faces, obj, pivot, vert_part, vert_w, knuckle, STEPS, spin=1.0,
                                                                              curl=curl, max_curl=MAX_CURL, contact_threshold=THR)))
    with np.errstate(all="ignore"):
        want = {"rigid": rigid(1.0), "rigid_spin0": rigid(0.0), "fingers": fingers(1.0), "fingers_curl0": fingers(0.0)}
    for a in [pivot, vert_part, vert_w, knuckle] + [x for d in want.values() for x in d.values()]:
        a.setflags(write=False)
    return pivot, vert_part, vert_w, knuckle, want


@functools.lru_cache(maxsize=None)
def ttt_case(V, N):
    """(targets, the ttt reference's outputs on ``case(V, N)`` with every odd vertex a target): computed once per size, never written to."""
    hand, faces, obj, _ = case(V, N)
    targets = np.arange(1, V, 2)
    with np.errstate(all="ignore"):
        full = ttt_ref.grasp_ttt(hand, faces, obj, targets, contact_threshold=THR)
    want = {k: full[k] for k in TTT}
    for a in [targets] + list(want.values()):
        a.setflags(write=False)
    return targets, want


def assert_same_bits(got, want, names, what):
    """Every number bit for bit; a NaN is a NaN (its payload is nobody's contract)."""
    for k in names:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.dtype, w.dtype)
        if w.dtype != np.float32:
            assert np.array_equal(g, w), (what, k, g, w)
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (what, k, g, w)
        assert np.array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan]), (what, k, g, w)


def digest(want):
    """sha256 over the three references' outputs in their documented order, every NaN as the one quiet NaN."""
    h = hashlib.sha256()
    for part, names in (("scores", SCORES), ("refine", REFINE), ("wrench", WRENCH)):
        for k in names:
            a = np.array(want[part][k])
            if a.dtype == np.float32:
                a[np.isnan(a)] = np.float32(np.nan)
            h.update(np.ascontiguousarray(a).astype(a.dtype.newbyteorder("<")).tobytes())
    return h.hexdigest()


# the references on two of the sizes, as they stood when the kernels came to share grasp_scan.h: a reference cannot drift together
# with the kernels
PINNED = {
    (5, 257): dict(n_interior=[88, 0, 150], n_contact=[40, 0, 47], iter=[2, 0, 2],
                   sha256="dce96c68039614fbe8940f1f30b24f4fe51d0c6ba50b653289f3b4bab8b93297"),
    (7, 1025): dict(n_interior=[559, 0, 346], n_contact=[97, 0, 181], iter=[2, 0, 2],
                    sha256="ccdbdb3e3d9b0b3e58369adf12582d771462b8e8d8604ce8e20c70cd33fc9e60"),
}
# the iterates the two upper levels' references kept on those sizes, as they stood when the three kernels became one text
PINNED_LADDER = {
    (5, 257): dict(rigid=[2, 0, 1], fingers=[2, 0, 1]),
    (7, 1025): dict(rigid=[2, 0, 2], fingers=[2, 0, 2]),
}
# the ttt reference's counts on the same two sizes with the odd vertices as targets, as they stood when the header's walk was
# written
PINNED_TTT = {
    (5, 257): dict(n_contact=[40, 0, 47], n_interior=[88, 0, 150]),
    (7, 1025): dict(n_contact=[97, 0, 181], n_interior=[559, 0, 346]),
}


@pytest.mark.parametrize("V,N", sorted(PINNED))
def test_the_references_give_what_they_gave(V, N):
    hand, faces, obj, want = case(V, N)
    assert len(faces) == {3: 1, 5: 3, 7: 6}[V] and np.isnan(hand[1]).sum() == 1 and np.isinf(obj[2]).sum() == 1
    assert np.isfinite(hand[[0, 2]]).all() and np.isfinite(obj[:2]).all()
    got = dict(n_interior=want["scores"]["n_interior"].tolist(), n_contact=want["scores"]["n_contact"].tolist(),
               iter=want["refine"]["iter"].tolist(), sha256=digest(want))
    assert got == PINNED[(V, N)]
    # what the kernels owe each other holds between the references too
    zero = dict(zip(REFINE, refine_ref.grasp_refine(hand, faces, obj, 0, contact_threshold=THR)))
    assert_same_bits(zero, want["scores"], SCORES, "reference: steps = 0")
    assert_same_bits(want["wrench"], want["scores"], SCORES, "reference: the wrench's scores")
    assert np.isnan(want["scores"]["penetration"][1]) and not np.isnan(want["scores"]["penetration"][0])


@pytest.mark.parametrize("V,N", SIZES)
def test_the_upper_levels_references_reduce_to_the_level_below(V, N):
    hand, faces, obj, want = case(V, N)
    pivot, vert_part, vert_w, knuckle, up = ladder(V, N)
    assert np.isfinite(pivot).all() and np.isfinite(knuckle).all()
    assert_same_bits(up["rigid_spin0"], want["refine"], REFINE, "reference: rigid at spin = 0 against the translation")
    assert np.array_equal(up["rigid_spin0"]["quat"], np.tile(IDENTITY, (3, 1)))
    assert_same_bits(up["fingers_curl0"], up["rigid"], RIGID, "reference: fingers at curl = 0 against rigid")
    assert np.array_equal(up["fingers_curl0"]["finger_quat"], np.tile(IDENTITY, (3, N_FINGERS, 1)))
    # the inputs exercise what they are for: the finite row turns, and one of its fingers curls (at V = 3 the knuckles are the
    # fingers' only vertices: no arm, no curl)
    if N >= 257:
        assert not np.array_equal(up["rigid"]["quat"][0], IDENTITY), up["rigid"]["quat"][0]
    curled = (up["fingers"]["finger_quat"][0] != IDENTITY).any(axis=1)
    if V == 3:
        assert not curled.any(), up["fingers"]["finger_quat"][0]
    elif N >= 257:
        assert curled.any(), up["fingers"]["finger_quat"][0]
    if (V, N) in PINNED_LADDER:
        assert dict(rigid=up["rigid"]["iter"].tolist(), fingers=up["fingers"]["iter"].tolist()) == PINNED_LADDER[(V, N)]


def assert_the_ttt_case_is_what_it_is_for(V, N):
    """The ttt reference's scores are the score reference's, rows 1 and 2 have no contact sum and no gradient, and from N = 257 up
    the finite row has contact and interior points and a gradient to gather."""
    _, _, _, want = case(V, N)
    _, ttt = ttt_case(V, N)
    assert_same_bits(ttt, want["scores"], SCORES, "reference: the ttt's scores")
    assert np.isnan(ttt["contact_sum"][1:]).all() and np.isnan(ttt["grad"][1:]).all()
    assert np.isfinite(ttt["contact_sum"][0]) and np.isfinite(ttt["grad"][0]).all()
    if N >= 257:
        assert ttt["n_contact"][0] > 0 and ttt["n_interior"][0] > 0 and ttt["grad"][0].any()


@pytest.mark.parametrize("V,N", SIZES)
def test_the_ttt_reference_on_the_seam_sizes(V, N):
    targets, ttt = ttt_case(V, N)
    assert targets.tolist() == {3: [1], 5: [1, 3], 7: [1, 3, 5]}[V]       # V = 5: the tail vertex 4 is none; V = 7: of the tail 4, 5, 6 one is
    assert_the_ttt_case_is_what_it_is_for(V, N)
    if (V, N) in PINNED_TTT:
        assert dict(n_contact=ttt["n_contact"].tolist(), n_interior=ttt["n_interior"].tolist()) == PINNED_TTT[(V, N)]


def gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)                          # (a copy: the cached arrays are read-only)


@pytest.mark.gpu
@pytest.mark.parametrize("V,N", SIZES)
def test_the_three_kernels_agree_with_their_references_and_each_other(V, N):
    hand, faces, obj, want = case(V, N)
    topo = contact.HandTopology(faces, V, DEV)
    args = (gpu(hand), topo.faces, topo.vf_off, topo.vf_face, gpu(obj))
    host = lambda names, out: dict(zip(names, (x.cpu().numpy() for x in out)))
    scores = host(SCORES, ops.grasp_scores(*args, contact_threshold=THR))
    zero = host(REFINE, ops.grasp_refine(*args, steps=0, contact_threshold=THR))
    refined = host(REFINE, ops.grasp_refine(*args, steps=STEPS, contact_threshold=THR))
    wrench = host(WRENCH, ops.grasp_wrench(*args, inv_length=INV_LENGTH, contact_threshold=THR))
    assert_same_bits(scores, want["scores"], SCORES, "grasp_scores")
    assert_same_bits(zero, scores, SCORES, "grasp_refine(steps=0) against grasp_scores")
    assert not zero["offset"].any() and not zero["iter"].any()
    assert_same_bits(wrench, scores, SCORES, "grasp_wrench's scores against grasp_scores")
    assert_same_bits(refined, want["refine"], REFINE, "grasp_refine")
    assert_same_bits(wrench, want["wrench"], WRENCH, "grasp_wrench")


@pytest.mark.gpu
@pytest.mark.parametrize("V,N", SIZES)
def test_the_upper_levels_agree_with_their_references_and_the_level_below(V, N):
    hand, faces, obj, _ = case(V, N)
    pivot, vert_part, vert_w, knuckle, want = ladder(V, N)
    topo = contact.HandTopology(faces, V, DEV)
    mesh, cloud, piv = (gpu(hand), topo.faces, topo.vf_off, topo.vf_face), gpu(obj), gpu(pivot)
    host = lambda names, out: dict(zip(names, (x.cpu().numpy() for x in out)))
    rigid = lambda spin: host(RIGID, ops.grasp_refine_rigid(*mesh, cloud, piv, steps=STEPS, spin=spin, contact_threshold=THR))
    fingers = lambda curl: host(FINGERS, ops.grasp_refine_fingers(*mesh, gpu(vert_part), gpu(vert_w), N_FINGERS, cloud, piv, gpu(knuckle),
                                                                  steps=STEPS, spin=1.0, curl=curl, max_curl=MAX_CURL,
                                                                  contact_threshold=THR))
    turned, curled = rigid(1.0), fingers(1.0)
    assert_same_bits(turned, want["rigid"], RIGID, "grasp_refine_rigid")
    assert_same_bits(curled, want["fingers"], FINGERS, "grasp_refine_fingers")
    shifted = host(REFINE, ops.grasp_refine(*mesh, cloud, steps=STEPS, contact_threshold=THR))
    assert_same_bits(rigid(0.0), shifted, REFINE, "grasp_refine_rigid(spin=0) against grasp_refine")
    assert_same_bits(fingers(0.0), turned, RIGID, "grasp_refine_fingers(curl=0) against grasp_refine_rigid")
    scores = host(SCORES, ops.grasp_scores(*mesh, cloud, contact_threshold=THR))
    assert_same_bits({k: curled[k + "0"] for k in SCORES}, scores, SCORES, "grasp_refine_fingers' iterate 0 against grasp_scores")


@pytest.mark.gpu
@pytest.mark.parametrize("V,N", SIZES)
def test_the_ttt_kernel_agrees_with_its_reference_and_with_grasp_scores(V, N):
    hand, faces, obj, _ = case(V, N)
    targets, want = ttt_case(V, N)
    assert_the_ttt_case_is_what_it_is_for(V, N)
    topo = contact.HandTopology(faces, V, DEV)
    args = (gpu(hand), topo.faces, topo.vf_off, topo.vf_face, gpu(obj))
    host = lambda names, out: dict(zip(names, (x.cpu().numpy() for x in out)))
    flags = contact.ContactTargets(targets, n_verts=V).on(DEV)
    got = host(TTT, ops.grasp_ttt(*args, flags, want_grad=True, contact_threshold=THR))
    scores = host(SCORES, ops.grasp_scores(*args, contact_threshold=THR))
    assert_same_bits(got, want, TTT, "grasp_ttt")
    assert_same_bits(got, scores, SCORES, "grasp_ttt's scores against grasp_scores")
    assert np.isnan(got["contact_sum"][1:]).all() and np.isnan(got["grad"][1:]).all()
