"""Translation push-out of generated grasps: the fused kernel (dvq_grasp_refine), its host API (ops.grasp_refine,
contact.refine_translation) and the ``refine_steps`` mode of generate_for_objects / the entry points.  The reference is
tests/grasp_refine_ref.py (numpy over oracle/contact_oracle.py and grasp_score_ref.tree_sum, all fp32); all five GPU outputs are
compared with it bit for bit.  Nothing here says anything about real grasps: no real checkpoint exists in the tree."""
import json
import lzma
import os
import re

import numpy as np
import pytest
import torch

import dvqvae_amd  # noqa: F401
from dvqvae_amd import _lib, contact, generate, ops, synth

import grasp_refine_ref as rref
import grasp_score_ref as ref

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
THR = 0.02 ** 2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def mano_pkl(tmp_path):
    """tests/golden/g9_mano_right.pkl.xz unpacked: the path of a MANO_RIGHT.pkl (real topology: 778 vertices, 1538 faces)."""
    path = str(tmp_path / "MANO_RIGHT.pkl")
    if not os.path.exists(path):
        with open(os.path.join(HERE, "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
    return path


# ------------------------------------------------------------------------------------------------------ CPU: parser, ABI, ops
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_has_the_refinement_flags(dataset):
    a = generate.parse_args(dataset, [])
    assert (a.refine_steps, a.refine_push, a.refine_pull) == (0, 1.0, 0.25)
    a = generate.parse_args(dataset, ["--refine_steps", "6", "--refine_push", "0.5", "--refine_pull", "0"])
    assert (a.refine_steps, a.refine_push, a.refine_pull) == (6, 0.5, 0.0)
    for bad in (["--refine_steps", "-1"], ["--refine_steps", "65"], ["--refine_push", "-0.1"], ["--refine_pull", "nan"]):
        with pytest.raises(SystemExit):
            generate.parse_args(dataset, bad)


def test_abi_declares_and_exports_the_entry_point():
    header = open(_lib.HEADER).read()
    assert re.search(r"^#define DVQ_ABI_VERSION 10$", header, re.M) and _lib.ABI_VERSION == 10
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert "dvq_grasp_refine" in _lib.SIGNATURES and len(_lib.SIGNATURES["dvq_grasp_refine"][1]) == 22
    assert "int dvq_grasp_refine(" in header and hasattr(lib, "dvq_grasp_refine")
    added = re.search(r"Entry points added since 10.*?\*/", header, re.S).group(0)
    assert "dvq_grasp_refine" in added


def test_ops_refuse_bad_arguments_before_any_device_use():
    v, f = ref.sphere_mesh(4, 6)
    faces, off, vf = (torch.from_numpy(a) for a in contact.face_csr(f, len(v)))
    hand = torch.from_numpy(v)[None].contiguous()
    good = dict(hand=hand, faces=faces, vf_off=off, vf_face=vf, obj=torch.zeros(1, 5, 3), steps=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_refine(**good)                                                     # well-formed, but not on a device
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grasp_refine(**{**good, "steps": 0, "push": 0.0, "pull": 0.0})
    for bad in (dict(hand=torch.zeros(1, 2049, 3), vf_off=torch.zeros(2050, dtype=torch.int32)), dict(steps=-1), dict(steps=65),
                dict(push=-1.0), dict(pull=-0.5), dict(push=float("inf")), dict(pull=float("nan")), dict(hand=hand.double()),
                dict(obj=torch.zeros(2, 5, 3)), dict(obj=torch.zeros(1, 0, 3)), dict(faces=faces.long()), dict(vf_off=off[:-1])):
        with pytest.raises(RuntimeError) as e:
            ops.grasp_refine(**{**good, **bad})
        assert "no CPU fallback" not in str(e.value), f"{list(bad)}: refused only for the device, not for the argument"


def test_generate_for_objects_refuses_bad_refinement_arguments():
    for kw in (dict(refine_steps=-1), dict(refine_steps=65), dict(refine_steps=2, refine_push=-1.0)):
        with pytest.raises(RuntimeError, match="refine"):
            generate.generate_for_objects(None, [torch.zeros(4, 8)], 5, True, 0, [0], **kw)


# ------------------------------------------------------------------------------------------------------ CPU: the reference itself
def test_reference_pushes_the_sphere_hand_out_of_the_sphere_cloud():
    v, f = ref.sphere_mesh()
    obj = rref.sphere_cloud()                                           # radius 0.04 at (0.07, 0.01, 0) against the hand's 0.05 at 0
    traces = []
    off, it, pen, n_in, n_ct = rref.grasp_refine(v[None], f, obj[None], 10, traces=traces)
    trace = traces[0]
    pen0 = trace[0][2]
    print("iterates (cls, pen, n_in, n_ct):", [x[1:] for x in trace], "kept", int(it[0]), "offset", off[0])
    assert bits(pen0) == bits(ref.grasp_scores(v[None], f, obj[None])[0][0])
    assert (0, float(pen[0])) <= (trace[0][1], float(pen0))             # the kept key is never worse than iterate 0's
    assert float(pen[0]) * 10 <= float(pen0), (pen, pen0)               # at least 10x less penetration
    assert n_ct[0] >= 1 and n_in[0] < trace[0][3] and it[0] > 0
    kept = trace[int(it[0])]
    assert np.array_equal(bits(kept[0]), bits(off[0])) and (kept[3], kept[4]) == (n_in[0], n_ct[0])
    assert all((x[1], float(x[2])) >= (kept[1], float(kept[2])) for x in trace)          # ... nor than any other iterate's
    assert all((x[1], float(x[2])) > (kept[1], float(kept[2])) for x in trace[:int(it[0])])   # the earliest among equals
    for steps in (1, 3, 6):                                             # every kept key <= the iterate-0 key, whatever the count
        o, i, p, a, c = rref.grasp_refine(v[None], f, obj[None], steps)
        assert float(p[0]) <= float(pen0) and c[0] >= 1 and i[0] <= steps


def test_reference_leaves_a_hand_out_of_reach_alone():
    v, f = ref.sphere_mesh()
    obj = rref.sphere_cloud(centre=(0.05 + 0.12 + 0.04, 0.0, 0.0))     # the nearest point 0.12 from the hand: no contact
    off, it, pen, n_in, n_ct = rref.grasp_refine(v[None], f, obj[None], 10)
    assert bits(off).tolist() == [[0, 0, 0]] and it[0] == 0 and bits(pen)[0] == 0 and n_in[0] == 0 and n_ct[0] == 0


def test_reference_with_no_steps_is_the_score_reference():
    v, f = ref.sphere_mesh()
    hand = np.stack([v, 0.9 * v]).astype(np.float32)
    obj = np.stack([rref.sphere_cloud(300), rref.sphere_cloud(300, centre=(0.0, 0.06, 0.01))])
    obj[1, 7, 1] = np.nan
    off, it, pen, n_in, n_ct = rref.grasp_refine(hand, f, obj, 0)
    want = ref.grasp_scores(hand, f, obj)
    assert np.isnan(pen[1]) and np.isnan(want[0][1]) and bits(pen)[0] == bits(want[0])[0]
    assert np.array_equal(n_in, want[1]) and np.array_equal(n_ct, want[2])
    assert not bits(off).any() and not it.any()


# ------------------------------------------------------------------------------------------------------ GPU: the fused kernel
def gpu(a):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def mano_faces(tmp_path):
    from dvqvae_amd import mano as dmano
    arrays = dmano.read_mano_pkl(mano_pkl(tmp_path))
    return arrays["faces"], np.asarray(arrays["v_template"], np.float32)


def five_situations():
    """The 5x257x776 case: sphere hands against a moderate overlap, a deep one, a cloud that touches without penetrating, one out of
    reach and a row with a NaN coordinate."""
    v, f = ref.sphere_mesh()
    B, N = 5, 257
    scale = np.linspace(0.9, 1.1, B).astype(np.float32)[:, None, None]
    hand = (v[None] * scale + synth.synthetic_normal((B, len(v), 3), 41, "refine/five/h", 0.0005).numpy()).astype(np.float32)
    obj = np.stack([rref.sphere_cloud(N, 0.04, (0.07, 0.01, 0.0)),      # moderate: the prototype's placement
                    rref.sphere_cloud(N, 0.02, (0.015, 0.0, 0.005)),    # deep: the whole cloud inside the hand
                    rref.sphere_cloud(N, 0.04, (0.0, 0.0, 0.1)),        # touching: 5 mm outside the hand's pole
                    rref.sphere_cloud(N, 0.04, (0.3, 0.0, 0.0)),        # out of reach
                    rref.sphere_cloud(N, 0.04, (0.0, 0.08, 0.01))])     # an overlap ...
    obj[4, 100, 2] = np.nan                                             # ... with a NaN coordinate
    return hand, f, obj.astype(np.float32)


def refine_case(name, tmp_path):
    """(hand [B,V,3], faces, obj [B,N,3]) numpy fp32; the hands as tests/test_grasp_select.py's score_case builds them."""
    rng = lambda tag, shape, scale: synth.synthetic_normal(shape, 31, f"scores/{name}/{tag}", scale).numpy()
    if name == "1x1x1":
        return rng("h", (1, 1, 3), 0.1), np.zeros((1, 3), np.int64), rng("o", (1, 1, 3), 0.1)      # one vertex, one degenerate face
    if name == "3x300x776":
        B, N = 3, 300
        v, f = ref.sphere_mesh()
        scale = np.linspace(0.8, 1.2, B).astype(np.float32)[:, None, None]
        hand = (v[None] * scale + rng("h", (B, len(v), 3), 0.002)).astype(np.float32)
        return hand, f, rng("o", (B, N, 3), 0.04)                                                    # points on both sides of the surface
    if name == "5x257x776":
        return five_situations()
    f, v = mano_faces(tmp_path)
    if name == "2x1024x778":
        return rng("h", (2, 778, 3), 0.05), f, rng("o", (2, 1024, 3), 0.05)                          # arbitrary vertices on the MANO topology
    assert name == "2x3000x778"
    hand = (v[None] + rng("h", (2, 778, 3), 0.001)).astype(np.float32)                               # the MANO template itself
    centre = v.mean(0, keepdims=True)[None]
    return hand, f, (centre + rng("o", (2, 3000, 3), 0.03)).astype(np.float32)


NAMES = ("offset", "iter", "penetration", "n_interior", "n_contact")


def run_refine(hand, faces, obj_dev, steps, **kw):
    topo = contact.HandTopology(faces, hand.shape[1], DEV)
    out = contact.refine_translation(topo, gpu(hand), obj_dev, steps, **kw)
    assert set(out) == set(NAMES)
    assert out["offset"].dtype == torch.float32 and tuple(out["offset"].shape) == (hand.shape[0], 3)
    assert out["penetration"].dtype == torch.float32 and all(out[k].dtype == torch.int32 for k in ("iter", "n_interior", "n_contact"))
    return topo, {k: v.cpu().numpy() for k, v in out.items()}


def assert_equal_bits(got, want, tag=""):
    """All five outputs bit for bit (a NaN is a NaN: its payload is nobody's contract)."""
    want = dict(zip(NAMES, want))
    print(tag, {k: got[k].tolist() for k in NAMES}, "reference", {k: want[k].tolist() for k in NAMES})
    for k in ("iter", "n_interior", "n_contact"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    nan = np.isnan(want["penetration"])
    assert np.array_equal(np.isnan(got["penetration"]), nan), tag
    assert np.array_equal(bits(got["penetration"])[~nan], bits(want["penetration"])[~nan]), (tag, got["penetration"], want["penetration"])
    assert np.array_equal(bits(got["offset"]), bits(want["offset"])), (tag, got["offset"], want["offset"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,steps", [("1x1x1", 3), ("3x300x776", 0), ("3x300x776", 1), ("3x300x776", 6), ("5x257x776", 5),
                                        ("2x1024x778", 4), ("2x3000x778", 2)])
def test_grasp_refine_equals_the_reference_bit_for_bit(name, steps, tmp_path):
    hand, faces, obj = refine_case(name, tmp_path)
    _, got = run_refine(hand, faces, gpu(obj), steps)
    want = rref.grasp_refine(hand, faces, obj, steps)
    assert_equal_bits(got, want, f"{name} steps {steps}")
    if steps == 0:
        assert not got["iter"].any() and not bits(got["offset"]).any()
    if name == "5x257x776":
        off, it, pen, n_in, n_ct = want
        assert (it > 0).any() and (it == 0).any()
        assert it[0] > 0 and n_in[0] > 0                                 # the moderate overlap moves
        assert it[3] == 0 and n_ct[3] == 0 and not bits(off[3]).any()    # out of reach: untouched
        assert np.isnan(pen[4]) and it[4] == 0 and not bits(off[4]).any()   # the NaN row: offset 0, iterate 0, NaN penetration
        pen0, n_in0, n_ct0 = ref.grasp_scores(hand, faces, obj)
        assert n_in0[1] == obj.shape[1] and it[1] > 0 and n_in[1] < n_in0[1]   # the deep one starts all interior and moves
        assert n_in0[2] == 0 and n_ct0[2] > 0 and it[2] == 0 and not bits(off[2]).any()   # touching: nothing to improve, the earliest kept
        assert all(np.isnan(pen0[b]) or pen[b] <= pen0[b] for b in range(5))


@pytest.mark.gpu
def test_grasp_refine_of_a_row_does_not_depend_on_the_batch():
    hand, faces, obj = five_situations()
    topo = contact.HandTopology(faces, hand.shape[1], DEV)
    pick = torch.arange(300, device=DEV) % 5
    big = contact.refine_translation(topo, gpu(hand)[pick].contiguous(), gpu(obj)[pick].contiguous(), 5)
    for b in range(5):
        one = contact.refine_translation(topo, gpu(hand[b:b + 1]), gpu(obj[b:b + 1]), 5)
        for k in NAMES:
            rows = big[k][pick == b].cpu().numpy()
            alone = one[k].cpu().numpy()
            assert np.array_equal(rows.view(np.uint32), np.repeat(alone, rows.shape[0], axis=0).view(np.uint32)), (k, b)
    assert (big["iter"] > 0).any() and (big["iter"] == 0).any()
    empty = contact.refine_translation(topo, gpu(hand)[:0].contiguous(), gpu(obj)[:0].contiguous(), 5)
    assert tuple(empty["offset"].shape) == (0, 3) and all(empty[k].shape == (0,) for k in NAMES[1:])


@pytest.mark.gpu
def test_grasp_refine_reads_a_channel_first_view_in_place():
    v, f = ref.sphere_mesh()
    B, N = 3, 500
    cloud = synth.synthetic_normal((B, 4, N), 32, "refine/cf", 0.02)                    # [B,4,N] as the generation path holds it
    cloud[:, 0] += 0.06                                                                  # across the hand's surface on the +x side
    hand = (v[None] * np.asarray([1.0, 0.9, 1.1], np.float32)[:, None, None]).astype(np.float32)
    view = gpu(cloud)[:, :3].transpose(1, 2)                                             # strides (4N, 1, N)
    assert not view.is_contiguous()
    _, got = run_refine(hand, f, view, 4)
    obj = cloud[:, :3].transpose(1, 2).contiguous().numpy()
    _, copy = run_refine(hand, f, gpu(obj), 4)
    for k in NAMES:
        assert np.array_equal(got[k].view(np.uint32), copy[k].view(np.uint32)), k
    assert_equal_bits(got, rref.grasp_refine(hand, f, obj, 4), "channel-first")
    assert (got["iter"] > 0).any()


@pytest.mark.gpu
def test_grasp_refine_with_no_steps_gives_the_bits_of_grasp_scores(tmp_path):
    for name in ("5x257x776", "2x1024x778"):
        hand, faces, obj = refine_case(name, tmp_path)
        topo, got = run_refine(hand, faces, gpu(obj), 0)
        pen, n_in, n_ct = ops.grasp_scores(gpu(hand), topo.faces, topo.vf_off, topo.vf_face, gpu(obj), THR)
        nan = np.isnan(got["penetration"])
        assert np.array_equal(nan, torch.isnan(pen).cpu().numpy())
        assert np.array_equal(bits(got["penetration"])[~nan], bits(pen.cpu().numpy())[~nan])
        assert np.array_equal(got["n_interior"], n_in.cpu().numpy()) and np.array_equal(got["n_contact"], n_ct.cpu().numpy())
        assert not got["iter"].any() and not bits(got["offset"]).any()


@pytest.mark.gpu
def test_grasp_refine_refuses_what_the_kernel_cannot_hold():
    v, f = ref.sphere_mesh(4, 6)
    topo = contact.HandTopology(f, len(v), DEV)
    hand = gpu(v)[None].contiguous()
    with pytest.raises(RuntimeError):
        contact.refine_translation(topo, hand, torch.zeros(1, 0, 3, device=DEV), 2)
    with pytest.raises(RuntimeError):
        contact.refine_translation(topo, hand, torch.zeros(1, 4, 3, device=DEV), 65)
    lib = _lib.load()                                                   # straight through the C ABI: DVQ_EINVAL, nothing launched
    one = torch.zeros(8, device=DEV)
    ok = dict(V=5, N=4, B=1, steps=2, push=1.0, pull=0.25)
    for bad in (dict(V=2049), dict(V=0), dict(N=0), dict(B=-1), dict(steps=-1), dict(steps=65), dict(push=-1.0), dict(pull=float("inf")),
                dict(push=float("nan"))):
        a = {**ok, **bad}
        rc = lib.dvq_grasp_refine(one.data_ptr(), topo.faces.data_ptr(), topo.vf_off.data_ptr(), topo.vf_face.data_ptr(), a["V"],
                                  one.data_ptr(), 0, 3, 1, a["B"], a["N"], 0.0004, a["steps"], a["push"], a["pull"], 1, one.data_ptr(),
                                  one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), None)
        assert rc == 1, bad
    rc = lib.dvq_grasp_refine(one.data_ptr(), topo.faces.data_ptr(), topo.vf_off.data_ptr(), topo.vf_face.data_ptr(), 5, one.data_ptr(), 0, 3, 1,
                              1, 4, 0.0004, 2, 1.0, 0.25, 1, None, one.data_ptr(), one.data_ptr(), one.data_ptr(), one.data_ptr(), None)
    assert rc == 1, "null pointer"


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


E2E_SEED, E2E_M, E2E_K, E2E_STEPS = 9, 8, 4, 3
E2E_INDICES = [5, 2]


def e2e_objects():
    """Two clouds of 256 points in 20 cm cubes around the place the synthetic weights put every hand (tests/test_grasp_select.py's
    e2e_objects(at_the_hand=True)), for calls without rotation."""
    centre = np.asarray([-0.08, -0.09, 0.13])
    return [generate.object_tensor(synth.synthetic_uniform((256, 3), 70 + i, "select/e2e", -0.1, 0.1).numpy().astype(np.float64) + centre)
            for i in range(2)]


def _pose(net, params):
    return net.rh_mano(betas=params[:, :10], global_orient=params[:, 10:13], hand_pose=params[:, 13:58], transl=params[:, 58:61]).vertices


@pytest.mark.gpu
def test_refined_best_of_m_end_to_end(tmp_path):
    net = _gennet(tmp_path)
    objs, M, k = e2e_objects(), E2E_M, E2E_K
    plain = generate.generate_for_objects(net, objs, M, False, E2E_SEED, E2E_INDICES)            # the parent's code path: all M rows
    faces = np.asarray(net.rh_mano.faces)
    first, moved = None, False
    for rows_per_call in (16384, 8):
        got = generate.generate_for_objects(net, objs, k, False, E2E_SEED, E2E_INDICES, rows_per_call=rows_per_call, candidates=M,
                                            refine_steps=E2E_STEPS)
        for i, (g, p) in enumerate(zip(got, plain)):
            cand, j = g["candidate"], g["json"]
            assert tuple(g["params"].shape) == (k, 61) and tuple(g["refine_offset"].shape) == (k, 3) and tuple(g["refine_iter"].shape) == (k,)
            assert g["refine_offset"].dtype == torch.float32 and g["refine_iter"].dtype == torch.int32
            assert torch.equal(g["params"][:, :58], p["params"][cand][:, :58]), f"object {i}: parameters 0 .. 57 changed"
            assert torch.equal(g["params"][:, 58:61], p["params"][cand][:, 58:61] + g["refine_offset"]), f"object {i}: translation"
            verts = _pose(net, g["params"].contiguous())
            assert torch.equal(verts, g["vertices"]), f"object {i}: the vertices are not those of the parameters written"
            written = np.asarray(j["recon_params"], np.float32)[:, 0]
            assert np.array_equal(bits(written), bits(g["params"].cpu().numpy()))
            assert np.array_equal(bits(np.asarray(j["refine_offset"], np.float32)), bits(g["refine_offset"].cpu().numpy()))
            assert j["refine_iter"] == g["refine_iter"].cpu().numpy().tolist() and all(0 <= x <= E2E_STEPS for x in j["refine_iter"])
            R = np.asarray(j["R_list"], np.float64)                                      # [k,3,4]: rotation | translation
            cloud = ops.transform_cloud(gpu(objs[i]).contiguous(), gpu(R[:, :, :3].astype(np.float32)).contiguous(),
                                        gpu(R[0, :, 3].astype(np.float32)).contiguous())
            pen, n_in, n_ct = ref.grasp_scores(verts.cpu().numpy(), faces, cloud[:, :3].transpose(1, 2).cpu().numpy())
            print(f"rows_per_call {rows_per_call} object {i}: kept {cand.tolist()} iter {j['refine_iter']} pen {j['penetration']} "
                  f"n_interior {j['n_interior']} n_contact {j['n_contact']}")
            assert np.array_equal(bits(np.asarray(j["penetration"], np.float32)), bits(pen)), f"object {i}: JSON penetration"
            assert j["n_interior"] == n_in.tolist() and j["n_contact"] == n_ct.tolist()
            assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact",
                              "refine_offset", "refine_iter"}
            moved |= any(x > 0 for x in j["refine_iter"])
        dumped = [json.dumps(g["json"]) for g in got]
        if first is None:
            first = dumped
        assert dumped == first, f"rows_per_call {rows_per_call}: the JSON differs from the 16384-row call's"
    assert moved, "no grasp was moved: the refinement is not exercised"


@pytest.mark.gpu
def test_refinement_without_candidates_reports_the_scores_of_the_written_hands(tmp_path):
    net = _gennet(tmp_path)
    objs, G = e2e_objects(), 6
    plain = generate.generate_for_objects(net, objs, G, False, E2E_SEED, E2E_INDICES)
    got = generate.generate_for_objects(net, objs, G, False, E2E_SEED, E2E_INDICES, refine_steps=E2E_STEPS)
    topo = contact.HandTopology(np.asarray(net.rh_mano.faces), 778, DEV)
    for i, (g, p) in enumerate(zip(got, plain)):
        j = g["json"]
        assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "refine_offset", "refine_iter", "penetration", "n_interior",
                          "n_contact"}
        assert torch.equal(g["params"][:, :58], p["params"][:, :58])
        assert torch.equal(g["params"][:, 58:61], p["params"][:, 58:61] + g["refine_offset"])
        assert torch.equal(_pose(net, g["params"].contiguous()), g["vertices"])
        R = np.asarray(j["R_list"], np.float64)
        cloud = ops.transform_cloud(gpu(objs[i]).contiguous(), gpu(R[:, :, :3].astype(np.float32)).contiguous(),
                                    gpu(R[0, :, 3].astype(np.float32)).contiguous())[:, :3].transpose(1, 2)
        want = contact.grasp_scores(topo, g["vertices"], cloud)
        for name in ("penetration", "n_interior", "n_contact"):
            assert torch.equal(g[name], want[name]) and j[name] == want[name].cpu().numpy().tolist(), name
        # the kernel's own iterates against the plain hands: the offsets are those of contact.refine_translation
        direct = contact.refine_translation(topo, p["vertices"], cloud, E2E_STEPS)
        assert torch.equal(direct["offset"], g["refine_offset"]) and torch.equal(direct["iter"], g["refine_iter"])


@pytest.mark.gpu
def test_refinement_needs_a_face_list():
    from dvqvae_amd import mano as dmano
    from dvqvae_amd.network.gen_net import GenNet
    from conftest import GOLDEN, gen_state_dict
    net = GenNet()
    net.load_state_dict(gen_state_dict(net.state_dict(), np.load(os.path.join(GOLDEN, "g7_gen.npz"))), strict=True)
    net.eval().to(DEV)
    net.set_rh_mano(dmano.ManoLayer(dmano.synthetic_mano_arrays()).to(DEV))
    with pytest.raises(RuntimeError, match="no face list"):
        generate.generate_for_objects(net, e2e_objects()[:1], 2, False, 1, [0], refine_steps=2)


def _run_main(dataset, out_dir, extra, mano="/nonexistent"):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent", "--mano_model", mano])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
def test_entry_point_files_with_and_without_refinement(tmp_path):
    mano = mano_pkl(tmp_path)
    base = ["--num_objects", "2", "--points", "256", "--num_grasp", "4"]
    names0, bytes0 = _run_main("ho3d", str(tmp_path / "plain"), base, mano)
    names, data = _run_main("ho3d", str(tmp_path / "zero"), base + ["--refine_steps", "0", "--refine_push", "2", "--refine_pull", "1"], mano)
    assert names == names0 and data == bytes0, "--refine_steps 0 must write the files of a run without the flag"
    assert set(json.loads(data[0])) == {"recon_params", "R_list", "trans_list", "r_list"}
    cand = ["--candidates", "8", "--refine_steps", "3"]
    names1, bytes1 = _run_main("ho3d", str(tmp_path / "refined"), base + cand, mano)
    names2, bytes2 = _run_main("ho3d", str(tmp_path / "refined8"), base + cand + ["--rows_per_call", "8"], mano)
    assert names1 == names0 and names2 == names0 and bytes1 == bytes2, "--rows_per_call 8: the files differ"
    j = json.loads(bytes1[0])
    assert set(j) == {"recon_params", "R_list", "trans_list", "r_list", "candidate", "penetration", "n_interior", "n_contact",
                      "refine_offset", "refine_iter"}
    assert all(len(j[f]) == 4 for f in j) and all(len(o) == 3 for o in j["refine_offset"])
    _, loop = _run_main("ho3d", str(tmp_path / "loop"), base + ["--refine_steps", "3", "--rows_per_call", "0"], mano)   # the grouped path
    assert set(json.loads(loop[0])) == {"recon_params", "R_list", "trans_list", "r_list", "refine_offset", "refine_iter", "penetration",
                                        "n_interior", "n_contact"}
