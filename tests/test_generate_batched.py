"""Batched grasp generation across objects: a grasp is identified by (seed, object index, grasp index) and is the same bits
whether it is generated alone with its object (generate_for_object, one call per object) or inside a call that mixes many
objects (per-row noise keys, dvq_transform_clouds, GenNet.gen(row_keys=), generate_for_objects, --rows_per_call).
Every comparison is exact except the one against the numpy restatement of the generator (libm's log)."""
import os

import numpy as np
import pytest
import torch

from dvqvae_amd import _lib, generate

DEV = "cuda:0"


# ------------------------------------------------------------------------------------------ host logic (no GPU)
@pytest.mark.parametrize("num_grasp", [1, 20, 100])
@pytest.mark.parametrize("rows_per_call", [1, 7, 100, 16384])
def test_plan_calls_partitions_objects_by_point_count(num_grasp, rows_per_call):
    counts = [3000, 1024, 3000, 778, 1024, 3000, 3000, 1024, 3000, 3000, 778] * 3
    calls = generate.plan_calls(counts, num_grasp, rows_per_call)
    flat = [p for c in calls for p in c]
    assert sorted(flat) == list(range(len(counts))), "every object exactly once"
    cap = max(1, rows_per_call // num_grasp)
    for c in calls:
        assert len(c) >= 1 and len({counts[p] for p in c}) == 1, "a call has one point count"
        assert c == sorted(c), "the given order is kept inside a call"
        assert len(c) <= cap
    for n in set(counts):                                    # the order is kept inside a GROUP too: calls of one N run in object order
        group = [p for c in calls for p in c if counts[p] == n]
        assert group == sorted(group)
    # a group is cut into as few calls as the cap allows
    assert len(calls) == sum(-(-counts.count(n) // cap) for n in set(counts))


def test_plan_calls_edge_cases():
    assert generate.plan_calls([], 5, 100) == []
    assert generate.plan_calls([300], 100, 7) == [[0]]       # rows_per_call < num_grasp: one object per call, never a split object
    assert generate.plan_calls([5, 5, 5], 2, 4) == [[0, 1], [2]]
    assert generate.plan_calls([5, 6, 5, 6], 1, 16384) == [[0, 2], [1, 3]]


@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_parser_accepts_rows_per_call(dataset):
    p = generate.build_parser(dataset)
    assert p.parse_args([]).rows_per_call == 16384
    assert p.parse_args(["--rows_per_call", "0"]).rows_per_call == 0
    assert p.parse_args(["--rows_per_call", "7"]).rows_per_call == 7


def test_abi_10_declares_the_batched_entry_points():
    assert _lib.ABI_VERSION == 10
    assert "dvq_exp1_noise_keyed" in _lib.SIGNATURES and "dvq_transform_clouds" in _lib.SIGNATURES
    header = open(_lib.HEADER).read()
    assert "int dvq_exp1_noise_keyed(" in header and "int dvq_transform_clouds(" in header


# ------------------------------------------------------------------------------------------ GPU
def _gennet():
    """The synthetic net of tests/test_gpu_parity.py::_gennet."""
    from conftest import GOLDEN, gen_state_dict
    from dvqvae_amd import mano as dmano
    from dvqvae_amd.network.gen_net import GenNet
    net = GenNet()
    sd = gen_state_dict(net.state_dict(), np.load(os.path.join(GOLDEN, "g7_gen.npz")))
    net.load_state_dict(sd, strict=True)
    net.eval().to(DEV)
    net.set_rh_mano(dmano.ManoLayer(dmano.synthetic_mano_arrays()).to(DEV))
    return net


def _i64(values):
    return torch.tensor(list(values), dtype=torch.int64, device=DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [9 * 512, 270, 4])
def test_keyed_noise_equals_the_per_stream_generator(cols):
    from dvqvae_amd import ops
    from oracle import philox
    seed = (7 << 32) | 12345
    streams = [3, 0, (1 << 32) - 1, 3, 17, 0, 3, (1 << 32) - 1, 1 << 31, 5, 3]        # shuffled, repeated, up to 2^32 - 1
    rows = [5, 0, (1 << 32) + 9, 0, 1 << 40, 7, 5, 2, (1 << 33) + 1, (1 << 62) + 3, 99]  # repeats of a whole key too; beyond 2^32
    got = ops.exp1_noise_keyed(_i64(streams), _i64(rows), cols, seed)
    assert tuple(got.shape) == (len(streams), cols) and got.dtype == torch.float32
    out = torch.full((len(streams), cols), -1.0, device=DEV)
    assert ops.exp1_noise_keyed(_i64(streams), _i64(rows), cols, seed, out=out) is out and torch.equal(out, got)
    pad = (cols + 3) // 4 * 4
    for r, (s, row) in enumerate(zip(streams, rows)):
        want = ops.exp1_noise(1, cols, seed, row0=row, stream_id=s, device=DEV)
        assert torch.equal(got[r:r + 1], want), f"row {r}: key (stream {s}, row {row}) differs from dvq_exp1_noise"
        ref = philox.exp1_noise(1, pad, seed, row0=row, stream_id=s)[:, :cols]
        np.testing.assert_allclose(got[r:r + 1].cpu().numpy(), ref, rtol=2e-6, atol=1e-7)


@pytest.mark.gpu
def test_keyed_noise_rejects_keys_outside_the_counter():
    from dvqvae_amd import ops
    for streams, rows in (([1, 1 << 32, 2], [0, 0, 0]), ([1, 2, 3], [0, -1, 0]), ([-1], [0])):
        with pytest.raises(RuntimeError):
            ops.exp1_noise_keyed(_i64(streams), _i64(rows), 16, 1)
    err = ops.new_err_flag(torch.device(DEV))                 # with a caller's flag: no raise, bit 0, that row NaN and only that row
    q = ops.exp1_noise_keyed(_i64([1, 1 << 32, 2]), _i64([0, 0, 0]), 16, 1, err=err)
    assert int(err.item()) & 1
    assert bool(torch.isnan(q[1]).all()) and bool(torch.isfinite(q[[0, 2]]).all())
    with pytest.raises(RuntimeError):
        ops.exp1_noise_keyed(_i64([1, 2]).to(torch.int32), _i64([0, 0]), 16, 1)
    with pytest.raises(RuntimeError):
        ops.exp1_noise_keyed(_i64([1, 2]), _i64([0]), 16, 1)
    with pytest.raises(RuntimeError):
        ops.exp1_noise_keyed(_i64([1, 2]).cpu(), _i64([0, 0]).cpu(), 16, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [3000, 1024, 778, 301, 1])
@pytest.mark.parametrize("C", [3, 4])
def test_transform_clouds_equals_transform_cloud_per_row(C, N):
    from dvqvae_amd import ops
    g = torch.Generator().manual_seed(100 * C + N)
    O = 5
    pc = (torch.randn(O, C, N, generator=g) * 0.3).to(DEV)
    obj_of_row = [4, 0, 0, 2, 4, 1, 0, 4, 2, 2, 1, 0, 4]                              # unordered, repeats, object 3 unused
    B = len(obj_of_row)
    R = torch.from_numpy(generate.rotation_xyz(np.random.default_rng(N).random((B, 3)) * 2 * np.pi)).float().to(DEV)
    for t in (None, torch.tensor(generate.CANONICAL_OFFSET, dtype=torch.float32, device=DEV)):
        got = ops.transform_clouds(pc, _i64(obj_of_row), R, t)
        assert tuple(got.shape) == (B, C, N)
        for b, o in enumerate(obj_of_row):
            want = ops.transform_cloud(pc[o].contiguous(), R[b:b + 1].contiguous(), t)
            assert torch.equal(got[b:b + 1], want), f"row {b} (object {o}) differs from dvq_transform_cloud"
        # the per-row form of the old entry point (one cloud per row) agrees as well
        assert torch.equal(got, ops.transform_cloud(pc[_i64(obj_of_row)].contiguous(), R, t))


@pytest.mark.gpu
def test_transform_clouds_rejects_indices_outside_the_clouds():
    from dvqvae_amd import ops
    pc = torch.randn(5, 4, 64, device=DEV)
    R = torch.eye(3, device=DEV).repeat(3, 1, 1)
    for bad in (5, -1):
        with pytest.raises(RuntimeError):
            ops.transform_clouds(pc, _i64([0, bad, 1]), R, None)
    err = ops.new_err_flag(torch.device(DEV))
    got = ops.transform_clouds(pc, _i64([0, 5, 1]), R, None, err=err)
    assert int(err.item()) & 1 and torch.equal(got[0], pc[0] + 0.0) and torch.equal(got[2], pc[1] + 0.0)
    with pytest.raises(RuntimeError):
        ops.transform_clouds(pc, _i64([0, 1]), R, None)                                 # one index per row
    with pytest.raises(RuntimeError):
        ops.transform_clouds(pc[0], _i64([0, 0, 0]), R, None)                           # [O,C,N] only


@pytest.mark.gpu
@pytest.mark.parametrize("n_obj,n_grasp", [(8, 100), (3, 5)])
def test_gen_row_keys_equals_per_object_calls(n_obj, n_grasp):
    """800 rows take the label-sort path of gen (B >= 512), 15 rows the direct one; rows of different objects interleaved."""
    from dvqvae_amd import synth
    net = _gennet()
    seed, B = 41, n_obj * n_grasp
    clouds = synth.synthetic_clouds(B, 256, seed=77).to(DEV)                             # cloud o * n_grasp + g: grasp g of object o
    order = torch.from_numpy(np.random.default_rng(3).permutation(B)).to(DEV)            # the mixed call's row order
    sid, rid = (order // n_grasp).contiguous(), (order % n_grasp).contiguous()
    stream0 = net._noise_stream
    recon, pos, aux = net.gen(clouds[order].contiguous(), seed=seed, row_keys=(sid, rid), return_aux=True)
    assert net._noise_stream == stream0, "row_keys must not advance the per-call stream"
    labels = set()
    for o in range(n_obj):
        r_o, p_o, a_o = net.gen(clouds[o * n_grasp:(o + 1) * n_grasp].contiguous(), seed=seed, row0=0, stream_id=o, return_aux=True)
        rows = (sid == o).nonzero().reshape(-1)
        g = rid[rows]
        assert torch.equal(recon[rows], r_o[g]) and torch.equal(pos[rows], p_o[g]), f"object {o}: parameters differ"
        assert torch.equal(aux["codes"][rows], a_o["codes"][g]), f"object {o}: sampled codes differ"
        labels |= set(a_o["idx6"].reshape(-1).tolist())
    assert len(labels) >= 2, "the inputs must exercise the label sort"
    obj = clouds[order].contiguous()
    with pytest.raises(RuntimeError):
        net.gen(obj, row_keys=(sid, rid), noise=torch.ones(B, 9, 512, device=DEV))
    with pytest.raises(RuntimeError):
        net.gen(obj, row_keys=(sid, rid), row0=0)
    with pytest.raises(RuntimeError):
        net.gen(obj, row_keys=(sid, rid), stream_id=1)
    with pytest.raises(RuntimeError):
        net.gen(obj, row_keys=(sid[:-1].contiguous(), rid[:-1].contiguous()))


@pytest.mark.gpu
def test_gen_range_fallback_under_row_keys():
    """One row of a mixed-object call leaves fp16's range (as in test_gen_range_fallback_regenerates_only_the_rows_that_need_it):
    it is generated again under ITS key -- equal to what its object's own call gives -- and the other rows keep their bits."""
    from dvqvae_amd import synth
    net = _gennet()
    n_obj, n_grasp, bad, seed = 4, 10, 17, 5
    B = n_obj * n_grasp
    clean = synth.synthetic_clouds(B, 300, seed=91).to(DEV)
    scale = None
    for s_try in (1.0e3, 1.0e4, 1.0e5, 1.0e6):                                          # the smallest scale that leaves fp16's range
        with torch.no_grad():
            f_bad, _, _ = net.obj_encoder_type(clean[bad:bad + 1] * s_try)
        if float(f_bad.abs().max()) > 7.0e4:
            scale = s_try
            break
    assert scale is not None, "no scale pushed the PointNet feature (a decoder input) beyond fp16's range"
    obj = clean.clone()
    obj[bad] *= scale
    sid = (torch.arange(B, device=DEV) % n_obj).contiguous()                             # row b: object b % 4, grasp b // 4
    rid = (torch.arange(B, device=DEV) // n_obj).contiguous()
    n0, r0 = net.range_fallbacks, net.range_fallback_rows
    r, p, aux = net.gen(obj, seed=seed, row_keys=(sid, rid), return_aux=True)
    assert net.range_fallbacks == n0 + 1 and net.range_fallback_rows == r0 + 1 and aux["fallback_rows"].tolist() == [bad]
    assert bool(torch.isfinite(r).all()) and bool(torch.isfinite(p).all())
    rc, pc = net.gen(clean, seed=seed, row_keys=(sid, rid))
    assert net.range_fallbacks == n0 + 1
    keep = [i for i in range(B) if i != bad]
    assert torch.equal(r[keep], rc[keep]) and torch.equal(p[keep], pc[keep]), "rows inside the range must keep their bits"
    o, g = bad % n_obj, bad // n_obj
    ro, po = net.gen(obj[o::n_obj].contiguous(), seed=seed, row0=0, stream_id=o)         # the object's own call (its own fallback)
    assert torch.equal(r[bad], ro[g]) and torch.equal(p[bad], po[g]), "the regenerated row must be its object's own result"
    assert torch.equal(r[o::n_obj], ro) and torch.equal(p[o::n_obj], po)


@pytest.mark.gpu
@pytest.mark.parametrize("rotate", [True, False])
@pytest.mark.parametrize("num_grasp", [1, 7])
def test_generate_for_objects_equals_the_per_object_loop(rotate, num_grasp):
    from dvqvae_amd import synth
    net = _gennet()
    seed = 9
    objs = [synth.synthetic_clouds(1, n, seed=50 + i)[0] for i, n in enumerate((700, 300, 700))]
    indices = [5, 2, 11]
    want = [generate.generate_for_object(net, objs[i], num_grasp, rotate, np.random.default_rng([seed, indices[i]]), seed=seed,
                                         object_index=indices[i]) for i in range(3)]
    for rows_per_call in (16384, 10, 1):
        got = generate.generate_for_objects(net, objs, num_grasp, rotate, seed, indices, rows_per_call=rows_per_call)
        assert len(got) == 3
        for i in range(3):
            assert set(got[i]) == set(want[i])
            assert torch.equal(got[i]["params"], want[i]["params"]), f"rows_per_call {rows_per_call}, object {i}: params"
            assert torch.equal(got[i]["vertices"], want[i]["vertices"]), f"rows_per_call {rows_per_call}, object {i}: vertices"
            assert got[i]["json"] == want[i]["json"], f"rows_per_call {rows_per_call}, object {i}: json"


def _run_main(dataset, out_dir, extra):
    paths = generate.main(dataset, extra + ["--out_dir", out_dir, "--seed", "3", "--checkpoint", "/nonexistent",
                                            "--mano_model", "/nonexistent"])
    return [os.path.basename(p) for p in paths], [open(p, "rb").read() for p in paths]


@pytest.mark.gpu
@pytest.mark.parametrize("dataset", ["obman", "ho3d", "grab", "FHAB"])
def test_entry_points_write_the_same_bytes_for_every_grouping(tmp_path, dataset):
    base = ["--num_objects", "5", "--points", "256"]
    names0, bytes0 = _run_main(dataset, str(tmp_path / "loop"), base + ["--rows_per_call", "0"])
    assert names0 == [f"obj_id_synthetic_{i}.json" for i in range(5)]
    for tag, extra in (("default", []), ("seven", ["--rows_per_call", "7"])):
        names, data = _run_main(dataset, str(tmp_path / tag), base + extra)
        assert names == names0, f"{tag}: file names / order"
        assert data == bytes0, f"{tag}: file bytes differ from the per-object loop"


@pytest.mark.gpu
def test_ho3d_entry_point_groups_object_files_of_two_point_counts(tmp_path):
    rng = np.random.default_rng(8)
    files = []
    for i, n in enumerate((300, 256, 300, 256, 300)):
        path = str(tmp_path / f"cloud_{i}.npy")
        np.save(path, rng.uniform(-0.1, 0.1, size=(n, 3)))
        files.append(path)
    base = ["--num_grasp", "9", "--objects"] + files
    names0, bytes0 = _run_main("ho3d", str(tmp_path / "loop"), base + ["--rows_per_call", "0"])
    assert names0 == [f"obj_id_cloud_{i}.json" for i in range(5)]
    for tag, extra in (("default", []), ("seven", ["--rows_per_call", "7"]), ("twenty", ["--rows_per_call", "20"])):
        names, data = _run_main("ho3d", str(tmp_path / tag), base + extra)
        assert names == names0, f"{tag}: file names / order (grouping by point count must not reorder the list)"
        assert data == bytes0, f"{tag}: file bytes differ from the per-object loop"
