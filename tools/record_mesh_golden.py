#!/usr/bin/env python3
"""Record the reference's inside-the-mesh test (metric/contactutils.py: batch_mesh_contains_points) for tests/test_grasp_mesh.py by
RUNNING the reference on the CPU -- the function is pure torch; the reference source is not read, and nothing of its text is written
here.

    python tools/record_mesh_golden.py --reference /path/to/the/reference/checkout

Cases: the test module's torus (16 x 8 quads, 128 vertices, 256 faces, major radius 5 cm, minor 2 cm) against two posed hands of
the committed MANO model (778 vertices) placed through the tube and the point sets of seeds 0 and 1 (tests/test_grasp_mesh.py:
point_set).  Everything is rounded to fp32 first and handed to the reference as float64, so that the recorded masks belong to
exactly the coordinates the tests read.

Writes tests/golden/g11_mesh_contains.npz (data only: verts fp32 [128,3], faces int16 [256,3]; per case k = 0 .. 3: points{k} fp32
[778,3] and exterior{k} bool [778], the reference's answer).  Runs on the CPU only."""
import argparse
import importlib.util
import lzma
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def hands():
    """Two posed hands of the committed hand model, their centroids moved onto the tube's centre circle (float64 [778,3])."""
    import mano_ref
    from dvqvae_amd import mano as dmano
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "MANO_RIGHT.pkl")
        with open(os.path.join(ROOT, "tests", "golden", "g9_mano_right.pkl.xz"), "rb") as f, open(path, "wb") as out:
            out.write(lzma.decompress(f.read()))
        arrays = mano_ref.device_arrays(dmano.read_mano_pkl(path))
    rng = np.random.default_rng(20241020)
    for centre in ((0.05, 0.0, 0.0), (-0.03, -0.04, 0.004)):
        betas, pose, go = rng.normal(0, 1.0, (1, 10)), rng.normal(0, 0.5, (1, 45)), rng.normal(0, 1.0, (1, 3))
        hand = np.asarray(mano_ref.mano_ref(arrays, betas, pose, go, np.zeros((1, 3)))[0], np.float64)[0]
        yield hand - hand.mean(axis=0) + np.asarray(centre)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reference", required=True, help="a checkout of the reference (the directory that holds metric/contactutils.py)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "g11_mesh_contains.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_contactutils", os.path.join(os.path.abspath(args.reference), "metric", "contactutils.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)                            # the reference, as it is
    import test_grasp_mesh as tm
    import grasp_mesh_ref as mesh_ref
    verts, faces = tm.torus()
    verts = verts.astype(np.float32)
    tri = torch.from_numpy(verts.astype(np.float64)[faces])[None]            # [1,256,3,3]
    out = {"verts": verts, "faces": faces.astype(np.int16)}
    for k, pts in enumerate(list(hands()) + [tm.point_set(0), tm.point_set(1)]):
        pts = np.asarray(pts, np.float32)
        with torch.no_grad():
            ext = ref.batch_mesh_contains_points(torch.from_numpy(pts.astype(np.float64))[None], tri,
                                                 direction=torch.tensor([0.4395064455, 0.617598629942, 0.652231566745], dtype=torch.float64))
        ext = ext[0].numpy().astype(bool)
        wind = np.abs(mesh_ref.winding_number(pts, verts, faces)) > 0.5
        print(f"case {k}: {int((~ext).sum())} of {len(pts)} points inside by the reference, {int(((~ext) != wind).sum())} differ from the "
              "float64 winding number")
        out.update({f"points{k}": pts, f"exterior{k}": ext})
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
