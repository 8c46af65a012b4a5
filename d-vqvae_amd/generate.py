"""Generation plumbing shared by the four ``gen_diverse_grasp_*`` entry points (reference:
gen_diverse_grasp_obman.py:194-365 and the ho3d/grab/FHAB variants): model build, checkpoint loading, per-object
random rotations, ONE batched ``GenNet.gen`` call for the grasps of MANY objects (the reference loops B=1 calls; every grasp
is keyed by (seed, object index, grasp index), so it does not depend on how objects are grouped into calls), 61-parameter
assembly, the final posed-MANO pass and the per-object JSON the downstream tools read.

Out of scope: the physics / mesh metrics (pybullet, igl, trimesh, V-HACD) and the dataset
readers for /data/ObMan, /data/GRAB_unzip, HO3D models -- objects come from ``--objects *.npy`` point clouds
([N,3], e.g. models/Object_models/*/…resampled.npy) or from the synthetic generator."""
from __future__ import annotations

import argparse
import dataclasses
import inspect
import json
import math
import os
import re
import time
import types
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import contact, dist, mano as dmano, ops, synth
from .network.gen_net import GenNet

CANONICAL_OFFSET = (-0.0793, 0.0208, -0.6924)       # gen_diverse_grasp_ho3d.py:221

DIVERSE_SPACES = ("params", "verts")                 # --diverse_space: squared distances over [61] or [778 * 3]
DIVERSITY_ITERS = 100                                # --diversity: the Lloyd iterations allowed (ops.segment_kmeans)

DATASETS = {                                         # grasps per object, random rotation per grasp
    "obman": dict(num_grasp=1, rotate=False),        # gen_diverse_grasp_obman.py:233
    "ho3d": dict(num_grasp=100, rotate=True),        # gen_diverse_grasp_ho3d.py:212
    "grab": dict(num_grasp=20, rotate=True),         # gen_diverse_grasp_grab.py:202
    "FHAB": dict(num_grasp=49, rotate=True),         # gen_diverse_grasp_FHAB.py:200
}


def build_parser(dataset: str) -> argparse.ArgumentParser:
    d = DATASETS[dataset]
    p = argparse.ArgumentParser(description=f"batched grasp generation ({dataset})")
    # the reference's ten flags (gen_diverse_grasp_obman.py:310-322); only use_cuda / num_grasp are ever read there
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--use_cuda", type=int, default=1)
    p.add_argument("--dataloader_workers", type=int, default=32)
    p.add_argument("--encoder_layer_sizes", type=list, default=[1024, 512, 256])
    p.add_argument("--decoder_layer_sizes", type=list, default=[1024, 256, 61])
    p.add_argument("--latent_size", type=int, default=64)
    p.add_argument("--obj_inchannel", type=int, default=4)
    p.add_argument("--condition_size", type=int, default=1024)
    p.add_argument("--num_grasp", type=int, default=d["num_grasp"])
    # additions
    p.add_argument("--objects", nargs="*", default=[], help="[N,3] point clouds (.npy); synthetic objects if omitted")
    p.add_argument("--num_objects", type=int, default=2, help="number of synthetic objects")
    p.add_argument("--points", type=int, default=3000)
    p.add_argument("--n_embeddings", type=int, default=128, help="codebook rows (128 = reference checkpoints)")
    p.add_argument("--checkpoint", default="./checkpoints/model_best.pth")
    p.add_argument("--prior_checkpoint", default="./checkpoints/LATENT_BLOCK_pixelcnn.pt")
    p.add_argument("--mano_model", default="./models/mano/MANO_RIGHT.pkl")
    p.add_argument("--out_dir", default=f"./diverse_grasp/{dataset}")
    p.add_argument("--device", default=None)
    p.add_argument("--rows_per_call", type=int, default=16384,
                   help="grasps per batched call: whole objects of one point count are grouped up to this many rows "
                        "(0 = one call per object); the files written do not depend on it")
    p.add_argument("--temperature", type=float, default=1.0,
                   help="divides the prior's logits before each draw: below 1 likelier and less diverse grasps, above 1 the opposite")
    p.add_argument("--top_k", type=int, default=0, help="draw every grid position from its top_k likeliest codes (0 = all)")
    p.add_argument("--log_prob", type=int, default=0,
                   help="1: every object's JSON gains \"log_prob\", each grasp's log-likelihood under the (untempered) prior")
    p.add_argument("--beam_width", type=int, default=0,
                   help="beam search instead of sampling: every pose of an object gets the beam_width likeliest distinct code grids of the "
                        "prior, in rank order, with no noise (0 = off); num_grasp (or --candidates) must equal beam_poses * beam_width; "
                        "the JSON gains \"log_prob\", \"beam_pose\", \"beam_rank\", \"beam_duplicate_of\"")
    p.add_argument("--beam_poses", type=int, default=1,
                   help="--beam_width: poses per object, drawn as the rotations of its first beam_poses grasps are drawn without the "
                        "flag; row p * beam_width + r is rank r of pose p (datasets that do not rotate take 1)")
    p.add_argument("--candidates", type=int, default=0,
                   help="best-of-M: generate this many candidates per object, score them on the device and keep the num_grasp best "
                        "(0 = off; otherwise >= num_grasp); the JSON gains \"candidate\", \"penetration\", \"n_interior\", \"n_contact\"")
    p.add_argument("--select_by", choices=["penetration", "log_prob", "stability"], default="penetration",
                   help="what ranks the candidates: least penetration among the hands that touch the object, the prior's log-likelihood, "
                        "or the contact-wrench stability proxy (smallest net wrench of unit contact forces; untuned, see --stability)")
    p.add_argument("--min_contact", type=int, default=1,
                   help="--select_by penetration: hands with fewer object points within 2 cm rank after all others")
    p.add_argument("--diverse_pool", type=int, default=0,
                   help="diverse best-of-M: keep the num_grasp most spread-out of the diverse_pool best-ranked candidates (greedy "
                        "farthest-point order, the best one first) instead of the num_grasp best; 0 = off, otherwise num_grasp <= "
                        "diverse_pool <= candidates; the JSON gains \"rank\" and \"novelty\"")
    p.add_argument("--diverse_space", choices=list(DIVERSE_SPACES), default="params",
                   help="what --diverse_pool measures distances in: the 61 parameters or the 778 posed vertices")
    p.add_argument("--refine_steps", type=int, default=0,
                   help="translation push-out: at most this many steps (<= 64) moving every generated hand out of its object along the "
                        "penetration proxy's gradient, before any scoring or selection (0 = off); the JSON gains \"refine_offset\" and "
                        "\"refine_iter\" (and the three scores when --candidates is off); untuned, effect on real grasps not measured")
    p.add_argument("--diversity", type=int, default=0,
                   help="the reference's diversity statistic of the grasps kept, on the device: k-means with this many clusters (the "
                        "paper uses 20; <= num_grasp and <= 64) over each object's [num_grasp,61] parameters, one deterministic run "
                        "from evenly spaced starting rows; 0 = off; every JSON gains \"diversity\" (clusters, entropy, mean_dist, "
                        "iters, counts) and the run writes the pooled statistic of all its grasps to diversity.json")
    p.add_argument("--object_contact", type=int, default=0,
                   help="1: where on the object its grasps land, of the grasps written (one kernel per call): every object's JSON gains "
                        "\"object_contact_map\" and \"object_interior_map\" (per point of the cloud file, how many of its grasps come "
                        "closer than --object_contact_threshold / have the point inside the hand), \"object_min_dist\" (cm, the nearest "
                        "any hand comes) and \"object_contact\" (grasps, coverage, entropy, threshold), and the run writes "
                        "object_contact.json; a proximity figure with an untuned threshold, effect on real grasps not measured")
    p.add_argument("--object_contact_threshold", type=float, default=0.02,
                   help="--object_contact: a hand closer than this many metres to an object point touches it (the scores' 2 cm; untuned)")
    p.add_argument("--stability", type=int, default=0,
                   help="1: every grasp's JSON gains \"force_residual\", \"torque_residual\", \"min_sv\" and \"stability_key\" (beside the "
                        "three scores): a frictionless unit-force force-closure proxy over the contact wrenches, without selecting by it "
                        "(--select_by stability writes them too); null where the hand touches nothing; a proxy with untuned constants that "
                        "replaces no physics run, effect on real grasps not measured")
    p.add_argument("--max_penetration", type=float, default=float("inf"),
                   help="--select_by stability: hands that penetrate more than this (the \"penetration\" score) rank after all others -- "
                        "the guard against hands that wrap the object by sinking into it (default: no limit)")
    p.add_argument("--torque_length", type=float, default=0.1,
                   help="--stability / --select_by stability: the length in metres that scales torques to forces (hand-sized default, untuned)")
    p.add_argument("--closure", type=int, default=0,
                   help="1: every grasp's JSON gains \"closure_quality\", \"force_closure\" and \"closure_direction\": the force-closure "
                        "quality with Coulomb friction of the hands written (one kernel per call) -- the smallest value, over "
                        "--closure_dirs sampled directions in wrench space, of the support function of the contacts' friction cones: an "
                        "upper bound of the L1 Ferrari-Canny quality, so a value <= 0 certifies NO force closure and a positive one "
                        "certifies nothing -- and the run writes closure.json; torques are scaled by --torque_length; null where the hand "
                        "touches nothing; no physics run, no soft contact, untuned constants, effect on real grasps not measured")
    p.add_argument("--friction", type=float, default=0.5, help="--closure / --min_closure: the Coulomb friction coefficient (untuned)")
    p.add_argument("--closure_dirs", type=int, default=256,
                   help=f"--closure / --min_closure: the number of sampled directions, 12..{ops.GRASP_CLOSURE_MAX_DIRS} (the signed axes, then "
                        "Halton points on the sphere in pairs u, -u)")
    p.add_argument("--min_closure", type=float, default=float("-inf"),
                   help="best-of-M: candidates whose closure quality is below this rank after all others that touch the object (the class "
                        "--max_penetration uses), whatever --select_by ranks by; needs --candidates (default: no guard)")
    p.add_argument("--volume", type=int, default=0,
                   help="1: every grasp's JSON gains \"penetration_volume\" (cm^3), \"penetration_depth\" (cm) and \"volume_voxels\": the "
                        "voxels shared by the sealed hand mesh and the convex hull of the object's cloud, counted on the device (one "
                        "kernel per call; the hulls are built on the host with scipy), and the run writes penetration.json with the "
                        "means and the contact ratio (the share of grasps with at least one voxel).  The hull of a sampled cloud lies "
                        "inside the mesh's: a lower bound of the reference's figure")
    p.add_argument("--volume_res", type=float, default=0.001, help="--volume / --max_volume: the voxel size in metres (the reference uses 1 mm)")
    p.add_argument("--max_volume", type=float, default=float("inf"),
                   help="best-of-M: candidates whose penetration volume exceeds this many cm^3 rank after all others that touch the object "
                        "(the class --max_penetration uses), whatever --select_by ranks by; needs --candidates (default: no limit)")
    p.add_argument("--volume_mesh", type=int, default=0,
                   help="--volume / --max_volume: what the hand's voxels are counted against.  0 = the convex hull of the object's "
                        "cloud (a lower bound of the reference's figure); 1 = the convex hull of the object's MESH vertices, the "
                        "reference's geometry (built on the host, the same kernel); 2 = the mesh itself, so that a finger in the hollow "
                        "of a cup or through a handle shares nothing with the object (one kernel per call): the solid intersection on "
                        "the object's own lattice, not metric/intersect.py's surface-voxel figure, undefined on an open mesh; "
                        "\"penetration_depth\" is then null (the depth against the mesh is --mesh_depth's).  1 and 2 need "
                        "--object_meshes; penetration.json gains \"against\"")
    p.add_argument("--parts", type=int, default=0,
                   help="1: every grasp's JSON gains \"fingers_in_contact\", \"part_contact\" and \"part_dist\" (cm) and every object's "
                        "\"hand_contact_map\": which parts of the hand -- thumb, four fingers, palm -- have vertices within "
                        "--part_threshold of the object's cloud, from the hand's side (one kernel per call), and the run writes "
                        "hand_contact.json; a proximity figure with an untuned threshold, no contact-force model, effect on real grasps "
                        "not measured")
    p.add_argument("--part_threshold", type=float, default=0.005,
                   help="--parts / --min_fingers / --need_thumb: a hand vertex closer than this many metres to the cloud touches (the "
                        "reference's 5 mm hard-contact tolerance; untuned)")
    p.add_argument("--part_min_verts", type=int, default=1, help="touching vertices a part needs to count as in contact")
    p.add_argument("--min_fingers", type=int, default=0,
                   help="best-of-M: candidates with fewer than this many of the five fingers in contact rank after all others that touch "
                        "the object (the class --max_penetration uses), whatever --select_by ranks by; 0..5, above 0 needs --candidates")
    p.add_argument("--need_thumb", type=int, default=0,
                   help="best-of-M: 1 = candidates whose thumb is not in contact join that class too; needs --candidates")
    p.add_argument("--hand_parts", default=None,
                   help="a label table {\"order\": [names], \"parts\": [[vertex indices], ...]} to use instead of the packaged one "
                        "(the fingers first, the thumb as part 0)")
    p.add_argument("--self_collision", type=int, default=0,
                   help="1: every grasp's JSON gains \"self_penetrating\", \"self_part_penetrating\", \"self_depth\" (cm), \"self_pairs\" "
                        "and \"self_clearance\" (cm): the vertices of a finger that lie behind the surface of another finger or of the palm "
                        "-- the hand against itself, after any push-out (one kernel per call) -- and the run writes self_collision.json; a "
                        "proximity figure on vertices only (a thin crossing between vertices is missed), calibrated against false alarms "
                        "only and untuned otherwise, effect on real grasps not measured")
    p.add_argument("--self_reach", type=float, default=0.01,
                   help="--self_collision / --max_self_verts: a vertex is tested against its nearest vertex of another part when that lies "
                        "within this many metres (untuned)")
    p.add_argument("--self_margin", type=float, default=0.001,
                   help="--self_collision / --max_self_verts: a vertex penetrates when it lies more than this many metres behind that "
                        "vertex's tangent plane (untuned)")
    p.add_argument("--self_seam", type=int, default=2,
                   help="--self_collision / --max_self_verts: vertices within this many edge rings of a join of two parts never count "
                        "(next to a join the test's sign is noise); 0 = every vertex counts")
    p.add_argument("--self_palm", type=int, default=1,
                   help="--self_collision / --max_self_verts: 1 = the fingers are tested against the palm too, 0 = against one another only")
    p.add_argument("--max_self_verts", type=int, default=None,
                   help="best-of-M: candidates with more than this many self-penetrating vertices rank after all others that touch the "
                        "object (the class --max_penetration uses), whatever --select_by ranks by; needs --candidates (default: no guard)")
    p.add_argument("--object_meshes", nargs="*", default=[],
                   help="the objects' triangle meshes, one per --objects file in the same order and in the cloud's own frame: .npz "
                        "(verts [n,3], faces [m,3]) or a Wavefront .obj of v / f lines; at most "
                        f"{ops.GRASP_MESH_MAX_FACES} faces each (decimate larger ones); what --mesh_depth and --max_mesh_depth test against "
                        "and what --mesh_points samples the clouds from (then there are no --objects files)")
    p.add_argument("--mesh_depth", type=int, default=0,
                   help="1: every grasp's JSON gains \"mesh_depth\" (cm) and \"mesh_interior\": the hand vertices inside the object's MESH "
                        "(a +z ray, watertight at edges and vertices) and the largest distance of one of them to its surface -- the "
                        "reference's metric/penetration.py figure, of the hands written (one kernel per call); every object's JSON gains "
                        "\"mesh_closed\" and \"mesh_penetration_map\", and the run writes mesh_penetration.json; needs --object_meshes; "
                        "on an open mesh the figures are undefined; work is rows x 1024 x faces pair tests: lower --rows_per_call for "
                        "big meshes")
    p.add_argument("--max_mesh_depth", type=float, default=float("inf"),
                   help="best-of-M: candidates whose mesh depth exceeds this many cm rank after all others that touch the object (the "
                        "class --max_penetration uses), whatever --select_by ranks by; needs --candidates and --object_meshes "
                        "(default: no guard)")
    p.add_argument("--mesh_points", type=int, default=0,
                   help="make every object's cloud from its mesh, on the device, instead of reading --objects: this many area-weighted "
                        "random points on the surface of each --object_meshes file (0 = off; the reference samples 3000 with trimesh). "
                        "The draws are the library's own keyed stream (seed, the object's global index, the sample index), NOT "
                        "trimesh's; objects are named by the mesh files' stems and every cloud is written to <out_dir>/obj_cloud_<name>.npy "
                        "([N,3] float32: the file --object_contact's point indices refer to); excludes --objects")
    p.add_argument("--mesh_points_even", type=int, default=1,
                   help="--mesh_points: above 1, draw mesh_points_even times as many samples and keep the mesh_points most spread-out "
                        "(farthest-point order from sample 0, on the device), so that the point-counting figures do not carry the "
                        f"sampling's clumps and holes; mesh_points * mesh_points_even <= {ops.CLOUD_FPS_MAX_P}; 1 = the samples as drawn; "
                        "effect on grasp quality not measured")
    p.add_argument("--refine_push", type=float, default=1.0, help="--refine_steps: step factor on the mean pull vector of the interior points")
    p.add_argument("--refine_pull", type=float, default=0.25,
                   help="--refine_steps: step factor on the mean pull vector of the points within 2 cm outside the hand")
    p.add_argument("--refine_spin", type=float, default=0.0,
                   help="--refine_steps: rigid push-out -- above 0 the hand may also turn about its wrist (the root joint), by this factor "
                        "times the least-squares small rotation towards the pull field per step; global_orient is updated and the JSON "
                        "gains \"refine_rotation\" (axis-angle); 0 = translation only; untuned, effect on real grasps not measured")
    p.add_argument("--refine_curl", type=float, default=0.0,
                   help="--refine_steps: articulated push-out -- above 0 every finger may also curl about its knuckle, by this factor times "
                        "the least-squares small rotation towards the pulls at its own vertices per step; hand_pose is updated, a row "
                        "whose re-posed hand scores worse than the hand as generated is reverted, and the JSON gains \"refine_curl\" "
                        "(axis-angles per finger) and \"refine_reverted\"; works with or without --refine_spin; 0 = no curl; untuned, "
                        "effect on real grasps not measured")
    p.add_argument("--refine_max_curl", type=float, default=0.35,
                   help="--refine_curl: the largest angle (radians) a finger may turn from the hand as generated; untuned")
    p.add_argument("--ttt_steps", type=int, default=0,
                   help="gradient refinement, the reference's test-time loop: this many steps (<= 1000; the reference runs 300) of SGD "
                        "with momentum on the 61 MANO parameters of every generated hand, down 7 * penetration + 1 * contact of the "
                        "reference's TTT_loss (one fused loss-and-gradient kernel and the MANO backward pass per step), after any "
                        "push-out and before any scoring or selection (0 = off); the JSON gains \"ttt_loss0\", \"ttt_loss\" and "
                        "\"ttt_iter\"; the constants are the reference's and untuned here, effect on real grasps not measured")
    p.add_argument("--ttt_lr", type=float, default=6.25e-6, help="--ttt_steps: the learning rate (the reference's)")
    p.add_argument("--ttt_momentum", type=float, default=0.8, help="--ttt_steps: the momentum (the reference's)")
    p.add_argument("--ttt_w_pen", type=float, default=840.0, help="--ttt_steps: the weight of the penetration term (the reference's 7 * 120)")
    p.add_argument("--ttt_w_con", type=float, default=7500.0,
                   help="--ttt_steps: the weight of the contact term, the mean squared distance of the object points within 2 cm to "
                        "the nearest contact vertex (the reference's 1 * 2.5 * 3000)")
    p.add_argument("--ttt_prior", default=None,
                   help="--ttt_steps: a JSON file holding the list of hand vertices the contact term measures distances to (the "
                        "reference uses 204 finger-pad and palm vertices); default: every vertex")
    p.add_argument("--ttt_keep_best", type=int, default=1,
                   help="--ttt_steps: 1 = every hand keeps its iterate of lowest loss, 0 = the last iterate, as the reference does")
    return p


def parse_args(dataset: str, argv: Optional[Sequence[str]] = None) -> argparse.Namespace:
    """build_parser(dataset).parse_args(argv) plus the checks of RULES; the dataset says whether its objects are rotated."""
    p = build_parser(dataset)
    args = p.parse_args(argv)
    o = types.SimpleNamespace(**vars(args), rotate=DATASETS[dataset]["rotate"])
    rule = _broken_rule(o, cli=True)
    if rule is not None:
        p.error(_rule_message(rule, o, cli=True))
    return args


def _prior_controls(temperature: float, top_k: int, log_prob: bool) -> Dict[str, object]:
    """Keyword arguments of GenNet.gen for the entry points' three flags: none at their defaults (today's call)."""
    if float(temperature) == 1.0 and int(top_k) == 0 and not log_prob:
        return {}
    return dict(temperature=float(temperature), top_k=int(top_k), log_prob=bool(log_prob), return_aux=True)


def grasp_log_prob(logp_model: torch.Tensor) -> torch.Tensor:
    """[B,9] per-position log-probabilities -> [B] per grasp: fp32 additions in raster order, written out so that a grasp's
    sum is the same bits in a call of any size (a library reduction may pick its order by the shape)."""
    total = logp_model[:, 0].clone()
    for i in range(1, logp_model.shape[1]):
        total = total + logp_model[:, i]
    return total


def rotation_xyz(angles: np.ndarray) -> np.ndarray:
    """Rx @ Ry @ Rz for angles [G,3] (gen_diverse_grasp_ho3d.py:214-219)."""
    cx, sx = np.cos(angles[:, 0]), np.sin(angles[:, 0])
    cy, sy = np.cos(angles[:, 1]), np.sin(angles[:, 1])
    cz, sz = np.cos(angles[:, 2]), np.sin(angles[:, 2])
    one, zero = np.ones_like(cx), np.zeros_like(cx)
    Rx = np.stack([one, zero, zero, zero, cx, -sx, zero, sx, cx], 1).reshape(-1, 3, 3)
    Ry = np.stack([cy, zero, sy, zero, one, zero, -sy, zero, cy], 1).reshape(-1, 3, 3)
    Rz = np.stack([cz, -sz, zero, sz, cz, zero, zero, zero, one], 1).reshape(-1, 3, 3)
    return Rx @ Ry @ Rz


def object_tensor(points_xyz: np.ndarray) -> torch.Tensor:
    """[N,3] cloud -> the datasets' [4,N] tensor: xyz + constant bbox-diagonal channel (dataset/dataset_FHAB.py:50-54)."""
    diag = float(np.linalg.norm(points_xyz.max(0) - points_xyz.min(0)))
    return torch.from_numpy(np.concatenate([points_xyz.T, np.full((1, points_xyz.shape[0]), diag)], 0).astype(np.float32))


def load_model(args, device) -> GenNet:
    net = GenNet(n_embeddings=args.n_embeddings)
    have = os.path.exists(args.checkpoint) and os.path.exists(args.prior_checkpoint)
    if have:                                         # gen_diverse_grasp_obman.py:333-346
        ck = torch.load(args.checkpoint, map_location="cpu")["network"]
        sd = net.state_dict()
        sd.update({k: v for k, v in ck.items() if k in sd})
        net.load_state_dict(sd)
        net.GatedPixelCNN.load_state_dict(torch.load(args.prior_checkpoint, map_location="cpu"))
    else:
        print(f"[generate] checkpoints not found ({args.checkpoint}); using deterministic synthetic weights")
        sd = synth.synthetic_state_dict(net.state_dict(), 1234)
        if args.n_embeddings < sd["GatedPixelCNN.output_conv.2.bias"].numel():
            sd["GatedPixelCNN.output_conv.2.bias"][args.n_embeddings:] = -1e4     # keep codes inside the codebooks
        net.load_state_dict(sd)
    net.eval().to(device)
    if os.path.exists(args.mano_model):
        layer = dmano.load(model_path=args.mano_model, model_type="mano", use_pca=True, num_pca_comps=45,
                           flat_hand_mean=True)
    else:
        print(f"[generate] {args.mano_model} not found; using the synthetic MANO-shaped model")
        layer = dmano.ManoLayer(dmano.synthetic_mano_arrays())
    net.set_rh_mano(layer.to(device))
    return net


@torch.no_grad()
def generate_for_object(net: GenNet, obj4n: torch.Tensor, num_grasp: int, rotate: bool, rng: np.random.Generator,
                        noise: Optional[torch.Tensor] = None, proxies: bool = False, seed: Optional[int] = None,
                        object_index: Optional[int] = None, row0: int = 0, temperature: float = 1.0, top_k: int = 0,
                        log_prob: bool = False) -> Dict[str, object]:
    """num_grasp grasps for one object in ONE batched call.  Returns the reference's JSON fields plus tensors.
    ``seed`` / ``object_index`` / ``row0`` key the prior's device noise (seed, stream = object, global grasp row), so the
    grasps of an object do not depend on which rank generates it or on how its grasps are split into calls.
    ``proxies``: also the per-grasp penetration / contact proxies (contact.grasp_proxies) of the posed hands against
    the (rotated) object clouds -- the cheap on-device stand-in for the scripts' trimesh / pybullet metrics.
    ``temperature`` / ``top_k``: controls on the prior's draws (GenNet.gen); ``log_prob``: also ``"log_prob"`` [G], each grasp's
    log-likelihood under the untempered prior (grasp_log_prob of aux["logp_model"]), and in the JSON."""
    dev = next(net.parameters()).device
    G = num_grasp
    if rotate:
        angles = rng.random((G, 3)) * np.pi * 2                                    # ho3d.py:214
        R = rotation_xyz(angles)
        t = np.asarray(CANONICAL_OFFSET)
    else:
        angles = np.zeros((G, 3))
        R = np.tile(np.eye(3), (G, 1, 1))
        t = np.zeros(3)
    batch = ops.transform_cloud(obj4n.to(dev).contiguous(), torch.as_tensor(R, dtype=torch.float32, device=dev),
                                torch.as_tensor(t, dtype=torch.float32, device=dev))
    recon, pos, *rest = net.gen(batch, noise=noise, seed=seed, row0=row0, stream_id=object_index,
                                **_prior_controls(temperature, top_k, log_prob))
    params = ops.assemble61(recon, pos)                                            # obman.py:243-247
    final = _pose(net, params)
    Rt = np.concatenate([R, np.broadcast_to(t.reshape(1, 3, 1), (G, 3, 1))], axis=2)
    extra, extra_json = {}, {}
    if log_prob:
        extra["log_prob"] = grasp_log_prob(rest[0]["logp_model"])
        extra_json["log_prob"] = extra["log_prob"].cpu().numpy().tolist()
    if proxies:
        extra["proxies"] = contact.grasp_proxies(_hand_topology(net, final.vertices.shape[1], dev), final.vertices, batch[:, :3].transpose(1, 2))
    return {**extra, "params": params, "vertices": final.vertices,
            "json": {"recon_params": [[p] for p in params.cpu().numpy().tolist()],   # [[61 floats]] per grasp, as the reference
                     "R_list": Rt.tolist(), "trans_list": [t.reshape(3, 1).tolist()] * G, "r_list": angles.tolist(), **extra_json}}


def _pose(net: GenNet, params: torch.Tensor):
    """The posed-MANO pass of [B,61] parameters: betas, global_orient, hand_pose, transl (obman.py:252-253)."""
    return net.rh_mano(betas=params[:, :10], global_orient=params[:, 10:13], hand_pose=params[:, 13:58], transl=params[:, 58:61])


def _hand_faces(net: GenNet) -> np.ndarray:
    faces = np.asarray(net.rh_mano.faces)
    if faces.size == 0 or int(faces.max()) == 0:
        raise RuntimeError("proxies: the MANO layer has no face list (synthetic model); load MANO_RIGHT.pkl")
    return faces


def _hand_topology(net: GenNet, n_verts: int, dev):
    faces = _hand_faces(net)
    topo = getattr(net, "_hand_topology", None)
    if topo is None or topo.faces.device != dev:
        topo = contact.HandTopology(faces, n_verts, dev)
        object.__setattr__(net, "_hand_topology", topo)
    return topo


def _finger_rig(net: GenNet):
    """The ``contact.FingerRig`` of the net's MANO layer, built once and kept on the model."""
    rig = getattr(net, "_finger_rig", None)
    if rig is None:
        rig = contact.FingerRig.from_mano(net.rh_mano)
        object.__setattr__(net, "_finger_rig", rig)
    return rig


REFINE_PIECES = ("offset", "iter", "rotation", "curl", "reverted")   # of a push-out's dict: what rides to the host, in this order


def _refine_fingers_call(net: GenNet, topo, params: torch.Tensor, first, cloud_xyz: torch.Tensor, steps: int, push: float, pull: float,
                         spin: float, curl: float, max_curl: float, min_contact: int):
    """The articulated push-out of one call's rows: contact.refine_fingers about the root joint and the knuckles of the first posed
    pass ``first``; the offset goes to ``transl``, the turn to ``global_orient``, the curls to ``hand_pose``
    (contact.compose_finger_pose), MANO is posed again -- and, because the kept iterate was the best only under the kernel's blend
    model, the hands that would be written are scored once (contact.grasp_scores) and a row whose key (class, penetration) came out
    worse than that of the hand as generated takes back its generated parameters, its first-pass vertices and joints, a zero offset,
    identity turns and iterate 0.  ``torch.where`` only: no host sync, no third MANO pass.  Returns (params, the hands written,
    refined); ``refined["scores"]`` holds ``contact.grasp_scores`` of the hands written, merged from the two score sets at hand."""
    rig = _finger_rig(net)
    knuckles = first.joints[:, rig.joints].contiguous()                            # [B,P,3]
    out = contact.refine_fingers(topo, rig, first.vertices, cloud_xyz, first.joints[:, 0].contiguous(), knuckles, steps, push, pull,
                                 spin, curl, max_curl, min_contact)
    new = params.clone()
    new[:, 10:13] = contact.compose_orient(params[:, 10:13], out["quat"])
    new[:, 13:58] = contact.compose_finger_pose(net.rh_mano, params[:, 10:13], params[:, 13:58], out["finger_quat"], rig)
    new[:, 58:61] = params[:, 58:61] + out["offset"]
    posed = _pose(net, new)
    scores1 = contact.grasp_scores(topo, posed.vertices, cloud_xyz)
    cls1, key1 = contact.select_keys(scores1, "penetration", min_contact)
    cls0, key0 = contact.select_keys({"penetration": out["penetration0"], "n_contact": out["n_contact0"]}, "penetration", min_contact)
    worse = (cls1 > cls0) | ((cls1 == cls0) & (key1 > key0))                       # [B]; a NaN key compares false: such a row never moved
    w1, w2 = worse.unsqueeze(-1), worse.view(-1, 1, 1)
    ident = torch.zeros_like(out["quat"])
    ident[:, 0] = 1.0
    quat = torch.where(w1, ident, out["quat"])
    fquat = torch.where(w2, ident.unsqueeze(1), out["finger_quat"])
    refined = {"offset": torch.where(w1, torch.zeros_like(out["offset"]), out["offset"]),
               "iter": torch.where(worse, torch.zeros_like(out["iter"]), out["iter"]), "quat": quat, "finger_quat": fquat,
               "curl": contact.quat_axis_angle(fquat.reshape(-1, 4)).reshape(fquat.shape[0], fquat.shape[1], 3),   # float64 [B,P,3]
               "reverted": worse.to(torch.int32),
               # the scores of the hands written: the guard's on the re-posed hands, iterate 0's (the bits of grasp_scores on the hand
               # as generated) on the reverted rows -- a caller that wants exactly these three needs no further launch
               "scores": {k: torch.where(worse, out[k + "0"], scores1[k]) for k in ("penetration", "n_interior", "n_contact")}}
    if spin:
        refined["rotation"] = contact.quat_axis_angle(quat)                        # float64 [B,3]
    final = types.SimpleNamespace(vertices=torch.where(w2, first.vertices, posed.vertices),
                                  joints=torch.where(w2, first.joints, posed.joints))
    return torch.where(w1, params, new), final, refined


def _hand_parts(net: GenNet, table):
    """The label table of ``generate_for_objects``' ``hand_parts``: a ``contact.HandParts`` as given, else the one read from the JSON
    path (None: the packaged table), kept on the model so that a run reads and uploads it once."""
    if isinstance(table, contact.HandParts):
        return table
    cached = getattr(net, "_hand_parts", None)
    if cached is None or cached[0] != table:
        cached = (table, contact.HandParts.from_json(table))
        object.__setattr__(net, "_hand_parts", cached)
    return cached[1]


def _self_table(net: GenNet, hand_parts, seam: int, palm: bool):
    """The ``contact.SelfTable`` of ``generate_for_objects``' self-collision switches: the label table of _hand_parts with the hand
    model's faces, kept on the model so that a run derives the seam and uploads it once."""
    parts = _hand_parts(net, hand_parts)
    cached = getattr(net, "_self_table", None)
    if cached is None or cached[0] is not parts or cached[1:3] != (int(seam), bool(palm)):
        cached = (parts, int(seam), bool(palm), contact.SelfTable(parts, _hand_faces(net), seam=seam, palm=palm, n_fingers=min(5, parts.n_parts)))
        object.__setattr__(net, "_self_table", cached)
    return cached[3]


def plan_calls(point_counts: Sequence[int], num_grasp: int, rows_per_call: int) -> List[List[int]]:
    """Positions of the objects of each batched call.  A call needs one point count: positions are grouped by it (groups in
    the order their first object appears, the given order inside a group) and every group is cut into calls of whole objects,
    at most ``max(1, rows_per_call // num_grasp)`` each -- an object's grasps are never split, so ``rows_per_call < num_grasp``
    gives one object per call.  Every position appears in exactly one call."""
    if num_grasp < 1 or rows_per_call < 1:
        raise ValueError(f"plan_calls: num_grasp and rows_per_call must be positive (got {num_grasp}, {rows_per_call})")
    per_call = max(1, rows_per_call // num_grasp)
    groups: Dict[int, List[int]] = {}
    for pos, n in enumerate(point_counts):
        groups.setdefault(int(n), []).append(pos)
    return [g[i:i + per_call] for g in groups.values() for i in range(0, len(g), per_call)]


@dataclasses.dataclass(frozen=True)
class _Options:
    """What generate_for_objects has validated, the same for every call of it: its keywords under their own names, filled by name, and
    five derived fields (_generate_objects): ``stability`` is also on with ``select_by="stability"``, ``figures`` holds the active
    per-row figures with their settings -- (_Figure, dict) pairs in the order of FIGURES, then those of EXTRA_FIGURES -- ``ttt`` the settings of
    contact.refine_ttt, or None, ``beam`` (poses, width) of a beam search, or None, and ``object_contact`` the threshold in metres of
    the object-side contact map, or None without it."""
    num_grasp: int
    rotate: bool
    seed: int
    proxies: bool
    temperature: float
    top_k: int
    log_prob: bool
    candidates: int
    select_by: str
    min_contact: int
    diverse_pool: int
    diverse_space: str
    refine_steps: int
    refine_push: float
    refine_pull: float
    refine_spin: float
    refine_curl: float
    refine_max_curl: float
    diversity: int
    stability: bool
    max_penetration: float
    torque_length: float
    figures: tuple
    ttt: Optional[Dict[str, object]]
    beam: Optional[tuple] = None
    object_contact: Optional[float] = None


@dataclasses.dataclass
class _Call:
    """The state of one batched call once its hands are final, for the figures' launches and _select_call: row o * G + g is grasp (or
    candidate) g of object o."""
    net: GenNet
    objs: Sequence[torch.Tensor]
    G: int                                      # rows per object
    batch: torch.Tensor                         # [O*G,4,N] the posed clouds
    err: torch.Tensor                           # the flag of ops.transform_clouds: read with the call's one copy
    obj_of_row: torch.Tensor
    frame: tuple                                # (R, t) on the device as the figures' kernels take them: (None, None) without rotation
    R: np.ndarray                               # [O*G,3,3], angles [O*G,3] and t [3] on the host
    angles: np.ndarray
    t: np.ndarray
    params: torch.Tensor
    vertices: torch.Tensor
    logp: Optional[torch.Tensor]                # [O*G] where the log-likelihood is written or ranked by
    refined: Optional[Dict[str, torch.Tensor]]  # the push-out's dict
    meshes: object                              # the contact.ObjectMeshes of the call's objects, or None
    indices: Sequence[int] = ()                 # the objects' global indices, for messages
    figs: Sequence = ()                         # (figure, settings, its launch's device tensors) of the active figures

    @property
    def cloud_xyz(self) -> torch.Tensor:
        return self.batch[:, :3].transpose(1, 2)


@torch.no_grad()
def _generate_call(net: GenNet, opt: _Options, objs: Sequence[torch.Tensor], object_indices: Sequence[int], meshes=None) -> List[Dict[str, object]]:
    """One batched call: the ``num_grasp`` grasps (with ``candidates`` = M: the M candidates) of each of ``objs`` (all of one point
    count), row o * G + g = grasp g of object o.  Every step is row-independent and keyed per row, so each object's slice holds the bits
    of its own ``generate_for_object`` call.  The stages, in order:
    1. the rotations of each object's own generator (``beam`` = (P, W): of its first P rows, W times each), ONE ``ops.transform_clouds``;
    2. ``GenNet.gen`` keyed per row -- or, with ``beam``, ONE ``GenNet.gen_beam`` search of width W per posed cloud, row p * W + r = rank r
       of pose p, the beams' scores as the rows' log-likelihoods -- then ``ops.assemble61`` and the posed-MANO pass;
    3. ``refine_steps``: the push-out of every row (contact.refine_translation; with ``refine_spin`` contact.refine_rigid about the root
       joint of the first pass; with ``refine_curl`` _refine_fingers_call) into the parameters, and MANO posed again;
    4. ``ttt``: contact.refine_ttt on every row, and MANO posed again -- everything below sees the hands of the parameters written;
    5. every active figure's ONE launch over all rows (_Figure.launch, in the order of FIGURES, then EXTRA_FIGURES);
    6. with ``candidates``: _select_call.  Otherwise the scores where a push-out or ``stability`` asks for them (contact.grasp_stability
       in the place of contact.grasp_scores; neither where the articulated push-out's guard has scored the rows), the k-means of
       ``diversity`` (_diversity_launch), the object-side contact map of ``object_contact`` over all rows (_object_contact_launch),
       the call's ONE device-to-host copy (_host_groups), the JSON lists of the whole call and the per-object split;
    7. _ttt_attach and _beam_attach."""
    dev = next(net.parameters()).device
    rotate, seed, beam = opt.rotate, opt.seed, opt.beam
    G, O = (opt.candidates or opt.num_grasp), len(objs)
    log_prob = bool(opt.log_prob) or bool(beam) or (bool(opt.candidates) and opt.select_by == "log_prob")   # the beams' scores: always written
    if rotate:                                  # each object's own generator, as the loop draws them; beam: its first P draws, W rows each
        P, W = beam if beam else (G, 1)
        angles = [np.repeat(np.random.default_rng([seed, int(gi)]).random((P, 3)) * np.pi * 2, W, axis=0) for gi in object_indices]
        R, angles, t = np.concatenate([rotation_xyz(a) for a in angles]), np.concatenate(angles), np.asarray(CANONICAL_OFFSET)
    else:
        R, angles, t = np.tile(np.eye(3), (O * G, 1, 1)), np.zeros((O * G, 3)), np.zeros(3)
    clouds = torch.stack([o.contiguous() for o in objs]).to(dev)                 # [O,4,N]: one copy per object, none per grasp
    obj_of_row = torch.arange(O, device=dev).repeat_interleave(G)
    stream_ids = torch.as_tensor(np.asarray(object_indices, dtype=np.int64), device=dev).repeat_interleave(G)
    row_ids = torch.arange(G, device=dev).repeat(O)
    err = ops.new_err_flag(dev)                                                    # read with the call's one copy below: no extra sync
    R_dev, t_dev = torch.as_tensor(R, dtype=torch.float32, device=dev), torch.as_tensor(t, dtype=torch.float32, device=dev)
    batch = ops.transform_clouds(clouds, obj_of_row, R_dev, t_dev, err=err)
    cloud_xyz = batch[:, :3].transpose(1, 2)
    baux = None
    if beam:                                                                       # one search per posed cloud: rows 0, W, 2 W, ... of the batch
        recon, pos, baux = net.gen_beam(batch[::beam[1]].contiguous(), int(beam[1]), return_aux=True)
        logp = baux["log_prob"]
    else:
        recon, pos, *rest = net.gen(batch, seed=seed, row_keys=(stream_ids, row_ids), **_prior_controls(opt.temperature, opt.top_k, log_prob))
        logp = grasp_log_prob(rest[0]["logp_model"]) if log_prob else None
    params = ops.assemble61(recon, pos)                                            # obman.py:243-247
    final = _pose(net, params)
    refined = None
    if opt.refine_steps:
        topo = _hand_topology(net, final.vertices.shape[1], dev)
        if opt.refine_curl:                                                        # fingers too: parameters, hands and the guard in one place
            params, final, refined = _refine_fingers_call(net, topo, params, final, cloud_xyz, opt.refine_steps, opt.refine_push,
                                                          opt.refine_pull, opt.refine_spin, opt.refine_curl, opt.refine_max_curl, opt.min_contact)
        elif opt.refine_spin:                                                      # about the wrist: the root joint's world position
            refined = contact.refine_rigid(topo, final.vertices, cloud_xyz, final.joints[:, 0].contiguous(), opt.refine_steps,
                                           opt.refine_push, opt.refine_pull, opt.refine_spin, opt.min_contact)
            params[:, 10:13] = contact.compose_orient(params[:, 10:13], refined["quat"])
            refined["rotation"] = contact.quat_axis_angle(refined["quat"])         # float64 [B,3]
        else:
            refined = contact.refine_translation(topo, final.vertices, cloud_xyz, opt.refine_steps, opt.refine_push, opt.refine_pull,
                                                 opt.min_contact)
        if not opt.refine_curl:
            params[:, 58:61] += refined["offset"]                                  # fp32; the hands below are those of these parameters
            final = _pose(net, params)
    tuned = None
    if opt.ttt:                                                                    # gradient refinement: after any push-out, before any score
        ttt = opt.ttt
        tuned = contact.refine_ttt(net.rh_mano, _hand_topology(net, final.vertices.shape[1], dev), params, cloud_xyz, ttt["steps"], ttt["lr"],
                                   ttt["momentum"], ttt["targets"], ttt["w_pen"], ttt["w_con"], ttt["keep_best"])
        params = tuned["params"]
        final = _pose(net, params)
        if refined is not None and "scores" in refined:                            # the push-out's guard scored the hands before this
            refined = {k: v for k, v in refined.items() if k != "scores"}
    call = _Call(net=net, objs=objs, G=G, batch=batch, err=err, obj_of_row=obj_of_row, frame=(R_dev, t_dev) if rotate else (None, None),
                 R=R, angles=angles, t=t, params=params, vertices=final.vertices, logp=logp, refined=refined,
                 meshes=meshes, indices=list(object_indices))
    call.figs = [(fig, s, fig.launch(s, call)) for fig, s in opt.figures]          # after the push-out: the hands of the parameters written
    if opt.candidates:
        return _beam_attach(_ttt_attach(_select_call(opt, call), tuned, G), baux, beam)
    div = _diversity_launch(params, O, G, opt.diversity) if opt.diversity else []
    omap = _object_contact_launch(call, O, G, None, opt.object_contact) if opt.object_contact else {}
    scores, s_names = {}, []
    if refined is not None or opt.stability:                                       # the scores of the hands written
        scores = _call_scores(opt, call)
        s_names = ["penetration", "n_interior", "n_contact"] + (["sums", "key"] if opt.stability else [])
    r_names = [k for k in REFINE_PIECES if k in refined] if refined is not None else []
    host = _host_groups({"params": [params], "refine": [refined[k] for k in r_names], "scores": [scores[k] for k in s_names],
                         **{fig.key: [d[k] for k in fig.pieces] for fig, _, d in call.figs}, "diversity": div,
                         "object_contact": [omap[k] for k in OBJECT_CONTACT_PIECES] if omap else [], "err": [err]})
    if int(host["err"][0][0]) != 0:
        raise RuntimeError("generate_for_objects: object index out of range in transform_clouds")
    # what every row shows beside its parameters, on the device and as JSON lists, in the order of the fields: the push-out's pieces,
    # the three scores, the stability figures
    s_host = dict(zip(s_names, host["scores"]))
    row_dev = {**{"refine_" + k: refined[k] for k in r_names}, **{k: scores[k] for k in s_names[:3]}}
    row_lists = {**{"refine_" + k: h.tolist() for k, h in zip(r_names, host["refine"])}, **{k: s_host[k].tolist() for k in s_names[:3]}}
    if opt.stability:
        row_dev.update(wrench_sums=scores["sums"], stability_key=scores["key"])
        row_lists.update(_stability_json(s_host["sums"], s_host["n_contact"], s_host["key"]))
    shown = [(fig, s, d, host[fig.key], fig.lists(s, host[fig.key])) for fig, s, d in call.figs]
    n_vol = sum(fig is _Volume for fig, _ in opt.figures)
    shown = shown[:n_vol] + ([None] if opt.diversity else []) + shown[n_vol:]    # here the diversity stands after the volume, before the rest
    div_dicts = _diversity_dicts(opt.diversity, host["diversity"]) if opt.diversity else None
    omap_json = _object_contact_json(opt.object_contact, host["object_contact"]) if opt.object_contact else None
    topo = _hand_topology(net, final.vertices.shape[1], dev) if opt.proxies else None
    # the JSON fields of the whole call as Python lists in ONE pass each (a .tolist() per object costs more than the device work at
    # one grasp per object), then the per-object split
    B = O * G
    p_list = host["params"][0].tolist()
    Rt_list = np.concatenate([call.R, np.broadcast_to(t.reshape(1, 3, 1), (B, 3, 1))], axis=2).tolist()
    r_list = call.angles.tolist()
    trans = t.reshape(3, 1).tolist()
    p_dev, v_dev = params.split(G), final.vertices.split(G)
    lp_list = logp.cpu().numpy().tolist() if logp is not None else None
    outs = []
    for o in range(O):
        lo, hi = o * G, (o + 1) * G
        extra, extra_json = {}, {}
        if logp is not None:
            extra["log_prob"] = logp[lo:hi]
            extra_json["log_prob"] = lp_list[lo:hi]
        if opt.proxies:                                                            # per object: the reductions see the loop's shapes
            extra["proxies"] = contact.grasp_proxies(topo, final.vertices[lo:hi], batch[lo:hi, :3].transpose(1, 2))
        if row_dev:                                                                # (one test: this loop is the cost of a call at one grasp per object)
            extra.update({k: x[lo:hi] for k, x in row_dev.items()})
            extra_json.update({k: v[lo:hi] for k, v in row_lists.items()})
        for entry in shown:
            if entry is None:
                extra["diversity"] = extra_json["diversity"] = div_dicts[o]
                continue
            fig, s, d, fig_h, lists = entry
            extra[fig.key] = {k: d[k][lo:hi] for k in fig.pieces[:fig.shown]}
            extra_json.update(fig.slice(s, lists, fig_h, lo, hi, call, o))
        if opt.object_contact:
            extra["object_contact"] = _object_contact_slice(omap, o, G)
            extra_json.update(omap_json[o])
        outs.append({**extra, "params": p_dev[o], "vertices": v_dev[o],
                     "json": {"recon_params": [[p] for p in p_list[lo:hi]],           # [[61 floats]] per grasp, as the reference
                              "R_list": Rt_list[lo:hi], "trans_list": [trans] * G, "r_list": r_list[lo:hi], **extra_json}})
    return _beam_attach(_ttt_attach(outs, tuned, G), baux, beam)


def _call_scores(opt: _Options, call: _Call) -> Dict[str, torch.Tensor]:
    """The scores of a call's hands against their clouds: ONE fused kernel -- contact.grasp_stability with ``stability``, else
    contact.grasp_scores -- or none where the articulated push-out's guard has scored these very hands (_refine_fingers_call)."""
    if not opt.stability and call.refined is not None and "scores" in call.refined:
        return dict(call.refined["scores"])
    topo = _hand_topology(call.net, call.vertices.shape[1], call.vertices.device)
    if opt.stability:
        return contact.grasp_stability(topo, call.vertices, call.cloud_xyz, opt.torque_length)
    return contact.grasp_scores(topo, call.vertices, call.cloud_xyz)


def _beam_attach(outs: List[Dict[str, object]], baux: Optional[Dict[str, torch.Tensor]], beam: Optional[Sequence[int]]) -> List[Dict[str, object]]:
    """``--beam_width``: where each grasp of a call's dicts came from -- all P * W rows of every object, or with best-of-M the rows
    ``candidate`` names -- as ``beam_pose``, ``beam_rank`` and ``beam_duplicate_of`` (the rank, within the same pose, of the first
    better beam with the same six hand codes, or -1: GenNet.beam_duplicates) int64 tensors and JSON lists.  The duplicates table of the
    call's O * P searches travels in a small copy of its own."""
    if baux is None:
        return outs
    P, W = int(beam[0]), int(beam[1])
    dup = baux["duplicate_of"].view(len(outs), P * W)
    dup_h = dup.cpu().numpy()
    for o, out in enumerate(outs):
        cand = np.asarray(out["json"]["candidate"], dtype=np.int64) if "candidate" in out["json"] else np.arange(P * W)
        out["beam_pose"], out["beam_rank"] = torch.from_numpy(cand // W), torch.from_numpy(cand % W)
        out["beam_duplicate_of"] = dup[o] if "candidate" not in out else dup[o].index_select(0, out["candidate"].reshape(-1))
        out["json"].update(beam_pose=(cand // W).tolist(), beam_rank=(cand % W).tolist(), beam_duplicate_of=dup_h[o][cand].tolist())
    return outs


TTT_PIECES = ("loss0", "loss", "iter")   # of contact.refine_ttt's dict: what rides to the host, in this order
TTT_MAX_STEPS = 1000                     # contact.TTT_MAX_STEPS


def _ttt_attach(outs: List[Dict[str, object]], tuned: Optional[Dict[str, torch.Tensor]], M: int) -> List[Dict[str, object]]:
    """``--ttt_steps``: the three figures of ``contact.refine_ttt`` for the grasps of a call's dicts -- all M rows of every object, or
    with best-of-M the rows ``candidate`` names -- as ``ttt_loss0`` / ``ttt_loss`` / ``ttt_iter`` tensors and JSON lists (a loss that
    is not finite becomes null), through one small device-to-host copy of their own.  ``tuned`` = None: the dicts as they are."""
    if tuned is None:
        return outs
    pieces = [tuned[k] for k in TTT_PIECES]
    if "candidate" in outs[0]:
        rows = torch.cat([out["candidate"] + o * M for o, out in enumerate(outs)])
        pieces = [x.index_select(0, rows) for x in pieces]
    n = pieces[0].shape[0] // len(outs)
    host = _host_copy(pieces)
    lists = [[float(x) if np.isfinite(x) else None for x in host[0]], [float(x) if np.isfinite(x) else None for x in host[1]],
             host[2].tolist()]
    for o, out in enumerate(outs):
        lo, hi = o * n, (o + 1) * n
        out.update({"ttt_" + k: x[lo:hi] for k, x in zip(TTT_PIECES, pieces)})
        out["json"].update({"ttt_" + k: v[lo:hi] for k, v in zip(TTT_PIECES, lists)})
    return outs


def _host_copy(pieces: Sequence[torch.Tensor]) -> List[np.ndarray]:
    """The given tensors (float32, float64, int32 or int64, in any order and of any length) on the host through ONE device-to-host copy: the
    pieces travel as bytes, and a piece that starts at an odd multiple of 4 bytes comes back as an unaligned view, which numpy reads
    correctly (tests/test_generate_combined.py)."""
    flat = [p.contiguous().reshape(-1).view(torch.uint8) for p in pieces]
    host = torch.cat(flat).cpu().numpy()
    out, lo = [], 0
    for p, f in zip(pieces, flat):
        dt = {torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}[p.dtype]
        out.append(host[lo:lo + f.numel()].view(dt).reshape(tuple(p.shape)))
        lo += f.numel()
    return out


def _stability_json(sums: np.ndarray, n_contact: np.ndarray, key: np.ndarray) -> Dict[str, list]:
    """``--stability`` / ``--select_by stability``: the four JSON lists of a call's rows from the host copies of the kernel's sums,
    contact counts and keys -- float64 on the host, row by row (contact.wrench_stats), so that a grasp's figures do not depend on which
    rows share the call.  A hand that touches nothing has no figure: null, and so has a key that is not finite."""
    out = contact.wrench_stats(sums, n_contact)
    out["stability_key"] = [float(k) if np.isfinite(k) else None for k in key]
    return out


def _host_groups(groups: Dict[str, Sequence[torch.Tensor]]) -> Dict[str, List[np.ndarray]]:
    """_host_copy by name: the device tensors of every group (a list, possibly empty) on the host under the group's own name, all of
    them through ONE device-to-host copy.  A call's paths build their groups by name and read them back by name, so no piece is found
    by its position in the packed copy."""
    host = iter(_host_copy([p for pieces in groups.values() for p in pieces]))
    return {name: [next(host) for _ in pieces] for name, pieces in groups.items()}


class _Figure:
    """One per-row figure of a call, described once: the two paths of a call (_generate_call, _select_call) and ``main`` loop over the
    active ones in the order of FIGURES.  ``s`` is the figure's settings, the dict generate_for_objects validated; ``call`` the _Call.
    ``key`` / ``scores_key``: where a dict shows the first ``shown`` of ``pieces`` -- of the grasps written and, with candidates, of ALL
    candidates.  ``pieces``: the device tensors of ``launch`` that ride in the call's one device-to-host copy, in this order; a piece
    named "err" is the kernel's error flag, every other one is per row.  ``launch(s, call)``: ONE kernel over all rows of the call,
    after the push-out and the gradient refinement have re-posed the hands.  ``guard(s, dev)``: with candidates, the class the figure
    raises -- the ranking's becomes the maximum of the two, whatever ``select_by`` ranks by: a guard only -- or None without a limit.
    ``lists(s, host)``: the per-row JSON lists from the host copies of the pieces, float64 on the host, row by row, so that a grasp's
    figures do not depend on which rows share the call; raises on the figure's own error flag.  ``slice(s, lists, host, lo, hi, call,
    o)``: the JSON fields of object o, whose grasps are the rows lo .. hi of the copies.  ``stem``, ``rows(json)`` and ``summary(args,
    net, rows)``: the run summary ``main`` writes to <stem>.json -- what it keeps of every object's JSON, and from those (in object
    order) the summary and the line printed; integers and exactly rounded sums, so that no grouping can change a bit.
    A figure is also the option group that asks for it (GROUPS, under ``key``): ``switch`` is the keyword that turns it on, ``limits``
    the keywords of its guard, ``limited(o)`` whether ``o`` -- anything with the options as attributes -- sets one of them, ``wanted(o)``
    whether the figure runs, ``keywords`` what ``main`` passes with it beside ``switch=True``, ``faces`` whether it needs the hand
    model's face list, and ``settings(o, net)`` the dict ``s``, built once every value check of the call has passed."""
    shown = None                                                                   # every piece
    faces = False

    @classmethod
    def wanted(cls, o) -> bool:
        return bool(getattr(o, cls.switch)) or cls.limited(o)

    @staticmethod
    def guard(s, dev):
        return None

    @staticmethod
    def slice(s, lists, host, lo, hi, call, o):
        return {k: v[lo:hi] for k, v in lists.items()}


def _mean(values: Sequence[float]) -> Optional[float]:
    return math.fsum(values) / len(values) if values else None


def _share(flags: Sequence[bool]) -> Optional[float]:
    return sum(1 for f in flags if f) / len(flags) if flags else None


VOLUME_PIECES = ("count", "depth", "status", "err")  # what a call's volume kernel leaves on the device (_Volume.launch)
VOLUME_AGAINST = {1: "mesh_hull", 2: "mesh"}         # --volume_mesh: what penetration.json's "against" says (absent at 0: the cloud's hull)
PARTS_PIECES = ("part_min", "part_count", "mask", "status")     # what a call's parts kernel leaves on the device (contact.grasp_parts)
SELF_PIECES = ("pen_count", "pen_depth", "gap_min", "pair_bits", "mask", "status")   # what a call's self-collision kernel leaves on the device
MESH_PIECES = ("n_inside", "depth", "mask", "err")   # what a call's mesh kernel leaves on the device (_Mesh.launch)


class _Volume(_Figure):
    """``--volume`` / ``--max_volume`` (settings ``res``, ``max_volume``): every object's convex hull once, on the host, from its own
    unrotated cloud (contact.hull_planes: scipy), and ONE ``contact.grasp_volume`` over all rows of the call with the call's
    ``obj_of_row``, ``R`` and ``t``.  ``--volume_mesh`` (setting ``mesh``, present only when it is not 0; the meshes are the call's
    ``contact.ObjectMeshes``): 1 = the hulls are those of the meshes' vertices, 2 = ONE ``contact.grasp_mesh_volume`` against the meshes
    themselves, which has no depth (the piece is NaN on the device and null in the JSON).  Candidates whose voxel count exceeds ``contact.volume_limit`` join class 1 and those without a
    figure class 2 (integer comparisons on the device).  The JSON fields are penetration_volume, penetration_depth and volume_voxels
    (contact.volume_stats); null where the kernel gives no figure (count < 0)."""
    key, scores_key, stem, pieces, shown = "volume", "volume_scores", "penetration", VOLUME_PIECES, 3
    switch, limits, keywords, faces = "volume", ("max_volume",), ("volume_res", "max_volume"), True

    @staticmethod
    def limited(o):
        return o.max_volume < math.inf

    @staticmethod
    def settings(o, net):
        mesh = int(getattr(o, "volume_mesh", 0))
        return dict(res=float(o.volume_res), max_volume=float(o.max_volume), **({"mesh": mesh} if mesh else {}))

    @staticmethod
    def launch(s, call):
        dev = call.vertices.device
        topo = _hand_topology(call.net, call.vertices.shape[1], dev)
        bad = ops.new_err_flag(dev)
        mesh = s.get("mesh", 0)
        if mesh == 2:                                                              # against the meshes themselves: no depth
            out = contact.grasp_mesh_volume(topo, call.meshes, call.vertices, call.obj_of_row, *call.frame, s["res"], err=bad)
            return {"count": out["count"], "depth": torch.full_like(out["count"], math.nan, dtype=torch.float32), "status": out["status"],
                    "err": bad}
        if mesh == 1:                                                              # the hulls of the meshes' vertices: the reference's geometry
            vo = call.meshes.vert_off
            hulls = [contact.hull_planes(call.meshes.verts[vo[o]:vo[o + 1]].astype(np.float64)) for o in range(len(call.objs))]
            for o, hull in enumerate(hulls):
                if hull.shape[0] > ops.GRASP_VOLUME_MAX_PLANES:
                    raise RuntimeError(f"generate_for_objects: volume_mesh=1: the hull of the mesh of object {call.indices[o]} has "
                                       f"{hull.shape[0]} planes, at most {ops.GRASP_VOLUME_MAX_PLANES} fit (decimate the mesh)")
        else:
            hulls = [contact.hull_planes(o[:3].T.cpu().numpy().astype(np.float64)) for o in call.objs]
        planes, plane_off = contact.pack_planes(hulls)
        out = contact.grasp_volume(topo, call.vertices, torch.from_numpy(planes).to(dev), torch.from_numpy(plane_off).to(dev),
                                   call.obj_of_row, *call.frame, s["res"], err=bad)
        return {**out, "err": bad}

    @staticmethod
    def guard(s, dev):
        if not s["max_volume"] < float("inf"):
            return None
        cnt = dev["count"]
        over = (cnt > contact.volume_limit(s["max_volume"], s["res"])).to(torch.int32)
        return torch.where(cnt < 0, torch.full_like(over, 2), over)

    @staticmethod
    def lists(s, host):
        count, depth, _, bad = host
        if int(bad[0]) != 0:
            raise RuntimeError("generate_for_objects: volume: an index of the hand topology, of the hulls or of the meshes is out of range")
        out = contact.volume_stats(count, depth, s["res"])
        if s.get("mesh", 0) == 2:                                                  # no depth against the mesh: null, never a NaN
            out["penetration_depth"] = [None] * len(out["penetration_depth"])
        out["volume_voxels"] = [int(k) if k >= 0 else None for k in count]
        return out

    @staticmethod
    def rows(j):                                                                   # (voxels, cm^3, cm) per grasp
        return list(zip(*(j[k] for k in ("volume_voxels", "penetration_volume", "penetration_depth"))))

    @staticmethod
    def summary(args, net, rows):
        # contact_ratio is the reference's rule, "volume > 0", on the voxel count
        rows = [r for obj in rows for r in obj if r[0] is not None]
        stat = {"res": args.volume_res, "grasps": len(rows), "mean_volume_cm3": _mean([r[1] for r in rows]),
                "mean_depth_cm": _mean([r[2] for r in rows if r[2] is not None]), "contact_ratio": _share([r[0] >= 1 for r in rows])}
        if args.volume_mesh:
            stat["against"] = VOLUME_AGAINST[args.volume_mesh]
        return stat, (f"penetration volume of {len(rows)} grasps at {args.volume_res} m: mean {stat['mean_volume_cm3']} cm^3, "
                      f"mean depth {stat['mean_depth_cm']} cm, contact ratio {stat['contact_ratio']}")


class _Parts(_Figure):
    """``--parts`` / ``--min_fingers`` / ``--need_thumb`` (settings ``table``, ``threshold``, ``min_verts``, ``min_fingers``,
    ``need_thumb``): ONE ``contact.grasp_parts`` over all rows of the call, every hand vertex against its row's cloud.  Too few fingers
    on the object joins class 1, a row without a figure class 2 (contact.parts_class).  The JSON fields are fingers_in_contact,
    part_contact and part_dist (contact.part_stats; null where a row has no figure) and, per object, "hand_contact_map": at every
    vertex, how many of its grasps touch there (contact.contact_map)."""
    key, scores_key, stem, pieces = "parts", "part_scores", "hand_contact", PARTS_PIECES
    switch, limits = "parts", ("min_fingers", "need_thumb")
    keywords = ("part_threshold", "part_min_verts", "min_fingers", "need_thumb", "hand_parts")

    @staticmethod
    def limited(o):
        return o.min_fingers > 0 or bool(o.need_thumb)

    @staticmethod
    def settings(o, net):
        return dict(table=_hand_parts(net, o.hand_parts), threshold=float(o.part_threshold), min_verts=int(o.part_min_verts),
                    min_fingers=int(o.min_fingers), need_thumb=bool(o.need_thumb))

    @staticmethod
    def launch(s, call):
        return contact.grasp_parts(s["table"], call.vertices, call.cloud_xyz, s["threshold"])

    @staticmethod
    def guard(s, dev):
        if not (s["min_fingers"] or s["need_thumb"]):
            return None
        return contact.parts_class(dev, s["min_fingers"], s["need_thumb"], s["min_verts"])

    @staticmethod
    def lists(s, host):
        part_min, part_count, _, status = host
        return contact.part_stats(part_min, part_count, status, s["min_verts"], min(5, s["table"].n_parts))

    @staticmethod
    def slice(s, lists, host, lo, hi, call, o):
        return {**_Figure.slice(s, lists, host, lo, hi, call, o), "hand_contact_map": contact.contact_map(host[2][lo:hi], s["table"].n_verts).tolist()}

    @staticmethod
    def rows(j):                                                                   # (fingers per grasp, contact map)
        return j["fingers_in_contact"], j["hand_contact_map"]

    @staticmethod
    def summary(args, net, rows):
        fingers = [f for obj in rows for f in obj[0] if f is not None]
        stat = {"parts": _hand_parts(net, args.hand_parts).names, "threshold": args.part_threshold, "min_verts": args.part_min_verts,
                "grasps": len(fingers), "hand_contact_map": [int(sum(col)) for col in zip(*(obj[1] for obj in rows))],
                "mean_fingers_in_contact": _mean(fingers), "fingers_histogram": [sum(1 for f in fingers if f == k) for k in range(6)]}
        return stat, (f"hand-side contact of {len(fingers)} grasps at {args.part_threshold} m: mean fingers in contact "
                      f"{stat['mean_fingers_in_contact']}, histogram 0..5 {stat['fingers_histogram']}")


class _Self(_Figure):
    """``--self_collision`` / ``--max_self_verts`` (settings ``table``, ``reach``, ``margin``, ``max_verts``): ONE ``contact.grasp_self``
    over all rows of the call -- the hands against themselves.  More than ``max_verts`` self-penetrating vertices joins class 1, a row
    without a figure class 2 (contact.self_class).  The JSON fields are the five of contact.self_stats; null where a row has no figure."""
    key, scores_key, stem, pieces = "self", "self_scores", "self_collision", SELF_PIECES
    switch, limits = "self_collision", ("max_self_verts",)
    keywords = ("self_reach", "self_margin", "self_seam", "self_palm", "max_self_verts", "hand_parts")

    @staticmethod
    def limited(o):
        return o.max_self_verts is not None

    @staticmethod
    def settings(o, net):
        return dict(table=_self_table(net, o.hand_parts, int(o.self_seam), bool(o.self_palm)), reach=float(o.self_reach),
                    margin=float(o.self_margin), max_verts=None if o.max_self_verts is None else int(o.max_self_verts))

    @staticmethod
    def launch(s, call):
        return contact.grasp_self(_hand_topology(call.net, call.vertices.shape[1], call.vertices.device), s["table"], call.vertices, s["reach"],
                                  s["margin"])

    @staticmethod
    def guard(s, dev):
        return contact.self_class(dev, s["max_verts"]) if s["max_verts"] is not None else None

    @staticmethod
    def lists(s, host):
        return contact.self_stats(dict(zip(SELF_PIECES, host)))

    @staticmethod
    def rows(j):                                                                   # (counts, pairs) per grasp
        return j["self_penetrating"], j["self_pairs"]

    @staticmethod
    def summary(args, net, rows):
        table = _self_table(net, args.hand_parts, args.self_seam, bool(args.self_palm))
        counts = [c for obj in rows for c in obj[0] if c is not None]
        pairs = [tuple(ab) for obj in rows for g in obj[1] if g is not None for ab in g]
        names = table.parts.names
        stat = {"parts": names, "reach": args.self_reach, "margin": args.self_margin, "seam": args.self_seam,
                "palm": int(args.self_palm), "seam_vertices": table.n_seam, "grasps": len(counts),
                "share_penetrating": _share([c > 0 for c in counts]), "mean_penetrating": _mean(counts),
                "pair_histogram": [[pairs.count((a, b)) for b in range(len(names))] for a in range(len(names))]}
        return stat, (f"self-collision of {len(counts)} grasps at reach {args.self_reach} m, margin {args.self_margin} m: share "
                      f"with a penetrating vertex {stat['share_penetrating']}, mean count {stat['mean_penetrating']}")


class _Mesh(_Figure):
    """``--mesh_depth`` / ``--max_mesh_depth`` (settings ``max_depth`` in cm; the meshes are the call's ``contact.ObjectMeshes``, packed
    and uploaded once per call): ONE ``contact.grasp_mesh`` over all rows of the call with the call's ``obj_of_row``, ``R`` and ``t``.
    Deeper inside the object's mesh than ``max_depth`` joins class 1, a row without a figure class 2 (contact.mesh_class).  The JSON
    fields are mesh_depth and mesh_interior (contact.mesh_stats; null where the kernel gives no figure, n_inside < 0) and, per object,
    whether its mesh is closed and "mesh_penetration_map": at every hand vertex, how many of its grasps have it inside the mesh."""
    key, scores_key, stem, pieces, shown = "mesh", "mesh_scores", "mesh_penetration", MESH_PIECES, 3
    switch, limits, keywords = "mesh_depth", ("max_mesh_depth",), ("max_mesh_depth",)   # (``object_meshes`` goes per call)

    @staticmethod
    def limited(o):
        return o.max_mesh_depth < math.inf

    @staticmethod
    def settings(o, net):
        return dict(max_depth=float(o.max_mesh_depth))

    @staticmethod
    def launch(s, call):
        bad = ops.new_err_flag(call.vertices.device)
        out = contact.grasp_mesh(call.meshes, call.vertices, call.obj_of_row, *call.frame, err=bad)
        return {**{k: out[k] for k in MESH_PIECES[:3]}, "err": bad}

    @staticmethod
    def guard(s, dev):
        return contact.mesh_class(dev, s["max_depth"]) if s["max_depth"] < float("inf") else None

    @staticmethod
    def lists(s, host):
        n_inside, depth, _, bad = host
        if int(bad[0]) != 0:
            raise RuntimeError("generate_for_objects: mesh depth: an object index, an object's range or a face index is out of range")
        return contact.mesh_stats({"n_inside": n_inside, "depth": depth})

    @staticmethod
    def slice(s, lists, host, lo, hi, call, o):
        return {**_Figure.slice(s, lists, host, lo, hi, call, o), "mesh_closed": bool(call.meshes.closed[o]),
                "mesh_penetration_map": contact.contact_map(host[2][lo:hi], call.vertices.shape[1]).tolist()}

    @staticmethod
    def rows(j):                                                                   # (depths, counts, map)
        return j["mesh_depth"], j["mesh_interior"], j["mesh_penetration_map"]

    @staticmethod
    def summary(args, net, rows):
        depths = [d for obj in rows for d in obj[0] if d is not None]
        counts = [c for obj in rows for c in obj[1] if c is not None]
        stat = {"grasps": len(counts), "mean_depth_cm": _mean(depths), "mean_interior": _mean(counts),
                "share_penetrating": _share([c > 0 for c in counts]),
                "mesh_penetration_map": [int(sum(col)) for col in zip(*(obj[2] for obj in rows))]}
        return stat, (f"penetration depth against the meshes of {len(counts)} grasps: mean depth {stat['mean_depth_cm']} cm, "
                      f"mean inside count {stat['mean_interior']}, share with a vertex inside {stat['share_penetrating']}")


FIGURES = (_Volume, _Parts, _Self, _Mesh)                                        # the order of launches, dict keys, JSON fields and summaries

CLOSURE_PIECES = ("quality", "worst_dir", "status")  # what a call's closure kernel leaves on the device (contact.grasp_closure)


class _Closure(_Figure):
    """``--closure`` / ``--min_closure`` (settings ``friction``, ``dirs``, ``min_closure``, ``length``): ONE ``contact.grasp_closure``
    over all rows of the call, the hands against their clouds at the scores' contact threshold and the stability proxy's torque length.
    A quality below ``min_closure`` joins class 1, and so does a hand that touches nothing; a row with a coordinate that is not finite
    joins class 2 (contact.closure_class).  The JSON fields are closure_quality, force_closure and closure_direction
    (contact.closure_stats; null where a row has no figure).  A figure like the four of FIGURES, but not one of them and not in GROUPS:
    its options are no keywords of generate_for_objects (they are generate_with_closure's), so _generate_objects appends it to the
    active figures, after the four, and ``main`` asks it by name."""
    key, scores_key, stem, pieces = "closure", "closure_scores", "closure", CLOSURE_PIECES
    switch, limits, keywords, faces = "closure", ("min_closure",), ("friction", "closure_dirs", "min_closure"), True

    @staticmethod
    def limited(o):
        return o.min_closure > -math.inf

    @staticmethod
    def settings(o, net):
        return dict(friction=float(o.friction), dirs=int(o.closure_dirs), min_closure=float(o.min_closure), length=float(o.torque_length))

    @staticmethod
    def launch(s, call):
        topo = _hand_topology(call.net, call.vertices.shape[1], call.vertices.device)
        return contact.grasp_closure(topo, call.vertices, call.cloud_xyz, s["length"], s["friction"], s["dirs"])

    @staticmethod
    def guard(s, dev):
        return contact.closure_class(dev, s["min_closure"]) if s["min_closure"] > -math.inf else None

    @staticmethod
    def lists(s, host):
        return contact.closure_stats(*host)

    @staticmethod
    def rows(j):                                                                   # (quality, force closure) per grasp
        return list(zip(j["closure_quality"], j["force_closure"]))

    @staticmethod
    def summary(args, net, rows):
        rows = [r for obj in rows for r in obj if r[0] is not None]
        stat = {"friction": args.friction, "dirs": args.closure_dirs, "torque_length": args.torque_length, "grasps": len(rows),
                "closure_ratio": _share([r[1] for r in rows]), "mean_quality": _mean([r[0] for r in rows])}
        return stat, (f"force-closure quality of {len(rows)} grasps at friction {args.friction} over {args.closure_dirs} directions: "
                      f"share not refuted {stat['closure_ratio']}, mean quality {stat['mean_quality']}")


EXTRA_FIGURES = (_Closure,)                                                      # figures outside FIGURES and GROUPS, in the order they follow the four


def _diversity_launch(kept: torch.Tensor, O: int, keep: int, clusters: int) -> List[torch.Tensor]:
    """``--diversity``: one ``ops.segment_kmeans`` over the call's kept parameters [O*keep,61], one segment per object, from evenly
    spaced starting rows; the device tensors whose host copies _diversity_dicts reads (counts, dist, iters_used, the error flag)."""
    from . import diversity as dv
    bad = ops.new_err_flag(kept.device)
    _, counts, _, dist, used = ops.segment_kmeans(kept, dv.kmeans_init(O, keep, clusters, "spaced", device=kept.device), O, keep,
                                                  DIVERSITY_ITERS, err=bad)
    return [counts, dist, used, bad]


def _diversity_dicts(clusters: int, host: Sequence[np.ndarray]) -> List[Dict[str, object]]:
    """The "diversity" entry of every object of a call from the host copies of _diversity_launch's tensors: float64 on the host, per
    object, so that an object's entry does not depend on which objects share the call."""
    from . import diversity as dv
    counts, dist, used, bad = host
    if int(bad[0]) != 0:
        raise RuntimeError("generate_for_objects: diversity: a starting row of the k-means is not finite")
    return [{k: d[k] for k in ("clusters", "entropy", "mean_dist", "iters", "counts")}
            for d in dv.segment_statistics(clusters, counts, dist, used)]


OBJECT_CONTACT_PIECES = ("touch", "inside", "dmin", "n_valid", "err")   # of _object_contact_launch's dict: what rides to the host, in this order


def _object_contact_launch(call: _Call, O: int, K: int, rows: Optional[torch.Tensor], threshold: float) -> Dict[str, torch.Tensor]:
    """``--object_contact``: one ``contact.object_contact`` over the grasps written -- all rows of the call (``rows`` = None: object o's
    are rows o * K .. o * K + K - 1), or the kept rows by their index list against the call's hands and clouds, read in place (no
    gather) -- at ``threshold`` metres; the kernel's tensors and its error flag."""
    dev = call.vertices.device
    bad = ops.new_err_flag(dev)
    out = contact.object_contact(_hand_topology(call.net, call.vertices.shape[1], dev), call.vertices, call.cloud_xyz, O, K, rows,
                                 float(threshold) ** 2, err=bad)
    return {**out, "err": bad}


def _object_contact_slice(omap: Dict[str, torch.Tensor], o: int, K: int) -> Dict[str, torch.Tensor]:
    """Object o's part of _object_contact_launch's tensors, on the device."""
    return {**{k: omap[k][o] for k in ("touch", "inside", "dmin", "near_sum", "n_valid")}, "row_status": omap["row_status"][o * K:(o + 1) * K]}


def _object_contact_json(threshold: float, host: Sequence[np.ndarray]) -> List[Dict[str, object]]:
    """The four object-side contact fields of every object of a call from the host copies of OBJECT_CONTACT_PIECES: float64 on the host,
    per object (contact.object_contact_stats), so that an object's entry does not depend on which objects share the call.  Index p is
    point p of the object's cloud.  A distance that is not finite becomes null."""
    touch, inside, dmin, n_valid, bad = host
    if int(bad[0]) != 0:
        raise RuntimeError("generate_for_objects: object_contact: a row index is out of range")
    stats = contact.object_contact_stats(touch, inside, dmin, np.zeros_like(dmin), n_valid)
    return [{"object_contact_map": t.tolist(), "object_interior_map": i.tolist(),
             "object_min_dist": [x if x is not None and math.isfinite(x) else None for x in st["min_dist"]],
             "object_contact": {"grasps": st["grasps"], "coverage": st["coverage"], "entropy": st["entropy"], "threshold": float(threshold)}}
            for t, i, st in zip(touch, inside, stats)]


def _select_call(opt: _Options, call: _Call) -> List[Dict[str, object]]:
    """Best-of-M for all the objects of a call together; row o * M + c is candidate c of object o, and nothing here depends on which
    objects share the call.  The stages, in order:
    1. the candidates' scores: ONE fused kernel (contact.grasp_stability with ``stability``, else contact.grasp_scores, or none where
       the articulated push-out's guard has scored the rows), their classes and keys (contact.select_keys), and every active figure's
       guard on the class (_Figure.guard);
    2. each object's ``num_grasp`` best (ops.segment_topk: one kernel) -- or, with ``diverse_pool`` = P, its P best and the
       ``num_grasp`` most spread-out of them in greedy farthest-point order (ops.segment_diverse over the parameters or the posed
       vertices, read in place), whose pool positions and squared gaps ride along;
    3. ONE ``index_select`` per tensor of the kept rows: parameters, vertices, scores, the push-out's REFINE_PIECES, the figures'
       pieces; the k-means of ``diversity`` over the kept parameters (_diversity_launch); the object-side contact map of
       ``object_contact`` over the kept rows, by their index list against the call's hands and clouds (_object_contact_launch);
    4. the call's ONE device-to-host copy (_host_groups), the JSON lists of the kept rows and the per-object split."""
    net, params, vertices, logp, refined = call.net, call.params, call.vertices, call.logp, call.refined
    O, M, keep, dev = len(call.objs), call.G, opt.num_grasp, params.device
    topo = _hand_topology(net, vertices.shape[1], dev) if opt.proxies else None
    scores = _call_scores(opt, call)
    if logp is not None:
        scores["log_prob"] = logp
    cls, key = contact.select_keys(scores, opt.select_by, opt.min_contact, log_prob=logp, max_penetration=opt.max_penetration)
    for fig, s, d in call.figs:
        guard = fig.guard(s, d)
        if guard is not None:
            cls = torch.maximum(cls, guard)
    diverse = []
    if opt.diverse_pool:
        pool = ops.segment_topk(cls.contiguous(), key.contiguous(), O, M, opt.diverse_pool)   # [O,P] candidate indices, best first
        feat = params if opt.diverse_space == "params" else vertices.reshape(vertices.shape[0], -1)
        pool_err = ops.new_err_flag(dev)                                                  # read with everything else, below
        sel, rank, gap = ops.segment_diverse(feat, pool, O, M, keep, err=pool_err)        # [O,keep] in pick order
        diverse = [rank, gap, pool_err]
    else:
        sel = ops.segment_topk(cls.contiguous(), key.contiguous(), O, M, keep)            # [O,keep] candidate indices, best first
    rows = (sel + torch.arange(O, device=dev).unsqueeze(1) * M).reshape(-1)                 # rows of the call
    kept_p, kept_v = params.index_select(0, rows), vertices.index_select(0, rows)
    kept_s = {k: v.index_select(0, rows) for k, v in scores.items()}
    names = sorted(kept_s)
    r_names = [k for k in REFINE_PIECES if k in refined] if refined is not None else []
    kept_r = [refined[k].index_select(0, rows) for k in r_names]
    div = _diversity_launch(kept_p, O, keep, opt.diversity) if opt.diversity else []
    omap = _object_contact_launch(call, O, keep, rows, opt.object_contact) if opt.object_contact else {}
    kept_f = {fig.key: {k: d[k] if k == "err" else d[k].index_select(0, rows) for k in fig.pieces} for fig, _, d in call.figs}
    host = _host_groups({"sel": [sel], "params": [kept_p], "scores": [kept_s[k] for k in names], "refine": kept_r,
                         **{k: list(f.values()) for k, f in kept_f.items()}, "diverse": diverse, "diversity": div,
                         "object_contact": [omap[k] for k in OBJECT_CONTACT_PIECES] if omap else [], "err": [call.err]})
    if int(host["err"][0][0]) != 0:
        raise RuntimeError("generate_for_objects: object index out of range in transform_clouds")
    sel_h, p_list = host["sel"][0], host["params"][0].tolist()
    s_host = dict(zip(names, host["scores"]))
    s_list = {k: h.tolist() for k, h in s_host.items() if k not in ("centre", "sums", "key")}
    stab_lists = _stability_json(s_host["sums"], s_host["n_contact"], s_host["key"]) if opt.stability else {}
    r_lists = [h.tolist() for h in host["refine"]]
    shown = [(fig, s, d, kept_f[fig.key], host[fig.key], fig.lists(s, host[fig.key])) for fig, s, d in call.figs]
    if opt.diverse_pool:
        rank_h, gap_h, pool_err_h = host["diverse"]
        if int(pool_err_h[0]) != 0:
            raise RuntimeError("generate_for_objects: pool entry out of range in segment_diverse")
        rank_list, gap_list = rank_h.tolist(), gap_h.tolist()
    div_dicts = _diversity_dicts(opt.diversity, host["diversity"]) if opt.diversity else None
    omap_json = _object_contact_json(opt.object_contact, host["object_contact"]) if opt.object_contact else None
    rows_h = (sel_h + np.arange(O)[:, None] * M).reshape(-1)
    t = call.t
    Rt_list = np.concatenate([call.R[rows_h], np.broadcast_to(t.reshape(1, 3, 1), (O * keep, 3, 1))], axis=2).tolist()
    r_list = call.angles[rows_h].tolist()
    c_list = sel_h.tolist()
    trans = t.reshape(3, 1).tolist()
    json_scores = ["penetration", "n_interior", "n_contact"] + (["log_prob"] if logp is not None else [])
    p_dev, v_dev = kept_p.split(keep), kept_v.split(keep)
    outs = []
    for o in range(O):
        lo, hi = o * keep, (o + 1) * keep
        extra = {"log_prob": kept_s["log_prob"][lo:hi]} if logp is not None else {}
        if opt.proxies:                                                            # of the kept grasps, as the plain path returns them
            extra["proxies"] = contact.grasp_proxies(topo, v_dev[o], call.batch.index_select(0, rows[lo:hi])[:, :3].transpose(1, 2))
        extra_json = {k: v[lo:hi] for k, v in stab_lists.items()}
        if opt.stability:
            extra["wrench_sums"], extra["stability_key"] = kept_s["sums"][lo:hi], kept_s["key"][lo:hi]
        if opt.diverse_pool:
            extra["rank"], extra["novelty"] = rank[o], gap[o]
            extra_json.update(rank=rank_list[o], novelty=gap_list[o])
        extra.update({"refine_" + k: x[lo:hi] for k, x in zip(r_names, kept_r)})
        extra_json.update({"refine_" + k: x[lo:hi] for k, x in zip(r_names, r_lists)})
        if opt.diversity:
            extra["diversity"] = extra_json["diversity"] = div_dicts[o]
        for fig, s, d, kept_d, fig_h, lists in shown:
            extra[fig.key] = {k: kept_d[k][lo:hi] for k in fig.pieces[:fig.shown]}
            extra[fig.scores_key] = {k: d[k][o * M:(o + 1) * M] for k in fig.pieces[:fig.shown]}    # of ALL candidates
            extra_json.update(fig.slice(s, lists, fig_h, lo, hi, call, o))
        if opt.object_contact:
            extra["object_contact"] = _object_contact_slice(omap, o, keep)
            extra_json.update(omap_json[o])
        outs.append({**extra, "params": p_dev[o], "vertices": v_dev[o], "candidate": sel[o],
                     "scores": {k: v[o * M:(o + 1) * M] for k, v in scores.items()},
                     "json": {"recon_params": [[p] for p in p_list[lo:hi]], "R_list": Rt_list[lo:hi], "trans_list": [trans] * keep,
                              "r_list": r_list[lo:hi], "candidate": c_list[o], **{k: s_list[k][lo:hi] for k in json_scores},
                              **extra_json}})
    return outs


@dataclasses.dataclass(frozen=True)
class _Group:
    """An option group without a per-row figure, in the vocabulary of _Figure: ``wanted(o)`` whether it is on, ``keywords`` what ``main``
    passes when it is (under the flags' own names), ``switch`` the bool keyword forced on with it, ``faces`` whether it needs the hand
    model's face list, ``settings(o, net)`` what _Options holds for it, built once every value check of the call has passed."""
    wanted: Callable[[object], bool]
    keywords: tuple
    switch: Optional[str] = None
    faces: bool = False
    settings: Optional[Callable] = None


def _ttt_settings(o, net) -> Dict[str, object]:
    return dict(steps=int(o.ttt_steps), lr=float(o.ttt_lr), momentum=float(o.ttt_momentum), w_pen=float(o.ttt_w_pen),
                w_con=float(o.ttt_w_con), targets=_ttt_targets(o.ttt_prior), keep_best=bool(o.ttt_keep_best))


# every option group by name: what is on for an ``o`` -- the parsed flags, or the bound keywords of a call -- is asked here and nowhere else
GROUPS = {
    "selection": _Group(lambda o: bool(o.candidates), ("candidates", "select_by", "min_contact"), faces=True),
    "diverse": _Group(lambda o: bool(o.diverse_pool), ("diverse_pool", "diverse_space")),
    "pushout": _Group(lambda o: bool(o.refine_steps), ("refine_steps", "refine_push", "refine_pull", "min_contact"), faces=True),
    "spin": _Group(lambda o: bool(o.refine_spin), ("refine_spin",)),
    "curl": _Group(lambda o: bool(o.refine_curl), ("refine_curl", "refine_max_curl")),
    "ttt": _Group(lambda o: bool(o.ttt_steps), ("ttt_steps", "ttt_lr", "ttt_momentum", "ttt_w_pen", "ttt_w_con", "ttt_prior", "ttt_keep_best"),
                  faces=True, settings=_ttt_settings),
    "diversity": _Group(lambda o: bool(o.diversity), ("diversity",)),
    "beam": _Group(lambda o: bool(o.beam_width), ("beam_width", "beam_poses"), settings=lambda o, net: (int(o.beam_poses), int(o.beam_width))),
    "stability": _Group(lambda o: bool(o.stability) or (bool(o.candidates) and o.select_by == "stability"),
                        ("max_penetration", "torque_length"), switch="stability", faces=True),
    **{fig.key: fig for fig in FIGURES},
    # (a flag, but no keyword of generate_for_objects: on the keyword path it is on inside generate_with_object_contact)
    "object_contact": _Group(lambda o: bool(o.object_contact), ("object_contact_threshold",), faces=True,
                             settings=lambda o, net: float(o.object_contact_threshold)),
}


@dataclasses.dataclass(frozen=True)
class _Rule:
    """One check of the options, stated once for both entry paths.  ``names``: the options refused; ``ok(o)``: the predicate over
    anything with the options as attributes (``rotate`` among them); ``text``: what follows the names in the message, ``$`` marking
    further option names; ``gate``: the group that must be on for the KEYWORD path to apply the rule (parse_args applies every rule it
    has: ``--torque_length -1`` is refused without ``--stability``); ``only``: "cli" or "keywords" where one path alone has the rule."""
    names: tuple
    ok: Callable[[object], bool]
    text: str
    gate: Optional[str] = None
    only: Optional[str] = None


VOLUME_MESH_OPTIONS = (0, 1, 2)   # --volume_mesh: the cloud's hull, the hull of the mesh's vertices, the mesh itself


def _rule(names: str, ok, text: str, gate: Optional[str] = None, only: Optional[str] = None) -> _Rule:
    return _Rule(tuple(names.split()), ok, text, gate, only)


def _positive(x) -> bool:
    return 0.0 < x < math.inf


def _not_negative(x) -> bool:
    return 0.0 <= x < math.inf


# --volume_mesh.  Marked "cli": the keyword is generate_with_volume_mesh's, not generate_for_objects' (whose keywords are pinned), so
# the keyword path's table has no such option to look at; _generate_objects applies these same three to it.
VOLUME_MESH_RULES = (
    _rule("volume_mesh", lambda o: o.volume_mesh in VOLUME_MESH_OPTIONS, "must be 0, 1 or 2", only="cli"),
    _rule("volume_mesh", lambda o: not o.volume_mesh or (bool(o.object_meshes) and len(o.object_meshes) == len(getattr(o, "objs", o.object_meshes))),
          "needs $object_meshes, one per object (the surfaces it counts against)", only="cli"),
    _rule("volume_mesh", lambda o: not o.volume_mesh or _Volume.wanted(o),
          "needs $volume or $max_volume (it says what the volume figure is counted against)", only="cli"),
)

# --closure and its three options.  Marked "cli" for the same reason: the keywords are generate_with_closure's, and _generate_objects
# applies these same six to them.  (The fifth names its second way in without the marker: the options a rule marks are the ones its
# message shows.)
CLOSURE_RULES = (
    _rule("closure", lambda o: o.closure in (0, 1), "is 0 or 1", only="cli"),
    _rule("friction", lambda o: _not_negative(o.friction), "must be finite and >= 0", only="cli"),
    _rule("closure_dirs", lambda o: 12 <= o.closure_dirs <= ops.GRASP_CLOSURE_MAX_DIRS,
          f"must lie between 12 and {ops.GRASP_CLOSURE_MAX_DIRS} (the directions $closure samples: the twelve signed axes first)", only="cli"),
    _rule("min_closure", lambda o: not math.isnan(o.min_closure), "must not be NaN", only="cli"),
    _rule("min_closure", lambda o: not _Closure.limited(o) or bool(o.candidates),
          "needs $candidates (a guard on the ranking of candidates; $closure alone writes the figures)", only="cli"),
    _rule("closure_dirs friction", lambda o: (o.closure_dirs == 256 and o.friction == 0.5) or _Closure.wanted(o),
          "away from their defaults need $closure, or a min_closure limit (they are the closure figure's settings)", only="cli"),
)

_TORQUE_LENGTH_RULE = _rule("torque_length", lambda o: _positive(o.torque_length), "must be finite and positive", "stability")

RULES = (
    _rule("candidates", lambda o: not o.candidates or o.candidates >= max(1, o.num_grasp), "must be 0 or at least $num_grasp"),
    # keywords only, as it has been: ``--candidates 5000`` gets past parse_args and dies in the call; drop the marker to refuse it there
    _rule("candidates", lambda o: o.candidates <= ops.SEGMENT_TOPK_MAX_M, f"may be at most {ops.SEGMENT_TOPK_MAX_M} per object", only="keywords"),
    _rule("select_by", lambda o: o.select_by in contact.SELECT_BY, f"must be one of {contact.SELECT_BY}", "selection", "keywords"),
    _rule("diverse_pool", lambda o: not o.diverse_pool or (bool(o.candidates) and o.num_grasp <= o.diverse_pool <= o.candidates),
          "must be 0, or lie between $num_grasp and $candidates"),
    _rule("diverse_space", lambda o: o.diverse_space in DIVERSE_SPACES, f"must be one of {DIVERSE_SPACES}", "diverse", "keywords"),
    _rule("diversity", lambda o: 0 <= o.diversity <= min(o.num_grasp, ops.SEGMENT_KMEANS_MAX_K),
          f"must lie between 0 and min($num_grasp, {ops.SEGMENT_KMEANS_MAX_K})"),
    *(_rule(name, lambda o, name=name: getattr(o, name) in (0, 1), "is 0 or 1", only="cli")
      for name in ("object_contact", "ttt_keep_best", "need_thumb", "parts", "self_collision", "self_palm", "mesh_depth")),
    _rule("object_contact_threshold", lambda o: _positive(o.object_contact_threshold), "must be finite and positive", "object_contact"),
    _rule("refine_steps", lambda o: 0 <= o.refine_steps <= ops.GRASP_REFINE_MAX_STEPS, f"must lie between 0 and {ops.GRASP_REFINE_MAX_STEPS}"),
    _rule("refine_push refine_pull", lambda o: _not_negative(o.refine_push) and _not_negative(o.refine_pull), "must be finite and >= 0", "pushout"),
    _rule("refine_spin", lambda o: _not_negative(o.refine_spin), "must be finite and >= 0"),
    _rule("refine_spin", lambda o: not o.refine_spin or bool(o.refine_steps), "needs $refine_steps (it turns the hand during the push-out)"),
    _rule("refine_curl", lambda o: _not_negative(o.refine_curl), "must be finite and >= 0"),
    _rule("refine_curl", lambda o: not o.refine_curl or bool(o.refine_steps), "needs $refine_steps (it curls the fingers during the push-out)"),
    _rule("refine_max_curl", lambda o: 0.0 < o.refine_max_curl <= math.pi, "must lie in (0, pi]"),
    _rule("ttt_steps", lambda o: 0 <= o.ttt_steps <= TTT_MAX_STEPS, f"must lie between 0 and {TTT_MAX_STEPS}"),
    _rule("ttt_lr", lambda o: _not_negative(o.ttt_lr), "must be finite and >= 0", "ttt"),
    _rule("ttt_momentum", lambda o: 0.0 <= o.ttt_momentum < 1.0, "must lie in [0, 1)", "ttt"),
    _rule("ttt_w_pen ttt_w_con", lambda o: _not_negative(o.ttt_w_pen) and _not_negative(o.ttt_w_con), "must be finite and >= 0", "ttt"),
    _rule("ttt_prior", lambda o: o.ttt_prior is None or bool(o.ttt_steps),
          "needs $ttt_steps (it names the contact vertices of the gradient refinement)"),
    _TORQUE_LENGTH_RULE,
    _rule("max_penetration", lambda o: o.max_penetration >= 0.0, "must be >= 0", "stability"),
    _rule("volume_res", lambda o: _positive(o.volume_res), "must be finite and positive", "volume"),
    _rule("max_volume", lambda o: o.max_volume >= 0.0, "must be >= 0", "volume"),
    _rule("part_threshold", lambda o: _positive(o.part_threshold), "must be finite and positive", "parts"),
    _rule("part_min_verts", lambda o: o.part_min_verts >= 1, "must be at least 1", "parts"),
    _rule("min_fingers", lambda o: 0 <= o.min_fingers <= 5, "must lie between 0 and 5"),
    _rule("self_reach", lambda o: _positive(o.self_reach), "must be finite and positive", "self"),
    _rule("self_margin", lambda o: _not_negative(o.self_margin), "must be finite and >= 0", "self"),
    _rule("self_seam", lambda o: o.self_seam >= 0, "must be >= 0", "self"),
    _rule("max_self_verts", lambda o: o.max_self_verts is None or o.max_self_verts >= 0, "must be >= 0"),
    _rule("max_mesh_depth", lambda o: o.max_mesh_depth >= 0.0, "must be >= 0", "mesh"),
    *(_rule(" ".join(fig.limits), lambda o, fig=fig: not fig.limited(o) or bool(o.candidates),
            f"needs $candidates (a guard on the ranking of candidates; ${fig.switch} alone writes the figures)") for fig in FIGURES),
    _rule("object_meshes", lambda o: not o.object_meshes or bool(o.mesh_points) or len(o.object_meshes) == len(o.objects),
          "needs one mesh per $objects file, in the same order", only="cli"),
    _rule("mesh_depth max_mesh_depth", lambda o: not _Mesh.wanted(o) or bool(o.object_meshes),
          "need $object_meshes (the surfaces they test against)", only="cli"),
    _rule("object_meshes", lambda o: o.object_meshes is not None and len(o.object_meshes) == len(o.objs),
          "must hold one (verts, faces) per object of $objs: what mesh_depth and max_mesh_depth test against", "mesh", "keywords"),
    _rule("object_indices", lambda o: len(o.object_indices) == len(o.objs), "must hold one index per object of $objs", only="keywords"),
    _rule("beam_width", lambda o: 0 <= o.beam_width <= ops.PIXELCNN_BEAM_MAX_W, f"must lie between 0 and {ops.PIXELCNN_BEAM_MAX_W}"),
    _rule("beam_poses", lambda o: o.beam_poses >= 1, "must be at least 1"),
    _rule("beam_poses", lambda o: bool(o.beam_width) or o.beam_poses == 1, "needs $beam_width (it counts the poses a beam search runs for)"),
    _rule("beam_poses", lambda o: not o.beam_width or o.beam_poses == 1 or bool(o.rotate),
          "must be 1 where the objects are not rotated: every pose would be the same $beam_width search"),
    _rule("beam_width", lambda o: not o.beam_width or (o.candidates or o.num_grasp) == o.beam_poses * o.beam_width,
          "times $beam_poses must equal $candidates or, without it, $num_grasp"),
    _rule("beam_width", lambda o: not o.beam_width or (o.temperature == 1.0 and o.top_k == 0),
          "excludes $temperature and $top_k: a beam search draws nothing"),
    # (new rules go to the END of the table: the tests name a rule by its position)
    _rule("mesh_points", lambda o: 0 <= o.mesh_points <= ops.MESH_SAMPLE_MAX_S, f"must lie between 0 and {ops.MESH_SAMPLE_MAX_S}", only="cli"),
    _rule("mesh_points_even", lambda o: o.mesh_points_even >= 1, "must be at least 1", only="cli"),
    _rule("mesh_points", lambda o: o.mesh_points_even <= 1 or o.mesh_points * o.mesh_points_even <= ops.CLOUD_FPS_MAX_P,
          f"times $mesh_points_even may be at most {ops.CLOUD_FPS_MAX_P} where $mesh_points_even is above 1 (the pool the even "
          "subsampling holds in registers)", only="cli"),
    _rule("mesh_points mesh_points_even", lambda o: not o.mesh_points or bool(o.object_meshes),
          "need $object_meshes (the surfaces the clouds are sampled from)", only="cli"),
    _rule("mesh_points", lambda o: not o.mesh_points or not o.objects,
          "excludes $objects: the clouds come from $object_meshes", only="cli"),
    _rule("mesh_points_even", lambda o: o.mesh_points_even == 1 or bool(o.mesh_points),
          "needs $mesh_points (it thins the cloud sampled from the mesh)", only="cli"),
    *CLOSURE_RULES,
    *VOLUME_MESH_RULES,
)


def _rule_options(rule: _Rule) -> List[str]:
    """The options a rule reads: its names, then those its text marks."""
    return list(dict.fromkeys(list(rule.names) + re.findall(r"\$(\w+)", rule.text)))


def _broken_rule(o, cli: bool) -> Optional[_Rule]:
    """The first of RULES that ``o`` breaks on the flag path (``cli``) or the keyword path, or None."""
    for rule in RULES:
        if rule.only == ("keywords" if cli else "cli") or (rule.gate and not cli and not GROUPS[rule.gate].wanted(o)):
            continue
        if not rule.ok(o):
            return rule
    return None


def _rule_message(rule: _Rule, o, cli: bool) -> str:
    """``--names text (got ...)`` for parse_args, the same without the dashes for the keyword path; a sequence shows its length."""
    dash = "--" if cli else ""
    got = ((n, getattr(o, n)) for n in _rule_options(rule))
    got = ", ".join(f"{dash}{n} {'of %d entries' % len(v) if isinstance(v, (list, tuple)) else repr(v)}" for n, v in got)
    return f"{' and '.join(dash + n for n in rule.names)} {rule.text.replace('$', dash)} (got {got})"


def generate_for_objects(net: GenNet, objs: Sequence[torch.Tensor], num_grasp: int, rotate: bool, seed: int,
                         object_indices: Sequence[int], proxies: bool = False, rows_per_call: int = 16384, temperature: float = 1.0,
                         top_k: int = 0, log_prob: bool = False, candidates: int = 0, select_by: str = "penetration",
                         min_contact: int = 1, diverse_pool: int = 0, diverse_space: str = "params", refine_steps: int = 0,
                         refine_push: float = 1.0, refine_pull: float = 0.25, diversity: int = 0, stability: bool = False,
                         max_penetration: float = float("inf"), torque_length: float = 0.1, volume: bool = False,
                         volume_res: float = 0.001, max_volume: float = float("inf"), parts: bool = False,
                         part_threshold: float = 0.005, part_min_verts: int = 1, min_fingers: int = 0, need_thumb: bool = False,
                         hand_parts=None, refine_spin: float = 0.0, refine_curl: float = 0.0,
                         refine_max_curl: float = 0.35, self_collision: bool = False, self_reach: float = 0.01,
                         self_margin: float = 0.001, self_seam: int = 2, self_palm: bool = True,
                         max_self_verts: Optional[int] = None, object_meshes=None, mesh_depth: bool = False,
                         max_mesh_depth: float = float("inf"), ttt_steps: int = 0, ttt_lr: float = 6.25e-6,
                         ttt_momentum: float = 0.8, ttt_w_pen: float = 840.0, ttt_w_con: float = 7500.0, ttt_prior=None,
                         ttt_keep_best: bool = True, beam_width: int = 0, beam_poses: int = 1) -> List[Dict[str, object]]:
    """``num_grasp`` grasps for each of ``objs`` ([4,N] tensors) in batched calls that mix objects (plan_calls): one dict per
    object, in the order given, equal to ``generate_for_object(net, objs[i], num_grasp, rotate,
    np.random.default_rng([seed, object_indices[i]]), seed=seed, object_index=object_indices[i], proxies=proxies)`` (and the same
    ``temperature`` / ``top_k`` / ``log_prob``) --
    tensors bit for bit, ``json`` as Python objects.  Per call: the rotations of each object's own generator, one
    ``ops.transform_clouds``, one ``GenNet.gen(row_keys=)`` with stream = object index and row = grasp index, one ``assemble61``,
    one posed-MANO pass, one device-to-host copy.  A call's clouds and intermediates are freed before the next call; the results
    returned stay on the device, so hand over one call's objects at a time (as ``main`` does) when the list is long.

    Best-of-M (``candidates`` = M >= ``num_grasp``): every call generates M rows per object -- candidate c is exactly grasp c of a
    ``num_grasp = M`` run -- scores them against their clouds (``contact.grasp_scores``), ranks them (``contact.select_keys`` by
    ``select_by`` / ``min_contact``, ``ops.segment_topk``) and keeps each object's ``num_grasp`` best, best first: ``params``
    [num_grasp,61], ``vertices``, ``candidate`` [num_grasp] (indices into the M), ``scores`` (the [M] tensors of ALL candidates:
    penetration, n_interior, n_contact and, when computed, log_prob) and ``json`` with the four reference fields of the kept grasps
    plus "candidate", "penetration", "n_interior", "n_contact" (and "log_prob" when asked for or selected by).  Still one
    device-to-host copy per call and no per-object device work; needs a MANO layer with a face list.

    Diverse best-of-M (``diverse_pool`` = P, ``num_grasp`` <= P <= ``candidates``): of each object's P best-ranked candidates the
    call keeps the ``num_grasp`` most spread-out ones, in greedy farthest-point order starting from the best (``ops.segment_diverse``;
    squared distances over the 61 parameters, or over the posed vertices with ``diverse_space="verts"``).  The kept grasps come in
    pick order; the dicts gain ``rank`` (int32 [num_grasp], the position in the ranking) and ``novelty`` (fp32 [num_grasp], the
    squared distance to the nearest earlier pick, -1 for the first), and ``json`` gains "rank" and "novelty" after the scores.
    ``diverse_pool = 0`` is the call without the keyword.

    Translation push-out (``refine_steps`` = K > 0, ``refine_push``, ``refine_pull``): after the posed-MANO pass and before any scoring
    or selection, ALL rows of a call go through ``contact.refine_translation`` against their clouds (one kernel; ``min_contact`` is
    its contact class too), ``params[:, 58:61] += offset`` in fp32 and MANO is posed again, so ``vertices`` are the vertices of the
    parameters returned; best-of-M then ranks the refined candidates.  The dicts gain ``refine_offset`` [num_grasp,3] and
    ``refine_iter`` [num_grasp] (the iterate kept, 0 = untouched), and so does ``json``; without ``candidates`` the dicts and ``json``
    also gain ``penetration``, ``n_interior``, ``n_contact``: ``contact.grasp_scores`` of the refined hands.  Everything rides in the
    call's one device-to-host copy; needs a face list like best-of-M.  Parameters 0 .. 57 are those of the call without it.
    ``refine_steps = 0`` is the call without the keyword.  The constants are untuned and the effect on real grasps is not measured.

    Rigid push-out (``refine_spin`` = S > 0 together with ``refine_steps``): the rows go through ``contact.refine_rigid`` instead, with
    the root joint's world position of the first posed pass (``joints[:, 0]``) as the pivot, so the hand may also turn about its wrist:
    besides the offset, ``params[:, 10:13]`` becomes ``contact.compose_orient(params[:, 10:13], quat)`` before MANO is posed again
    (parameters 0 .. 9 and 13 .. 57 stay).  The dicts gain ``refine_rotation`` [num_grasp,3] (float64: the axis-angle of the turn) next
    to ``refine_offset`` / ``refine_iter``, and so does ``json``.  ``refine_spin = 0`` is the call without the keyword.

    Articulated push-out (``refine_curl`` = C > 0 together with ``refine_steps``, with or without ``refine_spin``): the rows go through
    ``contact.refine_fingers`` instead, with the knuckles of the first posed pass (``joints[:, rig.joints]``, the rig built once from
    the layer: ``contact.FingerRig.from_mano``) as the fingers' pivots and ``refine_max_curl`` radians as the largest turn of a
    finger.  Besides the offset and the turn, ``params[:, 13:58]`` becomes ``contact.compose_finger_pose(...)`` before MANO is posed
    again (parameters 0 .. 9 stay).  The kernel searches with a blend model of the hand, so the re-posed hands are scored once and a
    row whose key (class, penetration) came out worse than that of the hand as generated is REVERTED: it keeps its generated
    parameters and hand, a zero offset, identity turns and ``refine_iter`` = 0.  The dicts gain ``refine_curl`` [num_grasp,P,3]
    (float64: the axis-angle of every finger's turn, in the rig's order) and ``refine_reverted`` [num_grasp] (int32), and so does
    ``json``.  ``refine_curl = 0`` is the call without the keyword.  Untuned; the effect on real grasps is not measured.

    Diversity statistic (``diversity`` = K, 1 <= K <= min(``num_grasp``, 64)): after selection and push-out the kept [num_grasp,61]
    parameters of every object of a call go through ONE ``ops.segment_kmeans`` (one segment per object, K clusters, evenly spaced
    starting rows, at most 100 iterations); counts and distances ride in the call's one device-to-host copy and the two floats are
    computed per object on the host (``diversity.kmeans_statistics``).  Each dict and each ``json`` gains ``"diversity"``: a dict of
    clusters, entropy, mean_dist, iters and counts -- one deterministic run, not scipy's best of 20 random starts
    (``diversity.diversity``).  ``diversity = 0`` is the call without the keyword.

    Stability proxy (``stability=True``, or ``select_by="stability"`` together with ``candidates``): the scores of a call come from
    ``contact.grasp_stability`` -- ONE kernel in the place of ``contact.grasp_scores``, after the push-out has re-posed the hands if
    there is one -- with ``torque_length`` as its length.  ``select_by="stability"`` ranks the candidates by its key (``min_contact``
    and ``max_penetration`` set the class, ``contact.select_keys``).  Each dict gains ``wrench_sums`` [num_grasp,27] and
    ``stability_key`` [num_grasp] (and ``scores`` gains centre, sums and key of all candidates); ``json`` gains "force_residual",
    "torque_residual", "min_sv" and "stability_key" per grasp (``contact.wrench_stats``, float64 on the host; null where the hand
    touches nothing) and, without ``candidates``, the three scores as well.  The sums ride in the call's one device-to-host copy.
    A frictionless unit-force proxy with untuned constants: it replaces no physics run and its effect on real grasps is not
    measured.  Without either switch nothing of it runs.

    Penetration volume (``volume=True``, or a finite ``max_volume`` together with ``candidates``): every call builds the convex hull
    of each of its objects once on the host (``contact.hull_planes`` of the object's own unrotated cloud; needs scipy) and launches ONE
    ``contact.grasp_volume`` over all its rows with the call's ``obj_of_row``, rotations and offset, after the push-out has re-posed
    the hands if there is one; ``volume_res`` is the voxel size in metres.  ``max_volume`` (cm^3): candidates whose voxel count
    exceeds ``contact.volume_limit(max_volume, volume_res)`` join class 1 -- the class of ``max_penetration`` -- and candidates without
    a figure class 2, whatever ``select_by`` ranks by.  Each dict gains ``volume`` (count, depth, status of its grasps; with
    ``candidates`` also ``volume_scores``, those of ALL candidates) and ``json`` gains "penetration_volume" (cm^3),
    "penetration_depth" (cm) and "volume_voxels" per grasp (``contact.volume_stats``, float64 on the host; null without a figure).
    They ride in the call's one device-to-host copy.  A lower bound of the reference's intersection_eval (the cloud's hull lies inside
    the mesh's) on the object's own lattice; no igl / trimesh run pins parity.  Without either switch nothing of it runs.

    Hand-side contact (``parts=True``, or ``min_fingers`` > 0 / ``need_thumb`` together with ``candidates``): every call launches ONE
    ``contact.grasp_parts`` over all its rows -- every hand vertex against its row's cloud, a vertex closer than ``part_threshold``
    metres touches -- after the push-out has re-posed the hands if there is one.  ``hand_parts``: the label table, a
    ``contact.HandParts``, a JSON path, or None for the packaged MANO table (thumb, four fingers, palm).  ``min_fingers`` = K:
    candidates with fewer than K of the five fingers in contact (a part counts with ``part_min_verts`` touching vertices) join class
    1, and so do candidates whose thumb does not touch under ``need_thumb``; rows without a figure join class 2
    (``contact.parts_class``), whatever ``select_by`` ranks by: a guard only, nothing is ranked by it.  Each dict gains ``parts``
    (part_min, part_count, mask, status of its grasps; with ``candidates`` also ``part_scores``, those of ALL candidates) and ``json``
    gains "fingers_in_contact", "part_contact" and "part_dist" (cm) per grasp (``contact.part_stats``, float64 on the host; null
    without a figure) and "hand_contact_map", per vertex the number of the object's grasps that touch there.  They ride in the
    call's one device-to-host copy.  A proximity figure with an untuned threshold: no contact-force model, effect on real grasps not
    measured.  Without these switches nothing of it runs.
    Self-collision (``self_collision=True``, or ``max_self_verts`` = K together with ``candidates``): every call launches ONE
    ``contact.grasp_self`` over all its rows -- the hands against themselves, the fingers of ``hand_parts`` against one another and,
    with ``self_palm``, against the remaining parts; ``self_reach`` / ``self_margin`` in metres, ``self_seam`` in edge rings
    (``contact.SelfTable``) -- after the push-out has re-posed the hands if there is one.  Candidates with more than K penetrating
    vertices join class 1, rows without a figure class 2 (``contact.self_class``), whatever ``select_by`` ranks by: a guard only,
    nothing is ranked by it.  Each dict gains ``self`` (the kernel's six tensors of its grasps; with ``candidates`` also
    ``self_scores``, those of ALL candidates) and ``json`` gains "self_penetrating", "self_part_penetrating", "self_depth" (cm),
    "self_pairs" and "self_clearance" (cm) per grasp (``contact.self_stats``, float64 on the host; null without a figure).  A
    proximity figure on vertices only, calibrated against false alarms only: untuned, effect on real grasps not measured.  Without
    these switches nothing of it runs.

    Gradient refinement (``ttt_steps`` = K > 0 with ``ttt_lr``, ``ttt_momentum``, ``ttt_w_pen``, ``ttt_w_con``, ``ttt_prior``,
    ``ttt_keep_best``): every row of a call goes through ``contact.refine_ttt`` -- K steps of SGD with momentum on the 61 parameters
    down the reference's test-time loss (one fused loss-and-gradient kernel and the MANO backward pass per step) -- after any push-out
    and before any scoring or selection, and MANO is posed again, so ``params`` / ``vertices`` are the refined ones and best-of-M ranks
    the refined candidates.  ``ttt_prior``: None (every vertex is a contact target), a ``contact.ContactTargets``, or the path of a
    JSON list of vertex indices (the reference's 204).  The dicts gain ``ttt_loss0``, ``ttt_loss`` [num_grasp] f32 and ``ttt_iter``
    [num_grasp] i32, and the JSON the same three lists (a loss that is not finite: null), through a small copy of their own.  Rows are
    refined independently: the results do not depend on ``rows_per_call``; ``ttt_steps = 0`` is the call without the keyword.  The
    constants are the reference's and untuned here; the effect on real grasps is not measured.

    Mesh depth (``mesh_depth=True``, or a finite ``max_mesh_depth`` together with ``candidates``; both need ``object_meshes``, one
    ``(verts, faces)`` per object in the cloud's own frame): every call packs its objects' meshes (``contact.ObjectMeshes``) and launches
    ONE ``contact.grasp_mesh`` over all its rows with the call's ``obj_of_row``, rotations and offset, after the push-out and the
    gradient refinement.  ``max_mesh_depth`` (cm): candidates whose deepest inside vertex lies farther than that from the mesh's surface
    join class 1 and candidates without a figure class 2 (``contact.mesh_class``), whatever ``select_by`` ranks by.  Each dict gains
    ``mesh`` (n_inside, depth, mask of its grasps; with ``candidates`` also ``mesh_scores``, those of ALL candidates) and ``json`` gains
    "mesh_depth" (cm) and "mesh_interior" per grasp (``contact.mesh_stats``, float64 on the host; null without a figure), "mesh_closed" and
    "mesh_penetration_map" per object.  On an open mesh the figures are undefined; it is not refused.

    Beam search (``beam_width`` = W > 0, ``beam_poses`` = P, P * W = ``candidates`` or ``num_grasp``): nothing is drawn.  Every object
    gets P poses -- the rotations of its first P grasp rows of the call without the keyword; P = 1 without ``rotate`` -- and every pose
    ONE ``GenNet.gen_beam`` search: row p * W + r is the r-th likeliest distinct code grid of pose p under the prior, decoded as
    ``gen`` decodes it.  Push-out, refinement, scores, selection and diversity see ordinary rows.  The dicts and ``json`` gain
    ``log_prob`` (the beam's score), ``beam_pose``, ``beam_rank`` and ``beam_duplicate_of`` (the rank within the pose of the first
    better beam with the same six hand codes, or -1).  Excludes ``temperature`` / ``top_k``; the searches of a call do not depend on
    one another, so the results do not depend on ``rows_per_call``.  fp16 weight images only, no bf16 fallback inside the search;
    whether likelier grids are better grasps is not measured.  ``beam_width = 0`` is the call without the keyword."""
    return _generate_objects(locals())                                             # (first statement: the locals are the keywords)


# the keywords that are 0/1 integers as flags: ``main`` converts them
BOOL_KEYWORDS = frozenset(k for k, p in inspect.signature(generate_for_objects).parameters.items() if isinstance(p.default, bool))


def generate_with_object_contact(net: GenNet, objs: Sequence[torch.Tensor], num_grasp: int, rotate: bool, seed: int,
                                 object_indices: Sequence[int], object_contact_threshold: float = 0.02, **options) -> List[Dict[str, object]]:
    """``generate_for_objects(net, objs, num_grasp, rotate, seed, object_indices, **options)`` with the object-side contact map:
    where on the object its grasps land, at ``object_contact_threshold`` = T metres.  After selection, push-out and refinement every
    call launches ONE ``contact.object_contact`` over the grasps WRITTEN -- all rows of the call, or with ``candidates`` the kept rows
    by their index list against the call's hands and clouds (no gather) -- one segment per object.  Each dict gains
    ``object_contact`` (touch, inside, dmin, near_sum [N], n_valid, row_status [num_grasp] on the device) and ``json`` gains
    "object_contact_map" and "object_interior_map" (N ints: how many of the object's grasps come closer than T to point p / have it
    inside the hand), "object_min_dist" (N floats in cm, null without a valid grasp) and "object_contact" (grasps, coverage, entropy,
    threshold: ``contact.object_contact_stats``, float64 on the host), after every other field.  Index p is point p of the object's
    cloud: a rotation does not permute points.  The maps ride in the call's one device-to-host copy and do not depend on
    ``rows_per_call``; everything else is what ``generate_for_objects`` returns, bit for bit.  A proximity figure at an untuned
    threshold; the effect on real grasps is not measured.  (A function of its own: the keywords of ``generate_for_objects`` are pinned.)"""
    call = inspect.signature(generate_for_objects).bind(net, objs, num_grasp, rotate, seed, object_indices, **options)
    call.apply_defaults()
    return _generate_objects(call.arguments, object_contact_threshold)


def generate_with_volume_mesh(net: GenNet, objs: Sequence[torch.Tensor], num_grasp: int, rotate: bool, seed: int,
                              object_indices: Sequence[int], volume_mesh: int = 0, object_contact_threshold: Optional[float] = None,
                              **options) -> List[Dict[str, object]]:
    """``generate_for_objects(net, objs, num_grasp, rotate, seed, object_indices, **options)`` with the volume figure (``volume=True``
    or a finite ``max_volume``) counted against the objects' MESHES, ``options["object_meshes"]``: the flag ``--volume_mesh`` under its
    own name and default.  0: the call without the keyword -- the hull of each object's cloud, the same bytes, no other launch.
    1: the half-spaces are ``contact.hull_planes`` of each mesh's VERTICES -- the reference's geometry, trimesh.convex.convex_hull of the
    object mesh -- through the same ``contact.grasp_volume``; a hull with more planes than ``contact.pack_planes`` admits raises, naming
    the object.  2: ONE ``contact.grasp_mesh_volume`` per call against the meshes themselves, so that a finger in the hollow of a cup or
    through a handle shares nothing with the object: the solid intersection on the object's own lattice -- not metric/intersect.py's
    figure (trimesh's surface voxels of the object inside the hand), undefined on an open mesh ("mesh_closed" of ``mesh_depth`` reports
    it), and with no igl / trimesh run behind it.  The kernel has no depth: ``volume["depth"]`` is NaN and "penetration_depth" null per
    grasp; ``max_volume`` compares the count as before.  Every call packs its objects' meshes once (``contact.ObjectMeshes``), whether
    or not ``mesh_depth`` asks for them too.  ``object_contact_threshold``: as ``generate_with_object_contact`` takes it, None for no
    map.  The results do not depend on ``rows_per_call``.  (A function of its own: the keywords of ``generate_for_objects`` are pinned.)"""
    call = inspect.signature(generate_for_objects).bind(net, objs, num_grasp, rotate, seed, object_indices, **options)
    call.apply_defaults()
    return _generate_objects(call.arguments, object_contact_threshold, volume_mesh)


def generate_with_closure(net: GenNet, objs: Sequence[torch.Tensor], num_grasp: int, rotate: bool, seed: int,
                          object_indices: Sequence[int], friction: float = 0.5, closure_dirs: int = 256, min_closure: float = float("-inf"),
                          object_contact_threshold: Optional[float] = None, volume_mesh: int = 0, **options) -> List[Dict[str, object]]:
    """``generate_for_objects(net, objs, num_grasp, rotate, seed, object_indices, **options)`` with the force-closure quality of the
    grasps WRITTEN: after push-out and gradient refinement every call launches ONE ``contact.grasp_closure`` over all its rows --
    Coulomb friction ``friction``, ``closure_dirs`` sampled directions (12 .. 1024: ``contact.closure_directions``), the torque length
    of ``options["torque_length"]`` and the scores' 2 cm contact threshold.  ``min_closure`` above -inf (needs ``candidates``):
    candidates whose quality is below it, or that touch nothing, join class 1 and rows with a coordinate that is not finite class 2
    (``contact.closure_class``), whatever ``select_by`` ranks by: a guard only, nothing is ranked by it.  Each dict gains ``closure``
    (quality, worst_dir, status of its grasps; with ``candidates`` also ``closure_scores``, those of ALL candidates) and ``json`` gains
    "closure_quality", "force_closure" and "closure_direction" per grasp (``contact.closure_stats``, float64 on the host; null without
    a figure), after the fields of the other figures.  They ride in the call's one device-to-host copy and do not depend on
    ``rows_per_call``; everything else is what ``generate_for_objects`` returns, bit for bit.  ``object_contact_threshold`` and
    ``volume_mesh``: as ``generate_with_object_contact`` and ``generate_with_volume_mesh`` take them (None / 0: off).  The quality is
    an upper bound of the L1 Ferrari-Canny figure over the sampled directions: <= 0 certifies no force closure, > 0 certifies nothing;
    no physics run, untuned constants, effect on real grasps not measured.  (A function of its own: the keywords of
    ``generate_for_objects`` are pinned.)"""
    call = inspect.signature(generate_for_objects).bind(net, objs, num_grasp, rotate, seed, object_indices, **options)
    call.apply_defaults()
    return _generate_objects(call.arguments, object_contact_threshold, volume_mesh,
                             dict(closure=1, friction=friction, closure_dirs=closure_dirs, min_closure=min_closure))


CLOSURE_OFF = dict(closure=0, friction=0.5, closure_dirs=256, min_closure=-math.inf)   # the flags' defaults


def _generate_objects(keywords, object_contact_threshold: Optional[float] = None, volume_mesh: int = 0,
                      closure: Optional[Dict[str, object]] = None) -> List[Dict[str, object]]:
    """The body of ``generate_for_objects`` -- ``keywords`` are its bound arguments by name -- of ``generate_with_object_contact``,
    which adds the threshold, of ``generate_with_volume_mesh``, which adds its option, and of ``generate_with_closure``, which adds
    its four (``closure``).  Every value check (RULES) comes first and sees no more than the values; then the face list, the tables and
    the files the groups' settings need; then one _Options for all the calls."""
    o = types.SimpleNamespace(**keywords, object_contact=object_contact_threshold is not None, object_contact_threshold=object_contact_threshold,
                              volume_mesh=volume_mesh, **(closure or CLOSURE_OFF))
    extra = [fig for fig in EXTRA_FIGURES if fig.wanted(o)]
    rule = _broken_rule(o, cli=False) or next((r for r in (*CLOSURE_RULES, *VOLUME_MESH_RULES) if not r.ok(o)), None)
    if rule is None and extra and not _TORQUE_LENGTH_RULE.ok(o):                   # (its gate is the stability proxy's: the closure figure reads it too)
        rule = _TORQUE_LENGTH_RULE
    if rule is not None:
        raise RuntimeError("generate_for_objects: " + _rule_message(rule, o, cli=False))
    on = {name: group for name, group in GROUPS.items() if group.wanted(o)}
    if any(group.faces for group in (*on.values(), *extra)):
        _hand_faces(o.net)                                                         # no face list: raise before any work
    settings = {name: group.settings(o, o.net) for name, group in on.items() if group.settings is not None}
    named = {f.name: keywords[f.name] for f in dataclasses.fields(_Options) if f.name in keywords}
    opt = _Options(**{**named, "stability": "stability" in on, "ttt": settings.get("ttt"), "beam": settings.get("beam"),
                      "object_contact": settings.get("object_contact"),
                      "figures": tuple((fig, settings[fig.key]) for fig in FIGURES if fig.key in on)
                                 + tuple((fig, fig.settings(o, o.net)) for fig in extra)})
    out: List[Optional[Dict[str, object]]] = [None] * len(o.objs)
    for call in plan_calls([x.shape[1] for x in o.objs], o.candidates or o.num_grasp, o.rows_per_call):
        # the call's objects' meshes, packed and uploaded once per call
        meshes = contact.ObjectMeshes([o.object_meshes[p] for p in call]) if _Mesh.key in on or o.volume_mesh else None
        res = _generate_call(o.net, opt, [o.objs[p] for p in call], [o.object_indices[p] for p in call], meshes)
        for p, r in zip(call, res):
            out[p] = r
    return out


def _ttt_targets(prior):
    """``ttt_prior`` -> what contact.refine_ttt takes: None (every vertex), a ``contact.ContactTargets`` as given, or the path of a
    JSON list of vertex indices (read once per path)."""
    if prior is None or isinstance(prior, contact.ContactTargets):
        return prior
    key = os.path.abspath(str(prior))
    if key not in _TTT_TARGETS:
        _TTT_TARGETS[key] = contact.ContactTargets.from_json(key)
    return _TTT_TARGETS[key]


_TTT_TARGETS: Dict[str, object] = {}


def _write_summary(out_dir: str, stem: str, rank: int, world: int, stat: Dict[str, object]) -> None:
    """A run summary of ``main``: <stem>.json, or <stem>_rank{rank}.json when several ranks share the run."""
    with open(os.path.join(out_dir, f"{stem}.json" if world == 1 else f"{stem}_rank{rank}.json"), "w") as f:
        json.dump(stat, f)


def _mesh_clouds(meshes, names: Sequence[str], object_indices: Sequence[int], args, device) -> List[tuple]:
    """--mesh_points: the (name, [4,N] tensor) of every mesh of this rank, the clouds sampled on the device in one call -- a cloud's
    bits depend on (seed, its global object index, its mesh) only -- and each written to <out_dir>/obj_cloud_<name>.npy as [N,3]
    float32: the file that ``--objects`` reads back to the same bits."""
    points, _ = contact.sample_clouds(contact.ObjectMeshes(meshes), args.mesh_points, args.seed, object_indices, even=args.mesh_points_even,
                                      device=device)
    clouds = points.cpu().numpy()
    out = []
    for name, cloud in zip(names, clouds):
        np.save(os.path.join(args.out_dir, f"obj_cloud_{name}.npy"), cloud)
        out.append((name, object_tensor(cloud.astype(np.float64))))
    return out


def main(dataset: str, argv: Optional[Sequence[str]] = None) -> List[str]:
    args = parse_args(dataset, argv)
    rank, local_rank, world = dist.init()
    if not torch.cuda.is_available():
        raise RuntimeError("the HIP path needs a GPU: there is no CPU fallback (use the reference on CPU)")
    device = torch.device(args.device) if args.device else torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    torch.manual_seed(args.seed)
    net = load_model(args, device)
    os.makedirs(args.out_dir, exist_ok=True)
    rank_meshes = None                                                             # --mesh_points: this rank's meshes, read once
    if args.mesh_points:
        names = [os.path.splitext(os.path.basename(p))[0] for p in args.object_meshes]
        lo, hi = dist.shard_range(len(names), rank, world)
        rank_meshes = [contact.load_mesh(p) for p in args.object_meshes[lo:hi]]
        objs = [(name, None) for name in names]                                    # (another rank's objects are never looked at)
        if hi > lo:
            objs[lo:hi] = _mesh_clouds(rank_meshes, names[lo:hi], list(range(lo, hi)), args, device)
    elif args.objects:
        objs = [(os.path.splitext(os.path.basename(p))[0], object_tensor(np.load(p).astype(np.float64))) for p in args.objects]
    else:
        clouds = synth.synthetic_clouds(args.num_objects, args.points, seed=args.seed)
        objs = [(f"synthetic_{i}", clouds[i]) for i in range(args.num_objects)]
    written = []
    lo, hi = dist.shard_range(len(objs), rank, world)                              # objects are independent: shard them
    total_t, total_g = 0.0, 0
    wall0 = time.time()
    rotate = DATASETS[dataset]["rotate"]
    if args.diversity and (hi - lo) * args.num_grasp > ops.SEGMENT_KMEANS_MAX_M:
        raise RuntimeError(f"--diversity: the pooled statistic takes at most {ops.SEGMENT_KMEANS_MAX_M} grasps per rank "
                           f"(got {(hi - lo) * args.num_grasp})")
    on = {name: group for name, group in GROUPS.items() if group.wanted(args)}
    extra = [fig for fig in EXTRA_FIGURES if fig.wanted(args)]                     # (no group of GROUPS: their keywords are generate_with_closure's)
    if args.rows_per_call > 0 or on or extra:
        # grouped calls (with any option group always: --rows_per_call 0 is then one object per call).  A group that is on passes its
        # keywords under the flags' names and forces its switch: --max_volume alone is volume=True
        rows_per_call, per_object = max(1, args.rows_per_call), (args.candidates or args.num_grasp)
        flags = {"rows_per_call": rows_per_call, **{k: getattr(args, k) for k in ("temperature", "top_k", "log_prob")}}
        for group in on.values():
            flags.update({k: getattr(args, k) for k in group.keywords}, **({group.switch: True} if group.switch else {}))
        flags = {k: bool(v) if k in BOOL_KEYWORDS else v for k, v in flags.items()}    # the 0/1 flags
        generate_call = generate_with_object_contact if "object_contact" in on else generate_for_objects
        if args.volume_mesh:                                                       # (the threshold, when on, is among the flags)
            generate_call, flags["volume_mesh"] = generate_with_volume_mesh, args.volume_mesh
        if _Closure in extra:                                                      # (it takes the threshold and volume_mesh too)
            generate_call = generate_with_closure
            flags.update({k: getattr(args, k) for k in _Closure.keywords}, torque_length=args.torque_length)
        need_meshes = _Mesh.key in on or bool(args.volume_mesh)
        # this rank's objects' meshes, read once
        meshes = [] if not need_meshes else rank_meshes if rank_meshes is not None else [contact.load_mesh(p) for p in args.object_meshes[lo:hi]]
        active = [fig for fig in FIGURES if fig.key in on] + extra
        fig_rows: Dict[str, Dict[int, object]] = {fig.key: {} for fig in active}   # every object's _Figure.rows, for the run summaries
        curl_rows: Dict[int, tuple] = {}                                           # --refine_curl: every object's (curled, reverted) counts
        kept: Dict[int, np.ndarray] = {}                                           # --diversity: every object's kept parameters, on the host
        omap_rows: Dict[int, Dict[str, object]] = {}                               # --object_contact: every object's "object_contact" entry
        # grouped calls: one call's objects at a time, its files written before the next call starts, so the device and the host
        # hold one call's results, not the whole list's
        mine = objs[lo:hi]
        paths: Dict[int, str] = {}
        for call in plan_calls([o.shape[1] for _, o in mine], per_object, rows_per_call):
            torch.cuda.synchronize(device)
            t0 = time.time()
            outs = generate_call(net, [mine[p][1] for p in call], args.num_grasp, rotate, args.seed, [lo + p for p in call],
                                 **flags, **({"object_meshes": [meshes[p] for p in call]} if need_meshes else {}))
            torch.cuda.synchronize(device)
            dt = time.time() - t0
            total_t += dt
            total_g += args.num_grasp * len(call)
            best_of = f" (the best of {args.candidates * len(call)} candidates)" if args.candidates else ""
            print(f"gen_time: {dt:.4f} s for {args.num_grasp * len(call)} grasps of {len(call)} objects{best_of}")
            for p, out in zip(call, outs):
                paths[p] = os.path.join(args.out_dir, f"obj_id_{mine[p][0]}.json")
                with open(paths[p], "w") as f:
                    json.dump(out["json"], f)
                if args.diversity:
                    kept[p] = np.asarray(out["json"]["recon_params"], dtype=np.float32).reshape(args.num_grasp, -1)
                if args.object_contact:
                    omap_rows[p] = out["json"]["object_contact"]
                if args.refine_curl:
                    curl_rows[p] = (sum(1 for g in out["json"]["refine_curl"] if any(x != 0 for a in g for x in a)),
                                    sum(out["json"]["refine_reverted"]))
                for fig in active:
                    fig_rows[fig.key][p] = fig.rows(out["json"])
            del outs, out
        written = [paths[p] for p in sorted(paths)]                                # object order, whatever the grouping
        if args.diversity and kept:
            # the pooled statistic of all of this rank's kept grasps in object order: one segment, uploaded once
            from . import diversity as dv
            pooled = torch.from_numpy(np.concatenate([kept[p] for p in sorted(kept)])).to(device)
            stat = dv.device_diversity(pooled, 1, pooled.shape[0], cls_num=args.diversity, iters=DIVERSITY_ITERS)[0]
            _write_summary(args.out_dir, "diversity", rank, world,
                           {**{k: stat[k] for k in ("clusters", "entropy", "mean_dist", "iters", "counts")}, "grasps": int(pooled.shape[0])})
            print(f"rank {rank}: diversity of {pooled.shape[0]} grasps in {stat['clusters']} clusters: entropy {stat['entropy']:.4f}, "
                  f"mean distance {stat['mean_dist']:.4f} ({stat['iters']} iterations)")
        if args.object_contact:
            # the run's figures of the object-side contact maps over this rank's objects in object order: exactly rounded sums of
            # per-object figures, so that no grouping can change a bit
            per_obj = [omap_rows[p] for p in sorted(omap_rows)]
            entropies = [d["entropy"] for d in per_obj if d["entropy"] is not None]
            stat = {"threshold": args.object_contact_threshold, "objects": len(per_obj), "grasps": sum(d["grasps"] for d in per_obj),
                    "mean_coverage": _mean([d["coverage"] for d in per_obj]), "mean_entropy": _mean(entropies),
                    "share_untouched": _share([d["entropy"] is None for d in per_obj])}
            _write_summary(args.out_dir, "object_contact", rank, world, stat)
            print(f"rank {rank}: object-side contact of {stat['grasps']} grasps on {stat['objects']} objects at "
                  f"{args.object_contact_threshold} m: mean coverage {stat['mean_coverage']}, mean entropy {stat['mean_entropy']}, "
                  f"share of objects no grasp touches {stat['share_untouched']}")
        if args.refine_curl:
            # the run's metadata of the articulated push-out: the rig's joints (the order of "refine_curl") and two integer counts
            stat = {"joints": _finger_rig(net).joints, "refine_curl": args.refine_curl, "refine_max_curl": args.refine_max_curl,
                    "grasps": args.num_grasp * len(curl_rows), "curled": sum(c for c, _ in curl_rows.values()),
                    "reverted": sum(r for _, r in curl_rows.values())}
            _write_summary(args.out_dir, "refine_curl", rank, world, stat)
            print(f"rank {rank}: articulated push-out of {stat['grasps']} grasps: {stat['curled']} with a curled finger, "
                  f"{stat['reverted']} reverted")
        for fig in active:                                                         # the run's figures over this rank's grasps in object order
            stat, line = fig.summary(args, net, [fig_rows[fig.key][p] for p in sorted(fig_rows[fig.key])])
            _write_summary(args.out_dir, fig.stem, rank, world, stat)
            print(f"rank {rank}: {line}")
    else:
        for gi, (name, obj) in enumerate(objs[lo:hi], start=lo):                   # --rows_per_call 0: one call per object
            torch.cuda.synchronize(device)
            t0 = time.time()
            rng = np.random.default_rng([args.seed, gi])                            # per OBJECT: rotations independent of the sharding
            out = generate_for_object(net, obj, args.num_grasp, rotate, rng, seed=args.seed, object_index=gi,
                                      temperature=args.temperature, top_k=args.top_k, log_prob=bool(args.log_prob))
            torch.cuda.synchronize(device)                                         # the reference times without a sync
            dt = time.time() - t0
            total_t += dt
            total_g += args.num_grasp
            print(f"gen_time: {dt:.4f} s for {args.num_grasp} grasps of {name}")
            path = os.path.join(args.out_dir, f"obj_id_{name}.json")
            with open(path, "w") as f:
                json.dump(out["json"], f)
            written.append(path)
    if total_g:
        print(f"rank {rank}: {total_g} grasps in {total_t:.3f} s ({total_g / max(total_t, 1e-9):.1f} grasps/s incl. first-call packing)")
        wall = time.time() - wall0
        print(f"rank {rank}: wall time {wall:.3f} s incl. JSON writing ({total_g / max(wall, 1e-9):.1f} grasps/s end to end)")
    dist.barrier()                                       # every rank's files are on disk when any rank returns
    if world > 1:
        dist.shutdown()
    return written
