"""Writes tests/golden/pointnet_sampling_ref.npz: what the reference's own HomeworkFinal code returns for the PointNet++ sampling /
grouping operators and for the object normalisation, on inputs DERIVED BY RULE from the committed scan tests/golden/kat_kitti_q5.npz
(derive_inputs below: the tests rebuild the same inputs, so the fixture holds reference OUTPUTS only).

Runs on a CPU (torch + numpy):   python tests/golden/gen_golden_pointnet.py <reference root>
  <reference root>/HomeworkFinal/models/pointnet_util.py       imported as it is (torch only)
  <reference root>/HomeworkFinal/data_utils/DataLoader.py      farthest_point_sample lifted out alone (the module imports open3d-free
  <reference root>/HomeworkFinal/foreground_obj_cls.py         code we do not need, and open3d); pc_normalize likewise
The archive is written with fixed zip time stamps, so the same inputs give the same bytes.
"""
from __future__ import annotations

import ast
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pointnet_sampling_ref.npz")

N_OBJ, OBJ_N = 64, 256           # the model's batch rows: 64 objects of 256 points
N_NBH, NBH_MIN = 30, 257         # ragged neighbourhoods of more than 256 points for the f64 mode
BALL_CASES = ((0.2, 8), (0.4, 16))
SCAN_PREFIX, SCAN_FPS, SCAN_BALL = 32768, 1024, (0.5, 32)
FULL_FPS = 2048
SG_B, SG_NPOINT, SG_RADIUS, SG_NSAMPLE = 4, 16, 0.4, 8


def load_scan():
    return np.ascontiguousarray(np.load(os.path.join(HERE, "kat_kitti_q5.npz"))["db_f32"][:, :3], np.float32)


def derive_inputs(scan):
    """The inputs of every case, from the scan alone (seeded):
    objs [64, 256, 3] f32   axis-aligned 2 m cubes around seeded scan points with at least 300 members: the first 256 members by index,
                            centred on their f64 mean and rounded to f32
    nbhs list of 30 [n, 3] f32, n > 256   axis-aligned 3 m cubes around seeded scan points: all members by index (the scan's own values)
    scan32k [1, 32768, 3], full [1, n, 3]   prefixes of the scan"""
    rng = np.random.default_rng(7)
    objs = []
    while len(objs) < N_OBJ:
        c = scan[rng.integers(len(scan))]
        m = np.flatnonzero((np.abs(scan - c) < 1.0).all(1))
        if m.size >= 300:
            o = scan[m[:OBJ_N]].astype(np.float64)
            objs.append((o - o.mean(0)).astype(np.float32))
    rng = np.random.default_rng(11)
    nbhs = []
    while len(nbhs) < N_NBH:
        c = scan[rng.integers(len(scan))]
        m = np.flatnonzero((np.abs(scan - c) < 1.5).all(1))
        if m.size >= NBH_MIN:
            nbhs.append(scan[m].copy())
    return {"objs": np.stack(objs), "nbhs": nbhs, "scan32k": scan[None, :SCAN_PREFIX].copy(), "full": scan[None].copy()}


def sg_features(objs):
    """the D = 3 feature channel of the sample_and_group case (any deterministic f32 values do)"""
    return (objs[:SG_B] * np.float32(2.0) + np.float32(0.25)).astype(np.float32)


def _lift(path, names):
    ns = {"np": np}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.FunctionDef) and node.name in names:
            exec(compile(ast.Module([node], []), path, "exec"), ns)
    return ns


def _write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main(ref_root):
    import torch
    torch.set_num_threads(8)
    sys.path.insert(0, os.path.join(ref_root, "HomeworkFinal", "models"))
    import pointnet_util as pu
    dl = _lift(os.path.join(ref_root, "HomeworkFinal", "data_utils", "DataLoader.py"), ("farthest_point_sample",))
    fg = _lift(os.path.join(ref_root, "HomeworkFinal", "foreground_obj_cls.py"), ("pc_normalize",))
    inp = derive_inputs(load_scan())
    objs = inp["objs"]
    out = {}

    def fps(x, npoint, seed):
        torch.manual_seed(seed)
        return pu.farthest_point_sample(torch.from_numpy(x), npoint).numpy()          # column 0 is the start the reference drew

    def ball(r, k, x, cent):
        new_xyz = np.stack([x[b][cent[b]] for b in range(x.shape[0])])
        return pu.query_ball_point(r, k, torch.from_numpy(x), torch.from_numpy(new_xyz)).numpy()

    # the model's two layers on the objects (f32 mode)
    l1 = fps(objs, 64, 1)
    out["fps_obj_l1"] = l1.astype(np.uint16)
    xyz1 = np.stack([objs[b][l1[b]] for b in range(N_OBJ)])
    out["fps_obj_l2"] = fps(xyz1, 32, 4).astype(np.uint16)
    for r, k in BALL_CASES:
        out[f"ball_obj_r{r}_k{k}"] = ball(r, k, objs, l1).astype(np.uint16)
    # scan-sized segments
    c2 = fps(inp["scan32k"], SCAN_FPS, 2)
    out["fps_scan32k"] = c2.astype(np.uint32)
    out["ball_scan32k"] = ball(SCAN_BALL[0], SCAN_BALL[1], inp["scan32k"], c2).astype(np.uint16)      # 32768 (an empty row) fits u16
    out["fps_full"] = fps(inp["full"], FULL_FPS, 3).astype(np.uint32)
    # sample_and_group, one small case with features
    torch.manual_seed(5)
    sx = torch.from_numpy(objs[:SG_B])
    new_xyz, new_points, _, fps_idx = pu.sample_and_group(SG_NPOINT, SG_RADIUS, SG_NSAMPLE, sx, torch.from_numpy(sg_features(objs)), returnfps=True)
    out["sg_new_xyz"] = new_xyz.numpy()
    out["sg_new_points"] = new_points.numpy()
    out["sg_fps_idx"] = fps_idx.numpy().astype(np.uint16)
    # f64 mode + normalisation: the path foreground_obj_cls.py:171-183 takes for a cluster of more than 256 points
    starts, picked, normed = [], [], []
    for t, nb in enumerate(inp["nbhs"]):
        pts = nb.astype(np.float64)                     # pcd_preprocessing returns f64
        np.random.seed(t)
        sel = dl["farthest_point_sample"](pts, 256)
        np.random.seed(t)
        starts.append(np.random.randint(0, len(pts)))   # the draw the call above made first
        picked.append(sel.astype(np.float32))           # (the scan's own f32 values: exact)
        normed.append(torch.from_numpy(fg["pc_normalize"](sel)).to(torch.float32).numpy())      # the one rounding of :183
    out["fps64_start"] = np.asarray(starts, np.uint32)
    out["fps64_points"] = np.stack(picked)
    out["obj_normalised"] = np.stack(normed)
    _write_npz(OUT, out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PCR_REFERENCE_ROOT", ""))
