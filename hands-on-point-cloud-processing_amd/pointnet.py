"""HomeworkFinal's PointNet++ sampling / grouping operators and its object extraction, on the GPU.

Mirrors (same names, argument order and return shapes):
  farthest_point_sample   HomeworkFinal/models/pointnet_util.py:66-87     (GPU: pcr_fps_f32, PCR_FPS_F32)
  query_ball_point        HomeworkFinal/models/pointnet_util.py:90-116    (GPU: pcr_ball_query_f32)
  index_points            HomeworkFinal/models/pointnet_util.py:46-63     (host indexing: it is a gather of a few KB)
  sample_and_group        HomeworkFinal/models/pointnet_util.py:119-156   (GPU: the three operators, one fused gather)
  classify_foreground_objects   the flow of HomeworkFinal/foreground_obj_cls.py:97-180 up to the classifier's input

The functions take [B, N, C] numpy arrays or torch tensors and return the same kind (indices as int64, like the reference).  Torch is
plumbing here: a tensor is brought to the host, the library works on its own device cloud, and the result is put back on the tensor's
device — one host round trip per call, no zero-copy hand-over.  There is no CPU fallback: without the library or a GPU a call raises.

What is unpinned: the reference draws the first FPS pick unseeded (torch.randint); pass `start=` to fix it, else it is drawn from
np.random.  Written from the contracts in include/pcr.h.
"""
from __future__ import annotations

import numpy as np

from . import PCR_AOS3, PCR_FPS_F32


def _ctx(ctx):
    if ctx is not None:
        return ctx
    from .hw4 import default_context
    return default_context()


def _to_host(a):
    """-> (numpy array, None) or (numpy array, the torch tensor it came from)"""
    if isinstance(a, np.ndarray) or a is None:
        return a, None
    if hasattr(a, "detach") and hasattr(a, "cpu"):
        return a.detach().cpu().numpy(), a
    return np.asarray(a), None


def _like(out, proto, integer=False):
    if proto is None:
        return out
    import torch
    t = torch.from_numpy(np.ascontiguousarray(out))
    return t.to(proto.device) if integer else t.to(device=proto.device, dtype=proto.dtype)


def _batch_cloud(ctx, xyz):
    """[B, N, 3] -> (device cloud of B * N points, seg_ptr)"""
    B, N = xyz.shape[0], xyz.shape[1]
    cloud = ctx.cloud(np.ascontiguousarray(xyz[..., :3], np.float32).reshape(B * N, 3), PCR_AOS3)
    return cloud, (np.arange(B + 1, dtype=np.int64) * N).astype(np.uint32)


def farthest_point_sample(xyz, npoint, start=None, *, ctx=None, mode=PCR_FPS_F32):
    """[B, N, 3] -> indices [B, npoint] (int64).  start: [B] first picks; None draws them as the reference does (unseeded)."""
    x, proto = _to_host(xyz)
    B, N = x.shape[0], x.shape[1]
    st, _ = _to_host(start)
    if st is None:
        st = np.random.randint(0, N, size=B)
    ctx = _ctx(ctx)
    cloud, seg = _batch_cloud(ctx, x)
    try:
        idx = ctx.fps(cloud, seg, int(npoint), np.asarray(st).reshape(B), mode)
    finally:
        cloud.free()
    return _like(idx.astype(np.int64), proto, integer=True)


def query_ball_point(radius, nsample, xyz, new_xyz, *, ctx=None):
    """xyz [B, N, 3], new_xyz [B, S, 3] -> group_idx [B, S, nsample] (int64); a row without a point in the ball holds N."""
    x, proto = _to_host(xyz)
    q, _ = _to_host(new_xyz)
    B, S = q.shape[0], q.shape[1]
    ctx = _ctx(ctx)
    cloud, seg = _batch_cloud(ctx, x)
    centres, cseg = _batch_cloud(ctx, q)
    try:
        idx, _ = ctx.ball_query(cloud, seg, centres, cseg, radius, int(nsample))
    finally:
        cloud.free()
        centres.free()
    return _like(idx.astype(np.int64).reshape(B, S, int(nsample)), proto, integer=True)


def index_points(points, idx):
    """points [B, N, C], idx [B, S] or [B, S, K] -> points gathered per batch row, [B, S, C] or [B, S, K, C]."""
    p, proto = _to_host(points)
    i, _ = _to_host(idx)
    i = np.asarray(i, np.int64)
    b = np.arange(p.shape[0]).reshape((-1,) + (1,) * (i.ndim - 1))
    return _like(p[b, i, :], proto)


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, *, start=None, ctx=None):
    """xyz [B, N, 3], points [B, N, D] or None -> (new_xyz [B, npoint, 3], new_points [B, npoint, nsample, 3 + D]) and, with
    returnfps, also (grouped_xyz [B, npoint, nsample, 3], fps_idx [B, npoint]).  The cloud is uploaded once for the three operators."""
    x, proto = _to_host(xyz)
    f, _ = _to_host(points)
    B, N = x.shape[0], x.shape[1]
    S, K = int(npoint), int(nsample)
    st, _ = _to_host(start)
    if st is None:
        st = np.random.randint(0, N, size=B)
    ctx = _ctx(ctx)
    cloud, seg = _batch_cloud(ctx, x)
    centres = None
    try:
        fps_idx = ctx.fps(cloud, seg, S, np.asarray(st).reshape(B), PCR_FPS_F32)
        flat = np.ascontiguousarray(x[..., :3], np.float32).reshape(B * N, 3)
        cpos = (fps_idx.astype(np.int64) + (np.arange(B, dtype=np.int64) * N)[:, None]).reshape(-1)
        centres = ctx.cloud(flat[cpos], PCR_AOS3)
        cseg = (np.arange(B + 1, dtype=np.int64) * S).astype(np.uint32)
        idx, _ = ctx.ball_query(cloud, seg, centres, cseg, radius, K)
        feat = None if f is None else np.ascontiguousarray(f, np.float32).reshape(B * N, -1)
        new_xyz, new_points = ctx.group_points(cloud, seg, centres, cseg, idx, feat)
    finally:
        cloud.free()
        if centres is not None:
            centres.free()
    new_xyz = new_xyz.reshape(B, S, 3)
    new_points = new_points.reshape(B, S, K, -1)
    if not returnfps:
        return _like(new_xyz, proto), _like(new_points, proto)
    grouped_xyz = x[np.arange(B)[:, None, None], idx.astype(np.int64).reshape(B, S, K), :3].astype(np.float32)
    return _like(new_xyz, proto), _like(new_points, proto), _like(grouped_xyz, proto), _like(fps_idx.astype(np.int64), proto, integer=True)


def classify_foreground_objects(points, npoints=256, eps=0.5, min_points=8, z_min_above_ground=0.5, z_extent=(1.0, 2.3), seed=0, *, ctx=None,
                                preprocess=True):
    """foreground_obj_cls.py:97-180 without the classifier (the reference ships no weights; the classifier stays the caller's):
    pcd_preprocessing -> ground_detection_on3segs -> ground_z = mean z of the ground -> cluster_dbscan(eps, min_points) on the foreground
    -> objects_from_labels.  points: (N, >= 3) scan rows.  Returns (objects f32 [n_obj, npoints, 3], codes i32 [n_clusters]: 3 where the
    reference writes 3, -1 = to be classified) and a dict with everything in between (points, ground / foreground indices, ground_z,
    labels, n_clusters, and the outputs of Context.objects_from_labels)."""
    from . import hw4
    ctx = _ctx(ctx)
    pts = np.asarray(points)[:, :3]
    pts = hw4.pcd_preprocessing(pts, ctx=ctx) if preprocess else np.asarray(pts, np.float64)
    ground_idx, foreground_idx = hw4.ground_detection_on3segs(pts, ctx=ctx)
    ground_z = float(np.mean(pts[ground_idx, 2])) if ground_idx.size else 0.0
    fg = np.ascontiguousarray(pts[foreground_idx], np.float32)
    cloud = ctx.cloud(fg, PCR_AOS3)
    try:
        labels, _, _, n_clusters = ctx.dbscan(cloud, eps, min_points)
        res = ctx.objects_from_labels(cloud, labels, n_clusters, npoints, ground_z, z_min_above_ground, z_extent, seed)
    finally:
        cloud.free()
    res.update(points=pts, ground_idx=ground_idx, foreground_idx=foreground_idx, ground_z=ground_z, labels=labels, n_clusters=n_clusters)
    return res["objects"], res["codes"], res
