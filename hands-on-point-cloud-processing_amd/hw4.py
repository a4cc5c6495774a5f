"""Host-side mirror of the Homework4 RANSAC ground-plane interface, running the inlier counts on the GPU.

Mirrors (same names, argument meaning and return values):
  estimate_plane_params   Homework4/ground_detection_ransac.py:158-169   (host, f64; 3 points)
  my_ransac               Homework4/ground_detection_ransac.py:104-155
  ransac_on_segments      Homework4/ground_detection_ransac.py:54-73
  ransac_on_segments_v2   Homework4/ground_detection_ransac.py:76-101
  extract_initial_seeds   Homework4/ground_detection_SVD.py:46-71        (GPU: radix-select of the lowest z, pcr_ground_seeds_f64)
  ground_detection        Homework4/ground_detection_SVD.py:88-101       (GPU: pcr_ground_detection_f64, PCA refit loop)
  ground_detection_on3segs  Homework4/ground_detection_SVD.py:104-126
  pcd_preprocessing       Homework4/ground_detection_SVD.py:22-37        (GPU: y crop on the host, pcr_statistical_outlier_f32)
  cluster_dbscan          open3d PointCloud.cluster_dbscan, ground_detection_SVD.py:173   (GPU: pcr_dbscan_f32)
  pcd_to_range_image      Homework4/foreground_clustering_range.py:13-48   (GPU: pcr_range_image_create_f32; :34 restated with atan2)
  range_image_labeling    Homework4/foreground_clustering_range.py:51-95   (GPU: pcr_range_image_label_f64; all connected components)
  cluster_assignment      Homework4/foreground_clustering_range.py:124-133 (GPU: pcr_range_image_assign)
  depth_completion        Homework4/foreground_clustering_range.py:136-149 (GPU: pcr_range_image_close_f64)
  cluster_range_image     Homework4/foreground_clustering_range.py:164-167 (__main__'s three calls at once: pcr_range_cluster_f32)

The hot loop of my_ransac — `dists = |[X 1] . params|; inliers = sum(dists < thr)` evaluated once per hypothesis
(:138-139) — becomes ONE launch of pcr_plane_count_f64 over all `max_iteration` hypotheses: the points are read
from HBM once instead of `max_iteration` times.  The final inlier mask (:152-153) is pcr_plane_mask_f64.

Call signatures are the reference's, positionally: `my_ransac(data, indices, max_iteration, threshold)`,
`ransac_on_segments(data, segment_x=0, max_iteration=40, threshold=0.15)`, `ground_segmentation(data)`, ... — a caller written
against ground_detection_ransac.py / ground_detection_SVD.py runs unchanged (tests/test_hw4_gpu.py calls them exactly as
ground_detection_ransac.py:42-73 does).  Two keyword-only extras exist on every function that reaches the GPU:
  ctx=  a pcr Context; default: one lazily created module-level context on device $PCR_DEVICE (default 0) — no CPU fallback;
  rng=  the reference draws its 3-point samples from a fresh, unseeded `np.random.default_rng()` per iteration (:132); an
        explicit generator makes runs reproducible (and equal to the reference's for an identical sample sequence).
"""
from __future__ import annotations

import math
import os
import struct

import numpy as np

_default_ctx = None


def default_context():
    """The module-level context the reference-signature calls run on (created on first use; raises without an MI355X)."""
    global _default_ctx
    if _default_ctx is None or not _default_ctx.h:
        from . import Context
        _default_ctx = Context(int(os.environ.get("PCR_DEVICE", "0")))
    return _default_ctx


def set_default_context(ctx):
    """Use `ctx` for every call that does not name one (None: drop it; the next call creates a fresh one)."""
    global _default_ctx
    _default_ctx = ctx


def read_velodyne_bin(path):
    """ground_detection_ransac.py:23-34: KITTI .bin (N x 4 f32) -> N x 3 float32 array (x, y, z)."""
    with open(path, "rb") as f:
        content = f.read()
    n = len(content) // struct.calcsize("ffff")        # iter_unpack raises on a ragged tail; the files are whole rows
    return np.frombuffer(content, dtype=np.float32, count=4 * n).reshape(n, 4)[:, :3].copy()


def estimate_plane_params(selected_points: np.ndarray) -> np.ndarray:
    """Plane (a, b, c, d)/|n| through 3 points — ground_detection_ransac.py:158-169."""
    p = np.asarray(selected_points)
    vector1 = p[1, :] - p[0, :]
    vector2 = p[2, :] - p[0, :]
    a = (vector1[1] * vector2[2]) - (vector1[2] * vector2[1])
    b = (vector1[2] * vector2[0]) - (vector1[0] * vector2[2])
    c = (vector1[0] * vector2[1]) - (vector1[1] * vector2[0])
    d = -(a * p[0, 0] + b * p[0, 1] + c * p[0, 2])
    n = math.sqrt(a ** 2 + b ** 2 + c ** 2)
    return np.array([a / n, b / n, c / n, d / n])


def extract_initial_seeds(pcd_points: np.ndarray, LPR_size: int, threshold_seeds: float, *, ctx=None) -> np.ndarray:
    """ground_detection_SVD.py:46-71: the points below z_high whose z is below LPR.z + threshold_seeds (input order kept).
    The selection of the LPR_size lowest z runs on the GPU (pcr_ground_seeds_f64)."""
    if pcd_points.shape[0] == 0:
        return pcd_points[:0]
    ctx = ctx or default_context()
    cloud = ctx.cloud(np.ascontiguousarray(pcd_points[:, :3], np.float32), 1)
    try:
        mask, _ = ctx.ground_seeds(cloud, LPR_size, threshold_seeds)
    finally:
        cloud.free()
    return pcd_points[mask, :]


def ground_detection(pcd_points: np.ndarray, pcd_indices: np.ndarray, max_iter: int, LPR_size: int, threshold_dist: float, *, ctx=None,
                     return_params: bool = False):
    """ground_detection_SVD.py:88-101 -> (seeds, ground indices, foreground indices), the reference's 3-tuple; the plane the
    reference prints (:100) is appended as a 4th value with return_params=True."""
    ctx = ctx or default_context()
    cloud = ctx.cloud(np.ascontiguousarray(pcd_points[:, :3], np.float32), 1)
    try:
        params, inliers_filter = ctx.ground_detection(cloud, max_iter, LPR_size, threshold_dist)
    finally:
        cloud.free()
    out = (pcd_points[inliers_filter], pcd_indices[inliers_filter], pcd_indices[np.logical_not(inliers_filter)])
    return out + (params,) if return_params else out


def ground_detection_on3segs(pcd_points: np.ndarray, main_dist=20, max_iter=6, threshold_dist=0.18, *, ctx=None):
    """ground_detection_SVD.py:104-126: three x-segments [x_min, -main_dist, main_dist, x_max], open intervals as written."""
    ctx = ctx or default_context()
    x_min, x_max = np.min(pcd_points[:, 0]), np.max(pcd_points[:, 0])
    segments_x = [x_min, -main_dist, main_dist, x_max]
    total_indices = np.array(range(pcd_points.shape[0]))
    stacked_ground_idx = np.empty(0, dtype=int)
    stacked_foregr_idx = np.empty(0, dtype=int)
    for i in range(len(segments_x) - 1):
        range_filter = np.logical_and(pcd_points[:, 0] < segments_x[i + 1], pcd_points[:, 0] > segments_x[i])
        if not range_filter.any():
            continue                                                    # the reference would fail on an empty segment
        _, ground, foreground = ground_detection(pcd_points[range_filter], total_indices[range_filter], max_iter,
                                                 LPR_size=10000, threshold_dist=threshold_dist, ctx=ctx)
        stacked_ground_idx = np.r_[stacked_ground_idx, ground]
        stacked_foregr_idx = np.r_[stacked_foregr_idx, foreground]
    return stacked_ground_idx, stacked_foregr_idx


def pcd_preprocessing(data, *, ctx=None) -> np.ndarray:
    """ground_detection_SVD.py:22-37: keep -15 < y < 30, then remove_statistical_outlier(nb_neighbors=20, std_ratio=2.7) ->
    the kept points as an f64 (N, 3) array in input order, as the reference returns them."""
    data = np.asarray(data)
    data = data[np.logical_and(data[:, 1] < 30, data[:, 1] > -15)]
    ctx = ctx or default_context()
    cloud = ctx.cloud(np.ascontiguousarray(data[:, :3], np.float32), 1)
    try:
        _, _, _, kept = ctx.statistical_outlier(cloud, 20, 2.7)
    finally:
        cloud.free()
    try:
        return kept.numpy().T.astype(np.float64)
    finally:
        kept.free()


def cluster_dbscan(points, eps, min_points, print_progress=False, *, ctx=None) -> np.ndarray:
    """open3d PointCloud.cluster_dbscan(eps, min_points, print_progress) on an (N, 3) array -> int32 labels, -1 = noise
    (ground_detection_SVD.py:173).  Labels follow pcr_dbscan_f32: sklearn.cluster.DBSCAN's; Open3D's are unpinned.
    print_progress is accepted for the signature and ignored."""
    pts = np.asarray(points)
    ctx = ctx or default_context()
    cloud = ctx.cloud(np.ascontiguousarray(pts[:, :3], np.float32), 1)
    try:
        labels, _, _, _ = ctx.dbscan(cloud, eps, min_points)
    finally:
        cloud.free()
    return labels


class IdxImage:
    """The reference's idx_image (foreground_clustering_range.py:29, :39): `.shape`, and `[r, c]` -> None for a pixel without a point, else
    the object array [None, i, ...] of the pixel's point indices, ascending.  Built lazily from the per-point pixels; keeps the
    device-resident image alive for range_image_labeling and cluster_assignment."""

    def __init__(self, handle, image, pixels):
        self.handle, self.image, self.pixels = handle, image, pixels
        self.shape = image.shape
        self.last_label = None
        self._order = self._start = None

    def __getitem__(self, rc):
        r, c = rc
        rows, cols = self.shape
        r, c = (r + rows if r < 0 else r), (c + cols if c < 0 else c)
        if not (0 <= r < rows and 0 <= c < cols):
            raise IndexError(f"index {rc} is out of bounds for shape {self.shape}")
        if self._order is None:
            self._order = np.argsort(self.pixels, kind="stable")                  # ascending point index inside a pixel
            self._start = np.searchsorted(self.pixels[self._order], np.arange(rows * cols + 1))
        p = r * cols + c
        members = self._order[self._start[p]:self._start[p + 1]]
        if members.size == 0:
            return None
        out = np.empty(members.size + 1, dtype=object)                           # np.append(None, i), repeated (:39)
        out[0] = None
        out[1:] = [int(i) for i in members]
        return out


def pcd_to_range_image(pcd_points, resolution, *, ctx=None):
    """foreground_clustering_range.py:13-48 -> (range_image f64, idx_image, d).  :34 (math.asin with two arguments: TypeError) is
    restated as atan2(z, sqrt(x*x + y*y)); a point the reference would raise IndexError on is dropped (in no pixel, label -1).  The
    points are taken as float32, the precision of the scans pcd_preprocessing returns widened."""
    pts = np.ascontiguousarray(np.asarray(pcd_points)[:, :3], np.float32)
    ctx = ctx or default_context()
    cloud = ctx.cloud(pts, 1)
    try:
        handle = ctx.range_image(cloud, resolution)
    finally:
        cloud.free()
    image = handle.image()
    return image, IdxImage(handle, image, handle.pixels()), np.linalg.norm(pts.astype(np.float64), axis=1)


def _same_array(a, b):
    return a is b or (isinstance(a, np.ndarray) and a.shape == b.shape and np.array_equal(a, b, equal_nan=True))


def range_image_labeling(range_image, idx_image, depth_list, phi, theta, nn_mode, *, ctx=None):
    """foreground_clustering_range.py:51-95 -> image_label (int32, -1 = no label): every connected component of the reference's
    neighbour test, numbered by its first pixel in raster order (pcr_range_image_label_f64 says how the reference's own flood fill
    relates to that).  idx_image and depth_list are unused there too (:82-85 are commented out)."""
    img = np.asarray(range_image, np.float64)
    if isinstance(idx_image, IdxImage) and idx_image.handle.h and _same_array(img, idx_image.image):
        label, _ = idx_image.handle.label(phi, theta, nn_mode)                  # the labels stay on the device for cluster_assignment
        idx_image.last_label = label
        return label
    handle = (ctx or default_context()).range_image_from_host(img)              # e.g. the image depth_completion returned
    try:
        return handle.label(phi, theta, nn_mode)[0]
    finally:
        handle.free()


def cluster_assignment(idx_image, image_label, pcd_size):
    """foreground_clustering_range.py:124-133 -> cluster_idx[pcd_size]: every point takes its pixel's label."""
    assert idx_image.shape == image_label.shape
    if idx_image.last_label is not None and idx_image.handle.h and _same_array(image_label, idx_image.last_label):
        out = idx_image.handle.assign()
    else:                                                                       # labels the device does not hold: a host gather
        pix = idx_image.pixels
        out = np.where(pix >= 0, np.asarray(image_label).reshape(-1)[np.maximum(pix, 0)], -1).astype(np.int32)
    cluster_idx = np.full(pcd_size, -1, dtype=np.int32)
    cluster_idx[:out.size] = out[:pcd_size]
    return cluster_idx


def depth_completion(image, pad, *, ctx=None):
    """foreground_clustering_range.py:136-149: dilation then erosion with a (2 pad + 1)^2 window, the pad border left at -1."""
    handle = (ctx or default_context()).range_image_from_host(np.asarray(image, np.float64))
    try:
        handle.close_gaps(pad)
        return handle.image()
    finally:
        handle.free()


def cluster_range_image(points, resolution=0.7, theta=30, nn_mode=7, *, ctx=None) -> np.ndarray:
    """foreground_clustering_range.py:164-167 in one call (phi = resolution, as there) -> cluster_idx int32, -1 = no cluster."""
    pts = np.ascontiguousarray(np.asarray(points)[:, :3], np.float32)
    ctx = ctx or default_context()
    cloud = ctx.cloud(pts, 1)
    try:
        return ctx.range_cluster(cloud, resolution, theta, nn_mode)[0]
    finally:
        cloud.free()


def my_ransac(data: np.ndarray, indices: np.ndarray, max_iteration: int, threshold: float, *, ctx=None, rng=None):
    """ground_detection_ransac.py:104-155 -> (inliers_idx, best_model_params)."""
    assert data.shape[0] == indices.shape[0]
    ctx = ctx or default_context()
    rng = np.random.default_rng() if rng is None else rng
    filtered_data = extract_initial_seeds(data, 40000, 1, ctx=ctx)              # :125
    if filtered_data.shape[0] < 3:
        return indices[:0], []
    hyps = np.zeros((max_iteration, 4), np.float64)
    for it in range(max_iteration):                                             # :131-135
        sel = rng.choice(filtered_data.shape[0], 3, replace=False)          # same draw as choice(range(n), ...) without building the list
        hyps[it] = estimate_plane_params(filtered_data[sel, :].astype(np.float64))
    valid = np.isfinite(hyps).all(axis=1)       # collinear samples give n = 0 -> NaN params; NaN < thr is False (:139)
    seeds = ctx.cloud(np.ascontiguousarray(filtered_data[:, :3], np.float32), 1)
    try:
        counts = np.zeros(max_iteration, np.int64)
        if valid.any():
            counts[valid] = ctx.plane_count(seeds, hyps[valid], float(threshold))   # :138-139, all hypotheses at once
    finally:
        seeds.free()
    best_set_size, best_model_params = 0, []
    for it in range(max_iteration):                                             # :140-142 (strict >: first maximum wins)
        if counts[it] > best_set_size:
            best_set_size = counts[it]
            best_model_params = hyps[it]
    if len(best_model_params) == 0:
        return indices[:0], []
    allpts = ctx.cloud(np.ascontiguousarray(data[:, :3], np.float32), 1)
    try:
        mask, _ = ctx.plane_mask(allpts, best_model_params, float(threshold))   # :152-153
    finally:
        allpts.free()
    return indices[mask.astype(bool)], best_model_params


def ground_segmentation(data, *, ctx=None, rng=None):
    """ground_detection_ransac.py:42-51: indices of the ground points of one full scan (prints what the reference prints)."""
    ground_indices = ransac_on_segments(data, ctx=ctx, rng=rng)
    print('origin data points num:', data.shape[0])
    print('segmented data points num:', ground_indices.shape[0])
    return ground_indices


def ransac_on_segments(data: np.ndarray, segment_x=0, max_iteration=40, threshold=0.15, *, ctx=None, rng=None):
    """ground_detection_ransac.py:54-73: RANSAC on the two x-segments, stacked inlier indices."""
    ctx = ctx or default_context()
    total = np.array(range(data.shape[0]))
    fwd = data[:, 0] >= segment_x
    idx1, _ = my_ransac(data[fwd], total[fwd], max_iteration, threshold, ctx=ctx, rng=rng)
    idx2, _ = my_ransac(data[np.logical_not(fwd)], total[np.logical_not(fwd)], max_iteration, threshold, ctx=ctx, rng=rng)
    return np.r_[idx1, idx2]


def ransac_on_segments_v2(data: np.ndarray, segments_num=5, max_iteration=40, threshold=0.15, *, ctx=None, rng=None):
    """ground_detection_ransac.py:76-101: RANSAC on `segments_num` uniform x-segments (open intervals, as written)."""
    ctx = ctx or default_context()
    total = np.array(range(data.shape[0]))
    x_min, x_max = np.min(data[:, 0]), np.max(data[:, 0])
    seg_bound = x_min + np.array(range(segments_num + 1)) * ((x_max - x_min) / segments_num)
    stacked = np.empty(0, dtype=int)
    for i in range(segments_num):
        flt = np.logical_and(data[:, 0] < seg_bound[i + 1], data[:, 0] > seg_bound[i])
        if not flt.any():
            continue
        idx, _ = my_ransac(data[flt], total[flt], max_iteration, threshold, ctx=ctx, rng=rng)
        if idx is None:
            continue
        stacked = np.r_[stacked, idx]
    return stacked
