"""HomeworkFinal's two ends on the GPU: the data set build (KITTI files -> instance files) and the labelled boxes behind the classifier.

Mirrors (same names, argument order and return values):
  raw_kitti_bin_reader      HomeworkFinal/dataset_building/dataset_build.py:16-17
  bbox_reader               dataset_build.py:54-75        (host: the label and calibration text, the reference's dtypes)
  get_points_idx_in_bbox    dataset_build.py:97-125       (GPU: pcr_points_in_boxes_f64, one box)
  get_objects_idx_dict      dataset_build.py:78-94        (GPU: pcr_points_in_boxes_f64, ONE call for all boxes of the frame)
  pcd_preprocessing         dataset_building/ground_detection_SVD.py:13-28   (GPU: pcr_statistical_outlier_f32 at (20, 1.5))
  ground_detection_on3segs  ground_detection_SVD.py:101-129                  (GPU: pcr_ground_detection_f64 per x-segment)
  build_frame               the body of build()'s loop, dataset_build.py:172-241, without the files
  build                     dataset_build.py:155-241      (the same directories and array('f').tofile bytes)
  get_mean_hwl              dataset_build.py:419-449
  object_bounding_boxes     HomeworkFinal/foreground_obj_cls.py:190-199      (GPU: pcr_label_aabb_f32)

Every function that reaches the GPU takes the keyword-only ctx= of hw4.py (default: the module-level context; no CPU fallback).
build_frame calls the stages through this module's own names, so a caller (or a test) that replaces one of them replaces that stage.

What is unpinned: DBSCAN's cluster numbering against Open3D's (include/pcr.h), and with it which clusters the `% 8` rule keeps.
Not mirrored: data_augmentation and generate_train_test_split_file (unseeded draws, os.listdir order) and every viewer.
"""
from __future__ import annotations

import linecache
import math
import os
from array import array

import numpy as np

from . import PCR_AOS3
from .hw4 import cluster_dbscan, default_context

CLASS_NAMES = ["Car", "Pedestrian", "Cyclist"]


def raw_kitti_bin_reader(path, file_name):
    """dataset_build.py:16-17: <path><file_name>.bin -> (N, 4) f32 rows (x, y, z, reflectance)."""
    return np.fromfile(path + file_name + ".bin", dtype=np.float32, count=-1).reshape(-1, 4)


def bbox_reader(label_path, calib_path, file_name):
    """dataset_build.py:54-75 -> {class: [(bbox_center f32[3], bbox_front f64[3], hwl f32[3]), ...]} for Car / Pedestrian / Cyclist, in label
    order; every other class is ignored.  Tr_velo_to_cam is line 6 of the calibration file, read as f32; the lidar frame is reached through
    its transpose (the inverse of a rotation) as the reference does."""
    Tr = np.array(linecache.getline(calib_path + file_name + ".txt", 6).split()[1:], dtype=np.float32).reshape(3, 4)
    R_inv = Tr[:, 0:3].transpose()
    t_inv = - R_inv.dot(Tr[:, 3])
    bbox_dict = {cls: [] for cls in CLASS_NAMES}
    with open(label_path + file_name + ".txt", "r") as f:
        for raw in f:
            line = raw.split()
            if len(line) == 0:
                break                                                          # the reference stops at the first blank line
            if line[0] not in bbox_dict:
                continue
            hwl = np.array(line[8:11], dtype=np.float32)
            theta_y = float(line[-1])
            bbox_center_camera = np.array(line[-4:-1], dtype=np.float32)
            half_l = hwl[2] / 2                                                # f32; the products below are f64 (np.cos of a Python float)
            bbox_front_camera = bbox_center_camera + [half_l * np.cos(-theta_y), 0, half_l * np.sin(-theta_y)]
            bbox_center = R_inv.dot(bbox_center_camera) + t_inv
            bbox_front = R_inv.dot(bbox_front_camera) + t_inv
            bbox_dict[line[0]].append((bbox_center, bbox_front, hwl))
    return bbox_dict


def bbox_to_obox(bbox_params):
    """(bbox_center, bbox_front, hwl) -> (center f64[3], R f64[3, 3], extent [3]) exactly as dataset_build.py:113-120 forms them: the centre
    lifted by h / 2, a rotation about z by atan2 of the heading, and the box widened to (1.15 l, 1.25 w, h)."""
    bbox_center, bbox_front, hwl = bbox_params
    orient_vec = bbox_front - bbox_center
    h, w, l = hwl[0], hwl[1], hwl[2]
    center = bbox_center + [0, 0, h / 2]
    theta_z_lidar = math.atan2(orient_vec[1], orient_vec[0])
    R = np.array([[np.cos(theta_z_lidar), - np.sin(theta_z_lidar), 0],
                  [np.sin(theta_z_lidar), np.cos(theta_z_lidar), 0],
                  [0, 0, 1]])
    extent = [1.15 * l, 1.25 * w, h]
    return center, R, extent


def obox_rows(oboxes):
    """[(center, R, extent)] -> the [n, 15] f64 rows Context.points_in_boxes takes (what Open3D's f64 box holds)."""
    out = np.zeros((len(oboxes), 15), np.float64)
    for k, (c, R, e) in enumerate(oboxes):
        out[k, 0:3] = np.asarray(c, np.float64)
        out[k, 3:12] = np.asarray(R, np.float64).reshape(9)
        out[k, 12:15] = np.asarray(e, np.float64)
    return out


def _bbox_8_pts(bbox_params):
    """dataset_build.py:103-111: the four corners of the label's own (l, w) rectangle at the bottom, then the same lifted by h."""
    bbox_center, bbox_front, hwl = bbox_params
    orient_vec = bbox_front - bbox_center
    normal = np.array([orient_vec[1], -orient_vec[0], 0])
    normal = hwl[1] / (2 * np.linalg.norm(normal)) * normal
    back = 2 * bbox_center - bbox_front
    quad = np.array([bbox_front + normal, bbox_front - normal, back + normal, back - normal])
    return np.vstack((quad, quad + [0, 0, hwl[0]]))


def _rows_in_boxes(points, oboxes, ctx):
    """one library call: the points of `points` inside each box -> (a list of int64 index arrays, ascending; hits u32 per point)"""
    pts = np.ascontiguousarray(np.asarray(points)[:, :3], np.float32)
    ctx = ctx or default_context()
    cloud = ctx.cloud(pts, PCR_AOS3)
    try:
        row_ptr, idx, hits = ctx.points_in_boxes(cloud, [0, pts.shape[0]], obox_rows(oboxes), [0, len(oboxes)])
    finally:
        cloud.free()
    rp = row_ptr.astype(np.int64)
    return [idx[rp[b]:rp[b + 1]].astype(np.int64) for b in range(len(oboxes))], hits


def get_points_idx_in_bbox(points, bbox_params, get_8_pts=False, *, ctx=None):
    """dataset_build.py:97-125 -> (indices of the points inside the widened box, ascending; the 8 corner points or None)."""
    rows, _ = _rows_in_boxes(points, [bbox_to_obox(bbox_params)], ctx)
    return rows[0], (_bbox_8_pts(bbox_params) if get_8_pts else None)


def get_objects_idx_dict(points, bbox_dict, get_8_pts=False, *, ctx=None, return_hits=False):
    """dataset_build.py:78-94 -> ({class: [indices per box]}, the corner points of all boxes stacked or None).  All boxes of the frame go
    through ONE library call.  return_hits=True appends the per-point box count (0 = a point of other_obj_idx)."""
    points_idx_dict = {cls: [] for cls in CLASS_NAMES}
    order = [(cls, bbox_params) for cls in bbox_dict for bbox_params in bbox_dict[cls]]
    rows, hits = _rows_in_boxes(points, [bbox_to_obox(p) for _, p in order], ctx)
    for (cls, _), idx in zip(order, rows):
        points_idx_dict[cls].append(idx)
    bbox_points = None
    if get_8_pts:
        bbox_points = np.empty((0, 3))
        for _, p in order:
            bbox_points = np.append(bbox_points, _bbox_8_pts(p), axis=0)
    return (points_idx_dict, bbox_points, hits) if return_hits else (points_idx_dict, bbox_points)


def pcd_preprocessing(data, match_image_range=False, *, ctx=None):
    """ground_detection_SVD.py:13-28: x > 5 (with match_image_range), then -15 < y < 30, then remove_statistical_outlier(20, 1.5) — this
    file's ratio, not Homework4's 2.7 -> the kept points as an f64 (N, 3) array in input order."""
    data = np.asarray(data)
    if match_image_range:
        data = data[data[:, 0] > 5]
    data = data[np.logical_and(data[:, 1] < 30, data[:, 1] > -15)]
    if data.shape[0] == 0:
        return np.zeros((0, 3), np.float64)
    ctx = ctx or default_context()
    cloud = ctx.cloud(np.ascontiguousarray(data[:, :3], np.float32), PCR_AOS3)
    try:
        _, _, _, kept = ctx.statistical_outlier(cloud, 20, 1.5)
    finally:
        cloud.free()
    try:
        return kept.numpy().T.astype(np.float64)
    finally:
        kept.free()


def ground_detection_on3segs(pcd_points, main_dist=20, max_iter=6, threshold_dist=0.18, match_image_range=False, *, ctx=None):
    """ground_detection_SVD.py:101-129 -> (stacked ground indices, stacked foreground indices).  x-segments (-150, -main_dist, main_dist,
    150), or (5, main_dist, 150) with match_image_range, open intervals; LPR_size 10000; the seed threshold is threshold_dist (:84).  A
    segment without a seed candidate (no point below z = -1.73 + 0.5, an empty segment included) is skipped, as :125-126 does."""
    pcd_points = np.asarray(pcd_points)
    segments_x = [5, main_dist, 150] if match_image_range else [-150, -main_dist, main_dist, 150]
    total_indices = np.array(range(pcd_points.shape[0]))
    stacked_ground_idx = np.empty(0, dtype=int)
    stacked_foregr_idx = np.empty(0, dtype=int)
    ctx = ctx or default_context()
    for i in range(len(segments_x) - 1):
        range_filter = np.logical_and(pcd_points[:, 0] < segments_x[i + 1], pcd_points[:, 0] > segments_x[i])
        seg_pts, seg_idx = pcd_points[range_filter], total_indices[range_filter]
        if not (np.asarray(seg_pts[:, 2], np.float32).astype(np.float64) < -1.73 + 0.5).any():      # the library's candidates: f32 z widened
            continue
        cloud = ctx.cloud(np.ascontiguousarray(seg_pts[:, :3], np.float32), PCR_AOS3)
        try:
            _, inliers = ctx.ground_detection(cloud, max_iter, 10000, threshold_dist)
        finally:
            cloud.free()
        stacked_ground_idx = np.r_[stacked_ground_idx, seg_idx[inliers]]
        stacked_foregr_idx = np.r_[stacked_foregr_idx, seg_idx[np.logical_not(inliers)]]
    return stacked_ground_idx, stacked_foregr_idx


def build_frame(points, bbox_dict, file_name="", *, ctx=None):
    """The body of build()'s loop (dataset_build.py:172-241) for one frame, writing nothing -> a dict:
      instances        [(name, (n, 3) f32)] in the reference's write order: Car, Pedestrian, Cyclist (the dict's order), box `num` of the class in
                       label order, boxes with fewer than 20 points left out (their `num` is still spent), name = <cls>_<file_name>_<num>.bin
      objects_idx_dict, other_obj_idx (the points in no box, ascending)
      remain_points    what pcd_preprocessing(match_image_range=True) keeps of them; fg_idx; foreground (= remain_points[fg_idx]); labels
      dontcare         [(name, (n, 3) f32)]: clusters in order of first appearance with id % 8 == 0 and more than 50 points, numbered by `num`
    points: (N, >= 3) scan rows.  A frame whose remainder is empty after preprocessing ends there (the reference's `continue`)."""
    points = np.asarray(points)
    objects_idx_dict, _, hits = get_objects_idx_dict(points[:, :3], bbox_dict, get_8_pts=False, ctx=ctx, return_hits=True)
    instances = []
    for cls in objects_idx_dict:
        for num, idx_sublist in enumerate(objects_idx_dict[cls]):
            if len(idx_sublist) < 20:
                continue
            instances.append((cls + "_" + file_name + "_" + str(num) + ".bin", np.asarray(points[idx_sublist, :3], np.float32)))
    other_obj_idx = np.flatnonzero(np.asarray(hits) == 0)                       # np.delete(range(N), every index of every box)
    out = {"instances": instances, "objects_idx_dict": objects_idx_dict, "other_obj_idx": other_obj_idx, "remain_points": np.zeros((0, 3)),
           "fg_idx": np.empty(0, dtype=int), "foreground": np.zeros((0, 3)), "labels": np.empty(0, np.int32), "dontcare": []}
    remain_points = pcd_preprocessing(points[other_obj_idx, :3], match_image_range=True, ctx=ctx)
    out["remain_points"] = remain_points
    if remain_points.shape[0] == 0:
        return out
    _, fg_idx = ground_detection_on3segs(remain_points, match_image_range=True, ctx=ctx)
    foreground = remain_points[fg_idx]
    labels = np.asarray(cluster_dbscan(foreground, 0.8, 20, print_progress=False, ctx=ctx), np.int32) if foreground.shape[0] else np.empty(0, np.int32)
    out.update(fg_idx=fg_idx, foreground=foreground, labels=labels)
    out["dontcare"] = dontcare_instances(foreground, labels, file_name)
    return out


def dontcare_instances(foreground, labels, file_name=""):
    """dataset_build.py:220-241: walk the clusters in order of first appearance; of those with id % 8 == 0 (one in eight) keep the ones with
    more than 50 points -> [(DontCare_<file_name>_<num>.bin, (n, 3) f32)], num counting the kept ones."""
    labels = np.asarray(labels)
    if labels.size == 0:
        return []
    first = {}
    for c, i in zip(*np.unique(labels, return_index=True)):
        first[int(c)] = int(i)
    out, num = [], 0
    for c in sorted(first, key=first.get):
        if c == -1 or c % 8 != 0:
            continue
        indices = np.flatnonzero(labels == c)
        if len(indices) > 50:
            out.append(("DontCare_" + file_name + "_" + str(num) + ".bin", np.asarray(foreground[indices, :], np.float32)))
            num += 1
    return out


def _write_instance(path, pts):
    with open(path, "wb") as f:
        array("f", np.asarray(pts, np.float32).flatten()).tofile(f)


def build(pcd_path, label_path, calib_path, my_db_path, *, ctx=None):
    """dataset_build.py:155-241: <my_db_path>/{Car, Cyclist, Pedestrian, DontCare}/<instance>.bin for every scan of pcd_path; an existing
    my_db_path is left alone."""
    if os.path.exists(my_db_path):
        print("{} already exists!".format(my_db_path))
        return
    os.mkdir(my_db_path)
    for d in ("Car", "Cyclist", "Pedestrian", "DontCare"):
        os.mkdir(os.path.join(my_db_path, d))
    for file_name in os.listdir(pcd_path):
        file_name = file_name.rstrip('.bin')
        points = raw_kitti_bin_reader(pcd_path, file_name)
        frame = build_frame(points, bbox_reader(label_path, calib_path, file_name), file_name, ctx=ctx)
        for name, pts in frame["instances"] + frame["dontcare"]:
            _write_instance(os.path.join(my_db_path, name.split("_")[0], name), pts)


def get_mean_hwl(pcd_path, label_path, calib_path):
    """dataset_build.py:419-449 -> [mean hwl of Car, of Cyclist, of Pedestrian] (f64[3] each) over the labels of every scan of pcd_path."""
    class_name = ["Car", "Cyclist", "Pedestrian"]
    class_hwl = [np.zeros(3), np.zeros(3), np.zeros(3)]
    class_num = [0, 0, 0]
    for file_name in os.listdir(pcd_path):
        file_name = file_name.rstrip('.bin')
        bbox_dict = bbox_reader(label_path, calib_path, file_name)
        for i in range(3):
            class_num[i] += len(bbox_dict[class_name[i]])
            for triple in bbox_dict[class_name[i]]:
                class_hwl[i] += triple[2]
    for i in range(3):
        class_hwl[i] /= class_num[i]
    return class_hwl


def object_bounding_boxes(points, labels, pred_final, *, ctx=None):
    """foreground_obj_cls.py:190-199: the axis-aligned box of every cluster classified 0, 1 or 2 -> ((k, 6) f64 rows of (min_bound,
    max_bound), the cluster ids int64 [k], ascending).  points: the (N, 3) foreground the labels index; pred_final: one class per cluster."""
    pred = np.asarray(pred_final).reshape(-1)
    pts = np.ascontiguousarray(np.asarray(points)[:, :3], np.float32)
    ctx = ctx or default_context()
    cloud = ctx.cloud(pts, PCR_AOS3)
    try:
        aabb, _ = ctx.label_aabb(cloud, labels, pred.size)
    finally:
        cloud.free()
    keep = np.flatnonzero(np.isin(pred, [0, 1, 2]))
    return aabb[keep].astype(np.float64), keep.astype(np.int64)
