"""Homework6 — the KITTI object evaluator (Homework6/devkit_object/cpp/evaluate_object.cpp) on the MI355X.

Mirrors the reference's function names and argument order; the GPU stages are csrc/kitti_eval.hip behind include/pcr.h (pcr_box_overlap_f64,
pcr_kitti_frame_stats_f64, pcr_kitti_thresholds_f64, pcr_kitti_eval_f64) and have NO CPU fallback.  Reading the files, matching the class names
and writing the result files is Python; cleanData's codes are the library's host function pcr_kitti_clean_data_f64.

  reference                                   here
  loadDetections(file, flags..., success)     load_detections(src)   -> Frames with .compute_aos, .eval_image / .eval_ground / .eval_3d
  loadGroundtruth(file, success)              load_groundtruth(src)  -> Frames
  imageBoxOverlap / groundBoxOverlap /        image_box_overlap / ground_box_overlap / box3d_overlap(det, gt, criterion=-1)
    box3DOverlap(det, gt, criterion)
  cleanData(class, gt, det, ..., difficulty)  clean_data(current_class, gt, det, difficulty) -> (ignored_gt, dontcare rows, ignored_det, n_gt)
  computeStatistics(...)                      compute_statistics(current_class, gt, det, difficulty, compute_fp, metric, compute_aos, thresh):
                                              the codes and the DontCare areas are derived inside from the class and the difficulty
  getThresholds(v, n_groundtruth)             get_thresholds(v, n_groundtruth)
  eval_class(..., difficulty, metric)         eval_class(current_class, groundtruth, detections, compute_aos) -> [metric][difficulty], ONE call
  eval(result_sha, mail)                      evaluate(gt, det) -> Result; Result.save(dir) writes stats_*.txt and plot/*.txt (no gnuplot, no mail)

Rows are 15 doubles in the order of the two fscanf calls with the name replaced by a class code (include/pcr.h).
  ctx=  a pcr Context; default: hw4's lazily created module-level context.
"""
from __future__ import annotations

import os

import numpy as np

from .hw4 import default_context

IMAGE, GROUND, BOX3D = 0, 1, 2
EASY, MODERATE, HARD = 0, 1, 2
CLASS_NAMES = ["car", "pedestrian", "cyclist"]
N_SAMPLE_PTS = 41
_CODES = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4, "dontcare": 5}
CODE_OTHER = 6


def class_code(name: str) -> int:
    """strcasecmp against the names the evaluator knows; everything else is one code"""
    return _CODES.get(name.lower(), CODE_OTHER)


class Frames:
    """the boxes of a run of frames: rows [n, 15] f64, row_ptr [n_frames + 1] u64; detections also carry loadDetections' flags"""

    def __init__(self, rows, row_ptr, compute_aos=True, eval_image=None, eval_ground=None, eval_3d=None):
        self.rows = np.ascontiguousarray(rows, np.float64).reshape(-1, 15)
        self.row_ptr = np.ascontiguousarray(row_ptr, np.uint64).reshape(-1)
        self.compute_aos = compute_aos
        self.eval_image = list(eval_image) if eval_image is not None else [False] * 3
        self.eval_ground = list(eval_ground) if eval_ground is not None else [False] * 3
        self.eval_3d = list(eval_3d) if eval_3d is not None else [False] * 3

    def __len__(self):
        return self.row_ptr.size - 1

    def frame(self, f: int) -> np.ndarray:
        return self.rows[int(self.row_ptr[f]):int(self.row_ptr[f + 1])]

    @classmethod
    def from_rows(cls, per_frame, **kw):
        per_frame = [np.asarray(r, np.float64).reshape(-1, 15) for r in per_frame]
        ptr = np.zeros(len(per_frame) + 1, np.uint64)
        ptr[1:] = np.cumsum([r.shape[0] for r in per_frame])
        rows = np.concatenate(per_frame) if per_frame else np.zeros((0, 15))
        return cls(rows, ptr, **kw)


def _texts(src):
    """a directory (every *.txt in name order), a file, one text, or a list of those -> list of texts, one per frame"""
    if isinstance(src, (list, tuple)):
        return [t for s in src for t in _texts(s)]
    if isinstance(src, str) and "\n" not in src and os.path.isdir(src):
        return [open(os.path.join(src, n)).read() for n in sorted(os.listdir(src)) if n.endswith(".txt")]
    if isinstance(src, str) and "\n" not in src and os.path.isfile(src):
        return [open(src).read()]
    return [src]


def _scan(text: str, n_fields: int, int_field: int = -1):
    """while (!feof) fscanf("%s %lf ..."): records of one word and n_fields numbers over whitespace-separated tokens; a record that does not
    convert is dropped and scanning resumes at the token that failed, as fscanf's does"""
    tok = text.split()
    pos, out = 0, []
    while pos < len(tok):
        vals = []
        for k in range(n_fields):
            if pos + 1 + k >= len(tok):
                break
            try:
                vals.append(float(int(tok[pos + 1 + k])) if k == int_field else float(tok[pos + 1 + k]))
            except ValueError:
                break
        if len(vals) == n_fields:
            out.append((tok[pos], vals))
        pos += 1 + len(vals)
    return out


def load_detections(src) -> Frames:
    """loadDetections for every frame of src: rows (class code, alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry, score, 0) and the flags
    compute_aos (no alpha == -10) and eval_image / eval_ground / eval_3d per class (detected once with valid fields)"""
    frames, aos = [], True
    ev = [[False] * 3 for _ in range(3)]
    for text in _texts(src):
        rows = []
        for name, v in _scan(text, 15):
            alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry, score = v[2:15]
            rows.append([class_code(name), alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry, score, 0.0])
            if alpha == -10:
                aos = False
            c = class_code(name)
            if c < 3:
                if x1 >= 0:
                    ev[0][c] = True
                if t1 != -1000 and t3 != -1000 and w > 0 and l > 0:
                    ev[1][c] = True
                if t1 != -1000 and t2 != -1000 and t3 != -1000 and h > 0 and w > 0 and l > 0:
                    ev[2][c] = True
        frames.append(rows)
    return Frames.from_rows(frames, compute_aos=aos, eval_image=ev[0], eval_ground=ev[1], eval_3d=ev[2])


def load_groundtruth(src) -> Frames:
    """loadGroundtruth: rows (class code, truncation, occlusion, alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry)"""
    frames = []
    for text in _texts(src):
        frames.append([[class_code(name)] + v for name, v in _scan(text, 14, int_field=1)])
    return Frames.from_rows(frames)


def _overlap(metric, det, gt, criterion, ctx):
    ctx = ctx or default_context()
    d = np.asarray(det, np.float64)
    g = np.asarray(gt, np.float64)
    single = d.ndim == 1 and g.ndim == 1
    d, g = d.reshape(-1, 15), g.reshape(-1, 15)
    _, out = ctx.box_overlap(metric, criterion, g, [0, g.shape[0]], d, [0, d.shape[0]])
    m = out.reshape(g.shape[0], d.shape[0])
    return float(m[0, 0]) if single else m


def image_box_overlap(det, gt, criterion=-1, *, ctx=None):
    """imageBoxOverlap(detection, ground truth, criterion): one pair -> float; rows -> the matrix [n_gt, n_det]"""
    return _overlap(IMAGE, det, gt, criterion, ctx)


def ground_box_overlap(det, gt, criterion=-1, *, ctx=None):
    return _overlap(GROUND, det, gt, criterion, ctx)


def box3d_overlap(det, gt, criterion=-1, *, ctx=None):
    return _overlap(BOX3D, det, gt, criterion, ctx)


def clean_data(current_class: int, gt, det, difficulty: int):
    """cleanData -> (ignored_gt i32, the DontCare rows, ignored_det i32, n_gt)"""
    import ctypes as C
    from . import lib, PcrError
    g = np.ascontiguousarray(gt, np.float64).reshape(-1, 15)
    d = np.ascontiguousarray(det, np.float64).reshape(-1, 15)
    ig, idt = np.zeros(max(len(g), 1), np.int32), np.zeros(max(len(d), 1), np.int32)
    n = C.c_uint64()
    rc = lib().pcr_kitti_clean_data_f64(int(current_class), int(difficulty), g.ctypes.data if len(g) else None, len(g), d.ctypes.data if len(d) else None, len(d),
                                        ig.ctypes.data, idt.ctypes.data, C.byref(n))
    if rc != 0:
        raise PcrError("clean_data: class and difficulty are 0 ... 2")
    return ig[:len(g)], g[g[:, 0] == 5], idt[:len(d)], int(n.value)


def compute_statistics(current_class: int, gt, det, difficulty: int, compute_fp: bool, metric: int, compute_aos: bool = False, thresh=0.0, *, ctx=None):
    """computeStatistics on ONE frame -> dict(tp, fp, fn, similarity, v); thresh may be a list (at most 41): the counts are then arrays"""
    ctx = ctx or default_context()
    g = np.asarray(gt, np.float64).reshape(-1, 15)
    d = np.asarray(det, np.float64).reshape(-1, 15)
    thr = np.atleast_1d(np.asarray(thresh, np.float64))
    r = ctx.kitti_frame_stats(current_class, metric, difficulty, compute_fp, compute_aos, thr if compute_fp else None, g, [0, len(g)], d, [0, len(d)])
    if not compute_fp:
        return {"tp": int(r["tp"][0]), "fp": 0, "fn": int(r["fn"][0]), "similarity": 0.0, "v": r["scores"][0]}
    if np.ndim(thresh) == 0:
        return {"tp": int(r["tp"][0, 0]), "fp": int(r["fp"][0, 0]), "fn": int(r["fn"][0, 0]), "similarity": float(r["similarity"][0, 0]), "v": np.zeros(0)}
    return {"tp": r["tp"][0], "fp": r["fp"][0], "fn": r["fn"][0], "similarity": r["similarity"][0], "v": np.zeros(0)}


def get_thresholds(v, n_groundtruth, *, ctx=None):
    return (ctx or default_context()).kitti_thresholds(v, int(n_groundtruth))


def eval_class(current_class: int, groundtruth: Frames, detections: Frames, compute_aos: bool, *, ctx=None):
    """eval_class for every (metric, difficulty) at once -> result[metric][difficulty] (Context.kitti_eval)"""
    if len(groundtruth) != len(detections):
        raise ValueError("groundtruth and detections hold the same frames")
    return (ctx or default_context()).kitti_eval(current_class, compute_aos, groundtruth.rows, groundtruth.row_ptr, detections.rows, detections.row_ptr)


def average_precision(curve, rule: str = "R11") -> float:
    """AP in percent from the 41 values of a curve: "R11" = every fourth point / 11 (what overall_results prints), "R40" = points 1 ... 40 / 40
    (the devkit readme's current rule)"""
    c = np.asarray(curve, np.float64).reshape(-1)
    if c.size != N_SAMPLE_PTS:
        raise ValueError("a curve has 41 values")
    if rule == "R11":
        return float(sum(c[0::4]) / 11.0 * 100.0)
    if rule == "R40":
        return float(sum(c[1:]) / 40.0 * 100.0)
    raise ValueError("rule: R11 or R40")


_KINDS = (("detection", ""), ("orientation", None), ("detection_ground", "_ground"), ("detection_3d", "_3d"))


class Result:
    """curves[(class name, kind)] = [easy, moderate, hard] x 41 for kind in detection, orientation, detection_ground, detection_3d, in the order
    the reference evaluates them"""

    def __init__(self, curves=None, detail=None):
        self.curves = dict(curves or {})
        self.detail = dict(detail or {})         # class name -> eval_class's [metric][difficulty]

    def ap(self, rule: str = "R11"):
        return {k: [average_precision(c, rule) for c in v] for k, v in self.curves.items()}

    def save(self, result_dir: str):
        """stats_<class>_detection[_ground|_3d].txt, stats_<class>_orientation.txt (rows of 41 "%f ") and plot/<class>_<kind>.txt"""
        plot = os.path.join(result_dir, "plot")
        os.makedirs(plot, exist_ok=True)
        for (name, kind), vals in self.curves.items():
            vals = np.asarray(vals, np.float64).reshape(3, N_SAMPLE_PTS)
            stats = f"stats_{name}_orientation.txt" if kind == "orientation" else f"stats_{name}_{kind}.txt"
            with open(os.path.join(result_dir, stats), "w") as fp:
                for row in vals:
                    fp.write("".join("%f " % x for x in row) + "\n")
            with open(os.path.join(plot, f"{name}_{kind}.txt"), "w") as fp:
                for i in range(N_SAMPLE_PTS):
                    fp.write("%f %f %f %f\n" % (i / (N_SAMPLE_PTS - 1.0), vals[0, i], vals[1, i], vals[2, i]))


def evaluate(gt: Frames, det: Frames, *, ctx=None) -> Result:
    """eval(): classes and metrics in the reference's order under its gating — a class is evaluated for a metric only if it was detected once
    with valid fields, AOS only for IMAGE and only if no alpha == -10 appeared"""
    res = Result()
    for c, name in enumerate(CLASS_NAMES):
        if not (det.eval_image[c] or det.eval_ground[c] or det.eval_3d[c]):
            continue
        r = eval_class(c, gt, det, det.compute_aos, ctx=ctx)
        res.detail[name] = r
    for c, name in enumerate(CLASS_NAMES):
        if det.eval_image[c]:
            res.curves[(name, "detection")] = [r["precision"] for r in res.detail[name][IMAGE]]
            if det.compute_aos:
                res.curves[(name, "orientation")] = [r["aos"] for r in res.detail[name][IMAGE]]
    for c, name in enumerate(CLASS_NAMES):
        if det.eval_ground[c]:
            res.curves[(name, "detection_ground")] = [r["precision"] for r in res.detail[name][GROUND]]
    for c, name in enumerate(CLASS_NAMES):
        if det.eval_3d[c]:
            res.curves[(name, "detection_3d")] = [r["precision"] for r in res.detail[name][BOX3D]]
    return res
