"""Writes tests/golden/hw6_eval_ref.npz, and holds the ORACLE of the Homework6 tests: a numpy / Python f64 restatement of
Homework6/devkit_object/cpp/evaluate_object.cpp (the reference evaluator needs boost::geometry and cannot be compiled where the tests run).

    python tests/golden/gen_golden_hw6.py <reference root>

The restatement is scalar: Python floats are IEEE f64 and every operation is rounded on its own, so the loops below are the reference's loops
(imageBoxOverlap, toPolygon, box3DOverlap's heights and volumes, cleanData, computeStatistics, getThresholds, eval_class) statement by
statement, with no vectorised shortcut in the matching.  The ONE thing that is not the reference's is the quad intersection, which boost
computes there: clip_inter is the rule written out in include/pcr.h, and angle_inter is a second routine of a different construction (the
vertices of each quad inside the other plus the edge crossings, ordered by angle about their mean) that must agree with it to
1e-12 * (area_d + area_g) on every fixture pair, so that the restatement is not its own judge.

Inputs: FRAMES consecutive result files of Homework6/final_result/data (PointRCNN's output, as arrays), a window chosen so that it holds an
empty file, a detection under 25 px and a negative score.  KITTI's labels are not in the reference: ground truth is drawn by rule from the
detections with SplitMix64 keys (drop some, jitter pose, size and 2D box, add unmatched boxes and DontCare rows; Car / Van / Pedestrian /
Cyclist; occlusion 0 ... 3, truncation over all three limits; two decimals as label files have).
Band condition: no (gt, det) pair of the fixture has an overlap within BAND = 1e-9 of 0.7 or 0.5 under any metric or criterion (the offending
box is redrawn; asserted at the end): outside the band every decision is unambiguous, so counts must be EQUAL to the library's.
Recorded reference results: the text of final_result/stats_car_*.txt, plot/car_*.txt and the four "AP:" lines of overall_results.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "hw6_eval_ref.npz")
FRAMES = 200
BAND = 1e-9
IMAGE, GROUND, BOX3D = 0, 1, 2
MIN_HEIGHT = (40, 25, 25)
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
N_SAMPLE_PTS = 41.0
CODES = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4, "dontcare": 5}
NO_DETECTION = -10000000.0
# ground-truth row: cls trunc occ alpha x1 y1 x2 y2 h w l t1 t2 t3 ry; detection row: cls alpha x1 y1 x2 y2 h w l t1 t2 t3 ry score pad
G = dict(cls=0, trunc=1, occ=2, alpha=3, x1=4, y1=5, x2=6, y2=7, h=8, w=9, l=10, t1=11, t2=12, t3=13, ry=14)
D = dict(cls=0, alpha=1, x1=2, y1=3, x2=4, y2=5, h=6, w=7, l=8, t1=9, t2=10, t3=11, ry=12, score=13)


def _min(a, b):          # std::min / std::max: the second argument wins only on a strict comparison
    return b if b < a else a


def _max(a, b):
    return b if a < b else a


def _div(a, b):          # IEEE division (Python raises on a zero divisor)
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _box(row, is_gt):
    k = G if is_gt else D
    return {n: float(row[k[n]]) for n in ("x1", "y1", "x2", "y2", "h", "w", "l", "t1", "t2", "t3", "ry", "alpha")}


def image_overlap(d, g, criterion=-1):
    """imageBoxOverlap(a = detection, b = ground truth)"""
    x1, y1, x2, y2 = _max(d["x1"], g["x1"]), _max(d["y1"], g["y1"]), _min(d["x2"], g["x2"]), _min(d["y2"], g["y2"])
    w, h = x2 - x1, y2 - y1
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    a_area = (d["x2"] - d["x1"]) * (d["y2"] - d["y1"])
    b_area = (g["x2"] - g["x1"]) * (g["y2"] - g["y1"])
    if criterion == -1:
        return _div(inter, a_area + b_area - inter)
    return _div(inter, a_area) if criterion == 0 else _div(inter, b_area)


def to_polygon(b):
    """toPolygon: mref = [[cos, sin], [-sin, cos]], the corner order of the reference, then + t1, + t3"""
    c, s = math.cos(b["ry"]), math.sin(b["ry"])
    hl, hw, ns = b["l"] / 2, b["w"] / 2, -s
    X, Z = (hl, hl, -hl, -hl), (hw, -hw, -hw, hw)
    return [((c * X[i] + s * Z[i]) + b["t1"], (ns * X[i] + c * Z[i]) + b["t3"]) for i in range(4)]


def clip_inter(gq, dq):
    """the area of dq ∩ gq by the rule of include/pcr.h: dq clipped by the four edges of gq in corner order, shoelace about vertex 0"""
    a2 = 0.0
    for k in (1, 2):
        a2 = a2 + ((gq[k][0] - gq[0][0]) * (gq[k + 1][1] - gq[0][1]) - (gq[k + 1][0] - gq[0][0]) * (gq[k][1] - gq[0][1]))
    sgn = -1.0 if a2 < 0.0 else 1.0
    v = list(dq)
    for e in range(4):
        ax, az = gq[e]
        ex, ez = gq[(e + 1) & 3][0] - ax, gq[(e + 1) & 3][1] - az
        d = [sgn * (ex * (p[1] - az) - ez * (p[0] - ax)) for p in v]
        out = []
        n = len(v)
        for k in range(n):
            kq = k + 1 if k + 1 < n else 0
            (px, pz), (qx, qz), dp, dq_ = v[k], v[kq], d[k], d[kq]
            in_p, in_q = dp >= 0.0, dq_ >= 0.0
            if in_p:
                out.append((px, pz))
            if in_p != in_q:                          # from the inside end
                (ix, iz), (jx, jz), di, dj = ((px, pz), (qx, qz), dp, dq_) if in_p else ((qx, qz), (px, pz), dq_, dp)
                t = _div(di, di - dj)
                out.append((ix + (jx - ix) * t, iz + (jz - iz) * t))
        v = out[:8]
    s = 0.0
    for k in range(1, len(v) - 1):
        s = s + ((v[k][0] - v[0][0]) * (v[k + 1][1] - v[0][1]) - (v[k + 1][0] - v[0][0]) * (v[k][1] - v[0][1]))
    return abs(s * 0.5)


def angle_inter(gq, dq):
    """the same area by another construction: corners of each quad inside the other, the crossings of their edges, sorted by angle about
    their mean, shoelace about the mean"""
    def inside(p, q):
        s = [(q[(i + 1) & 3][0] - q[i][0]) * (p[1] - q[i][1]) - (q[(i + 1) & 3][1] - q[i][1]) * (p[0] - q[i][0]) for i in range(4)]
        return all(x >= 0 for x in s) or all(x <= 0 for x in s)
    pts = [p for p in dq if inside(p, gq)] + [p for p in gq if inside(p, dq)]
    for i in range(4):
        a, b = gq[i], gq[(i + 1) & 3]
        for j in range(4):
            c, d = dq[j], dq[(j + 1) & 3]
            r, s = (b[0] - a[0], b[1] - a[1]), (d[0] - c[0], d[1] - c[1])
            den = r[0] * s[1] - r[1] * s[0]
            if den == 0.0:
                continue
            t = ((c[0] - a[0]) * s[1] - (c[1] - a[1]) * s[0]) / den
            u = ((c[0] - a[0]) * r[1] - (c[1] - a[1]) * r[0]) / den
            if 0.0 <= t <= 1.0 and 0.0 <= u <= 1.0:
                pts.append((a[0] + t * r[0], a[1] + t * r[1]))
    if len(pts) < 3:
        return 0.0
    mx, mz = sum(p[0] for p in pts) / len(pts), sum(p[1] for p in pts) / len(pts)
    pts.sort(key=lambda p: math.atan2(p[1] - mz, p[0] - mx))
    s = 0.0
    for k in range(len(pts)):
        p, q = pts[k], pts[(k + 1) % len(pts)]
        s += (p[0] - mx) * (q[1] - mz) - (q[0] - mx) * (p[1] - mz)
    return abs(s) * 0.5


def ground_overlap(d, g, criterion=-1, inter_fn=clip_inter):
    inter = inter_fn(to_polygon(g), to_polygon(d))
    ad, ag = abs(d["l"] * d["w"]), abs(g["l"] * g["w"])
    if criterion == -1:
        return _div(inter, ad + ag - inter)
    return _div(inter, ad) if criterion == 0 else _div(inter, ag)


def box3d_overlap(d, g, criterion=-1, inter_fn=clip_inter):
    inter = inter_fn(to_polygon(g), to_polygon(d))
    ymax = _min(d["t2"], g["t2"])
    ymin = _max(d["t2"] - d["h"], g["t2"] - g["h"])
    inter_vol = inter * _max(0.0, ymax - ymin)
    det_vol = d["h"] * d["l"] * d["w"]
    gt_vol = g["h"] * g["l"] * g["w"]
    if criterion == -1:
        return _div(inter_vol, det_vol + gt_vol - inter_vol)
    return _div(inter_vol, det_vol) if criterion == 0 else _div(inter_vol, gt_vol)


OVERLAP = (image_overlap, ground_overlap, box3d_overlap)


def overlap_rows(metric, det_row, gt_row, criterion=-1):
    return OVERLAP[metric](_box(det_row, False), _box(gt_row, True), criterion)


def _trunc_i32(a):
    return int(a) if (a == a and -2147483649.0 < a < 2147483648.0) else -2147483648


def clean_data(current_class, gt, det, difficulty):
    """cleanData -> (ignored_gt, indices of the DontCare rows, ignored_det, n_gt)"""
    ignored_gt, ignored_det, n_gt = [], [], 0
    for g in gt:
        code = int(g[G["cls"]])
        height = float(g[G["y2"]]) - float(g[G["y1"]])
        if code == current_class:
            valid_class = 1
        elif current_class == 1 and code == 4:
            valid_class = 0
        elif current_class == 0 and code == 3:
            valid_class = 0
        else:
            valid_class = -1
        ignore = _trunc_i32(g[G["occ"]]) > MAX_OCCLUSION[difficulty] or g[G["trunc"]] > MAX_TRUNCATION[difficulty] or height <= MIN_HEIGHT[difficulty]
        if valid_class == 1 and not ignore:
            ignored_gt.append(0)
            n_gt += 1
        elif valid_class == 0 or (ignore and valid_class == 1):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
    dc = [i for i, g in enumerate(gt) if int(g[G["cls"]]) == 5]
    for d in det:
        height = _trunc_i32(abs(float(d[D["y1"]]) - float(d[D["y2"]])))
        if height < MIN_HEIGHT[difficulty]:
            ignored_det.append(1)
        elif int(d[D["cls"]]) == current_class:
            ignored_det.append(0)
        else:
            ignored_det.append(-1)
    return ignored_gt, dc, ignored_det, n_gt


class FrameOverlaps:
    """boxoverlap(det[j], gt[i], criterion) of one frame, computed once per (metric, criterion, i, j)"""

    def __init__(self, gt, det):
        self.gt, self.det = gt, det
        self.g = [_box(r, True) for r in gt]
        self.d = [_box(r, False) for r in det]
        self.memo = {}

    def __call__(self, metric, j, i, criterion):
        key = (metric, criterion, i, j)
        if key not in self.memo:
            self.memo[key] = OVERLAP[metric](self.d[j], self.g[i], criterion)
        return self.memo[key]


def compute_statistics(current_class, gt, det, dc, ignored_gt, ignored_det, compute_fp, ov, metric, compute_aos=False, thresh=0.0):
    """computeStatistics; dc holds indices into gt; ov = FrameOverlaps(gt, det) -> dict(tp, fp, fn, similarity, v)"""
    min_overlap = 0.7 if current_class == 0 else 0.5
    tp = fp = fn = 0
    similarity = 0.0
    v, delta = [], []
    nd = len(det)
    assigned_detection = [False] * nd
    ignored_threshold = [False] * nd
    if compute_fp:
        for i in range(nd):
            if det[i][D["score"]] < thresh:
                ignored_threshold[i] = True
    for i in range(len(gt)):
        if ignored_gt[i] == -1:
            continue
        det_idx = -1
        valid_detection = NO_DETECTION
        max_overlap = 0.0
        assigned_ignored_det = False
        for j in range(nd):
            if ignored_det[j] == -1:
                continue
            if assigned_detection[j]:
                continue
            if ignored_threshold[j]:
                continue
            overlap = ov(metric, j, i, -1)
            if not compute_fp and overlap > min_overlap and det[j][D["score"]] > valid_detection:
                det_idx = j
                valid_detection = float(det[j][D["score"]])
            elif compute_fp and overlap > min_overlap and (overlap > max_overlap or assigned_ignored_det) and ignored_det[j] == 0:
                max_overlap = overlap
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = False
            elif compute_fp and overlap > min_overlap and valid_detection == NO_DETECTION and ignored_det[j] == 1:
                det_idx = j
                valid_detection = 1
                assigned_ignored_det = True
        if valid_detection == NO_DETECTION and ignored_gt[i] == 0:
            fn += 1
        elif valid_detection != NO_DETECTION and (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
            assigned_detection[det_idx] = True
        elif valid_detection != NO_DETECTION:
            tp += 1
            v.append(float(det[det_idx][D["score"]]))
            if compute_aos:
                delta.append(float(gt[i][G["alpha"]]) - float(det[det_idx][D["alpha"]]))
            assigned_detection[det_idx] = True
    if compute_fp:
        for i in range(nd):
            if not (assigned_detection[i] or ignored_det[i] == -1 or ignored_det[i] == 1 or ignored_threshold[i]):
                fp += 1
        nstuff = 0
        for i in dc:
            for j in range(nd):
                if assigned_detection[j]:
                    continue
                if ignored_det[j] == -1 or ignored_det[j] == 1:
                    continue
                if ignored_threshold[j]:
                    continue
                if ov(metric, j, i, 0) > min_overlap:
                    assigned_detection[j] = True
                    nstuff += 1
        fp -= nstuff
        if compute_aos:
            if tp > 0 or fp > 0:
                for x in delta:                       # accumulate(tmp): fp zeros, then the similarities in order
                    similarity = similarity + (1.0 + math.cos(x)) / 2.0
            else:
                similarity = -1.0
    return {"tp": tp, "fp": fp, "fn": fn, "similarity": similarity, "v": v}


def get_thresholds(v, n_groundtruth):
    v = sorted((float(x) for x in v), reverse=True)
    t = []
    current_recall = 0.0
    n_groundtruth = float(n_groundtruth)
    for i in range(len(v)):
        l_recall = _div(float(i + 1), n_groundtruth)
        r_recall = _div(float(i + 2), n_groundtruth) if i < len(v) - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(v) - 1:
            continue
        t.append(v[i])
        current_recall += 1.0 / (N_SAMPLE_PTS - 1.0)
    return t


def _max_from(a, i):     # *max_element(a.begin() + i, a.end()): the first largest under operator<
    best = a[i]
    for x in a[i + 1:]:
        if best < x:
            best = x
    return best


def eval_class(current_class, gt_frames, det_frames, compute_aos, difficulty, metric, keep_frames=False):
    """eval_class -> dict(n_gt, thresholds, tp, fp, fn, similarity per threshold, precision[41], aos[41] or None[, per-frame records])"""
    n_gt, v = 0, []
    clean, ovs, collect = [], [], []
    for gt, det in zip(gt_frames, det_frames):
        i_gt, dc, i_det, n = clean_data(current_class, gt, det, difficulty)
        n_gt += n
        clean.append((i_gt, dc, i_det))
        ovs.append(FrameOverlaps(gt, det))
        st = compute_statistics(current_class, gt, det, dc, i_gt, i_det, False, ovs[-1], metric)
        collect.append(st)
        v.extend(st["v"])
    thresholds = get_thresholds(v, n_gt)
    nt = len(thresholds)
    assert nt <= 41
    tp, fp, fn, sim = [0] * nt, [0] * nt, [0] * nt, [0.0] * nt
    frames = []
    for f, (gt, det) in enumerate(zip(gt_frames, det_frames)):
        i_gt, dc, i_det = clean[f]
        rec = []
        for t in range(nt):
            st = compute_statistics(current_class, gt, det, dc, i_gt, i_det, True, ovs[f], metric, compute_aos, thresholds[t])
            tp[t] += st["tp"]
            fp[t] += st["fp"]
            fn[t] += st["fn"]
            if st["similarity"] != -1:
                sim[t] += st["similarity"]
            rec.append(st)
        frames.append(rec)
    precision = [0.0] * 41
    aos = [0.0] * 41 if compute_aos else None
    for i in range(nt):
        precision[i] = _div(float(tp[i]), float(tp[i] + fp[i]))
        if compute_aos:
            aos[i] = _div(sim[i], float(tp[i] + fp[i]))
    for i in range(nt):
        precision[i] = _max_from(precision, i)
        if compute_aos:
            aos[i] = _max_from(aos, i)
    out = {"n_gt": n_gt, "thresholds": thresholds, "tp": tp, "fp": fp, "fn": fn, "similarity": sim, "precision": precision, "aos": aos}
    if keep_frames:
        out["collect"], out["frames"] = collect, frames
    return out


# ---- the fixture ------------------------------------------------------------------------------------------------------------------------------
MASK = (1 << 64) - 1


def key(*words):
    """SplitMix64 over a tuple of integers -> u64"""
    z = 0x6A09E667F3BCC909
    for a in words:
        z = (z ^ ((0x9E3779B97F4A7C15 * (int(a) + 1)) & MASK)) & MASK
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        z ^= z >> 31
    return z


def u01(*words):
    return (key(*words) >> 11) / float(1 << 53)


def sym(*words):
    return 2.0 * u01(*words) - 1.0


def parse_detections(text):
    rows = []
    for line in text.splitlines():
        p = line.split()
        if len(p) != 16:
            continue
        v = [float(x) for x in p[1:]]
        rows.append([CODES.get(p[0].lower(), 6)] + v[2:15] + [0.0])
    return np.array(rows, np.float64).reshape(-1, 15)


def pick(u, table):
    acc = 0.0
    for value, p in table:
        acc += p
        if u < acc:
            return value
    return table[-1][0]


def draw_gt_from(f, j, d, salt):
    """one ground-truth row from detection row d by rule; None = dropped"""
    if u01(f, j, salt, 0) < 0.2:
        return None
    cls = pick(u01(f, j, salt, 1), ((0, 0.80), (3, 0.08), (1, 0.06), (2, 0.06)))
    big = u01(f, j, salt, 2) < 0.4
    a = 0.8 if big else 0.15
    t1 = d[D["t1"]] + a * sym(f, j, salt, 3)
    t3 = d[D["t3"]] + a * sym(f, j, salt, 4)
    t2 = d[D["t2"]] + 0.1 * sym(f, j, salt, 5)
    h, w, l = (d[D[n]] * (1.0 + 0.1 * sym(f, j, salt, 6 + i)) for i, n in enumerate(("h", "w", "l")))
    ry = d[D["ry"]] + 0.15 * sym(f, j, salt, 9) + (math.pi if u01(f, j, salt, 10) < 0.03 else 0.0)
    px = 12.0 if big else 4.0
    x1, y1, x2, y2 = (d[D[n]] + px * sym(f, j, salt, 11 + i) for i, n in enumerate(("x1", "y1", "x2", "y2")))
    alpha = d[D["alpha"]] + 0.2 * sym(f, j, salt, 15)
    occ = pick(u01(f, j, salt, 16), ((0, 0.55), (1, 0.25), (2, 0.12), (3, 0.08)))
    trunc = pick(u01(f, j, salt, 17), ((0.0, 0.6), (0.1, 0.1), (0.2, 0.1), (0.4, 0.1), (0.6, 0.1)))
    return [cls, trunc, occ] + [round(x, 2) for x in (alpha, x1, y1, x2, y2, h, w, l, t1, t2, t3, ry)]


def draw_extra(f, k, salt):
    """an unmatched Car somewhere in front of the sensor"""
    z = 5.0 + 55.0 * u01(f, 1000 + k, salt, 0)
    x = 20.0 * sym(f, 1000 + k, salt, 1)
    u = 600.0 + 720.0 * x / z
    hpx = 1.5 * 720.0 / z
    return [0, 0.0, pick(u01(f, 1000 + k, salt, 2), ((0, 0.6), (1, 0.3), (2, 0.1)))] + [round(v, 2) for v in (
        sym(f, 1000 + k, salt, 3) * 3.0, u - hpx, 180.0 - 0.3 * hpx, u + hpx, 180.0 + 0.7 * hpx, 1.5, 1.6, 3.9, x, 1.6, z, sym(f, 1000 + k, salt, 4) * 3.1)]


def dontcare_around(d, f, j, salt):
    m = 3.0 + 5.0 * u01(f, j, salt, 20)
    return [5, -1.0, -1.0, -10.0] + [round(v, 2) for v in (d[D["x1"]] - m, d[D["y1"]] - m, d[D["x2"]] + m, d[D["y2"]] + m)] + [-1.0, -1.0, -1.0, -1000.0, -1000.0, -1000.0, -10.0]


def in_band(gt_row, det_rows):
    g = _box(gt_row, True)
    for d_row in det_rows:
        d = _box(d_row, False)
        for m in range(3):
            for c in (-1, 0, 1):
                o = OVERLAP[m](d, g, c)
                if abs(o - 0.7) < BAND or abs(o - 0.5) < BAND:
                    return True
    return False


def draw_frame_gt(f, det):
    rows = []

    def add(make):
        salt = 0
        while True:
            r = make(salt)
            if r is None or not in_band(r, det):
                break
            salt += 1                                     # the band condition: redraw the offending box
        if r is not None:
            rows.append(r)
        return r

    for j, d in enumerate(det):
        if add(lambda s: draw_gt_from(f, j, d, s)) is None and u01(f, j, 0, 21) < 0.4:
            add(lambda s: dontcare_around(d, f, j, s))
    for k in range(int(3 * u01(f, 999, 0, 0))):
        add(lambda s: draw_extra(f, k, s))
    return np.array(rows, np.float64).reshape(-1, 15)


def choose_window(data_dir):
    names = sorted(n for n in os.listdir(data_dir) if n.endswith(".txt"))
    dets = [parse_detections(open(os.path.join(data_dir, n)).read()) for n in names]
    for start in range(0, len(names) - FRAMES, 50):
        w = dets[start:start + FRAMES]
        rows = np.concatenate(w)
        if any(len(x) == 0 for x in w) and (np.abs(rows[:, D["y1"]] - rows[:, D["y2"]]) < 25).any() and (rows[:, D["score"]] < 0).any():
            return names[start], w
    raise SystemExit("no window of result files holds an empty file, a detection under 25 px and a negative score")


def flat(frames):
    ptr = np.zeros(len(frames) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(x) for x in frames])
    return (np.concatenate(frames) if frames else np.zeros((0, 15))).reshape(-1, 15), ptr


def all_overlaps(gt_frames, det_frames, inter_fn=clip_inter):
    """[3 metrics][3 criteria] flat matrices (gt-major per frame), and the largest |clip - angle| / (area_d + area_g) when asked"""
    out = [[[] for _ in range(3)] for _ in range(3)]
    for gt, det in zip(gt_frames, det_frames):
        gs, ds = [_box(r, True) for r in gt], [_box(r, False) for r in det]
        for g in gs:
            for d in ds:
                for ci, c in enumerate((-1, 0, 1)):
                    out[IMAGE][ci].append(image_overlap(d, g, c))
                    out[GROUND][ci].append(ground_overlap(d, g, c, inter_fn))
                    out[BOX3D][ci].append(box3d_overlap(d, g, c, inter_fn))
    return np.array(out, np.float64).reshape(3, 3, -1)


def formulation_gap(gt_frames, det_frames):
    """max over the pairs of |clip_inter - angle_inter| / (area_d + area_g), and of the difference of the overlaps the two give"""
    worst = 0.0
    for gt, det in zip(gt_frames, det_frames):
        for g_row in gt:
            g = _box(g_row, True)
            gq = to_polygon(g)
            for d_row in det:
                d = _box(d_row, False)
                dq = to_polygon(d)
                worst = max(worst, abs(clip_inter(gq, dq) - angle_inter(gq, dq)) / (abs(d["l"] * d["w"]) + abs(g["l"] * g["w"])))
    return worst


def main(ref_root):
    res_dir = os.path.join(ref_root, "Homework6", "final_result")
    first, det_frames = choose_window(os.path.join(res_dir, "data"))
    gt_frames = [draw_frame_gt(f, det) for f, det in enumerate(det_frames)]
    for gt, det in zip(gt_frames, det_frames):
        assert not any(in_band(g, det) for g in gt), "band condition"
    gap = formulation_gap(gt_frames, det_frames)
    assert gap <= 1e-12, gap
    ov_clip = all_overlaps(gt_frames, det_frames, clip_inter)
    ov_angle = all_overlaps(gt_frames, det_frames, angle_inter)
    with np.errstate(invalid="ignore"):
        ov_gap = float(np.nanmax(np.abs(ov_clip - ov_angle)))
    det_rows, det_ptr = flat(det_frames)
    gt_rows, gt_ptr = flat(gt_frames)
    compute_aos = not (det_rows[:, D["alpha"]] == -10).any()
    nf = len(det_frames)
    rec = {k: [] for k in ("n_gt", "n_thr", "thr", "tp", "fp", "fn", "sim", "precision", "aos", "fs_tp", "fs_fp", "fs_fn", "fs_sim", "c_tp", "c_fn", "c_scores", "c_ptr")}
    for m in range(3):
        for dif in range(3):
            r = eval_class(0, gt_frames, det_frames, compute_aos and m == IMAGE, dif, m, keep_frames=True)
            nt = len(r["thresholds"])
            pad = lambda a, fill=0: list(a) + [fill] * (41 - nt)
            rec["n_gt"].append(r["n_gt"]); rec["n_thr"].append(nt); rec["thr"].append(pad(r["thresholds"], 0.0))
            rec["tp"].append(pad(r["tp"])); rec["fp"].append(pad(r["fp"])); rec["fn"].append(pad(r["fn"])); rec["sim"].append(pad(r["similarity"], 0.0))
            rec["precision"].append(r["precision"]); rec["aos"].append(r["aos"] if r["aos"] is not None else [0.0] * 41)
            for name, fld in (("fs_tp", "tp"), ("fs_fp", "fp"), ("fs_fn", "fn"), ("fs_sim", "similarity")):
                rec[name].append([pad([s[fld] for s in fr], 0) for fr in r["frames"]])
            rec["c_tp"].append([s["tp"] for s in r["collect"]]); rec["c_fn"].append([s["fn"] for s in r["collect"]])
            sc = [x for s in r["collect"] for x in s["v"]]
            rec["c_ptr"].append(len(sc)); rec["c_scores"].extend(sc)
            print(f"metric {m} difficulty {dif}: n_gt {r['n_gt']}, {nt} thresholds, tp[0] {r['tp'][:1]}, precision[0] {r['precision'][0]:.4f}")
    text = {}
    for n in ("stats_car_detection.txt", "stats_car_orientation.txt", "stats_car_detection_ground.txt", "stats_car_detection_3d.txt"):
        text[n] = open(os.path.join(res_dir, n)).read()
    for n in ("car_detection", "car_orientation", "car_detection_ground", "car_detection_3d"):
        text["plot/" + n + ".txt"] = open(os.path.join(res_dir, "plot", n + ".txt")).read()
    ap_lines = [l for l in open(os.path.join(res_dir, "overall_results")).read().splitlines() if " AP: " in l]
    assert len(ap_lines) == 4
    names = sorted(text)
    np.savez_compressed(
        OUT, first_file=first, det_rows=det_rows, det_ptr=det_ptr, gt_rows=gt_rows, gt_ptr=gt_ptr, compute_aos=compute_aos,
        overlaps=ov_clip, formulation_gap=gap, overlap_gap=ov_gap, band=BAND,
        n_gt=np.array(rec["n_gt"], np.int64), n_thr=np.array(rec["n_thr"], np.int32), thr=np.array(rec["thr"], np.float64),
        tp=np.array(rec["tp"], np.int64), fp=np.array(rec["fp"], np.int64), fn=np.array(rec["fn"], np.int64), sim=np.array(rec["sim"], np.float64),
        precision=np.array(rec["precision"], np.float64), aos=np.array(rec["aos"], np.float64),
        fs_tp=np.array(rec["fs_tp"], np.int16), fs_fp=np.array(rec["fs_fp"], np.int16), fs_fn=np.array(rec["fs_fn"], np.int16),
        fs_sim=np.array(rec["fs_sim"][:3], np.float64),
        c_tp=np.array(rec["c_tp"], np.int16), c_fn=np.array(rec["c_fn"], np.int16), c_scores=np.array(rec["c_scores"], np.float64),
        c_ptr=np.concatenate([[0], np.cumsum(rec["c_ptr"])]).astype(np.int64),
        text_names=np.array(names), text_values=np.array([text[n] for n in names]), ap_lines=np.array(ap_lines))
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; frames {first} + {nf}; {len(det_rows)} detections ({sum(len(x) == 0 for x in det_frames)} empty files), "
          f"{len(gt_rows)} ground truth; pairs {ov_clip.shape[2]}; formulation gap {gap:.3e} of (area_d + area_g), overlap gap {ov_gap:.3e}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
