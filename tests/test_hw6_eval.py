"""Homework6: the KITTI object evaluator on the GPU (csrc/kitti_eval.hip, hw6.py) — box overlaps, computeStatistics, thresholds, AP curves.

THE ORACLE IS A RESTATEMENT, not the reference binary: Homework6/devkit_object/cpp/evaluate_object.cpp needs boost::geometry and cannot be
compiled where the tests run, so tests/golden/gen_golden_hw6.py restates it in scalar f64 Python (the reference's loops statement by statement,
no vectorised shortcut in the matching) and the tests import that module.  The quad intersection — boost's there — is the clip rule of
include/pcr.h, checked in the generator and here against a second routine of another construction (corners inside + edge crossings, sorted by
angle).  Fixture tests/golden/hw6_eval_ref.npz: 200 consecutive result files of Homework6/final_result/data (4 empty, detections under 25 px,
negative scores) with ground truth drawn by rule, every expected matrix, count and curve, and the recorded text of the reference's own
final_result (stats, plot, AP lines).

Bounds.  Counts, thresholds and precision: EQUAL (no fixture pair lies within 1e-9 of 0.7 or 0.5, the band condition).  IMAGE overlaps: equal.
GROUND / BOX3D overlaps: within 4 x the difference the restatement's two formulations show on the fixture's overlaps — measured 6.44e-15 (1.99e-15 of
area_d + area_g on the intersections), so 2.6e-14; the library runs the clip rule itself with the host libm's sine and cosine, and on an MI355X the
difference measured against the clip restatement is 0 for all nine (metric, criterion).  Frame similarity: 1e-12 (tp + fp); measured 0.
aos: 1e-12 (its total is summed on the grid 2^-40: at most 4.6e-13).  AP against overall_results: 1e-4 in percent (curves printed to 6
decimals: 5e-5; measured 1.6e-5)."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "hands-on-point-cloud-processing_amd"


@pytest.fixture(scope="module")
def ref():
    spec = importlib.util.spec_from_file_location("gen_golden_hw6", os.path.join(ROOT, "tests", "golden", "gen_golden_hw6.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def hw6(pcr):
    return importlib.import_module(PKG + ".hw6")


@pytest.fixture(scope="module")
def fx(golden):
    z = golden("hw6_eval_ref.npz")
    f = {k: z[k] for k in z.files}
    for a in f.values():
        a.setflags(write=False)
    return f


@pytest.fixture(scope="module")
def frames(fx):
    gp, dp = fx["gt_ptr"].astype(int), fx["det_ptr"].astype(int)
    return ([fx["gt_rows"][gp[f]:gp[f + 1]] for f in range(len(gp) - 1)], [fx["det_rows"][dp[f]:dp[f + 1]] for f in range(len(dp) - 1)])


@pytest.fixture(scope="module")
def ctx(pcr):
    with pcr.Context(0) as c:
        yield c


def gt_row(cls=0, trunc=0.0, occ=0, alpha=0.0, box=(100, 100, 200, 200), hwl=(1.5, 1.6, 3.9), t=(0.0, 1.6, 20.0), ry=0.0):
    return [cls, trunc, occ, alpha, *box, *hwl, *t, ry]


def det_row(cls=0, alpha=0.0, box=(100, 100, 200, 200), hwl=(1.5, 1.6, 3.9), t=(0.0, 1.6, 20.0), ry=0.0, score=1.0):
    return [cls, alpha, *box, *hwl, *t, ry, score, 0.0]


def flat(per_frame):
    per_frame = [np.asarray(r, np.float64).reshape(-1, 15) for r in per_frame]
    ptr = np.zeros(len(per_frame) + 1, np.uint64)
    ptr[1:] = np.cumsum([len(r) for r in per_frame])
    return np.concatenate(per_frame).reshape(-1, 15), ptr


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------------
def test_two_intersection_formulations_agree_and_the_band_is_empty(ref, fx, frames):
    gts, dets = frames
    worst, k = 0.0, 0
    ground = fx["overlaps"][ref.GROUND, 0]
    for gt, det in zip(gts, dets):
        for g_row in gt:
            g = ref._box(g_row, True)
            gq = ref.to_polygon(g)
            for d_row in det:
                d = ref._box(d_row, False)
                dq = ref.to_polygon(d)
                a, b = ref.clip_inter(gq, dq), ref.angle_inter(gq, dq)
                worst = max(worst, abs(a - b) / (abs(d["l"] * d["w"]) + abs(g["l"] * g["w"])))
                assert ref._div(a, abs(d["l"] * d["w"]) + abs(g["l"] * g["w"]) - a) == ground[k]         # the fixture is what the generator computes today
                k += 1
    assert k == ground.size
    print(f"formulations: worst |clip - angle| / (area_d + area_g) = {worst:.3e}; overlaps differ by at most {float(fx['overlap_gap']):.3e}")
    assert worst <= 1e-12 and worst == float(fx["formulation_gap"])
    ov = fx["overlaps"]
    assert not np.isnan(ov).any()
    assert (np.abs(ov - 0.7) >= ref.BAND).all() and (np.abs(ov - 0.5) >= ref.BAND).all()
    assert 0 < float(fx["overlap_gap"]) < 1e-13


def test_analytic_overlaps_in_the_restatement(ref):
    def ov(metric, d, g, c=-1):
        return ref.overlap_rows(metric, d, g, c)
    g = gt_row(ry=0.3)
    d = det_row(ry=0.3)
    for m in range(3):
        assert ov(m, d, g) == pytest.approx(1.0, abs=1e-14)                                                   # identical boxes
    far = det_row(box=(300, 100, 400, 200), t=(30.0, 1.6, 20.0))
    assert [ov(m, far, gt_row()) for m in range(3)] == [0.0, 0.0, 0.0]                                        # disjoint
    touch = det_row(box=(200, 100, 300, 200), t=(3.9, 1.6, 20.0))                                             # shares the edge x = 1.95
    assert [ov(m, touch, gt_row()) for m in range(3)] == [0.0, 0.0, 0.0]
    small = det_row(box=(120, 120, 160, 180), hwl=(1.0, 0.8, 2.0), t=(0.3, 1.5, 20.2))                        # a box inside a box
    assert ov(ref.IMAGE, small, gt_row(), 0) == 1.0 and ov(ref.IMAGE, small, gt_row()) == pytest.approx(40 * 60 / 1e4, abs=1e-15)
    assert ov(ref.GROUND, small, gt_row(), 0) == pytest.approx(1.0, abs=1e-14)
    assert ov(ref.GROUND, small, gt_row()) == pytest.approx(0.8 * 2.0 / (1.6 * 3.9), abs=1e-14)
    assert ov(ref.BOX3D, small, gt_row(), 0) == pytest.approx(1.0, abs=1e-14)
    a, b = gt_row(hwl=(1, 1, 4), t=(0, 1, 10), ry=0.0), det_row(hwl=(1, 1, 4), t=(0, 1, 10), ry=np.pi / 2)
    assert ov(ref.GROUND, b, a) == pytest.approx(1 / 7, abs=1e-14)                                            # two 4 x 1 boxes crossed at 90 degrees
    a, b = gt_row(hwl=(1, 1, 1), t=(5, 1, 10), ry=0.0), det_row(hwl=(1, 1, 1), t=(5, 1, 10), ry=np.pi / 4)
    octagon = 2 * (np.sqrt(2) - 1)
    assert ov(ref.GROUND, b, a, 0) == pytest.approx(octagon, abs=1e-14)                                       # a unit square against itself turned 45 degrees
    assert ov(ref.GROUND, b, a) == pytest.approx(octagon / (2 - octagon), abs=1e-14)
    above = det_row(t=(0.0, -0.5, 20.0))                                                                      # no vertical overlap
    assert ov(ref.BOX3D, above, gt_row()) == 0.0 and ov(ref.GROUND, above, gt_row()) == pytest.approx(1.0, abs=1e-14)
    flat_det = det_row(hwl=(1.5, 1.6, 0.0))                                                                   # zero area
    assert np.isnan(ov(ref.GROUND, flat_det, gt_row(), 0)) and ov(ref.GROUND, flat_det, gt_row()) == 0.0


def _recorded(fx):
    return dict(zip(fx["text_names"].tolist(), fx["text_values"].tolist()))


def test_average_precision_reproduces_the_recorded_ap_lines(hw6, fx):
    text = _recorded(fx)
    worst = 0.0
    for line in fx["ap_lines"].tolist():
        name, vals = re.match(r"(\w+) AP: (.*)", line).groups()
        cols = np.array([[float(x) for x in l.split()] for l in text[f"plot/{name}.txt"].splitlines()])
        assert cols.shape == (41, 4) and np.array_equal(cols[:, 0], np.array([float("%f" % (i / 40.0)) for i in range(41)]))
        for k, want in enumerate(float(x) for x in vals.split()):
            got = hw6.average_precision(cols[:, 1 + k], "R11")
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-4, (line, k, got)
    print(f"AP R11 against overall_results: worst difference {worst:.2e} percent")
    c = np.arange(41, dtype=np.float64) / 50
    assert hw6.average_precision(c, "R40") == pytest.approx(100 * c[1:].mean(), abs=1e-12)
    assert hw6.average_precision(c, "R11") == pytest.approx(100 * c[::4].mean(), abs=1e-12)
    with pytest.raises(ValueError):
        hw6.average_precision(c[:40])
    with pytest.raises(ValueError):
        hw6.average_precision(c, "R12")


def test_save_writes_the_recorded_stats_and_plot_bytes(hw6, fx, tmp_path):
    text = _recorded(fx)
    curves = {}
    for kind in ("detection", "orientation", "detection_ground", "detection_3d"):
        cols = np.array([[float(x) for x in l.split()] for l in text[f"plot/car_{kind}.txt"].splitlines()])
        curves[("car", kind)] = cols[:, 1:].T
        stats = np.array([[float(x) for x in l.split()] for l in text[f"stats_car_{kind}.txt"].splitlines()])
        assert np.array_equal(stats, cols[:, 1:].T)                                                        # the plot columns are the stats rows
    hw6.Result(curves).save(str(tmp_path))
    for name, want in text.items():
        assert open(tmp_path / name).read() == want, name
    assert sorted(os.listdir(tmp_path / "plot")) == sorted(n[5:] for n in text if n.startswith("plot/"))


def test_loaders_scan_as_fscanf_and_set_the_flags(hw6, fx, tmp_path):
    names = {0: "Car", 1: "Pedestrian", 2: "Cyclist", 3: "Van", 5: "DontCare"}
    dp, gp = fx["det_ptr"].astype(int), fx["gt_ptr"].astype(int)
    for f in range(6):
        with open(tmp_path / ("%06d.txt" % f), "w") as fp:
            for r in fx["det_rows"][dp[f]:dp[f + 1]]:
                fp.write(names[int(r[0])] + " -1 -1 " + " ".join(repr(float(x)) for x in r[1:14]) + "\n")
    det = hw6.load_detections(str(tmp_path))
    assert len(det) == 6 and np.array_equal(det.rows, fx["det_rows"][:dp[6]]) and np.array_equal(det.row_ptr, fx["det_ptr"][:7])
    assert det.compute_aos and det.eval_image == [True, False, False] and det.eval_ground == [True, False, False] and det.eval_3d == [True, False, False]
    gtext = ["".join(names[int(r[0])].upper() + " " + repr(float(r[1])) + " %d " % r[2] + " ".join(repr(float(x)) for x in r[3:]) + "\n"
                     for r in fx["gt_rows"][gp[f]:gp[f + 1]]) for f in range(6)]
    gt = hw6.load_groundtruth(gtext)
    assert np.array_equal(gt.rows, fx["gt_rows"][:gp[6]]) and np.array_equal(gt.row_ptr, fx["gt_ptr"][:7])               # names match without case
    one = hw6.load_detections("Pedestrian 0 0 -10 -1 5 6 7 8 0 1 1 -1000 2 3 0.1\nCar 1 2 broken\ncyclist 0 0 0.5 1 2 3 4 1 1 1 1 -1000 1 0 0.25 trailing")
    assert one.rows.shape == (2, 15) and not one.compute_aos                                                            # the broken record is dropped
    assert one.eval_image == [False, False, True] and one.eval_ground == [False, False, True] and one.eval_3d == [False, False, False]
    assert len(hw6.load_detections("")) == 1 and hw6.load_detections("").rows.shape == (0, 15)


def test_clean_data_codes_match_the_restatement(hw6, ref, frames):
    gts, dets = frames
    extra_gt = np.array([gt_row(cls=4), gt_row(cls=6), gt_row(cls=1, box=(0, 0, 10, 25)), gt_row(cls=1, box=(0, 0, 10, 25.01), trunc=0.3, occ=2)])
    extra_det = np.array([det_row(cls=1, box=(0, 0.0, 5, 25.9)), det_row(cls=1, box=(0, 40.0, 5, 0.0)), det_row(cls=2, box=(0, 0, 5, 39.99))])
    cases = [(gts[f], dets[f]) for f in range(0, len(gts), 7)] + [(extra_gt, extra_det), (np.zeros((0, 15)), np.zeros((0, 15)))]
    seen = set()
    for gt, det in cases:
        for cls in range(3):
            for dif in range(3):
                ig, dc, idt, n = hw6.clean_data(cls, gt, det, dif)
                rig, rdc, ridt, rn = ref.clean_data(cls, gt, det, dif)
                assert ig.tolist() == rig and idt.tolist() == ridt and n == rn and len(dc) == len(rdc)
                seen.update(rig + ridt)
    assert seen == {0, 1, -1}


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("metric", [0, 1, 2])
def test_gpu_overlaps_match_the_restatement(ctx, fx, metric):
    bound = 4 * float(fx["overlap_gap"])
    is_dc = np.concatenate([np.repeat(fx["gt_rows"][int(fx["gt_ptr"][f]):int(fx["gt_ptr"][f + 1]), 0] == 5, int(fx["det_ptr"][f + 1] - fx["det_ptr"][f]))
                            for f in range(len(fx["gt_ptr"]) - 1)])
    for ci, crit in enumerate((-1, 0, 1)):
        mat_ptr, got = ctx.box_overlap(metric, crit, fx["gt_rows"], fx["gt_ptr"], fx["det_rows"], fx["det_ptr"])
        want = fx["overlaps"][metric, ci]
        assert got.shape == want.shape and int(mat_ptr[-1]) == want.size
        diff = float(np.abs(got - want).max())
        print(f"metric {metric} criterion {crit}: max |gpu - restatement| = {diff:.3e} (bound {0 if metric == 0 else bound:.3e})")
        if metric == 0:
            assert np.array_equal(got, want)
        else:
            assert diff <= bound
            assert is_dc.any() and (got[is_dc] == 0).all()                                                 # DontCare rows with their -1000 fields


@pytest.mark.gpu
def test_gpu_overlap_edges(ctx, hw6, ref):
    g = gt_row(ry=0.4)
    for d in (det_row(hwl=(1.5, 0.0, 0.0)), det_row(hwl=(1.5, 1.6, 0.0))):                                  # a point, a segment along the heading axis
        assert np.isnan(hw6.ground_box_overlap(d, gt_row(), 0, ctx=ctx)) and hw6.ground_box_overlap(d, gt_row(), -1, ctx=ctx) == 0.0
        assert np.isnan(hw6.box3d_overlap(d, gt_row(), 0, ctx=ctx)) and hw6.box3d_overlap(d, gt_row(), -1, ctx=ctx) == 0.0
    a, b = gt_row(hwl=(1, 1, 4), t=(0, 1, 10)), det_row(hwl=(1, 1, 4), t=(0, 1, 10), ry=np.pi / 2)
    assert hw6.ground_box_overlap(b, a, ctx=ctx) == pytest.approx(1 / 7, abs=1e-14)
    assert hw6.image_box_overlap(det_row(), g, ctx=ctx) == 1.0 and hw6.box3d_overlap(det_row(t=(0.0, -0.5, 20.0)), g, ctx=ctx) == 0.0
    # any launch geometry, empty frames between full ones, one-sided frames
    gts, gp = flat([[g], [], [g, gt_row(t=(1, 1.6, 21))], []])
    dts, dp = flat([[det_row()], [det_row()], [det_row(ry=0.2), det_row(t=(1, 1.6, 20.5)), det_row(ry=1.0)], []])
    m1, o1 = ctx.box_overlap(1, -1, gts, gp, dts, dp)
    assert m1.tolist() == [0, 1, 1, 7, 7]
    want = [ref.overlap_rows(1, d, gg) for f in (0, 2) for gg in gts[int(gp[f]):int(gp[f + 1])] for d in dts[int(dp[f]):int(dp[f + 1])]]
    assert np.abs(o1 - np.array(want)).max() <= 1e-14
    ctx.tune("kitti_blocks", 1)
    try:
        assert np.array_equal(ctx.box_overlap(1, -1, gts, gp, dts, dp)[1], o1)
    finally:
        ctx.tune("kitti_blocks", 0)
    m0, o0 = ctx.box_overlap(2, 1, np.zeros((0, 15)), [0], np.zeros((0, 15)), [0])
    assert m0.tolist() == [0] and o0.size == 0


COMBOS = [(m, d) for m in range(3) for d in range(3)]


@pytest.mark.gpu
@pytest.mark.parametrize("metric,dif", COMBOS)
def test_gpu_frame_stats_match_the_restatement(ctx, fx, metric, dif):
    cb = 3 * metric + dif
    nt = int(fx["n_thr"][cb])
    aos = metric == 0 and bool(fx["compute_aos"])
    r = ctx.kitti_frame_stats(0, metric, dif, True, aos, fx["thr"][cb, :nt], fx["gt_rows"], fx["gt_ptr"], fx["det_rows"], fx["det_ptr"])
    for k in ("tp", "fp", "fn"):
        bad = np.argwhere(r[k] != fx["fs_" + k][cb][:, :nt])
        assert bad.size == 0, f"{k}: first mismatch at (frame, threshold) {bad[0]}"
    if aos:
        want = fx["fs_sim"][cb][:, :nt]
        err = np.abs(r["similarity"] - want)
        print(f"similarity: max error {err.max():.3e}")
        assert (err <= 1e-12 * np.maximum(r["tp"] + r["fp"], 0)).all() and ((want == -1) == ((r["tp"] == 0) & (r["fp"] == 0))).all()
    else:
        assert (r["similarity"] == 0).all()
    c = ctx.kitti_frame_stats(0, metric, dif, False, False, None, fx["gt_rows"], fx["gt_ptr"], fx["det_rows"], fx["det_ptr"])
    assert np.array_equal(c["tp"], fx["c_tp"][cb]) and np.array_equal(c["fn"], fx["c_fn"][cb]) and (c["fp"] == 0).all()
    assert np.array_equal(np.concatenate(c["scores"]), fx["c_scores"][int(fx["c_ptr"][cb]):int(fx["c_ptr"][cb + 1])])          # in the reference's push order


def assert_eval_equal(got, want, what=""):
    """got: Context.kitti_eval's [metric][difficulty]; want(m, d) -> the restatement's dict"""
    for m, d in COMBOS:
        g, w = got[m][d], want(m, d)
        nt = len(w["thresholds"])
        assert g["n_gt"] == w["n_gt"] and len(g["thresholds"]) == nt, (what, m, d, len(g["thresholds"]), nt)
        assert np.array_equal(g["thresholds"], np.array(w["thresholds"], np.float64)), (what, m, d)
        for k in ("tp", "fp", "fn"):
            assert g[k].tolist() == list(w[k])[:nt], (what, m, d, k)
        assert np.array_equal(g["precision"], np.array(w["precision"]), equal_nan=True), (what, m, d)
        if w["aos"] is None:
            assert g["aos"] is None
        else:
            assert np.abs(g["aos"] - np.array(w["aos"])).max() <= 1e-12, (what, m, d)


def stored(fx):
    def want(m, d):
        cb, nt = 3 * m + d, int(fx["n_thr"][3 * m + d])
        return {"n_gt": int(fx["n_gt"][cb]), "thresholds": fx["thr"][cb, :nt], "tp": fx["tp"][cb, :nt], "fp": fx["fp"][cb, :nt], "fn": fx["fn"][cb, :nt],
                "precision": fx["precision"][cb], "aos": fx["aos"][cb] if (m == 0 and bool(fx["compute_aos"])) else None}
    return want


@pytest.fixture(scope="module")
def whole(ctx, fx):
    return ctx.kitti_eval(0, bool(fx["compute_aos"]), fx["gt_rows"], fx["gt_ptr"], fx["det_rows"], fx["det_ptr"])


@pytest.mark.gpu
def test_gpu_eval_matches_the_restatement(whole, fx):
    assert_eval_equal(whole, stored(fx), "fixture")
    assert max(len(whole[m][d]["thresholds"]) for m, d in COMBOS) < 41 and (whole[0][1]["precision"][len(whole[0][1]["thresholds"]):] == 0).all()


def restated(ref, gts, dets, cls, aos):
    memo = {}

    def want(m, d):
        if (m, d) not in memo:
            memo[(m, d)] = ref.eval_class(cls, gts, dets, aos and m == 0, d, m)
        return memo[(m, d)]
    return want


def edge_frames(ref):
    """the smallest shapes that can go wrong, by rule: see the comments; every frame is (ground truth rows, detection rows)"""
    car = lambda k, **kw: gt_row(box=(100 + 150 * k, 100, 200 + 150 * k, 200), t=(6.0 * k, 1.6, 20.0), alpha=0.1 * k, **kw)
    hit = lambda k, score, **kw: det_row(box=(102 + 150 * k, 101, 199 + 150 * k, 202), t=(6.0 * k + 0.05, 1.6, 20.02), alpha=0.1 * k + 0.05, score=score, **kw)
    fr = []
    fr.append(([], [hit(0, 0.9), hit(1, 0.2)]))                                                             # no ground truth
    fr.append(([car(0), car(1, occ=1)], []))                                                                # no detections
    fr.append(([], []))                                                                                     # neither
    fr.append(([car(0), car(1), car(2)], [hit(0, 0.5), hit(1, 0.5), hit(2, 0.7), hit(3, 0.5)]))              # tied scores, a false positive
    fr.append(([car(0, occ=3)], [hit(0, 0.8)]))                                                             # matches only an ignored ground truth
    # the hand-over: a short detection (24.9 px truncates to 24: ignored_det 1) met before a tall one over the same ground truth (26 px: valid from
    # MODERATE on, ignored under EASY)
    fr.append(([gt_row(box=(100, 100, 200, 126))], [det_row(box=(100, 100.5, 200, 125.4), t=(0.02, 1.6, 20.0), score=0.9),
                                                    det_row(box=(100, 100, 200, 126.2), t=(0.01, 1.6, 20.01), score=0.6)]))
    fr.append(([car(0), gt_row(cls=5, trunc=-1, occ=-1, alpha=-10, box=(395, 95, 505, 205), hwl=(-1, -1, -1), t=(-1000, -1000, -1000), ry=-10)],
               [hit(0, 0.4), det_row(box=(400, 100, 500, 200), t=(30.0, 1.6, 40.0), score=0.95)]))           # swallowed by a DontCare box
    fr.append(([car(0), gt_row(cls=3, box=(250, 100, 350, 200), t=(6.0, 1.6, 20.0))], [hit(1, 0.3), det_row(cls=1, score=0.99)]))  # a Van takes a Car detection
    for n in (65, 130):                                                                                     # past one and two mask words
        g = [gt_row(box=(10 + 60 * (k % 16), 50 + 70 * (k // 16), 60 + 60 * (k % 16), 110 + 70 * (k // 16)),
                    t=(5.0 * (k % 16), 1.6, 10.0 + 8.0 * (k // 16))) for k in range(0, n, 2)]
        d = [det_row(box=(11 + 60 * (k % 16), 51 + 70 * (k // 16), 60 + 60 * (k % 16), 111 + 70 * (k // 16)), t=(5.0 * (k % 16) + 0.03, 1.6, 10.0 + 8.0 * (k // 16)),
                     score=((k * 37) % 101) / 50.0 - 0.5, alpha=0.01 * k) for k in range(n - 1, -1, -1)]
        fr.append((g, d))
    return [np.asarray(g, np.float64).reshape(-1, 15) for g, _ in fr], [np.asarray(d, np.float64).reshape(-1, 15) for _, d in fr]


@pytest.mark.gpu
def test_gpu_edge_shapes_match_the_restatement(ctx, ref, hw6):
    gts, dets = edge_frames(ref)
    (g, gp), (d, dp) = flat(gts), flat(dets)
    for cls in (0, 1):                                                                                      # Pedestrian: one detection, no ground truth: n_gt = 0
        assert_eval_equal(ctx.kitti_eval(cls, True, g, gp, d, dp), restated(ref, gts, dets, cls, True), f"edge frames, class {cls}")
    got = ctx.kitti_eval(0, True, g, gp, d, dp)
    assert got[0][0]["n_gt"] > 0 and 0 < len(got[0][0]["thresholds"]) <= 41
    for m, dif in COMBOS:                                                                                   # ... and frame by frame, with the spill path
        w = restated(ref, gts, dets, 0, True)(m, dif)
        r = ctx.kitti_frame_stats(0, m, dif, True, m == 0, w["thresholds"], g, gp, d, dp)
        full = ref.eval_class(0, gts, dets, m == 0, dif, m, keep_frames=True)
        for k, name in (("tp", "tp"), ("fp", "fp"), ("fn", "fn")):
            assert r[k].tolist() == [[s[name] for s in fr] for fr in full["frames"]], (m, dif, k)
    # three true positives in all: fewer than 41 thresholds; a difficulty with n_gt = 0 (every ground truth occluded: easy has none)
    few_g, few_d = gts[3:4] + gts[1:2], dets[3:4] + dets[1:2]
    assert_eval_equal(ctx.kitti_eval(0, True, *flat(few_g), *flat(few_d)), restated(ref, few_g, few_d, 0, True), "three true positives")
    occ_g = [np.array([gt_row(occ=1), gt_row(occ=2, box=(300, 100, 400, 200), t=(9, 1.6, 20))])]
    occ_d = [np.array([det_row(score=0.3), det_row(box=(300, 100, 400, 200), t=(9, 1.6, 20), score=0.6)])]
    e = ctx.kitti_eval(0, True, *flat(occ_g), *flat(occ_d))
    assert e[0][0]["n_gt"] == 0 and len(e[0][0]["thresholds"]) == 0 and (e[0][0]["precision"] == 0).all() and e[0][2]["n_gt"] == 2
    assert_eval_equal(e, restated(ref, occ_g, occ_d, 0, True), "n_gt = 0")
    # every ground truth found: all 41 thresholds
    many_g = [np.array([gt_row(box=(10 + 60 * k, 50, 60 + 60 * k, 110), t=(5.0 * k, 1.6, 10.0)) for k in range(9)]) for _ in range(10)]
    many_d = [np.array([det_row(box=(10 + 60 * k, 50, 60 + 60 * k, 110), t=(5.0 * k, 1.6, 10.0), score=0.01 * (9 * f + k)) for k in range(9)]) for f in range(10)]
    e = ctx.kitti_eval(0, True, *flat(many_g), *flat(many_d))
    assert len(e[1][1]["thresholds"]) == 41
    assert_eval_equal(e, restated(ref, many_g, many_d, 0, True), "41 thresholds")
    assert np.array_equal(hw6.get_thresholds([0.5, 0.5, 0.7, 0.1, 0.5], 6, ctx=ctx), np.array(ref.get_thresholds([0.5, 0.5, 0.7, 0.1, 0.5], 6)))
    assert hw6.get_thresholds([], 0, ctx=ctx).size == 0
    # empty input
    e = ctx.kitti_eval(2, True, np.zeros((0, 15)), [0], np.zeros((0, 15)), [0])
    assert e[2][2]["n_gt"] == 0 and len(e[2][2]["thresholds"]) == 0


@pytest.mark.gpu
def test_gpu_evaluate_honours_the_gating_and_writes_the_files(ctx, ref, hw6, fx, whole, tmp_path):
    det = hw6.Frames(fx["det_rows"], fx["det_ptr"], compute_aos=True, eval_image=[True, False, False], eval_ground=[True, False, False], eval_3d=[True, False, False])
    gt = hw6.Frames(fx["gt_rows"], fx["gt_ptr"])
    res = hw6.evaluate(gt, det, ctx=ctx)
    assert list(res.curves) == [("car", "detection"), ("car", "orientation"), ("car", "detection_ground"), ("car", "detection_3d")]   # a class never detected is not evaluated
    assert np.array_equal(res.curves[("car", "detection_3d")][2], whole[2][2]["precision"])
    res.save(str(tmp_path))
    rows = open(tmp_path / "stats_car_detection.txt").read().splitlines()
    assert len(rows) == 3 and rows[1] == "".join("%f " % x for x in fx["precision"][1])
    assert len(open(tmp_path / "plot" / "car_orientation.txt").read().splitlines()) == 41
    no_aos = fx["det_rows"].copy()
    no_aos[5, 1] = -10                                                                                      # alpha = -10 switches AOS off
    text = ["".join("Car -1 -1 " + " ".join(repr(float(x)) for x in r[1:14]) + "\n" for r in no_aos[int(fx["det_ptr"][f]):int(fx["det_ptr"][f + 1])]) for f in range(len(gt))]
    det2 = hw6.load_detections(text)
    assert not det2.compute_aos and np.array_equal(det2.rows, no_aos)
    res2 = hw6.evaluate(gt, det2, ctx=ctx)
    assert ("car", "orientation") not in res2.curves and np.array_equal(res2.curves[("car", "detection")], res.curves[("car", "detection")])
    ap = res.ap("R40")
    assert ap[("car", "detection")][1] == pytest.approx(100 * fx["precision"][1][1:].mean(), abs=1e-9)


def same_bits(a, b):
    for m, d in COMBOS:
        for k in ("n_gt", "thresholds", "tp", "fp", "fn", "similarity", "precision", "aos"):
            x, y = a[m][d][k], b[m][d][k]
            assert (x is None and y is None) or np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), (m, d, k)


@pytest.mark.gpu
def test_gpu_eval_bits_do_not_depend_on_order_chunks_geometry_or_context_history(pcr, ctx, synth, fx, frames, whole):
    gts, dets = frames
    aos = bool(fx["compute_aos"])
    same_bits(ctx.kitti_eval(0, aos, *flat(gts[::-1]), *flat(dets[::-1])), whole)                            # frames in reversed order
    ctx.tune("kitti_blocks", 3)                                                                             # 12 waves for 1800 (frame, metric, difficulty)
    try:
        same_bits(ctx.kitti_eval(0, aos, fx["gt_rows"], fx["gt_ptr"], fx["det_rows"], fx["det_ptr"]), whole)
    finally:
        ctx.tune("kitti_blocks", 0)
    # two calls' worth of frames: the halves' frame statistics at the whole's thresholds add up to the whole's totals, similarity on its grid included
    h = len(gts) // 2 + 3
    for m, d in ((0, 1), (2, 2)):
        w = whole[m][d]
        parts = [ctx.kitti_frame_stats(0, m, d, True, m == 0 and aos, w["thresholds"], *flat(gts[a:b]), *flat(dets[a:b])) for a, b in ((0, h), (h, len(gts)))]
        for k in ("tp", "fp", "fn"):
            assert np.array_equal(sum(p[k].sum(axis=0, dtype=np.int64) for p in parts), w[k])
        if m == 0 and aos:
            q = sum(np.rint(np.where(p["similarity"] == -1, 0.0, p["similarity"]) * 2.0 ** 40).astype(np.int64).sum(axis=0) for p in parts)
            assert np.array_equal(q / 2.0 ** 40, w["similarity"])
    with pcr.Context(0) as used:                                                                            # a context another stage has used
        cloud = used.cloud(np.ascontiguousarray(synth.kitti_like_scan(20000)[:, :3], np.float32), 1)
        labels = used.dbscan(cloud, 0.6, 8)[0]
        used.label_aabb(cloud, labels, int(labels.max()) + 1)
        same_bits(used.kitti_eval(0, aos, fx["gt_rows"], fx["gt_ptr"], fx["det_rows"], fx["det_ptr"]), whole)
        used.statistical_outlier(cloud, 20, 2.0)
        same_bits(used.kitti_eval(0, aos, fx["gt_rows"], fx["gt_ptr"], fx["det_rows"], fx["det_ptr"]), whole)


@pytest.mark.gpu
def test_gpu_eval_past_one_grid_pass(ctx, ref, fx, frames):
    """the fixture tiled 16 x: 28 800 (frame, metric, difficulty) for the 8 192 waves of the default grid.  n_gt is 16 x; the thresholds are the
    restatement's over the 16-fold pooled scores; tp / fp / fn are 16 x the restatement's frame sums at those thresholds"""
    gts, dets = frames
    aos = bool(fx["compute_aos"])
    (g, gp), (d, dp) = flat(gts * 16), flat(dets * 16)
    big = ctx.kitti_eval(0, aos, g, gp, d, dp)
    for m, dif in COMBOS:
        cb = 3 * m + dif
        b = big[m][dif]
        pooled = np.tile(fx["c_scores"][int(fx["c_ptr"][cb]):int(fx["c_ptr"][cb + 1])], 16)
        assert b["n_gt"] == 16 * int(fx["n_gt"][cb])
        assert np.array_equal(b["thresholds"], np.array(ref.get_thresholds(pooled, b["n_gt"])))
    for m, dif in ((0, 1), (2, 2)):
        b = big[m][dif]
        tp, fp, fn = (np.zeros(len(b["thresholds"]), np.int64) for _ in range(3))
        sim = np.zeros(len(b["thresholds"]))
        for gt, det in zip(gts, dets):
            i_gt, dc, i_det, _ = ref.clean_data(0, gt, det, dif)
            ov = ref.FrameOverlaps(gt, det)
            for t, thr in enumerate(b["thresholds"]):
                s = ref.compute_statistics(0, gt, det, dc, i_gt, i_det, True, ov, m, m == 0 and aos, thr)
                tp[t] += s["tp"]; fp[t] += s["fp"]; fn[t] += s["fn"]
                sim[t] += s["similarity"] if s["similarity"] != -1 else 0.0
        assert np.array_equal(b["tp"], 16 * tp) and np.array_equal(b["fp"], 16 * fp) and np.array_equal(b["fn"], 16 * fn)
        if m == 0 and aos:
            assert np.abs(b["similarity"] - 16 * sim).max() <= 1e-12 * (16 * (tp + fp)).max()


@pytest.mark.gpu
def test_gpu_refused_arguments(pcr, ctx, fx):
    L = pcr.lib()
    g, gp, d, dp = fx["gt_rows"], fx["gt_ptr"], fx["det_rows"], fx["det_ptr"]
    out = (pcr.KittiCurve * 9)()
    args = (g.ctypes.data, gp.ctypes.data, d.ctypes.data, dp.ctypes.data, len(gp) - 1)
    assert L.pcr_kitti_eval_f64(ctx.h, 3, 1, *args, out) == -1 and L.pcr_kitti_eval_f64(ctx.h, 0, 1, *args, None) == -1
    assert L.pcr_kitti_eval_f64(None, 0, 1, *args, out) == -1
    bad = gp.copy()
    bad[3] = bad[5] + 1
    assert L.pcr_kitti_eval_f64(ctx.h, 0, 1, g.ctypes.data, bad.ctypes.data, d.ctypes.data, dp.ctypes.data, len(gp) - 1, out) == -1
    mp = np.zeros(len(gp), np.uint64)
    assert L.pcr_box_overlap_f64(ctx.h, 3, -1, *args, mp.ctypes.data, None, 0) == -1 and L.pcr_box_overlap_f64(ctx.h, 1, 2, *args, mp.ctypes.data, None, 0) == -1
    assert L.pcr_box_overlap_f64(ctx.h, 1, -1, *args, mp.ctypes.data, None, 0) == -1 and int(mp[-1]) == fx["overlaps"].shape[2]      # the sizing call
    thr = np.zeros(42)
    z = np.zeros(42 * (len(gp) - 1), np.int32)
    assert L.pcr_kitti_frame_stats_f64(ctx.h, 0, 0, 0, 1, 0, thr.ctypes.data, 42, *args, z.ctypes.data, z.ctypes.data, z.ctypes.data, thr.ctypes.data, None) == -1
    assert L.pcr_kitti_clean_data_f64(3, 0, None, 0, None, 0, None, None, None) == -1
    same_bits(ctx.kitti_eval(0, bool(fx["compute_aos"]), g, gp, d, dp), ctx.kitti_eval(0, bool(fx["compute_aos"]), g, gp, d, dp))     # the context still works
