"""HomeworkFinal's two ends: the points inside oriented boxes (pcr_points_in_boxes_f64), the axis-aligned box of every cluster
(pcr_label_aabb_f32) and the module hwfinal that mirrors dataset_building/dataset_build.py and the box loop of foreground_obj_cls.py.

Parties: the REFERENCE's own bbox_reader and get_objects_idx_dict on one synthetic KITTI frame (tests/golden/dataset_build_ref.npz, written by
tests/golden/gen_golden_dataset_build.py on a CPU; the frame's scan is synth.kitti_like_scan(n), rebuilt here and checked against the recorded
checksum); the membership RULE of include/pcr.h restated in elementwise numpy f64 (gen.obb_rule — the reference for every drawn case: the
library computes the same f64 operations in the same order, so equality is exact); and the older signed-volume formulation of Open3D
(gen.signed_volume_rule), which must agree with the rule on the fixture.

Bounds.  Index lists, row_ptr and hits: equal.  bbox_reader: hwl equal; centre and front within 4 ulp of f32 at 128 m = 3.1e-5 m (a three-term
f32 dot plus an add whose order numpy's BLAS does not pin).  The boxes of label_aabb: equal to numpy's min / max as values.

The fixture's frame stores ONE DontCare instance (the synthetic scene has too few objects in front of the sensor for more, see the generator),
so the `% 8` and `> 50` rules are also exercised on labels drawn by rule, through hwfinal.dontcare_instances and the stand-in test."""
import ctypes as C
import hashlib
import importlib
import importlib.util
import inspect
import os
from array import array

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_golden_dataset_build", os.path.join(ROOT, "tests", "golden", "gen_golden_dataset_build.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

CLASSES = ["Car", "Pedestrian", "Cyclist"]
FRAME = "000000"
MIRRORED = {"dataset_building/dataset_build.py": ["raw_kitti_bin_reader", "bbox_reader", "get_objects_idx_dict", "get_points_idx_in_bbox", "build", "get_mean_hwl"],
            "dataset_building/ground_detection_SVD.py": ["pcd_preprocessing", "ground_detection_on3segs"]}


@pytest.fixture(scope="module")
def hwfinal(pcr):
    return importlib.import_module(pcr.__name__ + ".hwfinal")


@pytest.fixture(scope="module")
def fx(synth):
    """the fixture, the frame's scan rebuilt ((n, 3) f32) and the recorded index lists per box"""
    ref = np.load(os.path.join(ROOT, "tests", "golden", "dataset_build_ref.npz"))
    n = int(ref["n"][0])
    points = np.ascontiguousarray(synth.kitti_like_scan(n).T, np.float32)
    assert hashlib.sha256(points.tobytes()).digest() == ref["checksum"].tobytes(), "synth.kitti_like_scan no longer gives the fixture's scan"
    rp = ref["row_ptr"].astype(np.int64)
    rows = [ref["idx"][rp[b]:rp[b + 1]].astype(np.int64) for b in range(rp.size - 1)]
    idx_dict = {cls: [rows[b] for b in np.flatnonzero(ref["box_class"] == k)] for k, cls in enumerate(CLASSES)}
    return {"ref": ref, "n": n, "points": points, "rows": rows, "idx_dict": idx_dict, "label": ref["label_text"].tobytes().decode(),
            "calib": ref["calib_text"].tobytes().decode()}


@pytest.fixture(scope="module")
def ctx(pcr):
    c = pcr.Context(0)
    yield c
    c.close()


def write_frame(tmp_path, fx, with_scan=False):
    """the frame as KITTI files -> (pcd_path, label_path, calib_path), each a directory prefix as dataset_build.py takes them"""
    dirs = {}
    for name in ("velodyne", "label_2", "calib"):
        os.mkdir(tmp_path / name)
        dirs[name] = str(tmp_path / name) + os.sep
    with open(dirs["label_2"] + FRAME + ".txt", "w") as f:
        f.write(fx["label"])
    with open(dirs["calib"] + FRAME + ".txt", "w") as f:
        f.write(fx["calib"])
    if with_scan:
        np.concatenate([fx["points"], np.zeros((fx["n"], 1), np.float32)], axis=1).tofile(dirs["velodyne"] + FRAME + ".bin")
    return dirs["velodyne"], dirs["label_2"], dirs["calib"]


# ---- restatements (numpy, written from the reference's loops) ---------------------------------------------------------------------------
def rule_rows(points, seg, boxes, bseg):
    """pcr_points_in_boxes_f64 by the rule -> (row_ptr, idx, hits); a box with a non-finite field holds nothing"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    boxes = np.asarray(boxes, np.float64).reshape(-1, 15)
    rows, hits = [np.zeros(0, np.int64)] * int(bseg[0]), np.zeros(pts.shape[0], np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(len(seg) - 1):
            p = pts[seg[s]:seg[s + 1]]
            for b in range(bseg[s], bseg[s + 1]):
                inside = gen.obb_rule(p, boxes[b, 0:3], boxes[b, 3:12], boxes[b, 12:15]) if np.isfinite(boxes[b]).all() else np.zeros(p.shape[0], bool)
                rows.append(np.flatnonzero(inside))
                hits[seg[s]:seg[s + 1]] += inside.astype(np.uint32)
    sizes = np.array([r.size for r in rows], np.int64)
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), (np.concatenate(rows) if rows else np.zeros(0)).astype(np.uint32), hits


def restate_instances(points, idx_dict, file_name):
    """dataset_build.py:184-204 -> ([(name, bytes)], other_obj_idx)"""
    out, train = [], []
    for cls in idx_dict:
        train.append([i for sub in idx_dict[cls] for i in sub])
        for num, sub in enumerate(idx_dict[cls]):
            if len(sub) < 20:
                continue
            out.append((cls + "_" + file_name + "_" + str(num) + ".bin", array("f", points[sub, :3].flatten()).tobytes()))
    flat = [i for sub in train for i in sub]
    return out, np.delete(range(points.shape[0]), flat)


def restate_dontcare(remain_points, labels, file_name):
    """dataset_build.py:220-241 -> ([(name, bytes)], clusters rejected by % 8, clusters rejected by size)"""
    d = {}
    for i, c in enumerate(labels):
        d.setdefault(int(c), []).append(i)
    out, num, by_mod, by_size = [], 0, 0, 0
    for c in d:
        if c == -1:
            continue
        if c % 8 == 0:
            if len(d[c]) > 50:
                out.append(("DontCare_" + file_name + "_" + str(num) + ".bin", array("f", remain_points[d[c], :].flatten()).tobytes()))
                num += 1
            else:
                by_size += 1
        else:
            by_mod += 1
    return out, by_mod, by_size


def as_bytes(instances):
    return [(name, np.asarray(p, np.float32).tobytes()) for name, p in instances]


def drawn_boxes(rng, k, lo=-2.0, hi=2.0):
    """k oriented boxes by rule: centres in the cube, a rotation about a drawn axis, extents 0.3 ... 2.5"""
    out = np.zeros((k, 15))
    for b in range(k):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        a = rng.uniform(-np.pi, np.pi)
        K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
        R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
        out[b] = np.concatenate([rng.uniform(lo, hi, 3), R.reshape(9), rng.uniform(0.3, 2.5, 3)])
    return out


def lib_rows(pcr, ctx, points, seg, boxes, bseg):
    cloud = ctx.cloud(np.ascontiguousarray(points, np.float32).reshape(-1, 3), pcr.PCR_AOS3)
    try:
        return ctx.points_in_boxes(cloud, seg, boxes, bseg)
    finally:
        cloud.free()


def assert_same(got, want):
    for g, w, what in zip(got, want, ("row_ptr", "idx", "hits")):
        assert np.array_equal(np.asarray(g, np.uint64), np.asarray(w, np.uint64)), what


# ---- not GPU ----------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_module(pcr, hwfinal):
    for sym in ("pcr_points_in_boxes_f64", "pcr_label_aabb_f32"):
        assert sym in pcr.ABI_SYMBOLS and getattr(pcr.lib(), sym)
    for name in ("build_frame", "object_bounding_boxes", "dontcare_instances"):
        assert callable(getattr(hwfinal, name))


def test_signature_parity(hwfinal, fx):
    recorded = {}
    for s in fx["ref"]["signatures"].tolist():
        rel, rest = s.split(":", 1)
        name, args = rest[:-1].split("(", 1)
        recorded[(rel, name)] = [a.replace(" ", "") for a in args.split(",")] if args else []
    for rel, names in MIRRORED.items():
        for name in names:
            sig = inspect.signature(getattr(hwfinal, name))
            mine = [p.name if p.default is inspect.Parameter.empty else f"{p.name}={p.default!r}" for p in sig.parameters.values()
                    if p.kind is not inspect.Parameter.KEYWORD_ONLY]
            assert mine == recorded[(rel, name)], (name, mine, recorded[(rel, name)])
    sig = inspect.signature(hwfinal.build_frame)
    assert list(sig.parameters)[:3] == ["points", "bbox_dict", "file_name"] and sig.parameters["file_name"].default == ""


def test_rule_agrees_with_signed_volumes_on_the_fixture(fx):
    ref = fx["ref"]
    assert ref["obox"].shape[0] == len(fx["rows"]) == 14
    for b, want in enumerate(fx["rows"]):
        ob = ref["obox"][b]
        rule = np.flatnonzero(gen.obb_rule(fx["points"], ob[0:3], ob[3:12], ob[12:15]))
        vol, near = gen.signed_volume_rule(fx["points"], ob[0:3], ob[3:12], ob[12:15])
        assert np.array_equal(rule, want) and np.array_equal(np.flatnonzero(vol), want)
        assert near.min() > gen.BAND
    sizes = np.array([r.size for r in fx["rows"]])
    assert (sizes == 0).any() and ((sizes >= 1) & (sizes <= 19)).any() and any(np.unique(r // 2048).size > 1 for r in fx["rows"])
    allidx = np.concatenate(fx["rows"])
    assert np.unique(allidx).size < allidx.size                                   # two boxes overlap
    assert np.array_equal(np.delete(range(fx["n"]), allidx), ref["other_obj_idx"])


def test_bbox_reader_on_the_fixture_text(hwfinal, fx, tmp_path):
    _, label_path, calib_path = write_frame(tmp_path, fx)
    assert "Van " in fx["label"] and "DontCare " in fx["label"]
    got = hwfinal.bbox_reader(label_path, calib_path, FRAME)
    assert list(got) == CLASSES
    ref = fx["ref"]
    assert [len(got[c]) for c in CLASSES] == np.bincount(ref["box_class"], minlength=3).tolist()      # the Van and the DontCare line are ignored
    flat = [bp for c in CLASSES for bp in got[c]]
    for bp, rec in zip(flat, ref["box_params"]):
        assert bp[0].dtype == np.float32 and bp[1].dtype == np.float64 and bp[2].dtype == np.float32
        assert np.array_equal(np.asarray(bp[2], np.float64), rec[6:9])
        print("bbox_reader: |centre - ref|, |front - ref| =", np.abs(bp[0] - rec[0:3]).max(), np.abs(bp[1] - rec[3:6]).max())
        assert np.abs(np.asarray(bp[0], np.float64) - rec[0:3]).max() <= 3.1e-5 and np.abs(bp[1] - rec[3:6]).max() <= 3.1e-5
    # the box the library is handed, formed from the RECORDED label values, is the reference's own (center, R, extent): centre and extent are
    # IEEE sums and products (equal); R goes through atan2, cos and sin, each within an ulp of 1 on any libm: 1e-15
    for rec, ob in zip(ref["box_params"], ref["obox"]):
        row = hwfinal.obox_rows([hwfinal.bbox_to_obox((rec[0:3].astype(np.float32), rec[3:6], rec[6:9].astype(np.float32)))])[0]
        assert np.array_equal(row[0:3], ob[0:3]) and np.array_equal(row[12:15], ob[12:15]) and np.abs(row[3:12] - ob[3:12]).max() <= 1e-15


def drawn_labels(n, rng):
    """labels with 20 clusters of drawn sizes (some of the ids 0, 8, 16 above 50 members, one below) and noise, in a drawn order"""
    sizes = rng.integers(20, 60, 20)
    sizes[0], sizes[8], sizes[16] = 60, 30, 51
    lab = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)] + [np.full(n - int(sizes.sum()), -1)])
    return rng.permutation(lab).astype(np.int32)


def test_dontcare_rules_on_drawn_labels(hwfinal):
    rng = np.random.default_rng(5)
    n = 3000
    pts = rng.standard_normal((n, 3))
    labels = drawn_labels(n, rng)
    want, by_mod, by_size = restate_dontcare(pts, labels, FRAME)
    assert len(want) == 2 and by_mod >= 1 and by_size == 1
    assert as_bytes(hwfinal.dontcare_instances(pts, labels, FRAME)) == want
    assert hwfinal.dontcare_instances(pts[:0], labels[:0], FRAME) == []
    assert hwfinal.dontcare_instances(pts, np.full(n, -1), FRAME) == []


def test_build_frame_bookkeeping_with_stand_ins(hwfinal, fx, monkeypatch):
    """the selection and naming rules of build_frame without a GPU: every stage it calls is replaced by a numpy stand-in"""
    pts = fx["points"]
    rng = np.random.default_rng(6)

    def objects_stand_in(points, bbox_dict, get_8_pts=False, *, ctx=None, return_hits=False):
        d = {cls: [] for cls in CLASSES}
        hits = np.zeros(points.shape[0], np.uint32)
        for cls in bbox_dict:
            for bp in bbox_dict[cls]:
                c, R, e = hwfinal.bbox_to_obox(bp)
                m = gen.obb_rule(points, c, R, e)
                d[cls].append(np.flatnonzero(m))
                hits += m.astype(np.uint32)
        return d, None, hits

    state = {}

    def dbscan_stand_in(points, eps, min_points, print_progress=False, *, ctx=None):
        assert (eps, min_points) == (0.8, 20)
        state["labels"] = drawn_labels(points.shape[0], rng)
        return state["labels"]

    monkeypatch.setattr(hwfinal, "get_objects_idx_dict", objects_stand_in)
    monkeypatch.setattr(hwfinal, "pcd_preprocessing", lambda data, match_image_range=False, *, ctx=None: np.asarray(data[data[:, 0] > 5], np.float64))
    monkeypatch.setattr(hwfinal, "ground_detection_on3segs",
                        lambda p, match_image_range=False, *, ctx=None: (np.flatnonzero(p[:, 2] <= -1.4), np.flatnonzero(p[:, 2] > -1.4)))
    monkeypatch.setattr(hwfinal, "cluster_dbscan", dbscan_stand_in)
    ref = fx["ref"]
    bbox_dict = {cls: [(r[0:3].astype(np.float32), r[3:6], r[6:9].astype(np.float32)) for r in ref["box_params"][ref["box_class"] == k]]
                 for k, cls in enumerate(CLASSES)}
    scan4 = np.concatenate([pts, np.ones((fx["n"], 1), np.float32)], axis=1)          # rows of 4, as raw_kitti_bin_reader returns them
    out = hwfinal.build_frame(scan4, bbox_dict, FRAME)
    want, other = restate_instances(scan4, fx["idx_dict"], FRAME)
    assert as_bytes(out["instances"]) == want and len(want) >= 3
    assert [n for n, _ in want] == sorted([n for n, _ in want], key=lambda s: (CLASSES.index(s.split("_")[0]), int(s.split("_")[2][:-4])))
    skipped = [(cls, num) for cls in CLASSES for num, sub in enumerate(fx["idx_dict"][cls]) if len(sub) < 20]
    assert skipped and all(f"{cls}_{FRAME}_{num}.bin" not in dict(want) for cls, num in skipped)
    assert np.array_equal(out["other_obj_idx"], other) and np.array_equal(other, ref["other_obj_idx"])
    remain = scan4[other, :3].astype(np.float64)
    remain = remain[remain[:, 0] > 5]
    fg = remain[remain[:, 2] > -1.4]
    assert np.array_equal(out["remain_points"], remain) and np.array_equal(out["foreground"], fg) and np.array_equal(out["labels"], state["labels"])
    dc, by_mod, by_size = restate_dontcare(fg, state["labels"], FRAME)
    assert as_bytes(out["dontcare"]) == dc and len(dc) == 2 and by_mod >= 1 and by_size == 1


# ---- GPU: pcr_points_in_boxes_f64 ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_fixture_rows_are_the_references(pcr, ctx, fx):
    ref = fx["ref"]
    rp, idx, hits = lib_rows(pcr, ctx, fx["points"], [0, fx["n"]], ref["obox"], [0, ref["obox"].shape[0]])
    assert np.array_equal(rp.astype(np.int64), ref["row_ptr"]) and np.array_equal(idx, ref["idx"])
    assert np.array_equal(hits, np.bincount(ref["idx"], minlength=fx["n"]).astype(np.uint32))
    assert np.array_equal(np.flatnonzero(hits == 0), ref["other_obj_idx"])
    assert_same((rp, idx, hits), rule_rows(fx["points"], [0, fx["n"]], ref["obox"], [0, ref["obox"].shape[0]]))


@pytest.mark.gpu
def test_gpu_same_bits_for_every_tile(pcr, ctx, fx):
    ref = fx["ref"]
    base = None
    try:
        for tile in (64, 2048, 0, 1, 1 << 20, 100):                    # smallest, largest, default, and values the library clamps / rounds
            ctx.tune("pib_tile", tile)
            got = lib_rows(pcr, ctx, fx["points"], [0, fx["n"]], ref["obox"], [0, ref["obox"].shape[0]])
            base = base or got
            assert_same(got, base)
    finally:
        ctx.tune("pib_tile", 0)
    assert np.array_equal(base[1], ref["idx"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 511, 512, 513, 1025, 2600])
def test_gpu_points_per_segment(pcr, ctx, n):
    rng = np.random.default_rng(100 + n)
    pts = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    boxes = drawn_boxes(rng, 5)
    want = rule_rows(pts, [0, n], boxes, [0, 5])
    assert n < 64 or want[1].size > 0
    try:
        for tile in (0, 64):
            ctx.tune("pib_tile", tile)
            assert_same(lib_rows(pcr, ctx, pts, [0, n], boxes, [0, 5]), want)
    finally:
        ctx.tune("pib_tile", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n, k, tile", [(2600, 65, 64), (70000, 500, 64)])
def test_gpu_scan_levels(pcr, ctx, n, k, tile):
    """(tiles x boxes) counts beyond one scan block of 2048 (41 x 65), and beyond the 256 block sums one round of the top level takes (1094 x 500)"""
    rng = np.random.default_rng(k)
    pts = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    boxes = drawn_boxes(rng, k)
    boxes[:, 12:15] *= 0.25 if k > 100 else 1.0                       # many boxes: small ones, the lists stay short
    want = rule_rows(pts, [0, n], boxes, [0, k])
    assert -(-n // tile) * k > (2048 if k < 100 else 256 * 2048)
    try:
        ctx.tune("pib_tile", tile)
        assert_same(lib_rows(pcr, ctx, pts, [0, n], boxes, [0, k]), want)
    finally:
        ctx.tune("pib_tile", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 32, 33, 64, 65])
def test_gpu_box_counts(pcr, ctx, k):
    rng = np.random.default_rng(200 + k)
    pts = rng.uniform(-2, 2, (300, 3)).astype(np.float32)
    boxes = drawn_boxes(rng, k)
    got = lib_rows(pcr, ctx, pts, [0, 300], boxes, [0, k])
    assert_same(got, rule_rows(pts, [0, 300], boxes, [0, k]))
    assert got[0].size == k + 1 and (k == 0) == (got[1].size == 0)


@pytest.mark.gpu
def test_gpu_segments_are_local(pcr, ctx):
    rng = np.random.default_rng(7)
    pts = rng.uniform(-2, 2, (1500, 3)).astype(np.float32)
    seg, bseg = [100, 700, 700, 1450], [1, 4, 40, 42]                  # the middle segment is empty (and owns 36 boxes); box 0 belongs to no segment
    boxes = drawn_boxes(rng, 42)
    rp, idx, hits = lib_rows(pcr, ctx, pts, seg, boxes, bseg)
    assert_same((rp, idx, hits), rule_rows(pts, seg, boxes, bseg))
    rp = rp.astype(np.int64)
    assert rp[1] == 0 and rp[4] == rp[40] and idx.size > 0
    for s in range(3):                                                  # segment-local: every row against the segment's own points
        for b in range(bseg[s], bseg[s + 1]):
            row = idx[rp[b]:rp[b + 1]]
            assert (row < seg[s + 1] - seg[s]).all() and (np.diff(row.astype(np.int64)) > 0).all()
            assert np.array_equal(row, np.flatnonzero(gen.obb_rule(pts[seg[s]:seg[s + 1]], boxes[b, :3], boxes[b, 3:12], boxes[b, 12:])))
    assert not hits[:100].any() and not hits[1450:].any()


@pytest.mark.gpu
def test_gpu_faces_edges_corners_are_inside(pcr, ctx):
    """exact arithmetic: identity R, dyadic centre and extents and no face at 0, so t_a = p_a - c_a holds without rounding also one f32 step
    off a face (next to 0 a step is a denormal, which the f64 subtraction of the centre rounds away: the rule, not a fault)"""
    c, e = np.array([0.75, -1.25, 2.0]), np.array([1.0, 0.5, 0.25])
    h = e / 2
    up = lambda v: np.nextafter(np.float32(v), np.float32(np.inf))       # noqa: E731
    dn = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))      # noqa: E731
    pts = [c, c + [h[0], 0, 0], c - [0, h[1], 0], c + [h[0], h[1], 0], c + h, c - h, c + [h[0], -h[1], h[2]],      # centre, faces, edge, corners: inside
           [up(c[0] + h[0]), c[1], c[2]], [c[0], dn(c[1] - h[1]), c[2]], [c[0] + h[0], c[1] + h[1], up(c[2] + h[2])], [dn(c[0] - h[0]), c[1] - h[1], c[2] - h[2]]]
    pts = np.array(pts, np.float32)
    flat = np.concatenate([c, np.eye(3).reshape(9), [e[0], 0.0, e[2]]])     # a rectangle in the plane y = c_y
    boxes = np.stack([np.concatenate([c, np.eye(3).reshape(9), e]), flat])
    rp, idx, hits = lib_rows(pcr, ctx, pts, [0, len(pts)], boxes, [0, 2])
    assert np.array_equal(idx[:int(rp[1])], np.arange(7))
    assert np.array_equal(idx[int(rp[1]):], [0, 1])                          # exactly on the rectangle (7 lies in its plane, one step outside in x)
    assert np.array_equal(idx[int(rp[1]):], np.flatnonzero(gen.obb_rule(pts, c, np.eye(3), [e[0], 0.0, e[2]])))
    assert np.array_equal(hits, [2, 2, 1, 1, 1, 1, 1, 0, 0, 0, 0])


@pytest.mark.gpu
def test_gpu_hits_count_every_box(pcr, ctx):
    rng = np.random.default_rng(9)
    pts = rng.uniform(-3, 3, (500, 3)).astype(np.float32)
    pts[123] = [0.1, 0.2, -0.1]
    boxes = drawn_boxes(rng, 4)
    boxes[:3, 0:3] = [[0, 0, 0], [0.2, 0.1, 0], [-0.1, 0.3, 0.1]]
    boxes[:3, 12:15] = 2.0
    boxes[3, 0:3] = [2.5, 2.5, 2.5]
    boxes[3, 12:15] = 0.5
    rp, idx, hits = lib_rows(pcr, ctx, pts, [0, 500], boxes, [0, 4])
    assert_same((rp, idx, hits), rule_rows(pts, [0, 500], boxes, [0, 4]))
    assert hits[123] == 3 and all(123 in idx[int(rp[b]):int(rp[b + 1])] for b in range(3))


@pytest.mark.gpu
def test_gpu_non_finite_points_and_boxes(pcr, ctx):
    rng = np.random.default_rng(10)
    pts = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    pts[3, 0], pts[64, 1], pts[65, 2], pts[199] = np.nan, np.inf, -np.inf, [np.nan, np.inf, 0]
    boxes = drawn_boxes(rng, 6)
    boxes[:, 0:3] = 0
    boxes[:, 12:15] = 4.0                                               # every finite point is inside every finite box
    boxes[1, 5] = np.nan                                                # a NaN in R
    boxes[2, 13] = np.inf                                               # an infinite extent
    boxes[3, 0] = -np.inf                                               # an infinite centre
    boxes[4, 14] = np.nan
    rp, idx, hits = lib_rows(pcr, ctx, pts, [0, 200], boxes, [0, 6])
    assert_same((rp, idx, hits), rule_rows(pts, [0, 200], boxes, [0, 6]))
    finite = np.flatnonzero(np.isfinite(pts).all(1))
    assert finite.size == 196 and np.array_equal(np.diff(rp.astype(np.int64)), [196, 0, 0, 0, 0, 196])
    assert np.array_equal(idx[:196], finite) and not hits[[3, 64, 65, 199]].any() and (hits[finite] == 2).all()


@pytest.mark.gpu
def test_gpu_counting_call_fill_call_and_every_bad_argument(pcr, ctx):
    L = pcr.lib()
    rng = np.random.default_rng(11)
    pts = rng.uniform(-2, 2, (900, 3)).astype(np.float32)
    boxes = drawn_boxes(rng, 3)
    seg, bseg = np.array([0, 900], np.uint32), np.array([0, 3], np.uint32)
    want = rule_rows(pts, seg, boxes, bseg)
    total_want = int(want[0][-1])
    assert total_want > 3
    cloud = ctx.cloud(pts, pcr.PCR_AOS3)

    def call(c=ctx.h, cl=None, sp=seg, ns=1, bx=boxes, bp=bseg, rp=None, idx=None, cap=0, hits=None, total=None):
        return L.pcr_points_in_boxes_f64(c, cloud.h if cl is None else cl, None if sp is None else sp.ctypes.data, ns, None if bx is None else bx.ctypes.data,
                                         None if bp is None else bp.ctypes.data, None if rp is None else rp.ctypes.data, None if idx is None else idx.ctypes.data,
                                         cap, None if hits is None else hits.ctypes.data, None if total is None else C.byref(total))
    try:
        rp, total, hits = np.full(4, 77, np.uint64), C.c_uint64(), np.full(900, 77, np.uint32)
        assert call(rp=rp, total=total, hits=hits) == -1                     # the counting call: idx == NULL, idx_cap == 0 < total
        assert total.value == total_want and np.array_equal(rp, want[0]) and np.array_equal(hits, want[2])
        idx = np.full(total_want + 1, 0xDEAD, np.uint32)
        rp2, total2 = np.full(4, 77, np.uint64), C.c_uint64()
        assert call(rp=rp2, idx=idx, cap=total_want - 1, total=total2) == -1  # one short: idx untouched, row_ptr and total valid
        assert (idx == 0xDEAD).all() and np.array_equal(rp2, want[0]) and total2.value == total_want
        assert call(rp=rp2, idx=None, cap=total_want) == -1                  # room, but nowhere to write
        assert call(rp=rp2, idx=idx, cap=total_want) == 0
        assert np.array_equal(idx[:total_want], want[1]) and idx[total_want] == 0xDEAD
        # ---- PCR_ERR_ARG
        rp3 = np.zeros(4, np.uint64)
        assert L.pcr_points_in_boxes_f64(None, cloud.h, seg.ctypes.data, 1, boxes.ctypes.data, bseg.ctypes.data, rp3.ctypes.data, None, 0, None, None) == -1
        assert L.pcr_points_in_boxes_f64(ctx.h, None, seg.ctypes.data, 1, boxes.ctypes.data, bseg.ctypes.data, rp3.ctypes.data, None, 0, None, None) == -1
        assert call(sp=None, rp=rp3) == -1 and call(bp=None, rp=rp3) == -1 and call(rp=None) == -1 and call(bx=None, rp=rp3) == -1
        assert call(sp=np.array([5, 2], np.uint32), rp=rp3) == -1            # descends
        assert call(sp=np.array([0, 901], np.uint32), rp=rp3) == -1          # ends beyond the cloud
        assert call(sp=np.array([0, 10, 5], np.uint32), ns=2, bp=np.array([0, 1, 3], np.uint32), rp=rp3) == -1
        assert call(bp=np.array([3, 0], np.uint32), rp=rp3) == -1            # box_seg_ptr descends
        neg = boxes.copy()
        neg[1, 13] = -1e-300
        assert call(bx=neg, rp=rp3) == -1                                    # a negative extent
        # ---- the trivial cases
        rp4, tot4, hits4 = np.full(4, 77, np.uint64), C.c_uint64(5), np.full(900, 77, np.uint32)
        assert call(ns=0, bp=np.array([3], np.uint32), rp=rp4, total=tot4, hits=hits4) == 0 and not rp4.any() and tot4.value == 0 and not hits4.any()
        rp5 = np.full(1, 77, np.uint64)
        assert call(bx=None, bp=np.array([0, 0], np.uint32), rp=rp5, total=tot4) == 0 and rp5[0] == 0 and tot4.value == 0
        rp6 = np.full(4, 77, np.uint64)
        assert call(sp=np.array([40, 40], np.uint32), rp=rp6, total=tot4) == 0 and not rp6.any() and tot4.value == 0   # boxes, no point
    finally:
        cloud.free()


@pytest.mark.gpu
def test_gpu_more_counts_than_the_scan_takes_is_a_bad_argument(pcr, ctx):
    """boxes x tiles beyond 2^31 - 16: 2^16 boxes x 2^15 tiles of 64 points; refused on the host before any launch (the point and box limits
    themselves need arrays of 2^31 entries and are not run)"""
    n, k = 1 << 21, 1 << 16
    boxes = np.zeros((k, 15))
    boxes[:, [3, 7, 11]] = 1.0
    seg, bseg, rp, total = np.array([0, n], np.uint32), np.array([0, k], np.uint32), np.full(k + 1, 7, np.uint64), C.c_uint64(9)
    cloud = ctx.cloud(np.zeros((n, 3), np.float32), pcr.PCR_AOS3)
    try:
        ctx.tune("pib_tile", 64)
        rc = pcr.lib().pcr_points_in_boxes_f64(ctx.h, cloud.h, seg.ctypes.data, 1, boxes.ctypes.data, bseg.ctypes.data, rp.ctypes.data, None, 0, None, C.byref(total))
        assert rc == -1 and not rp.any() and total.value == 0
    finally:
        ctx.tune("pib_tile", 0)
        cloud.free()


@pytest.mark.gpu
def test_gpu_after_other_work_on_the_context(pcr, ctx, synth):
    """the scratch block is parked between calls: whatever an earlier call (of this operator or another) left there must not reach the scan"""
    rng = np.random.default_rng(12)
    big = rng.uniform(-2, 2, (30000, 3)).astype(np.float32)
    bb = drawn_boxes(rng, 40)
    small = rng.uniform(-2, 2, (700, 3)).astype(np.float32)
    sb = drawn_boxes(rng, 3)
    want_small = rule_rows(small, [0, 700], sb, [0, 3])
    assert_same(lib_rows(pcr, ctx, small, [0, 700], sb, [0, 3]), want_small)
    assert_same(lib_rows(pcr, ctx, big, [0, 30000], bb, [0, 40]), rule_rows(big, [0, 30000], bb, [0, 40]))
    cloud = ctx.cloud(big, pcr.PCR_AOS3)
    try:
        ctx.dbscan(cloud, 0.2, 5)                                           # fills the scratch block with its own tables
    finally:
        cloud.free()
    assert_same(lib_rows(pcr, ctx, small, [0, 700], sb, [0, 3]), want_small)


# ---- GPU: pcr_label_aabb_f32 ------------------------------------------------------------------------------------------------------------
def numpy_aabb(pts, labels, k):
    out = np.empty((k, 6), np.float32)
    out[:, :3], out[:, 3:] = np.inf, -np.inf
    cnt = np.zeros(k, np.uint32)
    for c in range(k):
        m = pts[labels == c]
        cnt[c] = m.shape[0]
        if m.shape[0]:
            with np.errstate(all="ignore"):
                lo, hi = np.nanmin(m, axis=0), np.nanmax(m, axis=0)
            out[c, :3], out[c, 3:] = np.where(np.isnan(lo), np.inf, lo), np.where(np.isnan(hi), -np.inf, hi)
    return out, cnt


@pytest.mark.gpu
def test_gpu_label_aabb_on_dbscan_labels(pcr, ctx, synth):
    scan = np.ascontiguousarray(synth.kitti_like_scan(20000).T, np.float32)
    fg = scan[scan[:, 2] > -1.4]
    cloud = ctx.cloud(fg, pcr.PCR_AOS3)
    try:
        labels, _, _, k = ctx.dbscan(cloud, 0.8, 20)
        assert k >= 3 and (labels == -1).any()
        aabb, cnt = ctx.label_aabb(cloud, labels, k + 2)                     # two ids nobody carries
        want, wcnt = numpy_aabb(fg, labels, k + 2)
        assert np.array_equal(aabb, want) and np.array_equal(cnt, wcnt)
        assert np.array_equal(aabb[k:, :3], np.full((2, 3), np.inf, np.float32)) and np.array_equal(aabb[k:, 3:], np.full((2, 3), -np.inf, np.float32)) and not cnt[k:].any()
        noise, ncnt = ctx.label_aabb(cloud, np.full(len(fg), -1, np.int32), 3)
        assert np.isposinf(noise[:, :3]).all() and np.isneginf(noise[:, 3:]).all() and not ncnt.any()
        L = pcr.lib()
        bad = labels.copy()
        bad[5] = k + 2
        out = np.zeros((k + 2, 6), np.float32)
        assert L.pcr_label_aabb_f32(ctx.h, cloud.h, bad.ctypes.data, k + 2, out.ctypes.data, None) == -1
        bad[5] = -2
        assert L.pcr_label_aabb_f32(ctx.h, cloud.h, bad.ctypes.data, k + 2, out.ctypes.data, None) == -1
        assert L.pcr_label_aabb_f32(ctx.h, cloud.h, None, k, out.ctypes.data, None) == -1
        assert L.pcr_label_aabb_f32(ctx.h, cloud.h, labels.ctypes.data, k, None, None) == -1
        assert L.pcr_label_aabb_f32(None, cloud.h, labels.ctypes.data, k, out.ctypes.data, None) == -1
        assert L.pcr_label_aabb_f32(ctx.h, cloud.h, np.full(len(fg), -1, np.int32).ctypes.data, 0, None, None) == 0
    finally:
        cloud.free()
    perm = np.random.default_rng(13).permutation(len(fg))
    pfg = fg[perm].copy()
    pfg[::97, 1] = np.nan                                                    # a NaN is skipped in its coordinate only
    fgn = fg.copy()
    fgn[perm[::97], 1] = np.nan
    c1, c2 = ctx.cloud(pfg, pcr.PCR_AOS3), ctx.cloud(fgn, pcr.PCR_AOS3)
    try:
        a1, n1 = ctx.label_aabb(c1, labels[perm], k)
        a2, n2 = ctx.label_aabb(c2, labels, k)
    finally:
        c1.free()
        c2.free()
    assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)) and np.array_equal(n1, n2) and np.array_equal(n1, wcnt[:k])
    wantn, _ = numpy_aabb(fgn, labels, k)
    assert np.array_equal(a2, wantn) and np.array_equal(a2[:, [0, 2, 3, 5]], want[:k][:, [0, 2, 3, 5]])


# ---- GPU: hwfinal end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame(hwfinal, ctx, fx, tmp_path_factory):
    """the fixture's frame through bbox_reader and build_frame, once"""
    tmp = tmp_path_factory.mktemp("kitti")
    pcd_path, label_path, calib_path = write_frame(tmp, fx, with_scan=True)
    bbox_dict = hwfinal.bbox_reader(label_path, calib_path, FRAME)
    points = hwfinal.raw_kitti_bin_reader(pcd_path, FRAME)
    return {"paths": (pcd_path, label_path, calib_path), "bbox_dict": bbox_dict, "points": points, "out": hwfinal.build_frame(points, bbox_dict, FRAME, ctx=ctx),
            "tmp": tmp}


@pytest.mark.gpu
def test_gpu_build_frame_on_the_fixture_frame(hwfinal, ctx, fx, frame):
    out, points = frame["out"], frame["points"]
    assert points.shape == (fx["n"], 4)
    for cls in CLASSES:
        assert len(out["objects_idx_dict"][cls]) == len(fx["idx_dict"][cls])
        assert all(np.array_equal(a, b) for a, b in zip(out["objects_idx_dict"][cls], fx["idx_dict"][cls]))
    want, other = restate_instances(points, fx["idx_dict"], FRAME)
    assert as_bytes(out["instances"]) == want and len(want) >= 3
    assert np.array_equal(out["other_obj_idx"], fx["ref"]["other_obj_idx"]) and np.array_equal(other, out["other_obj_idx"])
    # single boxes through get_points_idx_in_bbox, and the corner points
    bp = frame["bbox_dict"]["Car"][0]
    idx, eight = hwfinal.get_points_idx_in_bbox(points[:, :3], bp, True, ctx=ctx)
    assert np.array_equal(idx, fx["idx_dict"]["Car"][0]) and eight.shape == (8, 3) and np.allclose(eight[4:] - eight[:4], [0, 0, bp[2][0]])
    d2, pts8 = hwfinal.get_objects_idx_dict(points[:, :3], frame["bbox_dict"], True, ctx=ctx)
    assert pts8.shape == (8 * 14, 3) and np.array_equal(pts8[:8], eight) and list(d2) == CLASSES
    # the DontCare path on the library's own intermediates
    remain, fg_idx, labels = out["remain_points"], out["fg_idx"], out["labels"]
    assert remain.dtype == np.float64 and (remain[:, 0] > 5).all() and (remain[:, 1] < 30).all() and (remain[:, 1] > -15).all()
    assert 0 < remain.shape[0] < other.size and np.array_equal(out["foreground"], remain[fg_idx]) and labels.shape == (fg_idx.size,)
    dc, by_mod, by_size = restate_dontcare(out["foreground"], labels, FRAME)
    print("DontCare: stored", len(dc), "rejected by % 8", by_mod, "rejected by size", by_size, "clusters", int(labels.max()) + 1)
    assert as_bytes(out["dontcare"]) == dc and len(dc) >= 1 and by_mod >= 1
    stages = hwfinal.pcd_preprocessing(points[out["other_obj_idx"], :3], match_image_range=True, ctx=ctx)
    assert np.array_equal(stages, remain)
    g, f = hwfinal.ground_detection_on3segs(remain, match_image_range=True, ctx=ctx)
    assert np.array_equal(f, fg_idx) and np.intersect1d(g, f).size == 0 and g.size > 0
    assert (remain[np.r_[g, f], 0] > 5).all() and g.size + f.size == int(((remain[:, 0] > 5) & (remain[:, 0] != 20) & (remain[:, 0] < 150)).sum())
    far = remain + [200.0, 0, 0]                                               # nothing inside (5, 150): every segment is skipped
    g0, f0 = hwfinal.ground_detection_on3segs(far, match_image_range=True, ctx=ctx)
    assert g0.size == 0 and f0.size == 0
    g3, f3 = hwfinal.ground_detection_on3segs(np.r_[remain, remain * [-1, 1, 1]], ctx=ctx)      # the three-segment form
    assert g3.size and f3.size and np.intersect1d(g3, f3).size == 0


@pytest.mark.gpu
def test_gpu_build_writes_the_references_layout(hwfinal, ctx, fx, frame):
    pcd_path, label_path, calib_path = frame["paths"]
    db = str(frame["tmp"] / "my_kitti")
    hwfinal.build(pcd_path, label_path, calib_path, db, ctx=ctx)
    assert sorted(os.listdir(db)) == ["Car", "Cyclist", "DontCare", "Pedestrian"]
    want = {os.path.join(name.split("_")[0], name): b for name, b in as_bytes(frame["out"]["instances"] + frame["out"]["dontcare"])}
    got = {}
    for d in os.listdir(db):
        for f in os.listdir(os.path.join(db, d)):
            with open(os.path.join(db, d, f), "rb") as fh:
                got[os.path.join(d, f)] = fh.read()
    assert got == want and any(k.startswith("DontCare") for k in got) and any(k.startswith("Cyclist") for k in got)
    first = sorted(k for k in got if k.startswith("Car"))[0]
    assert np.array_equal(np.frombuffer(got[first], np.float32).reshape(-1, 3), fx["points"][fx["idx_dict"]["Car"][int(first[:-4].split("_")[-1])]])
    before = {k: os.path.getmtime(os.path.join(db, k)) for k in got}
    hwfinal.build(pcd_path, label_path, calib_path, db, ctx=ctx)                # an existing data base is left alone
    assert before == {k: os.path.getmtime(os.path.join(db, k)) for k in got}
    hwl = hwfinal.get_mean_hwl(pcd_path, label_path, calib_path)
    rec, cls = fx["ref"]["box_params"][:, 6:9], fx["ref"]["box_class"]
    for got_hwl, k in zip(hwl, (0, 2, 1)):                                      # Car, Cyclist, Pedestrian
        assert np.allclose(got_hwl, rec[cls == k].mean(0), rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_gpu_object_bounding_boxes_after_the_classifier(pcr, hwfinal, ctx):
    spec = importlib.util.spec_from_file_location("gen_golden_pointnet2", os.path.join(ROOT, "tests", "golden", "gen_golden_pointnet2.py"))
    g2 = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g2)
    pn = importlib.import_module(pcr.__name__ + ".pointnet")
    ref = np.load(os.path.join(ROOT, "tests", "golden", "pointnet2_cls_ref.npz"))
    model = pn.get_model(4).load_state_dict(g2.make_state(fc3_bias=ref["fc3_bias"])).eval()
    _, pred_final, res = pn.classify_foreground_objects(g2.base.load_scan(), seed=7, ctx=ctx, classifier=model)
    fg = res["points"][res["foreground_idx"]]
    boxes, ids = hwfinal.object_bounding_boxes(fg, res["labels"], pred_final, ctx=ctx)
    want_ids = np.flatnonzero(np.isin(pred_final, [0, 1, 2]))
    assert want_ids.size > 0 and (pred_final == 3).any() and np.array_equal(ids, want_ids) and boxes.shape == (want_ids.size, 6) and boxes.dtype == np.float64
    for row, c in zip(boxes, ids):
        m = fg[res["labels"] == c]
        assert np.array_equal(row[:3], m.min(0)) and np.array_equal(row[3:], m.max(0))
