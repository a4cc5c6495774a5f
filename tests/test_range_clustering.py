"""Homework4's second foreground path: range-image clustering (Homework4/foreground_clustering_range.py; pcr_range_image_*,
pcr_range_cluster_f32, hw4.pcd_to_range_image / range_image_labeling / cluster_assignment / depth_completion / cluster_range_image).

The numpy restatement below is the contract of include/pcr.h:
  project_ref   pcd_to_range_image (:13-48) with :34 restated as atan2(z, sqrt(x*x + y*y)) — the reference's own line raises TypeError —
                and a point the reference would raise IndexError on dropped
  label_loops   range_image_labeling (:51-95) as written, except that the flood fill keeps its own row / column variables (:66 overwrites
                the seed scan's `r`): every connected component, numbered by its first pixel in raster order
  label_ref     the same result from vectorised edge lists + scipy's connected components (checked against label_loops below); it also
                reports the pairs inside the rounding band
  assign_ref    cluster_assignment (:124-133);  close_ref: depth_completion (:136-149) as written
tests/golden/range_hw4_ref.npz (tests/golden/gen_golden_range.py) holds what the reference's own range_image_labeling and
cluster_assignment return on band-free inputs; the CPU tests check the relation pcr.h states between the two.

ROUNDING BAND (pcr.h): glibc's atan2 <= 1 ulp, the device's <= 6 ulp (OpenCL's bound for double atan2), one division on each side:
(7 + 1) * 2^-52 = 2^-49 relative, on a pixel coordinate q = angle / res_rad and on the edge angle against theta.  np.arctan2 may be a SIMD
implementation with a few ulp of its own, so the vectorised restatement re-decides every pair within 1e-12 (relative) of theta by math.atan2.
"""
import math
import os
import re

import numpy as np
import pytest

BAND = 2.0 ** -49
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["pcr_range_image_create_f32", "pcr_range_image_from_host_f64", "pcr_range_image_shape", "pcr_range_image_read",
             "pcr_range_image_close_f64", "pcr_range_image_label_f64", "pcr_range_image_assign", "pcr_range_image_destroy", "pcr_range_cluster_f32"]


# ------------------------------------------------------------------------------------------------------------------ restatement
def in_band(q):
    return abs(q - round(q)) <= BAND * max(abs(q), 1.0)


def project_ref(pts32, resolution):
    """-> dict(image (cropped f64), pix (per point: r * cols + c, -1 dropped), d, band (per point: a pixel coordinate inside the band),
    full_shape, dropped)"""
    p = np.asarray(pts32, np.float32).astype(np.float64)
    n = p.shape[0]
    res_rad = math.pi / 180 * resolution
    width, height = math.floor(360 / resolution) + 1, math.floor(60 / resolution) + 1
    ow, oh = math.ceil(width / 2), math.ceil(height / 2)
    full = np.full((height, width), -1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.linalg.norm(p, axis=1)
    pixfull = np.full(n, -1, np.int64)
    band = np.zeros(n, bool)
    for i in range(n):
        x, y, z = (float(v) for v in p[i])
        if not (math.isfinite(x) and math.isfinite(y) and math.isfinite(z)):
            continue
        qa = math.atan2(y, x) / res_rad
        qb = math.atan2(z, math.sqrt(x * x + y * y)) / res_rad
        band[i] = in_band(qa) or in_band(qb)
        cx = width - 1 - (math.floor(qa) + ow)
        ry = height - 1 - (math.floor(qb) + oh)
        if not (-width <= cx < width and -height <= ry < height):
            continue                                                    # numpy: IndexError
        cx, ry = cx % width, ry % height                                # numpy's negative indexing
        full[ry, cx] = d[i]
        pixfull[i] = ry * width + cx
    rowf = np.logical_not(np.all(full == -1, axis=1))
    colf = np.logical_not(np.all(full[rowf] == -1, axis=0)) if rowf.any() else np.zeros(width, bool)
    image = full[rowf][:, colf]
    rmap, cmap = np.cumsum(rowf) - 1, np.cumsum(colf) - 1
    ok = pixfull >= 0
    pix = np.full(n, -1, np.int64)
    pix[ok] = rmap[pixfull[ok] // width] * image.shape[1] + cmap[pixfull[ok] % width]
    return {"image": image, "pix": pix, "pixfull": pixfull, "d": d, "band": band, "full_shape": (height, width), "dropped": int(n - ok.sum())}


def label_loops(range_image, phi, theta, nn_mode):
    """range_image_labeling as written, with the flood fill's own variables (qr, qc) instead of the seed scan's (r, c)"""
    phi = phi * math.pi / 180
    threshold = theta * math.pi / 180
    label = 0
    rows, cols = range_image.shape
    image_label = np.full((rows, cols), -1, dtype=int)
    for r in range(rows):
        for c in range(cols):
            if image_label[r, c] == -1 and range_image[r, c] > 0:
                queue = [[r, c]]
                image_label[r, c] = label
                while queue:
                    qr, qc = queue.pop(0)
                    for rn in range(qr - nn_mode, qr + nn_mode + 1):
                        for cn in range(qc - nn_mode, qc + nn_mode + 1):
                            if rn < 0 or rn > rows - 1:
                                continue
                            if cn < 0:
                                cn += cols
                            if cn >= cols:
                                cn -= cols
                            if image_label[rn, cn] != -1:
                                continue
                            d1 = max(range_image[qr, qc], range_image[rn, cn])
                            d2 = min(range_image[qr, qc], range_image[rn, cn])
                            if d1 == -1 or d2 == -1:
                                continue
                            angle = math.atan2(d2 * math.sin(phi), (d1 - d2 * math.cos(phi)))
                            if angle > threshold and math.fabs(d1 - d2) < 1 and range_image[rn, cn] > 0:
                                queue.append([rn, cn])
                                image_label[rn, cn] = label
                label += 1
    return image_label


def edges_ref(range_image, phi, theta, nn_mode):
    """-> (a, b, certain, inband, linked): the forward half of every window as flat pixel pairs that pass every test but the angle's;
    linked = what the host's atan2 decides, inband = inside the rounding band of theta (linked or not), certain = linked and not inband"""
    img = np.asarray(range_image, np.float64)
    rows, cols = img.shape
    assert cols >= nn_mode
    phi_r, thr = phi * math.pi / 180, theta * math.pi / 180
    sphi, cphi = math.sin(phi_r), math.cos(phi_r)
    rr, cc = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    A, B, LINK, INB = [], [], [], []
    for dr in range(0, min(nn_mode, rows - 1) + 1):
        for dc in range(-nn_mode if dr else 1, nn_mode + 1):
            r1 = rr[:rows - dr].ravel()
            c1 = cc[:rows - dr].ravel()
            r2 = r1 + dr
            c2 = c1 + dc
            c2 = np.where(c2 < 0, c2 + cols, np.where(c2 >= cols, c2 - cols, c2))      # wrapped once
            a, b = r1 * cols + c1, r2 * cols + c2
            va, vb = img.ravel()[a], img.ravel()[b]
            keep = (va > 0) & (vb > 0) & (a != b)
            a, b, va, vb = a[keep], b[keep], va[keep], vb[keep]
            d1, d2 = np.maximum(va, vb), np.minimum(va, vb)
            with np.errstate(invalid="ignore"):
                near = np.abs(d1 - d2) < 1
            a, b, d1, d2 = a[near], b[near], d1[near], d2[near]
            yy, xx = d2 * sphi, d1 - d2 * cphi
            ang = np.arctan2(yy, xx)
            close = np.flatnonzero(np.abs(ang - thr) <= 1e-12 * np.maximum(np.abs(ang), thr))
            for k in close:                                                            # the reference's own atan2 decides
                ang[k] = math.atan2(float(yy[k]), float(xx[k]))
            inb = np.abs(ang - thr) <= BAND * np.maximum(np.abs(ang), thr)
            A.append(a), B.append(b), LINK.append(ang > thr), INB.append(inb)
    a, b, linked, inb = np.concatenate(A), np.concatenate(B), np.concatenate(LINK), np.concatenate(INB)
    return a, b, linked & ~inb, inb, linked


def components_ref(range_image, a, b):
    """labels of the components of the edge list, numbered by first pixel in raster order; -1 where range <= 0"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    img = np.asarray(range_image, np.float64)
    npix = img.size
    g = coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(npix, npix))
    _, comp = connected_components(g, directed=False)
    occ = np.flatnonzero(img.ravel() > 0)
    out = np.full(npix, -1, np.int64)
    if occ.size:
        first = np.full(comp.max() + 1, npix, np.int64)
        np.minimum.at(first, comp[occ], occ)
        order = np.argsort(first, kind="stable")                        # components without an occupied pixel sort last (first = npix)
        rank = np.empty_like(order)
        rank[order] = np.arange(order.size)
        out[occ] = rank[comp[occ]]
    return out.reshape(img.shape)


def label_ref(range_image, phi, theta, nn_mode):
    """-> (image_label as the host's atan2 decides every pair, number of in-band pairs)"""
    a, b, cert, inb, linked = edges_ref(range_image, phi, theta, nn_mode)
    return components_ref(range_image, a[linked], b[linked]), int(inb.sum())


def assign_ref(pix, image_label):
    flat = np.asarray(image_label).reshape(-1)
    return np.where(pix >= 0, flat[np.maximum(pix, 0)], -1)


def close_ref(image, pad):
    rows, cols = image.shape
    dila = np.full_like(image, -1, dtype=float)
    closing = np.full_like(image, -1, dtype=float)
    for r in range(pad, rows - pad):
        for c in range(pad, cols - pad):
            dila[r, c] = np.amax(image[r - pad: r + pad + 1, c - pad: c + pad + 1])
    for r in range(pad, rows - pad):
        for c in range(pad, cols - pad):
            closing[r, c] = np.amin(dila[r - pad: r + pad + 1, c - pad: c + pad + 1])
    return closing


def same_partition(x, y):
    """two labelings describe the same partition (and the same unlabelled set)"""
    x, y = np.asarray(x).ravel(), np.asarray(y).ravel()
    if not np.array_equal(x < 0, y < 0):
        return False
    m = x >= 0
    pairs = np.unique(np.stack([x[m], y[m]]), axis=1)
    return pairs.shape[1] == np.unique(x[m]).size == np.unique(y[m]).size


def refines(fine, coarse):
    """every set of `fine` lies inside one set of `coarse` (same unlabelled pixels)"""
    fine, coarse = np.asarray(fine).ravel(), np.asarray(coarse).ravel()
    if not np.array_equal(fine < 0, coarse < 0):
        return False
    m = fine >= 0
    pairs = np.unique(np.stack([fine[m], coarse[m]]), axis=1)
    return pairs.shape[1] == np.unique(fine[m]).size


# ------------------------------------------------------------------------------------------------------------------ synthetic inputs
def sphere_points(rng, n, resolution, rmin=4.0, rmax=40.0, beta_max=25.0):
    """points at random directions inside the image, ranges piecewise smooth in the direction (objects + gaps)"""
    az = rng.uniform(-180.0, 180.0, n)
    el = rng.uniform(-beta_max, beta_max, n)
    rng_ = rmin + (rmax - rmin) * (0.5 + 0.5 * np.sin(az / 17.0) * np.cos(el / 9.0)) + rng.normal(0, 0.05, n)
    rng_ = np.where(rng.random(n) < 0.3, rng_ * 0.5, rng_)
    a, e = np.radians(az), np.radians(el)
    pts = np.stack([rng_ * np.cos(e) * np.cos(a), rng_ * np.cos(e) * np.sin(a), rng_ * np.sin(e)], axis=1)
    return pts.astype(np.float32)


def random_image(rng, rows, cols, fill=0.5):
    """a range image of blobs: smooth ranges with steps, `fill` of the pixels occupied"""
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    img = 10.0 + 6.0 * np.sin(r / 5.0 + rng.uniform(0, 6)) * np.cos(c / 11.0 + rng.uniform(0, 6)) + rng.normal(0, 0.15, (rows, cols))
    img += np.where(rng.random((rows, cols)) < 0.2, rng.uniform(-3, 3, (rows, cols)), 0.0)
    img = np.abs(img) + 0.5
    img[rng.random((rows, cols)) >= fill] = -1.0
    return img


def spiral_image(rows, cols, value=10.0):
    """a one-pixel-wide rectangular spiral with one empty pixel between its turns: ONE component at nn_mode 1, a chain of thousands of
    pixels (long union-find paths).  The last two columns stay empty."""
    img = np.full((rows, cols), -1.0)
    w = cols - 2
    dirs = [(0, 1), (1, 0), (0, -1), (-1, 0)]
    r, c, d, turns = 0, 0, 0, 0
    img[0, 0] = value
    while turns < 2:
        dr, dc = dirs[d]
        r1, c1, r2, c2 = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        ahead_free = not (0 <= r2 < rows and 0 <= c2 < w) or img[r2, c2] < 0
        if 0 <= r1 < rows and 0 <= c1 < w and img[r1, c1] < 0 and ahead_free:
            r, c, turns = r1, c1, 0
            img[r, c] = value
        else:
            d, turns = (d + 1) % 4, turns + 1
    return img


# ------------------------------------------------------------------------------------------------------------------ CPU tests
@pytest.fixture(scope="module")
def fixture(golden):
    return golden("range_hw4_ref.npz")


def fixture_cases(fx):
    return [str(s) for s in fx["cases"]]


def test_abi_declares_and_exports_range_image(pcr):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcr.h")).read(), flags=re.S)
    L = pcr.lib()
    for sym in NEW_CALLS:
        assert re.search(r"\b" + sym + r"\s*\(", text), f"{sym} is not declared in include/pcr.h"
        assert hasattr(L, sym), f"{sym} is not exported by libpcr_hip.so"
        assert sym in pcr.ABI_SYMBOLS
    assert "typedef struct pcr_range_image pcr_range_image;" in text


def test_hw4_signatures_are_the_references(pcr):
    import importlib
    import inspect
    hw4 = importlib.import_module(pcr.__name__ + ".hw4")
    want = {"pcd_to_range_image": ["pcd_points", "resolution"],
            "range_image_labeling": ["range_image", "idx_image", "depth_list", "phi", "theta", "nn_mode"],
            "cluster_assignment": ["idx_image", "image_label", "pcd_size"],
            "depth_completion": ["image", "pad"],
            "cluster_range_image": ["points", "resolution", "theta", "nn_mode"]}
    for name, args in want.items():
        sig = inspect.signature(getattr(hw4, name))
        pos = [p.name for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert pos == args, name
        assert all(p.kind == p.KEYWORD_ONLY for p in sig.parameters.values() if p.name == "ctx")
    d = inspect.signature(hw4.cluster_range_image).parameters
    assert (d["resolution"].default, d["theta"].default, d["nn_mode"].default) == (0.7, 30, 7)       # __main__ :163-166


def test_vectorised_restatement_equals_the_loops():
    rng = np.random.default_rng(11)
    for rows, cols, nn, theta in ((1, 9, 3, 10.0), (7, 5, 2, 25.0), (12, 23, 4, 30.0), (9, 8, 8, 5.0), (20, 31, 7, 40.0)):
        img = random_image(rng, rows, cols, 0.6)
        got, _ = label_ref(img, 0.7, theta, nn)
        assert np.array_equal(got, label_loops(img, 0.7, theta, nn)), (rows, cols, nn)


def test_restatement_against_the_references_output(fixture):
    """On every fixture image: the reference's labels and the components correspond one to one on the pixels the reference labelled, and every
    occupied pixel it left at -1 lies in a component it labelled nowhere."""
    fx = fixture
    for name in fixture_cases(fx):
        img = fx[name + "_image"]
        ref = fx[name + "_ref_label"].astype(np.int64)
        phi, theta, nn = float(fx[name + "_params"][0]), float(fx[name + "_params"][1]), int(fx[name + "_params"][2])
        mine, inband = label_ref(img, phi, theta, nn)
        assert inband == 0, name                                        # the generator refuses images with a pair inside the band
        lab = ref >= 0
        assert np.array_equal(mine[lab] >= 0, np.ones(int(lab.sum()), bool))
        pairs = np.unique(np.stack([ref[lab], mine[lab]]), axis=1)
        assert pairs.shape[1] == np.unique(ref[lab]).size == np.unique(mine[lab]).size, f"{name}: no bijection on the labelled pixels"
        left = (ref < 0) & (img > 0)
        dropped = np.unique(mine[left])
        assert not np.isin(dropped, mine[lab]).any(), f"{name}: a pixel the reference left out lies in a component it labelled"
        assert np.array_equal(mine < 0, ~(img > 0))
        n_comp = int(mine.max()) + 1 if (mine >= 0).any() else 0
        assert (int(fx[name + "_counts"][0]), int(fx[name + "_counts"][1])) == (np.unique(ref[lab]).size, n_comp)
        assert int(fx[name + "_counts"][2]) == dropped.size and int(fx[name + "_counts"][3]) == int(left.sum())
        print(f"{name}: {img.shape[0]} x {img.shape[1]}, reference labels {np.unique(ref[lab]).size} of {n_comp} components; "
              f"{dropped.size} components ({int(left.sum())} pixels) never seeded; removed from the input: {int(fx[name + '_counts'][4])}")
        if name + "_points" in fx.files:                                # clouds: the projection and the reference's cluster_assignment
            pr = project_ref(fx[name + "_points"], phi)
            assert np.array_equal(pr["image"], img) and not pr["band"].any()
            want = assign_ref(pr["pix"], ref)
            assert np.array_equal(want, fx[name + "_ref_cluster"])


# ------------------------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def ctx(pcr):
    c = pcr.Context(0)
    yield c
    c.close()


_cloud_refs = {}


def cloud_ref(fx, name):
    """the restatement on a fixture cloud, computed once"""
    if name not in _cloud_refs:
        phi, theta, nn = float(fx[name + "_params"][0]), float(fx[name + "_params"][1]), int(fx[name + "_params"][2])
        pr = project_ref(fx[name + "_points"], phi)
        lab, inband = label_ref(pr["image"], phi, theta, nn)
        _cloud_refs[name] = (pr, lab, inband, (phi, theta, nn))
    return _cloud_refs[name]


def staged(ctx, pts, resolution, theta, nn, phi=None):
    cloud = ctx.cloud(np.ascontiguousarray(pts, np.float32), 1)
    try:
        ri = ctx.range_image(cloud, resolution)
    finally:
        cloud.free()
    try:
        img, pix = ri.image(), ri.pixels()
        label, nl = ri.label(resolution if phi is None else phi, theta, nn)
        return {"image": img, "pix": pix, "label": label, "n_labels": nl, "cluster": ri.assign(), "dropped": ri.n_dropped}
    finally:
        ri.free()


def label_host_image(ctx, img, phi, theta, nn):
    ri = ctx.range_image_from_host(img)
    try:
        return ri.label(phi, theta, nn)
    finally:
        ri.free()


def assert_label_equal(ctx, img, phi, theta, nn, what=""):
    want, inband = label_ref(img, phi, theta, nn)
    assert inband == 0, what
    got, nl = label_host_image(ctx, img, phi, theta, nn)
    assert np.array_equal(got, want), what
    assert nl == (int(want.max()) + 1 if (want >= 0).any() else 0)
    return want


@pytest.mark.gpu
def test_fixture_clouds_pixel_image_labels_equal(ctx, fixture):
    fx = fixture
    clouds = [n for n in fixture_cases(fx) if n + "_points" in fx.files]
    assert len(clouds) >= 3
    for name in clouds:
        pr, lab, inband, (phi, theta, nn) = cloud_ref(fx, name)
        got = staged(ctx, fx[name + "_points"], phi, theta, nn)
        assert np.array_equal(got["pix"], pr["pix"]), f"{name}: pixel of a point differs"
        assert got["image"].shape == pr["image"].shape
        assert np.array_equal(got["image"].view(np.uint64), pr["image"].view(np.uint64)), f"{name}: cropped image differs"
        assert got["dropped"] == pr["dropped"]
        assert np.array_equal(got["label"], lab), f"{name}: image_label differs"
        assert np.array_equal(got["cluster"], assign_ref(pr["pix"], lab)), f"{name}: cluster_idx differs"
        assert np.array_equal(got["image"], fx[name + "_image"])


@pytest.mark.gpu
def test_fixture_images_labels_equal(ctx, fixture):
    fx = fixture
    for name in fixture_cases(fx):
        if name + "_points" in fx.files:
            continue
        phi, theta, nn = float(fx[name + "_params"][0]), float(fx[name + "_params"][1]), int(fx[name + "_params"][2])
        assert_label_equal(ctx, fx[name + "_image"], phi, theta, nn, name)


@pytest.mark.gpu
def test_one_call_and_hw4_mirrors_agree_with_the_staged_calls(ctx, pcr, fixture):
    import importlib
    hw4 = importlib.import_module(pcr.__name__ + ".hw4")
    fx = fixture
    name = [n for n in fixture_cases(fx) if n + "_points" in fx.files][0]
    pr, lab, _, (phi, theta, nn) = cloud_ref(fx, name)
    pts = fx[name + "_points"]
    want = assign_ref(pr["pix"], lab)
    cloud = ctx.cloud(pts, 1)
    try:
        got, nc, st = ctx.range_cluster(cloud, phi, theta, nn)
    finally:
        cloud.free()
    assert np.array_equal(got, want) and nc == int(lab.max()) + 1
    assert (st["rows"], st["cols"], st["dropped"]) == (*pr["image"].shape, pr["dropped"])
    assert st["full_pixels"] == pr["full_shape"][0] * pr["full_shape"][1]
    assert np.array_equal(hw4.cluster_range_image(pts, phi, theta, nn, ctx=ctx), want)
    # __main__ :164-167 with the reference's names
    range_image, idx_image, depth_list = hw4.pcd_to_range_image(pts.astype(np.float64), phi, ctx=ctx)
    image_label = hw4.range_image_labeling(range_image, idx_image, depth_list, phi, theta, nn_mode=nn, ctx=ctx)
    cluster_idx = hw4.cluster_assignment(idx_image, image_label, pts.shape[0])
    assert np.array_equal(range_image, pr["image"]) and np.array_equal(depth_list, pr["d"])
    assert np.array_equal(image_label, lab) and np.array_equal(cluster_idx, want)
    assert np.array_equal(hw4.cluster_assignment(idx_image, image_label.copy() + 0, pts.shape[0]), want)
    assert idx_image.shape == range_image.shape
    order = np.argsort(pr["pix"], kind="stable")
    for p in (int(pr["pix"][pr["pix"] >= 0][0]), int(np.flatnonzero(pr["image"].ravel() == -1)[0])):
        members = order[np.searchsorted(pr["pix"][order], p):np.searchsorted(pr["pix"][order], p + 1)]
        cell = idx_image[p // range_image.shape[1], p % range_image.shape[1]]
        if members.size == 0:
            assert cell is None
        else:
            assert cell.dtype == object and cell[0] is None and list(cell[1:]) == sorted(int(i) for i in members)
    # from_host of the image that create + read returned labels the same way
    assert np.array_equal(label_host_image(ctx, range_image, phi, theta, nn)[0], lab)
    assert np.array_equal(hw4.range_image_labeling(range_image.copy(), None, None, phi, theta, nn, ctx=ctx), lab)


@pytest.mark.gpu
def test_small_shapes(ctx):
    rng = np.random.default_rng(5)
    # a 1-row image, a 1-column-tile image (cols <= 16), images smaller and just larger than one 16 x 16 tile
    for rows, cols, nn in ((1, 40, 3), (1, 8, 8), (40, 9, 4), (33, 16, 7), (16, 16, 1), (17, 17, 8), (5, 3, 3), (3, 1, 1)):
        img = random_image(rng, rows, cols, 0.7)
        assert_label_equal(ctx, img, 0.7, 20.0, nn, f"{rows} x {cols} nn {nn}")
    # cols between nn_mode and 2 nn_mode + 1: the window meets the same pixel twice (and, at cols == nn_mode, its own centre)
    for nn in (1, 2, 5, 8):
        for cols in range(nn, 2 * nn + 2):
            img = random_image(rng, 6, cols, 0.8)
            assert_label_equal(ctx, img, 0.7, 15.0, nn, f"6 x {cols} nn {nn}")


@pytest.mark.gpu
def test_seam_and_tile_borders(ctx):
    # one flat band across the column seam: the two ends are ONE component only through the wrap
    img = np.full((20, 50), -1.0)
    img[3, :4] = 10.0
    img[3, -5:] = 10.0
    img[12, 20:30] = 10.0
    want = assert_label_equal(ctx, img, 0.7, 30.0, 2, "seam")
    assert want[3, 0] == want[3, -1] == 0 and want[12, 25] == 1 and want.max() == 1
    # a component that crosses every tile border: a full flat image of 3 x 4 tiles (+ a ragged edge), every nn_mode
    img = np.full((45, 70), 10.0)
    for nn in (1, 3, 8):
        want = assert_label_equal(ctx, img, 0.7, 30.0, nn, f"flat nn {nn}")
        assert want.max() == 0
    # a diagonal staircase through all tiles, linked only at nn_mode >= 1 through corners
    img = np.full((64, 64), -1.0)
    img[np.arange(64), np.arange(64)] = 10.0
    want = assert_label_equal(ctx, img, 0.7, 30.0, 1, "diagonal")
    assert want.max() == 0
    # range 0 (a point at the origin) is neither empty nor labelled; a step >= 1 m is no link
    img = np.array([[5.0, 5.0, 0.0, 5.0, 6.0, 7.5]])
    want = assert_label_equal(ctx, img, 0.7, 1.0, 1, "zero")
    assert list(want[0]) == [0, 0, -1, 1, 2, 3]


@pytest.mark.gpu
def test_spiral_worst_case_for_the_union_find(ctx):
    img = spiral_image(64, 512)
    want = assert_label_equal(ctx, img, 0.7, 30.0, 1, "spiral")
    assert want.max() == 0 and (img > 0).sum() > 8000


@pytest.mark.gpu
def test_projection_edge_cases(ctx):
    res = 0.7                                                           # width 515, offset 258: alpha in [179.9, 180] deg gives x = -1
    rr = math.pi / 180 * res

    def at(az_pix, el_pix, rng_):                                        # the centre of the cell floor(alpha / rr) = az_pix, floor(beta / rr) = el_pix
        a, e = (az_pix + 0.5) * rr, (el_pix + 0.5) * rr
        return [rng_ * math.cos(e) * math.cos(a), rng_ * math.cos(e) * math.sin(a), rng_ * math.sin(e)]
    pts = [at(10, 2, 8.0), at(10, 2, 9.0), at(10, 2, 7.0),              # several points per pixel: the last index wins (7.0)
           at(11, 2, 7.2), at(30, 2, 7.5), at(60, -3, 7.7),             # emptied columns and rows in between: far pixels become adjacent
           [-5.0, 0.004, 0.1],                                         # alpha = 179.95 deg: x = -1, the last column
           [0.0, 0.0, 0.0],                                            # the origin: range 0
           [0.1, 0.0, -30.0], [0.0, 0.1, -9.0],                        # beta below -60 deg: an index past the image, dropped
           [float("nan"), 1.0, 1.0], [1.0, float("inf"), 1.0], [1.0, 1.0, float("-inf")],
           at(-40, 5, 15.0), at(-41, 5, 15.3)]
    pts = np.array(pts, np.float32)
    pr = project_ref(pts, res)
    height, width = pr["full_shape"]
    assert (height, width) == (86, 515) and pr["dropped"] == 5 and (pr["pix"][8:13] == -1).all()
    assert not pr["band"][[0, 1, 2, 3, 4, 5, 6, 13, 14]].any()
    assert pr["pix"][0] == pr["pix"][1] == pr["pix"][2] and pr["image"].ravel()[pr["pix"][2]] == pr["d"][2]
    assert pr["pixfull"][6] % width == width - 1                        # x = -1 wrapped as numpy's negative index
    assert pr["image"].ravel()[pr["pix"][7]] == 0.0
    got = staged(ctx, pts, res, 10.0, 2)
    assert np.array_equal(got["pix"], pr["pix"]) and got["dropped"] == 5
    assert np.array_equal(got["image"].view(np.uint64), pr["image"].view(np.uint64))
    lab, inband = label_ref(pr["image"], res, 10.0, 2)
    assert inband == 0
    assert np.array_equal(got["label"], lab) and np.array_equal(got["cluster"], assign_ref(pr["pix"], lab))
    assert got["cluster"][7] == -1 and (got["cluster"][8:13] == -1).all()
    assert got["cluster"][0] == got["cluster"][2] == got["cluster"][3] == got["cluster"][4] >= 0      # 19 columns apart before the crop, adjacent after it
    # a random cloud with 5 % duplicates of directions (several points per pixel), several blocks of 256 points
    rng = np.random.default_rng(3)
    big = sphere_points(rng, 1500, 1.0)
    big[::20] = big[1::20] * np.float32(1.01)
    pr = project_ref(big, 1.0)
    keep = ~pr["band"]
    big, pr = big[keep], project_ref(big[keep], 1.0)
    got = staged(ctx, big, 1.0, 25.0, 3)
    assert np.array_equal(got["pix"], pr["pix"]) and np.array_equal(got["image"].view(np.uint64), pr["image"].view(np.uint64))


@pytest.mark.gpu
def test_error_codes(ctx, pcr):
    pts = sphere_points(np.random.default_rng(1), 300, 1.0)
    cloud = ctx.cloud(pts, 1)
    for res in (0.0, -1.0, float("nan"), float("inf"), 1e-4):           # 1e-4: 3.6e6 x 6e5 pixels > 2^31 - 16
        with pytest.raises(pcr.PcrError, match="bad argument"):
            ctx.range_image(cloud, res)
    ri = ctx.range_image(cloud, 1.0)
    for theta in (-1.0, 90.0, 120.0, float("nan")):
        with pytest.raises(pcr.PcrError, match="bad argument"):
            ri.label(1.0, theta, 3)
    for nn in (0, -2, 9):
        with pytest.raises(pcr.PcrError, match="bad argument"):
            ri.label(1.0, 30.0, nn)
    with pytest.raises(pcr.PcrError, match="bad argument"):
        ri.label(float("inf"), 30.0, 3)
    with pytest.raises(pcr.PcrError, match="bad state"):
        ri.assign()                                                     # not labelled yet
    with pytest.raises(pcr.PcrError, match="bad argument"):
        ri.close_gaps(17)
    ri.label(1.0, 89.999, 8)
    ri.free()
    narrow = ctx.range_image_from_host(np.full((4, 3), 5.0))
    with pytest.raises(pcr.PcrError, match="bad argument"):
        narrow.label(1.0, 30.0, 4)                                      # narrower than nn_mode columns
    narrow.label(1.0, 30.0, 3)
    assert narrow.assign().size == 0                                    # an image from the host has no points
    narrow.free()
    with pytest.raises(pcr.PcrError, match="bad argument"):
        ctx.range_image_from_host(np.zeros((0, 4)))
    for t, nn in ((95.0, 3), (30.0, 0)):
        with pytest.raises(pcr.PcrError, match="bad argument"):
            ctx.range_cluster(cloud, 1.0, t, nn)
    cloud.free()
    for bad in (np.zeros((0, 3), np.float32), np.full((5, 3), np.nan, np.float32), np.array([[0.1, 0.0, -30.0]], np.float32)):
        c = ctx.cloud(bad, 1)
        with pytest.raises(pcr.PcrError, match="no correspondence kept"):    # PCR_ERR_EMPTY: no point lands in the image
            ctx.range_image(c, 1.0)
        with pytest.raises(pcr.PcrError, match="no correspondence kept"):
            ctx.range_cluster(c, 1.0, 30.0, 3)
        c.free()


@pytest.mark.gpu
def test_closing_against_the_loops(ctx, pcr):
    import importlib
    hw4 = importlib.import_module(pcr.__name__ + ".hw4")
    rng = np.random.default_rng(9)
    for rows, cols in ((37, 50), (16, 16), (3, 40), (4, 4)):
        img = random_image(rng, rows, cols, 0.6)
        for pad in (1, 2):
            got = hw4.depth_completion(img, pad, ctx=ctx)
            assert np.array_equal(got.view(np.uint64), close_ref(img, pad).view(np.uint64)), (rows, cols, pad)
    assert np.array_equal(hw4.depth_completion(img, 0, ctx=ctx), img)


def theta_at(angle):
    """a theta (degrees) whose threshold theta * pi / 180 lies within a few ulp of `angle`"""
    t = angle * 180 / math.pi
    best = t
    for _ in range(8):
        for cand in (np.nextafter(best, 0.0), np.nextafter(best, 1e9)):
            if abs(float(cand) * math.pi / 180 - angle) < abs(best * math.pi / 180 - angle):
                best = float(cand)
    return best


@pytest.mark.gpu
def test_randomised_sweep_with_pairs_inside_the_band(ctx):
    """About 30 images up to 96 x 600, random theta, nn_mode 1 ... 8; in every third image theta is placed ON the angle of one of the image's
    own pairs (inside the band).  The library's partition lies between the components of the certain links and those of the certain plus
    the in-band links; without a pair in the band the labels are equal."""
    rng = np.random.default_rng(20261017)
    seen_band = 0
    for trial in range(30):
        rows, cols = int(rng.integers(1, 97)), int(rng.integers(8, 601))
        if trial % 5 == 0:
            rows, cols = int(rng.integers(1, 20)), int(rng.integers(8, 40))
        nn = int(rng.integers(1, min(8, cols) + 1))
        phi = float(rng.choice([0.2, 0.7, 1.5]))
        theta = float(rng.uniform(0.0, 60.0))
        img = random_image(rng, rows, cols, float(rng.uniform(0.15, 0.9)))
        if trial % 3 == 0:
            a, b, _, _, _ = edges_ref(img, phi, theta, nn)
            if a.size:
                k = int(rng.integers(a.size))
                d1, d2 = max(img.ravel()[a[k]], img.ravel()[b[k]]), min(img.ravel()[a[k]], img.ravel()[b[k]])
                ang = math.atan2(d2 * math.sin(phi * math.pi / 180), d1 - d2 * math.cos(phi * math.pi / 180))
                if 0.0 < ang < 1.5:
                    theta = theta_at(ang)
        a, b, cert, inb, linked = edges_ref(img, phi, theta, nn)
        got, nl = label_host_image(ctx, img, phi, theta, nn)
        tag = f"trial {trial}: {rows} x {cols}, nn {nn}, phi {phi}, theta {theta!r}, {int(inb.sum())} pairs in the band"
        lo = components_ref(img, a[cert], b[cert])
        if inb.any():
            seen_band += 1
            hi = components_ref(img, a[cert | inb], b[cert | inb])
            assert refines(lo, got) and refines(got, hi), tag
            first = np.unique(got[got >= 0], return_index=True)[1]      # numbered by first pixel in raster order all the same
            assert np.array_equal(got[got >= 0][np.sort(first)], np.arange(first.size)), tag
        else:
            assert np.array_equal(got, lo), tag
        assert nl == (int(got.max()) + 1 if (got >= 0).any() else 0), tag
    assert seen_band >= 5


@pytest.mark.gpu
def test_rerun_on_a_reused_context_gives_the_same_bits(ctx, pcr, fixture, synth):
    fx = fixture
    name = [n for n in fixture_cases(fx) if n + "_points" in fx.files][-1]
    _, _, _, (phi, theta, nn) = cloud_ref(fx, name)
    pts = fx[name + "_points"]
    first = staged(ctx, pts, phi, theta, nn)
    src, tgt = synth.kitti_like_pair(3000)                              # other work in between: the scratch is reused and regrown
    cs, ct = ctx.cloud(src), ctx.cloud(tgt)
    ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=2, eps=1e-8)
    ctx.dbscan(ct, 0.8, 10)
    cs.free(), ct.free()
    again = staged(ctx, pts, phi, theta, nn)
    for k in ("image", "pix", "label", "cluster"):
        assert np.array_equal(first[k], again[k]), k
    ctx.tune("ri_prefilter", -1)                                        # every pair through atan2: the pre-filter decides nothing wrongly
    try:
        plain = staged(ctx, pts, phi, theta, nn)
    finally:
        ctx.tune("ri_prefilter", 1)
    assert np.array_equal(plain["label"], first["label"])
