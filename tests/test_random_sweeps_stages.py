"""Randomised sweeps over the stages added after tests/test_random_sweeps.py was written: DBSCAN and statistical outlier removal (hw4),
FPFH33, Harris3D, the voxel grid with normals and normal-space sampling (hw9), ball query, grouping and object extraction (PointNet++).

Every GPU result is compared with the numpy restatement of its contract in include/pcr.h, imported from the test module that owns it
(nothing is restated here).  What the fixed scenes of those modules do not reach, and these trials do:
  * rows of the cell grid above the 384-record threshold, where the radius walks binary-search an x-window ("dense" clouds: at least
    9 * 384 + 1 points inside a ball narrower than the radius, so by pigeonhole one of the nine rows a member walks is clipped, plus
    probe points whose x-offset from a member is within 0.15 % of the radius: a window that is a little too narrow loses them);
  * pairs whose squared distance EQUALS r2 (half-integer lattices with r in 0.5, 1.0, 1.5): strict and inclusive membership differ;
  * sizes 1, 2, 3, 63 .. 65, 255 .. 257, 1023, 1025 together with every lane count;
  * coordinates from 1e-12 to 1e11; non-finite points, non-finite / zero / oversized normals in every trial;
  * one context across a whole sweep of shrinking and growing problems.
A trial is a function of (PCR_SWEEP_SEED, sweep, trial number) alone: every assertion message names them, and `<sweep>_trial(number)`
rebuilds the inputs.  PCR_SWEEP_SCALE multiplies the trial counts.

CPU tests: the properties the GPU sweeps rely on, checked on the generators and the restatements (dense trials have a neighbourhood of
>= 3 457, lattice trials have >= 100 pairs exactly on the boundary, the fragile share of SPFH rows stays under the cap, no voxel trial
overflows).  GPU tests print their own reach (largest neighbourhood, trials with a clipped row, pairs on the boundary): run with -s."""
import os

import numpy as np
import pytest

from test_fpfh import check_fpfh, check_spfh, fpfh_numpy, neighbours, spfh_numpy
from test_harris3d import harris_numpy
from test_hw4_foreground import assert_dbscan_equal, assert_sor_equal, dbscan_ref, run_dbscan, run_sor, sor_ref
from test_normal_space_sampling import nss_numpy
from test_pointnet_sampling import ball_ref, group_ref, objects_ref
from test_random_sweeps import random_cloud32
from test_voxel_grid_normals import voxel_grid_numpy

# soak runs: PCR_SWEEP_SCALE multiplies the number of trials, PCR_SWEEP_SEED shifts every generator seed
SCALE = int(os.environ.get("PCR_SWEEP_SCALE", "1"))
SEED = int(os.environ.get("PCR_SWEEP_SEED", "0"))

F32 = np.float32
AOS3 = 1                                                            # PCR_AOS3
KIND = ("normal", "lattice", "clustered", "scaled", "dense")
FIXED_N = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025)          # every sweep begins with these sizes
FIXED_KIND = (0, 2, 3, 0, 2, 3, 1, 0, 1, 2, 1)                      # (a lattice trial needs a few hundred points to hold ties: it takes the larger ones)
LANES = (1, 2, 4, 8, 16, 32)
LATTICE_R = (0.5, 1.0, 1.5, 0.75)                                   # r2 exact in f32; axis neighbours sit exactly on the first three, nobody on 0.75
ON_BOUNDARY_R = (0.5, 1.0, 1.5)
CLIP = 384                                                          # clip_row_x<384> (grid_walk.hpp) searches rows longer than this
DENSE_MIN = 9 * CLIP + 1                                            # neighbours that force a clipped row among the nine a point walks
FRAGILE_CAP = 1e-3                                                  # the share of SPFH rows the restatement may mark fragile


# ---------------------------------------------------------------------------------------------------- generators
def trial_rng(sweep, trial):
    return np.random.default_rng([SEED, sweep, trial])


def plan(trial, rng, n_max, dense=True):
    """(kind, n) of a trial: every tenth trial is dense, the first eleven of the others take the fixed sizes, the rest kinds 0-3 in turn"""
    if dense and trial % 10 == 9:
        return 4, 0
    i = trial - trial // 10 if dense else trial
    if i < len(FIXED_N):
        return FIXED_KIND[i], FIXED_N[i]
    kind = i % 4
    return kind, int(rng.integers(300 if kind == 1 else 1, n_max))


def extent(pts):
    fin = pts[np.isfinite(pts).all(1)]
    ext = float(np.ptp(fin, axis=0).max()) if len(fin) else 0.0
    if not ext > 0:
        ext = float(np.abs(fin).max()) if len(fin) and np.abs(fin).max() > 0 else 1.0
    return ext


def dense_cloud(rng):
    """a ball of diameter 0.9 r with >= DENSE_MIN + 64 points, 200 probes at an x-offset of (0.9985 .. 1.0005) r from a ball point (and a
    transverse offset below 0.006 r: inside or outside the radius by a hair, far out in the x-window), 300 scattered points"""
    r = float(F32(rng.uniform(0.3, 1.5)))
    c = rng.normal(0, 5, 3)
    k = DENSE_MIN + 64 + int(rng.integers(0, 100))
    d = rng.normal(size=(k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ball = c + d * (0.45 * r * rng.uniform(0, 1, (k, 1)) ** (1 / 3))
    probes = ball[rng.integers(0, k, 200)] + boundary_offsets(rng, 200, r)
    far = c + rng.uniform(-40, 40, (300, 3)) * r
    pts = np.concatenate([ball, probes, far])
    order = rng.permutation(len(pts))
    return np.ascontiguousarray(pts[order].astype(F32)), r, np.flatnonzero(order < k)


def boundary_offsets(rng, k, r):
    return np.c_[rng.choice([-1.0, 1.0], k) * rng.uniform(0.9985, 1.0005, k), rng.uniform(-0.004, 0.004, (k, 2))] * r


def make_cloud(rng, kind, n, bad_points=True):
    """-> (points [n, 3] f32, radius: a Python float holding an f32 value, indices of the dense ball's points or None)"""
    ball = None
    if kind == 4:
        pts, r, ball = dense_cloud(rng)
    else:
        pts = np.ascontiguousarray(random_cloud32(rng, n, kind).T)
        r = float(rng.choice(LATTICE_R)) if kind == 1 else float(F32(rng.uniform(0.02, 0.4) * extent(pts)))
    if bad_points:
        n = len(pts)
        for i in rng.integers(0, n, int(rng.integers(0, 2 + n // 100))):
            pts[i, int(rng.integers(0, 3))] = rng.choice([np.nan, np.inf, -np.inf])
    return pts, r, ball


def make_normals(rng, n, kind):
    """unit random normals (lattice clouds: signed axis vectors: exact atan2 arguments, exact half-way bins) with a sprinkle of non-finite,
    zero and oversized ones (|component| = 2 still contributes to Harris3D and the voxel grid, above 2 it does not)"""
    if kind == 1:
        nrm = np.zeros((n, 3), F32)
        nrm[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
    else:
        v = rng.normal(size=(n, 3))
        nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    for i in rng.integers(0, n, int(rng.integers(0 if n < 8 else 1, 3 + n // 50))):
        what, ax = int(rng.integers(0, 4)), int(rng.integers(0, 3))
        if what == 0:
            nrm[i, ax] = np.nan
        elif what == 1:
            nrm[i, ax] = rng.choice([np.inf, -np.inf])
        elif what == 2:
            nrm[i] = 0
        else:
            nrm[i, ax] = rng.choice([2.0, -2.0, 2.5, -3.0, 1e30])
    return nrm


def foreign_keypoints(rng, pts, r, kind, ball):
    """keypoints that are not surface points: near, far, non-finite; lattice sites that hold no surface point; for dense clouds probes at
    an x-offset of about r from a ball point"""
    fin = pts[np.isfinite(pts).all(1)].astype(np.float64)
    if not len(fin):
        fin = np.zeros((1, 3))
    parts = [fin[rng.integers(0, len(fin), 40)] + rng.uniform(-0.6, 0.6, (40, 3)) * r,
             rng.uniform(fin.min(0) - 30 * r, fin.max(0) + 30 * r, (20, 3)), [[np.nan, 0, 0], [np.inf, 1, 1]]]
    if kind == 1:
        present = {tuple(p) for p in fin.tolist()}
        parts.append([p for p in (rng.integers(-3, 9, (60, 3)) * 0.5).tolist() if tuple(p) not in present] or [[-1.5, -1.5, -1.5]])
    if ball is not None:
        src = pts[ball][np.isfinite(pts[ball]).all(1)].astype(np.float64)
        parts.append(src[rng.integers(0, len(src), 60)] + boundary_offsets(rng, 60, r))
    return np.ascontiguousarray(np.concatenate(parts).astype(F32))


def fpfh_trial(trial):
    rng = trial_rng(1101, trial)
    kind, n = plan(trial, rng, 2500)
    pts, r, ball = make_cloud(rng, kind, n)
    return dict(trial=trial, kind=kind, pts=pts, r=r, ball=ball, nrm=make_normals(rng, len(pts), kind), lanes=int(rng.choice(LANES)),
                kp=foreign_keypoints(rng, pts, r, kind, ball))


def harris_trial(trial):
    rng = trial_rng(1202, trial)
    kind, n = plan(trial, rng, 2500)
    pts, r, ball = make_cloud(rng, kind, n)
    return dict(trial=trial, kind=kind, pts=pts, r=r, ball=ball, nrm=make_normals(rng, len(pts), kind), lanes=int(rng.choice(LANES)),
                method=int(rng.integers(0, 3)), nms=bool(rng.integers(0, 2)), thr_kind=int(rng.integers(0, 5)), quantile=float(rng.uniform(0.05, 0.95)),
                perm=rng.permutation(len(pts)) if trial % 4 == 0 else None)


def dbscan_trial(trial):
    rng = trial_rng(1303, trial)
    kind, n = plan(trial, rng, 3000)
    pts, r, ball = make_cloud(rng, kind, n)
    return dict(trial=trial, kind=kind, pts=pts, r=r, ball=ball, min_points=int(rng.integers(1, 51)), lanes=int(rng.choice(LANES)))


def sor_trial(trial):
    rng = trial_rng(1404, trial)
    kind, n = plan(trial, rng, 3000, dense=False)
    pts, _, _ = make_cloud(rng, kind, n)
    k = int(rng.integers(1, 33))
    if trial % 3 == 0 and n >= 2:                                   # more than k exact duplicates (all of the cloud when it is smaller): avg = 0
        idx = rng.permutation(n)[: k + 1 + int(rng.integers(0, 4))]
        pts[idx] = pts[idx[0]]
    return dict(trial=trial, kind=kind, pts=pts, k=k, std_ratio=float(rng.uniform(0.5, 4.0)))


def vgn_trial(trial):
    rng = trial_rng(1505, trial)
    kind, n = plan(trial, rng, 6000, dense=False)
    pts, _, _ = make_cloud(rng, kind, n)
    fin = pts[np.isfinite(pts).all(1)]
    ext, amax = extent(pts), (float(np.abs(fin).max()) if len(fin) else 0.0)
    # leaf >= extent / 100 keeps div_x * div_y * div_z <= 102^3, leaf >= |coordinate| / 1e6 keeps every voxel coordinate inside int32:
    # the call must succeed
    leaf = float(F32(max(rng.uniform(0.01, 0.5) * ext, ext / 1000, amax * 1e-6)))
    return dict(trial=trial, kind=kind, pts=pts, leaf=leaf, mode=trial % 2, nrm=make_normals(rng, n, kind) if trial % 3 else None,
                perm=rng.permutation(n) if trial % 4 == 0 else None)


def nss_trial(trial):
    rng = trial_rng(1606, trial)
    kind, n = plan(trial, rng, 5000, dense=False)
    pts, _, _ = make_cloud(rng, kind, n)
    return dict(trial=trial, kind=kind, pts=pts, nrm=make_normals(rng, n, kind), bins=tuple(int(b) for b in rng.integers(1, 33, 3)),
                sample=int(rng.integers(0, n + 6)), seed=int(rng.integers(0, 2 ** 64, dtype=np.uint64)))


def ball_trial(trial):
    """1-12 ragged segments (empty ones among them) of one cloud.  Two trials in three are `clean` (every centre is a finite member or
    lies within 0.52 r of one, so no row is empty and the rows can be grouped); the others add far and non-finite centres"""
    rng = trial_rng(1707, trial)
    kind, n = plan(trial, rng, 3000, dense=False)
    pts, r, _ = make_cloud(rng, kind, n)
    nseg = int(rng.integers(1, 13))
    cuts = np.sort(rng.integers(0, n + 1, nseg - 1))
    if nseg >= 3 and trial % 2:
        cuts[int(rng.integers(1, nseg - 1))] = cuts[0]             # an empty segment for sure
        cuts = np.sort(cuts)
    seg = np.concatenate([[0], cuts, [n]]).astype(np.uint32)
    clean = trial % 3 != 0
    cen, cseg = [], [0]
    for s in range(nseg):
        p = pts[seg[s]:seg[s + 1]]
        fin = p[np.isfinite(p).all(1)].astype(np.float64)
        rows = []
        if len(fin):
            m = int(rng.integers(40, 65)) if kind == 1 else int(rng.integers(1, 13))      # (enough lattice centres for >= 100 pairs on the boundary)
            rows.append(fin[rng.integers(0, len(fin), m)])                                                  # members
            rows.append(fin[rng.integers(0, len(fin), m // 2)] + rng.uniform(-0.3, 0.3, (m // 2, 3)) * r)   # foreign, within reach of one
            if kind == 1:
                rows.append(rng.integers(-1, 7, (m, 3)) * 0.5)                                              # lattice sites (a row may be empty)
        if not clean:
            base = fin[0] if len(fin) else np.zeros(3)
            rows.append([base + 1000.0 * r, [np.nan, 0, 0], [0, np.inf, 0]][: int(rng.integers(1 if s == 0 else 0, 4))])
        rows = [np.asarray(x, np.float64).reshape(-1, 3) for x in rows]
        c = np.concatenate(rows) if rows else np.zeros((0, 3))
        cen.append(c[rng.permutation(len(c))])
        cseg.append(cseg[-1] + len(c))
    D = int(rng.integers(0, 8))
    return dict(trial=trial, kind=kind, pts=pts, r=r, seg=seg, cen=np.ascontiguousarray(np.concatenate(cen).astype(F32)).reshape(-1, 3),
                cseg=np.asarray(cseg, np.uint32), nsample=int(rng.integers(1, 129)), D=D,
                feat=rng.normal(size=(n, D)).astype(F32) if D else None)


def objects_trial(trial):
    rng = trial_rng(1808, trial)
    npoints = int(rng.choice([1, 8, 64, 100, 256]))
    sizes = [0, 1, npoints - 1, npoints, npoints + 1, int(rng.integers(1000, 4000))] + [int(v) for v in rng.integers(1, 3 * npoints + 2, int(rng.integers(0, 5)))]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))] + [0] * int(rng.integers(0, 3))
    noise = int(rng.integers(0, 300))
    n = sum(sizes) + noise
    kind = trial % 4
    pts = np.ascontiguousarray(random_cloud32(rng, n, kind).T)
    labels = np.concatenate([np.full(s, c, np.int32) for c, s in enumerate(sizes)] + [np.full(noise, -1, np.int32)])[rng.permutation(n)]
    for i in np.flatnonzero(labels == -1)[:3]:                      # non-finite points are noise (what pcr_dbscan_f32 makes of them)
        pts[i, 1] = np.nan
    z = pts[labels >= 0, 2].astype(np.float64)
    zext = float(np.ptp(z)) or 1.0
    ground_z = float(rng.choice([1e30, np.median(z), z.min(), z.min() - 0.3 * zext]))
    thr = float(rng.uniform(0, 1) * zext)
    z_extent = (0.0, 1e30) if trial % 3 == 0 else (float(rng.uniform(0, 0.3) * zext), float(rng.uniform(0.5, 1.5) * zext))
    starts = None
    if trial % 2:
        starts = np.full(len(sizes), 0xFFFFFFFF, np.uint32)
        for c, s in enumerate(sizes):
            if s > npoints and rng.integers(0, 2):
                starts[c] = rng.integers(0, s)
    return dict(trial=trial, kind=kind, pts=pts, labels=labels, n_clusters=len(sizes), npoints=npoints, ground_z=ground_z, thr=thr, z_extent=z_extent,
                seed=int(rng.integers(0, 2 ** 64, dtype=np.uint64)), starts=starts)


# ---------------------------------------------------------------------------------------------------- what a trial reaches
def boundary_pairs(a, b, r, wide=False):
    """ordered pairs (a_i, b_j) whose squared distance EQUALS r2, in the arithmetic of the row: f32 with r2 = (float)(r * r) (FPFH33,
    Harris3D, ball query) or f64 (DBSCAN).  On such a pair `<` and `<=` disagree"""
    T = np.float64 if wide else F32
    a, b = np.asarray(a, F32).astype(T), np.asarray(b, F32).astype(T)
    r2 = T(np.float64(r) * np.float64(r))
    total = 0
    with np.errstate(all="ignore"):
        for k in range(0, len(a), 256):
            d = b[None, :, :] - a[k:k + 256, None, :]
            s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
            total += int((s == r2).sum())
    return total


def longest_row(pts, r):
    """records in the longest row of three x-cells of a grid of edge 1.01 r anchored at the cloud's minimum: an estimate of what the
    library's grid holds (it may choose a larger cell), -1 when that grid would be too large to count here"""
    fin = pts[np.isfinite(pts).all(1)].astype(np.float64)
    if not len(fin):
        return 0
    c = np.floor((fin - fin.min(0)) / max(1.01 * r, 2e-15))
    nc = c.max(0) + 1
    if nc.prod() > 4e6:
        return -1
    c, nc = c.astype(np.int64), nc.astype(np.int64)
    cnt = np.bincount((c[:, 2] * nc[1] + c[:, 1]) * nc[0] + c[:, 0], minlength=int(nc.prod())).reshape(nc[2], nc[1], nc[0])
    row = cnt.copy()
    row[..., 1:] += cnt[..., :-1]
    row[..., :-1] += cnt[..., 1:]
    return int(row.max())


class Reach:
    """the figures a sweep prints about itself"""

    def __init__(self, name, largest="neighbourhood"):
        self.name, self.what, self.trials, self.largest, self.pigeonhole, self.long_row, self.on_boundary = name, largest, 0, 0, 0, 0, 0
        self.kinds, self.radial = [0] * len(KIND), False

    def add(self, t, counts=None, radius=None, pairs=0):
        self.trials += 1
        self.kinds[t["kind"]] += 1
        big = int(np.max(counts, initial=0)) if counts is not None else 0
        self.largest = max(self.largest, big)
        if radius is not None:                                      # a row that walks the cell grid
            self.radial = True
            self.pigeonhole += big >= DENSE_MIN
            self.long_row += longest_row(t["pts"], radius) > CLIP
        self.on_boundary += pairs

    def report(self):
        line = f"{self.name}: {self.trials} trials ({', '.join(f'{k} {KIND[i]}' for i, k in enumerate(self.kinds) if k)})"
        if self.what:
            line += f", largest {self.what} {self.largest}"
        if self.radial:
            line += (f", {self.pigeonhole} trials with a neighbourhood >= {DENSE_MIN} (a clipped row for certain), {self.long_row} trials whose estimated grid "
                     f"has a row above {CLIP} records")
        print(line + (f", {self.on_boundary} pairs exactly on the boundary" if self.radial or self.on_boundary else ""))


def tag(t, **more):
    """everything needed to replay a trial"""
    parts = [f"trial {t['trial']}", f"kind {t['kind']} ({KIND[t['kind']]})", f"n {len(t['pts'])}"]
    parts += [f"{k} {t[k]!r}" for k in ("r", "leaf", "k", "std_ratio", "min_points", "lanes", "method", "nms", "mode", "bins", "sample", "seed", "nsample", "D", "npoints") if k in t]
    parts += [f"{k} {v!r}" for k, v in more.items()]
    return ", ".join(parts) + f", PCR_SWEEP_SEED {SEED}"


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- CPU: the sweeps' premises
@pytest.mark.parametrize("make,wide", [(fpfh_trial, False), (harris_trial, False), (dbscan_trial, True)], ids=["fpfh", "harris", "dbscan"])
def test_dense_trials_force_a_clipped_row_and_lattice_trials_sit_on_the_boundary(make, wide):
    """for the committed seeds at SCALE = 1: every dense trial has a point with >= 9 * 384 + 1 neighbours under the restatement's own
    membership test (so one of the nine rows it walks is longer than 384 records, whatever the grid), at least 20 surface pairs that lie
    inside the radius with an x-offset above 0.9996 r (lost by a window narrowed by 0.05 %), and every lattice trial at r in {0.5, 1.0,
    1.5} has >= 100 ordered pairs with s == r2 exactly"""
    dense = lattice = 0
    for trial in range(40):
        t = make(trial)
        pts, r = t["pts"], t["r"]
        if t["kind"] == 4:
            dense += 1
            probe = t["ball"][:8]
            if wide:
                cnt = dbscan_ref(pts, r, t["min_points"])[2][probe]
            else:
                qi, _, _ = neighbours(pts, pts[probe], r)
                cnt = np.bincount(qi, minlength=len(probe))
            fin = np.isfinite(pts[probe]).all(1)
            assert fin.any() and (cnt[fin] >= DENSE_MIN).all(), tag(t, counts=cnt.tolist())
            assert len(pts) >= DENSE_MIN + 300
            others = np.setdiff1d(np.arange(len(pts)), t["ball"])   # the probes and the scattered points as queries
            qi, j, _ = neighbours(pts, pts[others], r)
            far_in_x = np.abs(pts[j, 0].astype(np.float64) - pts[others[qi], 0]) > 0.9996 * r
            assert int(far_in_x.sum()) >= 20, tag(t, pairs=int(far_in_x.sum()))
        elif t["kind"] == 1 and r in ON_BOUNDARY_R:
            lattice += 1
            pairs = boundary_pairs(pts, pts, r, wide)
            assert pairs >= 100, tag(t, pairs=pairs)
    assert dense == 4 and lattice >= 3, (dense, lattice)


def test_ball_query_lattice_trials_sit_on_the_boundary():
    lattice = 0
    for trial in range(40):
        t = ball_trial(trial)
        if t["kind"] == 1 and t["r"] in ON_BOUNDARY_R:
            lattice += 1
            pairs = sum(boundary_pairs(t["cen"][t["cseg"][s]:t["cseg"][s + 1]], t["pts"][t["seg"][s]:t["seg"][s + 1]], t["r"]) for s in range(len(t["seg"]) - 1))
            assert pairs >= 100, tag(t, pairs=pairs)
    assert lattice >= 3, lattice


def test_fragile_share_of_the_fpfh_trials_is_under_the_cap():
    """the GPU sweep excuses an SPFH row only where the restatement marks it fragile (an f64 atan2 within 4 ulp of an f32 midpoint): over
    all trials of the committed seeds that is at most 0.1 % of the rows.  Every row of the dense trials is counted as well: their
    features cost most of this test's time, and they hold most of the pairs"""
    rows = fragile = pairs = 0
    for trial in range(40):
        t = fpfh_trial(trial)
        _, cnt, fr = spfh_numpy(t["pts"], t["nrm"], t["r"])
        rows, fragile, pairs = rows + len(fr), fragile + int(fr.sum()), pairs + int(cnt.sum())
    print(f"FPFH33 trials: {rows} rows, {pairs} pairs, {fragile} fragile rows")
    assert fragile <= FRAGILE_CAP * rows, (fragile, rows)


def test_voxel_grid_trials_stay_inside_int32():
    """the leaf rule of vgn_trial keeps every trial inside the contract: the restatement's own lattice arithmetic raises for none"""
    for trial in range(40):
        t = vgn_trial(trial)
        cent, _, vop, cnt = voxel_grid_numpy(t["pts"], None, t["leaf"])
        assert cent.shape[0] == cnt.size and int(cnt.sum()) == int(np.isfinite(t["pts"]).all(1).sum()), tag(t)


def test_trials_are_replayable_and_cover_the_sizes():
    a, b = fpfh_trial(17), fpfh_trial(17)
    assert np.array_equal(bits(a["pts"]), bits(b["pts"])) and np.array_equal(bits(a["kp"]), bits(b["kp"])) and a["lanes"] == b["lanes"]
    for make in (fpfh_trial, harris_trial, dbscan_trial):
        assert [len(make(trial)["pts"]) for trial in range(12) if trial != 9] == list(FIXED_N), make.__name__
    for make in (sor_trial, vgn_trial, nss_trial, ball_trial):
        assert [len(make(trial)["pts"]) for trial in range(11)] == list(FIXED_N), make.__name__
    lanes = {harris_trial(trial)["lanes"] for trial in range(40)}
    assert lanes == set(LANES)


# ---------------------------------------------------------------------------------------------------- GPU sweeps
@pytest.mark.gpu
def test_fpfh33_randomised(pcr):
    ctx = pcr.Context(0)
    reach = Reach("FPFH33")
    rows = excused_rows = 0
    try:
        for trial in range(40 * SCALE):
            t = fpfh_trial(trial)
            pts, nrm, r, kp = t["pts"], t["nrm"], t["r"], t["kp"]
            what = tag(t)
            ctx.tune("fpfh_lanes", t["lanes"])
            c, nc = ctx.cloud(pts, AOS3), ctx.cloud(nrm, AOS3)
            fp, cnt, sp = ctx.fpfh33(c, nc, r, spfh=True)
            sp_ref, cnt_ref, fragile = spfh_numpy(pts, nrm, r)
            assert np.array_equal(cnt, cnt_ref), f"neighbour counts differ at {np.flatnonzero(cnt != cnt_ref)[:5]}: {what}"
            excused = check_spfh(sp, sp_ref, fragile, what)
            rows, excused_rows = rows + len(pts), excused_rows + len(excused)
            sp_use = sp_ref.copy()
            sp_use[excused] = sp[excused]
            ref, rc = fpfh_numpy(pts, sp_use, r)
            assert np.array_equal(cnt, rc), what
            check_fpfh(fp, ref, what + ", keypoints=None", min_same=0.0)
            kc = ctx.cloud(kp, AOS3)
            f2, c2 = ctx.fpfh33(c, nc, r, keypoints=kc)
            ref2, rc2 = fpfh_numpy(pts, sp_use, r, kp)
            assert np.array_equal(c2, rc2), f"keypoint neighbour counts differ at {np.flatnonzero(c2 != rc2)[:5]}: {what}"
            check_fpfh(f2, ref2, what + ", foreign keypoints", min_same=0.0)
            for h in (kc, nc, c):
                h.free()
            reach.add(t, np.concatenate([cnt_ref, rc2]), r, boundary_pairs(pts, pts, r) + boundary_pairs(kp, pts, r) if t["kind"] == 1 else 0)
        print(f"FPFH33: {excused_rows} of {rows} SPFH rows differed and were excused as fragile")
        assert excused_rows <= FRAGILE_CAP * rows
        reach.report()
    finally:
        ctx.tune("fpfh_lanes", 0)
        ctx.close()


def harris_threshold(t, resp):
    fin = resp[np.isfinite(resp)]
    q = float(F32(np.quantile(fin, t["quantile"]))) if fin.size else 0.0
    return (-np.inf, 0.0, 1e-8, q, np.inf)[t["thr_kind"]]


def check_harris(ctx, pts, nrm, r, thr, method, nms, what):
    c, nc = ctx.cloud(pts, AOS3), ctx.cloud(nrm, AOS3)
    idx, resp, cnt = ctx.harris3d(c, nc, r, thr, method, nms)
    nc.free(); c.free()
    key, rr, rc = harris_numpy(pts, nrm, r, thr, method, nms)
    bad = np.flatnonzero(bits(resp) != bits(rr))
    assert np.array_equal(cnt, rc), f"neighbour counts differ at {np.flatnonzero(cnt != rc)[:5]}: {what}"
    assert bad.size == 0, f"{bad.size} responses differ, first {bad[:5]}: gpu {resp[bad[:5]]} restatement {rr[bad[:5]]}: {what}"
    mask = np.zeros(len(pts), bool)
    mask[idx] = True
    assert np.array_equal(mask, key), f"keys differ at {np.flatnonzero(mask != key)[:5]}: {what}"
    return resp, rc, mask


@pytest.mark.gpu
def test_harris3d_randomised(pcr):
    ctx = pcr.Context(0)
    reach = Reach("Harris3D")
    try:
        for trial in range(40 * SCALE):
            t = harris_trial(trial)
            pts, nrm, r = t["pts"], t["nrm"], t["r"]
            ctx.tune("harris_lanes", t["lanes"])
            thr = -np.inf
            if t["thr_kind"] == 3:                                  # a quantile of the restatement's own responses: about that share fails the threshold
                _, rr, _ = harris_numpy(pts, nrm, r, -np.inf, t["method"], False)
            else:
                rr = np.zeros(0, F32)
            thr = harris_threshold(t, rr)
            what = tag(t, threshold=thr)
            resp, cnt, mask = check_harris(ctx, pts, nrm, r, thr, t["method"], t["nms"], what)
            if t["perm"] is not None:                               # the contract is free of order: the same response for every point
                p = t["perm"]
                c, nc = ctx.cloud(pts[p], AOS3), ctx.cloud(nrm[p], AOS3)
                ip, rp, cp = ctx.harris3d(c, nc, r, thr, t["method"], t["nms"])
                nc.free(); c.free()
                mp = np.zeros(len(pts), bool)
                mp[ip] = True
                assert np.array_equal(bits(rp), bits(resp)[p]) and np.array_equal(cp, cnt[p]) and np.array_equal(mp, mask[p]), "permuted input: " + what
            reach.add(t, cnt, r, boundary_pairs(pts, pts, r) if t["kind"] == 1 else 0)
        reach.report()
    finally:
        ctx.tune("harris_lanes", 0)
        ctx.close()


@pytest.mark.gpu
def test_dbscan_randomised(pcr):
    ctx = pcr.Context(0)
    reach = Reach("DBSCAN")
    try:
        for trial in range(40 * SCALE):
            t = dbscan_trial(trial)
            pts, eps = t["pts"], t["r"]
            want = dbscan_ref(pts, eps, t["min_points"])
            assert_dbscan_equal(run_dbscan(ctx, pts, eps, t["min_points"], t["lanes"]), want, tag(t))
            reach.add(t, want[2], eps, boundary_pairs(pts, pts, eps, wide=True) if t["kind"] == 1 else 0)
        reach.report()
    finally:
        ctx.tune("dbscan_lanes", 32)
        ctx.close()


@pytest.mark.gpu
def test_statistical_outlier_randomised(pcr):
    ctx = pcr.Context(0)
    reach = Reach("statistical outlier removal", None)
    zero_avg = 0
    try:
        for trial in range(30 * SCALE):
            t = sor_trial(trial)
            want = sor_ref(t["pts"], t["k"], t["std_ratio"])
            assert_sor_equal(run_sor(ctx, t["pts"], t["k"], t["std_ratio"]), t["pts"], want, tag(t), equal_nan=True)
            zero_avg += int((want[1] == 0).sum())
            reach.add(t)
        print(f"statistical outlier removal: {zero_avg} points with avg = 0 (k or more exact duplicates, or k = 1)")
        reach.report()
    finally:
        ctx.close()


def check_voxel_grid(ctx, pts, nrm, leaf, mode, what):
    c = ctx.cloud(pts, AOS3)
    nc = None if nrm is None else ctx.cloud(nrm, AOS3)
    oc, on, vop, cnt = ctx.voxel_grid_normals(c, nc, leaf, mode)
    wc, wn, wvop, wcnt = voxel_grid_numpy(pts, nrm, leaf, mode)
    m = len(oc)
    got_c = np.ascontiguousarray(oc.numpy().T).reshape(-1, 3) if m else np.zeros((0, 3), F32)
    got_n = None if on is None else (np.ascontiguousarray(on.numpy().T).reshape(-1, 3) if m else np.zeros((0, 3), F32))
    for h in (on, oc, nc, c):
        if h is not None:
            h.free()
    assert m == wc.shape[0], f"{m} voxels, restatement {wc.shape[0]}: {what}"
    assert np.array_equal(vop, wvop), f"voxel_of_point differs at {np.flatnonzero(vop != wvop)[:5]}: {what}"
    assert np.array_equal(cnt.astype(np.int64), wcnt), what
    bad = np.flatnonzero((bits(got_c) != bits(wc)).any(1))
    assert bad.size == 0, f"{bad.size} centroids differ, first {bad[:3]}: gpu {got_c[bad[:3]]} restatement {wc[bad[:3]]}: {what}"
    if nrm is None:
        assert on is None
    else:
        bad = np.flatnonzero((bits(got_n) != bits(wn)).any(1))
        assert bad.size == 0, f"{bad.size} voxel normals differ, first {bad[:3]}: gpu {got_n[bad[:3]]} restatement {wn[bad[:3]]}: {what}"
    return got_c, got_n, vop, cnt


@pytest.mark.gpu
def test_voxel_grid_normals_randomised(pcr):
    ctx = pcr.Context(0)
    reach = Reach("voxel grid with normals", "voxel")
    try:
        for trial in range(40 * SCALE):
            t = vgn_trial(trial)
            pts, nrm = t["pts"], t["nrm"]
            what = tag(t, normals=nrm is not None)
            got_c, got_n, vop, cnt = check_voxel_grid(ctx, pts, nrm, t["leaf"], t["mode"], what)
            if t["perm"] is not None:                               # a function of the SET of (point, normal) pairs
                p = t["perm"]
                c2, n2, v2, k2 = check_voxel_grid(ctx, pts[p], None if nrm is None else nrm[p], t["leaf"], t["mode"], "permuted input: " + what)
                assert np.array_equal(bits(c2), bits(got_c)) and np.array_equal(v2, vop[p]) and np.array_equal(k2, cnt), "permuted input: " + what
                assert nrm is None or np.array_equal(bits(n2), bits(got_n)), "permuted input: " + what
            reach.add(t, cnt)
        reach.report()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_normal_space_sampling_randomised(pcr):
    ctx = pcr.Context(0)
    reach = Reach("normal-space sampling", None)
    try:
        for trial in range(40 * SCALE):
            t = nss_trial(trial)
            pts, nrm = t["pts"], t["nrm"]
            what = tag(t)
            c, nc = ctx.cloud(pts, AOS3), ctx.cloud(nrm, AOS3)
            idx, sc, sn = ctx.normal_space_sample(nc, t["bins"], t["sample"], t["seed"], gather=(c, nc))
            want = nss_numpy(nrm, t["bins"], t["sample"], t["seed"])
            assert np.array_equal(idx, want), f"{idx.size} indices, restatement {want.size}, first difference at {np.flatnonzero(idx[:min(idx.size, want.size)] != want[:min(idx.size, want.size)])[:3]}: {what}"
            assert len(sc) == idx.size and len(sn) == idx.size, what
            if idx.size:
                assert np.array_equal(bits(sc.numpy().T), bits(pts[idx])) and np.array_equal(bits(sn.numpy().T), bits(nrm[idx])), "gathered clouds: " + what
            for h in (sn, sc, nc, c):
                h.free()
            reach.add(t)
        reach.report()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_ball_query_and_grouping_randomised(pcr):
    ctx = pcr.Context(0)
    reach = Reach("ball query and grouping", "row (capped at nsample)")
    grouped = refused = 0
    try:
        for trial in range(40 * SCALE):
            t = ball_trial(trial)
            pts, cen, seg, cseg, r, k = t["pts"], t["cen"], t["seg"], t["cseg"], t["r"], t["nsample"]
            what = tag(t, segments=np.diff(seg.astype(np.int64)).tolist(), centres=np.diff(cseg.astype(np.int64)).tolist())
            c, cc = ctx.cloud(pts, AOS3), ctx.cloud(cen, AOS3)
            got, cnt = ctx.ball_query(c, seg, cc, cseg, r, k)
            want = [ball_ref(pts[seg[s]:seg[s + 1]], cen[cseg[s]:cseg[s + 1]], r, k) for s in range(len(seg) - 1)]
            wr = np.concatenate([w[0] for w in want]).reshape(-1, k)
            wc = np.concatenate([w[1] for w in want])
            assert np.array_equal(cnt, wc), f"counts differ at rows {np.flatnonzero(cnt != wc)[:5]}: {what}"
            assert np.array_equal(got, wr), f"index rows differ at rows {np.flatnonzero((got != wr).any(1))[:5]}: {what}"
            if (wc == 0).any():                                     # an empty row holds the segment's size: grouping refuses it
                with pytest.raises(pcr.PcrError, match=pcr.ERRORS[-1]):
                    ctx.group_points(c, seg, cc, cseg, got, t["feat"])
                refused += 1
            elif len(wc):
                nx, npts = ctx.group_points(c, seg, cc, cseg, got, t["feat"])
                for s in range(len(seg) - 1):
                    a, b = int(cseg[s]), int(cseg[s + 1])
                    if a == b:
                        continue
                    feat = None if t["feat"] is None else t["feat"][seg[s]:seg[s + 1]]
                    wx, wp = group_ref(pts[seg[s]:seg[s + 1]], cen[a:b], wr[a:b], feat)
                    assert np.array_equal(bits(nx[a:b]), bits(wx)) and np.array_equal(bits(npts[a:b]), bits(wp)), f"grouping, segment {s}: {what}"
                grouped += 1
            cc.free(); c.free()
            pairs = sum(boundary_pairs(cen[cseg[s]:cseg[s + 1]], pts[seg[s]:seg[s + 1]], r) for s in range(len(seg) - 1)) if t["kind"] == 1 else 0
            reach.add(t, wc, None, pairs)
        print(f"ball query and grouping: {grouped} trials grouped bit for bit, {refused} refused for an empty row (the largest neighbourhood is capped at nsample)")
        assert grouped >= 10 * SCALE and refused >= 5 * SCALE
        reach.report()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_objects_from_labels_randomised(pcr):
    ctx = pcr.Context(0)
    reach = Reach("objects from labels", "cluster")
    n_objects = 0
    try:
        for trial in range(30 * SCALE):
            t = objects_trial(trial)
            pts, lab, nc = t["pts"], t["labels"], t["n_clusters"]
            what = tag(t, ground_z=t["ground_z"], thr=t["thr"], z_extent=t["z_extent"], starts=t["starts"] is not None)
            c = ctx.cloud(pts, AOS3)
            res = ctx.objects_from_labels(c, lab, nc, t["npoints"], ground_z=t["ground_z"], z_min_above_ground=t["thr"], z_extent=t["z_extent"], seed=t["seed"],
                                          starts=t["starts"])
            c.free()
            codes, zmm, sizes, objs = objects_ref(pts, lab, nc, t["npoints"], t["ground_z"], t["thr"], t["z_extent"], t["seed"], t["starts"])
            assert np.array_equal(res["sizes"], sizes) and np.array_equal(res["z_min_max"], zmm), "sizes / z statistics: " + what
            assert np.array_equal(res["codes"], codes), f"codes differ at clusters {np.flatnonzero(res['codes'] != codes)[:5]}: {what}"
            assert res["cluster"].tolist() == [o[0] for o in objs], "object rows: " + what
            for row, (cl, pos, src, out) in enumerate(objs):
                assert np.array_equal(res["source_index"][row], src), f"members of cluster {cl} (size {sizes[cl]}): {what}"
                assert np.array_equal(bits(res["objects"][row]), bits(out)), f"normalised rows of cluster {cl} (size {sizes[cl]}): {what}"
            n_objects += len(objs)
            reach.add(t, sizes)
        print(f"objects from labels: {n_objects} object rows compared")
        assert n_objects >= 30 * SCALE
        reach.report()
    finally:
        ctx.close()
