"""k-NN on every route, list width and geometry class (pcr_cloud_knn_f64, pcr_db64_knn, pcr_knn_f64), and the normals built on it
(pcr_normals_knn_f64) on the neighbourhoods where the closed-form eigen solver changes branch.

One question, five code paths, picked silently by the batch size and the data (csrc/knn_grid.hip, csrc/search_f64.hip):
  A  batch kernel, self-query over the grid records           ctx.cloud_knn(c, c, ...)
  B  batch kernel, external queries through the permutation   ctx.cloud_knn(cdb, cq, ...); Db64.knn with knn_method 3 (or more than 4 096 queries)
  C  batch kernel, "direct" small batch from pinned memory    Db64.knn, >= 4 096 f32-representable points, 17 ... 4 096 queries (or knn_coop 2)
  D  one wave per query                                        the same handle, <= 16 queries
  E  exhaustive scan, database in slices + knn_merge_kernel   knn_method 1; fewer than 4 096 points; a coordinate f32 does not hold
  F  exhaustive scan, one slice                                E with knn_slices 2
A claimed route is proved with the profiler's scopes: A, B, C add to knn_grid and not to knn_f64, E and F to knn_f64 and not to knn_grid, and D
to NEITHER — the one-wave call opens no scope, so "no scope at all" is its proof.  Inside A and B the grid is the cloud's own x-sorted 1-NN grid
for a cloud under 256 points with k <= 4 and a widened grid, cached in one slot, otherwise (scope grid_build counts the builds).

The reference is ref_knn below: plain numpy f64, independent of the library and of the C oracle.  A CPU test checks it against BOTH oracles
(orc.knn_sq_f32pts, orc.knn_f64) on every fixture, and another asserts the property each fixture is built for on the reference alone.  Every GPU
assertion on k-NN output is EQUALITY — indices, `found`, values as uint64 bits — on every row.

Tune keys: the value 0 restores the default of every key; "off" is 2 (knn_coop, knn_slices)."""
from contextlib import contextmanager

import numpy as np
import pytest

import knn_route_cases as cases
from knn_route_cases import cached, soa32

DBL_MAX = float(np.finfo(np.float64).max)
K_SET = (1, 2, 4, 5, 8, 9, 16, 17, 32)          # every template width and the width just past it (k_out < K)
OFF = 2
BIG_IDS = ("lattice", "coincident", "line_x", "line_y", "line_z", "line_diag", "plane", "far", "bar", "shell", "collapse", "rule", "nonfinite_inf")


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ the contract
def ref_knn(db, q, k, radius=-1.0, squared=True):
    """-> (idx i32 [m, k], value f64 [m, k], found u32 [m]).
    s = ((dx*dx) + dy*dy) + dz*dz in f64 with d = t - q; value = s (squared) or sqrt(s); order: stable lexicographic on (value, index);
    cap: strict s < radius^2 when radius >= 0; a non-finite database point is never a neighbour, a non-finite query finds nothing;
    non-squared mode follows hw2's result set (worstDist starts at 1e10, `dist > worstDist` is rejected): d > 1e10 never enters, d == 1e10
    enters with its index; unused slots hold (DBL_MAX, -1) squared and (1e10, 0) otherwise; found = the number of real entries."""
    db, q = np.asarray(db, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3)
    n, m = db.shape[0], q.shape[0]
    idx = np.full((m, k), -1 if squared else 0, np.int32)
    val = np.full((m, k), DBL_MAX if squared else 1e10, np.float64)
    found = np.zeros(m, np.uint32)
    if n == 0:
        return idx, val, found
    db_ok = np.isfinite(db).all(1)
    for lo in range(0, m, 512):
        qq = q[lo:lo + 512]
        with np.errstate(all="ignore"):
            dx, dy, dz = (db[None, :, a] - qq[:, None, a] for a in range(3))
            s = (dx * dx + dy * dy) + dz * dz
            v = s if squared else np.sqrt(s)
            ok = db_ok[None, :] & np.isfinite(qq).all(1)[:, None]
            if radius >= 0:
                ok &= s < radius * radius
            if not squared:
                ok &= v <= 1e10
        # the k smallest (value, index) of a row without sorting all n: t = its k-th smallest value; everything below t, and of the entries AT t
        # the lowest indices, as many as are still missing (nonzero() walks a row in ascending index); a stable sort by value orders them
        key = np.where(ok, v, np.inf)
        kk = min(k, n)
        t = np.partition(key, kk - 1, axis=1)[:, kk - 1:kk]
        less, at = key < t, key == t
        pick = less | (at & (np.cumsum(at, axis=1) <= kk - less.sum(1, keepdims=True)))
        cols = np.nonzero(pick)[1].reshape(-1, kk)
        vals = np.take_along_axis(v, cols, 1)
        order = np.argsort(np.take_along_axis(key, cols, 1), axis=1, kind="stable")
        cols, vals = np.take_along_axis(cols, order, 1), np.take_along_axis(vals, order, 1)
        cnt = np.minimum(ok.sum(1), k)
        real = np.arange(kk)[None, :] < cnt[:, None]
        idx[lo:lo + 512, :kk] = np.where(real, cols, idx[lo:lo + 512, :kk])
        val[lo:lo + 512, :kk] = np.where(real, vals, val[lo:lo + 512, :kk])
        found[lo:lo + 512] = cnt
    return idx, val, found


def want(c, which, k, squared, radius=-1.0):
    """the reference rows of case c ("self": the database asks itself; "ext": c.q) — computed once at k = 32: the list for a smaller k is its
    head (the order is total, unused slots come last)"""
    def make():
        out = ref_knn(c.db, c.db if which == "self" else c.q, 32, radius, squared)
        for a in out:
            a.setflags(write=False)
        return out
    idx, val, found = cached(("ref", c.name, which, bool(squared), float(radius)), make)
    return idx[:, :k], val[:, :k], np.minimum(found, k).astype(np.uint32)


def assert_rows(got, ref, what):
    assert np.array_equal(got[0], ref[0]), what
    assert np.array_equal(bits64(got[1]), bits64(ref[1])), what
    if len(got) > 2:
        assert np.array_equal(got[2], ref[2]), what


# --------------------------------------------------------------------------------------------------- CPU: the restatement, the fixtures
SCAN_SHAPES = ((1, 1), (511, 255), (512, 256), (513, 257), (1025, 257))
CASE_MAKERS = dict(zip(BIG_IDS, cases.BIG_CASES))
CASE_MAKERS.update(nonfinite_nan=lambda: cases.nonfinite_case(True), lattice7=lambda: cases.small_lattice_case(7), lattice6=lambda: cases.small_lattice_case(6),
                   coincident300=lambda: cases.coincident_case(300), coincident200=lambda: cases.coincident_case(200))
CASE_MAKERS.update({f"scan{n}x{m}": (lambda n=n, m=m: cases.scan_case(n, m)) for n, m in SCAN_SHAPES})


def all_cases():
    return [make() for make in CASE_MAKERS.values()]


def test_fixtures_are_what_they_claim():
    for c in all_cases() + [cases.tilted_plane_case(), cases.sparse_case()]:
        assert cases.is_f32(c.db) and cases.is_f32(c.q), c.name                               # the twin cloud exists, clouds hold them exactly
        assert c.db.shape[0] <= 4200, c.name
    assert all(make().db.shape[0] >= 4096 for make in cases.BIG_CASES)
    assert all(name == c.name or name + "4096" == c.name for name, c in zip(CASE_MAKERS, all_cases()))
    for c in (cases.lattice_case(), cases.bar_case(), cases.shell_case(), cases.plane_case()):
        assert not np.array_equal(c.db, c.db[np.lexsort(c.db.T[::-1])])                          # shuffled: index order is not spatial order


@pytest.mark.parametrize("name", list(CASE_MAKERS))
def test_reference_restatement_equals_both_oracles(orc, name):
    """ref_knn against orc.knn_sq_f32pts (squared, with and without a cap) and orc.knn_f64 (non-squared) on every fixture, self-query and external.
    orc.knn_f64 restates hw2 literally, NaN included (`NaN > worst` is false: a NaN distance enters), where this contract says that a non-finite
    point is never a neighbour: for that oracle the non-finite database points are moved to 3e38 (beyond 1e10 from everything: never a neighbour
    there either) and the non-finite queries are left out."""
    c = CASE_MAKERS[name]()
    for which in ("self", "ext") if name in BIG_IDS else ("ext",):
        qq = c.db if which == "self" else c.q
        oi, os_, of = orc.knn_sq_f32pts(soa32(c.db), soa32(qq), 32)
        ri, rs, rf = want(c, which, 32, True)
        assert np.array_equal(oi, ri) and np.array_equal(bits64(os_), bits64(rs)) and np.array_equal(of, rf), which
        db_fin = np.where(np.isfinite(c.db).all(1)[:, None], c.db, cases.F32_3E38)
        keep = np.isfinite(qq).all(1)
        hi, hd = orc.knn_f64(db_fin, qq[keep], 32)
        ri, rd, _ = want(c, which, 32, False)
        assert np.array_equal(hi, ri[keep]) and np.array_equal(bits64(hd), bits64(rd[keep])), which
        assert (ri[~keep] == 0).all() and (rd[~keep] == 1e10).all()
    for r in {"lattice7": (0.3, 0.25, 0.0), "shell": (cases.R_SHELL, float(np.nextafter(cases.R_SHELL, 1.0)))}.get(name, ()):
        for which in ("self", "ext"):
            oi, os_, of = orc.knn_sq_f32pts(soa32(c.db), soa32(c.db if which == "self" else c.q), 32, r)
            ri, rs, rf = want(c, which, 32, True, r)
            assert np.array_equal(oi, ri) and np.array_equal(bits64(os_), bits64(rs)) and np.array_equal(of, rf), (which, r)


def test_lattice_tie_sets_and_clamped_queries():
    c = cases.lattice_case()
    idx, s, found = want(c, "ext", 32, True)
    rows = range(c.interior.start, c.interior.stop)
    for r in rows:                                                                         # tie sets of 1, 6, 12, 8 around an interior point ...
        assert np.array_equal(s[r, :27], np.repeat([0.0, 0.0625, 0.125, 0.1875], [1, 6, 12, 8])), r
        assert s[r, 27] == 0.25
        for a, b in ((1, 7), (7, 19), (19, 27)):
            assert (np.diff(idx[r, a:b]) > 0).all()                                        # ... each in ascending index
    ties6 = np.array([np.sort(np.flatnonzero(((c.db - c.q[r]) ** 2).sum(1) == 0.0625)) for r in rows])
    assert ties6.shape == (40, 6) and np.array_equal(idx[c.interior, 1:5], ties6[:, :4])   # k = 5 cuts the set of 6: the lowest indices win
    assert not np.array_equal(ties6, np.sort(ties6, axis=1)[:, ::-1]) and (ties6[:, 4] > ties6[:, 3]).all()
    assert np.array_equal(idx[c.lattice_rows, 0], c.at) and (s[c.lattice_rows, 0] == 0).all()
    # the clamped queries: (1e7,) * 3 is more than 2^22 cells away at any cell edge below 2.3, (3e38,) * 3 at any cell edge at all
    assert (found[:2] == 32).all() and s[0, 0] > 2.9e14 and s[1, 0] > 2.6e77
    i2, d2, f2 = want(c, "ext", 32, False)
    assert f2[0] == 32 and d2[0, 0] < 1e10
    assert f2[1] == 0 and (i2[1] == 0).all() and (d2[1] == 1e10).all()                     # non-squared: beyond 1e10, unused slots only


def test_degenerate_extents_lines_plane_coincident():
    for n in (4096, 300, 200):
        c = cases.coincident_case(n)
        assert np.ptp(c.db, axis=0).tolist() == [0.0, 0.0, 0.0]
        idx, s, found = want(c, "ext", 32, True)
        assert (idx[:20] == np.arange(32)).all() and (s[:20] == 0).all()                    # every row: indices 0 ... k - 1 at value 0
        idx, s, _ = want(c, "self", 32, True) if n == 4096 else ref_knn(c.db, c.db, 32)
        assert (idx == np.arange(32)).all() and (s == 0).all()
    for axis in ("x", "y", "z", "diag"):
        c = cases.line_case(axis)
        ext = np.ptp(c.db, axis=0)
        assert ((ext > 0) == (np.asarray(cases.LINE_DIRS[axis]) > 0)).all()                 # zero extent in two axes (none on the diagonal)
        zero = c.db[c.zeros]
        assert (zero == 0).all(1).sum() == (2 if axis == "diag" else 0) and np.signbit(zero).any() and not np.signbit(zero).all()
        idx, s, _ = want(c, "ext", 32, True)
        inner = idx[c.inner]
        assert np.array_equal(inner[:, 0], c.at)
        for a in range(1, 31, 2):                                                           # a line point ties pairwise, left and right
            assert (s[c.inner, a] == s[c.inner, a + 1]).all() and (inner[:, a] < inner[:, a + 1]).all()
        assert (np.diff(s[c.inner, 0:31:2], axis=1) > 0).all()
        assert s[0, 0] == 0 and s[0, 1] == 0 and sorted(idx[0, :2]) == sorted(c.zeros)       # the query +0.0 finds both zeros at 0 ...
        assert np.array_equal(idx[0, :2], idx[1, :2]) and np.array_equal(bits64(s[0]), bits64(s[1]))    # ... and so does -0.0, bit for bit
    c = cases.plane_case()
    assert np.ptp(c.db, axis=0).tolist() == [15.75, 15.75, 0.0]


def test_far_bar_shell_collapse_and_the_1e10_rule():
    c = cases.far_case()
    idx, s, found = want(c, "ext", 32, True)
    assert (np.sort(idx[:3, :3], axis=1) == np.sort(c.near_at)).all() and (s[:3, 2] < 1.0).all()
    assert (s[:3, 3] > 1700.0 ** 2).all() and (found[:3] == 32).all()                       # k = 8: five of them across a thousand empty units
    c = cases.bar_case()
    idx, s, _ = want(c, "ext", 32, True)
    on_bar = np.isin(idx[c.bar_rows], c.bar_at)
    assert on_bar.all() and (s[c.bar_rows, 31] <= (2.0 ** -7) ** 2).all()                   # 32 neighbours (33 records) of the row within 2^-7 ...
    assert np.unique(c.db[c.bar_at][:, 1:]).tolist() == [1.125] and c.bar_at.size == 2048   # ... all in ONE x-row: y = z = const
    assert (np.diff(np.sort(c.db[c.bar_at][:, 0])) == 2.0 ** -12).all()
    c = cases.shell_case()
    idx, s, found = want(c, "ext", 32, True)
    assert c.shell_at.size == 150 and np.array_equal(idx[0], c.shell_at[:32]) and (s[0] == 625.0 / 65536.0).all()
    d = c.db[c.shell_at] - np.asarray(cases.SHELL_CENTRE)
    assert ((d * d).sum(1) == 625.0 / 65536.0).all() and np.unique(np.floor(c.db[c.shell_at] / 0.05), axis=0).shape[0] > 8   # exact, and spread out
    assert want(c, "ext", 32, True, cases.R_SHELL)[2][0] == 0                               # the strict cap excludes the whole shell ...
    up = want(c, "ext", 32, True, float(np.nextafter(cases.R_SHELL, 1.0)))
    assert up[2][0] == 32 and np.array_equal(up[0][0], c.shell_at[:32])                     # ... the next radius admits it
    c = cases.collapse_case()
    assert c.ib < c.ia
    sa, sb = (((c.db[i] - c.q[0]) ** 2).sum() for i in (c.ia, c.ib))
    assert sa == 1.0 and sb == 1.0 + 2.0 ** -52 and np.sqrt(sb) == 1.0                      # the collapse itself
    assert want(c, "ext", 2, True)[0][0].tolist() == [c.ia, c.ib] and want(c, "ext", 2, False)[0][0].tolist() == [c.ib, c.ia]
    assert bits64(want(c, "ext", 2, False)[1][0]).tolist() == [bits64(np.float64(1.0))] * 2
    c = cases.rule_case()
    near, (far1, far2) = sorted(c.near_at), c.far_at
    idx, s, found = want(c, "ext", 8, True)
    assert found[0] == 8 and sorted(idx[0, :3]) == near and idx[0, 3:5].tolist() == [far1, far2] and s[0, 3] == 1e20    # squared: both are real
    idx, d, found = want(c, "ext", 8, False)
    assert found[0] == 4 and sorted(idx[0, :3]) == near and idx[0, 3] == far1 and d[0, 3] == 1e10                      # d == 1e10 enters ...
    assert (idx[0, 4:] == 0).all() and (d[0, 4:] == 1e10).all()                                                          # ... 1e10 + 1024 never
    assert found[1] == 5 and idx[1, 3:5].tolist() == [far1, far2] and d[1, 3] == 1e10 - 1024 and d[1, 4] == 1e10         # from (1024, 0, 0)
    assert found[2] == 4 and d[2, 3] < 1e10 and found[3] == 3                                                            # one step inside, outside
    c = cases.nonfinite_case(True)
    idx, s, found = want(c, "ext", 32, True)
    assert (found[: c.n_odd] == 0).all() and (found[c.n_odd:] == 32).all() and not np.isin(c.odd_at, idx[c.n_odd:]).any()


def test_scan_fixtures_put_ties_on_the_tile_and_slice_edges():
    c = cases.scan_case(1025, 257)
    idx, d, found = ref_knn(c.db, c.q, 32, squared=False)
    assert idx[0, :10].tolist() == [510, 511, 512, 513, 514, 1020, 1021, 1022, 1023, 1024] and (d[0, :10] == 0).all()
    assert 512 * 2 < c.db.shape[0] <= 512 * 2 + 1                                           # the third tile / slice holds one point: fewer than k
    idx, d, found = ref_knn(cases.scan_case(1, 1).db, cases.scan_case(1, 1).q, 32, squared=False)
    assert found[0] == 1 and (idx[0, 1:] == 0).all() and (d[0, 1:] == 1e10).all()


# ----------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def ctx(pcr):
    c = pcr.Context(0)
    yield c
    c.close()


@contextmanager
def tuned(ctx, **keys):
    try:
        for k, v in keys.items():
            ctx.tune(k, v)
        ctx.prof_reset()
        yield
    finally:
        for k in keys:
            ctx.tune(k, 0)


def scopes(ctx):
    """(launches under knn_grid, launches under knn_f64) since the last prof_reset (the scopes need tune prof >= 2)"""
    return ctx.prof_get("knn_grid")[0], ctx.prof_get("knn_f64")[0]


@contextmanager
def handles(ctx, c):
    cdb, cq, h = ctx.cloud(soa32(c.db)), ctx.cloud(soa32(c.q)), ctx.db64(c.db)
    try:
        yield cdb, cq, h
    finally:
        h.free()
        cq.free()
        cdb.free()


COOP_CHUNKS = ((0, 16), (16, 32), (32, 45), (45, 48))                                      # calls of 16, 16, 13 and 3 queries


def every_route(ctx, c, ks, twin=True):
    """routes A ... F on case c at every k of ks, both modes; twin = False: the database has no f32 twin (a NaN), a handle scans whatever is set"""
    m = c.q.shape[0]
    assert 48 <= m <= 4096
    with handles(ctx, c) as (cdb, cq, h):
        for squared in (True, False):
            def ext(k):
                return want(c, "ext", k, squared)[:2]
            with tuned(ctx, prof=2):                                                       # A
                for k in ks:
                    assert_rows(ctx.cloud_knn(cdb, cdb, k, -1.0, squared), want(c, "self", k, squared), (c.name, "A", k, squared))
                assert scopes(ctx) == (len(ks), 0)
            with tuned(ctx, prof=2):                                                       # B, between clouds
                for k in ks:
                    assert_rows(ctx.cloud_knn(cdb, cq, k, -1.0, squared), want(c, "ext", k, squared), (c.name, "B", k, squared))
                assert scopes(ctx) == (len(ks), 0)
            for route, keys, proof in (("B handle", dict(knn_method=3), (len(ks), 0)), ("C", {}, (len(ks), 0)),
                                       ("E", dict(knn_method=1), (0, len(ks))), ("F", dict(knn_method=1, knn_slices=OFF), (0, len(ks)))):
                with tuned(ctx, prof=2, **keys):
                    for k in ks:
                        assert_rows(h.knn(c.q, k, squared), ext(k), (c.name, route, k, squared))
                    assert scopes(ctx) == (proof if twin else (0, len(ks))), (c.name, route)
            for route, keys in (("C16", dict(knn_coop=OFF)), ("D", {})):                  # the first 48 queries in calls of <= 16
                with tuned(ctx, prof=2, **keys):
                    for k in ks:
                        for a, b in COOP_CHUNKS:
                            ref = ext(k)
                            assert_rows(h.knn(c.q[a:b], k, squared), (ref[0][a:b], ref[1][a:b]), (c.name, route, k, squared, a))
                    calls = len(ks) * len(COOP_CHUNKS)
                    # D: the one-wave call opens no scope — neither knn_grid (the batch kernel) nor knn_f64 (the scan) may have run
                    assert scopes(ctx) == ((0, calls) if not twin else (calls, 0) if route == "C16" else (0, 0)), (c.name, route)


@pytest.mark.gpu
@pytest.mark.parametrize("make", cases.BIG_CASES, ids=BIG_IDS)
def test_every_route_at_every_template_edge(ctx, make):
    every_route(ctx, make(), K_SET)


@pytest.mark.gpu
def test_nan_points_and_queries_on_the_cloud_routes_and_the_scan(ctx):
    """a NaN database point: the cloud routes (A, B) bin it into the non-finite cell, a handle has no twin cloud and scans (E, F)"""
    every_route(ctx, cases.nonfinite_case(True), (1, 5, 32), twin=False)


@pytest.mark.gpu
def test_natural_fallbacks_to_the_scan(ctx):
    """one coordinate that f32 does not hold (2^-40 added) — in a query, then in the database — sends the call to the exhaustive scan"""
    c = cases.lattice_case()
    q2 = c.q.copy()
    q2[3, 0] += 2.0 ** -40                                                 # (one of the first 16: the call of 16 queries holds it too)
    db2 = c.db.copy()
    db2[5, 2] += 2.0 ** -40
    assert not cases.is_f32(q2) and not cases.is_f32(db2)
    for db, q in ((c.db, q2), (db2, c.q)):
        h = ctx.db64(db)
        try:
            for squared in (True, False):
                ref = ref_knn(db, q, 9, squared=squared)
                with tuned(ctx, prof=2):
                    assert_rows(h.knn(q, 9, squared), ref[:2], squared)
                    assert_rows(h.knn(q[:16], 9, squared), (ref[0][:16], ref[1][:16]), squared)
                    assert scopes(ctx) == (0, 2)
        finally:
            h.free()


@pytest.mark.gpu
def test_every_list_width_on_the_batch_routes(ctx):
    """k = 1 ... 32 (every k_out < K) on 343 points, routes A and B, both modes; a capped radius: 0.3 admits the point and its six face
    neighbours, 0.25 is the face distance itself (strict: the point alone), 0 admits nothing"""
    c = cases.small_lattice_case(7)
    with handles(ctx, c) as (cdb, cq, h):
        with tuned(ctx, prof=2):
            for squared in (True, False):
                for k in range(1, 33):
                    assert_rows(ctx.cloud_knn(cdb, cdb, k, -1.0, squared), want(c, "self", k, squared), ("A", k, squared))
                    assert_rows(ctx.cloud_knn(cdb, cq, k, -1.0, squared), want(c, "ext", k, squared), ("B", k, squared))
                for k in (3, 7, 8, 9, 17, 32):
                    for r in (0.3, 0.25, 0.0):
                        for which, cloud in (("self", cdb), ("ext", cq)):
                            got = ctx.cloud_knn(cdb, cloud, k, r, squared)
                            assert_rows(got, want(c, which, k, squared, r), (which, k, r, squared))
                            if which == "self":
                                assert got[2].max() == (min(k, 7) if r == 0.3 else 1 if r == 0.25 else 0)
            assert scopes(ctx)[1] == 0 and scopes(ctx)[0] == 2 * (64 + 36)
            assert ctx.prof_get("grid_build")[0] >= 2                                      # 343 points: never the cloud's own grid


@pytest.mark.gpu
def test_small_clouds_walk_their_own_grid(ctx):
    """under 256 points and k <= 4 the walk runs on the cloud's own x-sorted 1-NN grid: one grid_build (that grid), a second one from k = 5 on"""
    for c in (cases.small_lattice_case(6), cases.coincident_case(200), cases.coincident_case(300)):
        with handles(ctx, c) as (cdb, cq, h):
            with tuned(ctx, prof=2):
                for squared in (True, False):
                    for k in (1, 2, 3, 4):
                        assert_rows(ctx.cloud_knn(cdb, cdb, k, -1.0, squared), ref_knn(c.db, c.db, k, squared=squared), (c.name, "A", k, squared))
                        assert_rows(ctx.cloud_knn(cdb, cq, k, -1.0, squared), want(c, "ext", k, squared), (c.name, "B", k, squared))
                small = c.db.shape[0] < 256
                assert ctx.prof_get("grid_build")[0] == (1 if small else 2), c.name
                for k in (5, 8, 32):
                    assert_rows(ctx.cloud_knn(cdb, cdb, k), ref_knn(c.db, c.db, k), (c.name, "A", k))
                    assert_rows(ctx.cloud_knn(cdb, cq, k, -1.0, False), want(c, "ext", k, False), (c.name, "B", k))
                assert ctx.prof_get("grid_build")[0] >= 2 and scopes(ctx)[1] == 0, c.name


@pytest.mark.gpu
def test_tie_shell_under_the_strict_cap(ctx):
    """150 points at exactly s = 625 / 65536 in several cells: k = 8, 16, 32 take the k lowest indices; radius = 25 / 256 excludes the whole
    shell (strict), the next double admits it"""
    c = cases.shell_case()
    up = float(np.nextafter(cases.R_SHELL, 1.0))
    with handles(ctx, c) as (cdb, cq, h):
        for squared in (True, False):
            for k in (8, 16, 32):
                for r, n_found in ((-1.0, k), (cases.R_SHELL, 0), (up, k)):
                    got = ctx.cloud_knn(cdb, cq, k, r, squared)
                    assert_rows(got, want(c, "ext", k, squared, r), (k, r, squared))
                    assert got[2][0] == n_found and (n_found == 0 or np.array_equal(got[0][0], c.shell_at[:k]))
                    assert_rows(ctx.cloud_knn(cdb, cdb, k, r, squared), want(c, "self", k, squared, r), ("self", k, r, squared))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2, 5])
def test_small_and_empty(ctx, n):
    """n in {0, 1, 2, 5} with k up to 32 on the cloud routes and the handle (fewer than 4 096 points: the scan), and an empty query set"""
    rng = np.random.default_rng(7)
    db = rng.integers(-8, 8, (n, 3)) / 4.0
    q = np.concatenate([db, rng.integers(-8, 8, (20, 3)) / 4.0])
    cdb, cq, h = ctx.cloud(soa32(db)), ctx.cloud(soa32(q)), ctx.db64(db)
    empty = ctx.cloud(np.zeros((3, 0), np.float32))
    try:
        for squared in (True, False):
            for k in (1, 4, 5, 32):
                ref = ref_knn(db, q, k, squared=squared)
                assert_rows(ctx.cloud_knn(cdb, cq, k, -1.0, squared), ref, ("B", n, k, squared))
                assert_rows(ctx.cloud_knn(cdb, cdb, k, -1.0, squared), ref_knn(db, db, k, squared=squared), ("A", n, k, squared))
                assert (ref[2] == min(n, k)).all()
                for keys in ({}, dict(knn_slices=OFF)):
                    with tuned(ctx, prof=2, **keys):
                        assert_rows(h.knn(q, k, squared), ref[:2], ("E/F", n, k, squared))
                        assert_rows(h.knn(q[:3], k, squared), (ref[0][:3], ref[1][:3]), ("E/F", n, k, squared))
                        assert scopes(ctx) == (0, 2)
                if not squared:
                    assert_rows(ctx.knn_f64(db, q, k), ref[:2], ("pcr_knn_f64", n, k))
                assert ctx.cloud_knn(cdb, empty, k, -1.0, squared)[0].shape == (0, k)
                assert h.knn(np.zeros((0, 3)), k, squared)[0].shape == (0, k)
    finally:
        for o in (h, empty, cq, cdb):
            o.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 511, 512, 513, 1025])
def test_exhaustive_scan_tile_and_slice_edges(ctx, n):
    """routes E and F at n around the LDS tile (512) and m around the workgroup (256): the sliced launch cuts n = 1 025 into slices of 512, 512
    and ONE point (unused slots meet real entries in knn_merge_kernel), the tie set 510 ... 514 straddles its first cut and the first tile edge of
    the one-slice launch.  Sliced and one-slice results are equal to each other and to the reference."""
    for m in (1, 255, 256, 257):
        c = cases.scan_case(n, m)
        h = ctx.db64(c.db)
        try:
            for squared in (True, False):
                for k in (1, 4, 5, 8, 32):
                    ref = ref_knn(c.db, c.q, k, squared=squared)
                    with tuned(ctx, prof=2):
                        sliced = h.knn(c.q, k, squared)
                        assert scopes(ctx) == (0, 1)
                    with tuned(ctx, prof=2, knn_slices=OFF):
                        whole = h.knn(c.q, k, squared)
                        assert scopes(ctx) == (0, 1)
                    assert_rows(sliced, ref[:2], (n, m, k, squared, "sliced"))
                    assert_rows(whole, ref[:2], (n, m, k, squared, "one slice"))
        finally:
            h.free()


@pytest.mark.gpu
def test_one_wave_ticket_across_calls_of_changing_size(ctx):
    """one context, one handle: calls of 1, 16, 16, 3, 1 queries (the ticket counts modulo m and is reset when m changes), a direct call of 17,
    then 16 and 2 — every call against the reference"""
    c = cases.lattice_case()
    h = ctx.db64(c.db)
    try:
        for squared, k in ((True, 8), (False, 5), (True, 32)):
            ref = want(c, "ext", k, squared)
            at = 0
            for m in (1, 16, 16, 3, 1, 17, 16, 2):
                with tuned(ctx, prof=2):
                    got = h.knn(c.q[at:at + m], k, squared)
                    assert scopes(ctx) == ((1, 0) if m == 17 else (0, 0)), m       # no scope at all: the one-wave route
                assert_rows(got, (ref[0][at:at + m], ref[1][at:at + m]), (squared, k, m, at))
                at += m
    finally:
        h.free()


@pytest.mark.gpu
def test_widened_grid_cache_follows_k(ctx):
    """the widened grid is cached in ONE slot with its factor min(2, sqrt(k / 4)): k = 4, 16, 4, 32, 1 on one cloud rebuilds it at every change of
    the factor (1, 2, 1, 2, 1) and keeps it when the factor stays (1 after 1, 32 after 16); then two clouds and their handles in turn"""
    c1, c2 = cases.bar_case(), cases.shell_case()
    with handles(ctx, c1) as (db1, q1, h1), handles(ctx, c2) as (db2, q2, h2):
        with tuned(ctx, prof=2):
            assert_rows(ctx.cloud_knn(db1, q1, 4), want(c1, "ext", 4, True), 4)
            first = ctx.prof_get("grid_build")[0]
            assert first == 2                                                      # the 1-NN grid (Morton order from 256 points on) and the widened one
            for k in (16, 4, 32, 1, 1, 16, 32):
                assert_rows(ctx.cloud_knn(db1, q1, k, -1.0, k != 4), want(c1, "ext", k, k != 4), k)
                assert_rows(ctx.cloud_knn(db1, db1, k), want(c1, "self", k, True), k)
            assert ctx.prof_get("grid_build")[0] == first + 5                      # 16, 4, 32, 1 and the 16 after 1; 1 -> 1 and 16 -> 32 keep the slot
        for k1, k2 in ((16, 4), (4, 32), (9, 9), (1, 17)):
            assert_rows(ctx.cloud_knn(db1, q1, k1), want(c1, "ext", k1, True), (k1, k2))
            assert_rows(ctx.cloud_knn(db2, q2, k2, -1.0, False), want(c2, "ext", k2, False), (k1, k2))
            assert_rows(h1.knn(c1.q, k2), want(c1, "ext", k2, False)[:2], (k1, k2))
            assert_rows(h2.knn(c2.q[:16], k1, True), tuple(a[:16] for a in want(c2, "ext", k1, True)[:2]), (k1, k2))


# ------------------------------------------------------------------------------------------------------------------- normals
# pcr_normals_knn_f64 = the squared-mode self-query with the cap `radius`, then the closed-form solver of csrc/eig3.hpp on the scatter matrix of every
# neighbourhood.  The constructed clouds put it on each branch: exactly planar (a zero eigenvalue), collinear (a double zero), coincident
# (big == 0), exactly isotropic (off2 == 0: the diagonal branch), fewer than 3 neighbours.
#
# The bounds.  orc.normals_knn_f64 runs the same algorithm with the host's libm; its deviation from the EXACT normal (planes, triangles), from
# the line's direction (lines) or from numpy.linalg.eigh (the scan) was measured on the CPU and is recorded below.  A bound is that value
# times FACTOR (the factor this project uses elsewhere) — or FLOOR = 64 ulp of 1.0 where the oracle's deviation is 0 — and the GPU's output has
# to meet it against the same exact normal / direction / eigh, never against the oracle.  *_GPU_WORST: the GPU's worst value, recorded after the run.
FACTOR = 8
FLOOR = 64 * 2.0 ** -52
PLANES_ORACLE_WORST = 3.3306690738754696e-16      # max of 1 - |n . n_true| over the plane and the tilted plane, both neighbourhood shapes
LINES_ORACLE_WORST = 9.208587861650769e-18        # max of |n . v| over the four lines, both shapes (the three axis lines: exactly 0)
TRIANGLES_ORACLE_WORST = 0.0                      # max of 1 - |n . n_true| over the 40 triangles of the sparse cloud
SCAN_ORACLE_WORST = 7.771561172376096e-16         # max of 1 - |n . v0(eigh)| over the separated rows of synth.kitti_like_scan(3000), k = 10, r = 5
# measured on an MI355X, as a share of the bound: the device's acos / cos move none of these figures off the oracle's
PLANES_GPU_WORST = 0.125                          # 3.3306690738754696e-16 (the tilted plane, k = 10), bound 2.66e-15
LINES_GPU_WORST = 0.125                           # 9.208587861650769e-18 (the diagonal, both shapes; the axis lines: 0), bound 7.37e-17
TRIANGLES_GPU_WORST = 0.0                         # 0.0, bound FLOOR = 1.42e-14
SCAN_GPU_WORST = 0.125                            # 7.771561172376096e-16 with every non-zero row compared (share 1.0), bound 6.22e-15
NORMAL_RUNS = (("plane", cases.plane_case, 10, -1.0), ("plane", cases.plane_case, 9, 0.3),
               ("plane", cases.tilted_plane_case, 10, -1.0), ("plane", cases.tilted_plane_case, 7, 0.4),
               ("line", lambda: cases.line_case("x"), 10, -1.0), ("line", lambda: cases.line_case("x"), 5, 0.04),
               ("line", lambda: cases.line_case("y"), 10, -1.0), ("line", lambda: cases.line_case("y"), 5, 0.04),
               ("line", lambda: cases.line_case("z"), 10, -1.0), ("line", lambda: cases.line_case("z"), 5, 0.04),
               ("line", lambda: cases.line_case("diag"), 10, -1.0), ("line", lambda: cases.line_case("diag"), 5, 0.04),
               ("zero", lambda: cases.coincident_case(4096), 10, -1.0), ("triangle", cases.sparse_case, 10, 1.0),
               ("isotropic", cases.lattice_case, 7, 0.3))
ORACLE_WORST = {"plane": PLANES_ORACLE_WORST, "line": LINES_ORACLE_WORST, "triangle": TRIANGLES_ORACLE_WORST}


def bound(oracle_worst):
    return FACTOR * oracle_worst if oracle_worst > 0 else FLOOR


def neighbourhoods(name, db, k, radius):
    """-> (idx, found, A): the reference's neighbour lists and the scatter matrix (xx xy xz yy yz zz) of every row, summed in neighbour order as
    pca_normal.py does: centre = sum / n, A = sum (p - c)(p - c)^T"""
    def make():
        idx, _, found = ref_knn(db, db, k, radius, True)
        s = np.zeros((db.shape[0], 3))
        for col in range(k):
            s = s + np.where((col < found)[:, None], db[idx[:, col]], 0.0)
        d_all = s / np.maximum(found, 1)[:, None]
        A = np.zeros((db.shape[0], 6))
        for col in range(k):
            d = db[idx[:, col]] - d_all
            A = A + np.where((col < found)[:, None], np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2], d[:, 2] * d[:, 2]], 1), 0.0)
        return idx, found, A
    return cached(("nbh", name, k, float(radius)), make)


def check_rows(nrm, found, A, what):
    """every output row is finite and either all zero or of norm 1 (1e-9: the bound of the existing normals test); the zero rows are exactly those
    with fewer than 3 neighbours or a scatter matrix whose signed maximum coefficient is 0.  -> the zero mask"""
    assert np.isfinite(nrm).all(), what
    zero = (nrm == 0).all(1)
    assert (np.abs(np.linalg.norm(nrm[~zero], axis=1) - 1.0) <= 1e-9).all(), what
    assert np.array_equal(zero, (found < 3) | (A.max(1) == 0)), what
    return zero


def constructed_deviation(kind, c, nrm, found, A, what):
    zero = check_rows(nrm, found, A, what)
    if kind == "plane":
        assert not zero.any()
        return float((1.0 - np.abs(nrm @ c.normal)).max())
    if kind == "line":
        assert zero.sum() <= 2                                              # (the two ends of the capped line see 2 neighbours)
        return float(np.abs(nrm[~zero] @ c.direction).max())
    if kind == "zero":
        assert zero.all()
        return 0.0
    if kind == "triangle":
        assert np.array_equal(zero, c.kinds < 3) and np.array_equal(found, c.kinds)       # 1, 2 and exactly 3 neighbours
        return float((1.0 - np.abs(nrm[~zero] @ c.normal)).max())
    inner = found == 7                                                       # isotropic: the point and its six face neighbours, A = diag(a, a, a)
    assert inner.sum() == 14 ** 3 and (A[inner][:, [1, 2, 4]] == 0).all() and (A[inner, 0] == A[inner, 3]).all() and (A[inner, 0] == A[inner, 5]).all()
    assert (nrm[inner] == [0.0, 0.0, 1.0]).all(), what                       # the diagonal branch: no arithmetic at all
    return 0.0


def scan_deviation(nrm, found, A):
    """sign-free against numpy.linalg.eigh on the rows whose two smallest eigenvalues are separated (w1 - w0 > 1e-6 w2, the rule of
    test_oracle_normals_match_numpy_eigh) -> (worst 1 - |n . v0|, share of the non-zero rows compared)"""
    zero = check_rows(nrm, found, A, "scan")
    w, v = np.linalg.eigh(np.stack([A[:, [0, 1, 2]], A[:, [1, 3, 4]], A[:, [2, 4, 5]]], 1))
    sep = (w[:, 1] - w[:, 0] > 1e-6 * w[:, 2]) & ~zero
    return float((1.0 - np.abs((nrm[sep] * v[sep][:, :, 0]).sum(1))).max()), sep.sum() / (~zero).sum()


RUN_IDS = [f"{make().name if kind != 'zero' else 'coincident'}-k{k}-r{radius}" for kind, make, k, radius in NORMAL_RUNS]


def constructed_run(run, normals_of):
    """one of NORMAL_RUNS through normals_of(case, k, radius): the row rules, then the family's deviation against its bound -> (case, normals, found)"""
    kind, make, k, radius = NORMAL_RUNS[run]
    c = make()
    _, found, A = neighbourhoods(c.name, c.db, k, radius)
    nrm = normals_of(c, k, radius)
    dev = constructed_deviation(kind, c, nrm, found, A, RUN_IDS[run])
    if kind in ORACLE_WORST:
        print(RUN_IDS[run], "deviation", dev, "bound", bound(ORACLE_WORST[kind]))
        assert dev <= bound(ORACLE_WORST[kind]), (RUN_IDS[run], dev, bound(ORACLE_WORST[kind]))
    return c, nrm, found


@pytest.mark.parametrize("run", range(len(NORMAL_RUNS)), ids=RUN_IDS)
def test_oracle_normals_on_every_solver_branch(orc, run):
    c, nrm, _ = constructed_run(run, lambda c, k, radius: orc.normals_knn_f64(soa32(c.db), k, radius))
    if c.name == "line_z":
        # diag(a, a, b), a < b: x, not the reference function's z (the direction of the line itself) — csrc/eig3.hpp REF_TIES
        assert (nrm[(nrm != 0).any(1)] == [1.0, 0.0, 0.0]).all()


def test_oracle_normals_of_a_scan_meet_the_condition(orc, synth):
    scan = synth.kitti_like_scan(3000)
    _, found, A = neighbourhoods("scan3000", scan.T.astype(np.float64), 10, 5.0)
    dev, share = scan_deviation(orc.normals_knn_f64(scan, 10, 5.0), found, A)
    print("oracle, scan: worst", dev, "compared", share)
    assert share >= 0.9 and dev <= bound(SCAN_ORACLE_WORST)                  # the oracle alone meets the condition on this cloud


def gpu_normals(ctx):
    def run(c, k, radius):
        cloud = ctx.cloud(soa32(c.db))
        try:
            return ctx.normals(cloud, k, radius)
        finally:
            cloud.free()
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("run", range(len(NORMAL_RUNS)), ids=RUN_IDS)
def test_gpu_normals_on_every_solver_branch(ctx, orc, run):
    c, nrm, found = constructed_run(run, gpu_normals(ctx))
    if NORMAL_RUNS[run][0] == "isotropic":                                   # no trigonometry on these rows: bit-equal to the oracle
        want_n = orc.normals_knn_f64(soa32(c.db), *NORMAL_RUNS[run][2:])
        assert np.array_equal(bits64(nrm[found == 7]), bits64(want_n[found == 7]))


@pytest.mark.gpu
def test_gpu_normals_of_a_scan_against_eigh(ctx, synth):
    scan = synth.kitti_like_scan(3000)
    _, found, A = neighbourhoods("scan3000", scan.T.astype(np.float64), 10, 5.0)
    cloud = ctx.cloud(scan)
    try:
        dev, share = scan_deviation(ctx.normals(cloud, 10, 5.0), found, A)
    finally:
        cloud.free()
    print("GPU, scan: worst", dev, "bound", bound(SCAN_ORACLE_WORST), "compared", share)
    assert share >= 0.9
    assert dev <= bound(SCAN_ORACLE_WORST), (dev, bound(SCAN_ORACLE_WORST))
