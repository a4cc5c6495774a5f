"""Radius search on every route, row-length class and boundary (pcr_db64_radius, pcr_radius_f64, pcr_db64_radius_rows).

Three implementations answer a radius search: the exhaustive LDS-tiled scan (csrc/search_f64.hip radius_f64_kernel, the database in
slices for small batches), the fused grid route (csrc/radius_grid.hip: count pass + radius_emit_kernel<CAP>, CAP = 1024 ... 16384 chosen
per row by its length) and the sorted grid route (radius_grid_kernel<true> + rocPRIM segmented sort + radius_dist_kernel: rows beyond
16 384 neighbours, databases beyond 262 144 points, or the fused route switched off).  Every test here compares with orc.radius_f64,
the CPU restatement of hw2's kd-tree contract — d = sqrt(((dx^2) + dy^2) + dz^2) in f64, member iff d <= r, rows in ascending index
order — and asks for EQUALITY of row offsets, indices and distance bits.  Where a test claims a route it proves it with the profiler's
scopes: the fused route launches radius_emit and no radius_sort, the sorted route radius_sort and no radius_emit, the exhaustive route
neither.

The fixtures are built here from f32-representable coordinates (the f32 twin cloud needs them) and checked against the oracle in a CPU
test, so that a wrong builder cannot hide a failure:
  lattice   16^3 points at multiples of 0.25 (4 096 points: the twin cloud, and far more than 64 grid cells at r = 0.1)
  clusters  L distinct points on a 2^-10 sub-lattice (the first L of a 26^3 cube) centred in a lattice void (0.125 + 0.25 i, 1.875, 1.875):
            the void centre has exactly L neighbours at r = 0.1 (the cube's corner is 0.0211 from the centre, the nearest lattice point
            0.2165), L on both sides of every CAP class edge
  bar       2 048 points at x = 1 + k 2^-12, y = z = 2.125: more than 256 records in the three-cell x range, so clip_row_x<256> searches; a query
            at bar point 512 with r = 0.125 has 1 025 members, two of them at exactly d == r
  shell     the 150 integer vectors with |v|^2 = 625 scaled by 2^-8 around (0.125, 0.125, 0.125): all at exactly d == r = 25/256; a second
            copy one f32 ulp outward along the largest component, a third one ulp inward (inside member()'s f32 band: f64 decides)

Tune keys: the value 0 means "the default" for every key (tune_get), so "off" is the documented 2 for radius_fused, and 2 for knn_slices
(any value but 1 leaves the database in one slice); setting a key back to 0 restores the default."""
import math
from contextlib import contextmanager
from fractions import Fraction

import numpy as np
import pytest

R = 0.1
R_BAR = 0.125
R_SHELL = 25.0 / 256.0
L_EDGES = (1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384)
L_SMALL = (63, 64, 65)
SHELL_CENTRE = (0.125, 0.125, 0.125)
OFF = 2                                                    # tune value for "off" (0 is "the default")
_CACHE = {}


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def frozen(a):
    a = np.ascontiguousarray(a, np.float64)
    a.setflags(write=False)
    return a


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------- builders
def lattice():
    g = np.arange(16) * 0.25
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def void_centre(i):
    return np.array([0.125 + 0.25 * i, 1.875, 1.875])


def empty_voids(count):
    """centres of lattice voids that hold nothing (z = 3.625: away from the clusters, the bar and the shells)"""
    k = np.arange(count)
    return np.stack([0.125 + 0.25 * (k % 10), 0.125 + 0.25 * (k // 10), np.full(count, 3.625)], 1)


def cluster(L, centre):
    k = np.arange(L)
    off = np.stack([k % 26, (k // 26) % 26, k // 676], 1) - 12.5
    return np.asarray(centre) + off * 2.0 ** -10


def bar():
    k = np.arange(2048)
    return np.stack([1.0 + k * 2.0 ** -12, np.full(2048, 2.125), np.full(2048, 2.125)], 1)


def shells():
    """(on, outward, inward): 150 points each"""
    r = np.arange(-25, 26)
    v = np.array([(a, b, c) for a in r for b in r for c in r if a * a + b * b + c * c == 625])
    assert v.shape == (150, 3)
    on = (np.asarray(SHELL_CENTRE) + v / 256.0).astype(np.float32)
    assert np.array_equal(on.astype(np.float64), np.asarray(SHELL_CENTRE) + v / 256.0)
    rows, k = np.arange(150), np.argmax(np.abs(v), axis=1)
    away = (np.sign(v[rows, k]) * np.inf).astype(np.float32)
    out, inn = on.copy(), on.copy()
    out[rows, k] = np.nextafter(on[rows, k], away)
    inn[rows, k] = np.nextafter(on[rows, k], -away)
    return on.astype(np.float64), out.astype(np.float64), inn.astype(np.float64)


def shuffled(parts, seed):
    """the parts stacked and put in a fixed random order: returns (database, position of every stacked row in it)"""
    pts = np.concatenate(parts)
    perm = np.random.default_rng(seed).permutation(pts.shape[0])
    where = np.empty(pts.shape[0], np.int64)
    where[perm] = np.arange(pts.shape[0])
    return frozen(pts[perm]), where


def cluster_db(Ls, with_bar=False, seed=11):
    """lattice + one cluster per L in the voids 0, 1, ... (+ the bar).  Returns (database, position of lattice point k, position of bar
    point k or None)."""
    def make():
        parts = [lattice()] + [cluster(L, void_centre(i)) for i, L in enumerate(Ls)] + ([bar()] if with_bar else [])
        db, where = shuffled(parts, seed)
        return db, where[:4096], (where[-2048:] if with_bar else None)
    return cached(("cluster_db", Ls, with_bar, seed), make)


def oracle(orc, key, db, q, r):
    def make():
        row, idx, dist = orc.radius_f64(db, q, r)
        for a in (row, idx, dist):
            a.setflags(write=False)
        return row, idx, dist
    return cached(("oracle", key, float(r) if r == r else "nan"), make)


def edge_case():
    """cluster database + 260 queries: the ten void centres, 200 lattice points, 50 empty voids"""
    db, lat_at, _ = cluster_db(L_EDGES)
    q = frozen(np.concatenate([[void_centre(i) for i in range(len(L_EDGES))], lattice()[::20][:200], empty_voids(50)]))
    return db, q, lat_at[::20][:200]


def long_row_case():
    """lattice + one cluster of 16 385: the void centre and three cluster points have rows beyond the largest class"""
    db, lat_at, _ = cluster_db((16385,))
    q = frozen(np.concatenate([[void_centre(0)], cluster(16385, void_centre(0))[[0, 9000, 16384]], lattice()[::200], empty_voids(5)]))
    return db, q


def boundary_case():
    """lattice + bar + the three shells; queries: every 37th bar point, bar point 512, the shell centre"""
    def make():
        db, where = shuffled([lattice(), bar()] + list(shells()), 12)
        q = frozen(np.concatenate([bar()[::37], bar()[512:513], [SHELL_CENTRE]]))
        return db, q, where[4096 + 2048:]
    return cached("boundary_case", make)


def rows_case():
    """cluster database + clusters of 63, 64, 65 + bar, 203 queries (not a multiple of 4) at r = 0.125: rows of 16 384 ... 1 023, 65, 64, 63
    (void centres), 1 025 (bar point 512: y and z constant), shorter bar rows, 1 (lattice points) and 0 (empty voids)"""
    db, lat_at, _ = cluster_db(L_EDGES + L_SMALL, with_bar=True)
    nv = len(L_EDGES) + len(L_SMALL)
    q = np.concatenate([[void_centre(i) for i in range(nv)], bar()[[512, 0, 5, 63, 100, 300, 1600, 2000, 2047]], empty_voids(50),
                        lattice()[::31][:131]])
    q = q[np.random.default_rng(13).permutation(q.shape[0])]                  # long and short rows share a workgroup
    assert q.shape[0] == 203
    return db, frozen(q)


def perturbed(db):
    return frozen(db + 1e-9 * np.arange(db.shape[0])[:, None])                 # not f32-representable: no twin cloud, the exhaustive route


# ------------------------------------------------------------------------------------------------- exact reductions and their bounds
def exact_ints(db):
    """every coordinate as an integer multiple of 2^-K (exact: the values are binary fractions)"""
    ratios = [v.as_integer_ratio() for v in db.ravel().tolist()]
    K = max(d.bit_length() - 1 for _, d in ratios)
    X = np.array([n << (K - (d.bit_length() - 1)) for n, d in ratios], dtype=object).reshape(-1, 3)
    return X, K


PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))                       # xx xy xz yy yz zz


def lane_sum(v):
    """the kernels' order: lane l adds entries l, l + 64, ... one after the other, then a xor tree over the 64 lanes"""
    L = v.shape[0]
    pad = np.zeros(((L + 63) // 64 * 64,) + v.shape[1:])
    pad[:L] = v
    acc = np.zeros((64,) + v.shape[1:])
    for chunk in pad.reshape((-1, 64) + v.shape[1:]):
        acc = acc + chunk
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[np.arange(64) ^ o]
    return acc[0]


def emulate_reductions(db, row, idx, dist):
    """numpy restatement of rows_reduce_kernel / rows_moments_kernel (same order of additions, s * (1 / cnt), no fused multiply-add)"""
    m = row.size - 1
    mx, sm, mean, cov = np.zeros(m), np.zeros(m), np.zeros((m, 3)), np.zeros((m, 6))
    for i in range(m):
        L = int(row[i + 1] - row[i])
        if L == 0:
            continue
        d, P = dist[row[i]:row[i + 1]], db[idx[row[i]:row[i + 1]]]
        mx[i], sm[i] = d.max(), lane_sum(d)
        inv = 1.0 / float(L)
        mean[i] = lane_sum(P) * inv
        c = P - mean[i]
        cov[i] = lane_sum(np.stack([c[:, a] * c[:, b] for a, b in PAIRS], 1)) * inv
    return np.diff(row).astype(np.float64), mx, sm, mean, cov


def check_reductions(db, row, idx, dist, cnt, mx, sm, mean, cov):
    """COUNT and MAX_DIST exactly; SUM_DIST against math.fsum; mean and covariance of EVERY row against exact rational arithmetic.

    Derivation of the bounds (u = 2^-53, L entries in the row).  A lane adds ceil(L / 64) entries one after the other — the first
    addition, to zero, is exact, so ceil(L / 64) - 1 of them round — and six tree levels follow: every entry passes through at most
    depth = ceil(L / 64) + 5 rounded additions.
      SUM_DIST  all terms are non-negative, so |sum^ - sum| <= depth u sum (1 + O(u)); the bound (depth + 1) 2^-52 sum keeps a factor 2.
      mean      m^ = fl(fl-sum * fl(1 / L)): the summation gives depth u sum|x| / L, the reciprocal and the product one u each, so
                |m^ - m| <= (depth + 2) u mean|x| (1 + O(u)); the bound is (depth + 3) 2^-52 mean|x|, again a factor 2 above.
      cov       c^_ij = fl(fl-sum of fl(dx^ dy^) * inv) with dx^ = fl(x - m^_x) = (x - m_x - e_x)(1 + O(u)), e = m^ - m.  Because
                sum (x - m_x) = 0 the shifted sum is exact in e: sum (x - m_x - e_x)(y - m_y - e_y) / L = c_ij + e_x e_y.
                Rounding: two differences, one product, depth additions, the reciprocal and the last product: at most (depth + 5) u
                relative to sum |dx^ dy^| / L, which is <= sqrt(c^_ii c^_jj) by Cauchy-Schwarz — the first term, a = (depth + 4) 2^-52.
                The rounded mean enters sum |dx^ dy^| and the roundings of the differences through |e| <= (depth + 2) u A, A = the
                largest |coordinate| of the row: cross terms of size |e_x| sqrt(c_jj) + |e_y| sqrt(c_ii) times O(depth u) — far
                below b A (sqrt(c_ii) + sqrt(c_jj)) with b = 2^-50 — and e_x e_y itself.  When c_ii = 0 exactly (the bar rows: every
                y equal) the sums are exact multiples of y, e comes from the reciprocal and one product only, |e| <= 2 u A, and
                c^_ii = e^2 <= 2^-104 A^2: the third term A^2 2^-100."""
    m = row.size - 1
    assert np.array_equal(cnt, np.diff(row).astype(np.float64))
    X, K = exact_ints(db)
    one = 1 << K
    worst = {"sum": 0.0, "mean": 0.0, "cov": 0.0}
    for i in range(m):
        L = int(row[i + 1] - row[i])
        if L == 0:
            assert mx[i] == 0.0 and sm[i] == 0.0 and not mean[i].any() and not cov[i].any(), i
            continue
        d, j = dist[row[i]:row[i + 1]], idx[row[i]:row[i + 1]]
        depth = (L + 63) // 64 + 5
        assert mx[i] == d.max(), (i, L)
        want = math.fsum(d.tolist())
        assert abs(sm[i] - want) <= (depth + 1) * 2.0 ** -52 * want, (i, L, sm[i], want)
        worst["sum"] = max(worst["sum"], abs(sm[i] - want) / ((depth + 1) * 2.0 ** -52 * want) if want else 0.0)
        P = X[j]
        A = Fraction(int(max(abs(v) for v in P.ravel().tolist())), one)
        em = [Fraction(int(P[:, a].sum()), L * one) for a in range(3)]
        mabs = [Fraction(int(sum(abs(v) for v in P[:, a].tolist())), L * one) for a in range(3)]
        ec = [Fraction(int((P[:, a] * P[:, b]).sum()), L * one * one) - em[a] * em[b] for a, b in PAIRS]
        for a in range(3):
            err, tol = abs(Fraction(float(mean[i, a])) - em[a]), Fraction(depth + 3, 1 << 52) * mabs[a]
            assert err <= tol, (i, L, a, float(err), float(tol))
            worst["mean"] = max(worst["mean"], float(err / tol) if tol else 0.0)
        sd = [math.sqrt(float(ec[k])) for k in (0, 3, 5)]
        for k, (a, b) in enumerate(PAIRS):
            tol = (depth + 4) * 2.0 ** -52 * sd[a] * sd[b] + 2.0 ** -50 * float(A) * (sd[a] + sd[b]) + float(A * A) * 2.0 ** -100
            err = abs(Fraction(float(cov[i, k])) - ec[k])
            assert err <= Fraction(tol), (i, L, k, float(err), tol)
            worst["cov"] = max(worst["cov"], float(err) / tol if tol else 0.0)
    return worst


# --------------------------------------------------------------------------------------------------------------- CPU: the builders
def test_builders_give_the_rows_the_gpu_tests_rely_on(orc):
    for pts in (lattice(), cluster(16385, void_centre(0)), bar()) + shells():
        assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)                # f32-representable
        assert np.unique(pts, axis=0).shape[0] == pts.shape[0]                                # distinct
    # class edges: the void centres have exactly L neighbours, nothing within 0.01 of r
    db, q, lat_at = edge_case()
    assert db.shape[0] == 52227 and q.shape[0] == 260
    row, idx, dist = oracle(orc, "edge", db, q, R)
    n_row = np.diff(row)
    assert tuple(n_row[:10]) == L_EDGES
    assert (n_row[10:210] == 1).all() and np.array_equal(idx[row[10:210]], lat_at) and (n_row[210:] == 0).all()
    for r in (R - 0.01, R + 0.01):
        assert np.array_equal(np.diff(orc.radius_f64(db, q, r)[0]), n_row)
    assert (np.diff(idx[row[9]:row[10]]) > 0).all() and not np.array_equal(db[:4096], lattice())   # ascending index is not the build order
    # a row beyond the largest class
    db, q = long_row_case()
    assert db.shape[0] == 20481
    n_row = np.diff(oracle(orc, "long", db, q, R)[0])
    assert (n_row[:4] == 16385).all() and (n_row[4:-5] == 1).all() and (n_row[-5:] == 0).all()
    # bar and shells: members at exactly d == r
    db, q, shell_at = boundary_case()
    assert db.shape[0] == 4096 + 2048 + 450
    row, idx, dist = oracle(orc, "boundary", db, q, R_BAR)
    k512 = q.shape[0] - 2
    d512 = dist[row[k512]:row[k512 + 1]]
    assert d512.size == 1025 and (d512 == R_BAR).sum() == 2
    assert row[-1] - row[-2] == 450                                                           # the shell centre sees all three copies
    row, idx, dist = oracle(orc, "boundary", db, q, R_SHELL)
    members, d_c = idx[row[-2]:row[-1]], dist[row[-2]:row[-1]]
    assert (d_c == R_SHELL).sum() >= 100
    assert np.isin(shell_at[:150], members).all() and np.isin(shell_at[300:], members).all()   # on the sphere and one ulp inside
    assert (~np.isin(shell_at[150:300], members)).sum() >= 100                                  # one ulp outside
    assert (dist[: row[-3]] == R_SHELL).any()                                                   # bar rows: k +- 400 at exactly r
    # rows: the lengths the reductions are tested at
    db, q = rows_case()
    row, idx, dist = oracle(orc, "rows", db, q, R_BAR)
    n_row = np.diff(row)
    for L in L_EDGES + L_SMALL + (0, 1):
        assert (n_row == L).any(), L
    assert (n_row == 1025).sum() == 2                                                           # the cluster and bar point 512
    for r in (R_BAR - 0.01, R_BAR + 0.01):                                                      # the cluster rows are as far from r here
        nv = np.isin(n_row, L_EDGES + L_SMALL) & ~np.isclose(q[:, 1], 2.125)
        assert np.array_equal(np.diff(orc.radius_f64(db, q[nv], r)[0]), n_row[nv])


def test_reduction_bounds_admit_the_kernels_order_of_operations(orc):
    db, q = rows_case()
    for key, base in (("rows", db), ("rows_perturbed", perturbed(db))):
        row, idx, dist = oracle(orc, key, base, q, R_BAR)
        worst = check_reductions(base, row, idx, dist, *emulate_reductions(base, row, idx, dist))
        print(key, "largest error / bound:", worst)


# --------------------------------------------------------------------------------------------------------------------- GPU
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


def route(ctx):
    """which implementation answered since the last prof_reset (the scopes need tune prof >= 2)"""
    count, emit, sort = (ctx.prof_get(k)[0] for k in ("radius_count", "radius_emit", "radius_sort"))
    assert count > 0                                                     # every route counts first: the profiler is on
    return {(True, False): "fused", (False, True): "sorted", (False, False): "exhaustive"}.get((emit > 0, sort > 0), "mixed")


def assert_rows(got, want, what=None):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(bits64(got[2]), bits64(want[2])), what


def row_of(res, i):
    row, idx, dist = res
    return idx[row[i]:row[i + 1]], bits64(dist[row[i]:row[i + 1]])


@pytest.mark.gpu
def test_class_edges_on_the_fused_route(ctx, orc):
    """rows of CAP and CAP + 1 for every class: the N > CAP guard, the host's class choice, staging at full CAP, the emit loop's tail"""
    db, q, _ = edge_case()
    want = oracle(orc, "edge", db, q, R)
    h = ctx.db64(db)
    try:
        with tuned(ctx, prof=3, radius_method=2):
            assert_rows(h.radius(q, R), want)
            assert route(ctx) == "fused"
            assert ctx.prof_get("radius_emit")[0] == 1
            assert ctx.prof_get("radius_emit_class")[0] == 5             # one launch per non-empty class
    finally:
        h.free()


@pytest.mark.gpu
def test_sorted_route_forced_and_natural(ctx, orc):
    db, q, _ = edge_case()
    want = oracle(orc, "edge", db, q, R)
    h = ctx.db64(db)
    try:
        with tuned(ctx, prof=2, radius_method=2, radius_fused=OFF):
            forced = h.radius(q, R)
            assert route(ctx) == "sorted"
        with tuned(ctx, prof=2, radius_method=2, radius_fused=1):
            fused = h.radius(q, R)
            assert route(ctx) == "fused"
        assert_rows(forced, want)
        assert_rows(forced, fused)
    finally:
        h.free()
    db, q = long_row_case()
    want = oracle(orc, "long", db, q, R)
    h = ctx.db64(db)
    try:
        with tuned(ctx, prof=2):                                         # no route key: a row of 16 385 is beyond the largest class
            assert_rows(h.radius(q, R), want)
            assert route(ctx) == "sorted"
    finally:
        h.free()


@pytest.mark.gpu
def test_exhaustive_route_sliced_and_whole(ctx, orc):
    db, q, _ = edge_case()
    want = oracle(orc, "edge", db, q, R)
    h = ctx.db64(db)
    try:
        with tuned(ctx, prof=2, radius_method=1):                        # 260 queries: the database in slices
            assert_rows(h.radius(q, R), want)
            assert route(ctx) == "exhaustive"
        with tuned(ctx, prof=2, radius_method=1, knn_slices=OFF):
            assert_rows(h.radius(q, R), want)
            assert route(ctx) == "exhaustive"
            assert_rows(ctx.radius_f64(db, q, R), want)                   # the one-shot entry point
    finally:
        h.free()


@pytest.mark.gpu
@pytest.mark.parametrize("r", [R_BAR, R_SHELL])
def test_inclusive_boundary_and_clip_x_on_every_route(ctx, orc, r):
    db, q, _ = boundary_case()
    want = oracle(orc, "boundary", db, q, r)
    h = ctx.db64(db)
    try:
        for name, keys in (("exhaustive", dict(radius_method=1)), ("fused", dict(radius_method=2, radius_fused=1)),
                           ("sorted", dict(radius_method=2, radius_fused=OFF))):
            with tuned(ctx, prof=2, **keys):
                got = h.radius(q, r)
                assert route(ctx) == name
            assert_rows(got, want, name)
            row, _, dist = got
            assert (dist[: row[-2]] == r).any(), name                     # bar rows: members at exactly d == r
            if r == R_BAR:
                assert (dist[row[-3]:row[-2]] == r).sum() == 2, name      # bar point 512: both ends of its 1 025 members
            else:
                assert (dist[row[-2]:row[-1]] == r).sum() >= 100, name    # the shell
    finally:
        h.free()


@pytest.mark.gpu
def test_query_paths_small_batch_sorted_batch_and_self_query(ctx, orc):
    """the same points asked as a batch of 4 096 (pinned-host view, the order given), of 4 097 (query cloud, cell-sorted) and as the
    self query (record order), through the host rows and the handle"""
    db, _, _ = cluster_db((1023, 1024, 1025))
    want = oracle(orc, "three_self", db, db, R)
    h = ctx.db64(db)
    try:
        with tuned(ctx, prof=2, radius_method=2):
            small = h.radius(db[:4096], R)
            big = h.radius(db[:4097], R)
            every = h.radius(db, R)
            rows = h.radius_rows(None, R)
            assert route(ctx) == "fused"
        assert_rows(every, want)
        assert np.array_equal(rows.row_ptr(), want[0])
        i2, d2 = rows.fetch(0, db.shape[0])
        assert np.array_equal(i2, want[1]) and np.array_equal(bits64(d2), bits64(want[2]))
        rows.free()
        cut = want[0][4096]
        assert_rows(small, (want[0][:4097], want[1][:cut], want[2][:cut]))
        cut = want[0][4097]
        assert_rows(big, (want[0][:4098], want[1][:cut], want[2][:cut]))
    finally:
        h.free()


@pytest.mark.gpu
def test_grid_cache_follows_the_radius(ctx, orc):
    """one database handle searched at 0.1, 0.2, 0.1, 0.125: the grid kept on the cloud (and its by-index copy) is rebuilt with r"""
    db, _, _ = cluster_db((1023, 1024, 1025))
    q = frozen(np.concatenate([[void_centre(i) for i in range(3)], db[:297]]))
    h = ctx.db64(db)
    try:
        with tuned(ctx, prof=2, radius_method=2):
            for r in (0.1, 0.2, 0.1, 0.125):
                want = oracle(orc, "cache", db, q, r)
                assert_rows(h.radius(q, r), want, r)
                fresh = ctx.db64(db)
                try:
                    assert_rows(fresh.radius(q, r), want, r)
                finally:
                    fresh.free()
            assert route(ctx) == "fused"
            assert ctx.prof_get("radius_grid_build")[0] == 4 + 4             # every change of r on the kept handle, every fresh handle
    finally:
        h.free()


@pytest.mark.gpu
def test_non_finite_and_far_queries(ctx, orc):
    db, _, _ = cluster_db((1023, 1024, 1025))
    fin = np.concatenate([[void_centre(i) for i in range(3)], db[:37]])
    inf = np.inf
    odd = np.array([[inf, 1.875, 1.875], [0.125, -inf, 1.875], [inf, inf, -inf], [-inf, -inf, -inf]])
    q_inf = np.concatenate([fin[:5], odd[:2], fin[5:], odd[2:]])
    q_nan = np.concatenate([q_inf, [[np.nan, 1.875, 1.875], [0.125, 1.875, np.nan]], fin[:3]])
    coarse = np.concatenate([fin[:3], lattice()[::300]])                 # multiples of 2^-3: still f32-representable 10^4 away
    far = np.concatenate([fin[:7], coarse + 1e4, fin[7:], coarse - 1e4, fin[:2]])
    assert np.array_equal(far.astype(np.float32).astype(np.float64), far)
    base = oracle(orc, "odd_fin", db, fin, R)
    h = ctx.db64(db)
    try:
        for name, q, want_route in (("inf", q_inf, "fused"), ("nan", q_nan, "exhaustive"), ("far", far, "fused")):
            want = oracle(orc, "odd_" + name, db, q, R)
            with tuned(ctx, prof=2, radius_method=2):
                got = h.radius(q, R)
                assert route(ctx) == want_route, name                     # infinity is f32-representable and stays on the grid, NaN is not
            assert_rows(got, want, name)
            n_row = np.diff(got[0])
            assert (n_row[~np.isfinite(q).all(axis=1)] == 0).all() and (n_row[np.abs(q).max(axis=1) > 1e3] == 0).all(), name
        # the finite rows are what they are without the odd ones
        keep = np.isfinite(q_inf).all(axis=1)
        with tuned(ctx, radius_method=2):
            got = h.radius(q_inf, R)
        for k, i in enumerate(np.flatnonzero(keep)):
            a, b = row_of(got, i), row_of(base, k)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        h.free()


@pytest.mark.gpu
def test_radius_below_the_cell_budget_and_degenerate_radii(ctx, orc):
    """r = 1e-4 is below extent / 4000: grid_build enlarges the cell; r = 0 matches duplicates only, r < 0 and r = NaN nothing"""
    lat = lattice()
    pairs = lat[::5] + np.array([2.0 ** -14, 0.0, 0.0])
    db, _ = shuffled([lat, pairs, lat[::9]], 14)                          # partners 2^-14 away, exact duplicates
    q = frozen(np.concatenate([db[::3], [[0.125, 0.125, 0.125]]]))
    h = ctx.db64(db)
    try:
        want = oracle(orc, "tiny", db, q, 1e-4)
        assert np.diff(want[0]).max() >= 3 and np.diff(want[0]).min() == 0
        with tuned(ctx, prof=2, radius_method=2):
            assert_rows(h.radius(q, 1e-4), want)
            assert route(ctx) == "fused"
        for r in (0.0, -1.0, float("nan")):
            want = oracle(orc, "tiny", db, q, r)
            assert (want[0][-1] > q.shape[0] // 9) == (r == 0.0)
            for meth in (1, 2):
                with tuned(ctx, radius_method=meth):
                    assert_rows(h.radius(q, r), want, (r, meth))
    finally:
        h.free()


@pytest.mark.gpu
def test_database_points_with_an_infinite_coordinate(ctx, orc):
    """they go to the grid's non-finite cell: never members, and the indices of the rest do not move"""
    base, _, _ = cluster_db((1023, 1024, 1025))
    db = base.copy()
    at = (100, 5000)
    db[at[0]] = (np.inf, 1.875, 1.875)
    db[at[1]] = (0.125, -np.inf, 1.875)
    db = frozen(db)
    q = frozen(np.concatenate([[void_centre(i) for i in range(3)], base[90:110], base[4990:5010], [[np.inf, 1.875, 1.875]]]))
    want = oracle(orc, "inf_db", db, q, R)
    assert not np.isin(at, want[1]).any() and want[0][-1] == want[0][-2]
    h = ctx.db64(db)
    try:
        for name, keys in (("exhaustive", dict(radius_method=1)), ("fused", dict(radius_method=2)), ("sorted", dict(radius_method=2, radius_fused=OFF))):
            with tuned(ctx, prof=2, **keys):
                got = h.radius(q, R)
                assert route(ctx) == name
            assert_rows(got, want, name)
    finally:
        h.free()


@pytest.mark.gpu
def test_rows_reductions_against_exact_references(ctx, orc):
    """pcr_rows COUNT / MAX_DIST / SUM_DIST / moments on rows of 0, 1, 63, 64, 65, 1 025, ... 16 384 entries, 203 rows (four rows per
    workgroup: the last workgroup is partial), on the grid route and on the exhaustive route; the bounds are derived in
    check_reductions and shown to admit the kernels' order of operations by the CPU test above"""
    db, q = rows_case()
    for key, base, want_route in (("rows", db, "fused"), ("rows_perturbed", perturbed(db), "exhaustive")):
        want = oracle(orc, key, base, q, R_BAR)
        h = ctx.db64(base)
        try:
            with tuned(ctx, prof=2):
                rows = h.radius_rows(q, R_BAR)
                assert route(ctx) == want_route, key
            assert rows.m == 203 and np.array_equal(rows.row_ptr(), want[0]), key
            idx, dist = rows.fetch(0, 203)
            assert np.array_equal(idx, want[1]) and np.array_equal(bits64(dist), bits64(want[2])), key
            mean, cov = rows.moments()
            worst = check_reductions(base, *want, rows.reduce(rows.COUNT), rows.reduce(rows.MAX_DIST), rows.reduce(rows.SUM_DIST), mean, cov)
            print(key, "largest error / bound:", worst)
            rows.free()
        finally:
            h.free()
