"""The constructed clouds that tests/test_knn_routes.py puts through every k-NN route and through the normals.  Not a test module.

Every coordinate is a dyadic rational that f32 holds (the f32 twin cloud of a database needs that), so s = ((dx*dx) + dy*dy) + dz*dz is exact
and ties are exact ties; every database is shuffled with a fixed seed, so index order is not spatial order and "the lowest index wins" is a real
statement.  A case is a namespace: db (n, 3) f64, q (m, 3) f64 with the special queries FIRST (the one-wave route asks the first 48 only), and
whatever its property test needs (positions of named points in the shuffled database).  No case has more than 4 200 database points."""
from types import SimpleNamespace

import numpy as np

_CACHE = {}
P_COINCIDENT = (1.5, -2.25, 0.75)
SHELL_CENTRE = (0.125, 0.125, 0.125)
R_SHELL = 25.0 / 256.0
LINE_DIRS = {"x": (1.0, 0.0, 0.0), "y": (0.0, 1.0, 0.0), "z": (0.0, 0.0, 1.0), "diag": (1.0, 1.0, 1.0)}
F32_1E10 = float(np.float32(1e10))
F32_1E10_UP = float(np.nextafter(np.float32(1e10), np.float32(np.inf)))       # 1e10 + 1024
F32_3E38 = float(np.float32(3e38))


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def frozen(a):
    a = np.ascontiguousarray(a, np.float64)
    a.setflags(write=False)
    return a


def is_f32(a):
    a = np.asarray(a, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        back = a.astype(np.float32).astype(np.float64)
    return bool(((back == a) | (np.isnan(a) & np.isnan(back))).all())


def soa32(a):
    """(n, 3) f64 -> the (3, n) f32 rows Context.cloud takes"""
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, 3).T.astype(np.float32))


def shuffled(parts, seed):
    """the parts stacked and put in a fixed random order: (database, position of every stacked row in it)"""
    pts = np.concatenate([np.asarray(p, np.float64).reshape(-1, 3) for p in parts])
    perm = np.random.default_rng(seed).permutation(pts.shape[0])
    where = np.empty(pts.shape[0], np.int64)
    where[perm] = np.arange(pts.shape[0])
    return pts[perm], where


def case(name, db, q, **more):
    return SimpleNamespace(name=name, db=frozen(db), q=frozen(q), **more)


def lattice(nx=16, ny=16, nz=16, step=0.25):
    z, y, x = np.meshgrid(np.arange(nz) * step, np.arange(ny) * step, np.arange(nx) * step, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def void_centres(count, nx=15, ny=15):
    k = np.arange(count)
    return np.stack([0.125 + 0.25 * (k % nx), 0.125 + 0.25 * ((k // nx) % ny), 0.125 + 0.25 * (k // (nx * ny))], 1)


# ------------------------------------------------------------------------------------------------------------------ 1. lattice
def lattice_case():
    """16^3 points at multiples of 0.25.  Queries: the two clamped by cell_coord (1e7 and 3e38 on every axis), one just outside every face and
    corner, 60 void centres, 200 lattice points (the first 40 of them interior)."""
    def make():
        lat = lattice()
        db, where = shuffled([lat], 21)
        lo, hi, mid = -0.0625, 3.8125, 1.875
        faces = [[lo, mid, mid], [hi, mid, mid], [mid, lo, mid], [mid, hi, mid], [mid, mid, lo], [mid, mid, hi]]
        corners = [[a, b, c] for a in (lo, hi) for b in (lo, hi) for c in (lo, hi)]
        ijk = np.stack(np.unravel_index(np.arange(4096), (16, 16, 16)), 1)            # (z, y, x) of lattice row r
        interior = np.flatnonzero(((ijk >= 3) & (ijk <= 12)).all(1))[::25][:40]
        rest = np.setdiff1d(np.arange(4096)[::23], interior)[:160]
        pick = np.concatenate([interior, rest])
        q = np.concatenate([[[1e7, 1e7, 1e7], [F32_3E38] * 3], faces, corners, void_centres(60), lat[pick]])
        return case("lattice", db, q, n_special=16, interior=slice(76, 116), lattice_rows=slice(76, 276), at=where[pick])
    return cached("lattice", make)


def small_lattice_case(side):
    """side^3 lattice points (343: the list-width sweep on the widened grid; 216: under 256 points, the cloud's own x-sorted grid for k <= 4)"""
    def make():
        lat = lattice(side, side, side)
        db, _ = shuffled([lat], 22 + side)
        q = np.concatenate([[[-0.0625, 0.625, 0.625], [5.0, 5.0, 5.0]], void_centres(40, side - 1, side - 1), lat[::5]])
        return case(f"lattice{side}", db, q, n_special=2)
    return cached(("small_lattice", side), make)


# --------------------------------------------------------------------------------------------------------------- 2. coincident
def coincident_case(n):
    def make():
        p = np.asarray(P_COINCIDENT)
        q = np.concatenate([np.tile(p, (20, 1)), [p + (0.5, 0.0, 0.0), p + (0.0, 0.0, -1.0), [0.0, 0.0, 0.0]], np.tile(p, (30, 1))])
        return case(f"coincident{n}", np.tile(p, (n, 1)), q, n_special=23)
    return cached(("coincident", n), make)


# -------------------------------------------------------------------------------------------------------------------- 3. lines
def line_case(axis):
    """4 096 points along one direction at spacing 2^-6: t = -2047 ... 2047 (t = 0 is +0.0) and one more point at -0.0.  Along x this is one
    long x-row (clip_row_x, the x-sort key on negative values and on both zeros); along y and z rows of one cell; along the diagonal all three."""
    def make():
        t = np.concatenate([(np.arange(4095) - 2047) * 2.0 ** -6, [-0.0]])
        fixed = {"x": (None, 0.5, -0.25), "y": (0.5, None, -0.25), "z": (0.5, -0.25, None), "diag": (None, None, None)}[axis]
        pts = np.stack([t if f is None else np.full(t.size, f) for f in fixed], 1)
        db, where = shuffled([pts], 30 + "xyzd".index(axis[0]))
        inner = np.arange(100, 3995, 25)
        inner = inner[np.abs(inner - 2047) >= 40][:150]                                  # 16 neighbours a side, never the doubled zero (row 2047)
        assert inner.size == 150
        off = pts[::41][:100] + np.array([2.0 ** -7, 2.0 ** -5, -(2.0 ** -6)])
        far = 40.0 * np.asarray(LINE_DIRS[axis])
        q = np.concatenate([pts[[2047, 4095, 0, 4094]], [pts[0] - far, pts[4094] + far], pts[inner], off])
        return case(f"line_{axis}", db, q, n_special=6, inner=slice(6, 156), at=where[inner], zeros=where[[2047, 4095]],
                    direction=np.asarray(LINE_DIRS[axis]) / np.linalg.norm(LINE_DIRS[axis]))
    return cached(("line", axis), make)


# -------------------------------------------------------------------------------------------------------------------- 4. plane
def plane_case():
    """64 x 64 at spacing 0.25, z = 1"""
    def make():
        g = np.arange(64) * 0.25
        y, x = np.meshgrid(g, g, indexing="ij")
        pts = np.stack([x.ravel(), y.ravel(), np.ones(4096)], 1)
        db, _ = shuffled([pts], 40)
        corners = [[a, b, 1.0] for a in (0.0, 15.75) for b in (0.0, 15.75)]
        above = [[7.875, 7.875, 1.5], [0.0, 0.0, -3.0], [16.0, 16.0, 1.0]]
        cells = np.stack([0.125 + 0.25 * (np.arange(60) % 8) * 7, 0.125 + 0.25 * (np.arange(60) // 8) * 7, np.ones(60)], 1)
        q = np.concatenate([corners, above, pts[::21][:190], cells])
        return case("plane", db, q, n_special=7, normal=np.array([0.0, 0.0, 1.0]))
    return cached("plane", make)


def tilted_plane_case():
    """x + y + z = 16 on the integer lattice scaled by 2^-2: (i, j, 64 - i - j) / 4 for i, j < 64 (normals only)"""
    def make():
        j, i = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
        pts = np.stack([i.ravel(), j.ravel(), 64 - i.ravel() - j.ravel()], 1) * 0.25
        db, _ = shuffled([pts], 41)
        return case("tilted_plane", db, db[:1], normal=np.ones(3) / np.sqrt(3.0))
    return cached("tilted_plane", make)


# ------------------------------------------------------------------------------------------------------------- 5. far clusters
NEAR3 = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.5, 0.25]])


def far_case():
    """three points near the origin, the other 4 093 a thousand units away: a query in the small cluster crosses empty shells with fewer than k
    points seen"""
    def make():
        db, where = shuffled([NEAR3, lattice()[:4093] + 1000.0], 50)
        near_q = np.concatenate([NEAR3, [[0.125, 0.125, 0.0], [-1.0, -1.0, -1.0], [3.0, 0.0, 0.0], [500.0, 500.0, 500.0]]])
        q = np.concatenate([near_q, lattice()[:4093:45] + 1000.0, void_centres(30) + 1000.0])
        return case("far", db, q, n_special=7, near_at=where[:3])
    return cached("far", make)


# ---------------------------------------------------------------------------------------------------------------------- 6. bar
def bar_case():
    """2 048 points at x = 1 + j 2^-12, y = z = 1.125, inside the lower half of the lattice (16 x 16 x 8 points): far more than 32 records in
    every x-row through the bar, whatever cell edge the library picks"""
    def make():
        j = np.arange(2048)
        bar = np.stack([1.0 + j * 2.0 ** -12, np.full(2048, 1.125), np.full(2048, 1.125)], 1)
        lat = lattice(16, 16, 8)
        db, where = shuffled([lat, bar], 60)
        q = np.concatenate([bar[[0, 512, 1024, 2047]], bar[8::16], [[1.25, 1.125, 1.0], [0.875, 1.125, 1.125], [1.625, 1.125, 1.125]], void_centres(40), lat[::20][:100]])
        return case("bar", db, q, n_special=4, bar_rows=slice(0, 132), bar_at=where[2048:])
    return cached("bar", make)


# --------------------------------------------------------------------------------------------------------------- 7. tie shell
def shell_vectors():
    r = np.arange(-25, 26)
    v = np.array([(a, b, c) for a in r for b in r for c in r if a * a + b * b + c * c == 625])
    assert v.shape == (150, 3)
    return v


def shell_case():
    """the 150 integer vectors with |v|^2 = 625, scaled by 2^-8, around the void centre (0.125, 0.125, 0.125) of the lattice: all at exactly
    s = 625 / 65536 from it.  3 946 lattice points + the shell = 4 096."""
    def make():
        shell = np.asarray(SHELL_CENTRE) + shell_vectors() / 256.0
        lat = lattice()[:3946]
        db, where = shuffled([lat, shell], 70)
        q = np.concatenate([[SHELL_CENTRE], shell[::15], void_centres(40)[1:], lat[::40]])
        return case("shell", db, q, n_special=11, shell_at=np.sort(where[3946:]))
    return cached("shell", make)


# --------------------------------------------------------------------------------------------------- 8. collapsing square roots
def collapse_case():
    """query at the origin, a = (1, 0, 0), b = (1, 2^-26, 0): s_a = 1, s_b = 1 + 2^-52, both square roots are 1.0.  b has the LOWER index, so
    squared mode orders a, b and non-squared mode b, a.  The lattice is moved to [8, 11.75]^3: nothing else within 13 of the origin."""
    def make():
        a, b = [1.0, 0.0, 0.0], [1.0, 2.0 ** -26, 0.0]
        db, where = shuffled([lattice() + 8.0, [a], [b]], 80)
        ia, ib = int(where[4096]), int(where[4097])
        if ib > ia:
            db[[ia, ib]] = db[[ib, ia]]
            ia, ib = ib, ia
        q = np.concatenate([[[0.0, 0.0, 0.0], [0.0, 2.0 ** -27, 0.0], a, b], lattice()[::80] + 8.0, void_centres(10) + 8.0])
        return case("collapse", db, q, n_special=4, ia=ia, ib=ib)
    return cached("collapse", make)


# ------------------------------------------------------------------------------------------------------------ 9. the 1e10 rule
def rule_case():
    """three points near the origin, one at (1e10, 0, 0) — d == 1e10 exactly from the origin — one at the next f32 above (1e10 + 1024), and
    4 091 fillers at x = -(2^35 + j 2^12): more than 3.4e10 from the origin, so that they never crowd the far points out of a list.
    Queries: the origin; (1024, 0, 0), from which the SECOND far point lies at exactly 1e10 and the first inside; (0.25, 0, 0) and (-1, 0, 0),
    one step inside and outside; two fillers."""
    def make():
        near = [[0.25, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, -0.25]]
        far = [[F32_1E10, 0.0, 0.0], [F32_1E10_UP, 0.0, 0.0]]
        j = np.arange(4091)
        fill = np.stack([-(2.0 ** 35 + j * 2.0 ** 12), np.zeros(4091), np.zeros(4091)], 1)
        db, where = shuffled([near, far, fill], 90)
        q = np.concatenate([[[0.0, 0.0, 0.0], [1024.0, 0.0, 0.0], [0.25, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, -0.25]], fill[[0, 2000, 4090]], far,
                            [[5e9, 0.0, 0.0], [0.0, 1e10, 0.0], [0.0, 0.0, F32_1E10_UP]], fill[5::100]])
        return case("rule", db, q, n_special=13, near_at=where[:3], far_at=where[3:5])
    return cached("rule", make)


# --------------------------------------------------------------------------------------------------------------- 10. non-finite
def nonfinite_case(with_nan):
    """the lattice with non-finite database points and queries.  A NaN keeps a database off the f32 twin cloud (the grid routes of a handle) and
    a NaN query keeps a batch off them, so there are two forms: infinities only (every route), and NaN + infinities (the cloud routes and the
    exhaustive scan)."""
    def make():
        db, where = shuffled([lattice()], 100)
        db[int(where[1000])] = (np.inf, 1.0, 1.0)
        db[int(where[2000])] = (1.0, -np.inf, 1.0)
        odd = [[np.inf, 1.0, 1.0], [1.0, 1.0, -np.inf], [np.inf, -np.inf, np.inf]]
        if with_nan:
            db[int(where[3000])] = (np.nan, 1.0, 1.0)
            db[int(where[3001])] = (2.0, 2.0, np.nan)
            odd += [[np.nan, 1.0, 1.0], [1.0, np.nan, np.nan]]
        near = lattice()[[1000, 2000, 3000, 3001]]                       # where the odd points were
        q = np.concatenate([odd, near, near + 0.125, void_centres(40), lattice()[::45]])
        return case("nonfinite_nan" if with_nan else "nonfinite_inf", db, q, n_special=len(odd) + 8, n_odd=len(odd), odd_at=where[[1000, 2000, 3000, 3001]][: 4 if with_nan else 2])
    return cached(("nonfinite", with_nan), make)


# ------------------------------------------------------------------------------------------------------- the exhaustive scan's edges
def scan_case(n, m):
    """n random points on a 2^-6 lattice (ties are frequent) with five identical points at indices 510 ... 514 — across the edge of the first LDS
    tile, which is the edge of the first slice when the database is cut — and at the last five indices, across the last tile edge of n = 1 025,
    whose last slice holds ONE point.  The first query is that point."""
    def make():
        rng = np.random.default_rng(1000 * n + m)
        db = rng.integers(-256, 256, (n, 3)) / 64.0
        tie = np.array([0.515625, -1.25, 2.0])
        if n >= 515:
            db[510:515] = tie
        if n >= 1025:
            db[n - 5:] = tie
        q = rng.integers(-256, 256, (m, 3)) / 64.0
        q[0] = tie
        return case(f"scan{n}x{m}", db, q, n_special=1)
    return cached(("scan", n, m), make)


# ---------------------------------------------------------------------------------------------------------------- normals only
def sparse_case():
    """40 lone points, 40 pairs and 40 triangles, 10 apart: with radius 1 a point sees 1, 2 or exactly 3 neighbours (itself included)"""
    def make():
        tri = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.0, 0.5, 0.25]])
        parts, kind, normal = [], [], []
        for g in range(120):
            base = np.array([10.0 * (g % 11), 10.0 * (g // 11), 2.0 * (g % 3)])
            cnt = 1 + g // 40
            parts.append(base + tri[:cnt])
            kind += [cnt] * cnt
            normal += [np.cross(tri[1] - tri[0], tri[2] - tri[0])] * cnt
        db, where = shuffled(parts, 110)
        kinds = np.empty(db.shape[0], np.int64)
        kinds[where] = kind
        nrm = np.asarray(normal[-1], np.float64)
        return case("sparse", db, db[:1], kinds=kinds, normal=nrm / np.linalg.norm(nrm))
    return cached("sparse", make)


BIG_CASES = (lattice_case, lambda: coincident_case(4096), lambda: line_case("x"), lambda: line_case("y"), lambda: line_case("z"), lambda: line_case("diag"),
             plane_case, far_case, bar_case, shell_case, collapse_case, rule_case, lambda: nonfinite_case(False))
