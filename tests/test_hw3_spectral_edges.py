"""Homework3 spectral clustering at its edges (include/pcr.h, csrc/spectral.hip, DESIGN §8n "edges"): clouds of 2 ... 24 rows and k_neighbors = 2, conjugate
pairs at and across the n_eig cut, the positive statuses, every instantiation of the kNN kernel, the graph kernel around its 256-lane workgroup, the three
ways to a duplicate, the argument checks, and the context after a call that ended in a status or an error.  The numpy restatement and the residual
helper are the ones of tests/test_hw3_spectral_oracle.py and tests/test_hw3_spectral.py.

The reference of an eigenvalue is numpy.linalg.eigvals of the restatement's dense L, the bar 1e-9.  numpy itself is off by about sqrt(eps) at a defective
eigenvalue (seen: n = 21, k = 5, seed 2 has a double eigenvalue 1, numpy returns 1 - 1.07e-8 for L and 1 for L^T), so where numpy's eig(L) and eig(L^T)
differ by more than 1e-10 the same spectrum is taken from mpmath at 60 digits instead; the bar stays.

Spec_Cluster on a small cloud ends in status 0, except where the restatement's dense spectrum has a conjugate pair in columns 1-2 (3 of the 192
2-D cases): the contract's answer there is PCR_SPECTRAL_COMPLEX, and the test asks for exactly that.

Not produced: PCR_SPECTRAL_FEW_SEEDS needs two feature rows closer than 0.01, which with unit eigenvectors means tens of thousands of rows per cluster,
where the solver does not converge in seconds (the 100 000-row line)."""
import ctypes
import functools
import importlib
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "hands-on-point-cloud-processing_amd"
TOL = 1e-10
EIG_BAR = 1e-9
FIGURES = {"eig": 0.0, "res": 0.0}          # the largest |eigenvalue - dense| and re-evaluated residual seen (printed by the tests that add to them)


def load(name):
    spec = importlib.util.spec_from_file_location("t_edges_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def rs():
    return load("test_hw3_spectral_oracle")


@functools.lru_cache(maxsize=None)
def base():
    """tests/test_hw3_spectral.py: residuals, knn_rows, cloud40"""
    return load("test_hw3_spectral")


@pytest.fixture(scope="module")
def ctx():
    pcr = importlib.import_module(PKG)
    c = pcr.Context(0)
    yield c
    c.close()


def lib_pcr():
    return importlib.import_module(PKG)


def dense_spectrum(L):
    """the eigenvalues of L ascending by real part (numpy; mpmath at 60 digits where numpy disagrees with itself, see the module's docstring)"""
    w = np.linalg.eigvals(L)
    w = w[np.argsort(w.real, kind="stable")]
    wt = np.linalg.eigvals(np.ascontiguousarray(L.T))
    if np.max(np.abs(np.sort(w.real) - np.sort(wt.real))) > 1e-10:
        import mpmath
        with mpmath.workdps(60):
            e, _ = mpmath.eig(mpmath.matrix(L.tolist()))
            w = np.array([complex(z) for z in e])
        w.imag[np.abs(w.imag) < 1e-30] = 0.0                   # a real eigenvalue comes back with an imaginary part near 1e-60
        w = w[np.argsort(w.real, kind="stable")]
    return w


def small_cloud(n, seed, dim=2):
    return np.ascontiguousarray(np.random.default_rng(1000 * n + seed).normal(0, 1, (n, dim)))


def small_ks(n):
    return sorted({2, min(5, n), min(10, n)})


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def small_case(ctx, n, k, seed, dim=2):
    """one cloud of section A -> (list of what failed, figures)"""
    pcr = lib_pcr()
    hw3 = importlib.import_module(PKG + ".hw3")
    R, B = rs(), base()
    x = small_cloud(n, seed, dim)
    ne = min(n, 8)
    bad, fig = [], {}
    m = ctx.mat64(x)
    try:
        g = m.spectral_graph(k)
        if g is None:
            return ["graph: duplicate"], fig
        graph = g.read()
        try:
            ev, vec, info, rc = g.embed(ne, 0, TOL)
            ev2, vec2, info2, rc2 = g.embed(ne, 0, TOL)
        except pcr.PcrError as e:
            return [f"embed: {e}"], fig
        finally:
            g.free()
    finally:
        m.free()
    dense = dense_spectrum(R.rs_dense(R.rs_graph(x, k)))
    fig["status"], fig["steps"] = rc, info["steps"]
    fig["eig"] = float(np.max(np.abs(np.sort(ev) - dense.real[:ne])))
    if rc != 0 or rc2 != 0:
        bad.append(f"embed status {rc} / {rc2} (steps {info['steps']}, residual {info['residual']:.3e})")
    if not (np.all(np.isfinite(ev)) and np.all(np.isfinite(vec))):
        return bad + ["outputs not finite"], fig
    res = B.residuals(graph, ev, vec, info)
    fig["res"] = float(max(res)) if res else 0.0
    if not fig["res"] <= 10 * TOL:
        bad.append(f"re-evaluated residual {fig['res']:.3e}")
    if not np.all(np.diff(ev) >= 0):
        bad.append(f"eigenvalues not ascending: {ev}")
    if not fig["eig"] <= EIG_BAR:
        bad.append(f"|eigenvalue - dense| {fig['eig']:.3e}: {ev} against {dense[:ne]}")
    if not (np.array_equal(bits(ev), bits(ev2)) and np.array_equal(bits(vec), bits(vec2)) and info["steps"] == info2["steps"]
            and info["complex_mask"] == info2["complex_mask"] and np.array_equal(bits(info["eigenvalues_im"]), bits(info2["eigenvalues_im"]))):
        bad.append("the second run differs from the first")
    # Spec_Cluster: status 0, or PCR_SPECTRAL_COMPLEX exactly where the dense spectrum has a pair inside the two columns
    im = np.abs(dense.imag[:2])
    assert not np.any((im > 0) & (im <= 1e-6)), "the restatement cannot tell whether columns 0-1 hold a pair"
    want = pcr.PCR_SPECTRAL_COMPLEX if np.any(im > 1e-6) else 0
    sc = hw3.Spec_Cluster(k, ne, n_clusters=2, ctx=ctx)
    try:
        labels = sc.fit(x)
        if not (labels.shape == (n,) and set(labels.tolist()) <= {0, 1}):
            bad.append(f"Spec_Cluster labels {labels}")
    except pcr.PcrError as e:
        if sc.info_ is None:
            bad.append(f"Spec_Cluster: {e}")
    fig["fit"] = sc.status_
    if sc.info_ is not None and sc.status_ != want:
        bad.append(f"Spec_Cluster status {sc.status_}, expected {want}")
    return bad, fig


# ---- A. small clouds and k = 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", list(range(2, 25)))
def test_small_clouds_every_k(ctx, n):
    """n <= 32 rows with the default basis: the dense host path (solver_steps 0).  Status 0, residual <= 10 tol from the read-back CSR, eigenvalues
    ascending and within 1e-9 of the dense spectrum (as sorted values: k = 2 ties many eigenvalues at 0, 1 and 2), a second run equal bit for bit"""
    failed = []
    for k in small_ks(n):
        for seed in range(3):
            bad, fig = small_case(ctx, n, k, seed)
            print(f"n = {n} k = {k} seed {seed}: {fig}")
            FIGURES["eig"], FIGURES["res"] = max(FIGURES["eig"], fig.get("eig", 0.0)), max(FIGURES["res"], fig.get("res", 0.0))
            if fig.get("status") == 0:
                assert fig["steps"] == 0
            failed += [f"n = {n} k = {k} seed {seed}: {b}" for b in bad]
    print(f"largest so far: |eigenvalue - dense| {FIGURES['eig']:.3e}, re-evaluated residual {FIGURES['res']:.3e}")
    assert not failed, "\n".join(failed)


@pytest.mark.gpu
def test_small_cloud_in_three_dimensions(ctx):
    for k in small_ks(11):
        bad, fig = small_case(ctx, 11, k, 0, dim=3)
        print(f"n = 11 dim 3 k = {k}: {fig}")
        assert not bad, bad


# ---- B. conjugate pairs and statuses --------------------------------------------------------------------------------------------------------------
def cloud32():
    return np.ascontiguousarray(np.random.default_rng(10218).normal(0, 1, (32, 2)))


@functools.lru_cache(maxsize=None)
def spectrum32():
    x = cloud32()
    return dense_spectrum(rs().rs_dense(rs().rs_graph(x, 4)))


def test_cloud32_has_its_pair_in_columns_1_and_2():
    """the premise of section B, from the restatement alone: 0, then 0.05758 +- 0.01239 i, then real eigenvalues"""
    w = spectrum32()
    assert abs(w[0]) < 1e-12
    assert [j for j in range(6) if abs(w[j].imag) > 1e-3] == [1, 2] and np.all(w[3:6].imag == 0)
    assert abs(w[1].real - 0.05758) < 1e-5 and abs(abs(w[1].imag) - 0.01239) < 1e-5 and w[2] == np.conj(w[1])
    assert np.allclose(w[3:6].real, [0.0689, 0.1579, 0.2422], atol=1e-4)


def embed_calls32(ctx):
    """the four embed calls of section B -> {name: (ev, vec, info, rc, graph)}"""
    out = {}
    m = ctx.mat64(cloud32())
    try:
        g = m.spectral_graph(4)
        graph = g.read()
        for name, args in (("3,8", (3, 8, TOL)), ("2,8", (2, 8, TOL)), ("2,2", (2, 2, TOL, 1024))):
            out[name] = g.embed(*args) + (graph,)
        g.free()
    finally:
        m.free()
    m = ctx.mat64(rs().fixture()["moons"][0])
    try:
        g = m.spectral_graph(10)
        out["moons"] = g.embed(8, 13, TOL, 256) + (g.read(),)
        g.free()
    finally:
        m.free()
    return out


def check_embed_calls32(out):
    pcr = lib_pcr()
    B = base()
    w = spectrum32()
    pair = w[1] if w[1].imag > 0 else w[2]
    # the whole pair inside n_eig
    ev, vec, info, rc, graph = out["3,8"]
    assert rc == 0 and info["complex_mask"] == 0b110 and info["residual"] <= TOL
    assert info["eigenvalues_im"][0] == 0 and info["eigenvalues_im"][1] > 0 and info["eigenvalues_im"][2] == -info["eigenvalues_im"][1]
    res = B.residuals(graph, ev, vec, info)
    eig_err = max(np.max(np.abs(ev - w.real[:3])), abs(info["eigenvalues_im"][1] - pair.imag))
    assert max(res) <= 10 * TOL and eig_err <= EIG_BAR and ev[1] == ev[2]
    # the pair cut by n_eig: completed inside, its first member handed out
    ev2, vec2, info2, rc2, _ = out["2,8"]
    assert rc2 == 0 and info2["complex_mask"] == 0b10 and info2["eigenvalues_im"][1] > 0
    assert abs(ev2[1] - pair.real) <= EIG_BAR and abs(ev2[0]) <= EIG_BAR
    v = vec2[:, 1] + 1j * vec[:, 2]                            # with the partner of the (3, 8) call
    lam = ev2[1] + 1j * info2["eigenvalues_im"][1]
    n, k = 32, 4
    C, V = graph[1].reshape(n, k), graph[2].reshape(n, k)
    cut_res = float(np.linalg.norm((V * v[C]).sum(axis=1) - lam * v))
    assert abs(np.linalg.norm(v) - 1) < 1e-12 and cut_res <= 10 * TOL
    assert max(B.residuals(graph, ev2, vec2, info2)) <= 10 * TOL      # column 0 (the helper skips a cut pair)
    # no room to complete the pair: the call cannot converge
    ev3, vec3, info3, rc3, _ = out["2,2"]
    assert rc3 == pcr.PCR_SPECTRAL_NOT_CONVERGED and info3["steps"] == 1024 and info3["residual"] > TOL
    assert np.all(np.isfinite(ev3)) and np.all(np.isfinite(vec3)) and np.isfinite(info3["residual"])
    # max_iter ends first on a data set that needs 9 984 steps
    ev4, vec4, info4, rc4, _ = out["moons"]
    assert rc4 == pcr.PCR_SPECTRAL_NOT_CONVERGED and info4["steps"] == 256 and info4["residual"] > TOL
    assert np.all(np.isfinite(ev4)) and np.all(np.isfinite(vec4)) and np.isfinite(info4["residual"])
    return float(eig_err), float(max(max(res), cut_res))


@pytest.mark.gpu
def test_pairs_at_the_cut_and_not_converged_on_both_launch_paths(ctx):
    one = embed_calls32(ctx)
    eig_err, res = check_embed_calls32(one)
    assert all(o[2]["one_workgroup"] for o in one.values())
    ctx.tune("spectral_path", 2)
    try:
        many = embed_calls32(ctx)
    finally:
        ctx.tune("spectral_path", 0)
    eig_err2, res2 = check_embed_calls32(many)
    assert not any(o[2]["one_workgroup"] for o in many.values())
    same_bits = True
    for name in one:
        a, b = one[name], many[name]
        assert a[3] == b[3] and a[2]["complex_mask"] == b[2]["complex_mask"] and a[2]["steps"] == b[2]["steps"], name
        diff = float(np.max(np.abs(a[0] - b[0])))
        same = np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))
        same_bits = same_bits and same
        print(f"embed({name}): status {a[3]} mask {a[2]['complex_mask']:#b} steps {a[2]['steps']} residual {a[2]['residual']:.3e} | "
              f"many-launch path: |eigenvalue difference| {diff:.3e}, bits {'equal' if same else 'differ'}")
        assert diff <= EIG_BAR, name
    print(f"section B: largest |eigenvalue - dense| {max(eig_err, eig_err2):.3e}, re-evaluated residual {max(res, res2):.3e}, both paths bit-equal: {same_bits}")


@pytest.mark.gpu
def test_complex_pair_inside_k_is_a_status(ctx):
    pcr = lib_pcr()
    hw3 = importlib.import_module(PKG + ".hw3")
    x = cloud32()
    m = ctx.mat64(x)
    try:
        labels, feat, info, rc = m.spectral_cluster(4, 6, n_clusters=2)
        assert rc == pcr.PCR_SPECTRAL_COMPLEX and info["K"] == 2 and feat is None
        assert info["complex_mask"] & 0b11 == 0b10 and info["steps"] == 0          # 32 rows, default basis: the dense path
        assert np.max(np.abs(info["eigenvalues"] - spectrum32().real[:6])) <= EIG_BAR
        labels, feat, info, rc = m.spectral_cluster(4, 6, n_clusters=1)
        assert rc == 0 and info["K"] == 1 and np.all(labels == 0) and feat.shape == (32, 1)
    finally:
        m.free()
    sc = hw3.Spec_Cluster(4, 6, n_clusters=2, ctx=ctx)
    with pytest.raises(pcr.PcrError):
        sc.fit(x)
    assert sc.status_ == pcr.PCR_SPECTRAL_COMPLEX and sc.K_clusters == 2
    context_still_works(ctx)


# ---- C. kNN: every instantiation ------------------------------------------------------------------------------------------------------------------
def knn_equals(ctx, x, k):
    m = ctx.mat64(x)
    try:
        idx, d2 = m.knn(k)
    finally:
        m.free()
    ridx, rd2 = rs().rs_knn(x, k)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(bits(d2), bits(rd2))


@pytest.mark.gpu
@pytest.mark.parametrize("dim", list(range(1, 9)))
@pytest.mark.parametrize("k", [1, 2, 16, 17, 32])
def test_knn_every_dim_and_both_lists(ctx, k, dim):
    """130 rows: two full 64-lane tiles and a 2-row tail"""
    knn_equals(ctx, np.random.default_rng(130 * dim + k).normal(0, 3, (130, dim)), k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [17, 32])
def test_knn_k_equals_n(ctx, n):
    knn_equals(ctx, np.random.default_rng(n).normal(0, 3, (n, 2)), n)


@pytest.mark.gpu
def test_knn_refuses_k_above_n_and_above_32(ctx):
    pcr = lib_pcr()
    for n, k in ((17, 18), (40, 33)):
        m = ctx.mat64(np.random.default_rng(n).normal(0, 3, (n, 2)))
        try:
            with pytest.raises(pcr.PcrError, match="bad argument"):
                m.knn(k)
        finally:
            m.free()
    knn_equals(ctx, np.random.default_rng(1).normal(0, 3, (40, 2)), 32)


@pytest.mark.gpu
def test_knn_lattice_ties_in_five_dimensions(ctx):
    knn_equals(ctx, np.random.default_rng(5).integers(0, 5, (200, 5)).astype(np.float64), 32)


@pytest.mark.gpu
def test_knn_first_size_of_the_wide_launch(ctx):
    """32 768 rows: the first size on 256-lane workgroups, here with the 32-slot list and the largest tile (dim 8)"""
    n = 32768
    x = np.random.default_rng(32768).normal(0, 10, (n, 8))
    m = ctx.mat64(x)
    try:
        idx, d2 = m.knn(17)
    finally:
        m.free()
    rows = np.concatenate([np.arange(64), np.arange(16352, 16416), np.arange(n - 64, n)])
    ridx, rd2 = base().knn_rows(x, rows, 17)
    assert np.array_equal(idx[rows], ridx) and np.array_equal(bits(d2[rows]), bits(rd2))


# ---- D. graph edges ---------------------------------------------------------------------------------------------------------------------------------
def graph_equals(ctx, x, k):
    n = x.shape[0]
    m = ctx.mat64(x)
    try:
        g = m.spectral_graph(k)
        assert g is not None
        row_ptr, col, val = g.read()
        g.free()
    finally:
        m.free()
    rp, rc, rv = rs().rs_graph(x, k)
    assert np.array_equal(row_ptr, rp) and np.array_equal(col, rc)
    assert np.array_equal(bits(val), bits(rv))
    C, V = col.reshape(n, k), val.reshape(n, k)
    assert np.all(np.diff(C, axis=1) > 0)
    assert np.all(V[C == np.arange(n)[:, None]] == 1.0) and np.all((C == np.arange(n)[:, None]).sum(axis=1) == 1)
    assert np.all(np.isfinite(V)) and np.all(np.abs(V.sum(axis=1)) <= n * np.finfo(np.float64).eps)


@pytest.mark.gpu
@pytest.mark.parametrize("n,k,dim", [(255, 2, 3), (256, 32, 1), (257, 10, 8), (513, 5, 5), (12, 12, 2)])
def test_graph_around_the_workgroup_and_at_both_ends_of_k(ctx, n, k, dim):
    graph_equals(ctx, np.random.default_rng(1000 * n + k).normal(0, 2, (n, dim)), k)


def duplicate_clouds():
    rng = np.random.default_rng(600)
    a = rng.normal(0, 1, (600, 2))
    a[500] = a[300]                                            # outside the first workgroup
    b = rng.normal(0, 1, (50, 2))
    b[20] = b[10]
    b[30] = b[10]                                              # k = 2: row 30 finds rows 10 and 20 at distance 0 before itself
    c = rng.normal(0, 1, (50, 2)) + [3.0, 0.0]
    c[0] = [0.0, 0.0]
    c[1] = [1e-170, 0.0]                                       # distinct, but d2 = 1e-340 underflows to 0
    return [("rows 300 and 500 of 600", a, 10), ("three copies, k = 2", b, 2), ("1e-170 apart", c, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1, 2])
def test_graph_every_way_to_a_duplicate(ctx, which):
    pcr = lib_pcr()
    name, x, k = duplicate_clouds()[which]
    assert rs().rs_graph(x, k) is None, name
    m = ctx.mat64(x)
    try:
        h = ctypes.c_void_p()
        assert pcr.lib().pcr_spectral_graph_f64(ctx.h, m.h, k, ctypes.byref(h)) == pcr.PCR_SPECTRAL_DUPLICATE and not h.value, name
        assert m.spectral_graph(k) is None
    finally:
        m.free()
    graph_equals(ctx, np.random.default_rng(which).normal(0, 1, (x.shape[0], 2)), k)      # the flag word is reset
    context_still_works(ctx)


@pytest.mark.gpu
def test_graph_of_two_points_1e150_apart_is_no_duplicate(ctx):
    x = np.random.default_rng(150).normal(0, 1, (50, 2)) + [3.0, 0.0]
    x[0] = [0.0, 0.0]
    x[1] = [1e-150, 0.0]                                       # d2 = 1e-300, w = 1e150
    graph_equals(ctx, x, 5)


# ---- E. arguments and context state -----------------------------------------------------------------------------------------------------------------
def context_still_works(ctx):
    """Spec_Cluster on the 40-point cloud and K_Means on 100 rows, on the context that has just returned a status or an error"""
    hw3 = importlib.import_module(PKG + ".hw3")
    sc = hw3.Spec_Cluster(6, 8, n_clusters=2, ctx=ctx)
    labels = sc.fit(base().cloud40())
    assert sc.status_ == 0 and rs().same_partition(labels.astype(np.int64), np.repeat([0, 1], 20))
    assert np.all(np.abs(sc.eigenvalues_[:2]) < 1e-9) and sc.eigenvalues_[2] > 1e-3
    rng = np.random.default_rng(100)
    x = np.ascontiguousarray(np.concatenate([rng.normal(0, 1, (50, 3)), rng.normal(0, 1, (50, 3)) + [20.0, 0.0, 0.0]]))
    km = hw3.K_Means(2, init_idx=[0, 50], ctx=ctx)
    km.fit(x)
    assert km.status_ == 0 and km.center_ is not None
    assert np.max(np.abs(km.center_ - np.array([x[:50].mean(axis=0), x[50:].mean(axis=0)]))) < 1e-12
    assert np.array_equal(km.predict(x), np.repeat([0, 1], 50))


@pytest.mark.gpu
def test_embed_argument_errors_leave_the_context_working(ctx):
    pcr = lib_pcr()
    m = ctx.mat64(small_cloud(10, 0))
    try:
        g = m.spectral_graph(4)
        for args in ((5, 3, TOL), (8, 17, TOL), (2, 12, TOL), (2, 6, float("nan"))):      # n_eig > n_basis, n_basis = 17, n_basis > n, tol = NaN
            with pytest.raises(pcr.PcrError, match="bad argument"):
                g.embed(*args)
            context_still_works(ctx)
        ev, vec, info, rc = g.embed(2, 6, TOL)
        assert rc == 0 and info["steps"] > 0                  # the graph is still usable; a given n_basis asks for the iteration
        g.free()
    finally:
        m.free()


@pytest.mark.gpu
def test_cluster_argument_errors_leave_the_context_working(ctx):
    pcr = lib_pcr()
    n = 20
    m = ctx.mat64(small_cloud(n, 0))
    m40 = ctx.mat64(np.random.default_rng(41).normal(0, 1, (40, 2)))
    try:
        for mat, args in ((m, (1, 8, 2)), (m40, (33, 8, 2)), (m, (n + 1, 8, 2)), (m, (6, 8, 9)), (m, (6, 3, 4))):
            with pytest.raises(pcr.PcrError, match="bad argument"):
                mat.spectral_cluster(*args)
            context_still_works(ctx)
        for mat, k in ((m, 1), (m40, 33), (m, n + 1)):
            with pytest.raises(pcr.PcrError, match="bad argument"):
                mat.spectral_graph(k)
    finally:
        m.free()
        m40.free()


@pytest.mark.gpu
def test_context_works_after_not_converged(ctx):
    pcr = lib_pcr()
    m = ctx.mat64(rs().fixture()["moons"][0])
    try:
        g = m.spectral_graph(10)
        assert g.embed(8, 13, TOL, 256)[3] == pcr.PCR_SPECTRAL_NOT_CONVERGED
        g.free()
    finally:
        m.free()
    context_still_works(ctx)


@pytest.mark.gpu
def test_embed_defaults_equal_the_explicit_call(ctx):
    m = ctx.mat64(base().cloud40())
    try:
        g = m.spectral_graph(6)
        ev, vec, info, rc = g.embed(0, 0, 0.0, 0)
        ev2, vec2, info2, rc2 = g.embed(8, 13, 1e-10)
        g.free()
    finally:
        m.free()
    assert rc == 0 and rc2 == 0 and ev.shape == (8,) and vec.shape == (40, 8)
    assert info["n_eig"] == 8 and info["n_basis"] == 13 and info["steps"] == info2["steps"] > 0
    assert np.array_equal(bits(ev), bits(ev2)) and np.array_equal(bits(vec), bits(vec2))


@pytest.mark.gpu
def test_cluster_info_is_zero_when_the_embedding_refuses_its_arguments(ctx):
    """n = 5, n_eig = 8: the graph is built, the embedding returns PCR_ERR_ARG before filling anything; the caller's struct then holds zeros"""
    pcr = lib_pcr()
    info = pcr.SpectralInfo()
    ctypes.memset(ctypes.byref(info), 0xFF, ctypes.sizeof(info))
    labels = np.full(5, -7, np.int32)
    m = ctx.mat64(small_cloud(5, 0))
    try:
        rc = pcr.lib().pcr_spectral_cluster_f64(ctx.h, m.h, 3, 8, 0, labels.ctypes.data, None, ctypes.byref(info))
    finally:
        m.free()
    assert rc == -1                                            # PCR_ERR_ARG
    assert bytes(info) == bytes(ctypes.sizeof(info))
    assert np.all(labels == -7)
    context_still_works(ctx)
