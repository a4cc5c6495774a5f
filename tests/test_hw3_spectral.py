"""Homework3 spectral clustering on the GPU (include/pcr.h, csrc/spectral.hip): the exhaustive kNN, the random-walk Laplacian of the kNN
graph, the block eigen-solver on both of its launch paths, and Spec_Cluster end to end against the labels the reference's binary recorded
(tests/golden/hw3_spectral_ref.npz) — from Python, and from the drop-in header through examples/hw3_spectral_driver.cpp.  The numpy restatement is the
one of tests/test_hw3_spectral_oracle.py."""
import functools
import importlib
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "hands-on-point-cloud-processing_amd"
INC = os.path.join(ROOT, "include", "pcr")
LIBDIR = os.path.join(ROOT, PKG)
LINK = ["-L" + LIBDIR, "-lpcr_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
TOL = 1e-10


@functools.lru_cache(maxsize=None)
def rs():
    spec = importlib.util.spec_from_file_location("t_hw3_spectral_restatement", os.path.join(ROOT, "tests", "test_hw3_spectral_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ctx():
    pcr = importlib.import_module(PKG)
    c = pcr.Context(0)
    yield c
    c.close()


def knn_rows(x, rows, k):
    """the restatement's kNN for some rows only"""
    d2 = np.zeros((len(rows), x.shape[0]))
    for d in range(x.shape[1]):
        df = x[rows, None, d] - x[None, :, d]
        d2 = d2 + df * df
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int32), np.take_along_axis(d2, idx, axis=1)


def two_grids(n):
    """two jittered square lattices 1 000 apart: with 5 neighbours every point links to its lattice neighbours, so the kNN graph has exactly two
    components"""
    rng = np.random.default_rng(n)
    out = []
    for b, m in enumerate((n // 2, n - n // 2)):
        w = int(np.ceil(np.sqrt(m)))
        p = np.stack([np.arange(m) % w, np.arange(m) // w], axis=1).astype(np.float64)
        out.append(p + rng.uniform(-0.05, 0.05, p.shape) + [1000.0 * b, 0.0])
    return np.ascontiguousarray(np.concatenate(out)), n // 2


def cloud40():
    rng = np.random.default_rng(40)
    return np.ascontiguousarray(np.concatenate([rng.normal(0, 1, (20, 2)), rng.normal(0, 1, (20, 2)) + [30.0, 0.0]]))


def residuals(graph, ev, vec, info):
    """|L v - lambda v| of every unit column (a conjugate pair: of its complex vector, reported on both columns)"""
    row_ptr, col, val = graph
    n = row_ptr.shape[0] - 1
    k = col.shape[0] // n
    C, V = col.reshape(n, k), val.reshape(n, k)
    out = []
    j = 0
    while j < vec.shape[1]:
        if info["complex_mask"] >> j & 1 and j + 1 < vec.shape[1]:
            v = vec[:, j] + 1j * vec[:, j + 1]
            lam = ev[j] + 1j * info["eigenvalues_im"][j]
            w = 2
        elif info["complex_mask"] >> j & 1:
            j += 1                                           # the pair is cut by n_eig: its second column was not handed out
            continue
        else:
            v, lam, w = vec[:, j], ev[j], 1
        assert abs(np.linalg.norm(v) - 1) < 1e-12
        r = float(np.linalg.norm((V * v[C]).sum(axis=1) - lam * v))
        out += [r] * w
        j += w
    return out


# ---- kNN --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [1, 2, 8])
@pytest.mark.parametrize("n", [1, 10, 11, 63, 64, 65, 257, 1500])
def test_knn_equals_brute_force(ctx, n, dim):
    k = min(10, n)
    x = np.random.default_rng(100 * n + dim).normal(0, 3, (n, dim))
    m = ctx.mat64(x)
    try:
        idx, d2 = m.knn(k)
    finally:
        m.free()
    ridx, rd2 = rs().rs_knn(x, k)
    assert np.array_equal(idx, ridx)
    assert np.array_equal(d2.view(np.uint64), rd2.view(np.uint64))
    assert np.array_equal(idx[:, 0], np.arange(n))           # the row itself, at distance 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 16, 17, 32])
def test_knn_lattice_full_of_ties_and_both_list_sizes(ctx, k):
    """an integer lattice with repeated points: whole shells at one distance, ordered by index; k = 16 | 17 is where the register list doubles"""
    x = np.random.default_rng(7).integers(0, 7, (300, 2)).astype(np.float64)
    m = ctx.mat64(x)
    try:
        idx, d2 = m.knn(k)
    finally:
        m.free()
    ridx, rd2 = rs().rs_knn(x, k)
    assert np.array_equal(idx, ridx) and np.array_equal(d2.view(np.uint64), rd2.view(np.uint64))


@pytest.mark.gpu
def test_knn_wide_workgroups(ctx):
    """from 32 768 rows the launch takes 256-lane workgroups and tiles; checked on 192 rows, the last ones among them"""
    n = 33001
    x = np.random.default_rng(33).normal(0, 10, (n, 3))
    m = ctx.mat64(x)
    try:
        idx, d2 = m.knn(10)
    finally:
        m.free()
    rows = np.concatenate([np.arange(64), np.arange(16350, 16414), np.arange(n - 64, n)])
    ridx, rd2 = knn_rows(x, rows, 10)
    assert np.array_equal(idx[rows], ridx) and np.array_equal(d2[rows].view(np.uint64), rd2.view(np.uint64))


# ---- graph ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cloud40", "moons"])
def test_graph_equals_the_restatement(ctx, which):
    x = cloud40() if which == "cloud40" else rs().fixture()["moons"][0]
    k = 6 if which == "cloud40" else 10
    m = ctx.mat64(x)
    try:
        g = m.spectral_graph(k)
        row_ptr, col, val = g.read()
        g.free()
    finally:
        m.free()
    rp, rc, rv = rs().rs_graph(x, k)
    assert np.array_equal(row_ptr, rp) and np.array_equal(col, rc)
    assert np.array_equal(val.view(np.uint64), rv.view(np.uint64))
    n = x.shape[0]
    C = col.reshape(n, k)
    assert np.all(np.diff(C, axis=1) > 0)                     # ascending columns
    assert np.all(np.abs(val.reshape(n, k).sum(axis=1)) <= n * np.finfo(np.float64).eps)


@pytest.mark.gpu
def test_graph_reports_a_duplicate_point(ctx):
    pcr = importlib.import_module(PKG)
    x = cloud40()
    x[17] = x[3]
    m = ctx.mat64(x)
    try:
        assert m.spectral_graph(6) is None
        h = pcr.C.c_void_p()
        assert pcr.lib().pcr_spectral_graph_f64(ctx.h, m.h, 6, pcr.C.byref(h)) == pcr.PCR_SPECTRAL_DUPLICATE and not h.value
    finally:
        m.free()


# ---- embedding --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_eigs40():
    x = cloud40()
    L = rs().rs_dense(rs().rs_graph(x, 6))
    return np.sort(np.linalg.eig(L)[0].real)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cloud40", "aniso", "blobs", "circle", "moons", "varied"])
def test_embedding_residuals_and_k(ctx, name):
    pcr = importlib.import_module(PKG)
    R = rs()
    x = cloud40() if name == "cloud40" else R.fixture()[name][0]
    k = 6 if name == "cloud40" else 10
    m = ctx.mat64(x)
    try:
        g = m.spectral_graph(k)
        graph = g.read()
        ev, vec, info, rc = g.embed(8, 13, TOL)
        g.free()
    finally:
        m.free()
    assert rc == 0 and info["residual"] <= TOL and info["one_workgroup"]
    res = residuals(graph, ev, vec, info)
    dense = dense_eigs40()[:8] if name == "cloud40" else R.rs_spectrum(name)[1].real[:8]
    print(f"{name}: steps {info['steps']}  solver residual {info['residual']:.3e}  re-evaluated max {max(res):.3e}  "
          f"max |eigenvalue - numpy dense| {np.max(np.abs(ev - dense)):.3e}  complex_mask {info['complex_mask']:#x}")
    assert max(res) <= 10 * TOL
    assert np.all(np.diff(ev) >= 0)
    for j in range(8):
        if not info["complex_mask"] >> j & 1:
            assert vec[np.argmax(np.abs(vec[:, j])), j] > 0
    if name in R.PINNED_K:
        assert pcr.spectral_select_k(ev) == R.rs_select_k(dense) == R.PINNED_K[name]
    if name == "circle":
        assert info["complex_mask"] != 0                      # the pair at 1.336e-4 +- 4.6e-5 i


@pytest.mark.gpu
@pytest.mark.parametrize("n", [14, 64, 65, 4096, 4097])
def test_embedding_both_launch_paths_find_the_null_space(ctx, n):
    """up to 4 096 rows one persistent workgroup iterates, beyond that one launch per step: both find the two components"""
    x, half = two_grids(n)
    m = ctx.mat64(x)
    try:
        g = m.spectral_graph(5)
        graph = g.read()
        ev, vec, info, rc = g.embed(2, 6, TOL)
        ev2, vec2, info2, rc2 = g.embed(2, 6, TOL)
        g.free()
    finally:
        m.free()
    print(f"n = {n}: steps {info['steps']} residual {info['residual']:.3e} eigenvalues {ev} one_workgroup {info['one_workgroup']}")
    assert rc == 0 and rc2 == 0
    assert info["one_workgroup"] == (n <= 4096)
    assert np.all(np.abs(ev) < 1e-9)
    assert max(residuals(graph, ev, vec, info)) <= 10 * TOL
    for part in (vec[:half], vec[half:]):                     # rows take two values
        assert np.max(np.abs(part - part[0])) <= 1e-6
    assert np.max(np.abs(vec[0] - vec[-1])) > 1e-3
    # a run repeats bit for bit
    assert np.array_equal(ev.view(np.uint64), ev2.view(np.uint64)) and np.array_equal(vec.view(np.uint64), vec2.view(np.uint64))
    assert info["steps"] == info2["steps"]


@pytest.mark.gpu
def test_embedding_many_launch_path_agrees_with_the_one_workgroup_path(ctx):
    """the many-launch path forced at 1 500 rows (tune spectral_path = 2) reaches the same eigenpairs as the persistent workgroup"""
    x = rs().fixture()["moons"][0]
    m = ctx.mat64(x)
    try:
        g = m.spectral_graph(10)
        graph = g.read()
        ev1, vec1, info1, rc1 = g.embed(8, 13, TOL)
        ctx.tune("spectral_path", 2)
        try:
            ev2, vec2, info2, rc2 = g.embed(8, 13, TOL)
        finally:
            ctx.tune("spectral_path", 0)
        g.free()
    finally:
        m.free()
    assert rc1 == 0 and rc2 == 0 and info1["one_workgroup"] and not info2["one_workgroup"]
    assert max(residuals(graph, ev2, vec2, info2)) <= 10 * TOL
    assert np.max(np.abs(ev1 - ev2)) <= 1e-9


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["aniso", "circle", "moons", "varied"])
def test_spec_cluster_equals_the_recorded_labels(ctx, name):
    hw3 = importlib.import_module(PKG + ".hw3")
    R = rs()
    x, ref = R.fixture()[name]
    sc = hw3.Spec_Cluster(10, 8, ctx=ctx)
    labels = sc.fit(x)
    print(f"{name}: K {sc.K_clusters} eigenvalues {sc.eigenvalues_} steps {sc.info_['steps']} kmeans passes {sc.info_['kmeans_iters']}")
    assert sc.K_clusters == R.PINNED_K[name]
    assert sc.features_.shape == (1500, sc.K_clusters) and sc.eigenvalues_.shape == (8,)
    assert R.same_partition(labels.astype(np.int64), ref)


@pytest.mark.gpu
def test_spec_cluster_blobs_refines_the_recorded_labels(ctx):
    hw3 = importlib.import_module(PKG + ".hw3")
    R = rs()
    x, ref = R.fixture()["blobs"]
    sc = hw3.Spec_Cluster(10, 8, n_clusters=3, ctx=ctx)
    labels = sc.fit(x).astype(np.int64)
    assert sc.K_clusters == 3 and sorted(np.bincount(labels).tolist()) == [500, 500, 500]
    assert R.refines(labels, ref)


def build_driver(tmp_path):
    if not os.path.exists(os.path.join(LIBDIR, "libpcr_hip.so")):
        pytest.fail("libpcr_hip.so not built")
    exe = tmp_path / "hw3_spectral_driver"
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-I" + INC, os.path.join(ROOT, "examples", "hw3_spectral_driver.cpp"), "-o", str(exe)] + LINK,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_dropin_header_and_driver_compile(tmp_path):
    build_driver(tmp_path)


@pytest.mark.gpu
def test_driver_writes_the_recorded_labels(tmp_path):
    """examples/hw3_spectral_driver.cpp = Homework3/hw3/main.cpp: ../data/<set>.txt -> ../result/predict_<set>.txt through the drop-in Spec_Cluster;
    the same checks as from Python"""
    R = rs()
    exe = build_driver(tmp_path)
    for d in ("build", "data", "result"):
        (tmp_path / d).mkdir()
    for name in R.SETS:
        np.savetxt(tmp_path / "data" / f"{name}.txt", R.fixture()[name][0], delimiter=",", fmt="%.17g")
    r = subprocess.run([str(exe), "blobs=3"], cwd=tmp_path / "build", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for name in R.SETS:
        labels = np.loadtxt(tmp_path / "result" / f"predict_{name}.txt", dtype=np.int64)
        ref = R.fixture()[name][1]
        assert labels.shape == (1500,)
        if name == "blobs":                                   # K fixed to 3 (the rule's choice between three equal zero eigenvalues is noise)
            assert R.refines(labels, ref) and sorted(np.bincount(labels).tolist()) == [500, 500, 500]
        else:
            assert R.same_partition(labels, ref), name
