"""Homework3 on the GPU: K-Means, its k-means++-style seeding and Gaussian-mixture EM (include/pcr.h, csrc/mixture.hip).

The numpy RESTATEMENT of the contracts lives in this file (rs_*).  tests/golden/gen_golden_hw3.py ran the reference's own classes
(Homework3/hw3/sript/KMeans.py, GMM.py with the working `posterior` of Homework3/nano_vs_my/sript/GMM.py) and stored what they returned
in tests/golden/hw3_clustering_ref.npz, together with the largest difference between this restatement and the reference per quantity
(em_step_err, fit_err): those recorded values, not anything the GPU produced, set the EM bars below.
  CPU tests: the restatement against the fixture, the ABI list, the hw3 module's surface.
  GPU tests (-m gpu): the library against the restatement and against the fixture.
"""
import importlib
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "hands-on-point-cloud-processing_amd"
GOLD = os.path.join(ROOT, "tests", "golden", "hw3_clustering_ref.npz")
SETS = ("aniso", "blobs", "circle", "moons", "varied")
NEW_SYMBOLS = ("pcr_mat64_create", "pcr_mat64_destroy", "pcr_mat64_info", "pcr_kmeans_step_f64", "pcr_kmeans_fit_f64", "pcr_kmeans_predict_f64",
               "pcr_kmeanspp_init_f64", "pcr_gmm_em_step_f64", "pcr_gmm_fit_f64", "pcr_gmm_predict_f64")
U = 2.0 ** -53


# ---- the restatement ----------------------------------------------------------------------------------------------------------
def rs_sqdist(x, c):
    """s[i, j] = sum_d (x_d - c_d)^2, ascending d, starting from (x_0 - c_0)^2, every operation rounded"""
    s = (x[:, None, 0] - c[None, :, 0]) ** 2
    for d in range(1, x.shape[1]):
        s = s + (x[:, None, d] - c[None, :, d]) ** 2
    return s


def rs_assign(x, c):
    s = rs_sqdist(x, c)
    return np.argmin(s, axis=1).astype(np.int32), s          # argmin: the first minimum = the lowest centre index


def rs_exact_centres(x, labels, k):
    """fsum(members) / m per cluster and coordinate (NaN for an empty cluster), and the counts"""
    out = np.full((k, x.shape[1]), np.nan)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    for j in range(k):
        mem = x[labels == j]
        if mem.shape[0]:
            out[j] = [math.fsum(mem[:, d]) / mem.shape[0] for d in range(x.shape[1])]
    return out, counts


def rs_kmeans_fit(x, c0, tol, max_iter, mode="py"):
    """-> (centres at the start of every pass + the final ones, passes, converged)"""
    c, hist, count, conv = np.array(c0, np.float64), [], 0, False
    while True:
        if mode == "py" and not (not conv and count <= max_iter):
            break
        count += 1
        hist.append(c.copy())
        labels, _ = rs_assign(x, c)
        new, counts = rs_exact_centres(x, labels, c.shape[0])
        if (counts == 0).any():
            c = new
            break
        if mode == "py":
            if np.all((new - c) < tol):
                conv = True
            c = new
        else:
            ok = bool(np.all(np.fabs(new - c) < tol))
            c = new
            if ok and count < max_iter:
                conv = True
                break
            if count > max_iter:
                break
    hist.append(c.copy())
    return hist, count, conv


def rs_near_tie(s, factor=32.0):
    """points whose two smallest s differ by <= factor 2^-53 (s_a + s_b)"""
    if s.shape[1] < 2:
        return np.zeros(s.shape[0], bool)
    two = np.sort(s, axis=1)[:, :2]
    return (two[:, 1] - two[:, 0]) <= factor * U * (two[:, 0] + two[:, 1])


def rs_seed(x, k, factor, u):
    """init_choice from caller's uniforms -> (picks, the distribution of the last pick)"""
    n = x.shape[0]
    picks = [min(int(math.floor(u[0] * n)), n - 1)]
    d, p = None, None
    for j in range(1, k):
        dj = np.sqrt(rs_sqdist(x, x[picks[-1]][None, :])[:, 0])
        d = dj if d is None else np.minimum(d, dj)
        mean = math.fsum(d) / n
        w = np.where(d < factor * mean, 0.0, np.exp(d))
        p = w / np.sum(w)
        cdf = np.cumsum(w)
        picks.append(int(np.searchsorted(cdf / cdf[-1], u[j], side="right")))
    return np.array(picks, np.int32), p


def rs_logpost(x, mean, cov, pi):
    """log pi_k N(x; mu_k, Sigma_k), n x k, through the Cholesky factor"""
    n, dim = x.shape
    out = np.empty((n, mean.shape[0]))
    for j in range(mean.shape[0]):
        L = np.linalg.cholesky(cov[j])
        y = np.linalg.solve(L, (x - mean[j]).T)
        out[:, j] = math.log(pi[j]) - 0.5 * (dim * math.log(2.0 * math.pi) + 2.0 * np.sum(np.log(np.diag(L)))) - 0.5 * np.sum(y * y, axis=0)
    return out


def rs_em_step(x, mean, cov, pi):
    lp = rs_logpost(x, np.asarray(mean), np.asarray(cov), np.asarray(pi))
    m = lp.max(axis=1, keepdims=True)
    ev = np.exp(lp - m)
    post = ev / ev.sum(axis=1, keepdims=True)
    ld = np.longdouble
    nk = np.sum(post.astype(ld), axis=0)
    pi_new = (nk / x.shape[0]).astype(np.float64)
    mean_new = np.empty_like(np.asarray(mean, np.float64))
    cov_new = np.empty_like(np.asarray(cov, np.float64))
    for j in range(mean_new.shape[0]):
        mean_new[j] = (np.sum((post[:, j, None] * x).astype(ld), axis=0) / nk[j]).astype(np.float64)
        df = x - mean_new[j]
        cov_new[j] = (np.sum(((post[:, j, None] * df)[:, :, None] * df[:, None, :]).astype(ld), axis=0) / nk[j]).astype(np.float64)
    return mean_new, cov_new, pi_new, post


def rs_gmm_fit(x, init_mean, amplitude, eps, max_iter):
    """GMM.fit without the reset rule firing (asserted) -> (mean, cov, pi, count, the three max-abs differences of every pass)"""
    k, dim = init_mean.shape
    mean, cov, pi = np.array(init_mean, np.float64), np.array([amplitude * np.identity(dim)] * k), np.full(k, 1.0 / k)
    count, margins = 0, []
    while True:
        count += 1
        m2, c2, p2, _ = rs_em_step(x, mean, cov, pi)
        assert all(np.linalg.norm(c2[j]) >= 0.01 for j in range(k)), "the reset rule fired"
        dm = [float(np.max(np.fabs(m2 - mean))), float(np.max(np.fabs(c2 - cov))), float(np.max(np.fabs(p2 - pi)))]
        margins.append(dm)
        mean, cov, pi = m2, c2, p2
        if max(dm) < eps or count == max_iter:
            return mean, cov, pi, count, np.array(margins)


def gold():
    return np.load(GOLD)


def widened_scan(n=100000):
    """a real scan widened to n x 3 f64: the KITTI excerpt of the fixtures, tiled with exact f32 offsets"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "kat_kitti_q5.npz"))
    key = [k for k in z.files if z[k].ndim == 2 and z[k].shape[1] >= 3][0]
    pts = z[key][:, :3].astype(np.float64)
    reps = -(-n // pts.shape[0])
    out = np.concatenate([pts + np.array([37.0 * r, -11.0 * r, 0.25 * r]) for r in range(reps)])[:n]
    return np.ascontiguousarray(out)


def spread_centres(x, k):
    return x[(np.arange(k) * (x.shape[0] // k) + 17) % x.shape[0]].copy()


# ---- CPU tests -----------------------------------------------------------------------------------------------------------------
def test_abi_lists_every_new_symbol_and_header_declares_it():
    pcr = importlib.import_module(PKG)
    header = open(os.path.join(ROOT, "include", "pcr.h")).read()
    for s in NEW_SYMBOLS:
        assert s in pcr.ABI_SYMBOLS, s
        assert f"int {s}(" in header, s
    assert "PCR_EMPTY_CLUSTER" in header and "UNPINNED" in header and "DIFFERS" in header
    assert pcr.PCR_EMPTY_CLUSTER == 1 and (pcr.PCR_KMEANS_PY, pcr.PCR_KMEANS_CPP) == (0, 1)


def test_hw3_module_surface():
    hw3 = importlib.import_module(PKG + ".hw3")
    km = hw3.K_Means(n_clusters=3, tolerance=1e-4, max_iter=200)
    assert (km.k_, km.tolerance_, km.max_iter_, km.center_, km.init_center) == (3, 1e-4, 200, None, None)
    assert km.predict(np.zeros((4, 2))) is None                 # "Fit model first!" (KMeans.py:77-79)
    g = hw3.GMM(n_clusters=3, max_iter=50)
    assert (g.n_clusters, g.max_iter, g.model_params) == (3, 50, None)
    for name in ("fit", "predict", "init_choice"):
        assert callable(getattr(km, name)) and callable(getattr(g, name))


def test_fixture_holds_data_only_and_is_small():
    assert os.path.getsize(GOLD) < (1 << 20)
    z = gold()
    for name in SETS:
        assert z[f"data_{name}"].shape == (1500, 2) and z[f"data_{name}"].dtype == np.float64


@pytest.mark.parametrize("name", SETS)
def test_restatement_matches_reference_kmeans(name):
    z = gold()
    x = z[f"data_{name}"]
    for t in range(3):
        init = z[f"km_{name}_{t}_init"]
        hist, count, conv = rs_kmeans_fit(x, x[init], 1e-4, 200)
        assert count == int(z[f"km_{name}_{t}_passes"]) and conv == bool(z[f"km_{name}_{t}_converged"])
        ref_hist = z[f"km_{name}_{t}_centres"]
        assert ref_hist.shape == (count + 1,) + hist[0].shape
        bound = 2.0 ** -52 * np.abs(x).max() * 11        # the reference's np.mean: pairwise f64 sums, <= 20 roundings at 1 500 rows; + one here
        assert np.max(np.abs(np.array(hist) - ref_hist)) <= bound
        labels, s = rs_assign(x, hist[-1])
        bad = labels != z[f"km_{name}_{t}_labels"]
        assert not (bad & ~rs_near_tie(s)).any() and bad.mean() <= 0.005


@pytest.mark.parametrize("name", SETS)
def test_restatement_matches_reference_seeding(name):
    z = gold()
    x = z[f"data_{name}"]
    for tag, factor in (("km", 1.0), ("gmm", 1.25)):
        u = z[f"seed_{tag}_{name}_u"]
        picks, p = rs_seed(x, u.size, factor, u)
        assert np.array_equal(picks, z[f"seed_{tag}_{name}_picks"])
        ref = z[f"seed_{tag}_{name}_p"]
        assert np.array_equal(p == 0, ref == 0) and np.all(np.abs(p - ref) <= 8 * U * ref)


@pytest.mark.parametrize("name", SETS)
def test_restatement_matches_reference_gmm(name):
    z = gold()
    x = z[f"data_{name}"]
    scale = np.abs(x).max()
    floors = np.array([scale, scale * scale, 1.0]) * 2.0 ** -40
    for r in range(z[f"em_{name}_in_mean"].shape[0]):
        got = rs_em_step(x, z[f"em_{name}_in_mean"][r], z[f"em_{name}_in_cov"][r], z[f"em_{name}_in_pi"][r])
        for q, (a, key) in enumerate(zip(got[:3], ("mean", "cov", "pi"))):
            assert np.max(np.abs(a - z[f"em_{name}_out_{key}"][r])) <= max(z[f"em_{name}_step_err"][q], floors[q])
    mean, cov, pi, count, margins = rs_gmm_fit(x, x[z[f"gmm_{name}_init"]], 0.3, 1e-4, 100)
    assert count == int(z[f"gmm_{name}_iters"])
    for q, (a, key) in enumerate(zip((mean, cov, pi), ("mean", "cov", "pi"))):
        assert np.max(np.abs(a - z[f"gmm_{name}_{key}"])) <= z[f"gmm_{name}_fit_err"][q]


# ---- GPU tests -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    pcr = importlib.import_module(PKG)
    c = pcr.Context(0)
    yield c
    c.close()


def _step_cases():
    z = gold()
    cases = [(name, z[f"data_{name}"], k) for name in SETS for k in (2, 3, 8)]
    scan = widened_scan()
    cases += [(f"scan{k}", scan, k) for k in (2, 8, 64)]
    g = np.stack(np.meshgrid(np.arange(40.0), np.arange(40.0), indexing="ij"), -1).reshape(-1, 2)      # lattice: exact ties between centres
    cases.append(("lattice", np.ascontiguousarray(g), 4))
    return cases


@pytest.mark.gpu
def test_step_parity_and_geometry_independence(ctx):
    for name, x, k in _step_cases():
        c = np.array([[10.0, 10.0], [20.0, 10.0], [10.0, 20.0], [20.0, 20.0]]) if name == "lattice" else spread_centres(x, k)
        m = ctx.mat64(x)
        try:
            ctx.tune("mixture_geometry", 0)
            labels, counts, new, rc = m.kmeans_step(c)
            want, s = rs_assign(x, c)
            assert np.array_equal(labels, want), f"{name}: {(labels != want).sum()} labels differ from the restatement"
            exact, wc = rs_exact_centres(x, want, k)
            assert np.array_equal(counts, wc) and rc == (1 if (wc == 0).any() else 0)
            ok = wc > 0
            err = np.max(np.abs(new[ok] - exact[ok]))
            print(f"{name} k={k}: max |c - fsum/m| = {err:.3e}, bound {2.0 ** -52 * np.abs(x).max():.3e}")
            assert err <= 2.0 ** -52 * np.abs(x).max()
            assert np.isnan(new[~ok]).all()
            assert np.array_equal(m.kmeans_predict(c), want)
            ctx.tune("mixture_geometry", 1)
            l2, c2, n2, rc2 = m.kmeans_step(c)
            assert np.array_equal(l2, labels) and np.array_equal(c2, counts) and rc2 == rc
            assert np.array_equal(n2.view(np.uint64), new.view(np.uint64)), f"{name}: centres depend on the launch geometry"
        finally:
            ctx.tune("mixture_geometry", 0)
            m.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_fit_against_reference_kmeans(ctx, name):
    pcr = importlib.import_module(PKG)
    z = gold()
    x = z[f"data_{name}"]
    m = ctx.mat64(x)
    bound = 2.0 ** -52 * np.abs(x).max()
    for t in range(3):
        init = z[f"km_{name}_{t}_init"]
        ref_hist = z[f"km_{name}_{t}_centres"]
        passes = int(z[f"km_{name}_{t}_passes"])
        centres, labels, iters, conv, rc = m.kmeans_fit(x[init], 1e-4, 200, pcr.PCR_KMEANS_PY)
        assert rc == 0 and iters == passes and conv == bool(z[f"km_{name}_{t}_converged"])
        c = x[init].copy()
        for it in range(passes):                                    # every recorded iteration: one step from the reference's own centres
            _, _, c, rc = m.kmeans_step(ref_hist[it])
            exact, _ = rs_exact_centres(x, rs_assign(x, ref_hist[it])[0], c.shape[0])
            assert rc == 0 and np.max(np.abs(c - exact)) <= bound
        err = np.max(np.abs(centres - ref_hist[-1]))
        print(f"{name}/{t}: passes {iters}, max |centres - reference| = {err:.3e}")
        assert err <= bound * 11                                     # the reference's own pairwise np.mean: <= 20 roundings at 1 500 rows
        _, s = rs_assign(x, centres)
        bad = labels != z[f"km_{name}_{t}_labels"]
        assert not (bad & ~rs_near_tie(s)).any() and bad.mean() <= 0.005
        cpp = m.kmeans_fit(x[init], 1e-4, 200, pcr.PCR_KMEANS_CPP)
        hist, count, cv = rs_kmeans_fit(x, x[init], 1e-4, 200, "cpp")
        assert cpp[2] == count and cpp[3] == cv and np.max(np.abs(cpp[0] - hist[-1])) <= bound
    m.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_seeding_against_reference(ctx, name):
    z = gold()
    x = z[f"data_{name}"]
    m = ctx.mat64(x)
    for tag, factor in (("km", 1.0), ("gmm", 1.25)):
        u = z[f"seed_{tag}_{name}_u"]
        picks, p = m.kmeanspp_init(u.size, factor, u=u, want_p=True)
        ref = z[f"seed_{tag}_{name}_p"]
        rel = np.max(np.abs(p - ref)[ref > 0] / ref[ref > 0])
        print(f"{name}/{tag}: max relative difference of p_last = {rel / U:.2f} x 2^-53")
        assert np.array_equal(p == 0, ref == 0) and rel <= 8 * U
        assert np.array_equal(picks, z[f"seed_{tag}_{name}_picks"])
    a, b = m.kmeanspp_init(5, 1.0, seed=7), m.kmeanspp_init(5, 1.0, seed=7)
    assert np.array_equal(a, b) and len(set(a.tolist())) == 5
    m.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_em_step_against_reference(ctx, name):
    z = gold()
    x = z[f"data_{name}"]
    scale = np.abs(x).max()
    floors = np.array([scale, scale * scale, 1.0]) * 2.0 ** -40
    m = ctx.mat64(x)
    for r in range(z[f"em_{name}_in_mean"].shape[0]):
        args = (z[f"em_{name}_in_mean"][r], z[f"em_{name}_in_cov"][r], z[f"em_{name}_in_pi"][r])
        ctx.tune("mixture_geometry", 0)
        got = m.gmm_em_step(*args, want_post=True)
        for q, key in enumerate(("mean", "cov", "pi")):
            err = np.max(np.abs(got[q] - z[f"em_{name}_out_{key}"][r]))
            bar = max(8 * z[f"em_{name}_step_err"][q], floors[q])
            print(f"{name} step {r} {key}: {err:.3e} (bar {bar:.3e})")
            assert err <= bar
        assert np.max(np.abs(got[3] - rs_em_step(x, *args)[3])) <= 1e-12 and np.allclose(got[3].sum(axis=1), 1.0, atol=1e-14)
        ctx.tune("mixture_geometry", 1)
        alt = m.gmm_em_step(*args)
        ctx.tune("mixture_geometry", 0)
        for q in range(3):
            assert np.array_equal(alt[q].view(np.uint64), got[q].view(np.uint64)), "EM sums depend on the launch geometry"
    m.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SETS)
def test_full_gmm_fit_against_reference(ctx, name):
    z = gold()
    x = z[f"data_{name}"]
    m = ctx.mat64(x)
    mean, cov, pi, info = m.gmm_fit(x[z[f"gmm_{name}_init"]], 0.3, 1e-4, 100, seed=1)
    assert info["iters"] == int(z[f"gmm_{name}_iters"]) and info["resets"] == 0
    for q, (a, key) in enumerate(zip((mean, cov, pi), ("mean", "cov", "pi"))):
        err = np.max(np.abs(a - z[f"gmm_{name}_{key}"]))
        print(f"{name} fit {key}: {err:.3e} (bar {8 * z[f'gmm_{name}_fit_err'][q]:.3e})")
        assert err <= 8 * z[f"gmm_{name}_fit_err"][q]
    labels = m.gmm_predict(mean, cov, pi)
    lp = np.sort(rs_logpost(x, mean, cov, pi), axis=1)
    close = (lp[:, -1] - lp[:, -2]) <= 1e-9
    bad = labels != z[f"gmm_{name}_labels"]
    assert not (bad & ~close).any() and bad.mean() <= 0.005
    m.free()


@pytest.mark.gpu
def test_errors_return(ctx):
    pcr = importlib.import_module(PKG)
    x = gold()["data_blobs"]
    m = ctx.mat64(x)
    far = np.array([[0.0, 0.0], [1e6, 1e6], [x[0, 0], x[0, 1]]])
    labels, counts, new, rc = m.kmeans_step(far)
    assert rc == pcr.PCR_EMPTY_CLUSTER and counts[1] == 0 and np.isnan(new[1]).all()
    out = m.kmeans_fit(far, 1e-4, 50)
    assert out[4] == pcr.PCR_EMPTY_CLUSTER and out[2] == 1
    sing = np.array([np.identity(2), [[1.0, 1.0], [1.0, 1.0]]])
    with pytest.raises(pcr.PcrError, match="bad state"):
        m.gmm_em_step(x[:2], sing, np.array([0.5, 0.5]))
    with pytest.raises(pcr.PcrError, match="bad argument"):
        ctx.mat64(np.zeros((10, 9)))
    with pytest.raises(pcr.PcrError, match="bad argument"):
        m.kmeans_step(np.zeros((65, 2)))
    bad = x.copy()
    bad[7, 1] = np.nan
    with pytest.raises(pcr.PcrError, match="bad argument"):
        ctx.mat64(bad)
    big = ctx.mat64(x * 1000.0)                                      # distances beyond 709: exp overflows
    with pytest.raises(pcr.PcrError, match="bad state"):
        big.kmeanspp_init(3, 1.0, u=np.array([0.1, 0.5, 0.9]))
    labels, counts, new, rc = m.kmeans_step(x[:3])                   # the context is still usable
    assert rc == 0 and counts.sum() == x.shape[0]
    big.free()
    m.free()


@pytest.mark.gpu
def test_hw3_classes_run_like_the_reference(ctx):
    hw3 = importlib.import_module(PKG + ".hw3")
    z = gold()
    x = z["data_blobs"]
    km = hw3.K_Means(n_clusters=3, init_idx=z["km_blobs_0_init"])
    km.fit(x)
    assert np.max(np.abs(km.center_ - z["km_blobs_0_centres"][-1])) <= 11 * 2.0 ** -52 * np.abs(x).max()
    assert np.array_equal(km.init_center, x[z["km_blobs_0_init"]])
    assert (km.predict(x) != z["km_blobs_0_labels"]).mean() <= 0.005
    g = hw3.GMM(n_clusters=3, init_idx=z["gmm_blobs_init"])
    g.fit(x)
    assert len(g.model_params) == 3 and g.iterations_ == int(z["gmm_blobs_iters"])
    assert (g.predict(x) != z["gmm_blobs_labels"]).mean() <= 0.005
    seeded = hw3.K_Means(n_clusters=3, seed=11)
    seeded.fit(x)
    again = hw3.K_Means(n_clusters=3, seed=11)
    again.fit(x)
    assert np.array_equal(seeded.center_, again.center_, equal_nan=True)
