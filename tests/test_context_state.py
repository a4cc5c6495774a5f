"""State a context keeps between calls (-m gpu): the per-query result buffer keys[], the sorted-cloud mapping, the pinned words that carry
index-build counters back to the host, shard indices on copies — and the default large-target kernels on real scan geometry.

Every search is compared bit for bit with the oracle (index equal, d2 as uint32 bits), every pose with the oracle's ICP or the CPU loop of
test_fullsize.py.  A "dirty" context has just answered a self-query nn1(P, P): every keys[i] then holds (d2 = 0, idx = i), a key no later
candidate can beat, so a search that merges with stale keys[] shows it."""
import os

import numpy as np
import pytest

from test_fullsize import THREADS, CpuIcp, assert_same_search, cpu_nn1
from test_gpu_parity import VARIANTS, pcr_mat4

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(idx, d2, oidx, od2, what):
    bad = np.flatnonzero((idx != oidx) | (bits32(d2) != bits32(od2)))
    assert bad.size == 0, f"{what}: {bad.size} queries differ, first {bad[:4]}: got {idx[bad[:4]]} {d2[bad[:4]]}, want {oidx[bad[:4]]} {od2[bad[:4]]}"


# ------------------------------------------------------------------ §A degenerate targets on a dirty context
P_DEG = np.array([1.5, -2.25, 0.5], np.float32)


def _deg_targets(synth):
    rng = np.random.default_rng(41)
    out = {}
    for nt in (1, 2, 300, 8192, 40000):
        out[f"coincident{nt}"] = np.ascontiguousarray(np.repeat(P_DEG[:, None], nt, axis=1))
    k = np.arange(8192)
    # extent ~1.5e-39: below the Morton lattice (1024 / extent overflows f32, key_inv = 0); subnormal coordinates, d2 underflows to 0
    out["sublattice"] = np.ascontiguousarray(np.stack([(k % 16) * 1e-40, (k // 16 % 16) * 1e-40, (k // 256) * 1e-40]).astype(np.float32))
    scan = synth.kitti_like_scan(40000, seed=43)
    out["collinear"] = np.ascontiguousarray(np.stack([scan[0], np.zeros(40000), np.zeros(40000)]).astype(np.float32))
    out["coplanar"] = np.ascontiguousarray(np.stack([scan[0], scan[1], np.zeros(40000)]).astype(np.float32))
    for m in (300, 4096):                      # a zero-radius super-tile (256 records) / level-1 super-tile (4 096 records)
        t = scan.copy()
        t[:, 5000:5000 + m] = t[:, 5000:5001]
        out[f"dup{m}"] = np.ascontiguousarray(t)
    t = scan.copy()                            # a cluster of radius ~1e-30 at the sensor: the f16 scale exponent of its tiles leaves [-60, 60]
    t[:, 7000:7600] = rng.normal(0.0, 1e-30, (3, 600)).astype(np.float32)
    out["cluster1e-30"] = np.ascontiguousarray(t)
    return out


def _deg_queries(synth, tgt):
    q = synth.kitti_like_scan(2500, seed=47)
    p = tgt[:, tgt.shape[1] // 2]
    special = np.stack([p, p, tgt[:, 0], [np.nan, 0, 0], [0, np.inf, 0], [-np.inf, 1, 2], [np.nan, np.nan, np.nan]], axis=1).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([q, special], axis=1))


def _dirty(ctx, P):
    ctx.tune("nn_method", 0); ctx.tune("nn1_variant", 0)
    i, d = ctx.nn1(P, P)
    assert (i == np.arange(len(P), dtype=np.uint32)).all() and (d == 0).all()


def _configs():
    yield "auto", {"nn_method": 0}
    for v in VARIANTS:
        yield f"brute-v{v}", {"nn_method": 1, "nn1_variant": v}
    yield "grid", {"nn_method": 2}


def _tune(ctx, cfg):
    ctx.tune("nn_method", 0); ctx.tune("nn1_variant", 0)
    for k, v in cfg.items():
        ctx.tune(k, v)


@pytest.fixture(scope="module")
def deg(synth):
    return _deg_targets(synth)


@pytest.mark.parametrize("name", ["coincident1", "coincident2", "coincident300", "coincident8192", "coincident40000", "sublattice",
                                  "collinear", "coplanar", "dup300", "dup4096", "cluster1e-30"])
def test_degenerate_target_one_shot_and_loop_on_dirty_and_fresh_context(pcr, orc, synth, deg, name, record_property):
    tgt = deg[name]
    src = _deg_queries(synth, tgt)
    oidx, od2 = orc.nn1_f32_mt(tgt, src, threads=THREADS)
    finite = np.isfinite(src).all(axis=0)
    if name.startswith("coincident"):
        assert (oidx[finite] == 0).all() and (oidx[~finite] == NONE).all()
    P = synth.kitti_like_scan(20000, seed=53)
    kernels = {}
    for dirty in (True, False):
        with pcr.Context(0) as ctx:
            cP, ct, cs = ctx.cloud(P), ctx.cloud(tgt), ctx.cloud(src)
            for label, cfg in _configs():
                if dirty:
                    _dirty(ctx, cP)
                _tune(ctx, cfg)
                idx, d2 = ctx.nn1(ct, cs)
                kern = ctx.mfma_check()["last_nn1_kernel"]
                kernels[label] = kern
                same(idx, d2, oidx, od2, f"{name} {label} dirty={dirty} ({kern})")
                if name.startswith("coincident"):
                    assert (idx[finite] == 0).all()
            # a caller's loop: sort the queries for the target, one bounded search
            for label, cfg in (("loop-brute", {"nn_method": 1}), ("loop-grid", {"nn_method": 2})):
                if dirty:
                    _dirty(ctx, cP)
                _tune(ctx, cfg)
                work = cs.clone()
                orig = ctx.sort_for_target(ct, work)
                assert np.array_equal(np.sort(orig), np.arange(src.shape[1], dtype=np.uint32))
                ctx.nn1_loop(ct, work, 1.0)
                idx, d2 = ctx.nn1_fetch(src.shape[1])
                gi, gd = np.empty_like(idx), np.empty_like(d2)
                gi[orig], gd[orig] = idx, d2
                inside = od2 < np.float32(1.0)
                same(gi[inside], gd[inside], oidx[inside], od2[inside], f"{name} {label} dirty={dirty}")
                assert (gi[~inside] == NONE).all() and np.isinf(gd[~inside]).all(), f"{name} {label}"
                work.free()
            _tune(ctx, {})
            for c in (cP, ct, cs):
                c.free()
    record_property("kernels", kernels)
    if name == "cluster1e-30":
        # the cluster's tiles leave f16's exponent range: a forced f16 variant falls back to a form without f16 operands
        assert kernels["brute-v10"] not in ("htrack", "strack", "strack3"), kernels
        assert kernels["brute-v7"] not in ("htrack", "strack", "strack3"), kernels


@pytest.mark.parametrize("name", ["coincident1", "coincident300", "coincident8192", "coincident40000", "sublattice", "collinear", "coplanar",
                                  "dup4096", "cluster1e-30"])
def test_degenerate_target_icp_follows_the_oracle_state_machine(pcr, orc, synth, deg, name):
    """onto a degenerate target the Kabsch matrix has rank 0 or 1: pose and stats (empty_pairs included) follow the oracle"""
    tgt = deg[name]
    src = _deg_queries(synth, tgt)
    src = np.ascontiguousarray(src[:, np.isfinite(src).all(axis=0)])
    oT, ost = orc.icp_p2p_f32(src, tgt, max_corr=1.0, max_iter=3, eps=1e-8)
    P = synth.kitti_like_scan(20000, seed=53)
    with pcr.Context(0) as ctx:
        cP, ct, cs = ctx.cloud(P), ctx.cloud(tgt), ctx.cloud(src)
        for method in (0, 1, 2):
            _dirty(ctx, cP)
            _tune(ctx, {"nn_method": method})
            T, st = ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=3, eps=1e-8)
            for k in ("iters_run", "converged", "empty_pairs", "last_pairs"):
                assert st[k] == ost[k], (name, method, k, st, ost)
            if name == "collinear":
                # a rank-1 cross-covariance leaves the rotation about the line free: any such pose is a Kabsch solution, so only where it
                # puts the line is compared (the kept source points' images, projected off the x axis, must agree)
                ps = src[:, :64].astype(np.float64)
                a_, b_ = T[:3, :3] @ ps + T[:3, 3:], oT[:3, :3] @ ps + oT[:3, 3:]
                assert np.allclose(a_[0], b_[0], atol=1e-4), (name, method)
                continue
            assert np.linalg.norm(T.astype(np.float64) - oT.astype(np.float64)) <= 1e-5, (name, method, T, oT)
        _tune(ctx, {})
        for c in (cP, ct, cs):
            c.free()


# ------------------------------------------------------------------ §B the sorted-cloud mapping survives other calls
def _loop_step(pcr, ctx, ct, work, T):
    ctx.nn1_loop(ct, work, 1.0)
    sums, last, last_d2 = ctx.kabsch_sums(ct, work, 1.0)
    rc, R, t = pcr.kabsch_solve(sums)
    assert rc == 0
    Td = np.eye(4, dtype=np.float32); Td[:3, :3], Td[:3, 3] = R, t
    ctx.transform(work, Td)
    return sums, last, last_d2, pcr_mat4(Td, T)


@pytest.mark.parametrize("cfg", [{"nn_method": 1}, {"nn_method": 2}, {"nn_method": 2, "grid_tile": 1}], ids=["brute", "grid", "grid-stile"])
def test_sorted_mapping_survives_interleaved_calls(pcr, orc, synth, cfg):
    n, steps = 30000, 4
    src, tgt = synth.kitti_like_pair(n)
    other_s, other_t = synth.kitti_like_pair(12000, seed_target=61, seed_pair=62)
    third = synth.kitti_like_scan(9000, seed=63)

    def run(interleave):
        out = []
        with pcr.Context(0) as ctx:
            for k, v in cfg.items():
                ctx.tune(k, v)
            cs, ct = ctx.cloud(src), ctx.cloud(tgt)
            os_, ot, c3 = ctx.cloud(other_s), ctx.cloud(other_t), ctx.cloud(third)
            work = cs.clone()
            orig = ctx.sort_for_target(ct, work)
            inv = np.argsort(orig)
            T = np.eye(4, dtype=np.float32)
            for it in range(steps):
                if interleave and it == 1:
                    ctx.icp_point2point(os_, ot, max_corr=1.0, max_iter=3, eps=1e-8)
                if interleave and it == 2:
                    ctx.sort_for_target(ot, c3)
                if interleave and it == 3:
                    ctx.nn1(ot, os_)
                cur = work.numpy()[:, inv]                                   # the moved cloud in the ORIGINAL order
                sums, last, last_d2, T = _loop_step(pcr, ctx, ct, work, T)
                kern = ctx.mfma_check()["last_nn1_kernel"]
                idx, d2 = ctx.nn1_fetch(n)
                gi, gd = np.empty_like(idx), np.empty_like(d2)
                gi[orig], gd[orig] = idx, d2
                osums, olast = orc.kabsch_accumulate(cur, tgt, gi, gd, 1.0)
                assert last == olast, (cfg, interleave, it, last, olast)          # `last` in the original numbering
                assert int(sums[15]) == int(osums[15])
                out.append((sums.copy(), last, np.float32(last_d2), T.copy(), kern))
            for c in (cs, ct, os_, ot, c3, work):
                c.free()
        return out

    ref, got = run(False), run(True)
    for it, (a, b) in enumerate(zip(ref, got)):
        assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)), (cfg, it)
        assert a[1] == b[1] and bits32(a[2]) == bits32(b[2]), (cfg, it)
        assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32)), (cfg, it)
        if cfg.get("grid_tile") == 1:
            assert a[4] == "grid-stile" and b[4] == "grid-stile", (it, a[4], b[4])


# ------------------------------------------------------------------ §C a copy of a spatial shard keeps its global index
def test_shard_clone_and_assign_keep_the_global_index(pcr, synth):
    src, tgt = synth.kitti_like_pair(20000)
    with pcr.Context(0) as ctx:
        ct, full = ctx.cloud(tgt), ctx.cloud(src)
        sh = ctx.shard_spatial(ct, full, 2, 1, 5)
        gi = ctx.global_index(sh)
        assert gi.size > 0 and np.array_equal(sh.numpy(), src[:, gi])
        cl = sh.clone()
        assert np.array_equal(ctx.global_index(cl), gi)
        # pcr_cloud_assign: dst becomes a copy of src, shard indices included — and loses its own when src has none
        plain = ctx.cloud(np.zeros((3, len(sh)), np.float32))
        with pytest.raises(pcr.PcrError):
            ctx.global_index(plain)
        plain.assign(sh)
        assert np.array_equal(ctx.global_index(plain), gi) and np.array_equal(plain.numpy(), sh.numpy())
        other = ctx.cloud(np.ones((3, len(sh)), np.float32))
        cl.assign(other)
        with pytest.raises(pcr.PcrError):
            ctx.global_index(cl)
        # single-rank ICP on the shard and on its copy: same pose bits and stats
        T1, s1 = ctx.icp_point2point(sh, ct, max_corr=1.0, max_iter=5, eps=1e-8)
        T2, s2 = ctx.icp_point2point(plain, ct, max_corr=1.0, max_iter=5, eps=1e-8)
        assert np.array_equal(T1.view(np.uint32), T2.view(np.uint32)) and s1["last_pairs"] == s2["last_pairs"]
        for c in (ct, full, sh, cl, plain, other):
            c.free()


# ------------------------------------------------------------------ §D a later grid build does not cost a large target its tile search
def test_unrelated_grid_build_keeps_the_tile_search(pcr, orc, synth):
    N = 4_200_000
    src, tgt = synth.kitti_like_pair(N)
    small = synth.kitti_like_scan(5000, seed=71)
    with pcr.Context(0) as ctx:
        ctx.tune("nn_method", 2)
        cs = ctx.cloud(src)
        kernels = []
        for extra in (False, True):
            ct = ctx.cloud(tgt)                                  # a fresh target: its grid is built by the sort below
            work = cs.clone()
            ctx.sort_for_target(ct, work)
            if extra:
                cdb, cq = ctx.cloud(small), ctx.cloud(small[:, ::3].copy())
                ctx.cloud_knn(cdb, cq, 4)                        # another grid build (and query sort) between the target's build and its loop
                cdb.free(); cq.free()
            ks = []
            for it in range(3):
                ctx.nn1_loop(ct, work, 1.0)
                ks.append(ctx.mfma_check()["last_nn1_kernel"])
            kernels.append(ks)
            if extra:
                idx, d2 = ctx.nn1_fetch(N)
                cur = work.numpy()
                sel = np.arange(0, N, N // 131072)[:131072] if orc.have_ref() else np.arange(0, N, N // 64)[:64]
                q = np.ascontiguousarray(cur[:, sel])
                ridx, rd2, _ = cpu_nn1(orc, tgt, q)
                inside = rd2 < np.float32(1.0)
                assert inside.mean() > 0.9
                gi, gd = idx[sel], d2[sel]
                assert (gi[~inside] == NONE).all() and np.isinf(gd[~inside]).all()
                assert_same_search(gi[inside], gd[inside], ridx[inside], rd2[inside], tgt, q[:, inside], "4.2M loop after a knn build")
            work.free(); ct.free()
        cs.free()
    assert kernels[0][1:] == ["grid-stile"] * 2, kernels
    assert kernels[1] == kernels[0], kernels


# ------------------------------------------------------------------ §E real scan geometry through the default large-target kernels
@pytest.fixture(scope="module")
def real_pair():
    g = np.load(os.path.join(ROOT, "tests", "golden", "kat_kitti_q5.npz"))
    tgt = np.ascontiguousarray(g["db_f32"][:, :3].T.astype(np.float32))
    n = tgt.shape[1]
    rng = np.random.default_rng(5)                               # as tools/run_real_scan.py perturbs it
    a = np.deg2rad(1.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    src = (R @ tgt[:, rng.permutation(n)].astype(np.float64) + np.array([[0.3], [0.1], [0.02]]) + rng.normal(0, 0.01, (3, n))).astype(np.float32)
    return np.ascontiguousarray(src), tgt


def test_real_scan_cold_one_shot_searches(pcr, orc, real_pair):
    src, tgt = real_pair
    n = src.shape[1]
    assert n == 100000
    ridx, rd2, _ = cpu_nn1(orc, tgt, src)
    with pcr.Context(0) as ctx:
        cs, ct = ctx.cloud(src), ctx.cloud(tgt)
        ctx.tune("nn_method", 1)
        idx, d2 = ctx.nn1(ct, cs)
        assert ctx.mfma_check()["last_nn1_kernel"] == "strack3"
        assert_same_search(idx, d2, ridx, rd2, tgt, src, "real scan, brute")
        ct.free(); ct = ctx.cloud(tgt)                           # cold again: no index on the target
        ctx.tune("nn_method", 2)
        idx, d2 = ctx.nn1(ct, cs)
        assert_same_search(idx, d2, ridx, rd2, tgt, src, "real scan, grid")
        ct.free(); ct = ctx.cloud(tgt)
        ctx.tune("grid_tile", 1)
        work = cs.clone()
        orig = ctx.sort_for_target(ct, work)
        ctx.nn1_loop(ct, work, 1.0)
        assert ctx.mfma_check()["last_nn1_kernel"] == "grid-stile"
        idx, d2 = ctx.nn1_fetch(n)
        gi, gd = np.empty_like(idx), np.empty_like(d2)
        gi[orig], gd[orig] = idx, d2
        inside = rd2 < np.float32(1.0)
        assert (gi[~inside] == NONE).all() and np.isinf(gd[~inside]).all()
        assert_same_search(gi[inside], gd[inside], ridx[inside], rd2[inside], tgt, src[:, inside], "real scan, tile search")
        for c in (cs, ct, work):
            c.free()


@pytest.mark.parametrize("method", [1, 2])
def test_real_scan_caller_loop_and_icp_vs_cpu(pcr, orc, real_pair, method):
    src, tgt = real_pair
    n = src.shape[1]
    iters = 20 if orc.have_ref() else 2                          # the exhaustive CPU fallback needs seconds per search
    cpu = CpuIcp(orc, src, tgt, 1.0, 1e-8)
    with pcr.Context(0) as ctx:
        ctx.tune("nn_method", method)
        cs, ct = ctx.cloud(src), ctx.cloud(tgt)
        work = cs.clone()
        orig = ctx.sort_for_target(ct, work)
        inv = np.argsort(orig)
        for it in range(iters):
            cur = work.numpy()[:, inv]
            ctx.nn1_loop(ct, work, 1.0)
            idx, d2 = ctx.nn1_fetch(n)
            gi, gd = np.empty_like(idx), np.empty_like(d2)
            gi[orig], gd[orig] = idx, d2
            ridx, rd2, _ = cpu_nn1(orc, tgt, cur)
            inside = rd2 < np.float32(1.0)
            assert (gi[~inside] == NONE).all() and np.isinf(gd[~inside]).all(), it
            assert_same_search(gi[inside], gd[inside], ridx[inside], rd2[inside], tgt, cur[:, inside], f"real scan loop, method {method}, it {it}")
            sums, last, _ = ctx.kabsch_sums(ct, work, 1.0)
            osums, olast = orc.kabsch_accumulate(cur, tgt, gi, gd, 1.0)
            assert last == olast and int(sums[15]) == int(osums[15]), (it, last, olast)
            cidx, cd2, _ = cpu_nn1(orc, tgt, cpu.cur)
            kept = cpu.step(cidx, cd2)
            assert int(sums[15]) == kept, (it, int(sums[15]), kept)
            rc, R, t = pcr.kabsch_solve(sums)
            assert rc == 0
            Td = np.eye(4, dtype=np.float32); Td[:3, :3], Td[:3, 3] = R, t
            ctx.transform(work, Td)
        T, st = ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=iters, eps=1e-8)
        assert np.linalg.norm(T.astype(np.float64) - cpu.T.astype(np.float64)) <= 1e-5, (T, cpu.T)
        assert st["iters_run"] == cpu.iters_run and st["converged"] == int(cpu.converged) and st["last_pairs"] == kept
        ctx.tune("nn_method", 3 - method)
        T2, st2 = ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=iters, eps=1e-8)
        assert np.array_equal(T.view(np.uint32), T2.view(np.uint32)) and st2["last_pairs"] == st["last_pairs"]
        for c in (cs, ct, work):
            c.free()
