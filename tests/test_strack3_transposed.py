"""STRACK3 reads its sphere-row masks from ONE ballot of the transposed product (csrc/nn1_sphere.hpp, tune nn1_s3_transposed: 1 = default,
2 = one ballot per accumulator, the earlier form kept as nn1_strack3_rows_kernel).  Flags only decide what is looked at and keys come from the
exact arithmetic, so both forms must return the same keys as the exact-only kernel (nn1_variant 2) bit for bit; and the transposed product
multiplies the same pairs of f16 values, so the flag sets — the counters of the diagnostics launch — must be the same too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCH = (1, 2)              # nn1_s3_transposed
GROUPS = (1, 2, 4)           # nn1_sphere_qg: the three instances of the kernel
KEYS = ("nn_method", "nn1_variant", "nn1_s3_transposed", "nn1_sphere_qg", "nn1_async_in_loop", "nn1_sphere_reseed", "nn1_sign_flush", "nn1_sphere_flush_end", "grid_stats")


def bits32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def ctx(pcr):
    c = pcr.Context(0)
    yield c
    c.close()


def reset(ctx):
    for k in KEYS:
        ctx.tune(k, 0)


def exact(ctx, ct, cs):
    ctx.tune("nn_method", 1); ctx.tune("nn1_variant", 2)
    out = ctx.nn1(ct, cs)
    ctx.tune("nn1_variant", 0)
    return out


def strack3(ctx, ct, cs, sw, qg):
    ctx.tune("nn_method", 1); ctx.tune("nn1_variant", 10); ctx.tune("nn1_s3_transposed", sw); ctx.tune("nn1_sphere_qg", qg)
    out = ctx.nn1(ct, cs)
    assert ctx.mfma_check()["last_nn1_kernel"] == "strack3", (sw, qg)
    return out


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits32(a[1]), bits32(b[1]))


@pytest.mark.parametrize("ns,nt", [(1, 1), (63, 5), (257, 1023), (1000, 1025), (3001, 7000), (5000, 2049), (4097, 33000)])
def test_ragged_sizes_both_forms_equal_the_exact_kernel(ctx, synth, ns, nt):
    src, _ = synth.kitti_like_pair(max(ns, 64), seed_target=7 + ns, seed_pair=11 + nt)
    tgt = synth.kitti_like_scan(max(nt, 64), seed=13 + nt)
    src, tgt = np.ascontiguousarray(src[:, :ns]), np.ascontiguousarray(tgt[:, :nt])
    cs, ct = ctx.cloud(src), ctx.cloud(tgt)
    ref = exact(ctx, ct, cs)
    for qg in GROUPS:
        got = {sw: strack3(ctx, ct, cs, sw, qg) for sw in SWITCH}
        assert same(got[1], got[2]), (ns, nt, qg)
        assert same(got[1], ref), (ns, nt, qg, int((got[1][0] != ref[0]).sum()))
    reset(ctx)


def test_ties_and_duplicates_both_forms_equal_the_exact_kernel(ctx, orc, synth):
    lat = synth.lattice_cloud(40000, 3, 10.0, seed=5, levels=10).astype(np.float32)
    q = synth.lattice_cloud(3000, 3, 10.0, seed=6, levels=10).astype(np.float32)
    tgt, src = np.ascontiguousarray(lat.T), np.ascontiguousarray(q.T)
    tgt[:, 20000:20500] = tgt[:, 1500:2000]                          # exact duplicates: the lowest index must win
    assert (orc.nn1_tiecount_f32(tgt, src) > 1).sum() > 1000
    cs, ct = ctx.cloud(src), ctx.cloud(tgt)
    ref = exact(ctx, ct, cs)
    for qg in GROUPS:
        got = {sw: strack3(ctx, ct, cs, sw, qg) for sw in SWITCH}
        assert same(got[1], got[2]) and same(got[1], ref), qg
    reset(ctx)


def test_nonfinite_queries_and_cold_stale_absent_seeds(ctx, synth):
    """Five poses in a row against one target: the first search of a fresh target is cold (it seeds itself), the later ones start from the keys
    of the pose before — metres away and rotated, i.e. stale —, once refreshed (default) and once kept as they are (nn1_sphere_reseed = 2);
    NaN / inf queries and queries 10^6 m away have no usable seed at all (the wave scans its slice exactly for their group)."""
    n = 40000
    src, tgt = synth.kitti_like_pair(n, seed_target=811, seed_pair=812)
    tgt = tgt.copy(); src = src.copy()
    tgt[:, :2000] = np.round(tgt[:, :2000] * 4) / 4
    tgt[:, 2000:2500] = tgt[:, 1500:2000]
    src[:, :500] = tgt[:, 1700:2200]
    src[:, 5] = np.nan; src[0, 77] = np.inf; src[2, 78] = -np.inf; src[:, 100:110] = 1.0e6
    c, s_ = np.float32(np.cos(0.7)), np.float32(np.sin(0.7))
    Rz = np.array([[c, -s_, 0], [s_, c, 0], [0, 0, 1]], np.float32)
    with np.errstate(invalid="ignore"):
        poses = [src, src + np.array([[0.05], [-0.03], [0.01]], np.float32), Rz @ src + np.array([[4.0], [-7.0], [0.5]], np.float32), src, src * np.float32(0.5)]
    poses = [np.ascontiguousarray(p_, np.float32) for p_ in poses]
    ct = ctx.cloud(tgt)
    clouds = [ctx.cloud(p_) for p_ in poses]
    ref = [exact(ctx, ct, c_) for c_ in clouds]
    ctx.tune("nn_method", 1); ctx.tune("nn1_variant", 10)
    for qg in GROUPS:
        for reseed, flush, fend in ((0, 0, 0), (2, 1, 0), (2, 100000, 128)):
            for sw in SWITCH:
                ctx.tune("nn1_s3_transposed", sw); ctx.tune("nn1_sphere_qg", qg); ctx.tune("nn1_sphere_reseed", reseed)
                ctx.tune("nn1_sign_flush", flush); ctx.tune("nn1_sphere_flush_end", fend)
                ctx.tune("nn1_async_in_loop", 1)
                fresh = ctx.cloud(tgt)
                for k, c_ in enumerate(clouds + clouds[:2]):
                    ctx.nn1_async(fresh, c_)
                    assert ctx.mfma_check()["last_nn1_kernel"] == "strack3", (qg, reseed, sw, k)
                    got = ctx.nn1_fetch(n)
                    assert same(got, ref[k % len(clouds)]), (qg, reseed, flush, sw, k, int((got[0] != ref[k % len(clouds)][0]).sum()))
                ctx.tune("nn1_async_in_loop", 0)
                fresh.free()
    reset(ctx)


def test_target_over_several_level0_supertiles(ctx, synth):
    n, nq = 300_000, 24_000
    src_all, tgt = synth.kitti_like_pair(n, seed_target=811, seed_pair=812)
    src = np.ascontiguousarray(src_all[:, :: n // nq][:, :nq]).copy()
    src[:, 17] = np.nan; src[1, 18] = np.inf
    src[:, 100:140] += np.float32(500.0)
    src[:, 200:230] *= np.float32(1.0e-3)
    ct, cs = ctx.cloud(tgt), ctx.cloud(src)
    ref = exact(ctx, ct, cs)
    for qg in GROUPS:
        for per_slice in (0, 1):
            ctx.tune("nn1_sphere_l0_per_slice", per_slice)
            got = {sw: strack3(ctx, ct, cs, sw, qg) for sw in SWITCH}
            assert same(got[1], got[2]) and same(got[1], ref), (qg, per_slice, int((got[1][0] != ref[0]).sum()))
    ctx.tune("nn1_sphere_l0_per_slice", 0)
    reset(ctx)


def test_icp_120k_pose_bits_stats_and_flag_counters_equal(ctx, synth):
    """The headline loop (20 iterations, 120 000 x 120 000, exhaustive search) under both forms: pose bits and stats equal; then the diagnostics
    launch at the final pose: level-1 tiles flagged by level 0 (word 3), level-2 tiles flagged by level 1 (word 9), (query, chunk) pairs
    evaluated exactly (word 6) and the MFMAs of levels 1 and 2 (words 8, 10) equal — the transposed product sets the same signs."""
    src, tgt = synth.kitti_like_pair(120000)
    cs, ct = ctx.cloud(src), ctx.cloud(tgt)
    ctx.tune("nn_method", 1)
    for qg in GROUPS:
        ctx.tune("nn1_sphere_qg", qg)
        out = {}
        for sw in SWITCH:
            ctx.tune("nn1_s3_transposed", sw)
            T, st = ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=20, eps=0.0)
            assert ctx.mfma_check()["last_nn1_kernel"] == "strack3", (qg, sw)
            ctx.tune("grid_stats", 1)
            ctx.icp_point2point(cs, ct, init_T=T, max_corr=1.0, max_iter=2, eps=0.0)
            w = [int(v) for v in ctx.nn1_stats()]
            ctx.tune("grid_stats", 0)
            out[sw] = (T.copy(), dict(st), w)
            print(f"qg {qg} nn1_s3_transposed {sw}: l0 mfma {w[7]} l1 tiles flagged {w[3]} l1 mfma {w[8]} l2 tiles flagged {w[9]} l2 mfma {w[10]} evaluated {w[6]}")
        (T1, s1, w1), (T2, s2, w2) = out[1], out[2]
        assert np.array_equal(T1.view(np.uint32), T2.view(np.uint32)), qg
        for k in ("iters_run", "converged", "empty_pairs", "last_pairs", "nn_launches"):
            assert s1[k] == s2[k], (qg, k, s1[k], s2[k])
        assert np.array_equal(bits32(s1["last_loss"]), bits32(s2["last_loss"])), (qg, s1["last_loss"], s2["last_loss"])
        assert w1[3] > 0 and w1[9] > 0 and w1[6] > 0, w1
        for word in (3, 9, 6, 8, 10):
            assert w1[word] == w2[word], (qg, word, w1, w2)
    reset(ctx)
