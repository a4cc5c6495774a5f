"""The fused sums + solve + move launch of single-rank ICP loops (csrc/kabsch.hip icp_sums_update_move_kernel): one launch whose
workgroups meet once at a grid barrier, in place of kabsch_partial + icp_update_move.  The yardstick is the three-launch chain in the same
process (tune icp_fused_sums = 2) and, for some cases, the synchronous host loop (icp_pipeline = -1): the pose as uint32, iters_run, converged,
empty_pairs, last_pairs and the bits of last_loss must all be equal — the sums are exact integers, so the new grouping of pairs changes no bit.
A workgroup covers WG = 4 x 512 points (4 x 256 with icp_fused_sums_threads = 256)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WG = 2048
TUNES = ("icp_fused_sums", "icp_fused_sums_threads", "icp_fused_sums_max_blocks", "icp_fused_sums_min", "icp_fused_sums_grid", "icp_pipeline", "icp_chunk",
         "nn_method")


@pytest.fixture(scope="module")
def ctx(pcr):
    c = pcr.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(ctx):
    # (by default the launch serves exhaustive loops from 60 000 points on: here every size and both searches take it)
    ctx.tune("icp_fused_sums_min", 1); ctx.tune("icp_fused_sums_grid", 1)
    yield
    for k in TUNES:
        ctx.tune(k, 0)
    ctx.tune("prof", 0)


def result(ctx, cs, ct, **kw):
    T, st = ctx.icp_point2point(cs, ct, **kw)
    return (T.view(np.uint32).tobytes(), st["iters_run"], st["converged"], st["empty_pairs"], st["last_pairs"], np.float32(st["last_loss"]).tobytes())


def both(ctx, cs, ct, sync=False, **kw):
    """(fused sums, three-launch chain[, synchronous loop]) on the same clouds"""
    out = []
    for fs, pipe in ((1, 0), (2, 0)) + (((2, -1),) if sync else ()):
        ctx.tune("icp_fused_sums", fs); ctx.tune("icp_pipeline", pipe)
        out.append(result(ctx, cs, ct, **kw))
    ctx.tune("icp_fused_sums", 0); ctx.tune("icp_pipeline", 0)
    return out


def small_pair(n, seed):
    rng = np.random.default_rng(seed)
    tgt = np.ascontiguousarray(rng.normal(0, 5, (3, n)).astype(np.float32))
    src = np.ascontiguousarray((tgt + rng.normal(0, 0.01, (3, n)) + np.array([[0.05], [-0.03], [0.02]])).astype(np.float32))
    return src, tgt


@pytest.fixture(scope="module")
def pair7000(ctx, synth):
    src, tgt = synth.kitti_like_pair(7000, seed_target=81, seed_pair=82)
    cs, ct, far = ctx.cloud(src), ctx.cloud(tgt), ctx.cloud(src + np.float32(1000.0))
    yield src, tgt, cs, ct, far
    cs.free(); ct.free(); far.free()


def test_the_fused_launch_runs_and_the_chain_when_the_grid_is_too_large(ctx, pair7000):
    """which kernels run: no sums pass of its own on the fused path; icp_fused_sums_max_blocks = 1 on a cloud of four workgroups is the
    three-launch chain again — with the same bits; so is a cloud below icp_fused_sums_min"""
    _, _, cs, ct, _ = pair7000
    ctx.tune("nn_method", 1); ctx.tune("prof", 2)
    got = []
    for cap, sums_launches in ((0, 0), (1, 6)):
        ctx.tune("icp_fused_sums_max_blocks", cap); ctx.prof_reset()
        got.append(result(ctx, cs, ct, max_iter=6, eps=0.0))
        assert ctx.prof_get("kabsch_partial")[0] == sums_launches, cap
        assert ctx.prof_get("icp_update")[0] == 6, cap
    assert got[0] == got[1]
    ctx.tune("icp_fused_sums_max_blocks", 0); ctx.tune("icp_fused_sums_min", 0); ctx.prof_reset()      # the default lower bound: 60 000 points
    assert result(ctx, cs, ct, max_iter=6, eps=0.0) == got[0] and ctx.prof_get("kabsch_partial")[0] == 6


@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("n", [1, 3, 4, 5, WG - 1, WG, WG + 1, 2 * WG])
def test_tail_group_and_workgroup_seam(ctx, n, method):
    src, tgt = small_pair(n, 900 + n)
    cs, ct = ctx.cloud(src), ctx.cloud(tgt)
    ctx.tune("nn_method", method)
    for kw in (dict(max_iter=7, eps=0.0), dict(max_iter=2, eps=1e-8, max_corr=0.01)):
        a, b, s = both(ctx, cs, ct, sync=True, **kw)
        assert a == b == s, (n, method, kw)
    if n >= WG - 1:                                   # the same seams with 256-thread workgroups (4 x 256 points each)
        ctx.tune("icp_fused_sums_threads", 256)
        a, b = both(ctx, cs, ct, max_iter=7, eps=0.0)
        assert a == b, (n, method)
    cs.free(); ct.free()


@pytest.mark.parametrize("method", [1, 2])
def test_exit_paths_at_7000(ctx, pair7000, method):
    _, _, cs, ct, far = pair7000
    init = np.eye(4, dtype=np.float32); init[1, 3] = -0.07
    ctx.tune("nn_method", method)
    cases = [(cs, dict(max_iter=0, eps=0.0), None), (cs, dict(max_iter=1, eps=0.0), 1), (cs, dict(max_iter=12, eps=1e-8), None),
             (cs, dict(max_iter=23, eps=0.0), 23), (cs, dict(max_iter=40, eps=1e30), 15),      # converged in the 16th iteration: the launches behind it still arrive
             (cs, dict(max_iter=9, eps=1e-8, max_corr=0.2, init_T=init), None), (far, dict(max_iter=5, eps=1e-8), 0)]
    for cloud, kw, iters in cases:
        a, b, s = both(ctx, cloud, ct, sync=True, **kw)
        assert a == b == s, (kw, method)
        if iters is not None:
            assert a[1] == iters, kw
        if cloud is far:
            assert a[3] == 1                                                                      # the empty exit
        for chunk in (1, 4, 7):
            ctx.tune("icp_chunk", chunk)
            assert result(ctx, cloud, ct, **kw) == a, (kw, method, chunk)
        ctx.tune("icp_chunk", 0)


@pytest.mark.parametrize("threads", [512, 256])
def test_dozens_of_workgroups_meet(ctx, synth, threads):
    n = 40961 - 38                                    # ragged: 20 workgroups of 512 threads, 40 of 256; the last one nearly empty + a float4 tail
    src, tgt = synth.kitti_like_pair(n, seed_target=91, seed_pair=92)
    cs, ct = ctx.cloud(src), ctx.cloud(tgt)
    ctx.tune("icp_fused_sums_threads", threads)
    for method in (1, 2):
        ctx.tune("nn_method", method)
        a, b = both(ctx, cs, ct, max_iter=8, eps=0.0)
        assert a == b and a[1] == 8, (threads, method)
    cs.free(); ct.free()


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_source_points(ctx, pair7000, bad):
    src, _, _, ct, _ = pair7000
    s = src.copy(); s[0, 3] = bad; s[2, 4101] = bad; s[1, 6999] = -bad
    cs = ctx.cloud(s)
    for method in (1, 2):
        ctx.tune("nn_method", method)
        a, b, y = both(ctx, cs, ct, sync=True, max_iter=6, eps=0.0)
        assert a == b == y, (bad, method)
    cs.free()


def test_overflow_exit_is_an_error_on_both_paths(ctx, pcr, pair7000):
    """a kept source beyond the accumulation grid (plan.lim), reached with a huge max_corr: PCR_ERR_STATE from either chain, and the context
    goes on working"""
    src, _, cs_ok, ct, _ = pair7000
    s = src.copy(); s[0, 5000] = 1e12
    cs = ctx.cloud(s)
    ctx.tune("nn_method", 1)
    for fs in (1, 2):
        ctx.tune("icp_fused_sums", fs)
        with pytest.raises(pcr.PcrError, match="target extents"):
            ctx.icp_point2point(cs, ct, max_corr=3e38, max_iter=5, eps=0.0)
    a, b = both(ctx, cs_ok, ct, max_iter=3, eps=0.0)
    assert a == b
    cs.free()


def test_counter_keeps_step_across_launches_of_different_grids(ctx, synth, pair7000):
    """the barrier's counter is never reset: 40 000 points, then 5 points, then a loop that stops early (its later launches only arrive), then
    7 000 on the same context"""
    _, _, cs7, ct7, _ = pair7000
    src, tgt = synth.kitti_like_pair(40000, seed_target=93, seed_pair=94)
    cb, tb = ctx.cloud(src), ctx.cloud(tgt)
    s5, t5 = small_pair(5, 77)
    c5, k5 = ctx.cloud(s5), ctx.cloud(t5)
    ctx.tune("nn_method", 1)
    runs = (((cb, tb), dict(max_iter=5, eps=0.0)), ((c5, k5), dict(max_iter=3, eps=0.0)), ((cs7, ct7), dict(max_iter=40, eps=1e30)),
            ((cs7, ct7), dict(max_iter=12, eps=1e-8)))
    ctx.tune("icp_fused_sums", 2)
    ref = [result(ctx, *clouds, **kw) for clouds, kw in runs]
    ctx.tune("icp_fused_sums", 1)
    for _ in range(2):
        assert [result(ctx, *clouds, **kw) for clouds, kw in runs] == ref
    cb.free(); tb.free(); c5.free(); k5.free()
