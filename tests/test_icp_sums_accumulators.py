"""The sums + solve launch of the chain search -> sums + solve (csrc/kabsch.hip icp_sums_solve_kernel): a workgroup's limb totals leave it as
int64 atomic adds into a few replicated accumulator rows, the workgroup that arrives last adds the replicas, propagates the carries as integers, solves,
and writes the zeros back.  The sums are exact integers whatever the grouping, so EVERY case compares bit for bit — pose as uint32, iters_run, converged,
empty_pairs, last_pairs, the bits of last_loss — against the synchronous host loop (icp_pipeline = -1) and against the three-launch chain
(icp_fused_sums = 2), for every built geometry: pairs per thread 1 / 2 / 4 (icp_sums_solve_pairs) x threads 256 / 512 (icp_sums_solve_threads).  The
set-up is that of test_icp_move_in_search.py: STRACK3 forced onto a target of 9 000 points (nn1_sphere = 1), icp_fused_sums_min = 1 so that every source
size takes the route; which chain ran is asserted through Context.icp_last_chain()."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

NT = 9000
TUNES = ("icp_move_in_search", "icp_fused_sums", "icp_fused_sums_min", "icp_pipeline", "icp_chunk", "nn_method", "nn1_sphere", "icp_sums_solve_threads",
         "icp_sums_solve_pairs")
MOVE, THREE_LAUNCH, SYNC = 4, 2, 0                          # Context.icp_last_chain()
GEOMETRIES = [(p, t) for t in (256, 512) for p in (1, 2, 4)]


@pytest.fixture(scope="module")
def ctx(pcr):
    c = pcr.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _defaults(request):
    if "ctx" not in request.fixturenames:
        yield
        return
    ctx = request.getfixturevalue("ctx")
    ctx.tune("nn_method", 1); ctx.tune("nn1_sphere", 1); ctx.tune("icp_fused_sums_min", 1)
    yield
    for k in TUNES:
        ctx.tune(k, 0)


@pytest.fixture(scope="module")
def scan(ctx, synth):
    """(src, tgt, device target): a 9 000-point pair and 45 000 sources for it (five draws from the same scan); sources of every size are prefixes"""
    tgt = synth.kitti_like_pair(NT, seed_target=181, seed_pair=182)[1]
    src = np.ascontiguousarray(np.concatenate([synth.kitti_like_pair(NT, seed_target=181, seed_pair=182 + k)[0] for k in range(5)], axis=1))
    ct = ctx.cloud(tgt)
    yield src, tgt, ct
    ct.free()


def result(ctx, cs, ct, **kw):
    T, st = ctx.icp_point2point(cs, ct, **kw)
    return (T.view(np.uint32).tobytes(), st["iters_run"], st["converged"], st["empty_pairs"], st["last_pairs"], np.float32(st["last_loss"]).tobytes())


def references(ctx, cs, ct, **kw):
    """the synchronous loop and the three-launch chain: equal; returns the common result"""
    ctx.tune("icp_move_in_search", 0); ctx.tune("icp_pipeline", -1)
    s = result(ctx, cs, ct, **kw)
    assert ctx.icp_last_chain() == SYNC
    ctx.tune("icp_pipeline", 0); ctx.tune("icp_fused_sums", 2)
    c = result(ctx, cs, ct, **kw)
    assert ctx.icp_last_chain() == THREE_LAUNCH
    ctx.tune("icp_fused_sums", 0)
    assert s == c, ("the three-launch chain against the synchronous loop", kw)
    return s


def accumulated(ctx, cs, ct, geometry, **kw):
    """the chain search -> sums + solve at one geometry of the sums + solve launch"""
    ctx.tune("icp_move_in_search", 1); ctx.tune("icp_sums_solve_pairs", geometry[0]); ctx.tune("icp_sums_solve_threads", geometry[1])
    a = result(ctx, cs, ct, **kw)
    assert ctx.icp_last_chain() == MOVE, (geometry, kw)
    return a


def every_geometry(ctx, cs, ct, **kw):
    want = references(ctx, cs, ct, **kw)
    for g in GEOMETRIES:
        assert accumulated(ctx, cs, ct, g, **kw) == want, (g, kw)
    return want


@gpu
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 5000, 40000])
def test_source_sizes(ctx, scan, n):
    """fewer workgroups than replicas (one at the small sizes), many more at 40 000 (157 of 256 x 1 pairs); wave and workgroup edges; sizes that are
    no multiple of the pairs per thread (the guarded tail group)"""
    src, _, ct = scan
    cs = ctx.cloud(np.ascontiguousarray(src[:, :n]))
    a = every_geometry(ctx, cs, ct, max_iter=9, eps=0.0)
    assert a[1] == 9 and (n < 63 or a[4] > 0)
    cs.free()


@gpu
def test_mixed_signs(ctx, scan):
    """a pair centred on the origin: coordinate and product limb totals take both signs, carries go negative"""
    src, tgt, _ = scan
    mid = tgt.astype(np.float64).mean(axis=1, keepdims=True)
    ct = ctx.cloud(np.ascontiguousarray((tgt - mid).astype(np.float32)))
    s = np.ascontiguousarray((src[:, :7001] - mid).astype(np.float32))
    assert (s.min(axis=1) < 0).all() and (s.max(axis=1) > 0).all()
    cs = ctx.cloud(s)
    a = every_geometry(ctx, cs, ct, max_iter=9, eps=0.0)
    assert a[4] > 700
    cs.free(); ct.free()


@gpu
def test_limb_range(ctx, scan):
    """the top limbs (a pair 1 000 m off the origin: the same residuals at the identity, sums a thousand times the scene's) and the low ones (the scene
    scaled to 1e-3)"""
    src, tgt, _ = scan
    off = np.array([[1000.0], [1000.0], [0.0]])
    ct = ctx.cloud(np.ascontiguousarray((tgt + off).astype(np.float32)))
    cs = ctx.cloud(np.ascontiguousarray((src[:, :6001] + off).astype(np.float32)))
    a = every_geometry(ctx, cs, ct, max_iter=7, eps=0.0)
    assert a[4] > 600
    cs.free(); ct.free()
    ct = ctx.cloud(np.ascontiguousarray((tgt * 1e-3).astype(np.float32)))
    cs = ctx.cloud(np.ascontiguousarray((src[:, :6001] * 1e-3).astype(np.float32)))
    a = every_geometry(ctx, cs, ct, max_iter=7, eps=0.0, max_corr=1e-6)
    assert a[4] > 600
    cs.free(); ct.free()


@gpu
def test_gate(ctx, scan):
    src, tgt, ct = scan
    cs = ctx.cloud(np.ascontiguousarray(src[:, :5000]))
    a = every_geometry(ctx, cs, ct, max_iter=5, eps=1e-8, max_corr=1e-30)          # a max_corr below every distance: no pair, the empty exit
    assert a[3] == 1 and a[1] == 0
    cs.free()
    s = src[:, :1500].copy(); s[2] += 500.0; s[:, 777] = tgt[:, 4321] + np.float32(0.01)     # exactly one pair within max_corr
    cs = ctx.cloud(np.ascontiguousarray(s))
    a = every_geometry(ctx, cs, ct, max_iter=1, eps=0.0)
    assert a[4] == 1
    every_geometry(ctx, cs, ct, max_iter=4, eps=0.0)
    cs.free()


@gpu
def test_duplicates_and_the_last_kept_key(ctx, scan):
    """duplicated targets (the lower index wins) and duplicated sources, among them the last point: the loss is that of the kept pair with the highest
    original index — the accumulators' atomic max — and equal keys meet in it"""
    src, tgt, _ = scan
    dup = np.ascontiguousarray(np.concatenate([tgt[:, :4500], tgt[:, :4500]], axis=1))
    ct = ctx.cloud(dup)
    cs = ctx.cloud(dup)                                                                       # source == target: distance 0 everywhere
    a = every_geometry(ctx, cs, ct, max_iter=5, eps=0.0)
    assert a[4] == NT
    cs.free()
    s = np.ascontiguousarray(np.concatenate([src[:, :2500], src[:, :2500], src[:, 2499:2500]], axis=1))
    cs = ctx.cloud(s)
    every_geometry(ctx, cs, ct, max_iter=5, eps=0.0)
    cs.free(); ct.free()


@gpu
def test_overflow_then_a_clean_call(ctx, pcr, scan):
    """a kept source point beyond the accumulation grid is PCR_ERR_STATE; the accumulators are cleared in front of the next call, which is clean"""
    src, _, ct = scan
    good = ctx.cloud(np.ascontiguousarray(src[:, :5000]))
    s = src[:, :5000].copy(); s[0, 2500] = 1e12
    bad = ctx.cloud(s)
    want = references(ctx, good, ct, max_iter=6, eps=0.0)
    for g in GEOMETRIES:
        ctx.tune("icp_move_in_search", 1); ctx.tune("icp_sums_solve_pairs", g[0]); ctx.tune("icp_sums_solve_threads", g[1])
        with pytest.raises(pcr.PcrError, match="target extents"):
            ctx.icp_point2point(bad, ct, max_corr=3e38, max_iter=5, eps=0.0)
        assert accumulated(ctx, good, ct, g, max_iter=6, eps=0.0) == want, g
        assert accumulated(ctx, good, ct, g, max_iter=6, eps=0.0) == want, g
    good.free(); bad.free()


@gpu
def test_reuse_of_one_context(ctx, scan):
    """nothing of a call stays in the accumulators: three calls of different sizes, then the first again — at every geometry, and across geometries"""
    src, _, ct = scan
    clouds = [ctx.cloud(np.ascontiguousarray(src[:, lo:hi])) for lo, hi in ((0, 5000), (3000, 3700), (100, 20100))]
    kw = dict(max_iter=7, eps=0.0)
    ref = [references(ctx, c, ct, **kw) for c in clouds]
    for g in GEOMETRIES:
        for k in (0, 1, 2, 0):
            assert accumulated(ctx, clouds[k], ct, g, **kw) == ref[k], (g, k)
    for c in clouds:
        c.free()


@gpu
def test_max_iter_and_convergence_inside_a_chunk(ctx, scan):
    src, _, ct = scan
    cs = ctx.cloud(np.ascontiguousarray(src[:, :5003]))
    for it in (1, 2):
        a = every_geometry(ctx, cs, ct, max_iter=it, eps=0.0)
        assert a[1] == it
    # converged after 15 of 40 iterations, inside a chunk of 2 and of 4: the launches enqueued behind the stop add nothing and leave the zeros alone
    for chunk in (1, 2, 4):
        ctx.tune("icp_chunk", chunk)
        a = every_geometry(ctx, cs, ct, max_iter=40, eps=1e30)
        assert a[1] == 15 and a[2] == 1, chunk
        assert every_geometry(ctx, cs, ct, max_iter=3, eps=0.0)[1] == 3, chunk       # ... and the next call starts from zeros
    cs.free()
