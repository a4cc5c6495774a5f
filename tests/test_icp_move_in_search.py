"""The chain search -> sums + solve of single-rank exhaustive ICP loops (tune icp_move_in_search): the search of iteration k + 1 moves the
working cloud by the Rd, td of solve k while it loads its queries and seeds itself on the way (csrc/nn1_sphere.hpp, MV); the sums + solve launch
(csrc/kabsch.hip icp_sums_solve_kernel) hands the reduce and the solve to the workgroup that arrives last, by a ticket — no grid barrier.  The sums are
exact integers, the solve is the same function of the same row and the move and the seed use the same unfused expressions, so EVERY case here compares
bit for bit — pose as uint32, iters_run, converged, empty_pairs, last_pairs, the bits of last_loss — against the synchronous host loop
(icp_pipeline = -1) and against icp_move_in_search = 2 in the same process (the fused sums + move launch; some cases the three-launch chain as well).
STRACK3 is forced onto a target of 9 000 points (nn1_sphere = 1: the working cloud is still sorted from 4 096 points on, so `orig` exists there), and
icp_fused_sums_min = 1 lets every source size take the route.  Which chain ran is asserted through Context.icp_last_chain()."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

NT = 9000
TUNES = ("icp_move_in_search", "icp_fused_sums", "icp_fused_sums_min", "icp_pipeline", "icp_chunk", "nn_method", "nn1_sphere", "nn1_sphere_qg", "nn1_s3_transposed",
         "icp_sums_solve_threads", "nn1_variant")
MOVE, FUSED_SUMS, THREE_LAUNCH, SYNC = 4, 3, 2, 0           # Context.icp_last_chain()


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
    """(src, tgt, device target): a 9 000-point pair; sources of every size are prefixes of src (a random subset of the target, moved and jittered)"""
    src, tgt = synth.kitti_like_pair(NT, seed_target=181, seed_pair=182)
    ct = ctx.cloud(tgt)
    yield src, tgt, ct
    ct.free()


def result(ctx, cs, ct, **kw):
    T, st = ctx.icp_point2point(cs, ct, **kw)
    return (T.view(np.uint32).tobytes(), st["iters_run"], st["converged"], st["empty_pairs"], st["last_pairs"], np.float32(st["last_loss"]).tobytes())


def arms(ctx, cs, ct, three=False, want=MOVE, **kw):
    """the move-in-search chain, the chain without it[, the three-launch chain], the synchronous loop: all equal; returns the common result"""
    ctx.tune("icp_move_in_search", 1)
    a = result(ctx, cs, ct, **kw)
    ran = kw.get("max_iter", 20) > 0                            # (the chain is chosen behind the first search: a loop without one never chooses)
    assert ctx.icp_last_chain() == (want if ran else FUSED_SUMS), kw
    assert not ran or ctx.mfma_check()["last_nn1_kernel"] == "strack3"
    ctx.tune("icp_move_in_search", 2)
    b = result(ctx, cs, ct, **kw)
    assert ctx.icp_last_chain() == FUSED_SUMS
    assert a == b, ("against icp_move_in_search = 2", kw)
    if three:
        ctx.tune("icp_fused_sums", 2)
        c = result(ctx, cs, ct, **kw)
        assert ctx.icp_last_chain() == THREE_LAUNCH
        ctx.tune("icp_fused_sums", 0)
        assert a == c, ("against the three-launch chain", kw)
    ctx.tune("icp_pipeline", -1)
    s = result(ctx, cs, ct, **kw)
    assert ctx.icp_last_chain() == SYNC
    ctx.tune("icp_pipeline", 0); ctx.tune("icp_move_in_search", 0)
    assert a == s, ("against the synchronous loop", kw)
    return a


# ---- host logic: the dispatch predicate (no GPU)
def test_route_predicate(pcr):
    """pcr_icp_move_route: one rank, the tune, the fused-sums switch and lower bound, the transposed form, ONE slice of level-0 super-tiles"""
    on = dict(move_in_search=1)
    assert pcr.icp_move_route(120000, 120000, **on)
    assert pcr.icp_move_route(120000, 120000) == pcr.icp_move_route(120000, 120000, move_in_search=0)        # auto: whatever the library's default is ...
    assert not pcr.icp_move_route(120000, 120000, move_in_search=2)                                             # ... but 2 is off
    for nranks in (0, 2, 8):
        assert not pcr.icp_move_route(120000, 120000, nranks=nranks, **on)
    assert not pcr.icp_move_route(120000, 120000, fused_sums=2, **on)                                           # icp_fused_sums = 2: the three-launch chain
    assert pcr.icp_move_route(120000, 120000, fused_sums=1, **on)
    assert pcr.icp_move_route(60000, 120000, **on) and not pcr.icp_move_route(59999, 120000, **on)              # icp_fused_sums_min, default 60 000
    assert pcr.icp_move_route(1, 9000, fused_sums_min=1, **on) and not pcr.icp_move_route(0, 9000, fused_sums_min=1, **on)
    assert not pcr.icp_move_route(4095, 9000, fused_sums_min=4096, **on) and pcr.icp_move_route(4096, 9000, fused_sums_min=4096, **on)
    assert not pcr.icp_move_route(120000, 120000, s3_transposed=2, **on) and pcr.icp_move_route(120000, 120000, s3_transposed=1, **on)
    # slices: one level-0 super-tile of 131 072 records is always one slice; more are cut into slices unless the launch already has ~1 024 workgroups
    assert pcr.icp_move_route(120000, 131072, **on) and not pcr.icp_move_route(120000, 131073, **on)
    assert not pcr.icp_move_route(20000, 300000, **on) and not pcr.icp_move_route(120000, 300000, **on)
    assert pcr.icp_move_route(262144, 300000, **on)                                                             # (2 048 query blocks: nothing to slice for)
    assert pcr.icp_move_route(120000, 300000, sphere_l0_per_slice=3, **on) and not pcr.icp_move_route(120000, 300000, sphere_l0_per_slice=2, **on)
    assert pcr.icp_move_route(120000, 300000, sphere_blocks=1, **on)                                            # (as few workgroups as there are query blocks)
    for qg in (1, 2, 4):
        assert pcr.icp_move_route(120000, 120000, sphere_qg=qg, **on) and not pcr.icp_move_route(120000, 300000, sphere_qg=qg, **on)


# ---- GPU
@gpu
def test_the_tune_selects_the_chain(ctx, scan):
    src, _, ct = scan
    cs = ctx.cloud(src[:, :5000])
    ctx.tune("prof", 2)
    got = {}
    for v, chain, sums in ((1, MOVE, 0), (2, FUSED_SUMS, 0)):
        ctx.tune("icp_move_in_search", v); ctx.prof_reset()
        got[v] = result(ctx, cs, ct, max_iter=6, eps=0.0)
        assert ctx.icp_last_chain() == chain
        # prof = 2 still works: one search and one icp_update per iteration on either chain, no sums pass of its own, and the only "transform" is the
        # call's clone + initial transform
        assert ctx.prof_get("nn1_brute")[0] == 6 and ctx.prof_get("icp_update")[0] == 6 and ctx.prof_get("kabsch_partial")[0] == sums and ctx.prof_get("transform")[0] == 1
    ctx.tune("prof", 0)
    assert got[1] == got[2] and got[1][1] == 6
    ctx.tune("icp_move_in_search", 1); ctx.tune("icp_fused_sums", 2)            # icp_fused_sums = 2 still means the three-launch chain
    assert result(ctx, cs, ct, max_iter=6, eps=0.0) == got[1] and ctx.icp_last_chain() == THREE_LAUNCH
    ctx.tune("icp_fused_sums", 0); ctx.tune("icp_fused_sums_min", 0)            # below the default lower bound of 60 000 points: not this chain
    assert result(ctx, cs, ct, max_iter=6, eps=0.0) == got[1] and ctx.icp_last_chain() == THREE_LAUNCH
    ctx.tune("icp_fused_sums_min", 1); ctx.tune("nn_method", 2)                 # a grid loop never takes it
    ctx.tune("icp_move_in_search", 1)
    result(ctx, cs, ct, max_iter=6, eps=0.0)
    assert ctx.icp_last_chain() != MOVE
    cs.free()


@gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097, 10001])
def test_source_sizes(ctx, synth, scan, n):
    """wave, workgroup and 4-per-thread edges of both kernels, the padded tail group, and the size from which the working cloud is sorted"""
    src, _, ct = scan
    if n > NT:                                                 # (more sources than targets: a second draw from the same scan behind the first)
        src = np.concatenate([src, synth.kitti_like_pair(NT, seed_target=181, seed_pair=183)[0]], axis=1)
    cs = ctx.cloud(np.ascontiguousarray(src[:, :n]))
    a = arms(ctx, cs, ct, three=n in (1, 129, 4096, 10001), max_iter=9, eps=0.0)
    assert a[1] == 9
    for threads in (128, 256):                                 # the other geometries of the sums + solve launch
        ctx.tune("icp_sums_solve_threads", threads); ctx.tune("icp_move_in_search", 1)
        assert result(ctx, cs, ct, max_iter=9, eps=0.0) == a and ctx.icp_last_chain() == MOVE, threads
    cs.free()


@gpu
def test_max_iter_and_convergence(ctx, scan):
    src, _, ct = scan
    cs = ctx.cloud(src[:, :5003])
    for it in (0, 1, 2, 3, 4, 5, 9):                           # odd and even (the two state buffers), across the chunk of 4
        a = arms(ctx, cs, ct, max_iter=it, eps=0.0)
        assert a[1] == it
        if it in (3, 9):
            for chunk in (1, 7):
                ctx.tune("icp_chunk", chunk); ctx.tune("icp_move_in_search", 1)
                assert result(ctx, cs, ct, max_iter=it, eps=0.0) == a, (it, chunk)
            ctx.tune("icp_chunk", 0)
    # converged in the 16th iteration: the launches enqueued behind it move nothing — the pose is the synchronous loop's
    a = arms(ctx, cs, ct, three=True, max_iter=40, eps=1e30)
    assert a[1] == 15 and a[2] == 1
    init = np.eye(4, dtype=np.float32); init[1, 3] = -0.07
    arms(ctx, cs, ct, max_iter=12, eps=1e-8, max_corr=0.2, init_T=init)
    cs.free()


@gpu
def test_exit_conditions(ctx, pcr, scan):
    src, _, ct = scan
    n = 5000
    cs = ctx.cloud(src[:, :n])
    a = arms(ctx, cs, ct, max_iter=5, eps=1e-8, max_corr=1e-30)                  # a max_corr below every distance: no pair in the first iteration
    assert a[3] == 1 and a[1] == 0
    cs.free()
    s = src[:, :n].copy(); s[0, 2500] = 1e12                                      # one kept source beyond plan.lim: PCR_ERR_STATE from every chain
    cs = ctx.cloud(s)
    for v in (1, 2):
        ctx.tune("icp_move_in_search", v)
        with pytest.raises(pcr.PcrError, match="target extents"):
            ctx.icp_point2point(cs, ct, max_corr=3e38, max_iter=5, eps=0.0)
    cs.free()
    for bad in (np.nan, np.inf):                                                  # NaN / inf coordinates at the wave edges and the last point
        s = src[:, :n].copy(); s[0, 0] = bad; s[1, 31] = bad; s[2, 32] = -bad; s[0, n - 1] = bad
        cs = ctx.cloud(s)
        arms(ctx, cs, ct, max_iter=6, eps=0.0)
        cs.free()


@gpu
def test_duplicates_and_ties(ctx, scan):
    _, tgt, _ = scan
    dup = np.ascontiguousarray(np.concatenate([tgt[:, :4500], tgt[:, :4500]], axis=1))          # every target point twice: the lower index wins
    ct = ctx.cloud(dup)
    cs = ctx.cloud(dup)                                                                        # source == target: distance 0 everywhere
    a = arms(ctx, cs, ct, three=True, max_iter=5, eps=0.0)
    assert a[4] == NT
    cs.free()
    cs = ctx.cloud(np.ascontiguousarray(dup[:, ::3] + np.float32(0.01)))
    arms(ctx, cs, ct, max_iter=5, eps=0.0)
    cs.free(); ct.free()


@gpu
def test_reuse_of_one_context(ctx, scan):
    """stale keys and seeds of an earlier loop do not leak: A, B (same size, then another size), A again — each equal to the synchronous loop's"""
    src, _, ct = scan
    a_np, b_np, c_np = src[:, :5000], np.ascontiguousarray(src[:, 3000:8000]), np.ascontiguousarray(src[:, 100:4200])
    ca, cb, cc = ctx.cloud(a_np), ctx.cloud(b_np), ctx.cloud(c_np)
    kw = dict(max_iter=7, eps=0.0)
    ctx.tune("icp_pipeline", -1)
    ref = [result(ctx, c, ct, **kw) for c in (ca, cb, cc)]
    ctx.tune("icp_pipeline", 0); ctx.tune("icp_move_in_search", 1)
    for _ in range(2):
        for k in (0, 1, 0, 2, 0):
            assert result(ctx, (ca, cb, cc)[k], ct, **kw) == ref[k] and ctx.icp_last_chain() == MOVE, k
    ca.free(); cb.free(); cc.free()


@gpu
@pytest.mark.parametrize("qg", [1, 2, 4])
def test_every_query_group_count(ctx, scan, qg):
    """who stores a moved query differs: both half-lanes own query n with one group per wave, one lane each with two or four"""
    src, _, ct = scan
    ctx.tune("nn1_sphere_qg", qg)
    for n in (129, 8999):
        cs = ctx.cloud(src[:, :n])
        arms(ctx, cs, ct, max_iter=9, eps=0.0)
        cs.free()


@gpu
def test_rows_form_falls_back(ctx, scan):
    """nn1_s3_transposed = 2 (one ballot per accumulator) is not built with the move: the whole call keeps the fused sums + move launch, same bits"""
    src, _, ct = scan
    cs = ctx.cloud(src[:, :5000])
    ctx.tune("icp_move_in_search", 1)
    want = result(ctx, cs, ct, max_iter=6, eps=0.0)
    assert ctx.icp_last_chain() == MOVE
    ctx.tune("nn1_s3_transposed", 2)
    arms(ctx, cs, ct, want=FUSED_SUMS, max_iter=6, eps=0.0)
    ctx.tune("icp_move_in_search", 1)
    assert result(ctx, cs, ct, max_iter=6, eps=0.0) == want and ctx.icp_last_chain() == FUSED_SUMS
    cs.free()


@gpu
def test_multi_slice_target_falls_back(ctx):
    """300 000 target points are three level-0 super-tiles and the search of 20 000 queries three slices: several workgroups read a query block, nobody
    may overwrite it — the chain is not taken (STRACK3 still is), and the bits are the synchronous loop's"""
    rng = np.random.default_rng(77)
    tgt = np.ascontiguousarray(rng.uniform(-40, 40, (3, 300000)).astype(np.float32))
    pick = rng.permutation(300000)[:20000]
    src = np.ascontiguousarray((tgt[:, pick] + rng.normal(0, 0.01, (3, 20000)) + np.array([[0.05], [-0.03], [0.02]])).astype(np.float32))
    ct, cs = ctx.cloud(tgt), ctx.cloud(src)
    arms(ctx, cs, ct, want=FUSED_SUMS, max_iter=4, eps=0.0)
    assert ctx.mfma_check()["last_nn1_kernel"] == "strack3"
    cs.free(); ct.free()
