"""The chain search -> sums of single-rank exhaustive ICP loops (tune icp_solve_in_search; Context.icp_last_chain() == 5): the sums launch
(csrc/kabsch.hip icp_sums_kernel) only adds a workgroup's limb totals into one of TWO sets of accumulator rows, and the search of iteration k + 1
(csrc/nn1_sphere.hpp, SV) reduces them, solves and steps the loop's state in every workgroup before it moves the cloud (csrc/icp_finish.hpp); one wave
behind the last sums launch of a call does the same (icp_finish_kernel).  No ticket, no fence: every dependency is a launch boundary.  The back half is
the text chain 4 runs, so EVERY case compares bit for bit — pose as uint32, iters_run, converged, empty_pairs, last_pairs, the bits of last_loss —
against the synchronous host loop (icp_pipeline = -1) and against chain 4 (icp_move_in_search = 1 with the new tune at 0), and asserts which chain ran.
Set-up as in test_icp_move_in_search.py: STRACK3 forced onto a 9 000-point target, icp_fused_sums_min = 1, sources are prefixes of draws of one scan."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

NT = 9000
TUNES = ("icp_solve_in_search", "icp_move_in_search", "icp_fused_sums", "icp_fused_sums_min", "icp_pipeline", "icp_chunk", "icp_host_snapshots", "nn_method",
         "nn1_sphere", "icp_sums_solve_threads", "icp_sums_solve_pairs", "grid_stats")
SOLVE, MOVE, FUSED_SUMS, THREE_LAUNCH, SYNC = 5, 4, 3, 2, 0           # Context.icp_last_chain()


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
    """(src, tgt, device target): a 9 000-point target and 45 000 source points — five draws of the same scan, one behind the other"""
    src, tgt = synth.kitti_like_pair(NT, seed_target=181, seed_pair=182)
    more = [synth.kitti_like_pair(NT, seed_target=181, seed_pair=s)[0] for s in (183, 184, 185, 186)]
    src = np.ascontiguousarray(np.concatenate([src] + more, axis=1))
    ct = ctx.cloud(tgt)
    yield src, tgt, ct
    ct.free()


def result(ctx, cs, ct, **kw):
    T, st = ctx.icp_point2point(cs, ct, **kw)
    return (T.view(np.uint32).tobytes(), st["iters_run"], st["converged"], st["empty_pairs"], st["last_pairs"], np.float32(st["last_loss"]).tobytes())


def chain(ctx, which, cs, ct, **kw):
    """one call on the chain `which` (tunes set for it and put back), its chain number asserted"""
    ran = kw.get("max_iter", 20) > 0                            # (the chain is chosen behind the first search: a loop without one never chooses)
    if which == SOLVE: ctx.tune("icp_solve_in_search", 1)
    elif which == MOVE: ctx.tune("icp_move_in_search", 1)
    elif which == FUSED_SUMS: ctx.tune("icp_move_in_search", 2)
    elif which == THREE_LAUNCH: ctx.tune("icp_fused_sums", 2)
    else: ctx.tune("icp_pipeline", -1)
    r = result(ctx, cs, ct, **kw)
    assert ctx.icp_last_chain() == (which if ran or which == SYNC else FUSED_SUMS), (which, kw)
    for k in ("icp_solve_in_search", "icp_move_in_search", "icp_fused_sums", "icp_pipeline"):
        ctx.tune(k, 0)
    return r


def reference(ctx, cs, ct, **kw):
    """the synchronous loop and chain 4, equal; returns the common result"""
    s, m = chain(ctx, SYNC, cs, ct, **kw), chain(ctx, MOVE, cs, ct, **kw)
    assert s == m, ("chain 4 against the synchronous loop", kw)
    return s


# ---- host logic: the selection (no GPU)
def test_route_predicate(pcr):
    """pcr_icp_solve_route: chain 4's conditions, and icp_solve_in_search = 1, or both tunes at auto and the library's default"""
    big = (120000, 120000)
    auto = pcr.icp_solve_in_search_auto()
    assert pcr.icp_solve_route(*big, solve_in_search=1)
    assert pcr.icp_solve_route(*big, solve_in_search=1, move_in_search=1)
    assert not pcr.icp_solve_route(*big, solve_in_search=2) and not pcr.icp_solve_route(*big, solve_in_search=2, move_in_search=1)
    assert not pcr.icp_solve_route(*big, move_in_search=1)                       # icp_move_in_search = 1 alone keeps chain 4 ...
    assert pcr.icp_move_route(*big, move_in_search=1)
    assert pcr.icp_solve_route(*big) == (big[0] <= auto and pcr.icp_move_route(*big))       # ... both auto: whatever the library's default is
    assert pcr.icp_solve_route(*big) == pcr.icp_solve_route(*big, solve_in_search=0, move_in_search=0)
    if auto:                                                                     # (on up to a source size: the search's workgroups in one round)
        assert pcr.icp_solve_route(auto, 131072) and not pcr.icp_solve_route(auto + 1, 131072)
        assert pcr.icp_solve_route(auto + 1, 131072, solve_in_search=1) and pcr.icp_move_route(auto + 1, 131072)
    # only where chain 4 would be taken: every condition of pcr_icp_move_route
    on = dict(solve_in_search=1)
    assert not pcr.icp_solve_route(*big, move_in_search=2, **on)
    for nranks in (0, 2, 8):
        assert not pcr.icp_solve_route(*big, nranks=nranks, **on)
    assert not pcr.icp_solve_route(*big, fused_sums=2, **on) and pcr.icp_solve_route(*big, fused_sums=1, **on)
    assert pcr.icp_solve_route(60000, 120000, **on) and not pcr.icp_solve_route(59999, 120000, **on)
    assert pcr.icp_solve_route(1, 9000, fused_sums_min=1, **on) and not pcr.icp_solve_route(0, 9000, fused_sums_min=1, **on)
    assert not pcr.icp_solve_route(*big, s3_transposed=2, **on)
    assert pcr.icp_solve_route(120000, 131072, **on) and not pcr.icp_solve_route(120000, 131073, **on)       # one slice of level-0 super-tiles
    for n_src, n_tgt, kw in ((120000, 120000, {}), (20000, 300000, {}), (262144, 300000, {}), (120000, 300000, dict(sphere_l0_per_slice=3)), (59999, 120000, {})):
        for mv in (0, 1, 2):
            assert pcr.icp_solve_route(n_src, n_tgt, move_in_search=mv, **kw, **on) == pcr.icp_move_route(n_src, n_tgt, move_in_search=mv, **kw)


# ---- GPU
@gpu
def test_the_tunes_select_the_chain(ctx, pcr, scan):
    src, _, ct = scan
    cs = ctx.cloud(src[:, :5000])
    kw = dict(max_iter=6, eps=0.0)
    want = reference(ctx, cs, ct, **kw)
    ctx.tune("prof", 2); ctx.prof_reset()
    assert chain(ctx, SOLVE, cs, ct, **kw) == want
    # one search and one sums launch per iteration, one finishing launch per call, no sums pass or move of their own
    assert ctx.prof_get("nn1_brute")[0] == 6 and ctx.prof_get("icp_update")[0] == 6 and ctx.prof_get("icp_finish")[0] == 1
    assert ctx.prof_get("kabsch_partial")[0] == 0 and ctx.prof_get("transform")[0] == 1
    ctx.tune("prof", 0)
    assert result(ctx, cs, ct, **kw) == want                                     # both auto: the library's default
    assert ctx.icp_last_chain() == (SOLVE if 5000 <= pcr.icp_solve_in_search_auto() else MOVE)
    ctx.tune("icp_solve_in_search", 1); ctx.tune("icp_move_in_search", 1)
    assert result(ctx, cs, ct, **kw) == want and ctx.icp_last_chain() == SOLVE
    ctx.tune("icp_solve_in_search", 2)
    assert result(ctx, cs, ct, **kw) == want and ctx.icp_last_chain() == MOVE
    ctx.tune("icp_solve_in_search", 1); ctx.tune("icp_move_in_search", 2)      # where chain 4 would not be taken, neither is this one
    assert result(ctx, cs, ct, **kw) == want and ctx.icp_last_chain() == FUSED_SUMS
    ctx.tune("icp_move_in_search", 0); ctx.tune("icp_fused_sums", 2)
    assert result(ctx, cs, ct, **kw) == want and ctx.icp_last_chain() == THREE_LAUNCH
    ctx.tune("icp_fused_sums", 0); ctx.tune("nn_method", 2)                     # a grid loop never takes it
    result(ctx, cs, ct, **kw)
    assert ctx.icp_last_chain() not in (SOLVE, MOVE)
    cs.free()


@gpu
@pytest.mark.parametrize("n", [1, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097, 10001])
def test_source_sizes(ctx, scan, n):
    """wave and workgroup edges of the search (128 queries a workgroup): one workgroup that solves and publishes, the first that does not publish, surplus
    waves that stay for the barrier, and the size from which the working cloud is sorted"""
    src, _, ct = scan
    cs = ctx.cloud(np.ascontiguousarray(src[:, :n]))
    kw = dict(max_iter=9, eps=0.0)
    want = reference(ctx, cs, ct, **kw)
    assert want[1] == 9
    for snaps in (0, 2):
        ctx.tune("icp_host_snapshots", snaps)
        assert chain(ctx, SOLVE, cs, ct, **kw) == want, snaps
        assert ctx.icp_last_snapshots() == (1 if snaps == 0 else 0)
    cs.free()


@gpu
@pytest.mark.parametrize("n", [511, 512, 513, 1023, 1024, 1025, 40000])
def test_sums_launch_sizes(ctx, scan, n):
    """the workgroup edges of every built geometry of the sums launch (threads x pairs); 40 000 points are 313 workgroups of the search (a solving wave
    other than wave 0) and up to 157 of the sums launch (every replica of a set, many times)"""
    src, _, ct = scan
    cs = ctx.cloud(np.ascontiguousarray(src[:, :n]))
    kw = dict(max_iter=5, eps=0.0)
    want = reference(ctx, cs, ct, **kw)
    for threads in (256, 512):
        for pairs in (1, 2, 4):
            ctx.tune("icp_sums_solve_threads", threads); ctx.tune("icp_sums_solve_pairs", pairs)
            assert chain(ctx, SOLVE, cs, ct, **kw) == want, (threads, pairs)
    cs.free()


@pytest.fixture(scope="module")
def loop_refs(ctx, scan):
    """max_iter -> the synchronous loop's result (= chain 4's) for the 5 003-point source of the loop-control cases; computed once"""
    src, _, ct = scan
    ctx.tune("nn_method", 1); ctx.tune("nn1_sphere", 1); ctx.tune("icp_fused_sums_min", 1)
    cs = ctx.cloud(src[:, :5003])
    refs = {it: reference(ctx, cs, ct, max_iter=it, eps=0.0) for it in range(42)}
    yield cs, refs
    cs.free()


@gpu
@pytest.mark.parametrize("chunk", [1, 2, 4, 8])
def test_loop_control(ctx, scan, loop_refs, chunk):
    """partial chunks, several trips round the ring of four slots, one iteration only (search, sums, finishing launch), none at all — with the state
    written into the host ring by the next chunk's first search and the finishing launch, and with copies and events"""
    _, _, ct = scan
    cs, refs = loop_refs
    ctx.tune("icp_chunk", chunk)
    for snaps in (0, 2):
        ctx.tune("icp_host_snapshots", snaps)
        for it in range(42):
            assert chain(ctx, SOLVE, cs, ct, max_iter=it, eps=0.0) == refs[it], (chunk, snaps, it)
            assert refs[it][1] == it
            assert ctx.icp_last_snapshots() == (1 if snaps == 0 and it > 0 else 0), (chunk, snaps, it)


@gpu
def test_stops(ctx, pcr, scan):
    src, _, ct = scan
    n = 5000
    cs = ctx.cloud(src[:, :n])
    # converged in the 16th iteration, inside a chunk or at its edge: what is enqueued behind it only forwards the stopped state
    kw = dict(max_iter=40, eps=1e30)
    want = reference(ctx, cs, ct, **kw)
    assert want[1] == 15 and want[2] == 1
    for chunk in (1, 3, 4, 5, 8):
        for snaps in (0, 2):
            ctx.tune("icp_chunk", chunk); ctx.tune("icp_host_snapshots", snaps)
            assert chain(ctx, SOLVE, cs, ct, **kw) == want, (chunk, snaps)
    ctx.tune("icp_chunk", 0); ctx.tune("icp_host_snapshots", 0)
    init = np.eye(4, dtype=np.float32); init[1, 3] = -0.07
    kw = dict(max_iter=12, eps=1e-8, max_corr=0.2, init_T=init)
    assert chain(ctx, SOLVE, cs, ct, **kw) == reference(ctx, cs, ct, **kw)
    # a max_corr below every distance: no pair in the first iteration
    kw = dict(max_iter=5, eps=1e-8, max_corr=1e-30)
    want = reference(ctx, cs, ct, **kw)
    assert want[3] == 1 and want[1] == 0
    assert chain(ctx, SOLVE, cs, ct, **kw) == want
    # one kept source beyond the accumulation grid: PCR_ERR_STATE, and a clean call behind it finds zeros in both accumulator sets
    kw = dict(max_iter=7, eps=0.0)
    want = reference(ctx, cs, ct, **kw)
    s = src[:, :n].copy(); s[0, 2500] = 1e12
    cbad = ctx.cloud(s)
    for it in (1, 2, 5):                                                         # (found by the finishing launch, by the second search, inside a chunk)
        ctx.tune("icp_solve_in_search", 1)
        with pytest.raises(pcr.PcrError, match="target extents"):
            ctx.icp_point2point(cbad, ct, max_corr=3e38, max_iter=it, eps=0.0)
        ctx.tune("icp_solve_in_search", 0)
        assert chain(ctx, SOLVE, cs, ct, **kw) == want, it
        assert chain(ctx, MOVE, cs, ct, **kw) == want, it
    cbad.free(); cs.free()


@gpu
def test_reuse_of_one_context(ctx, scan):
    """chains 5, 4, 3, 5 and the three-launch chain in turn on one context — the accumulators are all zero between calls whoever used them — and calls
    behind one that stopped early: no stale ring slot, state slot or accumulator set"""
    src, _, ct = scan
    ca, cb = ctx.cloud(src[:, :5000]), ctx.cloud(np.ascontiguousarray(src[:, 3000:7100]))
    kw = dict(max_iter=7, eps=0.0)
    ref = [reference(ctx, c, ct, **kw) for c in (ca, cb)]
    for _ in range(2):
        for which, k in ((SOLVE, 0), (MOVE, 1), (FUSED_SUMS, 0), (SOLVE, 1), (THREE_LAUNCH, 0), (SOLVE, 0), (SOLVE, 1)):
            assert chain(ctx, which, (ca, cb)[k], ct, **kw) == ref[k], (which, k)
    early = dict(max_iter=40, eps=1e30)
    want_early = reference(ctx, ca, ct, **early)
    for snaps in (0, 2):
        ctx.tune("icp_host_snapshots", snaps)
        for chunk in (1, 4):
            ctx.tune("icp_chunk", chunk)
            assert chain(ctx, SOLVE, ca, ct, **early) == want_early, (snaps, chunk)
            for it in (7, 6):                                                    # odd and even: either state slot and either set comes last
                assert chain(ctx, SOLVE, cb, ct, max_iter=it, eps=0.0) == (ref[1] if it == 7 else chain(ctx, SYNC, cb, ct, max_iter=6, eps=0.0)), (snaps, chunk, it)
            assert chain(ctx, MOVE, ca, ct, **kw) == ref[0], (snaps, chunk)
    ca.free(); cb.free()


@gpu
def test_diagnostics_pass_through(ctx, scan):
    """grid_stats = 1: the search's counters of a loop of two iterations are chain 4's (flagged tiles, evaluated pairs, MFMAs per level)"""
    src, _, ct = scan
    cs = ctx.cloud(src[:, :5000])
    w = {}
    for which in (MOVE, SOLVE):
        ctx.tune("grid_stats", 1)
        r = chain(ctx, which, cs, ct, max_iter=2, eps=0.0)
        w[which] = ([int(v) for v in ctx.nn1_stats()], r)
        ctx.tune("grid_stats", 0)
    assert w[MOVE][1] == w[SOLVE][1]
    assert w[MOVE][0][7] > 0 and w[MOVE][0][6] > 0, w[MOVE][0]
    for word in (2, 3, 6, 7, 8, 9, 10):
        assert w[MOVE][0][word] == w[SOLVE][0][word], (word, w)
    cs.free()
