"""State snapshots of the chain search -> sums + solve without a copy on the stream, and a ticket per replica (csrc/icp.cpp icp_pipelined,
csrc/kabsch.hip icp_sums_solve_kernel).  The launch that ends a chunk of iterations, or the call, stores the state it has just published into a slot of a
pinned host ring itself and then the slot's sequence number (a system-scope release); the host polls the slot two chunks back for that number and reads
the final state from the slot of the last launch.  Tune icp_host_snapshots: 0 = on where the chain is 4, 2 = copies and events as before; tune
icp_ticket_levels: 1 = one arrival counter, 2 = one per accumulator replica and the shared one behind them.  Neither changes any arithmetic, so EVERY case
compares bit for bit — pose as uint32, iters_run, converged, empty_pairs, last_pairs, the bits of last_loss — between the two snapshot modes and against
the synchronous host loop (icp_pipeline = -1); with prof = 1 also the searches enqueued (nn_launches) between the two modes, because the look-back is two
chunks in both.  The set-up is that of test_icp_sums_accumulators.py: STRACK3 forced onto a target of 9 000 points (nn1_sphere = 1, nn_method = 1),
icp_fused_sums_min = 1 so that every source size takes the route.  Chain 4 and Context.icp_last_snapshots() are asserted for every call that runs at
least one iteration; a call of max_iter = 0 enqueues no sums + solve launch, takes no chain at all and keeps the copy (icp_last_snapshots() = 0)."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

NT = 9000
TUNES = ("icp_move_in_search", "icp_fused_sums_min", "icp_pipeline", "icp_chunk", "nn_method", "nn1_sphere", "icp_sums_solve_threads", "icp_sums_solve_pairs",
         "icp_host_snapshots", "icp_ticket_levels", "prof")
MOVE, SYNC = 4, 0                                             # Context.icp_last_chain()
KERNEL, STREAM = 0, 2                                         # tune icp_host_snapshots


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
    ctx.tune("nn_method", 1); ctx.tune("nn1_sphere", 1); ctx.tune("icp_fused_sums_min", 1); ctx.tune("icp_move_in_search", 1)
    yield
    for k in TUNES:
        ctx.tune(k, 0)


def force_route(c):
    c.tune("nn_method", 1); c.tune("nn1_sphere", 1); c.tune("icp_fused_sums_min", 1); c.tune("icp_move_in_search", 1)


@pytest.fixture(scope="module")
def scan(ctx, synth):
    """(src, tgt, device target): a 9 000-point pair and 45 000 sources for it (five draws from the same scan); sources of every size are prefixes"""
    tgt = synth.kitti_like_pair(NT, seed_target=181, seed_pair=182)[1]
    src = np.ascontiguousarray(np.concatenate([synth.kitti_like_pair(NT, seed_target=181, seed_pair=182 + k)[0] for k in range(5)], axis=1))
    ct = ctx.cloud(tgt)
    yield src, tgt, ct
    ct.free()


@pytest.fixture(scope="module")
def five_thousand(ctx, scan):
    cs = ctx.cloud(np.ascontiguousarray(scan[0][:, :5000]))
    yield cs
    cs.free()


def result(c, cs, ct, **kw):
    T, st = c.icp_point2point(cs, ct, **kw)
    return (T.view(np.uint32).tobytes(), st["iters_run"], st["converged"], st["empty_pairs"], st["last_pairs"], np.float32(st["last_loss"]).tobytes()), st["nn_launches"]


def synchronous(c, cs, ct, **kw):
    c.tune("icp_pipeline", -1)
    s = result(c, cs, ct, **kw)[0]
    assert c.icp_last_chain() == SYNC and c.icp_last_snapshots() == 0
    c.tune("icp_pipeline", 0)
    return s


def pipelined(c, cs, ct, mode, **kw):
    """the chain search -> sums + solve with its snapshots written by the kernel (KERNEL) or copied on the stream (STREAM): (result, nn_launches)"""
    c.tune("icp_host_snapshots", mode)
    r = result(c, cs, ct, **kw)
    if kw.get("max_iter", 20) > 0:
        assert c.icp_last_chain() == MOVE and c.icp_last_snapshots() == (1 if mode == KERNEL else 0), (mode, kw)
    else:
        assert c.icp_last_snapshots() == 0, (mode, kw)
    return r


def both_modes(c, cs, ct, **kw):
    """kernel-written snapshots against copies: the same result, the same number of searches enqueued; returns the result"""
    a, la = pipelined(c, cs, ct, KERNEL, **kw)
    b, lb = pipelined(c, cs, ct, STREAM, **kw)
    assert a == b, ("kernel-written snapshots against copies on the stream", kw)
    assert la == lb, ("searches enqueued", la, lb, kw)
    return a


_sync_by_max_iter = {}


@gpu
@pytest.mark.parametrize("chunk", [1, 2, 4, 8])
def test_chunk_and_ring_edges(ctx, scan, five_thousand, chunk):
    """41 iterations at chunk 1 go ten times round the ring of four; sizes that are no multiple of the chunk end on a partial chunk; 0 enqueues nothing"""
    ct = scan[2]
    ctx.tune("prof", 1)
    for it in (0, 1, 2, 3, 4, 5, 9, 41):
        kw = dict(max_iter=it, eps=0.0)
        if it not in _sync_by_max_iter:
            _sync_by_max_iter[it] = synchronous(ctx, five_thousand, ct, **kw)
        ctx.tune("icp_chunk", chunk)
        a = both_modes(ctx, five_thousand, ct, **kw)
        ctx.tune("icp_chunk", 0)
        assert a == _sync_by_max_iter[it], (chunk, it)
        assert a[1] == it


@gpu
@pytest.mark.parametrize("levels", [1, 2])
def test_convergence_stops_the_enqueuing(ctx, scan, five_thousand, levels):
    """an eps above every change of the loss: `unchanged` passes 15 and the loop stops long before max_iter = 60 — the host must see it in a slot,
    the launches enqueued behind the stop publish the stopped state (and its snapshot) unchanged"""
    ct = scan[2]
    ctx.tune("prof", 1); ctx.tune("icp_ticket_levels", levels)
    kw = dict(max_iter=60, eps=1e30)
    want = synchronous(ctx, five_thousand, ct, **kw)
    assert want[2] == 1 and want[1] < 20
    for chunk in (1, 4):
        ctx.tune("icp_chunk", chunk)
        a, launches = pipelined(ctx, five_thousand, ct, KERNEL, **kw)
        assert a == want, chunk
        assert launches < 60, (chunk, launches)                      # the host did stop enqueuing
        assert both_modes(ctx, five_thousand, ct, **kw) == want, chunk
    ctx.tune("icp_chunk", 0)
    assert both_modes(ctx, five_thousand, ct, max_iter=3, eps=0.0)[1] == 3       # ... and the next call starts clean


@gpu
def test_empty_pairs_stop_the_enqueuing(ctx, scan):
    src, _, ct = scan
    s = src[:, :5000].copy(); s[0] += 1000.0                      # 1 000 m away: nothing within max_corr
    cs = ctx.cloud(np.ascontiguousarray(s))
    ctx.tune("prof", 1)
    kw = dict(max_iter=60, eps=0.0, max_corr=1.0)
    want = synchronous(ctx, cs, ct, **kw)
    assert want[3] == 1 and want[1] == 0
    a, launches = pipelined(ctx, cs, ct, KERNEL, **kw)
    assert a == want and launches < 60
    assert both_modes(ctx, cs, ct, **kw) == want
    cs.free()


@gpu
def test_overflow_then_a_clean_call(ctx, pcr, scan, five_thousand):
    """the overflow error reaches the host through a slot; the next call on the same context equals a fresh context's"""
    src, _, ct = scan
    s = src[:, :5000].copy(); s[0, 2500] = 1e12
    bad = ctx.cloud(s)
    fresh = pcr.Context(0)
    force_route(fresh)
    ft, fs = fresh.cloud(scan[1]), fresh.cloud(np.ascontiguousarray(src[:, :5000]))
    want = pipelined(fresh, fs, ft, KERNEL, max_iter=6, eps=0.0)[0]
    fs.free(); ft.free(); fresh.close()
    assert want == synchronous(ctx, five_thousand, ct, max_iter=6, eps=0.0)
    for mode in (KERNEL, STREAM):
        ctx.tune("icp_host_snapshots", mode)
        with pytest.raises(pcr.PcrError, match="target extents"):
            ctx.icp_point2point(bad, ct, max_corr=3e38, max_iter=5, eps=0.0)
        assert pipelined(ctx, five_thousand, ct, mode, max_iter=6, eps=0.0)[0] == want, mode
        assert pipelined(ctx, five_thousand, ct, mode, max_iter=6, eps=0.0)[0] == want, mode
    bad.free()


@gpu
def test_stale_slots(ctx, pcr, scan, five_thousand):
    """one context: 41 iterations at chunk 1 (every slot of the ring written ten times), then 1 iteration, then none, then a converging call — a slot
    left by an earlier call or an earlier trip round the ring is never taken for the one awaited: each call equals its result on a fresh context"""
    src, tgt, ct = scan
    calls = (dict(max_iter=41, eps=0.0), dict(max_iter=1, eps=0.0), dict(max_iter=0, eps=0.0), dict(max_iter=60, eps=1e30))
    want = []
    for kw in calls:
        fresh = pcr.Context(0)
        force_route(fresh); fresh.tune("icp_chunk", 1)
        ft, fs = fresh.cloud(tgt), fresh.cloud(np.ascontiguousarray(src[:, :5000]))
        want.append(pipelined(fresh, fs, ft, KERNEL, **kw)[0])
        fs.free(); ft.free(); fresh.close()
    assert want[3][2] == 1
    ctx.tune("icp_chunk", 1)
    for kw, w in zip(calls, want):
        assert pipelined(ctx, five_thousand, ct, KERNEL, **kw)[0] == w, kw
        assert w == synchronous(ctx, five_thousand, ct, **kw), kw


@gpu
@pytest.mark.parametrize("n", [1, 256, 257, 1792, 1793, 2049, 4096, 4097, 40000])
def test_replica_edges(ctx, scan, n):
    """at 256 threads x 1 pair: 1, 1, 2, 7, 8, 9, 16, 17 and 157 workgroups — fewer workgroups than replicas (replicas nobody arrives at must not be waited
    for), exactly eight, one more, replicas of unequal membership; the same sizes at the default 512 x 2.  One counter and a counter per replica give
    the same bits as the synchronous loop"""
    src, _, ct = scan
    cs = ctx.cloud(np.ascontiguousarray(src[:, :n]))
    kw = dict(max_iter=9, eps=0.0)
    want = synchronous(ctx, cs, ct, **kw)
    assert want[1] == 9
    for threads, pairs in ((256, 1), (512, 2)):
        ctx.tune("icp_sums_solve_threads", threads); ctx.tune("icp_sums_solve_pairs", pairs)
        for levels in (1, 2):
            ctx.tune("icp_ticket_levels", levels)
            assert both_modes(ctx, cs, ct, **kw) == want, (threads, pairs, levels)
    cs.free()


def test_replica_membership_counts_every_workgroup_once(pcr):
    """host logic: workgroup b arrives at replica b & 7; the members of the eight replicas sum to the workgroups of the launch, a replica has members
    exactly if the launch reaches it, and memberships differ by at most one"""
    for blocks in list(range(1, 21)) + [59, 118, 157, 235, 469]:
        m = [pcr.icp_replica_members(blocks, r) for r in range(8)]
        assert sum(m) == blocks, (blocks, m)
        assert m == [sum(1 for b in range(blocks) if b & 7 == r) for r in range(8)], (blocks, m)
        assert [v > 0 for v in m] == [r < blocks for r in range(8)], (blocks, m)
    assert pcr.icp_replica_members(5, 8) == 0 and pcr.icp_replica_members(0, 0) == 0
