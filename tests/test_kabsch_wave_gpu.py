"""The lane form of the Kabsch solve and of the state step on the device (csrc/kabsch_wave.hpp, csrc/icp_finish.hpp icp_state_step_wave).
pcr_kabsch_solve_batch_device — one wavefront per problem — against the scalar host solve on the classes of kabsch_wave_cases.py, bit for bit, at batch
sizes that cross a wave and a workgroup edge of the batch kernel; and the pipelined loops on every chain, whose kernels step the state with their first
wave (or, chain 5, with one wave of every search workgroup), against the synchronous loop, which uses the host's scalar solve: pose bits and stats.
Set-up of the loops as in test_icp_solve_in_search.py, with a 40 000-point target."""
import numpy as np
import pytest

import kabsch_wave_cases as cases

gpu = pytest.mark.gpu

NT = 40000
TUNES = ("icp_solve_in_search", "icp_move_in_search", "icp_fused_sums", "icp_fused_sums_min", "icp_pipeline", "nn_method", "nn1_sphere")
SOLVE, MOVE, FUSED_SUMS, THREE_LAUNCH, SYNC = 5, 4, 3, 2, 0           # Context.icp_last_chain()
PIPELINED = (SOLVE, MOVE, FUSED_SUMS, THREE_LAUNCH)


@pytest.fixture(scope="module")
def ctx(pcr):
    c = pcr.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool(pcr, synth):
    """(sums n x 16, rc, R bits, t bits) of the scalar host solve: every constructed class, then 1 000 seeded cases; computed once"""
    sums = np.concatenate([np.stack([s for _, s in cases.constructed(synth)]), cases.seeded(1000, seed=11)])
    rc, R, t = np.zeros(len(sums), np.int32), np.zeros((len(sums), 9), np.uint32), np.zeros((len(sums), 3), np.uint32)
    for i, s in enumerate(sums):
        rc[i], Ri, ti = pcr.kabsch_solve(s)
        R[i], t[i] = Ri.reshape(9).view(np.uint32), ti.view(np.uint32)
    assert (rc == 0).sum() > 1000 and (rc == cases.ERR_EMPTY).sum() == 2
    return sums, rc, R, t


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_batch_solve_bits(ctx, pool, n):
    """one problem, batches around 64, and one of 250 workgroups (a wave a problem, four problems a workgroup); every size but 1 begins with the thirty
    constructed cases"""
    sums, rc, R, t = pool
    lo = 0 if n >= 40 else 1                       # (n = 1: a diagonal H)
    sl = slice(lo, lo + n)
    assert lo + n <= len(sums)
    got_rc, got_R, got_t = ctx.kabsch_solve_batch_device(sums[sl])
    assert (got_rc == rc[sl]).all(), np.nonzero(got_rc != rc[sl])[0]
    bad = np.nonzero((got_R.reshape(n, 9).view(np.uint32) != R[sl]).any(1) | (got_t.view(np.uint32) != t[sl]).any(1))[0]
    assert bad.size == 0, (bad[:8], sums[sl][bad[:1]].tolist())


# ---- the loops
@pytest.fixture(autouse=True)
def _defaults(request):
    if "scan" not in request.fixturenames:
        yield
        return
    ctx = request.getfixturevalue("ctx")
    ctx.tune("nn_method", 1); ctx.tune("nn1_sphere", 1); ctx.tune("icp_fused_sums_min", 1)
    yield
    for k in TUNES:
        ctx.tune(k, 0)


@pytest.fixture(scope="module")
def scan(ctx, synth):
    src, tgt = synth.kitti_like_pair(NT, seed_target=181, seed_pair=182)
    ct = ctx.cloud(tgt)
    yield src, ct
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
    # (a loop without a search never chooses among chains 5, 4 and 3: it reports 3; the three-launch chain and the synchronous loop are set up front)
    assert ctx.icp_last_chain() == (which if ran or which in (SYNC, THREE_LAUNCH) else FUSED_SUMS), (which, kw)
    for k in ("icp_solve_in_search", "icp_move_in_search", "icp_fused_sums", "icp_pipeline"):
        ctx.tune(k, 0)
    return r


@gpu
@pytest.mark.parametrize("n", [1, 33, 129, 40000])
def test_loops_bits(ctx, scan, n):
    src, ct = scan
    cs = ctx.cloud(np.ascontiguousarray(src[:, :n]))
    for it in (0, 1, 2, 9):
        kw = dict(max_iter=it, eps=0.0)
        want = chain(ctx, SYNC, cs, ct, **kw)
        assert want[1] == it
        for which in PIPELINED:
            assert chain(ctx, which, cs, ct, **kw) == want, (which, it)
    cs.free()


@gpu
def test_loops_stop(ctx, scan):
    """the state machine's scalar part moved too: a loop that converges (16 unchanged losses) and one whose first iteration keeps no pair"""
    src, ct = scan
    cs = ctx.cloud(np.ascontiguousarray(src[:, :5000]))
    kw = dict(max_iter=40, eps=1e30)
    want = chain(ctx, SYNC, cs, ct, **kw)
    assert want[1] == 15 and want[2] == 1
    for which in PIPELINED:
        assert chain(ctx, which, cs, ct, **kw) == want, which
    kw = dict(max_iter=5, eps=1e-8, max_corr=1e-30)
    want = chain(ctx, SYNC, cs, ct, **kw)
    assert want[3] == 1 and want[1] == 0
    for which in PIPELINED:
        assert chain(ctx, which, cs, ct, **kw) == want, which
    cs.free()
