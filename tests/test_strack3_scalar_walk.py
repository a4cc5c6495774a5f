"""STRACK3's default instance (one query group, transposed: csrc/nn1_sphere.hpp, S3 SCALAR WALK) keeps the flag sets of levels 0 and 1 as ballots in
scalar registers and walks them there; the other instances (nn1_sphere_qg 2 / 4, nn1_s3_transposed 2) keep them as lists in LDS.  Both visit the same
tiles in the same order with the same evaluation cadence, so keys — and the counters of the diagnostics launch — must not differ.

CPU: the walk's index arithmetic (pcr_s3_walk_visits, built from the functions the kernel calls) against the list form written out below.
GPU: keys against the exact-only kernel (nn1_variant 2) at the ragged ends of every mask word, with stale far-side seeds that overfill the pair list, the counters of both forms at a
small size, and an ICP loop whose searches move the cloud against the synchronous loop."""
import numpy as np
import pytest

gpu = pytest.mark.gpu

KEYS = ("nn_method", "nn1_variant", "nn1_s3_transposed", "nn1_sphere_qg", "nn1_async_in_loop", "nn1_sphere_reseed", "nn1_sign_flush", "nn1_sphere_flush_end",
        "grid_stats", "icp_fused_sums_min", "icp_move_in_search", "icp_pipeline")
FORMS = [(qg, sw) for qg in (1, 2, 4) for sw in (1, 2)]          # (nn1_sphere_qg, nn1_s3_transposed)
L0_RECORDS = 131072                                              # records of a level-0 super-tile: 256 level-1 tiles of 512 = 4 096 level-2 tiles of 32


# ---------------------------------------------------------------------------------------------------------------- CPU: the walk against the list form
def list_form(S0, rows, tiles, n_rec):
    """What the LDS-list form of the kernel visits, step by step as it is written there: level 0 appends every flagged level-1 tile below
    n_l1_tiles to a list, bit by bit; level 1 takes from the list the (at most eight) entries of one level-1 super-tile — a run —, and appends
    the flagged level-2 tiles T2 with T2 * 32 < n_rec to a second list; level 2 goes through that list four entries at a time."""
    n_l1_tiles = (n_rec + 511) // 512
    l1list = []
    for t in range(8):
        T0 = S0 * 8 + t
        for j in range(32):
            if (int(rows[t]) >> j) & 1:
                T1 = T0 * 32 + j
                if T1 < n_l1_tiles:
                    l1list.append(T1)
    out, k = [], 0
    while k < len(l1list):
        S1 = l1list[k] >> 3
        out.append((0, S1))
        tl = []
        run = 0
        for u in range(8):
            if k + u >= len(l1list) or (l1list[k + u] >> 3) != S1:
                break
            run += 1
            T1 = l1list[k + u]
            out.append((1, T1))
            for k2 in range(16):
                if (int(tiles[T1 - S0 * 256]) >> k2) & 1:
                    T2 = T1 * 16 + k2
                    if T2 * 32 < n_rec:
                        tl.append(T2)
        k += run
        for k0 in range(0, len(tl), 4):
            batch = tl[k0:k0 + 4]
            out.append((2, len(batch)))
            out += [(3, T2) for T2 in batch]
    return out


def walk(pcr, S0, rows, tiles, n_rec):
    return [tuple(int(x) for x in r) for r in pcr.s3_walk_visits(S0, rows, tiles, n_rec)]


def test_walk_visits_equal_the_list_form(pcr):
    rng = np.random.default_rng(20260)
    full_rows, full_tiles = np.full(8, 0xFFFFFFFF, np.uint32), np.full(256, 0xFFFF, np.uint16)
    cases = []
    for S0 in (0, 1, 3):
        base, whole = S0 * L0_RECORDS, (S0 + 1) * L0_RECORDS
        cases.append((S0, np.zeros(8, np.uint32), full_tiles, whole))                      # nothing flagged
        cases.append((S0, full_rows, np.zeros(256, np.uint16), whole))                     # every run, no level-2 tile
        cases.append((S0, full_rows, full_tiles, whole))                                   # everything: 32 runs of 128 tiles
        # every validity bound: the records end in front of the super-tile, at its first record, around every word boundary of the row masks
        # (32 level-1 tiles = 16 384 records), around a run (4 096), a level-1 tile (512), the halves of the 128 tile bits (2 048) and a level-2 tile (32)
        ends = {0, base, base + 1, base + 31, base + 32, base + 33, whole - 32, whole - 1, whole, whole + 4096}
        for w in range(1, 8):
            ends |= {base + w * 16384 + d for d in (-512, -32, 0, 32, 512)}
        for edge in (512, 2048, 2048 + 32, 4096, 4096 + 32, 4096 + 2048, 4096 + 2048 - 32, 4608, 8192 - 32, 8192 + 64 * 32 + 32):
            ends |= {base + edge, base + edge - 1, base + edge + 1}
        for n_rec in sorted(e for e in ends if e >= 0):
            cases.append((S0, full_rows, full_tiles, n_rec))
        for density in (0.02, 0.2, 0.5, 0.9):                                              # random words, sparse to dense, cut at a random bound
            for _ in range(6):
                rows = np.zeros(8, np.uint32)
                for t in range(8):
                    rows[t] = sum(1 << j for j in range(32) if rng.random() < density)
                tiles = np.array([sum(1 << k2 for k2 in range(16) if rng.random() < density) for _ in range(256)], np.uint16)
                cases.append((S0, rows, tiles, int(rng.integers(base, whole + 1))))
                cases.append((S0, rows, tiles, whole))
        one = np.zeros(8, np.uint32); one[3] = 1 << 17                                     # single bits: one run of one tile, its first and its last level-2 tile
        t_one = np.zeros(256, np.uint16); t_one[3 * 32 + 17] = 0x8001
        cases.append((S0, one, t_one, whole))
    for S0, rows, tiles, n_rec in cases:
        want = list_form(S0, rows, tiles, n_rec)
        got = walk(pcr, S0, rows, tiles, n_rec)
        assert got == want, (S0, n_rec, [hex(int(r)) for r in rows], len(got), len(want), next((i, g, w) for i, (g, w) in enumerate(zip(got + [None], want + [None])) if g != w))
    # run grouping: the runs are the non-empty bytes of the row words, each named once, ascending
    runs = [v for kind, v in walk(pcr, 1, full_rows, full_tiles, 2 * L0_RECORDS) if kind == 0]
    assert runs == list(range(32, 64))
    assert sum(1 for kind, _ in walk(pcr, 1, full_rows, full_tiles, 2 * L0_RECORDS) if kind == 3) == 4096


def test_walk_visits_reports_a_short_buffer(pcr):
    import ctypes as C
    rows, tiles = np.full(8, 1, np.uint32), np.full(256, 1, np.uint16)
    out = np.zeros(4, np.uint32)
    m = C.c_size_t(0)
    rc = pcr.lib().pcr_s3_walk_visits(0, rows.ctypes.data, tiles.ctypes.data, L0_RECORDS, out.ctypes.data, out.size, C.byref(m))
    assert rc == -1 and m.value == len(list_form(0, rows, tiles, L0_RECORDS)) and list(out) == [0, 0, 1, 0]
    assert pcr.lib().pcr_s3_walk_visits(0, None, tiles.ctypes.data, L0_RECORDS, out.ctypes.data, out.size, C.byref(m)) == -1


# ---------------------------------------------------------------------------------------------------------------------------------------------- GPU
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


def strack3(ctx, ct, cs, qg, sw):
    ctx.tune("nn_method", 1); ctx.tune("nn1_variant", 10); ctx.tune("nn1_s3_transposed", sw); ctx.tune("nn1_sphere_qg", qg)
    out = ctx.nn1(ct, cs)
    assert ctx.mfma_check()["last_nn1_kernel"] == "strack3", (qg, sw)
    return out


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(bits32(a[1]), bits32(b[1]))


@pytest.fixture(scope="module")
def big_scan(synth):
    """one scan of 131 073 + 40 points and sources drawn from it: every smaller target and source is a prefix"""
    nt = 131073 + 40
    tgt = synth.kitti_like_scan(nt, seed=4711)
    src, _ = synth.kitti_like_pair(2048, seed_target=4712, seed_pair=4713)
    return tgt, src


@gpu
@pytest.mark.parametrize("nt", [1, 31, 33, 511, 513, 4095, 4097, 4608, 32768, 36865, 131073 + 40])
def test_ragged_ends_of_every_mask_word(ctx, big_scan, nt):
    """Targets that end one record before / at / one record behind a level-2 tile (32), a level-1 tile (512), a run (4 096), in a super-tile that holds
    one tile (4 608), at the size from which the kernel is the default (32 768), just behind a run of a larger index (36 865) and in a second level-0
    super-tile (131 113): every form returns the exact kernel's keys."""
    tgt_all, src_all = big_scan
    # (a strided subset keeps the scan's extent at every size)
    tgt = np.ascontiguousarray(tgt_all[:, :: tgt_all.shape[1] // nt][:, :nt]) if nt < tgt_all.shape[1] else tgt_all
    assert tgt.shape[1] == nt
    ct = ctx.cloud(tgt)
    for ns in ((64,) if nt > 131072 else (1, 33, 2000)):
        cs = ctx.cloud(np.ascontiguousarray(src_all[:, :ns]))
        ref = exact(ctx, ct, cs)
        for qg, sw in FORMS:
            got = strack3(ctx, ct, cs, qg, sw)
            assert same(got, ref), (nt, ns, qg, sw, int((got[0] != ref[0]).sum()))
        cs.free()
    ct.free()
    reset(ctx)


@gpu
def test_target_whose_last_level1_tile_has_no_finite_record(ctx, big_scan):
    """4 608 targets, the last 600 of them NaN / inf: the index sorts those behind the 4 008 finite ones, so its last tiles of 32, its whole last
    level-1 tile of 512 and most of the second super-tile of 4 096 hold no finite record (centres, scales and spheres of nothing).  Every sphere
    form returns the exact kernel's keys, and an ICP loop through the tile search the poses of the exhaustive loop."""
    tgt_all, src_all = big_scan
    nt = 4608
    tgt = np.ascontiguousarray(tgt_all[:, :: tgt_all.shape[1] // nt][:, :nt]).copy()
    tgt[:, nt - 600:nt - 300] = np.nan; tgt[0, nt - 300:] = np.inf; tgt[1, nt - 100:] = -np.inf
    ct = ctx.cloud(tgt)
    try:
        for ns in (1, 33, 2000):
            cs = ctx.cloud(np.ascontiguousarray(src_all[:, :ns]))
            ref = exact(ctx, ct, cs)
            assert ref[0].max() < nt - 600, ns
            for qg, sw in FORMS:
                got = strack3(ctx, ct, cs, qg, sw)
                assert same(got, ref), (ns, qg, sw, int((got[0] != ref[0]).sum()))
            cs.free()
        reset(ctx)
        cs = ctx.cloud(np.ascontiguousarray(src_all[:, :2000]))
        ctx.tune("nn_method", 1)
        ref = [ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=it, eps=0.0) for it in (1, 3, 6)]
        ctx.tune("nn_method", 2); ctx.tune("grid_order", 2); ctx.tune("grid_mode", 3); ctx.tune("grid_tile", 1)
        cm = ctx.cloud(tgt)                                    # a fresh cloud: its index is built Morton-ordered
        used = set()
        for it, (Tr, sr) in zip((1, 3, 6), ref):
            T, st = ctx.icp_point2point(cs, cm, max_corr=1.0, max_iter=it, eps=0.0)
            if it > 2:
                used.add(ctx.mfma_check()["last_nn1_kernel"])
            assert np.array_equal(T.view(np.uint32), Tr.view(np.uint32)), it
            assert st["last_pairs"] == sr["last_pairs"] and st["iters_run"] == sr["iters_run"], it
            assert np.float32(st["last_loss"]).view(np.uint32) == np.float32(sr["last_loss"]).view(np.uint32), it
        assert used == {"grid-stile"}, used
        cs.free(); cm.free()
    finally:                                                   # (the context is the module's: a failure must not leave the routes switched)
        for k in ("grid_order", "grid_mode", "grid_tile"):
            ctx.tune(k, 0)
        reset(ctx)
        ct.free()


@gpu
def test_far_queries_with_stale_seeds_overfill_the_pair_list(ctx, synth):
    """64 queries 300 m outside a target of 8 193 points, searched in a loop from alternating sides.  A search that keeps stale seeds
    (nn1_sphere_reseed = 2) starts from the winners of the pose 300 m on the OTHER side — the far side of the target as seen from here —, so a
    query's ball reaches across the target.  Measured with the diagnostics on (printed below): level 0 flags every row that holds records (17 per
    wave), level 1 about half of their level-2 tiles (133 per wave), and an evaluation carries 250 (query, chunk) pairs on average — the pair list
    passes S2_CAP = 128 inside a batch of four tiles every time.  (A run with all 128 tile bits set is the CPU test's case above.)  The three flush
    settings of test_strack3_transposed's stale-seed test; keys equal the exact kernel's under every form."""
    nt, nq = 8193, 64
    tgt = synth.kitti_like_scan(nt, seed=977)
    mid = (tgt.min(axis=1, keepdims=True) + tgt.max(axis=1, keepdims=True)) * np.float32(0.5)
    ext = float((tgt.max(axis=1) - tgt.min(axis=1))[0]) * 0.5
    rng = np.random.default_rng(978)
    jit = rng.normal(0.0, 0.5, (3, nq)).astype(np.float32)
    east = np.ascontiguousarray(mid + np.array([[ext + 300.0], [0.0], [0.0]], np.float32) + jit)
    west = np.ascontiguousarray(mid - np.array([[ext + 300.0], [0.0], [0.0]], np.float32) + jit)
    assert (east[0] - tgt[0].max()).min() > 295.0 and (tgt[0].min() - west[0]).min() > 295.0
    ct0 = ctx.cloud(tgt)
    ce, cw = ctx.cloud(east), ctx.cloud(west)
    ref = {"e": exact(ctx, ct0, ce), "w": exact(ctx, ct0, cw)}
    ctx.tune("nn_method", 1); ctx.tune("nn1_variant", 10)
    for qg, sw in FORMS:
        for reseed, flush, fend in ((0, 0, 0), (2, 1, 0), (2, 100000, 128)):
            ctx.tune("nn1_s3_transposed", sw); ctx.tune("nn1_sphere_qg", qg); ctx.tune("nn1_sphere_reseed", reseed)
            ctx.tune("nn1_sign_flush", flush); ctx.tune("nn1_sphere_flush_end", fend)
            ctx.tune("nn1_async_in_loop", 1)
            fresh = ctx.cloud(tgt)
            for k, (name, c_) in enumerate((("w", cw), ("e", ce), ("w", cw), ("e", ce))):
                ctx.tune("grid_stats", 1 if k == 3 else 0)
                ctx.nn1_async(fresh, c_)
                assert ctx.mfma_check()["last_nn1_kernel"] == "strack3", (qg, sw, reseed, k)
                got = ctx.nn1_fetch(nq)
                assert same(got, ref[name]), (qg, sw, reseed, flush, fend, k, int((got[0] != ref[name][0]).sum()))
            w = [int(v) for v in ctx.nn1_stats()]
            print(f"qg {qg} nn1_s3_transposed {sw} reseed {reseed} flush {flush} / {fend}: l1 tiles flagged {w[3]} l2 tiles flagged {w[9]} l2 mfma {w[10]} evaluated {w[6]} evaluations {w[2]}")
            ctx.tune("grid_stats", 0); ctx.tune("nn1_async_in_loop", 0)
            fresh.free()
    reset(ctx)


@gpu
def test_flag_counters_of_both_forms_equal_at_a_small_size(ctx, big_scan):
    """One one-shot search of 2 000 queries over 36 865 points with the diagnostics on: level-1 tiles flagged by level 0 (word 3), (query, chunk)
    pairs evaluated (6), level-1 MFMAs (8), level-2 tiles flagged by level 1 (9) and level-2 MFMAs (10) of the scalar walk equal those of the rows
    form, which lists — same visits, same cadence of evaluations, same thresholds."""
    tgt_all, src_all = big_scan
    nt = 36865
    tgt = np.ascontiguousarray(tgt_all[:, :: tgt_all.shape[1] // nt][:, :nt])
    ct, cs = ctx.cloud(tgt), ctx.cloud(np.ascontiguousarray(src_all[:, :2000]))
    ref = exact(ctx, ct, cs)
    w = {}
    for sw in (1, 2):
        ctx.tune("grid_stats", 1)
        got = strack3(ctx, ct, cs, 1, sw)
        w[sw] = [int(v) for v in ctx.nn1_stats()]
        ctx.tune("grid_stats", 0)
        assert same(got, ref), sw
        print(f"nn1_s3_transposed {sw}: l0 mfma {w[sw][7]} l1 tiles flagged {w[sw][3]} l1 mfma {w[sw][8]} l2 tiles flagged {w[sw][9]} l2 mfma {w[sw][10]} evaluated {w[sw][6]}")
    assert w[1][3] > 0 and w[1][9] > 0 and w[1][6] > 0, w[1]
    for word in (3, 6, 8, 9, 10):
        assert w[1][word] == w[2][word], (word, w[1], w[2])
    cs.free(); ct.free()
    reset(ctx)


@gpu
def test_moving_form_equals_the_synchronous_loop(ctx, big_scan, synth):
    """Six ICP iterations of 4 099 points against 36 865 with the cloud moved in the next search's prologue (chain 4: nn1_strack3_move_kernel<1>): pose
    bits and stats equal the synchronous loop's."""
    nt, ns = 36865, 4099
    src, tgt = synth.kitti_like_pair(nt, seed_target=4721, seed_pair=4722)
    cs, ct = ctx.cloud(np.ascontiguousarray(src[:, :: nt // ns][:, :ns])), ctx.cloud(tgt)
    ctx.tune("nn_method", 1); ctx.tune("nn1_variant", 10); ctx.tune("icp_fused_sums_min", 1)

    def result():
        T, st = ctx.icp_point2point(cs, ct, max_corr=1.0, max_iter=6, eps=0.0)
        return (T.view(np.uint32).tobytes(), st["iters_run"], st["converged"], st["empty_pairs"], st["last_pairs"], np.float32(st["last_loss"]).tobytes())

    ctx.tune("icp_move_in_search", 1)
    a = result()
    assert ctx.icp_last_chain() == 4
    assert ctx.mfma_check()["last_nn1_kernel"] == "strack3"
    ctx.tune("icp_pipeline", -1)
    s = result()
    assert ctx.icp_last_chain() == 0
    assert a[1] == 6 and a[4] > 0
    assert a == s
    cs.free(); ct.free()
    reset(ctx)
