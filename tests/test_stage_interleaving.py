"""Every stage of tests/stage_cases.py on a context and clouds that other stages have used.

The library is driven by programs that keep ONE context and a few Cloud handles alive through a dozen stages, and both carry state from call
to call: the correspondence workspace keys[] with the handles it belongs to, the query permutation, the winners' record
positions, parked buffers, scratch that only grows, tickets that count modulo the last batch; on a cloud the 1-NN grid (whose order depends
on the size and on grid_order when it was built), the matrix-core operands, one widened k-NN grid, one radius grid, absmax.  By design the
ROUTE of a call depends on that history.  The answer must not.

GPU tests (one context and one set of handles per test):
  ordered pairs     for every ordered pair (A, B) of stages: dirty the context as test_context_state._dirty does, run A, run B, check B, run A
                    again, check A.  One test per predecessor A; a failure names A in its id and B in its message.
  size walks        the searches and the loop's sums at 500 -> 20 000 -> 500 queries and back
  handle mutations  transform by a known pose, assign from another cloud, in-place sort, free + create, clone, trim — and tune flips —
                    between two runs of every stage that caches something on the handle; expected values from the moved / replaced model
  search -> consumer  pcr_nn1_fetch and pcr_kabsch_sums after a search with something in between: the contract of include/pcr.h
  random walks      seeded walks over stages, mutations and tune flips, every step checked; a failure prints seed and steps
  two contexts      alive at once on device 0, interleaved call by call
Every check is against the CPU reference of the stage and, while the handles hold their first content, against the same call on a fresh
context bit for bit (except the point-to-plane pose).  CPU tests: the references exist and are not trivial, every input lies on its side of
the thresholds read from the sources, the committed sequences cover every pair and every (mutation, caching stage)."""
import numpy as np
import pytest

import stage_cases as sc
from stage_cases import KINDS, MUTABLE, MUTATIONS, STAGES, TUNE_FLIPS
from test_context_state import _dirty

gpu = pytest.mark.gpu
WALK_SEEDS = (20261021, 20261022, 20261023)
WALK_STEPS = 40
COUNTS = {"pairs": 0, "mutations": 0, "tune flips": 0, "walk steps": 0, "size-walk calls": 0, "two-context calls": 0, "consumer cases": 0}


# ------------------------------------------------------------------------------------------------------------------ sequences
def pair_sequence(a):
    """what the ordered-pair test of predecessor a runs: (a, b) for every stage b, a itself included"""
    return [(a, b) for b in KINDS]


def mutation_cases(mutation, handle=None):
    """(handle, stage) for every stage that caches something on a handle the mutation applies to (trim: on any handle)"""
    if mutation == "trim":
        return [(h, s) for s in sc.CACHE_READERS for h in STAGES[s].caches[:1] if handle in (None, h)]
    return [(h, s) for s in sc.CACHE_READERS for h in STAGES[s].caches if h in MUTABLE and handle in (None, h)]


def walk(seed):
    """[(kind, ...)] of WALK_STEPS steps: ("stage", name) | ("mutate", mutation, handle) | ("flip", key, value)"""
    rng = np.random.default_rng(seed)
    steps = []
    for _ in range(WALK_STEPS):
        u = rng.uniform()
        if u < 0.7:
            steps.append(("stage", KINDS[int(rng.integers(len(KINDS)))]))
        elif u < 0.9:
            m = list(MUTATIONS)[int(rng.integers(len(MUTATIONS)))]
            steps.append(("mutate", m, MUTABLE[int(rng.integers(len(MUTABLE)))]))
        else:
            steps.append(("flip",) + TUNE_FLIPS[int(rng.integers(len(TUNE_FLIPS)))])
    return steps


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.fixture(scope="module")
def inp(synth, orc):
    return sc.inputs(synth, orc)


@pytest.fixture(scope="module")
def view(inp, orc, pcr):
    return sc.View(inp, orc, pcr)


def test_inputs_lie_on_their_side_of_every_threshold(inp):
    t = sc.thresholds()
    n3, n5, n66 = inp["P3t"].shape[1], inp["C5"].shape[1], inp["T66"].shape[1]
    assert inp["S3"].shape[1] == inp["P3s"].shape[1] == inp["ALT3"].shape[1] == n3 and all(set(STAGES[s].caches) <= set(MUTABLE) for s in STAGES)
    assert inp["S3"].shape[1] == n3 and inp["ALT5"].shape[1] == n5 and inp["ALT66"].shape[1] == n66
    assert t.loop_grid == t.oneshot_min <= n3 < t.twin_min                  # a loop on the small pair takes the grid ...
    assert n3 < t.oneshot_grid and n3 * n3 <= 2.0e9                         # ... its one-shot search the exhaustive kernels unless an index is there already
    assert n66 >= t.oneshot_grid                                            # the large target: the grid from its first one-shot search, and a fine query sort as a cloud
    assert n5 > t.knn_small_max and n5 >= t.twin_min                        # C5: a batch of its own size is no small batch; a Db64 of it has the f32 twin
    assert all(np.array_equal(sc._db_queries(sc.View(inp, None), m), sc._db_queries(sc.View(inp, None), m).astype(np.float32)) for m in sc.COOP_M + (17, 300))   # the twin's routes
    assert all(m <= t.knn_coop_max for m in sc.COOP_M) and len(set(sc.COOP_M)) > 2 and sc.COOP_M[0] == sc.COOP_M[-1]
    assert t.knn_coop_max < 17 and 300 <= t.knn_small_max
    assert min(n3, n5) >= t.morton_min                                      # every target: Morton order by default, x-sorted under grid_order 1
    assert sc.SIZES[0] < n3 < sc.SIZES[1] <= n66
    for k in ("T66", "S3", "P3t", "C5"):
        assert np.isfinite(inp[k]).all()


def test_expected_results_exist_and_are_not_trivial(view):
    want = {name: sc.expected(st, view) for name, st in STAGES.items() if st.expect is not None}
    assert set(STAGES) - set(want) == {"pn2_forward"}
    T, st = want["icp_big"]
    assert st["iters_run"] == 3 and st["last_pairs"] > 1500 and np.linalg.norm(T - np.eye(4)) > 0.1                  # ICP moves
    assert want["icp_iter0"][1]["iters_run"] == 0 and want["icp_iter1"][1]["iters_run"] == 1
    assert want["icp_converged"][1]["converged"] == 1 and 1 < want["icp_converged"][1]["iters_run"] < 40
    assert want["icp_empty"][1]["empty_pairs"] == 1 and want["icp_empty"][1]["iters_run"] == 0
    assert want["p2plane_sorted"][1]["iters_run"] == 4 and np.linalg.norm(want["p2plane_sorted"][0] - np.eye(4)) > 0.1
    for name in ("loop_sums_grid", "loop_sums_big"):
        gi, gd, sums, last = want[name]
        assert 0 < sums[15] < gi.size and (gi == sc.NONE).sum() == gi.size - sums[15] and last >= 0                  # the gate keeps some pairs and drops some
    labels, core, counts, nc = want["dbscan"]
    assert nc > 1 and (labels == -1).any() and core.any() and not core.all()                                           # clusters, noise, border points
    for r in sc.RADII:
        row = want[f"db64_radius_r{r}"][0]
        assert len(set(np.diff(row).tolist())) > 5                                                                      # radius rows of different lengths
    assert want["db64_radius_r0.5"][0][-1] < want["db64_radius_r1.25"][0][-1]
    for name in ("cloud_knn_resident", "cloud_knn_self"):
        found = want[name][-1][2]
        assert (found == 32).any() and (found < 32).any() and ((found > 0) & (found < 10)).any(), name                 # short k-NN rows, at k = 32 and at k = 10
    assert (want["cloud_knn_resident"][-1][2] == 0).any()                                                              # ... and empty ones
    keep = want["statistical_outlier"][1]
    assert 0 < keep.sum() < keep.size
    assert 0 < want["iss_keypoints"][0].sum() < 500 and 0 < want["harris3d"][0].sum() < 2500
    assert 100 < want["voxel_filter"][0].shape[1] < 5000 and want["normal_space_sample"][0].size == 700
    assert len(want["match_union"][0]) > 100 and len(want["match_inter"][0]) > 20 and want["ransac_global"][3] > 50
    assert want["plane_count_150"][0].max() > 1000 and 0 < want["plane_mask"][1] < 5000
    assert want["ground_detection"][1].sum() > 1000 and 0 < want["ground_seeds"][0].sum() < 5000
    assert (want["ball_query"][1] > 0).all() and (want["ball_query"][1] < sc.BALL[1]).any() and (want["ball_query"][1] == sc.BALL[1]).any()
    assert want["points_in_boxes"][0][-1] > 0 and (want["points_in_boxes"][2] > 1).any()                                # boxes hold points, some points lie in two
    assert len(set(want["kmeans_step"][0].tolist())) == 6
    sp, cnt, fragile, _ = want["fpfh33"]
    assert len(set(cnt.tolist())) > 20 and cnt.max() > 100 and fragile.mean() < 1e-3                                   # FPFH neighbourhoods of many sizes
    pr, cluster, n_clusters, _, _ = want["range_cluster"]
    assert cluster is not None and n_clusters > 10 and (cluster >= 0).all() and np.bincount(cluster).max() > 1000     # no pair in the band; a ground and objects
    idx, d2 = want["mat64_knn"]
    assert np.array_equal(idx[:, 0], np.arange(idx.shape[0])) and (d2[:, 1] > 0).any()
    rc = want["kabsch_batch"][0]
    assert (rc == 0).sum() > 50 and (rc != 0).any()


def test_a_moved_model_changes_what_is_expected(view, inp, orc, pcr):
    """the expected value of a mutated handle comes from the mutated model: another cache key, another answer"""
    V = sc.View(inp, orc, pcr)
    V.set("T66", orc.transform_f32(inp["T66"], sc.POSE[:3, :3], sc.POSE[:3, 3]), "T66@")
    a, b = sc.expected(STAGES["nn1_m0"], view), sc.expected(STAGES["nn1_m0"], V)
    assert a is sc.expected(STAGES["nn1_m0"], view) and a is not b and not np.array_equal(a[0], b[0])


def test_sequences_cover_every_pair_mutation_and_flip():
    pairs = {p for a in KINDS for p in pair_sequence(a)}
    assert pairs == {(a, b) for a in KINDS for b in KINDS} and len(KINDS) >= 50
    for m in MUTATIONS:
        cases = [c for h in MUTABLE for c in mutation_cases(m, h)]          # what the parametrised test runs
        assert {s for _, s in cases} == set(sc.CACHE_READERS), (m, set(sc.CACHE_READERS) - {s for _, s in cases})
        assert {h for h, _ in cases} == set(MUTABLE) and sorted(cases) == sorted(mutation_cases(m)), m
        assert all(h in STAGES[s].caches for h, s in cases), m
    assert len(sc.CACHE_READERS) >= 20
    steps = [s for seed in WALK_SEEDS for s in walk(seed)]
    assert walk(WALK_SEEDS[0]) == walk(WALK_SEEDS[0])                                           # a walk is a function of its seed
    assert {s[1] for s in steps if s[0] == "mutate"} == set(MUTATIONS) and {s[1] for s in steps if s[0] == "flip"} >= {"grid_order", "nn_method", "knn_cell_scale_x100"}
    assert len({s[1] for s in steps if s[0] == "stage"}) >= 35


# ------------------------------------------------------------------------------------------------------------------ GPU
_FRESH = {}


def fresh(pcr, orc, inp, name):
    """the stage on a context of its own with handles of its own, as bytes: computed once per module"""
    if name not in _FRESH:
        with pcr.Context(0) as ctx:
            H = sc.Handles(pcr, ctx, inp, orc)
            try:
                _FRESH[name] = sc.canon(STAGES[name].run(ctx, H))
            finally:
                H.close()
    return _FRESH[name]


def pristine(H, stage):
    """every array the stage reads, or reads an index of, is the one the fresh context holds"""
    return all(H.tok(n) == n for n in stage.uses + stage.caches)


def run_and_check(pcr, orc, inp, H, name, what):
    st = STAGES[name]
    got = st.run(H.ctx, H)
    if st.expect is not None:
        st.check(got, sc.expected(st, H), f"{name} {what}")
    if st.fresh_equal and pristine(H, st):
        assert sc.canon(got) == fresh(pcr, orc, inp, name), f"{name} {what}: not the bits of the same call on a fresh context"
    return got


@pytest.fixture(scope="module")
def references(view):
    """the CPU reference of every stage on the first content of the handles: computed once per module, ahead of the first GPU test"""
    return {name: sc.expected(st, view) for name, st in STAGES.items() if st.expect is not None}


@pytest.fixture(scope="module")
def fresh_answers(pcr, orc, inp):
    """every stage on a context of its own: computed once per module, ahead of the first GPU test"""
    for name in KINDS:
        fresh(pcr, orc, inp, name)
    return _FRESH


@pytest.fixture
def rig(pcr, orc, inp, references, fresh_answers):
    """one context, one set of handles"""
    ctx = pcr.Context(0)
    H = sc.Handles(pcr, ctx, inp, orc)
    dirt = ctx.cloud(inp["ALT66"][:, :20000])
    yield SimpleRig(pcr, orc, inp, ctx, H, dirt)
    sc.unflip(ctx)
    H.close()
    ctx.close()


class SimpleRig:
    def __init__(self, pcr, orc, inp, ctx, H, dirt):
        self.pcr, self.orc, self.inp, self.ctx, self.H, self.dirt = pcr, orc, inp, ctx, H, dirt

    def check(self, name, what):
        return run_and_check(self.pcr, self.orc, self.inp, self.H, name, what)


@gpu
@pytest.mark.parametrize("a", KINDS)
def test_ordered_pairs(rig, a):
    for _, b in pair_sequence(a):
        _dirty(rig.ctx, rig.dirt)
        STAGES[a].run(rig.ctx, rig.H)
        rig.check(b, f"after {a}")
        rig.check(a, f"after {a}, {b}")
        COUNTS["pairs"] += 1
    print(f"ordered pairs: predecessor {a}, {len(KINDS)} successors checked ({COUNTS['pairs']} pairs so far)")


@gpu
@pytest.mark.parametrize("order", [(0, 1, 0), (1, 0, 1)], ids=["small-large-small", "large-small-large"])
def test_size_walks(rig, order):
    for k in range(len(sc.SIZED[sc.SIZES[0]])):
        for pos, which in enumerate(order):
            st = sc.SIZED[sc.SIZES[which]][k]
            st.check(st.run(rig.ctx, rig.H), sc.expected(st, rig.H), f"{st.name}, call {pos} of {order}")
            COUNTS["size-walk calls"] += 1
    # ... and the loop's working copies (the parked buffers) at three sizes in turn
    for pos, name in enumerate(("icp_big", "icp_iter1", "icp_big", "icp_converged", "p2plane_sorted", "icp_big")):
        rig.check(name, f"size walk {order}, call {pos}")
        COUNTS["size-walk calls"] += 1
    print(f"size walks: {COUNTS['size-walk calls']} calls checked so far")


@gpu
@pytest.mark.parametrize("handle", MUTABLE)
@pytest.mark.parametrize("mutation", list(MUTATIONS))
def test_handle_mutation_between_two_cache_readers(rig, mutation, handle):
    cases = mutation_cases(mutation, handle)
    for _, name in cases:
        sc.reset(rig.H, handle)                                             # (the first content again: a few mutated contents, each reference computed once)
        rig.check(name, f"before {mutation}({handle})")                     # leaves its caches on the handle
        MUTATIONS[mutation](rig.H, handle)
        rig.check(name, f"after {mutation}({handle}) [{rig.H.tok(handle)}]")
        COUNTS["mutations"] += 1
    print(f"handle mutations: {mutation}({handle}) before {len(cases)} caching stages ({COUNTS['mutations']} cases so far)")


@gpu
@pytest.mark.parametrize("key,value", TUNE_FLIPS)
def test_tune_flip_between_two_cache_readers(rig, key, value):
    for name in sc.CACHE_READERS:
        rig.check(name, f"before {key} = {value}")
        sc.flip(rig.ctx, key, value)
        rig.check(name, f"under {key} = {value}")
        sc.unflip(rig.ctx)
        rig.check(name, f"after {key} = {value} and back")
        COUNTS["tune flips"] += 1
    print(f"tune flips: {key} = {value}, {len(sc.CACHE_READERS)} stages checked ({COUNTS['tune flips']} so far)")


# ---- search -> consumer ----------------------------------------------------------------------------------------------------------------
SEARCHES = {                                                    # name -> (target, source, nn_method, loop?)
    "loop-grid": ("P3t", "P3s", 2, True), "loop-brute": ("P3t", "P3s", 1, True), "loop-auto-big": ("T66", "S3", 0, True),
    "async-grid-big": ("T66", "S3", 0, False), "async-brute": ("P3t", "P3s", 1, False), "async-grid": ("P3t", "P3s", 2, False),
}
UNRELATED = ("dbscan", "cloud_knn_self", "db64_knn_coop", "db64_radius_r0.5", "normals", "voxel_filter", "plane_count_150", "harris3d", "ransac_global",
             "kabsch_batch", "fps_f32", "pointnet_forward", "kmeans_step")           # on C5 or on no cloud at all: none of them searches
SEARCHING = ("icp_big", "icp_iter1", "icp_empty", "p2plane_sorted")                    # write the correspondence workspace themselves


def search(rig, which):
    tgt, src, method, loop = SEARCHES[which]
    ct, cs = rig.H.cloud(tgt), rig.H.cloud(src)
    with sc.tuned(rig.ctx, nn_method=method):
        if loop:
            rig.ctx.nn1_loop(ct, cs, 1.0)
        else:
            rig.ctx.nn1_async(ct, cs)
    return ct, cs


def consume(rig, ct, cs):
    sums, last, last_d2 = rig.ctx.kabsch_sums(ct, cs, 1.0)
    idx, d2 = rig.ctx.nn1_fetch(len(cs))
    return idx, d2, sums, np.int64(last), np.float32(last_d2)


def consumer_reference(rig, which):
    tgt, src, _, loop = SEARCHES[which]
    gi, gd, sums, last = sc._gated(rig.H, tgt, src, 1.0)
    if not loop:                                                # an unbounded search reports every neighbour; the sums keep the same pairs
        gi, gd = rig.orc.nn1_f32_mt(rig.H.arr(tgt), rig.H.arr(src), threads=sc.THREADS)
    return gi, gd, sums, last


@gpu
@pytest.mark.parametrize("which", list(SEARCHES))
def test_unrelated_stage_between_search_and_consumer(rig, which):
    """a stage that does not search, on clouds the search did not touch, changes neither pcr_nn1_fetch nor pcr_kabsch_sums: the bits of the
    consumer right behind the search, and the oracle's rows and sums"""
    ct, cs = search(rig, which)
    base = consume(rig, ct, cs)
    sc._loop_check(base, consumer_reference(rig, which), which)
    for name in UNRELATED:
        ct, cs = search(rig, which)
        rig.check(name, f"between {which} and its consumers")
        got = consume(rig, ct, cs)
        assert sc.canon(got) == sc.canon(base), f"{name} between {which} and its consumers changed their answer"
        COUNTS["consumer cases"] += 1
    # reading, cloning and trimming are no modification either; nor is an ordering stage on other clouds
    ct, cs = search(rig, which)
    cs.numpy(); ct.clone().free(); rig.ctx.trim()
    rig.check("sort_for_target" if SEARCHES[which][0] != "T66" else "cloud_knn_resident", "between a search and its consumers")
    assert sc.canon(consume(rig, ct, cs)) == sc.canon(base), which


@gpu
@pytest.mark.parametrize("which", list(SEARCHES))
def test_searching_stage_between_search_and_consumer_is_a_state_error(rig, which):
    """include/pcr.h: after a stage that searches on the context itself, pcr_nn1_fetch and pcr_kabsch_sums return PCR_ERR_STATE — never that
    stage's correspondences — whether or not its search had the same number of queries; the next search of the caller's puts both back"""
    state = rig.pcr.ERRORS[-4]
    for name in SEARCHING:
        ct, cs = search(rig, which)
        rig.check(name, f"between {which} and its consumers")
        with pytest.raises(rig.pcr.PcrError, match=state):
            rig.ctx.kabsch_sums(ct, cs, 1.0)
        with pytest.raises(rig.pcr.PcrError, match=state):                  # (every one of them searched with as many queries: no bad argument)
            rig.ctx.nn1_fetch(len(cs))
        ct, cs = search(rig, which)
        sc._loop_check(consume(rig, ct, cs), consumer_reference(rig, which), f"{which} after {name}")
        COUNTS["consumer cases"] += 1


@gpu
@pytest.mark.parametrize("which", list(SEARCHES))
def test_mutated_handle_between_search_and_consumer_is_a_state_error(rig, which):
    """include/pcr.h: pcr_kabsch_sums needs the search of exactly this pair with neither cloud modified since; pcr_nn1_fetch still returns the
    rows of the search as it ran.  Includes the sequence search -> transform(target) -> a stage that rebuilds the target's grid -> sums, where
    the record positions of the search index another grid (hypothesis 1)."""
    state = rig.pcr.ERRORS[-4]
    tgt, src, _, _ = SEARCHES[which]
    # what builds the 1-NN grid of the target again without being a search of the caller's: a sort of another cloud FOR this target
    rebuild = "sort_for_target" if tgt == "T66" else "sort-C5-for-P3t"
    for mutation, handle, then in (("transform", tgt, rebuild), ("transform", tgt, None), ("clone", tgt, None), ("assign", tgt, rebuild), ("recreate", tgt, None),
                                   ("sort", tgt, None)):
        ct, cs = search(rig, which)
        rows = rig.ctx.nn1_fetch(len(cs))
        want_rows = consumer_reference(rig, which)[:2]
        sc.same(rows[0], rows[1], want_rows[0], want_rows[1], which)
        MUTATIONS[mutation](rig.H, handle)
        if then == "sort-C5-for-P3t":
            MUTATIONS["sort"](rig.H, "C5")                                  # (stage_cases.mut_sort orders C5 for P3t)
        elif then:
            rig.check(then, f"after {which}, {mutation}({handle})")
        ct = rig.H.cloud(tgt)
        with pytest.raises(rig.pcr.PcrError, match=state):
            rig.ctx.kabsch_sums(ct, cs, 1.0)
        if then is None or then not in STAGES or not STAGES[then].searches:
            again = rig.ctx.nn1_fetch(len(cs))
            assert sc.canon(again) == sc.canon(rows), f"{which}: the rows of the search changed with {mutation}({handle})"
        ct, cs = search(rig, which)                                         # the pair as it is now
        sc._loop_check(consume(rig, ct, cs), consumer_reference(rig, which), f"{which} after {mutation}({handle}) [{rig.H.tok(handle)}]")
        COUNTS["consumer cases"] += 1
    # the source: moved, or another handle of the same size and content
    ct, cs = search(rig, which)
    rig.ctx.transform(cs, np.eye(4, dtype=np.float32))
    with pytest.raises(rig.pcr.PcrError, match=state):
        rig.ctx.kabsch_sums(ct, cs, 1.0)
    ct, cs = search(rig, which)
    twin = cs.clone()
    with pytest.raises(rig.pcr.PcrError, match=state):
        rig.ctx.kabsch_sums(ct, twin, 1.0)
    twin.free()
    sc._loop_check(consume(rig, ct, cs), consumer_reference(rig, which), f"{which} after a refused twin")


@gpu
def test_refused_calls_leave_tickets_and_accumulators_alone(rig):
    """a call that returns an argument error has touched nothing: the one-wave k-NN ticket, the plane workspace and the loop's accumulators
    serve the next call as before"""
    bad = rig.pcr.ERRORS[-1]
    d, q = rig.H.db64("C5"), rig.H.rows64("S3")
    rig.check("db64_knn_coop", "first")
    for k in (0, 33):
        with pytest.raises(rig.pcr.PcrError, match=bad):
            d.knn(q[:7], k)
        rig.check("db64_knn_coop", f"after a refused k = {k}")
    rig.check("icp_big", "first")
    short = rig.ctx.cloud(rig.inp["N3t"][:, :100].copy())
    with pytest.raises(rig.pcr.PcrError):                                   # (normals of another size: test_p2plane.py)
        rig.ctx.icp_point2plane(rig.H.cloud("P3s"), rig.H.cloud("P3t"), short)
    short.free()
    for name in ("icp_big", "icp_empty", "icp_iter0", "icp_converged", "p2plane_sorted", "icp_iter1", "plane_count_150", "plane_count_20", "plane_count_150"):
        rig.check(name, "after a refused point-to-plane call")


@gpu
def test_one_wave_ticket_is_a_multiple_of_the_batch_size_between_calls(rig):
    """The wave that draws ticket m - 1 modulo m publishes the completion word of a one-wave k-NN call, so every call must find the ticket at a
    multiple of ITS m (include/pcr.h, pcr_ctx_knn_coop_state): with a ticket left over from another m the word goes out while waves still write
    their rows.  Read behind a stream synchronisation after every call of a sequence of changing m, refused calls and other stages in between."""
    t = sc.thresholds()
    d, q = rig.H.db64("C5"), rig.H.rows64("S3")
    calls = rig.ctx.knn_coop_state()["calls"]
    for step, m in enumerate(sc.COOP_M + (1, t.knn_coop_max, 3, 3, 7)):
        for k in (1, 32):
            d.knn(q[:m], k)
            st = rig.ctx.knn_coop_state()
            calls += 1
            assert st["m"] == m and st["calls"] == calls, (step, m, k, st)
            assert st["ticket"] % m == 0 and st["ticket"] <= m * calls, (step, m, k, st)
        if step % 3 == 1:
            with pytest.raises(rig.pcr.PcrError, match=rig.pcr.ERRORS[-1]):
                d.knn(q[:m + 1], 33)
            rig.check("db64_knn_small", "between one-wave calls")           # (17 and 300 queries: not the one-wave route, the same grid)
            assert rig.ctx.knn_coop_state()["calls"] == calls
    rig.check("db64_knn_coop", "after the ticket sequence")
    st = rig.ctx.knn_coop_state()
    assert st["m"] == sc.COOP_M[-1] and st["ticket"] % sc.COOP_M[-1] == 0 and st["calls"] == calls + len(sc.COOP_M) * len(sc.K_SET), st   # (the stage took the one-wave route)


# ---- walks, two contexts ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("seed", WALK_SEEDS)
def test_random_walk(rig, seed):
    steps = walk(seed)
    for k, step in enumerate(steps):
        try:
            if step[0] == "stage":
                rig.check(step[1], f"walk {seed}, step {k}")
            elif step[0] == "mutate":
                MUTATIONS[step[1]](rig.H, step[2])
            else:
                sc.flip(rig.ctx, step[1], step[2])
        except BaseException:
            print(f"walk seed {seed} failed at step {k}; replay with walk({seed})[:{k + 1}]:")
            for j, s in enumerate(steps[:k + 1]):
                print(f"  {j:3d} {s}")
            raise
        COUNTS["walk steps"] += 1
    print(f"random walk {seed}: {len(steps)} steps ({sum(s[0] == 'stage' for s in steps)} stages checked, {sum(s[0] == 'mutate' for s in steps)} mutations, "
          f"{sum(s[0] == 'flip' for s in steps)} tune flips); {COUNTS['walk steps']} steps so far")


@gpu
def test_two_contexts_interleaved(pcr, orc, inp, references, fresh_answers):
    with pcr.Context(0) as c1, pcr.Context(0) as c2:
        H1, H2 = sc.Handles(pcr, c1, inp, orc), sc.Handles(pcr, c2, inp, orc)
        try:
            n = len(KINDS)
            other = np.random.default_rng(5).permutation(n)                 # the second context sees every stage too, in another order
            for k in range(n):
                a, b = KINDS[k], KINDS[int(other[k])]
                run_and_check(pcr, orc, inp, H1, a, f"context 1, call {k}, next to context 2")
                run_and_check(pcr, orc, inp, H2, b, f"context 2, call {k}, next to context 1")
                COUNTS["two-context calls"] += 2
                if k == n // 3:                                             # handles change on one context only
                    MUTATIONS["transform"](H1, "T66")
                    MUTATIONS["recreate"](H2, "C5")
        finally:
            H1.close(); H2.close()
    print(f"two contexts: {COUNTS['two-context calls']} calls checked")


@gpu
def test_zz_report():
    """what this module checked in this run (run with -s)"""
    print("stage interleaving: " + ", ".join(f"{v} {k}" for k, v in COUNTS.items()))
