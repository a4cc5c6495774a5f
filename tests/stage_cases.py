"""The stages that tests/test_stage_interleaving.py runs after one another on ONE context and ONE set of handles.  Not a test module.

A stage is (name, run(ctx, H) -> tuple of arrays and scalars, expect(V) -> the CPU reference, check(got, want, what)).  H (Handles) owns the
device handles of a test and, next to every one, its host MODEL: the array the handle holds now.  A mutation (transform, assign, in-place
sort, free + create, clone, trim) changes handle and model together, so expect() always describes what the device holds: for a moved cloud
that is orc.transform_f32 of the model, followed by the stage's reference.  Expected results are kept in one cache keyed by (stage, the
tokens of the arrays it reads): every reference is computed once per process and never changed (arrays are read-only).

Every check is the comparison of the stage's own test module, with that module's restatement and helpers imported; a bar that is a literal
inside a test function there is repeated here with its origin next to it.  Except for the point-to-plane pose (block-ordered f64 sums,
DESIGN.md) and the order sort_for_target leaves inside a cell (atomic cursors) every result must ALSO equal the same call on a fresh context
bit for bit (test_stage_interleaving.py, `fresh`).

Stages without a CPU reference that can be imported free of GPU calls — the expected answer is the fresh context's:
  pn2_forward   (test_pointnet2_classifier.small_check feeds its restatement the library's own sampling through the public calls)

Inputs, all but ISSM seeded from synth (thresholds(): every size is asserted against the constants in the sources):
  S3 / T66    3 000 source points of a 66 000-point scan: T66 is above the one-shot auto-grid threshold (65 536) and is only ever queried by S3
  P3s / P3t   a 3 000-point pair: above the loop's grid threshold (2 048), below the one-shot one and below 4 096
  C5          5 000 points: above KNN_SMALL_MAX as a query batch, above the 4 096 points a Db64 needs for its f32 twin cloud
  ALT66, ALT5 other scans of the same sizes (assign, free + create)
  descriptor sets of 600 / 500 rows (test_global_registration.scene); ISSM: 4 000 points of the model cloud of tests/golden/iss_hw7.npz"""
import hashlib
import os
import re
from types import SimpleNamespace

import numpy as np

import kabsch_wave_cases
from test_context_state import NONE, same
from test_dataset_build import assert_same as assert_box_rows, drawn_boxes, numpy_aabb, rule_rows
from test_fullsize import THREADS, bits32, bits64
from test_global_registration import scene
from test_ground_fit import masks_agree
from test_fpfh import check_fpfh, check_spfh, fpfh_numpy, spfh_numpy
from test_harris3d import harris_numpy
from test_hw3_spectral_oracle import rs_knn
from test_hw3_clustering import rs_assign, rs_exact_centres
from test_hw4_foreground import assert_dbscan_equal, assert_sor_equal, dbscan_ref, sor_ref
from test_knn_routes import assert_rows, ref_knn
from test_normal_space_sampling import nss_numpy
from test_pointnet_sampling import ball_ref, fps_ref_segments, group_ref
from test_range_clustering import assign_ref, components_ref, edges_ref, label_ref, project_ref, refines
from test_voxel_grid_normals import voxel_grid_numpy
import test_pointnet2_classifier as pn2
import test_pointnet_cls as pn1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hands-on-point-cloud-processing_amd", "csrc")
AOS3 = 1
_G = np.load(os.path.join(ROOT, "tests", "golden", "iss_hw7.npz"))
ICP_POSE_BAR = 1e-5                 # |T - T_oracle|_F: test_context_state.py, test_p2plane.py, __graft_entry__.smoke
POSE = np.array([[0.9998477, -0.0174524, 0.0, 0.25], [0.0174524, 0.9998477, 0.0, -0.125], [0.0, 0.0, 1.0, 0.0625], [0, 0, 0, 1]], np.float32)   # 1 degree about z


# ------------------------------------------------------------------------------------------------------------------ constants in the sources
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1).replace("u", ""))


def thresholds():
    api, knn, f64, internal = _src("api.cpp"), _src("knn_grid.hip"), _src("search_f64.hip"), _src("pcr_internal.hpp")
    return SimpleNamespace(
        loop_grid=_const(api, r"if \(in_loop\) return tgt->n >= (\d+)"),
        oneshot_min=_const(api, r"if \(tgt->n < (\d+)\) return false;"),
        oneshot_grid=_const(api, r"return tgt->n >= (\d+) \|\| \(double\)ns"),
        knn_small_max=_const(internal, r"constexpr size_t KNN_SMALL_MAX = (\d+);"),
        knn_coop_max=_const(knn, r"constexpr size_t KNN_COOP_MAX = (\d+);"),
        twin_min=_const(f64, r"if \(n >= (\d+)\) \{"),
        morton_min=_const(_src("grid.hip"), r"ord == 0 && tgt->n >= (\d+)\)\) \? GRID_ORDER_MORTON"),
    )


# ------------------------------------------------------------------------------------------------------------------ inputs
_IN = {}
SIZES = (500, 20000)                    # below and far above every other query batch: keys[], wpos, far_list, scratch and the parked buffers grow and are reused


def frozen(a):
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a


def inputs(synth, orc):
    if _IN:
        return _IN
    S3, T66 = synth.kitti_like_pair(66000, n_src=3000)
    P3s, P3t = synth.kitti_like_pair(3000, seed_target=211, seed_pair=212)
    C5 = synth.kitti_like_scan(5000, seed=213)
    d = dict(S3=S3, T66=T66, P3s=P3s, P3t=P3t, C5=C5, ALT66=synth.kitti_like_scan(66000, seed=214), ALT5=synth.kitti_like_scan(5000, seed=215))
    d["ALT3"] = synth.kitti_like_pair(3000, seed_target=219, seed_pair=220)[1]
    d.update(BASE66=T66, BASE5=C5, BASE3=P3t)
    d["N3t"] = np.ascontiguousarray(orc.normals_knn_f64(P3t, 10, 5.0).astype(np.float32).T)       # target normals of the point-to-plane loop
    d["N_ALT3"] = np.ascontiguousarray(orc.normals_knn_f64(d["ALT3"], 10, 5.0).astype(np.float32).T)
    for n in SIZES:                     # the size walks: the first n points of another scan as queries of P3t
        d[f"Z{n}"] = d["ALT66"][:, :n]
    d["NC5"] = np.ascontiguousarray(orc.normals_knn_f64(C5, 10, 5.0).astype(np.float32).T)
    gs, gt, dsrc, dtgt, _, _ = scene(31, 600, 500, 250)
    d.update(GS=gs, GT=gt, DS=dsrc, DT=dtgt)
    rng = np.random.default_rng(216)
    d["PLANES"] = np.stack([orc.plane_from_3pts(C5.T[rng.choice(5000, 3, replace=False)].astype(np.float64)) for _ in range(200)])
    d["PLANES"] = d["PLANES"][np.isfinite(d["PLANES"]).all(1)]
    d["BOXES"] = drawn_boxes(rng, 9) * np.r_[np.ones(12), np.full(3, 4.0)]                        # extents 1.2 ... 10, centred on points of their segment
    d["BOXES"][:, :3] = C5.T[[100, 101, 900, 1500, 0, 1, 2000, 2001, 4000]]
    d["KSUMS"] = np.concatenate([np.stack([s for _, s in kabsch_wave_cases.constructed(synth)]), kabsch_wave_cases.seeded(70, seed=11)])
    d["M2"] = C5[:, :2000]                                                                         # the rows of the Mat64 k-NN (an n x n restatement)
    d["ISSM"] = np.ascontiguousarray(_G["xyz_airplane_0001"][:4000].T.astype(np.float32))
    d["PN2OBJ"] = pn2.small_inputs(5, 33, 38)
    d["PN1OBJ"] = np.random.default_rng(217).uniform(-1, 1, (5, 65, 3)).astype(np.float32)
    _IN.update({k: frozen(v) for k, v in d.items()})
    return _IN


class View:
    """the host side of a set of handles: arr(name) = what the handle holds now, tok(name) = a name for that content"""

    def __init__(self, inp, orc, pcr=None):
        self.inp, self.orc, self.pcr = inp, orc, pcr
        self.host, self.token = {}, {}

    def arr(self, name):
        return self.host.get(name, self.inp[name])

    def rows64(self, name):
        return np.ascontiguousarray(self.arr(name).T.astype(np.float64))

    def rows32(self, name):
        return np.ascontiguousarray(self.arr(name).T)

    def tok(self, name):
        return self.token.get(name, name)

    def set(self, name, array, token):
        self.host[name], self.token[name] = frozen(array), token


class Handles(View):
    """device handles next to their host model; created on first use, so a fresh context uploads only what its stage reads"""

    def __init__(self, pcr, ctx, inp, orc):
        super().__init__(inp, orc, pcr)
        self.ctx, self.dev, self.other = ctx, {}, {}

    def cloud(self, name):
        if name not in self.dev:
            self.dev[name] = self.ctx.cloud(self.arr(name))
        return self.dev[name]

    def db64(self, name):
        key = "db64:" + name
        if key not in self.other or self.other[key][1] != self.tok(name):
            if key in self.other:
                self.other[key][0].free()
            self.other[key] = (self.ctx.db64(self.rows64(name)), self.tok(name))
        return self.other[key][0]

    def mat64(self, name):
        key = "mat64:" + name
        if key not in self.other or self.other[key][1] != self.tok(name):
            if key in self.other:
                self.other[key][0].free()
            self.other[key] = (self.ctx.mat64(self.rows64(name)), self.tok(name))
        return self.other[key][0]

    def model(self, which):
        if which not in self.other:
            mod = pn2 if which == "pn2" else pn1
            m = mod.small_model()
            self.other[which] = ((self.ctx.pn2_model if which == "pn2" else self.ctx.pn1_model)(mod.desc_of(self.pcr, m), mod.flat(m)), m)
        return self.other[which][0]

    def close(self):
        for h, _ in self.other.values():
            h.free()
        for c in self.dev.values():
            c.free()
        self.other, self.dev = {}, {}


# ------------------------------------------------------------------------------------------------------------------ mutations
ALT = {"T66": "ALT66", "C5": "ALT5", "P3t": "ALT3"}         # "a different cloud of equal size"; back to the first content the next time
BASE = {"T66": "BASE66", "C5": "BASE5", "P3t": "BASE3"}     # handles of their own that hold the first content (assign copies from a handle)
NORMALS_OF = {"P3t": "N3t"}                                 # the point-to-plane loop pairs P3t with its normals by index: they follow its points and order
NORMALS = {"ALT3": "N_ALT3", "BASE3": "N3t"}


def _other(H, name):
    return ALT[name] if H.tok(name) != ALT[name] else BASE[name]


def _token(name, other):
    return name if other == BASE[name] else other          # the first content goes by the handle's own name again: the references are shared


def _follow(H, name, other=None, orig=None):
    """the normals of `name` become those of its new content (other) or take its new order (orig): free + create"""
    nrm = NORMALS_OF.get(name)
    if nrm is None:
        return
    if nrm in H.dev:
        H.dev.pop(nrm).free()
    if other is not None:
        H.set(nrm, H.inp[NORMALS[other]], NORMALS[other])
    else:
        H.set(nrm, H.arr(nrm)[:, orig], H.tok(nrm) + "^" + hashlib.sha1(orig.tobytes()).hexdigest()[:12])


def mut_transform(H, name):
    H.ctx.transform(H.cloud(name), POSE)
    H.set(name, H.orc.transform_f32(H.arr(name), POSE[:3, :3], POSE[:3, 3]), H.tok(name) + "@")


def mut_assign(H, name):
    other = _other(H, name)
    H.cloud(name).assign(H.cloud(other))
    H.set(name, H.inp[other], _token(name, other))
    _follow(H, name, other=other)


def mut_sort(H, name):
    tgt = "C5" if name != "C5" else "P3t"
    orig = H.ctx.sort_for_target(H.cloud(tgt), H.cloud(name))
    assert np.array_equal(np.sort(orig), np.arange(orig.size, dtype=np.uint32))
    # (the order inside a cell differs from run to run: the content is named by the order itself, never by how it came about)
    H.set(name, H.arr(name)[:, orig], H.tok(name) + "^" + hashlib.sha1(orig.tobytes()).hexdigest()[:12])
    _follow(H, name, orig=orig)


def mut_recreate(H, name):
    """free, then at once another cloud of the same size: the allocator may hand back the address and the parked buffer"""
    other = _other(H, name)
    H.cloud(name).free()
    H.dev[name] = H.ctx.cloud(H.inp[other])
    H.set(name, H.inp[other], _token(name, other))
    _follow(H, name, other=other)


def reset(H, name):
    """the handle back on its first content (free + create), unless it holds it"""
    if H.tok(name) != name:
        H.cloud(name).free()
        H.dev[name] = H.ctx.cloud(H.inp[name])
        H.set(name, H.inp[name], name)
        _follow(H, name, other=BASE[name])


def mut_clone(H, name):
    old = H.cloud(name)
    H.dev[name] = old.clone()
    old.free()


def mut_trim(H, name):
    H.ctx.trim()


MUTATIONS = {"transform": mut_transform, "assign": mut_assign, "sort": mut_sort, "recreate": mut_recreate, "clone": mut_clone, "trim": mut_trim}
MUTABLE = ("T66", "C5", "P3t")
# grid_tile 1 (the tile search forced on a target of any size) stays with its own tests, which run it on 30 000 points and more
TUNE_FLIPS = (("grid_order", 1), ("grid_order", 2), ("nn_method", 1), ("nn_method", 2), ("knn_cell_scale_x100", 150), ("knn_cell_scale_x100", 200), ("grid_tile", 2))


# ------------------------------------------------------------------------------------------------------------------ the table
STAGES = {}
_EXPECT = {}


def add(name, run, expect, check, uses, caches=(), fresh_equal=True, searches=False):
    """uses: the model arrays expect() reads.  caches: the handles whose cached indices the stage reads or builds (the targets of a mutation
    test).  searches: the stage writes the context's correspondence workspace"""
    assert name not in STAGES
    STAGES[name] = SimpleNamespace(name=name, run=run, expect=expect, check=check, uses=tuple(uses), caches=tuple(caches), fresh_equal=fresh_equal,
                                   searches=searches)


def expected(stage, V):
    key = (stage.name,) + tuple(V.tok(n) for n in stage.uses)
    if key not in _EXPECT:
        _EXPECT[key] = stage.expect(V)
    return _EXPECT[key]


def canon(res):
    """a result as bytes, for bit-for-bit comparison between contexts"""
    out = []
    for r in res if isinstance(res, (tuple, list)) else (res,):
        if isinstance(r, (tuple, list)):
            out.append(canon(r))
        elif isinstance(r, dict):
            out.append(canon([r[k] for k in sorted(r)]))
        else:
            a = np.ascontiguousarray(r)
            out.append((str(a.dtype), a.shape, a.tobytes()))
    return out


FLIPS = {}                              # (id(ctx), key) -> the value a walk has flipped the key to: a stage puts its own tunes back to that


def flip(ctx, key, value):
    FLIPS[(id(ctx), key)] = value
    ctx.tune(key, value)


def unflip(ctx):
    for (c, key) in [k for k in FLIPS if k[0] == id(ctx)]:
        ctx.tune(key, 0)
        del FLIPS[(c, key)]


def tuned(ctx, **tunes):
    class _T:
        def __enter__(self):
            for k, v in tunes.items():
                ctx.tune(k, v)

        def __exit__(self, *exc):
            for k in tunes:
                ctx.tune(k, FLIPS.get((id(ctx), k), 0))
    return _T()


def equal_all(got, want, what):
    """every part equal bit for bit (the reference's values in the dtype the library returns them in)"""
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g = np.ascontiguousarray(g)
        w = np.ascontiguousarray(w).astype(g.dtype)
        assert g.size == w.size, f"{what}: part {k} has {g.size} entries, the reference {w.size}"
        bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)) // max(g.dtype.itemsize, 1)
        assert bad.size == 0, f"{what}: part {k} differs at {np.unique(bad)[:5]}: {g.reshape(-1)[np.unique(bad)[:5]]} against {w.reshape(-1)[np.unique(bad)[:5]]}"


# ---- 1-NN ------------------------------------------------------------------------------------------------------------------------------
def _nn1_expect(tgt, src):
    return lambda V: V.orc.nn1_f32_mt(V.arr(tgt), V.arr(src), threads=THREADS)


def _nn1_check(got, want, what):
    same(got[0], got[1], want[0], want[1], what)


def _nn1_run(method, tgt, src, fetch=False):
    def run(ctx, H):
        with tuned(ctx, nn_method=method):
            if not fetch:
                return ctx.nn1(H.cloud(tgt), H.cloud(src))
            ctx.nn1_async(H.cloud(tgt), H.cloud(src))
            return ctx.nn1_fetch(len(H.cloud(src)))
    return run


for _m in (0, 1, 2):
    add(f"nn1_m{_m}", _nn1_run(_m, "T66", "S3"), _nn1_expect("T66", "S3"), _nn1_check, ("T66", "S3"), ("T66",), searches=True)
# the small pair on the library's own choice: exhaustive on a target without an index, the grid once another stage has left one there
add("nn1_small_auto", _nn1_run(0, "P3t", "P3s"), _nn1_expect("P3t", "P3s"), _nn1_check, ("P3t", "P3s"), ("P3t",), searches=True)
add("nn1_async_fetch", _nn1_run(0, "T66", "S3", True), _nn1_expect("T66", "S3"), _nn1_check, ("T66", "S3"), ("T66",), searches=True)


def _gated(V, tgt, src, gate):
    oidx, od2 = V.orc.nn1_f32_mt(V.arr(tgt), V.arr(src), threads=THREADS)
    inside = od2 < np.float32(gate)
    gi, gd = np.where(inside, oidx, NONE).astype(np.uint32), np.where(inside, od2, np.float32(np.inf)).astype(np.float32)
    sums, last = V.orc.kabsch_accumulate(V.arr(src), V.arr(tgt), gi, gd, gate)
    return gi, gd, sums, last


def _loop_run(method, tgt, src):
    def run(ctx, H):
        with tuned(ctx, nn_method=method):
            ct, cs = H.cloud(tgt), H.cloud(src)
            ctx.nn1_loop(ct, cs, 1.0)
            sums, last, last_d2 = ctx.kabsch_sums(ct, cs, 1.0)
            idx, d2 = ctx.nn1_fetch(len(cs))
            return idx, d2, sums, np.int64(last), np.float32(last_d2)
    return run


def _loop_check(got, want, what):
    idx, d2, sums, last, last_d2 = got
    gi, gd, osums, olast = want
    same(idx, d2, gi, gd, what)
    assert last == olast and int(sums[15]) == int(osums[15]), (what, last, olast, sums[15], osums[15])                      # test_context_state.py §B
    assert np.allclose(sums, osums, rtol=1e-13, atol=0), what                                       # test_gpu_parity.py::test_kabsch_sums_vs_oracle
    assert olast < 0 or bits32(last_d2) == bits32(gd[olast]), what


add("loop_sums_grid", _loop_run(2, "P3t", "P3s"), lambda V: _gated(V, "P3t", "P3s", 1.0), _loop_check, ("P3t", "P3s"), ("P3t",), searches=True)
add("loop_sums_brute", _loop_run(1, "P3t", "P3s"), lambda V: _gated(V, "P3t", "P3s", 1.0), _loop_check, ("P3t", "P3s"), ("P3t",), searches=True)
add("loop_sums_big", _loop_run(0, "T66", "S3"), lambda V: _gated(V, "T66", "S3", 1.0), _loop_check, ("T66", "S3"), ("T66",), searches=True)


# the same stages at other batch sizes (test_stage_interleaving.py, size walks): not part of KINDS
SIZED = {}
for _n in SIZES:
    _z = f"Z{_n}"
    SIZED[_n] = (SimpleNamespace(name=f"nn1_m0_{_n}", run=_nn1_run(0, "P3t", _z), expect=_nn1_expect("P3t", _z), check=_nn1_check, uses=("P3t", _z)),
                 SimpleNamespace(name=f"nn1_m1_{_n}", run=_nn1_run(1, "P3t", _z), expect=_nn1_expect("P3t", _z), check=_nn1_check, uses=("P3t", _z)),
                 SimpleNamespace(name=f"nn1_m2_{_n}", run=_nn1_run(2, "P3t", _z), expect=_nn1_expect("P3t", _z), check=_nn1_check, uses=("P3t", _z)),
                 SimpleNamespace(name=f"loop_sums_grid_{_n}", run=_loop_run(2, "P3t", _z), expect=lambda V, z=_z: _gated(V, "P3t", z, 1.0), check=_loop_check, uses=("P3t", _z)),
                 SimpleNamespace(name=f"loop_sums_brute_{_n}", run=_loop_run(1, "P3t", _z), expect=lambda V, z=_z: _gated(V, "P3t", z, 1.0), check=_loop_check, uses=("P3t", _z)))


# ---- ICP -------------------------------------------------------------------------------------------------------------------------------
STAT_KEYS = ("iters_run", "converged", "empty_pairs", "last_pairs")


def _icp(name, src, tgt, **kw):
    def run(ctx, H):
        T, st = ctx.icp_point2point(H.cloud(src), H.cloud(tgt), **kw)
        return T, np.array([st[k] for k in STAT_KEYS], np.int64), np.float32(st["last_loss"])

    def expect(V):
        return V.orc.icp_p2p_f32(V.arr(src), V.arr(tgt), **kw)

    def check(got, want, what):
        T, st, _ = got
        oT, ost = want
        assert st.tolist() == [ost[k] for k in STAT_KEYS], (what, st.tolist(), ost)
        assert np.linalg.norm(T.astype(np.float64) - oT.astype(np.float64)) <= ICP_POSE_BAR, (what, T, oT)
    add(name, run, expect, check, (src, tgt), (tgt,), searches=True)


_icp("icp_iter0", "P3s", "P3t", max_corr=1.0, max_iter=0, eps=1e-8)
_icp("icp_iter1", "P3s", "P3t", max_corr=1.0, max_iter=1, eps=1e-8)
_icp("icp_converged", "P3s", "P3t", max_corr=1.0, max_iter=40, eps=1e30)
_icp("icp_empty", "P3s", "P3t", max_corr=1e-30, max_iter=5, eps=1e-8)
_icp("icp_big", "S3", "T66", max_corr=1.0, max_iter=3, eps=1e-8)


def _p2plane(name, sort_work):
    kw = dict(max_corr=1.0, max_iter=4, eps=0.0)

    def run(ctx, H):
        with tuned(ctx, p2plane_sort_work=sort_work):
            T, st = ctx.icp_point2plane(H.cloud("P3s"), H.cloud("P3t"), H.cloud("N3t"), **kw)
        return T, np.array([st[k] for k in STAT_KEYS], np.int64), np.float64(st["last_loss"])

    def check(got, want, what):                                                                     # test_p2plane.py::test_gpu_p2plane_matches_oracle
        T, st, loss = got
        oT, ost = want
        assert np.linalg.norm(T.astype(np.float64) - oT.astype(np.float64)) <= ICP_POSE_BAR, (what, T, oT)
        assert st.tolist() == [ost[k] for k in STAT_KEYS], (what, st.tolist(), ost)
        assert abs(loss - ost["last_loss"]) <= 1e-5 * max(1.0, abs(ost["last_loss"])), what
    add(name, run, lambda V: V.orc.icp_p2plane_f32(V.arr("P3s"), V.arr("P3t"), V.arr("N3t"), **kw), check, ("P3s", "P3t", "N3t"), ("P3t",), fresh_equal=False,
        searches=True)


_p2plane("p2plane_sorted", 1)
_p2plane("p2plane_unsorted", 2)


def _sort_run(ctx, H):
    work = H.cloud("S3").clone()
    try:
        orig = ctx.sort_for_target(H.cloud("T66"), work)
        return orig, work.numpy()
    finally:
        work.free()


def _sort_check(got, want, what):
    orig, pts = got
    assert np.array_equal(np.sort(orig), np.arange(orig.size, dtype=np.uint32)), what
    assert np.array_equal(bits32(pts), bits32(want[:, orig])), what


# (below 65 536 points the order INSIDE a cell is the order in which the scatter's atomic cursors were taken, csrc/grid.hip scatter_perm_kernel: a valid
# sort, another one every run — no bits to compare with a fresh context; everything computed from a sorted cloud is free of its order)
add("sort_for_target", _sort_run, lambda V: V.arr("S3"), _sort_check, ("S3",), ("T66",), fresh_equal=False)


def _shard_run(ctx, H):
    out = []
    for rank in (0, 1):
        sh = ctx.shard_spatial(H.cloud("T66"), H.cloud("S3"), 2, rank, 5)
        out += [ctx.global_index(sh), sh.numpy()]
        sh.free()
    return tuple(out)


def _shard_check(got, want, what):                                                                  # test_context_state.py §C
    g0, p0, g1, p1 = got
    for gi, pts in ((g0, p0), (g1, p1)):
        assert gi.size > 0 and (np.diff(gi.astype(np.int64)) > 0).all() and np.array_equal(bits32(pts), bits32(want[:, gi])), what
    assert np.array_equal(np.sort(np.concatenate([g0, g1])), np.arange(want.shape[1], dtype=np.uint32)), what


add("shard_spatial", _shard_run, lambda V: V.arr("S3"), _shard_check, ("S3",), ("T66",))


def _kabsch_batch_expect(V):
    sums = V.inp["KSUMS"]
    rc, R, t = np.zeros(len(sums), np.int32), np.zeros((len(sums), 3, 3), np.float32), np.zeros((len(sums), 3), np.float32)
    for i, s in enumerate(sums):
        rc[i], R[i], t[i] = V.pcr.kabsch_solve(s)
    return rc, R, t


add("kabsch_batch", lambda ctx, H: ctx.kabsch_solve_batch_device(H.inp["KSUMS"]), _kabsch_batch_expect, equal_all, ())          # test_kabsch_wave_gpu.py: bits


# ---- k-NN, radius, PCA -----------------------------------------------------------------------------------------------------------------
K_SET = (1, 4, 10, 32)
KNN_CAP = 1.5


def _knn_slices(ref, squared):
    idx, val, found = ref
    return tuple((idx[:, :k], val[:, :k], np.minimum(found, k).astype(np.uint32)) for k in K_SET)


def _knn_check(got, want, what):
    for k, g, w in zip(K_SET, got, want):
        assert_rows(g, w[:len(g)], f"{what}, k {k}")


add("cloud_knn_resident", lambda ctx, H: tuple(ctx.cloud_knn(H.cloud("P3t"), H.cloud("C5"), k, KNN_CAP) for k in K_SET),
    lambda V: _knn_slices(ref_knn(V.rows64("P3t"), V.rows64("C5"), 32, KNN_CAP, True), True), _knn_check, ("P3t", "C5"), ("P3t",))
add("cloud_knn_self", lambda ctx, H: tuple(ctx.cloud_knn(H.cloud("C5"), H.cloud("C5"), k, KNN_CAP) for k in K_SET),
    lambda V: _knn_slices(ref_knn(V.rows64("C5"), V.rows64("C5"), 32, KNN_CAP, True), True), _knn_check, ("C5",), ("C5",))

COOP_M = (12, 5, 16, 12)                # the one-wave route's ticket counts modulo the last m


def _db_queries(V, m):
    """a handful of queries for the one-wave route: the first three inside the scan, the others hundreds of metres outside it — their waves walk
    for long after the first ones have drawn their tickets, so a completion word published by a wrong ticket is read with rows still missing"""
    if m > 300:
        return V.rows64("ALT5")
    q = V.rows64("S3")[:m].copy()
    if m <= 16:
        q[3:] += (300.0, 300.0, 50.0)
    return q.astype(np.float32).astype(np.float64)          # (f32-representable, or the handle answers with its exhaustive scan)


def _db_knn(ms):
    def run(ctx, H):
        d = H.db64("C5")
        return tuple(tuple(d.knn(_db_queries(H, m), k) for k in K_SET) for m in ms)

    def expect(V):
        return tuple(_knn_slices(ref_knn(V.rows64("C5"), _db_queries(V, m), 32, -1.0, False), False) for m in ms)

    def check(got, want, what):
        for m, g, w in zip(ms, got, want):
            _knn_check(g, w, f"{what}, {m} queries")
    return run, expect, check


add("db64_knn_coop", *_db_knn(COOP_M), ("C5", "S3"), ("C5",))
add("db64_knn_small", *_db_knn((17, 300)), ("C5", "S3"), ("C5",))
add("db64_knn_batch", *_db_knn((5000,)), ("C5", "ALT5"), ("C5",))


def _normals_check(got, want, what):                                                                # test_knn_grid.py::test_gpu_normals_match_oracle
    zero = (want == 0).all(1)
    assert np.array_equal(zero, (got == 0).all(1)), what
    err = np.linalg.norm(got - want, axis=1)
    assert np.median(err) < 1e-12 and (err < 1e-6).mean() > 0.99, what
    assert np.allclose(np.linalg.norm(got[~zero], axis=1), 1.0, atol=1e-9), what


add("normals", lambda ctx, H: ctx.normals(H.cloud("C5"), 10, 5.0), lambda V: V.orc.normals_knn_f64(V.arr("C5"), 10, 5.0), _normals_check, ("C5",), ("C5",))


def _eq_rows(got, want, what):                                                                      # test_gpu_parity.py: radius / knn rows against the oracle
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert np.array_equal(g, w) if g.dtype.kind in "iu" else np.array_equal(bits64(g), bits64(w)), what


add("knn_f64", lambda ctx, H: ctx.knn_f64(H.rows64("C5"), H.rows64("S3")[:300], 8), lambda V: V.orc.knn_f64(V.rows64("C5"), V.rows64("S3")[:300], 8), _eq_rows,
    ("C5", "S3"))
RADII = (0.5, 1.25)
for _r in RADII:
    add(f"radius_f64_r{_r}", lambda ctx, H, r=_r: ctx.radius_f64(H.rows64("C5"), H.rows64("C5")[::7], r),
        lambda V, r=_r: V.orc.radius_f64(V.rows64("C5"), V.rows64("C5")[::7], r), _eq_rows, ("C5",))
    add(f"db64_radius_r{_r}", lambda ctx, H, r=_r: H.db64("C5").radius(H.rows64("C5")[::7], r),
        lambda V, r=_r: V.orc.radius_f64(V.rows64("C5"), V.rows64("C5")[::7], r), _eq_rows, ("C5",), ("C5",))


def _rows_run(ctx, H):
    R = H.db64("C5").radius_rows(None, RADII[0])
    try:
        idx, dist = R.fetch(0, R.m)
        mean, cov = R.moments()
        return R.row_ptr(), idx, dist, R.reduce(R.COUNT), R.reduce(R.MAX_DIST), R.reduce(R.SUM_DIST), mean, cov
    finally:
        R.free()


def _rows_check(got, want, what):                                                                   # test_rows.py
    row, idx, dist, cnt, mx, sm, mean, cov = got
    orow, oidx, odist = want[0]
    db = want[1]
    assert np.array_equal(row, orow) and np.array_equal(idx, oidx) and np.array_equal(bits64(dist), bits64(odist)), what
    assert np.array_equal(cnt, np.diff(orow).astype(np.float64)), what
    nz = np.diff(orow) > 0
    assert np.array_equal(mx[nz], np.maximum.reduceat(odist, orow[:-1][nz])), what
    assert np.allclose(sm[nz], np.add.reduceat(odist, orow[:-1][nz]), rtol=1e-12, atol=0) and (sm[~nz] == 0).all(), what
    for i in range(0, len(db), 125):
        nb = db[oidx[orow[i]:orow[i + 1]]]
        m = nb.mean(axis=0)
        c = (nb - m).T @ (nb - m) / nb.shape[0]
        assert np.allclose(mean[i], m, rtol=1e-12, atol=1e-12), what
        assert np.allclose(cov[i], [c[0, 0], c[0, 1], c[0, 2], c[1, 1], c[1, 2], c[2, 2]], rtol=1e-9, atol=1e-12), what


add("db64_radius_rows", _rows_run, lambda V: (V.orc.radius_f64(V.rows64("C5"), V.rows64("C5"), RADII[0]), V.rows64("C5")), _rows_check, ("C5",), ("C5",))


def _pca_expect(V):
    data = V.rows64("C5")
    centre = np.sum(data, axis=0) / data.shape[0]
    cd = np.subtract(data, centre)
    ew, ev = np.linalg.eigh(cd.transpose().dot(cd))
    return centre, ew, ev


def _pca_check(got, want, what):                                                                    # test_knn_grid.py::test_gpu_cloud_pca_matches_numpy
    (w, v, c), (centre, ew, ev) = got, want
    assert np.allclose(c, centre, rtol=1e-12, atol=1e-12) and np.allclose(w, ew[::-1], rtol=1e-10), what
    for k in range(3):
        assert abs(v[:, k] @ ev[:, 2 - k]) > 1 - 1e-8, what
    assert np.allclose(v.T @ v, np.eye(3), atol=1e-12), what


add("pca", lambda ctx, H: ctx.pca(H.cloud("C5")), _pca_expect, _pca_check, ("C5",), ("C5",))


# ---- hw9 front and global registration -------------------------------------------------------------------------------------------------
def _voxel_run(ctx, H):
    f = ctx.voxel_filter(H.cloud("C5"), 0.5)
    try:
        return (f.numpy(),)
    finally:
        f.free()


add("voxel_filter", _voxel_run, lambda V: (V.orc.voxel_filter_f32(V.arr("C5"), 0.5),), equal_all, ("C5",))                      # test_voxel_filter.py: bits


def _clouds_rows(c):
    return np.ascontiguousarray(c.numpy().T).reshape(-1, 3) if len(c) else np.zeros((0, 3), np.float32)


def _vgn_run(ctx, H):
    oc, on, vop, cnt = ctx.voxel_grid_normals(H.cloud("C5"), H.cloud("NC5"), 0.75, 1)
    try:
        return _clouds_rows(oc), _clouds_rows(on), vop, cnt.astype(np.int64)
    finally:
        oc.free(); on.free()


def _vgn_expect(V):
    wc, wn, wvop, wcnt = voxel_grid_numpy(V.rows32("C5"), V.rows32("NC5"), 0.75, 1)
    return wc, wn, wvop, np.asarray(wcnt, np.int64)


add("voxel_grid_normals", _vgn_run, _vgn_expect, equal_all, ("C5", "NC5"))                         # test_random_sweeps_stages.check_voxel_grid: bits

# (the model cloud and the radii of test_iss.py, whose bar this is: on the sparse rings of a 5 000-point scan most neighbourhoods are close to
# collinear and the smallest eigenvalue has no six digits to compare)
ISS = dict(local_radius=float(_G["local_r"]), non_max_radius=float(_G["nms_r"]))


def _iss_check(got, want, what):                                                                    # test_iss.check_gpu_against_oracle
    idx, l3, cnt = got
    okey, ol3, row = want
    assert np.array_equal(cnt, np.diff(row).astype(np.uint32)), what
    flip = (l3 == -1) != (ol3 == -1)
    assert flip.sum() <= max(1, l3.size // 2000), what
    both = (l3 != -1) & (ol3 != -1)
    assert np.allclose(l3[both], ol3[both], rtol=1e-6, atol=0) and (bits32(l3[both]) == bits32(ol3[both])).mean() > 0.999, what
    if not flip.any() and np.array_equal(bits32(l3), bits32(ol3)):
        assert np.array_equal(idx, np.flatnonzero(okey)), what


add("iss_keypoints", lambda ctx, H: ctx.iss_keypoints(H.cloud("ISSM"), ISS["local_radius"], ISS["non_max_radius"]),
    lambda V: V.orc.iss_f32(V.arr("ISSM"), ISS["local_radius"], ISS["non_max_radius"], 0.9, 0.9, 5, True) + (V.orc.radius_f32(V.rows32("ISSM"), V.rows32("ISSM"), ISS["local_radius"])[0],),
    _iss_check, ("ISSM",))


def _harris_run(ctx, H):
    idx, resp, cnt = ctx.harris3d(H.cloud("C5"), H.cloud("NC5"), 1.0, 1e-8, 0, True)
    key = np.zeros(len(resp), bool)
    key[idx] = True
    return key, resp, cnt


def _harris_check(got, want, what):                                                                 # test_random_sweeps_stages.check_harris
    key, resp, cnt = got
    wkey, rr, rc = want
    assert np.array_equal(cnt, rc) and np.array_equal(bits32(resp), bits32(rr)) and np.array_equal(key, wkey), what


add("harris3d", _harris_run, lambda V: harris_numpy(V.rows32("C5"), V.rows32("NC5"), 1.0, 1e-8, 0, True), _harris_check, ("C5", "NC5"), ("C5",))


FPFH_R = 1.0
_FPFH_REF = {}


def _fpfh_check(got, want, what):                                                                   # test_fpfh.run_all_cases
    (fp, cnt, sp), (sp_ref, cnt_ref, fragile, pts) = got, want
    assert np.array_equal(cnt, cnt_ref), what
    excused = check_spfh(sp, sp_ref, fragile, what)
    sp_use = sp_ref.copy()
    sp_use[excused] = sp[excused]
    key = (id(sp_ref), excused.tobytes())                   # (the restatement's second pass, once per reference and set of excused rows)
    if key not in _FPFH_REF:
        _FPFH_REF[key] = fpfh_numpy(pts, sp_use, FPFH_R)
    ref, rc = _FPFH_REF[key]
    assert np.array_equal(cnt, rc), what
    check_fpfh(fp, ref, what)


add("fpfh33", lambda ctx, H: ctx.fpfh33(H.cloud("C5"), H.cloud("NC5"), FPFH_R, spfh=True),
    lambda V: tuple(spfh_numpy(V.rows32("C5"), V.rows32("NC5"), FPFH_R)) + (V.rows32("C5"),), _fpfh_check, ("C5", "NC5"), ("C5",))


def _nss_run(ctx, H):
    idx, sc = ctx.normal_space_sample(H.cloud("NC5"), (10, 10, 10), 700, 5, gather=(H.cloud("C5"),))
    try:
        return idx, _clouds_rows(sc)
    finally:
        sc.free()


def _nss_expect(V):
    idx = nss_numpy(V.rows32("NC5"), (10, 10, 10), 700, 5)
    return np.asarray(idx, np.uint32), V.rows32("C5")[idx]


add("normal_space_sample", _nss_run, _nss_expect, equal_all, ("C5", "NC5"))                        # test_random_sweeps_stages: indices and gathered bits


def _pairs(V):
    return V.orc.match_union_f32(V.inp["DS"], V.inp["DT"], 0.5)[0]


def _quads(V):
    return V.pcr.ransac_sample_quads(V.inp["GS"], _pairs(V), 800, 99)


def _poses(V):
    rng = np.random.default_rng(218)
    Rt = np.zeros((64, 12), np.float32)
    for h in range(64):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        Rt[h, :9], Rt[h, 9:] = q.reshape(9), rng.normal(0, 3, 3)
    return Rt


add("nn1_desc", lambda ctx, H: ctx.nn1_desc(H.inp["DS"], H.inp["DT"]), lambda V: V.orc.nn1_dim_f32(V.inp["DS"], V.inp["DT"]), equal_all, ())      # test_global_registration.py: bits
add("match_union", lambda ctx, H: ctx.match_union(H.inp["DS"], H.inp["DT"], 0.5), lambda V: V.orc.match_union_f32(V.inp["DS"], V.inp["DT"], 0.5), equal_all, ())
add("match_inter", lambda ctx, H: ctx.match_inter(H.inp["DS"], H.inp["DT"], 0.5), lambda V: V.orc.match_inter_f32(V.inp["DS"], V.inp["DT"], 0.5), equal_all, ())
add("consensus_count", lambda ctx, H: (ctx.consensus_count(H.inp["GS"], H.inp["GT"], _pairs(H), _poses(H), 2.0),),
    lambda V: (np.array([V.orc.consensus_count_f32(V.inp["GS"], V.inp["GT"], _pairs(V), p[:9], p[9:], 2.0) for p in _poses(V)], np.uint32),), equal_all, ())


def _ransac_run(ctx, H):
    win, R, t, best, counts = ctx.ransac_global(H.inp["GS"], H.inp["GT"], _pairs(H), _quads(H), 0.3)
    return np.int64(win), R, t, np.int64(best), counts


def _ransac_expect(V):
    ow, oR, ot, obest, ocounts = V.orc.ransac_global_f32(V.inp["GS"], V.inp["GT"], _pairs(V), _quads(V), 0.3)
    return np.int64(ow), oR, ot, np.int64(obest), ocounts


add("ransac_global", _ransac_run, _ransac_expect, equal_all, ())                                    # test_global_registration.py: counts, winner, pose bits


# ---- hw4 and hw3 -----------------------------------------------------------------------------------------------------------------------
for _n in (20, 150):                    # the workspace ticket after another number of hypotheses (more than one launch at 150)
    add(f"plane_count_{_n}", lambda ctx, H, n=_n: (ctx.plane_count(H.cloud("C5"), H.inp["PLANES"][:n], 0.15),),
        lambda V, n=_n: (np.asarray(V.orc.plane_count(V.arr("C5"), V.inp["PLANES"][:n], 0.15), np.int64),), equal_all, ("C5",))
add("plane_mask", lambda ctx, H: (lambda r: (r[0], np.int64(r[1])))(ctx.plane_mask(H.cloud("C5"), H.inp["PLANES"][3], 0.15)),
    lambda V: (lambda m: (np.asarray(m, np.uint8), np.int64(np.count_nonzero(m))))(V.orc.plane_mask(V.arr("C5"), V.inp["PLANES"][3], 0.15)), equal_all, ("C5",))
add("ground_seeds", lambda ctx, H: (lambda r: (r[0], np.float64(r[1])))(ctx.ground_seeds(H.cloud("C5"), 500, 0.2)),
    lambda V: (lambda r: (r[0].astype(bool), np.float64(r[1])))(V.orc.ground_seeds_f64(V.arr("C5"), 500, 0.2)), equal_all, ("C5",))          # test_ground_fit.py: mask and bound, bits


def _ground_check(got, want, what):                                                                 # test_ground_fit.py::test_gpu_ground_detection...
    (params, mask), (oparams, omask, _, soa) = got, want
    assert np.allclose(params, oparams, rtol=0, atol=1e-9), what
    ok, ndiff = masks_agree(oparams, soa.T, mask, omask, 0.2)
    assert ok and ndiff <= 2, what


add("ground_detection", lambda ctx, H: ctx.ground_detection(H.cloud("C5"), 4, 500, 0.2), lambda V: V.orc.ground_detection_f64(V.arr("C5"), 4, 500, 0.2) + (V.arr("C5"),),
    _ground_check, ("C5",))
DBSCAN = (0.8, 6)
add("dbscan", lambda ctx, H: ctx.dbscan(H.cloud("C5"), *DBSCAN), lambda V: dbscan_ref(V.rows32("C5"), *DBSCAN), assert_dbscan_equal, ("C5",), ("C5",))


def _sor_run(ctx, H):
    keep, avg, st, kept = ctx.statistical_outlier(H.cloud("C5"), 12, 2.0)
    try:
        return keep, avg, np.asarray(st), kept.numpy().T.copy()
    finally:
        kept.free()


add("statistical_outlier", _sor_run, lambda V: (V.rows32("C5"),) + tuple(sor_ref(V.rows32("C5"), 12, 2.0)),
    lambda got, want, what: assert_sor_equal(got, want[0], want[1:], what), ("C5",), ("C5",))


RANGE = (0.8, 10.0, 2)                  # resolution = phi (degrees), theta (degrees), nn_mode


def _range_expect(V):
    pr = project_ref(V.rows32("C5"), RANGE[0])
    lab, inband = label_ref(pr["image"], *RANGE)
    if inband == 0:
        return pr, assign_ref(pr["pix"], lab), int(lab.max()) + 1, None, None
    a, b, cert, inb, _ = edges_ref(pr["image"], *RANGE)                                            # a pair inside the band: between the two partitions
    return (pr, None, None, assign_ref(pr["pix"], components_ref(pr["image"], a[cert], b[cert])),
            assign_ref(pr["pix"], components_ref(pr["image"], a[cert | inb], b[cert | inb])))


def _range_check(got, want, what):                                                                  # test_range_clustering.py: one call against the staged restatement
    (cluster, nc, st), (pr, exact, n_exact, lo, hi) = got, want
    assert (st["rows"], st["cols"], st["dropped"]) == (*pr["image"].shape, pr["dropped"]) and st["full_pixels"] == pr["full_shape"][0] * pr["full_shape"][1], what
    if exact is not None:
        assert np.array_equal(cluster, exact) and nc == n_exact, what
    else:
        assert refines(lo, cluster) and refines(cluster, hi), what


add("range_cluster", lambda ctx, H: ctx.range_cluster(H.cloud("C5"), *RANGE), _range_expect, _range_check, ("C5",))


def _kmeans_centres(V):
    x = V.rows64("C5")
    return x[(np.arange(6) * (x.shape[0] // 6) + 17) % x.shape[0]].copy()                           # test_hw3_clustering.spread_centres


def _kmeans_expect(V):
    x, c = V.rows64("C5"), _kmeans_centres(V)
    labels, _ = rs_assign(x, c)
    exact, counts = rs_exact_centres(x, labels, 6)
    return labels, counts, exact, float(np.abs(x).max())


def _kmeans_check(got, want, what):                                                                 # test_hw3_clustering.py::test_step_parity...
    (labels, counts, new, rc), (wl, wc, exact, amax) = got, want
    assert np.array_equal(labels, wl) and np.array_equal(counts, wc) and rc == (1 if (wc == 0).any() else 0), what
    ok = wc > 0
    assert np.max(np.abs(new[ok] - exact[ok])) <= 2.0 ** -52 * amax and np.isnan(new[~ok]).all(), what


add("kmeans_step", lambda ctx, H: H.mat64("C5").kmeans_step(_kmeans_centres(H)), _kmeans_expect, _kmeans_check, ("C5",))


add("mat64_knn", lambda ctx, H: H.mat64("M2").knn(10), lambda V: rs_knn(V.rows64("M2"), 10), equal_all, ("M2",))                   # test_hw3_spectral.py: indices and d2 bits


# ---- HomeworkFinal ---------------------------------------------------------------------------------------------------------------------
SEG = np.array([0, 1700, 1700, 5000], np.uint32)           # three ragged segments of C5, the middle one empty
NPOINT = 24
STARTS = np.array([5, 0, 77], np.uint32)
BALL = (1.5, 16)


def _fps(mode):
    def run(ctx, H):
        return (ctx.fps(H.cloud("C5"), SEG[[0, 1, 3]], NPOINT, STARTS[[0, 2]], mode),)

    def expect(V):
        return (fps_ref_segments(V.rows32("C5"), SEG[[0, 1, 3]].astype(np.int64), NPOINT, STARTS[[0, 2]], mode).astype(np.uint32),)
    return run, expect, equal_all


add("fps_f32", *_fps(0), ("C5",))
add("fps_f64", *_fps(1), ("C5",))


def _centres(V):
    return np.ascontiguousarray(V.rows32("C5")[::100])      # 50 member points, 17 in the first segment and 33 in the last


CSEG = np.array([0, 17, 17, 50], np.uint32)


def _ball_expect(V):
    pts, cen = V.rows32("C5"), _centres(V)
    want = [ball_ref(pts[SEG[s]:SEG[s + 1]], cen[CSEG[s]:CSEG[s + 1]], *BALL) for s in range(3)]
    return np.concatenate([w[0] for w in want]).reshape(-1, BALL[1]), np.concatenate([w[1] for w in want])


def _ball_run(ctx, H):
    cc = ctx.cloud(_centres(H), AOS3)
    try:
        return ctx.ball_query(H.cloud("C5"), SEG, cc, CSEG, *BALL)
    finally:
        cc.free()


def _int_equal(got, want, what):
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g, np.int64), np.asarray(w, np.int64)), what


add("ball_query", _ball_run, _ball_expect, _int_equal, ("C5",))                                     # test_random_sweeps_stages: rows and counts equal


def _group_run(ctx, H):
    cc = ctx.cloud(_centres(H), AOS3)
    try:
        return ctx.group_points(H.cloud("C5"), SEG, cc, CSEG, _ball_expect(H)[0].astype(np.uint32))
    finally:
        cc.free()


def _group_expect(V):
    pts, cen, rows = V.rows32("C5"), _centres(V), _ball_expect(V)[0]
    parts = [group_ref(pts[SEG[s]:SEG[s + 1]], cen[CSEG[s]:CSEG[s + 1]], rows[CSEG[s]:CSEG[s + 1]], None) for s in (0, 2)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


add("group_points", _group_run, _group_expect, equal_all, ("C5",))
BSEG = np.array([0, 4, 6, 9], np.uint32)
add("points_in_boxes", lambda ctx, H: ctx.points_in_boxes(H.cloud("C5"), SEG, H.inp["BOXES"], BSEG), lambda V: rule_rows(V.rows32("C5"), SEG, V.inp["BOXES"], BSEG),
    lambda got, want, what: assert_box_rows(got, want), ("C5",))


def _labels(V):
    return (np.arange(5000) % 9 - 1).astype(np.int32)


add("label_aabb", lambda ctx, H: ctx.label_aabb(H.cloud("C5"), _labels(H), 10), lambda V: numpy_aabb(V.rows32("C5"), _labels(V), 10), equal_all, ("C5",))


def _pn1_run(ctx, H):
    out = ctx.pointnet_forward(H.model("pn1"), H.inp["PN1OBJ"], return_all=True)
    return tuple(out[k] for k in ("trans", "trans_feat", "global_feat", "logp", "pred"))


def _pn1_expect(V):
    m = pn1.small_model()
    r64, r32 = pn1.batch_np(m, V.inp["PN1OBJ"], np.float64), pn1.batch_np(m, V.inp["PN1OBJ"], np.float32)
    return r64, {k: float(np.abs(r32[k].astype(np.float64) - r64[k]).max()) for k in r64}


def _pn1_check(got, want, what):                                                                    # test_pointnet_cls.py::test_gpu_small_generic_model
    r64, e = want
    for k, g in zip(("trans", "trans_feat", "global_feat", "logp"), got):
        pn1.check(f"{what}: {k}", g, r64[k], e[k])
    assert np.array_equal(got[4], got[3].argmax(1)), what


add("pointnet_forward", _pn1_run, _pn1_expect, _pn1_check, ())


def _pn2_run(ctx, H):
    obj = H.inp["PN2OBJ"]
    starts = np.stack([np.arange(len(obj)) % obj.shape[1], np.arange(len(obj)) % 5]).astype(np.uint32)
    out = ctx.pn2_forward(H.model("pn2"), obj, starts, return_all=True)
    return out["global_feat"], out["logp"], out["pred"], out["fps_idx"][0], out["fps_idx"][1]


add("pn2_forward", _pn2_run, None, None, ())                # expected = the fresh context's answer (module docstring)

KINDS = tuple(STAGES)
CACHE_READERS = tuple(n for n, s in STAGES.items() if s.caches)
