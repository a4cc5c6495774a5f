"""csrc/pointnet_layers.hpp: the one place where a classifier's descriptor becomes its layers in weight order, or is rejected.  The eval
models (pointnet2.hip) and both training passes take their layers, their limits and their weight count from it.

The header is host-only, so tests/cpp/pointnet_layers_check.cpp is compiled with plain g++ (warnings are errors).  It builds a list of
descriptors by rule — both kinds at their smallest legal shape, every count at its largest, and every limit at its last accepted and first
rejected value (width 1024 / 1025, D0 1021 / 1022, widths[0] 128 / 129 with fstn, n_branch 4 / 5, summed branch width 1024 / 1025, nsample
65536 / 65537, group_all on a layer that is not the last, a negative, an infinite and a NaN radius, ...) — and prints each with the header's
verdict, weight count, markers and layers.

  CPU   the verdict of every case is the one pinned in EXPECT; the count and the part boundaries equal a restatement written here from the
        contract in include/pcr.h; pcr_pn2_msg_model_info(NULL, ...) / pcr_pn1_model_info(NULL, ...) of the built library give the same
        verdict, n_weights, n_class, c_last and n_sampling.
  GPU   for every accepted case whose widths are <= 32 the model and the trainer made from the SAME descriptor both succeed, report the
        header's n_weights and the same n_class, and one flat weight array drawn by rule loads into both (a multi-branch descriptor has no
        trainer: the model alone).  For every rejected case both return PCR_ERR_ARG with "a descriptor outside the limits".  No forward pass.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hands-on-point-cloud-processing_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "pointnet_layers_check.cpp")

# name -> accepted.  The driver's list and this one must hold the same names
EXPECT = {
    "ssg_min": True, "ssg_two": True, "ssg_two_D0_3": True, "ssg_full": True,
    "ssg_mlp_width_1024": True, "ssg_mlp_width_1025": False, "ssg_fc_width_1024": True, "ssg_fc_width_1025": False, "ssg_mlp_width_0": False,
    "ssg_D0_1021": True, "ssg_D0_1022": False,
    "ssg_nsample_65536": True, "ssg_nsample_65537": False, "ssg_nsample_0": False, "ssg_npoint_0": False,
    "ssg_group_all_not_last": False, "ssg_group_all_2": False,
    "ssg_radius_negative": False, "ssg_radius_inf": False, "ssg_radius_nan": False, "ssg_radius_0": True, "ssg_bn_eps_inf": False,
    "ssg_n_sa_0": False, "ssg_n_sa_5": False, "ssg_n_fc_0": False, "ssg_n_fc_5": False, "ssg_n_mlp_0": False, "ssg_n_mlp_5": False,
    "msg_two_branches": True, "msg_n_branch_4": True, "msg_n_branch_5": False, "msg_n_branch_0": False,
    "msg_branch_sum_1024": True, "msg_branch_sum_1025": False, "msg_branch_sum_1021_not_last": True, "msg_branch_sum_1022_not_last": False,
    "msg_xyz_last_2": False, "msg_second_branch_nsample_65537": False,
    "msg_group_all_two_branches": False,
    "pn1_min_plain": True, "pn1_min_stn3": True, "pn1_min_fstn": True, "pn1_min_both": True, "pn1_full": True,
    "pn1_width_1024": True, "pn1_width_1025": False, "pn1_fc_width_1024": True, "pn1_fc_width_1025": False,
    "pn1_tnet_conv_1024": True, "pn1_tnet_conv_1025": False, "pn1_tnet_fc_1024": True, "pn1_tnet_fc_1025": False,
    "pn1_plain_ignores_tnet_widths": True,
    "pn1_D0_1021": True, "pn1_D0_1022": False, "pn1_fstn_k_128": True, "pn1_fstn_k_129": False, "pn1_stn3_only_k_129": True,
    "pn1_stn3_2": False, "pn1_fstn_2": False, "pn1_bn_eps_inf": False,
    "pn1_n_mlp_1": False, "pn1_n_mlp_5": False, "pn1_n_fc_0": False, "pn1_n_fc_5": False,
}
# the accepted cases whose widths in use are all <= 32: the GPU test makes a model and a trainer of each
SMALL = ["ssg_min", "ssg_two", "ssg_two_D0_3", "ssg_full", "ssg_D0_1021", "ssg_nsample_65536", "ssg_radius_0", "msg_two_branches", "msg_n_branch_4",
         "pn1_min_plain", "pn1_min_stn3", "pn1_min_fstn", "pn1_min_both", "pn1_full", "pn1_plain_ignores_tnet_widths", "pn1_D0_1021"]
REJECTED = [n for n, ok in EXPECT.items() if not ok]

_cases = None


def cases():
    """name -> what the driver printed for it; compiled and run once per session"""
    global _cases
    if _cases is None:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            exe = os.path.join(tmp, "pointnet_layers_check")
            r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, "-o", exe], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
        rows = [json.loads(line) for line in r.stdout.splitlines()]
        _cases = {c["name"]: c for c in rows}
        assert len(_cases) == len(rows), "a case name twice"
    return _cases


def widths_in_use(c):
    d = c["desc"]
    if c["kind"] == "pn1":
        w = d["widths"][:d["n_mlp"]] + d["fc_widths"][:d["n_fc"]]
        return w + (d["tnet_conv"] + d["tnet_fc"] if d["stn3"] or d["fstn"] else [])
    w = d["fc_widths"][:d["n_fc"]]
    for s in d["sa"][:d["n_sa"]]:
        for b in s["branch"][:s["n_branch"]]:
            w = w + b["widths"][:b["n_mlp"]]
    return w


def count_of(shapes):
    """W [N][K], bias [N] and, with BN, gamma, beta, running_mean, running_var (include/pcr.h above pcr_pn2_model_create)"""
    return sum(K * N + N + (4 * N if bn else 0) for K, N, bn in shapes)


def restate_pn2(d):
    """layer by layer, branch by branch, convolution by convolution, then the FC layers; the last FC layer has no BN"""
    shapes, first, sa_in, sa_out, D, n_sampling = [], [], [], [], d["D0"], 0
    for s in d["sa"][:d["n_sa"]]:
        sa_in.append(3 + D)
        first.append([])
        width = 0
        for b in s["branch"][:s["n_branch"]]:
            first[-1].append(len(shapes))
            K = 3 + D
            for w in b["widths"][:b["n_mlp"]]:
                shapes.append([K, w, 1])
                K = w
            width += K
        sa_out.append(width)
        D = width
        n_sampling += 0 if s["group_all"] else 1
    head_first, K = len(shapes), D
    for i, w in enumerate(d["fc_widths"][:d["n_fc"]]):
        shapes.append([K, w, 1 if i + 1 < d["n_fc"] else 0])
        K = w
    return {"shapes": shapes, "first": first, "sa_in": sa_in, "sa_out": sa_out, "head_first": head_first, "n_sampling": n_sampling, "n_weights": count_of(shapes)}


def restate_pn1(d):
    """[stn3: conv1 conv2 conv3 fc1 fc2 fc3] [the encoder] [fstn: the same six layers] [the head]; a T-Net's fc3 has k k outputs and no BN"""
    shapes, C0 = [], 3 + d["D0"]

    def tnet(cin, k):
        K = cin
        for w in d["tnet_conv"] + d["tnet_fc"]:
            shapes.append([K, w, 1])
            K = w
        shapes.append([K, k * k, 0])

    if d["stn3"]:
        tnet(C0, 3)
    enc_first, K = len(shapes), C0
    for w in d["widths"][:d["n_mlp"]]:
        shapes.append([K, w, 1])
        K = w
    fstn_first = len(shapes)
    if d["fstn"]:
        tnet(d["widths"][0], d["widths"][0])
    head_first = len(shapes)
    for i, w in enumerate(d["fc_widths"][:d["n_fc"]]):
        shapes.append([K, w, 1 if i + 1 < d["n_fc"] else 0])
        K = w
    return {"shapes": shapes, "stn_first": 0, "enc_first": enc_first, "fstn_first": fstn_first, "head_first": head_first, "n_weights": count_of(shapes)}


def test_driver_verdicts_counts_and_markers():
    cs = cases()
    assert set(cs) == set(EXPECT)
    for name, c in cs.items():
        assert bool(c["ok"]) == EXPECT[name], name
        if not c["ok"]:
            continue
        want = restate_pn1(c["desc"]) if c["kind"] == "pn1" else restate_pn2(c["desc"])
        for key, v in want.items():
            assert c[key] == v, (name, key, c[key], v)
        if c["kind"] == "pn1":       # the five parts: a T-Net is 3 conv + 3 FC, a part the flags leave out is empty
            d = c["desc"]
            assert c["enc_first"] - c["stn_first"] == (6 if d["stn3"] else 0) and c["fstn_first"] - c["enc_first"] == d["n_mlp"]
            assert c["head_first"] - c["fstn_first"] == (6 if d["fstn"] else 0) and len(c["shapes"]) - c["head_first"] == d["n_fc"]
    assert sorted(SMALL) == sorted(n for n, c in cs.items() if c["ok"] and max(widths_in_use(c)) <= 32)
    # the limits the issue names, each on both sides
    for a, r in (("ssg_mlp_width_1024", "ssg_mlp_width_1025"), ("ssg_D0_1021", "ssg_D0_1022"), ("pn1_fstn_k_128", "pn1_fstn_k_129"), ("msg_n_branch_4", "msg_n_branch_5"),
                 ("msg_branch_sum_1024", "msg_branch_sum_1025"), ("ssg_nsample_65536", "ssg_nsample_65537"), ("pn1_width_1024", "pn1_width_1025"), ("pn1_D0_1021", "pn1_D0_1022")):
        assert cs[a]["ok"] and not cs[r]["ok"]
    assert cs["pn1_fstn_k_128"]["shapes"][cs["pn1_fstn_k_128"]["fstn_first"] + 5][1] == 128 * 128      # exempt from the width limit


def msg_desc_of(pcr, d):
    m = pcr.Pn2MsgDesc()
    m.D0, m.n_sa, m.n_fc, m.bn_eps = d["D0"], d["n_sa"], d["n_fc"], float.fromhex(d["bn_eps"])
    for k in range(4):
        m.fc_widths[k] = d["fc_widths"][k]
    for l, s in enumerate(d["sa"]):
        e = m.sa[l]
        e.npoint, e.group_all, e.xyz_last, e.n_branch = s["npoint"], s["group_all"], s["xyz_last"], s["n_branch"]
        for b, br in enumerate(s["branch"]):
            e.branch[b].radius, e.branch[b].nsample, e.branch[b].n_mlp = float.fromhex(br["radius"]), br["nsample"], br["n_mlp"]
            for k in range(4):
                e.branch[b].widths[k] = br["widths"][k]
    return m


def ssg_desc_of(pcr, d):
    """the single-scale descriptor of a case the driver made from one (branch 0 of every layer)"""
    s = pcr.Pn2Desc()
    s.D0, s.n_sa, s.n_fc, s.bn_eps = d["D0"], d["n_sa"], d["n_fc"], float.fromhex(d["bn_eps"])
    for k in range(4):
        s.fc_widths[k] = d["fc_widths"][k]
    for l, m in enumerate(d["sa"]):
        e, br = s.sa[l], m["branch"][0]
        e.npoint, e.group_all, e.radius, e.nsample, e.n_mlp = m["npoint"], m["group_all"], float.fromhex(br["radius"]), br["nsample"], br["n_mlp"]
        for k in range(4):
            e.widths[k] = br["widths"][k]
    return s


def pn1_desc_of(pcr, d):
    p = pcr.Pn1Desc()
    p.D0, p.stn3, p.fstn, p.n_mlp, p.n_fc, p.bn_eps = d["D0"], d["stn3"], d["fstn"], d["n_mlp"], d["n_fc"], float.fromhex(d["bn_eps"])
    for k in range(4):
        p.widths[k], p.fc_widths[k] = d["widths"][k], d["fc_widths"][k]
    for k in range(3):
        p.tnet_conv[k] = d["tnet_conv"][k]
    for k in range(2):
        p.tnet_fc[k] = d["tnet_fc"][k]
    return p


def test_library_info_without_a_model_agrees(pcr):
    L = pcr.lib()
    for name, c in cases().items():
        info = pcr.Pn2Info()
        if c["kind"] == "pn1":
            rc = L.pcr_pn1_model_info(None, 0, C.byref(info), C.byref(pn1_desc_of(pcr, c["desc"])))
            c_last = c["desc"]["widths"][c["desc"]["n_mlp"] - 1] if c["ok"] else 0
        else:
            rc = L.pcr_pn2_msg_model_info(None, 0, C.byref(info), C.byref(msg_desc_of(pcr, c["desc"])))
            c_last = c["sa_out"][-1] if c["ok"] else 0
        assert (rc == 0) == bool(c["ok"]) and rc in (0, -1), (name, rc)
        if c["ok"]:
            got = (int(info.n_weights), int(info.n_class), int(info.c_last), int(info.n_sampling))
            assert got == (c["n_weights"], c["shapes"][-1][1], c_last, c.get("n_sampling", 0)), (name, got)


def weights_by_rule(n):
    """every value in (0.25, 0.75): finite, and a running variance that is positive"""
    i = np.arange(n, dtype=np.uint64)
    return (0.25 + 0.5 * ((i * np.uint64(2654435761)) % np.uint64(1000003)).astype(np.float64) / 1000003.0).astype(np.float32)


@pytest.fixture(scope="module")
def ctx(pcr):
    c = pcr.Context(0)
    yield c
    c.close()


def creators(pcr, c):
    """(what, descriptor, create(ctx, desc, w, n, out), is a trainer) for a case: the model and, where the descriptor has one, the trainer"""
    L = pcr.lib()
    if c["kind"] == "pn1":
        d = pn1_desc_of(pcr, c["desc"])
        return [("pcr_pn1_model_create", d, lambda h, w, n, out: L.pcr_pn1_model_create(h, C.byref(d), w, n, out), False),
                ("pcr_pn1_trainer_create", d, lambda h, w, n, out: L.pcr_pn1_trainer_create(h, C.byref(d), w, n, 0.4, 0.1, 0.001, 0, out), True)]
    if c["ssg"]:
        d = ssg_desc_of(pcr, c["desc"])
        return [("pcr_pn2_model_create", d, lambda h, w, n, out: L.pcr_pn2_model_create(h, C.byref(d), w, n, out), False),
                ("pcr_pn2_trainer_create", d, lambda h, w, n, out: L.pcr_pn2_trainer_create(h, C.byref(d), w, n, 0.4, 0.1, 0, out), True)]
    d = msg_desc_of(pcr, c["desc"])
    return [("pcr_pn2_msg_model_create", d, lambda h, w, n, out: L.pcr_pn2_msg_model_create(h, C.byref(d), w, n, out), False)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL)
def test_model_and_trainer_of_one_descriptor_agree(pcr, ctx, name):
    c, L = cases()[name], pcr.lib()
    assert c["ok"] and max(widths_in_use(c)) <= 32
    w = weights_by_rule(c["n_weights"])
    seen = []
    for what, _, create, is_trainer in creators(pcr, c):
        h = C.c_void_p()
        rc = create(ctx.h, w.ctypes.data, w.size, C.byref(h))
        assert rc == 0 and h.value, (what, rc, L.pcr_ctx_last_error(ctx.h))
        try:
            if is_trainer:
                ti = pcr.Pn2TrainInfo()
                assert L.pcr_pn2_trainer_info(h, 0, 0, C.byref(ti)) == 0
                seen.append((int(ti.n_weights), int(ti.n_class)))
                back = np.zeros_like(w)
                assert L.pcr_pn2_trainer_get_weights(ctx.h, h, back.ctypes.data, back.size) == 0
                assert np.array_equal(back.view(np.uint32), w.view(np.uint32)), what
            else:
                mi = pcr.Pn2Info()
                info = L.pcr_pn1_model_info if c["kind"] == "pn1" else L.pcr_pn2_msg_model_info
                assert info(h, 0, C.byref(mi), None) == 0
                seen.append((int(mi.n_weights), int(mi.n_class)))
            # one float more or less is not the model's count
            for n in (w.size - 1, w.size + 1):
                h2 = C.c_void_p()
                w2 = weights_by_rule(n)
                assert create(ctx.h, w2.ctypes.data, n, C.byref(h2)) == -1 and not h2.value
                assert b"n_weights is not the model's count" in L.pcr_ctx_last_error(ctx.h)
        finally:
            (L.pcr_pn2_trainer_destroy if is_trainer else L.pcr_pn2_model_destroy)(ctx.h, h)
    assert all(s == (c["n_weights"], c["shapes"][-1][1]) for s in seen), seen
    assert len(seen) == (1 if c["kind"] == "pn2" and not c["ssg"] else 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", REJECTED)
def test_model_and_trainer_reject_the_same_descriptors(pcr, ctx, name):
    c, L = cases()[name], pcr.lib()
    assert not c["ok"]
    w = weights_by_rule(16)
    for what, _, create, _ in creators(pcr, c):
        h = C.c_void_p()
        rc = create(ctx.h, w.ctypes.data, w.size, C.byref(h))
        msg = L.pcr_ctx_last_error(ctx.h).decode()
        assert rc == -1 and not h.value, (what, rc)
        assert msg.startswith(what + ": a descriptor outside the limits"), (what, msg)
