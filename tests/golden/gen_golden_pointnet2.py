"""Writes tests/golden/pointnet2_cls_ref.npz: what the reference's own PointNet++ (SSG) classifier returns, in eval mode, for the 64 objects of
gen_golden_pointnet.derive_inputs and for weights DRAWN BY RULE (make_state below: the tests rebuild them, so the fixture holds reference
OUTPUTS only, plus the four floats of fc3.bias that the rule centres on the mean output — see below).

Runs on a CPU (torch + numpy):   python tests/golden/gen_golden_pointnet2.py <reference root>
  <reference root>/HomeworkFinal/models/pointnet2_cls_ssg.py, pointnet_util.py     imported as they are

The weight rule: He-scaled W, non-trivial biases and BN statistics (make_state).  With the plain rule every object gets class 0 (the global
feature is non-negative and alike for all objects, so one logit dominates); fc3.bias is therefore set to minus the mean f64 logit over the 64
objects, rounded to f32, and recorded.  The generator asserts that at least two classes are predicted, that every object's top-two margin in
f64 exceeds 1e-3, and that at most 10 % of the objects hold a pair inside the ball query's ambiguity band at either layer.

Recorded: the FPS picks of both layers (column 0 = the start the reference drew under torch.manual_seed(9)), both ball-query tensors, logp and
l3_points of the f32 pass, and from an f64 pass (model.double(), the recorded indices replayed: the reference's FPS cannot run in f64) logp of
all objects, l3 of the first 16, the outputs of sa1 and sa2 of the first 2 — and e_*: the f32 pass's largest deviation from each of them.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pointnet2_cls_ref.npz")
_spec = importlib.util.spec_from_file_location("gen_golden_pointnet", os.path.join(HERE, "gen_golden_pointnet.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

NUM_CLASS, WEIGHT_SEED, TORCH_SEED = 4, 2026, 9      # (weight seeds 2024 and 2027 fail the margin assertion below)
N_L3_F64, N_SA_F64 = 16, 2
SA = (("sa1", 64, 0.2, 8, (64, 64, 128)), ("sa2", 32, 0.4, 16, (128, 128, 256)), ("sa3", None, None, None, (256, 512, 1024)))
BN_KEYS = ("weight", "bias", "running_mean", "running_var")
BN_EPS = 1e-5


def layers(num_class=NUM_CLASS, in_channel=3):
    """(conv / linear prefix, BN prefix or None, out, in) in weight order"""
    out, last = [], in_channel
    for name, _, _, _, mlp in SA:
        cin = last if name == "sa1" else last + 3
        for i, w in enumerate(mlp):
            out.append((f"{name}.mlp_convs.{i}", f"{name}.mlp_bns.{i}", w, cin))
            cin = w
        last = cin
    for fc, bn, w in (("fc1", "bn1", 512), ("fc2", "bn2", 256), ("fc3", None, num_class)):
        out.append((fc, bn, w, last))
        last = w
    return out


def make_state(seed=WEIGHT_SEED, num_class=NUM_CLASS, in_channel=3, fc3_bias=None):
    """the weights by rule, as a state dict of f32 numpy arrays with the reference's key names (Conv2d weights [out, in, 1, 1])"""
    rng = np.random.default_rng(seed)
    st = {}
    for conv, bn, w, cin in layers(num_class, in_channel):
        W = (rng.standard_normal((w, cin)) * np.sqrt(2.0 / cin)).astype(np.float32)
        st[f"{conv}.weight"] = W.reshape(w, cin, 1, 1) if bn and conv.startswith("sa") else W
        st[f"{conv}.bias"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
        if bn:
            st[f"{bn}.weight"] = rng.uniform(0.8, 1.2, w).astype(np.float32)
            st[f"{bn}.bias"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
            st[f"{bn}.running_mean"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
            st[f"{bn}.running_var"] = rng.uniform(0.5, 1.5, w).astype(np.float32)
    if fc3_bias is not None:
        st["fc3.bias"] = np.asarray(fc3_bias, np.float32).reshape(num_class)
    return st


def main(ref_root):
    import torch
    torch.set_num_threads(8)
    sys.path.insert(0, os.path.join(ref_root, "HomeworkFinal"))
    import models.pointnet_util as pu
    from models.pointnet2_cls_ssg import get_model
    objs = base.derive_inputs(base.load_scan())["objs"]
    B = len(objs)
    rec = {"fps": [], "ball": []}
    replay = {"on": False, "fps": 0, "ball": 0}
    fps0, ball0 = pu.farthest_point_sample, pu.query_ball_point

    def fps(xyz, npoint):
        if replay["on"]:
            replay["fps"] += 1
            return rec["fps"][replay["fps"] - 1]
        rec["fps"].append(fps0(xyz, npoint))
        return rec["fps"][-1]

    def ball(radius, nsample, xyz, new_xyz):
        if replay["on"]:
            replay["ball"] += 1
            return rec["ball"][replay["ball"] - 1]
        rec["ball"].append(ball0(radius, nsample, xyz, new_xyz))
        return rec["ball"][-1]

    pu.farthest_point_sample, pu.query_ball_point = fps, ball

    def run(state, double):
        model = get_model(NUM_CLASS).eval()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
        if double:
            model = model.double()
        got = {}
        hooks = [model.sa1.register_forward_hook(lambda m, i, o: got.__setitem__("sa1", o[1])),
                 model.sa2.register_forward_hook(lambda m, i, o: got.__setitem__("sa2", o[1])),
                 model.fc3.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o))]
        x = torch.from_numpy(objs).transpose(2, 1).contiguous()
        replay.update(on=double, fps=0, ball=0)
        if not double:
            rec["fps"].clear(); rec["ball"].clear()
            torch.manual_seed(TORCH_SEED)
        with torch.no_grad():
            logp, l3 = model(x.double() if double else x)
        for h in hooks:
            h.remove()
        # [B, C, S] -> [B, S, C]
        return {"logp": logp.numpy(), "l3": l3.numpy()[:, :, 0], "sa1": got["sa1"].permute(0, 2, 1).numpy(), "sa2": got["sa2"].permute(0, 2, 1).numpy(),
                "logits": got["logits"].numpy()}

    state = make_state(fc3_bias=np.zeros(NUM_CLASS))
    run(state, False)
    fc3_bias = (-run(state, True)["logits"].mean(0)).astype(np.float32)
    state = make_state(fc3_bias=fc3_bias)
    r32 = run(state, False)
    r64 = run(state, True)
    fps_l1, fps_l2 = rec["fps"][0].numpy(), rec["fps"][1].numpy()
    ball_l1, ball_l2 = rec["ball"][0].numpy(), rec["ball"][1].numpy()
    # ---- the fixture conditions
    pred = r64["logp"].argmax(1)
    top = np.sort(r64["logp"], 1)
    margin = float((top[:, -1] - top[:, -2]).min())
    assert len(set(pred.tolist())) >= 2, "the weight rule predicts one class only"
    assert margin > 1e-3, f"top-two margin {margin}"
    assert (r32["logp"].argmax(1) == pred).all()
    exempt = np.zeros(B, bool)
    for b in range(B):
        c1 = objs[b][fps_l1[b]]
        exempt[b] = band_rows(objs[b], c1, SA[0][2]).any() or band_rows(c1, c1[fps_l2[b]], SA[1][2]).any()
    assert exempt.mean() <= 0.10, f"{int(exempt.sum())} of {B} objects hold a pair in the ambiguity band: change the input, not the cap"
    out = {"fc3_bias": fc3_bias, "fps_l1": fps_l1.astype(np.uint16), "fps_l2": fps_l2.astype(np.uint16), "ball_l1": ball_l1.astype(np.uint16),
           "ball_l2": ball_l2.astype(np.uint16), "logp_f32": r32["logp"], "l3_f32": r32["l3"], "logp_f64": r64["logp"], "l3_f64": r64["l3"][:N_L3_F64],
           "sa1_f64": r64["sa1"][:N_SA_F64], "sa2_f64": r64["sa2"][:N_SA_F64]}
    for k, n in (("logp", B), ("l3", N_L3_F64), ("sa1", N_SA_F64), ("sa2", N_SA_F64)):
        out[f"e_{k}"] = np.float64(np.abs(r32[k][:n].astype(np.float64) - r64[k][:n]).max())
    base._write_npz(OUT, out)
    print(OUT, os.path.getsize(OUT), "bytes;", "classes", np.bincount(pred, minlength=NUM_CLASS).tolist(), "margin", margin, "exempt", int(exempt.sum()),
          {k: float(v) for k, v in out.items() if k.startswith("e_")})


def band_rows(pts, centres, radius):
    """rows holding a pair inside the ball query's ambiguity band (the rule of tests/test_pointnet_sampling.py)"""
    q, p, r2 = centres.astype(np.float64), pts.astype(np.float64), float(radius) ** 2
    e = ((q[:, None, :] - p[None]) ** 2).sum(-1)
    tol = 8 * 2.0 ** -24 * ((q ** 2).sum(-1)[:, None] + (p ** 2).sum(-1)[None] + r2)
    return (np.abs(e - r2) <= tol).any(1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PCR_REFERENCE_ROOT", ""))
