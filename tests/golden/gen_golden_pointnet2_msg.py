"""Writes tests/golden/pointnet2_msg_ref.npz: what the reference's own PointNet++ multi-scale (MSG) classifier returns, in eval mode, for objects
of gen_golden_pointnet.derive_inputs and for weights DRAWN BY RULE (make_state below, the rule of gen_golden_pointnet2.make_state extended to
the MSG keys: the tests rebuild them, so the fixture holds reference OUTPUTS only, plus the four floats of fc3.bias).

Runs on a CPU (torch + numpy):   python tests/golden/gen_golden_pointnet2_msg.py <reference root>
  <reference root>/HomeworkFinal/models/pointnet2_cls_msg.py, pointnet_util.py     imported as they are

How: get_model(4, normal_channel=False).eval() on all 64 objects under torch.manual_seed(9) in f32 (one batch, so the FPS starts are the 64
draws of that seed), then as model.double() with the recorded FPS and ball indices replayed (in batches of 8: the f64 activations of 64 objects
do not fit).  fc3.bias is set to minus the mean f64 logit over the 64 objects, as the SSG generator does.  KEPT are the first 16 objects that
hold no pair inside the ball query's ambiguity band (gen_golden_pointnet2.band_rows) at any of the six radii.

Asserted (if one fails: change the input or the weight seed, not the cap): at least 16 such objects; at least two classes predicted among
them; every top-two f64 margin above 1e-3; at most 1 % of all ball rows of the 64 objects in the band; the file at most 512 KB.

Recorded: the 16 object ids and fc3_bias; the FPS picks of both layers for the 16 (npoint 512 over 256 points: once every distance is 0 the
pick is index 0); the six ball tensors of the first two; logp f32 and f64 of the 16; l3 f64 of the first 8; the f64 outputs of sa1 and sa2 for
the first 32 and 16 centres of object 0; e_*: the f32 pass's own deviation from each f64 tensor; the names and shapes of the reference model's
state_dict() entries.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pointnet2_msg_ref.npz")
_spec = importlib.util.spec_from_file_location("gen_golden_pointnet2", os.path.join(HERE, "gen_golden_pointnet2.py"))
ssg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ssg)
base = ssg.base

NUM_CLASS, WEIGHT_SEED, TORCH_SEED = 4, 2026, 9
N_KEEP, N_BALL, N_L3_F64, N_SA1_F64, N_SA2_F64 = 16, 2, 8, 32, 16
MAX_BYTES = 512 * 1024
# name, npoint, radii, nsamples, one list of widths per radius
SA = (("sa1", 512, (0.1, 0.2, 0.4), (16, 32, 128), ((32, 32, 64), (64, 64, 128), (64, 96, 128))),
      ("sa2", 128, (0.2, 0.4, 0.8), (32, 64, 128), ((64, 64, 128), (128, 128, 256), (128, 128, 256))))
SA3 = (256, 512, 1024)
BN_KEYS = ssg.BN_KEYS
BN_EPS = ssg.BN_EPS


def layers(num_class=NUM_CLASS, in_channel=0):
    """(conv / linear prefix, BN prefix or None, out, in) in weight order: layer by layer, branch by branch, convolution by convolution"""
    out, last = [], in_channel
    for name, _, _, _, mlps in SA:
        width = 0
        for i, mlp in enumerate(mlps):
            cin = last + 3
            for j, w in enumerate(mlp):
                out.append((f"{name}.conv_blocks.{i}.{j}", f"{name}.bn_blocks.{i}.{j}", w, cin))
                cin = w
            width += cin
        last = width
    cin = last + 3
    for j, w in enumerate(SA3):
        out.append((f"sa3.mlp_convs.{j}", f"sa3.mlp_bns.{j}", w, cin))
        cin = w
    for fc, bn, w in (("fc1", "bn1", 512), ("fc2", "bn2", 256), ("fc3", None, num_class)):
        out.append((fc, bn, w, cin))
        cin = w
    return out


def make_state(seed=WEIGHT_SEED, num_class=NUM_CLASS, in_channel=0, fc3_bias=None):
    """the weights by the rule of gen_golden_pointnet2.make_state, as a state dict of f32 numpy arrays with the reference's MSG key names"""
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


def band_flags(obj, fps_l1, fps_l2):
    """per radius (six): the rows of one object that hold a pair in the ambiguity band"""
    c1 = obj[fps_l1]
    c2 = c1[fps_l2]
    return [ssg.band_rows(obj, c1, r) for r in SA[0][2]] + [ssg.band_rows(c1, c2, r) for r in SA[1][2]]


def main(ref_root):
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.path.insert(0, os.path.join(ref_root, "HomeworkFinal", "models"))      # the MSG module imports pointnet_util by its bare name
    import pointnet_util as pu
    from pointnet2_cls_msg import get_model
    objs = base.derive_inputs(base.load_scan())["objs"]
    B = len(objs)
    rec = {"fps": [], "ball": []}
    replay = {"on": False, "fps": 0, "ball": 0, "lo": 0, "hi": B}
    fps0, ball0 = pu.farthest_point_sample, pu.query_ball_point

    def fps(xyz, npoint):
        if replay["on"]:
            replay["fps"] += 1
            return rec["fps"][replay["fps"] - 1][replay["lo"]:replay["hi"]]
        rec["fps"].append(fps0(xyz, npoint))
        return rec["fps"][-1]

    def ball(radius, nsample, xyz, new_xyz):
        if replay["on"]:
            replay["ball"] += 1
            return rec["ball"][replay["ball"] - 1][replay["lo"]:replay["hi"]]
        rec["ball"].append(ball0(radius, nsample, xyz, new_xyz))
        return rec["ball"][-1]

    pu.farthest_point_sample, pu.query_ball_point = fps, ball
    names = {}

    def run(state, double, batch):
        model = get_model(NUM_CLASS, normal_channel=False).eval()
        names.update({k: tuple(v.shape) for k, v in model.state_dict().items()})
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
        if double:
            model = model.double()
        got = {}
        hooks = [model.sa1.register_forward_hook(lambda m, i, o: got.__setitem__("sa1", o[1])),
                 model.sa2.register_forward_hook(lambda m, i, o: got.__setitem__("sa2", o[1])),
                 model.fc3.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o))]
        if not double:
            rec["fps"].clear(); rec["ball"].clear()
            torch.manual_seed(TORCH_SEED)
        parts = []
        for lo in range(0, B, batch):
            x = torch.from_numpy(objs[lo:lo + batch]).transpose(2, 1).contiguous()
            replay.update(on=double, fps=0, ball=0, lo=lo, hi=lo + batch)
            with torch.no_grad():
                logp, l3 = model(x.double() if double else x)
            # [B, C, S] -> [B, S, C]; of sa1 and sa2 only the first centres of the first batch's objects are held
            part = {"logp": logp.numpy(), "l3": l3.numpy()[:, :, 0], "logits": got["logits"].numpy()}
            if lo == 0:
                part["sa1"] = got["sa1"].permute(0, 2, 1).numpy()[:8, :N_SA1_F64].copy()
                part["sa2"] = got["sa2"].permute(0, 2, 1).numpy()[:8, :N_SA2_F64].copy()
            parts.append(part)
        for h in hooks:
            h.remove()
        out = {k: np.concatenate([p[k] for p in parts]) for k in ("logp", "l3", "logits")}
        out["sa1"], out["sa2"] = parts[0]["sa1"], parts[0]["sa2"]
        return out

    state = make_state(fc3_bias=np.zeros(NUM_CLASS))
    run(state, False, B)
    fc3_bias = (-run(state, True, 8)["logits"].mean(0)).astype(np.float32)
    state = make_state(fc3_bias=fc3_bias)
    r32 = run(state, False, B)
    r64 = run(state, True, 8)
    assert len(rec["fps"]) == 2 and len(rec["ball"]) == 6
    fps_l1, fps_l2 = rec["fps"][0].numpy(), rec["fps"][1].numpy()
    balls = [t.numpy() for t in rec["ball"]]
    # ---- the fixture conditions
    rows_in_band, rows_all, free = 0, 0, []
    for b in range(B):
        flags = band_flags(objs[b], fps_l1[b], fps_l2[b])
        rows_in_band += int(sum(f.sum() for f in flags))
        rows_all += int(sum(f.size for f in flags))
        if not any(f.any() for f in flags):
            free.append(b)
    assert len(free) >= N_KEEP, f"only {len(free)} objects are free of the ambiguity band"
    assert rows_in_band <= 0.01 * rows_all, f"{rows_in_band} of {rows_all} ball rows lie in the band"
    ids = np.array(free[:N_KEEP])
    p64 = r64["logp"][ids]
    pred = p64.argmax(1)
    top = np.sort(p64, 1)
    margin = float((top[:, -1] - top[:, -2]).min())
    assert len(set(pred.tolist())) >= 2, "the weight rule predicts one class only"
    assert margin > 1e-3, f"top-two margin {margin}"
    assert ids[0] < 8, "the sa1 / sa2 slices are held for the first 8 objects only"
    for r in (r32, r64):                     # object 0 of the kept ones
        r["sa1"], r["sa2"] = r["sa1"][ids[0]], r["sa2"][ids[0]]
    out = {"obj_ids": ids.astype(np.uint16), "fc3_bias": fc3_bias, "fps_l1": fps_l1[ids].astype(np.uint16), "fps_l2": fps_l2[ids].astype(np.uint16),
           "logp_f32": r32["logp"][ids], "logp_f64": p64, "l3_f64": r64["l3"][ids[:N_L3_F64]], "sa1_f64": r64["sa1"], "sa2_f64": r64["sa2"],
           "rows_in_band": np.int64(rows_in_band), "rows_all": np.int64(rows_all), "n_free": np.int64(len(free)),
           "state_names": np.array(sorted(names)), "state_shapes": np.array([",".join(str(v) for v in names[k]) for k in sorted(names)])}
    for k, t in enumerate(balls):
        out[f"ball_{k}"] = t[ids[:N_BALL]].astype(np.uint16)
    out["e_logp"] = np.float64(np.abs(r32["logp"][ids].astype(np.float64) - p64).max())
    out["e_l3"] = np.float64(np.abs(r32["l3"][ids[:N_L3_F64]].astype(np.float64) - out["l3_f64"]).max())
    out["e_sa1"] = np.float64(np.abs(r32["sa1"].astype(np.float64) - r64["sa1"]).max())
    out["e_sa2"] = np.float64(np.abs(r32["sa2"].astype(np.float64) - r64["sa2"]).max())
    base._write_npz(OUT, out)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, f"{size} bytes: shrink the recorded slices"
    print(OUT, size, "bytes;", "kept", ids.tolist(), "classes", np.bincount(pred, minlength=NUM_CLASS).tolist(), "margin", margin, "band-free", len(free),
          "rows in band", rows_in_band, "of", rows_all, {k: float(v) for k, v in out.items() if k.startswith("e_")})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PCR_REFERENCE_ROOT", ""))
