"""Writes tests/golden/pointnet2_msg_train_ref.npz: what the reference's own PointNet++ multi-scale (MSG) classifier gives in TRAINING mode —
loss, logp, every BatchNorm's batch statistics and new running statistics, the gradient of every parameter — for inputs, weights and dropout
masks DRAWN BY RULE (the functions below: the tests rebuild them, so the fixture holds reference OUTPUTS only, plus the recorded sampling).

Runs on a CPU (torch + numpy):   python tests/golden/gen_golden_pointnet2_msg_train.py <reference root>
  <reference root>/HomeworkFinal/models/pointnet2_cls_msg.py, pointnet_util.py     imported as they are

Written like gen_golden_pointnet2_train.py (from which it imports band_rows, toy_inputs and the constants), for the same reason:
the gradient is discontinuous at every ReLU zero and every max tie.
  T   get_model(4, normal_channel=False) with its attributes replaced by the reference's own classes at small sizes (CFG["T"]): two MSG layers
      of three and two branches, the group_all layer, fc 32 / 16 / 4 with p 0.4 / 0.5; 4 objects of 32 points.  The seed search has the SSG
      generator's conditions (guard ratio >= GUARD on every ReLU input and positive max lead, f32 / f64 agreement on signs and argmaxes, no
      pair in the ball query's ambiguity band at ANY radius) and one more: every branch has at least one padded row and one full row.
      Recorded (prefix T_): seed, guard, the picks (fps_l*), one ball tensor per (layer, branch) (ball_l*_b*), and from the f64 pass loss,
      logp, mu / var / new running statistics of every BN and all live gradients, each with e_*: the f32 pass's largest deviation from it.
  F   get_model(4, False) unchanged, the first F_OBJECTS objects of gen_golden_pointnet.derive_inputs without a banded pair at any of the six
      radii.  The weight seed advances until every gradient tensor's f32-vs-f64 relative L2 (e2_*) is <= 5e-3 (asserted).  Recorded (prefix
      F_): the forward quantities with e_*, the gradients at the stride of sample(., F_FULL_MAX), the picks in full, and the ball rows of the
      F_BALL_CENTRES leading centres of every object only (the full tensors are about 720 KB; the MSG eval tests pin the multi-radius query).
  toy the SSG generator's two-class problem (spheres against discs, 16 objects of 64 points) on the reduced MSG model CFG["toy"]: 40 steps
      of torch.optim.Adam on the reference, CPU; asserted: the last loss is below 0.25 x the first.  Recorded: toy_loss.
FPS and ball query are recorded in the f32 pass and replayed in the .double() pass; dropout is pinned by forward hooks on drop1 / drop2, each
with its own s = 1 / (1 - p) rounded to f32.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pointnet2_msg_train_ref.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ssg = _load("gen_golden_pointnet2_train")
base = ssg.base

GUARD, FULL_MAX, F_FULL_MAX = ssg.GUARD, ssg.FULL_MAX, 512
BN_EPS, MOMENTUM = ssg.BN_EPS, ssg.MOMENTUM
F_OBJECTS, F_WEIGHT_SEED0, F_BALL_CENTRES = 4, 5100, 16
TOY_STEPS, TOY_SEED = ssg.TOY_STEPS, ssg.TOY_SEED
# name -> sa: (npoint, radii, nsamples, one list of widths per radius) per MSG layer; sa3: the group_all layer's widths; fc; p: one dropout
# probability per FC layer but the last; objects; points
CFG = {
    "T": dict(sa=((8, (0.25, 0.35, 0.5), (3, 4, 6), ((8, 8), (8, 12), (8, 8, 16))), (4, (0.5, 0.8), (4, 6), ((16, 16), (16, 24)))), sa3=(32, 64),
              fc=(32, 16, 4), p=(0.4, 0.5), B=4, N=32),
    "F": dict(sa=((512, (0.1, 0.2, 0.4), (16, 32, 128), ((32, 32, 64), (64, 64, 128), (64, 96, 128))),
                  (128, (0.2, 0.4, 0.8), (32, 64, 128), ((64, 64, 128), (128, 128, 256), (128, 128, 256)))), sa3=(256, 512, 1024),
              fc=(512, 256, 4), p=(0.4, 0.5), B=F_OBJECTS, N=256),
    "toy": dict(sa=((32, (0.2, 0.4), (8, 16), ((16, 16, 32), (16, 16, 32))), (8, (0.4, 0.8), (8, 16), ((32, 32, 64), (32, 32, 64)))), sa3=(64, 128, 256),
                fc=(64, 32, 2), p=(0.4, 0.5), B=ssg.TOY_B, N=ssg.TOY_N),
}


def layers(cfg):
    """(conv / linear prefix, BN prefix or None, out, in) in weight order: layer by layer, branch by branch"""
    out, last = [], 0
    for l, (_, _, _, mlps) in enumerate(cfg["sa"]):
        width = 0
        for i, mlp in enumerate(mlps):
            cin = last + 3
            for j, w in enumerate(mlp):
                out.append((f"sa{l + 1}.conv_blocks.{i}.{j}", f"sa{l + 1}.bn_blocks.{i}.{j}", w, cin))
                cin = w
            width += cin
        last = width
    n, cin = len(cfg["sa"]) + 1, last + 3
    for j, w in enumerate(cfg["sa3"]):
        out.append((f"sa{n}.mlp_convs.{j}", f"sa{n}.mlp_bns.{j}", w, cin))
        cin = w
    for i, w in enumerate(cfg["fc"]):
        out.append((f"fc{i + 1}", f"bn{i + 1}" if i + 1 < len(cfg["fc"]) else None, w, cin))
        cin = w
    return out


def make_state(cfg, seed):
    """the weights by rule, as a state dict of f32 numpy arrays with the reference's key names (Conv2d weights [out, in, 1, 1])"""
    rng = np.random.default_rng(seed)
    st = {}
    for conv, bn, w, cin in layers(cfg):
        W = (rng.standard_normal((w, cin)) * np.sqrt(2.0 / cin)).astype(np.float32)
        st[f"{conv}.weight"] = W.reshape(w, cin, 1, 1) if conv.startswith("sa") else W
        st[f"{conv}.bias"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
        if bn:
            st[f"{bn}.weight"] = rng.uniform(0.8, 1.2, w).astype(np.float32)
            st[f"{bn}.bias"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
            st[f"{bn}.running_mean"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
            st[f"{bn}.running_var"] = rng.uniform(0.5, 1.5, w).astype(np.float32)
    return st


def param_keys(cfg):
    out = []
    for conv, bn, _, _ in layers(cfg):
        out += [f"{conv}.weight", f"{conv}.bias"] + ([f"{bn}.weight", f"{bn}.bias"] if bn else [])
    return out


def live_keys(cfg):
    """the parameters whose gradient is not analytically zero: all but the bias of a layer that BN follows (recorded and compared)"""
    dead = {f"{conv}.bias" for conv, bn, _, _ in layers(cfg) if bn}
    return [k for k in param_keys(cfg) if k not in dead]


def bn_names(cfg):
    return [bn for _, bn, _, _ in layers(cfg) if bn]


def dropout_s(cfg):
    """s_i = 1 / (1 - p_i) rounded to f32, per FC layer but the last"""
    return [np.float32(1.0 / (1.0 - p)) for p in cfg["p"]]


def draw_masks(cfg, seed):
    """the dropout masks by rule: one bool [B, width] per FC layer but the last, layer i with its own p"""
    rng = np.random.default_rng(seed)
    return [rng.uniform(size=(cfg["B"], w)) >= p for w, p in zip(cfg["fc"][:-1], cfg["p"])]


def t_inputs(seed):
    """T's inputs by rule: points f32 [B, N, 3], target, the weights, the masks"""
    cfg = CFG["T"]
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, (cfg["B"], cfg["N"], 3)).astype(np.float32)
    target = rng.integers(0, cfg["fc"][-1], cfg["B"]).astype(np.int64)
    return x, target, make_state(cfg, 100000 + seed), draw_masks(cfg, 200000 + seed)


def f_inputs(objs, chosen, weight_seed):
    """F's inputs by rule: chosen = the fixture's F_objects"""
    cfg = CFG["F"]
    x = np.ascontiguousarray(objs[np.asarray(chosen)], np.float32)
    target = (np.arange(cfg["B"]) % cfg["fc"][-1]).astype(np.int64)
    return x, target, make_state(cfg, weight_seed), draw_masks(cfg, 300000 + weight_seed)


def toy_inputs():
    """the SSG generator's toy problem on the reduced MSG model: f32 [16, 64, 3], target, the configuration, the weights"""
    x, target, _, _ = ssg.toy_inputs()
    return x, target, CFG["toy"], make_state(CFG["toy"], 4242)


def sample(a, full_max=FULL_MAX):
    """what the fixture keeps of a tensor: all of it up to full_max elements, else the flattened tensor at the fixed stride ceil(size / full_max)"""
    a = np.asarray(a).reshape(-1)
    return a if a.size <= full_max else a[::-(-a.size // full_max)]


def row_kinds(ball):
    """(has a padded row, has a full row) of one branch's ball tensor [B, S, K]: a padded row repeats its first entry behind position 0"""
    pad = (ball[..., 1:] == ball[..., :1]).any(-1) if ball.shape[-1] > 1 else np.zeros(ball.shape[:-1], bool)
    return bool(pad.any()), bool((~pad).any())


def main(ref_root):
    import torch
    import torch.nn as nn
    torch.set_num_threads(8)
    sys.path.insert(0, os.path.join(ref_root, "HomeworkFinal", "models"))      # the MSG module imports pointnet_util by its bare name
    import pointnet_util as pu
    from pointnet2_cls_msg import get_loss, get_model
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

    def build(cfg):
        m = get_model(cfg["fc"][-1], normal_channel=False)
        if cfg["sa"] != CFG["F"]["sa"] or cfg["fc"][:-1] != CFG["F"]["fc"][:-1]:
            last = 0
            for l, (npoint, radii, nsamples, mlps) in enumerate(cfg["sa"]):
                setattr(m, f"sa{l + 1}", pu.PointNetSetAbstractionMsg(npoint, list(radii), list(nsamples), last, [list(mlp) for mlp in mlps]))
                last = sum(mlp[-1] for mlp in mlps)
            m.sa3 = pu.PointNetSetAbstraction(None, None, None, last + 3, list(cfg["sa3"]), True)
            last = cfg["sa3"][-1]
            for i, w in enumerate(cfg["fc"]):
                setattr(m, f"fc{i + 1}", nn.Linear(last, w))
                if i + 1 < len(cfg["fc"]):
                    setattr(m, f"bn{i + 1}", nn.BatchNorm1d(w))
                last = w
            width = cfg["sa3"][-1]
            if width != 1024:                                    # the reference's forward views l3_points as [B, 1024]: the same statements at the model's width
                import torch.nn.functional as F

                def forward(xyz):
                    B = xyz.shape[0]
                    l1_xyz, l1_points = m.sa1(xyz, None)
                    l2_xyz, l2_points = m.sa2(l1_xyz, l1_points)
                    l3_xyz, l3_points = m.sa3(l2_xyz, l2_points)
                    x = l3_points.view(B, width)
                    x = m.drop1(F.relu(m.bn1(m.fc1(x))))
                    x = m.drop2(F.relu(m.bn2(m.fc2(x))))
                    return F.log_softmax(m.fc3(x), -1), l3_points
                m.forward = forward
        return m

    def run(cfg, x, target, state, masks, double, torch_seed=0):
        m = build(cfg).train()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
        if double:
            m = m.double()
        zin, pre, hooks = {}, {}, []
        mods = dict(m.named_modules())

        def keep_io(bn):
            def hook(mod, i, o):
                zin[bn], pre[bn] = i[0].detach(), o.detach()
            return hook

        for bn in bn_names(cfg):
            hooks.append(mods[bn].register_forward_hook(keep_io(bn)))
        for d, mk, s in zip((m.drop1, m.drop2), masks, dropout_s(cfg)):
            mkt = torch.from_numpy(mk)
            hooks.append(d.register_forward_hook(lambda mod, i, o, mkt=mkt, s=s: i[0] * mkt.to(i[0].dtype) * float(s)))
        replay.update(on=double, fps=0, ball=0)
        if not double:
            rec["fps"].clear(); rec["ball"].clear()
            torch.manual_seed(torch_seed)
        xx = torch.from_numpy(x).transpose(2, 1).contiguous()
        logp, _ = m(xx.double() if double else xx)
        loss = get_loss()(logp, torch.from_numpy(target), None)
        loss.backward()
        for h in hooks:
            h.remove()
        out = {"loss": np.float64(loss.item()), "logp": logp.detach().double().numpy(), "pre": pre,
               "grad": {k: p.grad.detach().double().numpy() for k, p in m.named_parameters()}}
        for bn in bn_names(cfg):
            z = zin[bn].double()
            dims = (0, 2, 3) if z.dim() == 4 else (0,)
            out[f"mu.{bn}"] = z.mean(dims).numpy()
            out[f"var.{bn}"] = z.var(dims, unbiased=False).numpy()
            out[f"rmean.{bn}"] = mods[bn].running_mean.detach().double().numpy()
            out[f"rvar.{bn}"] = mods[bn].running_var.detach().double().numpy()
        return out

    def guard_ratio(cfg, r32, r64):
        """(the smallest margin / error ratio over the layers, do the signs and argmaxes agree)"""
        ratio, agree = np.inf, True
        for bn in bn_names(cfg):
            a, b = r32["pre"][bn].double(), r64["pre"][bn]
            e = max((a - b).abs().max().item(), 1e-300)
            ratio = min(ratio, b.abs().min().item() / e)
            agree = agree and bool(((a > 0) == (b > 0)).all())
            if b.dim() == 4:                                     # [B, C, nsample, npoint]: the max runs over dim 2
                r = torch.relu(b)
                top, arg = r.max(2, keepdim=True)
                low = torch.where(r < top, r, torch.full_like(r, -1.0)).max(2, keepdim=True)[0]
                gap = torch.where((top > 0) & (low >= 0), top - low, torch.full_like(top, 1e30)).min().item()
                ratio = min(ratio, gap / e)
                a_r = torch.relu(a)
                a_top = a_r.max(2, keepdim=True)[0]
                agree = agree and bool(((a_r == a_top) == (r == top))[(top > 0).expand_as(r)].all())
        return ratio, agree

    def banded(cfg, x):
        """per object: does it hold a pair in the ambiguity band at any radius of any sampling layer (on the recorded picks)"""
        out = np.zeros(len(x), bool)
        for b in range(len(x)):
            pts = x[b]
            for l, (_, radii, _, _) in enumerate(cfg["sa"]):
                c = pts[rec["fps"][l][b].numpy()]
                for radius in radii:
                    out[b] = out[b] or ssg.band_rows(pts, c, radius).any()
                pts = c
        return out

    def balls(cfg):
        """the recorded ball tensors as (layer, branch, array)"""
        out, k = [], 0
        for l, (_, radii, _, _) in enumerate(cfg["sa"]):
            for b in range(len(radii)):
                out.append((l, b, rec["ball"][k].numpy()))
                k += 1
        return out

    def record(prefix, cfg, r32, r64, out, with_e2, full_max, ball_centres):
        keys = ["loss", "logp"] + [f"{q}.{bn}" for bn in bn_names(cfg) for q in ("mu", "var", "rmean", "rvar")]
        for k in keys:
            out[f"{prefix}_{k}"] = np.asarray(r64[k], np.float64)
            out[f"{prefix}_e_{k}"] = np.float64(np.abs(np.asarray(r32[k], np.float64) - r64[k]).max())
        for k in live_keys(cfg):
            g64, g32 = r64["grad"][k], r32["grad"][k]
            out[f"{prefix}_g_{k}"] = sample(g64, full_max).astype(np.float64)
            out[f"{prefix}_e_g_{k}"] = np.float64(np.abs(g32 - g64).max())
            if with_e2:
                out[f"{prefix}_e2_g_{k}"] = np.float64(np.linalg.norm(g32 - g64) / max(np.linalg.norm(g64), 1e-300))
        for l in range(len(rec["fps"])):
            out[f"{prefix}_fps_l{l + 1}"] = rec["fps"][l].numpy().astype(np.uint16)
        for l, b, a in balls(cfg):
            out[f"{prefix}_ball_l{l + 1}_b{b}"] = (a if ball_centres is None else a[:, :ball_centres]).astype(np.uint16)

    out = {}
    # ---- T
    cfg = CFG["T"]
    found = None
    for seed in range(20000):
        x, target, state, masks = t_inputs(seed)
        r32 = run(cfg, x, target, state, masks, False, torch_seed=seed)
        kinds = [row_kinds(a) for _, _, a in balls(cfg)]
        if not all(p and f for p, f in kinds) or banded(cfg, x).any():
            continue
        r64 = run(cfg, x, target, state, masks, True)
        ratio, agree = guard_ratio(cfg, r32, r64)
        if ratio >= GUARD and agree:
            found = seed
            break
    assert found is not None, "no seed reaches the guard ratio"
    assert all(p and f for p, f in kinds), "a branch without a padded row or without a full row"
    out["T_seed"], out["T_guard"] = np.int64(found), np.float64(ratio)
    record("T", cfg, r32, r64, out, False, FULL_MAX, None)
    print("T: seed", found, "guard", ratio, "loss", r64["loss"], flush=True)
    # ---- the toy problem: 40 Adam steps on the reference
    x, target, cfg, state = toy_inputs()
    torch.manual_seed(TOY_SEED)
    replay.update(on=False)
    m = build(cfg).train()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-08, weight_decay=1e-4)
    xx, tt, losses = torch.from_numpy(x).transpose(2, 1).contiguous(), torch.from_numpy(target), []
    for _ in range(TOY_STEPS):
        opt.zero_grad()
        logp, _ = m(xx)
        loss = get_loss()(logp, tt, None)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("toy: first", losses[0], "last", losses[-1], flush=True)
    assert losses[-1] < 0.25 * losses[0], "the reference does not learn the toy problem"
    out["toy_loss"] = np.asarray(losses, np.float64)
    # ---- F
    cfg = CFG["F"]
    objs = base.derive_inputs(base.load_scan())["objs"]
    pool, chosen = list(range(len(objs))), []
    while True:                                                  # the first F_OBJECTS objects that hold no banded pair in the run they are part of
        chosen = pool[:F_OBJECTS]
        assert len(chosen) == F_OBJECTS, "too few objects without a banded pair"
        x, target, state, masks = f_inputs(objs, chosen, F_WEIGHT_SEED0)
        with torch.no_grad():
            replay.update(on=False)
            rec["fps"].clear(); rec["ball"].clear()
            mm = build(cfg).train()
            mm.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
            torch.manual_seed(9)                                 # as run() seeds: behind the construction
            mm(torch.from_numpy(x).transpose(2, 1).contiguous())
        bad = banded(cfg, x)
        if not bad.any():
            break
        pool = [o for o in pool if o not in {chosen[i] for i in np.flatnonzero(bad)}]
    chosen = np.asarray(chosen)
    for wseed in range(F_WEIGHT_SEED0, F_WEIGHT_SEED0 + 50):
        x, target, state, masks = f_inputs(objs, chosen, wseed)
        r32 = run(cfg, x, target, state, masks, False, torch_seed=9)
        r64 = run(cfg, x, target, state, masks, True)
        e2 = {k: np.linalg.norm(r32["grad"][k] - r64["grad"][k]) / max(np.linalg.norm(r64["grad"][k]), 1e-300) for k in live_keys(cfg)}
        print("F: weight seed", wseed, "worst e2", max(e2.values()), "banded", int(banded(cfg, x).sum()), flush=True)
        if max(e2.values()) <= 5e-3 and not banded(cfg, x).any():
            break
    else:
        raise AssertionError("no weight seed keeps every e2 below 5e-3")
    out["F_objects"], out["F_weight_seed"] = chosen.astype(np.int64), np.int64(wseed)
    record("F", cfg, r32, r64, out, True, F_FULL_MAX, F_BALL_CENTRES)
    pu.farthest_point_sample, pu.query_ball_point = fps0, ball0
    base._write_npz(OUT, out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size <= 512 * 1024


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PCR_REFERENCE_ROOT", ""))
