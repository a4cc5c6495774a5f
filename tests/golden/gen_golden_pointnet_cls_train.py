"""Writes tests/golden/pointnet_cls_train_ref.npz: what the reference's own vanilla PointNet classifier (models/pointnet_cls.py, models/pointnet.py)
gives in TRAINING mode — total loss, nll, regulariser, logp, trans, trans_feat, every BatchNorm's batch statistics and new running statistics, the
gradient of every parameter — for inputs, weights and the dropout mask DRAWN BY RULE (the functions below: the tests rebuild them, so the fixture
holds reference OUTPUTS only).

Runs on a CPU (torch + numpy):   python tests/golden/gen_golden_pointnet_cls_train.py <reference root>
  <reference root>/HomeworkFinal/models/pointnet_cls.py, pointnet.py     imported as they are

The gradient of this network is discontinuous at every ReLU zero and every max tie, and two correct f32 implementations need not take the same
side of a kink.  The reference's forward hard-wires 1024 (view(-1, 1024) in both T-Nets and in the encoder), so tnet_conv[2] and widths[-1] stay
1024 and every stack carries objects x points x 1024 units in front of a max: with plainly drawn weights no input seed keeps all of them GUARD
errors away from their kinks.  T therefore draws its BatchNorm betas far from zero (make_state's beta rule).
  T   the reference's get_model(4, normal_channel=False), forward untouched, its layers replaced by attribute at small widths (CFG["T"]), 4 objects
      of 8 points.  The generator searches input seeds (cap T_SEED_CAP) until, in the f64 pass, every ReLU input, every positive T-Net max's lead
      and every lead of the encoder's signed max over the best different value is at least GUARD x the f32 pass's largest activation error in
      that layer, and the f32 pass agrees with f64 on every sign and argmax.  Recorded (prefix T_): the seed, the guard ratio, and from the f64
      pass loss, nll, reg, logp, trans, trans_feat, mu / var of every BN, the new running statistics and all gradients (g_*, the analytically
      zero ones included); e_* is the f32 pass's largest absolute deviation from each.  Tensors of more than T_FULL_MAX elements are sampled at
      a fixed stride (sample()).
  F   get_model(4, normal_channel=False) unchanged, the first 8 of the 64 objects of gen_golden_pointnet.derive_inputs (256 points), plain
      betas.  Recorded (prefix F_): the forward quantities with e_*, the gradients sampled (F_FULL_MAX, stored as f32), and e2_*: the f32 pass's
      relative L2 deviation from f64 per tensor; the generator asserts every live e2_* <= F_E2_CAP and moves to the next weight seed otherwise.
Dropout is pinned by a forward hook on `dropout` that applies the mask drawn by rule with s = 1 / (1 - 0.4) rounded to f32.
  toy  the two-class problem of gen_golden_pointnet2_train (noisy spheres against flat discs, 16 objects of 64 points): 40 steps of
      torch.optim.Adam on the reference model and its get_loss, CPU; asserted: the last loss is below 0.25 x the first.  Recorded: toy_loss.
  param_keys   the reference's named_parameters() order (one string, newline-separated).
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pointnet_cls_train_ref.npz")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


base = _load("gen_golden_pointnet")
ssg = _load("gen_golden_pointnet2_train")

GUARD, T_FULL_MAX, F_FULL_MAX, T_SEED_CAP = 16.0, 1024, 256, 4096
DROPOUT_P, BN_EPS, MOMENTUM, REG_SCALE = 0.4, 1e-5, 0.1, 0.001
DROPOUT_S = np.float32(1.0 / (1.0 - DROPOUT_P))
F_OBJECTS, F_WEIGHT_SEED0, F_E2_CAP = 8, 5100, 5e-3
TOY_B, TOY_N, TOY_STEPS, TOY_SEED = ssg.TOY_B, ssg.TOY_N, ssg.TOY_STEPS, ssg.TOY_SEED
CFG = {
    "T": dict(tnet_conv=(4, 8, 1024), tnet_fc=(8, 8), widths=(4, 8, 1024), fc=(16, 8, 4), D0=0, stn3=True, fstn=True, B=4, N=8),
    "F": dict(tnet_conv=(64, 128, 1024), tnet_fc=(512, 256), widths=(64, 128, 1024), fc=(512, 256, 4), D0=0, stn3=True, fstn=True, B=F_OBJECTS, N=256),
}


def layers(cfg):
    """(conv / linear prefix, BN prefix or None, out, in) in WEIGHT order: [feat.stn] [the encoder] [feat.fstn] [the head]"""
    def tnet(prefix, cin, k):
        out = []
        for i, w in enumerate(cfg["tnet_conv"]):
            out.append((f"{prefix}.conv{i + 1}", f"{prefix}.bn{i + 1}", w, cin))
            cin = w
        for i, w in enumerate(cfg["tnet_fc"]):
            out.append((f"{prefix}.fc{i + 1}", f"{prefix}.bn{4 + i}", w, cin))
            cin = w
        return out + [(f"{prefix}.fc3", None, k * k, cin)]

    cin = 3 + cfg["D0"]
    out = tnet("feat.stn", cin, 3) if cfg["stn3"] else []
    for i, w in enumerate(cfg["widths"]):
        out.append((f"feat.conv{i + 1}", f"feat.bn{i + 1}", w, cin))
        cin = w
    if cfg["fstn"]:
        out += tnet("feat.fstn", cfg["widths"][0], cfg["widths"][0])
    for i, w in enumerate(cfg["fc"]):
        out.append((f"fc{i + 1}", f"bn{i + 1}" if i + 1 < len(cfg["fc"]) else None, w, cin))
        cin = w
    return out


def last_enc_bn(cfg):
    return f"feat.bn{len(cfg['widths'])}"


def make_state(cfg, seed, beta_rule=False):
    """the weights by rule, as a state dict of f32 numpy arrays with the reference's key names (Conv1d weights [out, in, 1]).  beta_rule: every
    BN but the encoder's last gets |beta| in [4, 5] with a random sign, 70 % positive; its first two channels get 0.2 N(0, 1)"""
    rng = np.random.default_rng(seed)
    st = {}
    for conv, bn, w, cin in layers(cfg):
        W = (rng.standard_normal((w, cin)) * np.sqrt(2.0 / cin)).astype(np.float32)
        st[f"{conv}.weight"] = W.reshape(w, cin, 1) if ".conv" in conv else W
        st[f"{conv}.bias"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
        if bn:
            st[f"{bn}.weight"] = rng.uniform(0.8, 1.2, w).astype(np.float32)
            beta = 0.1 * rng.standard_normal(w)
            if beta_rule and bn != last_enc_bn(cfg):
                beta = rng.uniform(4.0, 5.0, w) * np.where(rng.uniform(size=w) < 0.7, 1.0, -1.0)
                beta[:2] = 0.2 * rng.standard_normal(min(2, w))
            st[f"{bn}.bias"] = beta.astype(np.float32)
            st[f"{bn}.running_mean"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
            st[f"{bn}.running_var"] = rng.uniform(0.5, 1.5, w).astype(np.float32)
    return st


def param_keys(cfg):
    """the reference's named_parameters() order: module by module, the convolutions and linear layers of a module before its BatchNorms"""
    groups = {}
    for conv, bn, _, _ in layers(cfg):
        g = groups.setdefault(conv.rsplit(".", 1)[0] if "." in conv else "", ([], []))
        g[0].append(conv)
        if bn:
            g[1].append(bn)
    return [f"{m}.{p}" for convs, bns in groups.values() for m in convs + bns for p in ("weight", "bias")]


def dead_keys(cfg):
    """the parameters whose gradient is ALWAYS analytically zero (compared absolutely, never by ratio): the bias of every layer that BN follows
    directly (the head's dropped layer excepted: dropout lies between it and its BN), and the encoder's last beta where the head's first layer is
    followed directly by its BN (three or more FC layers: the max commutes with + beta and that BN removes a constant)"""
    drop = f"fc{len(cfg['fc']) - 1}" if len(cfg["fc"]) >= 2 else None
    dead = {f"{conv}.bias" for conv, bn, _, _ in layers(cfg) if bn and conv != drop}
    if len(cfg["fc"]) >= 3:
        dead.add(f"{last_enc_bn(cfg)}.bias")
    return [k for k in param_keys(cfg) if k in dead]


def tnet_beta_keys(cfg):
    """both T-Nets' third beta: analytically zero in every channel where EVERY object has a positive maximum (the max commutes with + beta, the
    T-Net's first FC BatchNorm removes a constant) or none has (a max of 0 passes nothing), live in a channel where only some have"""
    return [f"{p}.bn3.bias" for p, on in (("feat.stn", cfg["stn3"]), ("feat.fstn", cfg["fstn"])) if on]


def live_keys(cfg):
    """the parameters whose gradient is compared by ratio: all but dead_keys and tnet_beta_keys"""
    dead = set(dead_keys(cfg)) | set(tnet_beta_keys(cfg))
    return [k for k in param_keys(cfg) if k not in dead]


def bn_names(cfg):
    return [bn for _, bn, _, _ in layers(cfg) if bn]


def draw_mask(cfg, seed):
    """the dropout mask by rule: bool [B, width of the last hidden FC layer] (None with a one-layer head)"""
    if len(cfg["fc"]) < 2:
        return None
    return np.random.default_rng(seed).uniform(size=(cfg["B"], cfg["fc"][-2])) >= DROPOUT_P


def t_inputs(seed, cfg=None):
    """T's inputs by rule: points f32 [B, N, 3 + D0], target, the weights (beta rule), the mask"""
    cfg = cfg or CFG["T"]
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.5, 0.5, (cfg["B"], cfg["N"], 3 + cfg["D0"])).astype(np.float32)
    target = rng.integers(0, cfg["fc"][-1], cfg["B"]).astype(np.int64)
    return x, target, make_state(cfg, 100000 + seed, beta_rule=True), draw_mask(cfg, 200000 + seed)


def f_inputs(objs, weight_seed):
    cfg = CFG["F"]
    x = np.ascontiguousarray(objs[:F_OBJECTS], np.float32)
    target = (np.arange(cfg["B"]) % cfg["fc"][-1]).astype(np.int64)
    return x, target, make_state(cfg, weight_seed), draw_mask(cfg, 300000 + weight_seed)


def toy_inputs():
    """the two-class toy problem of gen_golden_pointnet2_train by rule; the weights of the reference's architecture with two classes"""
    x, target, _, _ = ssg.toy_inputs()
    cfg = dict(CFG["F"], fc=(512, 256, 2), B=TOY_B, N=TOY_N)
    return x, target, cfg, make_state(cfg, 4242)


def sample(a, full_max):
    """what the fixture keeps of a tensor: all of it up to full_max elements, else the flattened tensor at the fixed stride ceil(size / full_max)"""
    a = np.asarray(a).reshape(-1)
    return a if a.size <= full_max else a[::-(-a.size // full_max)]


def main(ref_root):
    import torch
    import torch.nn as nn
    torch.set_num_threads(8)
    sys.path.insert(0, os.path.join(ref_root, "HomeworkFinal"))
    from models.pointnet_cls import get_loss, get_model

    def build(cfg):
        m = get_model(cfg["fc"][-1], normal_channel=cfg["D0"] == 3)
        if any(cfg[k] != CFG["F"][k] for k in ("tnet_conv", "tnet_fc", "widths")) or cfg["fc"][:-1] != CFG["F"]["fc"][:-1]:
            mods = {"feat.stn": m.feat.stn, "feat.fstn": m.feat.fstn, "feat": m.feat, "": m}
            for conv, bn, w, cin in layers(cfg):
                pre, name = conv.rsplit(".", 1) if "." in conv else ("", conv)
                setattr(mods[pre], name, nn.Conv1d(cin, w, 1) if name.startswith("conv") else nn.Linear(cin, w))
                if bn:
                    setattr(mods[pre], bn.rsplit(".", 1)[-1], nn.BatchNorm1d(w))
            m.feat.fstn.k = cfg["widths"][0]
        return m

    def run(cfg, x, target, state, mask, double):
        m = build(cfg).train()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
        if double:
            m = m.double()
        zin, pre, hooks, got = {}, {}, [], {}
        mods = dict(m.named_modules())

        def keep_io(bn):
            def hook(mod, i, o):
                zin[bn], pre[bn] = i[0].detach(), o.detach()
            return hook

        for bn in bn_names(cfg):
            hooks.append(mods[bn].register_forward_hook(keep_io(bn)))
        mkt = torch.from_numpy(mask)
        hooks.append(m.dropout.register_forward_hook(lambda mod, i, o: i[0] * mkt.to(i[0].dtype) * float(DROPOUT_S)))
        hooks.append(m.feat.register_forward_hook(lambda mod, i, o: got.update(trans=o[1].detach(), trans_feat=o[2].detach())))
        xx = torch.from_numpy(x).transpose(2, 1).contiguous()
        logp, tf = m(xx.double() if double else xx)
        tt = torch.from_numpy(target)
        loss = get_loss(REG_SCALE)(logp, tt, tf)
        loss.backward()
        nll = torch.nn.functional.nll_loss(logp, tt)
        for h in hooks:
            h.remove()
        out = {"loss": np.float64(loss.item()), "nll": np.float64(nll.item()), "logp": logp.detach().double().numpy(),
               "trans": got["trans"].double().numpy(), "trans_feat": got["trans_feat"].double().numpy(), "pre": pre,
               "grad": {k: p.grad.detach().double().numpy() for k, p in m.named_parameters()}, "param_keys": [k for k, _ in m.named_parameters()]}
        A = got["trans_feat"].double()
        out["reg"] = np.float64(torch.mean(torch.norm(torch.bmm(A, A.transpose(2, 1) - torch.eye(A.shape[1], dtype=A.dtype)[None]), dim=(1, 2))).item())
        for bn in bn_names(cfg):
            z = zin[bn].double()
            dims = (0, 2) if z.dim() == 3 else (0,)
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
            signed = bn == last_enc_bn(cfg)
            if not signed:                                       # a ReLU follows
                ratio = min(ratio, b.abs().min().item() / e)
                agree = agree and bool(((a > 0) == (b > 0)).all())
            if signed or bn in ("feat.stn.bn3", "feat.fstn.bn3"):     # [B, C, N]: a max over dim 2 follows
                r, a_r = (b, a) if signed else (torch.relu(b), torch.relu(a))
                top = r.max(2, keepdim=True)[0]
                low = torch.where(r < top, r, torch.full_like(r, -1e30)).max(2, keepdim=True)[0]
                live = (low > -1e29) if signed else ((top > 0) & (low >= 0))
                gap = torch.where(live, top - low, torch.full_like(top, 1e30)).min().item()
                ratio = min(ratio, gap / e)
                a_top = a_r.max(2, keepdim=True)[0]
                m = torch.ones_like(r, dtype=torch.bool) if signed else (top > 0).expand_as(r)
                agree = agree and bool(((a_r == a_top) == (r == top))[m].all())
        return ratio, agree

    def record(prefix, cfg, r32, r64, out, full_max, with_e2):
        keys = ["loss", "nll", "reg", "logp", "trans", "trans_feat"] + [f"{q}.{bn}" for bn in bn_names(cfg) for q in ("mu", "var", "rmean", "rvar")]
        for k in keys:
            a64, a32 = np.asarray(r64[k], np.float64), np.asarray(r32[k], np.float64)
            out[f"{prefix}_{k}"] = sample(a64, full_max) if k not in ("loss", "nll", "reg", "logp") else a64
            out[f"{prefix}_e_{k}"] = np.float64(np.abs(a32 - a64).max())
        for k in param_keys(cfg):
            g64, g32 = r64["grad"][k], r32["grad"][k]
            out[f"{prefix}_g_{k}"] = sample(g64, full_max).astype(np.float32 if with_e2 else np.float64)
            out[f"{prefix}_e_g_{k}"] = np.float64(np.abs(g32 - g64).max())
            out[f"{prefix}_n_g_{k}"] = np.float64(np.abs(g64).max())
            if with_e2:
                out[f"{prefix}_e2_g_{k}"] = np.float64(np.linalg.norm(g32 - g64) / max(np.linalg.norm(g64), 1e-300))

    out = {}
    # ---- T
    cfg = CFG["T"]
    found = None
    for seed in range(T_SEED_CAP):
        x, target, state, mask = t_inputs(seed)
        r32 = run(cfg, x, target, state, mask, False)
        r64 = run(cfg, x, target, state, mask, True)
        ratio, agree = guard_ratio(cfg, r32, r64)
        if ratio >= GUARD and agree:
            found = seed
            break
    assert found is not None, f"no seed below {T_SEED_CAP} reaches the guard ratio {GUARD}"
    assert r64["param_keys"] == param_keys(cfg)
    out["T_seed"], out["T_guard"] = np.int64(found), np.float64(ratio)
    out["param_keys"] = np.array("\n".join(k for k, _ in build(CFG["F"]).named_parameters()))
    record("T", cfg, r32, r64, out, T_FULL_MAX, False)
    print("T: seed", found, "guard", ratio, "loss", r64["loss"], "nll", r64["nll"], "reg", r64["reg"])
    # ---- F
    cfg = CFG["F"]
    objs = base.derive_inputs(base.load_scan())["objs"]
    for wseed in range(F_WEIGHT_SEED0, F_WEIGHT_SEED0 + 50):
        x, target, state, mask = f_inputs(objs, wseed)
        r32 = run(cfg, x, target, state, mask, False)
        r64 = run(cfg, x, target, state, mask, True)
        e2 = {k: np.linalg.norm(r32["grad"][k] - r64["grad"][k]) / max(np.linalg.norm(r64["grad"][k]), 1e-300) for k in live_keys(cfg)}
        print("F: weight seed", wseed, "worst e2", max(e2.values()), "median", float(np.median(list(e2.values()))))
        if max(e2.values()) <= F_E2_CAP:
            break
    else:
        raise AssertionError(f"no weight seed keeps every e2 below {F_E2_CAP}")
    assert r64["param_keys"] == param_keys(cfg)
    out["F_weight_seed"] = np.int64(wseed)
    record("F", cfg, r32, r64, out, F_FULL_MAX, True)
    # ---- the toy problem: 40 Adam steps on the reference
    x, target, cfg, state = toy_inputs()
    torch.manual_seed(TOY_SEED)
    m = build(cfg).train()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-08, weight_decay=1e-4)
    xx, tt, losses = torch.from_numpy(x).transpose(2, 1).contiguous(), torch.from_numpy(target), []
    for _ in range(TOY_STEPS):
        opt.zero_grad()
        logp, tf = m(xx)
        loss = get_loss(REG_SCALE)(logp, tt, tf)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("toy: first", losses[0], "last", losses[-1])
    assert losses[-1] < 0.25 * losses[0], "the reference does not learn the toy problem"
    out["toy_loss"] = np.asarray(losses, np.float64)
    base._write_npz(OUT, out)
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    assert size <= 768 * 1024


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PCR_REFERENCE_ROOT", ""))
