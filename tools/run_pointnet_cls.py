#!/usr/bin/env python3
"""Measures the vanilla PointNet classifier's forward pass (pcr_pointnet_forward_f32: pointnet_cls with both T-Nets) on 64 objects of 256 and of
1 024 points, next to a plain-torch restatement of the same math on the same GPU — written here from the contract in include/pcr.h, after
tools/run_pointnet2_msg.py.  It first records, per tensor, the library's deviation from the reference's f64 pass in units of the reference's own
f32 deviation (tests/golden/pointnet_cls_ref.npz: the ratios tests/test_pointnet_cls.py bounds by 8).  There is no pass / fail bar on time.  The
record is profiles/pointnet_cls.txt.

Protocol: wall time of the whole call, host copies included on both sides (the library takes and returns host arrays and ends in a stream
synchronise; the comparator uploads its input and downloads log-probabilities, which synchronises), weights resident on both sides.  Library and
comparator ALTERNATE call by call inside one timed loop, so both see the same machine; median of --reps calls each after --warmup calls, min and
max beside it.  The kernel-only figures come from the library's HIP-event profile (tune prof = 2) in a separate pass; the rate is counted on the
multiply-adds the library RUNS (convolution 0 three times, as the stages recompute it) against the 157.3 TF f32 matrix peak.

    python tools/run_pointnet_cls.py [--reps 20] [--warmup 3]      (appends to profiles/pointnet_cls.txt)
"""
import argparse
import importlib
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pcr = importlib.import_module("hands-on-point-cloud-processing_amd")
pn = importlib.import_module("hands-on-point-cloud-processing_amd.pointnet")


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tests", "golden", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load("gen_golden_pointnet_cls")
PEAK_TF = 157.3
OUT = os.path.join(ROOT, "profiles", "pointnet_cls.txt")
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def stats(t):
    return statistics.median(t), min(t), max(t)


def timed(fn):
    a = time.perf_counter()
    fn()
    return (time.perf_counter() - a) * 1e3


class TorchCls:
    """the same math in torch, weights folded as the library folds them and resident on the GPU"""

    def __init__(self, torch, state, channel=3):
        self.t = torch
        self.layers = []
        for conv, bn, w, cin in gen.layers(len(state["fc3.bias"]), channel):
            W = state[f"{conv}.weight"].reshape(w, cin).astype(np.float64)
            b = state[f"{conv}.bias"].astype(np.float64)
            if bn:
                s = state[f"{bn}.weight"].astype(np.float64) / np.sqrt(state[f"{bn}.running_var"].astype(np.float64) + gen.BN_EPS)
                W, b = s[:, None] * W, (b - state[f"{bn}.running_mean"]) * s + state[f"{bn}.bias"]
            self.layers.append((torch.from_numpy(W.astype(np.float32).T.copy()).cuda(), torch.from_numpy(b.astype(np.float32)).cuda()))

    def mlp(self, x, ls, relu_last=True):
        for i, (W, b) in enumerate(ls):
            x = x @ W + b
            if relu_last or i + 1 < len(ls):
                x = self.t.relu(x)
        return x

    def tnet(self, x, ls, k):
        pooled = self.mlp(x, ls[:3]).max(1)[0]
        return self.mlp(pooled, ls[3:], relu_last=False).view(-1, k, k) + self.t.eye(k, device=x.device)

    def forward(self, objs_host):
        torch = self.t
        x = torch.from_numpy(objs_host).cuda()
        L = self.layers
        x = torch.cat([torch.bmm(x[..., :3], self.tnet(x, L[0:6], 3)), x[..., 3:]], -1)
        h = self.mlp(x, L[6:7])
        h = torch.bmm(h, self.tnet(h, L[9:15], h.shape[-1]))
        g = self.mlp(h, L[7:9], relu_last=False).max(1)[0]
        return torch.log_softmax(self.mlp(g, L[15:], relu_last=False), -1).cpu().numpy()


def ratios(ctx, ref, sfx, handle, objs, n_gf, n_tf):
    out = ctx.pointnet_forward(handle, objs, return_all=True)
    parts = []
    for name, key, n in (("logp", "logp", len(objs)), ("global_feat", "gf", n_gf), ("trans", "trans", len(objs)), ("trans_feat", "tf", n_tf)):
        dev = float(np.abs(out[name][:n].astype(np.float64) - ref[f"{key}_f64{sfx}"]).max())
        e = float(ref[f"e_{key}{sfx}"].reshape(-1)[0])
        parts.append(f"{name} {dev:.2e} / {e:.2e} = {dev / e:.2f}")
    say(f"  normal_channel {bool(sfx)}: library deviation from the reference's f64 pass / the reference f32 pass's own: " + "; ".join(parts)
        + f"; predictions equal on {(out['pred'] == ref['logp_f64' + sfx].argmax(1)).sum()} of {len(objs)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    ref = np.load(os.path.join(ROOT, "tests", "golden", "pointnet_cls_ref.npz"))
    state = gen.make_state(fc3_bias=ref["fc3_bias"])
    base = gen.base.derive_inputs(gen.base.load_scan())["objs"]
    ctx = pcr.Context(0)
    say(f"device {ctx.device_info()['arch']}, torch {torch.__version__}; wall, median of {a.reps} calls after {a.warmup} warm-up calls, host copies included; "
        f"library and comparator alternate inside one loop")
    model = pn.get_model_cls(4, normal_channel=False).load_state_dict(state).eval()
    handle = model.model(ctx)
    say("deviation ratios on the fixture (tests/test_pointnet_cls.py bounds each by 8):")
    ratios(ctx, ref, "", handle, base, gen.N_GF, gen.N_TF)
    h6 = pn.get_model_cls(4).load_state_dict(gen.make_state(channel=6, fc3_bias=ref["fc3_bias6"])).eval().model(ctx)
    ratios(ctx, ref, "6", h6, gen.inputs6(base), gen.N_GF6, gen.N_TF6)
    tm = TorchCls(torch, state)
    conv0 = 3 * 64
    cases = []
    for npts in (256, 1024):
        objs = np.ascontiguousarray(np.concatenate([np.roll(base, k, 0) for k in range(npts // 256)], 1))       # 1 024 points: four objects' points
        macs = handle.info(npts)["macs_per_object"]
        run = macs + 2 * conv0 * npts                                       # stages 1 and 2 recompute convolution 0
        cases.append((npts, objs, run))
        lib, cmp_ = ctx.pointnet_forward(handle, objs), tm.forward(objs)
        say(f"64 objects of {npts} points: {macs / 1e9:.3f} G multiply-adds per object ({run / 1e9:.3f} G as run); largest |library - torch| log-probability "
            f"{np.abs(lib - cmp_).max():.2e}, predictions equal on {(lib.argmax(1) == cmp_.argmax(1)).sum()} of {len(objs)}")
        t = {"lib": [], "torch": []}
        for it in range(a.warmup + a.reps):
            for k, fn in (("lib", lambda: ctx.pointnet_forward(handle, objs)), ("torch", lambda: tm.forward(objs))):
                ms = timed(fn)
                if it >= a.warmup:
                    t[k].append(ms)
        tl, tt = stats(t["lib"]), stats(t["torch"])
        say(f"64 x {npts:4d}: library {tl[0]:8.3f} ms (min {tl[1]:.3f}, max {tl[2]:.3f})   torch batched {tt[0]:8.3f} ms (min {tt[1]:.3f}, max {tt[2]:.3f})   "
            f"torch / library {tt[0] / tl[0]:5.2f} x")
    ctx.tune("prof", 2)                                                     # kernel-only figures, in a pass of their own
    for npts, objs, run in cases:
        ctx.pointnet_forward(handle, objs)
        ctx.prof_reset()
        for _ in range(a.reps):
            ctx.pointnet_forward(handle, objs)
        parts = []
        for name in ("pn1_chain", "pn2_head", "pn2_logsoftmax"):
            n, ms = ctx.prof_get(name)
            parts.append(f"{name} {1e3 * ms / a.reps:.1f} us ({n // a.reps} scopes)")
        mm = (ctx.prof_get("pn1_chain")[1] + ctx.prof_get("pn2_head")[1]) / a.reps
        tf = 2.0 * run * len(objs) / (mm * 1e-3) / 1e12 if mm > 0 else 0.0
        say(f"kernels, 64 x {npts}: " + ", ".join(parts) + f"; multiply-adds as run over the chain kernels' time {tf:.2f} TF = {100 * tf / PEAK_TF:.1f} % of the "
            f"{PEAK_TF} TF f32 matrix peak (a pn1_chain scope holds the clear of the key rows, the chain and the decode)")
    ctx.close()
    with open(OUT, "a") as f:
        f.write(f"\n== pcr_pointnet_forward_f32 against the reference fixture and plain torch on the same GPU (python tools/run_pointnet_cls.py --reps {a.reps} "
                f"--warmup {a.warmup}, {time.strftime('%Y-%m-%d')}) ==\n")
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
