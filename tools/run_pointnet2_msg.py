#!/usr/bin/env python3
"""Measures the PointNet++ multi-scale (MSG) classifier's forward pass (pcr_pn2_forward_f32 on a pcr_pn2_msg_model_create model) at 1, 16 and 64
objects of 256 points, with padded rows (pn2_compact 0) and compacted rows (pn2_compact 1), against a plain-torch restatement of the same math
on the same GPU — written here from the contract in include/pcr.h, after tools/run_pointnet2_classifier.py.  It also reports the SSG model
under pn2_compact 1, for whoever revisits that default.  The record is profiles/pointnet2_msg.txt.

Protocol: wall time of the whole call, host copies included on both sides (the library takes and returns host arrays and ends in a stream
synchronise; the comparator uploads its input and downloads log-probabilities, which synchronises), weights resident on both sides.  The two
settings of pn2_compact ALTERNATE call by call inside one timed loop, so both see the same machine; median of --reps calls each after --warmup
calls, min and max beside it.  The kernel-only figures come from the library's HIP-event profile (tune prof = 2) in a separate pass; the rate
is counted on the padded multiply-adds of pcr_pn2_msg_model_info (what the reference runs) against the 157.3 TF f32 matrix peak, so under
pn2_compact 1 it is the rate of USEFUL work per second, not of the products issued.

    python tools/run_pointnet2_msg.py [--reps 20] [--warmup 3]      (appends to profiles/pointnet2_msg.txt)
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


gen = _load("gen_golden_pointnet2_msg")
PEAK_TF = 157.3
OUT = os.path.join(ROOT, "profiles", "pointnet2_msg.txt")
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


class TorchMsg:
    """the same math in torch, weights folded as the library folds them and resident on the GPU"""

    def __init__(self, torch, state):
        self.t = torch
        self.layers = []
        for conv, bn, w, cin in gen.layers():
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

    def fps(self, xyz, npoint, far):
        torch = self.t
        B, N, _ = xyz.shape
        out = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
        dist = torch.full((B, N), 1e10, dtype=torch.float32, device=xyz.device)
        rows = torch.arange(B, device=xyz.device)
        for i in range(npoint):
            out[:, i] = far
            d = torch.sum((xyz - xyz[rows, far, :].view(B, 1, 3)) ** 2, -1)
            dist = torch.minimum(dist, d)
            far = torch.max(dist, -1)[1]
        return out

    def ball(self, d, N, radius, nsample):
        torch = self.t
        B, S, _ = d.shape
        idx = torch.arange(N, device=d.device).view(1, 1, N).repeat(B, S, 1)
        idx[d > radius ** 2] = N
        idx = idx.sort(dim=-1)[0][:, :, :nsample]
        first = idx[:, :, 0].view(B, S, 1).repeat(1, 1, nsample)
        m = idx == N
        idx[m] = first[m]
        return idx

    def forward(self, objs_host, starts_host):
        torch = self.t
        xyz = torch.from_numpy(objs_host).cuda()
        st = torch.from_numpy(starts_host.astype(np.int64)).cuda()
        B = xyz.shape[0]
        rows = torch.arange(B, device=xyz.device)
        feat, k = None, 0
        for l, (_, npoint, radii, nsamples, mlps) in enumerate(gen.SA):
            cen = xyz[rows[:, None], self.fps(xyz, npoint, st[l])]
            d = torch.sum((cen[:, :, None, :] - xyz[:, None, :, :]) ** 2, -1)      # one distance matrix for the three radii
            outs = []
            for radius, nsample, mlp in zip(radii, nsamples, mlps):
                idx = self.ball(d, xyz.shape[1], radius, nsample)
                g = xyz[rows[:, None, None], idx] - cen[:, :, None, :]
                if feat is not None:
                    g = torch.cat([feat[rows[:, None, None], idx], g], -1)
                outs.append(self.mlp(g, self.layers[k:k + len(mlp)]).max(2)[0])
                k += len(mlp)
            xyz, feat = cen, torch.cat(outs, -1)
        l3 = self.mlp(torch.cat([xyz, feat], -1), self.layers[k:k + 3]).max(1)[0]
        return torch.log_softmax(self.mlp(l3, self.layers[k + 3:], relu_last=False), -1).cpu().numpy()


def measure(ctx, handle, objs, starts, reps, warmup, other=None):
    """median wall ms of pn2_forward under pn2_compact 0 and 1, alternating; other: a comparator timed in the same loop"""
    t = {0: [], 1: [], "other": []}
    for it in range(warmup + reps):
        for c in (0, 1):
            ctx.tune("pn2_compact", c)
            ms = timed(lambda: ctx.pn2_forward(handle, objs, starts))
            if it >= warmup:
                t[c].append(ms)
        if other is not None:
            ms = timed(other)
            if it >= warmup:
                t["other"].append(ms)
    ctx.tune("pn2_compact", -1)
    return {k: stats(v) for k, v in t.items() if v}


def kernels(ctx, handle, objs, starts, reps, macs, names):
    lines = []
    for c in (0, 1):
        ctx.tune("pn2_compact", c)
        ctx.pn2_forward(handle, objs, starts)
        ctx.prof_reset()
        for _ in range(reps):
            ctx.pn2_forward(handle, objs, starts)
        parts, total = [], 0.0
        for name in names:
            n, ms = ctx.prof_get(name)
            if n:
                total += ms / reps
                parts.append(f"{name} {1e3 * ms / reps:.1f} us ({n // reps} launches)")
        mm = (ctx.prof_get("pn2_sa")[1] + ctx.prof_get("pn2_head")[1]) / reps
        tf = 2.0 * macs * len(objs) / (mm * 1e-3) / 1e12 if mm > 0 else 0.0
        lines.append(f"  pn2_compact {c}: " + ", ".join(parts) + f"; sum {1e3 * total:.1f} us; padded multiply-adds over the chain kernels' time {tf:.2f} TF = "
                     f"{100 * tf / PEAK_TF:.1f} % of the {PEAK_TF} TF f32 matrix peak")
    ctx.tune("pn2_compact", -1)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    ref = np.load(os.path.join(ROOT, "tests", "golden", "pointnet2_msg_ref.npz"))
    state = gen.make_state(fc3_bias=ref["fc3_bias"])
    base = gen.base.derive_inputs(gen.base.load_scan())["objs"]
    ctx = pcr.Context(0)
    say(f"device {ctx.device_info()['arch']}, torch {torch.__version__}; wall, median of {a.reps} calls after {a.warmup} warm-up calls, host copies included; "
        f"pn2_compact 0 and 1 and the comparator alternate inside one loop")
    model = pn.get_model_msg(4, normal_channel=False).load_state_dict(state).eval()
    handle = model.model(ctx)
    macs = handle.info(256)["macs_per_object"]
    say(f"MSG model: {handle.info(256)['n_weights']} weights, {macs / 1e9:.3f} G multiply-adds per object of 256 points (padded rows)")
    tm = TorchMsg(torch, state)
    rng = np.random.default_rng(0)
    names = ("fps_small", "fps_large", "pn2_centres", "ball_query", "ball_query_multi", "pn2_scan", "pn2_sa", "pn2_head", "pn2_logsoftmax")
    cases = []
    for n_obj in (1, 16, 64):
        objs = np.ascontiguousarray(base[np.arange(n_obj) % len(base)])
        starts = np.stack([rng.integers(0, 256, n_obj), rng.integers(0, 512, n_obj)])
        cases.append((n_obj, objs, starts))
        ctx.tune("pn2_compact", 0)
        lib0 = ctx.pn2_forward(handle, objs, starts)
        ctx.tune("pn2_compact", 1)
        lib1 = ctx.pn2_forward(handle, objs, starts)
        ctx.tune("pn2_compact", -1)
        cmp_ = tm.forward(objs, starts)
        say(f"n_obj {n_obj}: pn2_compact 0 and 1 give the same bits: {bool(np.array_equal(lib0.view(np.uint32), lib1.view(np.uint32)))}; largest |library - torch| "
            f"log-probability {np.abs(lib1 - cmp_).max():.2e}, predictions equal on {(lib1.argmax(1) == cmp_.argmax(1)).sum()} of {n_obj}")
        t = measure(ctx, handle, objs, starts, a.reps, a.warmup, lambda: tm.forward(objs, starts))
        say(f"n_obj {n_obj:3d}: padded {t[0][0]:9.3f} ms (min {t[0][1]:.3f}, max {t[0][2]:.3f})   compacted {t[1][0]:9.3f} ms (min {t[1][1]:.3f}, max {t[1][2]:.3f})   "
            f"torch batched {t['other'][0]:9.3f} ms (min {t['other'][1]:.3f}, max {t['other'][2]:.3f})   padded / compacted {t[0][0] / t[1][0]:5.2f} x   "
            f"torch / compacted {t['other'][0] / t[1][0]:6.2f} x")
    # the SSG model under both settings (its default is 0)
    ssg_gen = gen.ssg
    ssg_ref = np.load(os.path.join(ROOT, "tests", "golden", "pointnet2_cls_ref.npz"))
    ssg = pn.get_model(4).load_state_dict(ssg_gen.make_state(fc3_bias=ssg_ref["fc3_bias"])).eval().model(ctx)
    ssg_cases = []
    for n_obj in (1, 16, 64):
        objs = np.ascontiguousarray(base[np.arange(n_obj) % len(base)])
        starts = np.stack([rng.integers(0, 256, n_obj), rng.integers(0, 64, n_obj)])
        ssg_cases.append((n_obj, objs, starts))
        t = measure(ctx, ssg, objs, starts, a.reps, a.warmup)
        say(f"SSG n_obj {n_obj:3d}: padded {t[0][0]:9.3f} ms (min {t[0][1]:.3f}, max {t[0][2]:.3f})   compacted {t[1][0]:9.3f} ms (min {t[1][1]:.3f}, max {t[1][2]:.3f})   "
            f"padded / compacted {t[0][0] / t[1][0]:5.2f} x")
    # kernel-only figures, in a pass of their own
    ctx.tune("prof", 2)
    for n_obj, objs, starts in cases:
        say(f"kernels, MSG n_obj {n_obj}:")
        for line in kernels(ctx, handle, objs, starts, a.reps, macs, names):
            say(line)
    for n_obj, objs, starts in ssg_cases[2:]:
        say(f"kernels, SSG n_obj {n_obj}:")
        for line in kernels(ctx, ssg, objs, starts, a.reps, ssg.info(256)["macs_per_object"], names):
            say(line)
    ctx.close()
    with open(OUT, "a") as f:
        f.write("\n== pcr_pn2_forward_f32 on the MSG model, padded and compacted rows, against plain torch on the same GPU (tools/run_pointnet2_msg.py) ==\n")
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
