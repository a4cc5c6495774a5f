#!/usr/bin/env python3
"""Measures the PointNet++ (SSG) classifier's forward pass (pcr_pn2_forward_f32) at 1, 64 and 300 objects of 256 points against a plain-torch
restatement of the same math on the same GPU — written here from the contract in include/pcr.h: FPS loop, ball query, gather, folded
matmul + ReLU, max, head, log_softmax — batched, and one object at a time (B = 1, as HomeworkFinal/foreground_obj_cls.py:182-188 feeds it).
The record is profiles/pointnet2_classifier.txt.

Protocol: wall time of the whole call, host copies included on both sides (the library takes and returns host arrays; the comparator uploads
its input and downloads log-probabilities), weights resident on both sides; median of --reps calls after --warmup calls, min and max beside
it.  The kernel-only figures come from the library's HIP-event profile (tune prof = 2) in a separate pass; the rate is counted on the
unpadded multiply-adds of pcr_pn2_model_info against the 157.3 TF f32 matrix peak.

    python tools/run_pointnet2_classifier.py [--reps 20] [--warmup 3]      (appends to profiles/pointnet2_classifier.txt)
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
_spec = importlib.util.spec_from_file_location("gen_golden_pointnet2", os.path.join(ROOT, "tests", "golden", "gen_golden_pointnet2.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

PEAK_TF = 157.3
OUT = os.path.join(ROOT, "profiles", "pointnet2_classifier.txt")
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        a = time.perf_counter()
        fn()
        t.append((time.perf_counter() - a) * 1e3)
    return statistics.median(t), min(t), max(t)


class TorchModel:
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

    def ball(self, radius, nsample, xyz, q):
        torch = self.t
        B, N, _ = xyz.shape
        S = q.shape[1]
        idx = torch.arange(N, device=xyz.device).view(1, 1, N).repeat(B, S, 1)
        d = torch.sum((q[:, :, None, :] - xyz[:, None, :, :]) ** 2, -1)
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
        for l, (_, npoint, radius, nsample, _) in enumerate(gen.SA[:2]):
            f = self.fps(xyz, npoint, st[l])
            cen = xyz[rows[:, None], f]
            idx = self.ball(radius, nsample, xyz, cen)
            g = xyz[rows[:, None, None], idx] - cen[:, :, None, :]
            if feat is not None:
                g = torch.cat([g, feat[rows[:, None, None], idx]], -1)
            feat = self.mlp(g, self.layers[k:k + 3]).max(2)[0]
            xyz, k = cen, k + 3
        l3 = self.mlp(torch.cat([xyz, feat], -1), self.layers[6:9]).max(1)[0]
        return torch.log_softmax(self.mlp(l3, self.layers[9:12], relu_last=False), -1).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    ref = np.load(os.path.join(ROOT, "tests", "golden", "pointnet2_cls_ref.npz"))
    state = gen.make_state(fc3_bias=ref["fc3_bias"])
    base = gen.base.derive_inputs(gen.base.load_scan())["objs"]
    ctx = pcr.Context(0)
    say(f"device {ctx.device_info()['arch']}, torch {torch.__version__}; wall, median of {a.reps} calls after {a.warmup} warm-up calls, host copies included")
    model = pn.get_model(4).load_state_dict(state).eval()
    handle = model.model(ctx)
    macs = handle.info(256)["macs_per_object"]
    say(f"model: {handle.info(256)['n_weights']} weights, {macs / 1e6:.1f} M multiply-adds per object of 256 points")
    tm = TorchModel(torch, state)
    rng = np.random.default_rng(0)
    for n_obj in (1, 64, 300):
        objs = np.ascontiguousarray(base[np.arange(n_obj) % len(base)])
        starts = np.stack([rng.integers(0, 256, n_obj), rng.integers(0, 64, n_obj)])
        lib = ctx.pn2_forward(handle, objs, starts)
        cmp_ = tm.forward(objs, starts)
        say(f"n_obj {n_obj}: largest |library - torch| log-probability {np.abs(lib - cmp_).max():.2e}, predictions equal on {(lib.argmax(1) == cmp_.argmax(1)).sum()} of {n_obj}")
        t_lib = median_ms(lambda: ctx.pn2_forward(handle, objs, starts), a.reps, a.warmup)
        t_bat = median_ms(lambda: tm.forward(objs, starts), a.reps, a.warmup)
        reps1 = max(2, a.reps // (1 + n_obj // 16))
        t_one = median_ms(lambda: [tm.forward(objs[b:b + 1], starts[:, b:b + 1]) for b in range(n_obj)], reps1, 1)
        say(f"n_obj {n_obj:4d}: library {t_lib[0]:9.3f} ms (min {t_lib[1]:.3f}, max {t_lib[2]:.3f})   torch batched {t_bat[0]:9.3f} ms (min {t_bat[1]:.3f}, max {t_bat[2]:.3f})   "
              f"torch B = 1 loop {t_one[0]:10.3f} ms (median of {reps1})   batched / library {t_bat[0] / t_lib[0]:6.2f} x   B = 1 / library {t_one[0] / t_lib[0]:7.1f} x")
    # kernel-only figures
    ctx.tune("prof", 2)
    for n_obj in (1, 64, 300):
        objs = np.ascontiguousarray(base[np.arange(n_obj) % len(base)])
        starts = np.zeros((2, n_obj), np.int64)
        ctx.pn2_forward(handle, objs, starts)
        ctx.prof_reset()
        for _ in range(a.reps):
            ctx.pn2_forward(handle, objs, starts)
        parts, total = [], 0.0
        for name in ("fps_small", "pn2_centres", "ball_query", "pn2_sa", "pn2_head", "pn2_logsoftmax"):
            n, ms = ctx.prof_get(name)
            per_call = ms / a.reps
            total += per_call
            parts.append(f"{name} {1e3 * per_call:.1f} us ({n // a.reps} launches)")
        n, ms = ctx.prof_get("pn2_sa")
        n2, ms2 = ctx.prof_get("pn2_head")
        mm = (ms + ms2) / a.reps
        tf = 2.0 * macs * n_obj / (mm * 1e-3) / 1e12 if mm > 0 else 0.0
        say(f"kernels, n_obj {n_obj:4d}: " + ", ".join(parts) + f"; sum {1e3 * total:.1f} us; the matmul kernels run {tf:.2f} TF = {100 * tf / PEAK_TF:.1f} % of the {PEAK_TF} TF f32 matrix peak")
    ctx.close()
    with open(OUT, "a") as f:      # appended behind the compile-time record
        f.write("\n== pcr_pn2_forward_f32 against a plain-torch restatement on the same GPU (tools/run_pointnet2_classifier.py) ==\n")
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
