#!/usr/bin/env python3
"""Measures one training pass of the vanilla PointNet classifier (pcr_pointnet_train_grad_f32: training-mode forward, loss with the
feature-transform regulariser, every gradient) at the reference's batch, 128 objects of 256 points, against a plain-torch training step of an
equivalent module on the same GPU — written here from the contract in include/pcr.h: Linear + BatchNorm1d (batch statistics) + ReLU over the
rows, max, the two T-Nets with their per-object transforms (bmm), the head with dropout before its second BatchNorm, nll_loss + the regulariser,
backward.  The record is profiles/pointnet_cls_train.txt.

Protocol: the library's kernels by HIP events (tune prof = 2), per profile name, mean of --reps calls after --warmup calls; beside them the
wall time of the whole call (host copies of the objects, logp and the gradient array included).  The comparator runs in a process of its own
(this script with --torch-child: torch's wheel carries its own HIP runtime): wall time of forward + backward around torch.cuda.synchronize,
input upload included, median of --reps.

    python tools/run_pointnet_cls_train.py [--reps 10] [--warmup 2] [--out profiles/pointnet_cls_train.txt]
"""
import argparse
import importlib
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("gen_golden_pointnet_cls_train", os.path.join(ROOT, "tests", "golden", "gen_golden_pointnet_cls_train.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

N_OBJ, NPTS = 128, 256
NAMES = ("pn1t_gemm_fwd", "pn2t_stat", "pn2t_bn_relu", "pn2t_max", "pn1t_identity", "pn1t_transform3", "pn1t_transform", "pn1t_smax", "pn1t_dropout", "pn2t_loss",
         "pn1t_reg", "pn1t_loss_fin", "pn2t_max_back", "pn2t_bn_back", "pn2t_gemm_dw", "pn2t_dw_reduce", "pn1t_gemm_dx", "pn1t_gemm_dt", "pn1t_add")
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def inputs():
    cfg = dict(gen.CFG["F"], B=N_OBJ, N=NPTS)
    base = gen.base.derive_inputs(gen.base.load_scan())["objs"]
    objs = np.ascontiguousarray(base[np.arange(N_OBJ) % len(base)])
    return cfg, gen.make_state(cfg, 1), objs, (np.arange(N_OBJ) % 4).astype(np.int64)


def torch_child(reps, warmup):
    import torch
    nn = torch.nn
    cfg, state, objs, target = inputs()

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin, self.bn = nn.ModuleDict(), nn.ModuleDict()
            for conv, bn, w, cin in gen.layers(cfg):
                lin = nn.Linear(cin, w)
                with torch.no_grad():
                    lin.weight.copy_(torch.from_numpy(state[f"{conv}.weight"].reshape(w, cin)))
                    lin.bias.copy_(torch.from_numpy(state[f"{conv}.bias"]))
                self.lin[conv.replace(".", "_")] = lin
                if bn:
                    b = nn.BatchNorm1d(w)
                    with torch.no_grad():
                        b.weight.copy_(torch.from_numpy(state[f"{bn}.weight"]))
                        b.bias.copy_(torch.from_numpy(state[f"{bn}.bias"]))
                    self.bn[conv.replace(".", "_")] = b
            self.drop = nn.Dropout(gen.DROPOUT_P)

        def layer(self, x, conv, relu=True, drop=False):
            k = conv.replace(".", "_")
            x = self.lin[k](x)
            if drop:
                x = self.drop(x)
            if k in self.bn:
                x = self.bn[k](x)
                if relu:
                    x = torch.relu(x)
            return x

        def tnet(self, pre, x, B, k):
            for i in (1, 2, 3):
                x = self.layer(x, f"{pre}.conv{i}")
            x = x.reshape(B, -1, x.shape[-1]).max(1)[0]
            x = self.layer(self.layer(x, f"{pre}.fc1"), f"{pre}.fc2")
            return self.layer(x, f"{pre}.fc3").reshape(B, k, k) + torch.eye(k, device=x.device)

        def forward(self, pts):
            B, N, _ = pts.shape
            x = torch.bmm(pts, self.tnet("feat.stn", pts.reshape(B * N, -1), B, 3)).reshape(B * N, -1)
            x = self.layer(x, "feat.conv1")
            A = self.tnet("feat.fstn", x, B, x.shape[-1])
            x = torch.bmm(x.reshape(B, N, -1), A).reshape(B * N, -1)
            x = self.layer(self.layer(x, "feat.conv2"), "feat.conv3", relu=False)
            x = x.reshape(B, N, -1).max(1)[0]
            x = self.layer(self.layer(x, "fc1"), "fc2", drop=True)
            return torch.log_softmax(self.layer(x, "fc3"), -1), A

    net = Net().cuda().train()
    tt = torch.from_numpy(target).cuda()
    t = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.zero_grad()
        logp, A = net(torch.from_numpy(objs).cuda())
        M = torch.bmm(A, A.transpose(2, 1) - torch.eye(A.shape[1], device=A.device)[None])
        loss = torch.nn.functional.nll_loss(logp, tt) + gen.REG_SCALE * torch.mean(torch.norm(M, dim=(1, 2)))
        loss.backward()
        torch.cuda.synchronize()
        if i >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"torch": torch.__version__, "median": statistics.median(t), "min": min(t), "max": max(t)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet_cls_train.txt"))
    ap.add_argument("--torch-child", action="store_true")
    a = ap.parse_args()
    if a.torch_child:
        return torch_child(a.reps, a.warmup)
    pcr = importlib.import_module("hands-on-point-cloud-processing_amd")
    pt = importlib.import_module("hands-on-point-cloud-processing_amd.pointnet_train")
    cfg, state, objs, target = inputs()
    ctx = pcr.Context(0)
    say(f"device {ctx.device_info()['arch']}; {N_OBJ} objects of {NPTS} points, {a.reps} calls after {a.warmup} warm-up calls")
    tr = pt.TrainerCls(4, False, ctx=ctx).load_state_dict(state)
    pts = np.ascontiguousarray(np.transpose(objs, (0, 2, 1)))
    info = tr.info(N_OBJ, NPTS)
    say(f"trainer: {info['n_weights']} weights, chunk_rows {info['chunk_rows']}, {info['device_bytes'] / 2 ** 20:.0f} MiB of device memory for this batch")
    wall = []
    for i in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        tr.step_grad(pts, target, seed=i)
        if i >= a.warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    say(f"library, whole call (wall, host copies included): median {statistics.median(wall):.2f} ms (min {min(wall):.2f}, max {max(wall):.2f})")
    ctx.tune("prof", 2)
    tr.step_grad(pts, target, seed=0)
    ctx.prof_reset()
    for i in range(a.reps):
        tr.step_grad(pts, target, seed=i)
    total = 0.0
    for name in NAMES:
        n, ms = ctx.prof_get(name)
        total += ms / a.reps
        if n:
            say(f"  {name:18s} {ms / a.reps:9.3f} ms per call ({n // a.reps} scopes)")
    say(f"library, kernels by HIP events: sum {total:.2f} ms per call")
    ctx.tune("prof", 0)
    tr.free()
    ctx.close()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--reps", str(a.reps), "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        say("plain torch: the comparator's process failed: " + r.stderr.strip().splitlines()[-1] if r.stderr.strip() else "plain torch: the comparator's process failed")
    else:
        t = json.loads(r.stdout.strip().splitlines()[-1])
        say(f"plain torch {t['torch']}, forward + backward of an equivalent module (wall): median {t['median']:.2f} ms (min {t['min']:.2f}, max {t['max']:.2f}); "
            f"library wall / torch wall {statistics.median(wall) / t['median']:.2f} x")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("== pcr_pointnet_train_grad_f32 against a plain-torch training step on the same GPU (tools/run_pointnet_cls_train.py) ==\n")
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
