#!/usr/bin/env python3
"""Measures what the optimiser on the device saves: for each of the three trainers, at the sizes README quotes for its pass (pointnet_cls and SSG 128 x 256,
MSG 32 x 256 and 8 x 256), the wall time of
  (a) the pass alone                 Trainer.step_grad: the gradient array comes down
  (b) the full step on the host      step_grad + torch.optim.Adam.step() on torch_parameters() + sync(): what a training step cost before
  (c) the fused device step          Trainer.step with a DeviceOptimizer: loss and logp alone come down
and the update kernel alone (pnopt_adam by HIP events, tune prof = 2) against a device-to-device copy that moves the same 28 bytes per parameter element.
The record is profiles/pointnet_optim.txt.

Protocol: three trainers of the same weights on one context, the three variants ALTERNATING call by call (so that they share whatever else the host is
doing), a host clock around calls that end in the library's wait; median of --reps rounds after --warmup rounds.  The copy runs in a process of its own
(this script with --copy-child: torch's own HIP runtime, device events around 20 copies, a 1 GiB copy beside it for the bandwidth of the device).

    python tools/run_pointnet_optim.py [--reps 10] [--warmup 2] [--out profiles/pointnet_optim.txt]
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

NPTS = 256
CASES = (("pointnet_cls", "TrainerCls", 128), ("pointnet2_cls_ssg", "Trainer", 128), ("pointnet2_cls_msg", "TrainerMsg", 32), ("pointnet2_cls_msg", "TrainerMsg", 8))
HP = dict(betas=(0.9, 0.999), eps=1e-08, weight_decay=1e-4)
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def copy_child(counts):
    import torch
    out = {}
    for n in counts + [0]:
        floats = (1 << 28) if n == 0 else (7 * n + 1) // 2       # 14 n bytes read and 14 n bytes written: the update's 28 n bytes of traffic
        a, b = torch.empty(floats, dtype=torch.float32, device="cuda"), torch.ones(floats, dtype=torch.float32, device="cuda")
        for _ in range(5):
            a.copy_(b)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(20):
            a.copy_(b)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 20
        out[str(n)] = {"ms": ms, "gbs": 2 * floats * 4 / ms / 1e6}
        del a, b
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointnet_optim.txt"))
    ap.add_argument("--copy-child", default=None)
    a = ap.parse_args()
    if a.copy_child is not None:
        return copy_child([int(v) for v in a.copy_child.split(",")])
    import torch
    pcr = importlib.import_module("hands-on-point-cloud-processing_amd")
    pt = importlib.import_module("hands-on-point-cloud-processing_amd.pointnet_train")
    base = gen.base.derive_inputs(gen.base.load_scan())["objs"]
    ctx = pcr.Context(0)
    say(f"device {ctx.device_info()['arch']}, torch {torch.__version__} (host optimiser); objects of {NPTS} points, {a.reps} rounds after {a.warmup} warm-up rounds, "
        "Adam 1e-3 / (0.9, 0.999) / 1e-8 / weight_decay 1e-4")
    counts, kernel_ms = [], {}
    for model, cls, n_obj in CASES:
        objs = np.ascontiguousarray(base[np.arange(n_obj) % len(base)])
        pts, target = np.ascontiguousarray(np.transpose(objs, (0, 2, 1))), (np.arange(n_obj) % 4).astype(np.int64)
        ta, tb, tc = (getattr(pt, cls)(4, False, ctx=ctx) for _ in range(3))
        topt = torch.optim.Adam(tb.torch_parameters(), lr=1e-3, **HP)
        dopt = tc.optimizer("Adam", lr=1e-3, **HP)
        n = tc._flat.size
        t = {"a": [], "b": [], "c": []}
        for i in range(a.warmup + a.reps):
            for key, fn in (("a", lambda: ta.step_grad(pts, target, seed=i)), ("b", lambda: tb.step(pts, target, topt, seed=i)), ("c", lambda: tc.step(pts, target, dopt, seed=i))):
                t0 = time.perf_counter()
                fn()
                if i >= a.warmup:
                    t[key].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        say(f"-- {model}, {n_obj} objects: {n} weights ({n * 4 / 1e6:.1f} MB an array)")
        for key, what in (("a", "(a) the pass alone (step_grad)"), ("b", "(b) step_grad + torch Adam on the host + sync()"), ("c", "(c) the fused device step")):
            say(f"   {what:50s} median {med[key]:8.2f} ms (min {min(t[key]):.2f}, max {max(t[key]):.2f})")
        say(f"   (b) - (a) = {med['b'] - med['a']:.2f} ms, (c) - (a) = {med['c'] - med['a']:.2f} ms; (b) / (c) = {med['b'] / med['c']:.2f} x")
        ctx.tune("prof", 2)
        tc.step(pts, target, dopt, seed=0)
        ctx.prof_reset()
        for i in range(a.reps):
            tc.step(pts, target, dopt, seed=i)
        calls, ms = ctx.prof_get("pnopt_adam")
        ctx.tune("prof", 0)
        if n not in counts:
            counts.append(n)
            kernel_ms[n] = ms / max(calls, 1)
        say(f"   pnopt_adam by HIP events: {ms / max(calls, 1) * 1e3:.1f} us a launch ({calls} launches), {28 * n / (ms / max(calls, 1)) / 1e6:.0f} GB/s of the 28 B an element")
        for tr in (ta, tb, tc):
            tr.free()
    ctx.close()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--copy-child", ",".join(str(n) for n in counts)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        say("device-to-device copy: the child process failed: " + (r.stderr.strip().splitlines()[-1] if r.stderr.strip() else ""))
    else:
        c = json.loads(r.stdout.strip().splitlines()[-1])
        say(f"device-to-device copy of 1 GiB (torch, device events): {c['0']['gbs']:.0f} GB/s read + written")
        for n in counts:
            say(f"   a copy with the update's traffic for {n} weights ({28 * n / 1e6:.0f} MB): {c[str(n)]['ms'] * 1e3:.1f} us, {c[str(n)]['gbs']:.0f} GB/s; "
                f"pnopt_adam / copy = {kernel_ms[n] / c[str(n)]['ms']:.2f} x")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write("== the optimiser on the device against the host detour (tools/run_pointnet_optim.py) ==\n")
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
