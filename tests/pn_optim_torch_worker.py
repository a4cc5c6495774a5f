"""Child process of tests/test_pointnet_optim.py::test_live_cross_check_against_torch: three fused device steps of the library's Adam on a small SSG
trainer, and the SAME gradients (read back from the device) fed to a live torch.optim.Adam on host copies, once in f32 and once in f64.  Then a
checkpoint each way.  On a context of its own that it closes before it ends.  Prints one JSON line.

Why a process of its own: torch's wheel carries its own HIP runtime, and importing it puts a second runtime beside the one libpcr_hip.so is
linked against.  The suite's process (which keeps contexts alive until the interpreter ends) stays free of it.
"""
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "hands-on-point-cloud-processing_amd"
HP = dict(betas=(0.9, 0.999), eps=1e-08, weight_decay=1e-4)
LRS = (1e-3, 7e-4, 2.5e-3)


def main():
    import numpy as np
    import torch
    pcr = importlib.import_module(PKG)
    pt = importlib.import_module(PKG + ".pointnet_train")
    sa = [dict(npoint=5, radius=0.45, nsample=3, mlp=[5, 6]), dict(group_all=True, mlp=[5])]      # test_pointnet_optim.py's small SSG trainer
    names = [("sa1.mlp_convs.0", "sa1.mlp_bns.0"), ("sa1.mlp_convs.1", "sa1.mlp_bns.1"), ("sa2.mlp_convs.0", "sa2.mlp_bns.0"), ("fc1", "bn1"), ("fc2", "bn2"), ("fc3", None)]
    out = {}
    ctx = pcr.Context(0)
    try:
        tr = pt.Trainer.from_desc(pcr.pn2_desc(sa, [5, 5, 3], D0=3), names, ctx=ctx, seed=3)
        keys = tr.param_keys()
        start = tr.state_dict()
        host = {dt: [torch.tensor(np.asarray(start[k], np.float64), dtype=dt).requires_grad_(True) for k in keys] for dt in (torch.float32, torch.float64)}
        topt = {dt: torch.optim.Adam(ps, lr=LRS[0], **HP) for dt, ps in host.items()}
        opt = tr.optimizer("Adam", lr=LRS[0], **HP)
        rng = np.random.default_rng(11)
        x, target = rng.uniform(-0.5, 0.5, (3, 6, 24)).astype(np.float32), rng.integers(0, 3, 3)
        out["lib_vs_f64"], out["t32_vs_f64"], out["lib_vs_f64_ulp"] = [], [], []
        for i, lr in enumerate(LRS):
            opt.param_groups[0]["lr"] = lr
            tr.step(x, target, opt, seed=100 + i)
            g, sd = tr.grads(), tr.state_dict()
            for dt, ps in host.items():
                topt[dt].param_groups[0]["lr"] = lr
                for k, p in zip(keys, ps):
                    p.grad = torch.tensor(np.asarray(g[k], np.float64), dtype=dt)
                topt[dt].step()
            lib = t32 = ulp = 0.0
            for k, p32, p64 in zip(keys, host[torch.float32], host[torch.float64]):
                ref = p64.detach().numpy()
                d = np.abs(np.asarray(sd[k], np.float64) - ref)
                lib = max(lib, float(d.max()))
                t32 = max(t32, float(np.abs(p32.detach().numpy().astype(np.float64) - ref).max()))
                ulp = max(ulp, float((d / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)).max()))
            out["lib_vs_f64"].append(lib)
            out["t32_vs_f64"].append(t32)
            out["lib_vs_f64_ulp"].append(ulp)                    # in units of the parameters' f32 ulp
        # ---- a checkpoint from the device loads into torch's optimiser, and torch's into the device's
        t32 = topt[torch.float32]
        dsd, tsd = opt.state_dict(as_torch=True), t32.state_dict()
        out["state_keys_equal"] = (list(dsd["state"]) == list(tsd["state"]) and all(list(dsd["state"][i]) == list(tsd["state"][i]) for i in tsd["state"])
                                   and all(tuple(dsd["state"][i]["exp_avg"].shape) == tuple(tsd["state"][i]["exp_avg"].shape) for i in tsd["state"])
                                   and [k for k in dsd["param_groups"][0]] == [k for k in tsd["param_groups"][0]])
        fresh = torch.optim.Adam([p.detach().clone().requires_grad_(True) for p in host[torch.float32]], lr=9.0)
        fresh.load_state_dict(dsd)
        for p in fresh.param_groups[0]["params"]:
            p.grad = torch.zeros_like(p)
        fresh.step()                                             # torch steps on the loaded state
        st = fresh.state[fresh.param_groups[0]["params"][0]]
        out["device_loads_into_torch"] = bool(float(st["step"]) == 4.0 and fresh.param_groups[0]["lr"] == LRS[-1]
                                              and np.isfinite(st["exp_avg"].numpy()).all())
        tr2 = pt.Trainer.from_desc(pcr.pn2_desc(sa, [5, 5, 3], D0=3), names, ctx=ctx, seed=4).load_state_dict(tr.state_dict())
        opt2 = tr2.optimizer("Adam", lr=9.0).load_state_dict(tsd)
        step, m, v = opt2._state()
        tr2.step(x, target, opt2, seed=7)
        out["torch_loads_into_device"] = bool(step == 3 and opt2.info()["step"] == 4 and opt2.param_groups[0]["lr"] == LRS[-1] and all(
            np.array_equal(tr2._view(k, m), tsd["state"][i]["exp_avg"].numpy()) and np.array_equal(tr2._view(k, v), tsd["state"][i]["exp_avg_sq"].numpy())
            for i, k in enumerate(keys)))
        tr.free()
        tr2.free()
    finally:
        ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
