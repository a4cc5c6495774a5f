"""Golden trajectories for the device optimiser of the PointNet trainers (tests/test_pointnet_optim.py): torch.optim.Adam and torch.optim.SGD themselves,
on a CPU, in f32 and in f64, on parameters and gradient sequences drawn by rule.  torch is the reference here: the file holds no program text of the
reference project, only train_cls.py's hyper-parameters (:147-155: Adam 1e-3 / (0.9, 0.999) / 1e-8 / weight_decay 1e-4; SGD 0.01 / momentum 0.9; StepLR 20 / 0.7).

    python tests/golden/gen_golden_pointnet_optim.py        # writes tests/golden/pointnet_optim_ref.npz

What is stored, per configuration c in CONFIGS (A: Adam as train_cls.py builds it; B: the same with weight_decay 0; S: SGD 0.01 / 0.9 / weight_decay 1e-4):
  c_p64_<t>      torch's f64 parameters after step t in STORED (flat, the tensors of SHAPES one behind the other)
  c_e32_<t>      max over elements of |torch f32 - torch f64| after step t: torch's own f32 error, the yardstick of the accuracy bar
  c_p32          torch's f32 parameters after the last step
  c_s64_<name>, c_e32_<name>     the same two for the final state (exp_avg, exp_avg_sq / momentum_buffer)
  lr             the learning rate of every step (StepLR stepped once per optimiser step, so it changes twice in the run)
  adam_group_keys / sgd_group_keys / adam_state_keys / sgd_state_keys      torch's state_dict layout: the names, in torch's order
The inputs are NOT stored: inputs() draws them again by rule.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pointnet_optim_ref.npz")

SHAPES = ((7, 5, 1, 1), (7,), (7,), (7,), (64, 61), (64,), (3, 25))      # 4 099 elements: no tensor but one starts on a multiple of 4
N = sum(int(np.prod(s)) for s in SHAPES)
STEPS, STORED = 45, (1, 21, 45)
STEP_SIZE, GAMMA = 20, 0.7
SEED = 20240
CONFIGS = {
    "A": dict(kind="Adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-08, weight_decay=1e-4),
    "B": dict(kind="Adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-08, weight_decay=0.0),
    "S": dict(kind="SGD", lr=0.01, momentum=0.9, dampening=0.0, weight_decay=1e-4),
}
ZERO_ALWAYS = slice(100, 116)            # gradient exactly 0 at every step
TINY = slice(200, 232)                   # |g| in 1e-23 ... 1e-20 and w = 0: g^2 is subnormal or underflows in f32, (1 - beta2) g^2 too


def inputs():
    """(w0 f32 [N], grads f32 [STEPS, N]): |g| = 10^u, u uniform in [-6, 0], random sign; a twentieth of the elements exactly 0 at any step, ZERO_ALWAYS
    at every step; the TINY elements start at w = 0 with |g| = 10^u, u uniform in [-23, -20]"""
    rng = np.random.default_rng(SEED)
    w0 = (0.5 * rng.standard_normal(N)).astype(np.float32)
    g = (10.0 ** rng.uniform(-6.0, 0.0, (STEPS, N)) * rng.choice([-1.0, 1.0], (STEPS, N))).astype(np.float32)
    g[rng.uniform(size=(STEPS, N)) < 0.05] = 0.0
    g[:, ZERO_ALWAYS] = 0.0
    n_tiny = TINY.stop - TINY.start
    g[:, TINY] = (10.0 ** rng.uniform(-23.0, -20.0, (STEPS, n_tiny)) * rng.choice([-1.0, 1.0], (STEPS, n_tiny))).astype(np.float32)
    w0[TINY] = 0.0
    return w0, g


def split(flat):
    out, off = [], 0
    for s in SHAPES:
        n = int(np.prod(s))
        out.append(flat[off:off + n].reshape(s))
        off += n
    return out


def lr_sequence(lr0):
    """StepLR's recurrence stepped once per optimiser step: the lr that step t (0-based) uses"""
    out, lr = [], lr0
    for t in range(STEPS):
        out.append(lr)
        if (t + 1) % STEP_SIZE == 0:
            lr = lr * GAMMA
    return out


def run_torch(cfg, dtype):
    import torch
    w0, g = inputs()
    params = [torch.tensor(a.astype(dtype)).requires_grad_(True) for a in split(w0)]
    kw = {k: v for k, v in cfg.items() if k != "kind"}
    opt = getattr(torch.optim, cfg["kind"])(params, **kw)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=STEP_SIZE, gamma=GAMMA)
    stored, lrs = {}, []
    for t in range(STEPS):
        for p, a in zip(params, split(g[t])):
            p.grad = torch.tensor(a.astype(dtype))
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
        if t + 1 in STORED:
            stored[t + 1] = np.concatenate([p.detach().numpy().reshape(-1) for p in params])
    names = ("exp_avg", "exp_avg_sq") if cfg["kind"] == "Adam" else ("momentum_buffer",)
    state = {n: np.concatenate([opt.state[p][n].numpy().reshape(-1) for p in params]) for n in names}
    sd = opt.state_dict()
    layout = ([k for k in sd["param_groups"][0] if k != "params"], list(sd["state"][0]))
    return stored, state, lrs, layout


def main():
    import torch
    torch.set_flush_denormal(False)
    out = {}
    for c, cfg in CONFIGS.items():
        p32, s32, lr32, layout = run_torch(cfg, np.float32)
        p64, s64, lr64, _ = run_torch(cfg, np.float64)
        assert lr32 == lr64 == lr_sequence(cfg["lr"])
        for t in STORED:
            out[f"{c}_p64_{t}"] = p64[t]
            out[f"{c}_e32_{t}"] = np.float64(np.abs(p32[t].astype(np.float64) - p64[t]).max())
        out[f"{c}_p32"] = p32[STORED[-1]]
        for n in s64:
            out[f"{c}_s64_{n}"] = s64[n]
            out[f"{c}_e32_{n}"] = np.float64(np.abs(s32[n].astype(np.float64) - s64[n]).max())
        out[f"{c}_lr"] = np.asarray(lr32, np.float64)
        kind = cfg["kind"].lower()
        out[f"{kind}_group_keys"], out[f"{kind}_state_keys"] = np.asarray(layout[0]), np.asarray(layout[1])
        print(c, {t: float(out[f"{c}_e32_{t}"]) for t in STORED}, {n: float(out[f"{c}_e32_{n}"]) for n in s64})
        if c == "B":
            v = s32["exp_avg_sq"][TINY]
            assert ((v > 0) & (v < np.finfo(np.float32).tiny)).any(), "no subnormal exp_avg_sq in the run"
    out["torch_version"] = np.asarray(torch.__version__)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
