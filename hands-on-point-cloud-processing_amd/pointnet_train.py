"""HomeworkFinal's training step for the PointNet++ (SSG, MSG) and PointNet classifiers on the GPU: training-mode forward pass, get_loss and the gradient of
every parameter (HomeworkFinal/train_cls.py:186-196 without its optimiser; models/pointnet2_cls_ssg.py).

  Trainer       the model in training mode on the library (pcr_pn2_train_grad_f32; the contract is above pcr_pn2_trainer_create in include/pcr.h)
  get_loss      models/pointnet2_cls_ssg.get_loss: the same call, (pred, target, trans_feat) -> the mean negative log-likelihood
  TrainerCls    the vanilla PointNet (models/pointnet_cls.get_model) in training mode (pcr_pointnet_train_grad_f32; the contract is above
                pcr_pn1_trainer_create in include/pcr.h): the same surface as Trainer, nothing is sampled
  get_loss_cls  models/pointnet_cls.get_loss: the NLL plus mat_diff_loss_scale x the feature-transform regulariser
  TrainerMsg    the multi-scale model (models/pointnet2_cls_msg.get_model) in training mode: the same call on a trainer of
                pcr_pn2_msg_trainer_create, with the head's two dropout probabilities (0.4, 0.5); get_loss serves it unchanged
  TRAINERS      the reference's module name (train_cls.py --model) -> the trainer class, for the two first built
  ALL_TRAINERS  the same for every model train_cls.py --model can name

  DeviceOptimizer   Trainer.optimizer("Adam" | "SGD", ...): torch.optim.Adam / SGD as train_cls.py:147-155 builds them, on the DEVICE (the contract is
                above pcr_pn2_trainer_optim_set in include/pcr.h), with torch's surface where train_cls.py uses it
  StepLR        torch.optim.lr_scheduler.StepLR's recurrence on a DeviceOptimizer (or on anything with param_groups)

The whole of train_cls.py:186-199 on the device: per step only the batch goes up, and loss and logp come down.

    tr = Trainer(num_class)
    opt = tr.optimizer("Adam", lr=1e-3, betas=(0.9, 0.999), eps=1e-08, weight_decay=1e-4)
    sched = StepLR(opt, step_size=20, gamma=0.7)
    for epoch in range(epochs):
        for points, target in loader:
            loss, logp = tr.step(points, target, opt)      # the pass and the update in one call, at opt.param_groups[0]["lr"]
        sched.step()
    torch.save({"model_state_dict": tr.state_dict(), "optimizer_state_dict": opt.state_dict()}, path)

Or the optimiser stays torch's own, on host tensors, exactly as train_cls.py:147-153 builds it:

    tr = Trainer(num_class)
    opt = torch.optim.Adam(tr.torch_parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-08, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=20, gamma=0.7)
    for points, target in loader:                  # points [B, 3 | 6, N]
        opt.zero_grad()                            # (optional: step_grad overwrites every .grad)
        loss, logp = tr.step_grad(points, target)
        opt.step()
        tr.sync()                                  # the stepped weights go to the device; the running statistics stay the device's
    classifier = tr.eval_model()                   # a pointnet.get_model in eval mode with the trained weights and running statistics

What is unpinned: the first FPS picks (start= fixes them) and the dropout masks (keep= fixes them); without them both are drawn from `seed`,
or from np.random where no seed is given, as the reference draws them from torch's stream.  pointnet.get_model is unchanged: its train() raises.
"""
from __future__ import annotations

import numpy as np

from .pointnet import _BN_KEYS, _SSG_FC, _SSG_SA, _ctx, _like, _to_host, get_model, get_model_cls, get_model_msg

_PARAM_BN = ("weight", "bias")


def _conv2d(conv):
    """whether a layer's weight is a Conv2d's [out, in, 1, 1] in the reference's state dict (an SA layer's convolution)"""
    return "mlp_convs" in conv or "conv_blocks" in conv


class _DescModel(get_model):
    """pointnet.get_model for the layers and the descriptor of a Trainer.from_desc"""

    def __init__(self, num_class, desc, layers):
        super().__init__(num_class, int(desc.D0) == 3)
        self._d, self._l = desc, layers
        nps = [int(desc.sa[l].npoint) for l in range(desc.n_sa) if not desc.sa[l].group_all]
        self._npoint1 = nps[0] if nps else 1

    def _layers(self):
        return list(self._l)

    def desc(self):
        return self._d

    def state_shapes(self):
        out = {}
        for conv, bn, w, cin in self._l:
            out[f"{conv}.weight"] = (w, cin, 1, 1) if _conv2d(conv) else (w, cin)
            out[f"{conv}.bias"] = (w,)
            for k in (_BN_KEYS if bn else ()):
                out[f"{bn}.{k}"] = (w,)
        return out


class _DescModelMsg(_DescModel, get_model_msg):
    """pointnet.get_model_msg for the layers and the descriptor of a TrainerMsg.from_desc (uploaded through pn2_msg_model)"""


def _desc_layers(desc, names):
    """(conv / linear prefix, BN prefix or None, out, in) in weight order for a Pn2Desc or a Pn2MsgDesc (layer by layer, branch by branch) and one
    (conv, bn) pair of names per layer"""
    shapes, D = [], int(desc.D0)
    for l in range(desc.n_sa):
        sa, width = desc.sa[l], 0
        for br in ([sa.branch[b] for b in range(sa.n_branch)] if hasattr(sa, "branch") else [sa]):      # a Pn2MsgDesc's branches, or the Pn2Desc's one
            cin = 3 + D
            for i in range(br.n_mlp):
                shapes.append((int(br.widths[i]), cin, True))
                cin = int(br.widths[i])
            width += cin
        D = width
    cin = D
    for i in range(desc.n_fc):
        shapes.append((int(desc.fc_widths[i]), cin, i + 1 < desc.n_fc))
        cin = int(desc.fc_widths[i])
    names = list(names)
    if len(names) != len(shapes):
        raise ValueError(f"names: one (conv, bn) pair per layer, the descriptor has {len(shapes)}")
    out = []
    for (conv, bn), (w, cin, has_bn) in zip(names, shapes):
        if has_bn != (bn is not None):
            raise ValueError(f"names: layer {conv} {'has' if has_bn else 'has no'} BatchNorm")
        out.append((conv, bn, w, cin))
    return out


class Trainer:
    """The reference's pointnet2_cls_ssg.get_model in TRAINING mode on the library.  Trainer(num_class, normal_channel, dropout, momentum,
    chunk_rows, ctx) is the reference's architecture; Trainer.from_desc(desc, names) any Pn2Desc (names: one (conv prefix, BN prefix or None) per
    layer in weight order).  Fresh weights follow torch's default initialisation rule (uniform in +-1 / sqrt(fan_in); gamma 1, beta 0), drawn
    from np.random.default_rng(seed); load_state_dict / state_dict use the reference's keys, the running statistics come from the device and
    num_batches_tracked is counted.  chunk_rows is part of the arithmetic contract (include/pcr.h): 0 = the library's default."""

    def __init__(self, num_class, normal_channel=False, dropout=0.4, momentum=0.1, chunk_rows=0, ctx=None, *, seed=0):
        from . import pn2_desc
        self.num_class, self.normal_channel = int(num_class), bool(normal_channel)
        proto = get_model(self.num_class, self.normal_channel)
        self._setup(proto.desc(), proto._layers(), dropout, momentum, chunk_rows, ctx, seed)
        self._generic = False

    @classmethod
    def from_desc(cls, desc, names, dropout=0.4, momentum=0.1, chunk_rows=0, ctx=None, *, seed=0):
        self = cls.__new__(cls)
        self.num_class, self.normal_channel = int(desc.fc_widths[desc.n_fc - 1]), int(desc.D0) == 3
        self._setup(desc, _desc_layers(desc, names), dropout, momentum, chunk_rows, ctx, seed)
        self._generic = True
        return self

    def _setup(self, desc, layers, dropout, momentum, chunk_rows, ctx, seed):
        self._desc, self._layer_list = desc, layers
        self.dropout = tuple(float(p) for p in dropout) if isinstance(dropout, (tuple, list)) else float(dropout)
        self.momentum, self.chunk_rows = float(momentum), int(chunk_rows)
        self._ctx_arg, self._trainer, self._trainer_ctx = ctx, None, None
        self._dirty = True                   # the host weights (running statistics included) are newer than the device's
        self._dev_ahead = False              # a DeviceOptimizer has stepped: the device's parameters are newer than the host mirror _flat
        self._grad_on_dev = False            # the last pass left its gradient on the device only
        self._optimizer = None               # the DeviceOptimizer attached to this trainer
        self._slots, off = {}, 0             # key -> (offset, shape) into the flat array
        for conv, bn, w, cin in layers:
            self._slots[f"{conv}.weight"] = (off, (w, cin, 1, 1) if _conv2d(conv) else (w, cin))
            off += w * cin
            self._slots[f"{conv}.bias"] = (off, (w,))
            off += w
            for k in (_BN_KEYS if bn else ()):
                self._slots[f"{bn}.{k}"] = (off, (w,))
                off += w
        self._flat = np.zeros(off, np.float32)
        self._gflat = np.zeros(off, np.float32)
        self._tracked = {bn: 0 for _, bn, _, _ in layers if bn}
        self._params = None
        rng = np.random.default_rng(seed)
        for conv, bn, w, cin in layers:
            bound = 1.0 / np.sqrt(cin)
            self._view(f"{conv}.weight")[...] = rng.uniform(-bound, bound, self._slots[f"{conv}.weight"][1])
            self._view(f"{conv}.bias")[...] = rng.uniform(-bound, bound, w)
            if bn:
                self._view(f"{bn}.weight")[...] = 1.0
                self._view(f"{bn}.running_var")[...] = 1.0

    def _view(self, key, flat=None):
        off, shape = self._slots[key]
        return (self._flat if flat is None else flat)[off:off + int(np.prod(shape))].reshape(shape)

    def param_keys(self):
        """the keys of named_parameters(), in the reference's order per layer: weight, bias, then the BN's weight, bias"""
        out = []
        for conv, bn, _, _ in self._layer_list:
            out += [f"{conv}.weight", f"{conv}.bias"] + ([f"{bn}.{k}" for k in _PARAM_BN] if bn else [])
        return out

    # ---- the device trainer
    def trainer(self, ctx=None):
        ctx = _ctx(ctx if ctx is not None else self._ctx_arg)
        if self._trainer is None or self._trainer_ctx is not ctx or not self._trainer.h:
            if self._trainer is not None:
                self._pull_all()
                self._trainer.free()
            self._trainer, self._trainer_ctx = self._make(ctx), ctx
            self._dirty = False
            if self._optimizer is not None:
                self._optimizer._attach(self._trainer)
        elif self._dirty:
            self._trainer.set_weights(self._flat, keep_running_stats=False)
            self._dirty = False
        return self._trainer

    def _make(self, ctx):
        """the device trainer of this class on ctx, from the host weights"""
        return ctx.pn2_trainer(self._desc, self._flat, self.dropout, self.momentum, self.chunk_rows)

    def _pull_all(self):
        """before the device trainer goes away: what state_dict() and grads() pull, and the optimiser's state"""
        self._pull_weights()
        self._pull_grad()
        self._dev_ahead = self._grad_on_dev = False
        if self._optimizer is not None:
            self._optimizer._save()

    def _pull_running(self):
        if self._trainer is None or not self._trainer.h or self._dirty:
            return
        dev = self._trainer.get_weights()
        for _, bn, _, _ in self._layer_list:
            if bn:
                for k in ("running_mean", "running_var"):
                    self._view(f"{bn}.{k}")[...] = self._view(f"{bn}.{k}", dev)

    def _pull_weights(self):
        """the running statistics, and after a DeviceOptimizer's step the parameters too, into the host mirror"""
        if self._dev_ahead and not self._dirty and self._trainer is not None and self._trainer.h:
            self._flat[...] = self._trainer.get_weights()
            self._dev_ahead = False
        else:
            self._pull_running()

    def info(self, n_obj=0, npts=0):
        return self.trainer().info(n_obj, npts)

    def optimizer(self, kind="Adam", lr=None, betas=(0.9, 0.999), eps=1e-08, weight_decay=0.0, momentum=0.0, dampening=0.0):
        """A DeviceOptimizer on this trainer: "Adam" (torch.optim.Adam, amsgrad off; lr defaults to 1e-3) or "SGD" (torch.optim.SGD, no nesterov; lr
        must be given).  It replaces the one the trainer had.  No device is touched before the first step."""
        self._optimizer = DeviceOptimizer(self, kind, lr, betas, eps, weight_decay, momentum, dampening)
        if self._trainer is not None and self._trainer.h:
            self._optimizer._attach(self._trainer)
        return self._optimizer

    # ---- state
    def state_dict(self):
        self._pull_weights()
        out = {}
        for conv, bn, _, _ in self._layer_list:
            out[f"{conv}.weight"] = self._view(f"{conv}.weight").copy()
            out[f"{conv}.bias"] = self._view(f"{conv}.bias").copy()
            if bn:
                for k in _BN_KEYS:
                    out[f"{bn}.{k}"] = self._view(f"{bn}.{k}").copy()
                out[f"{bn}.num_batches_tracked"] = np.int64(self._tracked[bn])
        return out

    def load_state_dict(self, state, strict=True):
        seen = set()
        for key, (off, shape) in self._slots.items():
            if key not in state:
                raise KeyError(f"missing key in state_dict: {key}")
            a = np.asarray(_to_host(state[key])[0], np.float32)
            if a.size != int(np.prod(shape)) or (a.ndim >= 1 and a.shape[0] != shape[0]):
                raise ValueError(f"size mismatch for {key}: {a.shape}, the model takes {shape}")
            self._view(key)[...] = a.reshape(shape)
            seen.add(key)
        for bn in self._tracked:
            k = f"{bn}.num_batches_tracked"
            self._tracked[bn] = int(np.asarray(_to_host(state[k])[0])) if k in state else 0
            seen.add(k)
        if strict:
            extra = [k for k in state if k not in seen]
            if extra:
                raise KeyError(f"unexpected keys in state_dict: {extra}")
        self._dirty, self._dev_ahead = True, False      # the host is the newer from here on; a DeviceOptimizer keeps its state, as torch's does
        return self

    # ---- the step
    def step_grad(self, points, target, start=None, seed=None, keep=None, *, ctx=None):
        """points [B, 3 | 6, N], target [B] or [B, 1] -> (loss, logp [B, num_class]), numpy / float or torch like `points`; every gradient is
        left in grads() and in the .grad of torch_parameters().  start: [n_sampling_layers, B] first FPS picks; keep: the dropout masks, one
        [B, width] array per FC layer but the last (or their concatenation); seed: draws whichever of the two is not given."""
        return self._pass(points, target, start, seed, keep, ctx, None)

    def _pass(self, points, target, start, seed, keep, ctx, lr):
        """step_grad (lr None), or the fused step at lr: the same pass, then the attached optimiser's update on the device; the gradient stays there"""
        x, proto = _to_host(points)
        C0 = 3 + int(self._desc.D0)
        if x.ndim != 3 or x.shape[1] != C0:
            raise ValueError(f"points: [B, {C0}, N]")
        B, N = x.shape[0], x.shape[2]
        tg = np.asarray(_to_host(target)[0]).reshape(-1)
        st, _ = _to_host(start)
        tr = self.trainer(ctx)
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
            if st is None:
                sizes = [N] + tr.sampling_npoints()[:-1]
                st = np.stack([np.random.randint(0, n, size=B) for n in sizes]) if tr.sampling_npoints() else None
        if keep is not None and isinstance(keep, (list, tuple)):
            keep = np.concatenate([np.asarray(_to_host(k)[0]).reshape(-1) for k in keep])
        elif keep is not None:
            keep = np.asarray(_to_host(keep)[0]).reshape(-1)
        obj = np.ascontiguousarray(np.transpose(x, (0, 2, 1)), np.float32)
        loss, logp, grad = tr.train_grad(obj, tg, st, seed, keep) if lr is None else tr.train_step(obj, tg, lr, st, seed, keep)
        if B:
            self._after_pass(grad)
        if proto is None:
            return loss, logp
        import torch
        return torch.tensor(loss, dtype=proto.dtype, device=proto.device), _like(logp, proto)

    def _after_pass(self, grad):
        """grad None: a fused step, the gradient stayed on the device and the device's parameters are now the newer"""
        if grad is None:
            self._grad_on_dev = self._dev_ahead = True
        else:
            self._gflat[...] = grad
            self._grad_on_dev = False
        for bn in self._tracked:
            self._tracked[bn] += 1

    def _pull_grad(self):
        if self._grad_on_dev and self._trainer is not None and self._trainer.h:
            self._gflat[...] = self._trainer.get_grad()
            self._grad_on_dev = False

    def grads(self):
        """key -> the gradient of the last step_grad in the reference's shape, for every key of named_parameters()"""
        self._pull_grad()
        return {k: self._view(k, self._gflat).copy() for k in self.param_keys()}

    def torch_parameters(self):
        """host torch tensors that SHARE the trainer's weights, in named_parameters() order, each with a .grad that shares the trainer's
        gradient: an optimiser's step() changes the trainer's host weights in place; sync() then uploads them"""
        import torch
        self._pull_weights()
        self._pull_grad()
        if self._params is None:
            self._params = []
            for k in self.param_keys():
                p = torch.from_numpy(self._view(k)).requires_grad_(True)
                p.grad = torch.from_numpy(self._view(k, self._gflat))
                self._params.append(p)
        else:
            for k, p in zip(self.param_keys(), self._params):      # zero_grad(set_to_none=True) drops the link: restore it
                if p.grad is None or p.grad.data_ptr() != self._view(k, self._gflat).ctypes.data:
                    p.grad = torch.from_numpy(self._view(k, self._gflat))
        return self._params

    def sync(self, *, ctx=None):
        """the host weights (after optimizer.step()) -> the device; the running statistics stay the device's"""
        if self._trainer is None or not self._trainer.h or self._dirty:
            self.trainer(ctx)
            return self
        if self._dev_ahead:                  # nothing on the host is newer than what a DeviceOptimizer left on the device
            return self
        self._trainer.set_weights(self._flat, keep_running_stats=True)
        return self

    def step(self, points, target, optimizer, **kw):
        """With a DeviceOptimizer: ONE fused call (the pass, then the update at optimizer.param_groups[0]["lr"]); the weights, the gradient and the
        optimiser's state stay on the device.  With a torch optimiser on torch_parameters(): step_grad -> relink the gradients -> optimizer.step()
        -> sync (zero_grad is not needed).  Returns step_grad's pair"""
        if isinstance(optimizer, DeviceOptimizer):
            if optimizer.trainer is not self or self._optimizer is not optimizer:
                raise ValueError("optimizer: not this trainer's (Trainer.optimizer makes it)")
            return self._pass(points, target, kw.get("start"), kw.get("seed"), kw.get("keep"), kw.get("ctx"), float(optimizer.param_groups[0]["lr"]))
        out = self.step_grad(points, target, **kw)
        self.torch_parameters()
        optimizer.step()
        self.sync()
        return out

    def eval_model(self):
        """a pointnet.get_model in eval mode loaded with the current weights and running statistics"""
        m = _DescModel(self.num_class, self._desc, self._layer_list) if self._generic else get_model(self.num_class, self.normal_channel)
        m.load_state_dict(self.state_dict(), strict=True)
        return m.eval()

    def train(self, mode=True):
        return self

    def free(self):
        if self._trainer is not None:
            self._pull_all()
            self._trainer.free()
        self._trainer, self._trainer_ctx = None, None
        self._dirty = True


class DeviceOptimizer:
    """torch.optim.Adam (amsgrad off, coupled weight decay) or torch.optim.SGD (momentum, dampening, weight decay, no nesterov) on the device trainer of a
    Trainer, with torch's surface where train_cls.py uses it.  Made by Trainer.optimizer.  param_groups[0]["lr"] is read at every step (StepLR writes
    it); the other hyper-parameters are fixed when the optimiser is made (or loaded).  The state lives on the device in the weight layout; state_dict /
    load_state_dict speak torch's layout: state[i] per parameter in the trainer's param_keys() order and the reference's shapes, plus param_groups."""

    def __init__(self, trainer, kind, lr, betas, eps, weight_decay, momentum, dampening):
        kind = {"adam": "Adam", "sgd": "SGD"}.get(str(kind).lower())
        if kind is None:
            raise ValueError('kind: "Adam" or "SGD"')
        if lr is None:
            if kind == "SGD":
                raise ValueError("lr: SGD has no default")
            lr = 1e-3
        self.trainer, self.kind = trainer, kind
        n = len(trainer.param_keys())
        if kind == "Adam":
            g = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay), amsgrad=False, maximize=False, foreach=None,
                     capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        else:
            g = dict(lr=float(lr), momentum=float(momentum), dampening=float(dampening), weight_decay=float(weight_decay), nesterov=False, maximize=False, foreach=None,
                     differentiable=False, fused=None)
        g["params"] = list(range(n))
        self.param_groups = [g]
        self._host = None                    # (step, state0, state1 or None) while the state is not on a device trainer
        self._dev = None

    # ---- the device side
    def _attach(self, dev):
        g = self.param_groups[0]
        dev.optim_set(self.kind, betas=g.get("betas", (0.9, 0.999)), eps=g.get("eps", 1e-8), weight_decay=g["weight_decay"], momentum=g.get("momentum", 0.0),
                      dampening=g.get("dampening", 0.0))
        if self._host is not None:
            dev.optim_set_state(*self._host)
        self._host, self._dev = None, dev

    def _save(self):
        """the state to the host: the device trainer is about to go away"""
        if self._dev is not None and self._dev.h:
            self._host = self._dev.optim_get_state()
        self._dev = None

    def _state(self):
        if self._dev is not None and self._dev.h:
            return self._dev.optim_get_state()
        if self._host is not None:
            return self._host
        n = self.trainer._flat.size
        return 0, np.zeros(n, np.float32), np.zeros(n, np.float32) if self.kind == "Adam" else None

    def info(self):
        """pcr_pn2_trainer_optim_info of the device trainer (made if there is none yet)"""
        return self.trainer.trainer().optim_info()

    # ---- torch's surface
    def zero_grad(self, set_to_none=True):
        """nothing: every pass overwrites the whole gradient"""

    def step(self):
        """one update from the gradient the last step_grad left on the device, at param_groups[0]["lr"]"""
        tr = self.trainer
        tr.trainer().optim_step(float(self.param_groups[0]["lr"]))
        tr._dev_ahead = True

    def state_dict(self, as_torch=False):
        """torch's optimizer.state_dict(): {"state": {i: {...}}, "param_groups": [...]}; the arrays numpy, or torch tensors with as_torch (what
        torch.optim's load_state_dict takes).  Before the first step the state is empty, as torch's is."""
        step, s0, s1 = self._state()
        tr, state = self.trainer, {}
        if as_torch:
            import torch
            conv = lambda a: torch.from_numpy(np.array(a))
        else:
            conv = lambda a: np.array(a)
        if step > 0:
            for i, k in enumerate(tr.param_keys()):
                if self.kind == "Adam":
                    state[i] = {"step": conv(np.float32(step)), "exp_avg": conv(tr._view(k, s0)), "exp_avg_sq": conv(tr._view(k, s1))}
                else:
                    state[i] = {"momentum_buffer": None if self.param_groups[0]["momentum"] == 0 else conv(tr._view(k, s0))}
        return {"state": state, "param_groups": [dict(g, params=list(g["params"])) for g in self.param_groups]}

    def load_state_dict(self, sd):
        """a state_dict of this class or of the torch optimiser of the same kind over the same parameters: the state, the step count and the
        hyper-parameters (the learning rate included) are the checkpoint's from here on"""
        tr = self.trainer
        keys = tr.param_keys()
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(keys):
            raise ValueError(f"param_groups: one group of {len(keys)} parameters")
        g = dict(groups[0])
        if ("betas" in g) != (self.kind == "Adam"):
            raise ValueError(f"the checkpoint is not {self.kind}'s")
        if g.get("amsgrad") or g.get("nesterov") or g.get("maximize") or g.get("decoupled_weight_decay"):
            raise ValueError("amsgrad, nesterov, maximize and decoupled weight decay are not built")
        n = tr._flat.size
        step, s0, s1 = 0, np.zeros(n, np.float32), np.zeros(n, np.float32) if self.kind == "Adam" else None
        state = sd["state"]
        if state:
            steps = set()
            for i, k in enumerate(keys):
                st = state[g["params"][i]]
                shape = tr._slots[k][1]
                for name, flat in (("exp_avg", s0), ("exp_avg_sq", s1)) if self.kind == "Adam" else (("momentum_buffer", s0),):
                    if st.get(name) is None:
                        continue
                    a = np.asarray(_to_host(st[name])[0], np.float32)
                    if a.shape != tuple(shape):
                        raise ValueError(f"size mismatch for {name} of {k}: {a.shape}, the parameter is {shape}")
                    tr._view(k, flat)[...] = a
                steps.add(int(np.asarray(_to_host(st["step"])[0])) if "step" in st else 1)
            if len(steps) != 1:
                raise ValueError("step: one count for all parameters")
            step = steps.pop()
        g["lr"] = float(g["lr"])
        if "betas" in g:
            g["betas"] = (float(g["betas"][0]), float(g["betas"][1]))
        g["params"] = list(range(len(keys)))
        self.param_groups = [g]
        self._host = (step, s0, s1)
        dev, self._dev = self._dev, None
        if dev is not None and dev.h:
            self._attach(dev)
        return self


class StepLR:
    """torch.optim.lr_scheduler.StepLR's recurrence: step() counts an epoch and, at every multiple of step_size, multiplies each group's lr by gamma
    (one f64 product per boundary, so the sequence is torch's to the bit).  Works on a DeviceOptimizer and on a torch optimiser."""

    def __init__(self, optimizer, step_size=20, gamma=0.7):
        self.optimizer, self.step_size, self.gamma, self.last_epoch = optimizer, int(step_size), float(gamma), 0
        for g in optimizer.param_groups:
            g.setdefault("initial_lr", g["lr"])
        self._last_lr = [g["lr"] for g in optimizer.param_groups]

    def step(self):
        self.last_epoch += 1
        if self.last_epoch % self.step_size == 0:
            for g in self.optimizer.param_groups:
                g["lr"] = g["lr"] * self.gamma
        self._last_lr = [g["lr"] for g in self.optimizer.param_groups]

    def get_last_lr(self):
        return list(self._last_lr)

    def state_dict(self):
        return {"step_size": self.step_size, "gamma": self.gamma, "last_epoch": self.last_epoch, "_last_lr": list(self._last_lr)}

    def load_state_dict(self, sd):
        self.step_size, self.gamma, self.last_epoch, self._last_lr = int(sd["step_size"]), float(sd["gamma"]), int(sd["last_epoch"]), list(sd["_last_lr"])


class get_loss:
    """models/pointnet2_cls_ssg.get_loss: (pred [B, num_class] log-probabilities, target [B], trans_feat ignored) -> the mean of
    -pred[b, target[b]] (F.nll_loss), a float for numpy input, a tensor like pred for torch input.  The sum runs in f64 over ascending b."""

    def forward(self, pred, target, trans_feat=None):
        p, proto = _to_host(pred)
        t = np.asarray(_to_host(target)[0]).reshape(-1).astype(np.int64)
        p = np.asarray(p, np.float64)
        s = 0.0
        for b in range(p.shape[0]):
            s += p[b, t[b]]
        loss = -s / max(p.shape[0], 1)
        if proto is None:
            return float(loss)
        import torch
        return torch.tensor(loss, dtype=proto.dtype, device=proto.device)

    __call__ = forward


# ---------------------------------------------------------------------------------------------------- the vanilla PointNet (pointnet_cls)
def _cls_layers(desc):
    """(conv / linear prefix, BN prefix or None, out, in) in weight order for a Pn1Desc, with the reference's names (feat.stn.*, feat.conv1 ...,
    feat.fstn.*, fc1 / bn1 ...)"""
    tc, tf = [int(w) for w in desc.tnet_conv], [int(w) for w in desc.tnet_fc]

    def tnet(prefix, cin, k):
        out = []
        for i, w in enumerate(tc):
            out.append((f"{prefix}.conv{i + 1}", f"{prefix}.bn{i + 1}", w, cin))
            cin = w
        for i, w in enumerate(tf):
            out.append((f"{prefix}.fc{i + 1}", f"{prefix}.bn{len(tc) + i + 1}", w, cin))
            cin = w
        return out + [(f"{prefix}.fc{len(tf) + 1}", None, k * k, cin)]

    cin = 3 + int(desc.D0)
    out = tnet("feat.stn", cin, 3) if desc.stn3 else []
    for i in range(desc.n_mlp):
        out.append((f"feat.conv{i + 1}", f"feat.bn{i + 1}", int(desc.widths[i]), cin))
        cin = int(desc.widths[i])
    if desc.fstn:
        out += tnet("feat.fstn", int(desc.widths[0]), int(desc.widths[0]))
    for i in range(desc.n_fc):
        out.append((f"fc{i + 1}", f"bn{i + 1}" if i + 1 < desc.n_fc else None, int(desc.fc_widths[i]), cin))
        cin = int(desc.fc_widths[i])
    return out


class _DescModelCls(get_model_cls):
    """pointnet.get_model_cls for the layers and the descriptor of a TrainerCls.from_desc"""

    def __init__(self, k, desc, layers):
        super().__init__(k, int(desc.D0) == 3)
        self._d, self._l = desc, layers

    def _layers(self):
        return list(self._l)

    def desc(self):
        return self._d

    def state_shapes(self):
        out = {}
        for conv, bn, w, cin in self._l:
            out[f"{conv}.weight"] = (w, cin, 1) if ".conv" in conv else (w, cin)
            out[f"{conv}.bias"] = (w,)
            for k in (_BN_KEYS if bn else ()):
                out[f"{bn}.{k}"] = (w,)
        return out


class TrainerCls(Trainer):
    """The reference's pointnet_cls.get_model in TRAINING mode on the library, with Trainer's whole surface.  TrainerCls(k, normal_channel, dropout,
    momentum, mat_diff_loss_scale, chunk_rows, ctx) is the reference's architecture; TrainerCls.from_desc(desc) any Pn1Desc (the reference's key
    names).  step_grad returns (loss, logp) with loss = nll + mat_diff_loss_scale x the regulariser, as pointnet_cls.get_loss gives it, and keeps
    last_nll, last_reg, last_trans and last_trans_feat.  Nothing is sampled: only the dropout mask is drawn (keep= fixes it)."""

    def __init__(self, k=40, normal_channel=True, dropout=0.4, momentum=0.1, mat_diff_loss_scale=0.001, chunk_rows=0, ctx=None, *, seed=0):
        self.num_class = self.k = int(k)
        self.normal_channel = bool(normal_channel)
        proto = get_model_cls(self.k, self.normal_channel)
        self._setup_cls(proto.desc(), proto._layers(), dropout, momentum, mat_diff_loss_scale, chunk_rows, ctx, seed)
        self._generic = False

    @classmethod
    def from_desc(cls, desc, dropout=0.4, momentum=0.1, mat_diff_loss_scale=0.001, chunk_rows=0, ctx=None, *, seed=0):
        self = cls.__new__(cls)
        self.num_class = self.k = int(desc.fc_widths[desc.n_fc - 1])
        self.normal_channel = int(desc.D0) == 3
        self._setup_cls(desc, _cls_layers(desc), dropout, momentum, mat_diff_loss_scale, chunk_rows, ctx, seed)
        self._generic = True
        return self

    def _setup_cls(self, desc, layers, dropout, momentum, scale, chunk_rows, ctx, seed):
        self._setup(desc, layers, dropout, momentum, chunk_rows, ctx, seed)
        self.mat_diff_loss_scale = float(scale)
        for conv, _, w, cin in layers:                           # Conv1d weights are [out, in, 1] in the reference's state dict
            if ".conv" in conv:
                self._slots[f"{conv}.weight"] = (self._slots[f"{conv}.weight"][0], (w, cin, 1))
        self.last_nll = self.last_reg = self.last_trans = self.last_trans_feat = None

    def param_keys(self):
        """the keys of named_parameters() in the reference's order: module by module (feat.stn, feat, feat.fstn, the head), the convolutions and
        linear layers of a module before its BatchNorms"""
        groups = {}
        for conv, bn, _, _ in self._layer_list:
            g = groups.setdefault(conv.rsplit(".", 1)[0] if "." in conv else "", ([], []))
            g[0].append(conv)
            if bn:
                g[1].append(bn)
        return [f"{m}.{p}" for convs, bns in groups.values() for m in convs + bns for p in _PARAM_BN]

    def _make(self, ctx):
        return ctx.pn1_trainer(self._desc, self._flat, self.dropout, self.momentum, self.mat_diff_loss_scale, self.chunk_rows)

    def step_grad(self, points, target, seed=None, keep=None, *, ctx=None):
        """points [B, 3 | 6, N], target [B] or [B, 1] -> (loss, logp [B, k]), numpy / float or torch like `points`; every gradient is left in
        grads() and in the .grad of torch_parameters().  keep: the dropout mask [B, width of the last hidden FC layer]; seed: draws it otherwise
        (None: a seed from np.random)."""
        return self._pass(points, target, None, seed, keep, ctx, None)

    def _pass(self, points, target, start, seed, keep, ctx, lr):
        x, proto = _to_host(points)
        C0 = 3 + int(self._desc.D0)
        if x.ndim != 3 or x.shape[1] != C0:
            raise ValueError(f"points: [B, {C0}, N]")
        B = x.shape[0]
        tg = np.asarray(_to_host(target)[0]).reshape(-1)
        tr = self.trainer(ctx)
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        if keep is not None:
            keep = np.asarray(_to_host(keep)[0]).reshape(-1)
        obj = np.ascontiguousarray(np.transpose(x, (0, 2, 1)), np.float32)
        res = tr.train_grad(obj, tg, seed, keep) if lr is None else tr.train_step(obj, tg, lr, seed, keep)
        if B:
            self._after_pass(res["grad"])
            self.last_nll, self.last_reg, self.last_trans, self.last_trans_feat = res["nll"], res["reg"], res["trans"], res["trans_feat"]
        if proto is None:
            return res["loss"], res["logp"]
        import torch
        return torch.tensor(res["loss"], dtype=proto.dtype, device=proto.device), _like(res["logp"], proto)

    def eval_model(self):
        """a pointnet.get_model_cls in eval mode loaded with the current weights and running statistics"""
        m = _DescModelCls(self.k, self._desc, self._layer_list) if self._generic else get_model_cls(self.k, self.normal_channel)
        m.load_state_dict(self.state_dict(), strict=True)
        return m.eval()


class get_loss_cls:
    """models/pointnet_cls.get_loss: (pred [B, k] log-probabilities, target [B], trans_feat [B, K, K]) -> F.nll_loss + mat_diff_loss_scale x
    the mean over objects of the Frobenius norm of A (A^T - I), on the host in f64; a float for numpy input, a tensor like pred for torch input."""

    def __init__(self, mat_diff_loss_scale=0.001):
        self.mat_diff_loss_scale = float(mat_diff_loss_scale)

    def forward(self, pred, target, trans_feat):
        p, proto = _to_host(pred)
        nll = float(get_loss()(np.asarray(p, np.float64), np.asarray(_to_host(target)[0])))
        A = np.asarray(_to_host(trans_feat)[0], np.float64)
        eye = np.eye(A.shape[1])[None]
        M = A @ (np.transpose(A, (0, 2, 1)) - eye)
        reg = float(np.mean(np.sqrt((M * M).sum((1, 2))))) if len(A) else 0.0
        loss = nll + reg * self.mat_diff_loss_scale
        if proto is None:
            return float(loss)
        import torch
        return torch.tensor(loss, dtype=proto.dtype, device=proto.device)

    __call__ = forward


# ---------------------------------------------------------------------------------------------------- PointNet++ multi-scale (pointnet2_cls_msg)
class TrainerMsg(Trainer):
    """The reference's pointnet2_cls_msg.get_model in TRAINING mode on the library, with Trainer's whole surface.  TrainerMsg(num_class,
    normal_channel, dropout, momentum, chunk_rows, ctx) is the reference's architecture (normal_channel defaults to False, as on Trainer);
    TrainerMsg.from_desc(desc, names, dropout) any Pn2MsgDesc whose last SA layer is group_all (names: one (conv prefix, BN prefix or None) per
    layer in weight order: layer by layer, branch by branch).  dropout: one probability per FC layer but the last (the reference: drop1 0.4,
    drop2 0.5); a number stands for all of them.  The state-dict keys are the reference's (sa1.conv_blocks.0.0.weight,
    sa1.bn_blocks.0.0.running_mean ..., sa3.mlp_convs.0.weight, fc1 / bn1 ...), as pointnet.get_model_msg speaks them."""

    def __init__(self, num_class, normal_channel=False, dropout=(0.4, 0.5), momentum=0.1, chunk_rows=0, ctx=None, *, seed=0):
        self.num_class, self.normal_channel = int(num_class), bool(normal_channel)
        proto = get_model_msg(self.num_class, self.normal_channel)
        self._setup(proto.desc(), proto._layers(), self._dropouts(dropout, 3), momentum, chunk_rows, ctx, seed)
        self._generic = False

    @classmethod
    def from_desc(cls, desc, names, dropout=(0.4, 0.5), momentum=0.1, chunk_rows=0, ctx=None, *, seed=0):
        self = cls.__new__(cls)
        self.num_class, self.normal_channel = int(desc.fc_widths[desc.n_fc - 1]), int(desc.D0) == 3
        self._setup(desc, _desc_layers(desc, names), cls._dropouts(dropout, int(desc.n_fc)), momentum, chunk_rows, ctx, seed)
        self._generic = True
        return self

    @staticmethod
    def _dropouts(dropout, n_fc):
        ps = tuple(float(p) for p in dropout) if isinstance(dropout, (tuple, list, np.ndarray)) else (float(dropout),) * (n_fc - 1)
        if len(ps) != n_fc - 1:
            raise ValueError(f"dropout: one probability per FC layer but the last, the model has {n_fc - 1}")
        return ps

    def _make(self, ctx):
        return ctx.pn2_msg_trainer(self._desc, self._flat, self.dropout, self.momentum, self.chunk_rows)

    def eval_model(self):
        """a pointnet.get_model_msg in eval mode loaded with the current weights and running statistics"""
        m = _DescModelMsg(self.num_class, self._desc, self._layer_list) if self._generic else get_model_msg(self.num_class, self.normal_channel)
        m.load_state_dict(self.state_dict(), strict=True)
        return m.eval()


# the trainers by the reference's module name (train_cls.py --model): the two first built, and all of them
TRAINERS = {"pointnet2_cls_ssg": Trainer, "pointnet_cls": TrainerCls}
ALL_TRAINERS = {**TRAINERS, "pointnet2_cls_msg": TrainerMsg}
