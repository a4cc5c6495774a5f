"""HomeworkFinal's PointNet++ sampling / grouping operators and its object extraction, on the GPU.

Mirrors (same names, argument order and return shapes):
  farthest_point_sample   HomeworkFinal/models/pointnet_util.py:66-87     (GPU: pcr_fps_f32, PCR_FPS_F32)
  query_ball_point        HomeworkFinal/models/pointnet_util.py:90-116    (GPU: pcr_ball_query_f32)
  index_points            HomeworkFinal/models/pointnet_util.py:46-63     (host indexing: it is a gather of a few KB)
  sample_and_group        HomeworkFinal/models/pointnet_util.py:119-156   (GPU: the three operators, one fused gather)
  get_model               HomeworkFinal/models/pointnet2_cls_ssg.py           (GPU: pcr_pn2_forward_f32, eval mode only)
  get_model_msg           HomeworkFinal/models/pointnet2_cls_msg.py           (GPU: the same call on a multi-scale model, eval mode only)
  get_model_cls           HomeworkFinal/models/pointnet_cls.py + pointnet.py  (GPU: pcr_pointnet_forward_f32, the vanilla PointNet with its T-Nets, eval mode only)
  MODELS                  the two PointNet++ models by the module name train_cls.py --model / test_cls.py import
  CLASSIFIERS             all three by that name (MODELS and pointnet_cls)
  classify_foreground_objects   the flow of HomeworkFinal/foreground_obj_cls.py:97-188: up to the classifier's input, or with
                          classifier= through it to pred_final

The functions take [B, N, C] numpy arrays or torch tensors and return the same kind (indices as int64, like the reference).  Torch is
plumbing here: a tensor is brought to the host, the library works on its own device cloud, and the result is put back on the tensor's
device — one host round trip per call, no zero-copy hand-over.  There is no CPU fallback: without the library or a GPU a call raises.

What is unpinned: the reference draws the first FPS pick unseeded (torch.randint); pass `start=` to fix it, else it is drawn from
np.random.  Written from the contracts in include/pcr.h.
"""
from __future__ import annotations

import numpy as np

from . import PCR_AOS3, PCR_FPS_F32


def _ctx(ctx):
    if ctx is not None:
        return ctx
    from .hw4 import default_context
    return default_context()


def _to_host(a):
    """-> (numpy array, None) or (numpy array, the torch tensor it came from)"""
    if isinstance(a, np.ndarray) or a is None:
        return a, None
    if hasattr(a, "detach") and hasattr(a, "cpu"):
        return a.detach().cpu().numpy(), a
    return np.asarray(a), None


def _like(out, proto, integer=False):
    if proto is None:
        return out
    import torch
    t = torch.from_numpy(np.ascontiguousarray(out))
    return t.to(proto.device) if integer else t.to(device=proto.device, dtype=proto.dtype)


def _batch_cloud(ctx, xyz):
    """[B, N, 3] -> (device cloud of B * N points, seg_ptr)"""
    B, N = xyz.shape[0], xyz.shape[1]
    cloud = ctx.cloud(np.ascontiguousarray(xyz[..., :3], np.float32).reshape(B * N, 3), PCR_AOS3)
    return cloud, (np.arange(B + 1, dtype=np.int64) * N).astype(np.uint32)


def farthest_point_sample(xyz, npoint, start=None, *, ctx=None, mode=PCR_FPS_F32):
    """[B, N, 3] -> indices [B, npoint] (int64).  start: [B] first picks; None draws them as the reference does (unseeded)."""
    x, proto = _to_host(xyz)
    B, N = x.shape[0], x.shape[1]
    st, _ = _to_host(start)
    if st is None:
        st = np.random.randint(0, N, size=B)
    ctx = _ctx(ctx)
    cloud, seg = _batch_cloud(ctx, x)
    try:
        idx = ctx.fps(cloud, seg, int(npoint), np.asarray(st).reshape(B), mode)
    finally:
        cloud.free()
    return _like(idx.astype(np.int64), proto, integer=True)


def query_ball_point(radius, nsample, xyz, new_xyz, *, ctx=None):
    """xyz [B, N, 3], new_xyz [B, S, 3] -> group_idx [B, S, nsample] (int64); a row without a point in the ball holds N."""
    x, proto = _to_host(xyz)
    q, _ = _to_host(new_xyz)
    B, S = q.shape[0], q.shape[1]
    ctx = _ctx(ctx)
    cloud, seg = _batch_cloud(ctx, x)
    centres, cseg = _batch_cloud(ctx, q)
    try:
        idx, _ = ctx.ball_query(cloud, seg, centres, cseg, radius, int(nsample))
    finally:
        cloud.free()
        centres.free()
    return _like(idx.astype(np.int64).reshape(B, S, int(nsample)), proto, integer=True)


def index_points(points, idx):
    """points [B, N, C], idx [B, S] or [B, S, K] -> points gathered per batch row, [B, S, C] or [B, S, K, C]."""
    p, proto = _to_host(points)
    i, _ = _to_host(idx)
    i = np.asarray(i, np.int64)
    b = np.arange(p.shape[0]).reshape((-1,) + (1,) * (i.ndim - 1))
    return _like(p[b, i, :], proto)


def sample_and_group(npoint, radius, nsample, xyz, points, returnfps=False, *, start=None, ctx=None):
    """xyz [B, N, 3], points [B, N, D] or None -> (new_xyz [B, npoint, 3], new_points [B, npoint, nsample, 3 + D]) and, with
    returnfps, also (grouped_xyz [B, npoint, nsample, 3], fps_idx [B, npoint]).  The cloud is uploaded once for the three operators."""
    x, proto = _to_host(xyz)
    f, _ = _to_host(points)
    B, N = x.shape[0], x.shape[1]
    S, K = int(npoint), int(nsample)
    st, _ = _to_host(start)
    if st is None:
        st = np.random.randint(0, N, size=B)
    ctx = _ctx(ctx)
    cloud, seg = _batch_cloud(ctx, x)
    centres = None
    try:
        fps_idx = ctx.fps(cloud, seg, S, np.asarray(st).reshape(B), PCR_FPS_F32)
        flat = np.ascontiguousarray(x[..., :3], np.float32).reshape(B * N, 3)
        cpos = (fps_idx.astype(np.int64) + (np.arange(B, dtype=np.int64) * N)[:, None]).reshape(-1)
        centres = ctx.cloud(flat[cpos], PCR_AOS3)
        cseg = (np.arange(B + 1, dtype=np.int64) * S).astype(np.uint32)
        idx, _ = ctx.ball_query(cloud, seg, centres, cseg, radius, K)
        feat = None if f is None else np.ascontiguousarray(f, np.float32).reshape(B * N, -1)
        new_xyz, new_points = ctx.group_points(cloud, seg, centres, cseg, idx, feat)
    finally:
        cloud.free()
        if centres is not None:
            centres.free()
    new_xyz = new_xyz.reshape(B, S, 3)
    new_points = new_points.reshape(B, S, K, -1)
    if not returnfps:
        return _like(new_xyz, proto), _like(new_points, proto)
    grouped_xyz = x[np.arange(B)[:, None, None], idx.astype(np.int64).reshape(B, S, K), :3].astype(np.float32)
    return _like(new_xyz, proto), _like(new_points, proto), _like(grouped_xyz, proto), _like(fps_idx.astype(np.int64), proto, integer=True)


# the reference's layers (pointnet2_cls_ssg.py:13-24): name in the state dict, npoint, radius, nsample, widths
_SSG_SA = (("sa1", 64, 0.2, 8, (64, 64, 128)), ("sa2", 32, 0.4, 16, (128, 128, 256)), ("sa3", None, None, None, (256, 512, 1024)))
_SSG_FC = (("fc1", "bn1", 512), ("fc2", "bn2", 256), ("fc3", None, None))
_BN_KEYS = ("weight", "bias", "running_mean", "running_var")


class get_model:
    """models/pointnet2_cls_ssg.get_model in eval mode on the library: the same constructor arguments, state-dict keys and call.
    load_state_dict takes the reference's checkpoint entries (Conv2d weights [out, in, 1, 1] or [out, in]; torch tensors or numpy arrays;
    num_batches_tracked is ignored); the model is uploaded (BN folded) on the first call and again after the next load_state_dict.
    __call__(xyz [B, 3 or 6, N]) -> (log_probs [B, num_class], l3_points [B, 1024, 1]), numpy or torch like the input; start= fixes the
    first FPS pick of both sampling layers ([2, B]; None draws them from np.random as the reference draws them unseeded), ctx= the context.
    Training is out of scope: train() raises."""

    _npoint1 = _SSG_SA[0][1]          # the size of the second sampling layer's cloud

    def __init__(self, num_class, normal_channel=False):
        self.num_class, self.normal_channel = int(num_class), bool(normal_channel)
        self.training = True
        self._state, self._model, self._model_ctx = None, None, None

    # ---- the layers in weight order: (prefix of the conv / linear, prefix of its BN or None, out, in)
    def _layers(self):
        out, last = [], 6 if self.normal_channel else 3
        for name, _, _, _, mlp in _SSG_SA:
            cin = last if name == "sa1" else last + 3
            for i, w in enumerate(mlp):
                out.append((f"{name}.mlp_convs.{i}", f"{name}.mlp_bns.{i}", w, cin))
                cin = w
            last = cin
        cin = last
        for fc, bn, w in _SSG_FC:
            w = self.num_class if w is None else w
            out.append((fc, bn, w, cin))
            cin = w
        return out

    def desc(self):
        from . import pn2_desc
        sa = [dict(group_all=True, mlp=mlp) if npoint is None else dict(npoint=npoint, radius=radius, nsample=nsample, mlp=mlp)
              for _, npoint, radius, nsample, mlp in _SSG_SA]
        return pn2_desc(sa, [512, 256, self.num_class], D0=3 if self.normal_channel else 0, bn_eps=1e-5)

    def state_dict(self):
        return dict(self._state or {})

    def load_state_dict(self, state, strict=True):
        new = {}
        for conv, bn, w, cin in self._layers():
            keys = [(f"{conv}.weight", (w, cin)), (f"{conv}.bias", (w,))] + ([(f"{bn}.{k}", (w,)) for k in _BN_KEYS] if bn else [])
            for key, shape in keys:
                if key not in state:
                    raise KeyError(f"missing key in state_dict: {key}")
                a = np.asarray(_to_host(state[key])[0], np.float32)
                if a.size != int(np.prod(shape)) or a.reshape(-1).size != a.size or (a.ndim >= 1 and a.shape[0] != shape[0]):
                    raise ValueError(f"size mismatch for {key}: {a.shape}, the model takes {shape}")
                new[key] = np.ascontiguousarray(a.reshape(shape))
        if strict:
            extra = [k for k in state if k not in new and not k.endswith("num_batches_tracked")]
            if extra:
                raise KeyError(f"unexpected keys in state_dict: {extra}")
        self._state = new
        self._drop()
        return self

    def state_shapes(self):
        """key -> shape of every entry load_state_dict takes, as the reference's state_dict() has them (Conv2d weights [out, in, 1, 1])"""
        out = {}
        for conv, bn, w, cin in self._layers():
            out[f"{conv}.weight"] = (w, cin, 1, 1) if conv.startswith("sa") else (w, cin)
            out[f"{conv}.bias"] = (w,)
            for k in (_BN_KEYS if bn else ()):
                out[f"{bn}.{k}"] = (w,)
        return out

    def flat_weights(self):
        """the flat f32 array pcr_pn2_model_create / pcr_pn2_msg_model_create takes"""
        if self._state is None:
            raise RuntimeError("no weights: call load_state_dict first (the reference ships no checkpoint)")
        parts = []
        for conv, bn, _, _ in self._layers():
            parts += [self._state[f"{conv}.weight"].reshape(-1), self._state[f"{conv}.bias"]]
            if bn:
                parts += [self._state[f"{bn}.{k}"] for k in _BN_KEYS]
        return np.concatenate(parts).astype(np.float32)

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("training is out of scope: the library runs the eval-mode forward pass only")
        return self.eval()

    def _drop(self):
        if self._model is not None:
            self._model.free()
        self._model, self._model_ctx = None, None

    def model(self, ctx=None):
        """the device model on ctx (uploaded once per context and state dict)"""
        ctx = _ctx(ctx)
        if self._model is None or self._model_ctx is not ctx or not self._model.h:
            self._drop()
            self._model, self._model_ctx = self._upload(ctx), ctx
        return self._model

    def _upload(self, ctx):
        return ctx.pn2_model(self.desc(), self.flat_weights())

    def forward(self, xyz, *, start=None, seed=None, ctx=None, return_all=False):
        if self.training:
            raise RuntimeError("the model is in training mode: call eval() (BatchNorm batch statistics and dropout are out of scope)")
        x, proto = _to_host(xyz)
        C0 = 6 if self.normal_channel else 3
        if x.ndim != 3 or x.shape[1] != C0:
            raise ValueError(f"xyz: [B, {C0}, N]")
        B, N = x.shape[0], x.shape[2]
        st, _ = _to_host(start)
        if st is None and seed is None:
            st = np.stack([np.random.randint(0, N, size=B), np.random.randint(0, self._npoint1, size=B)])
        ctx = _ctx(ctx)
        res = ctx.pn2_forward(self.model(ctx), np.ascontiguousarray(np.transpose(x, (0, 2, 1)), np.float32), st, 0 if seed is None else seed, return_all=True)
        out = _like(res["logp"], proto), _like(res["global_feat"][:, :, None], proto)
        return out + (res,) if return_all else out

    __call__ = forward


# the reference's layers (pointnet2_cls_msg.py:11-15): name, npoint, radii, nsamples, one list of widths per radius
_MSG_SA = (("sa1", 512, (0.1, 0.2, 0.4), (16, 32, 128), ((32, 32, 64), (64, 64, 128), (64, 96, 128))),
           ("sa2", 128, (0.2, 0.4, 0.8), (32, 64, 128), ((64, 64, 128), (128, 128, 256), (128, 128, 256))))
_MSG_SA3 = (256, 512, 1024)


class get_model_msg(get_model):
    """models/pointnet2_cls_msg.get_model in eval mode on the library: the same constructor arguments (normal_channel defaults to True, as
    there), state-dict keys (sa1.conv_blocks.{i}.{j}.*, sa1.bn_blocks.{i}.{j}.*, sa3.mlp_convs.{j}.*, fc1 / bn1 ...) and call.  sa1 and sa2
    are PointNetSetAbstractionMsg layers — three radii over one set of centres, input channels (features | xyz - centre) — and sa3 is the
    group_all PointNetSetAbstraction (xyz first).  Everything else is get_model's: load_state_dict, eval, train() raising, and
    __call__(xyz [B, 3 or 6, N], start=, seed=, ctx=, return_all=) -> (log_probs, l3_points [B, 1024, 1])."""

    _npoint1 = _MSG_SA[0][1]

    def __init__(self, num_class, normal_channel=True):
        super().__init__(num_class, normal_channel)

    def _layers(self):
        out, last = [], 3 if self.normal_channel else 0
        for name, _, _, _, mlps in _MSG_SA:
            width = 0
            for i, mlp in enumerate(mlps):
                cin = last + 3
                for j, w in enumerate(mlp):
                    out.append((f"{name}.conv_blocks.{i}.{j}", f"{name}.bn_blocks.{i}.{j}", w, cin))
                    cin = w
                width += cin
            last = width
        cin = last + 3
        for j, w in enumerate(_MSG_SA3):
            out.append((f"sa3.mlp_convs.{j}", f"sa3.mlp_bns.{j}", w, cin))
            cin = w
        for fc, bn, w in _SSG_FC:
            w = self.num_class if w is None else w
            out.append((fc, bn, w, cin))
            cin = w
        return out

    def desc(self):
        from . import pn2_msg_desc
        sa = [dict(npoint=npoint, xyz_last=True, branches=[dict(radius=r, nsample=k, mlp=mlp) for r, k, mlp in zip(radii, nsamples, mlps)])
              for _, npoint, radii, nsamples, mlps in _MSG_SA]
        sa.append(dict(group_all=True, mlp=_MSG_SA3))
        return pn2_msg_desc(sa, [512, 256, self.num_class], D0=3 if self.normal_channel else 0, bn_eps=1e-5)

    def _upload(self, ctx):
        return ctx.pn2_msg_model(self.desc(), self.flat_weights())


# the reference's layers (pointnet.py:10-24, :50-65, :89-101; pointnet_cls.py:15-22)
_CLS_ENC = (64, 128, 1024)
_CLS_TNET_CONV, _CLS_TNET_FC = (64, 128, 1024), (512, 256)


class get_model_cls(get_model):
    """models/pointnet_cls.get_model in eval mode on the library: the same constructor arguments and defaults (k=40, normal_channel=True),
    state-dict keys (feat.stn.conv1.weight ... feat.stn.fc3.bias, feat.conv1 ... feat.bn3, feat.fstn.*, fc1 / bn1 / fc2 / bn2 / fc3; Conv1d
    weights [out, in, 1] or [out, in]) and call.  __call__(x [B, 3 or 6, N], ctx=, return_all=) -> (log_probs [B, k], trans_feat [B, 64, 64]),
    numpy or torch like the input; with return_all a third value, the dict of Context.pointnet_forward.  The model samples nothing, so nothing is
    drawn: start= and seed= are accepted, as on the sibling classes, and ignored.  Everything else is get_model's: load_state_dict, eval,
    train() raising, state_shapes, flat_weights."""

    def __init__(self, k=40, normal_channel=True):
        super().__init__(k, normal_channel)
        self.k = self.num_class

    @staticmethod
    def _tnet(prefix, cin, k):
        out = []
        for i, w in enumerate(_CLS_TNET_CONV):
            out.append((f"{prefix}.conv{i + 1}", f"{prefix}.bn{i + 1}", w, cin))
            cin = w
        for i, w in enumerate(_CLS_TNET_FC):
            out.append((f"{prefix}.fc{i + 1}", f"{prefix}.bn{len(_CLS_TNET_CONV) + i + 1}", w, cin))
            cin = w
        return out + [(f"{prefix}.fc{len(_CLS_TNET_FC) + 1}", None, k * k, cin)]

    def _layers(self):
        channel = 6 if self.normal_channel else 3
        out, cin = self._tnet("feat.stn", channel, 3), channel
        for i, w in enumerate(_CLS_ENC):
            out.append((f"feat.conv{i + 1}", f"feat.bn{i + 1}", w, cin))
            cin = w
        out += self._tnet("feat.fstn", _CLS_ENC[0], _CLS_ENC[0])
        for fc, bn, w in _SSG_FC:
            w = self.num_class if w is None else w
            out.append((fc, bn, w, cin))
            cin = w
        return out

    def desc(self):
        from . import pn1_desc
        return pn1_desc(_CLS_ENC, [512, 256, self.num_class], D0=3 if self.normal_channel else 0, tnet_conv=_CLS_TNET_CONV, tnet_fc=_CLS_TNET_FC, bn_eps=1e-5)

    def state_shapes(self):
        """key -> shape of every entry load_state_dict takes, as the reference's state_dict() has them (Conv1d weights [out, in, 1])"""
        out = {}
        for conv, bn, w, cin in self._layers():
            out[f"{conv}.weight"] = (w, cin, 1) if ".conv" in conv else (w, cin)
            out[f"{conv}.bias"] = (w,)
            for k in (_BN_KEYS if bn else ()):
                out[f"{bn}.{k}"] = (w,)
        return out

    def _upload(self, ctx):
        return ctx.pn1_model(self.desc(), self.flat_weights())

    def forward(self, x, *, start=None, seed=None, ctx=None, return_all=False):
        if self.training:
            raise RuntimeError("the model is in training mode: call eval() (BatchNorm batch statistics and dropout are out of scope)")
        a, proto = _to_host(x)
        C0 = 6 if self.normal_channel else 3
        if a.ndim != 3 or a.shape[1] != C0:
            raise ValueError(f"x: [B, {C0}, N]")
        ctx = _ctx(ctx)
        res = ctx.pointnet_forward(self.model(ctx), np.ascontiguousarray(np.transpose(a, (0, 2, 1)), np.float32), return_all=True)
        out = _like(res["logp"], proto), _like(res["trans_feat"], proto)
        return out + (res,) if return_all else out

    __call__ = forward


# the PointNet++ classifiers by the reference's module name (train_cls.py --model, test_cls.py), and every classifier by that name
MODELS = {"pointnet2_cls_ssg": get_model, "pointnet2_cls_msg": get_model_msg}
CLASSIFIERS = dict(MODELS, pointnet_cls=get_model_cls)


def classify_foreground_objects(points, npoints=256, eps=0.5, min_points=8, z_min_above_ground=0.5, z_extent=(1.0, 2.3), seed=0, *, ctx=None,
                                preprocess=True, classifier=None):
    """foreground_obj_cls.py:97-188: pcd_preprocessing -> ground_detection_on3segs -> ground_z = mean z of the ground ->
    cluster_dbscan(eps, min_points) on the foreground -> objects_from_labels (-> the classifier).  points: (N, >= 3) scan rows.
    Without a classifier (the reference ships no weights) returns (objects f32 [n_obj, npoints, 3], codes i32 [n_clusters]: 3 where the
    reference writes 3, -1 = to be classified) and a dict with everything in between (points, ground / foreground indices, ground_z,
    labels, n_clusters, and the outputs of Context.objects_from_labels).
    With classifier= (a get_model, get_model_msg or get_model_cls in eval mode) every object goes through it in ONE batched forward pass (the first FPS picks, where the model samples, drawn from
    `seed`) and the second value is pred_final as the reference builds it (:152-188): i32 [n_clusters], 3 where it writes 3, the predicted
    class elsewhere; the dict then also holds log_probs [n_obj, num_class]."""
    from . import hw4
    ctx = _ctx(ctx)
    pts = np.asarray(points)[:, :3]
    pts = hw4.pcd_preprocessing(pts, ctx=ctx) if preprocess else np.asarray(pts, np.float64)
    ground_idx, foreground_idx = hw4.ground_detection_on3segs(pts, ctx=ctx)
    ground_z = float(np.mean(pts[ground_idx, 2])) if ground_idx.size else 0.0
    fg = np.ascontiguousarray(pts[foreground_idx], np.float32)
    cloud = ctx.cloud(fg, PCR_AOS3)
    try:
        labels, _, _, n_clusters = ctx.dbscan(cloud, eps, min_points)
        res = ctx.objects_from_labels(cloud, labels, n_clusters, npoints, ground_z, z_min_above_ground, z_extent, seed)
    finally:
        cloud.free()
    res.update(points=pts, ground_idx=ground_idx, foreground_idx=foreground_idx, ground_z=ground_z, labels=labels, n_clusters=n_clusters)
    if classifier is None:
        return res["objects"], res["codes"], res
    pred_final = np.array(res["codes"], np.int32)
    objects = np.asarray(res["objects"], np.float32)
    if len(objects):
        _, _, out = classifier(np.transpose(objects, (0, 2, 1)), seed=seed, ctx=ctx, return_all=True)
        pred_final[np.asarray(res["cluster"], np.int64)] = out["pred"]
        res["log_probs"] = out["logp"]
    else:
        res["log_probs"] = np.zeros((0, classifier.num_class), np.float32)
    res["pred_final"] = pred_final
    return res["objects"], pred_final, res
