"""Writes tests/golden/pointnet_cls_ref.npz: what the reference's own vanilla PointNet classifier (models/pointnet_cls.py with the T-Nets of
models/pointnet.py) returns, in eval mode, for the 64 objects of gen_golden_pointnet.derive_inputs and for weights DRAWN BY RULE (make_state
below, the rule of gen_golden_pointnet2.make_state on this model's keys: the tests rebuild them, so the fixture holds reference OUTPUTS only,
plus the floats of fc3.bias that the rule centres on the mean f64 logit).

Runs on a CPU (torch + numpy):   python tests/golden/gen_golden_pointnet_cls.py <reference root>
  <reference root>/HomeworkFinal/models/pointnet_cls.py, pointnet.py     imported as they are

Two models: get_model(4, normal_channel=False) on all 64 objects, and get_model(4, normal_channel=True) on the first 8 with unit normals drawn
by a seeded rule (normals below).  Each runs in f32 and as model.double().

Asserted for both (if one fails: change the weight seed, not the cap): at least two classes predicted; every object's f64 top-two margin above
1e-3; global_feat has entries below -0.1 (the encoder ends without a ReLU: the max over points is a SIGNED max); the file at most 512 KB.

Recorded (suffix 6 = the normal_channel model): fc3_bias; logp f32 and f64 of every object; trans f64 of every object; global_feat f32 and f64
of the first N_GF; trans_feat f64 of the first N_TF (f64 trans_feat of all 64 objects would be 2 MB); e_*: the f32 pass's largest deviation
from each f64 tensor; the names and shapes of the reference model's state_dict() entries.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pointnet_cls_ref.npz")
_spec = importlib.util.spec_from_file_location("gen_golden_pointnet", os.path.join(HERE, "gen_golden_pointnet.py"))
base = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(base)

NUM_CLASS, WEIGHT_SEED, NORMAL_SEED = 4, 2027, 77
N_OBJ6, N_GF, N_TF, N_GF6, N_TF6 = 8, 8, 4, 4, 1
MAX_BYTES = 512 * 1024
ENC = (64, 128, 1024)                      # feat.conv1 ... conv3
TNET_CONV, TNET_FC = (64, 128, 1024), (512, 256)
HEAD = (512, 256)
BN_KEYS = ("weight", "bias", "running_mean", "running_var")
BN_EPS = 1e-5
TNET_FC3_SCALE = 1.0 / 32                  # a T-Net's last layer: the transforms stay near the identity, as trained ones do (unscaled, the global feature reaches 5e3)


def tnet_layers(prefix, cin, k):
    out = []
    for i, w in enumerate(TNET_CONV):
        out.append((f"{prefix}.conv{i + 1}", f"{prefix}.bn{i + 1}", w, cin))
        cin = w
    for i, w in enumerate(TNET_FC):
        out.append((f"{prefix}.fc{i + 1}", f"{prefix}.bn{len(TNET_CONV) + i + 1}", w, cin))
        cin = w
    out.append((f"{prefix}.fc{len(TNET_FC) + 1}", None, k * k, cin))
    return out


def layers(num_class=NUM_CLASS, channel=3):
    """(conv / linear prefix, BN prefix or None, out, in) in weight order: feat.stn, the feat convolutions, feat.fstn, the head"""
    out = tnet_layers("feat.stn", channel, 3)
    cin = channel
    for i, w in enumerate(ENC):
        out.append((f"feat.conv{i + 1}", f"feat.bn{i + 1}", w, cin))
        cin = w
    out += tnet_layers("feat.fstn", ENC[0], ENC[0])
    for i, w in enumerate(HEAD):
        out.append((f"fc{i + 1}", f"bn{i + 1}", w, cin))
        cin = w
    out.append((f"fc{len(HEAD) + 1}", None, num_class, cin))
    return out


def make_state(seed=WEIGHT_SEED, num_class=NUM_CLASS, channel=3, fc3_bias=None):
    """the weights by the rule of gen_golden_pointnet2.make_state, as a state dict of f32 numpy arrays with the reference's key names (Conv1d
    weights [out, in, 1]); the last layer of both T-Nets is scaled by TNET_FC3_SCALE"""
    rng = np.random.default_rng(seed)
    st = {}
    for conv, bn, w, cin in layers(num_class, channel):
        scale = np.float32(TNET_FC3_SCALE if conv.endswith("stn.fc3") else 1.0)
        W = (rng.standard_normal((w, cin)) * np.sqrt(2.0 / cin)).astype(np.float32) * scale
        st[f"{conv}.weight"] = W.reshape(w, cin, 1) if ".conv" in conv else W
        st[f"{conv}.bias"] = (0.1 * rng.standard_normal(w)).astype(np.float32) * scale
        if bn:
            st[f"{bn}.weight"] = rng.uniform(0.8, 1.2, w).astype(np.float32)
            st[f"{bn}.bias"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
            st[f"{bn}.running_mean"] = (0.1 * rng.standard_normal(w)).astype(np.float32)
            st[f"{bn}.running_var"] = rng.uniform(0.5, 1.5, w).astype(np.float32)
    if fc3_bias is not None:
        st["fc3.bias"] = np.asarray(fc3_bias, np.float32).reshape(num_class)
    return st


def normals(n_obj=N_OBJ6, npts=256, seed=NORMAL_SEED):
    """unit normals by rule: a seeded Gaussian direction per point, normalised in f64, rounded to f32 -> [n_obj, npts, 3]"""
    v = np.random.default_rng(seed).standard_normal((n_obj, npts, 3))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def inputs6(objs):
    """the input of the normal_channel model: the first N_OBJ6 objects with their normals -> [N_OBJ6, 256, 6]"""
    return np.concatenate([objs[:N_OBJ6], normals(N_OBJ6, objs.shape[1])], -1).astype(np.float32)


def main(ref_root):
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    sys.path.insert(0, os.path.join(ref_root, "HomeworkFinal"))
    from models.pointnet_cls import get_model
    objs = base.derive_inputs(base.load_scan())["objs"]
    names = {}

    def run(state, x, normal_channel, double):
        model = get_model(NUM_CLASS, normal_channel=normal_channel).eval()
        names[normal_channel] = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()}, strict=False)
        if double:
            model = model.double()
        got = {}
        hooks = [model.feat.register_forward_hook(lambda m, i, o: got.update(gf=o[0], trans=o[1], tf=o[2])),
                 model.fc3.register_forward_hook(lambda m, i, o: got.__setitem__("logits", o))]
        t = torch.from_numpy(x).transpose(2, 1).contiguous()
        with torch.no_grad():
            logp, tf = model(t.double() if double else t)
        for h in hooks:
            h.remove()
        return {"logp": logp.numpy(), "gf": got["gf"].numpy(), "trans": got["trans"].numpy(), "tf": tf.numpy(), "logits": got["logits"].numpy()}

    out = {}
    for nc, x, sfx, n_gf, n_tf in ((False, objs, "", N_GF, N_TF), (True, inputs6(objs), "6", N_GF6, N_TF6)):
        ch = 6 if nc else 3
        state = make_state(channel=ch, fc3_bias=np.zeros(NUM_CLASS))
        fc3_bias = (-run(state, x, nc, True)["logits"].mean(0)).astype(np.float32)
        state = make_state(channel=ch, fc3_bias=fc3_bias)
        r32, r64 = run(state, x, nc, False), run(state, x, nc, True)
        pred = r64["logp"].argmax(1)
        top = np.sort(r64["logp"], 1)
        margin = float((top[:, -1] - top[:, -2]).min())
        assert len(set(pred.tolist())) >= 2, "the weight rule predicts one class only"
        assert margin > 1e-3, f"top-two margin {margin}"
        assert (r32["logp"].argmax(1) == pred).all()
        assert float(r64["gf"].min()) < -0.1, "the global feature has no negative entry: the signed max is not exercised"
        keep = {"logp": len(x), "trans": len(x), "gf": n_gf, "tf": n_tf}
        out[f"fc3_bias{sfx}"] = fc3_bias
        out[f"logp_f32{sfx}"] = r32["logp"]
        out[f"gf_f32{sfx}"] = r32["gf"][:n_gf]
        for k, n in keep.items():
            out[f"{k}_f64{sfx}"] = r64[k][:n]
            out[f"e_{k}{sfx}"] = np.float64(np.abs(r32[k][:n].astype(np.float64) - r64[k][:n]).max())
        ks = sorted(names[nc])
        out[f"state_names{sfx}"] = np.array(ks)
        out[f"state_shapes{sfx}"] = np.array([",".join(str(v) for v in names[nc][k]) for k in ks])
        print("normal_channel", nc, "classes", np.bincount(pred, minlength=NUM_CLASS).tolist(), "margin", margin, "global_feat min", float(r64["gf"].min()),
              "max", float(r64["gf"].max()))
    base._write_npz(OUT, out)
    size = os.path.getsize(OUT)
    assert size <= MAX_BYTES, f"{size} bytes: shrink the recorded slices"
    print(OUT, size, "bytes;", {k: float(v) for k, v in out.items() if k.startswith("e_")})


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PCR_REFERENCE_ROOT", ""))
