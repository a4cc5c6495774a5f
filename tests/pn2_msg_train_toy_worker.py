"""Child process of tests/test_pointnet2_msg_train.py::test_end_to_end_adam_learns_the_toy_problem: 40 steps of torch.optim.Adam on the library's
TrainerMsg (the generator's reduced MSG model) through torch_parameters() / sync(), on a context of its own that it closes before it ends.  Prints
one JSON line.

Why a process of its own: torch's wheel carries its own HIP runtime, and importing it puts a second runtime beside the one libpcr_hip.so is
linked against.  The suite's process (which keeps contexts alive until the interpreter ends) stays free of it.
"""
import importlib
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "hands-on-point-cloud-processing_amd"


def main():
    import numpy as np
    import torch
    pcr = importlib.import_module(PKG)
    pt = importlib.import_module(PKG + ".pointnet_train")
    pn = importlib.import_module(PKG + ".pointnet")
    spec = importlib.util.spec_from_file_location("gen_golden_pointnet2_msg_train", os.path.join(ROOT, "tests", "golden", "gen_golden_pointnet2_msg_train.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    x, target, cfg, state = gen.toy_inputs()
    sa = [dict(npoint=npoint, xyz_last=True, branches=[dict(radius=r, nsample=k, mlp=list(mlp)) for r, k, mlp in zip(radii, nsamples, mlps)])
          for npoint, radii, nsamples, mlps in cfg["sa"]] + [dict(group_all=True, mlp=list(cfg["sa3"]))]
    desc = pcr.pn2_msg_desc(sa, list(cfg["fc"]), bn_eps=gen.BN_EPS)
    out = {}
    ctx = pcr.Context(0)
    try:
        tr = pt.ALL_TRAINERS["pointnet2_cls_msg"].from_desc(desc, [(conv, bn) for conv, bn, _, _ in gen.layers(cfg)], dropout=cfg["p"], ctx=ctx).load_state_dict(state)
        params = tr.torch_parameters()
        out["n_params"], out["n_keys"] = len(params), len(gen.param_keys(cfg))
        out["shares_weights"] = all(p.data_ptr() == tr._view(k).ctypes.data for k, p in zip(tr.param_keys(), params))
        opt = torch.optim.Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-08, weight_decay=1e-4)
        pts, losses = np.transpose(x, (0, 2, 1)), []
        for step in range(gen.TOY_STEPS):
            opt.zero_grad()                                      # drops every .grad: torch_parameters() links them to the trainer's gradient again
            loss, _ = tr.step_grad(pts, target, seed=1000 + step)
            tr.torch_parameters()
            if step == 0:
                g = tr.grads()
                out["grad_linked"] = all(np.array_equal(p.grad.numpy(), g[k]) for k, p in zip(tr.param_keys(), params))
            opt.step()
            tr.sync()
            losses.append(float(loss))
        out["losses"] = losses
        em = tr.eval_model()
        out["eval_is_msg"] = isinstance(em, pn.get_model_msg)
        pred = em(pts, seed=3, ctx=ctx)[0].argmax(1)
        out["pred_shape"] = list(pred.shape)
        out["train_accuracy"] = float((pred == target).mean())
        out["tracked"] = int(tr.state_dict()["bn1.num_batches_tracked"])
        tr.free()
    finally:
        ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
