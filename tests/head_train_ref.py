"""Plain torch restatement of RADADModel's tail (fuse Linear + detection MLP) in training mode, for the head-training tests.

Written against the formulae of the feature (include/radad_hip.h, "RADADModel after the projection in training mode"), with
BatchNorm spelled out -- batch mean, biased variance as the mean of squared deviations from that mean, the unbiased factor
B / (B - 1) in the running variance -- and the concatenation [tpp | proj] built, as the reference module does.  Any dtype, any
device, caller-supplied dropout masks; gradients come from torch autograd (`out_and_grads`).

Parameter names: fuse.weight [P, D+P], fuse.bias, lin{i}.weight / lin{i}.bias per Linear layer i (the last one is the output
layer), bn{i}.weight / bn{i}.bias per hidden layer that has a BatchNorm.
"""
import numpy as np
import torch


def n_layers(p):
    return sum(1 for k in p if k.startswith("lin") and k.endswith(".weight"))


def param_names(p):
    """The order _FuseHeadTrainFn.apply takes the parameters in."""
    names = ["fuse.weight", "fuse.bias"]
    n = n_layers(p)
    for i in range(n):
        names += [f"lin{i}.weight", f"lin{i}.bias"]
        if i + 1 < n and f"bn{i}.weight" in p:
            names += [f"bn{i}.weight", f"bn{i}.bias"]
    return names


def forward(tpp, proj, p, masks=None, inv_keep=1.0, eps=1e-5, running=None, factor=None, train=True):
    """tpp [B,D], proj [B,P]; p: {name: tensor}; masks: per hidden layer a [B,d] tensor of 0/1 or None.
    running: per hidden layer (mean, var) or None; train=True normalises with the batch statistics and returns the updated
    running statistics (factor[i] per layer), train=False normalises with `running` (the eval form, no dropout).
    Returns (logits [B, d_out], new_running)."""
    n = n_layers(p)
    a = torch.cat([tpp, proj], dim=1) @ p["fuse.weight"].T + p["fuse.bias"]
    new_running = []
    for i in range(n):
        z = a @ p[f"lin{i}.weight"].T + p[f"lin{i}.bias"]
        if i + 1 == n:
            return z, new_running
        if f"bn{i}.weight" in p:
            if train:
                B = z.shape[0]
                mean = z.sum(0) / B
                var = ((z - mean) ** 2).sum(0) / B
                if running is not None and running[i] is not None:
                    f = factor[i]
                    new_running.append(((1 - f) * running[i][0] + f * mean.detach(), (1 - f) * running[i][1] + f * var.detach() * B / (B - 1)))
                else:
                    new_running.append(None)
            else:
                mean, var = running[i]
                new_running.append(running[i])
            z = (z - mean) / torch.sqrt(var + eps) * p[f"bn{i}.weight"] + p[f"bn{i}.bias"]
        else:
            new_running.append(None)
        a = torch.relu(z)
        if train and masks is not None and masks[i] is not None:
            a = a * masks[i] * inv_keep


def out_and_grads(tpp, proj, params, grad_out, dtype, device="cpu", masks=None, inv_keep=1.0, eps=1e-5, running=None, factor=None):
    """numpy in, float64 numpy out: (logits, {"tpp": dtpp, "proj": dproj, name: d name}, new running statistics) of
    sum(logits * grad_out) by torch autograd in `dtype`."""
    tt = lambda v, g=False: torch.tensor(np.asarray(v), dtype=dtype, device=device, requires_grad=g)
    t, pr = tt(tpp, True), tt(proj, True)
    p = {k: tt(v, True) for k, v in params.items()}
    m = None if masks is None else [None if x is None else tt(x) for x in masks]
    run = None if running is None else [None if r is None else (tt(r[0]), tt(r[1])) for r in running]
    logits, new_run = forward(t, pr, p, m, inv_keep, eps, run, factor)
    logits.backward(tt(grad_out))
    back = lambda v: v.detach().double().cpu().numpy()
    grads = {"tpp": back(t.grad), "proj": back(pr.grad)}
    grads.update({k: back(v.grad) for k, v in p.items()})
    return back(logits), grads, [None if r is None else (back(r[0]), back(r[1])) for r in new_run]


def params_of(fuse, detection_model):
    """{helper name: tensor} of an nn.Linear `fuse` and a DetectionModel, and the BatchNorm modules per hidden layer (or None)."""
    p = {"fuse.weight": fuse.weight, "fuse.bias": fuse.bias}
    bns = []
    layers = detection_model.head_layers()
    for i, (lin, bn) in enumerate(layers):
        p[f"lin{i}.weight"], p[f"lin{i}.bias"] = lin.weight, lin.bias
        if i + 1 < len(layers):
            bns.append(bn)
            if bn is not None:
                p[f"bn{i}.weight"], p[f"bn{i}.bias"] = bn.weight, bn.bias
    return p, bns
