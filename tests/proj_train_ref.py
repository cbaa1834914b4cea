"""Plain torch restatement of ProjectionLayer's forward (projection.py:68-106) in the reference's unfolded form, for the training tests.

`forward` takes tensors of any dtype on any device and an explicit dropout mask; gradients come from torch autograd
(`out_and_grads`).  Nothing here is folded or reordered: c = W4 relu(W3 x + b3) + b4 is built as [B,K,D] and weighted by the
softmax, exactly as the reference module does, so it is an independent statement of what csrc/proj_train.inc computes.
"""
import numpy as np
import torch

PARAM_NAMES = ("attention_score.weight", "attention_score.bias", "attention_final.weight", "attention_final.bias",
               "cst_hidden.weight", "cst_hidden.bias", "cst_output.weight", "cst_output.bias", "weight_sum.weight",
               "weight_sum.bias", "normalization.weight", "normalization.bias", "unified_embedding.weight",
               "unified_embedding.bias")


def forward(x, p, mask=None, inv_keep=1.0, keep=None):
    """x [B,K,D]; p: {reference parameter name: tensor}; mask [B,H] of 0/1 or None (eval form / no dropout).
    keep: a dict that receives the softmax weights a [B,K,1] with their gradient retained."""
    lin = lambda a, n: a @ p[n + ".weight"].T + p[n + ".bias"]
    s = lin(torch.tanh(lin(x, "attention_score")), "attention_final")            # :69-71  [B,K,1]
    c = lin(torch.relu(lin(x, "cst_hidden")), "cst_output")                      # :74-76  [B,K,D]
    a = torch.softmax(s, dim=1)                                                  # :87
    if keep is not None:
        a.retain_grad()
        keep["a"] = a
    u = (a * c).sum(1)                                                           # :88-89  [B,D]
    v = lin(u, "weight_sum")                                                     # :94
    n = torch.nn.functional.layer_norm(v, (v.shape[1],), p["normalization.weight"], p["normalization.bias"], 1e-6)   # :99
    if mask is not None:
        n = n * mask * inv_keep                                                  # :100 with the mask made explicit
    return lin(n, "unified_embedding")                                           # :101


def out_and_grads(x, params, grad_out, dtype, device="cpu", mask=None, inv_keep=1.0):
    """numpy in, float64 numpy out: (out, {"x": dx, name: d name ..., "_a": a, "_da": d a [B,K,1]}) of sum(out * grad_out) by
    torch autograd in `dtype`."""
    xt = torch.tensor(np.asarray(x), dtype=dtype, device=device, requires_grad=True)
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, device=device, requires_grad=True) for k, v in params.items()}
    m = None if mask is None else torch.tensor(np.asarray(mask), dtype=dtype, device=device)
    keep = {}
    out = forward(xt, p, m, inv_keep, keep)
    out.backward(torch.tensor(np.asarray(grad_out), dtype=dtype, device=device))
    grads = {"x": xt.grad.double().cpu().numpy(), "_a": keep["a"].detach().double().cpu().numpy(),
             "_da": keep["a"].grad.double().cpu().numpy()}
    grads.update({k: v.grad.double().cpu().numpy() for k, v in p.items()})
    return out.detach().double().cpu().numpy(), grads
