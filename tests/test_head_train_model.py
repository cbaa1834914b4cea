"""No GPU: the head-training tests' torch restatement against torch's own modules and the oracle, the config default, and the
argument checks of the head-training ABI.

tests/head_train_ref.forward is what tests/test_gpu_head_train.py differentiates.  Here, in float64, it is pinned to copies of
nn.Linear + DetectionModel.model in .train() under autograd (logits, every gradient, the running statistics after the step), and
its eval form to oracle.radad_oracle.radad_model_forward's tail on the projection.npz seeds.  The C entry points must refuse bad
shapes, NULL buffers, half-given pairs and a short workspace before they touch a device.
"""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import head_train_ref as HR
from oracle import radad_oracle as O
from oracle import synth
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
from radad_retrievalaugmenteddeepfakeaudiodetection_amd.config import Config
from radad_retrievalaugmenteddeepfakeaudiodetection_amd.radad_model import DetectionModel


def _modules(D, P, hidden, batch_norm=True, momentum=0.1, seed=3):
    cfg = Config()
    cfg.update(device=torch.device("cpu"), detection_hidden_dims=hidden, detection_dropout=0.0, use_batch_norm=batch_norm)
    torch.manual_seed(seed)
    fuse = torch.nn.Linear(D + P, P).double()
    head = DetectionModel(cfg, P).double().train()
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, torch.nn.Linear):
                m.bias.normal_(0, 0.3)
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.normal_(1, 0.1)
                m.bias.normal_(0, 0.1)
                m.running_mean.normal_(0, 0.5)
                m.running_var.uniform_(0.5, 2.0)
                m.momentum = momentum
    return fuse, head


@pytest.mark.parametrize("hidden,batch_norm,momentum", [([10, 6], True, 0.1), ([10, 6], True, None), ([7], False, 0.1), ([], True, 0.1)],
                         ids=["bn", "bn_momentum_none", "no_bn", "output_only"])
def test_helper_equals_torch_modules_in_float64(hidden, batch_norm, momentum):
    B, D, P = 9, 11, 5
    fuse, head = _modules(D, P, hidden, batch_norm, momentum)
    rng = np.random.default_rng(8)
    for step in range(2):                                   # two consecutive batches: momentum=None averages over both
        fuse.zero_grad()
        head.zero_grad()
        tpp, proj, g = rng.standard_normal((B, D)), rng.standard_normal((B, P)), rng.standard_normal((B, 1))
        p, bns = HR.params_of(fuse, head)
        params = {k: v.detach().numpy().copy() for k, v in p.items()}
        running = [None if bn is None else (bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()) for bn in bns]
        factor = [None if bn is None else (bn.momentum if bn.momentum is not None else 1.0 / (int(bn.num_batches_tracked) + 1))
                  for bn in bns]
        masks = [np.ones((B, d)) for d in hidden]
        logits, grads, new_run = HR.out_and_grads(tpp, proj, params, g, torch.float64, masks=masks, running=running, factor=factor)
        t = torch.tensor(tpp, requires_grad=True)
        pr = torch.tensor(proj, requires_grad=True)
        want = head.model(fuse(torch.cat([t, pr], 1)))
        want.backward(torch.tensor(g))
        close = dict(rtol=0, atol=1e-12)
        np.testing.assert_allclose(logits, want.detach().numpy(), **close)
        np.testing.assert_allclose(grads["tpp"], t.grad.numpy(), **close)
        np.testing.assert_allclose(grads["proj"], pr.grad.numpy(), **close)
        for k, v in p.items():
            np.testing.assert_allclose(grads[k], v.grad.numpy(), err_msg=k, **close)
        for bn, r in zip(bns, new_run):
            if bn is not None:
                assert int(bn.num_batches_tracked) == step + 1
                np.testing.assert_allclose(r[0], bn.running_mean.numpy(), **close)
                np.testing.assert_allclose(r[1], bn.running_var.numpy(), **close)


def test_helper_eval_form_equals_the_oracle(golden_dir):
    g = np.load(os.path.join(golden_dir, "projection.npz"))
    names = [str(n) for n in g["radad_names"]]
    shapes = {n: tuple(int(v) for v in str(s).split(",") if v) for n, s in zip(names, g["radad_shapes"])}
    sd = synth.fill_state_dict(shapes, int(g["radad_seed"]))
    proj, fused, want = O.radad_model_forward(g["radad_x"], g["radad_t"], sd)
    t64 = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64)
    lin = sorted(int(k.split(".")[2]) for k in sd if k.startswith("detection_model.model.") and np.ndim(sd[k]) == 2)
    p = {"fuse.weight": t64(sd["fuse.weight"]), "fuse.bias": t64(sd["fuse.bias"])}
    running = []
    for i, idx in enumerate(lin):
        p[f"lin{i}.weight"], p[f"lin{i}.bias"] = t64(sd[f"detection_model.model.{idx}.weight"]), t64(sd[f"detection_model.model.{idx}.bias"])
        if i + 1 < len(lin):
            b = f"detection_model.model.{idx + 1}."
            p[f"bn{i}.weight"], p[f"bn{i}.bias"] = t64(sd[b + "weight"]), t64(sd[b + "bias"])
            running.append((t64(sd[b + "running_mean"]), t64(sd[b + "running_var"])))
    assert len(lin) == 3 and len(running) == 2
    got, _ = HR.forward(t64(g["radad_t"]), t64(proj), p, running=running, train=False)
    np.testing.assert_allclose(got.squeeze(-1).numpy(), want, rtol=0, atol=1e-12)


def test_config_default_keeps_head_training_off():
    assert Config().head_train_hip is False


def _dims(*d):
    return (C.c_int32 * len(d))(*d)


def test_head_train_workspace_bytes_rejects_bad_arguments():
    lib = _lib.load()
    f = lib.radad_fuse_head_train_workspace_bytes
    assert f(256, 5376, 128, 3, _dims(128, 64, 32, 1)) > 0
    assert f(0, 512, 128, 3, _dims(128, 64, 32, 1)) >= 0
    assert f(2, 8, 1, 2, _dims(1, 1, 1)) > 0
    assert f(3, 5, 3, 1, _dims(3, 1)) > 0
    assert f(37, 64, 16, 6, _dims(16, 8, 8, 8, 8, 8, 1)) > 0
    assert f(4, 64, 8192, 2, _dims(8192, 8192, 1)) > 0
    for bad in ((-1, 512, 128, 2, _dims(128, 64, 1)), (4, 0, 128, 2, _dims(128, 64, 1)), (4, 512, 0, 2, _dims(0, 64, 1)),
                (4, 512, 128, 0, _dims(128)), (4, 512, 128, 7, _dims(128, 8, 8, 8, 8, 8, 8, 1)),
                (4, 512, 128, 2, _dims(64, 64, 1)), (4, 512, 128, 2, _dims(128, 0, 1)), (4, 512, 128, 2, _dims(128, 8193, 1)),
                (4, 512, 8193, 2, _dims(8193, 64, 1)), ((1 << 31) - 128, 512, 128, 2, _dims(128, 64, 1)),
                (4, 1 << 22, 128, 2, _dims(128, 64, 1)), (4, 512, 128, 2, None)):
        assert f(*bad) == -1, bad[:4]


def _structs(n_layers=3, dims=(16, 8, 4, 1), fake=0x1000):
    w, sv, gr = _lib.HeadTrainWeights(), _lib.HeadSaved(), _lib.HeadGrads()
    w.wf, w.bf, w.n_layers = fake, fake, n_layers
    sv.fused = fake
    gr.dwf, gr.dbf = fake, fake
    for i, d in enumerate(dims):
        w.dims[i] = d
    for l in range(n_layers):
        w.lw[l], w.lb[l] = fake, fake
        gr.dlw[l], gr.dlb[l] = fake, fake
        if l + 1 < n_layers:
            w.bn_gamma[l], w.bn_beta[l], w.bn_running_mean[l], w.bn_running_var[l] = fake, fake, fake, fake
            w.bn_eps[l], w.bn_factor[l] = 1e-5, 0.1
            sv.xh[l], sv.rstd[l], sv.act[l] = fake, fake, fake
            gr.dgamma[l], gr.dbeta[l] = fake, fake
    return w, sv, gr


def test_head_train_abi_argument_errors_without_gpu():
    """Every refusal below returns before the first HIP call: the pointers are made-up addresses that are never dereferenced."""
    lib = _lib.load()
    fake = 0x1000
    E, OK = _lib.RADAD_EINVAL, _lib.RADAD_OK
    B, D, P = 4, 64, 16
    need = lib.radad_fuse_head_train_workspace_bytes(B, D, P, 3, _dims(16, 8, 4, 1))
    assert need > 0

    def fwd(w, sv, tpp=fake, proj=fake, batch=B, dim=D, proj_dim=P, logits=fake, ws=fake, ws_bytes=1 << 40):
        return lib.radad_fuse_head_train_forward(None if w is None else C.byref(w), tpp, proj, None, 1.0, batch, dim, proj_dim,
                                                 None if sv is None else C.byref(sv), logits, ws, ws_bytes, 0, None)

    def bwd(w, sv, gr, tpp=fake, proj=fake, g=fake, batch=B, dim=D, proj_dim=P, ws=fake, ws_bytes=1 << 40):
        return lib.radad_fuse_head_backward(None if w is None else C.byref(w), tpp, proj, None, 1.0, None if sv is None else C.byref(sv),
                                            g, batch, dim, proj_dim, None if gr is None else C.byref(gr), None, fake, ws, ws_bytes, 0,
                                            None)

    def both(w, sv, gr, needle, **kw):
        assert fwd(w, sv, **kw) == E, needle
        assert needle in lib.radad_last_error(), lib.radad_last_error()
        assert bwd(w, sv, gr, **kw) == E, needle
        assert needle in lib.radad_last_error(), lib.radad_last_error()

    w, sv, gr = _structs()
    # n_layers outside 1..RADAD_HEAD_MAX_LAYERS
    for n in (0, 7, -1):
        w.n_layers = n
        both(w, sv, gr, b"n_layers")
    w, sv, gr = _structs()
    # a width above 8192, a width of zero, dims[0] != proj_dim, a bad batch or dim
    w.dims[1] = 8193
    both(w, sv, gr, b"bad shape")
    w.dims[1] = 0
    both(w, sv, gr, b"bad shape")
    w, sv, gr = _structs()
    both(w, sv, gr, b"proj_dim", proj_dim=8)
    both(w, sv, gr, b"bad shape", batch=(1 << 31) - 128)
    both(w, sv, gr, b"bad shape", batch=-1)
    both(w, sv, gr, b"bad shape", dim=0)
    # batch == 1 with a BatchNorm layer: refused, and the message names the layer
    both(w, sv, gr, b"layer 0: BatchNorm", batch=1)
    w.bn_gamma[0] = w.bn_beta[0] = None
    both(w, sv, gr, b"layer 1: BatchNorm", batch=1)
    w.bn_gamma[1] = w.bn_beta[1] = None
    w.bn_running_mean[0] = w.bn_running_var[0] = w.bn_running_mean[1] = w.bn_running_var[1] = None
    assert fwd(w, sv, batch=1, ws_bytes=0) == E and b"workspace too small" in lib.radad_last_error()   # no BatchNorm left: B = 1 is legal
    # batch == 0: nothing to do, no launch, no buffer needed
    w, sv, gr = _structs()
    assert fwd(w, sv, tpp=None, proj=None, batch=0, logits=None, ws=None, ws_bytes=0) == OK
    assert bwd(w, sv, gr, tpp=None, proj=None, g=None, batch=0, ws=None, ws_bytes=0) == OK
    # NULL structs and buffers
    assert fwd(None, sv) == E and fwd(w, None) == E
    assert bwd(None, sv, gr) == E and bwd(w, None, gr) == E and bwd(w, sv, None) == E
    for kw in (dict(tpp=None), dict(proj=None), dict(ws=None)):
        both(w, sv, gr, b"NULL buffer", **kw)
    assert fwd(w, sv, logits=None) == E and b"NULL buffer" in lib.radad_last_error()
    assert bwd(w, sv, gr, g=None) == E and b"NULL buffer" in lib.radad_last_error()
    # NULL weights
    w.wf = None
    both(w, sv, gr, b"NULL weight")
    w, sv, gr = _structs()
    w.lw[2] = None
    both(w, sv, gr, b"NULL weight")
    w, sv, gr = _structs()
    w.lb[1] = None
    assert fwd(w, sv) == E and b"NULL weight" in lib.radad_last_error()
    # NULL saved arrays
    for hole in ("fused", "xh", "rstd", "act"):
        w, sv, gr = _structs()
        if hole == "fused":
            sv.fused = None
        else:
            getattr(sv, hole)[1] = None
        both(w, sv, gr, b"NULL saved-activation buffer")
    # half-given pairs
    w, sv, gr = _structs()
    w.bn_beta[0] = None
    both(w, sv, gr, b"half NULL")
    w, sv, gr = _structs()
    w.bn_running_var[1] = None
    both(w, sv, gr, b"half NULL")
    # a short workspace
    w, sv, gr = _structs()
    both(w, sv, gr, b"workspace too small", ws_bytes=need - 1)
