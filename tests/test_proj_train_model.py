"""No GPU: the training tests' torch restatement against the oracle, the config default, and the argument checks of the training ABI.

tests/proj_train_ref.forward is what tests/test_gpu_proj_train.py differentiates; here its eval form in float64 is pinned to
oracle.radad_oracle.projection_forward (itself pinned to the reference module's outputs, tests/test_oracle_golden.py) on the
projection.npz seeds.  The C entry points must refuse bad shapes, NULL buffers and a short workspace before they touch a device.
"""
import ctypes as C
import os

import numpy as np
import torch

import proj_train_ref as PR
from oracle import radad_oracle as O
from oracle import synth
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
from radad_retrievalaugmenteddeepfakeaudiodetection_amd.config import Config


def _proj_shapes(D, H=256, Oo=128):
    return {"attention_score.weight": (H, D), "attention_score.bias": (H,), "attention_final.weight": (1, H),
            "attention_final.bias": (1,), "cst_hidden.weight": (H, D), "cst_hidden.bias": (H,),
            "cst_output.weight": (D, H), "cst_output.bias": (D,), "weight_sum.weight": (H, D), "weight_sum.bias": (H,),
            "normalization.weight": (H,), "normalization.bias": (H,), "unified_embedding.weight": (Oo, H),
            "unified_embedding.bias": (Oo,)}


def test_helper_eval_form_equals_the_oracle(golden_dir):
    g = np.load(os.path.join(golden_dir, "projection.npz"))
    for D in (512, 3584):
        shapes = _proj_shapes(D)
        assert tuple(shapes) == PR.PARAM_NAMES
        sd = synth.fill_state_dict(shapes, int(g[f"proj{D}_seed"]))
        x = g[f"proj{D}_x"]
        want = O.projection_forward(x, sd)
        got = PR.forward(torch.tensor(x, dtype=torch.float64), {k: torch.tensor(v, dtype=torch.float64) for k, v in sd.items()})
        np.testing.assert_allclose(got.numpy(), want, rtol=0, atol=1e-12)


def test_helper_mask_is_inverted_dropout():
    rng = np.random.default_rng(5)
    sd = {k: rng.standard_normal(s) for k, s in _proj_shapes(12, 8, 3).items()}
    x = rng.standard_normal((4, 3, 12))
    ones = np.ones((4, 8))
    base, _ = PR.out_and_grads(x, sd, np.ones((4, 3)), torch.float64)
    same, _ = PR.out_and_grads(x, sd, np.ones((4, 3)), torch.float64, mask=ones, inv_keep=1.0)
    np.testing.assert_array_equal(base, same)
    zero, _ = PR.out_and_grads(x, sd, np.ones((4, 3)), torch.float64, mask=0 * ones, inv_keep=2.0)
    np.testing.assert_allclose(zero, np.broadcast_to(sd["unified_embedding.bias"], (4, 3)), rtol=0, atol=1e-15)


def test_config_default_keeps_training_off():
    assert Config().projection_train_hip is False


def test_train_workspace_bytes_rejects_bad_arguments():
    lib = _lib.load()
    f = lib.radad_projection_train_workspace_bytes
    assert f(4, 5, 512, 256, 128) > 0
    assert f(0, 5, 512, 256, 128) >= 0
    for bad in ((-1, 5, 512, 256, 128), (4, 0, 512, 256, 128), (4, 5, 0, 256, 128), (4, 5, 512, 0, 128), (4, 5, 512, 256, 0),
                (4, 5, 512, 4097, 128), (1 << 30, 5, 512, 256, 128), (4, 5, 1 << 22, 256, 128), (4, 5, (1 << 22) - 63, 256, 128)):
        assert f(*bad) == -1, bad
    assert f(4, 5, (1 << 22) - 64, 256, 128) > 0        # the widest row whose column sums still fit one grid


def _call_forward(lib, w, x, mask, B, K, D, H, Oo, saved, out, ws, ws_bytes):
    return lib.radad_projection_train_forward(w, x, mask, 1.0, B, K, D, H, Oo, saved, out, ws, ws_bytes, 0, None)


def _call_backward(lib, w, x, saved, g, B, K, D, H, Oo, grads, dx, ws, ws_bytes):
    return lib.radad_projection_backward(w, x, None, 1.0, saved, g, B, K, D, H, Oo, grads, dx, ws, ws_bytes, 0, None)


def test_train_abi_argument_errors_without_gpu():
    """Every refusal below returns before the first HIP call: the pointers are made-up addresses that are never dereferenced."""
    lib = _lib.load()
    fake = 0x1000
    w = _lib.ProjWeights(*([fake] * 16))
    sv = _lib.ProjSaved(*([fake] * 7))
    gr = _lib.ProjGrads(*([fake] * 14))
    B, K, D, H, Oo = 4, 5, 64, 32, 8
    need = lib.radad_projection_train_workspace_bytes(B, K, D, H, Oo)
    E = _lib.RADAD_EINVAL
    # shapes
    for shape in ((-1, K, D, H, Oo), (B, 0, D, H, Oo), (B, K, 0, H, Oo), (B, K, D, 0, Oo), (B, K, D, H, 0), (B, K, D, 4097, Oo)):
        assert _call_forward(lib, C.byref(w), fake, None, *shape, C.byref(sv), fake, fake, 1 << 40) == E, shape
        assert _call_backward(lib, C.byref(w), fake, C.byref(sv), fake, *shape, C.byref(gr), None, fake, 1 << 40) == E, shape
    assert b"bad shape" in lib.radad_last_error()
    # K * hidden beyond the LDS: refused, never launched
    assert _call_forward(lib, C.byref(w), fake, None, B, 16, D, 2048, Oo, C.byref(sv), fake, fake, 1 << 40) == E
    assert b"LDS" in lib.radad_last_error()
    assert _call_backward(lib, C.byref(w), fake, C.byref(sv), fake, B, 16, D, 2048, Oo, C.byref(gr), None, fake, 1 << 40) == E
    # batch == 0: nothing to do, no launch, no buffer needed
    assert _call_forward(lib, C.byref(w), None, None, 0, K, D, H, Oo, C.byref(sv), None, None, 0) == _lib.RADAD_OK
    assert _call_backward(lib, C.byref(w), None, C.byref(sv), None, 0, K, D, H, Oo, C.byref(gr), None, None, 0) == _lib.RADAD_OK
    # NULL structs and buffers
    assert _call_forward(lib, None, fake, None, B, K, D, H, Oo, C.byref(sv), fake, fake, need) == E
    assert _call_forward(lib, C.byref(w), fake, None, B, K, D, H, Oo, None, fake, fake, need) == E
    assert _call_forward(lib, C.byref(w), None, None, B, K, D, H, Oo, C.byref(sv), fake, fake, need) == E
    assert _call_forward(lib, C.byref(w), fake, None, B, K, D, H, Oo, C.byref(sv), None, fake, need) == E
    assert _call_forward(lib, C.byref(w), fake, None, B, K, D, H, Oo, C.byref(sv), fake, None, need) == E
    w_hole = _lib.ProjWeights(*([fake] * 16))
    w_hole.w4 = None
    assert _call_forward(lib, C.byref(w_hole), fake, None, B, K, D, H, Oo, C.byref(sv), fake, fake, need) == E
    assert b"NULL weight" in lib.radad_last_error()
    sv_hole = _lib.ProjSaved(*([fake] * 7))
    sv_hole.xh = None
    assert _call_forward(lib, C.byref(w), fake, None, B, K, D, H, Oo, C.byref(sv_hole), fake, fake, need) == E
    assert _call_backward(lib, C.byref(w), fake, C.byref(sv_hole), fake, B, K, D, H, Oo, C.byref(gr), None, fake, need) == E
    assert _call_backward(lib, C.byref(w), fake, C.byref(sv), None, B, K, D, H, Oo, C.byref(gr), None, fake, need) == E
    assert _call_backward(lib, C.byref(w), fake, C.byref(sv), fake, B, K, D, H, Oo, None, None, fake, need) == E
    gr_half = _lib.ProjGrads(*([fake] * 14))
    gr_half.dw3 = None                         # dW1 and dW3 come from one product
    assert _call_backward(lib, C.byref(w), fake, C.byref(sv), fake, B, K, D, H, Oo, C.byref(gr_half), None, fake, need) == E
    assert b"both or neither" in lib.radad_last_error()
    # a short workspace
    assert _call_forward(lib, C.byref(w), fake, None, B, K, D, H, Oo, C.byref(sv), fake, fake, need - 1) == E
    assert b"workspace too small" in lib.radad_last_error()
    assert _call_backward(lib, C.byref(w), fake, C.byref(sv), fake, B, K, D, H, Oo, C.byref(gr), None, fake, need - 1) == E
    assert b"workspace too small" in lib.radad_last_error()
