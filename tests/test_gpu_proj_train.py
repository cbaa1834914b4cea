"""GPU: ProjectionLayer / RADADModel training forward and backward (csrc/proj_train.inc) against float64 autograd.

Accuracy measure, for `out` and each of the 15 gradients (dx and the 14 parameters):
    err = max|got - f64| / max|f64|        f64 = tests/proj_train_ref.py in float64 on the CPU
and the HIP path's err may be at most FACTOR = 4 times the err of torch's own float32 autograd of the same helper on the same
device and input (allow_tf32 off).  The factor allows for a different summation order (sum_K before W4, split-order partial
sums), not for more roundings per term.  Where torch's float32 result happens to be exact (err 0), the largest torch-float32
err over the gradient-parity cases of this file (plain random data) stands in as the floor.  Where float64 itself says a
gradient is exactly zero, the HIP gradient must be exactly zero.  Nothing is ever bounded against the HIP result itself.  Every
measured pair is printed (run with -s to see them); profiles/proj_train.md keeps one run's figures.

One gradient is zero in exact arithmetic for every input: db2 = sum ds (the softmax does not see a shift of all scores), so
float64 leaves 1e-16 of noise there and float32 1e-7, and a ratio of two noises measures nothing.  What a float32 evaluation of
that sum leaves is measured instead, in absolute terms: |db2| <= 4 max(|db2 of torch float32|, floor sum|ds|) -- torch's own
residue, or (where that happens to be exactly zero) the file's floor as the relative error of a sum whose terms add up to
sum|ds| in magnitude, ds from float64 autograd.  The bound does not grow with the number of rows, and one dropped row (|ds| is of
order 1) stands far above it.

Every test here fails without the feature with "inference-only" (or, below the module level, for want of the autograd function).
"""
import numpy as np
import pytest

import proj_train_ref as PR

pytestmark = pytest.mark.gpu

FACTOR = 4.0
NOISE = ("attention_final.bias", "_a", "_da")  # db2 is zero in exact arithmetic (module docstring); _a, _da are the helper's taps


def _params(D, H, Oo, seed, bias=0.3):
    """nn.Linear weights ~ N(0, 1/fan_in), biases ~ N(0, bias^2), LayerNorm gain 1 + N(0, 0.01)."""
    rng = np.random.default_rng(seed)
    w = lambda o, i: (rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
    b = lambda n, s=bias: (s * rng.standard_normal(n)).astype(np.float32)
    return {"attention_score.weight": w(H, D), "attention_score.bias": b(H), "attention_final.weight": w(1, H),
            "attention_final.bias": b(1), "cst_hidden.weight": w(H, D), "cst_hidden.bias": b(H), "cst_output.weight": w(D, H),
            "cst_output.bias": b(D), "weight_sum.weight": w(H, D), "weight_sum.bias": b(H),
            "normalization.weight": (1 + b(H, 0.1)).astype(np.float32), "normalization.bias": b(H, 0.1),
            "unified_embedding.weight": w(Oo, H), "unified_embedding.bias": b(Oo)}


def _plain(B, K, D, H, Oo, seed):
    rng = np.random.default_rng(seed + 1000)
    return {"x": rng.standard_normal((B, K, D)).astype(np.float32), "p": _params(D, H, Oo, seed),
            "g": rng.standard_normal((B, Oo)).astype(np.float32), "mask": None, "inv_keep": 1.0}


PARITY = [(1, 1, 8, 8, 1), (3, 5, 44, 24, 10), (37, 5, 130, 96, 24), (130, 1, 64, 128, 128), (9, 7, 447, 256, 128),
          (8, 5, 5376, 256, 128), (300, 5, 512, 256, 128)]
DESIGN_SHAPE = (6, 5, 44, 24, 10)


def _relu_ties():
    c = _plain(*DESIGN_SHAPE, seed=21)
    c["p"]["cst_hidden.bias"][:] = 0          # b3 = 0 and all-zero neighbour rows (what retrieval returns for id -1): q = 0 exactly
    c["x"][0, 1:] = 0
    c["x"][2, 4] = 0
    c["x"][5] = 0
    return c


def _saturated_tanh():
    c = _plain(*DESIGN_SHAPE, seed=22)
    c["x"][1] *= 50
    c["x"][3, 2] *= 50
    return c


def _spread_scores():
    c = _plain(*DESIGN_SHAPE, seed=23)
    c["p"]["attention_final.weight"] *= 150   # W2 tanh(.) spreads over +-80 and more: the softmax saturates
    c["p"]["attention_final.bias"][:] = 80
    return c


def _identical_neighbours():
    c = _plain(*DESIGN_SHAPE, seed=24)
    c["x"][:] = c["x"][:, :1]
    return c


def _dropout_half():
    c = _plain(37, 5, 130, 96, 24, seed=25)
    c["mask"] = (np.random.default_rng(99).random((37, 96)) < 0.5).astype(np.float32)
    c["inv_keep"] = 2.0
    return c


BUILDERS = {f"parity{i}": (lambda s=s, i=i: _plain(*s, seed=i)) for i, s in enumerate(PARITY)}
BUILDERS.update(relu_ties=_relu_ties, saturated_tanh=_saturated_tanh, spread_scores=_spread_scores,
                identical_neighbours=_identical_neighbours, dropout_half=_dropout_half)


def _rel(got, want):
    scale = float(np.abs(want).max())
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / (scale if scale > 0 else 1.0)


@pytest.fixture(scope="module")
def refs(gpu):
    """Per accuracy case: the inputs, float64 (out, grads) on the CPU, torch float32 errs on the device; and the file's floor."""
    import torch
    was = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    out = {}
    for name, build in BUILDERS.items():
        c = build()
        o64, g64 = PR.out_and_grads(c["x"], c["p"], c["g"], torch.float64, "cpu", c["mask"], c["inv_keep"])
        o32, g32 = PR.out_and_grads(c["x"], c["p"], c["g"], torch.float32, gpu, c["mask"], c["inv_keep"])
        t32 = {"out": _rel(o32, o64)}
        t32.update({k: _rel(g32[k], g64[k]) for k in g64})
        a, da = g64["_a"], g64["_da"]
        ds = a * (da - (a * da).sum(axis=1, keepdims=True))
        out[name] = dict(c, out64=o64, g64=g64, t32=t32, ds_abs=float(np.abs(ds).sum()),
                         db2_t32=float(np.abs(g32["attention_final.bias"]).max()))
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = was
    floor = max(v for name, r in out.items() if name.startswith("parity") for k, v in r["t32"].items() if k not in NOISE)
    assert 0 < floor < 1e-4, f"torch float32 autograd is off by {floor}: the reference itself is broken"
    for r in out.values():
        r["db2_bound"] = FACTOR * max(r["db2_t32"], floor * r["ds_abs"])
    return out, floor


def _hip(gpu, c, x_grad=True, frozen=()):
    """(out, {"x": dx, name: grad}) of the HIP autograd function on case c's inputs, as numpy; also the raw torch tensors."""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.projection import _ProjectionTrainFn
    x = torch.tensor(c["x"], device=gpu, requires_grad=x_grad)
    p = {k: torch.tensor(c["p"][k], device=gpu, requires_grad=k not in frozen) for k in PR.PARAM_NAMES}
    mask = None if c["mask"] is None else torch.tensor(c["mask"], device=gpu)
    out = _ProjectionTrainFn.apply(x, mask, c["inv_keep"], *[p[k] for k in PR.PARAM_NAMES])
    out.backward(torch.tensor(c["g"], device=gpu))
    grads = {"x": x.grad}
    grads.update({k: v.grad for k, v in p.items()})
    return out.detach().cpu().numpy(), {k: (None if v is None else v.cpu().numpy()) for k, v in grads.items()}


def _check_case(name, r, floor, out, grads):
    bad = []
    for key in ["out", "x"] + list(PR.PARAM_NAMES):
        got = out if key == "out" else grads[key]
        want = r["out64"] if key == "out" else r["g64"][key]
        assert got.shape == want.shape, f"{name} {key}: shape {got.shape} != {want.shape}"
        assert np.isfinite(got).all(), f"{name} {key}: not finite"
        e_hip, e_t32 = _rel(got, want), r["t32"][key]
        bound = FACTOR * (e_t32 if e_t32 > 0 else floor)
        if key == "attention_final.bias":
            print(f"proj_train {name:22s} {key:26s} |hip| {np.abs(got).max():.3e}  |torch32| {r['db2_t32']:.3e}  bound {r['db2_bound']:.3e}")
        else:
            print(f"proj_train {name:22s} {key:26s} hip {e_hip:.3e}  torch32 {e_t32:.3e}  bound {bound:.3e}")
        if key == "attention_final.bias":
            if not np.abs(got).max() <= r["db2_bound"]:
                bad.append(f"{key}: |db2| {np.abs(got).max():.3e} above {FACTOR} x max(torch float32's {r['db2_t32']:.3e}, floor x sum|ds|) = {r['db2_bound']:.3e}")
        elif not np.abs(want).max() > 0:
            if np.abs(got).max() != 0:
                bad.append(f"{key}: float64 says exactly zero, HIP gives up to {np.abs(got).max():.3e}")
        elif not e_hip <= bound:
            bad.append(f"{key}: err {e_hip:.3e} > {FACTOR} x torch float32 err {e_t32:.3e}")
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("i", range(len(PARITY)), ids=["x".join(map(str, s)) for s in PARITY])
def test_gradient_parity(gpu, refs, i):
    cases, floor = refs
    name = f"parity{i}"
    out, grads = _hip(gpu, cases[name])
    _check_case(name, cases[name], floor, out, grads)
    if PARITY[i][1] == 1:      # softmax of one neighbour: ds = 0, nothing reaches the score branch
        for k in ("attention_score.weight", "attention_score.bias", "attention_final.weight", "attention_final.bias"):
            assert not grads[k].any(), f"{name} {k}: must be exactly zero with one neighbour"


@pytest.mark.parametrize("name", ["relu_ties", "saturated_tanh", "spread_scores", "identical_neighbours", "dropout_half"])
def test_designed_inputs(gpu, refs, name):
    cases, floor = refs
    r = cases[name]
    if name == "relu_ties":        # the input really ties: some pre-activations of the relu branch are exactly zero
        q = r["x"].astype(np.float64) @ r["p"]["cst_hidden.weight"].astype(np.float64).T
        assert (q == 0).sum() >= 10 * DESIGN_SHAPE[3]
    if name == "spread_scores":    # some row's scores really are +-80 apart, far up the exponential (b2 = 80)
        s = np.tanh(r["x"].astype(np.float64) @ r["p"]["attention_score.weight"].astype(np.float64).T
                    + r["p"]["attention_score.bias"]) @ r["p"]["attention_final.weight"].astype(np.float64).T
        assert (s.max(axis=1) - s.min(axis=1)).max() > 160
    out, grads = _hip(gpu, r)
    _check_case(name, r, floor, out, grads)
    if name == "identical_neighbours":     # a is uniform and da equal: nothing may reach the score branch but rounding
        assert np.abs(grads["attention_score.weight"]).max() <= 1e-6 * np.abs(grads["cst_hidden.weight"]).max()


def _bitwise(a, b, what):
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, f"{what}: {k} given on one side only"
        else:
            assert np.array_equal(a[k], b[k]), f"{what}: {k} differs in {int((a[k] != b[k]).sum())} elements"


def test_backward_is_bitwise_reproducible_and_switches_change_nothing_else(gpu, refs):
    cases, _ = refs
    c = cases["parity6"]                                  # several reduction splits and column-sum chunks
    out1, g1 = _hip(gpu, c)
    out2, g2 = _hip(gpu, c)
    assert np.array_equal(out1, out2)
    _bitwise(g1, g2, "second run")
    # dx not requested: None for x, every other gradient unchanged
    _, g3 = _hip(gpu, c, x_grad=False)
    assert g3.pop("x") is None
    _bitwise({k: g1[k] for k in g3}, g3, "without dx")
    # frozen cst_output: None for its two gradients, the rest unchanged
    frozen = ("cst_output.weight", "cst_output.bias")
    _, g4 = _hip(gpu, c, frozen=frozen)
    for k in frozen:
        assert g4.pop(k) is None
    _bitwise({k: g1[k] for k in g4}, g4, "frozen cst_output")
    # the whole score and cst branch frozen and no dx: that half of the backward is not run, the head's gradients are unchanged
    frozen = PR.PARAM_NAMES[:8]
    _, g5 = _hip(gpu, c, x_grad=False, frozen=frozen)
    assert g5.pop("x") is None
    for k in frozen:
        assert g5.pop(k) is None
    assert sorted(g5) == sorted(PR.PARAM_NAMES[8:])
    _bitwise({k: g1[k] for k in g5}, g5, "frozen score and cst branch")
    # one of the pair (dW1, dW3) frozen: the other is unchanged
    _, g6 = _hip(gpu, c, frozen=("cst_hidden.weight",))
    assert g6.pop("cst_hidden.weight") is None
    _bitwise({k: g1[k] for k in g6}, g6, "frozen cst_hidden.weight")


def test_ones_mask_equals_no_mask_bitwise(gpu, refs):
    cases, _ = refs
    c = dict(cases["parity2"])
    out0, g0 = _hip(gpu, c)
    c["mask"] = np.ones((PARITY[2][0], PARITY[2][3]), np.float32)
    out1, g1 = _hip(gpu, c)
    assert np.array_equal(out0, out1)
    _bitwise(g0, g1, "mask of ones")


def _layer(gpu, D, H, Oo, sd, dropout=0.0, train_hip=True):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, projection_hidden_dim=H, projection_output_dim=Oo, projection_dropout=dropout,
               projection_train_hip=train_hip, use_gradient_checkpointing=True)
    layer = R.ProjectionLayer(cfg, D)
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return layer.train()


def _module_grads(layer, x_grad=None):
    g = {k: p.grad.cpu().numpy() for k, p in layer.named_parameters()}
    if x_grad is not None:
        g["x"] = x_grad.cpu().numpy()
    return g


def test_other_float_dtypes_are_cast_not_reinterpreted(gpu, refs):
    """The kernels read float32 through raw pointers.  Without autocast nothing casts for them, so the module does: a half or
    double input, or a .double() module, gives what the float32 call gives on the same values, gradients come back in the
    caller's dtype, and the autograd function itself refuses anything that is not float32."""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.projection import _ProjectionTrainFn
    cases, _ = refs
    c = cases["parity2"]
    B, K, D, H, Oo = PARITY[2]
    g = torch.tensor(c["g"], device=gpu)

    def run(layer, x):
        layer.zero_grad()
        out = layer(x)
        assert out.dtype == torch.float32 and out.shape == (B, Oo)
        out.backward(g)
        return out.detach().cpu().numpy(), _module_grads(layer, x.grad)

    layer = _layer(gpu, D, H, Oo, c["p"])
    x16 = torch.tensor(c["x"], device=gpu).half()                      # the values a half tensor holds, then as float32
    o32, g32 = run(layer, x16.float().requires_grad_(True))
    xh = x16.clone().requires_grad_(True)
    o16, g16 = run(layer, xh)
    assert xh.grad.dtype == torch.float16 and xh.grad.shape == xh.shape
    assert np.array_equal(o16, o32)
    dx16, dx32 = g16.pop("x"), g32.pop("x")
    _bitwise(g32, g16, "half input")
    assert np.array_equal(dx16, dx32.astype(np.float16))               # the float32 dx, rounded once to the caller's dtype
    xd = x16.double().requires_grad_(True)
    od, gd = run(layer, xd)
    assert xd.grad.dtype == torch.float64 and np.array_equal(od, o32)
    g32["x"] = dx32
    _bitwise(g32, {k: v.astype(np.float32) for k, v in gd.items()}, "double input")
    layer64 = _layer(gpu, D, H, Oo, c["p"]).double()                   # float64 parameters holding float32 values
    xd2 = x16.double().requires_grad_(True)
    o64, g64 = run(layer64, xd2)
    assert all(p.grad.dtype == torch.float64 for p in layer64.parameters()) and np.array_equal(o64, o32)
    _bitwise(g32, {k: v.astype(np.float32) for k, v in g64.items()}, "double module")
    params = [getattr(getattr(layer, m), leaf) for m, leaf in
              (n.rsplit(".", 1) for n in PR.PARAM_NAMES)]
    with pytest.raises(TypeError, match="float32"):
        _ProjectionTrainFn.apply(x16, None, 1.0, *params)
    with pytest.raises(TypeError, match="float32"):
        _ProjectionTrainFn.apply(x16.float(), None, 1.0, *[p.double() for p in params])
    with pytest.raises(ValueError, match="shape"):
        _ProjectionTrainFn.apply(x16.float()[:, :, :-1], None, 1.0, *params)


def test_training_mode_means_dropout_even_with_nothing_to_differentiate(gpu, refs):
    """A frozen projection under a trained head: the module is in training mode, so dropout applies (projection.py:100), although
    neither x nor any parameter needs a gradient."""
    import torch
    cases, _ = refs
    c = cases["parity2"]
    B, K, D, H, Oo = PARITY[2]
    layer = _layer(gpu, D, H, Oo, c["p"], dropout=0.5).requires_grad_(False)
    x = torch.tensor(c["x"], device=gpu)
    torch.manual_seed(11)
    a = layer(x)
    torch.manual_seed(12)
    b = layer(x)
    assert not a.requires_grad and not torch.equal(a, b)
    torch.manual_seed(11)
    mask = torch.empty((B, H), device=gpu, dtype=torch.float32).bernoulli_(0.5).cpu().numpy()
    want, _ = PR.out_and_grads(c["x"], c["p"], c["g"], torch.float64, "cpu", mask, 2.0)
    np.testing.assert_allclose(a.cpu().numpy(), want, rtol=0, atol=1e-4 * np.abs(want).max())
    with torch.no_grad():
        e1, e2 = layer(x), layer(x)                                    # no_grad: the eval kernels, no dropout, as before
    assert torch.equal(e1, e2)
    off = _layer(gpu, D, H, Oo, c["p"], dropout=0.5, train_hip=False).requires_grad_(False)
    assert torch.equal(off(x), e1)                                     # key unset: unchanged behaviour


def test_expanded_grad_output_equals_ones(gpu, refs):
    import torch
    cases, _ = refs
    c = cases["parity2"]
    B, K, D, H, Oo = PARITY[2]
    layer = _layer(gpu, D, H, Oo, c["p"])
    x = torch.tensor(c["x"], device=gpu)
    layer(x).sum().backward()                             # autograd hands the backward a stride-0 expand
    g_sum = _module_grads(layer)
    layer.zero_grad()
    out = layer(x)
    out.backward(torch.ones_like(out))
    _bitwise(g_sum, _module_grads(layer), "sum().backward() vs backward(ones)")


def test_module_dropout_follows_torch_seed(gpu, refs):
    import torch
    cases, _ = refs
    c = cases["parity2"]
    B, K, D, H, Oo = PARITY[2]
    layer = _layer(gpu, D, H, Oo, c["p"], dropout=0.5)
    x = torch.tensor(c["x"], device=gpu)
    torch.manual_seed(1234)
    a = layer(x).detach().cpu().numpy()
    torch.manual_seed(1234)
    b = layer(x).detach().cpu().numpy()
    torch.manual_seed(4321)
    d = layer(x).detach().cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, d)
    # the mask the module drew is torch's: the same seed and draw give the helper's output in float64 within the forward's bound
    torch.manual_seed(1234)
    mask = torch.empty((B, H), device=gpu, dtype=torch.float32).bernoulli_(0.5).cpu().numpy()
    want, _ = PR.out_and_grads(c["x"], c["p"], c["g"], torch.float64, "cpu", mask, 2.0)
    assert 0 < mask.mean() < 1
    np.testing.assert_allclose(a, want, rtol=0, atol=1e-4 * np.abs(want).max())


def test_autocast_and_grad_scaler(gpu, refs):
    """The reference's training step (pipeline.py:784-829): forward under autocast, GradScaler around the backward."""
    import torch
    cases, floor = refs
    c = cases["parity2"]
    B, K, D, H, Oo = PARITY[2]
    layer = _layer(gpu, D, H, Oo, c["p"])
    opt = torch.optim.SGD(layer.parameters(), lr=0.0)
    scaler = torch.amp.GradScaler("cuda", init_scale=1024.0)      # a power of two: scaling and unscaling are exact
    x = torch.tensor(c["x"], device=gpu, requires_grad=True)
    g = torch.tensor(c["g"], device=gpu)
    with torch.autocast("cuda"):
        out = layer(x)
        assert out.dtype == torch.float32
        assert layer(x.detach().half()).dtype == torch.float32    # a half input from upstream is cast up, not computed in half
        loss = (out.float() * g).sum()
    scaler.scale(loss).backward()
    scaler.unscale_(opt)
    _check_case("autocast", c, floor, out.detach().cpu().numpy(), _module_grads(layer, x.grad / scaler.get_scale()))   # unscale_ covers the parameters only


def test_train_forward_equals_eval_forward_and_fold_follows_the_optimizer(gpu, refs):
    import torch
    cases, _ = refs
    c = cases["parity6"]
    B, K, D, H, Oo = PARITY[6]
    layer = _layer(gpu, D, H, Oo, c["p"])
    x = torch.tensor(c["x"], device=gpu)
    out_train = layer(x)
    with torch.no_grad():
        out_eval = layer.eval()(x)
    np.testing.assert_allclose(out_train.detach().cpu().numpy(), out_eval.cpu().numpy(), rtol=0, atol=1e-4)
    layer.train()
    opt = torch.optim.SGD(layer.parameters(), lr=0.05)
    (layer(x) * torch.tensor(c["g"], device=gpu)).sum().backward()
    opt.step()
    sd = {k: v.detach().cpu().numpy() for k, v in layer.state_dict().items()}
    assert np.abs(sd["cst_output.weight"] - c["p"]["cst_output.weight"]).max() > 0
    want = PR.forward(torch.tensor(c["x"], dtype=torch.float64), {k: torch.tensor(v, dtype=torch.float64) for k, v in sd.items()})
    with torch.no_grad():
        got = layer.eval()(x).cpu().numpy()               # the W5 W4 fold cached before the step must not survive it
    np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-4)
    assert np.abs(got - out_eval.cpu().numpy()).max() > 1e-3


def test_lds_limit_is_a_value_error_not_a_launch(gpu):
    import torch
    layer = _layer(gpu, 16, 2048, 8, _params(16, 2048, 8, 3))
    x = torch.zeros((2, 16, 16), device=gpu)              # K * H = 32768: 2 K H floats do not fit the 160 KB LDS
    with pytest.raises(ValueError, match="LDS"):
        layer(x)
    assert layer(x[:, :5]).shape == (2, 8)                # the same layer with five neighbours runs


def test_thousands_of_neighbours_with_hidden_one(gpu):
    """K = 8200 is legal with hidden = 1 (the tail's LDS bound is on K * hidden); the attention backward then keeps 2 K floats in
    LDS, above the 64 KB a kernel gets unasked.  The call must run.  With one hidden unit LayerNorm's output is beta whatever
    comes in, so in exact arithmetic nothing upstream of it gets a gradient; out, dW6, db6 and dbeta are checked
    against float64 at 1e-5 of their size (sums of two or three float32 terms)."""
    import torch
    c = _plain(2, 8200, 4, 1, 3, seed=26)
    o64, g64 = PR.out_and_grads(c["x"], c["p"], c["g"], torch.float64)
    out, grads = _hip(gpu, c)
    live = ("unified_embedding.weight", "unified_embedding.bias", "normalization.bias")
    np.testing.assert_allclose(out, o64, rtol=0, atol=1e-5 * np.abs(o64).max())
    for k, v in grads.items():
        assert v.shape == g64[k].shape and np.isfinite(v).all(), k
        if k in live:
            np.testing.assert_allclose(v, g64[k], rtol=0, atol=1e-5 * np.abs(g64[k]).max(), err_msg=k)
        else:
            # float64 leaves 1e-13 here (rounding times rstd = 1000); float32 rounding of the O(1) values times rstd is 1e-4
            assert np.abs(g64[k]).max() < 1e-9 and np.abs(v).max() < 1e-3, f"{k}: nothing passes a LayerNorm over one unit"


def _radad_model(gpu, D, train_hip):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, projection_dropout=0.0, detection_dropout=0.0, projection_train_hip=train_hip)
    torch.manual_seed(7)
    return R.RADADModel(cfg, D).train()


def _restated_model(model, dtype, device):
    """RADADModel's training forward from the helper plus copies of the torch modules, parameters as leaves of `dtype`."""
    import copy
    import torch
    sd = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in model.projection_layer.named_parameters()}
    fuse = copy.deepcopy(model.fuse).to(device=device, dtype=dtype)
    head = copy.deepcopy(model.detection_model.model).to(device=device, dtype=dtype).train()

    def run(x, t, y):
        proj = PR.forward(x.to(device=device, dtype=dtype), sd)
        logits = head(fuse(torch.cat([t.to(device=device, dtype=dtype), proj], 1))).squeeze(-1)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, y.to(device=device, dtype=dtype))
        loss.backward()
        g = {"projection_layer." + k: v.grad for k, v in sd.items()}
        g.update({"fuse." + k: v.grad for k, v in fuse.named_parameters()})
        g.update({"detection_model.model." + k: v.grad for k, v in head.named_parameters()})
        return float(loss.detach()), {k: v.double().cpu().numpy() for k, v in g.items()}
    return run


def test_radad_model_trains(gpu, refs):
    import torch
    _, floor = refs
    B, K, D = 37, 5, 512
    rng = np.random.default_rng(77)
    x = torch.tensor(rng.standard_normal((B, K, D)).astype(np.float32), device=gpu)
    t = torch.tensor(rng.standard_normal((B, D)).astype(np.float32), device=gpu)
    y = torch.tensor((rng.random(B) < 0.5).astype(np.float32), device=gpu)
    off = _radad_model(gpu, D, train_hip=False)
    with pytest.raises(RuntimeError, match="inference-only"):
        off(x, t)
    model = _radad_model(gpu, D, train_hip=True)
    loss64, g64 = _restated_model(model, torch.float64, "cpu")(x, t, y)
    _, g32 = _restated_model(model, torch.float32, gpu)(x, t, y)
    bn = [m for m in model.detection_model.model if isinstance(m, torch.nn.BatchNorm1d)]
    before = [m.running_mean.clone() for m in bn]
    loss_fn = torch.nn.BCEWithLogitsLoss()
    loss = loss_fn(model(x, t), y)
    loss.backward()
    assert abs(float(loss.detach()) - loss64) < 1e-5
    assert bn and all(not torch.equal(m.running_mean, b) for m, b in zip(bn, before)), "BatchNorm running statistics did not move"
    # Gradients that are zero in exact arithmetic: a shift that is constant over the batch and reaches a training-mode BatchNorm
    # through Linear layers only is removed by the batch mean.  That holds for the Linear biases directly in front of a BatchNorm,
    # and here also for fuse.bias, the projection's b6 and beta (the same shift of `proj` in every row), and for db2 (module
    # docstring).  float64 leaves 1e-18 of noise there and float32 1e-9, and a ratio of two noises measures nothing.  They must
    # instead be zero to float32 rounding, measured as db2 is: at most 4 x the larger of torch float32's own residue and 1e-6 of the
    # largest gradient of the weight they belong to.
    mods = list(model.detection_model.model)
    assert isinstance(mods[0], torch.nn.Linear) and isinstance(mods[1], torch.nn.BatchNorm1d)
    dead = {f"detection_model.model.{i}.bias" for i, m in enumerate(mods[:-1])
            if isinstance(m, torch.nn.Linear) and isinstance(mods[i + 1], torch.nn.BatchNorm1d)}
    dead |= {"fuse.bias", "projection_layer.unified_embedding.bias", "projection_layer.normalization.bias",
             "projection_layer.attention_final.bias"}
    bad = []
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        e_hip, e_t32 = _rel(p.grad.cpu().numpy(), g64[k]), _rel(g32[k], g64[k])
        bound = FACTOR * (e_t32 if e_t32 > 0 else floor)
        if k in dead:
            got = np.abs(p.grad.cpu().numpy()).max()
            cap = FACTOR * max(np.abs(g32[k]).max(), 1e-6 * np.abs(g64[k.replace(".bias", ".weight")]).max())
            print(f"proj_train radad_model            {k:44s} |hip| {got:.3e}  |torch32| {np.abs(g32[k]).max():.3e}  cap {cap:.3e}  (zero in exact arithmetic)")
            if not got <= cap:
                bad.append(f"{k}: zero in exact arithmetic, must be of rounding size: {got:.3e} > {cap:.3e}")
            continue
        print(f"proj_train radad_model            {k:44s} hip {e_hip:.3e}  torch32 {e_t32:.3e}  bound {bound:.3e}")
        if not e_hip <= bound:
            bad.append(f"{k}: err {e_hip:.3e} > {FACTOR} x torch float32 err {e_t32:.3e}")
    assert not bad, "; ".join(bad)
    # fuse_and_detect follows the same switch
    proj = model.projection_layer(x)
    assert model.fuse_and_detect(t, proj).requires_grad
    with pytest.raises(RuntimeError, match="inference-only"):
        off.fuse_and_detect(t, proj.detach())
    # three SGD steps on the fixed batch lower the loss
    model.zero_grad()
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        l = loss_fn(model(x, t), y)
        losses.append(float(l.detach()))
        l.backward()
        opt.step()
    assert losses[3] < losses[0], losses
