"""GPU: training forward and backward of the fuse Linear + detection MLP (csrc/head_train.inc) against float64 autograd.

The bound is that of tests/test_gpu_proj_train.py.  For the logits, each gradient (dtpp, dproj and every parameter) and the
updated running statistics:
    err = max|got - f64| / max|f64|        f64 = tests/head_train_ref.py in float64 on the CPU
and the HIP path's err may be at most FACTOR = 4 times the err of torch's own float32 autograd of the same helper on the same
device and input (allow_tf32 off).  Where torch's float32 result happens to be exact (err 0), the largest torch-float32 err over
the plain parity cases of this file stands in as the floor.  Where float64 itself says a value is exactly zero, the HIP value must
be exactly zero.  Nothing is ever bounded against the HIP result itself.

Gradients that are zero in exact arithmetic for every input -- the bias of a Linear directly in front of a training-mode
BatchNorm, and fuse.bias when the first hidden layer has one (the batch mean removes a shift that is constant over the batch) --
leave 1e-16 of noise in float64 and 1e-8 in float32, and a ratio of two noises measures nothing.  They get that file's absolute
cap: |g| <= 4 max(|g of torch float32|, 1e-6 max|gradient of the weight the bias belongs to|).

Every measured pair is printed before it is asserted (run with -s); profiles/head_train.md keeps one run's figures.
Every test here fails without the feature: there is no _FuseHeadTrainFn, and config.head_train_hip does nothing.
"""
import numpy as np
import pytest

import head_train_ref as HR
import proj_train_ref as PR

pytestmark = pytest.mark.gpu

FACTOR = 4.0
F32 = np.float32


def _params(D, P, hidden, seed, bn=True):
    """nn.Linear weights ~ N(0, 1/fan_in), biases ~ N(0, 0.3^2), BatchNorm gain 1 + N(0, 0.01), shift N(0, 0.01)."""
    rng = np.random.default_rng(seed)
    w = lambda o, i: (rng.standard_normal((o, i)) / np.sqrt(i)).astype(F32)
    b = lambda n, s=0.3: (s * rng.standard_normal(n)).astype(F32)
    p = {"fuse.weight": w(P, D + P), "fuse.bias": b(P)}
    dims = [P] + list(hidden) + [1]
    for i in range(len(dims) - 1):
        p[f"lin{i}.weight"], p[f"lin{i}.bias"] = w(dims[i + 1], dims[i]), b(dims[i + 1])
        if bn and i < len(hidden):
            p[f"bn{i}.weight"], p[f"bn{i}.bias"] = (1 + b(dims[i + 1], 0.1)).astype(F32), b(dims[i + 1], 0.1)
    return p


def _plain(B, D, P, hidden, seed, bn=True):
    rng = np.random.default_rng(seed + 1000)
    c = {"tpp": rng.standard_normal((B, D)).astype(F32), "proj": rng.standard_normal((B, P)).astype(F32),
         "p": _params(D, P, hidden, seed, bn), "g": rng.standard_normal((B, 1)).astype(F32), "hidden": list(hidden),
         "masks": None, "inv_keep": 1.0, "eps": 1e-5, "factor": [0.1] * len(hidden)}
    c["running"] = [((0.5 * rng.standard_normal(d)).astype(F32), rng.uniform(0.5, 2.0, d).astype(F32)) if bn else None for d in hidden]
    return c


PARITY = [(2, 8, 1, [1]), (3, 5, 3, []), (37, 130, 24, [10, 3]), (130, 447, 128, [64, 32]), (300, 512, 128, [65, 130]),
          (37, 64, 16, [8, 8, 8, 8, 8])]
DESIGN_SHAPE = (37, 44, 24, [10, 6])


def _shifted_columns():
    c = _plain(*DESIGN_SHAPE, seed=31)
    c["p"]["lin0.bias"][:] = 1000          # z = 1000 +- 1: a one-pass E[z^2] - mean^2 variance loses every digit
    return c


def _constant_column():
    c = _plain(*DESIGN_SHAPE, seed=32)
    c["p"]["lin0.weight"][3] = 0            # z[:, 3] = b[3] in every row: variance exactly 0, xh = 0
    c["p"]["lin1.weight"][2] = 0
    return c


def _relu_ties():
    c = _plain(*DESIGN_SHAPE, seed=33)
    c["p"]["bn0.weight"][2] = c["p"]["bn0.bias"][2] = 0      # y = 0 in every row of the column: relu'(0) = 0, as torch
    c["p"]["bn1.weight"][4] = c["p"]["bn1.bias"][4] = 0
    return c


def _masks_half():
    c = _plain(*DESIGN_SHAPE, seed=34)
    rng = np.random.default_rng(98)
    c["masks"] = [(rng.random((DESIGN_SHAPE[0], d)) < 0.5).astype(F32) for d in DESIGN_SHAPE[3]]
    c["inv_keep"] = 2.0
    return c


BUILDERS = {f"parity{i}": (lambda s=s, i=i: _plain(*s, seed=i)) for i, s in enumerate(PARITY)}
BUILDERS["no_batch_norm"] = lambda: _plain(*PARITY[2], seed=11, bn=False)
BUILDERS.update(shifted_columns=_shifted_columns, constant_column=_constant_column, relu_ties=_relu_ties, masks_half=_masks_half)


def _rel(got, want):
    scale = float(np.abs(want).max())
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / (scale if scale > 0 else 1.0)


def _dead(p):
    """Gradients that are zero in exact arithmetic (module docstring) -> the weight whose size their cap is taken from."""
    n = HR.n_layers(p)
    dead = {f"lin{i}.bias": f"lin{i}.weight" for i in range(n - 1) if f"bn{i}.weight" in p}
    if "bn0.weight" in p:
        dead["fuse.bias"] = "fuse.weight"
    return dead


def _flat(logits, grads, running):
    """{key: value} of everything compared, from out_and_grads' (logits, grads, running) triple."""
    out = {"logits": logits}
    out.update(grads)
    for i, pair in enumerate(running):
        if pair is not None:
            out[f"running_mean{i}"], out[f"running_var{i}"] = pair
    return out


@pytest.fixture(scope="module")
def refs(gpu):
    """Per accuracy case: the inputs, float64 values on the CPU, torch float32 values and errs on the device; and the file's floor."""
    import torch
    was = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    out = {}
    for name, build in BUILDERS.items():
        c = build()
        args = (c["tpp"], c["proj"], c["p"], c["g"])
        kw = dict(masks=c["masks"], inv_keep=c["inv_keep"], eps=c["eps"], running=c["running"], factor=c["factor"])
        v64 = _flat(*HR.out_and_grads(*args, torch.float64, "cpu", **kw))
        v32 = _flat(*HR.out_and_grads(*args, torch.float32, gpu, **kw))
        out[name] = dict(c, v64=v64, v32=v32, t32={k: _rel(v32[k], v64[k]) for k in v64})
    torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = was
    floor = max(v for name, r in out.items() if name.startswith("parity") for k, v in r["t32"].items() if k not in _dead(r["p"]))
    assert 0 < floor < 0.5, f"torch float32 autograd is off by {floor}: the reference itself is broken"
    return out, floor


def _hip(gpu, c, tpp_grad=True, frozen=(), expand_grad=False):
    """{key: numpy} of the HIP autograd function on case c's inputs: logits, gradients (None where not asked for), running stats."""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.radad_model import HeadTrainSpec, _FuseHeadTrainFn
    dev = lambda a: torch.tensor(a, device=gpu)
    tpp, proj = dev(c["tpp"]).requires_grad_(tpp_grad), dev(c["proj"]).requires_grad_(True)
    p = {k: dev(v).requires_grad_(k not in frozen) for k, v in c["p"].items()}
    running = [None if r is None else (dev(r[0]), dev(r[1])) for r in c["running"]]
    masks = None if c["masks"] is None else [None if m is None else dev(m) for m in c["masks"]]
    spec = HeadTrainSpec([f"bn{i}.weight" in p for i in range(len(c["hidden"]))], [c["eps"]] * len(c["hidden"]), c["factor"], running,
                         masks, c["inv_keep"])
    logits, fused = _FuseHeadTrainFn.apply(tpp, proj, spec, *[p[k] for k in HR.param_names(p)])
    assert logits.dtype == torch.float32 and not fused.requires_grad
    if expand_grad:
        logits.sum().backward()               # autograd hands the backward a stride-0 expand
    else:
        logits.backward(dev(c["g"]))
    np_ = lambda t: None if t is None else t.detach().cpu().numpy()
    out = {"logits": np_(logits), "tpp": np_(tpp.grad), "proj": np_(proj.grad)}
    out.update({k: np_(v.grad) for k, v in p.items()})
    for i, pair in enumerate(running):
        if pair is not None:
            out[f"running_mean{i}"], out[f"running_var{i}"] = np_(pair[0]), np_(pair[1])
    return out


def _check_case(name, r, floor, got, skip=()):
    bad = []
    dead = _dead(r["p"])
    for key, want in r["v64"].items():
        if key in skip:
            continue
        g = got[key]
        assert g is not None and g.shape == want.shape, f"{name} {key}: shape {None if g is None else g.shape} != {want.shape}"
        assert np.isfinite(g).all(), f"{name} {key}: not finite"
        e_hip, e_t32 = _rel(g, want), r["t32"][key]
        bound = FACTOR * (e_t32 if e_t32 > 0 else floor)
        if key in dead:
            t32 = float(np.abs(r["v32"][key]).max())
            cap = FACTOR * max(t32, 1e-6 * float(np.abs(r["v64"][dead[key]]).max()))
            print(f"head_train {name:18s} {key:16s} |hip| {np.abs(g).max():.3e}  |torch32| {t32:.3e}  cap {cap:.3e}  (zero in exact arithmetic)")
            if not np.abs(g).max() <= cap:
                bad.append(f"{key}: zero in exact arithmetic, must be of rounding size: {np.abs(g).max():.3e} > {cap:.3e}")
            continue
        print(f"head_train {name:18s} {key:16s} hip {e_hip:.3e}  torch32 {e_t32:.3e}  bound {bound:.3e}")
        if not np.abs(want).max() > 0:
            if np.abs(g).max() != 0:
                bad.append(f"{key}: float64 says exactly zero, HIP gives up to {np.abs(g).max():.3e}")
        elif not e_hip <= bound:
            bad.append(f"{key}: err {e_hip:.3e} > {FACTOR} x torch float32 err {e_t32:.3e}")
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("i", range(len(PARITY)), ids=["x".join(map(str, s[:3])) + "x" + "-".join(map(str, s[3])) for s in PARITY])
def test_gradient_parity(gpu, refs, i):
    cases, floor = refs
    name = f"parity{i}"
    _check_case(name, cases[name], floor, _hip(gpu, cases[name]))


def test_without_batch_norm(gpu, refs):
    cases, floor = refs
    got = _hip(gpu, cases["no_batch_norm"])
    assert not any(k.startswith("running") for k in got)
    _check_case("no_batch_norm", cases["no_batch_norm"], floor, got)


def test_tpp_gradient_only_when_asked_for(gpu, refs):
    cases, floor = refs
    r = cases["parity2"]
    with_tpp = _hip(gpu, r)
    _check_case("parity2 (dtpp)", r, floor, with_tpp)
    without = _hip(gpu, r, tpp_grad=False)
    assert without.pop("tpp") is None
    _bitwise({k: with_tpp[k] for k in without}, without, "without dtpp")


@pytest.mark.parametrize("name", ["shifted_columns", "constant_column", "relu_ties", "masks_half"])
def test_designed_inputs(gpu, refs, name):
    cases, floor = refs
    r = cases[name]
    p64 = {k: v.astype(np.float64) for k, v in r["p"].items()}
    fused = np.concatenate([r["tpp"], r["proj"]], 1).astype(np.float64) @ p64["fuse.weight"].T + p64["fuse.bias"]
    z = fused @ p64["lin0.weight"].T + p64["lin0.bias"]
    if name == "shifted_columns":      # the input really defeats a one-pass variance in float32
        z32 = z.astype(F32)
        one_pass = (z32 * z32).mean(0, dtype=F32) - z32.mean(0, dtype=F32) ** 2
        assert (np.abs(one_pass - z.var(0)) / z.var(0)).max() > 0.01
        assert 0.2 < z.std(0).min() and np.abs(z.mean(0) - 1000).max() < 5
    if name == "constant_column":      # the column really is constant
        assert np.ptp(z[:, 3]) == 0 and np.ptp(z[:, 2]) > 0
    got = _hip(gpu, r)
    _check_case(name, r, floor, got)
    if name == "relu_ties":            # nothing passes the tied columns, exactly
        assert not got["bn0.weight"][2] and not got["bn0.bias"][2] and not got["lin0.weight"][2].any()
        assert not got["bn1.weight"][4] and not got["bn1.bias"][4] and not got["lin1.weight"][4].any()
        assert not r["v64"]["lin0.weight"][2].any()
    if name == "masks_half":
        assert 0.3 < r["masks"][0].mean() < 0.7


def _bitwise(a, b, what):
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, f"{what}: {k} given on one side only"
        else:
            assert np.array_equal(a[k], b[k]), f"{what}: {k} differs in {int((a[k] != b[k]).sum())} elements"


def test_ones_mask_equals_no_mask_bitwise(gpu, refs):
    cases, _ = refs
    c = dict(cases["parity2"])
    base = _hip(gpu, c)
    c["masks"] = [np.ones((PARITY[2][0], d), F32) for d in PARITY[2][3]]
    _bitwise(base, _hip(gpu, c), "mask of ones")


def test_reproducible_bitwise_and_freezing_changes_nothing_else(gpu, refs):
    cases, _ = refs
    c = cases["parity4"]                                  # several reduction splits, column-sum chunks and slabs
    g1 = _hip(gpu, c)
    _bitwise(g1, _hip(gpu, c), "second run")
    for frozen in (("fuse.weight",), ("lin0.weight", "lin0.bias"), ("bn1.weight",), ("bn0.bias", "lin2.weight", "fuse.bias")):
        g = _hip(gpu, c, frozen=frozen)
        for k in frozen:
            assert g.pop(k) is None, k
        _bitwise({k: g1[k] for k in g}, g, f"frozen {frozen}")
    c1 = dict(c, g=np.ones_like(c["g"]))
    _bitwise(_hip(gpu, c1), _hip(gpu, c1, expand_grad=True), "sum().backward() vs backward(ones)")


def test_function_refuses_what_the_kernels_cannot_index(gpu, refs):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.radad_model import HeadTrainSpec, _FuseHeadTrainFn
    cases, _ = refs
    c = cases["parity2"]
    dev = lambda a: torch.tensor(a, device=gpu)
    p = {k: dev(v) for k, v in c["p"].items()}
    order = HR.param_names(p)
    spec = lambda: HeadTrainSpec([True, True])
    tpp, proj = dev(c["tpp"]), dev(c["proj"])
    with pytest.raises(TypeError, match="float32"):
        _FuseHeadTrainFn.apply(tpp.double(), proj, spec(), *[p[k] for k in order])
    with pytest.raises(TypeError, match="float32"):
        _FuseHeadTrainFn.apply(tpp, proj, spec(), *[p[k].double() if k == "bn0.weight" else p[k] for k in order])
    with pytest.raises(ValueError, match="shape"):
        _FuseHeadTrainFn.apply(tpp[:, :-1], proj, spec(), *[p[k] for k in order])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        _FuseHeadTrainFn.apply(tpp[:1], proj[:1], spec(), *[p[k] for k in order])


# ---- module level -------------------------------------------------------------------------------------------------------------

def _radad_model(gpu, D, head_hip=True, proj_hip=True, dropout=0.0, **cfg_kw):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, projection_dropout=0.0, detection_dropout=dropout, projection_train_hip=proj_hip, head_train_hip=head_hip,
               **cfg_kw)
    torch.manual_seed(7)
    model = R.RADADModel(cfg, D).train()
    with torch.no_grad():                                  # running statistics away from their (0, 1) start
        for m in model.detection_model.model:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.normal_(0, 0.5)
                m.running_var.uniform_(0.5, 2.0)
    return model


def _head_case(model, t, proj, g=None):
    """The model's fuse + head as a helper case (numpy)."""
    p, bns = HR.params_of(model.fuse, model.detection_model)
    n = lambda v: v.detach().cpu().numpy()
    return {"tpp": n(t), "proj": n(proj), "p": {k: n(v) for k, v in p.items()}, "g": g,
            "running": [None if bn is None else (n(bn.running_mean), n(bn.running_var)) for bn in bns],
            "eps": bns[0].eps if bns and bns[0] is not None else 1e-5}, bns


def _batch(gpu, B=37, K=5, D=512, seed=77):
    import torch
    rng = np.random.default_rng(seed)
    x = torch.tensor(rng.standard_normal((B, K, D)).astype(F32), device=gpu)
    t = torch.tensor(rng.standard_normal((B, D)).astype(F32), device=gpu)
    y = torch.tensor((rng.random(B) < 0.5).astype(F32), device=gpu)
    return x, t, y


def _restated(model, dtype, device):
    """RADADModel's training step from the two helpers, parameters as leaves of `dtype`: (loss, {parameter name: gradient})."""
    import torch
    sd = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in model.projection_layer.named_parameters()}
    p, bns = HR.params_of(model.fuse, model.detection_model)
    names = {id(v): k for k, v in model.named_parameters()}
    to_model = {k: names[id(v)] for k, v in p.items()}
    p = {k: v.detach().to(device=device, dtype=dtype).requires_grad_(True) for k, v in p.items()}

    def run(x, t, y):
        proj = PR.forward(x.to(device=device, dtype=dtype), sd)
        logits, _ = HR.forward(t.to(device=device, dtype=dtype), proj, p, eps=bns[0].eps)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.squeeze(-1), y.to(device=device, dtype=dtype))
        loss.backward()
        g = {"projection_layer." + k: v.grad for k, v in sd.items()}
        g.update({to_model[k]: v.grad for k, v in p.items()})
        return float(loss.detach()), {k: v.double().cpu().numpy() for k, v in g.items()}
    return run


def test_whole_model_trains_in_hip(gpu, refs):
    import torch
    _, floor = refs
    x, t, y = _batch(gpu)
    model = _radad_model(gpu, 512)
    loss64, g64 = _restated(model, torch.float64, "cpu")(x, t, y)
    _, g32 = _restated(model, torch.float32, gpu)(x, t, y)
    bn = [m for m in model.detection_model.model if isinstance(m, torch.nn.BatchNorm1d)]
    before = [m.running_mean.clone() for m in bn]
    loss_fn = torch.nn.BCEWithLogitsLoss()
    logits = model(x, t)
    names = _graph_names(logits)
    assert "_FuseHeadTrainFnBackward" in names and "_ProjectionTrainFnBackward" in names, names
    assert not any("BatchNorm" in n or "Addmm" in n for n in names), f"torch modules still in the graph: {names}"
    loss = loss_fn(logits, y)
    loss.backward()
    assert abs(float(loss.detach()) - loss64) < 1e-5
    assert bn and all(not torch.equal(m.running_mean, b) for m, b in zip(bn, before)), "BatchNorm running statistics did not move"
    assert all(int(m.num_batches_tracked) == 1 for m in bn)
    # zero in exact arithmetic (module docstring; for the projection's b6, beta and b2 see tests/test_gpu_proj_train.py)
    mods = list(model.detection_model.model)
    dead = {f"detection_model.model.{i}.bias" for i, m in enumerate(mods[:-1])
            if isinstance(m, torch.nn.Linear) and isinstance(mods[i + 1], torch.nn.BatchNorm1d)}
    dead |= {"fuse.bias", "projection_layer.unified_embedding.bias", "projection_layer.normalization.bias",
             "projection_layer.attention_final.bias"}
    bad = []
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        got = p.grad.cpu().numpy()
        e_hip, e_t32 = _rel(got, g64[k]), _rel(g32[k], g64[k])
        bound = FACTOR * (e_t32 if e_t32 > 0 else floor)
        if k in dead:
            cap = FACTOR * max(np.abs(g32[k]).max(), 1e-6 * np.abs(g64[k.replace(".bias", ".weight")]).max())
            print(f"head_train radad_model        {k:44s} |hip| {np.abs(got).max():.3e}  |torch32| {np.abs(g32[k]).max():.3e}  cap {cap:.3e}  (zero in exact arithmetic)")
            if not np.abs(got).max() <= cap:
                bad.append(f"{k}: zero in exact arithmetic, must be of rounding size: {np.abs(got).max():.3e} > {cap:.3e}")
            continue
        print(f"head_train radad_model        {k:44s} hip {e_hip:.3e}  torch32 {e_t32:.3e}  bound {bound:.3e}")
        if not e_hip <= bound:
            bad.append(f"{k}: err {e_hip:.3e} > {FACTOR} x torch float32 err {e_t32:.3e}")
    assert not bad, "; ".join(bad)
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


def _graph_names(t):
    """Names of the autograd nodes behind t."""
    seen, stack, names = set(), [t.grad_fn], []
    while stack:
        node = stack.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        names.append(type(node).__name__)
        stack.extend(fn for fn, _ in node.next_functions)
    return names


def test_head_switch_alone_and_switch_off(gpu):
    import torch
    x, t, _ = _batch(gpu)
    proj = torch.tensor(np.random.default_rng(5).standard_normal((37, 128)).astype(F32), device=gpu, requires_grad=True)
    head_only = _radad_model(gpu, 512, head_hip=True, proj_hip=False)
    with pytest.raises(RuntimeError, match="inference-only"):
        head_only(x, t)                                    # the projection still refuses to train
    logits = head_only.fuse_and_detect(t, proj)
    assert logits.shape == (37,) and logits.requires_grad
    logits.sum().backward()
    assert proj.grad is not None and head_only.fuse.weight.grad is not None
    assert all(p.grad is not None for p in head_only.detection_model.parameters())
    lg, fused = head_only.fuse_and_detect(t, proj, return_fused=True)
    assert fused.shape == (37, 128) and not fused.requires_grad
    want = head_only.fuse(torch.cat([t, proj], 1))
    np.testing.assert_allclose(fused.cpu().numpy(), want.detach().cpu().numpy(), rtol=0, atol=1e-4)
    # switch off, projection switch on: the torch modules' graph, as before
    off = _radad_model(gpu, 512, head_hip=False, proj_hip=True)
    lo = off.fuse_and_detect(t, proj)
    names = _graph_names(lo)
    assert not any("FuseHeadTrainFn" in n for n in names) and any("NativeBatchNorm" in n for n in names), names
    assert any("FuseHeadTrainFn" in n for n in _graph_names(logits))
    # neither switch: inference-only, as before
    neither = _radad_model(gpu, 512, head_hip=False, proj_hip=False)
    with pytest.raises(RuntimeError, match="inference-only"):
        neither.fuse_and_detect(t, proj.detach())
    # eval / no_grad take the inference kernel whatever the switch says
    with torch.no_grad():
        a = head_only.fuse_and_detect(t, proj)
    b = head_only.eval().fuse_and_detect(t, proj.detach())
    assert not a.requires_grad and torch.equal(a, b)


def test_running_statistics_momentum_none_and_eval_follows(gpu, refs):
    """momentum=None: a cumulative average, the factor is 1 / num_batches_tracked.  Two steps, then the inference kernel in eval
    mode reads the updated statistics."""
    import torch
    _, floor = refs
    model = _radad_model(gpu, 512, proj_hip=False)
    bns = [m for m in model.detection_model.model if isinstance(m, torch.nn.BatchNorm1d)]
    for m in bns:
        m.momentum = None
    rng = np.random.default_rng(12)
    run64 = run32 = None
    for step in range(2):
        t = torch.tensor(rng.standard_normal((37, 512)).astype(F32), device=gpu)
        proj = torch.tensor(rng.standard_normal((37, 128)).astype(F32), device=gpu)
        c, _ = _head_case(model, t, proj, np.ones((37, 1), F32))
        factor = [1.0 / (step + 1)] * len(bns)
        args = (c["tpp"], c["proj"], c["p"], c["g"])
        _, _, run64 = HR.out_and_grads(*args, torch.float64, "cpu", eps=c["eps"], running=run64 or c["running"], factor=factor)
        _, _, run32 = HR.out_and_grads(*args, torch.float32, gpu, eps=c["eps"], running=run32 or c["running"], factor=factor)
        model.fuse_and_detect(t, proj)
        assert all(int(m.num_batches_tracked) == step + 1 for m in bns)
    bad = []
    for i, m in enumerate(bns):
        for what, got, j in (("running_mean", m.running_mean, 0), ("running_var", m.running_var, 1)):
            e_hip, e_t32 = _rel(got.cpu().numpy(), run64[i][j]), _rel(run32[i][j], run64[i][j])
            bound = FACTOR * (e_t32 if e_t32 > 0 else floor)
            print(f"head_train momentum_none      {what}{i:<4d} hip {e_hip:.3e}  torch32 {e_t32:.3e}  bound {bound:.3e}")
            if not e_hip <= bound:
                bad.append(f"{what}{i}: err {e_hip:.3e} > {FACTOR} x torch float32 err {e_t32:.3e}")
    assert not bad, "; ".join(bad)
    # eval: the inference kernel with the statistics the training steps left (the tolerance of the inference tests)
    c, _ = _head_case(model, t, proj)
    t64 = lambda v: torch.tensor(np.asarray(v), dtype=torch.float64)
    want, _ = HR.forward(t64(c["tpp"]), t64(c["proj"]), {k: t64(v) for k, v in c["p"].items()}, eps=c["eps"],
                         running=[(t64(a), t64(b)) for a, b in run64], train=False)
    got = model.eval().fuse_and_detect(t, proj)
    np.testing.assert_allclose(got.cpu().numpy(), want.squeeze(-1).numpy(), rtol=0, atol=1e-4)


def test_dropout_masks_follow_torch_seed(gpu, refs):
    import torch
    x, t, _ = _batch(gpu)
    proj = torch.tensor(np.random.default_rng(6).standard_normal((37, 128)).astype(F32), device=gpu)
    model = _radad_model(gpu, 512, proj_hip=False, dropout=0.5)
    state = {k: v.clone() for k, v in model.state_dict().items()}

    def run(seed):
        model.load_state_dict(state)                       # the running statistics move with every call
        torch.manual_seed(seed)
        return model.fuse_and_detect(t, proj).detach().cpu().numpy()
    a, b, d = run(1234), run(1234), run(4321)
    assert np.array_equal(a, b) and not np.array_equal(a, d)
    # the masks are torch's: the same seed and draws give the helper's logits in float64
    torch.manual_seed(1234)
    masks = [torch.empty((37, w), device=gpu, dtype=torch.float32).bernoulli_(0.5).cpu().numpy() for w in (64, 32)]
    model.load_state_dict(state)
    c, _ = _head_case(model, t, proj, np.ones((37, 1), F32))
    want, _, _ = HR.out_and_grads(c["tpp"], c["proj"], c["p"], c["g"], torch.float64, "cpu", masks=masks, inv_keep=2.0, eps=c["eps"])
    assert 0 < masks[0].mean() < 1
    np.testing.assert_allclose(a, want[:, 0], rtol=0, atol=1e-4 * np.abs(want).max())
    # detection_dropout = 0 draws nothing: the generator is where it was
    plain = _radad_model(gpu, 512, proj_hip=False, dropout=0.0)
    torch.manual_seed(99)
    before = torch.cuda.get_rng_state(torch.device(gpu))
    plain.fuse_and_detect(t, proj)
    assert torch.equal(before, torch.cuda.get_rng_state(torch.device(gpu)))
    with pytest.raises(ValueError, match="detection_dropout"):
        bad = _radad_model(gpu, 512, proj_hip=False, dropout=0.0)
        bad.config.detection_dropout = 1.0
        bad.fuse_and_detect(t, proj)


def test_autocast_and_grad_scaler(gpu, refs):
    """The reference's training step (pipeline.py:784-829): forward under autocast, GradScaler around the backward."""
    import torch
    _, floor = refs
    _, t, _ = _batch(gpu)
    rng = np.random.default_rng(9)
    proj0 = rng.standard_normal((37, 128)).astype(F32)
    g = torch.tensor(rng.standard_normal(37).astype(F32), device=gpu)

    def step(autocast):
        model = _radad_model(gpu, 512, proj_hip=False)
        proj = torch.tensor(proj0, device=gpu, requires_grad=True)
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        scaler = torch.amp.GradScaler("cuda", init_scale=1024.0, enabled=autocast)      # a power of two: scaling is exact
        with torch.autocast("cuda", enabled=autocast):
            logits = model.fuse_and_detect(t, proj)
            assert logits.dtype == torch.float32
            if autocast:
                assert model.fuse_and_detect(t.half(), proj.detach().half()).dtype == torch.float32
            loss = (logits.float() * g).sum()
        scaler.scale(loss).backward()
        scaler.unscale_(opt)
        grads = {k: p.grad.cpu().numpy() for k, p in model.named_parameters() if p.grad is not None}
        grads["proj"] = (proj.grad / scaler.get_scale()).cpu().numpy() if autocast else proj.grad.cpu().numpy()
        return model, logits.detach().cpu().numpy(), grads
    model, l0, g0 = step(False)
    _, l1, g1 = step(True)
    assert np.array_equal(l0, l1)
    c, _ = _head_case(_radad_model(gpu, 512, proj_hip=False), t, torch.tensor(proj0), g.cpu().numpy()[:, None])
    _, g64, _ = HR.out_and_grads(c["tpp"], c["proj"], c["p"], c["g"], torch.float64, "cpu", eps=c["eps"])
    _, g32, _ = HR.out_and_grads(c["tpp"], c["proj"], c["p"], c["g"], torch.float32, gpu, eps=c["eps"])
    p, _ = HR.params_of(model.fuse, model.detection_model)
    names = {id(v): k for k, v in model.named_parameters()}
    dead = _dead(c["p"])
    assert sorted(g1) == sorted(g0) and len(g1) == len(p) + 1
    bad = []
    for hk, v in list(p.items()) + [("proj", None)]:
        mk = "proj" if v is None else names[id(v)]
        assert np.isfinite(g1[mk]).all(), mk
        if hk in dead:
            continue
        e_hip, e_t32 = _rel(g1[mk], g64[hk]), _rel(g32[hk], g64[hk])
        bound = FACTOR * (e_t32 if e_t32 > 0 else floor)
        print(f"head_train autocast           {mk:34s} hip {e_hip:.3e}  torch32 {e_t32:.3e}  bound {bound:.3e}")
        if not e_hip <= bound:
            bad.append(f"{mk}: err {e_hip:.3e} > {FACTOR} x torch float32 err {e_t32:.3e}")
        assert _rel(g1[mk], g0[mk].astype(np.float64)) <= bound, f"{mk}: the autocast run differs from the plain run"
    assert not bad, "; ".join(bad)


def test_batch_of_one_is_a_value_error_not_a_launch(gpu):
    import torch
    model = _radad_model(gpu, 512, proj_hip=False)
    t = torch.zeros((1, 512), device=gpu)
    proj = torch.zeros((1, 128), device=gpu, requires_grad=True)
    before = [int(m.num_batches_tracked) for m in model.detection_model.model if isinstance(m, torch.nn.BatchNorm1d)]
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        model.fuse_and_detect(t, proj)
    assert before == [int(m.num_batches_tracked) for m in model.detection_model.model if isinstance(m, torch.nn.BatchNorm1d)]
    plain = _radad_model(gpu, 512, proj_hip=False, use_batch_norm=False)       # without BatchNorm one row trains
    assert plain.fuse_and_detect(t, proj).shape == (1,)
