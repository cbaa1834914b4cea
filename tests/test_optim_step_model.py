"""No GPU: tests/optim_step_ref.py against torch's own objects in float64, and every refusal of the optimiser-step ABI
(radad_optim_workspace_bytes, radad_optim_step, radad_bce_logits) and of HipTrainStep's argument checks.

optim_step_ref is what tests/test_gpu_optim_step.py bounds the kernels against.  Here it is pinned, in float64 on the CPU, to
torch.optim.Adam(weight_decay), clip_grad_norm_, torch.amp.GradScaler("cpu") and BCEWithLogitsLoss(pos_weight), to 1e-12.
The C entry points must refuse every bad argument before they touch a device: the pointers below are made-up addresses.
Every test here fails without the feature: the symbols, the ctypes structs and the module do not exist.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_step_ref as OR
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
from radad_retrievalaugmenteddeepfakeaudiodetection_amd import train_step as TS

CLOSE = dict(rtol=0, atol=1e-12)
SHAPES = [(7,), (3, 5), (1,), (11,), (2, 2, 3), (6,)]
GROUP_OF = [0, 0, 1, 1, 1, 3]                  # group 2 is empty; tensor 3 never has a gradient
HYPER = [dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5, max_norm=0.05),     # binds
         dict(lr=3e-3, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=1e-5, max_norm=1e3),       # slack
         dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5, max_norm=1.0),
         dict(lr=1e-3, beta1=0.5, beta2=0.9, eps=1e-8, weight_decay=0.0, max_norm=0.0)]         # norm reported, no clipping


def _torch_arm(params0, n_steps, grads, scaling, interval=3):
    """The reference's tail on float64 CPU tensors: one Adam per non-empty group, GradScaler("cpu"), the loop of
    pipeline.py:817-832 on pre-generated (already scaled) gradients.  Yields per step (params, moments, steps, norms, scale)."""
    ps = [torch.nn.Parameter(torch.tensor(a, dtype=torch.float64)) for a in params0]
    opts = {}
    for gi, h in enumerate(HYPER):
        mine = [ps[i] for i in range(len(ps)) if GROUP_OF[i] == gi]
        if mine:
            opts[gi] = torch.optim.Adam(mine, lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"], weight_decay=h["weight_decay"])
    scaler = torch.amp.GradScaler("cpu", init_scale=1024.0, growth_interval=interval, enabled=scaling)
    if scaling:
        scaler.scale(torch.zeros(1, dtype=torch.float64))           # creates the scale tensor
    for k in range(n_steps):
        for i, p in enumerate(ps):
            p.grad = None if grads[k][i] is None else torch.tensor(grads[k][i], dtype=torch.float64)
        norms = {}
        for gi, opt in opts.items():
            scaler.unscale_(opt)
        for gi, opt in opts.items():
            mine = [ps[i] for i in range(len(ps)) if GROUP_OF[i] == gi]
            if HYPER[gi]["max_norm"] > 0:
                norms[gi] = float(torch.nn.utils.clip_grad_norm_(mine, max_norm=HYPER[gi]["max_norm"]))
            else:
                norms[gi] = float(torch.linalg.vector_norm(torch.stack([q.grad.norm() for q in mine if q.grad is not None])))
        for opt in opts.values():
            scaler.step(opt)
        scaler.update()
        yield ps, opts, norms, (float(scaler.get_scale()) if scaling else None)


def _grads(rng, n_steps, scale, poison):
    out = []
    for k in range(n_steps):
        gs = [None if i == 3 else rng.standard_normal(s) * (scale or 1.0) for i, s in enumerate(SHAPES)]
        if k in poison:
            i, val = poison[k]
            gs[i].reshape(-1)[-1] = val
        out.append(gs)
    return out


@pytest.mark.parametrize("scaling", [True, False], ids=["loss_scale", "no_scale"])
def test_restatement_equals_torch_in_float64(scaling):
    rng = np.random.default_rng(5)
    params0 = [rng.standard_normal(s) for s in SHAPES]
    n_steps = 8
    # step 2: an inf in group 0; step 5: a NaN in group 1's one-element tensor.  Never three clean steps in a row, so with
    # growth_interval 3 the scale only halves, twice (growth: test_restatement_growth_event_equals_gradscaler).  The torch arm's
    # gradients stay multiplied by 1024 while the scale moves; the restatement gets the same numbers and the live scale
    poison = {2: (1, np.inf), 5: (2, np.nan)} if scaling else {}
    grads = _grads(rng, n_steps, 1024.0 if scaling else None, poison)
    p, m, v = params0, [np.zeros(s) for s in SHAPES], [np.zeros(s) for s in SHAPES]
    steps, scale, tracker = [0] * len(HYPER), (1024.0 if scaling else None), 0
    grew = False
    for k, (ps, opts, norms, tscale) in enumerate(_torch_arm(params0, n_steps, grads, scaling)):
        r = OR.optim_step(p, grads[k], m, v, GROUP_OF, steps, HYPER, scale=scale, tracker=tracker, interval=3)
        grew |= scaling and r["scale"] > scale
        p, m, v, steps, scale, tracker = r["p"], r["m"], r["v"], r["steps"], r["scale"], r["tracker"]
        for i, q in enumerate(ps):
            np.testing.assert_allclose(p[i], q.detach().numpy(), err_msg=f"step {k} param {i}", **CLOSE)
            st = opts[GROUP_OF[i]].state.get(q, {})
            if st:
                np.testing.assert_allclose(m[i], st["exp_avg"].numpy(), err_msg=f"step {k} exp_avg {i}", **CLOSE)
                np.testing.assert_allclose(v[i], st["exp_avg_sq"].numpy(), err_msg=f"step {k} exp_avg_sq {i}", **CLOSE)
                assert int(st["step"]) == steps[GROUP_OF[i]], (k, i)
            else:
                assert not m[i].any() and not v[i].any()
            if q.grad is not None and not r["skipped"][GROUP_OF[i]]:
                np.testing.assert_allclose(r["g"][i], q.grad.numpy(), err_msg=f"step {k} grad {i}", **CLOSE)
        for gi, want in norms.items():
            if np.isfinite(want):
                np.testing.assert_allclose(r["norms"][gi], want, rtol=1e-12, atol=0, err_msg=f"step {k} norm {gi}")
            else:
                assert not np.isfinite(r["norms"][gi]) and r["found"][gi] == 1
        assert r["norms"][2] == 0.0 and not r["found"][2] and steps[2] == 0          # the empty group
        if scaling:
            assert scale == tscale, (k, scale, tscale)
            assert r["skipped"] == [k == 2, k == 5, True, False], (k, r["skipped"])
    if scaling:
        assert steps == [7, 7, 0, 8] and scale == 1024.0 * 0.5 * 0.5 and not grew
        # a growth event: three clean steps in a row
        s, t = 256.0, 0
        for want in ((256.0, 1), (256.0, 2), (512.0, 0)):
            s, t = OR.scale_update(s, t, False, interval=3)
            assert (s, t) == want
        assert OR.scale_update(512.0, 2, True, interval=3) == (256.0, 0)
    else:
        assert steps == [8, 8, 0, 8]
    assert HYPER[0]["max_norm"] / (r["norms"][0] + 1e-6) < 1 < HYPER[1]["max_norm"] / (r["norms"][1] + 1e-6)     # binding and slack


def test_restatement_growth_event_equals_gradscaler():
    """growth_interval=3 over seven clean steps and one skip: the scale doubles after steps 2 and 5, halves at step 6."""
    rng = np.random.default_rng(6)
    params0 = [rng.standard_normal(s) for s in SHAPES]
    grads = _grads(rng, 8, 1024.0, {6: (0, np.inf)})
    p, m, v = params0, [np.zeros(s) for s in SHAPES], [np.zeros(s) for s in SHAPES]
    steps, scale, tracker, seen = [0] * len(HYPER), 1024.0, 0, []
    for k, (ps, opts, norms, tscale) in enumerate(_torch_arm(params0, 8, grads, True)):
        # the torch arm's gradients were scaled by 1024 throughout; hand the restatement the same numbers and the live scale
        r = OR.optim_step(p, grads[k], m, v, GROUP_OF, steps, HYPER, scale=scale, tracker=tracker, interval=3)
        p, m, v, steps, scale, tracker = r["p"], r["m"], r["v"], r["steps"], r["scale"], r["tracker"]
        seen.append(scale)
        assert scale == tscale, (k, scale, tscale)
        for i, q in enumerate(ps):
            np.testing.assert_allclose(p[i], q.detach().numpy(), err_msg=f"step {k} param {i}", **CLOSE)
    assert seen == [1024.0, 1024.0, 2048.0, 2048.0, 2048.0, 4096.0, 2048.0, 2048.0]


@pytest.mark.parametrize("pos_weight", [1.0, 3.7])
def test_restatement_bce_equals_torch_in_float64(pos_weight):
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.standard_normal(61) * 3, [0.0, 100.0, -100.0, 100.0, -100.0]])
    y = np.concatenate([(rng.random(61) < 0.4).astype(np.float64), [1.0, 1.0, 0.0, 0.0, 1.0]])
    loss, d, correct = OR.bce(x, y, pos_weight, scale=1024.0)
    xt = torch.tensor(x, requires_grad=True)
    want = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pos_weight], dtype=torch.float64))(xt, torch.tensor(y))
    (want * 1024.0).backward()
    assert np.isfinite(loss)
    np.testing.assert_allclose(loss, float(want.detach()), **CLOSE)
    np.testing.assert_allclose(d, xt.grad.numpy(), rtol=0, atol=1e-12 * 1024)
    assert correct == int(((xt.detach() > 0).double() == torch.tensor(y)).sum())


# ---- the C ABI's refusals ----------------------------------------------------------------------------------------------
FAKE = 0x1000


def _i64(*v):
    return (C.c_int64 * len(v))(*v)


def test_optim_workspace_bytes():
    f = _lib.load().radad_optim_workspace_bytes
    assert f(None, 0) > 0
    assert f(_i64(0), 1) == f(None, 0)
    sizes = [f(_i64(n), 1) for n in (1, 4096, 4097, 10 ** 6, 10 ** 9)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]                  # monotone in numel
    many = [f(_i64(*([5000] * n)), n) for n in (1, 2, 17, 64)]
    assert all(a <= b for a, b in zip(many, many[1:])) and many[0] < many[-1]                      # and in the tensor count
    assert f(_i64(*([1] * 64)), 64) > 0
    for bad in ((_i64(*([1] * 65)), 65), (_i64(1), -1), (None, 1), (_i64(3, -1), 2), (_i64(1 << 62), 1)):
        assert f(*bad) < 0


def _optim_args(n_tensors=2, n_groups=2):
    ts = (_lib.OptimTensor * max(n_tensors, 1))()
    for i in range(n_tensors):
        ts[i].param = ts[i].grad = ts[i].exp_avg = ts[i].exp_avg_sq = FAKE
        ts[i].numel, ts[i].group = 5000, i % n_groups
    gs = (_lib.OptimGroup * max(n_groups, 1))()
    for g in gs:
        g.lr, g.beta1, g.beta2, g.eps, g.weight_decay, g.max_norm = 1e-3, 0.9, 0.999, 1e-8, 1e-5, 1.0
    st = _lib.OptimState()
    st.scale = st.growth_tracker = st.steps = st.grad_norm = st.found_inf = FAKE
    return ts, gs, st


def test_optim_step_argument_errors_without_gpu():
    lib = _lib.load()
    E = _lib.RADAD_EINVAL

    def call(ts, gs, st, n_tensors=2, n_groups=2, growth=2.0, backoff=0.5, interval=2000, ws=FAKE, ws_bytes=1 << 40):
        return lib.radad_optim_step(ts, n_tensors, gs, n_groups, None if st is None else C.byref(st), growth, backoff, interval, ws,
                                    ws_bytes, 0, None)

    def refused(needle, *a, **kw):
        assert call(*a, **kw) == E, needle
        assert needle in lib.radad_last_error(), lib.radad_last_error()

    ts, gs, st = _optim_args()
    refused(b"n_tensors", ts, gs, st, n_tensors=65)
    refused(b"n_tensors", ts, gs, st, n_tensors=-1)
    refused(b"n_groups", ts, gs, st, n_groups=0)
    refused(b"n_groups", ts, gs, st, n_groups=9)
    refused(b"NULL struct", None, gs, st)
    refused(b"NULL struct", ts, None, st)
    refused(b"NULL struct", ts, gs, None)
    for hole in ("steps", "grad_norm", "found_inf"):
        ts, gs, st = _optim_args()
        setattr(st, hole, None)
        refused(b"NULL state pointer", ts, gs, st)
    ts, gs, st = _optim_args()
    st.growth_tracker = None
    refused(b"half NULL", ts, gs, st)
    ts, gs, st = _optim_args()
    refused(b"loss scale needs", ts, gs, st, growth=0.5)
    refused(b"loss scale needs", ts, gs, st, backoff=0.0)
    refused(b"loss scale needs", ts, gs, st, interval=0)
    for field, value, needle in (("beta1", 1.0, b"betas"), ("beta1", -0.1, b"betas"), ("beta2", 1.5, b"betas"),
                                 ("beta2", float("nan"), b"betas"), ("eps", 0.0, b"eps"), ("eps", -1e-8, b"eps"),
                                 ("lr", -1e-3, b"lr"), ("weight_decay", -1.0, b"weight_decay"), ("max_norm", float("nan"), b"max_norm")):
        ts, gs, st = _optim_args()
        setattr(gs[1], field, value)
        refused(needle, ts, gs, st)
    ts, gs, st = _optim_args()
    ts[1].group = 2
    refused(b"group 2 outside", ts, gs, st)
    ts[1].group = -1
    refused(b"group -1 outside", ts, gs, st)
    ts, gs, st = _optim_args()
    ts[0].numel = -1
    refused(b"negative", ts, gs, st)
    for hole in ("param", "exp_avg", "exp_avg_sq"):
        ts, gs, st = _optim_args()
        setattr(ts[1], hole, None)
        refused(b"NULL param", ts, gs, st)
    ts, gs, st = _optim_args()
    refused(b"NULL workspace", ts, gs, st, ws=None)
    need = lib.radad_optim_workspace_bytes(_i64(5000, 5000), 2)
    refused(b"workspace too small", ts, gs, st, ws_bytes=need - 1)
    ts[1].grad = None          # a tensor without a gradient still counts towards the workspace
    refused(b"workspace too small", ts, gs, st, ws_bytes=need - 1)


def test_bce_logits_argument_errors_without_gpu():
    lib = _lib.load()
    E = _lib.RADAD_EINVAL

    def call(x=FAKE, y=FAKE, n=8, pw=1.0, scale=None, loss=FAKE, d=FAKE, correct=FAKE):
        return lib.radad_bce_logits(x, y, n, pw, scale, loss, d, correct, 0, None)

    for kw, needle in ((dict(n=0), b"at least 1"), (dict(n=-3), b"at least 1"), (dict(pw=0.0), b"pos_weight"),
                       (dict(pw=-2.0), b"pos_weight"), (dict(pw=float("nan")), b"pos_weight"), (dict(x=None), b"NULL buffer"),
                       (dict(y=None), b"NULL buffer"), (dict(loss=None), b"NULL buffer"), (dict(d=None), b"NULL buffer"),
                       (dict(correct=None), b"NULL buffer")):
        assert call(**kw) == E, kw
        assert needle in lib.radad_last_error(), lib.radad_last_error()


# ---- HipTrainStep's checks, all in front of the first raw pointer ------------------------------------------------------------
def _p(*shape, dtype=torch.float32, device="cpu"):
    return torch.nn.Parameter(torch.zeros(*shape, dtype=dtype, device=device), requires_grad=dtype.is_floating_point)


def test_hip_train_step_type_and_value_errors_without_gpu():
    mk = lambda groups, **kw: TS.HipTrainStep(groups, **{**dict(lr=1e-3, weight_decay=1e-5), **kw})
    with pytest.raises(TypeError, match="must be tensors"):
        mk([[_p(3), 4.0]])
    with pytest.raises(TypeError, match="float32"):
        mk([[_p(3, dtype=torch.float64)]])
    with pytest.raises(TypeError, match="float32"):
        mk([[_p(3, dtype=torch.bfloat16)]])
    with pytest.raises(ValueError, match="groups"):
        mk([])
    with pytest.raises(ValueError, match="groups"):
        mk([[_p(1)] for _ in range(9)])
    with pytest.raises(ValueError, match="65 tensors"):
        mk([[_p(1) for _ in range(65)]])
    shared = _p(2)
    with pytest.raises(ValueError, match="more than one group"):
        mk([[shared], [shared]])
    with pytest.raises(ValueError, match="contiguous"):
        mk([[torch.zeros(4, 6).t()]])
    with pytest.raises(ValueError, match="one device"):
        mk([[_p(2), _p(2, device="meta")]])
    with pytest.raises(ValueError, match="ROCm device"):
        mk([[_p(2)], []])
    for kw, needle in ((dict(lr=-1.0), "learning rate"), (dict(eps=0.0), "epsilon"), (dict(eps=1e-60), "epsilon"),
                       (dict(betas=(1.0, 0.999)), "index 0"), (dict(betas=(0.9, -0.1)), "index 1"),
                       (dict(weight_decay=-1e-5), "weight_decay"), (dict(pos_weight=0.0), "pos_weight"),
                       (dict(init_scale=0.0), "init_scale"), (dict(growth_factor=0.5), "growth_factor"),
                       (dict(backoff_factor=1.5), "backoff_factor"), (dict(growth_interval=0), "growth_interval"),
                       (dict(lr=[1e-3, 1e-3]), "2 values for 1 groups"), (dict(max_norm=float("nan")), "max_norm")):
        with pytest.raises(ValueError, match=needle):
            TS.check_hyper(1, **{**dict(lr=1e-3, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, pos_weight=1.0,
                                        init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000), **kw})
    h = TS.check_hyper(2, lr=[1e-3, 1e-2], weight_decay=0.0, betas=[(0.9, 0.999), (0.5, 0.9)], eps=1e-8, max_norm=None, pos_weight=2.0,
                       init_scale=1.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=1)
    assert h[1]["beta1"] == 0.5 and h[0]["beta2"] == float(np.float32(0.999)) and h[0]["max_norm"] == 0.0
    assert h[1]["lr"] == float(np.float32(1e-2))


def test_backward_and_step_checks_without_gpu():
    cpu, meta = torch.device("cpu"), torch.device("meta")
    x, y = torch.zeros(4), torch.zeros(4)
    TS.check_logits(x, y, cpu)
    TS.check_logits(x.view(4, 1), y, cpu)
    with pytest.raises(TypeError, match="float32"):
        TS.check_logits(x.double(), y, cpu)
    with pytest.raises(TypeError, match="float32"):
        TS.check_logits([0.0], y, cpu)
    with pytest.raises(TypeError, match="labels"):
        TS.check_logits(x, [0.0] * 4, cpu)
    with pytest.raises(ValueError, match="parameters on"):
        TS.check_logits(x, y, meta)
    with pytest.raises(ValueError, match="number of"):
        TS.check_logits(x, torch.zeros(5), cpu)
    with pytest.raises(ValueError, match="number of"):
        TS.check_logits(torch.zeros(0), torch.zeros(0), cpu)
    p = _p(3, 2)
    TS.check_grad(p, torch.zeros(3, 2), cpu)
    with pytest.raises(TypeError, match="float32"):
        TS.check_grad(p, torch.zeros(3, 2, dtype=torch.float16), cpu)
    with pytest.raises(ValueError, match="left"):
        TS.check_grad(p, torch.zeros(3, 2, device="meta"), cpu)
    with pytest.raises(ValueError, match="contiguous"):
        TS.check_grad(torch.zeros(2, 3).t(), torch.zeros(3, 2), cpu)
