"""GPU: the training step behind the backward (csrc/optim_step.inc, train_step.HipTrainStep) against tests/optim_step_ref.py.

The error bar is the training tests' own.  For a compared array (per group: every param, gradient left behind, exp_avg,
exp_avg_sq of the group taken together; the gradient of the logits)
    err = max|got - f64| / max|f64|          f64 = tests/optim_step_ref.py in float64 on the CPU
and the HIP path's err may be at most FACTOR = 4 times the err of torch's own float32 path on the same device and the same
inputs: Adam(foreach=False), clip_grad_norm_ and BCEWithLogitsLoss.  Both arms start every step from the same float32 state (the
float64 trajectory rounded) and get the same pre-generated gradients, so nothing diverges by trajectory.  Where torch's result is
exact (err 0) the bound is FLOOR = 2^-23, one float32 ulp of the largest value: a float64 result rounded once is within half of it.
A quantity that is ONE number per case (a group's norm, the loss) has no maximum over elements to steady it -- torch's one
rounding error is as likely 1e-9 as 1e-7 -- so for those the two errs are each the largest over all cases of the test, and the
same factor applies to that pair.  Nothing is ever bounded against the HIP result itself.
Hyperparameters travel to the kernels as float32; all three arms get the float32 values (HipTrainStep.hyper).
Every measured pair is printed before it is asserted (run with -s).  CHUNK is OPTIM_CHUNK of csrc/optim_step.inc.
Every test here fails without the feature: there is no train_step module.
"""
import numpy as np
import pytest

import optim_step_ref as OR

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FLOOR = 2.0 ** -23
CHUNK = 4096
F32 = np.float32


def _f32(v):
    return float(np.float32(v))


def _hyper(lr, b1, b2, eps, wd, mx):
    return dict(lr=_f32(lr), beta1=_f32(b1), beta2=_f32(b2), eps=_f32(eps), weight_decay=_f32(wd), max_norm=_f32(mx))


# group 0: weight decay, clipping binds; group 1: one tensor, other lr / betas, no weight decay, clipping slack; group 2: empty
HYPER = [_hyper(1e-2, 0.9, 0.999, 1e-8, 1e-2, 0.5), _hyper(3e-3, 0.8, 0.99, 1e-6, 0.0, 1e4), _hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)]


def _table(n_tensors):
    """[(shape, group, kind)]: kind 'view' starts one float into its storage (4-byte aligned only), 'nograd' has .grad None."""
    t = [((n,), 0, "") for n in (1, 3, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1)]
    t += [((37, 19), 0, ""), ((CHUNK + 3,), 0, "view"), ((10,), 0, "nograd"), ((2 * CHUNK + 5,), 1, "")]
    t += [((5,), 0, "")] * (n_tensors - len(t))
    assert len(t) == n_tensors
    return t


def _rel(got, want):
    """err over a list of arrays taken together."""
    num = max(float(np.abs(np.asarray(g, np.float64) - w).max()) for g, w in zip(got, want))
    den = max(float(np.abs(w).max()) for w in want)
    return num / (den if den > 0 else 1.0)


def _bound(torch_err):
    return FACTOR * torch_err if torch_err > 0 else FLOOR


def _make_params(torch, dev, table, values):
    ps = []
    for (shape, _, kind), a in zip(table, values):
        if kind == "view":
            buf = torch.zeros(a.size + 1, device=dev)
            p = buf[1:]
            assert p.data_ptr() % 16 == 4 and p.is_contiguous()
        else:
            p = torch.nn.Parameter(torch.zeros(shape, device=dev))
        with torch.no_grad():
            p.copy_(torch.from_numpy(a))
        ps.append(p)
    return ps


def _set_grads(torch, dev, table, ps, grads):
    for (shape, _, kind), p, g in zip(table, ps, grads):
        if g is None:
            p.grad = None
        elif kind == "view":
            buf = torch.zeros(g.size + 1, device=dev)
            buf[1:] = torch.from_numpy(g)
            p.grad = buf[1:]
            assert p.grad.data_ptr() % 16 == 4
        else:
            p.grad = torch.from_numpy(g).to(dev)


def _hip_stepper(torch, dev, table, hyper, scale, interval=2000):
    """HipTrainStep over fresh tensors of the table; returns (object, params, set_state)."""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.train_step import HipTrainStep
    ps = _make_params(torch, dev, table, [np.zeros(s, F32) for s, _, _ in table])
    groups = [[p for p, (_, g, _) in zip(ps, table) if g == gi] for gi in range(len(hyper))]
    hs = HipTrainStep(groups, lr=[h["lr"] for h in hyper], weight_decay=[h["weight_decay"] for h in hyper],
                      betas=[(h["beta1"], h["beta2"]) for h in hyper], eps=[h["eps"] for h in hyper],
                      max_norm=[h["max_norm"] for h in hyper], init_scale=scale or 1.0, growth_interval=interval,
                      loss_scaling=scale is not None)
    assert hs.hyper == hyper
    order = [i for gi in range(len(hyper)) for i, (_, g, _) in enumerate(table) if g == gi]      # state_dict's order

    def set_state(p, m, v, steps, scale_now, tracker):
        with torch.no_grad():
            for q, a in zip(ps, p):
                q.copy_(torch.from_numpy(a))
        per_group = lambda arrs: [[torch.from_numpy(arrs[i]) for i in order if table[i][1] == gi] for gi in range(len(hyper))]
        hs.load_state_dict(dict(exp_avg=per_group(m), exp_avg_sq=per_group(v), steps=torch.tensor(steps),
                                scale=torch.tensor(scale_now if scale_now is not None else 1.0), growth_tracker=torch.tensor(tracker)))

    def get_state():
        flat = lambda gs: [t for g in gs for t in g]
        m, v = [None] * len(ps), [None] * len(ps)
        for i, a, b in zip(order, flat(hs.exp_avg), flat(hs.exp_avg_sq)):
            m[i], v[i] = a.cpu().numpy().copy(), b.cpu().numpy().copy()
        return ([q.detach().cpu().numpy().copy() for q in ps], m, v,
                [None if q.grad is None else q.grad.cpu().numpy().copy() for q in ps])

    return hs, ps, set_state, get_state


def _torch_step(torch, dev, table, hyper, p, m, v, steps, grads, inv_scale, groups):
    """torch's float32 tail on the device for the given groups from the given state: (p, m, v, g, norms)."""
    ps = [torch.nn.Parameter(torch.from_numpy(a).to(dev)) for a in p]
    norms = {}
    for gi in groups:
        h = hyper[gi]
        mine = [i for i, (_, g, _) in enumerate(table) if g == gi]
        if not mine:
            continue
        opt = torch.optim.Adam([ps[i] for i in mine], lr=h["lr"], betas=(h["beta1"], h["beta2"]), eps=h["eps"],
                               weight_decay=h["weight_decay"], foreach=False)
        for i in mine:
            if grads[i] is None:
                continue
            ps[i].grad = torch.from_numpy(grads[i]).to(dev) * inv_scale
            opt.state[ps[i]] = dict(step=torch.tensor(float(steps[gi])), exp_avg=torch.from_numpy(m[i]).to(dev),
                                    exp_avg_sq=torch.from_numpy(v[i]).to(dev))
        norms[gi] = float(torch.nn.utils.clip_grad_norm_([ps[i] for i in mine], max_norm=h["max_norm"], foreach=False))
        opt.step()
        for i in mine:
            if grads[i] is not None:
                m[i], v[i] = opt.state[ps[i]]["exp_avg"].cpu().numpy(), opt.state[ps[i]]["exp_avg_sq"].cpu().numpy()
    return ([q.detach().cpu().numpy() for q in ps], m, v, [None if q.grad is None else q.grad.cpu().numpy() for q in ps], norms)


def _trajectory(n_tensors, n_steps, seed, scale=None):
    """The float64 run: per step the float32 start state, the (scaled) float32 gradients and optim_step_ref's result."""
    table = _table(n_tensors)
    rng = np.random.default_rng(seed)
    group_of = [g for _, g, _ in table]
    p = [rng.standard_normal(s).astype(F32) for s, _, _ in table]
    m = [np.zeros(s, F32) for s, _, _ in table]
    v = [np.zeros(s, F32) for s, _, _ in table]
    steps, out = [0] * len(HYPER), []
    for _ in range(n_steps):
        # group 0's norm is about sqrt(13e3) * 0.05 = 6 > 0.5: the clip binds; group 1's stays under 1e4
        g = [None if kind == "nograd" else (0.05 * rng.standard_normal(s) * (scale or 1.0)).astype(F32) for s, _, kind in table]
        r = OR.optim_step(p, g, m, v, group_of, steps, HYPER, scale=scale)
        out.append(dict(p=p, m=m, v=v, steps=list(steps), g=g, ref=r))
        p, m, v = [[a.astype(F32) for a in r[k]] for k in ("p", "m", "v")]
        steps = r["steps"]
    assert out[0]["ref"]["coef"][0] < 1.0 and out[0]["ref"]["coef"][1] == 1.0
    return table, out


def _hip_run(torch, dev, table, traj, scale=None):
    hs, ps, set_state, get_state = _hip_stepper(torch, dev, table, HYPER, scale)
    res = []
    for st in traj:
        set_state(st["p"], st["m"], st["v"], st["steps"], scale, 0)
        _set_grads(torch, dev, table, ps, st["g"])
        hs.step()
        s = hs.stats()
        res.append(get_state() + (s,))
    return res


def _compare_steps(torch, dev, table, traj, hip, scale=None):
    """Prints and asserts every pair of the run; returns nothing."""
    live = [gi for gi in range(len(HYPER)) if any(g == gi for _, g, _ in table)]
    worst = {}
    norm_pair = [0.0, 0.0]
    for k, (st, (hp, hm, hv, hg, stats)) in enumerate(zip(traj, hip)):
        r = st["ref"]
        tp, tm, tv, tg, tnorm = _torch_step(torch, dev, table, HYPER, st["p"], [a.copy() for a in st["m"]], [a.copy() for a in st["v"]],
                                            st["steps"], st["g"], 1.0 / (scale or 1.0), live)
        for gi in live:
            idx = [i for i, (_, g, kind) in enumerate(table) if g == gi and kind != "nograd"]
            for name, got, tor, want in (("param", hp, tp, r["p"]), ("grad", hg, tg, r["g"]), ("exp_avg", hm, tm, r["m"]),
                                         ("exp_avg_sq", hv, tv, r["v"])):
                pick = lambda a: [a[i] for i in idx]
                eh, et = _rel(pick(got), pick(want)), _rel(pick(tor), pick(want))
                key = (gi, name)
                if key not in worst or eh / _bound(et) > worst[key][0] / _bound(worst[key][1]):
                    worst[key] = (eh, et, k)
                assert eh <= _bound(et), f"step {k} group {gi} {name}: hip {eh:.3e} torch {et:.3e}"
            norm_pair[0] = max(norm_pair[0], abs(stats["grad_norms"][gi] - r["norms"][gi]) / r["norms"][gi])
            norm_pair[1] = max(norm_pair[1], abs(tnorm[gi] - r["norms"][gi]) / r["norms"][gi])
        assert stats["steps"] == r["steps"] and stats["found_inf"] == [0] * len(HYPER)
        assert stats["grad_norms"][2] == 0.0                                              # the empty group
        for i, (_, _, kind) in enumerate(table):
            if kind == "nograd":      # no gradient: untouched
                assert np.array_equal(hp[i], st["p"][i]) and np.array_equal(hm[i], st["m"][i]) and np.array_equal(hv[i], st["v"][i])
    for (gi, name), (eh, et, k) in sorted(worst.items()):
        print(f"  group {gi} {name:10s} worst pair at step {k}: hip {eh:.3e}  torch f32 {et:.3e}  bound {_bound(et):.3e}")
    print(f"  grad norms over {len(traj)} steps: hip {norm_pair[0]:.3e}  torch f32 {norm_pair[1]:.3e}  bound {_bound(norm_pair[1]):.3e}")
    assert norm_pair[0] <= _bound(norm_pair[1])


@pytest.fixture(scope="module")
def run20(gpu):
    """The 20-step case, computed once: table, float64 trajectory, two HIP runs of it."""
    import torch
    table, traj = _trajectory(12, 20, seed=1)
    return table, traj, _hip_run(torch, gpu, table, traj), _hip_run(torch, gpu, table, traj)


@pytest.mark.parametrize("n_tensors,scale", [(12, None), (64, None), (12, 1024.0)], ids=["table12", "table64", "table12_scale1024"])
def test_one_step_against_float64(gpu, n_tensors, scale):
    import torch
    table, traj = _trajectory(n_tensors, 1, seed=n_tensors, scale=scale)
    hip = _hip_run(torch, gpu, table, traj, scale)
    _compare_steps(torch, gpu, table, traj, hip, scale)
    if scale:
        assert hip[0][4]["scale"] == scale and hip[0][4]["growth_tracker"] == 1


def test_twenty_steps_against_float64(gpu, run20):
    import torch
    table, traj, hip, _ = run20
    _compare_steps(torch, gpu, table, traj, hip)
    assert hip[-1][4]["steps"] == [20, 20, 0]


def test_two_runs_give_the_same_bits(gpu, run20):
    _, _, a, b = run20
    for k, (ra, rb) in enumerate(zip(a, b)):
        for xa, xb in zip(ra[:4], rb[:4]):
            for i, (u, w) in enumerate(zip(xa, xb)):
                assert (u is None and w is None) or np.array_equal(u.view(np.uint32), w.view(np.uint32)), (k, i)
        assert np.array_equal(np.array(ra[4]["grad_norms"], F32).view(np.uint32), np.array(rb[4]["grad_norms"], F32).view(np.uint32))
    import torch
    _, x, y = _bce_cases()[6]                      # n = 1000: several passes of the one workgroup
    la, da, _ = _bce_hip(torch, gpu, x, y, _f32(3.7), 1024.0)
    lb, db, _ = _bce_hip(torch, gpu, x, y, _f32(3.7), 1024.0)
    assert F32(la).view(np.uint32) == F32(lb).view(np.uint32) and np.array_equal(da.view(np.uint32), db.view(np.uint32))


# ---- skipping and the loss scale ---------------------------------------------------------------------------------------------
SKIP_TABLE = [((300,), 0, ""), ((2 * CHUNK + 5,), 0, ""), ((1,), 1, ""), ((CHUNK + 1,), 1, ""), ((513,), 2, ""), ((7, 9), 2, "")]
SKIP_HYPER = [_hyper(1e-2, 0.9, 0.999, 1e-8, 1e-2, 0.5), _hyper(3e-3, 0.8, 0.99, 1e-6, 0.0, 1.0), _hyper(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)]


def _skip_inputs(seed, scale, poison=True):
    rng = np.random.default_rng(seed)
    p = [rng.standard_normal(s).astype(F32) for s, _, _ in SKIP_TABLE]
    m = [(0.01 * rng.standard_normal(s)).astype(F32) for s, _, _ in SKIP_TABLE]
    v = [(1e-4 * rng.random(s)).astype(F32) for s, _, _ in SKIP_TABLE]
    g = [(0.05 * scale * rng.standard_normal(s)).astype(F32) for s, _, _ in SKIP_TABLE]
    if poison:
        g[1][-1] = np.inf          # the last element of the last chunk of group 0's largest tensor
        g[2][0] = np.nan           # group 1's one-element tensor
    return p, m, v, g


def test_a_group_with_a_non_finite_gradient_is_skipped_whole(gpu):
    import torch
    scale = 1024.0
    p, m, v, g = _skip_inputs(3, scale)
    steps = [4, 9, 2]
    hs, ps, set_state, get_state = _hip_stepper(torch, gpu, SKIP_TABLE, SKIP_HYPER, scale)
    set_state(p, m, v, steps, scale, 7)
    _set_grads(torch, gpu, SKIP_TABLE, ps, g)
    hs.step()
    hp, hm, hv, hg = get_state()
    s = hs.stats()
    r = OR.optim_step(p, g, m, v, [t[1] for t in SKIP_TABLE], steps, SKIP_HYPER, scale=scale, tracker=7)
    assert r["skipped"] == [True, True, False]
    for i in range(4):             # groups 0 and 1: bit-equal to before
        for got, was in ((hp, p), (hm, m), (hv, v)):
            assert np.array_equal(got[i].view(np.uint32), was[i].view(np.uint32)), i
    assert s["steps"] == [4, 9, 3] == r["steps"] and s["found_inf"] == [1, 1, 0]
    assert s["scale"] == 512.0 == r["scale"] and s["growth_tracker"] == 0 == r["tracker"]
    assert not np.isfinite(s["grad_norms"][0]) and not np.isfinite(s["grad_norms"][1])
    tp, tm, tv, tg, tnorm = _torch_step(torch, gpu, SKIP_TABLE, SKIP_HYPER, p, [a.copy() for a in m], [a.copy() for a in v], steps, g,
                                        1.0 / scale, [2])
    for name, got, tor, want in (("param", hp, tp, r["p"]), ("grad", hg, tg, r["g"]), ("exp_avg", hm, tm, r["m"]), ("exp_avg_sq", hv, tv, r["v"])):
        eh, et = _rel(got[4:], want[4:]), _rel(tor[4:], want[4:])
        print(f"  group 2 {name:10s}: hip {eh:.3e}  torch f32 {et:.3e}  bound {_bound(et):.3e}")
        assert eh <= _bound(et), name
    assert abs(s["grad_norms"][2] - r["norms"][2]) <= FLOOR * r["norms"][2]


def test_scale_grows_on_the_second_clean_step_and_not_after_a_skip(gpu):
    import torch
    scale = 1024.0
    hs, ps, set_state, _ = _hip_stepper(torch, gpu, SKIP_TABLE, SKIP_HYPER, scale, interval=2)
    p, m, v, _ = _skip_inputs(4, scale)
    set_state(p, m, v, [0, 0, 0], scale, 0)
    seen, want, tracker = [], [], 0
    s_ref = scale
    for k, poison in enumerate([False, False, True, False, False]):
        g = _skip_inputs(10 + k, 1.0, poison)[3]
        _set_grads(torch, gpu, SKIP_TABLE, ps, g)
        hs.step()
        st = hs.stats()
        seen.append((st["scale"], st["growth_tracker"]))
        s_ref, tracker = OR.scale_update(s_ref, tracker, poison, interval=2)
        want.append((s_ref, tracker))
    assert seen == want == [(1024.0, 1), (2048.0, 0), (1024.0, 0), (1024.0, 1), (2048.0, 0)]
    assert hs.stats()["steps"] == [4, 4, 5]


def test_without_a_scale_a_non_finite_gradient_spreads_as_in_torch(gpu):
    import torch
    p, m, v, g = _skip_inputs(5, 1.0)
    steps = [1, 1, 1]
    hs, ps, set_state, get_state = _hip_stepper(torch, gpu, SKIP_TABLE, SKIP_HYPER, None)
    set_state(p, m, v, steps, None, 0)
    _set_grads(torch, gpu, SKIP_TABLE, ps, g)
    hs.step()
    hp, hm, hv, hg = get_state()
    s = hs.stats()
    tp, tm, tv, tg, _ = _torch_step(torch, gpu, SKIP_TABLE, SKIP_HYPER, p, [a.copy() for a in m], [a.copy() for a in v], steps, g, 1.0,
                                    [0, 1, 2])
    assert s["steps"] == [2, 2, 2] and s["found_inf"] == [1, 1, 0] and s["scale"] == 1.0      # nothing skipped
    for name, got, tor in (("param", hp, tp), ("grad", hg, tg), ("exp_avg", hm, tm), ("exp_avg_sq", hv, tv)):
        for i in range(len(SKIP_TABLE)):
            assert np.array_equal(np.isnan(got[i]), np.isnan(tor[i])), (name, i)
            ok = ~np.isnan(tor[i])
            np.testing.assert_allclose(got[i][ok], tor[i][ok], rtol=1e-5, atol=1e-7, err_msg=f"{name} {i}")
    assert np.isnan(hp[2]).all() and np.isnan(hp[1][-1]) and np.isfinite(hp[4]).all()
    # group 0: an infinite norm clips every finite gradient to 0, the inf to NaN
    assert np.isnan(hg[1][-1]) and not hg[0].any() and not hg[1][:-1].any()


# ---- the loss ------------------------------------------------------------------------------------------------------------------
def _bce_hip(torch, dev, x, y, pw, scale):
    import ctypes as C
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    lib = _lib.load()
    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    st = torch.tensor([scale], device=dev, dtype=torch.float32) if scale is not None else None
    loss, d = torch.zeros(1, device=dev), torch.empty_like(xt)
    correct = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.check(lib.radad_bce_logits(xt.data_ptr(), yt.data_ptr(), x.size, pw, st.data_ptr() if st is not None else None, loss.data_ptr(),
                                    d.data_ptr(), correct.data_ptr(), 0, _lib.stream_ptr(dev)))
    return float(loss.item()), d.cpu().numpy(), int(correct.item())


def _bce_cases():
    rng = np.random.default_rng(11)
    cases = []
    for n in (1, 2, 63, 64, 65, 257, 1000):                    # 1000 > 256: more than one pass of the workgroup
        x = (3 * rng.standard_normal(n)).astype(F32)
        y = (rng.random(n) < 0.4).astype(F32)
        if n >= 63:
            x[:6] = [100, -100, 100, -100, 0, 0]
            y[:6] = [1, 0, 0, 1, 1, 0]
        cases.append((f"n{n}", x, y))
    x = (3 * rng.standard_normal(130)).astype(F32)
    cases += [("all0", x, np.zeros(130, F32)), ("all1", x, np.ones(130, F32))]
    return cases


def test_bce_logits_against_float64(gpu):
    import torch
    worst_loss = [0.0, 0.0]
    for name, x, y in _bce_cases():
        for pw in (1.0, 3.7):
            for scale in (None, 1.0, 1024.0):
                s = 1.0 if scale is None else scale
                pwf = _f32(pw)
                loss, d, correct = _bce_hip(torch, gpu, x, y, pwf, scale)
                rl, rd, rc = OR.bce(x, y, pwf, s)
                xt = torch.from_numpy(x).to(gpu).requires_grad_()
                tl = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([pwf], device=gpu))(xt, torch.from_numpy(y).to(gpu))
                (tl * s).backward()
                eh, et = _rel([d], [rd]), _rel([xt.grad.cpu().numpy()], [rd])
                lh, lt = abs(loss - rl) / abs(rl), abs(float(tl.detach()) - rl) / abs(rl)
                worst_loss = [max(worst_loss[0], lh), max(worst_loss[1], lt)]
                print(f"  {name:5s} pw {pw} scale {scale}: dlogits hip {eh:.3e} torch f32 {et:.3e} bound {_bound(et):.3e} | loss hip {lh:.3e} "
                      f"torch f32 {lt:.3e}")
                assert np.isfinite(loss) and correct == rc == int(((x > 0) == (y == 1)).sum())
                if x.size >= 63:
                    assert eh <= _bound(et), (name, pw, scale)
                if name.startswith("n") and x.size >= 63:
                    w = 1.0 + (pwf - 1.0)
                    near = lambda got, want: abs(got - want) <= FLOOR * abs(want)
                    assert d[0] == 0.0 and d[1] == 0.0                                   # saturated on the right side: exactly 0
                    assert near(d[2], s / x.size) and near(d[3], -s * w / x.size)        # on the wrong side: s w / n
                    assert near(d[4], -0.5 * s * w / x.size) and near(d[5], 0.5 * s / x.size)        # logit 0: predicted 0
                if x.size < 63:       # one or two numbers: the float32 format's own bar
                    assert eh <= FLOOR, (name, pw, scale)
    print(f"  loss over all cases: hip {worst_loss[0]:.3e}  torch f32 {worst_loss[1]:.3e}  bound {_bound(worst_loss[1]):.3e}")
    assert worst_loss[0] <= _bound(worst_loss[1])


# ---- through the public object -------------------------------------------------------------------------------------------------
def test_fold_cache_sees_the_step(gpu):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.train_step import HipTrainStep
    cfg = R.Config()
    cfg.update(device=gpu, projection_hidden_dim=32, projection_output_dim=16)
    torch.manual_seed(0)
    layer = R.ProjectionLayer(cfg, 64).eval()
    x = torch.randn(6, 3, 64, device=gpu)
    with torch.no_grad():
        before = layer(x).clone()
    hs = HipTrainStep([layer.parameters()], lr=1e-2, weight_decay=0.0, loss_scaling=False)
    for p in layer.parameters():
        p.grad = torch.randn_like(p)
    hs.step()
    with torch.no_grad():
        after = layer(x).clone()
    fresh = R.ProjectionLayer(cfg, 64).eval()
    fresh.load_state_dict(layer.state_dict())
    with torch.no_grad():
        want = fresh(x)
    assert not torch.equal(before, after)
    assert torch.equal(after, want)


def test_state_dict_round_trip_continues_bit_identically(gpu):
    import torch
    table, traj = _trajectory(12, 5, seed=9, scale=256.0)
    hs, ps, set_state, get_state = _hip_stepper(torch, gpu, table, HYPER, 256.0, interval=2)
    set_state(traj[0]["p"], traj[0]["m"], traj[0]["v"], [0, 0, 0], 256.0, 0)
    for st in traj[:3]:
        _set_grads(torch, gpu, table, ps, st["g"])
        hs.step()
    sd, p_mid = hs.state_dict(), [q.detach().cpu().numpy().copy() for q in ps]
    for st in traj[3:]:
        _set_grads(torch, gpu, table, ps, st["g"])
        hs.step()
    a, sa = get_state(), hs.stats()
    hs2, ps2, _, get2 = _hip_stepper(torch, gpu, table, HYPER, 256.0, interval=2)
    with torch.no_grad():
        for q, arr in zip(ps2, p_mid):
            q.copy_(torch.from_numpy(arr))
    hs2.load_state_dict(sd)
    for st in traj[3:]:
        _set_grads(torch, gpu, table, ps2, st["g"])
        hs2.step()
    b, sb = get2(), hs2.stats()
    assert sa == sb and sa["steps"] == [5, 5, 0] and sa["scale"] == 1024.0
    for xa, xb in zip(a[:3], b[:3]):
        for u, w in zip(xa, xb):
            assert np.array_equal(u.view(np.uint32), w.view(np.uint32))


def test_whole_model_five_steps(gpu):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd.train_step import HipTrainStep
    B, K, D = 8, 3, 64
    cfg = R.Config()
    cfg.update(device=gpu, projection_hidden_dim=32, projection_output_dim=16, detection_hidden_dims=[16, 8], projection_train_hip=True,
               head_train_hip=True)
    torch.manual_seed(2)
    model = R.RADADModel(cfg, D).train()
    hs = HipTrainStep.for_model(model, cfg, pos_weight=1.7)
    assert [h["lr"] for h in hs.hyper] == [_f32(1e-3)] * 3 and hs.hyper[0]["weight_decay"] == _f32(1e-5)
    flat = [(p, gi) for gi, g in enumerate(hs.groups) for p in g]
    table = [(tuple(p.shape), gi, "") for p, gi in flat]
    group_of = [gi for _, gi in flat]
    moments = lambda gs: [t.cpu().numpy().copy() for g in gs for t in g]
    worst, norm_pair = {}, [0.0, 0.0]
    for k in range(5):
        x, t = torch.randn(B, K, D, device=gpu), torch.randn(B, D, device=gpu)
        y = (torch.rand(B, device=gpu) < 0.5).float()
        logits = model(x, t)
        hs.zero_grad()
        loss, correct = hs.backward(logits, y)
        p0 = [p.detach().cpu().numpy().copy() for p, _ in flat]
        g0 = [p.grad.cpu().numpy().copy() for p, _ in flat]
        m0, v0, before = moments(hs.exp_avg), moments(hs.exp_avg_sq), hs.stats()
        hs.step()
        s = hs.stats()
        rl, _, rc = OR.bce(logits.detach().cpu().numpy(), y.cpu().numpy(), _f32(1.7))
        r = OR.optim_step(p0, g0, m0, v0, group_of, before["steps"], hs.hyper, scale=before["scale"], tracker=before["growth_tracker"])
        tp, _, _, _, tnorm = _torch_step(torch, gpu, table, hs.hyper, p0, m0, v0, before["steps"], g0, 1.0 / before["scale"], [0, 1, 2])
        assert s["correct"] == rc == int(correct.item()) and abs(s["loss"] - rl) <= FLOOR * abs(rl) and s["loss"] == float(loss.item())
        assert s["steps"] == [k + 1] * 3 == r["steps"] and s["found_inf"] == [0, 0, 0] and s["scale"] == 65536.0
        hp = [p.detach().cpu().numpy() for p, _ in flat]
        for gi in range(3):
            idx = [i for i, g in enumerate(group_of) if g == gi]
            eh, et = _rel([hp[i] for i in idx], [r["p"][i] for i in idx]), _rel([tp[i] for i in idx], [r["p"][i] for i in idx])
            if gi not in worst or eh / _bound(et) > worst[gi][0] / _bound(worst[gi][1]):
                worst[gi] = (eh, et, k)
            assert eh <= _bound(et), f"step {k} group {gi}: hip {eh:.3e} torch {et:.3e}"
            norm_pair[0] = max(norm_pair[0], abs(s["grad_norms"][gi] - r["norms"][gi]) / r["norms"][gi])
            norm_pair[1] = max(norm_pair[1], abs(tnorm[gi] - r["norms"][gi]) / r["norms"][gi])
    for gi, (eh, et, k) in sorted(worst.items()):
        print(f"  group {gi} params, worst pair at step {k}: hip {eh:.3e}  torch f32 {et:.3e}  bound {_bound(et):.3e}")
    print(f"  grad norms over 5 steps x 3 groups: hip {norm_pair[0]:.3e}  torch f32 {norm_pair[1]:.3e}  bound {_bound(norm_pair[1]):.3e}")
    assert norm_pair[0] <= _bound(norm_pair[1])
