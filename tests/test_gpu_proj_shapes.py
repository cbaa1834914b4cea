"""GPU: csrc/proj.hip (k_gemm_nt_splitk, k_proj_tail, k_fold_w54, k_fuse_head, k_splitk_finish) across shapes, against float64.

ProjectionLayer.forward, RADADModel.fuse_and_detect, radad_linear_forward and get_attention_weights at widths that are not
multiples of 4, hidden sizes whose [W1; W3] tiles straddle the two weights, K from 1 to 16, batches around the 128-row tile,
numerical edges (a saturated or shifted softmax, equal scores, all-zero neighbours, a nearly constant LayerNorm row, inputs
scaled by 1e-3 and 1e3), the LDS / hidden / head limits on both sides, strided and misaligned Linear operands.

Tolerance: every output is compared with the oracle's float64 value at CERR x the error scale that oracle/radad_oracle.py's
error model gives any float32 evaluation of the same arithmetic (`*_err`; sums of |terms| formed in float64).  Where the
problem itself is ill-conditioned (the nearly constant LayerNorm row, the saturated softmax), torch's float32 CPU forward of
the same weights is measured against float64 too, and the kernel may be at most FP32_MUL times as far off, plus a floor of
16 ulps of the largest output.
"""
import ctypes as C
import time

import numpy as np
import pytest

from oracle import radad_oracle as O

pytestmark = pytest.mark.gpu

CERR = 3.0
FP32_MUL = 8.0
LDS_FLOATS = 160 * 1024 // 4          # the tail's LDS budget in floats (proj.hip raise_lds)


@pytest.fixture(scope="module", autouse=True)
def _report(request):
    t0 = time.time()
    yield
    line = f"test_gpu_proj_shapes: {sum(1 for it in request.session.items if it.module is request.module)} cases in " \
           f"{time.time() - t0:.1f} s"

    class _Summary:     # printed in pytest's terminal summary at the end of the session
        @staticmethod
        def pytest_terminal_summary(terminalreporter):
            terminalreporter.write_line(line)
    request.config.pluginmanager.register(_Summary(), "proj_shapes_report")


def _check(case, got, want, err):
    """|got - want| <= CERR * err elementwise; the message names the case and the worst element."""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{case}: shape {got.shape} != {want.shape}"
    tol = CERR * np.broadcast_to(err, want.shape)
    diff = np.abs(got - want)
    ok = diff <= tol
    if not ok.all():
        ratio = np.where(np.isfinite(diff), diff / np.maximum(tol, 1e-300), np.inf)
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        pytest.fail(f"{case}: {int((~ok).sum())} of {ok.size} outside {CERR} x the float32 error scale; worst at {i}: "
                    f"got {got[i]!r} want {want[i]!r} |diff| {diff[i]:.3e} scale {tol[i] / CERR:.3e}")


def _check_vs_fp32(case, got, want, fp32):
    """Ill-conditioned edges: the kernel is at most FP32_MUL times as far from float64 as torch's float32 CPU forward."""
    e_gpu = float(np.abs(np.asarray(got, np.float64) - want).max())
    e_32 = float(np.abs(fp32 - want).max())
    floor = 16 * 2.0 ** -24 * float(np.abs(want).max())
    assert np.isfinite(e_gpu) and e_gpu <= FP32_MUL * e_32 + floor, \
        f"{case}: kernel error {e_gpu:.3e} > {FP32_MUL} x float32 CPU error {e_32:.3e} + floor {floor:.3e}"


def _proj_params(D, H, Oo, seed, bias=0.3):
    """nn.Linear weights ~ N(0, 1/fan_in), biases ~ N(0, bias^2), LayerNorm gain 1 + N(0, 0.01)."""
    rng = np.random.default_rng(seed)
    w = lambda o, i: (rng.standard_normal((o, i)) / np.sqrt(i)).astype(np.float32)
    b = lambda n, s=bias: (s * rng.standard_normal(n)).astype(np.float32)
    return {"attention_score.weight": w(H, D), "attention_score.bias": b(H), "attention_final.weight": w(1, H),
            "attention_final.bias": b(1), "cst_hidden.weight": w(H, D), "cst_hidden.bias": b(H), "cst_output.weight": w(D, H),
            "cst_output.bias": b(D), "weight_sum.weight": w(H, D), "weight_sum.bias": b(H),
            "normalization.weight": (1 + b(H, 0.1)).astype(np.float32), "normalization.bias": b(H, 0.1),
            "unified_embedding.weight": w(Oo, H), "unified_embedding.bias": b(Oo)}


def _layer(gpu, D, H, Oo, sd):
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, projection_hidden_dim=H, projection_output_dim=Oo)
    layer = R.ProjectionLayer(cfg, D).eval()
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return layer


def _run(layer, x, gpu):
    import torch
    with torch.no_grad():
        return layer(torch.from_numpy(np.ascontiguousarray(x)).to(gpu)).cpu().numpy()


def _fp32_forward(x, p):
    """The reference's arithmetic (projection.py:68-106, unfused order) in torch float32 on the CPU."""
    import torch
    T = {k: torch.from_numpy(v) for k, v in p.items()}
    lin = lambda a, n: a @ T[n + ".weight"].T + T[n + ".bias"]
    xt = torch.from_numpy(np.ascontiguousarray(x))
    s = lin(torch.tanh(lin(xt, "attention_score")), "attention_final")
    c = lin(torch.relu(lin(xt, "cst_hidden")), "cst_output")
    u = (torch.softmax(s, dim=1) * c).sum(dim=1)
    y = lin(u, "weight_sum")
    z = torch.nn.functional.layer_norm(y, (y.shape[1],), T["normalization.weight"], T["normalization.bias"], 1e-6)
    return lin(z, "unified_embedding").double().numpy()


# ---- ProjectionLayer.forward: a bounded, seeded draw from the shape cross product ------------------------------------------
SWEEP_D = [1, 3, 4, 90, 100, 128, 132, 448, 5375, 5376]
SWEEP_H = [4, 100, 128, 130, 256, 300, 1024]
SWEEP_O = [1, 64, 129]
SWEEP_K = [1, 2, 5, 15, 16]
SWEEP_B = [1, 2, 127, 128, 129, 1000]
WORK_CAP = 1.5e8        # B*K*D*H of one case: keeps the float64 oracle to a fraction of a second


def _sweep_cases(n=35, seed=20261016):
    """35 drawn cases and two named wide ones.  D cycles with period 10 and H with period 7, so 35 cases meet every D and every H (and 35 distinct (D, H) pairs); O and
    K cycle too; B is drawn, then lowered to the largest value of SWEEP_B that keeps B*K*D*H under WORK_CAP (K too if needed)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        D, H, Oo, K = SWEEP_D[i % 10], SWEEP_H[i % 7], SWEEP_O[i % 3], SWEEP_K[i % 5]
        B = int(rng.choice(SWEEP_B))
        while K > 1 and D * H * K > WORK_CAP:
            K = SWEEP_K[SWEEP_K.index(K) - 1]
        fits = [b for b in SWEEP_B if b * K * D * H <= WORK_CAP]
        B = B if B in fits else max(fits)
        out.append((D, H, Oo, K, B, 1000 + i))
    # the store width of the reference's 5376-wide pyramid against the widest hidden layer: many K-splits, 16 column tiles
    return out + [(5376, 1024, 129, 5, 2, 1100), (5375, 1024, 64, 16, 1, 1101)]


@pytest.mark.parametrize("D,H,Oo,K,B,seed", _sweep_cases())
def test_projection_forward_sweep(gpu, D, H, Oo, K, B, seed):
    sd = _proj_params(D, H, Oo, seed)
    x = np.random.default_rng(seed + 1).standard_normal((B, K, D)).astype(np.float32)
    want, err = O.projection_forward_err(x, sd)
    _check(f"projection D={D} H={H} O={Oo} K={K} B={B} seed={seed}", _run(_layer(gpu, D, H, Oo, sd), x, gpu), want, err)


def test_projection_sweep_covers_every_value():
    cases = _sweep_cases()
    for i, vals in enumerate((SWEEP_D, SWEEP_H, SWEEP_O, SWEEP_K)):
        assert {c[i] for c in cases} == set(vals)
    assert {c[4] for c in cases} == set(SWEEP_B)
    assert any(c[0] > 5000 and c[1] == 1024 for c in cases)              # many K-splits against a wide hidden layer


def test_projection_empty_batch(gpu):
    sd = _proj_params(90, 100, 129, 5)
    y = _run(_layer(gpu, 90, 100, 129, sd), np.zeros((0, 5, 90), np.float32), gpu)
    assert y.shape == (0, 129)


# ---- numerical edges --------------------------------------------------------------------------------------------------------
EDGE_SHAPE = (448, 130, 64, 5, 64)      # D, H, O, K, B: H = 130 straddles the W1 / W3 tile boundary


def _edge(name, seed=77):
    D, H, Oo, K, B = EDGE_SHAPE
    sd = _proj_params(D, H, Oo, seed)
    x = np.random.default_rng(seed + 1).standard_normal((B, K, D)).astype(np.float32)
    if name == "saturated_softmax":         # scores spread by ~50 and all shifted by 120: exp(s) alone would overflow float32
        sd["attention_final.weight"] = (sd["attention_final.weight"] * np.float32(50)).astype(np.float32)
        sd["attention_final.bias"] = np.asarray([120.0], np.float32)
    elif name == "equal_scores":            # K identical neighbour rows: every weight is exactly 1/K
        x[:] = x[:, :1, :]
    elif name == "zero_rows":               # what predict() passes for an empty store
        x[:] = 0
    elif name == "flat_layernorm":          # W5 ~ 0, constant b5: the row's variance is of the order of eps
        sd["weight_sum.weight"] = (sd["weight_sum.weight"] * np.float32(2e-3)).astype(np.float32)
        sd["weight_sum.bias"] = np.full(H, 4.0, np.float32)
    elif name == "x_small":
        x *= np.float32(1e-3)
    elif name == "x_large":
        x *= np.float32(1e3)
    return sd, x


@pytest.mark.parametrize("name", ["saturated_softmax", "equal_scores", "zero_rows", "flat_layernorm", "x_small", "x_large"])
def test_projection_numerical_edges(gpu, name):
    D, H, Oo, K, B = EDGE_SHAPE
    sd, x = _edge(name)
    got = _run(_layer(gpu, D, H, Oo, sd), x, gpu)
    want, err = O.projection_forward_err(x, sd)
    case = f"edge {name} D={D} H={H} O={Oo} K={K} B={B}"
    _check(case, got, want, err)
    if name == "saturated_softmax":
        a = O.attention_weights(x, sd)[:, :, 0]
        assert np.median(a.max(axis=1)) > 0.999, "the softmax is not saturated"
        _check_vs_fp32(case, got, want, _fp32_forward(x, sd))
    elif name == "flat_layernorm":
        f = lambda v: np.asarray(v, np.float64)
        c = np.maximum(f(x) @ f(sd["cst_hidden.weight"]).T + sd["cst_hidden.bias"], 0) @ f(sd["cst_output.weight"]).T \
            + sd["cst_output.bias"]
        ratio = np.median((f(c).mean(axis=1) @ f(sd["weight_sum.weight"]).T).var(axis=1) / 1e-6)
        assert 0.1 < ratio < 10, f"row variance / eps = {ratio}: not the regime this edge is for"
        _check_vs_fp32(case, got, want, _fp32_forward(x, sd))


# ---- limits: LDS of the tail, hidden <= 4096 ------------------------------------------------------------------------------
def _max_hidden(K):
    """Largest hidden whose tail fits: 2*K*H + 2*H + K + 8 floats <= 160 KB (proj.hip radad_projection_forward)."""
    return (LDS_FLOATS - 8 - K) // (2 * K + 2)


@pytest.mark.parametrize("K", [16, 5])
def test_projection_lds_boundary(gpu, K):
    D, Oo, B = 7, 3, 3
    H = _max_hidden(K)
    assert 2 * K * H + 2 * H + K + 8 <= LDS_FLOATS < 2 * K * (H + 1) + 2 * (H + 1) + K + 8
    sd = _proj_params(D, H, Oo, 91)
    x = np.random.default_rng(92).standard_normal((B, K, D)).astype(np.float32)
    want, err = O.projection_forward_err(x, sd)
    _check(f"LDS boundary K={K} H={H}", _run(_layer(gpu, D, H, Oo, sd), x, gpu), want, err)
    sd = _proj_params(D, H + 1, Oo, 93)
    with pytest.raises(ValueError, match="160 KB LDS"):
        _run(_layer(gpu, D, H + 1, Oo, sd), x, gpu)


def test_projection_hidden_limit(gpu):
    D, Oo, K, B = 5, 2, 1, 2
    sd = _proj_params(D, 4096, Oo, 95)
    x = np.random.default_rng(96).standard_normal((B, K, D)).astype(np.float32)
    want, err = O.projection_forward_err(x, sd)
    _check("hidden 4096", _run(_layer(gpu, D, 4096, Oo, sd), x, gpu), want, err)
    sd = _proj_params(D, 4097, Oo, 97)
    with pytest.raises(ValueError, match="hidden 4097 above 4096"):
        _run(_layer(gpu, D, 4097, Oo, sd), x, gpu)


# ---- get_attention_weights --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H,K,B", [(90, 4, 1, 3), (5375, 100, 2, 9), (132, 128, 5, 129), (448, 130, 15, 40), (3, 256, 16, 7),
                                     (100, 300, 5, 20), (1, 1024, 16, 5), (33, 99, 5, 11), (210, 30, 15, 6)])
def test_attention_weights(gpu, D, H, K, B):
    """projection.py:125-130 through radad_linear_forward, including hidden sizes that are not multiples of 4."""
    import torch
    sd = _proj_params(D, H, 3, 500 + H)
    x = np.random.default_rng(501 + D).standard_normal((B, K, D)).astype(np.float32)
    with torch.no_grad():
        got = _layer(gpu, D, H, 3, sd).get_attention_weights(torch.from_numpy(x).to(gpu)).cpu().numpy()
    want, err = O.attention_weights_err(x, sd)
    _check(f"attention weights D={D} H={H} K={K} B={B}", got, want, err)


# ---- RADADModel.fuse_and_detect --------------------------------------------------------------------------------------------
def _model(gpu, D, P, dims, bn, seed):
    """RADADModel with seeded weights (projection hidden 8: fuse_and_detect does not use it) and, with BatchNorm, running
    statistics far from the identity: mean ~ N(0, 1), var log-uniform over [1e-4, 1e2]."""
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    cfg = R.Config()
    cfg.update(device=gpu, projection_hidden_dim=8, projection_output_dim=P, detection_hidden_dims=list(dims), use_batch_norm=bn)
    model = R.RADADModel(cfg, D).eval()
    rng = np.random.default_rng(seed)
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith("num_batches_tracked"):
            sd[k] = np.zeros(tuple(v.shape), np.int64)
        elif k.endswith("running_var"):
            sd[k] = (10.0 ** rng.uniform(-4, 2, tuple(v.shape))).astype(np.float32)
        elif k.endswith("running_mean"):
            sd[k] = rng.standard_normal(tuple(v.shape)).astype(np.float32)
        elif v.dim() == 2:
            sd[k] = (rng.standard_normal(tuple(v.shape)) * np.sqrt(2.0 / v.shape[1])).astype(np.float32)
        elif k.endswith("weight"):
            sd[k] = (1 + 0.1 * rng.standard_normal(tuple(v.shape))).astype(np.float32)
        else:
            sd[k] = (0.3 * rng.standard_normal(tuple(v.shape))).astype(np.float32)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model, sd


HEAD_CASES = [   # D, P, detection_hidden_dims, use_batch_norm, B
    (210, 128, [], True, 37),
    (210, 130, [64, 32], True, 130),
    (3584, 1, [64, 32], True, 5),
    (5376, 130, [300, 7, 33], True, 9),
    (210, 130, [300, 7, 33], False, 129),
    (3584, 128, [50, 40, 30, 20, 10], True, 33),
    (210, 1, [50, 40, 30, 20, 10], False, 3),
    (5376, 128, [8192], True, 4),
    (3584, 130, [8192], False, 2),
    (210, 130, [64, 32], False, 1000),
]


@pytest.mark.parametrize("D,P,dims,bn,B", HEAD_CASES)
def test_fuse_and_detect(gpu, D, P, dims, bn, B):
    import torch
    model, sd = _model(gpu, D, P, dims, bn, 700 + D + P + len(dims))
    rng = np.random.default_rng(800 + B)
    t = rng.standard_normal((B, D)).astype(np.float32)
    pr = rng.standard_normal((B, P)).astype(np.float32)
    with torch.no_grad():
        logits, fused = model.fuse_and_detect(torch.from_numpy(t).to(gpu), torch.from_numpy(pr).to(gpu), return_fused=True)
    wf, ef, wl, el = O.head_forward_err(t, pr, sd)
    case = f"head D={D} P={P} dims={dims} bn={bn} B={B}"
    _check(case + " fused", fused.cpu().numpy(), wf, ef)
    _check(case + " logits", logits.cpu().numpy(), wl[:, 0], el[:, 0])
    assert logits.shape == (B,)


def test_head_limits(gpu):
    """Seven Linear layers and a width above 8192 raise ValueError; so does a raw call with n_layers = 7, or with
    n_layers = 0 and no fused output."""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    with pytest.raises(ValueError, match="at most 6 Linear layers"):
        _model(gpu, 30, 8, [9, 9, 9, 9, 9, 9], True, 1)
    model, _ = _model(gpu, 30, 8, [8193], True, 2)
    gen = torch.Generator().manual_seed(3)
    t, pr = torch.randn(2, 30, generator=gen).to(gpu), torch.randn(2, 8, generator=gen).to(gpu)
    with pytest.raises(ValueError, match="wider than 8192"):
        model.fuse_and_detect(t, pr)
    lib = _lib.load()
    w = _lib.HeadWeights()
    w.wf, w.bf = model.fuse.weight.data_ptr(), model.fuse.bias.data_ptr()
    ws = torch.empty(int(lib.radad_fuse_head_workspace_bytes(2, 30, 8)), dtype=torch.uint8, device=gpu)
    out = torch.empty(2, 8, device=gpu)

    def call(fused, logits):
        _lib.check(lib.radad_fuse_head_forward(C.byref(w), t.data_ptr(), pr.data_ptr(), 2, 30, 8, fused, logits, ws.data_ptr(),
                                               int(ws.numel()), gpu.index or 0, _lib.stream_ptr(gpu)), "fuse_head")
    w.n_layers = 7
    with pytest.raises(ValueError, match="too many head layers"):
        call(out.data_ptr(), out.data_ptr())
    w.n_layers = 0
    with pytest.raises(ValueError, match="no output buffer"):
        call(None, out.data_ptr())
    call(out.data_ptr(), None)                                   # n_layers = 0: the fused Linear alone, into fused_out
    wf, ef, _, _ = O.head_forward_err(t.cpu().numpy(), pr.cpu().numpy(),
                                      {"fuse.weight": model.fuse.weight.detach().cpu().numpy(),
                                       "fuse.bias": model.fuse.bias.detach().cpu().numpy()})
    _check("head n_layers=0", out.cpu().numpy(), wf, ef)


# ---- radad_linear_forward ---------------------------------------------------------------------------------------------------
LIN_IN = [1, 3, 31, 32, 33, 127, 129, 5375]


def _linear_cases():
    """every in_features x every activation; strides, a NULL bias and misaligned base pointers rotate through them"""
    out = []
    for i, n_in in enumerate(LIN_IN):
        for act in (0, 1, 2):
            j = 3 * i + act
            out.append((n_in, act, j % 2 == 1, j % 4 == 3, ("x", "w", "none")[j % 3]))
    return out


@pytest.mark.parametrize("n_in,act,strided,no_bias,misalign", _linear_cases())
def test_linear_forward(gpu, n_in, act, strided, no_bias, misalign):
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    lib = _lib.load()
    rows, n_out = 37 if n_in < 5000 else 3, 70
    ldx, ldw, ldo = (n_in + 3, n_in + 5, n_out + 2) if strided else (n_in, n_in, n_out)
    rng = np.random.default_rng(n_in * 3 + act)
    xs = rng.standard_normal((rows, ldx)).astype(np.float32)
    ws = (rng.standard_normal((n_out, ldw)) / np.sqrt(n_in)).astype(np.float32)
    b = (0.3 * rng.standard_normal(n_out)).astype(np.float32)
    # a misaligned operand lives one float into its buffer: base pointer 4 (mod 16) bytes
    xb = torch.from_numpy(np.concatenate([[0], xs.ravel()]).astype(np.float32)).to(gpu)
    wb = torch.from_numpy(np.concatenate([[0], ws.ravel()]).astype(np.float32)).to(gpu)
    xd = xb[1:] if misalign == "x" else xb[1:].clone()
    wd = wb[1:] if misalign == "w" else wb[1:].clone()
    assert (xd.data_ptr() % 16 == 4) == (misalign == "x") and (wd.data_ptr() % 16 == 4) == (misalign == "w")
    bd = torch.from_numpy(b).to(gpu)
    out = torch.full((rows, ldo), 7.0, device=gpu)
    need = lib.radad_linear_workspace_bytes(rows, n_out, n_in)
    wsp = torch.empty(int(need), dtype=torch.uint8, device=gpu)
    _lib.check(lib.radad_linear_forward(xd.data_ptr(), ldx, wd.data_ptr(), ldw, None if no_bias else bd.data_ptr(), act, rows,
                                        n_out, n_in, out.data_ptr(), ldo, wsp.data_ptr(), int(wsp.numel()), gpu.index or 0,
                                        _lib.stream_ptr(gpu)), "radad_linear_forward")
    got = out.cpu().numpy()
    want, err = O.linear_forward_err(xs[:, :n_in], ws[:, :n_in], None if no_bias else b, act)
    _check(f"linear in={n_in} act={act} ldx={ldx} ldw={ldw} ldo={ldo} bias={not no_bias} misaligned={misalign}",
           got[:, :n_out], want, err)
    assert (got[:, n_out:] == 7.0).all(), "wrote past out_features into the ldo padding"
    with pytest.raises(ValueError, match="row strides"):
        _lib.check(lib.radad_linear_forward(xd.data_ptr(), n_in - 1, wd.data_ptr(), ldw, bd.data_ptr(), act, rows, n_out, n_in,
                                            out.data_ptr(), ldo, wsp.data_ptr(), int(wsp.numel()), gpu.index or 0,
                                            _lib.stream_ptr(gpu)), "radad_linear_forward")


def test_row_count_limits(gpu):
    """batch * k (projection), rows (Linear) and batch (head) at 2^31 - 128 are refused before anything is read or launched."""
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import _lib
    lib = _lib.load()
    big = (1 << 31) - 128
    pw, hw = _lib.ProjWeights(), _lib.HeadWeights()
    with pytest.raises(ValueError, match="batch\\*k too large"):
        _lib.check(lib.radad_projection_forward(C.byref(pw), None, big // 4, 4, 8, 8, 2, None, None, 0, gpu.index or 0, None), "p")
    with pytest.raises(ValueError, match="bad shape"):
        _lib.check(lib.radad_linear_forward(None, 8, None, 8, None, 0, big, 4, 8, None, 4, None, 0, gpu.index or 0, None), "l")
    with pytest.raises(ValueError, match="bad shape"):
        _lib.check(lib.radad_fuse_head_forward(C.byref(hw), None, None, big, 8, 8, None, None, None, 0, gpu.index or 0, None), "h")
