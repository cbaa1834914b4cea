"""GPU: HipEvalMetrics (csrc/eval_metrics.inc) against tests/eval_metrics_ref.py on the same float32 scores.

Bounds, per include/radad_hip.h: pooled EER, its threshold, the ROC points and every group's EER (group_eers()) EQUAL the
model's; min t-DCF within 8 x 2^-53 relative (five roundings) at a threshold where the model's t-DCF
curve is within that bound of its minimum; AUC within 2^-52 relative of the exact-integer value; macro-EER within G x 2^-52
relative (summation order over G groups); correct / n / counts equal and the loss within (64 + n) x 2^-53 relative of the
exactly summed float64 model (a few ulp per log1p / exp term plus the summation of positive terms).

Sizes: 1, 2, 3; one below, at and above a thread's EVAL_ITEMS = 8, a workgroup's 256 and every merge-pass boundary
2048 x 2^p up to 65 536 (0 -> 1 ... 5 -> 6 passes: the finished sort changes buffers and the last run loses its partner); three
tiles (a run without a partner); 70 001 = 35 tiles, six passes with an odd run count at four of them.  A sort takes ceil(log2(tiles)) passes of one kernel, thirteen at the cap of 2^24 keys: test_every_merge_pass runs 2^23 + 9
keys (4097 tiles, thirteen passes) and, so that it stays quick, takes the model's counts per distinct score from torch.unique
on the device instead of numpy's sort of eight million doubles.  Batches are ragged (1, 7, 256, rest).
Every test here fails without the feature: the module and the symbols do not exist.
"""
import numpy as np
import pytest

import eval_metrics_ref as M

pytestmark = pytest.mark.gpu

ASV = M.ASV_2019
ASV_FALLING = dict(ASV, C_miss_cm=0.1)          # t-DCF falls with the miss rate: its minimum lies at the far end, at +inf or the last score
PW = float(np.float32(1.7))          # pos_weight travels as float32 (as the reference's pos_weight tensor is)
SIZES = [1, 2, 3, 7, 8, 9, 255, 256, 257, 6145, 70001]
SIZES += [(2048 << p) + d for p in range(6) for d in (-1, 0, 1)]          # every pass boundary up to 5 -> 6 passes: 2047 .. 65537
STORES = ["normal", "few_distinct", "all_equal", "signed_zero", "separable", "separable_flip3", "all_positive", "all_negative"]
GROUPINGS = ["none", "names", "giant_and_small", "one_class_groups", "one_group_with_both", "all_ids_equal"]


def make_scores(store, n, rng):
    y = (rng.random(n) < 0.4).astype(np.float32)
    if store == "normal":
        s = rng.standard_normal(n) * 3 + 1.5 * y
    elif store == "few_distinct":
        s = np.clip(np.rint(rng.standard_normal(n) * 1.5 + y), -3, 3)
    elif store == "all_equal":
        s = np.full(n, 0.75)
    elif store == "signed_zero":
        s = rng.choice(np.array([-1.0, -0.0, 0.0, 0.5]), n)
    elif store in ("separable", "separable_flip3"):
        s = np.where(y == 1, 1.0 + rng.random(n), -1.0 - rng.random(n))
        if store == "separable_flip3":
            flip = rng.choice(n, 3, replace=False)
            y[flip] = 1 - y[flip]
    elif store == "all_positive":
        s, y = rng.standard_normal(n), np.ones(n, dtype=np.float32)
    elif store == "all_negative":
        s, y = rng.standard_normal(n), np.zeros(n, dtype=np.float32)
    return s.astype(np.float32), y.astype(np.float32)


def make_groups(kind, n, y, rng):
    """(ids as the model sees them, what add() is given: None, a list of names per sample, or an int array)"""
    if kind == "none":
        return None, None
    if kind == "names":                                           # ids in order of first appearance, as the class assigns them
        raw = rng.integers(0, 23, n)
        first = {}
        ids = np.array([first.setdefault(int(v), len(first)) for v in raw], dtype=np.int32)
        return ids, [f"LA_{int(v):04d}" for v in raw]
    if kind == "giant_and_small":                                 # one group of half the samples, the rest in groups of 1-2
        ids = np.zeros(n, dtype=np.int32)
        m = n - n // 2
        ids[n // 2:] = 1 + np.arange(m) // 2
    elif kind == "one_class_groups":                              # no group holds both classes
        ids = (2 * rng.integers(0, 40, n) + (y == 1)).astype(np.int32)
    elif kind == "one_group_with_both":                           # macro-EER is then that group's EER
        ids = (2 * rng.integers(1, 40, n) + (y == 1)).astype(np.int32)
        ids[:max(n // 3, 2)] = 1
    elif kind == "all_ids_equal":
        ids = np.full(n, 5, dtype=np.int32)
    return ids[rng.permutation(n)] if kind == "giant_and_small" else ids, "ids"


def batches(n):
    cuts, at = [], 0
    for b in (1, 7, 256):
        if at + b < n:
            cuts.append((at, at + b))
            at += b
    return cuts + [(at, n)]


def feed(ev, gpu, s, y, ids, given, cuts=None):
    import torch
    xs, ys = torch.from_numpy(s).to(gpu), torch.from_numpy(y).to(gpu)
    for lo, hi in cuts or batches(len(s)):
        if given is None:
            sp = None
        elif isinstance(given, list):
            sp = given[lo:hi]
        else:
            sp = torch.from_numpy(ids[lo:hi]).to(gpu)
        ev.add(xs[lo:hi].view(-1, 1), ys[lo:hi].view(-1, 1), sp)


def same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def check(m, roc, s, y, ids, asv, label, geer=None):
    n = len(s)
    want = M.everything(s, y, ids, asv, PW)
    print(f"  {label}: n {n} eer {m['eer_percent']!r} thr {m['eer_threshold']!r} auc {m['auc']!r} (model {want['auc']!r}) macro "
          f"{m['macro_eer_percent']!r} (model {want['macro_eer_percent']!r}, {want['groups_scored']} groups) tdcf {m['min_tDCF']!r} "
          f"(model {want['min_tDCF']!r}) loss {m['loss']!r} (model {want['loss']!r})")
    assert m["n"] == n and m["correct"] == want["correct"] and m["acc"] == want["correct"] / n and m["nonfinite"] == 0
    assert abs(m["loss"] - want["loss"]) <= (64 + n) * 2.0 ** -53 * abs(want["loss"])
    assert m["positives"] == int((y == 1).sum()) and m["negatives"] == int((y != 1).sum())
    assert same(m["eer_percent"], want["eer_percent"]) and same(m["eer_threshold"], want["eer_threshold"])
    assert abs(m["auc"] - want["auc"]) <= 2.0 ** -52 * want["auc"]
    assert m["groups_scored"] == want["groups_scored"]
    if want["groups_scored"] == 0:
        assert np.isnan(m["macro_eer_percent"])
    else:
        assert abs(m["macro_eer_percent"] - want["macro_eer_percent"]) <= want["groups_scored"] * 2.0 ** -52 * want["macro_eer_percent"]
    if want["groups_scored"] == 1:                                    # one group's EER, no sum: equal
        assert m["macro_eer_percent"] == want["macro_eer_percent"]
    if geer is not None:                                              # every group's EER, ascending group id: equal
        per_group = M.group_eers(s, y, np.zeros(n, dtype=np.int32) if ids is None else ids)
        assert same(geer, list(per_group.values())), (label, geer[:4], list(per_group.values())[:4])
    curve = M.tdcf_curve(s, y, asv)
    if curve is None:
        assert np.isnan(m["min_tDCF"]) and np.isnan(m["min_tDCF_threshold"])
    else:
        bound = 8 * 2.0 ** -53 * abs(want["min_tDCF"])
        assert abs(m["min_tDCF"] - want["min_tDCF"]) <= bound
        at = np.flatnonzero(curve[0] == m["min_tDCF_threshold"])
        assert len(at) == 1 and curve[1][at[0]] - curve[1].min() <= bound
    fpr, tpr, thr = M.roc(s, y)
    assert same(roc[0], fpr) and same(roc[1], tpr) and same(roc[2], thr)
    assert m["distinct"] == len(np.unique(s.astype(np.float64) + 0.0))


def run(gpu, s, y, ids, given, asv=ASV, capacity=65536):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipEvalMetrics
    ev = HipEvalMetrics(PW, gpu, asv_params=asv, capacity=capacity)
    feed(ev, gpu, s, y, ids, given)
    m = ev.compute(curves=True)
    ev._geer = ev.group_eers()
    return ev, m, ev.roc_points()


@pytest.mark.parametrize("n", SIZES)
def test_sizes(gpu, n):
    rng = np.random.default_rng(n)
    s, y = make_scores("normal", n, rng)
    ids, given = make_groups("giant_and_small", n, y, rng)
    ev, m, roc = run(gpu, s, y, ids, given, capacity=max(n, 16))
    check(m, roc, s, y, ids, ASV, f"n={n}", geer=ev._geer)
    assert len(ev) == n and np.array_equal(ev.scores().cpu().numpy(), s) and np.array_equal(ev.labels().cpu().numpy(), y)


@pytest.mark.parametrize("store", STORES)
def test_stores(gpu, store):
    n = 5000
    rng = np.random.default_rng(len(store) * 101 + 7)
    s, y = make_scores(store, n, rng)
    ids, given = make_groups("giant_and_small", n, y, rng)
    ev, m, roc = run(gpu, s, y, ids, given)
    check(m, roc, s, y, ids, ASV, store, geer=ev._geer)


@pytest.mark.parametrize("kind", GROUPINGS)
@pytest.mark.parametrize("store", ["normal", "few_distinct"])
def test_groupings(gpu, store, kind):
    n = 5000
    rng = np.random.default_rng(GROUPINGS.index(kind) + 31)
    s, y = make_scores(store, n, rng)
    ids, given = make_groups(kind, n, y, rng)
    asv = None if kind == "none" else ASV if store == "normal" else ASV_FALLING
    ev, m, roc = run(gpu, s, y, ids, given, asv=asv)
    check(m, roc, s, y, ids, asv, f"{store}/{kind}", geer=ev._geer)
    if asv is ASV_FALLING:
        assert m["min_tDCF_threshold"] > 0
    if kind == "one_group_with_both":
        assert m["groups_scored"] == 1
    if kind == "one_class_groups":
        assert m["groups_scored"] == 0


def _device_counts(s, y):
    """eval_metrics_ref.counts from torch on the device: exact integer arithmetic that shares nothing with the kernels."""
    import torch
    u, inv = torch.unique(s.double() + 0.0, return_inverse=True)
    pos_at = torch.bincount(inv[y == 1], minlength=len(u))
    neg_at = torch.bincount(inv[y != 1], minlength=len(u))
    pb, nb = torch.cumsum(pos_at, 0) - pos_at, torch.cumsum(neg_at, 0) - neg_at
    return u.cpu().numpy(), pb.cpu().numpy(), nb.cpu().numpy(), int(pos_at.sum()), int(neg_at.sum())


def test_every_merge_pass(gpu):
    """2^23 + 9 keys: 4097 tiles, thirteen merge passes, the most a sort can take; four groups; 4001 distinct scores."""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipEvalMetrics
    n = (1 << 23) + 9
    gen = torch.Generator(device=gpu).manual_seed(77)
    y = (torch.rand(n, device=gpu, generator=gen) < 0.4).float()
    s = torch.clamp(torch.round((torch.randn(n, device=gpu, generator=gen) * 2 + y) * 250), -2000, 2000) / 16
    ids = torch.randint(0, 4, (n,), device=gpu, generator=gen, dtype=torch.int32)
    ev = HipEvalMetrics(PW, gpu, asv_params=ASV, capacity=1 << 20)
    ev.add(s[:n - 5], y[:n - 5], ids[:n - 5])
    ev.add(s[n - 5:], y[n - 5:], ids[n - 5:])
    m, roc = ev.compute(curves=True), ev.roc_points()
    c = _device_counts(s, y)
    assert m["n"] == n and m["positives"] == c[3] and m["negatives"] == c[4] and m["distinct"] == len(c[0]) and m["nonfinite"] == 0
    assert m["correct"] == int(((s > 0) == (y == 1)).sum())
    assert same((m["eer_percent"], m["eer_threshold"]), M.eer(None, None, c))
    want = M.auc(None, None, c)
    assert abs(m["auc"] - want) <= 2.0 ** -52 * want
    thr, curve = M.tdcf_curve(None, None, ASV, c)
    bound = 8 * 2.0 ** -53 * curve.min()
    at = np.flatnonzero(thr == m["min_tDCF_threshold"])
    assert abs(m["min_tDCF"] - curve.min()) <= bound and len(at) == 1 and curve[at[0]] - curve.min() <= bound
    assert all(same(a, b) for a, b in zip(roc, M.roc(None, None, c)))
    eers = [M.eer(None, None, _device_counts(s[ids == g], y[ids == g]))[0] for g in range(4)]
    macro = sum(eers) / 4
    assert same(ev.group_eers(), eers)
    print(f"  n {n}: eer {m['eer_percent']!r} auc {m['auc']!r} (model {want!r}) macro {m['macro_eer_percent']!r} (model {macro!r})")
    assert m["groups_scored"] == 4 and abs(m["macro_eer_percent"] - macro) <= 4 * 2.0 ** -52 * macro


def test_add_does_not_wait_for_the_device(gpu):
    """add() with the loader's forms (int64 labels on the host, speaker names; then host id tensors) returns while work queued
    in front of it is still running: an event recorded behind that work has not completed when add() is back."""
    import torch
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipEvalMetrics
    ev = HipEvalMetrics(PW, gpu, asv_params=ASV, capacity=2048)
    logits = torch.randn(256, 1, device=gpu)
    lbls = (torch.rand(256) < 0.5).long()
    names = [f"spk{i % 7}" for i in range(256)]
    forms = {"host int64 labels, names": (lbls, names), "host float labels, host int64 ids": (lbls.float(), torch.arange(256) % 7),
             "device labels, device ids": (lbls.to(gpu), (torch.arange(256) % 7).to(gpu)), "device labels, no speakers": (lbls.to(gpu), None)}
    for y, spk in forms.values():                                     # warm: library, allocators, pinned staging blocks
        ev.add(logits, y, spk)
    ev.reset()
    a = torch.randn(4096, 4096, device=gpu)
    c = torch.empty_like(a)
    torch.mm(a, a, out=c)
    torch.cuda.synchronize()
    busy = torch.cuda.Event()
    for _ in range(100):                                              # a tenth of a second or more of queued device work
        torch.mm(a, a, out=c)
    busy.record()
    waited = {}
    for form, (y, spk) in forms.items():
        ev.add(logits, y, spk)
        waited[form] = busy.query()                                   # True: the queued work was over when add() came back
    torch.cuda.synchronize()
    assert not any(waited.values()), f"add() waited for the device: {waited}"
    m = ev.compute()
    assert m["n"] == 1024 and m["groups_scored"] == 7, m


def test_curves_ride_on_one_compute(gpu):
    """compute(curves=True) leaves the ROC points and the groups' EERs behind: roc_points() / group_eers() then equal a fresh
    call's, and add() drops them."""
    rng = np.random.default_rng(21)
    s, y = make_scores("few_distinct", 3000, rng)
    ids, given = make_groups("names", 3000, y, rng)
    ev, m, roc = run(gpu, s, y, ids, given)
    assert ev._curves is not None
    fresh = type(ev)(PW, gpu, asv_params=ASV)
    feed(fresh, gpu, s, y, ids, given)
    roc2, geer2 = fresh.roc_points(), fresh.group_eers()               # no compute() in front: they run it themselves
    assert all(a.tobytes() == b.tobytes() for a, b in zip(roc, roc2)) and ev._geer.tobytes() == geer2.tobytes()
    assert len(geer2) == m["groups_scored"] == 23
    feed(ev, gpu, s[:10], y[:10], ids[:10], given if given == "ids" else given[:10], [(0, 10)])
    assert ev._curves is None and len(ev.roc_points()[0]) >= 2


def test_cdef_not_positive_gives_nan_tdcf(gpu):
    rng = np.random.default_rng(5)
    s, y = make_scores("normal", 300, rng)
    _, m, _ = run(gpu, s, y, None, None, asv=dict(ASV, pi_non=0.0))
    assert np.isnan(m["min_tDCF"]) and np.isnan(m["min_tDCF_threshold"]) and np.isfinite(m["eer_percent"])


def test_compute_twice_gives_identical_bytes(gpu):
    rng = np.random.default_rng(11)
    s, y = make_scores("few_distinct", 9000, rng)
    ids, given = make_groups("giant_and_small", 9000, y, rng)
    ev, m1, roc1 = run(gpu, s, y, ids, given)
    raw1 = ev._state.cpu().numpy().tobytes()
    m2 = ev.compute()
    raw2 = ev._state.cpu().numpy().tobytes()
    roc2 = ev.roc_points()
    assert raw1 == raw2 and repr(m1) == repr(m2)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(roc1, roc2))
    ev2, m3, roc3 = run(gpu, s, y, ids, given)                      # and a second object from scratch
    assert ev2._state.cpu().numpy().tobytes() == raw1 and all(a.tobytes() == b.tobytes() for a, b in zip(roc1, roc3))


def test_compute_then_more_adds_equals_one_pass(gpu):
    from radad_retrievalaugmenteddeepfakeaudiodetection_amd import HipEvalMetrics
    rng = np.random.default_rng(12)
    n = 6000
    s, y = make_scores("normal", n, rng)
    ids, given = make_groups("giant_and_small", n, y, rng)
    cuts = [(0, 1500), (1500, 3000), (3000, 5999), (5999, 6000)]
    a = HipEvalMetrics(PW, gpu, asv_params=ASV)
    feed(a, gpu, s[:3000], y[:3000], ids[:3000], given, cuts[:2])
    first = a.compute()
    check(first, a.roc_points(), s[:3000], y[:3000], ids[:3000], ASV, "first half")
    import torch
    xs, ys = torch.from_numpy(s).to(gpu), torch.from_numpy(y).to(gpu)
    for lo, hi in cuts[2:]:
        a.add(xs[lo:hi], ys[lo:hi], torch.from_numpy(ids[lo:hi]).to(gpu))
    b = HipEvalMetrics(PW, gpu, asv_params=ASV)
    feed(b, gpu, s, y, ids, given, cuts)
    ma, mb = a.compute(), b.compute()
    assert repr(ma) == repr(mb) and a._state.cpu().numpy().tobytes() == b._state.cpu().numpy().tobytes()
    check(ma, a.roc_points(), s, y, ids, ASV, "both halves")
    a.reset()
    assert len(a) == 0
    with pytest.raises(ValueError, match="no samples"):
        a.compute()
    feed(a, gpu, s[:100], y[:100], None, None)
    check(a.compute(), a.roc_points(), s[:100], y[:100], None, ASV, "after reset")


def test_growth_across_capacity_keeps_earlier_samples(gpu):
    rng = np.random.default_rng(13)
    n = 3000
    s, y = make_scores("normal", n, rng)
    ids, given = make_groups("names", n, y, rng)
    ev, m, roc = run(gpu, s, y, ids, given, capacity=16)          # 16 -> 4096 by doubling, through every batch of the ragged feed
    assert ev._cap == 4096
    check(m, roc, s, y, ids, ASV, "grown", geer=ev._geer)
    assert np.array_equal(ev.scores().cpu().numpy(), s) and np.array_equal(ev.labels().cpu().numpy(), y)


def test_non_finite_scores_give_nan_metrics_and_a_count(gpu):
    rng = np.random.default_rng(14)
    n = 3000
    s, y = make_scores("normal", n, rng)
    s[[3, 2500]] = np.inf
    s[7] = -np.inf
    s[2999] = np.nan
    ids, given = make_groups("giant_and_small", n, y, rng)
    ev, m, roc = run(gpu, s, y, ids, given)
    assert m["nonfinite"] == 4 and m["n"] == n and m["groups_scored"] == 0
    for k in ("auc", "eer_percent", "eer_threshold", "macro_eer_percent", "min_tDCF", "min_tDCF_threshold"):
        assert np.isnan(m[k]), k
    assert all(len(a) == 0 for a in roc)
    import torch
    torch.cuda.synchronize()                                          # nothing faulted


def test_beside_the_torch_tail_on_a_small_model(gpu):
    """HipEvalMetrics beside pipeline.py:725-733 and the numpy metrics on a small RADADModel's logits."""
    import torch
    import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R
    B, K, D = 8, 3, 64
    cfg = R.Config()
    cfg.update(device=gpu, projection_hidden_dim=32, projection_output_dim=16, detection_hidden_dims=[16, 8])
    torch.manual_seed(4)
    model = R.RADADModel(cfg, D).eval()
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([PW], device=gpu))
    ev = R.HipEvalMetrics(PW, gpu, asv_params=ASV, capacity=32)
    total_loss, correct, total, scores, labels, speakers = 0.0, 0, 0, [], [], []
    with torch.no_grad():
        for k in range(6):
            x, t = torch.randn(B, K, D, device=gpu), torch.randn(B, D, device=gpu)
            lbls = (torch.rand(B) < 0.5).long()                       # the loader's labels: int64 on the host
            spk = [f"spk{(k * B + i) % 5}" for i in range(B)]
            logits = model(x, t)
            if logits.ndim == 1:
                logits = logits.unsqueeze(-1)
            ev.add(logits, lbls, spk)
            y = lbls.to(gpu).to(dtype=logits.dtype).view_as(logits)
            total_loss += crit(logits, y).item() * B
            correct += ((logits > 0).to(y.dtype) == y).sum().item()
            total += B
            scores += logits.cpu().view(-1).tolist()
            labels += lbls.view(-1).tolist()
            speakers += spk
    m = ev.compute()
    s, y = np.asarray(scores, dtype=np.float32), np.asarray(labels, dtype=np.float32)
    first = {}
    ids = np.array([first.setdefault(v, len(first)) for v in speakers], dtype=np.int32)
    assert m["correct"] == correct and m["n"] == total == 48 and m["acc"] == correct / total
    assert abs(m["loss"] - total_loss / total) <= 1e-5 * abs(total_loss / total)          # torch's float32 loss, batch by batch
    check(m, ev.roc_points(), s, y, ids, ASV, "model tail")
