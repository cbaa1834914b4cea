#!/usr/bin/env python3
"""What a validation pass costs behind the model's forward (pipeline.py:725-733, 868-872), two ways on the same tensors:

  hip    HipEvalMetrics: add() per batch (csrc/eval_metrics.inc, no host read), compute() at the end (one device-to-host copy)
  ref    the reference-form tail: per batch criterion(...).item(), the accuracy .item(), logits.cpu().tolist() and
         lbls.cpu().tolist(); at the end EER, macro-EER by speaker, min t-DCF, ROC and AUC in numpy (tests/eval_metrics_ref.py)

Logits and labels for 25 000 samples of 20 speakers and 71 000 samples of 60 speakers, made once from a seed; batches of
config.eval_batch_size (256 where the config has none, as the reference's main.py sets it).  The logits are on the device (they
come out of the model), the labels an int64 host tensor (they come out of the loader), the speakers a list of names.  The arms
alternate in rounds on one device in one process; per round each arm does one whole pass; a host clock around work that ends in
a device synchronise.  Reported per arm: the per-batch cost (the batch loop's time over the number of batches) and the
end-of-pass cost, each the median round with the fastest and slowest beside it.  Those loops run on an idle stream.  A
validation loop does not: the forward is queued in front of every batch, and a tail that reads back waits for it while one that
does not lets the host run ahead.  So every round also times three loops with a stand-in forward (matrix products on the
stream) in front of each batch: the forward alone, forward + add(), forward + the reference-form reads; the loop's time per
batch (`behind_queued_forward`).  Writes one JSON file (--out).

--arm hip --size INDEX runs one arm alone for a kernel trace (a profiler run of its own; profiles/eval_metrics.md).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import eval_metrics_ref as M  # noqa: E402
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R  # noqa: E402

SIZES = [(25000, 20), (71000, 60)]
POS_WEIGHT = 1.7


def make(n, speakers, seed, dev):
    rng = np.random.default_rng(seed)
    y = (rng.random(n) < 0.3).astype(np.int64)
    s = (rng.standard_normal(n) * 2.0 + 2.5 * y - 1.0).astype(np.float32)
    spk = [f"LA_{v:04d}" for v in rng.integers(0, speakers, n)]
    return torch.from_numpy(s).to(dev).view(-1, 1), torch.from_numpy(y), spk


class Forward:
    """A stand-in for the model's forward in front of every batch: `k` matrix products of 2048 x 2048 floats on the stream."""

    def __init__(self, dev, k):
        self.a = torch.randn(2048, 2048, device=dev) / 45.0
        self.c = torch.empty_like(self.a)
        self.k = k

    def __call__(self):
        for _ in range(self.k):
            torch.mm(self.a, self.a, out=self.c)


def forward_only(fwd, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(batches):
        fwd()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def hip_pass(ev, logits, lbls, spk, bs, fwd=None):
    n = logits.shape[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev.reset()
    for lo in range(0, n, bs):
        if fwd:
            fwd()
        ev.add(logits[lo:lo + bs], lbls[lo:lo + bs], spk[lo:lo + bs])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    m = ev.compute()
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, m


def ref_pass(crit, logits_all, lbls_all, spk_all, bs, dev, fwd=None):
    n = logits_all.shape[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    total_loss, correct, total, scores, labels, speakers = 0.0, 0, 0, [], [], []
    for lo in range(0, n, bs):
        if fwd:
            fwd()
        logits, lbls = logits_all[lo:lo + bs], lbls_all[lo:lo + bs]
        y = lbls.to(dev).to(dtype=logits.dtype).view_as(logits)
        loss = crit(logits, y)
        total_loss += loss.item() * lbls.size(0)
        correct += ((logits > 0).to(y.dtype) == y).sum().item()
        total += y.numel()
        scores.extend(logits.detach().cpu().view(-1).tolist())
        labels.extend(lbls.detach().cpu().view(-1).tolist())
        speakers.extend(spk_all[lo:lo + bs])
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    s, y = np.asarray(scores, dtype=np.float64), np.asarray(labels, dtype=np.int32)
    g = np.unique(np.asarray(speakers), return_inverse=True)[1]
    eer, thr = M.eer(s, y)
    macro, groups = M.macro_eer(s, y, g)
    tdcf, tthr = M.min_tdcf(s, y, M.ASV_2019)
    fpr, tpr, _ = M.roc(s, y)
    auc = M.auc(s, y)
    t2 = time.perf_counter()
    m = {"loss": total_loss / total, "acc": correct / total, "eer_percent": eer, "eer_threshold": thr, "macro_eer_percent": macro,
         "groups_scored": groups, "min_tDCF": tdcf, "min_tDCF_threshold": tthr, "auc": auc, "roc_points": len(fpr)}
    return t1 - t0, t2 - t1, m


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--arm", choices=("all", "hip", "ref"), default="all")
    ap.add_argument("--size", type=int, default=None, metavar="INDEX")
    ap.add_argument("--forward-products", type=int, default=8, help="matrix products of the stand-in forward per batch")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device: a timing on the CPU says nothing"
    dev = torch.device("cuda:0")
    bs = int(getattr(R.Config(), "eval_batch_size", 256))
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([POS_WEIGHT], device=dev))
    result = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "batch_size": bs, "sizes": []}
    for si, (n, speakers) in enumerate(SIZES):
        if a.size is not None and si != a.size:
            continue
        logits, lbls, spk = make(n, speakers, 100 + si, dev)
        ev = R.HipEvalMetrics(POS_WEIGHT, dev, asv_params=M.ASV_2019)
        times = {"hip": ([], []), "ref": ([], [])}
        queued = {"forward": [], "hip": [], "ref": []}
        last = {}
        batches = (n + bs - 1) // bs
        fwd = Forward(dev, a.forward_products)
        for r in range(a.warmup + a.rounds):
            for arm in ("hip", "ref"):
                if a.arm not in ("all", arm):
                    continue
                tb, te, m = hip_pass(ev, logits, lbls, spk, bs) if arm == "hip" else ref_pass(crit, logits, lbls, spk, bs, dev)
                last[arm] = m
                if r >= a.warmup:
                    times[arm][0].append(tb)
                    times[arm][1].append(te)
            if a.arm == "all":                                         # the same loops behind a queued forward per batch
                tf = forward_only(fwd, batches)
                th = hip_pass(ev, logits, lbls, spk, bs, fwd)[0]
                tr = ref_pass(crit, logits, lbls, spk, bs, dev, fwd)[0]
                if r >= a.warmup:
                    for k, t in (("forward", tf), ("hip", th), ("ref", tr)):
                        queued[k].append(1e6 * t / batches)
        row = {"n": n, "speakers": speakers, "batches": batches}
        if queued["forward"]:
            row["behind_queued_forward"] = {"forward_products": a.forward_products,
                                            "loop_us_per_batch": {k: spread(v) for k, v in queued.items()}}
        for arm, (tb, te) in times.items():
            if tb:
                row[arm] = {"per_batch_us": spread([1e6 * t / batches for t in tb]), "end_of_pass_ms": spread([1e3 * t for t in te]),
                            "pass_ms": spread([1e3 * (x + y) for x, y in zip(tb, te)])}
        if len(last) == 2:                                             # the two arms computed the same pass
            h, f = last["hip"], last["ref"]
            row["same"] = {k: bool(h[k] == f[k]) for k in ("acc", "eer_percent", "eer_threshold", "groups_scored", "min_tDCF_threshold")}
            row["rel_diff"] = {k: abs(h[k] - f[k]) / abs(f[k]) for k in ("loss", "auc", "macro_eer_percent", "min_tDCF")}
            row["metrics"] = {k: h[k] for k in ("loss", "acc", "auc", "eer_percent", "macro_eer_percent", "min_tDCF")}
        result["sizes"].append(row)
        print(json.dumps(row))
    if a.arm == "all":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
