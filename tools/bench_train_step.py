#!/usr/bin/env python3
"""RADADModel's whole training step (pipeline.py:808-836: forward, loss, backward, unscale, clip, Adam, scale update, the numbers
the loop logs) with three ways of doing everything behind the forward, beside the step tools/bench_head_train.py times (forward,
BCEWithLogitsLoss, backward, zero_grad(): no optimizer) as the floor under all three.

  ref    the reference's tail verbatim: criterion, GradScaler, three unscale_, three clip_grad_norm_ each with float(), three
         scaler.step over torch.optim.Adam, update, loss.item(), the accuracy .item()
  fused  the best torch does without this package: Adam(fused=True), norms left on the device, everything logged read in one
         .tolist() per step
  hip    HipTrainStep (csrc/optim_step.inc) with one stats() read per step

config.projection_train_hip and config.head_train_hip are on in every arm, so forward and backward are the same kernels; the
forward runs without autocast in every arm (the HIP forward is float32 either way).  Shapes (B, K, D) = (256, 5, 5376),
(256, 5, 3584), (1024, 5, 512), default head [64, 32].  One model, one set of tensors, one process; each arm has its own optimizer
state.  The arms alternate in rounds; per round `--steps` steps of each, each window between two device events; the figure kept per
arm is the median round, with the fastest and slowest beside it.  Writes one JSON file (--out).

--arm base|ref|fused|hip --shape SHAPE_INDEX runs one arm alone, `--steps` times without warm-up, for a kernel trace (one
profiler run of its own per arm; profiles/train_step.md): launches per step = kernel calls / steps.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R  # noqa: E402
from radad_retrievalaugmenteddeepfakeaudiodetection_amd.train_step import HipTrainStep  # noqa: E402

SHAPES = [(256, 5, 5376), (256, 5, 3584), (1024, 5, 512)]
ARMS = ("base", "ref", "fused", "hip")
LR, WD, POS_WEIGHT = 1e-3, 1e-5, 1.7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arm", choices=("all",) + ARMS, default="all")
    ap.add_argument("--shape", type=int, default=None, metavar="SHAPE_INDEX")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device: a timing on the CPU says nothing"
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds, "head": [64, 32], "dropout": 0.1,
              "shapes": []}
    for si, (B, K, D) in enumerate(SHAPES):
        if a.shape is not None and si != a.shape:
            continue
        cfg = R.Config()
        cfg.update(device=dev, projection_train_hip=True, head_train_hip=True)
        torch.manual_seed(si)
        model = R.RADADModel(cfg, D).train()
        x = torch.randn(B, K, D, device=dev)
        t = torch.randn(B, D, device=dev)
        y = (torch.rand(B, device=dev) < 0.5).float()
        groups = [model.projection_layer, model.fuse, model.detection_model]
        n_params = sum(p.numel() for p in model.parameters())
        plain_loss = torch.nn.BCEWithLogitsLoss()
        criterion = torch.nn.BCEWithLogitsLoss(pos_weight=torch.tensor([POS_WEIGHT], device=dev, dtype=torch.float32))
        ref_opts = [torch.optim.Adam(g.parameters(), lr=LR, weight_decay=WD) for g in groups]
        ref_scaler = torch.amp.GradScaler("cuda")
        fused_opts = [torch.optim.Adam(g.parameters(), lr=LR, weight_decay=WD, fused=True) for g in groups]
        fused_scaler = torch.amp.GradScaler("cuda")
        hip = HipTrainStep.for_model(model, cfg, POS_WEIGHT)

        def base_step():                      # tools/bench_head_train.py's full_step
            plain_loss(model(x, t), y).backward()
            model.zero_grad()

        def ref_step():                       # pipeline.py:811-836
            logits = model(x, t)
            if logits.ndim == 1:
                logits = logits.unsqueeze(-1)
            labels = y.to(dtype=logits.dtype).view_as(logits)
            loss = criterion(logits, labels)
            for o in ref_opts:
                o.zero_grad()
            ref_scaler.scale(loss).backward()
            for o in ref_opts:
                ref_scaler.unscale_(o)
            norms = [float(torch.nn.utils.clip_grad_norm_(g.parameters(), max_norm=1.0)) for g in groups]
            for o in ref_opts:
                ref_scaler.step(o)
            ref_scaler.update()
            lv = loss.item()
            preds = (logits > 0).to(labels.dtype)
            return lv, (preds == labels).sum().item(), norms

        def fused_step():
            logits = model(x, t)
            loss = criterion(logits, y)
            for o in fused_opts:
                o.zero_grad()
            fused_scaler.scale(loss).backward()
            for o in fused_opts:
                fused_scaler.unscale_(o)
            norms = [torch.nn.utils.clip_grad_norm_(g.parameters(), max_norm=1.0) for g in groups]
            for o in fused_opts:
                fused_scaler.step(o)
            fused_scaler.update()
            correct = ((logits.detach() > 0) == (y > 0)).sum()
            return torch.stack([loss.detach(), correct.float()] + norms).tolist()

        def hip_step():
            logits = model(x, t)
            hip.zero_grad()
            hip.backward(logits, y)
            hip.step()
            return hip.stats()

        steps = {"base": base_step, "ref": ref_step, "fused": fused_step, "hip": hip_step}

        def window(step):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                step()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / a.steps

        if a.arm != "all":                        # a kernel trace of one arm: nothing but its steps
            window(steps[a.arm])
            print(json.dumps({"B": B, "K": K, "D": D, "arm": a.arm, "steps": a.steps, "parameters": n_params}), flush=True)
            continue
        for _ in range(a.warmup):
            for arm in ARMS:
                steps[arm]()
        torch.cuda.synchronize()
        ms = {arm: [] for arm in ARMS}
        for _ in range(a.rounds):
            for arm in ARMS:
                ms[arm].append(window(steps[arm]))
        stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
        row = {"B": B, "K": K, "D": D, "parameters": n_params}
        for arm in ARMS:
            row[f"step_{arm}_ms"] = stat(ms[arm])
        for arm in ARMS[1:]:
            row[f"tail_{arm}_ms"] = row[f"step_{arm}_ms"]["median"] - row["step_base_ms"]["median"]
        row["ref_over_hip"] = row["step_ref_ms"]["median"] / row["step_hip_ms"]["median"]
        row["fused_over_hip"] = row["step_fused_ms"]["median"] / row["step_hip_ms"]["median"]
        row["last_hip_stats"] = hip.stats()
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.arm == "all" and a.shape is None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
