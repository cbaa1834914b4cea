#!/usr/bin/env python3
"""RADADModel training step (forward + BCE-with-logits + backward + zero_grad) timing with the fuse Linear and the detection MLP
as torch modules (config.head_train_hip off: the behaviour before csrc/head_train.inc) against the same step with them in HIP
(config.head_train_hip on).  config.projection_train_hip is on in both arms, so the projection's share is the same kernels.

Shapes (B, K, D) = (256, 5, 5376), (256, 5, 3584), (1024, 5, 512) with the default head [64, 32], BatchNorm and dropout 0.1.
One model, one set of tensors, one process: the arms differ in the config switch alone.  They alternate in rounds; per round
`--steps` steps of one, then of the other, each window between two device events; the figure kept per arm is the median round,
with the fastest and slowest beside it.  A window is 200 steps (more than 70 ms).  Each step ends with the module's zero_grad()
(set_to_none, as an optimizer's), so both arms allocate their gradient tensors anew every step, as a training loop does.
The tail alone (fuse_and_detect on a given projection output, same loss, backward, zero_grad) is timed the same way beside it.
Writes one JSON file (--out).

--arm torch|hip --shape SHAPE_INDEX runs one arm's full step alone, `--steps` times without warm-up, for a kernel trace (one
profiler run of its own per arm; profiles/head_train.md): launches per step = kernel calls / steps.
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

SHAPES = [(256, 5, 5376), (256, 5, 3584), (1024, 5, 512)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arm", choices=("both", "torch", "hip"), default="both")
    ap.add_argument("--shape", type=int, default=None, metavar="SHAPE_INDEX")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_train_bench.json"))
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
        cfg.update(device=dev, projection_train_hip=True, head_train_hip=False)
        torch.manual_seed(si)
        model = R.RADADModel(cfg, D).train()
        x = torch.randn(B, K, D, device=dev)
        t = torch.randn(B, D, device=dev)
        proj = torch.randn(B, cfg.projection_output_dim, device=dev)
        y = (torch.rand(B, device=dev) < 0.5).float()
        loss_fn = torch.nn.BCEWithLogitsLoss()

        def full_step():
            loss_fn(model(x, t), y).backward()
            model.zero_grad()

        def tail_step():
            loss_fn(model.fuse_and_detect(t, proj), y).backward()
            model.zero_grad()

        def window(step, hip):
            cfg.head_train_hip = hip
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                step()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / a.steps

        if a.arm != "both":                       # a kernel trace of one arm: nothing but its steps
            window(full_step, a.arm == "hip")
            print(json.dumps({"B": B, "K": K, "D": D, "arm": a.arm, "steps": a.steps}), flush=True)
            continue
        for _ in range(a.warmup):
            for hip in (False, True):
                cfg.head_train_hip = hip
                full_step()
                tail_step()
        torch.cuda.synchronize()
        ms = {("full", False): [], ("full", True): [], ("tail", False): [], ("tail", True): []}
        for _ in range(a.rounds):
            for what, step in (("full", full_step), ("tail", tail_step)):
                for hip in (False, True):
                    ms[(what, hip)].append(window(step, hip))
        stat = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
        row = {"B": B, "K": K, "D": D,
               "step_torch_head_ms": stat(ms[("full", False)]), "step_hip_head_ms": stat(ms[("full", True)]),
               "tail_torch_ms": stat(ms[("tail", False)]), "tail_hip_ms": stat(ms[("tail", True)])}
        row["step_torch_over_hip"] = row["step_torch_head_ms"]["median"] / row["step_hip_head_ms"]["median"]
        row["tail_torch_over_hip"] = row["tail_torch_ms"]["median"] / row["tail_hip_ms"]["median"]
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.arm == "both" and a.shape is None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
