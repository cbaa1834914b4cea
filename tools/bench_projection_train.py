#!/usr/bin/env python3
"""ProjectionLayer training step (forward + backward + zero_grad) timing: the HIP path (config.projection_train_hip,
csrc/proj_train.inc) against torch float32 autograd of the reference's unfolded form (tests/proj_train_ref.py) on the same
device, the same parameters and the same inputs.

Shapes (B, K, D) = (256, 5, 5376), (256, 5, 3584), (1024, 5, 512) with H = 256, O = 128 and the default dropout 0.1; x needs
no gradient (the reference's train loop feeds retrieved vectors, pipeline.py:784-829).  The two paths alternate in rounds on
one process and one set of tensors: per round `--steps` steps of one, then of the other, each window between two device events;
the figure kept per path is the median round, with the fastest and slowest beside it.  A window is 200 steps (70-200 ms).
Each step ends with the module's zero_grad() (set_to_none, as an optimizer's), so both paths allocate their gradient tensors
anew every step, as a training loop does.  Writes one JSON file (--out).

--hip-only SHAPE_INDEX runs the HIP path alone for a kernel trace (one profiler run of its own; profiles/proj_train.md).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import proj_train_ref as PR  # noqa: E402
import radad_retrievalaugmenteddeepfakeaudiodetection_amd as R  # noqa: E402

SHAPES = [(256, 5, 5376), (256, 5, 3584), (1024, 5, 512)]
H, O = 256, 128
PEAK_F32_MATRIX_TFLOPS = 157.3


def gemm_flop(B, K, D):
    """FLOP of the matrix products one HIP step runs (dx not requested), by product."""
    M = B * K
    return {"fwd [W1;W3] x": 2 * M * D * 2 * H, "fwd u = W4 hbar": 2 * B * D * H, "fwd v = W5 u": 2 * B * H * D,
            "fwd out = W6 nd": 2 * B * O * H,
            "bwd dW6": 2 * B * O * H, "bwd dW5": 2 * B * H * D, "bwd du": 2 * B * D * H, "bwd dW4": 2 * B * D * H,
            "bwd dhbar": 2 * B * H * D, "bwd [dW1;dW3]": 2 * M * 2 * H * D}


def torch_flop(B, K, D):
    """FLOP of the reference's form: 3 units of 2 M D H forward (W1, W3, W4 per neighbour row) and 4 backward (dW1, dW3, dW4, dh)."""
    return 7 * 2 * B * K * D * H + 3 * 2 * B * H * D


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hip-only", type=int, default=None, metavar="SHAPE_INDEX")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proj_train_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a ROCm device: a timing on the CPU says nothing"
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "steps": a.steps, "rounds": a.rounds, "hidden": H, "out_dim": O,
              "dropout": 0.1, "peak_f32_matrix_tflops": PEAK_F32_MATRIX_TFLOPS, "shapes": []}
    for si, (B, K, D) in enumerate(SHAPES):
        if a.hip_only is not None and si != a.hip_only:
            continue
        cfg = R.Config()
        cfg.update(device=dev, projection_hidden_dim=H, projection_output_dim=O, projection_dropout=0.1, projection_train_hip=True)
        torch.manual_seed(si)
        layer = R.ProjectionLayer(cfg, D).train()
        x = torch.randn(B, K, D, device=dev)
        g = torch.randn(B, O, device=dev)
        params = dict(layer.named_parameters())

        def hip_step():
            layer(x).backward(g)
            layer.zero_grad()

        def torch_step():
            mask = torch.empty((B, H), device=dev).bernoulli_(0.9)
            PR.forward(x, params, mask, 1.0 / 0.9).backward(g)
            layer.zero_grad()

        def window(step):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                step()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1) / a.steps

        for _ in range(a.warmup):
            hip_step()
            if a.hip_only is None:
                torch_step()
        torch.cuda.synchronize()
        hip_ms, torch_ms = [], []
        for _ in range(a.rounds):
            hip_ms.append(window(hip_step))
            if a.hip_only is None:
                torch_ms.append(window(torch_step))
        row = {"B": B, "K": K, "D": D, "hip_ms": {"median": statistics.median(hip_ms), "min": min(hip_ms), "max": max(hip_ms)},
               "hip_gemm_flop": gemm_flop(B, K, D)}
        row["hip_step_tflops"] = sum(row["hip_gemm_flop"].values()) / (row["hip_ms"]["median"] * 1e-3) / 1e12
        if torch_ms:
            row["torch_ms"] = {"median": statistics.median(torch_ms), "min": min(torch_ms), "max": max(torch_ms)}
            row["torch_step_tflops"] = torch_flop(B, K, D) / (row["torch_ms"]["median"] * 1e-3) / 1e12
            row["torch_over_hip"] = row["torch_ms"]["median"] / row["hip_ms"]["median"]
        result["shapes"].append(row)
        print(json.dumps(row), flush=True)
    if a.hip_only is None:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
