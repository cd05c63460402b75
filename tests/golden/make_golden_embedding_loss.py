"""tests/golden/embedding_loss.npz: the reference's own EmbeddingLoss on the planted inputs of tests/embloss_cases.py.

    python tests/golden/make_golden_embedding_loss.py <reference>/lib/networks/embedding.py

Needs only torch: the reference module is loaded by file path and run on the CPU, once with float64 as the default dtype and
once in float32.  Stored per golden case: the three losses of both runs, the checksum of x, and the float64 gradient of
2 loss + 3 intra - inter with respect to x (case 0 in full, the others a strided sample of 4096 values, the sum and the largest
magnitude), plus the float32 run's distance to the float64 run (losses, relative; gradient, relative to its largest magnitude)."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import embloss_cases as EC  # noqa: E402


def load_reference(path):
    spec = importlib.util.spec_from_file_location("reference_embedding", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.EmbeddingLoss


def run(EmbeddingLoss, name, dtype):
    case = EC.CASES[name]
    x, labels = EC.planted(name)
    torch.set_default_dtype(dtype)
    try:
        x = x.to(dtype).clone().requires_grad_(True)
        crit = EmbeddingLoss(EC.ALPHA, case.delta, EC.LAMBDA_INTRA, EC.LAMBDA_INTER, case.metric, case.normalize)
        loss, intra, inter = crit(x, labels if labels.dtype == torch.int64 else labels.to(dtype))
        w = EC.GRAD_WEIGHTS
        (w[0] * loss + w[1] * intra + w[2] * inter).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return np.array([float(loss), float(intra), float(inter)], dtype=np.float64), grad.detach().double()


def main():
    EmbeddingLoss = load_reference(sys.argv[1])
    out = {}
    for name in EC.GOLDEN_CASES:
        l64, g64 = run(EmbeddingLoss, name, torch.float64)
        l32, g32 = run(EmbeddingLoss, name, torch.float32)
        x, _ = EC.planted(name)
        flat = g64.reshape(-1)
        out[f"{name}_losses64"], out[f"{name}_losses32"] = l64, l32
        out[f"{name}_checksum"] = np.float64(EC.checksum(x))
        out[f"{name}_grad"] = (flat if name == "0" else flat[EC.grad_sample_index(flat.numel())]).numpy()
        out[f"{name}_grad_sum"], out[f"{name}_grad_max"] = np.float64(flat.sum()), np.float64(flat.abs().max())
        gmax = max(float(flat.abs().max()), 1e-300)
        out[f"{name}_grad32_err"] = np.float64(float((g32 - g64).abs().max()) / gmax)
        rel = [abs(a - b) / abs(b) if b != 0 else abs(a) for a, b in zip(l32, l64)]
        out[f"{name}_loss32_err"] = np.float64(max(rel))
        print(name, l64, f"fp32 run: loss {max(rel):.2e} grad {float(out[name + '_grad32_err']):.2e}")
    np.savez_compressed(os.path.join(HERE, "embedding_loss.npz"), **out)


if __name__ == "__main__":
    main()
