"""Second-stage clustering of a batch of 224 x 224 crop maps: the batched call (mean_shift.mean_shift_smart_init_batched) against the
per-map loop (mean_shift.mean_shift_smart_init), 100 seeds, 10 iterations, 16 and 128 maps.  Both forms are timed in the same
process, alternating, with HIP events; the median of the runs after warm-up is reported, with the seeding stage alone beside it.
Prints one JSON line.

    python tools/probes/meanshift_crops_time.py [--runs 21] [--warmup 3] [--maps 16,128]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from unseenobjectswithmeanshift_amd import mean_shift as ms, ops, synthetic as syn  # noqa: E402

N, S, ITERS, KAPPA = 224 * 224, 100, 10, 20


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maps", default="16,128")
    args = ap.parse_args()
    if args.runs < 20:
        raise SystemExit("--runs must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this probe measures, it does not estimate")
    out = {"probe": "meanshift_crops", "device": torch.cuda.get_device_name(0), "n": N, "seeds": S, "iters": ITERS, "runs": args.runs, "cases": []}
    # a few distinct maps, repeated: what is timed does not depend on the data, and 128 distinct maps take a minute to synthesise
    base = torch.stack([syn.synth_unit_embeddings(N, 64, clusters=2 + m, sigma=0.2, seed=40 + m)[0] for m in range(4)]).cuda()
    for M in [int(v) for v in args.maps.split(",")]:
        X = base.repeat((M + 3) // 4, 1, 1)[:M].contiguous()
        first = [(N // 3 + 997 * m) % N for m in range(M)]
        first_dev = torch.tensor(first, device="cuda")
        forms = {
            "batched_ms": lambda: ms.mean_shift_smart_init_batched(X, KAPPA, S, ITERS, first_indices=first_dev),
            "loop_ms": lambda: [ms.mean_shift_smart_init(X[m], KAPPA, S, ITERS, first_index=first[m]) for m in range(M)],
            "seeding_batched_ms": lambda: ops.ms_select_seeds_batched(X, S, first_dev),
            "seeding_loop_ms": lambda: [ops.ms_select_seeds(X[m], S, first[m]) for m in range(M)],
        }
        lb, sb = forms["batched_ms"]()
        ll = forms["loop_ms"]()
        same = all(torch.equal(lb[m], ll[m][0]) and torch.equal(sb[m], ll[m][1]) for m in range(M))
        times = {k: [] for k in forms}
        for r in range(args.warmup + args.runs):
            for k, fn in forms.items():                      # alternating: both forms see the same state of the box
                t = event_ms(fn)
                if r >= args.warmup:
                    times[k].append(t)
        case = {"maps": M, "results_equal": bool(same)}
        for k, v in times.items():
            case[k] = round(statistics.median(v), 4)
            case[k.replace("_ms", "_min_ms")] = round(min(v), 4)
        case["speedup"] = round(case["loop_ms"] / case["batched_ms"], 3)
        case["seeding_speedup"] = round(case["seeding_loop_ms"] / case["seeding_batched_ms"], 3)
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
