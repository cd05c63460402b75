"""Record the bits of optim.FullModelClipAdamW: tests/golden/optim_adamw_bits.json, the fixture that tests/test_gpu_optim_scaler.py
holds the optimizer to and tests/test_optim_cases_cpu.py holds to the cases.

    python tools/record_optim_bits.py --commit <id of the commit that is recorded> [--out tests/golden/optim_adamw_bits.json]

Every case of tests/optim_cases.py on its edge table (sizes 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 chunk + 3, the two misaligned
views, the tensor without a gradient on step 2: the smallest shapes that reach every loop of the kernels), three steps each, no
scaler.  After every step, for every tensor, the SHA-256 of the raw bytes of p, .grad, exp_avg and exp_avg_sq (null where absent)
and the 32-bit patterns of last_grad_norm and last_clip_coef; beside them the SHA-256 of every start value and every gradient that
was fed, and a header: chunk size, torch and hipcc versions, the commit.  Hashes only, so the file is a few tens of kilobytes.

Only the public API is used (FullModelClipAdamW, tests/optim_cases.py), so this file runs unchanged on any commit that has them:
the fixture is recorded on the last commit whose bits are the accepted ones, never on the tree under test.  Needs a GPU."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import optim_cases as OC  # noqa: E402

STEPS = 3
QUANTITIES = ("p", "grad", "exp_avg", "exp_avg_sq")
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "optim_adamw_bits.json")


def sha(t):
    """SHA-256 of the raw bytes of a tensor's elements (a view: its own elements, in order); None for None."""
    return None if t is None else hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def bits(t):
    """The 32-bit pattern of a 0-d float32 tensor."""
    return int(t.detach().cpu().reshape(1).view(torch.int32)) & 0xFFFFFFFF


def cases():
    return {name: case._replace(steps=STEPS) for name, case in OC.CASES.items()}


def inputs(chunk):
    """The hashes of what a run is fed: the start values and the gradients of every case and step (host only)."""
    tensors = OC.edge_tensors(chunk)
    return {"values": {name: sha(v) for name, v in OC.values(tensors).items()},
            "gradients": {name: [{n: sha(g) for n, g in OC.gradients(tensors, case, step).items()} for step in range(1, STEPS + 1)]
                          for name, case in cases().items()}}


def run_case(case, chunk, device="cuda:0", pre_step=None):
    """STEPS steps of FullModelClipAdamW on the edge table; (optimizer, [per step: the hashes and bit patterns])."""
    from unseenobjectswithmeanshift_amd.optim import FullModelClipAdamW
    tensors = OC.edge_tensors(chunk)
    params = OC.make_params(tensors, device, torch.float32)
    opt = FullModelClipAdamW(OC.groups_of(tensors, params), max_norm=case.max_norm)
    shots = []
    for step in range(1, STEPS + 1):
        OC.set_grads(params, OC.gradients(tensors, case, step), device)
        if pre_step is not None:
            pre_step(opt)
        opt.step()
        shot = {"tensors": {}, "last_grad_norm": bits(opt.last_grad_norm), "last_clip_coef": bits(opt.last_clip_coef)}
        for name, p in params.items():
            st = opt.state.get(p, {})
            shot["tensors"][name] = dict(p=sha(p), grad=sha(p.grad), exp_avg=sha(st.get("exp_avg")), exp_avg_sq=sha(st.get("exp_avg_sq")))
        shots.append(shot)
    return opt, shots


def hipcc_version():
    try:
        out = subprocess.run(["hipcc", "--version"], capture_output=True, text=True, check=True).stdout
    except (OSError, subprocess.CalledProcessError):
        return None
    m = re.search(r"HIP version:\s*(\S+)", out)
    return m.group(1) if m else out.splitlines()[0]


def record(commit):
    from unseenobjectswithmeanshift_amd import ops
    chunk = ops.optim_chunk()
    doc = {"header": {"chunk": chunk, "steps": STEPS, "torch": torch.__version__, "hipcc": hipcc_version(), "commit": commit,
                      "device": torch.cuda.get_device_name(0)},
           "inputs": inputs(chunk), "cases": {}}
    for name, case in cases().items():
        doc["cases"][name] = run_case(case, chunk)[1]
    return doc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="id of the commit whose build is recorded (written into the header)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("record_optim_bits.py needs a GPU: the fixture holds what the kernels compute")
    doc = record(a.commit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    from unseenobjectswithmeanshift_amd import _lib
    print(f"wrote {a.out}: {len(doc['cases'])} cases x {STEPS} steps, chunk {doc['header']['chunk']}, commit {a.commit}, "
          f"library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
