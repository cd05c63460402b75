"""The optimizer cases decide what they claim to decide (tests/optim_cases.py), checked on the float64 reference alone, and
torch's own fp32 CPU run of the same cases meets the contract the GPU path is held to (its figures, printed with -s, stand beside
the kernels' in DESIGN.md).  No GPU and no library: the chunk size is read from the header."""
import json
import os
import sys

import pytest
import torch

import optim_cases as OC
from unseenobjectswithmeanshift_amd import _lib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_optim_bits as RB  # noqa: E402


def header_chunk():
    with open(_lib.HEADER_PATH) as f:
        return _lib._define(f.read(), "MSM_OPTIM_CHUNK")


CHUNK = header_chunk()


def test_chunk_is_whole_vector_rounds():
    assert CHUNK % 1024 == 0 and CHUNK >= 1024


def test_the_edge_table_covers_the_paths():
    tensors = OC.edge_tensors(CHUNK)
    assert [t.numel for t in tensors[:8]] == [1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
    assert any(t.offset_p and t.offset_g for t in tensors) and any(t.offset_p and not t.offset_g for t in tensors)
    params = OC.make_params(tensors, "cpu", torch.float32)
    assert all(params[t.name].data_ptr() % 16 == (4 if t.offset_p else 0) for t in tensors)
    rows = [OC.groups_of(tensors, params)[i] for i in range(3)]
    assert len({(r["lr"], r["weight_decay"], r["betas"]) for r in rows}) == 3 and all(1e-2 <= r["lr"] <= 1e-1 for r in rows)


def test_clip_regimes_are_what_they_say():
    shots = {name: OC.reference64(name, CHUNK) for name in OC.CASES}
    assert float(shots["clip_active"][0]["total_norm"]) > 1e3 * 0.01 and float(shots["clip_active"][0]["coef"]) < 1e-3
    assert len(shots["clip_active"]) == 3 and shots["clip_active"][1]["skip"]["grad"] is None
    assert float(shots["clip_active"][1]["skip"]["update"].abs().max()) == 0.0
    assert float(shots["clip_idle"][0]["total_norm"]) < 1.0 and float(shots["clip_idle"][0]["coef"]) == 1.0
    norm, coef = float(shots["clip_eps"][0]["total_norm"]), float(shots["clip_eps"][0]["coef"])
    assert abs(norm - 2e-5) < 1e-9 and abs(coef - 1e-5 / 2.1e-5) < 1e-6
    assert abs(1e-5 / norm - coef) > 400 * OC.RTOL * coef                 # without the 1e-6: 5 % off, 400 x the contract
    assert float(shots["zero_grads"][0]["total_norm"]) == 0.0 and float(shots["zero_grads"][0]["coef"]) == 1.0
    assert all(float(s["exp_avg"].abs().max()) == 0.0 for k, s in shots["zero_grads"][0].items() if isinstance(s, dict))
    assert shots["no_clip"][0]["total_norm"] is None and float(shots["no_clip"][0]["coef"]) == 1.0


def test_eps_placement_moves_the_update_by_more_than_ten_contracts():
    for name, (gap, to_torch, scale) in OC.eps_placement_gap(CHUNK).items():
        assert to_torch <= 1e-12 * scale, (name, to_torch, scale)         # adamw64 is torch's formula
        assert gap > 10 * OC.RTOL * scale, (name, gap, scale)             # otherwise the case decides nothing


def test_the_recorded_adamw_bits_are_of_these_cases_and_complete():
    """tests/golden/optim_adamw_bits.json (tools/record_optim_bits.py, recorded on a GPU) was fed what the cases produce here, and
    holds every (case, step, tensor, quantity) that tests/test_gpu_optim_scaler.py compares: that test cannot pass on an empty or
    stale file."""
    with open(RB.DEFAULT_OUT) as f:
        fixture = json.load(f)
    header = fixture["header"]
    assert header["chunk"] == CHUNK and header["steps"] == RB.STEPS == 3
    assert all(header.get(k) for k in ("torch", "hipcc", "commit")) and len(header["commit"]) == 40
    assert fixture["inputs"] == RB.inputs(CHUNK), "the start values or gradients changed: re-record on the recorded commit's arithmetic"
    tensors = OC.edge_tensors(CHUNK)
    assert set(fixture["cases"]) == set(OC.CASES) == set(fixture["inputs"]["gradients"])
    is_sha = lambda h: isinstance(h, str) and len(h) == 64 and set(h) <= set("0123456789abcdef")
    for name, case in RB.cases().items():
        shots = fixture["cases"][name]
        assert len(shots) == RB.STEPS, name
        seen = set()                                                  # tensors that have had a gradient: they have state
        for step, shot in enumerate(shots, 1):
            assert set(shot) == {"tensors", "last_grad_norm", "last_clip_coef"}, (name, step)
            assert all(isinstance(shot[q], int) and 0 <= shot[q] < 2 ** 32 for q in ("last_grad_norm", "last_clip_coef")), (name, step)
            assert set(shot["tensors"]) == {t.name for t in tensors}, (name, step)
            for t in tensors:
                absent = t.name in case.skip.get(step, ())
                seen |= set() if absent else {t.name}
                row = shot["tensors"][t.name]
                assert set(row) == set(RB.QUANTITIES), (name, step, t.name)
                assert is_sha(row["p"]), (name, step, t.name, "p")
                assert (row["grad"] is None) if absent else is_sha(row["grad"]), (name, step, t.name, "grad")
                for q in ("exp_avg", "exp_avg_sq"):
                    assert is_sha(row[q]) if t.name in seen else row[q] is None, (name, step, t.name, q)
        # a step moves every parameter that had a gradient (lr >= 0.03 in every row; zero gradients move only the decayed ones), and
        # leaves one without as it was
        for t in tensors:
            ps = [fixture["inputs"]["values"][t.name]] + [shot["tensors"][t.name]["p"] for shot in shots]
            for step in range(1, RB.STEPS + 1):
                if t.name in case.skip.get(step, ()):
                    assert ps[step] == ps[step - 1], (name, step, t.name)
                elif case.grads[0] != "zero":
                    assert ps[step] != ps[step - 1], (name, step, t.name)


@pytest.mark.parametrize("name", list(OC.CASES))
def test_torch_fp32_on_the_cpu_meets_the_contract(name):
    case = OC.CASES[name]
    shots = OC.run(OC.edge_tensors(CHUNK), case, lambda groups: OC.ClippedTorchAdamW(groups, case.max_norm, foreach=False),
                   dtype=torch.float32)[2]
    for step, (got, ref) in enumerate(zip(shots, OC.reference64(name, CHUNK)), 1):
        OC.compare(got, ref, f"torch fp32 cpu, {name} step {step}")
