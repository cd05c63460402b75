"""EmbeddingLoss on the GPU (csrc/embedding_loss.hip through unseenobjectswithmeanshift_amd.embedding_loss) against the float64
definition of tests/embloss_cases.py, which tests/test_embloss_cases_cpu.py pins to the reference's own module.

Bound: the project's fp32 contract (rtol 1e-4) -- each loss |delta| <= 1e-4 |ref| (a reference of exactly 0 is met
exactly), the gradient of 2 loss + 3 intra - inter max |delta| <= 1e-4 max |grad_ref| of the case.  The reference's own fp32 run
sits at ~1e-6 (losses) and ~3e-6 (gradient) of its float64 run (tests/golden/embedding_loss.npz); the kernels' figures are printed
(pytest -s) and recorded in DESIGN.md section 5r.  Needs a real MI355X (pytest -m gpu)."""
import functools

import pytest
import torch

import embloss_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-4


def _module(name, **kw):
    from unseenobjectswithmeanshift_amd.embedding_loss import EmbeddingLoss
    case = EC.CASES[name]
    return EmbeddingLoss(EC.ALPHA, case.delta, EC.LAMBDA_INTRA, EC.LAMBDA_INTER, case.metric, case.normalize, **kw)


def _run(name, weights=EC.GRAD_WEIGHTS, **kw):
    x, labels = EC.planted(name)
    x = x.to(DEV).requires_grad_(True)
    crit = _module(name, **kw)
    loss, intra, inter = crit(x, labels.to(DEV))
    (weights[0] * loss + weights[1] * intra + weights[2] * inter).backward()
    torch.cuda.synchronize()
    return dict(losses=torch.stack([loss, intra, inter]).detach().cpu(), grad=x.grad.cpu(), crit=crit,
                info={k: v.cpu() for k, v in crit.last_info.items()})


@functools.lru_cache(maxsize=None)
def _first(name):
    return _run(name)


def _check_losses(name, got, ref):
    for what, g, r in zip(("loss", "intra", "inter"), got.tolist(), (ref["loss"], ref["intra"], ref["inter"])):
        err = abs(g - r)
        print(f"embloss case {name}: {what} {g:.9g} ref {r:.9g} rel {err / abs(r) if r else err:.2e}")
        assert err <= RTOL * abs(r), (name, what, g, r)


def _check_grad(name, got, ref, what="grad"):
    gmax = float(ref["grad"].abs().max())
    err = float((got.double() - ref["grad"]).abs().max())
    print(f"embloss case {name}: {what} max|d| {err:.3e} of max|grad_ref| {gmax:.3e} -> {err / gmax if gmax else err:.2e}")
    assert err <= RTOL * gmax, (name, what, err, gmax)


@pytest.mark.parametrize("name", list(EC.CASES))
def test_matches_definition(name):
    case, ref, out = EC.CASES[name], EC.reference64(name), _first(name)
    info = out["info"]
    K = ref["K"]
    assert int(info["K"]) == K and int(info["status"]) == 0
    assert torch.equal(info["n"][:, :K].long(), ref["n"]) and torch.equal(info["N"][:, :K].long(), ref["N"])
    assert int(info["n"][:, K:].abs().sum()) == 0 and int(info["N"][:, K:].abs().sum()) == 0
    assert int(info["flag"]) == int(bool((ref["d"] > EC.ALPHA).any()))                      # the zero-intra branch
    _check_losses(name, out["losses"], ref)
    _check_grad(name, out["grad"], ref)
    unlabelled = ~ref["labelled"].reshape(case.B, case.H, case.W)
    assert float(out["grad"].permute(0, 2, 3, 1)[unlabelled].abs().max()) == 0.0            # exactly 0 on -1 pixels
    if name == "6k1":
        assert float(out["losses"].abs().max()) == 0.0 and float(out["grad"].abs().max()) == 0.0
    out["crit"].check()


@pytest.mark.parametrize("name", list(EC.CASES))
def test_second_call_is_bit_identical(name):
    a, b = _first(name), _run(name)
    assert torch.equal(a["losses"], b["losses"]) and torch.equal(a["grad"], b["grad"])
    assert all(torch.equal(a["info"][k], b["info"][k]) for k in a["info"])


@pytest.mark.parametrize("name", list(EC.CASES))
def test_separate_backwards_sum_to_the_combined(name):
    ref = EC.reference64(name)
    x, labels = EC.planted(name)
    x = x.to(DEV).requires_grad_(True)
    outs = _module(name)(x, labels.to(DEV))
    total = torch.zeros_like(x)
    for w, out in zip(EC.GRAD_WEIGHTS, outs):
        (g,) = torch.autograd.grad(out, x, retain_graph=True)
        total += w * g
    _check_grad(name, total.cpu(), ref, "sum of the three separate backward calls")


def test_status_word_reports_a_label_beyond_the_table():
    out = _run("0", max_clusters=3)                        # labels 3 and 4 do not fit a table of 3 rows
    assert int(out["info"]["status"]) & 1 and int(out["info"]["K"]) == 5
    assert bool(torch.isfinite(out["losses"]).all()) and bool(torch.isfinite(out["grad"]).all())
    with pytest.raises(ValueError, match="max_clusters"):
        out["crit"].check()
    ok = _first("0")
    assert int(ok["info"]["status"]) == 0 and int(ok["crit"].last_status.cpu()) == 0
    ok["crit"].check()


def test_no_host_synchronisation():
    x, labels = EC.planted("0")
    x, labels = x.to(DEV).requires_grad_(True), labels.to(DEV)
    crit = _module("0")
    crit(x, labels)[0].backward()                          # warm-up: first-use setup happens outside the checked region
    x.grad = None
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        with pytest.raises(RuntimeError):
            probe.item()                                   # the mode flags a deliberate synchronisation on this build
        loss, intra, inter = crit(x, labels)
        (2.0 * loss + 3.0 * intra - inter).backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    first = _first("0")
    assert torch.equal(torch.stack([loss, intra, inter]).detach().cpu(), first["losses"]) and torch.equal(x.grad.cpu(), first["grad"])


def test_graph_capture_replays_to_the_same_bits():
    from unseenobjectswithmeanshift_amd import ops
    case = EC.CASES["0"]
    x, labels = EC.planted("0")
    x, labels = x.to(DEV), labels.to(DEV).float().contiguous()
    Kt = ops.embloss_max_clusters(case.C)
    ws = torch.empty(ops.embloss_workspace_bytes(case.B, case.C, case.H * case.W, Kt), device=DEV, dtype=torch.uint8)
    gl = torch.tensor([EC.GRAD_WEIGHTS[0], EC.GRAD_WEIGHTS[1], EC.GRAD_WEIGHTS[2]], device=DEV)

    def step():                                            # one linear chain: six forward launches, one backward launch
        losses, info, _ = ops.embloss_fwd(x, labels, EC.ALPHA, case.delta, EC.LAMBDA_INTRA, EC.LAMBDA_INTER, case.metric,
                                          case.normalize, Kt, ws)
        return losses, info, ops.embloss_bwd(x, labels, gl, ws, case.metric, Kt)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [t.clone() for t in step()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    for _ in range(2):
        for t in static:
            t.zero_()
        ws.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, static))
    first = _first("0")
    assert torch.equal(static[0].cpu(), first["losses"]) and torch.equal(static[2].cpu(), first["grad"])
