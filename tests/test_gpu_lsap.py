"""The criterion's assignments on the device (pytest -m gpu): msm_lsap_match against criterion.lsap_numpy, bit for bit, on the
shared case table (tests/lsap_cases.py; scipy is the second witness where the optimum is unique), bad cost matrices inside a
good batch, and SetCriterion / training.decoder_losses with solver="device" against solver="host": same assignments, bitwise
equal losses, no host synchronisation."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lsap_cases as lc  # noqa: E402
from unseenobjectswithmeanshift_amd import criterion as cr  # noqa: E402
from unseenobjectswithmeanshift_amd import ops  # noqa: E402
from unseenobjectswithmeanshift_amd import synthetic as syn  # noqa: E402

try:
    from scipy.optimize import linear_sum_assignment as scipy_lsa
except ImportError:
    scipy_lsa = None

pytestmark = pytest.mark.gpu
DEV = "cuda"
NO_OBJECT = 7
GUARD = 3                      # sentinel rows on both sides of every output buffer
SENTINEL = -77


def _guarded(shape, dtype):
    """A sentinel-filled buffer with GUARD extra leading rows on both sides of the view the kernel writes."""
    full = torch.full((shape[0] + 2 * GUARD,) + tuple(shape[1:]), SENTINEL, dtype=dtype, device=DEV)
    return full, full[GUARD:GUARD + shape[0]]


def _run_guarded(cost, T, labels, no_object=NO_OBJECT):
    """ops.lsap_match into guarded buffers -> (pairs, target_classes, status) on the host, guards checked."""
    n_pred, Q, _ = cost.shape
    B = len(T)
    N = sum(min(Q, t) for t in T)
    fp, pairs = _guarded((n_pred * N, 4), torch.int32)
    ft, tc = _guarded((n_pred, B, Q), torch.int64)
    fs, st = _guarded((n_pred, B), torch.int32)
    got = ops.lsap_match(torch.from_numpy(cost).to(DEV), lc.toff_of(T), torch.from_numpy(labels).to(DEV), no_object,
                         out=(pairs, tc, st))
    assert got[0] is pairs and got[1] is tc and got[2] is st
    for full in (fp, ft, fs):
        assert bool((full[:GUARD] == SENTINEL).all()) and bool((full[-GUARD:] == SENTINEL).all()), "guard rows were written"
    return pairs.cpu().numpy(), tc.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("case", lc.cases(), ids=lc.case_id)
def test_lsap_match_equals_lsap_numpy(case):
    Q, T, kind, seed = case
    cost = lc.make_cost(Q, T, kind, seed)
    labels = lc.labels_of(T, seed)
    pairs, tc, st = _run_guarded(cost, T, labels)
    N = sum(min(Q, t) for t in T)
    assert pairs.shape == (lc.N_PRED * N, 4) and (st == 0).all()
    want_pairs, want_tc = lc.reference(cost, T, Q, labels, NO_OBJECT, cr.lsap_numpy)
    np.testing.assert_array_equal(pairs, want_pairs)
    np.testing.assert_array_equal(tc, want_tc)
    if kind != "ties" and scipy_lsa is not None:            # the optimum is unique (test_lsap_cases_cpu.py): scipy agrees
        sp_pairs, sp_tc = lc.reference(cost, T, Q, labels, NO_OBJECT, lambda c: scipy_lsa(c.astype(np.float64)))
        np.testing.assert_array_equal(pairs, sp_pairs)
        np.testing.assert_array_equal(tc, sp_tc)
    # the allocating form of the wrapper returns the same
    p2, t2, s2 = ops.lsap_match(torch.from_numpy(cost).to(DEV), lc.toff_of(T), torch.from_numpy(labels).to(DEV), NO_OBJECT)
    assert p2.dtype == torch.int32 and t2.dtype == torch.int64 and s2.dtype == torch.int32
    np.testing.assert_array_equal(p2.cpu().numpy(), want_pairs)
    np.testing.assert_array_equal(t2.cpu().numpy(), want_tc)
    assert s2.shape == (lc.N_PRED, len(T)) and int(s2.abs().sum()) == 0


def test_lsap_match_matrix_read_from_global_memory():
    """Q max_T above the staging limit (28672 values): the working matrix is read from `cost`, both orientations."""
    Q, T = 200, (150, 3, 201)
    cost = lc.make_cost(Q, T, "normal", 77)
    labels = lc.labels_of(T, 77)
    pairs, tc, st = _run_guarded(cost, T, labels)
    want_pairs, want_tc = lc.reference(cost, T, Q, labels, NO_OBJECT, cr.lsap_numpy)
    assert (st == 0).all()
    np.testing.assert_array_equal(pairs, want_pairs)
    np.testing.assert_array_equal(tc, want_tc)


def _bad_batch():
    """Q = 100, T = (8, 4, 6): prediction 0 holds a nan in image 0, a -inf in image 1 and an all-+inf column in image 2;
    prediction 1 is clean."""
    Q, T = 100, (8, 4, 6)
    cost = lc.make_cost(Q, T, "normal", 31)
    toff = lc.toff_of(T)
    cost[0, 57, toff[0] + 5] = np.nan
    cost[0, 3, toff[1] + 2] = -np.inf
    cost[0, :, toff[2] + 4] = np.inf
    return Q, T, cost, lc.labels_of(T, 31)


def test_lsap_match_bad_matrices_in_a_good_batch():
    Q, T, cost, labels = _bad_batch()
    toff = lc.toff_of(T)
    pairs, tc, st = _run_guarded(cost, T, labels)
    np.testing.assert_array_equal(st, [[1, 1, 2], [0, 0, 0]])
    N = sum(T)
    # prediction 0: the fallback pairs (q = j, target j), in range
    want, want_tc = [], np.full((len(T), Q), NO_OBJECT, np.int64)
    for b, t in enumerate(T):
        for j in range(t):
            want.append((0, len(want), b * Q + j, toff[b] + j))
            want_tc[b, j] = labels[toff[b] + j]
    np.testing.assert_array_equal(pairs[:N], np.array(want, np.int32))
    np.testing.assert_array_equal(tc[0], want_tc)
    assert (pairs[:, 2] >= 0).all() and (pairs[:, 2] < len(T) * Q).all() and (pairs[:, 3] >= 0).all() and (pairs[:, 3] < N).all()
    # prediction 1: solved exactly
    ref_pairs, ref_tc = lc.reference(cost[1:], T, Q, labels, NO_OBJECT, cr.lsap_numpy)
    ref_pairs[:, 0] = 1
    np.testing.assert_array_equal(pairs[N:], ref_pairs)
    np.testing.assert_array_equal(tc[1], ref_tc[0])


# ---- SetCriterion ----------------------------------------------------------------------------------------------------------
def _to_dev(outputs, targets, grad=True):
    preds = [outputs] + outputs["aux_outputs"]
    dev = [{k: v.to(DEV).requires_grad_(grad) for k, v in p.items() if k != "aux_outputs"} for p in preds]
    out = dict(dev[0])
    out["aux_outputs"] = dev[1:]
    return out, dev, [{"labels": t["labels"].to(DEV), "masks": t["masks"].to(DEV)} for t in targets]


def _criterion(generator=None, dec_layers=10, **kw):
    return cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=dec_layers,
                              generator=generator, **kw).to(DEV)


def _same_indices(a, b):
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        assert len(pa) == len(pb)
        for (i, j), (k, l) in zip(pa, pb):
            assert i.dtype == k.dtype == torch.int64 and i.device.type == "cpu"
            assert torch.equal(i, k) and torch.equal(j, l)


def _run_criterion(solver, outputs, targets, seed, **kw):
    out, preds, tg = _to_dev(outputs, targets)
    crit = _criterion(torch.Generator().manual_seed(seed), solver=solver, **kw)
    losses = crit(out, tg)
    sum(losses[k] * crit.weight_dict[k] for k in losses).backward()
    return crit, losses, preds


def test_set_criterion_device_equals_host():
    outputs, targets = syn.synth_criterion_inputs(n_pred=3, B=3, T=(0, 17, 4), Q=100, hm=60, wm=80, hg=240, wg=320, seed=5)
    kw = dict(dec_layers=3, train_num_points=2000)
    host, lh, ph = _run_criterion("host", outputs, targets, 4, **kw)
    dev, ld, pd = _run_criterion("device", outputs, targets, 4, **kw)
    assert host.last_status is None and dev.last_status.shape == (3, 3) and dev.last_status.is_cuda
    _same_indices(dev.last_indices, host.last_indices)
    assert dev.last_indices is dev.last_indices                                            # converted once
    assert list(ld) == list(lh) and len(ld) == 9
    for k in lh:
        assert torch.equal(ld[k], lh[k]), (k, float(ld[k]), float(lh[k]))                    # bitwise
    assert torch.equal(dev.last_selection, host.last_selection)
    for p in range(3):
        for name in ("pred_logits", "pred_masks"):
            want = ph[p][name].grad
            torch.testing.assert_close(pd[p][name].grad, want, rtol=1e-4, atol=1e-4 * float(want.abs().max()))
    dev.check_matching()


def test_hungarian_matcher_device_forward():
    outputs, targets = syn.synth_criterion_inputs(n_pred=1, B=3, T=(0, 17, 4), Q=100, hm=60, wm=80, hg=240, wg=320, seed=5)
    out, _, tg = _to_dev(outputs, targets, grad=False)
    got = cr.HungarianMatcher(2.0, 5.0, 5.0, num_points=500, generator=torch.Generator().manual_seed(1), solver="device")(out, tg)
    want = cr.HungarianMatcher(2.0, 5.0, 5.0, num_points=500, generator=torch.Generator().manual_seed(1))(out, tg)
    assert [len(i) for i, _ in got] == [0, 17, 4]
    for (i, j), (wi, wj) in zip(got, want):
        assert i.is_cuda and j.is_cuda and i.dtype == j.dtype == torch.int64
        assert torch.equal(i.cpu(), wi) and torch.equal(j.cpu(), wj)


def test_set_criterion_device_vs_golden(golden):
    gd = golden("set_criterion")
    seed = int(gd["seed"])
    outputs, targets = syn.synth_criterion_inputs(seed=seed)
    out, preds, tg = _to_dev(outputs, targets)
    crit = _criterion(torch.Generator().manual_seed(seed), solver="device")
    losses = crit(out, tg)
    keys = [str(k) for k in gd["loss_keys"]]
    assert list(losses) == keys
    crit.check_matching()
    for p, per in enumerate(crit.last_indices):                                            # assignments, exactly
        got = np.concatenate([np.stack([np.full(len(i), b), i.numpy(), j.numpy()], 1) for b, (i, j) in enumerate(per)])
        np.testing.assert_array_equal(got, gd["assign"][p])
    np.testing.assert_allclose(np.array([float(losses[k]) for k in keys]), gd["loss_values"], rtol=1e-4)
    total = sum(losses[k] * crit.weight_dict[k] for k in keys)
    assert abs(float(total) - float(gd["total"])) < 1e-4 * abs(float(gd["total"]))
    total.backward()
    for p in range(len(preds)):
        want = torch.from_numpy(gd["grad_logits"][p])
        torch.testing.assert_close(preds[p]["pred_logits"].grad.cpu(), want, rtol=1e-4, atol=1e-4 * float(want.abs().max()))


def test_device_solver_never_waits_for_the_gpu():
    """Targets on the device, the device generator: under torch's sync debug mode "error" a forward + backward with
    solver="device" completes, the same call with solver="host" raises."""
    outputs, targets = syn.synth_criterion_inputs(n_pred=3, B=3, T=(0, 17, 4), Q=100, hm=60, wm=80, hg=240, wg=320, seed=5)
    out, _, tg = _to_dev(outputs, targets)
    tg = [{"labels": t["labels"], "masks": t["masks"].to(torch.uint8)} for t in tg]
    crits = {s: _criterion(None, dec_layers=3, train_num_points=2000, solver=s) for s in ("host", "device")}
    for c in crits.values():                                # warm-up: lazy initialisation may synchronise once
        sum(c(out, tg).values()).backward()
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    old = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        try:
            probe.item()
            works = False
        except RuntimeError:
            works = True
        if not works:
            pytest.skip("torch.cuda.set_sync_debug_mode('error') does not flag a deliberate .item() on this build")
        losses = crits["device"](out, tg)
        sum(losses.values()).backward()
        with pytest.raises(RuntimeError):
            crits["host"](out, tg)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    crits["device"].check_matching()


def test_lazy_state_and_check_matching():
    outputs, targets = syn.synth_criterion_inputs(n_pred=2, B=3, T=(0, 17, 4), Q=100, hm=60, wm=80, hg=240, wg=320, seed=5)
    out, _, tg = _to_dev(outputs, targets, grad=False)
    crit = _criterion(torch.Generator().manual_seed(2), dec_layers=2, train_num_points=500, solver="device")
    crit(out, tg)
    pairs, toff, Q, n_pred = crit._last_pairs
    assert crit._last_indices is None and pairs.is_cuda and pairs.shape == (2 * 21, 4)
    _same_indices(crit.last_indices, cr.indices_from_pairs(pairs.cpu().numpy(), [0, 0, 17, 21], 100, 2))
    assert [len(i) for i, _ in crit.last_indices[1]] == [0, 17, 4]
    crit.check_matching()                                   # clean inputs: silent

    # the bad batch: statuses (1, 1, 2) in prediction 0; the first one is reported
    Q, T, cost, labels = _bad_batch()
    _, _, status = ops.lsap_match(torch.from_numpy(cost).to(DEV), lc.toff_of(T), torch.from_numpy(labels).to(DEV), 2)
    crit.last_status = status
    with pytest.raises(ValueError, match="nan or -inf"):
        crit.check_matching()
    crit.last_status = status[:, 2:]
    with pytest.raises(ValueError, match="infeasible"):
        crit.check_matching()
    crit.last_status = torch.tensor([[0, 3]], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="loop bound"):
        crit.check_matching()
    # a criterion call on nan predictions: the device path finishes on the fallback pairs and reports on request
    bad = {k: v.clone() for k, v in out.items() if k != "aux_outputs"}
    bad["pred_masks"][1, 5] = float("nan")
    bad["aux_outputs"] = out["aux_outputs"]
    crit(bad, tg)
    assert crit.last_status.cpu().tolist() == [[0, 1, 0], [0, 0, 0]]
    assert crit.last_indices[0][1][0].tolist() == list(range(17)) and crit.last_indices[0][1][1].tolist() == list(range(17))
    with pytest.raises(ValueError, match="nan or -inf"):
        crit.check_matching()


def test_decoder_losses_training_step_device_solver():
    from unseenobjectswithmeanshift_amd import training as tr
    from unseenobjectswithmeanshift_amd.modeling import MeanShiftTransformerDecoder
    dec = MeanShiftTransformerDecoder(in_channels=64, mask_classification=True, num_classes=2, hidden_dim=256, num_queries=100, nheads=8,
                                      dim_feedforward=2048, dec_layers=9, pre_norm=False, mask_dim=256, enforce_input_project=False)
    dec.load_state_dict(syn.synth_state_dict(syn.decoder_param_shapes()), strict=True)
    dec = dec.to(DEV)
    x, mf = syn.synth_decoder_inputs(2, 64, 96, seed=1)
    x, mf = [t.to(DEV) for t in x], mf.to(DEV)
    _, targets = syn.synth_criterion_inputs(n_pred=1, B=2, T=(3, 5), Q=100, hm=16, wm=24, hg=64, wg=96, seed=4)
    targets = [{"labels": t["labels"].to(DEV), "masks": t["masks"].to(DEV)} for t in targets]
    params = [(n, p) for n, p in dec.named_parameters() if p.requires_grad]

    def run(solver):
        crit = _criterion(torch.Generator().manual_seed(9), dec_layers=10, solver=solver)
        for _, p in params:
            p.grad = None
        losses = tr.decoder_losses(dec, x, mf, targets, crit)
        assert len(losses) == 30
        sum(losses.values()).backward()
        return crit, losses, {n: p.grad.clone() for n, p in params}

    host, lh, gh = run("host")
    dev, ld, gd = run("device")
    dev.check_matching()
    _same_indices(dev.last_indices, host.last_indices)
    for k in lh:
        assert torch.equal(ld[k], lh[k]), (k, float(ld[k]), float(lh[k]))                    # bitwise
    for name, _ in params:
        assert bool(torch.isfinite(gd[name]).all()) and float(gd[name].abs().sum()) > 0, name
        torch.testing.assert_close(gd[name], gh[name], rtol=1e-4, atol=1e-4 * float(gh[name].abs().max()), msg=lambda m: f"{name}: {m}")
