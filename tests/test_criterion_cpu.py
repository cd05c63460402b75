"""Host side of the set criterion (criterion.py), no GPU: the random-draw schedule against the reference's draws recorded in
tests/golden/set_criterion.npz, the numpy assignment solver, the weight dict, num_masks under a world-2 gloo group and the
refusal of host tensors."""
import itertools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from unseenobjectswithmeanshift_amd import criterion as cr
from unseenobjectswithmeanshift_amd import ops
from unseenobjectswithmeanshift_amd import synthetic as syn


def _criterion(generator=None, dec_layers=10):
    return cr.build_criterion(2, class_weight=2.0, mask_weight=5.0, dice_weight=5.0, no_object_weight=0.1, dec_layers=dec_layers,
                              generator=generator)


def test_draw_schedule_matches_reference(golden):
    """Every torch.rand of one reference call, in order (matcher per image, then loss_masks' oversampled and uniform points,
    final prediction first), replayed from a CPU generator with the fixture's seed."""
    gd = golden("set_criterion")
    g = torch.Generator().manual_seed(int(gd["seed"]))
    crit = _criterion(g)
    outputs, targets = syn.synth_criterion_inputs(seed=int(gd["seed"]))
    Q = outputs["pred_logits"].shape[1]
    N = sum(min(Q, len(t["labels"])) for t in targets)
    n_pred, B = 1 + len(outputs["aux_outputs"]), len(targets)
    mp_, os_, rnd = crit.draw_points(n_pred, B, N, "cpu")
    ours = []
    for p in range(n_pred):
        ours += [mp_[p, b:b + 1] for b in range(B)] + [os_[p], rnd[p]]
    assert len(ours) == len(gd["draw_sums"])
    for i, x in enumerate(ours):
        assert list(x.shape) == list(gd["draw_shapes"][i]), i
        assert float(x.double().sum()) == float(gd["draw_sums"][i]), i
        np.testing.assert_array_equal(x.reshape(-1)[:16].numpy(), gd["draw_first16"][i])
    # the generator is left where the reference left it: the next draw continues the same stream
    g2 = torch.Generator().manual_seed(int(gd["seed"]))
    for x in ours:
        torch.rand(x.shape, generator=g2)
    assert torch.equal(torch.rand(4, generator=g), torch.rand(4, generator=g2))


@pytest.mark.parametrize("shape", [(5, 5), (7, 3), (3, 7), (100, 17), (17, 100), (100, 1), (1, 1), (40, 40)])
def test_lsap_numpy_matches_scipy(shape):
    scipy_opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(sum(shape))
    for _ in range(3):
        c = rng.normal(size=shape)
        i, j = cr.lsap_numpy(c)
        si, sj = scipy_opt.linear_sum_assignment(c)
        assert len(i) == min(shape)
        assert np.all(np.diff(i) > 0)
        np.testing.assert_array_equal(i, si)
        np.testing.assert_array_equal(j, sj)


def test_lsap_numpy_brute_force_and_edges():
    rng = np.random.default_rng(3)
    for nr, nc in [(2, 2), (3, 3), (2, 4), (4, 2), (3, 5), (5, 3), (4, 4)]:
        for _ in range(5):
            c = np.round(rng.normal(size=(nr, nc)), 1)                   # ties allowed: compare the optimal total
            i, j = cr.lsap_numpy(c)
            assert len(set(i.tolist())) == len(i) == min(nr, nc) and len(set(j.tolist())) == len(j)
            if nr <= nc:
                best = min(sum(c[r, p[r]] for r in range(nr)) for p in itertools.permutations(range(nc), nr))
            else:
                best = min(sum(c[p[k], k] for k in range(nc)) for p in itertools.permutations(range(nr), nc))
            assert abs(c[i, j].sum() - best) < 1e-9
    i, j = cr.lsap_numpy(np.zeros((100, 0)))
    assert i.shape == j.shape == (0,)
    with pytest.raises(ValueError):
        cr.lsap_numpy(np.array([[np.nan, 1.0]]))


@pytest.mark.parametrize("dec_layers", [7, 10])
def test_weight_dict_matches_reference(dec_layers, golden):
    wd = _criterion(dec_layers=dec_layers).weight_dict
    expect = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    for i in range(dec_layers - 1):                                     # meanshiftformer_model.py:157-164
        expect.update({f"loss_ce_{i}": 2.0, f"loss_mask_{i}": 5.0, f"loss_dice_{i}": 5.0})
    assert wd == expect and list(wd) == list(expect)
    if dec_layers == 10:                                                # the fixture's reference call: 9 aux predictions
        assert [str(k) for k in golden("set_criterion")["loss_keys"]] == list(expect)
    crit = _criterion(dec_layers=dec_layers)
    assert crit.empty_weight.tolist() == pytest.approx([1.0, 1.0, 0.1])


def test_weighted_losses_filters_and_scales():
    from unseenobjectswithmeanshift_amd import training as tr
    got = tr.weighted_losses({"loss_ce": torch.tensor(2.0), "loss_x": torch.tensor(1.0), "loss_dice_3": torch.tensor(0.5)},
                             {"loss_ce": 2.0, "loss_dice_3": 5.0})
    assert list(got) == ["loss_ce", "loss_dice_3"] and float(got["loss_ce"]) == 4.0 and float(got["loss_dice_3"]) == 2.5


def test_num_masks_single_process():
    assert cr.average_num_masks(7) == 7.0
    assert cr.average_num_masks(0) == 1.0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, counts, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    q.put((rank, [cr.average_num_masks(c[rank]) for c in counts]))
    dist.destroy_process_group()


def test_num_masks_gloo_world2():
    """criterion.py:224-232: all-reduced, divided by the world size, clamped to 1."""
    counts = [(3, 0), (5, 8), (0, 0), (1, 0)]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, counts, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[0] == got[1] == [1.5, 6.5, 1.0, 1.0]


def test_host_tensors_raise():
    outputs, targets = syn.synth_criterion_inputs(n_pred=2, B=2, T=(2, 1), Q=8, hm=6, wm=8, hg=12, wg=16)
    with pytest.raises(RuntimeError, match="GPU"):
        _criterion(dec_layers=2)(outputs, targets)
    tgt = torch.zeros((1, 12, 16), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.match_cost([outputs["pred_logits"]], [outputs["pred_masks"]], tgt, torch.zeros(1, dtype=torch.int32), [0, 1, 1],
                       torch.rand(1, 2, 4, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.point_loss_fwd([outputs["pred_masks"]], tgt, torch.zeros((1, 4), dtype=torch.int32), torch.rand(1, 1, 6, 2),
                           torch.rand(1, 1, 1, 2), 3, 1.0)


def test_num_points_must_be_positive():
    m = cr.HungarianMatcher(1, 1, 1, num_points=0)
    outputs, targets = syn.synth_criterion_inputs(n_pred=1, B=1, T=(1,), Q=4, hm=6, wm=8, hg=12, wg=16)
    with pytest.raises(ValueError, match="num_points"):
        m(outputs, targets)
