"""The cosine (vMF) metric of the mean-shift clustering on the HIP path (msm_ms_select_seeds*, msm_ms_hill_climb*, msm_ms_assign,
msm_ms_connected_components; ops.ms_*, mean_shift.*) against the float64 definitions of tests/ms_cosine_cases.py, on every kernel
form: the stepwise, persistent (1, 2, 3 tiles), grouped and bf16 seeding kernels, every seed-block count of the fp32 hill climb
(both metrics), the split and bf16 climbs, the assignment's argmin, tie rule and bounds.  Needs a real MI355X (pytest -m gpu).

The float64 results come from the cached case module; tests/test_ms_cosine_cases_cpu.py checks the properties of the inputs that
the statements here rely on.  test_hill_climb prints err_gpu / err32 per case (the observed range is in the case module's header)."""
import pytest
import torch

import ms_cosine_cases as C
from oracle import msm_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from unseenobjectswithmeanshift_amd import ops as _ops
    return _ops


def ms():
    from unseenobjectswithmeanshift_amd import mean_shift as _ms
    return _ms


_X = {}


def xdev(case):
    if case not in _X:
        _X[case] = C.planted(case)[0].to(DEV)
    return _X[case]


def raw_seeds(case):
    """The float64 seeding's seeds of the case, on the device."""
    return xdev(case)[torch.from_numpy(C.seeds64(case)["idx"]).to(DEV)].contiguous()


_CONVERGED = {}


def converged(case):
    """The kernels' own seeds after 10 iterations (device), once per case."""
    if case not in _CONVERGED:
        S = C.CASES[case][3]
        seeds, idx = ops().ms_select_seeds(xdev(case), S, C.first_index(case))
        assert int(idx.min()) >= 0, "the persistent seeding kernel gave up on an idle GPU"
        _CONVERGED[case] = ops().ms_hill_climb(xdev(case), seeds, C.KAPPA, C.ITERS)
    return _CONVERGED[case]


def three_maps(case):
    """Three maps of the case's n: the case's own, its rows reversed, its rows rotated by five -> (X (3,n,64) on the host, firsts)."""
    X = C.planted(case)[0]
    n = X.shape[0]
    first = C.first_index(case)
    return torch.stack([X, X.flip(0), X.roll(5, 0)]).contiguous(), [first, n - 1 - first, (first + 5) % n]


# ---- seeding ---------------------------------------------------------------------------------------------------------------------
def check_picks(X_host, X_dev, seeds, idx, first, tol, what):
    """One form's result on its own: the first index, distinct picks, no give-up, seeds = X[idx] bit for bit, and -- replayed in
    float64 on X_host -- every pick a maximum of its step to ``tol``."""
    picks = idx.cpu().numpy()
    assert picks.min() >= 0, f"{what}: the persistent kernel gave up on an idle GPU"
    assert picks[0] == first and len(set(picks.tolist())) == len(picks)
    assert torch.equal(seeds, X_dev[idx])
    r = C.seeding64(X_host, len(picks), first, forced=picks)
    short = float((r["top"][1:] - r["pick"][1:]).max()) if len(picks) > 1 else 0.0
    print(f"{what}: largest maximum - pick {short:.2e} (tolerance {tol:.2e}), {int((r['idx'] != r['best']).sum())} picks are not the float64 argmax")
    assert (r["pick"][1:] >= r["top"][1:] - tol).all()
    return r


FORMS = ["default", "stepwise", "no_persistent", "batched", "batched_stepwise"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", range(9))                    # (case 9 is the map of case 5 with two seeds fewer)
def test_seeding_picks_a_maximum(case, form, lib_option):
    S, first = C.CASES[case][3], C.first_index(case)
    if form.startswith("batched"):
        maps, firsts = three_maps(case)
        Xd = maps.to(DEV)
        seeds, idx = ops().ms_select_seeds_batched(Xd, S, firsts, stepwise=form == "batched_stepwise")
        for m in range(3):
            check_picks(maps[m], Xd[m], seeds[m], idx[m], firsts[m], 2 * C.E, f"case {case} {form} map {m}")
        picks = idx[0]
    else:
        if form == "no_persistent":
            lib_option("MS_NO_PERSISTENT", 1)
        seeds, picks = ops().ms_select_seeds(xdev(case), S, first, stepwise=form == "stepwise")
        check_picks(C.planted(case)[0], xdev(case), seeds, picks, first, 2 * C.E, f"case {case} {form}")
    if case in C.EXACT_SEEDING:                                   # the float64 picks are the only legitimate ones
        assert picks.cpu().tolist() == C.seeds64(case)["idx"].tolist()


@pytest.mark.parametrize("tag", ["ng2", "ng3"])
def test_seeding_persistent_two_and_three_tiles(tag):
    X = C.planted(tag)[0]
    Xd = X.to(DEV)
    S, first = C.SEED_MAPS[tag][3], C.first_index(tag)
    seeds, idx = ops().ms_select_seeds(Xd, S, first)
    check_picks(X, Xd, seeds, idx, first, 2 * C.E, f"map {tag} persistent")


@pytest.mark.parametrize("stepwise", [False, True])
def test_seeding_bf16_picks_a_maximum(stepwise):
    """The bf16 forms work on the rounded points: the replay is on those, E scaled by the largest rounded row's norm; the seeds that
    come back are rows of the fp32 map."""
    X, Xr = C.planted("bf16")[0], C.planted_bf16("bf16")
    Xd = X.to(DEV)
    S, first = C.SEED_MAPS["bf16"][3], C.first_index("bf16")
    xb = ops().ms_pack_bf16(Xd)
    assert torch.equal(xb[:X.shape[0]].float().cpu(), Xr)
    seeds, idx = ops().ms_select_seeds(Xd, S, first, xb=xb, stepwise=stepwise)
    nmax = float(Xr.double().norm(dim=1).max())
    check_picks(Xr, Xd, seeds, idx, first, 2 * C.bound(nmax, nmax), f"bf16 map stepwise={stepwise}")


# ---- hill climb ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, C.ITERS])
@pytest.mark.parametrize("case", C.ALL)
def test_hill_climb(case, iters):
    """max |Z - Z64| <= max(4 err32, 2^-22), err32 the CPU fp32 evaluation of the definition.  One iteration: ten contract and
    hide a per-iteration error.  The last seed of a case with S > 1 is the far seed, which meets the bound of its own row."""
    h = C.hill_case(case, iters)
    X, Z0 = xdev(case), h["Z0"].to(DEV)
    Z = ops().ms_hill_climb(X, Z0, C.KAPPA, iters, precision="f32")
    diff = (Z.cpu().double() - h["Z64"]).abs()
    err = float(diff.max())
    print(f"case {case} iters {iters}: err_gpu {err:.3e}  err32 {h['err32']:.3e}  err_gpu / err32 {err / h['err32']:.2f}  "
          f"bound {C.hill_bound(h['err32']):.3e}")
    assert torch.isfinite(Z).all()
    assert err <= C.hill_bound(h["err32"])
    if C.CASES[case][3] > 1 and iters == 1:
        far = float(diff[-1].max())
        print(f"case {case}: far seed err_gpu {far:.3e}  err32 {h['err32_far']:.3e}")
        assert far <= C.hill_bound(h["err32_far"])
    assert float((Z.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    assert torch.equal(Z0.cpu(), h["Z0"])                                                  # the input is not modified
    assert torch.equal(Z, ops().ms_hill_climb(X, Z0, C.KAPPA, iters, precision="f32"))     # two runs, bit for bit


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_hill_climb_every_seed_block_count(metric, lib_option):
    """ms_hill_kernel<NSB> for NSB = 1 .. 8, one iteration on 304 seeds.  MS_CHUNK = 1 .. 8 caps the seed blocks per launch (19
    blocks: the launches come out 1, 2, 3, 4, 5, 5, 7, 7 wide and narrower at the end); the first 16 k seeds launched on their own
    take NSB = k exactly.  Every run meets the float64 bound.  A seed's arithmetic does not depend on the launch that carries it
    (the same grid and slab walk, accumulators per seed block, the same order over waves and workgroups): all runs are bit-equal."""
    from unseenobjectswithmeanshift_amd import _lib
    if metric == "cosine":
        h = C.hill_case(C.LIMIT, 1)
        X, Z0, Z64, bound = xdev(C.LIMIT), h["Z0"].to(DEV), h["Z64"], C.hill_bound(h["err32"])
    else:
        h = C.euclid_limit_case()
        X, Z0, Z64, bound = h["X"].to(DEV), h["Z0"].to(DEV), h["Z64"], max(4 * h["err32"], 5e-7)       # the Euclidean test's bound
    runs = []
    for cap in range(1, 9):
        lib_option("MS_CHUNK", cap)
        Z = ops().ms_hill_climb(X, Z0, C.KAPPA, 1, metric=metric)
        err = float((Z.cpu().double() - Z64).abs().max())
        print(f"{metric} MS_CHUNK {cap} (launches {C.launch_widths(304, cap)}): err_gpu {err:.3e}  bound {bound:.3e}")
        assert err <= bound
        runs.append(Z)
    lib_option("MS_CHUNK", _lib.OPT_AUTO)
    for k in range(1, 9):
        Zk = ops().ms_hill_climb(X, Z0[:16 * k].contiguous(), C.KAPPA, 1, metric=metric)
        assert float((Zk.cpu().double() - Z64[:16 * k]).abs().max()) <= bound
        assert torch.equal(Zk, runs[0][:16 * k]), f"NSB = {k} differs from NSB = 1"
    for cap in range(2, 9):
        assert torch.equal(runs[cap - 1], runs[0]), f"MS_CHUNK = {cap} differs from MS_CHUNK = 1"


LOW = [1, 2, 7, 9, 6, 8]     # n = 15, 16, 32789; S = 48, 128, 129 (case 7 again), 304


@pytest.mark.parametrize("iters", [1, C.ITERS])
@pytest.mark.parametrize("case", LOW)
def test_hill_climb_split(case, iters):
    """The split kernel is no further from float64 than 1.5 x the fp32 kernel, which is itself within the bound of test_hill_climb:
    absolutely, max(1.5 max(4 err32, 2^-22), 2e-7)."""
    h = C.hill_case(case, iters)
    X, Z0 = xdev(case), h["Z0"].to(DEV)
    z32 = ops().ms_hill_climb(X, Z0, C.KAPPA, iters).cpu().double()
    zsp = ops().ms_hill_climb(X, Z0, C.KAPPA, iters, precision="f32_split")
    e32, esp = float((z32 - h["Z64"]).abs().max()), float((zsp.cpu().double() - h["Z64"]).abs().max())
    print(f"case {case} iters {iters}: err fp32 MFMA {e32:.3e}  split {esp:.3e}  err32 {h['err32']:.3e}")
    assert e32 <= C.hill_bound(h["err32"])
    assert esp <= max(1.5 * e32, 2e-7) and esp <= max(1.5 * C.hill_bound(h["err32"]), 2e-7)
    assert float((zsp.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    assert torch.equal(zsp, ops().ms_hill_climb(X, Z0, C.KAPPA, iters, precision="f32_split")) and torch.equal(Z0.cpu(), h["Z0"])


@pytest.mark.parametrize("iters", [1, C.ITERS])
@pytest.mark.parametrize("case", LOW)
def test_hill_climb_bf16(case, iters):
    """Against the float64 iteration on the ROUNDED points what is left is the rounding of the weights to bf16 (2^-9 each, averaged
    over a cluster's points): 2e-3; against the exact points the points' own rounding comes on top: 4e-3."""
    h = C.hill_case(case, iters)
    X, Z0 = xdev(case), h["Z0"].to(DEV)
    xb = ops().ms_pack_bf16(X)
    z = ops().ms_hill_climb(X, Z0, C.KAPPA, iters, precision="bf16", xb=xb)
    er = float((z.cpu().double() - C.hill_case_bf16(case, iters)).abs().max())
    ex = float((z.cpu().double() - h["Z64"]).abs().max())
    print(f"case {case} iters {iters}: bf16 climb err on the rounded points {er:.2e}, on the exact points {ex:.2e}")
    assert er < 2e-3 and ex < 4e-3
    assert float((z.double().norm(dim=1) - 1).abs().max()) < 1e-5
    assert torch.equal(z, ops().ms_hill_climb(X, Z0, C.KAPPA, iters, precision="bf16")) and torch.equal(Z0.cpu(), h["Z0"])


# ---- assignment ------------------------------------------------------------------------------------------------------------------
def check_argmin(case, Z):
    """ms_assign on distinct seeds with one label per seed: every label a nearest seed to 2 E, the float64 argmin wherever the
    runner-up is more than 2 E away, counts = bincount(labels)."""
    X = xdev(case)
    S = Z.shape[0]
    labels, counts = ops().ms_assign(X, Z, torch.arange(S, device=DEV, dtype=torch.int64), S)
    taken = labels.cpu()
    assert int(taken.min()) >= 0 and int(taken.max()) < S
    chk = C.assign_check(C.planted(case)[0], Z.cpu(), taken)
    assert chk["admissible"] and chk["exact"], f"{chk['bad']} points took a seed that is not the nearest"
    assert torch.equal(counts.cpu(), torch.bincount(taken, minlength=S))
    return taken


@pytest.mark.parametrize("case", C.ALL)
def test_assign_raw_seeds(case):
    """(a) On the raw seeds the seeds are distinct and at most 0.54 % of the points ambiguous: the argmin is visible."""
    check_argmin(case, raw_seeds(case))


@pytest.mark.parametrize("case", C.MULTI)
def test_assign_seeds_behind_the_points(case):
    """Seeds that most points have behind them (every distance above 0.5): the zero rows that pad the seed tile are nearer than any
    seed and must not win."""
    check_argmin(case, C.behind_seeds(case).to(DEV))


@pytest.mark.parametrize("case", C.MULTI)
def test_assign_converged_seeds(case):
    """(b) On the converged seeds with the merged labels: every label is the merged label of an admissible seed, and the partition is
    the planted one."""
    X, Z = xdev(case), converged(case)
    S = Z.shape[0]
    merged, num = ops().ms_connected_components(Z, C.EPS)
    labels, counts = ops().ms_assign(X, Z, merged, S)
    d = C.dist64(C.planted(case)[0], Z.cpu())
    allowed = d <= d.min(dim=1, keepdim=True).values + 2 * C.E
    hit = merged.cpu()[None, :] == labels.cpu()[:, None]
    assert bool((allowed & hit).any(dim=1).all())
    assert torch.equal(counts.cpu(), torch.bincount(labels.cpu(), minlength=S))
    assert C.same_partition(labels.cpu(), C.planted(case)[1]) and int(num[0]) == C.CASES[case][1]


def test_assign_ties_take_the_first():
    """(c) Seed rows copied bit for bit onto later rows -- another lane of the same block, the same lane of the next block, the same
    place in the next chunk: the first argmin wins, no point takes a copy."""
    Z = C.tie_seeds().to(DEV)
    taken = check_argmin(C.LIMIT, Z)
    want = torch.argmin(C.dist64(C.planted(C.LIMIT)[0], Z.cpu()), dim=1)
    for src, dst in C.TIES:
        assert int((taken == dst).sum()) == 0, f"{int((taken == dst).sum())} points took the copy {dst} of seed {src}"
        assert torch.equal(taken == src, want == src)             # no other seed is within 2 E for the points these seeds win


@pytest.mark.parametrize("case", [4, 7])                          # n = 31, n = 32789
def test_assign_writes_n_labels(case):
    """(d) msm_ms_assign itself, on label buffers with 16 sentinel entries behind the last row: one map, and two maps, whose labels
    lie n apart (the second map's rows are the first's reversed: every row of the pair is checked against the one-map call)."""
    o = ops()
    X, Z = xdev(case), raw_seeds(case)
    n, S = X.shape[0], Z.shape[0]
    sl = torch.arange(S, device=DEV, dtype=torch.int64)
    want, want_counts = o.ms_assign(X, Z, sl, S)
    for M in (1, 2):
        Xm = torch.stack([X, X.flip(0)][:M]).contiguous()
        Zm, slm = Z[None].expand(M, -1, -1).contiguous(), sl[None].expand(M, -1).contiguous()
        buf = torch.full((M * n + 16,), -7, device=DEV, dtype=torch.int64)
        counts = torch.empty((M, S), device=DEV, dtype=torch.int64)
        o.check(o.lib().msm_ms_assign(o._p(Xm), M, n, 64, o._p(Zm), S, o._p(slm), o._p(buf), o._p(counts), S, o._stream()), "msm_ms_assign")
        assert bool((buf[M * n:] == -7).all()), "rows past n were written"
        assert torch.equal(buf[:n], want) and torch.equal(counts[0], want_counts)
        if M == 2:
            assert torch.equal(buf[n:2 * n], want.flip(0)) and torch.equal(counts[1], want_counts)


# ---- merge and end to end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.MULTI)
def test_connected_components(case):
    Z = converged(case)
    labels, num = ops().ms_connected_components(Z, C.EPS)
    assert C.eps_margin(Z.cpu()) >= 1e-4                          # no pair of seeds sits on the threshold
    want = O.connected_components(Z.cpu(), C.EPS)
    assert torch.equal(labels.cpu(), want) and int(num[0]) == len(torch.unique(want))
    assert torch.equal(ms().connected_components(Z, C.EPS), labels)


@pytest.mark.parametrize("precision", ["f32", "f32_split", "bf16"])
@pytest.mark.parametrize("case", C.MULTI)
def test_smart_init_recovers_the_planted_partition(case, precision):
    S, first = C.CASES[case][3], C.first_index(case)
    labels, sel = ms().mean_shift_smart_init(xdev(case), kappa=C.KAPPA, num_seeds=S, max_iters=C.ITERS, first_index=first,
                                             precision=precision)
    labels = labels.cpu()
    assert int(sel[0]) == first and int(sel.min()) >= 0 and sel.unique().numel() == S
    assert C.same_partition(labels, C.planted(case)[1])
    assert int(torch.bincount(labels).argmax()) == 0              # the largest cluster is label 0
    if precision != "bf16":                                       # the float64 pipeline's labels, when the seeds are the same
        own = C.smart_init64(case)
        if torch.equal(sel.cpu(), own["sel"]):
            assert torch.equal(labels, own["labels"])


@pytest.mark.parametrize("case", C.MULTI)
def test_smart_init_batched_equals_per_map(case):
    maps, firsts = three_maps(case)
    X = maps.to(DEV)
    S = C.CASES[case][3]
    labels, sel = ms().mean_shift_smart_init_batched(X, kappa=C.KAPPA, num_seeds=S, max_iters=C.ITERS, first_indices=firsts)
    assert int(sel.min()) >= 0
    for m in range(3):
        l1, s1 = ms().mean_shift_smart_init(X[m], kappa=C.KAPPA, num_seeds=S, max_iters=C.ITERS, first_index=firsts[m])
        assert torch.equal(labels[m], l1) and torch.equal(sel[m], s1)
