#!/usr/bin/env python
"""Headline benchmark: MSMFormer inference hot path, images/sec at 640x480, 100 queries, 9 decoder
layers (BASELINE.json).  One step = one pass of the hot path (MSDeformAttn pixel decoder ->
hypersphere transformer decoder -> instance post-processing) over one batch of 8 synthetic frames'
backbone features that are already resident in HBM.  Backbone excluded.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

* A plain run sets up, warms up (W steps), times exactly K steps, writes the last step's outputs when ``--dump-outputs DIR`` is
  given and prints the line: `value` (images/s), `ms_per_step` (one timed step), `steps` = K.
* ``--dump-outputs DIR``: what the timed path returned for its last step (scores, classes, boxes, query indices, a fixed seeded
  sample of the masks and every mask's area) as DIR/<name>.npy in float32 / float64.  The inputs are seeded: two builds run with
  the same arguments can be compared output for output.
* ``--full`` adds everything beyond the headline figure, listed below: the one-batch-in-flight figure, per-kernel timings and
  rooflines, the 16-bit plans (configs[2]), the mean-shift unit, configs[1..4] sub-results and the CPU baseline.
* ``--gpus N`` (N > 1) launched WITHOUT torch.distributed.run starts the N ranks itself (one process per GPU,
  LOCAL_RANK = device index, rendezvous on 127.0.0.1) -- the reference starts its N workers from one command the same way
  (MSMFormer/tabletop_train_net_pretrained.py:326-336).  Under ``python -m torch.distributed.run --nproc-per-node N ...
  bench.py --gpus N`` the ranks already exist (WORLD_SIZE is set) and nothing is spawned.
* Weak scaling: every rank processes its own batches of 8 images (independent units, no data-path collective); ranks
  exchange one small metrics record (images, elapsed, checksum) by all_gather after the timed region.
* Throughput mode by default: ``--inflight`` (4) batches of 8 are in flight at a time, each replayed from its own HIP graph
  on its own stream (graphs.PipelinedInference).  Under ``--full`` the JSON line also carries the figure with ONE batch in flight
  (``one_batch_in_flight``); ``--inflight 1`` times only that.
* The headline times exactly K steps (``steps`` = ``steps_requested`` = K).  Under ``--full`` the one-batch figure and the precision legs
  time at least ``--min-seconds`` (1 s) each.
* ``roofline`` (``--full``): the dominant kernel of the step by time, the fused encoder-layer tail (msm_encoder_block_fwd): FLOPs it executes /
  its mean launch duration (HIP events around graph replays of the step's six launches) / the fp32 MFMA peak, PMC traffic from
  profiles/step_traffic.json.  ``roofline.mask_step``: the Q x pixel-embedding mask step the metric names -- the full-resolution
  kernel characterised per launch, and what the default plan runs for the ten predictions (one full-resolution launch + nine at
  key resolution) with executed and reference FLOPs side by side.
* ``--full`` with N = 1 adds, on rank 0: ``kernels`` (event-timed per entry point of one eager pass), ``mean_shift`` (the classic UCN
  clustering unit with its own roofline entries), ``configs`` (BASELINE configs[2] slice / [3] / [4] timed by this run)
  and ``cpu_baseline`` (the oracle on the host cores).

Prints ONE JSON line on rank 0, at most 8000 bytes (compact_line): the contract's keys, a flat `roofline` and `cpu_baseline`, a short
`collective` and `summary`.  Under ``--full`` the full document (`kernels`, `configs`, `mean_shift`, per-rank detail) is written to
bench_out/bench_full.json (--detail).
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

# PipelinedInference keeps `--inflight` batches on separate HIP streams; with the runtime's default of 4 hardware queues a
# fifth stream shares a queue with another one and the two serialise (measured: 3 in flight 3.39k images/s with 8 queues,
# 3.08k with 4).  Must be set before the HIP runtime initialises.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32, 256 FLOP/clk/CU x 256 CUs x 2.4 GHz
PEAK_BF16_MFMA_TFLOPS = 2516.6   # same guide: dense bf16 MFMA (16x16x32), no sparsity
PEAK_HBM_GBPS = 8000.0
H, W, Q, C_MASK, BATCH = 480, 640, 100, 256, 8
METRIC = "images/sec @640x480 RGB-D, 100 queries, 9 decoder layers; % MFMA roofline"


def build_model(dev, num_queries=Q, dec_layers=9):
    from unseenobjectswithmeanshift_amd import synthetic as syn
    from unseenobjectswithmeanshift_amd.meta_arch import MeanShiftMaskFormer, build_resnet50_head
    head = build_resnet50_head(num_queries=num_queries, dec_layers=dec_layers)
    head.pixel_decoder.load_state_dict(syn.synth_state_dict(syn.pixel_decoder_param_shapes()), strict=True)
    head.predictor.load_state_dict(syn.synth_state_dict(syn.decoder_param_shapes(num_queries=num_queries, dec_layers=dec_layers)), strict=True)
    return MeanShiftMaskFormer(backbone=None, sem_seg_head=head.to(dev).eval(), num_queries=num_queries)


# ----------------------------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` starts N ranks
# ----------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n, argv):
    """Start `n` copies of this script as ranks 0..n-1 of one job (one process per GPU) and wait for them.  Rank 0 inherits
    stdout (the JSON line); a failing rank takes the others down.  Returns the exit code."""
    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env,
                                      stdout=None if r == 0 else subprocess.DEVNULL))
    rc = 0
    try:
        pending = set(range(n))
        while pending:
            for r in list(pending):
                code = procs[r].poll()
                if code is None:
                    continue
                pending.discard(r)
                if code != 0 and rc == 0:
                    rc = code
                    print(f"bench.py: rank {r} exited with code {code}; stopping the other ranks", file=sys.stderr, flush=True)
                    for o in pending:
                        procs[o].terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


# ----------------------------------------------------------------------------------------------------------------------
# CPU baseline (oracle as the thing TIMED on the host cores -- never on the product path)
# ----------------------------------------------------------------------------------------------------------------------
def cpu_baseline(iters=10, budget_s=28.0):
    """The oracle (CPU port of the reference algorithm, parity-pinned to reference goldens) on the host cores of this box,
    per piece as SURVEY 8d prescribes: pixel decoder / decoder / post-process at 640x480, batch 1 like the reference
    predictor (test_utils.py:165), and the classic mean-shift clustering at n = 307 200 (lib/utils/mean_shift.py:192-229) --
    3 warm-up + `iters` timed iterations each, MEDIAN reported.  Bounded: the whole leg stays within about `budget_s` seconds
    of CPU work (the mean-shift leg takes fewer iterations when the host is slow, and says how many)."""
    import statistics
    from oracle import msm_oracle as O
    from unseenobjectswithmeanshift_amd import synthetic as syn
    ncpu = os.cpu_count() or 1
    pd_sd = syn.synth_state_dict(syn.pixel_decoder_param_shapes())
    dec_sd = syn.synth_state_dict(syn.decoder_param_shapes())
    t_start = time.perf_counter()

    def one(seed):
        """-> seconds of (pixel decoder, decoder, post-process) for one frame"""
        feats = syn.synth_backbone_features(1, H, W, seed=seed)
        t0 = time.perf_counter()
        mf, _, ms = O.pixel_decoder_forward(pd_sd, feats)
        t1 = time.perf_counter()
        out = O.decoder_forward(dec_sd, ms, mf)
        t2 = time.perf_counter()
        O.instance_inference(out["pred_logits"][0], out["pred_masks"][0], (H, W), topk=20)
        return t1 - t0, t2 - t1, time.perf_counter() - t2

    # pick the intra-op thread count that serves this workload best (all hardware threads is rarely it
    # for torch's CPU kernels at these sizes); the choice is reported in `cores`
    best, sweep = None, {}
    for nt in sorted({min(ncpu, c) for c in (16, 32, 64)}):
        torch.set_num_threads(nt)
        one(100)                       # warm-up at this thread count
        t = sum(one(100))
        sweep[str(nt)] = round(1.0 / t, 3)
        if best is None or t < best[0]:
            best = (t, nt)
    warm, nt = best
    torch.set_num_threads(nt)
    for i in range(2):
        one(100)                       # 3 warm-up frames at the chosen thread count in all (one in the sweep)
    n_it = max(3, min(iters, int(0.45 * budget_s / max(warm, 1e-3))))
    samples = [one(101 + i) for i in range(n_it)]
    med = lambda xs: statistics.median(xs)
    t_pd, t_dec, t_post = (med([s_[i] for s_ in samples]) for i in range(3))
    t_e2e = med([sum(s_) for s_ in samples])
    # mean shift, its own unit (images/sec of the clustering of one 640x480 embedding map)
    X, _ = syn.synth_unit_embeddings(H * W, 64, clusters=12, sigma=0.15, seed=3)
    t0 = time.perf_counter()
    O.mean_shift_smart_init(X, 20.0, 100, 10, 7)
    t_first = time.perf_counter() - t0
    left = budget_s - (time.perf_counter() - t_start)
    n_ms = max(1, min(iters, int(left / max(t_first, 1e-3))))
    ms_samples = []
    for _ in range(n_ms):
        t0 = time.perf_counter()
        O.mean_shift_smart_init(X, 20.0, 100, 10, 7)
        ms_samples.append(time.perf_counter() - t0)
    t_ms = med(ms_samples)
    return {"value": round(1.0 / t_e2e, 4), "unit": "images/sec", "cores": torch.get_num_threads(), "host_cpus": ncpu,
            "threads_sweep_images_per_sec": sweep, "kind": "port", "statistic": "median", "iterations": n_it,
            "pieces": {"pixel_decoder_ms": round(1e3 * t_pd, 2), "decoder_ms": round(1e3 * t_dec, 2), "post_process_ms": round(1e3 * t_post, 2),
                       "end_to_end_ms": round(1e3 * t_e2e, 2)},
            "mean_shift": {"value": round(1.0 / t_ms, 4), "unit": "images/sec", "ms_per_image": round(1e3 * t_ms, 1), "iterations": n_ms,
                           "workload": "mean_shift_smart_init on n=307200 unit 64-d embeddings (12 planted clusters), 100 seeds, 10 iterations, kappa 20"},
            "sample_short": f"median of {n_it} frames 640x480, batch 1, oracle pixel decoder + decoder + post-process, {torch.get_num_threads()} threads; ~{int(time.perf_counter() - t_start)} s CPU",
            "sample": f"median of {n_it} frames at 640x480 (3 warm-up frames; thread-count sweep 16/32/64, best kept: "
                      f"{torch.get_num_threads()} threads of {ncpu} host CPUs), batch 1, oracle pixel decoder + 9-layer decoder + instance "
                      f"post-processing in fp32 torch, timed per piece; mean shift: median of {n_ms} clusterings of one 640x480 map after one warm-up"}


def pin_to_gpu_numa_node(local_rank):
    """One process per GPU: keep the rank's host threads on the CPUs of the NUMA node its GPU hangs off (launch and
    event-polling latency; on an 8-GPU node the default is whatever core the launcher forked on).  Returns a description for
    the JSON line with a ``status``: "pinned", "no-topology" (the sysfs files are not there, e.g. in a container: nothing to
    pin to) or "failed: ..." (the topology is there and the pin did not take -- main() refuses to time a multi-rank job then)."""
    try:
        props = torch.cuda.get_device_properties(local_rank)
        bdf = f"{getattr(props, 'pci_domain_id', 0):04x}:{props.pci_bus_id:02x}:{props.pci_device_id:02x}.0"
    except (AttributeError, RuntimeError) as e:
        return {"status": f"no-topology (device properties: {e})"}
    try:
        with open(f"/sys/bus/pci/devices/{bdf}/numa_node") as f:
            node = int(f.read().strip())
    except (OSError, ValueError):
        return {"status": "no-topology", "pci": bdf}
    if node < 0:
        return {"status": "no-topology", "pci": bdf, "numa_node": node}
    try:
        with open(f"/sys/devices/system/node/node{node}/cpulist") as f:
            cpus = set()
            for part in f.read().strip().split(","):
                lo, _, hi = part.partition("-")
                cpus.update(range(int(lo), int(hi or lo) + 1))
        allowed = cpus & os.sched_getaffinity(0)
        if not allowed:
            return {"status": f"failed: none of NUMA node {node}'s {len(cpus)} CPUs is in this process's affinity mask", "pci": bdf, "numa_node": node}
        os.sched_setaffinity(0, allowed)
        if os.sched_getaffinity(0) != allowed:
            return {"status": "failed: sched_setaffinity did not take", "pci": bdf, "numa_node": node}
        return {"status": "pinned", "pci": bdf, "numa_node": node, "cpus": len(allowed)}
    except (OSError, ValueError) as e:
        return {"status": f"failed: {e}", "pci": bdf, "numa_node": node}


# ----------------------------------------------------------------------------------------------------------------------
# measurement helpers
# ----------------------------------------------------------------------------------------------------------------------
def load_traffic(name, notes):
    """profiles/<name> (PMC byte counts of an earlier rocprofv3 pass: they cannot be collected in-process) -- or None when the file
    is missing, carries no stamp, or was collected on kernel sources that have been edited since (SHA-256 of csrc/<kernel>.hip
    recorded by tools/summarize_profile.py): a stale count is reported as `traffic: null`, with the reason in the line."""
    import hashlib
    try:
        with open(os.path.join(ROOT, "profiles", name)) as f:
            tab = json.load(f)
    except (OSError, ValueError):
        notes.append(f"{name}: missing")
        return None
    st = tab.get("stamp") or {}
    shas = st.get("kernel_source_sha256")
    if not shas:
        notes.append(f"{name}: no provenance stamp")
        return None
    for src, want in shas.items():
        try:
            with open(os.path.join(ROOT, "unseenobjectswithmeanshift_amd", "csrc", src), "rb") as f:
                have = hashlib.sha256(f.read()).hexdigest()
        except OSError:
            have = None
        if have != want:
            notes.append(f"{name}: {src} changed since commit {st.get('commit')} (the counter pass must be re-run)")
            return None
    notes.append(f"{name}: collected on commit {st.get('commit')}, kernel sources unchanged")
    return tab


def timed(fn, reps, sync=True):
    """Wall time per call of fn() over `reps` calls (after the caller's own warm-up), device-synchronised."""
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def timed_median(fn, reps):
    """Median wall time of `reps` individually synchronised calls (a call with its own host synchronisation inside, like the mean-shift
    driver: one slow call -- an allocator refill, a retried launch -- should not carry the figure)."""
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2]


def event_ms(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    for _ in range(reps):
        fn()
    e[1].record()
    e[1].synchronize()
    return e[0].elapsed_time(e[1]) / reps


def entry_graph_ms(step, names, reps=100):
    """One entry point of ops (or a list of them) on its own: its launches of one pass (their real arguments, recorded from `step()`),
    replayed back to back from a HIP graph between two HIP events on the current stream -- kernel time without the host's launch gaps
    and without the event records that sit between eager launches (what rocprofv3 reports per dispatch).
    -> (ms per replay of all recorded launches, number of launches)"""
    from unseenobjectswithmeanshift_amd import ops
    names = [names] if isinstance(names, str) else list(names)
    calls, origs = [], {n: getattr(ops, n) for n in names}

    def recorder(n):
        def rec(*a, **k):
            calls.append((n, a, k))
            return origs[n](*a, **k)
        return rec

    for n in names:
        setattr(ops, n, recorder(n))
    try:
        step()
    finally:
        for n in names:
            setattr(ops, n, origs[n])
    if not calls:
        return 0.0, 0
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        stream.synchronize()
        mg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(mg, stream=stream):
            for n, a, k in calls:
                origs[n](*a, **k)
        for _ in range(5):
            mg.replay()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            mg.replay()
        e1.record()
        e1.synchronize()
    torch.cuda.current_stream().wait_stream(stream)
    return e0.elapsed_time(e1) / reps, len(calls)


def mask_step_graph_ms(step, model, reps=100):
    """The full-resolution mask-step kernel on its own: the ten launches a pass makes when every prediction's mask step runs at
    120 x 160 (predictor.pooled_attention_masks = False for the recording).  -> (ms per launch, launches)"""
    pred = model.sem_seg_head.predictor
    keep = pred.pooled_attention_masks
    pred.pooled_attention_masks = False
    try:
        ms, n = entry_graph_ms(step, "mask_logits", reps)
    finally:
        pred.pooled_attention_masks = keep
    return ms / max(n, 1), n


def precision_leg(model, feats, dev, dist, args, precision, inflight, sparse_taps=False, pooled=True):
    """The per-GPU batch of 8 in another precision mode, timed on EVERY rank exactly like the headline region (barrier + sync on
    both sides, max over ranks): under --gpus 8 this is BASELINE configs[2] (batch 64 over 8 GPUs, bf16).  Returns this rank's
    (images, elapsed seconds, steps, one-batch-in-flight seconds per step)."""
    from unseenobjectswithmeanshift_amd.graphs import PipelinedInference
    model.set_precision(precision)
    model.sem_seg_head.predictor.sparse_taps = bool(sparse_taps)
    model.sem_seg_head.predictor.pooled_attention_masks = bool(pooled)
    roof = None
    if precision in ("bf16", "f16") and model.sem_seg_head.pixel_decoder._use_hm():
        # the two kernels that dominate the bf16 plan's step, each timed on its own (graph replays of the step's launches with
        # their real arguments, HIP events on the launch stream): the encoder-layer tail and the MSDeformAttn gather, with the
        # bytes the algorithm moves per launch (fp16 value / attention / sampling-projection tensors, fp32 residual stream)
        B = feats[next(iter(feats))].shape[0]
        tokens = B * ((H // 32) * (W // 32) + (H // 16) * (W // 16) + (H // 8) * (W // 8))
        step = lambda: model.inference(feats, (H, W))
        step()
        e_ms, e_n = entry_graph_ms(step, "encoder_block_hm")
        g_ms, g_n = entry_graph_ms(step, "ms_deform_attn_encoder_lp")
        # per token: fp16 attention in (128 B), fp32 residual in / out (512 B); all but the last layer: fp16 value (128 B) and the sampling
        # projection out (8 heads x 120 B: fp32 offsets + fp16 logits, round 5; 576 B before)
        e_bytes = tokens * (128 + 256 + 256) + tokens * (128 + 960) * (e_n - 1) / max(e_n, 1)
        e_flops = 2.0 * tokens * (64 * 64 + 2 * 64 * 1024) + 2.0 * tokens * (64 * 64 + 64 * 288) * (e_n - 1) / max(e_n, 1)
        # issued products: out_proj / value / sampling projection as three terms (w_lo x_hi + w_hi x_lo + w_hi x_hi), linear1 as two (x = h + l),
        # linear2 as one
        ffn_terms = 2 if precision == "f16" else 3              # f16: linear1 and linear2 one fp16 product each
        e_exec = 2.0 * tokens * (3 * 64 * 64 + ffn_terms * 64 * 1024) + 2.0 * tokens * 3 * (64 * 64 + 64 * 288) * (e_n - 1) / max(e_n, 1)
        g_bytes = tokens * (128 + 960 + 128)
        e_t, g_t = 1e-3 * e_ms / max(e_n, 1), 1e-3 * g_ms / max(g_n, 1)
        roof = {"bound": "hbm", "kernel": "enc_block_hm2_kernel (msm_encoder_block_hm_fwd): the 16-bit plans' encoder-layer tail",
                "achieved": round(e_bytes / e_t / 1e9, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s", "frac": round(e_bytes / e_t / 1e9 / PEAK_HBM_GBPS, 4),
                "traffic": None, "launches_per_step": e_n, "avg_launch_ms": round(1e3 * e_t, 4), "algorithmic_bytes_per_launch": e_bytes,
                "useful_flops_per_launch": e_flops, "useful_tflops": round(e_flops / e_t / 1e12, 1),
                "frac_of_bf16_mfma_peak": round(e_flops / e_t / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
                "issued_tflops": round(e_exec / e_t / 1e12, 1), "issued_frac_of_bf16_mfma_peak": round(e_exec / e_t / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
                "gather": {"kernel": "msda_enc_lp_kernel (msm_msdeform_attn_enc_lp_fwd)", "launches_per_step": g_n, "avg_launch_ms": round(1e3 * g_t, 4),
                           "algorithmic_bytes_per_launch": g_bytes, "achieved_gbps": round(g_bytes / g_t / 1e9, 1),
                           "frac_of_hbm_peak": round(g_bytes / g_t / 1e9 / PEAK_HBM_GBPS, 4)},
                "note": "bytes = fp16 attention in + fp32 residual in / out + fp16 value and the sampling projection (fp32 offsets, fp16 logits) out "
                        "(none for the last layer); useful FLOPs = the layer's GEMMs once (the kernel issues 1-3 products per operand pair)"}
        tnotes = []
        tr = load_traffic(f"step_traffic_{precision}.json", tnotes)      # PMC bytes of a committed rocprofv3 pass of THIS plan (stamped; stale -> null)
        if tr:
            roof["traffic"] = (tr.get("enc_block_hm_kernel") or {}).get("bytes_per_launch")
        roof["traffic_provenance"] = tnotes
    lone = PipelinedInference(model, depth=1)
    lone.submit(feats, (H, W))
    lone.drain()
    run_lone = lambda: lone.submit(None, (H, W), slot_inputs=True)
    for _ in range(3):
        run_lone()
    lone.drain()
    single = timed(run_lone, 100)
    del lone
    pipe = PipelinedInference(model, depth=inflight)
    for _ in range(inflight):
        pipe.submit(feats, (H, W))
    pipe.drain()
    run = lambda: pipe.submit(None, (H, W), slot_inputs=True)
    for _ in range(2 * inflight):
        run()
    pipe.drain()
    est = timed(run, 4 * inflight)
    steps = max(args.steps, int(math.ceil(args.min_seconds / max(est, 1e-6))))
    if dist is not None:
        t = torch.tensor([steps], device=dev if dist.get_backend() == "nccl" else "cpu", dtype=torch.int64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        steps = int(t.item())
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    del pipe
    model.set_precision("f32")
    model.sem_seg_head.predictor.sparse_taps = False
    return feats[next(iter(feats))].shape[0] * steps, elapsed, steps, single, roof


def mean_shift_unit(dev):
    """the classic UCN clustering timed as its own unit -- clustering_features (lib/fcn/test_dataset.py:44-59)
    on one 640x480 embedding map: n = 307 200 unit 64-vectors in 12 planted clusters, 100 seeds, 10 iterations, kappa 20."""
    from unseenobjectswithmeanshift_amd import mean_shift as ms
    from unseenobjectswithmeanshift_amd import ops
    from unseenobjectswithmeanshift_amd import synthetic as syn
    import numpy as np
    n, S, iters, kappa = H * W, 100, 10, 20.0
    X, _ = syn.synth_unit_embeddings(n, 64, clusters=12, sigma=0.15, seed=3)
    feats = X.t().reshape(1, 64, H, W).contiguous().to(dev)
    Xd = X.to(dev)
    t_seed = event_ms(lambda: ops.ms_select_seeds(Xd, S, 7), reps=10)
    seeds, _ = ops.ms_select_seeds(Xd, S, 7)
    t_hill = event_ms(lambda: ops.ms_hill_climb(Xd, seeds, kappa, iters), reps=10)
    Z = ops.ms_hill_climb(Xd, seeds, kappa, iters)
    lab = torch.zeros(S, dtype=torch.int64, device=dev)
    t_asg = event_ms(lambda: ops.ms_assign(Xd, Z, lab, 1), reps=10)
    np.random.seed(3)
    for _ in range(3):
        ms.clustering_features(feats, num_seeds=S)
    reps = 20
    # (median of individually synchronised calls, like configs[4]'s clustering: one call in twenty that finds the persistent seeding kernel's
    # workgroups not co-resident re-runs the seeding step by step -- 8 ms -- and would carry a mean)
    t_all = timed_median(lambda: ms.clustering_features(feats, num_seeds=S), reps)
    # the same unit with the hill climb in its f32_split form (fp32 results from six bf16 MFMAs per product; opt-in, not `value`)
    t_hill_sp = event_ms(lambda: ops.ms_hill_climb(Xd, seeds, kappa, iters, precision="f32_split"), reps=10)
    for _ in range(3):
        ms.clustering_features(feats, num_seeds=S, precision="f32_split")
    t_all_sp = timed_median(lambda: ms.clustering_features(feats, num_seeds=S, precision="f32_split"), reps)
    # the stress variant SURVEY 8d names: the same map with 2 % uniform background points -- the farthest-point seeds are then
    # background points that stay singletons: ~S clusters through the merge, the assignment and the relabel
    Xn, _ = syn.synth_unit_embeddings(n, 64, clusters=12, sigma=0.15, seed=3, background_frac=0.02)
    feats_n = Xn.t().reshape(1, 64, H, W).contiguous().to(dev)
    for _ in range(3):
        ms.clustering_features(feats_n, num_seeds=S)
    t_noisy = timed_median(lambda: ms.clustering_features(feats_n, num_seeds=S), reps)
    n_clusters_noisy = int(ms.clustering_features(feats_n, num_seeds=S)[0].unique().numel())
    ref_bytes = float(S) * n * 64 * 4                  # the reference re-reads X for every seed
    hill_flops = 4.0 * S * n * 64 * iters              # Z X^T and W X per iteration
    return {"workload": "clustering_features unit (lib/fcn/test_dataset.py:44-59): one 640x480 map, n=307200 unit 64-d embeddings in 12 "
                        "planted clusters, 100 seeds, 10 iterations, kappa 20; connected_components on the device, one host check per image",
            "value": round(1.0 / t_all, 2), "unit": "images/sec", "ms_per_image": round(1e3 * t_all, 3),
            "seeding": {"kernel": "ms_seed_persistent_kernel (one launch, map held in registers, data-tagged all-to-all exchange of the candidates per step)",
                        "ms": round(t_seed, 4), "bound": "hbm (reference form: S passes over X) -> exchange latency as executed",
                        "achieved": round(ref_bytes / (t_seed * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                        "frac": round(n * 256.0 / (t_seed * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
                        "executed_bytes": n * 256.0, "algorithmic_bytes": ref_bytes,
                        "note": "achieved = the reference algorithm's S*n*256 bytes over the time (effective); the kernel reads X "
                                "once (executed_bytes), frac is executed bytes / time / peak: the step is bound by S all-to-all exchanges"},
            "hill_climb": {"kernel": "ms_hill_kernel + ms_hill_finish_kernel", "ms": round(t_hill, 4), "bound": "mfma",
                           "achieved": round(hill_flops / (t_hill * 1e-3) / 1e12, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                           "frac": round(hill_flops / (t_hill * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4), "flops": hill_flops},
            "assign_ms": round(t_asg, 4),
            "background_2pct": {"value": round(1.0 / t_noisy, 2), "unit": "images/sec", "ms_per_image": round(1e3 * t_noisy, 3), "clusters": n_clusters_noisy,
                                "note": "same map with 2 % uniform background points (synth_unit_embeddings background_frac=0.02): nearly every seed a "
                                        "singleton cluster; parity: tests/test_gpu_modules.py::test_mean_shift_background_points_vs_oracle"},
            "f32_split": {"dtype": "f32 results, bf16x3 split products", "value": round(1.0 / t_all_sp, 2), "unit": "images/sec",
                          "ms_per_image": round(1e3 * t_all_sp, 3),
                          "hill_climb": {"kernel": "ms_split_planes_kernel (once) + ms_hill_planes_kernel + ms_hill_finish_kernel", "ms": round(t_hill_sp, 4),
                                         "useful_tflops": round(hill_flops / (t_hill_sp * 1e-3) / 1e12, 2),
                                         "vs_fp32_peak": round(hill_flops / (t_hill_sp * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                                         "executed_bf16_tflops": round(6.0 * hill_flops / (t_hill_sp * 1e-3) / 1e12, 2),
                                         "frac": round(6.0 * hill_flops / (t_hill_sp * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
                                         "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "bound": "vector issue (splitting) beside the bf16 MFMAs"},
                          "note": "labels identical to the fp32 path and the oracle on the test maps; not used for `value`"}}


def extra_configs(dev, args):
    """BASELINE configs[2] (per-GPU slice), configs[3] and configs[4], timed by this run (rank 0, N = 1)."""
    from unseenobjectswithmeanshift_amd import _lib
    from unseenobjectswithmeanshift_amd import mean_shift as ms
    from unseenobjectswithmeanshift_amd import ops
    from unseenobjectswithmeanshift_amd import synthetic as syn
    from unseenobjectswithmeanshift_amd import two_stage as ts
    from unseenobjectswithmeanshift_amd.meta_arch import Instances, MeanShiftMaskFormer, Network_RGBD
    out = {}
    model = build_model(dev)
    feats = {k: v.to(dev) for k, v in syn.synth_backbone_features(BATCH, H, W, seed=10).items()}
    # configs[1] again with fp32 GEMMs computed as exact three-term bf16 splits on the bf16 matrix pipe (six MFMAs per product:
    # fp32-accurate; csrc/enc_block_split.hip, kv_proj.hip, mask_logits.hip) -- NOT the headline: that keeps the fp32 MFMA everywhere
    class _A:
        steps, min_seconds = 50, 0.5
    imgs, el, st_, single, _ = precision_leg(model, feats, dev, None, _A, "f32_split", max(1, args.inflight))
    # the plan of rounds 1-3: every one of the ten mask steps at 120 x 160, the attention-mask taps pooled afterwards
    # (predictor.pooled_attention_masks = False) -- and the same with the nine intermediate steps restricted to the image rows their
    # attention masks sample (decoder.sparse_taps).  Reported next to the headline, which computes the intermediate attention masks at
    # key resolution (csrc/attn_mask.hip: interpolation and contraction commute; SURVEY 8d names the inference-only shortcut)
    fi, fel, fst, fsingle, _ = precision_leg(model, feats, dev, None, _A, "f32", max(1, args.inflight), pooled=False)
    si, sel, sst, ssingle, _ = precision_leg(model, feats, dev, None, _A, "f32", max(1, args.inflight), sparse_taps=True, pooled=False)
    model.sem_seg_head.predictor.pooled_attention_masks = True
    out["configs[1] full-resolution mask steps"] = {
        "workload": "batch 8, 640x480, fp32, as the headline except that all ten mask steps run at 120 x 160 (the attention-mask taps pooled "
                    f"from the full-resolution logits, as the reference orders it); {max(1, args.inflight)} batches of 8 in flight",
        "value": round(fi / fel, 1), "unit": "images/sec", "ms_per_step": round(1e3 * fel / fst, 4),
        "one_batch_in_flight": {"value": round(BATCH / fsingle, 1), "unit": "images/sec", "ms_per_step": round(1e3 * fsingle, 4)},
        "dtype": "f32",
        "sparse_taps": {"note": "the nine intermediate steps restricted to the row pairs their attention masks sample",
                        "value": round(si / sel, 1), "unit": "images/sec", "ms_per_step": round(1e3 * sel / sst, 4),
                        "one_batch_in_flight_ms": round(1e3 * ssingle, 4)}}
    model.set_precision("f32_split")
    ms_split, n_split = mask_step_graph_ms(lambda: model.inference(feats, (H, W)), model)
    model.set_precision("f32")
    fl_useful = 2.0 * Q * 64 * (H // 4) * (W // 4) * BATCH               # the folded contraction's FLOPs
    fl_bf16 = 6.0 * fl_useful                                            # six bf16 products per fp32 product
    out["configs[1] f32_split"] = {
        "workload": "batch 8, 640x480, fp32 results; the six encoder blocks, the batched K/V projection and the (folded) mask step multiply "
                    "exact three-term bf16 splits of their fp32 operands (6 bf16 MFMAs per product, fp32 accumulation); every other kernel "
                    f"as the headline; {max(1, args.inflight)} batches of 8 in flight",
        "value": round(imgs / el, 1), "unit": "images/sec", "ms_per_step": round(1e3 * el / st_, 4),
        "one_batch_in_flight": {"value": round(BATCH / single, 1), "unit": "images/sec", "ms_per_step": round(1e3 * single, 4)},
        "dtype": "f32 results, bf16x3 split products",
        "roofline": {"kernel": "mask_logits_split_kernel (msm_mask_logits_split_fwd)", "avg_launch_ms": round(ms_split, 4), "launches_per_step": n_split,
                     "vs_fp32_peak": {"achieved": round(fl_useful / (ms_split * 1e-3) / 1e12, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s (useful fp32 FLOPs)",
                                      "frac": round(fl_useful / (ms_split * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4)},
                     "bound": "mfma", "achieved": round(fl_bf16 / (ms_split * 1e-3) / 1e12, 2), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(fl_bf16 / (ms_split * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4), "traffic": None,
                     "note": "frac = executed bf16 MFMA FLOPs / time / 2516.6 (the step is then a stream over three bf16 copies of the activation, "
                             "59 MB per launch: HBM / L2 bound, not matrix bound)"}}
    del model
    # configs[1] end to end: the same batch of 8 frames with the ResNet-50 backbone (stock MIOpen convolutions, frozen BN
    # folded, channels_last) in front of the hot path -- reported separately, never mixed into the hot-path figure
    from unseenobjectswithmeanshift_amd.meta_arch import build_resnet50_model
    full = build_resnet50_model()
    full.sem_seg_head.pixel_decoder.load_state_dict(syn.synth_state_dict(syn.pixel_decoder_param_shapes()), strict=True)
    full.sem_seg_head.predictor.load_state_dict(syn.synth_state_dict(syn.decoder_param_shapes()), strict=True)
    full = full.to(dev).eval()
    images = torch.randn(BATCH, 3, H, W, device=dev)
    for _ in range(3):
        full([{"image": images}])
    t_bb = timed(lambda: full.backbone(images), 10)
    t_full = timed(lambda: full([{"image": images}]), 10)
    bbres = {"eager_fp32": {"value": round(BATCH / t_full, 1), "ms_per_step": round(1e3 * t_full, 3), "backbone_ms": round(1e3 * t_bb, 3)}}
    def two_in_flight(m, inputs, reps):
        """The whole model (backbone in every slot's graph) with two batches in flight, as the headline runs four of the head alone."""
        up = m.pipelined(depth=2, entry="inference_images")
        for _ in range(2):
            up.submit(inputs, (H, W))
        up.drain()
        run = lambda: up.submit(None, (H, W), slot_inputs=True)
        for _ in range(4):
            run()
        up.drain()
        t2 = timed(run, reps)
        up.drain()
        del up
        return t2

    for mode in ("f32", "bf16", "f16"):
        # the whole model -- backbone included -- replayed from ONE HIP graph; bf16: MIOpen bf16 convolutions (fp32 accumulation) +
        # the hot path's low-precision mode
        full.set_precision(mode)
        g = full.graphed(entry="inference_images")
        for _ in range(3):
            g({"image": images}, (H, W))
        t_g = timed(lambda: g({"image": images}, (H, W)), 20)
        t_2 = two_in_flight(full, {"image": images}, 20)
        for _ in range(2):
            full.backbone(images)
        t_b = timed(lambda: full.backbone(images), 10)
        bbres["hipgraph_" + mode] = {"value": round(BATCH / t_g, 1), "ms_per_step": round(1e3 * t_g, 3), "backbone_ms_eager": round(1e3 * t_b, 3),
                                     "two_batches_in_flight": {"value": round(BATCH / t_2, 1), "ms_per_step": round(1e3 * t_2, 3)}}
        del g
    full.set_precision("f32")
    out["configs[1] with backbone"] = {"workload": "batch 8, 640x480 RGB frames -> ResNet-50 (frozen BN folded, channels_last; 3x3 / 7x7 through MIOpen, 1x1 as hipBLASLt GEMMs, bias / ReLU / residual glue as one HIP launch each) -> hot "
                                                   "path -> instances; reported separately from the hot-path figure",
                                       "value": bbres["hipgraph_f32"]["value"], "unit": "images/sec", "ms_per_step": bbres["hipgraph_f32"]["ms_per_step"],
                                       "variants": bbres}
    del full
    # the literal 256-channel mask step (what a decoder handed a plain mask_features tensor runs; DEC:668 as written) with its
    # own roofline: executed FLOPs = the reference einsum's
    model = build_model(dev)
    model.sem_seg_head.predictor.folded_mask_features = False
    feats = {k: v.to(dev) for k, v in syn.synth_backbone_features(BATCH, H, W, seed=10).items()}
    g = model.graphed()
    for _ in range(3):
        g(feats, (H, W))
    t = timed(lambda: g(feats, (H, W)), 30)
    ms_lit, n_lit = mask_step_graph_ms(lambda: model.inference(feats, (H, W)), model)
    fl = 2.0 * Q * C_MASK * (H // 4) * (W // 4) * BATCH
    out["configs[1] literal mask step"] = {
        "workload": "batch 8, 640x480, fp32, the mask step contracting the 256-channel mask_features tensor as the reference writes it "
                    "(decoder.folded_mask_features = False); one HIP graph, one batch in flight, the graph copies its inputs",
        "value": round(BATCH / t, 1), "unit": "images/sec", "ms_per_step": round(1e3 * t, 3),
        "roofline": {"bound": "mfma", "kernel": "mask_logits_kernel, C = 256", "achieved": round(fl / (ms_lit * 1e-3) / 1e12, 2), "peak": PEAK_F32_MFMA_TFLOPS,
                     "unit": "TFLOP/s", "frac": round(fl / (ms_lit * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4), "flops_per_launch": fl,
                     "avg_launch_ms": round(ms_lit, 4), "launches_per_step": n_lit, "traffic": None}}
    del g, model
    # the UCN RGB-D path (configs/mixture_UCN.yaml): SimpleBasePixelDecoder + the single-level decoder whose keys
    # are every pixel of the 480x640 embedding (307 200 keys, 6 layers); backbone excluded like the headline
    from unseenobjectswithmeanshift_amd.meta_arch import PretrainedMeanShiftMaskFormer, build_ucn_head
    uh = build_ucn_head()
    uh.pixel_decoder.load_state_dict(syn.synth_state_dict({"mask_features.weight": (256, 64, 3, 3), "mask_features.bias": (256,)}, salt=3))
    uh.predictor.load_state_dict(syn.synth_state_dict(syn.decoder_param_shapes(dec_layers=6, num_feature_levels=1), salt=4))
    ucn = PretrainedMeanShiftMaskFormer(backbone=None, sem_seg_head=uh.to(dev).eval(), num_queries=Q)
    UB = 2
    X, _ = syn.synth_unit_embeddings(H * W, 64, clusters=12, sigma=0.3, seed=5)
    emb = X.view(1, H * W, 64).transpose(1, 2).reshape(1, 64, H, W).repeat(UB, 1, 1, 1).contiguous().to(dev)
    ufe = {"res5": emb}
    for _ in range(2):
        ucn.inference(ufe, (H, W))
    t_eager = timed(lambda: ucn.inference(ufe, (H, W)), 5)
    # the same pass replayed from a HIP graph, one and three batches in flight (graphs.PipelinedInference, as the headline)
    from unseenobjectswithmeanshift_amd.graphs import PipelinedInference
    t_pipe = {}
    for depth in (1, 3):
        up = PipelinedInference(ucn, depth=depth)
        for _ in range(depth):
            up.submit(ufe, (H, W))
        up.drain()
        urun = lambda: up.submit(None, (H, W), slot_inputs=True)
        for _ in range(2 * depth):
            urun()
        up.drain()
        t_pipe[depth] = timed(urun, 6 * depth)
        up.drain()
        del up
    t = min(t_pipe.values())
    with _lib.CallTimer() as ct:
        ucn.inference(ufe, (H, W))
        torch.cuda.synchronize()
    ud = ct.durations()
    # the same path in the 16-bit modes (bf16 K/V written by bf16 MFMAs, low-precision attention cores / tails / mask step; "f16": IEEE-half
    # operands where the range is bounded, fp16 keys): their own entries
    lp_modes = {}
    for mode in ("bf16", "f16"):
        ucn.set_precision(mode)
        for _ in range(2):
            ucn.inference(ufe, (H, W))
        t_lp = {}
        for depth in (1, 3):
            up = PipelinedInference(ucn, depth=depth)
            for _ in range(depth):
                up.submit(ufe, (H, W))
            up.drain()
            urun = lambda: up.submit(None, (H, W), slot_inputs=True)
            for _ in range(2 * depth):
                urun()
            up.drain()
            t_lp[depth] = timed(urun, 6 * depth)
            up.drain()
            del up
        with _lib.CallTimer() as ct:
            ucn.inference(ufe, (H, W))
            torch.cuda.synchronize()
        lp_modes[mode] = (t_lp, ct.durations())
    t_lp, ud_lp = lp_modes["bf16"]
    ucn.set_precision("f32")
    attn_ms = sum(ud.get("msm_hypersphere_attn_fwd", [0.0]))
    n_attn = len(ud.get("msm_hypersphere_attn_fwd", [])) or 1
    S_keys = H * W
    # cross-attention launches dominate (6 of the 12 attention launches carry 307 200 keys): FLOPs of Q^K^T and A V per launch
    attn_flops = 2.0 * 2.0 * Q * S_keys * 256 * UB
    cross = sorted(ud.get("msm_hypersphere_attn_fwd", [0.0]))[-6:]
    cross_ms = sum(cross) / max(1, len(cross))
    # bytes a cross-attention launch has to move: K and V (2 x S x 256 fp32) and the 1-byte mask (Q x S) per image
    attn_bytes = UB * (2.0 * S_keys * 256 * 4 + Q * S_keys)

    def fused_roofline(durs):
        """hs_attn_fkv_kernel (the 16-bit plans' cross attention at 307 200 keys: K/V projection inside the attention kernel).  Useful
        FLOPs per launch and image: the folded projection once per head (2 S 64 512), scores and P V on the Q real queries (2 x 2 Q S 256);
        bytes: the fp16 feature (128 B per key) + the bit-packed mask (16 B per key and 128-query chunk).  Its real limit is neither: the
        dependent chain projection -> norm -> 7 x (score -> exp -> P V) per 16-key block and Q S 8 exponentials on the vector pipe."""
        fk = durs.get("msm_hypersphere_attn_fused_kv_fwd", [])
        if not fk:
            return None
        ms = sum(fk) / len(fk)
        fl = UB * (2.0 * S_keys * 64 * 512 + 2.0 * 2.0 * Q * S_keys * 256)
        by = UB * (S_keys * 128.0 + S_keys * 16.0 * ((Q + 127) // 128))
        return {"bound": "mfma", "kernel": "hs_attn_fkv_kernel (msm_hypersphere_attn_fused_kv_fwd)", "achieved": round(fl / (ms * 1e-3) / 1e12, 1),
                "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(fl / (ms * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
                "flops_per_launch": fl, "bytes_per_launch": by, "hbm_frac": round(by / (ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
                "avg_launch_ms": round(ms, 4), "launches_per_step": len(fk), "share_of_kernel_time": round(sum(fk) / max(1e-9, sum(sum(v) for v in durs.values())), 3),
                "traffic": None,
                "note": "latency / vector-pipe bound: 2 Q S 8 exponentials with their mask and norm arithmetic are ~0.12 ms of VALU issue per launch; "
                        "the unfused pair (K/V written and read back) took 0.68 ms"}

    def mask_conv_entry(durs):
        """mask_conv_fold_kernel (16-bit plans): the mask step with the 3x3 mask_features convolution folded into per-query filters --
        executed FLOPs per launch 2 B Qpad 576 H W (K = 9 taps x 64 channels on fp16 MFMAs; the literal order executes 2 B Q 256 H W on a
        tensor this form never writes), bytes: the fp16 tokens once (128 B per key) + the bits written."""
        mc = durs.get("msm_mask_conv3x3_folded", [])
        if not mc:
            return None
        big = sorted(mc)[-max(1, len(mc) - 1):]                      # the Q = 100 launches (the last prediction runs on the K kept queries)
        ms = sum(big) / len(big)
        fl = 2.0 * UB * 112 * 576 * S_keys
        by = UB * (S_keys * 128.0 + S_keys * 16.0)
        return {"bound": "mfma", "kernel": "mask_conv_fold_kernel<0> (msm_mask_conv3x3_folded, Q = 100 -> attention-mask bits)",
                "achieved": round(fl / (ms * 1e-3) / 1e12, 1), "peak": PEAK_BF16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(fl / (ms * 1e-3) / 1e12 / PEAK_BF16_MFMA_TFLOPS, 4),
                "flops_per_launch": fl, "bytes_per_launch": by, "avg_launch_ms": round(ms, 4), "launches_per_step": len(mc),
                "all_launches_ms": round(sum(mc), 3), "traffic": None,
                "note": "replaces the 3x3 convolution to 256 channels (0.68 ms), its packed copy (0.18 ms), seven 0.13-ms mask steps over it and the "
                        "bit packing (6 x 0.016 ms) of the literal order: 1.9 -> 0.64 ms per pass; MFMA issue at the clock the part holds under this "
                        "load (~1.7 GHz) is 50 us of the 78 (tools/probes/mask_conv_parts.sh)"}
    out["ucn_path"] = {
        "workload": f"UCN RGB-D path: batch {UB} of 480x640 64-channel embeddings -> 3x3 mask_features convolution -> 6-layer hypersphere decoder "
                    "over 307 200 keys per image -> post-processing; HIP-graph replay, batches in flight as stated; backbone excluded",
        "value": round(UB / t, 1), "unit": "images/sec", "ms_per_step": round(1e3 * t, 3),
        "batches_in_flight": min(t_pipe, key=t_pipe.get),
        "one_batch_in_flight": {"value": round(UB / t_pipe[1], 1), "ms_per_step": round(1e3 * t_pipe[1], 3)},
        "three_batches_in_flight": {"value": round(UB / t_pipe[3], 1), "ms_per_step": round(1e3 * t_pipe[3], 3)},
        "eager": {"value": round(UB / t_eager, 1), "ms_per_step": round(1e3 * t_eager, 3)},
        "kernels_ms": {k: round(sum(v), 3) for k, v in sorted(ud.items(), key=lambda kv: -sum(kv[1]))[:6]},
        "bf16": {"dtype": "bf16 operands / fp32 accumulation; K/V projected inside the attention kernel, mask_features folded into the query embedding (never written)", "value": round(UB / min(t_lp.values()), 1), "unit": "images/sec",
                 "one_batch_in_flight": {"value": round(UB / t_lp[1], 1), "ms_per_step": round(1e3 * t_lp[1], 3)},
                 "three_batches_in_flight": {"value": round(UB / t_lp[3], 1), "ms_per_step": round(1e3 * t_lp[3], 3)},
                 "kernels_ms": {k: round(sum(v), 3) for k, v in sorted(ud_lp.items(), key=lambda kv: -sum(kv[1]))[:6]},
                 "roofline": fused_roofline(ud_lp), "mask_step": mask_conv_entry(ud_lp),
                 "parity": "tests/test_gpu_configs.py::test_ucn_path_480x640_bf16_vs_reference (final-mask mismatch 0.08 % (bf16) / 0.02 % (f16) against the fp32 reference golden)"},
        "f16": {"dtype": "fp16 / bf16 operands, fp32 accumulation; as the bf16 entry with fp16 score operands", "value": round(UB / min(lp_modes["f16"][0].values()), 1), "unit": "images/sec",
                "one_batch_in_flight": {"value": round(UB / lp_modes["f16"][0][1], 1), "ms_per_step": round(1e3 * lp_modes["f16"][0][1], 3)},
                "three_batches_in_flight": {"value": round(UB / lp_modes["f16"][0][3], 1), "ms_per_step": round(1e3 * lp_modes["f16"][0][3], 3)},
                "kernels_ms": {k: round(sum(v), 3) for k, v in sorted(lp_modes["f16"][1].items(), key=lambda kv: -sum(kv[1]))[:6]},
                "roofline": fused_roofline(lp_modes["f16"][1]), "mask_step": mask_conv_entry(lp_modes["f16"][1])},
        "roofline": {"bound": "hbm", "kernel": "hs_attn_kernel + combine at 307 200 keys (msm_hypersphere_attn_fwd)",
                     "achieved": round(attn_bytes / (cross_ms * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                     "frac": round(attn_bytes / (cross_ms * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4), "bytes_per_launch": attn_bytes,
                     "avg_launch_ms": round(cross_ms, 4), "launches_per_step": 6, "traffic": None,
                     "mfma_TFLOPs": round(attn_flops / (cross_ms * 1e-3) / 1e12, 2),
                     "mfma_frac": round(attn_flops / (cross_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                     "note": "AI = 4*Q*256 / (2*256*4 + Q) = 47.7 FLOP/B against an fp32 ridge of ~20: MFMA-bound in fp32 by the numbers; both fractions are given"}}
    del ucn, uh, emb
    # the TRUE RGB-D model end to end (lib/networks/SEG.py:26-126 -> pretrained_meanshiftformer_model.py:281-301): image +
    # xyz depth -> the two dilated ResNet34-8s towers (pinned to the reference by tests/golden/ucn_backbone.npz; stock MIOpen convolutions,
    # BatchNorm folded, channels_last) -> add fusion -> unit norm -> the UCN head above -> instances; one HIP graph per precision
    from unseenobjectswithmeanshift_amd.meta_arch import build_ucn_model
    um = build_ucn_model()
    um.backbone.load_state_dict(syn.ucn_backbone_state_dict(syn.ucn_backbone_param_shapes(), salt=6), strict=True)
    um.sem_seg_head.pixel_decoder.load_state_dict(syn.synth_state_dict({"mask_features.weight": (256, 64, 3, 3), "mask_features.bias": (256,)}, salt=3))
    um.sem_seg_head.predictor.load_state_dict(syn.synth_state_dict(syn.decoder_param_shapes(dec_layers=6, num_feature_levels=1), salt=4))
    um = um.to(dev).eval()
    gen = torch.Generator().manual_seed(5)
    uin = {"image": torch.randn(UB, 3, H, W, generator=gen).to(dev), "depth": torch.rand(UB, 3, H, W, generator=gen).to(dev)}
    e2e = {}
    for mode in ("f32", "bf16", "f16"):
        um.set_precision(mode)
        for _ in range(2):
            um.inference_images(uin, (H, W))
        t_bb = timed(lambda: um.backbone(uin["image"], None, uin["depth"]), 5)
        gph = um.graphed(entry="inference_images")
        for _ in range(3):
            gph(uin, (H, W))
        t_g = timed(lambda: gph(uin, (H, W)), 10)
        t_2 = two_in_flight(um, uin, 10)
        e2e[mode] = {"value": round(UB / t_g, 1), "unit": "images/sec", "ms_per_step": round(1e3 * t_g, 3), "backbone_ms_eager": round(1e3 * t_bb, 3),
                     "two_batches_in_flight": {"value": round(UB / t_2, 1), "ms_per_step": round(1e3 * t_2, 3)}}
        del gph
    um.set_precision("f32")
    out["ucn_rgbd_end_to_end"] = {
        "workload": f"the RGB-D model of mixture_UCN.yaml end to end: batch {UB} of 480x640 images + xyz depth maps -> two dilated ResNet34-8s towers "
                    "(MIOpen convolutions, BatchNorm folded, channels_last; bf16 plan: bf16 convolutions, f16 plan: IEEE-half convolutions) -> add fusion + unit norm -> "
                    "SimpleBasePixelDecoder + 6-layer hypersphere decoder over 307 200 keys -> instances; one HIP graph, one batch in flight",
        "value": e2e["f32"]["value"], "unit": "images/sec", "ms_per_step": e2e["f32"]["ms_per_step"], "variants": e2e}
    del um, uin
    # configs[3]: two-stage refinement over 16 frames
    model = build_model(dev)
    bb = syn.StandInBackbone().to(dev).eval()

    class RGBD(MeanShiftMaskFormer):
        def forward(self, batched_inputs):
            imgs = torch.stack([x["image"] for x in batched_inputs])
            deps = torch.stack([x["depth"] for x in batched_inputs])
            hh, ww = imgs.shape[-2:]
            scores, classes, masks, boxes, _ = self.inference(self.backbone(imgs, deps), (int(hh), int(ww)))
            return [{"instances": Instances((int(hh), int(ww)), pred_masks=masks[b], pred_boxes=boxes[b], scores=scores[b],
                                            pred_classes=classes[b])} for b in range(len(batched_inputs))]

    rgbd = RGBD(backbone=bb, sem_seg_head=model.sem_seg_head, num_queries=Q)
    crops = []

    class Pred(Network_RGBD):
        def batch_call(self, samples):
            crops.append(len(samples))
            with torch.no_grad():
                return self.model(samples)

        def batch_tensors(self, samples):              # the batched harness takes the model's batched tensors as they are
            crops.append(len(samples))
            imgs = torch.stack([x["image"] for x in samples])
            deps = torch.stack([x["depth"] for x in samples])
            with torch.no_grad():
                sc, cl, mk, _, _ = self.model.inference(self.model.backbone(imgs, deps), tuple(int(v) for v in imgs.shape[-2:]))
            return sc, cl, mk

    first, second = Network_RGBD(rgbd), Pred(rgbd)
    gen = torch.Generator().manual_seed(3)
    frames = [(torch.rand(3, H, W, generator=gen).to(dev), torch.rand(3, H, W, generator=gen).to(dev)) for _ in range(16)]
    samples = [{"image_color": im, "depth": dp} for im, dp in frames]

    def run_serial():                                   # the reference's loop structure: frame by frame (test_utils.py:375-406)
        for smp in samples:
            ts.test_sample_crop_nolabel(smp, first, second, confident_score=0.0, topk=False)

    def run_batch():                                    # configs[3]: the 16 frames as ONE batch
        return ts.test_batch_crop_nolabel(samples, second, second, confident_score=0.0, topk=False)

    run_serial()
    t_serial = timed(run_serial, 2)
    run_batch()
    crops.clear()
    t_eager32 = timed(run_batch, 5)
    n_crops = len(run_batch()[2])
    # the same batch under the 16-bit plans, eager and as the replayable pipeline (two_stage.BatchedTwoStage: both stages from HIP
    # graphs, the crop batch padded to a multiple of 16, two batches in flight so that the two device -> host transfers of a batch
    # overlap with the other batch's kernels)
    c3 = {}
    for mode in ("f32", "f16"):
        rgbd.set_precision(mode)
        run_batch()
        t_eager = timed(run_batch, 5)
        pipe2 = ts.BatchedTwoStage(rgbd, 16, (H, W), confident_score=0.0, topk=False)
        for _ in range(2):
            pipe2(samples)
        t_one = timed(lambda: pipe2(samples), 5)
        sink = lambda i, lab, ref, rows: None                      # (a consumer that leaves the slot's tensors where they are)
        pipe2.run([samples] * 4, consume=sink)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reps = 12
        pipe2.run([samples] * reps, consume=sink)
        torch.cuda.synchronize()
        t_two = (time.perf_counter() - t0) / reps
        c3[mode] = {"eager_ms_per_batch": round(1e3 * t_eager, 2), "graphs_one_batch_in_flight_ms": round(1e3 * t_one, 2),
                    "graphs_two_batches_in_flight_ms": round(1e3 * t_two, 2), "value": round(16 / t_two, 1), "unit": "frames/sec"}
        del pipe2
    rgbd.set_precision("f32")
    best = c3["f16"]
    out["configs[3]"] = {"workload": "two-stage RGB + depth-crop refinement, batch of 16 frames of 640x480 under set_precision('f16'): first stage on all 16 "
                                     "frames (one HIP graph: stand-in backbone, head, label images, depth filter, label statistics), ROI table on the "
                                     "host, every ROI of every frame cut and resized to 224x224 and all crops through the second stage (one HIP graph "
                                     "per crop-count bucket of 16), paste order on the host, one paste-back launch; two batches in flight: the two "
                                     "device->host transfers of a batch overlap with the other batch's kernels",
                         "value": best["value"], "unit": "frames/sec", "ms_per_frame": round(best["graphs_two_batches_in_flight_ms"] / 16, 3),
                         "ms_per_batch": best["graphs_two_batches_in_flight_ms"], "dtype": "f16 plan (IEEE-half operands, fp32 accumulation)",
                         "crops_per_frame": round(n_crops / 16, 1), "plans": c3,
                         "parity": "tests/test_gpu_configs.py::test_config3_two_stage_640x480_vs_oracle[f32 | f32_split | f16]",
                         "eager_f32": {"value": round(16 / t_eager32, 1), "unit": "frames/sec", "ms_per_batch": round(1e3 * t_eager32, 2),
                                       "note": "rounds 3-5's figure: eager launches, fp32 plan, one batch at a time"},
                         "frame_by_frame": {"value": round(16 / t_serial, 1), "unit": "frames/sec", "ms_per_frame": round(1e3 * t_serial / 16, 3),
                                            "note": "the reference's loop structure (one frame at a time, one batched second-stage call per frame), fp32"}}
    del rgbd, model
    # configs[4]: 1280x960, 300 queries; SURVEY 8d says "20 layers" -- timed with 20 decoder layers (21 predictions), and with the 19
    # layers the parity fixture head_cfg5_960x1280 holds (the reference builds DEC_LAYERS - 1 layers, DEC:529: DEC_LAYERS = 20 -> 19)
    res = {}
    for layers, batches in ((20, (1, 4)), (19, (1,))):
        model = build_model(dev, num_queries=300, dec_layers=layers)
        for B_ in batches:
            feats = {k: v.to(dev) for k, v in syn.synth_backbone_features(B_, 960, 1280, seed=9).items()}
            for mode in (("f32", "bf16", "f16") if layers == 20 else ("f32", "bf16")):
                model.set_precision(mode)
                g = model.graphed()
                for _ in range(2):
                    g(feats, (960, 1280))
                t = timed(lambda: g(feats, (960, 1280)), 10)
                res[f"{layers} layers, batch {B_}, {mode}"] = {"value": round(B_ / t, 1), "unit": "images/sec", "ms_per_batch": round(1e3 * t, 3)}
                del g
            del feats
        del model
    n, S, iters = 960 * 1280, 300, 20
    X, _ = syn.synth_unit_embeddings(n, 64, clusters=24, sigma=0.15, seed=3)
    Xd = X.to(dev)
    xb = ops.ms_pack_bf16(Xd)
    seeds, _ = ops.ms_select_seeds(Xd, S, 7)
    on_chip = 917504                          # rows the persistent bf16 seeding kernel holds in VGPRs + LDS (256 CUs x 32 groups x 7 tiles x 16)
    # f32: S - 1 passes over X; bf16: the copy once, then per step only the rows that are not on chip
    seed_bytes = {"f32": float(S) * n * 256, "f32_split": float(S) * n * 256, "bf16": n * 128.0 + (S - 1.0) * max(0, n - on_chip) * 128}
    hill_flops = 4.0 * S * n * 64 * iters
    msr = {}
    for mode in ("bf16", "f32_split", "f32"):
        for _ in range(2):
            ms.mean_shift_smart_init(Xd, 20.0, S, iters, first_index=7, precision=mode)
        t_ms = timed_median(lambda: ms.mean_shift_smart_init(Xd, 20.0, S, iters, first_index=7, precision=mode), 5)
        t_seed = event_ms(lambda: ops.ms_select_seeds(Xd, S, 7, xb=xb if mode == "bf16" else None), reps=3, warm=1)
        t_seed_stepwise = event_ms(lambda: ops.ms_select_seeds(Xd, S, 7, xb=xb, stepwise=True), reps=3, warm=1) if mode == "bf16" else None
        t_hill = event_ms(lambda: ops.ms_hill_climb(Xd, seeds, 20.0, iters, precision=mode, xb=xb if mode == "bf16" else None), reps=3, warm=1)
        mult, peak = {"f32": (1.0, PEAK_F32_MFMA_TFLOPS), "f32_split": (6.0, PEAK_BF16_MFMA_TFLOPS), "bf16": (1.5, PEAK_BF16_MFMA_TFLOPS)}[mode]
        msr[mode] = {"ms": round(1e3 * t_ms, 2),
                     "seeding": {"ms": round(t_seed, 3), "bound": "hbm", "algorithmic_bytes": seed_bytes[mode],
                                 "achieved": round(seed_bytes[mode] / (t_seed * 1e-3) / 1e9, 1), "peak": PEAK_HBM_GBPS, "unit": "GB/s",
                                 "frac": round(seed_bytes[mode] / (t_seed * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
                                 "kernel": ("ms_seed_persistent_bf16_kernel: one launch, 917 504 rows of the bf16 copy in VGPRs + LDS, the other 311 296 "
                                            "(40 MB) streamed per step; a step = that stream + the 5.6 us candidate exchange, so the HBM fraction is "
                                            "not the limit here") if mode == "bf16" else "ms_seed_step_kernel x (S - 1), 314 MB per pass"},
                     **({"seeding_one_launch_per_step": {"ms": round(t_seed_stepwise, 3), "algorithmic_bytes": float(S) * n * 128,
                                                         "frac_of_hbm_peak": round(float(S) * n * 128 / (t_seed_stepwise * 1e-3) / 1e9 / PEAK_HBM_GBPS, 4),
                                                         "kernel": "ms_seed_step_bf16_kernel x (S - 1), 157 MB per pass (the give-up fallback)"}}
                        if t_seed_stepwise is not None else {}),
                     "hill_climb": {"ms": round(t_hill, 3), "bound": "mfma", "useful_flops": hill_flops,
                                    "useful_tflops": round(hill_flops / (t_hill * 1e-3) / 1e12, 1),
                                    "executed_tflops": round(mult * hill_flops / (t_hill * 1e-3) / 1e12, 1), "peak": peak, "unit": "TFLOP/s",
                                    "frac": round(mult * hill_flops / (t_hill * 1e-3) / 1e12 / peak, 4),
                                    "products_per_useful_product": mult,
                                    "kernel": {"f32": "ms_hill_kernel (fp32 MFMA), 3 launches per iteration", "f32_split": "ms_hill_planes_kernel (six bf16 MFMAs per product), "
                                               "3 launches per iteration", "bf16": "ms_hill_bf16_kernel (Z as h + l: 2 score MFMAs + 1 W X MFMA per pair), 1 launch per iteration"}[mode]}}
    Xn, _ = syn.synth_unit_embeddings(n, 64, clusters=24, sigma=0.15, seed=3, background_frac=0.02)
    Xnd = Xn.to(dev)
    noisy = {}
    for mode in ("bf16", "f32"):
        for _ in range(2):
            ms.mean_shift_smart_init(Xnd, 20.0, S, iters, first_index=7, precision=mode)
        noisy[mode] = round(1e3 * timed_median(lambda: ms.mean_shift_smart_init(Xnd, 20.0, S, iters, first_index=7, precision=mode), 5), 2)
    msr["bf16"]["background_2pct"] = {"ms": noisy["bf16"], "ms_f32": noisy["f32"],
                                      "note": "the same clustering on a map with 2 % uniform background points (~S singleton clusters)"}
    del Xnd
    out["configs[4]"] = {"workload": "1280x960, 300 queries, batch 1 and 4 (pixel decoder + decoder + post-processing; 20 decoder layers as SURVEY 8d "
                                     "states the config, and the 19 of the parity fixture); classic mean shift on n=1228800 embeddings, 300 seeds, "
                                     "20 iterations (bf16 = the config's dtype: one bf16 copy of X shared by seeding and hill climb; f32 / f32_split exact)",
                         "hot_path": res,
                         "mean_shift": dict(msr["bf16"], dtype="bf16 copy of X, fp32 accumulation / distances / seeds", other_precisions={k: msr[k] for k in ("f32_split", "f32")})}
    return out


def build_summary(result):
    """<= 2 KB digest of the line, emitted as its LAST key (the driver keeps a fixed key set + the tail of stdout; the full line is
    ~20 KB): per config the throughput `v` (images/s unless noted), the one-batch-in-flight step `ms1`, the dtype `dt` and the
    roofline fraction `rf` of that config's dominant kernel.  Every number README / DESIGN quote is here or in `roofline`."""
    cfg = result.get("configs") or {}
    r = result.get("roofline") or {}                  # (empty in a plain run: the roofline legs are --full's)

    def pick(d, *path, nd=1):
        for k in path:
            if not isinstance(d, dict) or k not in d:
                return None
            d = d[k]
        return round(d, nd) if isinstance(d, float) else d

    s = {"c1": {"v": result["value"], "ms1": r.get("one_batch_in_flight_ms"), "v1": r.get("one_batch_in_flight_images_per_sec"), "dt": "f32",
                "rf": r.get("frac"), "mask_rf": r.get("mask_step_frac"), "mask_lit_rf": r.get("mask_step_literal_frac")}}
    c = cfg.get("configs[1] f32_split")
    if c:
        s["c1_split"] = {"v": c["value"], "ms1": pick(c, "one_batch_in_flight", "ms_per_step", nd=3), "dt": "f32 via bf16x3", "rf": pick(c, "roofline", "frac", nd=3)}
    c = cfg.get("configs[1] full-resolution mask steps")
    if c:
        s["c1_fullres"] = {"v": c["value"], "ms1": pick(c, "one_batch_in_flight", "ms_per_step", nd=3)}
    c = cfg.get("configs[1] literal mask step")
    if c:
        s["c1_literal"] = {"v": c["value"], "ms1": c["ms_per_step"], "rf": pick(c, "roofline", "frac", nd=3)}
    c = cfg.get("configs[1] with backbone")
    if c:
        s["c1_backbone"] = {k.replace("hipgraph_", ""): {"v": v["value"], "ms": v["ms_per_step"], "v2": pick(v, "two_batches_in_flight", "value")} for k, v in c["variants"].items() if k.startswith("hipgraph_")}
    # configs[2]'s headline entry is the f16 plan (the 16-bit plan that holds SURVEY 8c's bars with margin); the bf16 plan beside it
    for key, tag in (("configs[2]", "c2"), ("configs[2] bf16", "c2_bf16")):
        c = cfg.get(key)
        if c:
            s[tag] = {"v": c["value"], "ms1": pick(c, "one_batch_in_flight", "ms_per_step", nd=3), "dt": "f16" if tag == "c2" else "bf16",
                      "rf_hbm": pick(c, "roofline", "frac", nd=3), "rf_mfma": pick(c, "roofline", "frac_of_bf16_mfma_peak", nd=3),
                      "traffic": pick(c, "roofline", "traffic")}
    c = cfg.get("configs[3]")
    if c:
        s["c3"] = {"v": c["value"], "unit": "frames/s", "ms_batch16": c["ms_per_batch"], "dt": "f16", "ms1": pick(c, "plans", "f16", "graphs_one_batch_in_flight_ms"),
                   "f32_ms": pick(c, "plans", "f32", "graphs_two_batches_in_flight_ms"), "eager_f32_ms": pick(c, "eager_f32", "ms_per_batch")}
    c = cfg.get("configs[4]")
    if c:
        s["c4"] = {"hot": {k.replace(" layers, batch ", "L_b").replace(", ", "_"): v["value"] for k, v in c["hot_path"].items()},
                   "ms": {"bf16": pick(c, "mean_shift", "ms"), "f32_split": pick(c, "mean_shift", "other_precisions", "f32_split", "ms"),
                          "f32": pick(c, "mean_shift", "other_precisions", "f32", "ms"), "unit": "ms per clustering",
                          "seed_rf_hbm": pick(c, "mean_shift", "seeding", "frac", nd=3), "hill_rf_mfma": pick(c, "mean_shift", "hill_climb", "frac", nd=3),
                          "noisy_bf16": pick(c, "mean_shift", "background_2pct", "ms")}}
    c = cfg.get("ucn_path")
    if c:
        s["ucn"] = {"f32": {"v": c["value"], "ms1": pick(c, "one_batch_in_flight", "ms_per_step", nd=3)},
                    "bf16": {"v": pick(c, "bf16", "value"), "ms1": pick(c, "bf16", "one_batch_in_flight", "ms_per_step", nd=3)},
                    "f16": {"v": pick(c, "f16", "value"), "ms1": pick(c, "f16", "one_batch_in_flight", "ms_per_step", nd=3)},
                    "rf_hbm": pick(c, "roofline", "frac", nd=3), "fkv_rf_mfma": pick(c, "bf16", "roofline", "frac", nd=3),
                    "fkv_ms": pick(c, "bf16", "roofline", "avg_launch_ms", nd=4)}
    c = cfg.get("ucn_rgbd_end_to_end")
    if c:
        s["ucn_e2e"] = {k: {"v": v["value"], "ms": v["ms_per_step"], "v2": pick(v, "two_batches_in_flight", "value")} for k, v in c["variants"].items()}
    m = result.get("mean_shift")
    if m:
        s["ms640"] = {"v": m["value"], "split": pick(m, "f32_split", "value"), "noisy": pick(m, "background_2pct", "value"),
                      "hill_rf": pick(m, "hill_climb", "frac", nd=3)}
    c = result.get("cpu_baseline")
    if c:
        s["cpu"] = {"v": c["value"], "cores": c["cores"], "ms640": pick(c, "mean_shift", "value", nd=3)}
    while len(json.dumps(s)) > 2048 and len(s) > 1:          # never outgrow the budget: drop from the end
        s.popitem()
    return s


LINE_BUDGET = 8000          # bytes: the driver keeps the last 8 KB of stdout; a longer line is not parsed (round 5: 27 KB -> parsed: null)


def _short(s, n=118):
    """The driver's parser truncates strings at 120 characters: keep every string of the line below that."""
    return s if not isinstance(s, str) or len(s) <= n else s[:n - 1] + "~"


def compact_line(result, detail_path=None):
    """The ONE stdout line: the contract's scalar keys, `config`, a flat `roofline` (dominant kernel + the mask step's scalars), a flat
    `cpu_baseline`, a short `collective`, the <= 2 KB `summary` and the path of the file that holds everything else (`kernels`, `configs`,
    `mean_shift`, per-rank detail: written by main() to `detail_path`).  At most LINE_BUDGET bytes: tests/test_host_cpu.py builds it from a
    full result with every optional entry present and checks the size and the JSON round trip."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "steps_requested", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data")
    line = {k: result.get(k) for k in keep}
    cfg = result.get("config") or {}
    line["config"] = {k: _short(cfg[k]) for k in ("workload", "global_batch", "per_gpu_batch", "launch", "batches_in_flight", "parallelism",
                                                  "configs2_plan", "GPU_MAX_HW_QUEUES", "visible_gpus") if k in cfg}
    aff = cfg.get("rank0_cpu_affinity")
    if isinstance(aff, dict):
        line["config"]["rank0_numa"] = _short(str(aff.get("status")), 60)
    r = result.get("roofline") or {}
    flat = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_ms", "launches_per_step",
            "flops_per_launch", "share_of_step", "matrix_pipe", "one_batch_in_flight_ms", "one_batch_in_flight_images_per_sec", "mask_step_frac",
            "mask_step_avg_launch_ms", "mask_step_literal_frac", "traffic_source")
    line["roofline"] = {k: _short(r[k]) for k in flat if k in r}
    m = r.get("mask_step") or {}
    for src, dst in (("kernel_achieved_tflops", "mask_step_tflops"), ("plan_ms_per_step", "mask_plan_ms_per_step"),
                     ("plan_launches_per_step", "mask_plan_launches"), ("traffic_final_launch", "mask_step_traffic")):
        if src in m:
            line["roofline"][dst] = m[src]
    c = result.get("cpu_baseline")
    if c:
        flatc = {k: _short(c[k]) for k in ("value", "unit", "cores", "host_cpus", "kind", "statistic", "iterations") if k in c}
        for k, v in (c.get("pieces") or {}).items():
            flatc[k] = v
        ms = c.get("mean_shift") or {}
        if ms:
            flatc["mean_shift_images_per_sec"] = ms.get("value")
            flatc["mean_shift_ms_per_image"] = ms.get("ms_per_image")
        flatc["sample"] = _short(c.get("sample_short") or c.get("sample"))
        line["cpu_baseline"] = flatc
    if "per_rank" in result:
        pr = result["per_rank"]
        line["per_rank"] = {"images_per_sec": [p.get("images_per_sec") for p in pr], "checksum": [round(p.get("checksum", 0.0), 4) for p in pr],
                            "numa_pinned": sum(bool(p.get("numa_pinned")) for p in pr)}
    col = result.get("collective") or {}
    line["collective"] = {k: _short(col[k], 100) for k in ("backend", "world_size", "rccl_version", "transport", "all_gather_us", "note") if k in col}
    if "per_rank_elapsed_s" in col:
        line["collective"]["spread_pct"] = col["per_rank_elapsed_s"].get("spread_pct")
        line["collective"]["slowest_rank"] = col["per_rank_elapsed_s"].get("slowest_rank")
    line["detail"] = detail_path
    line["summary"] = result["summary"] if "summary" in result else build_summary(result)
    # never outgrow the driver's record: shed the optional members, largest first, until the line fits
    for victim in ("per_rank", "collective", "detail"):
        if len(json.dumps(line).encode()) <= LINE_BUDGET:
            break
        line.pop(victim, None)
    while len(json.dumps(line).encode()) > LINE_BUDGET and len(line["summary"]) > 1:
        line["summary"].popitem()
    assert len(json.dumps(line).encode()) <= LINE_BUDGET, "bench line over the driver's budget"
    return line


def write_detail(result, path):
    """Everything the compact line leaves out, as one JSON document (copied into profiles/ from the builder's own runs)."""
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(result, f)
        return path
    except OSError as e:
        print(f"bench.py: could not write {path}: {e}", file=sys.stderr, flush=True)
        return None


MASK_SAMPLE = 1 << 22          # mask values kept by --dump-outputs (16 MB as float32; the full masks are 8 x 20 x 480 x 640 = 197 MB)
MASK_SAMPLE_SEED = 20261016


def dump_outputs(outputs, path):
    """--dump-outputs: the arrays a caller of the timed path receives for one batch -- (scores, classes, masks, boxes, query_index)
    of model.inference -- as <path>/<name>.npy, float32 where the tensor is float32, float64 for the integer ones (exact).  The masks
    go in as a fixed sample (MASK_SAMPLE flat positions drawn with MASK_SAMPLE_SEED, in increasing order) and as every mask's area
    (float64), about 16 MB in all.  -> the names written."""
    import numpy as np
    scores, classes, masks, boxes, qidx = outputs
    arrays = {"scores": scores.float(), "classes": classes.double(), "boxes": boxes.float(), "query_index": qidx.double(),
              "masks_area": masks.sum(dim=(2, 3), dtype=torch.float64)}
    flat = masks.reshape(-1)
    idx = np.random.default_rng(MASK_SAMPLE_SEED).choice(flat.numel(), size=min(MASK_SAMPLE, flat.numel()), replace=False)
    idx.sort()
    arrays["masks_sample"] = flat[torch.from_numpy(idx).to(flat.device)].float()
    os.makedirs(path, exist_ok=True)
    for name, t in arrays.items():
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())
    return sorted(arrays)


# ----------------------------------------------------------------------------------------------------------------------
def collective_entry(dist, rec, all_gather_s, rccl_log=None):
    """What an N > 1 line says about its only collective: library version, the transport RCCL chose (rank 0's NCCL_DEBUG=INFO
    log, summarised), the all_gather's own wall time, and the spread of the ranks' timed regions -- so a SCALE record either
    shows ">= 6x at 8 GPUs over xGMI" or explains why not (a slow rank, a PCIe / SHM transport, an unpinned host thread)."""
    from unseenobjectswithmeanshift_amd.distributed import communicator_report
    el = [r["elapsed_s"] for r in rec]
    out = communicator_report(dist, rccl_log)
    out.update({"collective": "one all_gather of a per-rank metrics record (4-5 float64) after the timed region; none on the data path",
                "per_rank_elapsed_s": {"min": round(min(el), 6), "max": round(max(el), 6), "spread_pct": round(100.0 * (max(el) - min(el)) / max(el), 2),
                                       "slowest_rank": int(max(range(len(el)), key=el.__getitem__))}})
    if all_gather_s is not None:                    # (timed under --full only)
        out["all_gather_us"] = round(1e6 * all_gather_s, 1)
    return out


# ----------------------------------------------------------------------------------------------------------------------
def stub_main(args, world, rank):
    """Test hook (tests/test_distributed_cpu.py): the launcher, the process group (gloo), the barrier / max-over-ranks timing
    and the metrics all_gather with a trivial CPU step -- no GPU, no kernels, `data` says "stub"."""
    import torch.distributed as dist
    from unseenobjectswithmeanshift_amd.distributed import gather_metrics, shard_range
    if world > 1:
        dist.init_process_group("gloo")
    lo, hi = shard_range(world * BATCH, world, rank)
    x = torch.full((64, 64), float(rank + 1))
    acc = 0.0
    for _ in range(args.warmup):
        acc += float((x @ x).sum())
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        acc = float((x @ x).sum())
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    rec = gather_metrics({"images": (hi - lo) * args.steps, "elapsed_s": elapsed, "checksum": acc}, dist if world > 1 else None)
    from unseenobjectswithmeanshift_amd.distributed import timed_all_gather
    ag_s = timed_all_gather(dist if world > 1 else None, reps=5)
    if rank == 0:
        t_max = max(r["elapsed_s"] for r in rec)
        result = {"metric": METRIC, "value": round(sum(r["images"] for r in rec) / t_max, 2), "unit": "images/sec",
                  "n_gpus": world, "steps": args.steps, "steps_requested": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * t_max / args.steps, 4),
                  "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "stub",
                  "config": {"workload": "launcher self-test", "global_batch": world * BATCH, "per_gpu_batch": BATCH, "parallelism": f"dp{world}"},
                  "per_rank": [{"rank": i, "images": r["images"], "images_per_sec": round(r["images"] / r["elapsed_s"], 2), "checksum": r["checksum"]}
                               for i, r in enumerate(rec)],
                  "roofline": {}, "summary": {},
                  "collective": collective_entry(dist if world > 1 else None, rec, ag_s)}
        line = compact_line(result)
        line["per_rank"]["images"] = [p["images"] for p in result["per_rank"]]
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=120, help="timed steps (exactly this many)")
    ap.add_argument("--warmup", type=int, default=10, help="untimed steps before the timed ones")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed path computed in its last step to DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline figure does not need: one batch in flight, per-kernel timings and rooflines, "
                         "the 16-bit plans (configs[2]), the mean-shift unit, configs[1..4] sub-results, the CPU baseline")
    ap.add_argument("--min-seconds", type=float, default=1.0, help="--full: lower bound of the one-batch timing and of each precision leg")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a HIP graph")
    ap.add_argument("--inflight", type=int, default=4,
                    help="batches in flight, one HIP graph + stream each (graphs.PipelinedInference); 1 = one graph on one stream")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the mean-shift unit and the configs[2..4] sub-results")
    ap.add_argument("--no-bf16-leg", action="store_true", help="--full: skip the bf16 timing of the per-GPU batch (BASELINE configs[2]) that follows the fp32 region")
    ap.add_argument("--folded-mask", type=int, default=-1, help="1/0: contract the mask features in factored form (64-channel activation; "
                    "default: the decoder's own default, on) or literally (256-channel mask_features tensor)")
    ap.add_argument("--sparse-taps", action="store_true", help="skip mask rows that feed no attention-mask tap")
    ap.add_argument("--precision", choices=("f32", "f32_split", "bf16", "f16"), default="f32",
                    help="bf16 (configs 3/5) is NOT the headline configuration: the JSON line then says so in dtype")
    ap.add_argument("--batched-kv", type=int, default=-1, help="1/0: all K/V projections of the decoder in one launch (default: the decoder's own default)")
    ap.add_argument("--no-rccl-report", action="store_true", help="N > 1: do not record rank 0's NCCL_DEBUG=INFO log for the `collective` entry")
    ap.add_argument("--detail", default=None, help="--full: file that receives the full result document (default bench_out/bench_full.json)")
    ap.add_argument("--stub", action="store_true", help=argparse.SUPPRESS)
    # test hooks for the N > 1 code path on a ONE-GPU box (tests/test_gpu_configs.py): every rank on cuda:0, collectives over gloo
    ap.add_argument("--backend", choices=("nccl", "gloo"), default="nccl", help=argparse.SUPPRESS)
    ap.add_argument("--share-gpu", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        if not args.stub:
            have = torch.cuda.device_count()
            if have < args.gpus and not args.share_gpu:
                raise SystemExit(f"bench.py --gpus {args.gpus}: only {have} GPU(s) visible")
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(1, args.gpus):
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if args.stub:
        return stub_main(args, world, rank)
    dist = None
    if not torch.cuda.is_available():
        raise RuntimeError("bench.py needs an MI355X: the hot path has no CPU implementation (oracle/ is test-only)")
    if args.share_gpu:
        local_rank = 0
    # one process per GPU: a rank that cannot see the device it was told to use, or that would share it with another rank, is a
    # launch error -- say so instead of timing something else (the first real 8-GPU run either scales or says why)
    have = torch.cuda.device_count()
    if local_rank >= have:
        raise SystemExit(f"bench.py rank {rank}: LOCAL_RANK={local_rank} but this process sees {have} GPU(s) "
                         f"(HIP_VISIBLE_DEVICES={os.environ.get('HIP_VISIBLE_DEVICES')!r}, ROCR_VISIBLE_DEVICES={os.environ.get('ROCR_VISIBLE_DEVICES')!r})")
    if world > 1 and not args.share_gpu and have < int(os.environ.get("LOCAL_WORLD_SIZE", world)):
        raise SystemExit(f"bench.py rank {rank}: {os.environ.get('LOCAL_WORLD_SIZE', world)} local ranks but only {have} GPU(s) visible: ranks would share a device")
    torch.cuda.set_device(local_rank)           # before the process group: RCCL binds its communicator to the current device
    dev = torch.device("cuda", local_rank)
    affinity = pin_to_gpu_numa_node(local_rank)
    if world > 1 and affinity["status"].startswith("failed"):
        # a speed matter, not a correctness one: the run goes on, the line says how many ranks are pinned, stderr says why not
        print(f"bench.py rank {rank}: NOT pinned to the NUMA node of GPU {local_rank}: {affinity}", file=sys.stderr, flush=True)
    rccl_log = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.full and args.backend == "nccl" and rank == 0 and not args.no_rccl_report and "NCCL_DEBUG" not in os.environ:
            # rank 0 records what its communicator runs over (transport per channel, detected topology) into a file of its own --
            # stdout keeps the one JSON line -- and summarises it under `collective` (distributed.parse_rccl_debug)
            rccl_log = f"/tmp/msm_rccl_rank0_{os.getpid()}.log"
            os.environ.update(NCCL_DEBUG="INFO", NCCL_DEBUG_SUBSYS="INIT,GRAPH,P2P", NCCL_DEBUG_FILE=rccl_log)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")

    from unseenobjectswithmeanshift_amd import _lib, ops
    from unseenobjectswithmeanshift_amd import synthetic as syn
    from unseenobjectswithmeanshift_amd.distributed import communicator_report, gather_metrics, shard_range, timed_all_gather

    model = build_model(dev)
    pred = model.sem_seg_head.predictor
    pred.sparse_taps = args.sparse_taps
    if args.precision != "f32":
        if hasattr(model, "set_precision"):
            model.set_precision(args.precision)
        else:
            pred.mask_step_dtype = "bf16"
    if args.folded_mask >= 0:
        pred.folded_mask_features = bool(args.folded_mask)
    if args.batched_kv >= 0:
        pred.batched_kv = bool(args.batched_kv)
    # weak scaling: the global batch is world*8 images, rank r owns images [r*8, (r+1)*8)
    lo, hi = shard_range(world * BATCH, world, rank)
    feats = {k: v.to(dev) for k, v in syn.synth_backbone_features(hi - lo, H, W, seed=10 + rank).items()}

    def step():
        return model.inference(feats, (H, W))

    full = args.full
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        # throughput mode: `inflight` batches in flight, each a HIP graph on its own stream (graphs.PipelinedInference);
        # every slot keeps its own copy of the inputs resident in HBM, a step = one replay of one slot's graph
        inflight = 1 if args.no_graph else max(1, args.inflight)
        out = graph = pipe = None
        if inflight == 1 or full:
            # the single-stream form: the timed step itself (inflight 1), or under --full the one-batch figure beside the headline
            for _ in range(max(1, args.warmup) if args.no_graph else 2):
                out = step()
            stream.synchronize()
            if not args.no_graph:
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=stream):
                    out = step()
            one = graph.replay if graph is not None else step
            for _ in range(args.warmup):
                one()
            stream.synchronize()
        if inflight > 1:
            from unseenobjectswithmeanshift_amd.graphs import PipelinedInference
            pipe = PipelinedInference(model, depth=inflight)
            for _ in range(inflight):
                pipe.submit(feats, (H, W))
            pipe.drain()
            for _ in range(args.warmup):
                pipe.submit(None, (H, W), slot_inputs=True)
            pipe.drain()
            one_piped = lambda: pipe.submit(None, (H, W), slot_inputs=True)
        single = None
        if full and pipe is not None:
            # one batch in flight, next to the headline (untimed for `value`): >= --steps, >= --min-seconds of work
            est = timed(one, 10)
            single_steps = max(args.steps, int(math.ceil(args.min_seconds / max(est, 1e-6))))
            single = timed(one, single_steps) * single_steps
        steps = args.steps                          # the same on every rank
        run_one = one_piped if pipe is not None else one
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            last = run_one()
        t_host = time.perf_counter() - t0           # the host's share: Python + hipGraphLaunch per step, the GPU running behind
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        # what the timed path returned for its last step: the slot's outputs (pipelined), the graph's (one graph) or the pass's (eager)
        outputs = pipe.result(last, wait="host") if pipe is not None else (out if graph is not None else last)
        checksum = float(outputs[0].double().sum().item())
        if args.dump_outputs and rank == 0:
            names = dump_outputs(outputs, args.dump_outputs)
            print(f"bench.py: outputs of the last timed step ({', '.join(names)}) written to {args.dump_outputs}", file=sys.stderr, flush=True)
        if full:
            # what one submit costs the host when the queue is NOT full (a full queue makes submit wait for the GPU: t_host above is
            # then the GPU's time): `inflight` submits into an empty pipeline -- one per slot, none of them waits for its slot's previous
            # replay --, best of three rounds
            host_submit_us = float("inf")
            for _ in range(3):
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(inflight):
                    run_one()
                host_submit_us = min(host_submit_us, 1e6 * (time.perf_counter() - t1) / inflight)
            torch.cuda.synchronize()
            if pipe is not None:                      # the pipelined slots computed what the single graph computes
                for a, b in zip(pipe.result(0, wait="host"), out):
                    assert torch.equal(a, b), "pipelined slot differs from the single-stream graph"

            # per-entry-point launch durations of three eager passes: HIP events on this stream around every library launch
            with _lib.CallTimer() as ct:
                for _ in range(3):
                    step()
                stream.synchronize()
            dur = ct.durations()
            mask_graph_ms, mask_calls = mask_step_graph_ms(step, model)
            # what the default plan runs for the ten predictions: one full-resolution launch, the pooling launch, nine key-resolution launches
            plan_ms, plan_calls = entry_graph_ms(step, ["mask_logits", "pool_mask_taps", "attn_mask_pooled"])
            enc_name = {"f32": "encoder_block", "f32_split": "encoder_block_split",
                        "bf16": "encoder_block_hm" if model.sem_seg_head.pixel_decoder._use_hm() else "encoder_block_lp",
                        "f16": "encoder_block_hm" if model.sem_seg_head.pixel_decoder._use_hm() else "encoder_block_lp"}[args.precision]
            enc_ms_all, enc_calls = entry_graph_ms(step, enc_name)
        launch_label = "eager" if graph is None and pipe is None else ("hipgraph" if pipe is None else
                                                                       f"hipgraph x{inflight}: {inflight} batches of 8 in flight, one graph + stream each")

    mine = {"images": (hi - lo) * steps, "elapsed_s": elapsed, "checksum": checksum, "pinned": float(affinity["status"] == "pinned")}
    if full:
        mine["host_submit_us"] = host_submit_us
    rec = gather_metrics(mine, dist, keys=tuple(mine))
    # BASELINE configs[2] is a bf16 configuration (batch 64 over 8 GPUs): every rank also times its batch of 8 in the low-precision
    # mode, same barriers, same max-over-ranks rule -- a `configs` entry of the line, never `value`
    lp_rec = None
    if full and args.precision == "f32" and not args.no_graph and not args.no_bf16_leg:
        del pipe, graph
        pipe = graph = None
        with torch.cuda.stream(stream):
            lp_images, lp_elapsed, lp_steps, lp_single, lp_roof = precision_leg(model, feats, dev, dist, args, "bf16", max(1, args.inflight))
            h_images, h_elapsed, h_steps, h_single, h_roof = precision_leg(model, feats, dev, dist, args, "f16", max(1, args.inflight))
        lp_rec = gather_metrics({"images": lp_images, "elapsed_s": lp_elapsed, "single_s": lp_single}, dist, keys=("images", "elapsed_s", "single_s"))
        h_rec = gather_metrics({"images": h_images, "elapsed_s": h_elapsed, "single_s": h_single}, dist, keys=("images", "elapsed_s", "single_s"))
    ag_s = timed_all_gather(dist) if full else None     # every rank takes part: the path's only collective, timed on its own
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return
    t_max = max(r["elapsed_s"] for r in rec)
    total_images = sum(r["images"] for r in rec)
    collective = collective_entry(dist, rec, ag_s, rccl_log)
    bf16 = args.precision in ("bf16", "f16")
    result = {
        "metric": METRIC,
        "value": round(total_images / t_max, 2),
        "unit": "images/sec",
        "n_gpus": world,
        "steps": steps,
        "steps_requested": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * t_max / steps, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32" if not bf16 else f"{args.precision} operands / fp32 accumulation (NOT the headline configuration)",
        "data": "synthetic",
        "config": {"workload": "configs[1]: batch 8 of 640x480 per GPU, ResNet-50 features -> MSDeformAttn pixel decoder -> 9-layer decoder, 100 q -> top-20",
                   "workload_detail": "configs[1]: batch=8 640x480 frames per GPU, synthetic ResNet-50 res2..res5 features "
                                      "-> MSDeformAttn pixel decoder (6 layers) -> 9-layer hypersphere decoder (100 queries) "
                                      "-> top-20 instance post-processing; backbone excluded",
                   "global_batch": world * BATCH, "per_gpu_batch": BATCH, "launch": launch_label,
                   "batches_in_flight": inflight,
                   "sparse_taps": bool(args.sparse_taps), "folded_mask_step": bool(pred.folded_mask_features),
                   "configs2_plan": "f16 (IEEE-half operands, fp32 accumulation); the bf16 plan is reported beside it as c2_bf16",
                   "parallelism": f"dp{world}"},
        "per_rank": [{"rank": i, "images_per_sec": round(r["images"] / r["elapsed_s"], 2), "checksum": r["checksum"],
                      "numa_pinned": bool(r["pinned"])} for i, r in enumerate(rec)],
        "roofline": {},
    }
    result["config"]["rank0_cpu_affinity"] = affinity
    result["config"]["GPU_MAX_HW_QUEUES"] = os.environ.get("GPU_MAX_HW_QUEUES")
    result["config"]["visible_gpus"] = have
    if not full:
        # a plain run: the headline and nothing else (the rest is --full's)
        result["collective"] = collective if world > 1 else {"world_size": 1}
        print(json.dumps(compact_line(result)), flush=True)
        if dist is not None:
            dist.destroy_process_group()
        return
    mask_name = "msm_mask_logits_bf16_fwd" if (bf16 and "msm_mask_logits_bf16_fwd" in dur) else "msm_mask_logits_fwd"
    per_call = dur[mask_name]
    calls_per_step = mask_calls
    mask_eager_ms = sum(per_call) / len(per_call)
    mask_ms = mask_graph_ms
    folded = bool(pred.folded_mask_features)
    c_exec = 64 if folded else C_MASK                       # channels the launched kernel contracts over
    flops_ref = 2.0 * Q * C_MASK * (H // 4) * (W // 4) * (hi - lo)         # the reference einsum
    flops_exec = 2.0 * Q * c_exec * (H // 4) * (W // 4) * (hi - lo)        # what the kernel issues
    # HBM traffic of the same kernel comes from separate rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE; the
    # gfx950 x2 correction on FETCH_SIZE applied), summarised in profiles/ -- it cannot be measured in-process
    traffic, traffic_tab, traffic_note = None, {}, []
    mt = load_traffic("mask_step_traffic.json", traffic_note)
    if mt is not None:
        traffic = mt.get("bytes_per_launch")
    traffic_tab = load_traffic("step_traffic.json", traffic_note) or {}
    pooled_plan = bool(pred.pooled_attention_masks) and folded
    # the mask step (the kernel BASELINE's metric names).  `kernel_*`: the full-resolution kernel characterised over the ten launches
    # of a pass that runs every prediction at 120 x 160 (comparable with rounds 1-3); `plan_*`: what the default plan launches for the
    # ten predictions of a pass, with the FLOPs it executes and the reference's over the same time
    t_lv = [(H // 32) * (W // 32), (H // 16) * (W // 16), (H // 8) * (W // 8)]
    flops_plan = flops_exec + (sum(2.0 * Q * c_exec * t_lv[i % 3] * (hi - lo) for i in range(9)) if pooled_plan else 9 * flops_exec)
    mask_step = {"kernel": mask_name.replace("msm_", "").replace("_fwd", "") + " (" + mask_name + ")",
                 "kernel_avg_launch_ms": round(mask_ms, 4), "kernel_launches_timed": calls_per_step,
                 "kernel_flops_per_launch": flops_exec, "kernel_achieved_tflops": round(flops_exec / (mask_ms * 1e-3) / 1e12, 2),
                 "kernel_frac_of_fp32_mfma_peak": round(flops_exec / (mask_ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS, 4),
                 "plan": ("1 full-resolution launch (final prediction) + 1 pooling launch + 9 launches at key resolution (300 / 1200 / 4800 keys): "
                          "interpolate(einsum(e, F)) = einsum(e, interpolate(F))") if pooled_plan else "10 full-resolution launches",
                 "plan_launches_per_step": plan_calls, "plan_ms_per_step": round(plan_ms, 4),
                 "plan_executed_flops_per_step": flops_plan, "plan_reference_flops_per_step": 10 * flops_ref,
                 "plan_executed_tflops": round(flops_plan / (plan_ms * 1e-3) / 1e12, 2) if plan_ms else None,
                 "plan_effective_tflops": round(10 * flops_ref / (plan_ms * 1e-3) / 1e12, 2) if plan_ms else None,
                 "traffic_final_launch": (traffic_tab.get("mask_logits_kernel_final") or {}).get("bytes_per_launch"),
                 "traffic_kernel_avg_launch": traffic,
                 "note": "kernel_*: FLOPs the full-resolution kernel executes (the folded step contracts e.Wm with the 64-channel FPN activation, "
                         "einsum(e, Wm a + bm) = einsum(e Wm, a) + e.bm, a quarter of the reference einsum's FLOPs) over its graph-timed launch; "
                         "plan_effective divides the reference's ten full contractions (SURVEY 8d) by the time the plan's launches take"}
    # the dominant kernel of the step by time: the fused encoder-layer tail (6 launches, ~40 % of the step)
    tokens = (hi - lo) * sum(t_lv)
    enc_ms = enc_ms_all / max(enc_calls, 1)
    # per token: out_proj 64x64, linear1 / linear2 64x1024 each, and (all but the last layer) the next layer's value projection 64x64 and
    # sampling projection 64x288
    enc_flops = [2.0 * tokens * (64 * 64 + 2 * 64 * 1024 + (64 * 64 + 64 * 288 if l < enc_calls - 1 else 0)) for l in range(enc_calls)]
    enc_fl = sum(enc_flops) / max(enc_calls, 1)
    enc_traffic = (traffic_tab.get("enc_block_kernel") or {}).get("bytes_per_launch") if args.precision == "f32" else None
    if args.precision == "f32":
        enc_peak, enc_fl_exec, enc_unit_note = PEAK_F32_MFMA_TFLOPS, enc_fl, "fp32 MFMA (v_mfma_f32_16x16x4_f32)"
    elif args.precision == "f32_split":
        enc_peak, enc_fl_exec, enc_unit_note = PEAK_BF16_MFMA_TFLOPS, 6.0 * enc_fl, "bf16 MFMA, six products per fp32 product"
    else:
        enc_peak, enc_fl_exec, enc_unit_note = PEAK_BF16_MFMA_TFLOPS, enc_fl, "bf16 MFMA"
    enc_ach = enc_fl_exec / (enc_ms * 1e-3) / 1e12 if enc_ms else 0.0
    roofline = {"bound": "mfma", "kernel": f"enc_block_kernel (msm_{enc_name}_fwd): fused encoder-layer tail, the step's dominant kernel by time",
                "achieved": round(enc_ach, 2), "peak": enc_peak, "unit": "TFLOP/s", "frac": round(enc_ach / enc_peak, 4), "traffic": enc_traffic,
                "launches_per_step": enc_calls, "avg_launch_ms": round(enc_ms, 4), "flops_per_launch": enc_fl_exec,
                "share_of_step": None,
                "timing": "HIP events on the launch stream around 100 graph replays of the step's encoder-block launches (back to back, real arguments)",
                "matrix_pipe": enc_unit_note,
                "algorithmic_bytes_per_launch": (traffic_tab.get("enc_block_kernel") or {}).get("algorithmic_bytes_per_launch"),
                "traffic_provenance": traffic_note,
                "traffic_source": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this workload, profiles/step_traffic.json (stamped with the kernel sources' SHA-256)",
                "mask_step": mask_step,
                "note": "rounds 1-3 put the mask step here; with the intermediate attention masks computed at key resolution it is 1-2 % of the "
                        "step, so the object describes the kernel that dominates (MFMA-bound: 315 kFLOP per token against 2.3 KB of traffic) and "
                        "carries the mask step's figures in `mask_step`"}
    # flat copies of what the driver's record must show (its parser keeps the scalar members of `roofline`): the strict one-batch
    # figure, the dominant kernel's share of THAT step, and the mask step (the kernel the metric names) as a fraction of the peak
    one_ms = 1e3 * single / single_steps if single is not None else 1e3 * t_max / steps
    roofline["share_of_step"] = round(enc_ms_all / one_ms, 3)
    roofline["share_of_step_basis"] = "encoder-block launches of one pass / one batch in flight"
    roofline["one_batch_in_flight_images_per_sec"] = round((hi - lo) / (one_ms * 1e-3), 1)
    roofline["one_batch_in_flight_ms"] = round(one_ms, 4)
    roofline["mask_step_frac"] = mask_step["kernel_frac_of_fp32_mfma_peak"]
    roofline["mask_step_avg_launch_ms"] = mask_step["kernel_avg_launch_ms"]
    roofline["mask_step_literal_frac"] = None           # filled from configs["configs[1] literal mask step"] below (N = 1 with extras)
    kernels = {k: {"launches_per_step": len(v) // 3, "ms_per_step": round(sum(v) / 3, 4), "avg_launch_us": round(1e3 * sum(v) / len(v), 2)}
               for k, v in sorted(dur.items(), key=lambda kv: -sum(kv[1]))}
    result["config"]["attention_masks_at_key_resolution"] = pooled_plan
    for p, r in zip(result["per_rank"], rec):
        p["host_submit_us_per_step"] = round(r["host_submit_us"], 1)
    result["roofline"] = roofline
    result["kernels"] = {"launch": "eager, HIP events on the launch stream around every library entry point, mean of 3 passes", "by_entry_point": kernels,
                         "sum_ms_per_step": round(sum(v["ms_per_step"] for v in kernels.values()), 4)}
    if single is not None:
        # rank 0's own clock, one batch in flight (one graph, one stream): the latency-oriented figure
        result["one_batch_in_flight"] = {"value": round((hi - lo) * single_steps / single, 2), "unit": "images/sec",
                                         "ms_per_step": round(1e3 * single / single_steps, 4), "steps": single_steps}
    # multi-GPU readiness (no 8-GPU node was available to the builder): what a rank's host spends per step, and the hardware-queue
    # budget the streams of the pipelined mode share
    result["host_submit_us_per_step"] = round(host_submit_us, 1)
    result["host_loop_share_of_step"] = round(t_host / elapsed, 3)
    if lp_rec is not None:
        lp_t = max(r["elapsed_s"] for r in lp_rec)
        result.setdefault("configs", {})["configs[2] bf16"] = {
            "workload": f"batch {world * BATCH} at 640x480 sharded over {world} GPU(s) (8 per GPU), bf16 MFMA operands / fp32 accumulation "
                        f"(set_precision('bf16')), {max(1, args.inflight)} batches of 8 in flight per GPU; BASELINE configs[2] is this at 8 GPUs",
            "value": round(sum(r["images"] for r in lp_rec) / lp_t, 1), "unit": "images/sec", "n_gpus": world, "steps": lp_steps,
            "ms_per_step": round(1e3 * lp_t / lp_steps, 4), "dtype": "bf16 operands / fp32 accumulation",
            "one_batch_in_flight": {"value": round(BATCH / lp_single, 1), "unit": "images/sec per GPU (rank 0)", "ms_per_step": round(1e3 * lp_single, 4)},
            "per_rank_images_per_sec": [round(r["images"] / r["elapsed_s"], 1) for r in lp_rec],
            "storage": "fp16 value / attention tensors and fp32-offset sampling records between the encoder kernels (csrc/enc_lp.hip), bf16 K/V, fp32 residual streams",
            "parity": "tests/test_gpu_configs.py::test_config2_slices_low_precision_vs_reference[bf16]: 1.07 % of the final mask bits, mean IoU 0.952 over 3200 masks",
            "roofline": lp_roof}
        h_t = max(r["elapsed_s"] for r in h_rec)
        # configs[2]'s headline entry: the 16-bit plan that meets SURVEY 8c's IoU >= 0.95 with margin (f16); the bf16 plan is listed beside it
        result["configs"]["configs[2]"] = {
            "workload": f"batch {world * BATCH} at 640x480 sharded over {world} GPU(s) (8 per GPU) under set_precision('f16'): the 16-bit plan with IEEE-half operands "
                        "(v_mfma_f32_16x16x32_f16, the bf16 instruction's rate) wherever the operand's range is bounded -- decoder tails, encoder FFN, "
                        "K/V projection + attention scores, FPN 3x3 convolution, mask step -- and bf16 where it is not (softmax weights, value rows)",
            "value": round(sum(r["images"] for r in h_rec) / h_t, 1), "unit": "images/sec", "n_gpus": world, "steps": h_steps,
            "ms_per_step": round(1e3 * h_t / h_steps, 4), "dtype": "fp16 / bf16 operands, fp32 accumulation",
            "one_batch_in_flight": {"value": round(BATCH / h_single, 1), "unit": "images/sec per GPU (rank 0)", "ms_per_step": round(1e3 * h_single, 4)},
            "per_rank_images_per_sec": [round(r["images"] / r["elapsed_s"], 1) for r in h_rec],
            "parity": "tests/test_gpu_configs.py::test_config2_slices_low_precision_vs_reference[f16]: 0.47 % of the final mask bits, mean IoU 0.979 over 3200 masks",
            "roofline": h_roof}
    if world == 1 and not args.no_extras:
        pipe = graph = None
        result["mean_shift"] = mean_shift_unit(dev)
        result.setdefault("configs", {}).update(extra_configs(dev, args))
    if not args.no_cpu_baseline and world == 1:
        result["cpu_baseline"] = cpu_baseline()
    lit = (result.get("configs") or {}).get("configs[1] literal mask step")
    if lit:
        result["roofline"]["mask_step_literal_frac"] = lit["roofline"]["frac"]
    if world > 1:
        result["collective"] = collective
    else:
        result["collective"] = {"world_size": 1, "note": "N = 1: no process group; an N > 1 line carries the RCCL version, the transport of every channel "
                                                         "(rank 0's NCCL_DEBUG=INFO log summarised), the all_gather's wall time and the per-rank spread here"}
    result["summary"] = build_summary(result)
    # stdout carries ONE compact line (<= LINE_BUDGET bytes: the driver's record holds the last 8 KB of stdout); the full document --
    # `kernels`, `configs`, `mean_shift`, per-rank detail -- goes to a file (copied to profiles/ from the builder's runs)
    detail = write_detail(result, args.detail or os.path.join(ROOT, "bench_out", "bench_full.json"))
    print(f"bench.py: full result ({len(json.dumps(result))} bytes) written to {detail}", file=sys.stderr, flush=True)
    print(json.dumps(compact_line(result, detail and os.path.relpath(detail, ROOT))), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
