"""bench.py -- train tokens/s (query+passage) of the CaSE model on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one optimizer step of the reference's training loop (CumulativeTrainer.train_batch: forward of
CaSE.do_train, three losses, backward, RCCL gradient all-reduce when N > 1, clip-norm 1, Adam, EMA, LR schedule)
on one synthetic batch already resident in HBM.  Workload (BASELINE.json configs[1]): CaSE, d_model 512, 6
encoder layers, 10 passages x 384 tokens, 64-token query, 40-token answer, batch 32 per GPU, bf16 compute,
dropout ON (counter RNG), full-length sequences (padded-dense FLOPs == useful FLOPs).  Weak scaling:
every rank runs the same per-GPU batch; value = N * B * (Lq + P*Lp) * K / max-over-ranks time.

`python bench.py --gpus N` with N > 1 and no torch.distributed environment starts the N ranks ITSELF: before anything touches
the GPU the parent spawns `python -m torch.distributed.run --nproc-per-node N bench.py ...` as a child process, relays rank 0's
JSON line and exits with the child's code (it never initialises the GPU).  The line carries `world_size` as
`dist.get_world_size()` reports it and every rank's own step time.

A plain run sets up, warms up, times the K steps, writes the last step's outputs if --dump-outputs is given and prints the
line.  Everything else the benchmark measures runs only with --full: the objects below, and in decode mode the one-token pass that
splits the step into its phases (``phases`` and ``roofline``).

--dump-outputs DIR writes what the timed path returned in its last step as DIR/<name>.npy (float32; float64 for the losses), at
most 64 MB in all.  Train modes: ``losses`` (the step's loss values) and ``params`` (a fixed, seeded sample of every parameter
after the step).  Decode mode: every tensor the model returns;
encoder mode: the encoder's output and state.  An array longer than DUMP_SAMPLE elements is cut to a fixed, seeded sample of its elements.

Extra objects in the JSON line (--full only):
  roofline      dominant kernel family (the bf16 MFMA GEMM instantiation with the largest total time): algorithmic
                FLOPs per launch / average launch duration, both measured live with HIP events on the launch stream
                over one instrumented step after the timed region; peak = 2516.6 TFLOP/s dense bf16.
  cpu_baseline  the CPU oracle (a port of the reference, oracle/) timed on this host's cores on a bounded sample
                (training steps at batch 1 of the same shapes, at the fastest of several thread counts), rank 0, N = 1 only.
  north_star    (default mode, N = 1) the encoder-forward point of BASELINE.json's target measured in the same process after
                the timed region: TransformerSeqEncoder forward at 64 x 10 x 384 tokens, 6 layers, ms / TFLOP/s / fraction of peak.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2516.6  # 256 CU x 2.4 GHz x 4096 flop/clk/CU (MI355X_MICROARCH.md: ~2.5 PF dense)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8, help="timed steps (at least 1)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true", help="also run the measurements beyond the timed steps: roofline, north-star and decode "
                                                        "points, CPU baseline, decode phase split")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's outputs as DIR/<name>.npy")
    ap.add_argument("--batch", type=int, default=32, help="per-GPU batch (BASELINE cfg 2: 32)")
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--enc-layers", type=int, default=6, help="BASELINE cfg 2 says 6; the reference hard-codes 3")
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--answer-len", type=int, default=40)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-north-star", action="store_true", help="skip the encoder-forward point appended to the default line")
    ap.add_argument("--no-decode-point", action="store_true", help="skip the greedy-decode point (cfg 4) appended to the default line")
    ap.add_argument("--no-dropout", action="store_true", help="diagnostic only: the BASELINE workload keeps dropout on")
    ap.add_argument("--ragged", action="store_true", help="diagnostic only: sequences of random length (half .. full) + one filler passage per item, as the "
                                                          "parity fixtures have them; the BASELINE workload is full-length (every row is a token)")
    ap.add_argument("--model", default="case", choices=["case", "masque"])
    ap.add_argument("--mode", default="train", choices=["train", "decode", "encoder", "cfg5", "refdefault"],
                    help="train: tokens/s of the training step (default, BASELINE cfg 2); decode: greedy answers/s (cfg 4); "
                         "encoder: the north-star point, TransformerSeqEncoder forward at batch x passages x passage-len; "
                         "cfg5: the long-context training step (d_model 768, 40 passages x 512 tokens, batch 4 per GPU) with the "
                         "HBM roofline of its long-memory cross-attention")
    ap.add_argument("--reserve-cus", type=int, default=None,
                    help="data parallel: compute units the persistent kernels leave to RCCL while collectives are in flight (default: "
                         "CASE_DP_RESERVE_CUS or 8); sweep 0 / 8 / 16 and compare data_parallel.allreduce_exposed_ms")
    ap.add_argument("--decode-len", type=int, default=64)
    ap.add_argument("--graph", action="store_true", help="decode: replay the whole greedy pass from one captured hipGraph; train modes: replay the "
                                                         "training step from a hipGraph recorded after three untimed eager steps (CumulativeTrainer(capture=True): "
                                                         "dropout base / LR / Adam scalars in device memory, new masks on every replay)")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if not a.full:
        a.no_cpu_baseline = a.no_roofline = a.no_north_star = a.no_decode_point = True
    return a


def forward_flops(a):
    """Algorithmic padded-dense forward FLOPs of one batch (2 x MACs of the GEMM-like terms; SURVEY 8d model)."""
    B, P, Lp, Lq, T, H, V = a.batch, a.passages, a.passage_len, a.query_len, a.answer_len, a.hidden, a.vocab
    S = P * Lp

    def enc_layer(L, E):  # QKV + out + FFN(E) GEMMs, QK^T + PV
        return 12 * L * E * E + 4 * L * L * E

    def block(L, Ein, Eout):  # QKV + out at Ein, attention at Ein, Linear(Ein->Eout), Linear(Eout->Eout)
        return 8 * L * Ein * Ein + 4 * L * L * Ein + 2 * L * Ein * Eout + 2 * L * Eout * Eout

    enc = a.enc_layers * (P * enc_layer(Lp, H) + enc_layer(Lq, H))
    inter = P * 10 * Lp * Lq * H
    sel_p = P * (block(Lp, 5 * H, H) + 4 * block(Lp, H, H))
    sel_q = block(Lq, 5 * H, H) + 2 * block(Lq, H, H)
    total = enc + inter + sel_p + sel_q
    if a.model == "case":
        total += inter + P * (block(Lp, 5 * H, H) + 2 * block(Lp, H, H)) + block(Lq, 5 * H, H) + block(Lq, H, H)

    def dec_stack(Sm):  # 4 layers: self-attn, cross-attn (K/V projection of the memory dominates), FFN
        per = 8 * T * H * H + 4 * T * T * H + 4 * T * H * H + 4 * Sm * H * H + 4 * T * Sm * H + 4 * T * H * H
        return 4 * per

    dec = dec_stack(Lq) + dec_stack(S)
    additive = 2 * (S + Lq) * H * H + 2 * T * (S + Lq) * H  # key projection + tanh scores
    gen = 2 * T * 3 * H * H + 2 * T * H * V
    return B * (total + dec + additive + gen)


def build(a, device):
    import case_rg_amd
    from case_rg_amd.common.CumulativeTrainer import CumulativeTrainer, init_params
    from case_rg_amd.common.schedule import get_cosine_with_hard_restarts_schedule_with_warmup
    from case_rg_amd.common.Utils import init_seed
    from case_rg_amd.utils import make_vocab, synth_batch

    case_rg_amd.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    case_rg_amd.set_dropout(not a.no_dropout)
    if os.environ.get("CASE_ATTENTION_MODE"):  # A/B switch: "fused" / "unfused" instead of the per-head-dim policy
        case_rg_amd.ops.ATTENTION_MODE = os.environ["CASE_ATTENTION_MODE"]
    if os.environ.get("CASE_GEMM_TILE"):  # A/B switch: force one GEMM tiling (64 / 128 / 256) instead of case_gemm's cost model
        case_rg_amd.ops.GEMM_TILE = int(os.environ["CASE_GEMM_TILE"])
    if os.environ.get("CASE_NO_FUSED_BIAS_GRAD"):  # A/B switch: bias gradients by the separate column-sum pass
        case_rg_amd.ops.FUSE_BIAS_GRAD = False
    init_seed(123456)  # the reference's seed (CaSE/Run.py:92)
    v2i, i2v = make_vocab(a.vocab)
    if a.model == "case":
        from case_rg_amd.CaSE.Model import CaSE
        model = CaSE(4, a.answer_len, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
    else:
        from case_rg_amd.Masque.Model import Masque
        model = Masque(a.answer_len, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
    init_params(model)
    trainer = CumulativeTrainer(model, None, None, device.index, a.gpus, capture=bool(getattr(a, "graph", False)) or None)
    from case_rg_amd.optim import FusedAdam
    # CaSE/Run.py:27 optim.Adam(lr=2.5e-4): same update rule; the trainer's clip / EMA and the bf16 operand refresh ride in its pass (K15)
    opt = FusedAdam(model.parameters(), lr=2.5e-4, low_precision=torch.bfloat16 if a.dtype == "bf16" else None)
    sched = get_cosine_with_hard_restarts_schedule_with_warmup(opt, 2000, 100000)
    rank = dist.get_rank() if dist.is_initialized() else 0
    batch = synth_batch(a.batch, a.passages, a.passage_len, a.query_len, a.answer_len, a.vocab, seed=123456 + rank,
                        ragged=bool(getattr(a, "ragged", False)), model=a.model)
    batch = {k: v.to(device) for k, v in batch.items()}
    trainer.model.train()
    return trainer, opt, sched, batch


def workload_key(a):
    """What a committed PMC summary was measured on: a traffic figure is attached only to a run of the SAME workload."""
    return "%s/b%d/h%d/p%dx%d/enc%d/%s" % (a.model, a.batch, a.hidden, a.passages, a.passage_len, a.enc_layers, a.dtype)


def pmc_traffic(kernel_key, workload, pattern="*_pmc_traffic.json"):
    """ARCHIVED HBM bytes per launch of ``kernel_key``: the newest committed PMC summary (profiles/*_pmc_traffic.json, made by
    tools/pmc_traffic.py from two rocprofv3 --pmc passes, see tools/r06_profiles.sh) whose ``workload`` equals this run's; files written
    before round 5 carry no key and are skipped (what they were measured on is not recorded in them).  (None, None) when there is
    none: a PMC number of another model / batch is never printed beside this run's timings."""
    import glob
    here = os.path.dirname(os.path.abspath(__file__))
    for path in reversed(sorted(glob.glob(os.path.join(here, "profiles", pattern)))):
        try:
            with open(path) as fh:
                rec = json.load(fh)
            if rec.get("workload") != workload:
                continue
            k = rec["kernels"].get(kernel_key)
            if k:
                return k["hbm_bytes_per_launch"], "profiles/" + os.path.basename(path)
        except (OSError, ValueError, KeyError):
            continue
    return None, None


def roofline_step(a, trainer, opt, sched, batch):
    """One extra training step with a HIP event pair around every GEMM launch (on the launch stream)."""
    from case_rg_amd import ops
    records = []
    raw = ops.gemm

    def timed_gemm(A_, B_, C_, M, N, K, *args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = raw(A_, B_, C_, M, N, K, *args, **kw)
        e1.record()
        tile = ops.TILE_TRACE[-1]  # which tiling case_gemm picks for this launch (rocprofv3 names the two kernels apart)
        key = "%s<%s,%s,%s,%s>" % ({256: "gemm8w_kernel", 64: "gemm_small_kernel"}.get(tile, "gemm_kernel"), "bf16" if A_.dtype == torch.bfloat16 else "f32",
                                   "bf16" if C_.dtype == torch.bfloat16 else "f32",
                                   "Ak" if kw.get("a_kmajor") else "A", "Bk" if kw.get("b_kmajor") else "B")
        nb = kw.get("batch1", 1) * kw.get("batch2", 1)
        # algorithmic HBM bytes of the launch: each operand once, C once (read-modify-write counts twice for split-K
        # accumulation), plus the epilogue's aux operand / saved pre-activation when present
        nbytes = nb * ((M * K + N * K) * A_.element_size() + M * N * C_.element_size() * (2 if kw.get("split_k", 1) > 1 else 1))
        nbytes += nb * M * N * A_.element_size() * ((kw.get("aux") is not None) + (kw.get("aux_out") is not None))
        records.append((key, 2.0 * M * N * K * nb, e0, e1, (M, N, K, nb, kw.get("split_k", 1)), nbytes))
        return out

    ops.gemm, ops.TILE_TRACE = timed_gemm, []
    graphs, trainer.graphs = trainer.graphs, None  # the instrumented step is an eager one (a replayed graph calls no Python)
    try:
        trainer.train_batch(0, dict(batch), "train", opt, sched)
        torch.cuda.synchronize()
    finally:
        ops.gemm, ops.TILE_TRACE = raw, None
        trainer.graphs = graphs
    fam = {}
    shapes = {}
    for key, flops, e0, e1, shape, nbytes in records:
        ms = e0.elapsed_time(e1)
        f = fam.setdefault(key, [0.0, 0.0, 0, 0.0])
        f[0] += flops
        f[1] += ms * 1e-3
        f[2] += 1
        f[3] += nbytes
        sh = shapes.setdefault((key,) + shape, [0.0, 0.0, 0])
        sh[0] += flops
        sh[1] += ms
        sh[2] += 1
    if os.environ.get("CASE_BENCH_SHAPES"):  # per-shape table for tuning (not part of the JSON line)
        with open(os.environ["CASE_BENCH_SHAPES"], "w") as fh:
            for k, v in sorted(shapes.items(), key=lambda kv: -kv[1][1]):
                fh.write("%-32s M=%-7d N=%-6d K=%-7d batch=%-5d split=%-3d  n=%-4d %8.3f ms  %7.1f TFLOP/s\n"
                         % (k[0], k[1], k[2], k[3], k[4], k[5], v[2], v[1], v[0] / v[1] / 1e9))
    key, (flops, secs, n, alg_bytes) = max(fam.items(), key=lambda kv: kv[1][1])
    achieved = flops / secs / 1e12
    traffic, traffic_src = pmc_traffic(key, workload_key(a))
    all_flops, all_secs = sum(v[0] for v in fam.values()), sum(v[1] for v in fam.values())
    return {"bound": "mfma", "kernel": key, "achieved": round(achieved, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": traffic, "traffic_source": traffic_src, "traffic_archived": traffic is not None,
            "algorithmic_bytes_per_launch": round(alg_bytes / n), "launches": n,
            "avg_launch_ms": round(secs / n * 1e3, 4), "flops_per_launch": flops / n,
            "all_gemm_tflops": round(all_flops / all_secs / 1e12, 1), "all_gemm_ms_per_step": round(all_secs * 1e3, 2),
            "families": {k: {"ms": round(v[1] * 1e3, 2), "tflops": round(v[0] / v[1] / 1e12, 1), "launches": v[2]} for k, v in fam.items()}}


def roofline_cross_attention(a, device):
    """cfg 5: the decoder's cross-attention over the S = P * Lp token memory (T = 40 query rows per item, head_dim H / 8) is
    HBM-bound on the K/V stream: 2 * S * H * 2 bytes per item and layer.  Timed in isolation on the model's shapes
    with HIP events on the launch stream (forward: split-KV kernel + merge)."""
    from case_rg_amd import ops
    N, h, T, S, d = a.batch, 8, a.answer_len, a.passages * a.passage_len, a.hidden // 8
    E = h * d
    q = (torch.randn(N, T, E, device=device) * 0.5).to(torch.bfloat16)
    kv = (torch.randn(N, S, 2 * E, device=device) * 0.5).to(torch.bfloat16)
    valid = torch.ones(N, S, dtype=torch.bool, device=device)
    with torch.no_grad():
        for _ in range(3):
            ops.attention(q, kv, kv, 0, 0, E, h, d, key_valid=valid)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        iters = 20
        e0.record()
        for _ in range(iters):
            ops.attention(q, kv, kv, 0, 0, E, h, d, key_valid=valid)
        e1.record()
        torch.cuda.synchronize()
    secs = e0.elapsed_time(e1) / iters * 1e-3
    nbytes = N * S * 2 * E * 2
    # ARCHIVED PMC bytes of the split-KV forward launch alone (tools/cfg5_stream.py under two rocprofv3 passes: tools/r05_profiles.sh)
    traffic, traffic_src = pmc_traffic("fa_fwd_kernel", workload_key(a), "*_cfg5stream_pmc.json")
    return {"bound": "hbm", "kernel": "fa_fwd_kernel<96, split-KV> + fa_combine_kernel<96> (decoder cross-attention, S = %d)" % S,
            "achieved": round(nbytes / secs / 1e9, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(nbytes / secs / 8e12, 4),
            "traffic": traffic, "traffic_source": traffic_src, "traffic_archived": traffic is not None, "algorithmic_bytes_per_launch": nbytes,
            "avg_launch_ms": round(secs * 1e3, 4),
            "launches_per_step": "8 forward (2 stacks x 4 layers; the query-memory stack has S = %d)" % a.query_len}


def _thread_candidates(cores):
    return sorted({c for c in (8, 16, 32, cores) if 0 < c <= cores})


def cpu_baseline(a, max_passages=None):
    """The CPU oracle (fp32 port of the reference, oracle/) on this host: training steps (fwd + bwd + clip + Adam) at batch 1 of
    the same shapes, ALL P passages.  The thread count matters more than the core count (128 threads ran 4.5x SLOWER than 8 in
    round 2: oversubscribed intra-op pools), so the leg first probes one step at 8 / 16 / 32 / all threads on a 4-passage sample,
    then reports as ``value`` the median of three full-size steps at the FASTEST setting (``cores`` = that thread count); every
    probe is listed in ``by_threads``.  The oracle forms the Interaction scores from two small matrix products instead of the
    reference's [P, Lp, Lq, 3H] tensor, so it is FASTER than the reference itself would be on this host."""
    import statistics
    import oracle
    from case_rg_amd.utils import fill_params, make_vocab, synth_batch
    v2i, i2v = make_vocab(a.vocab)
    if a.model == "case":
        m = oracle.CaSE(4, a.answer_len, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
    else:
        m = oracle.Masque(a.answer_len, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
    fill_params(m, 1).train()
    opt = torch.optim.Adam(m.parameters(), lr=2.5e-4)

    def step(b):
        t0 = time.time()
        losses = m(dict(b), method="train")
        sum(l.mean() for l in losses).backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1)
        opt.step()
        opt.zero_grad()
        return time.time() - t0

    host = torch.get_num_threads()
    Ps = min(4, a.passages)
    Pf = a.passages if max_passages is None else min(a.passages, max_passages)  # cfg 5 (40 x 512, H 768): a bounded sample of the passages
    probe = synth_batch(1, Ps, a.passage_len, a.query_len, a.answer_len, a.vocab, seed=7, ragged=False, model=a.model)
    full = synth_batch(1, Pf, a.passage_len, a.query_len, a.answer_len, a.vocab, seed=7, ragged=False, model=a.model)
    tok_probe, tok_full = a.query_len + Ps * a.passage_len, a.query_len + Pf * a.passage_len
    by_threads = {}
    torch.set_num_threads(min(8, host))
    step(probe)  # warm-up (allocator, thread pool, first-call overheads)
    for n in _thread_candidates(host):
        torch.set_num_threads(n)
        step(probe)
        by_threads[str(n)] = round(tok_probe / step(probe), 1)
    best = int(max(by_threads, key=lambda k: by_threads[k]))
    torch.set_num_threads(best)
    step(full)
    times = [step(full) for _ in range(3)]
    med = statistics.median(times)
    torch.set_num_threads(host)
    return {"value": round(tok_full / med, 1), "unit": "tokens/s", "cores": best, "host_cores": host, "kind": "port",
            "by_threads": by_threads,
            "sample": "fp32 CPU oracle (decomposed Interaction: faster than the reference's own formulation), batch 1 x %d passages x %d "
                      "tokens, fwd+bwd+clip+Adam; thread count probed on a %d-passage step (tokens/s by threads in by_threads), then 1 "
                      "warm-up + median of 3 full steps at the fastest setting, %d threads (%.1f s each)" % (
                          Pf, a.passage_len, Ps, best, med)}


def cpu_baseline_decode(a):
    """Decode leg of the CPU baseline: the oracle's greedy ``do_test`` (the reference's own O(T^2) loop, CaSE/Model.py:91-123: the
    whole prefix is re-decoded every step) for ONE query with all P passages and the full T-token answer, on the thread count that
    is fastest for it (probed on a 4-token answer)."""
    import oracle
    from case_rg_amd.utils import fill_params, make_vocab, synth_batch
    v2i, i2v = make_vocab(a.vocab)
    m = fill_params(oracle.CaSE(4, a.decode_len, i2v, v2i, a.hidden, enc_layers=a.enc_layers), 1).eval()
    b = synth_batch(1, a.passages, a.passage_len, a.query_len, a.answer_len, a.vocab, seed=7, ragged=False)
    host = torch.get_num_threads()

    def run(T):
        m.max_target_length = T
        t0 = time.time()
        with torch.no_grad():
            m(dict(b), method="test")
        return time.time() - t0

    by_threads = {}
    torch.set_num_threads(min(8, host))
    run(2)
    for n in _thread_candidates(host):
        torch.set_num_threads(n)
        by_threads[str(n)] = round(1.0 / run(4), 3)
    best = int(max(by_threads, key=lambda k: by_threads[k]))
    torch.set_num_threads(best)
    t = run(a.decode_len)
    torch.set_num_threads(host)
    return {"value": round(1.0 / t, 4), "unit": "answers/s", "cores": best, "host_cores": host, "kind": "port",
            "by_threads_4_token_answers_per_s": by_threads,
            "sample": "fp32 CPU oracle, the reference's O(T^2) greedy loop (prefix re-decoded every step, no KV cache), 1 query x %d passages "
                      "x %d tokens, %d-token answer, one pass on %d threads (%.1f s)" % (a.passages, a.passage_len, a.decode_len, best, t)}


def case_rg_amd_reset(a):
    """Back to the training line's compute settings after an appended measurement changed them."""
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    case_rg_amd.set_dropout(not a.no_dropout)


def decode_main(a, device, world, rank):
    res = decode_measure(a, device, world, rank)
    if rank == 0 and world == 1 and not a.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline_decode(a)
    if rank == 0:
        emit(res)


def decode_point(a, device):
    """cfg 4 (BASELINE.json configs[3]: greedy decode, batch 256, 64-token answers, hipGraph-captured step) measured in the same process after
    the training line, so that the driver's default run also carries the decode step's HBM roofline fraction.  The pass is measured BOTH ways --
    replayed from a hipGraph (BASELINE's wording; independent of the box's host speed: a cached step is ~120 launches in ~2.2 ms, which a slow
    host turns launch-bound: 2.52 ms seen) and launched eagerly (on a fast host 2-7 % quicker than the replay: hipGraph nodes cost more per
    launch than this pool's eager queue) -- 3 timed passes after 1 warm-up each; the faster one is the point, both are recorded."""
    import copy
    both = {}
    for name, graph in (("hipgraph_replay", True), ("eager", False)):
        b = copy.copy(a)
        b.batch, b.steps, b.warmup, b.graph, b.mode = 256, 3, 1, graph, "decode"
        r = decode_measure(b, device, 1, 0)
        both[name] = {"workload": r["config"]["workload"], "answers_per_s": r["value"], "ms_per_cached_step": r["phases"]["ms_per_cached_step"],
                      "encode_plus_first_step_ms": r["phases"]["encode_plus_first_step_ms"], "roofline": r["roofline"]}
        torch.cuda.empty_cache()
    best = max(both, key=lambda k: both[k]["answers_per_s"])
    out = dict(both[best])
    out["path"] = best
    out["by_path"] = {k: {"answers_per_s": v["answers_per_s"], "ms_per_cached_step": v["ms_per_cached_step"]} for k, v in both.items()}
    return out


def decode_measure(a, device, world, rank):
    """cfg 4: greedy inference, B queries x P passages, T-token answers; a "step" = one whole batch (encode + T cached steps)."""
    import case_rg_amd
    from case_rg_amd.common.CumulativeTrainer import init_params
    from case_rg_amd.common.Utils import init_seed
    from case_rg_amd.utils import make_vocab, synth_batch
    case_rg_amd.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    init_seed(123456)
    v2i, i2v = make_vocab(a.vocab)
    from case_rg_amd.CaSE.Model import CaSE
    model = CaSE(4, a.decode_len, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
    init_params(model)
    model = model.to(device).eval()
    batch = synth_batch(a.batch, a.passages, a.passage_len, a.query_len, a.answer_len, a.vocab, seed=123456 + rank, ragged=False)
    batch = {k: v.to(device) for k, v in batch.items()}

    def run():
        with torch.no_grad():
            return model(dict(batch), method="test")

    graph = None
    for _ in range(max(1, a.warmup)):
        out = run()
    if a.graph:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = run()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    fence()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        if graph is not None:
            graph.replay()
        else:
            out = run()
    fence()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if a.dump_outputs is not None and rank == 0:
        dump_outputs(a.dump_outputs, out)
    res = {
        "metric": "decode answers/sec (CaSE greedy)", "value": round(world * a.batch * a.steps / elapsed, 2), "unit": "answers/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 2),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": "CaSE greedy decode (encode + %d KV-cached steps), d_model=%d, %d encoder layers, %d passages x %d tok, "
                               "per-GPU batch %d%s" % (a.decode_len, a.hidden, a.enc_layers, a.passages, a.passage_len, a.batch,
                                                       ", hipGraph replay" if a.graph else ""),
                   "global_batch": world * a.batch, "parallelism": "dp%d" % world},
        "answer_sample": out["answer"][0, :8].tolist(),
        "world_size": dist.get_world_size() if dist.is_initialized() else 1,
    }
    if not a.full:
        return res
    # phase split (rank 0): the same batch with a ONE-token answer = encode + projections of the memories + one cached step;
    # the cached step itself = (T-token pass - 1-token pass) / (T - 1)
    S, H, T = a.passages * a.passage_len + a.query_len, a.hidden, a.decode_len
    model.max_target_length = 1
    run()
    run_one = run
    if a.graph:  # the one-token pass replays from its own graph, like the full pass
        torch.cuda.synchronize()
        graph1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph1):
            run()
        run_one = graph1.replay
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(a.steps):
        run_one()
    torch.cuda.synchronize()
    one = (time.perf_counter() - t1) / a.steps
    model.max_target_length = T
    step_s = max(1e-9, (elapsed / a.steps - one) / max(1, T - 1))
    # algorithmic bytes streamed per item per cached step (SURVEY 8d cfg 4): 2 stacks x 4 layers x (K + V) of each memory in
    # bf16 + the additive-attention key cache of each memory
    bytes_item_step = (4 * 2 * S * H + S * H) * 2
    gbps = bytes_item_step * a.batch / step_s / 1e9
    # what the step actually MOVES since round 5: K21 attends the raw passage-memory rows (ONE stream of Sp x H per layer
    # instead of K and V), the 64-token query memory keeps its cached K / V, and the additive attention streams e^{2 uh} AND the value rows
    Sp, Lq = a.passages * a.passage_len, a.query_len
    moved_item_step = (4 * Sp * H + 4 * 2 * Lq * H + 2 * (Sp + Lq) * H) * 2
    moved_gbps = moved_item_step * a.batch / step_s / 1e9
    res.update({
        "phases": {"encode_plus_first_step_ms": round(one * 1e3, 2), "ms_per_cached_step": round(step_s * 1e3, 3),
                   "cached_steps": T - 1},
        "roofline": {"bound": "hbm", "kernel": "KV-cached greedy step (cross-attention K/V + additive-attention key streams)",
                     "achieved": round(gbps, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(gbps / 8000.0, 4), "traffic": None,
                     "algorithmic_bytes_per_step": bytes_item_step * a.batch,
                     "moved_bytes_per_step": moved_item_step * a.batch, "moved_gbps": round(moved_gbps, 1), "moved_frac": round(moved_gbps / 8000.0, 4),
                     "note": "achieved / frac price the step against SURVEY 8d's algorithm (K + V of four layers per memory + the additive keys); moved_* "
                             "against the bytes this implementation streams (absorbed cross-attention: one stream per layer; + the pointer context's value rows)"},
    })
    return res


def encoder_point(a, device, batch=None, steps=None, warmup=None):
    """North-star point: CaSE encoder forward, B x P x Lp tokens; returns (seconds per forward, algorithmic FLOPs, the last
    forward's output)."""
    import case_rg_amd
    from case_rg_amd.common.CumulativeTrainer import init_params
    from case_rg_amd.common.TransformerSeqEncoderDecoder import TransformerSeqEncoder
    from case_rg_amd.utils import synth_batch
    batch, steps, warmup = batch or a.batch, steps or a.steps, a.warmup if warmup is None else warmup
    case_rg_amd.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    enc = TransformerSeqEncoder(a.enc_layers, 8, a.vocab, a.hidden)
    init_params(enc)
    enc = enc.to(device).eval()
    ids = synth_batch(batch, a.passages, a.passage_len, a.query_len, a.answer_len, a.vocab, ragged=False)["passage"].to(device)
    with torch.no_grad():
        for _ in range(max(1, warmup)):
            enc(ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = enc(ids)
        torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    L, H, n = a.passage_len, a.hidden, batch * a.passages
    return dt, a.enc_layers * n * (12 * L * H * H + 4 * L * L * H), out


def encoder_main(a, device):
    dt, flops, out = encoder_point(a, device)
    if a.dump_outputs is not None:
        dump_outputs(a.dump_outputs, {"encoder_output": out[0], "encoder_state": out[1]})
    L, H, n = a.passage_len, a.hidden, a.batch * a.passages
    emit({"metric": "CaSE encoder forward (north-star point)", "value": round(n * L / dt, 1), "unit": "tokens/s", "n_gpus": 1,
                      "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt * 1e3, 3), "higher_is_better": True, "dtype": a.dtype,
                      "data": "synthetic", "config": {"workload": "TransformerSeqEncoder forward, %d layers, d_model %d, %d x %d x %d tokens" % (
                          a.enc_layers, H, a.batch, a.passages, L)},
                      "roofline": {"bound": "mfma", "achieved": round(flops / dt / 1e12, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                                   "frac": round(flops / dt / 1e12 / PEAK_BF16_TFLOPS, 4), "algorithmic_tflop": round(flops / 1e12, 3)}})


def north_star_point(a, device):
    """The target point of BASELINE.json (encoder forward at batch 64 x 10 passages x 384 tokens, bf16, eval mode), measured in
    the default run so that the driver's own bench line carries it."""
    dt, flops, _ = encoder_point(a, device, batch=64, steps=10, warmup=2)
    return {"workload": "TransformerSeqEncoder forward, %d layers, d_model %d, 64 x %d x %d tokens, bf16, eval" % (
                a.enc_layers, a.hidden, a.passages, a.passage_len),
            "batch": 64, "layers": a.enc_layers, "ms": round(dt * 1e3, 3), "tflops": round(flops / dt / 1e12, 1),
            "frac": round(flops / dt / 1e12 / PEAK_BF16_TFLOPS, 4), "target_frac": 0.5}


def spawn_ranks(a):
    """`python bench.py --gpus N` (N > 1) outside torch.distributed.run: start the N ranks as a CHILD process tree and relay its
    output.  Runs before this process has touched the GPU (torch.cuda.device_count() does not initialise it), and this process
    never does -- a program that holds the GPU must not be replaced by, or fork, another one on this pool."""
    have = torch.cuda.device_count()
    if have < a.gpus and not os.environ.get("CASE_BENCH_SHARE_GPU"):
        raise SystemExit("bench.py --gpus %d: this node shows %d GPU(s)" % (a.gpus, have))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL's cross-process buffers need it on this pool
    env.setdefault("OMP_NUM_THREADS", "8")
    proc = subprocess.run(cmd, env=env)
    raise SystemExit(proc.returncode)


DUMP_SAMPLE = 1 << 20  # elements kept of a longer output array (4 MB in float32)
DUMP_PER_PARAM = 4096  # elements sampled from each parameter tensor
DUMP_SEED = 20241016


def param_sample(model):
    """A fixed, seeded sample of every parameter (named_parameters order, at most DUMP_PER_PARAM elements each), as one f32 vector on
    the device.  The indices depend only on the parameter shapes, so two runs of the same arguments sample the same elements."""
    g = torch.Generator().manual_seed(DUMP_SEED)
    parts = []
    for _, p in model.named_parameters():
        flat = p.detach().reshape(-1)
        if flat.numel() > DUMP_PER_PARAM:
            flat = flat[torch.randint(flat.numel(), (DUMP_PER_PARAM,), generator=g).to(flat.device)]
        parts.append(flat.float())
    return torch.cat(parts)


def dump_outputs(path, arrays):
    """--dump-outputs: each array as <path>/<name>.npy, float64 kept as float64 and everything else as float32; an array of more than
    DUMP_SAMPLE elements is cut to a fixed, seeded sample of its flattened elements."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        t = torch.as_tensor(t).detach().reshape(-1)
        if t.numel() > DUMP_SAMPLE:
            g = torch.Generator().manual_seed(DUMP_SEED)
            t = t[torch.randint(t.numel(), (DUMP_SAMPLE,), generator=g).to(t.device)]
        arr = (t.double() if t.dtype == torch.float64 else t.float()).cpu().numpy()
        total += arr.nbytes
        if total > 64 << 20:
            raise SystemExit("bench.py --dump-outputs: more than 64 MB of outputs")
        np.save(os.path.join(path, name + ".npy"), arr)


_REAL_STDOUT = None


def emit(obj):
    """The ONE JSON line of the contract, on the process's original stdout.  RCCL 2.26 prints a five-line version banner to stdout when
    its first communicator is created (seen in the one-rank rehearsal, round 5): main() therefore points file descriptor 1 at stderr for
    the whole run and keeps the original for this call, so that whatever a library prints, stdout carries exactly one line."""
    line = (json.dumps(obj) + "\n").encode()
    if _REAL_STDOUT is None:
        sys.stdout.write(line.decode())
        sys.stdout.flush()
    else:
        os.write(_REAL_STDOUT, line)


def main():
    global _REAL_STDOUT
    a = parse()
    if "WORLD_SIZE" not in os.environ and (a.gpus > 1 or os.environ.get("CASE_BENCH_FORCE_SPAWN")):
        spawn_ranks(a)  # CASE_BENCH_FORCE_SPAWN: rehearse the self-launch with --gpus 1 on a one-GPU box
    os.environ.setdefault("NCCL_DEBUG", "WARN")
    sys.stdout.flush()
    _REAL_STDOUT = os.dup(1)
    os.dup2(2, 1)  # library chatter (the RCCL banner) goes to stderr
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus and not (world == 1 and a.gpus <= 1):
        raise SystemExit("bench.py --gpus %d was started with WORLD_SIZE=%d: launch one rank per GPU" % (a.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path has no CPU fallback")
    # CASE_BENCH_SHARE_GPU=1 (rehearsal on a one-GPU box, never a measurement): every rank runs on device 0 and the collectives go
    # through gloo -- RCCL refuses two ranks on one device; the launch, the rank bookkeeping and GradSync's bucket protocol are the real ones
    share = bool(os.environ.get("CASE_BENCH_SHARE_GPU"))
    if share:
        local = 0
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        if share:
            dist.init_process_group(backend="gloo", init_method="env://")
        else:
            dist.init_process_group(backend="nccl", init_method="env://", device_id=device)
    elif os.environ.get("CASE_FORCE_GRADSYNC"):  # rehearsal of the multi-GPU path on one GPU: a one-rank RCCL group, buckets + hooks live
        # (under torch.distributed.run the agent's store must be used -- an explicit tcp:// address makes the worker a CLIENT of a
        # store nobody serves and the rendezvous hangs)
        if "MASTER_ADDR" in os.environ and "RANK" in os.environ:
            dist.init_process_group(backend="nccl", init_method="env://", device_id=device)
        else:
            dist.init_process_group(backend="nccl", init_method="tcp://127.0.0.1:29577", rank=0, world_size=1, device_id=device)
    rank = dist.get_rank() if world > 1 else 0
    if a.mode == "encoder":
        if rank == 0:
            encoder_main(a, device)
        return
    if a.mode == "cfg5":  # BASELINE cfg 5: 40 passages x 512 tokens, d_model 768, 4 items per GPU; the reference's 3 encoder layers
        a.hidden, a.passages, a.passage_len, a.enc_layers = 768, 40, 512, 3
        a.batch = 4 if a.batch == 32 else a.batch
    if a.mode == "refdefault":
        # the reference's OWN default geometry (CaSE/Run.py:72-78: hidden 256, batch 16 per GPU; Prepare_dataset.py:13-17: query 60, passage
        # 100 tokens, 10 passages, answers of 40; CaSE/Model.py's 3 encoder layers): head_dim 32 in the encoder / H-wide blocks / decoder and
        # 160 in the 5H blocks -- what "drops into Run.py unchanged" lands on.  Reported like the training line; no roofline object.
        a.hidden, a.passages, a.passage_len, a.query_len, a.answer_len, a.enc_layers = 256, 10, 100, 60, 40, 3
        a.batch = 16 if a.batch == 32 else a.batch
        a.no_roofline, a.no_north_star, a.no_cpu_baseline, a.mode = not (a.full and os.environ.get("CASE_BENCH_SHAPES")), True, True, "train"  # (the per-shape tuning table rides on the roofline pass)
        a.refdefault = True
    if a.mode == "decode":
        decode_main(a, device, world, rank)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    if a.reserve_cus is not None:
        os.environ["CASE_DP_RESERVE_CUS"] = str(a.reserve_cus)
    trainer, opt, sched, batch = build(a, device)
    ranks_seen = None
    if dist.is_initialized():  # self-certification of the collective: a real 1-element all-reduce(SUM) of ones over the process group
        one = torch.ones(1, device=device)
        dist.all_reduce(one, op=dist.ReduceOp.SUM)
        ranks_seen = int(round(float(one.item())))
        if ranks_seen != max(1, a.gpus):  # a run mislabelled as N GPUs must not print a line
            raise SystemExit("bench.py --gpus %d: the all-reduce over the process group saw %d rank(s)" % (a.gpus, ranks_seen))

    def step():
        return trainer.train_batch(0, dict(batch), "train", opt, sched)

    if trainer.graphs is not None:  # captured steps: two eager steps + the recording pass happen before the contract's warm-up
        for _ in range(3 + (3 if trainer.graphs.auto else 0)):  # auto: + the three timed replays after which a capture that does not pay is dropped
            step()
        assert trainer.graphs.replays >= 1, "the training step was not captured"
    for _ in range(a.warmup):
        step()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    fence()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        losses = step()
    fence()
    elapsed = time.perf_counter() - t0
    if a.dump_outputs is not None and rank == 0:
        dump_outputs(a.dump_outputs, {"losses": torch.tensor(losses, dtype=torch.float64), "params": param_sample(trainer.model)})
    rank_ms = [round(elapsed / a.steps * 1e3, 2)]
    if world > 1:
        every = [torch.zeros(1, device=device, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(every, torch.tensor([elapsed], device=device, dtype=torch.float64))
        rank_ms = [round(float(t.item()) / a.steps * 1e3, 2) for t in every]
        elapsed = max(float(t.item()) for t in every)

    tokens_per_step = world * a.batch * (a.query_len + a.passages * a.passage_len)
    value = tokens_per_step * a.steps / elapsed
    fwd = forward_flops(a)
    out = {
        "metric": "train tokens/sec (query+passage) CaSE model" if a.model == "case" else "train tokens/sec (query+passage) Masque model",
        "value": round(value, 1), "unit": "tokens/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(elapsed / a.steps * 1e3, 2), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": a.dtype, "data": "synthetic",
        "config": {"workload": "%s train step fwd+bwd+allreduce+clip+Adam+EMA, d_model=%d, %d encoder layers, %d passages x %d tok, "
                               "query %d, answer %d, vocab %d, per-GPU batch %d, dropout %s" % (
                                   "CaSE" if a.model == "case" else "Masque", a.hidden, a.enc_layers, a.passages, a.passage_len,
                                   a.query_len, a.answer_len, a.vocab, a.batch, ("off (diagnostic)" if a.no_dropout else "on") +
                                   (", step replayed from a hipGraph" if trainer.graphs is not None and trainer.graphs.graphs else "") +
                                   (", RAGGED lengths (diagnostic: padding is counted as tokens)" if getattr(a, "ragged", False) else "")),
                   "global_batch": world * a.batch, "parallelism": "dp%d" % world,
                   "algorithmic_tflop_per_step": round(3 * fwd * world / 1e12, 2)},
        "step_mfma_frac": round(3 * fwd / (elapsed / a.steps) / 1e12 / PEAK_BF16_TFLOPS, 4),
        "last_losses": [round(x, 4) for x in losses],
        "world_size": dist.get_world_size() if dist.is_initialized() else 1, "rank_ms_per_step": rank_ms,
        "rccl_ranks_seen": ranks_seen, "collective_backend": dist.get_backend() if dist.is_initialized() else None,
    }
    if trainer.sync is not None and trainer.sync.active:
        # how long the compute stream stood still in GradSync.finish() per step (HIP events around the waits, this rank; the timed
        # steps only): the part of the gradient all-reduce that backward did not hide
        from case_rg_amd import _abi as _A
        out["data_parallel"] = {"allreduce_exposed_ms": round(trainer.sync.exposed_ms(last=a.steps), 3), "buckets": len(trainer.sync.buckets),
                                "bucket_mb": round(max(b["flat"].numel() for b in trainer.sync.buckets) * 4 / 2 ** 20, 1),
                                "gradient_mb": round(sum(b["flat"].numel() for b in trainer.sync.buckets) * 4 / 2 ** 20, 1),
                                "wire_dtype": "bf16" if trainer.sync.comm_dtype is not None else "f32",
                                "reserved_cus": int(getattr(trainer.sync, "reserved_cus", 0)), "reserved_while": "first all-reduce of the step .. finish()"}
    if getattr(a, "refdefault", False):
        out["metric"] += ", the reference's default geometry (hidden 256, 10 x 100-token passages, batch 16)"
    if a.mode == "cfg5":
        out["metric"] += ", cfg 5 long context"
        if rank == 0 and not a.no_roofline:
            out["roofline"] = roofline_cross_attention(a, device)
        elif world > 1 and not a.no_roofline:
            pass
    elif rank == 0 and not a.no_roofline:
        out["roofline"] = roofline_step(a, trainer, opt, sched, batch)
    elif world > 1 and not a.no_roofline:
        step()  # keep the ranks in lock-step with rank 0's instrumented step (it contains an all-reduce)
    if rank == 0 and world == 1 and a.mode == "train" and a.model == "case" and not a.no_north_star:
        trainer.close()
        del trainer, opt, sched  # the training step's parameters, moments and cached operand copies are not needed any more
        torch.cuda.empty_cache()
        out["north_star"] = north_star_point(a, device)
        if not a.no_decode_point and a.hidden == 512 and a.passages * a.passage_len == 3840:
            torch.cuda.empty_cache()
            out["decode_point"] = decode_point(a, device)
            case_rg_amd_reset(a)
    if rank == 0 and world == 1 and not a.no_cpu_baseline and a.mode == "train":
        out["cpu_baseline"] = cpu_baseline(a)
    if rank == 0 and world == 1 and not a.no_cpu_baseline and a.mode == "cfg5":
        out["cpu_baseline"] = cpu_baseline(a, max_passages=8)  # 8 of the 40 passages: ~20 s of CPU work per step
    if rank == 0:
        emit(out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
