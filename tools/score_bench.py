#!/usr/bin/env python
"""Teacher-forced scoring: K29 next to the unfused head chain, and whole ``do_score`` passes next to the greedy pass of the same items.

    python tools/score_bench.py [--out profiles/score_bench.json]

Kernel ("kernel" in the json): --rows x V 30 522 (2048 rows = one default head chunk), S = 64 + 3840 source keys, one key row per
--rows-per-source rows.  Two variants on the same build, ALTERNATING inside a repeat, device events around --kernel-iters launches:
  K29      ops.pointer_head_score: one read of the logits, nothing written but two floats per row;
  chain    the launches the unfused path runs on the same inputs: masked_softmax over the logits, p0 x gen, the sorted scatter on top of it
           (which clones its base), and the per-row gather of -log p (nll_rows).
Every launch of a repeat reads a DIFFERENT logits buffer of a ring that is larger than the Infinity Cache (256 MB), so the logits come
from HBM, as they do behind a vocabulary GEMM that has just written 250 MB.  Bytes are counted from the shapes: K29 reads R V 4 (the
logits; the keys and copy weights it touches are below 1 % of that); the chain moves R V 4 six times (softmax read + write, p0 x gen read +
write, the scatter's clone of its base read + write; the scatter itself and the gather touch a few entries per row, and the mixing
softmax and the pointer product are [R, S]-sized).  "hbm_fraction" = bytes / time / 8.0 TB/s (the spec peak;
a float4 copy measures 6.29 TB/s on this part).
Passes ("passes"): ``do_score`` at B --batch, T --decode-len, N in {1, 4} and the greedy pass of the same items (bf16, eager launches), the
host clock around a pass that ends in a synchronise, alternating; and ``torch.cuda.max_memory_allocated`` of the fused and the unfused
scoring pass (N = 1).
The event windows hold the wrappers' host work too, so they bound a kernel's time from above.  Stand-alone: bench.py does not call this.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--rows-per-source", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--decode-len", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--enc-layers", type=int, default=3)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ring", type=int, default=3, help="logits buffers the launches rotate over")
    ap.add_argument("--skip-passes", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
    return ap.parse_args()


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/score_bench.py measures on the GPU; there is none here")
    import case_rg_amd
    from case_rg_amd import ops
    dev = torch.device("cuda")

    def kernel():
        R, V, rps = a.rows, a.vocab, a.rows_per_source
        lens = [a.query_len, a.passages * a.passage_len]
        S = sum(lens)
        g = torch.Generator(device="cuda").manual_seed(3)
        ring = [torch.randn(R, V, device=dev, generator=g) * 2.0 for _ in range(a.ring)]
        mix = torch.randn(R, 1 + len(lens), device=dev, generator=g)
        src = ops.SortedSource(torch.randint(4, V, (R // rps, S), device=dev, generator=g), V)
        rows = src.select(torch.arange(R, device=dev) // rps)  # the chain scatters per row: its item's keys beside every row
        copies = [torch.softmax(torch.randn(R, n, device=dev, generator=g) * 2.0, dim=-1) for n in lens]
        targets = torch.randint(4, V, (R,), device=dev, generator=g)
        targets[::2] = src.ids[torch.arange(0, R, 2, device=dev) // rps, 7]  # half the targets occur in their source
        turn = [0]

        def k29():
            turn[0] += 1
            return ops.pointer_head_score(ring[turn[0] % a.ring], mix, src, rps, copies, targets, pad=0)

        def chain():
            turn[0] += 1
            gen = ops.masked_softmax(ring[turn[0] % a.ring].view(R, 1, V))
            pm = ops.masked_softmax(mix.view(R, 1, -1))
            d1 = pm[:, :, 0:1] * gen
            ptr = torch.cat([pm[:, :, k + 1:k + 2] * c.unsqueeze(1) for k, c in enumerate(copies)], dim=-1)
            dist = ops.copy_scatter(rows, ptr, V, base=d1)
            return ops.nll_rows(dist, targets)

        variants = {"K29": k29, "chain": chain}
        with torch.no_grad():
            p, _ = k29()
            nll = chain()
            scored = targets.ne(0)
            gap = float(((-torch.log(p + 1e-8) - nll).abs() * scored).max())
            for fn in variants.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            samples = {n: [] for n in variants}
            for _ in range(a.repeats):
                for n, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.kernel_iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    samples[n].append(e0.elapsed_time(e1) * 1e3 / a.kernel_iters)
        row_bytes = R * V * 4
        moved = {"K29": row_bytes, "chain": 6 * row_bytes}
        out = {"rows": R, "vocab": V, "source_keys": S, "rows_per_source": rps, "iters": a.kernel_iters, "repeats": a.repeats, "ring": a.ring,
               "max_abs_nll_gap_K29_vs_chain": float("%.3e" % gap), "bytes_moved": moved, "us_per_call": {}, "hbm_fraction_of_8TBs": {}}
        for n, v in samples.items():
            med = statistics.median(v)
            out["us_per_call"][n] = {"median": round(med, 1), "min": round(min(v), 1), "max": round(max(v), 1)}
            out["hbm_fraction_of_8TBs"][n] = round(moved[n] / (med * 1e-6) / HBM_PEAK, 3)
        out["chain_over_K29"] = round(out["us_per_call"]["chain"]["median"] / out["us_per_call"]["K29"]["median"], 2)
        return out

    def passes():
        from case_rg_amd.CaSE.Model import CaSE
        from case_rg_amd.common.CumulativeTrainer import init_params
        from case_rg_amd.common.Utils import init_seed
        from case_rg_amd.utils import make_vocab, synth_batch
        case_rg_amd.set_compute_dtype(torch.bfloat16)
        init_seed(123456)
        v2i, i2v = make_vocab(a.vocab)
        T = a.decode_len
        model = CaSE(4, T, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
        init_params(model)
        model = model.to(dev).eval()
        model.response_generation.decoder.eos_check_every = 1 << 30
        batch = synth_batch(a.batch, a.passages, a.passage_len, a.query_len, 40, a.vocab, seed=123456, ragged=False)
        batch = {k: v.to(dev) for k, v in batch.items()}
        g = torch.Generator(device="cuda").manual_seed(5)
        answers = {n: torch.randint(4, a.vocab, (a.batch, n, T), device=dev, generator=g) for n in (1, 4)}
        runs = {"greedy": lambda: model(dict(batch), method="test"),
                "score_N1": lambda: model.do_score(dict(batch), answers[1]),
                "score_N4": lambda: model.do_score(dict(batch), answers[4])}
        times = {n: [] for n in runs}
        with torch.no_grad():
            for fn in runs.values():
                for _ in range(a.warmup):
                    fn()
            torch.cuda.synchronize()
            for _ in range(a.steps):
                for n, fn in runs.items():
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[n].append(time.perf_counter() - t0)
            peak = {}
            for label, mode in (("fused", "auto"), ("unfused", "off")):
                old, ops.POINTER_SCORE = ops.POINTER_SCORE, mode
                try:
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    model.do_score(dict(batch), answers[1])
                    torch.cuda.synchronize()
                    peak[label] = {"max_memory_allocated_MB": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
                                   "allocated_before_MB": round(base / 2 ** 20, 1)}
                finally:
                    ops.POINTER_SCORE = old
        points = [{"pass": n, "batch": a.batch, "decode_len": T, "ms_per_pass": round(statistics.median(v) * 1e3, 2),
                   "ms_per_pass_min_max": [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]} for n, v in times.items()]
        chunk = model.response_generation.decoder.score_chunk_rows
        return {"points": points, "peak_memory_score_N1": peak, "head_rows": a.batch * T, "score_chunk_rows": chunk,
                "logits_chunk_MB": round(min(chunk, a.batch * T) * a.vocab * 4 / 2 ** 20, 1),
                "full_distribution_MB": round(a.batch * T * a.vocab * 4 / 2 ** 20, 1)}

    res = {"what": "teacher-forced scoring: K29 vs the unfused head chain; do_score passes vs the greedy pass, CaSE, cfg 4 decode geometry, bf16, eager",
           "config": {"batch": a.batch, "decode_len": a.decode_len, "hidden": a.hidden, "enc_layers": a.enc_layers, "passages": a.passages,
                      "passage_len": a.passage_len, "query_len": a.query_len, "vocab": a.vocab, "timed_passes": a.steps, "warmup": a.warmup},
           "device": torch.cuda.get_device_name(0), "kernel": kernel()}
    print(json.dumps(res["kernel"]))
    if not a.skip_passes:
        res["passes"] = passes()
        print(json.dumps(res["passes"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
