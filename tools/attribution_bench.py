#!/usr/bin/env python
"""Answer attribution: K39 next to K29 on the same operands, and ``do_attribute`` passes next to the passes they extend.

    python tools/attribution_bench.py [--out profiles/attribution_bench.json]

Kernel ("kernel" in the json), timed ALTERNATELY (one window of --kernel-iters calls of each in turn, --repeats rounds; median, min and max
of the rounds, microseconds per call, device events; the windows hold the wrappers' host work too -- output allocations, the float copies of
the operands, the ctypes call -- so they bound a kernel's time from above):
  --rows rows, V --vocab, S = --query-len + --passages x --passage-len, G = 1 + --passages segments, two memories, source ids drawn so
  that a target's run holds about --run positions:
           k29         ops.pointer_head_score: reads the logits row [V] of every row
           k39         ops.copy_attribution: no logits; 1 + nmem floats, two searches of the key row and the run
           host_form   evaluation.attribution.copy_attribution_host on the same device tensors (vectorised torch, f64, an [R, S] pass)
Passes ("passes"): CaSE, bf16, --pass-batch items, --passages x --passage-len, eager, alternating, the host clock around a pass that ends
in a device synchronise; medians of --steps passes:
           do_test                          --decode-len cached steps
           do_attribute(answers="test")     the same decode, then the teacher-forced pass with K39 behind K29
           do_score                         the teacher-forced pass over data['response']
           do_attribute(answers="response") the same pass with K39 behind K29 and the shares
Stand-alone: bench.py does not call this.
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


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--rows-per-source", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--run", type=int, default=6)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pass-batch", type=int, default=64)
    ap.add_argument("--decode-len", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--enc-layers", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-passes", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attribution_bench.json"))
    return ap.parse_args()


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/attribution_bench.py measures on the GPU; there is none here")
    import case_rg_amd
    from case_rg_amd import ops
    from case_rg_amd.evaluation.attribution import copy_attribution_host, source_segments
    dev = torch.device("cuda")

    def timed(variants, iters):
        """{name: fn} -> {name: {median, min, max}} in microseconds per call; the variants take turns inside every round."""
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        out = {n: [] for n in variants}
        for _ in range(a.repeats):
            for n, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters[n]):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out[n].append(e0.elapsed_time(e1) * 1e3 / iters[n])
        return {n: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in out.items()}

    def kernel():
        g = torch.Generator().manual_seed(7)
        R, V, rps = a.rows, a.vocab, a.rows_per_source
        S = a.query_len + a.passages * a.passage_len
        seg = source_segments(a.query_len, a.passages, a.passage_len)
        K = R // rps
        src = torch.randint(5, 5 + max(2, S // a.run), (K, S), generator=g)
        lens = [a.query_len, S - a.query_len]
        logits = (torch.randn(R, V, generator=g) * 2.0).to(dev)
        mix = torch.randn(R, 3, generator=g).to(dev)
        copies = [torch.softmax(torch.randn(R, n, generator=g) * 2.0, dim=-1).to(dev) for n in lens]
        targets = src[torch.arange(R) // rps, torch.randint(0, S, (R,), generator=g)].to(dev)
        sm = ops.SortedSource(src.to(dev), V)
        seg_dev = torch.tensor(seg, dtype=torch.int32, device=dev)
        variants = {"k29": lambda: ops.pointer_head_score(logits, mix, sm, rps, copies, targets, 0),
                    "k39": lambda: ops.copy_attribution(mix, sm, rps, copies, targets, seg, 0),
                    "k39_device_segments": lambda: ops.copy_attribution(mix, sm, rps, copies, targets, seg_dev, 0),
                    "host_form": lambda: copy_attribution_host(mix, sm.ids, copies, targets, seg, 0, V)}
        iters = {n: a.kernel_iters if n != "host_form" else max(1, a.kernel_iters // 20) for n in variants}
        us = timed(variants, iters)
        got, (_, k29) = variants["k39"](), variants["k29"]()
        host = variants["host_form"]()
        total = got["mass"].double().sum(1)
        gap = float(((total - k29.double()).abs() / k29.double().clamp_min(1e-300))[k29 > 0].max())
        host_gap = float(((got["mass"].double() - host["mass"].double()).abs() / host["mass"].double().clamp_min(1e-300))[host["mass"] > 0].max())
        return {"rows": R, "vocab": V, "source_positions": S, "segments": len(seg) - 1, "rows_per_source": rps,
                "mean_run": round(float(got["count"].float().mean()), 2), "us_per_call": us,
                "k29_over_k39": round(us["k29"]["median"] / us["k39"]["median"], 2),
                "host_form_over_k39": round(us["host_form"]["median"] / us["k39"]["median"], 1),
                "bytes_read_k29_logits": R * V * 4, "max_rel_gap_sum_of_masses_vs_k29_copy": float("%.3e" % gap),
                "max_rel_gap_k39_vs_host_form": float("%.3e" % host_gap),
                "pos_and_count_equal_host_form": bool(torch.equal(got["pos"], host["pos"]) and torch.equal(got["count"], host["count"]))}

    def passes():
        from case_rg_amd.CaSE.Model import CaSE
        from case_rg_amd.common.CumulativeTrainer import init_params
        from case_rg_amd.common.Utils import init_seed
        from case_rg_amd.utils import make_vocab, synth_batch
        case_rg_amd.set_compute_dtype(torch.bfloat16)
        init_seed(123456)
        v2i, i2v = make_vocab(a.vocab)
        model = CaSE(4, a.decode_len, i2v, v2i, a.hidden, enc_layers=a.enc_layers)
        init_params(model)
        model = model.to(dev).eval()
        model.response_generation.decoder.eos_check_every = 1 << 30
        batch = synth_batch(a.pass_batch, a.passages, a.passage_len, a.query_len, 40, a.vocab, seed=123456, ragged=False)
        batch = {k: v.to(dev) for k, v in batch.items()}
        with torch.no_grad():
            runs = {"test": lambda: model.do_test(dict(batch)), "attribute_test": lambda: model.do_attribute(dict(batch), answers="test"),
                    "score": lambda: model.do_score(dict(batch)), "attribute_response": lambda: model.do_attribute(dict(batch), answers="response")}
            times = {n: [] for n in runs}
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
            scored, attributed = runs["score"](), runs["attribute_response"]()
            same = all(bool(torch.equal(scored[k], attributed[k])) for k in ("token_probs", "copy_probs", "scores", "loss"))
            shares = attributed["support"][:, 0].mean(0)
        med = {n: statistics.median(v) * 1e3 for n, v in times.items()}
        return {"batch": a.pass_batch, "decode_len": a.decode_len, "response_len": int(batch["response"].shape[1]),
                "do_test_ms": round(med["test"], 2), "do_attribute_test_ms": round(med["attribute_test"], 2),
                "do_score_ms": round(med["score"], 2), "do_attribute_response_ms": round(med["attribute_response"], 2),
                "attribute_test_over_test": round(med["attribute_test"] / med["test"], 3),
                "attribute_response_over_score": round(med["attribute_response"] / med["score"], 3),
                "attribute_response_minus_score_ms": round(med["attribute_response"] - med["score"], 3),
                "score_bits_equal": same, "mean_support_gen_context_passages": [round(float(shares[0]), 4), round(float(shares[1]), 4),
                                                                                round(float(shares[2:].sum()), 4)],
                "ms_min_max": {n: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for n, v in times.items()}}

    res = {"what": "answer attribution: K39 vs K29 on the same operands; do_attribute vs do_test and do_score, CaSE, bf16, eager",
           "config": {"hidden": a.hidden, "passages": a.passages, "passage_len": a.passage_len, "query_len": a.query_len, "vocab": a.vocab,
                      "kernel_iters": a.kernel_iters, "repeats": a.repeats, "timed_passes": a.steps, "warmup": a.warmup},
           "note": "every figure holds the wrapper's host work (allocations, float copies, the ctypes call)",
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name, part, skip in (("kernel", kernel, False), ("passes", passes, a.skip_passes)):
        if skip:
            continue
        res[name] = part()
        print(json.dumps({name: res[name]}), flush=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
