#!/usr/bin/env python
"""Sampled decoding next to greedy decoding at the cfg 4 decode geometry (bench.py --mode decode: d_model 512, 3 encoder layers, ten 384-token
passages, 64-token answers, vocabulary 30 522, bf16), and K28 alone next to K23 alone.

    python tools/sample_bench.py [--out profiles/sample_bench.json]

Kernels ("kernels" in the json): 256 rows x V 30 522, S = 64 + 3840 source keys, no gen / dist write-back (what a decoding step asks for).
Each variant -- K23, K28 with the filters off, with top-k, with top-p, with temperature + top-k + top-p, and K28's ``dist_in`` mode -- is timed
with device events around --kernel-iters back-to-back launches, --repeats times, the variants ALTERNATING inside a repeat; reported are the
median and the spread (min, max) in us per launch, and the K28 : K23 ratios of the medians.
Passes ("points"): a greedy pass and sampled passes (filters off; 0.7 / 50 / 0.9) on 256 rows per step, alternating, --steps passes each
after --warmup; ms of one cached step = (T-step pass - 1-step pass) / (T - 1) as bench.py's phase split takes it.  The per-step difference
sampled - greedy is set against the K28 - K23 difference of the kernels: a sampled step launches K28 where the greedy step launches K23 and is
otherwise the same launches, so the two differences should agree.
The event windows hold the wrappers' host work too (20 - 40 us per call is near the launch floor), so they bound a kernel's time from above.
Kernel time proper is the profiler's: run the variants one after the other under a kernel trace, then read the trace back into the json --

    rocprofv3 --kernel-trace -d <dir> --output-format csv -- python tools/sample_bench.py --trace-order
    python tools/sample_bench.py --read-trace <dir> [--out profiles/sample_bench.json]      # no GPU needed

("kernel_trace" in the json: median, min, max of the last --kernel-iters dispatches of each variant, us, and the ratios to K23).
Stand-alone: bench.py does not call this.
"""
import argparse
import csv
import glob
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
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--decode-len", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--enc-layers", type=int, default=3)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-passes", action="store_true")
    ap.add_argument("--trace-order", action="store_true", help="launch the kernel variants one after the other (for a kernel trace); time nothing")
    ap.add_argument("--read-trace", default=None, help="directory of a kernel trace of a --trace-order run: add its kernel times to --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    return ap.parse_args()


VARIANTS = ("K23_ids_only", "K28_filters_off", "K28_top_k50", "K28_top_p09", "K28_t07_k50_p09", "K28_t07", "K28_dist_in_filters_off")
TRACE_WARM = 10


def read_trace(a):
    """The head kernels' dispatches of a --trace-order run, in start order: one K23 launch that makes the ``dist_in`` row, then TRACE_WARM +
    --kernel-iters launches per variant in VARIANTS' order."""
    rows = []
    for path in glob.glob(os.path.join(a.read_trace, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for r in csv.DictReader(fh):
                if "pointer_head_decode_kernel" in r["Kernel_Name"] or "pointer_head_sample_kernel" in r["Kernel_Name"]:
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    per = TRACE_WARM + a.kernel_iters
    if len(rows) != 1 + per * len(VARIANTS):
        raise SystemExit("expected %d head-kernel dispatches in the trace, found %d" % (1 + per * len(VARIANTS), len(rows)))
    out = {}
    for i, n in enumerate(VARIANTS):
        block = rows[1 + i * per + TRACE_WARM:1 + (i + 1) * per]
        assert all(("sample" in name) == n.startswith("K28") for _, _, name in block), n
        us = [(e - s) * 1e-3 for s, e, _ in block]
        out[n] = {"median": round(statistics.median(us), 2), "min": round(min(us), 2), "max": round(max(us), 2)}
    base = out["K23_ids_only"]["median"]
    res = {"what": "kernel durations from a kernel trace, us; the last %d of %d consecutive dispatches per variant" % (a.kernel_iters, per),
           "us_per_dispatch": out, "ratio_to_K23": {n: round(v["median"] / base, 3) for n, v in out.items() if n != "K23_ids_only"},
           "us_over_K23": {n: round(v["median"] - base, 2) for n, v in out.items() if n != "K23_ids_only"}}
    print(json.dumps(res))
    doc = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            doc = json.load(fh)
    doc["kernel_trace"] = res
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


def main():
    a = parse()
    if a.read_trace:
        return read_trace(a)
    if not torch.cuda.is_available():
        raise SystemExit("tools/sample_bench.py measures on the GPU; there is none here")
    import case_rg_amd
    from case_rg_amd import ops
    dev = torch.device("cuda")

    def kernels():
        R, V = a.rows, a.vocab
        lens = [a.query_len, a.passages * a.passage_len]
        g = torch.Generator(device="cuda").manual_seed(3)
        logits = torch.randn(R, V, device=dev, generator=g) * 2.0
        mix = torch.randn(R, 1 + len(lens), device=dev, generator=g)
        src = ops.SortedSource(torch.randint(4, V, (R, sum(lens)), device=dev, generator=g), V)
        copies = [torch.softmax(torch.randn(R, n, device=dev, generator=g) * 2.0, dim=-1) for n in lens]
        dist = ops.pointer_head_decode(logits, mix, src, copies)[1]
        ended = torch.zeros(R, dtype=torch.uint8, device=dev)

        def k28(tau, k, p, dist_in=None):
            if dist_in is None:
                return lambda: ops.pointer_head_sample(logits, mix, src, copies, ended, False, False, -1, -1, 0, tau, k, p, rng=(1, 0, None))
            return lambda: ops.pointer_head_sample(None, None, None, None, ended, False, False, -1, -1, 0, tau, k, p, rng=(1, 0, None), dist_in=dist_in)

        variants = {"K23_ids_only": lambda: ops.pointer_head_decode(logits, mix, src, copies, want_gen=False, want_dist=False),
                    "K28_filters_off": k28(1.0, 0, 1.0), "K28_top_k50": k28(1.0, 50, 1.0), "K28_top_p09": k28(1.0, 0, 0.9),
                    "K28_t07_k50_p09": k28(0.7, 50, 0.9), "K28_t07": k28(0.7, 0, 1.0), "K28_dist_in_filters_off": k28(1.0, 0, 1.0, dist)}
        assert tuple(variants) == VARIANTS
        if a.trace_order:
            torch.cuda.synchronize()
            for fn in variants.values():
                for _ in range(TRACE_WARM + a.kernel_iters):
                    fn()
                torch.cuda.synchronize()
            return None
        for fn in variants.values():
            for _ in range(10):
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
        out = {"rows": R, "vocab": V, "source_keys": sum(lens), "iters": a.kernel_iters, "repeats": a.repeats,
               "us_per_launch": {n: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for n, v in samples.items()}}
        base = out["us_per_launch"]["K23_ids_only"]["median"]
        out["ratio_to_K23"] = {n: round(v["median"] / base, 3) for n, v in out["us_per_launch"].items() if n != "K23_ids_only"}
        out["us_over_K23"] = {n: round(v["median"] - base, 2) for n, v in out["us_per_launch"].items() if n != "K23_ids_only"}
        return out

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
        model.response_generation.decoder.eos_check_every = 1 << 30  # every pass runs its full length: no look at the device, no early end
        batch = synth_batch(a.rows, a.passages, a.passage_len, a.query_len, 40, a.vocab, seed=123456, ragged=False)
        batch = {k: v.to(dev) for k, v in batch.items()}
        runs = {"greedy": lambda: model(dict(batch), method="test"),
                "sample_filters_off": lambda: model.do_sample(dict(batch), seed=1),
                "sample_t07_k50_p09": lambda: model.do_sample(dict(batch), temperature=0.7, top_k=50, top_p=0.9, seed=1)}
        T = a.decode_len
        times = {n: {T: [], 1: []} for n in runs}
        with torch.no_grad():
            for length in (T, 1):
                model.max_target_length = length
                for fn in runs.values():
                    for _ in range(a.warmup):
                        fn()
                torch.cuda.synchronize()
                for _ in range(a.steps):
                    for n, fn in runs.items():
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[n][length].append(time.perf_counter() - t0)
        model.max_target_length = T
        points = []
        for n in runs:
            full, one = statistics.median(times[n][T]), statistics.median(times[n][1])
            points.append({"decoder": n, "rows": a.rows, "ms_per_pass": round(full * 1e3, 2), "ms_per_pass_min_max": [round(min(times[n][T]) * 1e3, 2), round(max(times[n][T]) * 1e3, 2)],
                           "ms_one_step_pass": round(one * 1e3, 2), "ms_per_cached_step": round((full - one) / (T - 1) * 1e3, 4)})
        for p in points[1:]:
            p["us_per_step_over_greedy"] = round((p["ms_per_cached_step"] - points[0]["ms_per_cached_step"]) * 1e3, 1)
        return points

    if a.trace_order:
        kernels()
        return 0
    res = {"what": "sampled vs greedy decoding, CaSE, cfg 4 decode geometry, bf16, eager launches; K28 vs K23 alone",
           "config": {"rows_per_step": a.rows, "decode_len": a.decode_len, "hidden": a.hidden, "enc_layers": a.enc_layers, "passages": a.passages,
                      "passage_len": a.passage_len, "query_len": a.query_len, "vocab": a.vocab, "timed_passes": a.steps, "warmup": a.warmup},
           "device": torch.cuda.get_device_name(0), "kernels": kernels()}
    print(json.dumps(res["kernels"]))
    if not a.skip_passes:
        res["points"] = passes()
        for p in res["points"]:
            print(json.dumps(p))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
