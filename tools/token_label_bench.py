#!/usr/bin/env python
"""The supporting-token stage: K37 next to the host form of its rule, K38 next to ``torch.topk``, the extract-only pass next to the rank-only
and the greedy pass, and a training step that labels its batch on the device next to one that is handed the labels.

    python tools/token_label_bench.py [--out profiles/token_label_bench.json]

Kernels ("labels", "select" in the json), timed ALTERNATELY (one window of --kernel-iters calls of each in turn, --repeats rounds; median, min
and max of the rounds, microseconds per call, device events; the windows hold the wrappers' host work too -- output allocations, the ctypes
call -- so they bound a kernel's time from above):
  labels   --batch x --passages x --passage-len ids, answers of --answer-len ids, half of them copied from the passages:
           k37           ops.token_labels
           host_form     common.Utils.token_label on the same device tensors (vectorised torch, f64)
           python_rule   the per-token rule as the reference writes it (list membership, two set intersections per token), the host clock
                         over --host-rows rows, scaled to all rows: context, not a competitor
  select   --select-items x (--passages x --passage-len) keys, K 32, a tenth of the positions invalid:
           k38           ops.token_select          k38_counts   ... with labels: the five counts from the same pass
           topk          torch.topk(values.masked_fill(~valid, -inf), 32): no tie rule, no counts, no -1 slots
Passes ("passes"): CaSE, bf16, --pass-batch items, ``do_extract`` next to ``do_rank`` and ``do_test`` (--decode-len cached steps), eager,
alternating, the host clock around a pass that ends in a device synchronise; medians of --steps passes.
Step ("step"): the training step of bench.py's default line (cfg 2: batch 32, hidden 512, 6 encoder layers, bf16, dropout on), eager, with
``token_label`` / ``token_weight`` in the batch next to the same trainer on the batch without them (K37 inside the step), alternating.
Stand-alone: bench.py does not call this.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--answer-len", type=int, default=80)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--select-items", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--pass-batch", type=int, default=64)
    ap.add_argument("--decode-len", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--enc-layers", type=int, default=3)
    ap.add_argument("--step-enc-layers", type=int, default=6)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-passes", action="store_true")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "token_label_bench.json"))
    return ap.parse_args()


def python_rule(row, answer, freq):
    """One passage row by the reference's words: membership tests on a list, a ``set`` intersection per window."""
    L = len(row)
    f = [math.log(freq.get(t, 0) + 2) for t in row]
    g1 = [t in answer for t in row]
    pad3, pad5 = [0] + row + [0], [0, 0] + row + [0, 0]
    g3 = [len(set(pad3[i:i + 3]).intersection(answer)) for i in range(L)]
    g5 = [len(set(pad5[i:i + 5]).intersection(answer)) for i in range(L)]
    s = sum(f)
    return [float(g) for g in g1], [(s / f[i] * g3[i] * g5[i]) ** 0.2 if g1[i] else 1.0 for i in range(L)]


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/token_label_bench.py measures on the GPU; there is none here")
    import case_rg_amd
    from case_rg_amd import ops
    from case_rg_amd.common.Utils import token_label
    dev = torch.device("cuda")

    def timed(variants):
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
                for _ in range(a.kernel_iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                out[n].append(e0.elapsed_time(e1) * 1e3 / a.kernel_iters)
        return {n: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for n, v in out.items()}

    def labels():
        g = torch.Generator().manual_seed(7)
        B, P, L, T = a.batch, a.passages, a.passage_len, a.answer_len
        x = torch.randint(4, a.vocab, (B, P, L), generator=g)
        x[:, :, L - L // 8:] = 0  # the tail of every row is PAD
        y = torch.randint(4, a.vocab, (B, T), generator=g)
        y[:, ::2] = x.reshape(B, -1)[:, torch.randint(0, P * (L - L // 8), (T - T // 2,), generator=g)]
        freq = torch.randint(0, 2 * 10 ** 6, (a.vocab,), generator=g)
        dx, dy, df = x.to(dev), y.to(dev), freq.to(dev)
        us = timed({"k37": lambda: ops.token_labels(dx, dy, df), "host_form": lambda: token_label(dx, dy, df)})
        got, want = ops.token_labels(dx, dy, df), token_label(dx, dy, df)
        table = dict(enumerate(freq.tolist()))
        n = min(a.host_rows, P)
        rows, answer = x[0, :n].tolist(), [t for t in y[0].tolist() if t]  # (the reference is handed the answer without padding)
        t0 = time.perf_counter()
        slow = [python_rule(row, answer, table) for row in rows]
        rule_s = (time.perf_counter() - t0) * B * P / n
        same = all(got[0][0, p].tolist() == slow[p][0] for p in range(n))
        return {"shape": [B, P, L], "answer_len": T, "members": int(got[0].sum()), "us_per_call": us,
                "host_form_over_k37": round(us["host_form"]["median"] / us["k37"]["median"], 1),
                "python_rule_ms_scaled_to_all_rows": round(rule_s * 1e3, 1), "python_rows_timed": n,
                "python_rule_over_k37": round(rule_s * 1e6 / us["k37"]["median"], 0), "labels_equal_host_form": bool(torch.equal(got[0], want[0])),
                "labels_equal_python_rule_on_the_timed_rows": same,
                "max_rel_weight_diff_to_host_form": float(((got[1].double() - want[1].double()).abs() / want[1].double()).max())}

    def select():
        points = []
        g = torch.Generator().manual_seed(8)
        S, K = a.passages * a.passage_len, 32
        for B in a.select_items:
            values = torch.rand(B, S, generator=g).to(dev)
            valid = (torch.rand(B, S, generator=g) < 0.9).to(dev)
            scores = torch.randn(B, S, generator=g).to(dev)
            gold = (torch.rand(B, S, generator=g) < 0.1).float().to(dev)
            us = timed({"k38": lambda: ops.token_select(values, valid, K),
                        "k38_counts": lambda: ops.token_select(values, valid, K, scores=scores, labels=gold),
                        "topk": lambda: torch.topk(values.masked_fill(~valid, -math.inf), K, dim=1)})
            same = bool(torch.equal(ops.token_select(values, valid, K)["pos"].long(), torch.topk(values.masked_fill(~valid, -math.inf), K, dim=1).indices))
            points.append({"items": B, "positions": S, "k": K, "us_per_call": us, "topk_over_k38": round(us["topk"]["median"] / us["k38"]["median"], 2),
                           "positions_equal_topk": same})
        return {"points": points}

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
            runs = {"rank": lambda: model.do_rank(dict(batch)), "extract": lambda: model.do_extract(dict(batch)),
                    "extract_and_counts": lambda: model.do_extract(dict(batch), labels=batch["token_label"]),
                    "test": lambda: model.do_test(dict(batch))}
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
            same = bool(torch.equal(runs["rank"]()["rank"], runs["extract"]()["rank"]))
        med = {n: statistics.median(v) * 1e3 for n, v in times.items()}
        return {"batch": a.pass_batch, "decode_len": a.decode_len, "do_rank_ms": round(med["rank"], 2), "do_extract_ms": round(med["extract"], 2),
                "do_extract_with_counts_ms": round(med["extract_and_counts"], 2), "do_test_ms": round(med["test"], 2),
                "extract_over_rank": round(med["extract"] / med["rank"], 2), "test_over_extract": round(med["test"] / med["extract"], 1),
                "rank_equal_bits": same, "ms_min_max": {n: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for n, v in times.items()}}

    def step():
        from case_rg_amd.CaSE.Model import CaSE
        from case_rg_amd.common.CumulativeTrainer import CumulativeTrainer, init_params
        from case_rg_amd.common.Utils import init_seed
        from case_rg_amd.optim import FusedAdam
        from case_rg_amd.utils import make_vocab, synth_batch
        case_rg_amd.set_compute_dtype(torch.bfloat16)
        case_rg_amd.set_dropout(True)
        init_seed(123456)
        v2i, i2v = make_vocab(a.vocab)
        model = CaSE(4, 40, i2v, v2i, a.hidden, enc_layers=a.step_enc_layers)
        init_params(model)
        trainer = CumulativeTrainer(model, None, None, 0, 1, capture=False)
        model.set_token_freq(torch.randint(0, 2 * 10 ** 6, (a.vocab,), generator=torch.Generator().manual_seed(9)))
        opt = FusedAdam(model.parameters(), lr=2.5e-4, low_precision=torch.bfloat16)
        batch = synth_batch(a.batch, a.passages, a.passage_len, a.query_len, 40, a.vocab, seed=123456, ragged=False)
        present = {k: v.to(dev) for k, v in batch.items()}
        absent = {k: v for k, v in present.items() if k not in ("token_label", "token_weight")}
        trainer.model.train()
        runs = {"keys_present": present, "keys_absent": absent}
        times = {n: [] for n in runs}
        for _ in range(a.warmup + 1):
            for data in runs.values():
                trainer.train_batch(0, dict(data), "train", opt)
        torch.cuda.synchronize()
        for _ in range(a.steps):
            for n, data in runs.items():
                t0 = time.perf_counter()
                trainer.train_batch(0, dict(data), "train", opt)
                torch.cuda.synchronize()
                times[n].append(time.perf_counter() - t0)
        trainer.close()
        case_rg_amd.set_dropout(False)
        med = {n: statistics.median(v) * 1e3 for n, v in times.items()}
        return {"batch": a.batch, "enc_layers": a.step_enc_layers, "step_ms_keys_present": round(med["keys_present"], 2),
                "step_ms_keys_absent": round(med["keys_absent"], 2), "absent_minus_present_ms": round(med["keys_absent"] - med["keys_present"], 3),
                "ms_min_max": {n: [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)] for n, v in times.items()}}

    res = {"what": "supporting tokens: K37 vs the host form, K38 vs torch.topk, do_extract vs do_rank / do_test, a step that labels its batch",
           "config": {"hidden": a.hidden, "passages": a.passages, "passage_len": a.passage_len, "query_len": a.query_len, "vocab": a.vocab,
                      "kernel_iters": a.kernel_iters, "repeats": a.repeats, "timed_passes": a.steps, "warmup": a.warmup},
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name, part, skip in (("labels", labels, False), ("select", select, False), ("passes", passes, a.skip_passes), ("step", step, a.skip_step)):
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
