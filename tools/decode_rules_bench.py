#!/usr/bin/env python
"""The decoding rules (min_length, banned ids, the beam length penalty) next to the launches they extend.

    python tools/decode_rules_bench.py [--parent-lib other/libcase_hip.so] [--out profiles/decode_rules_bench.json]

Kernels ("kernels" in the json): 256 rows x V 30 522, S = 64 + 3840 source keys, step t = 3 of min_length 5, no gen / dist write-back.  K23,
K24 (W 4) and K28 (filters off), each in the LDS and in the global-row form, with the rules off and with min_length + a list of 3 ids, a
list of 256 ids for every item, and one list of 256 ids per item (4 rows per item); K25 on the flat history with the division and with
alpha = 0.6 (64 items x W 4); ``row_rules_`` alone.  Each variant is timed with device events around --kernel-iters back-to-back launches,
--repeats times, the variants ALTERNATING inside a repeat; reported are the median and the spread (min, max) in us per launch.  The event
windows hold the wrappers' host work too, so they bound a kernel's time from above.

A/B against another build of the library ("ab_rules_off"): with --parent-lib the rule-off launches of K23 / K24 / K28 (LDS and wide) and K25
(plain and flat history) go through BOTH libraries in this process by raw C-ABI calls on the same operands, alternating A / B inside every
repeat: both medians, both spreads, the difference of the medians, and whether each median lies inside the other build's min-max range.
Stand-alone: bench.py does not call this.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--decode-len", type=int, default=64)
    ap.add_argument("--passages", type=int, default=10)
    ap.add_argument("--passage-len", type=int, default=384)
    ap.add_argument("--query-len", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=30522)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--parent-lib", default=None, help="another build of libcase_hip.so (the parent commit's): A/B of the rule-off launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_rules_bench.json"))
    return ap.parse_args()


def _stats(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


def _time(variants, iters, repeats):
    for fn in variants.values():
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    samples = {n: [] for n in variants}
    for _ in range(repeats):
        for n, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            samples[n].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {n: _stats(v) for n, v in samples.items()}


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("tools/decode_rules_bench.py measures on the GPU; there is none here")
    from case_rg_amd import _abi, ops
    dev = torch.device("cuda")
    R, V, T, t, W, M = a.rows, a.vocab, a.decode_len, 3, 4, 5
    lens = [a.query_len, a.passages * a.passage_len]
    g = torch.Generator(device="cuda").manual_seed(3)
    logits = torch.randn(R, V, device=dev, generator=g) * 2.0
    mix = torch.randn(R, 1 + len(lens), device=dev, generator=g)
    src = ops.SortedSource(torch.randint(4, V, (R, sum(lens)), device=dev, generator=g), V)
    copies = [torch.softmax(torch.randn(R, n, device=dev, generator=g) * 2.0, dim=-1) for n in lens]
    ended = torch.zeros(R, dtype=torch.uint8, device=dev)
    Bb = R // W
    cand_p = torch.rand(R, W, device=dev, generator=g).sort(dim=1, descending=True)[0].contiguous()
    cand_id = torch.randint(4, V, (R, W), device=dev, generator=g)
    eos = 2
    rules = {"rules_off": None,
             "min_length_3_ids": ops.row_rules(eos, M, torch.tensor([100, 101, 102], dtype=torch.int32, device=dev), t=t),
             "256_ids": ops.row_rules(eos, M, torch.randint(4, V, (256,), device=dev, generator=g).to(torch.int32), t=t),
             "256_ids_per_item": ops.row_rules(eos, M, torch.randint(4, V, (Bb, 256), device=dev, generator=g).to(torch.int32), W, t=t)}

    def k23(r, row):
        return lambda: ops.pointer_head_decode(logits, mix, src, copies, want_gen=False, want_dist=False, rules=r, row=row)

    def k24(r, row):
        return lambda: ops.pointer_head_topk(logits, mix, src, copies, W, rules=r, row=row)

    def k28(r, row):
        return lambda: ops.pointer_head_sample(logits, mix, src, copies, ended, False, False, -1, -1, 0, 1.0, 0, 1.0, rng=(1, 0, None), rules=r, row=row)

    def k25(alpha):
        state = ops.BeamState(Bb, W, T, dev, flat=True)

        def run():  # a step in the middle of a pass: nothing retires (eos -1), the state keeps W live slots
            state.alive.fill_(1)
            ops.beam_advance(state, cand_p, cand_id, T - 2, None, length_penalty=alpha)
        return run

    dist = torch.rand(R, V, device=dev, generator=g)
    variants = {}
    for name, make in (("K23", k23), ("K24_w4", k24), ("K28_filters_off", k28)):
        for row in ("lds", "global"):
            for tag, r in rules.items():
                variants["%s_%s_%s" % (name, row, tag)] = make(r, row)
    variants.update({"K25_flat_division": k25(1.0), "K25_flat_alpha_0.6": k25(0.6),
                     "row_rules_256_ids_per_item": lambda: ops.row_rules_(dist, rules["256_ids_per_item"])})
    kernels = {"rows": R, "vocab": V, "source_keys": sum(lens), "t": t, "min_length": M, "iters": a.kernel_iters, "repeats": a.repeats,
               "us_per_launch": _time(variants, a.kernel_iters, a.repeats)}
    u = kernels["us_per_launch"]
    kernels["us_over_rules_off"] = {k: round(v["median"] - u[k[:k.index(row) + len(row)] + "_rules_off"]["median"], 2)
                                    for k, v in u.items() for row in ("lds", "global") if "_%s_" % row in k and not k.endswith("rules_off")}
    kernels["us_alpha_over_division"] = round(u["K25_flat_alpha_0.6"]["median"] - u["K25_flat_division"]["median"], 2)
    res = {"what": "decoding rules (min_length, banned ids, beam length penalty); eager launches, device events",
           "device": torch.cuda.get_device_name(0), "kernels": kernels}
    print(json.dumps(kernels))

    if a.parent_lib:
        other = C.CDLL(os.path.abspath(a.parent_lib))
        names = ("case_pointer_head_decode", "case_pointer_head_beam", "case_pointer_head_sample", "case_pointer_head_decode_wide",
                 "case_pointer_head_beam_wide", "case_pointer_head_sample_wide", "case_beam_advance", "case_beam_advance_ban")
        for lib in (other, _abi.lib):
            for name in names:
                getattr(lib, name).argtypes, getattr(lib, name).restype = _abi.SIGNATURES[name], C.c_int
        lg, mx, cs, ptrs, ln, nm, S = ops._head_operands(logits, mix, src, copies)
        ids = torch.empty(R, dtype=torch.int64, device=dev)
        prob = torch.empty(R, dtype=torch.float32, device=dev)
        cp, ci = torch.empty(R, W, device=dev), torch.empty(R, W, dtype=torch.int64, device=dev)
        ws, stride = ops._row_workspace(R, V, dev)
        st, stf = ops.BeamState(Bb, W, T, dev), ops.BeamState(Bb, W, T, dev, flat=True)
        p, stream = ops._ptr, ops._stream
        head = (p(lg), p(mx), p(src.keys), ptrs, ln, nm)
        no_ban = (None, 0, 0, 0)

        def raw(lib):
            def adv(s, flat):
                def run():
                    s.alive.fill_(1)
                    args = (p(cand_p), p(cand_id), p(s.alive), p(s.cum), p(s.len), p(s.parent), p(s.token), p(s.hist_parent), p(s.hist_token),
                            p(s.fin_key), p(s.fin_step), p(s.fin_slot), T - 2, T, Bb, W, -1)
                    if flat:
                        return lib.case_beam_advance_ban(*args, p(s.flat[0]), p(s.flat[1]), T, stream())
                    return lib.case_beam_advance(*args, stream())
                return run
            draw = (p(ids), p(prob), p(ended), None, R, V, S, 1.0, 0, 1.0, 1, 0, None, -1, -1, 0, 0, 0)
            return {"K23_lds": lambda: lib.case_pointer_head_decode(*head, None, None, p(ids), None, R, V, S, stream()),
                    "K24_w4_lds": lambda: lib.case_pointer_head_beam(*head, None, None, p(cp), p(ci), R, V, S, W, stream()),
                    "K28_filters_off_lds": lambda: lib.case_pointer_head_sample(*head, None, None, None, *draw, stream()),
                    "K23_global": lambda: lib.case_pointer_head_decode_wide(*head, None, None, p(ids), None, R, V, S, p(ws), stride, *no_ban, -1, stream()),
                    "K24_w4_global": lambda: lib.case_pointer_head_beam_wide(*head, None, None, p(cp), p(ci), R, V, S, W, p(ws), stride, *no_ban, -1,
                                                                             stream()),
                    "K28_filters_off_global": lambda: lib.case_pointer_head_sample_wide(*head, None, None, None, *draw, p(ws), stride, *no_ban, stream()),
                    "K25_plain": adv(st, False), "K25_flat": adv(stf, True)}
        keys = list(raw(_abi.lib))
        ab = {}
        for k in keys:
            ab["A_parent/" + k] = raw(other)[k]
            ab["B_this/" + k] = raw(_abi.lib)[k]
        for fn in ab.values():
            assert fn() in (0, None)
        timed = _time(ab, a.kernel_iters, a.repeats)

        def inside(x, rng):
            return rng["min"] <= x["median"] <= rng["max"]

        res["ab_rules_off"] = {"what": "the rule-off launches through the parent build (A) and this build (B), raw C-ABI calls on the same operands, alternating; us per launch",
                               "parent_lib": os.path.basename(a.parent_lib), "us_per_launch": timed,
                               "B_minus_A_us": {k: round(timed["B_this/" + k]["median"] - timed["A_parent/" + k]["median"], 2) for k in keys},
                               "medians_inside_each_others_range": {k: inside(timed["B_this/" + k], timed["A_parent/" + k])
                                                                    and inside(timed["A_parent/" + k], timed["B_this/" + k]) for k in keys}}
        print(json.dumps(res["ab_rules_off"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
