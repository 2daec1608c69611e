#!/usr/bin/env python
"""The n-gram ban (K32), the flat beam history and the device remove_duplicate (K33) next to the launches they extend.

    python tools/ngram_bench.py [--parent-lib other/libcase_hip.so] [--out profiles/ngram_bench.json]

Kernels ("kernels" in the json): 256 rows x V 30 522, S = 64 + 3840 source keys, step t = 63, no gen / dist write-back.  K23, K24 (W 4) and
K28 (filters off) with the ban off and with n = 1 and n = 3 (histories over 50 words, so windows match); K25 with and without the flat
history (64 items x W 4); K33 on 256 rows x T 64 of looping sentences.  Each variant is timed with device events around --kernel-iters
back-to-back launches, --repeats times, the variants ALTERNATING inside a repeat; reported are the median and the spread (min, max) in us per
launch.  The event windows hold the wrappers' host work too, so they bound a kernel's time from above.

A/B against another build of the library ("ab_ban_off"): with --parent-lib the ban-off launches of K23 / K24 / K28 / K25 go through BOTH
libraries in this process by raw C-ABI calls on the same operands, alternating A / B inside every repeat: both medians, both spreads and
the difference of the medians.  The requirement is that the ban-off launch of this build is not slower than the other build's beyond the
run-to-run spread.

Passes ("points"): a whole greedy, beam (W 4) and sampled pass of CaSE at the decode geometry (d_model 512, 3 encoder layers, ten 384-token
passages, 64-token answers, bf16) on --pass-rows items, ban off against n = 3, alternating, --steps passes each after --warmup.
Stand-alone: bench.py does not call this.
"""
import argparse
import ctypes as C
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
    ap.add_argument("--pass-rows", type=int, default=64)
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
    ap.add_argument("--parent-lib", default=None, help="another build of libcase_hip.so (the parent commit's): A/B of the ban-off launches")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ngram_bench.json"))
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
        raise SystemExit("tools/ngram_bench.py measures on the GPU; there is none here")
    import case_rg_amd
    from case_rg_amd import _abi, ops
    dev = torch.device("cuda")
    R, V, T, t, W = a.rows, a.vocab, a.decode_len, a.decode_len - 1, 4
    lens = [a.query_len, a.passages * a.passage_len]
    g = torch.Generator(device="cuda").manual_seed(3)
    logits = torch.randn(R, V, device=dev, generator=g) * 2.0
    mix = torch.randn(R, 1 + len(lens), device=dev, generator=g)
    src = ops.SortedSource(torch.randint(4, V, (R, sum(lens)), device=dev, generator=g), V)
    copies = [torch.softmax(torch.randn(R, n, device=dev, generator=g) * 2.0, dim=-1) for n in lens]
    hist = torch.randint(4, 54, (R, T), device=dev, generator=g).to(torch.int32)
    ended = torch.zeros(R, dtype=torch.uint8, device=dev)
    Bb = R // W
    cand_p = torch.rand(R, W, device=dev, generator=g).sort(dim=1, descending=True)[0].contiguous()
    cand_id = torch.randint(4, V, (R, W), device=dev, generator=g)

    def k23(n):
        return lambda: ops.pointer_head_decode(logits, mix, src, copies, want_gen=False, want_dist=False, ban=(hist, t, n, None) if n else None)

    def k24(n):
        return lambda: ops.pointer_head_topk(logits, mix, src, copies, W, ban=(hist, t, n, None) if n else None)

    def k28(n):
        return lambda: ops.pointer_head_sample(logits, mix, src, copies, ended, False, False, -1, -1, 0, 1.0, 0, 1.0, rng=(1, 0, None),
                                               ban=(hist, t, n) if n else None)

    def k25(flat):
        state = ops.BeamState(Bb, W, T, dev, flat=flat)
        state.alive.fill_(1)

        def run():  # a step in the middle of a pass: nothing retires (eos -1), the state keeps W live slots
            state.alive.fill_(1)
            ops.beam_advance(state, cand_p, cand_id, t - 1, None)
        return run

    loop = (torch.arange(T, device=dev) % 5 + 4).repeat(R, 1).contiguous()
    loop[:, :8] = torch.randint(10, 60, (R, 8), device=dev, generator=g)
    full = torch.full((R,), T, dtype=torch.int32, device=dev)

    def k33():
        ops.remove_duplicate_ids(loop.clone(), full.clone())

    def k33_floor():
        loop.clone(), full.clone()

    variants = {}
    for name, make in (("K23", k23), ("K24_w4", k24), ("K28_filters_off", k28)):
        for n in (0, 1, 3):
            variants["%s_%s" % (name, "ban_off" if n == 0 else "n%d" % n)] = make(n)
    variants.update({"K25_plain": k25(False), "K25_flat_history": k25(True), "K33_256x64_with_two_clones": k33, "two_clones_alone": k33_floor})
    kernels = {"rows": R, "vocab": V, "source_keys": sum(lens), "t": t, "iters": a.kernel_iters, "repeats": a.repeats,
               "us_per_launch": _time(variants, a.kernel_iters, a.repeats)}
    u = kernels["us_per_launch"]
    kernels["us_over_ban_off"] = {k: round(v["median"] - u[k.rsplit("_n", 1)[0] + "_ban_off"]["median"], 2) for k, v in u.items() if k[-2:] in ("n1", "n3")}
    kernels["us_flat_history_over_plain"] = round(u["K25_flat_history"]["median"] - u["K25_plain"]["median"], 2)
    res = {"what": "n-gram ban (K32), flat beam history and device remove_duplicate (K33); eager launches, device events",
           "device": torch.cuda.get_device_name(0), "kernels": kernels}
    print(json.dumps(kernels))

    if a.parent_lib:
        other = C.CDLL(os.path.abspath(a.parent_lib))
        names = ("case_pointer_head_decode", "case_pointer_head_beam", "case_pointer_head_sample", "case_beam_advance")
        for lib in (other, _abi.lib):
            for name in names:
                getattr(lib, name).argtypes, getattr(lib, name).restype = _abi.SIGNATURES[name], C.c_int
        lg, mx, cs, ptrs, ln, nm, S = ops._head_operands(logits, mix, src, copies)
        ids = torch.empty(R, dtype=torch.int64, device=dev)
        prob = torch.empty(R, dtype=torch.float32, device=dev)
        cp, ci = torch.empty(R, W, device=dev), torch.empty(R, W, dtype=torch.int64, device=dev)
        st = ops.BeamState(Bb, W, T, dev)
        p, stream = ops._ptr, ops._stream
        head = (p(lg), p(mx), p(src.keys), ptrs, ln, nm)

        def raw(lib):
            def adv():
                st.alive.fill_(1)
                lib.case_beam_advance(p(cand_p), p(cand_id), p(st.alive), p(st.cum), p(st.len), p(st.parent), p(st.token), p(st.hist_parent),
                                      p(st.hist_token), p(st.fin_key), p(st.fin_step), p(st.fin_slot), t - 1, T, Bb, W, -1, stream())
            return {"K23": lambda: lib.case_pointer_head_decode(*head, None, None, p(ids), None, R, V, S, stream()),
                    "K24_w4": lambda: lib.case_pointer_head_beam(*head, None, None, p(cp), p(ci), R, V, S, W, stream()),
                    "K28_filters_off": lambda: lib.case_pointer_head_sample(*head, None, None, None, p(ids), p(prob), p(ended), None, R, V, S, 1.0, 0, 1.0,
                                                                            1, 0, None, -1, -1, 0, 0, 0, stream()),
                    "K25": adv}
        ab = {}
        for k in ("K23", "K24_w4", "K28_filters_off", "K25"):
            ab["A_parent/" + k] = raw(other)[k]
            ab["B_this/" + k] = raw(_abi.lib)[k]
        for fn in ab.values():
            assert fn() in (0, None)
        timed = _time(ab, a.kernel_iters, a.repeats)
        res["ab_ban_off"] = {"what": "the ban-off launches through the parent build (A) and this build (B), raw C-ABI calls on the same operands, alternating; us per launch",
                             "parent_lib": os.path.basename(a.parent_lib), "us_per_launch": timed,
                             "B_minus_A_us": {k: round(timed["B_this/" + k]["median"] - timed["A_parent/" + k]["median"], 2)
                                              for k in ("K23", "K24_w4", "K28_filters_off", "K25")}}
        print(json.dumps(res["ab_ban_off"]))

    if not a.skip_passes:
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
        model.response_generation.decoder.eos_check_every = 1 << 30  # every pass runs its full length
        batch = synth_batch(a.pass_rows, a.passages, a.passage_len, a.query_len, 40, a.vocab, seed=123456, ragged=False)
        batch = {k: v.to(dev) for k, v in batch.items()}
        runs = {}
        for n in (0, 3):
            tag = "ban_off" if n == 0 else "n3"
            runs["greedy_" + tag] = lambda n=n: model.do_test(dict(batch), no_repeat_ngram=n)
            runs["beam_w4_" + tag] = lambda n=n: model.do_beam(dict(batch), width=4, no_repeat_ngram=n)
            runs["sample_" + tag] = lambda n=n: model.do_sample(dict(batch), seed=1, no_repeat_ngram=n)
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
                    times[n].append((time.perf_counter() - t0) * 1e3)
        res["points"] = [{"pass": n, "items": a.pass_rows, "steps": a.decode_len, "ms_per_pass": _stats(v)} for n, v in times.items()]
        for pt in res["points"]:
            print(json.dumps(pt))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
