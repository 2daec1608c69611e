"""Pins, without a GPU, what tests/test_additive_exact_gpu.py and tests/test_pointer_decode_exact_gpu.py rely on (tests/exact_inputs.py,
"K7 / K22"): the builders give what they claim for the seeds used (bf16-exact values, integer results, sums below 2^24); the shape lists
reach every launch path of case_additive_scores_fwd / _bwd (k7_paths restates the launchers); a float32 emulation of each arithmetic form
(tanhf; the factored exp2 with one reciprocal; exp(2x) with a division; K22's cached exponent) stays inside the derived bound on both
families; and each of seven restated faults -- a dropped h column, a neighbour's target row or source position, the gradient factor 4 taken
as 2, the prescale off by 1e-3, a missing j range of a split d_wq, a missing workgroup of d_v -- lands OUTSIDE the bound in at least one
element, so the bound is not so wide that it hides them.  The last is a condition on the inputs and the reference alone."""
import pytest
import torch

import exact_inputs as X
from test_small_ops_gpu import _tol

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SMALL = 1 << 21          # elements of [B, T, S, H] up to which a case is emulated on the host
MUTANT_SHAPES = [(2, 9, 70, 16), (2, 35, 17, 65)]   # the first has a split d_wq (two j ranges), the second a ragged target chunk


def _all_cases():
    """(B, T, S, H, dtype, aligned, which) of every GPU case."""
    out = [s + (dt, True, "fwd") for s in X.K7_FWD_TILED for dt in (F32, BF16)]
    out += [s[:4] + (dt, s[4], "fwd") for dt in (F32, BF16) for s in X.K7_FWD_ROWWISE[dt]]
    return out + [s + (dt, True, "bwd") for s in X.K7_BWD for dt in (F32, BF16)]


def _rounded(family, B, T, S, H, dt):
    wq, uh, v, ds = X.K7_FAMILIES[family](B, T, S, H, X.k7_seed(B, T, S, H))
    return wq, uh.to(dt).to(F64), v, ds


def test_shape_lists_reach_every_launch_path():
    fwd, bwd, figs = set(), set(), {}
    for B, T, S, H, dt, aligned, which in _all_cases():
        paths, fig = X.k7_paths(B, T, S, H, dt, aligned)
        figs[(B, T, S, H)] = fig
        if which == "fwd":
            fwd |= {p for p in paths if p.startswith("fwd")}
        else:
            bwd |= {p for p in paths if p.startswith("bwd")}
    assert X.K7_FWD_PATHS <= fwd, X.K7_FWD_PATHS - fwd
    assert X.K7_BWD_PATHS <= bwd, X.K7_BWD_PATHS - bwd
    # the figures the shapes were chosen for
    assert figs[(2, 70, 150, 512)]["gz"] == 3 and figs[(512, 70, 33, 8)]["gz"] == 1 and figs[(512, 70, 33, 8)]["tchunks"] == 3
    assert (figs[(2, 40, 200, 512)]["sch"], figs[(2, 40, 200, 512)]["last_range"], figs[(2, 40, 200, 512)]["hb"]) == (4, 8, 2)
    assert (figs[(128, 64, 300, 8)]["sch"], figs[(128, 64, 300, 8)]["j_per"], figs[(128, 64, 300, 8)]["last_range"]) == (2, 192, 108)
    assert (figs[(256, 64, 130, 8)]["base_wgs"], figs[(256, 64, 130, 8)]["sch"]) == (2048, 1)
    # every size the issue of these tests names is in a list
    assert {3, 32, 33, 70} <= {s[1] for s in X.K7_FWD_TILED} and {1, 63, 64, 65, 150} <= {s[2] for s in X.K7_FWD_TILED}
    assert {1, 63, 64, 65, 96, 512} <= {s[3] for s in X.K7_FWD_TILED}
    assert {4, 256, 260, 512, 6, 516} <= {s[3] for s in X.K7_FWD_ROWWISE[F32]} and {8, 512, 520, 1024, 1032} <= {s[3] for s in X.K7_FWD_ROWWISE[BF16]}
    assert all({1, 77, 1030} <= {s[2] for s in X.K7_FWD_ROWWISE[dt]} and {1, 2} == {s[1] for s in X.K7_FWD_ROWWISE[dt]} for dt in (F32, BF16))
    assert all(any(not s[4] for s in X.K7_FWD_ROWWISE[dt]) for dt in (F32, BF16))
    assert {1, 255, 256, 257, 512} <= {s[3] for s in X.K7_BWD} and {1, 7, 8, 9, 33, 65} <= {s[1] for s in X.K7_BWD}
    assert {1, 15, 16, 17, 64, 65} <= {s[2] for s in X.K7_BWD}


@pytest.mark.parametrize("case", sorted({c[:4] for c in _all_cases()}), ids=lambda s: "B%d-T%d-S%d-H%d" % s)
def test_builders_give_what_they_claim(case):
    B, T, S, H = case
    for family in ("ternary", "mid"):
        wq, uh, v, ds = X.K7_FAMILIES[family](B, T, S, H, X.k7_seed(B, T, S, H))
        assert float(wq.abs().max()) + float(uh.abs().max()) <= X.K7_CLAMP + 2 ** -4, "inside the clamp (a bf16 rounding of 10.5 included)"
        for t in (wq, v, ds):
            assert torch.equal(t.to(F32).to(F64), t)
    wq, uh, v, ds = X.k7_ternary(B, T, S, H, X.k7_seed(B, T, S, H))
    for t in (wq, uh, v, ds):
        assert torch.equal(t.to(BF16).to(F64), t), "ternary operands are exact in bf16"
    assert set(wq.unique().tolist()) <= {-10.0, 10.0} and set(uh.unique().tolist()) <= {-10.0, 10.0}
    assert set(v.unique().tolist()) <= {-2.0, -1.0, 1.0, 2.0} and float(ds.abs().max()) <= 3
    assert 3 * B * T * S < 2 ** 24 and 2 * 3 * max(T, S) < 2 ** 24 and 2 * H < 2 ** 24, "every sum of the family stays below 2^24"
    if B * T * S * H <= SMALL:
        ref = X.k7_reference(wq, uh, v, ds, "tanhf")
        for name, (val, _) in ref.items():
            exact = X.k7_ternary_exact(val)
            assert torch.equal(exact.to(F32).to(F64), exact), name
        if min(B, T, S, H) > 1:
            assert ref["s"][0].unique().numel() > 2 and ref["d_uh"][0].unique().numel() > 2


@pytest.mark.parametrize("form", X.K7_FORMS)
@pytest.mark.parametrize("family", ["ternary", "mid"])
def test_float32_emulation_of_each_form_stays_inside_the_bound(family, form):
    dt = F32 if form == "tanhf" else BF16
    cases = sorted({c[:4] for c in _all_cases() if c[0] * c[1] * c[2] * c[3] <= SMALL})
    assert len(cases) >= 20
    worst = 0.0
    for B, T, S, H in cases:
        wq, uh, v, ds = _rounded(family, B, T, S, H, dt)
        ds = None if form == "exp2x" else ds   # the row-wise kernel has no backward
        ref = X.k7_reference(wq, uh, v, ds, form)
        emu = X.k7_emulate(form, wq, uh, v, ds)
        for name, got in emu.items():
            val, bound = ref[name]
            if family == "ternary":   # on the host every form is exact (exp2(x) exp2(-x) is 1 there), up to the 1e-17 that 1 - tanh(20)^2 is
                assert float((got.to(F64) - val).abs().max()) < 1e-12, (form, name, (B, T, S, H))
            err = (got.to(F64) - val).abs()
            assert bool((err <= bound).all()), (form, name, (B, T, S, H), float((err / bound.clamp_min(1e-300)).max()))
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    assert worst < 1.0


def _mutants(wq, uh, v, ds, form, fig):
    """name -> {output: value} of each restated fault, in float64."""
    B, T, H = wq.shape
    S = uh.shape[1]
    ref = lambda *a, **k: {n: val for n, (val, _) in X.k7_reference(*a, form=form, **k).items()}
    v2 = v.clone()
    v2[-1] = 0.0
    wq2, uh2 = wq.clone(), uh.clone()
    wq2[:, T - 1] = wq[:, T - 2]
    uh2[:, S - 1] = uh[:, S - 2]
    good = ref(wq, uh, v, ds)
    out = {"the last h column dropped": ref(wq, uh, v2, ds),
           "the last target row reads its neighbour": ref(wq2, uh, v, ds),
           "the last source position reads its neighbour": ref(wq, uh2, v, ds),
           "the gradient factor 4 taken as 2": {"d_wq": good["d_wq"] / 2, "d_uh": good["d_uh"] / 2},
           "the prescale off by 1e-3": ref(wq, uh, v, ds, prescale=1.0 + 1e-3)}
    if fig["sch"] > 1:
        ds2 = ds.clone()
        ds2[:, :, (fig["sch"] - 1) * fig["j_per"]:] = 0.0
        out["one j range of the split d_wq missing"] = {"d_wq": ref(wq, uh, v, ds2)["d_wq"]}
    ds3 = ds.clone()
    ds3[B - 1, :, 16 * ((S - 1) // 16):] = 0.0
    out["d_v without one workgroup's contribution"] = {"d_v": ref(wq, uh, v, ds3)["d_v"]}
    return out


@pytest.mark.parametrize("form", ["tanhf", "factored"])
@pytest.mark.parametrize("family", ["ternary", "mid"])
def test_every_restated_fault_lands_outside_the_bound(family, form):
    dt = F32 if form == "tanhf" else BF16
    seen = set()
    for B, T, S, H in MUTANT_SHAPES:
        paths, fig = X.k7_paths(B, T, S, H, dt)
        wq, uh, v, ds = _rounded(family, B, T, S, H, dt)
        good = X.k7_reference(wq, uh, v, ds, form)
        for fault, outputs in _mutants(wq, uh, v, ds, form, fig).items():
            if fault == "the prescale off by 1e-3" and family == "ternary":
                continue   # the ternary family saturates: it is blind to the numerics, the mid-range family is there for them
            seen.add(fault)
            caught = []
            for name, val in outputs.items():
                ref, bound = good[name]
                if family == "ternary" and form == "tanhf":   # compared with torch.equal on the GPU
                    ref, val, bound = X.k7_ternary_exact(ref), X.k7_ternary_exact(val), torch.zeros_like(bound)
                if bool(((val - ref).abs() > bound).any()):
                    caught.append(name)
            assert caught, "%s hides inside the bound (%s, %s, B%d T%d S%d H%d)" % ((fault, family, form) + (B, T, S, H))
            if fault in ("the last h column dropped", "the last target row reads its neighbour", "the last source position reads its neighbour"):
                assert "s" in caught, "%s: the forward alone must show it" % fault
    assert len(seen) == (7 if family == "mid" else 6), seen


def test_key_exp_emulation_and_k22_scores_stay_inside_their_bounds():
    x = torch.cat([torch.linspace(-25.0, 25.0, 4001, dtype=F64).to(F32), torch.tensor([21.5, -21.5, 50.0, -50.0, 0.0, -0.0])])
    ref, f32_err = X.key_exp_reference(x)
    got = torch.exp((2.0 * x).clamp(-X.K22_CLAMP, X.K22_CLAMP)).to(BF16)
    assert bool(((got.to(F64) - ref).abs() <= _tol(ref, f32_err, BF16)).all())
    assert float((f32_err / ref).max()) < 2.0 ** -16 and bool((_tol(ref, f32_err, BF16) <= 2.0 ** -8 * (1 + 2.0 ** -7) * ref).all()), "half a bf16 ulp and the f32 error of __expf, not more"
    for B, S in ((3, 1), (3, 17), (2, 333)):
        wq, uh, v, mem = X.k22_midrange(B, S, seed=7 * S + B)
        eu = got.new_tensor(torch.exp((2.0 * uh.to(F32)).clamp(-43.0, 43.0)).tolist()).to(F64)   # the bf16 rows the kernel is handed
        ref = X.k22_reference(wq, eu, v, mem)
        s, s_b = ref["s"]
        assert bool(((X.k22_emulate(wq, eu, v).to(F64) - s).abs() <= s_b).all())
        assert float(s_b.max()) < 1e-3 and float((ref["p"][1] / ref["p"][0]).max()) < 2e-3, "f32 arithmetic only: far below the 3e-2 it replaces"
        # a wrong feature column or a neighbour's row is outside the bound on p
        eu2 = eu.clone()
        eu2[:, :, -1] = 1.0
        assert bool(((X.k22_reference(wq, eu2, v, mem)["p"][0] - ref["p"][0]).abs() > ref["p"][1]).any()) or S == 1
        if S > 1:
            eu3 = eu.clone()
            eu3[:, S - 1] = eu[:, S - 2]
            assert bool(((X.k22_reference(wq, eu3, v, mem)["p"][0] - ref["p"][0]).abs() > ref["p"][1]).any())


@pytest.mark.parametrize("B,S,n", [(3, 1, 1), (3, 17, 4), (2, 65, 64), (3, 333, 32), (2, 2048, 1024)])
def test_k22_ternary_family_is_exact(B, S, n):
    wq, uh, v, mem, best = X.k22_ternary(B, S, n, seed=S)
    for t in (wq, uh, v, mem):
        assert torch.equal(t.to(BF16).to(F64), t)
    assert bool((best.sum(-1) == n).all())
    eu = torch.exp(2.0 * uh.to(F32)).to(BF16).to(F64)
    ref = X.k22_reference(wq, eu, v, mem)
    s = ref["s"][0]
    assert torch.equal(ref["p"][0], best.to(F64) / n), "p is exactly 1 / n on the class and 0 elsewhere"
    for b in range(B):
        assert float(s[b][best[b]].max() - s[b][best[b]].min()) == 0.0, "the rows of the class have the same score"
        if (~best[b]).any():
            assert float(s[b][best[b]].min() - s[b][~best[b]].max()) >= 512.0, "e^-512 is 0 in f32"
    ctx = ref["ctx"][0]
    assert torch.equal((ctx * n).round() / n, ctx) and float(ctx.abs().max()) * n < 2 ** 24, "the class mean and its partial sums are exact in f32"
