"""The bounds of row_refs.py can tell right from wrong.

Each kernel of csrc/rowops.hip is emulated here in f32 torch, with every row or column sum taken in a shuffled, chunked order (as
exact_inputs.layer_norm_f32 does), and

(a) the honest emulation stays inside every bound, f32 and bf16, at every listed shape;
(b) each mutant is rejected on the f32, zero-mean cases -- except where BLIND says that a width or dtype cannot see it.

Known blind spots (nothing in (a) is loosened for them; test_row_ops_gpu.py adds spike rows for these):
* the (n + 2) u sum bound does not see ONE dropped term among thousands of comparable ones: on unit-normal rows of 4096 columns a mean or m2
  short of one column moves the statistic by |x| / n, against a bound of about n u * 0.8 -- seen only where the dropped value happens to be
  large, so those two are not REQUIRED to be rejected at 4096;
* an unbiased variance scales rstd by 1 + 1 / (2 n); at n = 4096 that is the (n + 8) u / 2 the variance sum is allowed, so it passes there, in
  f32 and bf16 alike (rstd is an f32 output in both);
* in bf16 the stored y / dx (half an ulp = 2^-9 relative) hide every one of these on rows wider than about 256: the bf16 rows of the matrix
  are rejected through the f32 outputs (mean, rstd, d_gamma, d_beta) and through the rows where the mutation happens to be large."""
import pytest
import torch

import row_refs as RR
from row_refs import BF16, F32

LN_SHAPES = [(37, 36, 0.0), (37, 256, 0.0), (5, 768, 100.0), (37, 2560, 0.0), (3, 2048, 0.0), (3, 4096, 0.0), (9, 512, 1000.0)]
LN_ZERO_MEAN = [(37, 36), (37, 256), (37, 2560), (3, 2048), (3, 4096)]
SM_WIDTHS = [9, 40, 384, 1024, 3000]


def _total(t, seed, dim=-1, drop_last=False):
    """Sum along ``dim`` in f32, eight shuffled chunks added one after the other."""
    t = t.movedim(dim, -1)
    n = t.shape[-1]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    if drop_last:
        perm = perm[perm != n - 1]
    acc = torch.zeros(t.shape[:-1], dtype=F32)
    for idx in perm.chunk(8):
        acc = acc + t[..., idx].sum(-1)
    return acc


def _v(case):
    v = case["x"].float()
    return v + case["x2"].float() if case["x2"] is not None else v


def emu_ln_fwd(case, seed, mutant=None):
    v, n = _v(case), case["cols"]
    gamma, beta = case["gamma"], case["beta"]
    if mutant == "gamma_neighbour":
        gamma = gamma.roll(1)
    mu = _total(v, seed, drop_last=mutant == "mean_short") / n
    d = v - mu[:, None]
    var = _total(d * d, seed + 1) / (n - 1 if mutant == "unbiased" else n)
    rs = torch.rsqrt(var + torch.tensor(case["eps"], dtype=F32))
    y = (d * rs[:, None]) * gamma + beta
    return y.to(case["dt"]), mu, rs


def emu_ln_bwd(case, mean, rstd, seed, mutant=None):
    v, n, R = _v(case), case["cols"], case["rows"]
    gamma, dy = case["gamma"], case["dy"].float()
    if mutant == "gamma_neighbour":
        gamma = gamma.roll(1)
    xh = (v - mean[:, None]) * rstd[:, None]
    gy = dy * gamma
    m1 = _total(gy, seed) / n
    m2 = _total(gy * xh, seed + 1, drop_last=mutant == "m2_short") / n
    if mutant == "m1_dropped":
        m1 = torch.zeros_like(m1)
    dx = rstd[:, None] * (gy - m1[:, None] - xh * m2[:, None])
    if case["dx_add"] is not None:
        dx = dx + case["dx_add"].float()
    dg = _total(dy * xh, seed + 2, dim=0, drop_last=mutant == "dgamma_short" and R > 1)
    db = _total(dy, seed + 3, dim=0)
    return dx.to(case["dt"]), dg, db


def emu_softmax_fwd(case, seed, mutant=None):
    c = dict(case)
    if mutant == "col_valid_shifted" and c["col_valid"] is not None:
        c["col_valid"] = c["col_valid"].roll(1, -1)
    live = RR.softmax_live(c)
    if mutant == "causal_r":
        R, C = c["R"], c["C"]
        live = live & (torch.arange(C)[None, :] < torch.arange(R)[:, None])
    x = c["x"].float()
    m = torch.where(live, x, torch.full_like(x, -float("inf"))).amax(-1, keepdim=True)
    ok = live.any(-1, keepdim=True)
    e = torch.where(live, torch.exp(x - torch.where(ok, m, torch.zeros_like(m))), torch.zeros_like(x))
    s = _total(e, seed, drop_last=mutant == "sum_short")[..., None]
    inv = torch.where(s > 0, 1.0 / s, torch.zeros_like(s))
    return (e * inv).to(c["out_dt"])


def emu_softmax_bwd(case, p, seed, mutant=None):
    g, pv = case["dy"].float(), p.float()
    dot = _total(g * pv, seed, drop_last=mutant == "dot_short")[..., None]
    return (pv * (g - dot)).to(case["in_dt"])


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the honest emulation is inside every bound
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln_case(rows, cols, shift, dt, x2, add, seed=1):
    case = RR.ln_inputs(rows, cols, dt, seed=seed, x2=x2, add=add)
    if shift:
        case["x"] = (case["x"].float() + shift).to(dt)
    return case


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols,shift", LN_SHAPES, ids=["%dx%d%s" % (r, c, "+%d" % s if s else "") for r, c, s in LN_SHAPES])
def test_honest_layernorm_is_inside_every_bound(rows, cols, shift, dt):
    stats = RR.Stats()
    for x2, add in ((False, False), (True, True)):
        case = _ln_case(rows, cols, shift, dt, x2, add)
        y, mu, rs = emu_ln_fwd(case, seed=3)
        RR.ln_fwd_check(case, y, mu, rs, stats, "forward")
        mean, rstd = RR.ln_stats_f32(case)
        dx, dg, db = emu_ln_bwd(case, mean, rstd, seed=5)
        RR.ln_bwd_check(case, mean, rstd, dx, dg, db, stats, "backward")
    assert stats.worst() <= 1.0
    print("layernorm %dx%d %s worst err/bound %.3f" % (rows, cols, dt, stats.worst()))


@pytest.mark.parametrize("cls", RR.LN_CLASSES + ("spike",))
@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
def test_honest_layernorm_input_classes(dt, cls):
    stats = RR.Stats()
    for cols in (36, 1280):
        spikes = RR.spike_columns(cols, dt, 256) if cls == "spike" else [None]
        for sp in spikes:
            case = RR.ln_inputs(5, cols, dt, cls="normal" if cls == "spike" else cls, seed=2, x2=True, add=True, spike=sp)
            y, mu, rs = emu_ln_fwd(case, seed=3)
            RR.ln_fwd_check(case, y, mu, rs, stats, "forward")
            mean, rstd = RR.ln_stats_f32(case)
            RR.ln_bwd_check(case, mean, rstd, *emu_ln_bwd(case, mean, rstd, seed=5), stats, "backward")


@pytest.mark.parametrize("add", [False, True], ids=["", "dx_add"])
def test_honest_concat5_is_inside_every_bound(add):
    H, rows = 512, 5
    case = RR.ln_inputs(rows, 5 * H, BF16, seed=4, add=add)
    x = case["x"]
    x[:, 3 * H:4 * H] = (x[:, :H].float() * x[:, H:2 * H].float()).to(BF16)
    x[:, 4 * H:] = (x[:, :H].float() * x[:, 2 * H:3 * H].float()).to(BF16)
    valid = torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)
    mean, rstd = RR.ln_stats_f32(case)
    dG, dg, db = emu_ln_bwd(case, mean, rstd, seed=6)
    g = dG.float()
    E, A1, A2 = (x[:, i * H:(i + 1) * H].float() for i in range(3))
    ok = valid.bool()[:, None]
    de = torch.where(ok, g[:, :H] + g[:, 3 * H:4 * H] * A1 + g[:, 4 * H:] * A2, torch.zeros(())).to(BF16)
    d1 = torch.where(ok, g[:, H:2 * H] + g[:, 3 * H:4 * H] * E, torch.zeros(())).to(BF16)
    d2 = torch.where(ok, g[:, 2 * H:3 * H] + g[:, 4 * H:] * E, torch.zeros(())).to(BF16)
    stats = RR.Stats()
    RR.concat5_check(case, mean, rstd, valid, de, d1, d2, dg, db, stats, "concat5")
    assert _rejected(lambda: RR.concat5_check(case, mean, rstd, valid, de, d2, d1, dg, db, RR.Stats(), "swapped"))
    live = torch.ones_like(valid)
    assert _rejected(lambda: RR.concat5_check(case, mean, rstd, live, de, d1, d2, dg, db, RR.Stats(), "no padding"))


def _sm_cases(C, in_dt, out_dt):
    yield "plain", RR.softmax_inputs(2, 3, 7, C, in_dt, out_dt, seed=1)
    yield "masks", RR.softmax_inputs(2, 3, 7, C, in_dt, out_dt, seed=2, cv="half", rv=True)
    yield "one", RR.softmax_inputs(2, 3, 7, C, in_dt, out_dt, seed=3, cv="one")
    yield "causal", RR.softmax_inputs(2, 1, 11, C, in_dt, out_dt, seed=4, cv="one", causal=True)
    yield "scale30", RR.softmax_inputs(1, 2, 3, C, in_dt, out_dt, seed=5, scale=30.0)


@pytest.mark.parametrize("in_dt,out_dt", [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)], ids=["f32", "bf16", "bf16-f32", "f32-bf16"])
@pytest.mark.parametrize("C", SM_WIDTHS)
def test_honest_softmax_is_inside_every_bound(C, in_dt, out_dt):
    stats = RR.Stats()
    for name, case in _sm_cases(C, in_dt, out_dt):
        p = emu_softmax_fwd(case, seed=7)
        RR.softmax_fwd_check(case, p, stats, name)
        RR.softmax_bwd_check(case, case["dy"], p, emu_softmax_bwd(case, p, seed=8), stats, name)
    assert stats.worst() <= 1.0
    print("softmax C=%d %s->%s worst err/bound %.3f" % (C, in_dt, out_dt, stats.worst()))


def test_softmax_reference_on_empty_and_minus_inf_rows():
    case = RR.softmax_inputs(2, 2, 3, 16, F32, F32, seed=1, cv="half", rv=True)
    case["x"][0, 0, 0, :] = -float("inf")        # a live row whose scores are all -inf
    case["x"][0, 1, 0, 3] = -float("inf")        # one -inf inside a live row (columns 0..7 are the live half of outer 0)
    p, bound, live = RR.softmax_fwd_ref(case)
    assert not live[0, 0, 0].any() and bool((p[0, 0, 0] == 0).all())
    assert p[0, 1, 0, 3] == 0 and abs(float(p[0, 1, 0].sum()) - 1) < 1e-12
    assert bool((p[-1, :, -1] == 0).all()), "row_valid 0"
    assert torch.isfinite(p).all() and torch.isfinite(bound).all()
    emu = emu_softmax_fwd(case, seed=2)
    RR.softmax_fwd_check(case, emu, RR.Stats(), "emulation")
    nan = emu.clone()
    nan[0, 0, 0] = float("nan")
    assert _rejected(lambda: RR.softmax_fwd_check(case, nan, RR.Stats(), "NaN row"))


def test_softmax_dropout_reference():
    case = RR.softmax_inputs(2, 3, 7, 40, F32, BF16, seed=9, cv="one")
    p = emu_softmax_fwd(dict(case, out_dt=F32), seed=1)
    keep = torch.rand(p.shape, generator=torch.Generator().manual_seed(3)) >= 0.3
    y = torch.where(keep, p * RR.keep_scale_f32(0.3), torch.zeros(())).to(BF16)
    stats = RR.Stats()
    kept = RR.softmax_dropout_check(case, y, 0.3, stats, "dropout")
    live = RR.softmax_live(case)
    assert torch.equal(kept, keep & live)
    pb = p.to(BF16)
    g = torch.where(kept, case["dy"].float() * RR.keep_scale_f32(0.3), torch.zeros(()))
    dot = (g * pb.float()).sum(-1, keepdim=True)
    dx = (pb.float() * (g - dot)).to(F32)
    RR.softmax_bwd_check(case, case["dy"], pb, dx, stats, "dropout", keep=kept, drop_p=0.3)
    other = kept.roll(1, -1)
    assert _rejected(lambda: RR.softmax_bwd_check(case, case["dy"], pb, dx, RR.Stats(), "other mask", keep=other, drop_p=0.3))
    assert _rejected(lambda: RR.softmax_dropout_check(case, (y.float() * 0.7).to(BF16), 0.3, RR.Stats(), "unscaled"))


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the mutants
# ---------------------------------------------------------------------------------------------------------------------------------
LN_FWD_MUTANTS = ("mean_short", "unbiased", "gamma_neighbour")
LN_BWD_MUTANTS = ("gamma_neighbour", "m2_short", "m1_dropped", "dgamma_short")
# (mutant, cols, dtype) the bounds cannot see on unit-normal rows -- see the module docstring.  Everything not listed must be rejected.
BLIND = {
    ("unbiased", 4096, "f32"), ("unbiased", 4096, "bf16"),
    ("mean_short", 4096, "f32"), ("mean_short", 4096, "bf16"),
    ("m2_short", 4096, "f32"), ("m2_short", 4096, "bf16"),
}
SM_BLIND = set()


def _ln_mutant_rejected(mutant, rows, cols, dt, fwd):
    case = RR.ln_inputs(rows, cols, dt, seed=1)
    if fwd:
        y, mu, rs = emu_ln_fwd(case, seed=3, mutant=mutant)
        return _rejected(lambda: RR.ln_fwd_check(case, y, mu, rs, RR.Stats(), mutant))
    mean, rstd = RR.ln_stats_f32(case)
    out = emu_ln_bwd(case, mean, rstd, seed=5, mutant=mutant)
    return _rejected(lambda: RR.ln_bwd_check(case, mean, rstd, *out, RR.Stats(), mutant))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mutant,fwd", [(m, True) for m in LN_FWD_MUTANTS] + [(m, False) for m in LN_BWD_MUTANTS],
                         ids=["fwd-" + m for m in LN_FWD_MUTANTS] + ["bwd-" + m for m in LN_BWD_MUTANTS])
def test_layernorm_mutants_are_rejected(mutant, fwd, dt):
    name = "f32" if dt == F32 else "bf16"
    seen = {}
    for rows, cols in LN_ZERO_MEAN:
        seen[cols] = _ln_mutant_rejected(mutant, rows, cols, dt, fwd)
    print(mutant, name, seen)
    missed = {c for c, hit in seen.items() if not hit}
    allowed = {c for (m, c, d) in BLIND if m == mutant and d == name}
    assert missed <= allowed, "%s (%s) passes at cols %s" % (mutant, name, sorted(missed - allowed))
    if dt == F32:
        assert any(seen.values())


@pytest.mark.parametrize("mutant", ["sum_short", "dot_short", "col_valid_shifted", "causal_r"])
def test_softmax_mutants_are_rejected(mutant):
    seen = {}
    for C in SM_WIDTHS:
        case = RR.softmax_inputs(2, 3, 7, C, F32, F32, seed=2, cv="one", causal=mutant == "causal_r")
        if mutant == "dot_short":
            p = emu_softmax_fwd(case, seed=7)
            dx = emu_softmax_bwd(case, p, seed=8, mutant=mutant)
            seen[C] = _rejected(lambda: RR.softmax_bwd_check(case, case["dy"], p, dx, RR.Stats(), mutant))
        else:
            p = emu_softmax_fwd(case, seed=7, mutant=mutant)
            seen[C] = _rejected(lambda: RR.softmax_fwd_check(case, p, RR.Stats(), mutant))
    print(mutant, seen)
    missed = {c for c, hit in seen.items() if not hit}
    assert missed <= {c for (m, c) in SM_BLIND if m == mutant}, "%s passes at C %s" % (mutant, sorted(missed))
    assert any(seen.values())
