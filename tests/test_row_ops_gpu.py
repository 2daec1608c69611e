"""Every LayerNorm and masked-softmax kernel form of csrc/rowops.hip, through the C ABI, against the float64 references and the derived
element-wise bounds of row_refs.py (whose power to tell right from wrong is shown by test_row_refs_cpu.py).

The calls are raw (_abi.call) onto NaN-filled outputs, so an element a kernel never writes is seen; the shapes are the smallest that reach
each branch of ln_fwd_vec_launch / ln_bwd_vec_launch / ln_bwd_drop_launch / softmax_launch.  Rows 1 (three of a workgroup's four waves
idle), 3 (fewer rows than waves) and 37 (odd: the tail row of the split kernels' row pair, several rows per wave with the prefetch of the
next row).  One short test per entry point runs the autograd wrapper and asserts that it makes the same call with the same bits.

With CASE_EXACT_LEDGER set, the forms run, the elements compared and the largest err / bound per form go to that file
(profiles/row_ops_parity.json)."""
import contextlib
import os

import pytest
import torch

import exact_ledger as L
import row_refs as RR
from exact_ledger import ledger  # noqa: F401  (autouse fixture)
from row_refs import BF16, F32

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROWS = (1, 3, 37)
FORMS = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def _ops():
    from case_rg_amd import config, ops
    config.set_dropout(False)
    return ops


def _code(dt):
    return 0 if dt == F32 else 1


def _name(dt):
    return "f32" if dt == F32 else "bf16"


def _misaligned(t):
    """A contiguous copy of ``t`` that does not start on a 16-byte boundary (one element into a fresh allocation)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 != 0
    return out


def _nan(*shape, dt=F32):
    return torch.full(shape, float("nan"), dtype=dt, device=DEV)


def _raw(name, *args):
    """The C entry point itself, on the current stream; tensors are passed as their addresses."""
    from case_rg_amd import _abi, ops
    _abi.call(name, *[ops._ptr(a) if torch.is_tensor(a) else a for a in args], ops._stream())


@contextlib.contextmanager
def _recording():
    """The C-ABI calls made inside the block: (name, the arguments that are not addresses)."""
    from case_rg_amd import _abi
    calls, inner = [], _abi.call

    def spy(name, *a):
        calls.append((name, a))
        return inner(name, *a)

    _abi.call = spy
    try:
        yield calls
    finally:
        _abi.call = inner


def _log(form, stats):
    """Per form: the cases run, the elements compared and the largest err / bound so far.  The ledger keeps figures per test function; the
    entry of a form is cumulative over the session, so the last test that ran a form holds its totals."""
    cur = FORMS.setdefault(form, {"cases": [], "elements": 0, "largest_err_over_bound": 0.0})
    cur["cases"].append(os.environ.get("PYTEST_CURRENT_TEST", "").split("::")[-1].split(" ")[0])
    cur["elements"] += stats.elements()
    cur["largest_err_over_bound"] = round(max(cur["largest_err_over_bound"], stats.worst()), 4)
    L.record(0, stats.elements(), "float64 reference, derived element-wise bound (row_refs.py)")
    L.note(form, {"cases": list(cur["cases"]), "elements": cur["elements"], "largest_err_over_bound": cur["largest_err_over_bound"]})


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln_table():
    t = []
    add = lambda dt, form, cols, mis=False: t.append((dt, cols, form, mis))
    for c in (36, 70):
        add(BF16, "scalar", c)
    add(BF16, "scalar", 512, True)
    for c in (8, 160, 520, 1032, 1544, 2056, 2568, 3080, 4088):  # 1, 1, 2 ... 8 chunks: every instantiation
        add(BF16, "guarded", c)
    for c in (256, 768, 1280):
        add(BF16, "wave8", c)
    for c in (1792, 2304, 2816, 3328, 3840):
        add(BF16, "split8", c)
    for c in (512, 1024):
        add(BF16, "wave", c)
    for c in (1536, 2048, 2560, 3072, 3584, 4096):
        add(BF16, "split", c)
    for c in (6, 2052, 4096):
        add(F32, "scalar", c)
    add(F32, "scalar", 256, True)
    for c in (4, 36, 260, 516, 772, 1028, 1284, 1540, 2044):
        add(F32, "guarded", c)
    for c in (256, 512):
        add(F32, "wave", c)
    for c in (768, 1024, 1280, 1536, 1792, 2048):
        add(F32, "split", c)
    return t


LN_TABLE = _ln_table()
LN_IDS = ["%s-%d-%s%s" % (_name(dt), c, form, "-misaligned" if mis else "") for dt, c, form, mis in LN_TABLE]
# the forward has one vector form per dtype (cols % E == 0, cols <= 512 E) and the scalar form; two widths above the vector range are added
LN_FWD_TABLE = LN_TABLE + [(BF16, 4104, "scalar", False)]
LN_FWD_IDS = LN_IDS + ["bf16-4104-scalar"]


def _expected_bwd_form(dt, cols, mis):
    """ln_bwd_vec_launch restated: which kernel a width reaches."""
    e = 4 if dt == F32 else 8
    if mis or cols % e or cols > 512 * e:
        return "scalar"
    if dt == BF16 and cols % 256 == 0 and cols % 512 != 0:
        return "wave8" if cols <= 1280 else "split8"
    nv = -(-cols // (64 * e))
    if cols != nv * 64 * e:
        return "guarded"
    return "split" if nv >= 3 else "wave"


def test_the_table_names_the_form_each_width_reaches():
    for dt, cols, form, mis in LN_TABLE:
        assert _expected_bwd_form(dt, cols, mis) == form, (dt, cols)
    assert {f for _, _, f, _ in LN_TABLE} == {"scalar", "guarded", "wave8", "split8", "wave", "split"}
    assert sorted(c // 256 for dt, c, f, _ in LN_TABLE if f == "split8") == [7, 9, 11, 13, 15]
    assert sorted(c // 512 for dt, c, f, _ in LN_TABLE if f == "split" and dt == BF16) == [3, 4, 5, 6, 7, 8]
    assert sorted(c // 256 for dt, c, f, _ in LN_TABLE if f == "split" and dt == F32) == [3, 4, 5, 6, 7, 8]


def _wave_cols(dt, form):
    return {"split8": 256, "split": 256 if dt == F32 else 512}.get(form)


def _ln_variants(dt, cols, form):
    """(label, case keyword arguments): the three row counts with all four of {x2, dx_add}, then every input class and the spike rows."""
    for rows in ROWS:
        for x2 in (False, True):
            for add in (False, True):
                yield "rows%d%s%s" % (rows, "+x2" if x2 else "", "+add" if add else ""), dict(rows=rows, x2=x2, add=add)
    for cls in RR.LN_CLASSES[1:]:
        yield cls, dict(rows=37, cls=cls, x2=True, add=True, seed=3)
    for sp in RR.spike_columns(cols, dt, _wave_cols(dt, form)):
        yield "spike%d" % sp, dict(rows=5, spike=sp, x2=sp % 2 == 0, add=True, seed=4)


def _ln_case(dt, cols, mis, **kw):
    case = RR.ln_inputs(kw.pop("rows"), cols, dt, dev=DEV, **kw)
    if mis:
        case["x"] = _misaligned(case["x"])
    return case


def _run_ln_fwd(case, gamma=None, beta=None):
    rows, cols, dt = case["rows"], case["cols"], case["dt"]
    y, mean, rstd = _nan(rows, cols, dt=dt), _nan(rows), _nan(rows)
    _raw("case_layernorm_fwd", case["x"], case["x2"], case["gamma"] if gamma is None else gamma, case["beta"] if beta is None else beta,
         y, mean, rstd, rows, cols, case["eps"], _code(dt))
    return y, mean, rstd


def _run_ln_bwd(case, mean, rstd):
    rows, cols, dt = case["rows"], case["cols"], case["dt"]
    dx = _nan(rows, cols, dt=dt)
    dg, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
    _raw("case_layernorm_bwd", case["dy"], case["x"], case["x2"], case["gamma"], mean, rstd, dx, case["dx_add"], dg, db, rows, cols, _code(dt))
    return dx, dg, db


@pytest.mark.parametrize("dt,cols,form,mis", LN_FWD_TABLE, ids=LN_FWD_IDS)
def test_layernorm_forward(dt, cols, form, mis):
    _ops()
    e = 4 if dt == F32 else 8
    fwd_form = "scalar" if mis or cols % e or cols > 512 * e else "vector"
    stats = RR.Stats()
    for label, kw in _ln_variants(dt, cols, form):
        if kw.pop("add"):
            if "cls" not in kw and "spike" not in kw:
                continue  # dx_add is no input of the forward
        case = _ln_case(dt, cols, mis, **kw)
        RR.ln_fwd_check(case, *_run_ln_fwd(case), stats, "%s %d %s" % (_name(dt), cols, label))
    _log("layernorm_fwd %s %s" % (_name(dt), fwd_form), stats)


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("which", ["gamma", "beta"])
def test_layernorm_forward_with_a_misaligned_parameter_takes_the_scalar_form(which, dt):
    _ops()
    stats = RR.Stats()
    for rows in ROWS:
        case = RR.ln_inputs(rows, 512, dt, x2=True, seed=6, dev=DEV)
        moved = _misaligned(case[which])
        want = _run_ln_fwd(case)
        got = _run_ln_fwd(case, **{which: moved})
        RR.ln_fwd_check(case, *got, stats, "misaligned %s" % which)
        RR.ln_fwd_check(case, *want, stats, "aligned")
    _log("layernorm_fwd %s scalar" % _name(dt), stats)


@pytest.mark.parametrize("dt,cols,form,mis", LN_TABLE, ids=LN_IDS)
def test_layernorm_backward(dt, cols, form, mis):
    _ops()
    stats = RR.Stats()
    for label, kw in _ln_variants(dt, cols, form):
        case = _ln_case(dt, cols, mis, **kw)
        mean, rstd = RR.ln_stats_f32(case)
        RR.ln_bwd_check(case, mean, rstd, *_run_ln_bwd(case, mean, rstd), stats, "%s %d %s" % (_name(dt), cols, label))
    _log("layernorm_bwd %s %s" % (_name(dt), form), stats)


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
def test_layernorm_backward_refuses_rows_wider_than_4096(dt):
    _ops()
    case = RR.ln_inputs(2, 4097, dt, dev=DEV)
    mean, rstd = RR.ln_stats_f32(case)
    with pytest.raises(RuntimeError, match="cols 4097 > 4096"):
        _run_ln_bwd(case, mean, rstd)


# ---- case_layernorm_bwd_dropout ---------------------------------------------------------------------------------------------------------
DROP_TABLE = [(BF16, c) for c in (256, 768, 1280, 2304, 3840, 512, 1024, 1536, 2560, 4096)] + [(F32, c) for c in (256, 512, 768, 2048)]
DROP_P, DROP_SEED, DROP_OFFSET = 0.3, 0x5EED1234, 4096 + 2


def _drop_form(dt, cols):
    if dt == BF16 and cols == 2560:
        return "rows5"
    return _expected_bwd_form(dt, cols, False)


def _run_ln_bwd_dropout(case, mean, rstd, offset=DROP_OFFSET):
    rows, cols, dt = case["rows"], case["cols"], case["dt"]
    dx, dropped = _nan(rows, cols, dt=dt), _nan(rows, cols, dt=dt)
    dg, db = torch.zeros(cols, device=DEV), torch.zeros(cols, device=DEV)
    _raw("case_layernorm_bwd_dropout", case["dy"], case["x"], case["gamma"], mean, rstd, dx, dropped, dg, db, rows, cols, DROP_P, DROP_SEED,
         offset, None, _code(dt))
    return dx, dropped, dg, db


def _dropout_keep(rows, cols, dt):
    ones = torch.ones(rows, cols, dtype=dt, device=DEV)
    out = _nan(rows, cols, dt=dt)
    _raw("case_dropout", ones, out, rows * cols, DROP_P, DROP_SEED, DROP_OFFSET, None, _code(dt))
    return out != 0


@pytest.mark.parametrize("dt,cols", DROP_TABLE, ids=["%s-%d-%s" % (_name(dt), c, _drop_form(dt, c)) for dt, c in DROP_TABLE])
def test_layernorm_backward_dropout(dt, cols):
    _ops()
    stats = RR.Stats()
    variants = [("rows%d" % r, dict(rows=r)) for r in ROWS] + [(c, dict(rows=37, cls=c, seed=3)) for c in RR.LN_CLASSES[1:]]
    variants += [("spike%d" % s, dict(rows=5, spike=s, seed=4)) for s in RR.spike_columns(cols, dt, _wave_cols(dt, _drop_form(dt, cols)))]
    for label, kw in variants:
        case = RR.ln_inputs(kw.pop("rows"), cols, dt, dev=DEV, **kw)
        mean, rstd = RR.ln_stats_f32(case)
        dx, dropped, dg, db = _run_ln_bwd_dropout(case, mean, rstd)
        what = "%s %d %s" % (_name(dt), cols, label)
        RR.ln_bwd_check(case, mean, rstd, dx, dg, db, stats, what)
        keep = _dropout_keep(case["rows"], cols, dt)
        kept = RR.dropped_check(dx, dropped, DROP_P, keep, what)
        if case["rows"] * cols >= 4096:
            assert 0.6 <= kept / keep.numel() <= 0.8, "%s: %d of %d kept at p = %.1f" % (what, kept, keep.numel(), DROP_P)
        stats.add("dx_dropped (bits)", keep.numel(), 0.0)
    _log("layernorm_bwd_dropout %s %s" % (_name(dt), _drop_form(dt, cols)), stats)


@pytest.mark.parametrize("dt,cols", [(BF16, 520), (BF16, 36), (BF16, 4104), (F32, 260), (F32, 2052)], ids=lambda v: _name(v) if isinstance(v, torch.dtype) else str(v))
def test_layernorm_backward_dropout_refuses_other_widths(dt, cols):
    _ops()
    case = RR.ln_inputs(3, cols, dt, dev=DEV)
    mean, rstd = RR.ln_stats_f32(case)
    with pytest.raises(RuntimeError, match="whole number of 64-lane chunks"):
        _run_ln_bwd_dropout(case, mean, rstd)


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
def test_layernorm_backward_dropout_refuses_an_odd_offset(dt):
    _ops()
    case = RR.ln_inputs(3, 512, dt, dev=DEV)
    mean, rstd = RR.ln_stats_f32(case)
    with pytest.raises(RuntimeError, match="offset must be even"):
        _run_ln_bwd_dropout(case, mean, rstd, offset=DROP_OFFSET + 1)


# ---- case_layernorm_bwd_concat5 ---------------------------------------------------------------------------------------------------------
def _concat5_case(rows, add, seed=5, **kw):
    H = 512
    case = RR.ln_inputs(rows, 5 * H, BF16, seed=seed, add=add, dev=DEV, **kw)
    x = case["x"]
    x[:, 3 * H:4 * H] = (x[:, :H].float() * x[:, H:2 * H].float()).to(BF16)  # G = [E | A1 | A2 | E o A1 | E o A2]
    x[:, 4 * H:] = (x[:, :H].float() * x[:, 2 * H:3 * H].float()).to(BF16)
    return case


def _run_concat5(case, mean, rstd, valid, H=512, dtype=None):
    rows, dt = case["rows"], case["dt"]
    de, d1, d2 = (_nan(rows, H, dt=dt) for _ in range(3))
    dg, db = torch.zeros(5 * H, device=DEV), torch.zeros(5 * H, device=DEV)
    x = case["x"]
    _raw("case_layernorm_bwd_concat5", case["dy"], x, case["gamma"], mean, rstd, case["dx_add"], x, x, x, valid, de, d1, d2, dg, db, rows, H,
         _code(dt) if dtype is None else dtype)
    return de, d1, d2, dg, db


def _paddings(rows):
    yield "all-live", torch.ones(rows, dtype=torch.uint8)
    for name, idx in (("first", 0), ("last", rows - 1), ("interior", rows // 2)):
        v = torch.ones(rows, dtype=torch.uint8)
        v[idx] = 0
        yield name, v
    if rows > 3:
        v = torch.ones(rows, dtype=torch.uint8)
        v[[0, rows // 2, rows - 1]] = 0
        yield "first+interior+last", v


@pytest.mark.parametrize("add", [False, True], ids=["", "dx_add"])
@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_backward_concat5(rows, add):
    _ops()
    stats = RR.Stats()
    variants = [("normal", {})] + ([(c, dict(cls=c)) for c in RR.LN_CLASSES[1:]] if rows == 37 else [])
    variants += [("spike%d" % s, dict(spike=s)) for s in RR.spike_columns(2560, BF16, 512)] if rows == 3 else []
    for label, kw in variants:
        case = _concat5_case(rows, add, **kw)
        mean, rstd = RR.ln_stats_f32(case)
        for pad, valid in _paddings(rows):
            valid = valid.to(DEV)
            RR.concat5_check(case, mean, rstd, valid, *_run_concat5(case, mean, rstd, valid), stats, "rows %d %s %s" % (rows, label, pad))
    _log("layernorm_bwd_concat5 bf16 rows5", stats)


def test_layernorm_backward_concat5_refuses_f32_and_other_widths():
    _ops()
    case = _concat5_case(3, False)
    mean, rstd = RR.ln_stats_f32(case)
    valid = torch.ones(3, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="built for bf16 rows of 5 x 512"):
        _run_concat5(case, mean, rstd, valid, dtype=0)
    with pytest.raises(RuntimeError, match="built for bf16 rows of 5 x 512"):
        _run_concat5(case, mean, rstd, valid, H=256)


# ---- the autograd wrappers make the same calls ------------------------------------------------------------------------------------------
def _scalars(call):
    name, args = call
    return name, tuple(a for a in args[:-1] if isinstance(a, (int, float)) and not isinstance(a, bool) and abs(a) < 2 ** 20)


@pytest.mark.parametrize("dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("carry", [False, True], ids=["layer_norm", "layer_norm_carry"])
def test_layernorm_wrappers_make_the_same_calls(carry, dt):
    ops = _ops()
    rows, cols = 3, 768  # one workgroup: the column sums' atomics have one order
    case = RR.ln_inputs(rows, cols, dt, x2=not carry, add=carry, seed=8, dev=DEV)
    x = case["x"].clone().requires_grad_()
    x2 = case["x2"].clone().requires_grad_() if not carry else None
    gamma, beta = case["gamma"].clone().requires_grad_(), case["beta"].clone().requires_grad_()
    with _recording() as calls:
        if carry:
            y, xc = ops.layer_norm_carry(x, gamma, beta, case["eps"])
            torch.autograd.backward([y, xc], [case["dy"], case["dx_add"]])
        else:
            y = ops.layer_norm(x, gamma, beta, case["eps"], add=x2)
            y.backward(case["dy"])
    with _recording() as raw:
        want_y, mean, rstd = _run_ln_fwd(case)
        want_dx, want_dg, want_db = _run_ln_bwd(case, mean, rstd)
    assert [_scalars(c) for c in calls] == [_scalars(c) for c in raw]
    assert [c[0] for c in calls] == ["case_layernorm_fwd", "case_layernorm_bwd"]
    RR.same_bits(y.detach(), want_y, "y")
    RR.same_bits(x.grad, want_dx, "dx")
    if x2 is not None:
        RR.same_bits(x2.grad, want_dx, "dx2")
    RR.same_bits(gamma.grad, want_dg, "d_gamma")
    RR.same_bits(beta.grad, want_db, "d_beta")
    stats = RR.Stats()
    RR.ln_fwd_check(case, want_y, mean, rstd, stats, "forward")
    RR.ln_bwd_check(case, mean, rstd, want_dx, want_dg, want_db, stats, "backward from the kernel's own statistics")


def test_concat5_layer_norm_carry_makes_the_same_calls():
    ops = _ops()
    rows, H = 3, 512
    case = _concat5_case(rows, True, seed=9)
    e, a1, a2 = (case["x"][:, i * H:(i + 1) * H].clone().requires_grad_() for i in range(3))
    valid = torch.tensor([1, 0, 1], dtype=torch.bool, device=DEV)
    gamma, beta = case["gamma"].clone().requires_grad_(), case["beta"].clone().requires_grad_()
    with _recording() as calls:
        G = ops.concat5(e, a1, a2, valid)
        out = ops.concat5_layer_norm_carry(G, gamma, beta, case["eps"])
        assert out is not None
        torch.autograd.backward(list(out), [case["dy"], case["dx_add"]])
    assert [c[0] for c in calls] == ["case_concat5_fwd", "case_layernorm_fwd", "case_layernorm_bwd_concat5"]
    case["x"] = G.detach()
    want_y, mean, rstd = _run_ln_fwd(case)
    vu = valid.view(torch.uint8)
    de, d1, d2, dg, db = _run_concat5(case, mean, rstd, vu)
    RR.same_bits(out[0].detach(), want_y, "y")
    for got, want, what in ((e.grad, de, "de"), (a1.grad, d1, "da1"), (a2.grad, d2, "da2"), (gamma.grad, dg, "d_gamma"), (beta.grad, db, "d_beta")):
        RR.same_bits(got, want, what)
    RR.concat5_check(case, mean, rstd, vu, de, d1, d2, dg, db, RR.Stats(), "wrapper")


# ---------------------------------------------------------------------------------------------------------------------------------
# softmax
# ---------------------------------------------------------------------------------------------------------------------------------
PAIRS = [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)]
PAIR_IDS = ["%s-%s" % (_name(a), _name(b)) for a, b in PAIRS]
SM_TABLE = [(8, False), (40, False), (512, False), (520, False), (1024, False), (1, False), (9, False), (63, False), (65, False), (1023, False),
            (512, True), (1025, False), (1032, False), (3000, False)]
SM_IDS = ["%d%s" % (c, "-misaligned" if m else "") for c, m in SM_TABLE]
MASKS = [("none", None, False), ("half", "half", False), ("one", "one", False), ("row_valid", None, True), ("both", "half", True)]


def _sm_form(in_dt, out_dt, C, mis, fwd):
    """softmax_launch restated."""
    if out_dt == BF16 and (fwd or in_dt == BF16) and C % 8 == 0 and C <= 1024 and not mis:
        return "vector%d" % (1 if C <= 512 else 2)
    return "scalar-wave" if C <= 1024 else "scalar-workgroup"


def test_the_softmax_table_reaches_every_form():
    seen = {(_name(i), _name(o), fwd, _sm_form(i, o, C, m, fwd)) for i, o in PAIRS for C, m in SM_TABLE for fwd in (True, False)}
    for i, o in PAIRS:
        for fwd in (True, False):
            want = {"scalar-wave", "scalar-workgroup"} | ({"vector1", "vector2"} if o == BF16 and (fwd or i == BF16) else set())
            assert {f for a, b, w, f in seen if (a, b, w) == (_name(i), _name(o), fwd)} == want


def _desc(case, drop=None):
    from case_rg_amd import ops
    return ops._softmax_desc(case["outer"], case["inner"], case["R"], case["C"], case["causal"], _code(case["in_dt"]), _code(case["out_dt"]), drop)


def _run_sm_fwd(case, drop=None, x=None, p_out=None):
    shape = (case["outer"], case["inner"], case["R"], case["C"])
    x = case["x"] if x is None else x
    p = _nan(*shape, dt=case["out_dt"]) if p_out is None else p_out
    y = _nan(*shape, dt=case["out_dt"]) if drop else p
    _raw("case_softmax_fwd", _desc(case, drop), x, case["col_valid"], case["row_valid"], p, y)
    return p, y


def _run_sm_bwd(case, dy, p, drop=None, dx=None):
    dx = _nan(*p.shape, dt=case["in_dt"]) if dx is None else dx
    _raw("case_softmax_bwd", _desc(case, drop), dy, p, dx)
    return dx


def _sm_case(in_dt, out_dt, C, mis, outer=2, inner=3, R=7, **kw):
    case = RR.softmax_inputs(outer, inner, R, C, in_dt, out_dt, dev=DEV, **kw)
    if mis:
        case["x"] = _misaligned(case["x"])
        case["dy"] = _misaligned(case["dy"])
    return case


def _sm_both(case, stats, label, mis=False):
    """Forward and backward of one case against float64; the in-place calls the product makes give the bits of the out-of-place ones."""
    p, _ = _run_sm_fwd(case)
    RR.softmax_fwd_check(case, p, stats, label)
    dx = _run_sm_bwd(case, case["dy"], p)
    RR.softmax_bwd_check(case, case["dy"], p, dx, stats, label)
    if case["in_dt"] == case["out_dt"]:
        dy2 = _misaligned(case["dy"]) if mis else case["dy"].clone()
        RR.same_bits(_run_sm_bwd(case, dy2, p, dx=dy2), dx, "%s: dx == dy in place" % label)
        if case["in_dt"] == F32:
            x2 = _misaligned(case["x"]) if mis else case["x"].clone()
            RR.same_bits(_run_sm_fwd(case, x=x2, p_out=x2)[0], p, "%s: p_out == x in place" % label)
    return p, dx


def _sm_log(case, mis, stats):
    i, o = case["in_dt"], case["out_dt"]
    _log("softmax %s->%s fwd %s / bwd %s" % (_name(i), _name(o), _sm_form(i, o, case["C"], mis, True), _sm_form(i, o, case["C"], mis, False)), stats)


@pytest.mark.parametrize("in_dt,out_dt", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("C,mis", SM_TABLE, ids=SM_IDS)
def test_softmax_layouts_and_masks(C, mis, in_dt, out_dt):
    _ops()
    stats = RR.Stats()
    for outer, inner, R in ((2, 3, 7), (1, 1, 1)):
        for name, cv, rv in MASKS:
            case = _sm_case(in_dt, out_dt, C, mis, outer, inner, R, seed=1, cv=cv, rv=rv)
            _sm_both(case, stats, "%dx%dx%d %s" % (outer, inner, R, name), mis)
    _sm_log(case, mis, stats)


CAUSAL_C = [8, 40, 520, 9, 65, 1025]


@pytest.mark.parametrize("in_dt,out_dt", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("C", CAUSAL_C)
def test_softmax_causal(C, in_dt, out_dt):
    _ops()
    stats = RR.Stats()
    for R in (C - 3, C, C + 2):
        for cv in (None, "one"):
            case = _sm_case(in_dt, out_dt, C, False, 2, 2, R, seed=2, cv=cv, causal=True)
            p, _ = _sm_both(case, stats, "R %d C %d cv %s" % (R, C, cv))
            assert bool((p[:, :, 0, 0] == 1).all()) and bool((p[:, :, 0, 1:] == 0).all()), "row 0 is exactly 1 on key 0"
            if R > C:
                assert bool((p[:, :, C:].float().sum(-1) - 1).abs().max() < 2e-2), "rows beyond C attend to every key"
    _sm_log(case, False, stats)


EMPTY_C = [40, 1024, 63, 1032]


@pytest.mark.parametrize("in_dt,out_dt", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("C", EMPTY_C)
def test_softmax_empty_and_minus_inf_rows(C, in_dt, out_dt):
    """A row with no admissible column, and a live row whose admissible scores are all -inf, give exact zeros and a zero gradient on
    every form (include/case_hip.h; common/BilinearAttention.py relies on it); one -inf inside a live row gives 0 there."""
    _ops()
    stats = RR.Stats()
    ninf = -float("inf")
    for causal in (False, True):
        case = _sm_case(in_dt, out_dt, C, False, 2, 3, 7, seed=3, cv="half", rv=True, causal=causal)
        x = case["x"]
        x[0, 0, 0, :] = ninf                      # every score of a live row
        x[0, 1, 1, case["col_valid"][0].bool()] = ninf  # every ADMISSIBLE score of a live row (outer 0 masks the upper half)
        x[1, 2, 0, :] = ninf                      # causal: row 0 sees key 0 only, which outer 1 masks as well
        x[1, 0, 2, C - 1] = ninf                  # one -inf inside a live row
        x[0, 2, 2, 0] = ninf
        case["row_valid"][0, :3] = 1
        case["row_valid"][1, 2] = 1
        p, dx = _sm_both(case, stats, "C %d causal %d" % (C, causal))
        for idx in ((0, 0, 0), (0, 1, 1), (1, 2, 0), (1, 0, 6)):
            assert bool((p[idx] == 0).all()) and bool((dx[idx] == 0).all()), "row %s is not exactly zero" % (idx,)
        assert p[1, 0, 2, C - 1] == 0 and p[0, 2, 2, 0] == 0
        assert torch.isfinite(p.float()).all() and torch.isfinite(dx.float()).all()
    _sm_log(case, False, stats)


@pytest.mark.parametrize("out_dt", [F32, BF16], ids=_name)
@pytest.mark.parametrize("C", [40, 1024, 63, 3000])
def test_softmax_large_scores(C, out_dt):
    """Scores of scale 30: exp(x - m) underflows for most columns (the 2^-126 floor of the bound)."""
    _ops()
    stats = RR.Stats()
    for name, cv, rv in MASKS[:1] + MASKS[4:]:
        case = _sm_case(F32, out_dt, C, False, 2, 3, 7, seed=4, scale=30.0, cv=cv, rv=rv)
        _sm_both(case, stats, "scale 30 %s" % name)
    _sm_log(case, False, stats)


@pytest.mark.parametrize("in_dt,out_dt", PAIRS, ids=PAIR_IDS)
@pytest.mark.parametrize("C", [40, 1024, 63, 1025])
def test_softmax_dropout(C, in_dt, out_dt):
    """y is 0 or p / (1 - p) within the bound; the backward, checked against float64 with the keep set read from the forward's own y, shows
    that the mask is regenerated identically.  Elements whose p is 0 carry no information and no weight."""
    _ops()
    stats = RR.Stats()
    drop = (0.3, 0xC0FFEE, 12346)
    for causal in (False, True):
        case = _sm_case(in_dt, out_dt, C, False, 2, 3, 7, seed=5, cv="one", causal=causal)
        p, y = _run_sm_fwd(case, drop)
        RR.softmax_fwd_check(case, p, stats, "dropout p")
        # a causal row r has r + 1 live keys: too few for the kept share to mean anything; the values are checked all the same
        kept = RR.softmax_dropout_check(case, y, drop[0], stats, "C %d causal %d" % (C, causal), share=not causal)
        dx = _run_sm_bwd(case, case["dy"], p, drop)
        RR.softmax_bwd_check(case, case["dy"], p, dx, stats, "dropout C %d causal %d" % (C, causal), keep=kept, drop_p=drop[0])
        if in_dt == out_dt:
            dy2 = case["dy"].clone()
            RR.same_bits(_run_sm_bwd(case, dy2, p, drop, dx=dy2), dx, "dropout: dx == dy in place")
    _sm_log(case, False, stats)


@pytest.mark.parametrize("in_dt,out_dt", PAIRS, ids=PAIR_IDS)
def test_masked_softmax_makes_the_same_calls(in_dt, out_dt):
    ops = _ops()
    case = _sm_case(in_dt, out_dt, 40, False, 2, 3, 7, seed=6, cv="one", rv=True)
    x = case["x"].clone().requires_grad_()
    with _recording() as calls:
        y = ops.masked_softmax(x, case["col_valid"].bool(), case["row_valid"].bool(), outer=2, out_dtype=out_dt)
        y.backward(case["dy"])
    assert [c[0] for c in calls] == ["case_softmax_fwd", "case_softmax_bwd"]
    for (_, args), want in zip(calls, (_desc(case), _desc(case))):
        got = args[0]
        assert all(getattr(got, f) == getattr(want, f) for f, _ in type(want)._fields_ if f != "state"), "descriptor"
    p, _ = _run_sm_fwd(case)
    RR.same_bits(y.detach(), p, "p")
    RR.same_bits(x.grad, _run_sm_bwd(case, case["dy"], p), "dx")
