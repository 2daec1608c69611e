"""K7, the additive (Bahdanau) attention of csrc/attn_pointer.hip -- additive_fwd_kernel, the eight additive_fwd_rowwise_kernel
instantiations, additive_bwd_uh_kernel and additive_bwd_wq_kernel -- through the C entry points case_additive_scores_fwd / _bwd on buffers
the test owns (NaN-filled; d_v zeroed, as the header requires), element by element against tests/exact_inputs.py's float64 restatement
(k7_reference), which is evaluated on the device from the SAME rounded inputs the kernel reads, in chunks over the items.

Two operand families (exact_inputs, "K7 / K22"; pinned on the CPU by test_additive_exact_cpu.py):

* ternary: every output is an integer (below 2^24) that depends on every one of b, t, j, h.  On the f32 path all four outputs -- d_v and
  the split d_wq through their atomics included -- must equal the reference in every bit (torch.equal).  On the bf16 path the only slack
  is that the device's 2^x 2^-x need not be exactly 1 and rcp(1 + tiny) need not be exactly 1: the bound below, (n + c) u sum |term| with
  the per-element terms of a saturated or centred tanh, far below the 1 an index error costs wherever n sum |term| < 2^22.
* mid-range: the bound is derived, not tuned.  k7_element gives the per-element error of the kernel's tanh and of its 1 - tanh^2 for each
  arithmetic form (tanhf; the factored 2^ws 2^us with one reciprocal; exp(2x) with a division) from the instructions' published accuracy
  (exact_inputs.EPS_EXP, EPS_RCP, EPS_FDIV, EPS_TANHF, each with its source) and the roundings of the arguments; k7_reference carries it
  through the sums:
      |ds|    <= sum_h |v_h| dth_h + c (H + 2) u sum_h |v_h|                      c = 2 for vsum - 2 acc (factored), else 1
      |dd_uh| <= |v_h| (sum_t |ds| dgp + (T + 4) u sum_t |ds| (1 - th^2))
      |dd_wq| <= |v_h| (sum_j |ds| dgp + (S + 4) u sum_j |ds| (1 - th^2))          any order, any split with atomics
      |dd_v|  <= sum_btj |ds| dth + c (B T S + 4) u sum_btj |ds| (|th| or 1)
  Nothing here is taken from what the kernels return.  A bound exceeded is a finding: the message names the element and both values.

Every case runs twice; s, d_uh and an un-split d_wq must be the same bits.  The shapes (exact_inputs.K7_FWD_TILED, K7_FWD_ROWWISE,
K7_BWD) are the smallest that reach each launch path; k7_paths restates the launchers and the CPU test asserts the reach.  All inputs
stay inside |x| <= 21 (the clamp's documented deviation is pinned in test_ops_gpu.py)."""
import pytest
import torch

import exact_inputs as X
import exact_ledger as L
from exact_ledger import ledger  # noqa: F401  (autouse fixture)
from test_small_ops_gpu import _check, _code, _counting, _misaligned, _nan, _raw, _same_bits, _tol

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTS = [F32, BF16]
FAMILIES = ["ternary", "mid"]


def _operands(family, B, T, S, H, dt, aligned=True):
    """The four operands as the kernel reads them, and the same values in float64."""
    wq, uh, v, ds = X.K7_FAMILIES[family](B, T, S, H, X.k7_seed(B, T, S, H))
    wq, v, ds = [t.to(DEV).to(F32).contiguous() for t in (wq, v, ds)]
    uh = uh.to(DEV).to(dt).contiguous()
    if not aligned:
        uh = _misaligned(uh)
    assert float(wq.abs().max()) + float(uh.float().abs().max()) <= X.K7_CLAMP
    return (wq, uh, v, ds), tuple(t.double() for t in (wq, uh, v, ds))


def _note(key, got, ref, bound):
    """The largest observed error over bound of this output, over the cases of the test function."""
    ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
    cur = L._CURRENT[0]
    if cur is not None:
        L.note(key, max(ratio, cur.get("figures", {}).get(key, 0.0)))


def _compare(name, got, ref, bound, family, dt, what):
    assert not torch.isnan(got).any(), "%s: %s has elements the kernel never wrote" % (what, name)
    if family == "ternary" and dt == F32:
        ref = X.k7_ternary_exact(ref)  # (the bf16 path is held to the unrounded value: its 4 r (1 - r) keeps the 1e-17 that 1 - tanh(20)^2 is)
        assert torch.equal(got.double(), ref), "%s: %s differs from the exact reference in %d of %d elements" % (
            what, name, int((got.double() != ref).sum()), ref.numel())
        L.record(ref.numel())
        return
    _check(got, ref, bound, "%s: %s" % (what, name))
    _note("%s %s %s: max error / bound" % (name, family, "f32" if dt == F32 else "bf16"), got, ref, bound)
    L.record(0, ref.numel(), "f32 sums and the device's tanhf / v_exp_f32 / v_rcp_f32 (bound derived in the docstring)")


def _fwd(ops, wq, uh, v, dt):
    B, T, H = wq.shape
    S = uh.shape[1]
    s = _nan(B, T, S)
    with _counting() as calls:
        _raw("case_additive_scores_fwd", wq, uh, v, s, B, T, S, H, _code(dt))
    assert calls == {"case_additive_scores_fwd": 1}
    return s


def _bwd(ops, ds, wq, uh, v, dt):
    B, T, H = wq.shape
    S = uh.shape[1]
    d_wq, d_uh, d_v = _nan(B, T, H), _nan(B, S, H), torch.zeros(H, dtype=F32, device=DEV)
    with _counting() as calls:
        _raw("case_additive_scores_bwd", ds, wq, uh, v, d_wq, d_uh, d_v, B, T, S, H, _code(dt))
    assert calls == {"case_additive_scores_bwd": 1}
    return d_wq, d_uh, d_v


@pytest.fixture
def ops():
    import case_rg_amd
    from case_rg_amd import ops
    case_rg_amd.set_dropout(False)
    return ops


def _forward_case(ops, family, dt, B, T, S, H, aligned, want_path):
    paths, fig = X.k7_paths(B, T, S, H, dt, aligned)
    assert fig["fwd"] == want_path, (fig, want_path)
    (wq, uh, v, _), (wq64, uh64, v64, _) = _operands(family, B, T, S, H, dt, aligned)
    ref, bound = X.k7_reference(wq64, uh64, v64, None, X.k7_form(want_path, dt))["s"]
    what = "%s %s B%d T%d S%d H%d%s" % (family, dt, B, T, S, H, "" if aligned else " misaligned")
    s = _fwd(ops, wq, uh, v, dt)
    _compare("s", s, ref, bound, family, dt, what)
    _same_bits(_fwd(ops, wq, uh, v, dt), s, what + ": s of a second launch")


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", X.K7_FWD_TILED, ids=lambda s: "B%d-T%d-S%d-H%d" % s)
def test_additive_forward_tiled(ops, shape, family, dt):
    _forward_case(ops, family, dt, *shape, True, "tiled")


def _rowwise_cases():
    return [pytest.param(dt, shape, id="%s-B%d-T%d-S%d-H%d-%s" % (("f32" if dt == F32 else "bf16",) + shape[:4] + ("aligned" if shape[4] else "misaligned",)))
            for dt in DTS for shape in X.K7_FWD_ROWWISE[dt]]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dt,shape", _rowwise_cases())
def test_additive_forward_rowwise_and_its_fallbacks(ops, dt, shape, family):
    B, T, S, H, aligned = shape
    ev = 4 if dt == F32 else 8
    rowwise = aligned and H % ev == 0 and H <= 128 * ev
    _forward_case(ops, family, dt, B, T, S, H, aligned, "rowwise" if rowwise else "tiled")


@pytest.mark.parametrize("dt", DTS, ids=["f32", "bf16"])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", X.K7_BWD, ids=lambda s: "B%d-T%d-S%d-H%d" % s)
def test_additive_backward(ops, shape, family, dt):
    B, T, S, H = shape
    paths, fig = X.k7_paths(B, T, S, H, dt)
    (wq, uh, v, ds), (wq64, uh64, v64, ds64) = _operands(family, B, T, S, H, dt)
    ref = X.k7_reference(wq64, uh64, v64, ds64, X.k7_form("tiled", dt))
    what = "%s %s B%d T%d S%d H%d" % ((family, dt) + shape)
    d_wq, d_uh, d_v = _bwd(ops, ds, wq, uh, v, dt)
    for name, got in (("d_wq", d_wq), ("d_uh", d_uh), ("d_v", d_v)):
        _compare(name, got, ref[name][0], ref[name][1], family, dt, what)
    d_wq2, d_uh2, d_v2 = _bwd(ops, ds, wq, uh, v, dt)
    _same_bits(d_uh2, d_uh, what + ": d_uh of a second launch")
    if "bwd.wq.unsplit" in paths:
        _same_bits(d_wq2, d_wq, what + ": un-split d_wq of a second launch")
    else:
        _compare("d_wq", d_wq2, ref["d_wq"][0], ref["d_wq"][1], family, dt, what + " (second launch)")
    _compare("d_v", d_v2, ref["d_v"][0], ref["d_v"][1], family, dt, what + " (second launch)")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", [(2, 9, 17, 257), (2, 40, 200, 512)], ids=lambda s: "B%d-T%d-S%d-H%d" % s)
def test_additive_scores_autograd_bf16_key_gradient(ops, shape, family):
    """ops.additive_scores with bf16 keys: s, d_wq and d_v by the same bounds, and the key gradient -- cast to bf16 by the Function -- within
    the ONE bf16 rounding of the f32 value."""
    B, T, S, H = shape
    (wq, uh, v, ds), (wq64, uh64, v64, ds64) = _operands(family, B, T, S, H, BF16)
    ref = X.k7_reference(wq64, uh64, v64, ds64, "factored")
    wq, uh, v = [t.requires_grad_() for t in (wq, uh, v)]
    s = ops.additive_scores(wq, uh, v)
    s.backward(ds)
    what = "autograd %s B%d T%d S%d H%d" % ((family,) + shape)
    assert uh.grad.dtype == BF16 and wq.grad.dtype == F32
    for name, got in (("s", s.detach()), ("d_wq", wq.grad), ("d_v", v.grad)):
        _compare(name, got, ref[name][0], ref[name][1], family, BF16, what)
    r, b = ref["d_uh"]
    _check(uh.grad, r, _tol(r, b, BF16), what + ": bf16 d_uh")
    L.record(0, r.numel(), "one rounding of the f32 key gradient to bf16")


def test_additive_scores_reject_bad_arguments_without_a_launch(ops):
    B, T, S, H = 2, 3, 5, 8
    (wq, uh, v, ds), _ = _operands("mid", B, T, S, H, F32)
    s, d_wq, d_uh, d_v = _nan(B, T, S), _nan(B, T, H), _nan(B, S, H), _nan(H)
    bad = [(65536, T, S, H), (0, T, S, H), (B, 0, S, H), (B, T, 0, H), (B, T, S, 0)]
    for dims in bad:
        for code in (0, 1):
            with pytest.raises(RuntimeError, match="bad argument"):
                _raw("case_additive_scores_fwd", wq, uh, v, s, *dims, code)
            with pytest.raises(RuntimeError, match="bad argument"):
                _raw("case_additive_scores_bwd", ds, wq, uh, v, d_wq, d_uh, d_v, *dims, code)
    fwd, bwd = [wq, uh, v, s], [ds, wq, uh, v, d_wq, d_uh, d_v]
    for i in range(len(fwd)):
        with pytest.raises(RuntimeError, match="bad argument"):
            _raw("case_additive_scores_fwd", *(fwd[:i] + [None] + fwd[i + 1:]), B, T, S, H, 0)
    for i in range(len(bwd)):
        with pytest.raises(RuntimeError, match="bad argument"):
            _raw("case_additive_scores_bwd", *(bwd[:i] + [None] + bwd[i + 1:]), B, T, S, H, 0)
    torch.cuda.synchronize()
    for name, t in (("s", s), ("d_wq", d_wq), ("d_uh", d_uh), ("d_v", d_v)):
        assert torch.isnan(t).all(), "%s was written by a rejected call" % name
    L.record(s.numel() + d_wq.numel() + d_uh.numel() + d_v.numel())
