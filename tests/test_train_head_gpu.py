"""The loss-only head of the training step on the MI355X: the two loss-form kernels (case_pointer_head_loss / _bwd) against K29 / K41 bit
for bit and against a float64 restatement; ``ops.TrainHeadFn`` against the dense chain (_generate + _mix + generation_nll) at one position of
the dropout stream; ``do_train`` of the tiny CaSE and Masque under CASE_TRAIN_HEAD=auto and =dense; the row-padded operand copy of the
vocabulary projection across optimizer steps, an EMA swap and a checkpoint load.  Measured figures go to profiles/train_head_parity.json."""
import json
import os

import pytest
import torch

from helpers import Calls, l2_error, scaled_error

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
CAP = 2e-5  # the cap of test_mrt_gpu.py's bars: none below is looser
# the loss-form kernels against the float64 restatement of nll = -log(prob + 1e-8): ten times the largest max |err| / max |ref| measured on
# the MI355X over every V and rows_per_source of the test (profiles/train_head_parity.json), never above the cap
LOSS_BAR = min(CAP, 10 * 1.344e-07)
# TrainHeadFn / do_train under auto against the dense chain in f32: ten times the largest distance measured on the MI355X, never above the cap
STEP_BAR = min(CAP, 10 * 1.038e-06)
# bf16, dense against fused (the tiny models): the losses by max error relative to scale, the parameter gradients by relative L2 error as
# tests/test_parity_prod_gpu.py measures them; ten times the measured distance, never looser than that file's bf16_auto bars (2e-2 / 0.11)
BF16_LOSS_BAR = min(2e-2, 10 * 6.973e-04)
BF16_GRAD_BAR = min(0.11, 10 * 1.489e-02)


def _measured(key, value, bar=None):
    """Add one measured maximum to profiles/train_head_parity.json."""
    path = os.path.join(ROOT, "profiles", "train_head_parity.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    data = {}
    if os.path.exists(path):
        with open(path) as fh:
            data = json.load(fh)
    data[key] = {"measured": float("%.3e" % value), "bar": bar}
    with open(path, "w") as fh:
        json.dump(data, fh, indent=1, sort_keys=True)
        fh.write("\n")


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class _Switch:
    """ops.<name> = value for the block."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        from case_rg_amd import ops
        self.old = getattr(ops, self.name)
        setattr(ops, self.name, self.value)

    def __exit__(self, *exc):
        from case_rg_amd import ops
        setattr(ops, self.name, self.old)


# ---------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------
def _restated_nll(logits, mix, copies, src_rows, targets):
    """nll [R] in the inputs' dtype, differentiable: -log(prob + 1e-8) of the rule in include/case_hip.h; prob is 1 at PAD (0) and 0 outside
    the vocabulary (neither depends on the inputs)."""
    R, V = logits.shape
    inside = (targets >= 0) & (targets < V)
    skip = targets.eq(0)
    y = targets.clamp(0, V - 1)
    gen_y = torch.softmax(logits, dim=-1).gather(1, y.unsqueeze(1)).squeeze(1)
    pm = torch.softmax(mix, dim=-1)
    hit = src_rows.eq(y.unsqueeze(1)).to(logits.dtype)
    p, at = pm[:, 0] * gen_y, 0
    for k, c in enumerate(copies):
        p = p + pm[:, 1 + k] * (c * hit[:, at:at + c.shape[1]]).sum(dim=1)
        at += c.shape[1]
    p = torch.where(skip, torch.ones_like(p), torch.where(inside, p, torch.zeros_like(p)))
    return torch.where(skip, torch.zeros_like(p), -torch.log(p + 1e-8))


def _k12_nll(prob, targets, pad):
    """-log(prob + 1e-8) in f32 with the logf of ``generation_nll``'s own kernel (K12, ops.nll_rows), 0 at PAD: every row's probability sits
    in column 1 of a two-column distribution and is gathered from there, so a row whose target lies outside the vocabulary (prob 0) is
    evaluated by the same expression.  ATen's log differs from the device logf in the last bit on some inputs; it is held to one ulp."""
    from case_rg_amd import ops
    dist = torch.stack([torch.zeros_like(prob), prob], dim=1)
    rows = ops.nll_rows(dist, torch.ones_like(targets))
    return torch.where(targets.eq(pad), torch.zeros_like(rows), rows)


@pytest.mark.parametrize("rps", [1, 4])
@pytest.mark.parametrize("V", [256, 257, 1000, 30522])
def test_loss_kernels_against_k29_k41_and_float64(V, rps):
    """13 rows (16 at rows_per_source 4: the entry points take whole items only), two memories of 5 + 19 positions, logits rows ld = V rounded
    up to 256 apart with NaN in the pad columns, d_logits NaN everywhere before the backward launch.  Targets hold PAD, -1, V and ids planted
    from the row's own source.  prob / copy / stats must carry K29's bits, nll = -log(prob + 1e-8) in f32 (0 at PAD), the f32 gradients
    K41's bits for g = -g_nll / (prob + 1e-8), the bf16 d_logits the round-to-nearest-even bf16 of the f32 one, the pad columns zeros;
    every gradient is held to LOSS_BAR against the float64 restatement; a second launch gives the same bits."""
    from case_rg_amd import ops
    R, lens, pad = (13 if rps == 1 else 16), [5, 19], 0
    ld = ops.rowpad_rows(V, 256)
    g = torch.Generator().manual_seed(7 * V + rps)
    logits = (torch.randn(R, V, generator=g) * 2.0).to(DEV)
    src = torch.randint(1, V, (R // rps, sum(lens)), generator=g)
    mix = torch.randn(R, 1 + len(lens), generator=g).to(DEV)
    copies = [(torch.softmax(torch.randn(R, n, generator=g) * 2.0, dim=-1) * (0.3 + 0.6 * torch.rand(R, 1, generator=g))).to(DEV) for n in lens]
    targets = torch.randint(1, V, (R,), generator=g)
    planted = torch.arange(R) % 3 == 0
    targets[planted] = src[torch.arange(R)[planted] // rps, torch.randint(0, sum(lens), (int(planted.sum()),), generator=g)]
    targets[1], targets[4], targets[9] = 0, -1, V
    g_nll = (torch.randn(R, generator=g) * 2.0).to(DEV)
    targets = targets.to(DEV)
    sm = ops.SortedSource(src.to(DEV), V)
    padded = torch.full((R, ld), float("nan"), device=DEV)
    padded[:, :V] = logits
    assert logits.data_ptr() % 16 == 0 and padded.data_ptr() % 16 == 0

    # forward: K29 with row statistics on the contiguous rows is the yardstick
    k_prob, k_copy, k_stats = ops.PointerScoreFn.apply(logits, mix, sm, rps, targets, pad, *copies)
    prob, copy, stats, nll = ops.pointer_head_loss(padded, V, mix, sm, rps, copies, targets, pad)
    assert _same_bits(prob, k_prob) and _same_bits(copy, k_copy) and _same_bits(stats, k_stats), "prob / copy / stats differ from K29's bits"
    want_nll = _k12_nll(prob, targets, pad)
    aten_nll = torch.where(targets.eq(pad), torch.zeros_like(prob), -torch.log(prob + 1e-8))
    print("V %d rps %d nll: %d rows differ from K12's logf, %d from ATen's log (max %d ulp)" % (
        V, rps, int((_bits(nll) != _bits(want_nll)).sum()), int((_bits(nll) != _bits(aten_nll)).sum()), int((_bits(nll) - _bits(aten_nll)).abs().max())))
    assert _same_bits(nll, want_nll), (nll, want_nll)
    assert int((_bits(nll) - _bits(aten_nll)).abs().max()) <= 1, "more than one ulp from ATen's log"
    assert float(nll[1]) == 0.0 and torch.isfinite(nll).all()
    again = ops.pointer_head_loss(padded, V, mix, sm, rps, copies, targets, pad)
    assert all(_same_bits(a, b) for a, b in zip(again, (prob, copy, stats, nll)))

    # backward: K41 fed dL/dprob is the yardstick
    g_prob = -g_nll / (prob + 1e-8)
    k_dl, k_dm, k_dc = ops.pointer_head_score_bwd(logits, mix, sm.ids, rps, copies, targets, pad, stats, prob, g_prob)

    def launch(dtype):
        out = (torch.full((R, ld), float("nan"), dtype=dtype, device=DEV), torch.full_like(mix, float("nan")),
               [torch.full_like(c, float("nan")) for c in copies])
        return ops.pointer_head_loss_bwd(padded, V, mix, sm.ids, rps, copies, targets, pad, stats, prob, g_nll, out=out)

    dl32, dm32, dc32 = launch(torch.float32)
    dl16, dm16, dc16 = launch(torch.bfloat16)
    assert _same_bits(dl32[:, :V], k_dl) and _same_bits(dm32, k_dm) and all(_same_bits(a, b) for a, b in zip(dc32, k_dc)), "not K41's bits"
    assert _same_bits(dm16, k_dm) and all(_same_bits(a, b) for a, b in zip(dc16, k_dc))
    assert _same_bits(dl16, dl32.to(torch.bfloat16)), "bf16 d_logits is not the f32 one rounded once to nearest even"
    assert bool((dl32[:, V:] == 0).all()) and bool((dl16[:, V:] == 0).all()), "pad columns of d_logits must be written as zeros"
    assert all(bool(torch.isfinite(t.float()).all()) for t in [dl32, dl16, dm32] + dc32)
    for a, b in zip(launch(torch.bfloat16)[0:1] + launch(torch.float32)[0:1], (dl16, dl32)):
        assert _same_bits(a, b), "two launches differ"

    # float64
    src_rows = sm.ids.repeat_interleave(rps, dim=0)
    leaves = [t.detach().double().requires_grad_(True) for t in [logits, mix] + copies]
    ref_nll = _restated_nll(leaves[0], leaves[1], leaves[2:], src_rows, targets)
    ref = torch.autograd.grad((ref_nll * g_nll.double()).sum(), leaves)
    scored = ((targets > 0) & (targets < V)).cpu().numpy()
    worst = {"nll": scaled_error("nll", nll.cpu().numpy()[scored], ref_nll.detach().cpu().numpy()[scored])}
    for name, want, got in zip(["d_logits", "d_mix"] + ["d_copy_%d" % k for k in range(len(lens))], ref, [dl32[:, :V], dm32] + dc32):
        worst[name] = scaled_error(name, got.cpu().numpy(), want.cpu().numpy())
    for name, e in worst.items():
        print("V %d rps %d %s: %.3e (bar %.3e)" % (V, rps, name, e, LOSS_BAR))
        _measured("kernels/V%d/rps%d/%s" % (V, rps, name), e, LOSS_BAR)
    assert all(e <= LOSS_BAR for e in worst.values()), worst


# ---------------------------------------------------------------------------------------------
# 2. the Function against the dense chain
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def fp32():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.set_dropout(True)
    case_rg_amd.config.manual_seed(77)
    yield
    case_rg_amd.set_dropout(False)
    case_rg_amd.set_compute_dtype(torch.float32)


def _decoder(V, H, seed=3):
    from case_rg_amd.CaSE.Model import CaSETransformerSeqDecoder
    from case_rg_amd.utils import fill_params
    return fill_params(CaSETransformerSeqDecoder(2, 1, 4, V, H), seed).to(DEV).train()


def _head_call_inputs(dec, B, T, lens, V, H, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(DEV).to(dtype)  # noqa: E731
    dec_in, x, feat = rnd(B, T, H), rnd(B, T, H), rnd(B, T, H)
    ctxs = [rnd(B, T, H) for _ in lens]
    copies = [torch.softmax(torch.randn(B, T, n, generator=g) * 2.0, dim=-1).to(DEV) for n in lens]
    src = torch.randint(1, V, (B, sum(lens)), generator=g)
    target = torch.randint(1, V, (B, T), generator=g)
    target[:, 0] = src[:, 0]
    target[:, T - 2:] = 0
    return dec_in, x, ctxs, copies, feat, src.to(DEV), target.to(DEV)


def _head_step(dec, inputs, mode, seed=77):
    """One call of the decoder's loss-only head under CASE_TRAIN_HEAD=``mode`` at dropout position (seed, 0): loss, gradients, the calls."""
    import case_rg_amd
    from case_rg_amd import ops
    from case_rg_amd.common.heads import nll_mean
    dec_in, x, ctxs, copies, feat, src, target = inputs
    leaves = [t.detach().clone().requires_grad_(True) for t in [dec_in, x, feat] + ctxs + copies]
    n = len(ctxs)
    case_rg_amd.config.manual_seed(seed)
    dec.zero_grad()
    with _Switch("TRAIN_HEAD", mode), Calls() as c:
        sm = ops.SortedSource(src, dec.tgt_vocab_size)
        rows = dec._train_nll(leaves[0], leaves[1], leaves[3:3 + n], leaves[3 + n:], leaves[2], sm, target)
        loss = nll_mean(rows, target)
        loss.backward()
    torch.cuda.synchronize()
    grads = {"in_%d" % i: t.grad.detach().clone() for i, t in enumerate(leaves) if t.grad is not None}
    grads.update({n_: p.grad.detach().clone() for n_, p in dec.named_parameters() if p.grad is not None})
    dec.zero_grad()
    return loss.detach(), rows.detach(), grads, c


def test_function_against_the_dense_chain(fp32):
    """H = 64, V = 1000, 80 rows (B = 4 x T = 20), f32, the generator's dropout on, both heads from the same position of the counter
    stream: the loss, the per-row losses and the gradients of every input and of gen[0], gen[2] and mix are held to STEP_BAR (max
    |difference| / max |dense| per tensor).  The gradient of the vocabulary weight is a contiguous [V, H] tensor."""
    V, H, B, T = 1000, 64, 4, 20
    dec = _decoder(V, H)
    inputs = _head_call_inputs(dec, B, T, [6, 18], V, H, seed=5)
    l_f, r_f, g_f, c_f = _head_step(dec, inputs, "auto")
    l_d, r_d, g_d, c_d = _head_step(dec, inputs, "dense")
    assert c_f.count("case_pointer_head_loss") == 1 and c_f.count("case_pointer_head_loss_bwd") == 1 and c_f.count("case_softmax_fwd") == 0, c_f.calls
    assert c_d.count("case_pointer_head_loss") == 0 and c_d.count("case_copy_scatter_sorted_fwd") == 1 and c_d.count("case_nll_gather_fwd") == 1
    assert set(g_f) == set(g_d) and "gen.2.weight" in g_f and "gen.0.bias" in g_f and "mix.weight" in g_f
    gw = g_f["gen.2.weight"]
    assert gw.shape == (V, H) and gw.is_contiguous()
    worst = {"loss": scaled_error("loss", l_f.cpu().numpy(), l_d.cpu().numpy()), "rows": scaled_error("rows", r_f.cpu().numpy(), r_d.cpu().numpy())}
    for k in g_d:
        if float(g_d[k].abs().max()) > 0:
            worst[k] = scaled_error(k, g_f[k].cpu().numpy(), g_d[k].cpu().numpy())
    for k, e in worst.items():
        print("function vs dense %s: %.3e (bar %.3e)" % (k, e, STEP_BAR))
        _measured("function/f32/%s" % k, e, STEP_BAR)
    assert all(e <= STEP_BAR for e in worst.values()), worst
    # the same dropout masks: both heads consumed the same stretch of the counter stream
    import case_rg_amd
    _head_step(dec, inputs, "auto")
    after_fused = case_rg_amd.config.rng_state()
    _head_step(dec, inputs, "dense")
    assert case_rg_amd.config.rng_state() == after_fused


def test_vocabulary_gemms_run_on_the_256_tiling():
    """bf16 at the benchmark's head shape (H = 512, V = 30 522, 1280 rows): the three vocabulary GEMMs of the fused head report tile 256,
    and no softmax / scatter / gather / cast launch touches a [rows, V] tensor."""
    import case_rg_amd
    from case_rg_amd import _abi, ops
    V, H, B, T = 30522, 512, 32, 40
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    case_rg_amd.set_dropout(True)
    try:
        dec = _decoder(V, H)
        inputs = _head_call_inputs(dec, B, T, [16, 48], V, H, seed=6, dtype=torch.bfloat16)
        dec_in, x, ctxs, copies, feat, src, target = inputs
        sm = ops.SortedSource(src, V)
        dec_out, gen_in = dec._head_parts(dec_in, x, feat)
        h = ops.linear(gen_in, dec.gen[0].weight, dec.gen[0].bias).detach().requires_grad_(True)
        mix = torch.randn(B * T, 3, device=DEV)
        sizes = []
        ops.TILE_TRACE = []
        with Calls() as c:
            counting = _abi.call

            def sized(name, *a):  # (element counts of the casts, on top of the call counts)
                if name == "case_cast":
                    sizes.append(a[2])
                return counting(name, *a)

            _abi.call = sized
            try:
                ops.cast_param_rowpad(dec.gen[-2].weight, torch.bfloat16, 256)  # (the operand copy exists before the step, as in training)
                sizes.clear()
                c.calls.clear()
                rows = ops.train_head_nll(h.reshape(B * T, H), dec.gen[-2].weight, mix, sm, T, [k.reshape(B * T, -1) for k in copies], target.reshape(-1))
                rows.sum().backward()
            finally:
                _abi.call = counting
        torch.cuda.synchronize()
        tiles = list(ops.TILE_TRACE)
        assert tiles == [256, 256, 256], tiles
        assert c.count("case_gemm") + c.count("case_gemm_dw_slabs") == 3, c.calls
        for name in c.calls:
            assert not name.startswith(("case_softmax", "case_copy_scatter", "case_nll")), c.calls
        assert all(n < B * T * V for n in sizes), "a cast over a [rows, V] tensor: %s" % sizes
        gw = dec.gen[-2].weight.grad
        assert gw.shape == (V, H) and gw.is_contiguous() and bool(torch.isfinite(gw).all()) and bool(torch.isfinite(h.grad.float()).all())
        assert bool(torch.isfinite(rows).all())
    finally:
        ops.TILE_TRACE = None
        case_rg_amd.set_dropout(False)
        case_rg_amd.set_compute_dtype(torch.float32)


# ---------------------------------------------------------------------------------------------
# 3. the models
# ---------------------------------------------------------------------------------------------
VOCAB = 300


def _model(kind, seed=40):
    from case_rg_amd.CaSE.Model import CaSE
    from case_rg_amd.Masque.Model import Masque
    from case_rg_amd.utils import fill_params, make_vocab
    v2i, i2v = make_vocab(VOCAB)
    m = CaSE(4, 8, i2v, v2i, 64) if kind == "case" else Masque(8, i2v, v2i, 64)
    return fill_params(m, seed).to(DEV)


def _batch(kind, seed=500, B=2):
    from case_rg_amd.utils import synth_batch
    return {k: v.to(DEV) for k, v in synth_batch(B, 3, 24, 12, 8, VOCAB, seed=seed, ragged=True, model=kind).items()}


def _train_step(model, batch, mode, seed=77):
    import case_rg_amd
    case_rg_amd.config.manual_seed(seed)
    model.zero_grad()
    with _Switch("TRAIN_HEAD", mode), Calls() as c:
        losses = model(dict(batch), method="train")
        sum(l.mean() for l in losses).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad()
    return [l.detach().clone() for l in losses], grads, c


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_do_train_auto_against_dense_f32(fp32, kind):
    """The tiny models in f32 with dropout on, one position of the counter stream: every loss and every parameter gradient under auto is
    held to STEP_BAR against dense.  ``Calls`` proves which head ran: under each switch, with CASE_POINTER_SCORE=off, and with a source map
    the decoder cannot sort on the device (a dense one-hot map, as a reference-style caller passes)."""
    m, b = _model(kind).train(), _batch(kind)
    l_f, g_f, c_f = _train_step(m, b, "auto")
    l_d, g_d, c_d = _train_step(m, b, "dense")
    assert c_f.count("case_pointer_head_loss") == 1 and c_f.count("case_pointer_head_loss_bwd") == 1 and c_f.count("case_nll_gather_fwd") == 0, c_f.calls
    assert c_d.count("case_pointer_head_loss") == 0 and c_d.count("case_nll_gather_fwd") == 1 and c_d.count("case_copy_scatter_sorted_fwd") == 1
    with _Switch("POINTER_SCORE", "off"):
        _, _, c_off = _train_step(m, b, "auto")
    assert c_off.count("case_pointer_head_loss") == 0 and c_off.count("case_nll_gather_fwd") == 1
    onehot = dict(b)
    onehot["source_map"] = torch.nn.functional.one_hot(b["source_map"], VOCAB).float()
    _, _, c_map = _train_step(m, onehot, "auto")
    assert c_map.count("case_pointer_head_loss") == 0 and c_map.count("case_nll_gather_fwd") == 1
    assert set(g_f) == set(g_d) and len(l_f) == len(l_d)
    worst_l = max(scaled_error("loss", a.cpu().numpy(), d.cpu().numpy()) for a, d in zip(l_f, l_d))
    worst_g = max(scaled_error(n, g_f[n].cpu().numpy(), g_d[n].cpu().numpy()) for n in g_d if float(g_d[n].abs().max()) > 0)
    print("%s f32: losses %.3e, worst parameter gradient %.3e (bar %.3e)" % (kind, worst_l, worst_g, STEP_BAR))
    _measured("do_train/%s/f32/losses" % kind, worst_l, STEP_BAR)
    _measured("do_train/%s/f32/param_grads" % kind, worst_g, STEP_BAR)
    assert worst_l <= STEP_BAR and worst_g <= STEP_BAR, (worst_l, worst_g)


@pytest.mark.parametrize("kind", ["case", "masque"])
def test_do_train_auto_against_dense_bf16(fp32, kind):
    """The same pair in bf16 (what the benchmark times): the losses by max error relative to scale, every parameter gradient by relative L2
    error, as tests/test_parity_prod_gpu.py measures its bf16_auto mode; the bars are the constants above."""
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    m, b = _model(kind).train(), _batch(kind)
    l_f, g_f, c_f = _train_step(m, b, "auto")
    l_d, g_d, _ = _train_step(m, b, "dense")
    assert c_f.count("case_pointer_head_loss") == 1
    worst_l = max(scaled_error("loss", a.float().cpu().numpy(), d.float().cpu().numpy()) for a, d in zip(l_f, l_d))
    worst_g = max(l2_error(g_f[n].float().cpu().numpy(), g_d[n].float().cpu().numpy()) for n in g_d if float(g_d[n].abs().max()) > 0)
    print("%s bf16: losses %.3e (bar %.3e), worst parameter gradient L2 %.3e (bar %.3e)" % (kind, worst_l, BF16_LOSS_BAR, worst_g, BF16_GRAD_BAR))
    _measured("do_train/%s/bf16/losses" % kind, worst_l, BF16_LOSS_BAR)
    _measured("do_train/%s/bf16/param_grads_l2" % kind, worst_g, BF16_GRAD_BAR)
    assert all(torch.isfinite(g).all() for g in g_f.values())
    assert worst_l <= BF16_LOSS_BAR and worst_g <= BF16_GRAD_BAR, (worst_l, worst_g)


def _padded_copy_is_current(w):
    from case_rg_amd import ops
    V = w.shape[0]
    wp = ops.cast_param_rowpad(w, torch.bfloat16, 256)
    assert wp.shape == (ops.rowpad_rows(V, 256), w.shape[1]) and wp.dtype == torch.bfloat16
    assert torch.equal(wp[:V], w.detach().to(torch.bfloat16)), "the padded copy's first V rows are not the bf16 cast of the parameter"
    assert bool((wp[V:] == 0).all()), "pad rows must be zero"
    return wp


def _decodes(model, batch):
    """(greedy answer, teacher-forced token probabilities of the reference answer) of ``model`` in eval mode: what do_test and do_score read
    through the operand copies of the registry."""
    was = model.training
    model.eval()
    with torch.no_grad():
        answer = model.do_test(dict(batch))["answer"].clone()
        probs = model.do_score(dict(batch))["token_probs"].clone()
    model.train(was)
    return answer, probs


def _decodes_like_a_fresh_model(model, batch, what):
    """do_test and do_score of ``model`` must give what a deep copy of it gives: the copy's Parameters are new objects, so every operand copy
    it reads is cast from its weights then and there and none can be stale.  -> the (answer, token_probs) of ``model``."""
    import copy
    got = _decodes(model, batch)
    want = _decodes(copy.deepcopy(model), batch)
    print("%s: token_probs differ from a fresh model's by %.3e" % (what, float((got[1] - want[1]).abs().max())))
    assert torch.equal(got[0], want[0]), "%s: do_test does not see the current weights" % what
    assert torch.equal(got[1], want[1]), "%s: do_score does not see the current weights" % what
    return got


def test_padded_operand_copy_follows_every_rewrite(fp32):
    """bf16 training of the tiny CaSE with FusedAdam (persistent operand copies) and an EMA.  After optimizer steps, an EMA swap, its restore
    and a checkpoint load over weights that have moved on, the row-padded operand copy of the vocabulary projection holds the bf16 cast of
    the parameter in its first V rows and zeros behind them, the optimizer's persistent copy is its prefix, and a following do_test and
    do_score give, bit for bit, what a deep copy of the model gives (which cannot read a stale copy).  The shadow weights, the trained
    weights and the weights one step later give different token probabilities, so the comparisons tell them apart."""
    import case_rg_amd
    from case_rg_amd import ops
    from case_rg_amd.common.EMA import EMA
    from case_rg_amd.optim import FusedAdam
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    m, b = _model("case").train(), _batch("case")
    w = m.response_generation.decoder.gen[-2].weight
    opt = FusedAdam(m.parameters(), lr=1e-2, low_precision=torch.bfloat16)
    ema = EMA(m, 0.9)
    ema.register()

    def step():
        m.zero_grad()
        sum(l.mean() for l in m(dict(b), method="train")).backward()
        opt.step(ema=ema)
        wp = _padded_copy_is_current(w)
        assert ops.cast_param(w, torch.bfloat16).data_ptr() == wp.data_ptr() == opt._low[id(w)].data_ptr(), "the optimizer's copy is the prefix"

    step()
    step()
    trained = w.detach().clone()
    at_trained = _decodes_like_a_fresh_model(m, b, "after two optimizer steps")
    ema.apply_shadow()
    assert not torch.equal(w.detach(), trained)
    _padded_copy_is_current(w)
    at_shadow = _decodes_like_a_fresh_model(m, b, "under the EMA shadow")
    assert not torch.equal(at_shadow[1], at_trained[1]), "the shadow weights must decode differently from the trained ones"
    ema.restore()
    assert torch.equal(w.detach(), trained)
    _padded_copy_is_current(w)
    restored = _decodes_like_a_fresh_model(m, b, "after the restore")
    assert torch.equal(restored[0], at_trained[0]) and torch.equal(restored[1], at_trained[1])
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step()  # the weights move on (and the optimizer refreshes its persistent copies) ...
    moved = _decodes_like_a_fresh_model(m, b, "after a third optimizer step")
    assert not torch.equal(moved[1], at_trained[1])
    m.load_state_dict(state)  # ... and the checkpoint brings the earlier ones back (in-place copies: the registry sees the moved _version)
    assert torch.equal(w.detach(), trained)
    _padded_copy_is_current(w)
    loaded = _decodes_like_a_fresh_model(m, b, "after the checkpoint load")
    assert torch.equal(loaded[0], at_trained[0]) and torch.equal(loaded[1], at_trained[1])
    m.train()
    with Calls() as c:
        losses = m(dict(b), method="train")
    assert c.count("case_pointer_head_loss") == 1 and all(torch.isfinite(l).all() for l in losses)


def _tiny_trainer(capture, seed=40):
    import case_rg_amd
    from case_rg_amd.CaSE.Model import CaSE
    from case_rg_amd.common.CumulativeTrainer import CumulativeTrainer
    from case_rg_amd.common.schedule import get_cosine_with_hard_restarts_schedule_with_warmup
    from case_rg_amd.optim import FusedAdam
    from case_rg_amd.utils import fill_params, make_vocab
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    case_rg_amd.set_dropout(True)
    case_rg_amd.config.manual_seed(99)
    v2i, i2v = make_vocab(VOCAB)
    model = fill_params(CaSE(4, 8, i2v, v2i, 64), seed).train()
    trainer = CumulativeTrainer(model, None, None, 0, 1, capture=capture)
    opt = FusedAdam(model.parameters(), lr=1e-3, low_precision=torch.bfloat16)
    return trainer, opt, get_cosine_with_hard_restarts_schedule_with_warmup(opt, 3, 100)


def test_captured_step_runs_the_fused_head_and_follows_the_eager_trainer():
    """Two bf16 trainers as in tests/test_step_graph_gpu.py (same weights, same five batches, dropout on): one eager, one that runs two
    eager steps, records the third and replays it for the rest.  The recorded step holds the fused head (nothing in it synchronises), losses and
    parameters follow the eager trainer to that file's bars -- the other weight gradients are f32 atomic sums -- and after the replays the
    row-padded operand copy is the bf16 cast of the vocabulary weight the replays left behind."""
    from case_rg_amd import config
    from case_rg_amd.utils import synth_batch
    batches = [{k: v.cuda() for k, v in synth_batch(2, 3, 24, 12, 8, VOCAB, seed=500 + s, ragged=False, model="case").items()} for s in range(5)]
    runs = []
    try:
        for capture_steps in (False, True):
            trainer, opt, sched = _tiny_trainer(capture=True)
            if not capture_steps:
                trainer.graphs = None  # device-state mode without captures: the eager yardstick
            losses, heads = [], []
            for b in batches:
                with Calls() as c:
                    losses.append(trainer.train_batch(0, b, "train", opt, sched))
                heads.append(c.count("case_pointer_head_loss"))
            torch.cuda.synchronize()
            w = trainer.model.response_generation.decoder.gen[-2].weight
            _padded_copy_is_current(w)
            runs.append(dict(losses=losses, heads=heads, params={n: p.detach().clone() for n, p in trainer.model.named_parameters()},
                             replays=0 if trainer.graphs is None else trainer.graphs.replays))
            trainer.close()
    finally:
        config.set_device_state(None)
        config.set_dropout(False)
        config.set_compute_dtype(torch.float32)
    eager, graph = runs
    assert eager["replays"] == 0 and graph["replays"] == 3
    assert eager["heads"] == [1] * 5 and graph["heads"] == [1, 1, 1, 0, 0], "the third step records the fused head, replays call no Python"
    for s, (a, b) in enumerate(zip(eager["losses"], graph["losses"])):
        assert all(abs(x - y) <= 2e-2 * max(1.0, abs(x)) for x, y in zip(a, b)), (s, a, b)
    for n, want in eager["params"].items():
        err = (graph["params"][n] - want).abs().max().item() / (want.abs().max().item() + 1e-12)
        assert err <= 5e-2, (n, err)
