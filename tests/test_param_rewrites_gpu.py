"""The forward reads the CURRENT weights after every way the parameters can be rewritten.

The hot path reads derived copies of the f32 parameters, not the parameters themselves: bf16 operand casts of whole parameters and of
views (ops.cast_param), the fused encoder chain's fragment-ordered packs (ops._chain_pack), the folded decode projections of K21
(MultiheadAttention.absorbed), Highway's row-concatenated weights and the optimizer's persistent bf16 copies (FusedAdam._low).  Every
check here runs a consumer once (filling its cache), rewrites the parameters through one path, runs the consumer again and compares
that result with (a) the same consumer after ops.invalidate_param_cache() -- a cold cache -- and (b) float64 torch on the CPU evaluated
from the current f32 weights, to the bf16 bar the suite uses for that op.  Each check also asserts that the rewrite moved the float64
output by at least ten times that bar, so that a stale copy cannot pass.  The replay of a captured training step rewrites every
parameter through raw pointers: the model-level scenario at the end predicts between replays without an EMA swap."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-2    # bf16 path vs float64, relative to max |reference| (test_encoder_chain_gpu.py, test_attn_mqa_gpu.py)
COLD = 1e-3   # warm vs cold cache: the same kernels on the same weights


@pytest.fixture()
def bf16_mode():
    import case_rg_amd
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    case_rg_amd.set_dropout(False)
    yield
    case_rg_amd.set_compute_dtype(torch.float32)
    case_rg_amd.ops.invalidate_param_cache()


class _Counting(object):
    """Counts the C-ABI launches by name while active."""

    def __enter__(self):
        from case_rg_amd import _abi
        self.calls, self._raw = {}, _abi.call

        def counting(name, *a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return self._raw(name, *a)

        _abi.call = counting
        return self

    def __exit__(self, *exc):
        from case_rg_amd import _abi
        _abi.call = self._raw


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references, evaluated from the module's current f32 weights
# ---------------------------------------------------------------------------------------------------------------------------------
def _d(t):
    return t.detach().double().cpu()


def _mha64(m, x, mem, valid):
    """Cross-attention of x [N, Lq, E] over mem [N, S, E] through m's projections, no residual."""
    E, h, d = m.embed_dim, m.num_heads, m.head_dim
    W, b = _d(m.in_proj_weight), _d(m.in_proj_bias)
    x, mem = _d(x), _d(mem)
    N, Lq, S = x.shape[0], x.shape[1], mem.shape[1]
    q = (x @ W[:E].T + b[:E]).reshape(N, Lq, h, d).transpose(1, 2)
    k = (mem @ W[E:2 * E].T + b[E:2 * E]).reshape(N, S, h, d).transpose(1, 2)
    v = (mem @ W[2 * E:].T + b[2 * E:]).reshape(N, S, h, d).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) / math.sqrt(d)
    s = s.masked_fill(~valid.cpu()[:, None, None, :], float("-inf"))
    o = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(N, Lq, E)
    return o @ _d(m.out_proj.weight).T + _d(m.out_proj.bias)


def _highway64(hw, x):
    x = _d(x)
    for n, l, g in zip(hw.nonlinear, hw.linear, hw.gate):
        gate = torch.sigmoid(x @ _d(g.weight).T + _d(g.bias))
        x = gate * torch.tanh(x @ _d(n.weight).T + _d(n.bias)) + (1 - gate) * (x @ _d(l.weight).T + _d(l.bias))
    return x


def _encoder64(enc, x, valid):
    import oracle
    layer = oracle.TransformerEncoderLayer(512, 8, dim_feedforward=512, dropout=0.1, activation="gelu")
    ref = oracle.TransformerEncoder(layer, len(enc.layers))
    ref.load_state_dict({k: v.detach().cpu() for k, v in enc.state_dict().items()})
    ref = ref.double().eval()
    with torch.no_grad():
        return ref(_d(x).transpose(0, 1), src_key_padding_mask=~valid.cpu()).transpose(0, 1) * valid.cpu().unsqueeze(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# consumers: (module, run() -> output on the GPU, ref() -> float64 output, launches that prove the cached path ran, single-launch path or None)
# ---------------------------------------------------------------------------------------------------------------------------------
def _linear():
    g = torch.Generator().manual_seed(1)
    mod = torch.nn.Linear(384, 256).to(DEV)
    x = torch.randn(64, 384, generator=g).to(DEV).to(torch.bfloat16)

    def run():
        from case_rg_amd import ops
        with torch.no_grad():
            return ops.linear(x, mod.weight, mod.bias).float()

    return mod, run, lambda: _d(x) @ _d(mod.weight).T + _d(mod.bias), {}, None


def _mha_views():
    from case_rg_amd.common.attention import MultiheadAttention
    g = torch.Generator().manual_seed(2)
    mod = MultiheadAttention(512, 8).to(DEV).eval()
    x = torch.randn(2, 16, 512, generator=g).to(DEV).to(torch.bfloat16)
    mem = torch.randn(2, 64, 512, generator=g).to(DEV).to(torch.bfloat16)
    valid = torch.ones(2, 64, dtype=torch.bool, device=DEV)
    valid[1, 40:] = False

    def run():  # the K/V rows (in_proj_weight[E:]) and the Q rows (in_proj_weight[:E]) as views of the packed parameter
        with torch.no_grad():
            return mod.cross_attention(x, None, valid, kv=mod.project_memory(mem)).float()

    return mod, run, lambda: _mha64(mod, x, mem, valid), {}, None


def _encoder_chain():
    import case_rg_amd
    from case_rg_amd.utils import fill_params
    ns = case_rg_amd.namespace()
    layer = ns.TransformerEncoderLayer(512, 8, dim_feedforward=512, dropout=0.1, activation="gelu")
    mod = fill_params(ns.TransformerEncoder(layer, 2), 71, gain=2.0).to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 100, 512, generator=g).to(DEV).to(torch.bfloat16)
    valid = torch.ones(3, 100, dtype=torch.bool, device=DEV)
    valid[2, 60:] = False

    def run():
        with torch.no_grad():
            return (mod.forward_batch_first(x, valid).float() * valid.unsqueeze(-1))

    def single():  # the single-launch path on the same weights: the yardstick of the chain's bf16 error (test_encoder_chain_gpu.py)
        from case_rg_amd import ops
        ops.ENCODER_CHAIN = "off"
        try:
            return run()
        finally:
            ops.ENCODER_CHAIN = "auto"

    return mod, run, lambda: _encoder64(mod, x, valid), {"case_encoder_chain": 3}, single


def _absorbed():
    from case_rg_amd.common.attention import MultiheadAttention
    g = torch.Generator().manual_seed(4)
    mod = MultiheadAttention(512, 8).to(DEV).eval()
    with torch.no_grad():
        mod.in_proj_bias.copy_(torch.randn(3 * 512, generator=g).to(DEV) * 0.2)
        mod.out_proj.bias.copy_(torch.randn(512, generator=g).to(DEV) * 0.2)
        mod.in_proj_weight.mul_(3.0)  # scores of a few units
    x = torch.randn(4, 1, 512, generator=g).to(DEV).to(torch.bfloat16)
    mem = torch.randn(4, 300, 512, generator=g).to(DEV).to(torch.bfloat16)
    valid = torch.ones(4, 300, dtype=torch.bool, device=DEV)
    valid[1, 200:] = False

    def run():
        with torch.no_grad():
            return mod.cross_attention_absorbed(x, mem, valid).float()

    return mod, run, lambda: _mha64(mod, x, mem, valid), {"case_attention_decode_mqa": 1}, None


def _highway():
    from case_rg_amd.common.Highway import Highway
    g = torch.Generator().manual_seed(5)
    mod = Highway(256, 256, num_layers=2).to(DEV)
    x = torch.randn(96, 256, generator=g).to(DEV).to(torch.bfloat16)

    def run():
        with torch.no_grad():
            return mod(x).float()

    return mod, run, lambda: _highway64(mod, x), {"case_highway_gate_fwd": 2}, None


def _training_forward():
    """A training forward (autograd on) whose weight operand comes from FusedAdam's persistent bf16 copy (seeded by the step)."""
    g = torch.Generator().manual_seed(6)
    mod = torch.nn.Linear(384, 256).to(DEV)
    x = torch.randn(64, 384, generator=g).to(DEV).to(torch.bfloat16)

    def run():
        from case_rg_amd import ops
        return ops.linear(x, mod.weight, mod.bias).detach().float()

    return mod, run, lambda: _d(x) @ _d(mod.weight).T + _d(mod.bias), {}, None


CONSUMERS = {"linear": _linear, "mha_views": _mha_views, "encoder_chain": _encoder_chain, "absorbed": _absorbed, "highway": _highway,
             "training_forward": _training_forward}


# ---------------------------------------------------------------------------------------------------------------------------------
# rewrite paths: each moves the parameters to other values (those of a twin filled from another seed, or an Adam step with a large lr)
# ---------------------------------------------------------------------------------------------------------------------------------
def _targets(mod):
    """Other values for every parameter of ``mod`` (the same on every call): xavier-uniform matrices at gain 2, 1-D weights 1 + U(-.2, .2),
    1-D biases U(-.2, .2)."""
    g = torch.Generator().manual_seed(9001)
    out = {}
    for n, p in mod.named_parameters():
        u = torch.rand(p.shape, generator=g, dtype=torch.float32) * 2 - 1
        if p.dim() > 1:
            t = u * 2.0 * math.sqrt(6.0 / (p.shape[0] + p.shape[1]))
        else:
            t = (1 + 0.2 * u) if n.endswith("weight") else 0.2 * u
        out[n] = t.to(p.device)
    return out


def _adam_step(mod, state):
    from case_rg_amd.optim import FusedAdam
    if "opt" not in state:
        state["opt"] = FusedAdam(mod.parameters(), lr=0.1, low_precision=torch.bfloat16)
    opt = state["opt"]
    g = torch.Generator().manual_seed(7)
    for p in mod.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    opt.zero_grad()


def _ema_swap(mod, state):
    from case_rg_amd.common.EMA import EMA
    ema = EMA(mod, 0.995)
    ema.shadow = {n: t.clone() for n, t in _targets(mod).items()}
    ema.apply_shadow()


def _ema_restore(mod, state):
    state["ema"].restore()


def _prepare_ema_restore(mod, state):
    from case_rg_amd.common.EMA import EMA
    ema = state["ema"] = EMA(mod, 0.995)
    ema.register()  # the current weights become the shadow ...
    ema.shadow = {n: t.clone() for n, t in _targets(mod).items()}
    ema.apply_shadow()  # ... and the consumer first runs on other weights; restore() brings the originals back


def _load_state_dict(mod, state):
    sd = mod.state_dict()
    sd.update({n: t.clone() for n, t in _targets(mod).items()})
    mod.load_state_dict(sd)


def _data_copy(mod, state):
    from case_rg_amd import ops
    t = _targets(mod)
    for n, p in mod.named_parameters():
        p.data.copy_(t[n])
    ops.invalidate_param_cache()  # the documented contract of writes through .data


def _data_assign(mod, state):
    from case_rg_amd import ops
    t = _targets(mod)
    for n, p in mod.named_parameters():
        p.data = t[n].clone()
    ops.invalidate_param_cache()


def _inplace_add(mod, state):
    t = _targets(mod)
    with torch.no_grad():
        for n, p in mod.named_parameters():
            p.add_(t[n] - p)  # moves _version: no invalidation needed


PATHS = {"adam": (None, _adam_step), "ema_swap": (None, _ema_swap), "ema_restore": (_prepare_ema_restore, _ema_restore),
         "load_state_dict": (None, _load_state_dict), "data_copy": (None, _data_copy), "data_assign": (None, _data_assign),
         "inplace_add": (None, _inplace_add)}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("consumer", list(CONSUMERS))
def test_consumer_reads_the_current_weights_after_a_rewrite(bf16_mode, consumer, path):
    from case_rg_amd import ops
    mod, run, ref, launches, single = CONSUMERS[consumer]()
    prepare, rewrite = PATHS[path]
    state = {}
    if consumer == "training_forward":
        _adam_step(mod, state)  # the operand copy is now the optimizer's persistent one
        assert ops.cast_param(mod.weight, torch.bfloat16).data_ptr() == state["opt"]._low[id(mod.weight)].data_ptr()
    if prepare is not None:
        prepare(mod, state)
    with _Counting() as c:
        run()
    for name, n in launches.items():
        assert c.calls.get(name, 0) == n, "%s: %d launches of %s, expected %d" % (consumer, c.calls.get(name, 0), name, n)
    before = ref()
    rewrite(mod, state)
    got = run()
    ops.invalidate_param_cache()
    cold = run()
    want = ref()
    torch.cuda.synchronize()
    moved = (want - before).abs().max().item() / max(want.abs().max().item(), before.abs().max().item())
    assert moved >= 10 * BAR, "the rewrite barely moved the float64 output (%.3e): the check would not see a stale copy" % moved
    assert torch.isfinite(got).all()
    e_cold, e_ref = _rel(got, cold), _rel(got, want)
    bar = BAR if single is None else max(BAR, 1.5 * _rel(single(), want))
    assert e_cold <= COLD, "%s after %s: %.3e from a cold cache (stale derived copy?)" % (consumer, path, e_cold)
    assert e_ref <= bar, "%s after %s: %.3e from float64 on the current weights (bar %.3e)" % (consumer, path, e_ref, bar)


def test_replay_leaves_the_step_kernel_count_and_reinstalls_the_low_copies(bf16_mode):
    """After a replay: no derived copy survives but the optimizer's bf16 copies, which are reinstalled as they are (no cast), and the
    next replay does not re-cast them either -- a replay gains no launch."""
    import case_rg_amd
    from case_rg_amd import config, ops, paramcache
    trainer, opt = _case_trainer(hidden=64, lr=1e-3)
    try:
        for s in range(4):  # two eager steps, the recording step, one replay
            trainer.train_batch(0, _batch(s, 64), "train", opt)
        assert trainer.graphs.replays == 2
        with torch.no_grad():
            trainer.model.eval()
            trainer.model(_batch(9, 64), method="test")
            trainer.model.train()
        bias = next(p for p in trainer.model.parameters() if p.dim() == 1)
        ops.cast_param(bias, torch.bfloat16)  # a cached copy of a parameter the optimizer keeps no bf16 copy of
        low = {id(v) for v in opt._low.values()}
        assert any(id(v) not in low for _, _, v in paramcache.entries("cast"))
        trainer.train_batch(0, _batch(4, 64), "train", opt)
        low = {id(v) for v in opt._low.values()}
        left = list(paramcache.entries())
        assert left and all(id(v) in low for _, _, v in left), "a derived copy survived the replay"
        assert not any(list(paramcache.entries(kind)) for kind in ("chain", "absorbed", "highway"))
        with _Counting() as c:
            trainer.train_batch(0, _batch(5, 64), "train", opt)
        assert trainer.graphs.replays == 4 and "case_cast" not in c.calls, c.calls
    finally:
        trainer.close()
        config.set_device_state(None)
        case_rg_amd.set_dropout(False)


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: CaSE, hidden 512, 8 heads, bf16, dropout on, captured steps; predict between replays without an EMA swap
# ---------------------------------------------------------------------------------------------------------------------------------
def _case_trainer(hidden, lr):
    import case_rg_amd
    from case_rg_amd.CaSE.Model import CaSE
    from case_rg_amd.common.CumulativeTrainer import CumulativeTrainer
    from case_rg_amd.optim import FusedAdam
    from case_rg_amd.utils import fill_params, make_vocab
    case_rg_amd.set_compute_dtype(torch.bfloat16)
    case_rg_amd.set_dropout(True)
    case_rg_amd.config.manual_seed(77)
    v2i, i2v = make_vocab(300)
    model = fill_params(CaSE(4, 6, i2v, v2i, hidden, enc_layers=2, dec_layers=2, heads=8), 21).train()
    trainer = CumulativeTrainer(model, None, None, 0, 1, capture=True)
    opt = FusedAdam(model.parameters(), lr=lr, low_precision=torch.bfloat16)
    return trainer, opt


def _batch(step, Lp=64, device=DEV):
    from case_rg_amd.utils import synth_batch
    b = synth_batch(2, 2, Lp, 16, 6, 300, seed=700 + step, ragged=False, model="case")
    return {k: v.to(device) for k, v in b.items()} if device is not None else b


def test_predict_between_replays_reads_the_replayed_weights(bf16_mode, monkeypatch):
    import case_rg_amd
    from case_rg_amd import config, ops, paramcache
    monkeypatch.setattr(ops, "DECODE_ABSORB_MIN_KEYS", 16)  # K21 on these small memories (16 query rows, 2 x 64 passage rows)
    trainer, opt = _case_trainer(hidden=512, lr=1e-2)
    data = _batch(50, device=None)

    def predict():
        with _Counting() as c:
            out = trainer.predict("test", [data], lambda xs: xs[0], 1)[0][1]
        trainer.model.train()
        return {k: v.detach().clone() for k, v in out.items()}, c.calls

    try:
        for s in range(4):  # two eager steps, the recording step, one replay
            trainer.train_batch(0, _batch(s), "train", opt)
        assert trainer.graphs.replays == 2
        first, calls = predict()
        assert calls.get("case_encoder_chain", 0) > 0 and calls.get("case_attention_decode_mqa", 0) > 0, calls
        for s in range(4, 6):
            trainer.train_batch(0, _batch(s), "train", opt)
        assert trainer.graphs.replays == 4
        second, _ = predict()
        # the derived copies the second predict read, against the same copies rebuilt from a cold cache
        by_owners = lambda kind: {tuple(map(id, owners)): v for owners, _, v in paramcache.entries(kind)}  # noqa: E731
        warm_packs = {k: v.clone() for k, v in by_owners("chain").items()}
        warm_folded = {k: {n: t.clone() for n, t in v.items()} for k, v in by_owners("absorbed").items()}
        ops.invalidate_param_cache()
        cold, _ = predict()
        cold_packs, cold_folded = by_owners("chain"), by_owners("absorbed")
    finally:
        trainer.close()
        config.set_device_state(None)
        case_rg_amd.set_dropout(False)
    assert warm_packs and sorted(warm_packs) == sorted(cold_packs)
    assert warm_folded and sorted(warm_folded) == sorted(cold_folded)
    for k, v in warm_packs.items():
        assert torch.equal(v, cold_packs[k]), "a chain pack outlived the replays"
    for owners, w in warm_folded.items():
        for k in w:
            assert torch.equal(w[k], cold_folded[owners][k]), "folded decode projection %s outlived the replays" % k
    moved = _rel(second["rank"], first["rank"])
    assert moved >= 10 * COLD, "two replays barely moved the passage scores (%.3e)" % moved
    assert torch.equal(second["answer"], cold["answer"]), "predict after replays decoded other tokens than from a cold cache"
    e = _rel(second["rank"], cold["rank"])
    assert e <= COLD, "predict after replays: %.3e from a cold cache (it read the previous predict's weights)" % e
