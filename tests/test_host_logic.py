"""Host-side logic that needs no GPU: batch schema, deterministic filler, module-attribute graph / state_dict
schema, helpers restated from common/Utils.py, LR schedule, dropout counter bookkeeping."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import oracle
from case_rg_amd import config
from case_rg_amd.utils import fill_params, make_vocab, synth_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_synth_batch_follows_the_collate_schema():
    b = synth_batch(3, 4, 16, 8, 6, 300, seed=1, model="case")
    assert b["query"].shape == (3, 1, 8) and b["passage"].shape == (3, 4, 16)
    assert b["source_map"].shape == (3, 8 + 4 * 16)
    assert torch.equal(b["source_map"], torch.cat([b["query"].reshape(3, -1), b["passage"].reshape(3, -1)], 1))
    assert (b["query"][:, 0, 0] == 101).all() and (b["passage"][:, :, 0] == 101).all()  # [CLS] first
    assert b["token_label"].shape == (3, 4, 16) and b["token_weight"].dtype == torch.float32
    assert ((b["token_label"] == 0) | (b["passage"] != 0)).all()
    last = b["response"].ne(0).sum(1) - 1
    assert (b["response"][torch.arange(3), last] == 2).all()  # ends with EOS
    assert "token_label" not in synth_batch(2, 2, 8, 4, 4, 300, model="masque")
    full = synth_batch(2, 3, 16, 8, 6, 300, ragged=False)
    assert (full["passage"] != 0).all() and (full["query"] != 0).all() and full["response"].shape == (2, 6)
    again = synth_batch(3, 4, 16, 8, 6, 300, seed=1, model="case")
    assert all(torch.equal(b[k], again[k]) for k in b)


def test_filler_is_name_keyed_and_alias_independent():
    v2i, i2v = make_vocab(200)
    a = fill_params(oracle.CaSE(4, 6, i2v, v2i, 32), 9)
    import case_rg_amd
    p = fill_params(case_rg_amd.namespace().CaSE(4, 6, i2v, v2i, 32), 9)
    sa, sp = a.state_dict(), p.state_dict()
    assert set(sa) == set(sp) and len(sa) == 1301
    for k in sa:
        assert torch.equal(sa[k], sp[k]), k
    # shared encoder: every alias sees the same tensor
    assert sp["query_encoder.embedding.0.weight"].data_ptr() == sp["response_generation.span_extraction.passage_selection.passage_encoder.embedding.0.weight"].data_ptr()
    other = fill_params(oracle.CaSE(4, 6, i2v, v2i, 32), 10)
    assert not torch.equal(other.state_dict()["passage_selection.scorer.weight"], sa["passage_selection.scorer.weight"])


def test_masque_schema_counts():
    import case_rg_amd
    v2i, i2v = make_vocab(200)
    m = case_rg_amd.namespace().Masque(6, i2v, v2i, 32)
    assert len(m.state_dict()) == 663 and len(list(m.parameters())) == 296
    assert hasattr(m, "do_infer") and hasattr(m, "do_ps_train")


def test_utils_restatements():
    from case_rg_amd.common import Utils
    from case_rg_amd.common.Constants import BOS_WORD, EOS_WORD, PAD_WORD, UNK_WORD
    v2i, i2v = make_vocab(200)
    ids = torch.tensor([[v2i[BOS_WORD], 110, 111, v2i[EOS_WORD], 112], [v2i[PAD_WORD], v2i[EOS_WORD], 5, 6, 7]])
    assert Utils.to_sentence(ids, i2v) == [["tok110", "tok111"], [UNK_WORD]]
    assert oracle.models.ids_to_tokens(ids, i2v) == Utils.to_sentence(ids, i2v)
    sents = [list("abcabc"), list("abcd")]
    Utils.remove_duplicate(sents)
    assert sents == [list("abc"), list("abcd")]
    assert Utils.neginf(torch.float32) == -1e20 and Utils.neginf(torch.float16) == -65504
    onehot = Utils.build_map(torch.tensor([[1, 3], [0, 2]]), max=4)
    assert torch.equal(onehot, oracle.build_map(torch.tensor([[1, 3], [0, 2]]), max=4))


def test_positional_table_matches_oracle():
    from case_rg_amd.common.PositionalEmbedding import sinusoid_table
    assert torch.allclose(sinusoid_table(50, 32), oracle.sinusoid_table(50, 32), atol=0, rtol=0)


def test_schedule_definition():
    from case_rg_amd.common.schedule import get_cosine_with_hard_restarts_schedule_with_warmup
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    sch = get_cosine_with_hard_restarts_schedule_with_warmup(opt, 10, 110)
    lrs = []
    for _ in range(111):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    assert lrs[0] == 0.0 and lrs[5] == pytest.approx(0.5) and lrs[10] == pytest.approx(1.0)
    assert lrs[60] == pytest.approx(0.5 * (1 + math.cos(math.pi * 0.5))) and lrs[110] == 0.0


def test_dropout_counter_bookkeeping():
    config.manual_seed(5)
    s0, o0, st0 = config.next_rng(100)
    s1, o1, st1 = config.next_rng(7)
    assert (s0, o0, s1, o1) == (5, 0, 5, 100) and st0 is None and st1 is None  # no device state: arguments only
    config.set_device_state(0x7f0000001000)
    # with a device-resident state the sites of a step are numbered from 0; the stream position moves into the base the kernels add
    assert config.next_rng(3) == (5, 0, 0x7f0000001000) and config.rng_state() == (5, 112)  # offsets stay even
    assert config.begin_step() == 112 and config.next_rng(10)[1] == 0
    config.skip_rng(6)  # a replayed capture consumed 6 counters
    assert config.rng_state() == (5, 128)
    config.set_device_state(None)
    assert config.next_rng(2) == (5, 128, None)
    config.set_dropout(False)
    assert config.drop_p(0.1, True) == 0.0
    config.set_dropout(True)
    assert config.drop_p(0.1, True) == pytest.approx(0.1) and config.drop_p(0.1, False) == 0.0
    config.set_dropout(False)
    with pytest.raises(ValueError):
        config.set_compute_dtype(torch.float16)


def _run_py(code, cwd="/tmp"):
    import subprocess
    import sys
    import textwrap
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], capture_output=True, text=True, cwd=cwd, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_install_dropin_standalone_aliases_whole_packages():
    """No reference tree on sys.path: ``common`` / ``CaSE`` / ``Masque`` resolve to this package (fresh interpreter)."""
    out = _run_py("""
        import sys
        sys.path.insert(0, %r)
        import case_rg_amd
        case_rg_amd.install_dropin()
        from CaSE.Model import CaSE
        from common.CumulativeTrainer import CumulativeTrainer, init_params
        from Masque.Model import Masque
        from common.Utils import build_map, to_sentence
        print(CaSE.__module__, Masque.__module__, CumulativeTrainer.__module__, build_map.__module__)
        """ % ROOT)
    assert out.split() == ["case_rg_amd.CaSE.Model", "case_rg_amd.Masque.Model", "case_rg_amd.common.CumulativeTrainer",
                           "case_rg_amd.common.Utils"]


# A stand-in for the reference tree: the package layout and the names its Run.py imports (CaSE/Run.py:1-11, Masque/Run.py:1-11), with
# bodies of its own.  The hot-path modules raise when imported, so a name install_dropin() fails to alias cannot go unnoticed.
_HOT = "raise ImportError('stand-in hot-path module: install_dropin() must alias it')\n"
_STANDIN = {
    "CaSE/CaSEDataset.py": "class CaSEDataset:\n    pass\n\n\ndef collate_fn(data):\n    return data\n",
    "CaSE/Model.py": _HOT,
    "Masque/MasqueDataset.py": "class MasqueDataset:\n    pass\n\n\ndef collate_fn(data):\n    return data\n",
    "Masque/Model.py": _HOT,
    "common/__init__.py": "",
    "common/Constants.py": "PAD_WORD = '[PAD]'\nBOS_WORD = '[CLS]'\nEOS_WORD = '[SEP]'\nUNK_WORD = '[UNK]'\n",
    "common/Utils.py": ("import torch\n\n\ndef bert_tokenizer(text):\n    return text.split()\n\n\ndef bert_detokenizer(tokens):\n"
                        "    return ' '.join(tokens)\n\n\ndef topk(gen_output, k=5, PAD=None, BOS=None, UNK=None):\n"
                        "    return torch.topk(gen_output, k, dim=1)\n\n\ndef build_map(b_map, max=None):\n    raise NotImplementedError\n\n\n"
                        "def init_seed(seed):\n    raise NotImplementedError\n"),
    "common/Generations.py": "from common.Utils import *\n\n\ndef greedy(model, data, vocab2id, max_len=20):\n    raise NotImplementedError\n",
    "Utils.py": "from common.Utils import *\n\n\ndef save_result(predictions, dataset, output_path):\n    raise NotImplementedError\n",
}
_STANDIN.update({"common/%s.py" % m: _HOT for m in ("TransformerBlock", "Interaction", "CumulativeTrainer", "TransformerSeqEncoderDecoder")})


@pytest.mark.parametrize("model", ["CaSE", "Masque"])
def test_install_dropin_under_the_reference_run_py_imports(model, tmp_path):
    """the import sequence of CaSE/Run.py:1-11 (Masque/Run.py:1-11) with install_dropin() in front,
    under the SURVEY 8(c) stubs for the three third-party modules the reference needs, against a stand-in tree with the
    reference's layout.  The tree's own dataset, tokenizer and result-writer names must keep resolving to ITS modules; the
    model, trainer and on-path helpers to the HIP path."""
    for rel, text in _STANDIN.items():
        (tmp_path / rel).parent.mkdir(parents=True, exist_ok=True)
        (tmp_path / rel).write_text(text)
    REF = str(tmp_path)
    ds = {"CaSE": "CaSEDataset", "Masque": "MasqueDataset"}[model]
    out = _run_py("""
        import sys, types, importlib.machinery, math, torch
        sys.dont_write_bytecode = True
        sys.path.insert(0, %r)
        sys.path.append(%r)                     # Run.py:3  sys.path.append('./') from the reference root
        for n in ("bcolz", "nltk", "transformers", "transformers.optimization"):
            m = types.ModuleType(n); m.__spec__ = importlib.machinery.ModuleSpec(n, loader=None); m.__all__ = []
            sys.modules[n] = m
        t = sys.modules["transformers"]; t.torch, t.math, t.__all__ = torch, math, ["torch", "math"]
        import case_rg_amd
        case_rg_amd.install_dropin()
        from {M}.{D} import *                   # Run.py:4
        from torch import optim
        from common.CumulativeTrainer import *  # :6
        import torch.backends.cudnn as cudnn
        import argparse
        from {M}.Model import *                 # :9
        from Utils import *                     # :10
        from transformers.optimization import *
        import common.TransformerBlock, common.Interaction, common.Constants, common.Generations
        names = dict(dataset={D}, collate_fn=collate_fn, bert_tokenizer=bert_tokenizer, bert_detokenizer=bert_detokenizer,
                     model={M}, trainer=CumulativeTrainer, init_params=init_params, save_result=save_result, init_seed=init_seed,
                     build_map=build_map, block=common.TransformerBlock.TransformerBlock, inter=common.Interaction.Interaction,
                     greedy=common.Generations.greedy)
        for k, v in names.items():
            print(k, v.__module__)
        print("constants", common.Constants.__file__)
        # the reference's own callers of topk (default k = 5, copy_topk, the baselines' decoders) still get ITS behaviour
        import common.Utils as CU
        x = torch.tensor([[0.1, 0.7, 0.06, 0.05, 0.04, 0.03, 0.02]])
        v5, i5 = CU.topk(x.clone())
        print("topk5", ",".join(str(int(i)) for i in i5[0]), tuple(v5.shape)[1])
        v1, i1 = CU.topk(x.clone(), k=1)
        print("topk1", int(i1[0, 0]), tuple(i1.shape)[1])
        """.replace("{M}", model).replace("{D}", ds) % (ROOT, REF))
    got = dict(line.split(None, 1) for line in out.strip().splitlines())
    hip = "case_rg_amd."
    assert got["topk5"] == "1,0,2,3,4 5" and got["topk1"] == "1 1"
    assert got["dataset"] == "%s.%s" % (model, ds) and got["collate_fn"] == "%s.%s" % (model, ds)
    assert got["bert_tokenizer"] == "common.Utils" and got["bert_detokenizer"] == "common.Utils"
    assert got["save_result"] == "Utils" and got["greedy"] == "common.Generations"
    assert got["constants"].startswith(REF)
    assert got["model"] == hip + model + ".Model"
    assert got["trainer"] == hip + "common.CumulativeTrainer" and got["init_params"] == hip + "common.CumulativeTrainer"
    assert got["init_seed"] == hip + "common.Utils" and got["build_map"] == hip + "common.Utils"
    assert got["block"] == hip + "common.TransformerBlock" and got["inter"] == hip + "common.Interaction"


def test_special_id_cache_follows_the_vocabulary_object():
    """to_sentence's BOS / PAD / EOS ids are remembered for the most recent vocabulary OBJECT (identity, not id())."""
    from case_rg_amd.common import Utils
    from case_rg_amd.common.Constants import BOS_WORD, EOS_WORD, PAD_WORD
    a = {0: PAD_WORD, 1: BOS_WORD, 2: EOS_WORD, 3: "x"}
    b = {0: "x", 5: PAD_WORD, 6: BOS_WORD, 7: EOS_WORD}
    assert Utils._specials(a) == (1, 0, 2)
    assert Utils._specials(b) == (6, 5, 7) and Utils._special_ids[0] is b
    assert Utils._specials(a) == (1, 0, 2)
    assert Utils._specials(["x", "y"]) == (-1, -1, -1)


def test_bench_gpus_flag_starts_the_ranks_itself_or_fails_loudly():
    """`python bench.py --gpus N` outside torch.distributed.run must not silently run one rank: it spawns the N
    ranks as a child process -- or, when the node has fewer GPUs, says so; and a WORLD_SIZE that contradicts --gpus is refused.
    Host-independent: more GPUs than any node has are asked for, and the devices are hidden from the child, so the
    "node shows N GPU(s)" branch is taken on every host.  (The spawn itself is rehearsed on the GPU box with CASE_BENCH_FORCE_SPAWN=1.)"""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HIP_VISIBLE_DEVICES"] = env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4096"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0 and "--gpus 4096" in (r.stderr + r.stdout) and "GPU(s)" in (r.stderr + r.stdout), r.stderr[-300:]
    env["WORLD_SIZE"] = "4"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=4" in (r.stderr + r.stdout), r.stderr[-300:]


def test_bench_flop_model_matches_the_survey():
    """20.06 TFLOP (3 encoder layers) / 21.53 TFLOP (6) forward at cfg 2."""
    import argparse
    import bench
    a = argparse.Namespace(batch=32, passages=10, passage_len=384, query_len=64, answer_len=40, hidden=512, vocab=30522,
                           enc_layers=3, model="case")
    assert bench.forward_flops(a) / 1e12 == pytest.approx(20.06, rel=0.03)
    a.enc_layers = 6
    assert bench.forward_flops(a) / 1e12 == pytest.approx(21.53, rel=0.03)



def test_bench_plain_run_is_lean_and_full_keeps_the_extras(monkeypatch):
    """A plain run measures the timed steps only; --full turns the roofline, north-star, decode-point and CPU-baseline legs back on
    (each still switched off by its --no-* flag); --steps below 1 is refused."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3"])
    a = bench.parse()
    assert a.steps == 3 and not a.full and a.dump_outputs is None
    assert a.no_roofline and a.no_north_star and a.no_decode_point and a.no_cpu_baseline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu-baseline"])
    a = bench.parse()
    assert not (a.no_roofline or a.no_north_star or a.no_decode_point) and a.no_cpu_baseline
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_bench_dump_outputs_writes_fixed_samples(tmp_path):
    """--dump-outputs: float64 stays float64, everything else becomes float32, and a long array or parameter is cut to the same
    seeded sample in every run."""
    import bench
    model = torch.nn.Sequential(torch.nn.Linear(200, 100), torch.nn.Linear(100, 3))
    s1, s2 = bench.param_sample(model), bench.param_sample(model)
    assert torch.equal(s1, s2) and s1.numel() == bench.DUMP_PER_PARAM + 100 + 300 + 3
    big = torch.arange(bench.DUMP_SAMPLE + 10, dtype=torch.float32).bfloat16()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"losses": torch.tensor([1.5, 2.5], dtype=torch.float64), "params": s1, "big": big,
                                               "ids": torch.arange(5)})
    for name, dtype, n in (("losses", np.float64, 2), ("params", np.float32, s1.numel()), ("big", np.float32, bench.DUMP_SAMPLE),
                           ("ids", np.float32, 5)):
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == dtype and x.shape == (n,) and np.array_equal(x, y), name


def test_split_k_heuristic_fills_whole_rounds():
    """Weight-gradient split-K: 256x256-eligible outputs fill rounds of 256 persistent workgroups, the rest rounds of 512."""
    from case_rg_amd import ops
    k = 122880  # B*P*Lp rows of cfg 2 are the reduction of every weight gradient
    for rows, cols in ((7680, 2560), (512, 512), (1536, 512), (2560, 2560), (1024, 512)):
        split = ops._split_for(rows, cols, k, 2)
        wgs = (rows // 256) * (cols // 256) * split
        assert wgs / (-(-wgs // 256) * 256.0) >= 0.92, (rows, cols, split)
        assert (k // 64) // split >= 8
    assert ops._split_for(512, 512, 1280, 2) == 4           # small output: 64 tiles of 64x64 x 4 splits = 256 workgroups, 5 K tiles each in LDS
    assert ops._split_for(512, 512, 2048, 2) == 4 and ops._split_for(1536, 512, 1280, 2) == 2
    assert ops._split_for(320, 512, 1280, 2) >= 5           # not a multiple of 64: 128x128 tiling, few K tiles per split
    assert ops._split_for(30522, 512, 1280, 2) <= 2         # 956 tiles already fill the chip
    assert ops._split_for(64, 64, 64, 4) == 1               # nothing to split


def test_lr_schedule_equals_the_installed_transformers_implementation():
    """CaSE/Run.py:28 takes get_cosine_with_hard_restarts_schedule_with_warmup from ``transformers`` (pinned 2.1.1, not in this image: SURVEY
    8c).  The image carries a later release of the same library; its implementation of the same function is the closest available pin of
    the restated formula: identical learning rates over warm-up, one and three cycles, and past the end (VERDICT r5 missing 8)."""
    transformers = pytest.importorskip("transformers")
    ref = getattr(transformers, "get_cosine_with_hard_restarts_schedule_with_warmup", None)
    if ref is None:
        pytest.skip("this transformers release has no get_cosine_with_hard_restarts_schedule_with_warmup")
    from case_rg_amd.common.schedule import get_cosine_with_hard_restarts_schedule_with_warmup as ours

    def trajectory(fn, **kw):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.SGD([p], lr=2.5e-4)
        sch = fn(opt, 20, 200, **kw)
        out = []
        for _ in range(260):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sch.step()
        return out

    for kw in ({}, {"num_cycles": 3}):
        a, b = trajectory(ref, **kw), trajectory(ours, **kw)
        assert max(abs(x - y) for x, y in zip(a, b)) <= 1e-12, kw


def test_device_state_is_refused_over_another_and_leaves_with_its_owner():
    import gc

    class Owner(object):
        pass

    config.set_device_state(None)
    owner = Owner()
    config.set_device_state(0x7f0000002000, owner=owner)
    config.set_device_state(0x7f0000002000)  # the same state again: a no-op
    with pytest.raises(RuntimeError, match="another device step state"):
        config.set_device_state(0x7f0000003000)
    assert config.device_state() == 0x7f0000002000
    del owner
    gc.collect()
    assert config.device_state() is None
    stale = Owner()
    config.set_device_state(0x7f0000002000, owner=stale)
    config.set_device_state(None)
    config.set_device_state(0x7f0000004000)
    del stale
    gc.collect()
    assert config.device_state() == 0x7f0000004000, "a finalizer of an earlier state must not detach a later one"
    config.set_device_state(None)


# ---------------------------------------------------------------------------------------------------------------------------------
# paramcache: the registry of weight-derived copies (CPU tensors; ``build`` callbacks that count their calls)
# ---------------------------------------------------------------------------------------------------------------------------------
class _Builds(object):
    def __init__(self):
        self.n = 0

    def __call__(self):
        self.n += 1
        return torch.full((1,), float(self.n))


@pytest.fixture()
def registry():
    from case_rg_amd import paramcache
    paramcache.rewritten()
    yield paramcache
    paramcache.rewritten()


def test_paramcache_serves_until_an_owner_moves(registry):
    p, build = torch.nn.Parameter(torch.ones(3, 4)), _Builds()
    first = registry.derived((p,), "x", build)
    assert registry.derived((p,), "x", build) is first and build.n == 1 and registry.peek((p,), "x") is first
    with torch.no_grad():
        p.mul_(2.0)  # in place: _version moves
    assert registry.peek((p,), "x") is None
    second = registry.derived((p,), "x", build)
    assert build.n == 2 and second is not first and registry.derived((p,), "x", build) is second
    p.data = torch.zeros(3, 4)  # storage swap: data_ptr moves, _version does not
    assert registry.peek((p,), "x") is None and registry.derived((p,), "x", build) is not second and build.n == 3
    third = registry.peek((p,), "x")
    p.data.mul_(3.0)  # silent: neither moves, so the registry has to be told
    assert registry.derived((p,), "x", build) is third and build.n == 3
    registry.rewritten()
    assert registry.peek((p,), "x") is None and registry.derived((p,), "x", build) is not third and build.n == 4


def test_paramcache_tracks_every_owner_and_keeps_none_in_place(registry):
    a, b, c = (torch.nn.Parameter(torch.ones(2, 2)) for _ in range(3))
    build = _Builds()
    for n, mover in enumerate((a, b, c)):
        value = registry.derived((a, b, c), "pack", build)
        assert registry.derived((a, b, c), "pack", build) is value and build.n == n + 1
        with torch.no_grad():
            mover.add_(1.0)
        assert registry.derived((a, b, c), "pack", build) is not value and build.n == n + 2, "one of several owners moved"
    build = _Builds()
    head, tail = registry.derived((None, a, b), "pack", build), registry.derived((a, b, None), "pack", build)
    assert build.n == 2 and head is not tail
    assert registry.derived((None, a, b), "pack", build) is head and registry.derived((a, b, None), "pack", build) is tail and build.n == 2
    assert registry.peek((a, None, b), "pack") is None and registry.peek((a, b), "pack") is None
    with torch.no_grad():
        b.add_(1.0)
    assert registry.peek((None, a, b), "pack") is None and registry.peek((a, b, None), "pack") is None


def test_paramcache_tags_do_not_collide(registry):
    p, one, two = torch.nn.Parameter(torch.ones(4, 4)), _Builds(), _Builds()
    x, y = registry.derived((p,), "one", one), registry.derived((p,), ("two", 0), two)
    assert x is not y and registry.derived((p,), "one", one) is x and registry.derived((p,), ("two", 0), two) is y
    assert (one.n, two.n) == (1, 1) and registry.peek((p,), ("two", 1)) is None
    assert [v for _, _, v in registry.entries("one")] == [x] and [v for _, _, v in registry.entries("two")] == [y]
    assert len(list(registry.entries())) == 2


def test_paramcache_forgets_dead_owners_and_is_not_fooled_by_a_recycled_id(registry):
    import gc
    build = _Builds()
    data, keep = torch.ones(5), torch.nn.Parameter(torch.ones(2))
    p = torch.nn.Parameter(data)
    registry.derived((p,), "x", build)
    registry.derived((keep, p), "y", build)
    dead_id = id(p)
    del p
    gc.collect()
    # new Parameters over the SAME storage (same data_ptr, _version 0, device) until one lands on the dead one's id(): only the weak
    # reference tells them apart
    held = []
    while len(held) < 1000 and (not held or id(held[-1]) != dead_id):
        held.append(torch.nn.Parameter(data))
    assert id(held[-1]) == dead_id, "the interpreter did not hand the id() out again: nothing was tested"
    assert any(None in owners for owners, _, _ in registry.entries("x"))  # dead, still listed: entries go at the next miss
    assert registry.peek((held[-1],), "x") is None and registry.peek((keep, held[-1]), "y") is None
    registry.derived((keep,), "z", build)
    assert sorted(tag for _, tag, _ in registry.entries()) == ["z"]


def test_paramcache_rewritten_keeps_the_optimizer_copies_where_cast_param_looks(registry):
    params = [torch.nn.Parameter(torch.ones(6, 4)), torch.nn.Parameter(torch.ones(4))]
    lows = [torch.zeros(6, 4, dtype=torch.bfloat16), torch.zeros(4, dtype=torch.bfloat16)]
    other, build = torch.nn.Parameter(torch.ones(3)), _Builds()
    registry.derived((other,), "chain", build)
    registry.derived(tuple(params), "highway", build)
    before = registry.EPOCH
    registry.rewritten(keep=zip(params, lows))
    assert registry.EPOCH == before + 1
    left = list(registry.entries())
    assert len(left) == 2 and {id(v) for _, _, v in left} == {id(t) for t in lows}
    for p, low in zip(params, lows):
        assert registry.peek((p,), registry.cast_tag(p, torch.bfloat16)) is low
        assert registry.peek((p,), registry.cast_tag(p.detach(), torch.bfloat16)) is low  # cast_param builds the tag from the detached view
    view = params[0][2:]  # a view of the first parameter: another geometry, another entry
    assert registry.peek((params[0],), registry.cast_tag(view, torch.bfloat16)) is None
    for n in range(3):
        registry.rewritten()
        assert registry.EPOCH == before + 2 + n and not list(registry.entries())
