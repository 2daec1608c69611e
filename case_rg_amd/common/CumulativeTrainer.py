"""Training / prediction loop (reference: common/CumulativeTrainer.py:13-156), same public API.

What is kept: constructor signature, ``train_batch`` / ``train_epoch`` / ``predict`` / ``serialize``, gradient
accumulation, clip-norm 1, optimizer -> EMA -> scheduler -> zero_grad order, DistributedSampler sharding, per-rank
prediction lists.  What differs (none of it changes the numbers):
  * data parallelism is ``case_rg_amd.parallel.GradSync`` (bucketed RCCL all-reduce overlapped with backward) instead of
    a DistributedDataParallel wrapper, so ``self.model`` stays the bare module and ``serialize`` also works on one GPU / CPU
    (the reference crashes on ``self.model.module`` there);
  * the per-loss ``.cpu().item()`` (3 device->host syncs per step, :57) is one stacked copy;
  * batches are uploaded one ahead on a side stream from pinned memory (``utils.pipeline.DevicePrefetcher``)
    instead of blocking ``.cuda()`` calls inside the step;
  * ``save_checkpoint`` / ``load_checkpoint`` write what a resume needs next to the reference's weights-only
    ``<epoch>.pkl`` (:80-86): optimizer moments + step, scheduler, EMA shadow, the accumulation counter and the RNG streams.
"""
import math
import os
import sys
import time

import torch
import torch.distributed as dist
from torch.utils.data.distributed import DistributedSampler

from .. import config, ops
from ..optim import FusedAdam
from ..parallel import GradSync
from ..utils.pipeline import DevicePrefetcher
from .EMA import EMA


def init_params(model, escape=None):
    """xavier-uniform on every parameter with dim > 1, embedding row 0 included (reference :13-24)."""
    for name, param in model.named_parameters():
        if escape is not None and escape in name:
            continue
        if param.data.dim() > 1:
            torch.nn.init.xavier_uniform_(param.data)
    if hasattr(model, 'reset_parameters'):
        model.reset_parameters()
    ops.invalidate_param_cache()  # writes through .data leave _version alone


class CumulativeTrainer(object):
    def __init__(self, model, tokenizer, detokenizer, local_rank, num_gpus, accumulation_steps=1, ema_rate=0.995, capture=None):
        """``capture`` (not in the reference; True / False / "auto"; default: environment CASE_STEP_GRAPH = 1 / 0 / auto): replay the training step from a hipGraph
        recorded after two eager steps per batch shape (``case_rg_amd.stepgraph``) -- for the geometries whose step is launch-bound
        (the reference's default: hidden 256, batch 16).  The per-step scalars then live in device memory (``self.step_state``)."""
        self.local_rank = local_rank
        self.num_gpus = num_gpus
        self.tokenizer = tokenizer
        self.detokenizer = detokenizer
        if local_rank is not None and torch.cuda.is_available():
            torch.cuda.set_device(local_rank)
        self.model = model.cuda() if torch.cuda.is_available() else model
        self.accumulation_steps = accumulation_steps
        self.accumulation_count = 0
        # CASE_FORCE_GRADSYNC: keep the bucket / hook / collective machinery live on a one-rank group (one-GPU rehearsal of the DP path)
        self.sync = (GradSync(self.model, force=bool(os.environ.get("CASE_FORCE_GRADSYNC")))
                     if dist.is_available() and dist.is_initialized() else None)
        self.ema = EMA(self.model, ema_rate)
        self.ema.register()
        self._loss_host = None
        if capture is None:
            env = os.environ.get("CASE_STEP_GRAPH", "0")
            capture = "auto" if env == "auto" else env == "1"
        self.step_state, self.graphs = None, None
        if capture and torch.cuda.is_available():
            from ..stepgraph import StepGraphs
            from ..stepstate import StepState
            self.step_state = StepState(next(self.model.parameters()).device)
            # every dropout site from here on adds the device-resident base (detached again by close(), or when the state is collected)
            config.set_device_state(self.step_state.address, owner=self.step_state)
            self.graphs = StepGraphs(self, auto=capture == "auto")  # "auto": a capture is kept only where its replay is faster than the eager step

    def close(self):
        """Detach the device-resident step state from the process-wide dropout configuration (a capturing trainer owns it)."""
        if self.step_state is not None and config.device_state() == self.step_state.address:
            config.set_device_state(None)
        self.step_state, self.graphs = None, None

    def train_batch(self, epoch, data, method, optimizer, scheduler=None):
        try:
            return self._train_batch(epoch, data, method, optimizer, scheduler)
        except Exception:
            # the step died between backward and finish(): release what GradSync holds (reserved CUs, bucket counters).  Only for ordinary
            # exceptions -- a KeyboardInterrupt / SystemExit must not wait on collectives whose peers may be gone -- and a failure inside
            # abort() is reported but never replaces the error that ended the step.  Recovery after a ONE-rank failure is not supported:
            # the other ranks are blocked in their collectives until the process group's timeout.
            if self.sync is not None:
                try:
                    self.sync.abort()
                except Exception as cleanup:  # noqa: BLE001
                    print("CumulativeTrainer: GradSync.abort() failed while handling the step's error: %r" % (cleanup,), file=sys.stderr)
            raise

    def _train_batch(self, epoch, data, method, optimizer, scheduler=None):
        if self.graphs is not None:
            losses = self.graphs.run(epoch, data, method, optimizer, scheduler)
            if losses is not None:
                self.accumulation_count += 1
                return losses
            t0 = time.perf_counter()
            losses = self._eager_batch(epoch, data, method, optimizer, scheduler)
            self.graphs.note_eager_ms((time.perf_counter() - t0) * 1e3)
            return losses
        return self._eager_batch(epoch, data, method, optimizer, scheduler)

    def _eager_batch(self, epoch, data, method, optimizer, scheduler=None):
        self.accumulation_count += 1
        boundary = self.accumulation_count % self.accumulation_steps == 0
        if self.sync is not None:
            self.sync.no_sync(not boundary)
        state = self.step_state if isinstance(optimizer, FusedAdam) else None
        if self.step_state is not None:
            # device-resident step scalars: the dropout sites of this step are numbered from 0 and add the base uploaded here -- the
            # same numbering a replayed capture of the step uses
            base = config.begin_step()
            if state is not None and boundary:
                optimizer.stage_step(state)
            self.step_state.upload(base)
        loss = self.model(data, method=method)
        if isinstance(loss, (tuple, list)):
            parts = torch.cat([l.mean().reshape(1) for l in loss])
        else:
            parts = loss.mean().reshape(1)
        (parts.sum() / self.accumulation_steps).backward()
        # the losses go to a pinned buffer without blocking; the host waits for them only AFTER the all-reduce wait and the
        # optimizer kernels are enqueued (round 3 drained the device here, in the middle of the step, before enqueueing them)
        host, done = None, None
        if parts.is_cuda:
            if self._loss_host is None or self._loss_host.numel() < parts.numel():
                self._loss_host = torch.empty(max(8, parts.numel()), dtype=torch.float32).pin_memory()
            host = self._loss_host[:parts.numel()]
            host.copy_(parts.detach().float(), non_blocking=True)
            done = torch.cuda.Event()
            done.record()
        if boundary:
            if self.sync is not None:
                self.sync.finish()
            if isinstance(optimizer, FusedAdam):  # clip + Adam + EMA + bf16 operand refresh in one multi-tensor pass (K15)
                optimizer.step(clip_norm=1.0, ema=self.ema, state=state)
            else:
                torch.nn.utils.clip_grad_norm_(self.model.parameters(), 1)
                optimizer.step()
                ops.invalidate_param_cache()  # optimizers that write through p.data leave _version alone
                self.ema.update()
            if scheduler is not None:
                scheduler.step()
            optimizer.zero_grad()
        if host is None:
            return parts.detach().cpu().tolist()
        done.synchronize()
        return host.tolist()

    def serialize(self, epoch, output_path):
        if self.local_rank not in (0, None):
            return
        output_path = os.path.join(output_path, 'model/')
        os.makedirs(output_path, exist_ok=True)
        torch.save(self.model.state_dict(), os.path.join(output_path, '.'.join([str(epoch), 'pkl'])))

    def save_checkpoint(self, epoch, output_path, optimizer, scheduler=None):
        """Resumable state of the loop after ``epoch``: ``<output_path>/model/<epoch>.ckpt`` (rank 0 only, like serialize)."""
        if self.local_rank not in (0, None):
            return None
        output_path = os.path.join(output_path, 'model/')
        os.makedirs(output_path, exist_ok=True)
        state = {
            'epoch': epoch,
            'model': self.model.state_dict(),
            'optimizer': optimizer.state_dict(),
            'scheduler': None if scheduler is None else scheduler.state_dict(),
            'ema_shadow': dict(self.ema.shadow),
            'ema_decay': self.ema.decay,
            'accumulation_count': self.accumulation_count,
            'rng': {'torch': torch.get_rng_state(), 'dropout_counter': config.rng_state(),
                    'cuda': torch.cuda.get_rng_state() if torch.cuda.is_available() else None},
        }
        path = os.path.join(output_path, '.'.join([str(epoch), 'ckpt']))
        torch.save(state, path)
        return path

    def load_checkpoint(self, path, optimizer, scheduler=None):
        """Restore everything ``save_checkpoint`` wrote (every rank loads the same file); returns the epoch it was taken after."""
        device = next(self.model.parameters()).device
        state = torch.load(path, map_location=device, weights_only=False)
        self.model.load_state_dict(state['model'], strict=True)
        optimizer.load_state_dict(state['optimizer'])
        if scheduler is not None and state['scheduler'] is not None:
            scheduler.load_state_dict(state['scheduler'])
        named = dict(self.model.named_parameters())
        if set(state['ema_shadow']) != set(self.ema.shadow):
            raise RuntimeError('checkpoint EMA shadow does not match the model\'s trainable parameters')
        self.ema.shadow = {n: t.to(named[n].device, copy=True) for n, t in state['ema_shadow'].items()}
        self.ema.decay = state['ema_decay']
        self.accumulation_count = state['accumulation_count']
        torch.set_rng_state(state['rng']['torch'].cpu())
        if state['rng']['cuda'] is not None and torch.cuda.is_available():
            torch.cuda.set_rng_state(state['rng']['cuda'].cpu())
        config.set_rng_state(state['rng']['dropout_counter'])
        if self.graphs is not None:
            self.graphs.reset()  # the captures read tensors this load replaced (EMA shadows, optimizer moments)
        ops.invalidate_param_cache()  # load_state_dict copies in place under no_grad: cached bf16 operand copies are stale
        return state['epoch']

    def _loader(self, dataset, collate_fn, batch_size, shuffle, epoch=None):
        if dist.is_available() and dist.is_initialized():
            sampler = DistributedSampler(dataset, shuffle=shuffle)
            if epoch is not None:
                sampler.set_epoch(epoch)
            return torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, sampler=sampler, pin_memory=True)
        return torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, shuffle=shuffle,
                                           pin_memory=torch.cuda.is_available())

    def train_epoch(self, method, train_dataset, train_collate_fn, batch_size, epoch, optimizer, scheduler=None):
        self.model.train()
        loader = self._loader(train_dataset, train_collate_fn, batch_size, True, epoch)
        start, count, bloss = time.time(), 0, 0

        def report():
            msg = ['Method', method, 'Epoch', epoch, 'Batch ', count, 'Loss ', bloss, 'Time ', time.time() - start]
            if scheduler is not None:
                msg += ['Learning rate ', scheduler.get_last_lr()]
            print(*msg)
            sys.stdout.flush()

        for j, data in enumerate(DevicePrefetcher(loader), 0):  # batch j+1 is uploaded on a side stream while j computes (f3)
            count += 1
            bloss = self.train_batch(epoch, data, method=method, optimizer=optimizer, scheduler=scheduler)
            if j > 0 and j % 100 == 0:
                report()
        if self.accumulation_count % self.accumulation_steps != 0:  # flush a partial group (no clip / EMA, reference :122-126)
            if self.sync is not None:
                self.sync.no_sync(False)
                self.sync.finish()
            optimizer.step()
            ops.invalidate_param_cache()
            if scheduler is not None:
                scheduler.step()
            optimizer.zero_grad()
        report()

    def predict(self, method, dataset, collate_fn, batch_size):
        self.model.eval()
        rs = []
        with torch.no_grad():
            for data in DevicePrefetcher(self._loader(dataset, collate_fn, batch_size, False)):
                rs.append([data, self.model(data, method=method)])
        return rs

    def evaluate_nll(self, dataset, collate_fn, batch_size):
        """Teacher-forced negative log-likelihood of ``dataset``'s responses (``model(data, method='score')`` per batch): dict(nll = the
        token-weighted corpus mean of the batches' ``loss``, perplexity = exp(nll), tokens = the non-PAD targets counted).  One process, under
        no_grad in eval mode; the model's mode is restored afterwards."""
        was_training = self.model.training
        self.model.eval()
        total, tokens = None, None
        try:
            with torch.no_grad():
                loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, shuffle=False,
                                                     pin_memory=torch.cuda.is_available())
                for data in DevicePrefetcher(loader):
                    out = self.model(data, method='score')
                    part, n = out['loss'].double().sum() * out['tokens'], out['tokens']
                    total, tokens = (part, n) if total is None else (total + part, tokens + n)
        finally:
            self.model.train(was_training)
        if total is None or int(tokens) == 0:
            return dict(nll=float('nan'), perplexity=float('nan'), tokens=0)
        nll = float(total) / int(tokens)  # (the one read-back of the evaluation)
        return dict(nll=nll, perplexity=math.exp(nll), tokens=int(tokens))

    def evaluate_rouge(self, dataset, collate_fn, batch_size, method='test', references='response', remove_duplicates=False, orders=()):
        """ROUGE-L of ``model(data, method)['answer']`` against ``data[references]`` (int64 [B, T'] or [B, M, T'], all-PAD rows = no ground truth
        there) without building a Python string: ``evaluation.eval_rouge_l_ids`` per batch, the sum kept on the device, one read-back at the
        end -> dict(rouge_l = the mean of the per-item best F x 100 rounded to 2 decimals -- ``evaluation.eval_rouge_l``'s number for
        ``predict`` + ``to_sentence`` --, items = the items counted).  ``remove_duplicates``: the answers go through the reference's
        ``remove_duplicate`` on the device first (K33): the number ``Run_Evaluation`` prints for ``save_result``'s answers.  One process, under no_grad in eval mode; the model's mode is restored
        afterwards.  ``orders``: ROUGE-N orders in 1..4 to report beside it from the same decoding pass, e.g. ``(1, 2)`` adds ``rouge_1`` and
        ``rouge_2`` (``evaluation.eval_rouge_n_ids``: K34 + K43 + K44; ``evaluation.eval_rouge``'s ROUGE_1_F1 / ROUGE_2_F1), summed on the
        device and rounded as ``rouge_l`` is; an order outside 1..4 is a ``ValueError`` before anything is decoded.  The default adds nothing."""
        from ..evaluation.rouge_ids import eval_rouge_l_ids, model_specials
        from ..evaluation.rouge_n_ids import check_orders, eval_rouge_n_ids
        orders = check_orders(orders, "evaluate_rouge")
        was_training = self.model.training
        self.model.eval()
        specials = model_specials(self.model.vocab2id)
        total, items = None, 0
        try:
            with torch.no_grad():
                loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, shuffle=False,
                                                     pin_memory=torch.cuda.is_available())
                for data in DevicePrefetcher(loader):
                    out = self.model(data, method=method)
                    part = eval_rouge_l_ids(out['answer'], data[references], specials, remove_duplicates).sum()
                    if orders:
                        by_order = eval_rouge_n_ids(out['answer'], data[references], specials, orders, remove_duplicates).sum(dim=0)
                        part = torch.cat([part.view(1), by_order])
                    total = part if total is None else total + part
                    items += out['answer'].shape[0]
        finally:
            self.model.train(was_training)
        names = tuple('rouge_%d' % k for k in orders)
        if items == 0:
            return dict({name: float('nan') for name in ('rouge_l',) + names}, items=0)
        if not orders:
            return dict(rouge_l=round(float(total) / items, 2), items=items)  # (the one read-back of the evaluation)
        sums = total.tolist()  # (the one read-back of the evaluation)
        return dict({name: round(s / items, 2) for name, s in zip(('rouge_l',) + names, sums)}, items=items)

    def evaluate_bleu(self, dataset, collate_fn, batch_size, method='test', references='response', remove_duplicates=False):
        """BLEU of ``model(data, method)['answer']`` against ``data[references]`` (as ``evaluate_rouge`` takes them), without building a Python
        string: ``evaluation.eval_bleu_ids`` per batch (K34 + K35: nltk's ``sentence_bleu`` with default arguments, all present ground truths
        of an item as its references), the sum kept on the device, one read-back at the end -> dict(bleu = the mean of the per-item BLEU x 100
        rounded to 2 decimals -- ``evaluation.eval_bleu``'s number for ``predict`` + ``to_sentence``, what the reference's ``eval_bleu_file``
        prints for the same tokens --, items = the items counted).  ``remove_duplicates`` as in ``evaluate_rouge``.  One process, under no_grad
        in eval mode; the model's mode is restored afterwards."""
        from ..evaluation.ngram_ids import eval_bleu_ids
        from ..evaluation.rouge_ids import model_specials
        was_training = self.model.training
        self.model.eval()
        specials = model_specials(self.model.vocab2id)
        total, items = None, 0
        try:
            with torch.no_grad():
                loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, shuffle=False,
                                                     pin_memory=torch.cuda.is_available())
                for data in DevicePrefetcher(loader):
                    out = self.model(data, method=method)
                    part = eval_bleu_ids(out['answer'], data[references], specials, remove_duplicates=remove_duplicates).sum()
                    total = part if total is None else total + part
                    items += out['answer'].shape[0]
        finally:
            self.model.train(was_training)
        if items == 0:
            return dict(bleu=float('nan'), items=0)
        return dict(bleu=round(float(total) / items, 2), items=items)  # (the one read-back of the evaluation)

    def evaluate_meteor(self, dataset, collate_fn, batch_size, method='test', references='response', remove_duplicates=False, classes=None):
        """METEOR of ``model(data, method)['answer']`` against ``data[references]`` (as ``evaluate_rouge`` takes them), without building a Python
        string: ``evaluation.eval_meteor_ids`` per batch (K40: nltk's ``meteor_score`` with default parameters, its exact stage on ids and
        ``classes`` -- an int32 [V] table id -> equivalence class, None: exact matches only -- in place of its stem and synonym stages; the
        best score over the present ground truths of an item), the sum kept on the device, one read-back at the end -> dict(meteor = the
        mean of the per-item METEOR x 100 rounded to 2 decimals -- ``evaluation.eval_meteor``'s number for ``predict`` + ``to_sentence``, what
        the reference's ``eval_meteor_file`` prints for the same tokens and the same stages --, items = the items counted).
        ``remove_duplicates`` as in ``evaluate_rouge``.  One process, under no_grad in eval mode; the model's mode is restored afterwards."""
        from ..evaluation.meteor_ids import eval_meteor_ids
        from ..evaluation.rouge_ids import model_specials
        was_training = self.model.training
        self.model.eval()
        specials = model_specials(self.model.vocab2id)
        total, items = None, 0
        try:
            with torch.no_grad():
                loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, shuffle=False,
                                                     pin_memory=torch.cuda.is_available())
                for data in DevicePrefetcher(loader):
                    out = self.model(data, method=method)
                    if classes is not None and classes.device != out['answer'].device:
                        classes = classes.to(out['answer'].device)
                    part = eval_meteor_ids(out['answer'], data[references], specials, classes, remove_duplicates=remove_duplicates).sum()
                    total = part if total is None else total + part
                    items += out['answer'].shape[0]
        finally:
            self.model.train(was_training)
        if items == 0:
            return dict(meteor=float('nan'), items=0)
        return dict(meteor=round(float(total) / items, 2), items=items)  # (the one read-back of the evaluation)

    GENERATION_METRICS = ('rouge_l', 'bleu', 'meteor')  # evaluate_generation's default
    ROUGE_N_METRICS = {'rouge_1': 1, 'rouge_2': 2}      # further names it takes: the other two ROUGE figures of Run_Evaluation's line

    def evaluate_generation(self, dataset, collate_fn, batch_size, method='test', references='response', remove_duplicates=False,
                            metrics=GENERATION_METRICS, classes=None):
        """The answer-quality line of ``Run_Evaluation`` from ONE decoding pass: per batch ``model(data, method)`` runs once and every metric
        named in ``metrics`` ('rouge_l', 'bleu', 'meteor') is computed from that pass's ``answer`` with the per-item function its
        single-metric method uses (``eval_rouge_l_ids``, ``eval_bleu_ids``, ``eval_meteor_ids``), the sums kept on the device, one read-back
        at the end -> dict(one entry per named metric, rounded exactly as ``evaluate_rouge`` / ``evaluate_bleu`` / ``evaluate_meteor`` round
        it, items = the items counted).  ``metrics`` may also name 'rouge_1' and 'rouge_2' (``eval_rouge_n_ids``, rounded as
        ``evaluate_rouge(orders=...)`` rounds them): with 'rouge_l' the three ROUGE figures of the reference's ``eval_rouge``.  An unknown
        metric name is a ``ValueError`` before anything is decoded.  ``remove_duplicates`` and ``classes`` as in those methods.  One process, under no_grad in eval mode; the model's mode is restored afterwards."""
        from ..evaluation.meteor_ids import eval_meteor_ids
        from ..evaluation.ngram_ids import eval_bleu_ids
        from ..evaluation.rouge_ids import eval_rouge_l_ids, model_specials
        from ..evaluation.rouge_n_ids import eval_rouge_n_ids
        metrics = (metrics,) if isinstance(metrics, str) else tuple(metrics)
        known = self.GENERATION_METRICS + tuple(self.ROUGE_N_METRICS)
        unknown = [name for name in metrics if name not in known]
        if unknown or not metrics:
            raise ValueError("evaluate_generation: metrics must name some of %s, not %r" % (known, metrics))
        was_training = self.model.training
        self.model.eval()
        specials = model_specials(self.model.vocab2id)
        per_item = dict(rouge_l=lambda hyp, ref: eval_rouge_l_ids(hyp, ref, specials, remove_duplicates),
                        bleu=lambda hyp, ref: eval_bleu_ids(hyp, ref, specials, remove_duplicates=remove_duplicates),
                        meteor=lambda hyp, ref: eval_meteor_ids(hyp, ref, specials, classes, remove_duplicates=remove_duplicates))
        orders = tuple(sorted({self.ROUGE_N_METRICS[name] for name in metrics if name in self.ROUGE_N_METRICS}))
        total, items = None, 0
        try:
            with torch.no_grad():
                loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, shuffle=False,
                                                     pin_memory=torch.cuda.is_available())
                for data in DevicePrefetcher(loader):
                    out = self.model(data, method=method)
                    if classes is not None and classes.device != out['answer'].device:
                        classes = classes.to(out['answer'].device)
                    if orders:  # (the named ROUGE-N orders share one K34 + K43 + K44 sequence)
                        by_order = eval_rouge_n_ids(out['answer'], data[references], specials, orders, remove_duplicates).sum(dim=0)
                    part = torch.stack([by_order[orders.index(self.ROUGE_N_METRICS[name])] if name in self.ROUGE_N_METRICS
                                        else per_item[name](out['answer'], data[references]).sum() for name in metrics])
                    total = part if total is None else total + part
                    items += out['answer'].shape[0]
        finally:
            self.model.train(was_training)
        if items == 0:
            return dict({name: float('nan') for name in metrics}, items=0)
        sums = total.tolist()  # (the one read-back of the evaluation)
        return dict({name: round(s / items, 2) for name, s in zip(metrics, sums)}, items=items)

    def evaluate_rank(self, dataset, collate_fn, batch_size, method='rank', labels='passage_label', keys=None, valid=None):
        """The TREC ranking metrics of ``model(data, method)['rank']`` [B, P] against ``data[labels]`` (int64 [B]: the index of the gold
        passage; or an integer [B, P] tensor of grades), every item its own query: ``evaluation.eval_rank_ids`` per batch (K36), the column
        sums kept on the device, one read-back at the end -> dict(map, ndcg, recall_5 .. recall_1000, recip_rank, P_1 = the plain means over
        the items, unrounded f64 -- what the reference's ``eval_trec_file`` prints for the run ``save_result`` writes, plus recip_rank and
        P_1 --, items = the items counted).  ``method="rank"`` stops after the selection stage; any method whose result carries ``rank`` may
        be named.  ``keys`` / ``valid`` name optional ``data`` entries (tie keys, the larger first; which slots hold a passage).  One
        process, under no_grad in eval mode; the model's mode is restored afterwards."""
        from .. import ops
        from ..evaluation.rank_ids import eval_rank_ids
        was_training = self.model.training
        self.model.eval()
        total, items = None, 0
        try:
            with torch.no_grad():
                loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, shuffle=False,
                                                     pin_memory=torch.cuda.is_available())
                for data in DevicePrefetcher(loader):
                    rank = self.model(data, method=method)['rank']
                    part = eval_rank_ids(rank, data[labels], None if keys is None else data[keys], None if valid is None else data[valid])
                    total = part if total is None else total + part
                    items += rank.shape[0]
        finally:
            self.model.train(was_training)
        if items == 0:
            return dict({name: float('nan') for name in ops.RANK_METRICS}, items=0)
        sums = total.tolist()  # (the one read-back of the evaluation)
        return dict({name: s / items for name, s in zip(ops.RANK_METRICS, sums)}, items=items)

    def evaluate_attribution(self, dataset, collate_fn, batch_size, answers="test", labels="passage_label", **decode):
        """Does the model cite the gold passage?  ``model.do_attribute(data, answers, **decode)`` per batch, the sums of
        ``evaluation.attribution_ids``' columns (slot 0 of every item's pool) kept on the device, one read-back at the end ->
        dict(cited_accuracy = the items whose ``cited`` passage is ``data[labels]`` / items -- an item that cites nothing (cited -1) is a
        miss --, rank_agreement = the items whose cited passage is the one the selection stage ranks first / items, gen_share /
        context_share / passage_share = the generator's, the conversation context's and all passages' shares of the answers' probability,
        token-weighted micro-averages, items, tokens = the non-PAD answer tokens counted).  One process, under no_grad in eval mode; the
        model's mode is restored afterwards."""
        from ..evaluation.attribution import ATTRIBUTION_COLUMNS, eval_attribution_ids
        was_training = self.model.training
        self.model.eval()
        total, items = None, 0
        try:
            with torch.no_grad():
                loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, shuffle=False,
                                                     pin_memory=torch.cuda.is_available())
                for data in DevicePrefetcher(loader):
                    part = eval_attribution_ids(self.model.do_attribute(data, answers=answers, **decode), data[labels])
                    total = part if total is None else total + part
                    items += data[labels].shape[0]
        finally:
            self.model.train(was_training)
        names = ("cited_accuracy", "rank_agreement", "gen_share", "context_share", "passage_share")
        if items == 0:
            return dict({name: float('nan') for name in names}, items=0, tokens=0)
        sums = dict(zip(ATTRIBUTION_COLUMNS, total.tolist()))  # (the one read-back of the evaluation)
        ratio = lambda a, b: a / b if b else 0.0  # noqa: E731
        tokens = int(sums["tokens"])
        return dict(cited_accuracy=sums["cited_hit"] / items, rank_agreement=sums["rank_agree"] / items,
                    gen_share=ratio(sums["gen_share"], tokens), context_share=ratio(sums["context_share"], tokens),
                    passage_share=ratio(sums["passage_share"], tokens), items=items, tokens=tokens)

    def evaluate_extract(self, dataset, collate_fn, batch_size, top_k=None, select="prior", labels="token_label", ranking=False):
        """Token-level metrics of the supporting-token stage: ``model.do_extract(data, top_k, select, labels=data[labels])`` per batch (K38
        counts the items while it selects their tokens), the column sums kept on the device, one read-back at the end -> dict(precision =
        tp / n_pred and recall = tp / n_pos of the tokens whose logit is positive, f1 = their harmonic mean, precision_at_k = hits /
        sum of min(K, n_valid) and recall_at_k = hits / n_pos of the K tokens ``select`` ranks first, items, tokens = the non-PAD tokens
        counted); micro-averages over tokens, 0.0 where a denominator is 0.  Where ``data`` lacks ``labels`` they come from
        ``model.label_batch(data)`` (K37; ``set_token_freq`` first).  ``ranking=True`` (K45, one more launch per batch, on the key
        ``select`` names) adds the threshold-free figures of ``evaluation.token_rank``: map = the mean AP over the items with a positive
        (ranked_items), auc = the mean AUC over the items with both classes (auc_items), auc_stratified = sum auc_num2 / sum 2 n_pos n_neg
        (the within-item pair-weighted figure), oracle_f1 = 2 sum best_tp / sum (best_n + n_pos) (the pooled F1 when every item is cut
        where its own F1 peaks: no threshold does better on any single item); their sums ride in f64 beside the counts, so the evaluation
        keeps its one read-back.  One process, under no_grad in eval mode; the model's mode is restored afterwards."""
        from ..evaluation.token_rank import rank_sums, summarize_rank
        was_training = self.model.training
        self.model.eval()
        total, rank_total, items = None, None, 0
        try:
            with torch.no_grad():
                loader = torch.utils.data.DataLoader(dataset, collate_fn=collate_fn, batch_size=batch_size, shuffle=False,
                                                     pin_memory=torch.cuda.is_available())
                for data in DevicePrefetcher(loader):
                    gold = data[labels] if labels in data else self.model.label_batch(data)['token_label']
                    got = self.model.do_extract(data, top_k=top_k, select=select, labels=gold, ranking=ranking)
                    counts = got['counts'].long()
                    K = self.model.support_top_k if top_k is None else int(top_k)
                    part = torch.cat([counts.sum(0), counts[:, 0].clamp(max=K).sum().reshape(1)])
                    total = part if total is None else total + part
                    if ranking:
                        part = rank_sums(torch.stack([got['token_ap'], got['token_auc']], dim=1), got['rank_counts'])
                        rank_total = part if rank_total is None else rank_total + part
                    items += counts.shape[0]
        finally:
            self.model.train(was_training)
        names = ("precision", "recall", "f1", "precision_at_k", "recall_at_k") + (("map", "auc", "auc_stratified", "oracle_f1") if ranking else ())
        if items == 0:
            return dict({name: float('nan') for name in names}, items=0, tokens=0, **(dict(ranked_items=0, auc_items=0) if ranking else {}))
        if ranking:  # (the counts are far below 2^53: exact in f64)
            sums = torch.cat([total.double(), rank_total]).tolist()  # (the one read-back of the evaluation)
            n_valid, n_pos, n_pred, tp, hits, slots = (int(v) for v in sums[:6])
        else:
            n_valid, n_pos, n_pred, tp, hits, slots = total.tolist()  # (the one read-back of the evaluation)
        ratio = lambda a, b: a / b if b else 0.0  # noqa: E731
        precision, recall = ratio(tp, n_pred), ratio(tp, n_pos)
        out = dict(precision=precision, recall=recall, f1=ratio(2 * precision * recall, precision + recall),
                   precision_at_k=ratio(hits, slots), recall_at_k=ratio(hits, n_pos), items=items, tokens=n_valid)
        if ranking:
            out.update(summarize_rank(sums[6:]))
        return out
