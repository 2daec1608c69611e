"""TREC ranking metrics of score tensors, on the device.

``trec.py`` beside this file is the host form (``{qid: {docid: score}}`` dicts, ``Fraction``) and states the definitions.  Here the scores
stay where the selection stage left them -- ``rank`` [B, P] of ``do_rank`` / ``do_test`` / ... --, every row is its own query, and K36
(``ops.rank_metrics``) sorts the row and computes every metric in one launch.  Nothing is read back to the host.

Items that share a query id are NOT merged (the reference's ``run[qid][pid] = score`` lets a later line overwrite an earlier one; the file
form of ``trec.py`` keeps that).  Limits: P <= 1024 document slots, P + R <= 2048 judged documents per row."""
import torch

from .. import ops


def _grades(scores, labels):
    """labels int64 [B] (the index of the one relevant slot, ``data['passage_label']``'s form) or an integer [B, P] tensor of grades -> int32
    [B, P]."""
    if not torch.is_tensor(scores) or scores.dim() != 2:
        raise TypeError("rank_metrics_ids: scores must be a float [B, P] tensor")
    B, P = scores.shape
    if not torch.is_tensor(labels) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise TypeError("rank_metrics_ids: labels must be an integer tensor, int64 [B] (gold index) or [B, P] (grades)")
    if labels.dim() == 1 and labels.shape[0] == B and labels.dtype == torch.int64:
        return torch.zeros(B, P, dtype=torch.int32, device=scores.device).scatter_(1, labels.unsqueeze(1), 1)
    if tuple(labels.shape) == (B, P):
        return labels.to(torch.int32)
    raise TypeError("rank_metrics_ids: labels must be int64 [B] (gold index) or an integer [B, P] tensor of grades for scores [%d, %d]" % (B, P))


def _metrics(scores, labels, keys, valid, extra_rel):
    rel = _grades(scores, labels)
    keys = None if keys is None else keys.to(torch.int32)
    extra_rel = None if extra_rel is None else extra_rel.to(torch.int32)
    return ops.rank_metrics(scores.float(), rel, keys, valid, extra_rel)


def rank_metrics_ids(scores, labels, keys=None, valid=None, extra_rel=None):
    """scores float [B, P] (every row one query), labels int64 [B] (gold index) or integer [B, P] (grades), keys integer [B, P] (tie keys:
    the larger first; None = the column index), valid bool [B, P] (None = all retrieved), extra_rel integer [B, R] (grades of judged but
    unretrieved documents, <= 0 = padding) -> dict of f64 [B] columns ``map``, ``ndcg``, ``recall_5`` .. ``recall_1000``, ``recip_rank``,
    ``P_1``, plus ``order`` int32 [B, P] (columns in rank order, -1 behind the retrieved ones) and ``num_rel`` int32 [B]."""
    got = _metrics(scores, labels, keys, valid, extra_rel)
    out = {name: got["metrics"][:, i] for i, name in enumerate(ops.RANK_METRICS)}
    out["order"], out["num_rel"] = got["order"], got["num_rel"]
    return out


def eval_rank_ids(scores, labels, keys=None, valid=None, extra_rel=None):
    """``rank_metrics_ids``' arguments -> f64 [13] on the device: the sums over the rows of the metrics in ``ops.RANK_METRICS``' order (divide
    by the number of rows for the corpus figure; a row with ``num_rel == 0`` adds 0 and still counts)."""
    return _metrics(scores, labels, keys, valid, extra_rel)["metrics"].sum(0)
