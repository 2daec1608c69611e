"""Token-level metrics of the supporting-token stage, on the device.

The stage's logits stay where ``CaSE.do_extract`` left them -- ``token_score`` [B, P, L] --, every row is one item, and K38
(``ops.token_select``) counts the row and picks its K best tokens in one launch.  Nothing is read back to the host.

A token is predicted where its logit is positive (sigmoid > 0.5) and labelled where its label exceeds 0.5; only valid (non-PAD) positions
count.  ``hits`` are the labelled tokens among the K selected ones, where the selection key (``select``) may differ from the logits, e.g.
``token_prior``.  Average precision, AUC and the best F1 cut over tokens are in ``token_rank`` (K45).  Limits: P x L <= 16384 positions per
item, K <= 256."""
import torch

from .. import ops


def _select(token_score, token_label, valid, top_k, select):
    if not torch.is_tensor(token_score) or not token_score.is_floating_point() or token_score.dim() < 2:
        raise TypeError("token_metrics_ids: token_score must be a float [B, S] or [B, P, L] tensor")
    B = token_score.shape[0]
    key = token_score if select is None else select
    for name, t in (("token_label", token_label), ("valid", valid), ("select", key)):
        if not torch.is_tensor(t) or t.shape != token_score.shape:
            raise TypeError("token_metrics_ids: %s must have token_score's shape %s" % (name, tuple(token_score.shape)))
    flat = lambda t: t.reshape(B, -1)  # noqa: E731
    return ops.token_select(flat(key).float(), flat(valid).bool(), top_k, scores=flat(token_score).float(), labels=flat(token_label).float())


def token_metrics_ids(token_score, token_label, valid, top_k=32, select=None):
    """token_score float [B, S] or [B, P, L] (logits, every row one item), token_label (0 / 1) and valid (bool) of the same shape, ``select``
    the keys the ``top_k`` tokens are chosen by (default ``token_score``; e.g. ``token_prior``) -> dict of int64 [B] columns ``n_valid``,
    ``n_pos`` (valid and label > 0.5), ``n_pred`` (valid and logit > 0), ``tp`` (both), ``hits`` (labelled among the selected), plus
    ``support_pos`` int32 [B, top_k] (flat positions, best first, -1 behind the valid ones)."""
    got = _select(token_score, token_label, valid, top_k, select)
    counts = got["counts"].long()
    out = {name: counts[:, i] for i, name in enumerate(ops.TOKEN_COUNTS)}
    out["support_pos"] = got["pos"]
    return out


def eval_token_ids(token_score, token_label, valid, top_k=32, select=None):
    """``token_metrics_ids``' arguments -> int64 [5] on the device: the sums over the items of the counts in ``ops.TOKEN_COUNTS``' order."""
    return _select(token_score, token_label, valid, top_k, select)["counts"].long().sum(0)
