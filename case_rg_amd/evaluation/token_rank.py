"""Threshold-free ranking metrics of the supporting-token stage: average precision, AUC and the best F1 cut over the tokens of an item.

``token_ids`` measures the stage at two operating points (``token_score > 0`` and the first K of the list).  The figures here say whether
the stage ranks supporting tokens above the rest, whatever threshold or K a caller later picks; they do not depend on the scale of the
logits.  K45 (``ops.token_rank``) computes them on the device in one launch per batch, nothing is read back; ``token_rank_host`` states
them in exact arithmetic.

Definitions.  Each row is one item with S positions, given as ``scores`` (float), ``labels`` (float) and ``valid`` (bool).
  - Only valid positions exist.
  - A valid position is positive where ``label > 0.5``, as in K38.  A label of exactly 0.5 is not positive.
  - n_pos and n_neg count the valid positives and the valid others.
  - Scores compare as K38's and K36's key does: NaN as -inf, ``-0.0 == +0.0``.
  - The valid positions fall into G groups of equal key, g = 1 .. G from the highest key down.
  - pos_g and neg_g are the group's counts.
  - tp_g and n_g are the cumulative positives and the cumulative positions through group g.  tp_0 = 0.
  - Nothing depends on the order inside a group, so nothing depends on position.
The figures:
  - AP, one threshold per distinct score: ``ap = (1 / n_pos) sum_g (tp_g - tp_{g-1}) tp_g / n_g``; 0.0 where n_pos = 0.  On a row without
    ties this is trec_eval's average precision, i.e. K36's ``map``.
  - AUC, Mann-Whitney with ties counted half: ``auc_num2 = sum_g pos_g (2 (n_neg - negcum_g) + neg_g)`` with negcum_g the cumulative
    negatives through g, an integer of at most 2 x 8192^2 < 2^31; ``auc = auc_num2 / (2 n_pos n_neg)``, one f64 division of exact
    integers; 0.0 where n_pos n_neg = 0 (the counts tell a caller that it is undefined there).
  - Best F1, the best cut the ranking allows: the g that maximises ``2 tp_g / (n_g + n_pos)``, fractions compared exactly by integer
    cross-multiplication, the lowest g among equal fractions -> ``best_tp``, ``best_n`` and ``best_threshold``, the group's score as f32
    in canonical form (+0.0 for either zero, -inf for NaN).  Where n_pos = 0 they are 0, 0 and +inf (predict nothing).
Limits: P x L <= 16384 positions per item.  Not computed: an AUC pooled over the items of a corpus, NDCG over tokens, precision-recall
curves."""
import math
import struct
from fractions import Fraction

import torch

from .. import ops

RANK_SUMS = ("ap", "auc", "ranked_items", "auc_items", "auc_num2", "auc_den2", "best_tp", "best_den")  # ``eval_token_rank_ids``' columns


def _rows(x, what):
    if torch.is_tensor(x):
        x = x.detach().cpu().tolist()
    elif hasattr(x, "tolist"):
        x = x.tolist()
    if not isinstance(x, (list, tuple)):
        raise TypeError("token_rank_host: %s must be a tensor, an array or a nested list" % what)
    if len(x) == 0 or not isinstance(x[0], (list, tuple)):
        return [list(x)], True
    return [list(r) for r in x], False


def canonical_score(x):
    """The f32 a score compares as: NaN -> -inf, either zero -> +0.0, anything else rounded to f32."""
    x = float(x)
    if x != x:
        return -math.inf
    try:
        x = struct.unpack("f", struct.pack("f", x))[0]
    except OverflowError:  # beyond f32's range
        x = math.copysign(math.inf, x)
    return 0.0 if x == 0.0 else x


def _row_host(scores, labels, valid):
    if not (len(scores) == len(labels) == len(valid)):
        raise ValueError("token_rank_host: scores, labels and valid must have one shape")
    groups = {}
    for s, l, v in zip(scores, labels, valid):
        if v:
            g = groups.setdefault(canonical_score(s), [0, 0])
            g[0 if float(l) > 0.5 else 1] += 1
    n_pos = sum(g[0] for g in groups.values())
    n_neg = sum(g[1] for g in groups.values())
    tp = n = negcum = auc_num2 = 0
    ap_sum = Fraction(0)
    best = None  # (fraction, tp, n, key)
    for key in sorted(groups, reverse=True):
        pos_g, neg_g = groups[key]
        tp_before = tp
        tp, n, negcum = tp + pos_g, n + pos_g + neg_g, negcum + neg_g
        ap_sum += Fraction((tp - tp_before) * tp, n)
        auc_num2 += pos_g * (2 * (n_neg - negcum) + neg_g)
        f = Fraction(2 * tp, n + n_pos)
        if best is None or f > best[0]:
            best = (f, tp, n, key)
    out = dict(n_valid=n_pos + n_neg, n_pos=n_pos, n_neg=n_neg, auc_num2=auc_num2, n_groups=len(groups))
    out["ap"] = ap_sum / n_pos if n_pos else Fraction(0)
    out["auc"] = Fraction(auc_num2, 2 * n_pos * n_neg) if n_pos and n_neg else None
    if n_pos:
        out.update(best_tp=best[1], best_n=best[2], best_threshold=best[3], best_f1=best[0])
    else:
        out.update(best_tp=0, best_n=0, best_threshold=math.inf, best_f1=None)
    return out


def token_rank_host(scores, labels, valid=None):
    """The definitions of this module in exact arithmetic.  scores, labels and valid (None: all) are tensors, arrays or nested lists, [S] or
    [B, S] -> for [S] one dict, for [B, S] a list of B dicts: ``n_valid``, ``n_pos``, ``n_neg``, ``auc_num2``, ``best_tp``, ``best_n``,
    ``n_groups`` (ints), ``ap`` (a ``Fraction``; 0 where n_pos = 0), ``auc`` and ``best_f1`` (``Fraction``s, None where undefined:
    n_pos n_neg = 0 and n_pos = 0) and ``best_threshold`` (a Python float in canonical form; +inf where n_pos = 0)."""
    s, single = _rows(scores, "scores")
    l, _ = _rows(labels, "labels")
    v = [[True] * len(r) for r in s] if valid is None else _rows(valid, "valid")[0]
    if not (len(s) == len(l) == len(v)):
        raise ValueError("token_rank_host: scores, labels and valid must have one shape")
    out = [_row_host(*row) for row in zip(s, l, v)]
    return out[0] if single else out


def _rank(who, token_score, token_label, valid, select):
    if not torch.is_tensor(token_score) or not token_score.is_floating_point() or token_score.dim() < 2:
        raise TypeError("%s: token_score must be a float [B, S] or [B, P, L] tensor" % who)
    B = token_score.shape[0]
    key = token_score if select is None else select
    for name, t in (("token_label", token_label), ("valid", valid), ("select", key)):
        if not torch.is_tensor(t) or t.shape != token_score.shape:
            raise TypeError("%s: %s must have token_score's shape %s" % (who, name, tuple(token_score.shape)))
    flat = lambda t: t.reshape(B, -1)  # noqa: E731
    return ops.token_rank(flat(key).float(), flat(valid).bool(), flat(token_label).float())


def token_rank_ids(token_score, token_label, valid, select=None):
    """token_score float [B, S] or [B, P, L] (every row one item), token_label (0 / 1) and valid (bool) of the same shape, ``select`` the
    keys the tokens are ranked by (default ``token_score``; e.g. ``token_prior``) -> dict of ``ap`` and ``auc`` f64 [B], the int64 [B]
    columns ``n_valid``, ``n_pos``, ``auc_num2``, ``best_tp``, ``best_n``, ``n_groups`` (``ops.TOKEN_RANK_COUNTS``) and ``n_neg``, and
    ``best_threshold`` f32 [B].  One K45 launch, nothing is read back."""
    got = _rank("token_rank_ids", token_score, token_label, valid, select)
    counts = got["counts"].long()
    out = {name: counts[:, i] for i, name in enumerate(ops.TOKEN_RANK_COUNTS)}
    out["n_neg"] = out["n_valid"] - out["n_pos"]
    out["ap"], out["auc"] = got["stats"][:, 0], got["stats"][:, 1]
    out["best_threshold"] = got["threshold"]
    return out


def rank_sums(stats, counts):
    """K45's ``stats`` f64 [B, 2] and ``counts`` int32 [B, 6] -> f64 [8] on the device, the sums over the items in ``RANK_SUMS``' order: ap,
    auc, [n_pos > 0], [n_pos n_neg > 0], auc_num2, 2 n_pos n_neg, best_tp, best_n + n_pos.  The integer columns are exact in f64 while a
    sum stays below 2^53: an item adds less than 2^28 to any of them, so that holds for the first 2^25 items at the least."""
    c = counts.double()
    n_valid, n_pos, auc_num2, best_tp, best_n = (c[:, i] for i in range(5))
    pairs2 = 2.0 * n_pos * (n_valid - n_pos)
    ranked = n_pos > 0
    cols = (stats[:, 0], stats[:, 1], ranked.double(), (pairs2 > 0).double(), auc_num2, pairs2, best_tp, best_n + n_pos)
    return torch.stack(cols, dim=1).sum(0)


def eval_token_rank_ids(token_score, token_label, valid, select=None):
    """``token_rank_ids``' arguments -> f64 [8] on the device: ``rank_sums`` of the batch (``RANK_SUMS`` names the columns)."""
    got = _rank("eval_token_rank_ids", token_score, token_label, valid, select)
    return rank_sums(got["stats"], got["counts"])


def summarize_rank(sums):
    """The eight sums (``RANK_SUMS``' order, Python numbers) -> dict(map = mean AP over the items with a positive, auc = mean AUC over the
    items with both classes, auc_stratified = sum auc_num2 / sum 2 n_pos n_neg (the within-item pair-weighted figure), oracle_f1 =
    2 sum best_tp / sum (best_n + n_pos): the pooled F1 when every item is cut where its own F1 peaks -- no threshold does better on any
    single item; the pooled figure itself is a mediant and no strict bound --, ranked_items, auc_items); a ratio with a zero denominator is
    0.0."""
    ap, auc, ranked, both, num2, den2, best_tp, best_den = sums
    ratio = lambda a, b: a / b if b else 0.0  # noqa: E731
    return dict(map=ratio(ap, ranked), auc=ratio(auc, both), auc_stratified=ratio(num2, den2), oracle_f1=ratio(2 * best_tp, best_den),
                ranked_items=int(ranked), auc_items=int(both))
