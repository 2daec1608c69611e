"""Model-side helpers of the hot path (the on-path subset of the reference's common/Utils.py).

Tokenizers, GloVe loaders, GRU helpers and beam utilities of the reference file are data-prep /
baseline-model code and are out of scope."""
import random

import numpy as np
import torch

from .. import ops
from .Constants import BOS_WORD, EOS_WORD, PAD_WORD, UNK_WORD

NEAR_INF = 1e20
NEAR_INF_FP16 = 65504


def neginf(dtype):
    """A representable finite number near -inf (reference: common/Utils.py:16-21)."""
    return -NEAR_INF_FP16 if dtype is torch.float16 else -NEAR_INF


def _device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")


def generate_square_subsequent_mask(sz):
    """[sz, sz] float mask, 0 on/below the diagonal and -1e20 above (reference :23-28).  The tensor is
    tagged so the attention modules run their causal kernel path without inspecting it."""
    allowed = torch.tril(torch.ones(sz, sz, dtype=torch.bool, device=_device()))
    mask = torch.zeros(sz, sz, device=_device()).masked_fill(~allowed, neginf(torch.float32))
    mask._case_causal = True
    return mask


def init_seed(seed=None):
    """Seeds numpy / torch / random and the dropout counter RNG of the HIP path (reference :57-65)."""
    import time
    from .. import config
    if seed is None:
        seed = int(time.time())
    np.random.seed(seed)
    torch.manual_seed(seed)
    random.seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    config.manual_seed(seed)


def new_tensor(array, requires_grad=False):
    return torch.tensor(array, device=_device(), requires_grad=requires_grad)


def build_map(b_map, max=None):
    """Dense one-hot copy map [B, S, V] (reference :344-355).  Kept for API compatibility only: the models
    pass the source *ids* to the pointer scatter kernel (K11) and never build this tensor."""
    B, S = b_map.shape
    if max is None:
        max = int(b_map.max()) + 1
    out = torch.zeros(B, S, max, device=b_map.device)
    out.scatter_(2, b_map.unsqueeze(2), 1.0)
    return out


def universal_sentence_embedding(sentences, mask, sqrt=False):
    """Masked mean over the sequence axis (reference :455-470); ``sqrt=True`` divides the masked sum by sqrt(count) instead
    (= mean * sqrt(count); not used on the CaSE / Masque path)."""
    mean = ops.masked_mean(sentences, mask)
    if sqrt:
        return mean * mask.sum(dim=1).view(-1, 1).to(mean.dtype).sqrt()
    return mean


def topk(gen_output, k=1, PAD=None, BOS=None, UNK=None):
    """(values, indices) of the k best columns per row, keepdim (reference :156-168).  k = 1 -- the greedy pick of the CaSE / Masque
    loop -- is the HIP row-argmax (lowest index on ties, as ``torch.max``); k > 1 is off the hot path and sorts with
    ``torch.topk`` as the reference does.  Unlike the reference the masked ids are zeroed in a copy, not in the caller's tensor."""
    if PAD is not None or BOS is not None or UNK is not None:
        gen_output = gen_output.clone()
        for tok in (PAD, BOS, UNK):
            if tok is not None:
                gen_output[:, tok] = 0
    if k > 1:
        return torch.topk(gen_output, k, dim=1, largest=True, sorted=True)
    idx, val = ops.row_argmax(gen_output)
    return val.unsqueeze(1), idx.unsqueeze(1)


_special_ids = (None, None)  # (vocabulary object, its special ids): the most recent vocabulary only, compared by identity


def _specials(id2vocab):
    """ids of BOS / PAD / EOS in ``id2vocab`` (-1 when absent).  Only the most recent vocabulary is remembered, together with
    the object itself: an ``id()`` key alone would serve stale ids once a freed vocabulary's address is reused by another one."""
    global _special_ids
    if _special_ids[0] is not id2vocab:
        items = id2vocab.items() if hasattr(id2vocab, "items") else enumerate(id2vocab)
        inv = {w: i for i, w in items if w in (BOS_WORD, PAD_WORD, EOS_WORD)}
        _special_ids = (id2vocab, tuple(inv.get(w, -1) for w in (BOS_WORD, PAD_WORD, EOS_WORD)))
    return _special_ids[1]


def to_sentence(batch_indices, id2vocab):
    """ids -> token lists: drop BOS / PAD, stop at EOS, empty -> [UNK] (reference :200-217).  Ids on the GPU are filtered and
    front-packed by one kernel (K13 post-processing) and come back with ONE device->host copy for the whole batch, instead of
    the reference's ``.item()`` per generated token; host ids take the plain loop."""
    if torch.is_tensor(batch_indices) and batch_indices.is_cuda and batch_indices.dim() == 2:
        bos, pad, eos = _specials(id2vocab)
        kept, count = ops.sentence_compact(batch_indices.long(), bos, pad, eos)
        rows, lens = kept.tolist(), count.tolist()
        return [[id2vocab[i] for i in row[:n]] if n else [UNK_WORD] for row, n in zip(rows, lens)]
    rows = batch_indices.tolist() if torch.is_tensor(batch_indices) else batch_indices
    out = []
    for row in rows:
        words = []
        for index in row:
            w = id2vocab[int(index)]
            if w == BOS_WORD or w == PAD_WORD:
                continue
            if w == EOS_WORD:
                break
            words.append(w)
        out.append(words if words else [UNK_WORD])
    return out


def remove_duplicate_once(sents, n=3):
    """One pass of trailing-n-gram de-duplication (reference :170-186)."""
    changed = False
    for b, sent in enumerate(sents):
        if len(sent) <= n:
            continue
        for i in range(len(sent) - n):
            cut = len(sent) - i - n
            if all(tok in sent[:cut] for tok in sent[cut:]):
                sents[b] = sent[:cut]
                changed = True
                break
    return changed


def remove_duplicate(sents, n=3):
    while remove_duplicate_once(sents, n):
        pass


def remove_duplicate_ids(ids, len, n=3, pad=0):
    """``remove_duplicate`` on the device (K33), in place on ``sentence_compact``'s outputs: ids int64 [B, T] front-packed, len int32 [B]
    -> (ids, len) with every row truncated as ``remove_duplicate`` truncates its token list and PAD behind the new length.  T <= 256."""
    return ops.remove_duplicate_ids(ids, len, n, pad)


def token_freq_table(vocab_freq, device=None):
    """``vocab_freq`` as the 1-D table K37 reads (the count of id v at [v]): a ``{id: count}`` dict becomes an int64 table (f32 when a
    count is not an integer) as long as its largest id + 1; a 1-D tensor is taken as it is (integer -> int64, floating -> f32)."""
    if isinstance(vocab_freq, dict):
        size = max((int(i) for i in vocab_freq), default=-1) + 1
        whole = all(float(c) == int(c) for c in vocab_freq.values())
        table = torch.zeros(size, dtype=torch.int64 if whole else torch.float32)
        if size:
            ids = torch.tensor([int(i) for i in vocab_freq], dtype=torch.int64)
            table[ids] = torch.tensor([c for c in vocab_freq.values()], dtype=table.dtype)
    elif torch.is_tensor(vocab_freq) and vocab_freq.dim() == 1:
        table = vocab_freq.detach().to(torch.float32 if vocab_freq.is_floating_point() else torch.int64)
    else:
        raise TypeError("vocab_freq must be a 1-D tensor of counts or an {id: count} dict")
    return table if device is None else table.to(device)


def token_label(passage, response, vocab_freq, pad=0):
    """The supervision of the supporting-token stage (reference: CaSE/CaSEDataset.py ``token_label``, a Python loop over every token) as
    vectorised torch on the device of ``passage``: passage int64 [B, P, L] with response int64 [B, T], or [P, L] with [T]; ``vocab_freq`` a
    1-D tensor of counts or an ``{id: count}`` dict (0 for an id without an entry) -> (label, weight) f32 of ``passage``'s shape.  With
    A = the ids of the response other than ``pad``, for every row x[0..L):
        label[i] = g1[i] = 1 where x[i] is in A (``pad`` never is)
        g3[i], g5[i] = the number of DISTINCT ids in A among x[i-1 .. i+1] and x[i-2 .. i+2] (positions outside the row read ``pad``)
        lf[i] = ln(f[x[i]] + 2),  S = the sum of lf over all L positions (PAD positions included, as in the reference)
        weight[i] = (S / lf[i] * g1[i] * g3[i] * g5[i]) ^ 0.2 where g1[i] = 1, exactly 1 elsewhere
    All arithmetic is f64, rounded to f32 once.  K37 (``ops.token_labels``) is the same rule in one launch."""
    label, weight = token_label_f64(passage, response, vocab_freq, pad)
    return label.float(), weight.float()


def token_label_f64(passage, response, vocab_freq, pad=0):
    """``token_label`` before its one rounding: (label, weight) as f64."""
    if passage.dim() == 2 and response.dim() == 1:
        label, weight = token_label_f64(passage.unsqueeze(0), response.unsqueeze(0), vocab_freq, pad)
        return label[0], weight[0]
    if passage.dim() != 3 or response.dim() != 2 or response.shape[0] != passage.shape[0]:
        raise TypeError("token_label: passage [B, P, L] with response [B, T], or [P, L] with [T]")
    B, P, L = passage.shape
    x, y = passage.long(), response.long().to(passage.device)
    if torch.is_tensor(vocab_freq) and vocab_freq.dim() == 1:
        table = vocab_freq.detach().to(x.device).double()
    else:
        table = token_freq_table(vocab_freq, x.device).double()
    member = ((x.unsqueeze(-1) == y[:, None, None, :]) & y.ne(pad)[:, None, None, :]).any(-1) & x.ne(pad)
    # the five slots of every window, the row extended by two PAD positions on either side
    xp = torch.nn.functional.pad(x, (2, 2), value=pad)
    mp = torch.nn.functional.pad(member, (2, 2), value=False)
    ids, flags = [xp[..., j:j + L] for j in range(5)], [mp[..., j:j + L] for j in range(5)]

    def distinct(first, last):  # members of slots first..last that no earlier slot of the window repeats
        count = torch.zeros_like(x)
        for j in range(first, last + 1):
            new = flags[j].clone()
            for k in range(first, j):
                new &= ids[k].ne(ids[j])
            count += new
        return count

    g3, g5 = distinct(1, 3), distinct(0, 4)
    F = table.numel()
    inside = (x >= 0) & (x < F)
    f = torch.where(inside, table[x.clamp(0, max(F - 1, 0))], torch.zeros((), dtype=torch.float64, device=x.device)) if F else \
        torch.zeros(x.shape, dtype=torch.float64, device=x.device)
    lf = torch.log(f + 2.0)
    g1 = member.double()
    weight = (lf.sum(-1, keepdim=True) / lf * g1 * g3.double() * g5.double()).pow(0.2)
    weight = torch.where(member, weight, torch.ones((), dtype=torch.float64, device=x.device))
    return g1, weight


def banned_tokens(history, n, vocab_size=None, eos=None):
    """The n-gram ban (K32) restated on a Python list: ``history`` = the ids a row has emitted so far (BOS excluded), t = len(history).
    -> the sorted ids v such that some j <= t - n has history[j : j + n - 1] == history[t - n + 1 : t] and history[j + n - 1] == v; for
    n = 1 every id of the history.  Empty for n < 1, t < n, or a history that holds ``eos``; ids outside [0, vocab_size) are left out."""
    history = [int(x) for x in history]
    t = len(history)
    if n < 1 or t < n or (eos is not None and eos in history):
        return []
    suffix = history[t - n + 1:t]
    banned = {history[j + n - 1] for j in range(t - n + 1) if history[j:j + n - 1] == suffix}
    return sorted(v for v in banned if v >= 0 and (vocab_size is None or v < vocab_size))
