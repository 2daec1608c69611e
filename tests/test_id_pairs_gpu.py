"""K30, K34, K40 and K43 hold a row by one rule (csrc/id_rows.h): a pool run against itself must say so.  For a row of length L against
itself the LCS is L, every k-gram is matched (clip = L - k + 1, hit = distinct, and K34's distinct = K43's), and METEOR's alignment is
the identity in one chunk: identities that need no host form, compared exactly.  The rows come from a 3-word vocabulary (full of
repeats), their lengths sit at the edges of the held words, two stated lengths lie outside 0 .. Ta, and 15 rows leave one of the four
waves of the last workgroup without a row."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, N, WORDS_OF_VOCAB = 3, 5, 3


def _pool(Ta):
    """-> (ids int64 [B, N, Ta] with ids of the vocabulary behind every length too, so that reading them would count; the stated lengths
    int32 [B, N]; the lengths that must be in effect)."""
    rng = np.random.RandomState(1000 + Ta)
    ids = rng.randint(0, WORDS_OF_VOCAB, size=(B, N, Ta)).astype(np.int64)
    stated = np.array([(0, 1, Ta - 1, Ta)[i % 4] for i in range(B * N)], dtype=np.int32)
    rng.shuffle(stated)
    stated[3], stated[11] = Ta + 5, -3  # must behave as Ta and 0
    return torch.from_numpy(ids).cuda(), torch.from_numpy(stated.reshape(B, N)).cuda(), torch.from_numpy(np.clip(stated, 0, Ta).reshape(B, N)).long().cuda()


def _diag(x):
    """[B, N, N, ...] -> [B, N, ...]: hypothesis n against reference n."""
    return torch.diagonal(x, dim1=1, dim2=2).movedim(-1, 1)


@pytest.mark.parametrize("Ta", (1, 64, 65, 128, 129, 256))
def test_a_pool_against_itself(Ta):
    from case_rg_amd import ops
    a, stated, L = _pool(Ta)
    assert set(L.flatten().tolist()) >= {0, Ta} and B * N % 4 != 0
    empty = L.eq(0)
    k = torch.arange(4, device=a.device)

    lcs, f = ops.lcs_pairs(a, stated, a, stated)
    assert torch.equal(_diag(lcs).long(), L)
    assert not lcs[empty].any() and not f[empty].any()

    for max_n in (2, 4):
        counts = ops.ngram_counts(a, stated, a, stated, max_n)
        distinct = ops.ngram_distinct(a, stated, max_n)
        assert torch.equal(counts["distinct"], distinct), "K34 and K43 count the distinct k-grams of the same rows"
        assert torch.equal(_diag(counts["hit"]), distinct)
        total = (L.unsqueeze(-1) - k).clamp_min(0)
        total = torch.where(k < max_n, total, torch.zeros_like(total))
        assert torch.equal(_diag(counts["clip"]).long(), total)
        assert not counts["distinct"][..., max_n:].any() and not counts["hit"][..., max_n:].any() and not counts["clip"][..., max_n:].any()
        assert not counts["clip_any"][..., max_n:].any() and not counts["hit_any"][..., max_n:].any()
        assert distinct[..., 0].gt(0).eq(L.gt(0)).all() and bool((distinct[..., 0] <= WORDS_OF_VOCAB).all())
        for name in ("clip", "clip_any", "hit", "hit_any", "distinct"):
            assert not counts[name][empty].any(), name
        assert not distinct[empty].any()

    out = ops.meteor(a, stated, a, stated, want_align=True)
    matches, exact, chunks = (_diag(out["counts"])[..., i].long() for i in range(3))
    assert torch.equal(matches, L) and torch.equal(exact, L) and torch.equal(chunks, L.gt(0).long())
    at = torch.arange(Ta, device=a.device)
    assert torch.equal(_diag(out["align"]).long(), torch.where(at < L.unsqueeze(-1), at, torch.full_like(at, -1)))
    assert not out["counts"][empty].any() and not out["meteor_pair"][empty].any() and not out["meteor"][empty].any()
    assert not out["align"][empty].ne(-1).any()
