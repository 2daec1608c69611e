"""Answer-quality metrics of the reference's evaluation scripts that the acceptance bar names (ROUGE-L): on the host over token strings
(``rouge``, with ROUGE-1 / ROUGE-2 beside it), and on the device over token ids together with the consensus pick over a pool of candidates
(``rouge_ids``; ROUGE-N: ``rouge_n_ids``); BLEU and the
n-gram overlap of an answer with its passages, on the host (``bleu``) and on the device (``ngram_ids``); METEOR with its exact stage on
ids and one caller-provided class table, on the host (``meteor``) and on the device (``meteor_ids``); the TREC ranking metrics of the
passage scores, on the host (``trec``) and on the device (``rank_ids``); the token-level counts of the supporting-token stage on the device
(``token_ids``) and its threshold-free ranking figures -- average precision, AUC, the best F1 cut -- (``token_rank``); answer attribution
-- which passage each answer token was copied from -- on the device (``attribution``); the expected cost of a pool of candidates under
the model's posterior and the minimum-risk training step built on it (``risk``)."""
from .rouge import eval_rouge, eval_rouge_l, lcs_length, rouge_l, rouge_n  # noqa: F401
from .rouge_ids import consensus, eval_rouge_l_ids, rouge_l_ids  # noqa: F401
from .rouge_n_ids import eval_rouge_n_ids, rouge_n_ids  # noqa: F401
from .bleu import eval_bleu, modified_precision, ngram_overlap, sentence_bleu  # noqa: F401
from .ngram_ids import bleu_ids, eval_bleu_ids, ngram_overlap_ids  # noqa: F401
from .meteor import best_meteor, count_chunks, eval_meteor, meteor_alignment, pair_meteor, sentence_meteor, stem_classes  # noqa: F401
from .meteor_ids import eval_meteor_ids, meteor_ids  # noqa: F401
from .trec import eval_trec_file, parse_qrel, parse_run, rank_metrics, run_lines  # noqa: F401
from .rank_ids import eval_rank_ids, rank_metrics_ids  # noqa: F401
from .token_ids import eval_token_ids, token_metrics_ids  # noqa: F401
from .token_rank import eval_token_rank_ids, token_rank_host, token_rank_ids  # noqa: F401
from .attribution import (attribution_ids, copy_attribution_host, eval_attribution_ids, source_segments,  # noqa: F401
                          summarize as summarize_attribution)
from .risk import assemble_pool, dedup_valid, minimum_risk_step, pool_cost, sequence_risk_host  # noqa: F401
