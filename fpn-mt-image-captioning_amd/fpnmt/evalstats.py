"""Held-out statistics from the device-side totals of Pipeline.validate
(TrainEngine.eval_step / fpnmt_caption_stats): pure host arithmetic."""
import math


def summarize(totals, captions):
    """totals = (sum of log-probabilities, tokens, hits) over the live
    positions of `captions` teacher-forced captions ->
    {"token_nll" = -sum logp / tokens, "perplexity" = exp(token_nll),
     "token_accuracy" = hits / tokens, "tokens", "captions", "totals"}.
    The totals are plain sums: those of several ranks' shards add before
    this. No live token raises ValueError (nothing to average over)."""
    if len(totals) != 3:
        raise ValueError(f"summarize: totals must hold 3 sums, got {len(totals)}")
    logp, tokens, hits = (float(x) for x in totals)
    if not tokens > 0 or tokens != int(tokens):
        raise ValueError(f"summarize: tokens must be a positive whole number, got {tokens}")
    if not 0 <= hits <= tokens or not logp <= 0 or int(captions) < 1:
        raise ValueError(f"summarize: inconsistent totals {(logp, tokens, hits)} for {captions} captions")
    nll = -logp / tokens
    return {"token_nll": nll, "perplexity": math.exp(nll) if nll < 709.0 else math.inf,
            "token_accuracy": hits / tokens, "tokens": int(tokens), "captions": int(captions),
            "totals": (logp, tokens, hits)}
