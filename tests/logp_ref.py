"""The contract of qg_policy_head_logp / qg_policy_mid_head_logp (include/qgym.h) restated in numpy, f64: the whole row of
log-probabilities and the arg-max of a matrix of logits.

  - a logit below HEAD_MASKED (-1e29; -inf, the dtype's lowest, the packed head's -1e30) is a masked action: probability 0, log-prob -inf;
  - log-prob of a live action = logit - logsumexp(live logits) -- an action far below the maximum keeps its finite value, whatever exp does;
  - the action is the largest logit, equal logits to the lowest index;
  - a row without a live action: action 0, best log-prob 0, entropy 0, every log-prob -inf."""
import numpy as np

HEAD_MASKED = -1.0e29


def logp_ref(logits):
    """logits [B, A] (f64; -inf / anything below HEAD_MASKED = masked) -> (rows f64 [B, A], action int64 [B], best f64 [B], entropy f64 [B])."""
    L = np.asarray(logits, dtype=np.float64)
    B, A = L.shape
    livem = L >= HEAD_MASKED
    any_live = livem.any(axis=1)
    Lm = np.where(livem, L, -np.inf)
    m = np.where(any_live, Lm.max(axis=1, initial=-np.inf), 0.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ex = np.where(livem, np.exp(np.where(livem, L - m[:, None], 0.0)), 0.0)
        s = ex.sum(axis=1)
        lse = m + np.log(np.where(any_live, s, 1.0))
        rows = np.where(livem & any_live[:, None], L - lse[:, None], -np.inf)
        p = ex / np.where(any_live, s, 1.0)[:, None]
        ent = -np.where(p > 0, p * np.where(livem, rows, 0.0), 0.0).sum(axis=1)
    action = np.where(any_live, Lm.argmax(axis=1), 0).astype(np.int64)  # argmax: the first of equal maxima
    best = np.where(any_live, rows[np.arange(B), action], 0.0)
    ent = np.where(any_live, ent, 0.0)
    return rows, action, best, ent


def logsumexp_rows(rows):
    """log sum_a exp(rows[e, a]) in f64 (-inf entries count 0); -inf for a row of -inf."""
    r = np.asarray(rows, dtype=np.float64)
    m = r.max(axis=1)
    ok = np.isfinite(m)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(ok, m + np.log(np.exp(r - np.where(ok, m, 0.0)[:, None]).sum(axis=1)), -np.inf)
    return out
