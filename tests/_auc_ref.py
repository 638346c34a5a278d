"""numpy statement of the full-rank AUC contract of llmrec_score_auc_f32 (include/llmrec_hip.h): integer pair counts over the candidates
(all items but the train row), the held-out row taken as a set."""
import numpy as np


def auc_counts(s, train_row, held_row, n_items):
    """s: float32 [n_items] scores of one user. Returns (c2, |P|, |N|, auc) with c2 an exact Python int."""
    s = np.asarray(s, dtype=np.float32)
    cand = np.ones(n_items, dtype=bool)
    t = np.asarray(train_row, dtype=np.int64)
    cand[t[(t >= 0) & (t < n_items)]] = False
    held = np.zeros(n_items, dtype=bool)
    h = np.asarray(held_row, dtype=np.int64)
    held[h[(h >= 0) & (h < n_items)]] = True
    pos, neg = cand & held, cand & ~held
    n_p, n_n = int(pos.sum()), int(neg.sum())
    if not np.isfinite(s[cand]).all():
        return 0, n_p, n_n, 0.0
    sp = np.sort(s[pos])
    sn = s[neg]
    lt = np.searchsorted(sp, sn, side="left").astype(np.int64)      # #{s_p <  s_n}
    le = np.searchsorted(sp, sn, side="right").astype(np.int64)     # #{s_p <= s_n}
    c2 = int((2 * (n_p - le) + (le - lt)).sum())
    auc = c2 / (2.0 * n_p * n_n) if n_p > 0 and n_n > 0 else 0.0
    return c2, n_p, n_n, auc


def reference_auc(s, train_row, held_row, n_items):
    """The reference's get_auc + metrics.auc (reference utility/batch_test.py:38-51, utility/metrics.py:95-100) over the candidates;
    None when sklearn is absent."""
    try:
        from sklearn.metrics import roc_auc_score
    except Exception:
        return None
    banned = set(int(i) for i in train_row)
    pos = set(int(i) for i in held_row)
    item_score = sorted(((i, s[i]) for i in range(n_items) if i not in banned), key=lambda kv: kv[1])
    item_score.reverse()
    r = [1 if i in pos else 0 for i, _ in item_score]
    try:
        return roc_auc_score(y_true=r, y_score=[v for _, v in item_score])
    except Exception:
        return 0.
