"""numpy restatement of the prune selection (bpr_rank_kernel and the multi-block selection of llmrec_bpr_prune_fwd_wide_f32), stated
without reference to how either computes it: of the global list m[0 .. Bg), sample j is kept iff fewer than k = int(remember * Bg)
entries precede it, where i precedes j when m[i] < m[j], or m[i] == m[j] and i < j. Comparison is float comparison (-0.0 == +0.0)."""
import numpy as np

from tests._tree_ref import tree_lds


def k_of(remember, Bg):
    return int(float(remember) * float(Bg))                              # (int)(remember_rate * (double)Bg)


def keep_mask(m, remember):
    """bool [Bg]: the k smallest entries, ties by lower index."""
    m = np.asarray(m, dtype=np.float32)
    k = k_of(remember, len(m))
    canon = np.where(m == 0, np.float32(0.0), m)                        # -0.0 -> +0.0: lexsort must not see two zeros
    keep = np.zeros(len(m), dtype=bool)
    keep[np.lexsort((np.arange(len(m)), canon))[:max(k, 0)]] = True
    return keep


def keep_mask_brute(m, remember):
    """the definition itself, O(Bg^2)"""
    m = np.asarray(m, dtype=np.float32)
    k = k_of(remember, len(m))
    idx = np.arange(len(m))
    before = (m[None, :] < m[:, None]) | ((m[None, :] == m[:, None]) & (idx[None, :] < idx[:, None]))
    return before.sum(1) < k


def expected(m_global, sg_local, remember, offset=0):
    """(keep [B], coef [B], kept_m [B], mf share) of the B = len(sg_local) samples at `offset` of the global list: coef are the bits of
    saved[0 .. B), kept_m those of the sg slots after the selection, the share those of out2[0] (bpr_reduce_kernel's tree)."""
    m_global = np.asarray(m_global, dtype=np.float32)
    sg_local = np.asarray(sg_local, dtype=np.float32)
    B = len(sg_local)
    k = k_of(remember, len(m_global))
    keep = keep_mask(m_global, remember)[offset:offset + B]
    m = m_global[offset:offset + B]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        coef = np.where(keep, np.float32(-1.0) / np.float32(k) * sg_local, np.float32(0.0)).astype(np.float32)
        kept_m = np.where(keep, m, np.float32(0.0)).astype(np.float32)
        share = -(np.float32(tree_lds(kept_m)) / np.float32(k))
    return keep, coef, kept_m, np.float32(share)
