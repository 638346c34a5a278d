"""numpy restatement of llmrec_score_topk_candidates_f32 (csrc/candidates.hip): the set rule of a candidate row, the removals, the ranking
by tests/_eval_ref.rank over tests/_eval_ref.chain_scores, and the workspace formula of include/llmrec_hip.h. Nothing here imports
llmrec_amd."""
import numpy as np

from tests._eval_ref import rank
from tests._serve_ref import A

SORT_SLACK = 32 << 20


def candidate_set(row, n_items, new_id=None):
    """The ids of a candidate row as a sorted set: repeats collapse; an id < 0, >= n_items or with new_id[id] < 0 is ignored."""
    ids = np.unique(np.asarray(row, dtype=np.int64))
    ids = ids[(ids >= 0) & (ids < n_items)]
    if new_id is not None:
        ids = ids[np.asarray(new_id, dtype=np.int64)[ids] >= 0]
    return ids


def survivors(row, n_items, train_row=(), excl_row=(), new_id=None):
    """candidate_set minus the train row minus the exclusion row (either may hold anything: repeats, padding, ids that are no items)."""
    ids = candidate_set(row, n_items, new_id)
    gone = np.concatenate([np.asarray(train_row, dtype=np.int64).reshape(-1), np.asarray(excl_row, dtype=np.int64).reshape(-1)])
    return ids[~np.isin(ids, gone)]


def topk_candidates(scores, query_users, train_rowptr, train_colidx, K, cand_rowptr, cand_colidx, excl_rowptr=None, excl_colidx=None, new_id=None):
    """(ids int32 [n, K], scores float32 [n, K]). scores: float32 [n_users, n_items], the chain scores of every pair (row u = user u). Query q
    ranks the survivors of candidate row q by (score desc, id asc): _eval_ref.rank with every other item in the place of the train row."""
    n_items = scores.shape[1]
    n = len(query_users)
    out_i = np.full((n, K), -1, dtype=np.int32)
    out_s = np.full((n, K), -np.inf, dtype=np.float32)
    every = np.arange(n_items)
    for q, u in enumerate(np.asarray(query_users, dtype=np.int64)):
        t = train_colidx[train_rowptr[u]:train_rowptr[u + 1]] if train_rowptr is not None else ()
        e = excl_colidx[excl_rowptr[q]:excl_rowptr[q + 1]] if excl_rowptr is not None else ()
        keep = survivors(cand_colidx[cand_rowptr[q]:cand_rowptr[q + 1]], n_items, t, e, new_id)
        out_i[q], out_s[q] = rank(scores[u], np.setdiff1d(every, keep), K)
    return out_i, out_s


def workspace_bytes(n_query, K, cand_nnz, excl_nnz):
    """error word; candidate keys x 2, ids x 2, the candidate sorts' temporary storage; exclusion keys x 2 and the exclusion sort's reserve"""
    if n_query < 0 or K < 1 or n_query * K >= 1 << 31 or not 0 <= cand_nnz < 1 << 31 or not 0 <= excl_nnz < 1 << 31:
        return -1
    if n_query == 0 or cand_nnz == 0:
        return 0
    return (256 + 2 * A(8 * cand_nnz) + 2 * A(4 * cand_nnz) + A(cand_nnz + SORT_SLACK) + 2 * A(8 * excl_nnz)
            + (A(excl_nnz + SORT_SLACK) if excl_nnz > 0 else 0))
