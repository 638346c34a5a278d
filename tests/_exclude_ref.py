"""numpy restatement of what csrc/exclude.hip puts in front of the sweeps: the merged mask rows of a call with per-query exclusion lists,
and the two workspace formulas of include/llmrec_hip.h."""
import numpy as np

from tests._serve_ref import A

SORT_SLACK = 32 << 20


def merged_rows(train_rowptr, train_colidx, query_users, excl_rowptr, excl_colidx, new_id, n_items=None):
    """(rowptr int32 [n_query + 1], colidx int32): row q = the ascending STABLE merge of
         the kept entries of the train row of query_users[q], in row order, in the swept numbering, and
         the kept entries of exclusion row q, sorted ascending, in the swept numbering;
    train entries come before equal exclusion entries, duplicates stay on both sides. new_id: the filter's map (its length is n_items), or
    None for the identity numbering over n_items items. An entry < 0, >= n_items or with new_id < 0 is dropped. train_rowptr None: no
    train side; excl_rowptr None: no exclusion side."""
    if new_id is not None:
        new_id = np.asarray(new_id, dtype=np.int64)
        n_items = len(new_id)

    def swept(ids):
        ids = np.asarray(ids, dtype=np.int64)
        ids = ids[(ids >= 0) & (ids < n_items)]
        if new_id is not None:
            ids = new_id[ids]
            ids = ids[ids >= 0]
        return ids

    rp, cols = [0], []
    for q, u in enumerate(np.asarray(query_users, dtype=np.int64)):
        a = swept(train_colidx[train_rowptr[u]:train_rowptr[u + 1]]) if train_rowptr is not None else np.zeros(0, np.int64)
        b = np.sort(swept(excl_colidx[excl_rowptr[q]:excl_rowptr[q + 1]])) if excl_rowptr is not None else np.zeros(0, np.int64)
        both = np.concatenate([a, b])
        side = np.concatenate([np.zeros(len(a), np.int64), np.ones(len(b), np.int64)])
        cols.append(both[np.lexsort((np.arange(len(both)), side, both))])       # by (id, train before exclusion, position)
        rp.append(rp[-1] + len(both))
    return np.asarray(rp, dtype=np.int32), (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int32)


def excluded_parts(n_query, n_items, n_kept, d, train_nnz, excl_nnz):
    """byte sizes, in order: item rows (under a filter that drops something), user rows, query list, error word, train counts, train row
    pointers, key bounds, train columns (+ 256 spare bytes), keys x 2, the sort's temporary storage, mask row pointers, mask columns (+ 256)"""
    d4 = -(-d // 4) * 4
    rp = A(4 * (n_query + 1))
    return [A(4 * n_kept * d4) if n_kept != n_items else 0, A(4 * n_query * d4), A(8 * n_query), 256, A(4 * n_query), rp, rp,
            A(4 * train_nnz) + 256, A(8 * excl_nnz), A(8 * excl_nnz), A(excl_nnz + SORT_SLACK) if excl_nnz > 0 else 0, rp,
            A(4 * (train_nnz + excl_nnz)) + 256]


def excluded_workspace_bytes(n_query, n_items, n_kept, d, train_nnz, excl_nnz, wide_bytes):
    """wide_bytes: llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz + excl_nnz)"""
    return 0 if n_kept == 0 else A(wide_bytes) + sum(excluded_parts(n_query, n_items, n_kept, d, train_nnz, excl_nnz))


def mask_offset(n_query, n_items, n_kept, d, train_nnz, excl_nnz, wide_bytes):
    return A(wide_bytes) + sum(excluded_parts(n_query, n_items, n_kept, d, train_nnz, excl_nnz)[:11])
