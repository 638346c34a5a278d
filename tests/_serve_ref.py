"""numpy restatement of what csrc/serve.hip puts in front of the sweeps: the id maps of an allow mask, the compact mask rows of a call,
and the two workspace formulas of include/llmrec_hip.h."""
import numpy as np


def id_maps(allow):
    """(new_id int32 [n], old_id int32 [n_kept], n_kept): any non-zero byte is eligible; new_id = rank among the eligible items or -1."""
    flags = np.asarray(allow).astype(np.uint8) != 0
    new_id = np.where(flags, np.cumsum(flags) - 1, -1).astype(np.int32)
    old_id = np.flatnonzero(flags).astype(np.int32)
    return new_id, old_id, int(flags.sum())


def mask_rows(rowptr, colidx, query_users, new_id):
    """(rowptr int32 [n_query + 1], colidx int32): row q = the entries c of the train row of query_users[q] with new_id[c] >= 0, as
    new_id[c], in row order - duplicates kept, one row per query whatever the user ids are."""
    rp, cols = [0], []
    for u in np.asarray(query_users, dtype=np.int64):
        row = new_id[np.asarray(colidx[rowptr[u]:rowptr[u + 1]], dtype=np.int64)]
        cols.append(row[row >= 0])
        rp.append(rp[-1] + len(cols[-1]))
    return np.asarray(rp, dtype=np.int32), (np.concatenate(cols) if cols else np.zeros(0)).astype(np.int32)


def A(x):
    return -(-x // 256) * 256


def filter_workspace_bytes(n_items, tile):
    return A(4 * -(-n_items // tile)) + 256


def filtered_parts(n_query, n_kept, d, train_nnz):
    """byte sizes, in order: item rows, user rows, query list, error word, counts, mask row pointers, mask columns (+ their 256 spare bytes)"""
    d4 = -(-d // 4) * 4
    return [A(4 * n_kept * d4), A(4 * n_query * d4), A(8 * n_query), 256, A(4 * n_query), A(4 * (n_query + 1)), A(4 * train_nnz) + 256]


def filtered_workspace_bytes(n_query, n_kept, d, train_nnz, wide_bytes):
    """wide_bytes: llmrec_score_topk_wide_workspace_bytes(n_query, n_kept, d, K, train_nnz)"""
    return 0 if n_kept == 0 else A(wide_bytes) + sum(filtered_parts(n_query, n_kept, d, train_nnz))


def mask_offset(n_query, n_kept, d, train_nnz, wide_bytes):
    return A(wide_bytes) + sum(filtered_parts(n_query, n_kept, d, train_nnz)[:5])
