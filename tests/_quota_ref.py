"""numpy restatement of llmrec_score_topk_candidates_capped_f32 (csrc/quota.hip): the survivors of tests/_candidates_ref.py ranked at full
length by tests/_eval_ref.rank, then the quota by the greedy walk down that ranking - and, for the test of the restatement itself, the
quota's other statement: rank within group below cap, then the first K. Nothing here imports llmrec_amd."""
import numpy as np

from tests._candidates_ref import survivors
from tests._candidates_ref import workspace_bytes                  # noqa: F401  (the capped call's workspace is the uncapped call's)
from tests._eval_ref import rank


def group_and_cap(item_group, n_groups, cap):
    """(group per item with -1 = no group, cap per group): a value outside [0, n_groups) is no group; cap is an int or n_groups ints."""
    g = np.asarray(item_group, dtype=np.int64)
    g = np.where((g >= 0) & (g < n_groups), g, -1)
    caps = np.full(n_groups, cap, dtype=np.int64) if np.ndim(cap) == 0 else np.asarray(cap, dtype=np.int64)
    assert caps.shape == (n_groups,)
    return g, caps


def greedy(order, group, caps, K):
    """Down the ranking `order` (item ids): take an item while its group still has room; stop at K."""
    room = caps.copy()
    out = []
    for i in order:
        if len(out) == K:
            break
        g = group[i]
        if g < 0:
            out.append(int(i))
        elif room[g] > 0:
            room[g] -= 1
            out.append(int(i))
    return out


def by_rank_within_group(order, group, caps, K):
    """The other statement: an item is kept if it has no group or fewer than cap(group) items of its group stand before it in `order`; the
    first K kept items."""
    order = np.asarray(order, dtype=np.int64)
    g = group[order]
    within = np.zeros(len(order), dtype=np.int64)
    for pos in range(len(order)):
        within[pos] = np.count_nonzero(g[:pos] == g[pos])
    kept = (g < 0) | (within < caps[np.maximum(g, 0)])
    return order[kept][:K].tolist()


def ranking(scores_row, keep):
    """The ids of `keep` by (score desc, id asc): _eval_ref.rank at full length, with every other item in the place of the train row."""
    ids, _ = rank(scores_row, np.setdiff1d(np.arange(len(scores_row)), keep), len(keep))
    return ids.astype(np.int64)


def topk_candidates_capped(scores, query_users, train_rowptr, train_colidx, K, cand_rowptr, cand_colidx, item_group, n_groups, cap,
                           excl_rowptr=None, excl_colidx=None, new_id=None, walk=greedy):
    """(ids int32 [n, K], scores float32 [n, K]). scores: float32 [n_users, n_items], the chain scores of every pair. cap: an int for every
    group or n_groups ints."""
    n_items = scores.shape[1]
    group, caps = group_and_cap(item_group, n_groups, cap)
    n = len(query_users)
    out_i = np.full((n, K), -1, dtype=np.int32)
    out_s = np.full((n, K), -np.inf, dtype=np.float32)
    for q, u in enumerate(np.asarray(query_users, dtype=np.int64)):
        t = train_colidx[train_rowptr[u]:train_rowptr[u + 1]] if train_rowptr is not None else ()
        e = excl_colidx[excl_rowptr[q]:excl_rowptr[q + 1]] if excl_rowptr is not None else ()
        keep = survivors(cand_colidx[cand_rowptr[q]:cand_rowptr[q + 1]], n_items, t, e, new_id)
        got = walk(ranking(scores[u], keep), group, caps, K)
        out_i[q, :len(got)] = got
        out_s[q, :len(got)] = scores[u, got]
    return out_i, out_s


def recommend_capped(scores, query_users, train_rowptr, train_colidx, K, item_group, n_groups, cap, excl_rowptr=None, excl_colidx=None, new_id=None):
    """The same over the whole catalogue: every query's candidate row is [0, n_items)."""
    n, n_items = len(query_users), scores.shape[1]
    rp = np.arange(n + 1, dtype=np.int64) * n_items
    ci = np.tile(np.arange(n_items, dtype=np.int64), n)
    return topk_candidates_capped(scores, query_users, train_rowptr, train_colidx, K, rp, ci, item_group, n_groups, cap, excl_rowptr, excl_colidx, new_id)
