"""The scatter plan of a batch (llmrec_bpr_scatter_plan, llmrec_bpr_scatter_plan_wide) restated in numpy: per side a sort of the keys
id << 32 | slot, the unused slots (samples at or beyond n_valid) with the id 0xffffffff at the end, and the run lengths. numpy only."""
import numpy as np

NO_ID = 0xFFFFFFFF


def _side(ids, slots_valid):
    """(sorted keys uint64, runlen int32) of one side: ids[i] is slot i's id where slots_valid[i], else the slot is unused"""
    n = len(ids)
    idv = np.where(slots_valid, np.asarray(ids, dtype=np.uint64), np.uint64(NO_ID))
    keys = np.sort((idv << np.uint64(32)) | np.arange(n, dtype=np.uint64))
    sid = keys >> np.uint64(32)
    head = np.ones(n, dtype=bool)
    head[1:] = sid[1:] != sid[:-1]
    starts = np.flatnonzero(head)
    lens = np.diff(np.append(starts, n))
    runlen = np.zeros(n, dtype=np.int32)
    runlen[starts] = lens
    runlen[sid == np.uint64(NO_ID)] = 0
    return keys, runlen


def plan(users, pos, neg, B_max, n_valid=None):
    """the LLMREC_BPR_PLAN_WORDS(B_max) = 5 B_max 64-bit words, as int64: 3 B_max keys, then 3 B_max int32 run lengths (1.5 B_max words)
    and, for an odd B_max, the half word nothing defines - zero here; compare words()[: 3 B_max] and runlens() instead of the raw tail"""
    B = B_max if n_valid is None else min(max(int(n_valid), 0), B_max)
    valid = np.arange(B_max) < B
    ku, ru = _side(np.asarray(users)[:B_max], valid)
    ki, ri = _side(np.concatenate([np.asarray(pos)[:B_max], np.asarray(neg)[:B_max]]), np.concatenate([valid, valid]))
    return np.concatenate([ku, ki]).view(np.int64), np.concatenate([ru, ri])


def split(words, B_max):
    """(keys int64 [3 B_max], runlen int32 [3 B_max]) of a device plan's words (int64, at least 5 B_max of them)"""
    words = np.ascontiguousarray(np.asarray(words, dtype=np.int64)[:5 * B_max])
    return words[:3 * B_max], words[3 * B_max:].view(np.int32)[:3 * B_max]


def runs(keys, runlen, B_max):
    """side -> {id: [slots ascending]} as the backward walks the plan: the head of a run owns the row"""
    out = {}
    for side, lo, hi in (("u", 0, B_max), ("i", B_max, 3 * B_max)):
        k, r = np.asarray(keys[lo:hi]).view(np.uint64), runlen[lo:hi]
        out[side] = {int(k[j] >> np.uint64(32)): [int(x & np.uint64(0xFFFFFFFF)) for x in k[j:j + r[j]]] for j in np.flatnonzero(r > 0)}
    return out
