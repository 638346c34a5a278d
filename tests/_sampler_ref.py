"""numpy statement of the device BPR sampler's contract (include/llmrec_hip.h R11: llmrec_sample_bpr, llmrec_sample_batch), vectorised over
the batch. An independent restatement: it imports nothing from llmrec_amd, tests membership of a candidate in a row with a sorted table of
(user, item) keys instead of a per-row binary search, and scales a 32-bit word to [0, n) by integer division instead of a multiply-high.

Stream, as documented:
  Philox4x32-10 (Salmon et al., SC'11), key = (seed low word, seed high word).
  keyed_perm(x, n): 4-round balanced Feistel on 2h bits, h = the smallest h >= 1 with 4^h >= n; round r's function = the low h bits of the
      64-bit word o[1] << 32 | o[0] at counter (R low, R high ^ (0xA5A50000 + r), step low, step high); cycle-walk while the image is >= n.
  slot b of a global batch of B:
      user     = exist_users[keyed_perm(b, n_exist)] if B <= n_exist, else exist_users[(o[1] << 32 | o[0]) mod n_exist] at (b, 0x55AA0001, step)
      positive = row[floor(o[0] * len(row) / 2^32)] at (b, 0x55AA0002, step)
      negative = the first floor(r * n_items / 2^32) that is not in the row, r running over the words of the counters (b, 0x55AA0003 + j, step),
                 j = 0, 1, ..., four words each; after 4096 words the 4096th candidate is returned as it is.
  augmented triples of a slice of B: key = seed ^ 0x9E3779B97F4A7C15; draw a < n_aug takes the slice's user at keyed_perm(a, B); its pair is kept
      iff 0 <= both ids < n_items; kept pairs first, in order of a, zeros behind them; n_valid = B + kept; the step counter becomes step + 1."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
MAX_TRIES = 4096
AUG_KEY_XOR = 0x9E3779B97F4A7C15


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Counter words and key words (anything that broadcasts, values < 2^32) -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(v) for v in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0                      # < 2^64: both factors are below 2^32
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def _steps(step, shape):
    """The step counter (one Python integer, or one per element) as a uint64 array of the given shape."""
    if isinstance(step, np.ndarray):
        return np.broadcast_to(step.astype(np.uint64), shape)
    return np.full(shape, int(step) & (2 ** 64 - 1), dtype=np.uint64)


def _philox(seed, step, c0, c1):
    """The sampler's use of the generator: counter (c0, c1, step low, step high), key (seed low, seed high); step: uint64 array."""
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32_10(c0, c1, step & M32, step >> S32, seed & 0xFFFFFFFF, seed >> 32)


def half_bits(n):
    h = 1
    while 4 ** h < n:
        h += 1
    return h


def keyed_perm(x, n, seed, step):
    """Images of the points x (each < n) under the keyed bijection of [0, n). step: one integer, or a uint64 array with one step per point."""
    x = _u64(x).copy().reshape(-1)
    step = _steps(step, x.shape)
    n = int(n)
    h = np.uint64(half_bits(n))
    mask = np.uint64((1 << int(h)) - 1)
    todo = np.arange(x.size)
    while todo.size:
        L, R = x[todo] >> h, x[todo] & mask
        for r in range(4):
            o = _philox(seed, step[todo], R & M32, (R >> S32) ^ np.uint64(0xA5A50000 + r))
            f = ((o[1].astype(np.uint64) << S32) | o[0].astype(np.uint64)) & mask
            L, R = R, L ^ f
        x[todo] = (L << h) | R
        todo = todo[x[todo] >= np.uint64(n)]
    return x


def _scale(r, n):
    """floor(r * n / 2^32) for 32-bit words r (n <= 2^32); r mod n beyond that."""
    n = int(n)
    if n <= 0xFFFFFFFF:
        return ((r.astype(np.uint64) * np.uint64(n)) // np.uint64(2 ** 32)).astype(np.int64)
    return (r.astype(np.uint64) % np.uint64(n)).astype(np.int64)


def edge_table(rowptr, colidx, n_items):
    """The sorted keys user * n_items + item of all train edges (what sample_bpr tests membership against)."""
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    edge_user = np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))
    return np.unique(edge_user * int(n_items) + colidx)


def _draw(seed, step, b, B, exist_users, n_items, rowptr, colidx, table):
    """Slots b (uint64 array) of the global batches of B triples at the steps `step` (uint64 array, one per slot)."""
    n_exist = exist_users.size
    if B <= n_exist:
        slot = keyed_perm(b, n_exist, seed, step)
    else:
        o = _philox(seed, step, b, 0x55AA0001)
        slot = ((o[1].astype(np.uint64) << S32) | o[0].astype(np.uint64)) % np.uint64(n_exist)   # (bias < n_exist / 2^64)
    users = exist_users[slot.astype(np.int64)]
    start, length = rowptr[users], rowptr[users + 1] - rowptr[users]
    o = _philox(seed, step, b, 0x55AA0002)
    pos = colidx[start + ((o[0].astype(np.uint64) * length.astype(np.uint64)) // np.uint64(2 ** 32)).astype(np.int64)]
    neg = np.zeros(b.size, dtype=np.int64)
    tries = np.zeros(b.size, dtype=np.int64)
    live = np.arange(b.size)                                     # the slots that are still rejecting
    for j in range(MAX_TRIES // 4):
        if not live.size:
            break
        words = _philox(seed, step[live], b[live], 0x55AA0003 + j)   # one refill: four candidates per live slot
        sel = np.arange(live.size)                               # positions within this refill of the slots still live
        for w in words:
            cand = _scale(w[sel], n_items)
            neg[live] = cand
            tries[live] += 1
            in_row = np.isin(users[live] * n_items + cand, table)
            live, sel = live[in_row], sel[in_row]
            if not live.size:
                break
    return users, pos, neg, tries


def sample_bpr(seed, step, exist_users, n_items, rowptr, colidx, B, first=0, count=None, return_tries=False, table=None):
    """Slots [first, first + count) of the global batch of B triples of (seed, step): int64 arrays (users, pos, neg);
    with return_tries also the number of negative candidates each slot looked at. table: edge_table(...) if the caller keeps one."""
    exist_users = np.asarray(exist_users, dtype=np.int64)
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    count = B - first if count is None else count
    if table is None:
        table = edge_table(rowptr, colidx, n_items)
    b = np.arange(first, first + count, dtype=np.uint64)
    out = _draw(seed, _steps(step, b.shape), b, B, exist_users, int(n_items), rowptr, colidx, table)
    return out if return_tries else out[:3]


def sample_bpr_steps(seed, steps, exist_users, n_items, rowptr, colidx, B):
    """The whole batches of several steps at once: three int64 arrays [len(steps), B] (row s = sample_bpr(seed, steps[s], ...))."""
    exist_users = np.asarray(exist_users, dtype=np.int64)
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    steps = np.asarray([int(t) & (2 ** 64 - 1) for t in steps], dtype=np.uint64)
    b = np.tile(np.arange(B, dtype=np.uint64), steps.size)
    out = _draw(seed, np.repeat(steps, B), b, B, exist_users, int(n_items), rowptr, colidx, edge_table(rowptr, colidx, n_items))
    return tuple(t.reshape(steps.size, B) for t in out[:3])


def sample_batch(seed, step, exist_users, n_items, rowptr, colidx, B_global, slice_begin, B, n_aug, aug_pos=None, aug_neg=None):
    """What one llmrec_sample_batch launch leaves behind: (users, pos, neg) of B + n_aug entries, n_valid, the next step counter."""
    u, p, q = sample_bpr(seed, step, exist_users, n_items, rowptr, colidx, B_global, slice_begin, B)
    users, pos, neg = (np.concatenate([t, np.zeros(n_aug, dtype=np.int64)]) for t in (u, p, q))
    kept = 0
    if n_aug:
        aug_pos, aug_neg = np.asarray(aug_pos, dtype=np.int64), np.asarray(aug_neg, dtype=np.int64)
        key = (int(seed) ^ AUG_KEY_XOR) & (2 ** 64 - 1)
        drawn = u[keyed_perm(np.arange(n_aug), B, key, step).astype(np.int64)]
        ap, an = aug_pos[drawn], aug_neg[drawn]
        ok = (ap >= 0) & (ap < n_items) & (an >= 0) & (an < n_items)
        kept = int(ok.sum())
        users[B:B + kept], pos[B:B + kept], neg[B:B + kept] = drawn[ok], ap[ok], an[ok]
    return users, pos, neg, B + kept, (int(step) + 1) & (2 ** 64 - 1)
