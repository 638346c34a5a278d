"""Serving a trained model: "the k best items for these users", optionally among the items that are eligible NOW.

    rec = Recommender.from_checkpoint(trainer, "ckpt/best.ckpt")
    items, scores = rec.recommend(users, 20, allow_items=in_stock)
    more, _ = rec.recommend(users, 20, allow_items=in_stock, exclude=items)         # the next page

Recommender holds the two embedding tables Trainer.test ranks by and the train CSR; recommend() is ops.score_topk - the evaluation's exact
masked top-K - or, under an allow / deny list, ops.score_topk_filtered: the eligible rows as a dense table, the same sweeps over it, the
ids mapped back (csrc/serve.hip). `exclude` adds one exclusion list PER LISTED USER - what the user bought, saw or dismissed since the graph
was built, what this session has shown, the earlier pages of a result: ops.score_topk_excluded sorts the lists on the device and merges
them with the train rows into the mask the same sweeps read (the same pipeline of csrc/serve.hip, with the exclusion stage of csrc/exclude.hip). The lists are exact: for every listed user the first k of
{eligible items, minus the user's train row with exclude_seen, minus the user's exclusion list} by (score descending, item id ascending),
the scores the bits of ops.scores.

Users who are not rows of the graph (fold_in=True at construction): rec.recommend_new(histories, 20) / rec.embed_new(histories) embed
each item history with the trained model, the item side held fixed (ops.FoldInTables / ops.fold_in_users, csrc/foldin.hip), and rank
the new rows by the same exact top-K, the history's own items excluded.

Per-request candidate lists - the output of a retrieval stage, a campaign's items, a shop's shelf: rec.rank(users, candidates, 20) /
rec.rank_new(histories, candidates, 20) return the k best of each user's OWN list by the same order and the same score bits
(ops.score_topk_candidates, csrc/candidates.hip: only the listed pairs are scored, two radix sorts select; no sweep of the catalogue). A
list is a set; allow / deny lists, the train row and `exclude` remove from it as they do for recommend().

Quotas - "at most m items of any one brand, seller, category or series in a list": group_of= (one group id per item, negative = none) and
per_group= (one cap, or one per group; 0 removes a group) on all four calls. The list is the greedy walk down the user's ranking that takes
an item while its group has room; equivalently an item is kept if fewer than cap(group) survivors of its group stand before it, and the
list is the first k kept items. rank / rank_new walk the ranking of the user's own list in the last launch of the candidate pipeline
(ops.score_topk_candidates_capped, csrc/quota.hip). recommend / recommend_new are exact over the whole catalogue in two rounds: round 1
fetches the first min(1024, overfetch * k) items of every ranking with the sweeps and walks them - a prefix of the ranking gives a prefix
of the walk, so a list that comes back full is final, and so is the list of a user whose fetched row was not full (it held every
survivor); round 2 walks the whole catalogue for the remaining users alone. The lists do not depend on `overfetch`; rec.last_quota says how
many users round 2 served.

Not covered: fold-in moves no item embedding and adds no user to the graph; dp.py and the sharded evaluations take
neither a filter nor exclusion or candidate lists nor quotas; recommend()'s allow-list is one item set for all users of a call (per-user
sets: rank); under quotas k <= 1024, and recommend()'s two rounds read one flag vector back, so that route is not capturable."""
from __future__ import annotations

import sys
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import ops

_MAX_FILTERS = 4                                                   # ItemFilters kept per Recommender (each holds 2 x n_items int32)
ROUND2_PAIRS = 1 << 23                                             # recommend() under quotas: (query, item) pairs per whole-catalogue call of round 2
#                                                                    (about 25 bytes of workspace per pair + 32 MiB: some 240 MiB)


def _ids(ids, what: str, bound: int, device) -> torch.Tensor:
    """An id list (sequence, numpy array or tensor) as an int64 tensor on `device`; an id outside [0, bound) raises ValueError (a tensor
    on the device costs one host read for that check)."""
    if isinstance(ids, torch.Tensor):
        t = ids.reshape(-1).to(torch.int64)
    else:
        a = np.asarray(ids)
        if a.size and a.dtype.kind not in "iu":
            raise ValueError("%s: integer ids expected, got %s" % (what, a.dtype))
        t = torch.from_numpy(a.reshape(-1).astype(np.int64))
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= bound):
        raise ValueError("%s: ids must lie in [0, %d); got %d .. %d" % (what, bound, int(t.min()), int(t.max())))
    return t.to(device)


def allow_flags(n_items: int, allow_items=None, deny_items=None, device="cpu") -> Optional[torch.Tensor]:
    """The uint8 flag vector [n_items] of an allow list and / or a deny list, built on `device`: eligible = (allowed, or every item without
    an allow list) and not denied. Neither list: None (no filter). Ids outside [0, n_items) raise ValueError; repeats are fine."""
    if allow_items is None and deny_items is None:
        return None
    if allow_items is None:
        flags = torch.ones(n_items, dtype=torch.uint8, device=device)
    else:
        flags = torch.zeros(n_items, dtype=torch.uint8, device=device)
        flags[_ids(allow_items, "allow_items", n_items, device)] = 1
    if deny_items is not None:
        flags[_ids(deny_items, "deny_items", n_items, device)] = 0
    return flags


def _int_array(a, what: str) -> np.ndarray:
    """ids of any accepted container as an int64 numpy array (a device tensor comes to the host); non-integers raise ValueError."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.size and a.dtype.kind not in "iu":
        raise ValueError("%s: integer ids expected, got %s" % (what, a.dtype))
    return a.astype(np.int64)


def exclusion_csr(exclude, users, n_items: int, what: str = "exclude") -> Optional[Tuple[np.ndarray, np.ndarray]]:
    """Recommender.recommend's `exclude`, normalised on the HOST to one CSR over the listed users: (rowptr int32 [n + 1], colidx int32), row
    q = the list of the q-th listed user, entries in the order given. `users`: the n listed user ids (host integers). Accepted:
      None                               -> None (no lists)
      a dict  user id -> ids             applied to EVERY occurrence of that user; keys that are not listed are ignored
      a TUPLE (rowptr, colidx)           a CSR over the listed users (rowptr [n + 1] from 0 to len(colidx), non-decreasing)
      an array or tensor [n, m]          one row per listed user, -1 padding: what a previous recommend() returned
      any other sequence of n sequences  one per listed user, in order (a list of two lists is this form; the pair is a tuple)
    Negative entries are padding and are dropped; an id >= n_items raises ValueError, as do a wrong row count, non-integer ids and a broken
    rowptr. `what` names the argument in the messages. Pure host code: no device is needed."""
    if exclude is None:
        return None
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    n = users.size
    if isinstance(exclude, dict):
        lists = {int(u): _int_array(v, "%s[%r]" % (what, u)).reshape(-1) for u, v in exclude.items()}
        none = np.zeros(0, np.int64)
        rows = [lists.get(int(u), none) for u in users]
    elif isinstance(exclude, tuple) and len(exclude) == 2:
        rp, ci = _int_array(exclude[0], what + " rowptr").reshape(-1), _int_array(exclude[1], what + " colidx").reshape(-1)
        if rp.size != n + 1:
            raise ValueError("%s: rowptr of %d entries for %d users (n + 1 expected)" % (what, rp.size, n))
        if rp[0] != 0 or rp[-1] != ci.size or np.any(np.diff(rp) < 0):
            raise ValueError("%s: rowptr must rise from 0 to len(colidx) = %d without decreasing" % (what, ci.size))
        rows = [ci[a:b] for a, b in zip(rp[:-1], rp[1:])]
    elif isinstance(exclude, (np.ndarray, torch.Tensor)) and exclude.ndim == 2:
        a = _int_array(exclude, what)
        if a.shape[0] != n:
            raise ValueError("%s: %d rows for %d users" % (what, a.shape[0], n))
        rows = list(a)
    else:
        if isinstance(exclude, (np.ndarray, torch.Tensor)) or not hasattr(exclude, "__len__"):
            raise ValueError("%s: a dict, a (rowptr, colidx) tuple, an [n, m] array or a sequence of n id sequences expected" % what)
        if len(exclude) != n:
            raise ValueError("%s: %d rows for %d users" % (what, len(exclude), n))
        rows = [_int_array(r, "%s[%d]" % (what, i)).reshape(-1) for i, r in enumerate(exclude)]
    rows = [r[r >= 0] for r in rows]
    top = max((int(r.max()) for r in rows if r.size), default=-1)
    if top >= n_items:
        raise ValueError("%s: ids must lie in [0, %d) or be negative padding; got %d" % (what, n_items, top))
    rowptr = np.concatenate([[0], np.cumsum([r.size for r in rows], dtype=np.int64)])
    if rowptr[-1] >= 1 << 31:
        raise ValueError("%s: %d entries exceed int32 row pointers" % (what, rowptr[-1]))
    colidx = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return rowptr.astype(np.int32), colidx.astype(np.int32)


def group_quota(group_of, per_group, n_items: int) -> Optional[Tuple[np.ndarray, object, int]]:
    """Recommender's `group_of` / `per_group`, normalised on the HOST: None without both, else (item_group int32 [n_items] with -1 = no group,
    cap, n_groups) - cap an int >= 1 for every group, or an int32 array [n_groups] of caps >= 0 (0 removes the group).
    group_of: an array or tensor of n_items integers, negative = no group. per_group: an int >= 1, or a sequence of n_groups ints >= 0 that
    covers every group id in group_of (with an int, n_groups is the largest group id + 1). One argument without the other raises
    ValueError, as do a wrong length, non-integer values and a negative cap. Pure host code: no device is needed."""
    if group_of is None and per_group is None:
        return None
    if group_of is None or per_group is None:
        raise ValueError("group_of and per_group go together: %s is missing" % ("group_of" if group_of is None else "per_group"))
    g = _int_array(group_of, "group_of")
    if g.ndim != 1 or g.size != n_items:
        raise ValueError("group_of: %d integers expected (one per item), got shape %s" % (n_items, tuple(g.shape)))
    top = int(g.max()) if g.size else -1
    if top >= (1 << 31) - 1:
        raise ValueError("group_of: group ids must lie below 2^31 - 1; got %d" % top)
    group = np.where(g < 0, -1, g).astype(np.int32)
    if isinstance(per_group, (bool, np.bool_)):
        raise ValueError("per_group: an integer or a sequence of integers expected, got %r" % (per_group,))
    if isinstance(per_group, (int, np.integer)):
        if per_group < 1:
            raise ValueError("per_group: one cap for every group must be at least 1; got %d" % per_group)
        return group, int(per_group), max(top + 1, 1)
    if isinstance(per_group, (float, np.floating)) or isinstance(per_group, (str, bytes, dict)) or \
            not (hasattr(per_group, "__len__") or isinstance(per_group, torch.Tensor)):
        raise ValueError("per_group: an integer or a sequence of integers expected, got %r" % (per_group,))
    caps = _int_array(per_group, "per_group")
    if caps.ndim != 1 or caps.size < 1 or caps.size <= top:
        raise ValueError("per_group: one cap per group expected (group ids reach %d), got shape %s" % (top, tuple(caps.shape)))
    if caps.min() < 0:
        raise ValueError("per_group: a cap must not be negative; got %d" % int(caps.min()))
    return group, np.minimum(caps, (1 << 31) - 1).astype(np.int32), int(caps.size)


def csr_rows(csr: Tuple[np.ndarray, np.ndarray], rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The listed rows of a host CSR, in the order listed, as a CSR of their own."""
    rp, ci = csr
    rows = np.asarray(rows, dtype=np.int64)
    lens = (rp[rows + 1] - rp[rows]).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(lens)])
    take = np.repeat(rp[rows].astype(np.int64) - rowptr[:-1], lens) + np.arange(rowptr[-1])
    return rowptr.astype(np.int32), ci[take].astype(np.int32)


def csr_slice(csr: Tuple[np.ndarray, np.ndarray], a: int, b: int) -> Tuple[np.ndarray, np.ndarray]:
    """Rows [a, b) of a host CSR as a CSR of their own: the row pointers rebased to 0."""
    rp, ci = csr
    return (rp[a:b + 1] - rp[a]).astype(np.int32), ci[rp[a]:rp[b]]


def history_csr(histories, n_items: int, n: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Recommender.recommend_new's `histories`, normalised on the HOST: (rowptr int32 [n + 1], colidx int32), row q = the item set of new
    user q - sorted, unique, in range. A history is a set, as a row of the binary adjacency is, and sorting makes the embedding
    independent of the order given, bit for bit. The container forms of exclusion_csr, except that a dict is keyed by POSITION: key q is
    new user q, and without `n` the dict has max key + 1 rows. n: the row count something else fixes (id_rows); another count raises
    ValueError, as do a dict key outside [0, n), an id >= n_items and non-integer ids. Negative ids are padding."""
    if histories is None:
        raise ValueError("histories: a dict, a (rowptr, colidx) tuple, an [n, m] array or a sequence of n id sequences expected")
    if isinstance(histories, dict):
        keys = [int(q) for q in histories]
        rows = (max(keys) + 1 if keys else 0) if n is None else int(n)
        if keys and (min(keys) < 0 or max(keys) >= rows):
            raise ValueError("histories: a dict is keyed by position, keys must lie in [0, %d); got %d .. %d" % (rows, min(keys), max(keys)))
    elif isinstance(histories, tuple) and len(histories) == 2:
        rows = _int_array(histories[0], "histories rowptr").size - 1
    elif hasattr(histories, "__len__") and not (isinstance(histories, (np.ndarray, torch.Tensor)) and histories.ndim != 2):
        rows = len(histories)
    else:
        rows = 0                                                   # (not a container: exclusion_csr names what is expected)
    if n is not None and rows != int(n):
        raise ValueError("histories: %d rows for %d new users" % (rows, n))
    rp, ci = exclusion_csr(histories, np.arange(rows), n_items, what="histories")
    q = np.repeat(np.arange(rows, dtype=np.int64), np.diff(rp))
    key = np.unique(q * n_items + ci)                              # sorted by (row, id), repeats collapsed
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key // n_items, minlength=rows), dtype=np.int64)])
    return rowptr.astype(np.int32), (key % n_items).astype(np.int32)


def csr_join(a: Tuple[np.ndarray, np.ndarray], b: Optional[Tuple[np.ndarray, np.ndarray]]) -> Tuple[np.ndarray, np.ndarray]:
    """Row q of the result = row q of `a` followed by row q of `b` (two host CSRs over the same rows; b None: a)."""
    if b is None:
        return a
    (ra, ca), (rb, cb) = a, b
    n = ra.size - 1
    q = np.concatenate([np.repeat(np.arange(n), np.diff(ra)), np.repeat(np.arange(n), np.diff(rb))])
    col = np.concatenate([ca, cb])[np.argsort(q, kind="stable")]
    return (ra.astype(np.int64) + rb).astype(np.int32), col.astype(np.int32)


class _Side(NamedTuple):
    """The query side of a request: who is asked for (Recommender._graph_side, ._new_side)."""
    n: int                                                         # queries
    keys: Callable[[], np.ndarray]                                 # the n host ids that dict-form lists are keyed by
    rows: Callable[[int, int], tuple]                              # (a, b) -> (Eu, query ids into Eu, train CSR or None) of queries [a, b)
    gone: Optional[Tuple[np.ndarray, np.ndarray]] = None           # a host CSR over the queries to leave out in front of `exclude`: a new user's history


_CATALOGUE = object()                                              # Recommender._serve's `candidates` of recommend / recommend_new: no lists


class Recommender:
    def __init__(self, E_u: torch.Tensor, E_i: torch.Tensor, train: Optional[ops.Csr], fold_in: Optional[ops.FoldInTables] = None,
                 iu: Optional[ops.Csr] = None):
        """E_u [n_users, d], E_i [n_items, d] fp32 on the GPU (CLONED here: a trainer that goes on training does not move them);
        train: the device CSR of the interactions to exclude (ops.Csr, rows ascending), or None. fold_in: the item-side tables
        recommend_new / embed_new gather (ops.FoldInTables, with the rates), iu: the item-side CSR they were built over - both None:
        only users of the graph can be served."""
        ops._need_gpu(E_u, E_i)
        if E_u.dim() != 2 or E_i.dim() != 2 or E_u.shape[1] != E_i.shape[1]:
            raise ValueError("Recommender: E_u [n_users, d] and E_i [n_items, d] expected, got %s and %s" % (tuple(E_u.shape), tuple(E_i.shape)))
        self.E_u, self.E_i = E_u.detach().clone(), E_i.detach().clone()
        self.n_users, self.n_items = self.E_u.shape[0], self.E_i.shape[0]
        self.train = train
        if fold_in is not None and (fold_in.n_items != self.n_items or fold_in.d != self.E_i.shape[1]):
            raise ValueError("Recommender: fold-in tables of %d items x d = %d beside E_i %s" % (fold_in.n_items, fold_in.d, tuple(self.E_i.shape)))
        self.fold_in, self.iu = fold_in, iu
        self._filters = {}                                         # flag bytes -> ops.ItemFilter

    @classmethod
    def from_trainer(cls, trainer, fold_in: bool = False) -> "Recommender":
        """The embeddings Trainer.test would rank by now: FusedStep.forward() on the fused routes, the model's no-grad forward in eval mode
        on the per-op path; the train CSR of the drop-in's data_generator.device_state. On a masking route (--mask / --mask_rate > 0) this
        forward is ONE MASKING ROUND, as every evaluation is: it advances the step's round counter.
        fold_in: also build the item-side tables of recommend_new / embed_new from the model's parameters (ops.FoldInTables.from_model:
        on either route, nothing is read from the fused step's buffers) and keep the item-side CSR and the rates. A masking
        configuration is refused: its features are redrawn every forward, and there is no one item side to hold fixed."""
        module = sys.modules[type(trainer).__module__]
        if fold_in and (module.args.mask or module.args.mask_rate != 0):
            raise RuntimeError("Recommender: fold_in is refused under --mask / --mask_rate != 0 (every forward is a masking round)")
        if trainer.model_mm.training:
            trainer.model_mm.eval()
        fused = trainer._fused_step()
        with torch.no_grad():
            if fused:
                fused.forward()
                E_u, E_i = fused.E_u, fused.E_i
            else:
                E_u, E_i, *_ = trainer.model_mm(trainer.ui_graph, trainer.iu_graph, trainer.image_ui_graph, trainer.image_iu_graph,
                                                trainer.text_ui_graph, trainer.text_iu_graph)
        tables = iu = None
        if fold_in:
            a = module.args
            tables = ops.FoldInTables.from_model(trainer.model_mm, trainer.ui_graph, trainer.iu_graph, (a.model_cat_rate, a.user_cat_rate, a.item_cat_rate))
            iu = ops.operand_from_sparse_tensor(trainer.iu_graph).fwd
        return cls(E_u, E_i, module.data_generator.device_state(E_u.device)["train"], tables, iu)

    @classmethod
    def from_checkpoint(cls, trainer, path: str, fold_in: bool = False) -> "Recommender":
        """trainer.load_checkpoint(path) (a file of another configuration fails its fingerprint check), then from_trainer."""
        trainer.load_checkpoint(path)
        return cls.from_trainer(trainer, fold_in=fold_in)

    def item_filter(self, flags: Optional[torch.Tensor]) -> Optional[ops.ItemFilter]:
        """The ItemFilter of a flag vector, cached on the vector's CONTENT (its bytes come to the host once per call to be compared; a new
        content costs the build and its one host read)."""
        if flags is None:
            return None
        key = flags.cpu().numpy().tobytes()
        filt = self._filters.pop(key, None)
        if filt is None:
            if len(self._filters) >= _MAX_FILTERS:
                self._filters.pop(next(iter(self._filters)))       # the least recently used
            filt = ops.ItemFilter(flags)
        self._filters[key] = filt                                  # (most recently used last)
        return filt

    # -----------------------------------------------------------------------------------------
    # A request = a query side (who asks: _Side) + what to rank among and what to leave out (_serve). The four public calls differ in
    # the side - users of the graph or new users - and in whether each query brings a candidate list; everything else is one driver.
    # -----------------------------------------------------------------------------------------
    def _graph_side(self, users, exclude_seen: bool) -> _Side:
        """The listed users of the graph: their rows of E_u and, with exclude_seen, the train CSR. Lists are keyed by user id."""
        q = _ids(users, "users", self.n_users, self.E_u.device)
        train = self.train if exclude_seen else None
        return _Side(q.numel(), lambda: q.cpu().numpy(), lambda a, b: (self.E_u, q[a:b], train))

    def _new_side(self, histories, id_rows, exclude_history: bool) -> _Side:
        """Users who are not rows of the graph: each chunk is embedded from its histories when it is asked for and queried as rows
        0 .. b - a of that table; there is no train CSR, the history is what exclude_history leaves out. Lists are keyed by position."""
        hist, ids = self._histories(histories, id_rows)
        n, dev = hist[0].size - 1, self.E_i.device
        return _Side(n, lambda: np.arange(n), lambda a, b: (self._embed(hist, ids, a, b), torch.arange(b - a, device=dev), None),
                     hist if exclude_history else None)

    def _on_device(self, csr, take, *at):
        """take(csr, *at) - csr_slice or csr_rows of a host CSR - on the device; None stays None."""
        if csr is None:
            return None
        rp, ci = take(csr, *at)
        dev = self.E_i.device
        return torch.from_numpy(rp).to(dev), torch.from_numpy(np.ascontiguousarray(ci)).to(dev)

    def _serve(self, side: _Side, k: int, allow_items, deny_items, exclude, chunk, candidates=_CATALOGUE, group_of=None, per_group=None,
               overfetch=None):
        """One request, for every public call: the filter, the host CSRs of `exclude` (behind the side's own history, if it leaves one out)
        and of `candidates`, the quota, then per chunk of `chunk` queries the slices of those CSRs on the device and one of the routes
          the catalogue              ops.score_topk_excluded (the sweeps)
          candidate lists            ops.score_topk_candidates, under a quota ops.score_topk_candidates_capped
          the catalogue under quota  the two rounds of _recommend_capped
        and the parts joined: (items int64 [n, k], scores float32 [n, k])."""
        dev, k, n = self.E_i.device, int(k), side.n
        filt = self.item_filter(allow_flags(self.n_items, allow_items, deny_items, dev))
        if candidates is None:
            raise ValueError("candidates: a dict, a (rowptr, colidx) tuple, an [n, m] array or a sequence of n id sequences expected")
        keys = side.keys() if exclude is not None or candidates is not _CATALOGUE else None          # (users on the device: one host read)
        cand = exclusion_csr(candidates, keys, self.n_items, what="candidates") if candidates is not _CATALOGUE else None
        excl = exclusion_csr(exclude, keys, self.n_items)
        if side.gone is not None:
            excl = csr_join(side.gone, excl)
        quota = group_quota(group_of, per_group, self.n_items)
        if quota is not None:
            group, cap, n_groups = quota
            group, cap = torch.from_numpy(group).to(dev), cap if isinstance(cap, int) else torch.from_numpy(cap).to(dev)
            capped = lambda Eu, qu, train, c, e, f: ops.score_topk_candidates_capped(Eu, self.E_i, qu, train, k, c, group, cap, e, f, n_groups=n_groups)
            two_rounds = self._recommend_capped(n, k, overfetch, excl, filt, capped) if cand is None else None
        step = n if not chunk or chunk >= n else int(chunk)
        parts = []
        for a in range(0, n, max(step, 1)):
            b = min(a + step, n)
            Eu, qu, train = side.rows(a, b)
            c, e = self._on_device(cand, csr_slice, a, b), self._on_device(excl, csr_slice, a, b)
            if quota is not None:
                parts.append(two_rounds(Eu, qu, train, e, a) if c is None else capped(Eu, qu, train, c, e, filt))
            elif c is None:
                parts.append(ops.score_topk_excluded(Eu, self.E_i, qu, train, k, e, filt))
            else:
                parts.append(ops.score_topk_candidates(Eu, self.E_i, qu, train, k, c, e, filt))
        if not parts:
            return torch.empty(0, k, dtype=torch.int64, device=dev), torch.empty(0, k, dtype=torch.float32, device=dev)
        idx, sc = parts[0] if len(parts) == 1 else tuple(torch.cat(p) for p in zip(*parts))
        return idx.to(torch.int64), sc

    def _recommend_capped(self, n: int, k: int, overfetch, excl, filt, capped):
        """recommend / recommend_new under quotas, exact over the whole catalogue: the route f(Eu, query list, train CSR or None, e, a) of
        the chunk of queries that starts at query a, e its exclusion rows on the device. excl: the host exclusion CSR over all n queries,
        or None; capped: ops.score_topk_candidates_capped with the quota bound. Per chunk:
          round 1  the first K1 = min(1024, overfetch * k) ids of every ranking (ops.score_topk_excluded: the sweeps), then those rows, -1
                   padding included, as candidate rows of ops.score_topk_candidates_capped. A prefix of the ranking gives a prefix of the
                   greedy walk, so a capped list that came back FULL is final; and a fetched row that was NOT full held every survivor,
                   so its capped list is final too. Such queries are settled. Finding the others costs one host read.
          round 2  the unsettled queries alone: the capped op with the whole catalogue as each query's candidate row, with the train rows,
                   the exclusion rows and the filter; at most ROUND2_PAIRS (query, item) pairs per call. Its lists replace round 1's.
        The lists therefore do not depend on overfetch or on the chunk. self.last_quota counts the queries and those sent to round 2."""
        dev = self.E_i.device
        top = ops.CONST["LLMREC_TOPK_WIDE_MAX"]
        if k < 1 or k > top:
            raise ValueError("k = %d: under quotas 1 <= k <= %d" % (k, top))
        if isinstance(overfetch, bool) or not isinstance(overfetch, (int, np.integer)) or overfetch < 1:
            raise ValueError("overfetch: an integer >= 1 expected, got %r" % (overfetch,))
        K1 = min(top, int(overfetch) * k)
        self.last_quota = {"queries": n, "round2": 0}
        every = torch.arange(self.n_items, dtype=torch.int32, device=dev)
        per_call = max(1, ROUND2_PAIRS // self.n_items)

        def chunk(Eu, qu, train, e, a):
            fetched, _ = ops.score_topk_excluded(Eu, self.E_i, qu, train, K1, e, filt)
            rows = torch.arange(qu.numel() + 1, dtype=torch.int32, device=dev) * K1, fetched.reshape(-1)
            idx, sc = capped(Eu, qu, None, rows, None, None)
            unsettled = ((idx[:, k - 1] < 0) & (fetched[:, K1 - 1] >= 0)).nonzero().reshape(-1)
            todo = unsettled.cpu().numpy()                         # (the one host read)
            self.last_quota["round2"] += int(todo.size)
            for s in range(0, todo.size, per_call):
                u = unsettled[s:s + per_call]
                m = u.numel()
                whole = torch.arange(m + 1, dtype=torch.int32, device=dev) * self.n_items, every.repeat(m)
                idx[u], sc[u] = capped(Eu, qu[u], train, whole, self._on_device(excl, csr_rows, a + todo[s:s + per_call]), filt)
            return idx, sc
        return chunk

    def recommend(self, users, k: int, allow_items=None, deny_items=None, exclude_seen: bool = True, chunk: Optional[int] = 65536,
                  exclude=None, group_of=None, per_group=None, overfetch: int = 2):
        """(items int64 [n, k], scores float32 [n, k]) for the listed users (any order, repeats allowed): the k best eligible items,
        -1 / -inf behind the last candidate. allow_items / deny_items: id lists or tensors - both given means allowed and not denied;
        exclude_seen: leave out the user's train row; chunk: users per call, which bounds the workspace (the lists do not depend on it;
        None = one call). k <= LLMREC_TOPK_WIDE_MAX (1024).
        exclude: one more exclusion list per listed user, in any form exclusion_csr accepts - a dict user id -> ids, a (rowptr, colidx)
        tuple, an [n, m] array or tensor with -1 padding (the `items` of an earlier call: the next page), or a sequence of n id
        sequences. It is normalised on the host (a device tensor comes to the host once) and sliced per chunk.
        group_of / per_group (both or neither): quotas - group_of[i] is the group of item i (n_items integers, negative = no group),
        per_group the cap: an int >= 1 for every group or one int >= 0 per group (group_quota). Of every group a list then holds at most
        its cap: the greedy walk down the user's ranking that takes an item while its group has room - exactly, over the whole catalogue,
        in two rounds (_recommend_capped). overfetch: round 1 looks at the first min(1024, overfetch * k) items of each ranking; the lists
        do not depend on it, only the number of users who need round 2 (self.last_quota = {"queries": n, "round2": r} after the call)."""
        return self._serve(self._graph_side(users, exclude_seen), k, allow_items, deny_items, exclude, chunk, _CATALOGUE, group_of, per_group,
                           overfetch)

    def rank(self, users, candidates, k: int, allow_items=None, deny_items=None, exclude_seen: bool = True, exclude=None,
             chunk: Optional[int] = 65536, group_of=None, per_group=None):
        """(items int64 [n, k], scores float32 [n, k]) for the listed users (any order, repeats allowed): the k best of each user's OWN
        candidate list, -1 / -inf behind the last candidate (ops.score_topk_candidates: only the listed pairs are scored). candidates: one
        id list per listed user, in any form exclusion_csr accepts - a dict user id -> ids (a listed user without a key has an empty
        list: its row comes back all -1), a (rowptr, colidx) tuple, an [n, m] array or tensor with -1 padding, a sequence of n id
        sequences; a list is a SET: order and repeats do not matter, bit for bit. allow_items / deny_items / exclude_seen / exclude /
        chunk: as for recommend (an ineligible, seen or excluded candidate is left out). Any k >= 1.
        group_of / per_group: quotas, as for recommend - the greedy walk down the ranking of the user's own list
        (ops.score_topk_candidates_capped; then k <= 1024)."""
        return self._serve(self._graph_side(users, exclude_seen), k, allow_items, deny_items, exclude, chunk, candidates, group_of, per_group)

    def recommend_new(self, histories, k: int, allow_items=None, deny_items=None, exclude_history: bool = True, exclude=None, id_rows=None,
                      chunk: Optional[int] = 65536, group_of=None, per_group=None, overfetch: int = 2):
        """recommend() for users who are not rows of the graph: (items int64 [n, k], scores float32 [n, k]) for n item histories, the k
        best eligible items by (score descending, item id ascending), -1 / -inf behind the last candidate, the scores the bits of
        ops.scores(embed_new(histories, id_rows), E_i, arange(n)). exclude_history: leave out the history's own items; exclude: one more
        list per new user, in any form exclusion_csr accepts (a dict is keyed by position here). allow_items / deny_items / chunk: as
        for recommend, as are group_of / per_group / overfetch (quotas, exact in two rounds). Needs fold_in=True at construction."""
        return self._serve(self._new_side(histories, id_rows, exclude_history), k, allow_items, deny_items, exclude, chunk, _CATALOGUE, group_of,
                           per_group, overfetch)

    def rank_new(self, histories, candidates, k: int, allow_items=None, deny_items=None, exclude_history: bool = True, exclude=None,
                 id_rows=None, chunk: Optional[int] = 65536, group_of=None, per_group=None):
        """rank() for users who are not rows of the graph, as recommend_new is to recommend: n item histories, one candidate list per new
        user (a dict is keyed by position here), the scores the bits of ops.scores(embed_new(histories, id_rows), E_i, arange(n)).
        exclude_history: leave out the history's own items. group_of / per_group: quotas, as for rank. Needs fold_in=True at
        construction."""
        return self._serve(self._new_side(histories, id_rows, exclude_history), k, allow_items, deny_items, exclude, chunk, candidates, group_of,
                           per_group)

    def _tables(self) -> ops.FoldInTables:
        if self.fold_in is None:
            raise RuntimeError("Recommender: built without fold_in=True - Recommender.from_trainer / from_checkpoint(..., fold_in=True) "
                               "build the item-side tables that new users are embedded from")
        return self.fold_in

    def _histories(self, histories, id_rows) -> Tuple[Tuple[np.ndarray, np.ndarray], Optional[torch.Tensor]]:
        """(history_csr of `histories`, `id_rows` as float32 [n, d] on the device or None); without fold-in tables the RuntimeError of
        _tables comes before anything else."""
        self._tables()
        ids = id_rows
        if ids is not None:
            ids = torch.as_tensor(ids).to(device=self.E_i.device, dtype=torch.float32)
            if ids.dim() != 2 or ids.shape[1] != self.E_i.shape[1]:
                raise ValueError("id_rows: [n, %d] expected, got %s" % (self.E_i.shape[1], tuple(ids.shape)))
            ids = ids.contiguous()
        return history_csr(histories, self.n_items, None if ids is None else ids.shape[0]), ids

    def _embed(self, hist: Tuple[np.ndarray, np.ndarray], id_rows: Optional[torch.Tensor], a: int, b: int) -> torch.Tensor:
        return ops.fold_in_users(self._tables(), *self._on_device(hist, csr_slice, a, b), id_rows=id_rows[a:b] if id_rows is not None else None)

    def embed_new(self, histories, id_rows=None) -> torch.Tensor:
        """E_new float32 [n, d]: the embeddings of n users who are not rows of the graph, from their item histories - what the trained
        model's forward gives a user with that row of the adjacency, the item side held fixed (ops.fold_in_users). histories: any form
        history_csr accepts (a history is a SET: order and repeats do not matter). id_rows [n, d]: the users' own id rows - a new
        user has none: zeros (None)."""
        hist, ids = self._histories(histories, id_rows)
        return self._embed(hist, ids, 0, hist[0].size - 1)
