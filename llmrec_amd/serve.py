"""Serving a trained model: "the k best items for these users", optionally among the items that are eligible NOW.

    rec = Recommender.from_checkpoint(trainer, "ckpt/best.ckpt")
    items, scores = rec.recommend(users, 20, allow_items=in_stock)
    more, _ = rec.recommend(users, 20, allow_items=in_stock, exclude=items)         # the next page

Recommender holds the two embedding tables Trainer.test ranks by and the train CSR; recommend() is ops.score_topk - the evaluation's exact
masked top-K - or, under an allow / deny list, ops.score_topk_filtered: the eligible rows as a dense table, the same sweeps over it, the
ids mapped back (csrc/serve.hip). `exclude` adds one exclusion list PER LISTED USER - what the user bought, saw or dismissed since the graph
was built, what this session has shown, the earlier pages of a result: ops.score_topk_excluded sorts the lists on the device and merges
them with the train rows into the mask the same sweeps read (csrc/exclude.hip). The lists are exact: for every listed user the first k of
{eligible items, minus the user's train row with exclude_seen, minus the user's exclusion list} by (score descending, item id ascending),
the scores the bits of ops.scores.

Not covered: dp.py and the sharded evaluations take neither a filter nor exclusion lists, and the allow-list is one
item set for all users of a call."""
from __future__ import annotations

import sys
from typing import Optional, Tuple

import numpy as np
import torch

from . import ops

_MAX_FILTERS = 4                                                   # ItemFilters kept per Recommender (each holds 2 x n_items int32)


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


def exclusion_csr(exclude, users, n_items: int) -> Optional[Tuple[np.ndarray, np.ndarray]]:
    """Recommender.recommend's `exclude`, normalised on the HOST to one CSR over the listed users: (rowptr int32 [n + 1], colidx int32), row
    q = the list of the q-th listed user, entries in the order given. `users`: the n listed user ids (host integers). Accepted:
      None                               -> None (no lists)
      a dict  user id -> ids             applied to EVERY occurrence of that user; keys that are not listed are ignored
      a TUPLE (rowptr, colidx)           a CSR over the listed users (rowptr [n + 1] from 0 to len(colidx), non-decreasing)
      an array or tensor [n, m]          one row per listed user, -1 padding: what a previous recommend() returned
      any other sequence of n sequences  one per listed user, in order (a list of two lists is this form; the pair is a tuple)
    Negative entries are padding and are dropped; an id >= n_items raises ValueError, as do a wrong row count, non-integer ids and a broken
    rowptr. Pure host code: no device is needed."""
    if exclude is None:
        return None
    users = np.asarray(users, dtype=np.int64).reshape(-1)
    n = users.size
    if isinstance(exclude, dict):
        lists = {int(u): _int_array(v, "exclude[%r]" % (u,)).reshape(-1) for u, v in exclude.items()}
        none = np.zeros(0, np.int64)
        rows = [lists.get(int(u), none) for u in users]
    elif isinstance(exclude, tuple) and len(exclude) == 2:
        rp, ci = _int_array(exclude[0], "exclude rowptr").reshape(-1), _int_array(exclude[1], "exclude colidx").reshape(-1)
        if rp.size != n + 1:
            raise ValueError("exclude: rowptr of %d entries for %d users (n + 1 expected)" % (rp.size, n))
        if rp[0] != 0 or rp[-1] != ci.size or np.any(np.diff(rp) < 0):
            raise ValueError("exclude: rowptr must rise from 0 to len(colidx) = %d without decreasing" % ci.size)
        rows = [ci[a:b] for a, b in zip(rp[:-1], rp[1:])]
    elif isinstance(exclude, (np.ndarray, torch.Tensor)) and exclude.ndim == 2:
        a = _int_array(exclude, "exclude")
        if a.shape[0] != n:
            raise ValueError("exclude: %d rows for %d users" % (a.shape[0], n))
        rows = list(a)
    else:
        if isinstance(exclude, (np.ndarray, torch.Tensor)) or not hasattr(exclude, "__len__"):
            raise ValueError("exclude: a dict, a (rowptr, colidx) tuple, an [n, m] array or a sequence of n id sequences expected")
        if len(exclude) != n:
            raise ValueError("exclude: %d rows for %d users" % (len(exclude), n))
        rows = [_int_array(r, "exclude[%d]" % i).reshape(-1) for i, r in enumerate(exclude)]
    rows = [r[r >= 0] for r in rows]
    top = max((int(r.max()) for r in rows if r.size), default=-1)
    if top >= n_items:
        raise ValueError("exclude: ids must lie in [0, %d) or be negative padding; got %d" % (n_items, top))
    rowptr = np.concatenate([[0], np.cumsum([r.size for r in rows], dtype=np.int64)])
    if rowptr[-1] >= 1 << 31:
        raise ValueError("exclude: %d entries exceed int32 row pointers" % rowptr[-1])
    colidx = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return rowptr.astype(np.int32), colidx.astype(np.int32)


def csr_slice(csr: Tuple[np.ndarray, np.ndarray], a: int, b: int) -> Tuple[np.ndarray, np.ndarray]:
    """Rows [a, b) of a host CSR as a CSR of their own: the row pointers rebased to 0."""
    rp, ci = csr
    return (rp[a:b + 1] - rp[a]).astype(np.int32), ci[rp[a]:rp[b]]


class Recommender:
    def __init__(self, E_u: torch.Tensor, E_i: torch.Tensor, train: Optional[ops.Csr]):
        """E_u [n_users, d], E_i [n_items, d] fp32 on the GPU (CLONED here: a trainer that goes on training does not move them);
        train: the device CSR of the interactions to exclude (ops.Csr, rows ascending), or None."""
        ops._need_gpu(E_u, E_i)
        if E_u.dim() != 2 or E_i.dim() != 2 or E_u.shape[1] != E_i.shape[1]:
            raise ValueError("Recommender: E_u [n_users, d] and E_i [n_items, d] expected, got %s and %s" % (tuple(E_u.shape), tuple(E_i.shape)))
        self.E_u, self.E_i = E_u.detach().clone(), E_i.detach().clone()
        self.n_users, self.n_items = self.E_u.shape[0], self.E_i.shape[0]
        self.train = train
        self._filters = {}                                         # flag bytes -> ops.ItemFilter

    @classmethod
    def from_trainer(cls, trainer) -> "Recommender":
        """The embeddings Trainer.test would rank by now: FusedStep.forward() on the fused routes, the model's no-grad forward in eval mode
        on the per-op path; the train CSR of the drop-in's data_generator.device_state. On a masking route (--mask / --mask_rate > 0) this
        forward is ONE MASKING ROUND, as every evaluation is: it advances the step's round counter."""
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
        data_generator = sys.modules[type(trainer).__module__].data_generator
        return cls(E_u, E_i, data_generator.device_state(E_u.device)["train"])

    @classmethod
    def from_checkpoint(cls, trainer, path: str) -> "Recommender":
        """trainer.load_checkpoint(path) (a file of another configuration fails its fingerprint check), then from_trainer."""
        trainer.load_checkpoint(path)
        return cls.from_trainer(trainer)

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

    def recommend(self, users, k: int, allow_items=None, deny_items=None, exclude_seen: bool = True, chunk: Optional[int] = 65536,
                  exclude=None):
        """(items int64 [n, k], scores float32 [n, k]) for the listed users (any order, repeats allowed): the k best eligible items,
        -1 / -inf behind the last candidate. allow_items / deny_items: id lists or tensors - both given means allowed and not denied;
        exclude_seen: leave out the user's train row; chunk: users per call, which bounds the workspace (the lists do not depend on it;
        None = one call). k <= LLMREC_TOPK_WIDE_MAX (1024).
        exclude: one more exclusion list per listed user, in any form exclusion_csr accepts - a dict user id -> ids, a (rowptr, colidx)
        tuple, an [n, m] array or tensor with -1 padding (the `items` of an earlier call: the next page), or a sequence of n id
        sequences. It is normalised on the host (a device tensor comes to the host once) and sliced per chunk."""
        dev = self.E_u.device
        q = _ids(users, "users", self.n_users, dev)
        filt = self.item_filter(allow_flags(self.n_items, allow_items, deny_items, dev))
        train = self.train if exclude_seen else None
        n = q.numel()
        step = n if not chunk or chunk >= n else int(chunk)
        excl = exclusion_csr(exclude, q.cpu().numpy(), self.n_items) if exclude is not None else None

        def rows(a):
            if excl is None:
                return None
            rp, ci = csr_slice(excl, a, min(a + step, n))
            return torch.from_numpy(rp).to(dev), torch.from_numpy(np.ascontiguousarray(ci)).to(dev)

        parts = [ops.score_topk_excluded(self.E_u, self.E_i, q[a:a + step], train, int(k), rows(a), filt) for a in range(0, n, max(step, 1))]
        if not parts:
            return torch.empty(0, k, dtype=torch.int64, device=dev), torch.empty(0, k, dtype=torch.float32, device=dev)
        idx, sc = (parts[0] if len(parts) == 1 else tuple(torch.cat(p) for p in zip(*parts)))
        return idx.to(torch.int64), sc
