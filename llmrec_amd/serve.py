"""Serving a trained model: "the k best items for these users", optionally among the items that are eligible NOW.

    rec = Recommender.from_checkpoint(trainer, "ckpt/best.ckpt")
    items, scores = rec.recommend(users, 20, allow_items=in_stock)

Recommender holds the two embedding tables Trainer.test ranks by and the train CSR; recommend() is ops.score_topk - the evaluation's exact
masked top-K - or, under an allow / deny list, ops.score_topk_filtered: the eligible rows as a dense table, the same sweeps over it, the
ids mapped back (csrc/serve.hip). The lists are exact: for every user the first k of {eligible items, minus the user's train row with
exclude_seen} by (score descending, item id ascending), the scores the bits of ops.scores.

Not covered: dp.py and the sharded evaluations take no filter, and there is no per-user extra exclusion list - the
filter is one item set for all users of a call."""
from __future__ import annotations

import sys
from typing import Optional

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

    def recommend(self, users, k: int, allow_items=None, deny_items=None, exclude_seen: bool = True, chunk: Optional[int] = 65536):
        """(items int64 [n, k], scores float32 [n, k]) for the listed users (any order, repeats allowed): the k best eligible items,
        -1 / -inf behind the last candidate. allow_items / deny_items: id lists or tensors - both given means allowed and not denied;
        exclude_seen: leave out the user's train row; chunk: users per call, which bounds the workspace (the lists do not depend on it;
        None = one call). k <= LLMREC_TOPK_WIDE_MAX (1024)."""
        dev = self.E_u.device
        q = _ids(users, "users", self.n_users, dev)
        filt = self.item_filter(allow_flags(self.n_items, allow_items, deny_items, dev))
        train = self.train if exclude_seen else None
        n = q.numel()
        step = n if not chunk or chunk >= n else int(chunk)
        parts = [ops.score_topk_filtered(self.E_u, self.E_i, q[a:a + step], train, int(k), filt) for a in range(0, n, max(step, 1))]
        if not parts:
            return torch.empty(0, k, dtype=torch.int64, device=dev), torch.empty(0, k, dtype=torch.float32, device=dev)
        idx, sc = (parts[0] if len(parts) == 1 else tuple(torch.cat(p) for p in zip(*parts)))
        return idx.to(torch.int64), sc
