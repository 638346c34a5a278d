"""Reference and table layouts for the evaluation kernels (llmrec_scores_f32, the llmrec_score_topk_* family, llmrec_score_auc_f32).
Nothing here imports llmrec_amd.

chain_scores   the scores' contract: the k-ordered fp32 fma chain of v_mfma_f32_16x16x4_f32 (oracle.scores_fma_chain), bit for bit.
rank           the lists' contract: (score desc, item id asc) over the items outside the train row, padded with -1 / -inf.
layouts        the same [n, d] values as views of differently strided / aligned allocations whose every other element is NaN: a kernel that
               reads one element outside the view - a tail element past d, a float4 across the row's end, the neighbouring column - turns a
               score into NaN, and a kernel that writes there is caught by Table.check()."""
import numpy as np
import torch

from oracle.oracle import scores_fma_chain

GUARD = 64            # NaN floats in front of and behind the rows (a multiple of 4: the guard does not move the base off 16 bytes)


def chain_scores(eu, ei):
    """float32 [n_users, n_items]: for c, for s in 0..3, for q in 0..3: k = 16 c + 4 q + s (k < d), acc = fmaf(eu[k], ei[k], acc)."""
    return scores_fma_chain(np.asarray(eu, dtype=np.float32), np.asarray(ei, dtype=np.float32), order="mfma16x16x4")


def rank(scores_row, train_items, K):
    """(ids int32 [K], scores float32 [K]) of one user: the K best items outside train_items by (score desc, item id asc); -1 / -inf where
    fewer than K candidates exist."""
    s = np.asarray(scores_row, dtype=np.float32)
    free = np.ones(s.shape[0], dtype=bool)
    t = np.asarray(train_items, dtype=np.int64)
    free[t[(t >= 0) & (t < s.shape[0])]] = False
    ids = np.flatnonzero(free)
    order = sorted(ids.tolist(), key=lambda i: (-float(s[i]), i))[:K]      # (a float32 negates and widens exactly)
    out_i = np.full(K, -1, dtype=np.int32)
    out_s = np.full(K, -np.inf, dtype=np.float32)
    out_i[:len(order)] = order
    out_s[:len(order)] = s[order]
    return out_i, out_s


def _ceil4(x):
    return (x + 3) // 4 * 4


class Table:
    """A float32 [n, d] view (`.t`) of a NaN-filled flat allocation (`.buf`): row r starts at element GUARD + col0 + r * ld."""

    def __init__(self, name, src, ld, col0, base_mod16, device):
        src = np.ascontiguousarray(src, dtype=np.float32)
        assert src.ndim == 2 and np.isfinite(src).all()
        n, d = src.shape
        assert ld >= d + col0
        self.name, self.src, self.ld, self.col0, self.base_mod16 = name, torch.from_numpy(src.copy()), ld, col0, base_mod16
        self.buf = torch.full((2 * GUARD + n * ld,), float("nan"), dtype=torch.float32, device=device)
        self.t = torch.as_strided(self.buf, (n, d), (ld, 1), GUARD + col0)
        self.t.copy_(self.src.to(device))
        idx = GUARD + col0 + torch.arange(n, device=device)[:, None] * ld + torch.arange(d, device=device)[None, :]
        self._outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=device)
        self._outside[idx.reshape(-1)] = False
        assert int(self._outside.sum()) == self.buf.numel() - n * d
        self.check()

    def check(self):
        """The promised stride and base; the view still holds the source and everything around it is still NaN (call it after the kernels too)."""
        t = self.t
        assert t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) == self.ld), (self.name, t.stride(), self.ld)
        if t.is_cuda:                                                       # (a host allocation promises no alignment)
            assert self.buf.data_ptr() % 16 == 0 and t.data_ptr() % 16 == self.base_mod16, (self.name, t.data_ptr() % 16)
        assert torch.equal(t.cpu(), self.src), "%s: the view no longer holds the source values" % self.name
        assert bool(torch.isnan(self.buf[self._outside]).all()), "%s: something wrote outside the view" % self.name


def layouts(d):
    """name -> builder(src [n, d] float32 numpy, device) -> Table. The vector path of the kernels (vec_ok) needs ld % 4 == 0 and 16-byte bases."""
    odd = d + 1 if (d + 1) % 4 else d + 2
    specs = {
        "contig": (d, 0, 0),                      # ld = d, base aligned
        "padded": (_ceil4(d) + 4, 0, 0),          # ld % 4 == 0, base aligned: the vector path on a non-contiguous table
        "odd_ld": (odd, 0, 0),                    # the smallest ld >= d + 1 with ld % 4 != 0: vec_ok off through the stride
        "shifted": (_ceil4(d + 1), 1, 4),         # ld % 4 == 0, the view starts one column into the allocation: vec_ok off through the base
    }

    def make(name):
        ld, col0, mod = specs[name]
        return lambda src, device="cuda": Table(name, src, ld, col0, mod, device)

    return {name: make(name) for name in specs}
