"""The yardstick of tests/test_gpu_step_rows.py for WHOLE training steps: the oracle step in a chosen precision, a comparator that works row
by row, the per-element AdamW check and the cases' inputs. Pure CPU (numpy, torch-CPU, scipy); tests/test_step_ref_cpu.py shows on
planted faults that it is neither blind nor too tight before any device is asked.

WHY ROWS. The gates that anchor the step (tests/test_gpu_step.py, bench.ParityGate, tests/test_gpu_trajectory.py) measure
max |a - b| / max |b| over a whole tensor. The user table's gradient has exactly the batch's rows non-zero, and 71 % of those - the samples
the prune loss drops, which carry the regulariser's gradient only - lie twelve orders of magnitude below the tensor's maximum: a step may
lose, double or leave stale any of them and that norm still reports 1e-7. Here every row is measured against ITS OWN maximum.

oracle_step(params, feats, R, batch, cfg, dtype)
  oracle.forward + oracle.step_loss + torch.autograd.grad in `dtype`. In both precisions the graph values are the ones the reference
  stores - normalized_graphs(R) in fp32 - widened, and the parameters and features are the given fp32 numbers widened: both sides read
  identical data, only the arithmetic differs. Returns float64 numpy arrays: fwd {name: [rows, d]} (the tensors of the 14-tuple,
  att_u/<key> and att_i/<key> included), bpr [8, 2] (mf, emb), loss, grad {name}, maxi [8][B] (the per-sample log-sigmoids the prune
  selection orders) and keep (the number of samples the prune keeps).
  THE OPT-IN MODES (tests/test_gpu_step_rows_modes.py). drop=Dropout(...): the projections times tests/_dropout_ref.keep_mask's masks and
  the fp32 quotient _dropout_ref.scale(p), in Models.forward's layout; P_usr is the dropped tensor. restore=Restoration(...): the
  attribute-restoration term of main.py:258-273 with autograd (the user stream detached, the decoder's weights constants), returned as
  re_vals - the 1 + len(keys) stream losses - and inside loss. Masking is NOT restated: the oracle is handed the device's own feature
  tensors as they stand after the step's masking round, bit copies - the principle of restarting from the device's own parameters; the
  round itself is checked on its own. Both default to None, which changes nothing.

row_check(got, want64, ref32, M)
  s_r = max_c |want64[r, c]|. A row with s_r == 0 must be exactly zero in got (-0.0 is zero). Else err_r(X) = max_c |X - want64| / s_r,
  the yardstick is y_r = max(err_r(ref32), q), q = the 95th percentile of err_r(ref32) over the tensor's non-zero rows (their maximum
  below 20 rows), and the row passes when err_r(got) <= M y_r. A 1-D tensor is one row. M = None measures only (zero rows still fail).

scalar_check: relative error against fp64, yardstick max(the fp32 oracle's relative error, 2^-23).

adamw_check: every element of p, m, v against tests/_rowops_ref.adamw - the value in fp64 from the device's OWN pre-step parameter, moments,
  step count and gradient, and that derivation's bound; no tolerance of this module's own. Parameters are never compared with
  oracle-gradients-then-oracle-AdamW: Adam's first steps turn a 1e-13 gradient error into a full lr step (bench.py, param_note).
  THE SCALED SOURCE. The folded step's user-table update reads inv * dE_u (inv = 1 / (layers + 1)) and stores that product as the table's
  .grad; dE_u's rows are cleared before the step ends, so the product's exact value is gone. The check feeds the STORED .grad, g_s =
  fl(inv dE_u), as adamw(g = 2 g_s, g_scale = 0.5): 2 g_s and 0.5 (2 g_s) are exact in binary floating point, so the value is computed
  from g_s itself, and because g_scale != 1 adamw() charges the one rounding it reports for g_out - eg = 2 u |gi| - and carries it
  through m (w1 eg), through p (em / denom) and, inside the constant 3 of ev, through v. That is exactly the widening by the rounding
  that separates the stored gradient from the exact product; nothing else is added.
"""
from __future__ import annotations

import os
from typing import Dict, NamedTuple, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import oracle as O
from tests import _rowops_ref as RR

PARAMS = ["image_trans.weight", "image_trans.bias", "text_trans.weight", "text_trans.bias", "user_trans.weight", "user_trans.bias",
          "item_trans.weight", "item_trans.bias", "user_id_embedding.weight", "item_id_embedding.weight"]
USER_TABLE, ITEM_TABLE = "user_id_embedding.weight", "item_id_embedding.weight"
TABLES = (USER_TABLE, ITEM_TABLE)
FWD = ("E_u", "E_i", "img_i", "txt_i", "img_u", "txt_u", "P_usr", "prof_u", "prof_i")
USER_ROWS = ("E_u", "img_u", "txt_u", "P_usr", "prof_u", "att_u", USER_TABLE)             # tensors whose rows are users (att_u/<key> too)
N_PROB = 8
SCALAR_FLOOR = 2.0 ** -23
M_MAX = 256
STEPS = 3
ADAM = dict(b1=0.9, b2=0.999, eps=1e-8, wd=0.01)          # ops.FusedAdamW's defaults = torch.optim.AdamW's


def family(name: str) -> str:
    """forward | table | linear: the family whose margin a tensor is held to"""
    if name in TABLES:
        return "table"
    return "linear" if name in PARAMS else "forward"


def side_of(name: str) -> Optional[str]:
    """'u' / 'i': whose rows a tensor's rows are; None for the Linear parameters"""
    if name in PARAMS and name not in TABLES:
        return None
    return "u" if name.split("/")[0] in USER_ROWS else "i"


# ------------------------------------------------------------------------------------------------------------------------------------
# the oracle step
# ------------------------------------------------------------------------------------------------------------------------------------
class Graphs:
    """normalized_graphs(R) in fp32, as the reference stores them, and their widened copies"""

    def __init__(self, R):
        import scipy.sparse as sp
        self.R = sp.csr_matrix(R)
        self._by = {torch.float32: O.normalized_graphs(self.R)}

    def get(self, dtype):
        if dtype not in self._by:
            self._by[dtype] = tuple(a.to(dtype) for a in self._by[torch.float32])
        return self._by[dtype]


def bpr_tables(fw, keys):
    """(user table, item table) of the eight BPR problems in the step's order (oracle.step_loss)"""
    return [(fw["E_u"], fw["E_i"]), (fw["img_u"], fw["img_i"]), (fw["txt_u"], fw["txt_i"])] + [(fw["prof_u"], fw["att_i"][k]) for k in keys]


class _MaskMul(torch.autograd.Function):
    """y = x * fwd, dx = dy * bwd: dropout whose backward factor can be stated apart from the forward's (they are the same tensor in a
    correct step; tests/test_step_ref_cpu.py plants the faults of a backward that reads another one)"""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.save_for_backward(bwd)
        return x * fwd

    @staticmethod
    def backward(ctx, dy):
        return dy * ctx.saved_tensors[0], None, None


class Dropout:
    """The fused step's dropout at device counter `step` for oracle_step(drop=): the keep masks are tests/_dropout_ref.keep_mask's, laid
    out as Models.forward lays the projections out - image = slice 0, text = slice 1, attribute k = slice 2 + k of the [n_items, S d]
    tensor under TAG_ITEM_STREAMS, the user profile [n_users, d] under TAG_USER_PROFILE - and the factor of a kept element is the fp32
    quotient _dropout_ref.scale(p), widened to the oracle's dtype."""

    def __init__(self, p, seed, step, n_users, n_items, d, keys):
        self.p, self.seed, self.step, self.U, self.I, self.d, self.keys = float(p), int(seed), int(step), n_users, n_items, d, tuple(keys)
        self._keep = {}

    def slice_of(self, name):
        return {"image": 0, "text": 1}.get(name, 2 + self.keys.index(name[5:]) if name.startswith("attr/") else None)

    def keep(self, step=None):
        """{feature name: bool [rows, d]} of the masks of counter value `step` (None: the step's own)"""
        from tests import _dropout_ref as DR
        step = self.step if step is None else step
        if step not in self._keep:
            S = 2 + len(self.keys)
            cat = DR.keep_mask(self.I, S * self.d, self.p, self.seed, step, DR.TAG_ITEM_STREAMS)
            out = {"user": DR.keep_mask(self.U, self.d, self.p, self.seed, step, DR.TAG_USER_PROFILE)}
            for name in ("image", "text") + tuple("attr/" + k for k in self.keys):
                s = self.slice_of(name)
                out[name] = cat[:, s * self.d:(s + 1) * self.d]
            self._keep[step] = out
        return self._keep[step]

    def factors(self, dtype, backward=False):
        """{feature name: [rows, d] tensor of `dtype`}: scale where kept, 0 where dropped"""
        from tests import _dropout_ref as DR
        scale = torch.tensor(float(DR.scale(self.p)), dtype=torch.float32).to(dtype)
        return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) * scale for k, v in self.keep().items()}

    def hooks(self, dtype):
        fwd, bwd = self.factors(dtype), self.factors(dtype, backward=True)
        return {k: (lambda x, k=k: _MaskMul.apply(x, fwd[k], bwd[k])) for k in fwd}


class Restoration:
    """The attribute-restoration term of main.py:258-273 for oracle_step(restore=), in the oracle's dtype with autograd:
    rate * (crit(u_net(prof_u[u_nodes].detach()), user_targets[u_nodes]) + sum_k crit(i_net(att_i[k][i_nodes]), item_targets[k][i_nodes])).
    crit(x, y, alpha): main.Trainer.sce_criterion / mse_criterion; decoder = {"u": (W, b), "i": (W, b), "slope": s} - the weights of
    Models.Decoder's two Linears as constants and the negative slope of its LeakyReLU as the drop-in constructs it; the targets are
    the UNMASKED embeddings, fp32 numbers widened like every other input."""

    def __init__(self, u_nodes, i_nodes, decoder, user_targets, item_targets, rate, crit, alpha):
        self.u_nodes, self.i_nodes = (torch.as_tensor(np.asarray(t), dtype=torch.long) for t in (u_nodes, i_nodes))
        f32 = lambda x: torch.as_tensor(np.asarray(x)).detach().float()
        self.net = {s: (f32(decoder[s][0]), f32(decoder[s][1])) for s in ("u", "i")}
        self.slope = float(decoder["slope"])
        self.user_targets, self.item_targets = f32(user_targets), {k: f32(v) for k, v in item_targets.items()}
        self.rate, self.crit, self.alpha = float(rate), crit, alpha

    def decode(self, side, x):
        W, b = (t.to(x.dtype) for t in self.net[side])
        return F.leaky_relu(F.linear(x, W, b), self.slope)

    def user_rows(self, prof_u):
        return prof_u[self.u_nodes].detach()                  # the reference wraps it in torch.tensor(...): no gradient

    def item_rows(self, att, key):
        return att[self.i_nodes]

    def streams(self, fw, keys):
        """the 1 + len(keys) stream losses (tensors): user, then the attributes in the keys' order"""
        dt = fw["prof_u"].dtype
        out = [self.crit(self.decode("u", self.user_rows(fw["prof_u"])), self.user_targets[self.u_nodes].to(dt), alpha=self.alpha)]
        for k in keys:
            out.append(self.crit(self.decode("i", self.item_rows(fw["att_i"][k], k)), self.item_targets[k][self.i_nodes].to(dt), alpha=self.alpha))
        return out

    def term(self, fw, keys):
        """(the term that joins the loss, the stream losses)"""
        vals = self.streams(fw, keys)
        total = vals[0]
        for v in vals[1:]:
            total = total + v
        return self.rate * total, vals


def oracle_step(params, feats, R, batch, cfg: O.Config, dtype, drop: Optional[Dropout] = None, restore: Optional[Restoration] = None):
    """drop / restore: the two opt-in modes (None: the default step, unchanged). With drop the forward's projections are dropped and
    fwd["P_usr"] is the dropped tensor; with restore the result gains "re_vals" (the 1 + len(keys) stream losses) and `loss` includes
    the term. Masking itself is not restated here: `feats` are the feature tensors as they stand after the step's masking round."""
    g = R if isinstance(R, Graphs) else Graphs(R)
    a_ui, a_iu = g.get(dtype)
    p = {k: torch.as_tensor(params[k]).detach().float().to(dtype).clone().requires_grad_(True) for k in PARAMS}
    f = {k: torch.as_tensor(v).float().to(dtype) for k, v in feats.items()}
    users, pos, neg = (torch.as_tensor(np.asarray(t), dtype=torch.long) for t in batch)
    if drop is None:
        fw = O.forward(p, f, a_ui, a_iu, cfg)
    else:
        fw = O.forward(p, f, a_ui, a_iu, cfg, drop=drop.hooks(dtype))
    loss, parts = O.step_loss(fw, users, pos, neg, g.R.shape[1], cfg)
    re_vals = None
    if restore is not None:
        term, re_vals = restore.term(fw, cfg.keys)
        loss = loss + term
    grads = torch.autograd.grad(loss, [p[k] for k in PARAMS])
    n64 = lambda t: t.detach().to(torch.float64).numpy()
    fwd = {k: n64(fw[k]) for k in FWD}
    for k in cfg.keys:
        fwd["att_u/" + k], fwd["att_i/" + k] = n64(fw["att_u"][k]), n64(fw["att_i"][k])
    maxi = []
    with torch.no_grad():
        for tu, ti in bpr_tables(fw, cfg.keys):
            maxi.append(n64(F.logsigmoid((tu[users] * ti[pos]).sum(1) - (tu[users] * ti[neg]).sum(1) + 1e-8)))
    out = {"fwd": fwd, "bpr": np.array([[float(a.detach()), float(b.detach())] for a, b in parts["bpr"]], dtype=np.float64), "loss": float(loss.detach()),
           "grad": {k: n64(t) for k, t in zip(PARAMS, grads)}, "maxi": maxi, "keep": int((1 - cfg.prune_loss_drop_rate) * len(users))}
    if re_vals is not None:
        out["re_vals"] = np.array([float(v.detach()) for v in re_vals], dtype=np.float64)
    return out


def kept_sets(maxi, keep):
    """per problem: the boolean [B] of the samples the prune keeps (stable ascending order, as oracle.prune_loss)"""
    out = []
    for m in maxi:
        k = np.zeros(len(m), dtype=bool)
        k[np.argsort(m, kind="stable")[:keep]] = True
        out.append(k)
    return out


def cut_gaps(r64, r32):
    """per problem (gap, err, gap / (64 err)): the distance of the fp64 maxi values on either side of the prune cut, the fp32 oracle's
    worst absolute error in that problem's maxi, and their ratio in units of the required 64 x: >= 1 is the condition, >= 2 what the
    seeds are chosen for. A cut that keeps every sample or none has no gap to violate: inf."""
    out = []
    for m64, m32 in zip(r64["maxi"], r32["maxi"]):
        keep, s = r64["keep"], np.sort(m64)
        gap = float(s[keep] - s[keep - 1]) if 0 < keep < len(s) else float("inf")
        err = float(np.abs(m32 - m64).max())
        out.append((gap, err, gap / (64.0 * err) if err > 0 else float("inf")))
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the comparator
# ------------------------------------------------------------------------------------------------------------------------------------
class RowResult(NamedTuple):
    name: str
    ok: bool
    ratio: float                     # the worst err_r(got) / y_r over the non-zero rows (inf: a violated zero row)
    row: int                         # its row (as stored; a transposed Linear gradient's column is reported as "T<col>" in `where`)
    where: str
    bad: tuple                       # every failing row, as (where-prefix, row)
    note: str                        # the provenance of the worst row


def _rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x.reshape(1, -1) if x.ndim <= 1 else x.reshape(x.shape[0], -1)


def _row_ratios(got, want, ref):
    """(ratio [rows] - inf on a violated zero row, 0 on a respected one -, err_got, y, s)"""
    s = np.abs(want).max(axis=1)
    live = s > 0
    ratio = np.zeros(len(s))
    err = np.zeros(len(s))
    y = np.zeros(len(s))
    dead_bad = ~live & ~(got == 0).all(axis=1)
    ratio[dead_bad] = np.inf
    if live.any():
        sl = s[live][:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            e_got = np.abs(got[live] - want[live]).max(axis=1) / sl[:, 0]
            e_got = np.where(np.isfinite(got[live]).all(axis=1), e_got, np.inf)
        e_ref = np.abs(ref[live] - want[live]).max(axis=1) / sl[:, 0]
        q = float(np.percentile(e_ref, 95)) if e_ref.size >= 20 else float(e_ref.max())
        yl = np.maximum(e_ref, q)
        with np.errstate(divide="ignore", invalid="ignore"):
            rl = np.where(e_got == 0, 0.0, np.where(yl > 0, e_got / yl, np.inf))
        ratio[live], err[live], y[live] = rl, e_got, yl
    return ratio, err, y, s


def row_check(got, want64, ref32, M, name="", prov=None) -> RowResult:
    """prov: {label: [rows] array} - what is printed about the worst row (in the batch? kept or dropped by the prune? its degree)"""
    got, want, ref = _rows(got), _rows(want64), _rows(ref32)
    assert got.shape == want.shape == ref.shape, (name, got.shape, want.shape, ref.shape)
    views = [("", got, want, ref)]
    if name in PARAMS and name not in TABLES and np.asarray(want64).ndim == 2:            # a Linear weight: as stored and transposed
        views.append(("T", got.T, want.T, ref.T))
    worst, bad = (-1.0, 0, "", 0.0, 0.0, 0.0), []
    for tag, g_, w_, r_ in views:
        ratio, err, y, s = _row_ratios(g_, w_, r_)
        limit = np.inf if M is None else float(M)
        fail = ~(ratio <= limit) if M is not None else np.isinf(ratio) & (s == 0)
        bad += [(tag, int(r)) for r in np.flatnonzero(fail)]
        r = int(np.argmax(ratio))
        if ratio[r] > worst[0]:
            worst = (float(ratio[r]), r, tag, float(err[r]), float(y[r]), float(s[r]))
    ratio, r, tag, err, y, s = worst
    note = "row %s%d: err %.3e, yardstick %.3e, row max %.3e, tensor max %.3e" % (tag, r, err, y, s, float(np.abs(want).max()))
    if prov and not tag:
        note += "; " + ", ".join("%s=%s" % (k, v[r]) for k, v in prov.items() if len(v) == got.shape[0])
    return RowResult(name, not bad, ratio, r, "%s%d" % (tag, r), tuple(bad), note)


def scalar_check(got, want64, ref32, M, name=""):
    """(ok, ratio): relative error against fp64 over the yardstick max(the fp32 oracle's relative error, 2^-23)"""
    got, want, ref = float(got), float(want64), float(ref32)
    assert want != 0.0, name
    y = max(abs(ref - want) / abs(want), SCALAR_FLOOR)
    ratio = abs(got - want) / abs(want) / y
    if not np.isfinite(got):
        ratio = float("inf")
    return (M is None or ratio <= M), ratio


class Provenance:
    """what row_check prints about a row: per side ('u' / 'i') whether the row is in the batch, how many of the eight problems' prunes keep
    one of its samples, and its degree"""

    def __init__(self, R, batch, kept):
        users, pos, neg = (np.asarray(t, dtype=np.int64) for t in batch)
        U, I = R.shape
        self.by = {}
        for side, n, ids in (("u", U, (users,)), ("i", I, (pos, neg))):
            in_batch = np.zeros(n, dtype=np.int64)
            kept_in = np.zeros(n, dtype=np.int64)
            for t in ids:
                np.add.at(in_batch, t, 1)
                for k in kept:
                    hit = np.zeros(n, dtype=bool)
                    hit[t[k]] = True
                    kept_in += hit
            self.by[side] = {"samples": in_batch, "kept_in_problems": kept_in, "degree": np.asarray(R.getnnz(1 if side == "u" else 0))}

    def of(self, name):
        return self.by.get(side_of(name))


def compare_step(got, r64, r32, M: Optional[Dict[str, float]], prov: Optional[Provenance] = None):
    """Every tensor and scalar of one step: got = {"fwd": {...}, "bpr": [8, 2], "loss": x, "grad": {...}} as oracle_step returns them.
    M: {"forward", "table", "linear", "scalar"} or None (measure). -> (failures [str], ratios {name: worst ratio})"""
    fails, ratios = [], {}
    m_of = (lambda fam: None) if M is None else (lambda fam: M[fam])
    assert sorted(got["fwd"]) == sorted(r64["fwd"]) and sorted(got["grad"]) == sorted(r64["grad"])
    for kind in ("fwd", "grad"):
        for name in r64[kind]:
            res = row_check(got[kind][name], r64[kind][name], r32[kind][name], m_of(family(name)), name, prov.of(name) if prov else None)
            ratios[kind + "/" + name] = res.ratio
            if not res.ok:
                fails.append("%s/%s: %d row(s) beyond the margin, first %s; worst ratio %.3g - %s" % (kind, name, len(res.bad), res.bad[:4], res.ratio, res.note))
    for p in range(N_PROB):
        for j, part in enumerate(("mf", "emb")):
            ok, ratio = scalar_check(got["bpr"][p][j], r64["bpr"][p][j], r32["bpr"][p][j], m_of("scalar"), "bpr%d/%s" % (p, part))
            ratios["bpr%d/%s" % (p, part)] = ratio
            if not ok:
                fails.append("bpr%d/%s: ratio %.3g (got %r, fp64 %r, fp32 %r)" % (p, part, ratio, float(got["bpr"][p][j]), r64["bpr"][p][j], r32["bpr"][p][j]))
    ok, ratio = scalar_check(got["loss"], r64["loss"], r32["loss"], m_of("scalar"), "loss")
    ratios["loss"] = ratio
    if not ok:
        fails.append("loss: ratio %.3g (got %r, fp64 %r, fp32 %r)" % (ratio, float(got["loss"]), r64["loss"], r32["loss"]))
    if "re_vals" in r64:                                                          # the restoration's stream losses: scalars like the others
        assert len(got["re_vals"]) == len(r64["re_vals"]) == len(r32["re_vals"])
        for j in range(len(r64["re_vals"])):
            ok, ratio = scalar_check(got["re_vals"][j], r64["re_vals"][j], r32["re_vals"][j], m_of("scalar"), "restore%d" % j)
            ratios["restore%d" % j] = ratio
            if not ok:
                fails.append("restore%d: ratio %.3g (got %r, fp64 %r, fp32 %r)" % (j, ratio, float(got["re_vals"][j]), r64["re_vals"][j], r32["re_vals"][j]))
    return fails, ratios


def family_of_key(key: str) -> str:
    """the margin family of one of compare_step's ratio keys"""
    if key == "loss" or key.startswith(("bpr", "restore")):
        return "scalar"
    return family(key.split("/", 1)[1])


# ------------------------------------------------------------------------------------------------------------------------------------
# AdamW, per element
# ------------------------------------------------------------------------------------------------------------------------------------
def adamw_check(name, pre, grad, post, t, lr, scaled_source=False):
    """pre / post = (p, m, v) float32 arrays before and after step number t (1-based) - m, v None before the first step: zeros -, grad =
    the gradient the device stored. -> [(what, flat index, |err|, bound)] of every element beyond tests/_rowops_ref.adamw's bound (the
    first 8 per tensor) and the worst |err| / bound per tensor. scaled_source: see the module docstring."""
    f32 = np.float32
    p, m, v = (None if x is None else np.asarray(x, dtype=f32).reshape(-1) for x in pre)
    m = np.zeros_like(p) if m is None else m
    v = np.zeros_like(p) if v is None else v
    g = np.asarray(grad, dtype=f32).reshape(-1)
    state = RR.adamw_state(t, lr, ADAM["b1"], ADAM["b2"])
    if scaled_source:
        assert np.isfinite(g * f32(2)).all()
        ref = RR.adamw(p, g * f32(2), m, v, state, lr=lr, g_scale=0.5, **ADAM)
    else:
        ref = RR.adamw(p, g, m, v, state, lr=lr, **ADAM)
    bad, worst = [], {}
    for what, x in zip(("p", "m", "v"), post):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        val, bound = ref[what]
        with np.errstate(invalid="ignore"):
            err = np.where(np.isinf(val), np.where(x == val, 0.0, np.inf), np.abs(x - val))
        err = np.where(np.isnan(err), np.inf, err)
        over = np.flatnonzero(~(err <= bound))
        bad += [("%s/%s" % (what, name), int(i), float(err[i]), float(bound[i])) for i in over[:8]]
        with np.errstate(divide="ignore", invalid="ignore"):
            worst[what] = float(np.where(err == 0, 0.0, err / bound).max())
    return bad, worst


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases' inputs (shared by the GPU test and the CPU test of the yardstick)
# ------------------------------------------------------------------------------------------------------------------------------------
# feat_scale: the generator's image / text features are unit gaussians, and a user's image row aggregates its own items': at that scale
#   more than 71 % of the image and text problems' samples saturate (maxi ~ -1e-46), the prune cut falls among values fp32 cannot tell
#   apart and no seed can give the cut a gap. Scaled by 1/8 (exact) the scores are of order one.
# A's --seed (initialisation AND the device sampler's stream): the cut-gap condition - eight problems, three steps, 64 fp32 errors,
#   twice that here - holds for about one seed in three thousand with sampled batches of 281 (the neighbours at a cut are ~1 / 281 of
#   the range apart, 64 fp32 errors are a fifth of that). 6375 came out of a search over several thousand seeds; 2022, the seed of
#   tests/test_gpu_step_host_wgrad.py, does not have it. B and C choose their triples instead (island_batches).
CASE_A = dict(dataset="netflix_valid_item", n_users=9000, n_items=1000, n_edges=40000, data_seed=11, dims=(128, 256, 128), max_deg=300,
              feat_scale=0.125, argv=["--batch_size", "256", "--seed", "6375", "--debug", "--lr", "0.001", "--layers", "2", "--embed_size", "64", "--epoch", "1"])
CASE_B = dict(dataset="preprocessed_raw_MovieLens", n_users=3000, n_items=800, n_edges=12000, data_seed=5, dims=(48, 200, 72), max_deg=300,
              n_communities=4, feat_scale=0.125,
              argv=["--batch_size", "512", "--seed", "2022", "--debug", "--lr", "0.001", "--weight_size", "[64, 64, 64]",
                    "--embed_size", "64", "--epoch", "1"], batch_seed=3, n_distinct=400, n_repeat=8, pool_chunks=16)
CASE_C = dict(CASE_B, argv=["--batch_size", "4608"] + CASE_B["argv"][2:], batch_seed=1, n_triples=4608, copies=8, pool_chunks=10)
# The opt-in modes (tests/test_gpu_step_rows_modes.py), all on B's dataset, schedule and batch structure. The forward differs per step
# here - a new dropout mask, or feature rows masked since the last step - so island_batches chooses every step's triples from the fp64
# forward under THAT step's masks or features (mode_forwards).
#   D  --drop_rate 0.3: the fp32 quotient 1 / (1 - p) is inexact (at the parity test's 0.5 it is 2).
#   K  --mask True --mask_rate 0.25 --att_re_rate 0.5: 750 user and 200 item nodes per round, about three quarters of them in blocks the
#      batch never reaches; K_MSE: the same under --feat_loss_type mse. eval_before: one evaluation - one masking round - precedes that
#      step, so the round counter leaves the step index (rounds 0, 1, 3).
#   U  --mask_rate 0.25 alone (user features only; the step keeps the schedule it has without the flag). ON B'S SHAPE, not A's hosted
#      one: A's batches are the device sampler's, and its cut-gap condition holds for about one --seed in three thousand (above). With
#      masking the seed also fixes the lists, so 6375 does not carry over, and a new search means several thousand seeds times three
#      fp64 and three fp32 oracle steps at 9000 x 1000 each - hours on the CPU, where B's chosen triples meet the condition by construction.
CASE_D = dict(CASE_B, argv=CASE_B["argv"] + ["--drop_rate", "0.3"], mode="drop")
CASE_K = dict(CASE_B, argv=CASE_B["argv"] + ["--mask", "True", "--mask_rate", "0.25", "--att_re_rate", "0.5"], mode="mask", eval_before=2,
              pool_chunks=64)          # (masked users and items score alike in the profile problems: fewer candidates clear the band)
CASE_K_MSE = dict(CASE_K, argv=CASE_K["argv"] + ["--feat_loss_type", "mse"])
CASE_U = dict(CASE_B, argv=CASE_B["argv"] + ["--mask_rate", "0.25"], mode="mask", eval_before=2, pool_chunks=64)


def mask_rounds(case):
    """The masking round of each of the STEPS steps: the step index, plus one from the step an evaluation precedes"""
    e = case.get("eval_before")
    return [s + (1 if e is not None and s >= e else 0) for s in range(STEPS)]


def masked_features(feats, keys, seed, m_users, m_items, n_rounds):
    """The feature tensors after each of the rounds 0 .. n_rounds - 1 (tests/_mask_ref.mask_round from from-scratch column sums; rounds
    are cumulative and a function of (seed, round) alone, so they are known before any step runs) -> per round (feats, u_nodes, i_nodes).
    m_items = 0: user features only."""
    from tests import _mask_ref as MR
    cur = {k: np.asarray(v, dtype=np.float32).copy() for k, v in feats.items()}
    masked = ["user"] + (["attr/" + k for k in keys] if m_items else [])
    sums = {k: MR.col_sums(cur[k]) for k in masked}
    out = []
    for rnd in range(n_rounds):
        u_nodes = MR.nodes(cur["user"].shape[0], m_users, seed, rnd, MR.SIDE_USERS)
        i_nodes = MR.nodes(cur["image"].shape[0], m_items, seed, rnd, MR.SIDE_ITEMS) if m_items else np.zeros(0, dtype=np.int64)
        for k in masked:
            cur[k], sums[k], _ = MR.mask_round(cur[k], sums[k], u_nodes if k == "user" else i_nodes)
        out.append(({k: torch.from_numpy(v.copy()) for k, v in cur.items()}, u_nodes, i_nodes))
    return out


def mode_forwards(case, data, cfg, args):
    """island_batches' per_step of a mode case: step -> (the feature tensors, the Dropout) the step's forward runs under"""
    n_u, n_i = data.n_users, data.n_items
    if case["mode"] == "drop":
        return lambda s: (data.feats, Dropout(args.drop_rate, args.seed, s, n_u, n_i, cfg.embed_size, cfg.keys))
    rounds = mask_rounds(case)
    after = masked_features(data.feats, cfg.keys, args.seed, int(args.mask_rate * n_u), int(args.mask_rate * n_i) if args.mask else 0, rounds[-1] + 1)
    return lambda s: (after[rounds[s]][0], None)


def write_case(case, root):
    """The case's dataset under root/<dataset> (llmrec_amd.synth.write_dataset). With n_communities the generator moves every draw into
    the user's own block (p_in = 1), but its de-duplication redraws a repeated pair uniformly among ALL items, which bridges the blocks;
    those bridges are removed here (an item belongs to the block most of its users are in), so that the graph falls into disjoint
    islands - asserted - and a batch drawn from one island leaves the other islands' rows of every gradient exactly zero."""
    import json
    import pickle
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    from llmrec_amd import synth
    ds = os.path.join(root, case["dataset"])
    C = case.get("n_communities", 0)
    synth.write_dataset(ds, case["n_users"], case["n_items"], case["n_edges"], seed=case["data_seed"], image_dim=case["dims"][0],
                        text_dim=case["dims"][1], llm_dim=case["dims"][2], keys=synth.DATASET_KEYS[case["dataset"]], max_deg=case["max_deg"],
                        n_communities=C, **({"p_in": 1.0} if C else {}))
    for name in ("image_feat.npy", "text_feat.npy"):                                # (a power of two: the scaled features are exact)
        path = os.path.join(ds, name)
        np.save(path, (np.load(path) * np.float32(case["feat_scale"])).astype(np.float32))
    if C:
        R = pickle.load(open(os.path.join(ds, "train_mat"), "rb")).tocoo()
        votes = np.zeros((case["n_items"], C), dtype=np.int64)
        np.add.at(votes, (R.col, R.row % C), 1)
        keep = votes.argmax(axis=1)[R.col] == R.row % C
        R2 = sp.csr_matrix((R.data[keep], (R.row[keep], R.col[keep])), shape=R.shape)
        _, lab = connected_components(sp.bmat([[None, R2], [R2.T, None]]).tocsr(), directed=False)
        for c in np.unique(lab):                                                    # no island holds users of two blocks
            assert np.unique(np.flatnonzero(lab[:R.shape[0]] == c) % C).size <= 1
        with open(os.path.join(ds, "train_mat"), "wb") as f:
            pickle.dump(R2, f)
        train = {}
        for u, i in zip(R2.tocoo().row.tolist(), R2.tocoo().col.tolist()):
            train.setdefault(str(u), []).append(i)
        with open(os.path.join(ds, "train.json"), "w") as f:
            json.dump(train, f)
    return ds


def case_argv(case, root):
    return ["--dataset", case["dataset"], "--data_path", root + "/"] + list(case["argv"])


def oracle_inputs(case, root, args):
    """(OracleData, Config, Graphs) of a case whose dataset write_case() put under root; args = the drop-in's parsed flags"""
    from llmrec_amd import synth
    keys = synth.DATASET_KEYS[case["dataset"]]
    data = O.load_dataset(os.path.join(root, case["dataset"]), keys)
    return data, O.Config.from_args(vars(args), keys), Graphs(data.train_mat)


def sampled_batch(data, exist_users, seed, batch_size, aug_rate, step):
    """The batch the device sampler draws at step counter `step` (tests/_sampler_ref.py, held to the kernels bit for bit by
    tests/test_gpu_sampler.py), with the augmented triples, as main.Trainer._device_batcher sets it up: the valid triples only."""
    import scipy.sparse as sp
    from tests import _sampler_ref as SR
    R = sp.csr_matrix(data.train_mat)
    R.sort_indices()
    big = np.iinfo(np.int64).max
    ap, an = np.full(data.n_users, big, dtype=np.int64), np.full(data.n_users, big, dtype=np.int64)
    for u_, pair in data.aug_dict.items():
        if 0 <= int(u_) < data.n_users:
            ap[int(u_)], an[int(u_)] = int(pair[0]), int(pair[1])
    u, p, n, nv, _ = SR.sample_batch(seed, step, exist_users, data.n_items, R.indptr, R.indices, batch_size, 0, batch_size,
                                     int(batch_size * aug_rate), ap, an)
    return u[:nv], p[:nv], n[:nv]


BAND = 0.1                       # a triple qualifies when |x_p| > BAND std(x_p) in every problem p


def island_batches(case, data, graphs, cfg, params0, per_step=None, only=None):
    """per_step (the mode cases: mode_forwards): step -> (feats, Dropout or None); a step's candidates are then judged in the fp64
    forward under THAT step's features and masks, with a candidate pool of its own. only = s: the batch of step s alone, as a list of
    one, from the parameters given - the step's own pre-step parameters (the generator is then seeded with (batch_seed, s)). The mode
    cases need that: in case K triples chosen from the initial parameters had lost the empty stretch at the cut by the third step
    (an exact tie across one problem's cut, gap 0, where B keeps 6 x the requirement; supposed cause: the restoration term pulls
    every entry of item_trans the same way step after step). The masks and lists are functions of
    (seed, round) alone, so the forward a step will run is known before it runs. per_step = None: one forward and one pool for all
    steps, as cases B and C have always drawn them (the generator's draws are in the same order).
    The injected batches of the STEPS steps of cases B and C: every user from block 0 (u % C == 0), every item from that block's
    island. B: n_distinct users once each and user[0] n_repeat + 1 >= 8 times; an item that is the positive of one triple and the
    negative of another (asserted); no two triples identical; fewer triples than the step's capacity. C: n_triples / copies distinct
    triples, each `copies` times, shuffled - copies divides both n_triples and the number of samples the prune keeps, so the ties
    never straddle the cut.
    THE GAP AT THE CUT IS BUILT IN. Sampled triples cannot give it: the fp32 oracle's error in maxi is ~3e-6 of the values' range and
    64 of those are a fifth of the mean distance of neighbours among 400 samples, so some of the eight problems' cuts would fall in a
    narrower gap at nearly every seed (the profile problems score user profiles against item attributes, which no interaction
    correlates). The triples are therefore CHOSEN: from the fp64 forward of the INITIAL parameters, x_p = <u, pos - neg> of every
    candidate in each of the eight problems; a triple is hard when x_p < -BAND std(x_p) in all eight, easy when x_p > +BAND std(x_p)
    in all eight, and is not used otherwise. A batch holds exactly as many hard triples as the prune keeps, int((1 - drop) n): the
    sorted maxi values of every problem fall into two groups and the cut lies in the empty stretch between them
    (tests/test_step_ref_cpu.py measures it over the oracle's three steps; the GPU test asserts it at every step)."""
    import scipy.sparse as sp
    R = sp.csr_matrix(data.train_mat)
    C = case["n_communities"]
    assert only is None or per_step is not None
    rng = np.random.default_rng(case["batch_seed"] if only is None else [case["batch_seed"], only])
    block_users = np.flatnonzero((np.arange(R.shape[0]) % C == 0) & (R.getnnz(1) > 0))
    block_items = np.unique(R[block_users].indices)
    a_ui, a_iu = graphs.get(torch.float64)
    tabs = []

    def forward_tables(feats, drop):
        with torch.no_grad():
            fw = O.forward({k: torch.as_tensor(params0[k]).detach().double() for k in PARAMS}, {k: v.double() for k, v in feats.items()},
                           a_ui, a_iu, cfg, **({} if drop is None else {"drop": drop.hooks(torch.float64)}))
            tabs[:] = [(tu.numpy(), ti.numpy()) for tu, ti in bpr_tables(fw, cfg.keys)]
        if per_step is not None:                                                  # the block's score matrices: a candidate costs two look-ups
            tabs[:] = [tu[block_users] @ ti[block_items].T for tu, ti in tabs]

    u_at, i_at = np.zeros(R.shape[0], dtype=np.int64), np.zeros(R.shape[1], dtype=np.int64)
    u_at[block_users], i_at[block_items] = np.arange(len(block_users)), np.arange(len(block_items))

    def signs(u, a, b):
        """+1 / -1 / 0 per candidate: easy / hard / unused"""
        lo = np.ones(len(u), dtype=bool)
        hi = np.ones(len(u), dtype=bool)
        for tab in tabs:
            if per_step is not None:
                x = tab[u_at[u], i_at[a]] - tab[u_at[u], i_at[b]]
            else:
                x = np.einsum("nd,nd->n", tab[0][u], tab[1][a] - tab[1][b])
            band = BAND * x.std()
            lo &= x < -band
            hi &= x > band
        return hi.astype(np.int64) - lo.astype(np.int64)

    star = int(block_users[0])                                                    # the user that appears n_repeat + 1 times: every pair
    ga, gb = np.meshgrid(block_items, block_items, indexing="ij")
    sa, sb = ga.reshape(-1), gb.reshape(-1)
    sa, sb = sa[sa != sb], sb[sa != sb]
    others = block_users[1:]

    def pools():
        """(pool, star_pool): {+1 / -1: [n, 3] triples} of the other users' random candidates and of every pair of the repeated user"""
        s_star = signs(np.full(len(sa), star), sa, sb)
        pool = {1: [], -1: []}
        for _ in range(case.get("pool_chunks", 6)):                               # random candidates of the other users, in chunks
            u = rng.choice(others, size=40000)
            a, b = rng.choice(block_items, size=u.size), rng.choice(block_items, size=u.size)
            sg = signs(u, a, b) * (a != b)
            for sign in (1, -1):
                pool[sign].append(np.stack([u, a, b], axis=1)[sg == sign])
        pool = {k: np.unique(np.concatenate(v), axis=0) for k, v in pool.items()}
        return pool, {k: np.stack([np.full(int((s_star == k).sum()), star), sa[s_star == k], sb[s_star == k]], axis=1) for k in (1, -1)}

    if per_step is None:
        forward_tables(data.feats, None)
        pool, star_pool = pools()
    n = case.get("n_triples")
    out = []
    for step in (range(STEPS) if only is None else [only]):
        if per_step is not None:
            forward_tables(*per_step(step))
            pool, star_pool = pools()
        if n is None:                                                             # B
            total = case["n_distinct"] + case["n_repeat"]
            keep = int((1 - cfg.prune_loss_drop_rate) * total)
            n_star = {-1: 3, 1: case["n_repeat"] + 1 - 3}
            parts = []
            for sign, count in ((-1, keep), (1, total - keep)):
                sp_ = star_pool[sign][rng.permutation(len(star_pool[sign]))[:n_star[sign]]]
                assert len(sp_) == n_star[sign], "island_batches: the repeated user has too few %s triples" % ("easy" if sign > 0 else "hard")
                cand = pool[sign][rng.permutation(len(pool[sign]))]
                _, first = np.unique(cand[:, 0], return_index=True)                # one triple per user: every other user appears once
                parts += [sp_, cand[np.sort(first)]]
            hard_o = parts[1][:keep - 3]
            fresh = ~np.isin(parts[3][:, 0], hard_o[:, 0])                         # easy triples of users not used yet first, then of the others
            easy_o = np.concatenate([parts[3][fresh], parts[3][~fresh]])[:total - keep - n_star[1]]
            assert len(hard_o) == keep - 3 and len(easy_o) == total - keep - n_star[1], ("island_batches: pool too small", len(hard_o), len(easy_o))
            t = np.concatenate([parts[0], hard_o, parts[2], easy_o])
            t = t[rng.permutation(len(t))]
        else:                                                                     # C
            copies = case["copies"]
            keep = int((1 - cfg.prune_loss_drop_rate) * n)
            assert n % copies == 0 and keep % copies == 0
            hard = pool[-1][rng.permutation(len(pool[-1]))[:keep // copies]]
            easy = pool[1][rng.permutation(len(pool[1]))[:(n - keep) // copies]]
            assert len(hard) == keep // copies and len(easy) == (n - keep) // copies, "island_batches: pool too small"
            t = np.repeat(np.concatenate([hard, easy]), copies, axis=0)
            t = t[rng.permutation(len(t))]
        out.append((t[:, 0].astype(np.int64), t[:, 1].astype(np.int64), t[:, 2].astype(np.int64)))
    return out


def relabel(params, feats, R, batch, seed):
    """The same step with users and items renamed by random permutations: (params, feats, R, batch) of the renamed problem and
    back(result) which renames an oracle_step result back. The sums of every SpMM row and weight gradient then run in another order."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    R = sp.csr_matrix(R)
    U, I = R.shape
    ou, oi = rng.permutation(U), rng.permutation(I)                  # new -> old
    nu, ni = np.argsort(ou), np.argsort(oi)                          # old -> new
    p2 = {k: torch.as_tensor(v).detach().clone() for k, v in params.items()}
    p2[USER_TABLE], p2[ITEM_TABLE] = p2[USER_TABLE][ou], p2[ITEM_TABLE][oi]
    f2 = {k: (torch.as_tensor(v)[ou] if k == "user" else torch.as_tensor(v)[oi]) for k, v in feats.items()}
    users, pos, neg = batch
    b2 = (nu[np.asarray(users)], ni[np.asarray(pos)], ni[np.asarray(neg)])

    def back(res):
        out = dict(res)
        out["fwd"] = {k: v[nu if side_of(k) == "u" else ni] for k, v in res["fwd"].items()}
        out["grad"] = {k: (v if side_of(k) is None else v[nu if side_of(k) == "u" else ni]) for k, v in res["grad"].items()}
        return out
    back.ou, back.oi, back.nu, back.ni = ou, oi, nu, ni              # for what else names rows: relabel_modes
    return p2, f2, R[ou][:, oi].tocsr(), b2, back


def relabel_modes(back, drop=None, restore=None):
    """(drop, restore) of the problem relabel() renamed: the same masks on the renamed rows, the same nodes under their new names"""
    d2 = r2 = None
    if drop is not None:
        d2 = Dropout(drop.p, drop.seed, drop.step, drop.U, drop.I, drop.d, drop.keys)
        d2.keep = lambda step=None: {k: v[back.ou if k == "user" else back.oi] for k, v in drop.keep(step).items()}
    if restore is not None:
        r2 = Restoration(back.nu[restore.u_nodes.numpy()], back.ni[restore.i_nodes.numpy()], dict(restore.net, slope=restore.slope),
                         restore.user_targets[back.ou], {k: v[back.oi] for k, v in restore.item_targets.items()}, restore.rate, restore.crit,
                         restore.alpha)
    return d2, r2


def restoration_of(m, tr, keys, u_nodes, i_nodes):
    """The Restoration of the drop-in module m's Trainer tr at its flags, for the round's node lists"""
    a = m.args
    crit = m.Trainer.mse_criterion if a.feat_loss_type == "mse" else m.Trainer.sce_criterion      # (neither reads self)
    u_net, i_net = tr.decoder.u_net, tr.decoder.i_net
    assert float(u_net[1].negative_slope) == float(i_net[1].negative_slope)
    w = lambda lin: (lin.weight.detach().cpu(), lin.bias.detach().cpu())
    return Restoration(u_nodes, i_nodes, {"u": w(u_net[0]), "i": w(i_net[0]), "slope": float(u_net[1].negative_slope)}, tr.user_init_embedding,
                       {k: tr.item_attribute_embedding[k] for k in keys}, a.att_re_rate, lambda x, y, alpha: crit(None, x, y, alpha=alpha), a.alpha_l)
