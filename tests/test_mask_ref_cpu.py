"""No GPU: the yardstick of tests/test_gpu_mask.py (tests/_mask_ref.py) and everything of the fused step's feature masking that is decided
on the host - the node lists' contract, the fp64 restatement of the restoration term against torch autograd, bounds that are neither
exceeded by a legitimate fp32 evaluation nor met by a planted defect, step_options.route / resolve under LLMREC_FUSED=mask, and the ABI with
every refusal the header states (status code before any HIP call)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from llmrec_amd import _lib, ops
from llmrec_amd import step_options as SO
from tests import _mask_ref as R
from tests import _sampler_ref as S

FAKE = 0x7f0000000000
EINVAL, EUNSUPPORTED = -1, _lib.EUNSUPPORTED
CAP, WIDE = 4096, 65536


# ------------------------------------------------------------------------------------------------------------------------------------
# node lists
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m", [(1, 1), (96, 24), (80, 20), (5000, 1), (5000, 4999), (17, 17)])
def test_a_node_list_is_m_distinct_ids_below_n(N, m):
    for rnd in (0, 3, 2 ** 32 + 3):
        for side in (R.SIDE_USERS, R.SIDE_ITEMS):
            got = R.nodes(N, m, 2022, rnd, side)
            assert got.dtype == np.int64 and got.shape == (m,) and got.min() >= 0 and got.max() < N and np.unique(got).size == m


def test_lists_differ_between_rounds_sides_and_seeds_and_use_their_own_key():
    base = R.nodes(5000, 1250, 2022, 3, R.SIDE_USERS)
    assert np.array_equal(base, R.nodes(5000, 1250, 2022, 3, R.SIDE_USERS))
    for other in (R.nodes(5000, 1250, 2022, 4, R.SIDE_USERS), R.nodes(5000, 1250, 2022, 3, R.SIDE_ITEMS), R.nodes(5000, 1250, 2023, 3, R.SIDE_USERS),
                  R.nodes(5000, 1250, 2022, 2 ** 32 + 3, R.SIDE_USERS)):
        assert not np.array_equal(base, other)
    # the step word is 2 round + side: (round 3, items) and (round 3, users) are the words 7 and 6, no two (round, side) pairs share one
    assert np.array_equal(R.nodes(96, 24, 5, 3, 1), S.keyed_perm(np.arange(24, dtype=np.uint64), 96, 5 ^ R.K_MASK, 7).astype(np.int64))
    # a stream of its own: not the sampler's two keys, not the dropout's
    assert R.K_MASK == ops.K_MASK and R.K_MASK not in (0, S.AUG_KEY_XOR, 0xD1B54A32D192ED03)
    assert (R.SIDE_USERS, R.SIDE_ITEMS, R.ROW_LANES) == (ops.MASK_SIDE_USERS, ops.MASK_SIDE_ITEMS, ops.MASK_ROW_LANES)


# ------------------------------------------------------------------------------------------------------------------------------------
# the restatement against autograd (float64, as Trainer._mask_loss writes the term)
# ------------------------------------------------------------------------------------------------------------------------------------
def _case(rows, Fdim, seed, d=64, n=None, special=True):
    """X [n, d], T [n, F], a duplicate-free list with gaps, W [F, d], b [F] (fp32 values). special: row 0 of the list has y = t up to
    rounding (cos = 1), row 1 - where there is one - is x = 0 (with b = 0 the eps branch)."""
    rng = np.random.default_rng(seed)
    n = 3 * rows + 5 if n is None else n
    X = rng.standard_normal((n, d)).astype(np.float32)
    T = rng.standard_normal((n, Fdim)).astype(np.float32)
    W = (rng.standard_normal((Fdim, d)) / 8).astype(np.float32)
    b = (rng.standard_normal(Fdim) / 4).astype(np.float32)
    nodes = rng.permutation(n)[:rows].astype(np.int64)
    if special:
        T[nodes[0]] = (X[nodes[0]].astype(np.float64) @ W.T.astype(np.float64) + b).astype(np.float32)
        if rows > 1:
            X[nodes[1]] = 0.0
    return X, T, nodes, W, b


def _torch_term(X, T, nodes, W, b, loss_type, alpha, rate):
    """rate x crit(decoder(x[nodes]), target[nodes]) and its gradient with respect to the WHOLE x (zero rows outside the list)."""
    x = torch.tensor(X, dtype=torch.float64, requires_grad=True)
    idx = torch.tensor(nodes)
    y = F.leaky_relu(F.linear(x[idx], torch.tensor(W, dtype=torch.float64), torch.tensor(b, dtype=torch.float64)), 1.0)   # LeakyReLU(True): slope 1
    t = torch.tensor(T, dtype=torch.float64)[idx]
    if loss_type == "mse":
        loss = F.mse_loss(F.normalize(y, p=2, dim=-1), F.normalize(t, p=2, dim=-1))
    else:
        loss = (1 - (F.normalize(y, p=2, dim=-1) * F.normalize(t, p=2, dim=-1)).sum(dim=-1)).pow_(alpha).mean()
    (rate * loss).backward()
    return float(loss.detach()), x.grad.numpy()


@pytest.mark.parametrize("zero_bias", [False, True])
@pytest.mark.parametrize("loss_type,alpha", [("sce", 1), ("sce", 2), ("sce", 3), ("mse", 1), ("mse", 2), ("mse", 3)])
def test_the_restatement_agrees_with_autograd_in_float64(loss_type, alpha, zero_bias):
    X, T, nodes, W, b = _case(17, 56, 11 + alpha)
    if zero_bias:
        b = np.zeros_like(b)                                              # the list's second row is then y = 0: F.normalize's eps branch
    want_loss, want_grad = _torch_term(X, T, nodes, W, b, loss_type, alpha, 0.5)
    got = R.restore(X, T, nodes, W, b, loss_type, alpha, scale=0.5, eps=1e-12)
    assert abs(got["loss"] - want_loss) <= 1e-13 * max(1.0, abs(want_loss))
    scale = np.abs(want_grad[nodes]).max()
    assert scale > 0 and np.abs(got["grad"] - want_grad[nodes]).max() <= 1e-12 * scale
    assert not want_grad[np.setdiff1d(np.arange(X.shape[0]), nodes)].any()
    if zero_bias:
        assert np.abs(got["grad"][1]).max() > 1e6 * np.abs(got["grad"][2:]).max()     # 1 / eps: the clamped norm does not move with y


# ------------------------------------------------------------------------------------------------------------------------------------
# the bounds are neither vacuous nor tight to one order of operations
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,Fdim", [(1, 56), (17, 64), (130, 200)])
@pytest.mark.parametrize("loss_type,alpha", [("sce", 1), ("sce", 2), ("sce", 3), ("mse", 2)])
def test_an_fp32_evaluation_keeps_half_of_every_restoration_bound_and_a_dropped_cosine_does_not(rows, Fdim, loss_type, alpha):
    X, T, nodes, W, b = _case(rows, Fdim, 100 * rows + Fdim)
    dst0 = np.random.default_rng(3).standard_normal((rows, 64)).astype(np.float32)
    exact = R.restore(X, T, nodes, W, b, loss_type, alpha, scale=0.5)
    bound = R.restore_bound(X, T, nodes, W, b, loss_type, alpha, scale=0.5, dst0=dst0)
    emu = R.restore_fp32(X, T, nodes, W, b, loss_type, alpha, scale=0.5, dst0=dst0)
    assert np.isfinite(bound["grad"]).all() and np.isfinite(bound["row_loss"]).all() and np.isfinite(bound["loss"])
    assert (np.abs(emu["row_loss"] - exact["row_loss"]) <= bound["row_loss"] / 2).all()
    assert abs(float(emu["loss"]) - exact["loss"]) <= bound["loss"] / 2
    # the update of a non-zero destination row ends in ONE rounding of size u |result|, a bound that is tight by nature: the whole bound
    # there, half of it on zero rows (what the step's scatter source holds outside the batch's items)
    assert (np.abs(emu["grad"].astype(np.float64) - (dst0 + exact["grad"])) <= bound["grad"]).all()
    bound0, emu0 = R.restore_bound(X, T, nodes, W, b, loss_type, alpha, scale=0.5), R.restore_fp32(X, T, nodes, W, b, loss_type, alpha, scale=0.5)
    assert (np.abs(emu0["grad"].astype(np.float64) - exact["grad"]) <= bound0["grad"] / 2).all()
    # the bound is fp32-sized: relative to the largest gradient entry of a row it is far below the project's 1e-4
    live = np.arange(rows) != 1                                           # (the x = 0 row's gradient is 1 / eps-sized only without a bias)
    assert (bound["grad"][live].max(1) <= 2e-5 * np.maximum(np.abs(dst0 + exact["grad"])[live].max(1), 1e-3)).all()
    planted = R.restore(X, T, nodes, W, b, loss_type, alpha, scale=0.5, planted="no_c")
    rows_hit = np.abs(planted["grad"] - exact["grad"]).max(1) > bound["grad"].max(1)
    assert rows_hit[2:].all() if rows > 2 else rows_hit.any() or rows == 1    # (row 0 has cos = 1: dropping c changes nothing there)


def test_the_running_sums_keep_their_bound_and_a_sum_updated_too_early_does_not():
    rng = np.random.default_rng(5)
    N, cols, m = 300, 200, 75
    X0 = (rng.standard_normal((N, cols)) + 0.5).astype(np.float32)
    for planted in (None, "sum_first"):
        X, sums, rb = X0.copy(), R.col_sums(X0), R.RunningBound(X0)
        assert (np.abs(sums - np.sum(X0.astype(np.float64), axis=0)) <= rb.bound() / 2).all()      # numpy's pairwise order: half the bound
        worst = 0.0
        for rnd in range(5):
            nodes = R.nodes(N, m, 9, rnd, R.SIDE_ITEMS)
            before, old = sums, X[nodes].copy()
            X, sums, mean = R.mask_round(X, sums, nodes, planted=planted)
            rb.round(old, mean, before)
            assert np.array_equal(X[nodes], np.broadcast_to(mean, (m, cols)))
            exact = np.sum(X.astype(np.float64), axis=0)
            worst = max(worst, float((np.abs(sums - exact) / rb.bound()).max()))
            if planted is None:
                assert np.array_equal(mean, (before / N).astype(np.float32))
        assert (worst <= 0.5) if planted is None else (worst > 1e3), (planted, worst)


# ------------------------------------------------------------------------------------------------------------------------------------
# route / resolve
# ------------------------------------------------------------------------------------------------------------------------------------
def _route(fused, fd=None, mask=False, mask_rate=0.0, drop_rate=0.0, b_max=1024, **kw):
    return SO.route(fused, fd, mask=mask, mask_rate=mask_rate, drop_rate=drop_rate, b_max=b_max, cap=CAP, wide_cap=WIDE, **kw)


def test_route_under_llmrec_fused_mask():
    nf = dict(n_users=13187, n_items=17366)
    # as "1" where nothing is masked
    assert _route("mask") == "fused" and _route("mask", b_max=CAP) == "fused" and _route("mask", b_max=CAP + 1) == "modular"
    assert _route("mask", drop_rate=0.5) == "modular" and _route("mask", "1", drop_rate=0.5) == "fused"
    # masking stays fused
    assert _route("mask", mask_rate=0.1) == "fused" and _route("mask", mask_rate=0.1, **nf) == "fused"
    assert _route("mask", mask=True, mask_rate=0.1, **nf) == "fused"
    assert _route("mask", mask=True, mask_rate=0.25, n_users=96, n_items=80) == "fused"
    # ... and every refusal of the docstring: the batch cap, dropout (with or without its own switch), --mask with an empty list
    assert _route("mask", mask=True, mask_rate=0.1, b_max=CAP + 1, **nf) == "modular"
    assert _route("mask", mask_rate=0.1, b_max=CAP + 1, **nf) == "modular"
    for fd in (None, "1"):
        assert _route("mask", fd, mask=True, mask_rate=0.1, drop_rate=0.5, **nf) == "modular"
        assert _route("mask", fd, mask_rate=0.1, drop_rate=0.5, **nf) == "modular"
    assert _route("mask", mask=True, mask_rate=0.0, **nf) == "modular"                          # --mask at rate 0: both lists empty
    assert _route("mask", mask=True, mask_rate=0.01, n_users=96, n_items=80) == "modular"        # int(0.96) == 0
    assert _route("mask", mask=True, mask_rate=0.012, n_users=96, n_items=80) == "modular"       # one user, no item
    assert _route("mask", mask=True, mask_rate=0.1) == "modular"                                 # sizes unknown
    assert _route("mask", mask_rate=0.001, n_users=96, n_items=80) == "fused"                    # without --mask an empty list is no NaN
    assert _route("mask", mask_rate=1.5, **nf) == "modular" and _route("mask", mask_rate=-0.1, **nf) == "modular"
    # every other value of the variable answers as before
    for fused in (None, "1", "wide", "0"):
        assert _route(fused, mask=True, mask_rate=0.1, **nf) == "modular" and _route(fused, mask_rate=0.1, **nf) == "modular"
    assert "LLMREC_FUSED" in SO.TRAINER_SWITCHES and len(SO.ENV_SWITCHES + SO.TRAINER_SWITCHES) == 13


LATENCY_NNZ = 1 << 20
NF = dict(n_users=13187, n_items=17366, d=64, n_attr=5, drop_rate=0.0, wgrad_rows_default=True, inline_adamw_default=True,
          fold_default=True, bwd_nnz=68933, bwd_valued=False, bwd_col_scaled=True, latency_nnz=LATENCY_NNZ)
NF_DEFAULT = SO.StepOptions(drop_rate=0.0, check_zero=False, multi_stream=False, gemm="bf16x3", preprop=True, wgrad_rows=True,
                            inline_adamw=True, fold=True, bwd_mask=True, bwd_zero_skip=True, host_chain=True)


def test_resolve_with_mask_items_and_restore():
    assert SO.resolve({}, **NF) == NF_DEFAULT == SO.resolve({}, **NF, mask_items=False, restore=False)
    masked = NF_DEFAULT._replace(preprop=False, wgrad_rows=False)
    assert SO.resolve({}, **NF, mask_items=True) == masked                                       # the batch's rows still bound the gradient
    assert SO.resolve({}, **NF, mask_items=True, restore=True) == masked._replace(bwd_mask=False, bwd_zero_skip=False)
    assert SO.resolve({"LLMREC_PREPROPAGATE": "0"}, **NF, mask_items=True) == masked
    assert SO.resolve({"LLMREC_GEMM": "f32"}, **NF, mask_items=True, restore=True) == masked._replace(gemm="f32", bwd_mask=False, bwd_zero_skip=False)
    with pytest.raises(RuntimeError, match="LLMREC_PREPROPAGATE"):
        SO.resolve({"LLMREC_PREPROPAGATE": "1"}, **NF, mask_items=True)
    assert SO.StepOptions._fields[-2:] == ("host_chain", "host_wgrad") and len(SO.StepOptions._fields) == 12


# ------------------------------------------------------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------------------------------------------------------
def _ptrs(*a):
    return (C.c_void_p * len(a))(*a)


def test_the_header_declares_the_entry_points_and_the_library_exports_them():
    protos = _lib.parse_header()
    want = {"llmrec_mask_nodes": 8, "llmrec_col_sums_f64": 7, "llmrec_mask_rows_f32": 9, "llmrec_restore_loss_f32": 22, "llmrec_restore_finish_f32": 12}
    lib = _lib.load()
    for name, n_args in want.items():
        assert len(protos[name][1]) == n_args and getattr(lib, name), name
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8 and lib.llmrec_abi_version() == 8              # additive: the ABI version stays
    assert _lib.CONST["LLMREC_MASK_ROW_LANES"] == 8 and _lib.CONST["LLMREC_MASK_MAX_TENSORS"] == 8
    from llmrec_amd.build import SOURCES
    assert "mask.hip" in SOURCES


def test_every_entry_point_refuses_what_its_header_says_before_any_hip_call():
    lib = _lib.load()

    def nodes(N=96, m=24, step=FAKE, side=0, out=FAKE + 0x1000):
        return lib.llmrec_mask_nodes(N, m, 1, step, side, out, None, None)
    for kw in (dict(N=0), dict(N=1 << 40), dict(m=-1), dict(m=97), dict(side=2), dict(side=-1), dict(step=None), dict(out=None)):
        assert nodes(**kw) == EINVAL and b"mask_nodes" in lib.llmrec_last_error(), kw

    X, Sm = _ptrs(FAKE, FAKE + 0x10000), _ptrs(FAKE + 0x100000, FAKE + 0x110000)

    def rows(entry, n=2, Xp=X, ldx=60, sums=Sm, N=96, cols=56, nodes=FAKE + 0x200000, m=24):
        if entry == "col_sums":
            return lib.llmrec_col_sums_f64(n, Xp, ldx, sums, N, cols, None)
        return lib.llmrec_mask_rows_f32(n, Xp, ldx, sums, N, cols, nodes, m, None)
    bad = [dict(n=0), dict(n=9), dict(N=0), dict(cols=0), dict(ldx=55), dict(Xp=None), dict(sums=None), dict(Xp=_ptrs(FAKE, None)),
           dict(sums=_ptrs(FAKE + 0x100000, None)), dict(Xp=_ptrs(FAKE + 2, FAKE)), dict(sums=_ptrs(FAKE + 0x100004, FAKE + 0x110000))]
    for kw in bad:
        for entry in ("col_sums", "mask_rows"):
            assert rows(entry, **kw) == EINVAL and entry.encode() in lib.llmrec_last_error(), (entry, kw)
    for kw in (dict(m=-1), dict(m=97), dict(nodes=None)):
        assert rows("mask_rows", **kw) == EINVAL and b"mask_rows" in lib.llmrec_last_error(), kw
    assert rows("mask_rows", m=0) == 0                                    # nothing to mask: no launch

    Xs, Ts, Ds = _ptrs(FAKE), _ptrs(FAKE + 0x100000), _ptrs(FAKE + 0x200000)

    def loss(n=1, Xp=Xs, ldx=64, Tp=Ts, ldt=56, Dp=Ds, lddx=64, nodes=FAKE + 0x300000, m=20, d=64, Fd=56, W=FAKE + 0x400000, ldw=64,
             b=FAKE + 0x500000, kind=0, alpha=2.0, rl=FAKE + 0x600000, lo=FAKE + 0x700000, flags=None, stamp=None):
        return lib.llmrec_restore_loss_f32(n, Xp, ldx, Tp, ldt, Dp, lddx, nodes, m, d, Fd, W, ldw, b, kind, alpha, 1.0, rl, lo, flags, stamp, None)
    bad = [dict(n=0), dict(n=9), dict(m=0), dict(m=1 << 31), dict(Fd=0), dict(d=0), dict(kind=2), dict(kind=-1), dict(alpha=0.5), dict(alpha=65.0),
           dict(alpha=float("nan")), dict(nodes=None), dict(W=None), dict(b=None), dict(rl=None), dict(lo=None), dict(Xp=None), dict(Tp=None),
           dict(Xp=_ptrs(None)), dict(Tp=_ptrs(None)), dict(Dp=_ptrs(None)), dict(flags=FAKE + 0x800000), dict(stamp=FAKE + 0x800000),
           dict(ldx=63), dict(ldt=55), dict(ldw=63), dict(lddx=63), dict(Xp=_ptrs(FAKE + 2)), dict(Tp=_ptrs(FAKE + 0x100001)),
           dict(Dp=_ptrs(FAKE + 0x200002)), dict(W=FAKE + 0x400002), dict(b=FAKE + 0x500001)]
    for kw in bad:
        assert loss(**kw) == EINVAL and b"restore_loss" in lib.llmrec_last_error(), kw
    for d in (32, 128):
        assert loss(d=d, ldx=d, ldw=d, lddx=d) == EUNSUPPORTED and b"restore_loss" in lib.llmrec_last_error()

    V = _ptrs(FAKE)

    def finish(nv=6, vals=FAKE + 0x900000, views=V, n_views=1, ld=448, cols=320, nodes=FAKE + 0x300000, m=20):
        return lib.llmrec_restore_finish_f32(nv, vals, 0.5, FAKE + 0xA00000, FAKE + 0xB00000, n_views, views, ld, cols, nodes, m, None)
    for kw in (dict(nv=-1), dict(nv=17), dict(vals=None), dict(n_views=-1), dict(n_views=9), dict(m=-1), dict(views=None), dict(nodes=None),
               dict(cols=0), dict(ld=319), dict(views=_ptrs(None)), dict(views=_ptrs(FAKE + 2))):
        assert finish(**kw) == EINVAL and b"restore_finish" in lib.llmrec_last_error(), kw
    assert finish(nv=0, n_views=0) == 0 and finish(nv=0, m=0) == 0          # nothing to do: no launch


def test_ops_refuse_cpu_tensors_and_mismatched_views():
    step = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_nodes(96, 24, 1, step, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.col_sums([torch.zeros(4, 4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_rows_([torch.zeros(4, 4)], [torch.zeros(4, dtype=torch.float64)], torch.zeros(1, dtype=torch.int64))
