"""GPU: dropout inside the fused step (opt-in: LLMREC_FUSED_DROPOUT=1 / FusedStep(drop_rate=)). torch's dropout stream cannot be reproduced
on the device and the reference ships no vectors for --drop_rate, so the contract is: the mask is the documented function of
(seed, step, tensor, row, column) - llmrec_dropout_rows_f32 against the numpy restatement tests/_dropout_ref.py, bit for bit - and a whole
step equals the per-op autograd path with the same masks injected, to the project's 1e-4 (tests/test_gpu_step.py's RTOL).

Worst relative errors of test_fused_step_matches_autograd_with_the_same_masks on an MI355X (nf_tiny, three steps, p = 0.5), bound 1e-4:
eager 6.9e-7 (step 0, image_trans.weight's gradient), graph 6.9e-7 (the same), f32 1.0e-6 (step 1, user_id_embedding.weight's gradient),
streams 6.9e-7; the loss itself within 1.4e-7 on all four.

That whole-step test measures max |a - b| / max |b| per tensor against the project's own per-op path on a 96 x 80 graph. The ROW-LEVEL
statement - every forward and gradient row against a float64 oracle with the restated masks, at p = 0.3 on a four-island 3000 x 800
graph, dropped elements exactly +0.0 - is tests/test_gpu_step_rows_modes.py, case D."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _dropout_ref as R
from tests._dropin import golden_argv
from tests._step_env import fused_trainer
from tests.conftest import GoldenCase
from tests.test_gpu_step import RTOL, TRAINABLE, rel

SENTINEL = -77.25
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.25], dtype=np.float32)


def _counter(value=0):
    """A device step counter as FusedStep keeps it: uint64 [1]."""
    return torch.tensor([value], dtype=torch.int64).cuda().view(torch.uint64)


def _read(counter):
    return int(counter.view(torch.int64).cpu()[0]) & (2 ** 64 - 1)


def _input(rows, cols, seed):
    """fp32 [rows, cols]: normal values of both signs with zeros, -0.0, the infinities, a NaN and a negative sprinkled over every 5th slot."""
    x = np.random.default_rng(seed).standard_normal((rows, cols)).astype(np.float32)
    flat = x.reshape(-1)
    at = np.arange(0, flat.size, 5)
    flat[at] = SPECIALS[np.arange(at.size) % SPECIALS.size]
    return x


def _same_bits(got: torch.Tensor, want: np.ndarray):
    """Equal bit for bit (so +0.0 is not -0.0) outside the NaNs, and NaN exactly where the restatement has one."""
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# (rows, cols, ldx, first column): the single element; guarded (cols % 4 != 0 groups, ldx == cols and ldx > cols); whole float4 groups;
# more than one block with 112 groups per row (a 128-lane tile); a view whose base is 4 bytes past a 16-byte boundary
SHAPES = [(1, 1, 1, 0), (37, 20, 20, 0), (37, 20, 24, 0), (96, 64, 64, 0), (1000, 448, 448, 0), (257, 63, 512, 1)]


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("rows,cols,ldx,first", SHAPES)
def test_kernel_matches_the_restatement_bit_for_bit(rows, cols, ldx, first, p):
    from llmrec_amd import ops
    seed, step, tag = 0x1234_5678_9ABC_DEF0, 3, 1
    x = _input(rows, cols, rows * 1000 + cols)
    buf = np.full((rows, ldx), SENTINEL, dtype=np.float32)
    buf[:, first:first + cols] = x
    dev = torch.from_numpy(buf).cuda()
    view = dev[:, first:first + cols]
    assert view.data_ptr() % 16 == (4 * first) % 16
    ops.dropout_rows_(view, p, seed, _counter(step), tag)
    want = buf.copy()
    want[:, first:first + cols] = R.apply(x, p, seed, step, tag)
    assert _same_bits(dev, want)                                         # the values AND the sentinels around them
    keep = R.keep_mask(rows, cols, p, seed, step, tag)
    got = view.cpu().numpy()
    assert np.all(got.view(np.uint32)[~keep] == 0)                        # dropped: +0.0 whatever x was
    if rows * cols > 5000:                                                # (> 500 non-finite inputs: both fates meet an inf / a NaN)
        assert (~keep & ~np.isfinite(x)).any() and (keep & ~np.isfinite(x)).any()


def test_counter_is_read_without_a_ticket_and_advanced_once_with_one():
    from llmrec_amd import ops
    rows, cols, p, seed, tag = 1000, 448, 0.5, 99, 0
    x = _input(rows, cols, 5)
    # no ticket: the launch only reads the counter
    step = _counter(6)
    a, b = torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda()
    ops.dropout_rows_(a, p, seed, step, tag)
    ops.dropout_rows_(b, p, seed, step, tag)
    assert _same_bits(a, b.cpu().numpy()) and _read(step) == 6
    assert _same_bits(a, R.apply(x, p, seed, 6, tag))
    # a ticket: the launch's 500 blocks count themselves off, the last one advances the counter and leaves the ticket at 0
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    c = torch.from_numpy(x).cuda()
    ops.dropout_rows_(c, p, seed, step, tag, ticket=ticket)
    assert _same_bits(c, R.apply(x, p, seed, 6, tag))                    # every block read the counter before it moved
    assert _read(step) == 7 and int(ticket) == 0
    e = torch.from_numpy(x).cuda()
    ops.dropout_rows_(e, p, seed, step, tag, ticket=ticket)
    assert _same_bits(e, R.apply(x, p, seed, 7, tag))
    assert _read(step) == 8 and int(ticket) == 0
    # the counter's high word reaches the mask
    high = _counter(2 ** 32 + 3)
    h = torch.from_numpy(x).cuda()
    ops.dropout_rows_(h, p, seed, high, tag)
    assert _same_bits(h, R.apply(x, p, seed, 2 ** 32 + 3, tag))
    assert not _same_bits(h, R.apply(x, p, seed, 3, tag))
    with pytest.raises(RuntimeError):
        ops.dropout_rows_(torch.zeros(4, 4), p, seed, step, tag)         # a CPU tensor: no fallback


def _trainer(monkeypatch, env, extra, seed=None):
    g = GoldenCase("nf_tiny")
    m, tr, _, _ = fused_trainer(monkeypatch, golden_argv(g) + list(extra), env, seed=g.args["seed"] if seed is None else seed)
    return g, m, tr


def _batch(g, s):
    return tuple(torch.tensor(g.z["step%d/%s" % (s, n)]).cuda() for n in ("users", "pos", "neg"))


def _run_steps(g, tr, n_steps, before_step=None):
    """n_steps training steps on the golden batches -> per step (loss, the 8 (mf, emb) pairs, {name: grad}, {name: param}) as numpy."""
    log, out = [], []
    tr._on_bpr = lambda mf, emb: log.append((float(mf), float(emb)))
    for s in range(n_steps):
        if before_step is not None:
            before_step(s)
        log.clear()
        loss, _, _ = tr.train_step(*_batch(g, s))
        params = dict(tr.model_mm.named_parameters())
        out.append((float(loss), np.array(log), {nm: params[nm].grad.detach().cpu().numpy().copy() for nm in TRAINABLE},
                    {nm: params[nm].detach().cpu().numpy().copy() for nm in TRAINABLE}))
    return out


_AUTOGRAD = {}


def _autograd_with_injected_masks(monkeypatch, p, n_steps):
    """The per-op autograd path (LLMREC_FUSED=0) with Models._drop replaced by the restated masks of steps 0 .. n_steps - 1, in the
    call order of Models.forward: image = slice 0, text = slice 1, the user profile = tag 1, attribute k = slice 2 + k. Computed once."""
    if (p, n_steps) in _AUTOGRAD:
        return _AUTOGRAD[(p, n_steps)]
    g, m, tr = _trainer(monkeypatch, {"LLMREC_FUSED": "0"}, ["--drop_rate", str(p)])
    assert tr._fused_step() is False
    model, seed = tr.model_mm, m.args.seed
    d, S = model.embedding_dim, 2 + len(model.item_feats)
    state = {"step": 0, "call": 0}
    scale = float(R.scale(p))

    def factor(keep):
        return torch.from_numpy(keep.astype(np.float32) * np.float32(scale)).cuda()

    def drop(x):
        call, s = state["call"], state["step"]
        state["call"] += 1
        if call == 2:
            return x * factor(R.keep_mask(model.n_users, d, p, seed, s, R.TAG_USER_PROFILE))
        sl = call if call < 2 else call - 1
        keep = R.keep_mask(model.n_items, S * d, p, seed, s, R.TAG_ITEM_STREAMS)[:, sl * d:(sl + 1) * d]
        return x * factor(keep)
    model._drop = drop

    def before(s):
        state["step"], state["call"] = s, 0
    out = _run_steps(g, tr, n_steps, before)
    assert state["call"] == 1 + S                                         # one forward per step, every projection dropped once
    _AUTOGRAD[(p, n_steps)] = out
    return out


@pytest.mark.parametrize("path", ["eager", "graph", "f32", "streams"])
def test_fused_step_matches_autograd_with_the_same_masks(path, monkeypatch):
    """Three steps of the drop-in at --drop_rate 0.5 in the fused step against the autograd path with the same masks: the loss, the eight
    (mf, emb) pairs, every gradient and every parameter within RTOL = 1e-4 (tests/test_gpu_step.py's). path: eager launches, the captured
    graph, the exact-fp32 GEMMs, four streams (eager)."""
    from llmrec_amd.fused import FusedStep
    p, n_steps = 0.5, 3
    want = _autograd_with_injected_masks(monkeypatch, p, n_steps)
    env = {"LLMREC_FUSED": "1", "LLMREC_FUSED_DROPOUT": "1", "LLMREC_GRAPH": "1" if path == "graph" else "0",
           "LLMREC_GEMM": "f32" if path == "f32" else "bf16x3", "LLMREC_STREAMS": "1" if path == "streams" else "0"}
    g, m, tr = _trainer(monkeypatch, env, ["--drop_rate", str(p)])
    fused = tr._fused_step()
    assert isinstance(fused, FusedStep) and fused.drop_rate == p and fused.drop_seed == m.args.seed and fused.preprop is False
    got = _run_steps(g, tr, n_steps)
    assert _read(fused.drop_step) == n_steps and int(fused.drop_ticket) == 0
    worst = (0.0, None)
    for s, ((loss, bpr, grads, params), (loss0, bpr0, grads0, params0)) in enumerate(zip(got, want)):
        errs = {"loss": abs(loss - loss0) / abs(loss0), "bpr": rel(bpr, bpr0)}
        assert bpr.shape == bpr0.shape == (8, 2)
        errs.update({"grad/" + nm: rel(grads[nm], grads0[nm]) for nm in TRAINABLE})
        errs.update({"param/" + nm: rel(params[nm], params0[nm]) for nm in TRAINABLE})
        top = max(errs, key=errs.get)
        worst = max(worst, (errs[top], (s, top)), key=lambda e: e[0])
        print("dropout step parity [%s] step %d: worst %.2e (%s), loss %.2e" % (path, s, errs[top], top, errs["loss"]))
        for nm, e in errs.items():
            assert e < RTOL, (path, s, nm, e)
    print("dropout step parity [%s]: worst relative error %.2e at %s" % (path, worst[0], worst[1]))


def _step_object(monkeypatch, env=None, cls=None, preprop=None, **kw):
    """A fresh drop-in Trainer (seeded: identical initialisation) and a step object of the given class over its model."""
    from llmrec_amd import ops
    from llmrec_amd.fused import FusedStep
    g, m, tr = _trainer(monkeypatch, dict(env or {}, **({} if preprop is None else {"LLMREC_PREPROPAGATE": preprop})), [])
    graph = type("G", (), {"ui": ops.operand_from_sparse_tensor(tr.ui_graph), "iu": ops.operand_from_sparse_tensor(tr.iu_graph)})
    a = m.args
    b_max = max(g.z["step%d/users" % s].size for s in range(g.n_steps))
    step = (cls or FusedStep)(tr.model_mm, graph, tr.hyper, (a.model_cat_rate, a.user_cat_rate, a.item_cat_rate), tr.optimizer, b_max, **kw)
    return g, m, tr, step


def _state(tr, step):
    params = dict(tr.model_mm.named_parameters())
    out = {nm: params[nm].detach().clone() for nm in TRAINABLE}
    for nm in TRAINABLE:
        m1, m2 = step.opt.state[params[nm]]
        out["m/" + nm], out["v/" + nm] = m1.clone(), m2.clone()
    return out


def test_graph_replays_draw_new_masks_and_same_seed_runs_agree(monkeypatch):
    """One capture (its warm-up is a real step) + three replays = four eager steps of a second object in the same state: every parameter
    and both AdamW moments, torch.equal. The counter lives on the device: it reads 4 on both. Another drop_seed trains other parameters."""
    env = {"LLMREC_GRAPH": "1", "LLMREC_STREAMS": "0"}
    g, _, tr_g, st_g = _step_object(monkeypatch, env, drop_rate=0.5, drop_seed=7)
    _, _, tr_e, st_e = _step_object(monkeypatch, env, drop_rate=0.5, drop_seed=7)
    _, _, tr_o, st_o = _step_object(monkeypatch, env, drop_rate=0.5, drop_seed=8)
    tr_g.model_mm.train(); tr_e.model_mm.train(); tr_o.model_mm.train()
    batch = _batch(g, 0)
    st_g.capture(*batch)
    for _ in range(3):
        st_g.step(*batch)
    for _ in range(4):
        st_e.step_eager(*batch)
        st_o.step_eager(*batch)
    torch.cuda.synchronize()
    assert _read(st_g.drop_step) == 4 and _read(st_e.drop_step) == 4 and int(st_g.drop_ticket) == 0 and int(st_e.drop_ticket) == 0
    sg, se, so = _state(tr_g, st_g), _state(tr_e, st_e), _state(tr_o, st_o)
    for nm in se:
        assert torch.equal(sg[nm], se[nm]), nm
    assert all(bool(torch.isfinite(t).all()) for t in se.values())
    for nm in ("image_trans.weight", "user_trans.weight", "item_trans.weight", "item_id_embedding.weight"):
        assert not torch.equal(so[nm], se[nm]), nm
    # four different masks: had a replay reused the capture's, P_usr's zeros of the last step would be the first step's
    last = (st_g.P_usr == 0).cpu().numpy()
    assert np.array_equal(last, ~R.keep_mask(st_g.U, st_g.d, 0.5, 7, 3, R.TAG_USER_PROFILE))


def test_evaluation_is_dropout_free_and_leaves_the_counter(monkeypatch):
    """eval_topk of a drop_rate = 0.5 step = eval_topk of a drop_rate = 0 step over the same parameters, torch.equal. (The rate-0 step is
    built in the same order of operations, LLMREC_PREPROPAGATE=0: bit equality is a statement about one arithmetic.)"""
    g, m, tr_d, st_d = _step_object(monkeypatch, drop_rate=0.5, drop_seed=7)
    _, _, tr_0, st_0 = _step_object(monkeypatch, preprop="0", drop_rate=0.0)
    assert st_0.preprop is False and st_d.preprop is False
    tr_d.model_mm.train()
    st_d.step_eager(*_batch(g, 0))                                       # parameters have moved, P_cat / P_usr hold dropped values
    assert _read(st_d.drop_step) == 1
    tr_0.model_mm.load_state_dict(tr_d.model_mm.state_dict())
    tr_d.model_mm.eval(); tr_0.model_mm.eval()
    q = torch.tensor(g.z["eval/users"]).cuda()
    train = m.data_generator.device_state(m.device)["train"]
    with torch.no_grad():
        idx_d, sc_d = st_d.eval_topk(q, train, 20)
        idx_0, sc_0 = st_0.eval_topk(q, train, 20)
    assert torch.equal(idx_d, idx_0) and torch.equal(sc_d, sc_0)
    assert not bool((st_d.P_usr == 0).any())                              # the evaluation's projections are whole
    assert _read(st_d.drop_step) == 1 and int(st_d.drop_ticket) == 0


def test_defaults_are_unchanged_and_unsupported_combinations_raise(monkeypatch):
    from llmrec_amd.dp import DataParallelStep
    from llmrec_amd.fused import FusedStep
    env = {"LLMREC_STREAMS": "0"}
    g, m, tr_a, plain = _step_object(monkeypatch, env)                   # the constructor as every caller wrote it so far
    _, _, tr_b, zero = _step_object(monkeypatch, env, drop_rate=0.0)
    _, _, tr_c, ref_order = _step_object(monkeypatch, env, preprop="0", drop_rate=0.0)
    _, _, tr_d, half = _step_object(monkeypatch, env, drop_rate=0.5, drop_seed=1)
    batch = _batch(g, 0)
    for tr, st in ((tr_a, plain), (tr_b, zero), (tr_c, ref_order), (tr_d, half)):
        tr.model_mm.train()
        st.step_eager(*batch)
    assert zero.preprop == plain.preprop and zero.entry_point_calls_per_step == plain.entry_point_calls_per_step
    assert zero.drop_rate == 0.0 and not hasattr(zero, "drop_step") and not hasattr(zero, "drop_ticket")
    assert half.preprop is False and ref_order.preprop is False
    assert half.entry_point_calls_per_step == ref_order.entry_point_calls_per_step + 4
    assert half.drop_step.dtype == torch.uint64 and half.drop_step.shape == (1,) and half.drop_ticket.dtype == torch.int32
    args = (tr_a.model_mm, type("G", (), {"ui": plain.ui, "iu": plain.iu}), tr_a.hyper, (plain.c_m, plain.c_u, plain.c_a), tr_a.optimizer, plain.b_max)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            FusedStep(*args, drop_rate=bad)
    with pytest.raises(RuntimeError, match="drop_rate"):
        DataParallelStep(*args, rank=0, world=1, drop_rate=0.5)
    monkeypatch.setenv("LLMREC_PREPROPAGATE", "1")
    with pytest.raises(RuntimeError, match="LLMREC_PREPROPAGATE"):
        FusedStep(*args, drop_rate=0.5)
    monkeypatch.delenv("LLMREC_PREPROPAGATE")
    # the drop-in: the switch alone changes nothing at --drop_rate 0, and --drop_rate > 0 without it leaves the fused step
    _, _, tr = _trainer(monkeypatch, {"LLMREC_STREAMS": "0", "LLMREC_FUSED_DROPOUT": "1"}, ["--drop_rate", "0"], seed=3)
    fused = tr._fused_step()
    assert isinstance(fused, FusedStep) and fused.drop_rate == 0.0 and fused.preprop == plain.preprop and not hasattr(fused, "drop_step")
    _, _, tr = _trainer(monkeypatch, env, ["--drop_rate", "0.5"], seed=3)
    assert tr._fused_step() is False
