"""GPU: feature masking and attribute restoration inside the fused step (opt-in: LLMREC_FUSED=mask / FusedStep(mask_rate=, mask_items=, ...)).
torch.randperm's lists cannot be reproduced on the device, so the contract is: the lists are the documented function of (seed, round, side) -
llmrec_mask_nodes against tests/_mask_ref.py, bit for bit; a masking round stores the fp32 mean of the running fp64 sums, which stay
within their bound of a from-scratch sum; the restoration launch's value and every gradient element are within the bound derived from
its own order of operations; and a whole step equals the per-op autograd path with the same lists injected, to the project's 1e-4
(tests/test_gpu_step.py's RTOL).

Measured on an MI355X. test_fused_step_matches_autograd_with_the_same_lists (nf_tiny, three steps and an evaluation), worst relative error
against the bound 1e-4: eager sce 7.3e-7 (step 1, text_trans.bias' gradient), graph sce 7.3e-7 (the same), f32 sce 1.1e-6 (step 0,
item_id_embedding.weight's gradient), eager mse 6.5e-7, four streams 7.3e-7; the top-20 scores within 2.4e-7 on all five; user masking alone 5.5e-7. The running sums came out equal
to the restated tree bit for bit. test_restoration_value_and_gradient_within_the_bound: worst error / bound 0.99 - the update of a
non-zero destination row ends in one rounding, whose bound u |result| is tight by nature.

The whole-step tests here measure max |a - b| / max |b| per tensor against the project's own per-op path on a 96 x 80 graph, where almost
no mask node lies outside the batch's reach. The ROW-LEVEL statement - every forward and gradient row and the restoration's stream losses
against a float64 oracle, every masking round on its own, sc_I all-zero after every step, on a four-island 3000 x 800 graph with 70 % of
the item list beyond the batch's reach - is tests/test_gpu_step_rows_modes.py, cases K, K_MSE and U."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _mask_ref as R
from tests._dropin import golden_argv
from tests._step_env import fused_trainer
from tests.conftest import GoldenCase
from tests.test_gpu_step import RTOL, TRAINABLE, rel
from tests.test_mask_ref_cpu import _case

SENTINEL = -77.25
SEED = 0x1234_5678_9ABC_DEF0


def _counter(value=0):
    return torch.tensor([value - (1 << 64) if value >= (1 << 63) else value], dtype=torch.int64).cuda().view(torch.uint64)


def _read(counter):
    return int(counter.view(torch.int64).cpu()[0]) & (2 ** 64 - 1)


# ------------------------------------------------------------------------------------------------------------------------------------
# kernels against the restatement
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,m", [(1, 1), (96, 24), (80, 20), (5000, 1), (5000, 4999)])
def test_node_lists_match_the_restatement_bit_for_bit(N, m):
    from llmrec_amd import ops
    for rnd in (0, 3, 2 ** 32 + 3):
        step = _counter(rnd)
        for side in (ops.MASK_SIDE_USERS, ops.MASK_SIDE_ITEMS):
            got = ops.mask_nodes(N, m, SEED, step, side).cpu().numpy()
            assert np.array_equal(got, R.nodes(N, m, SEED, rnd, side)), (N, m, rnd, side)
        assert _read(step) == rnd                                         # no ticket: the counter is only read


def test_the_ticketed_launch_advances_the_round_once_and_leaves_the_ticket_at_zero():
    from llmrec_amd import ops
    step, ticket = _counter(6), torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(4999, dtype=torch.int64, device="cuda")
    users = ops.mask_nodes(5000, 4999, 9, step, ops.MASK_SIDE_USERS).cpu().numpy()
    items = ops.mask_nodes(5000, 4999, 9, step, ops.MASK_SIDE_ITEMS, out=out, ticket=ticket).cpu().numpy()      # 20 blocks count themselves off
    assert np.array_equal(users, R.nodes(5000, 4999, 9, 6, 0)) and np.array_equal(items, R.nodes(5000, 4999, 9, 6, 1))
    assert _read(step) == 7 and int(ticket) == 0
    assert np.array_equal(ops.mask_nodes(5000, 20, 9, step, ops.MASK_SIDE_ITEMS, ticket=ticket).cpu().numpy(), R.nodes(5000, 20, 9, 7, 1))
    assert _read(step) == 8 and int(ticket) == 0
    ops.mask_nodes(5000, 0, 9, step, ops.MASK_SIDE_USERS, ticket=ticket)                                        # an empty list still counts the round
    assert _read(step) == 9 and int(ticket) == 0


@pytest.mark.parametrize("N,cols,ldx", [(96, 56, 56), (80, 56, 60), (300, 200, 200)])
def test_masking_rounds_store_the_mean_and_keep_the_running_sums(N, cols, ldx):
    from llmrec_amd import ops
    rng = np.random.default_rng(N + cols)
    m, n_t = N // 4, 2                                                    # two tensors share the list (and the launch)
    host = [np.full((N, ldx), SENTINEL, dtype=np.float32) for _ in range(n_t)]
    for k, h in enumerate(host):
        h[:, :cols] = (rng.standard_normal((N, cols)) * (k + 1) + 0.25).astype(np.float32)
    dev = [torch.from_numpy(h).cuda() for h in host]
    views = [t[:, :cols] for t in dev]
    sums = ops.col_sums(views)
    bounds = [R.RunningBound(h[:, :cols]) for h in host]
    for k in range(n_t):
        got = sums[k].cpu().numpy()
        assert (np.abs(got - host[k][:, :cols].astype(np.float64).sum(0)) <= bounds[k].bound()).all()
        print("col_sums [%d x %d] tensor %d: equal to the restated tree: %s" % (N, cols, k, np.array_equal(got, R.col_sums(host[k][:, :cols]))))
    for rnd in range(5):
        nodes = R.nodes(N, m, 77, rnd, R.SIDE_ITEMS)
        before = [s.cpu().numpy().copy() for s in sums]
        ops.mask_rows_(views, sums, torch.from_numpy(nodes).cuda())
        for k in range(n_t):
            mean = (before[k] / np.float64(N)).astype(np.float32)          # the fp32 mean of the sums the launch read
            bounds[k].round(host[k][nodes][:, :cols], mean, before[k])
            host[k][nodes, :cols] = mean
            got = dev[k].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), host[k].view(np.uint32)), (rnd, k)   # the rows, the other rows and columns [cols, ldx)
    fresh = ops.col_sums(views)
    for k in range(n_t):
        run, exact, b = sums[k].cpu().numpy(), host[k][:, :cols].astype(np.float64).sum(0), bounds[k].bound()
        print("running sums [%d x %d] tensor %d after 5 rounds: worst error / bound %.3g" % (N, cols, k, (np.abs(run - exact) / b).max()))
        assert (np.abs(run - exact) <= b).all()
        assert (np.abs(run - fresh[k].cpu().numpy()) <= b).all()
    ops.mask_rows_(views, sums, torch.zeros(0, dtype=torch.int64, device="cuda"))                  # an empty list: nothing moves
    assert all(np.array_equal(t.cpu().numpy().view(np.uint32), h.view(np.uint32)) for t, h in zip(dev, host))


LOSSES = [("sce", 1), ("sce", 2), ("sce", 3), ("mse", 1), ("mse", 2), ("mse", 3)]


@pytest.mark.parametrize("loss_type,alpha", LOSSES)
@pytest.mark.parametrize("Fdim", [56, 64, 200])
@pytest.mark.parametrize("rows", [1, 17, 130])
def test_restoration_value_and_gradient_within_the_bound(rows, Fdim, loss_type, alpha):
    """Two streams per launch (another X and T each, one list with gaps, one decoder); row 0 of the list has y = t up to rounding, row 1 is
    x = 0, which with the second run's b = 0 is F.normalize's eps branch. The destination rows hold values before (the launch adds)."""
    from llmrec_amd import ops
    d, scale, stamp = 64, 0.5, 41
    for zero_bias in (False, True):
        cases = [_case(rows, Fdim, 1000 * rows + Fdim + s, d) for s in range(2)]
        nodes, W, b = cases[0][2], cases[0][3], (np.zeros(Fdim, dtype=np.float32) if zero_bias else cases[0][4])
        n = cases[0][0].shape[0]
        Xs, Ts = [c[0] for c in cases], [c[1] for c in cases]
        for s in range(2):                                                # the second stream's special rows at the shared list's positions
            Ts[s][nodes[0]] = (Xs[s][nodes[0]].astype(np.float64) @ W.T.astype(np.float64) + b).astype(np.float32)
            if rows > 1:
                Xs[s][nodes[1]] = 0.0
        dst0 = [np.random.default_rng(5 + s).standard_normal((n, d)).astype(np.float32) for s in range(2)]
        cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dX, dn = [cuda(x) for x in dst0], cuda(nodes)
        row_loss, loss_out = torch.full((2 * rows,), SENTINEL, device="cuda"), torch.full((2,), SENTINEL, device="cuda")
        flags, stamp_dev = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.tensor([stamp], dtype=torch.int32, device="cuda")
        ops.restore_loss([cuda(x) for x in Xs], [cuda(t) for t in Ts], dn, cuda(W), cuda(b), loss_type, alpha, row_loss, loss_out, dXs=dX,
                         scale=scale, row_flags=flags, row_stamp=stamp_dev)
        want_flags = np.zeros(n, dtype=np.uint8)
        want_flags[nodes] = stamp % 255 + 1
        assert np.array_equal(flags.cpu().numpy(), want_flags)
        rl, lo = row_loss.cpu().numpy().astype(np.float64), loss_out.cpu().numpy().astype(np.float64)
        value_only_rl, value_only_lo = torch.full((2 * rows,), SENTINEL, device="cuda"), torch.full((2,), SENTINEL, device="cuda")
        ops.restore_loss([cuda(x) for x in Xs], [cuda(t) for t in Ts], dn, cuda(W), cuda(b), loss_type, alpha, value_only_rl, value_only_lo)
        assert torch.equal(value_only_rl, row_loss) and torch.equal(value_only_lo, loss_out)       # value only: the same values ...
        others = np.setdiff1d(np.arange(n), nodes)
        worst = 0.0
        for s in range(2):
            exact = R.restore(Xs[s], Ts[s], nodes, W, b, loss_type, alpha, scale=scale)
            bound = R.restore_bound(Xs[s], Ts[s], nodes, W, b, loss_type, alpha, scale=scale, dst0=dst0[s][nodes])
            assert np.isfinite(bound["grad"]).all() and np.isfinite(bound["row_loss"]).all()
            got = dX[s].cpu().numpy()
            assert np.array_equal(got[others].view(np.uint32), dst0[s][others].view(np.uint32))     # ... and no row outside the list is written
            e_rows = np.abs(rl[s * rows:(s + 1) * rows] - exact["row_loss"])
            e_grad = np.abs(got[nodes].astype(np.float64) - (dst0[s][nodes] + exact["grad"]))
            worst = max(worst, (e_rows / bound["row_loss"]).max(), abs(lo[s] - exact["loss"]) / bound["loss"], (e_grad / bound["grad"]).max())
            assert (e_rows <= bound["row_loss"]).all(), (s, zero_bias)
            assert abs(lo[s] - exact["loss"]) <= bound["loss"], (s, zero_bias)
            assert (e_grad <= bound["grad"]).all(), (s, zero_bias, (e_grad / bound["grad"]).max())
            if zero_bias and rows > 1:
                assert np.abs(exact["grad"][1]).max() > 1e6                # the eps branch: 1 / 1e-12
        print("restore %s alpha %d rows %d F %d b=0:%s worst error / bound %.3g" % (loss_type, alpha, rows, Fdim, zero_bias, worst))


def test_restore_finish_adds_the_term_and_clears_the_listed_rows():
    from llmrec_amd import ops
    rng = np.random.default_rng(8)
    host = rng.standard_normal((80, 448)).astype(np.float32)
    sc, nodes = torch.from_numpy(host).cuda(), R.nodes(80, 20, 1, 0, 1)
    vals = torch.tensor([0.5, 0.25, 1.5, 2.0, 0.125, 3.0], device="cuda")
    scal, run = torch.tensor([9.0, 4.0, 7.0, 8.0], device="cuda"), torch.tensor([10.0, 20.0, 30.0], dtype=torch.float64, device="cuda")
    ops.restore_finish(vals, 0.5, scal, run, views=[sc[:, 128:]], nodes=torch.from_numpy(nodes).cuda())
    assert scal.tolist() == [9.0, 4.0 + 0.5 * 7.375, 7.0, 8.0] and run.tolist() == [10.0 + 0.5 * 7.375, 20.0, 30.0]
    host[nodes, 128:] = 0.0
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), host.view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------------------------
# whole steps
# ------------------------------------------------------------------------------------------------------------------------------------
MASK_ARGV = ["--mask", "True", "--mask_rate", "0.25", "--att_re_rate", "0.5"]
USER_ARGV = ["--mask_rate", "0.25"]


def _trainer(monkeypatch, env, extra, seed=None):
    g = GoldenCase("nf_tiny")
    m, tr, _, _ = fused_trainer(monkeypatch, golden_argv(g) + list(extra), env, seed=g.args["seed"] if seed is None else seed)
    return g, m, tr


def _batch(g, s):
    return tuple(torch.tensor(g.z["step%d/%s" % (s, n)]).cuda() for n in ("users", "pos", "neg"))


def _inject_lists(m, tr):
    """Models.MM_Model._mask_features with torch.randperm replaced by the restated lists, round after round in call order."""
    model, a, state = tr.model_mm, m.args, {"round": 0}

    def masked():
        rnd = state["round"]
        state["round"] += 1
        i_nodes = None
        if a.mask:
            i_nodes = torch.from_numpy(R.nodes(model.n_items, int(a.mask_rate * model.n_items), a.seed, rnd, R.SIDE_ITEMS))
            for key in model.item_feats:
                model.item_feats[key][i_nodes] = model.item_feats[key].mean(0)
        n_u = int(a.mask_rate * model.n_users)
        u_nodes = torch.from_numpy(R.nodes(model.n_users, n_u, a.seed, rnd, R.SIDE_USERS))
        if n_u > 0:
            model.user_feats[u_nodes] = model.user_feats.mean(0)
        return i_nodes, u_nodes
    model._mask_features = masked
    return state


def _run(g, m, tr, n_steps=3, eval_before=2):
    """n_steps training steps on the golden batches with one Trainer.test() ahead of step `eval_before` -> per step (loss, the 8 (mf, emb)
    pairs, {name: grad}, {name: param}) and the evaluation's top-20 scores."""
    from llmrec_amd import ops
    log, out, scores = [], [], None
    tr._on_bpr = lambda mf, emb: log.append((float(mf.detach()), float(emb.detach())))
    seen, calls = {}, []
    fused = tr._fused_step()
    if not fused:
        inner = tr.model_mm.forward

        def forward(*a, **kw):
            fw = inner(*a, **kw)
            seen["E"] = (fw[0].detach(), fw[1].detach())
            return fw
        tr.model_mm.forward = forward
    for s in range(n_steps):
        if s == eval_before:
            tr.test(g.z["eval/users"].tolist(), is_val=False)
            E_u, E_i = (fused.E_u, fused.E_i) if fused else seen["E"]
            q = torch.tensor(g.z["eval/users"]).cuda()
            with torch.no_grad():
                scores = ops.score_topk(E_u, E_i, q, m.data_generator.device_state(m.device)["train"], 20)[1].cpu().numpy().copy()
        log.clear()
        loss, _, _ = tr.train_step(*_batch(g, s))
        if fused:
            calls.append(fused.entry_point_calls_per_step)
        params = dict(tr.model_mm.named_parameters())
        out.append((float(loss), np.array(log), {nm: params[nm].grad.detach().cpu().numpy().copy() for nm in TRAINABLE},
                    {nm: params[nm].detach().cpu().numpy().copy() for nm in TRAINABLE}))
    return out, scores, calls


_AUTOGRAD = {}


def _autograd_with_injected_lists(monkeypatch, argv):
    key = tuple(argv)
    if key not in _AUTOGRAD:
        g, m, tr = _trainer(monkeypatch, {"LLMREC_FUSED": "0"}, argv)
        assert tr._fused_step() is False
        state = _inject_lists(m, tr)
        _AUTOGRAD[key] = _run(g, m, tr)
        assert state["round"] == 4                                        # three training forwards and one evaluation
    return _AUTOGRAD[key]


def _assert_parity(tag, got, want):
    (steps, scores, _), (steps0, scores0, _) = got, want
    worst = (0.0, None)
    for s, ((loss, bpr, grads, params), (loss0, bpr0, grads0, params0)) in enumerate(zip(steps, steps0)):
        errs = {"loss": abs(loss - loss0) / abs(loss0), "bpr": rel(bpr, bpr0)}
        assert bpr.shape == bpr0.shape == (8, 2)
        errs.update({"grad/" + nm: rel(grads[nm], grads0[nm]) for nm in TRAINABLE})
        errs.update({"param/" + nm: rel(params[nm], params0[nm]) for nm in TRAINABLE})
        top = max(errs, key=errs.get)
        worst = max(worst, (errs[top], (s, top)), key=lambda e: e[0])
        print("mask step parity [%s] step %d: worst %.2e (%s), loss %.2e" % (tag, s, errs[top], top, errs["loss"]))
        for nm, e in errs.items():
            assert e < RTOL, (tag, s, nm, e)
    e = rel(scores, scores0)
    print("mask step parity [%s]: worst relative error %.2e at %s; top-20 scores %.2e" % (tag, worst[0], worst[1], e))
    assert scores.shape == scores0.shape and e < RTOL, (tag, e)


def _fused_env(path):
    return {"LLMREC_FUSED": "mask", "LLMREC_GRAPH": "1" if path == "graph" else "0", "LLMREC_GEMM": "f32" if path == "f32" else "bf16x3",
            "LLMREC_STREAMS": "1" if path == "streams" else "0"}


@pytest.mark.parametrize("path,loss_type", [("eager", "sce"), ("graph", "sce"), ("f32", "sce"), ("eager", "mse"), ("streams", "sce")])
def test_fused_step_matches_autograd_with_the_same_lists(path, loss_type, monkeypatch):
    """nf_tiny (U = 96, I = 80, F = 56, five attribute streams) at --mask True --mask_rate 0.25 --att_re_rate 0.5 - 24 users and 20 items
    per round: three training steps with one Trainer.test() between the second and the third, against the per-op path with the restated
    lists of rounds 0 .. 3 injected. path: eager launches, the captured graph, the exact-fp32 GEMMs, four streams (eager)."""
    from llmrec_amd.fused import FusedStep
    argv = MASK_ARGV + ["--feat_loss_type", loss_type]
    want = _autograd_with_injected_lists(monkeypatch, argv)
    g, m, tr = _trainer(monkeypatch, _fused_env(path), argv)
    fused = tr._fused_step()
    assert isinstance(fused, FusedStep) and fused.mask_items and fused.restore and fused.preprop is False and fused.mask_seed == m.args.seed
    assert (fused.m_users, fused.m_items) == (24, 20) and not fused.bwd_mask and not fused.wgrad_rows
    got = _run(g, m, tr)
    assert _read(fused.mask_step) == 4 and int(fused.mask_ticket) == 0
    _assert_parity("%s %s" % (path, loss_type), got, want)
    assert float(fused.sc_I.abs().max()) == 0.0                          # the restoration's rows are cleared again


def test_user_masking_alone_keeps_the_default_schedule(monkeypatch):
    """--mask_rate 0.25 without --mask: user_feats only. preprop is the default step's, the step gains exactly the two user-side launches
    (the list, the rows), and three steps with an evaluation agree with the per-op path."""
    from llmrec_amd.fused import FusedStep
    want = _autograd_with_injected_lists(monkeypatch, USER_ARGV)
    _, _, tr0 = _trainer(monkeypatch, {"LLMREC_FUSED": "1", "LLMREC_GRAPH": "0", "LLMREC_STREAMS": "0"}, [])
    plain = tr0._fused_step()
    g, m, tr = _trainer(monkeypatch, _fused_env("eager"), USER_ARGV)
    fused = tr._fused_step()
    assert isinstance(fused, FusedStep) and fused.mask_rate == 0.25 and not fused.mask_items and not fused.restore
    assert fused.preprop == plain.preprop and fused.wgrad_rows == plain.wgrad_rows and fused.bwd_mask == plain.bwd_mask
    got = _run(g, m, tr)
    tr0.model_mm.train()
    for s, calls in enumerate(got[2]):                                    # step by step (a step object's first step issues more calls)
        plain.step_eager(*_batch(g, s))
        assert calls == plain.entry_point_calls_per_step + 2, (s, calls, plain.entry_point_calls_per_step)
    assert _read(fused.mask_step) == 4 and int(fused.mask_ticket) == 0 and not hasattr(fused, "re_vals")
    _assert_parity("users only", got, want)


def _step_object(monkeypatch, env=None, cls=None, mask=None, **kw):
    """A fresh drop-in Trainer (seeded: identical initialisation) and a step object over its model. mask: None, "users" or "items" (with
    the trainer's decoder and targets and att_re_rate 0.5); kw: further constructor arguments."""
    from llmrec_amd import ops
    from llmrec_amd.fused import FusedStep
    g, m, tr = _trainer(monkeypatch, dict(env or {}), [])
    graph = type("G", (), {"ui": ops.operand_from_sparse_tensor(tr.ui_graph), "iu": ops.operand_from_sparse_tensor(tr.iu_graph)})
    a = m.args
    if mask is not None:
        kw = dict(dict(mask_rate=0.25, mask_seed=7), **kw)
    if mask == "items":
        kw = dict(dict(mask_items=True, decoder=tr.decoder, user_targets=tr.user_init_embedding, item_targets=tr.item_attribute_embedding,
                       att_re_rate=0.5), **kw)
    b_max = max(g.z["step%d/users" % s].size for s in range(g.n_steps))
    args = (tr.model_mm, graph, tr.hyper, (a.model_cat_rate, a.user_cat_rate, a.item_cat_rate), tr.optimizer, b_max)
    return g, m, tr, (cls or FusedStep)(*args, **kw), args


def _state(tr, step):
    params = dict(tr.model_mm.named_parameters())
    out = {nm: params[nm].detach().clone() for nm in TRAINABLE}
    for nm in TRAINABLE:
        m1, m2 = step.opt.state[params[nm]]
        out["m/" + nm], out["v/" + nm] = m1.clone(), m2.clone()
    out["feat/user"] = tr.model_mm.user_feats.clone()
    out["sum/user"] = step.user_sums[0].clone()
    for k, key in enumerate(step.keys):
        out["feat/" + key], out["sum/" + key] = tr.model_mm.item_feats[key].clone(), step.item_sums[k].clone()
    return out


def test_graph_replays_draw_new_lists_and_same_seed_runs_agree(monkeypatch):
    """One capture (its warm-up is a real step) + three replays = four eager steps of a second object in the same state: every parameter,
    both AdamW moments, the masked feature tensors and the running sums, torch.equal. Another mask_seed trains other parameters."""
    env = {"LLMREC_GRAPH": "1", "LLMREC_STREAMS": "0"}
    g, _, tr_g, st_g, _ = _step_object(monkeypatch, env, mask="items")
    _, _, tr_e, st_e, _ = _step_object(monkeypatch, env, mask="items")
    _, _, tr_o, st_o, _ = _step_object(monkeypatch, env, mask="items", mask_seed=8)
    for tr in (tr_g, tr_e, tr_o):
        tr.model_mm.train()
    batch = _batch(g, 0)
    st_g.capture(*batch)
    for _ in range(3):
        st_g.step(*batch)
    for _ in range(4):
        st_e.step_eager(*batch)
        st_o.step_eager(*batch)
    torch.cuda.synchronize()
    assert _read(st_g.mask_step) == 4 and _read(st_e.mask_step) == 4 and int(st_g.mask_ticket) == 0 and int(st_e.mask_ticket) == 0
    sg, se, so = _state(tr_g, st_g), _state(tr_e, st_e), _state(tr_o, st_o)
    for nm in se:
        assert torch.equal(sg[nm], se[nm]), nm
    assert all(bool(torch.isfinite(t).all()) for t in se.values())
    for nm in ("user_trans.weight", "item_trans.weight", "item_id_embedding.weight", "feat/user"):
        assert not torch.equal(so[nm], se[nm]), nm
    # four different lists: the last round's is round 3's
    assert np.array_equal(st_g.mask_nodes_i.cpu().numpy(), R.nodes(st_g.I, 20, 7, 3, R.SIDE_ITEMS))
    assert np.array_equal(st_g.mask_nodes_u.cpu().numpy(), R.nodes(st_g.U, 24, 7, 3, R.SIDE_USERS))
    # refresh_feature_sums: the running sums are those of the matrices as they stand
    run = [s.clone() for s in st_e.item_sums]
    st_e.refresh_feature_sums()
    for a, b_ in zip(run, st_e.item_sums):
        assert float((a - b_).abs().max()) <= 1e-9 * float(b_.abs().max() + 1)


def test_check_zero_passes_through_restoration_steps(monkeypatch):
    g, _, tr, st, _ = _step_object(monkeypatch, {"LLMREC_CHECK_ZERO": "1", "LLMREC_STREAMS": "0"}, mask="items")
    tr.model_mm.train()
    assert st.check_zero and st.restore
    for s in range(3):
        st.step_eager(*_batch(g, s))                                      # (raises if a scatter target is not all-zero before the loss backward)
    torch.cuda.synchronize()
    assert float(st.sc_I.abs().max()) == 0.0 and float(st.re_vals.abs().min()) > 0.0


def test_one_evaluation_is_one_round_also_when_it_captures(monkeypatch):
    g, m, tr, st, _ = _step_object(monkeypatch, {"LLMREC_STREAMS": "0"}, mask="items")
    tr.model_mm.eval()
    q = torch.tensor(g.z["eval/users"]).cuda()
    train = m.data_generator.device_state(m.device)["train"]
    before = tr.model_mm.user_feats.clone()
    with torch.no_grad():
        st.eval_topk(q, train, 20, use_graph=True)                       # warm-up (no masking), capture, ONE replay
        torch.cuda.synchronize()
        assert _read(st.mask_step) == 1 and int(st.mask_ticket) == 0
        changed = (tr.model_mm.user_feats != before).any(dim=1).nonzero().reshape(-1).cpu().numpy()
        assert set(changed) <= set(R.nodes(st.U, 24, 7, 0, R.SIDE_USERS).tolist()) and len(changed) > 0
        st.eval_topk(q, train, 20, use_graph=True)
        st.eval_topk(q, train, 20)                                       # eager: a round as well
    torch.cuda.synchronize()
    assert _read(st.mask_step) == 3 and int(st.mask_ticket) == 0


def test_defaults_are_unchanged_and_unsupported_combinations_raise(monkeypatch):
    from llmrec_amd.dp import DataParallelStep
    from llmrec_amd.fused import FusedStep
    env = {"LLMREC_STREAMS": "0"}
    g, m, tr_a, plain, args = _step_object(monkeypatch, env)             # the constructor as every caller wrote it so far
    _, _, tr_b, zero, _ = _step_object(monkeypatch, env, mask_rate=0.0)
    batch = _batch(g, 0)
    for tr, st in ((tr_a, plain), (tr_b, zero)):
        tr.model_mm.train()
        st.step_eager(*batch)
    new = ("mask_step", "mask_ticket", "mask_nodes_u", "mask_nodes_i", "user_sums", "item_sums", "re_vals", "re_rows_u", "re_rows_i", "decoder")
    for st in (plain, zero):
        assert not any(hasattr(st, nm) for nm in new) and st.mask_rate == 0.0 and not st.mask_items and not st.restore
    assert zero.preprop == plain.preprop and zero.entry_point_calls_per_step == plain.entry_point_calls_per_step
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            FusedStep(*args, mask_rate=bad)
    with pytest.raises(ValueError):
        FusedStep(*args, mask_items=True)                                 # --mask at rate 0
    with pytest.raises(RuntimeError, match="empty"):
        FusedStep(*args, mask_rate=0.01, mask_items=True)                 # int(0.96) == 0 users: the reference's NaN
    with pytest.raises(RuntimeError, match="decoder"):
        FusedStep(*args, mask_rate=0.25, mask_items=True, att_re_rate=0.5)
    with pytest.raises(RuntimeError, match="dropout"):
        FusedStep(*args, mask_rate=0.25, drop_rate=0.5)
    with pytest.raises(RuntimeError, match="mask_rate"):
        DataParallelStep(*args, rank=0, world=1, mask_rate=0.2)
    monkeypatch.setenv("LLMREC_PREPROPAGATE", "1")
    with pytest.raises(RuntimeError, match="LLMREC_PREPROPAGATE"):
        FusedStep(*args, mask_rate=0.25, mask_items=True)
    FusedStep(*args, mask_rate=0.25)                                      # user-side masking keeps the pre-propagated operands
    monkeypatch.delenv("LLMREC_PREPROPAGATE")
    # the drop-in: the switch alone changes nothing at rate 0 without --mask, and --mask without it leaves the fused step
    _, _, tr = _trainer(monkeypatch, {"LLMREC_STREAMS": "0", "LLMREC_FUSED": "mask"}, [], seed=3)
    fused = tr._fused_step()
    assert isinstance(fused, FusedStep) and fused.mask_rate == 0.0 and fused.preprop == plain.preprop and not hasattr(fused, "mask_step")
    tr.model_mm.train()
    fused.step_eager(*batch)
    assert fused.entry_point_calls_per_step == plain.entry_point_calls_per_step
    for env_ in ({"LLMREC_STREAMS": "0"}, {"LLMREC_STREAMS": "0", "LLMREC_FUSED": "1"}, {"LLMREC_STREAMS": "0", "LLMREC_FUSED": "wide"}):
        _, _, tr = _trainer(monkeypatch, env_, MASK_ARGV, seed=3)
        assert tr._fused_step() is False
        _, _, tr = _trainer(monkeypatch, env_, USER_ARGV, seed=3)
        assert tr._fused_step() is False
    _, _, tr = _trainer(monkeypatch, {"LLMREC_FUSED": "mask"}, MASK_ARGV + ["--drop_rate", "0.5"], seed=3)
    assert tr._fused_step() is False
