"""GPU: whole training steps of the fused step's OPT-IN modes against the float64 oracle, ROW BY ROW - the rig, margins and conditions of
tests/test_gpu_step_rows.py (tests/_step_ref.py; tests/test_step_ref_cpu.py shows on planted faults of each mode that the yardstick is
neither blind nor too tight), on case B's dataset and schedule: 3000 x 800 in four disjoint blocks, widths 48 / 200 / 72, three layers,
408 triples from ONE block with n_valid < b_max.

  D      --drop_rate 0.3 under LLMREC_FUSED_DROPOUT=1 (the fp32 quotient 1 / (1 - p) is inexact) - eager, graph.
  K      --mask True --mask_rate 0.25 --att_re_rate 0.5 under LLMREC_FUSED=mask (sce): 750 user and 200 item nodes per round, about
         72 % of the item list in blocks the batch never reaches - eager, graph, four streams (eager). K_MSE: --feat_loss_type mse, eager.
  U      --mask_rate 0.25 alone (user features only) - eager, graph. On B's shape: tests/_step_ref.py (CASE_U) says why not A's.
In K and U one Trainer.test() runs between the second and the third step: the round counter (0, 1, [2], 3) leaves the step index.

Per step: the device's counter is read and asserted, parameters, moments and (K, U) the feature tensors and their running sums are
snapshot, the step's triples are chosen from the DEVICE's pre-step parameters under the step's restated masks or features
(island_batches(only=s)), the step runs, everything is snapshot again. Then
  the masking round (K, U; also the evaluation's): every feature row outside tests/_mask_ref.nodes(seed, round, side) is bit-identical
      to its pre-round value, every listed row is within RunningBound.stored_mean_bound of the exact column mean of the pre-round tensor
      and equal, bit for bit, to fp32(the running sum the launch read / N); the device's lists are the restated ones;
  the oracle in fp64 and fp32 from the device's pre-step parameters, the device's POST-round features (bit copies) and the restated masks
      or lists: compare_step over every forward output and gradient row, the 17 scalars and (K) the six restoration stream losses;
      adamw_check on every element of the ten parameters and twenty moments;
  D: every element of P_usr the restated mask drops is +0.0 on the device (its kept elements are in compare_step's rows);
  clean-up: the five scatter sources (sc_I with the restoration's rows among them) all-zero, tickets at 0, counters advanced once.
The conditions of tests/test_gpu_step_rows.py are asserted unchanged at run time - every problem's cut gap >= 64 fp32-oracle errors,
the table gradients' rows >= 50 % exactly zero and >= 10 % non-zero (the restoration reaches no table: its gradient ends in
item_trans) - and in K every step's item list has >= 10 % of its nodes inside the batch's block and >= 50 % outside.

MARGINS: M of tests/test_gpu_step_rows.py (16 / 8 / 16 / 16; the restoration stream losses are scalars of that family), with ONE
mode-specific entry, by that file's rule (measured worst x 4, rounded up to a power of two, at most 256): the table family of D and U is 16.
  Measured: the item table's gradient at 2.02 (D, step 1) and 3.84 (U, step 2) x the yardstick - x 4 = 8.08 and 15.4, above 8. Cause,
  found from the device's saved inputs on the CPU: no row stands out - in those two steps EVERY live row of that tensor is off by the
  same relative amount (U step 2: median row 2.4, 99th percentile 3.2; the other steps' medians 0.2 - 0.9), a common-mode error of the
  chain all rows share (three softmax-closed layers back through six products). Its size depends on the summation order alone: the
  fp32 ORACLE itself, evaluated on U's step-2 inputs under eight random renamings of users and items, gives medians from 0.64 to 4.25
  and a worst row of 6.35, the device 2.6 / 4.2 against the same evaluation; on D's step-1 inputs 0.81 - 1.07 / 1.96, the device
  1.76 / 2.43. The device's absolute error (1.0e-6 and 5e-7 of the row maximum) is that of the other steps; the yardstick's own
  evaluation came out at the low end (4.2e-7 and 2.5e-7, elsewhere 4.8e-7 - 8.4e-7). A legitimate order-of-operations difference.
MEASURED on the MI355X, worst err / yardstick over the three steps (per tensor: profiles/experiments/step_rows.md; the paths of a case
agree to every digit, and share their batches and oracle steps through _memo for that reason):
                                   D (eager = graph)   K (eager = graph = streams)   K-mse    U (eager = graph)
  forward outputs                  2.30 (txt_u)        2.26                          2.26     2.06
  table gradients                  2.02                1.50                          1.50     3.84 (item table)
  Linear gradients                 1.48                2.14                          1.78     2.89 (item_trans.weight)
  scalars (16 BPR values, loss)    1.94                2.57 (bpr7/mf)                1.63     1.58
  restoration stream losses        -                   1.31                          0.66     -
  AdamW, worst |err| / bound       0.49                0.49                          0.48     0.50
  stored means, worst err / bound  -                   0.99                          0.99     0.97   (one fp32 rounding: tight by nature)
  smallest cut gap / (64 err)      191                 258                           384      278
No row failed; library code is unchanged.
"""
import hashlib

import numpy as np
import pytest
import torch

from tests import _dropout_ref as DR
from tests import _mask_ref as MR
from tests import _rowops_ref as RR
from tests import _step_ref as S
from tests.test_gpu_step_rows import M, _forward_of, _np, datasets  # noqa: F401  (datasets: the module fixture that writes the cases once)

pytestmark = pytest.mark.gpu

CASES = {"D": S.CASE_D, "K": S.CASE_K, "K_MSE": S.CASE_K_MSE, "U": S.CASE_U}
DROP = {"LLMREC_FUSED": "1", "LLMREC_FUSED_DROPOUT": "1"}
MASK = {"LLMREC_FUSED": "mask"}
PATHS = {
    ("D", "eager"): dict(DROP, LLMREC_GRAPH="0"),
    ("D", "graph"): dict(DROP, LLMREC_GRAPH="1"),
    ("K", "eager"): dict(MASK, LLMREC_GRAPH="0"),
    ("K", "graph"): dict(MASK, LLMREC_GRAPH="1"),
    ("K", "streams"): dict(MASK, LLMREC_GRAPH="0", LLMREC_STREAMS="1"),
    ("K_MSE", "eager"): dict(MASK, LLMREC_GRAPH="0"),
    ("U", "eager"): dict(MASK, LLMREC_GRAPH="0"),
    ("U", "graph"): dict(MASK, LLMREC_GRAPH="1"),
}
MARGINS = {"D": dict(M, table=16), "K": M, "K_MSE": M, "U": dict(M, table=16)}     # (table: 3.84 x 4 = 15.4 -> 16, module docstring)
assert all(max(v.values()) <= S.M_MAX for v in MARGINS.values())
SCATTER_SOURCES = ("dE_u", "dE_i", "sc_U", "sc_I", "sc_prof")

_MEMO = {}


def _memo(what, arrays, fn):
    """fn() once per content of `arrays`: the paths of a case run bitwise-equal steps, so the batch and both oracle steps of a
    (case, step) are computed once and shared - a path that differs in any bit computes its own."""
    h = hashlib.sha1(repr(what).encode())
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    key = h.hexdigest()
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def _read(counter):
    return int(counter.view(torch.int64).cpu()[0]) & (2 ** 64 - 1)


def _features(tr, keys):
    out = {"user": tr.model_mm.user_feats}
    out.update({"attr/" + k: tr.model_mm.item_feats[k] for k in keys})
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def _sums(step, keys):
    out = {"user": step.user_sums[0]}
    out.update({"attr/" + k: step.item_sums[j] for j, k in enumerate(keys) if step.mask_items})
    return {k: v.detach().cpu().numpy().copy() for k, v in out.items()}


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check_round(tag, step, rnd, seed, pre, post, sums_pre, bounds):
    """One masking round on the device (module docstring) -> (u_nodes, i_nodes) of the round; `bounds` ({name: RunningBound}) moves on."""
    u_nodes = MR.nodes(step.U, step.m_users, seed, rnd, MR.SIDE_USERS)
    i_nodes = MR.nodes(step.I, step.m_items, seed, rnd, MR.SIDE_ITEMS) if step.mask_items else np.zeros(0, dtype=np.int64)
    assert np.array_equal(step.mask_nodes_u.cpu().numpy(), u_nodes), (tag, "user list")
    if step.mask_items:
        assert np.array_equal(step.mask_nodes_i.cpu().numpy(), i_nodes), (tag, "item list")
    worst = 0.0
    for name in pre:
        nodes = u_nodes if name == "user" else i_nodes
        N = pre[name].shape[0]
        others = np.setdiff1d(np.arange(N), nodes)
        assert np.array_equal(_bits(post[name][others]), _bits(pre[name][others])), (tag, name, "a row outside the list moved")
        if not len(nodes):
            continue
        exact = np.asarray(pre[name].astype(np.longdouble).sum(axis=0) / N, dtype=np.float64)          # (the 80-bit sum: 2^-11 of an fp64 one's error)
        bound = bounds[name].stored_mean_bound(N, exact)
        err = np.abs(post[name][nodes].astype(np.float64) - exact)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (tag, name, "stored mean beyond its bound", float((err / bound).max()))
        stored = (sums_pre[name] / np.float64(N)).astype(np.float32)
        assert np.array_equal(_bits(post[name][nodes]), _bits(np.broadcast_to(stored, (len(nodes), stored.size)))), (tag, name, "stored mean is not fp32(sum / N)")
        bounds[name].round(pre[name][nodes], stored, sums_pre[name])
    return u_nodes, i_nodes, worst


@pytest.mark.parametrize("name,path", list(PATHS), ids=["%s-%s" % k for k in PATHS])
def test_three_steps_of_a_mode_row_by_row(datasets, monkeypatch, name, path):
    from llmrec_amd.fused import FusedStep
    from tests._step_env import fused_trainer, snapshot
    case, mode = CASES[name], CASES[name]["mode"]
    root = datasets("B", None)
    b = fused_trainer(monkeypatch, S.case_argv(case, root), PATHS[(name, path)], train=True, step=True)
    m, tr, step = b.m, b.trainer, b.step
    a = m.args
    data, cfg, graphs = datasets.inputs("B", a)
    keys, lr, dev = tuple(cfg.keys), float(a.lr), torch.device("cuda")
    assert lr == 1e-3 and cfg.n_layers == 3 and keys == tuple(data.keys) and len(keys) == 5
    assert isinstance(step, FusedStep) and step.L == 3 and step.gemm == "bf16x3" and not step.wgrad_rows and step.preprop is False
    assert step.multi_stream == (path == "streams")
    restore = False
    if mode == "drop":
        assert step.drop_rate == 0.3 == a.drop_rate and step.drop_seed == a.seed and step.mask_rate == 0.0
    else:
        restore = name != "U"
        assert step.drop_rate == 0.0 and step.mask_rate == 0.25 and step.mask_seed == a.seed and step.m_users == 750
        assert step.mask_items == restore == step.restore and step.m_items == (200 if restore else 0)
        if restore:
            assert not step.bwd_mask and step.feat_loss_type == ("mse" if name == "K_MSE" else "sce") and step.att_re_rate == 0.5
        feats0 = _features(tr, keys)
        for k, v in feats0.items():                                               # the oracle's files are the device's tensors
            assert np.array_equal(_bits(v), _bits(data.feats[k].numpy())), k
        bounds = {k: MR.RunningBound(v) for k, v in feats0.items() if k == "user" or restore}
        rounds = S.mask_rounds(case)
        assert rounds == [0, 1, 3]
        users_to_test = list(m.data_generator.test_set.keys())
    per_step = S.mode_forwards(case, data, cfg, a)
    C = case["n_communities"]
    R = data.train_mat.tocsr()
    inside = np.unique(R[np.flatnonzero(np.arange(R.shape[0]) % C == 0)].indices)
    folded = bool(step.fold)
    fails, worst, worst_adamw, gaps_min, worst_mean = [], {}, {}, np.inf, 0.0
    tag = "[step rows] %s-%s" % (name, path)

    def mask_state():
        return _features(tr, keys), _sums(step, keys)

    for s in range(S.STEPS):
        if mode == "mask" and s == case["eval_before"]:                           # one evaluation = one round (round 2), no step
            assert _read(step.mask_step) == s
            f_pre, sums_pre = mask_state()
            before = snapshot(tr, None, grads=False, cpu=True)
            tr.test(users_to_test, is_val=False)
            torch.cuda.synchronize()
            f_post, _ = mask_state()
            assert _read(step.mask_step) == s + 1 and int(step.mask_ticket) == 0
            _, _, w = _check_round(tag + " evaluation", step, s, a.seed, f_pre, f_post, sums_pre, bounds)
            worst_mean = max(worst_mean, w)
            after = snapshot(tr, None, grads=False, cpu=True)
            assert set(before) == set(after) and all(torch.equal(before[k], after[k]) for k in before)      # it trains nothing
        if mode == "drop":
            assert _read(step.drop_step) == s and int(step.drop_ticket) == 0
        else:
            assert _read(step.mask_step) == rounds[s] and int(step.mask_ticket) == 0
            f_pre, sums_pre = mask_state()
        pre = snapshot(tr, None, grads=False, cpu=True)
        params = {k: pre["p/" + k] for k in S.PARAMS}
        batch = _memo(("batch", name, s), [params[k].numpy() for k in S.PARAMS],
                      lambda: S.island_batches(case, data, graphs, cfg, params, per_step=per_step, only=s)[0])
        assert len(batch[0]) == 408 < step.b_max and (batch[0] % C == 0).all()
        tr.train_step(*(torch.from_numpy(t).to(dev) for t in batch))
        torch.cuda.synchronize()
        assert (step.graph_exec is not None) == (path == "graph")
        if path == "graph":
            assert int(step.static["n_valid"]) == len(batch[0])
        got = {"fwd": _forward_of(step.outputs(), keys), "bpr": _np(step.out[:step.n_prob]).reshape(S.N_PROB, 2), "loss": float(step.scal[1])}
        post = snapshot(tr, None, grads=True, cpu=True)
        got["grad"] = {k: post["g/" + k].numpy().astype(np.float64) for k in S.PARAMS}
        state = tr.optimizer.dev_state.cpu().numpy()
        assert state.view(np.int32).tolist() == RR.adamw_state(s + 1, lr, S.ADAM["b1"], S.ADAM["b2"]).view(np.int32).tolist(), ("AdamW state", s, state)
        # clean-up and counters
        for nm in SCATTER_SOURCES:
            assert float(getattr(step, nm).abs().max()) == 0.0, (tag, s, nm, "not all-zero after the step")
        feats, kw = data.feats, {}
        if mode == "drop":
            assert _read(step.drop_step) == s + 1 and int(step.drop_ticket) == 0
            kw["drop"] = S.Dropout(a.drop_rate, a.seed, s, data.n_users, data.n_items, cfg.embed_size, keys)
            keep = DR.keep_mask(data.n_users, cfg.embed_size, a.drop_rate, a.seed, s, DR.TAG_USER_PROFILE)
            p_usr = step.P_usr.detach().cpu().numpy()
            assert (_bits(p_usr)[~keep] == 0).all(), (tag, s, "a dropped element of P_usr is not +0.0")
            assert np.array_equal(keep, kw["drop"].keep()["user"])
        else:
            assert _read(step.mask_step) == rounds[s] + 1 and int(step.mask_ticket) == 0
            f_post, _ = mask_state()
            u_nodes, i_nodes, w = _check_round("%s step %d" % (tag, s), step, rounds[s], a.seed, f_pre, f_post, sums_pre, bounds)
            worst_mean = max(worst_mean, w)
            feats = dict(data.feats, **{k: torch.from_numpy(v) for k, v in f_post.items()})       # the device's post-round tensors
            if restore:
                share = float(np.isin(i_nodes, inside).mean())
                assert share >= 0.10 and 1.0 - share >= 0.50, (tag, s, "island shares of the item list", share)
                kw["restore"] = S.restoration_of(m, tr, keys, u_nodes, i_nodes)
                got["re_vals"] = _np(step.re_vals)
                assert got["re_vals"].shape == (1 + len(keys),)
        content = [params[k].numpy() for k in S.PARAMS] + [feats[k].numpy() for k in sorted(feats)] + list(batch)
        r64 = _memo(("r64", name, s), content, lambda: S.oracle_step(params, feats, graphs, batch, cfg, torch.float64, **kw))
        r32 = _memo(("r32", name, s), content, lambda: S.oracle_step(params, feats, graphs, batch, cfg, torch.float32, **kw))
        gaps = S.cut_gaps(r64, r32)
        gaps_min = min(gaps_min, min(g[2] for g in gaps))
        assert all(g[2] >= 1.0 for g in gaps), ("cut gap below 64 fp32 errors", name, path, s, gaps)
        for tab in S.TABLES:                                                      # the islands: exact zeros in both tables' gradients
            share = float((np.abs(r64["grad"][tab]).max(axis=1) > 0).mean())
            assert 0.10 < share <= 0.50, (tab, share)
        prov = S.Provenance(data.train_mat, batch, S.kept_sets(r64["maxi"], r64["keep"]))
        f, ratios = S.compare_step(got, r64, r32, MARGINS[name], prov)
        fails += ["step %d: %s" % (s, x) for x in f]
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        for k in S.PARAMS:
            bad, w = S.adamw_check(k, (pre["p/" + k].numpy(), pre["m/" + k].numpy() if "m/" + k in pre else None,
                                       pre["v/" + k].numpy() if "v/" + k in pre else None), post["g/" + k].numpy(),
                                   (post["p/" + k].numpy(), post["m/" + k].numpy(), post["v/" + k].numpy()), s + 1, lr,
                                   scaled_source=(folded and k == S.USER_TABLE))
            d = post["p/" + k].shape[-1]
            fails += ["step %d: AdamW %s element %d (row %d): |err| %.3e > bound %.3e" % (s, what, i, i // d, e, bd) for what, i, e, bd in bad]
            for what, v in w.items():
                worst_adamw[what] = max(worst_adamw.get(what, 0.0), v)
    by_family = {}
    for k, v in worst.items():
        by_family[S.family_of_key(k)] = max(by_family.get(S.family_of_key(k), 0.0), v)
    for k in sorted(worst):
        print("%s ratio %-28s %.3g" % (tag, k, worst[k]))
    print("%s families %s; AdamW worst |err| / bound %s; smallest cut gap / (64 err) %.3g; stored means, worst |err| / bound %.3g"
          % (tag, {k: "%.3g" % v for k, v in sorted(by_family.items())}, {k: "%.3g" % v for k, v in sorted(worst_adamw.items())}, gaps_min, worst_mean))
    assert not fails, "\n".join(fails[:12])
