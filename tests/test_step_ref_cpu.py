"""CPU: the yardstick of tests/test_gpu_step_rows.py (tests/_step_ref.py) is neither blind nor too tight, and the inputs of its cases A
and B - the same datasets, seeds and batches - satisfy the conditions the comparison rests on. Nothing here touches a device: the
"steps" are the fp32 oracle's own three-step trajectory (oracle.AdamW between them), each evaluated in fp32 and in fp64 from the same
fp32 parameters.

  inputs      the fp64 maxi values on either side of every prune cut are at least TWICE the 64 fp32-errors apart that the GPU test
              requires; case B's island batch leaves >= 50 % of the rows of both tables' gradients exactly zero and >= 10 % non-zero and
              has the duplicate structure it promises; in case A at least half of the user-table gradient's non-zero rows lie below 1e-8
              of the tensor's maximum - what a whole-tensor norm cannot see.
  not tight   a second fp32 evaluation in another summation order - the same step with users and items renamed by random permutations,
              renamed back - passes every row and scalar check at M = 4.
  not blind   twelve planted faults, each flagged at M = 256 (the largest margin the GPU test may use) in the right tensor and row, and
              nothing else flagged.
  the modes   the same three statements for the opt-in modes of tests/test_gpu_step_rows_modes.py - D (dropout), K / K_MSE (masking with
              restoration), U (user masking) -, whose triples are chosen per step from the trajectory's own parameters under that step's
              masks or features: cut gaps twice the requirement in all three steps; K's item lists >= 50 % outside and >= 10 % inside the
              batch's block; another summation order (masks and lists renamed with the rows) passes at 4; the restoration term's value
              and gradient equal tests/_mask_ref.restore's float64 numpy statement; eight planted faults, each flagged at the GPU test's
              margins - a mask node's restoration gradient lost, a row of the previous list still present, the user term not detached,
              att_re_rate missing from the loss, no mask on the backward, the backward's mask of step s + 1, one keep bit flipped, the
              attribute slices' masks shifted by one slice."""
import copy

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import _rowops_ref as RR
from tests import _step_ref as S
from tests._dropin import load_dropin

CASES = {"A": S.CASE_A, "B": S.CASE_B, "D": S.CASE_D, "K": S.CASE_K, "K_MSE": S.CASE_K_MSE, "U": S.CASE_U}
MODES = ["D", "K", "K_MSE", "U"]


def _trajectory(name, root):
    """ONE thread: the fp32 oracle's dense products then sum in one order whatever the machine's core count. It matters because the steps
    are chained through Adam, whose first updates turn a last-bit difference of a gradient into an lr-sized step: case A's smallest gap
    at step 1 moved between 1.7 and 3.0 x the requirement with the thread count alone. (The GPU test restarts the oracle from the
    device's parameters at every step, and the device's steps are bitwise reproducible.)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _trajectory_one_thread(name, root)
    finally:
        torch.set_num_threads(threads)


def _trajectory_one_thread(name, root):
    case = CASES[name]
    S.write_case(case, root)
    m = load_dropin(S.case_argv(case, root))
    m.set_seed(m.args.seed)
    tr = m.Trainer(data_config={})
    tr.logger.logging = lambda s: None
    data, cfg, graphs = S.oracle_inputs(case, root, m.args)
    sd = tr.model_mm.state_dict()
    params = {k: sd[k].detach().cpu().clone() for k in S.PARAMS}
    opt = O.AdamW(params, lr=cfg.lr)
    exist = list(m.data_generator.exist_users)
    steps = []
    mode = case.get("mode")
    per_step = S.mode_forwards(case, data, cfg, m.args) if mode else None
    islands = S.island_batches(case, data, graphs, cfg, params) if name != "A" and not mode else None
    if mode == "mask":                                                             # the rounds the steps run under (an evaluation is a round too)
        rounds = S.mask_rounds(case)
        m_items = int(m.args.mask_rate * data.n_items) if m.args.mask else 0
        after = S.masked_features(data.feats, cfg.keys, m.args.seed, int(m.args.mask_rate * data.n_users), m_items, rounds[-1] + 1)
    for s in range(S.STEPS):
        if mode:                                                                   # chosen from the step's own pre-step parameters
            batch = S.island_batches(case, data, graphs, cfg, params, per_step=per_step, only=s)[0]
        else:
            batch = S.sampled_batch(data, exist, m.args.seed, cfg.batch_size, cfg.aug_sample_rate, s) if name == "A" else islands[s]
        pre = {k: v.clone() for k, v in params.items()}
        pre_mv = {k: (opt.m[k].clone(), opt.v[k].clone()) for k in params}
        feats, kw, nodes = data.feats, {}, None
        if mode == "drop":
            kw["drop"] = per_step(s)[1]
        elif mode == "mask":
            feats, u_nodes, i_nodes = after[rounds[s]]
            nodes = dict(u=u_nodes, i=i_nodes, prev_i=after[rounds[s] - 1][2] if rounds[s] else None)
            if m.args.mask and m.args.att_re_rate != 0:
                kw["restore"] = S.restoration_of(m, tr, cfg.keys, u_nodes, i_nodes)
        r64 = S.oracle_step(pre, feats, graphs, batch, cfg, torch.float64, **kw)
        r32 = S.oracle_step(pre, feats, graphs, batch, cfg, torch.float32, **kw)
        opt.step({k: torch.from_numpy(r32["grad"][k]).float() for k in params})
        steps.append(dict(batch=batch, pre=pre, pre_mv=pre_mv, r64=r64, r32=r32, feats=feats, kw=kw, nodes=nodes))
    return dict(case=case, data=data, cfg=cfg, graphs=graphs, steps=steps, args=m.args)


@pytest.fixture(scope="module")
def traj(tmp_path_factory):
    made = {}

    def get(name):
        if name not in made:
            made[name] = _trajectory(name, str(tmp_path_factory.mktemp("step_ref_" + name)))
        return made[name]
    return get


def _nonzero_share(x):
    return float((np.abs(x).max(axis=1) > 0).mean())


@pytest.mark.parametrize("name", ["A", "B"] + MODES)
def test_cut_gaps_are_twice_the_required_distance(traj, name):
    t = traj(name)
    for s, st in enumerate(t["steps"]):
        gaps = S.cut_gaps(st["r64"], st["r32"])
        print("[step rows] case %s step %d: cut gap / (64 err) per problem: %s" % (name, s, " ".join("%.3g" % g[2] for g in gaps)))
        assert len(gaps) == S.N_PROB and 0 < st["r64"]["keep"] < len(st["batch"][0])
        assert all(g[2] >= 2.0 for g in gaps), (name, s, gaps)


def test_case_a_user_gradient_hides_most_of_its_rows_from_a_tensor_norm(traj):
    t = traj("A")
    for st in t["steps"]:
        g = st["r64"]["grad"][S.USER_TABLE]
        rows = np.abs(g).max(axis=1)
        live = rows[rows > 0]
        assert live.size == np.unique(st["batch"][0]).size                        # exactly the batch's rows
        small = float((live < 1e-8 * rows.max()).mean())
        print("[step rows] case A: %d non-zero rows, %.0f %% below 1e-8 of the tensor's maximum, median row max / tensor max %.2e"
              % (live.size, 100 * small, float(np.median(live) / rows.max())))
        assert small >= 0.5


def test_case_b_batch_and_zero_rows(traj):
    t = traj("B")
    case, R = t["case"], t["data"].train_mat.tocsr()
    C = case["n_communities"]
    cap = t["cfg"].batch_size + int(t["cfg"].batch_size * t["cfg"].aug_sample_rate)
    for st in t["steps"]:
        users, pos, neg = st["batch"]
        assert len(users) < cap                                                   # n_valid < b_max
        assert (users % C == 0).all()                                             # one block
        assert np.bincount(users).max() >= 8
        assert np.intersect1d(pos, neg).size >= 1
        assert len({(u, p, n) for u, p, n in zip(users.tolist(), pos.tolist(), neg.tolist())}) == len(users)
        for name in S.TABLES:
            share = _nonzero_share(st["r64"]["grad"][name])
            print("[step rows] case B: %s gradient: %.1f %% non-zero rows" % (name, 100 * share))
            assert 0.10 <= share <= 0.50, (name, share)


@pytest.mark.parametrize("name", ["A", "B"] + MODES)
def test_another_summation_order_passes_at_four(traj, name):
    t = traj(name)
    worst = {}
    for s, st in enumerate(t["steps"]):
        p2, f2, R2, b2, back = S.relabel(st["pre"], st["feats"], t["data"].train_mat, st["batch"], seed=100 + s)
        d2, r2 = S.relabel_modes(back, st["kw"].get("drop"), st["kw"].get("restore"))
        got = back(S.oracle_step(p2, f2, R2, b2, t["cfg"], torch.float32, drop=d2, restore=r2))
        fails, ratios = S.compare_step(got, st["r64"], st["r32"], dict(forward=4, table=4, linear=4, scalar=4))
        for k, v in ratios.items():
            worst[S.family_of_key(k)] = max(worst.get(S.family_of_key(k), 0.0), v)
        assert not fails, (name, s, fails[:5])
        assert any(not np.array_equal(got["grad"][k], st["r32"]["grad"][k]) for k in S.PARAMS)       # it IS another order
    print("[step rows] case %s: relabelled fp32 oracle, worst ratio per family: %s" % (name, {k: "%.3g" % v for k, v in sorted(worst.items())}))


# ------------------------------------------------------------------------------------------------------------------------------------
# planted faults
# ------------------------------------------------------------------------------------------------------------------------------------
M_CAP = dict(forward=S.M_MAX, table=S.M_MAX, linear=S.M_MAX, scalar=S.M_MAX)


def _flagged(got, st):
    """{(key, where)} of everything compare_step's checks flag at the cap"""
    out = set()
    for kind in ("fwd", "grad"):
        for name in st["r64"][kind]:
            res = S.row_check(got[kind][name], st["r64"][kind][name], st["r32"][kind][name], S.M_MAX, name)
            out |= {(kind + "/" + name, "%s%d" % b) for b in res.bad}
    for p in range(S.N_PROB):
        for j, part in enumerate(("mf", "emb")):
            if not S.scalar_check(got["bpr"][p][j], st["r64"]["bpr"][p][j], st["r32"]["bpr"][p][j], S.M_MAX)[0]:
                out.add(("bpr%d/%s" % (p, part), ""))
    if not S.scalar_check(got["loss"], st["r64"]["loss"], st["r32"]["loss"], S.M_MAX)[0]:
        out.add(("loss", ""))
    fails, _ = S.compare_step(got, st["r64"], st["r32"], M_CAP)
    assert bool(fails) == bool(out)                                                # compare_step reports what the single checks find
    return out


def _user_rows(st):
    """(a kept batch row, a pruned batch row of the 1e-13 kind, an unreached row) of the user table's gradient"""
    g = np.abs(st["r64"]["grad"][S.USER_TABLE]).max(axis=1)
    users = st["batch"][0]
    kept = S.kept_sets(st["r64"]["maxi"], st["r64"]["keep"])
    any_kept = np.zeros(len(g), dtype=bool)
    for k in kept:
        any_kept[users[k]] = True
    in_batch = np.zeros(len(g), dtype=bool)
    in_batch[users] = True
    kept_row = int(np.flatnonzero(in_batch & (g > 1e-4 * g.max()))[0])
    pruned_row = int(np.flatnonzero(in_batch & ~any_kept & (g > 0) & (g < 1e-8 * g.max()))[0])
    idle_row = int(np.flatnonzero(~in_batch)[0])
    assert any_kept[kept_row] and g[idle_row] == 0
    return kept_row, pruned_row, idle_row


FAULTS = ["kept_row_zero", "pruned_row_zero", "row_doubled", "row_of_previous_step", "unreached_row_1e-30", "item_row_scaled",
          "linear_element", "att_i_row_of_another_key", "emb_scaled"]


@pytest.mark.parametrize("fault", FAULTS)
def test_planted_fault_is_flagged_alone(traj, fault):
    t = traj("A")
    st, prev = t["steps"][1], t["steps"][0]
    got = copy.deepcopy({k: st["r32"][k] for k in ("fwd", "grad", "bpr", "loss")})
    assert not _flagged(got, st) if fault == FAULTS[0] else True                   # the fp32 oracle itself is clean
    kept_row, pruned_row, idle_row = _user_rows(st)
    gu, gi, keys = got["grad"][S.USER_TABLE], got["grad"][S.ITEM_TABLE], t["cfg"].keys
    if fault == "kept_row_zero":
        gu[kept_row] = 0.0
        want = {("grad/" + S.USER_TABLE, str(kept_row))}
    elif fault == "pruned_row_zero":
        assert 0 < np.abs(gu[pruned_row]).max() < 1e-8 * np.abs(gu).max()
        gu[pruned_row] = 0.0
        want = {("grad/" + S.USER_TABLE, str(pruned_row))}
    elif fault == "row_doubled":
        gu[pruned_row] *= 2.0
        want = {("grad/" + S.USER_TABLE, str(pruned_row))}
    elif fault == "row_of_previous_step":
        both = np.intersect1d(st["batch"][0], prev["batch"][0])
        row = int(both[0]) if both.size else kept_row                              # a row both steps wrote, else a row the previous one left zero
        gu[row] = prev["r32"]["grad"][S.USER_TABLE][row]
        want = {("grad/" + S.USER_TABLE, str(row))}
    elif fault == "unreached_row_1e-30":
        gu[idle_row] = 1e-30
        want = {("grad/" + S.USER_TABLE, str(idle_row))}
    elif fault == "item_row_scaled":
        row = int(st["batch"][1][0])
        gi[row] *= 1.0 + 1e-3
        want = {("grad/" + S.ITEM_TABLE, str(row))}
    elif fault == "linear_element":
        w = got["grad"]["item_trans.weight"]
        r, c = 5, 17
        w[r, c] += 1e-3 * np.abs(st["r64"]["grad"]["item_trans.weight"][r]).max()
        flagged = _flagged(got, st)
        assert ("grad/item_trans.weight", str(r)) in flagged
        assert flagged <= {("grad/item_trans.weight", str(r)), ("grad/item_trans.weight", "T%d" % c)}, flagged
        return
    elif fault == "att_i_row_of_another_key":
        row = int(st["batch"][1][3])
        got["fwd"]["att_i/" + keys[1]][row] = st["r32"]["fwd"]["att_i/" + keys[2]][row]
        want = {("fwd/att_i/" + keys[1], str(row))}
    else:
        got["bpr"][4][1] *= 1.0 + 1e-4
        want = {("bpr4/emb", "")}
    assert _flagged(got, st) == want


@pytest.mark.parametrize("fault", ["row_not_updated", "row_updated_twice", "v_not_decayed"])
def test_planted_adamw_fault_is_flagged_alone(traj, fault):
    """The device is played by the reference's own values rounded to fp32 (a correctly rounded kernel), on the item table at step 2 -
    every row has a gradient and non-zero moments there."""
    t = traj("A")
    st, lr, name, f32 = t["steps"][1], t["cfg"].lr, S.ITEM_TABLE, np.float32
    p0, (m0, v0), g = st["pre"][name].numpy(), tuple(x.numpy() for x in st["pre_mv"][name]), st["r32"]["grad"][name].astype(f32)
    assert (np.abs(v0).max(axis=1) > 0).all()
    state = RR.adamw_state(2, lr, S.ADAM["b1"], S.ADAM["b2"])
    step = lambda p, m, v: {k: x[0].astype(f32).reshape(p0.shape) for k, x in RR.adamw(p.reshape(-1), g.reshape(-1), m.reshape(-1), v.reshape(-1),
                                                                                      state, lr=lr, **S.ADAM).items()}
    one = step(p0, m0, v0)
    post = [one["p"].copy(), one["m"].copy(), one["v"].copy()]
    bad, worst = S.adamw_check(name, (p0, m0, v0), g, post, 2, lr)
    assert not bad and max(worst.values()) <= 0.5, worst                           # a correctly rounded update sits inside the bound
    row, d = 123, p0.shape[1]
    if fault == "row_not_updated":
        post[0][row] = p0[row]
        tensors = {"p/" + name}
    elif fault == "row_updated_twice":
        two = step(one["p"], one["m"], one["v"])
        for k, x in enumerate(("p", "m", "v")):
            post[k][row] = two[x][row]
        tensors = {"p/" + name, "m/" + name, "v/" + name}
    else:
        post[2][row] = (v0[row].astype(np.float64) + (1.0 - float(f32(S.ADAM["b2"]))) * g[row].astype(np.float64) ** 2).astype(f32)
        tensors = {"v/" + name}
    bad, _ = S.adamw_check(name, (p0, m0, v0), g, post, 2, lr)
    assert bad and {b[0] for b in bad} == tensors and {b[1] // d for b in bad} == {row}, bad[:4]


def test_scaled_source_widens_by_one_rounding_only(traj):
    """adamw_check(scaled_source=True): the same values, bounds no smaller than the plain ones and larger by less than a factor of two"""
    t = traj("A")
    st, lr, name, f32 = t["steps"][1], t["cfg"].lr, S.USER_TABLE, np.float32
    p0, (m0, v0), g = st["pre"][name].numpy().reshape(-1), tuple(x.numpy().reshape(-1) for x in st["pre_mv"][name]), st["r32"]["grad"][name].astype(f32).reshape(-1)
    state = RR.adamw_state(2, lr, S.ADAM["b1"], S.ADAM["b2"])
    plain = RR.adamw(p0, g, m0, v0, state, lr=lr, **S.ADAM)
    wide = RR.adamw(p0, g * f32(2), m0, v0, state, lr=lr, g_scale=0.5, **S.ADAM)
    for k in ("p", "m", "v"):
        assert np.array_equal(plain[k][0], wide[k][0])
        assert (wide[k][1] >= plain[k][1]).all() and (wide[k][1] <= 2 * plain[k][1]).all()
    assert (wide["m"][1] > plain["m"][1])[g != 0].all()


# ------------------------------------------------------------------------------------------------------------------------------------
# the opt-in modes: dropout (D), masking with restoration (K, K_MSE), user masking alone (U)
# ------------------------------------------------------------------------------------------------------------------------------------
def _block_items(t):
    R, C = t["data"].train_mat.tocsr(), t["case"]["n_communities"]
    return np.unique(R[np.flatnonzero(np.arange(R.shape[0]) % C == 0)].indices)


@pytest.mark.parametrize("name", ["K", "K_MSE"])
def test_case_k_lists_lie_mostly_outside_the_batch_island(traj, name):
    t = traj(name)
    inside = _block_items(t)
    assert [st["nodes"] is not None for st in t["steps"]] == [True] * S.STEPS and S.mask_rounds(t["case"]) == [0, 1, 3]
    for st in t["steps"]:
        nodes = st["nodes"]["i"]
        assert len(nodes) == 200 and len(st["nodes"]["u"]) == 750 and np.unique(nodes).size == 200
        share = float(np.isin(nodes, inside).mean())
        print("[step rows] case %s: %.1f %% of the item list inside the batch's block" % (name, 100 * share))
        assert share >= 0.10 and 1.0 - share >= 0.50, share
        assert np.isin(st["batch"][1], inside).all() and np.isin(st["batch"][2], inside).all()
        for tab in S.TABLES:                                                      # the restoration reaches no table: B's exact zeros stay
            nz = float((np.abs(st["r64"]["grad"][tab]).max(axis=1) > 0).mean())
            assert 0.10 <= nz <= 0.50, (tab, nz)


@pytest.mark.parametrize("name", ["K", "K_MSE"])
def test_restoration_term_agrees_with_the_numpy_statement(traj, name):
    """value and gradient of every attribute stream (and the user stream's value) against tests/_mask_ref.restore in float64"""
    from tests import _mask_ref as MR
    t = traj(name)
    st, keys = t["steps"][1], t["cfg"].keys
    rs, a = st["kw"]["restore"], t["args"]
    loss_type = "mse" if a.feat_loss_type == "mse" else "sce"
    assert rs.slope == 1.0                                                        # nn.LeakyReLU(True): the identity, as _mask_ref states y = W x + b
    leaves = {k: torch.from_numpy(st["r64"]["fwd"]["att_i/" + k]).clone().requires_grad_(True) for k in keys}
    prof_u = torch.from_numpy(st["r64"]["fwd"]["prof_u"])
    term, vals = rs.term({"prof_u": prof_u, "att_i": leaves}, keys)
    grads = torch.autograd.grad(term, [leaves[k] for k in keys])
    Wu, bu = (x.numpy() for x in rs.net["u"])
    Wi, bi = (x.numpy() for x in rs.net["i"])
    want_u = MR.restore(prof_u.numpy(), rs.user_targets.numpy(), rs.u_nodes.numpy(), Wu, bu, loss_type, a.alpha_l)
    assert abs(float(vals[0].detach()) - want_u["loss"]) <= 1e-12 * abs(want_u["loss"])
    total = want_u["loss"]
    for j, k in enumerate(keys):
        want = MR.restore(leaves[k].detach().numpy(), rs.item_targets[k].numpy(), rs.i_nodes.numpy(), Wi, bi, loss_type, a.alpha_l, scale=a.att_re_rate)
        total += want["loss"]
        assert abs(float(vals[1 + j].detach()) - want["loss"]) <= 1e-12 * abs(want["loss"]) and abs(st["r64"]["re_vals"][1 + j] - want["loss"]) <= 1e-12 * abs(want["loss"])
        g = grads[j].numpy()
        others = np.setdiff1d(np.arange(g.shape[0]), rs.i_nodes.numpy())
        assert not g[others].any()                                                # no row outside the list
        assert np.abs(g[rs.i_nodes.numpy()] - want["grad"]).max() <= 1e-10 * np.abs(want["grad"]).max()
    assert abs(float(term.detach()) - a.att_re_rate * total) <= 1e-12 * abs(total)


def _mode_flagged(got, st, case="K"):
    """the keys compare_step flags at the GPU test's margins for that case"""
    from tests.test_gpu_step_rows_modes import MARGINS
    M = MARGINS[case]
    fails, ratios = S.compare_step(got, st["r64"], st["r32"], M)
    flagged = {k for k, v in ratios.items() if not v <= M[S.family_of_key(k)]}
    assert bool(fails) == bool(flagged)
    return flagged


def _run32(t, st, **kw):
    return S.oracle_step(st["pre"], st["feats"], t["graphs"], st["batch"], t["cfg"], torch.float32, **dict(st["kw"], **kw))


RESTORE_FAULTS = ["node_outside_the_island_lost", "row_of_the_previous_list", "user_term_not_detached", "rate_missing_from_the_loss"]


@pytest.mark.parametrize("name", ["K", "K_MSE"])
@pytest.mark.parametrize("fault", RESTORE_FAULTS)
def test_planted_restoration_fault_is_flagged(traj, name, fault):
    t = traj(name)
    st = t["steps"][1]
    rs, inside = st["kw"]["restore"], _block_items(t)
    assert not _mode_flagged(_run32(t, st), st, name)                             # the fp32 oracle itself is clean
    if fault == "node_outside_the_island_lost":
        lost = int(np.flatnonzero(~np.isin(rs.i_nodes.numpy(), inside))[0])       # (a position of the list)

        class Faulty(S.Restoration):
            def item_rows(self, att, key):
                x = att[self.i_nodes]
                keep = torch.ones(len(self.i_nodes), 1, dtype=x.dtype)
                keep[lost] = 0
                return x * keep + (x * (1 - keep)).detach()
        want = "grad/item_trans.weight"
    elif fault == "row_of_the_previous_list":
        prev = st["nodes"]["prev_i"]
        stale = int(prev[~np.isin(prev, rs.i_nodes.numpy()) & ~np.isin(prev, inside)][0])

        class Faulty(S.Restoration):
            def term(self, fw, keys):
                """(a row the clean-up left in the scatter source: the previous list's gradient of that row joins this step's)"""
                total, vals = S.Restoration.term(self, fw, keys)
                old = S.Restoration(self.u_nodes, prev, dict(self.net, slope=self.slope), self.user_targets, self.item_targets, self.rate, self.crit, self.alpha)
                pos = int(np.flatnonzero(prev == stale)[0])

                def rows(att, key):
                    x = att[old.i_nodes]
                    keep = torch.zeros(len(prev), 1, dtype=x.dtype)
                    keep[pos] = 1
                    return x * keep + (x * (1 - keep)).detach()
                old.item_rows = rows
                extra = old.term(fw, keys)[0]
                return total + (extra - extra.detach()), vals
        want = "grad/item_trans.weight"
    elif fault == "user_term_not_detached":
        class Faulty(S.Restoration):
            def user_rows(self, prof_u):
                return prof_u[self.u_nodes]
        want = "grad/user_trans.weight"
    else:
        got = _run32(t, st)
        got["loss"] = got["loss"] - rs.rate * got["re_vals"].sum() + got["re_vals"].sum()
        assert _mode_flagged(got, st, name) == {"loss"}
        return
    bad = Faulty(rs.u_nodes, rs.i_nodes, dict(rs.net, slope=rs.slope), rs.user_targets, rs.item_targets, rs.rate, rs.crit, rs.alpha)
    flagged = _mode_flagged(_run32(t, st, restore=bad), st, name)
    print("[step rows] case %s, %s: flagged %s" % (name, fault, sorted(flagged)))
    assert want in flagged and all(k.startswith("grad/") for k in flagged), flagged


DROP_FAULTS = ["no_mask_on_the_backward", "backward_mask_of_the_next_step", "one_keep_bit_flipped", "attribute_slices_shifted"]


@pytest.mark.parametrize("fault", DROP_FAULTS)
def test_planted_dropout_fault_is_flagged(traj, fault):
    t = traj("D")
    st = t["steps"][1]
    dr = st["kw"]["drop"]
    assert dr.step == 1 and not _mode_flagged(_run32(t, st), st, "D")
    bad = S.Dropout(dr.p, dr.seed, dr.step, dr.U, dr.I, dr.d, dr.keys)
    if fault == "no_mask_on_the_backward":
        clean = bad.factors
        bad.factors = lambda dtype, backward=False: {k: torch.ones_like(v) for k, v in clean(dtype).items()} if backward else clean(dtype)
        want = {"grad/user_trans.weight", "grad/item_trans.weight", "grad/image_trans.weight", "grad/text_trans.weight"}
    elif fault == "backward_mask_of_the_next_step":
        nxt = S.Dropout(dr.p, dr.seed, dr.step + 1, dr.U, dr.I, dr.d, dr.keys)
        clean = bad.factors
        bad.factors = lambda dtype, backward=False: nxt.factors(dtype) if backward else clean(dtype)
        want = {"grad/user_trans.weight", "grad/item_trans.weight", "grad/image_trans.weight", "grad/text_trans.weight"}
    elif fault == "one_keep_bit_flipped":
        row, col = int(st["batch"][0][0]), 17
        flipped = {k: v.copy() for k, v in dr.keep().items()}
        flipped["user"][row, col] ^= True
        bad.keep = lambda step=None: flipped
        want = {"fwd/P_usr"}
    else:
        n = len(dr.keys)
        bad.slice_of = lambda name: 2 + (dr.keys.index(name[5:]) + 1) % n if name.startswith("attr/") else {"image": 0, "text": 1}[name]
        want = {"fwd/att_u/" + k for k in dr.keys} | {"fwd/att_i/" + k for k in dr.keys}
    flagged = _mode_flagged(_run32(t, st, drop=bad), st, "D")
    print("[step rows] case D, %s: flagged %s" % (fault, sorted(flagged)))
    assert want <= flagged, (want - flagged, flagged)
    if fault in DROP_FAULTS[:2]:                                                  # a backward fault leaves the forward and the values alone
        assert all(k.startswith("grad/") for k in flagged), flagged


def test_dropout_oracle_drops_what_the_restated_mask_drops(traj):
    from tests import _dropout_ref as DR
    t = traj("D")
    for s, st in enumerate(t["steps"]):
        keep = DR.keep_mask(t["data"].n_users, t["cfg"].embed_size, 0.3, t["args"].seed, s, DR.TAG_USER_PROFILE)
        for r in (st["r64"], st["r32"]):
            assert not r["fwd"]["P_usr"][~keep].any() and 0.25 < float((~keep).mean()) < 0.35
        assert float(DR.scale(0.3)) != 1.0 / 0.7                                  # the quotient is not exact in fp32
