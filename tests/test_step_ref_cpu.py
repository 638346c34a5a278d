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
              nothing else flagged."""
import copy

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import _rowops_ref as RR
from tests import _step_ref as S
from tests._dropin import load_dropin

CASES = {"A": S.CASE_A, "B": S.CASE_B}


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
    islands = S.island_batches(case, data, graphs, cfg, params) if name != "A" else None
    for s in range(S.STEPS):
        batch = S.sampled_batch(data, exist, m.args.seed, cfg.batch_size, cfg.aug_sample_rate, s) if name == "A" else islands[s]
        pre = {k: v.clone() for k, v in params.items()}
        pre_mv = {k: (opt.m[k].clone(), opt.v[k].clone()) for k in params}
        r64 = S.oracle_step(pre, data.feats, graphs, batch, cfg, torch.float64)
        r32 = S.oracle_step(pre, data.feats, graphs, batch, cfg, torch.float32)
        opt.step({k: torch.from_numpy(r32["grad"][k]).float() for k in params})
        steps.append(dict(batch=batch, pre=pre, pre_mv=pre_mv, r64=r64, r32=r32))
    return dict(case=case, data=data, cfg=cfg, graphs=graphs, steps=steps)


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


@pytest.mark.parametrize("name", ["A", "B"])
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


@pytest.mark.parametrize("name", ["A", "B"])
def test_another_summation_order_passes_at_four(traj, name):
    t = traj(name)
    worst = {}
    for s, st in enumerate(t["steps"]):
        p2, f2, R2, b2, back = S.relabel(st["pre"], t["data"].feats, t["data"].train_mat, st["batch"], seed=100 + s)
        got = back(S.oracle_step(p2, f2, R2, b2, t["cfg"], torch.float32))
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
