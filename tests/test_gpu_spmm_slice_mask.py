"""GPU: the slice-ranged, device-stamped row mask of the weighted product (llmrec_spmm_epilogue_t.x_mask_stamp / mask_from_slice).
Operands: a 300 x 200 graph of ~2 000 edges with empty rows, rows of 1 .. 32 non-zeros and - through a plan with low thresholds - one
row each in the wavefront, block and split buckets; X = [200, 7 x 64], masked from slice 2 on; stamps 1 and 255 (counter 0 and 254).
A single launch, a grouped launch (beside the chain's softmax backward and the profile product) and the launch that hosts the loss values.
  (a) with the inactive rows of the masked slices all-zero, Y equals the unmasked product bit for bit;
  (b) with those rows filled with NaN, Y does not change: they are not read;
  (c) in the in-place form, a -0 sentinel (which the unmasked Y += 0 turns into +0) stays in the masked slices of every unlisted row
      without an active neighbour, and the non-in-place form writes zeros there;
  (d) a refused shape (d = 16), an unweighted companion and any guest but the loss values return LLMREC_EUNSUPPORTED and launch nothing.
  (e) companions the masked instance cannot run - weighted by val, with or without col_scale - are refused too.
The bench's graph (13 187 x 17 366, 55 146 edges) runs the lane-group bucket as pipelines of three tasks, a 20 000 x 3 000 graph as
pipelines of five: the steady state, where the row pointers of task i + 3 are loaded inside the loop."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_spmm_multi import _rand, _single
from tests.test_gpu_spmm_guests import LossesGuest, PlanGuest, _same

DEV = "cuda"
D, S, FROM = 64, 7, 2
T_WAVE, T_BLOCK, SEGMENT = 64, 128, 64          # the small graph's plan: 50 non-zeros -> wavefront, 100 -> block, 190 -> split (3 pieces)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def small(ops):
    """(graph, plan of its transposed-by-user operand iu.bwd with one row per long bucket)"""
    rng = np.random.default_rng(14)
    U, I = 300, 200
    degs = rng.integers(1, 10, size=U)
    for k, dg in enumerate([0, 0, 0, 1, 15, 16, 17, 31, 32, 50, 100, 190]):
        degs[(k * 23 + 3) % U] = dg
    rows = np.repeat(np.arange(U), degs)
    cols = np.concatenate([np.sort(rng.choice(I, size=dg, replace=False)) for dg in degs])
    assert 1800 <= rows.size <= 2200
    g = ops.BipartiteGraph.from_edges(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), U, I)
    a = g.iu.bwd
    pl = ops.SpmmPlan.build(a.rowptr, T_WAVE, T_BLOCK, SEGMENT, colidx=a.colidx)
    assert (pl.n_wave, pl.n_block, pl.n_split, pl.n_seg) == (1, 1, 1, 3) and pl.slot_row is not None
    return g, pl


@pytest.fixture(scope="module")
def headline(ops):
    from llmrec_amd import synth
    U, I = 13187, 17366
    rows, cols = synth.bipartite_edges(U, I, 55146, seed=3)
    g = ops.BipartiteGraph.from_edges(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), U, I)
    return g, g.iu.bwd.plan_for(S * D)[1]


@pytest.fixture(scope="module")
def deep(ops):
    from llmrec_amd import synth
    U, I = 20000, 3000
    rows, cols = synth.bipartite_edges(U, I, 80000, seed=11)
    g = ops.BipartiteGraph.from_edges(torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV), U, I)
    return g, g.iu.bwd.plan_for(S * D)[1]


def _problem(ops, a, pl, X, Y, epi, sw):
    d = X.shape[1]
    partials = torch.empty(max(pl.n_seg, 1) * d, dtype=torch.float32, device=DEV)
    rp, ci = pl.csr_of(a)
    pc = pl.c_struct()
    pr = ops.SpmmProblemC(a.n_rows, a.n_cols, rp.data_ptr(), ci.data_ptr(), ops._ptr(a.val), ops._ptr(a.row_scale), ops._ptr(a.col_scale),
                          X.data_ptr(), ops._ld(X), Y.data_ptr(), ops._ld(Y), d, sw, ctypes.addressof(pc), partials.data_ptr(),
                          ctypes.addressof(epi) if epi is not None else None)
    return pr, (pc, epi, partials, rp, ci)


class World:
    """The operands of one case: flags with `stamp` at the active items, X with the promised zeros (and its NaN twin), the rows of A
    without an active neighbour."""

    def __init__(self, ops, g, pl, stamp, seed):
        rng = np.random.default_rng(seed)
        self.ops, self.g, self.pl, self.a = ops, g, pl, g.iu.bwd
        U, I = g.n_users, g.n_items
        active = rng.random(I) < 0.13
        other = rng.integers(0, 256, size=I)
        other[other == stamp] = 0                                                   # stale stamps of earlier steps, and never-stamped rows
        self.flags = torch.tensor(np.where(active, stamp, other).astype(np.uint8), device=DEV)
        self.counter = torch.tensor([stamp - 1 + 255 * 3], dtype=torch.int32, device=DEV)      # LLMREC_ROW_STAMP(counter) == stamp
        idle = torch.tensor(~active, device=DEV)
        self.X = _rand(rng, I, S * D)
        self.X[idle, FROM * D:] = 0.0
        self.X_nan = self.X.clone()
        self.X_nan[idle, FROM * D:] = float("nan")
        self.Y0 = _rand(rng, U, S * D)
        rp, ci = self.a.rowptr.cpu().numpy(), self.a.colidx.cpu().numpy()
        deg = rp[1:] - rp[:-1]
        has_active = np.array([active[ci[rp[r]:rp[r + 1]]].any() for r in range(U)])
        self.quiet = torch.tensor(~has_active & (deg <= 32), device=DEV)            # unlisted rows (lane-group bucket) without an active neighbour
        assert int(self.quiet.sum()) > 0 and bool((deg[self.quiet.cpu().numpy()] > 0).any()) and has_active.any()

    def epi(self, Y, masked, in_place=True):
        m = dict(x_row_mask=self.flags, x_mask_stamp=self.counter, mask_from_slice=FROM) if masked else {}
        return self.ops.spmm_epilogue(self.ops.EPI_NONE, 1.0, Y, **m) if in_place else self.ops.spmm_epilogue(self.ops.EPI_NONE, **m)

    def side(self, X, Y, masked, in_place=True):
        return _problem(self.ops, self.a, self.pl, X, Y, self.epi(Y, masked, in_place), D)

    def companions(self, rng):
        """the other two members of the backward's first group: [(a, X, Y0, epilogue of Y)]"""
        g, ops = self.g, self.ops
        U, I = g.n_users, g.n_items
        Z, Sm = _rand(rng, U, D), torch.softmax(_rand(rng, U, D), dim=-1)
        return [(g.iu.bwd, _rand(rng, I, D), torch.zeros(U, D, device=DEV), lambda Y: ops.spmm_epilogue(ops.EPI_SOFTMAX_BWD, 1 / 3, Z, Sm)),
                (g.ui.bwd, _rand(rng, U, D), _rand(rng, I, D), lambda Y: ops.spmm_epilogue(ops.EPI_NONE, 1.0, Y))]


def _launch(ops, w, X, masked, mode, comp, guest=None, in_place=True, Y0=None):
    """One run from fresh outputs -> ([Y of the side product, the companions' Ys], the guest's state or None)."""
    Y = (w.Y0 if Y0 is None else Y0).clone()
    probs, keep, outs = [], [], [Y]
    pr, k = w.side(X, Y, masked, in_place)
    probs.append(pr); keep.append(k)
    if mode != "single":
        for a, Xc, Yc0, epi_of in comp:
            Yc = Yc0.clone()
            pr, k = _problem(ops, a, a.plan_for(D, whole_row=epi_of(Yc).op != ops.EPI_NONE)[1], Xc, Yc, epi_of(Yc), 0)
            probs.append(pr); keep.append(k); outs.append(Yc)
    state = guest.state() if guest is not None else None
    if not masked:                                                       # the reference: today's separate calls
        if guest is not None:
            guest.alone(state)
        for pr in probs:
            _single(ops, pr)
    elif mode == "single":
        _single(ops, probs[0])
    elif mode == "grouped":
        assert ops.spmm_multi(probs), "the grouped masked launch was refused"
    else:
        assert ops.spmm_multi_guest(probs, guest.guest(state)), "the masked guest launch was refused"
    torch.cuda.synchronize()
    return outs, state


def _bits_equal(want, got, what):
    for i, (x, y) in enumerate(zip(want, got)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, i)


@pytest.mark.parametrize("stamp", [1, 255])
@pytest.mark.parametrize("mode", ["single", "grouped", "guest"])
def test_masked_product_equals_the_unmasked_one_and_reads_no_idle_row(ops, small, mode, stamp):
    g, pl = small
    w = World(ops, g, pl, stamp, seed=100 + stamp)
    rng = np.random.default_rng(7 + stamp)
    comp = w.companions(rng)
    guest = LossesGuest(ops, 257, True) if mode == "guest" else None
    want, s_want = _launch(ops, w, w.X, False, mode, comp, guest)
    got, s_got = _launch(ops, w, w.X, True, mode, comp, guest)                      # (a)
    _bits_equal(want, got, "zeros")
    got_nan, _ = _launch(ops, w, w.X_nan, True, mode, comp, guest)                  # (b)
    _bits_equal(want, got_nan, "NaN in the idle rows")
    if guest is not None:
        for k in s_want:
            assert _same(s_want[k], s_got[k]), k
        guest.check(s_got)
    # (c) in place: the -0 sentinel survives in the masked slices of the quiet rows (Y += 0 would store +0); everything else as unmasked
    Y0 = w.Y0.clone()
    Y0[w.quiet, FROM * D:] = -0.0
    want_c, _ = _launch(ops, w, w.X, False, mode, comp, guest, Y0=Y0)
    got_c, _ = _launch(ops, w, w.X_nan, True, mode, comp, guest, Y0=Y0)
    kept = got_c[0][w.quiet, FROM * D:].view(torch.int32)
    assert bool((kept == -2 ** 31).all()), "a quiet row was rewritten"
    assert bool((want_c[0][w.quiet, FROM * D:].view(torch.int32) == 0).all())       # (the sentinel does tell the two apart)
    assert torch.equal(want_c[0], got_c[0])                                         # -0 == +0; every other element has the same value
    loud = ~w.quiet
    assert torch.equal(want_c[0][loud].view(torch.int32), got_c[0][loud].view(torch.int32))
    assert torch.equal(want_c[0][:, :FROM * D].view(torch.int32), got_c[0][:, :FROM * D].view(torch.int32))
    # not in place (Y = A X): the quiet rows are written, as zeros
    want_n, _ = _launch(ops, w, w.X, False, mode, comp, guest, in_place=False)
    got_n, _ = _launch(ops, w, w.X_nan, True, mode, comp, guest, in_place=False)
    _bits_equal(want_n, got_n, "not in place")
    assert bool((got_n[0][w.quiet, FROM * D:] == 0).all())


@pytest.mark.parametrize("which", ["bench_graph", "steady_state"])
def test_pipelined_lane_groups(ops, headline, deep, which):
    g, pl = headline if which == "bench_graph" else deep
    # tasks per lane group = ceil(tasks / 32 768): three at the bench graph (prologue and drain only), five at the other one - from the
    # fourth task on the loop itself loads the row pointers of task i + 3 and rotates them through the stages
    assert pl.n_short * S > (2 if which == "bench_graph" else 4) * 32 * 1024
    w = World(ops, g, pl, 77, seed=5)
    want, _ = _launch(ops, w, w.X, False, "single", None)
    got, _ = _launch(ops, w, w.X, True, "single", None)
    _bits_equal(want, got, "zeros")
    Y0 = w.Y0.clone()
    Y0[w.quiet, FROM * D:] = -0.0
    got_c, _ = _launch(ops, w, w.X_nan, True, "single", None, Y0=Y0)
    assert bool((got_c[0][w.quiet, FROM * D:].view(torch.int32) == -2 ** 31).all())
    loud = ~w.quiet
    assert torch.equal(want[0][loud].view(torch.int32), got_c[0][loud].view(torch.int32))
    assert torch.equal(want[0][:, :FROM * D].view(torch.int32), got_c[0][:, :FROM * D].view(torch.int32))


def test_refused_shapes_and_companies_launch_nothing(ops, small):
    from llmrec_amd import _lib
    g, pl = small
    w = World(ops, g, pl, 9, seed=3)
    rng = np.random.default_rng(2)
    U, I = g.n_users, g.n_items
    # d = 16: another kernel family
    X16, Y16 = _rand(rng, I, 16), torch.full((U, 16), 7.0, device=DEV)
    epi = ops.spmm_epilogue(ops.EPI_NONE, 1.0, Y16, x_row_mask=w.flags, x_mask_stamp=w.counter, mask_from_slice=0)
    pr, keep = _problem(ops, w.a, w.a.plan_for(16)[1], X16, Y16, epi, 0)
    ok = _lib.call_unless_unsupported("llmrec_spmm_f32", pr.n_rows, pr.n_cols, pr.rowptr, pr.colidx, pr.val, pr.row_scale, pr.col_scale, pr.X,
                                      pr.ldx, pr.Y, pr.ldy, pr.d, pr.slice_width, pr.plan, pr.partials, pr.epilogue, ops._stream())
    assert not ok
    # an unweighted companion; a guest other than the loss values
    Y, Yf = torch.full((U, S * D), 7.0, device=DEV), torch.full((U, D), 7.0, device=DEV)
    side, k0 = w.side(w.X_nan, Y, True)
    a = g.ui.fwd
    plain, k1 = _problem(ops, a, a.plan_for(D)[1], _rand(rng, I, D), Yf, None, 0)
    assert not ops.spmm_multi([side, plain])
    # (e) companions weighted by val: the masked instance forms its weights from col_scale alone
    a0 = g.iu.bwd
    Yv = [torch.full((U, D), 7.0, device=DEV) for _ in range(2)]
    val = _rand(rng, a0.nnz).abs() + 0.5
    keep_v, lg = [], LossesGuest(ops, 257, False)
    ls = lg.state()
    for Yq, cs in zip(Yv, (None, a0.col_scale)):
        av = ops.Csr(a0.n_rows, a0.n_cols, a0.rowptr, a0.colidx, val, None, cs)
        comp, kq = _problem(ops, av, av.plan_for(D)[1], _rand(rng, I, D), Yq, ops.spmm_epilogue(ops.EPI_NONE, 1.0, Yq), 0)
        keep_v.append((av, kq))
        assert not ops.spmm_multi([side, comp])
        assert not ops.spmm_multi_guest([side, comp], lg.guest(ls))
    guest = PlanGuest(ops, g, 257, False)
    s = guest.state()
    before = {k: v.clone() for k, v in s.items()}
    assert not ops.spmm_multi_guest([side], guest.guest(s))
    torch.cuda.synchronize()
    assert bool((Y16 == 7.0).all()) and bool((Y == 7.0).all()) and bool((Yf == 7.0).all()) and all(bool((y == 7.0).all()) for y in Yv)
    for k in s:
        assert _same(before[k], s[k]), k
