"""GPU: the SpMM that gathers bf16 rows (llmrec_spmm_xbf16_f32, llmrec_rows_to_bf16: llmrec_amd/csrc/spmm_bf16.hip) and the opt-in bf16
gather mode of the row-sharded step (llmrec_amd/dist_fused.py, gather_dtype = "bf16").

Kernel cases (tests/_spmm_bf16_ref.py: the 100 x 2200 graph of tests/_spmm_ref.py - rows of 0 .. 2100 nnz, every bucket, segment tails of
one nnz - every family at its representative and its full width, the plain and the weighted kernel, the three threshold triples, plain
and permuted plans, every epilogue with and without post_scale at d = 64 and 128). Per case:
  (a) torch.equal with llmrec_spmm_f32 on the widened operand under the same plan - the determinism guarantee;
  (b) every element inside the float64 bound of the helper, which a kernel that gathered fp32 rows breaks in 93 of 94 rows;
  (c) Yb bit-equal to Y.to(torch.bfloat16), split rows (written by the finalize launch) included;
  (d) the guard rows around Y and Yb untouched, the operands unchanged; a refused call writes nothing.
llmrec_rows_to_bf16 is bit-exact against torch's float -> bfloat16, with and without row_scale, through strided views, on both paths.

The step (the 900 x 700 problem of tests/test_gpu_dist_fused.py, restated in the helper): a HipBackend subclass interposes on spmm /
to_bf16 / spmm_rows_compact and checks, for every bf16 product of three steps, that its output is the fp32 kernel's on the widened
shadow, that the shadow is the RNE of its fp32 source at the moment it is gathered, that Yb is the RNE of the output, and counts the
calls (a default two-layer step: 5 bf16 and 3 fp32 products at one chunk). Two fresh runs agree bit for bit on both tables and both
moments; the scatter targets end all-zero; two processes on one GPU keep their replicas bit-identical under both exchanges.

Closeness to the fp32 oracle is gated by a recorded figure: the oracle's own loop, run on the CPU with the gathered operands rounded
where the step rounds them, deviates from the fp32 oracle's losses (about 0.72) by at most 5.5e-6 (d = 64) and 1.26e-5 (d = 128, with
augmented triples) over the three steps - helper STEP_DEVIATION, recomputed by tests/test_spmm_bf16_cpu.py. The step's losses must stay
within FOUR times that figure of the fp32 oracle's (the factor covers the different summation trees of torch's CPU sums and the
kernels). The tables after AdamW are no useful gate: Adam's normalisation hides gradient error."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import _spmm_bf16_ref as B
from tests import _spmm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GR = 3                                 # guard rows on either side of a view
BF16_SENTINEL = 0x4640                 # 12288.0 as bf16 bits: what Yb and its guards hold before a call


class View:
    """rows x d elements at row stride ld inside a larger flat buffer (first element 16-byte aligned for fp32, 8-byte for bf16; ld % 4 == 0)"""

    def __init__(self, rows, d, dtype, fill, values=None):
        ld = (d + 3) // 4 * 4 + 8
        off = GR * ld + 8
        self.buf = torch.full(((rows + 2 * GR) * ld + 16,), fill, dtype=dtype, device=DEV)
        self.v = self.buf.as_strided((rows, d), (ld, 1), off)
        if values is not None:
            self.v.copy_(values)
        self.pristine = self.buf.clone()
        assert self.v.data_ptr() % (4 * self.buf.element_size()) == 0 and ld % 4 == 0

    def _bits(self, t):
        return t.view(torch.int32 if t.element_size() == 4 else torch.int16)

    def unchanged(self):
        return torch.equal(self._bits(self.buf), self._bits(self.pristine))

    def guards_unchanged(self):
        keep = self.v.clone()
        self.v.copy_(self.pristine.as_strided(self.v.shape, self.v.stride(), self.v.storage_offset()))
        ok = self.unchanged()
        self.v.copy_(keep)
        return ok


class Env:
    def __init__(self):
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        from llmrec_amd import ops
        self.ops = ops
        rowptr, colidx, _ = R.graph()
        self.rowptr, self.colidx = torch.from_numpy(np.array(rowptr)).to(DEV), torch.from_numpy(np.array(colidx)).to(DEV)
        self.g = {k: torch.from_numpy(np.array(v)).to(DEV) for k, v in R.graph_inputs().items()}
        self.plans = {}
        for name, triple in R.TRIPLES.items():
            self.plans[(name, False)] = ops.SpmmPlan.build(self.rowptr, *triple)
            self.plans[(name, True)] = ops.SpmmPlan.build(self.rowptr, *triple, colidx=self.colidx, order_rows=True)
            assert self.plans[(name, True)].slot_row is not None and self.plans[(name, False)].n_split > 0
        self.x = {}

    def operand(self, case):
        inp = R.inputs(case)
        rs = self.g["rs"] if case.has_rs else None
        return self.ops.Csr(R.N_ROWS, R.N_COLS, self.rowptr, self.colidx, self.g["val"] if case.has_val else None, rs,
                            self.g["cs"] if case.has_cs else None, {})

    def x_views(self, d):
        """(Xb: the bf16 operand, Xw: the fp32 tensor with the same values), guards NaN"""
        if d not in self.x:
            X = torch.from_numpy(np.array(R.width_inputs(d)[0])).to(DEV)
            Xb = View(R.N_COLS, d, torch.bfloat16, float("nan"), values=X.to(torch.bfloat16))
            Xw = View(R.N_COLS, d, torch.float32, float("nan"), values=Xb.v.float())
            assert np.array_equal(Xw.v.cpu().numpy(), B.rounded_x(d))                     # torch's rounding = the helper's bit formula
            self.x[d] = (Xb, Xw)
        return self.x[d]


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.x.clear()


def _run(env, case, bf16: bool):
    """one call of the case through ops.spmm_bf16 / ops.spmm_raw over fresh outputs; returns (Y view, Yb view or None, the operand views)"""
    ops = env.ops
    inp = R.inputs(case)
    Xb, Xw = env.x_views(case.d)
    a = env.operand(case)
    t = lambda arr: torch.from_numpy(np.array(arr)).to(DEV)
    Y = View(R.N_ROWS, case.d, torch.float32, R.SENTINEL, values=t(inp["Z"]) if case.op == "acc" else None)
    Z = View(R.N_ROWS, case.d, torch.float32, float("nan"), values=t(inp["Z"])) if case.op in ("z", "softmax_bwd") else None
    S = View(R.N_ROWS, case.d, torch.float32, float("nan"), values=t(inp["S"])) if case.op == "softmax_bwd" else None
    Zt = Y if case.op == "acc" else Z
    epi = ops.spmm_epilogue({"softmax": ops.EPI_SOFTMAX, "softmax_bwd": ops.EPI_SOFTMAX_BWD}.get(case.op, ops.EPI_NONE), float(case.alpha),
                            Zt.v if case.has_z else None, S.v if S is not None else None, env.g["ps"] if case.post else None)
    pl = env.plans[(case.plan, case.permuted)]
    Yb = None
    if bf16:
        Yb = View(R.N_ROWS, case.d, torch.bfloat16, 0.0)
        Yb.buf.view(torch.int16).fill_(BF16_SENTINEL); Yb.pristine = Yb.buf.clone()
        ops.spmm_bf16(a, Xb.v, out=Y.v, out_bf16=Yb.v, epilogue=epi, plan=pl)
    else:
        ops.spmm_raw(a, Xw.v, out=Y.v, epilogue=epi, plan=pl)
    torch.cuda.synchronize()
    for name, v in (("Xb", Xb), ("Xw", Xw), ("Z", Z), ("S", S)):
        assert v is None or v.unchanged(), "%s: the call wrote to %s or its guards" % (case.label(), name)
    assert Y.guards_unchanged(), "%s: the call wrote outside Y" % case.label()
    assert Yb is None or Yb.guards_unchanged(), "%s: the call wrote outside Yb" % case.label()
    return Y, Yb


CASES = B.cases()


@pytest.mark.parametrize("width", B.WIDTHS)
def test_bf16_row_product_against_the_fp32_kernel_and_float64(env, width):
    cases = [c for c in CASES if c.d == width]
    assert cases
    worst = 0.0
    for case in cases:
        Y, Yb = _run(env, case, True)
        twin, _ = _run(env, case, False)
        got = Y.v.contiguous()
        assert torch.equal(got.view(torch.int32), twin.v.contiguous().view(torch.int32)), \
            "%s: differs from llmrec_spmm_f32 on the widened operand" % case.label()                       # (a)
        g = got.cpu().numpy()
        assert np.isfinite(g).all(), case.label()
        want, bound, relative = B.reference(case)
        err = np.abs(g.astype(np.float64) - want)
        tol = bound * np.abs(want) if relative else bound
        bad = err > tol
        assert not bad.any(), "%s: %d elements in %d rows out of the float64 bound (worst row %d)" % (
            case.label(), int(bad.sum()), int(bad.any(1).sum()), int(np.argmax((err - tol).max(1))))        # (b)
        pos = tol > 0
        worst = max(worst, float((err[pos] / tol[pos]).max()))
        assert torch.equal(Yb.v.contiguous().view(torch.int16), got.to(torch.bfloat16).view(torch.int16)), \
            "%s: Yb is not the RNE of the finished rows" % case.label()                                      # (c)
        again, Yb2 = _run(env, case, True)                                                                   # a repeated call: the same bits
        assert torch.equal(again.v.contiguous().view(torch.int32), got.view(torch.int32)) and torch.equal(Yb2.v.contiguous(), Yb.v.contiguous())
    print("d = %d: %d cases, worst error / bound %.4f" % (width, len(cases), worst))


def test_a_refused_call_writes_nothing(env):
    ops = env.ops
    case = R.Case(64, "pattern_rs", "none", False, "buckets")
    Xb, _ = env.x_views(64)
    a = env.operand(case)
    Y = View(R.N_ROWS, 64, torch.float32, R.SENTINEL)
    Yb = View(R.N_ROWS, 64, torch.bfloat16, 3.0)
    mask = torch.full((R.N_COLS,), R.STAMP, dtype=torch.uint8, device=DEV)
    flag = torch.full((R.N_ROWS,), R.STAMP, dtype=torch.uint8, device=DEV)
    pl = env.plans[("buckets", False)]
    refused = [dict(epilogue=ops.spmm_epilogue(ops.EPI_NONE, x_row_mask=mask, x_mask_active=R.STAMP)),
               dict(epilogue=ops.spmm_epilogue(ops.EPI_NONE, y_row_needed=flag, x_mask_active=R.STAMP)),
               dict(epilogue=ops.spmm_epilogue(ops.EPI_NONE, rows_listed_only=True))]
    for kw in refused:
        with pytest.raises(RuntimeError, match="spmm_xbf16"):
            ops.spmm_bf16(a, Xb.v, out=Y.v, out_bf16=Yb.v, plan=pl, **kw)
    with pytest.raises(RuntimeError, match="spmm_xbf16"):                                  # rows of Xb that are not 8-byte aligned
        ops.spmm_bf16(a, Xb.buf[2:2 + R.N_COLS * 66].view(R.N_COLS, 66)[:, :64], out=Y.v, out_bf16=Yb.v, plan=pl)
    wide = torch.zeros(R.N_COLS, 260, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="spmm_xbf16: d = 260"):
        ops.spmm_bf16(a, wide, plan=pl)
    with pytest.raises(RuntimeError, match="bfloat16"):
        ops.spmm_bf16(a, wide.float(), plan=pl)
    torch.cuda.synchronize()
    assert Y.unchanged() and Yb.unchanged() and Xb.unchanged()


@pytest.mark.parametrize("rows,d", [(1000, 64), (257, 36), (33, 7), (5, 256), (70000, 128)])
def test_rows_to_bf16_is_torchs_rounding(rows, d):
    from llmrec_amd import ops
    rng = np.random.default_rng(rows + d)
    x = rng.standard_normal((rows, d + 12)).astype(np.float32)
    x[0, :8] = np.array([0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x00000001, 0x80008000, 0x7f7fffff, 0x7f800000], dtype=np.uint32).view(np.float32)[:8]
    big = torch.from_numpy(x).to(DEV)
    s = torch.from_numpy((rng.random(rows) + 0.5).astype(np.float32)).to(DEV)
    for X in (big[:, :d].contiguous(), big[:, :d], big[:, 4:4 + d], big[:, 1:1 + d]):      # contiguous, strided, strided off a 16-byte line
        for scale in (None, s):
            want = (X if scale is None else scale[:, None] * X).to(torch.bfloat16)
            got = ops.rows_to_bf16(X, row_scale=scale)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (tuple(X.stride()), scale is not None)
            out = torch.full((rows + 2, d + 4), 7.0, dtype=torch.bfloat16, device=DEV)      # into a strided view: nothing else written
            ops.rows_to_bf16(X, out=out[1:-1, :d], row_scale=scale)
            assert torch.equal(out[1:-1, :d].contiguous().view(torch.int16), want.view(torch.int16))
            assert bool((out[0] == 7.0).all()) and bool((out[-1] == 7.0).all()) and bool((out[:, d:] == 7.0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# the row-sharded step
# ------------------------------------------------------------------------------------------------------------------------------------
def _spy_backend():
    from llmrec_amd import dist as ld

    class Spy(ld.HipBackend):
        """counts the products and checks every bf16 one against the fp32 kernel on the widened shadow"""

        def __init__(self):
            super().__init__()
            self.n_bf16 = self.n_fp32 = self.n_conv = self.n_yb = 0

        def to_bf16(self, X, out, row_scale=None):
            r = super().to_bf16(X, out, row_scale)
            assert torch.equal(out.view(torch.int16), X.to(torch.bfloat16).view(torch.int16))
            self.n_conv += 1
            return r

        def spmm_rows_compact(self, csr, X, row_list, n_list, out):
            self.n_fp32 += 1
            return super().spmm_rows_compact(csr, X, row_list, n_list, out)

        def spmm(self, csr, X, out=None, epilogue=None, x_bf16=None, out_bf16=None):
            if x_bf16 is None:
                self.n_fp32 += 1
                return super().spmm(csr, X, out=out, epilogue=epilogue)
            o = self.ops
            # the shadow is the RNE of its fp32 source at the moment it is gathered
            assert torch.equal(x_bf16.view(torch.int16), X.to(torch.bfloat16).view(torch.int16)), "a stale or wrong shadow is gathered"
            e = epilogue or {}
            assert not any(e.get(k) is not None for k in ("x_row_mask", "y_row_flag", "z_row_flag", "y_row_gate", "y_row_needed"))
            epi = o.spmm_epilogue({"none": o.EPI_NONE, "softmax": o.EPI_SOFTMAX, "softmax_bwd": o.EPI_SOFTMAX_BWD}[e.get("op", "none")],
                                  e.get("alpha", 0.0), e.get("Z"), e.get("S"), e.get("post_scale"))
            twin = o.spmm_raw(csr, x_bf16.float(), out=torch.full_like(out, float("nan")), epilogue=epi, plan=csr.plan_for(X.shape[1], whole_row=True)[1])
            Y = super().spmm(csr, X, out=out, epilogue=epilogue, x_bf16=x_bf16, out_bf16=out_bf16)
            assert torch.equal(Y.view(torch.int32), twin.view(torch.int32)), "a bf16 product differs from the fp32 kernel on the widened shadow"
            if out_bf16 is not None:
                assert torch.equal(out_bf16.view(torch.int16), Y.to(torch.bfloat16).view(torch.int16))
                self.n_yb += 1
            self.n_bf16 += 1
            return Y
    return Spy()


def _run_rank(rank, world, n_chunks, D, n_aug, backend=None, steps=B.STEP_STEPS, **kw):
    from llmrec_amd import dist as ld
    from llmrec_amd.dist_fused import ShardedFusedID
    rows, cols, u_tab, i_tab, batches = B.step_problem(world, D, n_aug)
    comm, be = ld.Comm(), backend or ld.HipBackend()
    u0, u1 = ld.user_block(B.STEP_U, rank, world)
    sel = (rows >= u0) & (rows < u1)
    g = ld.ShardedGraph.build(torch.tensor(rows[sel] - u0).cuda(), torch.tensor(cols[sel]).cuda(), u1 - u0, B.STEP_I, u0, comm, be)
    st = ShardedFusedID(g, comm, be, D, B.STEP_L, B.STEP_U, seed=1, lr=B.STEP_LR, batch_local=B.STEP_B + n_aug, drop_rate=B.STEP_DROP,
                        decay=B.STEP_DECAY, n_chunks=n_chunks, user_init=torch.tensor(u_tab[u0:u1]), item_init=torch.tensor(i_tab),
                        batch_size_flag=float(world * B.STEP_B), gather_dtype="bf16", **kw)
    assert st.bf16 and st.Ub.dtype == torch.bfloat16 and st.message_bytes_per_step()["bf16_shadow_bytes"] == 2 * (st.U + st.I) * D
    losses = []
    for per_rank in batches[:steps]:
        us, ps, ns = per_rank[rank]
        loss, _ = st.step((torch.tensor(us - u0).cuda(), torch.tensor(ps).cuda(), torch.tensor(ns).cuda()))
        losses.append(float(loss))
        assert float(st.dE_u.abs().max()) == 0.0 and float(st.dE_i.abs().max()) == 0.0    # the scatter targets end all-zero
    return st, losses


def _state(st):
    out = [st.user_tab.detach().clone(), st.item_tab.detach().clone()]
    for p in (st.user_tab, st.item_tab):
        out += [t.clone() for t in st.opt.moments(p)]
    return out


def _assert_losses_gated(losses, D, n_aug, sparse_forward, world, what, key=None):
    ref = B.oracle_losses(world, D, n_aug, "fp32", True)
    gate = 4.0 * B.STEP_DEVIATION[key or (D, n_aug, sparse_forward, world)]
    dev = [abs(a - b) for a, b in zip(losses, ref)]
    print("%s: losses %s, fp32 oracle %s, deviation %s, gate %.3e" % (what, losses, list(ref), ["%.3e" % x for x in dev], gate))
    assert max(dev) <= gate, (what, dev, gate)


@pytest.mark.parametrize("D,n_aug", B.STEP_CASES)
@pytest.mark.parametrize("n_chunks", [1, 5])
@pytest.mark.parametrize("sparse_forward", [True, False])
def test_step_in_bf16_gather_mode(D, n_aug, n_chunks, sparse_forward):
    spy = _spy_backend()
    st, losses = _run_rank(0, 1, n_chunks, D, n_aug, backend=spy, sparse_forward=sparse_forward)
    assert len(st.chunks) == n_chunks and st.sparse_forward == sparse_forward
    n, steps = n_chunks, B.STEP_STEPS
    # per step - restricted forward: U1, I1 (chunks) | masked U2, listed I2, masked R g in fp32 | R^T h (chunks), R dI1, R^T h (chunks);
    #            dense forward: U1, I1, U2, I2 | masked R g in fp32 | the same three
    want_bf16, want_fp32, want_conv, want_yb = ((2 + 3 * n, 3, 3, 2) if sparse_forward else (3 + 4 * n, 1, 4, 3))
    assert (spy.n_bf16, spy.n_fp32, spy.n_conv, spy.n_yb) == (steps * want_bf16, steps * want_fp32, steps * want_conv, steps * want_yb)
    if n_chunks == 1 and sparse_forward:
        assert (want_bf16, want_fp32) == (5, 3)
    _assert_losses_gated(losses, D, n_aug, sparse_forward, 1, "d = %d, %d chunks, sparse_forward %s" % (D, n_chunks, sparse_forward))
    # a second fresh run (plain backend): the same bits in both tables and both moments
    st2, losses2 = _run_rank(0, 1, n_chunks, D, n_aug, sparse_forward=sparse_forward)
    assert losses2 == losses
    for a, b in zip(_state(st), _state(st2)):
        assert torch.equal(a, b)
    # evaluation runs the same mode: its forward gathers bf16 rows too
    before = spy.n_bf16
    idx, _ = st.eval_topk(torch.arange(16, device=DEV), K=10)
    assert spy.n_bf16 - before == 2 * (1 + n) and idx.shape == (16, 10)


def test_step_in_bf16_gather_mode_with_the_dense_backward():
    """sparse_backward=False: g is formed by dense passes and R g is a bf16 product with the softmax-backward epilogue - no fp32 product left"""
    spy = _spy_backend()
    st, losses = _run_rank(0, 1, 5, 64, 0, backend=spy, sparse_backward=False)
    assert not st.sparse_forward and (spy.n_bf16, spy.n_fp32, spy.n_conv, spy.n_yb) == tuple(B.STEP_STEPS * k for k in (4 + 4 * 5, 0, 4, 4))
    assert all(np.isfinite(losses))
    _assert_losses_gated(losses, 64, 0, False, 1, "d = 64, dense backward", key=(64, 0, False, 1, "dense backward"))


def test_the_default_mode_is_fp32_and_untouched_by_the_feature():
    from llmrec_amd import dist as ld
    from llmrec_amd.dist_fused import ShardedFusedID
    spy = _spy_backend()
    rows, cols, u_tab, i_tab, batches = B.step_problem(1, 64, 0)
    g = ld.ShardedGraph.build(torch.tensor(rows).cuda(), torch.tensor(cols).cuda(), B.STEP_U, B.STEP_I, 0, ld.Comm(), spy)
    st = ShardedFusedID(g, ld.Comm(), spy, 64, B.STEP_L, B.STEP_U, seed=1, lr=B.STEP_LR, batch_local=B.STEP_B, drop_rate=B.STEP_DROP, decay=B.STEP_DECAY)
    assert st.gather_dtype == "fp32" and st.Ub is None
    us, ps, ns = batches[0][0]
    st.step((torch.tensor(us).cuda(), torch.tensor(ps).cuda(), torch.tensor(ns).cuda()))
    assert spy.n_bf16 == 0 and spy.n_conv == 0 and spy.n_fp32 == 8


def _worker(rank, world, port, out_dir, D, n_aug, exchange):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    st, losses = _run_rank(rank, world, 3, D, n_aug, exchange=exchange)
    np.savez(os.path.join(out_dir, "g%d.npz" % rank), users=st.user_tab.detach().cpu().numpy(), items=st.item_tab.detach().cpu().numpy(),
             losses=np.array(losses))
    dist.barrier()
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("D,n_aug,exchange", [(64, 0, "all_reduce"), (128, 6, "rs_ag")])
def test_two_processes_on_one_gpu_keep_bit_identical_replicas(tmp_path, D, n_aug, exchange):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), D, n_aug, exchange), nprocs=world, join=True)
    r = [np.load(tmp_path / ("g%d.npz" % k)) for k in range(world)]
    assert np.array_equal(r[0]["items"].view(np.int32), r[1]["items"].view(np.int32))       # replicas bit-identical
    assert np.array_equal(r[0]["losses"], r[1]["losses"])
    _assert_losses_gated([float(x) for x in r[0]["losses"]], D, n_aug, True, world, "two processes, d = %d, %s" % (D, exchange))
