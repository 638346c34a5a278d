"""GPU: every row kernel of llmrec_amd/csrc/rowops.hip through the C ABI (llmrec_amd._lib with the ctypes structs of llmrec_amd.ops),
element by element against the fp64 references and per-element bounds of tests/_rowops_ref.py (tests/test_rowops_ref_cpu.py checks that
yardstick without a device). Operands are views of NaN-filled allocations (tests._eval_ref.Table), outputs views inside sentinel-filled
buffers whose surroundings - the padding columns between d and ld and the rows past the launch's row count included - are checked after
every call. Beside the bounds: the bit-exact relations the code promises (paired launches against single ones, the grouped launch against
its members, the unscaled softmax backward against alpha = 1, the listed against the full backward where the chains agree, the masked path
of the paired backward against the general one, repeated calls), the partial sums of llmrec_fuse_fwd_multi_sumsq_f32, the refusals and
rows == 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _rowops_ref as R
from tests._eval_ref import GUARD, Table

pytestmark = pytest.mark.gpu

DEV = "cuda"
assert GUARD == R.GUARD
WORST = {}                                                       # kernel -> the worst error / bound seen by this process


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


# ------------------------------------------------------------------------------------------------------------------------------------
# the calls (also used, with made-up addresses, by tests/test_rowops_ref_cpu.py for the refusals that return before any HIP call)
# ------------------------------------------------------------------------------------------------------------------------------------
def _tables(P, names):
    return (C.c_void_p * len(names))(*[P[n][0] for n in names]), (C.c_int64 * len(names))(*[P[n][1] for n in names])


def _fwd_problem(q, P, pre, n, keep):
    mt, ml = _tables(P, [pre + "m%d" % i for i in range(R.N_MEAN)])
    nt, nl = _tables(P, [pre + "n%d" % i for i in range(R.N_NORM)])
    rates = (C.c_float * R.N_NORM)(*R.RATES)
    keep += [mt, ml, nt, nl, rates]
    q.rows, q.mean_scale, q.n_mean, q.n_norm = n, R.MEAN_SCALE, R.N_MEAN, R.N_NORM
    q.mean_terms, q.mean_ld, q.norm_terms, q.norm_ld = (C.cast(x, C.c_void_p) for x in (mt, ml, nt, nl))
    q.rates, q.out, q.ldo = C.cast(rates, C.c_void_p), P[pre + "out"][0], P[pre + "out"][1]


def _bwd_tables(P, pre):
    nt, nl = _tables(P, [pre + "n%d" % i for i in range(R.N_NORM)])
    dt, dl = _tables(P, [pre + "d%d" % i for i in range(R.N_NORM)])
    src = {pre + "s0": P[pre + "s0"], pre + "s1": (None, 0), pre + "s2": P[pre + "s2"]}
    st, sl = _tables(src, [pre + "s%d" % i for i in range(R.N_NORM)])
    return nt, nl, dt, dl, st, sl, (C.c_float * R.N_NORM)(*R.RATES)


def _bwd_problem(q, P, pre, n, keep, flags=None, stamp=None, skip_from=0):
    nt, nl, dt, dl, st, sl, rates = _bwd_tables(P, pre)
    keep += [nt, nl, dt, dl, st, sl, rates]
    q.rows, q.dOut, q.lddo, q.n_norm = n, P[pre + "dOut"][0], P[pre + "dOut"][1], R.N_NORM
    q.norm_terms, q.norm_ld, q.rates, q.d_terms, q.d_ld, q.src_terms, q.src_ld = (C.cast(x, C.c_void_p) for x in (nt, nl, rates, dt, dl, st, sl))
    q.n_reg_terms, q.reg_two_coef, q.row_flags, q.row_stamp, q.zero_skip_from_term = R.N_REG, R.REG2, flags, stamp, skip_from


def launch(entry, d, rows, P, mode=None, stream=None, masks=None, sumsq=None, compact=None):
    """one call of `entry` -> the status. rows: an int, or (rows of problem 0, rows of problem 1); P: operand -> (address, ld);
    masks: per problem (row_flags, row_stamp, zero_skip_from_term); sumsq: (n_sumsq, partial address, capacity, c_int32 for the count);
    compact: (n_users, flags, row_list, n_rows) addresses"""
    from llmrec_amd import _lib, ops as O
    keep = []
    if entry == "softmax_fwd":
        args = ("llmrec_softmax_rows_fwd_f32", rows, d, *P["Z"], *P["Y"], stream)
    elif entry == "softmax_bwd":
        args = ("llmrec_softmax_rows_bwd_scaled_f32", rows, d, R.ALPHA, *P["Y"], *P["dY"], *P["dZ"], stream)
    elif entry == "softmax_bwd_unscaled":
        args = ("llmrec_softmax_rows_bwd_f32", rows, d, *P["Y"], *P["dY"], *P["dZ"], stream)
    elif entry == "fuse_fwd":
        mt, ml = _tables(P, ["m%d" % i for i in range(R.N_MEAN)])
        nt, nl = _tables(P, ["n%d" % i for i in range(R.N_NORM)])
        args = ("llmrec_fuse_fwd_f32", rows, d, R.MEAN_SCALE, R.N_MEAN, mt, ml, R.N_NORM, nt, nl, (C.c_float * R.N_NORM)(*R.RATES), *P["out"], stream)
    elif entry == "fuse_bwd":
        nt, nl, dt, dl, st, sl, rates = _bwd_tables(P, "")
        if mode == "source":
            args = ("llmrec_fuse_bwd_src_f32", rows, d, *P["dOut"], R.N_NORM, nt, nl, rates, dt, dl, st, sl, R.N_REG, R.REG2, stream)
        else:
            args = ("llmrec_fuse_bwd_f32", rows, d, *P["dOut"], R.N_NORM, nt, nl, rates, dt, dl, int(mode == "accumulate"), R.N_REG, R.REG2, stream)
    elif entry in ("fuse_fwd_multi", "fuse_fwd_multi_sumsq", "fuse_fwd_multi_sumsq_compact"):
        arr = (O.FuseFwdProblem * 2)()
        for k in (0, 1):
            _fwd_problem(arr[k], P, "p%d." % k, rows[k], keep)
        if entry == "fuse_fwd_multi":
            args = ("llmrec_fuse_fwd_multi_f32", 2, arr, d, stream)
        else:
            n_sumsq, partial, cap, count = sumsq
            args = ("llmrec_" + entry + "_f32", 2, arr, d, n_sumsq, partial, cap, C.byref(count)) + (tuple(compact) if compact else ()) + (stream,)
    elif entry == "fuse_bwd_src_multi":
        arr = (O.FuseBwdProblem * 2)()
        for k in (0, 1):
            _bwd_problem(arr[k], P, "p%d." % k, rows[k], keep, *(masks[k] if masks else ()))
        args = ("llmrec_fuse_bwd_src_multi_f32", 2, arr, d, stream)
    else:
        raise KeyError(entry)
    return _lib._invoke(args[0], args[1:])


def ok(status):
    from llmrec_amd import _lib
    assert status == 0, "status %d: %s" % (status, _lib.load().llmrec_last_error().decode())


# ------------------------------------------------------------------------------------------------------------------------------------
# buffers
# ------------------------------------------------------------------------------------------------------------------------------------
def tab(spec, src):
    ld, col0, mod = spec
    return Table("operand", src, ld, col0, mod, DEV)


class Out:
    """an output view [rows, cols] (row stride ld, first column col0) inside a sentinel-filled buffer; init: what the view holds before a
    call (None: the sentinel). get(n) checks that only the first n rows of the view were written."""

    def __init__(self, rows, cols, spec=None, init=None):
        ld, col0, mod = spec or (cols, 0, 0)
        self.buf = torch.full((2 * GUARD + rows * ld,), R.SENTINEL, dtype=torch.float32, device=DEV)
        self.v = torch.as_strided(self.buf, (rows, cols), (ld, 1), GUARD + col0)
        assert self.v.data_ptr() % 16 == mod
        idx = GUARD + col0 + torch.arange(rows, device=DEV)[:, None] * ld + torch.arange(cols, device=DEV)[None, :]
        self.outside = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        self.outside[idx.reshape(-1)] = False
        self.ld = ld
        self.fill(init)

    @property
    def p(self):
        return (self.v.data_ptr(), self.ld)

    def fill(self, init=None):
        self.init = np.full(tuple(self.v.shape), R.SENTINEL, dtype=np.float32) if init is None else np.ascontiguousarray(init, dtype=np.float32)
        self.v.copy_(torch.from_numpy(self.init).to(DEV))

    def get(self, n=None):
        assert bool((self.buf[self.outside] == R.SENTINEL).all()), "something wrote outside the output view"
        got = self.v.cpu().numpy().copy()
        n = got.shape[0] if n is None else n
        assert np.array_equal(bits(got[n:]), bits(self.init[n:])), "rows past the launch's row count were written"
        return got[:n]

    def untouched(self):
        return bool((self.buf[self.outside] == R.SENTINEL).all()) and np.array_equal(bits(self.v.cpu().numpy()), bits(self.init))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        i = tuple(int(x[0]) for x in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ in bits, first at %s: %r != %r" % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


def within(got, want, bound, what, kernel=None):
    """element by element |got - want| <= bound, every result finite (an inf the reference demands must be that inf)"""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), "%s: the overflowed elements differ" % what
    got, want, bound = got[~inf], want[~inf], np.broadcast_to(bound, inf.shape)[~inf]
    assert np.isfinite(got).all(), "%s: %d non-finite results" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    if kernel:
        WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)
    bad = err > bound
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError("%s: %d of %d elements over the bound, first (flat) %d: got %r want %r err %.3g bound %.3g; worst err / bound %.3g"
                             % (what, int(bad.sum()), bad.size, i, got[i], want[i], err[i], bound[i], ratio))
    return ratio


def report(kernel):
    print("[rowops] %s: worst error / bound so far = %.3g" % (kernel, WORST.get(kernel, 0.0)))


def stream(ops):
    return ops._stream()


# ------------------------------------------------------------------------------------------------------------------------------------
# one problem's operands on the device
# ------------------------------------------------------------------------------------------------------------------------------------
class SoftmaxOperands:
    def __init__(self, case, rmax):
        d = case.d
        self.Z, self.Y, self.dY = R.softmax_inputs(rmax, d, "softmax", d)
        self.t = {"Z": tab(case.spec("Z"), self.Z), "Y": tab(case.spec("Y"), self.Y), "dY": tab(case.spec("dY"), self.dY)}
        self.out = {"Y": Out(rmax, d, case.spec("Y")), "dZ": Out(rmax, d, case.spec("dZ"))}

    def P(self, fwd):
        if fwd:
            return {"Z": (self.t["Z"].t.data_ptr(), self.t["Z"].ld), "Y": self.out["Y"].p}
        return {"Y": (self.t["Y"].t.data_ptr(), self.t["Y"].ld), "dY": (self.t["dY"].t.data_ptr(), self.t["dY"].ld), "dZ": self.out["dZ"].p}

    def check(self):
        for t in self.t.values():
            t.check()


class FuseOperands:
    """the forward and the backward operands of one fusion problem; pre: "" or "p0." / "p1." (the names of R.OPERANDS)"""

    def __init__(self, case, pre, rmax, prob, fwd):
        d = case.d
        self.pre, self.inp = pre, R.fuse_inputs(rmax, d, "fuse", d, prob)
        f = self.inp
        self.t, self.out = {}, {}
        for i, x in enumerate(f.norms):
            self.t["n%d" % i] = tab(case.spec(pre + "n%d" % i), x)
        if fwd:
            for i, x in enumerate(f.means):
                self.t["m%d" % i] = tab(case.spec(pre + "m%d" % i), x)
            self.out["out"] = Out(rmax, d, case.spec(pre + "out"))
        else:
            self.t["dOut"] = tab(case.spec(pre + "dOut"), f.G)
            for i in (0, 2):
                self.t["s%d" % i] = tab(case.spec(pre + "s%d" % i), f.srcs[i])
            for i in range(R.N_NORM):
                self.out["d%d" % i] = Out(rmax, d, case.spec(pre + "d%d" % i))

    def P(self):
        P = {self.pre + k: (t.t.data_ptr(), t.ld) for k, t in self.t.items()}
        P.update({self.pre + k: o.p for k, o in self.out.items()})
        return P

    def fill(self, mode=None):
        for i in range(R.N_NORM):
            if "d%d" % i in self.out:
                self.out["d%d" % i].fill(self.inp.olds[i] if mode == "accumulate" else None)
        if "out" in self.out:
            self.out["out"].fill()

    def check(self):
        for t in self.t.values():
            t.check()


def bases_of(f, mode):
    return {"overwrite": (None,) * R.N_NORM, "accumulate": f.olds, "source": f.srcs, None: f.srcs}[mode]


def check_fuse_bwd(fo, n, L, mode, what, kernel):
    f = R.fuse_cut(fo.inp, n)
    ref = R.fuse_bwd(f.G, f.norms, R.RATES, L, bases_of(f, mode), R.N_REG, R.REG2)
    got = [fo.out["d%d" % i].get(n) for i in range(R.N_NORM)]
    for i, (g, (want, bound)) in enumerate(zip(got, ref)):
        within(g, want, bound, "%s term %d" % (what, i), kernel)
    return got


def check_fuse_fwd(fo, n, L, what, kernel):
    f = R.fuse_cut(fo.inp, n)
    want, bound = R.fuse_fwd(f.means, R.MEAN_SCALE, f.norms, R.RATES, L)
    got = fo.out["out"].get(n)
    within(got, want, bound, what, kernel)
    return got


def chain(inst):
    return inst[0] * inst[1]


# ------------------------------------------------------------------------------------------------------------------------------------
# every table case against fp64
# ------------------------------------------------------------------------------------------------------------------------------------
def _cases(entry):
    return [c for c in R.cases() if c.entry == entry]


_EXPF = {"rel_u": 0.0, "rest_u": -1e9, "ulp": -1e9}


@pytest.mark.parametrize("case", _cases("softmax_fwd"), ids=lambda c: c.name)
def test_softmax_forward(ops, case):
    so = SoftmaxOperands(case, max(case.rows))
    inst = case.expect()
    for n in case.rows:
        so.out["Y"].fill()
        ok(launch("softmax_fwd", case.d, n, so.P(True), stream=stream(ops)))
        got = so.out["Y"].get(n)
        want, bound = R.softmax_fwd(so.Z[:n], chain(inst))
        within(got, want, bound, "%s rows %d" % (case.name, n), "softmax_fwd_kernel<%d, %d>" % inst)
        for k, x in zip(("rel_u", "rest_u", "ulp"), R.softmax_expf_ulp(got, so.Z[:n], chain(inst))):
            _EXPF[k] = max(_EXPF[k], x)
    so.check()
    report("softmax_fwd_kernel<%d, %d>" % inst)
    print("[rowops] softmax forward so far: worst relative error %.3g u; less the exponent argument's rounding %.3g u; share left to expf %.3g ulp "
          "(E_EXP = %d)" % (_EXPF["rel_u"], _EXPF["rest_u"], _EXPF["ulp"], R.E_EXP))


@pytest.mark.parametrize("case", _cases("softmax_bwd"), ids=lambda c: c.name)
def test_softmax_backward(ops, case):
    so = SoftmaxOperands(case, max(case.rows))
    inst = case.expect()
    for n in case.rows:
        so.out["dZ"].fill()
        ok(launch("softmax_bwd", case.d, n, so.P(False), stream=stream(ops)))
        want, bound = R.softmax_bwd(so.Y[:n], so.dY[:n], R.ALPHA, chain(inst))
        within(so.out["dZ"].get(n), want, bound, "%s rows %d" % (case.name, n), "softmax_bwd_kernel<%d, %d>" % inst)
    so.check()
    report("softmax_bwd_kernel<%d, %d>" % inst)


@pytest.mark.parametrize("case", _cases("fuse_fwd"), ids=lambda c: c.name)
def test_fusion_forward(ops, case):
    fo = FuseOperands(case, "", max(case.rows), 0, True)
    inst = case.expect()
    for n in case.rows:
        fo.fill()
        ok(launch("fuse_fwd", case.d, n, fo.P(), stream=stream(ops)))
        check_fuse_fwd(fo, n, chain(inst), "%s rows %d" % (case.name, n), "fuse_fwd_kernel<%d, %d>" % inst)
    fo.check()
    report("fuse_fwd_kernel<%d, %d>" % inst)


@pytest.mark.parametrize("case", _cases("fuse_bwd"), ids=lambda c: c.name)
def test_fusion_backward(ops, case):
    fo = FuseOperands(case, "", max(case.rows), 0, False)
    for mode in R.MODES["fuse_bwd"]:
        inst = case.expect(mode)
        for n in case.rows:
            fo.fill(mode)
            ok(launch("fuse_bwd", case.d, n, fo.P(), mode=mode, stream=stream(ops)))
            check_fuse_bwd(fo, n, chain(inst), mode, "%s %s rows %d" % (case.name, mode, n), "fuse_bwd_kernel<%d, %d>" % inst)
        report("fuse_bwd_kernel<%d, %d>" % inst)
    fo.check()


@pytest.mark.parametrize("case", _cases("fuse_fwd_multi"), ids=lambda c: c.name)
def test_paired_fusion_forward(ops, case):
    fos = [FuseOperands(case, "p%d." % k, max(r), k, True) for k, r in enumerate((case.rows, case.rows1))]
    inst = case.expect()
    P = {**fos[0].P(), **fos[1].P()}
    for n0, n1 in zip(case.rows, case.rows1):
        for fo in fos:
            fo.fill()
        ok(launch("fuse_fwd_multi", case.d, (n0, n1), P, stream=stream(ops)))
        for fo, n in zip(fos, (n0, n1)):
            check_fuse_fwd(fo, n, chain(inst), "%s rows (%d, %d) problem %s" % (case.name, n0, n1, fo.pre), "fuse_fwd_multi_kernel<%d, %d>" % inst)
    for fo in fos:
        fo.check()
    report("fuse_fwd_multi_kernel<%d, %d>" % inst)


@pytest.mark.parametrize("case", _cases("fuse_bwd_src_multi"), ids=lambda c: c.name)
def test_paired_fusion_backward(ops, case):
    fos = [FuseOperands(case, "p%d." % k, max(r), k, False) for k, r in enumerate((case.rows, case.rows1))]
    inst = case.expect()
    P = {**fos[0].P(), **fos[1].P()}
    for n0, n1 in zip(case.rows, case.rows1):
        for fo in fos:
            fo.fill()
        ok(launch("fuse_bwd_src_multi", case.d, (n0, n1), P, stream=stream(ops)))
        for fo, n in zip(fos, (n0, n1)):
            check_fuse_bwd(fo, n, chain(inst), "source", "%s rows (%d, %d) problem %s" % (case.name, n0, n1, fo.pre),
                           "fuse_bwd_src_multi_kernel<%d, %d>" % inst)
    for fo in fos:
        fo.check()
    report("fuse_bwd_src_multi_kernel<%d, %d>" % inst)


# ------------------------------------------------------------------------------------------------------------------------------------
# the bit-exact relations
# ------------------------------------------------------------------------------------------------------------------------------------
def _contig(entry, d, rows, rows1=(), layout="contig"):
    """layout "ld1": ld = d + 1 on the entry's first operand - the scalar family at a d that is a multiple of 4"""
    return R.Case(entry, d, layout, None if layout == "contig" else R.OPERANDS[entry][0], rows, rows1)


_REL = dict(argnames="d,layout", argvalues=R.D_RELATIONS, ids=["%d-%s" % dl for dl in R.D_RELATIONS])


@pytest.mark.parametrize(**_REL)
def test_paired_launches_equal_the_single_ones_and_repeat(ops, d, layout):
    n = (67, 37)
    for fwd, multi, single in ((True, "fuse_fwd_multi", "fuse_fwd"), (False, "fuse_bwd_src_multi", "fuse_bwd")):
        case = _contig(multi, d, (n[0],), (n[1],), layout)
        assert case.expect() == R.instance(d, layout == "contig")
        fos = [FuseOperands(case, "p%d." % k, n[k], k, fwd) for k in (0, 1)]
        P = {**fos[0].P(), **fos[1].P()}
        names = ["out"] if fwd else ["d%d" % i for i in range(R.N_NORM)]
        runs = []
        for rep in range(2):
            for fo in fos:
                fo.fill()
            ok(launch(multi, d, n, P, stream=stream(ops)))
            runs.append([[fo.out[k].get() for k in names] for fo in fos])
        for k, fo in enumerate(fos):
            fo.fill()
            ok(launch(single, d, n[k], {key[len(fo.pre):]: v for key, v in fo.P().items()}, mode="source", stream=stream(ops)))
            # (the paired launch is scalar as soon as ONE operand of either problem is; alone, the other problem is a float4 shape: its
            # chain differs, and the family tests hold it to the bound)
            alone = R.Case(single, d, layout if k == 0 else "contig", R.OPERANDS[single][0] if layout != "contig" and k == 0 else None, (n[k],))
            for name, a, b in zip(names, runs[0][k], runs[1][k]):
                same_bits(b, a, "%s d %d problem %d %s repeated" % (multi, d, k, name))
                if alone.expect("source") == case.expect():
                    same_bits(a, fo.out[name].get(), "%s d %d problem %d %s against %s" % (multi, d, k, name, single))
                else:
                    assert layout != "contig" and k == 1


@pytest.mark.parametrize(**_REL)
def test_softmax_backward_relations(ops, d, layout):
    """unscaled = scaled at alpha 1; listed over all rows with a NULL post_scale = the full backward in bits where the full kernel is the
    scalar form (the listed chain is c += 16: the same order), under the bound elsewhere; listed rows with a post_scale, -1 and duplicates"""
    from llmrec_amd import _lib
    n = 67
    case = _contig("softmax_bwd", d, (n,), layout=layout)
    so = SoftmaxOperands(case, n)
    P, dZ = so.P(False), so.out["dZ"]
    inst = case.expect()
    assert inst == R.instance(d, layout == "contig")

    def run(fn):
        dZ.fill()
        ok(fn())
        return dZ.get()

    one = run(lambda: _lib._invoke("llmrec_softmax_rows_bwd_scaled_f32", (n, d, 1.0, *P["Y"], *P["dY"], *P["dZ"], stream(ops))))
    same_bits(run(lambda: launch("softmax_bwd_unscaled", d, n, P, stream=stream(ops))), one, "d %d unscaled against alpha = 1" % d)
    # alpha = 0.5: alpha g is exact, so a contraction of "alpha g - dot" in the listed kernel cannot change the value
    half = run(lambda: _lib._invoke("llmrec_softmax_rows_bwd_scaled_f32", (n, d, 0.5, *P["Y"], *P["dY"], *P["dZ"], stream(ops))))
    ids = torch.arange(n, dtype=torch.int64, device=DEV)
    listed = run(lambda: _lib._invoke("llmrec_softmax_rows_bwd_listed_f32", (n, ops._p(ids), d, 0.5, *P["Y"], *P["dY"], None, *P["dZ"], stream(ops))))
    want, bound = R.softmax_bwd(so.Y, so.dY, 0.5, R.ceil_div(d, 16))
    within(listed, want, bound, "d %d listed, all rows" % d, "softmax_bwd_listed_kernel")
    if inst[0] == 1:
        same_bits(listed, half, "d %d listed against the full scalar kernel" % d)
    pick = np.array([5, -1, 66, 0, 5, 17, 33, -1, 2, 4], dtype=np.int64)
    ps = R.mixed(n, 1, "post_scale", d)[:, 0]
    tps = Table("post_scale", ps.reshape(-1, 1), 1, 0, 0, DEV)
    ids = torch.from_numpy(pick).to(DEV)
    got = run(lambda: _lib._invoke("llmrec_softmax_rows_bwd_listed_f32",
                                   (len(pick), ops._p(ids), d, R.ALPHA, *P["Y"], *P["dY"], tps.t.data_ptr(), *P["dZ"], stream(ops))))
    want, bound = R.softmax_bwd(so.Y, so.dY, R.ALPHA, R.ceil_div(d, 16), post_scale=ps)
    rows = np.unique(pick[pick >= 0])
    within(got[rows], want[rows], bound[rows], "d %d listed rows with a post_scale" % d, "softmax_bwd_listed_kernel")
    rest = np.setdiff1d(np.arange(n), rows)
    assert (got[rest] == R.SENTINEL).all(), "an unlisted row was written"
    so.check(), tps.check()
    report("softmax_bwd_listed_kernel")


@pytest.mark.parametrize(**_REL)
@pytest.mark.parametrize("stamped", (False, True))
def test_masked_path_of_the_paired_backward_equals_the_general_path(ops, d, layout, stamped):
    """rows whose dOut and sources are all-zero, flagged not active: the same bits as the general path (no flags); with
    zero_skip_from_term = 2 the third term of such a row is not written"""
    n = (67, 37)
    case = _contig("fuse_bwd_src_multi", d, (n[0],), (n[1],), layout)
    fos = [FuseOperands(case, "p%d." % k, n[k], k, False) for k in (0, 1)]
    counter = 255 * 3 + 41                                        # LLMREC_ROW_STAMP(counter) = counter % 255 + 1
    active_value = counter % 255 + 1 if stamped else 7
    stale = 9 if stamped else 0                                   # a flag of another step / a clear flag: not active
    stamp = torch.tensor([counter], dtype=torch.int32, device=DEV)
    masks, idle = [], []
    for k, fo in enumerate(fos):
        off = np.arange(n[k]) % 3 == 1
        idle.append(off)
        sel = torch.from_numpy(off).to(DEV)
        for name in ("dOut", "s0", "s2"):                         # the promise of a row that is not active
            fo.t[name].t[sel] = 0.0
            fo.t[name].src[torch.from_numpy(off)] = 0.0
        flags = torch.full((n[k],), active_value, dtype=torch.uint8, device=DEV)
        flags[sel] = stale
        masks.append((flags, stamp if stamped else None))
    P = {**fos[0].P(), **fos[1].P()}
    names = ["d%d" % i for i in range(R.N_NORM)]

    def run(m):
        for fo in fos:
            fo.fill()
        ok(launch("fuse_bwd_src_multi", d, n, P, masks=m, stream=stream(ops)))
        return [[fo.out[k].get() for k in names] for fo in fos]

    general = run(None)
    masked = run([(f.data_ptr(), s.data_ptr() if s is not None else None, 0) for f, s in masks])
    skipped = run([(f.data_ptr(), s.data_ptr() if s is not None else None, 2) for f, s in masks])
    for k in (0, 1):
        for i in range(R.N_NORM):
            same_bits(masked[k][i], general[k][i], "d %d problem %d term %d masked against general" % (d, k, i))
            want = general[k][i].copy()
            if i >= 2:
                want[idle[k]] = R.SENTINEL
            same_bits(skipped[k][i], want, "d %d problem %d term %d with zero_skip_from_term" % (d, k, i))
        assert (general[k][2][idle[k]] == 0).all()                # (what the skipped rows would have held: zeros nobody reads)
    for fo in fos:
        fo.check()


# ------------------------------------------------------------------------------------------------------------------------------------
# the partial sums of the paired forward, and the launch that also compacts the reach flags
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,n", ((64, (R.BIG_ROWS, 37)), (20, (67, 37)), (256, (17, 67))))
def test_paired_forward_partial_sums(ops, d, n):
    case = _contig("fuse_fwd_multi", d, (n[0],), (n[1],))
    fos = [FuseOperands(case, "p%d." % k, n[k], k, True) for k in (0, 1)]
    P = {**fos[0].P(), **fos[1].P()}
    inst = case.expect()
    blocks = R.row_blocks(n[0]) + R.row_blocks(n[1])
    n_sumsq = 2
    part = Out(1, blocks + 8)
    count = C.c_int32(-1)
    ok(launch("fuse_fwd_multi_sumsq", d, n, P, sumsq=(n_sumsq, part.v.data_ptr(), blocks + 8, count), stream=stream(ops)))
    assert count.value == blocks
    got = part.get()[0]
    assert (got[blocks:] == R.SENTINEL).all()
    want, bound = R.multi_sumsq([x for fo in fos for x in fo.inp.norms[:n_sumsq]], chain(inst), max(R.row_passes(r) for r in n) * n_sumsq)
    within(np.array([got[:blocks].astype(np.float64).sum()]), np.array([want]), np.array([bound]), "partial sums d %d" % d, "fuse_fwd_multi sumsq partials")
    outs = [check_fuse_fwd(fo, r, chain(inst), "sumsq launch d %d problem %s" % (d, fo.pre), "fuse_fwd_multi_kernel<%d, %d>" % inst) for fo, r in zip(fos, n)]
    ws = Out(1, blocks - 1)                                       # too small a buffer: LLMREC_EWORKSPACE, nothing written
    for fo in fos:
        fo.fill()
    assert launch("fuse_fwd_multi_sumsq", d, n, P, sumsq=(n_sumsq, ws.v.data_ptr(), blocks - 1, count), stream=stream(ops)) == -3
    torch.cuda.synchronize()
    assert ws.untouched() and all(fo.out["out"].untouched() for fo in fos)
    if inst[0] == 4:                                              # the same launch behind the compaction block: the same bits, the ascending list
        n_users = 1000 + 5
        flags = torch.zeros(R.ceil_div(n_users, 16) * 16, dtype=torch.uint8, device=DEV)
        marked = np.array([0, 3, 16, 17, 255, 256, 999, 1004])
        flags[torch.from_numpy(marked).to(DEV)] = 1
        rl = torch.full((n_users + 32,), -7, dtype=torch.int32, device=DEV)
        nr = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        part2 = Out(1, blocks + 8)
        ok(launch("fuse_fwd_multi_sumsq_compact", d, n, P, sumsq=(n_sumsq, part2.v.data_ptr(), blocks + 8, count),
                  compact=(n_users, ops._p(flags), ops._p(rl), ops._p(nr)), stream=stream(ops)))
        same_bits(part2.get()[0], got, "partials behind the compaction block")
        for fo, r, o in zip(fos, n, outs):
            same_bits(fo.out["out"].get(r), o, "outputs behind the compaction block")
        assert int(nr[0]) == len(marked) and np.array_equal(rl[:len(marked)].cpu().numpy(), marked) and not bool(flags.any())
    for fo in fos:
        fo.check()
    report("fuse_fwd_multi sumsq partials")


# ------------------------------------------------------------------------------------------------------------------------------------
# the grouped launch of the step
# ------------------------------------------------------------------------------------------------------------------------------------
def adamw_buffers(n, key, g_scale=1.0, with_gout=False):
    p, g, m, v = R.adamw_inputs(n, key)
    t = {k: Out(1, n, init=x.reshape(1, -1)) for k, x in (("p", p), ("m", m), ("v", v))}
    t["g"] = Table("g", g.reshape(1, -1), n, 0, 0, DEV)
    if with_gout:
        t["g_out"] = Out(1, n)
    return dict(inp=(p, g, m, v), t=t, n=n, gs=g_scale)


def adamw_array(ops, bufs):
    arr = (ops.AdamwTensor * len(bufs))()
    for a, b in zip(arr, bufs):
        t = b["t"]
        a.p, a.g, a.m, a.v, a.n = t["p"].v.data_ptr(), t["g"].t.data_ptr(), t["m"].v.data_ptr(), t["v"].v.data_ptr(), b["n"]
        a.g_scale, a.g_out = b["gs"], (t["g_out"].v.data_ptr() if "g_out" in t else None)
    return arr


def adamw_reset(bufs):
    for b in bufs:
        for k, x in zip(("p", "m", "v"), (b["inp"][0], b["inp"][2], b["inp"][3])):
            b["t"][k].fill(x.reshape(1, -1))
        if "g_out" in b["t"]:
            b["t"]["g_out"].fill()


def adamw_check(bufs, state, what, kernel):
    got = []
    for b in bufs:
        p, g, m, v = b["inp"]
        ref = R.adamw(p, g, m, v, state, g_scale=b["gs"], **R.ADAMW)
        res = {k: b["t"][k].get()[0] for k in ("p", "m", "v") + (("g_out",) if "g_out" in b["t"] else ())}
        for k, x in res.items():
            within(x, ref[k][0], ref[k][1], "%s %s (n %d)" % (what, k, b["n"]), kernel)
        b["t"]["g"].check()
        got.append(res)
    return got


def device_state(ops):
    """state3 after one llmrec_adamw_advance, checked against the restated definition bit for bit"""
    from llmrec_amd import _lib
    st = torch.zeros(3, dtype=torch.float32, device=DEV)
    _lib.call("llmrec_adamw_advance", ops._p(st), R.ADAMW["lr"], R.ADAMW["b1"], R.ADAMW["b2"], stream(ops))
    want = R.adamw_state(1, R.ADAMW["lr"], R.ADAMW["b1"], R.ADAMW["b2"])
    same_bits(st.cpu().numpy(), want, "state3 after one advance")
    return st, want


def adamw_args():
    a = R.ADAMW
    return (a["lr"], a["b1"], a["b2"], a["eps"], a["wd"])


@pytest.mark.parametrize("gc", R.group_cases(), ids=lambda g: g.name)
def test_step_rows_group(ops, gc):
    from llmrec_amd import _lib
    d = 64
    case = _contig("fuse_bwd_src_multi", d, (gc.fuse_rows[0],), (gc.fuse_rows[1],))
    fos = [FuseOperands(case, "p%d." % k, gc.fuse_rows[k], k, False) for k in (0, 1)]
    so = SoftmaxOperands(_contig("softmax_bwd", d, (gc.sm_rows,)), gc.sm_rows)
    bufs = [adamw_buffers(n, ("group", i), g_scale=0.25 if i else 1.0, with_gout=bool(i)) for i, n in enumerate(gc.adamw_n)]
    st, state = device_state(ops)
    keep = []
    arr = (ops.FuseBwdProblem * 2)()
    P = {**fos[0].P(), **fos[1].P()}
    for k in (0, 1):
        _bwd_problem(arr[k], P, "p%d." % k, gc.fuse_rows[k], keep)
    ad = adamw_array(ops, bufs)
    sp = so.P(False)
    _lib.call("llmrec_step_rows_group_f32", 2, arr, d, len(bufs), ad, ops._p(st), *adamw_args(),
              gc.sm_rows, d, R.ALPHA, *sp["Y"], *sp["dY"], *sp["dZ"], stream(ops))
    grads = [check_fuse_bwd(fo, r, 4, "source", "group %s fusion %s" % (gc.name, fo.pre), "step_rows_group_kernel (fusion)") for fo, r in zip(fos, gc.fuse_rows)]
    want, bound = R.softmax_bwd(so.Y, so.dY, R.ALPHA, 4)
    dz = so.out["dZ"].get()
    within(dz, want, bound, "group %s softmax" % gc.name, "step_rows_group_kernel (softmax)")
    upd = adamw_check(bufs, state, "group %s AdamW" % gc.name, "step_rows_group_kernel (AdamW)")
    # ... and bit for bit the members' own entry points
    for fo in fos:
        fo.fill()
    so.out["dZ"].fill()
    adamw_reset(bufs)
    ok(launch("fuse_bwd_src_multi", d, gc.fuse_rows, P, stream=stream(ops)))
    ok(launch("softmax_bwd", d, gc.sm_rows, sp, stream=stream(ops)))
    _lib.call("llmrec_adamw_multi_f32", len(bufs), ad, ops._p(st), *adamw_args(), stream(ops))
    for k, fo in enumerate(fos):
        for i in range(R.N_NORM):
            same_bits(grads[k][i], fo.out["d%d" % i].get(), "group %s fusion problem %d term %d against its own entry" % (gc.name, k, i))
    same_bits(dz, so.out["dZ"].get(), "group %s softmax against its own entry" % gc.name)
    for b, res in zip(bufs, upd):
        for k, x in res.items():
            same_bits(x, b["t"][k].get()[0], "group %s AdamW %s against its own entry" % (gc.name, k))
    for fo in fos:
        fo.check()
    so.check()
    for k in ("fusion", "softmax", "AdamW"):
        report("step_rows_group_kernel (%s)" % k)


# ------------------------------------------------------------------------------------------------------------------------------------
# the flat kernels
# ------------------------------------------------------------------------------------------------------------------------------------
def _flat(entry):
    return [c for c in R.flat_cases() if c.entry == entry]


def _id(c):
    return "%s-%dx%d-ld%d" % c


@pytest.mark.parametrize("fc", _flat("sumsq"), ids=_id)
def test_sumsq(ops, fc):
    from llmrec_amd import _lib
    X = R.mixed(fc.rows, fc.d, "sumsq", fc.rows)
    tx = tab((fc.ld, 0, 0), X)
    blocks = R.sumsq_blocks(fc.rows * fc.d)
    ws_bytes = _lib.query("llmrec_sumsq_workspace_bytes", fc.rows, fc.d)
    assert ws_bytes == 4 * R.SUMSQ_BLOCKS
    ws = Out(1, R.SUMSQ_BLOCKS)
    coef, old = 1e-5 * 0.5 / 80, 0.375
    for acc in (None, old):
        out = Out(1, 1, init=np.full((1, 1), old, dtype=np.float32))
        _lib.call("llmrec_sumsq_f32", fc.rows, fc.d, tx.t.data_ptr(), fc.ld, coef, int(acc is not None), out.v.data_ptr(), ws.v.data_ptr(), ws_bytes, stream(ops))
        want, bound = R.sumsq(X, coef, acc, blocks)
        within(out.get()[0], np.array([want]), np.array([bound]), "sumsq %s accumulate %s" % (_id(fc), acc is not None), "sumsq_partial_kernel + sumsq_final_kernel")
        assert (ws.get()[0][blocks:] == R.SENTINEL).all()
    tx.check()
    report("sumsq_partial_kernel + sumsq_final_kernel")


@pytest.mark.parametrize("fc", _flat("axpy"), ids=_id)
def test_axpy(ops, fc):
    from llmrec_amd import _lib
    X, Y0 = R.mixed(fc.rows, fc.d, "axpy", "X", fc.d), R.mixed(fc.rows, fc.d, "axpy", "Y", fc.d)
    tx = tab((fc.ld, 0, 0), X)
    adev = Table("alpha_dev", np.full((1, 1), 0.3, dtype=np.float32), 1, 0, 0, DEV)
    y = Out(fc.rows, fc.d, (fc.ld + 4 if fc.ld == fc.d and fc.rows > 1 else fc.ld, 0, 0))
    for acc in (0, 1):
        for dev_alpha in (None, adev):
            y.fill(Y0)
            _lib.call("llmrec_axpy_f32", fc.rows, fc.d, R.ALPHA, dev_alpha.t.data_ptr() if dev_alpha else None, tx.t.data_ptr(), fc.ld, *y.p, acc, stream(ops))
            want, bound = R.axpy(X, Y0, R.ALPHA, 0.3 if dev_alpha else None, acc)
            within(y.get(), want, bound, "axpy %s accumulate %d" % (_id(fc), acc), "axpy_kernel")
    tx.check(), adev.check()
    report("axpy_kernel")


@pytest.mark.parametrize("fc", _flat("adamw"), ids=_id)
def test_adamw(ops, fc):
    """adamw_kernel and the multi-tensor launch (its float4 chunks, its scalar tail, a misaligned view, g_scale with g_out) against fp64;
    the multi launch with g_scale = 1 bit for bit the single one"""
    from llmrec_amd import _lib
    n = fc.d
    st, state = device_state(ops)
    single = [adamw_buffers(n, ("flat", n))]
    t = single[0]["t"]
    _lib.call("llmrec_adamw_f32", n, t["p"].v.data_ptr(), t["g"].t.data_ptr(), t["m"].v.data_ptr(), t["v"].v.data_ptr(), ops._p(st), *adamw_args(), stream(ops))
    one = adamw_check(single, state, "adamw_f32", "adamw_kernel")[0]
    adamw_reset(single)
    _lib.call("llmrec_adamw_multi_f32", 1, adamw_array(ops, single), ops._p(st), *adamw_args(), stream(ops))
    multi = adamw_check(single, state, "adamw_multi", "adamw_multi_kernel")[0]
    for k in one:
        same_bits(multi[k], one[k], "adamw_multi against adamw_f32: %s" % k)
    scaled = [adamw_buffers(n, ("flat", n), g_scale=0.25, with_gout=True), adamw_buffers(1029, ("flat", "b"), g_scale=-3.0, with_gout=True)]
    _lib.call("llmrec_adamw_multi_f32", 2, adamw_array(ops, scaled), ops._p(st), *adamw_args(), stream(ops))
    adamw_check(scaled, state, "adamw_multi with g_scale", "adamw_multi_kernel")
    report("adamw_kernel"), report("adamw_multi_kernel")


@pytest.mark.parametrize("fc", _flat("scale_rows"), ids=_id)
def test_scale_rows(ops, fc):
    from llmrec_amd import _lib
    X, s = R.mixed(fc.rows, fc.d, "scale", "X", fc.d), R.mixed(fc.rows, 1, "scale", "s", fc.d)
    tx, ts = tab((fc.ld, 0, 0), X), tab((1, 0, 0), s)
    y = Out(fc.rows, fc.d, (fc.ld + 1, 0, 0))
    _lib.call("llmrec_scale_rows_f32", fc.rows, fc.d, ts.t.data_ptr(), tx.t.data_ptr(), fc.ld, *y.p, stream(ops))
    want, bound = R.scale_rows(s[:, 0], X)
    within(y.get(), want, bound, "scale_rows %s" % _id(fc), "scale_rows_kernel")
    tx.check(), ts.check()
    report("scale_rows_kernel")


@pytest.mark.parametrize("fc", _flat("gather_mean"), ids=_id)
def test_gather_mean(ops, fc):
    from llmrec_amd import _lib
    terms = [R.mixed(fc.rows, fc.d, "gather", i, fc.d) for i in range(3)]
    tabs = [tab((fc.ld, 0, 0), x) for x in terms]
    idx = R._rng("gather", "idx", fc.d).integers(0, fc.rows, 33)
    ids = torch.from_numpy(idx.astype(np.int64)).to(DEV)
    pt, pl = (C.c_void_p * 3)(*[t.t.data_ptr() for t in tabs]), (C.c_int64 * 3)(*[fc.ld] * 3)
    out = Out(33, fc.d, (fc.d + 3, 0, 0))
    _lib.call("llmrec_gather_mean_f32", 33, ops._p(ids), fc.d, R.MEAN_SCALE, 3, pt, pl, *out.p, stream(ops))
    want, bound = R.gather_mean(terms, idx, R.MEAN_SCALE)
    within(out.get(), want, bound, "gather_mean %s" % _id(fc), "gather_mean_kernel")
    for t in tabs:
        t.check()
    report("gather_mean_kernel")


@pytest.mark.parametrize("fc", _flat("weighted_colsum"), ids=_id)
def test_weighted_colsum(ops, fc):
    from llmrec_amd import _lib
    n_groups = 3 if fc.d % 64 == 0 else 2
    gw = fc.d // n_groups
    X, w = R.mixed(fc.rows, fc.d, "colsum", "X", fc.d), R.mixed(fc.rows, 1, "colsum", "w", fc.d)
    tx, tw = tab((fc.ld, 0, 0), X), tab((1, 0, 0), w)
    dest = [0, 1, 0][:n_groups]                                   # groups 0 and 2 share a destination
    olds = [R.mixed(1, gw, "colsum", "old", k, fc.d) for k in (0, 1)]
    need = _lib.query("llmrec_weighted_colsum_workspace_bytes", fc.d)
    assert need == 4 * R.COLSUM_BLOCKS * fc.d
    ws = torch.empty(need // 4, dtype=torch.float32, device=DEV)
    for acc in (0, 1):
        for weights in (tw, None):
            outs = [Out(1, gw, init=o) for o in olds]
            table = (C.c_void_p * n_groups)(*[outs[k].v.data_ptr() for k in dest])
            _lib.call("llmrec_weighted_colsum_f32", fc.rows, n_groups, gw, tx.t.data_ptr(), fc.ld, weights.t.data_ptr() if weights else None, table, acc,
                      ops._p(ws), need, stream(ops))
            ref = R.weighted_colsum(X, w[:, 0] if weights else None, n_groups, gw, dest, [o[0] if acc else None for o in olds])
            for k, (want, bound) in ref.items():
                within(outs[k].get()[0], want, bound, "weighted_colsum %s destination %d accumulate %d" % (_id(fc), k, acc), "colsum_partial_kernel + colsum_final_kernel")
    tx.check(), tw.check()
    report("colsum_partial_kernel + colsum_final_kernel")


# ------------------------------------------------------------------------------------------------------------------------------------
# refusals and empty problems
# ------------------------------------------------------------------------------------------------------------------------------------
def _operands(case, rows, rows1):
    """(P, outputs, tables) of any templated entry's case"""
    if case.entry.startswith("softmax"):
        so = SoftmaxOperands(case, rows)
        fwd = case.entry == "softmax_fwd"
        return so.P(fwd), [so.out["Y" if fwd else "dZ"]], [so]
    fwd = "fwd" in case.entry
    if case.rows1:
        fos = [FuseOperands(case, "p%d." % k, r, k, fwd) for k, r in enumerate((rows, rows1))]
    else:
        fos = [FuseOperands(case, "", rows, 0, fwd)]
    P = {}
    for fo in fos:
        P.update(fo.P())
    return P, [o for fo in fos for o in fo.out.values()], fos


@pytest.mark.parametrize("case", R.refusals(), ids=lambda c: c.name)
def test_refusals_return_unsupported_and_write_nothing(ops, case):
    rows, rows1 = case.rows[0], (case.rows1[0] if case.rows1 else None)
    P, outs, holders = _operands(case, rows, rows1)
    n = (rows, rows1) if case.rows1 else rows
    for mode in R.MODES.get(case.entry, (None,)):
        assert case.expect(mode) is None
        extra = {}
        if case.entry == "fuse_fwd_multi_sumsq_compact":
            part, flags = Out(1, 64), torch.zeros(112, dtype=torch.uint8, device=DEV)
            flags[5] = 1
            rl, nr = torch.full((100 + 32,), -7, dtype=torch.int32, device=DEV), torch.full((1,), -1, dtype=torch.int32, device=DEV)
            extra = dict(sumsq=(2, part.v.data_ptr(), 64, C.c_int32(-1)), compact=(100, ops._p(flags), ops._p(rl), ops._p(nr)))
            outs = outs + [part]
        assert launch(case.entry, case.d, n, P, mode=mode, stream=stream(ops), **extra) == R.EUNSUPPORTED
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs)
        if extra:
            assert int(flags[5]) == 1 and int(nr[0]) == -1 and bool((rl == -7).all())
    for h in holders:
        h.check()


@pytest.mark.parametrize("entry", R.TEMPLATED)
def test_no_rows_is_ok_and_writes_nothing(ops, entry):
    case = R.Case(entry, 64, "contig", None, **R._rows(entry, (17,)))
    P, outs, holders = _operands(case, 17, 37 if case.rows1 else None)
    for mode in R.MODES.get(entry, (None,)):
        ok(launch(entry, 64, (0, 0) if case.rows1 else 0, P, mode=mode, stream=stream(ops)))
        torch.cuda.synchronize()
        assert all(o.untouched() for o in outs)
    if case.rows1:                                                # one empty problem beside a live one
        ok(launch(entry, 64, (0, 37), P, stream=stream(ops)))
        torch.cuda.synchronize()
        assert all(o.untouched() for o in holders[0].out.values()) and not any(o.untouched() for o in holders[1].out.values())
    for h in holders:
        h.check()
