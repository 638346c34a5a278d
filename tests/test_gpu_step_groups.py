"""GPU: the one-stream step's grouped row launches against the launches they replace, bit for bit, through the C ABI.

  * the wide (float4) path of the multi-tensor AdamW (llmrec_adamw_multi_f32 / llmrec_adamw_multi_zero_rows_f32) against the single-tensor
    llmrec_adamw_f32: sizes around the float4 width and the chunk, a misaligned view (4-byte path), a scaled gradient with g_out, the
    row clean-up riding in the same launch;
  * llmrec_step_rows_group_f32 (fusion backward + AdamW + softmax backward in one launch) against its three entry points, with every
    member absent in turn, with and without stamped row flags, and its refusal of d = 128."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR, B1, B2, EPS, WD = 1e-3, 0.9, 0.999, 1e-8, 0.01


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from llmrec_amd import ops as _ops
    return _ops


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------
# wide AdamW
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_cleanup", [False, True])
def test_multi_tensor_adamw_equals_the_single_tensor_kernel(ops, with_cleanup):
    from llmrec_amd import _lib
    from llmrec_amd.ops import _p, AdamwTensor, ZeroRowsJob
    chunk = _lib.CONST["LLMREC_ADAMW_CHUNK"]
    g = torch.Generator(device=DEV); g.manual_seed(8)
    rn = lambda n: torch.randn(n, generator=g, device=DEV)
    sizes = [1, 3, 4, 4095, 4096, 4097, 2 * chunk + 5]
    # (n, offset in floats into the storage, g_scale, store g_out)
    specs = [(n, 0, 1.0, False) for n in sizes] + [(3 * chunk + 2, 1, 1.0, False), (2 * chunk + 5, 0, 0.25, True), (chunk, 0, 3.0, True)]
    tens = []
    for n, off, gs, gout in specs:
        mk = lambda src: (torch.zeros(n + 4, device=DEV)[off:off + n].copy_(src))        # the view starts `off` floats into a 16-byte aligned block
        p0 = rn(n)
        t = {"n": n, "gs": gs, "p": mk(p0), "m": mk(torch.zeros(n, device=DEV)), "v": mk(torch.zeros(n, device=DEV)), "g": mk(rn(n)),
             "gout": mk(torch.full((n,), 7.0, device=DEV)) if gout else None,
             "rp": p0.clone(), "rm": torch.zeros(n, device=DEV), "rv": torch.zeros(n, device=DEV)}
        assert (t["p"].data_ptr() % 16 == 0) == (off == 0)
        tens.append(t)
    arr = (AdamwTensor * len(tens))()
    for a, t in zip(arr, tens):
        a.p, a.g, a.m, a.v, a.n, a.g_scale = t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["n"], t["gs"]
        a.g_out = t["gout"].data_ptr() if t["gout"] is not None else None
    # the clean-up riding along: two jobs of 40 listed rows, 29 of them valid
    cap, valid, rows, width = 40, 29, 97, 24
    ids = [torch.randperm(rows, generator=g, device=DEV)[:cap].contiguous() for _ in range(2)]
    dst = [torch.ones(rows, 2 * width, device=DEV) for _ in range(2)]
    n_valid = torch.tensor([valid], dtype=torch.int32, device=DEV)
    jobs = (ZeroRowsJob * 2)()
    for j in range(2):
        jobs[j].ids, jobs[j].dst, jobs[j].ldd, jobs[j].d = ids[j].data_ptr(), dst[j][:, width:].data_ptr(), 2 * width, width
    state = torch.zeros(3, device=DEV)
    for step in range(3):
        _lib.call("llmrec_adamw_advance", _p(state), LR, B1, B2, None)
        for t in tens:
            t["g"].copy_(rn(t["n"]))
            ref_g = t["g"] * t["gs"] if t["gs"] != 1.0 else t["g"].clone()           # one fp32 product per element, as the kernel's g_scale * g
            t["ref_g"] = ref_g
            _lib.call("llmrec_adamw_f32", t["n"], _p(t["rp"]), _p(ref_g), _p(t["rm"]), _p(t["rv"]), _p(state), LR, B1, B2, EPS, WD, None)
        if with_cleanup:
            for x in dst:
                x.fill_(1.0)
            _lib.call("llmrec_adamw_multi_zero_rows_f32", len(tens), arr, _p(state), LR, B1, B2, EPS, WD, 2, jobs, cap, _p(n_valid), None)
        else:
            _lib.call("llmrec_adamw_multi_f32", len(tens), arr, _p(state), LR, B1, B2, EPS, WD, None)
        torch.cuda.synchronize()
        for t in tens:
            key = (step, t["n"], t["gs"])
            assert _same(t["p"], t["rp"]) and _same(t["m"], t["rm"]) and _same(t["v"], t["rv"]), key
            if t["gout"] is not None:
                assert _same(t["gout"], t["ref_g"]), key
        if with_cleanup:
            for j in range(2):
                want = torch.ones(rows, 2 * width, device=DEV)
                want[ids[j][:valid], width:] = 0.0
                assert torch.equal(dst[j], want), (step, j)


# ---------------------------------------------------------------------------------------------
# fusion backward + AdamW + softmax backward in one launch
# ---------------------------------------------------------------------------------------------
def _tab(ts):
    from llmrec_amd.ops import _ld
    return ((C.c_void_p * len(ts))(*[t.data_ptr() if t is not None else None for t in ts]),
            (C.c_int64 * len(ts))(*[_ld(t) if t is not None else 0 for t in ts]))


class _RowsCase:
    """The three members' inputs at U = 300, I = 420 with 7 side streams, and two sets of outputs (grouped / separate launches)."""

    def __init__(self, d, flags):
        from llmrec_amd import _lib
        from llmrec_amd.ops import _p, AdamwTensor, FuseBwdProblem
        g = torch.Generator(device=DEV); g.manual_seed(23)
        rn = lambda *s: torch.randn(*s, generator=g, device=DEV)
        U, I, S = 300, 420, 7
        self.d, self.keep = d, []
        self.state = torch.zeros(3, device=DEV)
        _lib.call("llmrec_adamw_advance", _p(self.state), LR, B1, B2, None)
        self.counter = torch.tensor([4 + 255], dtype=torch.int32, device=DEV)        # active = 4 % 255 + 1 ... see LLMREC_ROW_STAMP
        active = int(self.counter.item()) % 255 + 1
        self.sides = []
        for rows in (I, U):                                                              # (problem 0 = items, 1 = users, as the step has them)
            cat = rn(rows, S * d); cat[5] = 0.0
            dout = rn(rows, d)
            srcs = [rn(rows, d) if k != 2 else None for k in range(S)]
            touched = torch.rand(rows, generator=g, device=DEV) < 0.3
            touched[5] = True
            if flags:                                                                    # untouched rows: zero dOut and zero sources, a stale stamp
                dout[~touched] = 0.0
                for t in srcs:
                    if t is not None:
                        t[~touched] = 0.0
            fl = torch.where(touched, torch.full((rows,), active, device=DEV), torch.full((rows,), 3, device=DEV)).to(torch.uint8).contiguous()
            self.sides.append({"rows": rows, "norms": [cat[:, k * d:(k + 1) * d] for k in range(S)], "dout": dout, "srcs": srcs,
                               "rates": (C.c_float * S)(*[0.05 * (k + 1) for k in range(S)]), "flags": fl if flags else None})
        dE_i, dE_u = self.sides[0]["dout"], self.sides[1]["dout"]
        self.Y = torch.softmax(rn(I, d), dim=1)
        self.table0, self.grad = rn(U, d), dE_u
        self.alpha = 1.0 / 3.0
        self.dE_i = dE_i
        self.FuseBwdProblem, self.AdamwTensor, self._lib, self._p = FuseBwdProblem, AdamwTensor, _lib, _p

    def outputs(self):
        d = self.d
        return {"fuse": [[torch.full((sd["rows"], d), 7.0, device=DEV) for _ in sd["norms"]] for sd in self.sides],
                "p": self.table0.clone(), "m": torch.full_like(self.table0, 0.5), "v": torch.full_like(self.table0, 0.25),
                "gout": torch.full_like(self.table0, 7.0), "dZ": torch.full_like(self.Y, 7.0)}

    @staticmethod
    def flat(o):
        return [t for side in o["fuse"] for t in side] + [o["p"], o["m"], o["v"], o["gout"], o["dZ"]]

    def args(self, o):
        fuse = (self.FuseBwdProblem * 2)()
        for pr, sd, dm in zip(fuse, self.sides, o["fuse"]):
            npt, nl = _tab(sd["norms"]); dp, dl = _tab(dm); sp, sl = _tab(sd["srcs"]); self.keep += [npt, nl, dp, dl, sp, sl]
            pr.rows, pr.dOut, pr.lddo, pr.n_norm = sd["rows"], sd["dout"].data_ptr(), self.d, len(sd["norms"])
            pr.norm_terms, pr.norm_ld, pr.rates = C.cast(npt, C.c_void_p), C.cast(nl, C.c_void_p), C.cast(sd["rates"], C.c_void_p)
            pr.d_terms, pr.d_ld, pr.src_terms, pr.src_ld = C.cast(dp, C.c_void_p), C.cast(dl, C.c_void_p), C.cast(sp, C.c_void_p), C.cast(sl, C.c_void_p)
            pr.n_reg_terms, pr.reg_two_coef = 2, 0.01
            if sd["flags"] is not None:
                pr.row_flags, pr.row_stamp = sd["flags"].data_ptr(), self.counter.data_ptr()
        ten = (self.AdamwTensor * 1)()
        ten[0].p, ten[0].g, ten[0].m, ten[0].v, ten[0].n = o["p"].data_ptr(), self.grad.data_ptr(), o["m"].data_ptr(), o["v"].data_ptr(), o["p"].numel()
        ten[0].g_scale, ten[0].g_out = self.alpha, o["gout"].data_ptr()
        p = self._p
        sm = (self.Y.shape[0], self.d, self.alpha, p(self.Y), self.d, p(self.dE_i), self.d, p(o["dZ"]), self.d)
        return fuse, ten, sm

    def grouped(self, o, absent=None):
        fuse, ten, sm = self.args(o)
        if absent == "softmax":
            sm = (0, 0, 1.0, None, 0, None, 0, None, 0)
        return self._lib.call_unless_unsupported(
            "llmrec_step_rows_group_f32", 0 if absent == "fuse" else 2, None if absent == "fuse" else fuse, self.d,
            0 if absent == "adamw" else 1, None if absent == "adamw" else ten, self._p(self.state), LR, B1, B2, EPS, WD, *sm, None)

    def separate(self, o, absent=None):
        fuse, ten, sm = self.args(o)
        if absent != "fuse":
            self._lib.call("llmrec_fuse_bwd_src_multi_f32", 2, fuse, self.d, None)
        if absent != "adamw":
            self._lib.call("llmrec_adamw_multi_f32", 1, ten, self._p(self.state), LR, B1, B2, EPS, WD, None)
        if absent != "softmax":
            self._lib.call("llmrec_softmax_rows_bwd_scaled_f32", *sm, None)


@pytest.mark.parametrize("flags", [False, True])
@pytest.mark.parametrize("absent", [None, "fuse", "adamw", "softmax"])
def test_rows_group_equals_its_three_launches(ops, absent, flags):
    case = _RowsCase(64, flags)
    got, want = case.outputs(), case.outputs()
    assert case.grouped(got, absent) is True
    case.separate(want, absent)
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(case.flat(got), case.flat(want))):
        assert _same(a, b), (absent, flags, k)
    if absent is None:                                      # (the members did write: nothing above compared 7.0 with 7.0)
        assert all(not bool((t == 7.0).all()) for t in case.flat(got))


def test_rows_group_refuses_rows_wider_than_64_without_launching(ops):
    case = _RowsCase(128, False)
    got = case.outputs()
    before = [t.clone() for t in case.flat(got)]
    assert case.grouped(got) is False                       # LLMREC_EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(case.flat(got), before))
    want = case.outputs()                                   # the three launches the caller then issues do run at d = 128
    case.separate(want)
    torch.cuda.synchronize()
    assert all(not _same(a, b) for a, b in zip(case.flat(want), before))
