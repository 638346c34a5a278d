"""No GPU: the bf16-row SpMM (llmrec_spmm_xbf16_f32, llmrec_rows_to_bf16) up to its launches - the ABI, every refusal (status code +
llmrec_last_error naming the entry point, nothing launched), the opt-in switch of ShardedFusedID - and the yardstick of
tests/test_gpu_spmm_bf16.py (tests/_spmm_bf16_ref.py): sound for a legitimate fp32 summation over the bf16 rows, broken by a kernel
that gathered the fp32 rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from llmrec_amd import _lib, ops
from tests import _spmm_bf16_ref as B
from tests import _spmm_ref as R

FAKE = 0x7f0000000000
EINVAL, EUNSUPPORTED = -1, _lib.EUNSUPPORTED
NAME = b"spmm_xbf16"


def test_the_header_declares_both_entry_points_and_the_library_exports_them():
    protos = _lib.parse_header()
    assert len(protos["llmrec_rows_to_bf16"][1]) == 8 and len(protos["llmrec_spmm_xbf16_f32"][1]) == 18
    assert protos["llmrec_spmm_xbf16_f32"][2][7:13] == ["Xb", "ldxb", "Y", "ldy", "Yb", "ldyb"]
    lib = _lib.load()
    assert lib.llmrec_rows_to_bf16 and lib.llmrec_spmm_xbf16_f32
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8 and lib.llmrec_abi_version() == 8          # additive: the ABI version stays


def _call(lib, d=64, ldxb=None, ldy=None, Xb=FAKE, Y=FAKE + 0x100000, Yb=None, ldyb=0, epi=None, plan=True, rowptr=FAKE, n_rows=100, partials=None):
    pl = ops.SpmmPlanC(64, 128, 128, 0, None, 0, None, 0, None, None, 0, None, 0, None)
    return lib.llmrec_spmm_xbf16_f32(n_rows, 2200, rowptr, FAKE, None, None, None, Xb, d if ldxb is None else ldxb, Y, d if ldy is None else ldy,
                                     Yb, ldyb, d, C.addressof(pl) if plan else None, partials, C.addressof(epi) if epi is not None else None, None)


def test_every_refusal_returns_its_status_and_names_the_entry_point():
    lib = _lib.load()
    E = ops.SpmmEpilogueC
    unsupported = [dict(d=260), dict(d=1024), dict(d=62), dict(d=15), dict(d=1),
                   dict(epi=E(x_row_mask=FAKE, x_mask_active=7)), dict(epi=E(x_row_mask=FAKE, x_mask_active=7, y_row_flag=FAKE)),
                   dict(epi=E(z_row_flag=FAKE)), dict(epi=E(x_row_mask=FAKE, x_mask_active=7, y_row_gate=FAKE)),
                   dict(epi=E(y_row_needed=FAKE, x_mask_active=7)), dict(epi=E(rows_listed_only=1)),
                   dict(epi=E(x_row_mask=FAKE, x_mask_stamp=FAKE, mask_from_slice=0))]
    for kw in unsupported:
        assert _call(lib, **kw) == EUNSUPPORTED, (kw, lib.llmrec_last_error())
        assert NAME in lib.llmrec_last_error(), (kw, lib.llmrec_last_error())
    invalid = [dict(n_rows=-1), dict(Xb=None), dict(Y=None), dict(rowptr=None), dict(ldxb=60), dict(ldy=60), dict(plan=False),
               dict(ldxb=66),                                  # rows of Xb not 8-byte aligned
               dict(Xb=FAKE + 2), dict(Xb=FAKE + 4),
               dict(Yb=FAKE + 0x200000, ldyb=60), dict(Yb=FAKE + 0x200000, ldyb=66), dict(Yb=FAKE + 0x200004, ldyb=64),
               dict(Yb=FAKE + 64, ldyb=64),                    # Yb inside Xb
               dict(Y=FAKE + 0x100004), dict(ldy=65),          # the fp32 operands as the vector path needs them
               dict(epi=E(op=ops.EPI_NONE, alpha=1.0, Z=FAKE + 0x300004, ldz=64)), dict(epi=E(op=ops.EPI_NONE, alpha=1.0, Z=FAKE + 0x300000, ldz=63)),
               dict(epi=E(op=ops.EPI_SOFTMAX_BWD)),            # no S
               dict(epi=E(op=3))]
    for kw in invalid:
        assert _call(lib, **kw) == EINVAL, (kw, lib.llmrec_last_error())
        assert NAME in lib.llmrec_last_error(), (kw, lib.llmrec_last_error())
    # nothing to do is not an error, and launches nothing
    assert _call(lib, n_rows=0) == 0 and _call(lib, d=0) == 0
    # llmrec_rows_to_bf16
    assert lib.llmrec_rows_to_bf16(4, 8, None, None, 8, FAKE, 8, None) == EINVAL and b"rows_to_bf16" in lib.llmrec_last_error()
    assert lib.llmrec_rows_to_bf16(4, 8, None, FAKE, 8, None, 8, None) == EINVAL and b"rows_to_bf16" in lib.llmrec_last_error()
    assert lib.llmrec_rows_to_bf16(4, 8, None, FAKE, 7, FAKE + 0x1000, 8, None) == EINVAL and b"rows_to_bf16" in lib.llmrec_last_error()
    assert lib.llmrec_rows_to_bf16(-1, 8, None, FAKE, 8, FAKE + 0x1000, 8, None) == EINVAL
    assert lib.llmrec_rows_to_bf16(0, 8, None, None, 8, None, 8, None) == 0


def test_ops_refuse_cpu_tensors():
    a = ops.Csr(2, 2, torch.zeros(3, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), None, None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rows_to_bf16(torch.zeros(4, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.spmm_bf16(a, torch.zeros(2, 8, dtype=torch.bfloat16))


def test_sharded_step_switch():
    """gather_dtype: only fp32 / bf16; bf16 needs a backend with the bf16-row product (the CPU stand-in has none) and a width the kernel has;
    None reads LLMREC_GATHER_DTYPE. All refused at construction, before anything is allocated."""
    from llmrec_amd import dist as ld
    from llmrec_amd.dist_fused import ShardedFusedID
    from tests._cpu_backend import CpuBackend
    comm, be = ld.Comm(), CpuBackend()
    rng = np.random.default_rng(0)
    key = np.unique(rng.integers(0, 30, size=200) * 20 + rng.integers(0, 20, size=200))
    g = ld.ShardedGraph.build(torch.tensor(key // 20), torch.tensor(key % 20), 30, 20, 0, comm, be)
    mk = lambda backend=be, d=8, **kw: ShardedFusedID(g, comm, backend, d, 2, 30, seed=1, lr=1e-3, batch_local=4, drop_rate=0.0, decay=1e-5, **kw)
    assert not getattr(be, "supports_bf16_gather", False)
    with pytest.raises(RuntimeError, match="supports_bf16_gather"):
        mk(gather_dtype="bf16")
    with pytest.raises(ValueError, match="gather_dtype"):
        mk(gather_dtype="fp16")
    st = mk()
    assert st.gather_dtype == "fp32" and st.Ub is None and st.Ib is None and st.message_bytes_per_step()["bf16_shadow_bytes"] == 0
    assert mk(gather_dtype="fp32").gather_dtype == "fp32"
    import os
    old = os.environ.get("LLMREC_GATHER_DTYPE")
    try:
        os.environ["LLMREC_GATHER_DTYPE"] = "bf16"
        with pytest.raises(RuntimeError, match="supports_bf16_gather"):
            mk()
        assert mk(gather_dtype="fp32").gather_dtype == "fp32"            # the argument wins over the variable
        os.environ["LLMREC_GATHER_DTYPE"] = "half"
        with pytest.raises(ValueError, match="gather_dtype"):
            mk()
    finally:
        if old is None:
            os.environ.pop("LLMREC_GATHER_DTYPE", None)
        else:
            os.environ["LLMREC_GATHER_DTYPE"] = old

    class Claims(CpuBackend):                                               # a backend with the product, asked for a width it lacks
        supports_bf16_gather = True
        bf16_gather_refusal = ld.HipBackend.bf16_gather_refusal
        ops = ops
    assert ld.HipBackend.supports_bf16_gather
    for d in (6, 260):
        with pytest.raises(RuntimeError, match="d = %d" % d):
            mk(backend=Claims(), d=d, gather_dtype="bf16")


def test_torch_rounds_to_bf16_as_the_kernels_bit_formula_does():
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    bits[:8] = [0x3f808000, 0x3f818000, 0x3f807fff, 0x3f808001, 0x00000001, 0x80008000, 0x7f7fffff, 0x7f800000]   # ties, subnormals, overflow
    x = bits.view(np.float32)
    finite = np.isfinite(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = B.rn_bf16_bits(x)
    assert np.array_equal(got[finite], want[finite]) and int(finite.sum()) > (1 << 20) * 0.99
    nan = np.isnan(x)
    assert nan.any() and np.all(np.isnan(B.widen(got[nan]))) and np.array_equal(got[np.isinf(x)], want[np.isinf(x)])
    assert np.array_equal(B.round_bf16(B.round_bf16(x[finite])), B.round_bf16(x[finite]))           # idempotent: widen is exact


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("kind", B.KINDS)
def test_the_bound_holds_for_an_fp32_chain_and_tells_the_gathers_apart(d, kind):
    """The (deg + 6) u bound on the rounded operand. A sequential NumPy fp32 chain over the bf16 rows is inside it everywhere - the plain
    product's at 0.12 of the bound (0.12006, in a row of 2 nnz: short rows have the tightest bound), the weighted one's at 0.22 / 0.28.
    The same chain over the fp32 rows - what a kernel that wrongly gathered X instead of Xb would compute - breaks it in 93 of the 94
    non-empty rows (plain; weighted: 93 and 94): the check on the GPU tells the two gathers apart."""
    case = R.Case(d, kind, "none", False, "buckets")
    want, bound, relative = B.reference(case)
    assert not relative
    deg = R.graph()[2]
    assert int((deg > 0).sum()) == 94
    good = B.fp32_chain(case, B.rounded_x(d))
    assert not B.rows_out_of_bound(good, want, bound).any()
    ratio = B.worst_ratio(good, want, bound)
    assert round(ratio, 2) <= (0.12 if kind == "pattern_rs" else 0.28), ratio
    assert np.all(good[deg == 0] == 0.0) and np.all(bound[deg == 0] == 0.0)
    impostor = B.fp32_chain(case, R.width_inputs(d)[0])
    out = B.rows_out_of_bound(impostor, want, bound)
    assert (int(out.sum()) == 93 if kind == "pattern_rs" else int(out.sum()) >= 93) and not out[deg == 0].any(), int(out.sum())


def test_the_case_table_reaches_every_family_plan_and_epilogue():
    cases = B.cases()
    assert len(cases) == len(set(cases)) and 70 <= len(cases) <= 90, len(cases)
    fam = {R.family_and_variant(c) for c in cases}
    assert fam == {(f, v) for f in range(5) for v in ("plain", "weighted")}
    assert {c.d for c in cases} == set(B.WIDTHS)
    for d in B.EPILOGUE_WIDTHS:
        for kind in B.KINDS:
            assert {(c.op, c.post) for c in cases if c.d == d and c.kind == kind} == set(R.EPILOGUES)
    for d in B.PLAN_WIDTHS:
        assert {(c.plan, c.permuted) for c in cases if c.d == d and c.kind == "pattern_rs"} >= {(p, q) for p in R.TRIPLES for q in (False, True)}
        assert {c.plan for c in cases if c.d == d and c.kind == "val_cs"} == set(R.TRIPLES)


@pytest.mark.parametrize("D,n_aug", B.STEP_CASES)
@pytest.mark.parametrize("sparse_forward", [True, False])
def test_the_recorded_loss_deviation_of_the_rounded_oracle(D, n_aug, sparse_forward):
    """STEP_DEVIATION (the figure the GPU test's gate is four times of) is what the oracle's loop gives with the gathered operands rounded."""
    for world in (1, 2):
        if (D, n_aug, sparse_forward, world) not in B.STEP_DEVIATION:
            continue
        rec = B.STEP_DEVIATION[(D, n_aug, sparse_forward, world)]
        got = B.step_deviation(D, n_aug, sparse_forward, world)
        assert 0.5 * rec <= got <= 2.0 * rec, (got, rec)
        assert 1e-6 < rec < 1e-4                                              # units of the loss's sixth digit
    if (D, sparse_forward) == (64, False):
        rec = B.STEP_DEVIATION[(D, n_aug, False, 1, "dense backward")]
        assert 0.5 * rec <= B.step_deviation(D, n_aug, False, 1, sparse_backward=False) <= 2.0 * rec
