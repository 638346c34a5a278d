"""CPU: the numpy restatement of the fused step's dropout mask (tests/_dropout_ref.py) has the statistics a Bernoulli mask must have,
its threshold and scale are the documented numbers, and llmrec_dropout_rows_f32 is declared, exported and refuses what the header says it
refuses before it touches the device."""
import math

import numpy as np
import pytest

from llmrec_amd import _lib
from tests import _dropout_ref as R

FAKE = 0x10000          # a 16-byte aligned "device" address: argument checks never dereference device pointers
SEED, STEP, TAG = 2022, 5, 0
EINVAL = _lib.CONST["LLMREC_EINVAL"]


@pytest.mark.parametrize("rows,cols,p", [(37, 20, 0.1), (96, 64, 0.9), (1000, 448, 0.5), (17366, 448, 0.3)])
def test_keep_fraction_is_one_minus_p(rows, cols, p):
    n = rows * cols
    kept = int(R.keep_mask(rows, cols, p, SEED, STEP, TAG).sum())
    sigma = math.sqrt(p * (1 - p) / n)
    dev = abs(kept / n - (1 - p))
    print("keep fraction (%d, %d, p = %g): %.6f, %.2f sigma" % (rows, cols, p, kept / n, dev / sigma))
    assert dev <= 5 * sigma, (kept / n, dev / sigma)


@pytest.mark.parametrize("rows,cols,p", [(1000, 448, 0.5), (1000, 448, 0.3), (96, 64, 0.9)])
@pytest.mark.parametrize("other", [dict(tag=1), dict(step=STEP + 1), dict(step=STEP + 2 ** 32), dict(seed=SEED + 1)])
def test_masks_that_differ_in_one_input_are_independent(rows, cols, p, other):
    base = dict(seed=SEED, step=STEP, tag=TAG)
    a = R.keep_mask(rows, cols, p, **base)
    b = R.keep_mask(rows, cols, p, **{**base, **other})
    n = rows * cols
    q = (1 - p) ** 2 + p ** 2                                   # two independent Bernoulli(1 - p) draws agree
    sigma = math.sqrt(q * (1 - q) / n)
    agree = float((a == b).sum()) / n
    print("agreement", other, "p = %g: %.6f, %.2f sigma" % (p, agree, abs(agree - q) / sigma))
    assert abs(agree - q) <= 5 * sigma, (agree, q)


def test_one_call_serves_four_columns_and_rows_and_groups_differ():
    w = R.words(8, 12, SEED, STEP, TAG)
    assert w.dtype == np.uint32 and w.shape == (8, 12)
    assert np.array_equal(w[:, :7], R.words(8, 7, SEED, STEP, TAG))          # a narrower tensor is a prefix: the word depends on (r, c) only
    assert len(np.unique(w)) == w.size                                        # 96 words of 32 bits: a repeat would be a layout mistake


def test_threshold_and_scale_are_the_documented_numbers():
    assert R.threshold(2.0 ** -32) == 1
    assert R.threshold(0.5) == 2 ** 31
    assert R.threshold(1 - 2.0 ** -24) == 2 ** 32 - 256
    assert R.threshold(2.0 ** -40) == 1                                       # the clamp's lower end
    for p, want in ((0.5, 2.0), (0.75, 4.0), (1 - 2.0 ** -24, 2.0 ** 24)):
        assert R.scale(p) == np.float32(want) and R.scale(p).dtype == np.float32
    for p in (0.1, 0.3, 0.9):
        one_minus = np.float32(1.0 - float(np.float32(p)))                    # exact in double, one rounding to fp32
        assert R.scale(p) == np.float32(1.0 / float(one_minus)), p


def test_values_keep_scaled_and_drop_to_plus_zero():
    x = np.array([[-1.5, 0.0, -0.0, np.inf, -np.inf, np.nan, 3.0, 1e-40]], dtype=np.float32).repeat(64, axis=0)
    y = R.apply(x, 0.5, SEED, STEP, TAG)
    keep = R.keep_mask(64, 8, 0.5, SEED, STEP, TAG)
    assert keep.any() and (~keep).any()
    assert np.all(y.view(np.uint32)[~keep] == 0)                              # +0.0, bit for bit, over -0.0, the infinities and the NaN
    with np.errstate(all="ignore"):
        assert np.array_equal(y.view(np.uint32)[keep], (x * np.float32(2.0)).view(np.uint32)[keep])


def test_the_entry_point_is_declared_and_exported_and_the_abi_version_stays():
    protos = _lib.parse_header()
    restype, argtypes, names = protos["llmrec_dropout_rows_f32"]
    assert names == ["rows", "cols", "X", "ldx", "p", "seed", "step_dev", "tensor_tag", "ticket", "stream"]
    lib = _lib.load()
    assert hasattr(lib, "llmrec_dropout_rows_f32")
    assert lib.llmrec_abi_version() == 8 and _lib.CONST["LLMREC_ABI_VERSION"] == 8


def test_the_entry_point_refuses_bad_arguments_without_a_device():
    lib = _lib.load()
    call = lib.llmrec_dropout_rows_f32
    # (rows, cols, X, ldx, p, seed, step_dev, tag, ticket, stream). rows = 0 is a success once the scalar arguments are valid, so a bad
    # scalar beside rows = 0 and null pointers shows that scalar's own check - and nothing can be launched
    assert call(0, 8, None, 8, 0.5, 1, None, 0, None, None) == 0
    for p in (0.0, 1.0, -0.25, 1.5, float("nan"), float("inf")):
        assert call(0, 8, None, 8, p, 1, None, 0, None, None) == EINVAL, p
        assert b"dropout_rows: p" in lib.llmrec_last_error()
    for cols in (0, -3):
        assert call(0, cols, None, 8, 0.5, 1, None, 0, None, None) == EINVAL, cols
        assert b"dropout_rows: bad sizes" in lib.llmrec_last_error()
    for tag in (-1, 256, 1 << 20):
        assert call(0, 8, None, 8, 0.5, 1, None, tag, None, None) == EINVAL, tag
        assert b"dropout_rows: tensor_tag" in lib.llmrec_last_error()
    for rows in (1 << 32, (1 << 40) + 7, -1):
        assert call(rows, 8, None, 8, 0.5, 1, None, 0, None, None) == EINVAL, rows
        assert b"dropout_rows: bad sizes" in lib.llmrec_last_error()
    # rows > 0: null pointers, a leading dimension below cols, a base that is not 4-byte aligned
    for X, ldx, step in ((None, 8, FAKE), (FAKE, 8, None), (None, 8, None), (FAKE, 7, FAKE), (FAKE + 2, 8, FAKE)):
        assert call(4, 8, X, ldx, 0.5, 1, step, 0, None, None) == EINVAL, (X, ldx, step)
        assert b"dropout_rows:" in lib.llmrec_last_error()
