"""CPU: the one-wavefront walk of the 1024-slot sum tree (llmrec_bpr_multi_losses_assemble_f32) performs the additions of the LDS
tree (bpr_reduce_kernel, block_tree_sum) on the same operands - float32 restatements of both agree bit for bit; and the entry point
still checks its arguments before it touches the device."""
import numpy as np
import pytest

from llmrec_amd import _lib
from tests._tree_ref import tree_lds, tree_wave

FAKE = 0x10000          # a 16-byte aligned "device" address: argument checks never dereference device pointers


def _mixed(rng, n):
    """magnitudes from 1e-6 to 1e4, both signs: a changed addition order changes the float32 sum"""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 4, size=n)).astype(np.float32)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 1126, 3000, 4096])
def test_wave_tree_equals_lds_tree_bit_for_bit(n):
    rng = np.random.default_rng(1000 + n)
    for _ in range(4):
        x = _mixed(rng, n)
        a, b = np.float32(tree_lds(x)), np.float32(tree_wave(x))
        assert a.view(np.uint32) == b.view(np.uint32), (n, a, b)
    x = np.abs(_mixed(rng, n))                                          # the squared norms' columns are non-negative
    assert np.float32(tree_lds(x)).view(np.uint32) == np.float32(tree_wave(x)).view(np.uint32)


def test_the_trees_are_order_sensitive_on_this_data():
    """the check above can fail: on the same data another association of the same operands gives other bits"""
    rng = np.random.default_rng(5)
    differ = 0
    for _ in range(8):
        x = _mixed(rng, 1126)
        differ += int(np.float32(tree_lds(x)).view(np.uint32) != np.float32(tree_lds(rng.permutation(x))).view(np.uint32))
    assert differ >= 4, differ


def test_losses_assemble_checks_its_arguments_without_a_device():
    import ctypes as C
    lib = _lib.load()
    call = lib.llmrec_bpr_multi_losses_assemble_f32
    w = (C.c_float * 8)(*[1.0] * 8)
    assert len(_lib.parse_header()["llmrec_bpr_multi_losses_assemble_f32"][1]) == 15
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8
    bad = [
        (0, 64, None, 0.5, 1e-5, 64.0, FAKE, FAKE, w, None, 0, 0.0, FAKE, None),            # no problem
        (9, 64, None, 0.5, 1e-5, 64.0, FAKE, FAKE, w, None, 0, 0.0, FAKE, None),            # more than LLMREC_BPR_MAX_PROBLEMS
        (1, -1, None, 0.5, 1e-5, 64.0, FAKE, FAKE, w, None, 0, 0.0, FAKE, None),            # negative capacity
        (1, 64, None, 0.5, 1e-5, 64.0, None, FAKE, w, None, 0, 0.0, FAKE, None),            # no out
        (1, 64, None, 0.5, 1e-5, 64.0, FAKE, FAKE, None, None, 0, 0.0, FAKE, None),         # no weights
        (1, 64, None, 0.5, 1e-5, 64.0, FAKE, FAKE, w, None, 5, 0.0, FAKE, None),            # partial sums announced, none given
        (1, 64, None, 0.5, 1e-5, 64.0, FAKE, FAKE, w, FAKE, -1, 0.0, FAKE, None),           # negative count
    ]
    for args in bad:
        assert call(*args, None) == -1, args
        assert b"bpr_multi_losses_assemble" in lib.llmrec_last_error()
    assert call(1, _lib.CONST["LLMREC_BPR_MAX_B"] + 1, None, 0.5, 1e-5, 64.0, FAKE, FAKE, w, None, 0, 0.0, FAKE, None, None) == _lib.EUNSUPPORTED
