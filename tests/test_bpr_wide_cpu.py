"""llmrec_bpr_prune_fwd_wide_f32 without a GPU: the declarations, the workspace query (host arithmetic), the refusals (every argument
is validated before anything is launched) and the selection reference the GPU tests compare with."""
import numpy as np

from llmrec_amd import _lib
from tests import _select_ref as S

FAKE = 0x1000                                                             # a non-null pointer that is never dereferenced: nothing is launched


def test_header_declares_the_wide_entry_points():
    protos = _lib.parse_header()
    assert "llmrec_bpr_prune_wide_workspace_bytes" in protos
    sharded, wide = protos["llmrec_bpr_prune_fwd_sharded_f32"], protos["llmrec_bpr_prune_fwd_wide_f32"]
    assert len(wide[1]) == len(sharded[1]) + 3
    assert set(wide[2]) - set(sharded[2]) == {"n_valid_dev", "workspace", "workspace_bytes"}
    assert _lib.CONST["LLMREC_BPR_WIDE_MAX_B"] == 1 << 22 and _lib.CONST["LLMREC_BPR_MAX_B"] == 4096
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8


def test_workspace_query_is_host_arithmetic():
    q = lambda n: _lib.query("llmrec_bpr_prune_wide_workspace_bytes", n)
    sizes = [0, 1, 4097, 12400, 1 << 16, 1 << 20, _lib.CONST["LLMREC_BPR_WIDE_MAX_B"]]
    got = [q(n) for n in sizes]
    assert all(g > 0 for g in got)
    assert got == sorted(got) and got[-1] > got[0]
    assert q(-1) == -1 and q(_lib.CONST["LLMREC_BPR_WIDE_MAX_B"] + 1) == -1


def _wide(lib, Eu=FAKE, Ei=FAKE, d=64, idx=FAKE, B=5000, global_m=None, global_B=0, offset=0, scores_only=0, out=FAKE, saved=FAKE,
          ws=FAKE, ws_bytes=1 << 20):
    return lib.llmrec_bpr_prune_fwd_wide_f32(Eu, d, Ei, d, d, idx, idx, idx, B, 0.29, 1e-5, 64.0, global_m, global_B, offset, scores_only,
                                             out, saved, None, ws, ws_bytes, None)


def test_wide_entry_refuses_before_it_launches():
    lib = _lib.load()
    cap = _lib.CONST["LLMREC_BPR_WIDE_MAX_B"]
    need = _lib.query("llmrec_bpr_prune_wide_workspace_bytes", 5000)
    cases = [
        ("above the cap (local)", dict(B=cap + 1), _lib.EUNSUPPORTED),
        ("above the cap (global)", dict(global_m=FAKE, global_B=cap + 1), _lib.EUNSUPPORTED),
        ("null tables", dict(Eu=None), -1),
        ("null indices", dict(idx=None), -1),
        ("no output", dict(out=None), -1),
        ("local batch with an offset", dict(offset=5), -1),
        ("local batch with another global size", dict(global_B=9000), -1),
        ("offset outside the list", dict(global_m=FAKE, global_B=9000, offset=4001), -1),
        ("negative offset", dict(global_m=FAKE, global_B=9000, offset=-1), -1),
        ("list shorter than the local batch", dict(global_m=FAKE, global_B=4999), -1),
        ("short workspace", dict(ws_bytes=need - 1), -3),
        ("no workspace", dict(ws=None), -3),
        ("workspace sized for the local batch, not the list", dict(global_m=FAKE, global_B=1 << 20, ws_bytes=need), -3),
    ]
    for what, kw, status in cases:
        assert _wide(lib, **kw) == status, what
        assert b"bpr_fwd_wide" in lib.llmrec_last_error(), (what, lib.llmrec_last_error())
    # the capped entry points keep their limits and their texts
    st = lib.llmrec_bpr_prune_fwd_f32(FAKE, 64, FAKE, 64, 64, FAKE, FAKE, FAKE, 4097, None, 0.29, 1e-5, 64.0, FAKE, FAKE, None)
    assert st == _lib.EUNSUPPORTED and b"bpr_fwd: B_max 4097 > 4096" in lib.llmrec_last_error()
    st = lib.llmrec_bpr_prune_fwd_sharded_f32(FAKE, 64, FAKE, 64, 64, FAKE, FAKE, FAKE, 4096, 0.29, 1e-5, 64.0, FAKE, 12289, 0, 0, FAKE, FAKE, None)
    assert st == _lib.EUNSUPPORTED and b"bpr_fwd_sharded: batch too large" in lib.llmrec_last_error()


def test_ops_route_by_size_only():
    import pytest
    import torch
    from llmrec_amd import ops
    idx = torch.zeros(_lib.CONST["LLMREC_BPR_WIDE_MAX_B"] + 1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="LLMREC_BPR_WIDE_MAX_B"):
        ops.bpr_prune(torch.zeros(4, 8), torch.zeros(4, 8), idx, idx, idx, 0.5, 1e-5, 64)
    idx = torch.zeros(4097, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # past the old refusal: it reaches the device check
        ops.bpr_prune(torch.zeros(4, 8), torch.zeros(4, 8), idx, idx, idx, 0.5, 1e-5, 64)


def test_select_ref_equals_the_brute_force_rank_count():
    rng = np.random.default_rng(7)
    pool = np.array([-np.inf, -3.5, -1.25, -1.25000012, -0.5, -0.0, 0.0, -1e-30], dtype=np.float32)
    m = pool[rng.integers(0, len(pool), size=300)]
    m[:40] = -rng.random(40).astype(np.float32)
    for remember in (0.0, 1e-5, 0.29, 0.5, 0.997, 1.0):
        assert np.array_equal(S.keep_mask(m, remember), S.keep_mask_brute(m, remember)), remember
        assert int(S.keep_mask(m, remember).sum()) == S.k_of(remember, 300)
    keep, coef, kept_m, share = S.expected(m, np.ones(100, dtype=np.float32), 0.29, offset=100)
    assert np.array_equal(keep, S.keep_mask_brute(m, 0.29)[100:200])
    assert np.array_equal(coef[keep], np.full(int(keep.sum()), np.float32(-1.0) / np.float32(S.k_of(0.29, 300))))
    assert not coef[~keep].any() and not kept_m[~keep].any()
