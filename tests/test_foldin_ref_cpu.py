"""CPU: the yardstick of the fold-in kernel checks itself (tests/_foldin_ref.py), the host normalisation of item histories
(llmrec_amd.serve.history_csr) and recommend.py's --histories flag. No device."""
import numpy as np
import pytest
import torch

from tests import _foldin_ref as R

MUTANTS = ("no_softmax", "deg_plus_1", "swap_profile_image", "mean_without_layer0")


def _worst(got, ref, bound):
    return float((np.abs(got.astype(np.float64) - ref) / bound).max())


@pytest.fixture(scope="module")
def emulated():
    """{(d, L, n_attr): (case, reference, bound, the emulated sums)} - computed once for the module"""
    out = {}
    for key in R.cases():
        c = R.case(*key)
        sums = R.gathered(c.T, c.rows)
        ref, bound = R.reference(c.T, c.rows, c.w, c.id_rows, c.L, c.n_attr, c.d, R.RATES, sums)
        out[key] = (c, ref, bound, R.emu_sums(c.T, c.rows), sums)
    return out


def test_the_case_table_is_what_the_tests_say_it_is():
    assert len(R.cases()) == 24 and set(R.PATH) == set(R.LENGTHS)
    c = R.case(20, 2, 5)
    lens = [len(h) for h in c.rows]
    assert len(c.rows) == R.N_ROWS == 203 and set(lens) == set(R.LENGTHS)
    for n, path in R.PATH.items():                                 # every length lands in the path the table names, more than once
        assert (R.nseg(n) == 1) == (path == "one") and lens.count(n) >= 22
    full = [h for h in c.rows if len(h) == R.N_ITEMS]
    assert all(np.array_equal(np.sort(h), np.arange(R.N_ITEMS)) for h in full)                     # every item once
    assert all(len(np.unique(h)) < 5000 for h in c.rows if len(h) == 5000)                          # repeats
    bad = c.rows[R.SPRINKLED_ROW]
    assert (bad == -1).sum() == 3 and (bad == R.N_ITEMS).sum() == 1 and (bad == R.N_ITEMS + 5).sum() == 1
    assert c.rowptr[-1] == c.colidx.size == sum(lens) and c.T.shape == (R.N_ITEMS, R.n_slices(2, 5) * 20)
    assert np.array_equal(c.w[:3], R.row_scale([0, 1, 2])) and c.w[0] == np.float32(1e4) and c.w[1] == 1.0


def test_the_emulation_stays_inside_the_bound(emulated):
    worst = {}
    for key, (c, ref, bound, S, sums) in emulated.items():
        assert (bound > 0).all() and np.isfinite(bound).all() and np.isfinite(ref).all()
        for ids in (c.id_rows, None):
            r, b = (ref, bound) if ids is not None else R.reference(c.T, c.rows, c.w, None, c.L, c.n_attr, c.d, R.RATES, sums)
            got = R.emulate(c.T, c.rows, c.w, ids, c.L, c.n_attr, c.d, R.RATES, S=S)
            worst[c.name, ids is not None] = _worst(got, r, b)
    print("worst |emulation - fp64| / bound per case:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def test_the_special_rows_do_what_they_are_there_for(emulated):
    c, ref, bound, S, sums = emulated[(64, 2, 5)]
    G = c.w[:, None].astype(np.float64) * sums[0]
    sl = lambda k: G[:, k * c.d:(k + 1) * c.d]
    assert (np.sqrt((sl(c.tiny_slice) ** 2).sum(1)) < 1e-13).all()                                  # the text term takes the clamp in every row
    assert (np.sqrt((sl(c.L) ** 2).sum(1))[[len(h) > 0 for h in c.rows]] > 1e-3).all()              # the image term does not
    logits = sl(c.L - 1)[R.HOT_ROW]
    assert logits.max() - logits.min() > 20                                                          # large logits
    empty = [r for r, h in enumerate(c.rows) if len(h) == 0]
    want = (c.id_rows[empty].astype(np.float64) + 1.0 / c.d) / (c.L + 1)                            # zero sums, a uniform softmax row
    assert np.allclose(ref[empty], want, rtol=0, atol=1e-15)
    # the entries that add nothing add nothing: the sprinkled row equals the row without them
    h = c.rows[R.SPRINKLED_ROW]
    clean = h[(h >= 0) & (h < R.N_ITEMS)]
    a = R.reference(c.T, [h], c.w[[R.SPRINKLED_ROW]], None, c.L, c.n_attr, c.d, R.RATES)[0]
    b = R.reference(c.T, [clean], c.w[[R.SPRINKLED_ROW]], None, c.L, c.n_attr, c.d, R.RATES)[0]
    assert len(clean) == 60 and np.array_equal(a, b)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_wrong_kernel_falls_outside_the_bound(emulated, mutant):
    """the bound is not vacuous: each deliberately wrong variant leaves it on the case table"""
    out = {}
    for key in ((64, 2, 5), (20, 1, 0), (7, 3, 5)):
        c, ref, bound, S, _ = emulated[key]
        got = R.emulate(c.T, c.rows, c.w, c.id_rows, c.L, c.n_attr, c.d, R.RATES, mutant=mutant, S=S)
        out[c.name] = _worst(got, ref, bound)
    assert max(out.values()) > 10.0, out


def test_history_normalisation_on_the_host():
    from llmrec_amd.serve import csr_join, exclusion_csr, history_csr
    want_rp, want_ci = [0, 2, 2, 5, 6], [1, 9, 1, 3, 9, 4]
    forms = {
        "dict": {0: [9, 1, 1], 2: np.array([9, 3, 1, 1]), 3: torch.tensor([4])},                   # keyed by POSITION; row 1 is missing: empty
        "sequences": [[9, 1, 1], [], (3, 9, 1, 1), torch.tensor([4])],
        "pair": (np.array([0, 3, 3, 7, 8]), [9, 1, 1, 1, 9, 3, 1, 4]),
        "pair of tensors": (torch.tensor([0, 3, 3, 7, 8], dtype=torch.int32), torch.tensor([1, 9, 1, 3, 1, 9, 3, 4], dtype=torch.int32)),
        "array": np.array([[9, 1, 1, -1], [-1, -1, -1, -1], [9, 1, 3, 1], [4, -1, -1, -1]]),
        "tensor": torch.tensor([[9, -1, 1, 1], [-1, -1, -1, -1], [3, 9, 1, 1], [-1, -1, 4, -1]]),  # padding anywhere
    }
    for name, form in forms.items():
        for n in (None, 4):
            rp, ci = history_csr(form, 10, n)
            assert rp.dtype == np.int32 and ci.dtype == np.int32, name
            assert rp.tolist() == want_rp and ci.tolist() == want_ci, name                         # sorted, repeats collapsed, padding dropped
    rp, ci = history_csr({1: [2]}, 10, 4)                          # the row count something else fixes
    assert rp.tolist() == [0, 0, 1, 1, 1] and ci.tolist() == [2]
    assert history_csr({}, 10)[0].tolist() == [0] and history_csr([], 10)[0].tolist() == [0]
    assert history_csr(np.zeros((0, 3), np.int64), 10)[0].tolist() == [0]
    rp, ci = history_csr([np.arange(10)[::-1], [-1, -7]], 10)      # the whole catalogue; only padding
    assert rp.tolist() == [0, 10, 10] and ci.tolist() == list(range(10))
    for bad, n, match in (([[1], [10]], None, r"\[0, 10\)"), ({0: [99]}, None, r"\[0, 10\)"), (torch.tensor([[10]]), None, r"\[0, 10\)"),
                          ([[1], [2]], 3, "rows"), (np.zeros((3, 2), np.int64), 4, "rows"), ({4: [1]}, 4, "position"), ({-1: [1]}, None, "position"),
                          ((np.array([0, 1, 2]), [1, 2]), 3, "rows"), ((np.array([0, 2, 1]), [1, 2]), None, "rowptr"),
                          ((np.array([1, 1, 2]), [1, 2]), None, "rowptr"), ([[1.5]], None, "integer"), (np.arange(4), None, "expected"),
                          (7, None, "expected"), (None, None, "expected")):
        with pytest.raises(ValueError, match=match):
            history_csr(bad, 10, n)
    # the exclusion rows of recommend_new: the history, then the extra list, row by row
    hist = history_csr([[9, 1], [], [4]], 10)
    rp, ci = csr_join(hist, exclusion_csr({0: [0], 1: [5, 5], 2: []}, np.arange(3), 10))
    assert rp.tolist() == [0, 3, 5, 6] and ci.tolist() == [1, 9, 0, 5, 5, 4] and rp.dtype == np.int32 and ci.dtype == np.int32
    assert csr_join(hist, None) is hist


def test_the_entry_points_and_the_abi_version():
    from llmrec_amd import _lib
    protos = _lib.parse_header()
    assert protos["llmrec_fold_in_users_f32"][2] == ["n", "rowptr", "colidx", "nnz", "row_scale", "id_rows", "ldid", "T", "ldt", "n_items", "L",
                                                     "n_attr", "d", "c_m", "c_u", "c_a", "out", "ldo", "workspace", "workspace_bytes", "stream"]
    assert _lib.CONST["LLMREC_ABI_VERSION"] == 8 and _lib.load().llmrec_abi_version() == 8          # additive: the ABI version stays
    q = lambda *a: _lib.query("llmrec_fold_in_users_workspace_bytes", *a)
    assert q(100, 256, 2, 5, 64) == 0 and q(100, 257, 2, 5, 64) == (100 + 1) * 10 * 64 * 4
    assert q(16384, 16384 * 200, 2, 5, 64) == (16384 + 12800) * 2560 and q(-1, 0, 1, 0, 64) == -1 and q(1, 0, 0, 0, 64) == -1
    # argument errors come back as a status before anything is launched (no device is touched)
    lib = _lib.load()
    call = lambda **kw: lib.llmrec_fold_in_users_f32(*[kw.get(k, v) for k, v in dict(
        n=4, rowptr=0x1000, colidx=0x2000, nnz=8, row_scale=0x3000, id_rows=None, ldid=0, T=0x4000, ldt=640, n_items=50, L=2, n_attr=5, d=64,
        c_m=0.5, c_u=0.1, c_a=0.01, out=0x5000, ldo=64, workspace=None, workspace_bytes=0, stream=None).items()])
    EINVAL, EUNSUPPORTED, EWORKSPACE = (_lib.CONST[k] for k in ("LLMREC_EINVAL", "LLMREC_EUNSUPPORTED", "LLMREC_EWORKSPACE"))
    assert call(n=0) == 0
    assert call(d=129, ldt=10 * 129) == EUNSUPPORTED and call(d=128, n_attr=9, L=5, ldt=17 * 128) == EUNSUPPORTED
    for bad in (dict(L=0), dict(n_attr=10), dict(ldt=639), dict(ldo=63), dict(rowptr=None), dict(T=None), dict(out=None), dict(row_scale=None),
                dict(colidx=None), dict(id_rows=0x6000, ldid=63), dict(n_items=0), dict(nnz=-1), dict(nnz=300)):
        assert call(**bad) == EINVAL, bad
    assert call(nnz=300, workspace=0x7000, workspace_bytes=(4 + 1) * 2560 - 1) == EWORKSPACE


def test_the_script_takes_users_or_histories(tmp_path, capsys):
    import recommend
    base = ["--checkpoint", "c.ckpt", "--topk", "20", "--out", "o.npz", "--dataset", "netflix_valid_item"]
    own, rest = recommend.split_argv(base + ["--histories", "h.txt", "--include_seen", "--lr", "0.1"])
    assert (own.histories, own.users, own.include_seen) == ("h.txt", None, True) and rest == ["--dataset", "netflix_valid_item", "--lr", "0.1"]
    own, rest = recommend.split_argv(base + ["--users", "u.txt"])
    assert (own.histories, own.users) == (None, "u.txt")
    for argv, word in ((base + ["--users", "u.txt", "--histories", "h.txt"], "not allowed with"), (base, "one of the arguments")):
        with pytest.raises(SystemExit) as e:
            recommend.split_argv(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err
    (tmp_path / "h.txt").write_text("0 5\n0 3\n\n2 7\n0 5\n")      # the format of --exclude
    pairs = recommend.read_pairs(str(tmp_path / "h.txt"))
    lists = recommend.exclusion_lists(pairs, np.arange(3))
    assert {k: v.tolist() for k, v in lists.items()} == {0: [5, 3, 5], 2: [7]}
