"""CPU: llmrec_amd.step_options.resolve - the one place FusedStep's switches are decided - against hand-written records. No GPU, no
library. nf = the Netflix shape (U = 13 187 <= I = 17 366, d = 64, five attribute streams, a small, pattern-only, column-scaled side
product); ml = the same with U > I."""
import os

import pytest

from llmrec_amd import step_options as SO

LATENCY_NNZ = 1 << 20              # a threshold of the test's own: resolve() takes ops.SPMM_LATENCY_NNZ as an argument
NF = dict(n_users=13187, n_items=17366, d=64, n_attr=5, drop_rate=0.0, wgrad_rows_default=True, inline_adamw_default=True,
          fold_default=True, bwd_nnz=68933, bwd_valued=False, bwd_col_scaled=True, latency_nnz=LATENCY_NNZ)
ML = dict(NF, n_users=17366, n_items=13187)
DP = dict(wgrad_rows_default=False, inline_adamw_default=False, fold_default=False)
NF_DEFAULT = SO.StepOptions(drop_rate=0.0, check_zero=False, multi_stream=False, gemm="bf16x3", preprop=True, wgrad_rows=True,
                            inline_adamw=True, fold=True, bwd_mask=True, bwd_zero_skip=True, host_chain=True)


def resolve(env=None, shape=NF, **kw):
    return SO.resolve(dict(env or {}), **dict(shape, **kw))


def test_the_two_shapes_with_an_empty_environment():
    assert resolve() == NF_DEFAULT
    assert resolve(shape=ML) == NF_DEFAULT._replace(preprop=False, wgrad_rows=False)
    assert all(type(v) is (str if k == "gemm" else float if k == "drop_rate" else bool) for k, v in resolve()._asdict().items())
    with pytest.raises(AttributeError):
        resolve().fold = False                                            # the record is immutable


def test_prepropagate_is_forced_by_1_and_0_and_left_to_the_shape_otherwise():
    assert resolve({"LLMREC_PREPROPAGATE": "1"}, ML) == NF_DEFAULT
    assert resolve({"LLMREC_PREPROPAGATE": "0"}) == NF_DEFAULT._replace(preprop=False, wgrad_rows=False)
    assert resolve({"LLMREC_PREPROPAGATE": "x"}) == NF_DEFAULT
    assert resolve({"LLMREC_PREPROPAGATE": "x"}, ML) == NF_DEFAULT._replace(preprop=False, wgrad_rows=False)


def test_the_embedding_width_limits_prepropagation_and_the_mask():
    wide = resolve({"LLMREC_PREPROPAGATE": "1"}, d=128)
    assert wide == NF_DEFAULT._replace(preprop=False, wgrad_rows=False, bwd_mask=False, bwd_zero_skip=False)
    assert resolve(d=16) == NF_DEFAULT._replace(bwd_mask=False, bwd_zero_skip=False)


def test_the_row_listed_weight_gradient_needs_bf16x3_its_switch_and_an_attribute_stream():
    assert resolve({"LLMREC_GEMM": "f32"}) == NF_DEFAULT._replace(gemm="f32", wgrad_rows=False)
    assert resolve({"LLMREC_WGRAD_ROWS": "0"}) == NF_DEFAULT._replace(wgrad_rows=False)
    assert resolve(n_attr=0) == NF_DEFAULT._replace(wgrad_rows=False, bwd_mask=False, bwd_zero_skip=False)


def test_fold_and_the_backward_mask():
    assert resolve({"LLMREC_FOLD": "0"}) == NF_DEFAULT._replace(fold=False, bwd_mask=False, bwd_zero_skip=False)
    assert resolve({"LLMREC_BWD_MASK": "0"}) == NF_DEFAULT._replace(bwd_mask=False, bwd_zero_skip=False)
    assert resolve({"LLMREC_BWD_MASK": "spmm"}) == NF_DEFAULT._replace(bwd_zero_skip=False)
    assert resolve({"LLMREC_BWD_MASK": "2"}) == NF_DEFAULT
    unmasked = NF_DEFAULT._replace(bwd_mask=False, bwd_zero_skip=False)
    assert resolve(bwd_valued=True) == unmasked
    assert resolve(bwd_col_scaled=False) == unmasked
    assert resolve(bwd_nnz=LATENCY_NNZ) == unmasked
    assert resolve(bwd_nnz=LATENCY_NNZ - 1) == NF_DEFAULT


def test_the_independent_switches_change_their_own_field_only():
    assert resolve({"LLMREC_STREAMS": "1"}) == NF_DEFAULT._replace(multi_stream=True)
    assert resolve({"LLMREC_HOST_CHAIN": "0"}) == NF_DEFAULT._replace(host_chain=False)
    assert resolve({"LLMREC_CHECK_ZERO": "1"}) == NF_DEFAULT._replace(check_zero=True)


def test_only_1_switches_a_boolean_on():
    assert resolve({"LLMREC_STREAMS": "true"}) == NF_DEFAULT
    assert resolve({"LLMREC_FOLD": "true"}) == NF_DEFAULT._replace(fold=False, bwd_mask=False, bwd_zero_skip=False)


def test_dropout_runs_in_the_reference_order():
    dropped = NF_DEFAULT._replace(drop_rate=0.5, preprop=False, wgrad_rows=False)
    assert resolve(drop_rate=0.5) == dropped
    assert resolve({"LLMREC_PREPROPAGATE": "0"}, drop_rate=0.5) == dropped
    with pytest.raises(RuntimeError, match="LLMREC_PREPROPAGATE=1 cannot be honoured"):
        resolve({"LLMREC_PREPROPAGATE": "1"}, drop_rate=0.5)
    assert resolve({"LLMREC_PREPROPAGATE": "1"}, drop_rate=0) == NF_DEFAULT
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
            resolve(drop_rate=bad)


def test_the_data_parallel_class_defaults():
    off = NF_DEFAULT._replace(wgrad_rows=False, inline_adamw=False, fold=False, bwd_mask=False, bwd_zero_skip=False)
    assert resolve(**DP) == off and off.preprop
    assert resolve({"LLMREC_FOLD": "1"}, **DP) == off
    assert resolve({"LLMREC_WGRAD_ROWS": "1"}, **DP) == off


class Recording(dict):
    """A mapping that notes every name looked up in it."""
    def __init__(self, *a):
        super().__init__(*a)
        self.asked = set()

    def get(self, key, default=None):
        self.asked.add(key)
        return super().get(key, default)

    def __getitem__(self, key):
        self.asked.add(key)
        return super().__getitem__(key)

    def __contains__(self, key):
        self.asked.add(key)
        return super().__contains__(key)


def test_every_variable_the_resolver_reads_is_listed():
    asked = set()
    for env in ({}, {k: "1" for k in SO.ENV_SWITCHES}, {k: "0" for k in SO.ENV_SWITCHES}):
        for kw in ({}, DP, {"d": 128}, {"n_attr": 0}):
            rec = Recording(env)
            SO.resolve(rec, **dict(NF, **kw))
            asked |= rec.asked
    assert asked == set(SO.ENV_SWITCHES)
    assert len(set(SO.ENV_SWITCHES + SO.TRAINER_SWITCHES)) == len(SO.ENV_SWITCHES) + len(SO.TRAINER_SWITCHES) == 13


def test_none_stands_for_the_process_environment(monkeypatch):
    for k in SO.ENV_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    assert SO.resolve(None, **NF) == NF_DEFAULT
    monkeypatch.setenv("LLMREC_STREAMS", "1")
    assert SO.resolve(None, **NF) == NF_DEFAULT._replace(multi_stream=True)


def test_the_step_reads_no_environment_itself():
    here = os.path.dirname(os.path.abspath(__file__))
    assert "environ" not in open(os.path.join(here, "..", "llmrec_amd", "fused.py")).read()
    src = open(SO.__file__).read()
    assert "import torch" not in src and "_lib" not in src
