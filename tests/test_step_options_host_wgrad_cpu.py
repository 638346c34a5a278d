"""CPU: the three values of LLMREC_HOST_CHAIN in llmrec_amd.step_options.resolve - "1" (default): the forward's and the weight
gradient's hosted products; "fwd": the forward's only (round 15's step, the A/B reference of the weight gradient's); "0": neither
(host_chain is off, and FusedStep's condition for the weight gradient's is host_chain and host_wgrad and its gate). Anything else is
the default. No other field moves, and host_wgrad is the record's LAST field with the default True, so records written before it
existed still compare equal to the default."""
from llmrec_amd import step_options as SO

NF = dict(n_users=13187, n_items=17366, d=64, n_attr=5, drop_rate=0.0, wgrad_rows_default=True, inline_adamw_default=True,
          fold_default=True, bwd_nnz=68933, bwd_valued=False, bwd_col_scaled=True, latency_nnz=1 << 20)


def resolve(value=None):
    return SO.resolve({} if value is None else {"LLMREC_HOST_CHAIN": value}, **NF)


def test_default_is_both_hostings():
    for value in (None, "1"):
        r = resolve(value)
        assert (r.host_chain, r.host_wgrad) == (True, True), value


def test_fwd_keeps_the_forward_hosting_only():
    r = resolve("fwd")
    assert (r.host_chain, r.host_wgrad) == (True, False)
    assert r == resolve()._replace(host_wgrad=False)


def test_zero_turns_the_chain_hosting_off():
    r = resolve("0")
    assert r.host_chain is False and r.host_wgrad is True          # (the effective condition is host_chain and host_wgrad)
    assert r == resolve()._replace(host_chain=False)


def test_junk_values_are_the_default():
    for value in ("", "2", "true", "FWD", "off", " 0"):
        assert resolve(value) == resolve(), value


def test_host_wgrad_is_the_last_field_and_defaults_to_true():
    assert SO.StepOptions._fields[-2:] == ("host_chain", "host_wgrad")
    assert SO.StepOptions._field_defaults == {"host_wgrad": True}
    assert "LLMREC_HOST_CHAIN" in SO.ENV_SWITCHES and not any("WGRAD_HOST" in n or "HOST_WGRAD" in n for n in SO.ENV_SWITCHES)
