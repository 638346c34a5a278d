"""The GPU tests' one way to a drop-in Trainer and its fused step: every switch of the step (llmrec_amd.step_options.ENV_SWITCHES) and of
the Trainer's choice of path (TRAINER_SWITCHES) is cleared first, so a test runs exactly what its `env` says whatever the shell had set,
and a new switch is cleared everywhere the day it joins those tuples."""
from collections import namedtuple

from llmrec_amd.step_options import ENV_SWITCHES, TRAINER_SWITCHES
from tests._dropin import load_dropin

Built = namedtuple("Built", "m trainer step batcher")          # the drop-in module, its Trainer, _fused_step() / _device_batcher() or None


def set_switches(monkeypatch, env):
    """The environment of one build: no switch set except those of `env`."""
    for k in ENV_SWITCHES + TRAINER_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def fused_trainer(monkeypatch, argv, env, seed=None, train=False, prepare=None, step=False, batcher=False) -> Built:
    """A fresh, seeded (seed=None: --seed), silenced Trainer of the drop-in started with `argv` under the switches `env`. train: the model
    in training mode; prepare(trainer): called before the step is built; step / batcher: also build tr._fused_step() / tr._device_batcher()."""
    set_switches(monkeypatch, env)
    m = load_dropin(argv)
    m.set_seed(m.args.seed if seed is None else seed)
    tr = m.Trainer(data_config={})
    tr.logger.logging = lambda s: None
    if train:
        tr.model_mm.train()
    if prepare is not None:
        prepare(tr)
    return Built(m, tr, tr._fused_step() if step else None, tr._device_batcher() if batcher else None)


def snapshot(trainer, step, extra=(), grads=True, cpu=False):
    """Clones of every parameter (p/), gradient (g/; grads), both Adam moments (m/, v/) and the step's tensors named in `extra`."""
    take = (lambda t: t.detach().cpu().clone()) if cpu else (lambda t: t.detach().clone())
    out = {name: take(getattr(step, name)) for name in extra}
    for name, p in trainer.model_mm.named_parameters():
        out["p/" + name] = take(p)
        if grads and p.grad is not None:
            out["g/" + name] = take(p.grad)
        st = trainer.optimizer.state.get(p)
        if st is not None and isinstance(st, tuple):
            out["m/" + name], out["v/" + name] = take(st[0]), take(st[1])
    return out
