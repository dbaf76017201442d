"""Training-step driver (mirrors the step semantics of the reference's ultralytics/engine/trainer.py) and the epoch
loop `fit` (engine/fit.py, the reference's BaseTrainer._do_train for one process).

`fit` below is the function: it takes the place of the submodule as the attribute `adrefine.engine.fit`. The
module's other names are reached with `from adrefine.engine.fit import ...` (resolved through sys.modules)."""
from .fit import fit  # noqa: F401
