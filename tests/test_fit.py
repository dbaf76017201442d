"""Host logic of engine/fit.py with stub trainer / validator / loader / checkpoint factories (no GPU): results.csv
formatting against the reference's own lines (tests/golden/results_csv.txt, scripts/gen_valloss_golden.py), the
close-mosaic epoch, validation of the last epoch under val=False, early stopping, resume, the lr column order."""
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from conftest import GOLDEN

from adrefine.engine import fit
from adrefine.engine import fit as fit_exported
from adrefine.engine.fit import CSV_KEYS, METRIC_KEYS, VAL_KEYS, Patience, close_epoch, csv_header, csv_row

NB = 3


class Trainer:
    def __init__(self):
        self.lr = [0.1, 0.2, 0.3]  # g0 decayed weights, g1 norm weights, g2 biases
        self.steps = 0

    def step(self, batch):
        self.steps += 1
        return torch.tensor([1.0, 2.0, 3.0]) * self.steps


class Validator:
    def __init__(self, fitness):
        self.fitness, self.calls, self.ema_loads = list(fitness), [], 0

    def load_ema(self, trainer):
        self.ema_loads += 1

    def __call__(self, loader):
        f = self.fitness[len(self.calls)]
        self.calls.append(f)
        return {**dict.fromkeys(METRIC_KEYS, f), **dict.fromkeys(VAL_KEYS, 2 * f + 0.000004), "fitness": f,
                "speed": {}}


class Loader:
    def __init__(self, n):
        self.n, self.resets = n, 0

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter([{"k": k} for k in range(self.n)])

    def reset(self):
        self.resets += 1


class Dataset:
    def __init__(self, trainer):
        self.trainer, self.closed_at_step = trainer, None

    def __len__(self):
        return 2 * NB

    def close_mosaic(self, hyp):
        assert self.closed_at_step is None
        self.closed_at_step = self.trainer.steps


class Checkpoint:
    def __init__(self, resume_to=None):
        self.saved, self.resume_to, self.resumed = [], resume_to, None

    def save_checkpoint(self, trainer, path, epoch, best_fitness=None, **kw):
        Path(path).write_bytes(b"last")
        self.saved.append(("last", epoch, None, best_fitness))

    def save_last_and_best(self, trainer, wdir, epoch, fitness, best_fitness=None, **kw):
        (Path(wdir) / "last.pt").write_bytes(b"last")
        if best_fitness is None or fitness >= best_fitness:
            (Path(wdir) / "best.pt").write_bytes(b"best")
        self.saved.append(("both", epoch, fitness, best_fitness))
        return fitness if best_fitness is None else max(best_fitness, fitness)

    def load_checkpoint(self, path):
        return {"path": str(path)}

    def resume(self, trainer, ckpt):
        self.resumed = ckpt
        return self.resume_to


def _run(tmp_path, fitness, ckpt=None, resume=None, **cfg):
    cfg = SimpleNamespace(**{"epochs": 5, "batch": 2, "close_mosaic": 0, "patience": 100, "val": True, **cfg})
    trainer, validator = Trainer(), Validator(fitness)
    ds = Dataset(trainer)
    loaders = []

    def loader_factory(dataset, batch, shuffle, prefetch):
        loaders.append(Loader(NB))
        return loaders[-1]

    ckpt = ckpt or Checkpoint()
    out = fit(SimpleNamespace(), cfg, ds, object(), tmp_path, resume=resume, graphs=False,
              trainer_factory=lambda model, c, nb, n: trainer, validator_factory=lambda model, c: validator,
              loader_factory=loader_factory, checkpoint=ckpt)
    rows = (tmp_path / "results.csv").read_text().splitlines()
    return SimpleNamespace(out=out, rows=rows, trainer=trainer, validator=validator, ds=ds, loaders=loaders, ckpt=ckpt)


def _reference_lines():
    lines = (GOLDEN / "results_csv.txt").read_text().splitlines()
    vals = dict(l.split("=", 1) for l in lines[2:])
    return lines[0], lines[1], {k: float(v) for k, v in vals.items()}


def test_exported():
    assert fit_exported is fit and callable(fit)


def test_csv_lines_are_the_references():
    header, row, vals = _reference_lines()
    assert csv_header() == header + "\n"
    assert tuple(header.split(",")) == CSV_KEYS
    assert csv_row(int(vals["epoch"]), vals["time"], vals) == row + "\n"


def test_results_csv_of_a_run(tmp_path):
    header, _, _ = _reference_lines()
    r = _run(tmp_path, [0.1, 0.2, 0.3, 0.4, 0.5])
    assert r.rows[0] == header and len(r.rows) == 6
    cols = r.rows[2].split(",")
    assert cols[0] == "2" and len(cols) == len(CSV_KEYS)
    # the running mean of epoch 1's items (steps 4, 5, 6 -> mean 5) and the metrics rounded to five decimals
    assert cols[2:5] == ["5", "10", "15"]
    assert cols[5:9] == ["0.2"] * 4 and cols[9:12] == ["0.4"] * 3  # 0.400004 -> round(.., 5) -> 0.4
    # the reference's param groups are (biases, decayed weights, norm weights) = the trainer's (g2, g0, g1)
    assert cols[12:15] == ["0.3", "0.1", "0.2"]
    results, last, best = r.out
    assert results["fitness"] == 0.5 and results["best_fitness"] == 0.5 and last.name == "last.pt" and best.exists()
    assert r.validator.ema_loads == 5
    assert [s[3] for s in r.ckpt.saved] == [None, 0.1, 0.2, 0.3, 0.4]  # the running best is handed back in


def test_close_mosaic_epoch(tmp_path):
    assert close_epoch(5, 2) == 3 and close_epoch(5, 0) is None
    r = _run(tmp_path, [0.1] * 5, close_mosaic=2)
    assert r.ds.closed_at_step == 3 * NB  # before the first batch of epoch index 3 = epochs - close_mosaic
    assert r.loaders[0].resets == 1 and r.loaders[1].resets == 0


def test_last_epoch_validates_under_val_false(tmp_path):
    r = _run(tmp_path, [0.9], val=False)
    assert len(r.validator.calls) == 1 and len(r.rows) == 6
    assert r.rows[4].split(",")[5:12] == ["0"] * 7  # never validated: the reference's initial zeros
    assert r.rows[5].split(",")[5:9] == ["0.9"] * 4
    assert [s[0] for s in r.ckpt.saved] == ["last"] * 4 + ["both"]


def test_early_stopping_epoch(tmp_path):
    """patience 2: best at epoch 1 (0.5), epochs 2 and 3 are worse -> delta = 2 >= patience after epoch 3."""
    seq = [0.5, 0.4, 0.3, 0.9, 0.9]
    st = Patience(2)
    assert [st.update(e + 1, f) for e, f in enumerate(seq[:3])] == [False, False, True]
    assert st.may_stop_next
    r = _run(tmp_path, seq, patience=2)
    assert len(r.rows) == 1 + 3 and r.trainer.steps == 3 * NB
    # a fitness equal to the best resets the count (>=), and patience 0 never stops
    st, flags = Patience(2), []
    for e, f in enumerate([0.5, 0.4, 0.5, 0.4, 0.4]):
        flags.append((st.update(e + 1, f), st.may_stop_next))
    # may_stop_next: one more epoch without a best would reach the limit
    assert flags == [(False, False), (False, True), (False, False), (False, True), (True, True)]
    never = Patience(0)
    assert not any(never.update(e, 0.0 if e == 1 else -1.0) or never.may_stop_next for e in range(1, 50))
    assert not Patience(1).update(1, None)  # no fitness (val=False): nothing changes


def test_possible_stop_validates_under_val_false(tmp_path):
    """val=False never gives the stopper a fitness, so it never stops and only the last epoch validates."""
    r = _run(tmp_path, [0.5], val=False, patience=1)
    assert len(r.rows) == 6 and len(r.validator.calls) == 1


def test_resume_epoch_and_best_fitness(tmp_path):
    first = _run(tmp_path, [0.1, 0.2, 0.3, 0.4, 0.5])  # only its csv matters: cut back to two epochs below
    assert len(first.rows) == 6
    (tmp_path / "results.csv").write_text("\n".join(first.rows[:3]) + "\n")  # header + epochs 1, 2
    ck = Checkpoint(resume_to=(2, 0.7))
    r = _run(tmp_path, [0.6, 0.8, 0.1], ckpt=ck, resume=tmp_path / "weights" / "last.pt", close_mosaic=2)
    assert ck.resumed == {"path": str(tmp_path / "weights" / "last.pt")}
    assert [row.split(",")[0] for row in r.rows[1:]] == ["1", "2", "3", "4", "5"]  # appended, continuing at epoch 3
    assert r.trainer.steps == 3 * NB
    assert [(s[1], s[3]) for s in ck.saved] == [(2, 0.7), (3, 0.7), (4, 0.8)]  # the saved best, then the running one
    assert r.ds.closed_at_step == NB  # epoch index 3 = the resumed run's second epoch
    # resumed past the close epoch: mosaic is closed before the first batch
    ck = Checkpoint(resume_to=(4, 0.7))
    r = _run(tmp_path, [0.6], ckpt=ck, resume="x.pt", close_mosaic=2)
    assert r.ds.closed_at_step == 0 and r.trainer.steps == NB


def test_world_size_raises(tmp_path):
    with pytest.raises(NotImplementedError):
        fit(None, SimpleNamespace(), None, None, tmp_path, world_size=2)
