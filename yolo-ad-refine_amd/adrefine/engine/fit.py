"""The epoch loop — the reference's BaseTrainer._do_train (engine/trainer.py:323-470) for one process, tying
FusedTrainer, the loader, close_mosaic, DetectionValidator(compute_loss=True), early stopping, results.csv and the
last.pt / best.pt checkpoints together.

`adrefine.engine` exports the function under the module's own name (`from adrefine.engine import fit`), so the
package attribute `adrefine.engine.fit` is the FUNCTION; reach this module's other names with
`from adrefine.engine.fit import ...` or `sys.modules["adrefine.engine.fit"]` (a `mock.patch("adrefine.engine.fit.X")`
would resolve to the function).

    results, last, best = fit(model, cfg, train_set, val_set, "runs/exp")

Per epoch (trainer.py:348-447): at epoch == epochs - close_mosaic the dataset's mosaic is closed and the loader reset
(:361-363); every batch is one FusedTrainer.step (warm-up, accumulate, lr and momentum by the batch index, as the
reference does in the loop body :368-381); the running mean of the loss items is `tloss = (tloss * i + items) / (i + 1)`
(:388-390), kept on the device and read once per epoch. After the epoch, when `val` is set, on the last epoch, or when
the stopper may stop next epoch (:435): validator.load_ema(trainer) and a validation with compute_loss=True; the
results are rounded to five decimals as the reference's training-mode validator returns them (engine/validator.py:205,
detect/train.py:108). One results.csv row (save_metrics :652-659: `epoch,time,<keys>`, values `%.6g`), then the stopper
(`Patience`, the rule of utils/torch_utils.py EarlyStopping), then the checkpoint (:443-445).

results.csv columns, in the reference's order: epoch, time, train/box_loss, train/cls_loss, train/dfl_loss,
metrics/precision(B), metrics/recall(B), metrics/mAP50(B), metrics/mAP50-95(B), val/box_loss, val/cls_loss,
val/dfl_loss, lr/pg0, lr/pg1, lr/pg2. lr/pgN is the reference optimizer's param_groups[N]['lr'] after the epoch's last
batch; its groups are (biases, decayed weights, norm weights) = the trainer's (g2, g0, g1) — see trainer.Schedule.
Until an epoch validates the metric and val columns are 0 (the reference's initial self.metrics, :297-298).

Resume (`resume=<last.pt>`): checkpoint.resume restores model, EMA, optimizer state and the batch counter as the
reference's resume_training does (model and EMA from the fp16 EMA weights); the loop continues at the saved epoch + 1
with the saved best fitness, the loader's permutation generator is advanced past the finished epochs, and mosaic is
closed at once when the resumed epoch lies past the close epoch (:744-746). That is the default and the reference's
behaviour. With exact_resume=True (opt-in) fit also writes `last_state.pt` next to last.pt, FusedTrainer.state_dict()
of the same epoch (fp32 model state, EMA, optimizer moments, gradient arena, step counters: about five times the
parameter bytes), and a resume with exact_resume=True loads it over the fp16 state when it belongs to the
checkpoint's epoch, so the resumed run continues with the bits the interrupted one had.

Not here: world_size > 1 (raises NotImplementedError; FusedTrainer itself keeps its DDP support), plots, json / txt
export, rect training, the tuner, the `time` budget, and callbacks other than on_epoch_end(epoch, row).
"""
from __future__ import annotations

import copy
import time
from pathlib import Path

import torch

TRAIN_KEYS = ("train/box_loss", "train/cls_loss", "train/dfl_loss")
METRIC_KEYS = ("metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)")
VAL_KEYS = ("val/box_loss", "val/cls_loss", "val/dfl_loss")
LR_KEYS = ("lr/pg0", "lr/pg1", "lr/pg2")
CSV_KEYS = ("epoch", "time", *TRAIN_KEYS, *METRIC_KEYS, *VAL_KEYS, *LR_KEYS)

# cfg/default.yaml
_DEFAULTS = dict(epochs=100, batch=16, imgsz=640, patience=100, optimizer="auto", cos_lr=False, close_mosaic=10,
                 lr0=0.01, lrf=0.01, momentum=0.937, weight_decay=0.0005, warmup_epochs=3.0, warmup_momentum=0.8,
                 warmup_bias_lr=0.1, nbs=64, val=True, save=True, multi_scale=False, rect=False, pretrained=True)


def _arg(cfg, name):
    v = getattr(cfg, name, None)
    return _DEFAULTS[name] if v is None else v


class Patience:
    """The early-stopping rule of the reference (utils/torch_utils.py:716-759), restated: the run ends once `limit`
    epochs in a row brought no fitness at least as high as the best before them (a tie counts as a new best, and the
    best starts at 0, so an all-zero early phase keeps resetting the count). limit 0 / None never stops; an epoch
    without a fitness (val=False) changes nothing. `may_stop_next` tells the loop that the coming epoch could be
    the last, so it must validate."""

    def __init__(self, limit):
        self.limit = limit if limit else float("inf")
        self.top, self.top_epoch = 0.0, 0
        self.may_stop_next = False

    def update(self, epoch, fitness):
        """`epoch` counts from 1. Returns whether to stop after it."""
        if fitness is None:
            return False
        if fitness >= self.top:
            self.top, self.top_epoch = fitness, epoch
        waited = epoch - self.top_epoch
        self.may_stop_next = waited + 1 >= self.limit
        return waited >= self.limit


def csv_header():
    """The header line of results.csv: the column names joined by commas (what save_metrics writes, trainer.py:656)."""
    return ",".join(CSV_KEYS) + "\n"


def csv_row(epoch, seconds, metrics):
    """One value line for epoch index `epoch` (written 1-based) in save_metrics' number format, %.6g (trainer.py:659)."""
    cells = [epoch + 1, seconds, *(metrics[k] for k in CSV_KEYS[2:])]
    return ",".join(format(v, ".6g") for v in cells) + "\n"


def lr_columns(trainer_lr):
    """{'lr/pg0', 'lr/pg1', 'lr/pg2'} from the trainer's (g0 decayed weights, g1 norm weights, g2 biases): the
    reference's param_groups are (biases, decayed weights, norm weights) (trainer.py:798-808)."""
    g0, g1, g2 = (float(v) for v in trainer_lr)
    return dict(zip(LR_KEYS, (g2, g0, g1)))


def close_epoch(epochs, close_mosaic):
    """The epoch index whose first batch already runs without mosaic (trainer.py:361), or None (close_mosaic 0)."""
    return epochs - close_mosaic if close_mosaic else None


def _default_trainer(model, cfg, nb, n_images, **kw):
    from .trainer import FusedTrainer, optimizer_iterations
    batch, nbs, epochs = _arg(cfg, "batch"), _arg(cfg, "nbs"), _arg(cfg, "epochs")
    opt = _arg(cfg, "optimizer")
    return FusedTrainer(model, lr0=_arg(cfg, "lr0"), momentum=_arg(cfg, "momentum"),
                        weight_decay=_arg(cfg, "weight_decay"), nbs=nbs, batch_size=batch, epochs=epochs, nb=nb,
                        lrf=_arg(cfg, "lrf"), warmup_epochs=_arg(cfg, "warmup_epochs"),
                        warmup_bias_lr=_arg(cfg, "warmup_bias_lr"), warmup_momentum=_arg(cfg, "warmup_momentum"),
                        cos_lr=_arg(cfg, "cos_lr"), optimizer=opt,
                        iterations=optimizer_iterations(n_images, batch, nbs, epochs) if opt == "auto" else None,
                        multi_scale=_arg(cfg, "multi_scale"), imgsz=_arg(cfg, "imgsz"), **kw)


def _default_validator(model, cfg):
    from .validator import DetectionValidator
    val_model = copy.deepcopy(model).eval()  # the validator's own copy; load_ema overwrites its weights
    return DetectionValidator(val_model, val_model.model[-1].nc, compute_loss=True)


def _default_loader(dataset, batch, shuffle, prefetch):
    from ..data.build import build_dataloader
    return build_dataloader(dataset, batch, shuffle=shuffle, prefetch=prefetch)


def _train_args(cfg):
    """cfg as the checkpoint's train_args: a `pretrained` given as weights is recorded as True and a path as its
    string, so the file holds the arguments, not a second copy of the weights, and still loads weights_only."""
    args = dict(vars(cfg)) if hasattr(cfg, "__dict__") else {}
    pre = args.get("pretrained")
    if pre is not None and not isinstance(pre, bool):
        args["pretrained"] = str(pre) if isinstance(pre, (str, Path)) else True
    return args


def _state_path(last):
    return Path(last).with_name("last_state.pt")


def fit(model, cfg, train_set, val_set, save_dir, resume=None, graphs=True, prefetch=1, world_size=1,
        on_epoch_end=None, exact_resume=False, trainer_factory=None, validator_factory=None, loader_factory=None,
        checkpoint=None, trainer_kw=None):
    """Train `model` for cfg.epochs epochs on `train_set`, validating on `val_set` after each epoch.

    cfg: a namespace with the reference's training arguments (epochs, batch, imgsz, nbs, optimizer, lr0, lrf, momentum,
    weight_decay, warmup_*, cos_lr, multi_scale, close_mosaic, patience, val, save, pretrained; absent ones take
    cfg/default.yaml's values) and the augmentation hyper-parameters close_mosaic edits. pretrained: a path or a
    state_dict is loaded with model.load before the validator copies the model (True / False / None load nothing:
    there is no hub). train_set / val_set: datasets
    as data.build.build_yolo_dataset returns them (mode 'train' / 'val'). graphs=True captures the step into hipGraphs
    after the first eager step; graphs=False runs every step eagerly. on_epoch_end(epoch, row) is called with the
    epoch index and the dict written to results.csv; a true return value stops the run after that epoch's checkpoint.
    trainer_factory(model, cfg, nb, n_images), validator_factory(model, cfg), loader_factory(dataset, batch, shuffle,
    prefetch) and `checkpoint` (an object with save_checkpoint, save_last_and_best, load_checkpoint, resume; default
    engine.checkpoint) replace the parts, for tests of the host logic. exact_resume=True (off by default) also keeps
    FusedTrainer.state_dict() in last_state.pt beside last.pt and, on resume, loads it over the checkpoint's state.

    Returns (results, last, best): the last results.csv row as a dict plus 'fitness', 'best_fitness' and 'tloss'
    (the last epoch's running mean of the loss items before rounding, a CPU fp32 tensor), and the paths of last.pt
    and best.pt (None for a file the run did not write)."""
    if world_size > 1:
        raise NotImplementedError("fit runs one process; for DDP drive FusedTrainer(world_size=...) per rank")
    if _arg(cfg, "rect"):
        raise NotImplementedError("fit: rect training is not supported")
    if checkpoint is None:
        from . import checkpoint
    epochs, batch = int(_arg(cfg, "epochs")), int(_arg(cfg, "batch"))
    save_dir = Path(save_dir)
    wdir = save_dir / "weights"
    wdir.mkdir(parents=True, exist_ok=True)
    csv = save_dir / "results.csv"
    last, best = wdir / "last.pt", wdir / "best.pt"

    # get_model (models/yolo/detect/train.py:86-91): pretrained weights go into the model before anything copies it
    # or caches its weights. True / False / None load nothing (there is no hub to fetch a default from)
    pretrained = _arg(cfg, "pretrained")
    if pretrained is not None and not isinstance(pretrained, bool) and not resume:  # a resume takes last.pt's weights
        model.load(pretrained)
    loader = (loader_factory or _default_loader)(train_set, batch, True, prefetch)
    nb = len(loader)
    validator = (validator_factory or _default_validator)(model, cfg)  # copies the model before the trainer tags it
    trainer = (trainer_factory or _default_trainer)(model, cfg, nb, len(train_set), **(trainer_kw or {}))
    val_loader = (loader_factory or _default_loader)(val_set, batch * 2, False, 0)
    stopper = Patience(_arg(cfg, "patience"))
    close_at = close_epoch(epochs, int(_arg(cfg, "close_mosaic")))

    def close():
        from ..data.augment import close_mosaic
        close_dataset = getattr(train_set, "close_mosaic", None)  # a dataset bound as INTEGRATION.md shows
        close_dataset(hyp=cfg) if close_dataset is not None else close_mosaic(train_set, cfg)
        loader.reset()

    start_epoch, best_fitness = 0, None
    if resume:
        ckpt = checkpoint.load_checkpoint(resume)
        start_epoch, best_fitness = checkpoint.resume(trainer, ckpt)
        if exact_resume and _state_path(resume).is_file():
            state = torch.load(_state_path(resume), map_location="cpu", weights_only=True)
            if state.get("epoch") == start_epoch - 1:  # written with this checkpoint
                trainer.load_state_dict(state["trainer"])
        if hasattr(loader, "indices"):
            for _ in range(start_epoch):  # the finished epochs' permutations
                loader.indices()
        if close_at is not None and start_epoch > close_at:
            close()
    elif csv.exists():
        csv.unlink()  # a fresh run writes a fresh file (the reference picks a new save_dir)

    # the reference's initial self.metrics: every validator key and val loss 0 until an epoch validates
    metrics = dict.fromkeys(METRIC_KEYS + VAL_KEYS, 0)
    fitness, row, stop, tloss = None, None, False, None
    t0 = time.time()
    captured = False
    for epoch in range(start_epoch, epochs):
        if hasattr(loader, "set_epoch"):
            loader.set_epoch(epoch)
        if epoch == close_at:
            close()
        tloss = None
        for i, b in enumerate(loader):
            items = trainer.step(b)
            tloss = (tloss * i + items) / (i + 1) if tloss is not None else items.clone()
            if graphs and not captured:  # the first step ran eagerly (lazy caches, the parameter table)
                trainer.capture(b)
                captured = True
        final_epoch = epoch + 1 >= epochs
        if _arg(cfg, "val") or final_epoch or stopper.may_stop_next or stop:
            validator.load_ema(trainer)
            res = validator(val_loader)
            metrics = {k: round(float(res[k]), 5) for k in METRIC_KEYS + VAL_KEYS}
            fitness = round(float(res["fitness"]), 5)
        tloss = tloss.cpu() if tloss is not None else torch.zeros(3)  # the epoch's one read of the train losses
        train_items = [round(float(x), 5) for x in tloss.tolist()]
        row = {**dict(zip(TRAIN_KEYS, train_items)), **metrics, **lr_columns(trainer.lr)}
        with open(csv, "a") as f:
            f.write(("" if csv.stat().st_size else csv_header()) + csv_row(epoch, time.time() - t0, row))
        stop = stop or stopper.update(epoch + 1, fitness) or final_epoch
        if _arg(cfg, "save") or final_epoch:
            kw = dict(train_args=_train_args(cfg), train_metrics={**row})
            if fitness is None:  # never validated: last.pt only
                checkpoint.save_checkpoint(trainer, last, epoch, best_fitness=best_fitness, **kw)
            else:
                best_fitness = checkpoint.save_last_and_best(trainer, wdir, epoch, fitness, best_fitness, **kw)
            if exact_resume:
                torch.save({"epoch": int(epoch), "trainer": trainer.state_dict()}, _state_path(last))
        if on_epoch_end is not None and on_epoch_end(epoch, dict(row)):
            stop = True
        if stop:
            break
    results = dict(row or {}, fitness=fitness, best_fitness=best_fitness, tloss=tloss)
    return results, (last if last.exists() else None), (best if best.exists() else None)
