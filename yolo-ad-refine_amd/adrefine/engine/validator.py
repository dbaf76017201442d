"""Detection validator — the reference's models/yolo/detect/val.py DetectionValidator on the device
(engine/validator.py:104-216 the loop, val.py:92-161 postprocess + update_metrics, :179-187 get_stats).

Per batch: the collated uint8 images go through a FusedPredictor (forward + decode + NMS with the validator's
settings, one hipGraph after the first batch), then adr_scale_boxes maps the padded detections to each source image
and adr_val_match does all per-image bookkeeping in one launch (labels to native space, TP matching at the ten IoU
thresholds, confusion matrix, label tallies). Nothing is read back inside the loop: the statistics stay on the
device until the AP integration at the end (utils/metrics.DetectionStats.results).

Differences from the reference, by design: one hipGraph holds the forward, the decode and the NMS, so
speed['inference'] covers all three and speed['postprocess'] is the scaling + matching (the reference counts NMS as
postprocess); single_cls on a model with more than one class needs agnostic multi-label NMS, which adr_nms does not
provide (the predictor raises NotImplementedError) — a single_cls run evaluates a one-class model, as the
reference's single_cls dataset yields; no json / txt export and no plots.
"""
from __future__ import annotations

import torch

from ..utils.metrics import DetectionStats
from .predictor import FusedPredictor

RESULT_KEYS = ("metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)", "metrics/mAP50-95(B)", "fitness")
LOSS_KEYS = ("val/box_loss", "val/cls_loss", "val/dfl_loss")  # label_loss_items(prefix="val"), detect/train.py:109-118


class DetectionValidator:
    """validator = DetectionValidator(model, nc); results = validator(batches).

    batches: an iterable of collated validation batches (data/augment.collate_fn on the val LetterBox + Format
    chain): `img` uint8 (B, 3, H, W), `cls`, `bboxes` (normalised xywh), `batch_idx` (host tensors), and the
    per-image lists `ori_shape` and `ratio_pad`. The first batch's shape is captured; a smaller last batch runs
    eagerly. Returns the reference's results_dict keys plus 'fitness', the per-class arrays and tallies of
    DetectionStats.results() ('p', 'r', 'ap', 'ap_class_index', 'nt_per_class', 'nt_per_image', 'seen',
    'confusion_matrix') and 'speed' = {'preprocess', 'inference', 'postprocess'} in ms per image from HIP events
    read after the loop.

    `model` is the validator's own copy of the network (eval mode; load_ema overwrites its weights). augment=True
    validates with the reference's test-time augmentation (val(..., augment=True); FusedPredictor(augment=True)).

    compute_loss=True is the validation loss of a training run (engine/validator.py:184, `self.loss +=
    model.loss(batch, preds)[1]`): after each batch's forward the criterion is evaluated value-only (adr_det_loss
    without gradients) on the predictor's kept level maps, with targets built from the batch's batch_idx / cls /
    bboxes at the batch's own image size and zero-padded to FusedTrainer.capacity_bucket rows per image. The three
    items are summed on the device in fp32 in batch order (adr_axpy, a = 1) and read once after the loop; the
    results gain 'val/box_loss', 'val/cls_loss', 'val/dfl_loss' = sum / number of batches (validator.py:204,
    `self.loss.cpu() / len(self.dataloader)`). The loss is timed in a slot of its own, as the reference's dt[2]:
    'speed' gains 'loss' (ms per image: target preparation, the loss launches and the sum) and the other three
    slots cover what they cover without compute_loss. Not available with augment=True (TTA keeps no level maps)."""

    def __init__(self, model, nc, conf=0.001, iou=0.7, max_det=300, agnostic=False, single_cls=False, cm_conf=None,
                 augment=False, compute_loss=False):
        if compute_loss and augment:
            raise ValueError("compute_loss=True with augment=True: test-time augmentation returns no level maps, "
                             "and the reference computes no validation loss under it")
        self.model, self.nc = model, nc
        self.single_cls = bool(single_cls)
        self.compute_loss = bool(compute_loss)
        self.criterion = None
        # val.py:94-102: multi_label=True, agnostic = single_cls or agnostic_nms
        self.predictor = FusedPredictor(model, conf=conf, iou=iou, max_det=max_det,
                                        agnostic=bool(agnostic or single_cls), multi_label=True, augment=augment,
                                        keep_feats=self.compute_loss)
        self.cm_conf = conf if cm_conf is None else cm_conf  # val.py:83 ConfusionMatrix(conf=args.conf)
        self.stats = None

    def load_ema(self, trainer):
        """Evaluate the trainer's EMA weights (the reference validates self.ema.ema, engine/trainer.py:437):
        floating entries from trainer.ema_state_dict(), integer buffers from trainer.ema_int, then the predictor's
        packed operands and eval BatchNorm coefficients are refreshed (a captured graph stays valid)."""
        ema = trainer.ema_state_dict()
        with torch.no_grad():
            for k, v in self.model.state_dict().items():
                src = ema.get(k) if v.dtype.is_floating_point else trainer.ema_int.get(k)
                if src is None:
                    raise KeyError(f"load_ema: the trainer's EMA has no entry {k}")
                v.copy_(src.to(v.device))
        self.predictor.sync_weights()

    def _batch_loss(self, feats, batch, imgsz, dev):
        """The batch's three loss items (device, fp32), value-only."""
        from ..utils.loss import preprocess_targets, v8DetectionLoss
        from .trainer import FusedTrainer
        if self.criterion is None:
            self.criterion = v8DetectionLoss(self.model)
        gt = preprocess_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], feats[0].shape[0], imgsz)
        # a fixed row count per capacity bucket: the loss workspace keeps its size from batch to batch; the padded
        # zero rows are masked out by the assigner (mask_gt), as the trainer's captured steps pad theirs
        pad = torch.zeros(gt.shape[0], FusedTrainer.capacity_bucket(gt.shape[1]), 5, dtype=torch.float32, device=dev)
        if gt.shape[1]:
            pad[:, :gt.shape[1]].copy_(gt, non_blocking=True)
        with torch.no_grad():
            return self.criterion(feats, {"gt": pad})[1]

    def __call__(self, batches):
        from .. import kernels as K
        from ..native import lib
        dev = next(self.model.parameters()).device
        self.stats = stats = DetectionStats(self.nc)
        events = []
        loss_sum = torch.zeros(3, dtype=torch.float32, device=dev) if self.compute_loss else None
        nbatches = 0
        for batch in batches:
            img = batch["img"]
            if self.predictor.graph is None:
                self.predictor.capture(img.to(dev))
            e = [torch.cuda.Event(enable_timing=True) for _ in range(5 if self.compute_loss else 4)]
            e[0].record()
            img = img.to(dev, non_blocking=True)
            e[1].record()
            out, n = self.predictor.run_padded(img)[:2]
            e[2].record()
            if self.compute_loss:
                items = self._batch_loss(self.predictor.feats, batch, tuple(img.shape[2:]), dev).contiguous()
                lib.adr_axpy(3, 1.0, K.fptr(items), K.fptr(loss_sum), K.stream())
                nbatches += 1
                e[4].record()
            stats.update_batched(out, n, batch, imgsz=img.shape[2:], cm_conf=self.cm_conf,
                                 single_cls=self.single_cls)
            e[3].record()
            events.append((e, img.shape[0]))
        res = stats.results()
        if self.compute_loss:
            mean = (loss_sum.cpu() / max(nbatches, 1)).tolist()  # the one host read of the losses
            res.update(zip(LOSS_KEYS, mean))
        torch.cuda.synchronize(dev)
        seen = max(sum(b for _, b in events), 1)
        # event order per batch: 0 copy 1 forward+NMS 2 [loss 4] scaling+matching 3
        spans = [(0, 1), (1, 2), (4 if self.compute_loss else 2, 3)]
        ms = [sum(e[a].elapsed_time(e[b]) for e, _ in events) / seen for a, b in spans]
        res["speed"] = dict(zip(("preprocess", "inference", "postprocess"), ms))
        if self.compute_loss:
            res["speed"]["loss"] = sum(e[2].elapsed_time(e[4]) for e, _ in events) / seen
        return res
