"""Batched detection inference — the device part of the reference's predict / val loop
(engine/predictor.py:130-160 preprocess + inference, models/yolo/detect/predict.py:25-40 postprocess,
models/yolo/detect/val.py:82-99 the validator's NMS call).

One batch = the dataloader's uint8 NCHW images -> /255 (fused into the stem kernel, detect/train.py:57-59's
preprocess) -> eval forward (BatchNorm with running statistics) -> DFL decode (adr_detect_decode) ->
non_max_suppression (adr_nms). After one eager warm-up the whole chain is captured into a single hipGraph, so a
batch is one graph launch plus (for `predict`) one host read of the per-image detection counts. `predict`,
`run_padded` and `capture` take network-sized uint8 batches; `predict_images` takes raw source images of any
sizes: it letterboxes them on the device (adr_letterbox_u8, straight into the graph's input) and maps the
detections back to each source image (adr_scale_boxes).
"""
from __future__ import annotations

import torch

from .. import kernels as K
from ..utils.ops import check_counts, non_max_suppression_padded


class FusedPredictor:
    """predict(img) -> list of (n_i, 6) [x1, y1, x2, y2, conf, cls] tensors, as ops.non_max_suppression returns.

    conf / iou / max_det default to the predictor's (cfg/default.yaml: conf 0.25, iou 0.7, max_det 300); pass the
    validator's conf=0.001, multi_label=True for mAP evaluation. augment=True is the reference's test-time
    augmentation (nn/tasks.py:357-394): three forwards (scale 1, 0.83 left-right flipped, 0.67) merged before the NMS,
    boxes in the base batch's coordinates — views, forwards, merge and NMS are captured into the one hipGraph.

    keep_feats=True also keeps the eval forward's three raw level maps (B, 4*reg_max + nc, Hi, Wi) — the reference's
    preds[1], what model.loss(batch, preds) evaluates (engine/validator.py:184): run_padded then returns
    (out, n, feats), and `feats` holds the last run's maps. After capture() they are the graph's own output tensors
    (`static_feats`): each replay rewrites them in place, so they stay valid (and are overwritten by the next batch).
    Without keep_feats nothing of the forward is kept and the graph is the same as before. The reference's TTA
    returns no level maps (tasks.py:372 `return torch.cat(y, -1), None`), so keep_feats with augment is refused."""

    def __init__(self, model, conf=0.25, iou=0.7, max_det=300, agnostic=False, multi_label=False, classes=None,
                 augment=False, keep_feats=False):
        if keep_feats and augment:
            raise ValueError("keep_feats=True with augment=True: test-time augmentation returns no level maps "
                             "(and the reference computes no loss under it)")
        self.model = model
        self.augment = bool(augment)
        self.keep_feats = bool(keep_feats)
        self.feats = None
        self.static_feats = None
        self.conf, self.iou, self.max_det = conf, iou, max_det
        self.agnostic, self.multi_label, self.classes = agnostic, multi_label, classes
        self.graph = None
        self.static_in = None
        self.static_out = None
        # bf16 conv operands and the eval BatchNorm scale/shift computed once, not per batch (weights are fixed here)
        self.packs = K.PackCache(cache_bn_coefs=True)
        from ..nn.tasks import register_dependent
        register_dependent(model, self)  # DetectionModel.load then calls sync_weights: no predict with the old folded weights

    def sync_weights(self):
        """Repack the bf16 conv operands and recompute the eval BatchNorm coefficients after the model's weights or
        running statistics changed (e.g. between training epochs, or DetectionModel.load). In place: a captured graph
        reads the same buffers and needs no new capture."""
        self.packs.pack_all()
        self.packs.refresh_bn_coefs()

    def _run(self, img):
        with torch.no_grad(), K.pack_scope(self.packs):
            first = not self.packs.valid
            y = self.model(img, augment=True) if self.augment else self.model(img)
            if first and self.packs.specs:
                self.packs.valid = True  # the recording forward packed every operand into the cache
            if self.keep_feats:
                if not (isinstance(y, (list, tuple)) and len(y) == 2 and y[1] is not None):
                    raise RuntimeError("keep_feats=True: the model's eval forward returned no level maps")
                self.feats = list(y[1])
            y = y[0] if isinstance(y, (list, tuple)) else y
            res = non_max_suppression_padded(y, self.conf, self.iou, self.classes, self.agnostic,
                                             self.multi_label, self.max_det)
            return (*res, self.feats) if self.keep_feats else res

    def capture(self, img):
        """Record preprocess + forward + decode + NMS for batches shaped like `img` into one hipGraph (run one
        eager batch first so lazy caches and the NMS workspace exist)."""
        self.model.eval()
        self.static_in = img.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._run(self.static_in)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            self.static_out = self._run(self.static_in)
        self.static_feats = self.static_out[2] if self.keep_feats else None
        self.graph = g

    def run_padded(self, img):
        """(out (B, max_det, 6), n (B,) int32) on the device, no host sync; with keep_feats (out, n, feats)."""
        self.model.eval()
        if self.graph is not None and img.shape == self.static_in.shape and img.dtype == self.static_in.dtype:
            if img.data_ptr() != self.static_in.data_ptr():
                self.static_in.copy_(img, non_blocking=True)
            self.graph.replay()
            self.feats = self.static_feats
            return self.static_out
        return self._run(img)

    def predict(self, img):
        out, n = self.run_padded(img)[:2]
        counts = n.tolist()
        check_counts(counts, out.device)
        return [out[i, :k].clone() for i, k in enumerate(counts)]

    def predict_images(self, imgs, imgsz=None):
        """The reference's predict on raw images (engine/predictor.py:125, 144-156 letterbox + BGR -> RGB + CHW;
        models/yolo/detect/predict.py postprocess with ops.scale_boxes): `imgs` is a list of HWC BGR uint8 numpy
        images of any sizes; returns the list of (n_i, 6) tensors in each source image's own coordinates.

        With a captured graph, 1 <= len(imgs) <= B of the captured batch: every image is letterboxed (auto=False) to
        the captured (H, W) by adr_letterbox_u8 directly into the graph's static input (unused slots are filled with
        114 and their outputs dropped), the graph is replayed, adr_scale_boxes maps the padded output back in place
        and the per-image counts are the one host read. Without a graph the batch runs eagerly at `imgsz` (int or
        (h, w)). The reference's auto=True minimum rectangle for batches of same-shape images is not used: the
        shapes are fixed by the graph."""
        from ..data.augment import render_letterbox
        from ..kernels import fptr, stream
        from ..native import lib
        from ..utils.ops import scale_boxes_table, scale_gain_pad
        imgs = list(imgs)
        if self.graph is not None and imgsz is None:
            B, _, H, W = self.static_in.shape
            if not 1 <= len(imgs) <= B:
                raise ValueError(f"predict_images: {len(imgs)} images for a graph captured at batch {B}")
            batch, _ = render_letterbox(imgs, (H, W), out=self.static_in, rgb=True, auto=False)
        else:
            if imgsz is None:
                raise ValueError("predict_images: without a captured graph pass imgsz")
            H, W = (imgsz, imgsz) if isinstance(imgsz, int) else imgsz
            if not imgs:
                raise ValueError("predict_images: no images")
            dev = next(self.model.parameters()).device
            batch, _ = render_letterbox(imgs, (H, W), device=dev, rgb=True, auto=False)
        out, n = self.run_padded(batch)[:2]
        rows = []
        for i in range(out.shape[0]):
            h0, w0 = imgs[i].shape[:2] if i < len(imgs) else (H, W)
            gain, pad = scale_gain_pad((H, W), (h0, w0))
            rows.append((gain, pad[0], pad[1], w0, h0))
        tab = scale_boxes_table(rows, out.device)
        lib.adr_scale_boxes(fptr(out), fptr(n), fptr(tab), out.shape[0], out.shape[1], out.shape[2], 0, stream())
        counts = n.tolist()
        check_counts(counts, out.device)
        return [out[i, :counts[i]].clone() for i in range(len(imgs))]

    __call__ = predict
