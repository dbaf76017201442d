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
    boxes in the base batch's coordinates — views, forwards, merge and NMS are captured into the one hipGraph."""

    def __init__(self, model, conf=0.25, iou=0.7, max_det=300, agnostic=False, multi_label=False, classes=None,
                 augment=False):
        self.model = model
        self.augment = bool(augment)
        self.conf, self.iou, self.max_det = conf, iou, max_det
        self.agnostic, self.multi_label, self.classes = agnostic, multi_label, classes
        self.graph = None
        self.static_in = None
        self.static_out = None
        # bf16 conv operands and the eval BatchNorm scale/shift computed once, not per batch (weights are fixed here)
        self.packs = K.PackCache(cache_bn_coefs=True)

    def sync_weights(self):
        """Repack the bf16 conv operands and recompute the eval BatchNorm coefficients after the model's weights or
        running statistics changed (e.g. between training epochs)."""
        self.packs.pack_all()
        self.packs.refresh_bn_coefs()

    def _run(self, img):
        with torch.no_grad(), K.pack_scope(self.packs):
            first = not self.packs.valid
            y = self.model(img, augment=True) if self.augment else self.model(img)
            if first and self.packs.specs:
                self.packs.valid = True  # the recording forward packed every operand into the cache
            y = y[0] if isinstance(y, (list, tuple)) else y
            return non_max_suppression_padded(y, self.conf, self.iou, self.classes, self.agnostic,
                                              self.multi_label, self.max_det)

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
        self.graph = g

    def run_padded(self, img):
        """(out (B, max_det, 6), n (B,) int32) on the device, no host sync."""
        self.model.eval()
        if self.graph is not None and img.shape == self.static_in.shape and img.dtype == self.static_in.dtype:
            if img.data_ptr() != self.static_in.data_ptr():
                self.static_in.copy_(img, non_blocking=True)
            self.graph.replay()
            return self.static_out
        return self._run(img)

    def predict(self, img):
        out, n = self.run_padded(img)
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
        out, n = self.run_padded(batch)
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
