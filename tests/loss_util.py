"""Shared pieces of the detection-loss edge-case tests (test infrastructure): seeded scenarios for v8DetectionLoss
(head outputs + labels) that reach the branches random square fixtures never reach, the oracle's assignment taken
apart far enough to state what each scenario covers, and the stability margins of the assigner.

  scenario(name) -> (feats, batch, nc, (H, W)): three NCHW fp32 CPU head outputs (strides 8, 16, 32), the label
                    batch {batch_idx (n,), cls (n, 1), bboxes (n, 4) normalised xywh}, the class count, the image size.
  trace(name)    -> the oracle's intermediates (align, overlaps, masks, fg, targets, SlideLoss mu ...).
  margins(name)  -> (top-k gap, argmax gap): how far the oracle's discrete decisions are from flipping.
  oracle(name)   -> loss, items, gradients, fg mask of oracle.detection_loss on the CPU.

Every shape has A >= 640 anchors: the kernel's top-10 reproduces the selection of torch.topk's CPU partial_sort, and
torch only takes that path when 10 * 64 <= A. The scenario tensors are cached: callers do not write into them."""
import functools
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "oracle"))
import adr_oracle as O  # noqa: E402

STRIDES = (8, 16, 32)
RM = 16
NAMES = ("random_nonsquare", "trained", "trained_nonsquare", "no_labels", "empty_image", "many_labels", "overlap",
         "degenerate", "nc8", "nc16", "nc96", "exact_ties")
GOLDEN = ("trained_nonsquare", "exact_ties")  # scenarios with a reference fixture tests/golden/loss_edge_<name>.npz
# bf16 head outputs (the v_rcp / __logf softplus path): bound on |loss - oracle(rounded inputs)| / |oracle|.
# 4 x the largest deviation measured on the MI355X over all scenarios: 4.890e-07 (trained; loss_320_bs4: 2.578e-07).
BF16_LOSS_RTOL = 4 * 4.890e-07


def _randn_feats(B, nc, H, W, seed):
    """The recipe of the loss_* fixtures: randn head outputs, x2 on the 64 box channels."""
    gen = torch.Generator().manual_seed(seed)
    feats = [torch.randn(B, 4 * RM + nc, H // s, W // s, generator=gen) for s in STRIDES]
    for f in feats:
        f[:, :4 * RM] *= 2.0
    return feats


def _batch(rows, H, W):
    """rows: (image, class, cx, cy, w, h) in pixels -> the dataloader's normalised label batch."""
    if not rows:
        return {"batch_idx": torch.zeros(0), "cls": torch.zeros(0, 1), "bboxes": torch.zeros(0, 4)}
    t = torch.tensor(rows, dtype=torch.float64)
    box = t[:, 2:6] / torch.tensor([W, H, W, H], dtype=torch.float64)
    return {"batch_idx": t[:, 0].float(), "cls": t[:, 1:2].float(), "bboxes": box.float()}


def _rand_rows(counts, nc, H, W, seed, lo=16.0, hi=0.6):
    """counts[b] labels per image: centres uniform, sides log-uniform in [lo px, hi * side], kept inside the image."""
    gen = torch.Generator().manual_seed(seed)
    rows = []
    for b, n in enumerate(counts):
        for _ in range(n):
            u = torch.rand(5, generator=gen, dtype=torch.float64).tolist()
            w = math.exp(math.log(lo) + (math.log(hi * W) - math.log(lo)) * u[2])
            h = math.exp(math.log(lo) + (math.log(hi * H) - math.log(lo)) * u[3])
            cx = w / 2 + (W - w) * u[0]
            cy = h / 2 + (H - h) * u[1]
            rows.append((b, int(u[4] * nc) % nc, cx, cy, w, h))
    return rows


def _train_like(feats, rows, nc, seed, noise=1.2):
    """What a trained head puts out, written over randn features: at every anchor whose centre lies inside a label
    (the smallest such label), each side's 16 DFL logits are a soft peak (width 0.7 bins) at the true distance to
    the label's edge plus seeded noise, the label's class logit is raised and the other classes are lowered."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.arange(RM, dtype=torch.float32).view(1, RM, 1, 1)
    for f, s in zip(feats, STRIDES):
        h, w = f.shape[2:]
        ys = ((torch.arange(h, dtype=torch.float32) + 0.5) * s).view(h, 1)
        xs = ((torch.arange(w, dtype=torch.float32) + 0.5) * s).view(1, w)
        for b, c, cx, cy, bw, bh in sorted(rows, key=lambda r: -r[4] * r[5]):
            x1, y1, x2, y2 = cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2
            m = (xs > x1) & (xs < x2) & (ys > y1) & (ys < y2)
            d = torch.stack(((xs - x1).expand(h, w), (ys - y1).expand(h, w), (x2 - xs).expand(h, w),
                             (y2 - ys).expand(h, w))) / s
            lg = -(q - d.clamp(0, RM - 1).unsqueeze(1)) ** 2 / (2 * 0.7 ** 2)
            lg = lg + noise * torch.randn(4, RM, h, w, generator=gen)
            cl = 0.5 * torch.randn(nc, h, w, generator=gen) - 3.0
            cl[c] = 0.5 * torch.randn(h, w, generator=gen) + 2.0
            new = torch.cat((lg.view(4 * RM, h, w), cl))
            f[b] = torch.where(m, new, f[b])
    return feats


# ---- exact_ties: every number exactly representable (in bf16 too) ----
# (image, class, x1, y1, x2, y2) in pixels. Edges = stride/2 mod stride of one level, so that level's anchors are a
# whole number of cells away from every edge: stride 8 for the first two, 16 for the third, 32 for the fourth.
_TIE_BOXES = ((0, 3, 36, 44, 132, 108), (0, 7, 156, 148, 220, 228), (1, 1, 40, 24, 168, 136), (1, 5, 48, 144, 208, 240))


def _tie_q(dn, df):
    """First of the two equal bins (q, q + 2; decoded distance q + 1) for a side at distance dn whose opposite side
    is at df: the true distance where dn * df is no multiple of 3 (decoded edge == label edge, bit for bit, at the
    level whose cells the label's edges follow), one cell further otherwise. Symmetric under dn <-> df, so anchors
    mirrored about the box centre predict mirrored boxes."""
    dec = torch.round(dn) + ((torch.round(dn) * torch.round(df)) % 3 == 0).float()
    return (dec - 1).clamp(0, RM - 3)


def _exact_ties():
    H = W = 256
    nc, B = 80, 2
    feats = []
    for s in STRIDES:
        h, w = H // s, W // s
        f = torch.zeros(B, 4 * RM + nc, h, w)
        iy = torch.arange(h).view(h, 1).expand(h, w)
        ix = torch.arange(w).view(1, w).expand(h, w)
        f[:, 4 * RM:] = -4.0 + 0.5 * ((ix + 2 * iy) % 4).float()  # background class logits in {-4, ..., -2.5}
        ys, xs = (iy.float() + 0.5) * s, (ix.float() + 0.5) * s
        qs = torch.arange(RM).view(RM, 1, 1)
        for b, c, x1, y1, x2, y2 in _TIE_BOXES:
            m = (xs > x1) & (xs < x2) & (ys > y1) & (ys < y2)
            d = [(xs - x1) / s, (ys - y1) / s, (x2 - xs) / s, (y2 - ys) / s]
            new = torch.full((4 * RM + nc, h, w), -4.0)
            for k in range(4):
                qk = _tie_q(d[k], d[(k + 2) % 4]).long().unsqueeze(0)
                new[k * RM:(k + 1) * RM] = torch.where((qs == qk) | (qs == qk + 2), 0.0, -64.0)
            new[4 * RM + c] = 2.0
            f[b] = torch.where(m, new, f[b])
        feats.append(f)
    rows = [(b, c, (x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1) for b, c, x1, y1, x2, y2 in _TIE_BOXES]
    return feats, _batch(rows, H, W), nc, (H, W)


def _overlap_rows():
    rows = [(0, 4, 96, 96, 120, 100), (0, 9, 96, 96, 60, 50), (0, 9, 98, 97, 64, 52), (0, 2, 94, 99, 58, 54),
            (0, 11, 100, 92, 66, 48), (0, 4, 96, 96, 24, 20),  # nested and heavily overlapping around one centre
            (1, 6, 80, 110, 90, 70), (1, 13, 80, 110, 90, 70),  # an exact duplicate pair, different classes
            (1, 6, 84, 106, 84, 74), (1, 3, 120, 70, 80, 90), (1, 3, 116, 74, 76, 84)]
    return rows


def _degenerate_rows():
    return [(0, 1, 70, 90, 0, 60),  # zero width
            (0, 2, 120, 50, 50, 0),  # zero height
            (0, 3, 96, 96, 192, 192),  # the whole image
            (0, 5, 60, 140, 40, 36),
            (1, 4, 172.8, 172.8, 76.8, 76.8),  # reaches past the right and bottom edge
            (1, 6, 64, 64, 2, 2),  # 2 px around a cell corner of every level: holds no anchor centre
            (1, 7, 70, 60, 56, 44)]


def _many_rows(H, W):
    """Image 0: 70 small labels; image 1: none; image 2: two flat boxes wider than 15 stride-8 cells, each holding two
    rows of stride-8 anchor centres and no centre of another level, so their positives sit at stride 8 with the far
    side's DFL target on the reg_max - 1.01 clamp."""
    rows = _rand_rows((70,), 80, H, W, seed=71, lo=7.0, hi=0.09)
    rows += [(2, 8, 128, 64, 250, 14), (2, 12, 126, 128, 244, 14)]
    return rows


@functools.lru_cache(maxsize=None)
def scenario(name):
    if name == "random_nonsquare":
        H, W, nc = 160, 256, 80
        return _randn_feats(3, nc, H, W, 101), _batch(_rand_rows((3, 5, 2), nc, H, W, 102), H, W), nc, (H, W)
    if name in ("trained", "trained_nonsquare"):
        H, W = (192, 192) if name == "trained" else (160, 256)
        nc, seed = 80, 324
        rows = _rand_rows((4, 3), nc, H, W, seed, lo=24.0)
        feats = _train_like(_randn_feats(2, nc, H, W, seed + 1), rows, nc, seed + 2)
        return feats, _batch(rows, H, W), nc, (H, W)
    if name == "no_labels":
        return _randn_feats(2, 80, 192, 192, 131), _batch([], 192, 192), 80, (192, 192)
    if name == "empty_image":  # nmax = 7, B * nmax = 21
        rows = [r if r[0] == 0 else (2, *r[1:]) for r in _rand_rows((7, 4), 80, 192, 192, 142)]
        return _randn_feats(3, 80, 192, 192, 141), _batch(rows, 192, 192), 80, (192, 192)
    if name == "many_labels":
        H, W = 160, 256
        return _randn_feats(3, 80, H, W, 151), _batch(_many_rows(H, W), H, W), 80, (H, W)
    if name == "overlap":
        return _randn_feats(2, 80, 192, 192, 174), _batch(_overlap_rows(), 192, 192), 80, (192, 192)
    if name == "degenerate":
        return _randn_feats(2, 80, 192, 192, 171), _batch(_degenerate_rows(), 192, 192), 80, (192, 192)
    if name in ("nc8", "nc16", "nc96"):
        nc = int(name[2:])
        return (_randn_feats(2, nc, 192, 192, 180 + nc), _batch(_rand_rows((3, 4), nc, 192, 192, 280 + nc), 192, 192),
                nc, (192, 192))
    if name == "exact_ties":
        return _exact_ties()
    raise KeyError(name)


def inputs(name, dtype=None):
    """The scenario's features as the kernel sees them in `dtype`: rounded to it, held in fp32."""
    feats, batch, nc, hw = scenario(name)
    if dtype is not None and dtype != torch.float32:
        feats = [f.to(dtype).float() for f in feats]
    return feats, batch, nc, hw


@functools.lru_cache(maxsize=None)
def trace(name, dtype=None):
    """oracle.detection_loss up to the assignment, taken apart: the calls and expressions of detection_loss /
    tal_assign on the same inputs, keeping the intermediates."""
    feats, batch, nc, (H, W) = inputs(name, dtype)
    B, no = feats[0].shape[0], nc + 4 * RM
    pd, ps = torch.cat([f.view(B, no, -1) for f in feats], 2).split((4 * RM, nc), 1)
    ps, pd = ps.permute(0, 2, 1).contiguous(), pd.permute(0, 2, 1).contiguous()
    anc, st = O.make_anchors([f.shape[2:] for f in feats], STRIDES)
    tg = O.preprocess_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], B, torch.tensor([float(H), float(W)]))
    gt_labels, gt_bboxes = tg.split((1, 4), 2)
    mask_gt = gt_bboxes.sum(2, keepdim=True).gt(0)
    A, nmax = pd.shape[1], tg.shape[1]
    pbox = O.dist2bbox(pd.view(B, A, 4, RM).softmax(3).matmul(torch.arange(RM, dtype=torch.float32)), anc, xywh=False)
    scores = ps.sigmoid()
    t_labels, t_bboxes, t_scores, fg, tgi = O.tal_assign(scores, pbox * st, anc * st, gt_labels, gt_bboxes, mask_gt, nc)
    out = dict(B=B, A=A, nmax=nmax, nc=nc, anc=anc, st=st, pbox=pbox, gt=tg, mask_gt=mask_gt, fg=fg, tgi=tgi,
               t_scores=t_scores, n_fg=int(fg.sum()))
    if nmax:
        lt, rb = gt_bboxes.view(-1, 1, 4).chunk(2, 2)
        deltas = torch.cat(((anc * st)[None] - lt, rb - (anc * st)[None]), 2).view(B, nmax, A, -1)
        in_gts = deltas.amin(3).gt(1e-9)
        m = in_gts & mask_gt
        ov = O.bbox_iou_ciou(gt_bboxes.unsqueeze(2).expand(-1, -1, A, -1), (pbox * st).unsqueeze(1)).squeeze(-1)
        ov = torch.where(m, ov.clamp(0), torch.zeros(()))
        lab = gt_labels.squeeze(-1).long().clamp(0, nc - 1)
        sc = torch.where(m, scores.permute(0, 2, 1).gather(1, lab.unsqueeze(-1).expand(-1, -1, A)), torch.zeros(()))
        align = sc.pow(0.5) * ov.pow(6.0)
        out.update(in_gts=in_gts, overlaps=ov, align=align)
    if out["n_fg"]:
        tb = (t_bboxes / st)[fg]
        out["ciou_fg"] = O.bbox_iou_ciou(pbox[fg], tb).squeeze(-1)
        out["mu"] = max(float(out["ciou_fg"].mean()), 0.2)
        out["tltrb_fg"] = torch.cat((anc.expand(B, -1, -1)[fg] - tb[:, :2], tb[:, 2:] - anc.expand(B, -1, -1)[fg]), -1)
        out["tbox_fg"], out["pbox_fg"] = tb, pbox[fg]
    return out


def topk_rows(name, dtype=None):
    """Per (image, label) row with mask_gt: (10th, 11th) largest align value."""
    t = trace(name, dtype)
    if not t["nmax"]:
        return []
    v = t["align"].sort(-1, descending=True).values
    return [(float(v[b, j, 9]), float(v[b, j, 10])) for b in range(t["B"]) for j in range(t["nmax"])
            if t["mask_gt"][b, j, 0]]


def claimants(name, dtype=None):
    """(B, nmax, A) bool: label j holds anchor a in its top-10, inside the box (mask_pos before the overlap argmax):
    the oracle's own lines (tal_assign)."""
    t = trace(name, dtype)
    idx = torch.topk(t["align"], 10, dim=-1, largest=True).indices
    idx = idx.masked_fill(~t["mask_gt"].expand(-1, -1, 10), 0)
    count = torch.zeros(t["align"].shape, dtype=torch.int8)
    ones = torch.ones_like(idx[:, :, :1], dtype=torch.int8)
    for k in range(10):
        count.scatter_add_(-1, idx[:, :, k:k + 1], ones)
    count.masked_fill_(count > 1, 0)
    return count.bool() & t["in_gts"] & t["mask_gt"]


def margins(name, dtype=None):
    """(top-k gap, argmax gap) of the oracle's assignment, both relative; inf where nothing can flip.
    Top-k gap: min over label rows of (v10 - v11) / v10, rows whose cut is an exact tie left out (the kernel makes
    the selection torch.topk makes among equal values). Argmax gap: at anchors claimed by more than one label, the
    best overlap against the best overlap of a label with a different box (identical boxes tie exactly; argmax then
    takes the first, in kernel and oracle alike)."""
    t = trace(name, dtype)
    if not t["nmax"]:
        return math.inf, math.inf
    gaps = [(a - b) / a for a, b in topk_rows(name, dtype) if a != b]
    cl = claimants(name, dtype)
    amin = math.inf
    for b, a in (cl.sum(1) > 1).nonzero().tolist():
        o = t["overlaps"][b, :, a]
        j = int(o.argmax())
        other = [float(o[k]) for k in range(t["nmax"]) if not torch.equal(t["gt"][b, k, 1:], t["gt"][b, j, 1:])]
        if other and float(o[j]) > 0:
            amin = min(amin, (float(o[j]) - max(other)) / float(o[j]))
    return (min(gaps) if gaps else math.inf), amin


@functools.lru_cache(maxsize=None)
def oracle(name, dtype=None):
    """oracle.detection_loss and its gradient on the CPU: dict(loss, items, grads [NCHW per level], fg (B, A), n_fg)."""
    feats, batch, nc, _ = inputs(name, dtype)
    fs = [f.clone().requires_grad_(True) for f in feats]
    loss, items = O.detection_loss(fs, batch["batch_idx"], batch["cls"], batch["bboxes"], nc=nc)
    loss.backward()
    t = trace(name, dtype)
    return dict(loss=loss.detach(), items=items, grads=[f.grad for f in fs], fg=t["fg"], n_fg=t["n_fg"])


def box_grad_rows(grads, nc):
    """(B, A) bool: anchors whose 64 box-channel gradients are not all zero (levels concatenated in anchor order)."""
    B = grads[0].shape[0]
    g = torch.cat([x.detach().float().cpu().reshape(B, 4 * RM + nc, -1)[:, :4 * RM] for x in grads], 2)
    return (g != 0).any(1)
