"""multi_scale's size draw (engine/trainer.multi_scale_shape) against a literal restatement of the reference's lines
(models/yolo/detect/train.py:60-71) under one seeded random.Random each: every returned shape, the set of sizes, and
the generator's state afterwards (one randrange per call, drawn even when the result is 1:1)."""
import math
import random

import pytest
import torch

from adrefine.engine.trainer import FusedTrainer, multi_scale_shape


def _reference_draw(rng, imgsz, stride, hw):
    """detect/train.py:60-71 with self.args.imgsz, self.stride and imgs.shape[2:] as arguments: the new shape the
    reference interpolates to, or None where it leaves the batch alone (sf == 1)."""
    sz = (
        rng.randrange(int(imgsz * 0.5), int(imgsz * 1.5 + stride))
        // stride
        * stride
    )  # size
    sf = sz / max(hw)  # scale factor
    if sf != 1:
        ns = [
            math.ceil(x * sf / stride) * stride for x in hw
        ]  # new shape (stretched to gs-multiple)
        return ns
    return None


@pytest.mark.parametrize("imgsz,hw", [(640, (640, 640)), (256, (256, 256)), (256, (256, 320)), (640, (512, 640))])
def test_shape_draws_are_the_references(imgsz, hw):
    stride, n = 32, 4000
    ours, ref = random.Random(1234), random.Random(1234)
    got = [multi_scale_shape(imgsz, stride, torch.Size(hw), rng=ours) for _ in range(n)]
    want = [_reference_draw(ref, imgsz, stride, torch.Size(hw)) for _ in range(n)]
    assert got == want
    assert ours.getstate() == ref.getstate()  # the same number of draws, 1:1 results included
    assert any(s is None for s in got) and any(s is not None for s in got)
    for s in got:
        assert s is None or (len(s) == 2 and all(isinstance(v, int) and v % stride == 0 and v > 0 for v in s))


def test_sizes_at_640_are_320_to_960():
    rng = random.Random(7)
    got = [multi_scale_shape(640, 32, (640, 640), rng=rng) for _ in range(4000)]
    sizes = {640 if s is None else s[0] for s in got}
    assert sizes == set(range(320, 961, 32)) and len(sizes) == 21
    assert all(s is None or s[0] == s[1] for s in got)
    assert [640, 640] not in got  # a 1:1 draw is None: the batch stays uint8


def test_default_rng_is_the_random_module():
    random.seed(99)
    a = [multi_scale_shape(256, 32, (256, 256)) for _ in range(50)]
    ref = random.Random(99)
    assert a == [_reference_draw(ref, 256, 32, (256, 256)) for _ in range(50)]


def test_multi_scale_needs_imgsz():
    with pytest.raises(ValueError, match="imgsz"):
        FusedTrainer(torch.nn.Linear(2, 2), multi_scale=True)
