"""State-dict helpers of the reference's utils/torch_utils.py."""
from __future__ import annotations


def intersect_dicts(da, db, exclude=()):
    """utils/torch_utils.py:470-472: the entries of `da` whose key is also in `db`, contains none of the `exclude`
    substrings, and whose shape equals db's. Values are da's."""
    return {k: v for k, v in da.items() if k in db and all(x not in k for x in exclude) and v.shape == db[k].shape}
