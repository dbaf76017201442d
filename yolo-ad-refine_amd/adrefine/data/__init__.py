"""Training-data side of the hot path: the v8 augmentation chain with its pixel work on the GPU (augment.py), the
HBM-resident image pool (pool.py), YOLODataset (dataset.py) and the loader (build.py)."""
