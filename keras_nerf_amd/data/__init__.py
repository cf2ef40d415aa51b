from .raybatch import RayBatchDataset, ray_batch_permutation  # noqa: F401
