from .raybatch import RayBatchDataset, ray_batch_permutation  # noqa: F401
from .llff import LLFFDatasetLoader  # noqa: F401
