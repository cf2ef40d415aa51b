from .raybatch import RayBatchDataset, ray_batch_permutation  # noqa: F401
from .llff import LLFFDatasetLoader  # noqa: F401
from .cameras import CameraModel  # noqa: F401
from .colmap import ColmapDatasetLoader  # noqa: F401
