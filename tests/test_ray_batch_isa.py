"""Build-time guard of the ray-batch kernel (no GPU needed: hipcc cross-compiles).

csrc/raybatch.hip: `raybatch_kernel` compiles for gfx950 without spills or scratch.  csrc/raygen.hip keeps `raygen_kernel` (its ray
arithmetic moved to rays.h, which raybatch.hip shares), and the training kernels' digest is unchanged: the feature touches none of
build.KERNEL_FILES."""
import os

import pytest

from tests.test_isa_guard import HIPCC, _asm, _kernels
from tests.test_query_isa import PARENT_KERNEL_DIGEST, _clean


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return {"raybatch": _kernels(_asm("raybatch")), "raygen": _kernels(_asm("raygen"))}


def test_the_ray_batch_kernel_is_free_of_spills(isa):
    names = list(isa["raybatch"])
    assert sum("raybatch_kernel" in n for n in names) == 1, names
    for name, (body, meta) in isa["raybatch"].items():
        _clean(name, body, meta)
        assert meta.get("vgpr_count", 999) <= 64, (name, meta)


def test_raygen_kernel_is_still_there_and_clean(isa):
    names = list(isa["raygen"])
    assert sum("raygen_kernel" in n for n in names) == 1, names
    for name, (body, meta) in isa["raygen"].items():
        _clean(name, body, meta)


def test_the_training_kernels_digest_is_unchanged():
    from keras_nerf_amd import build
    assert build.kernel_digest() == PARENT_KERNEL_DIGEST
    assert "raybatch.hip" in build.SOURCES and "raybatch.hip" not in build.SLICED and "rays.h" in build.HEADERS
    assert "raygen.hip" in build.SOURCES
    assert not set(build.KERNEL_FILES) & {"raybatch.hip", "rays.h", "raygen.hip"}
