"""Build-time guard of the early-ray-termination kernels (no GPU needed: hipcc cross-compiles).

csrc/termination.hip: the fused path's mark / emit kernels and the general-shape path's walk kernel compile for gfx950 without spills
or scratch.  occupancy.hip keeps its four kernels (the cell lookup moved to occupancy.h; termination.hip shares it), and the training
kernels' digest is unchanged: the feature touches none of build.KERNEL_FILES."""
import os

import pytest

from tests.test_isa_guard import HIPCC, _asm, _kernels
from tests.test_query_isa import PARENT_KERNEL_DIGEST, _clean


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return {"term": _kernels(_asm("termination")), "occ": _kernels(_asm("occupancy"))}


def test_termination_kernels_are_free_of_spills(isa):
    names = []
    for name, (body, meta) in isa["term"].items():
        _clean(name, body, meta)
        assert meta.get("vgpr_count", 999) <= 64, (name, meta)
        names.append(name)
    for frag in ("term_mark_kernel", "term_emit_kernel", "term_walk_kernel"):
        assert sum(frag in n for n in names) == 1, (frag, names)


def test_occupancy_kernels_are_all_still_there(isa):
    names = list(isa["occ"])
    for frag in ("occ_mark_kernel", "occ_scan_kernel", "occ_emit_kernel", "occ_build_kernel"):
        assert any(frag in n for n in names), (frag, names)


def test_the_training_kernels_digest_is_unchanged():
    from keras_nerf_amd import build
    assert build.kernel_digest() == PARENT_KERNEL_DIGEST
    assert "termination.hip" in build.SOURCES and "termination.hip" not in build.SLICED and "termination.h" in build.HEADERS
    assert not set(build.KERNEL_FILES) & {"termination.hip", "termination.h", "occupancy.hip", "occupancy.h", "query.hip", "query.h"}
