"""Build-time guard of the occupancy-grid kernels (no GPU needed: hipcc cross-compiles).

csrc/query.hip query_list_kernel<S>: the render pass's live samples through the inference chain of query_kernel<S> (a third prologue
that reads a device list; workgroups past the list's length leave before they touch LDS).  It waits on the same hand-counted vmcnt /
lgkmcnt immediates, so, as for query_kernel: no spills, no scratch, and the same MFMA and LDS-DMA counts as the query kernel of its
shape (978 / 254 for Shape<8, 4, 256>).  Checked for the default shape (slice 0) and for Shape<4, 2, 128> (slice 11).
csrc/occupancy.hip: the mark / scan / emit / build kernels use no scratch.
And the training kernels' digest is unchanged: the feature touches none of build.KERNEL_FILES."""
import os

import pytest

from tests.test_isa_guard import HIPCC, SLICE0, _asm, _count, _kernels
from tests.test_query_isa import PARENT_KERNEL_DIGEST, _clean

SLICE11 = ["-DKNERF_SHAPE_SLICE=11", "-DKNERF_OWN_11=,"]      # Shape<4, 2, 128> (csrc/layout.h KNERF_BUILTIN_SHAPES index 11)


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return {"s0": _kernels(_asm("query", SLICE0)), "s11": _kernels(_asm("query", SLICE11)), "occ": _kernels(_asm("occupancy", SLICE0))}


def _pair(ks, shape):
    q = {k: v for k, v in ks.items() if "query_kernelINS_5Shape" + shape in k}
    lst = {k: v for k, v in ks.items() if "query_list_kernelINS_5Shape" + shape in k}
    assert len(q) == 1 and len(lst) == 1, sorted(ks)
    return next(iter(q.items())), next(iter(lst.items()))


@pytest.mark.parametrize("slice_, shape, mfma", [("s0", "ILi8ELi4ELi256EEE", 978), ("s11", "ILi4ELi2ELi128EEE", None)])
def test_list_kernel_matches_the_query_kernel_of_its_shape(isa, slice_, shape, mfma):
    (qn, (qb, qm)), (ln, (lb, lm)) = _pair(isa[slice_], shape)
    _clean(ln, lb, lm)
    assert lm.get("vgpr_count", 999) <= 256, lm
    n_q, n_l = _count(qb, "v_mfma_f32_32x32x16_bf16"), _count(lb, "v_mfma_f32_32x32x16_bf16")
    assert n_l == n_q > 0, (n_l, n_q)
    if mfma is not None:
        assert n_l == mfma
    assert _count(lb, "global_load_lds_dwordx4") == _count(qb, "global_load_lds_dwordx4") > 0


def test_occupancy_kernels_are_free_of_spills(isa):
    names = []
    for name, (body, meta) in isa["occ"].items():
        _clean(name, body, meta)
        names.append(name)
    for frag in ("occ_mark_kernel", "occ_scan_kernel", "occ_emit_kernel", "occ_build_kernel"):
        assert any(frag in n for n in names), (frag, names)


def test_the_training_kernels_digest_is_unchanged():
    from keras_nerf_amd import build
    assert build.kernel_digest() == PARENT_KERNEL_DIGEST
    assert "occupancy.hip" in build.SOURCES and "occupancy.hip" not in build.SLICED
    assert not set(build.KERNEL_FILES) & {"occupancy.hip", "occupancy.h", "query.hip", "query.h"}
