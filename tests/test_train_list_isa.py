"""Build-time guard of the list-mode training forward (no GPU needed: hipcc cross-compiles).

csrc/train_list.hip mlp_fwd_list_kernel<S, NET> is the SAVE instantiation of mlp_fwd_kernel (mlp_fwd.hip) behind a list prologue (compacted
entry i reads sample list[i] of the pass; workgroups past the device-side length leave before they touch LDS).  It waits on the same
hand-counted vmcnt / lgkmcnt immediates and issues the same saved-tensor stores, so: no spills, no scratch, at most 256 VGPRs, and the
same MFMA and LDS-DMA counts as mlp_fwd_kernel<S, true, NET> (978 / 254 for Shape<8, 4, 256>).  Checked for the default shape (slice 0)
and for Shape<4, 2, 128> (slice 11), for both net instantiations.  The gather kernel that prepares the compacted backward uses no scratch.
And the training kernels' digest is unchanged: the feature includes build.KERNEL_FILES but edits none of them."""
import os

import pytest

from tests.test_isa_guard import HIPCC, SLICE0, _asm, _count, _kernels
from tests.test_query_isa import PARENT_KERNEL_DIGEST, _clean

SLICE11 = ["-DKNERF_SHAPE_SLICE=11", "-DKNERF_OWN_11=,"]      # Shape<4, 2, 128> (csrc/layout.h KNERF_BUILTIN_SHAPES index 11)


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return {"s0": (_kernels(_asm("mlp_fwd", SLICE0)), _kernels(_asm("train_list", SLICE0))),
            "s11": (_kernels(_asm("mlp_fwd", SLICE11)), _kernels(_asm("train_list", SLICE11)))}


@pytest.mark.parametrize("net", [0, 1])
@pytest.mark.parametrize("slice_, shape, mfma, dma", [("s0", "ILi8ELi4ELi256EEE", 978, 254), ("s11", "ILi4ELi2ELi128EEE", None, None)])
def test_list_forward_matches_the_saving_forward_of_its_shape(isa, slice_, shape, mfma, dma, net):
    fwd, lst = isa[slice_]
    f = {k: v for k, v in fwd.items() if f"mlp_fwd_kernelINS_5Shape{shape}Lb1ELi{net}EEEvNS_7FwdArgsE" in k}
    li = {k: v for k, v in lst.items() if f"mlp_fwd_list_kernelINS_5Shape{shape}Li{net}EEEvNS_13TrainListArgsE" in k}
    assert len(f) == 1 and len(li) == 1, (sorted(fwd), sorted(lst))
    (fn, (fb, fm)), (ln, (lb, lm)) = next(iter(f.items())), next(iter(li.items()))
    _clean(ln, lb, lm)
    assert lm.get("vgpr_count", 999) <= 256, lm
    n_f, n_l = _count(fb, "v_mfma_f32_32x32x16_bf16"), _count(lb, "v_mfma_f32_32x32x16_bf16")
    assert n_l == n_f > 0, (n_l, n_f)
    d_f, d_l = _count(fb, "global_load_lds_dwordx4"), _count(lb, "global_load_lds_dwordx4")
    assert d_l == d_f > 0, (d_l, d_f)
    if mfma is not None:
        assert (n_l, d_l) == (mfma, dma)


def test_gather_kernel_is_free_of_spills(isa):
    names = [n for n in isa["s0"][1] if "occ_train_gather_kernel" in n]
    assert len(names) == 1, sorted(isa["s0"][1])
    body, meta = isa["s0"][1][names[0]]
    _clean(names[0], body, meta)
    assert not any("occ_train_gather_kernel" in n for n in isa["s11"][1])      # slice 0 alone holds it


def test_the_training_kernels_digest_is_unchanged():
    from keras_nerf_amd import build
    assert build.kernel_digest() == PARENT_KERNEL_DIGEST
    assert "train_list.hip" in build.SOURCES and "train_list.hip" in build.SLICED and "train_list.h" in build.HEADERS
    assert not set(build.KERNEL_FILES) & {"train_list.hip", "train_list.h", "occupancy.hip", "occupancy.h"}
