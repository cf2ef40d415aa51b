"""Build-time guard of the two kernel files the point / grid queries and the mesh export add (no GPU needed: hipcc cross-compiles).

csrc/query.hip: query_kernel<S> is the inference chain of mlp_fwd.hip behind another prologue and epilogue, so it waits on the same
hand-counted vmcnt / lgkmcnt immediates (chain.h; a plain wait table, no saved-tensor stores).  As test_isa_guard.py does for the
three big kernels: no VGPR/SGPR spills, no private segment, no scratch instruction, and the instruction counts the tables imply.
Default shape Shape<8, 4, 256>: MFMA = kFwdBlocks = 978 (layer_0 4 x 8, seven 256x256 layers 16 x 8, the concat layer 4 more k-steps
x 8 tiles, head 16 + 2 = 18: 32 + 6 x 128 + 160 + 18 = 978); LDS-DMA 2 x (5 prologue pages + 61 + 61 barriers) = 254.
csrc/mesh.hip: no spills or scratch in any of its kernels.
Also: adding them changed nothing the training kernels are built from (build.kernel_digest, which bench.py quotes)."""
import os
import re

import pytest

from tests.test_isa_guard import HIPCC, SLICE0, _asm, _count, _kernels

PARENT_KERNEL_DIGEST = "46ecbcca9812e9d0"      # build.kernel_digest() of the tree before the query / mesh files existed


def _clean(name, body, meta):
    assert meta.get("vgpr_spill_count") == 0 and meta.get("sgpr_spill_count") == 0, (name, meta)
    assert meta.get("private_segment_fixed_size") == 0, (name, meta)
    assert not re.search(r"^\s+scratch_", body, re.M), f"{name}: scratch instruction"
    assert not re.search(r"^\s+buffer_(load|store)", body, re.M), f"{name}: buffer access (stack?)"


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return {"query": _kernels(_asm("query", SLICE0)), "mesh": _kernels(_asm("mesh", SLICE0))}


def test_query_kernel_of_the_default_shape_matches_its_wait_tables(isa):
    ks = {k: v for k, v in isa["query"].items() if "query_kernelINS_5ShapeILi8ELi4ELi256EEE" in k}
    assert len(ks) == 1, sorted(isa["query"])
    for name, (body, meta) in ks.items():
        _clean(name, body, meta)
        assert _count(body, "v_mfma_f32_32x32x16_bf16") == 978
        assert _count(body, "global_load_lds_dwordx4") == 254
        assert meta.get("vgpr_count", 999) <= 256, meta
        vm = set(re.findall(r"s_waitcnt vmcnt\((\d+)\)", body))
        assert len(vm) >= 2 and re.search(r"s_waitcnt lgkmcnt\(3\)", body), sorted(vm)


def test_every_query_and_mesh_kernel_is_free_of_spills(isa):
    names = []
    for f in ("query", "mesh"):
        for name, (body, meta) in isa[f].items():
            _clean(name, body, meta)
            names.append(name)
    for frag in ("query_gather_kernel", "query_scatter_kernel", "edge_flag_kernel", "cube_count_kernel", "vertex_emit_kernel",
                 "face_emit_kernel", "scan_block_kernel", "scan_add_kernel"):
        assert any(frag in n for n in names), (frag, names)


def test_the_training_kernels_digest_is_unchanged():
    from keras_nerf_amd import build
    assert build.kernel_digest() == PARENT_KERNEL_DIGEST
    assert not set(build.KERNEL_FILES) & {"query.hip", "query.h", "mesh.hip", "mesh_table.h"}
