"""Build-level guard for the duplicate-group kernels (CPU only: hipcc
cross-compiles gfx950 here; skipped where hipcc is absent), in the manner of
tests/test_kernel_resources_self.py: the components mode of gemm_f32_kernel
(mode 4: the 128 x 128 variant with and without resident query rows and the
256 x 256 variant, three metrics each) and the two forest kernels of
pmm_range.hip use no scratch.  Reads the resource metadata and counts scratch
instructions only."""
import os
import re
import subprocess
import tempfile

import pytest

from isa_util import CSRC, FLAGS, HIPCC, all_isa, have_hipcc
from test_kernel_resources import scratch_by_kernel

# gemm_f32_kernel<NB, NW, MODE, METRIC, AK>: MODE is the third template argument
_COMPONENTS_MODE = re.compile(r"gemm_f32_kernelILi(\d+)ELi(\d+)ELi4ELi(\d+)ELb([01])E")


@pytest.mark.skipif(not have_hipcc(), reason="hipcc not available")
def test_components_mode_instantiations_use_no_scratch():
    sc = scratch_by_kernel(all_isa()[("pmm_kernels.hip", ())])
    found = {}
    for name, use in sc.items():
        m = _COMPONENTS_MODE.search(name)
        if m:
            found[tuple(int(x) for x in m.groups())] = use
    want = {(4, 4, metric, ak) for metric in range(3) for ak in (0, 1)} | {(8, 8, metric, 0) for metric in range(3)}
    assert want == set(found), f"components instantiations: {sorted(found)}, wanted {sorted(want)}"
    bad = {k: v for k, v in found.items() if v != (0, 0)}
    assert not bad, f"scratch (bytes, instructions) in components-mode kernels: {bad}"


@pytest.mark.skipif(not have_hipcc(), reason="hipcc not available")
def test_forest_kernels_use_no_scratch():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "range.s")
        subprocess.run([HIPCC, *FLAGS, "-I", CSRC, "-o", out, os.path.join(CSRC, "pmm_range.hip")], check=True,
                       capture_output=True, timeout=600)
        asm = open(out).read()
    sc = scratch_by_kernel(asm)
    for kernel in ("components_init_kernel", "components_label_kernel"):
        hits = {k: v for k, v in sc.items() if kernel in k}
        assert hits, f"{kernel} not in pmm_range.hip's assembly: {sorted(sc)}"
        assert set(hits.values()) == {(0, 0)}, f"scratch (bytes, instructions): {hits}"
