"""The global search's kernels (csrc/icp_global.hip) compile for gfx950, are the file's kernel set by name, spill nothing and keep
their static LDS within 64 KB (the bound and refinement kernels hold a heading's offsets, 4 bytes per beam up to
TBNAV_ICP_MAX_BEAMS): the kernel descriptors' metadata of one device-only compile of the file (hipcc cross-compiles without a
GPU)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("icp_global_bound", "icp_global_field", "icp_global_hist", "icp_global_list", "icp_global_offsets", "icp_global_pool",
           "icp_global_refine")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    """{kernel name: (static LDS bytes, private segment bytes)}"""
    out = tmp_path_factory.mktemp("icp_global_isa") / "icp_global.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-fast-math", f"-I{ROOT}/include", f"-I{CSRC}",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(CSRC, "icp_global.hip"), "-o", str(out)],
                   check=True, stderr=subprocess.DEVNULL)
    meta = re.findall(r"\.group_segment_fixed_size:\s*(\d+)\s*\n(?:.*\n)*?\s*\.name:\s*(\S+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s*(\d+)",
                      out.read_text())
    return {n: (int(g), int(p)) for g, n, p in meta}


def test_the_kernel_set(descriptors):
    names = sorted(descriptors)
    assert len(names) == len(KERNELS), names
    for want in KERNELS:
        assert sum(want in got for got in names) == 1, (want, names)


def test_no_kernel_has_a_private_segment(descriptors):
    for name, (_, private) in descriptors.items():
        assert private == 0, (name, private)


def test_static_lds_is_within_64_kb(descriptors):
    for name, (static, _) in descriptors.items():
        assert static <= 64 * 1024, (name, static)
    offsets = 4 * 4096                                       # a heading's offsets at TBNAV_ICP_MAX_BEAMS
    for k in ("icp_global_bound", "icp_global_refine"):
        assert next(v for n, v in descriptors.items() if k in n)[0] >= offsets, k
    assert next(v for n, v in descriptors.items() if "icp_global_field" in n)[0] >= 48 * 8 + 2 * 8 * 8 + 1
