"""The kernel that measures the shape of the correlative search's score volume (csrc/icp_search_shape.hip) compiles for gfx950,
spills nothing and fits in LDS: the kernel descriptors of one device-only compile of the file (hipcc cross-compiles without a
GPU).  There is one kernel, one instantiation (the translations per thread are a runtime count); its
private_segment_fixed_size is 0, and static plus dynamic LDS at the largest table (TBNAV_ICP_SEARCH_MAX_SIDE) and 4096 beams
stays inside the 64 KB a workgroup may have.  Only descriptors are read, never the instruction stream."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
MAX_SIDE, MAX_BEAMS = 208, 4096

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    """{kernel name: (static LDS bytes, private segment bytes)}"""
    out = tmp_path_factory.mktemp("icp_search_shape_isa") / "icp_search_shape.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-fast-math", f"-I{ROOT}/include", f"-I{CSRC}",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(CSRC, "icp_search_shape.hip"), "-o", str(out)],
                   check=True, stderr=subprocess.DEVNULL)
    meta = re.findall(r"\.group_segment_fixed_size:\s*(\d+)\s*\n(?:.*\n)*?\s*\.name:\s*(\S+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s*(\d+)",
                      out.read_text())
    return {n: (int(g), int(p)) for g, n, p in meta}


def test_the_kernel_set(descriptors):
    names = sorted(descriptors)
    assert len(names) == 1 and "icp_search_shape" in names[0], names


def test_no_kernel_spills(descriptors):
    for name, (_, private) in descriptors.items():
        assert private == 0, (name, private)


def test_lds_fits_at_the_largest_table_and_beam_count(descriptors):
    table = (MAX_SIDE * MAX_SIDE + 15) & ~15           # the padded byte table, whole 16-byte loads
    cells = 2 * MAX_BEAMS                              # uint16 base cells
    for name, (static, _) in descriptors.items():
        assert static + table + cells <= 64 * 1024, (name, static, table + cells)
