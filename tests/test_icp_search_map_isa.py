"""The map search's table kernel (csrc/icp_search_map.hip) compiles for gfx950, is the file's only kernel, spills nothing and fits in
LDS whatever the stamp's half width (its LDS is static: 48 staged rows, the value table for k = 8 and the transposed tile): the kernel
descriptors' metadata of one device-only compile of the file (hipcc cross-compiles without a GPU)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    """{kernel name: (static LDS bytes, private segment bytes)}"""
    out = tmp_path_factory.mktemp("icp_search_map_isa") / "icp_search_map.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-fast-math", f"-I{ROOT}/include", f"-I{CSRC}",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(CSRC, "icp_search_map.hip"), "-o", str(out)],
                   check=True, stderr=subprocess.DEVNULL)
    meta = re.findall(r"\.group_segment_fixed_size:\s*(\d+)\s*\n(?:.*\n)*?\s*\.name:\s*(\S+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s*(\d+)",
                      out.read_text())
    return {n: (int(g), int(p)) for g, n, p in meta}


def test_the_kernel_set(descriptors):
    names = sorted(descriptors)
    assert len(names) == 1 and "icp_search_table_from_occ" in names[0], names


def test_the_kernel_does_not_spill(descriptors):
    for name, (_, private) in descriptors.items():
        assert private == 0, (name, private)


def test_lds_fits_at_the_widest_stamp(descriptors):
    rows, values, tile = 48 * 8, 2 * 8 * 8 + 1, 32 * 32      # what k = 8 needs at the least
    for name, (static, _) in descriptors.items():
        assert rows + values + tile <= static <= 64 * 1024, (name, static)
