"""The hypotheses' kernels (csrc/icp_hyp.hip) compile for gfx950, are the file's kernel set by name, spill nothing and keep their static
LDS within 64 KB (the collecting kernel holds a heading's offsets, 4 bytes per beam up to TBNAV_ICP_MAX_BEAMS); and the global search's
file still holds its own seven kernels and none of these: the kernel descriptors' metadata of one device-only compile of each file
(hipcc cross-compiles without a GPU)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("icp_hyp_collect", "icp_hyp_knock", "icp_hyp_select")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def _descriptors(tmp, name):
    out = tmp / (name + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-fast-math", f"-I{ROOT}/include", f"-I{CSRC}",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(CSRC, name + ".hip"), "-o", str(out)],
                   check=True, stderr=subprocess.DEVNULL)
    meta = re.findall(r"\.group_segment_fixed_size:\s*(\d+)\s*\n(?:.*\n)*?\s*\.name:\s*(\S+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s*(\d+)",
                      out.read_text())
    return {n: (int(g), int(p)) for g, n, p in meta}


@pytest.fixture(scope="module")
def descriptors(tmp_path_factory):
    return _descriptors(tmp_path_factory.mktemp("icp_hyp_isa"), "icp_hyp")


def test_the_kernel_set(descriptors):
    names = sorted(descriptors)
    assert len(names) == len(KERNELS), names
    for want in KERNELS:
        assert sum(want in got for got in names) == 1, (want, names)


def test_no_kernel_has_a_private_segment_and_static_lds_is_within_64_kb(descriptors):
    for name, (static, private) in descriptors.items():
        assert private == 0 and static <= 64 * 1024, (name, static, private)
    assert next(v for n, v in descriptors.items() if "icp_hyp_collect" in n)[0] >= 4 * 4096     # a heading's offsets at TBNAV_ICP_MAX_BEAMS


def test_the_global_search_file_holds_none_of_them(tmp_path):
    names = sorted(_descriptors(tmp_path, "icp_global"))
    assert len(names) == 7 and not any(k in n for k in KERNELS for n in names), names
