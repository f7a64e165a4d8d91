"""The ICP kernel (csrc/icp.hip, icp_align<Metric, P, C>) compiles for gfx950 and spills nothing: no scratch instruction in any
instantiation of either metric nor in icp_normals, and static LDS that leaves room for the largest cloud (the same method as
test_isa_no_scratch.py; hipcc cross-compiles without a GPU).  One compile of the file serves every test here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ros-turtlebot-navigation_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
POINT = r"icp_alignI\w*PointMetricELi"   # the mangled names of icp_align<PointMetric, P, C> ...
LINE = r"icp_alignI\w*LineMetricELi"     # ... and icp_align<LineMetric, P, C>

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def _kernels(lines, pattern):
    out, cur = {}, None
    for l in lines:
        m = re.match(r"^(_Z\S+):", l)
        if m:
            cur = m.group(1) if re.search(pattern, m.group(1)) else None
            if cur:
                out[cur] = []
            continue
        if cur is not None:
            if ".Lfunc_end" in l:
                cur = None
            else:
                out[cur].append(l)
    return out


@pytest.fixture(scope="module")
def icp_asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("icp_isa") / "icp.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-fast-math", f"-I{ROOT}/include", f"-I{CSRC}",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(CSRC, "icp.hip"), "-o", str(out)],
                   check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


def _no_scratch(ks):
    for name, body in ks.items():
        assert any("ds_read" in l or "ds_load" in l for l in body), name   # a kernel body, not a stub
        hits = [l.strip() for l in body if re.match(r"\s*(scratch_|buffer_(load|store)\S*\s.*\boffen\b)", l)]
        assert not hits, (name, hits[:4])


def _descriptors(text, pattern):
    """(static LDS bytes, name, private segment bytes) of the kernels whose name matches"""
    meta = re.findall(r"\.group_segment_fixed_size:\s*(\d+)\s*\n(?:.*\n)*?\s*\.name:\s*(\S+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s*(\d+)", text)
    return [(int(g), n, int(p)) for g, n, p in meta if re.search(pattern, n)]


def test_icp_kernel_has_no_scratch_instruction(icp_asm):
    ks = _kernels(icp_asm.split("\n"), POINT)
    assert len(ks) == 8, sorted(ks)   # P = 1, 2, 3, 4, 6, 8, 12, 16 source beams per thread
    _no_scratch(ks)
    # what the kernel descriptors say of the same thing, and of static LDS: the tree of nine sums, so that the 32 KB of cloud
    # at 4096 beams stay inside the 64 KB a workgroup may have
    point = _descriptors(icp_asm, POINT)
    assert len(point) == 8, point
    for g, n, p in point:
        assert p == 0, (n, p)
        assert g + 8 * 4096 <= 64 * 1024, (n, g)


def test_line_kernel_has_no_scratch_instruction(icp_asm):
    lines = icp_asm.split("\n")
    ks = _kernels(lines, LINE)
    assert len(ks) == 6, sorted(ks)   # P = 1, 2, 3, 4, 6, 8 source beams per thread (n_beams <= 2048)
    ks.update(_kernels(lines, r"icp_normals"))
    assert len(ks) == 7, sorted(ks)
    _no_scratch(ks)
    # what the kernel descriptors say of the same thing, and of static LDS: 16 KB for the tree, so that the 32 KB of cloud
    # and normals at 2048 beams stay inside the 64 KB a workgroup may have
    line = _descriptors(icp_asm, LINE)
    assert len(line) == 6, line
    for g, n, p in line:
        assert p == 0, (n, p)
        assert g + 2 * 8 * 2048 <= 64 * 1024, (n, g)
    assert len(_kernels(lines, POINT)) == 8
