"""The line-metric ICP kernel (csrc/icp.hip, icp_align_line) compiles for gfx950 and spills nothing: no scratch instruction in
any of its instantiations, by the method of test_icp_isa.py (hipcc cross-compiles without a GPU); and adding it left the
point kernel's eight instantiations in place."""
import os
import re
import subprocess

import pytest

from test_icp_isa import CSRC, HIPCC, ROOT, _kernels


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_line_kernel_has_no_scratch_instruction(tmp_path):
    out = tmp_path / "icp.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-fast-math", f"-I{ROOT}/include", f"-I{CSRC}",
                    "-ffp-contract=off", "-S", "--cuda-device-only", os.path.join(CSRC, "icp.hip"), "-o", str(out)],
                   check=True, stderr=subprocess.DEVNULL)
    text = out.read_text()
    lines = text.split("\n")
    ks = _kernels(lines, r"icp_align_lineILi")
    assert len(ks) == 6, sorted(ks)   # P = 1, 2, 3, 4, 6, 8 source beams per thread (n_beams <= 2048)
    ks.update(_kernels(lines, r"icp_normals"))
    assert len(ks) == 7, sorted(ks)
    for name, body in ks.items():
        assert any("ds_read" in l or "ds_load" in l for l in body), name   # a kernel body, not a stub
        hits = [l.strip() for l in body if re.match(r"\s*(scratch_|buffer_(load|store)\S*\s.*\boffen\b)", l)]
        assert not hits, (name, hits[:4])
    # what the kernel descriptors say of the same thing, and of static LDS: 16 KB for the tree, so that the 32 KB of cloud
    # and normals at 2048 beams stay inside the 64 KB a workgroup may have
    meta = re.findall(r"\.group_segment_fixed_size:\s*(\d+)\s*\n(?:.*\n)*?\s*\.name:\s*(\S+)\s*\n(?:.*\n)*?\s*\.private_segment_fixed_size:\s*(\d+)", text)
    line = [(int(g), n, int(p)) for g, n, p in meta if "icp_align_lineILi" in n]
    assert len(line) == 6, meta
    for g, n, p in line:
        assert p == 0, (n, p)
        assert g + 2 * 8 * 2048 <= 64 * 1024, (n, g)
    assert len(_kernels(lines, r"icp_alignILi")) == 8
