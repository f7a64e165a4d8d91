"""The per-file compile flags of csrc/Makefile (CONTRACT_<file>, PRELOAD_<file>), so that the ISA tools look at the code object the
library ships:  per_file_flags("mppi_rollout") -> ["-ffp-contract=fast-honor-pragmas", "-mllvm", "-amdgpu-kernarg-preload-count=16"]"""
import os
import re
import shlex

MAKEFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ros-turtlebot-navigation_amd", "csrc", "Makefile")


def per_file_flags(src, kinds=("CONTRACT", "PRELOAD")):
    stem = os.path.splitext(os.path.basename(src))[0]
    text = open(MAKEFILE).read()
    out = []
    for kind in kinds:
        m = re.search(rf"^{kind}_{re.escape(stem)}\s*:=\s*(.*)$", text, re.M)
        if m:
            out += shlex.split(m.group(1))
    return out
