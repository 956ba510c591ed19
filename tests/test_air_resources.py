"""The kernels that interpret constraint programs keep their register file in LDS: none of them may use scratch (CPU only: read
from the resource record of the build that produced the shipped library, as tests/test_build_resources.py does)."""
import os
import re

import __graft_entry__ as entry


def test_no_air_kernel_uses_scratch():
    entry.build_hip()
    if not os.path.exists(entry.RESOURCES) or os.path.getmtime(entry.RESOURCES) < os.path.getmtime(entry.LIB) - 5:
        entry.build_hip(force=True)
    remarks = open(entry.RESOURCES).read()
    blocks = re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]
    seen = 0
    for b in blocks:
        name = b.split(" ")[0]
        if "air_" not in name:
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
        assert m, name
        assert int(m.group(1)) == 0, f"{name} uses {m.group(1)} bytes of scratch per lane"
        seen += 1
    assert seen >= 1
