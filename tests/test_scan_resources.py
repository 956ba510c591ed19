"""The accumulator-column kernels (include/toyni_hip.h 3g) keep a thread's group of elements in registers that are indexed by
constants only: none of them may use scratch (CPU only: read from the resource record of the build that produced the shipped library,
as tests/test_air_resources.py does)."""
import os
import re

import __graft_entry__ as entry


def test_no_scan_or_batch_inverse_kernel_uses_scratch():
    entry.build_hip()
    if not os.path.exists(entry.RESOURCES) or os.path.getmtime(entry.RESOURCES) < os.path.getmtime(entry.LIB) - 5:
        entry.build_hip(force=True)
    remarks = open(entry.RESOURCES).read()
    blocks = re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]
    seen = set()
    for b in blocks:
        name = b.split(" ")[0]
        if "scan" not in name and "batch_inverse" not in name:
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b)
        assert m, name
        assert int(m.group(1)) == 0, f"{name} uses {m.group(1)} bytes of scratch per lane"
        seen.add(name)
    # aggregate, prefix and apply for each op, and the inversion
    assert len(seen) == 7 and sum("column_scan" in s for s in seen) == 6 and sum("batch_inverse" in s for s in seen) == 1, sorted(seen)
