"""The kernel-coverage guard of tests/test_zz_kernel_coverage.py for the second translation unit of libtoyni_hip.so: every __global__
symbol of toyni_amd/csrc/batch/toyni_hip_fib_batch.hip (include/toyni_hip.h 3s) must have been launched by the GPU test session that is just
finishing.  That file reads the kernels of the shipped library from the remarks of toyni_hip.hip's build; the remarks of the second
unit are kept in a file of their own (__graft_entry__.RESOURCES_FIB_BATCH), so its kernels are held here, by the same rule: the
library's in-memory list of launched kernels, and what the session's child processes dumped into $TOYNI_LAUNCH_LOG.  Nothing is
allowed to stay unlaunched.  (This file sorts behind that one on purpose.)"""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shipped_kernels():
    import __graft_entry__ as entry
    entry.build_hip()
    return sorted(set(re.findall(r"Function Name: (\S+)", open(entry.RESOURCES_FIB_BATCH).read())))


def test_kernel_list_of_the_second_unit_is_present_and_is_in_the_library():
    import subprocess
    import __graft_entry__ as entry
    names = shipped_kernels()
    assert len(names) == 13 and any("copy_rows_kernel" in n for n in names) and any("fib_quotient_batch_kernel" in n for n in names)
    # the unit is linked into the shipped library: the kernels' host-side handles are defined there
    syms = subprocess.run(["nm", "-D", "--defined-only", entry.LIB], capture_output=True, text=True).stdout
    assert all(re.search(r"\b%s\b" % re.escape(n), syms) for n in names), [n for n in names if n not in syms]


@pytest.mark.gpu
def test_every_kernel_of_the_second_unit_was_launched_by_this_session(request):
    # judged only when the whole GPU suite ran in this session (a -k / single-file run proves nothing about coverage)
    ran = {os.path.basename(str(item.fspath)) for item in request.session.items}
    gpu_files = set()
    for f in glob.glob(os.path.join(ROOT, "tests", "test_*.py")):
        src = open(f).read()
        if re.search(r"^pytestmark = pytest\.mark\.gpu|^@pytest\.mark\.gpu|^@gpu$", src, flags=re.M):
            gpu_files.add(os.path.basename(f))
    missing_files = sorted(gpu_files - ran)
    if missing_files:
        pytest.skip(f"partial session (no tests from {missing_files}): coverage is judged on full `-m gpu` runs")
    log = os.environ.get("TOYNI_LAUNCH_LOG")
    assert log and os.path.exists(log), "tests/conftest.py sets TOYNI_LAUNCH_LOG for the session"
    launched = {l.strip() for l in open(log) if l.strip()}
    from toyni_amd import _lib
    launched |= set(_lib.launched_kernels())
    never = [k for k in shipped_kernels() if k not in launched]
    assert not never, "kernels of toyni_hip_fib_batch.hip that no GPU test launched:\n  " + "\n  ".join(never)
