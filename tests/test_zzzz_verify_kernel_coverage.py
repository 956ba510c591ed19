"""The kernel-coverage guard of tests/test_zzz_fib_batch_kernel_coverage.py for the third translation unit of libtoyni_hip.so: every
__global__ symbol of toyni_amd/csrc/verify/toyni_hip_verify.hip (include/toyni_hip.h 3t) must have been launched by the GPU test session
that is just finishing -- the library's in-memory list of launched kernels, and what the session's child processes dumped into
$TOYNI_LAUNCH_LOG.  Nothing is allowed to stay unlaunched.  (This file sorts behind the other two guards on purpose.)"""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shipped_kernels():
    import __graft_entry__ as entry
    entry.build_hip()
    return sorted(set(re.findall(r"Function Name: (\S+)", open(entry.RESOURCES_VERIFY).read())))


def test_kernel_list_of_the_third_unit_is_present_and_is_in_the_library():
    import subprocess
    import __graft_entry__ as entry
    names = shipped_kernels()
    assert len(names) == 5 and any("merkle_verify_records_batch_kernel" in n for n in names) and any("fib_verify_replay_kernel" in n for n in names)
    syms = subprocess.run(["nm", "-D", "--defined-only", entry.LIB], capture_output=True, text=True).stdout
    assert all(re.search(r"\b%s\b" % re.escape(n), syms) for n in names), [n for n in names if n not in syms]
    files = sorted(os.path.basename(f) for f in glob.glob(os.path.join(ROOT, "tests", "test_zz*_coverage.py")))
    assert files[-1] == os.path.basename(__file__), files


@pytest.mark.gpu
def test_every_kernel_of_the_third_unit_was_launched_by_this_session(request):
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
    assert not never, "kernels of toyni_hip_verify.hip that no GPU test launched:\n  " + "\n  ".join(never)
