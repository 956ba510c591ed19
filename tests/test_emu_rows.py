"""Steps the row-leaf body of the Merkle row commitment (merkle_row_leaf_at, toyni_amd/csrc/merkle_kernels.hpp) on the CPU under
AddressSanitizer + UBSan and compares every digest with hashlib: widths 1..40, salted and unsalted, column-major (padded column
stride) and row-major (word loads, and 16-byte loads where the width is a multiple of 4), values from {0, 1, p - 1, random}.
CPU only; the shipped library contains none of tests/emu."""
import hashlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "toyni_amd", "csrc")
MAX_WIDTH = 40


def build_emu_rows() -> str:
    src = os.path.join(ROOT, "tests", "emu", "emu_rows.cpp")
    out = os.path.join(ROOT, "tests", "emu", "build", "emu_rows_asan")
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-Wno-unknown-pragmas", "-I", CSRC, "-o", out, src])
    return out


def test_row_leaf_body_matches_hashlib_on_cpu():
    res = subprocess.run([build_emu_rows(), str(MAX_WIDTH)], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = res.stdout.split("\n")
    assert lines[-2] == "DONE"
    seen = set()            # (width, salted, layout, vec)
    blocks_of = {}          # (width, salted) -> block count the program reports
    values = set()
    for line in lines[:-2]:
        width, salted, layout, vec, blocks, leaf_hex, digest_hex = line.split()
        width, salted, layout, vec, blocks = int(width), int(salted), int(layout), int(vec), int(blocks)
        leaf = bytes.fromhex(leaf_hex)
        assert len(leaf) == 16 * salted + 8 * width
        msg = 1 + len(leaf)
        assert blocks == (msg + 9 + 63) // 64
        assert hashlib.sha256(b"\x00" + leaf).hexdigest() == digest_hex, (width, salted, layout, vec)
        seen.add((width, salted, layout, vec))
        blocks_of[(width, salted)] = blocks
        body = leaf[16 * salted:]
        values.update(int.from_bytes(body[8 * c:8 * c + 8], "little") for c in range(width))
    for width in range(1, MAX_WIDTH + 1):
        for salted in (0, 1):
            assert (width, salted, 0, 0) in seen and (width, salted, 1, 0) in seen
            assert ((width, salted, 1, 1) in seen) == (width % 4 == 0)
    assert {0, 1, 2013265921 - 1} <= values and len(values) > 100
    # L mod 64 = 57: the padding needs a block of its own.  Unsalted width = 7 (mod 8), salted width = 5 (mod 8); the range must
    # hold such widths at both block counts they can have, so that nobody shrinks it past them.
    for salted, residue in ((0, 7), (1, 5)):
        ws = [w for w in range(1, MAX_WIDTH + 1) if w % 8 == residue]
        assert len(ws) == 5
        for w in ws:
            assert (1 + 16 * salted + 8 * w) % 64 == 57
            # one block more than the data alone would take
            assert blocks_of[(w, salted)] == (1 + 16 * salted + 8 * w + 63) // 64 + 1
        assert len({blocks_of[(w, salted)] for w in ws}) >= 2
    assert {blocks_of[(w, s)] for w in range(1, MAX_WIDTH + 1) for s in (0, 1)} >= {1, 2, 3, 4, 5, 6}
