"""CPU checks of tests/guarded.py: the edge-value generators are deterministic and complete, and a guard-banded buffer on host
memory reports an overrun of one word at either end (with its offset) and passes an untouched buffer."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import GUARD_MIN, P, SENTINEL, U64_NONCANONICAL, Guarded, HostMem, edge_classes, edge_residues, edge_u64, reduce_u64  # noqa: E402


def test_edge_classes_are_what_they_claim():
    c = edge_classes()
    r = (1 << 32) % P
    assert c["mont=1"] * r % P == 1 and c["mont=p-1"] * r % P == P - 1
    rinv = pow(r, -1, P)
    assert c["invmont=1"] * rinv % P == 1 and c["invmont=p-1"] * rinv % P == P - 1
    assert c["(p-1)/2"] * 2 == P - 1 and c["(p+1)/2"] * 2 == P + 1
    assert all(0 <= v < P for v in c.values())


@pytest.mark.parametrize("n", [16, 64, 1 << 12, 1 << 16])
def test_edge_residues_deterministic_canonical_complete(n):
    a, b = edge_residues(n, 7), edge_residues(n, 7)
    assert a.dtype == np.uint32 and a.size == n
    assert (a == b).all()
    assert n <= 32 or not (a == edge_residues(n, 8)).all()
    assert int(a.max()) < P
    present = set(a.tolist())
    missing = [k for k, v in edge_classes().items() if v not in present]
    assert not missing, missing
    # runs of p-1 and alternating 0 / p-1 blocks in the second half: butterfly partners at distance n/2 are edges too
    h = a[n // 2:]
    assert n <= 32 or ((h == P - 1).sum() >= 2 and (h == 0).sum() >= 1)
    assert a[0] in (0, 1) and a[n // 2] == max(edge_classes().values())


def test_edge_residues_fraction():
    a = edge_residues(1 << 16, 3, frac=0.5)
    edges = np.isin(a, np.array(list(edge_classes().values()), dtype=np.uint32))
    assert 0.4 < edges.mean() < 0.7
    assert np.isin(edge_residues(1 << 16, 3, frac=0.0)[100:1 << 15], list(edge_classes().values())).mean() < 0.01


def test_edge_u64_has_every_noncanonical_value():
    for n in (8, 1000, 1 << 14):
        a = edge_u64(n, 5)
        assert a.dtype == np.uint64 and a.size == n and (a == edge_u64(n, 5)).all()
        for v in U64_NONCANONICAL:
            assert (a == np.uint64(v)).any(), (n, v)
        r = reduce_u64(a)
        assert int(r.max()) < P
        assert all(int(r[i]) == int(a[i]) % P for i in range(0, n, max(1, n // 97)))


@pytest.mark.parametrize("offset", [0, 4, 8, 12])
@pytest.mark.parametrize("word", [1, 4, 8])
def test_guard_reports_one_word_overrun_at_either_end(offset, word):
    mem = HostMem()
    w = max(word, 4)
    payload = 40 * w
    g = Guarded(mem, payload, offset=offset, word=word)
    try:
        assert g.ptr % 16 == offset and g.guard >= GUARD_MIN
        assert (g.download(np.uint8) == SENTINEL).all()          # the payload starts as sentinel too
        g.upload(np.arange(payload, dtype=np.uint8))
        g.check()                                              # payload writes are not damage
        view = mem.view(g.base, g.total)
        # one word past the end
        view[g.front + payload: g.front + payload + w] = 0
        with pytest.raises(AssertionError, match=r"back guard damaged 0 bytes past the payload end .* %d bytes long" % w):
            g.check()
        view[g.front + payload: g.front + payload + w] = SENTINEL
        g.check()
        # one word before the start
        view[g.front - w: g.front] = 1
        with pytest.raises(AssertionError, match=r"front guard damaged %d bytes before the payload start .* %d bytes long" % (w, w)):
            g.check()
        view[g.front - w: g.front] = SENTINEL
        # a stray write deep in the back guard (a whole tile past the end)
        view[g.front + payload + 4096] = 0
        with pytest.raises(AssertionError, match="4096 bytes past the payload end"):
            g.check()
        view[g.front + payload + 4096] = SENTINEL
    finally:
        g.free()


def test_random_guard_pattern_is_canonical_and_checked():
    mem = HostMem()
    g = Guarded(mem, 256, offset=4, seed=3)
    g.refill("random")
    view = mem.view(g.base, g.total)
    back = view[g.front + 256: g.front + 256 + g.guard].view(np.uint32)
    assert int(back.max()) < P and (back != back[0]).any()
    g.check()
    view[g.front + 256] ^= 1
    with pytest.raises(AssertionError, match="back guard"):
        g.check()
    view[g.front + 256] ^= 1
    g.refill("sentinel")
    assert (view[:g.front] == SENTINEL).all()
    g.free()
    assert g.base is None


def test_free_checks_and_still_releases():
    mem = HostMem()
    g = Guarded(mem, 64)
    mem.view(g.base, g.total)[g.front + 64] = 0
    with pytest.raises(AssertionError):
        g.free()
    assert g.base is None and not mem._blocks
