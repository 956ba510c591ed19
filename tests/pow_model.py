"""The proof-of-work step of include/toyni_hip.h 3n in hashlib alone: the model every expected nonce of every test comes from (never
from the library).

    accept(S, nonce, bits)  <=>  the first `bits` bits of SHA256(S || LE64(nonce)) are zero, most significant bit of byte 0 first
    grind(S, bits, start, tries) = the smallest accepted nonce of [start, start + tries), or None

A test caps its model search (`cap` below) and treats a None inside the cap as a test ERROR, never as a skip: must_grind raises."""
import hashlib

CAPACITY = 1008
E_RANGE = 10006
MAX_BITS = 32
P = 2013265921
START_STATE = b"toyni-stark-v1"
TABLE_LENGTHS = [0, 32, 47, 48, 55, 56, 63, 64, 96, 119, 120, 1000]


def pattern(n, seed):
    return bytes((seed * 131 + 7 * i + (i >> 8)) & 0xFF for i in range(n))


def table_states():
    """the states of the checked table: (name, bytes)"""
    return [("n=0", pattern(0, 0)), ("toyni-stark-v1", START_STATE)] + [(f"n={n}", pattern(n, n)) for n in TABLE_LENGTHS[1:]]


def le64(nonce):
    return int(nonce).to_bytes(8, "little")


def accept(state, nonce, bits):
    assert 0 <= bits <= MAX_BITS and 0 <= nonce < 1 << 64
    h = hashlib.sha256(bytes(state) + le64(nonce)).digest()
    return bits == 0 or int.from_bytes(h[:4], "big") >> (32 - bits) == 0


def grind(state, bits, start, tries):
    base = hashlib.sha256(bytes(state))
    for nonce in range(start, min(start + tries, 1 << 64)):
        h = base.copy()
        h.update(le64(nonce))
        if bits == 0 or int.from_bytes(h.digest()[:4], "big") >> (32 - bits) == 0:
            return nonce
    return None


def cap(bits):
    """candidates the model may search for a case that is expected to have an answer"""
    return 1 << 22 if bits > 16 else 1 << 20


def must_grind(state, bits, start=0):
    nonce = grind(state, bits, start, cap(bits))
    if nonce is None:
        raise RuntimeError(f"the model finds no {bits}-bit nonce within {cap(bits)} candidates from {start}: the case is wrong")
    return nonce


class Transcript:
    """src/transcript.rs behind the capacity and the sticky status of include/toyni_hip.h 3l, with the grinding step of 3n"""

    def __init__(self, state=b"", status=0):
        self.state, self.status = bytes(state), status

    def absorb(self, data):
        if self.status:
            return
        if len(self.state) + len(data) > CAPACITY:
            self.status = E_RANGE
            return
        self.state += bytes(data)

    def squeeze(self, count):
        if self.status:
            return [0] * count
        out = []
        for _ in range(count):
            self.state = hashlib.sha256(self.state).digest()
            out.append(int.from_bytes(self.state[:8], "little") % P)
        return out

    def squeeze_indices(self, count, mx):
        if self.status:
            return [0] * count
        out, state = [], self.state
        for _ in range(64 * count + 64):
            state = hashlib.sha256(state).digest()
            idx = int.from_bytes(state[:8], "little") % mx
            if idx not in out:
                out.append(idx)
                if len(out) == count:
                    self.state = state
                    return out
        self.status = E_RANGE
        return [0] * count

    def grind(self, bits, start=0, tries=None):
        """the nonce the device leaves in *d_nonce: 0 where the call refuses"""
        if self.status:
            return 0
        if len(self.state) + 8 > CAPACITY:
            self.status = E_RANGE
            return 0
        nonce = grind(self.state, bits, start, cap(bits) if tries is None else tries)
        if nonce is None:
            self.status = E_RANGE
            return 0
        self.state += le64(nonce)
        return nonce
