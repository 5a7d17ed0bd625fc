"""What the CPU tests of the take session and of takev share: the fake device pointers, the header walk of the host decoder
restated, what the replay's stand-in decoder answers for an archive, and the golden archives by folder. A plain module next to
the tests, imported the way cshim is; the names are the ones the two test files use."""
import os

import numpy as np

from conftest import GOLDEN

FAKE_SRC, FAKE_DST, FAKE_WORK, FAKE_RES = 0x10000, 0x30000, 0x40000, 0x50000  # device pointers that are never dereferenced
BAD_BLOCK_SIZES = (0, 1000, 2048, 4095, 5000, 3 << 12, 1 << 22)
BAD_PLAN = -1000  # the replay's answer when a chunk's plan breaks a promise (tests/take/take_replay.h)


def _hash8(hdr7: bytes) -> int:
    M = (1 << 64) - 1
    h = int.from_bytes(hdr7 + b"\0", "little") ^ 0x9E3779B97F4A7C15
    h ^= (h << 13) & M
    h ^= h >> 7
    h ^= (h << 17) & M
    return ((h >> 32) ^ h) & 0xFF


def _host_walk(comp: bytes, file_ck: int, limit: int):
    """frame_source of zxc_host.c, restated: -> [(comp_off, comp_size)] of the blocks a header walk finds, at most `limit`"""
    ip, jobs = 16, []
    while len(jobs) < limit and ip < len(comp):
        rem = len(comp) - ip
        if rem < 8 or comp[ip + 7] != _hash8(comp[ip: ip + 7]) or comp[ip] == 255:
            break
        phys = 8 + int.from_bytes(comp[ip + 3: ip + 7], "little") + 4 * file_ck
        jobs.append((ip, min(phys, rem)))
        if phys >= rem:
            break
        ip += phys
    return jobs


class Blocks:
    """what the stand-in decoder answers for an archive: per block of the header walk the oracle decoder's bytes and status"""

    def __init__(self, shim, oracle, comp, bs, cap, verify):
        flags = int(shim.t_head(comp, len(comp), max(cap, 1), bs, int(verify)))
        self.file_ck, self.verify = flags & 1, (flags >> 1) & 1
        data, at, st = [], [], []
        for off, n in _host_walk(comp, self.file_ck, -(-cap // bs) + 1):
            rc, out = oracle.decode_block(comp[off: off + n], bs, checksum=bool(self.verify))
            at.append(sum(len(d) for d in data))
            st.append(rc)
            data.append(out[:max(rc, 0)] if rc > 0 else b"")
        self.n = len(st)
        self.bytes = np.frombuffer(b"".join(data) + b"\0", dtype=np.uint8)
        self.at = np.array(at + [0], dtype=np.uint64)
        self.st = np.array(st + [0], dtype=np.int32)


def _goldens(sub):
    p = os.path.join(GOLDEN, sub)
    return [f"{sub}/{f}" for f in sorted(os.listdir(p)) if f.endswith(".zxc")]
