"""What the batch wrappers of conv, t2j and generic share: the arena a host
entry reads, the DG_E_NOMEM retry, the outputs cut apart."""
import numpy as np

from . import _lib


def arena(msgs):
    """(arena, in_off): the messages back to back with 16 spare bytes, and
    uint64[n + 1] offsets from 0."""
    n = len(msgs)
    in_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(m) for m in msgs), dtype=np.uint64, count=n), out=in_off[1:])
    return np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8), in_off


def until_fits(call, cap: int, need):
    """call(cap) -> (rc, out) with room for `cap`; on DG_E_NOMEM (-3) with a
    larger *need, once more at that size. Returns the out that fitted."""
    while True:
        rc, out = call(cap)
        if rc == -3 and need.value > cap:
            cap = int(need.value)
            continue
        _lib.check(rc)
        return out


def split(out, out_off):
    """[bytes of out[out_off[i]:out_off[i + 1]] for every i]"""
    off = out_off.tolist()
    whole = out[:off[-1]].tobytes()
    return [whole[a:b] for a, b in zip(off, off[1:])]
