"""CPU: the kernels' field-name lookups themselves (key_eq, the flat kernel's
fl_lookup, the wave kernel's wv_lookup), built for the host by keys_host.cpp,
against the Python name map: every (struct, key) pair of descgen's names,
aliases and ids families, near misses included -- equal hashes, chains that
wrap the table, keys one byte off at every position, one shorter, one longer,
followed by NUL bytes -- with the key at every alignment and the blob in a
heap block of exactly total_len bytes."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import descgen as G
from dynamicgo_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))


def build_keys(out, extra=()):
    subprocess.run([B.HIPCC, "-x", "hip", "--offload-arch=" + B.ARCH, "-O1", "-std=c++17", "-fPIC",
                    "-Wno-ignored-attributes", "-Wno-unused-value", *extra, "-o", out,
                    os.path.join(HERE, "keys_host.cpp")], check=True)
    return out


def corpus():
    """(bytes, queries): the corpus keys_host.cpp reads and, per query,
    (case name, raw key, wanted global field index)."""
    cases = G.names_family()[0] + G.aliases_family() + G.ids_family()
    blobs, rows, queries = [], [], []
    for bi, c in enumerate(cases):
        fl = c.flat
        blobs.append(struct.pack("<I", len(fl.blob)) + fl.blob)
        sd = c.td.struct
        index = {id(f): k for k, f in enumerate(fl.fields)}
        keys = set()
        for it, m in zip(c.intents, c.msgs):
            keys.add(it.ids[0] if it.kind == G.UNKNOWN else None)
        keys.discard(None)
        keys |= {k.encode() for k in sd.names}
        for raw in sorted(keys):
            f = G.lookup(sd, raw)
            want = index[id(sd.ids[f.id])] if f is not None else -1
            rows.append(struct.pack("<IIIi", bi, 0, len(raw), want) + raw + bytes(-len(raw) % 4))
            queries.append((c.name, raw, want))
    data = struct.pack("<I", len(blobs)) + b"".join(blobs) + struct.pack("<I", len(rows)) + b"".join(rows)
    return data, queries


@pytest.fixture(scope="module")
def keys(tmp_path_factory):
    if not os.path.exists(B.HIPCC):
        pytest.skip("no %s to build the host lookups with" % B.HIPCC)
    lib = C.CDLL(build_keys(str(tmp_path_factory.mktemp("keys") / "libkeys.so"), ("-shared",)))
    lib.keys_run.restype = C.c_long
    lib.keys_run.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p]
    return lib


def test_lookups_equal_the_name_map(keys):
    data, queries = corpus()
    out = np.full(4 * len(queries), -9, dtype=np.int32)
    wrong = keys.keys_run(data, len(data), out.ctypes.data)
    out = out.reshape(-1, 4)
    bad = [(q, tuple(o)) for q, o in zip(queries, out.tolist()) if o[0] != q[2] or o[1] != q[2] or o[2] != 0]
    assert not bad and wrong == 0, (wrong, len(bad), bad[:6])
    # the corpus does what it says: hits and misses, misses whose length equals a name's
    # (key_eq decides), keys on both sides of the word and 16-byte seams, NUL tails
    hits = sum(q[2] >= 0 for q in queries)
    assert hits >= 90 and len(queries) - hits >= 2000, (hits, len(queries))
    assert sum(q[2] < 0 and o[3] > 0 for q, o in zip(queries, out.tolist())) >= 1000
    lens = {len(q[1]) for q in queries if q[2] >= 0}
    assert lens >= set(range(41))
    assert sum(q[1].endswith(b"\x00") and q[2] < 0 for q in queries) >= 400
    for name in ("N1", "N16", "N17", "NL", "Aliases", "Ids"):
        assert any(q[0] == name and q[2] >= 0 for q in queries) and any(q[0] == name and q[2] < 0 for q in queries)
