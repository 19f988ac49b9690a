"""Batched GetByPath over Thrift-binary messages on the GPU: the reference's
thrift/generic Node.GetByPath / Value.GetByPath (node.go:431-484,
value.go:102-161) for every message of a batch and every path of a set in one
launch (include/dgj2t.h dg_path_* / dg_tget_*). Nothing but field headers is
decoded; a result is the sub-value's byte span and wire type.

    paths = [[PathFieldId(255), PathFieldName("LogID")], [PathFieldId(3), PathFieldId(9), PathStrKey("b")]]
    for per_msg in get_by_path_batch(msgs, paths, desc):
        log_id, b = per_msg            # .status .type .start .end .raw .error
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .conv import Context, default_context
from .http import ConvError

STRUCT, MAP, SET, LIST = 12, 13, 14, 15
OK, NOT_FOUND, E_READ, E_TYPE = 0, 1, 2, 3  # DG_TGET_* (include/dgj2t_defs.h)
ERROR_NAMES = {OK: None, NOT_FOUND: "ErrNotFound", E_READ: "ErrRead", E_TYPE: "ErrDismatchType"}
PATH_MAGIC, PATH_VERSION = 0x31504744, 1
MAX_PATHS, MAX_STEPS = 8, 16
PS_FIELD, PS_INDEX, PS_STRKEY, PS_INTKEY, PS_BINKEY = 1, 2, 3, 4, 5
_PS_NAME = 0  # PathFieldName: host only, resolved to PS_FIELD by compile_paths

REC_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("type", "u1"), ("status", "u1"), ("step", "<u2"),
                      ("aux", "<u4")])  # dg_tget_rec


class Path:
    """One step of a path (thrift/generic/path.go Path)."""
    __slots__ = ("kind", "val")

    def __init__(self, kind: int, val):
        self.kind = kind
        self.val = val

    def __repr__(self):
        return "Path(%s, %r)" % (["name", "field", "index", "strkey", "intkey", "binkey"][self.kind], self.val)


def PathFieldId(fid: int) -> Path:
    if not -32768 <= int(fid) <= 32767:
        raise ValueError("field id %d outside int16" % fid)
    return Path(PS_FIELD, int(fid))


def PathFieldName(name: str) -> Path:
    return Path(_PS_NAME, name)


def PathIndex(i: int) -> Path:
    """The reference takes a negative index as it comes: its `id >= size`
    test (node.go:321) lets it through, no element is skipped and whatever
    follows the list header is read as the element, even in an empty list:
    undefined results. Here it is a ValueError (and DG_E_ARG in the C ABI)."""
    if int(i) < 0:
        raise ValueError("negative path index %d" % i)
    return Path(PS_INDEX, int(i))


def PathStrKey(key) -> Path:
    return Path(PS_STRKEY, key.encode() if isinstance(key, str) else bytes(key))


def PathIntKey(key: int) -> Path:
    if not -(1 << 63) <= int(key) < (1 << 63):
        raise ValueError("int key %d outside int64" % key)
    return Path(PS_INTKEY, int(key))


def PathBinKey(key: bytes) -> Path:
    """The key as its Thrift-binary encoding stands in the message (an i32
    key 2: 00 00 00 02; a string key: its 4-byte length, then its bytes)."""
    return Path(PS_BINKEY, bytes(key))


def _resolve(path: Sequence[Path], desc) -> List[Path]:
    """PathFieldName -> PathFieldId through the descriptor, walking it along
    the path as Value.GetByPath does (value.go:118-143): a field step moves to
    the field's type, an index or key step to the element type."""
    out = []
    d = desc
    for st in path:
        if st.kind == _PS_NAME:
            if d is None or d.struct is None:
                raise ConvError("ErrUnsupportedType", "field name '%s' needs a struct descriptor" % st.val)
            f = d.struct.names.get(st.val)
            if f is None:
                raise ConvError("ErrUnknownField", "field name '%s' is not defined in IDL" % st.val)
            out.append(Path(PS_FIELD, f.id))
            d = f.type
            continue
        out.append(st)
        if d is None:
            continue
        if st.kind == PS_FIELD:
            f = d.struct.field_by_id(st.val) if d.struct is not None else None
            d = f.type if f is not None else None
        else:
            d = d.elem
    return out


def compile_paths(paths: Sequence[Sequence[Path]], desc=None) -> bytes:
    """The path-set blob dg_path_create takes (layout: include/dgj2t_defs.h,
    DG_PATH_MAGIC). 1 to 8 paths of up to 16 steps; names are resolved through
    `desc` (a thrift.TypeDescriptor) and raise ConvError("ErrUnknownField")
    with the reference's text when the IDL does not define them."""
    paths = [_resolve(p, desc) for p in paths]
    if not 1 <= len(paths) <= MAX_PATHS:
        raise ValueError("%d paths (1 to %d)" % (len(paths), MAX_PATHS))
    ents, steps, pool = bytearray(), bytearray(), bytearray()
    n_steps = 0
    for p in paths:
        if len(p) > MAX_STEPS:
            raise ValueError("a path of %d steps (at most %d)" % (len(p), MAX_STEPS))
        ents += struct.pack("<II", n_steps, len(p))
        for st in p:
            if st.kind in (PS_STRKEY, PS_BINKEY):
                steps += struct.pack("<IIq", st.kind, len(st.val), len(pool))
                pool += st.val
            else:
                if st.kind == PS_INDEX and st.val < 0:
                    raise ValueError("negative path index %d" % st.val)
                steps += struct.pack("<IIq", st.kind, 0, st.val)
            n_steps += 1
    off_steps = (32 + len(ents) + 7) & ~7
    off_pool = off_steps + len(steps)
    hdr = struct.pack("<8I", PATH_MAGIC, PATH_VERSION, off_pool + len(pool), len(paths), n_steps, off_steps, off_pool,
                      len(pool))
    return hdr + bytes(ents) + b"\0" * (off_steps - 32 - len(ents)) + bytes(steps) + bytes(pool)


class PathSet:
    """A compiled path set on one context's device (dg_path)."""

    def __init__(self, paths, desc=None, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.blob = paths if isinstance(paths, (bytes, bytearray)) else compile_paths(paths, desc)
        h = C.c_void_p()
        _lib.check(_lib.lib().dg_path_create(self.ctx.h, bytes(self.blob), len(self.blob), C.byref(h)))
        self.h = h
        self.count = int(_lib.lib().dg_path_count(h))

    def close(self):
        if self.h:
            _lib.lib().dg_path_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Result:
    """One path on one message: .status (OK / NOT_FOUND / E_READ / E_TYPE),
    .type (wire type), .start / .end (the span in the message), .step, .aux,
    .raw (the sub-value's bytes, empty unless OK), .error (None, "ErrNotFound",
    "ErrRead" or "ErrDismatchType": the meta error the reference returns)."""
    __slots__ = ("status", "type", "start", "end", "step", "aux", "raw", "error")

    def __init__(self, rec, msg: bytes):
        self.start, self.end = int(rec["start"]), int(rec["end"])
        self.type, self.status = int(rec["type"]), int(rec["status"])
        self.step, self.aux = int(rec["step"]), int(rec["aux"])
        self.raw = msg[self.start:self.end] if self.status == OK else b""
        self.error = ERROR_NAMES.get(self.status, "ErrRead")

    def __repr__(self):
        return "Result(status=%d, type=%d, span=[%d,%d), step=%d)" % (self.status, self.type, self.start, self.end,
                                                                       self.step)


def get_by_path_records(msgs: Sequence[bytes], paths, desc=None, root_type: int = STRUCT,
                        ctx: Optional[Context] = None) -> np.ndarray:
    """The records of dg_tget_batch_host as a (len(msgs), P) array of REC_DTYPE."""
    ps = paths if isinstance(paths, PathSet) else PathSet(paths, desc, ctx)
    try:
        n = len(msgs)
        rec = np.zeros((n, ps.count), dtype=REC_DTYPE)
        if n == 0:
            _lib.check(_lib.lib().dg_tget_batch_host(ps.ctx.h, ps.h, root_type, None, None, 0, None))
            return rec
        lens = np.fromiter((len(m) for m in msgs), dtype=np.uint64, count=n)
        in_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(lens, out=in_off[1:])
        arena = np.frombuffer(b"".join(msgs) + b"\0" * 16, dtype=np.uint8)
        _lib.check(_lib.lib().dg_tget_batch_host(ps.ctx.h, ps.h, root_type, arena.ctypes.data, in_off.ctypes.data, n,
                                                 rec.ctypes.data))
        return rec
    finally:
        if ps is not paths:
            ps.close()


def get_by_path_batch(msgs: Sequence[bytes], paths, desc=None, root_type: int = STRUCT,
                      ctx: Optional[Context] = None) -> List[List[Result]]:
    """Every path of `paths` (a list of paths, each a list of Path steps, or a
    PathSet) on every message: result[i][k] is path k on msgs[i]."""
    rec = get_by_path_records(msgs, paths, desc, root_type, ctx)
    return [[Result(rec[i, k], msgs[i]) for k in range(rec.shape[1])] for i in range(len(msgs))]


def _ptr(x) -> Optional[int]:
    if x is None:
        return None
    return int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x)


def get_by_path_device(paths: PathSet, thrift, in_off, n: int, rec, val_off=None, val_len=None,
                       root_type: int = STRUCT, stream=None, max_len: int = 0):
    """Device-resident batch (dg_tget_batch_device) over torch tensors or raw
    device pointers: thrift uint8[>= in_off[n] + 16]; in_off int64[n + 1]; rec
    n * P 16-byte records (e.g. an int32 tensor of shape (n, P, 4)); val_off
    int64[n * P] and val_len int32[n * P] optional (what dg_pack_device_scan
    takes). Asynchronous on `stream` (a torch stream, a raw stream handle, or
    None for torch's current stream when `thrift` is a tensor)."""
    if stream is None and hasattr(thrift, "device"):
        import torch
        stream = torch.cuda.current_stream(thrift.device)
    s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    _lib.check(_lib.lib().dg_tget_batch_device(paths.ctx.h, paths.h, root_type, _ptr(thrift), _ptr(in_off), n, _ptr(rec),
                                               _ptr(val_off), _ptr(val_len), s, max_len))
