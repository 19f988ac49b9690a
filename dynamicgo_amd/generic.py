"""thrift/generic on the GPU. Row column writes (the last part of this
module: RowValuePlan, row_values_batch, row_values_device, set_rows_batch,
build_row_lists_batch: NewNodeList / NewNodeSet of structs over row tensors),
entry column writes (EntryValuePlan, entry_values_batch, entry_values_device),
typed column writes (the part before them: ValuePlan, values_batch,
values_device, set_columns_batch, build_structs_batch: the NewNode*
constructors over tensors), row columns
(RowPlan, rows_batch, rows_device, row_list_device: the fields of every element
of a list as ragged tensors), entry columns
(the part before them: EntryPlan, entries_batch, entries_device,
entry_emit_device: GetByPath followed by Node.List of strings / StrMap / IntMap
as ragged tensors), typed column
reads (the part before that: ColumnPlan, columns_batch, columns_device, column_list_device:
GetByPath followed by Node.Int / Float64 / String / List ... as tensors),
batched SetMany (EditManyPlan, set_many_batch,
unset_many_batch, edit_many_device: several children of one node edited in one
pass), batched Children (the fourth part of this
module: children_batch, children_records, children_device), batched
SetByPath / UnsetByPath (the third
part of this module: EditPlan, set_by_path_batch, unset_by_path_batch,
edit_device), batched MarshalTo ("cutting", Value.MarshalTo,
value.go:375-552; the second half of this module: compile_cut, CutPlan,
marshal_to_batch, marshal_to_device), and
batched GetByPath over Thrift-binary messages: the reference's
thrift/generic Node.GetByPath / Value.GetByPath (node.go:431-484,
value.go:102-161) for every message of a batch and every path of a set in one
launch (include/dgj2t.h dg_path_* / dg_tget_*). Nothing but field headers is
decoded; a result is the sub-value's byte span and wire type.

    paths = [[PathFieldId(255), PathFieldName("LogID")], [PathFieldId(3), PathFieldId(9), PathStrKey("b")]]
    for per_msg in get_by_path_batch(msgs, paths, desc):
        log_id, b = per_msg            # .status .type .start .end .raw .error
"""
from __future__ import annotations

import contextlib
import ctypes as C
import operator
import struct
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._batch import arena as _arena, split as _split, until_fits as _until_fits
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
    return _resolve_to(path, desc)[0]


def _resolve_to(path: Sequence[Path], desc):
    """_resolve's steps and the descriptor the path ends at (None when it is not known)."""
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
    return out, d


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


class _Handle:
    """What the plan classes share: .h, a handle of the library that
    close() gives to the function named _destroy, and `with`."""
    _destroy = None
    h = None

    def close(self):
        if self.h:
            getattr(_lib.lib(), self._destroy)(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class _KindPlan(_Handle):
    """What ColumnPlan and EntryPlan share: the constructor of a plan of
    (path, kind) columns. A class names the library's create and count entries
    (_create, _count) and the function that resolves a kind (_kind)."""
    _create = _count = _kind = None

    def __init__(self, columns, desc=None, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.kinds = [self._kind(k) for _, k in columns]
        self.blob = compile_paths([p for p, _ in columns], desc)
        h = C.c_void_p()
        _lib.check(getattr(_lib.lib(), self._create)(self.ctx.h, self.blob, len(self.blob), bytes(self.kinds),
                                                     len(self.kinds), C.byref(h)))
        self.h = h
        self.count = int(getattr(_lib.lib(), self._count)(h))


@contextlib.contextmanager
def _unless_given(made, given):
    """Closes `made` after the block unless it is the caller's own `given`."""
    try:
        yield
    finally:
        if made is not given:
            made.close()


class PathSet(_Handle):
    """A compiled path set on one context's device (dg_path)."""
    _destroy = "dg_path_destroy"

    def __init__(self, paths, desc=None, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.blob = paths if isinstance(paths, (bytes, bytearray)) else compile_paths(paths, desc)
        h = C.c_void_p()
        _lib.check(_lib.lib().dg_path_create(self.ctx.h, bytes(self.blob), len(self.blob), C.byref(h)))
        self.h = h
        self.count = int(_lib.lib().dg_path_count(h))


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
    with _unless_given(ps, paths):
        n = len(msgs)
        rec = np.zeros((n, ps.count), dtype=REC_DTYPE)
        if n == 0:
            _lib.check(_lib.lib().dg_tget_batch_host(ps.ctx.h, ps.h, root_type, None, None, 0, None))
            return rec
        arena, in_off = _arena(msgs)
        _lib.check(_lib.lib().dg_tget_batch_host(ps.ctx.h, ps.h, root_type, arena.ctypes.data, in_off.ctypes.data, n,
                                                 rec.ctypes.data))
        return rec


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


def _stream_handle(stream, thrift):
    """A torch stream, a raw stream handle, or None for torch's current stream
    when `thrift` is a tensor -> the raw handle."""
    if stream is None and hasattr(thrift, "device"):
        import torch
        stream = torch.cuda.current_stream(thrift.device)
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream


def get_by_path_device(paths: PathSet, thrift, in_off, n: int, rec, val_off=None, val_len=None,
                       root_type: int = STRUCT, stream=None, max_len: int = 0):
    """Device-resident batch (dg_tget_batch_device) over torch tensors or raw
    device pointers: thrift uint8[>= in_off[n] + 16]; in_off int64[n + 1]; rec
    n * P 16-byte records (e.g. an int32 tensor of shape (n, P, 4)); val_off
    int64[n * P] and val_len int32[n * P] optional (what dg_pack_device_scan
    takes). Asynchronous on `stream` (a torch stream, a raw stream handle, or
    None for torch's current stream when `thrift` is a tensor)."""
    s = _stream_handle(stream, thrift)
    _lib.check(_lib.lib().dg_tget_batch_device(paths.ctx.h, paths.h, root_type, _ptr(thrift), _ptr(in_off), n, _ptr(rec),
                                               _ptr(val_off), _ptr(val_len), s, max_len))


# ---------------------------------------------------------------------------
# MarshalTo ("cutting"): a message written under a wide descriptor re-emitted
# under a narrower one (thrift/generic/value.go:375-552; dg_cut_* in dgj2t.h)
# ---------------------------------------------------------------------------
CUT_MAGIC, CUT_VERSION = 0x31434744, 1  # DG_CUT_MAGIC (include/dgj2t_defs.h)
CUT_MAX_DEPTH = 64  # DG_CUT_MAX_DEPTH
CUT_COPY, CUT_MISMATCH, CUT_LIST, CUT_MAP, CUT_STRUCT = 1, 2, 3, 4, 5
CUT_DROP, CUT_NO_BIT = 0xFFFFFFFF, 0xFF
CUT_WRITE_DEFAULT, CUT_DISALLOW_UNKNOWN, CUT_NOT_CHECK_REQ = 1, 2, 4
CUT_OK, CUT_E_READ, CUT_E_TYPE, CUT_E_UNKNOWN, CUT_E_REQUIRED, CUT_E_DEPTH, CUT_E_OVERFLOW = 0, 1, 2, 3, 4, 5, 0xF0
CUT_ERROR_NAMES = {CUT_OK: None, CUT_E_READ: "ErrRead", CUT_E_TYPE: "ErrDismatchType",
                   CUT_E_UNKNOWN: "ErrUnknownField", CUT_E_REQUIRED: "ErrMissRequiredField",
                   CUT_E_DEPTH: "ErrDepth", CUT_E_OVERFLOW: "ErrOverflow"}
_CUT_HDR, _CUT_NODE, _CUT_FIELD, _CUT_LIT = "<16I", "<6I2Q", "<hBBI", "<hHI"
_REQUIRED = 2  # thrift.REQUIRED


def same_descriptor(a, b) -> bool:
    """The reference compares descriptor pointers (`to.Elem() == from.Elem()`)
    and shares its builtin descriptors (thrift/idl.go:540-551); thrift.py's
    builtin() makes a new object per use. So two descriptors are the same when
    they are the same Python object, or when both are base types (no struct,
    key or elem) of equal `type` and `name`."""
    if a is b:
        return True
    if a is None or b is None:
        return False

    def base(d):
        return d.struct is None and d.key is None and d.elem is None

    return base(a) and base(b) and a.type == b.type and a.name == b.name


def write_empty(td) -> bytes:
    """BinaryProtocol.WriteEmpty (thrift/binary.go:483-515)."""
    t = td.type
    fixed = {2: 1, 3: 1, 6: 2, 8: 4, 10: 8, 4: 8, 11: 4}  # a string: its zero length
    if t in fixed:
        return b"\0" * fixed[t]
    if t in (LIST, SET):
        return bytes([td.elem.type]) + b"\0\0\0\0"
    if t == MAP:
        return bytes([td.key.type, td.elem.type]) + b"\0\0\0\0"
    if t == STRUCT:
        return b"\0"  # "to avoid self-cycled type dead loop here, just write empty struct"
    raise ValueError("invalid type %d" % t)


def compile_cut(from_desc, to_desc) -> bytes:
    """The cut plan dg_cut_create takes (layout: include/dgj2t_defs.h,
    DG_CUT_MAGIC): the graph of (from, to) descriptor pairs marshalTo can
    reach, walked once and memoised on (id(from), id(to)), so recursive
    descriptors terminate. Per pair, as value.go:392-543 decides it: a `to`
    struct is cut field by field; a `to` list, set or map whose element (and
    key) descriptors are not the same as `from`'s (same_descriptor: the same
    object, or base types of equal type and name) is cut entry by entry;
    everything else is a whole-value copy when the two types are equal and
    ErrDismatchType, raised when such a value is reached in a message, when
    they are not.

    Where this differs from the reference:
      * the same struct descriptor on both sides (value.go:395-397 returns
        without reading, which desynchronises its reader): ValueError;
      * `to` is a struct and `from` is not (a nil dereference there):
        ValueError;
      * differing root types: ConvError("ErrDismatchType"), as MarshalTo
        returns it before reading;
      * a `to` struct with more than 64 tracked fields (StructDescriptor.requires
        set), or a tracked field with a negative id (RequiresBitmap.Set
        panics on one): ValueError -- the live mask is one 64-bit word;
      * more than CUT_MAX_DEPTH cut containers open in a message end it with
        CUT_E_DEPTH (the reference recurses without limit); nesting inside a
        skipped or copied value is not counted and keeps SkipType's 1023."""
    if from_desc.type != to_desc.type:
        raise ConvError("ErrDismatchType", "to descriptor dismatches from descriptor")
    nodes, fields, lits, pool = [], [], [], bytearray()
    memo = {}
    keep = []  # the descriptors whose id() keys the memo
    max_unset = 0

    def skip_val(f, t):
        return (CUT_COPY, t.type) if f.type == t.type else (CUT_MISMATCH, 0)

    def node(f, t) -> int:
        nonlocal max_unset
        key = (id(f), id(t))
        if key in memo:
            return memo[key]
        idx = memo[key] = len(nodes)
        keep.append((f, t))
        nodes.append(None)
        tt = t.type
        row = None
        if tt == STRUCT:
            if f is t or (f.struct is not None and f.struct is t.struct):
                raise ValueError("the same struct descriptor '%s' on both sides of a cut" % t.name)
            if f.type != STRUCT or f.struct is None or t.struct is None:
                raise ValueError("'%s' is a struct in the to descriptor and none in the from descriptor" % t.name)
            tracked = sorted(fid for fid, on in t.struct.requires.items() if on)
            if len(tracked) > 64:
                raise ValueError("struct '%s': %d tracked fields (at most 64)" % (t.name, len(tracked)))
            if tracked and tracked[0] < 0:
                raise ValueError("struct '%s': tracked field id %d is negative" % (t.name, tracked[0]))
            bit_of = {fid: k for k, fid in enumerate(tracked)}
            required, unset = 0, 0
            lit0 = len(lits)
            for k, fid in enumerate(tracked):
                tf = t.struct.field_by_id(fid)
                if tf.required == _REQUIRED:
                    required |= 1 << k
                    lits.append(struct.pack(_CUT_LIT, fid, 0, 0))
                else:
                    lit = struct.pack(">Bh", tf.type.type, fid) + write_empty(tf.type)
                    lits.append(struct.pack(_CUT_LIT, fid, len(lit), len(pool)))
                    pool.extend(lit)
                    unset += len(lit)
            max_unset = max(max_unset, unset)
            ffs = sorted(f.struct.ids.values(), key=lambda x: x.id)
            fld0 = len(fields)
            fields.extend([None] * len(ffs))  # the range stays contiguous while children add theirs
            for k, ff in enumerate(ffs):
                tf = t.struct.field_by_id(ff.id)
                child = CUT_DROP if tf is None else node(ff.type, tf.type)
                bit = CUT_NO_BIT if tf is None else bit_of.get(ff.id, CUT_NO_BIT)
                fields[fld0 + k] = struct.pack(_CUT_FIELD, ff.id, ff.type.type, bit, child)
            row = (CUT_STRUCT, fld0, 0, len(ffs), lit0, len(tracked), (1 << len(tracked)) - 1, required)
        elif tt in (LIST, SET):
            if f.type not in (LIST, SET):
                row = (CUT_MISMATCH, 0)
            elif same_descriptor(t.elem, f.elem):
                row = skip_val(f, t)
            else:
                row = (CUT_LIST, node(f.elem, t.elem))
        elif tt == MAP:
            if f.type != MAP:
                row = (CUT_MISMATCH, 0)
            elif same_descriptor(t.elem, f.elem) and same_descriptor(t.key, f.key):
                row = skip_val(f, t)
            else:
                row = (CUT_MAP, node(f.key, t.key), node(f.elem, t.elem))
        else:
            row = skip_val(f, t)
        row = tuple(row) + (0,) * (8 - len(row))
        nodes[idx] = struct.pack(_CUT_NODE, *row)
        return idx

    root = node(from_desc, to_desc)
    off_nodes = 64
    off_fields = off_nodes + 40 * len(nodes)
    off_lits = off_fields + 8 * len(fields)
    off_pool = off_lits + 8 * len(lits)
    hdr = struct.pack(_CUT_HDR, CUT_MAGIC, CUT_VERSION, off_pool + len(pool), root, len(nodes), off_nodes, len(fields),
                      off_fields, len(lits), off_lits, off_pool, len(pool), max_unset, 0, 0, 0)
    return hdr + b"".join(nodes) + b"".join(fields) + b"".join(lits) + bytes(pool)


class CutOptions:
    """thrift/generic Options as marshalTo reads them: WriteDefault,
    DisallowUnknow, NotCheckRequireNess."""
    __slots__ = ("write_default", "disallow_unknown", "not_check_requireness")

    def __init__(self, write_default=False, disallow_unknown=False, not_check_requireness=False):
        self.write_default = bool(write_default)
        self.disallow_unknown = bool(disallow_unknown)
        self.not_check_requireness = bool(not_check_requireness)

    def word(self) -> int:
        return (CUT_WRITE_DEFAULT * self.write_default | CUT_DISALLOW_UNKNOWN * self.disallow_unknown |
                CUT_NOT_CHECK_REQ * self.not_check_requireness)


def _cut_word(opts) -> int:
    return 0 if opts is None else opts.word() if hasattr(opts, "word") else int(opts)


class CutPlan(_Handle):
    """A compiled cut plan on one context's device (dg_cut)."""
    _destroy = "dg_cut_destroy"

    def __init__(self, from_desc, to_desc=None, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.blob = from_desc if isinstance(from_desc, (bytes, bytearray)) else compile_cut(from_desc, to_desc)
        h = C.c_void_p()
        _lib.check(_lib.lib().dg_cut_create(self.ctx.h, bytes(self.blob), len(self.blob), C.byref(h)))
        self.h = h

    def slot_bound(self, length: int, opts=None) -> int:
        return int(_lib.lib().dg_cut_slot_bound(self.h, length, _cut_word(opts)))


class CutResult:
    """One message: .status (CUT_OK, CUT_E_*), .raw (the cut message, empty
    unless CUT_OK), .error (None, "ErrRead", "ErrDismatchType",
    "ErrUnknownField", "ErrMissRequiredField", "ErrDepth"), .aux (the field id
    of a field-level error, sign-extended to 32 bits as the device stores it)."""
    __slots__ = ("status", "raw", "error", "aux")

    def __init__(self, ret: int, raw: bytes):
        self.status, self.aux = int(ret) & 0xFF, int(ret) >> 32
        self.raw = raw if self.status == CUT_OK else b""
        self.error = CUT_ERROR_NAMES.get(self.status, "ErrRead")

    def __repr__(self):
        return "CutResult(status=%d, aux=%d, %d bytes)" % (self.status, self.aux, len(self.raw))


def marshal_to_batch(msgs: Sequence[bytes], from_desc, to_desc=None, opts=None,
                     ctx: Optional[Context] = None) -> List[CutResult]:
    """Value.MarshalTo for every message of a batch (dg_cut_batch_host):
    msgs[i], written under from_desc, cut to to_desc. from_desc may be a
    CutPlan (to_desc is then unused). Descriptor sameness: same_descriptor."""
    plan = from_desc if isinstance(from_desc, CutPlan) else CutPlan(from_desc, to_desc, ctx)
    with _unless_given(plan, from_desc):
        n = len(msgs)
        L = _lib.lib()
        if n == 0:
            _lib.check(L.dg_cut_batch_host(plan.ctx.h, plan.h, _cut_word(opts), None, None, 0, None, 0, None, None, None))
            return []
        arena, in_off = _arena(msgs)
        out_off = np.zeros(n + 1, dtype=np.uint64)
        ret = np.zeros(n, dtype=np.uint64)
        need = C.c_uint64(0)

        def call(cap):
            out = np.zeros(cap, dtype=np.uint8)
            return L.dg_cut_batch_host(plan.ctx.h, plan.h, _cut_word(opts), arena.ctypes.data, in_off.ctypes.data, n,
                                       out.ctypes.data, cap, out_off.ctypes.data, ret.ctypes.data, C.byref(need)), out

        out = _until_fits(call, int(in_off[n]) + 4096, need)  # a guess the literals may outgrow
        return [CutResult(r, o) for r, o in zip(ret.tolist(), _split(out, out_off))]


def marshal_to_device(plan: CutPlan, thrift, in_off, n: int, out, out_off, out_len, ret, opts=None, stream=None,
                      max_len: int = 0):
    """Device-resident batch (dg_cut_batch_device) over torch tensors or raw
    device pointers: thrift uint8[>= in_off[n] + 16]; in_off int64[n + 1]; out
    uint8, message i's slot out[out_off[i], out_off[i + 1]) (out_off int64[n +
    1]; plan.slot_bound gives a size that cannot overflow); out_len int32[n];
    ret int64[n] (status | aux << 32). out must not alias thrift. Asynchronous
    on `stream` (a torch stream, a raw stream handle, or None for torch's
    current stream when `thrift` is a tensor)."""
    s = _stream_handle(stream, thrift)
    _lib.check(_lib.lib().dg_cut_batch_device(plan.ctx.h, plan.h, _cut_word(opts), _ptr(thrift), _ptr(in_off), n, _ptr(out),
                                              _ptr(out_off), _ptr(out_len), _ptr(ret), s, max_len))


# ---------------------------------------------------------------------------
# SetByPath / UnsetByPath: one path rewritten in every message of a batch
# (thrift/generic/value.go:263-333, node.go:825-920, 1009-1127; dg_edit_* in
# dgj2t.h)
# ---------------------------------------------------------------------------
EDIT_SET, EDIT_UNSET = 1, 2  # DG_EDIT_SET / DG_EDIT_UNSET (include/dgj2t_defs.h)
EDIT_OK, EDIT_NOT_FOUND, EDIT_E_READ, EDIT_E_TYPE, EDIT_E_OVERFLOW = 0, 1, 2, 3, 0xF0
EDIT_EXISTED = 1 << 8
EDITM_E_SAME = 5  # DG_EDITM_E_SAME: only a many-edit (EditManyPlan) returns it
EDIT_ERROR_NAMES = {EDIT_OK: None, EDIT_NOT_FOUND: "ErrNotFound", EDIT_E_READ: "ErrRead",
                    EDIT_E_TYPE: "ErrDismatchType", EDITM_E_SAME: "ErrSame", EDIT_E_OVERFLOW: "ErrOverflow"}


class EditPlan(_Handle):
    """One edit on one context's device (dg_edit): ONE path of at least one
    step (a list of Path steps; PathFieldName is resolved through `desc` by
    compile_paths) and an op, EDIT_SET or EDIT_UNSET. `path` may also be the
    compiled one-path blob.

    SET replaces the value at the path (its wire type must be the new
    value's), or, when only the path's last step misses, inserts it at the
    FRONT of the container: a field header + the value at the struct's first
    byte, an element after the list header, key + value after the map header,
    the container's count + 1. UNSET drops the field, element or map entry and
    writes count - 1; a missing PARENT leaves the message as it is.

    Where this differs from the reference:
      1. a missing field of a nested struct is inserted at the front of the
         struct that was searched (the reference inserts it at byte 0 of the
         root message: searchFieldId returns start 0 on a miss);
      2. the key of an int-key insert is encoded at the width of the map's own
         key type (the reference uses the value's type);
      3. an insert whose val_type is not the list's element / the map's value
         type is ErrDismatchType (the reference writes a corrupt message);
      4. unset of an absent map key is ErrNotFound (the reference deletes the
         map's last entry, and writes count -1 on an empty map);
      5. keys are matched as get_by_path_batch matches them, its I08 rule
         included, not by deleteChild's raw compare;
      6. unset on a parent that is no container is ErrDismatchType (the
         reference silently does nothing);
      7. the empty path (`*self = sub`) is refused: ValueError here, DG_E_ARG in
         the C ABI.
    Several children of one node in one pass: EditManyPlan (SetMany). Items
    under different parents stay a second edit on the first one's output."""
    _destroy = "dg_edit_destroy"

    def __init__(self, path, op: int, desc=None, ctx: Optional[Context] = None):
        self.op = int(op)
        if isinstance(path, (bytes, bytearray)):
            self.blob = bytes(path)
        else:
            if len(path) == 0:
                raise ValueError("the empty path is no edit")
            self.blob = compile_paths([path], desc)
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        _lib.check(_lib.lib().dg_edit_create(self.ctx.h, self.blob, len(self.blob), self.op, C.byref(h)))
        self.h = h

    def slot_bound(self, length: int, val_len: int = 0) -> int:
        """The exact worst case of one message's output (dg_edit_slot_bound)."""
        return int(_lib.lib().dg_edit_slot_bound(self.h, length, val_len))


class EditResult:
    """One message: .status (EDIT_OK, EDIT_NOT_FOUND, EDIT_E_READ, EDIT_E_TYPE),
    .existed (the path was there: a replace or a delete; False for an insert
    or an untouched message; set only with EDIT_OK), .raw (the edited message,
    empty unless EDIT_OK), .error (None, "ErrNotFound", "ErrRead",
    "ErrDismatchType"), .aux (the wire type a type error met, or the lookup's)."""
    __slots__ = ("status", "existed", "raw", "error", "aux")

    def __init__(self, ret: int, raw: bytes):
        self.status, self.aux = int(ret) & 0xFF, int(ret) >> 32
        self.existed = bool(int(ret) & EDIT_EXISTED)
        self.raw = raw if self.status == EDIT_OK else b""
        self.error = EDIT_ERROR_NAMES.get(self.status, "ErrRead")

    def __repr__(self):
        return "EditResult(status=%d, existed=%s, aux=%d, %d bytes)" % (self.status, self.existed, self.aux,
                                                                        len(self.raw))


def _edit_batch(msgs, plan: EditPlan, values, val_type: int, root_type: int) -> List[EditResult]:
    n = len(msgs)
    L = _lib.lib()
    if n == 0:
        _lib.check(L.dg_edit_batch_host(plan.ctx.h, plan.h, root_type, None, None, 0, val_type, None, None, 0, None, 0,
                                        None, None, None))
        return []
    arena, in_off = _arena(msgs)
    val = val_off = None
    val_len = vtotal = 0
    if values is not None:
        if isinstance(values, (bytes, bytearray)):
            val = np.frombuffer(bytes(values) + b"\0" * 16, dtype=np.uint8)
            val_len = len(values)
        else:
            if len(values) != n:
                raise ValueError("%d values for %d messages" % (len(values), n))
            val, val_off = _arena([bytes(v) for v in values])
            vtotal = int(val_off[n])
    out_off = np.zeros(n + 1, dtype=np.uint64)
    ret = np.zeros(n, dtype=np.uint64)
    need = C.c_uint64(0)

    def call(cap):
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        return L.dg_edit_batch_host(plan.ctx.h, plan.h, root_type, arena.ctypes.data, in_off.ctypes.data, n, val_type,
                                    None if val is None else val.ctypes.data,
                                    None if val_off is None else val_off.ctypes.data, val_len, out.ctypes.data, cap,
                                    out_off.ctypes.data, ret.ctypes.data, C.byref(need)), out

    out = _until_fits(call, int(in_off[n]) + vtotal, need)  # a guess the inserts may outgrow
    return [EditResult(r, o) for r, o in zip(ret.tolist(), _split(out, out_off))]


def set_by_path_batch(msgs: Sequence[bytes], path, values, val_type: int, desc=None, root_type: int = STRUCT,
                      ctx: Optional[Context] = None) -> List[EditResult]:
    """SetByPath for every message of a batch (dg_edit_batch_host): the value
    at `path` (a list of Path steps, or an EditPlan of op EDIT_SET) becomes
    `values`, one `bytes` for all messages or a sequence with one entry per
    message: the value's Thrift-binary bytes, taken as given, of wire type
    val_type. Semantics and the deviations from the reference: EditPlan."""
    plan = path if isinstance(path, EditPlan) else EditPlan(path, EDIT_SET, desc, ctx)
    with _unless_given(plan, path):
        if plan.op != EDIT_SET:
            raise ValueError("set_by_path_batch needs an EDIT_SET plan")
        return _edit_batch(msgs, plan, values, val_type, root_type)


def unset_by_path_batch(msgs: Sequence[bytes], path, desc=None, root_type: int = STRUCT,
                        ctx: Optional[Context] = None) -> List[EditResult]:
    """UnsetByPath for every message of a batch: the field, element or map
    entry at `path` (a list of Path steps, or an EditPlan of op EDIT_UNSET) is
    dropped. Semantics and the deviations from the reference: EditPlan."""
    plan = path if isinstance(path, EditPlan) else EditPlan(path, EDIT_UNSET, desc, ctx)
    with _unless_given(plan, path):
        if plan.op != EDIT_UNSET:
            raise ValueError("unset_by_path_batch needs an EDIT_UNSET plan")
        return _edit_batch(msgs, plan, None, 0, root_type)


def edit_device(plan: EditPlan, thrift, in_off, n: int, val_type: int, val, val_off, out, out_off, out_len, ret,
                root_type: int = STRUCT, val_len: int = 0, stream=None, max_len: int = 0):
    """Device-resident batch (dg_edit_batch_device) over torch tensors or raw
    device pointers: thrift uint8[>= in_off[n] + 16]; in_off int64[n + 1]; val
    uint8 with 16 spare bytes, val_off int64[n + 1] or None (then val[0,
    val_len) serves every message; with val_off, val_len is the longest value
    or 0); out uint8, message i's slot out[out_off[i], out_off[i + 1])
    (plan.slot_bound gives the size that cannot overflow); out_len int32[n];
    ret int64[n] (status | EDIT_EXISTED | aux << 32). An UNSET plan ignores
    val_type, val, val_off and val_len. out must not alias thrift. max_len,
    when given, must not be less than the longest message. Asynchronous on
    `stream` (a torch stream, a raw stream handle, or None for torch's current
    stream when `thrift` is a tensor)."""
    s = _stream_handle(stream, thrift)
    _lib.check(_lib.lib().dg_edit_batch_device(plan.ctx.h, plan.h, root_type, _ptr(thrift), _ptr(in_off), n, val_type,
                                               _ptr(val), _ptr(val_off), val_len, _ptr(out), _ptr(out_off),
                                               _ptr(out_len), _ptr(ret), s, max_len))


# ---------------------------------------------------------------------------
# SetMany: several children of one node rewritten in one pass over every
# message of a batch (thrift/generic/node.go:930-1007; dg_editm_* in dgj2t.h)
# ---------------------------------------------------------------------------
EDITM_MAX_ITEMS = MAX_PATHS - 1  # DG_EDITM_MAX_ITEMS


def _step_class(kind: int) -> int:
    return 0 if kind == PS_FIELD else 1 if kind == PS_INDEX else 2


class EditManyPlan(_Handle):
    """One many-edit on one context's device (dg_editm): a `parent` path of 0
    to 15 steps, 1 to 7 last `steps` below it and an op. Every step is one
    Path; all are of one class: all fields (PathFieldId / PathFieldName,
    resolved through `desc` by compile_paths), all indexes, or all keys
    (PathStrKey, PathIntKey and PathBinKey may mix).

    EDIT_SET: every item is decided as EditPlan decides a single SET. Found
    items are replaced in place; missing ones are all inserted at the front
    of the container in the order given, and the count is patched once.
    EDIT_UNSET: every item is decided as a single UNSET on the ORIGINAL
    message (indexes do not shift between items). A message is edited as a
    whole or not at all: the first failing item in item order gives the
    message its status.

    Where this differs from the reference, besides EditPlan's 1 to 7:
      8. a replace checks the wire type (replaceMany does not);
      9. items that resolve to overlapping spans (a string key and the same
         key as a binary key, an existing index twice) are ErrSame (the
         reference writes a corrupt buffer); two MISSING duplicates are a
         legal double insert;
      10. mixed step classes are refused: ValueError here, DG_E_ARG in the C
          ABI."""
    _destroy = "dg_editm_destroy"

    def __init__(self, parent, steps, op: int, desc=None, ctx: Optional[Context] = None):
        self.op = int(op)
        steps = list(steps)
        if not 1 <= len(steps) <= EDITM_MAX_ITEMS:
            raise ValueError("%d items (1 to %d)" % (len(steps), EDITM_MAX_ITEMS))
        paths = [_resolve(list(parent) + [st], desc) for st in steps]
        if len({_step_class(p[-1].kind) for p in paths}) != 1:
            raise ValueError("mixed step classes")
        self.k = len(steps)
        self.blob = compile_paths(paths)
        self.ctx = ctx or default_context()
        h = C.c_void_p()
        _lib.check(_lib.lib().dg_editm_create(self.ctx.h, self.blob, len(self.blob), self.op, C.byref(h)))
        self.h = h

    def slot_bound(self, length: int, val_total: int = 0) -> int:
        """The exact worst case of one message's output (dg_editm_slot_bound);
        val_total: the K values' lengths together."""
        return int(_lib.lib().dg_editm_slot_bound(self.h, length, val_total))


class EditManyResult:
    """One message: .status (EDIT_OK, EDIT_NOT_FOUND, EDIT_E_READ, EDIT_E_TYPE,
    EDITM_E_SAME), .existed (a tuple of K bools: item j was a replace or a
    drop; all False unless EDIT_OK), .item (the failing item, 0 when OK),
    .aux, .raw (the edited message, empty unless EDIT_OK), .error (None,
    "ErrNotFound", "ErrRead", "ErrDismatchType", "ErrSame")."""
    __slots__ = ("status", "existed", "item", "raw", "error", "aux")

    def __init__(self, ret: int, raw: bytes, k: int):
        ret = int(ret)
        self.status, self.aux = ret & 0xFF, ret >> 32
        self.existed = tuple(bool(ret >> (8 + j) & 1) for j in range(k))
        self.item = ret >> 16 & 7
        self.raw = raw if self.status == EDIT_OK else b""
        self.error = EDIT_ERROR_NAMES.get(self.status, "ErrRead")

    def __repr__(self):
        return "EditManyResult(status=%d, existed=%s, item=%d, aux=%d, %d bytes)" % (
            self.status, self.existed, self.item, self.aux, len(self.raw))


def _editm_batch(msgs, plan: EditManyPlan, values, val_types, root_type: int, encoded=None) -> List[EditManyResult]:
    """encoded: (val, val_off) of values_batch instead of `values`"""
    n, k = len(msgs), plan.k
    L = _lib.lib()
    vt = np.asarray(val_types if val_types is not None else [0] * k, dtype=np.uint8)
    vl = np.zeros(k, dtype=np.uint64)
    if n == 0:
        _lib.check(L.dg_editm_batch_host(plan.ctx.h, plan.h, root_type, None, None, 0, vt.ctypes.data, None, None,
                                         vl.ctypes.data, None, 0, None, None, None))
        return []
    arena, in_off = _arena(msgs)
    val = val_off = None
    vtotal = 0
    if encoded is not None:
        val, val_off = np.concatenate([encoded[0], np.zeros(16, dtype=np.uint8)]), encoded[1]
        vtotal = int(val_off[n * k])
    elif values is not None:
        if all(isinstance(v, (bytes, bytearray)) for v in values):
            vl[:] = [len(v) for v in values]
            val = np.frombuffer(b"".join(bytes(v) for v in values) + b"\0" * 16, dtype=np.uint8)
        else:
            for v in values:
                if not isinstance(v, (bytes, bytearray)) and len(v) != n:
                    raise ValueError("%d values for %d messages" % (len(v), n))
            val, val_off = _arena([bytes(v) if isinstance(v, (bytes, bytearray)) else bytes(v[i])
                                   for i in range(n) for v in values])
            vtotal = int(val_off[n * k])
    out_off = np.zeros(n + 1, dtype=np.uint64)
    ret = np.zeros(n, dtype=np.uint64)
    need = C.c_uint64(0)

    def call(cap):
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        return L.dg_editm_batch_host(plan.ctx.h, plan.h, root_type, arena.ctypes.data, in_off.ctypes.data, n,
                                     vt.ctypes.data, None if val is None else val.ctypes.data,
                                     None if val_off is None else val_off.ctypes.data, vl.ctypes.data, out.ctypes.data,
                                     cap, out_off.ctypes.data, ret.ctypes.data, C.byref(need)), out

    out = _until_fits(call, int(in_off[n]) + vtotal, need)  # a guess the inserts may outgrow
    return [EditManyResult(r, o, k) for r, o in zip(ret.tolist(), _split(out, out_off))]


def set_many_batch(msgs: Sequence[bytes], parent, items, desc=None, root_type: int = STRUCT,
                   ctx: Optional[Context] = None) -> List[EditManyResult]:
    """SetMany for every message of a batch (dg_editm_batch_host): below the
    node at `parent` (a list of Path steps, possibly empty), every item
    (step, value_or_values, val_type) sets the child at `step` to the value's
    Thrift-binary bytes, taken as given, of wire type val_type: one `bytes`
    for all messages or a sequence with one entry per message. `parent` may
    be an EditManyPlan of op EDIT_SET; its steps are then the plan's and the
    items' steps are not looked at. Semantics: EditManyPlan."""
    plan = parent if isinstance(parent, EditManyPlan) else \
        EditManyPlan(parent, [it[0] for it in items], EDIT_SET, desc, ctx)
    with _unless_given(plan, parent):
        if plan.op != EDIT_SET or plan.k != len(items):
            raise ValueError("set_many_batch needs an EDIT_SET plan of as many steps as items")
        return _editm_batch(msgs, plan, [it[1] for it in items], [it[2] for it in items], root_type)


def unset_many_batch(msgs: Sequence[bytes], parent, steps=None, desc=None, root_type: int = STRUCT,
                     ctx: Optional[Context] = None) -> List[EditManyResult]:
    """The UNSET counterpart: the children at `steps` below `parent` (or an
    EditManyPlan of op EDIT_UNSET) are dropped from every message, every step
    addressing the original message. Semantics: EditManyPlan."""
    plan = parent if isinstance(parent, EditManyPlan) else EditManyPlan(parent, steps, EDIT_UNSET, desc, ctx)
    with _unless_given(plan, parent):
        if plan.op != EDIT_UNSET:
            raise ValueError("unset_many_batch needs an EDIT_UNSET plan")
        return _editm_batch(msgs, plan, None, None, root_type)


def edit_many_device(plan: EditManyPlan, thrift, in_off, n: int, val_types, val, val_off, val_lens, out, out_off,
                     out_len, ret, root_type: int = STRUCT, stream=None, max_len: int = 0):
    """Device-resident batch (dg_editm_batch_device) over torch tensors or raw
    device pointers, as edit_device. val_types and val_lens are HOST
    sequences of K entries; val uint8 with 16 spare bytes; val_off
    int64[n * K + 1], message-major (item j of message i is val[val_off[i*K+j],
    val_off[i*K+j+1]); val_lens[j] is then item j's longest value or 0), or
    None: val holds the K values back to back, val_lens[j] bytes each, for
    every message. ret int64[n]: status | existed mask << 8 | failing item
    << 16 | aux << 32. An UNSET plan ignores the value arguments."""
    s = _stream_handle(stream, thrift)
    vt = np.asarray(val_types if val_types is not None else [0] * plan.k, dtype=np.uint8)
    vl = np.asarray(val_lens if val_lens is not None else [0] * plan.k, dtype=np.uint64)
    if len(vt) != plan.k or len(vl) != plan.k:
        raise ValueError("val_types / val_lens need %d entries" % plan.k)
    _lib.check(_lib.lib().dg_editm_batch_device(plan.ctx.h, plan.h, root_type, _ptr(thrift), _ptr(in_off), n,
                                                vt.ctypes.data, _ptr(val), _ptr(val_off), vl.ctypes.data, _ptr(out),
                                                _ptr(out_off), _ptr(out_len), _ptr(ret), s, max_len))


# ---------------------------------------------------------------------------
# Children: the table of a node's children, or its whole subtree, for every
# message of a batch (thrift/generic/node.go:1133-1154, path.go:796-836,
# 1121-1248; dg_kids_* in dgj2t.h)
# ---------------------------------------------------------------------------
KIDS_E_UNSUPPORTED, KIDS_E_OVERFLOW = 4, 0xF0  # DG_KIDS_E_* (include/dgj2t_defs.h)
KIDS_F_RECURSE, KIDS_F_COUNTED = 1, 2
KIDS_NO_PARENT = 0xFFFFFFFF
KIDS_ERROR_NAMES = dict(ERROR_NAMES)
KIDS_ERROR_NAMES.update({KIDS_E_UNSUPPORTED: "ErrUnsupportedType", KIDS_E_OVERFLOW: "ErrOverflow"})
KIDS_REC_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("key_start", "<u4"), ("parent", "<u4"), ("key", "<i8"),
                           ("type", "u1"), ("kind", "u1"), ("depth", "<u2"), ("n_desc", "<u4")])  # dg_kid_rec
KIDS_HEAD_DTYPE = np.dtype([("count", "<u4"), ("direct", "<u4"), ("start", "<u4"), ("type", "u1"), ("key_type", "u1"),
                            ("elem_type", "u1"), ("status", "u1")])  # dg_kids_head


class Child:
    """One child: .path (the step that reaches it from its parent, built by
    PathFieldId / PathIndex / PathIntKey, or PathStrKey / PathBinKey over the
    key's bytes in the message), .type (wire type), .start / .end (the value's
    span in the message), .raw, .parent (index
    of the enclosing child in the message's list, None for a direct child),
    .depth (1 = direct), .n_desc (children below it in the list)."""
    __slots__ = ("path", "type", "start", "end", "raw", "parent", "depth", "n_desc")

    def __init__(self, rec, msg: bytes):
        kind, key, ks = int(rec["kind"]), int(rec["key"]), int(rec["key_start"])
        if kind == PS_FIELD:
            self.path = PathFieldId(key)
        elif kind == PS_INDEX:
            self.path = PathIndex(key)
        elif kind == PS_INTKEY:
            self.path = PathIntKey(key)
        elif kind == PS_STRKEY:
            self.path = PathStrKey(msg[ks + 4:ks + 4 + key])
        else:
            self.path = PathBinKey(msg[ks:ks + key])
        self.type, self.start, self.end = int(rec["type"]), int(rec["start"]), int(rec["end"])
        self.raw = msg[self.start:self.end]
        self.parent = None if int(rec["parent"]) == KIDS_NO_PARENT else int(rec["parent"])
        self.depth, self.n_desc = int(rec["depth"]), int(rec["n_desc"])

    def __repr__(self):
        return "Child(%r, type=%d, span=[%d,%d), depth=%d)" % (self.path, self.type, self.start, self.end, self.depth)


class ChildrenResult:
    """One message: .status (OK / NOT_FOUND / E_READ / E_TYPE /
    KIDS_E_UNSUPPORTED), .error (None, "ErrNotFound", "ErrRead",
    "ErrDismatchType", "ErrUnsupportedType"), the node's .type / .key_type /
    .elem_type, .direct (its own children: Node.Len of a list, set or map; the
    failing step when the status is not OK), .start, .children (a list of
    Child in wire order, preorder in recursive mode; empty unless OK)."""
    __slots__ = ("status", "error", "type", "key_type", "elem_type", "direct", "start", "children")

    def __init__(self, head, recs, msg: bytes):
        self.status = int(head["status"])
        self.error = KIDS_ERROR_NAMES.get(self.status, "ErrRead")
        self.type, self.key_type, self.elem_type = int(head["type"]), int(head["key_type"]), int(head["elem_type"])
        self.direct, self.start = int(head["direct"]), int(head["start"])
        self.children = [Child(r, msg) for r in recs]

    def __repr__(self):
        return "ChildrenResult(status=%d, type=%d, %d children)" % (self.status, self.type, len(self.children))


def _one_path(path, desc, ctx):
    return path if isinstance(path, PathSet) else PathSet([list(path)], desc, ctx)


def children_records(msgs: Sequence[bytes], path=(), recurse: bool = False, desc=None, root_type: int = STRUCT,
                     ctx: Optional[Context] = None, count_only: bool = False):
    """(head, rec_off, recs) of dg_kids_batch_host: KIDS_HEAD_DTYPE[n],
    uint64[n + 1] and KIDS_REC_DTYPE[rec_off[n]]; message i's records are
    recs[rec_off[i]:rec_off[i + 1]]. count_only stops after the count (recs is
    empty): head["direct"] is batched Node.Len."""
    ps = _one_path(path, desc, ctx)
    with _unless_given(ps, path):
        n = len(msgs)
        L = _lib.lib()
        head = np.zeros(n, dtype=KIDS_HEAD_DTYPE)
        rec_off = np.zeros(n + 1, dtype=np.uint64)
        flags = KIDS_F_RECURSE if recurse else 0
        need = C.c_uint64(0)
        if n == 0:
            _lib.check(L.dg_kids_batch_host(ps.ctx.h, ps.h, root_type, flags, None, None, 0, None, rec_off.ctypes.data, None,
                                            0, C.byref(need)))
            return head, rec_off, np.zeros(0, dtype=KIDS_REC_DTYPE)
        arena, in_off = _arena(msgs)

        def call(cap):
            recs = np.zeros(cap, dtype=KIDS_REC_DTYPE)
            return L.dg_kids_batch_host(ps.ctx.h, ps.h, root_type, flags, arena.ctypes.data, in_off.ctypes.data, n,
                                        head.ctypes.data, rec_off.ctypes.data, recs.ctypes.data if cap else None, cap,
                                        C.byref(need)), recs

        # a guess the call corrects; no records and no room: the call only counts
        recs = _until_fits(call, 0 if count_only else int(in_off[n]) // 8 + 64, need)
        return head, rec_off, recs[:0 if count_only else int(rec_off[n])]


def children_batch(msgs: Sequence[bytes], path=(), recurse: bool = False, desc=None, root_type: int = STRUCT,
                   ctx: Optional[Context] = None) -> List[ChildrenResult]:
    """Node.Children for every message of a batch: the children of the node at
    the end of `path` (a list of Path steps, () for the message's root, or a
    PathSet of one path), or with recurse the whole subtree below it in
    preorder. PathFieldName steps are resolved through `desc`."""
    head, rec_off, recs = children_records(msgs, path, recurse, desc, root_type, ctx)
    return [ChildrenResult(head[i], recs[int(rec_off[i]):int(rec_off[i + 1])], msgs[i]) for i in range(len(msgs))]


def children_device(pathset: PathSet, thrift, in_off, n: int, head, rec_off, recs, rec_cap: int, recurse: bool = False,
                    counted: bool = False, root_type: int = STRUCT, stream=None, max_len: int = 0):
    """Device-resident batch (dg_kids_batch_device) over torch tensors or raw
    device pointers: thrift uint8[>= in_off[n] + 16]; in_off int64[n + 1]; head
    n 16-byte heads (e.g. an int32 tensor of shape (n, 4)); rec_off int64[n +
    1]; recs rec_cap 32-byte records (e.g. int32 of shape (rec_cap, 8)) or None
    to stop after the count; counted: head / rec_off come from an earlier call
    with the same batch, path and mode. Asynchronous on `stream` (a torch
    stream, a raw stream handle, or None for torch's current stream when
    `thrift` is a tensor)."""
    s = _stream_handle(stream, thrift)
    flags = (KIDS_F_RECURSE if recurse else 0) | (KIDS_F_COUNTED if counted else 0)
    _lib.check(_lib.lib().dg_kids_batch_device(pathset.ctx.h, pathset.h, root_type, flags, _ptr(thrift), _ptr(in_off), n,
                                               _ptr(head), _ptr(rec_off), _ptr(recs), rec_cap, s, max_len))


# ---------------------------------------------------------------------------
# Typed column reads: GetByPath followed by Node.Bool / Byte / Int / Float64 /
# String / Len / List for every message of a batch
# (thrift/generic/cast.go:50-224; dg_cols_* in dgj2t.h)
# ---------------------------------------------------------------------------
COL_BOOL, COL_BYTE, COL_INT, COL_F64, COL_STR, COL_LEN, COL_LIST = 1, 2, 3, 4, 5, 6, 16  # DG_COL_*
COL_LIST_INT, COL_LIST_F64 = COL_LIST | COL_INT, COL_LIST | COL_F64
COL_E_UNSUPPORTED = 4  # DG_COL_E_UNSUPPORTED
COL_ERROR_NAMES = dict(ERROR_NAMES)
COL_ERROR_NAMES[COL_E_UNSUPPORTED] = "ErrUnsupportedType"
COL_CELL_DTYPE = np.dtype([("status", "u1"), ("type", "u1"), ("step", "<u2"), ("aux", "<u4")])  # dg_col_cell
_COL_KINDS = {"bool": COL_BOOL, "byte": COL_BYTE, "int": COL_INT, "float64": COL_F64, "str": COL_STR, "len": COL_LEN,
              "list[int]": COL_LIST_INT, "list[float64]": COL_LIST_F64}


def col_kind(kind) -> int:
    """A kind as DG_COL_* or by name: bool, byte, int, float64, str, len, list[int], list[float64]."""
    k = _COL_KINDS.get(kind, kind)
    if k not in _COL_KINDS.values():
        raise ValueError("unknown column kind %r" % (kind,))
    return int(k)


class ColumnPlan(_KindPlan):
    """1 to 8 columns, each a path (a list of Path steps; PathFieldName is
    resolved through `desc`) and a kind (col_kind), on one context's device
    (dg_cols). `columns` is a list of (path, kind)."""
    _destroy, _create, _count, _kind = "dg_cols_destroy", "dg_cols_create", "dg_cols_count", staticmethod(col_kind)

    def __init__(self, columns, desc=None, ctx: Optional[Context] = None):
        super().__init__(columns, desc, ctx)
        self.lists = [k for k, kind in enumerate(self.kinds) if kind & COL_LIST]


def columns_device(plan: ColumnPlan, thrift, in_off, n: int, val, cell, lens=None, root_type: int = STRUCT,
                   stream=None, max_len: int = 0):
    """The cell pass (dg_cols_batch_device) over torch tensors or raw device
    pointers: thrift uint8[>= in_off[n] + 16]; in_off int64[n + 1]; val
    int64[P, n] (a float64 column: val[k].view(torch.float64)); cell P * n
    8-byte cells (e.g. int32 of shape (P, n, 2)); lens int32[P, n], None when
    no column is str or a list. Column-major: a column is one contiguous
    tensor. Asynchronous on `stream` (a torch stream, a raw stream handle, or
    None for torch's current stream when `thrift` is a tensor)."""
    s = _stream_handle(stream, thrift)
    _lib.check(_lib.lib().dg_cols_batch_device(plan.ctx.h, plan.h, root_type, _ptr(thrift), _ptr(in_off), n, _ptr(val),
                                               _ptr(cell), _ptr(lens), s, max_len))


def column_list_device(plan: ColumnPlan, k: int, thrift, n: int, val_k, cell_k, len_k, elem_off, elems, elem_cap: int,
                       stream=None):
    """List column k's elements (dg_cols_list_device) behind columns_device on
    the same stream: val_k / cell_k / len_k are column k's rows of its
    outputs; elem_off int64[n + 1] receives the scanned counts ([n] = the
    total); elems int64[elem_cap] (a float64 list: .view(torch.float64)) the
    elements, or None to stop after the scan."""
    s = _stream_handle(stream, thrift)
    _lib.check(_lib.lib().dg_cols_list_device(plan.ctx.h, plan.h, k, _ptr(thrift), n, _ptr(val_k), _ptr(cell_k),
                                              _ptr(len_k), _ptr(elem_off), _ptr(elems), elem_cap, s))


class Column:
    """One column of columns_batch: .kind; .status (uint8[n]: OK, NOT_FOUND,
    E_READ, E_TYPE or COL_E_UNSUPPORTED), .valid (status == OK), .type,
    .step, .aux (the cell's other fields), .error(i) (None, "ErrNotFound",
    "ErrRead", "ErrDismatchType" or "ErrUnsupportedType"). .values by kind:
    bool -> bool[n], byte -> uint8[n], int and len -> int64[n], float64 ->
    float64[n] (0 where not valid); str -> a list of n bytes (b"" where not
    valid), with .offsets / .lengths into the arena the messages form back to
    back; list[int] / list[float64] -> all elements as int64 / float64, row
    i's at .values[.offsets[i]:.offsets[i + 1]]."""
    __slots__ = ("kind", "status", "valid", "type", "step", "aux", "values", "offsets", "lengths")

    def error(self, i: int):
        return COL_ERROR_NAMES.get(int(self.status[i]), "ErrRead")

    def __repr__(self):
        return "Column(kind=%d, %d cells, %d valid)" % (self.kind, len(self.status), int(self.valid.sum()))


def columns_records(msgs: Sequence[bytes], plan: ColumnPlan, root_type: int = STRUCT):
    """The raw outputs of dg_cols_batch_host: (val uint64[P, n], cell
    COL_CELL_DTYPE[P, n], lens uint32[P, n], elem_off uint64[L, n + 1], elems
    uint64[all elements], arena), L = len(plan.lists); STR and list values are
    offsets into `arena`, the messages back to back."""
    n, P, L = len(msgs), plan.count, len(plan.lists)
    lib = _lib.lib()
    val = np.zeros((P, n), dtype=np.uint64)
    cell = np.zeros((P, n), dtype=COL_CELL_DTYPE)
    lens = np.zeros((P, n), dtype=np.uint32)
    elem_off = np.zeros((max(L, 1), n + 1), dtype=np.uint64)
    need = C.c_uint64(0)
    if n == 0:
        _lib.check(lib.dg_cols_batch_host(plan.ctx.h, plan.h, root_type, None, None, 0, None, None, None,
                                          elem_off.ctypes.data, None, 0, C.byref(need)))
        return val, cell, lens, elem_off[:L], np.zeros(0, dtype=np.uint64), np.zeros(16, dtype=np.uint8)
    arena, in_off = _arena(msgs)

    def call(cap):
        out = np.zeros(cap, dtype=np.uint64)
        return lib.dg_cols_batch_host(plan.ctx.h, plan.h, root_type, arena.ctypes.data, in_off.ctypes.data, n,
                                      val.ctypes.data, cell.ctypes.data, lens.ctypes.data, elem_off.ctypes.data,
                                      out.ctypes.data if cap else None, cap, C.byref(need)), out

    # a guess the call corrects (an element takes at least one byte of its message, four as a rule)
    elems = _until_fits(call, int(in_off[n]) // 4 + 64 if L else 0, need)
    return val, cell, lens, elem_off[:L], elems[:int(need.value)], arena


def columns_batch(msgs: Sequence[bytes], columns, desc=None, root_type: int = STRUCT,
                  ctx: Optional[Context] = None) -> List[Column]:
    """GetByPath and a cast for every message of a batch (dg_cols_batch_host):
    `columns` is a list of (path, kind) or a ColumnPlan; one Column comes back
    per path."""
    plan = columns if isinstance(columns, ColumnPlan) else ColumnPlan(columns, desc, ctx)
    with _unless_given(plan, columns):
        n = len(msgs)
        val, cell, lens, elem_off, elems, arena = columns_records(msgs, plan, root_type)
        out = []
        for k, kind in enumerate(plan.kinds):
            c = Column()
            c.kind, c.status, c.type, c.step, c.aux = kind, cell[k]["status"], cell[k]["type"], cell[k]["step"], cell[k]["aux"]
            c.valid = c.status == OK
            c.offsets = c.lengths = None
            if kind & COL_LIST:
                eo = elem_off[plan.lists.index(k)]
                seg = elems[int(eo[0]):int(eo[n])]
                c.values = seg.view(np.float64) if kind == COL_LIST_F64 else seg.view(np.int64)
                c.offsets, c.lengths = (eo - eo[0]).astype(np.int64), lens[k]
            elif kind == COL_STR:
                c.offsets, c.lengths = val[k].astype(np.int64), lens[k]
                c.values = [arena[int(o):int(o) + int(ln)].tobytes() if ok else b""
                            for o, ln, ok in zip(c.offsets, c.lengths, c.valid)]
            elif kind == COL_BOOL:
                c.values = val[k] != 0
            elif kind == COL_BYTE:
                c.values = val[k].astype(np.uint8)
            elif kind == COL_F64:
                c.values = val[k].view(np.float64)
            else:
                c.values = val[k].view(np.int64)
            out.append(c)
        return out


# ---------------------------------------------------------------------------
# Row columns: the fields of every element of a list or set as ragged columns:
# GetByPath(parent), Children one level, then GetByPath(sub) and a cast per
# element (dg_rows_* in dgj2t.h)
# ---------------------------------------------------------------------------
ROWS_MAX_COLS = 8  # DG_ROWS_MAX_COLS
ROWS_HEAD_DTYPE = np.dtype([("first", "<u8"), ("count", "<u4"), ("status", "u1"), ("type", "u1"), ("elem_type", "u1"),
                            ("step", "u1")])  # dg_rows_head
ROW_ENT_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("msg", "<u4")])  # dg_row_ent
ROWS_KEY_STR, ROWS_KEY_INT = 1, 2  # DG_ROWS_KEY_*
_ROWS_KEYS = {None: 0, "str": ROWS_KEY_STR, "int": ROWS_KEY_INT}


class RowPlan(_Handle):
    """One parent path (a list of Path steps, () for the message's root) and 1
    to 8 row columns, each (sub_path, kind): the sub-path is looked up in every
    element of the list or set the parent path ends at, the kind is col_kind's.
    PathFieldName steps of the parent are resolved through `desc`, those of a
    sub-path through the descriptor of the list's elements; a name step
    without a descriptor raises (dg_rows). keys = "str" or "int" makes a map
    plan: the parent path ends at a map<string, V> or a map of integer keys,
    a row is an entry, the sub-paths are looked up in its value (names
    through the descriptor of the map's values) and every row has its key."""
    _destroy = "dg_rows_destroy"

    def __init__(self, parent, columns, desc=None, ctx: Optional[Context] = None, keys=None):
        if keys not in _ROWS_KEYS:
            raise ValueError("unknown key kind %r (\"str\", \"int\" or None)" % (keys,))
        self.ctx = ctx or default_context()
        self.keys, self.key_kind = keys, _ROWS_KEYS[keys]
        self.kinds = [col_kind(k) for _, k in columns]
        steps, at = _resolve_to(list(parent), desc)
        self.parent_blob = compile_paths([steps])
        self.blob = compile_paths([list(p) for p, _ in columns], at.elem if at is not None else None)
        h = C.c_void_p()
        args = (self.ctx.h, self.parent_blob, len(self.parent_blob), self.blob, len(self.blob), bytes(self.kinds),
                len(self.kinds))
        if self.key_kind:
            _lib.check(_lib.lib().dg_rows_create_map(*args, self.key_kind, C.byref(h)))
        else:
            _lib.check(_lib.lib().dg_rows_create(*args, C.byref(h)))
        self.h = h
        self.count = int(_lib.lib().dg_rows_count(h))
        self.lists = [k for k, kind in enumerate(self.kinds) if kind & COL_LIST]


def rows_device(plan: RowPlan, thrift, in_off, n: int, head, row_off, index=None, val=None, cell=None, lens=None,
                row_cap: int = 0, root_type: int = STRUCT, stream=None, max_len: int = 0, keys=None, key_lens=None):
    """Device-resident batch (dg_rows_batch_device) over torch tensors or raw
    device pointers: thrift uint8[>= in_off[n] + 16]; in_off int64[n + 1]; head
    n 16-byte heads (e.g. int32 of shape (n, 4)); row_off int64[n + 1]
    ([n] = the total R); index row_cap 16-byte entries or None (the plan's
    context keeps it); val int64[P, row_cap], cell P * row_cap 8-byte cells
    (e.g. int32 of shape (P, row_cap, 2)), lens int32[P, row_cap] (None when no
    column is str or a list). val and cell None: the sizing call (heads and
    row_off; with index given, the index too). No row at an
    index >= row_cap is stored. Asynchronous on `stream` (a torch stream, a raw
    stream handle, or None for torch's current stream when `thrift` is a
    tensor). A map plan goes to dg_rows_map_batch_device: keys int64[row_cap]
    and key_lens int32[row_cap] (each may be None) receive every indexed row's
    key: an int key's value and width, a string key's arena offset and length."""
    s = _stream_handle(stream, thrift)
    if plan.key_kind:
        _lib.check(_lib.lib().dg_rows_map_batch_device(plan.ctx.h, plan.h, root_type, _ptr(thrift), _ptr(in_off), n,
                                                       _ptr(head), _ptr(row_off), _ptr(index), _ptr(keys), _ptr(key_lens),
                                                       _ptr(val), _ptr(cell), _ptr(lens), row_cap, s, max_len))
        return
    if keys is not None or key_lens is not None:
        raise ValueError("keys for a list plan")
    _lib.check(_lib.lib().dg_rows_batch_device(plan.ctx.h, plan.h, root_type, _ptr(thrift), _ptr(in_off), n, _ptr(head),
                                               _ptr(row_off), _ptr(index), _ptr(val), _ptr(cell), _ptr(lens), row_cap, s,
                                               max_len))


def row_list_device(plan: RowPlan, k: int, thrift, n_rows: int, val_k, cell_k, len_k, elem_off, elems, elem_cap: int,
                    stream=None):
    """List-kind row column k's elements (dg_rows_list_device) behind
    rows_device on the same stream: val_k / cell_k / len_k are column k's rows
    of its outputs, n_rows the rows whose cells were written; elem_off
    int64[n_rows + 1] receives the scanned counts, elems int64[elem_cap] the
    elements, or None to stop after the scan."""
    s = _stream_handle(stream, thrift)
    _lib.check(_lib.lib().dg_rows_list_device(plan.ctx.h, plan.h, k, _ptr(thrift), n_rows, _ptr(val_k), _ptr(cell_k),
                                              _ptr(len_k), _ptr(elem_off), _ptr(elems), elem_cap, s))


def rows_records(msgs: Sequence[bytes], plan: RowPlan, root_type: int = STRUCT, count_only: bool = False):
    """The raw outputs of dg_rows_batch_host: (head ROWS_HEAD_DTYPE[n], row_off
    uint64[n + 1], index ROW_ENT_DTYPE[R], val uint64[P, R], cell
    COL_CELL_DTYPE[P, R], lens uint32[P, R], arena); offsets point into `arena`,
    the messages back to back. count_only stops after the heads (R = 0 rows
    come back): head["count"] is batched Node.Len. A map plan goes through
    dg_rows_map_batch_host and gets two more items behind the seven: key
    uint64[R] and key_len uint32[R]."""
    n, P = len(msgs), plan.count
    lib = _lib.lib()
    if plan.key_kind:
        def host(thrift, in_off, n, head, row_off, index, val, cell, lens, cap, need, key=None, key_len=None):
            return lib.dg_rows_map_batch_host(plan.ctx.h, plan.h, root_type, thrift, in_off, n, head, row_off, index, key,
                                              key_len, val, cell, lens, cap, need)
    else:
        def host(thrift, in_off, n, head, row_off, index, val, cell, lens, cap, need):
            return lib.dg_rows_batch_host(plan.ctx.h, plan.h, root_type, thrift, in_off, n, head, row_off, index, val, cell,
                                          lens, cap, need)
    head = np.zeros(n, dtype=ROWS_HEAD_DTYPE)
    row_off = np.zeros(n + 1, dtype=np.uint64)
    need = C.c_uint64(0)

    def outs(R):
        return (np.zeros(R, dtype=ROW_ENT_DTYPE), np.zeros((P, R), dtype=np.uint64), np.zeros((P, R), dtype=COL_CELL_DTYPE),
                np.zeros((P, R), dtype=np.uint32))

    def keys(R):
        return (np.zeros(R, dtype=np.uint64), np.zeros(R, dtype=np.uint32)) if plan.key_kind else ()

    if n == 0:
        _lib.check(host(None, None, 0, None, row_off.ctypes.data, None, None, None, None, 0, C.byref(need)))
        return (head, row_off) + outs(0) + (np.zeros(16, dtype=np.uint8),) + keys(0)
    arena, in_off = _arena(msgs)
    _lib.check(host(arena.ctypes.data, in_off.ctypes.data, n, head.ctypes.data, row_off.ctypes.data, None, None, None, None, 0,
                    C.byref(need)))
    R = 0 if count_only else int(need.value)
    index, val, cell, lens = outs(R)
    kv = keys(R)
    if R:
        _lib.check(host(arena.ctypes.data, in_off.ctypes.data, n, head.ctypes.data, row_off.ctypes.data, index.ctypes.data,
                        val.ctypes.data, cell.ctypes.data, lens.ctypes.data, R, C.byref(need),
                        *(a.ctypes.data for a in kv)))
    return (head, row_off, index, val, cell, lens, arena) + kv


def _row_list_elems(plan: RowPlan, k: int, arena, val_k, cell_k, len_k):
    """(elem_off int64[R + 1], elems uint64) of list-kind row column k: the host
    arrays of rows_records through dg_rows_list_device."""
    import torch
    R = len(val_k)
    dev = torch.device("cuda", plan.ctx.device)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream()
        d_arena = torch.from_numpy(np.array(arena)).to(dev)
        d_val = torch.from_numpy(val_k.view(np.int64).copy()).to(dev)
        d_cell = torch.from_numpy(cell_k.copy().view(np.int64)).to(dev)
        d_len = torch.from_numpy(len_k.view(np.int32).copy()).to(dev)
        total = int(len_k.astype(np.uint64).sum())
        d_off = torch.zeros(R + 1, dtype=torch.int64, device=dev)
        d_el = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
        row_list_device(plan, k, d_arena, R, d_val, d_cell, d_len, d_off, d_el if total else None, total, stream=s)
        s.synchronize()
        return d_off.cpu().numpy(), d_el.cpu().numpy()[:total].view(np.uint64)


class Rows:
    """What rows_batch returns: .head (ROWS_HEAD_DTYPE[n]: status, step, type,
    elem_type, count, first), .status (uint8[n]), .error(i) (None,
    "ErrNotFound", "ErrRead", "ErrDismatchType" or "ErrUnsupportedType"),
    .offsets (int64[n + 1]: message i owns rows offsets[i]:offsets[i + 1]),
    .index (ROW_ENT_DTYPE[R]: every row's element span in the arena and its
    message) and .columns, one Column per row column over the R rows (a list
    kind's .offsets index its elements by row). Under a map plan a row is an
    entry of the map, .index its value's span, and .keys holds the rows' keys:
    int64[R] for int keys, a list of R bytes for string keys, with
    .key_lengths (uint32[R]) the string keys' lengths or the int keys' widths
    in bytes; both are None under a list plan."""
    __slots__ = ("head", "status", "offsets", "index", "columns", "keys", "key_lengths")

    def error(self, i: int):
        return COL_ERROR_NAMES.get(int(self.status[i]), "ErrRead")

    def __repr__(self):
        return "Rows(%d messages, %d rows, %d columns)" % (len(self.status), len(self.index), len(self.columns))


def rows_batch(msgs: Sequence[bytes], parent, columns=None, desc=None, root_type: int = STRUCT,
               ctx: Optional[Context] = None, keys=None) -> Rows:
    """For every message the list or set at `parent` and, for every element of
    it, GetByPath(sub_path) and a cast: `columns` is a list of (sub_path, kind);
    `parent` may be a RowPlan instead (then `columns` is not given). keys =
    "str" or "int": `parent` ends at a map, the rows are its entries."""
    plan = parent if isinstance(parent, RowPlan) else RowPlan(parent, columns, desc, ctx, keys)
    with _unless_given(plan, parent):
        head, row_off, index, val, cell, lens, arena, *kv = rows_records(msgs, plan, root_type)
        out = Rows()
        out.head, out.status, out.offsets, out.index = head, head["status"], row_off.astype(np.int64), index
        out.keys = out.key_lengths = None
        if plan.key_kind:
            out.key_lengths = kv[1]
            out.keys = kv[0].view(np.int64) if plan.key_kind == ROWS_KEY_INT else \
                [arena[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(kv[0], kv[1])]
        out.columns = []
        for k, kind in enumerate(plan.kinds):
            c = Column()
            c.kind, c.status, c.type, c.step, c.aux = kind, cell[k]["status"], cell[k]["type"], cell[k]["step"], cell[k]["aux"]
            c.valid = c.status == OK
            c.offsets = c.lengths = None
            if kind & COL_LIST:
                eo, elems = _row_list_elems(plan, k, arena, val[k], cell[k], lens[k]) if len(index) else \
                    (np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.uint64))
                c.values = elems.view(np.float64) if kind == COL_LIST_F64 else elems.view(np.int64)
                c.offsets, c.lengths = eo, lens[k]
            elif kind == COL_STR:
                c.offsets, c.lengths = val[k].astype(np.int64), lens[k]
                c.values = [arena[int(o):int(o) + int(ln)].tobytes() if ok else b""
                            for o, ln, ok in zip(c.offsets, c.lengths, c.valid)]
            elif kind == COL_BOOL:
                c.values = val[k] != 0
            elif kind == COL_BYTE:
                c.values = val[k].astype(np.uint8)
            elif kind == COL_F64:
                c.values = val[k].view(np.float64)
            else:
                c.values = val[k].view(np.int64)
            out.columns.append(c)
        return out


# ---------------------------------------------------------------------------
# Entry columns: GetByPath followed by Node.List with String per element,
# Node.StrMap or Node.IntMap for every message of a batch, as ragged columns
# (thrift/generic/cast.go:198-286; dg_ents_* in dgj2t.h)
# ---------------------------------------------------------------------------
ENT_BOOL, ENT_INT, ENT_F64, ENT_STR = 1, 3, 4, 5  # DG_ENT_*: the value kinds
ENT_LISTSTR, ENT_STRMAP, ENT_INTMAP = 0x15, 0x20, 0x40
_ENT_VALS = {"bool": ENT_BOOL, "int": ENT_INT, "float64": ENT_F64, "f64": ENT_F64, "str": ENT_STR}
_ENT_KINDS = {"list[str]": ENT_LISTSTR}
_ENT_KINDS.update({"%s[%s]" % (m, v): c | k for m, c in (("strmap", ENT_STRMAP), ("intmap", ENT_INTMAP))
                   for v, k in _ENT_VALS.items()})


def ent_kind(kind) -> int:
    """A kind as DG_ENT_* or by name: list[str], strmap[v] and intmap[v] with v one of bool, int, float64 (f64), str."""
    k = _ENT_KINDS.get(kind, kind)
    if k not in _ENT_KINDS.values():
        raise ValueError("unknown entry kind %r" % (kind,))
    return int(k)


class EntryPlan(_KindPlan):
    """1 to 8 entry columns, each a path (a list of Path steps; PathFieldName
    is resolved through `desc`) and a kind (ent_kind), on one context's device
    (dg_ents). `columns` is a list of (path, kind)."""
    _destroy, _create, _count, _kind = "dg_ents_destroy", "dg_ents_create", "dg_ents_count", staticmethod(ent_kind)


def entries_device(plan: EntryPlan, thrift, in_off, n: int, val, cell, lens, spans, root_type: int = STRUCT,
                   stream=None, max_len: int = 0):
    """The cell pass (dg_ents_batch_device) over torch tensors or raw device
    pointers: thrift uint8[>= in_off[n] + 16]; in_off int64[n + 1]; val
    int64[P, n]; cell P * n 8-byte cells (e.g. int32 of shape (P, n, 2)); lens
    and spans int32[P, n]. Column-major: a column is one contiguous tensor.
    Asynchronous on `stream` (a torch stream, a raw stream handle, or None for
    torch's current stream when `thrift` is a tensor)."""
    s = _stream_handle(stream, thrift)
    _lib.check(_lib.lib().dg_ents_batch_device(plan.ctx.h, plan.h, root_type, _ptr(thrift), _ptr(in_off), n, _ptr(val),
                                               _ptr(cell), _ptr(lens), _ptr(spans), s, max_len))


def entry_emit_device(plan: EntryPlan, k: int, thrift, n: int, val_k, cell_k, len_k, span_k, ent_off, keys=None,
                      key_lens=None, vals=None, val_lens=None, ent_cap: int = 0, stream=None):
    """Column k's entries (dg_ents_emit_device) behind entries_device on the
    same stream: val_k / cell_k / len_k / span_k are column k's rows of its
    outputs; ent_off int64[n + 1] receives the scanned counts ([n] = the
    total); keys and vals int64[ent_cap] (float64 values:
    .view(torch.float64)), key_lens and val_lens int32[ent_cap]; any of the
    four may be None, all four None stops after the scan."""
    s = _stream_handle(stream, thrift)
    _lib.check(_lib.lib().dg_ents_emit_device(plan.ctx.h, plan.h, k, _ptr(thrift), n, _ptr(val_k), _ptr(cell_k),
                                              _ptr(len_k), _ptr(span_k), _ptr(ent_off), _ptr(keys), _ptr(key_lens),
                                              _ptr(vals), _ptr(val_lens), ent_cap, s))


class EntryColumn:
    """One column of entries_batch: .kind; .status (uint8[n]: OK, NOT_FOUND,
    E_READ, E_TYPE or COL_E_UNSUPPORTED), .valid, .type, .step, .aux (the
    cell's other fields; a map cell's aux: key type | value type << 8),
    .error(i), .offsets (int64[n + 1]: message i's entries are
    [offsets[i], offsets[i + 1])) and .lengths (the counts). .keys[i] and
    .values[i] are message i's keys and values in wire order, duplicates kept:
    ints, bools, floats or bytes by kind; .keys is None for list[str].
    .items(i) pairs them."""
    __slots__ = ("kind", "status", "valid", "type", "step", "aux", "offsets", "lengths", "keys", "values")

    def error(self, i: int):
        return COL_ERROR_NAMES.get(int(self.status[i]), "ErrRead")

    def items(self, i: int):
        return list(zip(self.keys[i], self.values[i])) if self.keys is not None else list(self.values[i])

    def __repr__(self):
        return "EntryColumn(kind=%#x, %d cells, %d valid)" % (self.kind, len(self.status), int(self.valid.sum()))


def entries_records(msgs: Sequence[bytes], plan: EntryPlan, root_type: int = STRUCT):
    """The raw outputs of dg_ents_batch_host: (val uint64[P, n], cell
    COL_CELL_DTYPE[P, n], lens uint32[P, n], ent_off uint64[P, n + 1], keys
    uint64[all], key_lens uint32[all], vals uint64[all], val_lens uint32[all],
    arena); string keys, values and elements are offsets into `arena`, the
    messages back to back."""
    n, P = len(msgs), plan.count
    lib = _lib.lib()
    val = np.zeros((P, n), dtype=np.uint64)
    cell = np.zeros((P, n), dtype=COL_CELL_DTYPE)
    lens = np.zeros((P, n), dtype=np.uint32)
    ent_off = np.zeros((P, n + 1), dtype=np.uint64)
    need = C.c_uint64(0)
    if n == 0:
        _lib.check(lib.dg_ents_batch_host(plan.ctx.h, plan.h, root_type, None, None, 0, None, None, None,
                                          ent_off.ctypes.data, None, None, None, None, 0, C.byref(need)))
        z8, z4 = np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint32)
        return val, cell, lens, ent_off, z8, z4, z8.copy(), z4.copy(), np.zeros(16, dtype=np.uint8)
    arena, in_off = _arena(msgs)

    def call(cap):
        out = (np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint64),
               np.zeros(cap, dtype=np.uint32))
        return lib.dg_ents_batch_host(plan.ctx.h, plan.h, root_type, arena.ctypes.data, in_off.ctypes.data, n,
                                      val.ctypes.data, cell.ctypes.data, lens.ctypes.data, ent_off.ctypes.data,
                                      *(o.ctypes.data if cap else None for o in out), cap, C.byref(need)), out

    # a guess the call corrects (an entry takes at least two bytes of its message, five as a rule)
    out = _until_fits(call, int(in_off[n]) // 4 + 64, need)
    return (val, cell, lens, ent_off) + tuple(o[:int(need.value)] for o in out) + (arena,)


def entries_batch(msgs: Sequence[bytes], columns, desc=None, root_type: int = STRUCT,
                  ctx: Optional[Context] = None) -> List[EntryColumn]:
    """GetByPath and Node.List / StrMap / IntMap for every message of a batch
    (dg_ents_batch_host): `columns` is a list of (path, kind) or an EntryPlan;
    one EntryColumn comes back per path."""
    plan = columns if isinstance(columns, EntryPlan) else EntryPlan(columns, desc, ctx)
    with _unless_given(plan, columns):
        n = len(msgs)
        val, cell, lens, ent_off, keys, klens, vals, vlens, arena = entries_records(msgs, plan, root_type)
        raw = arena.tobytes()

        def decode(v, ls, is_str, vk):
            if is_str:
                return [raw[o:o + ln] for o, ln in zip(v.tolist(), ls.tolist())]
            if vk == ENT_F64:
                return v.view(np.float64).tolist()
            if vk == ENT_BOOL:
                return (v != 0).tolist()
            return v.view(np.int64).tolist()

        out = []
        for k, kind in enumerate(plan.kinds):
            c = EntryColumn()
            c.kind, c.status, c.type, c.step, c.aux = kind, cell[k]["status"], cell[k]["type"], cell[k]["step"], cell[k]["aux"]
            c.valid = c.status == OK
            eo = ent_off[k].astype(np.int64)
            a, b = int(eo[0]), int(eo[n])
            c.offsets, c.lengths = eo - eo[0], lens[k]
            cuts = c.offsets.tolist()
            vs = decode(vals[a:b], vlens[a:b], kind == ENT_LISTSTR or kind & 15 == ENT_STR, kind & 15)
            c.values = [vs[x:y] for x, y in zip(cuts, cuts[1:])]
            c.keys = None
            if kind != ENT_LISTSTR:
                ks = decode(keys[a:b], klens[a:b], bool(kind & ENT_STRMAP), ENT_INT)
                c.keys = [ks[x:y] for x, y in zip(cuts, cuts[1:])]
            out.append(c)
        return out


# ---------------------------------------------------------------------------
# Typed column writes, the inverse of the reads above: tensors encoded to
# Thrift-binary values (NewNodeBool ... NewNodeString / NewNodeList /
# NewNodeSet) or whole struct messages (NewNodeStruct)
# (thrift/generic/node.go:92-201; dg_vals_* in dgj2t.h)
# ---------------------------------------------------------------------------
VAL_BOOL, VAL_I08, VAL_F64, VAL_I16, VAL_I32, VAL_I64, VAL_STR = 2, 3, 4, 6, 8, 10, 11  # the wire types
VAL_LIST, VAL_SET = 0x40, 0x80  # DG_VAL_LIST, DG_VAL_SET
VAL_OK, VAL_E_SIZE = 0, 1  # DG_VAL_*
VALS_MAX_COLS = 16  # DG_VALS_MAX_COLS
_VAL_KINDS = {"bool": VAL_BOOL, "byte": VAL_I08, "i8": VAL_I08, "f64": VAL_F64, "double": VAL_F64, "i16": VAL_I16,
              "i32": VAL_I32, "i64": VAL_I64, "str": VAL_STR, "string": VAL_STR, "binary": VAL_STR}
_VAL_ELEMS = (VAL_BOOL, VAL_I08, VAL_F64, VAL_I16, VAL_I32, VAL_I64)


def val_kind(kind) -> int:
    """A kind as DG_VAL_* or by name: bool, byte / i8, i16, i32, i64, f64 /
    double, str / string / binary, ("list", elem) and ("set", elem) with elem
    any of those but str."""
    if isinstance(kind, (tuple, list)) and len(kind) == 2 and kind[0] in ("list", "set"):
        elem = val_kind(kind[1])
        if elem not in _VAL_ELEMS:
            raise ValueError("unknown value kind %r" % (kind,))
        return (VAL_LIST if kind[0] == "list" else VAL_SET) | elem
    k = _VAL_KINDS.get(kind, kind) if isinstance(kind, str) else kind
    ok = isinstance(k, int) and (k == VAL_STR or k in _VAL_ELEMS or (
        k & (VAL_LIST | VAL_SET) in (VAL_LIST, VAL_SET) and k & 0x3F in _VAL_ELEMS and k < 0x100))
    if not ok:
        raise ValueError("unknown value kind %r" % (kind,))
    return int(k)


class _WritePlan(_Handle):
    """What ValuePlan and EntryValuePlan share: the constructor of a plan of kinds with optional field ids. A class
    names the library's entries (_create, _count, _wire_type, _destroy, and _host, the host batch), the function that
    resolves a kind (_kind), the kinds array's numpy dtype (_kind_dtype) and the column record with its pointer fields."""
    _create = _count = _wire_type = _host = _kind = _kind_dtype = _rec = _fields = None

    def __init__(self, kinds, field_ids=None, ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.kinds = [self._kind(k) for k in kinds]
        self.field_ids = None if field_ids is None else [int(f) for f in field_ids]
        if self.field_ids is not None and len(self.field_ids) != len(self.kinds):
            raise ValueError("%d field ids for %d columns" % (len(self.field_ids), len(self.kinds)))
        ids = None if self.field_ids is None else np.array(self.field_ids, dtype=np.int16)
        lib, h = _lib.lib(), C.c_void_p()
        _lib.check(getattr(lib, self._create)(self.ctx.h, np.array(self.kinds, dtype=self._kind_dtype).tobytes(),
                                              len(self.kinds), None if ids is None else ids.ctypes.data, C.byref(h)))
        self.h = h
        self.count = int(getattr(lib, self._count)(h))
        self.wire_types = [int(getattr(lib, self._wire_type)(h, k)) for k in range(self.count)]

    def _cols(self, cols):
        """_rec[K] from per-column dicts (or tuples in _fields' order) of tensors, arrays or raw pointers and the int n_ent"""
        if len(cols) != self.count:
            raise ValueError("%d columns for a plan of %d" % (len(cols), self.count))
        recs = (self._rec * self.count)()
        for r, c in zip(recs, cols):
            c = c if isinstance(c, dict) else dict(zip(self._fields, c))
            for f in self._fields:
                x = c.get(f)
                setattr(r, f, x.ctypes.data if isinstance(x, np.ndarray) else _ptr(x))
            if hasattr(r, "n_ent"):
                r.n_ent = int(c["n_ent"])
        return recs


class ValuePlan(_WritePlan):
    """1 to 16 columns to write, each a kind (val_kind), on one context's
    device (dg_vals). With `field_ids` (one int16 per column) the plan builds
    struct messages: every item gets its field header and every message its
    STOP; without, the items are bare values, what edit_many_device takes.
    .wire_types: the columns' wire types (edit_many_device's val_types)."""
    _create, _count, _wire_type, _destroy = "dg_vals_create", "dg_vals_count", "dg_vals_wire_type", "dg_vals_destroy"
    _host, _kind, _kind_dtype = "dg_vals_batch_host", staticmethod(val_kind), np.uint8
    _rec, _fields = _lib.ValCol, ("val", "len", "src", "elem_off", "elems", "present")


def _device_call(out, out_off, cap, stream):
    """(the stream's handle, cap) of a *_device write: cap defaults to out's size less 16, 0 without out"""
    if cap is None:
        cap = int(out.numel()) - 16 if hasattr(out, "numel") else 0
    return _stream_handle(stream, out_off), max(cap, 0)


def values_device(plan: ValuePlan, cols, n: int, out, out_off, status=None, out_base: int = 0, cap: Optional[int] = None,
                  stream=None):
    """Device-resident batch (dg_vals_batch_device) over torch tensors or raw
    device pointers. cols: one dict per column with the keys its kind reads,
    in the shapes columns_device / column_list_device write: val int64[n] (a
    scalar's value, a float64 column viewed as int64; str: the payload's
    offset in src), len int32[n] and src uint8 (str; src with 16 spare bytes),
    elem_off int64[n + 1] and elems int64 (lists and sets), present uint8[n]
    (struct mode, optional). out uint8[cap + 16] or None to stop after the
    offsets (sizing); out_off int64[n * K + 1]; status uint8[n * K] or None.
    cap defaults to out's size less 16. What it fills is what
    edit_many_device takes as val / val_off. Asynchronous on `stream`."""
    s, cap = _device_call(out, out_off, cap, stream)
    _lib.check(_lib.lib().dg_vals_batch_device(plan.ctx.h, plan.h, plan._cols(cols), n, out_base, _ptr(out), cap,
                                               _ptr(out_off), _ptr(status), s))


def _pack_strings(rows):
    """str / bytes -> (offsets uint64, lengths uint32, the payloads back to back with 16 spare bytes)"""
    pay = [x.encode() if isinstance(x, str) else bytes(x) for x in rows]
    lens = np.fromiter((len(x) for x in pay), dtype=np.uint64, count=len(pay))
    return (np.cumsum(lens) - lens).astype(np.uint64), lens.astype(np.uint32), \
        np.frombuffer(b"".join(pay) + b"\0" * 16, dtype=np.uint8)


def _present_col(present, n: int) -> np.ndarray:
    p = np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8)
    if len(p) != n:
        raise ValueError("present of %d entries for %d messages" % (len(p), n))
    return p


def _host_column(kind: int, column, n: int, present=None):
    """a column of values_batch as the arrays dg_vals_batch_host reads"""
    if len(column) != n:
        raise ValueError("a column of %d values for %d messages" % (len(column), n))
    c = {}
    if kind & (VAL_LIST | VAL_SET):
        off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum([len(x) for x in column], out=off[1:])
        dt = np.float64 if kind & 0x3F == VAL_F64 else None
        rows = [np.asarray(x, dtype=dt) for x in column if len(x)]
        flat = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        c["elem_off"], c["elems"] = off, _as_u64(flat, kind & 0x3F)
    elif kind == VAL_STR:
        c["val"], c["len"], c["src"] = _pack_strings(column)
    else:
        c["val"] = _as_u64(np.asarray(column, dtype=np.float64 if kind == VAL_F64 else None), kind)
    if present is not None:
        c["present"] = _present_col(present, n)
    return c


def _as_u64(a: np.ndarray, elem: int) -> np.ndarray:
    """the 64-bit inputs: floats as their bits (for a DOUBLE), integers mod 2^64"""
    if a.dtype.kind == "f":
        if elem != VAL_F64:
            raise ValueError("a float array for an integer kind")
        return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    if a.dtype.kind == "b":
        return a.astype(np.uint64)
    if a.dtype.kind == "O":  # Python ints beyond int64
        return np.array([int(x) & (2 ** 64 - 1) for x in a], dtype=np.uint64)
    if a.dtype.kind not in "iu":
        raise ValueError("a column of dtype %s" % a.dtype)
    return np.ascontiguousarray(a.astype(np.int64) if a.dtype.kind == "i" else a.astype(np.uint64)).view(np.uint64)


def _write_host(plan: _WritePlan, cols, n: int):
    """the plan's host entry over host columns: (arena, off, status)"""
    k = plan.count
    off = np.zeros(n * k + 1, dtype=np.uint64)
    status = np.zeros(n * k, dtype=np.uint8)
    need = C.c_uint64(0)
    recs = plan._cols(cols)
    for sized in (False, True):  # the first call sizes: the arena's bytes are known exactly after it
        cap = int(need.value) if sized else 0
        out = np.zeros(cap, dtype=np.uint8)
        _lib.check(getattr(_lib.lib(), plan._host)(plan.ctx.h, plan.h, recs, n, out.ctypes.data if cap else None, cap,
                                                   off.ctypes.data, status.ctypes.data, C.byref(need)))
        if not need.value:
            break
    return out, off, status


_values_host = _entry_values_host = _write_host  # the names the two components' tests call it by


def _write_batch(cls, host_col, columns, plan, ctx):
    """values_batch / entry_values_batch: cls the plan class, host_col its host-column function"""
    wp = plan if isinstance(plan, cls) else cls(plan, None, ctx)
    with _unless_given(wp, plan):
        if len(columns) != wp.count:
            raise ValueError("%d columns for a plan of %d" % (len(columns), wp.count))
        n = len(columns[0])
        return _write_host(wp, [host_col(k, c, n) for k, c in zip(wp.kinds, columns)], n)


def _set_write_columns(cls, host_col, msgs, parent, columns, desc, root_type, ctx):
    """set_columns_batch / set_entry_columns_batch"""
    columns = list(columns)
    if not 1 <= len(columns) <= EDITM_MAX_ITEMS:
        raise ValueError("%d columns (1 to %d)" % (len(columns), EDITM_MAX_ITEMS))
    with cls([c[1] for c in columns], None, ctx) as wp:
        if any(len(c[2]) != len(msgs) for c in columns):
            raise ValueError("a column's length is not the batch's")
        arena, off, _ = _write_batch(cls, host_col, [c[2] for c in columns], wp, None) if msgs else \
            (np.zeros(0, np.uint8), np.zeros(1, np.uint64), None)
        with EditManyPlan(parent, [c[0] for c in columns], EDIT_SET, desc, ctx) as plan:
            return _editm_batch(msgs, plan, None, wp.wire_types, root_type, encoded=(arena, off))


def _build_write_structs(cls, host_col, fields, ctx):
    """build_structs_batch / build_entry_structs_batch"""
    fields = [tuple(f) for f in fields]
    n = len(fields[0][2])
    with cls([f[1] for f in fields], [f[0] for f in fields], ctx) as wp:
        cols = [host_col(k, f[2], n, f[3] if len(f) > 3 else None) for k, f in zip(wp.kinds, fields)]
        arena, off, _ = _write_host(wp, cols, n)
        return _split(arena, off[::wp.count])


def values_batch(columns, plan, ctx: Optional[Context] = None):
    """The host path (dg_vals_batch_host): `plan` is a ValuePlan or a list of
    kinds; per column a numpy integer or float array (a DOUBLE column: floats,
    or integers taken as bits), a sequence of bytes / str (str columns), or a
    sequence of sequences (lists and sets). Integers are taken mod 2^64 and
    written at the kind's width. Returns (arena uint8, off uint64[n * K + 1],
    status uint8[n * K]), message-major: item j of message i is
    arena[off[i * K + j]:off[i * K + j + 1]]."""
    return _write_batch(ValuePlan, _host_column, columns, plan, ctx)


def set_columns_batch(msgs: Sequence[bytes], parent, columns, desc=None, root_type: int = STRUCT,
                      ctx: Optional[Context] = None) -> List[EditManyResult]:
    """SetMany from columns: below the node at `parent`, every (step, kind,
    column) sets the child at `step` of message i to column[i] encoded as
    `kind` (values_batch, then set_many_batch's host entry with the kinds'
    wire types). At most EDITM_MAX_ITEMS columns."""
    return _set_write_columns(ValuePlan, _host_column, msgs, parent, columns, desc, root_type, ctx)


def build_structs_batch(fields, ctx: Optional[Context] = None) -> List[bytes]:
    """NewNodeStruct for a batch: `fields` is a list of (field_id, kind,
    column[, present]); message i holds, in the order given, every field whose
    present[i] is true (all, without present), then STOP."""
    return _build_write_structs(ValuePlan, _host_column, fields, ctx)


# ---------------------------------------------------------------------------
# Entry column writes, the inverse of the entry columns above: ragged tensors
# encoded to list<string>, set<string> and map values (NewNodeList /
# NewNodeSet / NewNodeMap) or to struct messages of such fields
# (thrift/generic/node.go:154-187; dg_evals_* in dgj2t.h)
# ---------------------------------------------------------------------------
EVAL_MAP = 0x100  # DG_EVAL_MAP
EVAL_E_RANGE = 2  # DG_EVAL_E_RANGE
EVALS_MAX_ENT = 0xFFFFFFFF  # DG_EVALS_MAX_ENT
_EVAL_KEYS = (VAL_I08, VAL_I16, VAL_I32, VAL_I64, VAL_STR)
_EVAL_VALS = _VAL_ELEMS + (VAL_STR,)


def eval_kind(kind) -> int:
    """A kind as a number (DG_VAL_LIST | 11, DG_VAL_SET | 11, DG_EVAL_MAP | kt
    << 4 | vt) or by name: ("list", "str"), ("set", "str") (str / string /
    binary) and ("map", key, value) with key one of byte / i8, i16, i32, i64,
    str and value any of val_kind's scalar names or str."""
    k = kind
    if isinstance(kind, (tuple, list)):
        try:
            parts = [_VAL_KINDS[p] if isinstance(p, str) else int(p) for p in kind[1:]]
        except (KeyError, TypeError, ValueError):
            raise ValueError("unknown entry value kind %r" % (kind,))
        if kind[0] in ("list", "set") and parts == [VAL_STR]:
            k = (VAL_LIST if kind[0] == "list" else VAL_SET) | VAL_STR
        elif kind[0] == "map" and len(parts) == 2:
            k = EVAL_MAP | parts[0] << 4 | parts[1]
        else:
            raise ValueError("unknown entry value kind %r" % (kind,))
    try:
        k = operator.index(k)  # numpy integers too
    except TypeError:
        raise ValueError("unknown entry value kind %r" % (kind,))
    ok = k in (VAL_LIST | VAL_STR, VAL_SET | VAL_STR) or (
        k & ~0xFF == EVAL_MAP and k >> 4 & 15 in _EVAL_KEYS and k & 15 in _EVAL_VALS)
    if not ok:
        raise ValueError("unknown entry value kind %r" % (kind,))
    return int(k)


def _eval_types(kind: int):
    """(key type or 0, value type) of a kind"""
    return (kind >> 4 & 15, kind & 15) if kind & EVAL_MAP else (0, VAL_STR)


class EntryValuePlan(_WritePlan):
    """1 to 16 container columns to write, each a kind (eval_kind), on one
    context's device (dg_evals). With `field_ids` the plan builds struct
    messages, as ValuePlan does. .wire_types: the columns' wire types
    (edit_many_device's val_types)."""
    _create, _count, _wire_type, _destroy = "dg_evals_create", "dg_evals_count", "dg_evals_wire_type", "dg_evals_destroy"
    _host, _kind, _kind_dtype = "dg_evals_batch_host", staticmethod(eval_kind), np.uint16
    _rec, _fields = _lib.EvalCol, ("ent_off", "key", "key_len", "val", "val_len", "key_src", "val_src", "present")

    def work_bytes(self, n: int, n_ent) -> int:
        """the bytes of `work` entry_values_device needs for n messages whose column k holds n_ent[k] entries"""
        ne = np.array(list(n_ent), dtype=np.uint64)
        if len(ne) != self.count:
            raise ValueError("%d entry counts for a plan of %d" % (len(ne), self.count))
        return max(int(_lib.lib().dg_evals_work_bytes(self.h, n, ne.ctypes.data)), 8)


def entry_values_device(plan: EntryValuePlan, cols, n: int, out, out_off, work, status=None, out_base: int = 0,
                        cap: Optional[int] = None, stream=None):
    """Device-resident batch (dg_evals_batch_device) over torch tensors or raw
    device pointers. cols: one dict per column in the shapes entry_emit_device
    writes: ent_off int64[n + 1], key / val int64 per entry, key_len / val_len
    int32 per entry, key_src / val_src uint8 (16 spare bytes; the thrift arena
    for both when the tensors come from entry_emit_device), present uint8[n]
    (struct mode, optional), and n_ent, the entries the arrays hold (an int: no
    read-back). A list kind's elements are val / val_len / val_src. out
    uint8[cap + 16] or None (sizing); out_off int64[n * K + 1]; status uint8[n
    * K] or None; work a uint8 tensor of plan.work_bytes(n, [n_ent...]) bytes,
    this call's alone until it has run. Asynchronous on `stream`."""
    s, cap = _device_call(out, out_off, cap, stream)
    wb = int(work.numel()) * int(work.element_size()) if hasattr(work, "numel") else plan.work_bytes(n, [c["n_ent"] for c in cols])
    _lib.check(_lib.lib().dg_evals_batch_device(plan.ctx.h, plan.h, plan._cols(cols), n, out_base, _ptr(out), cap,
                                                _ptr(out_off), _ptr(status), _ptr(work), wb, s))


def _host_entry_column(kind: int, column, n: int, present=None):
    """a column of entry_values_batch as the arrays dg_evals_batch_host reads"""
    if len(column) != n:
        raise ValueError("a column of %d values for %d messages" % (len(column), n))
    kt, vt = _eval_types(kind)
    rows = [list(r.items()) if isinstance(r, dict) else list(r) for r in column]
    if not kt:
        rows = [[(None, e) for e in r] for r in rows]
    flat = [e for r in rows for e in r]
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    c = {"ent_off": off, "n_ent": len(flat)}
    for t, side, x in ((kt, "key", 0), (vt, "val", 1)):
        if not t:
            continue
        if t == VAL_STR:
            c[side], c[side + "_len"], c[side + "_src"] = _pack_strings(e[x] for e in flat)
        else:
            vals = [e[x] for e in flat]
            c[side] = _as_u64(np.asarray(vals, dtype=np.float64 if t == VAL_F64 else None), t) if vals else \
                np.zeros(0, dtype=np.uint64)
    if present is not None:
        c["present"] = _present_col(present, n)
    return c


def entry_values_batch(columns, plan, ctx: Optional[Context] = None):
    """The host path (dg_evals_batch_host): `plan` is an EntryValuePlan or a
    list of kinds; a list column is a sequence of sequences of str / bytes, a
    map column a sequence of dicts or of sequences of (key, value) pairs (pairs
    keep their order and their duplicates). Returns (arena uint8, off uint64[n
    * K + 1], status uint8[n * K]), message-major as values_batch's."""
    return _write_batch(EntryValuePlan, _host_entry_column, columns, plan, ctx)


def set_entry_columns_batch(msgs: Sequence[bytes], parent, columns, desc=None, root_type: int = STRUCT,
                            ctx: Optional[Context] = None) -> List[EditManyResult]:
    """SetMany from entry columns, the counterpart of set_columns_batch: below
    the node at `parent`, every (step, kind, column) sets the child at `step`
    of message i to column[i] encoded as the container `kind`."""
    return _set_write_columns(EntryValuePlan, _host_entry_column, msgs, parent, columns, desc, root_type, ctx)


def build_entry_structs_batch(fields, ctx: Optional[Context] = None) -> List[bytes]:
    """The counterpart of build_structs_batch for container fields: `fields`
    is a list of (field_id, kind, column[, present]); message i holds, in the
    order given, every field whose present[i] is true (all, without present),
    then STOP."""
    return _build_write_structs(EntryValuePlan, _host_entry_column, fields, ctx)


# ---------------------------------------------------------------------------
# Row column writes, the inverse of the row columns above: ragged row tensors
# encoded to list<struct> and set<struct> values (NewNodeList / NewNodeSet over
# []interface{} of map[FieldID]interface{}, thrift/generic/node.go:154-187;
# dg_rvals_* in dgj2t.h)
# ---------------------------------------------------------------------------
class RowValuePlan(_WritePlan):
    """The elements of a list<struct> (container "list" / 15) or set<struct>
    ("set" / 14) to write: 1 to 16 columns, each a kind (val_kind) and a field
    id, on one context's device (dg_rvals). A column is indexed by row; message
    i owns the rows [row_off[i], row_off[i + 1]). .wire_type: the wire type of
    every message's item (edit_many_device's val_types entry)."""
    _create, _count, _wire_type, _destroy = "dg_rvals_create", "dg_rvals_count", "dg_rvals_wire_type", "dg_rvals_destroy"
    _host, _kind, _kind_dtype = "dg_rvals_batch_host", staticmethod(val_kind), np.uint8
    _rec, _fields = _lib.ValCol, ("val", "len", "src", "elem_off", "elems", "present")

    def __init__(self, kinds, field_ids, container="list", ctx: Optional[Context] = None):
        self.ctx = ctx or default_context()
        self.kinds = [self._kind(k) for k in kinds]
        if field_ids is None:
            raise ValueError("field ids are required: the elements are structs")
        self.field_ids = [int(f) for f in field_ids]
        if len(self.field_ids) != len(self.kinds):
            raise ValueError("%d field ids for %d columns" % (len(self.field_ids), len(self.kinds)))
        container = {"list": LIST, "set": SET}.get(container, container)
        if not isinstance(container, int) or not 0 <= container <= 255:
            raise ValueError("unknown container %r" % (container,))
        ids = np.array(self.field_ids, dtype=np.int16)
        lib, h = _lib.lib(), C.c_void_p()
        _lib.check(lib.dg_rvals_create(self.ctx.h, np.array(self.kinds, dtype=np.uint8).tobytes(), len(self.kinds),
                                       ids.ctypes.data, container, C.byref(h)))
        self.h = h
        self.count = int(lib.dg_rvals_count(h))
        self.wire_type = int(lib.dg_rvals_wire_type(h))
        self.wire_types = [self.wire_type]  # one item per message

    def work_bytes(self, n: int, n_rows: int) -> int:
        """the bytes of `work` that row_values_device needs for n messages over n_rows rows"""
        return max(int(_lib.lib().dg_rvals_work_bytes(self.h, n, n_rows)), 8)


def row_values_device(plan: RowValuePlan, cols, row_off, n: int, n_rows: int, out, out_off, work, status=None,
                      cell_status=None, out_base: int = 0, cap: Optional[int] = None, stream=None):
    """Device-resident batch (dg_rvals_batch_device) over torch tensors or raw
    device pointers. row_off int64[n + 1] (rows_device's); cols: one dict per
    column, indexed by row, in the shapes rows_device / row_list_device write:
    val int64[n_rows], len int32[n_rows] and src uint8 (str; 16 spare bytes),
    elem_off int64[n_rows + 1] and elems int64 (lists and sets), present
    uint8[n_rows] (optional). n_rows is an int: no read-back. out uint8[cap +
    16] or None (sizing); out_off int64[n + 1]; status uint8[n] and cell_status
    uint8[n_rows * K] or None; work a uint8 tensor of plan.work_bytes(n, n_rows)
    bytes, this call's alone until it has run. What it fills is what
    edit_many_device takes as val / val_off for one item of plan.wire_type.
    Asynchronous on `stream`."""
    s, cap = _device_call(out, out_off, cap, stream)
    wb = int(work.numel()) * int(work.element_size()) if hasattr(work, "numel") else plan.work_bytes(n, n_rows)
    _lib.check(_lib.lib().dg_rvals_batch_device(plan.ctx.h, plan.h, plan._cols(cols), _ptr(row_off), n, n_rows, out_base,
                                                _ptr(out), cap, _ptr(out_off), _ptr(status), _ptr(cell_status), _ptr(work),
                                                wb, s))


def _row_values_host(plan: RowValuePlan, cols, row_off, n: int, n_rows: int):
    """the host entry over host columns: (arena, off[n + 1], status[n], cell_status[n_rows * K])"""
    off = np.zeros(n + 1, dtype=np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    cell_status = np.zeros(n_rows * plan.count, dtype=np.uint8)
    row_off = np.ascontiguousarray(row_off, dtype=np.uint64)
    need = C.c_uint64(0)
    recs = plan._cols(cols)
    out = np.zeros(0, dtype=np.uint8)
    for sized in (False, True):  # the first call sizes: the arena's bytes are known exactly after it
        cap = int(need.value) if sized else 0
        out = np.zeros(cap, dtype=np.uint8)
        _lib.check(_lib.lib().dg_rvals_batch_host(plan.ctx.h, plan.h, recs, row_off.ctypes.data, n, n_rows,
                                                  out.ctypes.data if cap else None, cap, off.ctypes.data, status.ctypes.data,
                                                  cell_status.ctypes.data, C.byref(need)))
        if not need.value:
            break
    return out, off, status, cell_status


def _rows_as_columns(plan: RowValuePlan, rows):
    """per message a list of rows, a row a tuple in column order with None for an absent field -> (cols, row_off, n_rows)"""
    flat = [tuple(r) for m in rows for r in m]
    if any(len(r) != plan.count for r in flat):
        raise ValueError("a row's length is not the plan's %d columns" % plan.count)
    row_off = np.zeros(len(rows) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in rows], out=row_off[1:])
    if not flat:  # every list is empty: no per-row array is read, and none is made (an empty column has no dtype)
        return [{} for _ in plan.kinds], row_off, 0
    cols = []
    for j, kind in enumerate(plan.kinds):
        present = [r[j] is not None for r in flat]
        empty = [] if kind & (VAL_LIST | VAL_SET) else b"" if kind == VAL_STR else 0
        column = [empty if r[j] is None else r[j] for r in flat]
        cols.append(_host_column(kind, column, len(flat), None if all(present) else present))
    return cols, row_off, len(flat)


def row_values_batch(rows, plan, ctx: Optional[Context] = None):
    """The host path (dg_rvals_batch_host): `rows` is, per message, a list of
    rows; a row is a tuple in column order, with None for an absent field
    (values as values_batch takes them). `plan` is a RowValuePlan or a list of
    (field_id, kind). Returns (arena uint8, off uint64[n + 1], status uint8[n],
    cell_status uint8[n_rows * K]): message i's list is arena[off[i]:off[i + 1]]."""
    wp = plan if isinstance(plan, RowValuePlan) else RowValuePlan([f[1] for f in plan], [f[0] for f in plan], "list", ctx)
    with _unless_given(wp, plan):
        if not rows:
            return np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.uint8)
        cols, row_off, n_rows = _rows_as_columns(wp, rows)
        return _row_values_host(wp, cols, row_off, len(rows), n_rows)


def set_rows_batch(msgs: Sequence[bytes], path, fields, rows, container="list", desc=None, root_type: int = STRUCT,
                   ctx: Optional[Context] = None) -> List[EditManyResult]:
    """SetMany of one list<struct> per message: `fields` is a list of (field_id,
    kind), `rows` per message a list of rows (row_values_batch); the list is
    encoded on the device and set as the child that `path`'s last step names,
    below the node at the steps before it (set_many_batch's host entry with one
    item of the plan's wire type). The statuses of row_values_batch are not
    returned, as set_columns_batch returns none: a message flagged SIZE is set
    as the empty list and a flagged cell as the empty value of its kind; call
    row_values_batch where they matter."""
    path = list(path)
    if not path:
        raise ValueError("the empty path names no item")
    if len(rows) != len(msgs):
        raise ValueError("%d row lists for %d messages" % (len(rows), len(msgs)))
    with RowValuePlan([f[1] for f in fields], [f[0] for f in fields], container, ctx) as wp:
        arena, off, _, _ = row_values_batch(rows, wp)
        with EditManyPlan(path[:-1], [path[-1]], EDIT_SET, desc, ctx) as plan:
            return _editm_batch(msgs, plan, None, [wp.wire_type], root_type, encoded=(arena, off))


def build_row_lists_batch(fields, rows, container="list", ctx: Optional[Context] = None) -> List[bytes]:
    """NewNodeList of structs for a batch: `fields` is a list of (field_id,
    kind), `rows` per message a list of rows (row_values_batch); returns the
    bare list values as bytes. The statuses are not returned: a flagged message
    is the empty list, a flagged cell the empty value (row_values_batch gives
    them)."""
    with RowValuePlan([f[1] for f in fields], [f[0] for f in fields], container, ctx) as wp:
        arena, off, _, _ = row_values_batch(rows, wp)
        return _split(arena, off)
