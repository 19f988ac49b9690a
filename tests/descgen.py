"""Descriptor families whose outcomes are known from how they are built.

The conversions read two inputs, the message and the flattened descriptor
blob (include/dgj2t_desc.h). This module builds the second one on purpose:
every family is a list of ``Case`` (a TypeDescriptor and its messages), every
message comes with an ``Intent`` -- what the conversion must make of it, worked
out from the construction and the struct's Python name map, never from a
converter -- and every shape the blob is built for (table sizes, probe chains,
struct indices, total_len, field flags) can be read back from the blob with
the helpers at the end.

Deterministic: fixed construction, integer arithmetic, no random numbers.

  names     key lengths 0..40 around the 8- and 16-byte seams, equal 32-bit
            hashes, probe chains that wrap the table end, 1 / 16 / 17 / 52
            names (tables of 2 / 32 / 64 / 128 slots), near-miss keys
  aliases   alias != name, aliases that shadow names and each other
            (DG_FF_ALIAS_SELF), aliases that need escapes (DG_FF_KEY_PLAIN)
  ids       ids 1 .. 32767 declared out of order, keys in every order
  counts    1 .. 257 fields, flat and nested (list, map, recursive)
  reqarena  recursive wide structs that exhaust the lane kernel's requires
            arena before its frames
  structs   a chain of 72 structs: REQUIRED checks at struct index 62 .. 65;
            a tree of 81 with those indices three levels down
  sizes     the same live struct in blobs of 12 288 / 16 384 / 49 152 bytes
            and 8 bytes to either side
"""
import os
import re
import struct
from collections import namedtuple

from dynamicgo_amd import thrift as T

HIT, UNKNOWN, MISSING = "hit", "unknown", "missing"
# kind HIT: ret 0 and the Thrift bytes carry the field ids `ids` (of the
#   innermost struct the message fills); UNKNOWN: the key ids[0] names no
#   field -- skipped under F_ALLOW_UNKNOWN (the fields ids[1] are written),
#   ERR_UNKNOWN_FIELD without;
#   MISSING: REQUIRED field ids[0] is the lowest one absent. `escaped`: the
#   JSON key carries an escape, so the fast routes must hand the message on.
#   `depth`: structs the message opens (1 = the root only).
Intent = namedtuple("Intent", "kind ids escaped depth", defaults=(False, 1))

E_NULL_REQUIRED, E_UNKNOWN_FIELD = 10, 12  # reference native/native.h error codes
F_ALLOW_UNKNOWN, F_WRITE_DEFAULT, F_WRITE_REQUIRE, F_WRITE_OPTIONAL = 0x1, 0x2, 0x20, 0x80
FLAG_WORDS = (0x0, 0x1, 0x3, 0x21, 0x83, 0xa3)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dynamicgo_amd", "csrc")


def kernel_const(header, name):
    """An integer constant of the kernels, read from the header that defines it."""
    with open(os.path.join(CSRC, header)) as fh:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, fh.read())
    return int(eval(m.group(1), {"__builtins__": {}}))  # "16 * 1024", "48 * 1024", "256"


class Case:
    def __init__(self, name, td, msgs, **props):
        self.name = name
        self.td = td
        self.msgs = [m for m, _ in msgs]
        self.intents = [i for _, i in msgs]
        self.props = props
        self._flat = None

    @property
    def flat(self):
        if self._flat is None:
            self._flat = T.flatten(self.td)
        return self._flat

    def __repr__(self):
        return "Case(%s, %d msgs)" % (self.name, len(self.msgs))


I32 = T.builtin("i32")
SCALARS = ["i32", "i64", "string", "bool", "double", "byte", "i16"]
VALUES = {"i32": b"7", "i64": b"5", "string": b'"s"', "bool": b"true", "double": b"1.5", "byte": b"3", "i16": b"4"}
REQ_CYCLE = (T.OPTIONAL, T.DEFAULT, T.REQUIRED)


def jkey(raw: bytes) -> bytes:
    """The JSON text of a key: the reference's own quoting."""
    return b'"' + T.json_quote(raw) + b'"'


def one_key(key_json: bytes, value: bytes = b"7") -> bytes:
    return b"{" + key_json + b":" + value + b"}"


def lookup(sd, raw: bytes):
    """The struct's name map (alias and name, last Set wins) on raw key bytes."""
    try:
        return sd.names.get(raw.decode("utf-8"))
    except UnicodeDecodeError:
        return None


def intent_for_keys(sd, raws, escaped=False, depth=1):
    """What a message with these (unescaped) keys must give: the first key
    that names no field, else the lowest REQUIRED field left out, else a hit
    of every field named."""
    found = [lookup(sd, r) for r in raws]
    ids = [f.id for f in found if f is not None]
    for r, f in zip(raws, found):
        if f is None:
            return Intent(UNKNOWN, (r, tuple(ids)), escaped, depth)
    miss = sorted(f.id for f in sd.fields if f.required == T.REQUIRED and f.id not in ids)
    if miss:
        return Intent(MISSING, (miss[0],), escaped, depth)
    return Intent(HIT, tuple(ids), escaped, depth)


# ---------------------------------------------------------------- names
ALPHA = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def hash_from(h, tail: bytes):
    for b in tail:
        h = (((h << 5) + h) & 0xFFFFFFFF) ^ b
    return h


def find_collisions(prefix: bytes, want: int):
    """`want` pairs of distinct names prefix+xy with equal name_hash, found by
    searching the two-letter tails (h = h*33 ^ b makes them plentiful)."""
    h0 = hash_from(5381, prefix)
    seen, pairs, used = {}, [], set()
    for a in ALPHA:
        for b in ALPHA:
            t = (a + b).encode()
            h = hash_from(h0, t)
            o = seen.setdefault(h, t)
            if o != t and o not in used and t not in used:
                pairs.append((prefix + o, prefix + t))
                used.update((o, t))
                if len(pairs) == want:
                    return pairs
    raise AssertionError("no collisions after %r" % prefix)


def names_for_slot(slot, mask, count, length, taken):
    """`count` names of `length` bytes whose hash starts them at `slot`."""
    out = []
    for k in range(52 ** min(length, 3)):
        n = bytes(ALPHA[(k // 52 ** j) % 52].encode()[0] for j in range(length))
        if T.name_hash(n) & mask == slot and n not in taken:
            out.append(n)
            if len(out) == count:
                return out
    raise AssertionError("no %d names for slot %d" % (count, slot))


INV33 = pow(33, -1, 1 << 32)
_nul_cache = {}


def nul_proof_names(count, zero_bits=26):
    """Six-letter names whose hash has `zero_bits` trailing zero bits. A NUL
    byte multiplies the hash by 33, and 33^2 - 1 = 2^6 * 17, so name + two NUL
    bytes has the SAME 32-bit hash as the name, starts at the same slot and
    equals the name's zero-padded pool word: only the `key_len == kn` test of
    a lookup tells the two apart. Found by meeting in the middle (the hash
    step is invertible): three letters forward from the seed, three back from
    a target."""
    if (count, zero_bits) in _nul_cache:
        return list(_nul_cache[count, zero_bits])
    fwd = {}
    for a in ALPHA:
        for b in ALPHA:
            for c in ALPHA:
                t = (a + b + c).encode()
                fwd.setdefault(hash_from(5381, t), t)
    out = []
    for target in range(1 << zero_bits, 1 << 32, 1 << zero_bits):
        for a in ALPHA:
            for b in ALPHA:
                for c in ALPHA:
                    t = (a + b + c).encode()
                    h = target
                    for ch in reversed(t):
                        h = ((h ^ ch) * INV33) & 0xFFFFFFFF
                    if h in fwd:
                        n = fwd[h] + t
                        assert T.name_hash(n) == target == T.name_hash(n + b"\0\0")
                        out.append(n)
                        if len(out) == count:
                            _nul_cache[count, zero_bits] = tuple(out)
                            return out
    raise AssertionError("no such names")


def lname(n, tag=b"k"):
    """A name of exactly n bytes, different for every (n, tag)."""
    return (tag + b"%d" % n + b"abcdefghijklmnopqrstuvwxyz0123456789ABCD")[:n]


SEAMS = (7, 8, 9, 15, 16, 17, 24, 25)


def near_misses(raw: bytes):
    """JSON key texts next to a name: (key json, raw bytes after unquoting,
    written with an escape)."""
    out = []
    for i in range(len(raw)):
        out.append(raw[:i] + bytes([raw[i] ^ 1]) + raw[i + 1:])
    out.append(raw[:-1] if raw else b"x")
    out.append(raw + b"x")
    if raw.swapcase() != raw:
        out.append(raw.swapcase())
    res = [(b'"' + r + b'"', r, False) for r in out]
    for k in range(1, 9):
        r = raw + bytes(k)
        res.append((b'"' + r + b'"', r, False))  # raw NUL bytes in the JSON text
        res.append((b'"' + raw + b"\\u0000" * k + b'"', r, True))
    return res


def _names_case(tag, names):
    sd_fields = [T.FieldDescriptor(k + 1, n.decode(), I32, T.OPTIONAL) for k, n in enumerate(names)]
    td = T.struct_type(tag, sd_fields)
    sd = td.struct
    assert len(sd.names) == len(names), tag
    msgs = []
    for k, n in enumerate(names):
        v = b"%d" % (1000 + k)
        msgs.append((one_key(jkey(n), v), intent_for_keys(sd, [n])))
        for kj, raw, esc in near_misses(n):
            msgs.append((one_key(kj, v), intent_for_keys(sd, [raw], esc)))
    return Case(tag, td, msgs, n_names=len(names))


def names_family():
    pairs = find_collisions(b"", 2) + find_collisions(b"collide-", 1) + find_collisions(b"0123456789abcd", 1)
    assert len({T.name_hash(a) for a, _ in pairs}) == len(pairs)
    for a, b in pairs:
        assert a != b and T.name_hash(a) == T.name_hash(b)
    cases = [_names_case("N1", [lname(8)])]
    # 16 names, 32 slots: the seams, the empty name, a pair with one hash,
    # two names that name + NUL NUL cannot be told from by hash and bytes,
    # three names that start at the last slot: the chain wraps to slots 0 and 1
    n16 = [lname(n) for n in SEAMS] + [b""]
    nul = nul_proof_names(2)
    n16 += list(pairs[0]) + nul
    n16 += names_for_slot(31, 31, 3, 6, n16)
    assert len(n16) == 16
    cases.append(_names_case("N16", n16))
    # 17 names, 64 slots: one more than the flat kernel's key table takes
    n17 = [lname(n, b"m") for n in SEAMS] + list(pairs[1]) + nul[:1]
    n17 += [b"pre", b"prefix", b"prefixed"] + names_for_slot(63, 63, 3, 5, n17)
    assert len(n17) == 17
    cases.append(_names_case("N17", n17))
    # every length 0..40, 128 slots; a 16-byte pair that differs in its last word
    nl = [lname(n, b"L") for n in range(41)] + nul + [pairs[0][0] + b"SUFFIX", pairs[0][1] + b"SUFFIX"] + list(pairs[2]) + list(pairs[3]) + names_for_slot(127, 127, 3, 11, [])
    cases.append(_names_case("NL", nl))
    for c in cases[1:]:
        c.props["nul_proof"] = nul
    return cases, pairs


# ---------------------------------------------------------------- aliases
def aliases_family():
    F = T.FieldDescriptor
    specials = [b'q"uote', b"back\\slash", b"ctl\x01x", "é中".encode(), b"nul\x00in", b'"', b"\\"]
    fields = [
        F(1, "alpha", I32, T.OPTIONAL, alias="ALPHA"),     # alias != name, both are keys
        F(2, "beta", I32, T.OPTIONAL, alias="alpha"),      # alias == field 1's name: "alpha" is field 2 now
        F(3, "gamma", I32, T.OPTIONAL, alias="shared"),    # one alias, two fields: the later one keeps it
        F(4, "delta", I32, T.OPTIONAL, alias="shared"),
        F(5, "eps", I32, T.OPTIONAL, alias="zeta"),        # alias shadowed by field 6's NAME
        F(6, "zeta", I32, T.OPTIONAL, alias="zeta6"),
    ]
    fields += [F(7 + k, "sp%d" % k, I32, T.OPTIONAL, alias=s.decode()) for k, s in enumerate(specials)]
    td = T.struct_type("Aliases", fields)
    sd = td.struct
    msgs = []
    keys = sorted({k.encode() for k in sd.names} | {f.alias.encode() for f in fields} | {f.name.encode() for f in fields})
    for k, raw in enumerate(keys):
        kj = jkey(raw)
        esc = b"\\" in kj
        v = b"%d" % (2000 + k)
        msgs.append((one_key(kj, v), intent_for_keys(sd, [raw], esc)))
        # the same key written with a needless \u escape for its first byte
        if raw:
            msgs.append((one_key(b'"\\u%04x' % raw[0] + T.json_quote(raw[1:]) + b'"', v) if raw[0] < 0x80 else
                         one_key(kj, v), intent_for_keys(sd, [raw], raw[0] < 0x80 or esc)))
        for kj2, r2, e2 in near_misses(raw):
            if b'"' in r2 or b"\\" in r2 or any(c < 0x20 and c != 0 for c in r2):
                kj2, e2 = jkey(r2), True
            msgs.append((one_key(kj2, v), intent_for_keys(sd, [r2], e2)))
    # two keys of one field and the shadowed pairs side by side (last write is a duplicate field)
    for a, b in ((b"ALPHA", b"alpha"), (b"shared", b"gamma"), (b"zeta", b"eps"), (b"delta", b"shared")):
        msgs.append((b"{" + jkey(a) + b":1," + jkey(b) + b":2}", intent_for_keys(sd, [a, b])))
    want_self = {1: True, 2: True, 3: False, 4: True, 5: False, 6: True}
    # DG_FF_KEY_PLAIN as dgj2t_desc.h defines it and thrift.flatten sets it: no '"' and no '\' byte in the
    # alias (no escape can start inside a key equal to it). A control byte, NUL or non-ASCII bytes leave it
    # set: their JSON keys are escaped (or, non-ASCII, raw and equal), which the key scan sees for itself.
    want_plain = {7: False, 8: False, 9: True, 10: True, 11: True, 12: False, 13: False}
    return [Case("Aliases", td, msgs, alias_self=want_self, key_plain=want_plain)]


# ---------------------------------------------------------------- ids
IDS = (1, 127, 128, 255, 256, 32766, 32767)
DECL = (256, 1, 32767, 127, 32766, 128, 255)


def ids_desc():
    return T.struct_type("Ids", [T.FieldDescriptor(i, "f%d" % i, I32, (T.OPTIONAL, T.DEFAULT)[k & 1])
                                 for k, i in enumerate(DECL)])


def ids_family():
    td = ids_desc()
    sd = td.struct
    orders = {"id": sorted(DECL), "decl": list(DECL), "reversed": sorted(DECL, reverse=True),
              "rotated": sorted(DECL)[1:] + sorted(DECL)[:1]}
    msgs = []
    for order in orders.values():
        for take in range(1, len(order) + 1):
            ks = [b"f%d" % i for i in order[:take]]
            body = b",".join(jkey(k) + b":%d" % (3000 + i) for k, i in zip(ks, order))
            msgs.append((b"{" + body + b"}", intent_for_keys(sd, ks)))
    for i in DECL:
        for d in (-1, 1):
            k = b"f%d" % (i + d)
            msgs.append((one_key(jkey(k)), intent_for_keys(sd, [k])))
    msgs.append((b"{}", intent_for_keys(sd, [])))
    return [Case("Ids", td, msgs, orders=orders)]


# ---------------------------------------------------------------- counts
COUNTS = (1, 7, 8, 9, 23, 24, 25, 63, 64, 65, 128, 129, 257)
FORMS = ("flat", "list", "map", "self")


def wide_struct(n, name="W", self_field=False, phase=0):
    """n fields c0..c{n-1}, ids 1..n, types and requireness cycling (from
    REQ_CYCLE[phase]); with self_field, field 0 (OPTIONAL) is the struct itself."""
    sd = T.StructDescriptor(name)
    td = T.TypeDescriptor(T.STRUCT, name, struct=sd)
    kinds = []
    for k in range(n):
        if self_field and k == 0:
            ft, kind = td, "self"
        else:
            kind = SCALARS[k % len(SCALARS)]
            ft = T.builtin(kind)
        kinds.append(kind)
        sd.add_field(T.FieldDescriptor(k + 1, "c%d" % k, ft, T.OPTIONAL if kind == "self" else REQ_CYCLE[(k + phase) % 3]))
    return td, kinds


def _obj(ks, kinds):
    return b"{" + b",".join(b'"c%d":' % k + VALUES[kinds[k]] for k in ks) + b"}"


def counts_case(n, form, phase=0):
    """phase 2 makes the LAST field of a 64-field struct REQUIRED (bit 63 of
    the requires word and of the wave kernel's REQUIRED mask)."""
    wd, kinds = wide_struct(n, "W%d" % n, self_field=(form == "self"), phase=phase)
    sd = wd.struct
    scal = [k for k in range(n) if kinds[k] != "self"]
    req = [k for k in scal if REQ_CYCLE[(k + phase) % 3] == T.REQUIRED]
    sets = [scal, [], req, req[:-1], scal[-1:], scal[-1:] * 3]
    picks = scal if n <= 65 else [k for k in (1, 61, 62, 63, 64, 65, 66, 127, 128, 129, n - 2, n - 1) if k < n]
    sets += [sorted(set(req) | {k}) for k in picks]
    sets += [[k] + req for k in picks[-3:]]  # the late field first: the prediction never hits
    if form == "flat":
        td = wd
        wrap, depth = (lambda o: o), 1
    elif form == "list":
        td = T.struct_type("L", [T.FieldDescriptor(1, "l", T.list_of(wd), T.OPTIONAL)])
        wrap, depth = (lambda o: b'{"l":[' + o + b"," + o + b"]}"), 2
    elif form == "map":
        td = T.struct_type("M", [T.FieldDescriptor(1, "m", T.map_of(T.builtin("string"), wd), T.OPTIONAL)])
        wrap, depth = (lambda o: b'{"m":{"k":' + o + b"}}"), 2
    else:
        td = wd
        depth = 2
    msgs = []
    for ks in sets:
        inner = intent_for_keys(sd, [b"c%d" % k for k in ks], depth=depth)
        o = _obj(ks, kinds)
        if form == "self":
            # the outer level carries every REQUIRED field, so the verdict is the inner one's
            outer = b",".join([b'"c%d":' % k + VALUES[kinds[k]] for k in req] + [b'"c0":' + o])
            m = b"{" + outer + b"}"
        else:
            m = wrap(o)
        msgs.append((m, inner))
    return Case("W%d-%s%s" % (n, form, "-p%d" % phase if phase else ""), td, msgs, n=n, form=form, wide=sd, phase=phase)


def counts_family(forms=FORMS, counts=COUNTS):
    return [counts_case(n, f) for f in forms for n in counts] + [counts_case(64, f, phase=2) for f in forms]


# ---------------------------------------------------------------- reqarena
def reqarena_case():
    """The exact machine keeps the requires bits of every open struct of more
    than 64 fields in a per-lane arena of WS_REQCAP words (j2t_machine.h:
    `reqlen + sd.req_words > ws.reqcap` -> DG_ST_DEEP, the deep pass redoes
    the message). The lane kernel has LDS_DEPTH frames per lane, so the arena
    runs out first only for structs of more than WS_REQCAP / LDS_DEPTH words:
    the struct here has w = WS_REQCAP / (LDS_DEPTH / 2) words, fits exactly
    `fit` = LDS_DEPTH / 2 deep (fit * w == WS_REQCAP) and not one deeper."""
    reqcap, frames = kernel_const("j2t_machine.h", "WS_REQCAP"), kernel_const("j2t_machine.h", "LDS_DEPTH")
    fit = frames // 2
    w = reqcap // fit
    assert fit * w == reqcap and fit + 2 < frames
    n = 64 * (w - 1) + 1
    sd = T.StructDescriptor("Arena")
    td = T.TypeDescriptor(T.STRUCT, "Arena", struct=sd)
    sd.add_field(T.FieldDescriptor(1, "c0", td, T.OPTIONAL))
    for k in range(1, n):
        # OPTIONAL and DEFAULT in turn: under F_WRITE_DEFAULT every open level walks all its
        # requires words and writes the 2016 unset DEFAULT fields (14 KB a level)
        sd.add_field(T.FieldDescriptor(k + 1, "c%d" % k, I32, T.REQUIRED if k == n - 1 else (T.OPTIONAL, T.DEFAULT)[k & 1]))
    last = b'"c%d":9' % (n - 1)
    msgs = []
    for depth in (1, fit - 1, fit, fit + 1, fit + 2):
        for rep in range(3):
            m = b"{" + last + b',"c%d":%d}' % (1 + rep, rep)
            for _ in range(depth - 1):
                m = b"{" + last + b',"c0":' + m + b"}"
            msgs.append((m, Intent(HIT, (n, 2 + rep), False, depth)))
    m = b"{" + last + b"}"
    for _ in range(fit):  # beyond the arena, and the innermost struct lacks nothing / the outermost its REQUIRED field
        m = b'{"c0":' + m + b"}"
    msgs.append((m, Intent(MISSING, (n,), False, fit + 1)))
    return Case("Arena", td, msgs, fit=fit, req_words=w, n=n)


# ---------------------------------------------------------------- structs
CHAIN = 72
CHECKED = (0, 10, 62, 63, 64, 65)


def structs_case():
    """S0 -> S1 -> ... -> S71: "n" is the next struct, "r" a REQUIRED i32.
    The struct's blob index is its place in the chain (flatten visits in
    that order); the wave kernel keeps REQUIRED masks for the first
    WV_REQMASKS structs only."""
    tds = []
    for k in range(CHAIN):
        sd = T.StructDescriptor("S%d" % k)
        tds.append(T.TypeDescriptor(T.STRUCT, "S%d" % k, struct=sd))
    for k in range(CHAIN):
        sd = tds[k].struct
        if k + 1 < CHAIN:
            sd.add_field(T.FieldDescriptor(1, "n", tds[k + 1], T.OPTIONAL))
        sd.add_field(T.FieldDescriptor(2, "r", I32, T.REQUIRED))
        if k % 2:
            sd.add_field(T.FieldDescriptor(3, "o", I32, T.OPTIONAL))

    def nest(depth, missing=None):
        m = b""
        for lvl in range(depth - 1, -1, -1):
            parts = [] if lvl == missing else [b'"r":%d' % lvl]
            if m:
                parts.append(b'"n":' + m)
            m = b"{" + b",".join(parts) + b"}"
        return m
    msgs, missing_at = [], []
    for depth in (1, 2, 11, 63, 64, 65, 66, 67, CHAIN):
        msgs.append((nest(depth), Intent(HIT, (2,), False, depth)))
        missing_at.append(None)
    for lvl in CHECKED:
        for depth in (lvl + 1, lvl + 2, min(CHAIN, lvl + 4)):
            msgs.append((nest(depth, missing=lvl), Intent(MISSING, (2,), False, depth)))
            missing_at.append(lvl)
    return Case("Chain", tds[0], msgs, checked=CHECKED, missing_at=missing_at)


def tree_case():
    """Struct indices past the wave kernel's mask table at a depth it takes:
    R {a0..a7: A_k}, A_k {b0..b8: B_kj}, B_kj {r: REQUIRED i32} -- 81 structs,
    A_k at blob index 1 + 10k, so the B's with index 62..66 are three levels down. (The chain reaches those
    indices only 63 and more levels deep, where the wave kernel has long
    handed the message on.)"""
    leaves = {}
    a_fields = []
    for k in range(8):
        b_fields = []
        for j in range(9):
            leaves[k, j] = T.struct_type("B%d%d" % (k, j), [T.FieldDescriptor(1, "r", I32, T.REQUIRED)])
            b_fields.append(T.FieldDescriptor(j + 1, "b%d" % j, leaves[k, j], T.OPTIONAL))
        a_fields.append(T.FieldDescriptor(k + 1, "a%d" % k, T.struct_type("A%d" % k, b_fields), T.OPTIONAL))
    td = T.struct_type("Tree", a_fields)
    msgs, leaf_of = [], []
    for (k, j) in sorted(leaves):
        for body, intent in ((b'{"r":%d}' % (10 * k + j), Intent(HIT, (1,), False, 3)), (b"{}", Intent(MISSING, (1,), False, 3))):
            msgs.append((b'{"a%d":{"b%d":' % (k, j) + body + b"}}", intent))
            leaf_of.append((k, j))
    return Case("Tree", td, msgs, leaves=leaves, leaf_of=leaf_of)


# ---------------------------------------------------------------- sizes
SIZE_EDGES = (12288, 16384, 49152)
SIZE_TARGETS = tuple(t + d for t in SIZE_EDGES for d in (-8, 0, 8))
LIVE = (("req", "i32", T.REQUIRED), ("str", "string", T.OPTIONAL), ("big", "i64", T.DEFAULT),
        ("dbl", "double", T.OPTIONAL), ("yes", "bool", T.OPTIONAL))
N_PAD = 56


def sized_desc(target, n_pad=N_PAD):
    """The live struct plus n_pad OPTIONAL i32 fields no message names, their
    names as long as it takes for the blob to be exactly `target` bytes (pool
    keys are padded to 8 bytes, so the blob moves in steps of 8)."""
    def build(lens):
        fs = [T.FieldDescriptor(k + 1, n, T.builtin(t), r) for k, (n, t, r) in enumerate(LIVE)]
        fs += [T.FieldDescriptor(100 + k, ("p%02d" % k).ljust(ln, "x"), I32, T.OPTIONAL) for k, ln in enumerate(lens)]
        return T.struct_type("Sized", fs)
    lens = [8] * n_pad
    base = len(T.flatten(build(lens)))
    assert (target - base) % 8 == 0 and target >= base, (target, base)
    extra = (target - base) // 8
    for k in range(n_pad):
        lens[k] += 8 * (extra // n_pad + (1 if k < extra % n_pad else 0))
    td = build(lens)
    assert len(T.flatten(td)) == target
    return td


def sizes_messages():
    """One batch for every size: the live fields in and out of order, each
    alone, unknown keys, the REQUIRED one missing."""
    live = [n.encode() for n, _, _ in LIVE]
    kinds = {n.encode(): t for n, t, _ in LIVE}
    sd = T.struct_type("Live", [T.FieldDescriptor(k + 1, n, T.builtin(t), r) for k, (n, t, r) in enumerate(LIVE)]).struct
    sets = [live, live[::-1], live[1:] + live[:1], [], [b"req"]]
    sets += [[b"req", k] for k in live[1:]] + [[k, b"req"] for k in live[1:]] + [[k] for k in live[1:]]
    sets += [[b"req", b"nope"], [b"p00", b"req"], [b"req", b"p00xxxx"], [b"req", b"re"], [b"req", b"reqq"]]
    msgs = []
    for rep in range(40):  # a few hundred messages, more than one wave of them
        for ks in sets:
            body = b",".join(jkey(k) + b":" + (VALUES[kinds[k]] if k in kinds else b"%d" % rep) for k in ks)
            msgs.append((b"{" + body + b"}", intent_for_keys(sd, ks)))
    return msgs


def sizes_family(targets=SIZE_TARGETS):
    msgs = sizes_messages()
    return [Case("Sized%d" % t, sized_desc(t), msgs, total_len=t) for t in targets]


def chain_sized_desc(target):
    """A blob of exactly `target` bytes whose t2j side table stays small (the
    t2j wave kernel also wants the side table in LDS): the live fields plus a
    chain of one-field structs no message enters, the last one with a field
    whose name makes up the difference."""
    def build(n, tune):
        tds = [T.TypeDescriptor(T.STRUCT, "P%d" % k, struct=T.StructDescriptor("P%d" % k)) for k in range(n)]
        for k in range(n - 1):
            tds[k].struct.add_field(T.FieldDescriptor(1, "n", tds[k + 1], T.OPTIONAL))
        tds[-1].struct.add_field(T.FieldDescriptor(1, "t".ljust(tune, "u"), I32, T.OPTIONAL))
        fs = [T.FieldDescriptor(k + 1, nm, T.builtin(t), r) for k, (nm, t, r) in enumerate(LIVE)]
        return T.struct_type("ChainSized", fs + [T.FieldDescriptor(50, "pad", tds[0], T.OPTIONAL)])
    n = 2
    while len(T.flatten(build(n + 1, 8))) <= target:
        n += 1
    diff = target - len(T.flatten(build(n, 8)))
    td = build(n, 8 + diff)
    assert len(T.flatten(td)) == target, (target, len(T.flatten(td)))
    return td


# ---------------------------------------------------------------- t2j messages
def t2j_value(kind):
    return {"i32": b"\x08", "i64": b"\x0a", "string": b"\x0b", "bool": b"\x02", "double": b"\x04", "byte": b"\x03",
            "i16": b"\x06"}[kind], {"i32": struct.pack(">i", 7), "i64": struct.pack(">q", -5),
                                    "string": struct.pack(">i", 2) + b"s\"", "bool": b"\x01",
                                    "double": struct.pack(">d", 1.5), "byte": b"\x03", "i16": struct.pack(">h", 4)}[kind]


_KIND_OF = {T.I32: "i32", T.I64: "i64", T.STRING: "string", T.BOOL: "bool", T.DOUBLE: "double", T.BYTE: "byte",
            T.I16: "i16"}


def t2j_field(fid, kind):
    t, v = t2j_value(kind)
    return t + struct.pack(">H", fid & 0xFFFF) + v


def t2j_messages(sd, limit=24):
    """Thrift structs over sd's scalar fields: sorted, reversed and shuffled
    (a fixed stride permutation), every REQUIRED one / all but the last,
    and unknown ids id-1, id+1, 0, 0x7FFF, 0x8000, 0xFFFF next to known ones
    (an unknown id that is a field of sd is simply that field)."""
    fs = [(f.id, _KIND_OF[f.type.type]) for f in sorted(sd.fields, key=lambda f: f.id) if f.type.type in _KIND_OF]
    n = len(fs)
    known = {i for i, _ in fs}
    stride = next(s for s in range(max(2, n // 3), n + 3) if n < 2 or _gcd(s, n) == 1)
    shuffled = [fs[(k * stride) % n] for k in range(n)]
    req = [(i, k) for i, k in fs if sd.ids[i].required == T.REQUIRED]
    orders = [fs, fs[::-1], shuffled, req, req[:-1], [], fs[-1:] * 2]
    step = max(1, n // limit)
    for j in range(0, n, step):
        fid, kind = fs[j]
        for u in (fid - 1, fid + 1, 0, 0x7FFF, 0x8000, 0xFFFF):
            if (u & 0xFFFF) in known:
                continue
            orders.append(req + [(u, "i32"), (fid, kind), (u, "string")])
            orders.append([(fid, kind), (u, "i64")] + req[::-1])
    return [b"".join(t2j_field(i, k) for i, k in o) + b"\x00" for o in orders]


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


# ---------------------------------------------------------------- reading the blob back
Hdr = namedtuple("Hdr", "magic version total_len root_type n_types off_types n_structs off_structs n_fields "
                        "off_fields n_names off_names n_reqwords off_reqwords pool_len off_pool")


def blob_hdr(blob):
    return Hdr(*struct.unpack_from(T.HDR_FMT, blob, 0))


def blob_struct(blob, si):
    h = blob_hdr(blob)
    return struct.unpack_from(T.STRUCT_FMT, blob, h.off_structs + 32 * si)  # field_begin n_fields name_begin name_mask ...


def blob_type(blob, ti):
    return struct.unpack_from(T.TYPE_FMT, blob, blob_hdr(blob).off_types + 16 * ti)  # ttype flags pad key elem st


def blob_field(blob, fi):
    # id required flags vm key_len type dflt_off dflt_len key_off
    return struct.unpack_from(T.FIELD_FMT, blob, blob_hdr(blob).off_fields + 24 * fi)


def blob_names(blob, si):
    """The struct's name table: per slot None or (hash, key bytes, field)."""
    h = blob_hdr(blob)
    _, _, nb, mask = blob_struct(blob, si)[:4]
    out = []
    for s in range(mask + 1):
        hs, ko, kl, fi = struct.unpack_from(T.NAME_FMT, blob, h.off_names + 16 * (nb + s))
        out.append(None if fi == T.DG_NONE else (hs, blob[h.off_pool + ko:h.off_pool + ko + kl], fi))
    return out


def probe_chains(blob, si):
    """(longest probe chain, whether one of at least 3 wraps the table end):
    a key's chain is the slots from its hash's start slot to where it sits."""
    slots = blob_names(blob, si)
    size = len(slots)
    longest, wraps = 0, False
    for j, s in enumerate(slots):
        if s is None:
            continue
        start = s[0] & (size - 1)
        ln = ((j - start) % size) + 1
        longest = max(longest, ln)
        wraps |= ln >= 3 and j < start
    return longest, wraps


def thrift_structs(buf):
    """Field ids of every struct in a Thrift-binary value that is a struct,
    outermost first: [(depth, [ids])]."""
    out = []

    def value(t, p, depth):
        if t == T.STRUCT:
            mine = []
            out.append((depth, mine))
            while True:
                ft = buf[p]
                p += 1
                if ft == 0:
                    return p
                mine.append(struct.unpack_from(">H", buf, p)[0])
                p = value(ft, p + 2, depth + 1)
        if t in (T.BOOL, T.BYTE):
            return p + 1
        if t == T.I16:
            return p + 2
        if t == T.I32:
            return p + 4
        if t in (T.I64, T.DOUBLE):
            return p + 8
        if t == T.STRING:
            return p + 4 + struct.unpack_from(">i", buf, p)[0]
        if t in (T.LIST, T.SET):
            et, n = buf[p], struct.unpack_from(">i", buf, p + 1)[0]
            p += 5
            for _ in range(n):
                p = value(et, p, depth)
            return p
        if t == T.MAP:
            kt, vt, n = buf[p], buf[p + 1], struct.unpack_from(">i", buf, p + 2)[0]
            p += 6
            for _ in range(n):
                p = value(kt, p, depth)
                p = value(vt, p, depth)
            return p
        raise ValueError("wire type %d" % t)
    end = value(T.STRUCT, 0, 1)
    assert end == len(buf), (end, len(buf))
    return out


def check_intent(intent, flags, ret, out):
    """None if (ret, out) is what the intent says under `flags`, else why not."""
    code = ret & 0xFF
    if intent.kind == UNKNOWN and not flags & F_ALLOW_UNKNOWN:
        return None if code == E_UNKNOWN_FIELD else "want ERR_UNKNOWN_FIELD, got %#x" % ret
    if intent.kind == MISSING and not flags & F_WRITE_REQUIRE:
        if code != E_NULL_REQUIRED or (ret >> 40) != intent.ids[0]:
            return "want ERR_NULL_REQUIRED of field %d, got %#x" % (intent.ids[0], ret)
        return None
    if ret != 0:
        return "want ret 0, got %#x" % ret
    structs = thrift_structs(out)
    deepest = max(d for d, _ in structs)
    if deepest != intent.depth:
        return "want %d structs deep, got %d" % (intent.depth, deepest)
    inner = [ids for d, ids in structs if d == deepest]
    if intent.kind == MISSING:
        return None if all(intent.ids[0] in ids for ids in inner) else "field %d not written" % intent.ids[0]
    # HIT: the fields named; UNKNOWN (skipped): the fields named beside it.
    # They are written as they are met, in the message's order; what a write
    # flag adds for the unset fields comes at the struct's end and is none of them.
    want = list(intent.ids[1] if intent.kind == UNKNOWN else intent.ids)
    adds = flags & (F_WRITE_DEFAULT | F_WRITE_REQUIRE | F_WRITE_OPTIONAL)
    for ids in inner:
        if ids[:len(want)] != want or set(ids[len(want):]) & set(want) or (not adds and len(ids) != len(want)):
            return "want ids %r%s, got %r" % (want[:8], " first" if adds else "", ids[:len(want) + 4][:12])
    return None
