"""Inputs of the path-lookup tests that the CPU build of the walk
(test_tget_walk_host.py) and the GPU tests (test_gpu_tget_deep.py) share:
container chains that count skip frames, string keys around the 16-byte compare
window, integer keys at the edges of their widths, and a way to run the
recursive checker (tgetref.py) on inputs nested to MaxSkipDepth."""
import struct
import sys
import threading

import tgetref as R

F, I, S, N, B = R.FIELD, R.INDEX, R.STRKEY, R.INTKEY, R.BINKEY
LDS_FRAMES = 8  # TG_LDS_DEPTH (dynamicgo_amd/csrc/tget_device.h): a skip that opens more is a deep pair
KINDS, LEAVES = "SLEMK", "islme"


def _wstr(s: bytes) -> bytes:
    return struct.pack(">i", len(s)) + s


def _leaf(leaf):
    if leaf == "i":
        return R.I32, struct.pack(">i", 7)
    if leaf == "s":
        return R.STRING, _wstr(b"leaf")
    if leaf == "l":  # list<i64> of 2: a multiplication, no frame
        return R.LIST, struct.pack(">bi", R.I64, 2) + struct.pack(">qq", 1, -1)
    if leaf == "m":  # map<i32, double> of 1: a multiplication, no frame
        return R.MAP, struct.pack(">bbi", R.I32, R.DOUBLE, 1) + struct.pack(">id", 3, 0.5)
    if leaf == "e":  # list<string>: one frame
        return R.LIST, struct.pack(">bi", R.STRING, 2) + _wstr(b"") + _wstr(b"xy")
    raise ValueError(leaf)


def chain_message(kinds: str, leaf: str) -> bytes:
    """struct{1: <chain>, 2: i32 9}; the chain wraps the leaf in len(kinds)
    containers of one element each, kinds[0] the outermost: S struct (field 1),
    L list, E set, M map<string, X> with the key "k", K map<X, i32> with the
    chain as the key."""
    t, v = _leaf(leaf)
    for k in reversed(kinds):
        if k == "S":
            t, v = R.STRUCT, struct.pack(">bh", t, 1) + v + b"\x00"
        elif k == "L":
            t, v = R.LIST, struct.pack(">bi", t, 1) + v
        elif k == "E":
            t, v = R.SET, struct.pack(">bi", t, 1) + v
        elif k == "M":
            t, v = R.MAP, struct.pack(">bbi", R.STRING, t, 1) + _wstr(b"k") + v
        elif k == "K":
            t, v = R.MAP, struct.pack(">bbi", t, R.I32, 1) + v + struct.pack(">i", 5)
        else:
            raise ValueError(k)
    return struct.pack(">bh", t, 1) + v + struct.pack(">bhi", R.I32, 2, 9) + b"\x00"


CHAIN_PATHS = [[], [(F, 1)], [(F, 2)], [(F, 3)]]


def chain_frames(kinds: str, leaf: str, path) -> int:
    """How many skip frames are open at once at most while `path` (one of
    CHAIN_PATHS) is looked up in chain_message(kinds, leaf), as skipType
    (binary_skip.go:109-204) nests: one per container of the chain, one more
    for leaf e, one more for the top struct under the empty path; a list, set
    or K map straight over leaf i reduces to a multiplication and opens none."""
    n = len(kinds) + (leaf == "e") - (leaf == "i" and kinds[-1:] in ("L", "E", "K"))
    return n + (len(path) == 0)


def random_chain(rng, depth: int):
    return "".join(rng.choice(KINDS) for _ in range(depth)), rng.choice(LEAVES)


# the 16-step path: field 1 of the top struct, then one step per container of SIXTEEN_KINDS
SIXTEEN_KINDS = "SLM" * 5
SIXTEEN_PATH = [(F, 1)] + [{"S": (F, 1), "L": (I, 0), "M": (S, b"k")}[k] for k in SIXTEEN_KINDS]


def sixteen_step_inputs():
    """The 16-step path and its prefixes over a chain that ends where the path
    does (little left to skip) and one that goes on for 10 more lists (more than
    8 frames left after the descent), whole and cut short twice."""
    short = chain_message(SIXTEEN_KINDS, "e")
    long_ = chain_message(SIXTEEN_KINDS + "L" * 10, "e")
    msgs = [short, long_, short[:len(short) // 2], short[:-9], long_[:len(long_) // 2], long_[:-14]]
    return msgs, [SIXTEEN_PATH[:n] for n in (16, 15, 13, 10, 8, 7, 3, 1)]


# ---------------------------------------------------------------- string keys
KEY_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100)
KEYS = [bytes(65 + (7 * i + j) % 26 for j in range(n)) for i, n in enumerate(KEY_LENGTHS)]
EXACT, LAST, LONGER, SHORTER, BYTE8 = range(5)  # how a key enters a message


def key_variant(key: bytes, v: int):
    """The key as variant v, None where the key is too short to have it."""
    if v == EXACT:
        return key
    if v == LAST:
        return key[:-1] + bytes([key[-1] ^ 0xFF]) if key else None
    if v == LONGER:
        return key + b"Z"
    if v == SHORTER:
        return key[:-1] if key else None
    if v == BYTE8:
        return key[:8] + bytes([key[8] ^ 0x80]) + key[9:] if len(key) > 9 else None
    raise ValueError(v)


def long_key_messages(rng, n):
    """n messages struct{1: map<string, i32>} and, per message, the variant
    each of KEYS went in as (None = left out)."""
    msgs, how = [], []
    for _ in range(n):
        ents, vs = [], []
        for key in KEYS:
            r = rng.random()
            v = EXACT if r < 0.4 else LAST if r < 0.6 else LONGER if r < 0.7 else SHORTER if r < 0.8 else \
                BYTE8 if r < 0.9 else None
            k = key_variant(key, v) if v is not None else None
            vs.append(v if k is not None else None)
            if k is not None:
                ents.append(_wstr(k) + struct.pack(">i", rng.randrange(-99, 99)))
        rng.shuffle(ents)
        msgs.append(struct.pack(">bhbbi", R.MAP, 1, R.STRING, R.I32, len(ents)) + b"".join(ents) + b"\x00")
        how.append(vs)
    return msgs, how


def long_key_paths(prefix=((F, 1),)):
    """The 24 key paths in three sets of eight: every key as STRKEY, then as BINKEY."""
    ps = [list(prefix) + [(S, k)] for k in KEYS] + [list(prefix) + [(B, _wstr(k))] for k in KEYS]
    return [ps[0:8], ps[8:16], ps[16:24]]


# --------------------------------------------------------------- integer keys
INT_KEY_SETS = (
    (R.BYTE, ">b", (0, 127, -128, -1, 1)),
    (R.I16, ">h", (-32768, 32767, -1, 255, 256)),
    (R.I32, ">i", (-2 ** 31, 2 ** 31 - 1, -1, 65536, 255)),
    (R.I64, ">q", (-2 ** 63, 2 ** 63 - 1, -1, 2 ** 32, 2 ** 32 + 1, 1)),
)
INT_LOOKUPS = sorted({k for _, _, ks in INT_KEY_SETS for k in ks} | {128, 255, 65535, 2 ** 31, 2 ** 32 - 1})


def int_key_messages(rng, n):
    """n messages struct{1: map<i8, string>, 2: map<i16, string>, 3: map<i32,
    string>, 4: map<i64, string>}, each edge key kept with p = 0.6."""
    msgs = []
    for _ in range(n):
        out = bytearray()
        for fid, (kt, fmt, keys) in enumerate(INT_KEY_SETS, 1):
            ks = [k for k in keys if rng.random() < 0.6]
            rng.shuffle(ks)
            out += struct.pack(">bhbbi", R.MAP, fid, kt, R.STRING, len(ks))
            for k in ks:
                out += struct.pack(fmt, k) + _wstr(b"v%d" % (k & 0xFF))
        out.append(0)
        msgs.append(bytes(out))
    return msgs


def int_key_paths():
    """Every map looked up with every value of INT_LOOKUPS, eight paths a set."""
    ps = [[(F, fid), (N, v)] for fid in range(1, 5) for v in INT_LOOKUPS]
    return [ps[i:i + 8] for i in range(0, len(ps), 8)]


def write_corpus(path, msgs, blob: bytes, root_type: int = R.STRUCT):
    """The file tget_walk_host.cpp's stand-alone program (-DWALK_MAIN) reads: u32
    n_msgs, n_paths, root_type, off_steps, off_pool, blob length; the path-set
    blob (generic.compile_paths); per message a u32 length and the bytes."""
    n_paths, _, off_steps, off_pool = struct.unpack_from("<4I", blob, 12)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<6I", len(msgs), n_paths, root_type, off_steps, off_pool, len(blob)) + blob)
        for m in msgs:
            fh.write(struct.pack("<I", len(m)) + m)


# ------------------------------------------------------------------- checker
def deep_checker(fn):
    """fn() in a thread with a large stack and a raised recursion limit: the
    checker's skipType recurses per list, set and map level as the Go does, and
    1023 of them do not fit Python's defaults. Both are put back afterwards."""
    box = {}

    def run():
        try:
            box["v"] = fn()
        except BaseException as e:  # handed to the caller's thread
            box["e"] = e

    old_limit, old_stack = sys.getrecursionlimit(), threading.stack_size(512 << 20)
    sys.setrecursionlimit(20000)
    try:
        t = threading.Thread(target=run)
        t.start()
        t.join()
    finally:
        sys.setrecursionlimit(old_limit)
        threading.stack_size(old_stack)
    if "e" in box:
        raise box["e"]
    return box["v"]
