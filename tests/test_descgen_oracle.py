"""CPU: the descriptor families of descgen.py against the two CPU checkers.

For every family and every flag word the compiled reference (when built), the
C restatement and the intent descgen states for the message agree, message by
message: no family can quietly turn into a batch of errors, and no share of
the cases is left out. The shapes the families promise -- table sizes, probe
chains that wrap, struct indices, blob sizes, field flags -- are read back from
the flattened blob here."""
import pytest

import descgen as G
import oracle
from dynamicgo_amd import thrift as T


def checkers():
    out = [("port", oracle.PortOracle())]
    ref = oracle.RefOracle()
    if ref is not None:
        out.insert(0, ("ref", ref))
    return out


def agree(case, flag_words=G.FLAG_WORDS):
    """Every checker's verdict on every message is the intent's, and the
    checkers give the same bytes."""
    bad = []
    for flags in flag_words:
        results = []
        for name, chk in checkers():
            rets, outs = chk.j2t_batch(case.flat, case.msgs, flags)
            results.append((rets, outs))
            for i, (m, it) in enumerate(zip(case.msgs, case.intents)):
                why = G.check_intent(it, flags, int(rets[i]), outs[i])
                if why:
                    bad.append((case.name, name, hex(flags), i, m[:80], it.kind, why))
        if len(results) == 2:
            for i in range(len(case.msgs)):
                if int(results[0][0][i]) != int(results[1][0][i]) or results[0][1][i] != results[1][1][i]:
                    bad.append((case.name, "ref != port", hex(flags), i, case.msgs[i][:80]))
    return bad


def kinds(case):
    return {it.kind for it in case.intents}


@pytest.fixture(scope="module")
def names():
    return G.names_family()


def test_names_family(names):
    cases, pairs = names
    assert len(pairs) >= 3
    for a, b in pairs:
        assert a != b and len(a) == len(b) and T.name_hash(a) == T.name_hash(b)
    assert {len(a) for a, _ in pairs} >= {2, 10, 16}
    sizes = {c.name: len(G.blob_names(c.flat.blob, 0)) for c in cases}
    assert sizes == {"N1": 2, "N16": 32, "N17": 64, "NL": 128}
    for c in cases:
        keys = [s[1] for s in G.blob_names(c.flat.blob, 0) if s]
        assert len(keys) == c.props["n_names"]
        if c.name != "N1":
            assert {len(k) for k in keys} >= set(G.SEAMS), c.name
            longest, wraps = G.probe_chains(c.flat.blob, 0)
            assert longest >= 3 and wraps, (c.name, longest, wraps)
            hashes = [s[0] for s in G.blob_names(c.flat.blob, 0) if s]
            assert len(set(hashes)) < len(hashes), c.name  # two names, one full hash
        assert kinds(c) == {G.HIT, G.UNKNOWN}
        assert any(it.escaped for it in c.intents)
        for n in c.props.get("nul_proof", ())[:1]:  # name NUL NUL: the name's hash, slot and pool word, and no field
            assert T.name_hash(n + bytes(2)) == T.name_hash(n) and len(n) + 2 <= 8
            assert [it.kind for m, it in zip(c.msgs, c.intents) if m.startswith(b'{"' + n + bytes(2) + b'"')] == [G.UNKNOWN]
        bad = agree(c)
        assert not bad, (len(bad), bad[:5])
    nl = cases[-1]
    assert {len(s[1]) for s in G.blob_names(nl.flat.blob, 0) if s} >= set(range(41))
    # a name that is a prefix of another, and the name one byte longer, are both asked
    n17 = cases[2]
    assert any(it.kind == G.HIT and m.startswith(b'{"pre":') for m, it in zip(n17.msgs, n17.intents))
    assert any(it.kind == G.UNKNOWN and m.startswith(b'{"prefi":') for m, it in zip(n17.msgs, n17.intents))


def test_aliases_family():
    (c,) = G.aliases_family()
    blob = c.flat.blob
    fb, nf = G.blob_struct(blob, 0)[:2]
    for k in range(nf):
        fid, _, fl = G.blob_field(blob, fb + k)[:3]
        if fid in c.props["alias_self"]:
            assert bool(fl & 4) == c.props["alias_self"][fid], fid
        if fid in c.props["key_plain"]:
            assert bool(fl & 8) == c.props["key_plain"][fid], fid
    sd = c.td.struct
    assert sd.names["alpha"].id == 2 and sd.names["ALPHA"].id == 1 and sd.names["shared"].id == 4
    assert sd.names["zeta"].id == 6 and sd.names["gamma"].id == 3 and sd.names["eps"].id == 5
    hit_ids = {it.ids[0] for it in c.intents if it.kind == G.HIT}
    assert hit_ids == {f.id for f in sd.fields}
    assert {it.ids[0] for it in c.intents if it.kind == G.HIT and it.escaped} >= {7, 8, 9, 11, 12, 13}
    assert kinds(c) == {G.HIT, G.UNKNOWN}
    bad = agree(c)
    assert not bad, (len(bad), bad[:5])


def test_ids_family():
    (c,) = G.ids_family()
    blob = c.flat.blob
    fb, nf = G.blob_struct(blob, 0)[:2]
    assert [G.blob_field(blob, fb + k)[0] for k in range(nf)] == sorted(G.IDS)
    assert list(G.DECL) != sorted(G.DECL) and set(G.DECL) == set(G.IDS)
    assert sum(it.kind == G.HIT and len(it.ids) == len(G.IDS) for it in c.intents) == 4
    bad = agree(c)
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("form", G.FORMS)
def test_counts_family(form):
    for c in G.counts_family((form,)):
        n = c.props["n"]
        blob = c.flat.blob
        wide = [si for si in range(G.blob_hdr(blob).n_structs) if G.blob_struct(blob, si)[1] == n]
        assert wide, c.name
        assert G.blob_struct(blob, wide[0])[5] == (n + 63) // 64  # req_words
        reqs = [f.required for f in sorted(c.props["wide"].fields, key=lambda f: f.id)]
        ph = c.props["phase"]
        assert reqs == [T.OPTIONAL if form == "self" and k == 0 else G.REQ_CYCLE[(k + ph) % 3] for k in range(n)]
        if ph:  # the struct whose field index 63 is REQUIRED, and a message that lacks exactly it
            assert n == 64 and reqs[63] == T.REQUIRED
            assert any(it.kind == G.MISSING and it.ids == (64,) for it in c.intents)
        assert G.HIT in kinds(c) and (n < 3 or G.MISSING in kinds(c)), c.name
        bad = agree(c)
        assert not bad, (c.name, len(bad), bad[:5])


def test_reqarena_family():
    c = G.reqarena_case()
    fit, w = c.props["fit"], c.props["req_words"]
    assert G.blob_struct(c.flat.blob, 0)[5] == w
    assert fit * w == G.kernel_const("j2t_machine.h", "WS_REQCAP")
    assert fit + 2 < G.kernel_const("j2t_machine.h", "LDS_DEPTH")
    assert {it.depth for it in c.intents} >= {fit, fit + 1, fit + 2}
    # F_WRITE_DEFAULT (0x3, 0x83, 0xa3) walks the 64-word bitmap of every open level for its unset DEFAULT fields
    sd = c.td.struct
    assert sum(f.required == T.DEFAULT for f in sd.fields) == (c.props["n"] - 1) // 2 and sd.fields[-1].required == T.REQUIRED
    chk = checkers()[0][1]
    assert max(map(len, chk.j2t_batch(c.flat, c.msgs, 0x3)[1])) > 7 * 2016 * fit
    bad = agree(c)
    assert not bad, (len(bad), bad[:5])


def test_structs_family():
    c = G.structs_case()
    blob = c.flat.blob
    h = G.blob_hdr(blob)
    assert h.n_structs == G.CHAIN >= 70 and h.total_len <= 16384
    assert h.total_len <= G.kernel_const("j2t_wave.h", "WV_DESC")
    assert G.kernel_const("j2t_wave.h", "WV_REQMASKS") == 64
    # struct k's field "n" is of the type whose struct is k + 1; "r" is REQUIRED in every struct
    for k in range(G.CHAIN):
        fb, nf = G.blob_struct(blob, k)[:2]
        fields = [G.blob_field(blob, fb + j) for j in range(nf)]
        assert [f[0] for f in fields][:2] == ([1, 2] if k + 1 < G.CHAIN else [2, 3])
        r = next(f for f in fields if f[0] == 2)
        assert r[1] == T.REQUIRED
        if k + 1 < G.CHAIN:
            assert G.blob_type(blob, fields[0][5])[5] == k + 1
    assert G.blob_type(blob, h.root_type)[5] == 0
    for lvl in (62, 63, 64, 65):  # struct index lvl: its REQUIRED field missing as the innermost struct and inside, and present
        at = [it.depth for it, m in zip(c.intents, c.props["missing_at"]) if m == lvl]
        assert lvl + 1 in at and max(at) > lvl + 1 and all(it.kind == G.MISSING for it, m in
                                                           zip(c.intents, c.props["missing_at"]) if m == lvl)
        assert sum(it.kind == G.HIT and it.depth == lvl + 1 for it in c.intents) == 1
    bad = agree(c)
    assert not bad, (len(bad), bad[:5])


def test_tree_family():
    c = G.tree_case()
    blob = c.flat.blob
    h = G.blob_hdr(blob)
    assert h.n_structs == 81 and h.total_len <= G.kernel_const("j2t_wave.h", "WV_DESC")
    # the blob index of every leaf struct, through the types table
    index = {}
    for ti in range(h.n_types):
        t = G.blob_type(blob, ti)
        if t[0] == T.STRUCT and G.blob_struct(blob, t[5])[1] == 1:
            index[id(c.flat.types[ti].struct)] = t[5]
    at = {kj: index[id(td.struct)] for kj, td in c.props["leaves"].items()}
    assert len(set(at.values())) == 72 and set(at.values()) >= {62, 63, 64, 65, 66}
    for si in (62, 63, 64, 65, 66):  # present and missing in each, at depth 3
        ks = [it.kind for it, kj in zip(c.intents, c.props["leaf_of"]) if at[kj] == si]
        assert ks == [G.HIT, G.MISSING], (si, ks)
    bad = agree(c)
    assert not bad, (len(bad), bad[:5])


def test_sizes_family():
    cases = G.sizes_family()
    assert [G.blob_hdr(c.flat.blob).total_len for c in cases] == list(G.SIZE_TARGETS)
    for name, hdr, const in (("SM_DESC", "j2t_small.h", 12288), ("FL_DESC", "j2t_flat.h", 16384),
                             ("WV_DESC", "j2t_wave.h", 16384), ("DESC_LDS_BYTES", "j2t_machine.h", 49152)):
        assert G.kernel_const(hdr, name) == const and const in G.SIZE_EDGES
    first = None
    for c in cases:
        assert len(c.flat.blob) == c.props["total_len"]
        assert G.blob_struct(c.flat.blob, 0)[1] == len(G.LIVE) + G.N_PAD <= 64
        assert kinds(c) == {G.HIT, G.UNKNOWN, G.MISSING}
    # the intents once (the batch is the same), the bytes at every size
    bad = agree(cases[0])
    assert not bad, (len(bad), bad[:5])
    chk = checkers()[0][1]
    for flags in G.FLAG_WORDS:
        for c in cases:
            rets, outs = chk.j2t_batch(c.flat, c.msgs, flags)
            got = ([int(r) for r in rets], outs)
            if first is None or first[0] != flags:
                first = (flags, got)
            assert got == first[1], (c.name, hex(flags))


def test_t2j_messages_cover_orders_and_unknown_ids():
    sd = G.ids_desc().struct
    msgs = G.t2j_messages(sd)
    assert len(set(msgs)) >= 40
    ids = [[f for f in G.thrift_structs(m)[0][1]] for m in msgs]
    assert sorted(G.IDS) in ids and sorted(G.IDS, reverse=True) in ids
    assert any(sorted(i) == sorted(G.IDS) and i not in (sorted(G.IDS), sorted(G.IDS, reverse=True)) for i in ids)
    seen = {i for row in ids for i in row}
    assert {0, 0x8000, 0xFFFF, 126, 129, 257} <= seen
    # 0x7FFF is a field of Ids, so it is unknown only where the struct has no
    # such id: beside the fields of a wide struct
    wide = G.wide_struct(65, "W65")[0].struct
    rows = [G.thrift_structs(m)[0][1] for m in G.t2j_messages(wide)]
    assert 0x7FFF not in wide.ids and {0, 0x7FFF, 0x8000, 0xFFFF, 66} <= {i for row in rows for i in row}
