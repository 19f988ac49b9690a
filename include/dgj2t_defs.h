/*
 * dgj2t_defs.h — the constants of the C ABI (include/dgj2t.h): the
 * reference's j2t flag word, the library's per-message statuses and the API
 * error codes. Split out so the device code includes only these.
 */
#ifndef DGJ2T_DEFS_H
#define DGJ2T_DEFS_H

/* j2t flag bits (reference native/thrift.h:23-32) */
#define DG_F_ALLOW_UNKNOWN (1ull << 0)
#define DG_F_WRITE_DEFAULT (1ull << 1)
#define DG_F_ENABLE_VM (1ull << 2)
#define DG_F_ENABLE_HM (1ull << 3)
#define DG_F_ENABLE_I2S (1ull << 4)
#define DG_F_WRITE_REQUIRE (1ull << 5)
#define DG_F_NO_BASE64 (1ull << 6)
#define DG_F_WRITE_OPTIONAL (1ull << 7)
#define DG_F_TRACE_BACK (1ull << 8)
#define DG_F_NO_WRITE_BASE (1ull << 9)
#define DG_F_VALIDATE_UTF8 (1ull << 16) /* extension: reject invalid UTF-8 in strings */
#define DG_F_NO_FAST_PATH (1ull << 17)  /* extension: run every message on the exact machine (testing) */
#define DG_F_NO_WAVE_PATH (1ull << 18)  /* extension: skip the wave-per-message kernel, lane kernel only (testing) */
#define DG_F_FLAT_PATH (1ull << 19)     /* extension: force the field-major flat kernel (j2t_flat.h) for a flat root
                                           struct (the default whenever the batch's messages are <= 256 B) */
#define DG_F_HM_SPLIT (1ull << 20)      /* extension, with F_ENABLE_HM: the host has already run handleHttpMappings
                                           (conv/j2t/impl.go:243-292) for the ROOT struct; the root raises no ERR_HM,
                                           the mapped fields the host wrote (all of them, or those of the per-message
                                           mask of dg_j2t_batch_*_hm) count as set and their JSON keys are skipped
                                           (native/thrift.c:725), the others are read from the body
                                           (ReadHttpValueFallback). The output is the body part: the host puts its
                                           mapped-field bytes in front. Nested structs with mapped fields still
                                           return ERR_HM. */
#define DG_F_NO_FLAT_PATH (1ull << 21)  /* extension: lane-per-message small kernel even for a flat root (testing) */
#define DG_F_CB_COLLECT (1ull << 22)    /* extension: at a callback the host must serve (ERR_VM_END, a nested
                                           ERR_HM_END, see dg_cb_entry) the machine records it and converts on
                                           instead of stopping; the message ends with DG_ST_CB_LIST and every
                                           callback of one pass recorded, so k callbacks take 2 passes, not k + 1 */

/* library-internal per-message statuses (code byte values the reference never
 * produces). The host entry points resolve them before returning; the device
 * entry point leaves them for the caller and counts them in *d_pending. */
#define DG_ST_OUT_OVERFLOW 0xF0u /* slot too small; out_len = bytes needed (value bits: same, saturated at 2^24-1) */
#define DG_ST_DEEP 0xF1u         /* (internal) nesting beyond the fast kernel's stack */
#define DG_ST_HM_END 0xF2u       /* DG_F_HM_SPLIT + F_TRACE_BACK: the ROOT's ERR_HM_END (native/thrift.c:898-903)
                                    for the host to serve (handleUnmatchedFields, conv/j2t/impl_amd64.go:71-115):
                                    out_len covers the output so far followed by the root's remaining requires
                                    words (big-endian u64, `value` of them); the host appends the cached fields'
                                    bytes and the STOP */
#define DG_ST_HM_END_AT 0xF4u    /* a nested struct's ERR_HM_END for the host (dg_cb_entry) */
#define DG_ST_CB_LIST 0xF5u      /* DG_F_CB_COLLECT: `value` callbacks recorded in the slot, in the order the
                                    message meets them (out_len bytes): each is the status word the stop would
                                    have returned (big-endian u64: code 24 or DG_ST_HM_END_AT, its pos and value)
                                    followed by that stop's record (dg_cb_entry). The host answers them in order
                                    and converts the message again with the answers; an error met after a
                                    callback is reported by that pass, as the reference reports it after Go
                                    served the callback. */
#define DG_ST_HM_ERR 0xF3u       /* DG_F_HM_SPLIT: the message opened a struct whose HTTP-mapping entry is an
                                    error (dg_hm_entry.len == DG_HM_ERR): handleHttpMappings failed for it on the
                                    host; value = the entry's slot, pos = the struct's '{' */

/* HTTP-mapping table of dg_j2t_batch_*_hm: per message, one entry per struct
 * of the descriptor with HTTP-mapped fields (slot j = the j-th such struct in
 * blob order): the bytes the host's handleHttpMappings (conv/j2t/impl.go:
 * 243-292) writes for that struct, at hm_bytes[off, off + len), and the mask
 * of its mapped fields it wrote (bit k = the struct's k-th field in id order;
 * an unset bit = reqs.Set(id, Required), read from the body:
 * ReadHttpValueFallback). len == DG_HM_ERR: the host failed (DG_ST_HM_ERR). */
typedef struct dg_hm_entry {
    uint32_t off;
    uint32_t len;
    uint64_t mask;
} dg_hm_entry;
#define DG_HM_ERR 0xFFFFFFFFu

/* Callbacks the reference returns to its Go host mid-message and resumes
 * after (handleError, conv/j2t/impl_amd64.go:169-247), served here by
 * converting the message again with the host's answers:
 *  - ERR_VM_END (native/thrift.c:641-665): a non-inline value mapping (a
 *    value-mapping type above DG_VM_INLINE_MAX under F_ENABLE_VM; the device
 *    serves DG_VM_BODY_DYNAMIC on a STRING field itself). The host writes the
 *    field header and runs the annotation's ValueMapping.Write on the value's
 *    JSON text (handleValueMapping, impl_amd64.go:117-155).
 *  - ERR_HM_END (native/thrift.c:898-903,952-957) of a NESTED struct under
 *    DG_F_HM_SPLIT + F_TRACE_BACK (the root's is DG_ST_HM_END): the host
 *    writes the cached fields from the request, then STOP
 *    (handleUnmatchedFields, impl_amd64.go:71-115).
 * Per message one dg_cb_entry: `count` answers at bytes[off..], in the order
 * the message meets the callbacks, each a u32 little-endian length and that
 * many bytes. The (count+1)-th callback stops the message:
 *  - ERR_VM_END: status code 24, pos = the value's end (as the reference packs
 *    it); out_len 16: the value's start and the field's descriptor index, two
 *    big-endian u64.
 *  - nested ERR_HM_END: status DG_ST_HM_END_AT (below), value = w, pos = the
 *    position after the '}'; out_len 8 + 8w: the struct's descriptor index,
 *    then w big-endian u64 words whose set bits are the cached fields (bit k =
 *    the struct's k-th field in id order). */
typedef struct dg_cb_entry {
    uint32_t off;
    uint32_t count;
} dg_cb_entry;

/* The host's answers to the reference's Go callbacks for one batch
 * (dg_j2t_batch_*_cb): HTTP-mapping entries (n_hm per message, see
 * dg_hm_entry; hm_tab NULL: none) and callback answers (one dg_cb_entry per
 * message; ans_tab NULL: none), both pointing into `bytes` (len bytes). */
typedef struct dg_cb_tables {
    const dg_hm_entry *hm_tab;
    uint32_t n_hm;
    const dg_cb_entry *ans_tab;
    const uint8_t *bytes;
    uint64_t len;
} dg_cb_tables;

/* API error codes */
#define DG_OK 0
#define DG_E_INVALID (-1)
#define DG_E_HIP (-2)
#define DG_E_NOMEM (-3)
#define DG_E_DESC (-4)
#define DG_E_AGAIN (-5) /* dg_agg_submit(nonblock): no open batch right now */
#define DG_E_ARG (-6)   /* a path-set blob that breaks the layout or a limit below */

/* tget (batched GetByPath, include/dgj2t.h): per-record statuses */
#define DG_TGET_OK 0
#define DG_TGET_NOT_FOUND 1 /* errNotFound */
#define DG_TGET_E_READ 2    /* meta.ErrRead */
#define DG_TGET_E_TYPE 3    /* meta.ErrDismatchType */

/* Path-set blob: everything little-endian, tables 8-aligned.
 *
 *   offset 0             dg_path_hdr (32 bytes)
 *   offset 32            n_paths x dg_path_ent (8 bytes each)
 *   offset off_steps     n_steps x dg_path_step (16 bytes each)
 *   offset off_pool      pool_len key bytes (STRKEY / BINKEY), unpadded and
 *                        back to back; the pool is the blob's last part
 *   total_len            = off_pool + pool_len, at most the length passed
 *
 * Path k owns steps [first, first + count) of the step table; count may be 0
 * (the empty path: the whole top value). Limits: 1 <= n_paths <=
 * DG_TGET_MAX_PATHS; count <= DG_TGET_MAX_STEPS; first + count <= n_steps;
 * off_steps >= 32 + 8 n_paths; off_steps and off_pool multiples of 8;
 * off_steps + 16 n_steps <= off_pool.
 * A step, by kind (the reference's PathType of the same name):
 *   DG_PS_FIELD   val = the field id, -32768..32767        (PathFieldId)
 *   DG_PS_INDEX   val = the index, >= 0                     (PathIndex)
 *   DG_PS_STRKEY  key bytes pool[val, val + key_len)        (PathStrKey)
 *   DG_PS_INTKEY  val = the key, any int64                  (PathIntKey)
 *   DG_PS_BINKEY  key bytes pool[val, val + key_len): the key's Thrift-binary
 *                 encoding as it stands in the message      (PathBinKey)
 * key_len is 0 for the other kinds; val + key_len <= pool_len for keys.
 * PathFieldName has no wire form: the host resolves names to ids through the
 * IDL first, as Value.GetByPath does (thrift/generic/value.go:123-131). */
#define DG_PATH_MAGIC 0x31504744u /* "DGP1" */
#define DG_PATH_VERSION 1u
#define DG_TGET_MAX_PATHS 8u
#define DG_TGET_MAX_STEPS 16u
#define DG_PS_FIELD 1u
#define DG_PS_INDEX 2u
#define DG_PS_STRKEY 3u
#define DG_PS_INTKEY 4u
#define DG_PS_BINKEY 5u
typedef struct dg_path_hdr {
    uint32_t magic, version, total_len, n_paths, n_steps, off_steps, off_pool, pool_len;
} dg_path_hdr;
typedef struct dg_path_ent {
    uint32_t first, count;
} dg_path_ent;
typedef struct dg_path_step {
    uint32_t kind, key_len;
    int64_t val;
} dg_path_step;

/* cut (batched MarshalTo, include/dgj2t.h dg_cut_*): option bits (the
 * thrift/generic Options fields marshalTo reads) and per-message statuses */
#define DG_CUT_WRITE_DEFAULT (1ull << 0)    /* WriteDefault */
#define DG_CUT_DISALLOW_UNKNOWN (1ull << 1) /* DisallowUnknow */
#define DG_CUT_NOT_CHECK_REQ (1ull << 2)    /* NotCheckRequireNess */
#define DG_CUT_OK 0u
#define DG_CUT_E_READ 1u         /* meta.ErrRead */
#define DG_CUT_E_TYPE 2u         /* meta.ErrDismatchType */
#define DG_CUT_E_UNKNOWN 3u      /* meta.ErrUnknownField */
#define DG_CUT_E_REQUIRED 4u     /* meta.ErrMissRequiredField */
#define DG_CUT_E_DEPTH 5u        /* more than DG_CUT_MAX_DEPTH cut containers open (no reference counterpart) */
#define DG_CUT_E_OVERFLOW 0xF0u  /* slot too small (the value of DG_ST_OUT_OVERFLOW) */
#define DG_CUT_MAX_DEPTH 64u

/* Cut-plan blob (generic.compile_cut): everything little-endian, tables
 * 8-aligned, the pool last; the device copy has 16 zero bytes after it.
 *
 *   offset 0           dg_cut_hdr (64 bytes)
 *   offset off_nodes   n_nodes x dg_cut_node (40 bytes each)
 *   offset off_fields  n_fields x dg_cut_field (8 bytes each)
 *   offset off_lits    n_lits x dg_cut_lit (8 bytes each)
 *   offset off_pool    pool_len literal bytes
 *   total_len          = off_pool + pool_len
 *
 * A node is one (from, to) descriptor pair; `root` is the pair the messages
 * start with. By kind:
 *   DG_CUT_COPY      a = the descriptor's type: SkipType(a), the span copied
 *   DG_CUT_MISMATCH  ErrDismatchType when a value of this pair is reached
 *   DG_CUT_LIST      a = the element's node (LIST and SET)
 *   DG_CUT_MAP       a = the key's node, b = the element's node
 *   DG_CUT_STRUCT    fields [a, a + n_fields) of the field table, sorted by
 *                    id, one per field of `from` (an id not among them is
 *                    unknown); lits [lit0, lit0 + n_lits): one entry per
 *                    tracked field of `to` (RequiresBitmap bit set), ascending
 *                    id, entry k = bit k of `tracked`, the mask a struct
 *                    instance starts with; `required` = the bits whose field is
 *                    Required. n_lits <= 64.
 * A field: the wire type `from` declares (another one in the message is
 * ErrDismatchType), child = the node of the (from, to) field types or
 * DG_CUT_DROP when `to` lacks the id, bit = the field's bit in the masks or
 * DG_CUT_NO_BIT. A lit: the field id and, for a field that is not Required,
 * pool[off, off + len) = its field header + WriteEmpty of its type (what
 * WriteDefault emits while the bit is still set at STOP); len 0 for Required.
 * max_unset = the largest total of a struct's lit lengths. */
#define DG_CUT_MAGIC 0x31434744u /* "DGC1" */
#define DG_CUT_VERSION 1u
#define DG_CUT_COPY 1u
#define DG_CUT_MISMATCH 2u
#define DG_CUT_LIST 3u
#define DG_CUT_MAP 4u
#define DG_CUT_STRUCT 5u
#define DG_CUT_DROP 0xFFFFFFFFu
#define DG_CUT_NO_BIT 0xFFu
typedef struct dg_cut_hdr {
    uint32_t magic, version, total_len, root, n_nodes, off_nodes, n_fields, off_fields, n_lits, off_lits, off_pool,
        pool_len, max_unset, pad[3];
} dg_cut_hdr;
typedef struct dg_cut_node {
    uint32_t kind, a, b, n_fields, lit0, n_lits;
    uint64_t tracked, required;
} dg_cut_node;
typedef struct dg_cut_field {
    int16_t id;
    uint8_t type, bit;
    uint32_t child;
} dg_cut_field;
typedef struct dg_cut_lit {
    int16_t id;
    uint16_t len;
    uint32_t off;
} dg_cut_lit;

/* edit (batched SetByPath / UnsetByPath, include/dgj2t.h dg_edit_*): the two
 * ops and the per-message return word, status (bits 0-7, tget's numbers) |
 * DG_EDIT_EXISTED | aux << 32 */
#define DG_EDIT_SET 1u
#define DG_EDIT_UNSET 2u
#define DG_EDIT_OK 0u
#define DG_EDIT_NOT_FOUND 1u      /* meta.ErrNotFound */
#define DG_EDIT_E_READ 2u         /* meta.ErrRead */
#define DG_EDIT_E_TYPE 3u         /* meta.ErrDismatchType */
#define DG_EDIT_E_OVERFLOW 0xF0u  /* slot too small (the value of DG_ST_OUT_OVERFLOW) */
#define DG_EDIT_EXISTED (1ull << 8) /* the path was there: a replace or a delete, not an insert or a no-op */

/* editm (batched SetMany, include/dgj2t.h dg_editm_*): up to DG_EDITM_MAX_ITEMS
 * last steps below one parent path in one edit, so that parent + items are one
 * path set. The return word is status | existed mask << 8 (bit 8 + j: item j was
 * a replace or a drop) | failing item << 16 (3 bits, 0 when OK) | aux << 32 */
#define DG_EDITM_MAX_ITEMS (DG_TGET_MAX_PATHS - 1u)
#define DG_EDITM_E_SAME 5u /* two items resolve to overlapping spans of the message (4 is DG_KIDS_E_UNSUPPORTED) */

/* kids (batched Children, include/dgj2t.h dg_kids_*): the statuses a message
 * can have besides DG_TGET_OK / NOT_FOUND / E_READ / E_TYPE, the flags, and the
 * two records (little-endian, no padding) */
#define DG_KIDS_E_UNSUPPORTED 4u   /* meta.ErrUnsupportedType: the node is no struct, list, set or map */
#define DG_KIDS_E_OVERFLOW 0xF0u   /* the message's records would pass rec_cap (the value of DG_ST_OUT_OVERFLOW) */
#define DG_KIDS_F_RECURSE 1u       /* Children(recurse = true): the whole subtree, preorder */
#define DG_KIDS_F_COUNTED 2u       /* d_head / d_rec_off come from an earlier call: emit only */
#define DG_KIDS_NO_PARENT 0xFFFFFFFFu
typedef struct dg_kid_rec {
    uint32_t start, end; /* the child's value in the message */
    uint32_t key_start;  /* STRKEY: the key's bytes at key_start + 4; BINKEY: at key_start; a field: start - 3; an
                            element: start */
    uint32_t parent;     /* index, among this message's records, of the enclosing child; DG_KIDS_NO_PARENT for a
                            direct child */
    int64_t key;         /* field id, index or int key; STRKEY / BINKEY: the key's length */
    uint8_t type, kind;  /* wire type; DG_PS_FIELD / INDEX / STRKEY / INTKEY / BINKEY */
    uint16_t depth;      /* 1 = a direct child */
    uint32_t n_desc;     /* records in the subtree below this one (0 in one-level mode and for scalars) */
} dg_kid_rec; /* 32 bytes */
typedef struct dg_kids_head {
    uint32_t count;  /* records of the message, 0 unless DG_TGET_OK */
    uint32_t direct; /* direct children (Node.Len of a list, set or map); not OK: the failing step, the path's
                        length for a failure in the scan */
    uint32_t start;  /* where the node starts (OK and DG_KIDS_E_UNSUPPORTED / E_OVERFLOW) */
    uint8_t type, key_type, elem_type; /* the node's types; key and element types 0 for a struct */
    uint8_t status;
} dg_kids_head; /* 16 bytes */

/* cols (typed column reads, include/dgj2t.h dg_cols_*): a column's kind is
 * the cast behind the lookup; DG_COL_LIST | DG_COL_INT and DG_COL_LIST |
 * DG_COL_F64 are the two list kinds. A cell's status is the lookup's
 * (DG_TGET_*) or DG_COL_E_UNSUPPORTED. */
#define DG_COL_BOOL 1u  /* Node.Bool */
#define DG_COL_BYTE 2u  /* Node.Byte */
#define DG_COL_INT 3u   /* Node.Int */
#define DG_COL_F64 4u   /* Node.Float64 */
#define DG_COL_STR 5u   /* Node.String / Node.Binary */
#define DG_COL_LEN 6u   /* Node.Len */
#define DG_COL_LIST 16u /* Node.List, each element through Int or Float64 */
#define DG_COL_E_UNSUPPORTED 4u /* meta.ErrUnsupportedType: the cast does not take the wire type found (the value of
                                   DG_KIDS_E_UNSUPPORTED) */
typedef struct dg_col_cell {
    uint8_t status; /* DG_TGET_OK / NOT_FOUND / E_READ / E_TYPE or DG_COL_E_UNSUPPORTED */
    uint8_t type;   /* the wire type found (OK and E_UNSUPPORTED; an OK list cell: its element type); a failed lookup:
                       dg_tget_rec's type */
    uint16_t step;  /* dg_tget_rec's step */
    uint32_t aux;   /* dg_tget_rec's aux; a list whose element type the cast rejects: that element type */
} dg_col_cell; /* 8 bytes */

/* rows (row columns, include/dgj2t.h dg_rows_*): the elements of a list or set
 * as rows. A head's status is DG_TGET_OK / NOT_FOUND / E_READ / E_TYPE or
 * DG_COL_E_UNSUPPORTED; a cell is a dg_col_cell (little-endian, no padding). */
#define DG_ROWS_MAX_COLS 8u
typedef struct dg_rows_head {
    uint64_t first; /* OK: the arena offset of element 0 (the byte after the list header); else 0 */
    uint32_t count; /* OK: the node's element count (Node.Len), the message's rows; else 0 */
    uint8_t status;
    uint8_t type;      /* OK: LIST or SET; DG_COL_E_UNSUPPORTED: the wire type found; else 0 */
    uint8_t elem_type; /* OK: the element type, the root type of every row's lookup; else 0 */
    uint8_t step;      /* a failed lookup: the failing step; otherwise the parent path's length */
} dg_rows_head; /* 16 bytes */
typedef struct dg_row_ent {
    uint64_t off; /* the arena offset of the element's first byte */
    uint32_t len; /* the element's byte length */
    uint32_t msg; /* the message the row belongs to */
} dg_row_ent; /* 16 bytes */
/* The key kind of a map plan (dg_rows_create_map): the rows are the entries of
 * a map, the index entry is the VALUE's span, and each row has a key beside it.
 * Under a map plan an OK head's type is MAP, elem_type the value type and first
 * the arena offset of entry 0's key (the byte after the 6-byte header); a key
 * type the kind does not take is DG_COL_E_UNSUPPORTED with type = MAP and
 * elem_type = the key type found. */
#define DG_ROWS_KEY_STR 1u /* STRING keys: the payload's arena offset and length */
#define DG_ROWS_KEY_INT 2u /* I08 / I16 / I32 / I64 keys: the value as ReadInt gives it, and the width in bytes */

/* ents (entry columns, include/dgj2t.h dg_ents_*): Node.List with String per
 * element, Node.StrMap and Node.IntMap as ragged columns. A kind is
 * DG_ENT_LISTSTR, or DG_ENT_STRMAP / DG_ENT_INTMAP with the value kind in its
 * low four bits: DG_ENT_BOOL, DG_ENT_INT, DG_ENT_F64 or DG_ENT_STR (the numbers
 * of DG_COL_BOOL / INT / F64 / STR). A cell is a dg_col_cell; in the cells of a
 * map kind aux holds the header's type bytes: the key type in bits 0-7, the
 * value type in bits 8-15. */
#define DG_ENT_BOOL 1u
#define DG_ENT_INT 3u
#define DG_ENT_F64 4u
#define DG_ENT_STR 5u
#define DG_ENT_LISTSTR 0x15u /* for e in node.List(): e.String() */
#define DG_ENT_STRMAP 0x20u  /* Node.StrMap, | the value kind */
#define DG_ENT_INTMAP 0x40u  /* Node.IntMap, | the value kind */

/* vals (typed column writes, include/dgj2t.h dg_vals_*): a column's kind names
 * the wire encoding to write: a scalar kind is the Thrift wire type itself (2
 * BOOL, 3 I08, 4 DOUBLE, 6 I16, 8 I32, 10 I64, 11 STRING); DG_VAL_LIST | elem
 * and DG_VAL_SET | elem, elem one of 2, 3, 4, 6, 8, 10, are the container kinds.
 * A cell's status is DG_VAL_OK or DG_VAL_E_SIZE. */
#define DG_VALS_MAX_COLS 16u
#define DG_VAL_LIST 0x40u
#define DG_VAL_SET 0x80u
#define DG_VAL_OK 0u
#define DG_VAL_E_SIZE 1u /* a STRING length or a list count above 2^31 - 1, or an item of 2^32 bytes or more: the
                            cell is written as the empty value of its kind */
/* one column's inputs, in the shapes dg_cols_* writes (device pointers at the
 * device entry, host pointers at the host entry); what a kind does not read
 * may be NULL, and so may d_src and d_elems of a column whose strings or lists
 * are all empty */
typedef struct dg_val_col {
    const uint64_t *d_val;      /* n: a scalar's value (DOUBLE: its bits); STRING: the payload's byte offset in d_src */
    const uint32_t *d_len;      /* n: STRING: the payload's length */
    const uint8_t *d_src;       /* STRING: the arena the offsets point into, 16 readable bytes after its last payload
                                   byte */
    const uint64_t *d_elem_off; /* n + 1: lists and sets: dg_cols_list_device's d_elem_off */
    const uint64_t *d_elems;    /* lists and sets: its d_elems, 8 bytes an element */
    const uint8_t *d_present;   /* n or NULL (all present); struct mode only: 0 leaves the field out of the message */
} dg_val_col;

/* evals (entry column writes, include/dgj2t.h dg_evals_*), the inverse of
 * ents: a kind is a uint16_t. DG_VAL_LIST | 11 and DG_VAL_SET | 11 are a list
 * and a set of strings or binaries; DG_EVAL_MAP | kt << 4 | vt is a map with
 * the key's wire type kt (3, 6, 8, 10 or 11) and the value's vt (2, 3, 4, 6, 8,
 * 10 or 11). A cell's status is DG_VAL_OK, DG_VAL_E_SIZE or DG_EVAL_E_RANGE. */
#define DG_EVAL_MAP 0x100u
#define DG_EVAL_E_RANGE 2u /* d_ent_off[i] > d_ent_off[i + 1], or d_ent_off[i + 1] > n_ent: the cell is written as the
                              empty container of its kind */
#define DG_EVALS_MAX_ENT 0xFFFFFFFFull /* the most entries one column's arrays may hold (n_ent) */
/* one column's inputs, in the shapes dg_ents_emit_device writes (device
 * pointers at the device entry, host pointers at the host entry); what a kind
 * does not read may be NULL, and so may everything but d_ent_off when n_ent is
 * 0. The list kinds' elements are d_val / d_val_len / d_val_src. */
typedef struct dg_eval_col {
    const uint64_t *d_ent_off; /* n + 1: message i owns the entries [d_ent_off[i], d_ent_off[i + 1]) */
    const uint64_t *d_key;     /* per entry: an int key (its low bits are written at the key's width); a string key:
                                  the payload's byte offset in d_key_src */
    const uint32_t *d_key_len; /* per entry, string keys: the payload's length */
    const uint64_t *d_val;     /* per entry: a scalar (DOUBLE: its bits); a string: the payload's offset in d_val_src */
    const uint32_t *d_val_len; /* per entry, string values and list elements: the payload's length */
    const uint8_t *d_key_src;  /* the arenas the offsets point into, 16 readable bytes after the last payload byte */
    const uint8_t *d_val_src;
    const uint8_t *d_present;  /* n or NULL (all present); struct mode only: 0 leaves the field out of the message */
    uint64_t n_ent;            /* the entries the four per-entry arrays hold, at most DG_EVALS_MAX_ENT: no entry at
                                  an index >= n_ent is read, and the launch geometry comes from it */
} dg_eval_col;

/* t2j (Thrift binary -> JSON, conv/t2j) option bits: the conv.Options fields
 * conv/t2j/impl.go reads (conv/api.go:52-121) */
#define DG_T2J_BYTE_AS_UINT8 (1ull << 0)     /* ByteAsUint8 */
#define DG_T2J_INT64_AS_STRING (1ull << 1)   /* Int642String */
#define DG_T2J_NULL_FOR_NAN_INF (1ull << 2)  /* EncodeNullJSONForInfOrNan */
#define DG_T2J_NO_BASE64 (1ull << 3)         /* NoBase64Binary */
#define DG_T2J_DISALLOW_UNKNOWN (1ull << 4)  /* DisallowUnknownField */
#define DG_T2J_WRITE_DEFAULT (1ull << 5)     /* WriteDefaultField */
#define DG_T2J_WRITE_REQUIRE (1ull << 6)     /* WriteRequireField */
#define DG_T2J_WRITE_OPTIONAL (1ull << 7)    /* WriteOptionalField */
#define DG_T2J_ENABLE_VM (1ull << 8)         /* EnableValueMapping (api.js_conv, agw.body_dynamic) */
/* the Go-side options, with the host's part done around the kernels
 * (dynamicgo_amd.t2j): */
#define DG_T2J_CONVERT_EXC (1ull << 9)       /* ConvertException: the ROOT struct's first field with a non-zero id
                                                ends the conversion (conv/t2j/impl.go:154-159,173-187): status
                                                DG_T2J_E_EXCEPTION, out = that field's value JSON (then any unset
                                                fields written by handleUnsets) */
#define DG_T2J_HM (1ull << 11)               /* EnableHttpMapping (writeHttpValue, conv/t2j/impl.go:515-588): mapped
                                                fields of the root struct and of its fields' struct values stop for
                                                the host (DG_T2J_E_CALLBACK) */
#define DG_T2J_SKIP_RESP_BASE (1ull << 10)   /* EnableThriftBase with a context BaseResp (readResponseBase,
                                                conv/t2j/impl.go:54-72,120-128): the ROOT's response-base fields
                                                (DG_FF_RESPONSE_BASE) are skipped as STRUCTs, no key written; the
                                                last one's value span [lo, hi) of the message goes to aux as
                                                lo | hi << 32 (~0: none) for the host to FastRead */

/* t2j per-message status codes (bits 0-7 of the status word; pos = Thrift
 * read offset, value as noted). The reference returns Go errors whose
 * meta.ErrorCode behaviour is given. */
#define DG_T2J_E_READ 1           /* ErrRead: truncated input, invalid type / size, skip depth; value = reason */
#define DG_T2J_E_UNKNOWN_FIELD 2  /* ErrUnknownField: value = field id */
#define DG_T2J_E_DISMATCH_TYPE 3  /* ErrDismatchType: value = expected << 8 | got */
#define DG_T2J_E_UNSUPPORTED 4    /* ErrUnsupportedType: value = type */
#define DG_T2J_E_NAN_INF 5        /* ErrWrite: "encounter Nan or Inf double" */
#define DG_T2J_E_MISS_REQUIRED 6  /* ErrMissRequiredField: value = field id */
#define DG_T2J_E_NEEDS_HOST 7     /* a Go-side feature: IDL default JSON values, HTTP mapping, non-inline value mapping,
                                     structs of more than 64 fields */
#define DG_T2J_E_DEPTH 8          /* nesting beyond 4096 containers (the GPU's frame budget; Go recurses further) */
#define DG_T2J_E_WRITE 9          /* ErrWrite: a truncated BYTE/I16/I32/I64/DOUBLE value (doRecurse wraps those reads
                                     as meta.ErrWrite, conv/t2j/impl.go:200-236); value = RD_EOF (1) */
#define DG_T2J_E_EXCEPTION 11     /* DG_T2J_CONVERT_EXC: the exception field's JSON is the output (Go: errors.New(out)) */
#define DG_T2J_E_CALLBACK 12      /* DG_T2J_HM: a writeHttpValue call for the host. out: the payload (the JSON
                                     of a mapped container value, else empty), then a 16-byte trailer of two
                                     little-endian u64: kind (1 a mapped field's value, 2 an unset mapped
                                     field HandleRequires writes) | has-ResponseSetter << 8 | the call's
                                     index << 16 | the field's descriptor index << 32, and the value's start
                                     | its end << 32 (kind 1). The host answers each call (dg_cb_tables
                                     ans_tab, one byte per call in call order: 0 = the response took it, 1 =
                                     write it to the JSON as well, 2 = open: the calls converting its value
                                     follow) and converts the message again. */
#define DG_T2J_E_CONVERT 10       /* ErrConvert: a map key failed (buildinTypeToKey, wrapped as meta.ErrConvert by
                                     conv/t2j/impl.go:355-358): value = the read reason (RD_*), or 0x100 | type for
                                     a key type it does not support */

#endif /* DGJ2T_DEFS_H */
