/* The row-column walk (dynamicgo_amd/csrc/rows_device.h) built for the host: the
 * two sinks behind kd_scan (rw_head_msg with KDCount, rw_index_msg with RWStore)
 * and the row cell (rw_cell: tg_walk over an index entry, then cl_cell), each
 * with 8 frames and then with 1024 where that ends deep, as the kernels do.
 * One message is a batch of its own: arena offsets are offsets in the message.
 * test_rows_host.py loads it; with -DROWS_MAIN it is a program that runs corpus
 * files with every message, blob, index array and cell array in an exactly
 * sized heap block of its own (messages and blobs with their 16 spare bytes),
 * for a sanitizer to watch the reads and the stores. */
#define TGI inline
#include "../dynamicgo_amd/csrc/rows_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <uint32_t CAP>
struct HostFrames {
    static constexpr uint32_t cap = CAP;
    uint64_t *base;
    uint64_t &at(uint32_t l) const { return base[l]; }
    uint64_t &aux(uint32_t l) const { return base[l]; }
};

struct Plan {
    const uint8_t *parent, *sub; /* path-set blobs, 16 zero bytes after each */
    uint32_t n_cols, root_type;
    uint64_t kinds;
};

static dg::RWParams params(const Plan &pl, const uint8_t *msg, const uint64_t *in_off, dg_rows_head *head, uint32_t *count,
                           uint64_t *row_off)
{
    dg::RWParams A = {};
    dg_path_hdr h, sh;
    memcpy(&h, pl.parent, sizeof h);
    memcpy(&sh, pl.sub, sizeof sh);
    A.par.src = msg, A.par.in_off = in_off, A.par.root_type = pl.root_type;
    A.par.blob = pl.parent, A.par.off_steps = h.off_steps, A.par.off_pool = h.off_pool;
    A.sub.blob = pl.sub, A.sub.off_steps = sh.off_steps, A.sub.off_pool = sh.off_pool, A.sub.P = pl.n_cols;
    A.n = 1, A.n_steps = h.n_steps, A.kinds = pl.kinds;
    A.head = head, A.count = count, A.row_off = row_off;
    return A;
}

/* the head of one message; returns whether it needed the 1024 frames */
extern "C" int rows_head(const uint8_t *msg, uint64_t len, const uint8_t *parent, const uint8_t *sub, uint32_t n_cols,
                         uint32_t root_type, uint64_t kinds, dg_rows_head *head)
{
    std::vector<uint64_t> mem(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull); /* garbage a frame must not inherit */
    const uint64_t in_off[2] = {0, len};
    uint32_t count = 0;
    const dg::RWParams A = params(Plan{parent, sub, n_cols, root_type, kinds}, msg, in_off, head, &count, nullptr);
    const int deep = dg::rw_head_msg(A, 0, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
    if (deep && dg::rw_head_msg(A, 0, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()})) return -1;
    return deep;
}

/* after rows_head: the index entries (min(count, row_cap) of them) and the
 * cells, row-major, seven words a cell: status, type, step, aux, len, the
 * value's low and high word. Returns index deep | deep cells << 1. */
extern "C" int rows_rest(const uint8_t *msg, uint64_t len, const uint8_t *parent, const uint8_t *sub, uint32_t n_cols,
                         uint32_t root_type, uint64_t kinds, dg_rows_head *head, uint64_t row_cap, dg_row_ent *index,
                         uint32_t *cells)
{
    std::vector<uint64_t> mem(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull);
    const uint64_t in_off[2] = {0, len};
    uint64_t row_off[2] = {0, head->count};
    uint32_t count = head->count;
    dg::RWParams A = params(Plan{parent, sub, n_cols, root_type, kinds}, msg, in_off, head, &count, row_off);
    A.idx = index, A.row_cap = row_cap;
    int deep = dg::rw_index_msg(A, 0, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
    if (deep && dg::rw_index_msg(A, 0, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()})) return -1;
    const uint64_t rows = dg::rw_rows(A);
    for (uint64_t g = 0; g < rows; g++)
        for (uint32_t k = 0; k < n_cols; k++) {
            dg::CLCell c = dg::rw_cell(A, g, k, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
            if (c.status == dg::TG_ST_DEEP) {
                deep += 2;
                c = dg::rw_cell(A, g, k, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()});
            }
            const uint64_t w = dg::cl_cell_word(c); /* the stored form, taken apart again */
            const uint32_t v[7] = {(uint32_t)(w & 0xFF), (uint32_t)(w >> 8 & 0xFF), (uint32_t)(w >> 16 & 0xFFFF),
                                   (uint32_t)(w >> 32), c.len, (uint32_t)c.val, (uint32_t)(c.val >> 32)};
            memcpy(cells + (g * n_cols + k) * 7, v, sizeof v);
        }
    return deep;
}

#ifdef ROWS_MAIN
static uint8_t *block(FILE *fh, uint32_t len, int fill)
{
    uint8_t *p = (uint8_t *)malloc(len + 16);
    if (fread(p, 1, len, fh) != len) exit(2);
    memset(p + len, fill, 16);
    return p;
}

/* corpus (rowsgen.write_corpus): u32 n_msgs, n_cols, root_type, parent blob length, sub blob length; 8 kind bytes;
 * the two blobs; per message u32 len, bytes. Prints the heads' and the cells' status counts, the rows and the sum of
 * all index entries' offsets and lengths and all scalar values. */
int main(int argc, char **argv)
{
    unsigned long msgs = 0, rows = 0, cells = 0, deep = 0, hby[256] = {}, cby[256] = {};
    uint64_t sum = 0;
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t h[5], len;
        uint8_t kb[8];
        if (!fh || fread(h, 4, 5, fh) != 5 || fread(kb, 1, 8, fh) != 8) return 2;
        uint64_t kinds;
        memcpy(&kinds, kb, 8);
        uint8_t *parent = block(fh, h[3], 0), *sub = block(fh, h[4], 0);
        for (uint32_t i = 0; i < h[0]; i++, msgs++) {
            if (fread(&len, 4, 1, fh) != 1) return 2;
            uint8_t *m = block(fh, len, 0xAA);
            dg_rows_head *head = (dg_rows_head *)malloc(sizeof *head);
            const int d = rows_head(m, len, parent, sub, h[1], h[2], kinds, head);
            if (d < 0) return 3;
            deep += d;
            hby[head->status]++;
            const uint32_t n = head->count;
            if (head->status == DG_TGET_OK && n) {
                dg_row_ent *index = (dg_row_ent *)malloc(n * sizeof *index);
                uint32_t *out = (uint32_t *)malloc((size_t)n * h[1] * 28);
                const int r = rows_rest(m, len, parent, sub, h[1], h[2], kinds, head, n, index, out);
                if (r < 0) return 3;
                deep += r;
                for (uint32_t g = 0; g < n; g++, rows++) {
                    sum += index[g].off + index[g].len;
                    for (uint32_t k = 0; k < h[1]; k++, cells++) {
                        const uint32_t *c = out + ((size_t)g * h[1] + k) * 7;
                        cby[c[0] & 255]++;
                        if (kb[k] != DG_COL_STR && !(kb[k] & DG_COL_LIST)) sum += c[5] | (uint64_t)c[6] << 32;
                    }
                }
                free(index);
                free(out);
            }
            free(head);
            free(m);
        }
        free(parent);
        free(sub);
        fclose(fh);
    }
    printf("%lu messages: OK %lu, NOT_FOUND %lu, E_READ %lu, E_TYPE %lu, E_UNSUPPORTED %lu; %lu rows, %lu cells: OK %lu, "
           "NOT_FOUND %lu, E_READ %lu, E_TYPE %lu, E_UNSUPPORTED %lu; sum %llu; %lu deep\n",
           msgs, hby[0], hby[1], hby[2], hby[3], hby[4], rows, cells, cby[0], cby[1], cby[2], cby[3], cby[4],
           (unsigned long long)sum, deep);
    return 0;
}
#endif
