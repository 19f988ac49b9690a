/* The map-row walk (dynamicgo_amd/csrc/rows_device.h, map plans) built for the
 * host: the map head (rw_map_head_msg: tg_seek, the header, the key-kind test,
 * kd_scan with KDCount) and the map index (rw_map_index_msg: the arithmetic
 * route, or kd_scan with the storing sink RWMapStore), each with 8 frames and
 * then with 1024 where that ends deep, as the kernels do. One message is a
 * batch of its own: arena offsets are offsets in the message. The row cells are
 * the list plan's (rows_host.cpp builds those). test_mrows_host.py loads it;
 * with -DMROWS_MAIN it is a program that runs corpus files with every message,
 * blob, head, index array, key array and key-length array in an exactly sized
 * heap block of its own (messages and blobs with their 16 spare bytes), for a
 * sanitizer to watch the reads and the stores. */
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

static dg::RWMapParams params(const uint8_t *parent, uint32_t root_type, uint32_t key_kind, const uint8_t *msg,
                              const uint64_t *in_off, dg_rows_head *head, uint32_t *count, uint64_t *row_off)
{
    dg::RWMapParams A = {};
    dg_path_hdr h;
    memcpy(&h, parent, sizeof h);
    A.par.src = msg, A.par.in_off = in_off, A.par.root_type = root_type;
    A.par.blob = parent, A.par.off_steps = h.off_steps, A.par.off_pool = h.off_pool;
    A.n = 1, A.n_steps = h.n_steps, A.key_kind = key_kind;
    A.head = head, A.count = count, A.row_off = row_off;
    return A;
}

/* the head of one message; returns whether it needed the 1024 frames */
extern "C" int mrows_head(const uint8_t *msg, uint64_t len, const uint8_t *parent, uint32_t root_type, uint32_t key_kind,
                          dg_rows_head *head)
{
    std::vector<uint64_t> mem(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull); /* garbage a frame must not inherit */
    const uint64_t in_off[2] = {0, len};
    uint32_t count = 0;
    const dg::RWMapParams A = params(parent, root_type, key_kind, msg, in_off, head, &count, nullptr);
    const int deep = dg::rw_map_head_msg(A, 0, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
    if (deep && dg::rw_map_head_msg(A, 0, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()})) return -1;
    return deep;
}

/* after mrows_head: the index entries, keys and key lengths (min(count,
 * row_cap) of each; key and key_len may be null). Returns whether the walk
 * needed the 1024 frames. */
extern "C" int mrows_index(const uint8_t *msg, uint64_t len, const uint8_t *parent, uint32_t root_type, uint32_t key_kind,
                           dg_rows_head *head, uint64_t row_cap, dg_row_ent *index, uint64_t *key, uint32_t *key_len)
{
    std::vector<uint64_t> mem(dg::TG_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull);
    const uint64_t in_off[2] = {0, len};
    uint64_t row_off[2] = {0, head->count};
    uint32_t count = head->count;
    dg::RWMapParams A = params(parent, root_type, key_kind, msg, in_off, head, &count, row_off);
    A.idx = index, A.row_cap = row_cap, A.key = key, A.key_len = key_len;
    const int deep = dg::rw_map_index_msg(A, 0, HostFrames<dg::TG_LDS_DEPTH>{mem.data()});
    if (deep && dg::rw_map_index_msg(A, 0, HostFrames<dg::TG_DEEP_DEPTH>{mem.data()})) return -1;
    return deep;
}

#ifdef MROWS_MAIN
static uint8_t *block(FILE *fh, uint32_t len, int fill)
{
    uint8_t *p = (uint8_t *)malloc(len + 16);
    if (fread(p, 1, len, fh) != len) exit(2);
    memset(p + len, fill, 16);
    return p;
}

/* corpus (mrowsgen.write_corpus): u32 n_msgs, root_type, key_kind, the parent blob's length; the blob; per message
 * u32 len, bytes. Prints the heads' status counts, the rows and the sum of all index entries' offsets and lengths,
 * all int keys (string keys: their offsets) and all key lengths. */
int main(int argc, char **argv)
{
    unsigned long msgs = 0, rows = 0, deep = 0, hby[256] = {};
    uint64_t sum = 0;
    for (int f = 1; f < argc; f++) {
        FILE *fh = fopen(argv[f], "rb");
        uint32_t h[4], len;
        if (!fh || fread(h, 4, 4, fh) != 4) return 2;
        uint8_t *parent = block(fh, h[3], 0);
        for (uint32_t i = 0; i < h[0]; i++, msgs++) {
            if (fread(&len, 4, 1, fh) != 1) return 2;
            uint8_t *m = block(fh, len, 0xAA);
            dg_rows_head *head = (dg_rows_head *)malloc(sizeof *head);
            const int d = mrows_head(m, len, parent, h[1], h[2], head);
            if (d < 0) return 3;
            deep += d;
            hby[head->status]++;
            const uint32_t n = head->count;
            if (head->status == DG_TGET_OK && n) {
                dg_row_ent *index = (dg_row_ent *)malloc(n * sizeof *index);
                uint64_t *key = (uint64_t *)malloc(n * sizeof *key);
                uint32_t *key_len = (uint32_t *)malloc(n * sizeof *key_len);
                const int r = mrows_index(m, len, parent, h[1], h[2], head, n, index, key, key_len);
                if (r < 0) return 3;
                deep += r;
                for (uint32_t g = 0; g < n; g++, rows++) sum += index[g].off + index[g].len + key[g] + key_len[g];
                free(index);
                free(key);
                free(key_len);
            }
            free(head);
            free(m);
        }
        free(parent);
        fclose(fh);
    }
    printf("%lu messages: OK %lu, NOT_FOUND %lu, E_READ %lu, E_TYPE %lu, E_UNSUPPORTED %lu; %lu rows; sum %llu; %lu deep\n", msgs,
           hby[0], hby[1], hby[2], hby[3], hby[4], rows, (unsigned long long)sum, deep);
    return 0;
}
#endif
