/* The Children walk (dynamicgo_amd/csrc/kids_device.h) built for the host: the
 * count pass and the emit pass of one message as the kernels run them, with 8
 * levels, then with 1024 where that ends deep. test_kids_host.py loads it; with
 * -DKIDS_MAIN it is a program that runs a corpus file with every message, the
 * blob, the heads and the record array in heap blocks of their own (16 spare
 * bytes after a message and the blob, none after the rest; the record array
 * holds exactly the total) for a sanitizer to watch the reads and the stores. */
#define TGI inline
#include "../dynamicgo_amd/csrc/kids_device.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

template <uint32_t CAP>
struct HostFrames {
    static constexpr uint32_t cap = CAP;
    uint64_t *base;
    uint64_t &at(uint32_t l) const { return base[l]; }
    uint64_t &aux(uint32_t l) const { return base[CAP + l]; }
};

static dg::KDParams params(const uint8_t *msg, const uint64_t *in_off, const uint8_t *blob, uint32_t off_steps,
                           uint32_t off_pool, uint32_t n_steps, uint32_t root_type, uint32_t recurse, dg_kids_head *head,
                           uint64_t *rec_off, dg_kid_rec *recs)
{
    dg::KDParams A = {};
    A.tg.src = msg, A.tg.in_off = in_off, A.tg.blob = blob, A.tg.off_steps = off_steps, A.tg.off_pool = off_pool;
    A.tg.root_type = root_type;
    A.n = 1, A.n_steps = n_steps, A.recurse = recurse, A.head = head, A.rec_off = rec_off, A.recs = recs;
    return A;
}

/* the count pass: *head; returns whether the message needed the 1024 levels */
extern "C" int kids_count(const uint8_t *msg, uint64_t len, const uint8_t *blob, uint32_t off_steps, uint32_t off_pool,
                          uint32_t n_steps, uint32_t root_type, uint32_t recurse, dg_kids_head *head)
{
    std::vector<uint64_t> mem(2 * dg::KD_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull); /* garbage a frame must not inherit */
    const uint64_t in_off[2] = {0, len};
    const dg::KDParams A = params(msg, in_off, blob, off_steps, off_pool, n_steps, root_type, recurse, head, nullptr, nullptr);
    const int deep = dg::kd_count_msg(A, 0, HostFrames<dg::KD_LDS_DEPTH>{mem.data()});
    if (deep && dg::kd_count_msg(A, 0, HostFrames<dg::KD_DEEP_DEPTH>{mem.data()})) return -1;
    return deep;
}

/* the emit pass of a message whose head is OK: head->count records at recs */
extern "C" int kids_emit(const uint8_t *msg, uint64_t len, uint32_t n_steps, uint32_t recurse, dg_kids_head *head,
                         dg_kid_rec *recs)
{
    std::vector<uint64_t> mem(2 * dg::KD_DEEP_DEPTH, 0xA5A5A5A5A5A5A5A5ull);
    const uint64_t in_off[2] = {0, len};
    uint64_t rec_off[2] = {0, head->count};
    const dg::KDParams A = params(msg, in_off, nullptr, 0, 0, n_steps, 0, recurse, head, rec_off, recs);
    const int deep = dg::kd_emit_msg(A, 0, head->count, HostFrames<dg::KD_LDS_DEPTH>{mem.data()});
    if (deep && dg::kd_emit_msg(A, 0, head->count, HostFrames<dg::KD_DEEP_DEPTH>{mem.data()})) return -1;
    return deep;
}

#ifdef KIDS_MAIN
/* corpus (tgetgen.write_corpus): u32 n_msgs, n_paths, root_type, off_steps, off_pool, blob_len; the blob; per message
 * u32 len, bytes. Every corpus runs in both modes. */
int main(int argc, char **argv)
{
    unsigned long msgs = 0, deep = 0, total = 0, by[256] = {};
    for (int f = 1; f < argc; f++) {
        for (uint32_t recurse = 0; recurse < 2; recurse++) {
            FILE *fh = fopen(argv[f], "rb");
            uint32_t h[6], n_steps;
            if (!fh || fread(h, 4, 6, fh) != 6) return 2;
            uint8_t *blob = (uint8_t *)malloc(h[5] + 16);
            if (fread(blob, 1, h[5], fh) != h[5]) return 2;
            memset(blob + h[5], 0, 16);
            memcpy(&n_steps, blob + 16, 4);
            std::vector<uint8_t *> m(h[0]);
            std::vector<uint32_t> len(h[0]);
            dg_kids_head *head = (dg_kids_head *)malloc(h[0] * sizeof(dg_kids_head));
            uint64_t need = 0;
            for (uint32_t i = 0; i < h[0]; i++, msgs++) {
                if (fread(&len[i], 4, 1, fh) != 1) return 2;
                m[i] = (uint8_t *)malloc(len[i] + 16);
                if (fread(m[i], 1, len[i], fh) != len[i]) return 2;
                memset(m[i] + len[i], 0xAA, 16);
                const int d = kids_count(m[i], len[i], blob, h[3], h[4], n_steps, h[2], recurse, head + i);
                if (d < 0) return 3;
                deep += d;
                by[head[i].status]++;
                need += head[i].count;
            }
            dg_kid_rec *recs = (dg_kid_rec *)malloc(need * sizeof(dg_kid_rec)); /* exactly the total */
            uint64_t at = 0;
            for (uint32_t i = 0; i < h[0]; i++) {
                if (head[i].status == DG_TGET_OK && head[i].count && kids_emit(m[i], len[i], n_steps, recurse, head + i, recs + at) < 0)
                    return 3;
                at += head[i].count;
                free(m[i]);
            }
            for (uint64_t k = 0; k < need; k++) /* every record was written: no record ends before it starts */
                if (recs[k].end < recs[k].start || recs[k].depth == 0) return 4;
            total += need;
            free(recs);
            free(head);
            free(blob);
            fclose(fh);
        }
    }
    printf("%lu messages, %lu deep, %lu records; OK %lu, NOT_FOUND %lu, E_READ %lu, E_TYPE %lu, E_UNSUPPORTED %lu\n", msgs,
           deep, total, by[0], by[1], by[2], by[3], by[4]);
    return 0;
}
#endif
