/* The layout arithmetic of the thrift/generic host entries
 * (dynamicgo_amd/csrc/host_layout.h) as a stand-alone program for the
 * sanitizers (test_host_layout_host.py):
 *
 *   host_layout_host CASES       a text file, one case per line
 *
 * A line is a name and unsigned numbers, inputs first, then what the routine
 * must leave behind:
 *   rebase K count off[count + 1]
 *          rc written rel[written] longest[K]
 *   layout n in_off[n + 1] extra[n] with_idx m idx[m] with_so with_src with_longest
 *          rc bad bad_cap written io[written] written so[written] written src[written] longest
 * layout's capacity of message i is extra[i] + the length it is handed; idx,
 * so, src and longest are null unless their flag is set (without idx, m = n;
 * without longest, the line's last number is the fill). `written`
 * counts the leading entries the routine has to write; the rest of that array
 * must still hold the fill. Every input and output array is a heap block of
 * exactly its size, so an index past it is caught. Plain C++: the header
 * takes no HIP. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../dynamicgo_amd/csrc/host_layout.h"

static const uint64_t FILL = 0xA5A5A5A5A5A5A5A5ull, MOST = 1u << 20;

/* an exact-size heap block of n words (n = 0: still a block of its own), or none */
struct Block {
    uint64_t *p;
    uint64_t n;
    explicit Block(uint64_t n_, bool have = true) : p(have ? (uint64_t *)malloc(n_ ? n_ * 8 : 1) : nullptr), n(have ? n_ : 0)
    {
        for (uint64_t k = 0; k < n; k++) p[k] = FILL;
    }
    ~Block() { free(p); }
    Block(const Block &) = delete;
};

static std::vector<uint64_t> words;
static size_t at;
static bool short_line;
static uint64_t next()
{
    if (at >= words.size()) {
        short_line = true;
        return 0;
    }
    return words[at++];
}
static void read_into(Block &b)
{
    for (uint64_t k = 0; k < b.n; k++) b.p[k] = next();
}
/* the line's next number says how many leading words of b were to be written;
 * they are the numbers after it, and the others still the fill (no block: 0) */
static bool holds(const Block &b)
{
    const uint64_t written = next();
    bool ok = written <= b.n;
    for (uint64_t k = 0; k < b.n; k++) ok &= b.p[k] == (k < written ? next() : FILL);
    return ok;
}

static bool run(const std::string &name)
{
    if (name == "rebase") {
        const uint64_t K = next(), count = next();
        if (K < 1 || K > 64 || count > MOST) return false;
        Block off(count + 1), rel(count + 1), longest(K);
        read_into(off);
        const bool same = (uint64_t)dg::hl_rebase(off.p, count, K, rel.p, longest.p) == next();
        const bool rel_ok = holds(rel);
        for (uint64_t j = 0; j < K; j++)
            if (longest.p[j] != next()) return false;
        return same && rel_ok;
    }
    if (name == "layout") {
        const uint64_t n = next();
        if (n > MOST) return false;
        Block in_off(n + 1), extra(n);
        read_into(in_off);
        read_into(extra);
        const bool with_idx = next();
        const uint64_t m = next();
        if (m > MOST || (!with_idx && m != n)) return false;
        Block idx(m, with_idx);
        read_into(idx);
        const bool with_so = next(), with_src = next(), with_longest = next();
        Block io(m + 1), so(m + 1, with_so), src(m, with_src);
        uint64_t longest = FILL, bad = FILL, bad_cap = FILL;
        const uint64_t rc = (uint64_t)dg::hl_layout(
            in_off.p, idx.p, m, [&](uint64_t i, uint64_t len) { return extra.p[i] + len; }, io.p, so.p, src.p,
            with_longest ? &longest : nullptr, &bad, &bad_cap);
        const uint64_t want_rc = next(), want_bad = next(), want_cap = next();
        bool ok = rc == want_rc && (rc == dg::HL_OK || bad == want_bad) && (rc != dg::HL_TOO_LONG || bad_cap == want_cap);
        ok &= holds(io);
        ok &= holds(so);
        ok &= holds(src);
        return longest == (with_longest ? next() : FILL) && ok;
    }
    return false;
}

int main(int argc, char **argv)
{
    FILE *fh = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!fh) {
        fprintf(stderr, "usage: host_layout_host CASES\n");
        return 2;
    }
    static char line[1 << 20];
    int cases = 0, bad = 0;
    while (fgets(line, sizeof line, fh)) {
        char *tok = strtok(line, " \n");
        if (!tok) continue;
        const std::string name = tok;
        words.clear(), at = 0, short_line = false;
        while ((tok = strtok(nullptr, " \n"))) words.push_back(strtoull(tok, nullptr, 0));
        cases++;
        if (!run(name) || short_line || at != words.size()) {
            fprintf(stderr, "case %d (%s): not what the line expects\n", cases, name.c_str());
            bad++;
        }
    }
    fclose(fh);
    printf("%d cases, %d bad\n", cases, bad);
    return bad || !cases;
}
