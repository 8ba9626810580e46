// Stand-alone host check of alink_amd/ops/csrc/kmeans_v10_map.h, built and run by tests/test_kmeans_v10_map.py.
// It walks every workgroup of a launch exactly as a loader wave of the kernel does -- one unsigned byte offset,
// re-based when it meets its limit -- and checks every staged tile.  Prints one line per failure; exit status 1 then.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "kmeans_v10_map.h"

using namespace km10map;

static long g_fail = 0;
static long g_tiles = 0;

#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            if (g_fail < 40) {                 \
                printf("FAIL %s: ", #cond);    \
                printf(__VA_ARGS__);           \
                printf("\n");                  \
            }                                  \
            ++g_fail;                          \
        }                                      \
    } while (0)

// window: 0 = the production length
template <int S>
static void check_launch(int64_t N, int grid_req, int window) {
    const int ntiles = (int)((N + TILE_ROWS - 1) / TILE_ROWS);
    const int G = grid<S>(ntiles, grid_req);
    const int W = window > 0 ? window : max_window<S>(G);
    const int64_t xbytes = N * ROW_BYTES;
    CHECK(G >= 1 && G <= grid_req && G <= ntiles, "S %d N %ld grid %d -> %d", S, (long)N, grid_req, G);
    CHECK(window_span<S>(G, W) * TILE_BYTES < RSRC_LIMIT || window > 0, "S %d G %d W %d span", S, G, W);
    if (window == 0)
        CHECK(window_span<S>(G, W + 1) * TILE_BYTES >= RSRC_LIMIT, "S %d G %d: W %d is not the largest", S, G, W);
    std::vector<unsigned char> seen(ntiles, 0);
    std::vector<int> fwd;
    int64_t total = 0;
    for (int b = 0; b < G; ++b) {
        Geom g;
        g.N = N, g.ntiles = ntiles, g.G = G, g.b = b, g.W = W;
        g.nt = owned<S>(ntiles, G, b);
        g.ntp = (g.nt + 1) / 2 * 2;
        CHECK(g.nt >= 1, "S %d N %ld G %d b %d owns %d", S, (long)N, G, b, g.nt);
        if (b > 0) {
            const int prev = owned<S>(ntiles, G, b - 1);
            CHECK(g.nt <= prev, "S %d N %ld G %d b %d owns %d, b-1 owns %d", S, (long)N, G, b, g.nt, prev);
        }
        total += g.nt;
        fwd.assign(g.ntp, -2);
        for (int rev = 0; rev < 2; ++rev) {
            g.rev = rev;
            const uint32_t st = step<S>(g);
            Walk w = walk_begin(g);          // soff == lim: the first tile re-bases
            Rebase r = {0, 0};
            int phantoms = 0, rebases = 0, turns = 0;
            for (int t = 0; t < g.ntp; ++t) {
                turns += w.soff == w.lim;
                // the kernel's own step: turn if due (the callback is where the kernel makes the resource), the tile's
                // offset, advance
                const uint32_t soff =
                    walk_tile<S>(g, t, st, w.soff, w.lim, w.win_lo, w.win_last, [&](const Rebase& nr) {
                        r = nr;
                        ++rebases;
                    });
                const int o = owned_of_logical(g, t);
                const int64_t base = (int64_t)r.base_tile * TILE_BYTES;
                CHECK(r.base_tile >= 0 && r.records > 0 && base + r.records <= xbytes,
                      "S %d N %ld G %d W %d b %d rev %d t %d: window [%ld, +%d) outside X", S, (long)N, G, W, b, rev,
                      t, (long)base, r.records);
                CHECK((int64_t)soff + TILE_BYTES < RSRC_LIMIT, "S %d N %ld G %d W %d b %d rev %d t %d: offset %u", S,
                      (long)N, G, W, b, rev, t, soff);
                int gt = -1;
                if (phantom(g, o)) {
                    ++phantoms;
                    CHECK(o == g.nt && (g.nt & 1), "S %d N %ld G %d b %d rev %d t %d: phantom at %d of %d", S,
                          (long)N, G, b, rev, t, o, g.nt);
                    CHECK((int64_t)soff >= r.records, "S %d N %ld G %d b %d rev %d t %d: the phantom tile reads X", S,
                          (long)N, G, b, rev, t);
                } else {
                    gt = global_tile<S>(G, b, o);
                    CHECK(gt >= 0 && gt < ntiles, "S %d N %ld G %d b %d o %d: global tile %d", S, (long)N, G, b, o,
                          gt);
                    CHECK(base + soff == (int64_t)gt * TILE_BYTES,
                          "S %d N %ld G %d W %d b %d rev %d t %d: reads %ld, tile %d is at %ld", S, (long)N, G, W, b,
                          rev, t, (long)(base + soff), gt, (long)gt * TILE_BYTES);
                    // every byte of the tile that exists is inside the window
                    int64_t live = xbytes - (int64_t)gt * TILE_BYTES;
                    if (live > TILE_BYTES) live = TILE_BYTES;
                    CHECK((int64_t)soff + live <= r.records,
                          "S %d N %ld G %d W %d b %d rev %d t %d: tile ends past its window", S, (long)N, G, W, b,
                          rev, t);
                    if (!rev && gt >= 0 && gt < ntiles) {
                        CHECK(seen[gt] == 0, "S %d N %ld G %d: tile %d owned twice", S, (long)N, G, gt);
                        seen[gt] = 1;
                    }
                }
                if (!rev) fwd[t] = gt;
                else
                    CHECK(fwd[g.ntp - 1 - t] == gt, "S %d N %ld G %d W %d b %d: reverse tile %d is %d, forward %d", S,
                          (long)N, G, W, b, t, gt, fwd[g.ntp - 1 - t]);
                ++g_tiles;
            }
            CHECK(phantoms == (g.nt & 1), "S %d N %ld G %d b %d rev %d: %d phantoms", S, (long)N, G, b, rev,
                  phantoms);
            // the resource is re-based once per window, at the phantom and behind it; the other turns are chunk ends
            const int most = (g.nt + W - 1) / W + 2;
            CHECK(rebases <= most, "S %d N %ld G %d W %d b %d rev %d: %d re-bases, at most %d", S, (long)N, G, W, b,
                  rev, rebases, most);
            CHECK(turns - rebases <= (S > 1 ? g.nt / S + 1 : 0), "S %d N %ld G %d W %d b %d rev %d: %d chunk turns", S,
                  (long)N, G, W, b, rev, turns - rebases);
        }
    }
    CHECK(total == ntiles, "S %d N %ld G %d: %ld tiles owned of %d", S, (long)N, G, (long)total, ntiles);
    for (int i = 0; i < ntiles; ++i)
        if (!seen[i]) {
            CHECK(false, "S %d N %ld G %d: tile %d owned by nobody", S, (long)N, G, i);
            break;
        }
}

template <int S>
static void check_all() {
    // the rows of tests/test_kmeans_v10_sweep_gpu.py's shapes, and bench.py's 1e8 (1,562,500 tiles)
    const int64_t rows[] = {133, 253, 257, 320, 10513, 4248, 5504, 1409, 11969, 640, 1665, 5440, 100000000};
    const int grids[] = {1, 3, 4, 7, 256};
    const int windows[] = {3, 4, 0};
    for (int64_t n : rows)
        for (int gr : grids)
            for (int w : windows) check_launch<S>(n, gr, w);
}

int main() {
    check_all<1>();
    check_all<2>();
    check_all<8>();
    printf("%s: %ld staged tiles checked, %ld failures\n", g_fail ? "FAILED" : "ok", g_tiles, g_fail);
    return g_fail ? 1 : 0;
}
