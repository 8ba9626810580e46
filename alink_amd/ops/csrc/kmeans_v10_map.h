// KMeans v10: which tiles a workgroup owns and how its loader waves walk them -- the swept tile order.
//
// X is cut into 64-row tiles and the tiles into chunks of S consecutive tiles (S is a compile-time power of two).
// Workgroup b of G owns the chunks b, b + G, b + 2G, ...: its owned tile o is the global tile
//     ((o / S) * G + b) * S + o % S,
// so at any moment the G workgroups together read one moving window of X instead of G runs far apart.  When the
// chunk count is no multiple of G the first workgroups own one chunk more; the last chunk of X may be short, and it
// is the last chunk of the workgroup that owns it.
//
// A workgroup's tiles span all of X, more than one buffer resource (< 2 GiB) can cover.  The owned tiles are
// therefore cut into windows of W owned tiles; a window's resource starts at its first owned tile and ends with
// its last one (or with X), and a tile is addressed by a byte offset from that base.  The walk's whole state is that
// one scalar offset `soff` and the value `lim` at which it has to be looked at again: per staged tile
//     if (soff == lim) turn();  stage(soff);  soff += step;                          (walk_tile)
// turn() is reached at a chunk's end (S > 1: the offset jumps over the other workgroups' chunks, a few scalar
// instructions) and, a dozen times per launch, where the resource is re-based: at the first tile, at a window's end
// and at the phantom tile.
//
// The kernel works on tile PAIRS, so a workgroup with an odd tile count nt walks ntp = nt + 1 tiles: owned tile nt
// is a phantom.  Its index may fall past the end of X or into another workgroup's tile; it is never read -- its
// resource is the last real tile's and its offset lies one tile past that resource's end, so the loads return
// zeros -- and never published or counted.  The reverse (serpentine) walk takes logical tile t to owned tile
// ntp - 1 - t: the forward walk backwards, with the same windows.
//
// Plain C++: the kernel (device), its launch wrapper (host) and tests/test_kmeans_v10_map.py (a stand-alone host
// program) all compile this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KM10_HD __host__ __device__ __forceinline__
#else
#define KM10_HD inline
#endif

namespace km10map {

constexpr int TILE_ROWS = 64;
constexpr int ROW_BYTES = 256;
constexpr int TILE_BYTES = TILE_ROWS * ROW_BYTES;
constexpr int64_t RSRC_LIMIT = (int64_t)1 << 31;     // bytes one buffer resource may cover (exclusive)

// one workgroup's view of a launch: N rows in ntiles tiles, workgroup b of G, nt owned tiles walked as ntp (even),
// windows of W owned tiles, rev = the serpentine direction
struct Geom {
    int64_t N;
    int ntiles, G, b, nt, ntp, W, rev;
};

template <int S>
KM10_HD int chunks(int ntiles) {
    return (int)(((int64_t)ntiles + S - 1) / S);
}

// workgroups that own at least one chunk
template <int S>
KM10_HD int grid(int ntiles, int grid) {
    const int nch = chunks<S>(ntiles);
    return grid < nch ? grid : nch;
}

// tiles workgroup b owns
template <int S>
KM10_HD int owned(int ntiles, int G, int b) {
    const int nch = chunks<S>(ntiles);
    const int c = nch / G + (b < nch % G ? 1 : 0);
    int nt = c * S;
    if (c > 0 && (nch - 1) % G == b) nt -= (int)((int64_t)nch * S - ntiles);     // the short last chunk
    return nt;
}

template <int S>
KM10_HD int global_tile(int G, int b, int o) {
    static_assert(S >= 1 && (S & (S - 1)) == 0, "the chunk is a power of two");
    return ((o / S) * G + b) * S + o % S;
}

KM10_HD int owned_of_logical(const Geom& g, int t) { return g.rev ? g.ntp - 1 - t : t; }

KM10_HD bool phantom(const Geom& g, int o) { return o >= g.nt; }

// global tiles from the first to the last of W consecutive owned tiles, at most
template <int S>
KM10_HD int64_t window_span(int G, int W) {
    return (int64_t)((W + S - 2) / S) * (G - 1) * S + W;
}

// the production window: the largest W whose span stays under one buffer resource
template <int S>
KM10_HD int max_window(int G) {
    int lo = 1, hi = (int)(RSRC_LIMIT / TILE_BYTES) - 1;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (window_span<S>(G, mid) * TILE_BYTES < RSRC_LIMIT) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the walk's byte step per staged tile (unsigned: it wraps, as the offset does)
template <int S>
KM10_HD uint32_t step(const Geom& g) {
    const uint32_t s = S == 1 ? (uint32_t)g.G * (uint32_t)TILE_BYTES : (uint32_t)TILE_BYTES;
    return g.rev ? 0u - s : s;
}

struct Rebase {
    int base_tile;      // global tile the window's buffer resource starts at
    int records;        // bytes that resource covers
};

// The walk of one loader wave: soff = byte offset of the next staged tile from the resource's base, lim = the soff at
// which the walk turns; the resource covers the owned tiles win_lo .. win_last (none while win_last < win_lo: before
// the first tile and behind a phantom)
struct Walk {
    uint32_t soff, lim;
    int win_lo, win_last;
};

// before the first tile: soff == lim, so the first tile turns, and no resource
KM10_HD Walk walk_begin(const Geom& g) {
    Walk w;
    w.soff = w.lim = 0u;
    w.win_lo = g.rev && g.nt > 0 ? (g.nt - 1) / g.W * g.W : 0;     // the window the walk starts in
    w.win_last = -1;
    return w;
}

// soff has met lim at logical tile t.  Inside the current window that is a chunk's end (S > 1): the offset jumps
// over the other workgroups' chunks, nothing else moves, and false is returned.  Otherwise (the first tile, a
// window's end, the phantom tile, the tile behind a phantom) the resource is re-based: r is filled, true returned.
template <int S>
KM10_HD bool walk_turn(const Geom& g, int t, uint32_t& w_soff, uint32_t& w_lim, int& w_win_lo, int& w_win_last,
                       Rebase& r) {
    const int o = owned_of_logical(g, t);
    const uint32_t st = step<S>(g);
    if (S > 1 && o >= w_win_lo && o <= w_win_last) {
        const uint32_t jump = (uint32_t)(g.G - 1) * (uint32_t)(S * TILE_BYTES);
        w_soff += g.rev ? 0u - jump : jump;
        int n = g.rev ? o - w_win_lo + 1 : w_win_last - o + 1;      // tiles up to the window's end, this one included
        if (n > S) n = S;                                           // ... and up to the next chunk's end
        w_lim = w_soff + (uint32_t)n * st;
        return false;
    }
    const int64_t xbytes = g.N * ROW_BYTES;
    if (phantom(g, o)) {
        r.base_tile = global_tile<S>(g.G, g.b, g.nt - 1);
        const int64_t rem = xbytes - (int64_t)r.base_tile * TILE_BYTES;
        r.records = (int)(rem < TILE_BYTES ? rem : TILE_BYTES);
        w_soff = (uint32_t)TILE_BYTES;
        w_lim = w_soff + st;
        w_win_last = -1;
        return true;
    }
    if (o >= w_win_lo + g.W) w_win_lo += g.W;
    else if (o < w_win_lo) w_win_lo -= g.W;
    w_win_last = w_win_lo + g.W - 1 < g.nt - 1 ? w_win_lo + g.W - 1 : g.nt - 1;
    r.base_tile = global_tile<S>(g.G, g.b, w_win_lo);
    int64_t end = (int64_t)(global_tile<S>(g.G, g.b, w_win_last) + 1) * TILE_BYTES;
    if (end > xbytes) end = xbytes;
    r.records = (int)(end - (int64_t)r.base_tile * TILE_BYTES);
    w_soff = (uint32_t)(global_tile<S>(g.G, g.b, o) - r.base_tile) * (uint32_t)TILE_BYTES;
    int n = g.rev ? o - w_win_lo + 1 : w_win_last - o + 1;
    if (S > 1) {
        const int c = g.rev ? o % S + 1 : S - o % S;
        if (c < n) n = c;
    }
    w_lim = w_soff + (uint32_t)n * st;
    return true;
}

#if defined(__GNUC__) || defined(__clang__)
#define KM10_UNLIKELY(x) __builtin_expect(!!(x), 0)
#else
#define KM10_UNLIKELY(x) (x)
#endif

// One staged tile, as the kernel's loader waves and the host check both run it: turn if the offset has met its
// limit (rebuild(r) is where the caller makes the buffer resource when the window changed), hand out
// the tile's offset, step on.  st = step<S>(g), kept by the caller; the walk's state goes in as its four scalars
// (the kernel keeps each in a scalar register of its own).
template <int S, class F>
KM10_HD uint32_t walk_tile(const Geom& g, int t, uint32_t st, uint32_t& w_soff, uint32_t& w_lim, int& w_win_lo,
                           int& w_win_last, F&& rebuild) {
    if (KM10_UNLIKELY(w_soff == w_lim)) {
        Rebase r;
        if (walk_turn<S>(g, t, w_soff, w_lim, w_win_lo, w_win_last, r)) rebuild(r);
    }
    const uint32_t soff = w_soff;
    w_soff += st;
    return soff;
}

}  // namespace km10map
