// conv_thin_addr_check.hip -- the geometry and global-address rules of csrc/conv_thin_addr.h on the CPU.  The loops below
// are the kernels' own (block -> (strip, unit) -> segment; thread, slot, item -> request), with the header's functions in
// the places where ct_out_kernel, ct_in_kernel and ct_wg_kernel call them, over
//   CU counts {64, 256, 304} x N {1, 2, 8, 64, 128} x H {1, 2, 7, 8, 9, 19, 67, 132, 140}
//   x every supported W up to 264 in steps of the dtype's granularity, 512 and 1024 (weight gradient: W % 8 == 0)
//   x Ct 1..4, Cw {32, 64}, K {3, 5} with Ct * K <= 16 x element sizes {2, 4}.
// Asserted: every request and store of a possibly masked lane lies in [0, tensor elements) for its full 16 bytes (more:
// inside its own image row) and is 16-byte aligned relative to the base; the segments tile [0, H) once; both block
// mappings are bijections onto (strip, unit); the dynamic LDS stays under the limit the launchers raise; the staging
// writes stay inside the LDS image; ct_wg_geom ends with RS >= 1.
// What is enumerated and what is bounded: an offset is  image(n) + f(lane, slot, item) + row * W  with non-negative
// coefficients, every (image, segment, strip) combination is a block (the bijection), so where a term is affine it is
// walked at its two ends (n in {0, N - 1}; a clamped row at the least and the greatest row any segment requests; the
// channel lane and tile of the wide request at (0, 0, 0) and (15, last, last)) and everything else -- strips, segments,
// threads, slots, chunks, items, lane groups -- is walked in full.  A walk that only depends on (rows per segment) is
// not repeated for a second (CU count, N) that gives the same split.
// The `while` loop of ct_wg_geom (the thin image of a segment must fit LDS) needs Ct * W beyond what a quick GPU test
// can hold: this program is its only coverage (W = 512 and 1024 reach it).
// Negative control: the wide request as it was before the column clamp covered 8 * kg must be reported out of bounds by
// exactly 24, 16 and 8 elements at W = 8, 16, 24 and in bounds from W = 32.  No HIP call; tests/test_conv_thin_addr.py
// builds this with the host sanitizers and expects exit code 0.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <set>
#include <vector>
#include "../../ofa-for-super-resolution_amd/csrc/conv_thin_addr.h"

using namespace ofasr;

static long bad = 0;
static long long walked = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond) && bad++ < 10) fprintf(stderr, "line %d: %s  [%s]\n", __LINE__, #cond, ctx);   \
    } while (0)
static char ctx[256];

struct Shape { int cus, N, H, W, es, Ct, Cw, K; };
static void set_ctx(const char* what, const Shape& s) {
    snprintf(ctx, sizeof ctx, "%s cus=%d N=%d H=%d W=%d es=%d Ct=%d Cw=%d K=%d", what, s.cus, s.N, s.H, s.W, s.es, s.Ct, s.Cw, s.K);
}

// a 16-byte request of `epc` elements at element offset `off` inside image n of [N][C][H][W]: inside the tensor, aligned
static void check_request(long long img_off, long long off, int C, long long plane, int N, int epc) {
    const long long total = (long long)N * C * plane;
    CHECK(off >= 0 && off + epc <= (long long)C * plane);                  // inside its image
    CHECK(img_off + off >= 0 && img_off + off + epc <= total);             // inside the tensor
    CHECK((img_off + off) % epc == 0);
    ++walked;
}

static void check_tiling(int H, int RS, int segs) {
    CHECK(RS >= 1);
    int next = 0;
    for (int seg = 0; seg < segs; ++seg) {
        const int ys = seg * RS, ye = ys + RS < H ? ys + RS : H;
        CHECK(ys == next && ye > ys);
        next = ye;
    }
    CHECK(next == H);
}

template <typename Map> static void check_bijection(int units, int strips, Map map) {
    std::vector<char> seen((size_t)units * strips, 0);
    for (int b = 0; b < units * strips; ++b) {
        int strip = -1, unit = -1;
        map(b, strip, unit);
        CHECK(strip >= 0 && strip < strips && unit >= 0 && unit < units);
        if (strip >= 0 && strip < strips && unit >= 0 && unit < units) {
            CHECK(!seen[(size_t)unit * strips + strip]);
            seen[(size_t)unit * strips + strip] = 1;
        }
    }
}
static void check_mappings(const CtGeom& g) {
    const int units = g.N * g.segs;
    check_bijection(units, g.strips, [&](int b, int& s, int& u) { ct_block_map(b, units, g.strips, s, u); });
    check_bijection(units, g.strips, [&](int b, int& s, int& u) { ct_block_map_plain(b, g.strips, s, u); });
    if (ct_block_map_is_xcd(units)) check_bijection(units, g.strips, [&](int b, int& s, int& u) { ct_block_map_xcd(b, g.strips, s, u); });
}

// ---- ct_out_kernel: the staged-row requests (prologue, the CT_D - 1 rows ahead, the row loop) ----------------------------
static void check_out(const Shape& s) {
    set_ctx("ct_out", s);
    const CtGeom g = ct_geom(s.N, s.Ct, s.Cw, s.H, s.W, s.es, s.cus);
    const bool is16 = s.es == 2;
    const int THREADS = is16 ? 576 : 512, NC = s.Cw / 32, P = s.K / 2, epc = ct_epc(s.es), CW = ct_cw(s.es);
    const int NCH = s.Cw * CT_CHUNKS, SLOTS = (NCH + THREADS - 1) / THREADS;
    const long long plane = (long long)s.H * s.W;
    CHECK(ct_out_lds_bytes(is16, s.K, NC) <= CT_LDS_LIMIT);
    CHECK(g.strips * CW >= s.W && (g.strips - 1) * CW < s.W);
    // every row any segment requests: least and greatest (each one inside the image)
    int rmin = s.H, rmax = -1;
    auto row = [&](int r) {
        CHECK(r >= 0 && r < s.H);
        rmin = r < rmin ? r : rmin;
        rmax = r > rmax ? r : rmax;
    };
    for (int seg = 0; seg < g.segs; ++seg) {
        const int ys = seg * g.RS, ye = ys + g.RS < s.H ? ys + g.RS : s.H;
        for (int i = 0; i < s.K; ++i) row(ct_out_prologue_row(ys, P, i, s.H));
        for (int d = 1; d < CT_D; ++d) row(ct_out_request_row(ys + P + d, ye, P, s.H));
        const int trips = (ye - ys + CT_D - 1) / CT_D;
        for (int it = 0; it < trips; ++it)
            for (int d = 0; d < CT_D; ++d) row(ct_out_request_row(ys + it * CT_D + d + P + CT_D, ye, P, s.H));
    }
    for (int strip = 0; strip < g.strips; ++strip) {
        const int x0 = strip * CW;
        std::vector<char> covered(NCH, 0);
        for (int q = 0; q < SLOTS; ++q)
            for (int tid = 0; tid < THREADS; ++tid) {
                const CtOutChunk k = ct_out_chunk((q * THREADS + tid) % NCH, x0, epc, s.W, plane);
                CHECK(k.c >= 0 && k.c < s.Cw && k.jc >= 0 && k.jc < CT_CHUNKS);
                const long long col = k.g_off - (long long)k.c * plane;       // the clamped column: the chunk lies inside the row
                CHECK(col >= 0 && col + epc <= s.W);
                CHECK(k.c * CT_ROWB + k.jc * 16 + 16 <= 32 * NC * CT_ROWB);    // the LDS slot of the chunk inside one staged row
                covered[k.c * CT_CHUNKS + k.jc] = 1;
                for (int n = 0; n < s.N; n += (s.N > 1 ? s.N - 1 : 1))
                    for (int r = rmin; r <= rmax; r += (rmax > rmin ? rmax - rmin : 1))
                        check_request(ct_image_off(n, s.Cw, plane), k.g_off + ct_row_off(r, s.W), s.Cw, plane, s.N, epc);
            }
        for (int i = 0; i < NCH; ++i) CHECK(covered[i]);                      // every chunk of the staged row has a lane
    }
}

// ---- the thin-image staging of ct_in_kernel (x0 = strip * CW, 18 chunks) and ct_wg_kernel (whole rows, trow / 16 chunks) -------
static void check_thin_stage(const Shape& s, int RS, int segs, int strips, bool wg, int trow) {
    const int P = s.K / 2, epc = ct_epc(s.es), CW = ct_cw(s.es);
    const int cpr = wg ? trow / 16 : CT_CHUNKS, rowb = wg ? trow : CT_ROWB;
    const long long plane = (long long)s.H * s.W;
    for (int strip = 0; strip < strips; ++strip)
        for (int seg = 0; seg < segs; ++seg) {
            const int x0 = strip * CW, ys = seg * RS, ye = ys + RS < s.H ? ys + RS : s.H;
            const int nheld = ye - ys + s.K - 1, total = nheld * s.Ct * cpr;
            const long long image_bytes = (long long)(RS + s.K - 1) * s.Ct * rowb;
            // the kernels walk id = min(id0 + u * THREADS + tid, total - 1) over whole rounds: the ids are [0, total)
            for (int id = 0; id < total; ++id) {
                const CtThinItem k = ct_thin_item(id, cpr, s.Ct, ys, P);
                const int col = wg ? ct_wg_chunk_col(k.jc, epc) : ct_in_chunk_col(x0, k.jc, epc);
                const bool ok = ct_thin_ok(k.row, col, s.H, s.W);
                const long long src = ct_thin_src(k.t, k.row, col, s.W, plane, ok);
                CHECK(k.t >= 0 && k.t < s.Ct);
                if (ok) CHECK(col + epc <= s.W && src == (long long)k.t * plane + (long long)k.row * s.W + col);
                for (int n = 0; n < s.N; n += (s.N > 1 ? s.N - 1 : 1))
                    check_request(ct_image_off(n, s.Ct, plane), src, s.Ct, plane, s.N, epc);
                CHECK((long long)k.rc * rowb + k.jc * 16 + 16 <= image_bytes);
            }
        }
}

static void check_in(const Shape& s, std::set<int>& staged, std::set<int>& stored) {
    set_ctx("ct_in", s);
    const CtGeom g = ct_geom_in(s.N, s.Ct, s.Cw, s.H, s.W, s.es, s.cus);
    const int epc = ct_epc(s.es), CW = ct_cw(s.es), CWD = s.Cw;
    const long long plane = (long long)s.H * s.W;
    CHECK(g.RS <= CT_IN_MAXRS);
    CHECK(ct_in_lds_bytes(s.K, s.Ct, s.Cw, g.RS) <= CT_LDS_LIMIT);
    // the staging reads no wide channel: one Cw
    if (s.Cw == 32 && staged.insert(g.RS).second) check_thin_stage(s, g.RS, g.segs, g.strips, false, 0);
    // the row stores: affine in the row and the image; they read neither Ct, K nor the split: once per N
    if (!(s.Ct == 1 && s.K == 3 && stored.insert(s.N).second)) return;
    for (int strip = 0; strip < g.strips; ++strip) {
        const int x0 = strip * CW;
        for (int n = 0; n < s.N; n += (s.N > 1 ? s.N - 1 : 1))
            for (int r = 0; r < s.H; r += (s.H > 1 ? s.H - 1 : 1)) {
                const long long orow = ct_in_store_row(n, s.Cw, plane, r, s.W, x0);
                for (int u = 0; u < (CWD * 16 + CT_IN_THREADS - 1) / CT_IN_THREADS; ++u)
                    for (int tid = 0; tid < CT_IN_THREADS; ++tid) {
                        const int id = u * CT_IN_THREADS + tid;
                        if (ct_in_store_live(id, CWD, x0, epc, s.W)) {
                            const long long off = orow + ct_in_store_chan_off(id, plane) + ct_in_store_col_off(id, epc);
                            CHECK(x0 + ct_in_store_col_off(id, epc) + epc <= s.W);
                            check_request(0, off - ct_image_off(n, s.Cw, plane), s.Cw, plane, 1, epc);
                            CHECK(off + epc <= (long long)s.N * s.Cw * plane);
                        }
                    }
            }
    }
}

// ---- ct_wg_kernel: the wide request.  `Wide` gives the element offset inside image n of (l16, kg, nt, q, row, xb) ------------------
struct WideNow {
    long long operator()(int l16, int kg, int nt, int q, int row, int xb, int W, long long plane) const {
        return ct_wg_wide_lane(l16, plane) + ct_wg_wide_rowcol(row, xb, kg, W) + ct_wg_wide_tile_off(nt, plane) + ct_wg_wide_half_off(q);
    }
};
// the request before the fix: 8 * kg in the lane's constant, the clamp on xb alone
struct WideBefore {
    long long operator()(int l16, int kg, int nt, int q, int row, int xb, int W, long long plane) const {
        const long long b_lane = (long long)l16 * plane + 8 * kg;
        const bool ok = xb + 8 * kg < W;
        return b_lane + (long long)row * W + (ok ? xb : 0) + (long long)nt * 16 * plane + q * 4;
    }
};
// the greatest (end of a request - end of the tensor) over the blocks of the launch, in elements: <= 0 means in bounds
template <typename Wide> static long long wide_overshoot(const Shape& s, const CtWgGeom& g, Wide wide, bool check) {
    const int epc = ct_epc(s.es), NT = s.Cw / 16, BV = s.es == 2 ? 1 : 2;
    const long long plane = (long long)s.H * s.W, total = (long long)s.N * s.Cw * plane;
    long long over = -total;
    for (int seg = 0; seg < g.segs; ++seg) {
        const int ys = seg * g.RS, ye = ys + g.RS < s.H ? ys + g.RS : s.H;
        const int nitems = (ye - ys) * g.nchunks;
        // request(d, it) takes item min(wave + 8 * it, nitems - 1) for it = 0 .. trips * CT_WPD + CT_WPD - 2: the items are [0, nitems)
        for (int i = 0; i < nitems; ++i) {
            int row, xb;
            ct_wg_item(i, g.nchunks, ys, row, xb);
            if (check) CHECK(row >= ys && row < ye && xb >= 0 && xb < s.W);
            for (int kg = 0; kg < 4; ++kg)
                for (int e = 0; e < 2; ++e) {   // the lane's channel, tile and half at their two ends (affine, non-negative)
                    const long long off = wide(e ? 15 : 0, kg, e ? NT - 1 : 0, e ? BV - 1 : 0, row, xb, s.W, plane);
                    for (int n = 0; n < s.N; n += (s.N > 1 ? s.N - 1 : 1)) {
                        const long long img = ct_image_off(n, s.Cw, plane);
                        if (check) check_request(img, off, s.Cw, plane, s.N, epc);
                        over = img + off + epc - total > over ? img + off + epc - total : over;
                    }
                }
            if (check)
                for (int kg = 0; kg < 4; ++kg) {   // the 8 pixels of a lane group: inside the row
                    const long long rc = ct_wg_wide_rowcol(row, xb, kg, s.W) - (long long)row * s.W;
                    CHECK(rc >= 0 && rc + 8 <= s.W && rc % 8 == 0);
                }
        }
    }
    return over;
}

static void check_wg(const Shape& s, std::set<int>& staged) {
    set_ctx("ct_wg", s);
    const CtWgGeom g = ct_wg_geom(s.N, s.Ct, s.Cw, s.H, s.W, s.es, s.cus);   // (returns: the halving loop ends)
    CHECK(g.RS >= 1 && g.segs >= 1 && g.trow % 16 == 0 && g.nchunks * 32 >= s.W);
    check_tiling(s.H, g.RS, g.segs);
    CHECK(ct_wg_lds_bytes(s.K, s.Cw / 16, g.RS, s.Ct, g.trow) <= CT_LDS_LIMIT);
    if (staged.insert(g.RS).second) {
        check_thin_stage(s, g.RS, g.segs, 1, true, g.trow);
        if (s.Ct == 1 && s.K == 3) CHECK(wide_overshoot(s, g, WideNow(), true) <= 0);   // the wide request reads neither Ct nor K
    }
}

static void negative_control() {
    // N = 2, H = 9, head-sized channels, 16-bit; any shape ends at the last row of the last channel of the last image
    for (int W = 8; W <= 64; W += 8) {
        Shape s{256, 2, 9, W, 2, 3, 64, 5};
        set_ctx("negative control", s);
        const CtWgGeom g = ct_wg_geom(s.N, s.Ct, s.Cw, s.H, s.W, s.es, s.cus);
        const long long before = wide_overshoot(s, g, WideBefore(), false), now = wide_overshoot(s, g, WideNow(), false);
        printf("wide request before the fix, W=%d: %lld elements past the end; now: %lld\n", W, before > 0 ? before : 0, now > 0 ? now : 0);
        CHECK(before == (W < 32 ? 32 - W : 0));
        CHECK(now == 0);
    }
}

int main() {
    static const int CUS[] = {64, 256, 304}, NS[] = {1, 2, 8, 64, 128}, HS[] = {1, 2, 7, 8, 9, 19, 67, 132, 140};
    long geoms = 0;
    for (int es = 2; es <= 4; es += 2) {
        std::vector<int> widths;
        for (int W = ct_epc(es); W <= 264; W += ct_epc(es)) widths.push_back(W);
        widths.push_back(512);
        widths.push_back(1024);
        for (int W : widths)
            for (int H : HS) {
                // the split of ct_out / ct_in reads neither the channel counts nor K: tiling and mappings once per (cus, N)
                for (int cus : CUS)
                    for (int N : NS) {
                        Shape s{cus, N, H, W, es, 3, 64, 5};
                        set_ctx("geometry", s);
                        const CtGeom go = ct_geom(N, 3, 64, H, W, es, cus), gi = ct_geom_in(N, 3, 64, H, W, es, cus);
                        check_tiling(H, go.RS, go.segs);
                        check_tiling(H, gi.RS, gi.segs);
                        check_mappings(go);
                        if (gi.RS != go.RS) check_mappings(gi);
                        geoms += 2;
                    }
                for (int K = 3; K <= 5; K += 2)
                    for (int Cw = 32; Cw <= 64; Cw += 32)
                        for (int Ct = 1; Ct <= 4 && Ct * K <= 16; ++Ct) {
                            std::set<int> out_done, in_staged, in_stored, wg_staged;
                            for (int cus : CUS)
                                for (int N : NS) {
                                    Shape s{cus, N, H, W, es, Ct, Cw, K};
                                    // ct_out reads no thin channel: one Ct; its walk depends on (RS, N > 1) alone
                                    if (Ct == 1) {
                                        const CtGeom g = ct_geom(N, Ct, Cw, H, W, es, cus);
                                        if (out_done.insert(g.RS * 2 + (N > 1)).second) check_out(s);
                                    }
                                    check_in(s, in_staged, in_stored);
                                    if (W % 8 == 0) {
                                        check_wg(s, wg_staged);
                                        ++geoms;
                                    }
                                    ++geoms;
                                }
                        }
            }
    }
    negative_control();
    printf("%ld geometries, %lld requests walked, %ld failed checks\n", geoms, walked, bad);
    return bad != 0;
}
