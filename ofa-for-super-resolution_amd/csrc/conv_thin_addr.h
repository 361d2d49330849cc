// conv_thin_addr.h -- what the thin-side convolutions of conv_thin.hip decide from integers alone, each rule stated once:
//   ct_geom / ct_geom_in / ct_wg_geom     the work split (column strips, row segments, rows per segment) of a shape on a
//                                         device of `cus` compute units;
//   ct_block_map (_xcd / _plain)          blockIdx -> (strip, unit): the XCD-ordered mapping and the plain one;
//   ct_out_chunk, ct_out_request_row, ct_out_prologue_row, ct_row_off
//                                         the staged-row requests of ct_out_kernel;
//   ct_thin_item, ct_in_chunk_col, ct_wg_chunk_col, ct_thin_ok, ct_thin_src
//                                         the thin-image staging loads of ct_in_kernel and ct_wg_kernel;
//   ct_in_store_live, ct_in_store_row, ct_in_store_chan_off / ct_in_store_col_off, ct_image_off
//                                         the 16-byte row stores of ct_in_kernel;
//   ct_wg_item, ct_wg_wide_lane, ct_wg_wide_rowcol, ct_wg_wide_tile_off, ct_wg_wide_half_off   the wide-operand request of ct_wg_kernel;
//   ct_out_lds_bytes / ct_in_lds_bytes / ct_wg_lds_bytes      the dynamic LDS the launchers ask for.
// Every request above is issued by a lane whether or not its value is used (a masked lane's value is zeroed AFTER the
// load), so each offset must lie inside the tensor for every lane: the rule is "clamp the whole address, then mask".
// All of it is __host__ __device__ integer arithmetic: tests/host/conv_thin_addr_check.hip walks every block, lane and
// item of a sweep of shapes on the CPU and asserts bounds, alignment, tiling and the LDS budget.  Everything is
// __forceinline__ and changes no access width.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ofasr {

constexpr int CT_ROWB = 288;             // bytes per channel row of a staged image row: 18 chunks of 16 B (72 dwords = 8 mod 64:
                                         // the 8 channel rows a half-wave's transposing read touches fall on disjoint banks)
constexpr int CT_CHUNKS = 18;
constexpr int CT_D = 4;                  // image rows requested ahead of the one being computed
constexpr int CT_PSTRIDE = 148;          // floats per row of the P image (4 * 148 = 16 mod 32: the two 16-lane groups of a
                                         // half-wave store to disjoint banks)
constexpr int CT_PSTRIDE_F32 = 84;       // the same for the fp32 kernel's 5 column tiles (4 * 84 = 16 mod 32)
constexpr int CT_IN_THREADS = 512;
constexpr int CT_OSTR = 272;             // bytes per channel row of the output tile: 68 dwords = 4 mod 32 (2-way at worst, the minimum)
constexpr int CT_IN_MAXRS = 64;
constexpr int CT_WG_THREADS = 512;
constexpr int CT_WG_HALO = 8;            // thin image of the weight gradient: column index = column + CT_WG_HALO
constexpr size_t CT_LDS_LIMIT = 160 * 1024 - 256;   // what every launcher raises the dynamic LDS limit to

// CW: output columns per strip; EPC: elements per 16-byte chunk, by element size (2: bf16 / f16, 4: fp32).  A staged row
// holds CT_CHUNKS * EPC columns starting at column x0 - EPC (one chunk of left halo, one of right halo).
__host__ __device__ constexpr int ct_cw(int es) { return es == 2 ? 128 : 64; }
__host__ __device__ constexpr int ct_epc(int es) { return 16 / es; }

__host__ __device__ __forceinline__ int64_t ct_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct CtGeom {
    int N, H, W;        // images, rows, columns
    int Ct, Cw;         // thin / wide channel counts
    int strips, segs, RS;   // column strips per row, row segments per image, rows per segment
};

// one workgroup per CU: as few row segments as that allows (every segment re-reads 2 * (k / 2) halo rows), of 8 rows at least
__host__ __device__ __forceinline__ CtGeom ct_geom(int64_t N, int64_t Ct, int64_t Cw, int64_t H, int64_t W, int es, int cus) {
    CtGeom g{};
    g.N = (int)N; g.H = (int)H; g.W = (int)W; g.Ct = (int)Ct; g.Cw = (int)Cw;
    g.strips = (int)ct_cdiv(W, ct_cw(es));
    const int64_t units = N * g.strips;
    int64_t segs = ct_cdiv(cus, units);
    int64_t RS = ct_cdiv(H, segs < 1 ? 1 : segs);
    if (RS < 8) RS = H < 8 ? H : 8;
    g.RS = (int)RS;
    g.segs = (int)ct_cdiv(H, RS);
    return g;
}

// ct_in_kernel holds the thin rows of a whole segment in LDS: at most CT_IN_MAXRS rows
__host__ __device__ __forceinline__ CtGeom ct_geom_in(int64_t N, int64_t Ct, int64_t Cw, int64_t H, int64_t W, int es, int cus) {
    CtGeom g = ct_geom(N, Ct, Cw, H, W, es, cus);
    if (g.RS > CT_IN_MAXRS) {
        g.RS = CT_IN_MAXRS;
        g.segs = (int)ct_cdiv(H, g.RS);
    }
    return g;
}

struct CtWgGeom {
    int N, H, W, Ct, Cw;
    int segs, RS;          // row segments per image, rows per segment
    int nchunks;           // 32-pixel chunks per row
    int trow;              // bytes per (row, channel) of the thin LDS image: (W + 16 + pad) elements
};

__host__ __device__ __forceinline__ CtWgGeom ct_wg_geom(int64_t N, int64_t Ct, int64_t Cw, int64_t H, int64_t W, int es, int cus) {
    CtWgGeom g{};
    g.N = (int)N; g.H = (int)H; g.W = (int)W; g.Ct = (int)Ct; g.Cw = (int)Cw;
    g.nchunks = (int)ct_cdiv(W, 32);
    // bytes per (row, channel): columns -8 .. 32 * nchunks + 8 + 2 (the funnel shift reads one dword further)
    g.trow = (int)((32 * g.nchunks + 24) * es + 15) / 16 * 16;
    int64_t segs = ct_cdiv(cus, N);
    int64_t RS = ct_cdiv(H, segs < 1 ? 1 : segs);
    // a block's fixed costs (thin image, the waves' fold, its 20 KB slab) want >= 8 items per wave
    const int64_t min_rows = ct_cdiv(64, g.nchunks);
    if (RS < min_rows) RS = H < min_rows ? H : min_rows;
    // the thin image of a segment must fit LDS: halve the segment until it does (ends at RS <= 4 at the latest; RS >= 1)
    while (RS > 4 && (RS + 4) * Ct * g.trow > 96 * 1024) RS = (RS + 1) / 2;
    g.RS = (int)RS;
    g.segs = (int)ct_cdiv(H, RS);
    return g;
}

// ---- blockIdx -> (strip, unit), unit = image * segs + segment -----------------------------------------------------------
// The strips of one (image, segment) request each other's edge lines (a 16-byte halo chunk lies in the neighbour's
// 128-byte line), so they must share an L2: workgroups go to the 8 XCDs round robin by blockIdx, hence the strips of
// a unit are 8 apart in blockIdx and run side by side on one XCD (measured without: 1.95x the algorithmic reads).
__host__ __device__ __forceinline__ void ct_block_map_xcd(int b, int strips, int& strip, int& unit) {   // units % 8 == 0
    const int grp = b / (8 * strips), rem = b % (8 * strips);
    strip = rem / 8;
    unit = grp * 8 + rem % 8;
}
__host__ __device__ __forceinline__ void ct_block_map_plain(int b, int strips, int& strip, int& unit) {
    strip = b % strips;
    unit = b / strips;
}
__host__ __device__ __forceinline__ bool ct_block_map_is_xcd(int units) { return units % 8 == 0; }
__host__ __device__ __forceinline__ void ct_block_map(int b, int units, int strips, int& strip, int& unit) {
    if (ct_block_map_is_xcd(units)) ct_block_map_xcd(b, strips, strip, unit);
    else ct_block_map_plain(b, strips, strip, unit);
}

// ---- ct_out_kernel: 16-byte chunk `id` (< Cw * CT_CHUNKS) of a staged image row ------------------------------------------
struct CtOutChunk {
    int c, jc;          // channel, chunk of the staged row
    bool col_ok;        // the chunk's columns lie inside the image row
    long long g_off;    // element offset inside an image row of X (channel * plane + CLAMPED column)
};
__host__ __device__ __forceinline__ CtOutChunk ct_out_chunk(int id, int x0, int epc, int W, long long plane) {
    CtOutChunk k;
    k.c = id / CT_CHUNKS;
    k.jc = id % CT_CHUNKS;
    const int col = x0 - epc + k.jc * epc;
    k.col_ok = col >= 0 && col < W;
    k.g_off = (long long)k.c * plane + (k.col_ok ? col : 0);
    return k;
}
// rows above / below the image are zero (handled at the LDS write); the request itself goes to a clamped row, and rows
// beyond what this segment needs re-request the last needed row (a cache hit, no HBM traffic)
__host__ __device__ __forceinline__ int ct_out_request_row(int row, int ye, int P, int H) {
    const int last = ye - 1 + P < H - 1 ? ye - 1 + P : H - 1;   // the same for every row of a block
    const int r = row < last ? row : last;
    return r > 0 ? r : 0;
}
// row i of the prologue's k rows ys - P .. ys + P
__host__ __device__ __forceinline__ int ct_out_prologue_row(int ys, int P, int i, int H) {
    const int r = ys - P + i < H - 1 ? ys - P + i : H - 1;
    return r > 0 ? r : 0;
}
// a request's element offset inside image n: the chunk's g_off + the row's offset (added to the pointer in that order:
// the first sum is the same for every row)
__host__ __device__ __forceinline__ long long ct_row_off(int r, int W) { return (long long)r * W; }

// ---- thin-image staging of ct_in_kernel and ct_wg_kernel: chunk `id` of [held row][thin channel][cpr chunks] ----------------
struct CtThinItem { int jc, rc, t, row; };   // chunk of the row, (held row, channel) index, channel, image row
__host__ __device__ __forceinline__ CtThinItem ct_thin_item(int id, int cpr, int Ct, int ys, int P) {
    CtThinItem it;
    it.jc = id % cpr;
    it.rc = id / cpr;
    it.t = it.rc % Ct;
    it.row = ys - P + it.rc / Ct;
    return it;
}
// Four rules of ct_in_kernel are macros with a function on top.  hipcc compiles that kernel measurably differently (more
// SGPRs, another schedule: +4 % on the head's 16-bit input gradient) when these four sit behind a call, inlined or not,
// so the kernel expands the macro -- the same tokens it always had -- and everything else (the CPU check, ct_wg_kernel)
// calls the function.  Either way the rule is written once.  CT_IN_STORE_ROW is deliberately NOT parenthesised as a
// whole: `out + CT_IN_STORE_ROW(...)` must stay a chain of pointer additions; use it in no other context.
#define CT_CHUNK_COL(x0, jc, epc) ((x0) - (epc) + (jc) * (epc))
#define CT_THIN_OK(row, col, H, W) ((row) >= 0 && (row) < (H) && (col) >= 0 && (col) < (W))
#define CT_IN_STORE_LIVE(id, ch, cwd, x0, epc, W) ((id) < (cwd) * 16 && (x0) + (ch) * (epc) < (W))
#define CT_IN_STORE_ROW(n, Cw, plane, r, W, x0) (long long)(n) * (Cw) * (plane) + (long long)(r) * (W) + (x0)
__host__ __device__ __forceinline__ int ct_in_chunk_col(int x0, int jc, int epc) { return CT_CHUNK_COL(x0, jc, epc); }
__host__ __device__ __forceinline__ int ct_wg_chunk_col(int jc, int epc) { return jc * epc - CT_WG_HALO; }
// a chunk inside the image (its columns are all in or all out: W is a multiple of the chunk's elements) ...
__host__ __device__ __forceinline__ bool ct_thin_ok(int row, int col, int H, int W) { return CT_THIN_OK(row, col, H, W); }
// ... and its element offset inside image n of the thin tensor; a chunk outside requests (t, 0, 0) and is zeroed afterwards
__host__ __device__ __forceinline__ long long ct_thin_src(int t, int row, int col, int W, long long plane, bool ok) {
    return (long long)t * plane + (long long)(ok ? row : 0) * W + (ok ? col : 0);
}

// ---- ct_in_kernel: 16-byte row stores of the [channel][16 chunks] output tile, item id = u * CT_IN_THREADS + tid -------------
// an item is stored when it is one of the tile's and its chunk (ch = id & 15) starts inside the row: then it ends inside it
// too, W being a multiple of the chunk's elements
__host__ __device__ __forceinline__ bool ct_in_store_live(int id, int cwd, int x0, int epc, int W) {
    return CT_IN_STORE_LIVE(id, id & 15, cwd, x0, epc, W);
}
// element offset of (image n, row r, column x0) of the result; the item's channel and chunk offsets are added to the pointer
__host__ __device__ __forceinline__ long long ct_in_store_row(int n, int Cw, long long plane, int r, int W, int x0) {
    return CT_IN_STORE_ROW(n, Cw, plane, r, W, x0);
}
// element offset of image n of a tensor of C channels
__host__ __device__ __forceinline__ long long ct_image_off(int n, int C, long long plane) { return (long long)n * C * plane; }
__host__ __device__ __forceinline__ long long ct_in_store_chan_off(int id, long long plane) { return (long long)(id >> 4) * plane; }
__host__ __device__ __forceinline__ int ct_in_store_col_off(int id, int epc) { return (id & 15) * epc; }

// ---- ct_wg_kernel: the wide operand, 8 pixels xb + 8 kg .. + 7 of row `row`, channel 16 nt + l16 -----------------------------
// item i of a block: (row, first pixel of its 32-pixel chunk)
__host__ __device__ __forceinline__ void ct_wg_item(int i, int nchunks, int ys, int& row, int& xb) {
    row = ys + i / nchunks;
    xb = 32 * (i % nchunks);
}
__host__ __device__ __forceinline__ long long ct_wg_wide_lane(int l16, long long plane) { return (long long)l16 * plane; }
// (W % 8 == 0: the 8 pixels are all in or all out.)  The WHOLE column is clamped: a lane group beyond the row's end
// requests the row's first pixels.  With 8 kg outside the select, W = 8, 16, 24 put the groups kg >= W / 8 at column
// 8 kg >= W -- on the last row of the last channel of the last image 24, 16, 8 elements past the tensor's end.
__host__ __device__ __forceinline__ long long ct_wg_wide_rowcol(int row, int xb, int kg, int W) {
    const bool ok = xb + 8 * kg < W;
    return (long long)row * W + (ok ? xb + 8 * kg : 0);
}
// channel tile nt and request q (fp32: two per lane) from there
__host__ __device__ __forceinline__ long long ct_wg_wide_tile_off(int nt, long long plane) { return (long long)nt * 16 * plane; }
__host__ __device__ __forceinline__ int ct_wg_wide_half_off(int q) { return q * 4; }

// ---- dynamic LDS ----------------------------------------------------------------------------------------------------------
__host__ __device__ constexpr int ct_out_ring_rows(bool is16, int K) { return is16 ? K + 1 : K; }
__host__ __device__ constexpr int ct_out_planes(bool is16, int K, int NC) { return is16 ? 2 : K * NC; }
__host__ __device__ constexpr size_t ct_out_lds_bytes(bool is16, int K, int NC) {
    return (size_t)ct_out_ring_rows(is16, K) * 32 * NC * CT_ROWB +
           (size_t)ct_out_planes(is16, K, NC) * 16 * (is16 ? CT_PSTRIDE : CT_PSTRIDE_F32) * sizeof(float);
}
__host__ __device__ constexpr size_t ct_in_lds_bytes(int K, int Ct, int Cw, int RS) {
    return (size_t)(RS + K - 1) * Ct * CT_ROWB + 2 * (size_t)Cw * CT_OSTR + 64;
}
// the thin image of the segment, or the slab the waves fold into (it re-uses the image's space), whichever is larger
__host__ __device__ constexpr size_t ct_wg_lds_bytes(int K, int NT, int RS, int Ct, int trow) {
    const size_t img = (size_t)(RS + K - 1) * Ct * trow, slab = (size_t)K * NT * 256 * sizeof(float);
    return img < slab ? slab : img;
}

}  // namespace ofasr
