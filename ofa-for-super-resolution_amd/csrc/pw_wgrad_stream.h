// pw_wgrad_stream.h -- plan and address model of the streaming operand path of pw_wgrad_direct_kernel (pwconv.hip).
//
// A workgroup of 8 waves owns WS_ROWS rows of the wide operand R x the <= 64 rows of the narrow operand S over the
// 64-pixel stages of one split-K range (or of the two ranges whose slabs the reduce launch adds first).  A stage is WS_LINES lines of 128 bytes in LDS: line l < WS_ROWS is R row
// row0 + l, line WS_ROWS + s is S row s; a line holds the row's 64 pixels of the stage, i.e. eight 16-byte chunks that are
// each the 8 k-values of one MFMA fragment.  The lines are filled by LDS-DMA (global_load_lds, 16 bytes per lane): one
// wave instruction ("piece") writes 1 KiB = 8 whole lines at piece base + lane * 16, so the LDS image is lane-linear and
// the bank swizzle lives in the per-lane SOURCE address: slot j of line l holds source chunk j ^ ws_swz(l), and a
// fragment read of chunk c of line l goes to slot c ^ ws_swz(l) (the same involution on both sides).
//
// Everything here is plain integer arithmetic shared by the kernel and by tools/probe/pw_wgrad_stream_addr.cpp, which
// checks on the CPU that every source chunk lies inside its tensor, every destination inside its ring slot, every
// (line, chunk) of a stage is written exactly once and the splits tile the stages.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WS_HD __host__ __device__ inline
#else
#define WS_HD inline
#endif

namespace ofasr {

constexpr int WS_ROWS = 192;                          // R rows of a workgroup's tile
constexpr int WS_COLS = 64;                           // S rows (output columns), clamped + zeroed beyond NS
constexpr int WS_PX = 64;                             // pixels of a stage
constexpr int WS_LINES = WS_ROWS + WS_COLS;           // 128-byte lines of a stage
constexpr int WS_LINE_BYTES = 128;
constexpr int WS_STAGE_BYTES = WS_LINES * WS_LINE_BYTES;   // 32 KiB
constexpr int WS_RING = 3;                            // stages in the LDS ring
constexpr int WS_PIECE_BYTES = 1024;                  // one wave instruction: 64 lanes x 16 bytes = 8 lines
constexpr int WS_PIECES = WS_STAGE_BYTES / WS_PIECE_BYTES;   // 32: pieces [0, 24) are R lines, [24, 32) S lines
constexpr int WS_WAVES = 8;
constexpr int WS_PPW = WS_PIECES / WS_WAVES;          // pieces per wave and stage: wave w issues w, w + 8, w + 16, w + 24
constexpr int WS_PAIR_STRIDE = 16;                    // pw_wgrad_reduce_kernel adds slabs z and z + 16 first (its WR_ZL)
constexpr int WS_PAIR_GROUP = 4 * WS_PAIR_STRIDE;     // ... in groups of 64 slabs: (z + z+16) + (z+32 + z+48)

// Rows r and r + 2 of one parity share a 128-byte half of the 256-byte bank row; 16 consecutive lines (one ds_read_b128
// lane group) get 8 different chunk slots per parity, i.e. all 64 banks once.
WS_HD int ws_swz(int line) { return (line >> 1) & 7; }

// byte offset inside a ring slot of chunk `chunk` (0..7) of line `line`: the fragment read address
WS_HD int ws_frag_off(int line, int chunk) { return line * WS_LINE_BYTES + ((chunk ^ ws_swz(line)) << 4); }

// the piece that wave `wave` issues as its k-th of a stage
WS_HD int ws_piece_of(int wave, int k) { return wave + WS_WAVES * k; }

// byte offset inside a ring slot that lane `lane` of piece `piece` writes (the hardware's piece base + lane * 16)
WS_HD int ws_piece_lds(int piece, int lane) { return piece * WS_PIECE_BYTES + lane * 16; }

struct WsSrc {
    int is_s;    // 0: the R operand, 1: the S operand
    int row;     // channel row inside the operand's image, clamped into [0, rows)
    int chunk;   // 16-byte chunk of the row's 64 stage pixels
    int live;    // 0: the line lies beyond the operand's rows (its fragments are zeroed after the LDS read)
};

// what lane `lane` of piece `piece` copies, for the row tile that starts at R row `row0`
WS_HD WsSrc ws_piece_src(int piece, int lane, int row0, int MR, int NS) {
    const int line = piece * 8 + (lane >> 3);
    WsSrc s;
    s.is_s = line >= WS_ROWS;
    const int want = s.is_s ? line - WS_ROWS : row0 + line;
    const int rows = s.is_s ? NS : MR;
    s.live = want < rows;
    s.row = s.live ? want : rows - 1;
    s.chunk = (lane & 7) ^ ws_swz(line);
    return s;
}

// element offset (16-bit elements) of a source chunk inside its tensor [N][rows][HW]: stage q of the launch
WS_HD long long ws_src_elem(int q, int stages_per_img, int rows, int HW, int row, int chunk) {
    const int n = q / stages_per_img;
    const int p0 = (q - n * stages_per_img) * WS_PX;
    return ((long long)n * rows + row) * HW + p0 + chunk * 8;
}

// k-step j (0..3) of a stage takes, from lane half h, chunk j + 4h: pixels [8j, 8j + 8) and [32 + 8j, 32 + 8j + 8) -- the
// k-slot <-> pixel map of the per-lane-load body (its lane (row, h) owns pixels [32h, 32h + 32) of a quad), so that both
// bodies feed every MFMA the same operands
WS_HD int ws_kstep_chunk(int j, int h) { return j + 4 * h; }

// The split count is the per-lane-load body's (384-row tiles x splits ~ `blocks` workgroups, at least 4 stages per split):
// the streaming body forms the same partial sums.
WS_HD int ws_nsplit(int total_stages, int MR, int NS, int blocks) {
    const int tiles = ((MR + 383) / 384) * ((NS + 63) / 64);
    int want = blocks / (tiles > 0 ? tiles : 1);
    if (want > total_stages / 4) want = total_stages / 4;
    return want < 1 ? 1 : want;
}

// Whole groups of 64 splits: the reduce launch adds (p_z + p_(z+16)) + (p_(z+32) + p_(z+48)) per group and never meets a
// single slab, so a workgroup can form p_z + p_(z+16) itself and write ONE slab for the two: nsplit / 2 slabs.
WS_HD bool ws_pairs_ok(int nsplit) { return nsplit > 0 && nsplit % WS_PAIR_GROUP == 0; }

// first split z of stored slab k (the second is z + WS_PAIR_STRIDE): slab k = 32 g + 16 half + zl  <->  z = 64 g + 32 half + zl
WS_HD int ws_pair_first(int k) {
    const int g = k / (WS_PAIR_GROUP / 2), r = k % (WS_PAIR_GROUP / 2);
    return WS_PAIR_GROUP * g + 2 * WS_PAIR_STRIDE * (r / WS_PAIR_STRIDE) + r % WS_PAIR_STRIDE;
}

// stages [q0, q1) of split `split` (the formula of the direct path)
WS_HD int ws_split_begin(int split, int nsplit, int total_stages) {
    return (int)((long long)split * total_stages / nsplit);
}

// does the shape take the streaming path (the operand bases must be 16-byte aligned as well)
WS_HD bool ws_shape_ok(long long NS, long long HW) { return HW > 0 && HW % WS_PX == 0 && NS <= WS_COLS; }

}  // namespace ofasr
