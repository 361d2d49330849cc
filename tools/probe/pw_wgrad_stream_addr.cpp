// pw_wgrad_stream_addr.cpp -- CPU check of the address model of the streaming pointwise weight gradient
// (csrc/pw_wgrad_stream.h, used by pw_wgrad_direct_kernel).  No GPU, no HIP: the header is plain integer arithmetic.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I ofa-for-super-resolution_amd/csrc tools/probe/pw_wgrad_stream_addr.cpp -o tools/probe/pw_wgrad_stream_addr.bin
//   tools/probe/pw_wgrad_stream_addr.bin
//
// For every shape of tests/test_hip_pw_wgrad_stream.py (and the flagship) it walks every workgroup, stage, wave, piece and
// lane exactly as the kernel does and asserts that
//   * every 16-byte source chunk lies inside its tensor (the copy is made from real host arrays, so the address
//     sanitizer sees every byte read as well),
//   * every LDS destination lies inside its ring slot and every (line, chunk) of a stage is written exactly once,
//   * a fragment read through ws_frag_off() returns the chunk the MFMA k-slot wants (source and read swizzle agree),
//   * the splits tile the stages exactly, and the flagship plans at most 128 slabs.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "pw_wgrad_stream.h"

using namespace ofasr;

#define CHECK(c, ...)                                                          \
    do {                                                                       \
        if (!(c)) {                                                            \
            fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #c);     \
            fprintf(stderr, __VA_ARGS__);                                      \
            fprintf(stderr, "\n");                                             \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

struct Shape {
    int N, NS, MR, HW;
};

// element value that names its own position: tensor tag, image, row, pixel / 8
static uint16_t tag16(int is_s, long long elem) { return (uint16_t)((elem * 2654435761u + (is_s ? 0x5bd1u : 0)) >> 7); }

static void check_shape(const Shape& sh, int blocks) {
    const int N = sh.N, NS = sh.NS, MR = sh.MR, HW = sh.HW;
    CHECK(ws_shape_ok(NS, HW), "shape (%d, %d, %d, %d) is not a streaming shape", N, NS, MR, HW);
    const int spi = HW / WS_PX, total = N * spi;
    const int nsplit = ws_nsplit(total, MR, NS, blocks);
    const int tiles = (MR + WS_ROWS - 1) / WS_ROWS;
    CHECK(nsplit >= 1 && nsplit <= total, "nsplit %d of %d stages", nsplit, total);
    // the stage lists of the stored slabs (one split, or with pairs the splits z and z + 16) cover every stage once
    const bool pairs = ws_pairs_ok(nsplit);
    const int stored = pairs ? nsplit / 2 : nsplit;
    std::vector<int> seen((size_t)total), split_seen((size_t)nsplit);
    for (int k = 0; k < stored; ++k) {
        const int za = pairs ? ws_pair_first(k) : k;
        for (int z = za; z <= (pairs ? za + WS_PAIR_STRIDE : za); z += WS_PAIR_STRIDE) {
            CHECK(z >= 0 && z < nsplit && split_seen[(size_t)z]++ == 0, "slab %d: split %d of %d", k, z, nsplit);
            const int q0 = ws_split_begin(z, nsplit, total), q1 = ws_split_begin(z + 1, nsplit, total);
            CHECK(0 <= q0 && q0 < q1 && q1 <= total, "split %d of %d is [%d, %d)", z, nsplit, q0, q1);
            for (int q = q0; q < q1; ++q) seen[(size_t)q]++;
        }
        // slab k is what the reduce launch's pair branch reads as (group g, half, lane zl)
        if (pairs) CHECK(za % WS_PAIR_GROUP < WS_PAIR_STRIDE || (za % WS_PAIR_GROUP >= 2 * WS_PAIR_STRIDE && za % WS_PAIR_GROUP < 3 * WS_PAIR_STRIDE), "slab %d starts at split %d", k, za);
    }
    for (int q = 0; q < total; ++q) CHECK(seen[(size_t)q] == 1, "stage %d is walked %d times", q, seen[(size_t)q]);
    // the k-steps of a stage take every chunk once, in the per-lane-load body's order
    {
        int used[8] = {0};
        for (int j = 0; j < 4; ++j)
            for (int h = 0; h < 2; ++h) used[ws_kstep_chunk(j, h)]++;
        for (int ch = 0; ch < 8; ++ch) CHECK(used[ch] == 1, "chunk %d is used %d times", ch, used[ch]);
    }
    // the tensors, exactly sized: one element past either end is an address-sanitizer report
    const long long rn = (long long)N * MR * HW, sn = (long long)N * NS * HW;
    std::vector<uint16_t> R((size_t)rn), S((size_t)sn);
    for (long long i = 0; i < rn; ++i) R[(size_t)i] = tag16(0, i);
    for (long long i = 0; i < sn; ++i) S[(size_t)i] = tag16(1, i);
    std::vector<unsigned char> ring((size_t)WS_RING * WS_STAGE_BYTES);
    std::vector<int> written((size_t)WS_STAGE_BYTES / 16);
    long long chunks = 0;
    for (int tile = 0; tile < tiles; ++tile) {
        const int row0 = tile * WS_ROWS;
        for (int q = 0; q < total; ++q) {
            const int slot = q % WS_RING;
            unsigned char* sl = ring.data() + (size_t)slot * WS_STAGE_BYTES;
            memset(written.data(), 0, written.size() * sizeof(int));
            for (int wave = 0; wave < WS_WAVES; ++wave)
                for (int k = 0; k < WS_PPW; ++k) {
                    const int piece = ws_piece_of(wave, k);
                    CHECK(piece >= 0 && piece < WS_PIECES, "piece %d", piece);
                    for (int lane = 0; lane < 64; ++lane) {
                        const WsSrc s = ws_piece_src(piece, lane, row0, MR, NS);
                        CHECK((k == WS_PPW - 1) == (s.is_s != 0), "wave %d piece %d: the kernel takes its last piece from S", wave, k);
                        const int rows = s.is_s ? NS : MR;
                        CHECK(s.row >= 0 && s.row < rows && s.chunk >= 0 && s.chunk < 8, "row %d chunk %d", s.row, s.chunk);
                        const long long e = ws_src_elem(q, spi, rows, HW, s.row, s.chunk);
                        CHECK(e >= 0 && e + 8 <= (s.is_s ? sn : rn), "source [%lld, +8) outside a tensor of %lld", e, s.is_s ? sn : rn);
                        CHECK(e % 8 == 0, "source element %lld is not 16-byte aligned", e);
                        const int d = ws_piece_lds(piece, lane);
                        CHECK(d >= 0 && d + 16 <= WS_STAGE_BYTES && d % 16 == 0, "LDS offset %d", d);
                        CHECK((d >> 7) == piece * 8 + (lane >> 3), "a piece crosses a line");
                        CHECK(written[(size_t)d / 16]++ == 0, "LDS chunk %d written twice", d / 16);
                        memcpy(sl + d, (s.is_s ? S.data() : R.data()) + e, 16);
                        ++chunks;
                    }
                }
            for (size_t i = 0; i < written.size(); ++i) CHECK(written[i] == 1, "LDS chunk %zu written %d times", i, written[i]);
            // every fragment the kernel reads: line, k-step s (4 of 16 pixels), half h -> chunk 2 s + h
            const int n = q / spi, p0 = (q - n * spi) * WS_PX;
            for (int line = 0; line < WS_LINES; ++line)
                for (int chunk = 0; chunk < 8; ++chunk) {
                    const int off = ws_frag_off(line, chunk);
                    CHECK(off >= 0 && off + 16 <= WS_STAGE_BYTES && (off >> 7) == line, "fragment offset %d of line %d", off, line);
                    const bool is_s = line >= WS_ROWS;
                    const int want = is_s ? line - WS_ROWS : row0 + line, rows = is_s ? NS : MR;
                    if (want >= rows) continue;   // zeroed after the read
                    const long long e = ((long long)n * rows + want) * HW + p0 + chunk * 8;
                    CHECK(memcmp(sl + off, (is_s ? S.data() : R.data()) + e, 16) == 0,
                          "line %d chunk %d of stage %d holds the wrong pixels", line, chunk, q);
                }
        }
    }
    printf("ok  N=%d NS=%d MR=%d HW=%d: %d tiles x %d splits over %d stages, %lld chunks\n", N, NS, MR, HW, tiles, nsplit, total,
           chunks);
}

int main() {
    const Shape shapes[] = {
        {1, 64, 384, 64},   {1, 64, 384, 192},  {2, 64, 192, 1024}, {2, 64, 256, 2304},
        {3, 64, 384, 4096}, {1, 60, 380, 128},  {1, 64, 384, 832},  {1, 1, 1, 64},
    };
    for (const Shape& s : shapes) check_shape(s, 256);
    check_shape(Shape{1, 64, 384, 832}, 7);     // a split count that does not divide the stages
    // the flagship: N = 16, 64 <-> 384 channels at 64 x 64 -- at most 128 slabs (plan only; the walk above covers the shapes)
    const int total = 16 * (4096 / WS_PX);
    const int nsp = ws_nsplit(total, 384, 64, 256);
    CHECK(ws_pairs_ok(nsp), "flagship: %d splits do not pair", nsp);
    const int ns = nsp / 2;
    CHECK(ns <= 128 && ns * ((384 + WS_ROWS - 1) / WS_ROWS) == 256, "flagship plans %d slabs", ns);
    check_shape(Shape{16, 64, 384, 4096}, 256);   // the flagship itself: paired splits
    printf("ok  flagship: %d splits, %d slabs, %d workgroups\n", nsp, ns, ns * 2);
    return 0;
}
