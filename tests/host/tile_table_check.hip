// tile_table_check.hip -- the clamps of csrc/tile_table.h on the CPU: scatter_row / scatter_dest (plain and even) and
// window_origin over table rows made of extreme values, with the post-conditions that make every later access of the
// kernels legal.  No HIP call; tests/test_tile_table.py builds it with the host sanitizers (address, undefined: a signed
// overflow in a clamp aborts) and expects exit code 0.
#include "../../ofa-for-super-resolution_amd/csrc/tile_table.h"
#include <limits.h>

namespace ofasr {
void set_error(const char*, ...) {}
}
using namespace ofasr;

static long bad = 0;
#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond) && bad++ < 10) fprintf(stderr, "line %d: %s\n", __LINE__, #cond);   \
    } while (0)

static const long long VALS[] = {LLONG_MIN, -(1LL << 62), -5, -1, 0, 1, 3, 7, 1LL << 31, 1LL << 62, LLONG_MAX};
static const int NV = sizeof(VALS) / sizeof(VALS[0]);

struct Shape { long long sh, sw, OH, OW, max_eh, max_ew; };
static const Shape SHAPES[] = {
    {20, 28, 40, 56, 16, 24},
    {1, 1, 2, 2, 1, 1},
    {96, 96, 1LL << 20, 1LL << 20, 96, 96},               // the destination at the 2^40 cap
    {1LL << 30, 1LL << 10, 1LL << 39, 2, 1LL << 30, 2},   // the source at its own cap, a destination of two columns
};

static void check_row(const ScatterRow& r, const long long* t, const Shape& s, bool src, bool even) {
    if (src) {
        CHECK(0 <= r.sy && 0 <= r.eh && r.sy + r.eh <= s.sh);
        CHECK(0 <= r.sx && 0 <= r.ew && r.sx + r.ew <= s.sw);
    } else {
        CHECK(r.sy == t[0] && r.sx == t[1]);
    }
    CHECK(0 <= r.dy && 0 <= r.eh && r.dy + r.eh <= s.OH && r.eh <= s.max_eh);
    CHECK(0 <= r.dx && 0 <= r.ew && r.dx + r.ew <= s.OW && r.ew <= s.max_ew);
    if (even) CHECK(((r.dy | r.dx | r.eh | r.ew) & 1) == 0);
}

int main() {
    long long t[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // the row under test is row 1
    long rows = 0;
    for (int a = 0; a < NV; ++a)
        for (int b = 0; b < NV; ++b)
            for (int c = 0; c < NV; ++c)
                for (int d = 0; d < NV; ++d)
                    for (int e = 0; e < NV; ++e)
                        for (int f = 0; f < NV; ++f) {
                            t[6] = VALS[a], t[7] = VALS[b], t[8] = VALS[c], t[9] = VALS[d], t[10] = VALS[e], t[11] = VALS[f];
                            for (const Shape& s : SHAPES)
                                for (int even = 0; even < 2; ++even) {
                                    check_row(scatter_row(t, 1, s.sh, s.sw, s.OH, s.OW, s.max_eh, s.max_ew, even != 0), t + 6, s,
                                              true, even != 0);
                                    check_row(scatter_dest(t, 1, s.OH, s.OW, s.max_eh, s.max_ew, even != 0), t + 6, s, false,
                                              even != 0);
                                }
                            ++rows;
                        }
    // window_origin: (H, W, h, w), the last two with the frame at the cap and a window as large as the frame
    const long long frames[][4] = {{40, 56, 20, 28}, {2, 2, 1, 2}, {1LL << 20, 1LL << 20, 96, 96}, {1LL << 39, 2, 1LL << 39, 2}};
    long long o[4] = {0, 0, 0, 0};
    for (int a = 0; a < NV; ++a)
        for (int b = 0; b < NV; ++b) {
            o[2] = VALS[a], o[3] = VALS[b];
            for (const auto& fr : frames) {
                const WindowOrigin w = window_origin(o, 1, fr[0], fr[1], fr[2], fr[3]);
                CHECK(0 <= w.y0 && w.y0 <= fr[0] - fr[2]);
                CHECK(0 <= w.x0 && w.x0 <= fr[1] - fr[3]);
            }
        }
    // the slab split covers [0, nrows) once, in order
    for (long long nrows = 1; nrows <= 70; ++nrows)
        for (long long S = 1; S <= WINDOW_MAX_SLABS && S <= nrows; ++S) {
            long long next = 0;
            for (long long s = 0; s < S; ++s) {
                long long lo, hi;
                slab_rows(nrows, s, S, lo, hi);
                CHECK(lo == next && lo <= hi && hi <= nrows);
                next = hi;
            }
            CHECK(next == nrows);
        }
    CHECK(window_slabs(0, 5, 16384) == 0 && window_slabs(1, 1, 16384) == 1 && window_slabs(3, 1LL << 40, 16384) == 3);
    CHECK(window_slabs(1LL << 20, 1LL << 20, 16384) == WINDOW_MAX_SLABS && window_slabs(LLONG_MAX, LLONG_MAX, 16384) == WINDOW_MAX_SLABS);
    printf("%ld scatter rows x %d shapes x 2 variants, %ld failed checks\n", rows, (int)(sizeof(SHAPES) / sizeof(SHAPES[0])), bad);
    return bad != 0;
}
