// Stand-alone check of genpc_amd/csrc/ws_layout.h (host code only; tests/test_ws_layout.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints its line.
// What it is not: the three "library" layouts below are copies of the piece lists of icp.hip, nn_seeded.hip and pose.hip with
// stand-in struct sizes (those files need HIP).  They pin the helper's arithmetic to the hand-written arithmetic it replaced; a
// later edit to a real site or struct does not fail here -- the GPU suite's bit-exact tests cover the sites themselves.
#include "ws_layout.h"

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

using genpc::WsLayout;

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { printf("FAILED line %d: %s\n", __LINE__, #cond); g_failed++; } \
    } while (0)

// stand-ins of the device structs, by size (csrc/icp.hip IcpState, csrc/pose.h PoseState, csrc/grid.h CellGridHdr, float4)
struct IcpState { char x[24]; };
struct PoseState { char x[236]; };
struct CellGridHdr { char x[52]; };
struct Float4 { char x[16]; };
constexpr size_t kCellGridMaxCells = 15360, kAcc = 48;

struct Piece { const void *p; size_t bytes; };

// 256-aligned, inside the block, pairwise disjoint (sizes rounded up to 256, as the helper reserves them)
static void check_pieces(const Piece *v, int n, const char *base, size_t total)
{
    for (int i = 0; i < n; i++) {
        const char *a = (const char *)v[i].p;
        const size_t la = WsLayout::up(v[i].bytes);
        CHECK(((uintptr_t)a & 255) == 0);
        CHECK(a >= base && a + la <= base + total);
        for (int j = 0; j < i; j++) {
            const char *b = (const char *)v[j].p;
            const size_t lb = WsLayout::up(v[j].bytes);
            CHECK(la == 0 || lb == 0 || a + la <= b || b + lb <= a);
        }
    }
}

static void check_offsets(void *const *ptrs, const size_t *want, int n, const char *base)
{
    for (int i = 0; i < n; i++) CHECK((size_t)((const char *)ptrs[i] - base) == want[i]);
}

int main()
{
    // a block as the pool hands it out: 256-byte aligned
    const size_t cap = 1 << 20;
    char *base = (char *)aligned_alloc(256, cap);
    if (!base) return 2;

    {   // a header with hand-placed fields, absent pieces, a piece of no elements, a nested layout inside a piece of the parent
        int *status; double *a; float *absent = (float *)base; short *odd; char *empty; char *block; int *tail_absent = (int *)base; Float4 *last;
        float *in0; unsigned char *in1; double *in_absent = (double *)base;
        WsLayout inner;
        inner.add(in0, 77);
        inner.add_if(false, in_absent, 1000);
        inner.add(in1, 300);
        CHECK(inner.bytes() == 512 + 512);
        WsLayout L;
        L.add(status, 64);
        L.add(a, 33);
        L.add_if(false, absent, 12345);
        L.add(odd, 129);
        L.add(empty, 0);
        L.add(block, inner.bytes());
        L.add_if(false, tail_absent, 1);
        L.add(last, 1);
        CHECK(L.ok());
        CHECK(status == nullptr && last == nullptr);          // nothing is handed out before bind
        const size_t before = L.bytes();
        CHECK(before == 256 + 512 + 512 + 0 + 1024 + 256);
        CHECK(before <= cap);
        L.bind(base);
        inner.bind(block);
        CHECK(L.bytes() == before && inner.bytes() == 1024);
        CHECK(absent == nullptr && tail_absent == nullptr && in_absent == nullptr);
        CHECK((char *)status == base);
        CHECK(empty == block);                                // a piece of no elements points at its successor
        const Piece v[] = {{status, 256}, {a, 33 * 8}, {odd, 129 * 2}, {block, 1024}, {last, 16}};
        check_pieces(v, 5, base, before);
        const Piece w[] = {{in0, 77 * 4}, {in1, 300}};
        check_pieces(w, 2, block, 1024);
        // the fields of the header stay where their owner puts them
        unsigned *bounds = (unsigned *)(status + 16);
        CHECK((char *)bounds - base == 64 && (char *)(status + 48) - base == 192);
    }

    {   // an unrounded tail: taken as it is, and it closes the layout
        int *x; char *t; int *more = (int *)base;
        WsLayout L;
        L.add(x, 1);
        CHECK(L.add_tail(t, 1000));
        CHECK(L.bytes() == 256 + 1000);
        CHECK(!L.add(more, 1));
        CHECK(!L.ok() && L.bytes() == 256 + 1000 && more == nullptr);
    }

    {   // the capacity: the piece beyond it is refused and reported, nothing is written past the tables
        int *p[WsLayout::kMaxPieces + 2];
        WsLayout L;
        for (int i = 0; i < WsLayout::kMaxPieces; i++) CHECK(L.add(p[i], 1));
        CHECK(L.ok());
        const size_t full = L.bytes();
        CHECK(full == (size_t)WsLayout::kMaxPieces * 256);
        CHECK(!L.add(p[WsLayout::kMaxPieces], 1));
        CHECK(!L.add_if(true, p[WsLayout::kMaxPieces + 1], 1));
        CHECK(!L.ok() && L.bytes() == full);
        L.bind(base);
        CHECK(p[WsLayout::kMaxPieces] == nullptr && p[WsLayout::kMaxPieces + 1] == nullptr);
        CHECK((char *)p[WsLayout::kMaxPieces - 1] - base == (ptrdiff_t)(full - 256));
    }

    // Three layouts of the library against the offsets their hand-written arithmetic gave before the helper existed
    // (sum of sizes each rounded up to 256, in order).
    {   // genpc_icp_batch, launch-per-pass path: k = 3, ns = 1000, nt = 777
        const size_t k = 3, ns = 1000, nt = 777;
        double *accum; IcpState *state; float *pts, *tgt, *d; int *idx;
        WsLayout L;
        L.add(accum, k * 17);
        L.add(state, k);
        L.add(pts, k * ns * 3);
        L.add(tgt, k * nt * 3);
        L.add(d, k * ns);
        L.add(idx, k * ns);
        CHECK(L.ok() && L.bytes() == 89088);
        L.bind(base);
        void *const got[] = {accum, state, pts, tgt, d, idx};
        const size_t want[] = {0, 512, 768, 36864, 65024, 77056};
        check_offsets(got, want, 6, base);
    }
    {   // seeded_grids_layout: b = 2, nm = 300 (moving), ns = 5000 (static)
        const size_t b = 2, nm = 300, ns = 5000;
        const CellGridHdr *hdr_static, *hdr_rest; const int *start_static, *start_rest; const Float4 *sorted_static, *sorted_rest;
        WsLayout L;
        L.add(hdr_static, b);
        L.add(hdr_rest, b);
        L.add(start_static, b * (kCellGridMaxCells + 1));
        L.add(start_rest, b * (kCellGridMaxCells + 1));
        L.add(sorted_static, b * ns);
        L.add(sorted_rest, b * nm);
        CHECK(L.ok() && L.bytes() == 416512);
        L.bind(base);
        void *const got[] = {(void *)hdr_static, (void *)hdr_rest, (void *)start_static, (void *)start_rest, (void *)sorted_static, (void *)sorted_rest};
        const size_t want[] = {0, 256, 512, 123648, 246784, 406784};
        check_offsets(got, want, 6, base);
    }
    {   // genpc_pose_optimize_batch without the mask term: b = 4 (elements), nc = 4493, np = 886
        const size_t b = 4, nc = 4493, np = 886;
        double *accum; PoseState *S; float *center, *pts, *d1, *d2; int *i1, *i2;
        WsLayout L;
        L.add(accum, 2 * b * kAcc);
        L.add(S, 2 * b);
        L.add(center, b * 4);
        L.add(pts, b * nc * 3);
        L.add(d1, b * nc);
        L.add(d2, b * np);
        L.add(i1, b * nc);
        L.add(i2, b * np);
        CHECK(L.ok() && L.bytes() == 393728);
        L.bind(base);
        void *const got[] = {accum, S, center, pts, d1, d2, i1, i2};
        const size_t want[] = {0, 3072, 5120, 5376, 221184, 293120, 307456, 379392};
        check_offsets(got, want, 8, base);
    }

    free(base);
    if (g_failed) {
        printf("ws_layout_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("ws_layout_check: ok\n");
    return 0;
}
