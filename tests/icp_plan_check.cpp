// Stand-alone check of genpc_amd/csrc/icp_plan.h (host code only; tests/test_icp_plan.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
// The boundaries below are literals worked out by hand from the kernel's LDS layout, no second copy of the header's expressions:
//   fixed part: 1024 queries x 16 + 1024 keys x 8 + 16 waves x 512 pairs x 4 + 17 sums x 16 waves x 8 + transform 128 + sums 136
//             = 16384 + 8192 + 32768 + 2176 + 128 + 136 = 59784 bytes
//   budget:     160 KiB - 1024 (the kernel's __shared__ variables) - 59784 = 103032 bytes for the cloud (16 bytes a point,
//               padded to a multiple of four points) and the cells (4 bytes each)
//   8192 cells: (103032 - 32768) / 16 = 4391.5 -> 4388 points     4096: (103032 - 16384) / 16 = 5415.5 -> 5412
//   2048 cells: (103032 -  8192) / 16 = 5927.5 -> 5924            1024: (103032 -  4096) / 16 = 6183.5 -> 6180
#include "icp_plan.h"

#include <stdio.h>

using namespace genpc;

static int g_failed = 0;

static void expect(const char *what, int nt, long long got, long long want)
{
    if (got != want) { printf("FAILED nt %d: %s = %lld, expected %lld\n", nt, what, got, want); g_failed++; }
}

static void row(int nt, int one, int cells, int lds)
{
    const IcpPlan p = icp_plan(nt);
    expect("one_workgroup", nt, p.one_workgroup, one);
    expect("cells", nt, p.cells, cells);
    expect("lds_bytes", nt, p.lds_bytes, lds);
}

int main()
{
    // each budget's last nt, the first nt of the next, the first multi-launch nt (lds = padded points x 16 + cells x 4 + 59784)
    row(1, 1, 8192, 16 * 4 + 32768 + 59784);
    row(4, 1, 8192, 16 * 4 + 32768 + 59784);
    row(5, 1, 8192, 16 * 8 + 32768 + 59784);
    row(4388, 1, 8192, 70208 + 32768 + 59784);
    row(4389, 1, 4096, 70272 + 16384 + 59784);
    row(5412, 1, 4096, 86592 + 16384 + 59784);
    row(5413, 1, 2048, 86656 + 8192 + 59784);
    row(5924, 1, 2048, 94784 + 8192 + 59784);
    row(5925, 1, 1024, 94848 + 4096 + 59784);
    row(6180, 1, 1024, 98880 + 4096 + 59784);
    row(6181, 0, 0, 0);
    row(12002, 0, 0, 0);
    row(65535, 0, 0, 0);
    row(65536, 0, 0, 0);
    row(0x7fffffff, 0, 0, 0);
    row(0, 0, 0, 0);
    row(-7, 0, 0, 0);

    // every nt a call can bring up to well past the index limit: the plan is monotone (cells never grow, a fused plan never
    // follows a multi-launch one), a fused plan fits a compute unit's LDS beside the kernel's own 1024 bytes and holds its
    // cloud and cells, its cells are one of the four budgets, and nothing from 65536 targets on is fused
    IcpPlan prev = icp_plan(1);
    int budgets_seen = 0, last_cells = 0;
    for (int nt = 1; nt <= 70000; nt++) {
        const IcpPlan p = icp_plan(nt);
        if (p.one_workgroup) {
            if (!prev.one_workgroup) { printf("FAILED nt %d: fused after multi-launch\n", nt); g_failed++; }
            if (p.cells > prev.cells) { printf("FAILED nt %d: cells grow %d -> %d\n", nt, prev.cells, p.cells); g_failed++; }
            if (p.cells != 8192 && p.cells != 4096 && p.cells != 2048 && p.cells != 1024) { printf("FAILED nt %d: cells %d\n", nt, p.cells); g_failed++; }
            if ((long long)p.lds_bytes + 1024 > 160 * 1024) { printf("FAILED nt %d: %d bytes of LDS\n", nt, p.lds_bytes); g_failed++; }
            const long long need = (long long)((nt + 3) / 4 * 4) * 16 + (long long)p.cells * 4 + 59784;
            if (p.lds_bytes != need) { printf("FAILED nt %d: lds_bytes %d, layout needs %lld\n", nt, p.lds_bytes, need); g_failed++; }
            if (nt >= 65536) { printf("FAILED nt %d: fused past the 16-bit position\n", nt); g_failed++; }
            if (p.cells != last_cells) { budgets_seen++; last_cells = p.cells; }
        } else if (p.cells != 0 || p.lds_bytes != 0) {
            printf("FAILED nt %d: multi-launch plan with cells %d lds %d\n", nt, p.cells, p.lds_bytes);
            g_failed++;
        }
        prev = p;
    }
    expect("cell budgets met", 0, budgets_seen, 4);
    // ... and at the far end of int
    for (int nt = 0x7fffffff - 8; nt > 0 && nt <= 0x7fffffff; nt++) {
        if (icp_plan(nt).one_workgroup) { printf("FAILED nt %d: fused\n", nt); g_failed++; }
        if (nt == 0x7fffffff) break;
    }

    if (g_failed) {
        printf("icp_plan_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("icp_plan_check: ok\n");
    return 0;
}
