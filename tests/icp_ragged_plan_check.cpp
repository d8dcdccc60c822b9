// Stand-alone check of genpc_amd/csrc/icp_ragged_plan.h (host code only; tests/test_icp_ragged_plan.py builds it with
// -fsanitize=address,undefined and runs it).  Exit status 0 = every check passed; each failure prints what it found.
// The target counts come from icp_plan itself: for each cell budget the LARGEST nt that gets it, the FIRST multi-launch nt, and 1;
// what is expected of the split is counted here pair by pair, with no second copy of the header's loop.
#include "icp_ragged_plan.h"

#include <stdio.h>
#include <vector>

using namespace genpc;

static int g_failed = 0;

static void expect(const char *what, const char *which, long long got, long long want)
{
    if (got != want) { printf("FAILED %s: %s = %lld, expected %lld\n", what, which, got, want); g_failed++; }
}

static void check(const char *what, const std::vector<int> &nts, int fused, int loop, int lds)
{
    std::vector<int> toff(nts.size() + 1, 0);          // exactly c + 1 entries: the sanitizer sees a read past them
    for (size_t j = 0; j < nts.size(); j++) toff[j + 1] = toff[j] + nts[j];
    const IcpRaggedPlan p = icp_ragged_plan((int)nts.size(), toff.data());
    expect(what, "fused_pairs", p.fused_pairs, fused);
    expect(what, "loop_pairs", p.loop_pairs, loop);
    expect(what, "lds_bytes", p.lds_bytes, lds);
}

int main()
{
    // the sizes, from icp_plan: each budget's last nt, the first multi-launch nt
    std::vector<int> last;                              // largest nt of each cell budget, largest budget first
    int first_loop = 0;
    {
        IcpPlan prev = icp_plan(1);
        if (!prev.one_workgroup) { printf("FAILED: nt 1 is not fused\n"); return 1; }
        for (int nt = 2; nt <= 70000 && !first_loop; nt++) {
            const IcpPlan p = icp_plan(nt);
            if (!p.one_workgroup) { last.push_back(nt - 1); first_loop = nt; }
            else if (p.cells != prev.cells) last.push_back(nt - 1);
            prev = p;
        }
    }
    expect("sizes", "cell budgets", (long long)last.size(), 4);
    if (!first_loop || last.empty()) { printf("FAILED: no multi-launch nt up to 70000\n"); return 1; }
    for (size_t i = 0; i < last.size(); i++) {
        if (!icp_plan(last[i]).one_workgroup) { printf("FAILED: nt %d is not fused\n", last[i]); g_failed++; }
        if (i + 1 < last.size() && icp_plan(last[i] + 1).cells >= icp_plan(last[i]).cells) { printf("FAILED: nt %d is no boundary\n", last[i]); g_failed++; }
    }
    expect("sizes", "first multi-launch follows the last budget", first_loop, last.back() + 1);

    // c = 0: zero everywhere, and the table is not looked at
    check("no pair", {}, 0, 0, 0);
    {
        const IcpRaggedPlan p = icp_ragged_plan(0, nullptr);
        expect("no pair, null table", "sum", p.fused_pairs + p.loop_pairs + p.lds_bytes, 0);
    }
    // one pair of each size: the launch's LDS is that pair's plan
    check("nt 1", {1}, 1, 0, icp_plan(1).lds_bytes);
    for (int nt : last) check("one fused pair", {nt}, 1, 0, icp_plan(nt).lds_bytes);
    check("one loop pair", {first_loop}, 0, 1, 0);
    // an all-fused call: the maximum is the largest plan among them wherever it stands (lds is not monotone in nt: it drops
    // where the cell budget halves, so the largest cloud need not ask the most)
    {
        std::vector<int> nts = {1};
        int want = icp_plan(1).lds_bytes, arg = 1;
        for (int nt : last) {
            nts.push_back(nt);
            if (icp_plan(nt).lds_bytes > want) { want = icp_plan(nt).lds_bytes; arg = nt; }
        }
        check("all fused", nts, (int)nts.size(), 0, want);
        std::vector<int> rev(nts.rbegin(), nts.rend());
        check("all fused, reversed", rev, (int)rev.size(), 0, want);
        if ((long long)want + (long long)kFLdsStatic > (long long)kFLdsBudget) { printf("FAILED: %d bytes of LDS (nt %d)\n", want, arg); g_failed++; }
        // the same with loop pairs and empty targets among them: only the counts move
        std::vector<int> mixed = nts;
        mixed.insert(mixed.begin() + 2, first_loop);
        mixed.push_back(0);
        mixed.push_back(first_loop + 5821);
        mixed.insert(mixed.begin(), 0);
        check("mixed", mixed, (int)nts.size(), 2, want);
    }
    // an all-loop call: zero on the other side
    check("all loop", {first_loop, first_loop + 5821, 65536, first_loop}, 0, 4, 0);
    // only empty targets: on neither side
    check("all empty", {0, 0, 0}, 0, 0, 0);
    // the most pairs a call may bring
    {
        std::vector<int> nts(kIcpRaggedMaxPairs, 1);
        nts[kIcpRaggedMaxPairs - 1] = first_loop;
        nts[7] = last[0];
        check("256 pairs", nts, kIcpRaggedMaxPairs - 1, 1, icp_plan(last[0]).lds_bytes > icp_plan(1).lds_bytes ? icp_plan(last[0]).lds_bytes : icp_plan(1).lds_bytes);
    }
    // three offset tables of kIcpRaggedMaxPairs + 1 ints and what else the launch takes fit the 4 KiB of kernel arguments
    if ((size_t)3 * (kIcpRaggedMaxPairs + 1) * sizeof(int) + 128 > 4096) { printf("FAILED: the tables do not fit the kernel arguments\n"); g_failed++; }

    if (g_failed) {
        printf("icp_ragged_plan_check: %d check(s) failed\n", g_failed);
        return 1;
    }
    printf("icp_ragged_plan_check: ok\n");
    return 0;
}
