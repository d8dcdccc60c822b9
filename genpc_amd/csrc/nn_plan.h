// nn_plan.h -- the plan of one nearest-neighbour call (chamfer.hip nn_forward, behind genpc_chamfer_forward, genpc_nm_distance,
// the alignment loop, ICP and the scale search): the kernel family and its template instance, the slice length, the blocks of the
// launches and where each direction's begin, the size of the workspace.  nn_forward, launch_nn_f16 and launch_nn_finish read the
// plan and decide nothing besides; the measured numbers behind every threshold stand beside it here.
// Host code only, no HIP: a plain C++ program can include it (tests/nn_plan_check.cpp does); the library exports the function as
// genpc_nn_plan, and the GPU tests ask that call which shapes reach which kernel form on the device at hand.
#pragma once
#include <algorithm>

namespace genpc {

constexpr int kChunk = 32;             // targets per min-only chunk of the VALU path (re-scan granularity)
constexpr int kBlock = 256;            // 4 waves
constexpr int kMaxLists = 16;          // slices x lists per lane a finish block reads per query
constexpr int kHTile = 1024;           // f16 filter, targets per LDS tile: 2 planes x 16 B = 32 KiB (template parameter HT: 1024 or 2048)
constexpr int kFQ = 64;                // queries per finish block

// kernel families; the values are genpc_nn_tune's
enum NNFamily {
    kNNValu = 0,       // nn_forward_kernel (cross-check)
    kNNMfma32 = 1,     // nn_mfma_kernel: fp32 MFMA filter and its merge in one launch (small problems)
    kNNF16 = 3,        // nn_f16_kernel + nn_finish_kernel: two-piece f16 MFMA filter, exact finish (default)
    kNNGrid = 4,       // nn_grid.hip: cell-sorted pruned search, three launches, O(N + M) work (opt-in; the only one that stops at a radius)
};

// the forms of the f16 filter's 512-query blocks (Q = 4; Q = 2 has the first alone)
enum NNForm {
    kNNFourWave = 0,       // 4-wave blocks, two per CU, 1024-target LDS tile
    kNNThreeWave = 1,      // 4-wave blocks, three per CU (168 VGPRs, a little scratch): launches of three rounds and more
    kNNTile2048 = 2,       // 4-wave blocks, two per CU, 2048-target LDS tile (66 KiB per block): slices over 1024 targets
    kNNWide = 3,           // 8-wave blocks of 1024 queries, one per CU, 2048-target tile: single-round launches, slices over 1024
};

struct NNAsk {
    int b = 0;
    int ndir = 0;              // directions with work (add() skips the others)
    int nq[2] = {0, 0}, nt[2] = {0, 0};
    bool swapped = false;      // direction 1's queries are direction 0's targets and the converse (the cell search needs it)
    bool radius = false;       // a search limit was given
    int cus = 256;             // compute units of the device
    int forced = -1;           // genpc_nn_tune's family of the calling thread, -1: none
    // the switches, as given (a value that is not accepted counts as not given)
    int env_family = -1;       // GENPC_NN_PATH: a family, -1: not given
    int env_r = 0;             // GENPC_NN_R: VALU path, queries per lane, 2 | 4
    int env_q = 0;             // GENPC_NN_Q: MFMA filters, 32-query tiles per wave, 1 | 2 | 4
    int env_u = 0;             // GENPC_NN_U: target tiles per bookkeeping unit, 1 | 2 (fp32 MFMA), 2 | 4 (f16)
    int env_wps = 0;           // GENPC_NN_WPS: resident blocks per CU the planner assumes, > 0

    // A direction with no queries or no targets does nothing (the reference's loops do not execute, outputs keep the
    // caller's zeros): it is no part of the plan.
    bool add(int n, int m)
    {
        if (b <= 0 || n <= 0 || m <= 0 || ndir >= 2) return false;
        nq[ndir] = n;
        nt[ndir] = m;
        ndir++;
        return true;
    }
};

struct NNPlanDir {
    int qblocks;           // blocks that share a slice: ceil(nq / queries per block)
    int slices;            // ceil(nt / slice_len)
    int block_begin;       // first block of this direction in the (first) launch
    int unit_begin;        // its first arrival counter
    int fin_begin;         // its first finish block (f16)
    bool partials;         // it hands per-slice words to a merge or to the finish launch
};

struct NNPlan {
    NNFamily family;
    int r;                 // VALU: queries per lane, 2 | 4
    int q;                 // MFMA filters: 32-query tiles per wave -- fp32 1 | 2, f16 2 | 4
    int unit;              // target tiles per bookkeeping unit -- fp32 1 | 2, f16 2 | 4
    int nl;                // f16: candidate lists per lane, 1 | 2
    NNForm form;           // f16
    int slice_len;         // targets per slice: all blocks of the launch do equal work
    NNPlanDir dir[2];
    long long blocks;      // of the VALU / MFMA / filter launch
    long long units;       // arrival counters: one per (batch element, query block)
    int pwords;            // 8-byte words per (slice, query)
    long long part_words;  // partial words of all directions
    long long fin_blocks;  // f16: blocks of the finish launch
    int hint_stride;       // f16: every hint_stride-th finish block reports its re-dos
    bool early;            // f16: every finish block is resident at once (nn_finish_kernel's EARLY form)
    bool too_large;        // a launch would take more than 2^31 - 1 blocks: the call fails
};

inline long long nn_ceil(long long a, long long b) { return (a + b - 1) / b; }

inline NNPlan nn_plan(const NNAsk &a)
{
    NNPlan p{};
    const int nd = a.ndir, b = a.b, cus = a.cus;
    if (nd == 0) return p;
    int nt_max = 0;
    double pairs = 0.0;
    for (int d = 0; d < nd; d++) {
        nt_max = std::max(nt_max, a.nt[d]);
        pairs += (double)b * a.nq[d] * a.nt[d];
    }
    const bool env_path = a.env_family == kNNValu || a.env_family == kNNMfma32 || a.env_family == kNNF16 || a.env_family == kNNGrid;
    int family = a.forced >= 0 ? a.forced : (env_path ? a.env_family : kNNF16);
    // measured on MI355X (tools/nn_sweep.py): below ~6M pairs the single-launch fp32-MFMA
    // kernel wins (1x1024^2 11.0 vs 13.5 us), from 2048^2 on the two-launch f16 filter
    if (family == kNNF16 && pairs < 6e6 && a.forced < 0 && !env_path) family = kNNMfma32;
    if (a.radius) family = kNNGrid;      // only the cell search knows how to stop at a distance
    if (family == kNNGrid) {
        // needs both directions to be each other's swap
        if (nd == 1 || a.swapped) {
            p.family = kNNGrid;
            return p;
        }
        family = kNNF16;
    }
    if (family == kNNF16 && nt_max >= (1 << 25)) family = kNNMfma32;      // finish kernel packs tile indices in 21 bits
    p.family = (NNFamily)family;
    const bool f16 = family == kNNF16, valu = family == kNNValu;

    // queries per block, slice granularity (one bookkeeping unit), resident blocks per CU
    int qper, gran, per_cu = a.env_wps > 0 ? a.env_wps : 4;
    if (valu) {
        // R = 4 (fewer LDS reads per pair, more independent chains per lane) when the query
        // blocks alone fill the chip; R = 2 otherwise: twice the blocks, half the per-wave
        // epilogue (measured on MI355X: 1x16384^2 87 us vs 97 us, 13x16384^2 870 us vs 835 us).
        p.r = a.env_r == 2 || a.env_r == 4 ? a.env_r : 0;
        if (!p.r) {
            long long unsplit4 = 0;
            for (int d = 0; d < nd; d++) unsplit4 += (long long)b * nn_ceil(a.nq[d], kBlock * 4);
            p.r = unsplit4 >= cus ? 4 : 2;
        }
        qper = kBlock * p.r;
        gran = kChunk;
        p.pwords = 1;
    } else {
        // MFMA filters: a block covers 128 * Q queries.
        // fp32 MFMA: Q = 2 measured slower at every size from 1x2048^2 to 13x16384^2
        // f16 filter: 512-query blocks (Q = 4) once there is enough work to fill the chip with
        // them (1x16384^2 37.8 vs 49.7 us), 256-query blocks below (1x8192^2 20.4 vs 21.6 us)
        int q = a.env_q == 1 || a.env_q == 2 || a.env_q == 4 ? a.env_q : 0;
        if (!q) q = f16 ? (pairs >= 2e8 ? 4 : 2) : 1;
        // f16 filter: at least two accumulator chains per wave (see the hazard note in nn_f16.hip)
        if (f16 && q < 2) q = 2;
        if (f16 && a.env_wps <= 0) per_cu = q == 4 ? 2 : 3;      // (VGPRs)
        qper = 128 * q;
        gran = f16 ? 128 : 64;
        p.pwords = 3;
        // (GENPC_NN_Q=4 with the fp32 family sizes the blocks for 512 queries; the kernel has Q = 1 and 2 only)
        p.q = f16 || q == 2 ? q : 1;
    }
    const long long want_blocks = (long long)cus * per_cu;

    // One slice length for the whole launch, so that every block does the same amount
    // of work, and per-direction slice counts S_d = ceil(nt_d / slice_len) (no empty
    // slices when the two clouds differ in size).
    long long work = 0;          // blocks x targets if every block took one target
    for (int d = 0; d < nd; d++) {
        p.dir[d].qblocks = (int)nn_ceil(a.nq[d], qper);
        work += (long long)b * p.dir[d].qblocks * a.nt[d];
    }
    auto blocks_at = [&](long long len) {
        long long t = 0;
        for (int d = 0; d < nd; d++) t += (long long)b * p.dir[d].qblocks * nn_ceil(a.nt[d], len);
        return t;
    };
    long long len;
    if (!f16) {
        // slice_len is what makes the launch ~want_blocks blocks: sum_d b * qblocks_d * nt_d / want_blocks, but never below 8
        // chunks, and not below 16 chunks (512 targets: below that the per-block staging /
        // merge latency outweighs the parallelism; measured 1x8192^2 44 us vs 51 us) as long
        // as two blocks per CU remain.
        len = nn_ceil(nn_ceil(work, want_blocks), gran) * gran;
        if (len < kChunk * 8) len = kChunk * 8;
        if (len < kChunk * 16 && blocks_at(kChunk * 16) >= 2 * cus) len = kChunk * 16;
        if (len > nt_max) len = nn_ceil(nt_max, gran) * gran;
        // bookkeeping per 64 targets once a block has enough of them to amortise the coarser
        // re-scan (measured: 1x2048^2 14.5 vs 16.0 us, 1x16384^2 63.6 vs 61.2, 13x16384^2 644 vs 590)
        if (!valu) p.unit = a.env_u == 1 || a.env_u == 2 ? a.env_u : (len >= 2048 ? 2 : 1);
    } else {
        // The launch runs in rounds of resident blocks, so the slice count is chosen to minimise
        // rounds x (targets per block + a fixed per-block cost worth ~192 targets), over the slice counts that keep a query's
        // candidate lists (slices x NL; NL = 2 lists per lane below three slices: a query is flagged only when THREE
        // candidate units fall into one list) within kMaxLists.
        auto lists_of = [&](long long l, int &nl_out) {
            long long smin = 1 << 30, smax = 0;
            for (int d = 0; d < nd; d++) {
                const long long sd = nn_ceil(a.nt[d], l);
                smin = std::min(smin, sd);
                smax = std::max(smax, sd);
            }
            nl_out = smin >= 3 ? 1 : 2;
            return smax * nl_out;
        };
        // The 512-query blocks (Q = 4) exist in two register budgets: 2 resident
        // blocks per CU, or 3 (168 VGPRs, a little scratch: ~4 % faster per pair over many rounds,
        // ~1 us slower when the launch is a single round).  All resident blocks share the VALU, so
        // a round costs (resident blocks) x (targets per block + fixed part).
        const bool budgets = p.q == 4 && a.env_wps <= 0;
        long long best_len = 0;
        double best_cost = 0.0;
        int best_res = 0;
        for (int res = budgets ? 3 : 0; res >= 0; res = res == 3 ? 2 : -1) {
            const long long slots = res ? (long long)cus * res : want_blocks;
            const double per_block = res == 3 ? 3.0 * 0.96 : (res == 2 ? 2.0 : 1.0);
            for (int sc = 1; sc <= 16; sc++) {
                const long long l = nn_ceil(nn_ceil(nt_max, sc), gran) * gran;
                if (sc > 1 && l < 256) break;
                int nl_c;
                if (lists_of(l, nl_c) > kMaxLists) continue;
                const long long rounds = nn_ceil(blocks_at(l), slots);
                if (res == 3 && rounds < 3) continue;         // few rounds: the leaner kernel wins
                const double cost = (double)rounds * (double)(std::min<long long>(l, nt_max) + 192) * per_block;
                if (!best_len || cost < best_cost * 0.98) {      // prefer fewer slices unless clearly better
                    best_len = l;
                    best_cost = cost;
                    best_res = res;
                }
            }
        }
        len = best_len;
        (void)lists_of(len, p.nl);
        p.pwords = 2 * p.nl;        // (a1, c1) (codes of a2 | a3, c2) per list: list_enc in nn.h
        p.form = kNNFourWave;
        if (p.q == 4) {
            if (best_res == 3) {
                p.form = kNNThreeWave;
            } else if (len > kHTile) {
                // HT = 2048 (a slice of up to 2048 targets is resident) where two waves per SIMD are all the
                // registers allow anyway (4 x 16384 x 8192, slices of 4096: 57.9 -> 54.7 us)
                p.form = kNNTile2048;
                // Single-round launches: blocks of 8 waves / 1024 queries,
                // one per CU -- the same two waves per SIMD, but a slice is read, split into f16 pieces and staged once per
                // 1024 queries instead of once per 512 (the prologue was a third of a block's time: tools/nn_timeline.py).
                if (blocks_at(len) <= 2 * (long long)cus) {
                    p.form = kNNWide;
                    for (int d = 0; d < nd; d++) p.dir[d].qblocks = (int)nn_ceil(a.nq[d], 2 * qper);
                }
            }
        }
        // bookkeeping unit: the finish kernel re-reads 16 targets per tile of every candidate unit --
        // per QUERY, while the filter's work is per PAIR: short target clouds (many queries per
        // pair) take 64-target units (half the re-read, +10 % filter VALU), long ones 128
        p.unit = a.env_u == 2 || a.env_u == 4 ? a.env_u : (nt_max <= 8192 ? 2 : 4);
    }
    p.slice_len = (int)len;

    for (int d = 0; d < nd; d++) {
        NNPlanDir &D = p.dir[d];
        D.slices = (int)nn_ceil(a.nt[d], p.slice_len);
        D.block_begin = (int)p.blocks;
        D.unit_begin = (int)p.units;
        D.fin_begin = (int)p.fin_blocks;
        p.blocks += (long long)D.slices * b * D.qblocks;
        p.units += (long long)b * D.qblocks;
        D.partials = D.slices > 1 || f16;      // the filter always hands its lists to a second launch
        if (D.partials) p.part_words += (long long)D.slices * b * a.nq[d] * p.pwords;
        if (f16) p.fin_blocks += (long long)b * nn_ceil(a.nq[d], kFQ);
    }
    p.too_large = p.blocks > 0x7fffffffLL || p.fin_blocks > 0x7fffffffLL;
    if (f16) {
        // re-dos are reported sampled: at most 16 atomics on host memory per launch (nn_finish_kernel)
        p.hint_stride = (int)nn_ceil(p.fin_blocks, 16);
        p.early = p.fin_blocks <= 2 * (long long)cus;
    }
    return p;
}

}  // namespace genpc
