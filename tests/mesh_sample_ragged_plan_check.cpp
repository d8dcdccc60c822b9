// mesh_sample_ragged_plan_check.cpp -- csrc/mesh_sample_ragged_plan.h as a stand-alone program (built with the address and
// undefined-behaviour sanitizers by tests/test_mesh_sample_ragged_host.py).  For random offset tables:
//   * every face belongs to exactly one chunk item of its own mesh, every sample to exactly one sample item of its own mesh;
//   * the chunk-sum slots of different meshes do not overlap, and a mesh's slots are its ceil(nf / 1024) first ones;
//   * the scratch size covers the headers, the per-face weights and every slot, the pieces 256-byte aligned and disjoint;
//   * ms_ragged_fill's refusals and its padding of the unused table entries.
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "mesh_sample_ragged_plan.h"

using namespace genpc;

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 32);
}

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
            exit(1);                                                            \
        }                                                                       \
    } while (0)

// every element of [off[j], off[j + 1]) is covered once by an item of mesh j; items ascend; at most one idle item per mesh
static void check_items(const int *off, int c, int shift)
{
    const int items = ms_ragged_first_item(off, c, shift);
    std::vector<int> seen((size_t)off[c], 0);
    std::vector<int> idle((size_t)c, 0), owned((size_t)c, 0);
    for (int item = 0; item < items; item++) {
        const int j = ms_ragged_mesh_of(off, c, item, shift);
        CHECK(j >= 0 && j < c);
        CHECK(ms_ragged_first_item(off, j, shift) <= item && item < ms_ragged_first_item(off, j + 1, shift));
        const int n = off[j + 1] - off[j];
        const int base = ms_ragged_item_base(off, j, item, shift);
        CHECK(base >= 0);
        owned[j]++;
        if (base >= n) { idle[j]++; continue; }
        const int end = base + (1 << shift) < n ? base + (1 << shift) : n;
        for (int i = base; i < end; i++) seen[(size_t)off[j] + i]++;
    }
    for (int i = 0; i < off[c]; i++) CHECK(seen[i] == 1);
    for (int j = 0; j < c; j++) {
        CHECK(idle[j] <= 1 && owned[j] >= 1);
        CHECK(owned[j] - idle[j] == ((off[j + 1] - off[j]) + (1 << shift) - 1) >> shift);
    }
}

static void check_table(int c, const std::vector<int> &voff, const std::vector<int> &foff, const std::vector<int> &soff)
{
    std::vector<unsigned long long> seeds((size_t)c);
    for (int j = 0; j < c; j++) seeds[j] = ((unsigned long long)rnd() << 32) | rnd();
    MsRaggedTable t;
    const char *err = nullptr;
    CHECK(ms_ragged_fill(c, voff.data(), foff.data(), soff.data(), seeds.data(), t, &err) == 1 && !err);
    CHECK(t.c == c);
    for (int j = 0; j <= kMsRaggedMaxMeshes; j++) {
        const int k = j < c ? j : c;
        CHECK(t.voff[j] == voff[k] && t.foff[j] == foff[k] && t.soff[j] == soff[k]);
    }
    for (int j = 0; j < kMsRaggedMaxMeshes; j++) CHECK(t.seed[j] == (j < c ? seeds[j] : 0));
    check_items(t.foff, c, kMsRaggedChunkShift);
    check_items(t.soff, c, kMsRaggedSampleShift);
    // the chunk-sum slots: mesh j's are [first(j), first(j) + chunks_j), inside [first(j), first(j + 1))
    const int slots = ms_ragged_first_item(t.foff, c, kMsRaggedChunkShift);
    std::vector<int> owner((size_t)slots, -1);
    for (int j = 0; j < c; j++) {
        const int nf = t.foff[j + 1] - t.foff[j], chunks = (nf + 1023) / 1024;
        const int first = ms_ragged_first_item(t.foff, j, kMsRaggedChunkShift);
        for (int k = 0; k < chunks; k++) {
            CHECK(first + k < slots && owner[first + k] == -1);
            owner[first + k] = j;
        }
    }
    // the scratch
    WsLayout L;
    MsRaggedScratch s;
    ms_ragged_layout(t, L, s);
    CHECK(L.ok());
    std::vector<char> block(L.bytes() + 256);
    char *base = block.data() + (256 - (size_t)block.data() % 256) % 256;
    L.bind(base);
    char *hdr = (char *)s.hdr, *cum = (char *)s.cum, *sum = (char *)s.chunk_sum, *end = base + L.bytes();
    CHECK(hdr == base && (size_t)(cum - base) % 256 == 0 && (size_t)(sum - base) % 256 == 0);
    CHECK(hdr + (size_t)c * sizeof(MsRaggedHeader) <= cum);
    CHECK(cum + (size_t)t.foff[c] * 8 <= sum);
    CHECK(sum + (size_t)slots * 8 <= end);
    // (touch every word the kernels may touch: the sanitizer watches the block)
    for (int j = 0; j < c; j++) s.hdr[j].amax_bits = 0, s.hdr[j].bad = 0;
    for (int f = 0; f < t.foff[c]; f++) s.cum[f] = 1;
    for (int k = 0; k < slots; k++) s.chunk_sum[k] = 2;
}

static void refusals()
{
    MsRaggedTable t;
    const char *err = nullptr;
    const int z2[2] = {0, 5}, up[3] = {0, 5, 9}, down[3] = {0, 9, 5}, one[3] = {1, 5, 9}, flat[3] = {0, 5, 5};
    const unsigned long long sd[3] = {1, 2, 3};
    CHECK(ms_ragged_fill(-1, up, up, up, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(0, nullptr, nullptr, nullptr, nullptr, t, &err) == 0 && !err);
    CHECK(ms_ragged_fill(kMsRaggedMaxMeshes + 1, up, up, up, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, nullptr, up, up, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, up, nullptr, up, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, up, up, nullptr, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, up, up, up, nullptr, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, one, up, up, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, up, one, up, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, up, up, one, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, down, up, up, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, up, down, up, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, up, up, down, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(2, flat, up, up, sd, t, &err) == -1 && err);          // nv_1 = 0
    CHECK(ms_ragged_fill(2, up, flat, up, sd, t, &err) == -1 && err);          // nf_1 = 0
    CHECK(ms_ragged_fill(2, up, up, flat, sd, t, &err) == 1 && !err);          // count_1 = 0 is allowed
    const int big[2] = {0, (1 << 24) + 1}, most[2] = {0, 1 << 24};
    CHECK(ms_ragged_fill(1, z2, big, z2, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(1, z2, most, z2, sd, t, &err) == 1 && !err);
    const int over[2] = {0, (1 << 28) + 1};
    CHECK(ms_ragged_fill(1, over, z2, z2, sd, t, &err) == -1 && err);
    CHECK(ms_ragged_fill(1, z2, z2, over, sd, t, &err) == -1 && err);
}

int main()
{
    refusals();
    const int face_sizes[] = {1, 2, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 5000, 70000};
    const int sample_sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 4097};
    for (int round = 0; round < 400; round++) {
        const int c = round < 4 ? (round == 0 ? 1 : round == 1 ? kMsRaggedMaxMeshes : 1 + (int)(rnd() % 3)) : 1 + (int)(rnd() % kMsRaggedMaxMeshes);
        std::vector<int> voff(1, 0), foff(1, 0), soff(1, 0);
        for (int j = 0; j < c; j++) {
            const unsigned pick = rnd() % 4;
            const int nf = pick == 0 ? face_sizes[rnd() % 13] : pick == 1 ? 1 + (int)(rnd() % 3000) : 1024 * (1 + (int)(rnd() % 4)) + (int)(rnd() % 3) - 1;
            const int ns = rnd() % 2 ? sample_sizes[rnd() % 11] : (int)(rnd() % 1500);
            voff.push_back(voff.back() + 1 + (int)(rnd() % 2000));
            foff.push_back(foff.back() + nf);
            soff.push_back(soff.back() + ns);
        }
        check_table(c, voff, foff, soff);
    }
    printf("mesh_sample_ragged_plan_check: ok\n");
    return 0;
}
