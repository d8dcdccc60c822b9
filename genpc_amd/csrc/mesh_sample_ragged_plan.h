// mesh_sample_ragged_plan.h -- how one genpc_mesh_sample_ragged call deals c meshes to its workgroups and its scratch.
//
// The table -- three offset arrays and the seeds -- travels BY VALUE in the kernel arguments, as ragged_table.h's does: no copy
// is enqueued, nothing of the caller's host arrays is read after the entry point returns, and 4 KiB of arguments bound a call
// at kMsRaggedMaxMeshes meshes.  Every index a kernel forms into it is uniform over the workgroup.
// Work items are numbered as ragged_items.h numbers them, here over any ascending offset array: mesh j's first item of 2^shift
// elements is (off[j] >> shift) + j.  With a = off[j], b = off[j + 1], K = 2^shift the mesh needs
//     ceil((b - a) / K)  <=  floor(b / K) - floor(a / K) + 1
// items (ragged_items.h has the proof) and the right-hand side is the distance to mesh j + 1's first item.  So the ranges do
// not overlap, the numbering ascends strictly, a binary search finds the mesh of an item, an item never leaves its mesh, and
// at most one item per mesh -- the last of its range -- is idle.  Two numberings are used:
//   * faces, shift 10: item = a chunk of 1024 faces of the mesh's OWN numbering.  The chunk's sum lies in slot `item` of the
//     chunk sums: mesh j's sums are the consecutive slots from ms_ragged_first_item(foff, j, 10), disjoint from every other mesh's.
//   * samples, shift 8: item = the 256 samples a workgroup of the sampling launch draws, all of one mesh.
// Host code only, no HIP: tests/mesh_sample_ragged_plan_check.cpp includes it under the sanitizers.
#pragma once
#include "ragged_offsets.h"
#include "ws_layout.h"

namespace genpc {

constexpr int kMsRaggedMaxMeshes = 128;           // 3 x 129 ints + 128 seeds = 2576 bytes of the 4096 a kernel may take
constexpr int kMsRaggedMaxFaces = 1 << 24;        // per mesh: genpc_mesh_sample's own bound (16384 chunk sums, one scan workgroup)
constexpr int kMsRaggedMaxTotal = 1 << 28;        // vertices, faces, samples of all meshes together: 3 x either and the items stay ints
constexpr int kMsRaggedChunkShift = 10;           // = log2 kMsChunk (mesh_sample_ragged.hip asserts it)
constexpr int kMsRaggedSampleShift = 8;           // = log2 kMsBlock

struct MsRaggedTable {
    int c;
    int voff[kMsRaggedMaxMeshes + 1];             // vertices of mesh j: [voff[j], voff[j + 1])
    int foff[kMsRaggedMaxMeshes + 1];             // faces
    int soff[kMsRaggedMaxMeshes + 1];             // samples
    unsigned long long seed[kMsRaggedMaxMeshes];
};
static_assert(sizeof(MsRaggedTable) <= 3584, "the table and a dozen pointers must fit the kernel arguments");

struct MsRaggedHeader {                           // = mesh_sample.h's MsHeader (mesh_sample_ragged.hip asserts the size)
    unsigned long long amax_bits;
    int bad, pad;
};

// the number of the first work item of mesh j   (0 <= j <= c; j == c: the number of items of the launch)
GENPC_RAGGED_HD inline int ms_ragged_first_item(const int *off, int j, int shift) { return (off[j] >> shift) + j; }

// the mesh a work item serves: the largest j with (off[j] >> shift) + j <= item   (0 <= item < ms_ragged_first_item(off, c, shift))
GENPC_RAGGED_HD inline int ms_ragged_mesh_of(const int *off, int c, int item, int shift) { return ragged_item_owner(off, c, item, shift); }

// the first element of a work item, counted inside its mesh; at or beyond the mesh's size: the item is idle
GENPC_RAGGED_HD inline int ms_ragged_item_base(const int *off, int mesh, int item, int shift)
{
    return (item - ms_ragged_first_item(off, mesh, shift)) << shift;
}

// Checks the caller's tables and copies them.  1: there is work; 0: no mesh; -1 with *err set: refused.
inline int ms_ragged_fill(int c, const int *voff, const int *foff, const int *soff, const unsigned long long *seeds, MsRaggedTable &t,
                          const char **err)
{
    *err = nullptr;
    if (c < 0) { *err = "negative number of meshes"; return -1; }
    if (c == 0) return 0;
    if (c > kMsRaggedMaxMeshes) { *err = "more than 128 meshes in one call"; return -1; }
    static_assert(kMsRaggedMaxMeshes == 128, "the message above names the bound");
    if (!voff || !foff || !soff || !seeds) { *err = "null offset or seed table"; return -1; }
    if ((*err = ragged_offsets_fault(c, {voff, foff, soff}))) return -1;
    if (voff[c] > kMsRaggedMaxTotal || foff[c] > kMsRaggedMaxTotal || soff[c] > kMsRaggedMaxTotal) {
        *err = "more than 2^28 vertices, faces or samples in one call";
        return -1;
    }
    for (int j = 0; j < c; j++) {
        const int nf = foff[j + 1] - foff[j];
        if (nf < 1 || nf > kMsRaggedMaxFaces) { *err = "every mesh needs 1 <= nf <= 2^24 faces"; return -1; }
        if (voff[j + 1] == voff[j]) { *err = "every mesh needs nv >= 1 vertices"; return -1; }
    }
    t.c = c;
    ragged_pad_copy(t.voff, voff, c);
    ragged_pad_copy(t.foff, foff, c);
    ragged_pad_copy(t.soff, soff, c);
    for (int j = 0; j < kMsRaggedMaxMeshes; j++) t.seed[j] = j < c ? seeds[j] : 0;
    return 1;
}

// The scratch of a call: per-mesh headers | per-face local cumulative weights (the areas before), restarted every 1024 faces
// of the mesh's own numbering | one sum per chunk item.  16 bytes a mesh, 8 bytes a face, 8 bytes per 1024 faces and mesh.
struct MsRaggedScratch {
    MsRaggedHeader *hdr;
    unsigned long long *cum, *chunk_sum;
};
inline void ms_ragged_layout(const MsRaggedTable &t, WsLayout &L, MsRaggedScratch &s)
{
    L.add(s.hdr, (size_t)t.c);
    L.add(s.cum, (size_t)t.foff[t.c]);
    L.add(s.chunk_sum, (size_t)ms_ragged_first_item(t.foff, t.c, kMsRaggedChunkShift));
}

}  // namespace genpc
