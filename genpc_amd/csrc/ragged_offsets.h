// ragged_offsets.h -- what every ragged call does with a host offset table (c + 1 ints: entry j owns [off[j], off[j + 1])),
// stated once: the check, the copy into a by-value kernel-argument array, and the search that finds an owner.
//   * ragged_offsets_fault: a table must start at 0 and ascend; entries may be empty.
//   * ragged_pad_copy: the kernel-argument array has a fixed bound; the entries beyond c repeat off[c], so every entry reads
//     as an empty one and off[j + 1] is defined for every j a kernel can form.
//   * ragged_search: the largest j in [0, c) with key(j) <= x, for a key that does not descend and has key(0) <= x.  Its two
//     named forms: ragged_owner (key = off[j]: the owner of a packed position, empty entries passed over whether they lie
//     before, between or behind the others) and ragged_item_owner (key = (off[j] >> shift) + j: the owner of a work item in the
//     numbering that ragged_items.h proves).  Every index they form is uniform where x is: scalar loads of the argument segment.
// Host and device, no HIP include: a plain C++ program can include it (tests/ragged_offsets_check.cpp does, under the sanitizers).
#pragma once
#include <initializer_list>

#if defined(__HIPCC__)
#define GENPC_RAGGED_HD __host__ __device__
#else
#define GENPC_RAGGED_HD
#endif

namespace genpc {

// Tables checked together: null when each starts at 0 and ascends, else what is wrong -- where they start comes before how
// they ascend, whichever table it is.  (A call that checks its tables one after the other asks once per table.)
inline const char *ragged_offsets_fault(int c, std::initializer_list<const int *> tables)
{
    for (const int *off : tables)
        if (off[0] != 0) return "offsets must start at 0";
    for (int j = 0; j < c; j++)
        for (const int *off : tables)
            if (off[j + 1] < off[j]) return "offsets must ascend";
    return nullptr;
}
inline const char *ragged_offsets_fault(int c, const int *off) { return ragged_offsets_fault(c, {off}); }

// dst[j] = src[j] up to c, src[c] from there to the array's last entry
template <int N>
inline void ragged_pad_copy(int (&dst)[N], const int *src, int c)
{
    for (int j = 0; j < N; j++) dst[j] = src[j < c ? j : c];
}

// the largest j in [0, c) with key(j) <= x
template <typename Key>
GENPC_RAGGED_HD inline int ragged_search(int c, int x, Key key)
{
    int lo = 0, hi = c - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key(mid) <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the owner of packed position (or candidate, or workgroup) x, 0 <= x < off[c]: the largest j with off[j] <= x
GENPC_RAGGED_HD inline int ragged_owner(const int *off, int c, int x)
{
    return ragged_search(c, x, [off](int j) { return off[j]; });
}

// the owner of work item `item` of 2^shift elements, 0 <= item < (off[c] >> shift) + c: the largest j with (off[j] >> shift) + j <= item
GENPC_RAGGED_HD inline int ragged_item_owner(const int *off, int c, int item, int shift)
{
    return ragged_search(c, item, [off, shift](int j) { return (off[j] >> shift) + j; });
}

}  // namespace genpc
