// ptv_xcd_map.hpp — dispatch slot -> block of the tile grid, for launches with no block order.
#pragma once

#if defined(__HIPCC__)
#define PTV_XCD_HD __host__ __device__
#else
#define PTV_XCD_HD  // a plain C++ translation unit (the host test of the map)
#endif

namespace ptv {

constexpr int kXcds = 8;  // the dispatcher deals workgroups round-robin over the 8 XCDs

// Bijection of [0, nb).  Dispatch slot lb runs on XCD lb % 8 as that XCD's slot lb / 8.  The blocks
// of the linear order are cut into chunks of `chunk` consecutive blocks, dealt round-robin: XCD x
// takes chunks x, x + 8, x + 16, ..., and consecutive slots of an XCD take consecutive blocks of a
// chunk, so that every XCD samples the whole grid and neighbouring tiles still share its L2.  Only
// whole rounds of 8 chunks are dealt; the rest (fewer than 8 * chunk blocks) is cut into 8 contiguous
// ranges, one per XCD, the first nb % 8 of them one block longer, which is also the whole map when
// chunk <= 0 or nb < 16 * chunk (fewer than two rounds).
PTV_XCD_HD inline int xcd_chunk_block(int lb, int nb, int chunk) {
    const int x = lb & (kXcds - 1);
    int i = lb >> 3;
    int rounds = chunk > 0 ? (nb / chunk) >> 3 : 0;
    if (rounds < 2) rounds = 0;
    const int dealt = rounds * chunk;  // slots of each XCD that the whole rounds fill
    if (i < dealt) {
        const int m = i / chunk;
        return (m * kXcds + x) * chunk + (i - m * chunk);
    }
    i -= dealt;
    const int base = dealt * kXcds;
    const int rem = nb - base;
    const int q = rem >> 3, r = rem & 7;
    return base + ((x < r) ? x * (q + 1) + i : r * (q + 1) + (x - r) * q + i);
}

}  // namespace ptv
