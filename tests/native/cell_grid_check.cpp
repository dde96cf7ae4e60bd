// Host check of the integer part of csrc/cell_grid.h: the order-preserving integers of doubles and the 3 x 21-bit cell
// keys.  Built and run by tests/test_abi.py::test_cell_grid_integers (g++, no GPU).
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "cell_grid.h"

static uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

int main() {
    long bad = 0, checks = 0;
    // a sorted list: ord_of is strictly monotone over it (-0.0 below +0.0) and ord_back gives the same bits back
    const double den = 4.9406564584124654e-324;   // the smallest denormal
    const std::vector<double> sorted = { -DBL_MAX, -1e300, -2.5, -1.0, -DBL_MIN, -DBL_MIN / 2, -2 * den, -den, -0.0, 0.0, den, 2 * den,
                                         DBL_MIN / 2, DBL_MIN, 0.1, 1.0, 1.0 + DBL_EPSILON, 1048576.0, 1e300, DBL_MAX };
    for (size_t i = 0; i < sorted.size(); i++) {
        checks++;
        if (bits(ord_back(ord_of(sorted[i]))) != bits(sorted[i])) { bad++; printf("round trip of %a\n", sorted[i]); }
        if (i > 0) {
            checks++;
            if (!(ord_of(sorted[i - 1]) < ord_of(sorted[i]))) { bad++; printf("order of %a and %a\n", sorted[i - 1], sorted[i]); }
        }
    }
    // pack and extract round-trip at the ends of the cell range, with either bias
    const long long ends[3] = { 0, 1, (1LL << 20) - 1 };
    for (int bias = 0; bias <= 1; bias++)
        for (long long cx : ends) for (long long cy : ends) for (long long cz : ends) {
            const uint64_t k = grid_pack(cx, cy, cz, bias);
            const long long c[3] = { cx, cy, cz };
            for (int a = 0; a < 3; a++) {
                checks++;
                if ((long long)grid_field(k, a) - bias != c[a]) { bad++; printf("field %d of (%lld %lld %lld) bias %d\n", a, cx, cy, cz, bias); }
            }
            checks++;
            if (k >> 63) { bad++; printf("bit 63 set\n"); }
        }
    // bias 1: the 13 forward neighbours of the component filter's union pass, added to the key as one integer, change
    // the intended fields only -- at the low and at the high end of the cell range
    for (long long e : { 0LL, (1LL << 20) - 1 })
        for (int dx = 0; dx <= 1; dx++) for (int dy = -1; dy <= 1; dy++) for (int dz = -1; dz <= 1; dz++) {
            if (!(dx > 0 || dy > 0 || (dy == 0 && dz > 0))) continue;
            const uint64_t k = grid_pack(e, e, e, 1) + (uint64_t)(((long long)dx << 42) + ((long long)dy << 21) + dz);
            const long long d[3] = { dx, dy, dz };
            for (int a = 0; a < 3; a++) {
                checks++;
                if ((long long)grid_field(k, a) != e + 1 + d[a]) { bad++; printf("neighbour (%d %d %d) of cell %lld, field %d\n", dx, dy, dz, e, a); }
            }
            checks++;
            if (k >> 63) { bad++; printf("bit 63 set\n"); }
        }
    // the extent check: 2^20 cells fit (cells 0 .. 2^20 - 1), one more does not
    double cells;
    checks += 2;
    if (!grid_axis_fits(0.0, 1048575.5, 1.0, &cells) || cells != 1048575.0) { bad++; printf("2^20 cells\n"); }
    if (grid_axis_fits(0.0, 1048576.0, 1.0, &cells)) { bad++; printf("2^20 + 1 cells\n"); }
    printf("%ld checks, %ld bad\n", checks, bad);
    return bad != 0;
}
