// Host check of the candidate records of csrc/rh_internal.h: the float record a Float32 cloud's kernels derive from the
// binary64 one -- prepf_of_kind(prep_one(s)) -- against the record written out here from the shape alone (the field casts,
// a plane's normal normalised in binary32, the sign slot, zeros elsewhere), byte for byte; and rh_prep_host against
// prep_one.  Built and run by tests/test_abi.py::test_prep_records (host compile only, no GPU).
#include <cmath>
#include <cstdio>
#include <cstring>
#include "rh_internal.h"

// the expected float record, from the shape's own numbers
static void expect_record(const rh_shape &s, float e[12])
{
    for (int i = 0; i < 12; i++) e[i] = 0.0f;
    const float sgn = s.outwards ? 1.0f : -1.0f;
    if (s.kind == RH_PLANE) {
        for (int i = 0; i < 6; i++) e[i] = (float)s.v[i];
        const float inv = 1.0f / sqrtf((e[3] * e[3] + e[4] * e[4]) + e[5] * e[5]);
        e[6] = inv * e[3]; e[7] = inv * e[4]; e[8] = inv * e[5];
    } else if (s.kind == RH_SPHERE) {
        for (int i = 0; i < 4; i++) e[i] = (float)s.v[i];
        e[4] = sgn;
    } else if (s.kind == RH_CYLINDER) {
        for (int i = 0; i < 7; i++) e[i] = (float)s.v[i];
        e[7] = sgn;
    } else {
        for (int i = 0; i < 6; i++) e[i] = (float)s.v[i];
        e[6] = (float)s.v[7]; e[7] = (float)s.v[8];
        e[8] = sgn;
    }
}

int main()
{
    // per case the nine numbers a shape can hold: binary32-representable, rounding (0.1, 1/3, ...), around 1e6
    const double vals[3][9] = {
        { 0.5, -1.25, 2.0, 0.75, -0.5, 3.0, 1.5, 0.875, -0.484375 },
        { 0.1, -1.0 / 3.0, 0.7, 1.0 / 3.0, -0.1, 0.9, 0.3, 0.955336489125606, -0.29552020666133955 },
        { 1000000.1, -999999.7, 1234567.9, 1000001.3, -1000000.9, 987654.3, 1000000.7, 0.6, -0.8 },
    };
    long checks = 0, bad = 0;
    for (int kind = 0; kind < 4; kind++)
        for (int outwards = 0; outwards <= 1; outwards++)
            for (int v = 0; v < 3; v++) {
                rh_shape s;
                memset(&s, 0, sizeof s);
                s.kind = kind;
                s.outwards = outwards;
                for (int i = 0; i < 9; i++) s.v[i] = vals[v][i];
                rh_prep P, H;
                prep_one(s, P);
                rh_prep_host(s, &H);
                checks++;
                if (memcmp(&P, &H, sizeof P) != 0) { bad++; printf("rh_prep_host differs from prep_one: kind %d sign %d case %d\n", kind, outwards, v); }
                const rh_prepf F = prepf_of_kind(P, kind);
                float e[12];
                expect_record(s, e);
                checks++;
                if (memcmp(F.f, e, sizeof e) != 0) {
                    bad++;
                    printf("float record: kind %d sign %d case %d\n", kind, outwards, v);
                    for (int i = 0; i < 12; i++) printf("  f[%d] = %a, expected %a\n", i, (double)F.f[i], (double)e[i]);
                }
            }
    printf("%ld checks, %ld bad\n", checks, bad);
    return bad != 0;
}
