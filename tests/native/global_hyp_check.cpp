// Host check of csrc/global_hyp.h, the validity tests, frames and transform of rh_register_global's hypotheses.  Built with
// -fsanitize=address,undefined -ffp-contract=off and run by tests/test_global_host.py::test_hypotheses_under_the_sanitizers
// (g++, no GPU).  The cases are those the numpy twin is pinned by: a quarter turn about z plus an integer shift comes back
// with every entry exact, and every validity clause refuses its triple.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "global_hyp.h"

static long bad = 0, checks = 0;
static void expect(bool ok, const char *what) { checks++; if (!ok) { bad++; printf("FAILED: %s\n", what); } }

int main() {
    const double Q[7][3] = { { 0, 0, 0 }, { 3, 0, 0 }, { 0, 3, 0 }, { 6, 0, 0 }, { 1, 2, 3 }, { -4, 5, 1 }, { 2, 2, 2 } };
    const double shift[3] = { 5, -7, 2 };
    std::vector<double> pairs(7 * 6);              // heap: the sanitizer sees every read past the last pair
    for (int i = 0; i < 7; i++) {
        for (int k = 0; k < 3; k++) pairs[6 * i + k] = Q[i][k];
        pairs[6 * i + 3] = -Q[i][1] + shift[0];    // Rz: (x, y, z) -> (-y, x, z)
        pairs[6 * i + 4] = Q[i][0] + shift[1];
        pairs[6 * i + 5] = Q[i][2] + shift[2];
    }
    rh_global_params p;
    memset(&p, 0, sizeof p);
    p.trials = 1; p.tau = 1e-9; p.edge_ratio = 0.9; p.min_edge = 0.0;
    GlobHyp h;
    expect(gl_hypothesis(pairs.data(), 0, 1, 2, p, h), "the triple (0, 1, 2) is valid");
    const double Rz[9] = { 0, -1, 0, 1, 0, 0, 0, 0, 1 };
    for (int k = 0; k < 9; k++) expect(h.R[k] == Rz[k], "R is the quarter turn, every entry exact");
    for (int k = 0; k < 3; k++) expect(h.t[k] == shift[k], "t is the shift, every entry exact");
    for (int i = 0; i < 7; i++)                    // every pair agrees exactly: the count of step 5 is c
        for (int k = 0; k < 3; k++) {
            const double *q = &pairs[6 * i];
            const double z = (((h.R[3 * k] * q[0] + h.R[3 * k + 1] * q[1]) + h.R[3 * k + 2] * q[2]) + h.t[k]) - q[3 + k];
            expect(z == 0.0, "a residual of the exact image is zero");
        }
    expect(gl_hypothesis(pairs.data(), 6, 4, 5, p, h), "the last pairs are addressed (6, 4, 5)");
    // each validity clause
    expect(!gl_hypothesis(pairs.data(), 0, 1, 1, p, h) && !gl_hypothesis(pairs.data(), 0, 0, 2, p, h) && !gl_hypothesis(pairs.data(), 2, 1, 2, p, h),
           "a repeated index");
    expect(!gl_hypothesis(pairs.data(), 0, 1, 3, p, h), "a collinear triple has no frame");
    p.min_edge = 3.0;
    expect(gl_hypothesis(pairs.data(), 0, 1, 2, p, h), "min_edge = the shortest query edge");
    p.min_edge = 3.0000001;
    expect(!gl_hypothesis(pairs.data(), 0, 1, 2, p, h), "min_edge above the shortest query edge");
    p.min_edge = 0.0;
    std::vector<double> twice(pairs);
    for (int i = 0; i < 7; i++) for (int k = 3; k < 6; k++) twice[6 * i + k] *= 2.0;
    expect(!gl_hypothesis(twice.data(), 0, 1, 2, p, h), "reference edges twice as long: 9 < 0.81 * 36");
    p.edge_ratio = 0.5;
    expect(gl_hypothesis(twice.data(), 0, 1, 2, p, h), "edge_ratio 0.5 accepts 9 >= 0.25 * 36");
    std::vector<double> same(pairs);               // identical points: hh = 0, no division by it
    for (int k = 0; k < 6; k++) same[6 + k] = same[k];
    p.edge_ratio = 1.0;
    expect(!gl_hypothesis(same.data(), 0, 1, 2, p, h), "a zero edge has no frame");
    double F[3][3];
    const double x0[3] = { 1, 1, 1 }, x1[3] = { 1, 1, 3 }, x2[3] = { 1, 5, 1 };
    expect(gl_frame(x0, x1, x2, F) && F[2][0] == 1.0 && F[1][1] == 1.0 && F[0][2] == -1.0 && F[0][0] == 0.0,
           "a frame by hand: e1 = e_z, e3 = e_z x e_y = -e_x, e2 = e3 x e1 = e_y");
    expect(!gl_frame(x0, x0, x2, F) && !gl_frame(x0, x1, x1, F), "no frame without two directions");
    printf("%ld checks, %ld bad\n", checks, bad);
    return bad ? 1 : 0;
}
