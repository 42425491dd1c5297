// transfer_rules.cpp -- the inter-level transfer rules of suhmo_amd/csrc/suhmo_transfer.h evaluated on the HOST: the header compiled as plain C++
// (-ffp-contract=off, address and undefined-behaviour sanitizers) by tests/test_transfer_rules_cpu.py, which compares the results bit for bit
// with the numpy twins of the rules.  CPU only; needs no device.
//   transfer_rules RULE IN OUT     IN: rows of doubles, one operand set per row (flags and kinds as 0.0 / 1.0 / ...); OUT: the results, row by row
#include <cstdio>
#include <cstring>
#include <vector>
#define __device__
#define __forceinline__ inline
#include "../../suhmo_amd/csrc/suhmo_transfer.h"

struct Rule { const char *name; int nin, nout; void (*fn)(const double *x, double *y); };
static const Rule RULES[] = {
    {"cf_tangential", 4, 3, [](const double *x, double *y) { y[0] = cf_tangential((int)x[0], x[1], x[2], x[3], y[1], y[2]); }},
    {"cf_ghost", 6, 1, [](const double *x, double *y) { y[0] = cf_ghost(x[0], x[1], x[2], x[3], x[4], x[5]); }},
    // the 3 x 3 block row by row, then xl xh yl yh tangential_only
    {"limited_slopes", 14, 2, [](const double *x, double *y) {
         double nb[3][3];
         memcpy(nb, x, sizeof nb);
         limited_slopes(nb, x[9] != 0.0, x[10] != 0.0, x[11] != 0.0, x[12] != 0.0, x[13] != 0.0, y[0], y[1]); }},
    {"child_value", 5, 1, [](const double *x, double *y) { y[0] = child_value(x[0], x[1], x[2], x[3], x[4]); }},
    {"avg4", 4, 1, [](const double *x, double *y) { y[0] = avg4(x[0], x[1], x[2], x[3]); }},
    {"avg2", 2, 1, [](const double *x, double *y) { y[0] = avg2(x[0], x[1]); }},
    {"prolong2_nl", 5, 1, [](const double *x, double *y) { y[0] = prolong2_nl(x[0], x[1], x[2], x[3], x[4]); }},
    {"bc_ghost", 4, 1, [](const double *x, double *y) { y[0] = bc_ghost((int)x[0], x[1], x[2], x[3]); }},
    // one face as the kernels chain the calls: tsize bc phihi philo cs | bf ph_hi ph_lo (twice) | fs | acc sign rscale rhs -> plain, residual
    {"reflux", 16, 2, [](const double *x, double *y) {
         double reg = reflux_coarse(x[0], x[1], x[2], x[3], x[4]);
         for (int k = 0; k < 2; k++) reg = reflux_add_fine(reg, x[0], x[5 + 3 * k], x[6 + 3 * k], x[7 + 3 * k], x[11]);
         y[0] = reflux_apply(x[12], x[13], x[14], reg);
         y[1] = reflux_residual(y[0], x[15]); }},
};

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    for (const Rule &r : RULES) {
        if (strcmp(r.name, argv[1])) continue;
        FILE *f = fopen(argv[2], "rb");
        if (!f) return 2;
        std::vector<double> in;
        double buf[4096];
        for (size_t n; (n = fread(buf, sizeof(double), 4096, f)) > 0;) in.insert(in.end(), buf, buf + n);
        fclose(f);
        if (in.size() % r.nin) return 3;
        const size_t rows = in.size() / r.nin;
        std::vector<double> out(rows * r.nout);
        for (size_t k = 0; k < rows; k++) r.fn(&in[k * r.nin], &out[k * r.nout]);
        FILE *g = fopen(argv[3], "wb");
        if (!g || fwrite(out.data(), sizeof(double), out.size(), g) != out.size()) return 2;
        fclose(g);
        return 0;
    }
    return 4;
}
