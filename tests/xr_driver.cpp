// TEST INFRASTRUCTURE (never part of the library): the planner of the synthetic radiograph - xr_plan, xr_step and xr_finish of
// csrc/prep_plan.cpp - behind a main of its own, so that it runs as a plain program under the address and undefined-behaviour sanitizers
// (tests/test_xray_cpu.py).  It touches no device.
//
//   xr_driver <cases.txt> <out.bin>
// cases.txt: one geometry per line, `nz ny nx sx sy sz sdd sod pa parallel du dv nu nv` (the floats as C99 hex floats: exact).
// out.bin: per case the return code as a float64 and, where it is 0, t [ny], a [nu], cx [nu], b [nv], cz [nv], step [nv][nu] and the float32
// radiograph (as float64) xr_finish makes of the sums 0.375 * (k * nu + i + 1).  stdout: `refused <case>: <message>` per refused case.
#include "engine_internal.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace ts2d {
static char g_error[512];
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace ts2d

static void put(FILE* f, const double* v, size_t n) {
    if (n && fwrite(v, sizeof(double), n, f) != n) { fprintf(stderr, "xr_driver: short write\n"); exit(2); }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: xr_driver <cases.txt> <out.bin>\n"); return 2; }
    FILE* in = fopen(argv[1], "r");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) { fprintf(stderr, "xr_driver: cannot open the files\n"); return 2; }
    char line[1024];
    int n_case = 0;
    while (fgets(line, sizeof(line), in)) {
        ts2d::XrGeometry g;
        char f[7][64];
        if (sscanf(line, "%d %d %d %63s %63s %63s %63s %63s %d %d %63s %63s %d %d", &g.nz, &g.ny, &g.nx, f[0], f[1], f[2], f[3], f[4], &g.pa,
                   &g.parallel, f[5], f[6], &g.nu, &g.nv) != 14) {
            fprintf(stderr, "xr_driver: malformed line %d\n", n_case);
            return 2;
        }
        g.sx = strtod(f[0], nullptr); g.sy = strtod(f[1], nullptr); g.sz = strtod(f[2], nullptr);
        g.sdd = strtod(f[3], nullptr); g.sod = strtod(f[4], nullptr); g.du = strtod(f[5], nullptr); g.dv = strtod(f[6], nullptr);
        ts2d::XrPlan pl;
        const double rc = (double)ts2d::xr_plan("xr_driver", g, &pl);
        put(out, &rc, 1);
        if (rc != 0.0) {
            printf("refused %d: %s\n", n_case++, ts2d::g_error);
            continue;
        }
        put(out, pl.t.data(), pl.t.size());
        put(out, pl.a.data(), pl.a.size());
        put(out, pl.cx.data(), pl.cx.size());
        put(out, pl.b.data(), pl.b.size());
        put(out, pl.cz.data(), pl.cz.size());
        const size_t n = (size_t)g.nu * g.nv;
        std::vector<double> step(n), sum(n), xr64(n);
        std::vector<float> xr(n);
        for (int k = 0; k < g.nv; ++k)
            for (int i = 0; i < g.nu; ++i) {
                step[(size_t)k * g.nu + i] = ts2d::xr_step(pl, k, i);
                sum[(size_t)k * g.nu + i] = 0.375 * (double)((size_t)k * g.nu + i + 1);      // (exact)
            }
        ts2d::xr_finish(pl, sum.data(), xr.data());
        for (size_t j = 0; j < n; ++j) xr64[j] = (double)xr[j];
        put(out, step.data(), n);
        put(out, xr64.data(), n);
        ++n_case;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    return 0;
}
