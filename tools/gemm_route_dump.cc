// Prints the GEMM planner's routes (controllable_xgating_amd/csrc/xg_gemm_route.h), one JSON object per input line.  Host only:
//     g++ -std=c++17 -O1 -o gemm_route_dump tools/gemm_route_dump.cc && ./gemm_route_dump < shapes.txt
// An input line is a list of key=value tokens (integers; anything not named is 0 / the tuning default):
//     mode ta tb M N K lda ldb ldc (0: contiguous) aA aB aC (address % 16) bias relu acc cs bg alone wide a16 b16 aA16 aB16
// and, for the diagnosis switches, the members of XgGemmTuning by name (no_pk pk_min no_bg force_bg no_w1 w1_bm w1_bn force_tile
// force_splitk x3_fp32 no_td td_all td_ks td_depth no_bx no_g16 g16_cfg; w1_bm sets w1_tile, force_tile sets force and force_ok).
// tools/gen_gemm_routes_golden.py records the table tests/test_gemm_routes_cpu.py pins.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "../controllable_xgating_amd/csrc/xg_gemm_route.h"

static const char* family_name(const XgGemmRoute& r) {
    switch (r.family) {
    case XGR_GEMM: return "gemm_kernel";
    case XGR_W1: return "gemm_w1";
    case XGR_PK: return "gemm_pk";
    case XGR_TD: return "gemm_td";
    case XGR_BS: return r.planes == 3 ? "gemm_bs3" : "gemm_bs1";
    case XGR_BX: return "gemm_bx";
    case XGR_G16: return "g16";
    default: return "none";
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "--w1-tiles")) {      // the candidates of the one-workgroup-per-CU kernel: [[bm, bn, bk], ...]
        printf("[");
        for (int c = 0; c < xgr::f32::W1_NTILES; ++c)
            printf("%s[%d, %d, %d]", c ? ", " : "", xgr::f32::W1_TILES[c].bm, xgr::f32::W1_TILES[c].bn, xgr::f32::W1_TILES[c].bk);
        printf("]\n");
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        XgGemmIn in{};
        XgGemmTuning t;
        std::istringstream ss(line);
        std::string tok;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "bad token: %s\n", tok.c_str()); return 2; }
            const std::string k = tok.substr(0, eq);
            const long v = atol(tok.c_str() + eq + 1);
#define KEY(name, lhs) if (k == name) { lhs; continue; }
            KEY("mode", in.mode = (int)v) KEY("wide", in.wide_forced = v != 0) KEY("ta", in.transA = v != 0) KEY("tb", in.transB = v != 0)
            KEY("M", in.M = (int)v) KEY("N", in.N = (int)v) KEY("K", in.K = (int)v)
            KEY("lda", in.lda = (int)v) KEY("ldb", in.ldb = (int)v) KEY("ldc", in.ldc = (int)v)
            KEY("aA", in.alignA = (int)v) KEY("aB", in.alignB = (int)v) KEY("aC", in.alignC = (int)v)
            KEY("bias", in.bias = v != 0) KEY("relu", in.relu = v != 0) KEY("acc", in.accumulate = v != 0) KEY("cs", in.colsum = v != 0)
            KEY("bg", in.bg = v != 0) KEY("alone", in.alone = v != 0)
            KEY("a16", in.hasA16 = v != 0) KEY("b16", in.hasB16 = v != 0) KEY("aA16", in.alignA16 = (int)v) KEY("aB16", in.alignB16 = (int)v)
            KEY("no_pk", t.no_pk = v != 0) KEY("pk_min", t.pk_min = v) KEY("no_bg", t.no_bg = v != 0) KEY("force_bg", t.force_bg = v != 0)
            KEY("no_w1", t.no_w1 = v != 0) KEY("w1_bm", (t.w1_tile = true, t.w1_bm = (int)v)) KEY("w1_bn", t.w1_bn = (int)v)
            KEY("force_tile", (t.force = t.force_ok = true, t.force_tile = (int)v)) KEY("force_splitk", t.force_splitk = (int)v)
            KEY("x3_fp32", t.x3_fp32 = (int)v) KEY("no_td", t.no_td = v != 0) KEY("td_all", t.td_all = (int)v) KEY("td_ks", t.td_ks = (int)v)
            KEY("td_depth", t.td_depth = (int)v) KEY("no_bx", t.no_bx = v != 0) KEY("no_g16", t.no_g16 = v != 0) KEY("g16_cfg", t.g16_cfg = (int)v)
#undef KEY
            fprintf(stderr, "unknown key: %s\n", k.c_str());
            return 2;
        }
        if (in.lda == 0) in.lda = in.transA ? in.M : in.K;
        if (in.ldb == 0) in.ldb = in.transB ? in.K : in.N;
        if (in.ldc == 0) in.ldc = in.N;
        const XgGemmRoute r = xg_gemm_plan(in, t);
        char rect[64] = "[]";      // [r0, c0, rows, cols] where a rectangle is cleared
        if (r.clear == XGR_CLEAR_RECT) snprintf(rect, sizeof(rect), "[%d, %d, %d, %d]", r.r0, r.c0, r.rows, r.cols);
        printf("{\"rc\": %d, \"family\": \"%s\", \"bm\": %d, \"bn\": %d, \"bk\": %d, \"vec\": %d, \"fast\": %d, \"a16\": %d, \"b16\": %d, "
               "\"splitk\": %d, \"grid\": %d, \"threads\": %d, \"gm\": %d, \"rounds\": %d, \"tail_wgs\": %d, \"ring\": %d, \"cfg\": %d, "
               "\"lds\": %d, \"pad_lds\": %d, \"clear\": %d, \"rect\": %s, \"colsum\": %d}\n",
               r.rc, family_name(r), r.bm, r.bn, r.bk, (int)r.vec, (int)r.fast, (int)r.a16, (int)r.b16, r.splitk, r.grid, r.threads, r.gm,
               r.rounds, r.tail_wgs, r.ring, r.cfg, r.lds, (int)r.pad_lds, r.clear, rect, r.colsum);
    }
    return 0;
}
