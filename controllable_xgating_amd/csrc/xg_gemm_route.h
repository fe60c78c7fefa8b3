// The GEMM planner: which kernel a product gets -- family, tile, split, grid, LDS, what is cleared first, where the column sums
// ride -- as ONE pure host function of the shape.  Host-only C++17: no HIP, no pointer, no environment, no state; it compiles with
// a plain C++ compiler (tools/gemm_route_dump.cc prints routes, tests/test_gemm_routes_cpu.py pins them), and the launchers of
// xg_gemm.hip / xg_gemm_bf16.hip / xg_gemm_g16.hip launch what it says.  The tile geometry the rules depend on lives here too and
// the kernels take it from here.
#pragma once
#include <stdint.h>
#include "../../include/xgate.h"
#include "xg_hostmath.h"

// Tile order shared by the three GEMM kernels: row-major over (tm, tn) would sweep the whole B operand once per tile row.
// With groups of `gm` tile rows walked column by column, the 32 workgroups in flight on one XCD share gm A panels and 32/gm B
// tile columns, so its 4 MB L2 holds gm + 64/gm operand panels of 128 x k_depth floats instead of 1 + 64 (measured: the
// bf16 vocabulary product re-read W from HBM at 4.3 TB/s in row-major order).  Deep reductions keep the row-major order:
// their panels do not fit anyway and consecutive tiles should then share the bigger operand's panel.
static inline int xgk_group_rows(int k_depth) {
    const int g = 4096 / (k_depth > 0 ? k_depth : 1);
    return g < 1 ? 1 : (g > 8 ? 8 : g);
}
// `mode | XGK_GEMM_BG`: the product is launched on a side stream beside a latency-bound chain of small launches; the
// persistent kernel then takes half of every CU instead of all of it (plan_pk below)
enum { XGK_GEMM_BG = 0x100,
       // `mode | XGK_GEMM_ALONE`: nothing latency-bound runs beside this product (the encoder's weight gradients at the tail of an
       // iteration): the weight-gradient layout takes the operands-from-memory kernel (gemm_td_kernel), 18 % faster alone on the
       // mid-size shapes and kept away from them elsewhere because it slows a launch chain on another stream (plan_td below)
       XGK_GEMM_ALONE = 0x200 };

namespace xgr {

// ---- tile geometry of the fp32 kernels (xg_gemm.hip)
namespace f32 {
constexpr int BKS = 32;          // slab depth
constexpr int LDK = BKS + 4;     // row stride of a k-contiguous LDS image
constexpr int MCP = 4;           // padding of a k-row of an m-contiguous LDS image
// floats of one operand's LDS image: ROWS x BK, k-contiguous rows padded by 4 (an odd number of 16-byte slots), m-contiguous by MCP
constexpr int tile_lds_floats(int rows, int bk, bool kc) { return kc ? rows * (bk + 4) : bk * (rows + MCP); }
template <int ROWS, bool KC>
struct TileGeom {
    static constexpr int lds_floats = tile_lds_floats(ROWS, BKS, KC);
    static constexpr int nvec = ROWS * BKS / 4 / 256;   // float4 per thread per slab
};
template <int ROWS, int BK, bool KC>
struct TileW {
    static constexpr int ld = KC ? BK + 4 : ROWS + MCP;
    static constexpr int lds_floats = tile_lds_floats(ROWS, BK, KC);
    static constexpr int nvec = ROWS * BK / 4 / 256;        // float4 per thread per slab
    static_assert(ROWS * BK % 1024 == 0, "tile must divide over 256 threads");
};
constexpr int TD_LDW = 68;           // row pitch of a wave's partial tile in LDS (floats)
struct W1Tile { int bm, bn, bk; };
constexpr W1Tile W1_TILES[] = {{64, 64, 128}, {64, 128, 64}, {128, 64, 64}, {128, 128, 64}, {128, 192, 32}, {192, 128, 32},
                               {128, 256, 32}, {256, 128, 32}};     // (with the slab depth: 4096-8192 MFMA cycles per slab)
constexpr int W1_NTILES = (int)(sizeof(W1_TILES) / sizeof(W1_TILES[0]));
constexpr int LDS_ONE_PER_CU = 82 * 1024;      // dynamic LDS past half a CU: the dispatcher cannot pair two such workgroups
}  // namespace f32

// ---- the register-staged bf16 kernels (xg_gemm_bf16.hip)
namespace b16 {
constexpr int BM = 128, BN = 128, BK = 32;
constexpr int LDKC = BK + 8;       // k-contiguous image: row stride in bf16 (80 B)
constexpr int LDMC = BM + 16;      // [k][m] image of an m-contiguous operand: row stride in bf16 (288 B: the 4 k rows of a
                                   // transposing read land 8 banks apart)
// an m-contiguous operand whose rows are 16-byte loadable keeps its memory order in LDS and is transposed by the READ
// (ds_read_b64_tr_b16); otherwise it is transposed by the thread assignment of dword loads into the k-contiguous image
constexpr bool tr_image_of(bool kc, bool vec) { return !kc && vec; }
constexpr int plane_elems_of(bool kc, bool vec) { return tr_image_of(kc, vec) ? BK * LDMC : BM * LDKC; }
template <bool KC, bool VEC> constexpr bool tr_image() { return tr_image_of(KC, VEC); }
template <bool KC, bool VEC = false> constexpr int plane_elems() { return plane_elems_of(KC, VEC); }
constexpr int BX_TM = 256, BX_TN = 128, BX_WGM = 4, BX_WGN = 2;      // the 256 x 128 plain-bf16 kernel: 8 waves
}  // namespace b16

// ---- the LDS-DMA bf16 kernel (xg_gemm_g16.hip)
namespace g16 {
constexpr int TM = 128, TN = 128;
// TK = slab depth (64 or 32), NS = LDS stages of the ring (NS - 1 slabs in flight while one is multiplied)
constexpr int opb_of(int tk) { return 128 * tk * 2; }              // bytes of one operand's stage image
template <int TK> constexpr int opb() { return opb_of(TK); }
template <int TK> constexpr int stb() { return 2 * opb<TK>(); }    // bytes of one stage
}  // namespace g16

}  // namespace xgr

enum XgGemmFamily { XGR_NONE = 0, XGR_GEMM, XGR_W1, XGR_PK, XGR_TD, XGR_BS, XGR_BX, XGR_G16 };
enum XgGemmClear { XGR_CLEAR_NONE = 0, XGR_CLEAR_ALL, XGR_CLEAR_RECT };
enum XgGemmColsum { XGR_CS_NONE = 0, XGR_CS_FUSED, XGR_CS_PASS };      // in the product / xgk_colsum3 before it

// What a product is, without its data.  align*: address modulo 16.
struct XgGemmIn {
    int mode;                 // 0 fp32, 1 bf16, 3 split-bf16 (XGK_GEMM_BG / XGK_GEMM_ALONE already taken out into bg / alone)
    bool wide_forced;         // the bf16 family whatever the size (modes 1 / 3 of xg_gemm_mode, xg_gemm_bf16_operands)
    bool transA, transB;
    int M, N, K, lda, ldb, ldc;
    int alignA, alignB, alignC;
    bool bias, relu, accumulate, colsum;
    bool bg, alone;
    bool hasA16, hasB16;      // bf16 copies of the operands exist ...
    int alignA16, alignB16;   // ... at these addresses modulo 16
};

// Every diagnosis switch of the routing; the member defaults are the product's rules.  The -DXG_DIAG library fills
// one from the environment, once (xg_gemm.hip: gemm_tuning, which names the variables); the product library has only the defaults.
struct XgGemmTuning {
    bool no_pk = false;               // no persistent kernel
    long pk_min = -1;                 // slabs per workgroup the persistent kernel asks for (< 0: the measured floors)
    bool no_bg = false;               // no background form (one workgroup per CU) for XGK_GEMM_BG products
    bool force_bg = false;            // every product takes the persistent kernel's background form
    bool no_w1 = false;               // no one-workgroup-per-CU kernel
    bool w1_tile = false;             // that kernel with this tile, whatever it covers
    int w1_bm = 0, w1_bn = 0;
    bool force = false;               // gemm_kernel only ...
    bool force_ok = false;            // ... and, when both numbers parsed, this tile and split
    int force_tile = 0, force_splitk = 1;
    int x3_fp32 = 1;                  // classes routed to exact fp32 in mode 3 -- 1 TN, 2 NT, 4 NN
    bool no_td = false;               // no operands-from-memory kernel
    int td_all = 0;                   // every eligible product takes gemm_td_kernel
    int td_ks = 0;                    // its split of the reduction (0: the rule)
    int td_depth = 8;                 // its ring depth: 4 / 8 / 12
    bool no_bx = false;               // no 256 x 128 plain-bf16 kernel
    bool no_g16 = false;              // no LDS-DMA kernel
    int g16_cfg = -1;                 // its configuration: 642 / 643 / 322 / 323 / 324 / 325 / 843 / 844 (< 0: the measured rule)
};

// Everything a launcher needs, and nothing it has to work out.
struct XgGemmRoute {
    int rc = XG_OK;                   // XG_EINVAL: the shape is refused, nothing is launched
    int family = XGR_NONE;
    int planes = 0;                   // gemm_bs: 1 or 3 bf16 planes
    int bm = 0, bn = 0, bk = 0;       // tile and slab depth
    bool akc = false, bkc = false;    // operand is k-contiguous
    bool vec = false;                 // 16-byte operand loads
    bool fast = false;                // fp32 vector kernels: offset-based unpredicated loads (all byte offsets < 2^31)
    bool a16 = false, b16 = false;    // operand read from its bf16 copy
    int splitk = 1;
    int grid = 0, threads = 256;
    int gm = 1;                       // tile rows per group of the tile order
    int rounds = 0, tail_wgs = 0;     // gemm_pk: whole-tile rounds, workgroups that share the tail
    int ring = 0;                     // gemm_td: steps in flight per wave; g16: LDS stages
    int cfg = 0;                      // g16: <wave groups, slab depth, stages> as one number (642 / 844 / 323 ...)
    int lds = 0;                      // dynamic LDS bytes of the launch
    bool pad_lds = false;             // ... padded past half a CU: one workgroup per CU
    int clear = XGR_CLEAR_NONE;       // what is zeroed before the launch: all of C, or rows x cols at (r0, c0)
    int r0 = 0, c0 = 0, rows = 0, cols = 0;
    int colsum = XGR_CS_NONE;
};

namespace xgr {

inline bool vec_ok(const XgGemmIn& in) {
    // 16-byte vector loads need aligned bases, ld % 4 == 0 and the vectorised extent % 4 == 0
    const bool akc = !in.transA, bkc = in.transB;
    return in.alignA == 0 && in.alignB == 0 && in.lda % 4 == 0 && in.ldb % 4 == 0 && (akc ? in.K : in.M) % 4 == 0 &&
           (bkc ? in.K : in.N) % 4 == 0;
}
inline int clear_all_if_split(const XgGemmIn& in, int splitk) {      // partial tiles are atomically added: start from zero
    return splitk > 1 && !in.accumulate ? XGR_CLEAR_ALL : XGR_CLEAR_NONE;
}

// ---- weight-gradient layout straight from memory (gemm_td_kernel); false when the product is not this kernel's kind
inline bool plan_td(const XgGemmIn& in, const XgGemmTuning& t, XgGemmRoute& r) {
    if (t.no_td || !r.fast || in.relu || in.bias || in.M % 4 || in.N % 4 || in.K % 16 || in.ldc % 4 || in.alignC != 0) return false;
    if (in.M < 64 || in.N < 64 || in.K < 16 * 16) return false;      // (>= 2 rings of 8 steps)
    const int nrounds = in.K / 16;
    const long tiles = (long)xg_cdiv(in.M, 64) * xg_cdiv(in.N, 64);
    if (tiles < 32) return false;
    // Production rule: the vocabulary head's weight gradient (a background product, or >= 1024 tiles).  The mid-size weight
    // gradients are 18 % faster here when they run ALONE (51.6 vs 61.0 us at 2048 x 512 x 2688) but the iteration is 1 % slower
    // with them (5.95-5.99 vs 5.88-5.91 ms, three runs each way, tools/ubench/td_iter*.sh): they run beside the recurrent launch
    // chains, which are the critical path, and a product that keeps 16 wide loads per wave in flight lengthens every round trip of
    // the chain next to it.  Tuning::td_all sends every eligible product here.
    if (!t.td_all && !in.bg && !in.alone && tiles < 1024) return false;
    int ks = 1;
    if (tiles < 192) { ks = (int)(256 / tiles); if (ks > nrounds / 16) ks = nrounds / 16; if (ks < 1) ks = 1; }
    if (t.td_ks > 0) ks = t.td_ks;
    if (ks > nrounds / 8) ks = nrounds / 8;      // every part: at least one ring
    const bool bg = in.bg && !t.no_bg;
    const long items = tiles * ks;
    const long rounds = xg_cdiv64(items, bg ? 256 : 512);
    r.family = XGR_TD;
    r.bm = r.bn = 64; r.bk = 16;
    r.splitk = ks;
    r.clear = clear_all_if_split(in, ks);
    r.grid = (int)xg_cdiv64(items, rounds);      // the fewest rounds, evened out over the workgroups
    r.lds = (4 * 64 * f32::TD_LDW + 256) * (int)sizeof(float);
    if (bg && r.lds < f32::LDS_ONE_PER_CU) { r.lds = f32::LDS_ONE_PER_CU; r.pad_lds = true; }      // one workgroup per CU beside a launch chain (see plan_pk)
    r.ring = t.td_depth == 4 ? 4 : (t.td_depth == 12 && nrounds / ks >= 12 ? 12 : 8);      // (td_depth: tests run the 4- and 12-step rings too)
    return true;
}

// ---- the one-workgroup-per-CU kernel (gemm_w1_kernel): the tile (wave grid 2 x 2 of 32 x 32 MFMA tiles) whose ONE round over the
// 256 CUs wastes the least; false when no candidate covers the chip well enough (or the shape is not its kind)
inline bool plan_w1(const XgGemmIn& in, const XgGemmTuning& t, XgGemmRoute& r) {
    if (t.no_w1 || !r.fast || r.colsum == XGR_CS_FUSED || in.bg || in.K < 256) return false;
    int best = -1;
    double best_eff = 0.0;
    for (int c = 0; c < f32::W1_NTILES; ++c) {
        const f32::W1Tile& w = f32::W1_TILES[c];
        if (in.K % w.bk || in.M < w.bm / 2 || in.N < w.bn / 2) continue;
        const long tiles = (long)xg_cdiv(in.M, w.bm) * xg_cdiv(in.N, w.bn);
        if (t.w1_tile) { if (w.bm == t.w1_bm && w.bn == t.w1_bn) { best = c; best_eff = 1.0; } continue; }
        if (tiles > 256) continue;
        // useful fraction of the chip's matrix time in that one round; larger tiles stream fewer operand bytes per flop
        const double eff = (double)in.M * in.N / (256.0 * w.bm * w.bn);
        const double score = eff * (w.bm * w.bn >= 128 * 128 ? 1.03 : (w.bm * w.bn >= 64 * 128 ? 1.0 : 0.97));
        if (score > best_eff) { best_eff = score; best = c; }
    }
    if (best < 0 || best_eff < 0.70) return false;
    const f32::W1Tile& w = f32::W1_TILES[best];
    r.family = XGR_W1;
    r.bm = w.bm; r.bn = w.bn; r.bk = w.bk;
    r.splitk = 1;
    r.gm = xgk_group_rows(in.K);
    r.grid = xg_cdiv(in.M, w.bm) * xg_cdiv(in.N, w.bn);
    r.lds = 2 * (f32::tile_lds_floats(w.bm, w.bk, r.akc) + f32::tile_lds_floats(w.bn, w.bk, r.bkc)) * (int)sizeof(float);
    return true;
}

// ---- the persistent 128 x 128 kernel (gemm_pk_kernel); false when the shape should take the one-tile-per-workgroup kernel
inline bool plan_pk(const XgGemmIn& in, const XgGemmTuning& t, XgGemmRoute& r) {
    constexpr int BM = 128, BN = 128;
    if (t.no_pk || !r.fast || in.M < BM || in.N < BN) return false;
    const int ntm = xg_cdiv(in.M, BM), ntn = xg_cdiv(in.N, BN), nslab = xg_cdiv(in.K, f32::BKS);
    const int gm = xgk_group_rows(in.K);             // the persistent kernel walks whole reductions
    const long T = (long)ntm * ntn;
    const long units = T * nslab;
    // measured (tools/ubench/gemm_bench.py): the persistent form wins 3-6 % when every workgroup has >= ~40 slabs of work
    // (vocabulary head: logits, dW_logit, dH) and loses 10-15 % to 64x64 tiles + split-K on the mid-size products
    const long min_units = t.pk_min >= 0 ? t.pk_min : 40;      // (pk_min: tests force the kernel onto small shapes)
    // 2 workgroups per CU (73.7 KB of LDS each) -- or, for a background product, ONE per CU (LDS padded past half a CU so
    // that the dispatcher cannot pair them): 512 persistent workgroups own every register file and LDS for the whole
    // product (0.7 ms for dW_logit), and a recurrent chain on another stream then waits for leftovers -- its step took
    // 120 us instead of 53 beside dW_logit.  One workgroup per CU leaves 256 VGPRs per SIMD and 78 KB of LDS, exactly one
    // 8-wave (or two 4-wave) skinny workgroups, and costs the product itself ~10 %.
    const bool bg = (in.bg || t.force_bg) && !t.no_bg;      // (force_bg: tests send every product through the background form)
    const int GMAX = bg ? 256 : 512;
    // A background product is here for the chain beside it, not for its own speed: every other kernel of this file fills whole
    // CUs and stops that chain.  Its floor is what the one-workgroup-per-CU grid needs -- one share of 4 slabs for each of the 256
    // workgroups -- so that a chunk of two or three decoder steps' logits (256 x 20000 x 512: 314 tiles, one round + 58) still
    // runs in this form, and so does a product of fewer than 256 tiles (rounds == 0: stream-K shares only).  Everything else
    // keeps the measured floor above.
    if (units < (bg && t.pk_min < 0 ? 256L * 4 : 512L * min_units)) return false;
    int G, rounds, tail_wgs;
    const bool split = !in.relu && nslab >= 2;
    if (!split) {
        if (T < GMAX) return false;
        // whole tiles only (a ReLU epilogue cannot be split): the fewest rounds, evened out over the workgroups; the ragged
        // last round goes through the tail logic as one whole tile per share
        G = (int)xg_cdiv64(T, xg_cdiv64(T, GMAX));
        rounds = (int)(T / G);
        tail_wgs = (int)(T - (long)rounds * G);
    } else {
        G = GMAX;
        rounds = (int)(T / G);
        const long tail = T - (long)rounds * G;
        const long U = tail * nslab;
        long tw = U / 4;                            // >= 4 slabs per share
        if (tw > G) tw = G;
        if (tail > 0 && tw < 1) tw = 1;
        tail_wgs = (int)tw;
    }
    // zero the tiles that receive partial sums (non-accumulating products only): every tail tile unless each share is a
    // whole tile.  The tail is the END of the swizzled order: inside the last group of tile rows it is a set of whole tile
    // columns plus at most one partial column -- clear the bounding rectangle (whole tiles inside it overwrite the zeros).
    const long dp = (long)rounds * G, tail = T - dp;
    const bool whole_shares = tail == tail_wgs;     // one tile per share (U / tail_wgs == nslab)
    int clear = XGR_CLEAR_NONE, r0 = 0, c0 = 0;
    if (tail > 0 && !whole_shares && !in.accumulate) {
        if (in.ldc % 4 != 0 || in.alignC != 0) return false;
        const int per = gm * ntn;
        const int grp = (int)(dp / per), first = grp * gm, gsz = (ntm - first) < gm ? (ntm - first) : gm;
        const int tn0 = (int)((dp - (long)grp * per) / gsz);
        const bool one_group = first + gsz >= ntm;               // tail confined to the last group
        r0 = first * BM; c0 = one_group ? tn0 * BN : 0;
        if (r0 < in.M && c0 < in.N) clear = XGR_CLEAR_RECT;
    }
    r.family = XGR_PK;
    r.bm = BM; r.bn = BN; r.bk = f32::BKS;
    r.splitk = 1;
    r.gm = gm;
    r.grid = G; r.rounds = rounds; r.tail_wgs = tail_wgs;
    r.clear = clear;
    if (clear == XGR_CLEAR_RECT) { r.r0 = r0; r.c0 = c0; r.rows = in.M - r0; r.cols = in.N - c0; }
    r.lds = 2 * (f32::tile_lds_floats(BM, f32::BKS, r.akc) + f32::tile_lds_floats(BN, f32::BKS, r.bkc)) * (int)sizeof(float) + 4096;   // + csum scratch
    if (bg && r.lds < f32::LDS_ONE_PER_CU) { r.lds = f32::LDS_ONE_PER_CU; r.pad_lds = true; }
    return true;
}

// ---- exact fp32 (xg_gemm.hip): td -> w1 -> pk -> one tile per workgroup
inline XgGemmRoute plan_f32(const XgGemmIn& in, const XgGemmTuning& t, XgGemmRoute r) {
    const int M = in.M, N = in.N, K = in.K;
    r.vec = vec_ok(in);
    {   // offset-based loads: the largest byte offset inside either operand must fit 31 bits, and the m/n-contiguous
        // clamp needs at least 4 rows
        const uint64_t ea = (uint64_t)(r.akc ? M : K) * (uint64_t)(int64_t)in.lda, eb = (uint64_t)(r.bkc ? N : K) * (uint64_t)(int64_t)in.ldb;
        r.fast = (ea * 4 < (1u << 31)) && (eb * 4 < (1u << 31)) && M >= 4 && N >= 4;
    }
    // column sums: fused into the vector kernels (the tiles of tile column 0 sum the A slabs they stream anyway); the
    // scalar-load kernels get a separate pass
    r.colsum = in.colsum ? (r.vec ? XGR_CS_FUSED : XGR_CS_PASS) : XGR_CS_NONE;
    const long t128 = (long)xg_cdiv(M, 128) * xg_cdiv(N, 128);
    const long t64 = (long)xg_cdiv(M, 64) * xg_cdiv(N, 64);
    const int nslab = xg_cdiv(K, f32::BKS);
    int splitk = 1;
    bool big = false;
    // measured on MI355X (tools/ubench/gemm_bench.py): 128x128 wins with >= ~400 tiles (x2 split when the reduction is
    // deep), and for FEW tiles under a very deep reduction (dH = dlogits W: 84 tiles, K = 20000) when split-K fills exactly
    // one round of 512 workgroups (87.6 -> 104 TF); otherwise 64x64 tiles with enough K splits to put ~1000-1500
    // workgroups in flight.  (A per-shape cost model over rounds x depth was tried and lost on the mid-size shapes.)
    if (t128 >= 1024) big = true;
    else if (t128 >= 384) { big = true; if (!in.relu && nslab >= 32) splitk = 2; }
    else if (!in.relu && t128 >= 32 && nslab >= 256 && 512 / t128 >= 2) {
        big = true;
        long sk = 512 / t128;
        if (sk > nslab / 16) sk = nslab / 16;
        splitk = (int)sk;
    }
    else if (!in.relu && t64 >= 4) {
        const long target = (r.akc && r.bkc) ? 768 : 1536;
        long sk = target / t64;
        if (sk > nslab / 16) sk = nslab / 16;      // keep K >= 512 per split
        if (sk >= 2) splitk = (int)sk;
    }
    // tuning hook for tools/ubench/gemm_bench.py: this tile and split
    if (t.force_ok) { big = t.force_tile == 128; splitk = in.relu ? 1 : (t.force_splitk < 1 ? 1 : t.force_splitk); }
    if (r.vec && !t.force) {
        if (!r.akc && !r.bkc && plan_td(in, t, r)) return r;      // the weight-gradient layout: operands straight from memory
        if (plan_w1(in, t, r)) return r;
        if (plan_pk(in, t, r)) return r;
    }
    r.family = XGR_GEMM;
    r.bm = r.bn = big ? 128 : 64; r.bk = f32::BKS;
    r.splitk = splitk;
    r.gm = xgk_group_rows(K / splitk);
    r.clear = clear_all_if_split(in, splitk);
    r.grid = xg_cdiv(M, r.bm) * xg_cdiv(N, r.bn) * splitk;
    r.lds = 2 * (f32::tile_lds_floats(r.bm, f32::BKS, r.akc) + f32::tile_lds_floats(r.bn, f32::BKS, r.bkc)) * (int)sizeof(float);
    return r;
}

// Shapes the DMA kernel handles (xg_gemm_g16.hip, header, on edges): 16-byte loadable rows, 32-bit byte offsets, and a K tail only
// where one operand supplies zeros for it (an m-contiguous operand: its k rows past K are past the end of the buffer) while the
// other's overrun stays inside its own data (k-contiguous with lda == K: the next row's head; or m-contiguous as well).
// (base alignment, pitch % 8 and extent % 8 are what made the bf16 copies usable at all: r.a16 && r.b16)
inline bool g16_ok(const XgGemmIn& in, const XgGemmRoute& r) {
    const int M = in.M, N = in.N, K = in.K;
    if (!r.a16 || !r.b16 || M < 128 || N < 128 || K < 128) return false;
    const int64_t ea = (int64_t)((r.akc ? M : K) + 128) * in.lda * 2, eb = (int64_t)((r.bkc ? N : K) + 128) * in.ldb * 2;
    if (ea >= (int64_t)1 << 31 || eb >= (int64_t)1 << 31) return false;
    if (K % 64) {
        const bool a_zero = !r.akc, b_zero = !r.bkc;                  // zero k rows past K for free
        const bool a_safe = !r.akc || in.lda == K, b_safe = !r.bkc || in.ldb == K;
        if (!((a_zero && b_safe) || (b_zero && a_safe))) return false;
    }
    return true;
}
inline XgGemmRoute plan_g16(const XgGemmIn& in, const XgGemmTuning& t, XgGemmRoute r) {
    // Configuration <wave groups, slab depth, ring stages> (tools/ubench/g16_cfg.sh / g16_burst.sh, products alone):
    //   64-deep slabs in two stages, four waves, two workgroups per CU ("642") everywhere but the weight-gradient layout, where
    //   - with at most one tile per CU, EIGHT waves per tile win (two groups of four that split every slab's depth; one workgroup
    //     per CU, four-stage ring: "844"): 4096 x 1024 x 5120 58-65 against 71-73 us, 4096 x 1024 x 2688 36-40 against 48-53,
    //     1024 x 1536 x 5120 40-43 against 48-54 -- and lose everywhere else (logits 241 against 200, dH 193 against 143);
    //   - with >= 1024 tiles, 32-deep slabs in three stages (three workgroups per CU, "323") are 10-20 % ahead (dW_logit 143
    //     against 173 us); wherever an operand is k-contiguous they lose (64-byte row pieces = half cache lines).
    //   One workgroup of four waves per CU with three 64-deep stages loses everywhere (277 against 188 us on the logits): what this
    //   kernel needs is waves to switch to, not bytes in flight.
    const long tiles = (long)xg_cdiv(in.M, g16::TM) * xg_cdiv(in.N, g16::TN);
    const bool tn_layout = !r.akc && !r.bkc;
    const int c = t.g16_cfg >= 0 ? t.g16_cfg : (tn_layout && tiles >= 1024 ? 323 : (tn_layout && tiles <= 256 ? 844 : 642));
    // Split of the reduction across workgroups.  A part's result is added with fp32 atomics behind a memset of C, and that
    // epilogue is expensive here: 5120 x 1024 x 1536 takes 34 us unsplit and 58-70 us in two parts, 5120 x 1024 x 4096 76 against
    // 85-114 us.  Measured rule (tools/ubench/g16_sk.sh): split only while tiles x parts stay ONE round of the slots (512 with two
    // workgroups per CU, 256 with one) and every part keeps a reduction of >= 2560 -- 2688 x 1024 x 20000: 3 parts (158 us; 1 / 2 / 4
    // parts: 322 / 198 / 228) -- or, while the tiles alone leave CUs empty, of >= 1024 (1024 x 1536 x 5120, 96 tiles, four waves:
    // 87 / 65 / 55 / 51 / 52 us in 1 / 2 / 3 / 4 / 5 parts).
    // (Keeping a product beside a latency-bound chain, XGK_GEMM_BG, to ONE workgroup per CU was measured at the end of round 5 and
    //  is inside the noise: gone.)
    int splitk = 1;
    if (!in.relu) {
        const long slots = c >= 800 ? 256 : 512;
        const int deep = tiles < 256 ? 1024 : 2560;
        long sk = slots / tiles;
        if (sk > in.K / deep) sk = in.K / deep;
        splitk = sk < 1 ? 1 : (int)sk;
    }
    int kg = 1;                       // 844 / 843: eight waves (two k groups), one workgroup per CU
    r.cfg = c;
    switch (c) {
    case 323: r.bk = 32; r.ring = 3; break;
    case 844: r.bk = 64; r.ring = 4; kg = 2; break;
    case 322: r.bk = 32; r.ring = 2; break;          // (this one and the four below: instantiated in the diag library only)
    case 843: r.bk = 64; r.ring = 3; kg = 2; break;
    case 643: r.bk = 64; r.ring = 3; break;
    case 324: r.bk = 32; r.ring = 4; break;
    case 325: r.bk = 32; r.ring = 5; break;
    default: r.cfg = 642; r.bk = 64; r.ring = 2; break;
    }
    r.family = XGR_G16;
    r.bm = g16::TM; r.bn = g16::TN;
    r.splitk = splitk;
    r.gm = xgk_group_rows(in.K / splitk / 2);          // (an operand panel is 128 x k_depth bf16 = half the bytes the rule was made for)
    r.clear = clear_all_if_split(in, splitk);
    r.grid = xg_cdiv(in.M, g16::TM) * xg_cdiv(in.N, g16::TN) * splitk;
    r.threads = 256 * kg;
    r.lds = r.ring * 2 * g16::opb_of(r.bk);
    return r;
}

// ---- the bf16 matrix cores (xg_gemm_bf16.hip, xg_gemm_g16.hip): planes = 1 bf16 compute, 3 split-bf16 (fp32-class accuracy)
inline XgGemmRoute plan_wide(const XgGemmIn& in, const XgGemmTuning& t, XgGemmRoute r) {
    const int M = in.M, N = in.N, K = in.K, planes = in.mode;
    r.vec = vec_ok(in);
    r.colsum = in.colsum ? XGR_CS_FUSED : XGR_CS_NONE;      // every kernel of the family sums the A slabs of its tn == 0 tiles
    if (planes == 1 && r.vec) {      // 16-byte loads of 8 bf16: base, pitch and contiguous extent in multiples of 8 elements
        const int xa = r.akc ? K : M, xb = r.bkc ? K : N;
        r.a16 = in.hasA16 && in.alignA16 == 0 && in.lda % 8 == 0 && xa % 8 == 0 && xa >= 8;
        r.b16 = in.hasB16 && in.alignB16 == 0 && in.ldb % 8 == 0 && xb % 8 == 0 && xb >= 8;
    }
    const long tiles = (long)xg_cdiv(M, b16::BM) * xg_cdiv(N, b16::BN);
    const int nslab = xg_cdiv(K, b16::BK);
    int splitk = 1;
    if (!in.relu && tiles < 512) {                  // fill the chip by splitting deep reductions (3 workgroups per CU would fit,
                                                    // but 768 shares were measured slower: dX 52 -> 83 us, dW_logit 157 -> 169 us)
        // ... and never PAST the 512 slots (round 5): the rule used to round up, so 104 tiles became 5 x 104 = 520 workgroups -- a
        // second round for 8 of them -- and 416 tiles two rounds of 832.  Rounded down (split-bf16, alone): encoder embedding
        // 98 -> 63 us, dX 110 -> 74, PRE 104 -> 59, v2a(V) 94 -> 58 (tools/ubench/bs_skmax.sh)
        long sk = 512 / tiles;
        if (sk > nslab / 8) sk = nslab / 8;
        if (sk >= 2) splitk = (int)sk;
    }
    // plain bf16 with a k-contiguous A (forward and data-gradient layouts): 256 x 128 tiles, 43 flop per operand byte instead
    // of 32 -- logits 170 -> 145 us, PRE 79 -> 59 us; hidden-1024 iteration 9.19 -> 9.02 ms.  Measured and not used: the
    // weight-gradient layout on these tiles (dW_logit 186 -> 276 us) and 256 x 256 tiles (one workgroup per CU: 10.4 ms).
    if (planes == 1 && r.vec && r.akc && !t.no_bx && M >= 256 && !r.a16 && !r.b16) {
        const long t2 = (long)xg_cdiv(M, b16::BX_TM) * xg_cdiv(N, b16::BX_TN);
        splitk = 1;
        if (!in.relu && t2 < 256) {
            long sk = (256 + t2 - 1) / t2;
            if (sk > nslab / 8) sk = nslab / 8;
            if (sk >= 2) splitk = (int)sk;
        }
        r.family = XGR_BX;
        r.planes = 1;
        r.bm = b16::BX_TM; r.bn = b16::BX_TN; r.bk = b16::BK;
        r.splitk = splitk;
        r.gm = xgk_group_rows(2 * K / splitk);
        r.clear = clear_all_if_split(in, splitk);
        r.grid = (int)t2 * splitk;
        r.threads = 64 * b16::BX_WGM * b16::BX_WGN;
        r.lds = (b16::BX_TM + b16::BX_TN) * b16::LDKC * (int)sizeof(unsigned short);
        return r;
    }
    // both operands bf16 in memory: tiles by LDS-DMA, 64-deep slabs, one barrier per slab
    if (!t.no_g16 && g16_ok(in, r)) return plan_g16(in, t, r);
    r.family = XGR_BS;
    r.planes = planes;
    r.bm = b16::BM; r.bn = b16::BN; r.bk = b16::BK;
    r.splitk = splitk;
    r.gm = xgk_group_rows(K / splitk);
    r.clear = clear_all_if_split(in, splitk);
    r.grid = (int)tiles * splitk;
    r.lds = planes * (b16::plane_elems_of(r.akc, r.vec) + b16::plane_elems_of(r.bkc, r.vec)) * (int)sizeof(unsigned short);
    return r;
}

}  // namespace xgr

// The route of a product.  (M <= 0 || N <= 0 is no product: the callers return XG_OK before they get here.)
inline XgGemmRoute xg_gemm_plan(const XgGemmIn& in, const XgGemmTuning& t = XgGemmTuning()) {
    XgGemmRoute r;
    r.akc = !in.transA;   // A (M,K) row-major -> k contiguous
    r.bkc = in.transB;    // B (N,K) row-major -> k contiguous
    // (column sums are a side output of the weight-gradient layout only: transA)
    if (in.colsum && !in.transA) { r.rc = XG_EINVAL; return r; }
    // large products may run on the bf16 matrix cores (split-bf16 or plain bf16); skinny / tiny ones stay fp32
    // Split-bf16 (mode 3) keeps the weight-gradient layout (transA) in exact fp32 (round 5): alone the fp32 kernels are level or
    // ahead there (2048 x 512 x 2688: 60 against 65 us, dW_logit 504 against 530), and inside the iteration the 21 split-bf16
    // weight gradients ran at 131 us each beside the chains (63 alone) and held the encoder's backward and the update back by
    // 0.4 ms.  The other layouts stay split (logits 453 against 539 us, dH 381 against 514, PRE 58 against 80).
    // (Tuning::x3_fp32 = mask of the classes routed to exact fp32 in mode 3 -- 1 TN, 2 NT, 4 NN; default 1)
    const bool x3_exact = in.mode == 3 && (t.x3_fp32 & (in.transA ? 1 : (in.transB ? 2 : 4)));
    // (... and shallow reductions: the gradients of the initial-state projections are R x R x B products -- 1024 x 1024 x 128 at hidden
    // 1024 -- that took 62 us each on the bf16 tile kernel, four slabs per tile)
    constexpr int bf16_mink = 256;
    const bool wide = (in.mode == 1 || in.mode == 3) && (in.wide_forced || (!x3_exact && in.M >= 256 && in.N >= 64 && in.K >= bf16_mink));
    return wide ? xgr::plan_wide(in, t, r) : xgr::plan_f32(in, t, r);
}
