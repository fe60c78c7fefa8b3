// bf16 GEMM for operands that are BOTH bf16 in memory (gemm_mode 1 with weight shadows / activation mirrors): the tiles go
// global -> LDS by LDS-DMA (`buffer_load_dwordx4 ... lds`, 1 KiB per wave-instruction), never through registers.
//
//   C[M,N] (+)= op(A) op(B) (+ bias, relu), fp32 accumulate, v_mfma_f32_32x32x16_bf16.
//   128 x 128 tiles, a wave's share 64 x 64 = 2 x 2 MFMA tiles; a ring of NS LDS stages of TK-deep slabs, filled by DMA and drained
//   by COUNT (s_waitcnt vmcnt(N) + the raw s_barrier: __syncthreads() would drain the whole DMA queue), ONE barrier per slab; the
//   DMA instructions of the next slab sit between the MFMA groups of the slab being multiplied.  Three forms (xg_gemm_route.h: plan_g16 picks):
//     TK 64, NS 2, four waves  -- 64 KiB, two workgroups per CU: the default;
//     TK 32, NS 3, four waves  -- 48 KiB, three workgroups per CU: the weight-gradient layout with >= 1024 tiles;
//     TK 64, NS 4, EIGHT waves -- two groups of four share the tile and split every slab's depth, 128 KiB, one workgroup per CU:
//                                 weight gradients of at most one tile per CU.
//
// The predecessor (xg_gemm_bf16.hip: gemm_bs_kernel<1,..,A16,B16>) staged 32-deep slabs through registers into ONE LDS image with
// two barriers per slab: 516-576 TF alone on the hidden-1024 vocabulary shapes.  What an LDS-DMA costs is that the LDS image of
// a wave-instruction is lane-linear (base + 16 * lane): no padding.  Bank conflicts are removed by a swizzle that is applied
// on the SOURCE side (which 16 bytes of global memory a lane fetches) and undone by the fragment reads:
//   k-contiguous operand  (rows x 64 k, 128 B per row):  16-byte slot j of row r is stored in slot j ^ ((r >> 1) & 7).
//        A ds_read_b128 fragment read (32 rows x one slot per half-wave) is serviced in the 16-lane groups
//        {0-3,12-15,20-27} / {4-11,16-19,28-31}: their 8 even and 8 odd rows get 8 distinct slots of each 128-byte half of the
//        256-byte bank row -> conflict-free.
//   m-contiguous operand  (64 k x 128 m, 256 B per k row = one bank row; transposed by ds_read_b64_tr_b16):  the four 64-byte
//        quarters of k row k are stored XOR-ed with (k & 3): the four k rows of one transposing read land in four quarters.
// Edges: the DMA goes through a buffer descriptor whose extent is the operand's; a fetch past the end writes zeros.  Rows past
// the last row of a k-contiguous operand and k rows past K of an m-contiguous operand are therefore zero for free; columns
// past the end of an INNER row fetch the next row's head (finite data), which only ever meets unstored outputs or a zero row
// of the other operand -- the planner (xg_gemm_route.h: g16_ok) admits exactly the shapes for which that holds.
#include "xg_common.h"
#include "xg_kernels.h"
#include <cstdlib>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short v4s __attribute__((ext_vector_type(4)));

namespace {

using namespace xgr::g16;      // TM, TN, opb, stb: xg_gemm_route.h (the planner sizes LDS from them)

struct GArgs {
    const unsigned short* A; const unsigned short* B; float* C; const float* bias;
    int M, N, K, lda, ldb, ldc, relu, accumulate, splitk, gm;
    float* csum[3];
    int pad_;
};

typedef __attribute__((address_space(3))) void lds_void;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t g16_rsrc(const unsigned short* P, unsigned bytes) {
    const uint64_t a = reinterpret_cast<uint64_t>(P);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a), hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, (int)bytes, 0x00020000);
}

// per-lane byte offsets of a wave's four DMA instructions into the operand, slab 0 (the range check of a raw buffer looks at
// the VECTOR offset only, so the whole offset lives there; a slab advance is one add per instruction)
template <bool KC, int TK, int NI>
__device__ __forceinline__ void g16_offsets(unsigned (&off)[NI], int ld, int r0, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int q = wave * NI + i;
        if (KC) {       // TK = 64: instruction q = rows 8q .. 8q + 7; lane -> row 8q + (lane >> 3), stored slot lane & 7
                        // TK = 32: rows 16q .. 16q + 15 of 64 bytes; lane -> row 16q + (lane >> 2), stored slot lane & 3
            constexpr int LPR = TK / 8;                      // lanes (16-byte slots) per row
            const int r = q * (64 / LPR) + lane / LPR;
            const int x = TK == 64 ? ((r >> 1) & 7) : ((r >> 2) & 3);
            const int j = (lane % LPR) ^ x;
            off[i] = ((unsigned)(r0 + r) * (unsigned)ld + (unsigned)j * 8u) * 2u;
        } else {        // instruction q = k rows 4q .. 4q + 3; lane -> k row 4q + (lane >> 4), stored slot lane & 15
            const int k = q * 4 + (lane >> 4);
            const int j = (lane & 15) ^ ((k & 3) << 2);
            off[i] = ((unsigned)k * (unsigned)ld + (unsigned)(r0 + j * 8)) * 2u;
        }
    }
}

// KG = 2: eight waves -- two groups of four that share the tile and split every slab's depth between them (same tile, same operand
// traffic, twice the waves per workgroup: ONE workgroup per CU with a four-stage ring = three slabs in flight instead of one);
// the groups exchange the half of the accumulators they do not store through LDS at the end.
template <bool AKC, bool BKC, int TK, int NS, int KG>
__global__ void __launch_bounds__(256 * KG, 2) gemm_g16_kernel(GArgs g) {
    constexpr int NI = TK / 16 / KG, OPB = opb<TK>(), STB = stb<TK>(), P = NS - 1;      // NI: DMA instructions per wave, operand and slab
    static_assert(KG == 1 || (KG == 2 && TK == 64), "two wave groups: 64-deep slabs, two 16-deep blocks each");
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem_g16[];

    const int ntm = (g.M + TM - 1) / TM, ntn = (g.N + TN - 1) / TN;
    const int nwg = ntm * ntn * g.splitk;
    int bid = blockIdx.x;
    {
        const int q = nwg / 8, r = nwg % 8, xcd = bid % 8, idx = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int ks = bid % g.splitk;
    bid /= g.splitk;
    int tm, tn;
    {
        const int per = g.gm * ntn, grp = bid / per, in = bid - grp * per;
        const int first = grp * g.gm, gsz = min(ntm - first, g.gm);
        tn = in / gsz;
        tm = first + (in - tn * gsz);
    }
    const int m0 = tm * TM, n0 = tn * TN;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int w4 = wave & 3, kg = wave >> 2;
    const int wm = w4 >> 1, wn = w4 & 1, half = lane >> 5, l31 = lane & 31;

    const int nslab_all = (g.K + TK - 1) / TK;
    const int s_begin = (int)(((long)ks * nslab_all) / g.splitk), s_end = (int)(((long)(ks + 1) * nslab_all) / g.splitk);

    // ---- DMA side
    const __amdgpu_buffer_rsrc_t rsA = g16_rsrc(g.A, AKC ? ((unsigned)(g.M - 1) * g.lda + g.K) * 2u : ((unsigned)(g.K - 1) * g.lda + g.M) * 2u);
    const __amdgpu_buffer_rsrc_t rsB = g16_rsrc(g.B, BKC ? ((unsigned)(g.N - 1) * g.ldb + g.K) * 2u : ((unsigned)(g.K - 1) * g.ldb + g.N) * 2u);
    unsigned offA[NI], offB[NI];
    g16_offsets<AKC, TK, NI>(offA, g.lda, m0, wave, lane);
    g16_offsets<BKC, TK, NI>(offB, g.ldb, n0, wave, lane);
    const unsigned slabA = AKC ? TK * 2u : (unsigned)TK * (unsigned)g.lda * 2u;
    const unsigned slabB = BKC ? TK * 2u : (unsigned)TK * (unsigned)g.ldb * 2u;
#pragma unroll
    for (int i = 0; i < NI; ++i) { offA[i] += (unsigned)s_begin * slabA; offB[i] += (unsigned)s_begin * slabB; }
    // (Every workgroup walks its slabs from the first one.  Workgroups of one round run in step and the tiles that share an operand
    // panel then ask L2 for the same slab at the same moment; a tile-dependent start -- tried against the suspicion that 2 KB row
    // pitches pile every request of a moment onto two L2 channels -- made every shape 5-45 % SLOWER: tools/ubench/g16_rot.sh.)
    auto issue = [&](int buf) {
        unsigned char* base = smem_g16 + buf * STB + wave * (NI * 1024);
#pragma unroll
        for (int i = 0; i < NI; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void*)(base + i * 1024), 16, (int)offA[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NI; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void*)(base + OPB + i * 1024), 16, (int)offB[i], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NI; ++i) { offA[i] += slabA; offB[i] += slabB; }
    };
    // the same slab one DMA instruction at a time (piece 0 .. 2 NI - 1: A's, then B's): placed BETWEEN the MFMA groups of the slab that
    // is being multiplied -- issued in one burst in front of them, a wave's eight instructions hold its instruction stream for their
    // whole issue time (the address unit takes them at 100-200 cycles apiece under load) before its first fragment read
    auto issue_piece = [&](int buf, int pc) {
        unsigned char* base = smem_g16 + buf * STB + wave * (NI * 1024);
        if (pc < NI) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void*)(base + pc * 1024), 16, (int)offA[pc], 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (lds_void*)(base + OPB + (pc - NI) * 1024), 16, (int)offB[pc - NI], 0, 0, 0);
    };
    auto issue_advance = [&]() {
#pragma unroll
        for (int i = 0; i < NI; ++i) { offA[i] += slabA; offB[i] += slabB; }
    };

    // ---- fragment side: byte addresses inside an operand's stage image
    // k-contiguous: row * 128 + (((2 kk + half) ^ x) << 4), x = (row >> 1) & 7 = (l31 >> 1) & 7 for both 32-row tiles of the wave
    // m-contiguous: (kk * 16 + half * 8 [+ 4] + kq) * 256 + ((2 m) ^ (kq << 6)), kq = (lane & 15) >> 2, m = wave origin + i * 32 + (l31 & 16) + 4 (lane & 3)
    const int s16 = lane & 15, kq = s16 >> 2;
    const unsigned xa = TK == 64 ? (unsigned)((l31 >> 1) & 7) : (unsigned)((l31 >> 2) & 3);
    const unsigned fa0 = AKC ? (unsigned)(wm * 64 + l31) * (TK * 2u)
                             : (unsigned)(half * 8 + kq) * 256u + (((unsigned)(wm * 64 + (l31 & 16) + ((s16 & 3) << 2)) * 2u) ^ ((unsigned)kq << 6));
    const unsigned fb0 = BKC ? (unsigned)(wn * 64 + l31) * (TK * 2u)
                             : (unsigned)(half * 8 + kq) * 256u + (((unsigned)(wn * 64 + (l31 & 16) + ((s16 & 3) << 2)) * 2u) ^ ((unsigned)kq << 6));

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // bias gradients as a side output (weight-gradient layout: A m-contiguous): column sums of the A slabs of tile column 0
    const bool cs_on = !AKC && g.csum[0] != nullptr && tn == 0;
    float csv0 = 0.f, csv1 = 0.f;

    auto frag = [&](const unsigned char* img, bool kc, unsigned f0, int i, int kk) -> bf16x8 {
        if (kc) {
            const unsigned a = f0 + (unsigned)i * (32u * TK * 2u) + ((((unsigned)(2 * kk + half)) ^ xa) << 4);
            return *reinterpret_cast<const bf16x8*>(img + a);
        }
        typedef __attribute__((address_space(3))) v4s lds_v4s;
        // (i * 32 rows = 64 bytes: bit 6 of the in-row offset, which the XOR with kq << 6 may have set -> add, not or, after removing it)
        const unsigned inrow = ((f0 & 255u) ^ ((unsigned)kq << 6)) + (unsigned)i * 64u;
        const unsigned a = (f0 & ~255u) + (unsigned)kk * (16u * 256u) + (inrow ^ ((unsigned)kq << 6));
        const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(img + a));
        const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(img + a + 4 * 256));
        bf16x8 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
        return v;
    };

    // ring of NS stages: slabs s + 1 .. s + P are in flight while slab s is multiplied.  The DMA queue is drained by COUNT
    // (a wave's 2 NI instructions per slab retire in order), and the barrier is the raw instruction: __syncthreads() would
    // drain the whole queue in front of every barrier.
    int nis = 0;                                                // slabs issued so far
#pragma unroll
    for (int p = 0; p < P; ++p)
        if (s_begin + p < s_end) { issue(p); ++nis; }
    int buf = 0, ibuf = P % NS;
    for (int s = s_begin; s < s_end; ++s) {
        const int rem = nis - 1 - (s - s_begin);                // slabs that may stay in flight once slab s has landed
        if (rem >= 3) { if constexpr (P >= 4) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * NI * 3) : "memory"); }
        else if (rem == 2) { if constexpr (P >= 3) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * NI * 2) : "memory"); }
        else if (rem == 1) { if constexpr (P >= 2) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * NI * 1) : "memory"); }
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                           // slab s is in LDS for everybody; everybody is done with slab s - 1
        __builtin_amdgcn_sched_barrier(0);
        const bool more = s + P < s_end;                        // ... whose stage takes slab s + P
        const int jbuf = ibuf;
        if (more) ++nis;
        ibuf = ibuf + 1 == NS ? 0 : ibuf + 1;
        const unsigned char* Ai = smem_g16 + buf * STB;
        const unsigned char* Bi = Ai + OPB;
        if (cs_on) {
            // thread -> m pair (t & 63), k rows wave * TK / (4 KG) .. of the [TK k][128 m] image
            const unsigned mb = (unsigned)(threadIdx.x & 63) * 4u;
#pragma unroll
            for (int e = 0; e < TK / (4 * KG); ++e) {
                const unsigned k = (unsigned)(wave * (TK / (4 * KG)) + e);
                const unsigned w = *reinterpret_cast<const unsigned*>(Ai + k * 256u + (mb ^ ((k & 3u) << 6)));
                csv0 += __uint_as_float(w << 16);
                csv1 += __uint_as_float(w & 0xFFFF0000u);
            }
        }
        {
            // every fragment of the slab is requested before its first MFMA (a wave's LDS reads then run under its own MFMAs,
            // not only under the other waves'); the scheduler is told to keep that order
            constexpr int KK = TK / 16 / KG;                    // 16-deep blocks of the slab this wave multiplies
            const int kk0 = kg * KK;
            bf16x8 fa[KK][2], fb[KK][2];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[kk][i] = frag(Ai, AKC, fa0, i, kk0 + kk);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[kk][j] = frag(Bi, BKC, fb0, j, kk0 + kk);
            }
            __builtin_amdgcn_sched_barrier(0);
            constexpr int PPK = 2 * NI / KK;                    // DMA pieces per 16-deep block
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                if (more) {
#pragma unroll
                    for (int q = 0; q < PPK; ++q) issue_piece(jbuf, kk * PPK + q);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[kk][i], fb[kk][j], acc[i][j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (more) issue_advance();
        }
        buf = buf + 1 == NS ? 0 : buf + 1;
    }

    if constexpr (!AKC) {
        if (cs_on) {                                            // (workgroup-uniform)
            __syncthreads();
            float* red = reinterpret_cast<float*>(smem_g16);
            red[threadIdx.x * 2 + 0] = csv0;
            red[threadIdx.x * 2 + 1] = csv1;
            __syncthreads();
            const int r = threadIdx.x;
            if (r < TM && m0 + r < g.M) {
                float v = 0.f;
#pragma unroll
                for (int w = 0; w < 4 * KG; ++w) v += red[((r >> 1) + 64 * w) * 2 + (r & 1)];
#pragma unroll
                for (int o = 0; o < 3; ++o) if (g.csum[o]) unsafeAtomicAdd(g.csum[o] + m0 + r, v);
            }
        }
    }
    auto store_rows = [&](int i, const f32x16 (&ai)[2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = n0 + wn * 64 + j * 32 + l31;
            if (col >= g.N) continue;
            const float bv = (g.bias && ks == 0) ? g.bias[col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                if (row < g.M) {
                    float* dst = g.C + (size_t)row * g.ldc + col;
                    float v = ai[j][r] + bv;
                    if (g.splitk > 1) { unsafeAtomicAdd(dst, v); continue; }
                    if (g.accumulate) v += *dst;
                    if (g.relu) v = fmaxf(v, 0.f);
                    *dst = v;
                }
            }
        }
    };
    if constexpr (KG == 1) {
        store_rows(0, acc[0]);
        store_rows(1, acc[1]);
    } else {
        // group kg stores the wave's 32-row block i = kg: it hands the other block's partial sums to the other group through LDS
        // ([group][wave][j][r][lane] floats, 32 KB per group) and adds what the other group left for its own block
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __syncthreads();                                        // every wave is done with the stage images
        float* X = reinterpret_cast<float*>(smem_g16);
        float* mine = X + kg * 8192 + w4 * 2048 + lane;
        const float* theirs = X + (1 - kg) * 8192 + w4 * 2048 + lane;
        if (kg == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) mine[(j * 16 + r) * 64] = acc[1][j][r];
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) mine[(j * 16 + r) * 64] = acc[0][j][r];
        }
        __syncthreads();
        if (kg == 0) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[0][j][r] += theirs[(j * 16 + r) * 64];
            store_rows(0, acc[0]);
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[1][j][r] += theirs[(j * 16 + r) * 64];
            store_rows(1, acc[1]);
        }
    }
}

}  // namespace

// the DMA kernel as the route says it (xg_gemm_route.h: g16_ok admits the shapes, plan_g16 picks configuration and split)
int xgk_gemm_g16(hipStream_t st, const XgGemmRoute& r, const XgGemmIn& in, const XgGemmPtrs& p) {
    const GArgs g{p.A16, p.B16, p.C, p.bias, in.M, in.N, in.K, in.lda, in.ldb, in.ldc, in.relu ? 1 : 0, in.accumulate ? 1 : 0, r.splitk, r.gm,
                  {p.cs[0], p.cs[1], p.cs[2]}, 0};
    return xgk_with_layout(r, [&](auto akc, auto bkc) {
        constexpr bool A = decltype(akc)::value, B = decltype(bkc)::value;
        switch (r.cfg) {      // <wave groups, slab depth, ring stages>
        case 642: return xgk_launch_route<&gemm_g16_kernel<A, B, 64, 2, 1>>(st, r, r.lds, g);
        case 323: return xgk_launch_route<&gemm_g16_kernel<A, B, 32, 3, 1>>(st, r, r.lds, g);
        case 844: return xgk_launch_route<&gemm_g16_kernel<A, B, 64, 4, 2>>(st, r, r.lds, g);       // eight waves (two k groups), one workgroup per CU
#ifdef XG_DIAG
        case 322: return xgk_launch_route<&gemm_g16_kernel<A, B, 32, 2, 1>>(st, r, r.lds, g);
        case 843: return xgk_launch_route<&gemm_g16_kernel<A, B, 64, 3, 2>>(st, r, r.lds, g);
        case 643: return xgk_launch_route<&gemm_g16_kernel<A, B, 64, 3, 1>>(st, r, r.lds, g);
        case 324: return xgk_launch_route<&gemm_g16_kernel<A, B, 32, 4, 1>>(st, r, r.lds, g);
        case 325: return xgk_launch_route<&gemm_g16_kernel<A, B, 32, 5, 1>>(st, r, r.lds, g);
#endif
        default: return (int)XG_EINVAL;      // (a configuration this build has no kernel for)
        }
    });
}