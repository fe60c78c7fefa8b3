// Temporal soft attention for SEVERAL decoder rows of ONE video (include/xgate_control.h): the captioner rolled out under S POS
// templates per video keeps v2a(V) (B,K,A) and V (B,K,R) per VIDEO and only p (M,A), alpha (M,K) and af (M,R) per row, row
// b S + s.  The expressions are xg_attn.hip's:
//
//   e_k   = w_a . tanh(p + q_k)      alpha = softmax_k(e) over all K frames      af = sum_k alpha_k V_k
//
// cap_attn_group_kernel (the shapes of attn_fwd_fast): one 1024-thread workgroup serves up to G = XGCC_TEMPLATE_GROUP rows of one
// video.  A wave streams whole q rows (lane = 16 B) ONCE and applies each to the G p-vectors, which sit in LDS (at 1024 threads a
// wave has 128 VGPRs: G rows of p at A = 1536 would take 96 of them); the thread's V tile is requested first of all and weighted
// G times.  The step reads the video's 209 KB ceil(S / G) times instead of S times.  A row's sums run in one fixed order that
// knows neither the row's place in its group nor whether the group is full; rows a partial group lacks are neither computed nor
// stored.  cap_attn_rows_kernel covers every other shape with attn_fwd_kernel's loop, one workgroup per row.
#include "xg_common.h"
#include "xg_kernels.h"
#include "../../include/xgate_control.h"

namespace {

#ifdef XG_CONTROL_GROUP                 // measurement builds only (docs/CAPTION_CONTROL.md): another group size behind the same ABI
constexpr int CG = XG_CONTROL_GROUP;
#else
constexpr int CG = XGCC_TEMPLATE_GROUP;
#endif
constexpr int CT = 1024, CW = CT / 64;
constexpr int CRT = 512;

// NI: 256-column groups of A per lane; VMAX: V rows held per thread (K <= VMAX * nkp).  LDS: [G x A p-vectors, later two
// (nkp, R) context slabs] | w (A) | e (G x K4).
template <int NI, int VMAX, int G>
__global__ void __launch_bounds__(CT) __attribute__((amdgpu_waves_per_eu(4, 4)))
cap_attn_group_kernel(const float* __restrict__ p, const float* __restrict__ vproj, const float* __restrict__ V,
                      const float* __restrict__ w, float* __restrict__ alpha, float* __restrict__ af, int S, int K, int R, int A,
                      int front_floats) {
    extern __shared__ float sm[];
    XG_CHAIN_PRIO();
    float* ps = sm;                                   // (G, A); dead after the scores: the context slabs take its place
    float* wsh = sm + front_floats;                   // (A)
    float* se = wsh + A;                              // (G, K4)
    const int K4 = (K + 3) & ~3;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ng = (S + G - 1) / G;
    const int b = blockIdx.x / ng, g0 = (blockIdx.x - b * ng) * G;
    const int cnt = S - g0 < G ? S - g0 : G;          // rows of this group (a video's last group may be partial)
    const size_t row0 = (size_t)b * S + g0;
    const float* qb = vproj + (size_t)b * K * A;
    const float* Vb = V + (size_t)b * K * R;
    // context pass mapping: thread -> (4 consecutive r, k-part); its V loads go out first
    const int r4n = R >> 2, nkp = CT / r4n > 0 ? min(CT / r4n, K) : 1;
    const int myr = (tid % r4n) << 2, mykp = tid / r4n;
    float4 vreg[VMAX];
#pragma unroll
    for (int j = 0; j < VMAX; ++j) {
        const int k = mykp + j * nkp;
        vreg[j] = (mykp < nkp && k < K) ? *reinterpret_cast<const float4*>(Vb + (size_t)k * R + myr) : make_float4(0, 0, 0, 0);
    }
    // the wave's first q row is under way while the p-vectors are staged
    float4 q[NI];
    if (wave < K) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int a = lane * 4 + 256 * i;
            q[i] = a < A ? *reinterpret_cast<const float4*>(qb + (size_t)wave * A + a) : make_float4(0, 0, 0, 0);
        }
    }
    for (int a = tid * 4; a < A; a += CT * 4) {
        *reinterpret_cast<float4*>(wsh + a) = *reinterpret_cast<const float4*>(w + a);
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (g < cnt) *reinterpret_cast<float4*>(ps + (size_t)g * A + a) = *reinterpret_cast<const float4*>(p + (row0 + g) * A + a);
    }
    __syncthreads();
    // the wave's NEXT q row is requested before this one's tanh where the registers allow a second row (load before use, as
    // attn_fwd_fast issues everything up front), otherwise behind it, ahead of the reductions
    constexpr bool TWO = VMAX == 8 && NI <= 6;
    float4 qn[TWO ? NI : 1];
    for (int k = wave; k < K; k += CW) {
        const int kn = k + CW;
        if (TWO && kn < K) {
#pragma unroll
            for (int i = 0; i < (TWO ? NI : 1); ++i) {
                const int a = lane * 4 + 256 * i;
                qn[i] = a < A ? *reinterpret_cast<const float4*>(qb + (size_t)kn * A + a) : make_float4(0, 0, 0, 0);
            }
        }
        float acc[G];
#pragma unroll
        for (int g = 0; g < G; ++g) acc[g] = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int a = lane * 4 + 256 * i;
            if (a < A) {
                const float4 w4 = *reinterpret_cast<const float4*>(wsh + a);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (g < cnt) {
                        const float4 p4 = *reinterpret_cast<const float4*>(ps + (size_t)g * A + a);
                        acc[g] += w4.x * xg_tanh(p4.x + q[i].x) + w4.y * xg_tanh(p4.y + q[i].y) + w4.z * xg_tanh(p4.z + q[i].z) +
                                  w4.w * xg_tanh(p4.w + q[i].w);
                    }
                }
            }
        }
        if (!TWO && kn < K) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int a = lane * 4 + 256 * i;
                q[i] = a < A ? *reinterpret_cast<const float4*>(qb + (size_t)kn * A + a) : make_float4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g < cnt) {
                const float e = wave_sum(acc[g]);
                if (lane == 0) se[g * K4 + k] = e;
            }
        }
        if (TWO) {
#pragma unroll
            for (int i = 0; i < (TWO ? NI : 1); ++i) q[i] = qn[i];
        }
    }
    __syncthreads();                                  // the scores are final and every wave is done with ps
    float* slab[2] = {sm, sm + (size_t)nkp * R};
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g >= cnt) break;                          // (workgroup-uniform)
        const float* eg = se + g * K4;
        float* al_out = alpha ? alpha + (row0 + g) * K : nullptr;
        float4 s4 = make_float4(0, 0, 0, 0);
        if (K <= 64) {
            // softmax over the K scores, once per wave with lane k holding e_k
            const float e = lane < K ? eg[lane] : -INFINITY;
            const float mx = wave_max(e);
            const float ex = lane < K ? expf(e - mx) : 0.f;
            const float al_lane = ex * (1.0f / wave_sum(ex));
            if (al_out && wave == 0 && lane < K) al_out[lane] = al_lane;
#pragma unroll
            for (int j = 0; j < VMAX; ++j) {
                const int k = mykp + j * nkp;
                const float al = __shfl(al_lane, k < K ? k : 0);
                if (mykp < nkp && k < K) { s4.x += al * vreg[j].x; s4.y += al * vreg[j].y; s4.z += al * vreg[j].z; s4.w += al * vreg[j].w; }
            }
        } else {
            float mx = -INFINITY;
            for (int k = 0; k < K; ++k) mx = fmaxf(mx, eg[k]);
            float den = 0.f;
            for (int k = 0; k < K; ++k) den += expf(eg[k] - mx);
            const float inv = 1.0f / den;
#pragma unroll
            for (int j = 0; j < VMAX; ++j) {
                const int k = mykp + j * nkp;
                if (mykp < nkp && k < K) {
                    const float al = expf(eg[k] - mx) * inv;
                    s4.x += al * vreg[j].x; s4.y += al * vreg[j].y; s4.z += al * vreg[j].z; s4.w += al * vreg[j].w;
                }
            }
            if (al_out && tid < K) al_out[tid] = expf(eg[tid] - mx) * inv;
        }
        // two slabs in turn: row g + 1 writes the other one, and the barrier of row g + 1 lies between the readers of this
        // one and its next writers (row g + 2)
        float* part = slab[g & 1];
        if (mykp < nkp) *reinterpret_cast<float4*>(part + (size_t)mykp * R + myr) = s4;
        __syncthreads();
        for (int r = tid; r < R; r += CT) {
            float s = 0.f;
            for (int j = 0; j < nkp; ++j) s += part[(size_t)j * R + r];
            af[(row0 + g) * R + r] = s;
        }
    }
}

// every other shape: attn_fwd_kernel's loop, one workgroup per row, the video's operands at row / S
__global__ void __launch_bounds__(CRT) cap_attn_rows_kernel(const float* __restrict__ p, const float* __restrict__ vproj,
                                                             const float* __restrict__ V, const float* __restrict__ w,
                                                             float* __restrict__ alpha, float* __restrict__ af, int S, int K, int R,
                                                             int A) {
    extern __shared__ float sm[];          // e[K]
    const int row = blockIdx.x, b = row / S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = CRT / 64;
    const float* pb = p + (size_t)row * A;
    const float* qb = vproj + (size_t)b * K * A;
    for (int k = wave; k < K; k += nw) {
        const float* qk = qb + (size_t)k * A;
        float acc = 0.f;
        for (int a = lane; a < A; a += 64) acc += w[a] * xg_tanh(pb[a] + qk[a]);
        acc = wave_sum(acc);
        if (lane == 0) sm[k] = acc;
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmaxf(mx, sm[k]);
    float den = 0.f;
    for (int k = 0; k < K; ++k) den += expf(sm[k] - mx);
    const float inv = 1.0f / den;
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += CRT) {
        const float al = expf(sm[k] - mx) * inv;
        sm[k] = al;
        if (alpha) alpha[(size_t)row * K + k] = al;
    }
    __syncthreads();
    const float* Vb = V + (size_t)b * K * R;
    for (int r = threadIdx.x; r < R; r += CRT) {
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += sm[k] * Vb[(size_t)k * R + r];
        af[(size_t)row * R + r] = s;
    }
}

}  // namespace

// p (B*S,A), alpha (B*S,K) or null, af (B*S,R) per row; vproj (B,K,A), V (B,K,R) per video
int xgk_attn_fwd_group(hipStream_t st, const float* p, const float* vproj, const float* V, const float* w, float* alpha, float* af,
                       int B, int S, int K, int R, int A) {
    if (B < 1 || S < 1 || K < 1 || K > 8192 || (int64_t)B * S > (1 << 20)) return XG_EINVAL;
    const bool al16 = ((uintptr_t)p % 16 == 0) && ((uintptr_t)vproj % 16 == 0) && ((uintptr_t)V % 16 == 0) && ((uintptr_t)w % 16 == 0) &&
                      ((uintptr_t)af % 16 == 0);
    if (al16 && A % 4 == 0 && A <= 2048 && R % 4 == 0 && R <= 4 * CT && R >= 4) {
        const int r4n = R / 4;
        const int nkp = CT / r4n > 0 ? (CT / r4n < K ? CT / r4n : K) : 1;
        const int ni = (A + 255) / 256;
        // the register plan: 8 V rows per thread at any A <= 2048 (80 - 98 VGPRs); 16 of them only beside <= 4 column groups
        // (115 / 123 VGPRs; with 6 or 8 groups the 128 VGPRs of a 1024-thread workgroup's waves would spill)
        if (K <= 8 * nkp || (K <= 16 * nkp && ni <= 4)) {
            const size_t slabs = 2 * (size_t)nkp * R, pvec = (size_t)CG * A;
            const int front = (int)(slabs > pvec ? slabs : pvec);
            const size_t lds = ((size_t)front + A + (size_t)CG * ((K + 3) & ~3)) * sizeof(float);
            if (lds <= 60000) {
                const int grid = B * ((S + CG - 1) / CG);
#define XG_CATTN_LAUNCH(NI_, VM_) hipLaunchKernelGGL((cap_attn_group_kernel<NI_, VM_, CG>), dim3(grid), dim3(CT), lds, st, p, vproj, V, w, alpha, af, S, K, R, A, front)
                if (K <= 8 * nkp) {
                    if (ni <= 2) XG_CATTN_LAUNCH(2, 8); else if (ni <= 4) XG_CATTN_LAUNCH(4, 8);
                    else if (ni <= 6) XG_CATTN_LAUNCH(6, 8); else XG_CATTN_LAUNCH(8, 8);
                } else {
                    if (ni <= 2) XG_CATTN_LAUNCH(2, 16); else XG_CATTN_LAUNCH(4, 16);
                }
#undef XG_CATTN_LAUNCH
                XG_CHECK_LAUNCH();
                return XG_OK;
            }
        }
    }
    hipLaunchKernelGGL(cap_attn_rows_kernel, dim3(B * S), dim3(CRT), K * sizeof(float), st, p, vproj, V, w, alpha, af, S, K, R, A);
    XG_CHECK_LAUNCH();
    return XG_OK;
}
