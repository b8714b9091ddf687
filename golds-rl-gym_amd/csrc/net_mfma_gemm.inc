// Included inside namespace grl by net_flat_mfma.inc (FlatPolicyVNetwork), net_gated.hip (the Ticker gated trader),
// net_gauss.hip (the A3C Gaussian agent) and net_discrete.hip (the A3C savings-grid agent): the
// fp32 MFMA building blocks of the [feature][sample] LDS layout (row stride LS, 64 samples per group) and the fixed-order
// reduction of per-workgroup gradient slabs.  The includer defines LS and sigmoidf_.

typedef float f32x16f __attribute__((ext_vector_type(16)));

enum { FACT_NONE = 0, FACT_RELU = 1, FACT_TANH = 2, FACT_SIGMOID = 3 };

__device__ __forceinline__ float flat_act(float v, int act) {
    if (act == FACT_RELU) return fmaxf(v, 0.f);
    if (act == FACT_TANH) return tanhf(v);
    if (act == FACT_SIGMOID) return sigmoidf_(v);
    return v;
}

// out[o][s] = act(b[o] + sum_{i<K} W[i*ldw + o] * X[i][s]) for o < N, s < 64.  wsf != nullptr: also stored to the
// training workspace row (wsf + o*64)[s] (wsf = ws_row of the layer's first feature) for samples sbase + s < n.
// KC > 0: the reduction length is the compile-time constant KC (the GRU's D + 32 for the two geometries the reference uses):
// the k loop unrolls completely, so all operand loads of a tile are issued before the first MFMA instead of one
// load -> wait -> MFMA round trip per k pair (with a run-time K the unroll pragma is refused).
template <int KC = 0>
__device__ __forceinline__ void mm_fwd(const float *__restrict__ W, int ldw, const float *__restrict__ b, const float *X, int K, int N,
                                       float *out, int act, float *__restrict__ wsf, int n, int sbase, int wave, int lane) {
    const int ntiles = ((N + 31) >> 5) * 2, lr = lane & 31, kh = lane >> 5;
    for (int tile = wave; tile < ntiles; tile += 4) {
        const int o0 = (tile >> 1) * 32, s0 = (tile & 1) * 32;
        const int oa = o0 + lr, oc = oa < N ? oa : N - 1;
        f32x16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        if constexpr (KC > 0) {
            constexpr int NP = (KC + 1) / 2;
            float av[NP], bv[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const int i = 2 * j + kh, ic = i < KC ? i : KC - 1;
                av[j] = W[(long)ic * ldw + oc];
                bv[j] = X[ic * LS + s0 + lr];
                av[j] = (i < KC && oa < N) ? av[j] : 0.f;
                bv[j] = i < KC ? bv[j] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < NP; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
        } else {
#pragma unroll 16
            for (int k = 0; k < K; k += 2) {
                const int i = k + kh, ic = i < K ? i : K - 1;
                float av = W[(long)ic * ldw + oc];
                float bv = X[ic * LS + s0 + lr];
                av = (i < K && oa < N) ? av : 0.f;
                bv = i < K ? bv : 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
            }
        }
        const int s = s0 + lr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int o = o0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (o < N) {
                const float v = flat_act(acc[r] + b[o], act);
                out[o * LS + s] = v;
                if (wsf && sbase + s < n) wsf[o * 64 + s] = v;
            }
        }
    }
}

// dx[i][s] (=|+=) sum_{o<N} W[i*N + o] * dZ[o][s] for i < K
__device__ __forceinline__ void mm_dx(const float *__restrict__ W, int K, int N, const float *dZ, float *dx, bool accumulate, int wave, int lane) {
    const int ntiles = ((K + 31) >> 5) * 2, lr = lane & 31, kh = lane >> 5;
    for (int tile = wave; tile < ntiles; tile += 4) {
        const int i0 = (tile >> 1) * 32, s0 = (tile & 1) * 32;
        const int ia = i0 + lr, iac = ia < K ? ia : K - 1;
        f32x16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 16
        for (int k = 0; k < N; k += 2) {
            const int o = k + kh, oc = o < N ? o : N - 1;
            float av = W[(long)iac * N + oc];
            float bv = dZ[oc * LS + s0 + lr];
            av = (o < N && ia < K) ? av : 0.f;
            bv = o < N ? bv : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        const int s = s0 + lr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (i < K) dx[i * LS + s] = accumulate ? dx[i * LS + s] + acc[r] : acc[r];
        }
    }
}

// gW[i*N + o] += sum_s X[i][s] * dZ[o][s] (i < K, o < N);  gb[o] += sum_s dZ[o][s]
__device__ __forceinline__ void mm_wgrad(const float *X, const float *dZ, int K, int N, float *__restrict__ gW, float *__restrict__ gb,
                                         int wave, int lane, bool bias = true) {
    const int to = (N + 31) >> 5, ntiles = ((K + 31) >> 5) * to, lr = lane & 31, kh = lane >> 5;
    for (int tile = wave; tile < ntiles; tile += 4) {
        const int i0 = (tile / to) * 32, o0 = (tile % to) * 32;
        const int ia = i0 + lr, iac = ia < K ? ia : K - 1, oa = o0 + lr, oc = oa < N ? oa : N - 1;
        f32x16f acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
        for (int s = 0; s < 64; s += 2) {
            float av = X[iac * LS + s + kh];
            float bv = dZ[oc * LS + s + kh];
            av = ia < K ? av : 0.f;
            bv = oa < N ? bv : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
        }
        if (oa < N) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = i0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (i < K) gW[(long)i * N + oa] += acc[r];
            }
        }
    }
    for (int o = wave; bias && o < N; o += 4) {
        float v = dZ[o * LS + lane];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
        if (lane == 0) gb[o] += v;
    }
}

// dst[i] = sum over the workgroups' slabs, in a fixed order: 64 parameters per block, thread (q, p) adds the slabs q, q + 16, ..
// for parameter p (16 loads in flight per parameter instead of one thread walking all 256 slabs), the 16 partial sums then in order.
// static: every including translation unit has its own copy
static __global__ __launch_bounds__(1024) void flat_slab_reduce_kernel(const float *__restrict__ slab, int blocks, long n, float *__restrict__ dst) {
    __shared__ float part[16][64];
    const int p = threadIdx.x & 63, q = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 64 + p;
    float s = 0.f;
    if (i < n)
        for (int b = q; b < blocks; b += 16) s += slab[(long)b * n + i];
    part[q][p] = s;
    __syncthreads();
    if (q == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += part[k][p];
        dst[i] = t;
    }
}
